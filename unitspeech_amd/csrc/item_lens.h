// Per-item lengths of a batch (speaker.hip, vocoder.hip, hubert.hip, mel.hip, resample.hip): how a kernel learns them, how the host walks a
// batch in groups of as many items as one launch carries, and how a length out of range is refused.
//
// How a kernel learns an item's length.  A kernel that looks along time is a template over a policy LN with `ragged` and `lens(b, T)`, the valid
// steps of item b of the launch; rows are T apart either way.  SameT is the uniform call: the length is the row stride, and the instantiation
// is the kernel as it would be without the policy.  ItemLens<N> carries the lengths of up to N items as a kernel argument (one scalar load per
// workgroup, indexed by the block's item): item b is then a tensor of lens.n[b] steps stored with row stride T.  The item is a grid dimension
// of the launch, so no grid dimension caps the batch, and more than N items are a launch (or a pass of launches) per N: for_item_groups.
// A kernel without a uniform form (mel, resample, HuBERT / WavLM) is no template: it takes the carrier alone and reads lens.n[b].
// The handle-free calls (units, ctc, ctc_train, level, tts_train) take the lengths as a device array of int64 instead: item_len, row_live.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

namespace us {

struct SameT {                 // every item has T steps
  static constexpr bool ragged = false;
  __device__ __forceinline__ int operator()(int, int T) const { return T; }
};

template <int N> struct ItemLens {      // item b of the launch has n[b] steps; what the bounds are is the module's business
  static constexpr bool ragged = true;
  int n[N];
  __device__ __forceinline__ int operator()(int b, int) const { return n[b]; }
};
static_assert(sizeof(ItemLens<32>) == 32 * sizeof(int) && sizeof(ItemLens<64>) == 64 * sizeof(int), "N ints at offset 0: a kernel's argument segment");

// Valid steps of item b from a device array: lengths[b] clamped to [0, cap]; a null array is "every item has cap steps".
__device__ __forceinline__ int item_len(const long long* __restrict__ lengths, int b, int cap) {
  return lengths ? (int)min((long long)cap, max(0LL, lengths[b])) : cap;
}
// whether row (= b * Tmax + t) of a [B][Tmax] batch flattened to `rows` rows exists and lies inside its item
__device__ __forceinline__ bool row_live(const long long* __restrict__ lengths, int row, int rows, int Tmax) {
  if (row >= rows) return false;
  const int b = row / Tmax;
  return row - b * Tmax < item_len(lengths, b, Tmax);
}

// The batch in groups of N items: launch(b0, nb, lens, longest) for the nb <= N items from b0 on, lens.n[i] = len(b0 + i) and longest the
// largest of them.  The item is a grid dimension of size nb, so the entries past nb are never read; they hold 1.
template <int N, class Len, class Launch> void for_item_groups(int B, Len&& len, Launch&& launch) {
  for (int b0 = 0; b0 < B; b0 += N) {
    const int nb = std::min(N, B - b0);
    ItemLens<N> lens;
    int longest = 1;
    for (int i = 0; i < N; ++i) {
      lens.n[i] = i < nb ? (int)len(b0 + i) : 1;
      longest = std::max(longest, lens.n[i]);
    }
    launch(b0, nb, lens, longest);
  }
}

// "" when every lengths[b] lies in [lo, hi] (or lengths is null: the module's "every item has the full length"), else the head of the refusal
// for the first one that does not, `what: lengths[b] = v`; the caller finishes the sentence in the module's own words
inline std::string bad_length(const char* what, const int64_t* lengths, int B, long long lo, long long hi) {
  for (int b = 0; lengths && b < B; ++b)
    if (lengths[b] < lo || lengths[b] > hi)
      return std::string(what) + ": lengths[" + std::to_string(b) + "] = " + std::to_string((long long)lengths[b]);
  return std::string();
}

}  // namespace us
