// The recogniser's end of the library: a CTC head on encoder features, greedy CTC decoding and an edit distance, as handle-free calls
// that allocate nothing, need no scratch and only enqueue on the stream.
//
//   us_ctc_pack_head   weight [V][H], bias [V] -> the GEMM operand P[Hpad][Vpad] (h-major, zero padded) followed by bias[Vpad].
//   us_ctc_logits      logits[b][t][v] = hidden[b][t] . weight[v] + bias[v] on the fp32 matrix cores (the tile loop of dense_tile.h,
//                      shared with the unit scorer).  The rows are the MFMA's A operand, so a row's index lands on the accumulator registers and the vocabulary on the lanes: the stores are coalesced along V.  A row's H products are
//                      added in one fixed order (two interleaved chains over ascending h, one addition, then the bias) wherever the row
//                      lies, so an item has the same bits alone and in a ragged batch.  A second kernel, one wave per row, reads the
//                      written logits: ids = their argmax (the lower index on ties), log_probs = (x - max) - logf(sum expf(x - max)).
//                      Rows at or beyond lengths[b] get logits 0, log_probs 0 and ids -1.
//   us_ctc_collapse    greedy CTC decoding per item: a frame is kept when it differs from the frame before it and is not the blank.
//                      One workgroup per item, an LDS scan over chunk counts (block_scan256, as the units' run-length encoding), any Tmax.
//   us_edit_distance   Levenshtein distance with unit costs, one workgroup per pair, anti-diagonal sweep over three rolling diagonals
//                      of int32 in LDS (indexed by the hypothesis position), one barrier per diagonal.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/unitspeech_hip.h"
#include "ctc_limits.h"
#include "dense_tile.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kMaxTokens = 4096;

__global__ __launch_bounds__(256) void ctc_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, float* __restrict__ p, int V,
                                                       int H, int Vpad, int Hpad) {
  const size_t n = (size_t)Hpad * Vpad;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n + Vpad; i += (size_t)gridDim.x * 256) {
    if (i < n) {
      const int v = (int)(i % Vpad), h = (int)(i / Vpad);
      p[i] = (v < V && h < H) ? w[(size_t)v * H + h] : 0.f;
    } else {
      const int v = (int)(i - n);
      p[i] = (bias && v < V) ? bias[v] : 0.f;
    }
  }
}

// Workgroup: 64 rows x 64 vocabulary entries, four waves of 32 x 32.  Both operands go through LDS k-major (two stages); the rows are
// transposed on the way in.
__global__ __launch_bounds__(256) void ctc_logits_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ bias,
                                                         const long long* __restrict__ lengths, float* __restrict__ out, int rows, int Tmax,
                                                         int V, int H, int Hpad, int Vpad) {
  __shared__ float Ws[2][kDtBK][kDtTile];
  __shared__ float Xs[2][kDtBK][kDtLdT];
  const int tid = threadIdx.x;
  DENSE_LANE(tid);
  DENSE_STAGE_K(tid);                                    // weight slice: 16 k x 64 entries, one float4 per thread
  DENSE_STAGE_T(tid);                                    // feature slice: 64 rows x 16 k, one float4 per thread
  const int vh = wave & 1, rh = wave >> 1;
  const int r0 = blockIdx.x * kDtTile, c0 = blockIdx.y * kDtTile;
  const bool xlive = row_live(lengths, r0 + tr, rows, Tmax);   // a padding row is never read: what lies there may be anything
  const float* __restrict__ xrow = X + (size_t)(xlive ? r0 + tr : 0) * H;
  float4 wreg, xreg;
  auto load = [&](int k0) {
    wreg = *reinterpret_cast<const float4*>(P + (size_t)(k0 + sk) * Vpad + c0 + sc);
    xreg = (xlive && k0 + tk < H) ? *reinterpret_cast<const float4*>(xrow + k0 + tk) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store = [&](int buf) {
    *reinterpret_cast<float4*>(&Ws[buf][sk][sc]) = wreg;
    Xs[buf][tk + 0][tr] = xreg.x;
    Xs[buf][tk + 1][tr] = xreg.y;
    Xs[buf][tk + 2][tr] = xreg.z;
    Xs[buf][tk + 3][tr] = xreg.w;
  };
  f32x16 acc[2];
  dense_tile_mainloop(Xs, Ws, rh, vh, Hpad / kDtBK, acc, load, store);
  // the MFMA row is the row of X, the MFMA column the vocabulary entry: 32 lanes store 32 neighbouring floats
  const int v = c0 + DENSE_AT(vh);
  if (v >= V) return;
  const float bv = bias[v];
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = r0 + DENSE_ROW(rh, r);
    if (row >= rows) continue;
    const int b = row / Tmax;
    const bool live = row - b * Tmax < item_len(lengths, b, Tmax);
    out[(size_t)row * V + v] = live ? (acc[0][r] + acc[1][r]) + bv : 0.f;
  }
}

// One wave per row over the written logits: lane l holds entries l, l + 64, ...; fixed butterflies join the lanes.
__global__ __launch_bounds__(256) void ctc_rows_kernel(const float* __restrict__ logits, const long long* __restrict__ lengths,
                                                       float* __restrict__ log_probs, long long* __restrict__ ids, int rows, int Tmax, int V) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = row / Tmax;
  const float* __restrict__ x = logits + (size_t)row * V;
  if (row - b * Tmax >= item_len(lengths, b, Tmax)) {
    if (log_probs)
      for (int v = lane; v < V; v += 64) log_probs[(size_t)row * V + v] = 0.f;
    if (ids && lane == 0) ids[row] = -1;
    return;
  }
  float xv[kMaxV / 64];
  float best = -INFINITY;
  int bi = 0x7fffffff;
#pragma unroll
  for (int j = 0; j < kMaxV / 64; ++j) {
    const int v = lane + 64 * j;
    xv[j] = v < V ? x[v] : -INFINITY;
    if (v < V && (xv[j] > best || bi == 0x7fffffff)) {   // ascending v: a later equal value does not replace an earlier one
      best = xv[j];
      bi = v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                     // "higher value, then lower index": associative and commutative
    const float ob = __shfl_xor(best, o);
    const int oi = __shfl_xor(bi, o);
    if (ob > best || (ob == best && oi < bi)) {
      best = ob;
      bi = oi;
    }
  }
  if (ids && lane == 0) ids[row] = bi;
  if (!log_probs) return;
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxV / 64; ++j)
    if (lane + 64 * j < V) s += expf(xv[j] - best);
  s = wave_sum(s);
  const float ls = logf(s);                              // (x - max) - log(sum): no rounding at the size of the maximum itself
#pragma unroll
  for (int j = 0; j < kMaxV / 64; ++j)
    if (lane + 64 * j < V) log_probs[(size_t)row * V + lane + 64 * j] = (xv[j] - best) - ls;
}

// One workgroup of 256 threads per item: thread i owns the contiguous chunk i of ids[0, len), counts the frames it keeps, an LDS scan
// places them.
__global__ __launch_bounds__(256) void ctc_collapse_kernel(const long long* __restrict__ ids, const long long* __restrict__ lengths,
                                                           long long blank, long long* __restrict__ tokens, long long* __restrict__ first_frame,
                                                           long long* __restrict__ n_out, int Tmax) {
  __shared__ int scan[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const size_t o = (size_t)b * Tmax;
  const long long* __restrict__ u = ids + o;
  const int len = item_len(lengths, b, Tmax);
  const int chunk = (len + 255) / 256;
  const int t0 = min(len, tid * chunk), t1 = min(len, t0 + chunk);
  int cnt = 0;
  for (int t = t0; t < t1; ++t) cnt += (u[t] != blank && (t == 0 || u[t] != u[t - 1])) ? 1 : 0;
  block_scan256(scan, cnt);
  const int n = scan[255];
  int pos = scan[tid] - cnt;
  for (int t = t0; t < t1; ++t) {
    if (u[t] != blank && (t == 0 || u[t] != u[t - 1])) {
      tokens[o + pos] = u[t];
      if (first_frame) first_frame[o + pos] = t;
      ++pos;
    }
  }
  for (int p = n + tid; p < Tmax; p += 256) {            // disjoint from the places written above
    tokens[o + p] = 0;
    if (first_frame) first_frame[o + p] = 0;
  }
  if (tid == 0) n_out[b] = n;
}

// D[i][j]: the distance of hyp[0, i) and ref[0, j).  Diagonal d holds the cells with i + j = d at index i; a cell reads index i - 1 and
// i of diagonal d - 1 and index i - 1 of diagonal d - 2.  cap = Lh + 1 ints per diagonal.
__global__ __launch_bounds__(256) void edit_distance_kernel(const long long* __restrict__ hyp, const long long* __restrict__ n_hyp, int Lh,
                                                            const long long* __restrict__ ref, const long long* __restrict__ n_ref, int Lr,
                                                            long long* __restrict__ dist) {
  extern __shared__ int diag[];
  const int p = blockIdx.x, tid = threadIdx.x;
  const int cap = Lh + 1;
  const int n = item_len(n_hyp, p, Lh), m = item_len(n_ref, p, Lr);
  const long long* __restrict__ a = hyp + (size_t)p * Lh;
  const long long* __restrict__ c = ref + (size_t)p * Lr;
  int* cur = diag;
  int* p1 = diag + cap;
  int* p2 = diag + 2 * cap;
  for (int d = 0; d <= n + m; ++d) {
    const int lo = max(0, d - m), hi = min(n, d);
    for (int i = lo + tid; i <= hi; i += 256) {
      const int j = d - i;
      int v;
      if (i == 0 || j == 0) {
        v = d;
      } else {
        const int sub = p2[i - 1] + (a[i - 1] != c[j - 1] ? 1 : 0);
        v = min(sub, min(p1[i - 1], p1[i]) + 1);
      }
      cur[i] = v;
    }
    __syncthreads();                                     // diagonal d is complete; the buffer of d - 2 is free to take d + 1
    int* t = p2;
    p2 = p1;
    p1 = cur;
    cur = t;
  }
  if (tid == 0) dist[p] = p1[n];
}

}  // namespace
}  // namespace us

using namespace us;

extern "C" {

size_t us_ctc_packed_bytes(int V, int H) {
  if (head_error(V, H)) return 0;
  return ((size_t)round_up(H, kDtBK) * round_up(V, kDtTile) + round_up(V, kDtTile)) * sizeof(float);
}

int us_ctc_pack_head(const float* weight, const float* bias, int V, int H, void* packed, size_t packed_bytes, us_stream stream) {
  if (const char* m = head_error(V, H)) {
    char buf[128];
    snprintf(buf, sizeof buf, "us_ctc_pack_head: %s (V = %d, H = %d)", m, V, H);
    return bad_arg(buf);
  }
  if (!weight || !packed || packed_bytes < us_ctc_packed_bytes(V, H)) return bad_arg("us_ctc_pack_head: bad argument");
  hipLaunchKernelGGL(ctc_pack_kernel, dim3(512), dim3(256), 0, static_cast<hipStream_t>(stream), weight, bias, static_cast<float*>(packed), V, H,
                     round_up(V, kDtTile), round_up(H, kDtBK));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_ctc_pack_head", e);
}

int us_ctc_logits(const float* hidden, const int64_t* lengths, const void* packed, int B, int Tmax, int V, int H, float* logits,
                  float* log_probs, int64_t* ids, us_stream stream) {
  if (const char* m = head_error(V, H)) {
    char buf[128];
    snprintf(buf, sizeof buf, "us_ctc_logits: %s (V = %d, H = %d)", m, V, H);
    return bad_arg(buf);
  }
  if (!hidden || !packed || !logits || !rows_ok(B, Tmax)) return bad_arg("us_ctc_logits: bad argument");
  const int rows = B * Tmax, Vpad = round_up(V, kDtTile), Hpad = round_up(H, kDtBK);
  const float* P = static_cast<const float*>(packed);
  const long long* lens = reinterpret_cast<const long long*>(lengths);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(ctc_logits_kernel, dim3((rows + kDtTile - 1) / kDtTile, Vpad / kDtTile), dim3(256), 0, s, hidden, P, P + (size_t)Hpad * Vpad, lens,
                     logits, rows, Tmax, V, H, Hpad, Vpad);
  if (log_probs || ids)
    hipLaunchKernelGGL(ctc_rows_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, lens, log_probs, reinterpret_cast<long long*>(ids), rows,
                       Tmax, V);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_ctc_logits", e);
}

int us_ctc_collapse(const int64_t* ids, const int64_t* lengths, int B, int Tmax, int64_t blank, int64_t* tokens, int64_t* first_frame,
                    int64_t* n, us_stream stream) {
  if (!ids || !tokens || !n || !rows_ok(B, Tmax) || ids == tokens || ids == first_frame) return bad_arg("us_ctc_collapse: bad argument");
  hipLaunchKernelGGL(ctc_collapse_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(ids),
                     reinterpret_cast<const long long*>(lengths), (long long)blank, reinterpret_cast<long long*>(tokens),
                     reinterpret_cast<long long*>(first_frame), reinterpret_cast<long long*>(n), Tmax);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_ctc_collapse", e);
}

int us_edit_distance(const int64_t* hyp, const int64_t* n_hyp, int Lh, const int64_t* ref, const int64_t* n_ref, int Lr, int P, int64_t* dist,
                     us_stream stream) {
  if (Lh < 0 || Lr < 0 || Lh > kMaxTokens || Lr > kMaxTokens) {
    char buf[160];
    snprintf(buf, sizeof buf, "us_edit_distance: a sequence holds at most %d tokens (Lh = %d, Lr = %d)", kMaxTokens, Lh, Lr);
    return bad_arg(buf);
  }
  if (P < 0 || P > (1 << 24)) return bad_arg("us_edit_distance: P must be in [0, 2^24]");
  if (P == 0) return US_OK;
  if (!n_hyp || !n_ref || !dist || (Lh > 0 && !hyp) || (Lr > 0 && !ref)) return bad_arg("us_edit_distance: bad argument");
  const size_t lds = 3 * (size_t)(Lh + 1) * sizeof(int);       // at most 49164 bytes: within the 64 KB a kernel gets unasked
  hipLaunchKernelGGL(edit_distance_kernel, dim3(P), dim3(256), lds, static_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(hyp),
                     reinterpret_cast<const long long*>(n_hyp), Lh, reinterpret_cast<const long long*>(ref),
                     reinterpret_cast<const long long*>(n_ref), Lr, reinterpret_cast<long long*>(dist));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_edit_distance", e);
}

}  // extern "C"
