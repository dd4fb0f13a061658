// Mel-spectrogram front end (the reference's unitspeech/vocoder/meldataset.py:51-74 `mel_spectrogram(..., center=False)` and the
// normalisation of finetune.py:104): waveform [B][Tmax] with per-item lengths -> log-mel [B][num_mels][Tmax / hop], fp32 storage and
// accumulation, exact fp32 products.
//
// With n_fft = taps * hop the STFT is a convolution.  Fold the reflect-padded waveform into a planar tensor X[ci][q] = y_pad[q * hop + ci]
// (ci < hop); frame q of the windowed DFT is then sum_{j < taps, ci < hop} P[j * hop + ci][co] * X[ci][q + j], a Conv1d(hop -> 2 * bins,
// k = taps) in the form conv1d_planar.h's main loop multiplies on v_mfma_f32_32x32x2_f32.  The mel projection is a k = 1 convolution of
// the same kind.  The kernels:
//  - mel_frame_kernel: reflect padding by p = (n_fft - hop) / 2 at the item's own length and the de-interleave into X [B][hop][Q],
//    Q = Tmax / hop + taps - 1, zero past the item's padded end; transposed through LDS so that reads and writes are both coalesced.
//  - mel_dft_kernel: the windowed DFT.  Output channel 2 f is Re, 2 f + 1 is Im of bin f, so registers (r, r + 1) of an accumulator
//    lane are the two halves of one bin and the epilogue writes sqrt(re^2 + im^2 + 1e-9) as [B][live][F].  The operand is built once
//    per window by mel_dft_pack_kernel: the angle index (f n) mod n_fft reduced in integers, cospi / sinpi and the product with the
//    (centred) window in fp64, one rounding to fp32.
//  - mel_proj_kernel: mel_basis (k = 1, Cin = live bins) with log(max(x, 1e-5)), the optional normalisation and the padding of the
//    frames past an item's own count in its epilogue.  "Live" bins: those up to the highest one with a non-zero column in mel_basis (372
//    of 513 for fmax = 8000 at 22050 Hz); neither GEMM touches the others.
//  - mel_minmax_kernel: per-band minimum and maximum over the valid frames of a batch.
// A frame's value depends on its own item's samples only and every sum has a fixed order: an item alone or in a batch, and repeated
// calls, give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/unitspeech_hip.h"
#include "conv1d_planar.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

// Frames per workgroup: planar_conv_mainloop<2, 1>, a wave's tile is 32 channels x 64 frames with ONE accumulator chain per sub-tile (the
// two sub-tiles keep the matrix core busy).  A second chain would take every other pair of samples of a frame: for a smooth waveform each
// half is then a large sum of alternating sign at the upper bins, and the two cancel only in the final addition.  Taken in sample order
// the partial sums of window x twiddle x signal stay small (emulated on the CPU in fp32: 0.4 of the reference's own fp32 error on
// integrated noise with one chain, 9 times it with two interleaved ones).
constexpr int kMelBN = 128;
constexpr int kMelItems = 64;       // batch items per launch (item_lens.h): samples (mel_frame_kernel) or frames (mel_proj_kernel, mel_minmax_kernel)
constexpr int kMelMaxFft = 4096;
constexpr int kMelMaxMels = 1024;

// X[b][ci][q] = y_pad[q * hop + ci]; y_pad[i] = wav[reflect(i - p)] for i < len + 2 p, 0 beyond.  len > p, so a reflected index
// stays inside [0, len): nothing at or past wav[b][len] is read.  One workgroup: 64 ci x 64 q.
__global__ __launch_bounds__(256) void mel_frame_kernel(const float* __restrict__ wav, float* __restrict__ x, ItemLens<kMelItems> lens, int Tmax,
                                                        int hop, int p, int Q) {
  planar_fold_tile(wav, x, lens, Tmax, hop, Q, [=](const float* __restrict__ w, long long len, int q, int ci) {
    float v = 0.f;
    const long long i = (long long)q * hop + ci;
    if (q < Q && ci < hop && i < len + 2 * p) {
      long long s = i - p;
      s = s < 0 ? -s : (s >= len ? 2 * (len - 1) - s : s);
      v = w[s];
    }
    return v;
  });
}

// P[n][2 f + part] = round_fp32(w[n] * (cos, -sin)(2 pi (f n mod n_fft) / n_fft)) for n < n_fft, f < live, zero in the padding; w is the
// window centred in n_fft samples (torch.stft's treatment of win_length < n_fft)
__global__ void mel_dft_pack_kernel(const float* __restrict__ window, float* __restrict__ p, int n_fft, int win, int live, int Kpad, int ldw) {
  const int total = Kpad * ldw, lo = (n_fft - win) / 2;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int co = i % ldw, n = i / ldw, f = co >> 1;
    float v = 0.f;
    if (n < n_fft && f < live && n >= lo && n < lo + win) {
      const int m = (int)(((long long)f * n) % n_fft);
      const double a = 2.0 * (double)m / (double)n_fft;
      const double c = (co & 1) ? -sinpi(a) : cospi(a);
      v = (float)(c * (double)window[n - lo]);
    }
    p[i] = v;
  }
}

// P[ci][co] = mel_basis[co][ci] for ci < live, zero in the padding
__global__ void mel_basis_pack_kernel(const float* __restrict__ basis, float* __restrict__ p, int num_mels, int bins, int live, int Kpad, int ldw) {
  const int total = Kpad * ldw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int co = i % ldw, ci = i / ldw;
    p[i] = (co < num_mels && ci < live) ? basis[(size_t)co * bins + ci] : 0.f;
  }
}

// *live = 1 + the highest bin whose column of mel_basis has a non-zero entry (0 for an all-zero matrix); one workgroup
__global__ __launch_bounds__(256) void mel_live_kernel(const float* __restrict__ basis, int* __restrict__ live, int num_mels, int bins) {
  __shared__ int best[256];
  int m = 0;
  for (int i = threadIdx.x; i < num_mels * bins; i += 256)
    if (basis[i] != 0.f) m = max(m, i % bins + 1);
  best[threadIdx.x] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) best[threadIdx.x] = max(best[threadIdx.x], best[threadIdx.x + o]);
    __syncthreads();
  }
  if (threadIdx.x == 0) *live = best[0];
}

struct MelDftArgs {
  const float* x;             // [B][hop][Q]
  const float* w;             // [Kpad][ldw]
  float* mag;                 // [B][live][F]
  int hop, Q, F, live, Kdim, Kpad, ldw;
};

__global__ __launch_bounds__(256) void mel_dft_kernel(MelDftArgs a) {
  PLANAR_LANE(threadIdx.x);
  const int b = blockIdx.z;
  const int m0 = blockIdx.y * kPcBM, n0 = blockIdx.x * kMelBN;
  f32x16 acc[2][1];
  planar_conv_mainloop<2, 1>({a.x + (size_t)b * a.hop * a.Q, a.w, a.hop, a.Q, 1, 0, a.Kdim, a.Kpad, a.ldw, m0, n0}, acc);
  float* __restrict__ mag = a.mag + (size_t)b * a.live * a.F;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int t = n0 + PLANAR_COL(2, n);
    if (t >= a.F) continue;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      const int f = PLANAR_CHANNEL(m0, r) >> 1;                            // rows (r, r + 1) are (2 f, 2 f + 1)
      if (f >= a.live) continue;
      const float re = acc[n][0][r], im = acc[n][0][r + 1];
      mag[(size_t)f * a.F + t] = sqrtf(re * re + im * im + 1e-9f);    // meldataset.py:69
    }
  }
}

struct MelProjArgs {
  const float* mag;           // [B][live][F]
  const float* w;             // [Kpad][ldw]
  const float* mel_min;       // n_norm values (1: one for all bands), or null
  const float* mel_max;
  float* out;                 // [B][num_mels][F]
  ItemLens<kMelItems> frames;
  float pad_value;
  int n_norm, num_mels, F, live, Kpad, ldw;
};

__global__ __launch_bounds__(256) void mel_proj_kernel(MelProjArgs a) {
  PLANAR_LANE(threadIdx.x);
  const int b = blockIdx.z;
  const int m0 = blockIdx.y * kPcBM, n0 = blockIdx.x * kMelBN;
  f32x16 acc[2][1];
  planar_conv_mainloop<2, 1>({a.mag + (size_t)b * a.live * a.F, a.w, a.live, a.F, 1, 0, a.live, a.Kpad, a.ldw, m0, n0}, acc);
  float* __restrict__ out = a.out + (size_t)b * a.num_mels * a.F;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int t = n0 + PLANAR_COL(2, n);
    if (t >= a.F) continue;
    const bool valid = t < a.frames.n[b];
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = PLANAR_CHANNEL(m0, r);
      if (co >= a.num_mels) continue;
      float v = a.pad_value;
      if (valid) {
        v = logf(fmaxf(acc[n][0][r], 1e-5f));                         // meldataset.py:30, clip_val 1e-5
        if (a.n_norm > 0) {
          // finetune.py:104, (m - mel_min) / (mel_max - mel_min) * 2 - 1: every operation rounded on its own, like the tensor ops
          const int j = a.n_norm == 1 ? 0 : co;
          const float mn = a.mel_min[j], span = sub_rn(a.mel_max[j], mn);
          v = sub_rn(mul_rn(__fdiv_rn(sub_rn(v, mn), span), 2.f), 1.f);
        }
      }
      out[(size_t)co * a.F + t] = v;
    }
  }
}

// out[0][m] = min, out[1][m] = max of mel[b][m][t] over t < frames[b] of the launch's items; `merge` folds in what out already holds
// (the next kMelItems items of a larger batch).  One workgroup per band.  +inf / -inf when no item has a frame.
__global__ __launch_bounds__(256) void mel_minmax_kernel(const float* __restrict__ mel, ItemLens<kMelItems> frames, int B, int num_mels,
                                                         int F, float* __restrict__ out, int merge) {
  __shared__ float smin[4], smax[4];
  const int m = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  float lo = INFINITY, hi = -INFINITY;
  for (int b = 0; b < B; ++b) {
    const float* __restrict__ row = mel + ((size_t)b * num_mels + m) * F;
    const int n = min(frames.n[b], F);
    for (int t = threadIdx.x; t < n; t += 256) {
      lo = fminf(lo, row[t]);
      hi = fmaxf(hi, row[t]);
    }
  }
  lo = -wave_max(-lo);
  hi = wave_max(hi);
  if (lane == 0) { smin[wave] = lo; smax[wave] = hi; }
  __syncthreads();
  if (threadIdx.x == 0) {
    lo = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    hi = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    if (merge) {
      lo = fminf(lo, out[m]);
      hi = fmaxf(hi, out[num_mels + m]);
    }
    out[m] = lo;
    out[num_mels + m] = hi;
  }
}

}  // namespace
}  // namespace us

struct us_mel : us::WeightTable {
  us_mel_config cfg{};
  int bins = 0, taps = 0, pad = 0;
  int live = 0;                        // bins the two GEMMs compute; known once mel_basis is loaded
  int dft_Kpad = 0, dft_ldw = 0, proj_Kpad = 0, proj_ldw = 0;
  float* dft = nullptr;                // [round_up(n_fft, kPcBK)][round_up(2 bins, kPcBM)], of which [dft_Kpad][dft_ldw] is in use
  float* proj = nullptr;               // [round_up(bins, kPcBK)][round_up(num_mels, kPcBM)]
  int* live_dev = nullptr;
};

namespace us {
namespace {

hipError_t mel_alloc(us_mel* h) {
  hipError_t e = hipSuccess;
  auto alloc = [&](auto** p, size_t bytes) {
    if (e == hipSuccess && !*p) e = hipMalloc(p, bytes);
  };
  for (auto& kv : h->w) alloc(&kv.second.dev, kv.second.numel() * sizeof(float));
  alloc(&h->dft, (size_t)round_up(h->cfg.n_fft, kPcBK) * round_up(2 * h->bins, kPcBM) * sizeof(float));
  alloc(&h->proj, (size_t)round_up(h->bins, kPcBK) * round_up(h->cfg.num_mels, kPcBM) * sizeof(float));
  alloc(&h->live_dev, sizeof(int));
  return e;
}

// the two packed operands from the loaded tensors (both depend on `live`)
void mel_pack(us_mel* h, hipStream_t s) {
  const auto& c = h->cfg;
  h->dft_Kpad = round_up(c.n_fft, kPcBK);
  h->dft_ldw = round_up(2 * h->live, kPcBM);
  h->proj_Kpad = round_up(h->live, kPcBK);
  h->proj_ldw = round_up(c.num_mels, kPcBM);
  auto grid = [](int n) { return dim3((unsigned)std::min((n + 255) / 256, 4096)); };
  hipLaunchKernelGGL(mel_dft_pack_kernel, grid(h->dft_Kpad * h->dft_ldw), dim3(256), 0, s, h->w.at("window").dev, h->dft, c.n_fft, c.win, h->live,
                     h->dft_Kpad, h->dft_ldw);
  hipLaunchKernelGGL(mel_basis_pack_kernel, grid(h->proj_Kpad * h->proj_ldw), dim3(256), 0, s, h->w.at("mel_basis").dev, h->proj, c.num_mels,
                     h->bins, h->live, h->proj_Kpad, h->proj_ldw);
}

// item lengths of a call: every one in (lo, hi]; NULL = all hi
int mel_check_lengths(us_mel* h, const char* what, const int64_t* lengths, int B, long long lo, long long hi) {
  const std::string bad = bad_length(what, lengths, B, lo + 1, hi);
  return bad.empty() ? US_OK : h->fail(US_EINVAL, bad + " is outside (" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
}

}  // namespace
}  // namespace us

extern "C" {

using namespace us;

int us_mel_create(us_mel_handle* out, const us_mel_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_mel_create: null argument");
  const auto& c = *cfg;
  if (c.n_fft <= 0 || c.hop <= 0 || c.win <= 0 || c.num_mels <= 0 || c.num_mels > kMelMaxMels)
    return WeightTable::fail(nullptr, US_EINVAL, "us_mel_create: n_fft, hop, win and num_mels must be positive (num_mels at most 1024)");
  if (c.n_fft > kMelMaxFft) return WeightTable::fail(nullptr, US_EINVAL, "us_mel_create: n_fft above 4096 is not built");
  if (c.n_fft % c.hop != 0)
    return WeightTable::fail(nullptr, US_EINVAL, "us_mel_create: hop must divide n_fft (the STFT runs as a convolution with n_fft / hop taps)");
  if ((c.n_fft - c.hop) % 2 != 0) return WeightTable::fail(nullptr, US_EINVAL, "us_mel_create: n_fft - hop must be even (the reflect padding is half of it)");
  if (c.win > c.n_fft) return WeightTable::fail(nullptr, US_EINVAL, "us_mel_create: win must not exceed n_fft");
  auto* h = new us_mel();
  h->cfg = c;
  h->bins = c.n_fft / 2 + 1;
  h->taps = c.n_fft / c.hop;
  h->pad = (c.n_fft - c.hop) / 2;
  (void)hipGetDevice(&h->device);
  h->add("mel_basis", {c.num_mels, h->bins});
  h->add("window", {c.win});
  *out = h;
  return US_OK;
}

int us_mel_destroy(us_mel_handle h) {
  if (!h) return US_OK;
  h->free_weights();
  if (h->dft) (void)hipFree(h->dft);
  if (h->proj) (void)hipFree(h->proj);
  if (h->live_dev) (void)hipFree(h->live_dev);
  delete h;
  return US_OK;
}

int us_mel_num_weights(us_mel_handle h) { return h ? h->num() : 0; }
const char* us_mel_weight_key(us_mel_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_mel_last_error(us_mel_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_mel_load_weight(us_mel_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  Weight* w;
  int rc = WeightTable::find(h, "us_mel_load_weight", key, data, shape, ndim, &w);
  if (rc != US_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (!h->dft && (e = mel_alloc(h)) != hipSuccess) return h->hip("us_mel_load_weight: hipMalloc", e);
  if ((rc = h->copy(*w, data, s)) != US_OK) return rc;
  w->loaded = true;
  if (std::string(key) == "mel_basis") {
    // the number of live bins sizes both GEMMs, so the host has to know it: the one synchronisation, at load time
    int live = 0;
    hipLaunchKernelGGL(mel_live_kernel, dim3(1), dim3(256), 0, s, w->dev, h->live_dev, h->cfg.num_mels, h->bins);
    if ((e = hipMemcpyAsync(&live, h->live_dev, sizeof(int), hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (e = hipStreamSynchronize(s)) != hipSuccess)
      return h->hip("us_mel_load_weight: reading the live bin count", e);
    h->live = std::max(live, 1);
  }
  if (h->w.at("mel_basis").loaded && h->w.at("window").loaded) mel_pack(h, s);
  e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_mel_load_weight", e);
}

int us_mel_frames(us_mel_handle h, int T) { return (h && T > 0) ? T / h->cfg.hop : 0; }

// X [B][hop][Q] and the magnitudes [B][bins][F] (sized for every bin: the answer does not depend on what has been loaded)
size_t us_mel_workspace_bytes(us_mel_handle h, int B, int Tmax) {
  if (!h || B <= 0 || Tmax <= 0) return 0;
  const size_t F = (size_t)(Tmax / h->cfg.hop), Q = F + h->taps - 1;
  return (pad64((size_t)B * h->cfg.hop * Q) + pad64((size_t)B * h->bins * F)) * sizeof(float) + 256;
}

int us_mel_forward(us_mel_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, const float* mel_min, const float* mel_max,
                   int n_norm, float pad_value, float* out, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!h || !wav || !out || B <= 0 || Tmax <= 0) return WeightTable::fail(h, US_EINVAL, "us_mel_forward: bad argument");
  const auto& c = h->cfg;
  if (n_norm != 0 && n_norm != 1 && n_norm != c.num_mels)
    return h->fail(US_EINVAL, "us_mel_forward: n_norm must be 0 (no normalisation), 1 or num_mels");
  if (n_norm != 0 && (!mel_min || !mel_max)) return h->fail(US_EINVAL, "us_mel_forward: n_norm > 0 needs mel_min and mel_max");
  if (Tmax < c.hop || Tmax <= h->pad)
    return h->fail(US_EINVAL, "us_mel_forward: Tmax must be at least hop and above (n_fft - hop) / 2 (the reflect padding)");
  if (Tmax > (1 << 30)) return h->fail(US_EINVAL, "us_mel_forward: Tmax above 2^30 is not built");      // q * hop + ci and 2 len - s stay far inside 64 bits
  int rc = mel_check_lengths(h, "us_mel_forward", lengths, B, h->pad, Tmax);
  if (rc != US_OK) return rc;
  if ((rc = h->all_loaded("us_mel_forward")) != US_OK) return rc;
  if (!workspace || workspace_bytes < us_mel_workspace_bytes(h, B, Tmax))
    return h->fail(US_EWORKSPACE, "us_mel_forward: workspace too small (us_mel_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int F = Tmax / c.hop, Q = F + h->taps - 1, live = h->live;
  float* X = ws_align(workspace);
  float* MAG = X + pad64((size_t)B * c.hop * Q);
  const unsigned tiles = (unsigned)((F + kMelBN - 1) / kMelBN);
  for_item_groups<kMelItems>(B, [&](int b) { return lengths ? lengths[b] : Tmax; }, [&](int b0, int nb, const ItemLens<kMelItems>& samples, int) {
    float* Xb = X + (size_t)b0 * c.hop * Q;
    float* Mb = MAG + (size_t)b0 * live * F;
    hipLaunchKernelGGL(mel_frame_kernel, dim3((unsigned)((Q + 63) / 64), (unsigned)((c.hop + 63) / 64), (unsigned)nb), dim3(256), 0, s,
                       wav + (size_t)b0 * Tmax, Xb, samples, Tmax, c.hop, h->pad, Q);
    MelDftArgs d{Xb, h->dft, Mb, c.hop, Q, F, live, c.n_fft, h->dft_Kpad, h->dft_ldw};
    hipLaunchKernelGGL(mel_dft_kernel, dim3(tiles, (unsigned)(h->dft_ldw / kPcBM), (unsigned)nb), dim3(256), 0, s, d);
    MelProjArgs p{};
    p.mag = Mb; p.w = h->proj; p.mel_min = mel_min; p.mel_max = mel_max; p.out = out + (size_t)b0 * c.num_mels * F;
    for (int i = 0; i < kMelItems; ++i) p.frames.n[i] = samples.n[i] / c.hop;
    p.pad_value = pad_value; p.n_norm = n_norm; p.num_mels = c.num_mels; p.F = F; p.live = live;
    p.Kpad = h->proj_Kpad; p.ldw = h->proj_ldw;
    hipLaunchKernelGGL(mel_proj_kernel, dim3(tiles, (unsigned)(h->proj_ldw / kPcBM), (unsigned)nb), dim3(256), 0, s, p);
  });
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_mel_forward", e);
}

int us_mel_minmax(us_mel_handle h, const float* mel, const int64_t* lengths_frames, int B, int F, float* out, us_stream stream) {
  if (!h || !mel || !out || B <= 0 || F <= 0) return WeightTable::fail(h, US_EINVAL, "us_mel_minmax: bad argument");
  int rc = mel_check_lengths(h, "us_mel_minmax", lengths_frames, B, -1, F);
  if (rc != US_OK) return rc;
  if ((rc = h->on_device("us_mel_minmax")) != US_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int M = h->cfg.num_mels;
  for_item_groups<kMelItems>(B, [&](int b) { return lengths_frames ? lengths_frames[b] : F; }, [&](int b0, int nb, const ItemLens<kMelItems>& frames, int) {
    hipLaunchKernelGGL(mel_minmax_kernel, dim3((unsigned)M), dim3(256), 0, s, mel + (size_t)b0 * M * F, frames, nb, M, F, out, b0 > 0 ? 1 : 0);
  });
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_mel_minmax", e);
}

}  // extern "C"
