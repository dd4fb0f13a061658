// Sinc resampler (torchaudio.transforms.Resample / torchaudio.functional.resample, which the reference calls at finetune.py:113,
// scripts/voice_conversion.py:63 and data.py:75,193): waveform [B][Tmax] with per-item lengths -> [B][ceil(new * Tmax / orig)], fp32 storage
// and accumulation, exact fp32 products.  orig and new are the two rates divided by their gcd.
//
// torchaudio's resampler is a strided Conv1d(1 -> new, k = K = orig + 2 width, stride = orig) over the zero-padded waveform; output sample
// i = q * new + c of an item of len samples is
//   out[i] = sum_{k < K} kernel[c][0][k] * y[q * orig + k - width],   y = 0 outside [0, len),   i < ceil(new * len / orig).
// Fold the waveform into a planar tensor X[ci][q] = y[q * orig + ci - width] (ci < orig): with k = j * orig + ci the sum is
// sum_{j, ci} P[j * orig + ci][c] * X[ci][q + j], a Conv1d(orig -> new, taps = ceil(K / orig)) in the form conv1d_planar.h's main loop
// multiplies on v_mfma_f32_32x32x2_f32, the phase c as the MFMA row and the frame q as the column.  The kernels:
//  - rs_fold_kernel: the zero padding at the item's own length and the de-interleave into X [B][orig][Q], transposed through LDS so that
//    reads and writes are both coalesced.  Nothing at or past wav[b][len_b] is read (a batch row's tail may hold anything).
//  - rs_pack_kernel: P[k][c] = kernel[c][0][k], zero in the padding, once per loaded kernel.
//  - rs_gemm_kernel: the main loop with Cin = orig, dil 1, off 0 and Kdim = K -- NOT taps * orig: the loader zeroes the operand rows at
//    and past Kdim, so a tap count that does not divide K costs no products (K = 459 runs 464 rows, not 882) and a sample outside
//    [q * orig - width, q * orig - width + K) never meets frame q, not even as 0 * NaN.
//    planar_conv_mainloop<2, 1>: a wave's tile is 32 phases x 64 frames with ONE accumulator chain per sub-tile, the two sub-tiles keep the
//    matrix core busy.  A second chain would take every other pair of taps; the taps of a windowed sinc alternate in sign every orig / new
//    samples or so, and for a smooth waveform the two halves would each be a partial sum that cancels only in the final addition (mel.hip
//    has the same note for its twiddles).  One chain adds the K products in sample order, which is the order the accuracy bar of
//    tests/test_resample_gpu.py was derived for.
//    Epilogue: for a fixed q the phases of a tile are contiguous in the output, but an accumulator lane holds one q and 16 phases.  The
//    tile goes through LDS, 64 frames x 64 phases at a time (row pitch 65 floats: a half-wave's ds_write_b32 hits 32 different banks, the
//    row reads are contiguous), and is stored as one flat run per frame -- for new <= 64, where one tile holds every phase, the frames'
//    runs join into one contiguous run per 32 frames.  The main loop's LDS arrays are private to it, so the staging tile is the kernel's
//    own: 24 KiB + 16.25 KiB per workgroup.  Outputs from the item's own count to the row's end are 0; nothing at or past
//    out[b][out_len] is written.
// A sample's value depends on its own item's samples only and every sum has a fixed order: an item alone or in a batch, and repeated
// calls, give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/unitspeech_hip.h"
#include "conv1d_planar.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kRsBN = 128;          // frames per workgroup (planar_conv_mainloop<2, 1>)
constexpr int kRsItems = 64;        // batch items per launch (item_lens.h): the samples of each
constexpr int kRsMaxRate = 4096;

// X[b][ci][q] = y_b[q * orig + ci - width], 0 outside [0, len_b).  One workgroup: 64 ci x 64 q.
__global__ __launch_bounds__(256) void rs_fold_kernel(const float* __restrict__ wav, float* __restrict__ x, ItemLens<kRsItems> lens, int Tmax,
                                                      int orig, int width, int Q) {
  planar_fold_tile(wav, x, lens, Tmax, orig, Q, [=](const float* __restrict__ w, long long len, int q, int ci) {
    const long long s = (long long)q * orig + ci - width;
    return (q < Q && ci < orig && s >= 0 && s < len) ? w[s] : 0.f;
  });
}

// P[k][c] = kernel[c][0][k] for k < K, c < nw, zero in the padding
__global__ void rs_pack_kernel(const float* __restrict__ kernel, float* __restrict__ p, int nw, int K, int Kpad, int ldw) {
  const int total = Kpad * ldw;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
    const int c = i % ldw, k = i / ldw;
    p[i] = (c < nw && k < K) ? kernel[(size_t)c * K + k] : 0.f;
  }
}

struct RsGemmArgs {
  const float* x;             // [B][orig][Q]
  const float* w;             // [Kpad][ldw]
  float* out;                 // [B][out_ld]
  ItemLens<kRsItems> samples;
  long long out_ld;           // ceil(nw * Tmax / orig)
  int orig, nw, Q, Kdim, Kpad, ldw;
};

__global__ __launch_bounds__(256) void rs_gemm_kernel(RsGemmArgs a) {
  __shared__ float stage[64][65];
  PLANAR_LANE(threadIdx.x);
  const int b = blockIdx.z;
  const int m0 = blockIdx.y * kPcBM, n0 = blockIdx.x * kRsBN;
  f32x16 acc[2][1];
  planar_conv_mainloop<2, 1>({a.x + (size_t)b * a.orig * a.Q, a.w, a.orig, a.Q, 1, 0, a.Kdim, a.Kpad, a.ldw, m0, n0}, acc);
  const long long target = ((long long)a.nw * a.samples.n[b] + a.orig - 1) / a.orig;
  float* __restrict__ out = a.out + (size_t)b * a.out_ld;
  const int live = min(kPcBM, a.nw - m0);          // phases of this tile that exist
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    if (n) __syncthreads();                        // pass 0's reads are done
    // pass n: sub-tile n of every wave.  Staging row PLANAR_COL(1, 0) = 32 nh + cl is frame n0 + PLANAR_COL(2, n) = n0 + (2 nh + n) * 32 + cl.
#pragma unroll
    for (int r = 0; r < 16; ++r) stage[PLANAR_COL(1, 0)][PLANAR_ROW(r)] = acc[n][0][r];
    __syncthreads();
    for (int e = threadIdx.x; e < 64 * live; e += 256) {
      const int j = e / live, c = e - j * live;
      const int q = n0 + ((j >> 5) * 2 + n) * 32 + (j & 31);
      const long long i = (long long)q * a.nw + m0 + c;
      if (i < a.out_ld) out[i] = i < target ? stage[j][c] : 0.f;
    }
  }
}

}  // namespace
}  // namespace us

struct us_resample : us::WeightTable {
  us_resample_config cfg{};
  int K = 0, taps = 0, Kpad = 0, ldw = 0;
  float* packed = nullptr;             // [Kpad][ldw]
};

namespace us {
namespace {

long long rs_out_length(const us_resample* h, long long T) { return ((long long)h->cfg.new_freq * T + h->cfg.orig_freq - 1) / h->cfg.orig_freq; }
// frames the GEMM computes for rows of Tmax samples, and the columns of X they read
long long rs_frames(const us_resample* h, long long Tmax) { return (rs_out_length(h, Tmax) + h->cfg.new_freq - 1) / h->cfg.new_freq; }

}  // namespace
}  // namespace us

extern "C" {

using namespace us;

int us_resample_create(us_resample_handle* out, const us_resample_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_resample_create: null argument");
  const auto& c = *cfg;
  if (c.orig_freq <= 0 || c.new_freq <= 0) return WeightTable::fail(nullptr, US_EINVAL, "us_resample_create: orig_freq and new_freq must be positive");
  if (c.width < 0) return WeightTable::fail(nullptr, US_EINVAL, "us_resample_create: width must not be negative");
  if (c.orig_freq > kRsMaxRate || c.new_freq > kRsMaxRate)
    return WeightTable::fail(nullptr, US_EINVAL, "us_resample_create: orig_freq or new_freq above 4096 after the division by their gcd is not built");
  if (c.width > (1 << 16)) return WeightTable::fail(nullptr, US_EINVAL, "us_resample_create: width above 2^16 is not built");      // Kpad * ldw < 2^31
  int g = c.orig_freq, r = c.new_freq;
  while (r) { const int t = g % r; g = r; r = t; }
  if (g != 1) return WeightTable::fail(nullptr, US_EINVAL, "us_resample_create: orig_freq and new_freq must be divided by their gcd");
  auto* h = new us_resample();
  h->cfg = c;
  h->K = c.orig_freq + 2 * c.width;
  h->taps = (h->K + c.orig_freq - 1) / c.orig_freq;
  h->Kpad = round_up(h->K, kPcBK);
  h->ldw = round_up(c.new_freq, kPcBM);
  (void)hipGetDevice(&h->device);
  h->add("kernel", {c.new_freq, 1, h->K});
  *out = h;
  return US_OK;
}

int us_resample_destroy(us_resample_handle h) {
  if (!h) return US_OK;
  h->free_weights();
  if (h->packed) (void)hipFree(h->packed);
  delete h;
  return US_OK;
}

int us_resample_num_weights(us_resample_handle h) { return h ? h->num() : 0; }
const char* us_resample_weight_key(us_resample_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_resample_last_error(us_resample_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_resample_load_weight(us_resample_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  Weight* w;
  int rc = WeightTable::find(h, "us_resample_load_weight", key, data, shape, ndim, &w);
  if (rc != US_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e;
  if (!h->packed && (e = hipMalloc(&h->packed, (size_t)h->Kpad * h->ldw * sizeof(float))) != hipSuccess)
    return h->hip("us_resample_load_weight: hipMalloc", e);
  if ((rc = h->copy(*w, data, s)) != US_OK) return rc;
  w->loaded = true;
  const int total = h->Kpad * h->ldw;
  hipLaunchKernelGGL(rs_pack_kernel, dim3((unsigned)std::min((total + 255) / 256, 4096)), dim3(256), 0, s, w->dev, h->packed, h->cfg.new_freq, h->K,
                     h->Kpad, h->ldw);
  e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_resample_load_weight", e);
}

int64_t us_resample_out_length(us_resample_handle h, int64_t T) { return (h && T > 0) ? (int64_t)rs_out_length(h, T) : 0; }

// X [B][orig][Q], Q = frames + taps - 1
size_t us_resample_workspace_bytes(us_resample_handle h, int B, int Tmax) {
  if (!h || B <= 0 || Tmax <= 0) return 0;
  const size_t Q = (size_t)rs_frames(h, Tmax) + h->taps - 1;
  return pad64((size_t)B * h->cfg.orig_freq * Q) * sizeof(float) + 256;
}

int us_resample_forward(us_resample_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, float* out, void* workspace,
                        size_t workspace_bytes, us_stream stream) {
  if (!h || !wav || !out || B <= 0) return WeightTable::fail(h, US_EINVAL, "us_resample_forward: bad argument");
  const auto& c = h->cfg;
  // q * orig + ci, q * new + c and new * len stay far inside 64 bits, the frame count inside 32
  if (Tmax < 1 || Tmax > (1 << 30)) return h->fail(US_EINVAL, "us_resample_forward: Tmax must be in [1, 2^30]");
  const std::string bad = bad_length("us_resample_forward", lengths, B, 1, Tmax);
  if (!bad.empty()) return h->fail(US_EINVAL, bad + " is outside [1, " + std::to_string(Tmax) + "]");
  int rc = h->all_loaded("us_resample_forward");
  if (rc != US_OK) return rc;
  if (!workspace || workspace_bytes < us_resample_workspace_bytes(h, B, Tmax))
    return h->fail(US_EWORKSPACE, "us_resample_forward: workspace too small (us_resample_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long out_ld = rs_out_length(h, Tmax);
  const int F = (int)rs_frames(h, Tmax), Q = F + h->taps - 1;
  float* X = ws_align(workspace);
  const unsigned tiles = (unsigned)((F + kRsBN - 1) / kRsBN);
  for_item_groups<kRsItems>(B, [&](int b) { return lengths ? lengths[b] : Tmax; }, [&](int b0, int nb, const ItemLens<kRsItems>& samples, int) {
    RsGemmArgs g{};
    g.samples = samples;
    float* Xb = X + (size_t)b0 * c.orig_freq * Q;
    hipLaunchKernelGGL(rs_fold_kernel, dim3((unsigned)((Q + 63) / 64), (unsigned)((c.orig_freq + 63) / 64), (unsigned)nb), dim3(256), 0, s,
                       wav + (size_t)b0 * Tmax, Xb, samples, Tmax, c.orig_freq, c.width, Q);
    g.x = Xb; g.w = h->packed; g.out = out + (size_t)b0 * out_ld; g.out_ld = out_ld;
    g.orig = c.orig_freq; g.nw = c.new_freq; g.Q = Q; g.Kdim = h->K; g.Kpad = h->Kpad; g.ldw = h->ldw;
    hipLaunchKernelGGL(rs_gemm_kernel, dim3(tiles, (unsigned)(h->ldw / kPcBM), (unsigned)nb), dim3(256), 0, s, g);
  });
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_resample_forward", e);
}

}  // extern "C"
