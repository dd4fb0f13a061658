// ECAPA-TDNN speaker encoder, eval-mode forward (the reference's unitspeech/speaker_encoder/ecapa_tdnn.py:248-287 `get_feat` +
// `forward`, :15-161 the modules they call): the upstream model's hidden states [L][B][T][C] -> embedding [B][emb_dim], fp32
// storage and fp32 accumulation throughout.
//
// Activations are planar [B][C][T] (time contiguous), the layout of the reference's tensors.  The kernels:
//  - sp_combine_kernel: the softmax-weighted sum over the L hidden states (+ 1e-6), read once and coalesced along C, transposed
//    through LDS into [B][C][T];  sp_instnorm_kernel: InstanceNorm1d, one wave per (b, c) row.
//  - sp_conv_kernel: every dense convolution (layer1's k = 5, the 1x1 ones, the pooling's two) as an implicit GEMM on the fp32 matrix
//    cores (v_mfma_f32_32x32x2_f32, exact fp32 products): D[co][t] = sum_kk W[co][kk] X[kk][t], kk = tap * Cin + ci.  Epilogue: bias,
//    a per-(b, co) bias (the global-context terms of the pooling), ReLU / tanh, then the eval-mode BatchNorm as one scale and one
//    shift per channel (it follows the ReLU, so it cannot live in the weights).
//  - sp_res2_kernel: the seven chained width -> width k = 3 dilated convolutions of a Res2Conv1dReluBn for one time tile, the running
//    chunk held in LDS with a 7 * dilation halo on either side; plain fp32 FMAs (the vector units have the fp32 matrix cores' rate and
//    the chunks are 64 channels at most), each lane one time step, the weights wave-uniform.
//  - sp_rowmean_kernel / sp_se_kernel / sp_scale_res_kernel: SE_Connect and the block residual.
//  - sp_rowstats_kernel / sp_ctx_bias_kernel: the global-context mean / std and their share of pooling.linear1 as a bias.
//  - sp_pool_kernel: softmax over T and the weighted mean / std per (b, c) row, `bn` applied;  sp_linear_kernel;  sp_normalize_kernel.
// Every reduction is a fixed-order tree inside one wave (or a fixed-order loop over waves): no atomics, so a batch item's result
// does not depend on its neighbours or on the run.
//
// Ragged batches (us_speaker_forward_lengths): every kernel that looks along time is a template over how it learns an item's length, SameT
// or ItemLens<kSpItems> (item_lens.h; an item's length is at least 1 and at most T).  The time tiles start where they start when the item
// runs alone, and every sum runs over the same terms in the same order, so the item's result has the bits of the uniform call on the item
// alone.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <map>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"
#include "conv1d_planar.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kSpOut = 1536;       // ecapa_tdnn.py:222: channels of `conv` and of the pooling
constexpr int kSpAtt = 128;        // se_bottleneck_dim and attention_channels (:225-232)
constexpr int kSpScale = 8;        // Res2 scale
constexpr int kSpStages = kSpScale - 1;
constexpr float kBnEps = 1e-5f;

constexpr int kSpItems = 32;       // batch items per launch of the ragged form (item_lens.h)

// The (b, c) row of a one-wave-per-row kernel and its valid steps; false: the wave has no row.  Uniform: rows are numbered through the
// whole batch, four per workgroup.  Ragged: blockIdx.y is the item (its length a scalar load), blockIdx.x * 4 + wave the channel.
template <class LN>
__device__ __forceinline__ bool sp_row(const LN& lens, int C, int rows, int T, int& row, int& n) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (LN::ragged) {
    if (w >= C) return false;
    row = blockIdx.y * C + w;
    n = lens(blockIdx.y, T);
    return true;
  }
  row = w;
  n = T;
  return w < rows;
}

// ---- feature combine + instance norm (get_feat, :261-271) ------------------------------------------------------------------
constexpr int kCmbT = 16, kCmbC = 64;

// B: the items of the whole tensor h (its layer stride), of which this launch takes gridDim.z from h on
template <class LN>
__global__ __launch_bounds__(256) void sp_combine_kernel(const float* __restrict__ h, const float* __restrict__ lw, float* __restrict__ x,
                                                         int L, int B, int T, int C, LN lens) {
  __shared__ float tile[kCmbT][kCmbC + 1];
  const int tid = threadIdx.x, cl = tid & 63, tr = tid >> 6;
  const int c0 = blockIdx.x * kCmbC, t0 = blockIdx.y * kCmbT, b = blockIdx.z;
  const int n = lens(b, T);
  if (LN::ragged && t0 >= n) return;
  const int c = c0 + cl;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  const size_t lstride = (size_t)B * T * C;
  const float* hb = h + (size_t)b * T * C + c;
  for (int l = 0; l < L; ++l) {
    const float wl = lw[l];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int t = t0 + tr + 4 * i;
      if (t < n && c < C) acc[i] = fmaf(wl, hb[(size_t)l * lstride + (size_t)t * C], acc[i]);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) tile[tr + 4 * i][cl] = acc[i] + 1e-6f;
  __syncthreads();
  const int cc = tid >> 2, tq = (tid & 3) * 4;
  if (c0 + cc < C) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int t = t0 + tq + j;
      if (t < n) x[((size_t)b * C + c0 + cc) * T + t] = tile[tq + j][cc];
    }
  }
}

__global__ void sp_layer_softmax_kernel(const float* __restrict__ w, float* __restrict__ lw, int L) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float m = w[0];
  for (int l = 1; l < L; ++l) m = fmaxf(m, w[l]);
  float s = 0.f;
  for (int l = 0; l < L; ++l) s += expf(w[l] - m);
  for (int l = 0; l < L; ++l) lw[l] = expf(w[l] - m) / s;
}

// InstanceNorm1d without affine: biased variance over the item's n steps, eps 1e-5.  One wave per row; `out` may be `in`.  The ragged form
// writes zeros on [n, T): layer1.conv (k = 5) then reads past an item's end the zeros it pads with when the item runs alone.
template <class LN>
__global__ __launch_bounds__(256) void sp_instnorm_kernel(const float* in, float* out, int C, int rows, int T, LN lens) {
  const int lane = threadIdx.x & 63;
  int row, n;
  if (!sp_row(lens, C, rows, T, row, n)) return;
  const float* r = in + (size_t)row * T;
  float s = 0.f;
  for (int t = lane; t < n; t += 64) s += r[t];
  const float mean = wave_sum(s) / (float)n;
  float v = 0.f;
  for (int t = lane; t < n; t += 64) {
    const float d = r[t] - mean;
    v = fmaf(d, d, v);
  }
  const float rs = 1.f / sqrtf(wave_sum(v) / (float)n + 1e-5f);
  float* o = out + (size_t)row * T;
  for (int t = lane; t < n; t += 64) o[t] = (r[t] - mean) * rs;
  if (LN::ragged)
    for (int t = n + lane; t < T; t += 64) o[t] = 0.f;
}

// ---- implicit-GEMM convolution ------------------------------------------------------------------------------------------------
// out[b][co][t] = post(bias[co] + bias2[b][co] + sum_{j < taps, ci} P[j * Cin + ci][co] * in[b][ci][t + j - taps / 2]), in[] = 0 outside
// [0, T): the main loop and the pack P are conv1d_planar.h's.  64 steps per workgroup: a wave's tile is 32 channels x 32 steps,
// planar_conv_mainloop<1, 2> (one sub-tile, two accumulator chains taking the K slice's products in turn).  `in` and `out` carry their
// own batch strides, so a tensor may be a channel slice of a wider one (the [out2, out3, out4] concatenation is written in place by the
// three blocks).
constexpr int kSpBN = 64;      // time steps per workgroup
enum { kActNone = US_SPEAKER_ACT_NONE, kActRelu = US_SPEAKER_ACT_RELU, kActTanh = US_SPEAKER_ACT_TANH };

struct SpConvArgs {
  const float* in;
  const float* w;             // [Kpad][ldw]
  const float* bias;          // [Cout]
  const float* bias2;         // [B][Cout] or null
  const float* scale;         // [Cout] or null: applied with shift after the activation
  const float* shift;
  float* out;
  long long in_bs, out_bs;    // floats between batch items
  int Cin, Cout, T, off, Kdim, Kpad, ldw, act;
};

// Ragged: a workgroup whose 64 steps all lie at or past the item's end returns before the first barrier, and no step at or past it is
// stored.  The loader still reads columns up to the row's T: a k = 1 output column depends on its own input column alone, so whatever
// lies past the end stays in columns that are never stored, and layer1's k = 5 reads the zeros sp_instnorm_kernel wrote there.
template <class LN>
__global__ __launch_bounds__(256) void sp_conv_kernel(SpConvArgs a, LN lens) {
  PLANAR_LANE(threadIdx.x);
  const int b = blockIdx.z;
  const int m0 = blockIdx.y * kPcBM, n0 = blockIdx.x * kSpBN;
  const int n = lens(b, a.T);
  if (LN::ragged && n0 >= n) return;
  f32x16 acc[1][2];
  planar_conv_mainloop<1, 2>({a.in + (size_t)b * a.in_bs, a.w, a.Cin, a.T, 1, a.off, a.Kdim, a.Kpad, a.ldw, m0, n0}, acc);
  const int t = PLANAR_STEP(1, n0, 0);
  if (t >= n) return;
  float* __restrict__ out = a.out + (size_t)b * a.out_bs;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int co = PLANAR_CHANNEL(m0, r);
    if (co >= a.Cout) continue;
    float v = (acc[0][0][r] + acc[0][1][r]) + a.bias[co];
    if (a.bias2) v += a.bias2[(size_t)b * a.Cout + co];
    if (a.act == kActRelu) v = fmaxf(v, 0.f);
    else if (a.act == kActTanh) v = tanhf(v);
    if (a.scale) v = fmaf(v, a.scale[co], a.shift[co]);
    out[(size_t)co * a.T + t] = v;
  }
}

// BatchNorm1d in eval mode as y = x * scale + shift
__global__ void sp_bnfold_kernel(const float* __restrict__ w, const float* __restrict__ b, const float* __restrict__ rm, const float* __restrict__ rv,
                                 float* __restrict__ scale, float* __restrict__ shift, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const float s = w[i] / sqrtf(rv[i] + kBnEps);
  scale[i] = s;
  shift[i] = b[i] - rm[i] * s;
}

// ---- Res2Conv1dReluBn (:35-51) --------------------------------------------------------------------------------------------------
// One workgroup: batch item b, output steps [t0, t0 + TT), all seven stages.  Its LDS window holds kRes2W = TT + 14 * dil positions,
// position p <-> time t0 - 7 dil + p.  Stage i reads the window S (= stage i - 1's output + split i; split 0 for i = 0) and writes
// bn(relu(conv(S))) over the WHOLE window, taking S as zero beyond the window's ends: a position within (i + 1) dil of an end is then
// wrong, which after seven stages still leaves the TT central ones exact.  A position outside [0, T) is forced to zero at every stage
// (each convolution pads its own input with zeros; the value the previous stage would compute there from zeros is not one).  Ragged: the
// item's end n takes the place of T in `inside` and in every read, rows stay T apart, and a tile that starts at or past n returns at once.
// Lane = position, so the weights of a (ci, tap) are wave-uniform: 16 output channels per lane, packed contiguously.
constexpr int kRes2W = 128;
constexpr int kRes2Co = 16;

template <class LN>
__global__ __launch_bounds__(512) void sp_res2_kernel(const float* __restrict__ y, float* __restrict__ out, const float* __restrict__ wp,
                                                      const float* __restrict__ bss, int width, int wpad, int T, int dil, int TT, LN lens) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int b = blockIdx.y, t0 = blockIdx.x * TT, halo = kSpStages * dil, base = t0 - halo;
  const int n = lens(b, T);
  if (LN::ragged && t0 >= n) return;
  const size_t bo = (size_t)b * kSpScale * width * T;
  const float* __restrict__ yb = y + bo;
  float* __restrict__ ob = out + bo;
  const int half = width * kRes2W;              // the two windows: stage i reads the one at (i & 1) * half and writes the other
  for (int idx = tid; idx < width * kRes2W; idx += 512) {
    const int ci = idx / kRes2W, p = idx - ci * kRes2W, t = base + p;
    lds[idx] = (t >= 0 && t < n) ? yb[(size_t)ci * T + t] : 0.f;
  }
  // the eighth split passes through (:47-48)
  for (int idx = tid; idx < width * TT; idx += 512) {
    const int ci = idx / TT, t = t0 + idx - ci * TT;
    if (t < n) ob[(size_t)((kSpScale - 1) * width + ci) * T + t] = yb[(size_t)((kSpScale - 1) * width + ci) * T + t];
  }
  __syncthreads();
  const int p = (wave & 1) * 64 + lane, t = base + p, cog = wave >> 1;
  const bool inside = t >= 0 && t < n;
  const bool centre = inside && p >= halo && p < halo + TT;
  const bool lo = p - dil >= 0, hi = p + dil < kRes2W;
  for (int i = 0; i < kSpStages; ++i) {
    const float* __restrict__ cur = lds + (i & 1) * half;
    float* __restrict__ nxt = lds + ((i & 1) ^ 1) * half;
    const float* __restrict__ wi = wp + (size_t)i * width * 3 * wpad;
    const float* __restrict__ bi = bss + (size_t)i * 3 * wpad;
    for (int co0 = cog * kRes2Co; co0 < width; co0 += 4 * kRes2Co) {
      float acc[kRes2Co];
#pragma unroll
      for (int j = 0; j < kRes2Co; ++j) acc[j] = bi[co0 + j];
      for (int ci = 0; ci < width; ++ci) {
        const float* row = cur + ci * kRes2W + p;
        const float xm = lo ? row[-dil] : 0.f, x0 = row[0], xp = hi ? row[dil] : 0.f;
        const float* __restrict__ w = wi + (size_t)ci * 3 * wpad + co0;
#pragma unroll
        for (int j = 0; j < kRes2Co; ++j) {
          acc[j] = fmaf(w[j], xm, acc[j]);
          acc[j] = fmaf(w[wpad + j], x0, acc[j]);
          acc[j] = fmaf(w[2 * wpad + j], xp, acc[j]);
        }
      }
#pragma unroll
      for (int j = 0; j < kRes2Co; ++j) {
        const int co = co0 + j;
        if (co >= width) break;
        float v = fmaf(fmaxf(acc[j], 0.f), bi[wpad + co], bi[2 * wpad + co]);
        v = inside ? v : 0.f;
        if (centre) ob[(size_t)(i * width + co) * T + t] = v;
        if (i + 1 < kSpStages) nxt[co * kRes2W + p] = v + (inside ? yb[(size_t)((i + 1) * width + co) * T + t] : 0.f);
      }
    }
    __syncthreads();
  }
}

// stage i of a block: wp[i][ci][tap][co] (co padded to wpad with zeros) and bss[i][{bias, bn scale, bn shift}][co]
__global__ void sp_res2_pack_kernel(const float* __restrict__ w, const float* __restrict__ bias, const float* __restrict__ bw,
                                    const float* __restrict__ bb, const float* __restrict__ rm, const float* __restrict__ rv, float* __restrict__ wp,
                                    float* __restrict__ bss, int width, int wpad) {
  const int n = width * 3 * wpad;
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
    const int co = i % wpad, k = (i / wpad) % 3, ci = i / (3 * wpad);
    wp[i] = co < width ? w[((size_t)co * width + ci) * 3 + k] : 0.f;
  }
  for (int co = blockIdx.x * blockDim.x + threadIdx.x; co < wpad; co += gridDim.x * blockDim.x) {
    const bool live = co < width;
    const float s = live ? bw[co] / sqrtf(rv[co] + kBnEps) : 0.f;
    bss[co] = live ? bias[co] : 0.f;
    bss[wpad + co] = s;
    bss[2 * wpad + co] = live ? bb[co] - rm[co] * s : 0.f;
  }
}

// ---- SE_Connect (:78-84) and the block residual (:126) --------------------------------------------------------------------------
template <class LN>
__global__ __launch_bounds__(256) void sp_rowmean_kernel(const float* __restrict__ in, float* __restrict__ mean, int C, int rows, int T, LN lens) {
  const int lane = threadIdx.x & 63;
  int row, n;
  if (!sp_row(lens, C, rows, T, row, n)) return;
  const float* r = in + (size_t)row * T;
  float s = 0.f;
  for (int t = lane; t < n; t += 64) s += r[t];
  s = wave_sum(s);
  if (lane == 0) mean[row] = s / (float)n;
}

// s[b][c] = sigmoid(W2 relu(W1 mean[b] + b1) + b2); one workgroup per batch item, one wave per output
__global__ __launch_bounds__(1024) void sp_se_kernel(const float* __restrict__ mean, const float* __restrict__ w1, const float* __restrict__ b1,
                                                     const float* __restrict__ w2, const float* __restrict__ b2, float* __restrict__ s, int ch) {
  extern __shared__ float sm[];          // mean [ch], hidden [kSpAtt]
  float* hid = sm + ch;
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int c = threadIdx.x; c < ch; c += 1024) sm[c] = mean[(size_t)b * ch + c];
  __syncthreads();
  for (int j = wave; j < kSpAtt; j += 16) {
    float a = 0.f;
    for (int c = lane; c < ch; c += 64) a = fmaf(w1[(size_t)j * ch + c], sm[c], a);
    a = wave_sum(a);
    if (lane == 0) hid[j] = fmaxf(a + b1[j], 0.f);
  }
  __syncthreads();
  for (int c = wave; c < ch; c += 16) {
    float a = 0.f;
    for (int j = lane; j < kSpAtt; j += 64) a = fmaf(w2[(size_t)c * kSpAtt + j], hid[j], a);
    a = wave_sum(a);
    if (lane == 0) s[(size_t)b * ch + c] = 1.f / (1.f + expf(-(a + b2[c])));
  }
}

// Ragged: the loop runs over the item's ch * n valid elements only, so the workgroups past them (the grid is sized for T) have no turn
template <class LN>
__global__ __launch_bounds__(256) void sp_scale_res_kernel(const float* __restrict__ y, const float* __restrict__ s, const float* __restrict__ res,
                                                           float* __restrict__ out, int ch, int T, long long res_bs, long long out_bs, LN lens) {
  const int b = blockIdx.y;
  const int len = lens(b, T);
  const size_t n = (size_t)ch * T, live = (size_t)ch * len;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < live; i += (size_t)gridDim.x * blockDim.x) {
    const int c = (int)(i / len);
    const size_t j = LN::ragged ? (size_t)c * T + (i - (size_t)c * len) : i;
    out[(size_t)b * out_bs + j] = fmaf(y[(size_t)b * n + j], s[(size_t)b * ch + c], res[(size_t)b * res_bs + j]);
  }
}

// ---- AttentiveStatsPool (:145-161) ------------------------------------------------------------------------------------------------
// global context: ctx[b][0][c] = mean over T, ctx[b][1][c] = sqrt(unbiased var + 1e-10) (torch.var's default; NaN for T = 1 as there)
template <class LN>
__global__ __launch_bounds__(256) void sp_rowstats_kernel(const float* __restrict__ in, float* __restrict__ ctx, int C, int rows, int T, LN lens) {
  const int lane = threadIdx.x & 63;
  int row, n;
  if (!sp_row(lens, C, rows, T, row, n)) return;
  const float* r = in + (size_t)row * T;
  float s = 0.f;
  for (int t = lane; t < n; t += 64) s += r[t];
  const float mean = wave_sum(s) / (float)n;
  float v = 0.f;
  for (int t = lane; t < n; t += 64) {
    const float d = r[t] - mean;
    v = fmaf(d, d, v);
  }
  v = wave_sum(v) / (float)(n - 1);
  if (lane == 0) {
    const int b = row / C, c = row - b * C;
    ctx[((size_t)b * 2) * C + c] = mean;
    ctx[((size_t)b * 2 + 1) * C + c] = sqrtf(v + 1e-10f);
  }
}

// the two constant thirds of linear1's input as a bias: bias2[b][j] = sum_c W1[j][C + c] mean[b][c] + W1[j][2 C + c] std[b][c]
__global__ __launch_bounds__(1024) void sp_ctx_bias_kernel(const float* __restrict__ ctx, const float* __restrict__ w1, float* __restrict__ bias2, int C) {
  const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const float* cb = ctx + (size_t)b * 2 * C;
  for (int j = wave; j < kSpAtt; j += 16) {
    const float* w = w1 + (size_t)j * 3 * C + C;
    float a = 0.f;
    for (int c = lane; c < 2 * C; c += 64) a = fmaf(w[c], cb[c], a);
    a = wave_sum(a);
    if (lane == 0) bias2[(size_t)b * kSpAtt + j] = a;
  }
}

// one wave per (b, c) row: alpha = softmax_T(e), mean = sum alpha x, std = sqrt(clamp(sum alpha x^2 - mean^2, 1e-9)); raw[b] = [mean | std]
// and bnd = raw * scale + shift (the eval-mode `bn` of :284)
template <class LN>
__global__ __launch_bounds__(256) void sp_pool_kernel(const float* __restrict__ x, const float* __restrict__ e, const float* __restrict__ scale,
                                                      const float* __restrict__ shift, float* __restrict__ raw, float* __restrict__ bnd, int C,
                                                      int rows, int T, LN lens) {
  const int lane = threadIdx.x & 63;
  int row, n;
  if (!sp_row(lens, C, rows, T, row, n)) return;
  const float* xr = x + (size_t)row * T;
  const float* er = e + (size_t)row * T;
  float m = -INFINITY;
  for (int t = lane; t < n; t += 64) m = fmaxf(m, er[t]);
  m = wave_max(m);
  float se = 0.f, sx = 0.f, sxx = 0.f;
  for (int t = lane; t < n; t += 64) {
    const float w = expf(er[t] - m), v = xr[t];
    se += w;
    sx = fmaf(w, v, sx);
    sxx = fmaf(w * v, v, sxx);
  }
  se = wave_sum(se);
  sx = wave_sum(sx);
  sxx = wave_sum(sxx);
  if (lane == 0) {
    const int b = row / C, c = row - b * C;
    const float mean = sx / se;
    // mean^2 rounded on its own, as the reference's `mean ** 2`: contracted into an fma the difference keeps the rounding error of
    // sxx / se, and at T = 1 (sxx / se = round(x^2), mean = x) that error, up to 6e-8 x^2, takes the place of the exact 0 the clamp is for
    // (the clamp keeps a NaN, as torch.clamp does and fmaxf does not: with the global context and T = 1 the reference's std is NaN)
    const float var = sxx / se - mul_rn(mean, mean);
    const float sd = sqrtf(var < 1e-9f ? 1e-9f : var);
    const size_t o = (size_t)b * 2 * C;
    raw[o + c] = mean;
    raw[o + C + c] = sd;
    bnd[o + c] = fmaf(mean, scale[c], shift[c]);
    bnd[o + C + c] = fmaf(sd, scale[C + c], shift[C + c]);
  }
}

// out[b][j] = bias[j] + sum_i W[j][i] p[b][i]; one wave per output
__global__ __launch_bounds__(256) void sp_linear_kernel(const float* __restrict__ p, const float* __restrict__ w, const float* __restrict__ bias,
                                                        float* __restrict__ out, int B, int in_dim, int out_dim) {
  const int lane = threadIdx.x & 63, o = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (o >= B * out_dim) return;
  const int b = o / out_dim, j = o - b * out_dim;
  float a = 0.f;
  for (int i = lane; i < in_dim; i += 64) a = fmaf(w[(size_t)j * in_dim + i], p[(size_t)b * in_dim + i], a);
  a = wave_sum(a);
  if (lane == 0) out[o] = a + bias[j];
}

// x /= |x| over the n elements of row blockIdx.x (finetune.py:110); one workgroup per row, the sum of squares in fp64 in a fixed order
__global__ __launch_bounds__(256) void sp_normalize_kernel(float* __restrict__ x, int n) {
  __shared__ double part[256];
  x += (size_t)blockIdx.x * n;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)x[i] * (double)x[i];
  part[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) part[threadIdx.x] += part[threadIdx.x + o];
    __syncthreads();
  }
  const float norm = (float)sqrt(part[0]);
  for (int i = threadIdx.x; i < n; i += 256) x[i] = x[i] / norm;
}

// ---- host side ---------------------------------------------------------------------------------------------------------

struct SpBn {                   // one folded BatchNorm1d
  int n = 0;
  float* scale = nullptr;       // [2][n]: scale, shift
};

struct SpRes2 {
  float* wp = nullptr;          // [7][width][3][wpad]
  float* bss = nullptr;         // [7][3][wpad]
};

}  // namespace
}  // namespace us

struct us_speaker : us::WeightTable {      // keys: the floating-point entries only
  us_speaker_config cfg{};
  int width = 0, wpad = 0;
  std::map<std::string, us::PlanarConv> conv;
  std::map<std::string, us::SpBn> bn;
  std::map<std::string, us::SpRes2> res2;
  float* lw = nullptr;                 // softmax(feature_weight)
  bool allocated = false;              // device tensors exist (made by the first load, so creating a handle touches no device)
  bool dirty = true;                   // a weight changed since the derived forms were made
};

namespace us {
namespace {

void sp_add_conv(us_speaker* h, const std::string& p, int cin, int cin_tot, int cout, int k) {
  h->add(p + ".weight", {cout, cin_tot, k});
  h->add(p + ".bias", {cout});
  h->conv[p].conv(cin, cin_tot, cout, k, 1);
}

void sp_add_bn(us_speaker* h, const std::string& p, int n, bool folded) {
  h->add(p + ".weight", {n});
  h->add(p + ".bias", {n});
  h->add(p + ".running_mean", {n});
  h->add(p + ".running_var", {n});
  if (folded) h->bn[p].n = n;
}

void sp_add_linear(us_speaker* h, const std::string& p, int in, int out) {
  h->add(p + ".weight", {out, in});
  h->add(p + ".bias", {out});
}

// module registration order of ecapa_tdnn.py:206-234 (and :103-106, :27-33 inside a block)
void speaker_keys(us_speaker* h) {
  const auto& c = h->cfg;
  const int ch = c.channels;
  if (c.n_layers > 0) h->add("feature_weight", {c.n_layers});
  sp_add_conv(h, "layer1.conv", c.feat_dim, c.feat_dim, ch, 5);
  sp_add_bn(h, "layer1.bn", ch, true);
  for (int l = 2; l <= 4; ++l) {
    const std::string p = "layer" + std::to_string(l);
    sp_add_conv(h, p + ".Conv1dReluBn1.conv", ch, ch, ch, 1);
    sp_add_bn(h, p + ".Conv1dReluBn1.bn", ch, true);
    for (int i = 0; i < kSpStages; ++i) {
      const std::string q = p + ".Res2Conv1dReluBn.convs." + std::to_string(i);
      h->add(q + ".weight", {h->width, h->width, 3});
      h->add(q + ".bias", {h->width});
    }
    for (int i = 0; i < kSpStages; ++i) sp_add_bn(h, p + ".Res2Conv1dReluBn.bns." + std::to_string(i), h->width, false);
    h->res2[p];
    sp_add_conv(h, p + ".Conv1dReluBn2.conv", ch, ch, ch, 1);
    sp_add_bn(h, p + ".Conv1dReluBn2.bn", ch, true);
    sp_add_linear(h, p + ".SE_Connect.linear1", ch, kSpAtt);
    sp_add_linear(h, p + ".SE_Connect.linear2", kSpAtt, ch);
  }
  sp_add_conv(h, "conv", 3 * ch, 3 * ch, kSpOut, 1);
  sp_add_conv(h, "pooling.linear1", kSpOut, c.global_context_att ? 3 * kSpOut : kSpOut, kSpAtt, 1);
  sp_add_conv(h, "pooling.linear2", kSpAtt, kSpAtt, kSpOut, 1);
  sp_add_bn(h, "bn", 2 * kSpOut, true);
  sp_add_linear(h, "linear", 2 * kSpOut, c.emb_dim);
}

// every tensor the forward reads, at once: after the first load neither a load nor a forward allocates
hipError_t sp_alloc(us_speaker* h) {
  hipError_t e = hipSuccess;
  auto alloc = [&](float** p, size_t n) {
    if (e == hipSuccess && !*p) e = hipMalloc(p, std::max<size_t>(n, 1) * sizeof(float));
  };
  for (auto& kv : h->w) alloc(&kv.second.dev, kv.second.numel());
  for (auto& kv : h->conv) alloc(&kv.second.packed, kv.second.packed_floats());
  for (auto& kv : h->bn) alloc(&kv.second.scale, 2 * (size_t)kv.second.n);
  for (auto& kv : h->res2) {
    alloc(&kv.second.wp, (size_t)kSpStages * h->width * 3 * h->wpad);
    alloc(&kv.second.bss, (size_t)kSpStages * 3 * h->wpad);
  }
  alloc(&h->lw, 64);
  h->allocated = e == hipSuccess;
  return e;
}

// every derived form (packed GEMM weights, folded BatchNorms, the Res2 stage packs, the layer softmax) from the loaded tensors
void sp_prepare(us_speaker* h, hipStream_t s) {
  auto W = [&](const std::string& k) { return h->w.at(k).dev; };
  for (auto& kv : h->conv) kv.second.pack(W(kv.first + ".weight"), s);
  for (auto& kv : h->bn) {
    SpBn& b = kv.second;
    const std::string& p = kv.first;
    hipLaunchKernelGGL(sp_bnfold_kernel, dim3((b.n + 255) / 256), dim3(256), 0, s, W(p + ".weight"), W(p + ".bias"), W(p + ".running_mean"),
                       W(p + ".running_var"), b.scale, b.scale + b.n, b.n);
  }
  for (auto& kv : h->res2) {
    const std::string p = kv.first + ".Res2Conv1dReluBn.";
    for (int i = 0; i < kSpStages; ++i) {
      const std::string cv = p + "convs." + std::to_string(i), bn = p + "bns." + std::to_string(i);
      hipLaunchKernelGGL(sp_res2_pack_kernel, dim3(16), dim3(256), 0, s, W(cv + ".weight"), W(cv + ".bias"), W(bn + ".weight"), W(bn + ".bias"),
                         W(bn + ".running_mean"), W(bn + ".running_var"), kv.second.wp + (size_t)i * h->width * 3 * h->wpad,
                         kv.second.bss + (size_t)i * 3 * h->wpad, h->width, h->wpad);
    }
  }
  if (h->cfg.n_layers > 0) hipLaunchKernelGGL(sp_layer_softmax_kernel, dim3(1), dim3(64), 0, s, W("feature_weight"), h->lw, h->cfg.n_layers);
  h->dirty = false;
}

struct SpPlan {                 // float offsets into the 256-byte aligned workspace
  size_t x0, o1, cat, a, r, y, big, att, e, mean, s, ctx, b2, praw, pbn, total;
};

SpPlan sp_plan(const us_speaker_config& c, int B, int T) {
  SpPlan p{};
  WsTake take;
  const size_t bt = (size_t)B * T, ch = (size_t)c.channels;
  p.x0 = take(bt * c.feat_dim);
  p.o1 = take(bt * ch);
  p.cat = take(bt * 3 * ch);
  p.a = take(bt * ch);
  p.r = take(bt * ch);
  p.y = take(bt * ch);
  p.big = take(bt * kSpOut);
  p.att = take(bt * kSpAtt);
  p.e = take(bt * kSpOut);
  p.mean = take((size_t)B * ch);
  p.s = take((size_t)B * ch);
  p.ctx = take((size_t)B * 2 * kSpOut);
  p.b2 = take((size_t)B * kSpAtt);
  p.praw = take((size_t)B * 2 * kSpOut);
  p.pbn = take((size_t)B * 2 * kSpOut);
  p.total = take.total;
  return p;
}

template <class LN>
void sp_conv(us_speaker* h, hipStream_t s, const std::string& p, const std::string& bn, int act, const float* in, long long in_bs, float* out,
             long long out_bs, const float* bias2, int B, int T, const LN& lens) {
  const PlanarConv& c = h->conv.at(p);
  SpConvArgs a{};
  a.in = in; a.w = c.packed; a.bias = h->w.at(p + ".bias").dev; a.bias2 = bias2; a.out = out;
  if (!bn.empty()) {
    const SpBn& f = h->bn.at(bn);
    a.scale = f.scale; a.shift = f.scale + f.n;
  }
  a.in_bs = in_bs; a.out_bs = out_bs;
  a.Cin = c.cin; a.Cout = c.cout; a.T = T; a.off = c.off[0]; a.Kdim = c.Kdim(); a.Kpad = c.Kpad; a.ldw = c.ldw; a.act = act;
  hipLaunchKernelGGL((sp_conv_kernel<LN>), dim3((T + kSpBN - 1) / kSpBN, (c.cout + kPcBM - 1) / kPcBM, B), dim3(256), 0, s, a, lens);
}

// One wave per (b, c) row: the uniform form numbers the rows through the batch, the ragged one puts the item on blockIdx.y (sp_row)
template <class LN>
dim3 sp_rows_grid(int nb, int C) {
  return LN::ragged ? dim3((unsigned)((C + 3) / 4), (unsigned)nb) : dim3((unsigned)(((long long)nb * C + 3) / 4));
}

// The forward of the nb items from item b0 on, of a batch of B items with rows T apart: every launch of `ECAPA_TDNN.forward` from
// get_feat's input on.  The uniform call makes one pass over the whole batch (b0 = 0, nb = B); the ragged one makes a pass per kSpItems
// items, `lens` holding theirs.
template <class LN>
void sp_run(us_speaker* h, hipStream_t s, const float* hidden_states, int L, int B, int T, int b0, int nb, const LN& lens, float* base,
            const SpPlan& p, float* emb_out) {
  const auto& c = h->cfg;
  const int ch = c.channels, F = c.feat_dim;
  const long long ct = (long long)ch * T;
  const size_t o = (size_t)b0;                                  // every buffer is [B][...]: this pass works on its items' part
  auto W = [&](const std::string& k) { return h->w.at(k).dev; };
  // get_feat (:261-271)
  float* X0 = base + p.x0 + o * F * T;
  if (L > 0) {
    hipLaunchKernelGGL((sp_combine_kernel<LN>), dim3((F + kCmbC - 1) / kCmbC, (T + kCmbT - 1) / kCmbT, nb), dim3(256), 0, s,
                       hidden_states + o * T * F, h->lw, X0, L, B, T, F, lens);
    hipLaunchKernelGGL((sp_instnorm_kernel<LN>), sp_rows_grid<LN>(nb, F), dim3(256), 0, s, X0, X0, F, nb * F, T, lens);
  } else {
    hipLaunchKernelGGL((sp_instnorm_kernel<LN>), sp_rows_grid<LN>(nb, F), dim3(256), 0, s, hidden_states + o * F * T, X0, F, nb * F, T, lens);
  }
  float* O1 = base + p.o1 + o * ct;
  float* CAT = base + p.cat + o * 3 * ct;
  float* A = base + p.a + o * ct;
  float* R = base + p.r + o * ct;
  float* Y = base + p.y + o * ct;
  float* MEAN = base + p.mean + o * ch;
  float* S = base + p.s + o * ch;
  sp_conv(h, s, "layer1.conv", "layer1.bn", kActRelu, X0, (long long)F * T, O1, ct, nullptr, nb, T, lens);
  static const int dils[3] = {2, 3, 4};                       // :225-227
  for (int blk = 0; blk < 3; ++blk) {
    const std::string q = "layer" + std::to_string(blk + 2);
    const float* in = blk == 0 ? O1 : CAT + (size_t)(blk - 1) * ct;
    const long long in_bs = blk == 0 ? ct : 3 * ct;
    sp_conv(h, s, q + ".Conv1dReluBn1.conv", q + ".Conv1dReluBn1.bn", kActRelu, in, in_bs, A, ct, nullptr, nb, T, lens);
    const int dil = dils[blk], TT = kRes2W - 2 * kSpStages * dil;
    const SpRes2& r2 = h->res2.at(q);
    hipLaunchKernelGGL((sp_res2_kernel<LN>), dim3((T + TT - 1) / TT, nb), dim3(512), 2 * (size_t)h->width * kRes2W * sizeof(float), s, A, R, r2.wp,
                       r2.bss, h->width, h->wpad, T, dil, TT, lens);
    sp_conv(h, s, q + ".Conv1dReluBn2.conv", q + ".Conv1dReluBn2.bn", kActRelu, R, ct, Y, ct, nullptr, nb, T, lens);
    hipLaunchKernelGGL((sp_rowmean_kernel<LN>), sp_rows_grid<LN>(nb, ch), dim3(256), 0, s, Y, MEAN, ch, nb * ch, T, lens);
    hipLaunchKernelGGL(sp_se_kernel, dim3(nb), dim3(1024), (size_t)(ch + kSpAtt) * sizeof(float), s, MEAN, W(q + ".SE_Connect.linear1.weight"),
                       W(q + ".SE_Connect.linear1.bias"), W(q + ".SE_Connect.linear2.weight"), W(q + ".SE_Connect.linear2.bias"), S, ch);
    hipLaunchKernelGGL((sp_scale_res_kernel<LN>), dim3((unsigned)std::min<long long>((ct + 255) / 256, 2048), nb), dim3(256), 0, s, Y, S, in,
                       CAT + (size_t)blk * ct, ch, T, in_bs, 3 * ct, lens);
  }
  const long long bt = (long long)kSpOut * T, at = (long long)kSpAtt * T;
  float* BIG = base + p.big + o * bt;
  float* ATT = base + p.att + o * at;
  float* E = base + p.e + o * bt;
  float* CTX = base + p.ctx + o * 2 * kSpOut;
  float* B2 = base + p.b2 + o * kSpAtt;
  float* PRAW = base + p.praw + o * 2 * kSpOut;
  float* PBN = base + p.pbn + o * 2 * kSpOut;
  sp_conv(h, s, "conv", "", kActRelu, CAT, 3 * ct, BIG, bt, nullptr, nb, T, lens);
  const float* bias2 = nullptr;
  if (c.global_context_att) {
    hipLaunchKernelGGL((sp_rowstats_kernel<LN>), sp_rows_grid<LN>(nb, kSpOut), dim3(256), 0, s, BIG, CTX, kSpOut, nb * kSpOut, T, lens);
    hipLaunchKernelGGL(sp_ctx_bias_kernel, dim3(nb), dim3(1024), 0, s, CTX, W("pooling.linear1.weight"), B2, kSpOut);
    bias2 = B2;
  }
  sp_conv(h, s, "pooling.linear1", "", kActTanh, BIG, bt, ATT, at, bias2, nb, T, lens);
  sp_conv(h, s, "pooling.linear2", "", kActNone, ATT, at, E, bt, nullptr, nb, T, lens);
  const SpBn& fb = h->bn.at("bn");
  hipLaunchKernelGGL((sp_pool_kernel<LN>), sp_rows_grid<LN>(nb, kSpOut), dim3(256), 0, s, BIG, E, fb.scale, fb.scale + fb.n, PRAW, PBN, kSpOut,
                     nb * kSpOut, T, lens);
  hipLaunchKernelGGL(sp_linear_kernel, dim3((unsigned)(((long long)nb * c.emb_dim + 3) / 4)), dim3(256), 0, s, PBN, W("linear.weight"),
                     W("linear.bias"), emb_out + o * c.emb_dim, nb, 2 * kSpOut, c.emb_dim);
}

// what the two forward entry points check alike; US_OK: `s` has the derived weight forms enqueued
int sp_forward_checks(us_speaker* h, const std::string& what, int L, int B, int T, void* workspace, size_t workspace_bytes, hipStream_t s) {
  const auto& c = h->cfg;
  if (L != 0 && L != c.n_layers)
    return h->fail(US_EINVAL, what + ": L must be the configuration's n_layers (" + std::to_string(c.n_layers) +
                                  "), or 0 for already combined [B][feat_dim][T] features");
  const long long big = std::max<long long>(std::max(c.feat_dim, 3 * c.channels), kSpOut);
  if ((long long)B * T * big >= (1ll << 31) || B > 65535) return h->fail(US_EINVAL, what + ": B * T * channels too large");
  const int rc = h->all_loaded(what.c_str());
  if (rc != US_OK) return rc;
  if (!workspace || workspace_bytes < us_speaker_workspace_bytes(h, B, T))
    return h->fail(US_EWORKSPACE, what + ": workspace too small (us_speaker_workspace_bytes)");
  if (h->dirty) sp_prepare(h, s);
  return US_OK;
}

}  // namespace
}  // namespace us

extern "C" {

using namespace us;

int us_speaker_create(us_speaker_handle* out, const us_speaker_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_speaker_create: null argument");
  const auto& c = *cfg;
  if (c.feat_dim <= 0 || c.feat_dim > 8192 || c.emb_dim <= 0 || c.emb_dim > 8192 || c.n_layers < 0 || c.n_layers > 64 ||
      c.global_context_att < 0 || c.global_context_att > 1)
    return WeightTable::fail(nullptr, US_EINVAL, "us_speaker_create: bad feat_dim / emb_dim / n_layers / global_context_att");
  if (c.channels <= 0 || c.channels % kSpScale != 0 || c.channels > 64 * kSpScale)
    return WeightTable::fail(nullptr, US_EINVAL, "us_speaker_create: channels must be a multiple of 8, at most 512 (a Res2 chunk of 64 "
                                                 "channels is what the chained kernel holds in LDS)");
  auto* h = new us_speaker();
  h->cfg = c;
  h->width = c.channels / kSpScale;
  h->wpad = round_up(h->width, kRes2Co);
  (void)hipGetDevice(&h->device);
  speaker_keys(h);
  *out = h;
  return US_OK;
}

int us_speaker_destroy(us_speaker_handle h) {
  if (!h) return US_OK;
  h->free_weights();
  for (auto& kv : h->conv) kv.second.release();
  for (auto& kv : h->bn)
    if (kv.second.scale) (void)hipFree(kv.second.scale);
  for (auto& kv : h->res2) {
    if (kv.second.wp) (void)hipFree(kv.second.wp);
    if (kv.second.bss) (void)hipFree(kv.second.bss);
  }
  if (h->lw) (void)hipFree(h->lw);
  delete h;
  return US_OK;
}

int us_speaker_num_weights(us_speaker_handle h) { return h ? h->num() : 0; }
const char* us_speaker_weight_key(us_speaker_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_speaker_last_error(us_speaker_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_speaker_load_weight(us_speaker_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  // shortcuts are refused by name, before the key lookup (and after the null-argument check, which find() makes)
  if (h && key && data && shape && std::string(key).find(".shortcut.") != std::string::npos)
    return h->fail(US_ENOKEY, std::string("us_speaker_load_weight: '") + key +
                                  "': SE_Res2Block shortcuts (in_channels != out_channels) are not built");
  Weight* w;
  int rc = WeightTable::find(h, "us_speaker_load_weight", key, data, shape, ndim, &w);
  if (rc != US_OK) return rc;
  hipError_t e;
  if (!h->allocated && (e = sp_alloc(h)) != hipSuccess) return h->hip("us_speaker_load_weight: hipMalloc", e);
  if ((rc = h->copy(*w, data, static_cast<hipStream_t>(stream))) != US_OK) return rc;      // sp_alloc made w->dev: no allocation here
  w->loaded = true;
  h->dirty = true;
  return US_OK;
}

size_t us_speaker_workspace_bytes(us_speaker_handle h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  return sp_plan(h->cfg, B, T).total * sizeof(float) + 256;
}

int us_speaker_forward(us_speaker_handle h, const float* hidden_states, int L, int B, int T, float* emb_out, int normalize, void* workspace,
                       size_t workspace_bytes, us_stream stream) {
  if (!h || !hidden_states || !emb_out || B <= 0 || T <= 0 || L < 0) return WeightTable::fail(h, US_EINVAL, "us_speaker_forward: bad argument");
  if (normalize && B != 1) return h->fail(US_EINVAL, "us_speaker_forward: normalize divides the whole output by its norm and is defined for B = 1");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = sp_forward_checks(h, "us_speaker_forward", L, B, T, workspace, workspace_bytes, s);
  if (rc != US_OK) return rc;
  sp_run(h, s, hidden_states, L, B, T, 0, B, SameT{}, ws_align(workspace), sp_plan(h->cfg, B, T), emb_out);
  if (normalize) hipLaunchKernelGGL(sp_normalize_kernel, dim3(1), dim3(256), 0, s, emb_out, B * h->cfg.emb_dim);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_speaker_forward", e);
}

int us_speaker_forward_lengths(us_speaker_handle h, const float* hidden_states, int L, int B, int Tmax, const int64_t* lengths, float* emb_out,
                               int normalize, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!h || !hidden_states || !emb_out || B <= 0 || Tmax <= 0 || L < 0)
    return WeightTable::fail(h, US_EINVAL, "us_speaker_forward_lengths: bad argument");
  if (!lengths) return h->fail(US_EINVAL, "us_speaker_forward_lengths: lengths is null (B host values in [1, Tmax]; us_speaker_forward is the uniform call)");
  const std::string bad = bad_length("us_speaker_forward_lengths", lengths, B, 1, Tmax);
  if (!bad.empty()) return h->fail(US_EINVAL, bad + " must be at least 1 and at most Tmax = " + std::to_string(Tmax));
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = sp_forward_checks(h, "us_speaker_forward_lengths", L, B, Tmax, workspace, workspace_bytes, s);
  if (rc != US_OK) return rc;
  const SpPlan p = sp_plan(h->cfg, B, Tmax);
  float* base = ws_align(workspace);
  for_item_groups<kSpItems>(B, [&](int b) { return lengths[b]; }, [&](int b0, int nb, const ItemLens<kSpItems>& lens, int) {
    sp_run(h, s, hidden_states, L, B, Tmax, b0, nb, lens, base, p, emb_out);
  });
  if (normalize) hipLaunchKernelGGL(sp_normalize_kernel, dim3(B), dim3(256), 0, s, emb_out, h->cfg.emb_dim);      // each row by its own norm
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_speaker_forward_lengths", e);
}

int us_speaker_debug_conv(us_speaker_handle h, const char* prefix, const char* bn_prefix, int act, const float* in, int64_t in_bs, float* out,
                          int64_t out_bs, const float* bias2, int B, int T, us_stream stream) {
  if (!h || !prefix || !in || !out || B <= 0 || T <= 0 || (act != kActNone && act != kActRelu && act != kActTanh))
    return WeightTable::fail(h, US_EINVAL, "us_speaker_debug_conv: bad argument");
  const std::string p(prefix), bn(bn_prefix ? bn_prefix : "");
  const auto ci = h->conv.find(p);
  if (ci == h->conv.end()) return h->fail(US_ENOKEY, "us_speaker_debug_conv: unknown convolution '" + p + "'");
  const PlanarConv& c = ci->second;
  if (!bn.empty()) {
    const auto bi = h->bn.find(bn);
    if (bi == h->bn.end()) return h->fail(US_ENOKEY, "us_speaker_debug_conv: unknown folded BatchNorm '" + bn + "'");
    if (bi->second.n < c.cout) return h->fail(US_EINVAL, "us_speaker_debug_conv: BatchNorm '" + bn + "' has fewer channels than '" + p + "'");
  }
  if ((long long)std::max(c.cin, c.cout) * T >= (1ll << 31) || B > 65535)
    return h->fail(US_EINVAL, "us_speaker_debug_conv: B or channels * T too large");
  if (in_bs < (long long)c.cin * T || out_bs < (long long)c.cout * T)
    return h->fail(US_EINVAL, "us_speaker_debug_conv: a batch stride is shorter than the tensor (in_bs >= Cin * T, out_bs >= Cout * T)");
  const int rc = h->all_loaded("us_speaker_debug_conv");
  if (rc != US_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->dirty) sp_prepare(h, s);
  sp_conv(h, s, p, bn, act, in, in_bs, out, out_bs, bias2, B, T, SameT{});
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_speaker_debug_conv", e);
}

int us_speaker_stage(us_speaker_handle h, int stage, int B, int T, void* workspace, size_t workspace_bytes, const float** data, int64_t* shape) {
  if (!h || !data || !shape || B <= 0 || T <= 0) return WeightTable::fail(h, US_EINVAL, "us_speaker_stage: bad argument");
  if (!workspace || workspace_bytes < us_speaker_workspace_bytes(h, B, T))
    return h->fail(US_EWORKSPACE, "us_speaker_stage: workspace too small (us_speaker_workspace_bytes)");
  const SpPlan p = sp_plan(h->cfg, B, T);
  const float* base = ws_align(workspace);
  shape[0] = B;
  shape[2] = T;
  switch (stage) {
    case US_SPEAKER_STAGE_FEAT: *data = base + p.x0; shape[1] = h->cfg.feat_dim; break;
    case US_SPEAKER_STAGE_LAYER1: *data = base + p.o1; shape[1] = h->cfg.channels; break;
    case US_SPEAKER_STAGE_BLOCKS: *data = base + p.cat; shape[1] = 3 * h->cfg.channels; break;
    case US_SPEAKER_STAGE_POOLING: *data = base + p.praw; shape[1] = 2 * kSpOut; shape[2] = 1; break;
    default: return h->fail(US_EINVAL, "us_speaker_stage: unknown stage");
  }
  return US_OK;
}

}  // extern "C"
