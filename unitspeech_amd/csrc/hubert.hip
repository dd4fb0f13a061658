// HuBERT encoder, eval-mode forward (transformers.HubertModel with the group-norm extractor and post-LN layers; fairseq's
// extract_features(output_layer = n)): 16 kHz waveform [B][Tmax] with per-item lengths -> dense features [B][F][H], fp32 storage and exact-fp32
// products (v_mfma_f32_32x32x2_f32 in the GEMMs, v_mfma_f32_16x16x4_f32 in attention) throughout.
//
// Activations are planar [B][C][T] (time contiguous); the result and the optional hidden states are channel-last [B][F][H].  Every buffer
// holds 0 at and past an item's valid length of that stage, so a kernel that looks across time (the positional convolution) sees zeros there.
// The launches of one call:
//  - hb_wavstats_kernel (normalize only): mean and 1 / sqrt(var + 1e-5) of an item's own samples, two-pass.
//  - hb_conv0_kernel: extractor layer 0 (Cin = 1) on the vector units, one output step per lane, the weights wave-uniform.
//  - hb_gn_gelu_kernel: GroupNorm(C, C) + GELU in place, one workgroup per (item, channel) row: mean, then centred squares.
//  - hb_gemm_kernel<STRIDE>: every other product as conv1d_planar.h's implicit GEMM: the strided extractor layers (STRIDE = the layer's,
//    GELU), the feature projection, the grouped positional convolution (a group is an ordinary convolution over its own H / g channels; bias,
//    GELU, + residual), the fused QKV projection (q rows scaled by d^-1/2), out_proj, and the two feed-forward layers (GELU on the first).
//  - hb_ln_kernel: LayerNorm over the channel axis of a planar tensor with the residual add in front, 32 columns x 32 channel slices per
//    workgroup, fixed-order two-pass; it also writes the channel-last copies (hidden state, result) through an LDS transpose.
//  - hb_attn_kernel<DT>: softmax(Q^T K) V per (item, head, 64-query tile) with an online softmax: key / value tiles of 64 streamed through
//    LDS, running maximum and sum in registers, scores of keys at or past the item's frames set to -inf, tiles without a live key skipped.
// Every reduction has a fixed order and no tile depends on the batch: an item alone or in a batch, and repeated calls, give the same bits.
//
// The WavLM encoder (transformers.WavLMModel; us_wavlm_*) runs on the same kernels and host schedule.  Its large form has a layer-norm extractor
// (every layer: convolution + bias, hb_ln_kernel over the channels with GELU) and a pre-LN encoder (x + attn(LN(x)), h + ffn(LN(h)), the residual
// added in the GEMM's epilogue; hidden state i < L is the un-normalised stream, copied channel-last by hb_export_kernel, hidden state L is
// encoder.layer_norm of it); its base form is HuBERT's schedule.  Both add the gated relative position bias in attention:
//  - wl_gate_kernel: gate[item][head][frame] from gru_rel_pos_linear of the head's own channels of the attention's input.
//  - wl_table_kernel (once per weight load): table[head][delta + D] = rel_attn_embed[bucket(delta)][head] over delta in [-D, D], D the first
//    saturated distance of the host-made bucket map; wl_attn_kernel<DT> adds gate[q] * table[head][clamp(key - q)] to each score.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"
#include "conv1d_planar.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"
#include "whisper_encoder.h"

namespace us {
namespace {

constexpr int kHbItems = 32;        // batch items per launch (item_lens.h)
constexpr int kHbMaxConv = US_HUBERT_MAX_CONV;
constexpr int kHbMaxK0 = 16;        // taps of layer 0 held in registers

struct HbLens : ItemLens<kHbItems> {                // n[]: samples per item
  int k[kHbMaxConv], s[kHbMaxConv];
};
static_assert(sizeof(HbLens) == (kHbItems + 2 * kHbMaxConv) * sizeof(int), "n[], k[], s[] in this order: a kernel's argument segment");

// item b's valid length after `level` extractor layers (0: samples)
__device__ __forceinline__ int hb_len(const HbLens& L, int b, int level) {
  int n = L.n[b];
  for (int i = 0; i < level; ++i) n = (n - L.k[i]) / L.s[i] + 1;
  return n;
}

__device__ __forceinline__ float hb_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

// the workgroup's sum of one value per thread in a fixed order (waves in index order); every thread gets it.  `red`: one float per wave
__device__ __forceinline__ float hb_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float t = 0.f;
  for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += red[w];
  return t;
}

// ---- the reader's F.layer_norm(x, x.shape): stats[b] = {mean, 1 / sqrt(biased var + 1e-5)} over the item's own samples -------------------------
__global__ __launch_bounds__(1024) void hb_wavstats_kernel(const float* __restrict__ wav, float* __restrict__ stats, HbLens lens, int Tmax) {
  __shared__ float red[16];
  const int b = blockIdx.x, n = lens.n[b];
  const float* x = wav + (size_t)b * Tmax;
  float s = 0.f;
  for (int t = threadIdx.x; t < n; t += 1024) s += x[t];
  const float mean = hb_block_sum(s, red) / (float)n;
  float v = 0.f;
  for (int t = threadIdx.x; t < n; t += 1024) {
    const float d = x[t] - mean;
    v = fmaf(d, d, v);
  }
  const float var = hb_block_sum(v, red) / (float)n;
  if (threadIdx.x == 0) {
    stats[2 * b] = mean;
    stats[2 * b + 1] = 1.f / sqrtf(var + 1e-5f);
  }
}

// ---- extractor layer 0: out[b][c][q] = (bias[c] +) sum_j w[c][j] * x[b][s q + j], x = (wav - mean) * rstd; 0 at and past the item's steps ------
__global__ __launch_bounds__(256) void hb_conv0_kernel(const float* __restrict__ wav, const float* __restrict__ stats, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ out, HbLens lens, int Tmax, int C, int T1) {
  const int b = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
  if (q >= T1) return;
  const int k = lens.k[0], s = lens.s[0];
  const bool live = q < hb_len(lens, b, 1);
  const float mean = stats ? stats[2 * b] : 0.f, rs = stats ? stats[2 * b + 1] : 1.f;
  const float* x = wav + (size_t)b * Tmax + (size_t)q * s;
  float xr[kHbMaxK0];
#pragma unroll
  for (int j = 0; j < kHbMaxK0; ++j) xr[j] = (live && j < k) ? (x[j] - mean) * rs : 0.f;
  float* o = out + (size_t)b * C * T1 + q;
  for (int c = 0; c < C; ++c) {
    const float* wc = w + (size_t)c * k;
    float a = 0.f;
#pragma unroll
    for (int j = 0; j < kHbMaxK0; ++j)
      if (j < k) a = fmaf(wc[j], xr[j], a);
    o[(size_t)c * T1] = bias && live ? a + bias[c] : a;
  }
}

// ---- GroupNorm(C, C) + GELU in place: per (item, channel) row over the item's valid steps, biased variance, eps 1e-5 -----------------------------
__global__ __launch_bounds__(256) void hb_gn_gelu_kernel(float* __restrict__ x, const float* __restrict__ gamma, const float* __restrict__ beta,
                                                         HbLens lens, int C, int T1) {
  __shared__ float red[4];
  const int b = blockIdx.y, c = blockIdx.x, n = hb_len(lens, b, 1);
  float* r = x + ((size_t)b * C + c) * T1;
  float s = 0.f;
  for (int t = threadIdx.x; t < n; t += 256) s += r[t];
  const float mean = hb_block_sum(s, red) / (float)n;
  float v = 0.f;
  for (int t = threadIdx.x; t < n; t += 256) {
    const float d = r[t] - mean;
    v = fmaf(d, d, v);
  }
  const float rs = 1.f / sqrtf(hb_block_sum(v, red) / (float)n + 1e-5f);
  const float g = gamma[c], be = beta[c];
  for (int t = threadIdx.x; t < n; t += 256) r[t] = hb_gelu(fmaf((r[t] - mean) * rs, g, be));
}

// ---- implicit-GEMM convolution (conv1d_planar.h's main loop, 64 channels x 64 steps per workgroup) -----------------------------------------
// out[b][G Cout + co][t] = post(bias + sum_{j, ci} P_G[j * Cin + ci][co] * in[b][G Cin + ci][STRIDE * t + off + j]) for t below the item's length
// at `level`, 0 from there to Tout.  post: rows below nscale times scale, GELU, + res.  blockIdx.y = group * mtiles + channel tile.
struct HbGemmArgs {
  const float* in;
  const float* w;             // [groups][Kpad][ldw]
  const float* bias;          // [groups * Cout] or null
  const float* res;           // planar like out, or null
  float* out;
  long long in_bs, out_bs, res_bs;
  int Cin, Cout, Tin, Tout, off, Kdim, Kpad, ldw;
  int gelu, nscale, mtiles, level;
  float scale;
};

template <int STRIDE>
__global__ __launch_bounds__(256) void hb_gemm_kernel(HbGemmArgs a, HbLens lens) {
  PLANAR_LANE(threadIdx.x);
  const int b = blockIdx.z, grp = blockIdx.y / a.mtiles, mt = blockIdx.y - grp * a.mtiles;
  const int m0 = mt * kPcBM, n0 = blockIdx.x * 64;
  f32x16 acc[1][2];
  planar_conv_mainloop<1, 2, STRIDE>({a.in + (size_t)b * a.in_bs + (size_t)grp * a.Cin * a.Tin, a.w + (size_t)grp * a.Kpad * a.ldw, a.Cin, a.Tin, 1,
                                      a.off, a.Kdim, a.Kpad, a.ldw, m0, n0},
                                     acc);
  const int t = PLANAR_STEP(1, n0, 0);
  if (t >= a.Tout) return;
  const bool live = t < hb_len(lens, b, a.level);
  float* __restrict__ out = a.out + (size_t)b * a.out_bs;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int cg = PLANAR_CHANNEL(m0, r);
    if (cg >= a.Cout) continue;
    const int co = grp * a.Cout + cg;
    float v = acc[0][0][r] + acc[0][1][r];
    if (a.bias) v += a.bias[co];
    if (co < a.nscale) v *= a.scale;
    if (a.gelu) v = hb_gelu(v);
    if (a.res) v += a.res[(size_t)b * a.res_bs + (size_t)co * a.Tout + t];
    out[(size_t)co * a.Tout + t] = live ? v : 0.f;
  }
}

// ---- LayerNorm over the channel axis of a planar tensor, residual in front ---------------------------------------------------------------------
// y[c][t] = ((x[c][t] + res[c][t]) - mean_t) * rstd_t * gamma[c] + beta[c] for t below the item's frames, 0 past them.  A workgroup is 32
// columns (tid & 31) x 32 channel slices (tid >> 5): slice s adds up channels s, s + 32, ... in order, the 32 partials of a column are then
// added in slice order.  e1 / e2 (optional): the same values channel-last, [T][C] per item, written 32 x 32 through LDS.  gelu: GELU
// after the affine (the layer-norm extractor's layers).
constexpr int kLnCols = 32, kLnSlices = 32;

__global__ __launch_bounds__(1024) void hb_ln_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ e1,
                                                     float* __restrict__ e2, long long e1_bs, long long e2_bs, HbLens lens, int level, int C,
                                                     int T, float eps, int gelu) {
  __shared__ float red[kLnSlices][kLnCols];
  __shared__ float tile[kLnCols][kLnSlices + 1];
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int b = blockIdx.y, t0 = blockIdx.x * kLnCols, t = t0 + col;
  const int n = hb_len(lens, b, level);
  const bool in = t < T, live = t < n;
  const size_t bo = (size_t)b * C * T;
  auto at = [&](int c) {
    const size_t i = bo + (size_t)c * T + t;
    return res ? x[i] + res[i] : x[i];
  };
  auto column_sum = [&](float v) {
    __syncthreads();
    red[sl][col] = v;
    __syncthreads();
    float s = 0.f;
#pragma unroll 8
    for (int i = 0; i < kLnSlices; ++i) s += red[i][col];
    return s;
  };
  float s = 0.f;
  if (live)
    for (int c = sl; c < C; c += kLnSlices) s += at(c);
  const float mean = column_sum(s) / (float)C;
  float v = 0.f;
  if (live)
    for (int c = sl; c < C; c += kLnSlices) {
      const float d = at(c) - mean;
      v = fmaf(d, d, v);
    }
  const float rs = 1.f / sqrtf(column_sum(v) / (float)C + eps);
  const int tr = threadIdx.x >> 5, cr = threadIdx.x & 31;      // the transposed read: row (time) tr, channel cr of the 32 x 32 tile
  for (int c0 = 0; c0 < C; c0 += kLnSlices) {
    const int c = c0 + sl;
    float o = 0.f;
    if (live && c < C) {
      o = fmaf((at(c) - mean) * rs, gamma[c], beta[c]);
      if (gelu) o = hb_gelu(o);
    }
    if (y && in && c < C) y[bo + (size_t)c * T + t] = o;
    if (e1 || e2) {
      __syncthreads();
      tile[col][sl] = o;
      __syncthreads();
      if (t0 + tr < T && c0 + cr < C) {
        const float q = tile[tr][cr];
        const size_t i = (size_t)(t0 + tr) * C + c0 + cr;
        if (e1) e1[(size_t)b * e1_bs + i] = q;
        if (e2) e2[(size_t)b * e2_bs + i] = q;
      }
    }
  }
}

// ---- the channel-last copy of a planar tensor (the pre-LN encoder's un-normalised hidden states), 32 x 32 through LDS --------------------------
// e1 / e2 [T][C] per item from x [C][T]; x already holds 0 past the item's frames.  grid: (time tiles, channel tiles, items)
__global__ __launch_bounds__(1024) void hb_export_kernel(const float* __restrict__ x, float* __restrict__ e1, float* __restrict__ e2, long long e1_bs,
                                                         long long e2_bs, int C, int T) {
  __shared__ float tile[kLnCols][kLnSlices + 1];
  const int col = threadIdx.x & 31, sl = threadIdx.x >> 5;
  const int b = blockIdx.z, t0 = blockIdx.x * kLnCols, c0 = blockIdx.y * kLnSlices;
  tile[col][sl] = (t0 + col < T && c0 + sl < C) ? x[(size_t)b * C * T + (size_t)(c0 + sl) * T + t0 + col] : 0.f;
  __syncthreads();
  if (t0 + sl < T && c0 + col < C) {
    const float q = tile[sl][col];
    const size_t i = (size_t)(t0 + sl) * C + c0 + col;
    if (e1) e1[(size_t)b * e1_bs + i] = q;
    if (e2) e2[(size_t)b * e2_bs + i] = q;
  }
}

// ---- WavLM's gate of the relative position bias, per (item, head, frame) ---------------------------------------------------------------------
// p = w x_head + bias (8 values from the head's own d channels of the attention's input x [H][F]), a = sigmoid(p0 + p1 + p2 + p3),
// b = sigmoid(p4 + .. + p7), gate = a (b cst[head] - 1) + 2.  One frame per lane, the channels in index order.  grid: (frame tiles, heads, items)
__global__ __launch_bounds__(256) void wl_gate_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      const float* __restrict__ cst, float* __restrict__ gate, int H, int d, int F) {
  const int b = blockIdx.z, head = blockIdx.y, t = blockIdx.x * 256 + threadIdx.x;
  if (t >= F) return;
  const float* xr = x + ((size_t)b * H + (size_t)head * d) * F + t;
  float p[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) p[j] = bias[j];
#pragma unroll 8
  for (int c = 0; c < d; ++c) {
    const float v = xr[(size_t)c * F];
#pragma unroll
    for (int j = 0; j < 8; ++j) p[j] = fmaf(w[j * d + c], v, p[j]);
  }
  const float ga = 1.f / (1.f + expf(-(((p[0] + p[1]) + p[2]) + p[3])));
  const float gb = 1.f / (1.f + expf(-(((p[4] + p[5]) + p[6]) + p[7])));
  gate[((size_t)b * gridDim.y + head) * F + t] = fmaf(ga, fmaf(gb, cst[head], -1.f), 2.f);
}

// table[h][i] = rel_attn_embed[bucket[i]][h] for i = delta + D in [0, 2 D]
__global__ __launch_bounds__(256) void wl_table_kernel(const float* __restrict__ emb, const int* __restrict__ bucket, float* __restrict__ table,
                                                       int heads, int n) {
  const int i = blockIdx.x * 256 + threadIdx.x, h = blockIdx.y;
  if (i < n) table[(size_t)h * n + i] = emb[(size_t)bucket[i] * heads + h];
}

// ---- attention ---------------------------------------------------------------------------------------------------------------------------------
// qkv [3 H][F] planar per item (q already scaled); head h owns rows [h d, (h + 1) d) of each third.  A workgroup is 64 queries of one (item,
// head), a wave 16 of them.  Per key tile of 64 (through LDS, K as [c][key] with rows of 80 floats, V with rows of 68: both conflict-free
// for the reads below) a wave takes, on v_mfma_f32_16x16x4_f32,
//   S^T[key][q] = sum_c K[c][key] Q[c][q]     A = K^T (lane: key l & 15, c l >> 4), B = Q (registers, loaded once): four 16-key accumulators;
//   O^T[c][q]  += sum_key V[c][key] P^T[key][q]:  a lane's accumulator register r of key block ks IS P^T[16 ks + 4 (l >> 4) + r][q = l & 15],
//                 the B operand of a k-step whose four keys are {16 ks + 4 g + r : g = l >> 4}; A reads V at those same keys (one float4).
// So the probabilities never leave their registers.  The head dimension is padded to 16 DT with zero rows (d = 20: DT = 2).
// BIAS (WavLM): the score gets + gate[q] * table[head][clamp(key - q, -D, D) + D] before the masking and the running maximum.  The 127
// differences a 64 x 64 tile can hold are staged per key tile in two more rows of Ks; the gate is one register per lane.
constexpr int kAtQ = 64, kAtK = 64, kAtKs = 80, kAtVs = 68;

template <int DT, bool BIAS>
__device__ __forceinline__ void hb_attn_body(const float* __restrict__ qkv, float* __restrict__ out, HbLens lens, int level, int H, int d,
                                             int F, long long qkv_bs, long long out_bs, const float* __restrict__ gate,
                                             const float* __restrict__ table, int D) {
  __shared__ float Ks[16 * DT + (BIAS ? 2 : 0)][kAtKs];
  __shared__ __attribute__((aligned(16))) float Vs[16 * DT][kAtVs];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const int b = blockIdx.z, head = blockIdx.y, qt0 = blockIdx.x * kAtQ;
  const int n = hb_len(lens, b, level);
  const float* __restrict__ Q = qkv + (size_t)b * qkv_bs + (size_t)head * d * F;
  const float* __restrict__ K = Q + (size_t)H * F;
  const float* __restrict__ V = K + (size_t)H * F;
  float* __restrict__ O = out + (size_t)b * out_bs + (size_t)head * d * F;
  if (qt0 >= n) {                                    // no live query: the rows are 0
    for (int i = tid; i < d * kAtQ; i += 256) {
      const int c = i >> 6, t = qt0 + (i & 63);
      if (t < F) O[(size_t)c * F + t] = 0.f;
    }
    return;
  }
  const int tq = qt0 + wave * 16 + li;
  float qr[4 * DT];
#pragma unroll
  for (int s = 0; s < 4 * DT; ++s) {
    const int c = 4 * s + lg;
    qr[s] = (c < d && tq < n) ? Q[(size_t)c * F + tq] : 0.f;
  }
  float* Bs = &Ks[16 * DT][0];                       // BIAS: table[key - query] for key - query = k0 - qt0 - 63 + i, i < 127
  const float* __restrict__ tab = BIAS ? table + (size_t)head * (2 * D + 1) + D : nullptr;
  const float gq = BIAS && tq < n ? gate[((size_t)b * gridDim.y + head) * F + tq] : 0.f;
  const int bq = 63 - (wave * 16 + li) + lg * 4;
  f32x4 o[DT];
#pragma unroll
  for (int ct = 0; ct < DT; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -INFINITY, l = 0.f;
  const int nkt = (n + kAtK - 1) / kAtK;             // tiles with a live key
  for (int kt = 0; kt < nkt; ++kt) {
    const int k0 = kt * kAtK;
    __syncthreads();
    for (int r = wave; r < 16 * DT; r += 4) {
      const int key = k0 + lane;
      const bool ok = r < d && key < n;
      Ks[r][lane] = ok ? K[(size_t)r * F + key] : 0.f;
      Vs[r][lane] = ok ? V[(size_t)r * F + key] : 0.f;
    }
    if (BIAS && tid < 127) Bs[tid] = tab[max(-D, min(D, k0 - qt0 - 63 + tid))];
    __syncthreads();
    f32x4 s[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) s[ks] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < 4 * DT; ++st)
#pragma unroll
      for (int ks = 0; ks < 4; ++ks) s[ks] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ks[4 * st + lg][ks * 16 + li], qr[st], s[ks], 0, 0, 0);
    float mx = -INFINITY;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (BIAS) s[ks][r] = fmaf(gq, Bs[bq + ks * 16 + r], s[ks][r]);
        if (k0 + ks * 16 + lg * 4 + r >= n) s[ks][r] = -INFINITY;
        mx = fmaxf(mx, s[ks][r]);
      }
    mx = fmaxf(mx, __shfl_xor(mx, 16));
    mx = fmaxf(mx, __shfl_xor(mx, 32));
    const float mn = fmaxf(m, mx);                   // finite: the tile has a live key
    const float alpha = expf(m - mn);
    m = mn;
    float ps = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        s[ks][r] = expf(s[ks][r] - mn);
        ps += s[ks][r];
      }
    l = fmaf(l, alpha, ps);                          // this lane's share of the row sum; the four shares meet after the last tile
#pragma unroll
    for (int ct = 0; ct < DT; ++ct) o[ct] *= alpha;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      f32x4 v4[DT];
#pragma unroll
      for (int ct = 0; ct < DT; ++ct) v4[ct] = *reinterpret_cast<const f32x4*>(&Vs[ct * 16 + li][ks * 16 + lg * 4]);
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int ct = 0; ct < DT; ++ct) o[ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(v4[ct][r], s[ks][r], o[ct], 0, 0, 0);
    }
  }
  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (tq >= F) return;
  const float inv = tq < n ? 1.f / l : 0.f;
#pragma unroll
  for (int ct = 0; ct < DT; ++ct)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int c = ct * 16 + lg * 4 + r;
      if (c < d) O[(size_t)c * F + tq] = o[ct][r] * inv;
    }
}

template <int DT>
__global__ __launch_bounds__(256) void hb_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, HbLens lens, int level, int H, int d,
                                                      int F, long long qkv_bs, long long out_bs) {
  hb_attn_body<DT, false>(qkv, out, lens, level, H, d, F, qkv_bs, out_bs, nullptr, nullptr, 0);
}

// the bias variant is held to four waves per SIMD (hb_attn_kernel<4>'s occupancy): left alone it takes 119 + 16 registers at DT = 4 and runs three
template <int DT>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4))) void wl_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out,
                                                                                                HbLens lens, int level, int H, int d, int F,
                                                                                                long long qkv_bs, long long out_bs,
                                                                                                const float* __restrict__ gate,
                                                                                                const float* __restrict__ table, int D) {
  hb_attn_body<DT, true>(qkv, out, lens, level, H, d, F, qkv_bs, out_bs, gate, table, D);
}

struct HbLayer {
  PlanarConv qkv, out, ff1, ff2;
  float* qkv_w = nullptr;     // [3 H][H]: q | k | v
  float* qkv_b = nullptr;     // [3 H]
};

// what us_hubert and us_wavlm share: the configuration, the weight table and the packed GEMM operands
struct HbModel : WeightTable {
  us_hubert_config cfg{};
  const char* abi = "us_hubert";           // the prefix of the entry points' names in messages
  int d = 0, cg = 0;                       // head dimension; channels per positional-convolution group
  std::vector<PlanarConv> ext;             // extractor layers 1 .. n_conv - 1 (index i - 1)
  PlanarConv proj, pos;                    // pos: one group's geometry, `packed` holds all groups
  std::vector<HbLayer> layers;
  bool allocated = false;                  // device tensors exist (made by the first load, so creating a handle touches no device)
  bool dirty = true;                       // a weight changed since the derived forms were made
  // WavLM only
  bool wavlm = false;
  int conv_bias = 0, num_buckets = 0, max_distance = 0;
  int D = 0;                               // the first saturated distance: bucket(delta) is constant for |delta| >= D on either side
  std::vector<int> bucket;                 // bucket(delta) for delta = i - D, i in [0, 2 D]
  int* bucket_dev = nullptr;
  float* table = nullptr;                  // [heads][2 D + 1]: rel_attn_embed[bucket(delta)][head]
  bool layer_ext() const { return cfg.feat_extract_norm == US_HUBERT_NORM_LAYER; }
  bool pre_ln() const { return cfg.do_stable_layer_norm != 0; }
};

}  // namespace
}  // namespace us

struct us_hubert : us::HbModel {};
struct us_wavlm : us::HbModel {};

namespace us {
namespace {

std::string hb_conv_key(int i) { return "feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight"; }
std::string hb_conv_prefix(int i) { return "feature_extractor.conv_layers." + std::to_string(i) + "."; }
std::string hb_layer_key(int i) { return "encoder.layers." + std::to_string(i) + "."; }

void hb_add_affine(HbModel* h, const std::string& p, int n) {
  h->add(p + ".weight", {n});
  h->add(p + ".bias", {n});
}
void hb_add_linear(HbModel* h, const std::string& p, int out, int in) {
  h->add(p + ".weight", {out, in});
  h->add(p + ".bias", {out});
}

// transformers.HubertModel's / WavLMModel's registration order (the positional convolution's weight in its folded form: g v / |v|)
void hubert_keys(HbModel* h) {
  const auto& c = h->cfg;
  const int H = c.hidden_size, I = c.intermediate_size, Cl = c.conv_dim[c.n_conv - 1];
  for (int i = 0; i < c.n_conv; ++i) {
    h->add(hb_conv_key(i), {c.conv_dim[i], i ? c.conv_dim[i - 1] : 1, c.conv_kernel[i]});
    if (h->conv_bias) h->add(hb_conv_prefix(i) + "conv.bias", {c.conv_dim[i]});
    if (i == 0 || h->layer_ext()) hb_add_affine(h, hb_conv_prefix(i) + "layer_norm", c.conv_dim[i]);
  }
  hb_add_affine(h, "feature_projection.layer_norm", Cl);
  hb_add_linear(h, "feature_projection.projection", H, Cl);
  h->add("encoder.pos_conv_embed.conv.bias", {H});
  h->add("encoder.pos_conv_embed.conv.weight", {H, h->cg, c.pos_conv_kernel});
  hb_add_affine(h, "encoder.layer_norm", H);
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = hb_layer_key(i);
    if (h->wavlm) h->add(p + "attention.gru_rel_pos_const", {1, c.n_heads, 1, 1});
    for (const char* n : {"k_proj", "v_proj", "q_proj", "out_proj"}) hb_add_linear(h, p + "attention." + n, H, H);
    if (h->wavlm) {
      hb_add_linear(h, p + "attention.gru_rel_pos_linear", 8, h->d);
      if (i == 0) h->add(p + "attention.rel_attn_embed.weight", {h->num_buckets, c.n_heads});
    }
    hb_add_affine(h, p + "layer_norm", H);
    hb_add_linear(h, p + "feed_forward.intermediate_dense", I, H);
    hb_add_linear(h, p + "feed_forward.output_dense", H, I);
    hb_add_affine(h, p + "final_layer_norm", H);
  }
}

void hb_geometry(HbModel* h) {
  const auto& c = h->cfg;
  const int H = c.hidden_size, I = c.intermediate_size;
  h->ext.resize(c.n_conv - 1);
  for (int i = 1; i < c.n_conv; ++i) {
    h->ext[i - 1].conv(c.conv_dim[i - 1], c.conv_dim[i - 1], c.conv_dim[i], c.conv_kernel[i], 1);
    h->ext[i - 1].off[0] = 0;                                     // no padding: step q reads s q + j
  }
  h->proj.conv(c.conv_dim[c.n_conv - 1], c.conv_dim[c.n_conv - 1], H, 1, 1);
  h->pos.conv(h->cg, h->cg, h->cg, c.pos_conv_kernel, 1);
  h->pos.off[0] = -(c.pos_conv_kernel / 2);                       // padding k / 2; an even k's extra last step is never computed
  h->layers.resize(c.n_layers);
  for (auto& l : h->layers) {
    l.qkv.conv(H, H, 3 * H, 1, 1);
    l.out.conv(H, H, H, 1, 1);
    l.ff1.conv(H, H, I, 1, 1);
    l.ff2.conv(I, I, H, 1, 1);
  }
}

// WavLM's T5-style bucket of delta = key - query: num_buckets / 2 per sign, exact below num_buckets / 4, logarithmic up to max_distance,
// clamped to the last bucket from there
int wl_bucket(int num_buckets, int max_distance, long long delta) {
  const int nb = num_buckets / 2, max_exact = nb / 2;
  const int r = delta > 0 ? nb : 0;
  const long long a = delta < 0 ? -delta : delta;
  if (a < max_exact) return r + (int)a;
  const double v = std::log((double)a / max_exact) / std::log((double)max_distance / max_exact) * (nb - max_exact);
  return r + (int)std::min<long long>(max_exact + (long long)v, nb - 1);
}

// the delta -> bucket map over [-D, D], D the first distance whose bucket is the last one (at most max_distance)
void wl_bucket_map(HbModel* h) {
  int D = 0;
  while (D < h->max_distance && wl_bucket(h->num_buckets, h->max_distance, -D) != h->num_buckets / 2 - 1) ++D;
  h->D = D;
  h->bucket.resize(2 * D + 1);
  for (int i = 0; i <= 2 * D; ++i) h->bucket[i] = wl_bucket(h->num_buckets, h->max_distance, i - D);
}

// every tensor the forward reads, at once: after the first load neither a load nor a forward allocates
hipError_t hb_alloc(HbModel* h) {
  hipError_t e = hipSuccess;
  auto alloc = [&](float** p, size_t n) {
    if (e == hipSuccess && !*p) e = hipMalloc(p, std::max<size_t>(n, 1) * sizeof(float));
  };
  const size_t H = (size_t)h->cfg.hidden_size;
  for (auto& kv : h->w) alloc(&kv.second.dev, kv.second.numel());
  for (auto& c : h->ext) alloc(&c.packed, c.packed_floats());
  alloc(&h->proj.packed, h->proj.packed_floats());
  alloc(&h->pos.packed, h->pos.packed_floats() * h->cfg.pos_conv_groups);
  for (auto& l : h->layers) {
    alloc(&l.qkv.packed, l.qkv.packed_floats());
    alloc(&l.out.packed, l.out.packed_floats());
    alloc(&l.ff1.packed, l.ff1.packed_floats());
    alloc(&l.ff2.packed, l.ff2.packed_floats());
    alloc(&l.qkv_w, 3 * H * H);
    alloc(&l.qkv_b, 3 * H);
  }
  if (h->wavlm) {
    const size_t n = h->bucket.size();
    alloc(&h->table, n * h->cfg.n_heads);
    if (e == hipSuccess && !h->bucket_dev) e = hipMalloc(&h->bucket_dev, n * sizeof(int));
    if (e == hipSuccess) e = hipMemcpy(h->bucket_dev, h->bucket.data(), n * sizeof(int), hipMemcpyHostToDevice);
  }
  h->allocated = e == hipSuccess;
  return e;
}

// the packed GEMM weights (and the q | k | v concatenation, and WavLM's per-head bias table) from the loaded tensors
hipError_t hb_prepare(HbModel* h, hipStream_t s) {
  auto W = [&](const std::string& k) { return h->w.at(k).dev; };
  const auto& c = h->cfg;
  const size_t H = (size_t)c.hidden_size;
  for (int i = 1; i < c.n_conv; ++i) h->ext[i - 1].pack(W(hb_conv_key(i)), s);
  h->proj.pack(W("feature_projection.projection.weight"), s);
  const PlanarConv& p = h->pos;
  for (int g = 0; g < c.pos_conv_groups; ++g)
    hipLaunchKernelGGL(planar_conv_pack_kernel, dim3((unsigned)std::min<size_t>((p.packed_floats() + 255) / 256, 4096)), dim3(256), 0, s,
                       W("encoder.pos_conv_embed.conv.weight") + (size_t)g * h->cg * h->cg * c.pos_conv_kernel, p.packed + (size_t)g * p.packed_floats(),
                       p.cin, p.cin_tot, p.cout, p.k, 0, 0, p.taps, p.Kpad, p.ldw, 1);
  for (int i = 0; i < c.n_layers; ++i) {
    HbLayer& l = h->layers[i];
    const std::string a = hb_layer_key(i) + "attention.";
    const char* names[3] = {"q_proj", "k_proj", "v_proj"};
    for (int j = 0; j < 3; ++j) {
      hipError_t e = hipMemcpyAsync(l.qkv_w + j * H * H, W(a + names[j] + ".weight"), H * H * sizeof(float), hipMemcpyDeviceToDevice, s);
      if (e == hipSuccess) e = hipMemcpyAsync(l.qkv_b + j * H, W(a + names[j] + ".bias"), H * sizeof(float), hipMemcpyDeviceToDevice, s);
      if (e != hipSuccess) return e;
    }
    l.qkv.pack(l.qkv_w, s);
    l.out.pack(W(a + "out_proj.weight"), s);
    l.ff1.pack(W(hb_layer_key(i) + "feed_forward.intermediate_dense.weight"), s);
    l.ff2.pack(W(hb_layer_key(i) + "feed_forward.output_dense.weight"), s);
  }
  if (h->wavlm && c.n_layers > 0) {
    const int n = 2 * h->D + 1;
    hipLaunchKernelGGL(wl_table_kernel, dim3((n + 255) / 256, c.n_heads), dim3(256), 0, s, W("encoder.layers.0.attention.rel_attn_embed.weight"),
                       h->bucket_dev, h->table, c.n_heads, n);
  }
  h->dirty = false;
  return hipGetLastError();
}

// valid steps after `level` extractor layers of an n-sample item; 0 when it is shorter than the receptive field
long long hb_steps(const us_hubert_config& c, long long n, int level) {
  for (int i = 0; i < level; ++i) {
    if (n < c.conv_kernel[i]) return 0;
    n = (n - c.conv_kernel[i]) / c.conv_stride[i] + 1;
  }
  return n;
}

long long hb_receptive_field(const us_hubert_config& c) {
  long long n = 1;
  for (int i = c.n_conv - 1; i >= 0; --i) n = (n - 1) * c.conv_stride[i] + c.conv_kernel[i];
  return n;
}

struct HbPlan {                 // float offsets into the 256-byte aligned workspace
  size_t stats, a, b, x0, p, x, x1, y, qkv, att, ff, gate, total;
};

HbPlan hb_plan(const HbModel* h, int B, int Tmax) {
  const us_hubert_config& c = h->cfg;
  HbPlan p{};
  WsTake take;
  size_t ea = 0, eb = 0;        // the extractor's two buffers: layer i writes a (i even) or b (i odd); the projection's LayerNorm takes the other
  for (int i = 0; i <= c.n_conv; ++i) {
    const int ch = c.conv_dim[std::min(i, c.n_conv - 1)];
    const size_t n = (size_t)B * ch * (size_t)hb_steps(c, Tmax, std::min(i + 1, c.n_conv));
    (i % 2 == 0 ? ea : eb) = std::max(i % 2 == 0 ? ea : eb, n);
  }
  if (h->layer_ext()) ea = eb = std::max(ea, eb);       // every layer is a convolution into one and a LayerNorm into the other
  const size_t bf = (size_t)B * (size_t)hb_steps(c, Tmax, c.n_conv), H = (size_t)c.hidden_size;
  p.stats = take(2 * (size_t)B);
  p.a = take(ea);
  p.b = take(eb);
  p.x0 = take(bf * H);
  p.p = take(bf * H);
  p.x = take(bf * H);
  p.x1 = take(bf * H);
  p.y = take(bf * H);
  p.qkv = take(bf * 3 * H);
  p.att = take(bf * H);
  p.ff = take(bf * (size_t)c.intermediate_size);
  p.gate = take(h->wavlm ? bf * (size_t)c.n_heads : 0);
  p.total = take.total;
  return p;
}

struct HbGemm {                 // one launch of hb_gemm_kernel
  const PlanarConv* c;
  const float *in, *bias, *res;
  float* out;
  int Tin, Tout, stride = 1, groups = 1, gelu = 0, nscale = 0, level = 0;
  float scale = 1.f;
  long long res_bs = -1;        // the residual's item stride when it is not the output's (0: one tensor for every item)
};

void hb_gemm(hipStream_t s, const HbGemm& g, const HbLens& lens, int nb) {
  const PlanarConv& c = *g.c;
  HbGemmArgs a{};
  a.in = g.in; a.w = c.packed; a.bias = g.bias; a.res = g.res; a.out = g.out;
  a.in_bs = (long long)c.cin * g.groups * g.Tin;
  a.out_bs = a.res_bs = (long long)c.cout * g.groups * g.Tout;
  if (g.res_bs >= 0) a.res_bs = g.res_bs;
  a.Cin = c.cin; a.Cout = c.cout; a.Tin = g.Tin; a.Tout = g.Tout; a.off = c.off[0]; a.Kdim = c.Kdim(); a.Kpad = c.Kpad; a.ldw = c.ldw;
  a.gelu = g.gelu; a.nscale = g.nscale; a.scale = g.scale; a.level = g.level;
  a.mtiles = (c.cout + kPcBM - 1) / kPcBM;
  const dim3 grid((g.Tout + 63) / 64, a.mtiles * g.groups, nb);
  switch (g.stride) {
    case 1: hipLaunchKernelGGL(hb_gemm_kernel<1>, grid, dim3(256), 0, s, a, lens); break;
    case 2: hipLaunchKernelGGL(hb_gemm_kernel<2>, grid, dim3(256), 0, s, a, lens); break;
    case 3: hipLaunchKernelGGL(hb_gemm_kernel<3>, grid, dim3(256), 0, s, a, lens); break;
    default: hipLaunchKernelGGL(hb_gemm_kernel<4>, grid, dim3(256), 0, s, a, lens); break;
  }
}

// gate / table: null for plain attention (HuBERT), else WavLM's gated relative position bias
void hb_attn(hipStream_t s, const float* qkv, float* out, const HbLens& lens, int level, int H, int heads, int d, int F, int nb, const float* gate,
             const float* table, int D) {
  const dim3 grid((F + kAtQ - 1) / kAtQ, heads, nb);
  const long long qb = 3ll * H * F, ob = (long long)H * F;
  const int dt = (d + 15) / 16;
  if (gate) {
    switch (dt) {
      case 1: hipLaunchKernelGGL(wl_attn_kernel<1>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob, gate, table, D); break;
      case 2: hipLaunchKernelGGL(wl_attn_kernel<2>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob, gate, table, D); break;
      case 3: hipLaunchKernelGGL(wl_attn_kernel<3>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob, gate, table, D); break;
      default: hipLaunchKernelGGL(wl_attn_kernel<4>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob, gate, table, D); break;
    }
    return;
  }
  switch (dt) {
    case 1: hipLaunchKernelGGL(hb_attn_kernel<1>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
    case 2: hipLaunchKernelGGL(hb_attn_kernel<2>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
    case 3: hipLaunchKernelGGL(hb_attn_kernel<3>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
    default: hipLaunchKernelGGL(hb_attn_kernel<4>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
  }
}

// the checks us_hubert_create and us_wavlm_create share; "" when the geometry is built
std::string hb_check_geometry(const us_hubert_config& c) {
  if (c.n_conv < 1 || c.n_conv > kHbMaxConv) return "1 to 8 feature-extractor layers";
  for (int i = 0; i < c.n_conv; ++i) {
    if (c.conv_dim[i] < 1 || c.conv_dim[i] > 8192 || c.conv_kernel[i] < 1 || c.conv_kernel[i] > 64 || c.conv_stride[i] < 1)
      return "bad conv_dim / conv_kernel / conv_stride at layer " + std::to_string(i);
    if (i == 0 ? c.conv_kernel[0] > kHbMaxK0 || c.conv_stride[0] > 64 : c.conv_stride[i] > 4)
      return "layer 0 takes at most 16 taps, the others a stride of at most 4";
  }
  if (c.hidden_size < 1 || c.hidden_size > 8192 || c.intermediate_size < 1 || c.intermediate_size > 32768 || c.n_layers < 0 || c.n_layers > 64)
    return "bad hidden_size / intermediate_size / n_layers";
  if (c.n_heads < 1 || c.hidden_size % c.n_heads != 0) return "hidden_size must be divisible by the number of heads";
  const int d = c.hidden_size / c.n_heads;
  if (d > 64 || d % 4 != 0) return "the head dimension must be a multiple of 4, at most 64 (got " + std::to_string(d) + ")";
  if (c.pos_conv_groups < 1 || c.hidden_size % c.pos_conv_groups != 0) return "hidden_size must be divisible by the positional convolution's groups";
  if (c.pos_conv_kernel < 1 || c.pos_conv_kernel > 1024) return "bad positional convolution kernel";
  if (!(c.layer_norm_eps > 0.f)) return "layer_norm_eps must be positive";
  return "";
}

void hb_init(HbModel* h) {
  h->d = h->cfg.hidden_size / h->cfg.n_heads;
  h->cg = h->cfg.hidden_size / h->cfg.pos_conv_groups;
  (void)hipGetDevice(&h->device);
  hubert_keys(h);
  hb_geometry(h);
}

void hb_release(HbModel* h) {
  h->free_weights();
  for (auto& c : h->ext) c.release();
  h->proj.release();
  h->pos.release();
  for (auto& l : h->layers) {
    l.qkv.release();
    l.out.release();
    l.ff1.release();
    l.ff2.release();
    if (l.qkv_w) (void)hipFree(l.qkv_w);
    if (l.qkv_b) (void)hipFree(l.qkv_b);
  }
  if (h->bucket_dev) (void)hipFree(h->bucket_dev);
  if (h->table) (void)hipFree(h->table);
}

int hb_load_weight(HbModel* h, const char* what, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  Weight* w;
  int rc = WeightTable::find(h, what, key, data, shape, ndim, &w);
  if (rc != US_OK) return rc;
  hipError_t e;
  if (!h->allocated && (e = hb_alloc(h)) != hipSuccess) return h->hip((std::string(what) + ": hipMalloc").c_str(), e);
  if ((rc = h->copy(*w, data, static_cast<hipStream_t>(stream))) != US_OK) return rc;      // hb_alloc made w->dev: no allocation here
  w->loaded = true;
  h->dirty = true;
  return US_OK;
}

int hb_frames(HbModel* h, const char* what, int64_t T) {
  if (!h) return WeightTable::fail(nullptr, US_EINVAL, std::string(what) + ": null handle");
  const long long f = T > 0 ? hb_steps(h->cfg, T, h->cfg.n_conv) : 0;
  if (f < 1 || f >= (1ll << 31))
    return h->fail(US_EINVAL, std::string(what) + ": " + std::to_string((long long)T) + " samples are fewer than the receptive field (" +
                                  std::to_string(hb_receptive_field(h->cfg)) + "), or too many");
  return (int)f;
}

size_t hb_workspace_bytes(HbModel* h, int B, int Tmax) {
  if (!h || B <= 0 || Tmax <= 0 || hb_steps(h->cfg, Tmax, h->cfg.n_conv) < 1) return 0;
  return hb_plan(h, B, Tmax).total * sizeof(float) + 256;
}

// hidden state l of item b starts at hidden_states + b * hs_bs + l * hs_ls (floats)
int hb_forward(HbModel* h, const std::string& what, const float* wav, const int64_t* lengths, int B, int Tmax, int normalize, int n_layers_out,
               float* out, float* hidden_states, long long hs_bs, long long hs_ls, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!h || !wav || !out || B <= 0 || Tmax <= 0) return WeightTable::fail(h, US_EINVAL, what + ": bad argument");
  const auto& c = h->cfg;
  if (n_layers_out < 0 || n_layers_out > c.n_layers)
    return h->fail(US_EINVAL, what + ": n_layers_out must be between 0 and the configuration's " + std::to_string(c.n_layers) + " layers");
  const long long field = hb_receptive_field(c);
  if (Tmax < field)
    return h->fail(US_EINVAL, what + ": Tmax = " + std::to_string(Tmax) + " is shorter than the receptive field (" + std::to_string(field) +
                                  " samples)");
  const std::string bad = bad_length(what.c_str(), lengths, B, field, Tmax);
  if (!bad.empty()) return h->fail(US_EINVAL, bad + " must be at least the receptive field (" + std::to_string(field) + " samples) and at most Tmax");
  const int H = c.hidden_size, I = c.intermediate_size, nl = c.n_conv;
  int Tl[kHbMaxConv + 1];                 // buffer widths: the steps of a Tmax-sample item after each layer
  Tl[0] = Tmax;
  long long big = 0;
  for (int i = 1; i <= nl; ++i) {
    Tl[i] = (int)hb_steps(c, Tmax, i);
    big = std::max(big, (long long)c.conv_dim[i - 1] * Tl[i]);
  }
  const int F = Tl[nl];
  big = std::max(big, (long long)std::max(3 * H, I) * F);
  if (big >= (1ll << 31)) return h->fail(US_EINVAL, what + ": channels * steps of one item too large");
  const size_t fh = (size_t)F * H;
  if (hidden_states) {
    const long long f = (long long)fh, n1 = n_layers_out + 1;
    const bool items_outer = hs_ls >= f && hs_bs >= n1 * hs_ls, layers_outer = hs_bs >= f && hs_ls >= (long long)B * hs_bs;
    if (!items_outer && !layers_outer)
      return h->fail(US_EINVAL, what + ": the hidden states' item and layer strides must describe [B][n + 1][F][H] or [n + 1][B][F][H] without overlap");
  }
  const int rc = h->all_loaded(what.c_str());
  if (rc != US_OK) return rc;
  if (!workspace || workspace_bytes < hb_workspace_bytes(h, B, Tmax))
    return h->fail(US_EWORKSPACE, what + ": workspace too small (" + h->abi + "_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->dirty) {
    const hipError_t e = hb_prepare(h, s);
    if (e != hipSuccess) return h->hip((what + ": preparing the weights").c_str(), e);
  }
  const HbPlan p = hb_plan(h, B, Tmax);
  float* base = ws_align(workspace);
  auto W = [&](const std::string& k) { return h->w.at(k).dev; };
  auto Wopt = [&](const std::string& k) { return h->conv_bias ? h->w.at(k).dev : nullptr; };
  const bool pre_ln = h->pre_ln();
  for_item_groups<kHbItems>(B, [&](int b) { return lengths ? lengths[b] : Tmax; }, [&](int b0, int nb, const ItemLens<kHbItems>& items, int) {
    HbLens lens{items, {}, {}};
    for (int i = 0; i < kHbMaxConv; ++i) {
      lens.k[i] = i < nl ? c.conv_kernel[i] : 1;
      lens.s[i] = i < nl ? c.conv_stride[i] : 1;
    }
    const float* x = wav + (size_t)b0 * Tmax;
    float* stats = nullptr;
    if (normalize) {
      stats = base + p.stats + 2 * (size_t)b0;
      hipLaunchKernelGGL(hb_wavstats_kernel, dim3(nb), dim3(1024), 0, s, x, stats, lens, Tmax);
    }
    // LayerNorm over the channels of a planar [C][T] tensor of the items at hand; e1 / e2: channel-last copies
    auto ln_launch = [&](const float* in, const float* res, const std::string& key, float* y, float* e1, float* e2, long long e1_bs, int level, int C,
                         int T, float eps, int gelu) {
      hipLaunchKernelGGL(hb_ln_kernel, dim3((T + kLnCols - 1) / kLnCols, nb), dim3(1024), 0, s, in, res, W(key + ".weight"), W(key + ".bias"), y, e1, e2,
                         e1_bs, (long long)fh, lens, level, C, T, eps, gelu);
    };
    // the feature extractor
    float* eb[2] = {base + p.a, base + p.b};
    float* cur = eb[0] + (size_t)b0 * c.conv_dim[0] * Tl[1];
    const float* feat;                    // the feature projection's normalised input
    const int Cl = c.conv_dim[nl - 1];
    hipLaunchKernelGGL(hb_conv0_kernel, dim3((Tl[1] + 255) / 256, nb), dim3(256), 0, s, x, stats, W(hb_conv_key(0)), Wopt(hb_conv_prefix(0) + "conv.bias"),
                       cur, lens, Tmax, c.conv_dim[0], Tl[1]);
    if (h->layer_ext()) {                 // conv (+ bias) into one buffer, LayerNorm over channels + GELU into the other
      int at = 0;                         // the buffer `cur` lies in
      auto other = [&](int ch, int T) {
        at ^= 1;
        return eb[at] + (size_t)b0 * ch * T;
      };
      for (int i = 0; i < nl; ++i) {
        if (i > 0) {
          float* nxt = other(c.conv_dim[i], Tl[i + 1]);
          HbGemm g{&h->ext[i - 1], cur, Wopt(hb_conv_prefix(i) + "conv.bias"), nullptr, nxt, Tl[i], Tl[i + 1]};
          g.stride = c.conv_stride[i]; g.level = i + 1;
          hb_gemm(s, g, lens, nb);
          cur = nxt;
        }
        float* nrm = other(c.conv_dim[i], Tl[i + 1]);
        ln_launch(cur, nullptr, hb_conv_prefix(i) + "layer_norm", nrm, nullptr, nullptr, 0ll, i + 1, c.conv_dim[i], Tl[i + 1], 1e-5f, 1);
        cur = nrm;
      }
      float* nrm = other(Cl, F);
      ln_launch(cur, nullptr, "feature_projection.layer_norm", nrm, nullptr, nullptr, 0ll, nl, Cl, F, c.layer_norm_eps, 0);
      feat = nrm;
    } else {
      hipLaunchKernelGGL(hb_gn_gelu_kernel, dim3(c.conv_dim[0], nb), dim3(256), 0, s, cur, W("feature_extractor.conv_layers.0.layer_norm.weight"),
                         W("feature_extractor.conv_layers.0.layer_norm.bias"), lens, c.conv_dim[0], Tl[1]);
      for (int i = 1; i < nl; ++i) {
        float* nxt = eb[i & 1] + (size_t)b0 * c.conv_dim[i] * Tl[i + 1];
        HbGemm g{&h->ext[i - 1], cur, Wopt(hb_conv_prefix(i) + "conv.bias"), nullptr, nxt, Tl[i], Tl[i + 1]};
        g.stride = c.conv_stride[i]; g.gelu = 1; g.level = i + 1;
        hb_gemm(s, g, lens, nb);
        cur = nxt;
      }
      float* nrm = eb[nl & 1] + (size_t)b0 * Cl * F;
      ln_launch(cur, nullptr, "feature_projection.layer_norm", nrm, nullptr, nullptr, 0ll, nl, Cl, F, c.layer_norm_eps, 0);
      feat = nrm;
    }
    float* X0 = base + p.x0 + b0 * fh;
    float* P = base + p.p + b0 * fh;
    float* X = base + p.x + b0 * fh;
    float* X1 = base + p.x1 + b0 * fh;
    float* Y = base + p.y + b0 * fh;
    float* QKV = base + p.qkv + 3 * b0 * fh;
    float* ATT = base + p.att + b0 * fh;
    float* FF = base + p.ff + (size_t)b0 * F * I;
    float* G = h->wavlm ? base + p.gate + (size_t)b0 * c.n_heads * F : nullptr;
    {
      HbGemm g{&h->proj, feat, W("feature_projection.projection.bias"), nullptr, X0, F, F};
      g.level = nl;
      hb_gemm(s, g, lens, nb);
    }
    // x + gelu(pos_conv(x))
    {
      HbGemm g{&h->pos, X0, W("encoder.pos_conv_embed.conv.bias"), X0, P, F, F};
      g.groups = c.pos_conv_groups; g.gelu = 1; g.level = nl;
      hb_gemm(s, g, lens, nb);
    }
    // layer >= 0: the encoder's state after that many layers, which goes to its hidden_states slot and, when it is the last one asked for, to out
    auto slot = [&](int layer) { return layer >= 0 && hidden_states ? hidden_states + (size_t)b0 * hs_bs + (size_t)layer * hs_ls : nullptr; };
    auto result = [&](int layer) { return layer == n_layers_out ? out + b0 * fh : nullptr; };
    auto ln = [&](const float* in, const float* res, const std::string& key, float* y, int layer) {
      ln_launch(in, res, key, y, slot(layer), result(layer), hs_bs, nl, H, F, c.layer_norm_eps, 0);
    };
    auto attention = [&](const float* in, const HbLayer& l, const std::string& q) {          // in -> ATT
      if (h->wavlm)
        hipLaunchKernelGGL(wl_gate_kernel, dim3((F + 255) / 256, c.n_heads, nb), dim3(256), 0, s, in, W(q + "attention.gru_rel_pos_linear.weight"),
                           W(q + "attention.gru_rel_pos_linear.bias"), W(q + "attention.gru_rel_pos_const"), G, H, h->d, F);
      HbGemm g{&l.qkv, in, l.qkv_b, nullptr, QKV, F, F};
      g.nscale = H; g.scale = 1.f / sqrtf((float)h->d); g.level = nl;
      hb_gemm(s, g, lens, nb);
      hb_attn(s, QKV, ATT, lens, nl, H, c.n_heads, h->d, F, nb, G, h->table, h->D);
    };
    if (pre_ln) {
      // the residual stream stays un-normalised: x + attn(LN(x)), then h + ffn(LN(h)), the residual added in the GEMM's epilogue.  Hidden state
      // i < L is the stream before layer i (a transposing copy), hidden state L is encoder.layer_norm of it.
      float* S = P;                       // the stream
      float* S2 = X;                      // the buffer the next stream is written to
      auto export_stream = [&](int layer) {
        float* e1 = slot(layer);
        float* e2 = result(layer);
        if (e1 || e2)
          hipLaunchKernelGGL(hb_export_kernel, dim3((F + kLnCols - 1) / kLnCols, (H + kLnSlices - 1) / kLnSlices, nb), dim3(1024), 0, s, S, e1, e2, hs_bs,
                             (long long)fh, H, F);
      };
      for (int i = 0; i < n_layers_out; ++i) {
        const HbLayer& l = h->layers[i];
        const std::string q = hb_layer_key(i);
        export_stream(i);
        ln_launch(S, nullptr, q + "layer_norm", X1, nullptr, nullptr, 0ll, nl, H, F, c.layer_norm_eps, 0);
        attention(X1, l, q);
        {
          HbGemm g{&l.out, ATT, W(q + "attention.out_proj.bias"), S, Y, F, F};
          g.level = nl;
          hb_gemm(s, g, lens, nb);
        }
        ln_launch(Y, nullptr, q + "final_layer_norm", X1, nullptr, nullptr, 0ll, nl, H, F, c.layer_norm_eps, 0);
        {
          HbGemm g{&l.ff1, X1, W(q + "feed_forward.intermediate_dense.bias"), nullptr, FF, F, F};
          g.gelu = 1; g.level = nl;
          hb_gemm(s, g, lens, nb);
        }
        {
          HbGemm g{&l.ff2, FF, W(q + "feed_forward.output_dense.bias"), Y, S2, F, F};
          g.level = nl;
          hb_gemm(s, g, lens, nb);
        }
        std::swap(S, S2);
      }
      if (n_layers_out == c.n_layers)
        ln(S, nullptr, "encoder.layer_norm", nullptr, n_layers_out);
      else
        export_stream(n_layers_out);
      return;
    }
    ln(P, nullptr, "encoder.layer_norm", X, 0);
    for (int i = 0; i < n_layers_out; ++i) {
      const HbLayer& l = h->layers[i];
      const std::string q = hb_layer_key(i);
      attention(X, l, q);
      {
        HbGemm g{&l.out, ATT, W(q + "attention.out_proj.bias"), nullptr, Y, F, F};
        g.level = nl;
        hb_gemm(s, g, lens, nb);
      }
      ln(Y, X, q + "layer_norm", X1, -1);
      {
        HbGemm g{&l.ff1, X1, W(q + "feed_forward.intermediate_dense.bias"), nullptr, FF, F, F};
        g.gelu = 1; g.level = nl;
        hb_gemm(s, g, lens, nb);
      }
      {
        HbGemm g{&l.ff2, FF, W(q + "feed_forward.output_dense.bias"), nullptr, Y, F, F};
        g.level = nl;
        hb_gemm(s, g, lens, nb);
      }
      ln(Y, X1, q + "final_layer_norm", X, i + 1);
    }
  });
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip(what.c_str(), e);
}

}  // namespace

// ---- Whisper's encoder (whisper_encoder.h; us_whisper_* in whisper.hip) on the kernels above -----------------------------------------------------
// GELU(conv1) (k 3, padding 1), GELU(conv2) (k 3, stride 2, padding 1) + embed_positions in the GEMM's epilogue, WavLM-large's pre-LN layer
// schedule without the relative position bias, encoder.layer_norm.  Every item has S frames: the length carrier holds S (2 S for conv1).
struct WhEncoder {
  WhEncGeometry g{};
  PlanarConv conv1, conv2;
  std::vector<HbLayer> layers;
  std::vector<PlanarConv> cross;      // per decoder layer: [k_proj | v_proj] of the encoder's output
  std::vector<float*> cross_w, cross_b;
  float* pos = nullptr;               // embed_positions as a planar [d_model][S] tensor
};

namespace {
std::string wh_enc_key(int i) { return "model.encoder.layers." + std::to_string(i) + "."; }
std::string wh_cross_key(int i) { return "model.decoder.layers." + std::to_string(i) + ".encoder_attn."; }

HbLens wh_lens(int n) {
  HbLens l{};
  for (int i = 0; i < kHbItems; ++i) l.n[i] = n;
  for (int i = 0; i < kHbMaxConv; ++i) l.k[i] = l.s[i] = 1;
  return l;
}
}  // namespace

WhEncoder* wh_encoder_new(const WhEncGeometry& g) {
  auto* e = new WhEncoder();
  e->g = g;
  const int H = g.d_model;
  e->conv1.conv(g.n_mels, g.n_mels, H, 3, 1);
  e->conv2.conv(H, H, H, 3, 1);
  e->layers.resize(g.layers);
  for (auto& l : e->layers) {
    l.qkv.conv(H, H, 3 * H, 1, 1);
    l.out.conv(H, H, H, 1, 1);
    l.ff1.conv(H, H, g.ffn, 1, 1);
    l.ff2.conv(g.ffn, g.ffn, H, 1, 1);
  }
  e->cross.resize(g.dec_layers);
  for (auto& c : e->cross) c.conv(H, H, 2 * H, 1, 1);
  e->cross_w.assign(g.dec_layers, nullptr);
  e->cross_b.assign(g.dec_layers, nullptr);
  return e;
}

void wh_encoder_free(WhEncoder* e) {
  if (!e) return;
  e->conv1.release();
  e->conv2.release();
  for (auto& l : e->layers) {
    l.qkv.release();
    l.out.release();
    l.ff1.release();
    l.ff2.release();
    if (l.qkv_w) (void)hipFree(l.qkv_w);
    if (l.qkv_b) (void)hipFree(l.qkv_b);
  }
  for (auto& c : e->cross) c.release();
  for (float* p : e->cross_w)
    if (p) (void)hipFree(p);
  for (float* p : e->cross_b)
    if (p) (void)hipFree(p);
  if (e->pos) (void)hipFree(e->pos);
  delete e;
}

hipError_t wh_encoder_alloc(WhEncoder* e) {
  hipError_t err = hipSuccess;
  auto alloc = [&](float** p, size_t n) {
    if (err == hipSuccess && !*p) err = hipMalloc(p, std::max<size_t>(n, 1) * sizeof(float));
  };
  const size_t H = (size_t)e->g.d_model;
  alloc(&e->conv1.packed, e->conv1.packed_floats());
  alloc(&e->conv2.packed, e->conv2.packed_floats());
  alloc(&e->pos, H * e->g.S);
  for (auto& l : e->layers) {
    alloc(&l.qkv.packed, l.qkv.packed_floats());
    alloc(&l.out.packed, l.out.packed_floats());
    alloc(&l.ff1.packed, l.ff1.packed_floats());
    alloc(&l.ff2.packed, l.ff2.packed_floats());
    alloc(&l.qkv_w, 3 * H * H);
    alloc(&l.qkv_b, 3 * H);
  }
  for (int i = 0; i < e->g.dec_layers; ++i) {
    alloc(&e->cross[i].packed, e->cross[i].packed_floats());
    alloc(&e->cross_w[i], 2 * H * H);
    alloc(&e->cross_b[i], 2 * H);
  }
  return err;
}

hipError_t wh_encoder_prepare(WhEncoder* e, WeightTable& t, hipStream_t s) {
  auto W = [&](const std::string& k) { return t.w.at(k).dev; };
  const size_t H = (size_t)e->g.d_model, S = (size_t)e->g.S;
  hipError_t err = hipSuccess;
  auto copy = [&](float* dst, const float* src, size_t n) {
    if (err == hipSuccess) err = src ? hipMemcpyAsync(dst, src, n * sizeof(float), hipMemcpyDeviceToDevice, s) : hipMemsetAsync(dst, 0, n * sizeof(float), s);
  };
  e->conv1.pack(W("model.encoder.conv1.weight"), s);
  e->conv2.pack(W("model.encoder.conv2.weight"), s);
  // embed_positions [S][H] read as a planar [C = S][T = H] tensor: its channel-last copy is [H][S]
  hipLaunchKernelGGL(hb_export_kernel, dim3((unsigned)((H + kLnCols - 1) / kLnCols), (unsigned)((S + kLnSlices - 1) / kLnSlices), 1), dim3(1024), 0, s,
                     W("model.encoder.embed_positions.weight"), e->pos, (float*)nullptr, 0ll, 0ll, (int)S, (int)H);
  for (int i = 0; i < e->g.layers; ++i) {
    HbLayer& l = e->layers[i];
    const std::string a = wh_enc_key(i) + "self_attn.";
    copy(l.qkv_w, W(a + "q_proj.weight"), H * H);
    copy(l.qkv_w + H * H, W(a + "k_proj.weight"), H * H);
    copy(l.qkv_w + 2 * H * H, W(a + "v_proj.weight"), H * H);
    copy(l.qkv_b, W(a + "q_proj.bias"), H);
    copy(l.qkv_b + H, nullptr, H);
    copy(l.qkv_b + 2 * H, W(a + "v_proj.bias"), H);
    if (err != hipSuccess) return err;
    l.qkv.pack(l.qkv_w, s);
    l.out.pack(W(a + "out_proj.weight"), s);
    l.ff1.pack(W(wh_enc_key(i) + "fc1.weight"), s);
    l.ff2.pack(W(wh_enc_key(i) + "fc2.weight"), s);
  }
  for (int i = 0; i < e->g.dec_layers; ++i) {
    const std::string a = wh_cross_key(i);
    copy(e->cross_w[i], W(a + "k_proj.weight"), H * H);
    copy(e->cross_w[i] + H * H, W(a + "v_proj.weight"), H * H);
    copy(e->cross_b[i], nullptr, H);
    copy(e->cross_b[i] + H, W(a + "v_proj.bias"), H);
    if (err != hipSuccess) return err;
    e->cross[i].pack(e->cross_w[i], s);
  }
  return hipGetLastError();
}

namespace {
struct WhEncPlan {
  size_t c1, x, x2, x1, y, qkv, att, ff, total;
};
WhEncPlan wh_enc_plan(const WhEncGeometry& g, int B) {
  WhEncPlan p{};
  WsTake take;
  const size_t bs = (size_t)B * g.S, H = (size_t)g.d_model;
  p.c1 = take(2 * bs * H);
  p.x = take(bs * H);
  p.x2 = take(bs * H);
  p.x1 = take(bs * H);
  p.y = take(bs * H);
  p.qkv = take(3 * bs * H);
  p.att = take(bs * H);
  p.ff = take(bs * (size_t)g.ffn);
  p.total = take.total;
  return p;
}
}  // namespace

size_t wh_encoder_ws_floats(const WhEncoder* e, int B) { return wh_enc_plan(e->g, B).total; }

hipError_t wh_encoder_forward(WhEncoder* e, WeightTable& t, const float* feats, int B, float* planar, float* out, float* ws, hipStream_t s) {
  auto W = [&](const std::string& k) { return t.w.at(k).dev; };
  const WhEncGeometry& g = e->g;
  const int H = g.d_model, S = g.S, I = g.ffn, d = H / g.heads;
  const size_t sh = (size_t)S * H;
  const WhEncPlan p = wh_enc_plan(g, B);
  const HbLens lens = wh_lens(S), lens2 = wh_lens(2 * S);
  for (int b0 = 0; b0 < B; b0 += kHbItems) {
    const int nb = std::min(kHbItems, B - b0);
    float* C1 = ws + p.c1 + 2 * b0 * sh;
    float* X = ws + p.x + b0 * sh;
    float* X2 = ws + p.x2 + b0 * sh;
    float* X1 = ws + p.x1 + b0 * sh;
    float* Y = ws + p.y + b0 * sh;
    float* QKV = ws + p.qkv + 3 * b0 * sh;
    float* ATT = ws + p.att + b0 * sh;
    float* FF = ws + p.ff + (size_t)b0 * S * I;
    auto ln_launch = [&](const float* in, const std::string& key, float* y, float* e2) {
      hipLaunchKernelGGL(hb_ln_kernel, dim3((S + kLnCols - 1) / kLnCols, nb), dim3(1024), 0, s, in, (const float*)nullptr, W(key + ".weight"),
                         W(key + ".bias"), y, (float*)nullptr, e2, 0ll, (long long)sh, lens, 0, H, S, 1e-5f, 0);
    };
    {
      HbGemm c{&e->conv1, feats + (size_t)b0 * g.n_mels * 2 * S, W("model.encoder.conv1.bias"), nullptr, C1, 2 * S, 2 * S};
      c.gelu = 1;
      hb_gemm(s, c, lens2, nb);
    }
    {
      HbGemm c{&e->conv2, C1, W("model.encoder.conv2.bias"), e->pos, X, 2 * S, S};
      c.stride = 2; c.gelu = 1; c.res_bs = 0;
      hb_gemm(s, c, lens, nb);
    }
    float* St = X;
    float* St2 = X2;
    for (int i = 0; i < g.layers; ++i) {
      const HbLayer& l = e->layers[i];
      const std::string q = wh_enc_key(i);
      ln_launch(St, q + "self_attn_layer_norm", X1, nullptr);
      {
        HbGemm c{&l.qkv, X1, l.qkv_b, nullptr, QKV, S, S};
        c.nscale = H; c.scale = 1.f / sqrtf((float)d);
        hb_gemm(s, c, lens, nb);
      }
      hb_attn(s, QKV, ATT, lens, 0, H, g.heads, d, S, nb, nullptr, nullptr, 0);
      {
        HbGemm c{&l.out, ATT, W(q + "self_attn.out_proj.bias"), St, Y, S, S};
        hb_gemm(s, c, lens, nb);
      }
      ln_launch(Y, q + "final_layer_norm", X1, nullptr);
      {
        HbGemm c{&l.ff1, X1, W(q + "fc1.bias"), nullptr, FF, S, S};
        c.gelu = 1;
        hb_gemm(s, c, lens, nb);
      }
      {
        HbGemm c{&l.ff2, FF, W(q + "fc2.bias"), Y, St2, S, S};
        hb_gemm(s, c, lens, nb);
      }
      std::swap(St, St2);
    }
    ln_launch(St, "model.encoder.layer_norm", planar + b0 * sh, out ? out + b0 * sh : nullptr);
  }
  return hipGetLastError();
}

hipError_t wh_encoder_cross_kv(WhEncoder* e, WeightTable& t, const float* planar, int B, float* kv, hipStream_t s) {
  const WhEncGeometry& g = e->g;
  const size_t sh = (size_t)g.S * g.d_model;
  const HbLens lens = wh_lens(g.S);
  for (int i = 0; i < g.dec_layers; ++i)
    for (int b0 = 0; b0 < B; b0 += kHbItems) {
      const int nb = std::min(kHbItems, B - b0);
      HbGemm c{&e->cross[i], planar + b0 * sh, e->cross_b[i], nullptr, kv + ((size_t)i * B + b0) * 2 * sh, g.S, g.S};
      hb_gemm(s, c, lens, nb);
    }
  return hipGetLastError();
}

}  // namespace us

extern "C" {

using namespace us;

int us_hubert_create(us_hubert_handle* out, const us_hubert_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_hubert_create: null argument");
  const auto& c = *cfg;
  auto bad = [](const std::string& m) { return WeightTable::fail(nullptr, US_EINVAL, "us_hubert_create: " + m); };
  if (c.feat_extract_norm != US_HUBERT_NORM_GROUP) return bad("only the group-norm feature extractor (feat_extract_norm = \"group\") is built");
  if (c.do_stable_layer_norm) return bad("the pre-LN encoder (do_stable_layer_norm) is not built");
  const std::string m = hb_check_geometry(c);
  if (!m.empty()) return bad(m);
  auto* h = new us_hubert();
  h->cfg = c;
  hb_init(h);
  *out = h;
  return US_OK;
}

int us_hubert_destroy(us_hubert_handle h) {
  if (!h) return US_OK;
  hb_release(h);
  delete h;
  return US_OK;
}

int us_hubert_num_weights(us_hubert_handle h) { return h ? h->num() : 0; }
const char* us_hubert_weight_key(us_hubert_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_hubert_last_error(us_hubert_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_hubert_load_weight(us_hubert_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  return hb_load_weight(h, "us_hubert_load_weight", key, data, shape, ndim, stream);
}

int us_hubert_frames(us_hubert_handle h, int64_t T) { return hb_frames(h, "us_hubert_frames", T); }

size_t us_hubert_workspace_bytes(us_hubert_handle h, int B, int Tmax) { return hb_workspace_bytes(h, B, Tmax); }

int us_hubert_forward(us_hubert_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, int normalize, int n_layers_out, float* out,
                      float* hidden_states, void* workspace, size_t workspace_bytes, us_stream stream) {
  long long fh = 0;
  if (h && Tmax > 0) fh = std::max(0ll, hb_steps(h->cfg, Tmax, h->cfg.n_conv)) * h->cfg.hidden_size;
  return hb_forward(h, "us_hubert_forward", wav, lengths, B, Tmax, normalize, n_layers_out, out, hidden_states,
                    (long long)(std::max(n_layers_out, 0) + 1) * fh, fh, workspace, workspace_bytes, stream);
}

int us_wavlm_create(us_wavlm_handle* out, const us_wavlm_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_wavlm_create: null argument");
  auto bad = [](const std::string& m) { return WeightTable::fail(nullptr, US_EINVAL, "us_wavlm_create: " + m); };
  us_hubert_config c{};
  c.n_conv = cfg->n_conv;
  for (int i = 0; i < US_HUBERT_MAX_CONV; ++i) {
    c.conv_dim[i] = cfg->conv_dim[i];
    c.conv_kernel[i] = cfg->conv_kernel[i];
    c.conv_stride[i] = cfg->conv_stride[i];
  }
  c.hidden_size = cfg->hidden_size; c.n_heads = cfg->n_heads; c.intermediate_size = cfg->intermediate_size; c.n_layers = cfg->n_layers;
  c.pos_conv_kernel = cfg->pos_conv_kernel; c.pos_conv_groups = cfg->pos_conv_groups;
  c.feat_extract_norm = cfg->feat_extract_norm; c.do_stable_layer_norm = cfg->do_stable_layer_norm ? 1 : 0; c.layer_norm_eps = cfg->layer_norm_eps;
  const bool large = c.feat_extract_norm == US_HUBERT_NORM_LAYER && c.do_stable_layer_norm && cfg->conv_bias;
  const bool base = c.feat_extract_norm == US_HUBERT_NORM_GROUP && !c.do_stable_layer_norm && !cfg->conv_bias;
  if (!large && !base)
    return bad("feat_extract_norm, do_stable_layer_norm and conv_bias must be (layer, 1, 1), WavLM-large's form, or (group, 0, 0), WavLM-base's");
  const std::string m = hb_check_geometry(c);
  if (!m.empty()) return bad(m);
  if (cfg->num_buckets < 4 || cfg->num_buckets > 4096 || cfg->num_buckets % 2 != 0) return bad("num_buckets must be even, from 4 to 4096");
  if (cfg->max_bucket_distance <= cfg->num_buckets / 4 || cfg->max_bucket_distance > (1 << 20))
    return bad("max_bucket_distance must be above num_buckets / 4 and at most 2^20");
  auto* h = new us_wavlm();
  h->cfg = c;
  h->abi = "us_wavlm";
  h->wavlm = true;
  h->conv_bias = cfg->conv_bias ? 1 : 0;
  h->num_buckets = cfg->num_buckets;
  h->max_distance = cfg->max_bucket_distance;
  wl_bucket_map(h);
  hb_init(h);
  *out = h;
  return US_OK;
}

int us_wavlm_destroy(us_wavlm_handle h) {
  if (!h) return US_OK;
  hb_release(h);
  delete h;
  return US_OK;
}

int us_wavlm_num_weights(us_wavlm_handle h) { return h ? h->num() : 0; }
const char* us_wavlm_weight_key(us_wavlm_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_wavlm_last_error(us_wavlm_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_wavlm_load_weight(us_wavlm_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  return hb_load_weight(h, "us_wavlm_load_weight", key, data, shape, ndim, stream);
}

int us_wavlm_frames(us_wavlm_handle h, int64_t T) { return hb_frames(h, "us_wavlm_frames", T); }

size_t us_wavlm_workspace_bytes(us_wavlm_handle h, int B, int Tmax) { return hb_workspace_bytes(h, B, Tmax); }

int us_wavlm_position_bucket(us_wavlm_handle h, int64_t delta) {
  if (!h) return WeightTable::fail(nullptr, US_EINVAL, "us_wavlm_position_bucket: null handle");
  const long long D = h->D;
  return h->bucket[(size_t)(std::max<long long>(-D, std::min<long long>(D, delta)) + D)];
}

int us_wavlm_forward(us_wavlm_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, int normalize, int n_layers_out, float* out,
                     float* hidden_states, int64_t hs_item_stride, int64_t hs_layer_stride, void* workspace, size_t workspace_bytes,
                     us_stream stream) {
  return hb_forward(h, "us_wavlm_forward", wav, lengths, B, Tmax, normalize, n_layers_out, out, hidden_states, hs_item_stride, hs_layer_stride,
                    workspace, workspace_bytes, stream);
}

}  // extern "C"
