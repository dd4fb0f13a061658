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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"
#include "conv1d_planar.h"
#include "handle.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kHbItems = 32;        // batch items per launch: their lengths travel as kernel arguments (the caller's are on the host)
constexpr int kHbMaxConv = US_HUBERT_MAX_CONV;
constexpr int kHbMaxK0 = 16;        // taps of layer 0 held in registers

struct HbLens {
  int n[kHbItems];                  // samples per item
  int k[kHbMaxConv], s[kHbMaxConv];
};

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

// ---- extractor layer 0: out[b][c][q] = sum_j w[c][j] * x[b][s q + j], x = (wav - mean) * rstd; 0 at and past the item's steps -------------------
__global__ __launch_bounds__(256) void hb_conv0_kernel(const float* __restrict__ wav, const float* __restrict__ stats, const float* __restrict__ w,
                                                       float* __restrict__ out, HbLens lens, int Tmax, int C, int T1) {
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
    o[(size_t)c * T1] = a;
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
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int mh = wave & 1, nh = wave >> 1, kl = lane >> 5, cl = lane & 31;
  const int b = blockIdx.z, grp = blockIdx.y / a.mtiles, mt = blockIdx.y - grp * a.mtiles;
  const int m0 = mt * kPcBM, n0 = blockIdx.x * 64;
  f32x16 acc[1][2];
  planar_conv_mainloop<1, 2, STRIDE>({a.in + (size_t)b * a.in_bs + (size_t)grp * a.Cin * a.Tin, a.w + (size_t)grp * a.Kpad * a.ldw, a.Cin, a.Tin, 1,
                                      a.off, a.Kdim, a.Kpad, a.ldw, m0, n0},
                                     acc);
  const int t = n0 + nh * 32 + cl;
  if (t >= a.Tout) return;
  const bool live = t < hb_len(lens, b, a.level);
  float* __restrict__ out = a.out + (size_t)b * a.out_bs;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int cg = m0 + mh * 32 + mfma32_row(r, kl);
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
// added in slice order.  e1 / e2 (optional): the same values channel-last, [T][C] per item, written 32 x 32 through LDS.
constexpr int kLnCols = 32, kLnSlices = 32;

__global__ __launch_bounds__(1024) void hb_ln_kernel(const float* __restrict__ x, const float* __restrict__ res, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, float* __restrict__ y, float* __restrict__ e1,
                                                     float* __restrict__ e2, long long e1_bs, long long e2_bs, HbLens lens, int level, int C,
                                                     int T, float eps) {
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
    if (live && c < C) o = fmaf((at(c) - mean) * rs, gamma[c], beta[c]);
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

// ---- attention ---------------------------------------------------------------------------------------------------------------------------------
// qkv [3 H][F] planar per item (q already scaled); head h owns rows [h d, (h + 1) d) of each third.  A workgroup is 64 queries of one (item,
// head), a wave 16 of them.  Per key tile of 64 (through LDS, K as [c][key] with rows of 80 floats, V with rows of 68: both conflict-free
// for the reads below) a wave takes, on v_mfma_f32_16x16x4_f32,
//   S^T[key][q] = sum_c K[c][key] Q[c][q]     A = K^T (lane: key l & 15, c l >> 4), B = Q (registers, loaded once): four 16-key accumulators;
//   O^T[c][q]  += sum_key V[c][key] P^T[key][q]:  a lane's accumulator register r of key block ks IS P^T[16 ks + 4 (l >> 4) + r][q = l & 15],
//                 the B operand of a k-step whose four keys are {16 ks + 4 g + r : g = l >> 4}; A reads V at those same keys (one float4).
// So the probabilities never leave their registers.  The head dimension is padded to 16 DT with zero rows (d = 20: DT = 2).
constexpr int kAtQ = 64, kAtK = 64, kAtKs = 80, kAtVs = 68;
typedef float f32x4 __attribute__((ext_vector_type(4)));

template <int DT>
__global__ __launch_bounds__(256) void hb_attn_kernel(const float* __restrict__ qkv, float* __restrict__ out, HbLens lens, int level, int H, int d,
                                                      int F, long long qkv_bs, long long out_bs) {
  __shared__ float Ks[16 * DT][kAtKs];
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

struct HbLayer {
  PlanarConv qkv, out, ff1, ff2;
  float* qkv_w = nullptr;     // [3 H][H]: q | k | v
  float* qkv_b = nullptr;     // [3 H]
};

}  // namespace
}  // namespace us

struct us_hubert : us::WeightTable {
  us_hubert_config cfg{};
  int d = 0, cg = 0;                       // head dimension; channels per positional-convolution group
  std::vector<us::PlanarConv> ext;         // extractor layers 1 .. n_conv - 1 (index i - 1)
  us::PlanarConv proj, pos;                // pos: one group's geometry, `packed` holds all groups
  std::vector<us::HbLayer> layers;
  bool allocated = false;                  // device tensors exist (made by the first load, so creating a handle touches no device)
  bool dirty = true;                       // a weight changed since the derived forms were made
};

namespace us {
namespace {

std::string hb_conv_key(int i) { return "feature_extractor.conv_layers." + std::to_string(i) + ".conv.weight"; }
std::string hb_layer_key(int i) { return "encoder.layers." + std::to_string(i) + "."; }

void hb_add_affine(us_hubert* h, const std::string& p, int n) {
  h->add(p + ".weight", {n});
  h->add(p + ".bias", {n});
}
void hb_add_linear(us_hubert* h, const std::string& p, int out, int in) {
  h->add(p + ".weight", {out, in});
  h->add(p + ".bias", {out});
}

// transformers.HubertModel's registration order (the positional convolution's weight in its folded form: g v / |v|)
void hubert_keys(us_hubert* h) {
  const auto& c = h->cfg;
  const int H = c.hidden_size, I = c.intermediate_size, Cl = c.conv_dim[c.n_conv - 1];
  for (int i = 0; i < c.n_conv; ++i) {
    h->add(hb_conv_key(i), {c.conv_dim[i], i ? c.conv_dim[i - 1] : 1, c.conv_kernel[i]});
    if (i == 0) hb_add_affine(h, "feature_extractor.conv_layers.0.layer_norm", c.conv_dim[0]);
  }
  hb_add_affine(h, "feature_projection.layer_norm", Cl);
  hb_add_linear(h, "feature_projection.projection", H, Cl);
  h->add("encoder.pos_conv_embed.conv.bias", {H});
  h->add("encoder.pos_conv_embed.conv.weight", {H, h->cg, c.pos_conv_kernel});
  hb_add_affine(h, "encoder.layer_norm", H);
  for (int i = 0; i < c.n_layers; ++i) {
    const std::string p = hb_layer_key(i);
    for (const char* n : {"k_proj", "v_proj", "q_proj", "out_proj"}) hb_add_linear(h, p + "attention." + n, H, H);
    hb_add_affine(h, p + "layer_norm", H);
    hb_add_linear(h, p + "feed_forward.intermediate_dense", I, H);
    hb_add_linear(h, p + "feed_forward.output_dense", H, I);
    hb_add_affine(h, p + "final_layer_norm", H);
  }
}

void hb_geometry(us_hubert* h) {
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

// every tensor the forward reads, at once: after the first load neither a load nor a forward allocates
hipError_t hb_alloc(us_hubert* h) {
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
  h->allocated = e == hipSuccess;
  return e;
}

// the packed GEMM weights (and the q | k | v concatenation) from the loaded tensors
hipError_t hb_prepare(us_hubert* h, hipStream_t s) {
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

size_t hb_pad(size_t n) { return (n + 63) / 64 * 64; }

struct HbPlan {                 // float offsets into the 256-byte aligned workspace
  size_t stats, a, b, x0, p, x, x1, y, qkv, att, ff, total;
};

HbPlan hb_plan(const us_hubert_config& c, int B, int Tmax) {
  HbPlan p{};
  size_t o = 0;
  auto take = [&](size_t n) { const size_t at = o; o += hb_pad(n); return at; };
  size_t ea = 0, eb = 0;        // the extractor's two buffers: layer i writes a (i even) or b (i odd); the projection's LayerNorm takes the other
  for (int i = 0; i <= c.n_conv; ++i) {
    const int ch = c.conv_dim[std::min(i, c.n_conv - 1)];
    const size_t n = (size_t)B * ch * (size_t)hb_steps(c, Tmax, std::min(i + 1, c.n_conv));
    (i % 2 == 0 ? ea : eb) = std::max(i % 2 == 0 ? ea : eb, n);
  }
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
  p.total = o;
  return p;
}

struct HbGemm {                 // one launch of hb_gemm_kernel
  const PlanarConv* c;
  const float *in, *bias, *res;
  float* out;
  int Tin, Tout, stride = 1, groups = 1, gelu = 0, nscale = 0, level = 0;
  float scale = 1.f;
};

void hb_gemm(hipStream_t s, const HbGemm& g, const HbLens& lens, int nb) {
  const PlanarConv& c = *g.c;
  HbGemmArgs a{};
  a.in = g.in; a.w = c.packed; a.bias = g.bias; a.res = g.res; a.out = g.out;
  a.in_bs = (long long)c.cin * g.groups * g.Tin;
  a.out_bs = a.res_bs = (long long)c.cout * g.groups * g.Tout;
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

void hb_attn(hipStream_t s, const float* qkv, float* out, const HbLens& lens, int level, int H, int heads, int d, int F, int nb) {
  const dim3 grid((F + kAtQ - 1) / kAtQ, heads, nb);
  const long long qb = 3ll * H * F, ob = (long long)H * F;
  switch ((d + 15) / 16) {
    case 1: hipLaunchKernelGGL(hb_attn_kernel<1>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
    case 2: hipLaunchKernelGGL(hb_attn_kernel<2>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
    case 3: hipLaunchKernelGGL(hb_attn_kernel<3>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
    default: hipLaunchKernelGGL(hb_attn_kernel<4>, grid, dim3(256), 0, s, qkv, out, lens, level, H, d, F, qb, ob); break;
  }
}

}  // namespace
}  // namespace us

extern "C" {

using namespace us;

int us_hubert_create(us_hubert_handle* out, const us_hubert_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_hubert_create: null argument");
  const auto& c = *cfg;
  auto bad = [](const std::string& m) { return WeightTable::fail(nullptr, US_EINVAL, "us_hubert_create: " + m); };
  if (c.feat_extract_norm != US_HUBERT_NORM_GROUP) return bad("only the group-norm feature extractor (feat_extract_norm = \"group\") is built");
  if (c.do_stable_layer_norm) return bad("the pre-LN encoder (do_stable_layer_norm) is not built");
  if (c.n_conv < 1 || c.n_conv > kHbMaxConv) return bad("1 to 8 feature-extractor layers");
  for (int i = 0; i < c.n_conv; ++i) {
    if (c.conv_dim[i] < 1 || c.conv_dim[i] > 8192 || c.conv_kernel[i] < 1 || c.conv_kernel[i] > 64 || c.conv_stride[i] < 1)
      return bad("bad conv_dim / conv_kernel / conv_stride at layer " + std::to_string(i));
    if (i == 0 ? c.conv_kernel[0] > kHbMaxK0 || c.conv_stride[0] > 64 : c.conv_stride[i] > 4)
      return bad("layer 0 takes at most 16 taps, the others a stride of at most 4");
  }
  if (c.hidden_size < 1 || c.hidden_size > 8192 || c.intermediate_size < 1 || c.intermediate_size > 32768 || c.n_layers < 0 || c.n_layers > 64)
    return bad("bad hidden_size / intermediate_size / n_layers");
  if (c.n_heads < 1 || c.hidden_size % c.n_heads != 0) return bad("hidden_size must be divisible by the number of heads");
  const int d = c.hidden_size / c.n_heads;
  if (d > 64 || d % 4 != 0) return bad("the head dimension must be a multiple of 4, at most 64 (got " + std::to_string(d) + ")");
  if (c.pos_conv_groups < 1 || c.hidden_size % c.pos_conv_groups != 0) return bad("hidden_size must be divisible by the positional convolution's groups");
  if (c.pos_conv_kernel < 1 || c.pos_conv_kernel > 1024) return bad("bad positional convolution kernel");
  if (!(c.layer_norm_eps > 0.f)) return bad("layer_norm_eps must be positive");
  auto* h = new us_hubert();
  h->cfg = c;
  h->d = d;
  h->cg = c.hidden_size / c.pos_conv_groups;
  (void)hipGetDevice(&h->device);
  hubert_keys(h);
  hb_geometry(h);
  *out = h;
  return US_OK;
}

int us_hubert_destroy(us_hubert_handle h) {
  if (!h) return US_OK;
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
  delete h;
  return US_OK;
}

int us_hubert_num_weights(us_hubert_handle h) { return h ? h->num() : 0; }
const char* us_hubert_weight_key(us_hubert_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_hubert_last_error(us_hubert_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_hubert_load_weight(us_hubert_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  Weight* w;
  int rc = WeightTable::find(h, "us_hubert_load_weight", key, data, shape, ndim, &w);
  if (rc != US_OK) return rc;
  hipError_t e;
  if (!h->allocated && (e = hb_alloc(h)) != hipSuccess) return h->hip("us_hubert_load_weight: hipMalloc", e);
  if ((rc = h->copy(*w, data, static_cast<hipStream_t>(stream))) != US_OK) return rc;      // hb_alloc made w->dev: no allocation here
  w->loaded = true;
  h->dirty = true;
  return US_OK;
}

int us_hubert_frames(us_hubert_handle h, int64_t T) {
  if (!h) return WeightTable::fail(nullptr, US_EINVAL, "us_hubert_frames: null handle");
  const long long f = T > 0 ? hb_steps(h->cfg, T, h->cfg.n_conv) : 0;
  if (f < 1 || f >= (1ll << 31))
    return h->fail(US_EINVAL, "us_hubert_frames: " + std::to_string((long long)T) + " samples are fewer than the receptive field (" +
                                  std::to_string(hb_receptive_field(h->cfg)) + "), or too many");
  return (int)f;
}

size_t us_hubert_workspace_bytes(us_hubert_handle h, int B, int Tmax) {
  if (!h || B <= 0 || Tmax <= 0 || hb_steps(h->cfg, Tmax, h->cfg.n_conv) < 1) return 0;
  return hb_plan(h->cfg, B, Tmax).total * sizeof(float) + 256;
}

int us_hubert_forward(us_hubert_handle h, const float* wav, const int64_t* lengths, int B, int Tmax, int normalize, int n_layers_out, float* out,
                      float* hidden_states, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!h || !wav || !out || B <= 0 || Tmax <= 0) return WeightTable::fail(h, US_EINVAL, "us_hubert_forward: bad argument");
  const auto& c = h->cfg;
  if (n_layers_out < 0 || n_layers_out > c.n_layers)
    return h->fail(US_EINVAL, "us_hubert_forward: n_layers_out must be between 0 and the configuration's " + std::to_string(c.n_layers) + " layers");
  const long long field = hb_receptive_field(c);
  if (Tmax < field)
    return h->fail(US_EINVAL, "us_hubert_forward: Tmax = " + std::to_string(Tmax) + " is shorter than the receptive field (" + std::to_string(field) +
                                  " samples)");
  for (int b = 0; lengths && b < B; ++b)
    if (lengths[b] < field || lengths[b] > Tmax)
      return h->fail(US_EINVAL, "us_hubert_forward: lengths[" + std::to_string(b) + "] = " + std::to_string((long long)lengths[b]) +
                                    " must be at least the receptive field (" + std::to_string(field) + " samples) and at most Tmax");
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
  if (big >= (1ll << 31)) return h->fail(US_EINVAL, "us_hubert_forward: channels * steps of one item too large");
  const int rc = h->all_loaded("us_hubert_forward");
  if (rc != US_OK) return rc;
  if (!workspace || workspace_bytes < us_hubert_workspace_bytes(h, B, Tmax))
    return h->fail(US_EWORKSPACE, "us_hubert_forward: workspace too small (us_hubert_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (h->dirty) {
    const hipError_t e = hb_prepare(h, s);
    if (e != hipSuccess) return h->hip("us_hubert_forward: preparing the weights", e);
  }
  const HbPlan p = hb_plan(c, B, Tmax);
  float* base = ws_align(workspace);
  auto W = [&](const std::string& k) { return h->w.at(k).dev; };
  const size_t fh = (size_t)F * H;
  const long long hs_bs = (long long)(n_layers_out + 1) * F * H;
  for (int b0 = 0; b0 < B; b0 += kHbItems) {
    const int nb = std::min(kHbItems, B - b0);
    HbLens lens{};
    for (int i = 0; i < kHbItems; ++i) lens.n[i] = i < nb ? (lengths ? (int)lengths[b0 + i] : Tmax) : (int)field;
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
    // the feature extractor
    float* eb[2] = {base + p.a, base + p.b};
    float* cur = eb[0] + (size_t)b0 * c.conv_dim[0] * Tl[1];
    hipLaunchKernelGGL(hb_conv0_kernel, dim3((Tl[1] + 255) / 256, nb), dim3(256), 0, s, x, stats, W(hb_conv_key(0)), cur, lens, Tmax, c.conv_dim[0],
                       Tl[1]);
    hipLaunchKernelGGL(hb_gn_gelu_kernel, dim3(c.conv_dim[0], nb), dim3(256), 0, s, cur, W("feature_extractor.conv_layers.0.layer_norm.weight"),
                       W("feature_extractor.conv_layers.0.layer_norm.bias"), lens, c.conv_dim[0], Tl[1]);
    for (int i = 1; i < nl; ++i) {
      float* nxt = eb[i & 1] + (size_t)b0 * c.conv_dim[i] * Tl[i + 1];
      HbGemm g{&h->ext[i - 1], cur, nullptr, nullptr, nxt, Tl[i], Tl[i + 1]};
      g.stride = c.conv_stride[i]; g.gelu = 1; g.level = i + 1;
      hb_gemm(s, g, lens, nb);
      cur = nxt;
    }
    // the feature projection
    const int Cl = c.conv_dim[nl - 1];
    float* nrm = eb[nl & 1] + (size_t)b0 * Cl * F;
    hipLaunchKernelGGL(hb_ln_kernel, dim3((F + kLnCols - 1) / kLnCols, nb), dim3(1024), 0, s, cur, (const float*)nullptr,
                       W("feature_projection.layer_norm.weight"), W("feature_projection.layer_norm.bias"), nrm, (float*)nullptr, (float*)nullptr, 0ll,
                       0ll, lens, nl, Cl, F, c.layer_norm_eps);
    float* X0 = base + p.x0 + b0 * fh;
    float* P = base + p.p + b0 * fh;
    float* X = base + p.x + b0 * fh;
    float* X1 = base + p.x1 + b0 * fh;
    float* Y = base + p.y + b0 * fh;
    float* QKV = base + p.qkv + 3 * b0 * fh;
    float* ATT = base + p.att + b0 * fh;
    float* FF = base + p.ff + (size_t)b0 * F * I;
    {
      HbGemm g{&h->proj, nrm, W("feature_projection.projection.bias"), nullptr, X0, F, F};
      g.level = nl;
      hb_gemm(s, g, lens, nb);
    }
    // x + gelu(pos_conv(x)), then the encoder's LayerNorm
    {
      HbGemm g{&h->pos, X0, W("encoder.pos_conv_embed.conv.bias"), X0, P, F, F};
      g.groups = c.pos_conv_groups; g.gelu = 1; g.level = nl;
      hb_gemm(s, g, lens, nb);
    }
    auto ln = [&](const float* in, const float* res, const std::string& key, float* y, int layer) {
      // layer >= 0: the encoder's state after that many layers, which goes to its hidden_states slot and, when it is the last one asked for, to out
      float* e1 = layer >= 0 && hidden_states ? hidden_states + (size_t)b0 * hs_bs + (size_t)layer * fh : nullptr;
      float* e2 = layer == n_layers_out ? out + b0 * fh : nullptr;
      hipLaunchKernelGGL(hb_ln_kernel, dim3((F + kLnCols - 1) / kLnCols, nb), dim3(1024), 0, s, in, res, W(key + ".weight"), W(key + ".bias"), y, e1, e2,
                         hs_bs, (long long)fh, lens, nl, H, F, c.layer_norm_eps);
    };
    ln(P, nullptr, "encoder.layer_norm", X, 0);
    for (int i = 0; i < n_layers_out; ++i) {
      const HbLayer& l = h->layers[i];
      const std::string q = hb_layer_key(i);
      {
        HbGemm g{&l.qkv, X, l.qkv_b, nullptr, QKV, F, F};
        g.nscale = H; g.scale = 1.f / sqrtf((float)h->d); g.level = nl;
        hb_gemm(s, g, lens, nb);
      }
      hb_attn(s, QKV, ATT, lens, nl, H, c.n_heads, h->d, F, nb);
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
  }
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip("us_hubert_forward", e);
}

}  // extern "C"
