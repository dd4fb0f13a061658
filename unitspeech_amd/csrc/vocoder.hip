// BigVGAN vocoder, inference (the reference's unitspeech/vocoder/models.py:169-191 `BigVGAN.forward`, :60-69 `AMPBlock1.forward`,
// activations.py `Snake` / `SnakeBeta`, alias_free_torch/{act,resample,filter}.py `Activation1d`): mel [B][num_mels][T] ->
// waveform [B][1][T * prod(upsample_rates)], exact fp32 throughout (storage, products and sums).
//
// Activations are planar [B][C][T] (time contiguous), the layout the reference's tensors have, so the mel the decoder's
// finish_mel_kernel writes is taken as it is.  Three kernels do the work:
//  - vc_conv_kernel: every dense Conv1d (conv_pre, the AMP convolutions) and every ConvTranspose1d (polyphase form, below) as an
//    implicit GEMM on the fp32 matrix cores (v_mfma_f32_32x32x2_f32): D[co][q] = sum_kk W[co][kk] * X[kk][q] with kk = tap * Cin + ci.
//    The output channel is the MFMA row and time the column, so each of a lane's 16 results goes to a 32-sample run of one channel
//    (coalesced stores).  Epilogue: bias, then the residual (`x = xt + x`, models.py:68), then the AMP-block sum (`xs += ...`,
//    :184-186) and its division by num_kernels (:187) in the reference's order.
//  - vc_act_kernel: one Activation1d (2x up-sampling, Snake / SnakeBeta, low-pass + 2x down-sampling) reading [C][T] once and
//    writing [C][T] once.
//  - vc_post_kernel: conv_post (C -> 1, k = 7) as a per-sample fp32 reduction with the tanh in its epilogue.
//
// Ragged batches (us_vocoder_forward_lengths): each of the three kernels is a template over how it learns an item's length, SameT or
// ItemLens<kVcItems> (item_lens.h; an item's length is at least 1 and at most the padded row stride).  Every read along time is bounded or
// clamped by the item's own length, so nothing at or past an item's end is read and nothing there is written (conv_post alone writes zeros
// over the padded tail of the waveform); the time tiles start where they start when the item runs alone and BigVGAN has no reduction along
// time, so the item's samples have the bits of the uniform call on the item alone.
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

// ---- implicit-GEMM convolution --------------------------------------------------------------------------------------------
// Output step q in [0, Tin) of phase r computes   out[b][co][q * ostride + r] = bias[co] + sum_{j < taps, ci} P_r[j * Cin + ci][co]
// * in[b][ci][q + off[r] + j * dil]   with in[] = 0 outside [0, Tin): the main loop, the pack P and the polyphase form of a
// ConvTranspose1d are conv1d_planar.h's.  128 steps per workgroup: a wave's tile is 32 channels x 64 steps, planar_conv_mainloop<2, 1>
// (two 32-step sub-tiles, one accumulator chain each).
constexpr int kVcBN = 128;    // output steps per workgroup

constexpr int kVcItems = 32;  // batch items per launch of the ragged form (item_lens.h)

struct VcConvArgs {
  const float* in;            // [B][Cin][Tin]
  const float* w;             // [nph][Kpad][ldw]
  const float* bias;          // [Cout]
  const float* res;           // [B][Cout][Tout] added after the bias, or null (may alias out)
  const float* sum;           // [B][Cout][Tout] running AMP sum the result is added to, or null (may alias out)
  float* out;                 // [B][Cout][Tout]
  int Cin, Cout, Tin, Tout;
  int dil, Kdim, Kpad, ldw;
  int nph, ostride;
  float div;                  // > 0: the final value is divided by it (the last AMP block of a level)
  int off[kPcMaxPhases];
};

// Uniform grid: (time tiles, channel tiles, B * phases).  Ragged grid: (time tiles, channel tiles * phases, items of the launch), so the
// batch is not capped by a grid dimension.  Ragged: Tin / Tout are the padded row strides and item b has n = lens.n[b] input steps; the
// main loop takes in[] as zero at or past n, a workgroup whose 128 steps all lie at or past n returns before its first barrier (the
// test is workgroup-uniform), and no step at or past n is stored.
template <class LN>
__global__ __launch_bounds__(256) void vc_conv_kernel(VcConvArgs a, LN lens) {
  PLANAR_LANE(threadIdx.x);
  const int b = LN::ragged ? blockIdx.z : blockIdx.z / a.nph;
  const int mt = LN::ragged ? blockIdx.y / a.nph : blockIdx.y;
  const int ph = LN::ragged ? blockIdx.y - mt * a.nph : blockIdx.z - b * a.nph;
  const int m0 = mt * kPcBM, n0 = blockIdx.x * kVcBN;
  const int nv = lens(b, a.Tin);
  if (LN::ragged && n0 >= nv) return;
  f32x16 acc[2][1];
  planar_conv_mainloop<2, 1, 1, LN::ragged>({a.in + (size_t)b * a.Cin * a.Tin, a.w + (size_t)ph * a.Kpad * a.ldw, a.Cin, a.Tin, a.dil,
                                             a.off[ph], a.Kdim, a.Kpad, a.ldw, m0, n0, nv},
                                            acc);
  float* out = a.out + (size_t)b * a.Cout * a.Tout;        // not __restrict__: res / sum may alias it
  const size_t bo = (size_t)b * a.Cout * a.Tout;
#pragma unroll
  for (int n = 0; n < 2; ++n) {
    const int q = PLANAR_STEP(2, n0, n);
    if (q >= nv) continue;
    const int t = q * a.ostride + ph;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int co = PLANAR_CHANNEL(m0, r);
      if (co >= a.Cout) continue;
      const size_t idx = (size_t)co * a.Tout + t;
      float v = acc[n][0][r] + a.bias[co];
      if (a.res) v = v + a.res[bo + idx];
      if (a.sum) v = a.sum[bo + idx] + v;
      if (a.div > 0.f) v = v / a.div;
      out[idx] = v;
    }
  }
}

// ---- anti-aliased Snake / SnakeBeta (Activation1d with up_ratio = down_ratio = 2, 12-tap filters) ----------------------------
// UpSample1d (resample.py): pad = 12 / 2 - 1 = 5 samples of replicate padding, conv_transpose with stride 2, times 2, crop 15 / 15.
// With x(i) = x[clamp(i, 0, T - 1)] that is, for m in [0, 2T):
//   u[2q]     = 2 * sum_{s < 6} f[2s + 1] * x(q + 2 - s)
//   u[2q + 1] = 2 * sum_{s < 6} f[2s]     * x(q + 3 - s)
// then v = act(u), and LowPassFilter1d(stride 2) replicate-pads v by (5, 6):   out[n] = sum_{j < 12} g[j] * v[clamp(2n + j - 5, 0, 2T - 1)].
// A workgroup makes kActN outputs of one (b, c) row: it stages x(n0 - 6 .. n0 + kActN + 5) and v(clamp(2 n0 - 6 .. 2 n0 + 2 kActN + 5))
// in LDS; every index those formulas touch lies in those windows.
// Uniform grid: (tiles, B * C).  Ragged grid: (tiles, C, items of the launch); T is the padded row stride and the item's n takes its place
// in both replicate clamps (the sequence's last sample is the item's, not the padding's) and in the store bound; a tile at or past n returns.
constexpr int kActN = 256;

template <class LN>
__global__ __launch_bounds__(256) void vc_act_kernel(const float* __restrict__ x, float* __restrict__ out, const float* __restrict__ ab,
                                                     const float* __restrict__ fup, const float* __restrict__ fdown, int C, int Trow, LN lens) {
  __shared__ float xs[kActN + 12];
  __shared__ float vs[2 * kActN + 12];
  __shared__ float f[24];
  const int row = LN::ragged ? blockIdx.z * C + blockIdx.y : blockIdx.y;
  const int c = LN::ragged ? blockIdx.y : row % C;
  const int n0 = blockIdx.x * kActN;
  const int T = lens(LN::ragged ? blockIdx.z : 0, Trow);
  if (LN::ragged && n0 >= T) return;
  const float* __restrict__ xr = x + (size_t)row * Trow;
  if (threadIdx.x < 12) {
    f[threadIdx.x] = fup[threadIdx.x];
    f[12 + threadIdx.x] = fdown[threadIdx.x];
  }
  for (int i = threadIdx.x; i < kActN + 12; i += blockDim.x) xs[i] = xr[min(max(n0 - 6 + i, 0), T - 1)];
  __syncthreads();
  const float alpha = ab[c], inv = ab[C + c];
  for (int i = threadIdx.x; i < 2 * kActN + 12; i += blockDim.x) {
    const int m = min(max(2 * n0 - 6 + i, 0), 2 * T - 1);
    const int q = m >> 1, odd = m & 1;
    const float* xq = xs + (q - n0 + 6) + 2 + odd;        // x(q + 2 + odd - s) = xq[-s]
    float acc = 0.f;
#pragma unroll
    for (int s = 0; s < 6; ++s) acc = fmaf(f[2 * s + 1 - odd], xq[-s], acc);
    const float uval = 2.f * acc;
    const float sn = sinf(mul_rn(uval, alpha));
    vs[i] = add_rn(uval, mul_rn(inv, mul_rn(sn, sn)));    // x + 1 / (beta + 1e-9) * sin(x alpha)^2, each op rounded as in activations.py
  }
  __syncthreads();
  for (int l = threadIdx.x; l < kActN; l += blockDim.x) {
    if (n0 + l >= T) break;
    float acc = 0.f;
#pragma unroll
    for (int j = 0; j < 12; ++j) acc = fmaf(f[12 + j], vs[2 * l + j + 1], acc);
    out[(size_t)row * Trow + n0 + l] = acc;
  }
}

// alpha / beta of one Snake(Beta) module -> ab[0][c] = alpha' (exp(alpha) with snake_logscale), ab[1][c] = 1 / (beta' + 1e-9);
// `which` 0: from alpha (Snake fills both halves from it), 1: beta (SnakeBeta's second parameter)
__global__ void vc_snake_param_kernel(const float* __restrict__ p, float* __restrict__ ab, int C, int which, int both, int logscale) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= C) return;
  const float v = logscale ? expf(p[c]) : p[c];
  if (which == 0) ab[c] = v;
  if (which == 1 || both) ab[C + c] = 1.f / (v + 1e-9f);
}

// ---- conv_post: Conv1d(C, 1, 7, padding 3) + tanh --------------------------------------------------------------------------------
constexpr int kPostK = 7;

// Ragged: Trow is the padded row stride, the item's n takes T's place in the zero padding, and the samples on [n, Trow) are written as
// 0.0f, so the whole returned waveform is defined.
template <class LN>
__global__ __launch_bounds__(256) void vc_post_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                      float* __restrict__ out, int C, int Trow, LN lens) {
  extern __shared__ float ws[];
  for (int i = threadIdx.x; i < C * kPostK; i += blockDim.x) ws[i] = w[i];
  __syncthreads();
  const int b = blockIdx.y, t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= Trow) return;
  const int T = lens(b, Trow);
  if (LN::ragged && t >= T) {
    out[(size_t)b * Trow + t] = 0.f;
    return;
  }
  const float* __restrict__ xb = x + (size_t)b * C * Trow;
  float acc = 0.f;
  for (int ci = 0; ci < C; ++ci) {
    const float* xr = xb + (size_t)ci * Trow;
#pragma unroll
    for (int j = 0; j < kPostK; ++j) {
      const int tt = t + j - kPostK / 2;
      if (tt >= 0 && tt < T) acc = fmaf(ws[ci * kPostK + j], xr[tt], acc);
    }
  }
  out[(size_t)b * Trow + t] = tanhf(acc + bias[0]);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

struct VcAct {                  // one Activation1d
  std::string prefix;
  int C = 0;
  float* ab = nullptr;          // [2][C]
};

}  // namespace
}  // namespace us

struct us_vocoder : us::WeightTable {      // keys: the remove_weight_norm form
  us_vocoder_config cfg{};
  std::map<std::string, us::PlanarConv> conv;
  std::map<std::string, us::VcAct> act;
};

namespace us {
namespace {

void vc_add_conv(us_vocoder* h, const std::string& p, int cin, int cout, int k, int dil) {
  h->add(p + ".weight", {cout, cin, k});
  h->add(p + ".bias", {cout});
  h->conv[p].conv(cin, cin, cout, k, dil);
}

void vc_add_up(us_vocoder* h, const std::string& p, int cin, int cout, int k, int u) {
  h->add(p + ".weight", {cin, cout, k});      // ConvTranspose1d weight layout [in, out, k]
  h->add(p + ".bias", {cout});
  h->conv[p].transposed(cin, cout, k, u);
}

void vc_add_act(us_vocoder* h, const std::string& p, int C) {
  h->add(p + ".act.alpha", {C});
  if (h->cfg.activation == US_VOCODER_SNAKEBETA) h->add(p + ".act.beta", {C});
  h->add(p + ".upsample.filter", {1, 1, 12});
  h->add(p + ".downsample.lowpass.filter", {1, 1, 12});
  VcAct& a = h->act[p];
  a.prefix = p; a.C = C;
}

int channels(const us_vocoder_config& c, int level) { return c.upsample_initial_channel >> level; }   // after up-sampler `level - 1`

// module registration order of models.py:125-165, remove_weight_norm() form
void vocoder_keys(us_vocoder* h) {
  const auto& c = h->cfg;
  vc_add_conv(h, "conv_pre", c.num_mels, c.upsample_initial_channel, 7, 1);
  for (int i = 0; i < c.n_up; ++i)
    vc_add_up(h, "ups." + std::to_string(i) + ".0", channels(c, i), channels(c, i + 1), c.upsample_kernel_sizes[i], c.upsample_rates[i]);
  for (int i = 0; i < c.n_up; ++i)
    for (int j = 0; j < c.n_kernels; ++j) {
      const std::string p = "resblocks." + std::to_string(i * c.n_kernels + j);
      const int ch = channels(c, i + 1), k = c.resblock_kernel_sizes[j];
      for (int l = 0; l < 3; ++l) vc_add_conv(h, p + ".convs1." + std::to_string(l), ch, ch, k, c.resblock_dilation_sizes[j][l]);
      for (int l = 0; l < 3; ++l) vc_add_conv(h, p + ".convs2." + std::to_string(l), ch, ch, k, 1);
      for (int a = 0; a < 6; ++a) vc_add_act(h, p + ".activations." + std::to_string(a), ch);
    }
  const int ch = channels(c, c.n_up);
  vc_add_act(h, "activation_post", ch);
  h->add("conv_post.weight", {1, ch, kPostK});
  h->add("conv_post.bias", {1});
}

long long vc_hop(const us_vocoder_config& c) {
  long long hop = 1;
  for (int i = 0; i < c.n_up; ++i) hop *= c.upsample_rates[i];
  return hop;
}

// largest C * T of any activation per batch item (conv_pre's output or a level's), in floats
long long vc_max_ct(const us_vocoder_config& c, int T) {
  long long m = (long long)c.upsample_initial_channel * T, t = T;
  for (int i = 0; i < c.n_up; ++i) {
    t *= c.upsample_rates[i];
    m = std::max(m, (long long)channels(c, i + 1) * t);
  }
  return m;
}

constexpr int kVcBuffers = 5;      // level input, AMP sum, residual stream, activation output, first-conv output

// Ragged launches: `lengths` counts item b's steps in units of which this level has `rate` each; the time tiles cover the group's longest item
void conv(us_vocoder* h, hipStream_t s, const std::string& p, const float* in, float* out, const float* res, const float* sum, float div,
          int B, int Tin, const int64_t* lengths = nullptr, long long rate = 1) {
  const PlanarConv& c = h->conv.at(p);
  VcConvArgs a{};
  a.in = in; a.w = c.packed; a.bias = h->w.at(p + ".bias").dev; a.res = res; a.sum = sum; a.out = out;
  a.Cin = c.cin; a.Cout = c.cout; a.Tin = Tin; a.Tout = Tin * c.nph;
  a.dil = c.dil; a.Kdim = c.Kdim(); a.Kpad = c.Kpad; a.ldw = c.ldw;
  a.nph = c.nph; a.ostride = c.nph; a.div = div;
  for (int r = 0; r < c.nph; ++r) a.off[r] = c.off[r];
  const int mt = (c.cout + kPcBM - 1) / kPcBM;
  if (!lengths) {
    hipLaunchKernelGGL(vc_conv_kernel<SameT>, dim3((Tin + kVcBN - 1) / kVcBN, mt, B * c.nph), dim3(256), 0, s, a, SameT{});
    return;
  }
  for_item_groups<kVcItems>(B, [&](int b) { return lengths[b] * rate; }, [&](int b0, int nb, const ItemLens<kVcItems>& lens, int longest) {
    VcConvArgs g = a;
    const size_t io = (size_t)b0 * c.cin * Tin, oo = (size_t)b0 * c.cout * a.Tout;
    g.in = in + io; g.out = out + oo;
    if (res) g.res = res + oo;
    if (sum) g.sum = sum + oo;
    hipLaunchKernelGGL(vc_conv_kernel<ItemLens<kVcItems>>, dim3((longest + kVcBN - 1) / kVcBN, mt * c.nph, nb), dim3(256), 0, s, g, lens);
  });
}

void activation(us_vocoder* h, hipStream_t s, const std::string& p, const float* in, float* out, int B, int T,
                const int64_t* lengths = nullptr, long long rate = 1) {
  const VcAct& a = h->act.at(p);
  const float* fup = h->w.at(p + ".upsample.filter").dev;
  const float* fdown = h->w.at(p + ".downsample.lowpass.filter").dev;
  if (!lengths) {
    hipLaunchKernelGGL(vc_act_kernel<SameT>, dim3((T + kActN - 1) / kActN, B * a.C), dim3(256), 0, s, in, out, a.ab, fup, fdown, a.C, T,
                       SameT{});
    return;
  }
  for_item_groups<kVcItems>(B, [&](int b) { return lengths[b] * rate; }, [&](int b0, int nb, const ItemLens<kVcItems>& lens, int longest) {
    const size_t o = (size_t)b0 * a.C * T;
    hipLaunchKernelGGL(vc_act_kernel<ItemLens<kVcItems>>, dim3((longest + kActN - 1) / kActN, a.C, nb), dim3(256), 0, s, in + o, out + o, a.ab, fup,
                       fdown, a.C, T, lens);
  });
}

void post(us_vocoder* h, hipStream_t s, const float* in, float* out, int B, int T, const int64_t* lengths = nullptr, long long rate = 1) {
  const int ch = channels(h->cfg, h->cfg.n_up);
  const size_t lds = (size_t)ch * kPostK * sizeof(float);
  const float* w = h->w.at("conv_post.weight").dev;
  const float* bias = h->w.at("conv_post.bias").dev;
  if (!lengths) {
    hipLaunchKernelGGL(vc_post_kernel<SameT>, dim3((T + 255) / 256, B), dim3(256), lds, s, in, w, bias, out, ch, T, SameT{});
    return;
  }
  // every tile of the padded row is launched: the ones past an item's end write its zeros
  for_item_groups<kVcItems>(B, [&](int b) { return lengths[b] * rate; }, [&](int b0, int nb, const ItemLens<kVcItems>& lens, int) {
    hipLaunchKernelGGL(vc_post_kernel<ItemLens<kVcItems>>, dim3((T + 255) / 256, nb), dim3(256), lds, s, in + (size_t)b0 * ch * T, w, bias,
                       out + (size_t)b0 * T, ch, T, lens);
  });
}

// "", or a refusal that names the first item whose length is outside [1, Tmax]
std::string vc_bad_length(const char* what, const int64_t* lengths, int B, int Tmax, const char* tname) {
  const std::string bad = bad_length(what, lengths, B, 1, Tmax);
  return bad.empty() ? bad : bad + " must be at least 1 and at most " + tname + " = " + std::to_string(Tmax);
}

// BigVGAN.forward (models.py:169-191); lengths null: every item has T frames
int vc_forward(us_vocoder* h, const char* what, const float* mel, const int64_t* lengths, float* wav, int B, int T, void* workspace,
               size_t workspace_bytes, us_stream stream) {
  const std::string name(what);
  const auto& c = h->cfg;
  const long long hop = vc_hop(c);
  if (vc_max_ct(c, T) >= (1ll << 31) || (long long)T * hop >= (1ll << 31))
    return h->fail(US_EINVAL, name + ": B * channels or T * hop too large");
  // the uniform launches number the (item, channel) and (item, phase) pairs along one grid dimension; the ragged ones give the item its own
  if (!lengths && ((long long)B * c.upsample_initial_channel > 65535 || (long long)B * kPcMaxPhases > 65535))
    return h->fail(US_EINVAL, name + ": B * channels or T * hop too large");
  const int rc = h->all_loaded(what);
  if (rc != US_OK) return rc;
  if (!workspace || workspace_bytes < us_vocoder_workspace_bytes(h, B, T))
    return h->fail(US_EWORKSPACE, name + ": workspace too small (us_vocoder_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const size_t slab = (size_t)B * (size_t)vc_max_ct(c, T);
  float* X = ws_align(workspace);     // level input (the up-sampler's output)
  float* S = X + slab;           // level output: the AMP-block sum (conv_pre writes here too)
  float* R = S + slab;           // residual stream x_l of the running AMP block (l = 1, 2)
  float* A = R + slab;           // Activation1d output
  float* H = A + slab;           // output of the block's first convolution
  const int64_t* ln = lengths;
  conv(h, s, "conv_pre", mel, S, nullptr, nullptr, 0.f, B, T, ln, 1);
  int t = T;
  long long r = 1;                    // steps per mel frame at this level
  for (int i = 0; i < c.n_up; ++i) {
    conv(h, s, "ups." + std::to_string(i) + ".0", S, X, nullptr, nullptr, 0.f, B, t, ln, r);
    t *= c.upsample_rates[i];
    r *= c.upsample_rates[i];
    for (int j = 0; j < c.n_kernels; ++j) {
      // AMPBlock1.forward (models.py:60-69): x_{l+1} = c2(a2(c1(a1(x_l)))) + x_l, x_0 = the level input
      const std::string p = "resblocks." + std::to_string(i * c.n_kernels + j);
      const float* xl = X;
      for (int l = 0; l < 3; ++l) {
        const std::string ls = std::to_string(l);
        activation(h, s, p + ".activations." + std::to_string(2 * l), xl, A, B, t, ln, r);
        conv(h, s, p + ".convs1." + ls, A, H, nullptr, nullptr, 0.f, B, t, ln, r);
        activation(h, s, p + ".activations." + std::to_string(2 * l + 1), H, A, B, t, ln, r);
        if (l < 2) {
          conv(h, s, p + ".convs2." + ls, A, R, xl, nullptr, 0.f, B, t, ln, r);
          xl = R;
        } else {        // the block's output goes straight into the level sum: xs (+)= x_3, then / num_kernels (:180-187)
          conv(h, s, p + ".convs2." + ls, A, S, xl, j > 0 ? S : nullptr, j == c.n_kernels - 1 ? (float)c.n_kernels : 0.f, B, t, ln, r);
        }
      }
    }
  }
  activation(h, s, "activation_post", S, A, B, t, ln, r);
  post(h, s, A, wav, B, t, ln, r);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip(what, e);
}

}  // namespace
}  // namespace us

extern "C" {

using namespace us;

int us_vocoder_create(us_vocoder_handle* out, const us_vocoder_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: null argument");
  const auto& c = *cfg;
  if (c.resblock != 1)
    return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: only resblock \"1\" (AMPBlock1) is built; AMPBlock2 is not");
  if (c.activation != US_VOCODER_SNAKE && c.activation != US_VOCODER_SNAKEBETA)
    return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: activation must be snake or snakebeta");
  if (c.num_mels <= 0 || c.num_mels > 4096 || c.upsample_initial_channel <= 0 || c.upsample_initial_channel > 8192 || c.n_up <= 0 ||
      c.n_up > 8 || c.n_kernels <= 0 || c.n_kernels > 4 || c.snake_logscale < 0 || c.snake_logscale > 1)
    return WeightTable::fail(nullptr, US_EINVAL,
                             "us_vocoder_create: bad num_mels / upsample_initial_channel / number of up-samplers or kernels");
  if (c.upsample_initial_channel % (1 << c.n_up) != 0)
    return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: upsample_initial_channel must be divisible by 2^len(upsample_rates)");
  for (int i = 0; i < c.n_up; ++i) {
    const int u = c.upsample_rates[i], k = c.upsample_kernel_sizes[i];
    if (u <= 0 || u > kPcMaxPhases || k < u || k % u != 0 || (k - u) % 2 != 0)
      return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: up-sampler " + std::to_string(i) +
                                                       ": rate in [1, 16] and kernel a multiple of the rate with (kernel - rate) even are built");
  }
  for (int j = 0; j < c.n_kernels; ++j) {
    const int k = c.resblock_kernel_sizes[j];
    if (k <= 0 || k > 31 || k % 2 == 0)
      return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: resblock kernel sizes must be odd and at most 31");
    for (int l = 0; l < 3; ++l)
      if (c.resblock_dilation_sizes[j][l] <= 0 || c.resblock_dilation_sizes[j][l] > 64)
        return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: resblock dilations must be in [1, 64]");
  }
  if ((size_t)(c.upsample_initial_channel >> c.n_up) * kPostK * sizeof(float) > 48 * 1024)
    return WeightTable::fail(nullptr, US_EINVAL, "us_vocoder_create: too many channels at conv_post");
  auto* h = new us_vocoder();
  h->cfg = c;
  (void)hipGetDevice(&h->device);
  vocoder_keys(h);
  *out = h;
  return US_OK;
}

int us_vocoder_destroy(us_vocoder_handle h) {
  if (!h) return US_OK;
  h->free_weights();
  for (auto& kv : h->conv) kv.second.release();
  for (auto& kv : h->act)
    if (kv.second.ab) (void)hipFree(kv.second.ab);
  delete h;
  return US_OK;
}

int us_vocoder_num_weights(us_vocoder_handle h) { return h ? h->num() : 0; }
const char* us_vocoder_weight_key(us_vocoder_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_vocoder_last_error(us_vocoder_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_vocoder_load_weight(us_vocoder_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  hipStream_t s = static_cast<hipStream_t>(stream);
  Weight* wp;
  const int rc = WeightTable::load(h, "us_vocoder_load_weight", key, data, shape, ndim, s, &wp);
  if (rc != US_OK) return rc;
  Weight& w = *wp;
  hipError_t e;
  const std::string k(key);
  const auto dot = k.rfind('.');
  const std::string prefix = k.substr(0, dot), leaf = k.substr(dot + 1);
  auto ci = h->conv.find(prefix);
  if (ci != h->conv.end() && leaf == "weight") {
    PlanarConv& c = ci->second;
    if (!c.packed && (e = hipMalloc(&c.packed, c.packed_floats() * sizeof(float))) != hipSuccess) return h->hip("hipMalloc(packed weight)", e);
    c.pack(w.dev, s);
  }
  const auto adot = prefix.rfind('.');
  if (adot != std::string::npos && prefix.substr(adot + 1) == "act" && (leaf == "alpha" || leaf == "beta")) {
    VcAct& a = h->act.at(prefix.substr(0, adot));
    if (!a.ab && (e = hipMalloc(&a.ab, 2 * (size_t)a.C * sizeof(float))) != hipSuccess) return h->hip("hipMalloc(snake parameters)", e);
    const bool snake = h->cfg.activation == US_VOCODER_SNAKE;
    hipLaunchKernelGGL(vc_snake_param_kernel, dim3((a.C + 255) / 256), dim3(256), 0, s, w.dev, a.ab, a.C, leaf == "alpha" ? 0 : 1, snake ? 1 : 0,
                       h->cfg.snake_logscale ? 1 : 0);
  }
  if ((e = hipGetLastError()) != hipSuccess) return h->hip("us_vocoder_load_weight", e);
  w.loaded = true;
  return US_OK;
}

size_t us_vocoder_workspace_bytes(us_vocoder_handle h, int B, int T) {
  if (!h || B <= 0 || T <= 0) return 0;
  return (size_t)kVcBuffers * (size_t)B * (size_t)vc_max_ct(h->cfg, T) * sizeof(float) + 256;
}

int us_vocoder_forward(us_vocoder_handle h, const float* mel, float* wav, int B, int T, void* workspace, size_t workspace_bytes,
                       us_stream stream) {
  if (!h || !mel || !wav || B <= 0 || T <= 0) return WeightTable::fail(h, US_EINVAL, "us_vocoder_forward: bad argument");
  return vc_forward(h, "us_vocoder_forward", mel, nullptr, wav, B, T, workspace, workspace_bytes, stream);
}

int us_vocoder_forward_lengths(us_vocoder_handle h, const float* mel, const int64_t* lengths, float* wav, int B, int Tmax, void* workspace,
                               size_t workspace_bytes, us_stream stream) {
  if (!h || !mel || !wav || B <= 0 || Tmax <= 0) return WeightTable::fail(h, US_EINVAL, "us_vocoder_forward_lengths: bad argument");
  if (!lengths)
    return h->fail(US_EINVAL, "us_vocoder_forward_lengths: lengths is null (B host values in [1, Tmax]; us_vocoder_forward is the uniform call)");
  const std::string bad = vc_bad_length("us_vocoder_forward_lengths", lengths, B, Tmax, "Tmax");
  if (!bad.empty()) return h->fail(US_EINVAL, bad);
  return vc_forward(h, "us_vocoder_forward_lengths", mel, lengths, wav, B, Tmax, workspace, workspace_bytes, stream);
}

}  // extern "C"

namespace us {
namespace {

// one layer alone; lengths null: every item has Tin steps
int vc_debug_layer(us_vocoder* h, const char* what, const char* prefix, const float* in, const float* res, const float* sum, float div,
                   float* out, int B, int Tin, const int64_t* lengths, us_stream stream) {
  const std::string name(what), p(prefix);
  const auto ci = h->conv.find(p);
  const bool is_act = h->act.count(p) != 0, is_post = p == "conv_post";
  if (ci == h->conv.end() && !is_act && !is_post) return h->fail(US_ENOKEY, name + ": unknown layer '" + p + "'");
  if (ci == h->conv.end() && (res || sum || div != 0.f))
    return h->fail(US_EINVAL, name + ": res / sum / div belong to a convolution's epilogue; '" + p + "' is not one");
  // the largest C * T this layer reads or writes, under us_vocoder_forward's limits
  long long ct;
  if (ci != h->conv.end())
    ct = std::max((long long)ci->second.cin * Tin, (long long)ci->second.cout * Tin * ci->second.nph);
  else
    ct = (long long)(is_act ? h->act.at(p).C : channels(h->cfg, h->cfg.n_up)) * Tin;
  if (ct >= (1ll << 31) || (!lengths && ((long long)B * h->cfg.upsample_initial_channel > 65535 || (long long)B * kPcMaxPhases > 65535)))
    return h->fail(US_EINVAL, name + ": B * channels or C * T too large");
  const int rc = h->all_loaded(what);
  if (rc != US_OK) return rc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (ci != h->conv.end())
    conv(h, s, p, in, out, res, sum, div, B, Tin, lengths, 1);
  else if (is_act)
    activation(h, s, p, in, out, B, Tin, lengths, 1);
  else
    post(h, s, in, out, B, Tin, lengths, 1);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip(what, e);
}

}  // namespace
}  // namespace us

extern "C" {

int us_vocoder_debug_layer(us_vocoder_handle h, const char* prefix, const float* in, const float* res, const float* sum, float div, float* out,
                           int B, int Tin, us_stream stream) {
  if (!h || !prefix || !in || !out || B <= 0 || Tin <= 0 || !(div >= 0.f))
    return WeightTable::fail(h, US_EINVAL, "us_vocoder_debug_layer: bad argument");
  return vc_debug_layer(h, "us_vocoder_debug_layer", prefix, in, res, sum, div, out, B, Tin, nullptr, stream);
}

int us_vocoder_debug_layer_lengths(us_vocoder_handle h, const char* prefix, const float* in, const float* res, const float* sum, float div,
                                   float* out, int B, int Tin_max, const int64_t* lengths, us_stream stream) {
  if (!h || !prefix || !in || !out || B <= 0 || Tin_max <= 0 || !(div >= 0.f))
    return WeightTable::fail(h, US_EINVAL, "us_vocoder_debug_layer_lengths: bad argument");
  if (!lengths) return h->fail(US_EINVAL, "us_vocoder_debug_layer_lengths: lengths is null (B host values in [1, Tin_max])");
  const std::string bad = vc_bad_length("us_vocoder_debug_layer_lengths", lengths, B, Tin_max, "Tin_max");
  if (!bad.empty()) return h->fail(US_EINVAL, bad);
  return vc_debug_layer(h, "us_vocoder_debug_layer_lengths", prefix, in, res, sum, div, out, B, Tin_max, lengths, stream);
}

}  // extern "C"
