// Training side of the `DurationPredictor` (unitspeech/duration_predictor.py:47-63 in train mode):
//   x    = cat(detach(x), g^T repeated over L)                        no gradient leaves through x or g
//   h1   = drop(LayerNorm(relu(conv_1(x  * mask))))                   eps 1e-5; the ReLU comes BEFORE the LayerNorm, the Dropout AFTER it
//   h2   = drop(LayerNorm(relu(conv_2(h1 * mask))))
//   logw = proj(h2 * mask) * mask
// and the reverse=False loss sum((logw - log(w + 1e-6) * mask)^2) / sum(mask) (:60-62).
//
// Layout: channel-last [B][L][C] (row = b * L + l), as in frontend.hip.  conv_1 and conv_2 are the fp32-MFMA implicit GEMM of
// encoder_train.hip (forward, weight gradient, and conv_2's data gradient; conv_1's data gradient is never computed: the reference
// detaches x, and g gets no gradient here).  Everything between the GEMMs is two kernel forms, one wave per symbol:
//   dt_norm_fwd_kernel   LayerNorm + dropout of a symbol's channels; the head form goes on to the mask and the dot product with
//                        proj.weight (one output channel: a 64x64 MFMA tile would waste 63 columns), writing logw directly
//   dt_norm_bwd_kernel   regenerates the dropout factor, takes the upstream gradient (the head form builds it from grad_logw and
//                        proj.weight, the other reads conv_2's data gradient) through the LayerNorm and the ReLU gate, writes the
//                        convolution's output gradient and the per-chunk partial sums of gamma, beta, the convolution's bias and,
//                        in the head form, proj.weight and proj.bias
// Forward: 5 kernels (cat, conv_1, norm_1, conv_2, head) and one device copy of the mask into the tape.  Backward: 10 kernels (head
// backward, its sums; conv_2 weight gradient + its split sum, flipped-weight pack + data gradient; norm_1 backward, its sums; conv_1
// weight gradient + its split sum).
//
// Every reduction is a fixed-order two-pass sum (a workgroup owns a contiguous chunk of rows, its four waves walk it with stride 4
// and meet in LDS in wave order; a second kernel adds the chunks in order): no atomics, two runs give the same bits.  Dropout is
// frontend.h's stream: site 0 follows norm_1, site 1 follows norm_2, flat index of the reference's [B][filter_channels][L] tensor.
#include <hip/hip_runtime.h>

#include <cmath>
#include <map>
#include <string>

#include "../../include/unitspeech_hip.h"
#include "frontend.h"
#include "kernels.h"

namespace us {
namespace {

constexpr float kDtEps = 1e-5f;          // duration_predictor.py:10
constexpr int kDtChunks = 256;           // row chunks of the backward's partial sums
constexpr int kDtSums = 4;               // gamma, beta, conv bias, proj.weight

// mean and 1 / sqrt(var + eps) of one symbol's channels, the arithmetic of fe_layernorm_kernel
template <int kPer>
__device__ __forceinline__ void dt_stats(const float* v, int lane, int F, float& mean, float& rstd) {
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kPer; ++i)
    if (lane + 64 * i < F) s += v[i];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  mean = s / (float)F;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kPer; ++i)
    if (lane + 64 * i < F) { const float d = sub_rn(v[i], mean); q = __builtin_fmaf(d, d, q); }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  rstd = 1.f / sqrtf(add_rn(q / (float)F, kDtEps));
}

struct DtFwdArgs {
  const float* r;                       // [rows][F] relu(conv(.))
  const float* gamma; const float* beta;
  const float* mask;                    // [rows]
  const float* pw; const float* pb;     // head: proj.weight [F], proj.bias [1]
  float* out;                           // head: logw [rows]; else drop(LN(r)) [rows][F]
  long long rows;
  int F, L;
  Drop drop;
};

// out = drop(LN(r)); head: logw = (sum_c pw[c] * (out[c] * mask) + pb) * mask.  One wave per symbol, four symbols per workgroup.
template <int kPer, bool kHead>
__global__ void __launch_bounds__(256) dt_norm_fwd_kernel(DtFwdArgs a) {
  const int lane = threadIdx.x & 63;
  const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= a.rows) return;
  float v[kPer];
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int c = lane + 64 * i;
    v[i] = c < a.F ? a.r[row * a.F + c] : 0.f;
  }
  float mean, rstd;
  dt_stats<kPer>(v, lane, a.F, mean, rstd);
  const float m = a.mask[row];
  float dot = 0.f;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int c = lane + 64 * i;
    if (c < a.F) {
      float y = add_rn(mul_rn(mul_rn(sub_rn(v[i], mean), rstd), a.gamma[c]), a.beta[c]);
      y *= et_keep(a.drop, et_cf_index(row, c, a.F, a.L));
      if (kHead) dot = __builtin_fmaf(mul_rn(y, m), a.pw[c], dot);
      else a.out[row * a.F + c] = y;
    }
  }
  if (kHead) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) dot += __shfl_xor(dot, o, 64);
    if (lane == 0) a.out[row] = mul_rn(add_rn(dot, a.pb[0]), m);
  }
}

struct DtBwdArgs {
  const float* r;                       // [rows][F] relu(conv(.)): the LayerNorm's input and the ReLU gate
  const float* gamma; const float* beta;
  const float* mask;                    // [rows]
  const float* dy;                      // !head: [rows][F] gradient of drop(LN(r))
  const float* glogw;                   // head: [rows] gradient of logw
  const float* pw;                      // head: proj.weight [F]
  float* dc;                            // [rows][F] gradient of the convolution's output
  float* part;                          // [kDtChunks][kDtSums][F]
  float* part_b;                        // [kDtChunks] (head: proj.bias)
  long long rows;
  int per;                              // rows per chunk
  int F, L;
  Drop drop;
};

// One workgroup per chunk of `per` rows; wave w takes rows lo + w, lo + w + 4, ... (one wave per symbol) and keeps the column sums of
// its rows in registers.  The four waves' sums meet in LDS and are added in wave order.
template <int kPer, bool kHead>
__global__ void __launch_bounds__(256) dt_norm_bwd_kernel(DtBwdArgs a) {
  __shared__ float red[4][kPer * 64];
  __shared__ float red_b[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const long long lo = (long long)blockIdx.x * a.per;
  const long long hi = lo + a.per < a.rows ? lo + a.per : a.rows;
  float sg[kPer], sb[kPer], sc[kPer], sw[kPer], gam[kPer], bet[kPer], pwv[kPer];
  float spb = 0.f;
#pragma unroll
  for (int i = 0; i < kPer; ++i) {
    const int c = lane + 64 * i;
    sg[i] = sb[i] = sc[i] = sw[i] = 0.f;
    gam[i] = c < a.F ? a.gamma[c] : 0.f;
    bet[i] = (kHead && c < a.F) ? a.beta[c] : 0.f;
    pwv[i] = (kHead && c < a.F) ? a.pw[c] : 0.f;
  }
  for (long long row = lo + wave; row < hi; row += 4) {
    float v[kPer], g[kPer];
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int c = lane + 64 * i;
      v[i] = c < a.F ? a.r[row * a.F + c] : 0.f;
    }
    float mean, rstd;
    dt_stats<kPer>(v, lane, a.F, mean, rstd);
    float gl = 0.f, glm = 0.f;
    if (kHead) {
      const float m = a.mask[row];
      gl = a.glogw[row] * m;            // logw = (.) * mask
      glm = gl * m;                     // proj reads h2 * mask
      spb += gl;
    }
    float s1 = 0.f, s2 = 0.f;           // sum dxhat, sum dxhat * xhat
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int c = lane + 64 * i;
      g[i] = 0.f;
      if (c < a.F) {
        const float xh = (v[i] - mean) * rstd;
        const float keep = et_keep(a.drop, et_cf_index(row, c, a.F, a.L));
        float d;                        // gradient of LN(r)[c]
        if (kHead) {
          sw[i] += glm * ((xh * gam[i] + bet[i]) * keep);
          d = glm * pwv[i] * keep;
        } else {
          d = a.dy[row * a.F + c] * keep;
        }
        sg[i] += d * xh;
        sb[i] += d;
        const float dxh = d * gam[i];
        g[i] = dxh;
        s1 += dxh;
        s2 += dxh * xh;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
    s1 /= (float)a.F;
    s2 /= (float)a.F;
#pragma unroll
    for (int i = 0; i < kPer; ++i) {
      const int c = lane + 64 * i;
      if (c < a.F) {
        const float xh = (v[i] - mean) * rstd;
        const float dx = v[i] > 0.f ? rstd * (g[i] - s1 - xh * s2) : 0.f;      // the ReLU's gate: r > 0 iff conv > 0
        sc[i] += dx;
        a.dc[row * a.F + c] = dx;
      }
    }
  }
  // the four waves' column sums, added in wave order
  auto meet = [&](const float* mine, int q) {
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kPer; ++i) red[wave][lane + 64 * i] = mine[i];
    __syncthreads();
    if (wave == 0) {
#pragma unroll
      for (int i = 0; i < kPer; ++i) {
        const int c = lane + 64 * i;
        if (c < a.F) a.part[((long long)blockIdx.x * kDtSums + q) * a.F + c] = ((red[0][c] + red[1][c]) + red[2][c]) + red[3][c];
      }
    }
  };
  meet(sg, 0);
  meet(sb, 1);
  meet(sc, 2);
  if (kHead) {
    meet(sw, 3);
    if (lane == 0) red_b[wave] = spb;
    __syncthreads();
    if (threadIdx.x == 0) a.part_b[blockIdx.x] = ((red_b[0] + red_b[1]) + red_b[2]) + red_b[3];
  }
}

struct DtSumArgs {
  const float* part; const float* part_b;
  float* dst[kDtSums];                  // gamma, beta, conv bias, proj.weight (null: not this form)
  float* dst_b;                         // proj.bias (null: not this form)
  int F;
};
// dst[q][c] = sum over chunks, in order, of part[chunk][q][c] (accumulated in fp64, rounded once)
__global__ void dt_sum_kernel(DtSumArgs a) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e < kDtSums * a.F) {
    const int q = e / a.F, c = e - q * a.F;
    if (!a.dst[q]) return;
    double s = 0.0;
    for (int k = 0; k < kDtChunks; ++k) s += (double)a.part[((long long)k * kDtSums + q) * a.F + c];
    a.dst[q][c] = (float)s;
  } else if (e == kDtSums * a.F && a.dst_b) {
    double s = 0.0;
    for (int k = 0; k < kDtChunks; ++k) s += (double)a.part_b[k];
    a.dst_b[0] = (float)s;
  }
}

// duration_predictor.py:60-62 and d loss / d logw.  One workgroup, fixed strided sums in fp64 and a fixed tree: deterministic.
__global__ __launch_bounds__(256) void dt_mse_loss_kernel(const float* __restrict__ logw, const float* __restrict__ w,
                                                          const float* __restrict__ mask, float* __restrict__ loss,
                                                          float* __restrict__ d_logw, int n) {
  __shared__ double red[2][256];
  double s = 0.0, ms = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) {
    const double d = (double)logw[i] - (double)(logf(w[i] + 1e-6f) * mask[i]);
    s += d * d;
    ms += (double)mask[i];
  }
  red[0][threadIdx.x] = s;
  red[1][threadIdx.x] = ms;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      red[0][threadIdx.x] += red[0][threadIdx.x + o];
      red[1][threadIdx.x] += red[1][threadIdx.x + o];
    }
    __syncthreads();
  }
  const double den = red[1][0];
  if (threadIdx.x == 0) loss[0] = (float)(red[0][0] / den);
  if (!d_logw) return;
  for (int i = threadIdx.x; i < n; i += 256)
    d_logw[i] = (float)(2.0 * ((double)logw[i] - (double)(logf(w[i] + 1e-6f) * mask[i])) / den);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

// workspace of one training forward (the tape) and of its backward, in floats from a 256-byte aligned base
struct DtLayout {
  size_t xin, mask, r1, h1, r2, tape_end;
  size_t dc, dh, wd, wpart, part, part_b, arena, total;
};

DtLayout dt_layout(const us_frontend* h, int B, int L) {
  const auto& c = h->dc;
  const size_t rows = (size_t)B * L, F = c.filter_channels, Cin = (size_t)c.in_channels + c.spk_emb_dim, K = c.kernel_size;
  DtLayout o{};
  WsTake take;
  o.xin = take(rows * Cin); o.mask = take(rows); o.r1 = take(rows * F); o.h1 = take(rows * F); o.r2 = take(rows * F);
  o.tape_end = take.total;
  o.dc = take(rows * F); o.dh = take(rows * F);
  o.wd = take(F * F * K);
  o.wpart = take((size_t)wgrad_splits((long long)rows) * F * std::max(F, Cin) * K);
  o.part = take((size_t)kDtChunks * kDtSums * F);
  o.part_b = take(kDtChunks);
  o.arena = take(h->total_numel());
  o.total = take.total;
  return o;
}

int dt_check(us_frontend* h, const char* what, int B, int L) {
  const int rc = fe_accept(h, kDuration, what, B, L);
  return rc != US_OK ? rc : h->all_loaded(what);
}

template <bool kHead>
void dt_norm_fwd(hipStream_t s, const DtFwdArgs& a) {
  const dim3 grid((unsigned)((a.rows + 3) / 4));
  if (a.F <= 256) hipLaunchKernelGGL((dt_norm_fwd_kernel<4, kHead>), grid, dim3(256), 0, s, a);
  else hipLaunchKernelGGL((dt_norm_fwd_kernel<16, kHead>), grid, dim3(256), 0, s, a);
}
template <bool kHead>
void dt_norm_bwd(hipStream_t s, const DtBwdArgs& a) {
  if (a.F <= 256) hipLaunchKernelGGL((dt_norm_bwd_kernel<4, kHead>), dim3(kDtChunks), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((dt_norm_bwd_kernel<16, kHead>), dim3(kDtChunks), dim3(256), 0, s, a);
}

}  // namespace
}  // namespace us

extern "C" {

using namespace us;

size_t us_duration_predictor_train_workspace_bytes(us_frontend_handle h, int B, int L) {
  if (!h || h->kind != kDuration || B <= 0 || L <= 0) return 0;
  return dt_layout(h, B, L).total * sizeof(float) + 256;
}

int us_duration_predictor_forward_train(us_frontend_handle h, const float* x, const float* x_mask, const float* g, float* logw, int B, int L,
                                        float p_dropout, uint64_t seed, void* workspace, size_t workspace_bytes, us_stream stream) {
  int rc = dt_check(h, "us_duration_predictor_forward_train", B, L);
  if (rc != US_OK) return rc;
  const auto& c = h->dc;
  if (!x || !x_mask || !logw) return fe_fail(h, US_EINVAL, "us_duration_predictor_forward_train: null argument");
  if ((c.spk_emb_dim > 0) != (g != nullptr))
    return fe_fail(h, US_EINVAL, "us_duration_predictor_forward_train: g must be given exactly when the module was built with spk_emb_dim > 0");
  if (!(p_dropout < 1.f)) return fe_fail(h, US_EINVAL, "us_duration_predictor_forward_train: p_dropout must be below 1");
  if (!workspace || workspace_bytes < us_duration_predictor_train_workspace_bytes(h, B, L))
    return fe_fail(h, US_EWORKSPACE, "us_duration_predictor_forward_train: workspace too small (us_duration_predictor_train_workspace_bytes)");
  const DtLayout l = dt_layout(h, B, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* base = ws_align(workspace);
  const long long rows = (long long)B * L;
  const int F = c.filter_channels;
  const float p = p_dropout < 0.f ? 0.f : p_dropout;       // negative: the reference in eval mode (autograd still runs)
  float* mask = base + l.mask;
  hipError_t e = hipMemcpyAsync(mask, x_mask, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s);
  if (e != hipSuccess) return h->hip("us_duration_predictor_forward_train", e);
  fe_gather_concat(s, x, g, base + l.xin, B, L, c.in_channels, c.spk_emb_dim);
  gemm_conv_fwd(h, s, "conv_1", base + l.xin, base + l.r1, mask, nullptr, rows, L, true, true, false, no_drop());
  DtFwdArgs a{};
  a.r = base + l.r1; a.gamma = h->w["norm_1.gamma"].dev; a.beta = h->w["norm_1.beta"].dev; a.mask = mask; a.out = base + l.h1;
  a.rows = rows; a.F = F; a.L = L; a.drop = make_drop(seed, 0, p);
  dt_norm_fwd<false>(s, a);
  gemm_conv_fwd(h, s, "conv_2", base + l.h1, base + l.r2, mask, nullptr, rows, L, true, true, false, no_drop());
  a.r = base + l.r2; a.gamma = h->w["norm_2.gamma"].dev; a.beta = h->w["norm_2.beta"].dev; a.out = logw;      // [B][L][1] == [B][1][L]
  a.pw = h->w["proj.weight"].dev; a.pb = h->w["proj.bias"].dev; a.drop = make_drop(seed, 1, p);
  dt_norm_fwd<true>(s, a);
  if ((rc = fe_launched(h, "us_duration_predictor_forward_train")) != US_OK) return rc;
  h->tapes[workspace] = EncoderTape{B, L, p_dropout, seed};
  return US_OK;
}

int us_duration_predictor_backward(us_frontend_handle h, const float* grad_logw, int B, int L, const char* const* keys, float* const* grads,
                                   int n_grads, void* workspace, size_t workspace_bytes, us_stream stream) {
  int rc = dt_check(h, "us_duration_predictor_backward", B, L);
  if (rc != US_OK) return rc;
  EncoderTape tape;
  if ((rc = fe_tape(h, "us_duration_predictor_backward", "us_duration_predictor_forward_train", B, L, workspace, workspace_bytes,
                    us_duration_predictor_train_workspace_bytes(h, B, L), &tape)) != US_OK) return rc;
  if (!grad_logw) return fe_fail(h, US_EINVAL, "us_duration_predictor_backward: null grad_logw");
  const DtLayout l = dt_layout(h, B, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  float* base = ws_align(workspace);
  const long long rows = (long long)B * L;
  const int F = h->dc.filter_channels;
  std::map<std::string, float*> dst;
  if ((rc = fe_grad_table(h, "us_duration_predictor_backward", keys, grads, n_grads, base + l.arena, &dst)) != US_OK) return rc;
  auto G = [&](const char* k) { return dst.at(k); };
  const float p = tape.p_dropout < 0.f ? 0.f : tape.p_dropout;
  float* mask = base + l.mask;
  float* dc = base + l.dc;
  float* dh = base + l.dh;
  const int sum_blocks = (kDtSums * F + 1 + 255) / 256;
  // head: logw = proj(h2 * mask) * mask, h2 = drop(LN(r2)), r2 = relu(conv_2(h1 * mask))
  DtBwdArgs a{};
  a.r = base + l.r2; a.gamma = h->w["norm_2.gamma"].dev; a.beta = h->w["norm_2.beta"].dev; a.mask = mask; a.glogw = grad_logw;
  a.pw = h->w["proj.weight"].dev; a.dc = dc; a.part = base + l.part; a.part_b = base + l.part_b;
  a.rows = rows; a.per = (int)((rows + kDtChunks - 1) / kDtChunks); a.F = F; a.L = L; a.drop = make_drop(tape.seed, 1, p);
  dt_norm_bwd<true>(s, a);
  DtSumArgs q{};
  q.part = a.part; q.part_b = a.part_b; q.F = F;
  q.dst[0] = G("norm_2.gamma"); q.dst[1] = G("norm_2.beta"); q.dst[2] = G("conv_2.bias"); q.dst[3] = G("proj.weight"); q.dst_b = G("proj.bias");
  hipLaunchKernelGGL(dt_sum_kernel, dim3(sum_blocks), dim3(256), 0, s, q);
  gemm_conv_wgrad(h, s, "conv_2", base + l.h1, mask, true, dc, rows, L, base + l.wpart, G("conv_2.weight"));
  gemm_conv_dgrad(h, s, "conv_2", dc, dh, mask, nullptr, nullptr, 1.f, true, rows, L, base + l.wd);
  // layer 1: h1 = drop(LN(r1)), r1 = relu(conv_1(x * mask)); dh is the gradient of h1 (conv_2 read h1 * mask: masked by the data gradient)
  a.r = base + l.r1; a.gamma = h->w["norm_1.gamma"].dev; a.beta = nullptr; a.glogw = nullptr; a.pw = nullptr; a.dy = dh;
  a.drop = make_drop(tape.seed, 0, p);
  dt_norm_bwd<false>(s, a);
  q.dst[0] = G("norm_1.gamma"); q.dst[1] = G("norm_1.beta"); q.dst[2] = G("conv_1.bias"); q.dst[3] = nullptr; q.dst_b = nullptr;
  hipLaunchKernelGGL(dt_sum_kernel, dim3(sum_blocks), dim3(256), 0, s, q);
  // conv_1: weight gradient only (x is detached by the reference and g gets no gradient: the data gradient is never computed)
  gemm_conv_wgrad(h, s, "conv_1", base + l.xin, mask, true, dc, rows, L, base + l.wpart, G("conv_1.weight"));
  return fe_launched(h, "us_duration_predictor_backward");
}

int us_duration_predictor_tape_release(us_frontend_handle h, const void* workspace) {
  return fe_tape_release(h, kDuration, "us_duration_predictor_tape_release", workspace);
}

int us_duration_predictor_dropout_mask(us_frontend_handle h, uint64_t seed, int site, int B, int L, float p_dropout, float* out,
                                       us_stream stream) {
  if (!h || h->kind != kDuration || !out || B <= 0 || L <= 0) return fe_fail(h, US_EINVAL, "us_duration_predictor_dropout_mask: bad argument");
  if (site < 0 || site > 1) return fe_fail(h, US_EINVAL, "us_duration_predictor_dropout_mask: no such site");
  if (!(p_dropout < 1.f)) return fe_fail(h, US_EINVAL, "us_duration_predictor_dropout_mask: p_dropout must be below 1");
  return fe_keep_mask(h, "us_duration_predictor_dropout_mask", static_cast<hipStream_t>(stream), out, (long long)B * h->dc.filter_channels * L,
                      make_drop(seed, site, p_dropout < 0.f ? 0.f : p_dropout));
}

int us_duration_predictor_mse_loss(const float* logw, const float* w, const float* x_mask, float* loss, float* d_logw, int B, int L,
                                   us_stream stream) {
  if (!logw || !w || !x_mask || !loss || B <= 0 || L <= 0) return fe_fail(nullptr, US_EINVAL, "us_duration_predictor_mse_loss: bad argument");
  hipLaunchKernelGGL(dt_mse_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), logw, w, x_mask, loss, d_logw, B * L);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : fe_fail(nullptr, US_EHIP, std::string("us_duration_predictor_mse_loss: ") + hipGetErrorString(e));
}

}  // extern "C"
