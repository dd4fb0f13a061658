// The MOS predictor's end of the library (s3prl's `mos_wav2vec2`): the learned layer mix over an encoder's hidden states and the downstream
// head (connector, attention or mean pooling, one linear, the optional clipping), as handle-free calls that allocate nothing and only
// enqueue on the stream.
//
// Everything between the hidden states and the pooling's softmax is linear.  With s = softmax(weights), hh[t] = sum_l s_l h_l[t],
// z[t] = C hh[t] + c:
//     e[t]  = a . z[t] + a0 = v_e . hh[t] + k_e,   v_e = C^T a,  k_e = a . c + a0
//     mu[t] = m . z[t] + m0 = v_m . hh[t] + k_m,   v_m = C^T m,  k_m = m . c + m0
//     score = sum_t alpha_t mu[t],  alpha = softmax_t(e)        (sum alpha = 1; without attention pooling alpha_t = 1 / F)
// so the device never forms z: the head is two H-vectors and the hot path one stream over the hidden states.
//
//   us_mos_pack_head   the unfolded weights -> `packed`: a header (sizes, the variant flag, k_e, k_m), s[32], v_e[H], v_m[H].  The softmax over
//                      the layers and every sum over p (ascending) run in fp64 and are rounded to fp32 once.
//   us_mos_score       mos_frame_kernel, one wave per frame: lane l holds the float4 pieces l, l + 64, ... of the row (at most 4), walks the
//                      layers in ascending order with fmaf(s_l, h, acc), then forms v_e . hh and v_m . hh over its own pieces in ascending
//                      order and joins the lanes by the fixed butterfly; (v_e . hh, mu) go to the workspace.  The softmax does not change
//                      when a constant is added to every e, so k_e is left out of it: a large a0 costs no bits.
//                      mos_pool_kernel, one workgroup per item: thread i takes frames i, i + 256, ... in ascending order; the maximum, then
//                      sum exp(e - max) and sum exp(e - max) mu meet by (butterfly, waves in order); score, clipping, optional outputs.
//                      No float atomics; every order is a function of H, n_states and the item's own frames alone: an item has the same
//                      bits alone, in any batch, at any Tmax and in repeated calls.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/unitspeech_hip.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kMosMaxStates = 32, kMosMaxH = 1024, kMosMaxP = 4096;

struct MosHeader {             // 32 bytes: what follows it stays 16-byte aligned
  int n_states, H, P, attention;
  float k_e, k_m;
  int pad[2];
};
constexpr int kMosHeaderFloats = sizeof(MosHeader) / sizeof(float);
static_assert(sizeof(MosHeader) == 32, "the header is 8 words");

constexpr bool mos_dims_ok(int n_states, int H) { return n_states >= 1 && n_states <= kMosMaxStates && H >= 4 && H <= kMosMaxH && H % 4 == 0; }
constexpr bool mos_head_ok(int n_states, int H, int P) { return mos_dims_ok(n_states, H) && P >= 1 && P <= kMosMaxP; }

__device__ __forceinline__ const float* mos_s(const float* packed) { return packed + kMosHeaderFloats; }
__device__ __forceinline__ const float* mos_ve(const float* packed) { return packed + kMosHeaderFloats + kMosMaxStates; }

// Blocks 0 .. gridDim.x - 2: thread h folds column h of the connector.  The last block's first thread: the layer softmax, k_e, k_m, the header.
__global__ __launch_bounds__(256) void mos_pack_kernel(const float* __restrict__ w, const float* __restrict__ C, const float* __restrict__ c,
                                                       const float* __restrict__ a, const float* __restrict__ a0, const float* __restrict__ m,
                                                       const float* __restrict__ m0, float* __restrict__ packed, int n, int H, int P) {
  float* s = packed + kMosHeaderFloats;
  float* ve = s + kMosMaxStates;
  float* vm = ve + H;
  if (blockIdx.x == gridDim.x - 1) {
    if (threadIdx.x != 0) return;
    double mx = w[0];
    for (int l = 1; l < n; ++l) mx = fmax(mx, (double)w[l]);
    double z = 0.0;
    for (int l = 0; l < n; ++l) z += exp((double)w[l] - mx);
    for (int l = 0; l < kMosMaxStates; ++l) s[l] = l < n ? (float)(exp((double)w[l] - mx) / z) : 0.f;
    double ke = 0.0, km = 0.0;
    for (int p = 0; c && p < P; ++p) {
      if (a) ke += (double)a[p] * (double)c[p];
      km += (double)m[p] * (double)c[p];
    }
    if (a && a0) ke += (double)a0[0];
    if (m0) km += (double)m0[0];
    MosHeader hd = {n, H, P, a ? 1 : 0, (float)ke, (float)km, {0, 0}};
    *reinterpret_cast<MosHeader*>(packed) = hd;
    return;
  }
  const int h = blockIdx.x * 256 + threadIdx.x;
  if (h >= H) return;
  double se = 0.0, sm = 0.0;
  for (int p = 0; p < P; ++p) {
    const double cv = C[(size_t)p * H + h];
    if (a) se += cv * (double)a[p];
    sm += cv * (double)m[p];
  }
  ve[h] = (float)se;
  vm[h] = (float)sm;
}

__global__ __launch_bounds__(256) void mos_unpack_kernel(const float* __restrict__ packed, float* __restrict__ s, float* __restrict__ ve,
                                                         float* __restrict__ vm, float* __restrict__ k, int n, int H) {
  const MosHeader hd = *reinterpret_cast<const MosHeader*>(packed);
  const bool same = hd.n_states == n && hd.H == H;      // another head's pack: NaN, and nothing is read past it
  const float* ps = mos_s(packed);
  const float* pe = mos_ve(packed);
  const float nan = __builtin_nanf("");
  for (int i = threadIdx.x; i < H; i += 256) {
    if (ve) ve[i] = same ? pe[i] : nan;
    if (vm) vm[i] = same ? pe[H + i] : nan;
  }
  if (s && threadIdx.x < n) s[threadIdx.x] = same ? ps[threadIdx.x] : nan;
  if (k && threadIdx.x == 0) {
    k[0] = same ? hd.k_e : nan;
    k[1] = same ? hd.k_m : nan;
  }
}

__device__ __forceinline__ float dot4(const float4& x, const float4& v, float d) {
  d = fmaf(x.x, v.x, d);
  d = fmaf(x.y, v.y, d);
  d = fmaf(x.z, v.z, d);
  return fmaf(x.w, v.w, d);
}

__device__ __forceinline__ void mos_mix(float4& acc, float sl, const float4& x) {
  acc.x = fmaf(sl, x.x, acc.x);
  acc.y = fmaf(sl, x.y, acc.y);
  acc.z = fmaf(sl, x.z, acc.z);
  acc.w = fmaf(sl, x.w, acc.w);
}

// grid: (frames, items), one wave.  NP = the float4 pieces a lane holds: ceil(H / 256).  The layers are loaded four at a time, every load
// 16 bytes and independent of the others, and added in ascending order.
template <int NP>
__global__ __launch_bounds__(64) void mos_frame_kernel(const float* __restrict__ hidden, long long item_stride, long long state_stride,
                                                      const long long* __restrict__ lengths, const float* __restrict__ packed,
                                                      float2* __restrict__ em, int Tmax, int n, int H) {
  const int t = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
  if (t >= item_len(lengths, b, Tmax)) return;           // a padding row is never read: what lies there may be anything
  const MosHeader hd = *reinterpret_cast<const MosHeader*>(packed);
  float2* __restrict__ out = em + (size_t)b * Tmax + t;
  if (hd.n_states != n || hd.H != H) {                   // the pack of another head: no vector of it is read
    if (lane == 0) *out = make_float2(__builtin_nanf(""), __builtin_nanf(""));
    return;
  }
  const float* __restrict__ s = mos_s(packed);
  const int H4 = H >> 2;
  const float4* __restrict__ row = reinterpret_cast<const float4*>(hidden + (long long)b * item_stride + (long long)t * H);
  const long long ss4 = state_stride >> 2;
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  float4 acc[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) acc[j] = zero;
  bool mine[NP];
#pragma unroll
  for (int j = 0; j < NP; ++j) mine[j] = lane + 64 * j < H4;
  int l = 0;
  for (; l + 4 <= n; l += 4) {                           // whole groups of four layers: 4 NP loads in flight per lane
    float4 x[4][NP];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NP; ++j) x[i][j] = mine[j] ? row[(long long)(l + i) * ss4 + lane + 64 * j] : zero;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < NP; ++j) mos_mix(acc[j], s[l + i], x[i][j]);
  }
  for (; l < n; ++l) {                                   // the last n % 4 layers
    float4 x[NP];
#pragma unroll
    for (int j = 0; j < NP; ++j) x[j] = mine[j] ? row[(long long)l * ss4 + lane + 64 * j] : zero;
#pragma unroll
    for (int j = 0; j < NP; ++j) mos_mix(acc[j], s[l], x[j]);
  }
  const float4* __restrict__ ve = reinterpret_cast<const float4*>(mos_ve(packed));
  const float4* __restrict__ vm = ve + H4;
  float de = 0.f, dm = 0.f;
#pragma unroll
  for (int j = 0; j < NP; ++j) {
    const int p = lane + 64 * j;
    if (p < H4) {
      if (hd.attention) de = dot4(acc[j], ve[p], de);
      dm = dot4(acc[j], vm[p], dm);
    }
  }
  de = wave_sum(de);
  dm = wave_sum(dm);
  if (lane == 0) *out = make_float2(de, dm + hd.k_m);
}

// one value per thread of the 256 -> the workgroup's maximum / sum in every thread: the butterfly inside a wave, then the four waves in order
__device__ __forceinline__ float mos_block_max(float v, float* red) {
  v = wave_max(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(fmaxf(red[0], red[1]), red[2]), red[3]);
}
__device__ __forceinline__ float mos_block_sum(float v, float* red) {
  v = wave_sum(v);
  __syncthreads();
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  return ((red[0] + red[1]) + red[2]) + red[3];
}

// grid: items.  em[b][t] = (e, mu) of the item's own frames.
__global__ __launch_bounds__(256) void mos_pool_kernel(const float2* __restrict__ em, const long long* __restrict__ lengths, int Tmax, int clipping,
                                                       float* __restrict__ scores, float* __restrict__ frame_scores, float* __restrict__ attention) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int len = item_len(lengths, b, Tmax);
  const float2* __restrict__ x = em + (size_t)b * Tmax;
  float mx = -INFINITY;
  for (int t = tid; t < len; t += 256) mx = fmaxf(mx, x[t].x);
  mx = mos_block_max(mx, red);
  float se = 0.f, sn = 0.f;
  for (int t = tid; t < len; t += 256) {
    const float2 v = x[t];
    const float w = expf(v.x - mx);
    se += w;
    sn = fmaf(w, v.y, sn);
  }
  se = mos_block_sum(se, red);
  sn = mos_block_sum(sn, red);
  if (tid == 0) {
    float sc = len > 0 ? sn / se : __builtin_nanf("");   // the mean of nothing, as torch has it
    if (clipping) sc = fmaf(2.f, tanhf(sc), 3.f);
    scores[b] = sc;
  }
  if (!frame_scores && !attention) return;
  const size_t o = (size_t)b * Tmax;
  for (int t = tid; t < Tmax; t += 256) {
    const bool live = t < len;
    const float2 v = live ? x[t] : make_float2(0.f, 0.f);
    if (frame_scores) frame_scores[o + t] = live ? v.y : 0.f;
    if (attention) attention[o + t] = live ? expf(v.x - mx) / se : 0.f;
  }
}

template <int NP>
void mos_launch_frames(hipStream_t s, const float* hidden, int64_t item_stride, int64_t state_stride, const long long* lens, const float* packed,
                       float2* em, int B, int Tmax, int n, int H) {
  hipLaunchKernelGGL(mos_frame_kernel<NP>, dim3(Tmax, B), dim3(64), 0, s, hidden, (long long)item_stride, (long long)state_stride, lens, packed, em,
                     Tmax, n, H);
}

}  // namespace
}  // namespace us

using namespace us;

extern "C" {

size_t us_mos_packed_bytes(int n_states, int H, int P) {
  if (!mos_head_ok(n_states, H, P)) return 0;
  return (size_t)(kMosHeaderFloats + kMosMaxStates + 2 * H) * sizeof(float);
}

int us_mos_pack_head(const float* weights, const float* connector_weight, const float* connector_bias, const float* attention_weight,
                     const float* attention_bias, const float* mean_weight, const float* mean_bias, int n_states, int H, int P, void* packed,
                     size_t packed_bytes, us_stream stream) {
  if (!mos_head_ok(n_states, H, P)) {
    char buf[200];
    snprintf(buf, sizeof buf, "us_mos_pack_head: n_states in [1, %d], H a multiple of 4 in [4, %d] and P in [1, %d] are what is built (n_states = %d, "
             "H = %d, P = %d)", kMosMaxStates, kMosMaxH, kMosMaxP, n_states, H, P);
    return bad_arg(buf);
  }
  if (!weights || !connector_weight || !mean_weight || !packed || packed_bytes < us_mos_packed_bytes(n_states, H, P) ||
      (reinterpret_cast<uintptr_t>(packed) & 15) || (!attention_weight && attention_bias))
    return bad_arg("us_mos_pack_head: bad argument");
  hipLaunchKernelGGL(mos_pack_kernel, dim3((H + 255) / 256 + 1), dim3(256), 0, static_cast<hipStream_t>(stream), weights, connector_weight,
                     connector_bias, attention_weight, attention_bias, mean_weight, mean_bias, static_cast<float*>(packed), n_states, H, P);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_mos_pack_head", e);
}

int us_mos_unpack_head(const void* packed, int n_states, int H, float* s, float* v_e, float* v_m, float* k, us_stream stream) {
  if (!mos_dims_ok(n_states, H) || !packed || (reinterpret_cast<uintptr_t>(packed) & 15)) return bad_arg("us_mos_unpack_head: bad argument");
  hipLaunchKernelGGL(mos_unpack_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), static_cast<const float*>(packed), s, v_e, v_m, k,
                     n_states, H);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_mos_unpack_head", e);
}

size_t us_mos_workspace_bytes(int B, int Tmax) { return rows_ok(B, Tmax) ? (size_t)B * Tmax * sizeof(float2) : 0; }

int us_mos_score(const float* hidden, int64_t item_stride, int64_t state_stride, const int64_t* lengths, const void* packed, int B, int Tmax,
                 int n_states, int H, int clipping, float* scores, float* frame_scores, float* attention, void* workspace, size_t workspace_bytes,
                 us_stream stream) {
  if (!mos_dims_ok(n_states, H)) {
    char buf[160];
    snprintf(buf, sizeof buf, "us_mos_score: n_states in [1, %d] and H a multiple of 4 in [4, %d] are what is built (n_states = %d, H = %d)",
             kMosMaxStates, kMosMaxH, n_states, H);
    return bad_arg(buf);
  }
  if (!rows_ok(B, Tmax)) return bad_arg("us_mos_score: B in [1, 65535], Tmax >= 1 and B * Tmax <= 2^24 are what a call takes");
  if (!hidden || !packed || !scores || !workspace) return bad_arg("us_mos_score: bad argument");
  if ((reinterpret_cast<uintptr_t>(hidden) & 15) || (reinterpret_cast<uintptr_t>(packed) & 15) || (item_stride & 3) || (state_stride & 3) ||
      item_stride < 0 || state_stride < 0)
    return bad_arg("us_mos_score: hidden and packed must be 16-byte aligned and the strides non-negative multiples of 4 elements");
  if ((reinterpret_cast<uintptr_t>(workspace) & 7) || workspace_bytes < us_mos_workspace_bytes(B, Tmax))
    return bad_arg("us_mos_score: the workspace is misaligned or shorter than us_mos_workspace_bytes(B, Tmax)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const long long* lens = reinterpret_cast<const long long*>(lengths);
  const float* pk = static_cast<const float*>(packed);
  float2* em = static_cast<float2*>(workspace);
  switch ((H / 4 + 63) / 64) {
    case 1: mos_launch_frames<1>(s, hidden, item_stride, state_stride, lens, pk, em, B, Tmax, n_states, H); break;
    case 2: mos_launch_frames<2>(s, hidden, item_stride, state_stride, lens, pk, em, B, Tmax, n_states, H); break;
    case 3: mos_launch_frames<3>(s, hidden, item_stride, state_stride, lens, pk, em, B, Tmax, n_states, H); break;
    default: mos_launch_frames<4>(s, hidden, item_stride, state_stride, lens, pk, em, B, Tmax, n_states, H); break;
  }
  hipLaunchKernelGGL(mos_pool_kernel, dim3(B), dim3(256), 0, s, em, lens, Tmax, clipping ? 1 : 0, scores, frame_scores, attention);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_mos_score", e);
}

}  // extern "C"
