// The planar Conv1d implicit GEMM on v_mfma_f32_32x32x2_f32 that the vocoder, the speaker encoder, HuBERT / WavLM, the mel front end and the
// resampler share (vc_conv_kernel, sp_conv_kernel, hb_gemm_kernel, mel_dft_kernel, mel_proj_kernel, rs_gemm_kernel): the main loop, the lane
// map (PLANAR_*) its epilogues read, the fold in front of the last three, the weight pack and the host-side description of a layer.
//
// Activations are planar [B][C][T] (time contiguous).  Output step q of one batch item and one phase:
//   D[co][q] = sum_{j < taps, ci < Cin} P[j * Cin + ci][co] * in[ci][q + off + j * dil],   in[] = 0 outside [0, T),
// with the output channel as the MFMA row and time as the column.  P is packed once per layer with its taps * Cin rows padded to a
// multiple of kPcBK and its columns to a multiple of kPcBM (zeros), so the weight tile needs no bounds checks:
//  Conv1d(k, dilation d, padding d (k - 1) / 2) reading the first Cin of CinTot input channels:  one phase, taps k, dil d, off
//    -d (k - 1) / 2, P[j * Cin + ci][co] = W[co][ci][j].
//  ConvTranspose1d(Cin, Cout, k, stride u, padding p = (k - u) / 2), k = K * u:  y[co][t] = bias[co] + sum_{ci, j} W[ci][co][j] *
//    x[ci][i] over the (i, j) with i * u - p + j = t.  Write t = q * u + r and (r + p) = a_r * u + b_r (0 <= b_r < u): then j must
//    be n * u + b_r (n in [0, K)) and i = q + a_r - n.  So phase r is an ordinary convolution with K taps, dil 1, off[r] = a_r -
//    (K - 1) (tap n' = K - 1 - n reads x[q + off[r] + n']) and P_r[n' * Cin + ci][co] = W[ci][co][(K - 1 - n') * u + b_r]: every one
//    of its K taps is a real product (none of the zeros of the stride-u dilated input is ever computed), and the u phases
//    together write each output sample exactly once (t = q * u + r covers [0, Tin * u)).
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>

#include "handle.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kPcBM = 64;     // output channels per workgroup
constexpr int kPcBK = 16;     // reduction slice per LDS stage
constexpr int kPcMaxPhases = 16;

struct PlanarConvTile {       // what one workgroup of 256 threads multiplies
  const float* in;            // [Cin][T] of this batch item
  const float* w;             // [Kpad][ldw] of this phase
  int Cin, T, dil, off;
  int Kdim, Kpad, ldw;        // Kdim = taps * Cin live rows of w
  int m0, n0;                 // first output channel and first output step
  int n = 0;                  // valid steps of every row (rows stay T apart): read by the VALID main loop only, in[] = 0 outside [0, n)
};

// A thread's place in the 256-thread tile, written once: wave (mh, nh) = (wave & 1, wave >> 1) owns channels [32 mh, +32) and the NSUB 32-step
// sub-tiles from step 32 NSUB nh on; inside a sub-tile the lane feeds K row kl and column cl of an MFMA and holds, in register r of the
// accumulator, row mfma32_row(r, kl) of column cl.  The main loop's LDS reads and every epilogue take the channel and the step from these, so
// the two agree.  They are macros, not functions: the expressions then reach the optimiser inside the kernel, as the lines they replace did
// (inline functions are optimised on their own first, and every epilogue then compiled to other instructions).  PLANAR_STEP(NSUB, n0, n) and
// n0 + PLANAR_COL(NSUB, n) are the same number; the first keeps the wave's and the sub-tile's offsets apart, as the vocoder wrote it.
#define PLANAR_LANE(tid)                          \
  const int lane = (tid) & 63, wave = (tid) >> 6; \
  const int mh = wave & 1, nh = wave >> 1, kl = lane >> 5, cl = lane & 31
#define PLANAR_ROW(r) (mh * 32 + mfma32_row(r, kl))                   /* within the tile: the channel of accumulator register r */
#define PLANAR_COL(NSUB, n) ((nh * (NSUB) + (n)) * 32 + cl)           /* within the tile: the step of sub-tile n */
#define PLANAR_CHANNEL(m0, r) ((m0) + mh * 32 + mfma32_row(r, kl))    /* in the tensor, for a tile that starts at channel m0 ... */
#define PLANAR_STEP(NSUB, n0, n) ((n0) + nh * ((NSUB) * 32) + (n) * 32 + cl) /* ... and step n0 */

// The main loop.  The workgroup's tile is kPcBM channels x 64 NSUB steps, shared out among the waves as PLANAR_LANE says.  Sub-tile n
// accumulates into acc[n][0 .. NCHAIN): MFMA s of a K slice goes to chain s % NCHAIN, so with two chains no MFMA waits on the one before it,
// and the caller adds the chains up.
// K slices of kPcBK are double-buffered in LDS: the next slice's global loads are in flight while this one is multiplied.
// STRIDE > 1 is the strided convolution D[co][q] = sum P[j * Cin + ci][co] * in[ci][STRIDE * q + off + j * dil] (the HuBERT extractor); the
// default multiplies by a compile-time 1, so every other instantiation's code is what it was.
// VALID bounds the input loads by the tile's valid length g.n instead of its row stride g.T (a ragged batch item: n steps stored T apart, so
// nothing at or past an item's end is ever read and no producer has to write zeros there); the default never looks at g.n.
template <int NSUB, int NCHAIN, int STRIDE = 1, bool VALID = false>
__device__ __forceinline__ void planar_conv_mainloop(const PlanarConvTile& g, f32x16 (&acc)[NSUB][NCHAIN]) {
  constexpr int BN = 64 * NSUB, NX = BN / 16;
  __shared__ float As[2][kPcBK][kPcBM];
  __shared__ float Bs[2][kPcBK][BN];
  const int tid = threadIdx.x;
  PLANAR_LANE(tid);
  const float* __restrict__ in = g.in;
  const float* __restrict__ w = g.w;
  // global -> register staging: weights 4 floats per thread (one float4 of row tid / 16), input NX floats of row tid / 16
  const int wr = tid >> 4, wc = (tid & 15) * 4;
  const int xr = tid >> 4, xc = tid & 15;
  float4 wreg;
  float xreg[NX];
  auto load = [&](int k0) {
    wreg = *reinterpret_cast<const float4*>(w + (size_t)(k0 + wr) * g.ldw + g.m0 + wc);
    const int kk = k0 + xr;
    const bool live = kk < g.Kdim;
    const int j = live ? kk / g.Cin : 0, ci = live ? kk - j * g.Cin : 0;
    const float* row = in + (size_t)ci * g.T;
    const int t0 = g.n0 * STRIDE + g.off + j * g.dil;
    const int end = VALID ? g.n : g.T;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const int t = t0 + (xc + 16 * i) * STRIDE;
      xreg[i] = (live && t >= 0 && t < end) ? row[t] : 0.f;
    }
  };
  auto store = [&](int buf) {
    *reinterpret_cast<float4*>(&As[buf][wr][wc]) = wreg;
#pragma unroll
    for (int i = 0; i < NX; ++i) Bs[buf][xr][xc + 16 * i] = xreg[i];
  };
#pragma unroll
  for (int n = 0; n < NSUB; ++n)
#pragma unroll
    for (int c = 0; c < NCHAIN; ++c)
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[n][c][r] = 0.f;
  const int nk = g.Kpad / kPcBK;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * kPcBK);
#pragma unroll
    for (int s = 0; s < kPcBK / 2; ++s) {
      const float fa = As[cur][2 * s + kl][mh * 32 + cl];
#pragma unroll
      for (int n = 0; n < NSUB; ++n) {
        const float fb = Bs[cur][2 * s + kl][PLANAR_COL(NSUB, n)];
        acc[n][s % NCHAIN] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[n][s % NCHAIN], 0, 0, 0);
      }
    }
    if (kt + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }
}

// The fold in front of a convolution whose input is a strided view of a waveform (mel.hip, resample.hip): rows wav[b][Tmax] of lens.n[b] valid
// samples -> x[b][ci][q] = src(w, len, q, ci) for ci < C, q < Q, where w and len are item b's row and length and src gives 0.f where the
// element is padding or (q, ci) lies outside the tensor.  One workgroup of 256 threads per 64 ci x 64 q of one item (blockIdx: q tile, ci tile,
// item).  w is read along ci and x written along q: transposed through LDS so that both are coalesced.
template <class Lens, class Src>
__device__ __forceinline__ void planar_fold_tile(const float* __restrict__ wav, float* __restrict__ x, const Lens& lens, int Tmax, int C, int Q,
                                                 Src&& src) {
  __shared__ float tile[64][65];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int q0 = blockIdx.x * 64, c0 = blockIdx.y * 64, b = blockIdx.z;
  const long long len = lens.n[b];
  const float* __restrict__ w = wav + (size_t)b * Tmax;
  for (int r = wave; r < 64; r += 4) tile[r][lane] = src(w, len, q0 + r, c0 + lane);
  __syncthreads();
  float* __restrict__ xb = x + (size_t)b * C * Q;
  for (int r = wave; r < 64; r += 4) {
    const int ci = c0 + r, q = q0 + lane;
    if (ci < C && q < Q) xb[(size_t)ci * Q + q] = tile[lane][r];
  }
}

// P[ph][kk][co] (zero padded), kk = j * Cin + ci, from a Conv1d weight W[Cout][CinTot][k] of which the first Cin input channels are
// taken (u == 0), or from a ConvTranspose1d weight W[Cin][Cout][k] (u > 0, k = taps * u, padding pad): the packing described on top
__global__ void planar_conv_pack_kernel(const float* __restrict__ w, float* __restrict__ p, int Cin, int CinTot, int Cout, int k, int u,
                                        int pad, int taps, int Kpad, int ldw, int nph) {
  const size_t n = (size_t)nph * Kpad * ldw;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % ldw);
    const int kk = (int)((i / ldw) % Kpad);
    const int ph = (int)(i / ((size_t)ldw * Kpad));
    float v = 0.f;
    if (co < Cout && kk < taps * Cin) {
      const int j = kk / Cin, ci = kk - j * Cin;
      if (u == 0) {
        v = w[((size_t)co * CinTot + ci) * k + j];
      } else {
        const int br = (ph + pad) % u;
        v = w[((size_t)ci * Cout + co) * k + (taps - 1 - j) * u + br];
      }
    }
    p[i] = v;
  }
}

struct PlanarConv {             // one Conv1d / ConvTranspose1d in packed form
  int cin = 0, cin_tot = 0, cout = 0, k = 0, dil = 1, u = 0, pad = 0;     // u > 0: transposed with stride u
  int taps = 0, Kpad = 0, ldw = 0, nph = 1;
  int off[kPcMaxPhases] = {};
  float* packed = nullptr;      // [nph][Kpad][ldw]

  void conv(int cin_, int cin_tot_, int cout_, int k_, int dil_) {
    cin = cin_; cin_tot = cin_tot_; cout = cout_; k = k_; dil = dil_; taps = k_;
    pads();
    off[0] = -dil * (k - 1) / 2;
  }
  void transposed(int cin_, int cout_, int k_, int u_) {
    cin = cin_tot = cin_; cout = cout_; k = k_; u = u_; pad = (k_ - u_) / 2; taps = k_ / u_; nph = u_;
    pads();
    for (int r = 0; r < u; ++r) off[r] = (r + pad) / u - (taps - 1);
  }
  void pads() { Kpad = round_up(taps * cin, kPcBK); ldw = round_up(cout, kPcBM); }
  int Kdim() const { return taps * cin; }
  size_t packed_floats() const { return (size_t)nph * Kpad * ldw; }
  void pack(const float* w, hipStream_t s) const {      // w: the layer's weight in the reference layout; `packed` is allocated
    hipLaunchKernelGGL(planar_conv_pack_kernel, dim3((unsigned)std::min<size_t>((packed_floats() + 255) / 256, 4096)), dim3(256), 0, s, w,
                       packed, cin, cin_tot, cout, k, u, pad, taps, Kpad, ldw, nph);
  }
  void release() {
    if (packed) (void)hipFree(packed);
    packed = nullptr;
  }
};

}  // namespace
}  // namespace us
