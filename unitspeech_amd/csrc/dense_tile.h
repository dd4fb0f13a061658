// The dense-row fp32 GEMM tile on v_mfma_f32_32x32x2_f32 that the unit scorer and the CTC head share (un_score_kernel in units.hip,
// ctc_logits_kernel in ctc.hip, ctc_head_dw_kernel and ctc_head_dx_kernel in ctc_train.hip): the tile constants, the lane map the main
// loop's LDS reads and every epilogue take their indices from, and the main loop itself.
//
// A workgroup of 256 threads multiplies a 64 x 64 tile, four waves of 32 x 32: D[m][n] = sum_k A[k][m] B[k][n], both operands k-major in LDS
// in slices of 16 k, two stages.  An operand that is row-major in memory (a row per m or n, k contiguous) is transposed on the way in, to
// rows of stride 68: one store instruction of a wave writes 16 neighbouring words of each of four LDS rows 4 k apart, and 4 * 68 = 272
// words are 16 banks (mod 32), so the 64 lanes meet every bank twice, the least they can (with stride 64 the four rows would share banks).
//
// A product's terms are added in one fixed order wherever its row and column lie: MFMA s of a slice multiplies k = 2 s and 2 s + 1 and goes
// to chain s & 1, so each chain is an fp32 fma chain over ascending k (chain 0: k = 0, 1, 4, 5, ...; chain 1: k = 2, 3, 6, 7, ...), and the
// epilogue adds acc[0][r] + acc[1][r] once.  The bit-exactness promises (an item alone has the bits it has in a ragged batch) and the
// units' error bound E ("two interleaved chains of D / 2 terms and one addition") rest on that order: it is written here and nowhere else.
//
// planar_conv_mainloop (conv1d_planar.h) is the same loop with a convolution's address arithmetic for B, NSUB column sub-tiles and its
// own LDS; here the staging and the LDS arrays are the caller's, because the four kernels differ in nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include "kernels.h"

namespace us {
namespace {

constexpr int kDtTile = 64;   // rows and columns of a workgroup's tile; the packed operands are padded to it
constexpr int kDtBK = 16;     // reduction slice per LDS stage; the packed operands' k is padded to it
constexpr int kDtLdT = 68;    // row stride of a transposed slice (above)

// A thread's place in the 256-thread tile, written once.  The kernel gives each wave a 32-row half of A and a 32-column half of B (one of
// wave & 1, wave >> 1 each); the lane then feeds k row kl and element DENSE_AT(half) of an operand slice to the MFMA and holds, in register r
// of the accumulator, row DENSE_ROW(a half, r) of column DENSE_AT(b half).  Macros, as PLANAR_LANE is: the expressions reach the optimiser
// inside the kernel.  DENSE_STAGE_* is the global -> LDS staging, four floats per thread and slice: of a k-major slice (_K) row sk, columns
// [sc, sc + 4); of a row-major one (_T) row tr, k [tk, tk + 4), stored to [tk + i][tr].
#define DENSE_LANE(tid)                           \
  const int lane = (tid) & 63, wave = (tid) >> 6; \
  const int kl = lane >> 5, cl = lane & 31
#define DENSE_AT(half) ((half) * 32 + cl)
#define DENSE_ROW(half, r) ((half) * 32 + mfma32_row(r, kl))
#define DENSE_STAGE_K(tid) const int sk = (tid) >> 4, sc = ((tid) & 15) * 4
#define DENSE_STAGE_T(tid) const int tr = (tid) >> 2, tk = ((tid) & 3) * 4

struct DenseNoHook {
  template <class... A> __device__ __forceinline__ void operator()(A...) const {}
};

// The main loop: acc = 0; stage slice 0; per slice: the next slice's global loads, 8 MFMAs in turn on the two chains (no MFMA waits on the
// one before it), the next slice's LDS stores to the other stage, barrier.  load(k0) reads slice k0 into the caller's registers, store(buf)
// writes them to stage buf of As / Bs; ah and bh are the wave's halves of A and B (passed as halves, not as DENSE_AT indices: the index
// expression must meet the optimiser next to the LDS read, or ctc_logits_kernel takes two more registers).  on_mfma(fa, fb) sees every
// operand pair (the units' sum of squares); on_slice(cur) runs after a slice's MFMAs and before the next store, while stage cur is still
// whole (db's column sums).  Every thread of the workgroup calls it, with the same nk; when the stages may still be read, the caller puts
// a barrier in front.
template <int LDA, int LDB, class Load, class Store, class OnMfma = DenseNoHook, class OnSlice = DenseNoHook>
__device__ __forceinline__ void dense_tile_mainloop(const float (&As)[2][kDtBK][LDA], const float (&Bs)[2][kDtBK][LDB], int ah, int bh, int nk,
                                                    f32x16 (&acc)[2], Load&& load, Store&& store, OnMfma&& on_mfma = OnMfma{},
                                                    OnSlice&& on_slice = OnSlice{}) {
  DENSE_LANE(threadIdx.x);
  (void)wave;
#pragma unroll
  for (int n = 0; n < 2; ++n)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[n][r] = 0.f;
  load(0);
  store(0);
  __syncthreads();
  for (int kt = 0; kt < nk; ++kt) {
    const int cur = kt & 1;
    if (kt + 1 < nk) load((kt + 1) * kDtBK);
#pragma unroll
    for (int s = 0; s < kDtBK / 2; ++s) {
      const float fa = As[cur][2 * s + kl][DENSE_AT(ah)];
      const float fb = Bs[cur][2 * s + kl][DENSE_AT(bh)];
      on_mfma(fa, fb);
      acc[s & 1] = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc[s & 1], 0, 0, 0);
    }
    on_slice(cur);
    if (kt + 1 < nk) store(cur ^ 1);
    __syncthreads();
  }
}

}  // namespace
}  // namespace us
