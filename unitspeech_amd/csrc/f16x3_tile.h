// What the f16x3 GEMM kernels share: conv_igemm_kernel<.., F16>, wino_stream_kernel, wino_persist_kernel (conv_igemm.hip)
// and wgrad_f16_kernel (train.hip).  The pipelines stay in the kernels; written here and nowhere else are the product step and its close
// (the summation order every "same bits" statement cites), the two LDS operand images with their swizzles, and the turn-round patch.
// The index arithmetic is plain C++ (US_HD): tools/f16x3_layout_check.cpp walks it on the host.
#pragma once
#include "mfma_layout.h"
#if defined(__HIPCC__)
#include "kernels.h"
#endif
namespace us {
// Two-plane row: per 8 channels [8 x hi][8 x lo], so 16-byte piece 2 g + p is plane p (0 = hi, 1 = lo) of channel group g.  In 16-deep
// step s lane half hh supplies channels 16 s + 8 hh .. + 7, i.e. group 2 s + hh:
constexpr US_HD int f16x3_piece(int s, int hh, int plane) { return ((2 * s + hh) << 1) + plane; }
// Chunk image (general and persistent kernels): rows of bk channels = bk / 4 pieces, lane-linear as the LDS-DMA requires; piece c of row
// r sits in slot c ^ chunk_swz(r), so a ds_read_b128 lane group hits 16 distinct slots of the 256-byte bank window.  One involution for
// both sides: the lane feeding slot `pos` fetches piece chunk_slot(r, pos); piece c is read from slot chunk_slot(r, c).
constexpr US_HD int chunk_swz(int row, int bk = 32) { return (int)(((unsigned)row / (64u / (unsigned)bk)) % ((unsigned)bk / 4u)); }
constexpr US_HD int chunk_slot(int row, int piece, int bk = 32) { return piece ^ chunk_swz(row, bk); }
// Stream image (wino_stream_kernel): 32 rows with the whole of K each, K / 4 pieces (a multiple of 16); both sides as above.
constexpr US_HD int stream_swz(int row) { return row & 15; }
constexpr US_HD int stream_slot(int row, int piece) { return piece ^ stream_swz(row); }
// Turn-round: a 32 x 32 accumulator block (column on the lane, rows in registers) goes through a per-wave patch of 32 rows x (32 + 4
// pad) floats so that a lane ends up with 4 consecutive columns of one row: 16-byte stores, 8 rows x 128 bytes per wave instruction.
constexpr int kTurnLd = 36;                               // floats per patch row
constexpr int kTurnFloats = 32 * kTurnLd;                 // per wave
constexpr US_HD int turn_bytes(int waves) { return waves * kTurnFloats * 4; }
constexpr US_HD int turn_write_at(int r, int lane) { return mfma32_row(r, lane >> 5) * kTurnLd + (lane & 31); }      // register r, r < 16
constexpr US_HD int turn_read_row(int k, int lane) { return (lane >> 3) + 8 * k; }                                    // read-back k, k < 4
constexpr US_HD int turn_read_col(int lane) { return (lane & 7) * 4; }
#if defined(__HIPCC__)
// x ~= hi + lo * 2^-11 on both operands; a_lo b_lo ~ 2^-22 is dropped.  THE ORDER, per output element: ascending 16-deep steps; in a
// step  acc += a_hi b_hi,  then  cross += a_hi b_lo,  then  cross += a_lo b_hi  (three v_mfma_f32_32x32x16_f16, products exact in the
// fp32 accumulators); after the last step ONE  fma(cross, 2^-11, acc).  Kernels that promise each other's bits promise this.
// `hook(m)` runs after MFMA m = 0, 1, 2 of the step: where a pipeline hangs its LDS-DMA pieces under executing MFMAs.
struct F16x3NoHook { __device__ __forceinline__ void operator()(int) const {} };
template <class V, class Hook = F16x3NoHook>
__device__ __forceinline__ void f16x3_step(f32x16& acc, f32x16& cross, const V& a_hi, const V& a_lo, const V& b_hi, const V& b_lo, Hook&& hook = Hook()) {
  static_assert(sizeof(V) == 16, "one MFMA operand: eight halves");
  const half8 ah = __builtin_bit_cast(half8, a_hi), al = __builtin_bit_cast(half8, a_lo);
  const half8 bh = __builtin_bit_cast(half8, b_hi), bl = __builtin_bit_cast(half8, b_lo);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
  hook(0);
  cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, cross, 0, 0, 0);
  hook(1);
  cross = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, cross, 0, 0, 0);
  hook(2);
}
__device__ __forceinline__ float f16x3_close(float acc, float cross) { return __builtin_fmaf(cross, 0x1p-11f, acc); }
// Fragments of step s from a chunk image: fa[2 i + p] / fb[2 j + p] = plane p of the MB / NB blocks (32 rows apart) whose first rows of
// this lane are a_row / b_row, sw = chunk_swz(that row).  MB = 0: the caller makes its own A fragments (the in-kernel split).
template <int MB, int NB>
__device__ __forceinline__ void f16x3_read_frags(f32x4* fa, f32x4* fb, const float* a_row, const float* b_row, int s, int hh, int sw) {
#pragma unroll
  for (int p = 0; p < 2; ++p) {
    const int co = (f16x3_piece(s, hh, p) ^ sw) * 4;
#pragma unroll
    for (int i = 0; i < MB; ++i) fa[i * 2 + p] = *reinterpret_cast<const f32x4*>(a_row + i * 32 * 32 + co);
#pragma unroll
    for (int j = 0; j < NB; ++j) fb[j * 2 + p] = *reinterpret_cast<const f32x4*>(b_row + j * 32 * 32 + co);
  }
}
// One block through the wave's patch `tr`: val(r) is the value of accumulator register r (the caller may close the sum there);
// emit(row, col, v) gets v = columns col .. col + 3 of row `row`, four times.  16 patch writes, then 4 reads each followed by its emit:
// the counted vmcnt waits of the streaming and persistent kernels rely on "four stores per block".
template <class Val, class Emit>
__device__ __forceinline__ void turn_round(float* tr, int lane, Val&& val, Emit&& emit) {
  float* wr = tr + turn_write_at(0, lane);      // one base per lane and constant offsets: mfma32_row is linear (keeps the ds_write2 pairs)
#pragma unroll
  for (int r = 0; r < 16; ++r) wr[mfma32_row(r, 0) * kTurnLd] = val(r);
  const int row0 = turn_read_row(0, lane), col = turn_read_col(lane);
  const float* rd = tr + row0 * kTurnLd + col;
#pragma unroll
  for (int k = 0; k < 4; ++k) emit(row0 + 8 * k, col, *reinterpret_cast<const f32x4*>(rd + 8 * k * kTurnLd));
}
#endif

}  // namespace us
