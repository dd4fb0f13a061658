// Text-to-speech training step (train_STEP1.py:307-387): the alignment side that has no decoder in it.
//
//   us_mas_log_prior  the Gaussian log-prior of every (symbol, frame) pair (:336-342) followed by `maximum_path`'s value * mask:
//                     log_prior[b][x][y] = -0.5 sum_f y^2 + sum_f mu_x y - 0.5 sum_f mu_x^2 - 0.5 F log 2 pi, 0 where
//                     x_mask[b][x] y_mask[b][y] == 0.  The cross term is a GEMM over F on the fp32 matrix cores
//                     (v_mfma_f32_32x32x2_f32, exact products, fp32 accumulation); the two norms are summed alongside it from
//                     the same operand registers and added in the epilogue in the reference's order.
//   us_maximum_path   monotonic alignment search (glow-tts `maximum_path`, the external module :343 calls) on the device:
//                     attn[b][x][y] 0/1 and durations[b][x] = sum_y attn[b][x][y], bit-identical to the sequential algorithm.
//   us_duration_loss  sum((logw - log(1e-8 + d) x_mask)^2) / sum(x_lengths) (:348-349, util.duration_loss) and d loss / d logw.
//
// maximum_path, one workgroup per item, one row x per thread (Tx <= 1024: 16 waves).  The forward sweep visits the frames y in
// order; value[x][y] += max(v_prev, v_cur) with v_cur = value[x][y-1] (-1e9 when x == y) and v_prev = value[x-1][y-1] (-1e9 when
// x == 0 < y, 0 at x == y == 0), for x in [max(0, tx + y - ty), min(tx, y + 1)); cells outside that range keep their log-prior.
// Each thread keeps its row's value in a register and takes its upper neighbour's with a DPP wave shift; the first row of a wave
// takes it from the wave above through an LDS ring, read once per block.  Waves run skewed by one block of kBlk frames: in round
// r wave w sweeps block r - w, so the block of the wave above that it needs was finished one round (one barrier) earlier -- one
// barrier per kBlk frames.
// The backtrack (from tx - 1 at ty - 1: step down iff x != 0 and (x == y or value[x][y-1] < value[x-1][y-1]), strict: a tie stays
// on the row) only needs that decision per cell, so the sweep stores one bit per cell, packed 32 frames to a word, in LDS (up to
// kTableWords words: 512 x 2048 fits) or, for an item whose table does not fit, in the caller's workspace.  Wave 0 walks back one
// word column at a time: lane j holds the word of row index - j, the walk reads bits with readlane (no memory access per frame).
// Exactness: the sweep does the algorithm's fp32 additions and comparisons, in its order; nothing is contracted or reassociated.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "../../include/unitspeech_hip.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

// ---- log-prior GEMM ----------------------------------------------------------------------------------------------------
// Workgroup tile 64 (x) x 64 (y), four waves of 32 x 32.  Operands come straight from global memory (F = 80: a 32 x 32 tile reads
// 20 KB of operands for 40 MFMAs; L2 serves the repeats): A(x, f) = mu_x[b][f][x], B(f, y) = y[b][f][y], both lane-contiguous.
__global__ __launch_bounds__(256) void mas_log_prior_kernel(const float* __restrict__ mu, const float* __restrict__ yv,
                                                            const float* __restrict__ x_mask, const float* __restrict__ y_mask,
                                                            float* __restrict__ out, int F, int Tx, int Ty, float cst) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int kl = lane >> 5, cl = lane & 31;
  const int b = blockIdx.z;
  const int x = blockIdx.y * 64 + (wave & 1) * 32 + cl;
  const int y = blockIdx.x * 64 + (wave >> 1) * 32 + cl;
  const float* mb = mu + (size_t)b * F * Tx;
  const float* yb = yv + (size_t)b * F * Ty;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  float sa = 0.f, sb = 0.f;          // sum over the f of this lane's parity of mu^2 (row x) and y^2 (column y)
  for (int f0 = 0; f0 < F; f0 += 2) {
    const int f = f0 + kl;
    const float a = (f < F && x < Tx) ? mb[(size_t)f * Tx + x] : 0.f;
    const float c = (f < F && y < Ty) ? yb[(size_t)f * Ty + y] : 0.f;
    sa += a * a;
    sb += c * c;
    acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, c, acc, 0, 0, 0);
  }
  sa += __shfl_xor(sa, 32);
  sb += __shfl_xor(sb, 32);
  const float ysq = -0.5f * sb, ym = y < Ty ? y_mask[(size_t)b * Ty + y] : 0.f;
  // the MFMA column is y, the MFMA row x; the row's mu^2 sum lives in lane `row`
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int ri = mfma32_row(r, kl);
    const float msq = -0.5f * __shfl(sa, ri);
    const int xr = blockIdx.y * 64 + (wave & 1) * 32 + ri;
    if (xr >= Tx || y >= Ty) continue;                          // after the shuffle: every lane takes part in it
    const float v = ((ysq + acc[r]) + msq) + cst;                // y_square - y_mu_double + mu_square + const (:342)
    out[((size_t)b * Tx + xr) * Ty + y] = v * (x_mask[(size_t)b * Tx + xr] * ym);
  }
}

// ---- maximum_path ------------------------------------------------------------------------------------------------------
constexpr int kBlk = 16;                       // frames per round
constexpr int kMaxWaves = 16;                  // Tx <= 1024
constexpr int kRingBytes = 2 * kMaxWaves * kBlk * 4;
// The table is static and sized to all of LDS, so every launch holds a whole CU per item whatever its lengths: one item per CU,
// which is what B <= the CU count (256) wants anyway.  Batches beyond that would run in waves of 256 items; a dynamic-LDS launch
// sized to the largest table would let short items share a CU.
constexpr int kTableWords = (160 * 1024 - kRingBytes) / 4;
constexpr float kNeg = -1e9f;                  // maximum_path's max_neg_val

__global__ __launch_bounds__(1024) void maximum_path_kernel(const float* __restrict__ lp, const long long* __restrict__ x_lengths,
                                                            const long long* __restrict__ y_lengths, float* __restrict__ attn,
                                                            float* __restrict__ durations, unsigned* __restrict__ ws, int Tx, int Ty) {
  __shared__ float ring[2][kMaxWaves][kBlk];   // last row of each wave, per frame of the block it swept last
  __shared__ unsigned table_lds[kTableWords];
  const int b = blockIdx.x;
  const int x = threadIdx.x, lane = x & 63, w = x >> 6;
  const int tx = item_len(x_lengths, b, Tx), ty = item_len(y_lengths, b, Ty);
  if (tx == 0 || ty == 0) return;
  const int W = (ty + 31) >> 5;                                // words per row of the bit table
  const bool in_lds = (long long)tx * W <= kTableWords;
  unsigned* table = in_lds ? table_lds : ws + (size_t)b * Tx * ((Ty + 31) >> 5);
  const float* row = lp + ((size_t)b * Tx + min(x, tx - 1)) * Ty;
  const bool live = x < tx;
  const int nw = (tx + 63) >> 6, nblk = (ty + kBlk - 1) / kBlk;

  float v = 0.f;          // value[x][y - 1]
  float carry = 0.f;      // lane 0: value[x - 1][y - 1] for the first frame of the next block
  unsigned word = 0u;
  float cur[kBlk], nxt[kBlk];
  for (int r = 0; r < nblk + nw - 1; ++r) {
    const int cb = r - w;
    if (w < nw && cb >= 0 && cb < nblk) {
      const int y0 = cb * kBlk;
      if (cb == 0) {
#pragma unroll
        for (int k = 0; k < kBlk; ++k) cur[k] = (live && k < ty) ? row[k] : 0.f;
      }
      if (cb + 1 < nblk) {                                     // prefetch the next block while this one is swept
#pragma unroll
        for (int k = 0; k < kBlk; ++k) nxt[k] = (live && y0 + kBlk + k < ty) ? row[y0 + kBlk + k] : 0.f;
      }
      float above[kBlk];                                       // lane 0: the wave above's last row on this block's frames
#pragma unroll
      for (int k = 0; k < kBlk; ++k) above[k] = (lane == 0 && w > 0) ? ring[cb & 1][w - 1][k] : 0.f;
#pragma unroll
      for (int k = 0; k < kBlk; ++k) {
        const int y = y0 + k;
        if (y < ty) {                                          // uniform over the workgroup
          // lane i takes lane i - 1's value (DPP wave_shr:1, no LDS round trip); lane 0 takes the wave above's
          float nb = __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xF, 0xF, false));
          if (lane == 0) nb = (k == 0) ? carry : above[k - 1];
          const unsigned bit = (y >= 1 && x >= 1 && (x == y || v < nb)) ? 1u : 0u;
          float nv = cur[k];
          if (x >= max(0, tx + y - ty) && x < min(tx, y + 1)) {
            const float v_cur = (x == y) ? kNeg : v;
            const float v_prev = (x == 0) ? (y == 0 ? 0.f : kNeg) : nb;
            nv = cur[k] + fmaxf(v_prev, v_cur);
          }
          v = nv;
          word |= bit << (y & 31);
          if ((y & 31) == 31 || y == ty - 1) {
            if (live) table[(size_t)x * W + (y >> 5)] = word;
            word = 0u;
          }
          if (lane == 63) ring[cb & 1][w][k] = v;
        }
      }
      carry = above[kBlk - 1];
#pragma unroll
      for (int k = 0; k < kBlk; ++k) cur[k] = nxt[k];
    }
    __syncthreads();
  }
  if (w != 0) return;
  // backtrack: path[index][y] = 1, then index -= bit(index, y)
  float* ab = attn + (size_t)b * Tx * Ty;
  float* db = durations + (size_t)b * Tx;
  int index = tx - 1, run_end = ty - 1;
  for (int wc = W - 1; wc >= 0; --wc) {
    const int rr = index - lane;
    const unsigned wd = (rr >= 0 && lane < 32) ? table[(size_t)rr * W + wc] : 0u;
    const int i0 = index;
    int my_row = -1;
    for (int y = min(ty - 1, wc * 32 + 31); y >= wc * 32; --y) {
      if (lane == (y & 31)) my_row = index;
      const unsigned bits = (unsigned)__builtin_amdgcn_readlane((int)wd, __builtin_amdgcn_readfirstlane(i0 - index));
      if ((bits >> (y & 31)) & 1u) {
        if (lane == 0) db[index] = (float)(run_end - y + 1);
        run_end = y - 1;
        --index;
      }
    }
    if (lane < 32 && my_row >= 0) ab[(size_t)my_row * Ty + wc * 32 + lane] = 1.f;
  }
  if (lane == 0) db[index] = (float)(run_end + 1);
}

// ---- duration loss -----------------------------------------------------------------------------------------------------
// One workgroup: each thread sums a fixed strided set of elements, then a fixed tree; so the result is deterministic.
__global__ __launch_bounds__(256) void duration_loss_kernel(const float* __restrict__ logw, const float* __restrict__ dur,
                                                            const float* __restrict__ x_mask, const long long* __restrict__ x_lengths,
                                                            float* __restrict__ loss, float* __restrict__ d_logw, int B, int n) {
  __shared__ float red[256];
  __shared__ float len;
  if (threadIdx.x == 0) {
    long long s = 0;
    for (int i = 0; i < B; ++i) s += x_lengths[i];
    len = (float)s;
  }
  float s = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = logw[i] - logf(1e-8f + dur[i]) * x_mask[i];
    s += d * d;
  }
  red[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) loss[0] = red[0] / len;               // torch: sum / sum(lengths) (one fp32 division)
  if (!d_logw) return;
  for (int i = threadIdx.x; i < n; i += 256) d_logw[i] = 2.f * (logw[i] - logf(1e-8f + dur[i]) * x_mask[i]) / len;
}

size_t table_words(int Tx, int Ty) { return (size_t)Tx * ((Ty + 31) / 32); }

}  // namespace
}  // namespace us

using namespace us;

extern "C" {

int us_mas_log_prior(const float* mu_x, const float* y, const float* x_mask, const float* y_mask, float* log_prior, int B, int F, int Tx,
                     int Ty, us_stream stream) {
  if (!mu_x || !y || !x_mask || !y_mask || !log_prior || B <= 0 || F <= 0 || Tx <= 0 || Ty <= 0 || B > 65535)
    return bad_arg("us_mas_log_prior: bad argument");
  const float cst = (float)(-0.5 * std::log(2.0 * M_PI) * F);  // a Python double added to an fp32 tensor (:338)
  hipLaunchKernelGGL(mas_log_prior_kernel, dim3((Ty + 63) / 64, (Tx + 63) / 64, B), dim3(256), 0, static_cast<hipStream_t>(stream), mu_x, y,
                     x_mask, y_mask, log_prior, F, Tx, Ty, cst);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_mas_log_prior", e);
}

size_t us_maximum_path_workspace_bytes(int B, int Tx, int Ty) {
  if (B <= 0 || Tx <= 0 || Ty <= 0 || table_words(Tx, Ty) <= (size_t)kTableWords) return 0;
  return (size_t)B * table_words(Tx, Ty) * sizeof(unsigned);
}

int us_maximum_path(const float* log_prior, const int64_t* x_lengths, const int64_t* y_lengths, float* attn, float* durations, int B, int Tx,
                    int Ty, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!log_prior || !x_lengths || !y_lengths || !attn || !durations || B <= 0 || Tx <= 0 || Ty <= 0)
    return bad_arg("us_maximum_path: bad argument");
  if (Tx > 64 * kMaxWaves) return bad_arg("us_maximum_path: more than 1024 symbols per utterance");
  const size_t need = us_maximum_path_workspace_bytes(B, Tx, Ty);
  if (need && (!workspace || workspace_bytes < need)) {
    set_last_error("us_maximum_path: workspace too small (us_maximum_path_workspace_bytes)");
    return US_EWORKSPACE;
  }
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(attn, 0, (size_t)B * Tx * Ty * sizeof(float), s);
  if (e == hipSuccess) e = hipMemsetAsync(durations, 0, (size_t)B * Tx * sizeof(float), s);
  if (e != hipSuccess) return hip_fail("us_maximum_path", e);
  const int threads = 64 * ((Tx + 63) / 64);
  hipLaunchKernelGGL(maximum_path_kernel, dim3(B), dim3(threads), 0, s, log_prior, reinterpret_cast<const long long*>(x_lengths),
                     reinterpret_cast<const long long*>(y_lengths), attn, durations, static_cast<unsigned*>(workspace), Tx, Ty);
  e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_maximum_path", e);
}

int us_duration_loss(const float* logw, const float* durations, const float* x_mask, const int64_t* x_lengths, float* loss, float* d_logw,
                     int B, int Tx, us_stream stream) {
  if (!logw || !durations || !x_mask || !x_lengths || !loss || B <= 0 || Tx <= 0) return bad_arg("us_duration_loss: bad argument");
  hipLaunchKernelGGL(duration_loss_kernel, dim3(1), dim3(256), 0, static_cast<hipStream_t>(stream), logw, durations, x_mask,
                     reinterpret_cast<const long long*>(x_lengths), loss, d_logw, B, B * Tx);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_duration_loss", e);
}

}  // extern "C"
