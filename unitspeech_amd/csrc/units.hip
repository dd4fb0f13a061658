// Unit extraction from the dense upstream features on (finetune.py:112-128 of the reference: k-means `predict`,
// `unique_consecutive`, util.py `process_unit`), on the device, with integer results that are exact.
//
//   us_units_pack_centers  centres [K, D] -> the GEMM operand P[Dpad][Kpad] (d-major, zero padded), h[k] = fp32(1/2 |c_k|^2 in fp64)
//                          (+inf on the padding, which therefore never wins) and C = max_k |c_k| rounded up.
//   us_units_quantize      units[b][t] = argmin_k |x - c_k|^2 = argmin_k (h[k] - x . c_k).  The products run on the fp32 matrix cores
//                          (the tile loop of dense_tile.h: fp32 fma chains); the epilogue keeps (best, second best, index) per row and the
//                          [T, K] scores never reach memory.  A row whose gap is not above twice the proven fp32 error bound E is
//                          flagged, and a second kernel takes the fp64 argmin of sum_d (x_d - c_kd)^2 over all K for the flagged rows
//                          (compacted list in workspace, length read on the device).  So every row gets the fp64 argmin with the lower
//                          index on exact ties.  A row with a non-finite feature gets -1 and counts in counters[0]; rows at or beyond
//                          lengths[b] get -1.
//   us_units_dedup         run-length encoding per item (`unique_consecutive(return_counts=True)`), padded, counts on the device.
//   us_units_process       `process_unit` in closed form: 50 Hz frame f holds samples [f spf, (f + 1) spf), output frame j takes the
//                          unit with the most samples in [j hop, (j + 1) hop) (ties: the smallest unit value), then run lengths again.
//   us_units_encode        quantize + process for a batch in one call.
//
// Error bound: with u = 2^-24, X = |x|, C = max |c_k|, the score s~ = fl(h - a~), a~ two interleaved fma chains of
// D / 2 terms and one addition, obeys |s~ - s| <= u ((D / 2 + 2) X C + C^2) (1 + 2^-12) + D 2^-150.  The kernel uses
// E = 1.0625 u ((D + 1) X C + C^2) + FLT_MIN with X from an fp32 sum of squares (relative error below 2^-13) and all of it evaluated in
// fp32 (a handful of roundings): the 1.0625 covers those.  gap > 2 E means the fp32 winner is the exact one.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>

#include "../../include/unitspeech_hip.h"
#include "dense_tile.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kMaxK = 2048, kMaxD = 1024, kMaxSpan = 64;
constexpr int kTargetGroups = 512;   // workgroups wanted before the centres stop being split across workgroups (two per CU)

// ---- pack ---------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void un_norm_kernel(const float* __restrict__ c, float* __restrict__ hn, float* __restrict__ meta, int K,
                                                       int D, int Kpad) {
  __shared__ float red[1024];
  float mx = 0.f;
  for (int k = threadIdx.x; k < Kpad; k += 1024) {
    if (k >= K) {
      hn[k] = INFINITY;
      continue;
    }
    double s = 0.0;
    for (int d = 0; d < D; ++d) {
      const double v = (double)c[(size_t)k * D + d];
      s = fma(v, v, s);
    }
    hn[k] = (float)(0.5 * s);
    const double n = sqrt(s) * (1.0 + 1e-12);          // above the true norm whatever the fp64 roundings did
    float f = (float)n;
    if ((double)f < n) f = nextafterf(f, INFINITY);
    mx = (f > mx || f != f) ? f : mx;                  // a NaN centre poisons the bound: every row is then decided in fp64
  }
  red[threadIdx.x] = mx;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) {
      const float a = red[threadIdx.x], b = red[threadIdx.x + o];
      red[threadIdx.x] = (b > a || b != b) ? b : a;
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    meta[0] = red[0];
    meta[1] = meta[2] = meta[3] = 0.f;
  }
}

__global__ __launch_bounds__(256) void un_transpose_kernel(const float* __restrict__ c, float* __restrict__ p, int K, int D, int Kpad, int Dpad) {
  const size_t n = (size_t)Dpad * Kpad;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) {
    const int k = (int)(i % Kpad), d = (int)(i / Kpad);
    p[i] = (k < K && d < D) ? c[(size_t)k * D + d] : 0.f;
  }
}

// ---- score GEMM with the running (best, second best, index) epilogue ------------------------------------------------------------
struct Best {
  float b1, b2;
  int i1;
};
// "lower score, then lower index": argmin's first-index rule, associative and commutative, so any grouping of the K slices agrees
__device__ __forceinline__ Best merge(const Best a, const Best o) {
  const bool ow = (o.b1 < a.b1) || (o.b1 == a.b1 && o.i1 < a.i1);
  Best r;
  r.b1 = ow ? o.b1 : a.b1;
  r.i1 = ow ? o.i1 : a.i1;
  r.b2 = fminf(ow ? a.b1 : o.b1, ow ? o.b2 : a.b2);
  return r;
}

// Workgroup: 64 rows x the centre tiles [split * tps, (split + 1) * tps) of 64 centres; four waves of 32 centres x 32 rows.  The centres
// are the MFMA's A operand (their index lands on the accumulator registers), the rows its B operand (on the lanes): a lane reduces its
// 16 centres in registers, one shuffle joins the two lane halves, LDS joins the two centre halves.
__global__ __launch_bounds__(256) void un_score_kernel(const float* __restrict__ X, const float* __restrict__ P, const float* __restrict__ hn,
                                                       float4* __restrict__ part, float* __restrict__ xsq, int rows, int D, int Dpad, int Kpad,
                                                       int ntiles, int tps, int nsplit) {
  __shared__ float Cs[2][kDtBK][kDtTile];
  __shared__ float Xs[2][kDtBK][kDtLdT];
  __shared__ float4 join[2][32];
  const int tid = threadIdx.x;
  DENSE_LANE(tid);
  DENSE_STAGE_K(tid);                                    // centre slice: 16 k x 64 centres, one float4 per thread
  DENSE_STAGE_T(tid);                                    // feature slice: 64 rows x 16 k, one float4 per thread
  const int ch = wave & 1, rh = wave >> 1;
  const int r0 = blockIdx.x * kDtTile, split = blockIdx.y;
  const bool xlive = r0 + tr < rows;
  const float* __restrict__ xrow = X + (size_t)(xlive ? r0 + tr : 0) * D;
  const int nk = Dpad / kDtBK;
  Best best{INFINITY, INFINITY, 0x7fffffff};
  float sx = 0.f;
  const int t_begin = split * tps, t_end = min(ntiles, t_begin + tps);
  for (int tile = t_begin; tile < t_end; ++tile) {
    const int c0 = tile * kDtTile;
    float4 creg, xreg;
    auto load = [&](int k0) {
      creg = *reinterpret_cast<const float4*>(P + (size_t)(k0 + sk) * Kpad + c0 + sc);
      xreg = (xlive && k0 + tk < D) ? *reinterpret_cast<const float4*>(xrow + k0 + tk) : make_float4(0.f, 0.f, 0.f, 0.f);
    };
    auto store = [&](int buf) {
      *reinterpret_cast<float4*>(&Cs[buf][sk][sc]) = creg;
      Xs[buf][tk + 0][tr] = xreg.x;
      Xs[buf][tk + 1][tr] = xreg.y;
      Xs[buf][tk + 2][tr] = xreg.z;
      Xs[buf][tk + 3][tr] = xreg.w;
    };
    f32x16 acc[2];
    const bool first = tile == t_begin;
    __syncthreads();                                     // the tile before this one is done with both buffers
    dense_tile_mainloop(Cs, Xs, ch, rh, nk, acc, load, store, [&](float, float fb) {
      if (first) sx = fmaf(fb, fb, sx);                  // |x|^2 of the lane's row: the first tile sees every k once
    });
    // the MFMA column is the row of X, the MFMA row the centre: a lane meets its centres in ascending order
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int c = c0 + DENSE_ROW(ch, r);
      const float s = hn[c] - (acc[0][r] + acc[1][r]);
      if (s < best.b1) {
        best.b2 = best.b1;
        best.b1 = s;
        best.i1 = c;
      } else if (s < best.b2) {
        best.b2 = s;
      }
    }
  }
  Best o;
  o.b1 = __shfl_xor(best.b1, 32);
  o.b2 = __shfl_xor(best.b2, 32);
  o.i1 = __shfl_xor(best.i1, 32);
  best = merge(best, o);
  sx += __shfl_xor(sx, 32);
  if (ch == 1 && kl == 0) join[rh][cl] = make_float4(best.b1, best.b2, __int_as_float(best.i1), 0.f);
  __syncthreads();
  if (ch == 0 && kl == 0) {
    const float4 j = join[rh][cl];
    o.b1 = j.x;
    o.b2 = j.y;
    o.i1 = __float_as_int(j.z);
    best = merge(best, o);
    const int row = r0 + DENSE_AT(rh);
    if (row < rows) {
      part[(size_t)row * nsplit + split] = make_float4(best.b1, best.b2, __int_as_float(best.i1), 0.f);
      if (split == 0) xsq[row] = sx;
    }
  }
}

// One thread per row: join the splits, decide on the fp32 result or put the row on the list of the fp64 kernel.
__global__ __launch_bounds__(256) void un_decide_kernel(const float4* __restrict__ part, const float* __restrict__ xsq,
                                                        const float* __restrict__ meta, const long long* __restrict__ lengths,
                                                        long long* __restrict__ units, int* __restrict__ list, int* __restrict__ counters,
                                                        int rows, int Tmax, int D, int nsplit) {
  const int row = blockIdx.x * 256 + threadIdx.x;
  if (row >= rows) return;
  const int b = row / Tmax, t = row - b * Tmax;
  if ((long long)t >= lengths[b]) {
    units[row] = -1;
    return;
  }
  Best best{INFINITY, INFINITY, 0x7fffffff};
  for (int s = 0; s < nsplit; ++s) {
    const float4 p = part[(size_t)row * nsplit + s];
    Best o{p.x, p.y, __float_as_int(p.z)};
    best = merge(best, o);
  }
  const float C = meta[0], Xn = sqrtf(xsq[row]);
  const float E = 1.0625f * 5.9604645e-8f * ((float)(D + 1) * Xn * C + C * C) + FLT_MIN;
  const float gap = best.b2 - best.b1;
  if (gap > 2.f * E) {                                   // false for a NaN anywhere: such a row goes to the fp64 kernel
    units[row] = best.i1;
  } else {
    units[row] = -1;
    list[atomicAdd(&counters[1], 1)] = row;
  }
}

// The flagged rows over all K in fp64: score_k = sum_d (x_d - c_kd)^2, d ascending; lower score, then lower index.
__global__ __launch_bounds__(256) void un_exact_kernel(const float* __restrict__ X, const float* __restrict__ P, const int* __restrict__ list,
                                                       int* __restrict__ counters, long long* __restrict__ units, int K, int D, int Kpad) {
  __shared__ double xs[kMaxD];
  __shared__ double rs[256];
  __shared__ int ri[256];
  const int n = counters[1];
  for (int f = blockIdx.x; f < n; f += gridDim.x) {
    const int row = list[f];
    int bad = 0;
    for (int d = threadIdx.x; d < D; d += 256) {
      const float v = X[(size_t)row * D + d];
      xs[d] = (double)v;
      bad |= !(fabsf(v) <= FLT_MAX);
    }
    if (__syncthreads_or(bad)) {
      if (threadIdx.x == 0) {
        units[row] = -1;
        atomicAdd(&counters[0], 1);
      }
      continue;
    }
    double bs = INFINITY;
    int bi = 0x7fffffff;
    for (int k = threadIdx.x; k < K; k += 256) {
      double s = 0.0;
      for (int d = 0; d < D; ++d) {
        const double v = xs[d] - (double)P[(size_t)d * Kpad + k];
        s = fma(v, v, s);
      }
      if (s < bs) {
        bs = s;
        bi = k;
      }
    }
    rs[threadIdx.x] = bs;
    ri[threadIdx.x] = bi;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if ((int)threadIdx.x < o) {
        const double s2 = rs[threadIdx.x + o];
        const int i2 = ri[threadIdx.x + o];
        if (s2 < rs[threadIdx.x] || (s2 == rs[threadIdx.x] && i2 < ri[threadIdx.x])) {
          rs[threadIdx.x] = s2;
          ri[threadIdx.x] = i2;
        }
      }
      __syncthreads();
    }
    if (threadIdx.x == 0) units[row] = ri[0] == 0x7fffffff ? -1 : ri[0];
    __syncthreads();                                     // xs, rs, ri are reused by the next row
  }
}

// ---- run-length encoding -----------------------------------------------------------------------------------------------------
// One workgroup of 256 threads: thread i owns the contiguous chunk i of u[0, len), counts the run heads in it, an LDS scan places
// them, and the run lengths are differences of neighbouring head positions (kept in `starts`, workspace).
__device__ void rle_block(const long long* __restrict__ u, int len, long long* __restrict__ out_u, long long* __restrict__ out_d,
                          float* __restrict__ out_f, long long* __restrict__ n_out, int* __restrict__ starts, int cap) {
  __shared__ int scan[256];
  const int tid = threadIdx.x;
  const int chunk = (len + 255) / 256;
  const int t0 = min(len, tid * chunk), t1 = min(len, t0 + chunk);
  int cnt = 0;
  for (int t = t0; t < t1; ++t) cnt += (t == 0 || u[t] != u[t - 1]) ? 1 : 0;
  __syncthreads();                                       // scan[] may still be read by a previous use
  block_scan256(scan, cnt);
  const int n = scan[255];
  int pos = scan[tid] - cnt;
  for (int t = t0; t < t1; ++t) {
    if (t == 0 || u[t] != u[t - 1]) {
      out_u[pos] = u[t];
      starts[pos] = t;
      ++pos;
    }
  }
  __syncthreads();
  for (int p = tid; p < cap; p += 256) {
    if (p < n) {
      const int d = ((p + 1 < n) ? starts[p + 1] : len) - starts[p];
      out_d[p] = d;
      if (out_f) out_f[p] = (float)d;
    } else {
      out_u[p] = 0;
      out_d[p] = 0;
      if (out_f) out_f[p] = 0.f;
    }
  }
  if (tid == 0) n_out[0] = n;
}

__global__ __launch_bounds__(256) void un_dedup_kernel(const long long* __restrict__ units, const long long* __restrict__ lengths,
                                                       long long* __restrict__ out_u, long long* __restrict__ out_d,
                                                       long long* __restrict__ n_out, int* __restrict__ starts, int Tmax) {
  const int b = blockIdx.x;
  const size_t o = (size_t)b * Tmax;
  rle_block(units + o, item_len(lengths, b, Tmax), out_u + o, out_d + o, nullptr, n_out + b, starts + o, Tmax);
}

// ---- process_unit ------------------------------------------------------------------------------------------------------------
// One workgroup per item.  cum[i] = 50 Hz frames up to and including run i (workspace; the runs are the units themselves when
// durations is null), frames[j] = the unit of output frame j (workspace), then rle_block.  n_out[b] = -1 when the item has more
// output frames than the outputs hold (Lout).
__global__ __launch_bounds__(256) void un_process_kernel(const long long* __restrict__ units, const long long* __restrict__ durations,
                                                         const long long* __restrict__ n_in, long long* __restrict__ out_u,
                                                         long long* __restrict__ out_d, float* __restrict__ out_f,
                                                         long long* __restrict__ n_out, long long* __restrict__ cum_ws,
                                                         long long* __restrict__ frames_ws, int* __restrict__ starts_ws, int Lin, int Lout,
                                                         long long spf, long long hop) {
  __shared__ long long scan[256];
  const int b = blockIdx.x, tid = threadIdx.x;
  const long long* __restrict__ u = units + (size_t)b * Lin;
  const long long* __restrict__ dur = durations ? durations + (size_t)b * Lin : nullptr;
  long long* __restrict__ cum = cum_ws + (size_t)b * Lin;
  long long* __restrict__ fr = frames_ws + (size_t)b * Lout;
  const int n = item_len(n_in, b, Lin);
  const int chunk = (n + 255) / 256;
  const int i0 = min(n, tid * chunk), i1 = min(n, i0 + chunk);
  long long s = 0;
  for (int i = i0; i < i1; ++i) s += dur ? max(0LL, dur[i]) : 1LL;
  block_scan256(scan, s);
  const long long total = scan[255];
  long long run = scan[tid] - s;
  for (int i = i0; i < i1; ++i) {
    run += dur ? max(0LL, dur[i]) : 1LL;
    cum[i] = run;
  }
  __syncthreads();
  const long long nf = total * spf / hop;
  if (nf > (long long)Lout) {
    for (int p = tid; p < Lout; p += 256) {
      out_u[(size_t)b * Lout + p] = 0;
      out_d[(size_t)b * Lout + p] = 0;
      if (out_f) out_f[(size_t)b * Lout + p] = 0.f;
    }
    if (tid == 0) n_out[b] = -1;
    return;
  }
  for (int j = tid; j < (int)nf; j += 256) {
    const long long a = (long long)j * hop, e = a + hop;
    int lo = 0, hi = n - 1;                              // first run whose end is beyond sample a (exists: e <= total * spf)
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cum[mid] * spf > a) hi = mid; else lo = mid + 1;
    }
    long long bu = 0, bw = -1;
    for (int p = lo; p < n; ++p) {
      const long long ps = (p ? cum[p - 1] : 0) * spf;
      if (ps >= e) break;
      if (cum[p] * spf <= ps) continue;                  // an empty run
      const long long up = u[p];
      long long w = 0;
      for (int q = lo; q < n; ++q) {
        const long long qs = (q ? cum[q - 1] : 0) * spf, qe = cum[q] * spf;
        if (qs >= e) break;
        if (u[q] == up) w += max(0LL, min(e, qe) - max(a, qs));
      }
      if (w > bw || (w == bw && up < bu)) {
        bw = w;
        bu = up;
      }
    }
    fr[j] = bu;
  }
  __syncthreads();
  rle_block(fr, (int)nf, out_u + (size_t)b * Lout, out_d + (size_t)b * Lout, out_f ? out_f + (size_t)b * Lout : nullptr, n_out + b,
            starts_ws + (size_t)b * Lout, Lout);
}

// ---- host --------------------------------------------------------------------------------------------------------------------
const char* shape_error(int K, int D) {
  if (K < 1 || K > kMaxK) return "K must be in [1, 2048]";
  if (D < 4 || D > kMaxD || D % 4) return "D must be a multiple of 4 in [4, 1024]";
  return nullptr;
}
size_t align16(size_t v) { return (v + 15) / 16 * 16; }

struct Split {
  int ntiles, tps, nsplit;
};
Split split_for(int rows, int K) {
  Split s;
  s.ntiles = round_up(K, kDtTile) / kDtTile;
  const int groups = (rows + kDtTile - 1) / kDtTile;
  int want = (kTargetGroups + groups - 1) / groups;
  want = want < 1 ? 1 : (want > s.ntiles ? s.ntiles : want);
  s.tps = (s.ntiles + want - 1) / want;
  s.nsplit = (s.ntiles + s.tps - 1) / s.tps;
  return s;
}

// workspace layout: [quantize: partials | xsq | list | units of encode] [process: cum | frames | starts]
struct Layout {
  size_t part, xsq, list, units50, cum, frames, starts, total;
};
Layout layout(int B, int Tmax, int K, int Lout) {
  Layout l;
  const size_t rows = (size_t)B * Tmax;
  size_t o = 0;
  l.part = o;
  o += K > 0 ? align16(rows * split_for((int)rows, K).nsplit * sizeof(float4)) : 0;
  l.xsq = o;
  o += K > 0 ? align16(rows * sizeof(float)) : 0;
  l.list = o;
  o += K > 0 ? align16(rows * sizeof(int)) : 0;
  l.units50 = o;
  o += K > 0 && Lout > 0 ? align16(rows * sizeof(long long)) : 0;
  l.cum = o;
  o += Lout > 0 ? align16(rows * sizeof(long long)) : 0;
  l.frames = o;
  o += Lout > 0 ? align16((size_t)B * Lout * sizeof(long long)) : 0;
  l.starts = o;
  o += align16((size_t)B * (Tmax > Lout ? Tmax : Lout) * sizeof(int));
  l.total = o;
  return l;
}

}  // namespace
}  // namespace us

using namespace us;

extern "C" {

size_t us_units_packed_bytes(int K, int D) {
  if (shape_error(K, D)) return 0;
  return ((size_t)round_up(D, kDtBK) * round_up(K, kDtTile) + round_up(K, kDtTile) + 4) * sizeof(float);
}

int us_units_pack_centers(const float* centers, int K, int D, void* packed, size_t packed_bytes, us_stream stream) {
  if (const char* m = shape_error(K, D)) {
    char buf[128];
    snprintf(buf, sizeof buf, "us_units_pack_centers: %s (K = %d, D = %d)", m, K, D);
    return bad_arg(buf);
  }
  if (!centers || !packed || packed_bytes < us_units_packed_bytes(K, D)) return bad_arg("us_units_pack_centers: bad argument");
  const int Kpad = round_up(K, kDtTile), Dpad = round_up(D, kDtBK);
  float* P = static_cast<float*>(packed);
  float* hn = P + (size_t)Dpad * Kpad;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(un_norm_kernel, dim3(1), dim3(1024), 0, s, centers, hn, hn + Kpad, K, D, Kpad);
  hipLaunchKernelGGL(un_transpose_kernel, dim3(512), dim3(256), 0, s, centers, P, K, D, Kpad, Dpad);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_units_pack_centers", e);
}

size_t us_units_workspace_bytes(int B, int Tmax, int K, int D, int Lout) {
  if (!rows_ok(B, Tmax) || Lout < 0 || K < 0 || (K > 0 && shape_error(K, D)) || (Lout > 0 && !rows_ok(B, Lout))) return 0;
  return layout(B, Tmax, K, Lout).total;
}

int us_units_quantize(const float* dense, const int64_t* lengths, const void* packed, int B, int Tmax, int K, int D, int64_t* units,
                      int32_t* counters, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (const char* m = shape_error(K, D)) {
    char buf[128];
    snprintf(buf, sizeof buf, "us_units_quantize: %s (K = %d, D = %d)", m, K, D);
    return bad_arg(buf);
  }
  if (!dense || !lengths || !packed || !units || !counters || !rows_ok(B, Tmax)) return bad_arg("us_units_quantize: bad argument");
  const Layout l = layout(B, Tmax, K, 0);
  if (!workspace || workspace_bytes < l.total) {
    set_last_error("us_units_quantize: workspace too small (us_units_workspace_bytes)");
    return US_EWORKSPACE;
  }
  const int rows = B * Tmax, Kpad = round_up(K, kDtTile), Dpad = round_up(D, kDtBK);
  const Split sp = split_for(rows, K);
  const float* P = static_cast<const float*>(packed);
  const float* hn = P + (size_t)Dpad * Kpad;
  char* ws = static_cast<char*>(workspace);
  float4* part = reinterpret_cast<float4*>(ws + l.part);
  float* xsq = reinterpret_cast<float*>(ws + l.xsq);
  int* list = reinterpret_cast<int*>(ws + l.list);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipError_t e = hipMemsetAsync(counters, 0, 2 * sizeof(int32_t), s);
  if (e != hipSuccess) return hip_fail("us_units_quantize", e);
  hipLaunchKernelGGL(un_score_kernel, dim3((rows + kDtTile - 1) / kDtTile, sp.nsplit), dim3(256), 0, s, dense, P, hn, part, xsq, rows, D, Dpad, Kpad,
                     sp.ntiles, sp.tps, sp.nsplit);
  hipLaunchKernelGGL(un_decide_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, part, xsq, hn + Kpad,
                     reinterpret_cast<const long long*>(lengths), reinterpret_cast<long long*>(units), list, counters, rows, Tmax, D, sp.nsplit);
  hipLaunchKernelGGL(un_exact_kernel, dim3(rows < 2048 ? rows : 2048), dim3(256), 0, s, dense, P, list, counters,
                     reinterpret_cast<long long*>(units), K, D, Kpad);
  e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_units_quantize", e);
}

int us_units_dedup(const int64_t* units, const int64_t* lengths, int B, int Tmax, int64_t* out_units, int64_t* out_durations, int64_t* n,
                   void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!units || !lengths || !out_units || !out_durations || !n || !rows_ok(B, Tmax) || units == out_units)
    return bad_arg("us_units_dedup: bad argument");
  const Layout l = layout(B, Tmax, 0, 0);
  if (!workspace || workspace_bytes < l.total) {
    set_last_error("us_units_dedup: workspace too small (us_units_workspace_bytes)");
    return US_EWORKSPACE;
  }
  hipLaunchKernelGGL(un_dedup_kernel, dim3(B), dim3(256), 0, static_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(units),
                     reinterpret_cast<const long long*>(lengths), reinterpret_cast<long long*>(out_units),
                     reinterpret_cast<long long*>(out_durations), reinterpret_cast<long long*>(n),
                     reinterpret_cast<int*>(static_cast<char*>(workspace) + l.starts), Tmax);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_units_dedup", e);
}

static int process_at(const int64_t* units, const int64_t* durations, const int64_t* n_in, int B, int Lin, int sampling_rate, int hop_length,
                      int64_t* out_units, int64_t* out_durations, float* duration_f, int64_t* n_out, int Lout, char* ws, const Layout& l,
                      hipStream_t s) {
  hipLaunchKernelGGL(un_process_kernel, dim3(B), dim3(256), 0, s, reinterpret_cast<const long long*>(units),
                     reinterpret_cast<const long long*>(durations), reinterpret_cast<const long long*>(n_in),
                     reinterpret_cast<long long*>(out_units), reinterpret_cast<long long*>(out_durations), duration_f,
                     reinterpret_cast<long long*>(n_out), reinterpret_cast<long long*>(ws + l.cum), reinterpret_cast<long long*>(ws + l.frames),
                     reinterpret_cast<int*>(ws + l.starts), Lin, Lout, (long long)(sampling_rate / 50), (long long)hop_length);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_units_process", e);
}

static const char* rate_error(int sampling_rate, int hop_length) {
  if (sampling_rate < 50 || hop_length < 1) return "sampling_rate must be at least 50 and hop_length at least 1";
  const int spf = sampling_rate / 50;
  if ((hop_length + spf - 2) / spf + 1 > kMaxSpan) return "an output frame would span more than 64 frames of the 50 Hz stream";
  return nullptr;
}

int us_units_process(const int64_t* units, const int64_t* durations, const int64_t* n_in, int B, int Lin, int sampling_rate, int hop_length,
                     int64_t* out_units, int64_t* out_durations, float* duration_f, int64_t* n_out, int Lout, void* workspace,
                     size_t workspace_bytes, us_stream stream) {
  if (const char* m = rate_error(sampling_rate, hop_length)) {
    char buf[160];
    snprintf(buf, sizeof buf, "us_units_process: %s (sampling_rate = %d, hop_length = %d)", m, sampling_rate, hop_length);
    return bad_arg(buf);
  }
  if (!units || !n_in || !out_units || !out_durations || !n_out || !rows_ok(B, Lin) || !rows_ok(B, Lout))
    return bad_arg("us_units_process: bad argument");
  const Layout l = layout(B, Lin, 0, Lout);
  if (!workspace || workspace_bytes < l.total) {
    set_last_error("us_units_process: workspace too small (us_units_workspace_bytes)");
    return US_EWORKSPACE;
  }
  return process_at(units, durations, n_in, B, Lin, sampling_rate, hop_length, out_units, out_durations, duration_f, n_out, Lout,
                    static_cast<char*>(workspace), l, static_cast<hipStream_t>(stream));
}

int us_units_encode(const float* dense, const int64_t* lengths, const void* packed, int B, int Tmax, int K, int D, int sampling_rate,
                    int hop_length, int64_t* out_units, int64_t* out_durations, float* duration_f, int64_t* n_out, int Lout,
                    int32_t* counters, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (const char* m = rate_error(sampling_rate, hop_length)) {
    char buf[160];
    snprintf(buf, sizeof buf, "us_units_encode: %s (sampling_rate = %d, hop_length = %d)", m, sampling_rate, hop_length);
    return bad_arg(buf);
  }
  if (shape_error(K, D) || !rows_ok(B, Tmax) || !rows_ok(B, Lout) || !out_units || !out_durations || !n_out)
    return bad_arg("us_units_encode: bad argument");
  const Layout l = layout(B, Tmax, K, Lout);
  if (!workspace || workspace_bytes < l.total) {
    set_last_error("us_units_encode: workspace too small (us_units_workspace_bytes)");
    return US_EWORKSPACE;
  }
  char* ws = static_cast<char*>(workspace);
  int64_t* units50 = reinterpret_cast<int64_t*>(ws + l.units50);
  // the quantize sections of the two layouts coincide (they come first and depend on B, Tmax, K only)
  const int rc = us_units_quantize(dense, lengths, packed, B, Tmax, K, D, units50, counters, workspace, workspace_bytes, stream);
  if (rc != US_OK) return rc;
  return process_at(units50, nullptr, lengths, B, Tmax, sampling_rate, hop_length, out_units, out_durations, duration_f, n_out, Lout, ws, l,
                    static_cast<hipStream_t>(stream));
}

}  // extern "C"
