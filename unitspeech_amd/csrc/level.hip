// ITU-T P.56 method B active speech level (the "speech voltmeter" behind sv56) and the gain normalisation that goes with it, on ragged
// batches, as handle-free calls that allocate nothing and only enqueue on the stream.  Everything that decides a count runs in fp64.
//
//   envelope      p[k] = g p[k-1] + (1-g) |x[k]|, q[k] = g q[k-1] + (1-g) p[k].  n samples act on the state (p, q) as the affine map
//                 (G p + P, G q + n (1-g) G p + Q) with G = g^n; (n1, G1, P1, Q1) followed by (n2, G2, P2, Q2) is
//                 (n1 + n2, G1 G2, G2 P1 + P2, G2 Q1 + n2 (1-g) G2 P1 + Q2): associative, so it scans.
//   chunks        an item is cut into chunks of kChunk samples from its own start; a thread owns kRun consecutive samples of a chunk.  What
//                 a chunk computes depends on the item's samples and length alone, so an item has the same bits alone, in any batch and from
//                 run to run.  No workgroup waits for another: the passes are separate launches joined in a fixed order.
//   measure       1 level_summary_kernel   (item, chunk): the chunk's map and its sum x^2, sum x, max, min, non-finite flag
//                 2 level_carry_kernel     one thread per item walks the chunk maps in order: every chunk's carry-in (p, q), the item's totals
//                 3 level_tuple_kernel     (item, chunk): q from the carry-in; per threshold the first and last index at or above it and the
//                                          count the chunk has when no hangover enters it
//                 4 level_final_kernel     one wave per item: lane j composes threshold j's tuples in order (the entering hangover adds
//                                          min(first or chunk length, max(0, I - d_in)) samples); lane 0 evaluates the level in fp64
//   apply         5 level_apply_kernel     (item, chunk): 8 samples per thread and step with 16-byte loads and stores, out = x * factor as
//                                          fp32 or as int16 rounded half away from zero and saturated; the chunk's clipped count
//                 6 level_gain_kernel      one wave per item: gain, and the clipped counts added up (integers)
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>

#include "../../include/unitspeech_hip.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kChunk = 4096;              // samples per chunk
constexpr int kThreads = 256;
constexpr int kRun = kChunk / kThreads;   // consecutive samples per thread in the measuring passes
constexpr int kThr = 15;                  // thresholds 2^-15 .. 2^-1
constexpr int kUnit = 8;                  // samples per 16-byte int16 vector: the apply kernel's step
constexpr double kMargin = 15.9, kSilent = -100.0;
static_assert(kRun == 16, "the loaders below read 16 samples per thread");

struct Map {                              // the action of n samples on (p, q)
  int n;
  double G, P, Q;
};
__device__ __forceinline__ Map map_identity() { return Map{0, 1.0, 0.0, 0.0}; }
__device__ __forceinline__ Map map_then(const Map& a, const Map& b, double h) {      // a first, then b; h = 1 - g
  Map r;
  r.n = a.n + b.n;
  r.G = a.G * b.G;
  r.P = b.G * a.P + b.P;
  r.Q = b.G * a.Q + ((double)b.n * h) * (b.G * a.P) + b.Q;
  return r;
}
__device__ __forceinline__ void map_apply(const Map& m, double& p, double& q, double h) {
  const double p0 = p;
  p = m.G * p0 + m.P;
  q = m.G * q + ((double)m.n * h) * (m.G * p0) + m.Q;
}
__device__ __forceinline__ Map map_shfl_up(const Map& m, int o) {
  Map r;
  r.n = __shfl_up(m.n, o);
  r.G = __shfl_up(m.G, o);
  r.P = __shfl_up(m.P, o);
  r.Q = __shfl_up(m.Q, o);
  return r;
}

// The workgroup's exclusive scan of the threads' maps in thread order: -> what precedes this thread in the chunk; total = the whole chunk.
__device__ __forceinline__ Map block_scan(const Map& mine, double h, Map* wave_tot, Map& total) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  Map inc = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const Map up = map_shfl_up(inc, o);
    if (lane >= o) inc = map_then(up, inc, h);
  }
  Map exc = map_shfl_up(inc, 1);
  if (lane == 0) exc = map_identity();
  if (lane == 63) wave_tot[wave] = inc;
  __syncthreads();
  Map pre = map_identity();
  total = map_identity();
#pragma unroll
  for (int w = 0; w < kThreads / 64; ++w) {
    if (w == wave) pre = total;
    total = map_then(total, wave_tot[w], h);
  }
  return map_then(pre, exc, h);
}

// The reference's float -> int16 route: an fp32 product truncated toward zero, held to the int16 range.
__device__ __forceinline__ int quantize_ref(float v) { return (int)fminf(fmaxf(v * 32767.0f, -32768.0f), 32767.0f); }

// One sample in units of full scale; a non-finite float sets `bad` and counts as 0 in the measurement.
__device__ __forceinline__ double sample_value(float v, bool quant, bool& bad) {
  if (!isfinite(v)) {
    bad = true;
    return 0.0;
  }
  return quant ? (double)quantize_ref(v) * (1.0 / 32768.0) : (double)v;
}
__device__ __forceinline__ double sample_value(short v, bool, bool&) { return (double)v * (1.0 / 32768.0); }

// The thread's run of kRun samples from row + s (nv of them live): 16-byte loads when the row allows it and the run is whole.
__device__ __forceinline__ void load_run(const float* __restrict__ row, long long s, int nv, bool vec, bool quant, double (&x)[kRun], bool& bad) {
  if (vec && nv == kRun) {
#pragma unroll
    for (int v = 0; v < kRun / 4; ++v) {
      const float4 f = *reinterpret_cast<const float4*>(row + s + 4 * v);
      x[4 * v + 0] = sample_value(f.x, quant, bad);
      x[4 * v + 1] = sample_value(f.y, quant, bad);
      x[4 * v + 2] = sample_value(f.z, quant, bad);
      x[4 * v + 3] = sample_value(f.w, quant, bad);
    }
  } else {
#pragma unroll
    for (int i = 0; i < kRun; ++i) x[i] = i < nv ? sample_value(row[s + i], quant, bad) : 0.0;
  }
}
__device__ __forceinline__ void load_run(const short* __restrict__ row, long long s, int nv, bool vec, bool quant, double (&x)[kRun], bool& bad) {
  if (vec && nv == kRun) {
#pragma unroll
    for (int v = 0; v < kRun / 8; ++v) {
      const int4 w = *reinterpret_cast<const int4*>(row + s + 8 * v);
      const int d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        x[8 * v + 2 * e + 0] = sample_value((short)(d[e] & 0xffff), quant, bad);
        x[8 * v + 2 * e + 1] = sample_value((short)(d[e] >> 16), quant, bad);
      }
    }
  } else {
#pragma unroll
    for (int i = 0; i < kRun; ++i) x[i] = i < nv ? sample_value(row[s + i], quant, bad) : 0.0;
  }
}

// The map of the thread's run (from the zero state: P and Q are then the state itself).
__device__ __forceinline__ Map run_map(const double (&x)[kRun], int nv, double g, double h) {
  Map m = map_identity();
#pragma unroll
  for (int i = 0; i < kRun; ++i)
    if (i < nv) {
      m.G *= g;
      m.P = g * m.P + h * fabs(x[i]);
      m.Q = g * m.Q + h * m.P;
    }
  m.n = nv;
  return m;
}

// Workspace, in this order: sums [B][nch][8] fp64, carry [B][nch][2] fp64, totals [B][8] fp64, tuples [B][nch][15][4] int32,
// clipped [B][nch] int32.  sums: P, Q, sum x^2, sum x, max, min, non-finite, samples.
struct Work {
  double* sums;
  double* carry;
  double* totals;
  int* tuples;
  int* clipped;
};
inline int chunks_of(int T) { return (T + kChunk - 1) / kChunk; }
inline size_t work_bytes(int B, int Tmax) {
  const size_t n = (size_t)B * chunks_of(Tmax);
  return n * 8 * sizeof(double) + n * 2 * sizeof(double) + (size_t)B * 8 * sizeof(double) + n * kThr * 4 * sizeof(int) + n * sizeof(int);
}
inline Work carve(void* ws, int B, int Tmax) {
  const size_t n = (size_t)B * chunks_of(Tmax);
  Work w;
  w.sums = static_cast<double*>(ws);
  w.carry = w.sums + n * 8;
  w.totals = w.carry + n * 2;
  w.tuples = reinterpret_cast<int*>(w.totals + (size_t)B * 8);
  w.clipped = w.tuples + n * kThr * 4;
  return w;
}

template <typename T>
__global__ __launch_bounds__(kThreads) void level_summary_kernel(const T* __restrict__ wav, const long long* __restrict__ lengths, int Tmax,
                                                                 int vec, int quant, double g, double* __restrict__ sums) {
  __shared__ Map wave_tot[kThreads / 64];
  __shared__ double red[kThreads / 64][4];
  __shared__ int red_bad[kThreads / 64];
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int len = item_len(lengths, b, Tmax);
  const int n = min(kChunk, len - ch * kChunk);                // samples of this chunk
  if (n <= 0) return;                                          // the whole workgroup: nothing of this item lies here
  const int nv = min(kRun, max(0, n - tid * kRun));
  const double h = 1.0 - g;
  double x[kRun];
  bool bad = false;
  load_run(wav + (size_t)b * Tmax, (long long)ch * kChunk + tid * kRun, nv, vec != 0, quant != 0, x, bad);
  Map total;
  block_scan(run_map(x, nv, g, h), h, wave_tot, total);
  double sq = 0.0, sm = 0.0, mx = -INFINITY, mn = INFINITY;
#pragma unroll
  for (int i = 0; i < kRun; ++i)
    if (i < nv) {
      sq += x[i] * x[i];
      sm += x[i];
      mx = fmax(mx, x[i]);
      mn = fmin(mn, x[i]);
    }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {                           // butterflies of a commutative operation: every lane ends with the same bits
    sq += __shfl_xor(sq, o);
    sm += __shfl_xor(sm, o);
    mx = fmax(mx, __shfl_xor(mx, o));
    mn = fmin(mn, __shfl_xor(mn, o));
  }
  const int any_bad = __any(bad);
  if (lane == 0) {
    red[wave][0] = sq;
    red[wave][1] = sm;
    red[wave][2] = mx;
    red[wave][3] = mn;
    red_bad[wave] = any_bad;
  }
  __syncthreads();
  if (tid == 0) {
    int nb = 0;
    sq = 0.0, sm = 0.0, mx = -INFINITY, mn = INFINITY;
    for (int w = 0; w < kThreads / 64; ++w) {                  // the waves in order
      sq += red[w][0];
      sm += red[w][1];
      mx = fmax(mx, red[w][2]);
      mn = fmin(mn, red[w][3]);
      nb |= red_bad[w];
    }
    double* __restrict__ o = sums + ((size_t)b * gridDim.x + ch) * 8;
    o[0] = total.P;
    o[1] = total.Q;
    o[2] = sq;
    o[3] = sm;
    o[4] = mx;
    o[5] = mn;
    o[6] = nb ? 1.0 : 0.0;
    o[7] = (double)n;
  }
}

__global__ __launch_bounds__(64) void level_carry_kernel(const long long* __restrict__ lengths, int B, int Tmax, int nch, double g, double gC,
                                                         const double* __restrict__ sums, double* __restrict__ carry,
                                                         double* __restrict__ totals) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= B) return;
  const int len = item_len(lengths, b, Tmax);
  const int nc = (len + kChunk - 1) / kChunk;
  const double h = 1.0 - g;
  double p = 0.0, q = 0.0, sq = 0.0, sm = 0.0, mx = -INFINITY, mn = INFINITY, bad = 0.0;
  for (int ch = 0; ch < nc; ++ch) {
    const double* __restrict__ s = sums + ((size_t)b * nch + ch) * 8;
    carry[((size_t)b * nch + ch) * 2 + 0] = p;
    carry[((size_t)b * nch + ch) * 2 + 1] = q;
    const Map m{kChunk, gC, s[0], s[1]};                       // exact for every chunk but the last, whose carry-out nobody reads
    map_apply(m, p, q, h);
    sq += s[2];
    sm += s[3];
    mx = fmax(mx, s[4]);
    mn = fmin(mn, s[5]);
    bad = fmax(bad, s[6]);
  }
  double* __restrict__ t = totals + (size_t)b * 8;
  t[0] = sq;
  t[1] = sm;
  t[2] = nc ? mx : 0.0;
  t[3] = nc ? mn : 0.0;
  t[4] = bad;
  t[5] = (double)len;
}

// q >= 2^(j-15) for exactly the j below the value returned: the thresholds are powers of two, so the exponent decides.
__device__ __forceinline__ int thresholds_reached(double q) {
  if (!(q >= 0x1p-15)) return 0;
  const int e = (int)((__double_as_longlong(q) >> 52) & 0x7ff) - 1023;
  return min(e + 16, kThr);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void level_tuple_kernel(const T* __restrict__ wav, const long long* __restrict__ lengths, int Tmax,
                                                               int vec, int quant, double g, int hang, const double* __restrict__ carry,
                                                               int* __restrict__ tuples) {
  __shared__ Map wave_tot[kThreads / 64];
  __shared__ int w_last[kThreads / 64][kThr], w_first[kThreads / 64][kThr], w_count[kThreads / 64][kThr];
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int len = item_len(lengths, b, Tmax);
  const int n = min(kChunk, len - ch * kChunk);
  if (n <= 0) return;
  const int s0 = tid * kRun;
  const int nv = min(kRun, max(0, n - s0));
  const double h = 1.0 - g;
  double x[kRun];
  bool bad = false;
  load_run(wav + (size_t)b * Tmax, (long long)ch * kChunk + s0, nv, vec != 0, quant != 0, x, bad);
  Map total;
  const Map before = block_scan(run_map(x, nv, g, h), h, wave_tot, total);
  double p = carry[((size_t)b * gridDim.x + ch) * 2 + 0], q = carry[((size_t)b * gridDim.x + ch) * 2 + 1];
  map_apply(before, p, q, h);
  int lv[kRun];                                                // thresholds reached per sample
#pragma unroll
  for (int i = 0; i < kRun; ++i) {
    p = g * p + h * fabs(x[i]);
    q = g * q + h * p;
    lv[i] = i < nv ? thresholds_reached(q) : 0;
  }
  // per threshold: the last index at or above it in this run and before it in the chunk, the first one in the chunk
  int prev[kThr];
#pragma unroll
  for (int j = 0; j < kThr; ++j) {
    int last = -1, fst = kChunk;
#pragma unroll
    for (int i = 0; i < kRun; ++i)
      if (lv[i] > j) {
        last = s0 + i;
        fst = min(fst, s0 + i);
      }
    int inc = last;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int up = __shfl_up(inc, o);
      if (lane >= o) inc = max(inc, up);
    }
    int exc = __shfl_up(inc, 1);
    if (lane == 0) exc = -1;
    prev[j] = exc;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) fst = min(fst, __shfl_xor(fst, o));
    if (lane == 63) w_last[wave][j] = inc;
    if (lane == 0) w_first[wave][j] = fst;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kThr; ++j) {
    int last = prev[j];
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w)
      if (w < wave) last = max(last, w_last[w][j]);
    int c = 0;
#pragma unroll
    for (int i = 0; i < kRun; ++i) {
      const int k = s0 + i;
      if (lv[i] > j) {
        last = k;
        ++c;
      } else if (i < nv && last >= 0 && k - last <= hang) {
        ++c;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) w_count[wave][j] = c;
  }
  __syncthreads();
  if (tid < kThr) {
    int last = -1, fst = kChunk, c = 0;
    for (int w = 0; w < kThreads / 64; ++w) {
      last = max(last, w_last[w][tid]);
      fst = min(fst, w_first[w][tid]);
      c += w_count[w][tid];
    }
    int* __restrict__ o = tuples + (((size_t)b * gridDim.x + ch) * kThr + tid) * 4;
    o[0] = last >= 0 ? fst : -1;
    o[1] = last;
    o[2] = c;
    o[3] = n;
  }
}

__global__ __launch_bounds__(64) void level_final_kernel(const long long* __restrict__ lengths, int Tmax, int nch, int hang,
                                                         const double* __restrict__ totals, const int* __restrict__ tuples,
                                                         double* __restrict__ stats, long long* __restrict__ counts) {
  __shared__ long long a_s[kThr];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int len = item_len(lengths, b, Tmax);
  const int nc = (len + kChunk - 1) / kChunk;
  const double* __restrict__ t = totals + (size_t)b * 8;
  const bool bad = t[4] != 0.0;
  if (lane < kThr) {
    long long a = 0;
    long long d = hang;                                        // samples since the last crossing, saturated: the ITU loop starts saturated
    for (int ch = 0; ch < nc; ++ch) {
      const int* __restrict__ u = tuples + (((size_t)b * nch + ch) * kThr + lane) * 4;
      const int first = u[0], last = u[1], c0 = u[2], n = u[3];
      const long long enter = max(0LL, (long long)hang - d);   // samples the entering hangover still covers
      a += c0 + min((long long)(first >= 0 ? first : n), enter);
      d = last >= 0 ? (long long)(n - 1 - last) : min((long long)hang, d + n);
    }
    if (bad) a = 0;
    a_s[lane] = a;
    if (counts) counts[(size_t)b * kThr + lane] = a;
  }
  __syncthreads();
  if (lane != 0) return;
  double* __restrict__ o = stats + (size_t)b * 8;
  const double sq = t[0];
  double level = kSilent, activity = 0.0, rms = kSilent;
  if (len > 0) {
    rms = 10.0 * log10(sq / (double)len + 1e-20);
    double A[kThr], D[kThr];
    for (int j = 0; j < kThr; ++j) {
      A[j] = 10.0 * log10(sq / (a_s[j] > 0 ? (double)a_s[j] : 1e-20) + 1e-20);
      D[j] = A[j] - 20.0 * log10(ldexp(1.0, j - 15));
    }
    if (a_s[0] > 0 && !(D[0] < kMargin)) {
      for (int j = 1; j < kThr; ++j)
        if (D[j] <= kMargin) {
          const double den = D[j - 1] - D[j];
          const double w = den != 0.0 ? (D[j - 1] - kMargin) / den : 0.0;
          level = A[j - 1] + w * (A[j] - A[j - 1]);
          activity = pow(10.0, (rms - level) / 10.0);
          break;
        }
    }
  }
  if (bad) level = activity = rms = NAN;
  o[0] = level;
  o[1] = activity;
  o[2] = rms;
  o[3] = bad ? NAN : fmax(fabs(t[2]), fabs(t[3]));
  o[4] = len > 0 ? t[1] / (double)len : 0.0;
  o[5] = t[2];
  o[6] = t[3];
  o[7] = (double)len;
}

// The gain of an item from its measured level: 1 where there is no measurable speech (-100) or the level is NaN.
__device__ __forceinline__ double gain_of(double level, double ndb) {
  if (!isfinite(level) || level <= kSilent) return 1.0;
  return pow(10.0, (ndb - level) / 20.0);
}

__device__ __forceinline__ float out_sample(float v, bool quant, double factor, float*, int&) {
  if (!isfinite(v)) return v;                                  // only in an item that is left unchanged (factor 1)
  const double x = quant ? (double)quantize_ref(v) * (1.0 / 32768.0) : (double)v;
  return (float)(x * factor);
}
__device__ __forceinline__ float out_sample(short v, bool, double factor, float*, int&) { return (float)((double)v * (1.0 / 32768.0) * factor); }
__device__ __forceinline__ short to_i16(double y, int& clipped) {
  const double r = round(y);                                   // half away from zero
  if (r > 32767.0) {
    ++clipped;
    return 32767;
  }
  if (r < -32768.0) {
    ++clipped;
    return -32768;
  }
  return (short)(int)r;
}
__device__ __forceinline__ short out_sample(float v, bool quant, double factor, short*, int& clipped) {
  if (!isfinite(v)) return 0;
  const double x = quant ? (double)quantize_ref(v) * (1.0 / 32768.0) : (double)v;
  return to_i16(x * factor * 32768.0, clipped);
}
__device__ __forceinline__ short out_sample(short v, bool, double factor, short*, int& clipped) {
  return to_i16((double)v * (1.0 / 32768.0) * factor * 32768.0, clipped);
}

__device__ __forceinline__ void load_unit(const float* __restrict__ p, float (&v)[kUnit]) {
  const float4 a = *reinterpret_cast<const float4*>(p), c = *reinterpret_cast<const float4*>(p + 4);
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w, v[4] = c.x, v[5] = c.y, v[6] = c.z, v[7] = c.w;
}
__device__ __forceinline__ void load_unit(const short* __restrict__ p, short (&v)[kUnit]) {
  const int4 w = *reinterpret_cast<const int4*>(p);
  const int d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    v[2 * e] = (short)(d[e] & 0xffff);
    v[2 * e + 1] = (short)(d[e] >> 16);
  }
}
__device__ __forceinline__ void store_unit(float* __restrict__ p, const float (&v)[kUnit]) {
  *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  *reinterpret_cast<float4*>(p + 4) = make_float4(v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void store_unit(short* __restrict__ p, const short (&v)[kUnit]) {
  int d[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) d[e] = (int)((unsigned)(unsigned short)v[2 * e] | ((unsigned)(unsigned short)v[2 * e + 1] << 16));
  *reinterpret_cast<int4*>(p) = make_int4(d[0], d[1], d[2], d[3]);
}

// Every sample of the row below Tmax is written: x * factor below the item's length, 0 from there on (those are never read).
template <typename TI, typename TO>
__global__ __launch_bounds__(kThreads) void level_apply_kernel(const TI* __restrict__ wav, const long long* __restrict__ lengths, int Tmax,
                                                               int vec, int quant, const double* __restrict__ stats, double ndb,
                                                               TO* __restrict__ out, int* __restrict__ clipped) {
  __shared__ int red[kThreads / 64];
  const int b = blockIdx.y, ch = blockIdx.x, tid = threadIdx.x;
  const int len = item_len(lengths, b, Tmax);
  const double factor = gain_of(stats[(size_t)b * 8], ndb);
  const TI* __restrict__ src = wav + (size_t)b * Tmax;
  TO* __restrict__ dst = out + (size_t)b * Tmax;
  int clip = 0;
#pragma unroll
  for (int i = 0; i < kChunk / (kUnit * kThreads); ++i) {
    const long long s = (long long)ch * kChunk + (long long)(i * kThreads + tid) * kUnit;
    if (s >= Tmax) continue;
    const int live = (int)max(0LL, min((long long)kUnit, (long long)len - s));
    const int room = (int)min((long long)kUnit, (long long)Tmax - s);
    TI v[kUnit];
    if (vec && live == kUnit) {
      load_unit(src + s, v);
    } else {
#pragma unroll
      for (int e = 0; e < kUnit; ++e) v[e] = e < live ? src[s + e] : (TI)0;
    }
    TO y[kUnit];
#pragma unroll
    for (int e = 0; e < kUnit; ++e) y[e] = e < live ? out_sample(v[e], quant != 0, factor, (TO*)nullptr, clip) : (TO)0;
    if (vec) {                                                 // Tmax is a multiple of kUnit then: the unit lies inside the row
      store_unit(dst + s, y);
    } else {
#pragma unroll
      for (int e = 0; e < kUnit; ++e)
        if (e < room) dst[s + e] = y[e];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) clip += __shfl_xor(clip, o);
  if ((tid & 63) == 0) red[tid >> 6] = clip;
  __syncthreads();
  if (tid == 0) {
    int c = 0;
    for (int w = 0; w < kThreads / 64; ++w) c += red[w];
    clipped[(size_t)b * gridDim.x + ch] = c;
  }
}

__global__ __launch_bounds__(64) void level_gain_kernel(int nch, const double* __restrict__ stats, double ndb, const int* __restrict__ clipped,
                                                        double* __restrict__ gain, long long* __restrict__ clipped_out) {
  const int b = blockIdx.x, lane = threadIdx.x;
  long long c = 0;
  for (int ch = lane; ch < nch; ch += 64) c += clipped[(size_t)b * nch + ch];
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
  if (lane == 0) {
    if (gain) gain[b] = gain_of(stats[(size_t)b * 8], ndb);
    if (clipped_out) clipped_out[b] = c;
  }
}

bool dtype_ok(int d) { return d == US_LEVEL_F32 || d == US_LEVEL_I16; }
bool shape_ok(int B, int Tmax) { return B >= 1 && B <= 65535 && Tmax >= 1 && Tmax <= (1 << 30); }
bool aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }
// whether every row of [B][Tmax] elements of `bytes` bytes starts on a 16-byte boundary and holds whole 16-byte vectors
bool rows_vector(const void* p, int Tmax, int bytes) { return aligned16(p) && Tmax % (16 / bytes) == 0; }

}  // namespace
}  // namespace us

using namespace us;

extern "C" {

int us_level_chunk(void) { return kChunk; }

size_t us_level_workspace_bytes(int B, int Tmax) { return shape_ok(B, Tmax) ? work_bytes(B, Tmax) : 0; }

int us_level_measure(const void* wav, int in_dtype, int quantize_input, const int64_t* lengths, int B, int Tmax, int sample_rate, double* stats,
                     int64_t* counts, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (sample_rate <= 0) return bad_arg("us_level_measure: the sample rate must be positive");
  if (!shape_ok(B, Tmax)) return bad_arg("us_level_measure: B must be in [1, 65535] and Tmax in [1, 2^30]");
  if (!dtype_ok(in_dtype)) return bad_arg("us_level_measure: in_dtype must be US_LEVEL_F32 or US_LEVEL_I16");
  if (!wav || !stats || !workspace) return bad_arg("us_level_measure: bad argument");
  if (workspace_bytes < work_bytes(B, Tmax)) {
    set_last_error("us_level_measure: the workspace is smaller than us_level_workspace_bytes");
    return US_EWORKSPACE;
  }
  const double g = exp(-1.0 / ((double)sample_rate * 0.03)), gC = exp(-(double)kChunk / ((double)sample_rate * 0.03));
  const int hang = (int)floor(0.2 * (double)sample_rate + 0.5);
  const int nch = chunks_of(Tmax);
  const Work w = carve(workspace, B, Tmax);
  const long long* lens = reinterpret_cast<const long long*>(lengths);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(nch, B);
  const int quant = in_dtype == US_LEVEL_F32 && quantize_input;
  if (in_dtype == US_LEVEL_F32) {
    const float* x = static_cast<const float*>(wav);
    const int vec = rows_vector(x, Tmax, 4);
    hipLaunchKernelGGL(level_summary_kernel<float>, grid, dim3(kThreads), 0, s, x, lens, Tmax, vec, quant, g, w.sums);
    hipLaunchKernelGGL(level_carry_kernel, dim3((B + 63) / 64), dim3(64), 0, s, lens, B, Tmax, nch, g, gC, w.sums, w.carry, w.totals);
    hipLaunchKernelGGL(level_tuple_kernel<float>, grid, dim3(kThreads), 0, s, x, lens, Tmax, vec, quant, g, hang, w.carry, w.tuples);
  } else {
    const short* x = static_cast<const short*>(wav);
    const int vec = rows_vector(x, Tmax, 2);
    hipLaunchKernelGGL(level_summary_kernel<short>, grid, dim3(kThreads), 0, s, x, lens, Tmax, vec, 0, g, w.sums);
    hipLaunchKernelGGL(level_carry_kernel, dim3((B + 63) / 64), dim3(64), 0, s, lens, B, Tmax, nch, g, gC, w.sums, w.carry, w.totals);
    hipLaunchKernelGGL(level_tuple_kernel<short>, grid, dim3(kThreads), 0, s, x, lens, Tmax, vec, 0, g, hang, w.carry, w.tuples);
  }
  hipLaunchKernelGGL(level_final_kernel, dim3(B), dim3(64), 0, s, lens, Tmax, nch, hang, w.totals, w.tuples, stats,
                     reinterpret_cast<long long*>(counts));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_level_measure", e);
}

int us_level_apply(const void* wav, int in_dtype, int quantize_input, const int64_t* lengths, int B, int Tmax, const double* stats, double ndb,
                   void* out, int out_dtype, double* gain, int64_t* clipped, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!shape_ok(B, Tmax)) return bad_arg("us_level_apply: B must be in [1, 65535] and Tmax in [1, 2^30]");
  if (!dtype_ok(in_dtype) || !dtype_ok(out_dtype)) return bad_arg("us_level_apply: a dtype must be US_LEVEL_F32 or US_LEVEL_I16");
  if (!wav || !stats || !out || !workspace || !std::isfinite(ndb)) return bad_arg("us_level_apply: bad argument");
  if (workspace_bytes < work_bytes(B, Tmax)) {
    set_last_error("us_level_apply: the workspace is smaller than us_level_workspace_bytes");
    return US_EWORKSPACE;
  }
  const int nch = chunks_of(Tmax);
  const Work w = carve(workspace, B, Tmax);
  const long long* lens = reinterpret_cast<const long long*>(lengths);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const dim3 grid(nch, B);
  const int quant = in_dtype == US_LEVEL_F32 && quantize_input;
  const int vec = aligned16(wav) && aligned16(out) && Tmax % kUnit == 0;
  if (in_dtype == US_LEVEL_F32 && out_dtype == US_LEVEL_F32)
    hipLaunchKernelGGL((level_apply_kernel<float, float>), grid, dim3(kThreads), 0, s, static_cast<const float*>(wav), lens, Tmax, vec, quant,
                       stats, ndb, static_cast<float*>(out), w.clipped);
  else if (in_dtype == US_LEVEL_F32)
    hipLaunchKernelGGL((level_apply_kernel<float, short>), grid, dim3(kThreads), 0, s, static_cast<const float*>(wav), lens, Tmax, vec, quant,
                       stats, ndb, static_cast<short*>(out), w.clipped);
  else if (out_dtype == US_LEVEL_F32)
    hipLaunchKernelGGL((level_apply_kernel<short, float>), grid, dim3(kThreads), 0, s, static_cast<const short*>(wav), lens, Tmax, vec, 0, stats,
                       ndb, static_cast<float*>(out), w.clipped);
  else
    hipLaunchKernelGGL((level_apply_kernel<short, short>), grid, dim3(kThreads), 0, s, static_cast<const short*>(wav), lens, Tmax, vec, 0, stats,
                       ndb, static_cast<short*>(out), w.clipped);
  hipLaunchKernelGGL(level_gain_kernel, dim3(B), dim3(64), 0, s, nch, stats, ndb, w.clipped, gain, reinterpret_cast<long long*>(clipped));
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_level_apply", e);
}

}  // extern "C"
