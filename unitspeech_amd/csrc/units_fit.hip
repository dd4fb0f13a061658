// Fitting the unit codebook on the device: the half of a k-means iteration that us_units_quantize does not do.
//
//   us_units_fit_accumulate  labels [rows] (us_units_quantize's: -1 = not a row) and features [rows][D] -> added into the state: fp64
//                            sums [K][D], int64 counts [K], the fp64 inertia sum (x_d - c_label,d)^2, rows used and skipped.
//                            No float atomics: an inverted index (per-chunk histograms laid out [k][chunk], one exclusive scan, a
//                            stable scatter of row numbers, so every centre's list is in ascending row order), then one workgroup
//                            per (centre, 512-row piece of its list) reads each row once, coalesced along D, and adds in fp64 in list
//                            order (four waves, a quarter each, joined in wave order); a last pass adds the pieces of a centre in
//                            piece order.  Same bits on every run.
//   us_units_fit_update      Lloyd: c = fp32(sum / count); mini-batch: c = fp32((c total + sum) / (total + count)); a centre without
//                            rows keeps its value.  Writes the record {inertia, shift2, empty, used, skipped} and clears the state.
//   us_units_fit_seed_step   one step of plain D^2 k-means++: fp64 mind[rows], a blocked fixed-order inclusive scan, the smallest
//                            valid row whose cumulative sum exceeds u * total (uniform over the valid rows on step 0 and when the
//                            total is 0).
//
// Every dependency between workgroups is a kernel boundary; every loop's bound is a launch argument or a constant.
#include <hip/hip_runtime.h>

#include <cfloat>
#include <cmath>
#include <cstdio>

#include "../../include/unitspeech_hip.h"
#include "handle.h"
#include "kernels.h"
#include "units_fit_layout.h"

namespace us {
namespace {

using namespace fit;

struct SeedSel {
  int block;          // block of kSeedBlock rows that holds the pick (-1: no valid row)
  int uniform;        // 1: count valid rows, 0: sum mind
  double prefix;      // cumulative sum before the block
  double target;      // u * total
  long long prefix_n; // valid rows before the block
  long long target_n; // floor(u * n_valid), clamped
};

// ---- inverted index --------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void stage_labels(const long long* __restrict__ labels, int* lab, int r0, int rows, int K) {
  for (int i = threadIdx.x; i < kRowChunk; i += 256) {
    const int row = r0 + i;
    const long long l = row < rows ? labels[row] : -1;
    lab[i] = (l >= 0 && l < (long long)K) ? (int)l : -1;
  }
}

// grid (nchunks, ceil(K / 256)): thread = one centre, counts its rows in the chunk; offs is [K][nchunks]
__global__ __launch_bounds__(256) void uf_hist_kernel(const long long* __restrict__ labels, int* __restrict__ offs, int* __restrict__ skip,
                                                      int rows, int K, int nchunks) {
  __shared__ __attribute__((aligned(16))) int lab[kRowChunk];
  __shared__ int red[256];
  const int chunk = blockIdx.x, r0 = chunk * kRowChunk, tid = threadIdx.x;
  stage_labels(labels, lab, r0, rows, K);
  __syncthreads();
  const int k = blockIdx.y * 256 + tid;
  if (k < K) {
    int c = 0;
    for (int i = 0; i < kRowChunk; i += 4) {
      const int4 v = *reinterpret_cast<const int4*>(&lab[i]);
      c += (v.x == k) + (v.y == k) + (v.z == k) + (v.w == k);
    }
    offs[(size_t)k * nchunks + chunk] = c;
  }
  if (blockIdx.y == 0) {
    int s = 0;
    for (int i = tid * 4; i < tid * 4 + 4; ++i) s += (r0 + i < rows && lab[i] < 0) ? 1 : 0;
    red[tid] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
      if (tid < o) red[tid] += red[tid + o];
      __syncthreads();
    }
    if (tid == 0) skip[chunk] = red[0];
  }
}

// blocked exclusive scan of offs[0, m) in place, offs[m] = the total: block sums, one workgroup over them, apply
__device__ __forceinline__ int block_exclusive_scan(int v, int* scan) {   // returns the exclusive prefix of the thread; scan[255] = total
  const int tid = threadIdx.x;
  scan[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const int a = tid >= o ? scan[tid - o] : 0;
    __syncthreads();
    scan[tid] += a;
    __syncthreads();
  }
  return scan[tid] - v;
}

__global__ __launch_bounds__(256) void uf_scan_sums_kernel(const int* __restrict__ offs, int* __restrict__ bsum, long long m) {
  __shared__ int scan[256];
  const long long i0 = (long long)blockIdx.x * kScanItems + threadIdx.x * 16;
  int s = 0;
  for (int i = 0; i < 16; ++i) s += i0 + i < m ? offs[i0 + i] : 0;
  block_exclusive_scan(s, scan);
  if (threadIdx.x == 0) bsum[blockIdx.x] = scan[255];
}

__global__ __launch_bounds__(256) void uf_scan_top_kernel(int* __restrict__ bsum, int* __restrict__ offs, int nscan, long long m) {
  __shared__ int scan[256];
  const int span = (nscan + 255) / 256, b0 = threadIdx.x * span;
  int s = 0;
  for (int i = 0; i < span; ++i) s += b0 + i < nscan ? bsum[b0 + i] : 0;
  int run = block_exclusive_scan(s, scan);
  for (int i = 0; i < span; ++i) {
    if (b0 + i < nscan) {
      const int v = bsum[b0 + i];
      bsum[b0 + i] = run;
      run += v;
    }
  }
  if (threadIdx.x == 0) offs[m] = scan[255];
}

__global__ __launch_bounds__(256) void uf_scan_apply_kernel(int* __restrict__ offs, const int* __restrict__ bsum, long long m) {
  __shared__ int scan[256];
  const long long i0 = (long long)blockIdx.x * kScanItems + threadIdx.x * 16;
  int v[16], s = 0;
  for (int i = 0; i < 16; ++i) {
    v[i] = i0 + i < m ? offs[i0 + i] : 0;
    s += v[i];
  }
  int run = block_exclusive_scan(s, scan) + bsum[blockIdx.x];
  for (int i = 0; i < 16; ++i) {
    if (i0 + i < m) offs[i0 + i] = run;
    run += v[i];
  }
}

// cstart[k] = first (centre, list piece) work item of centre k, cstart[K] = their number
__global__ __launch_bounds__(256) void uf_table_kernel(const int* __restrict__ offs, int* __restrict__ cstart, int K, int nchunks) {
  __shared__ int scan[256];
  const int span = (K + 255) / 256, k0 = threadIdx.x * span;
  int s = 0;
  for (int i = 0; i < span; ++i) {
    const int k = k0 + i;
    if (k < K) s += (offs[(size_t)(k + 1) * nchunks] - offs[(size_t)k * nchunks] + kListChunk - 1) / kListChunk;
  }
  int run = block_exclusive_scan(s, scan);
  for (int i = 0; i < span; ++i) {
    const int k = k0 + i;
    if (k < K) {
      cstart[k] = run;
      run += (offs[(size_t)(k + 1) * nchunks] - offs[(size_t)k * nchunks] + kListChunk - 1) / kListChunk;
    }
  }
  if (threadIdx.x == 0) cstart[K] = scan[255];
}

// thread = one centre: walks the chunk's labels in row order, so its list comes out ascending
__global__ __launch_bounds__(256) void uf_scatter_kernel(const long long* __restrict__ labels, const int* __restrict__ offs,
                                                         int* __restrict__ index, int rows, int K, int nchunks) {
  __shared__ __attribute__((aligned(16))) int lab[kRowChunk];
  const int chunk = blockIdx.x, r0 = chunk * kRowChunk;
  stage_labels(labels, lab, r0, rows, K);
  __syncthreads();
  const int k = blockIdx.y * 256 + threadIdx.x;
  if (k >= K) return;
  int pos = offs[(size_t)k * nchunks + chunk];
  const int end = offs[(size_t)k * nchunks + chunk + 1];      // the next (centre, chunk) entry, or offs[m]: this entry's count bounds the writes
  for (int i = 0; i < kRowChunk; i += 4) {
    const int4 v = *reinterpret_cast<const int4*>(&lab[i]);
    if (v.x == k && pos < end) index[pos++] = r0 + i;
    if (v.y == k && pos < end) index[pos++] = r0 + i + 1;
    if (v.z == k && pos < end) index[pos++] = r0 + i + 2;
    if (v.w == k && pos < end) index[pos++] = r0 + i + 3;
  }
}

// ---- gather-sum ------------------------------------------------------------------------------------------------------------------
// One workgroup per work item (centre k, piece j of kListChunk rows of its list); wave v of the four takes the v-th quarter of the piece's rows.
// Lane l owns the features [4 (64 i + l), + 4) for i < NV, so a row is read once with float4 loads that are contiguous across the
// wave.  U rows are in flight per wave; they are added in list order, and the four quarters are joined in wave order through LDS.
template <int NV, int U>
__global__ __launch_bounds__(256) void uf_gather_kernel(const float* __restrict__ X, const float* __restrict__ C, const int* __restrict__ index,
                                                        const int* __restrict__ offs, const int* __restrict__ cstart,
                                                        double* __restrict__ part, double* __restrict__ pin, int K, int D, int nchunks) {
  __shared__ double join[3][NV * 4 + 1][64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int w = blockIdx.x;
  if (w >= cstart[K]) return;                               // the same for the whole workgroup
  int lo = 0, hi = K;                                       // the k with cstart[k] <= w < cstart[k + 1]
  for (int it = 0; it < 12 && hi - lo > 1; ++it) {
    const int mid = (lo + hi) >> 1;
    if (cstart[mid] <= w) lo = mid; else hi = mid;
  }
  const int k = lo, j = w - cstart[k];
  const int lbeg = offs[(size_t)k * nchunks], lend = offs[(size_t)(k + 1) * nchunks];
  const int pbeg = lbeg + j * kListChunk, pn = min(kListChunk, lend - pbeg);
  const int quarter = (pn + 3) / 4;                         // the piece's rows in four equal runs, one per wave
  const int beg = pbeg + wave * quarter;
  const int n = max(0, min(quarter, pbeg + pn - beg));
  bool live[NV];
  double c[NV][4], acc[NV][4], ia = 0.0;
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int d = 4 * (64 * v + lane);
    live[v] = d < D;
    const float4 cv = live[v] ? *reinterpret_cast<const float4*>(C + (size_t)k * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
    c[v][0] = cv.x, c[v][1] = cv.y, c[v][2] = cv.z, c[v][3] = cv.w;
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[v][e] = 0.0;
  }
  for (int i = 0; i < n; i += U) {
    float4 x[U][NV];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int r = i + u < n ? index[beg + i + u] : -1;
#pragma unroll
      for (int v = 0; v < NV; ++v)
        x[u][v] = (r >= 0 && live[v]) ? *reinterpret_cast<const float4*>(X + (size_t)r * D + 4 * (64 * v + lane)) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (i + u < n) {
#pragma unroll
        for (int v = 0; v < NV; ++v) {
          const double xv[4] = {(double)x[u][v].x, (double)x[u][v].y, (double)x[u][v].z, (double)x[u][v].w};
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            acc[v][e] += xv[e];
            const double df = live[v] ? xv[e] - c[v][e] : 0.0;
            ia = fma(df, df, ia);
          }
        }
      }
    }
  }
  if (wave > 0) {
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) join[wave - 1][v * 4 + e][lane] = acc[v][e];
    join[wave - 1][NV * 4][lane] = ia;
  }
  __syncthreads();
  if (wave > 0) return;
  for (int q = 0; q < 3; ++q) {                             // quarters in order; an empty quarter adds zeros
#pragma unroll
    for (int v = 0; v < NV; ++v)
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[v][e] += join[q][v * 4 + e][lane];
    ia += join[q][NV * 4][lane];
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    if (live[v]) {
      double* p = part + (size_t)w * D + 4 * (64 * v + lane);
      *reinterpret_cast<double2*>(p) = make_double2(acc[v][0], acc[v][1]);
      *reinterpret_cast<double2*>(p + 2) = make_double2(acc[v][2], acc[v][3]);
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) ia += __shfl_xor(ia, o);   // a fixed butterfly: every lane ends with the same bits
  if (lane == 0) pin[w] = ia;
}

// block (k < K, y): sums[k][256 y + tid] += the pieces of centre k in piece order, counts[k] += its rows.  Block (K, 0): the scalars.
__global__ __launch_bounds__(256) void uf_reduce_kernel(const double* __restrict__ part, const double* __restrict__ pin,
                                                        const int* __restrict__ offs, const int* __restrict__ cstart,
                                                        const int* __restrict__ skip, double* __restrict__ sums, long long* __restrict__ counts,
                                                        long long* __restrict__ scalars, int K, int D, int nchunks, int max_items) {
  __shared__ double red[256];
  __shared__ int redi[256];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < K) {
    const int k = blockIdx.x, c0 = cstart[k], c1 = min(cstart[k + 1], max_items);
    const int d = blockIdx.y * 256 + tid;
    if (d < D) {
      double s = sums[(size_t)k * D + d];
      int wi = c0;
      for (; wi + 8 <= c1; wi += 8) {                       // eight loads in flight, added in piece order
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = part[(size_t)(wi + u) * D + d];
#pragma unroll
        for (int u = 0; u < 8; ++u) s += v[u];
      }
      for (; wi < c1; ++wi) s += part[(size_t)wi * D + d];
      sums[(size_t)k * D + d] = s;
    }
    if (tid == 0 && blockIdx.y == 0) counts[k] += (long long)(offs[(size_t)(k + 1) * nchunks] - offs[(size_t)k * nchunks]);
    return;
  }
  if (blockIdx.y != 0) return;
  const int items = min(cstart[K], max_items);
  const int span = (max_items + 255) / 256;
  double s = 0.0;
  for (int i = 0; i < span; ++i) {
    const int wi = tid * span + i;
    if (wi < items) s += pin[wi];
  }
  int sk = 0;
  for (int i = tid; i < nchunks; i += 256) sk += skip[i];
  red[tid] = s;
  redi[tid] = sk;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o];
      redi[tid] += redi[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double* inertia = reinterpret_cast<double*>(scalars);
    inertia[0] += red[0];
    scalars[1] += (long long)offs[(size_t)K * nchunks];
    scalars[2] += (long long)redi[0];
  }
}

// ---- update ----------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double blend(double c, double total, double sum, double n) {
#pragma clang fp contract(off)
  return (c * total + sum) / (total + n);
}

// block = one centre.  cin and cout may be the same buffer (every element is read and written by one thread).
__global__ __launch_bounds__(256) void uf_update_kernel(const float* cin, float* cout, const long long* __restrict__ totals_in,
                                                        double* __restrict__ sums, const long long* __restrict__ counts,
                                                        double* __restrict__ shift, int D, int minibatch) {
  __shared__ double red[256];
  const int k = blockIdx.x, tid = threadIdx.x;
  const long long n = counts[k];
  const double total = minibatch && totals_in ? (double)totals_in[k] : 0.0;
  double sh = 0.0;
  for (int d = tid; d < D; d += 256) {
    const size_t i = (size_t)k * D + d;
    const float old = cin[i];
    float nw = old;
    if (n > 0) nw = (float)(minibatch ? blend((double)old, total, sums[i], (double)n) : sums[i] / (double)n);
    cout[i] = nw;
    const double df = (double)nw - (double)old;
    sh = fma(df, df, sh);
    sums[i] = 0.0;
  }
  red[tid] = sh;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  if (tid == 0) shift[k] = red[0];
}

// one workgroup: the record, the running totals, and the rest of the state cleared
__global__ __launch_bounds__(256) void uf_record_kernel(const long long* totals_in, long long* totals_out, long long* __restrict__ counts,
                                                        const double* __restrict__ shift, long long* __restrict__ scalars,
                                                        long long* __restrict__ record, int K, int minibatch) {
  __shared__ double red[256];
  __shared__ int redi[256];
  const int tid = threadIdx.x, span = (K + 255) / 256;
  double s = 0.0;
  int empty = 0;
  for (int i = 0; i < span; ++i) {
    const int k = tid * span + i;
    if (k < K) {
      const long long n = counts[k];
      s += shift[k];
      empty += n == 0;
      if (totals_out) totals_out[k] = (minibatch && totals_in ? totals_in[k] : 0) + n;
      counts[k] = 0;
    }
  }
  red[tid] = s;
  redi[tid] = empty;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o];
      redi[tid] += redi[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    record[0] = scalars[0];                                  // the inertia's bits
    reinterpret_cast<double*>(record)[1] = red[0];
    record[2] = redi[0];
    record[3] = scalars[1];
    record[4] = scalars[2];
    scalars[0] = scalars[1] = scalars[2] = scalars[3] = 0;
  }
}

// ---- seeding ---------------------------------------------------------------------------------------------------------------------
// 128 rows per workgroup, 32 features at a time through LDS: the loads are whole cache lines, and thread t then walks row t with d
// ascending.  c == nullptr: mind = +inf on a valid row (t < lengths[b], every feature finite), -1 otherwise.  Else
// mind = min(mind, sum_d (x_d - c_d)^2) on the valid rows.
__global__ __launch_bounds__(128) void uf_seed_dist_kernel(const float* __restrict__ X, const long long* __restrict__ lengths,
                                                           const float* __restrict__ cbase, int prev,
                                                           double* __restrict__ mind, int rows, int Tmax, int D) {
  __shared__ float tile[128][33];
  __shared__ float cs[32];
  const int tid = threadIdx.x, r0 = blockIdx.x * 128;
  const float* __restrict__ c = cbase ? cbase + (size_t)prev * D : nullptr;
  double s = 0.0;
  int bad = 0;
  for (int d0 = 0; d0 < D; d0 += 32) {
    __syncthreads();
    for (int i = 0; i < 8; ++i) {
      const int idx = i * 128 + tid, rr = idx >> 3, q = (idx & 7) * 4;
      const int row = r0 + rr, d = d0 + q;
      const float4 v = (row < rows && d < D) ? *reinterpret_cast<const float4*>(X + (size_t)row * D + d) : make_float4(0.f, 0.f, 0.f, 0.f);
      tile[rr][q + 0] = v.x;
      tile[rr][q + 1] = v.y;
      tile[rr][q + 2] = v.z;
      tile[rr][q + 3] = v.w;
    }
    if (tid < 32) cs[tid] = (c && d0 + tid < D) ? c[d0 + tid] : 0.f;
    __syncthreads();
    const int nd = min(32, D - d0);
    for (int d = 0; d < nd; ++d) {
      const float v = tile[tid][d];
      bad |= !(fabsf(v) <= FLT_MAX);
      const double df = (double)v - (double)cs[d];
      s = fma(df, df, s);
    }
  }
  const int row = r0 + tid;
  if (row >= rows) return;
  if (!c) {
    const int b = row / Tmax, t = row - b * Tmax;
    mind[row] = (!bad && (long long)t < lengths[b]) ? INFINITY : -1.0;
  } else {
    const double m = mind[row];
    if (m >= 0.0 && s < m) mind[row] = s;
  }
}

__device__ __forceinline__ double seed_weight(double m, int uniform) { return m >= 0.0 ? (uniform ? 1.0 : m) : 0.0; }

// per block of kSeedBlock rows: the fp64 sum of mind over the valid rows (thread = 4 consecutive rows, then a fixed tree) and their number
__global__ __launch_bounds__(256) void uf_seed_bsum_kernel(const double* __restrict__ mind, double* __restrict__ bsum, int* __restrict__ bcnt,
                                                           int rows, int first) {
  __shared__ double red[256];
  __shared__ int redi[256];
  const int tid = threadIdx.x, r0 = blockIdx.x * kSeedBlock + tid * 4;
  double s = 0.0;
  int n = 0;
  for (int i = 0; i < 4; ++i) {
    const double m = r0 + i < rows ? mind[r0 + i] : -1.0;
    n += m >= 0.0;
    s += first ? 0.0 : seed_weight(m, 0);
  }
  red[tid] = s;
  redi[tid] = n;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) {
      red[tid] += red[tid + o];
      redi[tid] += redi[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    bsum[blockIdx.x] = red[0];
    bcnt[blockIdx.x] = redi[0];
  }
}

// one workgroup over the block sums: totals, the mode, and the first block whose inclusive cumulative sum exceeds the target
__global__ __launch_bounds__(256) void uf_seed_block_kernel(const double* __restrict__ bsum, const int* __restrict__ bcnt, SeedSel* __restrict__ sel,
                                                            int nb, int first, double u) {
  __shared__ double sd[256];
  __shared__ long long sn[256];
  __shared__ int cand, last;
  const int tid = threadIdx.x, span = (nb + 255) / 256, b0 = tid * span;
  double td = 0.0;
  long long tn = 0;
  for (int i = 0; i < span; ++i) {
    if (b0 + i < nb) {
      td += bsum[b0 + i];
      tn += bcnt[b0 + i];
    }
  }
  sd[tid] = td;
  sn[tid] = tn;
  if (tid == 0) cand = 0x7fffffff, last = -1;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const double a = tid >= o ? sd[tid - o] : 0.0;
    const long long b = tid >= o ? sn[tid - o] : 0;
    __syncthreads();
    sd[tid] += a;
    sn[tid] += b;
    __syncthreads();
  }
  const double total = sd[255];
  const long long nvalid = sn[255];
  const int uniform = first || !(total > 0.0) || !(total <= DBL_MAX);
  const double target = u * total;
  long long target_n = (long long)floor(u * (double)nvalid);
  target_n = target_n < 0 ? 0 : (target_n > nvalid - 1 ? nvalid - 1 : target_n);
  double pd = tid ? sd[tid - 1] : 0.0;
  long long pn = tid ? sn[tid - 1] : 0;
  double my_pd = 0.0;
  long long my_pn = 0;
  int mine = -1;
  for (int i = 0; i < span; ++i) {
    const int b = b0 + i;
    if (b >= nb) break;
    const double nd = pd + bsum[b];
    const long long nn = pn + bcnt[b];
    const bool has = uniform ? bcnt[b] > 0 : bsum[b] > 0.0;
    if (has) atomicMax(&last, b);
    if (mine < 0 && has && (uniform ? nn > target_n : nd > target)) {
      mine = b;
      my_pd = pd;
      my_pn = pn;
    }
    pd = nd;
    pn = nn;
  }
  if (mine >= 0) atomicMin(&cand, mine);
  __syncthreads();
  const int pick = nvalid <= 0 ? -1 : (cand != 0x7fffffff ? cand : last);
  if (tid == 0 && pick < 0) {
    sel->block = -1;
    sel->uniform = uniform;
  }
  if (pick >= 0 && pick >= b0 && pick < b0 + span) {
    if (mine != pick) {                                     // the rounding fallback: recompute the prefix of the last non-empty block
      my_pd = tid ? sd[tid - 1] : 0.0;
      my_pn = tid ? sn[tid - 1] : 0;
      for (int b = b0; b < pick; ++b) {
        my_pd += bsum[b];
        my_pn += bcnt[b];
      }
    }
    sel->block = pick;
    sel->uniform = uniform;
    sel->prefix = my_pd;
    sel->target = target;
    sel->prefix_n = my_pn;
    sel->target_n = target_n;
  }
}

// one workgroup over the chosen block: the smallest valid row whose inclusive cumulative sum exceeds the target becomes centre `step`
__global__ __launch_bounds__(256) void uf_seed_row_kernel(const float* __restrict__ X, const double* __restrict__ mind, const SeedSel* __restrict__ sel,
                                                          float* __restrict__ centers, long long* __restrict__ picked, int rows, int D, int step) {
  __shared__ double sd[256];
  __shared__ int cand, last;
  const int tid = threadIdx.x;
  const int block = sel->block, uniform = sel->uniform;
  if (block < 0) {
    if (tid == 0) picked[step] = -1;
    return;
  }
  const int r0 = block * kSeedBlock + tid * 4;
  double w[4], t = 0.0;
  for (int i = 0; i < 4; ++i) {
    w[i] = seed_weight(r0 + i < rows ? mind[r0 + i] : -1.0, uniform);
    t += w[i];
  }
  sd[tid] = t;
  if (tid == 0) cand = 0x7fffffff, last = -1;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const double a = tid >= o ? sd[tid - o] : 0.0;
    __syncthreads();
    sd[tid] += a;
    __syncthreads();
  }
  const double base = uniform ? (double)sel->prefix_n : sel->prefix;
  const double target = uniform ? (double)sel->target_n : sel->target;   // counts are exact in fp64
  double p = base + (tid ? sd[tid - 1] : 0.0);
  int mine = -1;
  for (int i = 0; i < 4; ++i) {
    p += w[i];
    if (w[i] > 0.0) {
      atomicMax(&last, r0 + i);
      if (mine < 0 && p > target) mine = r0 + i;
    }
  }
  if (mine >= 0) atomicMin(&cand, mine);
  __syncthreads();
  const int row = cand != 0x7fffffff ? cand : last;
  if (row < 0) {
    if (tid == 0) picked[step] = -1;
    return;
  }
  if (tid == 0) picked[step] = row;
  for (int d = tid * 4; d < D; d += 1024)
    *reinterpret_cast<float4*>(centers + (size_t)step * D + d) = *reinterpret_cast<const float4*>(X + (size_t)row * D + d);
}

// ---- host ------------------------------------------------------------------------------------------------------------------------
int uf_bad(const char* what, int64_t rows, int K, int D) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: K must be in [1, 2048], D a multiple of 4 in [4, 1024], rows in [1, 2^24] (K = %d, D = %d, rows = %lld)", what,
           K, D, (long long)rows);
  set_last_error(buf);
  return US_EINVAL;
}
int uf_small(const char* msg) {
  set_last_error(msg);
  return US_EWORKSPACE;
}

}  // namespace
}  // namespace us

using namespace us;

extern "C" {

size_t us_units_fit_workspace_bytes(int64_t rows, int K, int D) {
  if (!shape_ok(K, D) || !rows_ok(rows)) return 0;
  return work_layout(rows, K, D).total;
}

size_t us_units_fit_state_bytes(int K, int D) {
  if (!shape_ok(K, D)) return 0;
  return state_layout(K, D).total;
}

int us_units_fit_state_clear(void* state, size_t state_bytes, int K, int D, us_stream stream) {
  if (!shape_ok(K, D)) return uf_bad("us_units_fit_state_clear", 1, K, D);
  const size_t n = state_layout(K, D).total;
  if (!state || state_bytes < n) return uf_small("us_units_fit_state_clear: state too small (us_units_fit_state_bytes)");
  hipError_t e = hipMemsetAsync(state, 0, n, static_cast<hipStream_t>(stream));
  return e == hipSuccess ? US_OK : hip_fail("us_units_fit_state_clear", e);
}

int us_units_fit_accumulate(const float* dense, const int64_t* labels, const float* centers, int64_t rows, int K, int D, void* state,
                            size_t state_bytes, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!shape_ok(K, D) || !rows_ok(rows)) return uf_bad("us_units_fit_accumulate", rows, K, D);
  if (!dense || !labels || !centers) return bad_arg("us_units_fit_accumulate: bad argument");
  const StateLayout sl = state_layout(K, D);
  const WorkLayout wl = work_layout(rows, K, D);
  if (!state || state_bytes < sl.total) return uf_small("us_units_fit_accumulate: state too small (us_units_fit_state_bytes)");
  if (!workspace || workspace_bytes < wl.total) return uf_small("us_units_fit_accumulate: workspace too small (us_units_fit_workspace_bytes)");
  const IndexDims dm = index_dims(rows, K);
  char* ws = static_cast<char*>(workspace);
  char* st = static_cast<char*>(state);
  int* offs = reinterpret_cast<int*>(ws + wl.offs);
  int* bsum = reinterpret_cast<int*>(ws + wl.bsum);
  int* skip = reinterpret_cast<int*>(ws + wl.skip);
  int* index = reinterpret_cast<int*>(ws + wl.index);
  int* cstart = reinterpret_cast<int*>(ws + wl.cstart);
  double* part = reinterpret_cast<double*>(ws + wl.part);
  double* pin = reinterpret_cast<double*>(ws + wl.pin);
  const long long* lab = reinterpret_cast<const long long*>(labels);
  const int n = (int)rows, ky = (K + 255) / 256, items = (int)dm.max_items;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(uf_hist_kernel, dim3(dm.nchunks, ky), dim3(256), 0, s, lab, offs, skip, n, K, dm.nchunks);
  hipLaunchKernelGGL(uf_scan_sums_kernel, dim3(dm.nscan), dim3(256), 0, s, offs, bsum, (long long)dm.m);
  hipLaunchKernelGGL(uf_scan_top_kernel, dim3(1), dim3(256), 0, s, bsum, offs, dm.nscan, (long long)dm.m);
  hipLaunchKernelGGL(uf_scan_apply_kernel, dim3(dm.nscan), dim3(256), 0, s, offs, bsum, (long long)dm.m);
  hipLaunchKernelGGL(uf_table_kernel, dim3(1), dim3(256), 0, s, offs, cstart, K, dm.nchunks);
  hipLaunchKernelGGL(uf_scatter_kernel, dim3(dm.nchunks, ky), dim3(256), 0, s, lab, offs, index, n, K, dm.nchunks);
  const dim3 gg(items), gb(256);
  switch ((D + 255) / 256) {
    case 1: hipLaunchKernelGGL((uf_gather_kernel<1, 8>), gg, gb, 0, s, dense, centers, index, offs, cstart, part, pin, K, D, dm.nchunks); break;
    case 2: hipLaunchKernelGGL((uf_gather_kernel<2, 8>), gg, gb, 0, s, dense, centers, index, offs, cstart, part, pin, K, D, dm.nchunks); break;
    case 3: hipLaunchKernelGGL((uf_gather_kernel<3, 4>), gg, gb, 0, s, dense, centers, index, offs, cstart, part, pin, K, D, dm.nchunks); break;
    default: hipLaunchKernelGGL((uf_gather_kernel<4, 4>), gg, gb, 0, s, dense, centers, index, offs, cstart, part, pin, K, D, dm.nchunks); break;
  }
  hipLaunchKernelGGL(uf_reduce_kernel, dim3(K + 1, (D + 255) / 256), dim3(256), 0, s, part, pin, offs, cstart, skip, reinterpret_cast<double*>(st + sl.sums),
                     reinterpret_cast<long long*>(st + sl.counts), reinterpret_cast<long long*>(st + sl.scalars), K, D, dm.nchunks, items);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_units_fit_accumulate", e);
}

int us_units_fit_update(int mode, const float* centers_in, float* centers_out, const int64_t* totals_in, int64_t* totals_out, int K, int D,
                        void* state, size_t state_bytes, void* record, us_stream stream) {
  if (!shape_ok(K, D)) return uf_bad("us_units_fit_update", 1, K, D);
  if (mode != US_UNITS_FIT_LLOYD && mode != US_UNITS_FIT_MINIBATCH) return bad_arg("us_units_fit_update: mode must be US_UNITS_FIT_LLOYD or US_UNITS_FIT_MINIBATCH");
  if (!centers_in || !centers_out || !record || (mode == US_UNITS_FIT_MINIBATCH && (!totals_in || !totals_out)))
    return bad_arg("us_units_fit_update: bad argument");
  const StateLayout sl = state_layout(K, D);
  if (!state || state_bytes < sl.total) return uf_small("us_units_fit_update: state too small (us_units_fit_state_bytes)");
  char* st = static_cast<char*>(state);
  const int mb = mode == US_UNITS_FIT_MINIBATCH;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(uf_update_kernel, dim3(K), dim3(256), 0, s, centers_in, centers_out, reinterpret_cast<const long long*>(totals_in),
                     reinterpret_cast<double*>(st + sl.sums), reinterpret_cast<const long long*>(st + sl.counts),
                     reinterpret_cast<double*>(st + sl.shift), D, mb);
  hipLaunchKernelGGL(uf_record_kernel, dim3(1), dim3(256), 0, s, reinterpret_cast<const long long*>(totals_in),
                     reinterpret_cast<long long*>(totals_out), reinterpret_cast<long long*>(st + sl.counts),
                     reinterpret_cast<const double*>(st + sl.shift), reinterpret_cast<long long*>(st + sl.scalars),
                     reinterpret_cast<long long*>(record), K, mb);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_units_fit_update", e);
}

int us_units_fit_seed_step(const float* dense, const int64_t* lengths, int B, int Tmax, int K, int D, int step, double u, double* mind,
                           float* centers, int64_t* picked, void* workspace, size_t workspace_bytes, us_stream stream) {
  const int64_t rows = (int64_t)B * Tmax;
  if (!shape_ok(K, D) || B < 1 || Tmax < 1 || !rows_ok(rows)) return uf_bad("us_units_fit_seed_step", rows, K, D);
  if (!dense || !lengths || !mind || !centers || !picked || step < 0 || step >= K || !(u >= 0.0 && u < 1.0))
    return bad_arg("us_units_fit_seed_step: bad argument (step in [0, K), u in [0, 1))");
  const WorkLayout wl = work_layout(rows, K, D);
  if (!workspace || workspace_bytes < wl.total) return uf_small("us_units_fit_seed_step: workspace too small (us_units_fit_workspace_bytes)");
  char* ws = static_cast<char*>(workspace);
  double* bsum = reinterpret_cast<double*>(ws + wl.seed_sum);
  int* bcnt = reinterpret_cast<int*>(ws + wl.seed_cnt);
  SeedSel* sel = reinterpret_cast<SeedSel*>(ws + wl.seed_sel);
  const int n = (int)rows, nb = (int)ceil_div(rows, kSeedBlock), first = step == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(uf_seed_dist_kernel, dim3((n + 127) / 128), dim3(128), 0, s, dense, reinterpret_cast<const long long*>(lengths),
                     first ? nullptr : centers, step - 1, mind, n, Tmax, D);
  hipLaunchKernelGGL(uf_seed_bsum_kernel, dim3(nb), dim3(256), 0, s, mind, bsum, bcnt, n, first);
  hipLaunchKernelGGL(uf_seed_block_kernel, dim3(1), dim3(256), 0, s, bsum, bcnt, sel, nb, first, u);
  hipLaunchKernelGGL(uf_seed_row_kernel, dim3(1), dim3(256), 0, s, dense, mind, sel, centers, reinterpret_cast<long long*>(picked), n, D, step);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_units_fit_seed_step", e);
}

}  // extern "C"
