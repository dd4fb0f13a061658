// Fitting a CTC head on frozen encoder features, and the alignment that goes with it: the CTC loss with its gradient, the head's backward
// pass and a forced alignment, as handle-free calls that allocate nothing and only enqueue on the stream.  Scratch comes from the caller,
// sized by the *_workspace_bytes host functions.  ctc.hip (the forward head, the greedy collapse, the edit distance) is untouched.
//
//   us_ctc_loss            One wave per row takes the row's maximum and log-sum-exp (ctc_rows_kernel's scheme) into the workspace; an
//                          emission is then (x - max) - logsumexp, never stored.  One workgroup of 256 threads per item walks the extended
//                          label sequence of S = 2 L + 1 states, thread i owning states i, i + 256, ...  (at most 9: L <= 1024).  alpha is kept
//                          in log space as fp64 registers; only the exp / log of each step run in fp32, on differences from the step's
//                          maximum, so a step's error does not grow with |alpha|.  Neighbouring states are exchanged through two LDS
//                          buffers with one barrier per frame, and the next frame's emissions are loaded a frame ahead.  alpha goes to the
//                          workspace; the beta sweep runs backwards, forms the occupancies as it goes and hands them, one frame late,
//                          to the threads that own a vocabulary entry: grad = grad_out * (softmax - occupancy).
//                          The occupancy of an entry that occurs several times in the target is added along a chain of the occurrences
//                          in ascending position; the blank's is each thread's own states in ascending order, a fixed butterfly over
//                          the wave, then the four waves in order.  No float atomics, nothing depends on the batch.
//                          `stage` lets a training step run the two sweeps as two calls around the moment it learns grad_out
//                          (US_CTC_FORWARD leaves alpha and the log-likelihoods in the workspace, US_CTC_BACKWARD resumes from them).
//   us_ctc_head_backward   dW = g^T x and dX = g W on the fp32 matrix cores (the tile loop of dense_tile.h), db in plain fp32.  The rows are cut
//                          into chunks whose partial dW / db go to the workspace; a second kernel adds them in chunk order.
//   us_ctc_forced_align    Viterbi over the same states in fp32 (best predecessor + score, so the path's own sum in frame order has the
//                          same bits), a 2-bit back-pointer per (t, s) packed per thread into one word per frame, then one thread of
//                          the first wave walks back through the words, staged 16 frames at a time in LDS by the whole workgroup.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>

#include "../../include/unitspeech_hip.h"
#include "ctc_limits.h"
#include "dense_tile.h"
#include "handle.h"
#include "item_lens.h"
#include "kernels.h"

namespace us {
namespace {

constexpr int kMaxL = 1024;                     // tokens per target
constexpr int kNT = 256;                         // threads per item
constexpr int kMaxS = 2 * kMaxL + 1;
constexpr int kNJ = (kMaxS + kNT - 1) / kNT;     // states per thread: 9
constexpr int kNV = kMaxV / kNT;                 // vocabulary entries per thread: 8
constexpr int kWalk = 16;                        // frames of back-pointers staged per step of the backtrace

// ---- row statistics ---------------------------------------------------------------------------------------------------------------
// stat[row] = (max, log sum exp(x - max)); rows at or beyond the item's frames are not written and never read.
__global__ __launch_bounds__(256) void ctc_rowstat_kernel(const float* __restrict__ logits, const long long* __restrict__ lengths,
                                                          float2* __restrict__ stat, int rows, int Tmax, int V) {
  const int lane = threadIdx.x & 63;
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int b = row / Tmax;
  if (row - b * Tmax >= item_len(lengths, b, Tmax)) return;
  const float* __restrict__ x = logits + (size_t)row * V;
  float xv[kMaxV / 64];
  float best = -INFINITY;
#pragma unroll
  for (int j = 0; j < kMaxV / 64; ++j) {
    const int v = lane + 64 * j;
    xv[j] = v < V ? x[v] : -INFINITY;
    best = fmaxf(best, xv[j]);
  }
  best = wave_max(best);
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < kMaxV / 64; ++j)
    if (lane + 64 * j < V) s += expf(xv[j] - best);
  s = wave_sum(s);
  if (lane == 0) stat[row] = make_float2(best, logf(s));
}

// log(exp(p0) + exp(p1) + exp(p2)) with the fp64 maximum taken out first: the fp32 part sees differences only
__device__ __forceinline__ double lse3(double p0, double p1, double p2) {
  const double mx = fmax(p0, fmax(p1, p2));
  if (mx == -INFINITY) return mx;
  const float s = (expf((float)(p0 - mx)) + expf((float)(p1 - mx))) + expf((float)(p2 - mx));
  return mx + (double)logf(s);
}

// What a thread knows of its states: the vocabulary entry each emits and whether the skip transitions into it (from s - 2) and out of it
// (to s + 2) exist.  `bad` comes back set when a target lies outside [0, V) or is the blank.
struct States {
  int lab[kNJ];
  unsigned skip_in, skip_out;
};
__device__ __forceinline__ bool load_states(States& st, const long long* __restrict__ tg, int L, int S, int V, int blank, int tid) {
  bool bad = false;
  st.skip_in = st.skip_out = 0;
#pragma unroll
  for (int j = 0; j < kNJ; ++j) {
    const int s = tid + kNT * j;
    st.lab[j] = blank;
    if (s < S && (s & 1)) {
      const int i = s >> 1;
      const long long v = tg[i];
      if (v < 0 || v >= V || v == blank) {
        bad = true;
      } else {
        st.lab[j] = (int)v;
        if (i > 0 && tg[i - 1] != v) st.skip_in |= 1u << j;
        if (i + 1 < L && tg[i + 1] != v) st.skip_out |= 1u << j;
      }
    }
  }
  return bad;
}

// One workgroup per item.  ws_alpha: [B][Tmax][2 Lmax + 1] fp64 and ws_ll: [B] fp64 (the log-likelihood; -inf without a path).
// ALPHA: the forward sweep runs (else ws_ll and ws_alpha hold an earlier call's); STORE: it writes them; GRAD: the backward sweep runs.
template <bool ALPHA, bool STORE, bool GRAD>
__global__ __launch_bounds__(kNT) void ctc_loss_kernel(const float* __restrict__ logits, const float2* __restrict__ stat,
                                                       const long long* __restrict__ frame_lengths, const long long* __restrict__ targets,
                                                       const long long* __restrict__ target_lengths, const float* __restrict__ grad_out,
                                                       float* __restrict__ loss, float* __restrict__ grad, double* __restrict__ ws_alpha,
                                                       double* __restrict__ ws_ll, int Tmax, int V, int Lmax, int blank, int zero_infinity) {
  static_assert(ALPHA || GRAD, "nothing to do");
  static_assert(!GRAD || STORE || !ALPHA, "the backward sweep reads the stored alpha");
  // state s lives at index s + 2: [0], [1] and everything from S + 2 on stay -inf (the neighbours of the first and last states)
  __shared__ double ex[2][kMaxS + 4];
  __shared__ float occ_lab[GRAD ? 2 : 1][GRAD ? kMaxL : 1];     // per target position: the occupancy of its state
  __shared__ float occ_blank[2][4];                             // per wave: the occupancy of its blank states
  __shared__ int nxt[GRAD ? kMaxL : 1];                         // the next position with the same entry, or -1
  __shared__ int head[GRAD ? kMaxV : 1];                        // the first position of an entry, or -1
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = item_len(frame_lengths, b, Tmax), L = item_len(target_lengths, b, Lmax), S = 2 * L + 1;
  const int Smax = 2 * Lmax + 1;
  const long long* __restrict__ tg = targets + (size_t)b * Lmax;
  const float* __restrict__ x = logits + (size_t)b * Tmax * V;
  const float2* __restrict__ rs = stat + (size_t)b * Tmax;
  float* __restrict__ g = GRAD ? grad + (size_t)b * Tmax * V : nullptr;
  double* __restrict__ wa = (STORE || GRAD) ? ws_alpha + (size_t)b * Tmax * Smax : nullptr;

  States st;
  const bool bad = __syncthreads_or(load_states(st, tg, L, S, V, blank, tid) ? 1 : 0) != 0;
  for (int i = tid; i < 2 * (kMaxS + 4); i += kNT) (&ex[0][0])[i] = -INFINITY;
  __syncthreads();

  // ---- alpha ----
  double a[kNJ] = {};
  float xn[kNJ] = {};             // raw logits of the coming frame at this thread's entries, and that frame's statistics
  float2 sn = make_float2(0.f, 0.f);
  auto fetch = [&](int t) {
    sn = rs[t];
#pragma unroll
    for (int j = 0; j < kNJ; ++j)
      if (tid + kNT * j < S) xn[j] = x[(size_t)t * V + st.lab[j]];
  };
  double ll = -INFINITY;
  if (!ALPHA) {
    ll = ws_ll[b];
  } else if (!bad && T > 0) {
    fetch(0);
    for (int t = 0; t < T; ++t) {
      const int cur = t & 1, prev = cur ^ 1;
      float e[kNJ];
#pragma unroll
      for (int j = 0; j < kNJ; ++j) e[j] = (xn[j] - sn.x) - sn.y;
      if (t + 1 < T) fetch(t + 1);
#pragma unroll
      for (int j = 0; j < kNJ; ++j) {
        const int s = tid + kNT * j;
        if (s < S) {
          if (t == 0) {
            a[j] = s < 2 ? (double)e[j] : -INFINITY;
          } else {
            const double p1 = ex[prev][s + 1], p2 = (st.skip_in >> j & 1) ? ex[prev][s] : -INFINITY;
            a[j] = lse3(a[j], p1, p2) + (double)e[j];
          }
          ex[cur][s + 2] = a[j];
          if (STORE) wa[(size_t)t * Smax + s] = a[j];
        }
      }
      __syncthreads();
    }
    const int last = (T - 1) & 1;
    ll = lse3(ex[last][S - 1 + 2], S > 1 ? ex[last][S - 2 + 2] : -INFINITY, -INFINITY);
  } else if (!bad && L == 0) {
    ll = 0.0;                     // no frame, no token: the empty path
  }
  const bool feasible = ll != -INFINITY;
  if (tid == 0) {
    loss[b] = bad ? NAN : (feasible ? (float)-ll : (zero_infinity ? 0.f : INFINITY));
    if (ALPHA && STORE) ws_ll[b] = ll;
  }
  if (!GRAD) return;

  // ---- rows without a gradient ----
  const int live = (feasible && !bad) ? T : 0;
  for (size_t i = (size_t)live * V + tid; i < (size_t)Tmax * V; i += kNT) g[i] = 0.f;
  if (live == 0) return;

  // ---- the chains of equal entries (once per item) ----
  for (int v = tid; v < V; v += kNT) head[v] = -1;
  __syncthreads();
  for (int i = tid; i < L; i += kNT) {
    const long long v = tg[i];
    int n = -1;
    for (int k = i + 1; k < L; ++k)
      if (tg[k] == v) {
        n = k;
        break;
      }
    nxt[i] = n;
    bool first = true;
    for (int k = i - 1; k >= 0; --k)
      if (tg[k] == v) {
        first = false;
        break;
      }
    if (first) head[(int)v] = i;
  }
  __syncthreads();              // also: every read of ex[] by the alpha sweep is done

  // ---- beta, occupancy, gradient ----
  const float go = grad_out ? grad_out[b] : 1.f;
  const int wave = tid >> 6;
  double an[kNJ] = {};            // alpha of the coming frame
  float xr[kNV] = {};             // the coming frame's logits at the entries this thread writes
  auto fetch_b = [&](int t) {
    fetch(t);
#pragma unroll
    for (int j = 0; j < kNJ; ++j)
      if (tid + kNT * j < S) an[j] = wa[(size_t)t * Smax + tid + kNT * j];
#pragma unroll
    for (int j = 0; j < kNV; ++j)
      if (tid + kNT * j < V) xr[j] = x[(size_t)t * V + tid + kNT * j];
  };
  // frame t's gradient row from the occupancies in buffer `buf`
  auto emit_row = [&](int t, int buf, const float* xrow, float2 srow) {
#pragma unroll
    for (int j = 0; j < kNV; ++j) {
      const int v = tid + kNT * j;
      if (v < V) {
        float occ = 0.f;
        if (v == blank) {
          occ = ((occ_blank[buf][0] + occ_blank[buf][1]) + occ_blank[buf][2]) + occ_blank[buf][3];
        } else {
          for (int i = head[v]; i >= 0; i = nxt[i]) occ += occ_lab[buf][i];
        }
        g[(size_t)t * V + v] = go * (expf((xrow[j] - srow.x) - srow.y) - occ);
      }
    }
  };
  double bt[kNJ] = {};
  float xc[kNV] = {};
  float2 sc = make_float2(0.f, 0.f);
  fetch_b(T - 1);
  for (int t = T - 1; t >= 0; --t) {
    const int cur = t & 1, prev = cur ^ 1;
    float e[kNJ], xp[kNV];
    double al[kNJ];
    const float2 sp = sc;                                   // frame t + 1, whose row is written in this step
#pragma unroll
    for (int j = 0; j < kNV; ++j) xp[j] = xc[j];
    sc = sn;
#pragma unroll
    for (int j = 0; j < kNV; ++j) xc[j] = xr[j];
#pragma unroll
    for (int j = 0; j < kNJ; ++j) {
      e[j] = (xn[j] - sn.x) - sn.y;
      al[j] = an[j];
    }
    if (t > 0) fetch_b(t - 1);
    float blank_part = 0.f;
#pragma unroll
    for (int j = 0; j < kNJ; ++j) {
      const int s = tid + kNT * j;
      if (s < S) {
        if (t == T - 1) {
          bt[j] = s >= S - 2 ? (double)e[j] : -INFINITY;
        } else {
          const double p1 = ex[prev][s + 3], p2 = (st.skip_out >> j & 1) ? ex[prev][s + 4] : -INFINITY;
          bt[j] = lse3(bt[j], p1, p2) + (double)e[j];
        }
        ex[cur][s + 2] = bt[j];
        const float occ = (al[j] == -INFINITY || bt[j] == -INFINITY) ? 0.f : expf((float)(((al[j] + bt[j]) - (double)e[j]) - ll));
        if (s & 1)
          occ_lab[cur][s >> 1] = occ;
        else
          blank_part += occ;
      }
    }
    blank_part = wave_sum(blank_part);
    if ((tid & 63) == 0) occ_blank[cur][wave] = blank_part;
    if (t + 1 < T) emit_row(t + 1, prev, xp, sp);
    __syncthreads();
  }
  emit_row(0, 0, xc, sc);
}

// ---- forced alignment ---------------------------------------------------------------------------------------------------------------
// ws_bp: [B][Tmax][W] words, W = align_words(Lmax); word (t, i) holds the back-pointers of thread i's states at frame t, 2 bits each.
__host__ __device__ constexpr int align_words(int Lmax) { return (2 * Lmax + 1 >= kNT) ? kNT : (2 * Lmax + 1 + 63) / 64 * 64; }

__global__ __launch_bounds__(kNT) void ctc_align_kernel(const float* __restrict__ scores, const long long* __restrict__ frame_lengths,
                                                        const long long* __restrict__ targets, const long long* __restrict__ target_lengths,
                                                        long long* __restrict__ path, float* __restrict__ score, long long* __restrict__ start,
                                                        long long* __restrict__ frames, unsigned* __restrict__ ws_bp, int Tmax, int V, int Lmax,
                                                        int blank) {
  __shared__ float ex[2][kMaxS + 2];           // state s at index s + 2
  __shared__ unsigned bp[kWalk * kNT];
  __shared__ int tgs[kMaxL], first[kMaxL], count[kMaxL];
  const int b = blockIdx.x, tid = threadIdx.x;
  const int T = item_len(frame_lengths, b, Tmax), L = item_len(target_lengths, b, Lmax), S = 2 * L + 1;
  const int W = align_words(Lmax);
  const long long* __restrict__ tg = targets + (size_t)b * Lmax;
  const float* __restrict__ x = scores + (size_t)b * Tmax * V;
  unsigned* __restrict__ wb = ws_bp + (size_t)b * Tmax * W;
  long long* __restrict__ pth = path + (size_t)b * Tmax;

  States st;
  const bool bad = __syncthreads_or(load_states(st, tg, L, S, V, blank, tid) ? 1 : 0) != 0;
  for (int i = tid; i < 2 * (kMaxS + 2); i += kNT) (&ex[0][0])[i] = -INFINITY;
  for (int i = tid; i < L; i += kNT) {
    tgs[i] = bad ? 0 : (int)tg[i];
    first[i] = 0;
    count[i] = 0;
  }
  __syncthreads();

  float d[kNJ] = {}, xn[kNJ] = {};
  auto fetch = [&](int t) {
#pragma unroll
    for (int j = 0; j < kNJ; ++j)
      if (tid + kNT * j < S) xn[j] = x[(size_t)t * V + st.lab[j]];
  };
  float best = -INFINITY;
  int send = 0;
  if (!bad && T > 0) {
    fetch(0);
    for (int t = 0; t < T; ++t) {
      const int cur = t & 1, prev = cur ^ 1;
      float e[kNJ];
#pragma unroll
      for (int j = 0; j < kNJ; ++j) e[j] = xn[j];
      if (t + 1 < T) fetch(t + 1);
      unsigned word = 0;
#pragma unroll
      for (int j = 0; j < kNJ; ++j) {
        const int s = tid + kNT * j;
        if (s < S) {
          if (t == 0) {
            d[j] = s < 2 ? e[j] : -INFINITY;
          } else {
            const float p1 = ex[prev][s + 1], p2 = (st.skip_in >> j & 1) ? ex[prev][s] : -INFINITY;
            float m = d[j];                    // staying wins over s - 1, s - 1 over s - 2
            unsigned k = 0;
            if (p1 > m) {
              m = p1;
              k = 1;
            }
            if (p2 > m) {
              m = p2;
              k = 2;
            }
            d[j] = m + e[j];
            word |= k << (2 * j);
          }
          ex[cur][s + 2] = d[j];
        }
      }
      if (tid < W) wb[(size_t)t * W + tid] = word;
      __syncthreads();
    }
    const int last = (T - 1) & 1;
    const float eb = ex[last][S - 1 + 2], el = S > 1 ? ex[last][S - 2 + 2] : -INFINITY;
    if (eb > el) {                             // the last label wins over the final blank
      best = eb;
      send = S - 1;
    } else {
      best = el;
      send = S - 2;
    }
  } else if (!bad && L == 0) {
    best = 0.f;
  }
  const bool feasible = best != -INFINITY;
  if (tid == 0) score[b] = bad ? NAN : best;
  const int live = (feasible && !bad) ? T : 0;
  for (int t = live + tid; t < Tmax; t += kNT) pth[t] = -1;

  // ---- backtrace: the words of kWalk frames at a time into LDS, then thread 0 walks them ----
  int s = send;
  for (int hi = live; hi > 0; hi -= kWalk) {
    const int lo = max(0, hi - kWalk);
    __syncthreads();                           // the stores of the sweep are visible; the stage of the step before is no longer read
    for (int i = tid; i < (hi - lo) * W; i += kNT) bp[i] = wb[(size_t)lo * W + i];
    __syncthreads();
    if (tid == 0) {
      for (int t = hi - 1; t >= lo; --t) {
        if (s & 1) {
          pth[t] = tgs[s >> 1];
          first[s >> 1] = t;
          ++count[s >> 1];
        } else {
          pth[t] = blank;
        }
        s -= (int)(bp[(t - lo) * W + (s & (kNT - 1))] >> (2 * (s >> 8)) & 3u);   // frame 0's word is 0
      }
    }
  }
  __syncthreads();
  for (int i = tid; i < Lmax; i += kNT) {
    start[(size_t)b * Lmax + i] = i < L && live ? first[i] : 0;
    frames[(size_t)b * Lmax + i] = i < L && live ? count[i] : 0;
  }
}

// ---- the head's backward pass ---------------------------------------------------------------------------------------------------------
// part_w[chunk][V][H] = sum over the chunk's live rows of g[row][v] x[row][h] (the MFMA's M is the vocabulary, its N the hidden index: the
// lanes store along h); part_b[chunk][V] = the column sums of g, added in row order by the workgroups of the first h tile.
__global__ __launch_bounds__(256) void ctc_head_dw_kernel(const float* __restrict__ g, const float* __restrict__ x,
                                                          const long long* __restrict__ lengths, float* __restrict__ part_w,
                                                          float* __restrict__ part_b, int rows, int Tmax, int V, int H, int chunk) {
  __shared__ float Gs[2][kDtBK][kDtTile];
  __shared__ float Xs[2][kDtBK][kDtTile];
  const int tid = threadIdx.x;
  DENSE_LANE(tid);
  DENSE_STAGE_K(tid);                                    // both slices: 16 rows x 64 columns, four neighbouring columns per thread
  const int hh = wave & 1, vh = wave >> 1;
  const int r0 = blockIdx.x * chunk, r1 = min(rows, r0 + chunk);
  const int c0 = blockIdx.y * kDtTile, h0 = blockIdx.z * kDtTile;
  float greg[4];
  float4 xreg;
  auto load = [&](int k0) {
    const int row = r0 + k0 + sk;
    const bool live = row < r1 && row_live(lengths, row, rows, Tmax);   // a dead row's features may hold anything: they are not read
#pragma unroll
    for (int i = 0; i < 4; ++i) greg[i] = (live && c0 + sc + i < V) ? g[(size_t)row * V + c0 + sc + i] : 0.f;   // V need not be a multiple of 4
    xreg = (live && h0 + sc < H) ? *reinterpret_cast<const float4*>(x + (size_t)row * H + h0 + sc) : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) Gs[buf][sk][sc + i] = greg[i];
    *reinterpret_cast<float4*>(&Xs[buf][sk][sc]) = xreg;
  };
  f32x16 acc[2];
  float bsum = 0.f;
  dense_tile_mainloop(Gs, Xs, vh, hh, (r1 - r0 + kDtBK - 1) / kDtBK, acc, load, store, DenseNoHook{}, [&](int cur) {
    if (blockIdx.z == 0 && tid < kDtTile) {
#pragma unroll
      for (int k = 0; k < kDtBK; ++k) bsum += Gs[cur][k][tid];
    }
  });
  if (blockIdx.z == 0 && tid < kDtTile && c0 + tid < V) part_b[(size_t)blockIdx.x * V + c0 + tid] = bsum;
  const int h = h0 + DENSE_AT(hh);
  if (h >= H) return;
  float* __restrict__ pw = part_w + (size_t)blockIdx.x * V * H;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int v = c0 + DENSE_ROW(vh, r);
    if (v < V) pw[(size_t)v * H + h] = acc[0][r] + acc[1][r];
  }
}

// dst[i] = part[0][i] + part[1][i] + ... in chunk order, for dW (n = V H) followed by db (n = V)
__global__ __launch_bounds__(256) void ctc_head_sum_kernel(const float* __restrict__ part_w, const float* __restrict__ part_b,
                                                           float* __restrict__ dw, float* __restrict__ db, size_t nw, int nb, int nchunks) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= nw + nb) return;
  const bool isw = i < nw;
  const float* __restrict__ p = isw ? part_w + i : part_b + (i - nw);
  const size_t stride = isw ? nw : (size_t)nb;
  float s = 0.f;
  for (int c = 0; c < nchunks; ++c) s += p[(size_t)c * stride];
  if (isw)
    dw[i] = s;
  else
    db[i - nw] = s;
}

// dX[row][h] = sum over v of g[row][v] W[v][h]: the rows are the MFMA's M (a row-major operand of dense_tile.h, transposed into LDS
// on the way in), h its N.  A row at or beyond its item's frames gets 0.
__global__ __launch_bounds__(256) void ctc_head_dx_kernel(const float* __restrict__ g, const float* __restrict__ w,
                                                          const long long* __restrict__ lengths, float* __restrict__ dx, int rows, int Tmax,
                                                          int V, int H) {
  __shared__ float Ws[2][kDtBK][kDtTile];
  __shared__ float Gt[2][kDtBK][kDtLdT];
  const int tid = threadIdx.x;
  DENSE_LANE(tid);
  DENSE_STAGE_K(tid);                                    // weight slice: 16 entries x 64 hidden, one float4 per thread
  DENSE_STAGE_T(tid);                                    // gradient slice: 64 rows x 16 entries, four neighbouring entries per thread
  const int hh = wave & 1, rh = wave >> 1;
  const int r0 = blockIdx.x * kDtTile, h0 = blockIdx.y * kDtTile;
  const bool glive = row_live(lengths, r0 + tr, rows, Tmax);
  const float* __restrict__ grow = g + (size_t)(glive ? r0 + tr : 0) * V;
  float4 wreg;
  float greg[4];
  auto load = [&](int k0) {
    wreg = (k0 + sk < V && h0 + sc < H) ? *reinterpret_cast<const float4*>(w + (size_t)(k0 + sk) * H + h0 + sc) : make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
    for (int i = 0; i < 4; ++i) greg[i] = (glive && k0 + tk + i < V) ? grow[k0 + tk + i] : 0.f;   // V need not be a multiple of 4
  };
  auto store = [&](int buf) {
    *reinterpret_cast<float4*>(&Ws[buf][sk][sc]) = wreg;
#pragma unroll
    for (int i = 0; i < 4; ++i) Gt[buf][tk + i][tr] = greg[i];
  };
  f32x16 acc[2];
  dense_tile_mainloop(Gt, Ws, rh, hh, (V + kDtBK - 1) / kDtBK, acc, load, store);
  const int h = h0 + DENSE_AT(hh);
  if (h >= H) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int row = r0 + DENSE_ROW(rh, r);
    if (row < rows) dx[(size_t)row * H + h] = acc[0][r] + acc[1][r];       // a dead row's operand was all zeros
  }
}

// "" or why the sizes of a loss / alignment call are refused
const char* seq_error(int B, int Tmax, int V, int Lmax, long long blank, char* buf, size_t n, const char* what) {
  if (Lmax < 0 || Lmax > kMaxL) {
    snprintf(buf, n, "%s: a target holds at most %d tokens (Lmax = %d)", what, kMaxL, Lmax);
    return buf;
  }
  if (V < 2 || V > kMaxV) {
    snprintf(buf, n, "%s: V must be in [2, %d] (V = %d)", what, kMaxV, V);
    return buf;
  }
  if (blank < 0 || blank >= V) {
    snprintf(buf, n, "%s: the blank %lld is not in [0, %d)", what, blank, V);
    return buf;
  }
  if (!rows_ok(B, Tmax)) {
    snprintf(buf, n, "%s: B must be in [1, 65535] and B * Tmax in [1, 2^24] (B = %d, Tmax = %d)", what, B, Tmax);
    return buf;
  }
  return nullptr;
}
size_t align256(size_t n) { return (n + 255) / 256 * 256; }
size_t stat_bytes(int B, int Tmax) { return align256((size_t)B * Tmax * sizeof(float2)); }
size_t ll_bytes(int B) { return align256((size_t)B * sizeof(double)); }
int head_chunk(int rows) { return std::max(kDtTile, round_up((rows + 63) / 64, kDtBK)); }     // at most 64 chunks

}  // namespace
}  // namespace us

using namespace us;

extern "C" {

size_t us_ctc_loss_workspace_bytes(int B, int Tmax, int Lmax, int with_grad) {
  if (!rows_ok(B, Tmax) || Lmax < 0 || Lmax > kMaxL) return 0;
  return stat_bytes(B, Tmax) + ll_bytes(B) + (with_grad ? (size_t)B * Tmax * (2 * Lmax + 1) * sizeof(double) : 0);
}

int us_ctc_loss(const float* logits, const int64_t* frame_lengths, const int64_t* targets, const int64_t* target_lengths, const float* grad_out,
                int B, int Tmax, int V, int Lmax, int64_t blank, int zero_infinity, int stage, float* loss, float* grad_logits, void* workspace,
                size_t workspace_bytes, us_stream stream) {
  char buf[192];
  if (const char* m = seq_error(B, Tmax, V, Lmax, blank, buf, sizeof buf, "us_ctc_loss")) return bad_arg(m);
  if (stage < US_CTC_WHOLE || stage > US_CTC_BACKWARD || (stage == US_CTC_FORWARD && grad_logits) || (stage == US_CTC_BACKWARD && !grad_logits))
    return bad_arg("us_ctc_loss: stage must be US_CTC_WHOLE, US_CTC_FORWARD (without grad_logits) or US_CTC_BACKWARD (with grad_logits)");
  if (!logits || !target_lengths || !loss || (Lmax > 0 && !targets) || !workspace ||
      workspace_bytes < us_ctc_loss_workspace_bytes(B, Tmax, Lmax, grad_logits != nullptr || stage != US_CTC_WHOLE))
    return bad_arg("us_ctc_loss: bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rows = B * Tmax;
  float2* stat = static_cast<float2*>(workspace);
  double* ll = reinterpret_cast<double*>(static_cast<char*>(workspace) + stat_bytes(B, Tmax));
  double* alpha = reinterpret_cast<double*>(static_cast<char*>(workspace) + stat_bytes(B, Tmax) + ll_bytes(B));
  const long long* fl = reinterpret_cast<const long long*>(frame_lengths);
  const long long* tg = reinterpret_cast<const long long*>(targets);
  const long long* tl = reinterpret_cast<const long long*>(target_lengths);
  if (stage != US_CTC_BACKWARD)           // the statistics of an earlier US_CTC_FORWARD are still there
    hipLaunchKernelGGL(ctc_rowstat_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, fl, stat, rows, Tmax, V);
  auto launch = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(B), dim3(kNT), 0, s, logits, stat, fl, tg, tl, grad_out, loss, grad_logits, alpha, ll, Tmax, V, Lmax,
                       (int)blank, zero_infinity);
  };
  if (stage == US_CTC_BACKWARD)
    launch(ctc_loss_kernel<false, false, true>);
  else if (stage == US_CTC_FORWARD)
    launch(ctc_loss_kernel<true, true, false>);
  else if (grad_logits)
    launch(ctc_loss_kernel<true, true, true>);
  else
    launch(ctc_loss_kernel<true, false, false>);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_ctc_loss", e);
}

size_t us_ctc_align_workspace_bytes(int B, int Tmax, int Lmax) {
  if (!rows_ok(B, Tmax) || Lmax < 0 || Lmax > kMaxL) return 0;
  return (size_t)B * Tmax * align_words(Lmax) * sizeof(unsigned);
}

int us_ctc_forced_align(const float* scores, const int64_t* frame_lengths, const int64_t* targets, const int64_t* target_lengths, int B, int Tmax,
                        int V, int Lmax, int64_t blank, int64_t* path, float* score, int64_t* start, int64_t* frames, void* workspace,
                        size_t workspace_bytes, us_stream stream) {
  char buf[192];
  if (const char* m = seq_error(B, Tmax, V, Lmax, blank, buf, sizeof buf, "us_ctc_forced_align")) return bad_arg(m);
  if (!scores || !target_lengths || !path || !score || (Lmax > 0 && (!targets || !start || !frames)) || !workspace ||
      workspace_bytes < us_ctc_align_workspace_bytes(B, Tmax, Lmax))
    return bad_arg("us_ctc_forced_align: bad argument");
  hipLaunchKernelGGL(ctc_align_kernel, dim3(B), dim3(kNT), 0, static_cast<hipStream_t>(stream), scores,
                     reinterpret_cast<const long long*>(frame_lengths), reinterpret_cast<const long long*>(targets),
                     reinterpret_cast<const long long*>(target_lengths), reinterpret_cast<long long*>(path), score,
                     reinterpret_cast<long long*>(start), reinterpret_cast<long long*>(frames), static_cast<unsigned*>(workspace), Tmax, V,
                     Lmax, (int)blank);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_ctc_forced_align", e);
}

size_t us_ctc_head_backward_workspace_bytes(int B, int Tmax, int V, int H) {
  if (!rows_ok(B, Tmax) || head_error(V, H)) return 0;
  const int rows = B * Tmax, chunk = head_chunk(rows), nchunks = (rows + chunk - 1) / chunk;
  return (size_t)nchunks * ((size_t)V * H + V) * sizeof(float);
}

int us_ctc_head_backward(const float* grad_logits, const float* hidden, const int64_t* lengths, const float* weight, int B, int Tmax, int V,
                         int H, float* d_weight, float* d_bias, float* d_hidden, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (head_error(V, H)) {
    char buf[160];
    snprintf(buf, sizeof buf, "us_ctc_head_backward: V must be in [2, %d] and H a multiple of 4 in [4, %d] (V = %d, H = %d)", kMaxV, kMaxH, V, H);
    return bad_arg(buf);
  }
  if (!grad_logits || !hidden || !d_weight || !d_bias || (d_hidden && !weight) || !rows_ok(B, Tmax) || !workspace ||
      workspace_bytes < us_ctc_head_backward_workspace_bytes(B, Tmax, V, H))
    return bad_arg("us_ctc_head_backward: bad argument");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rows = B * Tmax, chunk = head_chunk(rows), nchunks = (rows + chunk - 1) / chunk;
  const int vt = (V + kDtTile - 1) / kDtTile, ht = (H + kDtTile - 1) / kDtTile;
  const long long* lens = reinterpret_cast<const long long*>(lengths);
  float* part_w = static_cast<float*>(workspace);
  float* part_b = part_w + (size_t)nchunks * V * H;
  hipLaunchKernelGGL(ctc_head_dw_kernel, dim3(nchunks, vt, ht), dim3(256), 0, s, grad_logits, hidden, lens, part_w, part_b, rows, Tmax, V, H,
                     chunk);
  const size_t nw = (size_t)V * H;
  hipLaunchKernelGGL(ctc_head_sum_kernel, dim3((unsigned)((nw + V + 255) / 256)), dim3(256), 0, s, part_w, part_b, d_weight, d_bias, nw, V,
                     nchunks);
  if (d_hidden)
    hipLaunchKernelGGL(ctc_head_dx_kernel, dim3((rows + kDtTile - 1) / kDtTile, ht), dim3(256), 0, s, grad_logits, weight, lens, d_hidden, rows, Tmax,
                       V, H);
  hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : hip_fail("us_ctc_head_backward", e);
}

}  // extern "C"
