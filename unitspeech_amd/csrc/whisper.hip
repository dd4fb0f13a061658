// Whisper (transformers.WhisperForConditionalGeneration, eval mode): log-mel features [B][n_mels][2 S] -> encoder -> greedy decoder -> token
// ids.  fp32 storage and exact-fp32 products (v_mfma_f32_16x16x4_f32 in the decoder's GEMMs) throughout.
//
// The encoder and the cross-attention keys / values run on hubert.hip's kernels (whisper_encoder.h).  This file is the decoder step: up to
// kWhItems items of one launch group advance by one position per step, one row each.
//  - wh_embed_kernel: x[m] = embed_tokens[token] + embed_positions[pos]; the token is the host's (prompt, teacher forcing) or the one the
//    last wh_argmax_kernel chose.
//  - wh_gemm_kernel: the skinny GEMM y[m][n] = post(sum_k pre(x)[m][k] W[n][k]) for M <= 16 rows, the rows padded to the 16 columns of the
//    MFMA with zeros.  A workgroup is 16 outputs n; its four waves take the k range in interleaved slices of 16 and their partial sums meet in
//    LDS in wave order, so the weights are read once and an element's summation order depends on K alone, not on M or on the row's place.
//    pre: LayerNorm of the row (two-pass, fixed order, recomputed per workgroup: K floats per row).  post: + bias, * scale, GELU, + residual.
//    Up to three weight matrices share one launch (q | k | v: blockIdx.y), each with its own output: k and v go straight into the self cache.
//  - wh_self_attn_kernel: one query of an (item, head) over the item's self cache [layer][item][2][max_target_positions][d_model], one wave.
//  - wh_cross_attn_kernel: one query over the item's planar cross keys / values [layer][item][2 d_model][S], sixteen waves.
//  - wh_argmax_kernel: the suppression masks, then (value, index) argmax per item with the lower index on exact ties (torch.argmax), the end of
//    an item (eos) and the count of items still running.
//  - wh_select_partial_kernel + wh_select_close_kernel: the selection stage of us_whisper_decode and us_whisper_select.  SuppressTokens,
//    begin-suppress, the timestamp rules and the greedy choice at temperature 0 from the step's logits and the item's history on the
//    device (tokens sampled, last, penultimate, last timestamp, done).  The partial kernel runs on a (chunk of kWhChunk logits, item) grid
//    and writes, for the text side [0, timestamp_begin) and the timestamp side separately, the largest surviving logit, its index (the
//    lower one on a tie) and sum exp(x - max); the closing kernel, one workgroup per item, joins the partials by a tree fixed by the
//    chunk index, decides (the log-sum-exp of the timestamps strictly above the best text logit: a timestamp), and writes the token, its
//    log-probability and the new history.  No atomics on floats; an item's summation order depends on V alone.
//  - wh_nospeech_kernel: softmax(unfiltered logits)[no_speech] at the start token's position, from the partial kernel's plain mode.
//  - wh_beam_partial_kernel + wh_beam_row_kernel + wh_beam_book_kernel, wh_beam_final_kernel: beam search under the same rules
//    (us_whisper_decode_beam, us_whisper_beam_select).  An item's n rows ride in one launch group; the cross keys / values stay per item
//    (wh_cross_attn_kernel reads item m / rpi), the self cache stays where each row wrote it and wh_self_attn_kernel<true> finds every
//    position's key through a per-row ancestry table.  See the section in front of the kernels.
// The host side of us_whisper_generate, us_whisper_decode and us_whisper_decode_beam is one function, wh_walk: per launch group it starts the
// state, teacher-forces the prompt but for its last token, then runs at most max_new steps of embed, layers, logits and selection and reads
// the running count back every kWhPoll steps.  A WhPolicy names the five places where the three differ: the rows per item (and with them
// whose self cache a row writes), the state that holds cur / running, the launches that start the state and that select, the ancestry table
// of the step's parity, and the launch behind the last step.  us_whisper_decoder_logits runs the same position step (wh_position) with
// logits at every position.  No kernel waits on a value another kernel writes.  Every reduction has a fixed order and no launch depends on
// the batch: an item alone or in a batch, and repeated calls, give the same bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"
#include "handle.h"
#include "kernels.h"
#include "whisper_beam.h"
#include "whisper_encoder.h"

namespace us {
namespace {

constexpr int kWhItems = 16;        // items (rows) per launch group: the columns of one 16x16x4 MFMA
constexpr int kWhPoll = 8;          // generate: steps between two reads of the running count
constexpr int kWhMaxKeys = 2048;    // keys one attention workgroup holds in LDS (S and max_target_positions)

struct WhTokens {                   // the host's token of each row of the group, or -1: take the one argmax chose
  int id[kWhItems];
};

__device__ __forceinline__ float wh_gelu(float x) { return 0.5f * x * (1.f + erff(x * 0.70710678118654752f)); }

__global__ __launch_bounds__(256) void wh_embed_kernel(const float* __restrict__ emb, const float* __restrict__ pos, const int* __restrict__ cur,
                                                       WhTokens forced, float* __restrict__ x, int H, int p) {
  const int m = blockIdx.x;
  const int tok = forced.id[m] >= 0 ? forced.id[m] : cur[m];
  for (int c = threadIdx.x; c < H; c += 256) x[(size_t)m * H + c] = emb[(size_t)tok * H + c] + pos[(size_t)p * H + c];
}

struct WhSeg {
  const float* w;             // [N][K], torch's Linear layout
  const float* bias;          // [N] or null
  float* y;                   // row m at y + m * ldy
  long long ldy;
  float scale;
};
struct WhGemmArgs {
  const float* x;             // [M][K], rows ldx apart
  const float* ln_g;          // LayerNorm of the row in front (eps 1e-5), or null
  const float* ln_b;
  const float* res;           // added last, indexed like segment 0's output; or null
  WhSeg seg[3];
  long long ldx;
  int M, N, K, gelu;
};

__global__ __launch_bounds__(256) void wh_gemm_kernel(WhGemmArgs a) {
  __shared__ float stat[kWhItems][2];
  __shared__ float red[4][16][17];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lg = lane >> 4;
  const WhSeg sg = a.seg[blockIdx.y];
  const int n0 = blockIdx.x * 16, K = a.K;
  if (a.ln_g) {
    for (int m = wave; m < kWhItems; m += 4) {
      float mean = 0.f, rs = 0.f;
      if (m < a.M) {
        const float* xr = a.x + (size_t)m * a.ldx;
        float s = 0.f;
        for (int k = lane; k < K; k += 64) s += xr[k];
        mean = wave_sum(s) / (float)K;
        float v = 0.f;
        for (int k = lane; k < K; k += 64) {
          const float d = xr[k] - mean;
          v = fmaf(d, d, v);
        }
        rs = 1.f / sqrtf(wave_sum(v) / (float)K + 1e-5f);
      }
      if (lane == 0) {
        stat[m][0] = mean;
        stat[m][1] = rs;
      }
    }
    __syncthreads();
  }
  const bool row = li < a.M;
  const float mean = a.ln_g && row ? stat[li][0] : 0.f, rs = a.ln_g && row ? stat[li][1] : 0.f;
  const float* __restrict__ wr = sg.w + (size_t)min(n0 + li, a.N - 1) * K;       // a row past N is row N - 1 again: never stored
  const float* __restrict__ xr = a.x + (size_t)(row ? li : 0) * a.ldx;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  // A = W (lane: output n0 + li, k + lg-th quarter), B = x (lane: row li, the same k): D[n = 4 lg + r][m = li]
#pragma unroll 4
  for (int k0 = wave * 16; k0 < K; k0 += 64) {
    const int k = k0 + 4 * lg;
    f32x4 w4 = {0.f, 0.f, 0.f, 0.f}, x4 = {0.f, 0.f, 0.f, 0.f};
    if (k < K) {                                                                   // K is a multiple of 4
      w4 = *reinterpret_cast<const f32x4*>(wr + k);
      if (row) {
        x4 = *reinterpret_cast<const f32x4*>(xr + k);
        if (a.ln_g) {
          const f32x4 g4 = *reinterpret_cast<const f32x4*>(a.ln_g + k), b4 = *reinterpret_cast<const f32x4*>(a.ln_b + k);
#pragma unroll
          for (int j = 0; j < 4; ++j) x4[j] = fmaf((x4[j] - mean) * rs, g4[j], b4[j]);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(w4[j], x4[j], acc, 0, 0, 0);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) red[wave][4 * lg + r][li] = acc[r];
  __syncthreads();
  const int m = tid >> 4, nl = tid & 15, n = n0 + nl;
  if (m >= a.M || n >= a.N) return;
  float v = ((red[0][nl][m] + red[1][nl][m]) + red[2][nl][m]) + red[3][nl][m];
  if (sg.bias) v += sg.bias[n];
  v *= sg.scale;
  if (a.gelu) v = wh_gelu(v);
  if (a.res) v += a.res[(size_t)m * sg.ldy + n];
  sg.y[(size_t)m * sg.ldy + n] = v;
}

// q [M][H] (scaled) against keys 0 .. n - 1 of the item's cache: kc [n][H] keys, vc the values; head h owns channels [h d, (h + 1) d).
// grid: (heads, items), one wave.  Lane j takes keys j, j + 64, ...; the maximum and the sum meet by wave_max / wave_sum; lane c then adds up
// channel c over the keys in order.
// kAnc (beam search): row m's key and value of position j live in the cache of row anc[m][j] of the group (the row that computed them: an
// ancestor of m, or m itself); the arithmetic and its order are the same.
template <bool kAnc>
__global__ __launch_bounds__(64) void wh_self_attn_kernel(const float* __restrict__ q, const float* __restrict__ cache, float* __restrict__ out,
                                                          const int* __restrict__ anc, long long item_stride, int Tm, int H, int d, int n) {
  __shared__ float qs[64];
  __shared__ float ps[kWhMaxKeys];
  __shared__ int rw[kAnc ? kWhMaxKeys : 1];
  const int lane = threadIdx.x, head = blockIdx.x, m = blockIdx.y, hd = head * d;
  const float* __restrict__ kc = cache + (kAnc ? (size_t)0 : (size_t)m * item_stride) + hd;
  const float* __restrict__ vc = kc + (size_t)Tm * H;
  qs[lane] = lane < d ? q[(size_t)m * H + hd + lane] : 0.f;
  if (kAnc)
    for (int j = lane; j < n; j += 64) rw[j] = anc[(size_t)m * Tm + j];
  __syncthreads();
  float mx = -INFINITY;
  for (int j = lane; j < n; j += 64) {
    const float* kr = kc + (kAnc ? (size_t)rw[j] * item_stride : (size_t)0) + (size_t)j * H;
    float s = 0.f;
    for (int c = 0; c < d; c += 4) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(kr + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) s = fmaf(qs[c + i], k4[i], s);
    }
    ps[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float l = 0.f;
  for (int j = lane; j < n; j += 64) {
    const float e = expf(ps[j] - mx);
    ps[j] = e;
    l += e;
  }
  l = wave_sum(l);
  __syncthreads();
  if (lane < d) {
    float o = 0.f;
    for (int j = 0; j < n; ++j) o = fmaf(ps[j], vc[(kAnc ? (size_t)rw[j] * item_stride : (size_t)0) + (size_t)j * H + lane], o);
    out[(size_t)m * H + hd + lane] = o / l;
  }
}

// q [M][H] (scaled) against the S encoder frames: kv [2 H][S] planar per item (keys, then values).  grid: (heads, rows), kWhCrossWaves waves.
// Row m reads item m / rpi: greedy decoding has one row per item (rpi = 1), a beam's rows share their item's keys and values.
// Thread t takes frames t, t + 64 kWhCrossWaves, ...; wave w then adds up channels w, w + kWhCrossWaves, ... of the head, a lane over frames
// lane, lane + 64, ...  The loops are unrolled so that a thread has several loads in flight; the order of every sum is the loop's.
constexpr int kWhCrossWaves = 16;

__global__ __launch_bounds__(64 * kWhCrossWaves) void wh_cross_attn_kernel(const float* __restrict__ q, const float* __restrict__ kv,
                                                                           float* __restrict__ out, long long item_stride, int S, int H, int d,
                                                                           int rpi) {
  constexpr int NT = 64 * kWhCrossWaves;
  __shared__ float qs[64];
  __shared__ float ps[kWhMaxKeys];
  __shared__ float red[kWhCrossWaves];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, head = blockIdx.x, m = blockIdx.y, hd = head * d;
  const float* __restrict__ kp = kv + (size_t)(m / rpi) * item_stride + (size_t)hd * S;
  const float* __restrict__ vp = kp + (size_t)H * S;
  if (tid < 64) qs[tid] = tid < d ? q[(size_t)m * H + hd + tid] : 0.f;
  __syncthreads();
  float mx = -INFINITY;
  for (int j = tid; j < S; j += NT) {
    float s = 0.f;
#pragma unroll 16
    for (int c = 0; c < d; ++c) s = fmaf(qs[c], kp[(size_t)c * S + j], s);
    ps[j] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  mx = red[0];
#pragma unroll
  for (int w = 1; w < kWhCrossWaves; ++w) mx = fmaxf(mx, red[w]);
  float l = 0.f;
  for (int j = tid; j < S; j += NT) {
    const float e = expf(ps[j] - mx);
    ps[j] = e;
    l += e;
  }
  l = wave_sum(l);
  __syncthreads();
  if (lane == 0) red[wave] = l;
  __syncthreads();
  l = 0.f;
#pragma unroll
  for (int w = 0; w < kWhCrossWaves; ++w) l += red[w];
  for (int c = wave; c < d; c += kWhCrossWaves) {
    const float* vr = vp + (size_t)c * S;
    float o = 0.f;
#pragma unroll 8
    for (int j = lane; j < S; j += 64) o = fmaf(ps[j], vr[j], o);
    o = wave_sum(o);
    if (lane == 0) out[(size_t)m * H + hd + c] = o / l;
  }
}

struct WhDecState {                 // a group's loop state in the workspace, one row per item
  int *cur, *done, *running;        // [kWhItems] the token chosen last, the item has ended; the items of the group that have not
  int *count, *last, *pen, *last_ts;        // [kWhItems] tokens sampled so far, the last two of them, the last timestamp (-1: none)
  double* sum;                      // [kWhItems] the sum of the log-probabilities
};

// item m of the group: the largest logit that no mask suppresses, the lower index on a tie; tokens[m][step] and the item's end
__global__ __launch_bounds__(256) void wh_argmax_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ suppress,
                                                        const unsigned char* __restrict__ begin, WhDecState st, long long* __restrict__ tokens,
                                                        long long* __restrict__ n, int V, int max_new, int step, int eos) {
  __shared__ float rv[4];
  __shared__ int ri[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.x;
  const float* __restrict__ x = logits + (size_t)m * V;
  float best = -INFINITY;
  int idx = 0x7fffffff;
  for (int v = tid; v < V; v += 256) {
    if ((suppress && suppress[v]) || (begin && begin[v])) continue;
    const float y = x[v];
    if (y > best || (idx == 0x7fffffff && y == best)) {
      best = y;
      idx = v;
    }
  }
  auto take = [&](float ov, int oi) {
    if (ov > best || (ov == best && oi < idx)) {
      best = ov;
      idx = oi;
    }
  };
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) take(__shfl_xor(best, o), __shfl_xor(idx, o));
  if (lane == 0) {
    rv[wave] = best;
    ri[wave] = idx;
  }
  __syncthreads();
  if (tid != 0) return;
  for (int w = 1; w < 4; ++w) take(rv[w], ri[w]);
  if (st.done[m]) return;                               // tokens[m][step] holds eos already
  const int tok = idx == 0x7fffffff ? eos : idx;        // every token suppressed: the item ends
  st.cur[m] = tok;
  tokens[(size_t)m * max_new + step] = tok;
  if (tok == eos) {
    st.done[m] = 1;
    atomicSub(st.running, 1);
  } else {
    n[m] += 1;
  }
}

// ---- the selection stage under the timestamp rules ----------------------------------------------------------------------------------

constexpr int kWhChunk = 512;       // logits per workgroup of the partial kernel: 102 chunks at V = 51,865

struct WhRules {
  int eos, tb, max_init;            // tb = no_timestamps + 1: the first timestamp token; max_init -1: no cap at the first position
};
struct WhPart {                     // one side of one chunk: the largest surviving logit (-inf: none), sum exp(x - m), the index of m
  float m, s;
  int bi, pad;
};
struct WhHistory {                  // us_whisper_select, us_whisper_beam_select: the histories of a group's rows, from the host
  int count[kWhItems], last[kWhItems], pen[kWhItems], last_ts[kWhItems], done[kWhItems];
};
constexpr int kWhNone = 0x7fffffff;

__device__ __forceinline__ void wh_take(float& bv, int& bi, float ov, int oi) {       // the larger value, the lower index on a tie
  if (ov > bv || (ov == bv && oi < bi)) {
    bv = ov;
    bi = oi;
  }
}
// (value, index) of every thread of a 256-thread workgroup -> the best of all in every thread; red: 4 slots each
__device__ __forceinline__ void wh_block_best(float& bv, int& bi, float* rv, int* ri) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) wh_take(bv, bi, __shfl_xor(bv, o), __shfl_xor(bi, o));
  __syncthreads();
  if (lane == 0) {
    rv[wave] = bv;
    ri[wave] = bi;
  }
  __syncthreads();
  bv = rv[0];
  bi = ri[0];
#pragma unroll
  for (int w = 1; w < 4; ++w) wh_take(bv, bi, rv[w], ri[w]);
}
// one value per thread -> the workgroup's sum in every thread: the wave butterfly, then the four waves in order
__device__ __forceinline__ float wh_block_sum(float v, float* rs) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  v = wave_sum(v);
  __syncthreads();
  if (lane == 0) rs[wave] = v;
  __syncthreads();
  return ((rs[0] + rs[1]) + rs[2]) + rs[3];
}

// grid: (chunks, items).  plain: every token survives and counts as text (the no-speech probability).
// the surviving ranges of the two sides, from a row's history: text [text_lo, text_hi), timestamps [ts_lo, ts_hi); first: no token sampled yet
struct WhRanges {
  int text_lo, text_hi, ts_lo, ts_hi, first;
};
__device__ __forceinline__ WhRanges wh_ranges(const WhRules& r, int V, int count, int last, int pen, int lts) {
  WhRanges g{0, r.tb, r.tb, V, count == 0};
  const bool last_is = count >= 1 && last >= r.tb, pen_is = count < 2 || pen >= r.tb;
  if (last_is && pen_is) g.ts_hi = g.ts_lo;
  if (last_is && !pen_is) g.text_lo = r.eos;
  if (lts >= 0) g.ts_lo = max(g.ts_lo, last_is && !pen_is ? lts : lts + 1);
  if (g.first) {
    g.text_hi = 0;
    if (r.max_init >= 0) g.ts_hi = min(g.ts_hi, r.tb + r.max_init + 1);
  }
  return g;
}

__global__ __launch_bounds__(256) void wh_select_partial_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ suppress,
                                                                const unsigned char* __restrict__ begin, WhDecState st, WhRules r,
                                                                WhPart* __restrict__ part, int V, int nchunks, int plain) {
  __shared__ float rv[4], rs[4];
  __shared__ int ri[4];
  const int tid = threadIdx.x, chunk = blockIdx.x, m = blockIdx.y;
  // the surviving ranges of the two sides
  int text_lo = 0, text_hi = r.tb, ts_lo = r.tb, ts_hi = V, first = 0, no_ts = r.tb - 1;
  if (plain) {
    text_hi = V;
    ts_lo = V;
    no_ts = -1;
  } else {
    const WhRanges g = wh_ranges(r, V, st.count[m], st.last[m], st.pen[m], st.last_ts[m]);
    text_lo = g.text_lo, text_hi = g.text_hi, ts_lo = g.ts_lo, ts_hi = g.ts_hi, first = g.first;
  }
  const float* __restrict__ x = logits + (size_t)m * V;
  float y[2];
  int side[2];                      // 0 text, 1 timestamp, -1 masked
  float tv = -INFINITY, sv = -INFINITY;
  int ti = kWhNone, si = kWhNone;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int v = chunk * kWhChunk + j * 256 + tid;
    side[j] = -1;
    y[j] = -INFINITY;
    if (v >= V || v == no_ts) continue;
    if (!plain && ((suppress && suppress[v]) || (first && begin && begin[v]))) continue;
    if (v >= text_lo && v < text_hi) side[j] = 0;
    else if (v >= ts_lo && v < ts_hi) side[j] = 1;
    else continue;
    y[j] = x[v];
    if (side[j] == 0) wh_take(tv, ti, y[j], v);
    else wh_take(sv, si, y[j], v);
  }
  wh_block_best(tv, ti, rv, ri);
  wh_block_best(sv, si, rv, ri);
  float te = 0.f, se = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (side[j] == 0 && tv > -INFINITY) te += expf(y[j] - tv);
    if (side[j] == 1 && sv > -INFINITY) se += expf(y[j] - sv);
  }
  te = wh_block_sum(te, rs);
  se = wh_block_sum(se, rs);
  if (tid == 0) {
    part[((size_t)m * 2 + 0) * nchunks + chunk] = WhPart{tv, te, ti, 0};
    part[((size_t)m * 2 + 1) * nchunks + chunk] = WhPart{sv, se, si, 0};
  }
}

// the partials of one side of item m -> (max, its index, sum exp(x - max)) in every thread
__device__ __forceinline__ void wh_join(const WhPart* __restrict__ p, int nchunks, float& M, int& I, float& S, float* rv, int* ri, float* rs) {
  M = -INFINITY;
  I = kWhNone;
  for (int c = threadIdx.x; c < nchunks; c += 256) wh_take(M, I, p[c].m, p[c].bi);
  wh_block_best(M, I, rv, ri);
  float s = 0.f;
  if (M > -INFINITY)
    for (int c = threadIdx.x; c < nchunks; c += 256)
      if (p[c].m > -INFINITY) s += p[c].s * expf(p[c].m - M);
  S = wh_block_sum(s, rs);
}

// grid: items.  tokens[m][step], n[m] and the running count as wh_argmax_kernel; sum_out[m] the item's summed log-probability so far;
// step_lp / decided (or null): this step's log-probability and whether the timestamps won the decision.
__global__ __launch_bounds__(256) void wh_select_close_kernel(const WhPart* __restrict__ part, WhDecState st, WhRules r, long long* __restrict__ tokens,
                                                              long long* __restrict__ n, float* __restrict__ sum_out, float* __restrict__ step_lp,
                                                              int* __restrict__ decided, int nchunks, int max_new, int step) {
  __shared__ float rv[4], rs[4];
  __shared__ int ri[4];
  const int m = blockIdx.x;
  float Mt, St, Ms, Ss;
  int It, Is;
  wh_join(part + ((size_t)m * 2 + 0) * nchunks, nchunks, Mt, It, St, rv, ri, rs);
  wh_join(part + ((size_t)m * 2 + 1) * nchunks, nchunks, Ms, Is, Ss, rv, ri, rs);
  if (threadIdx.x != 0 || st.done[m]) return;            // a done item: tokens[m][step] holds eos already
  const float lse_ts = Ss > 0.f ? Ms + logf(Ss) : -INFINITY;
  const bool ts_wins = lse_ts > Mt;
  int tok = r.eos;                                      // nothing survives: the item ends, at no cost
  float lp = 0.f;
  if (ts_wins) {
    tok = Is;
    lp = Ms - lse_ts;
  } else if (It != kWhNone) {
    const float M = fmaxf(Mt, Ms);                      // Mt is finite or It the first of a side of -inf
    const float S = (Mt > -INFINITY ? St * expf(Mt - M) : 0.f) + (Ms > -INFINITY ? Ss * expf(Ms - M) : 0.f);
    tok = It;
    lp = S > 0.f ? Mt - (M + logf(S)) : 0.f;
  }
  st.cur[m] = tok;
  st.pen[m] = st.last[m];
  st.last[m] = tok;
  st.count[m] += 1;
  if (tok >= r.tb) st.last_ts[m] = tok;
  st.sum[m] += (double)lp;
  tokens[(size_t)m * max_new + step] = tok;
  if (sum_out) sum_out[m] = (float)st.sum[m];
  if (step_lp) step_lp[m] = lp;
  if (decided) decided[m] = ts_wins ? 1 : 0;
  if (tok == r.eos) {
    st.done[m] = 1;
    atomicSub(st.running, 1);
  } else {
    n[m] += 1;
  }
}

// grid: items.  out[item] = exp(x[no_speech] - logsumexp(x)) of row m = item * rpi (a beam's first row) from the plain partials (the text
// side holds every token)
__global__ __launch_bounds__(256) void wh_nospeech_kernel(const WhPart* __restrict__ part, const float* __restrict__ logits, float* __restrict__ out,
                                                          int V, int nchunks, int no_speech, int rpi) {
  __shared__ float rv[4], rs[4];
  __shared__ int ri[4];
  const int m = blockIdx.x * rpi;
  float M, S;
  int I;
  wh_join(part + ((size_t)m * 2 + 0) * nchunks, nchunks, M, I, S, rv, ri, rs);
  if (threadIdx.x == 0) out[blockIdx.x] = S > 0.f ? expf(logits[(size_t)m * V + no_speech] - (M + logf(S))) : 0.f;
}

// The state of a group of nb items as a decoding starts (hist null in effect: use_hist 0) or from the host's histories (us_whisper_select),
// and what an item returns that never chooses a token: tokens = eos, n = 0, and zeros in whichever of sum_out / logprob / decided is given.
__global__ __launch_bounds__(256) void wh_state_init_kernel(WhDecState st, WhHistory hist, int use_hist, long long* __restrict__ tokens,
                                                            long long* __restrict__ n, float* __restrict__ sum_out, float* __restrict__ logprob,
                                                            int* __restrict__ decided, int nb, int max_new, long long eos) {
  const int tid = threadIdx.x;
  if (tid < kWhItems) {
    st.cur[tid] = 0;
    st.done[tid] = use_hist ? hist.done[tid] : 0;
    st.count[tid] = use_hist ? hist.count[tid] : 0;
    st.last[tid] = use_hist ? hist.last[tid] : -1;
    st.pen[tid] = use_hist ? hist.pen[tid] : -1;
    st.last_ts[tid] = use_hist ? hist.last_ts[tid] : -1;
    st.sum[tid] = 0.0;
  }
  if (tid < nb) {
    n[tid] = 0;
    if (sum_out) sum_out[tid] = 0.f;
    if (logprob) logprob[tid] = 0.f;
    if (decided) decided[tid] = 0;
  }
  if (tid == 0) *st.running = nb;
  for (int i = tid; i < nb * max_new; i += 256) tokens[i] = eos;
}

inline int wh_chunks(int V) { return (V + kWhChunk - 1) / kWhChunk; }
// floats of the selection stage's state and partials: 8 int arrays, the sums (doubles), n (long long), the partials of both sides
inline size_t wh_select_floats(int V) { return pad64(8 * kWhItems) + pad64(2 * kWhItems) + pad64(2 * kWhItems) + pad64((size_t)kWhItems * 2 * wh_chunks(V) * 4); }

struct WhSelect {                   // the stage's buffers in a scratch of wh_select_floats(V) floats
  WhDecState st;
  long long* n;
  WhPart* part;
};
inline WhSelect wh_select_carve(float* base) {
  int* ints = reinterpret_cast<int*>(base);
  WhSelect c;
  c.st = WhDecState{ints, ints + kWhItems, ints + 2 * kWhItems, ints + 3 * kWhItems, ints + 4 * kWhItems, ints + 5 * kWhItems, ints + 6 * kWhItems,
                    reinterpret_cast<double*>(base + pad64(8 * kWhItems))};
  c.n = reinterpret_cast<long long*>(base + pad64(8 * kWhItems) + pad64(2 * kWhItems));
  c.part = reinterpret_cast<WhPart*>(base + pad64(8 * kWhItems) + 2 * pad64(2 * kWhItems));
  return c;
}

// the two launches of one selection step of a group
inline void wh_select_step(const float* L, const unsigned char* suppress, const unsigned char* begin, const WhSelect& c, const WhRules& r, long long* tokens,
                           long long* n, float* sum_out, float* step_lp, int* decided, int V, int nb, int max_new, int step, hipStream_t s) {
  const int nc = wh_chunks(V);
  hipLaunchKernelGGL(wh_select_partial_kernel, dim3(nc, nb), dim3(256), 0, s, L, suppress, begin, c.st, r, c.part, V, nc, 0);
  hipLaunchKernelGGL(wh_select_close_kernel, dim3(nb), dim3(256), 0, s, c.part, c.st, r, tokens, n, sum_out, step_lp, decided, nc, max_new, step);
}

// ---- beam search under the timestamp rules ------------------------------------------------------------------------------------------
// An item has n rows (beam_size), item-major in a launch group of floor(16 / n) whole items, so a group's step still streams every weight
// once.  Four launches follow the step's logits:
//  - wh_beam_partial_kernel, grid (chunks, rows): wh_select_partial_kernel's masks, maxima and sums, and beside them per side the chunk's top
//    n + 1 finite survivors (value, index), placed by counting rank in LDS (the larger value, the lower index on a tie);
//  - wh_beam_row_kernel, grid rows: joins the partials as wh_select_close_kernel does, decides text against timestamps, and picks the row's top
//    n + 1 survivors out of the chunks' lists, one after the other in the strict order (value, index): the result does not depend on how the
//    lists are visited.  -> the row's candidates (token, log-probability);
//  - wh_beam_book_kernel, one workgroup per item: ranks the <= n (n + 1) candidates by counting in LDS, walks them (whisper_beam.h), and writes
//    the new rows' scores, histories, sequences and ancestry, the pool and the item's end;
//  - wh_beam_final_kernel, once per group: tops the pool up, ranks it, and writes the winner.
// Sequences and ancestry are ping-pong tables indexed by the step's parity; scores are doubles, as us_whisper_decode's sums.

constexpr int kWhTop = kWbMaxBeam + 1;      // candidates a row offers at most

struct WhBeamState {                // a group's state: rows [kWhItems], items [kWhItems]
  int *cur, *live, *count, *last, *pen, *last_ts;       // rows: the token to embed next, live, and the history as WhDecState
  int *cand_n, *done, *pool_n, *nsteps, *running;       // rows: candidates offered; items: ended, pool entries, steps taken; the group's running items
  double* score;                    // rows
  int* cand_tok;                    // [rows][kWhTop]
  float* cand_lp;
  int *seq, *anc;                   // [2][rows][L] the sampled sequences, [2][rows][Tm] position -> group row that holds its key
  double* pool_score;               // [items][kWbMaxPool]
  int *pool_len, *pool_seq;         // [items][kWbMaxPool], [items][kWbMaxPool][L]
  WhPart* part;                     // [rows][2][chunks]
  float* topv;                      // [rows][2][chunks][kWhTop]
  int *topi, *topn;                 // the same, and [rows][2][chunks] how many are valid
};
struct WhBeamHist {                 // us_whisper_beam_select: the group's rows, from the host; a row that is not done is live
  WhHistory h;
  double score[kWhItems];
};
struct WhBeamOut {                  // us_whisper_beam_select's results per item, or nulls
  int* parent;                      // [items][n], -1: the row is dead
  long long* token;                 // [items][n]
  double* score;                    // [items][n]
  int* n_live;                      // [items]
  int* fin_parent;                  // [items][n] in walk order
  double* fin_score;
  int* n_fin;                       // [items]
};

// hist: null (a decoding starts: row 0 of every item live, nothing sampled) or the host's rows.  L, Tm: the strides of seq and anc.
__global__ __launch_bounds__(256) void wh_beam_init_kernel(WhBeamState st, WhBeamHist hist, int use_hist, int n, int items, int eos, int L, int Tm) {
  const int tid = threadIdx.x;
  if (tid < kWhItems) {
    const bool row = tid < items * n;
    st.cur[tid] = eos;
    st.live[tid] = row && (use_hist ? !hist.h.done[tid] : tid % n == 0) ? 1 : 0;
    st.count[tid] = use_hist ? hist.h.count[tid] : 0;
    st.last[tid] = use_hist ? hist.h.last[tid] : -1;
    st.pen[tid] = use_hist ? hist.h.pen[tid] : -1;
    st.last_ts[tid] = use_hist ? hist.h.last_ts[tid] : -1;
    st.score[tid] = use_hist ? hist.score[tid] : 0.0;
    st.cand_n[tid] = 0;
    st.done[tid] = 0;
    st.pool_n[tid] = 0;
    st.nsteps[tid] = 0;
  }
  if (tid == 0) *st.running = items;
  for (int i = tid; i < 2 * kWhItems * Tm; i += 256) st.anc[i] = (i / Tm) % kWhItems;
  for (int i = tid; i < 2 * kWhItems * L; i += 256) st.seq[i] = eos;
}

// grid: (chunks, rows)
__global__ __launch_bounds__(256) void wh_beam_partial_kernel(const float* __restrict__ logits, const unsigned char* __restrict__ suppress,
                                                              const unsigned char* __restrict__ begin, WhBeamState st, WhRules r, int V, int nchunks,
                                                              int n) {
  __shared__ float rv[4], rs[4];
  __shared__ int ri[4];
  __shared__ float yv[kWhChunk];
  __shared__ int sd[kWhChunk];
  const int tid = threadIdx.x, chunk = blockIdx.x, m = blockIdx.y, K = n + 1;
  if (!st.live[m] || st.done[m / n]) return;            // the row offers nothing: its partials are not read
  const WhRanges g = wh_ranges(r, V, st.count[m], st.last[m], st.pen[m], st.last_ts[m]);
  const int no_ts = r.tb - 1;
  const float* __restrict__ x = logits + (size_t)m * V;
  float y[2];
  int side[2];                      // 0 text, 1 timestamp, -1 masked
  float tv = -INFINITY, sv = -INFINITY;
  int ti = kWhNone, si = kWhNone;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int v = chunk * kWhChunk + j * 256 + tid;
    side[j] = -1;
    y[j] = -INFINITY;
    if (v < V && v != no_ts && !((suppress && suppress[v]) || (g.first && begin && begin[v]))) {
      if (v >= g.text_lo && v < g.text_hi) side[j] = 0;
      else if (v >= g.ts_lo && v < g.ts_hi) side[j] = 1;
      if (side[j] >= 0) {
        y[j] = x[v];
        if (side[j] == 0) wh_take(tv, ti, y[j], v);
        else wh_take(sv, si, y[j], v);
      }
    }
    yv[j * 256 + tid] = y[j];
    sd[j * 256 + tid] = y[j] > -INFINITY ? side[j] : -1;        // a token at -inf is never a candidate
  }
  wh_block_best(tv, ti, rv, ri);
  wh_block_best(sv, si, rv, ri);
  float te = 0.f, se = 0.f, tc = 0.f, sc = 0.f;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    if (side[j] == 0 && tv > -INFINITY) te += expf(y[j] - tv);
    if (side[j] == 1 && sv > -INFINITY) se += expf(y[j] - sv);
    if (side[j] == 0 && y[j] > -INFINITY) tc += 1.f;
    if (side[j] == 1 && y[j] > -INFINITY) sc += 1.f;
  }
  te = wh_block_sum(te, rs);
  se = wh_block_sum(se, rs);
  tc = wh_block_sum(tc, rs);        // counts up to 512: exact
  sc = wh_block_sum(sc, rs);
  const size_t p0 = ((size_t)m * 2 + 0) * nchunks + chunk, p1 = ((size_t)m * 2 + 1) * nchunks + chunk;
  if (tid == 0) {
    st.part[p0] = WhPart{tv, te, ti, 0};
    st.part[p1] = WhPart{sv, se, si, 0};
    st.topn[p0] = min((int)tc, K);
    st.topn[p1] = min((int)sc, K);
  }
  // the place of each finite survivor among those of its side in this chunk: the larger value first, then the lower index
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int own = j * 256 + tid, sj = sd[own];
    if (sj < 0) continue;
    int rank = 0;
    for (int u = 0; u < kWhChunk && rank < K; ++u) rank += sd[u] == sj && (yv[u] > y[j] || (yv[u] == y[j] && u < own)) ? 1 : 0;
    if (rank < K) {
      const size_t e = (sj == 0 ? p0 : p1) * kWhTop + rank;
      st.topv[e] = y[j];
      st.topi[e] = chunk * kWhChunk + own;
    }
  }
}

// grid: rows.  The row's candidates: its top n + 1 survivors (token, log-probability), or (eos, 0) when nothing survives.
__global__ __launch_bounds__(256) void wh_beam_row_kernel(WhBeamState st, WhRules r, int nchunks, int n) {
  __shared__ float rv[4], rs[4];
  __shared__ int ri[4];
  const int m = blockIdx.x, K = n + 1;
  if (!st.live[m] || st.done[m / n]) {
    if (threadIdx.x == 0) st.cand_n[m] = 0;
    return;
  }
  const WhPart* pt = st.part + ((size_t)m * 2 + 0) * nchunks;
  float Mt, St, Ms, Ss;
  int It, Is;
  wh_join(pt, nchunks, Mt, It, St, rv, ri, rs);
  wh_join(pt + nchunks, nchunks, Ms, Is, Ss, rv, ri, rs);
  const float lse_ts = Ss > 0.f ? Ms + logf(Ss) : -INFINITY;
  const bool ts_wins = lse_ts > Mt;
  float lse = lse_ts;
  if (!ts_wins) {
    const float M = fmaxf(Mt, Ms);
    const float S = (Mt > -INFINITY ? St * expf(Mt - M) : 0.f) + (Ms > -INFINITY ? Ss * expf(Ms - M) : 0.f);
    lse = S > 0.f ? M + logf(S) : -INFINITY;
  }
  // entries [side][chunk][k]; with the timestamps winning only side 1 counts
  const int e0 = ts_wins ? nchunks * kWhTop : 0, e1 = 2 * nchunks * kWhTop;
  const float* tv = st.topv + (size_t)m * 2 * nchunks * kWhTop;
  const int* ti = st.topi + (size_t)m * 2 * nchunks * kWhTop;
  const int* tn = st.topn + (size_t)m * 2 * nchunks;
  float pv = INFINITY;
  int pi = -1, got = 0;
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY;
    int bi = kWhNone;
    for (int e = e0 + threadIdx.x; e < e1; e += 256) {
      if (e % kWhTop >= tn[e / kWhTop]) continue;
      const float v = tv[e];
      const int i = ti[e];
      if (v < pv || (v == pv && i > pi)) wh_take(bv, bi, v, i);       // behind the last one taken
    }
    wh_block_best(bv, bi, rv, ri);
    if (bi == kWhNone || !(lse > -INFINITY)) break;
    if (threadIdx.x == 0) {
      st.cand_tok[m * kWhTop + k] = bi;
      st.cand_lp[m * kWhTop + k] = bv - lse;
    }
    pv = bv;
    pi = bi;
    ++got;
  }
  if (threadIdx.x == 0) {
    if (got == 0) {
      st.cand_tok[m * kWhTop] = r.eos;
      st.cand_lp[m * kWhTop] = 0.f;
      got = 1;
    }
    st.cand_n[m] = got;
  }
}

// grid: items.  step: the sequences hold `step` tokens; pos: the position this step's rows wrote in the self cache.  tables: 0 leaves the
// sequence, ancestry and pool tables alone (us_whisper_beam_select).
__global__ __launch_bounds__(256) void wh_beam_book_kernel(WhBeamState st, WhRules r, WhBeamOut out, int n, int C, int step, int pos, int L, int Tm,
                                                           int tables) {
  __shared__ double tot[kWbMaxCands];
  __shared__ int par[kWbMaxCands], tok[kWbMaxCands], ord[kWbMaxCands];
  __shared__ int cbase[kWbMaxBeam + 1], hc[kWbMaxBeam], hl[kWbMaxBeam], hts[kWbMaxBeam];
  __shared__ WbRow rows[kWbMaxBeam];
  __shared__ WbFin fin[kWbMaxCands];
  __shared__ WbWalk w;
  const int tid = threadIdx.x, item = blockIdx.x, base = item * n;
  if (st.done[item]) return;
  if (tid == 0) {
    int c = 0;
    for (int j = 0; j < n; ++j) {
      cbase[j] = c;
      c += st.live[base + j] ? min(max(st.cand_n[base + j], 0), n + 1) : 0;
    }
    cbase[n] = c;
  }
  if (tid < n) {
    hc[tid] = st.count[base + tid];
    hl[tid] = st.last[base + tid];
    hts[tid] = st.last_ts[base + tid];
  }
  __syncthreads();
  const int count = cbase[n];
  for (int c = tid; c < count; c += 256) {
    int j = 0;
    while (j + 1 < n && cbase[j + 1] <= c) ++j;
    const int k = c - cbase[j];
    par[c] = j;
    tok[c] = st.cand_tok[(base + j) * kWhTop + k];
    tot[c] = st.score[base + j] + (double)st.cand_lp[(base + j) * kWhTop + k];
  }
  __syncthreads();
  for (int c = tid; c < count; c += 256) ord[wb_rank(tot, count, c)] = c;
  __syncthreads();
  // a row offers eos at most once, so at most n entries finish (fin holds one per candidate all the same)
  if (tid == 0) w = wb_walk(ord, par, tok, tot, count, n, C, r.eos, st.pool_n[item], rows, fin);
  __syncthreads();
  const int ob = step & 1, nb = ob ^ 1, pool0 = st.pool_n[item];
  if (tables) {
    for (int a = 0; a < w.added; ++a) {
      const int* src = st.seq + ((size_t)ob * kWhItems + base + fin[a].parent) * L;
      int* dst = st.pool_seq + ((size_t)item * kWbMaxPool + pool0 + a) * L;
      for (int t = tid; t < step; t += 256) dst[t] = src[t];
    }
    for (int k = 0; k < n; ++k) {
      const int j = k < w.rows ? rows[k].parent : k;
      if (k < w.rows) {
        const int* src = st.seq + ((size_t)ob * kWhItems + base + j) * L;
        int* dst = st.seq + ((size_t)nb * kWhItems + base + k) * L;
        for (int t = tid; t < step; t += 256) dst[t] = src[t];
        if (tid == 0 && step < L) dst[step] = rows[k].token;
      }
      const int* as = st.anc + ((size_t)ob * kWhItems + base + j) * Tm;
      int* ad = st.anc + ((size_t)nb * kWhItems + base + k) * Tm;
      for (int t = tid; t <= pos + 1 && t < Tm; t += 256) ad[t] = t <= pos && k < w.rows ? as[t] : base + k;
    }
  }
  __syncthreads();                  // every read of the old rows lies in front of these writes
  if (tid < n) {
    const int k = tid, m = base + k;
    if (k < w.rows) {
      const int j = rows[k].parent, t = rows[k].token;
      st.live[m] = 1;
      st.cur[m] = t;
      st.count[m] = hc[j] + 1;
      st.pen[m] = hl[j];
      st.last[m] = t;
      st.last_ts[m] = t >= r.tb ? t : hts[j];
      st.score[m] = rows[k].score;
    } else {
      st.live[m] = 0;
      st.cur[m] = r.eos;
    }
    if (out.parent) {
      out.parent[m] = k < w.rows ? rows[k].parent : -1;
      out.token[m] = k < w.rows ? rows[k].token : r.eos;
      out.score[m] = k < w.rows ? rows[k].score : 0.0;
      out.fin_parent[m] = k < w.finished ? fin[k].parent : -1;
      out.fin_score[m] = k < w.finished ? fin[k].score : 0.0;
    }
  }
  if (tid == 0) {
    for (int a = 0; a < w.added; ++a) {
      st.pool_score[item * kWbMaxPool + pool0 + a] = fin[a].score;
      st.pool_len[item * kWbMaxPool + pool0 + a] = step;
    }
    st.pool_n[item] = pool0 + w.added;
    st.nsteps[item] = step + 1;
    if (out.parent) {
      out.n_live[item] = w.rows;
      out.n_fin[item] = w.finished;
    }
    if (w.ended) {
      st.done[item] = 1;
      atomicSub(st.running, 1);
    }
  }
}

// grid: items.  finalise and rank: tokens[item][max_new] (eos at and after the end), cnt[item], sum_out[item]
__global__ __launch_bounds__(256) void wh_beam_final_kernel(WhBeamState st, long long* __restrict__ tokens, long long* __restrict__ cnt,
                                                            float* __restrict__ sum_out, int n, int L, int max_new, int eos) {
  __shared__ double sc[kWbMaxPool + kWbMaxBeam];
  __shared__ int len[kWbMaxPool + kWbMaxBeam], top[kWbMaxBeam];
  __shared__ int win, total, pool;
  const int tid = threadIdx.x, item = blockIdx.x, base = item * n;
  if (tid == 0) {
    pool = min(st.pool_n[item], kWbMaxPool);
    for (int i = 0; i < pool; ++i) {
      sc[i] = st.pool_score[item * kWbMaxPool + i];
      len[i] = st.pool_len[item * kWbMaxPool + i];
    }
    const int k = wb_top_up(st.live + base, st.score + base, n, pool, top);
    for (int u = 0; u < k; ++u) {
      sc[pool + u] = st.score[base + top[u]];
      len[pool + u] = st.count[base + top[u]];
    }
    total = pool + k;
    win = total > 0 ? wb_winner(sc, len, total) : -1;
  }
  __syncthreads();
  const int length = win < 0 ? 0 : min(len[win], max_new);
  const int* src = win < 0 ? nullptr
                   : win < pool ? st.pool_seq + ((size_t)item * kWbMaxPool + win) * L
                                : st.seq + ((size_t)(st.nsteps[item] & 1) * kWhItems + base + top[win - pool]) * L;
  for (int t = tid; t < max_new; t += 256) tokens[(size_t)item * max_new + t] = t < length ? src[t] : eos;
  if (tid == 0) {
    cnt[item] = length;
    sum_out[item] = win < 0 ? 0.f : (float)sc[win];
  }
}

// floats of a group's beam state with sequences of L tokens, ancestry over Tm positions and the partials of V logits
inline size_t wh_beam_floats(int V, int L, int Tm) {
  const size_t nc = (size_t)wh_chunks(V), R = kWhItems;
  return pad64(11 * R) + pad64(2 * R) + 2 * pad64(R * kWhTop) + pad64(2 * R * L) + pad64(2 * R * Tm) + pad64(2 * R * kWbMaxPool) + pad64(R * kWbMaxPool) +
         pad64(R * kWbMaxPool * L) + pad64(R * 2 * nc * 4) + 2 * pad64(R * 2 * nc * kWhTop) + pad64(R * 2 * nc);
}
inline WhBeamState wh_beam_carve(float* base, int V, int L, int Tm) {
  const size_t nc = (size_t)wh_chunks(V), R = kWhItems;
  WsTake take;
  auto at = [&](size_t floats) { return base + take(floats); };
  int* ints = reinterpret_cast<int*>(at(11 * R));
  WhBeamState s{};
  s.cur = ints; s.live = ints + R; s.count = ints + 2 * R; s.last = ints + 3 * R; s.pen = ints + 4 * R; s.last_ts = ints + 5 * R;
  s.cand_n = ints + 6 * R; s.done = ints + 7 * R; s.pool_n = ints + 8 * R; s.nsteps = ints + 9 * R; s.running = ints + 10 * R;
  s.score = reinterpret_cast<double*>(at(2 * R));
  s.cand_tok = reinterpret_cast<int*>(at(R * kWhTop));
  s.cand_lp = at(R * kWhTop);
  s.seq = reinterpret_cast<int*>(at(2 * R * L));
  s.anc = reinterpret_cast<int*>(at(2 * R * Tm));
  s.pool_score = reinterpret_cast<double*>(at(2 * R * kWbMaxPool));
  s.pool_len = reinterpret_cast<int*>(at(R * kWbMaxPool));
  s.pool_seq = reinterpret_cast<int*>(at(R * kWbMaxPool * L));
  s.part = reinterpret_cast<WhPart*>(at(R * 2 * nc * 4));
  s.topv = at(R * 2 * nc * kWhTop);
  s.topi = reinterpret_cast<int*>(at(R * 2 * nc * kWhTop));
  s.topn = reinterpret_cast<int*>(at(R * 2 * nc));
  return s;
}

// the three launches of one beam step of a group of `items` items behind its logits
inline void wh_beam_step(const float* L, const unsigned char* suppress, const unsigned char* begin, const WhBeamState& st, const WhRules& r,
                         const WhBeamOut& out, int V, int n, int C, int items, int step, int pos, int Ls, int Tm, int tables, hipStream_t s) {
  const int nc = wh_chunks(V);
  hipLaunchKernelGGL(wh_beam_partial_kernel, dim3(nc, items * n), dim3(256), 0, s, L, suppress, begin, st, r, V, nc, n);
  hipLaunchKernelGGL(wh_beam_row_kernel, dim3(items * n), dim3(256), 0, s, st, r, nc, n);
  hipLaunchKernelGGL(wh_beam_book_kernel, dim3(items), dim3(256), 0, s, st, r, out, n, C, step, pos, Ls, Tm, tables);
}

struct WhLinear {
  const float *w = nullptr, *b = nullptr;
};
struct WhDecLayer {
  const float *ln1_g, *ln1_b, *ln2_g, *ln2_b, *ln3_g, *ln3_b;
  WhLinear q, k, v, o, cq, co, fc1, fc2;
};

}  // namespace
}  // namespace us

struct us_whisper : us::WeightTable {
  us_whisper_config cfg{};
  us::WhEncoder* enc = nullptr;
  std::vector<us::WhDecLayer> dec;
  const float *embed_tokens = nullptr, *embed_positions = nullptr, *ln_g = nullptr, *ln_b = nullptr;       // the decoder's embeddings and final LayerNorm
  bool allocated = false, dirty = true;
};

namespace us {
namespace {

void wh_keys(us_whisper* h) {
  const auto& c = h->cfg;
  const int H = c.d_model;
  auto affine = [&](const std::string& p) {
    h->add(p + ".weight", {H});
    h->add(p + ".bias", {H});
  };
  auto linear = [&](const std::string& p, int out, int in, bool bias = true) {
    h->add(p + ".weight", {out, in});
    if (bias) h->add(p + ".bias", {out});
  };
  auto attn = [&](const std::string& p) {
    linear(p + ".k_proj", H, H, false);
    linear(p + ".v_proj", H, H);
    linear(p + ".q_proj", H, H);
    linear(p + ".out_proj", H, H);
  };
  h->add("model.encoder.conv1.weight", {H, c.n_mels, 3});
  h->add("model.encoder.conv1.bias", {H});
  h->add("model.encoder.conv2.weight", {H, H, 3});
  h->add("model.encoder.conv2.bias", {H});
  h->add("model.encoder.embed_positions.weight", {c.max_source_positions, H});
  for (int i = 0; i < c.encoder_layers; ++i) {
    const std::string p = "model.encoder.layers." + std::to_string(i);
    attn(p + ".self_attn");
    affine(p + ".self_attn_layer_norm");
    linear(p + ".fc1", c.encoder_ffn, H);
    linear(p + ".fc2", H, c.encoder_ffn);
    affine(p + ".final_layer_norm");
  }
  affine("model.encoder.layer_norm");
  h->add("model.decoder.embed_tokens.weight", {c.vocab_size, H});
  h->add("model.decoder.embed_positions.weight", {c.max_target_positions, H});
  for (int i = 0; i < c.decoder_layers; ++i) {
    const std::string p = "model.decoder.layers." + std::to_string(i);
    attn(p + ".self_attn");
    affine(p + ".self_attn_layer_norm");
    attn(p + ".encoder_attn");
    affine(p + ".encoder_attn_layer_norm");
    linear(p + ".fc1", c.decoder_ffn, H);
    linear(p + ".fc2", H, c.decoder_ffn);
    affine(p + ".final_layer_norm");
  }
  affine("model.decoder.layer_norm");
}

hipError_t wh_alloc(us_whisper* h) {
  hipError_t e = hipSuccess;
  for (auto& kv : h->w)
    if (e == hipSuccess && !kv.second.dev) e = hipMalloc(&kv.second.dev, std::max<size_t>(kv.second.numel(), 1) * sizeof(float));
  if (e == hipSuccess) e = wh_encoder_alloc(h->enc);
  h->allocated = e == hipSuccess;
  return e;
}

hipError_t wh_prepare(us_whisper* h, hipStream_t s) {
  auto W = [&](const std::string& k) { return (const float*)h->w.at(k).dev; };
  h->dec.resize(h->cfg.decoder_layers);
  for (int i = 0; i < h->cfg.decoder_layers; ++i) {
    const std::string p = "model.decoder.layers." + std::to_string(i) + ".";
    WhDecLayer& l = h->dec[i];
    l.ln1_g = W(p + "self_attn_layer_norm.weight"); l.ln1_b = W(p + "self_attn_layer_norm.bias");
    l.ln2_g = W(p + "encoder_attn_layer_norm.weight"); l.ln2_b = W(p + "encoder_attn_layer_norm.bias");
    l.ln3_g = W(p + "final_layer_norm.weight"); l.ln3_b = W(p + "final_layer_norm.bias");
    l.q = {W(p + "self_attn.q_proj.weight"), W(p + "self_attn.q_proj.bias")};
    l.k = {W(p + "self_attn.k_proj.weight"), nullptr};
    l.v = {W(p + "self_attn.v_proj.weight"), W(p + "self_attn.v_proj.bias")};
    l.o = {W(p + "self_attn.out_proj.weight"), W(p + "self_attn.out_proj.bias")};
    l.cq = {W(p + "encoder_attn.q_proj.weight"), W(p + "encoder_attn.q_proj.bias")};
    l.co = {W(p + "encoder_attn.out_proj.weight"), W(p + "encoder_attn.out_proj.bias")};
    l.fc1 = {W(p + "fc1.weight"), W(p + "fc1.bias")};
    l.fc2 = {W(p + "fc2.weight"), W(p + "fc2.bias")};
  }
  h->embed_tokens = W("model.decoder.embed_tokens.weight");
  h->embed_positions = W("model.decoder.embed_positions.weight");
  h->ln_g = W("model.decoder.layer_norm.weight");
  h->ln_b = W("model.decoder.layer_norm.bias");
  const hipError_t e = wh_encoder_prepare(h->enc, *h, s);
  if (e == hipSuccess) h->dirty = false;
  return e;
}

struct WhPlan {                 // float offsets into the aligned workspace
  size_t enc, planar, kv, cache, x, q, att, ff, logits, select, total;
};

WhPlan wh_plan(const us_whisper* h, int B) {
  const auto& c = h->cfg;
  WhPlan p{};
  WsTake take;
  const size_t H = (size_t)c.d_model, S = (size_t)c.max_source_positions;
  p.enc = take(wh_encoder_ws_floats(h->enc, B));
  p.planar = take((size_t)B * H * S);
  p.kv = take((size_t)c.decoder_layers * B * 2 * H * S);
  p.cache = take((size_t)c.decoder_layers * B * 2 * c.max_target_positions * H);
  p.x = take(kWhItems * H);
  p.q = take(kWhItems * H);
  p.att = take(kWhItems * H);
  p.ff = take((size_t)kWhItems * c.decoder_ffn);
  p.logits = take((size_t)kWhItems * c.vocab_size);
  p.select = take(wh_select_floats(c.vocab_size));       // the group's state, and the selection stage's partials
  p.total = take.total;
  return p;
}

size_t wh_workspace_bytes(const us_whisper* h, int B) { return wh_plan(h, B).total * sizeof(float) + 256; }

// the checks every computing entry point starts with, then the encoder: -> planar (and out), cross keys / values when `cross`
int wh_begin(us_whisper* h, const std::string& what, const float* feats, int B, int T, float* out, bool cross, void* ws, size_t ws_bytes,
             hipStream_t s) {
  if (!h || !feats || B <= 0) return WeightTable::fail(h, US_EINVAL, what + ": bad argument");
  const auto& c = h->cfg;
  if (T != 2 * c.max_source_positions)
    return h->fail(US_EINVAL, what + ": the features have " + std::to_string(T) + " frames, the model takes exactly 2 * max_source_positions = " +
                                  std::to_string(2 * c.max_source_positions));
  if (B > 65535) return h->fail(US_EINVAL, what + ": at most 65535 items");
  const int rc = h->all_loaded(what.c_str());
  if (rc != US_OK) return rc;
  if (!ws || ws_bytes < wh_workspace_bytes(h, B)) return h->fail(US_EWORKSPACE, what + ": workspace too small (us_whisper_workspace_bytes)");
  hipError_t e;
  if (h->dirty && (e = wh_prepare(h, s)) != hipSuccess) return h->hip((what + ": preparing the weights").c_str(), e);
  const WhPlan p = wh_plan(h, B);
  float* base = ws_align(ws);
  if ((e = wh_encoder_forward(h->enc, *h, feats, B, base + p.planar, out, base + p.enc, s)) != hipSuccess) return h->hip(what.c_str(), e);
  if (cross && (e = wh_encoder_cross_kv(h->enc, *h, base + p.planar, B, base + p.kv, s)) != hipSuccess) return h->hip(what.c_str(), e);
  return US_OK;
}

struct WhStep {                 // one group's buffers
  us_whisper* h;
  hipStream_t s;
  float *X, *Q, *ATT, *FF, *cache, *kv;        // cache / kv: the group's first row / item of layer 0
  int B, nb;                    // the items of the call (a layer of kv is B items), the rows of the group
  int cache_rows = 0, rpi = 1;  // rows of a layer of the self cache; rows per item: row m attends to the cross keys of item m / rpi
  const int* anc = nullptr;     // beam search: [rows][max_target_positions], the group row that holds each position's key (else the row's own)
};

void wh_gemm(const WhStep& t, const float* x, int K, const float* ln_g, const float* ln_b, const float* res, int N, int gelu, int nseg, const WhSeg* seg) {
  WhGemmArgs a{};
  a.x = x; a.ldx = K; a.ln_g = ln_g; a.ln_b = ln_b; a.res = res; a.M = t.nb; a.N = N; a.K = K; a.gelu = gelu;
  for (int i = 0; i < nseg; ++i) a.seg[i] = seg[i];
  hipLaunchKernelGGL(wh_gemm_kernel, dim3((N + 15) / 16, nseg), dim3(256), 0, t.s, a);
}

// the decoder layers at position `pos`: X holds the embedded rows on entry and the last layer's stream on return
void wh_layers(const WhStep& t, int pos) {
  const auto& c = t.h->cfg;
  const int H = c.d_model, I = c.decoder_ffn, Tm = c.max_target_positions, S = c.max_source_positions, d = H / c.decoder_heads;
  const float qs = 1.f / sqrtf((float)d);
  const long long cache_item = 2ll * Tm * H, kv_item = 2ll * H * S;
  for (int i = 0; i < c.decoder_layers; ++i) {
    const WhDecLayer& l = t.h->dec[i];
    float* cache = t.cache + (size_t)i * t.cache_rows * cache_item;
    const float* kv = t.kv + (size_t)i * t.B * kv_item;
    const WhSeg qkv[3] = {{l.q.w, l.q.b, t.Q, H, qs},
                          {l.k.w, nullptr, cache + (size_t)pos * H, cache_item, 1.f},
                          {l.v.w, l.v.b, cache + (size_t)(Tm + pos) * H, cache_item, 1.f}};
    wh_gemm(t, t.X, H, l.ln1_g, l.ln1_b, nullptr, H, 0, 3, qkv);
    if (t.anc) hipLaunchKernelGGL(wh_self_attn_kernel<true>, dim3(c.decoder_heads, t.nb), dim3(64), 0, t.s, t.Q, cache, t.ATT, t.anc, cache_item, Tm, H, d, pos + 1);
    else hipLaunchKernelGGL(wh_self_attn_kernel<false>, dim3(c.decoder_heads, t.nb), dim3(64), 0, t.s, t.Q, cache, t.ATT, t.anc, cache_item, Tm, H, d, pos + 1);
    const WhSeg o{l.o.w, l.o.b, t.X, H, 1.f};
    wh_gemm(t, t.ATT, H, nullptr, nullptr, t.X, H, 0, 1, &o);
    const WhSeg cq{l.cq.w, l.cq.b, t.Q, H, qs};
    wh_gemm(t, t.X, H, l.ln2_g, l.ln2_b, nullptr, H, 0, 1, &cq);
    hipLaunchKernelGGL(wh_cross_attn_kernel, dim3(c.decoder_heads, t.nb), dim3(64 * kWhCrossWaves), 0, t.s, t.Q, kv, t.ATT, kv_item, S, H, d, t.rpi);
    const WhSeg co{l.co.w, l.co.b, t.X, H, 1.f};
    wh_gemm(t, t.ATT, H, nullptr, nullptr, t.X, H, 0, 1, &co);
    const WhSeg f1{l.fc1.w, l.fc1.b, t.FF, I, 1.f};
    wh_gemm(t, t.X, H, l.ln3_g, l.ln3_b, nullptr, I, 1, 1, &f1);
    const WhSeg f2{l.fc2.w, l.fc2.b, t.X, H, 1.f};
    wh_gemm(t, t.FF, I, nullptr, nullptr, t.X, H, 0, 1, &f2);
  }
}


// logits of the rows in X: decoder.layer_norm, then the tied embedding; row m at y + m * ldy
void wh_logits(const WhStep& t, float* y, long long ldy) {
  const WhSeg sg{t.h->embed_tokens, nullptr, y, ldy, 1.f};
  wh_gemm(t, t.X, t.h->cfg.d_model, t.h->ln_g, t.h->ln_b, nullptr, t.h->cfg.vocab_size, 0, 1, &sg);
}

// position `pos` of a group through the embedding and the layers.  host: row m takes ids[b0 + m / rpi][pos] of the host's [B][P]; else cur[m]
void wh_position(const WhStep& t, const int64_t* ids, int P, int b0, int pos, const int* cur, bool host) {
  WhTokens f;
  for (int m = 0; m < kWhItems; ++m) f.id[m] = !host ? -1 : m < t.nb ? (int)ids[(size_t)(b0 + m / t.rpi) * P + pos] : 0;
  hipLaunchKernelGGL(wh_embed_kernel, dim3(t.nb), dim3(256), 0, t.s, t.h->embed_tokens, t.h->embed_positions, cur, f, t.X, t.h->cfg.d_model, pos);
  wh_layers(t, pos);
}

// the buffers of the group of nb rows, rpi per item, whose first item is b0.  cache: the group's rows of layer 0 in a self cache of cache_rows
// rows a layer, or null: the items' own rows of the plan's
WhStep wh_group(us_whisper* h, const WhPlan& p, float* base, float* cache, int cache_rows, int rpi, int B, int b0, int nb, hipStream_t s) {
  const auto& c = h->cfg;
  const size_t H = (size_t)c.d_model;
  return WhStep{h, s, base + p.x, base + p.q, base + p.att, base + p.ff, cache ? cache : base + p.cache + (size_t)b0 * 2 * c.max_target_positions * H,
                base + p.kv + (size_t)b0 * 2 * H * c.max_source_positions, B, nb, cache ? cache_rows : B, rpi, nullptr};
}

// rows of the largest launch group of B items at beam size n: floor(16 / n) whole items
inline int wh_beam_group_rows(int B, int n) { return std::min(B, kWhItems / n) * n; }

struct WhBeamPlan {             // float offsets behind wh_plan(h, B): the self cache of one group's rows, the group's beam state
  size_t cache, state, total;
};
WhBeamPlan wh_beam_plan(const us_whisper* h, int B, int n) {
  const auto& c = h->cfg;
  WhBeamPlan p{};
  WsTake take;
  take(wh_plan(h, B).total);
  p.cache = take((size_t)c.decoder_layers * wh_beam_group_rows(B, n) * 2 * c.max_target_positions * c.d_model);
  p.state = take(wh_beam_floats(c.vocab_size, c.max_target_positions, c.max_target_positions));
  p.total = take.total;
  return p;
}

// ---- the decoding walk --------------------------------------------------------------------------------------------------------------
// us_whisper_generate, us_whisper_decode and us_whisper_decode_beam are one walk over launch groups, prompt positions and steps; a policy
// names the five places where they differ.

struct WhPolicy {
  int rpi;                      // rows per item: a launch group is kWhItems / rpi whole items
  int *cur, *running;           // the state's [kWhItems] token each row embeds next, and its count of the group's items that have not ended
  const int* anc;               // null, or the ancestry tables [2][kWhItems][max_target_positions]: a step reads the one of its parity
  float* cache;                 // with anc: the self cache the groups' rows share, cache_rows rows a layer; null: every item has its own
  int cache_rows;
  std::function<void(int b0, int items)> init;         // the group's state, and what an item returns that chooses nothing
  std::function<void(const float* L, int b0, int items, int step, int pos)> select;       // the step's logits -> tokens, cur, running
  std::function<void(int b0, int items)> final;        // behind the group's last step, or empty
};
struct WhProbe {                // the no-speech probability: softmax(unfiltered logits)[token] behind the prompt's token sot -> out [B]; token < 0: none
  int token, sot;
  float* out;
};

// The prompt [B][P] but for its last token is teacher-forced (keys and values only); up to max_new steps follow, the first from the prompt's
// last token, the others from the token the selection chose.  The running count is read back every kWhPoll steps: the first error of that
// read stops the call with nothing launched behind it, else hipGetLastError() closes it.
hipError_t wh_walk(us_whisper* h, const WhPlan& p, float* base, const int64_t* prompt, int B, int P, int max_new, const WhProbe& probe,
                   const WhPolicy& pol, hipStream_t s) {
  const int V = h->cfg.vocab_size, Tm = h->cfg.max_target_positions, nc = wh_chunks(V), ipg = kWhItems / pol.rpi;
  const WhSelect sel = wh_select_carve(base + p.select);        // the probe's plain partials: they read neither the state nor the rules
  float* L = base + p.logits;
  for (int b0 = 0; b0 < B; b0 += ipg) {
    const int items = std::min(ipg, B - b0), M = items * pol.rpi;
    WhStep t = wh_group(h, p, base, pol.cache, pol.cache_rows, pol.rpi, B, b0, M, s);
    t.anc = pol.anc;
    pol.init(b0, items);
    auto probe_here = [&]() {                           // L holds the logits behind sot; an item's first row speaks for it
      hipLaunchKernelGGL(wh_select_partial_kernel, dim3(nc, M), dim3(256), 0, s, L, nullptr, nullptr, sel.st, WhRules{}, sel.part, V, nc, 1);
      hipLaunchKernelGGL(wh_nospeech_kernel, dim3(items), dim3(256), 0, s, sel.part, L, probe.out + b0, V, nc, probe.token, pol.rpi);
    };
    for (int pos = 0; pos + 1 < P; ++pos) {
      wh_position(t, prompt, P, b0, pos, pol.cur, true);
      if (probe.token >= 0 && pos == probe.sot) {
        wh_logits(t, L, V);
        probe_here();
      }
    }
    for (int step = 0; step < max_new; ++step) {
      const int pos = P - 1 + step;
      if (pol.anc) t.anc = pol.anc + (size_t)(step & 1) * kWhItems * Tm;
      wh_position(t, prompt, P, b0, pos, pol.cur, step == 0);
      wh_logits(t, L, V);
      if (step == 0 && probe.token >= 0 && pos == probe.sot) probe_here();
      pol.select(L, b0, items, step, pos);
      if ((step + 1) % kWhPoll == 0 && step + 1 < max_new) {
        int running = 1;
        hipError_t e = hipMemcpyAsync(&running, pol.running, sizeof(int), hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return e;
        if (running <= 0) break;
      }
    }
    if (pol.final) pol.final(b0, items);
  }
  return hipGetLastError();
}

// ---- refusals: "" or the text -------------------------------------------------------------------------------------------------------

std::string wh_bad_token(const std::string& what, const int64_t* ids, size_t n, int V) {
  for (size_t i = 0; i < n; ++i)
    if (ids[i] < 0 || ids[i] >= V)
      return what + ": token " + std::to_string((long long)ids[i]) + " at index " + std::to_string(i) + " lies outside the vocabulary [0, " +
             std::to_string(V) + ")";
  return std::string();
}

std::string wh_bad_span(const std::string& what, int P, int max_new, int Tm) {
  if (P >= 1 && max_new >= 1 && (long long)P + max_new <= Tm) return std::string();
  return what + ": a prompt of " + std::to_string(P) + " and " + std::to_string(max_new) +
         " new tokens need P >= 1, max_new >= 1 and P + max_new <= max_target_positions = " + std::to_string(Tm);
}

// what the selection rules ask of the options and a vocabulary of V tokens
std::string wh_bad_rules(const std::string& what, const us_whisper_decode_options& o, int V) {
  if (V < 1 || V > (1 << 24)) return what + ": V must lie in [1, 2^24]";
  if (o.eos < 0 || o.eos >= o.no_timestamps)
    return what + ": eos = " + std::to_string(o.eos) + " must lie in [0, no_timestamps = " + std::to_string(o.no_timestamps) + ")";
  if ((long long)o.no_timestamps + 1 >= V)
    return what + ": no_timestamps + 1 = " + std::to_string((long long)o.no_timestamps + 1) + " >= vocab_size = " + std::to_string(V) +
           ": the vocabulary has no timestamp token";
  if (o.max_initial_timestamp_index < -1) return what + ": max_initial_timestamp_index must be -1 (none) or an index";
  return std::string();
}

// the options and the prompt of us_whisper_decode and us_whisper_decode_beam
std::string wh_bad_decode(const std::string& what, const us_whisper_config& c, const us_whisper_decode_options& o, const int64_t* prompt, int B, int P,
                          const float* no_speech_prob) {
  std::string bad = wh_bad_span(what, P, o.max_new, c.max_target_positions);
  if (bad.empty()) bad = wh_bad_rules(what, o, c.vocab_size);
  if (!bad.empty()) return bad;
  if (o.no_speech < -1 || o.no_speech >= c.vocab_size) return what + ": no_speech lies outside the vocabulary (-1: none)";
  if (o.no_speech >= 0 && !no_speech_prob) return what + ": a no_speech token needs no_speech_prob";
  if (o.sot_index < 0 || o.sot_index >= P) return what + ": sot_index = " + std::to_string(o.sot_index) + " lies outside the prompt of " + std::to_string(P);
  return wh_bad_token(what, prompt, (size_t)B * P, c.vocab_size);
}

std::string wh_bad_history(const std::string& what, const us_whisper_history* history, long long rows) {
  for (long long m = 0; m < rows; ++m)
    if (history[m].n_sampled < 0) return what + ": history[" + std::to_string(m) + "].n_sampled is negative";
  return std::string();
}

// the host's histories of a group's `rows` rows as the kernels take them; a slot past the group repeats its last row
WhHistory wh_history(const us_whisper_history* history, int rows, int tb) {
  WhHistory g{};
  for (int m = 0; m < kWhItems; ++m) {
    const us_whisper_history& h = history[std::min(m, rows - 1)];
    g.count[m] = h.n_sampled;
    g.last[m] = h.n_sampled >= 1 ? h.last : -1;
    g.pen[m] = h.n_sampled >= 2 ? h.penultimate : -1;
    g.last_ts[m] = h.last_timestamp >= tb ? h.last_timestamp : -1;
    g.done[m] = h.done != 0;
  }
  return g;
}

}  // namespace
}  // namespace us

extern "C" {

using namespace us;

int us_whisper_create(us_whisper_handle* out, const us_whisper_config* cfg) {
  if (!out || !cfg) return WeightTable::fail(nullptr, US_EINVAL, "us_whisper_create: null argument");
  const auto& c = *cfg;
  auto bad = [](const std::string& m) { return WeightTable::fail(nullptr, US_EINVAL, "us_whisper_create: " + m); };
  if (c.n_mels < 1 || c.n_mels > 1024 || c.d_model < 4 || c.d_model > 8192 || c.vocab_size < 1 || c.vocab_size > (1 << 24)) return bad("bad n_mels / d_model / vocab_size");
  if (c.encoder_layers < 0 || c.encoder_layers > 64 || c.decoder_layers < 1 || c.decoder_layers > 64) return bad("0 to 64 encoder layers, 1 to 64 decoder layers");
  if (c.encoder_ffn < 4 || c.decoder_ffn < 4 || c.encoder_ffn > 32768 || c.decoder_ffn > 32768 || c.decoder_ffn % 4 != 0)
    return bad("the feed-forward sizes must lie in [4, 32768], the decoder's a multiple of 4");
  if (c.max_source_positions < 1 || c.max_source_positions > kWhMaxKeys || c.max_target_positions < 1 || c.max_target_positions > kWhMaxKeys)
    return bad("max_source_positions and max_target_positions must lie in [1, " + std::to_string(kWhMaxKeys) + "]");
  for (int heads : {c.encoder_heads, c.decoder_heads}) {
    if (heads < 1 || c.d_model % heads != 0) return bad("d_model must be divisible by the number of heads");
    const int d = c.d_model / heads;
    if (d > 64 || d % 4 != 0) return bad("the head dimension must be a multiple of 4, at most 64 (got " + std::to_string(d) + ")");
  }
  auto* h = new us_whisper();
  h->cfg = c;
  (void)hipGetDevice(&h->device);
  h->enc = wh_encoder_new({c.n_mels, c.d_model, c.encoder_heads, c.encoder_ffn, c.encoder_layers, c.max_source_positions, c.decoder_layers});
  wh_keys(h);
  *out = h;
  return US_OK;
}

int us_whisper_destroy(us_whisper_handle h) {
  if (!h) return US_OK;
  h->free_weights();
  wh_encoder_free(h->enc);
  delete h;
  return US_OK;
}

int us_whisper_num_weights(us_whisper_handle h) { return h ? h->num() : 0; }
const char* us_whisper_weight_key(us_whisper_handle h, int i) { return h ? h->key(i) : nullptr; }
const char* us_whisper_last_error(us_whisper_handle h) { return h ? h->last_error() : us_last_error(nullptr); }

int us_whisper_load_weight(us_whisper_handle h, const char* key, const float* data, const int64_t* shape, int ndim, us_stream stream) {
  Weight* w;
  int rc = WeightTable::find(h, "us_whisper_load_weight", key, data, shape, ndim, &w);
  if (rc != US_OK) return rc;
  hipError_t e;
  if (!h->allocated && (e = wh_alloc(h)) != hipSuccess) return h->hip("us_whisper_load_weight: hipMalloc", e);
  if ((rc = h->copy(*w, data, static_cast<hipStream_t>(stream))) != US_OK) return rc;
  w->loaded = true;
  h->dirty = true;
  return US_OK;
}

size_t us_whisper_workspace_bytes(us_whisper_handle h, int B) { return h && B > 0 && B <= 65535 ? wh_workspace_bytes(h, B) : 0; }

size_t us_whisper_beam_workspace_bytes(us_whisper_handle h, int B, int beam_size) {
  return h && B > 0 && B <= 65535 && beam_size >= 1 && beam_size <= kWbMaxBeam ? wh_beam_plan(h, B, beam_size).total * sizeof(float) + 256 : 0;
}

size_t us_whisper_select_scratch_bytes(int V) { return V >= 1 && V <= (1 << 24) ? wh_select_floats(V) * sizeof(float) + 256 : 0; }

size_t us_whisper_beam_select_scratch_bytes(int V, int beam_size) {
  return V >= 1 && V <= (1 << 24) && beam_size >= 1 && beam_size <= kWbMaxBeam ? wh_beam_floats(V, 1, 2) * sizeof(float) + 256 : 0;
}

int us_whisper_encode(us_whisper_handle h, const float* features, int B, int T, float* out, void* workspace, size_t workspace_bytes, us_stream stream) {
  if (!out) return WeightTable::fail(h, US_EINVAL, "us_whisper_encode: bad argument");
  return wh_begin(h, "us_whisper_encode", features, B, T, out, false, workspace, workspace_bytes, static_cast<hipStream_t>(stream));
}

// Teacher forcing with the logits of every position and no step: not wh_walk, which takes logits inside the prompt for the probe alone and
// into the group's one buffer.
int us_whisper_decoder_logits(us_whisper_handle h, const float* features, int B, int T, const int64_t* ids, int N, float* logits, void* workspace,
                              size_t workspace_bytes, us_stream stream) {
  const std::string what = "us_whisper_decoder_logits";
  if (!h || !ids || !logits || B <= 0) return WeightTable::fail(h, US_EINVAL, what + ": bad argument");
  const auto& c = h->cfg;
  if (N < 1 || N > c.max_target_positions)
    return h->fail(US_EINVAL, what + ": " + std::to_string(N) + " positions, the model has max_target_positions = " + std::to_string(c.max_target_positions));
  const std::string bad = wh_bad_token(what, ids, (size_t)B * N, c.vocab_size);
  if (!bad.empty()) return h->fail(US_EINVAL, bad);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = wh_begin(h, what, features, B, T, nullptr, true, workspace, workspace_bytes, s);
  if (rc != US_OK) return rc;
  const WhPlan p = wh_plan(h, B);
  float* base = ws_align(workspace);
  for (int b0 = 0; b0 < B; b0 += kWhItems) {
    const WhStep t = wh_group(h, p, base, nullptr, 0, 1, B, b0, std::min(kWhItems, B - b0), s);
    for (int pos = 0; pos < N; ++pos) {
      wh_position(t, ids, N, b0, pos, nullptr, true);
      wh_logits(t, logits + ((size_t)b0 * N + pos) * c.vocab_size, (long long)N * c.vocab_size);
    }
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip(what.c_str(), e);
}

int us_whisper_generate(us_whisper_handle h, const float* features, int B, int T, const int64_t* prompt, int P, int max_new, int64_t eos,
                        const unsigned char* suppress, const unsigned char* begin_suppress, int64_t* tokens, int64_t* n, void* workspace,
                        size_t workspace_bytes, us_stream stream) {
  const std::string what = "us_whisper_generate";
  if (!h || !prompt || !tokens || !n || B <= 0) return WeightTable::fail(h, US_EINVAL, what + ": bad argument");
  const int V = h->cfg.vocab_size;
  std::string bad = wh_bad_span(what, P, max_new, h->cfg.max_target_positions);
  if (bad.empty() && (eos < 0 || eos >= V)) bad = what + ": eos lies outside the vocabulary";
  if (bad.empty()) bad = wh_bad_token(what, prompt, (size_t)B * P, V);
  if (!bad.empty()) return h->fail(US_EINVAL, bad);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = wh_begin(h, what, features, B, T, nullptr, true, workspace, workspace_bytes, s);
  if (rc != US_OK) return rc;
  const WhPlan p = wh_plan(h, B);
  float* base = ws_align(workspace);
  const WhDecState st = wh_select_carve(base + p.select).st;
  long long *tok = reinterpret_cast<long long*>(tokens), *cnt = reinterpret_cast<long long*>(n);
  WhPolicy pol{1, st.cur, st.running, nullptr, nullptr, 0};
  pol.init = [&](int b0, int items) {
    hipLaunchKernelGGL(wh_state_init_kernel, dim3(1), dim3(256), 0, s, st, WhHistory{}, 0, tok + (size_t)b0 * max_new, cnt + b0, nullptr, nullptr, nullptr,
                       items, max_new, (long long)eos);
  };
  pol.select = [&](const float* L, int b0, int items, int step, int) {
    hipLaunchKernelGGL(wh_argmax_kernel, dim3(items), dim3(256), 0, s, L, suppress, step == 0 ? begin_suppress : nullptr, st, tok + (size_t)b0 * max_new,
                       cnt + b0, V, max_new, step, (int)eos);
  };
  const hipError_t e = wh_walk(h, p, base, prompt, B, P, max_new, WhProbe{-1, 0, nullptr}, pol, s);
  return e == hipSuccess ? US_OK : h->hip(what.c_str(), e);
}

int us_whisper_select(const float* logits, int B, int V, const us_whisper_history* history, const us_whisper_decode_options* options,
                      const unsigned char* suppress, const unsigned char* begin_suppress, int64_t* token, float* logprob,
                      int32_t* decided_timestamp, void* scratch, size_t scratch_bytes, us_stream stream) {
  const std::string what = "us_whisper_select";
  auto refuse = [&](int code, const std::string& m) { return WeightTable::fail(nullptr, code, m); };
  if (!logits || !history || !options || !token || !logprob || !decided_timestamp || B < 1) return refuse(US_EINVAL, what + ": bad argument");
  const auto& o = *options;
  std::string bad = wh_bad_rules(what, o, V);
  if (!bad.empty()) return refuse(US_EINVAL, bad);
  if (!scratch || scratch_bytes < us_whisper_select_scratch_bytes(V)) return refuse(US_EWORKSPACE, what + ": scratch too small (us_whisper_select_scratch_bytes)");
  if (!(bad = wh_bad_history(what, history, B)).empty()) return refuse(US_EINVAL, bad);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const WhSelect c = wh_select_carve(ws_align(scratch));
  const WhRules r{o.eos, o.no_timestamps + 1, o.max_initial_timestamp_index};
  for (int b0 = 0; b0 < B; b0 += kWhItems) {
    const int nb = std::min(kWhItems, B - b0);
    long long* tok = reinterpret_cast<long long*>(token) + b0;
    hipLaunchKernelGGL(wh_state_init_kernel, dim3(1), dim3(256), 0, s, c.st, wh_history(history + b0, nb, r.tb), 1, tok, c.n, nullptr, logprob + b0,
                       decided_timestamp + b0, nb, 1, (long long)o.eos);
    wh_select_step(logits + (size_t)b0 * V, suppress, begin_suppress, c, r, tok, c.n, nullptr, logprob + b0, decided_timestamp + b0, V, nb, 1, 0, s);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : refuse(US_EHIP, what + ": " + hipGetErrorString(e));
}

int us_whisper_decode(us_whisper_handle h, const float* features, int B, int T, const int64_t* prompt, int P,
                      const us_whisper_decode_options* options, const unsigned char* suppress, const unsigned char* begin_suppress, int64_t* tokens,
                      int64_t* n, float* sum_logprobs, float* no_speech_prob, void* workspace, size_t workspace_bytes, us_stream stream) {
  const std::string what = "us_whisper_decode";
  if (!h || !prompt || !options || !tokens || !n || !sum_logprobs || B <= 0) return WeightTable::fail(h, US_EINVAL, what + ": bad argument");
  const auto& o = *options;
  const int V = h->cfg.vocab_size, max_new = o.max_new;
  const std::string bad = wh_bad_decode(what, h->cfg, o, prompt, B, P, no_speech_prob);
  if (!bad.empty()) return h->fail(US_EINVAL, bad);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = wh_begin(h, what, features, B, T, nullptr, true, workspace, workspace_bytes, s);
  if (rc != US_OK) return rc;
  const WhPlan p = wh_plan(h, B);
  float* base = ws_align(workspace);
  const WhSelect sel = wh_select_carve(base + p.select);
  const WhRules r{o.eos, o.no_timestamps + 1, o.max_initial_timestamp_index};
  long long *tok = reinterpret_cast<long long*>(tokens), *cnt = reinterpret_cast<long long*>(n);
  WhPolicy pol{1, sel.st.cur, sel.st.running, nullptr, nullptr, 0};
  pol.init = [&](int b0, int items) {
    hipLaunchKernelGGL(wh_state_init_kernel, dim3(1), dim3(256), 0, s, sel.st, WhHistory{}, 0, tok + (size_t)b0 * max_new, cnt + b0, sum_logprobs + b0,
                       nullptr, nullptr, items, max_new, (long long)o.eos);
  };
  pol.select = [&](const float* L, int b0, int items, int step, int) {
    wh_select_step(L, suppress, begin_suppress, sel, r, tok + (size_t)b0 * max_new, cnt + b0, sum_logprobs + b0, nullptr, nullptr, V, items, max_new, step, s);
  };
  const hipError_t e = wh_walk(h, p, base, prompt, B, P, max_new, WhProbe{o.no_speech, o.sot_index, no_speech_prob}, pol, s);
  return e == hipSuccess ? US_OK : h->hip(what.c_str(), e);
}

int us_whisper_beam_select(const float* logits, int B, int V, int beam_size, const us_whisper_history* history, const double* scores,
                           const us_whisper_decode_options* options, const unsigned char* suppress, const unsigned char* begin_suppress,
                           int32_t* parent, int64_t* token, double* score, int32_t* n_live, int32_t* fin_parent, double* fin_score, int32_t* n_fin,
                           void* scratch, size_t scratch_bytes, us_stream stream) {
  const std::string what = "us_whisper_beam_select";
  auto refuse = [&](int code, const std::string& m) { return WeightTable::fail(nullptr, code, m); };
  if (!logits || !history || !scores || !options || !parent || !token || !score || !n_live || !fin_parent || !fin_score || !n_fin || B < 1)
    return refuse(US_EINVAL, what + ": bad argument");
  const auto& o = *options;
  const int n = beam_size;
  if (n < 1 || n > kWbMaxBeam) return refuse(US_EINVAL, what + ": beam_size must lie in [1, " + std::to_string(kWbMaxBeam) + "]");
  std::string bad = wh_bad_rules(what, o, V);
  if (!bad.empty()) return refuse(US_EINVAL, bad);
  if (!scratch || scratch_bytes < us_whisper_beam_select_scratch_bytes(V, n))
    return refuse(US_EWORKSPACE, what + ": scratch too small (us_whisper_beam_select_scratch_bytes)");
  if (!(bad = wh_bad_history(what, history, (long long)B * n)).empty()) return refuse(US_EINVAL, bad);
  hipStream_t s = static_cast<hipStream_t>(stream);
  const WhBeamState st = wh_beam_carve(ws_align(scratch), V, 1, 2);
  const WhRules r{o.eos, o.no_timestamps + 1, o.max_initial_timestamp_index};
  for (int b0 = 0, ipg = kWhItems / n; b0 < B; b0 += ipg) {
    const int items = std::min(ipg, B - b0);
    const size_t m0 = (size_t)b0 * n;
    WhBeamHist hist{wh_history(history + m0, items * n, r.tb), {}};
    for (int m = 0; m < items * n; ++m) hist.score[m] = scores[m0 + m];
    const WhBeamOut out{parent + m0, reinterpret_cast<long long*>(token) + m0, score + m0, n_live + b0, fin_parent + m0, fin_score + m0, n_fin + b0};
    hipLaunchKernelGGL(wh_beam_init_kernel, dim3(1), dim3(256), 0, s, st, hist, 1, n, items, o.eos, 1, 2);
    wh_beam_step(logits + m0 * V, suppress, begin_suppress, st, r, out, V, n, kWbMaxPool, items, 0, 0, 1, 2, 0, s);
  }
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : refuse(US_EHIP, what + ": " + hipGetErrorString(e));
}

int us_whisper_decode_beam(us_whisper_handle h, const float* features, int B, int T, const int64_t* prompt, int P,
                           const us_whisper_decode_options* options, int beam_size, int max_candidates, const unsigned char* suppress,
                           const unsigned char* begin_suppress, int64_t* tokens, int64_t* n, float* sum_logprobs, float* no_speech_prob,
                           void* workspace, size_t workspace_bytes, us_stream stream) {
  const std::string what = "us_whisper_decode_beam";
  if (!h || !prompt || !options || !tokens || !n || !sum_logprobs || B <= 0) return WeightTable::fail(h, US_EINVAL, what + ": bad argument");
  const auto& o = *options;
  const int V = h->cfg.vocab_size, max_new = o.max_new, nb = beam_size, C = max_candidates, Tm = h->cfg.max_target_positions;
  if (nb < 1 || nb > kWbMaxBeam)
    return h->fail(US_EINVAL, what + ": beam_size = " + std::to_string(nb) + " must lie in [1, " + std::to_string(kWbMaxBeam) + "]");
  if (C < 1 || C > kWbMaxPool)
    return h->fail(US_EINVAL, what + ": max_candidates = " + std::to_string(C) + " must lie in [1, " + std::to_string(kWbMaxPool) + "]");
  const std::string bad = wh_bad_decode(what, h->cfg, o, prompt, B, P, no_speech_prob);
  if (!bad.empty()) return h->fail(US_EINVAL, bad);
  if (B > 65535) return h->fail(US_EINVAL, what + ": at most 65535 items");
  if (!workspace || workspace_bytes < us_whisper_beam_workspace_bytes(h, B, nb))
    return h->fail(US_EINVAL, what + ": workspace too small (us_whisper_beam_workspace_bytes)");
  hipStream_t s = static_cast<hipStream_t>(stream);
  const int rc = wh_begin(h, what, features, B, T, nullptr, true, workspace, workspace_bytes, s);
  if (rc != US_OK) return rc;
  const WhPlan p = wh_plan(h, B);
  const WhBeamPlan bp = wh_beam_plan(h, B, nb);
  float* base = ws_align(workspace);
  const WhBeamState st = wh_beam_carve(base + bp.state, V, Tm, Tm);
  const WhRules r{o.eos, o.no_timestamps + 1, o.max_initial_timestamp_index};
  long long *tok = reinterpret_cast<long long*>(tokens), *cnt = reinterpret_cast<long long*>(n);
  WhPolicy pol{nb, st.cur, st.running, st.anc, base + bp.cache, wh_beam_group_rows(B, nb)};
  pol.init = [&](int, int items) { hipLaunchKernelGGL(wh_beam_init_kernel, dim3(1), dim3(256), 0, s, st, WhBeamHist{}, 0, nb, items, o.eos, Tm, Tm); };
  pol.select = [&](const float* L, int, int items, int step, int pos) {
    wh_beam_step(L, suppress, begin_suppress, st, r, WhBeamOut{}, V, nb, C, items, step, pos, Tm, Tm, 1, s);
  };
  pol.final = [&](int b0, int items) {
    hipLaunchKernelGGL(wh_beam_final_kernel, dim3(items), dim3(256), 0, s, st, tok + (size_t)b0 * max_new, cnt + b0, sum_logprobs + b0, nb, Tm, max_new, o.eos);
  };
  const hipError_t e = wh_walk(h, p, base, prompt, B, P, max_new, WhProbe{o.no_speech, o.sot_index, no_speech_prob}, pol, s);
  return e == hipSuccess ? US_OK : h->hip(what.c_str(), e);
}

}  // extern "C"
