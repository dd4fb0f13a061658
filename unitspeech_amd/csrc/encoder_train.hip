// Training side of the text / unit `Encoder` (unitspeech/encoder.py:253-308 in train mode): a forward with every Dropout of
// the reference, and the backward to every state_dict key.  The forward's schedule and its embedding, LayerNorm, attention and
// layout kernels are frontend.hip's (encoder_forward in training mode); this file holds its convolution, the tape and the backward.
//
// Layout: activations channel-last [B][L][C] (row = b * L + l), as in frontend.hip.  Every convolution (the prenet's k = 5,
// the FFN's k = kernel_size, the 1x1 q / k / v / o / proj / proj_m) is one implicit GEMM on the fp32 matrix cores
// (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation), in three forms:
//   forward  out[row][n]  = sum_{tap, ci} in[row + tap - pad][ci] * W[tap][ci][n]      (rows outside the item read 0)
//   dgrad    the forward form with the tap-flipped, transposed weight Wd[tap][co][ci] = w[co][ci][K - 1 - tap]
//   wgrad    dW[tap][ci][co] = sum_rows in[row + tap - pad][ci] * dout[row][co], split over row ranges into partial sums that
//            a second kernel adds in a fixed order (no atomics: the result is deterministic)
// Bias, LayerNorm and relative-embedding gradients are column sums of the same two-pass fixed-order kind; the embedding
// gradient is one workgroup per vocabulary row that walks the rows in order.  So the whole backward is deterministic.
//
// Dropout (torch.nn.Dropout: keep with probability 1 - p, kept values times 1 / (1 - p)) draws its keep bit from Philox4x32-10
// (the generator of us_fill_normal) keyed by the seed, with counter (flat element index / 4, site): element e of a site uses
// word e % 4 of the block e / 4.  The flat index is that of the reference's tensor ([B][C][L] activations, [B][H][L][L]
// attention probabilities), so a mask does not depend on launch geometry or on the library's layout, and the backward
// regenerates it instead of storing it.  Sites: 0..2 the prenet's relu_drop (p = 0.5); for transformer layer i, 3 + 4i the
// attention probabilities, 4 + 4i EncoderModule.drop after attention, 5 + 4i the FFN's drop after the ReLU, 6 + 4i
// EncoderModule.drop after the FFN (p = p_dropout).  With p = 0 no random number is drawn.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"
#include "frontend.h"
#include "kernels.h"

namespace us {
namespace {

// ---- implicit-GEMM convolution on the fp32 matrix cores ----------------------------------------------------------------
constexpr int kBM = 64, kBN = 64, kBK = 16;

struct GemmArgs {
  const float* in;        // [rows][Cin]
  const float* mask;      // [rows]
  int mask_in;            // the input is read multiplied by mask (the reference's conv(x * x_mask))
  int rows, L, Cin, N, K, pad;
  // forward / dgrad form
  const float* w;         // [K][Cin][N]
  const float* bias;      // [N] or null
  const float* gate;      // [rows][N] or null: v = gate > 0 ? v * gate_scale : 0 (ReLU + dropout backward through the stored output)
  float gate_scale;
  const float* add;       // [rows][N] or null: added before the output mask (may alias out)
  float* out;             // [rows][N]
  int relu, mask_out;
  Drop drop;              // epilogue dropout after the ReLU, flat index of the [B][N][L] tensor
  // wgrad form
  const float* dout;      // [rows][N]
  float* part;            // [S][K][Cin][N]
  int rows_per_split, splits;
  // the Linear front of a ContentVec handle (kFront; K = 1, no bias): a row at or past its item's length is not read (it may
  // hold anything, NaN included) and counts as zeros
  const long long* lengths;   // [B], forward: which rows are read; the forward also writes mask_w[row] = row's frame < lengths[b]
  float* mask_w;              // [rows]
  float scale;                // forward: out = product * scale, rounded separately (encoder.py:295)
};

// Workgroup tile 64 x 64 of D, four waves of 32 x 32 (one 32x32x2 MFMA accumulator each), reduction slices of 16 staged in LDS
// through registers (the next slice is loaded while the current one is multiplied).
//   forward / dgrad:  D[row][n],  A(row, r = tap * Cin + ci) = in[row + tap - pad][ci],  B(r, n) = w[r][n]
//   wgrad:            D[ci][co] of tap blockIdx.z / splits,  A(ci, row) = in[row + tap - pad][ci],  B(row, co) = dout[row][co]
//   front (kFront): the forward form at K = 1 on in = feats, w = emb.weight packed [Cin][N]; its wgrad reads mask (the tape's) for
//   the rows it may read
template <bool kWgrad, bool kFront = false>
__global__ __launch_bounds__(256) void et_gemm_kernel(GemmArgs a) {
  __shared__ float As[2][kBK][kBM + 4];
  __shared__ float Bs[2][kBK][kBN + 4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = (wave & 1) * 32, wn = (wave >> 1) * 32;
  const int m0 = blockIdx.x * kBM, n0 = blockIdx.y * kBN;
  int tap = 0, split = 0, k_lo = 0, k_hi;
  if (kWgrad) {
    tap = blockIdx.z / a.splits;
    split = blockIdx.z - tap * a.splits;
    k_lo = split * a.rows_per_split;
    k_hi = min(a.rows, k_lo + a.rows_per_split);
  } else {
    k_hi = a.K * a.Cin;
  }
  float areg[4], breg[4];
  auto load = [&](int k0) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      float v = 0.f;
      if (kWgrad) {
        const int mm = e & 63, kk = e >> 6;
        const int row = k0 + kk, ci = m0 + mm;
        if (row < k_hi && ci < a.Cin) {
          const int b = row / a.L, t = row - b * a.L, tt = t + tap - a.pad;
          if (tt >= 0 && tt < a.L) {
            const long long src = (long long)row + tap - a.pad;
            if (kFront) {
              if (a.mask[src] != 0.f) v = a.in[src * a.Cin + ci];
            } else {
              v = a.in[src * a.Cin + ci];
              if (a.mask_in) v *= a.mask[src];
            }
          }
        }
      } else {
        const int kk = e & 15, mm = e >> 4;
        const int row = m0 + mm, r = k0 + kk;
        if (row < a.rows && r < k_hi) {
          const int tp = r / a.Cin, ci = r - tp * a.Cin;
          const int b = row / a.L, t = row - b * a.L, tt = t + tp - a.pad;
          if (tt >= 0 && tt < a.L) {
            const long long src = (long long)row + tp - a.pad;
            if (kFront) {
              if (t < a.lengths[b]) v = a.in[src * a.Cin + ci];
            } else {
              v = a.in[src * a.Cin + ci];
              if (a.mask_in) v *= a.mask[src];
            }
          }
        }
      }
      areg[i] = v;
      const int nn = e & 63, kk = e >> 6, n = n0 + nn, r = k0 + kk;
      float u = 0.f;
      if (n < a.N && r < k_hi) u = kWgrad ? a.dout[(long long)r * a.N + n] : a.w[(long long)r * a.N + n];
      breg[i] = u;
    }
  };
  auto store = [&](int buf) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int e = tid + 256 * i;
      if (kWgrad) As[buf][e >> 6][e & 63] = areg[i];
      else As[buf][e & 15][e >> 4] = areg[i];
      Bs[buf][e >> 6][e & 63] = breg[i];
    }
  };
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  const int kl = lane >> 5, cl = lane & 31;
  load(k_lo);
  store(0);
  __syncthreads();
  int cur = 0;
  for (int k0 = k_lo; k0 < k_hi; k0 += kBK) {
    const bool more = k0 + kBK < k_hi;
    if (more) load(k0 + kBK);
#pragma unroll
    for (int s = 0; s < kBK / 2; ++s) {
      const float fa = As[cur][2 * s + kl][wm + cl];
      const float fb = Bs[cur][2 * s + kl][wn + cl];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(fa, fb, acc, 0, 0, 0);
    }
    if (more) store(cur ^ 1);
    __syncthreads();
    cur ^= 1;
  }
  if (kFront && !kWgrad && blockIdx.y == 0 && tid < kBM && m0 + tid < a.rows) {      // x_mask, by the first column of workgroups
    const int row = m0 + tid, b = row / a.L;
    a.mask_w[row] = (long long)(row - b * a.L) < a.lengths[b] ? 1.f : 0.f;
  }
  const int n = n0 + wn + cl;
  if (n >= a.N) return;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm + mfma32_row(r, kl);
    if (kWgrad) {
      if (m < a.Cin) a.part[(((long long)split * a.K + tap) * a.Cin + m) * a.N + n] = acc[r];
      continue;
    }
    if (m >= a.rows) continue;
    const long long o = (long long)m * a.N + n;
    if (kFront) {      // product first, then the scale; a row past its length summed zeros
      a.out[o] = mul_rn(acc[r], a.scale);
      continue;
    }
    float v = acc[r];
    if (a.bias) v += a.bias[n];
    if (a.relu) v = v > 0.f ? v : 0.f;
    if (a.drop.site >= 0) v *= et_keep(a.drop, et_cf_index(m, n, a.N, a.L));
    if (a.gate) v = a.gate[o] > 0.f ? v * a.gate_scale : 0.f;
    if (a.add) v = a.add[o] + v;
    if (a.mask_out) v *= a.mask[m];
    a.out[o] = v;
  }
}

// grad[co][ci][tap] (torch layout) = scale * sum over splits, in order, of part[s][tap][ci][co]
__global__ void et_wgrad_finish_kernel(const float* part, float* grad, int S, int K, int Cin, int Cout, float scale) {
  const long long n = (long long)Cout * Cin * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int k = (int)(i % K);
    const long long r = i / K;
    const int ci = (int)(r % Cin), co = (int)(r / Cin);
    float s = 0.f;
    for (int sp = 0; sp < S; ++sp) s += part[(((long long)sp * K + k) * Cin + ci) * Cout + co];
    grad[i] = mul_rn(s, scale);
  }
}

// Wd[tap][co][ci] = w[co][ci][K - 1 - tap]: the dgrad weight, so that dgrad is the forward form
__global__ void et_pack_dgrad_kernel(const float* w, float* out, int Cout, int Cin, int K) {
  const long long n = (long long)Cout * Cin * K;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    const long long r = i / Cin;
    const int co = (int)(r % Cout), tap = (int)(r / Cout);
    out[i] = w[((long long)co * Cin + ci) * K + (K - 1 - tap)];
  }
}

// ---- column sums (bias / LayerNorm / relative-embedding gradients), two fixed-order passes --------------------------------
constexpr int kColChunks = 64;
// part[chunk][c] = sum over the chunk's rows of x[row][c] (4 row groups per workgroup, added in order)
__global__ __launch_bounds__(256) void et_colsum_kernel(const float* x, float* part, int rows, int N) {
  __shared__ float red[4][64];
  const int c = blockIdx.x * 64 + (threadIdx.x & 63), g = threadIdx.x >> 6;
  const int per = (rows + kColChunks - 1) / kColChunks;
  const int lo = blockIdx.y * per, hi = min(rows, lo + per);
  float s = 0.f;
  if (c < N)
    for (int r = lo + g; r < hi; r += 4) s += x[(long long)r * N + c];
  red[g][threadIdx.x & 63] = s;
  __syncthreads();
  if (g == 0 && c < N) part[(long long)blockIdx.y * N + c] = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) + red[3][threadIdx.x];
}
__global__ void et_colsum_finish_kernel(const float* part, float* out, int N, int chunks, float scale) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= N) return;
  float s = 0.f;
  for (int k = 0; k < chunks; ++k) s += part[(long long)k * N + c];
  out[c] = s * scale;
}

// ---- embedding gradient, layout --------------------------------------------------------------------------------------
// emb_grad[v][:] = scale * sum over rows (in order) with ids[row] == v of dx0[row][:]
__global__ __launch_bounds__(256) void et_embed_grad_kernel(const long long* ids, const float* dx0, float* grad, long long rows, int C,
                                                            float scale) {
  const int v = blockIdx.x;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  for (long long r = 0; r < rows; ++r) {
    if (ids[r] != v) continue;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int c = threadIdx.x + 256 * i;
      if (c < C) acc[i] += dx0[r * C + c];
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int c = threadIdx.x + 256 * i;
    if (c < C) grad[(long long)v * C + c] = acc[i] * scale;
  }
}

// channel-first [B][C][L] (the caller's gradients) -> channel-last [B][L][C], optionally times mask[b][l]
__global__ void et_to_channel_last_kernel(const float* in, const float* mask, float* out, int L, int C) {
  __shared__ float tile[32][33];
  const int b = blockIdx.z, l0 = blockIdx.x * 32, c0 = blockIdx.y * 32;
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    const int c = c0 + r, l = l0 + threadIdx.x;
    tile[threadIdx.x][r] = (l < L && c < C) ? in[((long long)b * C + c) * L + l] : 0.f;
  }
  __syncthreads();
  for (int r = threadIdx.y; r < 32; r += blockDim.y) {
    const int l = l0 + r, c = c0 + threadIdx.x;
    if (l < L && c < C) {
      float v = tile[r][threadIdx.x];
      if (mask) v *= mask[(long long)b * L + l];
      out[((long long)b * L + l) * C + c] = v;
    }
  }
}

// out[row][c] = in[row][c] * keep(site, (b, c, l)) * mask[row]
__global__ void et_drop_mask_kernel(const float* in, const float* mask, float* out, long long rows, int C, int L, Drop d) {
  const long long n = rows * C;
  for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
    const long long row = i / C;
    const int c = (int)(i - row * C);
    float v = in[i] * et_keep(d, et_cf_index(row, c, C, L));
    if (mask) v *= mask[row];
    out[i] = v;
  }
}

// ---- LayerNorm backward (eps 1e-4, encoder.py:21-30) -------------------------------------------------------------------
constexpr int kLnPerLane = 16;      // C <= 1024
// dx of y = LN(x) for upstream dy; with `gate` (the stored prenet output drop(relu(y))), dy is first taken through the dropout
// and the ReLU: dy = gate > 0 ? dy * gate_scale : 0.  dyx[row][c] = dy * xhat and dyo[row][c] = dy feed the gamma / beta sums.
struct LnBwdArgs {
  const float* x; const float* gamma;
  const float* dy; const float* gate; float gate_scale;
  float* dx; float* dyx; float* dyo;
  int C; float eps;
};
__global__ __launch_bounds__(64) void et_ln_bwd_kernel(LnBwdArgs a) {
  const long long row = blockIdx.x;
  const int lane = threadIdx.x;
  float v[kLnPerLane], g[kLnPerLane];
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < kLnPerLane; ++i) {
    const int c = lane + 64 * i;
    v[i] = 0.f;
    g[i] = 0.f;
    if (c < a.C) {
      v[i] = a.x[row * a.C + c];
      float d = a.dy[row * a.C + c];
      if (a.gate) d = a.gate[row * a.C + c] > 0.f ? d * a.gate_scale : 0.f;
      g[i] = d;
      s += v[i];
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
  const float mean = s / (float)a.C;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < kLnPerLane; ++i) {
    const int c = lane + 64 * i;
    if (c < a.C) { const float d = sub_rn(v[i], mean); q = __builtin_fmaf(d, d, q); }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) q += __shfl_xor(q, o, 64);
  const float rstd = 1.f / sqrtf(add_rn(q / (float)a.C, a.eps));
  float s1 = 0.f, s2 = 0.f;        // sum dxhat, sum dxhat * xhat
#pragma unroll
  for (int i = 0; i < kLnPerLane; ++i) {
    const int c = lane + 64 * i;
    if (c < a.C) {
      const float xh = (v[i] - mean) * rstd, dxh = g[i] * a.gamma[c];
      v[i] = xh;
      s1 += dxh;
      s2 += dxh * xh;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
  s1 /= (float)a.C;
  s2 /= (float)a.C;
#pragma unroll
  for (int i = 0; i < kLnPerLane; ++i) {
    const int c = lane + 64 * i;
    if (c < a.C) {
      const long long o = row * a.C + c;
      a.dx[o] = rstd * (g[i] * a.gamma[c] - s1 - v[i] * s2);
      a.dyx[o] = g[i] * v[i];
      a.dyo[o] = g[i];
    }
  }
}

// ---- relative-position self-attention backward (encoder.py:115-144; AttnArgs and the forward kernel: frontend.h / .hip) ------
// backward, one (query i, head, item): dpd[j] = dO_i.v_j (+ dO_i.rel_v[j-i+W] in the band), dp = dpd * keep,
// ds[j] = p[j] (dp[j] - sum_k p[k] dp[k]) (0 where the score was filled: no gradient flows through -1e4); dq_i from ds
__global__ void __launch_bounds__(128) et_attn_bwd_q_kernel(AttnArgs a) {
  extern __shared__ float sm[];          // g[L], dO[D], red[128]
  float* g = sm;
  float* dos = sm + a.L;
  float* red = dos + a.D;
  const int i = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const long long base = (long long)b * a.L * a.C + (long long)h * a.D;
  const long long prow = (((long long)b * a.H + h) * a.L + i) * a.L;
  for (int d = tid; d < a.D; d += blockDim.x) dos[d] = a.dO[base + (long long)i * a.C + d];
  __syncthreads();
  float s = 0.f;
  for (int j = tid; j < a.L; j += blockDim.x) {
    const float* vj = a.v + base + (long long)j * a.C;
    float t = 0.f;
    for (int d = 0; d < a.D; ++d) t = __builtin_fmaf(dos[d], vj[d], t);
    const int off = j - i;
    if (a.rel_v && off >= -a.W && off <= a.W) {
      const float* rv = a.rel_v + (long long)(off + a.W) * a.D;
      for (int d = 0; d < a.D; ++d) t = __builtin_fmaf(dos[d], rv[d], t);
    }
    const float pdp = a.P[prow + j] * (t * et_keep(a.drop, (unsigned long long)(prow + j)));
    g[j] = pdp;
    s += pdp;
  }
  red[tid] = s;
  __syncthreads();
  for (int o = 64; o > 0; o >>= 1) {
    if (tid < o) red[tid] += red[tid + o];
    __syncthreads();
  }
  s = red[0];
  const float mi = a.mask[(long long)b * a.L + i];
  for (int j = tid; j < a.L; j += blockDim.x) {
    const bool filled = mi * a.mask[(long long)b * a.L + j] == 0.f;
    const float ds = filled ? 0.f : g[j] - a.P[prow + j] * s;
    g[j] = ds;
    a.DS[prow + j] = ds;
  }
  __syncthreads();
  for (int d = tid; d < a.D; d += blockDim.x) {
    float t = 0.f;
    for (int j = 0; j < a.L; ++j) t = __builtin_fmaf(g[j], a.k[base + (long long)j * a.C + d], t);
    if (a.rel_k)
      for (int off = -a.W; off <= a.W; ++off) {
        const int j = i + off;
        if (j >= 0 && j < a.L) t = __builtin_fmaf(g[j], a.rel_k[(long long)(off + a.W) * a.D + d], t);
      }
    a.dq[base + (long long)i * a.C + d] = t / a.sqrt_d;
  }
}

// backward, one (key j, head, item): dv_j = sum_i pd[i][j] dO_i, dk_j = sum_i ds[i][j] q_i / sqrt(D)
__global__ void __launch_bounds__(128) et_attn_bwd_kv_kernel(AttnArgs a) {
  extern __shared__ float sm[];          // pd[L], ds[L]
  float* pd = sm;
  float* ds = sm + a.L;
  const int j = blockIdx.x, h = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
  const long long base = (long long)b * a.L * a.C + (long long)h * a.D;
  const long long pbase = ((long long)b * a.H + h) * a.L * a.L;
  for (int i = tid; i < a.L; i += blockDim.x) {
    const long long idx = pbase + (long long)i * a.L + j;
    pd[i] = a.P[idx] * et_keep(a.drop, (unsigned long long)idx);
    ds[i] = a.DS[idx];
  }
  __syncthreads();
  for (int d = tid; d < a.D; d += blockDim.x) {
    float tv = 0.f, tk = 0.f;
    for (int i = 0; i < a.L; ++i) {
      tv = __builtin_fmaf(pd[i], a.dO[base + (long long)i * a.C + d], tv);
      tk = __builtin_fmaf(ds[i], a.q[base + (long long)i * a.C + d], tk);
    }
    a.dv[base + (long long)j * a.C + d] = tv;
    a.dk[base + (long long)j * a.C + d] = tk / a.sqrt_d;
  }
}

// per item b and offset: rel_part[0][b][off][d] = sum_{h, i} pd[i][i+off] dO_i[hD+d],  rel_part[1][b][off][d] = sum_{h, i}
// ds[i][i+off] q_i[hD+d] (heads share the embeddings, encoder.py:86-92); the item sums are added in order by the finish kernel
__global__ void __launch_bounds__(128) et_attn_bwd_rel_kernel(AttnArgs a) {
  const int oi = blockIdx.x, off = oi - a.W, b = blockIdx.y, nw = 2 * a.W + 1;
  const int i0 = off < 0 ? -off : 0, i1 = off > 0 ? a.L - off : a.L;
  for (int d = threadIdx.x; d < a.D; d += blockDim.x) {
    double sv = 0.0, sk = 0.0;      // H * L terms per item that largely cancel: fp64 sums keep fp32 products' accuracy
    for (int h = 0; h < a.H; ++h) {
      const long long base = (long long)b * a.L * a.C + (long long)h * a.D + d;
      const long long pbase = ((long long)b * a.H + h) * a.L * a.L;
      for (int i = i0; i < i1; ++i) {
        const long long idx = pbase + (long long)i * a.L + (i + off);
        sv += (double)(a.P[idx] * et_keep(a.drop, (unsigned long long)idx)) * a.dO[base + (long long)i * a.C];
        sk += (double)a.DS[idx] * a.q[base + (long long)i * a.C];
      }
    }
    const long long B = gridDim.y;
    a.rel_part[((long long)b * nw + oi) * a.D + d] = sv;
    a.rel_part[((B + b) * nw + oi) * a.D + d] = sk;
  }
}

__global__ void et_rel_finish_kernel(const double* part, float* grad_v, float* grad_k, int B, int n, float inv_sqrt_d) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  double sv = 0.0, sk = 0.0;
  for (int b = 0; b < B; ++b) {
    sv += part[(long long)b * n + e];
    sk += part[((long long)B + b) * n + e];
  }
  grad_v[e] = (float)sv;
  grad_k[e] = (float)(sk * inv_sqrt_d);
}

// ---- host side ---------------------------------------------------------------------------------------------------------

unsigned et_blocks(long long n, int threads) {
  const long long b = (n + threads - 1) / threads;
  return (unsigned)(b < 1 ? 1 : (b > 4096 ? 4096 : b));
}

// workspace layout of one training forward (the tape) and of its backward, in floats from a 256-byte aligned base
struct Layout {
  size_t ids, mask, x0, pc[kPrenetLayers], pa[kPrenetLayers], mu, xf;
  std::vector<size_t> x, q, k, v, at, n1, x1, n2, hd, p;        // per transformer layer
  size_t tape_end;
  size_t g, t, d1, dh, dyx, dyo, dq, dk, dv, ds, wd, wpart, cpart, rpart, arena;
  int splits;
  size_t total;
};

size_t conv_numel(const us_frontend* h) {      // largest convolution weight (the Linear front counts as one)
  const us_encoder_config& c = h->ec;
  size_t m = (size_t)c.n_channels * c.n_channels * kPrenetKernel;
  m = std::max(m, (size_t)c.n_channels * h->n_contentvec);
  m = std::max(m, (size_t)c.filter_channels * c.n_channels * c.kernel_size);
  m = std::max(m, (size_t)c.n_feats * c.n_channels);
  return m;
}

Layout et_layout(const us_frontend* h, int B, int L) {
  const auto& c = h->ec;
  const size_t rows = (size_t)B * L, C = c.n_channels, F = c.filter_channels, H = c.n_heads;
  const size_t plane = rows * C, att = (size_t)B * H * L * L;
  Layout o{};
  WsTake take;
  o.ids = take(2 * rows);
  o.mask = take(rows);
  o.x0 = take(plane);
  for (int i = 0; i < kPrenetLayers; ++i) o.pc[i] = take(plane);
  for (int i = 0; i < kPrenetLayers; ++i) o.pa[i] = take(plane);
  for (int i = 0; i < c.n_layers; ++i) {
    o.x.push_back(take(plane)); o.q.push_back(take(plane)); o.k.push_back(take(plane)); o.v.push_back(take(plane));
    o.at.push_back(take(plane)); o.n1.push_back(take(plane)); o.x1.push_back(take(plane)); o.n2.push_back(take(plane));
    o.hd.push_back(take(rows * F)); o.p.push_back(take(att));
  }
  o.xf = take(plane);
  o.mu = take(rows * c.n_feats);
  o.tape_end = take.total;
  const size_t wide = rows * std::max(std::max(C, F), (size_t)c.n_feats);
  o.g = take(plane); o.t = take(plane); o.d1 = take(wide); o.dh = take(wide); o.dyx = take(plane); o.dyo = take(plane);
  o.dq = take(plane); o.dk = take(plane); o.dv = take(plane); o.ds = take(att);
  o.splits = wgrad_splits((long long)rows);
  o.wd = take(conv_numel(h));
  o.wpart = take((size_t)o.splits * conv_numel(h));
  o.cpart = take((size_t)kColChunks * std::max(std::max(C, F), (size_t)c.n_feats));
  const size_t nw = 2 * (size_t)c.window_size + 1, D = C / H;
  o.rpart = take(4 * (size_t)B * nw * D);      // doubles
  o.arena = take(h->total_numel());
  o.total = take.total;
  return o;
}

struct Ctx {
  us_frontend* h;
  hipStream_t s;
  float* base;
  const Layout* lay;
  int B, L;
  long long rows;
  float* mask;
  float* f(size_t off) const { return base + off; }
};

const float* wdev(us_frontend* h, const std::string& k) { return h->w[k].dev; }

// din = (add + dgrad(dout)) [gated] [* mask]; dW, db of the convolution `key` whose forward input was `in` (read times mask when
// mask_in); dw / db are the destinations in torch layout
void conv_bwd(const Ctx& x, const std::string& key, const float* in, bool mask_in, const float* dout, float* din, const float* add,
              const float* gate, float gate_scale, bool mask_out, float* dw, float* db) {
  const int Cout = (int)x.h->w[key + ".weight"].shape[0];
  const Layout& l = *x.lay;
  gemm_conv_wgrad(x.h, x.s, key, in, x.mask, mask_in, dout, x.rows, x.L, x.f(l.wpart), dw);
  // bias gradient
  hipLaunchKernelGGL(et_colsum_kernel, dim3((Cout + 63) / 64, kColChunks), dim3(256), 0, x.s, dout, x.f(l.cpart), (int)x.rows, Cout);
  hipLaunchKernelGGL(et_colsum_finish_kernel, dim3((Cout + 255) / 256), dim3(256), 0, x.s, x.f(l.cpart), db, Cout, kColChunks, 1.f);
  if (din) gemm_conv_dgrad(x.h, x.s, key, dout, din, x.mask, add, gate, gate_scale, mask_out, x.rows, x.L, x.f(l.wd));
}

void ln_bwd(const Ctx& x, const std::string& key, const float* in, const float* dy, const float* gate, float gate_scale, float* dx,
            float* dgamma, float* dbeta) {
  const Layout& l = *x.lay;
  const int C = x.h->ec.n_channels;
  LnBwdArgs a{};
  a.x = in; a.gamma = wdev(x.h, key + ".gamma"); a.dy = dy; a.gate = gate; a.gate_scale = gate_scale;
  a.dx = dx; a.dyx = x.f(l.dyx); a.dyo = x.f(l.dyo); a.C = C; a.eps = 1e-4f;
  hipLaunchKernelGGL(et_ln_bwd_kernel, dim3((unsigned)x.rows), dim3(64), 0, x.s, a);
  hipLaunchKernelGGL(et_colsum_kernel, dim3((C + 63) / 64, kColChunks), dim3(256), 0, x.s, x.f(l.dyx), x.f(l.cpart), (int)x.rows, C);
  hipLaunchKernelGGL(et_colsum_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, x.s, x.f(l.cpart), dgamma, C, kColChunks, 1.f);
  hipLaunchKernelGGL(et_colsum_kernel, dim3((C + 63) / 64, kColChunks), dim3(256), 0, x.s, x.f(l.dyo), x.f(l.cpart), (int)x.rows, C);
  hipLaunchKernelGGL(et_colsum_finish_kernel, dim3((C + 255) / 256), dim3(256), 0, x.s, x.f(l.cpart), dbeta, C, kColChunks, 1.f);
}

AttnArgs attn_args(const Ctx& x, int i) {
  const auto& c = x.h->ec;
  const Layout& l = *x.lay;
  const std::string ap = "encoder.attn_layers." + std::to_string(i);
  AttnArgs a{};
  a.q = x.f(l.q[i]); a.k = x.f(l.k[i]); a.v = x.f(l.v[i]); a.mask = x.mask; a.P = x.f(l.p[i]); a.out = x.f(l.at[i]);
  a.rel_k = c.window_size > 0 ? wdev(x.h, ap + ".emb_rel_k") : nullptr;
  a.rel_v = c.window_size > 0 ? wdev(x.h, ap + ".emb_rel_v") : nullptr;
  a.L = x.L; a.C = c.n_channels; a.H = c.n_heads; a.D = c.n_channels / c.n_heads; a.W = c.window_size;
  a.sqrt_d = sqrtf((float)a.D);
  return a;
}

// DS, dq, dk, dv of one layer's attention for upstream a.dO (a.P and a.drop as the forward left them), and the gradients of the
// relative embeddings the heads share
void attn_bwd(hipStream_t s, const AttnArgs& a, int B, float* grad_rel_v, float* grad_rel_k) {
  hipLaunchKernelGGL(et_attn_bwd_q_kernel, dim3(a.L, a.H, B), dim3(128), ((size_t)a.L + a.D + 128) * sizeof(float), s, a);
  hipLaunchKernelGGL(et_attn_bwd_kv_kernel, dim3(a.L, a.H, B), dim3(128), (size_t)2 * a.L * sizeof(float), s, a);
  if (a.W > 0) {
    const int nw = 2 * a.W + 1, ne = nw * a.D;
    hipLaunchKernelGGL(et_attn_bwd_rel_kernel, dim3(nw, B), dim3(128), 0, s, a);
    hipLaunchKernelGGL(et_rel_finish_kernel, dim3((ne + 255) / 256), dim3(256), 0, s, a.rel_part, grad_rel_v, grad_rel_k, B, ne, 1.f / a.sqrt_d);
  }
}

// emb.weight's gradient from the gradient dx0 of emb(ids) * sqrt(C)
void embed_grad(hipStream_t s, const long long* ids, const float* dx0, float* grad, long long rows, int n_vocab, int C) {
  hipLaunchKernelGGL(et_embed_grad_kernel, dim3(n_vocab), dim3(256), 0, s, ids, dx0, grad, rows, C, sqrtf((float)C));
}

// scratch of the us_encoder_debug_* entry points: the backward's own slots (conv_bwd, ln_bwd and attn_bwd read them from a Layout)
Layout et_debug_layout(const us_frontend* h, int B, int L) {
  const auto& c = h->ec;
  const size_t rows = (size_t)B * L, C = c.n_channels, F = c.filter_channels;
  Layout o{};
  WsTake take;
  o.splits = wgrad_splits((long long)rows);
  o.wd = take(conv_numel(h));
  o.wpart = take((size_t)o.splits * conv_numel(h));
  o.cpart = take((size_t)kColChunks * std::max(std::max(C, F), (size_t)c.n_feats));
  o.dyx = take(rows * C);
  o.dyo = take(rows * C);
  o.rpart = take(4 * (size_t)B * (2 * (size_t)c.window_size + 1) * (C / c.n_heads));      // doubles
  o.total = take.total;
  return o;
}

// the attention backward keeps two rows of L and one of D in LDS
int et_lds_bound(us_frontend* h, const char* what, int L) {
  const int D = h->ec.n_channels / h->ec.n_heads;
  if (((size_t)2 * L + D + 128) * sizeof(float) > 64 * 1024)
    return h->fail(US_EINVAL, std::string(what) + ": more than ~8000 symbols per utterance");
  return US_OK;
}

// features: the entry point is one of the *_features ones (the handle must be a ContentVec one, and the other way round)
int et_check(us_frontend* h, const char* what, bool features, int B, int L) {
  int rc = fe_accept(h, kEncoder, what, B, L);
  if (rc == US_OK) rc = fe_front(h, what, features);
  if (rc == US_OK) rc = h->all_loaded(what);
  return rc != US_OK ? rc : et_lds_bound(h, what, L);
}

// us_encoder_forward_train (ids; feats null) and us_encoder_forward_features_train (feats; ids null)
int et_forward_train(us_frontend* h, const char* what, bool features, const int64_t* ids, const float* feats, const int64_t* lengths, float* mu_x,
                     float* x_out, float* x_mask, int B, int L, float p_dropout, uint64_t seed, void* workspace, size_t workspace_bytes,
                     us_stream stream) {
  int rc = et_check(h, what, features, B, L);
  if (rc != US_OK) return rc;
  if ((features ? !feats : !ids) || !lengths || !mu_x || !x_out || !x_mask) return fe_fail(h, US_EINVAL, std::string(what) + ": null argument");
  if (!(p_dropout < 1.f)) return fe_fail(h, US_EINVAL, std::string(what) + ": p_dropout must be below 1");
  const bool no_dropout = p_dropout < 0.f;         // the reference in eval mode (autograd still runs): no site drops
  if (!workspace || workspace_bytes < us_encoder_train_workspace_bytes(h, B, L))
    return fe_fail(h, US_EWORKSPACE, std::string(what) + ": workspace too small (us_encoder_train_workspace_bytes)");
  const auto& c = h->ec;
  const Layout l = et_layout(h, B, L);
  Ctx x{h, static_cast<hipStream_t>(stream), ws_align(workspace), &l, B, L, (long long)B * L, nullptr};
  x.mask = x.f(l.mask);
  // the tape: one slot per entry and layer (Layout); conv_o / conv_2's output goes to backward scratch, free during the forward
  EncoderBufs b{};
  b.mask = x.mask; b.ids_tape = reinterpret_cast<long long*>(x.f(l.ids)); b.x0 = x.f(l.x0);
  for (int i = 0; i < kPrenetLayers; ++i) { b.pc[i] = x.f(l.pc[i]); b.pa[i] = x.f(l.pa[i]); }
  b.y = x.f(l.g); b.xf = x.f(l.xf); b.mu = x.f(l.mu);
  for (int i = 0; i < c.n_layers; ++i)
    b.layer.push_back({x.f(l.x[i]), x.f(l.q[i]), x.f(l.k[i]), x.f(l.v[i]), x.f(l.at[i]), x.f(l.n1[i]), x.f(l.x1[i]), x.f(l.hd[i]),
                       x.f(l.n2[i]), x.f(l.p[i])});
  EncoderMode m;
  m.train = m.gemm = true; m.seed = seed; m.p = no_dropout ? 0.f : p_dropout; m.p_prenet = no_dropout ? 0.f : kPrenetP;
  if ((rc = encoder_forward(h, x.s, b, m, ids, feats, lengths, mu_x, x_out, B, L)) != US_OK) return rc;
  hipError_t e = hipMemcpyAsync(x_mask, x.mask, (size_t)x.rows * sizeof(float), hipMemcpyDeviceToDevice, x.s);
  if (e == hipSuccess) e = hipGetLastError();
  if (e != hipSuccess) return h->hip(what, e);
  h->tapes[workspace] = EncoderTape{B, L, p_dropout, seed};
  return US_OK;
}

}  // namespace

int wgrad_splits(long long rows) {
  long long s = rows / 512;
  return (int)(s < 1 ? 1 : (s > 32 ? 32 : s));
}

void gemm_conv_wgrad(us_frontend* h, hipStream_t s, const std::string& key, const float* in, const float* mask, bool mask_in, const float* dout,
                     long long rows, int L, float* part, float* dw) {
  const Weight& w = h->w[key + ".weight"];
  const int Cout = (int)w.shape[0], Cin = (int)w.shape[1], K = (int)w.shape[2];
  const int splits = wgrad_splits(rows);
  GemmArgs g{};
  g.in = in; g.mask = mask; g.mask_in = mask_in;
  g.rows = (int)rows; g.L = L; g.Cin = Cin; g.N = Cout; g.K = K; g.pad = K / 2;
  g.dout = dout; g.part = part; g.splits = splits;
  g.rows_per_split = (int)(((rows + splits - 1) / splits + kBK - 1) / kBK * kBK);
  g.drop.site = -1;
  hipLaunchKernelGGL(et_gemm_kernel<true>, dim3((Cin + kBM - 1) / kBM, (Cout + kBN - 1) / kBN, K * splits), dim3(256), 0, s, g);
  hipLaunchKernelGGL(et_wgrad_finish_kernel, dim3(et_blocks((long long)Cout * Cin * K, 256)), dim3(256), 0, s, part, dw, splits, K, Cin, Cout, 1.f);
}

// emb.weight's gradient of a ContentVec handle: dw [C][n_contentvec] = sqrt(C) * sum over valid rows of dx0[row][c] * feats[row][k],
// the split wgrad GEMM at K = 1 (rows whose mask is 0 are not read)
void gemm_front_wgrad(us_frontend* h, hipStream_t s, const float* feats, const float* mask, const float* dx0, long long rows, int L,
                      float* part, float* dw) {
  const int C = h->ec.n_channels, Cin = h->n_contentvec;
  const int splits = wgrad_splits(rows);
  GemmArgs g{};
  g.in = feats; g.mask = mask;
  g.rows = (int)rows; g.L = L; g.Cin = Cin; g.N = C; g.K = 1; g.pad = 0;
  g.dout = dx0; g.part = part; g.splits = splits;
  g.rows_per_split = (int)(((rows + splits - 1) / splits + kBK - 1) / kBK * kBK);
  g.drop.site = -1;
  hipLaunchKernelGGL((et_gemm_kernel<true, true>), dim3((Cin + kBM - 1) / kBM, (C + kBN - 1) / kBN, splits), dim3(256), 0, s, g);
  hipLaunchKernelGGL(et_wgrad_finish_kernel, dim3(et_blocks((long long)C * Cin, 256)), dim3(256), 0, s, part, dw, splits, 1, Cin, C,
                     sqrtf((float)C));
}

// x0 [rows][C] = (feats [rows][n_contentvec] . emb.weight^T) * sqrt(C) with zeros at rows past their item's length, and x_mask
void gemm_front_fwd(us_frontend* h, hipStream_t s, const float* feats, const int64_t* lengths, float* x0, float* mask, long long rows, int L) {
  const Weight& w = h->w["emb.weight"];
  GemmArgs a{};
  a.in = feats; a.lengths = reinterpret_cast<const long long*>(lengths); a.mask_w = mask;
  a.rows = (int)rows; a.L = L; a.N = (int)w.shape[0]; a.Cin = (int)w.shape[1]; a.K = 1; a.pad = 0;
  a.w = w.packed; a.out = x0; a.scale = sqrtf((float)a.N);
  a.drop.site = -1;
  hipLaunchKernelGGL((et_gemm_kernel<false, true>), dim3((rows + kBM - 1) / kBM, (a.N + kBN - 1) / kBN), dim3(256), 0, s, a);
}

// the forward form with the tap-flipped transposed weight
void gemm_conv_dgrad(us_frontend* h, hipStream_t s, const std::string& key, const float* dout, float* din, const float* mask, const float* add,
                     const float* gate, float gate_scale, bool mask_out, long long rows, int L, float* wd) {
  const Weight& w = h->w[key + ".weight"];
  const int Cout = (int)w.shape[0], Cin = (int)w.shape[1], K = (int)w.shape[2];
  hipLaunchKernelGGL(et_pack_dgrad_kernel, dim3(et_blocks((long long)Cout * Cin * K, 256)), dim3(256), 0, s, w.dev, wd, Cout, Cin, K);
  GemmArgs a{};
  a.in = dout; a.mask = mask; a.mask_in = 0;
  a.rows = (int)rows; a.L = L; a.Cin = Cout; a.N = Cin; a.K = K; a.pad = K / 2;
  a.w = wd; a.gate = gate; a.gate_scale = gate_scale; a.add = add; a.out = din; a.mask_out = mask_out;
  a.drop.site = -1;
  hipLaunchKernelGGL(et_gemm_kernel<false>, dim3((rows + kBM - 1) / kBM, (Cin + kBN - 1) / kBN), dim3(256), 0, s, a);
}

void gemm_conv_fwd(us_frontend* h, hipStream_t s, const std::string& key, const float* in, float* out, const float* mask, const float* add,
                   long long rows, int L, bool mask_in, bool relu, bool mask_out, Drop drop) {
  const Weight& w = h->w[key + ".weight"];
  GemmArgs a{};
  a.in = in; a.mask = mask; a.mask_in = mask_in;
  a.rows = (int)rows; a.L = L; a.N = (int)w.shape[0]; a.Cin = (int)w.shape[1]; a.K = (int)w.shape[2]; a.pad = a.K / 2;
  a.w = w.packed; a.bias = wdev(h, key + ".bias"); a.add = add; a.out = out; a.relu = relu; a.mask_out = mask_out;
  a.drop = drop;
  hipLaunchKernelGGL(et_gemm_kernel<false>, dim3((rows + kBM - 1) / kBM, (a.N + kBN - 1) / kBN), dim3(256), 0, s, a);
}

}  // namespace us

extern "C" {

using namespace us;

size_t us_encoder_train_workspace_bytes(us_frontend_handle h, int B, int L) {
  if (!h || h->kind != kEncoder || B <= 0 || L <= 0) return 0;
  return et_layout(h, B, L).total * sizeof(float) + 256;
}

int us_encoder_forward_train(us_frontend_handle h, const int64_t* ids, const int64_t* lengths, float* mu_x, float* x_out, float* x_mask,
                             int B, int L, float p_dropout, uint64_t seed, void* workspace, size_t workspace_bytes, us_stream stream) {
  return et_forward_train(h, "us_encoder_forward_train", false, ids, nullptr, lengths, mu_x, x_out, x_mask, B, L, p_dropout, seed, workspace,
                          workspace_bytes, stream);
}

int us_encoder_forward_features_train(us_frontend_handle h, const float* feats, const int64_t* lengths, float* mu_x, float* x_out,
                                      float* x_mask, int B, int L, float p_dropout, uint64_t seed, void* workspace, size_t workspace_bytes,
                                      us_stream stream) {
  return et_forward_train(h, "us_encoder_forward_features_train", true, nullptr, feats, lengths, mu_x, x_out, x_mask, B, L, p_dropout, seed,
                          workspace, workspace_bytes, stream);
}

namespace {

// us_encoder_backward (feats null: the ids are on the tape) and us_encoder_backward_features (the caller passes feats again)
int et_backward(us_frontend* h, const char* what, const char* fwd, bool features, const float* feats, const float* grad_mu,
                const float* grad_x, int B, int L, const char* const* keys, float* const* grads, int n_grads, void* workspace,
                size_t workspace_bytes, us_stream stream) {
  int rc = et_check(h, what, features, B, L);
  if (rc != US_OK) return rc;
  if (features && !feats) return fe_fail(h, US_EINVAL, std::string(what) + ": null argument");
  EncoderTape tape;
  if ((rc = fe_tape(h, what, fwd, B, L, workspace, workspace_bytes, us_encoder_train_workspace_bytes(h, B, L), &tape)) != US_OK) return rc;
  const auto& c = h->ec;
  const Layout l = et_layout(h, B, L);
  Ctx x{h, static_cast<hipStream_t>(stream), ws_align(workspace), &l, B, L, (long long)B * L, nullptr};
  x.mask = x.f(l.mask);
  const int C = c.n_channels, nf = c.n_feats;
  std::map<std::string, float*> dst;
  if ((rc = fe_grad_table(h, what, keys, grads, n_grads, x.f(l.arena), &dst)) != US_OK) return rc;
  auto G = [&](const std::string& k) { return dst.at(k); };
  const float p = tape.p_dropout < 0.f ? 0.f : tape.p_dropout, p_prenet = tape.p_dropout < 0.f ? 0.f : kPrenetP;
  const uint64_t seed = tape.seed;
  float* g = x.f(l.g);         // gradient of the current block's output (already masked)
  float* t = x.f(l.t);
  float* d1 = x.f(l.d1);
  float* dh = x.f(l.dh);
  // upstream: x = xf (masked), mu = proj_m(xf) * mask
  if (grad_x)
    hipLaunchKernelGGL(et_to_channel_last_kernel, dim3((L + 31) / 32, (C + 31) / 32, B), dim3(32, 8), 0, x.s, grad_x, x.mask, g, L, C);
  else
    (void)hipMemsetAsync(g, 0, (size_t)x.rows * C * sizeof(float), x.s);
  if (grad_mu) {
    hipLaunchKernelGGL(et_to_channel_last_kernel, dim3((L + 31) / 32, (nf + 31) / 32, B), dim3(32, 8), 0, x.s, grad_mu, x.mask, d1, L, nf);
    conv_bwd(x, "proj_m", x.f(l.xf), false, d1, g, g, nullptr, 1.f, true, G("proj_m.weight"), G("proj_m.bias"));
  } else {
    (void)hipMemsetAsync(G("proj_m.weight"), 0, (size_t)nf * C * sizeof(float), x.s);
    (void)hipMemsetAsync(G("proj_m.bias"), 0, (size_t)nf * sizeof(float), x.s);
  }
  const float ps = p > 0.f ? 1.f / (1.f - p) : 1.f;
  for (int i = c.n_layers - 1; i >= 0; --i) {
    const std::string n = std::to_string(i), ap = "encoder.attn_layers." + n, fp = "encoder.ffn_layers." + n;
    const std::string n1 = "encoder.norm_layers_1." + n, n2 = "encoder.norm_layers_2." + n;
    // x_out = LN2(x1 + drop(y2)) (* mask: g is masked), y2 = conv_2(hd * mask) * mask, hd = drop(relu(conv_1(x1 * mask)))
    ln_bwd(x, n2, x.f(l.n2[i]), g, nullptr, 1.f, t, G(n2 + ".gamma"), G(n2 + ".beta"));
    hipLaunchKernelGGL(et_drop_mask_kernel, dim3(et_blocks(x.rows * C, 256)), dim3(256), 0, x.s, t, x.mask, d1, x.rows, C, L,
                       make_drop(seed, layer_site(i, kSiteFfnOut), p));
    conv_bwd(x, fp + ".conv_2", x.f(l.hd[i]), true, d1, dh, nullptr, x.f(l.hd[i]), ps, true, G(fp + ".conv_2.weight"), G(fp + ".conv_2.bias"));
    conv_bwd(x, fp + ".conv_1", x.f(l.x1[i]), true, dh, t, t, nullptr, 1.f, true, G(fp + ".conv_1.weight"), G(fp + ".conv_1.bias"));
    // x1 = LN1(x + drop(conv_o(attn(x))))
    ln_bwd(x, n1, x.f(l.n1[i]), t, nullptr, 1.f, g, G(n1 + ".gamma"), G(n1 + ".beta"));
    hipLaunchKernelGGL(et_drop_mask_kernel, dim3(et_blocks(x.rows * C, 256)), dim3(256), 0, x.s, g, nullptr, d1, x.rows, C, L,
                       make_drop(seed, layer_site(i, kSiteAttnOut), p));
    conv_bwd(x, ap + ".conv_o", x.f(l.at[i]), false, d1, dh, nullptr, nullptr, 1.f, false, G(ap + ".conv_o.weight"), G(ap + ".conv_o.bias"));
    AttnArgs a = attn_args(x, i);
    a.drop = make_drop(seed, layer_site(i, kSiteAttnP), p);
    a.dO = dh; a.DS = x.f(l.ds); a.dq = x.f(l.dq); a.dk = x.f(l.dk); a.dv = x.f(l.dv); a.rel_part = reinterpret_cast<double*>(x.f(l.rpart));
    attn_bwd(x.s, a, B, c.window_size > 0 ? G(ap + ".emb_rel_v") : nullptr, c.window_size > 0 ? G(ap + ".emb_rel_k") : nullptr);
    // the block's input x (masked on entry): residual + q / k / v data gradients, then the entry mask
    const float* xin = x.f(l.x[i]);
    conv_bwd(x, ap + ".conv_q", xin, false, x.f(l.dq), g, g, nullptr, 1.f, false, G(ap + ".conv_q.weight"), G(ap + ".conv_q.bias"));
    conv_bwd(x, ap + ".conv_k", xin, false, x.f(l.dk), g, g, nullptr, 1.f, false, G(ap + ".conv_k.weight"), G(ap + ".conv_k.bias"));
    conv_bwd(x, ap + ".conv_v", xin, false, x.f(l.dv), g, g, nullptr, 1.f, true, G(ap + ".conv_v.weight"), G(ap + ".conv_v.bias"));
  }
  // prenet output (x0 + proj(a_2)) * mask: g is its (masked) gradient
  conv_bwd(x, "prenet.proj", x.f(l.pa[kPrenetLayers - 1]), false, g, t, nullptr, nullptr, 1.f, false, G("prenet.proj.weight"),
           G("prenet.proj.bias"));
  for (int i = kPrenetLayers - 1; i >= 0; --i) {
    const std::string n = std::to_string(i), cp = "prenet.conv_layers." + n, np = "prenet.norm_layers." + n;
    // t: gradient of a_i;  a_i = drop(relu(LN(c_i))), c_i = conv(in * mask)
    ln_bwd(x, np, x.f(l.pc[i]), t, x.f(l.pa[i]), p_prenet > 0.f ? 1.f / (1.f - p_prenet) : 1.f, d1, G(np + ".gamma"), G(np + ".beta"));
    if (i > 0) conv_bwd(x, cp, x.f(l.pa[i - 1]), true, d1, t, nullptr, nullptr, 1.f, true, G(cp + ".weight"), G(cp + ".bias"));
    else conv_bwd(x, cp, x.f(l.x0), true, d1, g, g, nullptr, 1.f, true, G(cp + ".weight"), G(cp + ".bias"));
  }
  // g: the (masked) gradient of x0
  if (features) gemm_front_wgrad(h, x.s, feats, x.mask, g, x.rows, L, x.f(l.wpart), G("emb.weight"));
  else embed_grad(x.s, reinterpret_cast<const long long*>(x.f(l.ids)), g, G("emb.weight"), x.rows, c.n_vocab, C);
  return fe_launched(h, what);
}

}  // namespace

int us_encoder_backward(us_frontend_handle h, const float* grad_mu, const float* grad_x, int B, int L, const char* const* keys,
                        float* const* grads, int n_grads, void* workspace, size_t workspace_bytes, us_stream stream) {
  return et_backward(h, "us_encoder_backward", "us_encoder_forward_train", false, nullptr, grad_mu, grad_x, B, L, keys, grads, n_grads,
                     workspace, workspace_bytes, stream);
}

int us_encoder_backward_features(us_frontend_handle h, const float* feats, const float* grad_mu, const float* grad_x, int B, int L,
                                 const char* const* keys, float* const* grads, int n_grads, void* workspace, size_t workspace_bytes,
                                 us_stream stream) {
  return et_backward(h, "us_encoder_backward_features", "us_encoder_forward_features_train", true, feats, grad_mu, grad_x, B, L, keys,
                     grads, n_grads, workspace, workspace_bytes, stream);
}

int us_encoder_tape_release(us_frontend_handle h, const void* workspace) {
  return fe_tape_release(h, kEncoder, "us_encoder_tape_release", workspace);
}

int us_encoder_dropout_mask(us_frontend_handle h, uint64_t seed, int site, int B, int L, float p_dropout, float* out, us_stream stream) {
  if (!h || h->kind != kEncoder || !out || B <= 0 || L <= 0) return fe_fail(h, US_EINVAL, "us_encoder_dropout_mask: bad argument");
  const auto& c = h->ec;
  if (site < 0 || site >= kPrenetLayers + kSitesPerLayer * c.n_layers) return fe_fail(h, US_EINVAL, "us_encoder_dropout_mask: no such site");
  long long n = (long long)B * c.n_channels * L;
  if (!(p_dropout < 1.f)) return fe_fail(h, US_EINVAL, "us_encoder_dropout_mask: p_dropout must be below 1");
  float p = p_dropout < 0.f ? 0.f : p_dropout;
  if (site < kPrenetLayers) p = p_dropout < 0.f ? 0.f : kPrenetP;
  else if ((site - kPrenetLayers) % kSitesPerLayer == kSiteAttnP) n = (long long)B * c.n_heads * L * L;
  else if ((site - kPrenetLayers) % kSitesPerLayer == kSiteFfnRelu) n = (long long)B * c.filter_channels * L;
  return fe_keep_mask(h, "us_encoder_dropout_mask", static_cast<hipStream_t>(stream), out, n, make_drop(seed, site, p));
}

// ---- one launch group alone, for kernel-level parity tests (tests/test_encoder_train_kernels_gpu.py) ---------------------------
namespace {

// what every debug entry point checks before anything else; `lay` receives the scratch layout
int et_debug_check(us_frontend* h, const char* what, int B, int L, void* workspace, size_t workspace_bytes, Layout* lay) {
  int rc = fe_accept(h, kEncoder, what, B, L);
  if (rc != US_OK) return rc;
  if ((long long)B * L > 0x7fffffffLL / 1024) return h->fail(US_EINVAL, std::string(what) + ": bad B or L");
  if ((rc = et_lds_bound(h, what, L)) != US_OK || (rc = h->all_loaded(what)) != US_OK) return rc;
  if (lay) {
    *lay = et_debug_layout(h, B, L);
    if (!workspace || workspace_bytes < lay->total * sizeof(float) + 256)
      return h->fail(US_EWORKSPACE, std::string(what) + ": workspace too small (us_encoder_debug_workspace_bytes)");
  }
  return US_OK;
}

}  // namespace

size_t us_encoder_debug_workspace_bytes(us_frontend_handle h, int B, int L) {
  if (!h || h->kind != kEncoder || B <= 0 || L <= 0) return 0;
  return et_debug_layout(h, B, L).total * sizeof(float) + 256;
}

int us_encoder_debug_conv(us_frontend_handle h, const char* key, int mode, const float* in, const float* dout, const float* mask,
                          const float* add, const float* gate, float gate_scale, unsigned flags, int drop_site, float p_dropout, uint64_t seed,
                          float* out, float* dw, float* db, int B, int L, void* workspace, size_t workspace_bytes, us_stream stream) {
  const char* what = "us_encoder_debug_conv";
  int rc = fe_accept(h, kEncoder, what);
  if (rc != US_OK) return rc;
  if (!key || mode < US_ENCODER_CONV_FWD || mode > US_ENCODER_CONV_DGRAD || (flags & ~7u))
    return fe_fail(h, US_EINVAL, std::string(what) + ": null key, unknown mode or unknown flag");
  const bool mask_in = flags & US_ENCODER_CONV_MASK_IN, relu = flags & US_ENCODER_CONV_RELU, mask_out = flags & US_ENCODER_CONV_MASK_OUT;
  const bool fwd = mode == US_ENCODER_CONV_FWD, wgrad = mode == US_ENCODER_CONV_WGRAD, dgrad = mode == US_ENCODER_CONV_DGRAD;
  if ((fwd && (!in || !out || dout || gate || dw || db)) || (wgrad && (!in || !dout || !dw || !db || out || add || gate || relu || mask_out)) ||
      (dgrad && (!dout || !out || in || dw || db || relu || mask_in)) || ((mask_in || mask_out) && !mask))
    return fe_fail(h, US_EINVAL, std::string(what) + ": an operand this mode needs is null, or one it does not take is given");
  const auto& c = h->ec;
  if (fwd && drop_site >= 0 && (drop_site >= kPrenetLayers + kSitesPerLayer * c.n_layers || !(p_dropout >= 0.f && p_dropout < 1.f)))
    return fe_fail(h, US_EINVAL, std::string(what) + ": no such dropout site, or p_dropout outside [0, 1)");
  if (!fwd && drop_site >= 0) return fe_fail(h, US_EINVAL, std::string(what) + ": only the forward has a dropout site");
  const std::string k(key);
  auto wi = h->w.find(k + ".weight");
  if (wi == h->w.end() || wi->second.shape.size() != 3 || !h->w.count(k + ".bias"))
    return fe_fail(h, US_ENOKEY, std::string(what) + ": unknown convolution '" + k + "'");
  Layout l;
  if ((rc = et_debug_check(h, what, B, L, workspace, workspace_bytes, &l)) != US_OK) return rc;
  Ctx x{h, static_cast<hipStream_t>(stream), ws_align(workspace), &l, B, L, (long long)B * L, const_cast<float*>(mask)};
  if (fwd) gemm_conv_fwd(h, x.s, k, in, out, mask, add, x.rows, L, mask_in, relu, mask_out, drop_site >= 0 ? make_drop(seed, drop_site, p_dropout) : no_drop());
  else if (wgrad) conv_bwd(x, k, in, mask_in, dout, nullptr, nullptr, nullptr, 1.f, false, dw, db);
  else gemm_conv_dgrad(h, x.s, k, dout, out, mask, add, gate, gate_scale, mask_out, x.rows, L, x.f(l.wd));
  return fe_launched(h, what);
}

int us_encoder_debug_ln_bwd(us_frontend_handle h, const char* key, const float* x_in, const float* dy, const float* gate, float gate_scale,
                            float* dx, float* dgamma, float* dbeta, int B, int L, void* workspace, size_t workspace_bytes, us_stream stream) {
  const char* what = "us_encoder_debug_ln_bwd";
  int rc = fe_accept(h, kEncoder, what);
  if (rc != US_OK) return rc;
  if (!key || !x_in || !dy || !dx || !dgamma || !dbeta) return fe_fail(h, US_EINVAL, std::string(what) + ": null argument");
  const std::string k(key);
  if (!h->w.count(k + ".gamma") || !h->w.count(k + ".beta")) return fe_fail(h, US_ENOKEY, std::string(what) + ": unknown LayerNorm '" + k + "'");
  Layout l;
  if ((rc = et_debug_check(h, what, B, L, workspace, workspace_bytes, &l)) != US_OK) return rc;
  Ctx x{h, static_cast<hipStream_t>(stream), ws_align(workspace), &l, B, L, (long long)B * L, nullptr};
  ln_bwd(x, k, x_in, dy, gate, gate_scale, dx, dgamma, dbeta);
  return fe_launched(h, what);
}

int us_encoder_debug_attention(us_frontend_handle h, int layer, const float* q, const float* k, const float* v, const float* mask, float p_dropout,
                               uint64_t seed, float* out, float* P, const float* dO, float* DS, float* dq, float* dk, float* dv,
                               float* grad_rel_k, float* grad_rel_v, int B, int L, void* workspace, size_t workspace_bytes, us_stream stream) {
  const char* what = "us_encoder_debug_attention";
  int rc = fe_accept(h, kEncoder, what);
  if (rc != US_OK) return rc;
  const auto& c = h->ec;
  if (!q || !k || !v || !mask || !out || !P || !(p_dropout >= 0.f && p_dropout < 1.f))
    return fe_fail(h, US_EINVAL, std::string(what) + ": null argument, or p_dropout outside [0, 1)");
  const bool rel = c.window_size > 0;
  if (dO ? (!DS || !dq || !dk || !dv || (rel && (!grad_rel_k || !grad_rel_v))) : (DS || dq || dk || dv || grad_rel_k || grad_rel_v))
    return fe_fail(h, US_EINVAL, std::string(what) + ": the backward takes dO and every gradient buffer, the forward alone none of them");
  if (layer < 0 || layer >= c.n_layers) return fe_fail(h, US_ENOKEY, std::string(what) + ": no attention layer " + std::to_string(layer));
  Layout l;
  if ((rc = et_debug_check(h, what, B, L, workspace, workspace_bytes, &l)) != US_OK) return rc;
  Ctx x{h, static_cast<hipStream_t>(stream), ws_align(workspace), &l, B, L, (long long)B * L, const_cast<float*>(mask)};
  const std::string ap = "encoder.attn_layers." + std::to_string(layer);
  AttnArgs a{};
  a.q = q; a.k = k; a.v = v; a.mask = mask; a.P = P; a.out = out;
  a.rel_k = rel ? wdev(h, ap + ".emb_rel_k") : nullptr;
  a.rel_v = rel ? wdev(h, ap + ".emb_rel_v") : nullptr;
  a.L = L; a.C = c.n_channels; a.H = c.n_heads; a.D = c.n_channels / c.n_heads; a.W = c.window_size;
  a.sqrt_d = sqrtf((float)a.D);
  a.drop = make_drop(seed, layer_site(layer, kSiteAttnP), p_dropout);
  rel_attention_fwd(x.s, a, B, true);
  if (dO) {
    a.dO = dO; a.DS = DS; a.dq = dq; a.dk = dk; a.dv = dv; a.rel_part = reinterpret_cast<double*>(x.f(l.rpart));
    attn_bwd(x.s, a, B, grad_rel_v, grad_rel_k);
  }
  return fe_launched(h, what);
}

int us_encoder_debug_embed_grad(us_frontend_handle h, const int64_t* ids, const float* dx0, float* grad, int B, int L, us_stream stream) {
  const char* what = "us_encoder_debug_embed_grad";
  int rc = fe_accept(h, kEncoder, what);
  if (rc != US_OK) return rc;
  if (!ids || !dx0 || !grad) return fe_fail(h, US_EINVAL, std::string(what) + ": null argument");
  if ((rc = fe_front(h, what, false)) != US_OK) return rc;
  if ((rc = et_debug_check(h, what, B, L, nullptr, 0, nullptr)) != US_OK) return rc;
  embed_grad(static_cast<hipStream_t>(stream), reinterpret_cast<const long long*>(ids), dx0, grad, (long long)B * L, h->ec.n_vocab, h->ec.n_channels);
  return fe_launched(h, what);
}

}  // extern "C"
