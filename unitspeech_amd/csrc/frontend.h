// Host-side state of a `us_frontend_handle` and what crosses between frontend.hip (the Encoder's forward in both modes, the
// DurationPredictor), encoder_train.hip (the MFMA convolution, the Encoder's backward) and duration_train.hip (the
// DurationPredictor's training): the dropout stream, the attention arguments, the forward's buffer table, the launchers the
// files call in each other, and the host logic the two trainable modules share (the entry check, the tape, the gradient table).
#pragma once
#include <hip/hip_runtime.h>

#include <map>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"
#include "handle.h"

namespace us {

// what one us_encoder_forward_train / us_duration_predictor_forward_train left in a caller-owned workspace (keyed by the
// workspace's base address)
struct EncoderTape {
  int B = 0, L = 0;
  float p_dropout = 0.f;
  uint64_t seed = 0;
};
enum { kEncoder = 0, kDuration = 1 };      // us_frontend::kind

}  // namespace us

struct us_frontend : us::WeightTable {
  int kind = us::kEncoder;
  us_encoder_config ec{};
  int n_contentvec = 0;                           // > 0: a ContentVec handle, emb is Linear(n_contentvec -> n_channels, bias=False)
  us_duration_config dc{};
  std::map<const void*, us::EncoderTape> tapes;   // training forwards whose tape a workspace holds (us_encoder_tape_release)
};

namespace us {

constexpr int kPrenetLayers = 3, kPrenetKernel = 5;      // encoder.py:283-284
constexpr float kPrenetP = 0.5f;                         // encoder.py:285-286

// ---- dropout stream (the scheme is described at the top of encoder_train.hip) ----------------------------------------------
struct Drop {
  unsigned long long seed;
  int site;          // < 0: no dropout
  float p, scale;
};
constexpr int kSitesPerLayer = 4;
enum { kSiteAttnP = 0, kSiteAttnOut = 1, kSiteFfnRelu = 2, kSiteFfnOut = 3 };
inline Drop make_drop(uint64_t seed, int site, float p) {
  Drop d{};
  d.seed = seed; d.site = p > 0.f ? site : -1; d.p = p; d.scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  return d;
}
inline Drop no_drop() { return make_drop(0, -1, 0.f); }
inline int layer_site(int layer, int which) { return kPrenetLayers + kSitesPerLayer * layer + which; }

#if defined(__HIPCC__)
__device__ __forceinline__ void et_philox(uint32_t c[4], uint32_t k0, uint32_t k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = __umulhi(0xD2511F53u, c[0]), lo0 = 0xD2511F53u * c[0];
    uint32_t hi1 = __umulhi(0xCD9E8D57u, c[2]), lo1 = 0xCD9E8D57u * c[2];
    uint32_t n0 = hi1 ^ c[1] ^ k0, n1 = lo1, n2 = hi0 ^ c[3] ^ k1, n3 = lo0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
}
// the factor element `idx` of a site is multiplied by: 0 or 1 / (1 - p); 1 when p == 0 or there is no site
__device__ __forceinline__ float et_keep(const Drop& d, unsigned long long idx) {
  if (d.site < 0 || d.p <= 0.f) return 1.f;
  uint32_t c[4] = {(uint32_t)(idx >> 2), (uint32_t)(idx >> 34), (uint32_t)d.site, 0u};
  et_philox(c, (uint32_t)d.seed, (uint32_t)(d.seed >> 32));
  const uint32_t w = c[idx & 3];
  return (float)(w >> 8) * 5.9604644775390625e-08f >= d.p ? d.scale : 0.f;      // uniform in [0, 1) on a 2^-24 grid
}
// flat index of channel-last element (row, c) in the reference's [B][C][L] tensor
__device__ __forceinline__ unsigned long long et_cf_index(long long row, int c, int C, int L) {
  const long long b = row / L, l = row - b * L;
  return ((unsigned long long)b * C + c) * L + l;
}
#endif

// ---- relative-position self-attention (encoder.py:115-144) --------------------------------------------------------------
struct AttnArgs {
  const float* q; const float* k; const float* v;     // [B][L][C], head h owns channels [h * D, (h + 1) * D)
  const float* rel_k; const float* rel_v;             // [2W+1][D] (heads share them) or null
  const float* mask;                                  // [B][L]
  float* P;                                           // training: [B][H][L][L] softmax probabilities before dropout
  float* out;                                         // [B][L][C]
  // backward
  const float* dO;                                    // [B][L][C] gradient of `out`
  float* DS;                                          // [B][H][L][L] gradient of the scores (0 where filled with -1e4)
  float* dq; float* dk; float* dv;                    // [B][L][C]
  double* rel_part;                                   // [2][B][2W+1][D]
  int L, C, D, H, W;
  float sqrt_d;
  Drop drop;                                          // training: dropout of p_attn, flat index of [B][H][L][L]
};

// ---- one Encoder forward ---------------------------------------------------------------------------------------------------
// The buffers encoder_forward walks, channel-last [B][L][C] unless noted.  Inference points them into seven planes that it
// reuses (entries alias, LayerNorm runs in place); training gives every entry its own slot of the tape.
struct EncoderBufs {
  float* mask;                 // [B][L], written by the embedding kernel (the front GEMM of a ContentVec handle)
  long long* ids_tape;         // training: the ids, kept for the embedding gradient (a ContentVec handle keeps nothing)
  float* x0;                   // emb(ids) * sqrt(C) / emb(feats) * sqrt(C)
  float* pc[kPrenetLayers];    // prenet conv_i output
  float* pa[kPrenetLayers];    // prenet relu_drop(LayerNorm(pc[i]))
  float* y;                    // conv_o / conv_2 output, dead after the LayerNorm that adds it
  float* xf;                   // the last block's output (the prenet's when n_layers == 0): `x`
  float* mu;                   // [B][L][n_feats] proj_m output
  struct Layer {
    float* x;                  // block input (masked)
    float *q, *k, *v, *at;
    float* n1;                 // training: x + drop(conv_o(at)), LayerNorm 1's input
    float* x1;                 // LayerNorm 1 output
    float* hd;                 // [B][L][F] drop(relu(conv_1))
    float* n2;                 // training: x1 + drop(conv_2(hd)), LayerNorm 2's input
    float* P;                  // training: [B][H][L][L]
  };
  std::vector<Layer> layer;    // n_layers entries
};
// train: the reference's Dropout sites at p / p_prenet (0: nothing is drawn) and the training entries of EncoderBufs stored; else
// eval mode.  gemm: the convolutions run on the MFMA GEMM of encoder_train.hip, else on fe_conv1d_kernel.  The entry point sets
// it and B or L never do: training does; inference does not, for either kind of handle (frontend.hip, encoder_forward)
struct EncoderMode {
  bool train = false, gemm = false;
  uint64_t seed = 0;
  float p = 0.f, p_prenet = 0.f;
};

// the table's fail under the name the three front-end files call it by (h may be null)
inline int fe_fail(us_frontend* h, int code, const std::string& msg) { return WeightTable::fail(h, code, msg); }
// how an entry point `what` ends once everything is enqueued: a launch's error is the call's
inline int fe_launched(us_frontend* h, const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? US_OK : h->hip(what, e);
}
// ---- frontend.hip: what the entry points of the two modules share --------------------------------------------------------
// how an entry point opens: h is a handle of `kind` (not null after this) and B, L are in 1..65535 (they become grid dimensions)
int fe_accept(us_frontend* h, int kind, const char* what, int B = 1, int L = 1);
// where a backward writes each key's gradient: the caller's buffer for keys[i], for a key nobody asked for its slot of `arena`
// (total_numel() floats that end a training workspace: every key's gradient in state_dict order, unpadded)
int fe_grad_table(us_frontend* h, const char* what, const char* const* keys, float* const* grads, int n_grads, float* arena,
                  std::map<std::string, float*>* dst);
// *out = the tape the training forward `fwd` left in `workspace` (of `need` bytes) for this B and L
int fe_tape(us_frontend* h, const char* what, const char* fwd, int B, int L, const void* workspace, size_t have, size_t need,
            EncoderTape* out);
int fe_tape_release(us_frontend* h, int kind, const char* what, const void* workspace);
// out[i] = the factor element i of site d.site is multiplied by, in the reference's layout (the *_dropout_mask test hooks)
int fe_keep_mask(us_frontend* h, const char* what, hipStream_t s, float* out, long long n, Drop d);
// frontend.hip: embedding -> prenet -> transformer blocks -> proj_m -> mu_x, x_out in the reference's [B][C][L]
// (ids for an id handle, feats [B][L][n_contentvec] for a ContentVec handle; the other is null)
int encoder_forward(us_frontend* h, hipStream_t s, const EncoderBufs& b, const EncoderMode& m, const int64_t* ids, const float* feats,
                    const int64_t* lengths, float* mu_x, float* x_out, int B, int L);
// the handle's front is the one the entry point `what` is for (features: one of the *_features entry points)
int fe_front(us_frontend* h, const char* what, bool features);
// encoder_train.hip: the Linear front as a K = 1 GEMM: x0 = (feats . emb.weight^T) * sqrt(C) and x_mask; rows past an item's
// length are not read and give zeros.  gemm_front_wgrad: emb.weight's gradient [C][n_contentvec] from dx0 over the rows mask keeps
void gemm_front_fwd(us_frontend* h, hipStream_t s, const float* feats, const int64_t* lengths, float* x0, float* mask, long long rows, int L);
void gemm_front_wgrad(us_frontend* h, hipStream_t s, const float* feats, const float* mask, const float* dx0, long long rows, int L,
                      float* part, float* dw);
// encoder_train.hip: the convolution `key` as an implicit GEMM on the fp32 matrix cores (training forward)
void gemm_conv_fwd(us_frontend* h, hipStream_t s, const std::string& key, const float* in, float* out, const float* mask, const float* add,
                   long long rows, int L, bool mask_in, bool relu, bool mask_out, Drop drop);
// encoder_train.hip: the two gradient forms of the same GEMM, on the caller's scratch.
// dw (torch layout [Cout][Cin][K]) of the convolution `key` whose forward read `in` (times mask when mask_in) and whose output
// gradient is dout; `part` holds wgrad_splits(rows) * K * Cin * Cout floats, added in a fixed order
int wgrad_splits(long long rows);
void gemm_conv_wgrad(us_frontend* h, hipStream_t s, const std::string& key, const float* in, const float* mask, bool mask_in, const float* dout,
                     long long rows, int L, float* part, float* dw);
// din = (add + dgrad(dout)) [gate > 0 ? * gate_scale : 0] [* mask]; `wd` holds the K * Cout * Cin floats of the flipped weight
void gemm_conv_dgrad(us_frontend* h, hipStream_t s, const std::string& key, const float* dout, float* din, const float* mask, const float* add,
                     const float* gate, float gate_scale, bool mask_out, long long rows, int L, float* wd);
// frontend.hip: the attention of one layer for B items (training: a.P is stored and a.drop applied)
void rel_attention_fwd(hipStream_t s, const AttnArgs& a, int B, bool train);
// frontend.hip: out[b][l] = x[b][:][l] | g[b][:] (channel-first in, channel-last out: the DurationPredictor's cat, :49-50)
void fe_gather_concat(hipStream_t s, const float* x_cf, const float* g, float* out, int B, int L, int C, int S);

}  // namespace us
