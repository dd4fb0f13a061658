// What whisper.hip asks of hubert.hip: Whisper's encoder and the cross-attention keys / values of its decoder run on HuBERT / WavLM's kernels
// (hb_gemm_kernel, hb_ln_kernel, hb_attn_kernel, hb_export_kernel), which stay in hubert.hip; the schedule stands there beside WavLM's pre-LN
// one.  The encoder's packed operands live behind an opaque pointer, the weights themselves in the caller's table under transformers' keys.
#pragma once
#include <hip/hip_runtime.h>

#include "handle.h"

namespace us {

struct WhEncGeometry {
  int n_mels, d_model, heads, ffn, layers, S;      // S = max_source_positions: the input has 2 S frames
  int dec_layers;                                  // decoder layers: one k | v projection of the encoder's output each
};

struct WhEncoder;                                  // hubert.hip

WhEncoder* wh_encoder_new(const WhEncGeometry& g);
void wh_encoder_free(WhEncoder* e);
hipError_t wh_encoder_alloc(WhEncoder* e);         // the packed forms; after it neither prepare nor a forward allocates
// the packed GEMM operands from the loaded tensors of `t` (model.encoder.*, model.decoder.layers.*.encoder_attn.{k,v}_proj.*)
hipError_t wh_encoder_prepare(WhEncoder* e, WeightTable& t, hipStream_t s);
size_t wh_encoder_ws_floats(const WhEncoder* e, int B);
// feats [B][n_mels][2 S] -> `planar` [B][d_model][S], encoder.layer_norm of the last layer's stream (always written), and the same
// channel-last in out [B][S][d_model] when out is not null.  ws: wh_encoder_ws_floats(e, B) floats, 256-byte aligned.
hipError_t wh_encoder_forward(WhEncoder* e, WeightTable& t, const float* feats, int B, float* planar, float* out, float* ws, hipStream_t s);
// kv [dec_layers][B][2 d_model][S] planar (k rows, then v rows: k_proj has no bias) from `planar`
hipError_t wh_encoder_cross_kv(WhEncoder* e, WeightTable& t, const float* planar, int B, float* kv, hipStream_t s);

}  // namespace us
