// Host-side state of a `us_frontend_handle`, shared by the inference forward (frontend.hip) and the Encoder's training
// forward / backward (encoder_train.hip).
#pragma once
#include <map>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"

namespace us {

struct Weight {
  std::vector<int64_t> shape;
  float* dev = nullptr;        // reference layout
  float* packed = nullptr;     // conv weights: [K][Cin][Cout]
  bool loaded = false;
  size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

// what one us_encoder_forward_train left in a caller-owned workspace (keyed by the workspace's base address)
struct EncoderTape {
  int B = 0, L = 0;
  float p_dropout = 0.f;
  uint64_t seed = 0;
};

}  // namespace us

struct us_frontend {
  int kind = 0;                        // 0: Encoder, 1: DurationPredictor
  us_encoder_config ec{};
  us_duration_config dc{};
  int device = 0;
  std::vector<std::string> keys;       // state_dict order
  std::map<std::string, us::Weight> w;
  std::string err;
  std::map<const void*, us::EncoderTape> tapes;   // training forwards whose tape a workspace holds (us_encoder_tape_release)
};
