// The sizes of a CTC head that ctc.hip (forward) and ctc_train.hip (loss, backward, alignment) both accept.
#pragma once

namespace us {

constexpr int kMaxV = 2048, kMaxH = 1024;

// nullptr, or why a head of V entries over H features is refused
inline const char* head_error(int V, int H) {
  if (V < 2 || V > kMaxV) return "V must be in [2, 2048]";
  if (H < 4 || H > kMaxH || H % 4) return "H must be a multiple of 4 in [4, 1024]";
  return nullptr;
}

}  // namespace us
