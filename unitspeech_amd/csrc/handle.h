// The host plumbing every handle that takes its weights by state_dict key shares (us_frontend, us_vocoder, us_speaker, us_mel, us_resample, us_hubert, us_wavlm, us_whisper): the weight
// table with its error reporting, device binding and load_weight prefix, and the small workspace helpers that came with each copy.  The
// decoder's handle (deferred raw copies and a flush) is a different design and does not use this.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <map>
#include <string>
#include <vector>

#include "../../include/unitspeech_hip.h"
#include "kernels.h"

namespace us {

struct Weight {
  std::vector<int64_t> shape;
  float* dev = nullptr;        // reference layout
  float* packed = nullptr;     // front end: conv weights as [K][Cin][Cout]; null where a module keeps its packed forms elsewhere
  bool loaded = false;
  size_t numel() const { size_t n = 1; for (auto s : shape) n *= (size_t)s; return n; }
};

// A handle struct derives from this.  The functions a C entry point calls before it knows its handle is not null are static and
// take the table as a pointer.
struct WeightTable {
  int device = 0;                      // the device that was current at creation: weights live there, launches go to its streams
  std::vector<std::string> keys;       // state_dict order
  std::map<std::string, Weight> w;
  std::string err;

  static int fail(WeightTable* t, int code, const std::string& msg) {
    if (t) t->err = msg;
    set_last_error(msg.c_str());
    return code;
  }
  int fail(int code, const std::string& msg) { return fail(this, code, msg); }
  int hip(const char* what, hipError_t e) { return fail(US_EHIP, std::string(what) + ": " + hipGetErrorString(e)); }

  void add(const std::string& k, std::vector<int64_t> shape) {
    keys.push_back(k);
    w[k].shape = std::move(shape);
  }

  int on_device(const char* what) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != device)
      return fail(US_EINVAL, std::string(what) + ": the current device (" + std::to_string(dev) + ") is not the handle's (" +
                                 std::to_string(device) + ")");
    return US_OK;
  }
  // every weight is loaded (else the first missing key in state_dict order) and the current device is the handle's
  int all_loaded(const char* what) {
    for (const auto& k : keys)
      if (!w[k].loaded) return fail(US_EWEIGHTS, std::string(what) + ": weight '" + k + "' has not been loaded");
    return on_device(what);
  }

  int num() const { return (int)keys.size(); }
  size_t total_numel() const { size_t n = 0; for (const auto& kv : w) n += kv.second.numel(); return n; }      // floats of all weights
  const char* key(int i) const { return (i >= 0 && i < num()) ? keys[i].c_str() : nullptr; }
  const char* last_error() const { return err.c_str(); }

  // us_*_load_weight up to the copy: null arguments, unknown key, shape, device.  `what` is the entry point's name.
  static int find(WeightTable* t, const char* what, const char* key, const float* data, const int64_t* shape, int ndim, Weight** out) {
    if (!t || !key || !data || !shape) return fail(t, US_EINVAL, std::string(what) + ": null argument");
    auto it = t->w.find(key);
    if (it == t->w.end()) return t->fail(US_ENOKEY, std::string(what) + ": unknown key '" + key + "'");
    Weight& wt = it->second;
    bool same = ndim == (int)wt.shape.size();
    for (int i = 0; same && i < ndim; ++i) same = shape[i] == wt.shape[i];
    if (!same) return t->fail(US_ESHAPE, std::string(what) + ": shape of '" + key + "' does not match the configuration");
    *out = &wt;
    return t->on_device(what);
  }
  // the copy itself, device to device on `s`; allocates wt.dev when the module has not
  int copy(Weight& wt, const float* data, hipStream_t s) {
    const size_t bytes = wt.numel() * sizeof(float);
    hipError_t e;
    if (!wt.dev && (e = hipMalloc(&wt.dev, bytes)) != hipSuccess) return hip("hipMalloc(weight)", e);
    if ((e = hipMemcpyAsync(wt.dev, data, bytes, hipMemcpyDeviceToDevice, s)) != hipSuccess) return hip("hipMemcpyAsync(weight)", e);
    return US_OK;
  }
  // find + copy.  The module makes its derived forms from *out and sets `loaded` itself.
  static int load(WeightTable* t, const char* what, const char* key, const float* data, const int64_t* shape, int ndim, hipStream_t s,
                  Weight** out) {
    const int rc = find(t, what, key, data, shape, ndim, out);
    return rc != US_OK ? rc : t->copy(**out, data, s);
  }

  void free_weights() {
    for (auto& kv : w) {
      if (kv.second.dev) (void)hipFree(kv.second.dev);
      if (kv.second.packed) (void)hipFree(kv.second.packed);
    }
  }
};

// What the handle-free entry points (glue, units, units_fit, ctc, ctc_train, level, tts_train) answer: a HIP error by name, a refused argument,
// and the batch a launch of one workgroup per item or per 64 rows takes: B in [1, 65535], T > 0, B * T <= 2^24.
inline int hip_fail(const char* what, hipError_t e) {
  char buf[256];
  snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  set_last_error(buf);
  return US_EHIP;
}
inline int bad_arg(const char* msg) {
  set_last_error(msg);
  return US_EINVAL;
}
constexpr bool rows_ok(int B, int T) { return B > 0 && T > 0 && B <= 65535 && (long long)B * T <= (1LL << 24); }

// a caller-owned workspace starts at its first 256-byte boundary (the *_workspace_bytes functions include the slack)
inline float* ws_align(void* ws) { return reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(ws) + 255) & ~uintptr_t(255)); }

constexpr int round_up(int v, int m) { return (v + m - 1) / m * m; }

// every buffer of a workspace takes a multiple of 64 floats, so each starts on a 256-byte boundary
constexpr size_t pad64(size_t n) { return (n + 63) / 64 * 64; }

// float offsets into the aligned workspace, handed out in order: take(n) is where a buffer of n floats starts, `total` what all of them need
struct WsTake {
  size_t total = 0;
  size_t operator()(size_t n) { const size_t at = total; total += pad64(n); return at; }
};

}  // namespace us
