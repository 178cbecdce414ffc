// What the three training hosts (kdlae_train.cpp, kdlae_st.cpp, asdqe_train.cpp) share: the handle
// base and its parameter entry points, the record of the last forward, the backward's side stream and
// the flat-buffer accessors of a plan-based context.  Host code only.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "param_layout.h"
#include "runtime.h"

namespace kdlae {

// kdlae_tt_handle, kdlae_st_handle and asdqe_train_handle derive from it (each adds its config)
struct TrainHandleBase {
  int device = 0;
  ParamLayout lay{4};  // the model's parameter order, every key 16-byte aligned
  virtual ~TrainHandleBase() = default;
};
// the bodies of *_num_params / *_param_info / *_num_floats / *_destroy
inline int train_num_params(const TrainHandleBase* h, int null_value) { return h ? h->lay.size() : null_value; }
inline int train_param_info(const TrainHandleBase* h, int i, const char** name, int64_t* numel, int64_t* offset) {
  if (!h) return fail(KDLAE_EPARAM, "param index out of range");
  return h->lay.info(i, name, numel, offset);
}
inline int64_t train_num_floats(const TrainHandleBase* h) { return h ? h->lay.total : -1; }
inline int train_destroy(TrainHandleBase* h) {
  delete h;
  return KDLAE_OK;
}

// The last forward: its activations live in the caller's workspace `ws`, so a backward serves only
// that workspace.  The forwards call set(), the backwards check().
struct LastForward {
  bool valid = false;
  const void* ws = nullptr;
  int B = 0, F = 1, H = 0, W = 0;
  void set(const void* ws_, int B_, int F_, int H_, int W_) {
    valid = true;
    ws = ws_; B = B_; F = F_; H = H_; W = W_;
  }
  // KDLAE_ESTATE unless `bwd` (an entry's name) follows a `fwd` on the workspace ws_
  int check(const void* ws_, const char* bwd, const char* fwd) const {
    if (valid && ws == ws_) return KDLAE_OK;
    return fail(KDLAE_ESTATE, std::string(bwd) + " needs a preceding " + fwd + " on the same workspace");
  }
};

// true while `s` is being captured into a graph (an error answer, the null stream beside another thread's
// capture, counts as no)
inline bool stream_capturing(hipStream_t s) {
  hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(s, &st) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return st != hipStreamCaptureStatusNone;
}

// A backward's side stream (non-blocking) with its fork and join events: launches that only read what
// the main stream leaves alone until the next join (weight and bias gradients) run there, beside the
// input-gradient chain on the caller's stream.  Lives in the handle; destroyed with it.
struct SideStream {
  hipStream_t s = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  ~SideStream() {
    if (ev_fork) (void)hipEventDestroy(ev_fork);
    if (ev_join) (void)hipEventDestroy(ev_join);
    if (s) (void)hipStreamDestroy(s);
  }
  // *use = this, created on the current device at the first call; *use stays as it is (null: every
  // launch on the caller's stream, same results) under KDLAE_DEBUG=train_serial, and while `main` is being
  // captured into a graph: the side stream and the handle's events outlive any graph, so they are never
  // drawn into a caller's capture (include/kdlae.h, "Caller's stream")
  int acquire(SideStream** use, hipStream_t main) {
    if (debug_flag("train_serial")) return KDLAE_OK;
    if (stream_capturing(main)) return KDLAE_OK;
    if (!s) {
      HIPCHK(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
      HIPCHK(hipEventCreateWithFlags(&ev_fork, hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&ev_join, hipEventDisableTiming));
    }
    *use = this;
    return KDLAE_OK;
  }
  // the side stream waits for everything enqueued on `main` so far
  int fork(hipStream_t main) {
    HIPCHK(hipEventRecord(ev_fork, main));
    HIPCHK(hipStreamWaitEvent(s, ev_fork, 0));
    return KDLAE_OK;
  }
  // `main` waits for every side launch enqueued so far
  int join(hipStream_t main) {
    HIPCHK(hipEventRecord(ev_join, s));
    HIPCHK(hipStreamWaitEvent(main, ev_join, 0));
    return KDLAE_OK;
  }
};

// Base of the KDLAE-S and ASDQE contexts: workspace offsets (bytes, from the handle's plan) and the
// parameters / gradients by key (an unknown key throws).  KDLAE-T's context has its own lookup: a
// nullable one that records which gradient keys a pass touches.
struct FlatCtx {
  const ParamLayout* lay;
  const float* th;
  float* gr;
  char* ws;
  float* buf(size_t o) const { return reinterpret_cast<float*>(ws + o); }
  const float* P(const std::string& k) const { return th + lay->at(k); }
  float* G(const std::string& k) const { return gr + lay->at(k); }
};

}  // namespace kdlae
