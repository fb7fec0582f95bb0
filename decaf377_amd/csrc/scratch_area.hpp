// scratch_area.hpp -- the per-device scratch areas that launches on ANY stream share: the guard that hands an area from
// stream to stream, the scope that holds it for one launch, and the grow-only area itself.  Nothing of the device code is
// included, so tests/cpp/scratch_area_host.cpp compiles this header against a fake runtime.
#pragma once
#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdio.h>
#include <vector>

#include "../../include/decaf377_amd.h"

extern thread_local char d377_g_err[512];

namespace d377 {

inline int fail(int code, const char* fmt, const char* detail) {
  snprintf(d377_g_err, sizeof d377_g_err, fmt, detail);
  return code;
}
#define HIP_TRY(expr)                                                                     \
  do {                                                                                    \
    hipError_t e_ = (expr);                                                               \
    if (e_ != hipSuccess) return ::d377::fail(D377_ERR_HIP, #expr ": %s", hipGetErrorString(e_)); \
  } while (0)

// A per-device scratch area that kernels launched on ANY stream may use (the variable-base window
// tables, the MSM workspace).  Users are serialised on the device: a launch first makes its stream wait
// for the previous user's completion event and records its own afterwards, so two `_dev` calls on
// different streams (or a host-path call on the context's private stream while a `_dev` launch is in
// flight) queue up instead of racing.  Host-side access to this struct is under d377_ctx::mu.
struct ScratchGuard {
  hipEvent_t ev = nullptr;
  bool used = false;
  std::vector<void*> retired;            // outgrown blocks of this guard's areas that a captured graph may still name (ScratchArea::reserve)
  int init() { HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming)); return D377_OK; }
  void destroy() {                       // with the context: the retired blocks go too
    if (ev) (void)hipEventDestroy(ev);
    ev = nullptr; used = false;
    for (void* r : retired) (void)hipFree(r);
    retired.clear();
  }
  // A stream that is being captured into a hipGraph takes no part in the hand-over (an event recorded outside
  // the capture cannot be waited on inside it): within the graph the launches keep their stream order.  What that
  // means for a replay that overlaps other calls is area-specific: the lane-set areas (window tables, inversion
  // records) are claimed atomically by every workgroup and never reset, so overlapping kernels simply share them;
  // the MSM workspace is exclusive, and a caller who replays a graph containing an MSM while another MSM of the same
  // device is in flight on a different stream must order the two (include/decaf377_amd.h, "Threads and streams").
  static bool capturing(hipStream_t s) {
    hipStreamCaptureStatus st = hipStreamCaptureStatusNone;
    return hipStreamIsCapturing(s, &st) == hipSuccess && st != hipStreamCaptureStatusNone;
  }
  bool seen_capture = false;             // some launch on this guard's areas has been captured into a graph (see ScratchArea)
  int acquire(hipStream_t s) {
    if (capturing(s)) { seen_capture = true; return D377_OK; }
    if (used) HIP_TRY(hipStreamWaitEvent(s, ev, 0));
    return D377_OK;
  }
  int release(hipStream_t s) { if (capturing(s)) return D377_OK; HIP_TRY(hipEventRecord(ev, s)); used = true; return D377_OK; }
  int drain() { if (used) HIP_TRY(hipEventSynchronize(ev)); return D377_OK; }   // before freeing the area
};

// Holds a scratch area for one launch: queues the launch behind the area's last user and records the hand-over event
// on EVERY path out of the launch once the area has been acquired -- also when a later step of the launch fails, so
// that the next user on another stream still queues behind whatever was enqueued.
struct GuardScope {
  ScratchGuard& g;
  hipStream_t s;
  bool held = false;
  int acquire() { int rc = g.acquire(s); held = rc == D377_OK; return rc; }
  // the success path hands over explicitly and reports a failed event record (the next user would not queue behind this
  // launch); the destructor covers the error paths
  int finish() { if (!held) return D377_OK; held = false; return g.release(s); }
  ~GuardScope() { if (held) (void)g.release(s); }
};

// How far past the bytes asked for an area grows: to b + b / div + add (div 0: no proportional part).
struct Slack { size_t div, add; };
constexpr Slack SLACK_TABLE_SCRATCH{0, 0}, SLACK_PARTIALS{4, 4096}, SLACK_MSM_WORKSPACE{8, 0};

// A grow-only area under a guard (the Straus table scratch, the long sums' partials, the MSM workspace).  Once a launch on
// the guard's areas has been captured into a hipGraph the graph holds pointers into the block it saw: from then on an
// outgrown block is retired (kept on the guard's list until the context is destroyed) instead of freed, so a replay never
// touches freed memory.
struct ScratchArea {
  void* mem = nullptr;
  size_t cap = 0;
  template <class T> T* as() const { return static_cast<T*>(mem); }
  // Room for `bytes`, before the launch's scope acquires the guard.  Growth is refused inside a stream capture
  // (D377_ERR_ARG, text `in_capture`) and waits for the guard's last user; a failed allocation is D377_ERR_HIP with text
  // `no_memory`, a format that is given the bytes asked of hipMalloc (%zu, if it wants them).  A failure leaves the area
  // unchanged or {null, 0}, never naming a block it no longer owns.
  int reserve(ScratchGuard& g, hipStream_t s, size_t bytes, Slack slack, const char* in_capture, const char* no_memory) {
    if (bytes <= cap) return D377_OK;
    if (ScratchGuard::capturing(s)) return fail(D377_ERR_ARG, "%s", in_capture);
    int rc;
    if ((rc = g.drain())) return rc;                         // a launch on another stream may still be using the old block
    void* old = mem;
    mem = nullptr; cap = 0;
    if (old && g.seen_capture) g.retired.push_back(old);     // a captured graph may still point into it
    else if (old) HIP_TRY(hipFree(old));
    const size_t want = bytes + (slack.div ? bytes / slack.div : 0) + slack.add;
    if (hipMalloc(&mem, want) != hipSuccess) {
      (void)hipGetLastError();                               // (the runtime's sticky error)
      mem = nullptr;
      snprintf(d377_g_err, sizeof d377_g_err, no_memory, want);
      return D377_ERR_HIP;
    }
    cap = want;
    return D377_OK;
  }
  void release() { (void)hipFree(mem); mem = nullptr; cap = 0; }   // with the context, after the guard has been drained
};

}  // namespace d377
