// The protocol of the guarded scratch areas (decaf377_amd/csrc/scratch_area.hpp: ScratchGuard, GuardScope, ScratchArea) on the
// host, against a fake runtime: no GPU and no HIP library.  This file defines the few runtime entry points the header calls;
// malloc/free back the fake blocks and events, so the -fsanitize=address,undefined build (tests/test_scratch_area_host.py
// builds both and runs them as ordinary programs) sees a double free or a leak.  Every call is logged; a capture flag and a
// "the next call of this name fails" switch are the only controls.  What the GPU tests cannot tell apart -- a drain from the
// wait hipFree performs on its own, a dangling pointer after a failed free -- is asserted here on the log and the fields.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <string>
#include <vector>

#include "scratch_area.hpp"

#define CHECK(c) do { if (!(c)) { std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); std::exit(1); } } while (0)

thread_local char d377_g_err[512];

// ---- the fake runtime ---------------------------------------------------------------------------------------------------------
namespace {
struct Call { std::string name; const void* arg; };
std::vector<Call> g_log;
std::set<const void*> g_live;                                  // blocks and events handed out and not yet given back
bool g_capturing = false;                                      // every stream is being captured
const char* g_fail_next = nullptr;                             // the next call of this name fails
hipError_t g_sticky = hipSuccess;

hipError_t called(const char* name, const void* arg) {
  g_log.push_back({name, arg});
  if (g_fail_next && !std::strcmp(g_fail_next, name)) { g_fail_next = nullptr; return g_sticky = hipErrorOutOfMemory; }
  return hipSuccess;
}
void* fake_new(size_t bytes) { void* p = std::malloc(bytes ? bytes : 1); CHECK(p); g_live.insert(p); return p; }
void fake_delete(const void* p) { CHECK(g_live.erase(p) == 1); std::free(const_cast<void*>(p)); }
}  // namespace

extern "C" {
hipError_t hipMalloc(void** p, size_t bytes) {
  hipError_t e = called("hipMalloc", (const void*)bytes);
  if (e == hipSuccess) *p = fake_new(bytes);
  return e;
}
hipError_t hipFree(void* p) {
  hipError_t e = called("hipFree", p);
  if (e == hipSuccess && p) fake_delete(p);
  return e;
}
hipError_t hipEventCreateWithFlags(hipEvent_t* ev, unsigned) {
  hipError_t e = called("hipEventCreateWithFlags", nullptr);
  if (e == hipSuccess) *ev = (hipEvent_t)fake_new(1);
  return e;
}
hipError_t hipEventDestroy(hipEvent_t ev) {
  hipError_t e = called("hipEventDestroy", ev);
  if (e == hipSuccess) fake_delete(ev);
  return e;
}
hipError_t hipEventRecord(hipEvent_t ev, hipStream_t) { return called("hipEventRecord", ev); }
hipError_t hipEventSynchronize(hipEvent_t ev) { return called("hipEventSynchronize", ev); }
hipError_t hipStreamWaitEvent(hipStream_t, hipEvent_t ev, unsigned) { return called("hipStreamWaitEvent", ev); }
hipError_t hipStreamIsCapturing(hipStream_t s, hipStreamCaptureStatus* st) {
  *st = g_capturing ? hipStreamCaptureStatusActive : hipStreamCaptureStatusNone;
  return called("hipStreamIsCapturing", s);
}
hipError_t hipGetLastError(void) { (void)called("hipGetLastError", nullptr); hipError_t e = g_sticky; g_sticky = hipSuccess; return e; }
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "fake failure"; }
}

// ---- the checks ---------------------------------------------------------------------------------------------------------------
using namespace d377;
namespace {
const hipStream_t S = (hipStream_t)0x40;
const char* IN_CAPTURE = "test: must grow inside a capture";
const char* NO_MEMORY = "test: no memory for %zu bytes";

// the log is exactly these names, in this order
bool log_is(std::initializer_list<const char*> names) {
  if (g_log.size() != names.size()) return false;
  size_t i = 0;
  for (const char* n : names) if (g_log[i++].name != n) return false;
  return true;
}
int count(const char* name, const void* arg) {
  int c = 0;
  for (const Call& k : g_log) c += k.name == name && k.arg == arg;
  return c;
}
int position(const char* name, const void* arg) {
  for (size_t i = 0; i < g_log.size(); ++i) if (g_log[i].name == name && g_log[i].arg == arg) return (int)i;
  return -1;
}
// one launch on the guard, as the launch functions do it: acquire, (the launch), finish
void use(ScratchGuard& g) { GuardScope sc{g, S}; CHECK(sc.acquire() == D377_OK); CHECK(sc.finish() == D377_OK); }

struct Fixture {                                               // a guard with its event, and nothing alive when it goes
  ScratchGuard g;
  Fixture() { g_log.clear(); g_capturing = false; g_fail_next = nullptr; g_sticky = hipSuccess; CHECK(g.init() == D377_OK); g_log.clear(); }
  ~Fixture() { g.destroy(); CHECK(g_live.empty()); }
};

void within_capacity() {                                       // 1
  Fixture f; ScratchArea a;
  CHECK(a.reserve(f.g, S, 1000, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_OK);
  void* p = a.mem;
  g_log.clear();
  for (size_t b : {(size_t)0, (size_t)1, (size_t)999, (size_t)1000})
    CHECK(a.reserve(f.g, S, b, SLACK_PARTIALS, IN_CAPTURE, NO_MEMORY) == D377_OK);
  CHECK(g_log.empty() && a.mem == p && a.cap == 1000);
  a.release();
}

void growth_used_guard() {                                     // 2: the capacities are the issue's table, as literals
  struct { Slack rule; size_t bytes, cap; } rows[] = {
    {SLACK_TABLE_SCRATCH, 5003, 5003}, {SLACK_TABLE_SCRATCH, 1048576, 1048576},       // b
    {SLACK_PARTIALS, 5003, 10349}, {SLACK_PARTIALS, 1048576, 1314816},                // b + b/4 + 4096
    {SLACK_MSM_WORKSPACE, 5003, 5628}, {SLACK_MSM_WORKSPACE, 1048576, 1179648}};      // b + b/8
  for (auto& r : rows) {
    Fixture f; ScratchArea a;
    CHECK(a.reserve(f.g, S, 16, r.rule, IN_CAPTURE, NO_MEMORY) == D377_OK);
    use(f.g);
    void* old = a.mem;
    g_log.clear();
    CHECK(a.reserve(f.g, S, r.bytes, r.rule, IN_CAPTURE, NO_MEMORY) == D377_OK);
    CHECK(log_is({"hipStreamIsCapturing", "hipEventSynchronize", "hipFree", "hipMalloc"}));
    CHECK(g_log[1].arg == f.g.ev && g_log[2].arg == old && g_log[3].arg == (const void*)r.cap);
    CHECK(a.cap == r.cap && g_live.count(a.mem) == 1 && g_live.size() == 2);   // the event and the new block (which may reuse the address)
    a.release();
  }
}

void growth_fresh_guard() {                                    // 3
  Fixture f; ScratchArea a;
  CHECK(a.reserve(f.g, S, 100, SLACK_MSM_WORKSPACE, IN_CAPTURE, NO_MEMORY) == D377_OK);
  CHECK(log_is({"hipStreamIsCapturing", "hipMalloc"}) && a.cap == 112);
  void* old = a.mem;
  g_log.clear();
  CHECK(a.reserve(f.g, S, 200, SLACK_MSM_WORKSPACE, IN_CAPTURE, NO_MEMORY) == D377_OK);   // still unused: freed without a wait
  CHECK(log_is({"hipStreamIsCapturing", "hipFree", "hipMalloc"}) && g_log[1].arg == old && a.cap == 225);
  a.release();
}

void growth_after_capture() {                                  // 4
  void *first, *second;
  {
    Fixture f; ScratchArea a;
    CHECK(a.reserve(f.g, S, 100, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_OK);
    g_capturing = true;
    use(f.g);                                                  // a captured launch: the graph now names a.mem
    g_capturing = false;
    CHECK(f.g.seen_capture && !f.g.used);
    first = a.mem;
    g_log.clear();
    CHECK(a.reserve(f.g, S, 200, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_OK);
    CHECK(log_is({"hipStreamIsCapturing", "hipMalloc"}));
    CHECK(f.g.retired == std::vector<void*>{first} && g_live.count(first) == 1);
    second = a.mem;
    CHECK(a.reserve(f.g, S, 300, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_OK);
    CHECK((f.g.retired == std::vector<void*>{first, second}) && count("hipFree", first) == 0 && count("hipFree", second) == 0);
    a.release();
    g_log.clear();
  }                                                            // the guard's destroy()
  CHECK(count("hipFree", first) == 1 && count("hipFree", second) == 1);
}

void growth_refused_in_capture() {                             // 5
  Fixture f; ScratchArea a;
  CHECK(a.reserve(f.g, S, 100, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_OK);
  use(f.g);
  void* p = a.mem;
  g_capturing = true;
  g_log.clear();
  d377_g_err[0] = 0;
  CHECK(a.reserve(f.g, S, 101, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_ERR_ARG);
  CHECK(!std::strcmp(d377_g_err, IN_CAPTURE));
  CHECK(log_is({"hipStreamIsCapturing"}) && a.mem == p && a.cap == 100);
  g_log.clear();
  CHECK(a.reserve(f.g, S, 100, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_OK && g_log.empty() && a.mem == p);
  a.release();
}

void malloc_fails(bool captured) {                             // 6: the old block freed, or retired, exactly once
  Fixture f; ScratchArea a;
  CHECK(a.reserve(f.g, S, 100, SLACK_PARTIALS, IN_CAPTURE, NO_MEMORY) == D377_OK);
  g_capturing = captured;
  use(f.g);
  g_capturing = false;
  void* old = a.mem;
  g_log.clear();
  g_fail_next = "hipMalloc";
  d377_g_err[0] = 0;
  CHECK(a.reserve(f.g, S, 8000, SLACK_PARTIALS, IN_CAPTURE, NO_MEMORY) == D377_ERR_HIP);
  CHECK(!std::strcmp(d377_g_err, "test: no memory for 14096 bytes"));
  CHECK(a.mem == nullptr && a.cap == 0);
  CHECK(g_sticky == hipSuccess && position("hipGetLastError", nullptr) > position("hipMalloc", (const void*)14096));
  CHECK(count("hipFree", old) == (captured ? 0 : 1));
  CHECK(f.g.retired == (captured ? std::vector<void*>{old} : std::vector<void*>{}));
  g_log.clear();
  CHECK(a.reserve(f.g, S, 8000, SLACK_PARTIALS, IN_CAPTURE, NO_MEMORY) == D377_OK);
  CHECK(captured ? log_is({"hipStreamIsCapturing", "hipMalloc"}) : log_is({"hipStreamIsCapturing", "hipEventSynchronize", "hipMalloc"}));
  CHECK(a.mem && a.cap == 14096);                              // (nothing was left to free)
  a.release();
}

void free_fails() {                                            // 7
  Fixture f; ScratchArea a;
  CHECK(a.reserve(f.g, S, 100, SLACK_MSM_WORKSPACE, IN_CAPTURE, NO_MEMORY) == D377_OK);
  use(f.g);
  void* old = a.mem;
  g_fail_next = "hipFree";
  CHECK(a.reserve(f.g, S, 1000, SLACK_MSM_WORKSPACE, IN_CAPTURE, NO_MEMORY) == D377_ERR_HIP);
  CHECK(a.mem == nullptr && a.cap == 0);
  CHECK(a.reserve(f.g, S, 1000, SLACK_MSM_WORKSPACE, IN_CAPTURE, NO_MEMORY) == D377_OK && a.mem != old && a.cap == 1125);
  a.release();
  fake_delete(old);                                            // (the fake runtime kept it: its free failed)
}

void guard_scope() {                                           // 8
  Fixture f;
  { GuardScope sc{f.g, S}; }                                   // never acquired
  CHECK(g_log.empty() && !f.g.used);
  {
    GuardScope sc{f.g, S};
    CHECK(sc.acquire() == D377_OK);                            // an unused guard: nothing to wait for
    CHECK(log_is({"hipStreamIsCapturing"}));
    CHECK(sc.finish() == D377_OK);
    CHECK(log_is({"hipStreamIsCapturing", "hipStreamIsCapturing", "hipEventRecord"}) && g_log[2].arg == f.g.ev && f.g.used);
  }
  CHECK(g_log.size() == 3);                                    // finished: the destructor records nothing more
  g_log.clear();
  {
    GuardScope sc{f.g, S};
    CHECK(sc.acquire() == D377_OK);                            // a used guard: the stream waits on the event
    CHECK(log_is({"hipStreamIsCapturing", "hipStreamWaitEvent"}) && g_log[1].arg == f.g.ev);
  }                                                            // left without finish(): an error path
  CHECK(log_is({"hipStreamIsCapturing", "hipStreamWaitEvent", "hipStreamIsCapturing", "hipEventRecord"}));
  g_log.clear();
  g_capturing = true;
  {
    GuardScope sc{f.g, S};
    CHECK(!f.g.seen_capture && sc.acquire() == D377_OK && f.g.seen_capture);
    CHECK(sc.finish() == D377_OK);
  }
  CHECK(log_is({"hipStreamIsCapturing", "hipStreamIsCapturing"}));   // neither waited nor recorded
}

void release_then_destroy() {                                  // 9: three areas on two guards, as a device holds them
  g_log.clear();
  g_capturing = false;
  ScratchGuard vb, msm;
  ScratchArea tab, partials, ws;
  CHECK(vb.init() == D377_OK && msm.init() == D377_OK);
  for (size_t b : {(size_t)100, (size_t)5000, (size_t)90000}) {
    CHECK(tab.reserve(vb, S, b, SLACK_TABLE_SCRATCH, IN_CAPTURE, NO_MEMORY) == D377_OK);
    CHECK(partials.reserve(vb, S, b, SLACK_PARTIALS, IN_CAPTURE, NO_MEMORY) == D377_OK);
    CHECK(ws.reserve(msm, S, b, SLACK_MSM_WORKSPACE, IN_CAPTURE, NO_MEMORY) == D377_OK);
    g_capturing = true;                                        // from the first round on, outgrown blocks are retired
    use(vb); use(msm);
    g_capturing = false;
    use(vb); use(msm);
  }
  CHECK(vb.retired.size() == 4 && msm.retired.size() == 2 && g_live.size() == 2 + 3 + 6);
  (void)vb.drain(); (void)msm.drain();
  tab.release(); partials.release(); ws.release();
  vb.destroy(); msm.destroy();
  CHECK(g_live.empty() && vb.retired.empty() && msm.retired.empty() && !tab.mem && !partials.mem && !ws.mem && !ws.cap);
  int mallocs = 0, frees = 0;
  for (const Call& k : g_log) {
    mallocs += k.name == "hipMalloc";
    frees += k.name == "hipFree" && k.arg;
    if (k.name == "hipFree" && k.arg) CHECK(count("hipFree", k.arg) == 1);
  }
  CHECK(mallocs == 9 && frees == 9);
  vb.destroy();                                                // a second destroy finds nothing
  CHECK(g_live.empty());
}
}  // namespace

int main() {
  within_capacity();
  growth_used_guard();
  growth_fresh_guard();
  growth_after_capture();
  growth_refused_in_capture();
  malloc_fails(false);
  malloc_fails(true);
  free_fails();
  guard_scope();
  release_then_destroy();
  std::printf("OK\n");
  return 0;
}
