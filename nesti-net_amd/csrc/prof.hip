// Optional per-category kernel timing with hipEvents on the launch stream (common.h: prof_phase / prof_begin / prof_end; bench.py's
// roofline leg reads it through nesti_profile_enable / nesti_profile_read).  No forward path depends on it: switched off, prof_begin
// returns -1 and prof_end does nothing.
#include <mutex>
#include <vector>

#include "common.h"

namespace nesti {

constexpr int kProfSlots = NESTI_PROF_PHASES * NESTI_PROF_CATEGORIES;   // slot = phase * NESTI_PROF_CATEGORIES + category
struct ProfState {
  bool on = false;
  int phase = NESTI_PHASE_INPUT;     // set by the forward path (prof_phase); launches are booked under it
  std::vector<hipEvent_t> pool;      // recycled events
  std::vector<std::pair<hipEvent_t, hipEvent_t>> spans[kProfSlots];
  double ms[kProfSlots] = {0};
  long long launches[kProfSlots] = {0};
};
static ProfState g_prof;
static std::mutex g_prof_mu;   // forward calls may come from several host threads (one stream each)

static hipEvent_t prof_event() {
  if (!g_prof.pool.empty()) { hipEvent_t e = g_prof.pool.back(); g_prof.pool.pop_back(); return e; }
  hipEvent_t e = nullptr;
  (void)hipEventCreate(&e);
  return e;
}
bool stream_capturing(hipStream_t st) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(st, &cs) != hipSuccess) { (void)hipGetLastError(); return false; }
  return cs != hipStreamCaptureStatusNone;
}
void prof_phase(int phase) { if (g_prof.on) g_prof.phase = phase; }
// prof_begin returns a token for prof_end (-1: nothing recorded): slot * 2^20 + index of the span within the slot.  A stream that is
// being captured into a hipGraph records nothing: events captured into a graph cannot be synchronised on or timed afterwards.
int prof_begin(int cat, hipStream_t st) {
  if (!g_prof.on || stream_capturing(st)) return -1;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  // the input kernels are launched between forward passes, whatever phase the last one ended in
  const int phase = (cat == NESTI_PROF_MUPS || cat == NESTI_PROF_PATCHES) ? NESTI_PHASE_INPUT : g_prof.phase;
  const int slot = phase * NESTI_PROF_CATEGORIES + cat;
  if (g_prof.spans[slot].size() >= (1u << 20)) return -1;
  hipEvent_t a = prof_event(), b = prof_event();
  (void)hipEventRecord(a, st);
  g_prof.spans[slot].push_back({a, b});
  return (slot << 20) | ((int)g_prof.spans[slot].size() - 1);
}
void prof_end(int, int token, hipStream_t st) {
  if (token < 0) return;
  std::lock_guard<std::mutex> lk(g_prof_mu);
  const int slot = token >> 20, idx = token & ((1 << 20) - 1);
  if (slot < kProfSlots && idx < (int)g_prof.spans[slot].size()) (void)hipEventRecord(g_prof.spans[slot][idx].second, st);
}
static void prof_collect() {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  for (int c = 0; c < kProfSlots; ++c) {
    for (auto& sp : g_prof.spans[c]) {
      (void)hipEventSynchronize(sp.second);
      float ms = 0.f;
      if (hipEventElapsedTime(&ms, sp.first, sp.second) == hipSuccess) g_prof.ms[c] += ms;
      g_prof.launches[c] += 1;
      g_prof.pool.push_back(sp.first);
      g_prof.pool.push_back(sp.second);
    }
    g_prof.spans[c].clear();
  }
}

}  // namespace nesti

using namespace nesti;

extern "C" {

int nesti_profile_enable(int on) {
  prof_collect();
  for (int c = 0; c < kProfSlots; ++c) { g_prof.ms[c] = 0; g_prof.launches[c] = 0; }
  g_prof.on = on != 0;
  g_prof.phase = NESTI_PHASE_INPUT;
  return 0;
}

int nesti_profile_read(double* ms, long long* launches) {
  prof_collect();   // synchronises on the recorded events
  for (int c = 0; c < kProfSlots; ++c) {
    if (ms) ms[c] = g_prof.ms[c];
    if (launches) launches[c] = g_prof.launches[c];
  }
  return 0;
}

}  // extern "C"
