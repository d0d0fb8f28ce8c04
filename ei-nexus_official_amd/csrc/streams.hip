// streams.hip -- the library's side streams (include/einx.h, "Side streams"): which stream runs beside which.
//
// HIP deals streams onto a few hardware queues (GPU_MAX_HW_QUEUES, 4 by default), and which one a stream got depends on everything
// the process created before it (torch's stream pool, a process group's streams, a loader's copy streams): under torchrun
// einx_stream_overlap_us(caller, fork stream) read 2.1 before streams were probed.  Per device and lane, a pool of streams that is
// never destroyed (destroying streams between hipGraph captures made hipGraphLaunch of ROCm 7.2 crash in hip::Graph::UpdateStreams,
// profiles/r06_notes.md 7) and a fixed table of slots whose events are created once and kept for every later key.
// g_table_mu guards keys, pool indices and use stamps, and is held only to find or claim a slot.  A slot's own mutex is held while
// its key is probed and while a call enqueues its fork .. join section (two host threads that fork from one stream cannot
// interleave on its events); a slot whose mutex is held is never re-keyed.  Probes of one device take turns on its probe_mu (two
// at once would measure each other).  Two slots may borrow one pool stream: their sections then run one after the other.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <mutex>
#include <vector>

#include "einx_common.h"

namespace {

struct Slot {
  hipStream_t caller = nullptr;
  int lane = -1;    // -1: no key
  int pool_i = -1;  // the lent pool stream; -1 while the key is being probed
  unsigned long long last_use = 0;
  EinxSide side;
  std::mutex mu;
};

struct Device {
  hipStream_t pool[2][EINX_FORK_STREAM_POOL] = {};  // one pool per lane: a fork stream is never lent as a lane-1 caller
  int n_pool[2] = {0, 0};                           // (created at a lane's first use, under probe_mu)
  Slot slots[EINX_FORK_STREAMS_MAX];
  std::mutex probe_mu;
};

std::mutex g_table_mu;
unsigned long long g_clock = 0;

std::map<int, Device*>& devices() {  // called with g_table_mu held
  static std::map<int, Device*>* devs = new std::map<int, Device*>();  // (never destructed: no HIP calls at process exit)
  return *devs;
}

Device& device(int dev) {
  Device*& d = devices()[dev];
  if (!d) d = new Device();
  return *d;
}

bool stream_device(hipStream_t stream, int* dev) {  // the stream's OWN device, not the current one
  return (stream ? hipStreamGetDevice(stream, dev) : hipGetDevice(dev)) == hipSuccess;
}

// The stream of its lane's pool for slot `self` of `caller`: one that runs BESIDE it.  The pool's streams are tried, least borrowed
// first (ties: pool order), until one overlaps with the caller and, if possible, with the streams the host names (`beside`) and
// the streams of the two most recently used other slots of the device; the cheapest is lent.  Skipped (least borrowed stream taken) while the
// caller is capturing.  A few hundred microseconds per stream tried, once per key.  Called with self->mu and D.probe_mu held and
// the slot's device current.
constexpr int kProbeSpinUs = 100;
int pick_side_stream(Device& D, const Slot* self, hipStream_t caller, void* const* beside, int n_beside) {
  static const bool debug = getenv("EINX_DEBUG_STREAMS") != nullptr;
  static const bool no_probe = getenv("EINX_NO_STREAM_PROBE") != nullptr;  // (diagnostics: no probe, least borrowed stream)
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  const bool probe = !no_probe && hipStreamIsCapturing(caller, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone;
  if (!probe) (void)hipGetLastError();
  // peers: (stream, weight) -- the caller first
  std::vector<std::pair<hipStream_t, int>> peers;
  peers.push_back({caller, 8});
  for (int i = 0; probe && i < n_beside; ++i)
    if ((hipStream_t)beside[i] != caller) peers.push_back({(hipStream_t)beside[i], 2});
  const int np = D.n_pool[self->lane];
  const hipStream_t* pool = D.pool[self->lane];
  int borrowed[EINX_FORK_STREAM_POOL] = {};
  {
    std::lock_guard<std::mutex> tl(g_table_mu);
    const Slot* recent[2] = {nullptr, nullptr};
    for (const Slot& s : D.slots) {
      if (s.lane < 0 || s.pool_i < 0) continue;
      if (s.lane == self->lane) ++borrowed[s.pool_i];
      if (&s == self) continue;
      if (!recent[0] || s.last_use > recent[0]->last_use) {
        recent[1] = recent[0];
        recent[0] = &s;
      } else if (!recent[1] || s.last_use > recent[1]->last_use) {
        recent[1] = &s;
      }
    }
    for (int k = 0; probe && k < 2 && recent[k]; ++k) {
      bool have = false;
      for (const std::pair<hipStream_t, int>& pr : peers) have = have || pr.first == recent[k]->side.stream;
      if (!have) peers.push_back({recent[k]->side.stream, 2});
    }
  }
  int order[EINX_FORK_STREAM_POOL];
  for (int i = 0; i < np; ++i) order[i] = i;
  std::stable_sort(order, order + np, [&](int x, int y) { return borrowed[x] < borrowed[y]; });
  int best_i = -1, best_cost = 1 << 30;
  for (int c = 0; c < np; ++c) {
    hipStream_t st = pool[order[c]];
    if (st == caller) continue;
    int cost = 0;
    if (probe) {
      for (const std::pair<hipStream_t, int>& pr : peers) {
        if (pr.first == st) {  // a stream the side has to stay clear of IS this pool stream
          cost += 4 * pr.second;
          continue;
        }
        float us = 0.f;
        if (einx_stream_overlap_us((void*)pr.first, (void*)st, kProbeSpinUs, &us) != EINX_OK) continue;  // (no verdict: no cost)
        const float ratio = us / kProbeSpinUs;
        cost += ratio > 1.6f ? 4 * pr.second : ratio > 1.25f ? pr.second : 0;  // one queue / (probably) one pipe
        if (debug) fprintf(stderr, "[einx streams] caller %p pool stream %d (%p) vs %p: %.2f\n", (void*)caller, order[c], (void*)st, (void*)pr.first, ratio);
      }
    }
    if (debug) fprintf(stderr, "[einx streams] caller %p pool stream %d cost %d (borrowed by %d)\n", (void*)caller, order[c], cost, borrowed[order[c]]);
    if (cost < best_cost) {
      best_cost = cost;
      best_i = order[c];
    }
    if (cost == 0) break;
  }
  return best_i;
}

// The slot of (caller, lane), locked in *lock; a new key is probed first.  NULL: every slot of the device is held, or the pool
// stream / events could not be created.
Slot* claim(hipStream_t caller, int lane, void* const* beside, int n_beside, std::unique_lock<std::mutex>* lock) {
  int dev = 0;
  if (!stream_device(caller, &dev)) return nullptr;
  std::unique_lock<std::mutex> tl(g_table_mu);
  Device& D = device(dev);
  for (;;) {
    Slot* s = nullptr;
    for (Slot& c : D.slots)
      if (c.lane == lane && c.caller == caller) s = &c;
    if (!s) break;
    tl.unlock();
    std::unique_lock<std::mutex> sl(s->mu);
    tl.lock();
    if (s->lane == lane && s->caller == caller) {  // (a key is only left unprobed while its slot is held)
      s->last_use = ++g_clock;
      *lock = std::move(sl);
      return s;
    }
  }
  // a new key: a free slot, else the least recently used one that nobody holds
  Slot* s = nullptr;
  auto age = [](const Slot& c) { return c.lane < 0 ? 0ull : c.last_use; };
  for (Slot& c : D.slots)
    if ((!s || age(c) < age(*s)) && c.mu.try_lock()) {
      if (s) s->mu.unlock();
      s = &c;
    }
  if (!s) return nullptr;
  std::unique_lock<std::mutex> sl(s->mu, std::adopt_lock);
  s->caller = caller;
  s->lane = lane;
  s->pool_i = -1;
  s->side.stream = nullptr;
  s->last_use = ++g_clock;
  tl.unlock();
  int pool_i = -1;
  {
    std::lock_guard<std::mutex> pl(D.probe_mu);
    int cur = 0;
    const bool sw = hipGetDevice(&cur) == hipSuccess && cur != dev;
    if (sw) (void)hipSetDevice(dev);
    int& np = D.n_pool[lane];
    if (np == 0) {
      while (np < EINX_FORK_STREAM_POOL && hipStreamCreateWithFlags(&D.pool[lane][np], hipStreamNonBlocking) == hipSuccess) ++np;
      if (np < EINX_FORK_STREAM_POOL) (void)hipGetLastError();
    }
    const bool events = (s->side.fork || hipEventCreateWithFlags(&s->side.fork, hipEventDisableTiming) == hipSuccess) &&
                        (s->side.join || hipEventCreateWithFlags(&s->side.join, hipEventDisableTiming) == hipSuccess);
    if (events && np > 0) pool_i = pick_side_stream(D, s, caller, beside, n_beside);
    if (sw) (void)hipSetDevice(cur);
  }
  tl.lock();
  if (pool_i < 0) {
    s->lane = -1;
    return nullptr;
  }
  s->pool_i = pool_i;
  s->side.stream = D.pool[lane][pool_i];
  *lock = std::move(sl);
  return s;
}

}  // namespace

const EinxSide* einx_side_acquire(hipStream_t caller, std::unique_lock<std::mutex>* lock) {
  const Slot* s = claim(caller, 0, nullptr, 0, lock);
  return s ? &s->side : nullptr;
}

EINX_EXPORT void* einx_side_stream(void* stream, int lane, void* const* beside, int n_beside) {
  if (lane < 0 || lane > 1 || n_beside < 0 || n_beside > 8 || (!beside && n_beside != 0)) {
    einx_set_error("%s: lane 0 or 1, 0..8 streams to stay clear of", __func__);
    return nullptr;
  }
  std::unique_lock<std::mutex> lk;
  const Slot* s = claim((hipStream_t)stream, lane, beside, n_beside, &lk);
  if (!s) einx_set_error("%s: every slot of the device is busy, or the pool stream / events could not be created", __func__);
  return s ? (void*)s->side.stream : nullptr;
}

EINX_EXPORT int einx_fork_stream_prepare_beside(void* stream, void* const* beside, int n_beside) {
  EINX_CHECK_ARG(n_beside >= 0 && n_beside <= 8 && (beside || n_beside == 0), "0..8 streams to stay clear of");
  return einx_side_stream(stream, 0, beside, n_beside) ? EINX_OK : EINX_ERR_LAUNCH;
}

EINX_EXPORT int einx_fork_stream_prepare(void* stream) { return einx_fork_stream_prepare_beside(stream, nullptr, 0); }

EINX_EXPORT int einx_fork_stream_release(void* stream) {
  std::vector<Slot*> keyed;
  {
    std::lock_guard<std::mutex> tl(g_table_mu);
    for (const std::pair<const int, Device*>& d : devices())
      for (Slot& s : d.second->slots)
        if (s.lane >= 0 && s.caller == (hipStream_t)stream) keyed.push_back(&s);
  }
  for (Slot* s : keyed) {
    std::lock_guard<std::mutex> sl(s->mu);  // (after a section in flight on it)
    std::lock_guard<std::mutex> tl(g_table_mu);
    if (s->caller == (hipStream_t)stream) s->lane = -1;
  }
  return EINX_OK;
}

EINX_EXPORT void* einx_fork_stream_of(void* stream) {
  int dev = 0;
  if (!stream_device((hipStream_t)stream, &dev)) return nullptr;
  std::lock_guard<std::mutex> tl(g_table_mu);
  for (const Slot& s : device(dev).slots)
    if (s.lane == 0 && s.caller == (hipStream_t)stream) return (void*)s.side.stream;
  return nullptr;
}

EINX_EXPORT int einx_fork_stream_count(void) {
  std::lock_guard<std::mutex> tl(g_table_mu);
  int n = 0;
  for (const std::pair<const int, Device*>& d : devices())
    for (const Slot& s : d.second->slots) n += s.lane >= 0;
  return n;
}
