// edv_runtime.hip -- host runtime and C-ABI of libedv.so (include/edv.h):
// device contexts, streams and scratch, the device-resident, host-buffer
// (synchronous, field-ordered), asynchronous and pipelined paths, sharding and
// placement over devices.  Host code only: the kernels are in edv_verify.hip
// and edv_prep.hip, launched through edv_launch.h.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdlib.h>
#include <stdio.h>
#include <algorithm>
#include <atomic>
#include <mutex>
#include <new>
#include <thread>
#include <unistd.h>
#include <vector>
#include <string>

#include "edv_kernels.h"
#include "edv_hostplan.h"
#include "edv_launch.h"
#include "edv_ledger.h"
#include "edv_merkle.h"
#include "edv_tables.h"
#include "edv_selftest_cases.h"
#include "../../include/edv.h"

using namespace edv;

namespace {

// ------------------------------------------------------------ host runtime
thread_local std::string g_err;

int set_err(int code, const char* what, hipError_t e = hipSuccess) {
  char buf[256];
  if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
  else snprintf(buf, sizeof buf, "%s", what);
  g_err = buf;
  return code;
}
#define HIPOK(call, what)                                  \
  do {                                                     \
    hipError_t e_ = (call);                                \
    if (e_ != hipSuccess) return set_err(EDV_E_HIP, what, e_); \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  uint64_t cap = 0;
  int ensure(uint64_t bytes) {
    if (bytes <= cap) return 0;
    release();
    if (hipMalloc(&p, bytes) != hipSuccess) { p = nullptr; return set_err(EDV_E_OOM, "hipMalloc"); }
    cap = bytes;
    return 0;
  }
  void release() {  // the caller guarantees that nothing queued still uses it (edv_trim, edv_release)
    if (p) (void)hipFree(p);
    p = nullptr; cap = 0;
  }
};

// Pinned (page-locked, portable) host memory: staging of pageable inputs
struct PinnedBuf {
  void* p = nullptr;
  void* dev = nullptr;  // its device-side address (zero-copy), looked up once per allocation
  uint64_t cap = 0;
  int ensure(uint64_t bytes) {
    if (bytes <= cap) return 0;
    release();
    bytes = pinned_capacity(bytes);  // headroom: message bytes vary from call to call
    if (hipHostMalloc(&p, bytes, hipHostMallocPortable) != hipSuccess) {
      p = nullptr;
      return set_err(EDV_E_OOM, "hipHostMalloc");
    }
    cap = bytes;
    if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess) {
      (void)hipGetLastError();
      dev = nullptr;
    }
    return 0;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr; dev = nullptr; cap = 0;
  }
};

// Where a host path's n verdicts go (sink_open, sink_d2h, sink_deliver): the
// kernels write them to `dev`; they reach the page-locked `host` (the caller's
// buffer if pinned, else the library's) by themselves when zero_copy (`dev` is
// its device-side address), else by a D2H copy; a pageable `caller` buffer
// gets them by memcpy once they are in.
struct VerdictSink {
  uint8_t *caller = nullptr, *host = nullptr, *dev = nullptr;
  uint64_t n = 0;
  bool pinned = false, zero_copy = false;
};

// The host-path streams.  A shard larger than a chunk alternates its sub-batches
// over the first two (sub_split), so the H2D copy of one overlaps the kernels
// of the other; stream q uses scratch slots [q pmax, (q + 1) pmax).  The field
// path runs on hs[0] and spreads its message slices' hash sides over hs[1..3].
constexpr int kQ = 4;
// In-flight batches of the asynchronous host path per device: a Node keeps one
// per prod in flight, and a pool of nodes in one process (C5) one per node, so
// eight slots let up to eight callers overlap before a submission has to wait.
constexpr int kAsyncSlots = 8;
// An asynchronous batch of at most this many requests (a Node's prod carries a
// few hundred) runs on its slot's own stream with its slot's own scratch
// (~25 MB), so the small batches of several callers execute side by side on
// the GPU instead of queueing behind each other on one stream: a batch that
// small is one wave per SIMD on a few SIMDs, and its latency (one main-kernel
// walk, ~0.45 ms) is all it costs.  Larger batches share the chunk scratch.
constexpr uint64_t kSmallAsync = 8192;
// The latency path (edv_quad.hip: one launch, sixteen lanes per signature up to
// 4,096 requests, eight above) takes every batch of at most this many requests
// on the host paths and the device-resident path (edv_set_latency_path changes
// it per device; 0 = off).  Below one wave per SIMD the batch kernels' time is
// one lane's serial chain whatever n is; the latency kernels split each point
// operation over a quad of lanes.
// profiles/r06/latency_paths_s3.jsonl: faster than the batch kernels at every n up to 8,192;
// profiles/r06/quad_limit_s51.jsonl: the two-walk kernel at 12,288 / 16,384 requests 386 / 392 us
// against 569 / 567 for the batch kernels (two waves per SIMD), level at 20,480, behind at 32,768
constexpr uint64_t kQuadMaxDefault = 16384;
constexpr uint64_t kQuadMaxLimit = 16384;  // the quad kernel's per-signature table scratch grows with n (57 MB here)

// One set of per-chunk state buffers (ChunkState storage + bucket permutation)
// for `cap` signatures (~5.5 kB each: ~1.4 GB for a whole 2^18 chunk).  Sized
// by use, not up front: a set grows to the largest batch it has served (in
// steps of powers of two from 4,096, at most the chunk), so a Node verifying
// prods of a few hundred requests holds ~25 MB of it, not 1.4 GB.  The caller
// guarantees that no queued kernel still uses a set it grows (grow_state).
struct ChunkBufs {
  DevBuf atab, rtab, dig, alive;  // ChunkState storage
  DevBuf perm, bucket_ctr;  // length-bucket permutation of a chunk; histogram + cursors (one set per stream)
  uint64_t cap = 0;         // signatures the set holds (the row stride of dig / alive)
  bool fits(uint64_t need) const { return need <= cap; }
  int ensure(uint64_t need, uint64_t limit) {
    if (need <= cap) return 0;
    const uint64_t c = chunk_capacity(need, limit);
    if (atab.ensure(c * kAWords * 4) || rtab.ensure(c * kAWords * 4) || dig.ensure(c * kDigWords * 4) ||
        alive.ensure(3 * c) || perm.ensure(c * 4) || bucket_ctr.ensure(uint64_t(kQ) * 2 * kBuckets * 4)) {
      cap = 0;
      return EDV_E_OOM;
    }
    cap = c;
    return 0;
  }
  uint64_t bytes() const { return atab.cap + rtab.cap + dig.cap + alive.cap + perm.cap + bucket_ctr.cap; }
  void release() {
    for (DevBuf* b : {&atab, &rtab, &dig, &alive, &perm, &bucket_ctr}) b->release();
    cap = 0;
  }
};

// The Merkle buffers of a context (edv_hostplan.h names and sizes them), none
// allocated before the call that needs it.  `done` (mk_done) is recorded after
// the last kernel that used the scratch, on whatever stream; the next user and
// whoever grows it wait for it (as st_done).  The staging is a host form's under mu.
struct MerkleBufs {
  DevBuf b[kMerkleBufs];
  hipEvent_t done = nullptr;  // created by the first extend (launch_merkle)
  // the buffer as T*; with `need`: null where the call does not touch it
  template <class T = uint8_t>
  T* at(MerkleBuf i) const { return static_cast<T*>(b[i].p); }
  uint8_t* at(MerkleBuf i, const MerkleSizes& need) const { return need[i] ? at(i) : nullptr; }
  uint64_t bytes() const {
    uint64_t t = 0;
    for (const DevBuf& x : b) t += x.cap;
    return t;
  }
  void trim(const MerkleSizes& limit) {  // the caller guarantees what DevBuf::release asks
    for (int i = 0; i < kMerkleBufs; i++)
      if (b[i].cap > limit[i]) b[i].release();
  }
  // Grows what is smaller than the call needs.  What grew before a failure stays.
  int ensure(const MerkleSizes& need) {
    bool idle = !done;  // the scratch has no queued user (left)
    for (int i = 0; i < kMerkleBufs; i++) {
      if (need[i] <= b[i].cap) continue;
      if (!idle && (i == mk_roots || i == mk_fleafh || i == mk_fnodeh)) {
        HIPOK(hipEventSynchronize(done), "merkle scratch sync");
        idle = true;
      }
      if (b[i].ensure(need[i])) return EDV_E_OOM;
    }
    return 0;
  }
};

struct DevCtx {
  std::mutex mu;
  bool ready = false;
  std::atomic<bool> live{false};   // ready, readable without mu (placement, edv_context_count)
  std::atomic<int> running{0};     // synchronous calls placed here and not yet returned
  int dev = -1;                    // logical device (edv_* device index)
  int phys = -1;                   // HIP device it runs on
  hipStream_t stream = nullptr;    // the library stream (edv_stream)
  const int32_t* sb_compact = nullptr;  // the GPU's [S]B table sets this context holds (shared_tables / drop_tables)
  const int32_t* sb_large = nullptr;
  int policy = kTablesAuto;        // which set a batch uses (edv_set_table_policy; EDV_SB_TABLES at start)
  bool sb_failed = false;          // a build of the large set failed and is not retried (edv_table_state)
  int sb_err = 0;                  // why pick_tables had no set to give
  bool env_read = false;           // EDV_CHUNK applies to the first context only: edv_release keeps the settings
  int32_t* comb = nullptr;         // signer comb table, built on first edv_sign_* call
  uint64_t chunk = kChunkDefault;  // EDV_CHUNK overrides (tests exercise chunk seams)
  int length_buckets = 2;          // 0 never, 1 always, 2 auto (edv_set_length_buckets)
  uint64_t quad_max = kQuadMaxDefault;  // latency path up to this batch size (edv_set_latency_path)
  ChunkBufs st;                    // scratch of the ordinary paths
  // st_done: recorded after the last kernel that used `st`, on whatever stream
  // that was; every later user waits for it first, so launches on different
  // caller streams never share the scratch concurrently.
  hipEvent_t st_done = nullptr;
  // host path (edv_verify_batch)
  hipStream_t hs[kQ] = {};
  hipEvent_t hs_staged[kQ] = {};   // pinned slot q may be refilled once its H2D copies are done
  hipEvent_t hs_end[kQ] = {};
  // the field path: copies on hcp; part_copied: signatures, keys and offsets
  // are on the device; part_prepped: the bucket permutation is written
  hipStream_t hcp = nullptr;
  hipEvent_t part_copied = nullptr, part_prepped = nullptr;
  hipEvent_t slice_copied[kSlices] = {}, slice_hashed[kSlices] = {};
  int host_slices = 0;              // 0 = one slice per kMinSliceReqs requests
  // asynchronous host path (edv_verify_batch_async): kAsyncSlots slots used in turn,
  // H2D copies on hcp, kernels and the verdicts' D2H on hac, so the copies of
  // batch k+1 run while batch k computes
  struct AsyncSlot {
    DevBuf sigs, pks, msgs, off, acc, dig;
    PinnedBuf stage, acc_host, dig_host;
    hipEvent_t copied = nullptr, done = nullptr;
    int64_t ticket = -1;         // batch held by the slot, -1 = none
    VerdictSink verdicts;        // where the batch's verdicts go (async_complete hands them over)
    uint8_t* digests = nullptr;  // the caller's SHA-256 buffer (null: none asked for)
    uint64_t n = 0;
    bool dig_pinned = false;     // digests DMA'd straight into `digests`
    hipStream_t st = nullptr;    // small batches: copies, kernels and D2H all on this stream
    ChunkBufs cb;                // small batches: the slot's own chunk scratch (grown to the batch)
    DevBuf qtab;                 // latency-path batches: the quad kernel's table scratch
#ifdef EDV_MEASUREMENT_API
    bool injected = false;       // edv_test_fail_async: this batch launched nothing and fails
#endif
  };
  AsyncSlot as[kAsyncSlots];
  hipStream_t hac = nullptr;
  // tickets issued and failed (edv_ledger.h); a failed batch's slot drops it,
  // so nothing is copied into the caller's buffers afterwards
  AsyncLedger ledger;
  DevBuf sigs, pks, msgs, off, acc;
  DevBuf fblob;  // the field path's signatures | keys | offsets block when they arrive in one copy
  // latency path of the synchronous and device-resident calls: packed inputs
  // (one DMA) and the quad kernel's table scratch (ordered by st_done, like
  // the chunk scratch)
  DevBuf qblob, qtab;
  PinnedBuf qstage;
  PinnedBuf stage[kQ], acc_host;
  // Pipelined submission (edv_verify_batch_dev_pipelined): two state sets, a
  // prep stream and a main stream, so the prep kernel of batch k+1 runs on the
  // SIMDs beside the main kernel of batch k.  prep_done[b] orders main after its
  // prep; main_done[b] keeps the next prep from overwriting state set b early.
  bool pipe_ready = false;
  ChunkBufs pst[2];
  hipStream_t sp = nullptr, sm = nullptr;
  hipEvent_t prep_done[2] = {nullptr, nullptr}, main_done[2] = {nullptr, nullptr}, inputs_ready = nullptr;
  hipEvent_t perm_done[2] = {nullptr, nullptr};  // split prep: state set b's bucket permutation is written
  bool pending[2] = {false, false};
  int next = 0;
  MerkleBufs mk;                   // the Merkle extension, batched append and proof verification
#ifdef EDV_MEASUREMENT_API
  int64_t inject_fail = -1;        // edv_test_fail_async (libedv_measure.so only)
#endif
};

std::mutex g_mu;
std::vector<DevCtx*> g_ctx;
int g_ndev = -1;

// ---- the [S]B tables (the prep kernel's R side): one copy per GPU and shape
// in a process, shared by every logical device (EDV_VIRTUAL_DEVICES) mapped
// onto that GPU.  Which set a batch runs against is the device's policy
// (edv_set_table_policy, edv_tables.h), EDV_SB_TABLES until it is set:
//   auto (default)  the compact set (64 MiB) at context creation; the large
//                   set (3 GiB, 4 fewer additions per verify, +1 % at C2) once
//                   a batch of at least kLargeTablesMin requests arrives -- a
//                   Node verifying prods of a few hundred requests never
//                   allocates it (footprint)
//   compact         never the large set
//   large           the large set at context creation (the compact one never)
// A failed allocation of the large set leaves the compact one in use and is
// not tried again (DevCtx::sb_failed).  A context holds the sets it has used
// (DevCtx::sb_compact / sb_large); a set is freed when its last holder drops
// it (edv_trim, edv_release).
int sb_policy() {
  static const int p = [] {
    const char* e = getenv("EDV_SB_TABLES");
    if (e && !strcmp(e, "compact")) return int(kTablesCompact);
    if (e && !strcmp(e, "large")) return int(kTablesLarge);
    return int(kTablesAuto);
  }();
  return p;
}
struct SbSet {
  int phys;
  int bits;
  int32_t* p;
  uint64_t bytes;
  int holders;
};
std::mutex g_sb_mu;
std::vector<SbSet> g_sb;
// One more hold on the table set of shape sh on GPU phys (current device =
// phys), built on first use; nullptr (with the error set) if it cannot be
// allocated or built.  Contexts pair it with drop_tables; the measurement
// build's probes do not, so a set they have used stays for the process.
const int32_t* shared_tables(int phys, SbShape sh, hipStream_t s, int* err) {
  std::lock_guard<std::mutex> lk(g_sb_mu);
  for (SbSet& t : g_sb)
    if (t.phys == phys && t.bits == sh.bits) {
      t.holders++;
      return t.p;
    }
  const uint64_t bytes = sb_alloc_bytes(sh);
  int32_t* p = nullptr;
  if (hipMalloc(&p, bytes) != hipSuccess) {
    (void)hipGetLastError();
    *err = set_err(EDV_E_OOM, "hipMalloc [S]B tables");
    return nullptr;
  }
  hipError_t e = launch_btab_kernel(s, p, sh);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    (void)hipFree(p);
    *err = set_err(EDV_E_HIP, "[S]B table build", e);
    return nullptr;
  }
  g_sb.push_back({phys, sh.bits, p, bytes, 1});
  return p;
}
// Gives one hold back; the last one frees the set (current device = phys, and
// nothing queued by the caller still reads it).
void drop_tables(int phys, SbShape sh) {
  std::lock_guard<std::mutex> lk(g_sb_mu);
  for (size_t k = 0; k < g_sb.size(); k++) {
    SbSet& t = g_sb[k];
    if (t.phys != phys || t.bits != sh.bits) continue;
    if (--t.holders <= 0) {
      (void)hipFree(t.p);
      g_sb.erase(g_sb.begin() + k);
    }
    return;
  }
}
uint64_t shared_tables_bytes(int phys) {
  std::lock_guard<std::mutex> lk(g_sb_mu);
  uint64_t b = 0;
  for (const SbSet& t : g_sb)
    if (t.phys == phys) b += t.bytes;
  return b;
}

// Logical devices.  Normally one per visible HIP device.  EDV_VIRTUAL_DEVICES=k
// (testing knob) presents k logical devices mapped round-robin onto the
// physical ones, each with its own context, streams and buffers, so the
// multi-device host path (one thread per device, shard split, error
// propagation) runs on a one-GPU box exactly as it does on eight GPUs.
int device_count_locked() {
  if (g_ndev >= 0) return g_ndev;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); n = 0; }
  int logical = n;
  if (const char* e = getenv("EDV_VIRTUAL_DEVICES")) {
    const long v = strtol(e, nullptr, 10);
    if (n > 0 && v > 0 && v <= 32) logical = int(v);
  }
  g_ndev = logical;
  g_ctx.resize(logical, nullptr);
  for (int i = 0; i < logical; i++) {
    g_ctx[i] = new DevCtx();
    g_ctx[i]->dev = i;
    g_ctx[i]->phys = n > 0 ? i % n : 0;
    g_ctx[i]->policy = sb_policy();
  }
  return logical;
}

// Every stream and every event a context can hold, each list written once, for
// creation, destruction, drain and quiesce: f(object, lazy), lazy = created on
// first use by its path (a slot's stream, the pipeline's streams and events,
// the Merkle scratch's event) and null until then, the others by ctx_init.
template <class F>
void for_each_stream(DevCtx& c, F f) {
  f(c.stream, false);
  for (hipStream_t& s : c.hs) f(s, false);
  for (hipStream_t* s : {&c.hcp, &c.hac}) f(*s, false);
  for (auto& a : c.as) f(a.st, true);
  for (hipStream_t* s : {&c.sp, &c.sm}) f(*s, true);
}
template <class F>
void for_each_event(DevCtx& c, F f) {
  for (auto* set : {&c.hs_staged, &c.hs_end})
    for (hipEvent_t& e : *set) f(e, false);
  for (auto* set : {&c.slice_copied, &c.slice_hashed})
    for (hipEvent_t& e : *set) f(e, false);
  for (auto& a : c.as)
    for (hipEvent_t* e : {&a.copied, &a.done}) f(*e, false);
  for (hipEvent_t* e : {&c.part_copied, &c.part_prepped, &c.st_done}) f(*e, false);
  for (auto* set : {&c.prep_done, &c.main_done, &c.perm_done})
    for (hipEvent_t& e : *set) f(e, true);
  for (hipEvent_t* e : {&c.inputs_ready, &c.mk.done}) f(*e, true);
}

// Idempotent: a failure part-way leaves what was created in place and the next
// call resumes from there (no second stream or table per retry).
int ctx_init(DevCtx& c) {
  if (c.ready) return 0;
  HIPOK(hipSetDevice(c.phys), "hipSetDevice");
  hipDeviceProp_t prop;
  HIPOK(hipGetDeviceProperties(&prop, c.phys), "hipGetDeviceProperties");
  if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return set_err(EDV_E_NODEV, "device is not gfx950");
  hipError_t made = hipSuccess;
  for_each_stream(c, [&](hipStream_t& s, bool lazy) {
    if (made == hipSuccess && !lazy && !s) made = hipStreamCreateWithFlags(&s, hipStreamNonBlocking);
  });
  HIPOK(made, "hipStreamCreate");
  for_each_event(c, [&](hipEvent_t& ev, bool lazy) {
    if (made == hipSuccess && !lazy && !ev) made = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  });
  HIPOK(made, "event");
  if (const char* e = c.env_read ? nullptr : getenv("EDV_CHUNK")) {
    const uint64_t v = strtoull(e, nullptr, 10);
    if (v >= kBlock && v <= (uint64_t(1) << 24)) c.chunk = (v / kBlock) * kBlock;
  }
  c.env_read = true;
  // the scratch grows by use (ChunkBufs); the [S]B tables: the device's policy (pick_tables)
  int err = 0;
  if (c.policy == kTablesLarge) {
    if (!c.sb_large && !(c.sb_large = shared_tables(c.phys, sb_large(), c.stream, &err))) return err;
  } else if (!c.sb_compact && !(c.sb_compact = shared_tables(c.phys, sb_compact(), c.stream, &err))) {
    return err;
  }
  c.ready = true;
  c.live.store(true);
  return 0;
}

DevCtx* get_ctx(int dev, int* err) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int n = device_count_locked();
  if (dev < 0 || dev >= n) { *err = set_err(EDV_E_NODEV, "no such device"); return nullptr; }
  *err = 0;
  return g_ctx[dev];
}

// Lock a device's context, initialise it and make its HIP device current.
struct CtxLock {
  DevCtx* c = nullptr;
  std::unique_lock<std::mutex> lk;
  int err = 0;
  explicit CtxLock(int device) {
    c = get_ctx(device, &err);
    if (!c) return;
    lk = std::unique_lock<std::mutex>(c->mu);
    if ((err = ctx_init(*c))) return;
    if (hipSetDevice(c->phys) != hipSuccess) err = set_err(EDV_E_HIP, "hipSetDevice");
  }
};

int phys_of(int device, int* phys) {
  int err = 0;
  DevCtx* c = get_ctx(device, &err);
  if (!c) return err;
  *phys = c->phys;
  return 0;
}

// The [S]B table set a batch of n requests runs against: choose_tables
// (edv_tables.h) over the device's policy and the sets the context holds,
// building the one it asks for.  A failed build of the large set is kept in
// edv_last_error, marks the context (sb_failed: no further 3 GiB hipMalloc per
// batch) and leaves the batch on the compact set.  *t stays null, with the
// code in c.sb_err, only when no set can be had at all (no_tables).  Caller
// holds c.mu; the current device is c.phys.
void pick_tables(DevCtx& c, uint64_t n, const int32_t** t, SbShape* sh) {
  *t = nullptr;
  for (int round = 0; round < 2; round++) {
    const TableChoice ch = choose_tables(c.policy, n, c.sb_compact != nullptr, c.sb_large != nullptr, c.sb_failed);
    c.sb_failed = ch.failed;
    const bool large = ch.use == kSetLarge;
    const int32_t*& held = large ? c.sb_large : c.sb_compact;
    if (ch.build != kSetNone) {
      int err = 0;
      held = shared_tables(c.phys, large ? sb_large() : sb_compact(), c.stream, &err);
      if (!held) {
        c.sb_err = err;
        if (!large) return;
        c.sb_failed = true;  // ask again: the compact set
        continue;
      }
    }
    *t = held;
    *sh = large ? sb_large() : sb_compact();
    return;
  }
}
// The error of a launch for which pick_tables had no table set.
int no_tables(const DevCtx& c) { return c.sb_err ? c.sb_err : set_err(EDV_E_HIP, "no [S]B table set"); }

// Grow the context's ordinary chunk scratch to `need` signatures (at most one
// chunk's worth is ever used at once), after every queued user of it is done.
int grow_state(DevCtx& c, uint64_t need) {
  if (need > c.chunk) need = c.chunk;
  if (c.st.fits(need)) return 0;
  HIPOK(hipEventSynchronize(c.st_done), "scratch sync");
  return c.st.ensure(need, c.chunk);
}

VerifyArgs make_args(DevCtx& c, ChunkBufs& b, const uint8_t* d_sigs, const uint8_t* d_pks,
                     const uint8_t* d_msgs, const uint64_t* d_off, uint64_t msg_base, uint8_t* d_accept, bool bucket,
                     uint64_t slot0 = 0, uint64_t batch = 0) {
  VerifyArgs va;
  va.sigs = reinterpret_cast<const uint32_t*>(d_sigs);
  va.pks = reinterpret_cast<const uint32_t*>(d_pks);
  va.msgs = d_msgs;
  va.off = d_off;
  va.msg_base = msg_base;
  va.accept = d_accept;
  // slots [slot0, slot0 + n) of the chunk scratch (dig stays indexed w * cap + slot)
  va.st = ChunkState{static_cast<int32_t*>(b.atab.p) + slot0 * kAWords, static_cast<int32_t*>(b.rtab.p) + slot0 * kAWords,
                     static_cast<uint32_t*>(b.dig.p) + slot0,
                     static_cast<uint8_t*>(b.alive.p) + slot0, b.cap,
                     bucket ? static_cast<uint32_t*>(b.perm.p) + slot0 : nullptr};
  pick_tables(c, batch, &va.btab, &va.sb);
  va.base = 0;
  va.n = 0;
  va.side0 = 0;
  va.nsides = 3;
  return va;
}

// length buckets of one chunk on stream s (ctr: this stream's histogram + cursors)
int launch_buckets(uint32_t* ctr, const VerifyArgs& va, const uint64_t* d_off, hipStream_t s) {
  const unsigned blocks = unsigned((va.n + kBlock - 1) / kBlock);
  HIPOK(hipMemsetAsync(ctr, 0, 2 * kBuckets * 4, s), "memset buckets");
  HIPOK(launch_bucket_kernels(blocks, s, d_off, va.base, va.n, ctr, const_cast<uint32_t*>(va.st.perm)),
        "bucket launch");
  return 0;
}
// the prep kernel over the sides va.side0 .. va.side0 + va.nsides - 1
int launch_prep_sides(const VerifyArgs& va, hipStream_t s) {
#ifdef EDV_MEASURE_NO_VERIFY
  return 0;  // measurement build: see launch_main
#endif
  const unsigned blocks = unsigned((va.n + kBlock - 1) / kBlock);
  HIPOK(launch_prep_kernel(unsigned(va.nsides) * blocks, s, va), "prep launch");
  return 0;
}
// [length buckets,] prep kernel (all three sides) of one chunk on stream s
int launch_prep(uint32_t* ctr, const VerifyArgs& va, const uint64_t* d_off, bool bucket, hipStream_t s) {
#ifdef EDV_MEASURE_NO_VERIFY
  return 0;  // measurement build: see launch_main
#endif
  int err;
  if (bucket && (err = launch_buckets(ctr, va, d_off, s))) return err;
  return launch_prep_sides(va, s);  // hash, A and R sides
}
int launch_main(const VerifyArgs& va, hipStream_t s, bool prio = false) {
#ifdef EDV_MEASURE_NO_VERIFY
  // Measurement build only (variants/libedv_noverify.so, loaded by bench.py's
  // C5 leg through EDV_LIB in a separate process, never the product library):
  // every request of the chunk is reported valid without the verify kernels,
  // so a pool run can tell what verification costs from what everything around
  // it costs.  (A chunk's slots map onto accept[base, base + n), in any order.)
  HIPOK(hipMemsetAsync(va.accept + va.base, 1, va.n, s), "memset accept");
  return 0;
#endif
  const unsigned blocks = unsigned((va.n + kBlock - 1) / kBlock);
  HIPOK(launch_main_kernel(blocks, s, va, prio), "main launch");
  return 0;
}
uint32_t* bucket_ctr(ChunkBufs& b, int q) { return static_cast<uint32_t*>(b.bucket_ctr.p) + q * 2 * kBuckets; }

// Length buckets cost three small launches per chunk (memset, histogram,
// scatter).  Per call: EDV_FLAG_UNIFORM_LENGTH turns them off,
// EDV_FLAG_BUCKETS forces them; otherwise the device mode decides
// (edv_set_length_buckets).  Verdicts never depend on it.
bool bucketing_enabled(const DevCtx& c, uint32_t flags) {
  if (flags & EDV_FLAG_UNIFORM_LENGTH) return false;
  if (flags & EDV_FLAG_BUCKETS) return true;
  return c.length_buckets != 0;
}

// ---- the latency path (edv_quad.hip)
// The quad kernel over n requests whose inputs are device pointers (offsets
// absolute, minus msg_base), verdicts to d_acc[0, n); qtab is this launch's
// scratch (the caller orders it against its previous user).
int launch_quad(DevCtx& c, DevBuf& qtab, const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                const uint64_t* d_off, uint64_t msg_base, uint64_t n, uint8_t* d_acc, hipStream_t s) {
  if (n == 0) return 0;
  // up to kRtlMax requests (one workgroup per CU): the right-to-left kernel, no
  // table scratch; above: the two-walk kernel over per-signature tables
  const bool rtl = n <= kRtlMax;
  // the last workgroup's 64 quads all write their tables, in range or not
  if (!rtl && qtab.ensure((n + 63) / 64 * 64 * kQSigWords * 4)) return EDV_E_OOM;
  VerifyArgs va;
  memset(&va, 0, sizeof va);
  va.sigs = reinterpret_cast<const uint32_t*>(d_sigs);
  va.pks = reinterpret_cast<const uint32_t*>(d_pks);
  va.msgs = d_msgs;
  va.off = d_off;
  va.msg_base = msg_base;
  va.base = 0;
  va.n = n;
  va.accept = d_acc;
  pick_tables(c, n, &va.btab, &va.sb);
  if (!va.btab) return no_tables(c);
#ifdef EDV_MEASURE_NO_VERIFY
  HIPOK(hipMemsetAsync(d_acc, 1, n, s), "memset accept");  // measurement build: see launch_main
  return 0;
#endif
  if (rtl) HIPOK(launch_rtl_kernel(s, va), "rtl launch");
  else HIPOK(launch_quad_kernel(s, va, static_cast<int32_t*>(qtab.p)), "quad launch");
  return 0;
}

// The chunk walk: requests [0, n) of va in chunks of `step` on stream s, per chunk [length buckets (ctr: this
// stream's histogram + cursors),] prep kernel, main kernel.  The caller orders the scratch (st_done).
int walk_chunks(uint32_t* ctr, VerifyArgs va, bool bucket, uint64_t n, uint64_t step, hipStream_t s) {
  int err;
  for (uint64_t base = 0; base < n; base += step) {
    va.base = base;
    va.n = (n - base) < step ? (n - base) : step;
    if ((err = launch_prep(ctr, va, va.off, bucket, s)) || (err = launch_main(va, s))) return err;
  }
  return 0;
}

// Ordinary device path: launch on stream s; caller holds c.mu.  The batch is
// walked in chunks of c.chunk signatures (walk_chunks), after every earlier
// user of the scratch.
int launch(DevCtx& c, const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs, const uint64_t* d_off,
           uint64_t msg_base, uint64_t n, uint8_t* d_accept, hipStream_t s, uint32_t flags) {
  if (n == 0) return 0;
  const bool bucket = bucketing_enabled(c, flags);
  int err;
  if (n <= c.quad_max) {  // the latency path, its scratch ordered like the chunk scratch
    HIPOK(hipStreamWaitEvent(s, c.st_done, 0), "wait scratch");
    if ((err = launch_quad(c, c.qtab, d_sigs, d_pks, d_msgs, d_off, msg_base, n, d_accept, s))) return err;
    HIPOK(hipEventRecord(c.st_done, s), "record scratch");
    return 0;
  }
  if ((err = grow_state(c, n))) return err;
  HIPOK(hipStreamWaitEvent(s, c.st_done, 0), "wait scratch");
  const VerifyArgs va = make_args(c, c.st, d_sigs, d_pks, d_msgs, d_off, msg_base, d_accept, bucket, 0, n);
  if (!va.btab) return no_tables(c);
  if ((err = walk_chunks(bucket_ctr(c.st, 0), va, bucket, n, c.chunk, s))) return err;
  HIPOK(hipEventRecord(c.st_done, s), "record scratch");
  return 0;
}

// A small asynchronous batch on its slot's own scratch (cb, grown to the batch
// by the caller once the slot's previous batch is complete) and stream: not
// ordered against the shared scratch, so batches of different slots run side by side.
int launch_own(DevCtx& c, ChunkBufs& cb, const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
               const uint64_t* d_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept, hipStream_t s,
               uint32_t flags) {
  if (n == 0) return 0;
  const bool bucket = bucketing_enabled(c, flags);
  const VerifyArgs va = make_args(c, cb, d_sigs, d_pks, d_msgs, d_off, msg_base, d_accept, bucket, 0, n);
  if (!va.btab) return no_tables(c);
  return walk_chunks(bucket_ctr(cb, 0), va, bucket, n, c.chunk < cb.cap ? c.chunk : cb.cap, s);
}

int pipe_init(DevCtx& c) {
  if (c.pipe_ready) return 0;
  if (!c.sp) HIPOK(hipStreamCreateWithFlags(&c.sp, hipStreamNonBlocking), "hipStreamCreate");
  if (!c.sm) HIPOK(hipStreamCreateWithFlags(&c.sm, hipStreamNonBlocking), "hipStreamCreate");
  for (int b = 0; b < 2; b++) {
    if (!c.prep_done[b]) HIPOK(hipEventCreateWithFlags(&c.prep_done[b], hipEventDisableTiming), "event");
    if (!c.main_done[b]) HIPOK(hipEventCreateWithFlags(&c.main_done[b], hipEventDisableTiming), "event");
    if (!c.perm_done[b]) HIPOK(hipEventCreateWithFlags(&c.perm_done[b], hipEventDisableTiming), "event");
  }
  if (!c.inputs_ready) HIPOK(hipEventCreateWithFlags(&c.inputs_ready, hipEventDisableTiming), "event");
  c.pipe_ready = true;
  return 0;
}

// Pipelined path: chunk k's prep goes on stream sp into state set k%2 (after
// the main kernel that last read that set), its main on stream sm after that
// prep.  Work already queued on the library stream (e.g. the batch signer)
// is ordered before the first prep.  Caller holds c.mu.
int launch_pipelined(DevCtx& c, const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                     const uint64_t* d_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept, uint32_t flags) {
  int err;
  if ((err = pipe_init(c))) return err;
  const bool bucket = bucketing_enabled(c, flags);
  const bool split = (flags & EDV_FLAG_SPLIT_PREP) != 0;
  HIPOK(hipEventRecord(c.inputs_ready, c.stream), "record");
  HIPOK(hipStreamWaitEvent(c.sp, c.inputs_ready, 0), "wait");
  if (split) HIPOK(hipStreamWaitEvent(c.sm, c.inputs_ready, 0), "wait");
  for (uint64_t base = 0; base < n; base += c.chunk) {
    const int b = c.next;
    c.next ^= 1;
    ChunkBufs& cb = c.pst[b];
    const uint64_t cn = (n - base) < c.chunk ? (n - base) : c.chunk;
    if (!cb.fits(cn)) {  // state set b grows: its last main kernel must be done
      if (c.pending[b]) HIPOK(hipEventSynchronize(c.main_done[b]), "pipeline sync");
      if (cb.ensure(cn, c.chunk)) return EDV_E_OOM;
    }
    VerifyArgs va = make_args(c, cb, d_sigs, d_pks, d_msgs, d_off, msg_base, d_accept, bucket, 0, n);
    if (!va.btab) return no_tables(c);
    va.base = base;
    va.n = cn;
    if (c.pending[b]) HIPOK(hipStreamWaitEvent(c.sp, c.main_done[b], 0), "wait");
    if (split) {
      // Split prep: the hash side (one latency-bound SHA-512 chain per lane,
      // light on issue) goes on sp, where it runs beside the main kernel of the
      // previous chunk; the two point sides (issue-bound exponentiations) go on
      // sm in front of this chunk's main kernel, which waits for the hash side.
      // State set b's previous main kernel ran on sm, so sm needs no wait for
      // it; sp waited for it above.
      if (bucket) {
        if ((err = launch_buckets(bucket_ctr(cb, 0), va, d_off, c.sp))) return err;
        HIPOK(hipEventRecord(c.perm_done[b], c.sp), "record");
        HIPOK(hipStreamWaitEvent(c.sm, c.perm_done[b], 0), "wait");
      }
      VerifyArgs vh = va, vp = va;
      vh.side0 = 0;
      vh.nsides = 1;
      vp.side0 = 1;
      vp.nsides = 2;
      if ((err = launch_prep_sides(vh, c.sp))) return err;
      HIPOK(hipEventRecord(c.prep_done[b], c.sp), "record");
      if ((err = launch_prep_sides(vp, c.sm))) return err;
      HIPOK(hipStreamWaitEvent(c.sm, c.prep_done[b], 0), "wait");
      if ((err = launch_main(va, c.sm, true))) return err;
      HIPOK(hipEventRecord(c.main_done[b], c.sm), "record");
      c.pending[b] = true;
      continue;
    }
    if ((err = launch_prep(bucket_ctr(cb, 0), va, d_off, bucket, c.sp))) return err;
    HIPOK(hipEventRecord(c.prep_done[b], c.sp), "record");
    HIPOK(hipStreamWaitEvent(c.sm, c.prep_done[b], 0), "wait");
    if ((err = launch_main(va, c.sm))) return err;
    HIPOK(hipEventRecord(c.main_done[b], c.sm), "record");
    c.pending[b] = true;
  }
  return 0;
}

// Drain every stream of the context (before scratch is reallocated).
// The scratch's users on caller streams are waited for through st_done and
// mk_done; asynchronous batches stay pending until edv_wait_async.  Returns
// the first error (nothing after it is waited for).
int drain(DevCtx& c) {
  hipError_t e = hipSuccess;
  for_each_stream(c, [&](hipStream_t& s, bool) {
    if (e == hipSuccess && s) e = hipStreamSynchronize(s);
  });
  HIPOK(e, "stream sync");
  HIPOK(hipEventSynchronize(c.st_done), "scratch sync");
  if (c.mk.done) HIPOK(hipEventSynchronize(c.mk.done), "merkle scratch sync");
  if (c.pipe_ready) c.pending[0] = c.pending[1] = false;
  return 0;
}

// Best effort after a failed host-path call: wait for whatever was already
// queued on the context's streams (copies may still read the caller's pinned
// buffers), so no DMA touches them after the error is returned.
void quiesce(DevCtx& c) {
  for_each_stream(c, [](hipStream_t& s, bool) {
    if (s) (void)hipStreamSynchronize(s);
  });
  (void)hipGetLastError();
}

// ---- host memory: pinned detection and a parallel staging copy
bool is_pinned(const void* p) {
  if (!p) return false;
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();  // pageable memory: not an error for us
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// ---- the verdict sink for n verdicts owed to `accept`.  Its host side: the
// caller's buffer if page-locked, else `own`, the path's pinned buffer.
int sink_host(VerdictSink& v, uint8_t* accept, uint64_t n, PinnedBuf& own) {
  v = VerdictSink{accept, nullptr, nullptr, n, is_pinned(accept), false};
  if (!v.pinned && own.ensure(n)) return EDV_E_OOM;
  v.host = v.pinned ? accept : static_cast<uint8_t*>(own.p);
  return 0;
}
// ... and the address the kernels write: the host side's own (cached for
// `own`, looked up for a page-locked `accept`), else `fallback`, ensured only then
int sink_open(VerdictSink& v, uint8_t* accept, uint64_t n, PinnedBuf& own, DevBuf& fallback) {
  if (sink_host(v, accept, n, own)) return EDV_E_OOM;
  void* zc = v.pinned ? nullptr : own.dev;
  if (v.pinned && (hipHostGetDevicePointer(&zc, accept, 0) != hipSuccess || !zc)) {
    (void)hipGetLastError();
    zc = nullptr;
  }
  if (!zc && fallback.ensure(n)) return EDV_E_OOM;
  v.zero_copy = zc != nullptr;
  v.dev = static_cast<uint8_t*>(zc ? zc : fallback.p);
  return 0;
}
// The D2H of the verdicts on stream s, behind the kernels, when they did not write the host memory themselves
int sink_d2h(const VerdictSink& v, hipStream_t s) {
  if (!v.zero_copy) HIPOK(hipMemcpyAsync(v.host, v.dev, v.n, hipMemcpyDeviceToHost, s), "d2h accept");
  return 0;
}
// After the sync: a pageable caller buffer gets its verdicts
void sink_deliver(const VerdictSink& v) {
  if (!v.pinned) memcpy(v.caller, v.host, v.n);
}

struct Seg {
  uint8_t* dst;
  const uint8_t* src;
  uint64_t n;
};
int copy_threads() {
  static const int t = [] {
    if (const char* e = getenv("EDV_COPY_THREADS")) {
      const long v = strtol(e, nullptr, 10);
      if (v >= 1 && v <= 64) return int(v);
    }
    const unsigned hw = std::thread::hardware_concurrency();
    return int(hw >= 16 ? 8 : (hw >= 2 ? hw / 2 : 1));
  }();
  return t;
}
// memcpy of several segments, split evenly by bytes over up to copy_threads()
// threads (a single thread below 4 MiB)
void par_copy(const std::vector<Seg>& segs) {
  uint64_t total = 0;
  for (const Seg& s : segs) total += s.n;
  const int T = total < (uint64_t(4) << 20) ? 1 : copy_threads();
  auto part = [&](int t) {
    const uint64_t lo = total * t / T, hi = total * (t + 1) / T;
    uint64_t pos = 0;
    for (const Seg& s : segs) {
      const uint64_t a = lo > pos ? lo - pos : 0, b = hi - pos < s.n ? hi - pos : s.n;
      if (hi > pos && a < b && a < s.n) memcpy(s.dst + a, s.src + a, b - a);
      pos += s.n;
      if (pos >= hi) break;
    }
  };
  if (T == 1) { part(0); return; }
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(part, t);
  part(0);
  for (auto& x : th) x.join();
}

// ---- the input stager: requests [lo, hi) of a caller's batch onto the device.
// Where the four parts are read from: the caller's memory, or the pinned
// staging once stage_inputs has packed them there.  The offsets stay absolute
// (msg_base = mbase).
struct HostIn {
  const uint8_t *sigs, *pks, *off, *msgs;  // of request lo
  uint64_t n, mbase, mbytes;
};
HostIn host_in(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, uint64_t lo,
               uint64_t hi) {
  return {sigs + 64 * lo, pks + 32 * lo,    reinterpret_cast<const uint8_t*>(off + lo), msgs + off[lo],
          hi - lo,        off[lo],          off[hi] - off[lo]};
}
// Page-locked inputs (the native authenticator's arena, edv_host_alloc) are
// DMA'd straight from the caller's memory: no host copy on the Node's thread.
bool inputs_pinned(const HostIn& h) {
  return is_pinned(h.sigs) && is_pinned(h.pks) && is_pinned(h.off) && (h.mbytes == 0 || is_pinned(h.msgs));
}
// Pageable inputs are packed into pinned staging (packed_layout, the read
// slack zeroed), where h reads them afterwards; without the messages, their
// place is left for the caller to fill (stage_and_send) and h.msgs stays the
// caller's.  The staging's previous user is done (the caller's to know).
int stage_inputs(PinnedBuf& stage, HostIn& h, bool with_msgs) {
  const PackedLayout l = packed_layout(h.n, h.mbytes);
  if (stage.ensure(l.padded)) return EDV_E_OOM;
  uint8_t* p = static_cast<uint8_t*>(stage.p);
  par_copy({{p, h.sigs, 64 * h.n}, {p + l.pks, h.pks, 32 * h.n}, {p + l.off, h.off, 8 * (h.n + 1)},
            {p + l.msgs, h.msgs, with_msgs ? h.mbytes : 0}});
  memset(p + l.bytes, 0, kReadSlack);
  h = {p, p + l.pks, p + l.off, with_msgs ? p + l.msgs : h.msgs, h.n, h.mbase, h.mbytes};
  return 0;
}
// Do h's signatures, keys and offsets go in one copy?  (Once staged, or packed by the caller into one pinned buffer.)
OneSpan input_span(const HostIn& h) {
  return one_span(reinterpret_cast<uintptr_t>(h.sigs), reinterpret_cast<uintptr_t>(h.pks),
                  reinterpret_cast<uintptr_t>(h.off), h.n);
}
// h to the device on stream s.  The fixed part (signatures, keys, offsets): ONE
// copy of `span` bytes to d_sigs, a block laid out as the host region
// (input_span), when `one`, else three; each separate copy costs the DMA engine
// a gap (~12 us, trace_sync).  Then the messages in one copy, unless d_msgs is
// null: the field path sends them in slices.
int upload(const HostIn& h, bool one, uint64_t span, void* d_sigs, void* d_pks, void* d_off, void* d_msgs,
           hipStream_t s) {
  if (one) {
    HIPOK(hipMemcpyAsync(d_sigs, h.sigs, span, hipMemcpyHostToDevice, s), "h2d sigs+pks+off");
  } else {
    HIPOK(hipMemcpyAsync(d_sigs, h.sigs, 64 * h.n, hipMemcpyHostToDevice, s), "h2d sigs");
    HIPOK(hipMemcpyAsync(d_pks, h.pks, 32 * h.n, hipMemcpyHostToDevice, s), "h2d pks");
    HIPOK(hipMemcpyAsync(d_off, h.off, 8 * (h.n + 1), hipMemcpyHostToDevice, s), "h2d off");
  }
  if (d_msgs && h.mbytes) HIPOK(hipMemcpyAsync(d_msgs, h.msgs, h.mbytes, hipMemcpyHostToDevice, s), "h2d msgs");
  return 0;
}

// Pageable inputs of a latency-path batch are packed into page-locked staging
// anyway; the quad kernel then reads them from there over PCIe (its phase 1
// reads each input once, at its start) instead of waiting for a DMA of them:
// EDV_QUAD_ZERO_COPY=0 turns that off (A/B).
bool quad_zero_copy() {
  static const bool on = [] {
    const char* e = getenv("EDV_QUAD_ZERO_COPY");
    return !(e && !strcmp(e, "0"));
  }();
  return on;
}
// Device pointers of a batch's inputs
struct DevIn {
  const uint8_t *sigs, *pks, *msgs;
  const uint64_t* off;
};
// ... in a block at b with the keys at gp, the offsets at go, the messages at gm
DevIn dev_in_at(const void* b, uint64_t gp, uint64_t go, uint64_t gm) {
  const uint8_t* p = static_cast<const uint8_t*>(b);
  return {p, p + gp, p + gm, reinterpret_cast<const uint64_t*>(p + go)};
}
// Inputs h of a latency-path batch for the quad kernel, on stream s: pageable
// ones are packed into the pinned `stage` and read there by the kernel, or
// (EDV_QUAD_ZERO_COPY=0) copied from there in ONE DMA; page-locked ones go
// into device buffer `blob`, the fixed part in one copy when it lies in one region.
int quad_upload(DevBuf& blob, PinnedBuf& stage, HostIn h, hipStream_t s, DevIn* d) {
  int err;
  if (!inputs_pinned(h)) {
    if ((err = stage_inputs(stage, h, true))) return err;
    const PackedLayout l = packed_layout(h.n, h.mbytes);
    const bool in_place = quad_zero_copy() && stage.dev;  // the staging's previous user is done
    if (!in_place) {  // the whole packed block, messages and slack included, in ONE copy
      if (blob.ensure(l.padded)) return EDV_E_OOM;
      HIPOK(hipMemcpyAsync(blob.p, stage.p, l.padded, hipMemcpyHostToDevice, s), "h2d packed");
    }
    *d = dev_in_at(in_place ? stage.dev : blob.p, l.pks, l.off, l.msgs);
    return 0;
  }
  const OneSpan sp = input_span(h);
  const uint64_t moff = (sp.span + 15) / 16 * 16;
  if (blob.ensure(moff + h.mbytes + kReadSlack)) return EDV_E_OOM;
  uint8_t* b = static_cast<uint8_t*>(blob.p);
  *d = dev_in_at(b, sp.gp, sp.go, moff);
  return upload(h, sp.one, sp.span, b, b + sp.gp, b + sp.go, b + moff, s);
}
// memcpy of src[0, bounds[K]) into pinned staging over copy_threads() threads,
// part by part (part k = [bounds[k], bounds[k+1])), with part k's DMA to the
// device queued on stream s -- and ev[k], if given, recorded after it -- as
// soon as every thread has copied its share of it, so the staging of part k+1
// overlaps the DMA of part k (pageable inputs of a synchronous call: the
// messages, 71 % of a C2 batch's bytes).  A copy below 8 MiB is staged by one
// par_copy per part.
int stage_and_send(uint8_t* dev, uint8_t* stage, const uint8_t* src, const uint64_t* bounds, int K, hipStream_t s,
                   const hipEvent_t* ev) {
  const uint64_t bytes = bounds[K] - bounds[0];
  auto send = [&](int k) -> int {
    const uint64_t c0 = bounds[k], c1 = bounds[k + 1];
    if (c1 > c0) HIPOK(hipMemcpyAsync(dev + c0, stage + c0, c1 - c0, hipMemcpyHostToDevice, s), "h2d part");
    if (ev) HIPOK(hipEventRecord(ev[k], s), "record");
    return 0;
  };
  if (bytes < (uint64_t(8) << 20)) {
    int err;
    for (int k = 0; k < K; k++) {
      par_copy({{stage + bounds[k], src + bounds[k], bounds[k + 1] - bounds[k]}});
      if ((err = send(k))) return err;
    }
    return 0;
  }
  const int T = copy_threads();
  std::vector<std::atomic<int>> done(K);
  for (auto& d : done) d.store(0);
  auto part = [&](int t) {
    for (int k = 0; k < K; k++) {
      const uint64_t c0 = bounds[k], c1 = bounds[k + 1];
      const uint64_t a = c0 + (c1 - c0) * t / T, b = c0 + (c1 - c0) * (t + 1) / T;
      memcpy(stage + a, src + a, b - a);
      done[k].fetch_add(1, std::memory_order_release);
    }
  };
  std::vector<std::thread> th;
  for (int t = 1; t < T; t++) th.emplace_back(part, t);
  int err = 0;
  for (int k = 0; k < K; k++) {
    const uint64_t c0 = bounds[k], c1 = bounds[k + 1];
    memcpy(stage + c0, src + c0, (c1 - c0) / T);  // thread 0's share of part k
    while (done[k].load(std::memory_order_acquire) < T - 1) std::this_thread::yield();
    if (!err) err = send(k);
  }
  for (auto& x : th) x.join();
  return err;
}

uint64_t sha512_blocks(const uint64_t* off, uint64_t i) { return (64 + (off[i + 1] - off[i]) + 17 + 127) / 128; }
// One branch-free pass over the offsets of requests [lo, hi): are they
// non-decreasing, and do all messages have request lo's SHA-512 block count?
// (It vectorises: at C2 the two early-exit loops it replaces took ~0.1 ms of a
// synchronous call's host time before the first copy.)
struct OffScan {
  bool ok, uniform;
};
// Built twice (target_clones): an AVX2 clone, picked at load time on hosts
// that have it (the C2 scan in ~20 us), and the x86-64 baseline for the rest;
// the rest of the library's host code is baseline x86-64.
#if defined(__HIP_DEVICE_COMPILE__)
#define EDV_HOST_CLONES
#else
#define EDV_HOST_CLONES __attribute__((target_clones("avx2", "default")))
#endif
EDV_HOST_CLONES OffScan scan_offsets(const uint64_t* off, uint64_t lo,
                                                                        uint64_t hi) {
  const uint64_t nb0 = sha512_blocks(off, lo);
  uint64_t bad = 0, diff = 0;
  for (uint64_t i = lo; i < hi; i++) {
    const uint64_t a = off[i], b = off[i + 1];
    bad |= uint64_t(b < a);
    diff |= ((64 + (b - a) + 17 + 127) >> 7) ^ nb0;  // garbage when b < a: then bad is set
  }
  return {bad == 0, diff == 0};
}

// A shard of one chunk, copied field by field (the default host path for a
// shard that fits one chunk).  Splitting the copy by requests cannot help: a
// sub-batch's kernels take a whole batch's time (latency-bound lanes, DESIGN.md
// section 3).  Splitting it by input field can: the two point sides need only
// the signatures (R) and keys (A), 27 % of the bytes, and the hash side only
// the messages (71 %) besides.  So: H2D of sigs, pks and offsets (one copy
// when they are contiguous), then of the messages in `slices` slices by request,
// on the copy stream; the point sides (and the length buckets) start on stream
// hs[0] as soon as the first part is in, while the messages still copy; the
// hash side of each slice as soon as its messages are in (one slice: in order
// on hs[0]; several: on hs[1..3] in turn), so only the last slice's hash side
// is left after the copy; the main kernel on hs[0] after all of them, writing
// the verdicts straight into page-locked host memory.  Length-bucketed shards
// (messages of several SHA-512 block counts) hash in one piece after the whole
// copy: the bucket permutation spans the shard.  Anatomy of a C2 call:
// DESIGN.md section 3, "The synchronous call".  Caller holds c.mu.
// uniform: 1 / 0 = the offsets were checked and every message has (not) one
// SHA-512 block count; -1 = not checked yet: the check runs here, on the host,
// while the first copy (whose size depends on n only) is already on its way,
// and a failed check returns EDV_E_ARG before anything reads the offsets.
// h: the shard's inputs (pinned: page-locked, so copied from where they are);
// the device buffers c.sigs, pks, msgs, off and acc are the caller's to ensure.
int run_shard_fields(DevCtx& c, HostIn h, const uint64_t* off, uint64_t lo, uint64_t hi, bool pinned, int uniform,
                     uint8_t* accept) {
  const uint64_t n = h.n, mbase = h.mbase, mbytes = h.mbytes;
  const hipStream_t cp = c.hcp, s0 = c.hs[0];
  uint8_t *d_sigs = static_cast<uint8_t*>(c.sigs.p), *d_pks = static_cast<uint8_t*>(c.pks.p),
          *d_msgs = static_cast<uint8_t*>(c.msgs.p);
  uint64_t* d_off = static_cast<uint64_t*>(c.off.p);
  int err;
  if ((err = grow_state(c, n))) return err;
  // the scratch's previous users (any stream) finish before the kernels write it,
  // and the copies follow the previous call's (nothing to wait for when its
  // last user is already done, e.g. the previous synchronous call)
  if (hipEventQuery(c.st_done) != hipSuccess) {
    (void)hipGetLastError();
    HIPOK(hipStreamWaitEvent(cp, c.st_done, 0), "wait scratch");
    for (int q = 0; q < kQ; q++) HIPOK(hipStreamWaitEvent(c.hs[q], c.st_done, 0), "wait scratch");
  }
  const uint8_t* src_m = h.msgs;  // the caller's: staged slice by slice below when pageable
  PinnedBuf& sl = c.stage[0];
  if (!pinned) {
    HIPOK(hipEventSynchronize(c.hs_staged[0]), "stage wait");  // the slot's previous H2D is done
    if ((err = stage_inputs(sl, h, false))) return err;
  }
  // The fixed part in ONE copy, into a device block of the host region's
  // layout, when it lies in one region (input_span); else into the three buffers.
  const OneSpan sp = input_span(h);
  if (sp.one) {
    if (c.fblob.ensure(sp.span)) return EDV_E_OOM;
    d_sigs = static_cast<uint8_t*>(c.fblob.p);
    d_pks = d_sigs + sp.gp;
    d_off = reinterpret_cast<uint64_t*>(d_sigs + sp.go);
  }
  // queued before the offsets scan below: its size depends on n only
  if ((err = upload(h, sp.one, sp.span, d_sigs, d_pks, d_off, nullptr, cp))) return err;
  if (uniform < 0) {
    const OffScan sc = scan_offsets(off, lo, hi);
    if (!sc.ok) {
      HIPOK(hipStreamSynchronize(cp), "stream sync");  // nothing may read the caller's buffers after we return
      return set_err(EDV_E_ARG, "msg_off not non-decreasing");
    }
    uniform = sc.uniform ? 1 : 0;
  }
  const bool bucket = bucketing_enabled(c, uniform ? EDV_FLAG_UNIFORM_LENGTH : EDV_FLAG_BUCKETS);
  // the message slices (field_slices, edv_hostplan.h): one per 65,536 requests,
  // edv_set_host_slices overrides; a bucketed shard is one slice
  uint64_t rb[kSlices + 1], mb[kSlices + 1];  // request / message-byte bounds of the slices (shard-relative)
  const int K = field_slices(n, c.host_slices, bucket, kBlock, rb);
  for (int k = 0; k <= K; k++) mb[k] = off[lo + rb[k]] - mbase;
  HIPOK(hipEventRecord(c.part_copied, cp), "record");
  // The kernels write the verdicts straight into the page-locked host buffer
  // (one 64-byte PCIe write per wave), so no D2H copy and its launch gap follow
  // the main kernel (C2 pinned 1.075 -> 1.046 ms, with the in-stream hash side
  // below 1.033-1.048 ms: profiles/r05/ab_sync_s4.jsonl).
  VerdictSink v;
  if ((err = sink_open(v, accept, n, c.acc_host, c.acc))) return err;
  uint8_t* const d_acc = v.dev;
  // the point sides first: they need only what has just been queued
  VerifyArgs va = make_args(c, c.st, d_sigs, d_pks, d_msgs, d_off, mbase, d_acc, bucket, 0, n);
  if (!va.btab) return no_tables(c);
  va.n = n;
  HIPOK(hipStreamWaitEvent(s0, c.part_copied, 0), "wait copy");
  if (bucket && (err = launch_buckets(bucket_ctr(c.st, 0), va, d_off, s0))) return err;
  HIPOK(hipEventRecord(c.part_prepped, s0), "record");  // the bucket permutation is written
  VerifyArgs vp = va;
  vp.side0 = 1;
  vp.nsides = 2;
  if ((err = launch_prep_sides(vp, s0))) return err;
  // then the messages, slice by slice (staged in the same slices when pageable)
  if (!pinned) {
    uint8_t* pm = static_cast<uint8_t*>(sl.p) + packed_layout(n, mbytes).msgs;
    if (mbytes && (err = stage_and_send(d_msgs, pm, src_m, mb, K, cp, c.slice_copied))) return err;
    if (!mbytes)
      for (int k = 0; k < K; k++) HIPOK(hipEventRecord(c.slice_copied[k], cp), "record");
    HIPOK(hipEventRecord(c.hs_staged[0], cp), "record");
  } else {
    for (int k = 0; k < K; k++) {
      if (mb[k + 1] > mb[k])
        HIPOK(hipMemcpyAsync(d_msgs + mb[k], src_m + mb[k], mb[k + 1] - mb[k], hipMemcpyHostToDevice, cp), "h2d msgs");
      HIPOK(hipEventRecord(c.slice_copied[k], cp), "record");
    }
  }
  for (int k = 0; k < K; k++) {
    // one slice: the hash side in order behind the point sides on s0 (they are
    // done long before the messages land), so main follows it in-stream with no
    // cross-stream event between them
    const hipStream_t hk = K == 1 ? s0 : c.hs[1 + k % (kQ - 1)];
    // requests [rb[k], rb[k+1]) of the shard: scratch slots and request index
    // both start at rb[k] (a bucketed shard is one slice, over the permutation)
    VerifyArgs vh = make_args(c, c.st, d_sigs, d_pks, d_msgs, d_off, mbase, d_acc, bucket, rb[k], n);
    vh.base = rb[k];
    vh.n = rb[k + 1] - rb[k];
    vh.side0 = 0;
    vh.nsides = 1;
    HIPOK(hipStreamWaitEvent(hk, c.slice_copied[k], 0), "wait copy");
    if (bucket) HIPOK(hipStreamWaitEvent(hk, c.part_prepped, 0), "wait buckets");
    if ((err = launch_prep_sides(vh, hk))) return err;
    HIPOK(hipEventRecord(c.slice_hashed[k], hk), "record");
  }
  if (K > 1)
    for (int k = 0; k < K; k++) HIPOK(hipStreamWaitEvent(s0, c.slice_hashed[k], 0), "wait hash side");
  if ((err = launch_main(va, s0)) || (err = sink_d2h(v, s0))) return err;
  HIPOK(hipEventRecord(c.st_done, s0), "record scratch");
  HIPOK(hipStreamWaitEvent(c.stream, c.st_done, 0), "join");
  HIPOK(hipStreamSynchronize(s0), "stream sync");
  sink_deliver(v);
  return 0;
}

// The latency path of a synchronous call (a shard of at most c.quad_max
// requests): inputs DMA'd straight from pinned caller memory, or packed into
// the pinned staging block and read there by the kernel (quad_upload), the
// quad kernel, verdicts written straight into page-locked host memory.
// Caller holds c.mu.
int run_shard_quad(DevCtx& c, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                   uint64_t lo, uint64_t hi, uint8_t* accept) {
  const uint64_t n = hi - lo, mbase = off[lo];
  const hipStream_t s = c.hs[0];
  // the table-free kernel (n <= kRtlMax) touches no device scratch, so it need
  // not be ordered after (nor before) the scratch's other users; the qblob /
  // qstage / acc buffers are this call's alone while it holds c.mu
  const bool scratch = n > kRtlMax;
  if (scratch && hipEventQuery(c.st_done) != hipSuccess) {  // the scratch's previous user (any stream)
    (void)hipGetLastError();
    HIPOK(hipStreamWaitEvent(s, c.st_done, 0), "wait scratch");
  }
  int err;
  DevIn d;
  VerdictSink v;
  if ((err = quad_upload(c.qblob, c.qstage, host_in(sigs, pks, msgs, off, lo, hi), s, &d)) ||
      (err = sink_open(v, accept + lo, n, c.acc_host, c.acc)) ||
      (err = launch_quad(c, c.qtab, d.sigs, d.pks, d.msgs, d.off, mbase, n, v.dev, s)) || (err = sink_d2h(v, s)))
    return err;
  if (scratch) HIPOK(hipEventRecord(c.st_done, s), "record scratch");
  HIPOK(hipStreamSynchronize(s), "stream sync");
  sink_deliver(v);
  return 0;
}

// One shard on one device, host buffers: one sub-batch on the field path, or
// sub-batches of P requests alternating over two streams (sub_split); per
// sub-batch: H2D copies (straight from the caller's memory when it is pinned,
// else through this stream's pinned slot, filled by a parallel memcpy while
// earlier sub-batches run), [length buckets,] prep, main, D2H of its accept bytes.  Caller holds c.mu.
// uniform: 1 = every message of the whole batch has one SHA-512 block count
// (known from the argument check), 0 = not, so the shard is scanned for it;
// -1 = the offsets are not checked yet (a large one-shard call: the field path
// checks them while its first copy runs, the other paths first thing).
// no_latency: this call takes the batch kernels whatever c.quad_max is (edv_self_test).
int run_shard(DevCtx& c, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off, uint64_t lo,
              uint64_t hi, uint8_t* accept, int uniform, bool no_latency = false) {
  const uint64_t n = hi - lo;
  if (n == 0) return 0;
  if (!no_latency && n <= c.quad_max) return run_shard_quad(c, sigs, pks, msgs, off, lo, hi, accept);
  // A shard that fits one chunk is one sub-batch (the field path): split 2 or
  // 4 ways at 64k it measured 1.6x / 1.9x slower (profiles/r02/e2e_probe_s4.json),
  // as a 16k sub-batch still takes a whole batch's latency at one wave per
  // SIMD.  A larger shard alternates two streams of half-chunk sub-batches, so
  // the H2D copy of one overlaps the kernels of the other.
  const auto [Q, pmax, P, nsub] = sub_split(n, c.chunk, kBlock);
  if (uniform < 0 && nsub != 1) {
    const OffScan sc = scan_offsets(off, lo, hi);
    if (!sc.ok) return set_err(EDV_E_ARG, "msg_off not non-decreasing");
    uniform = sc.uniform ? 1 : 0;
  }
  if (uniform == 0) uniform = scan_offsets(off, lo, hi).uniform ? 1 : 0;  // this shard may be uniform
  const uint64_t mbase = off[lo], mbytes = off[hi] - off[lo];
  if (c.sigs.ensure(n * 64) || c.pks.ensure(n * 32) || c.msgs.ensure(mbytes + 64) ||
      c.off.ensure((n + nsub) * 8) || c.acc.ensure(n))
    return EDV_E_OOM;
  const bool pinned = inputs_pinned(host_in(sigs, pks, msgs, off, lo, hi));
  // One chunk: copied field by field, the point sides starting before the
  // messages are in.
  if (nsub == 1)
    return run_shard_fields(c, host_in(sigs, pks, msgs, off, lo, hi), off, lo, hi, pinned, uniform, accept + lo);
  // bucket by SHA block count only when the shard's messages differ in block count
  const uint32_t flags = uniform == 0 ? EDV_FLAG_BUCKETS : EDV_FLAG_UNIFORM_LENGTH;
  uint8_t *d_sigs = static_cast<uint8_t*>(c.sigs.p), *d_pks = static_cast<uint8_t*>(c.pks.p),
          *d_msgs = static_cast<uint8_t*>(c.msgs.p);
  uint64_t* d_off = static_cast<uint64_t*>(c.off.p);
  int err;
  VerdictSink v;  // never zero-copy here: each sub-batch's verdicts are copied back from c.acc as it finishes
  if ((err = sink_host(v, accept + lo, n, c.acc_host))) return err;
  v.dev = static_cast<uint8_t*>(c.acc.p);
  if ((err = grow_state(c, uint64_t(Q) * pmax))) return err;  // sub-batch stream q uses slots [q pmax, (q + 1) pmax)
  for (int q = 0; q < Q; q++) HIPOK(hipStreamWaitEvent(c.hs[q], c.st_done, 0), "wait scratch");
  for (uint64_t k = 0; k < nsub; k++) {
    const int q = int(k % Q);
    hipStream_t s = c.hs[q];
    const uint64_t a = lo + k * P, b = (a + P) < hi ? (a + P) : hi, cnt = b - a;
    // sub-batch k's offsets live at d_off + (a - lo) + k: one private n+1 window each
    uint64_t* d_o = d_off + (a - lo) + k;
    HostIn h = host_in(sigs, pks, msgs, off, a, b);
    if (!pinned) {
      // pageable: staged through this stream's pinned slot (a parallel memcpy),
      // then copied by DMA.  (Staging in four parts with each part's H2D queued
      // as soon as it was staged measured slower at C2, 2.43 vs 1.78 ms per 64k:
      // profiles/r02/e2e_probe_s6.json.)
      HIPOK(hipEventSynchronize(c.hs_staged[q]), "stage wait");  // the slot's previous H2D is done
      if ((err = stage_inputs(c.stage[q], h, true))) return err;
    }
    if ((err = upload(h, false, 0, d_sigs + 64 * (a - lo), d_pks + 32 * (a - lo), d_o, d_msgs + (h.mbase - mbase), s)))
      return err;
    if (!pinned) HIPOK(hipEventRecord(c.hs_staged[q], s), "record");
    const bool bucket = bucketing_enabled(c, flags);
    const VerifyArgs va = make_args(c, c.st, d_sigs + 64 * (a - lo), d_pks + 32 * (a - lo), d_msgs, d_o, mbase,
                                    v.dev + (a - lo), bucket, uint64_t(q) * pmax, n);
    if (!va.btab) return no_tables(c);
    if ((err = walk_chunks(bucket_ctr(c.st, q), va, bucket, cnt, cnt, s))) return err;
    HIPOK(hipMemcpyAsync(v.host + (a - lo), v.dev + (a - lo), cnt, hipMemcpyDeviceToHost, s), "d2h accept");
  }
  // join the sub-batch streams into the library stream: the scratch's next user waits for all of them
  for (int q = 0; q < Q; q++) {
    HIPOK(hipEventRecord(c.hs_end[q], c.hs[q]), "record");
    HIPOK(hipStreamWaitEvent(c.stream, c.hs_end[q], 0), "wait");
  }
  HIPOK(hipEventRecord(c.st_done, c.stream), "record scratch");
  HIPOK(hipStreamSynchronize(c.stream), "stream sync");
  sink_deliver(v);
  return 0;
}

int launch_sha256(const uint8_t* d_msgs, const uint64_t* d_off, uint64_t msg_base, uint64_t n, uint8_t* d_out,
                  hipStream_t s) {
  if (n == 0) return 0;
  const unsigned blocks = unsigned((n + kBlock - 1) / kBlock);
  HIPOK(launch_sha256_kernel(blocks, s, d_msgs, d_off, msg_base, n, reinterpret_cast<uint32_t*>(d_out)),
        "sha256 launch");
  return 0;
}

// SHA-256 digests of messages [lo, hi) on one device, host buffers; caller holds c.mu
int run_digest_shard(DevCtx& c, const uint8_t* msgs, const uint64_t* off, uint64_t lo, uint64_t hi, uint8_t* out) {
  const uint64_t n = hi - lo;
  if (n == 0) return 0;
  const uint64_t mbase = off[lo], mbytes = off[hi] - off[lo];
  if (c.msgs.ensure(mbytes + 64) || c.off.ensure((n + 1) * 8) || c.sigs.ensure(n * 32)) return EDV_E_OOM;
  // the host verify path shares these buffers; it finishes (synchronously) under the same lock
  if (mbytes) HIPOK(hipMemcpyAsync(c.msgs.p, msgs + mbase, mbytes, hipMemcpyHostToDevice, c.stream), "h2d msgs");
  HIPOK(hipMemcpyAsync(c.off.p, off + lo, (n + 1) * 8, hipMemcpyHostToDevice, c.stream), "h2d off");
  int err;
  if ((err = launch_sha256(static_cast<uint8_t*>(c.msgs.p), static_cast<uint64_t*>(c.off.p), mbase, n,
                           static_cast<uint8_t*>(c.sigs.p), c.stream)))
    return err;
  HIPOK(hipMemcpyAsync(out + 32 * lo, c.sigs.p, n * 32, hipMemcpyDeviceToHost, c.stream), "d2h digests");
  HIPOK(hipStreamSynchronize(c.stream), "stream sync");
  return 0;
}

// ---- Merkle-tree extension (edv_merkle.h).  Extends (old_size, d_old) by the
// n leaves at d_leaves / d_off on stream s: the passes (merkle_for_each_pass),
// then the finish.  d_leafh / d_nodeh may be null.  The tile roots go through
// mk_roots; launches on different streams are ordered on it by c.mk.done.
// d_aroots / d_paths (either may be null): the per-leaf roots and packed audit
// paths of the batched append, by one more kernel after the finish.  Where it
// reads leaf or node hashes that d_leafh / d_nodeh do not take, they go to
// mk_fleafh / mk_fnodeh, scratch under the same event.  d_leaf_in (row f-9):
// the n leaf hashes instead of d_leaves / d_off; pass 0 reads them.  Caller
// holds c.mu.
int launch_merkle(DevCtx& c, uint64_t old_size, const uint8_t* d_old, const uint8_t* d_leaves, const uint64_t* d_off,
                  uint64_t leaf_base, uint64_t n, uint8_t* d_leafh, uint8_t* d_nodeh, uint8_t* d_new, uint8_t* d_root,
                  hipStream_t s, uint8_t* d_aroots = nullptr, uint8_t* d_paths = nullptr,
                  const uint8_t* d_leaf_in = nullptr) {
  MerkleBufs& m = c.mk;
  const uint64_t new_size = old_size + n;
  if (!m.done) HIPOK(hipEventCreateWithFlags(&m.done, hipEventDisableTiming), "event");
  const MerkleSizes need = merkle_extend_needs(old_size, n, 0, false, d_leafh, d_nodeh, d_aroots, d_paths);
  if (const int err = m.ensure(need)) return err;
  const bool scratch = need[mk_roots] || need[mk_fleafh] || need[mk_fnodeh];
  if (scratch) HIPOK(hipStreamWaitEvent(s, m.done, 0), "wait merkle scratch");
  if (need[mk_fleafh]) d_leafh = m.at(mk_fleafh);
  if (need[mk_fnodeh]) d_nodeh = m.at(mk_fnodeh);
  MerklePass a = merkle_pass_args(old_size, new_size, d_old, d_leafh, d_nodeh, d_new);
  HIPOK(merkle_for_each_pass(old_size, new_size, m.at<uint32_t>(mk_roots), a,
                             [&](const MerklePass& p) { return launch_merkle_pass_kernel(s, p, d_leaves, d_off, leaf_base); },
                             reinterpret_cast<const uint32_t*>(d_leaf_in)),
        "merkle pass launch");
  HIPOK(launch_merkle_finish_kernel(s, old_size, new_size, a.old_hashes, a.new_hashes,
                                    reinterpret_cast<uint32_t*>(d_root)),
        "merkle finish launch");
  if (n && (d_aroots || d_paths))
    HIPOK(launch_merkle_append_kernel(s, merkle_append_args(old_size, n, d_old, d_leafh, d_nodeh, d_aroots, d_paths)),
          "merkle append launch");
  if (scratch) HIPOK(hipEventRecord(m.done, s), "record merkle scratch");
  return 0;
}

// The host form: staged like run_digest_shard, in buffers of its own
// (merkle_extend_needs); copies back only the outputs asked for (roots /
// audit_paths: the batched append's, null from edv_merkle_extend).  Caller
// holds c.mu.
int run_merkle_host(DevCtx& c, uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves, const uint64_t* off,
                    uint64_t n, uint8_t* leaf_hashes, uint8_t* node_hashes, uint8_t* new_hashes, uint8_t* root,
                    uint8_t* roots = nullptr, uint8_t* audit_paths = nullptr) {
  MerkleBufs& m = c.mk;
  const uint64_t new_size = old_size + n, nodes = merkle_node_count(new_size) - merkle_node_count(old_size);
  const uint64_t nold = uint64_t(popc64(old_size)), nnew = uint64_t(popc64(new_size));
  const uint64_t mbase = n ? off[0] : 0, mbytes = n ? off[n] - off[0] : 0;
  const MerkleSizes need = merkle_extend_needs(old_size, n, mbytes, true, leaf_hashes, node_hashes, roots, audit_paths);
  if (const int err = m.ensure(need)) return err;
  const hipStream_t s = c.stream;
  uint8_t *d_old = m.at(mk_hashes), *d_new = d_old + 32 * kMerkleMaxHashes, *d_root = d_new + 32 * kMerkleMaxHashes;
  if (mbytes) HIPOK(hipMemcpyAsync(m.at(mk_leaves), leaves + mbase, mbytes, hipMemcpyHostToDevice, s), "h2d leaves");
  if (n) HIPOK(hipMemcpyAsync(m.at(mk_off), off, (n + 1) * 8, hipMemcpyHostToDevice, s), "h2d leaf_off");
  if (nold) HIPOK(hipMemcpyAsync(d_old, old_hashes, 32 * nold, hipMemcpyHostToDevice, s), "h2d old hashes");
  // null where nothing is to be written: no leaves, no nodes, not asked for and not read by the fold
  uint8_t *d_leafh = m.at(mk_leafh, need), *d_nodeh = m.at(mk_nodeh, need), *d_aroots = m.at(mk_aroots, need),
          *d_paths = m.at(mk_paths, need);
  if (const int err = launch_merkle(c, old_size, d_old, m.at(mk_leaves), m.at<uint64_t>(mk_off), mbase, n, d_leafh,
                                    d_nodeh, d_new, d_root, s, d_aroots, d_paths))
    return err;
  if (d_aroots) HIPOK(hipMemcpyAsync(roots, d_aroots, 32 * n, hipMemcpyDeviceToHost, s), "d2h roots");
  if (d_paths) HIPOK(hipMemcpyAsync(audit_paths, d_paths, need[mk_paths], hipMemcpyDeviceToHost, s), "d2h audit paths");
  if (leaf_hashes && d_leafh) HIPOK(hipMemcpyAsync(leaf_hashes, d_leafh, 32 * n, hipMemcpyDeviceToHost, s), "d2h leaf hashes");
  if (node_hashes && d_nodeh) HIPOK(hipMemcpyAsync(node_hashes, d_nodeh, 32 * nodes, hipMemcpyDeviceToHost, s), "d2h node hashes");
  if (nnew) HIPOK(hipMemcpyAsync(new_hashes, d_new, 32 * nnew, hipMemcpyDeviceToHost, s), "d2h new hashes");
  HIPOK(hipMemcpyAsync(root, d_root, 32, hipMemcpyDeviceToHost, s), "d2h root");
  HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// ---- proof verification (edv_merkle.h, row f-7).  The host forms: inputs
// staged in the mv_* buffers (merkle_verify_needs), the device forms' launch
// on the library stream, the statuses (and the computed roots, if asked for)
// copied back, synchronous.  The windows [off[0], off[n]) of the leaf bytes and
// of the proof entries are what is copied, and off[0] is the kernel's base.
// Caller holds c.mu and has checked the arguments.
struct WordStage {
  uint64_t* next;  // mv_words, from its start
  hipStream_t s;
  hipError_t e = hipSuccess;  // the first copy's that failed
  const uint64_t* put(const uint64_t* src, uint64_t count) {
    if (e == hipSuccess) e = hipMemcpyAsync(next, src, 8 * count, hipMemcpyHostToDevice, s);
    next += count;
    return next - count;
  }
};
int stage_proofs(DevCtx& c, const uint8_t* proofs, const uint64_t* proof_off, uint64_t n) {
  if (const uint64_t bytes = 32 * (proof_off[n] - proof_off[0]))
    HIPOK(hipMemcpyAsync(c.mk.at(mv_proofs), proofs + 32 * proof_off[0], bytes, hipMemcpyHostToDevice, c.stream),
          "h2d proofs");
  return 0;
}
// launch(d_status, d_computed) runs the kernel; cbytes: computed bytes per proof
template <class Launch>
int run_proofs_out(DevCtx& c, uint64_t n, uint64_t cbytes, uint8_t* status, uint8_t* computed, Launch launch) {
  uint8_t* d_comp = computed ? c.mk.at(mv_out) : nullptr;
  uint8_t* d_status = c.mk.at(mv_out) + (computed ? cbytes * n : 0);
  HIPOK(launch(d_status, d_comp), "merkle verify launch");
  HIPOK(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, c.stream), "d2h proof status");
  if (computed) HIPOK(hipMemcpyAsync(computed, d_comp, cbytes * n, hipMemcpyDeviceToHost, c.stream), "d2h computed roots");
  HIPOK(hipStreamSynchronize(c.stream), "stream sync");
  return 0;
}

int run_verify_inclusion_host(DevCtx& c, const uint8_t* leaves, const uint64_t* leaf_off, const uint8_t* leaf_hashes,
                              const uint64_t* leaf_index, const uint64_t* tree_size, const uint8_t* roots,
                              const uint8_t* proofs, const uint64_t* proof_off, uint64_t n, uint8_t* status,
                              uint8_t* computed) {
  MerkleBufs& m = c.mk;
  const hipStream_t s = c.stream;
  const uint64_t lbytes = leaves ? leaf_off[n] - leaf_off[0] : 32 * n;
  if (const int err = m.ensure(merkle_verify_needs(true, n, lbytes, proof_off[n] - proof_off[0], computed))) return err;
  if (const int err = stage_proofs(c, proofs, proof_off, n)) return err;
  if (lbytes)
    HIPOK(hipMemcpyAsync(m.at(mv_leaves), leaves ? leaves + leaf_off[0] : leaf_hashes, lbytes, hipMemcpyHostToDevice, s),
          "h2d leaves");
  HIPOK(hipMemcpyAsync(m.at(mv_roots), roots, 32 * n, hipMemcpyHostToDevice, s), "h2d roots");
  WordStage w{m.at<uint64_t>(mv_words), s};
  const uint64_t* d_leaf_off = leaves ? w.put(leaf_off, n + 1) : nullptr;
  const uint64_t *d_index = w.put(leaf_index, n), *d_size = w.put(tree_size, n), *d_poff = w.put(proof_off, n + 1);
  HIPOK(w.e, "h2d proof words");
  return run_proofs_out(c, n, 32, status, computed, [&](uint8_t* d_status, uint8_t* d_comp) {
    return launch_merkle_verify_inclusion_kernel(
        s, merkle_verify_inclusion_args(n, leaves ? m.at(mv_leaves) : nullptr, d_leaf_off, leaves ? leaf_off[0] : 0,
                                        leaves ? nullptr : m.at(mv_leaves), d_index, d_size, m.at(mv_roots),
                                        m.at(mv_proofs), d_poff, proof_off[0], d_status, d_comp));
  });
}

int run_verify_consistency_host(DevCtx& c, const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_roots,
                                const uint8_t* new_roots, const uint8_t* proofs, const uint64_t* proof_off, uint64_t n,
                                uint8_t* status, uint8_t* computed) {
  MerkleBufs& m = c.mk;
  const hipStream_t s = c.stream;
  if (const int err = m.ensure(merkle_verify_needs(false, n, 0, proof_off[n] - proof_off[0], computed))) return err;
  if (const int err = stage_proofs(c, proofs, proof_off, n)) return err;
  uint8_t* d_roots = m.at(mv_roots);
  HIPOK(hipMemcpyAsync(d_roots, old_roots, 32 * n, hipMemcpyHostToDevice, s), "h2d old roots");
  HIPOK(hipMemcpyAsync(d_roots + 32 * n, new_roots, 32 * n, hipMemcpyHostToDevice, s), "h2d new roots");
  WordStage w{m.at<uint64_t>(mv_words), s};
  const uint64_t *d_old = w.put(old_size, n), *d_new = w.put(new_size, n), *d_poff = w.put(proof_off, n + 1);
  HIPOK(w.e, "h2d proof words");
  return run_proofs_out(c, n, 64, status, computed, [&](uint8_t* d_status, uint8_t* d_comp) {
    return launch_merkle_verify_consistency_kernel(
        s, merkle_verify_consistency_args(n, d_old, d_new, d_roots, d_roots + 32 * n, m.at(mv_proofs), d_poff,
                                          proof_off[0], d_status, d_comp));
  });
}

// ---- proof generation (edv_merkle.h, row f-8).  The host forms: the store
// prefix the largest valid tree size reads, the three 64-bit arrays and the
// slots' window [off[0], off[n]) staged in the mp_* buffers
// (merkle_prove_needs; the slots go up too, so what no lane writes comes back
// as the caller had it), the device forms' launch on the library stream, the
// slots, the statuses and the outputs asked for copied back, synchronous.
// Caller holds c.mu and has checked the arguments.  a / b: leaf_index /
// tree_size or first / second; out1 / out2: roots / leaf hashes or old / new roots.
template <bool kConsistency>
int run_prove_host(DevCtx& c, const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves,
                   const uint64_t* a, const uint64_t* b, const uint64_t* proof_off, uint64_t n, uint8_t* proofs,
                   uint8_t* status, uint8_t* out1, uint8_t* out2) {
  MerkleBufs& m = c.mk;
  const hipStream_t s = c.stream;
  const uint64_t prefix = merkle_prove_prefix(kConsistency, a, b, n, store_leaves);
  const uint64_t nodes = prefix ? merkle_node_count(prefix) : 0, pbytes = 32 * (proof_off[n] - proof_off[0]);
  if (const int err = m.ensure(merkle_prove_needs(n, prefix, pbytes / 32, out1, out2))) return err;
  if (prefix) HIPOK(hipMemcpyAsync(m.at(mp_leaves), leaf_store, 32 * prefix, hipMemcpyHostToDevice, s), "h2d leaf store");
  if (nodes) HIPOK(hipMemcpyAsync(m.at(mp_nodes), node_store, 32 * nodes, hipMemcpyHostToDevice, s), "h2d node store");
  if (pbytes) HIPOK(hipMemcpyAsync(m.at(mp_proofs), proofs + 32 * proof_off[0], pbytes, hipMemcpyHostToDevice, s), "h2d slots");
  WordStage w{m.at<uint64_t>(mp_words), s};
  const uint64_t *d_a = w.put(a, n), *d_b = w.put(b, n), *d_poff = w.put(proof_off, n + 1);
  HIPOK(w.e, "h2d proof words");
  const MerkleProveOut o = merkle_prove_out(n, out1, out2);
  uint8_t *d_out = m.at(mp_out), *d_1 = out1 ? d_out + o.first : nullptr, *d_2 = out2 ? d_out + o.second : nullptr,
          *d_status = d_out + o.status;
  // the staged prefix is the store the lanes see: a valid pair reads nothing past it
  if (kConsistency)
    HIPOK(launch_merkle_prove_consistency_kernel(
              s, merkle_prove_consistency_args(m.at(mp_leaves), m.at(mp_nodes), prefix, d_a, d_b, d_poff, proof_off[0], n,
                                               m.at(mp_proofs), d_status, d_1, d_2)),
          "merkle prove launch");
  else
    HIPOK(launch_merkle_prove_inclusion_kernel(
              s, merkle_prove_inclusion_args(m.at(mp_leaves), m.at(mp_nodes), prefix, d_a, d_b, d_poff, proof_off[0], n,
                                             m.at(mp_proofs), d_status, d_1, d_2)),
          "merkle prove launch");
  if (pbytes) HIPOK(hipMemcpyAsync(proofs + 32 * proof_off[0], m.at(mp_proofs), pbytes, hipMemcpyDeviceToHost, s), "d2h proofs");
  HIPOK(hipMemcpyAsync(status, d_status, n, hipMemcpyDeviceToHost, s), "d2h proof status");
  if (out1) HIPOK(hipMemcpyAsync(out1, d_1, 32 * n, hipMemcpyDeviceToHost, s), "d2h roots");
  if (out2) HIPOK(hipMemcpyAsync(out2, d_2, 32 * n, hipMemcpyDeviceToHost, s), "d2h roots");
  HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// ---- auditing a stored tree (edv_merkle.h, row f-9).  The host forms: the
// store prefix the slice reads (nodes) or the slice of stored hashes with the
// leaf bytes and offsets (leaves) staged where the prove and verify forms stage
// (merkle_audit_*_needs), the summary set to empty on the device, the device
// forms' launch on the library stream, the summary and the statuses (if asked
// for) copied back, synchronous.  Caller holds c.mu and has checked the
// arguments; count / n > 0.
int finish_audit_host(DevCtx& c, uint64_t n, uint8_t* status, uint64_t summary[2]) {
  uint8_t* d_out = c.mk.at(mp_out);
  HIPOK(hipMemcpyAsync(summary, d_out, kAuditSummaryBytes, hipMemcpyDeviceToHost, c.stream), "d2h audit summary");
  if (status) HIPOK(hipMemcpyAsync(status, d_out + kAuditSummaryBytes, n, hipMemcpyDeviceToHost, c.stream), "d2h audit status");
  HIPOK(hipStreamSynchronize(c.stream), "stream sync");
  return 0;
}
int run_audit_nodes_host(DevCtx& c, const uint8_t* leaf_store, const uint8_t* node_store, uint64_t node_lo,
                         uint64_t count, uint8_t* status, uint64_t summary[2]) {
  MerkleBufs& m = c.mk;
  const hipStream_t s = c.stream;
  if (const int err = m.ensure(merkle_audit_nodes_needs(node_lo, count))) return err;
  const MerkleAuditPrefix p = merkle_audit_nodes_prefix(node_lo, count);
  uint64_t empty[2];
  merkle_audit_summary_init(empty);
  uint8_t* d_out = m.at(mp_out);
  HIPOK(hipMemcpyAsync(m.at(mp_leaves), leaf_store, 32 * p.leaves, hipMemcpyHostToDevice, s), "h2d leaf store");
  HIPOK(hipMemcpyAsync(m.at(mp_nodes), node_store, 32 * p.nodes, hipMemcpyHostToDevice, s), "h2d node store");
  HIPOK(hipMemcpyAsync(d_out, empty, kAuditSummaryBytes, hipMemcpyHostToDevice, s), "h2d audit summary");
  HIPOK(launch_merkle_audit_nodes_kernel(s, merkle_audit_nodes_args(m.at(mp_leaves), m.at(mp_nodes), node_lo, count,
                                                                    status ? d_out + kAuditSummaryBytes : nullptr),
                                         reinterpret_cast<uint64_t*>(d_out)),
        "merkle audit launch");
  return finish_audit_host(c, count, status, summary);
}
int run_audit_leaves_host(DevCtx& c, const uint8_t* leaf_store, uint64_t leaf_lo, const uint8_t* leaves,
                          const uint64_t* leaf_off, uint64_t n, uint8_t* status, uint64_t summary[2]) {
  MerkleBufs& m = c.mk;
  const hipStream_t s = c.stream;
  const uint64_t lbytes = leaf_off[n] - leaf_off[0];
  if (const int err = m.ensure(merkle_audit_leaves_needs(n, lbytes))) return err;
  uint64_t empty[2];
  merkle_audit_summary_init(empty);
  uint8_t* d_out = m.at(mp_out);
  HIPOK(hipMemcpyAsync(m.at(mp_leaves), leaf_store + 32 * leaf_lo, 32 * n, hipMemcpyHostToDevice, s), "h2d leaf store");
  if (lbytes) HIPOK(hipMemcpyAsync(m.at(mv_leaves), leaves + leaf_off[0], lbytes, hipMemcpyHostToDevice, s), "h2d leaves");
  HIPOK(hipMemcpyAsync(m.at(mp_words), leaf_off, 8 * (n + 1), hipMemcpyHostToDevice, s), "h2d leaf_off");
  HIPOK(hipMemcpyAsync(d_out, empty, kAuditSummaryBytes, hipMemcpyHostToDevice, s), "h2d audit summary");
  // the staged slice starts at entry leaf_lo of the store, the staged bytes at leaf_off[0]
  HIPOK(launch_merkle_audit_leaves_kernel(
            s, merkle_audit_leaves_args(m.at(mp_leaves), leaf_lo, leaf_lo, n, m.at(mv_leaves), m.at<uint64_t>(mp_words),
                                        leaf_off[0], status ? d_out + kAuditSummaryBytes : nullptr),
            reinterpret_cast<uint64_t*>(d_out)),
        "merkle audit launch");
  return finish_audit_host(c, n, status, summary);
}
// The host form of the extend from hashes: run_merkle_host without leaf bytes;
// the n hashes go up into mk_leafh and pass 0 reads them there.
int run_merkle_hashed_host(DevCtx& c, uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaf_hashes,
                           uint64_t n, uint8_t* node_hashes, uint8_t* new_hashes, uint8_t* root) {
  MerkleBufs& m = c.mk;
  const uint64_t new_size = old_size + n, nodes = merkle_node_count(new_size) - merkle_node_count(old_size);
  const uint64_t nold = uint64_t(popc64(old_size)), nnew = uint64_t(popc64(new_size));
  const MerkleSizes need = merkle_extend_hashed_needs(old_size, n, true, node_hashes);
  if (const int err = m.ensure(need)) return err;
  const hipStream_t s = c.stream;
  uint8_t *d_old = m.at(mk_hashes), *d_new = d_old + 32 * kMerkleMaxHashes, *d_root = d_new + 32 * kMerkleMaxHashes;
  if (n) HIPOK(hipMemcpyAsync(m.at(mk_leafh), leaf_hashes, 32 * n, hipMemcpyHostToDevice, s), "h2d leaf hashes");
  if (nold) HIPOK(hipMemcpyAsync(d_old, old_hashes, 32 * nold, hipMemcpyHostToDevice, s), "h2d old hashes");
  uint8_t* d_nodeh = m.at(mk_nodeh, need);
  if (const int err = launch_merkle(c, old_size, d_old, nullptr, nullptr, 0, n, nullptr, d_nodeh, d_new, d_root, s,
                                    nullptr, nullptr, n ? m.at(mk_leafh) : nullptr))
    return err;
  if (node_hashes && d_nodeh) HIPOK(hipMemcpyAsync(node_hashes, d_nodeh, 32 * nodes, hipMemcpyDeviceToHost, s), "d2h node hashes");
  if (nnew) HIPOK(hipMemcpyAsync(new_hashes, d_new, 32 * nnew, hipMemcpyDeviceToHost, s), "d2h new hashes");
  HIPOK(hipMemcpyAsync(root, d_root, 32, hipMemcpyDeviceToHost, s), "d2h root");
  HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// ---- catch-up (edv_merkle.h, row f-10).  launch_merkle's passes over the n
// leaves, then one lane per reply on the same stream, ordered on the scratch by
// the same event.  `a` comes from merkle_catchup_args with the caller's leaf
// and node hash buffers (null: the fold scratch takes them, merkle_catchup_needs'
// device form); the new tree's entries, which the passes write and nothing
// reads, go to the front of mk_fnodeh.  Caller holds c.mu.
int launch_merkle_catchup(DevCtx& c, MerkleCatchup a, const uint8_t* d_leaves, const uint64_t* d_off, uint64_t leaf_base,
                          hipStream_t s) {
  MerkleBufs& m = c.mk;
  const uint64_t old_size = a.t.old_size, n = a.t.n, new_size = old_size + n;
  if (!m.done) HIPOK(hipEventCreateWithFlags(&m.done, hipEventDisableTiming), "event");
  const MerkleSizes need = merkle_catchup_needs(old_size, n, 0, a.replies, 0, false, a.t.leaf_hashes, a.t.node_hashes, false);
  if (const int err = m.ensure(need)) return err;
  HIPOK(hipStreamWaitEvent(s, m.done, 0), "wait merkle scratch");
  if (need[mk_fleafh]) a.t.leaf_hashes = m.at<uint32_t>(mk_fleafh);
  if (need[mk_fnodeh] > kCatchupNewBytes) a.t.node_hashes = m.at<uint32_t>(mk_fnodeh) + kCatchupNewBytes / 4;
  MerklePass p = merkle_pass_args(old_size, new_size, a.t.old_hashes, const_cast<uint32_t*>(a.t.leaf_hashes),
                                  const_cast<uint32_t*>(a.t.node_hashes), m.at(mk_fnodeh));
  HIPOK(merkle_for_each_pass(old_size, new_size, m.at<uint32_t>(mk_roots), p,
                             [&](const MerklePass& q) { return launch_merkle_pass_kernel(s, q, d_leaves, d_off, leaf_base); }),
        "merkle pass launch");
  HIPOK(launch_merkle_catchup_kernel(s, a), "merkle catchup launch");
  HIPOK(hipEventRecord(m.done, s), "record merkle scratch");
  return 0;
}

// The host form: the leaves staged as run_merkle_host stages them, the reply
// ends, proof offsets, target root and proof entries as the verify forms stage
// theirs (merkle_catchup_needs); copies back the statuses and the outputs asked
// for.  Caller holds c.mu and has checked the arguments; replies > 0.
int run_merkle_catchup_host(DevCtx& c, uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves,
                            const uint64_t* off, uint64_t n, const uint64_t* reply_end, uint64_t replies,
                            uint64_t final_size, const uint8_t* final_root, const uint8_t* proofs,
                            const uint64_t* proof_off, uint8_t* leaf_hashes, uint8_t* node_hashes, uint8_t* reply_roots,
                            uint8_t* status) {
  MerkleBufs& m = c.mk;
  const uint64_t nodes = merkle_node_count(old_size + n) - merkle_node_count(old_size);
  const uint64_t nold = uint64_t(popc64(old_size));
  const uint64_t mbase = n ? off[0] : 0, mbytes = n ? off[n] - off[0] : 0;
  const MerkleSizes need = merkle_catchup_needs(old_size, n, mbytes, replies, proof_off[replies] - proof_off[0], true,
                                                leaf_hashes, node_hashes, reply_roots);
  if (const int err = m.ensure(need)) return err;
  const hipStream_t s = c.stream;
  if (mbytes) HIPOK(hipMemcpyAsync(m.at(mk_leaves), leaves + mbase, mbytes, hipMemcpyHostToDevice, s), "h2d leaves");
  if (n) HIPOK(hipMemcpyAsync(m.at(mk_off), off, (n + 1) * 8, hipMemcpyHostToDevice, s), "h2d leaf_off");
  if (nold) HIPOK(hipMemcpyAsync(m.at(mk_hashes), old_hashes, 32 * nold, hipMemcpyHostToDevice, s), "h2d old hashes");
  HIPOK(hipMemcpyAsync(m.at(mv_roots), final_root, 32, hipMemcpyHostToDevice, s), "h2d final root");
  if (const int err = stage_proofs(c, proofs, proof_off, replies)) return err;
  WordStage w{m.at<uint64_t>(mv_words), s};
  const uint64_t *d_end = w.put(reply_end, replies), *d_poff = w.put(proof_off, replies + 1);
  HIPOK(w.e, "h2d reply words");
  uint8_t *d_leafh = m.at(mk_leafh, need), *d_nodeh = m.at(mk_nodeh, need);
  uint8_t* d_rroots = reply_roots ? m.at(mv_out) : nullptr;
  uint8_t* d_status = m.at(mv_out) + (reply_roots ? 32 * replies : 0);
  if (const int err = launch_merkle_catchup(
          c, merkle_catchup_args(old_size, n, m.at(mk_hashes), d_leafh, d_nodeh, d_end, replies, final_size,
                                 m.at(mv_roots), m.at(mv_proofs), d_poff, proof_off[0], d_rroots, d_status),
          m.at(mk_leaves), m.at<uint64_t>(mk_off), mbase, s))
    return err;
  HIPOK(hipMemcpyAsync(status, d_status, replies, hipMemcpyDeviceToHost, s), "d2h reply status");
  if (reply_roots) HIPOK(hipMemcpyAsync(reply_roots, d_rroots, 32 * replies, hipMemcpyDeviceToHost, s), "d2h reply roots");
  if (leaf_hashes && n) HIPOK(hipMemcpyAsync(leaf_hashes, d_leafh, 32 * n, hipMemcpyDeviceToHost, s), "d2h leaf hashes");
  if (node_hashes && nodes) HIPOK(hipMemcpyAsync(node_hashes, d_nodeh, 32 * nodes, hipMemcpyDeviceToHost, s), "d2h node hashes");
  HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// Asynchronous host path.  Wait for a slot's batch and hand over its verdicts.
void async_fail(DevCtx& c, DevCtx::AsyncSlot& s) {
  c.ledger.fail(s.ticket);
  s.ticket = -1;
}
int async_complete(DevCtx& c, DevCtx::AsyncSlot& s) {
  if (s.ticket < 0) return 0;
  if (const hipError_t e = hipEventSynchronize(s.done); e != hipSuccess) {
    async_fail(c, s);
    return set_err(EDV_E_HIP, "async wait", e);
  }
#ifdef EDV_MEASUREMENT_API
  if (s.injected) {
    s.injected = false;
    async_fail(c, s);
    return set_err(EDV_E_HIP, "async batch failed (injected by edv_test_fail_async)");
  }
#endif
  sink_deliver(s.verdicts);
  if (s.digests && !s.dig_pinned) memcpy(s.digests, s.dig_host.p, 32 * s.n);
  s.ticket = -1;
  return 0;
}

// What both submission routes end with, on stream ks, for batch t on slot s
// with its inputs d on the device: the verify kernels (launch(d_acc): the
// route's), the D2H of the verdicts, the digests if asked for, the slot's done
// event, its bookkeeping and the ticket.
template <class Launch>
int async_run(DevCtx& c, DevCtx::AsyncSlot& s, int64_t t, const DevIn& d, uint64_t mbase, uint64_t n, uint8_t* accept,
              uint8_t* digests, hipStream_t ks, int64_t* ticket, Launch launch) {
  int err;
  // verdicts written by the kernels straight into page-locked host memory, as
  // in the synchronous path: no D2H between this batch's main kernel and the
  // next batch's prep on the stream (a C2 stream of batches 0.945 -> 0.965x
  // device-resident, profiles/r05/ab_async_s7.jsonl)
  if ((err = sink_open(s.verdicts, accept, n, s.acc_host, s.acc))) return err;
  bool skip = false;  // edv_test_fail_async (measurement build): no kernels, and the wait fails
#ifdef EDV_MEASUREMENT_API
  skip = s.injected = (t == c.inject_fail);
#endif
  if ((!skip && (err = launch(s.verdicts.dev))) || (err = sink_d2h(s.verdicts, ks))) return err;
  if (digests && !skip) {
    // Request.getDigest of requests whose signing bytes ARE the message (the
    // caller decides which): SHA-256 of the message bytes already on the device
    uint8_t* d_dig = static_cast<uint8_t*>(s.dig.p);
    if ((err = launch_sha256(d.msgs, d.off, mbase, n, d_dig, ks))) return err;
    uint8_t* h_dig = s.dig_pinned ? digests : static_cast<uint8_t*>(s.dig_host.p);
    HIPOK(hipMemcpyAsync(h_dig, d_dig, 32 * n, hipMemcpyDeviceToHost, ks), "d2h digests");
  }
  HIPOK(hipEventRecord(s.done, ks), "record");
  s.ticket = t;
  s.digests = digests;
  s.n = n;
  *ticket = c.ledger.issue();
  return 0;
}

// Queue one host batch: H2D copies on hcp (from the caller's memory when it is
// pinned, else through the slot's pinned staging, filled here while the
// previous batch computes), then on hac the kernels and the D2H of the
// verdicts; a batch of at most kSmallAsync requests does all of that on its
// slot's own stream and scratch instead.  A slot is reused kAsyncSlots
// submissions later, after its batch is complete.  Caller holds c.mu.
int submit_async(DevCtx& c, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* off,
                 uint64_t n, uint8_t* accept, uint8_t* digests, bool uniform, int64_t* ticket) {
  const int64_t t = c.ledger.next;
  DevCtx::AsyncSlot& s = c.as[t % kAsyncSlots];
  int err;
  if ((err = async_complete(c, s))) return err;  // the batch of kAsyncSlots submissions ago
  // an unfilled verdict buffer rejects: whatever happens to this batch, no stale
  // byte of a reused buffer can read as "accept"
  memset(accept, 0, n);
  const uint64_t mbase = off[0], mbytes = off[n] - mbase;
  if (s.sigs.ensure(n * 64) || s.pks.ensure(n * 32) || s.msgs.ensure(mbytes + 64) || s.off.ensure((n + 1) * 8) ||
      s.acc.ensure(n) || (digests && s.dig.ensure(32 * n)))
    return EDV_E_OOM;
  s.dig_pinned = digests && is_pinned(digests);
  if (digests && !s.dig_pinned && s.dig_host.ensure(32 * n)) return EDV_E_OOM;
  HostIn h = host_in(sigs, pks, msgs, off, 0, n);
  // small batch: everything on the slot's stream and scratch (see kSmallAsync)
  const bool own = n <= kSmallAsync, quad = n <= c.quad_max;
  if ((own || quad) && !s.st) HIPOK(hipStreamCreateWithFlags(&s.st, hipStreamNonBlocking), "hipStreamCreate");
  // the latency path: inputs packed into the slot's pinned staging and read
  // there, or DMA'd (quad_upload), the quad kernel on the slot's own stream
  if (quad) {
    DevIn d;
    if ((err = quad_upload(s.msgs, s.stage, h, s.st, &d))) return err;
    return async_run(c, s, t, d, mbase, n, accept, digests, s.st, ticket, [&](uint8_t* d_acc) {
      return launch_quad(c, s.qtab, d.sigs, d.pks, d.msgs, d.off, mbase, n, d_acc, s.st);
    });
  }
  if (own && s.cb.ensure(n, kSmallAsync)) return EDV_E_OOM;  // the slot's previous batch is complete
  const hipStream_t cs = own ? s.st : c.hcp, ks = own ? s.st : c.hac;
  const uint32_t lflags = uniform ? EDV_FLAG_UNIFORM_LENGTH : EDV_FLAG_BUCKETS;
  if (!inputs_pinned(h) && (err = stage_inputs(s.stage, h, true))) return err;
  const DevIn d = {static_cast<uint8_t*>(s.sigs.p), static_cast<uint8_t*>(s.pks.p), static_cast<uint8_t*>(s.msgs.p),
                   static_cast<uint64_t*>(s.off.p)};
  if ((err = upload(h, false, 0, s.sigs.p, s.pks.p, s.off.p, s.msgs.p, cs))) return err;
  if (!own) {
    HIPOK(hipEventRecord(s.copied, c.hcp), "record");
    HIPOK(hipStreamWaitEvent(c.hac, s.copied, 0), "wait copy");
  }
  return async_run(c, s, t, d, mbase, n, accept, digests, ks, ticket, [&](uint8_t* d_acc) {
    return own ? launch_own(c, s.cb, d.sigs, d.pks, d.msgs, d.off, mbase, n, d_acc, ks, lflags)
               : launch(c, d.sigs, d.pks, d.msgs, d.off, mbase, n, d_acc, ks, lflags);
  });
}

// Per-verify cost in SHA-512-block units for the shard split: W(m) of SURVEY.md
// section 8d is 217,600 + 5,500 * blocks INT32 ops, i.e. ~40 blocks' worth of
// fixed work (decompress, scalar multiplication, encode) per signature.
constexpr uint64_t kVerifyBlocks = 40;

// Split [0, n) into g contiguous shards by request index: equal counts when
// every message has the same SHA-512 block count (C2/C3), else equal estimated
// cost, sum over the shard of (kVerifyBlocks + blocks_i) (C4).
void shard_bounds(const uint64_t* off, uint64_t n, uint32_t g, uint64_t* b, int uniform = -1) {
  b[0] = 0;
  b[g] = n;
  if (g == 1) return;
  if (n == 0 || uniform == 1 || (uniform < 0 && scan_offsets(off, 0, n).uniform)) {
    for (uint32_t k = 1; k < g; k++) b[k] = uint64_t((unsigned __int128)n * k / g);
    return;
  }
  // total cost = kVerifyBlocks * n + sum of blocks; shard k starts at the first
  // request whose prefix cost reaches total * k / g
  unsigned __int128 total = 0;
  for (uint64_t i = 0; i < n; i++) total += kVerifyBlocks + sha512_blocks(off, i);
  unsigned __int128 pre = 0;
  uint32_t k = 1;
  for (uint64_t i = 0; i < n && k < g; i++) {
    while (k < g && pre * g >= total * k) b[k++] = i;
    pre += kVerifyBlocks + sha512_blocks(off, i);
  }
  while (k < g) b[k++] = n;
}

// ---- device placement (several GPUs in one process)
// A shard smaller than one wave per SIMD of a whole MI355X (256 CUs x 4 SIMDs x
// 64 lanes) takes as long as a full one: prep and main run one serial chain per
// lane and a lane's latency, not the lane count, sets the time (profiles/r03/
// e2e_host_parts_s36.jsonl, profiles/r04/latency_vs_n_*.jsonl).  So a batch is
// split only into shards of at least that many requests; a smaller batch (a
// Node's prod: a few hundred, or a single Verifier.verify) runs whole on ONE
// device, with no thread spawned and no other device touched.
// EDV_MIN_SHARD overrides (tests split small batches on purpose).
constexpr uint64_t kMinShard = 65536;
uint64_t min_shard() {
  static const uint64_t v = [] {
    if (const char* e = getenv("EDV_MIN_SHARD")) {
      const long long x = strtoll(e, nullptr, 10);
      if (x >= 1) return uint64_t(x);
    }
    return kMinShard;
  }();
  return v;
}

// Asynchronous batches of a context still running on the GPU: slots holding a
// ticket whose done event has not completed (a batch stops counting as soon as
// it is finished, waited for or not).  If another thread holds the context's
// lock, a call is running there: count it as one.
int async_running(DevCtx& c) {
  std::unique_lock<std::mutex> lk(c.mu, std::try_to_lock);
  if (!lk.owns_lock()) return 1;
  int k = 0;
  for (auto& s : c.as)
    if (s.ticket >= 0 && s.done && hipEventQuery(s.done) == hipErrorNotReady) k++;
  (void)hipGetLastError();  // hipErrorNotReady is not an error of ours
  return k;
}
int device_load(int d) {
  DevCtx& c = *g_ctx[d];
  return c.running.load() + (c.live.load() ? async_running(c) : 0);
}

// Placement of the g shards of a batch on g of the devices `devs` (g == 1: a
// batch that runs on one device).  Preference: initialised devices whose load is
// below `busy_at` (1 for synchronous calls: nothing running; so a process that
// verifies one batch at a time stays on its contexts); then devices not yet
// initialised, in an order that starts at pid mod ndev (the processes of a node
// spread over its GPUs); then the least-loaded busy devices.  Load = synchronous calls placed on the device + its asynchronous
// batches still running.  Chosen devices are reserved (running + 1) under one
// placement lock, so concurrent callers see each other's choices; the caller
// releases them (Placed).
std::mutex g_place_mu;
std::vector<int> place(const std::vector<int>& devs, uint32_t g, int busy_at = 1) {
  const int k = int(devs.size());
  std::vector<int> out;
  std::lock_guard<std::mutex> lk(g_place_mu);
  if (uint32_t(k) <= g) {
    out = devs;
  } else {
    const int start = int(uint64_t(getpid()) % uint64_t(k));
    std::vector<std::pair<int, int>> busy;  // (load, device)
    std::vector<int> idle, fresh;
    for (int j = 0; j < k; j++) {
      const int d = devs[(start + j) % k];
      if (!g_ctx[d]->live.load()) {
        if (g_ctx[d]->running.load()) busy.push_back({g_ctx[d]->running.load(), d});  // being initialised
        else fresh.push_back(d);
        continue;
      }
      const int load = device_load(d);
      if (load < busy_at) idle.push_back(d);
      else busy.push_back({load, d});
    }
    std::stable_sort(busy.begin(), busy.end(), [](const auto& x, const auto& y) { return x.first < y.first; });
    for (int d : idle) out.push_back(d);
    for (int d : fresh) out.push_back(d);
    for (auto& b : busy) out.push_back(b.second);
    out.resize(g);
  }
  for (int d : out) g_ctx[d]->running.fetch_add(1);
  return out;
}
// The asynchronous path's pick (edv_pick_device): an initialised device with
// fewer than two batches running still counts as free -- a Node that keeps one
// prod's batch in flight while it submits the next stays on its context (small
// batches run side by side on their slots' own streams, kSmallAsync), while
// several nodes' prods in flight together spread over the GPUs.
constexpr int kAsyncBusyAt = 2;
int pick_device(const std::vector<int>& devs) {
  if (devs.size() == 1) return devs[0];
  const int d = place(devs, 1, kAsyncBusyAt)[0];
  g_ctx[d]->running.fetch_sub(1);  // a pick only advises (edv_pick_device): no reservation kept
  return d;
}
// Releases a device reserved by place() when the shard on it returns.
struct Placed {
  DevCtx* c;
  ~Placed() { c->running.fetch_sub(1); }
};

std::vector<int> devices_of(uint32_t device_mask, int* err) {
  int ndev;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    ndev = device_count_locked();
  }
  std::vector<int> devs;
  for (int d = 0; d < ndev && d < 32; d++)
    if (device_mask == 0 || (device_mask >> d) & 1u) devs.push_back(d);
  *err = devs.empty() ? set_err(EDV_E_NODEV, "no device selected / visible") : 0;
  return devs;
}

// Validate a host batch and split [0, n) over the devices of device_mask (at
// most one shard per min_shard() requests), one host thread per shard; a batch
// that is one shard runs on the calling thread.  The devices are place()'s
// choice.  shard(ctx, lo, hi) does the work under the context lock.
template <class Shard>
int for_each_shard(const uint64_t* off, uint64_t n, uint32_t device_mask, Shard shard, int uniform = -1) {
  int err;
  std::vector<int> devs = devices_of(device_mask, &err);
  if (err) return err;
  const uint64_t most = n / min_shard();
  const uint32_t g = uint32_t(most < devs.size() ? (most > 1 ? most : 1) : devs.size());
  const std::vector<int> on = place(devs, g);
  auto one = [&](int dev, uint64_t lo, uint64_t hi) {
    Placed placed{g_ctx[dev]};
    CtxLock cl(dev);
    if (cl.err) return cl.err;
    const int rc = shard(*cl.c, lo, hi);
    if (rc) quiesce(*cl.c);
    return rc;
  };
  if (g == 1) return one(on[0], 0, n);
  std::vector<uint64_t> bounds(g + 1);
  shard_bounds(off, n, g, bounds.data(), uniform);
  std::vector<int> rc(g, 0);
  std::vector<std::string> errs(g);
  std::vector<std::thread> th;
  for (uint32_t k = 0; k < g; k++) {
    th.emplace_back([&, k]() {
      rc[k] = one(on[k], bounds[k], bounds[k + 1]);
      errs[k] = g_err;
    });
  }
  for (auto& t : th) t.join();
  for (uint32_t k = 0; k < g; k++)
    if (rc[k]) { g_err = errs[k]; return rc[k]; }
  return 0;
}

// One pass over the offsets: valid (non-decreasing), and -- into *uniform if
// asked -- whether every message has the same SHA-512 block count.
constexpr uint64_t kDeferScanMin = 16384;  // see edv_verify_batch
int check_offsets(const uint64_t* msg_off, uint64_t n, bool* uniform = nullptr) {
  const OffScan sc = scan_offsets(msg_off, 0, n);
  if (!sc.ok) return set_err(EDV_E_ARG, "msg_off not non-decreasing");
  if (uniform) *uniform = sc.uniform;
  return 0;
}

// device pointers the kernels read as 16-byte vectors must be 16-byte aligned
int check_dev_align(const void* d_sigs, const void* d_pks, const void* d_off) {
  if ((reinterpret_cast<uintptr_t>(d_sigs) & 15) || (reinterpret_cast<uintptr_t>(d_pks) & 15) ||
      (reinterpret_cast<uintptr_t>(d_off) & 7))
    return set_err(EDV_E_ARG, "d_sigs / d_pks must be 16-byte and d_msg_off 8-byte aligned");
  return 0;
}

// ---- context lifecycle (edv_prepare, edv_self_test, edv_trim, edv_release)
// An asynchronous batch not yet handed over, or a pipelined batch not yet
// synced, still owns caller buffers: the context cannot be trimmed or released.
bool ctx_busy(const DevCtx& c) {
  for (const auto& s : c.as)
    if (s.ticket >= 0) return true;
  return c.pending[0] || c.pending[1];
}

// Message bytes per request the warm-up batches of edv_prepare carry (what a
// buffer may hold per request of keep_batch and still survive edv_trim:
// kTrimMsgBytes, edv_hostplan.h).
constexpr uint64_t kPrepareMsgBytes = 512;
constexpr uint64_t kPrepareMax = uint64_t(1) << 20;  // a warm-up batch is built in host memory: 0.7 GB here

// Free what is larger than a batch of `keep` requests needs (0: everything),
// after the context is drained.  Caller holds c.mu; the current device is c.phys.
void trim_buffers(DevCtx& c, uint64_t keep) {
  const uint64_t k = keep;
  const TrimLimits t = trim_limits(keep, c.chunk);  // edv_hostplan.h
  const uint64_t kq = k < kQuadMaxLimit ? k : kQuadMaxLimit;
  const uint64_t qtab = kq > kRtlMax ? (kq + 63) / 64 * 64 * kQSigWords * 4 : 0;
  auto dev = [](auto& b, uint64_t limit) {  // a DevBuf or a PinnedBuf: freed if larger
    if (b.cap > limit) b.release();
  };
  auto set = [&](ChunkBufs& b) {
    if (b.cap > t.slots) b.release();
  };
  set(c.st);
  set(c.pst[0]);
  set(c.pst[1]);
  dev(c.sigs, t.sigs);
  dev(c.pks, t.pks);
  dev(c.msgs, t.msgs);
  dev(c.off, t.off);
  dev(c.acc, t.acc);
  dev(c.fblob, t.packed);
  dev(c.qblob, t.blob);
  dev(c.qtab, qtab);
  dev(c.qstage, t.stage);
  dev(c.acc_host, t.acc_host);
  for (int q = 0; q < kQ; q++) dev(c.stage[q], t.stage);
  c.mk.trim(merkle_trim_limits(keep, t));
  for (auto& a : c.as) {
    set(a.cb);
    dev(a.sigs, t.sigs);
    dev(a.pks, t.pks);
    dev(a.msgs, t.blob);  // the latency path packs the whole batch here
    dev(a.off, t.slot_off);
    dev(a.acc, t.acc);
    dev(a.dig, t.dig);
    dev(a.qtab, qtab);
    dev(a.stage, t.stage);
    dev(a.acc_host, t.acc_host);
    dev(a.dig_host, t.dig_host);
  }
}

// Drop the holds on the table sets a batch of `keep` requests would not run
// against under the device's policy in a fresh context (under `auto` below
// kLargeTablesMin: the large set); all = both.  Caller holds c.mu, the context
// is drained, the current device is c.phys.
void trim_tables(DevCtx& c, uint64_t keep, bool all) {
  const int keepset = all ? int(kSetNone) : choose_tables(c.policy, keep, false, false, false).use;
  if (c.sb_large && keepset != kSetLarge) {
    drop_tables(c.phys, sb_large());
    c.sb_large = nullptr;
  }
  // the compact set goes only when the set used instead is there
  if (c.sb_compact && (all || (keepset == kSetLarge && c.sb_large))) {
    drop_tables(c.phys, sb_compact());
    c.sb_compact = nullptr;
  }
}

// Back to the state before ctx_init: no stream, event, buffer or table hold.
// The settings (chunk, policy, latency path, ...) and the ledger stay.
void ctx_destroy(DevCtx& c) {
  trim_buffers(c, 0);
  trim_tables(c, 0, true);
  if (c.comb) (void)hipFree(c.comb);
  c.comb = nullptr;
  for_each_event(c, [](hipEvent_t& e, bool) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  });
  for_each_stream(c, [](hipStream_t& s, bool) {
    if (s) (void)hipStreamDestroy(s);
    s = nullptr;
  });
  for (auto& a : c.as) {
    a.ticket = -1;
    a.verdicts = VerdictSink();
    a.digests = nullptr;
    a.n = 0;
  }
  c.pending[0] = c.pending[1] = false;
  c.pipe_ready = false;
  c.next = 0;
  c.ready = false;
  c.live.store(false);
}

// A batch of n requests laid out as edv_verify_batch takes it, in one block
// (signatures | keys | offsets | messages | verdicts | digests), in pageable
// or page-locked memory: the self-test's cases in turn with their own messages
// and verdicts (pad == 0), or the cases' signatures and keys over `pad` zero
// bytes each (a warm-up batch: its verdicts mean nothing).
struct KatBatch {
  std::vector<uint8_t> heap;
  uint8_t* base = nullptr;
  bool pinned = false;
  uint64_t n = 0;
  uint8_t *sigs = nullptr, *pks = nullptr, *msgs = nullptr, *accept = nullptr, *digests = nullptr;
  uint64_t* off = nullptr;
  std::vector<uint8_t> want;
  int build(uint64_t count, uint64_t pad, bool pin) {
    n = count;
    pinned = pin;
    const SelfTestCase* k = selftest_cases();
    uint64_t mbytes = 0;
    for (uint64_t i = 0; i < n; i++) mbytes += pad ? pad : k[i % kSelfTestCases].mlen;
    const uint64_t o_off = 96 * n, o_msg = o_off + 8 * (n + 1), o_acc = (o_msg + mbytes + 64 + 15) / 16 * 16,
                   o_dig = (o_acc + n + 15) / 16 * 16, total = o_dig + 32 * n;
    if (pin) {
      void* p = nullptr;
      if (hipHostMalloc(&p, total, hipHostMallocPortable) != hipSuccess) return set_err(EDV_E_OOM, "hipHostMalloc");
      base = static_cast<uint8_t*>(p);
      memset(base, 0, total);
    }
    try {  // the C-ABI never throws
      if (!pin) heap.assign(total, 0);
      want.resize(n);
    } catch (const std::bad_alloc&) {
      return set_err(EDV_E_OOM, "host memory for a self-test batch");
    }
    if (!pin) base = heap.data();
    sigs = base;
    pks = base + 64 * n;
    off = reinterpret_cast<uint64_t*>(base + o_off);
    msgs = base + o_msg;
    accept = base + o_acc;
    digests = base + o_dig;
    uint64_t pos = 0;
    for (uint64_t i = 0; i < n; i++) {
      const SelfTestCase& t = k[i % kSelfTestCases];
      memcpy(sigs + 64 * i, t.sig, 64);
      memcpy(pks + 32 * i, t.pk, 32);
      off[i] = pos;
      if (!pad) memcpy(msgs + pos, t.msg, t.mlen);
      pos += pad ? pad : t.mlen;
      want[i] = t.accept;
    }
    off[n] = pos;
    return 0;
  }
  ~KatBatch() {
    if (pinned && base) (void)hipHostFree(base);
  }
};

// One family of edv_self_test: the case list tiled to the smallest batch that
// routes to the family's kernels, through the synchronous path, every verdict
// compared with libsodium's.  Caller holds c.mu.
int selftest_family(DevCtx& c, uint32_t family) {
  const char* name = family == EDV_SELFTEST_RTL ? "RTL" : family == EDV_SELFTEST_TWO_WALK ? "TWO_WALK" : "BATCH";
  const uint64_t n = family == EDV_SELFTEST_RTL ? 16 : family == EDV_SELFTEST_TWO_WALK ? kRtlMax + 1 : 256;
  KatBatch b;
  int err;
  if ((err = b.build(n, 0, false))) return err;
  // the latency kernels whatever the device's latency-path limit is (n picks
  // the kernel), or the batch kernels with that limit bypassed for this call
  err = family == EDV_SELFTEST_BATCH ? run_shard(c, b.sigs, b.pks, b.msgs, b.off, 0, n, b.accept, -1, true)
                                     : run_shard_quad(c, b.sigs, b.pks, b.msgs, b.off, 0, n, b.accept);
  if (err) {
    quiesce(c);
    return err;
  }
  for (uint64_t i = 0; i < n; i++) {
    if (b.accept[i] == b.want[i]) continue;
    char buf[160];
    snprintf(buf, sizeof buf, "self-test failed: family %s, case %d (request %llu of %llu): verdict %d, libsodium's %d",
             name, int(i % kSelfTestCases), (unsigned long long)i, (unsigned long long)n, int(b.accept[i]),
             int(b.want[i]));
    return set_err(EDV_E_SELFTEST, buf);
  }
  return 0;
}
int run_selftest(DevCtx& c, uint32_t families) {
  int err;
  for (uint32_t f : {uint32_t(EDV_SELFTEST_RTL), uint32_t(EDV_SELFTEST_TWO_WALK), uint32_t(EDV_SELFTEST_BATCH)})
    if ((families & f) && (err = selftest_family(c, f))) return err;
  return 0;
}

// One warm-up batch of n requests through the synchronous path, and through
// every asynchronous slot if asked (with digests, as a Node's prod asks for
// them), so that the buffers and table sets such a batch needs exist.
int warm_up(DevCtx& c, uint64_t n, bool async, bool pin) {
  KatBatch b;
  int err;
  if ((err = b.build(n, kPrepareMsgBytes, pin))) return err;
  if ((err = run_shard(c, b.sigs, b.pks, b.msgs, b.off, 0, n, b.accept, 1))) {
    quiesce(c);
    return err;
  }
  for (int k = 0; async && k < kAsyncSlots; k++) {
    int64_t t = -1;
    DevCtx::AsyncSlot& s = c.as[c.ledger.next % kAsyncSlots];
    if ((err = submit_async(c, b.sigs, b.pks, b.msgs, b.off, n, b.accept, b.digests, true, &t))) {
      quiesce(c);
      return err;
    }
    if ((err = async_complete(c, s))) return err;
  }
  return 0;
}

// edv_trim / edv_release: f on the context of `device`, idle and drained, under its lock (no context: nothing to do)
template <class F>
int on_drained_ctx(int device, const char* busy, F f) {
  g_err.clear();
  int err = 0;
  DevCtx* c = get_ctx(device, &err);
  if (!c) return err;
  std::lock_guard<std::mutex> lk(c->mu);
  if (c->ready) {
    if (ctx_busy(*c)) return set_err(EDV_E_BUSY, busy);
    HIPOK(hipSetDevice(c->phys), "hipSetDevice");
    if ((err = drain(*c))) return err;
    f(*c);
  }
  c->sb_failed = false;
  return 0;
}

// The edv_set_* of a setting that needs no context made: set under the device's lock, if the value is valid
template <class F>
int set_on_ctx(int device, bool valid, const char* what, F set) {
  g_err.clear();
  int err = 0;
  DevCtx* c = get_ctx(device, &err);
  if (!c) return err;
  if (!valid) return set_err(EDV_E_ARG, what);
  std::lock_guard<std::mutex> lk(c->mu);
  set(*c);
  return 0;
}
}  // namespace

// ------------------------------------------------------------------ C-ABI
extern "C" {

// Builds whose verdicts are not libsodium's say so in their version string;
// edv.lib() refuses them unless EDV_ALLOW_MEASUREMENT_LIB=1.
#if defined(EDV_MEASURE_NO_VERIFY)
const char* edv_version(void) { return "edv 0.2.0 gfx950 MEASUREMENT-ONLY: verification skipped"; }
#else
const char* edv_version(void) { return "edv 0.2.0 gfx950"; }
#endif
const char* edv_last_error(void) { return g_err.c_str(); }

int edv_device_count(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  return device_count_locked();
}

int edv_context_count(void) {
  std::lock_guard<std::mutex> lk(g_mu);
  const int n = device_count_locked();
  int k = 0;
  for (int d = 0; d < n; d++) k += g_ctx[d]->live.load() ? 1 : 0;
  return k;
}

int edv_context_memory(int device, uint64_t out[7]) {
  g_err.clear();
  if (!out) return set_err(EDV_E_ARG, "null pointer");
  for (int k = 0; k < 7; k++) out[k] = 0;
  int err = 0;
  DevCtx* c = get_ctx(device, &err);
  if (!c) return err;
  std::lock_guard<std::mutex> lk(c->mu);
  if (!c->ready) return 0;
  out[1] = shared_tables_bytes(c->phys);
  out[2] = c->st.bytes() + c->mk.bytes();
  for (const auto& a : c->as)
    out[3] += a.sigs.cap + a.pks.cap + a.msgs.cap + a.off.cap + a.acc.cap + a.dig.cap + a.cb.bytes() + a.qtab.cap;
  out[4] = c->pst[0].bytes() + c->pst[1].bytes();
  out[5] = c->sigs.cap + c->pks.cap + c->msgs.cap + c->off.cap + c->acc.cap + c->fblob.cap + c->qblob.cap +
           c->qtab.cap;
  out[6] = c->comb ? uint64_t(kCombRows) * kCombEntries * kBStride * 4 : 0;
  for (int k = 1; k < 7; k++) out[0] += out[k];
  return 0;
}

int edv_pick_device(uint32_t device_mask) {
  g_err.clear();
  int err;
  const std::vector<int> devs = devices_of(device_mask, &err);
  if (err) return err;
  return pick_device(devs);
}

int edv_shard_split(const uint64_t* msg_off, uint64_t n, uint32_t g, uint64_t* bounds) {
  g_err.clear();
  if (!bounds || g == 0 || (n > 0 && !msg_off)) return set_err(EDV_E_ARG, "null pointer / zero shards");
  int err;
  if (n > 0 && (err = check_offsets(msg_off, n))) return err;
  shard_bounds(msg_off, n, g, bounds);
  return 0;
}

int edv_verify_batch(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* msg_off,
                     uint64_t n, uint8_t* accept, uint32_t device_mask) {
  g_err.clear();
  if (n == 0) return 0;
  if (!sigs || !pks || !msg_off || !accept) return set_err(EDV_E_ARG, "null pointer");
  if (!msgs && msg_off[n] != msg_off[0]) return set_err(EDV_E_ARG, "null msgs");
  int err;
  // A batch that runs as one shard (below 2 x min_shard()) has its offsets
  // checked by the shard path itself, while its first copy is in flight (the
  // scan of a C2 batch's 65,537 offsets is a few tens of microseconds of host
  // time before the first byte would otherwise move); a small batch, or one
  // that is split over devices (the split needs the scan), is checked here.
  int uniform = -1;
  if (msg_off[n] < msg_off[0]) return set_err(EDV_E_ARG, "msg_off not non-decreasing");
  if (n < kDeferScanMin || n / min_shard() >= 2) {
    bool u = false;
    if ((err = check_offsets(msg_off, n, &u))) return err;
    uniform = u ? 1 : 0;
  }
  memset(accept, 0, n);  // fail closed: a call that fails part-way leaves rejections
  return for_each_shard(
      msg_off, n, device_mask,
      [&](DevCtx& c, uint64_t lo, uint64_t hi) { return run_shard(c, sigs, pks, msgs, msg_off, lo, hi, accept, uniform); },
      uniform);
}

int edv_verify_batch_async(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs, const uint64_t* msg_off,
                           uint64_t n, uint8_t* accept, int device, int64_t* ticket) {
  return edv_verify_digest_batch_async(sigs, pks, msgs, msg_off, n, accept, nullptr, device, ticket);
}

int edv_verify_digest_batch_async(const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
                                  const uint64_t* msg_off, uint64_t n, uint8_t* accept, uint8_t* digests, int device,
                                  int64_t* ticket) {
  g_err.clear();
  if (!ticket) return set_err(EDV_E_ARG, "null ticket");
  if (n > 0 && (!sigs || !pks || !msg_off || !accept)) return set_err(EDV_E_ARG, "null pointer");
  if (n > 0 && !msgs && msg_off[n] != msg_off[0]) return set_err(EDV_E_ARG, "null msgs");
  int err;
  bool uniform = false;
  if (n > 0 && (err = check_offsets(msg_off, n, &uniform))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  if (n == 0) {
    *ticket = cl.c->ledger.issue();
    return 0;
  }
  if ((err = submit_async(*cl.c, sigs, pks, msgs, msg_off, n, accept, digests, uniform, ticket))) {
    // whatever was queued before the failure may still read the caller's
    // buffers: let it finish before the caller gets the error back
    quiesce(*cl.c);
  }
  return err;
}

int edv_wait_async(int device, int64_t ticket) {
  g_err.clear();
  CtxLock cl(device);
  if (cl.err) return cl.err;
  if (!cl.c->ledger.known(ticket)) return set_err(EDV_E_ARG, "unknown ticket");
  for (auto& s : cl.c->as) {
    if (s.ticket != ticket) continue;
    // wait without holding the device lock (other threads keep submitting);
    // a submission that reuses the slot meanwhile completes this batch itself
    const hipEvent_t done = s.done;
    cl.lk.unlock();
    const hipError_t e = hipEventSynchronize(done);
    cl.lk.lock();
    if (e != hipSuccess) {
      if (s.ticket == ticket) async_fail(*cl.c, s);
      return set_err(EDV_E_HIP, "async wait", e);
    }
    if (s.ticket == ticket) return async_complete(*cl.c, s);
    break;  // a submission reusing the slot completed it meanwhile: its outcome is in the ledger
  }
  // already complete (waited for, or its slot was reused) -- unless a batch at
  // or after it failed (sticky, edv_ledger.h)
  if (cl.c->ledger.settled(ticket) != 0) return set_err(EDV_E_HIP, "async batch failed earlier");
  return 0;
}

int edv_query_async(int device, int64_t ticket) {
  g_err.clear();
  CtxLock cl(device);
  if (cl.err) return cl.err;
  if (!cl.c->ledger.known(ticket)) return set_err(EDV_E_ARG, "unknown ticket");
  for (auto& s : cl.c->as) {
    if (s.ticket != ticket) continue;
    const hipError_t e = hipEventQuery(s.done);
    if (e == hipErrorNotReady) {
      (void)hipGetLastError();
      return EDV_PENDING;
    }
    if (e != hipSuccess) {
      async_fail(*cl.c, s);
      return set_err(EDV_E_HIP, "async query", e);
    }
    return async_complete(*cl.c, s);  // done: hand over as edv_wait_async would, without blocking
  }
  if (cl.c->ledger.settled(ticket) != 0) return set_err(EDV_E_HIP, "async batch failed earlier");
  return 0;
}

int edv_sha256_batch(const uint8_t* msgs, const uint64_t* msg_off, uint64_t n, uint8_t* out, uint32_t device_mask) {
  g_err.clear();
  if (n == 0) return 0;
  if (!msg_off || !out) return set_err(EDV_E_ARG, "null pointer");
  if (!msgs && msg_off[n] != msg_off[0]) return set_err(EDV_E_ARG, "null msgs");
  int err;
  if ((err = check_offsets(msg_off, n))) return err;
  return for_each_shard(msg_off, n, device_mask, [&](DevCtx& c, uint64_t lo, uint64_t hi) {
    return run_digest_shard(c, msgs, msg_off, lo, hi, out);
  });
}

int edv_pack_bits_dev(const uint8_t* d_accept, uint64_t n, uint8_t* d_bits, int device, void* stream) {
  g_err.clear();
  if (n == 0) return 0;
  if (!d_accept || !d_bits) return set_err(EDV_E_ARG, "null pointer");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  // after every verify launched on this device so far, on whatever stream:
  // the ordinary paths record st_done after their last kernel, the pipelined
  // path main_done per state set
  HIPOK(hipStreamWaitEvent(s, c->st_done, 0), "wait verdicts");
  if (c->pipe_ready)
    for (int b = 0; b < 2; b++)
      if (c->pending[b]) HIPOK(hipStreamWaitEvent(s, c->main_done[b], 0), "wait verdicts");
  HIPOK(launch_pack_bits_kernel(s, d_accept, n, d_bits), "pack bits launch");
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

int edv_sha256_batch_dev(const uint8_t* d_msgs, const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n,
                         uint8_t* d_out, int device, void* stream) {
  g_err.clear();
  // before anything reaches the GPU: the kernel reads the offsets as 64-bit
  // words and stores each digest as two 16-byte vectors
  if (n && (!d_msgs || !d_msg_off || !d_out)) return set_err(EDV_E_ARG, "sha256: null d_msgs / d_msg_off / d_out");
  if ((reinterpret_cast<uintptr_t>(d_msg_off) & 7) || (reinterpret_cast<uintptr_t>(d_out) & 15))
    return set_err(EDV_E_ARG, "sha256: d_msg_off must be 8-byte and d_out 16-byte aligned");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  int err;
  if ((err = launch_sha256(d_msgs, d_msg_off, msg_base, n, d_out, s))) return err;
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

int edv_merkle_extend(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves, const uint64_t* leaf_off,
                      uint64_t n, uint8_t* leaf_hashes, uint8_t* node_hashes, uint8_t* new_hashes, uint8_t* root,
                      int device) {
  return edv_merkle_append_batch(old_size, old_hashes, leaves, leaf_off, n, leaf_hashes, node_hashes, new_hashes, root,
                                 nullptr, nullptr, device);
}

// What both forms of an append check first: the sizes and the pointers every
// call needs; d: "d_" for the device form's names in the messages.
static int check_append_args(uint64_t old_size, uint64_t n, const void* old_hashes, const void* new_hashes,
                             const void* root, const std::string& d) {
  if (n > EDV_MERKLE_MAX_LEAVES) return set_err(EDV_E_ARG, "merkle: more than EDV_MERKLE_MAX_LEAVES leaves");
  if (old_size > kMerkleMaxSize || old_size + n > kMerkleMaxSize) return set_err(EDV_E_ARG, "merkle: tree size above 2^62");
  if (old_size && !old_hashes) return set_err(EDV_E_ARG, ("merkle: null " + d + "old_hashes").c_str());
  if (!new_hashes || !root) return set_err(EDV_E_ARG, ("merkle: null " + d + "new_hashes / " + d + "root").c_str());
  return 0;
}

int edv_merkle_append_batch(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves,
                            const uint64_t* leaf_off, uint64_t n, uint8_t* leaf_hashes, uint8_t* node_hashes,
                            uint8_t* new_hashes, uint8_t* root, uint8_t* roots, uint8_t* audit_paths, int device) {
  g_err.clear();
  int err;
  if ((err = check_append_args(old_size, n, old_hashes, new_hashes, root, ""))) return err;
  if (n) {
    if (!leaf_off) return set_err(EDV_E_ARG, "merkle: null leaf_off");
    if ((err = check_offsets(leaf_off, n))) return err;
    if (!leaves && leaf_off[n] != leaf_off[0]) return set_err(EDV_E_ARG, "merkle: null leaves");
  }
  CtxLock cl(device);
  if (cl.err) return cl.err;
  return run_merkle_host(*cl.c, old_size, old_hashes, leaves, leaf_off, n, leaf_hashes, node_hashes, new_hashes, root,
                         roots, audit_paths);
}

int edv_merkle_path_entries(uint64_t old_size, uint64_t n, uint64_t* entries) {
  g_err.clear();
  if (!entries) return set_err(EDV_E_ARG, "merkle: null entries");
  if (old_size > kMerkleMaxSize || n > kMerkleMaxSize || old_size + n > kMerkleMaxSize)
    return set_err(EDV_E_ARG, "merkle: tree size above 2^62");
  *entries = merkle_path_entries(old_size, n);
  return 0;
}

int edv_merkle_extend_dev(uint64_t old_size, const uint8_t* d_old_hashes, const uint8_t* d_leaves,
                          const uint64_t* d_leaf_off, uint64_t leaf_base, uint64_t n, uint8_t* d_leaf_hashes,
                          uint8_t* d_node_hashes, uint8_t* d_new_hashes, uint8_t* d_root, int device, void* stream) {
  return edv_merkle_append_batch_dev(old_size, d_old_hashes, d_leaves, d_leaf_off, leaf_base, n, d_leaf_hashes,
                                     d_node_hashes, d_new_hashes, d_root, nullptr, nullptr, device, stream);
}

int edv_merkle_append_batch_dev(uint64_t old_size, const uint8_t* d_old_hashes, const uint8_t* d_leaves,
                                const uint64_t* d_leaf_off, uint64_t leaf_base, uint64_t n, uint8_t* d_leaf_hashes,
                                uint8_t* d_node_hashes, uint8_t* d_new_hashes, uint8_t* d_root, uint8_t* d_roots,
                                uint8_t* d_audit_paths, int device, void* stream) {
  g_err.clear();
  int err;
  if ((err = check_append_args(old_size, n, d_old_hashes, d_new_hashes, d_root, "d_"))) return err;
  if (n && (!d_leaves || !d_leaf_off)) return set_err(EDV_E_ARG, "merkle: null d_leaves / d_leaf_off");
  // before anything reaches the GPU: the kernels read the offsets as 64-bit
  // words and read and store every hash as two 16-byte vectors
  if (reinterpret_cast<uintptr_t>(d_leaf_off) & 7) return set_err(EDV_E_ARG, "merkle: d_leaf_off must be 8-byte aligned");
  for (const uint8_t* p : {d_old_hashes, static_cast<const uint8_t*>(d_leaf_hashes),
                           static_cast<const uint8_t*>(d_node_hashes), static_cast<const uint8_t*>(d_new_hashes),
                           static_cast<const uint8_t*>(d_root), static_cast<const uint8_t*>(d_roots),
                           static_cast<const uint8_t*>(d_audit_paths)})
    if (reinterpret_cast<uintptr_t>(p) & 15) return set_err(EDV_E_ARG, "merkle: hash buffers must be 16-byte aligned");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  if ((err = launch_merkle(*cl.c, old_size, d_old_hashes, d_leaves, d_leaf_off, leaf_base, n, d_leaf_hashes,
                           d_node_hashes, d_new_hashes, d_root, s, d_roots, d_audit_paths)))
    return err;
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// Proof verification (row f-7).  What both forms of a call check before
// anything is launched or written; *empty: n = 0, nothing to do.
static int check_proof_args(uint64_t n, bool both_leaf_forms, std::initializer_list<const void*> required, bool* empty) {
  *empty = n == 0;
  if (n > EDV_MERKLE_MAX_LEAVES) return set_err(EDV_E_ARG, "merkle verify: more than EDV_MERKLE_MAX_LEAVES proofs");
  if (both_leaf_forms) return set_err(EDV_E_ARG, "merkle verify: give leaves or leaf_hashes, not both");
  if (n)
    for (const void* p : required)
      if (!p) return set_err(EDV_E_ARG, "merkle verify: null pointer");
  return 0;
}
static int check_proof_align(std::initializer_list<const void*> words, std::initializer_list<const void*> hashes) {
  for (const void* p : words)
    if (reinterpret_cast<uintptr_t>(p) & 7) return set_err(EDV_E_ARG, "merkle verify: 64-bit arrays must be 8-byte aligned");
  for (const void* p : hashes)
    if (reinterpret_cast<uintptr_t>(p) & 15) return set_err(EDV_E_ARG, "merkle verify: hash buffers must be 16-byte aligned");
  return 0;
}

int edv_merkle_verify_inclusion(const uint8_t* leaves, const uint64_t* leaf_off, const uint8_t* leaf_hashes,
                                const uint64_t* leaf_index, const uint64_t* tree_size, const uint8_t* roots,
                                const uint8_t* proofs, const uint64_t* proof_off, uint64_t n, uint8_t* status,
                                uint8_t* computed, int device) {
  g_err.clear();
  int err;
  bool empty;
  if ((err = check_proof_args(n, leaves && leaf_hashes,
                              {leaves ? static_cast<const void*>(leaves) : leaf_hashes, leaves ? leaf_off : proof_off,
                               leaf_index, tree_size, roots, proofs, proof_off, status},
                              &empty)))
    return err;
  if (empty) return 0;
  if (leaves && (err = check_offsets(leaf_off, n))) return err;
  if ((err = check_offsets(proof_off, n))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  memset(status, EDV_PROOF_UNVERIFIED, n);  // a call that fails part-way leaves rejections
  return run_verify_inclusion_host(*cl.c, leaves, leaf_off, leaf_hashes, leaf_index, tree_size, roots, proofs, proof_off,
                                   n, status, computed);
}

int edv_merkle_verify_inclusion_dev(const uint8_t* d_leaves, const uint64_t* d_leaf_off, uint64_t leaf_base,
                                    const uint8_t* d_leaf_hashes, const uint64_t* d_leaf_index,
                                    const uint64_t* d_tree_size, const uint8_t* d_roots, const uint8_t* d_proofs,
                                    const uint64_t* d_proof_off, uint64_t proof_base, uint64_t n, uint8_t* d_status,
                                    uint8_t* d_computed, int device, void* stream) {
  g_err.clear();
  int err;
  bool empty;
  if ((err = check_proof_args(n, d_leaves && d_leaf_hashes,
                              {d_leaves ? static_cast<const void*>(d_leaves) : d_leaf_hashes,
                               d_leaves ? d_leaf_off : d_proof_off, d_leaf_index, d_tree_size, d_roots, d_proofs,
                               d_proof_off, d_status},
                              &empty)))
    return err;
  // the lanes read sizes, indices and offsets as 64-bit words and every hash as two 16-byte vectors
  if ((err = check_proof_align({d_leaf_off, d_leaf_index, d_tree_size, d_proof_off},
                               {d_leaf_hashes, d_roots, d_proofs, d_computed})))
    return err;
  if (empty) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  HIPOK(launch_merkle_verify_inclusion_kernel(
            s, merkle_verify_inclusion_args(n, d_leaves, d_leaf_off, leaf_base, d_leaf_hashes, d_leaf_index, d_tree_size,
                                            d_roots, d_proofs, d_proof_off, proof_base, d_status, d_computed)),
        "merkle verify launch");
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

int edv_merkle_verify_consistency(const uint64_t* old_size, const uint64_t* new_size, const uint8_t* old_roots,
                                  const uint8_t* new_roots, const uint8_t* proofs, const uint64_t* proof_off, uint64_t n,
                                  uint8_t* status, uint8_t* computed, int device) {
  g_err.clear();
  int err;
  bool empty;
  if ((err = check_proof_args(n, false, {old_size, new_size, old_roots, new_roots, proofs, proof_off, status}, &empty)))
    return err;
  if (empty) return 0;
  if ((err = check_offsets(proof_off, n))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  memset(status, EDV_PROOF_UNVERIFIED, n);
  return run_verify_consistency_host(*cl.c, old_size, new_size, old_roots, new_roots, proofs, proof_off, n, status,
                                     computed);
}

int edv_merkle_verify_consistency_dev(const uint64_t* d_old_size, const uint64_t* d_new_size, const uint8_t* d_old_roots,
                                      const uint8_t* d_new_roots, const uint8_t* d_proofs, const uint64_t* d_proof_off,
                                      uint64_t proof_base, uint64_t n, uint8_t* d_status, uint8_t* d_computed,
                                      int device, void* stream) {
  g_err.clear();
  int err;
  bool empty;
  if ((err = check_proof_args(n, false, {d_old_size, d_new_size, d_old_roots, d_new_roots, d_proofs, d_proof_off, d_status},
                              &empty)))
    return err;
  if ((err = check_proof_align({d_old_size, d_new_size, d_proof_off}, {d_old_roots, d_new_roots, d_proofs, d_computed})))
    return err;
  if (empty) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  HIPOK(launch_merkle_verify_consistency_kernel(
            s, merkle_verify_consistency_args(n, d_old_size, d_new_size, d_old_roots, d_new_roots, d_proofs, d_proof_off,
                                              proof_base, d_status, d_computed)),
        "merkle verify launch");
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// Proof generation (row f-8).  The offset helpers touch no device.
static int prove_offsets(bool consistency, const uint64_t* a, const uint64_t* b, uint64_t n, uint64_t store_leaves,
                         uint64_t* proof_off) {
  g_err.clear();
  if (!proof_off || (n && (!a || !b))) return set_err(EDV_E_ARG, "merkle prove: null pointer");
  merkle_prove_offsets(consistency, a, b, n, store_leaves, proof_off);
  return 0;
}
int edv_merkle_inclusion_offsets(const uint64_t* leaf_index, const uint64_t* tree_size, uint64_t n, uint64_t store_leaves,
                                 uint64_t* proof_off) {
  return prove_offsets(false, leaf_index, tree_size, n, store_leaves, proof_off);
}
int edv_merkle_consistency_offsets(const uint64_t* first, const uint64_t* second, uint64_t n, uint64_t store_leaves,
                                   uint64_t* proof_off) {
  return prove_offsets(true, first, second, n, store_leaves, proof_off);
}

// What both forms of a prove call check before anything is launched or written; *empty: n = 0
static int check_prove_args(uint64_t n, uint64_t store_leaves, const void* leaf_store, const void* node_store,
                            std::initializer_list<const void*> required, bool* empty) {
  *empty = n == 0;
  if (n > EDV_MERKLE_MAX_LEAVES) return set_err(EDV_E_ARG, "merkle prove: more than EDV_MERKLE_MAX_LEAVES proofs");
  if (store_leaves > kMerkleMaxSize) return set_err(EDV_E_ARG, "merkle prove: store_leaves above 2^62");
  if (n)
    for (const void* p : required)
      if (!p) return set_err(EDV_E_ARG, "merkle prove: null pointer");
  if (store_leaves && !leaf_store) return set_err(EDV_E_ARG, "merkle prove: null leaf_store");
  if (store_leaves > 1 && !node_store) return set_err(EDV_E_ARG, "merkle prove: null node_store");
  return 0;
}

static int prove_host(bool consistency, const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves,
                      const uint64_t* a, const uint64_t* b, const uint64_t* proof_off, uint64_t n, uint8_t* proofs,
                      uint8_t* status, uint8_t* out1, uint8_t* out2, int device) {
  g_err.clear();
  int err;
  bool empty;
  if ((err = check_prove_args(n, store_leaves, leaf_store, node_store, {a, b, proof_off, proofs, status}, &empty)))
    return err;
  if (empty) return 0;
  if ((err = check_offsets(proof_off, n))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  memset(status, EDV_PROOF_UNVERIFIED, n);  // a call that fails part-way leaves no proof marked as made
  return consistency ? run_prove_host<true>(*cl.c, leaf_store, node_store, store_leaves, a, b, proof_off, n, proofs,
                                            status, out1, out2)
                     : run_prove_host<false>(*cl.c, leaf_store, node_store, store_leaves, a, b, proof_off, n, proofs,
                                             status, out1, out2);
}
int edv_merkle_prove_inclusion(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves,
                               const uint64_t* leaf_index, const uint64_t* tree_size, const uint64_t* proof_off,
                               uint64_t n, uint8_t* proofs, uint8_t* status, uint8_t* roots, uint8_t* leaf_hashes_out,
                               int device) {
  return prove_host(false, leaf_store, node_store, store_leaves, leaf_index, tree_size, proof_off, n, proofs, status,
                           roots, leaf_hashes_out, device);
}
int edv_merkle_prove_consistency(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves,
                                 const uint64_t* first, const uint64_t* second, const uint64_t* proof_off, uint64_t n,
                                 uint8_t* proofs, uint8_t* status, uint8_t* old_roots, uint8_t* new_roots, int device) {
  return prove_host(true, leaf_store, node_store, store_leaves, first, second, proof_off, n, proofs, status, old_roots,
                          new_roots, device);
}

static int prove_dev(bool consistency, const uint8_t* d_leaf_store, const uint8_t* d_node_store,
                     uint64_t store_leaves, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_proof_off,
                     uint64_t proof_base, uint64_t n, uint8_t* d_proofs, uint8_t* d_status, uint8_t* d_out1, uint8_t* d_out2, int device, void* stream) {
  g_err.clear();
  int err;
  bool empty;
  if ((err = check_prove_args(n, store_leaves, d_leaf_store, d_node_store, {d_a, d_b, d_proof_off, d_proofs, d_status},
                              &empty)))
    return err;
  // the lanes read sizes, indices and offsets as 64-bit words and every hash as two 16-byte vectors
  if ((err = check_proof_align({d_a, d_b, d_proof_off}, {d_leaf_store, d_node_store, d_proofs, d_out1, d_out2}))) return err;
  if (empty) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  if (consistency)
    HIPOK(launch_merkle_prove_consistency_kernel(
              s, merkle_prove_consistency_args(d_leaf_store, d_node_store, store_leaves, d_a, d_b, d_proof_off, proof_base,
                                               n, d_proofs, d_status, d_out1, d_out2)),
          "merkle prove launch");
  else
    HIPOK(launch_merkle_prove_inclusion_kernel(
              s, merkle_prove_inclusion_args(d_leaf_store, d_node_store, store_leaves, d_a, d_b, d_proof_off, proof_base,
                                             n, d_proofs, d_status, d_out1, d_out2)),
          "merkle prove launch");
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}
int edv_merkle_prove_inclusion_dev(const uint8_t* d_leaf_store, const uint8_t* d_node_store, uint64_t store_leaves,
                                   const uint64_t* d_leaf_index, const uint64_t* d_tree_size,
                                   const uint64_t* d_proof_off, uint64_t proof_base, uint64_t n, uint8_t* d_proofs,
                                   uint8_t* d_status, uint8_t* d_roots, uint8_t* d_leaf_hashes_out, int device,
                                   void* stream) {
  return prove_dev(false, d_leaf_store, d_node_store, store_leaves, d_leaf_index, d_tree_size, d_proof_off, proof_base, n,
                          d_proofs, d_status, d_roots, d_leaf_hashes_out, device, stream);
}
int edv_merkle_prove_consistency_dev(const uint8_t* d_leaf_store, const uint8_t* d_node_store, uint64_t store_leaves,
                                     const uint64_t* d_first, const uint64_t* d_second, const uint64_t* d_proof_off,
                                     uint64_t proof_base, uint64_t n, uint8_t* d_proofs, uint8_t* d_status,
                                     uint8_t* d_old_roots, uint8_t* d_new_roots, int device, void* stream) {
  return prove_dev(true, d_leaf_store, d_node_store, store_leaves, d_first, d_second, d_proof_off, proof_base, n, d_proofs,
                         d_status, d_old_roots, d_new_roots, device, stream);
}

// Auditing a stored tree (row f-9).  What both forms of a call check before
// anything is launched or written: the slice [lo, lo + count) against `total`
// entries (the store's nodes or leaves), the summary, the stores a non-empty
// slice reads.
static int check_audit_args(uint64_t store_leaves, uint64_t lo, uint64_t count, uint64_t total, const void* summary,
                            std::initializer_list<const void*> read) {
  if (count > EDV_MERKLE_MAX_LEAVES) return set_err(EDV_E_ARG, "merkle audit: more than EDV_MERKLE_MAX_LEAVES entries");
  if (store_leaves > kMerkleMaxSize) return set_err(EDV_E_ARG, "merkle audit: store_leaves above 2^62");
  if (lo > total || count > total - lo) return set_err(EDV_E_ARG, "merkle audit: the slice reaches past the store");
  if (!summary) return set_err(EDV_E_ARG, "merkle audit: null summary");
  if (count)
    for (const void* p : read)
      if (!p) return set_err(EDV_E_ARG, "merkle audit: null pointer");
  return 0;
}

int edv_merkle_audit_nodes(const uint8_t* leaf_store, const uint8_t* node_store, uint64_t store_leaves, uint64_t node_lo,
                           uint64_t count, uint8_t* status, uint64_t summary[2], int device) {
  g_err.clear();
  if (const int err = check_audit_args(store_leaves, node_lo, count,
                                       store_leaves <= kMerkleMaxSize ? merkle_node_count(store_leaves) : 0, summary,
                                       {leaf_store, node_store}))
    return err;
  merkle_audit_summary_init(summary);
  if (!count) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  if (status) memset(status, EDV_AUDIT_UNCHECKED, count);  // a call that fails part-way leaves nothing marked good
  return run_audit_nodes_host(*cl.c, leaf_store, node_store, node_lo, count, status, summary);
}

int edv_merkle_audit_leaves(const uint8_t* leaf_store, uint64_t store_leaves, uint64_t leaf_lo, const uint8_t* leaves,
                            const uint64_t* leaf_off, uint64_t n, uint8_t* status, uint64_t summary[2], int device) {
  g_err.clear();
  int err;
  if ((err = check_audit_args(store_leaves, leaf_lo, n, store_leaves, summary, {leaf_store, leaf_off}))) return err;
  if (n) {
    if ((err = check_offsets(leaf_off, n))) return err;
    if (!leaves && leaf_off[n] != leaf_off[0]) return set_err(EDV_E_ARG, "merkle audit: null leaves");
  }
  merkle_audit_summary_init(summary);
  if (!n) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  if (status) memset(status, EDV_AUDIT_UNCHECKED, n);
  return run_audit_leaves_host(*cl.c, leaf_store, leaf_lo, leaves, leaf_off, n, status, summary);
}

int edv_merkle_audit_nodes_dev(const uint8_t* d_leaf_store, const uint8_t* d_node_store, uint64_t store_leaves,
                               uint64_t node_lo, uint64_t count, uint8_t* d_status, uint64_t* d_summary, int device,
                               void* stream) {
  g_err.clear();
  int err;
  if ((err = check_audit_args(store_leaves, node_lo, count,
                              store_leaves <= kMerkleMaxSize ? merkle_node_count(store_leaves) : 0, d_summary,
                              {d_leaf_store, d_node_store})))
    return err;
  // the lanes read every hash as two 16-byte vectors; the summary's words are 64-bit atomics' targets
  if ((err = check_proof_align({d_summary}, {d_leaf_store, d_node_store}))) return err;
  if (!count) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  HIPOK(launch_merkle_audit_nodes_kernel(s, merkle_audit_nodes_args(d_leaf_store, d_node_store, node_lo, count, d_status),
                                         d_summary),
        "merkle audit launch");
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

int edv_merkle_audit_leaves_dev(const uint8_t* d_leaf_store, uint64_t store_leaves, uint64_t leaf_lo,
                                const uint8_t* d_leaves, const uint64_t* d_leaf_off, uint64_t leaf_base, uint64_t n,
                                uint8_t* d_status, uint64_t* d_summary, int device, void* stream) {
  g_err.clear();
  int err;
  if ((err = check_audit_args(store_leaves, leaf_lo, n, store_leaves, d_summary, {d_leaf_store, d_leaves, d_leaf_off})))
    return err;
  if ((err = check_proof_align({d_summary, d_leaf_off}, {d_leaf_store}))) return err;
  if (!n) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  HIPOK(launch_merkle_audit_leaves_kernel(
            s, merkle_audit_leaves_args(d_leaf_store, 0, leaf_lo, n, d_leaves, d_leaf_off, leaf_base, d_status), d_summary),
        "merkle audit launch");
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// Extend from leaf hashes (row f-9): the extend's checks, passes and scratch; pass 0 reads hashes.
int edv_merkle_extend_hashed(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaf_hashes, uint64_t n,
                             uint8_t* node_hashes, uint8_t* new_hashes, uint8_t* root, int device) {
  g_err.clear();
  int err;
  if ((err = check_append_args(old_size, n, old_hashes, new_hashes, root, ""))) return err;
  if (n && !leaf_hashes) return set_err(EDV_E_ARG, "merkle: null leaf_hashes");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  return run_merkle_hashed_host(*cl.c, old_size, old_hashes, leaf_hashes, n, node_hashes, new_hashes, root);
}

int edv_merkle_extend_hashed_dev(uint64_t old_size, const uint8_t* d_old_hashes, const uint8_t* d_leaf_hashes, uint64_t n,
                                 uint8_t* d_node_hashes, uint8_t* d_new_hashes, uint8_t* d_root, int device,
                                 void* stream) {
  g_err.clear();
  int err;
  if ((err = check_append_args(old_size, n, d_old_hashes, d_new_hashes, d_root, "d_"))) return err;
  if (n && !d_leaf_hashes) return set_err(EDV_E_ARG, "merkle: null d_leaf_hashes");
  for (const uint8_t* p : {d_old_hashes, d_leaf_hashes, static_cast<const uint8_t*>(d_node_hashes),
                           static_cast<const uint8_t*>(d_new_hashes), static_cast<const uint8_t*>(d_root)})
    if (reinterpret_cast<uintptr_t>(p) & 15) return set_err(EDV_E_ARG, "merkle: hash buffers must be 16-byte aligned");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  if ((err = launch_merkle(*cl.c, old_size, d_old_hashes, nullptr, nullptr, 0, n, nullptr, d_node_hashes, d_new_hashes,
                           d_root, s, nullptr, nullptr, n ? d_leaf_hashes : nullptr)))
    return err;
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

// Catch-up (row f-10).  What both forms check of the sizes and of the pointers
// every call needs; d: "d_" for the device form's names in the messages.
static int check_catchup_args(uint64_t old_size, uint64_t n, uint64_t replies, const void* old_hashes,
                              const void* reply_end, const void* final_root, const void* proof_off, const void* status,
                              const std::string& d) {
  if (n > EDV_MERKLE_MAX_LEAVES) return set_err(EDV_E_ARG, "merkle: more than EDV_MERKLE_MAX_LEAVES leaves");
  if (old_size > kMerkleMaxSize || old_size + n > kMerkleMaxSize) return set_err(EDV_E_ARG, "merkle: tree size above 2^62");
  if (old_size && !old_hashes) return set_err(EDV_E_ARG, ("merkle: null " + d + "old_hashes").c_str());
  if (!reply_end || !final_root || !proof_off || !status)
    return set_err(EDV_E_ARG, ("merkle catchup: null " + d + "reply_end / " + d + "final_root / " + d + "proof_off / " +
                               d + "status").c_str());
  if (replies == 0 && n) return set_err(EDV_E_ARG, "merkle catchup: leaves without a reply");
  if (replies > n + 1) return set_err(EDV_E_ARG, "merkle catchup: more than n + 1 replies");
  return 0;
}

int edv_merkle_catchup(uint64_t old_size, const uint8_t* old_hashes, const uint8_t* leaves, const uint64_t* leaf_off,
                       uint64_t n, const uint64_t* reply_end, uint64_t replies, uint64_t final_size,
                       const uint8_t* final_root, const uint8_t* proofs, const uint64_t* proof_off, uint8_t* leaf_hashes,
                       uint8_t* node_hashes, uint8_t* reply_roots, uint8_t* status, int device) {
  g_err.clear();
  int err;
  if ((err = check_catchup_args(old_size, n, replies, old_hashes, reply_end, final_root, proof_off, status, ""))) return err;
  if (n) {
    if (!leaf_off) return set_err(EDV_E_ARG, "merkle: null leaf_off");
    if ((err = check_offsets(leaf_off, n))) return err;
    if (!leaves && leaf_off[n] != leaf_off[0]) return set_err(EDV_E_ARG, "merkle: null leaves");
  }
  if (replies == 0) return 0;
  for (uint64_t k = 1; k < replies; k++)
    if (reply_end[k] < reply_end[k - 1]) return set_err(EDV_E_ARG, "merkle catchup: reply_end not non-decreasing");
  if (reply_end[replies - 1] != n) return set_err(EDV_E_ARG, "merkle catchup: the last reply does not end at n");
  for (uint64_t k = 0; k < replies; k++)
    if (proof_off[k + 1] < proof_off[k]) return set_err(EDV_E_ARG, "merkle catchup: proof_off not non-decreasing");
  if (!proofs && proof_off[replies] != proof_off[0]) return set_err(EDV_E_ARG, "merkle catchup: null proofs");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  memset(status, EDV_PROOF_UNVERIFIED, replies);  // a call that fails part-way leaves rejections
  return run_merkle_catchup_host(*cl.c, old_size, old_hashes, leaves, leaf_off, n, reply_end, replies, final_size,
                                 final_root, proofs, proof_off, leaf_hashes, node_hashes, reply_roots, status);
}

int edv_merkle_catchup_dev(uint64_t old_size, const uint8_t* d_old_hashes, const uint8_t* d_leaves,
                           const uint64_t* d_leaf_off, uint64_t leaf_base, uint64_t n, const uint64_t* d_reply_end,
                           uint64_t replies, uint64_t final_size, const uint8_t* d_final_root, const uint8_t* d_proofs,
                           const uint64_t* d_proof_off, uint64_t proof_base, uint8_t* d_leaf_hashes,
                           uint8_t* d_node_hashes, uint8_t* d_reply_roots, uint8_t* d_status, int device, void* stream) {
  g_err.clear();
  int err;
  if ((err = check_catchup_args(old_size, n, replies, d_old_hashes, d_reply_end, d_final_root, d_proof_off, d_status, "d_")))
    return err;
  if (n && (!d_leaves || !d_leaf_off)) return set_err(EDV_E_ARG, "merkle: null d_leaves / d_leaf_off");
  // before anything reaches the GPU: the kernels read ends and offsets as 64-bit
  // words and read and store every hash as two 16-byte vectors
  for (const uint64_t* p : {d_leaf_off, d_reply_end, d_proof_off})
    if (reinterpret_cast<uintptr_t>(p) & 7) return set_err(EDV_E_ARG, "merkle catchup: 64-bit arrays must be 8-byte aligned");
  for (const uint8_t* p : {d_old_hashes, d_final_root, d_proofs, static_cast<const uint8_t*>(d_leaf_hashes),
                           static_cast<const uint8_t*>(d_node_hashes), static_cast<const uint8_t*>(d_reply_roots)})
    if (reinterpret_cast<uintptr_t>(p) & 15) return set_err(EDV_E_ARG, "merkle: hash buffers must be 16-byte aligned");
  if (replies == 0) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  if ((err = launch_merkle_catchup(
           *cl.c, merkle_catchup_args(old_size, n, d_old_hashes, d_leaf_hashes, d_node_hashes, d_reply_end, replies,
                                      final_size, d_final_root, d_proofs, d_proof_off, proof_base, d_reply_roots, d_status),
           d_leaves, d_leaf_off, leaf_base, s)))
    return err;
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

int edv_verify_batch_dev_flags(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                               const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept, int device,
                               void* stream, uint32_t flags) {
  g_err.clear();
  int err;
  if ((err = check_dev_align(d_sigs, d_pks, d_msg_off))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : cl.c->stream;
  if ((err = launch(*cl.c, d_sigs, d_pks, d_msgs, d_msg_off, msg_base, n, d_accept, s, flags))) return err;
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

int edv_verify_batch_dev(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                         const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept, int device,
                         void* stream) {
  return edv_verify_batch_dev_flags(d_sigs, d_pks, d_msgs, d_msg_off, msg_base, n, d_accept, device, stream, 0);
}

int edv_verify_batch_dev_pipelined(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                                   const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept,
                                   int device, uint32_t flags) {
  g_err.clear();
  int err;
  if ((err = check_dev_align(d_sigs, d_pks, d_msg_off))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  if (n == 0) return 0;
  return launch_pipelined(*cl.c, d_sigs, d_pks, d_msgs, d_msg_off, msg_base, n, d_accept, flags);
}

int edv_pipeline_sync(int device) {
  g_err.clear();
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  if (!c->pipe_ready) return 0;
  HIPOK(hipStreamSynchronize(c->sp), "pipeline sync");
  HIPOK(hipStreamSynchronize(c->sm), "pipeline sync");
  c->pending[0] = c->pending[1] = false;
  return 0;
}

static int ensure_comb(DevCtx& c) {
  if (c.comb) return 0;
  int32_t* p = nullptr;
  HIPOK(hipMalloc(&p, uint64_t(kCombRows) * kCombEntries * kBStride * 4), "hipMalloc comb");
  hipError_t e = launch_comb_kernel(c.stream, p);
  if (e == hipSuccess) e = hipStreamSynchronize(c.stream);
  if (e != hipSuccess) {
    (void)hipFree(p);
    return set_err(EDV_E_HIP, "comb table", e);
  }
  c.comb = p;
  return 0;
}

int edv_sign_batch_dev(const uint8_t* d_seeds, const uint8_t* d_msgs, const uint64_t* d_msg_off, uint64_t msg_base,
                       uint64_t n, uint8_t* d_pks, uint8_t* d_sigs, int device, void* stream) {
  g_err.clear();
  if ((reinterpret_cast<uintptr_t>(d_seeds) & 15) || (reinterpret_cast<uintptr_t>(d_pks) & 15) ||
      (reinterpret_cast<uintptr_t>(d_sigs) & 15))
    return set_err(EDV_E_ARG, "d_seeds / d_pks / d_sigs must be 16-byte aligned");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  int err;
  if ((err = ensure_comb(*c))) return err;
  if (n == 0) return 0;
  hipStream_t s = stream ? static_cast<hipStream_t>(stream) : c->stream;
  const unsigned blocks = unsigned((n + kBlock - 1) / kBlock);
  HIPOK(launch_sign_kernel(blocks, s, reinterpret_cast<const uint32_t*>(d_seeds), d_msgs, d_msg_off, msg_base, n,
                           reinterpret_cast<uint32_t*>(d_pks), reinterpret_cast<uint32_t*>(d_sigs), c->comb),
        "sign launch");
  if (!stream) HIPOK(hipStreamSynchronize(s), "stream sync");
  return 0;
}

int edv_stream(int device, void** out) {
  g_err.clear();
  CtxLock cl(device);
  if (cl.err) return cl.err;
  *out = static_cast<void*>(cl.c->stream);
  return 0;
}

int edv_sync(int device) {
  g_err.clear();
  CtxLock cl(device);
  if (cl.err) return cl.err;
  HIPOK(hipStreamSynchronize(cl.c->stream), "stream sync");
  return 0;
}

int edv_set_chunk(int device, uint64_t chunk) {
  g_err.clear();
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  if (chunk == 0) chunk = kChunkDefault;
  if (chunk < kBlock || chunk > (uint64_t(1) << 24)) return set_err(EDV_E_ARG, "chunk out of range");
  int err;
  if ((err = drain(*c))) return err;  // nothing may still use the scratch being reallocated
  c->chunk = (chunk / kBlock) * kBlock;  // the scratch grows to it by use
  return 0;
}

int edv_set_host_slices(int device, int slices) {
  return set_on_ctx(device, slices >= 0 && slices <= kSlices, "slices must be 0..8",
                    [&](DevCtx& c) { c.host_slices = slices; });
}
int edv_set_latency_path(int device, uint64_t max_requests) {
  return set_on_ctx(device, max_requests <= kQuadMaxLimit, "latency path is for batches of at most 16,384",
                    [&](DevCtx& c) { c.quad_max = max_requests; });
}
int edv_set_length_buckets(int device, int mode) {
  return set_on_ctx(device, mode >= 0 && mode <= 2, "length-bucket mode must be 0, 1 or 2",
                    [&](DevCtx& c) { c.length_buckets = mode; });
}

int edv_set_table_policy(int device, int policy) {
  g_err.clear();
  if (policy != EDV_TABLES_AUTO && policy != EDV_TABLES_COMPACT && policy != EDV_TABLES_LARGE)
    return set_err(EDV_E_ARG, "table policy must be EDV_TABLES_AUTO, _COMPACT or _LARGE");
  int err = 0;
  DevCtx* c = get_ctx(device, &err);
  if (!c) return err;
  std::lock_guard<std::mutex> lk(c->mu);
  c->policy = policy;  // the next batch builds what it asks for (pick_tables); nothing is freed here
  c->sb_failed = false;
  return 0;
}

int edv_table_state(int device, uint64_t out[4]) {
  g_err.clear();
  if (!out) return set_err(EDV_E_ARG, "null pointer");
  for (int k = 0; k < 4; k++) out[k] = 0;
  int err = 0;
  DevCtx* c = get_ctx(device, &err);
  if (!c) return err;
  std::lock_guard<std::mutex> lk(c->mu);
  out[0] = uint64_t(c->policy);
  out[1] = c->sb_compact ? sb_alloc_bytes(sb_compact()) : 0;
  out[2] = c->sb_large ? sb_alloc_bytes(sb_large()) : 0;
  out[3] = c->sb_failed ? 1 : 0;
  return 0;
}

int edv_self_test(int device, uint32_t families) {
  g_err.clear();
  const uint32_t all = EDV_SELFTEST_RTL | EDV_SELFTEST_TWO_WALK | EDV_SELFTEST_BATCH;
  if (families == 0 || (families & ~all)) return set_err(EDV_E_ARG, "self-test families: a mask of EDV_SELFTEST_*");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  return run_selftest(*cl.c, families);
}

int edv_prepare(int device, uint64_t max_batch, uint32_t flags) {
  g_err.clear();
  if (max_batch == 0 || max_batch > kPrepareMax || (flags & ~uint32_t(EDV_PREPARE_ASYNC)))
    return set_err(EDV_E_ARG, "prepare: 0 < max_batch <= 2^20, flags 0 or EDV_PREPARE_ASYNC");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx& c = *cl.c;
  const bool was_failed = c.sb_failed;
  // one warm-up batch per route a batch of at most max_batch can take: the
  // right-to-left kernel, the two-walk kernel, the batch kernels
  std::vector<uint64_t> sizes = {max_batch < kRtlMax ? max_batch : kRtlMax, max_batch};
  if (c.quad_max) sizes.push_back(max_batch < c.quad_max ? max_batch : c.quad_max);
  std::sort(sizes.begin(), sizes.end());
  sizes.erase(std::unique(sizes.begin(), sizes.end()), sizes.end());
  int err;
  for (const uint64_t n : sizes)
    for (const bool pin : {false, true})
      if ((err = warm_up(c, n, (flags & EDV_PREPARE_ASYNC) != 0, pin))) return err;
  // a build of the large set that failed here: the batches would run (on the
  // compact set), but a Node had better know at start-up
  if (c.sb_failed && !was_failed) return c.sb_err ? c.sb_err : EDV_E_OOM;
  uint32_t families = EDV_SELFTEST_RTL;
  if (max_batch > kRtlMax) families |= EDV_SELFTEST_TWO_WALK;
  if (max_batch > c.quad_max) families |= EDV_SELFTEST_TWO_WALK | EDV_SELFTEST_BATCH;
  return run_selftest(c, families);
}

int edv_trim(int device, uint64_t keep_batch) {
  return on_drained_ctx(device, "trim: asynchronous or pipelined batches not yet handed over", [&](DevCtx& c) {
    trim_buffers(c, keep_batch);
    trim_tables(c, keep_batch, false);
  });
}
int edv_release(int device) {
  return on_drained_ctx(device, "release: asynchronous or pipelined batches not yet handed over", ctx_destroy);
}

int edv_dev_alloc(int device, uint64_t bytes, void** out) {
  int phys, err;
  if ((err = phys_of(device, &phys))) return err;
  HIPOK(hipSetDevice(phys), "hipSetDevice");
  HIPOK(hipMalloc(out, bytes ? bytes : 1), "hipMalloc");
  return 0;
}
int edv_dev_free(int device, void* p) {
  int phys, err;
  if ((err = phys_of(device, &phys))) return err;
  HIPOK(hipSetDevice(phys), "hipSetDevice");
  HIPOK(hipFree(p), "hipFree");
  return 0;
}
int edv_h2d(int device, void* dst, const void* src, uint64_t bytes) {
  int phys, err;
  if ((err = phys_of(device, &phys))) return err;
  HIPOK(hipSetDevice(phys), "hipSetDevice");
  HIPOK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice), "hipMemcpy h2d");
  return 0;
}
int edv_d2h(int device, void* dst, const void* src, uint64_t bytes) {
  int phys, err;
  if ((err = phys_of(device, &phys))) return err;
  HIPOK(hipSetDevice(phys), "hipSetDevice");
  HIPOK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost), "hipMemcpy d2h");
  return 0;
}

int edv_host_alloc(uint64_t bytes, void** out) {
  g_err.clear();
  if (!out) return set_err(EDV_E_ARG, "null pointer");
  int n;
  {
    std::lock_guard<std::mutex> lk(g_mu);
    n = device_count_locked();
  }
  if (n == 0) return set_err(EDV_E_NODEV, "no device visible");
  HIPOK(hipSetDevice(g_ctx[0]->phys), "hipSetDevice");
  if (hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) {
    *out = nullptr;
    return set_err(EDV_E_OOM, "hipHostMalloc");
  }
  return 0;
}
int edv_host_free(void* p) {
  g_err.clear();
  if (p) HIPOK(hipHostFree(p), "hipHostFree");
  return 0;
}

}  // extern "C"

#ifdef EDV_MEASUREMENT_API
#include "edv_measure.inc"
#endif
