// edv_measure.inc -- the measurement entry points of libedv_measure.so
// (include/edv_measure.h): kernel timing on the kernels' own stream, the
// Infinity-Cache flush probe, the prep kernel's sides timed apart, the
// asynchronous path's fault hook, the device math probes and the stage probes
// (prep state out, main on a chosen state, table readback: host code around
// the product's kernels, no device code) and the latency probes (phase 1 out,
// walk on a chosen state: probe kernels of edv_probe_latency.hip, which
// instantiate edv_quad.hip's header functions).  Included at the end of edv_runtime.hip only
// when EDV_MEASUREMENT_API is defined (the Makefile's libedv_measure.so); the
// product libedv.so has none of it.
#include "../../include/edv_measure.h"
#include "edv_probe.h"

namespace {

// HIP events of a measurement helper, destroyed on every return path
struct Events {
  hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr};
  int n = 0;
  int create(int k) {
    for (n = 0; n < k; n++) HIPOK(hipEventCreate(&e[n]), "event");
    return 0;
  }
  ~Events() {
    for (int i = 0; i < n; i++) (void)hipEventDestroy(e[i]);
  }
};

// Read and rewrite a buffer larger than the Infinity Cache, so whatever the
// previous kernel left there (the prep kernel's tables) is evicted before the
// next one runs.
__global__ __launch_bounds__(kBlock) void edv_flush_kernel(int4* p, uint64_t n16) {
  for (uint64_t i = uint64_t(blockIdx.x) * kBlock + threadIdx.x; i < n16; i += uint64_t(gridDim.x) * kBlock) {
    int4 v = p[i];
    v.x += 1;
    p[i] = v;
  }
}

// a device buffer of the stage probes: lives for the call only
struct StageBuf : DevBuf {
  ~StageBuf() {
    if (p) (void)hipFree(p);
  }
};

// elapsed ms between two events, accumulated
int add_elapsed(float* acc, hipEvent_t a, hipEvent_t b) {
  float ms = 0;
  HIPOK(hipEventElapsedTime(&ms, a, b), "elapsed");
  *acc += ms;
  return 0;
}

}  // namespace

extern "C" {

int edv_time_batch_dev(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                       const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept, int device,
                       int iters, float* ms_out) {
  g_err.clear();
  int err;
  if ((err = check_dev_align(d_sigs, d_pks, d_msg_off))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  Events ev;
  if ((err = ev.create(2))) return err;
  HIPOK(hipEventRecord(ev.e[0], c->stream), "record");
  for (int it = 0; it < iters; it++)
    if ((err = launch(*c, d_sigs, d_pks, d_msgs, d_msg_off, msg_base, n, d_accept, c->stream, 0))) return err;
  HIPOK(hipEventRecord(ev.e[1], c->stream), "record");
  HIPOK(hipEventSynchronize(ev.e[1]), "event sync");
  float ms = 0;
  if ((err = add_elapsed(&ms, ev.e[0], ev.e[1]))) return err;
  if (ms_out) *ms_out = ms;
  return 0;
}

int edv_profile_batch_dev_flush(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                                const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept,
                                int device, int iters, uint64_t flush_bytes, float* ms_prep, float* ms_flush,
                                float* ms_main) {
  g_err.clear();
  int err;
  if ((err = check_dev_align(d_sigs, d_pks, d_msg_off))) return err;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  if (n == 0 || n > c->chunk || iters <= 0) return set_err(EDV_E_ARG, "profile needs 0 < n <= chunk, iters > 0");
  if ((err = grow_state(*c, n))) return err;
  const bool bucket = bucketing_enabled(*c, 0);
  VerifyArgs va = make_args(*c, c->st, d_sigs, d_pks, d_msgs, d_msg_off, msg_base, d_accept, bucket, 0, n);
  if (!va.btab) return no_tables(*c);
  va.n = n;
  uint32_t* hist = bucket_ctr(c->st, 0);
  const unsigned blocks = unsigned((n + kBlock - 1) / kBlock);
  // the flush buffer lives for this call only (DevBuf keeps its memory; this frees it)
  struct FlushBuf : DevBuf {
    ~FlushBuf() {
      if (p) (void)hipFree(p);
    }
  } flush;
  flush_bytes &= ~uint64_t(15);
  if (flush_bytes && flush.ensure(flush_bytes)) return EDV_E_OOM;
  if (flush_bytes) HIPOK(hipMemsetAsync(flush.p, 0, flush_bytes, c->stream), "memset flush");
  Events ev;
  if ((err = ev.create(4))) return err;
  HIPOK(hipStreamWaitEvent(c->stream, c->st_done, 0), "wait scratch");
  float tp = 0, tf = 0, tm = 0;
  // iteration -1 is untimed: the first launch of a kernel in a process loads
  // its code object (this library's contexts are separate from the
  // product's, so its kernels start cold even after the bench's timed steps)
  for (int it = -1; it < iters; it++) {
    if (bucket) {
      HIPOK(hipMemsetAsync(hist, 0, 2 * kBuckets * 4, c->stream), "memset buckets");
      HIPOK(launch_bucket_kernels(blocks, c->stream, d_msg_off, 0, n, hist, const_cast<uint32_t*>(va.st.perm)),
            "bucket launch");
    }
    HIPOK(hipEventRecord(ev.e[0], c->stream), "record");
    HIPOK(launch_prep_kernel(3 * blocks, c->stream, va), "prep launch");
    HIPOK(hipEventRecord(ev.e[1], c->stream), "record");
    if (flush_bytes) {
      edv_flush_kernel<<<dim3(4096), dim3(kBlock), 0, c->stream>>>(static_cast<int4*>(flush.p), flush_bytes / 16);
      HIPOK(hipGetLastError(), "flush launch");
    }
    HIPOK(hipEventRecord(ev.e[2], c->stream), "record");
    HIPOK(launch_main_kernel(blocks, c->stream, va, false), "main launch");
    HIPOK(hipEventRecord(ev.e[3], c->stream), "record");
    HIPOK(hipEventSynchronize(ev.e[3]), "event sync");
    if (it < 0) continue;
    if ((err = add_elapsed(&tp, ev.e[0], ev.e[1])) || (err = add_elapsed(&tf, ev.e[1], ev.e[2])) ||
        (err = add_elapsed(&tm, ev.e[2], ev.e[3])))
      return err;
  }
  HIPOK(hipEventRecord(c->st_done, c->stream), "record scratch");
  HIPOK(hipStreamSynchronize(c->stream), "stream sync");  // the flush buffer is freed on return
  if (ms_prep) *ms_prep = tp / iters;
  if (ms_flush) *ms_flush = tf / iters;
  if (ms_main) *ms_main = tm / iters;
  return 0;
}

int edv_profile_batch_dev(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                          const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept, int device,
                          int iters, float* ms_prep, float* ms_main) {
  return edv_profile_batch_dev_flush(d_sigs, d_pks, d_msgs, d_msg_off, msg_base, n, d_accept, device, iters, 0,
                                     ms_prep, nullptr, ms_main);
}

int edv_profile_prep_sides(const uint8_t* d_sigs, const uint8_t* d_pks, const uint8_t* d_msgs,
                           const uint64_t* d_msg_off, uint64_t msg_base, uint64_t n, uint8_t* d_accept, int device,
                           int iters, float ms[5]) {
  g_err.clear();
  int err;
  if ((err = check_dev_align(d_sigs, d_pks, d_msg_off))) return err;
  if (!ms) return set_err(EDV_E_ARG, "null ms");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  if (n == 0 || n > c->chunk || iters <= 0) return set_err(EDV_E_ARG, "profile needs 0 < n <= chunk, iters > 0");
  if ((err = grow_state(*c, n))) return err;
  VerifyArgs va = make_args(*c, c->st, d_sigs, d_pks, d_msgs, d_msg_off, msg_base, d_accept, false, 0, n);
  if (!va.btab) return no_tables(*c);
  va.n = n;
  const unsigned blocks = unsigned((n + kBlock - 1) / kBlock);
  Events ev;
  if ((err = ev.create(2))) return err;
  HIPOK(hipStreamWaitEvent(c->stream, c->st_done, 0), "wait scratch");
  HIPOK(launch_prep_kernel(3 * blocks, c->stream, va), "prep launch");  // untimed: code object load
  const int32_t cfg[5][2] = {{0, 1}, {1, 1}, {2, 1}, {0, 3}, {1, 2}};  // (side0, nsides)
  for (int k = 0; k < 5; k++) {
    VerifyArgs v = va;
    v.side0 = cfg[k][0];
    v.nsides = cfg[k][1];
    float t = 0;
    for (int it = 0; it < iters; it++) {
      HIPOK(hipEventRecord(ev.e[0], c->stream), "record");
      HIPOK(launch_prep_kernel(unsigned(v.nsides) * blocks, c->stream, v), "prep launch");
      HIPOK(hipEventRecord(ev.e[1], c->stream), "record");
      HIPOK(hipEventSynchronize(ev.e[1]), "event sync");
      if ((err = add_elapsed(&t, ev.e[0], ev.e[1]))) return err;
    }
    ms[k] = t / iters;
  }
  HIPOK(hipEventRecord(c->st_done, c->stream), "record scratch");
  HIPOK(hipStreamSynchronize(c->stream), "stream sync");
  return 0;
}

int edv_test_fail_async(int device, int64_t ticket) {
  g_err.clear();
  CtxLock cl(device);
  if (cl.err) return cl.err;
  cl.c->inject_fail = ticket;
  return 0;
}

int edv_probe_math(int device, int op, const void* in, uint64_t in_stride, void* out, uint64_t out_stride,
                   uint64_t n) {
  g_err.clear();
  const ProbeSize sz = probe_size(op);
  if (!sz.in) return set_err(EDV_E_ARG, "probe: unknown op");
  if (!in || !out) return set_err(EDV_E_ARG, "probe: null buffer");
  if (in_stride < sz.in || out_stride < sz.out || (in_stride & 3) || (out_stride & 3) || in_stride > 4096 ||
      out_stride > 4096)
    return set_err(EDV_E_ARG, "probe: strides are multiples of 4, from the op's sizes up to 4096");
  if (n > (uint64_t(1) << 24)) return set_err(EDV_E_ARG, "probe: at most 2^24 cases");
  if (n == 0) return 0;
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  // the two buffers live for this call only
  struct ProbeBuf : DevBuf {
    ~ProbeBuf() {
      if (p) (void)hipFree(p);
    }
  } din, dout;
  if (din.ensure(n * in_stride) || dout.ensure(n * out_stride)) return EDV_E_OOM;
  int err;
  if (op == EDV_PROBE_SCALARMULT_BASE && (err = ensure_comb(*c))) return err;  // the signer's table, as it builds it
  HIPOK(hipMemcpyAsync(din.p, in, n * in_stride, hipMemcpyHostToDevice, c->stream), "probe copy in");
  HIPOK(hipMemsetAsync(dout.p, 0, n * out_stride, c->stream), "probe memset");
  HIPOK(probe_is_quad(op) ? launch_probe_quad(c->stream, op, static_cast<const uint8_t*>(din.p), in_stride,
                                              static_cast<uint8_t*>(dout.p), out_stride, n)
                          : launch_probe_lane(c->stream, op, static_cast<const uint8_t*>(din.p), in_stride,
                                              static_cast<uint8_t*>(dout.p), out_stride, n, c->comb),
        "probe launch");
  HIPOK(hipMemcpyAsync(out, dout.p, n * out_stride, hipMemcpyDeviceToHost, c->stream), "probe copy out");
  HIPOK(hipStreamSynchronize(c->stream), "probe sync");  // the buffers are freed on return
  return 0;
}

// ---- the stage probes (include/edv_measure.h): the product's kernels on a
// state the caller reads back or writes
int edv_probe_prep_state(int device, const uint8_t* sigs, const uint8_t* pks, const uint8_t* msgs,
                         const uint64_t* msg_off, uint64_t n, int set, int side0, int nsides, uint32_t flags,
                         uint32_t* dig, uint8_t* alive, int32_t* atab, int32_t* rtab, uint32_t* perm, uint8_t* accept,
                         uint64_t* cap_out) {
  g_err.clear();
  if (set != EDV_TABLE_SET_COMPACT && set != EDV_TABLE_SET_LARGE) return set_err(EDV_E_ARG, "prep probe: unknown table set");
  if (side0 < 0 || nsides < 1 || side0 > 2 || nsides > 3 || side0 + nsides > 3)
    return set_err(EDV_E_ARG, "prep probe: sides out of range");
  if (flags & ~(EDV_STAGE_BUCKETS | EDV_STAGE_SPLIT)) return set_err(EDV_E_ARG, "prep probe: unknown flag");
  if ((flags & EDV_STAGE_SPLIT) && !(side0 == 0 && nsides == 3))
    return set_err(EDV_E_ARG, "prep probe: the split launches are sides 0 / 3");
  if (n > EDV_STAGE_CAP) return set_err(EDV_E_ARG, "prep probe: at most EDV_STAGE_CAP requests");
  const uint64_t cap = EDV_STAGE_CAP;
  if (cap_out) *cap_out = cap;
  if (n == 0) return 0;
  const bool bucket = flags & EDV_STAGE_BUCKETS;
  if (!sigs || !pks || !msg_off || !dig || !alive || !atab || !rtab || !accept || (bucket && !perm))
    return set_err(EDV_E_ARG, "prep probe: null buffer");
  for (uint64_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i]) return set_err(EDV_E_ARG, "prep probe: msg_off not non-decreasing");
  const uint64_t mbytes = msg_off[n];
  if (mbytes && !msgs) return set_err(EDV_E_ARG, "prep probe: null buffer");
  if (mbytes > (uint64_t(1) << 30)) return set_err(EDV_E_ARG, "prep probe: at most 1 GiB of messages");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  int err = 0;
  const SbShape sh = set == EDV_TABLE_SET_LARGE ? sb_large() : sb_compact();
  const int32_t* tables = shared_tables(c->phys, sh, c->stream, &err);  // this GPU's set, built on first use
  if (!tables) return err;
  StageBuf dsigs, dpks, dmsgs, doff, dacc, datab, drtab, ddig, dalive, dperm, dctr;
  if (dsigs.ensure(64 * n) || dpks.ensure(32 * n) || dmsgs.ensure(mbytes + 64) || doff.ensure(8 * (n + 1)) ||
      dacc.ensure(n) || datab.ensure(n * kAWords * 4) || drtab.ensure(n * kAWords * 4) ||
      ddig.ensure(cap * kDigWords * 4) || dalive.ensure(3 * cap) || dperm.ensure(4 * n) ||
      dctr.ensure(2 * kBuckets * 4))
    return EDV_E_OOM;
  hipStream_t s = c->stream;
  HIPOK(hipMemcpyAsync(dsigs.p, sigs, 64 * n, hipMemcpyHostToDevice, s), "prep probe copy in");
  HIPOK(hipMemcpyAsync(dpks.p, pks, 32 * n, hipMemcpyHostToDevice, s), "prep probe copy in");
  HIPOK(hipMemsetAsync(dmsgs.p, 0, mbytes + 64, s), "prep probe memset");  // the kernels read whole words past a message's end
  if (mbytes) HIPOK(hipMemcpyAsync(dmsgs.p, msgs, mbytes, hipMemcpyHostToDevice, s), "prep probe copy in");
  HIPOK(hipMemcpyAsync(doff.p, msg_off, 8 * (n + 1), hipMemcpyHostToDevice, s), "prep probe copy in");
  HIPOK(hipMemsetAsync(dacc.p, EDV_STAGE_SENTINEL, n, s), "prep probe memset");
  HIPOK(hipMemsetAsync(datab.p, EDV_STAGE_SENTINEL, n * kAWords * 4, s), "prep probe memset");
  HIPOK(hipMemsetAsync(drtab.p, EDV_STAGE_SENTINEL, n * kAWords * 4, s), "prep probe memset");
  HIPOK(hipMemsetAsync(ddig.p, EDV_STAGE_SENTINEL, cap * kDigWords * 4, s), "prep probe memset");
  HIPOK(hipMemsetAsync(dalive.p, EDV_STAGE_SENTINEL, 3 * cap, s), "prep probe memset");
  HIPOK(hipMemsetAsync(dperm.p, EDV_STAGE_SENTINEL, 4 * n, s), "prep probe memset");
  VerifyArgs va;
  va.sigs = static_cast<const uint32_t*>(dsigs.p);
  va.pks = static_cast<const uint32_t*>(dpks.p);
  va.msgs = static_cast<const uint8_t*>(dmsgs.p);
  va.off = static_cast<const uint64_t*>(doff.p);
  va.msg_base = 0;
  va.base = 0;
  va.n = n;
  va.accept = static_cast<uint8_t*>(dacc.p);
  va.st = ChunkState{static_cast<int32_t*>(datab.p), static_cast<int32_t*>(drtab.p), static_cast<uint32_t*>(ddig.p),
                     static_cast<uint8_t*>(dalive.p), cap, bucket ? static_cast<uint32_t*>(dperm.p) : nullptr};
  va.btab = tables;
  va.sb = sh;
  const unsigned blocks = unsigned((n + kBlock - 1) / kBlock);
  if (bucket) {
    HIPOK(hipMemsetAsync(dctr.p, 0, 2 * kBuckets * 4, s), "memset buckets");
    HIPOK(launch_bucket_kernels(blocks, s, va.off, 0, n, static_cast<uint32_t*>(dctr.p),
                                static_cast<uint32_t*>(dperm.p)),
          "bucket launch");
  }
  const int32_t joint[1][2] = {{side0, nsides}}, split[2][2] = {{0, 1}, {1, 2}};  // (side0, nsides) per launch
  const int32_t(*cfg)[2] = (flags & EDV_STAGE_SPLIT) ? split : joint;
  for (int k = 0; k < ((flags & EDV_STAGE_SPLIT) ? 2 : 1); k++) {
    va.side0 = cfg[k][0];
    va.nsides = cfg[k][1];
    HIPOK(launch_prep_kernel(unsigned(va.nsides) * blocks, s, va), "prep launch");
  }
  HIPOK(hipMemcpyAsync(dig, ddig.p, cap * kDigWords * 4, hipMemcpyDeviceToHost, s), "prep probe copy out");
  HIPOK(hipMemcpyAsync(alive, dalive.p, 3 * cap, hipMemcpyDeviceToHost, s), "prep probe copy out");
  HIPOK(hipMemcpyAsync(atab, datab.p, n * kAWords * 4, hipMemcpyDeviceToHost, s), "prep probe copy out");
  HIPOK(hipMemcpyAsync(rtab, drtab.p, n * kAWords * 4, hipMemcpyDeviceToHost, s), "prep probe copy out");
  if (bucket) HIPOK(hipMemcpyAsync(perm, dperm.p, 4 * n, hipMemcpyDeviceToHost, s), "prep probe copy out");
  HIPOK(hipMemcpyAsync(accept, dacc.p, n, hipMemcpyDeviceToHost, s), "prep probe copy out");
  HIPOK(hipStreamSynchronize(s), "prep probe sync");  // the buffers are freed on return
  return 0;
}

int edv_probe_main_state(int device, uint64_t n, uint64_t cap, const uint32_t* dig, const uint8_t* alive,
                         const int32_t* atab, const int32_t* rtab, const uint32_t* perm, uint32_t flags,
                         uint8_t* accept) {
  g_err.clear();
  if (flags & ~EDV_STAGE_PRIO) return set_err(EDV_E_ARG, "main probe: unknown flag");
  if (n > cap || cap > EDV_STAGE_CAP) return set_err(EDV_E_ARG, "main probe: n <= cap <= EDV_STAGE_CAP");
  if (n == 0) return 0;
  if (!dig || !alive || !atab || !rtab || !accept) return set_err(EDV_E_ARG, "main probe: null buffer");
  // the domain the kernel is written for: verdicts land inside accept[0, n),
  // a live slot walks at most kAWindows windows
  for (uint64_t j = 0; j < n; j++) {
    if (perm && perm[j] >= n) return set_err(EDV_E_ARG, "main probe: perm entry out of range");
    if (alive[j] && alive[cap + j] && alive[2 * cap + j] && (dig[uint64_t(kDigNwin) * cap + j] & 0xff) > uint32_t(kAWindows))
      return set_err(EDV_E_ARG, "main probe: window count above kAWindows");
  }
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  StageBuf dacc, datab, drtab, ddig, dalive, dperm;
  if (dacc.ensure(n) || datab.ensure(n * kAWords * 4) || drtab.ensure(n * kAWords * 4) ||
      ddig.ensure(cap * kDigWords * 4) || dalive.ensure(3 * cap) || (perm && dperm.ensure(4 * n)))
    return EDV_E_OOM;
  hipStream_t s = c->stream;
  HIPOK(hipMemcpyAsync(ddig.p, dig, cap * kDigWords * 4, hipMemcpyHostToDevice, s), "main probe copy in");
  HIPOK(hipMemcpyAsync(dalive.p, alive, 3 * cap, hipMemcpyHostToDevice, s), "main probe copy in");
  HIPOK(hipMemcpyAsync(datab.p, atab, n * kAWords * 4, hipMemcpyHostToDevice, s), "main probe copy in");
  HIPOK(hipMemcpyAsync(drtab.p, rtab, n * kAWords * 4, hipMemcpyHostToDevice, s), "main probe copy in");
  if (perm) HIPOK(hipMemcpyAsync(dperm.p, perm, 4 * n, hipMemcpyHostToDevice, s), "main probe copy in");
  HIPOK(hipMemsetAsync(dacc.p, EDV_STAGE_SENTINEL, n, s), "main probe memset");
  VerifyArgs va{};
  va.n = n;
  va.accept = static_cast<uint8_t*>(dacc.p);
  va.st = ChunkState{static_cast<int32_t*>(datab.p), static_cast<int32_t*>(drtab.p), static_cast<uint32_t*>(ddig.p),
                     static_cast<uint8_t*>(dalive.p), cap, perm ? static_cast<uint32_t*>(dperm.p) : nullptr};
  va.nsides = 3;
  HIPOK(launch_main_kernel(unsigned((n + kBlock - 1) / kBlock), s, va, flags & EDV_STAGE_PRIO), "main launch");
  HIPOK(hipMemcpyAsync(accept, dacc.p, n, hipMemcpyDeviceToHost, s), "main probe copy out");
  HIPOK(hipStreamSynchronize(s), "main probe sync");  // the buffers are freed on return
  return 0;
}

int edv_probe_table(int device, int set, const int32_t* tj, uint64_t n, int32_t* out) {
  g_err.clear();
  if (set != EDV_TABLE_SET_COMPACT && set != EDV_TABLE_SET_LARGE && set != EDV_TABLE_SET_COMB)
    return set_err(EDV_E_ARG, "table probe: unknown table set");
  if (n > (uint64_t(1) << 20)) return set_err(EDV_E_ARG, "table probe: at most 2^20 entries");
  if (n == 0) return 0;
  if (!tj || !out) return set_err(EDV_E_ARG, "table probe: null buffer");
  const SbShape sh = set == EDV_TABLE_SET_LARGE ? sb_large() : sb_compact();
  const int rows = set == EDV_TABLE_SET_COMB ? kCombRows : sh.tables;
  const int entries = set == EDV_TABLE_SET_COMB ? kCombEntries : sh.entries;
  for (uint64_t k = 0; k < n; k++)
    if (tj[2 * k] < 0 || tj[2 * k] >= rows || tj[2 * k + 1] < 0 || tj[2 * k + 1] >= entries)
      return set_err(EDV_E_ARG, "table probe: entry out of range");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  int err = 0;
  const int32_t* table;
  if (set == EDV_TABLE_SET_COMB) {
    if ((err = ensure_comb(*c))) return err;
    table = c->comb;
  } else if (!(table = shared_tables(c->phys, sh, c->stream, &err))) {
    return err;
  }
  StageBuf stage;
  if (stage.ensure(n * kBStride * 4)) return EDV_E_OOM;
  // one device-side copy per run of consecutive entries, then one copy out
  for (uint64_t k = 0; k < n;) {
    uint64_t e = k + 1;
    while (e < n && tj[2 * e] == tj[2 * k] && tj[2 * e + 1] == tj[2 * k + 1] + int32_t(e - k)) e++;
    const int32_t* src = table + (size_t(tj[2 * k]) * size_t(entries) + size_t(tj[2 * k + 1])) * kBStride;
    HIPOK(hipMemcpyAsync(static_cast<int32_t*>(stage.p) + k * kBStride, src, (e - k) * kBStride * 4,
                         hipMemcpyDeviceToDevice, c->stream),
          "table probe copy");
    k = e;
  }
  HIPOK(hipMemcpyAsync(out, stage.p, n * kBStride * 4, hipMemcpyDeviceToHost, c->stream), "table probe copy out");
  HIPOK(hipStreamSynchronize(c->stream), "table probe sync");  // the buffer is freed on return
  return 0;
}

// ---- the latency probes (include/edv_measure.h): probe kernels that
// instantiate edv_quad.hip's phase 1 and walks (edv_probe_latency.hip), NOT
// the product's kernel objects
int edv_probe_latency_phase1(int device, int kernel, int set, const uint8_t* sigs, const uint8_t* pks,
                             const uint8_t* msgs, const uint64_t* msg_off, uint64_t n, uint32_t* dig, int32_t* pt,
                             uint8_t* ok, uint8_t* accept) {
  g_err.clear();
  const uint64_t ns = uint64_t(probe_latency_sigs(kernel));
  if (!ns) return set_err(EDV_E_ARG, "latency phase-1 probe: unknown kernel");
  if (set != EDV_TABLE_SET_COMPACT && set != EDV_TABLE_SET_LARGE)
    return set_err(EDV_E_ARG, "latency phase-1 probe: unknown table set");
  if (n > EDV_STAGE_CAP) return set_err(EDV_E_ARG, "latency phase-1 probe: at most EDV_STAGE_CAP requests");
  if (n == 0) return 0;
  if (!sigs || !pks || !msg_off || !dig || !pt || !ok || !accept)
    return set_err(EDV_E_ARG, "latency phase-1 probe: null buffer");
  for (uint64_t i = 0; i < n; i++)
    if (msg_off[i + 1] < msg_off[i]) return set_err(EDV_E_ARG, "latency phase-1 probe: msg_off not non-decreasing");
  const uint64_t mbytes = msg_off[n];
  if (mbytes && !msgs) return set_err(EDV_E_ARG, "latency phase-1 probe: null buffer");
  if (mbytes > (uint64_t(1) << 30)) return set_err(EDV_E_ARG, "latency phase-1 probe: at most 1 GiB of messages");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  int err = 0;
  const SbShape sh = set == EDV_TABLE_SET_LARGE ? sb_large() : sb_compact();
  const int32_t* tables = shared_tables(c->phys, sh, c->stream, &err);  // this GPU's set, built on first use
  if (!tables) return err;
  const uint64_t slots = (n + ns - 1) / ns * ns;
  const uint64_t dig_b = slots * 17 * 4, pt_b = slots * 3 * 40 * 4, ok_b = slots * 3;
  StageBuf dsigs, dpks, dmsgs, doff, dacc, ddig, dpt, dok;
  if (dsigs.ensure(64 * n) || dpks.ensure(32 * n) || dmsgs.ensure(mbytes + 64) || doff.ensure(8 * (n + 1)) ||
      dacc.ensure(n) || ddig.ensure(dig_b) || dpt.ensure(pt_b) || dok.ensure(ok_b))
    return EDV_E_OOM;
  hipStream_t s = c->stream;
  HIPOK(hipMemcpyAsync(dsigs.p, sigs, 64 * n, hipMemcpyHostToDevice, s), "latency probe copy in");
  HIPOK(hipMemcpyAsync(dpks.p, pks, 32 * n, hipMemcpyHostToDevice, s), "latency probe copy in");
  HIPOK(hipMemsetAsync(dmsgs.p, 0, mbytes + 64, s), "latency probe memset");  // whole words are read past a message's end
  if (mbytes) HIPOK(hipMemcpyAsync(dmsgs.p, msgs, mbytes, hipMemcpyHostToDevice, s), "latency probe copy in");
  HIPOK(hipMemcpyAsync(doff.p, msg_off, 8 * (n + 1), hipMemcpyHostToDevice, s), "latency probe copy in");
  HIPOK(hipMemsetAsync(dacc.p, EDV_STAGE_SENTINEL, n, s), "latency probe memset");
  HIPOK(hipMemsetAsync(ddig.p, EDV_STAGE_SENTINEL, dig_b, s), "latency probe memset");
  HIPOK(hipMemsetAsync(dpt.p, EDV_STAGE_SENTINEL, pt_b, s), "latency probe memset");
  HIPOK(hipMemsetAsync(dok.p, EDV_STAGE_SENTINEL, ok_b, s), "latency probe memset");
  VerifyArgs va;
  memset(&va, 0, sizeof va);
  va.sigs = static_cast<const uint32_t*>(dsigs.p);
  va.pks = static_cast<const uint32_t*>(dpks.p);
  va.msgs = static_cast<const uint8_t*>(dmsgs.p);
  va.off = static_cast<const uint64_t*>(doff.p);
  va.n = n;
  va.accept = static_cast<uint8_t*>(dacc.p);
  va.btab = tables;
  va.sb = sh;
  HIPOK(launch_probe_latency_phase1(s, kernel, va, static_cast<uint32_t*>(ddig.p), static_cast<int32_t*>(dpt.p),
                                    static_cast<uint8_t*>(dok.p)),
        "latency phase-1 probe launch");
  HIPOK(hipMemcpyAsync(dig, ddig.p, dig_b, hipMemcpyDeviceToHost, s), "latency probe copy out");
  HIPOK(hipMemcpyAsync(pt, dpt.p, pt_b, hipMemcpyDeviceToHost, s), "latency probe copy out");
  HIPOK(hipMemcpyAsync(ok, dok.p, ok_b, hipMemcpyDeviceToHost, s), "latency probe copy out");
  HIPOK(hipMemcpyAsync(accept, dacc.p, n, hipMemcpyDeviceToHost, s), "latency probe copy out");
  HIPOK(hipStreamSynchronize(s), "latency probe sync");  // the buffers are freed on return
  return 0;
}

int edv_probe_latency_walk(int device, int kernel, uint64_t n, uint64_t slots, const uint32_t* dig, const int32_t* pt,
                           const uint8_t* ok, uint32_t flags, uint8_t* accept) {
  g_err.clear();
  const uint64_t ns = uint64_t(probe_latency_sigs(kernel));
  if (!ns) return set_err(EDV_E_ARG, "latency walk probe: unknown kernel");
  if (flags) return set_err(EDV_E_ARG, "latency walk probe: unknown flag");
  if (n > EDV_STAGE_CAP) return set_err(EDV_E_ARG, "latency walk probe: at most EDV_STAGE_CAP requests");
  if (n == 0) return 0;
  if (slots != (n + ns - 1) / ns * ns)
    return set_err(EDV_E_ARG, "latency walk probe: slots is n rounded up to the workgroup's 16 or 32");
  if (!dig || !pt || !ok || !accept) return set_err(EDV_E_ARG, "latency walk probe: null buffer");
  // the domain the walks are written for: a slot all three sides passed walks
  // at most kAWindows windows (the right-to-left kernel's waves meet through
  // counters that run to the window count: never driven outside it)
  for (uint64_t g = 0; g < slots / ns; g++)
    for (uint64_t j = 0; j < ns; j++)
      if (ok[(g * 3 + 0) * ns + j] && ok[(g * 3 + 1) * ns + j] && ok[(g * 3 + 2) * ns + j] &&
          (dig[(g * 17 + 16) * ns + j] & 0xff) > uint32_t(kAWindows))
        return set_err(EDV_E_ARG, "latency walk probe: window count above kAWindows");
  CtxLock cl(device);
  if (cl.err) return cl.err;
  DevCtx* c = cl.c;
  const uint64_t dig_b = slots * 17 * 4, pt_b = slots * 3 * 40 * 4, ok_b = slots * 3;
  StageBuf dacc, ddig, dpt, dok, dqtab;
  if (dacc.ensure(slots) || ddig.ensure(dig_b) || dpt.ensure(pt_b) || dok.ensure(ok_b)) return EDV_E_OOM;
  // the two-walk kernel's table scratch, as launch_quad sizes it (the last
  // workgroup's 64 quads all write their tables, in range or not)
  if (kernel == EDV_LAT_QUAD && dqtab.ensure((n + 63) / 64 * 64 * kQSigWords * 4)) return EDV_E_OOM;
  hipStream_t s = c->stream;
  HIPOK(hipMemcpyAsync(ddig.p, dig, dig_b, hipMemcpyHostToDevice, s), "latency probe copy in");
  HIPOK(hipMemcpyAsync(dpt.p, pt, pt_b, hipMemcpyHostToDevice, s), "latency probe copy in");
  HIPOK(hipMemcpyAsync(dok.p, ok, ok_b, hipMemcpyHostToDevice, s), "latency probe copy in");
  HIPOK(hipMemsetAsync(dacc.p, EDV_STAGE_SENTINEL, slots, s), "latency probe memset");
  VerifyArgs va;
  memset(&va, 0, sizeof va);
  va.n = n;
  va.accept = static_cast<uint8_t*>(dacc.p);
  HIPOK(launch_probe_latency_walk(s, kernel, va, static_cast<int32_t*>(dqtab.p), static_cast<const uint32_t*>(ddig.p),
                                  static_cast<const int32_t*>(dpt.p), static_cast<const uint8_t*>(dok.p)),
        "latency walk probe launch");
  HIPOK(hipMemcpyAsync(accept, dacc.p, slots, hipMemcpyDeviceToHost, s), "latency probe copy out");
  HIPOK(hipStreamSynchronize(s), "latency probe sync");  // the buffers are freed on return
  return 0;
}

}  // extern "C"
