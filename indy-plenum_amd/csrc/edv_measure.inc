// edv_measure.inc -- the measurement entry points of libedv_measure.so
// (include/edv_measure.h): kernel timing on the kernels' own stream, the
// Infinity-Cache flush probe, the prep kernel's sides timed apart, the
// asynchronous path's fault hook and the device math probes.  Included at the end of edv_runtime.hip only
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
  HIPOK(hipMemcpyAsync(din.p, in, n * in_stride, hipMemcpyHostToDevice, c->stream), "probe copy in");
  HIPOK(hipMemsetAsync(dout.p, 0, n * out_stride, c->stream), "probe memset");
  HIPOK((probe_is_quad(op) ? launch_probe_quad : launch_probe_lane)(c->stream, op, static_cast<const uint8_t*>(din.p),
                                                                    in_stride, static_cast<uint8_t*>(dout.p),
                                                                    out_stride, n),
        "probe launch");
  HIPOK(hipMemcpyAsync(out, dout.p, n * out_stride, hipMemcpyDeviceToHost, c->stream), "probe copy out");
  HIPOK(hipStreamSynchronize(c->stream), "probe sync");  // the buffers are freed on return
  return 0;
}

}  // extern "C"
