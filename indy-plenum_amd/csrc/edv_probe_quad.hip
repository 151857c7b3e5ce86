// edv_probe_quad.hip -- TESTS ONLY, libedv_measure.so only: probes of the
// latency path's quad arithmetic (edv_quad_math.h), which has no CPU build.
// One quad (4 consecutive lanes, coordinate q on lane q) runs one case, so a
// wave holds 16 different cases side by side and a quad_perm that read a
// neighbouring quad would show.  Compiled as edv_quad.hip is (no scheduling
// fences).  Every lane of a launched wave computes (lanes past the last case
// repeat it and store nothing): the DPP moves never read an idle lane.
#define EDV_NO_SCHED_FENCE 1
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edv_probe.h"
#include "edv_quad_math.h"

namespace edv {
namespace {

template <int OP>
__global__ __launch_bounds__(256) void edv_probe_quad_kernel(const uint8_t* in, uint64_t in_stride, uint8_t* out,
                                                             uint64_t out_stride, uint64_t n) {
  const uint64_t t = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  const uint64_t c = t >> 2, i = c < n ? c : n - 1;  // n > 0 (the caller launches nothing otherwise)
  const QLane Q(int(threadIdx.x & 63));
  const uint32_t* x = reinterpret_cast<const uint32_t*>(in + i * in_stride);
  fe r;
  if constexpr (OP == EDV_PROBE_QUAD_SQ_SHIFT) {
    r = fe_sq_shift(probe_fe(x + 11 * Q.q), int32_t(x[11 * Q.q + 10]));
  } else if constexpr (OP == EDV_PROBE_QUAD_DBL) {
    r = quad_dbl(probe_fe(x + 10 * Q.q), Q);
  } else if constexpr (OP == EDV_PROBE_QUAD_ADD) {
    r = quad_add(probe_fe(x + 10 * Q.q), probe_fe(x + 40 + 10 * Q.q), Q);
  } else if constexpr (OP == EDV_PROBE_QUAD_CACHED) {
    r = quad_cached(probe_fe(x + 10 * Q.q), Q);
  } else {
    static_assert(OP == EDV_PROBE_QUAD_CACHED_SIGNED, "a quad probe op");
    r = quad_cached_signed(probe_fe(x + 10 * Q.q), int32_t(x[40]), Q);
  }
  if (c < n) probe_put(reinterpret_cast<uint32_t*>(out + c * out_stride) + 10 * Q.q, r);
}

}  // namespace

hipError_t launch_probe_quad(hipStream_t s, int op, const uint8_t* in, uint64_t in_stride, uint8_t* out,
                             uint64_t out_stride, uint64_t n) {
  const dim3 grid(unsigned((4 * n + 255) / 256)), block(256);
  switch (op) {
#define EDV_PROBE_CASE(OP) \
  case OP: edv_probe_quad_kernel<OP><<<grid, block, 0, s>>>(in, in_stride, out, out_stride, n); break;
    EDV_PROBE_CASE(EDV_PROBE_QUAD_SQ_SHIFT)
    EDV_PROBE_CASE(EDV_PROBE_QUAD_DBL)
    EDV_PROBE_CASE(EDV_PROBE_QUAD_ADD)
    EDV_PROBE_CASE(EDV_PROBE_QUAD_CACHED)
    EDV_PROBE_CASE(EDV_PROBE_QUAD_CACHED_SIGNED)
#undef EDV_PROBE_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace edv
