// edv_probe.hip -- TESTS ONLY, libedv_measure.so only: the one-lane math
// probes (include/edv_measure.h edv_probe_math).  One lane runs one case of
// edv_probe_ops.h's probe_lane_op, which calls the header function unchanged;
// compiled like the batch path's main kernel (edv_verify.hip), with the field
// arithmetic's scheduling fences.  Straight-line code and loops with fixed
// bounds only.  fe_sq_floor's chained columns are on, as in the prep kernel,
// the one that runs them: the unchained form is what the latency probes
// (edv_probe_latency.hip) and every verdict test of that path cover.
#define EDV_CHAIN_FLOOR 1
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edv_probe.h"

namespace edv {
namespace {

template <int OP>
__global__ __launch_bounds__(256) void edv_probe_lane_kernel(const uint8_t* in, uint64_t in_stride, uint8_t* out,
                                                             uint64_t out_stride, uint64_t n) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  probe_lane_op<OP>(reinterpret_cast<const uint32_t*>(in + i * in_stride),
                    reinterpret_cast<uint32_t*>(out + i * out_stride));
}

// EDV_PROBE_SCALARMULT_BASE: the walk reads the comb table as the sign kernel does
__global__ __launch_bounds__(256) void edv_probe_comb_kernel(const uint8_t* in, uint64_t in_stride, uint8_t* out,
                                                             uint64_t out_stride, uint64_t n, const int32_t* comb) {
  const uint64_t i = uint64_t(blockIdx.x) * 256 + threadIdx.x;
  if (i >= n) return;
  probe_scalarmult_base(reinterpret_cast<const uint32_t*>(in + i * in_stride),
                        reinterpret_cast<uint32_t*>(out + i * out_stride), GlobalComb{comb});
}

}  // namespace

hipError_t launch_probe_lane(hipStream_t s, int op, const uint8_t* in, uint64_t in_stride, uint8_t* out,
                             uint64_t out_stride, uint64_t n, const int32_t* comb) {
  const dim3 grid(unsigned((n + 255) / 256)), block(256);
  switch (op) {
    case EDV_PROBE_SCALARMULT_BASE:
      if (!comb) return hipErrorInvalidValue;
      edv_probe_comb_kernel<<<grid, block, 0, s>>>(in, in_stride, out, out_stride, n, comb);
      break;
#define EDV_PROBE_CASE(OP) \
  case OP: edv_probe_lane_kernel<OP><<<grid, block, 0, s>>>(in, in_stride, out, out_stride, n); break;
    EDV_PROBE_CASE(EDV_PROBE_FE_MUL)
    EDV_PROBE_CASE(EDV_PROBE_FE_SQ)
    EDV_PROBE_CASE(EDV_PROBE_FE_SQ2)
    EDV_PROBE_CASE(EDV_PROBE_FE_SQ_FLOOR)
    EDV_PROBE_CASE(EDV_PROBE_FE_TOBYTES)
    EDV_PROBE_CASE(EDV_PROBE_FE_FROMBYTES)
    EDV_PROBE_CASE(EDV_PROBE_FE_INVERT_SAFEGCD)
    EDV_PROBE_CASE(EDV_PROBE_FE_POW22523)
    EDV_PROBE_CASE(EDV_PROBE_SC_REDUCE)
    EDV_PROBE_CASE(EDV_PROBE_HALF_SCALARS)
    EDV_PROBE_CASE(EDV_PROBE_RECODE5)
    EDV_PROBE_CASE(EDV_PROBE_APPROX_DIV)
    EDV_PROBE_CASE(EDV_PROBE_FDIV_FLOOR)
    EDV_PROBE_CASE(EDV_PROBE_EUCLID_DIV)
    EDV_PROBE_CASE(EDV_PROBE_GE_FROMBYTES)
    EDV_PROBE_CASE(EDV_PROBE_SC_MULADD)
    EDV_PROBE_CASE(EDV_PROBE_RECODE8)
    EDV_PROBE_CASE(EDV_PROBE_GE_P3_TOBYTES)
#undef EDV_PROBE_CASE
    default: return hipErrorInvalidValue;
  }
  return hipGetLastError();
}

}  // namespace edv
