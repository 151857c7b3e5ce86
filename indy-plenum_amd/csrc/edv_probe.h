// edv_probe.h -- launch wrappers of the math probe kernels (edv_probe.hip,
// edv_probe_quad.hip: libedv_measure.so only), for edv_measure.inc.  Device
// buffers, strides in bytes (multiples of 4, at least probe_size(op)); each
// launches on stream s and returns hipGetLastError(), hipErrorInvalidValue for
// an op that is not its kind.  comb: the context's comb table (the batch
// signer's, edv_launch.h), read by EDV_PROBE_SCALARMULT_BASE only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edv_kernels.h"
#include "edv_probe_ops.h"

namespace edv {

hipError_t launch_probe_lane(hipStream_t s, int op, const uint8_t* in, uint64_t in_stride, uint8_t* out,
                             uint64_t out_stride, uint64_t n, const int32_t* comb);
hipError_t launch_probe_quad(hipStream_t s, int op, const uint8_t* in, uint64_t in_stride, uint8_t* out,
                             uint64_t out_stride, uint64_t n);

// The latency probes (edv_probe_latency.hip): the latency kernels cut at phase
// 1's barrier.  kernel: EDV_LAT_RTL or EDV_LAT_QUAD; the state arrays hold
// ceil(va.n / sigs) workgroups of sigs = probe_latency_sigs(kernel) slots
// (layout: edv_probe_latency.hip).  phase1 reads va as the product kernel
// does and writes the state; walk reads the state and va.n, va.base and
// va.accept only (qtab: the two-walk kernel's table scratch, as launch_quad
// sizes it).  hipErrorInvalidValue for an unknown kernel or va.n = 0.
int probe_latency_sigs(int kernel);  // 16, 32, or 0 for an unknown kernel
hipError_t launch_probe_latency_phase1(hipStream_t s, int kernel, const VerifyArgs& va, uint32_t* dig, int32_t* pt,
                                       uint8_t* ok);
hipError_t launch_probe_latency_walk(hipStream_t s, int kernel, const VerifyArgs& va, int32_t* qtab,
                                     const uint32_t* dig, const int32_t* pt, const uint8_t* ok);

}  // namespace edv
