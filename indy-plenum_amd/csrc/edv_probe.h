// edv_probe.h -- launch wrappers of the math probe kernels (edv_probe.hip,
// edv_probe_quad.hip: libedv_measure.so only), for edv_measure.inc.  Device
// buffers, strides in bytes (multiples of 4, at least probe_size(op)); each
// launches on stream s and returns hipGetLastError(), hipErrorInvalidValue for
// an op that is not its kind.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "edv_probe_ops.h"

namespace edv {

hipError_t launch_probe_lane(hipStream_t s, int op, const uint8_t* in, uint64_t in_stride, uint8_t* out,
                             uint64_t out_stride, uint64_t n);
hipError_t launch_probe_quad(hipStream_t s, int op, const uint8_t* in, uint64_t in_stride, uint8_t* out,
                             uint64_t out_stride, uint64_t n);

}  // namespace edv
