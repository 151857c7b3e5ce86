// edv_quad.hip -- the latency path: one kernel launch verifies a small batch
// (a Node's prod, a single Verifier.verify) with several lanes per signature:
// edv_rtl_kernel (sixteen lanes, no tables, at most 4,096 requests: below) and
// edv_quad_kernel (eight lanes, per-signature tables, up to 16,384 requests),
// described first.
//
// The batch path (edv_prep.hip, edv_verify.hip) runs one signature per lane:
// best for throughput, but a lane's serial chain -- two exponentiations, ~130
// doublings, ~70 additions, every field product one after the other -- sets
// the latency of any batch that leaves most of the chip idle (~0.55 ms of
// kernels for n <= 16k: one wave per SIMD at most).  Here a 256-thread
// workgroup takes 32 signatures:
//
//   phase 1  wave-specialised (uniform within a wave, so no divergence):
//              wave 0: V2-V4 byte checks, V6/V7 h = SHA-512(R || A || M) mod L,
//                      the half-size scalars (a, b) and their digits
//              wave 1: canonical / small-order checks, decompress -A
//              wave 2: the same for R
//              wave 3: [S]B from the shared tables (from identity)
//            results through LDS, then one barrier;
//   phase 2  per signature two quads (4 consecutive lanes each): quad 0 builds
//            the 0..8 x (-A) table, quad 1 computes Q = [S]B - R and builds
//            0..8 x Q, in global scratch;
//   phase 3  quad 0 walks [a](-A), quad 1 walks [b](+-Q) -- the batch path's
//            fixed signed 4-bit windows, split into the
//            two scalars' walks -- then [a](-A) == -[b](+-Q) projectively.
//
// Quad arithmetic.  A point is DISTRIBUTED: lane q of a quad holds coordinate
// q of (X : Y : Z : T).  The extended-coordinate formulas have four
// independent field products per stage, so each lane computes one: a doubling
// is two product latencies (X^2 | Y^2 | 2Z^2 | (X+Y)^2, then X1 T1 | Y1 Z1 |
// Z1 T1 | X1 Y1) instead of seven, an addition two instead of eight.  The
// operands a lane needs are gathered from its quad with DPP quad_perm moves
// (v_mov_b32_dpp / DPP-modified VOP2 adds: the exchange costs a few VOP2 per
// limb, no LDS); per-lane signs and selects are mask arithmetic and v_bfi_b32
// (no VCC-mask v_cndmask_b32, ~23 cycles on gfx950).  A table entry is read
// one coordinate per lane (48-byte slots): the digit's sign picks which slot
// (YpX <-> YmX) and negates T2d, so no data is selected after the load.
//
// Same verdicts as the batch path (same strictness checks, same lattice
// scalars, same windows), checked against libsodium's golden and corpus
// verdicts by the GPU tests; the field arithmetic is edv_math.h's.
#define EDV_NO_SCHED_FENCE 1
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edv_kernels.h"
#include "edv_launch.h"
#include "edv_quad_body.h"

namespace edv {
namespace {

// the LDS layouts, phase1 and the walks (rtl_body = phase1; barrier; rtl_walk,
// quad_body = phase1; barrier; quad_walk): edv_quad_body.h

__global__ __launch_bounds__(256) void edv_rtl_kernel(VerifyArgs a) {
  __shared__ RtlLds lds;
  rtl_body<kBBits>(a, lds);
}
__global__ __launch_bounds__(256) void edv_rtl_kernel_compact(VerifyArgs a) {
  __shared__ RtlLds lds;
  rtl_body<kBBitsCompact>(a, lds);
}

__global__ __launch_bounds__(256) void edv_quad_kernel(VerifyArgs a, int32_t* qtab) {
  __shared__ QuadLds lds;
  quad_body<kBBits>(a, qtab, lds);
}
__global__ __launch_bounds__(256) void edv_quad_kernel_compact(VerifyArgs a, int32_t* qtab) {
  __shared__ QuadLds lds;
  quad_body<kBBitsCompact>(a, qtab, lds);
}

}  // namespace

hipError_t launch_rtl_kernel(hipStream_t s, const VerifyArgs& va) {
  const unsigned blocks = unsigned((va.n + kRSigs - 1) / kRSigs);
  if (va.sb.bits == kBBits) edv_rtl_kernel<<<dim3(blocks), dim3(256), 0, s>>>(va);
  else edv_rtl_kernel_compact<<<dim3(blocks), dim3(256), 0, s>>>(va);
  return hipGetLastError();
}

hipError_t launch_quad_kernel(hipStream_t s, const VerifyArgs& va, int32_t* qtab) {
  const unsigned blocks = unsigned((va.n + kQSigs - 1) / kQSigs);
  if (va.sb.bits == kBBits) edv_quad_kernel<<<dim3(blocks), dim3(256), 0, s>>>(va, qtab);
  else edv_quad_kernel_compact<<<dim3(blocks), dim3(256), 0, s>>>(va, qtab);
  return hipGetLastError();
}

}  // namespace edv
