// edv_probe_latency.hip -- TESTS ONLY, libedv_measure.so only: the latency
// path's kernels (edv_quad.hip) cut at phase 1's barrier.  The phase-1 probe
// runs phase1<BITS, NS> exactly as the product kernel does and, after the
// barrier, copies the workgroup's L.dig, L.pt and L.ok to global memory; the
// walk probe fills the same LDS fields from global memory, executes the
// barrier and runs rtl_walk / quad_walk unchanged.  These kernels INSTANTIATE
// the header functions the product's kernels are made of (edv_quad_body.h);
// unlike the prep and main stage probes they are not the product's own kernel
// objects.  Compiled as edv_quad.hip is (no scheduling fences).
//
// Global layout of a state of G workgroups of NS slots (NS = 16 for the
// right-to-left kernel, 32 for the two-walk kernel), as the LDS arrays:
//   dig[(g * 17 + w) * NS + j]          word w of slot j of workgroup g
//   pt[((g * 3 + k) * 40 + w) * NS + j]  point k (0: -A, 1: -R, 2: [S]B), X | Y | Z | T
//   ok[(g * 3 + k) * NS + j]            side k (0 hash, 1 A, 2 R)
#define EDV_NO_SCHED_FENCE 1
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edv_probe.h"
#include "edv_quad_body.h"

namespace edv {
namespace {

static_assert(kQDigWords == 17 && kQPtWords == 40, "the probes' documented layout (include/edv_measure.h)");

template <int NS, class Lds>
__device__ __forceinline__ void state_out(const Lds& L, uint32_t* dig, int32_t* pt, uint8_t* ok) {
  const uint64_t g = blockIdx.x;
  for (int t = int(threadIdx.x); t < kQDigWords * NS; t += 256) dig[g * (kQDigWords * NS) + t] = L.dig[t / NS][t % NS];
  for (int t = int(threadIdx.x); t < 3 * kQPtWords * NS; t += 256)
    pt[g * (3 * kQPtWords * NS) + t] = L.pt[t / (kQPtWords * NS)][(t / NS) % kQPtWords][t % NS];
  for (int t = int(threadIdx.x); t < 3 * NS; t += 256) ok[g * (3 * NS) + t] = L.ok[t / NS][t % NS];
}
template <int NS, class Lds>
__device__ __forceinline__ void state_in(Lds& L, const uint32_t* dig, const int32_t* pt, const uint8_t* ok) {
  const uint64_t g = blockIdx.x;
  for (int t = int(threadIdx.x); t < kQDigWords * NS; t += 256) L.dig[t / NS][t % NS] = dig[g * (kQDigWords * NS) + t];
  for (int t = int(threadIdx.x); t < 3 * kQPtWords * NS; t += 256)
    L.pt[t / (kQPtWords * NS)][(t / NS) % kQPtWords][t % NS] = pt[g * (3 * kQPtWords * NS) + t];
  for (int t = int(threadIdx.x); t < 3 * NS; t += 256) L.ok[t / NS][t % NS] = ok[g * (3 * NS) + t];
}

// phase 1 as rtl_body / quad_body run it, then the LDS state out
template <int BITS, int NS, class Lds>
__global__ __launch_bounds__(256) void edv_probe_latency_phase1_kernel(VerifyArgs a, uint32_t* dig, int32_t* pt,
                                                                       uint8_t* ok) {
  __shared__ Lds lds;
  const int tid = int(threadIdx.x), wave = tid >> 6, lane = tid & 63;
  const uint64_t g0 = uint64_t(blockIdx.x) * NS;
  phase1<BITS, NS>(a, lds, g0, wave, lane);
  __syncthreads();
  state_out<NS>(lds, dig, pt, ok);
}

// the caller's state in, the barrier, then the product's walk
__global__ __launch_bounds__(256) void edv_probe_rtl_walk_kernel(VerifyArgs a, const uint32_t* dig, const int32_t* pt,
                                                                 const uint8_t* ok) {
  __shared__ RtlLds lds;
  state_in<kRSigs>(lds, dig, pt, ok);
  __syncthreads();
  rtl_walk<kBBitsCompact>(a, lds, int(threadIdx.x) & 63);  // the walk uses nothing of BITS
}
__global__ __launch_bounds__(256) void edv_probe_quad_walk_kernel(VerifyArgs a, int32_t* qtab, const uint32_t* dig,
                                                                  const int32_t* pt, const uint8_t* ok) {
  __shared__ QuadLds lds;
  state_in<kQSigs>(lds, dig, pt, ok);
  __syncthreads();
  quad_walk(a, qtab, lds);
}

}  // namespace

int probe_latency_sigs(int kernel) { return kernel == EDV_LAT_RTL ? kRSigs : kernel == EDV_LAT_QUAD ? kQSigs : 0; }

hipError_t launch_probe_latency_phase1(hipStream_t s, int kernel, const VerifyArgs& va, uint32_t* dig, int32_t* pt,
                                       uint8_t* ok) {
  const int ns = probe_latency_sigs(kernel);
  if (!ns || va.n == 0) return hipErrorInvalidValue;
  const dim3 grid(unsigned((va.n + ns - 1) / ns)), block(256);
  const bool large = va.sb.bits == kBBits;
  if (kernel == EDV_LAT_RTL) {
    if (large) edv_probe_latency_phase1_kernel<kBBits, kRSigs, RtlLds><<<grid, block, 0, s>>>(va, dig, pt, ok);
    else edv_probe_latency_phase1_kernel<kBBitsCompact, kRSigs, RtlLds><<<grid, block, 0, s>>>(va, dig, pt, ok);
  } else {
    if (large) edv_probe_latency_phase1_kernel<kBBits, kQSigs, QuadLds><<<grid, block, 0, s>>>(va, dig, pt, ok);
    else edv_probe_latency_phase1_kernel<kBBitsCompact, kQSigs, QuadLds><<<grid, block, 0, s>>>(va, dig, pt, ok);
  }
  return hipGetLastError();
}

hipError_t launch_probe_latency_walk(hipStream_t s, int kernel, const VerifyArgs& va, int32_t* qtab,
                                     const uint32_t* dig, const int32_t* pt, const uint8_t* ok) {
  const int ns = probe_latency_sigs(kernel);
  if (!ns || va.n == 0 || (kernel == EDV_LAT_QUAD && !qtab)) return hipErrorInvalidValue;
  const dim3 grid(unsigned((va.n + ns - 1) / ns)), block(256);
  if (kernel == EDV_LAT_RTL) edv_probe_rtl_walk_kernel<<<grid, block, 0, s>>>(va, dig, pt, ok);
  else edv_probe_quad_walk_kernel<<<grid, block, 0, s>>>(va, qtab, dig, pt, ok);
  return hipGetLastError();
}

}  // namespace edv
