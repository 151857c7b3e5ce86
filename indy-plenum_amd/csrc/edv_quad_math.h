// edv_quad_math.h -- the quad arithmetic of the latency path (edv_quad.hip): a
// point DISTRIBUTED over four consecutive lanes, lane q of a quad holding
// coordinate q of (X : Y : Z : T), its operands gathered with DPP quad_perm
// moves.  Device only.  In a header of its own so the math probes of the
// measurement build (edv_probe_quad.hip) run the very code the latency kernels
// run; the including translation unit defines EDV_NO_SCHED_FENCE first, as
// edv_quad.hip does.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "edv_math.h"

namespace edv {
namespace {

// ------------------------------------------------------------ quad helpers
constexpr int qp(int a, int b, int c, int d) { return a | (b << 2) | (c << 4) | (d << 6); }
template <int C>
__device__ __forceinline__ int32_t dpp(int32_t x) {
  return __builtin_amdgcn_mov_dpp(x, C, 0xf, 0xf, true);
}
template <int C>
__device__ __forceinline__ fe fdpp(const fe& f) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = dpp<C>(f.v[i]);
  return r;
}
__device__ __forceinline__ fe fand(const fe& f, int32_t m) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = f.v[i] & m;
  return r;
}
// s = 0: f; s = -1: -f
__device__ __forceinline__ fe fcneg(const fe& f, int32_t s) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = (f.v[i] ^ s) - s;
  return r;
}
// m = -1: a; m = 0: b -- one v_bfi_b32 per limb (LLVM makes the AND / OR
// form two instructions: v_and_b32 + v_and_or_b32)
__device__ __forceinline__ int32_t bfi(int32_t m, int32_t a, int32_t b) {
  int32_t r;
  asm("v_bfi_b32 %0, %1, %2, %3" : "=v"(r) : "v"(m), "v"(a), "v"(b));
  return r;
}
__device__ __forceinline__ fe fsel(int32_t m, const fe& a, const fe& b) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = bfi(m, a.v[i], b.v[i]);
  return r;
}
__device__ __forceinline__ fe fshl(const fe& f, int32_t sh) {
  fe r;
#pragma unroll
  for (int i = 0; i < 10; i++) r.v[i] = f.v[i] << sh;
  return r;
}

// Per-lane constants of a quad (opaque, so LLVM keeps them as mask arithmetic)
struct QLane {
  int32_t q;           // lane within the quad
  int32_t m1, m2, m3;  // all ones on lane 1 / 2 / 3
  int32_t m01;         // all ones on lanes 0 and 1
  int32_t m13;         // all ones on lanes 1 and 3
  int32_t s1;          // -1 on lane 1
  int32_t s03, s02;    // -1 on lanes 0, 3 / lanes 0, 2
  int32_t sh2, sh3;    // 1 on lane 2 / lane 3 (shift amounts)
  __device__ explicit QLane(int lane) {
    q = lane & 3;
    m1 = opaque_i32(-int32_t(q == 1));
    m2 = opaque_i32(-int32_t(q == 2));
    m3 = opaque_i32(-int32_t(q == 3));
    m01 = opaque_i32(-int32_t(q < 2));
    m13 = opaque_i32(-int32_t(q & 1));
    s1 = m1;
    s03 = opaque_i32(-int32_t(q == 0 || q == 3));
    s02 = opaque_i32(-int32_t(q == 0 || q == 2));
    sh2 = opaque_i32(int32_t(q == 2));
    sh3 = opaque_i32(int32_t(q == 3));
  }
};

// f^2, doubled on lanes where sh = 1 (2 Z^2 for the doubling's lane 2): the
// unbiased columns are shifted before the rounding bias goes in, so the one
// biased carry chain reduces either (output bounds of fe_sq)
__device__ __forceinline__ fe fe_sq_shift(const fe& f, int32_t sh) {
  int64_t h[10];
  fe_sq_cols<false, false>(f, h);
#pragma unroll
  for (int k = 0; k < 10; k++) {
    // (h << sh) + bias in one v_lshl_add_u64 (its shift may be a VGPR, low 3 bits)
    int64_t r;
    asm("v_lshl_add_u64 %0, %1, %2, %3" : "=v"(r) : "v"(h[k]), "v"(sh), "v"(bias_reg(k)));
    h[k] = r;
  }
  return fe_carry64_biased(h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], h[8], h[9]);
}

// Doubling of a distributed point (dbl-2008-hwcd, a = -1), T ignored on
// input, all four of X3 Y3 Z3 T3 out.
__device__ __forceinline__ fe quad_dbl(const fe& p, const QLane& L) {
  // stage A: X^2 | Y^2 | 2 Z^2 | (X + Y)^2
  const fe y3 = fand(fdpp<qp(1, 1, 1, 1)>(p), L.m3);   // Y on lane 3
  const fe u = fe_add(fdpp<qp(0, 1, 2, 0)>(p), y3);     // X | Y | Z | X + Y
  const fe r = fe_sq_shift(u, L.sh2);
  // stage B: Y1 = YY + XX, Z1 = YY - XX, X1 = A - Y1, T1 = B - Z1
  const fe a0 = fdpp<qp(0, 0, 0, 0)>(r), a1 = fdpp<qp(1, 1, 1, 1)>(r);
  const fe S = fe_add(a1, a0), D = fe_sub(a1, a0);
  const fe X1 = fe_sub(fdpp<qp(3, 3, 3, 3)>(r), S);
  const fe T1 = fe_sub(fdpp<qp(2, 2, 2, 2)>(r), D);
  const fe uu = fsel(L.m1, S, fsel(L.m2, D, X1));  // X1 | Y1 | Z1 | X1
  const fe vv = fsel(L.m1, D, fsel(L.m3, S, T1));  // T1 | Z1 | T1 | Y1
  return fe_mul(uu, vv);                           // X3 | Y3 | Z3 | T3
}

// Addition of a distributed point and one cached-form coordinate per lane
// (e: YpX | YmX | T2d | Z of the addend, already negated if need be).
__device__ __forceinline__ fe quad_add(const fe& p, const fe& e, const QLane& L) {
  // stage A: A = (Y+X) YpX | B = (Y-X) YmX | C = T T2d | ZZ = Z Z'
  const fe x = fcneg(fand(fdpp<qp(0, 0, 0, 0)>(p), L.m01), L.s1);  // X | -X | 0 | 0
  const fe u = fe_add(fdpp<qp(1, 1, 3, 2)>(p), x);                   // Y+X | Y-X | T | Z
  const fe r = fshl(fe_mul(u, e), L.sh3);                            // A | B | C | D = 2 ZZ
  // stage B: X1 = A - B, Y1 = A + B, Z1 = D + C, T1 = D - C
  const fe uu = fe_add(fdpp<qp(0, 0, 3, 0)>(r), fcneg(fdpp<qp(1, 1, 2, 1)>(r), L.s03));  // X1 | Y1 | Z1 | X1
  const fe vv = fe_add(fdpp<qp(3, 3, 3, 0)>(r), fcneg(fdpp<qp(2, 2, 2, 1)>(r), L.s02));  // T1 | Z1 | T1 | Y1
  return fe_mul(uu, vv);                                                                  // X3 | Y3 | Z3 | T3
}

// Cached form of a distributed point, one coordinate per lane:
// YpX | YmX | T2d | Z (the table slot order, quad_add's e)
__device__ __forceinline__ fe quad_cached(const fe& p, const QLane& L) {
  const fe x = fcneg(fand(fdpp<qp(0, 0, 0, 0)>(p), L.m01), L.s1);
  const fe w = fe_add(fdpp<qp(1, 1, 3, 2)>(p), x);  // Y+X | Y-X | T | Z
  return fe_mul(w, fsel(L.m2, fe_d2(), fe_one()));  // x 1 | x 1 | x 2d | x 1
}

__device__ __forceinline__ fe quad_identity(const QLane& L) {
  fe f = fe_zero();
  f.v[0] = (L.q == 1 || L.q == 2) ? 1 : 0;  // X = 0 | Y = 1 | Z = 1 | T = 0
  return f;
}
// the cached form of +-P (YpX | YmX | T2d | Z): for -P, YpX and YmX trade
// places and T2d changes sign
__device__ __forceinline__ fe quad_cached_signed(const fe& p, int32_t neg, const QLane& L) {
  const fe c = quad_cached(p, L);
  const fe sw = fsel(neg & L.m01, fdpp<qp(1, 0, 2, 3)>(c), c);
  return fcneg(sw, neg & L.m2);
}

}  // namespace
}  // namespace edv
