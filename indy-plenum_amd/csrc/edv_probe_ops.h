// edv_probe_ops.h -- TESTS ONLY: the one-lane math probes of
// include/edv_measure.h (edv_probe_math), each a header function of
// edv_math.h / edv_verify_core.h called unchanged on one packed case.
// __host__ __device__, so the probe kernels (edv_probe.hip, measurement build)
// and the CPU harness (edv_hostcheck.cpp, hc_probe_math) unpack and pack a
// case with the same code and the tests drive both through one layout.
#pragma once
#include "edv_verify_core.h"
#include "../../include/edv_measure.h"

namespace edv {

struct ProbeSize {
  uint32_t in, out;  // bytes per case; 0 / 0: no such op
};
EDV_HD constexpr ProbeSize probe_size(int op) {
  switch (op) {
    case EDV_PROBE_FE_MUL: return ProbeSize{80, 40};
    case EDV_PROBE_FE_SQ:
    case EDV_PROBE_FE_SQ2:
    case EDV_PROBE_FE_SQ_FLOOR:
    case EDV_PROBE_FE_INVERT_SAFEGCD:
    case EDV_PROBE_FE_POW22523: return ProbeSize{40, 40};
    case EDV_PROBE_FE_TOBYTES: return ProbeSize{40, 32};
    case EDV_PROBE_FE_FROMBYTES: return ProbeSize{32, 40};
    case EDV_PROBE_SC_REDUCE: return ProbeSize{64, 32};
    case EDV_PROBE_HALF_SCALARS: return ProbeSize{32, 68};
    case EDV_PROBE_RECODE5: return ProbeSize{32, 36};
    case EDV_PROBE_APPROX_DIV:
    case EDV_PROBE_FDIV_FLOOR: return ProbeSize{16, 8};
    case EDV_PROBE_EUCLID_DIV: return ProbeSize{128, 64};
    case EDV_PROBE_GE_FROMBYTES: return ProbeSize{32, 172};
    case EDV_PROBE_QUAD_SQ_SHIFT: return ProbeSize{176, 160};
    case EDV_PROBE_QUAD_DBL:
    case EDV_PROBE_QUAD_CACHED: return ProbeSize{160, 160};
    case EDV_PROBE_QUAD_ADD: return ProbeSize{320, 160};
    case EDV_PROBE_QUAD_CACHED_SIGNED: return ProbeSize{164, 160};
    case EDV_PROBE_SC_MULADD: return ProbeSize{96, 32};
    case EDV_PROBE_RECODE8: return ProbeSize{32, 32};
    case EDV_PROBE_SCALARMULT_BASE: return ProbeSize{32, 192};
    case EDV_PROBE_GE_P3_TOBYTES: return ProbeSize{160, 32};
    default: return ProbeSize{0, 0};
  }
}
EDV_HD constexpr bool probe_is_quad(int op) { return op >= EDV_PROBE_QUAD_SQ_SHIFT && op <= EDV_PROBE_QUAD_CACHED_SIGNED; }

EDV_HD fe probe_fe(const uint32_t* x) {
  fe f;
#pragma unroll
  for (int i = 0; i < 10; i++) f.v[i] = int32_t(x[i]);
  return f;
}
EDV_HD void probe_put(uint32_t* y, const fe& f) {
#pragma unroll
  for (int i = 0; i < 10; i++) y[i] = uint32_t(f.v[i]);
}
EDV_HD ge_p3 probe_p3(const uint32_t* x) { return ge_p3{probe_fe(x), probe_fe(x + 10), probe_fe(x + 20), probe_fe(x + 30)}; }
EDV_HD void probe_put_p3(uint32_t* y, const ge_p3& p) {
  probe_put(y, p.X);
  probe_put(y + 10, p.Y);
  probe_put(y + 20, p.Z);
  probe_put(y + 30, p.T);
}
EDV_HD double probe_f64(const uint32_t* x) { return __builtin_bit_cast(double, pack64(x[0], x[1])); }
EDV_HD void probe_put_f64(uint32_t* y, double d) {
  const uint64_t b = __builtin_bit_cast(uint64_t, d);
  y[0] = uint32_t(b);
  y[1] = uint32_t(b >> 32);
}

// one case of a one-lane op: x = the packed input words, y = the output words
template <int OP>
EDV_HD void probe_lane_op(const uint32_t* x, uint32_t* y) {
  if constexpr (OP == EDV_PROBE_FE_MUL) {
    probe_put(y, fe_mul(probe_fe(x), probe_fe(x + 10)));
  } else if constexpr (OP == EDV_PROBE_FE_SQ) {
    probe_put(y, fe_sq(probe_fe(x)));
  } else if constexpr (OP == EDV_PROBE_FE_SQ2) {
    probe_put(y, fe_sq2(probe_fe(x)));
  } else if constexpr (OP == EDV_PROBE_FE_SQ_FLOOR) {
    probe_put(y, fe_sq_floor(probe_fe(x)));
  } else if constexpr (OP == EDV_PROBE_FE_TOBYTES) {
    uint32_t w[8];
    fe_tobytes(w, probe_fe(x));
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = w[i];
  } else if constexpr (OP == EDV_PROBE_FE_FROMBYTES) {
    uint32_t w[8];
#pragma unroll
    for (int i = 0; i < 8; i++) w[i] = x[i];
    probe_put(y, fe_frombytes(w));
  } else if constexpr (OP == EDV_PROBE_FE_INVERT_SAFEGCD) {
    probe_put(y, fe_invert_safegcd(probe_fe(x)));
  } else if constexpr (OP == EDV_PROBE_FE_POW22523) {
    probe_put(y, fe_pow22523(probe_fe(x)));
  } else if constexpr (OP == EDV_PROBE_SC_REDUCE) {
    uint32_t w[16], o[8];
#pragma unroll
    for (int i = 0; i < 16; i++) w[i] = x[i];
    sc_reduce(o, w);
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = o[i];
  } else if constexpr (OP == EDV_PROBE_HALF_SCALARS) {
    uint32_t h[8], a[8], u[8];
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = x[i];
    bool neg = false;
    half_scalars(h, a, u, neg);
#pragma unroll
    for (int i = 0; i < 8; i++) { y[i] = a[i]; y[8 + i] = u[i]; }
    y[16] = neg ? 1u : 0u;
  } else if constexpr (OP == EDV_PROBE_RECODE5) {
    uint32_t s[8], d[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = x[i];
    recode5(d, s);
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = d[i];
    y[8] = uint32_t(digits5_windows(d));
  } else if constexpr (OP == EDV_PROBE_APPROX_DIV) {
    probe_put_f64(y, approx_div(probe_f64(x), probe_f64(x + 2)));
  } else if constexpr (OP == EDV_PROBE_FDIV_FLOOR) {
    probe_put_f64(y, fdiv_floor(probe_f64(x), probe_f64(x + 2)));
  } else if constexpr (OP == EDV_PROBE_EUCLID_DIV) {
    uint32_t r0[8], t0[8], r1[8], t1[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { r0[i] = x[i]; t0[i] = x[8 + i]; r1[i] = x[16 + i]; t1[i] = x[24 + i]; }
    euclid_div(r0, t0, r1, t1);
#pragma unroll
    for (int i = 0; i < 8; i++) { y[i] = r0[i]; y[8 + i] = t0[i]; }
  } else if constexpr (OP == EDV_PROBE_GE_FROMBYTES) {
    uint32_t s[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = x[i];
    ge_p3 p;
    y[0] = ge_is_canonical(s) ? 1u : 0u;
    y[1] = has_small_order(s) ? 1u : 0u;
    y[2] = ge_frombytes_negate(p, s) ? 1u : 0u;
    probe_put_p3(y + 3, p);
  } else if constexpr (OP == EDV_PROBE_SC_MULADD) {
    uint32_t a[8], b[8], c[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; i++) { a[i] = x[i]; b[i] = x[8 + i]; c[i] = x[16 + i]; }
    sc_muladd(o, a, b, c);
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = o[i];
  } else if constexpr (OP == EDV_PROBE_RECODE8) {
    uint32_t s[8], d[8];
#pragma unroll
    for (int i = 0; i < 8; i++) s[i] = x[i];
    recode8(d, s);
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = d[i];
  } else {
    static_assert(OP == EDV_PROBE_GE_P3_TOBYTES, "a one-lane probe op");
    uint32_t w[8];
    ge_p3_tobytes(w, probe_p3(x));
#pragma unroll
    for (int i = 0; i < 8; i++) y[i] = w[i];
  }
}

// EDV_PROBE_SCALARMULT_BASE: the signer's comb walk over the caller's table
// view (GlobalComb on the device, HostComb on the CPU), the point as it comes
// out and its encoding
template <class CombTab>
EDV_HD void probe_scalarmult_base(const uint32_t* x, uint32_t* y, const CombTab& ct) {
  uint32_t k[8], w[8];
#pragma unroll
  for (int i = 0; i < 8; i++) k[i] = x[i];
  const ge_p3 p = scalarmult_base(k, ct);
  probe_put_p3(y, p);
  ge_p3_tobytes(w, p);
#pragma unroll
  for (int i = 0; i < 8; i++) y[40 + i] = w[i];
}

}  // namespace edv
