"""The math-probe cases and their Python-integer checkers (math_cases.py), run
through the CPU build of the headers (libedv_hostcheck.so, hc_probe_math):
proves the generators, packing and references here, before the same families
run on the device build (test_gpu_math_device.py).  The quad arithmetic has no
CPU build: its references are checked by consistency with the affine group law,
the oracle's fixed-base multiplication and the host build's plain ge_add /
ge_p2_dbl, its lane-level mirror against the references, and its limb bounds by
interval arithmetic."""
import ctypes
import random
from fractions import Fraction

import numpy as np

import hostcheck_lib
import math_cases as mc
import probe_lib as pl
from math_cases import P


def base_points(n=24, seed=77):
    import oracle_lib as orc
    r = random.Random(seed)
    ks = [1, 2, 3, mc.L - 1, 2**252 - 1] + [r.randrange(1, mc.L) for _ in range(n - 5)]
    return [orc.scalarmult_base(k.to_bytes(32, "little")) for k in ks]


def test_fe_mul_sq():
    mc.family_fe_mul_sq(pl.host)


def test_fe_sq_floor():
    mc.family_fe_sq_floor(pl.host)


def test_fe_bytes():
    mc.family_fe_bytes(pl.host)


def test_fe_invert_pow():
    mc.family_fe_invert_pow(pl.host)


def test_sc_reduce():
    mc.family_sc_reduce(pl.host)


def test_half_scalars():
    mc.family_half_scalars(pl.host)


def test_recode():
    mc.family_recode(pl.host)


def test_approx_div():
    """the host build divides exactly: half an ulp"""
    assert mc.family_approx_div(pl.host) <= Fraction(1, 2**53)


def test_fdiv_floor():
    assert mc.family_fdiv_floor(pl.host) >= 52


def test_euclid_div():
    mc.family_euclid_div(pl.host)


def test_ge_frombytes():
    mc.family_ge_frombytes(pl.host, base_points())


def test_sc_muladd():
    assert mc.family_sc_muladd(pl.host) == 3361


def test_recode8():
    assert mc.family_recode8(pl.host) == 2082


def test_scalarmult_base():
    """the CPU build walks HostComb, the table hc_comb_entries reads back"""
    assert mc.family_scalarmult_base(pl.host) == 563


def test_ge_p3_tobytes():
    assert mc.family_ge_p3_tobytes(pl.host, base_points()) == 32 * 8


def test_single_case_wrappers_agree_with_the_packed_probe():
    """hc_approx_div, hc_fdiv_floor, hc_euclid_div, hc_recode5_windows and
    hc_ge_frombytes_negate_limbs are the packed ops' functions"""
    hc = hostcheck_lib.load()
    hc.hc_approx_div.restype = hc.hc_fdiv_floor.restype = ctypes.c_double
    hc.hc_approx_div.argtypes = hc.hc_fdiv_floor.argtypes = [ctypes.c_double, ctypes.c_double]
    hc.hc_euclid_div.argtypes = [ctypes.c_void_p] * 4
    hc.hc_recode5_windows.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    hc.hc_ge_frombytes_negate_limbs.argtypes = [ctypes.c_char_p, ctypes.c_void_p]
    assert hc.hc_approx_div(7.0, 2.0) == 3.5 and hc.hc_fdiv_floor(7.0, 2.0) == 3.0
    cases = mc.euclid_div_cases()[::97]
    want = pl.host("euclid_div", pl.pack_ints(cases, 32))
    for c, w in zip(cases, want):
        bufs = [np.frombuffer(int(v).to_bytes(32, "little"), np.uint32).copy() for v in c]
        hc.hc_euclid_div(*(b.ctypes.data for b in bufs))
        assert bufs[0].tobytes() + bufs[1].tobytes() == w.tobytes()
    vals = mc.recode5_values()[::41]
    want = pl.host("recode5", pl.pack_ints([[v] for v in vals], 32))
    for v, w in zip(vals, want):
        out = np.zeros(8, np.uint32)
        n = hc.hc_recode5_windows(v.to_bytes(32, "little"), out.ctypes.data)
        assert out.tobytes() == w[:32].tobytes() and n == int(w[32:].view(np.uint32)[0])
    enc = mc.ge_frombytes_encodings(base_points(8))[::7]
    want = pl.host("ge_frombytes", np.array([list(b) for b in enc], np.uint8))
    for b, w in zip(enc, want):
        out = np.zeros(40, np.int32)
        fl = hc.hc_ge_frombytes_negate_limbs(b, out.ctypes.data)
        assert [fl & 1, (fl >> 1) & 1, fl >> 2] == w[:12].view(np.int32).tolist()
        if fl >> 2:
            assert out.tobytes() == w[12:].tobytes()


# ---- the quad references (no CPU build of the quad arithmetic itself)
def _host_group(fn, *pts):
    hc = hostcheck_lib.load()
    out = np.zeros(40, np.int32)
    args = [np.array([w for f in p for w in f], np.int32) for p in pts]
    getattr(hc, fn)(*[ctypes.c_void_p(a.ctypes.data) for a in args], ctypes.c_void_p(out.ctypes.data))
    return [mc.val(out[10 * k:10 * k + 10].tolist()) % P for k in range(4)]


def test_quad_references_against_the_group_law_and_the_host_build():
    """ref_quad_add(p, ref_quad_cached(q)) and ref_quad_dbl(p): coordinate by
    coordinate the host build's ge_add / ge_p2_dbl (on arbitrary reduced field
    elements too: the same polynomials), the affine group law on curve points,
    and k B + B = (k + 1) B by the oracle's scalarmult_base."""
    import oracle_lib as orc
    r = random.Random(81)
    pool, pairs = mc.quad_point_cases(base_points())
    for a, b in pairs[::5]:
        ea, eb = mc.extended(r, a), mc.extended(r, b)
        got = mc.ref_quad_add(mc._vals(ea), mc.ref_quad_cached(mc._vals(eb)))
        assert got == _host_group("hc_ge_add_p3", ea, eb)
        zi = pow(got[2], P - 2, P)
        assert (got[0] * zi % P, got[1] * zi % P) == mc.ed_add(a, b) and got[3] * got[2] % P == got[0] * got[1] % P
        neg = mc.ref_quad_add(mc._vals(ea), mc.ref_quad_cached(mc._vals(eb), -1))
        zi = pow(neg[2], P - 2, P)
        assert (neg[0] * zi % P, neg[1] * zi % P) == mc.ed_add(a, ((P - b[0]) % P, b[1]))
    for a in pool:
        ea = mc.extended(r, a, rand_t=True)
        got = mc.ref_quad_dbl(mc._vals(ea))
        assert got == _host_group("hc_ge_dbl_p3", ea)
        zi = pow(got[2], P - 2, P)
        assert (got[0] * zi % P, got[1] * zi % P) == mc.ed_add(a, a) and got[3] * got[2] % P == got[0] * got[1] % P
    for c in mc.quad_limb_cases(8, 300):                     # arbitrary field elements
        assert mc.ref_quad_add(mc._vals(c[:4]), mc.ref_quad_cached(mc._vals(c[4:]))) == \
            _host_group("hc_ge_add_p3", c[:4], c[4:])
        assert mc.ref_quad_dbl(mc._vals(c[:4])) == _host_group("hc_ge_dbl_p3", c[:4])
    Bp = mc.ed_decode(orc.scalarmult_base((1).to_bytes(32, "little")))
    for k in (1, 2, 7, 2**200 + 5, mc.L - 2):
        kb = mc.ed_decode(orc.scalarmult_base(k.to_bytes(32, "little")))
        got = mc.ref_quad_add(mc._vals(mc.extended(r, kb)), mc.ref_quad_cached(mc._vals(mc.extended(r, Bp))))
        zi = pow(got[2], P - 2, P)
        assert mc.ed_encode((got[0] * zi % P, got[1] * zi % P)) == orc.scalarmult_base((k + 1).to_bytes(32, "little"))


def test_quad_lane_mirror_matches_the_references():
    """the lanes' data movement as written (quad_perm indices, masks, shifts),
    mirrored in Python, computes the reference polynomials"""
    for c in mc.quad_limb_cases(8, 400):
        p, e = mc._vals(c[:4]), mc._vals(c[4:])
        assert [x % P for x in mc.mirror_quad_add(p, e)] == mc.ref_quad_add(p, e)
        assert [x % P for x in mc.mirror_quad_dbl(p)] == mc.ref_quad_dbl(p)


def test_quad_stage_operands_stay_inside_the_multiply_bound():
    """Interval arithmetic: with every input limb at the reduced bound, each
    operand that stages A and B of quad_dbl and quad_add hand to fe_mul /
    fe_sq_cols stays inside BOUND, the bound test_fe_mul_sq_against_python and
    family_fe_mul_sq prove the products for (lane 2 of quad_add's stage B adds
    the doubled product to an undoubled one: 3 x RED, the largest)."""
    seen = mc.quad_bounds()
    assert set(seen) == {"add stage A lhs", "add stage A rhs", "add stage B lhs", "add stage B rhs",
                         "dbl stage A", "dbl stage B lhs", "dbl stage B rhs"}
    assert all(v <= 1.0 for v in seen.values()), seen
    # the sums are what the derivation in math_cases says: 2 x RED into stage A, 3 x RED into stage B
    three = max(3 * a / b for a, b in zip(mc.RED, mc.BOUND))
    assert seen["add stage B lhs"] == three and seen["add stage B rhs"] == three and seen["dbl stage B lhs"] == three
    assert seen["add stage A lhs"] == seen["dbl stage A"] == max(2 * a / b for a, b in zip(mc.RED, mc.BOUND))
