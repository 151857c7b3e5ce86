"""Context lifecycle (include/edv.h: edv_set_table_policy, edv_table_state,
edv_self_test, edv_prepare, edv_trim, edv_release), the parts that need no GPU:
the header and the libraries' exports, argument checks made before any device
is touched, the table-set decision the runtime makes per batch (edv_tables.h,
through the CPU build libedv_hostcheck.so) and the known answers embedded in
the library for the self-test (edv_selftest_cases.h)."""
import ctypes
import itertools
import json
import os
import re
import subprocess

import numpy as np
import pytest

import golden_io
import oracle_lib as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "edv.h")
CSRC = os.path.join(ROOT, "indy-plenum_amd", "csrc")
NEW = ("edv_set_table_policy", "edv_table_state", "edv_self_test", "edv_prepare", "edv_trim", "edv_release")
NO_GPU = not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK))

AUTO, COMPACT, LARGE = 0, 1, 2          # EDV_TABLES_*
SET_NONE, SET_COMPACT, SET_LARGE = -1, 0, 1
# SelfTestRule (edv_selftest_cases.h)
RULE_NONE, RULE_SCALAR, RULE_SMALL_R, RULE_NONCANON_A, RULE_SMALL_A, RULE_OFFCURVE_A, RULE_EQUATION = 0, 2, 3, 4, 5, 6, 7


def _hostcheck():
    """libedv_hostcheck.so, rebuilt if a header it is made of is newer."""
    subprocess.check_call(["make", "-s", "-C", CSRC, "../libedv_hostcheck.so"])
    lib = ctypes.CDLL(os.path.join(ROOT, "indy-plenum_amd", "libedv_hostcheck.so"))
    lib.hc_choose_tables.argtypes = [ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                     ctypes.c_void_p]
    lib.hc_selftest_case.argtypes = [ctypes.c_int] + [ctypes.c_void_p] * 6
    lib.hc_verify_batch.argtypes = [ctypes.c_char_p] * 3 + [ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p]
    return lib


@pytest.fixture(scope="module")
def hc():
    return _hostcheck()


def _defines():
    src = open(HDR).read()
    return {k: int(v.rstrip("u")) for k, v in re.findall(r"^#define (EDV_\w+) (-?\d+u?)\s", src, re.M)}


def _exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return set(re.findall(r" T (edv_\w+)$", out, re.M))


def test_header_declares_and_libraries_export_the_lifecycle():
    from indy_plenum_amd import edv
    src = open(HDR).read()
    for name in NEW:
        assert re.search(r"^int %s\(" % name, src, re.M), name
    d = _defines()
    assert (d["EDV_E_BUSY"], d["EDV_E_SELFTEST"]) == (-5, -6) == (edv.EDV_E_BUSY, edv.EDV_E_SELFTEST)
    assert (d["EDV_TABLES_AUTO"], d["EDV_TABLES_COMPACT"], d["EDV_TABLES_LARGE"]) == (0, 1, 2)
    assert (edv.TABLES_AUTO, edv.TABLES_COMPACT, edv.TABLES_LARGE) == (0, 1, 2)
    assert (d["EDV_SELFTEST_RTL"], d["EDV_SELFTEST_TWO_WALK"], d["EDV_SELFTEST_BATCH"]) == (1, 2, 4)
    assert (edv.SELFTEST_RTL, edv.SELFTEST_TWO_WALK, edv.SELFTEST_BATCH, edv.SELFTEST_ALL) == (1, 2, 4, 7)
    assert d["EDV_PREPARE_ASYNC"] == edv.PREPARE_ASYNC == 1
    libs = [edv.LIB_PATH, edv.MEASURE_LIB_PATH]
    noverify = os.path.join(os.path.dirname(edv.LIB_PATH), "variants", "libedv_noverify.so")
    if os.path.exists(noverify):
        libs.append(noverify)   # the measurement variants take the entry points from the same source
    for path in libs:
        assert set(NEW) <= _exported(path), path
    lib = edv.lib()
    for name in NEW:
        assert getattr(lib, name).argtypes is not None, name


def test_arguments_are_checked_before_the_device():
    from indy_plenum_amd import edv
    lib = edv.lib()
    assert lib.edv_set_table_policy(0, 7) == edv.EDV_E_ARG
    assert lib.edv_set_table_policy(0, -1) == edv.EDV_E_ARG
    assert lib.edv_table_state(0, None) == edv.EDV_E_ARG
    with pytest.raises(edv.EdvError) as ex:
        edv.set_table_policy(0, 3)
    assert ex.value.code == edv.EDV_E_ARG
    # an empty or unknown family mask, no batch size, unknown flags
    assert lib.edv_self_test(0, 0) == edv.EDV_E_ARG
    assert lib.edv_self_test(0, 8) == edv.EDV_E_ARG
    assert lib.edv_prepare(0, 0, 0) == edv.EDV_E_ARG
    assert lib.edv_prepare(0, 400, 2) == edv.EDV_E_ARG


@pytest.mark.skipif(not NO_GPU, reason="a GPU is present")
def test_no_gpu_means_loud_failure_of_the_lifecycle_calls():
    from indy_plenum_amd import edv
    from indy_plenum_amd import node_integration
    assert edv.device_count() == 0
    for call in (lambda: edv.prepare(0, 400), lambda: edv.self_test(0, 7), lambda: edv.release(0),
                 lambda: edv.trim(0, 0), lambda: edv.table_state(0),
                 lambda: edv.set_table_policy(0, edv.TABLES_COMPACT), lambda: node_integration.prepare_node(400)):
        with pytest.raises(edv.EdvUnavailable):
            call()


# ---- the decision function
def _choose(hc, policy, n, have_compact, have_large, failed):
    out = (ctypes.c_int * 3)()
    hc.hc_choose_tables(policy, n, int(have_compact), int(have_large), int(failed), out)
    return tuple(out)


def _expected(policy, n, have_compact, have_large, failed):
    """The issue's rules, written out independently of edv_tables.h: (use, build, failed)."""
    failed = failed and not have_large             # the flag speaks of a set that is not there
    if policy == COMPACT:
        want_large = False
    elif policy == LARGE:
        want_large = have_large or not failed      # the compact set only after a failed build
    else:
        want_large = have_large or (n >= 65536 and not failed)
    if want_large:
        return (SET_LARGE, SET_NONE if have_large else SET_LARGE, int(failed))
    return (SET_COMPACT, SET_NONE if have_compact else SET_COMPACT, int(failed))


GRID = list(itertools.product((AUTO, COMPACT, LARGE), (1, 65535, 65536), (False, True), (False, True), (False, True)))


def test_table_decision_truth_table(hc):
    assert len(GRID) == 72
    for policy, n, hcpt, hlrg, failed in GRID:
        got = _choose(hc, policy, n, hcpt, hlrg, failed)
        assert got == _expected(policy, n, hcpt, hlrg, failed), (policy, n, hcpt, hlrg, failed, got)
        use, build, _f = got
        assert use in (SET_COMPACT, SET_LARGE) and build in (SET_NONE, use)   # only the set used is ever built
        assert (build == SET_NONE) == (hlrg if use == SET_LARGE else hcpt)    # and only when it is not held


def test_table_decision_named_properties(hc):
    for policy, n, hcpt, hlrg, failed in GRID:
        use, build, f = _choose(hc, policy, n, hcpt, hlrg, failed)
        if policy == AUTO and failed and not hlrg:
            assert build != SET_LARGE and use == SET_COMPACT and f == 1     # sticky: no second 3 GiB hipMalloc
        if policy == COMPACT:
            assert use == SET_COMPACT and build != SET_LARGE
        if policy == LARGE and hlrg:
            assert use == SET_LARGE and build == SET_NONE
        if policy == AUTO and hlrg:
            assert use == SET_LARGE                                          # also at n = 1: today's behaviour
    # today's auto policy, in a context that holds the compact set
    assert _choose(hc, AUTO, 1, True, False, False) == (SET_COMPACT, SET_NONE, 0)
    assert _choose(hc, AUTO, 65535, True, False, False) == (SET_COMPACT, SET_NONE, 0)
    assert _choose(hc, AUTO, 65536, True, False, False) == (SET_LARGE, SET_LARGE, 0)
    assert _choose(hc, AUTO, 1, True, True, False) == (SET_LARGE, SET_NONE, 0)
    assert _choose(hc, AUTO, 65536, True, False, True) == (SET_COMPACT, SET_NONE, 1)
    # a policy set on a context that holds only the other set builds its own
    assert _choose(hc, COMPACT, 65536, False, True, False) == (SET_COMPACT, SET_COMPACT, 0)
    assert _choose(hc, LARGE, 1, True, False, False) == (SET_LARGE, SET_LARGE, 0)
    # a trimmed context under auto builds the compact set again
    assert _choose(hc, AUTO, 400, False, False, False) == (SET_COMPACT, SET_COMPACT, 0)


# ---- the embedded known answers
@pytest.fixture(scope="module")
def cases(hc):
    out = []
    for i in range(hc.hc_selftest_count()):
        sig, pk, msg = (ctypes.create_string_buffer(k) for k in (64, 32, 64))
        mlen, accept, rule = ctypes.c_uint64(0), ctypes.c_int(-1), ctypes.c_int(-1)
        cap = hc.hc_selftest_case(i, sig, pk, msg, ctypes.byref(mlen), ctypes.byref(accept), ctypes.byref(rule))
        assert 0 < cap <= 64 and mlen.value <= cap
        out.append((sig.raw, pk.raw, msg.raw[:mlen.value], accept.value, rule.value))
    assert hc.hc_selftest_case(len(out), None, None, None, None, None, None) == -1
    return out


def test_selftest_cases_have_the_stored_verdicts(hc, cases):
    """The CPU build of the kernels' math, the oracle and (where the image has
    it) libsodium all give each embedded case the verdict stored beside it."""
    assert len(cases) >= 10
    want = np.array([c[3] for c in cases], np.uint8)
    assert set(want.tolist()) == {0, 1}
    sigs, pks, msgs = (b"".join(c[k] for c in cases) for k in range(3))
    off = np.zeros(len(cases) + 1, np.uint64)
    off[1:] = np.cumsum([len(c[2]) for c in cases])
    acc = np.zeros(len(cases), np.uint8)
    assert hc.hc_verify_batch(sigs, pks, msgs + b"\0" * 64, off.ctypes.data, len(cases), acc.ctypes.data) == 0
    assert acc.tolist() == want.tolist()
    assert [int(orc.verify(s, m, p)) for s, p, m, _v, _r in cases] == want.tolist()
    assert list(orc.verify_batch(sigs, pks, msgs, off, len(cases))) == want.tolist()
    if orc.sodium_batch():
        a = (np.frombuffer(x + b"\0" * 64, np.uint8) for x in (sigs, pks, msgs))
        assert orc.sodium_verify_batch(*a, off).tolist() == want.tolist()


def test_selftest_cases_come_from_the_committed_fixtures(cases):
    """RFC 8032 section 7.1 vectors 1-3 first, then cases of the golden set
    with the libsodium verdicts committed there."""
    with open(os.path.join(golden_io.GOLDEN, "rfc8032_7_1.json")) as f:
        rfc = [tuple(bytes.fromhex(v[k]) for k in ("sig", "pk", "msg")) for v in json.load(f)["vectors"]]
    assert len(rfc) == 3 and [c[:3] for c in cases[:3]] == rfc
    assert all(c[3] == 1 and c[4] == RULE_NONE for c in cases[:3])
    golden = {(s, p, m): v for v, _c, s, p, m in golden_io.load_ed25519_golden()}
    for sig, pk, msg, v, _rule in cases[3:]:
        assert golden[(sig, pk, msg)] == v


def test_selftest_cases_hit_every_strictness_rule(cases):
    """Each rejecting case is rejected by the rule it is stored under and by no
    earlier one, by the oracle's own predicates, in oref_verify_detached's
    order: V2 S >= L, V3 small-order R, V4 non-canonical / small-order A, V5 A
    off the curve; then the equation."""
    lib = orc.load()

    def first_rule(sig, pk, msg):
        if (sig[63] & 0xF0) and not lib.oref_sc_is_canonical(sig[32:]):
            return RULE_SCALAR
        if lib.oref_has_small_order(sig[:32]):
            return RULE_SMALL_R
        if not lib.oref_ge_is_canonical(pk):
            return RULE_NONCANON_A
        if lib.oref_has_small_order(pk):
            return RULE_SMALL_A
        if orc.point_add(pk, pk) is None:           # the decode fails
            return RULE_OFFCURVE_A
        return RULE_NONE if orc.verify(sig, msg, pk) else RULE_EQUATION

    for k in ("oref_sc_is_canonical", "oref_has_small_order", "oref_ge_is_canonical"):
        getattr(lib, k).argtypes = [ctypes.c_char_p]
    rules = [first_rule(s, p, m) for s, p, m, _v, _r in cases]
    assert rules == [c[4] for c in cases]
    assert {RULE_SCALAR, RULE_SMALL_R, RULE_NONCANON_A, RULE_SMALL_A, RULE_OFFCURVE_A, RULE_EQUATION} <= set(rules)
    assert all((r == RULE_NONE) == bool(c[3]) for r, c in zip(rules, cases))
    # the accepted mixed-order key: of neither small nor prime order (L * A is
    # a non-trivial point of the torsion subgroup), canonical, and accepted
    L = (2**252 + 27742317777372353535851937790883648493).to_bytes(32, "little")
    mixed = [c for c in cases[3:] if c[3] == 1]
    assert mixed
    for _s, pk, _m, _v, _r in mixed:
        t = orc.scalarmult(L, pk)
        assert t is not None and lib.oref_has_small_order(t) and t != (1).to_bytes(32, "little")
