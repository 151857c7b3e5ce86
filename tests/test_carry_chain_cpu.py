"""fe_mul, fe_sq, fe_sq2, fe_sq_floor, fe_sqn and fe_pow22523 of the CPU build
of edv_math.h, limb for limb against tests/golden/carry_chain_golden.json (the
results of the code before the column carries were chained, on random
canonical elements, the bound-extreme vectors of math_cases.py and, for the
floor squarings, limbs at 2^26 - 1 / 2^25 + 2^16), and the fixture itself
against Python integers.  Then the same arithmetic as a stand-alone program
under UBSan (tools/ubsan_carry_chain.cpp): the 64-bit columns, with a carry
as their start where the columns are chained, must stay inside int64 on every
extreme input, and the chained and the unchained floor squaring must print
one checksum."""
import ctypes
import os
import shutil
import subprocess

import pytest

import carry_chain_cases as cc
import hostcheck_lib

V = ctypes.c_int32 * 10
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def golden():
    return cc.load()


def call(name, *args):
    out = V()
    getattr(hostcheck_lib.load(), name)(*[V(*a) if isinstance(a, list) else a for a in args], out)
    return list(out)


def test_fixture_is_exact(golden):
    cc.check_values(golden)
    assert all(len(golden["out"][op]) == cc.N for op in ("fe_mul", "fe_sq", "fe_sq2", "fe_pow22523"))
    assert len(golden["out"]["fe_sq_floor"]) == cc.FLOOR_DEPTH


def test_fe_mul_limbs(golden):
    for (f, g), want in zip(golden["in"]["fe_mul"], golden["out"]["fe_mul"]):
        assert call("hc_fe_mul", f, g) == want, (f, g)


@pytest.mark.parametrize("op", ["fe_sq", "fe_sq2", "fe_pow22523"])
def test_fe_sq_limbs(golden, op):
    for (f,), want in zip(golden["in"]["fe_sq"], golden["out"][op]):
        assert call("hc_" + op, f) == want, (op, f)


def test_fe_sq_floor_run_limbs(golden):
    cur = [f for (f,) in golden["in"]["fe_sq_floor"]]
    for k, want in enumerate(golden["out"]["fe_sq_floor"]):
        cur = [call("hc_fe_sq_floor", f) for f in cur]
        assert cur == want, ("step", k)


def test_fe_sqn_limbs(golden):
    """fe_sqn(f, n) is the run's step n (its squarings are the floor ones)"""
    for n in (1, 2, cc.FLOOR_DEPTH):
        for (f,), want in zip(golden["in"]["fe_sq_floor"], golden["out"]["fe_sq_floor"][n - 1]):
            assert call("hc_fe_sqn", f, ctypes.c_int(n)) == want, (n, f)


def test_columns_stay_inside_int64_under_ubsan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "the UBSan program needs the C++ compiler the harness library is built with"
    src = os.path.join(ROOT, "tools", "ubsan_carry_chain.cpp")
    outs = []
    for name, flags in (("chained", []), ("unchained", ["-DEDV_CHAIN_FLOOR=0"])):
        exe = str(tmp_path / name)
        subprocess.check_call([cxx, "-O1", "-std=c++17", "-fsanitize=signed-integer-overflow,undefined",
                               "-fno-sanitize-recover=all", "-Wno-unknown-pragmas"] + flags + [src, "-o", exe])
        r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and not r.stderr, (name, r.returncode, r.stderr[-2000:])
        outs.append(r.stdout)
    assert outs[0] == outs[1] and outs[0].startswith("ok 12294 "), outs
