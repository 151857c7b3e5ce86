"""The device build of fe_mul, fe_sq, fe_sq2, fe_sq_floor and fe_pow22523
(the probe kernels of libedv_measure.so), limb for limb against
tests/golden/carry_chain_golden.json: the limbs of the code before the column
carries were chained.  Each op runs as one wave of 64 lanes and as 65 lanes,
so the last case sits alone in a second wave."""
import pytest

import carry_chain_cases as cc
import probe_lib as pl

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def golden():
    return cc.load()


def run(op, cases, n):
    return [h[0] for h in pl.unpack_limbs(pl.device(op, pl.pack_limbs(cases[:n])))]


@pytest.mark.parametrize("n", [64, 65])
def test_fe_mul_limbs(golden, n):
    assert run("fe_mul", golden["in"]["fe_mul"], n) == golden["out"]["fe_mul"][:n]


@pytest.mark.parametrize("n", [64, 65])
@pytest.mark.parametrize("op", ["fe_sq", "fe_sq2", "fe_pow22523"])
def test_fe_sq_limbs(golden, op, n):
    assert run(op, golden["in"]["fe_sq"], n) == golden["out"][op][:n]


@pytest.mark.parametrize("n", [64, 65])
def test_fe_sq_floor_run_limbs(golden, n):
    """every step of the run from the step before, as the CPU test walks it"""
    cur = [f for (f,) in golden["in"]["fe_sq_floor"]]
    for k, want in enumerate(golden["out"]["fe_sq_floor"]):
        cur = run("fe_sq_floor", [[f] for f in cur], n)
        assert cur == want[:n], ("step", k)
