"""Inputs and the committed results (tests/golden/carry_chain_golden.json) for
the limb-for-limb checks of fe_mul, fe_sq, fe_sq2, fe_sq_floor and
fe_pow22523: how a column's carry reaches the next column is an
implementation choice, and no limb may depend on it.  The results were
produced once by the hostcheck library of the commit before the carries were
chained (tests/golden/make_carry_chain_golden.py); both builds of the headers
must reproduce them, the CPU build in test_carry_chain_cpu.py and the device
build in test_gpu_carry_chain.py.  Not a conftest.

N = 65 cases per op: one wave of 64 lanes and one lane of a second wave."""
import json
import os
import random

import math_cases as mc

N = 65
FLOOR_DEPTH = 10
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "carry_chain_golden.json")
# the largest limbs fe_sq_floor is specified for (edv_math.h): 2^26 - 1 (even), 2^25 + 2^16 (odd)
FLOOR_TOP = [(1 << 26) - 1 if i % 2 == 0 else (1 << 25) + (1 << 16) for i in range(10)]


def _sign_patterns():
    """every limb at +-BOUND: all one sign, alternating, one limb against the rest"""
    pats = [[1] * 10, [-1] * 10, [1 if i % 2 == 0 else -1 for i in range(10)],
            [-1 if i % 2 == 0 else 1 for i in range(10)]]
    pats += [[-1 if i == k else 1 for i in range(10)] for k in (0, 1, 8, 9)]
    return [[s * b for s, b in zip(p, mc.BOUND)] for p in pats]


def field_inputs():
    """N limb vectors inside the multiply's input bound: random canonical
    elements, math_cases' bound-extreme vectors, the uniform sign patterns and
    random vectors inside the bound"""
    r = random.Random(0xCA221)
    fs = [mc.limbs(x) for x in (0, 1, mc.P - 1, 2**255 - 20)] + [mc.limbs(r.randrange(mc.P)) for _ in range(16)]
    fs += _sign_patterns()
    fs += [mc.rand_limbs(r, extreme=True) for _ in range(N - len(fs) - 8)]
    fs += [mc.rand_limbs(r) for _ in range(8)]
    assert len(fs) == N
    return fs


def mul_inputs():
    """N pairs: field_inputs() against a rotation of itself, so the extremes meet extremes and canonical values"""
    fs = field_inputs()
    return [[fs[i], fs[(7 * i + 3) % N]] for i in range(N)]


def floor_inputs():
    """N starts of a floor-squaring run: every limb at FLOOR_TOP; each limb at
    FLOOR_TOP or 0 in random patterns and with one limb lowered; math_cases'
    own starts (signed reduced, unsigned extreme); random canonical elements"""
    r = random.Random(0xF100B)
    fs = [list(FLOOR_TOP), [t if i % 2 == 0 else 0 for i, t in enumerate(FLOOR_TOP)],
          [t if i % 2 == 1 else 0 for i, t in enumerate(FLOOR_TOP)]]
    fs += [[t - (1 if i == k else 0) for i, t in enumerate(FLOOR_TOP)] for k in range(10)]
    fs += [[r.choice((t, t, 0, r.randrange(t + 1))) for t in FLOOR_TOP] for _ in range(20)]
    starts = mc.fe_sq_floor_starts()
    fs += starts[-4:] + starts[:12]
    fs += [mc.limbs(r.randrange(mc.P)) for _ in range(N - len(fs))]
    assert len(fs) == N
    return fs


def inputs():
    return {"fe_mul": mul_inputs(), "fe_sq": [[f] for f in field_inputs()], "fe_sq_floor": [[f] for f in floor_inputs()]}


def load():
    """-> {"in": {"fe_mul", "fe_sq", "fe_sq_floor"}, "out": {"fe_mul", "fe_sq",
    "fe_sq2", "fe_pow22523": N limb vectors; "fe_sq_floor": FLOOR_DEPTH lists
    of N limb vectors, step k the square of step k - 1}}.  fe_sq's inputs are
    fe_sq2's and fe_pow22523's."""
    with open(GOLDEN) as f:
        g = json.load(f)
    assert g["in"] == inputs(), "the fixture was made from other inputs: tests/golden/make_carry_chain_golden.py"
    return g


def check_values(g):
    """every committed result against Python integers mod p"""
    P, val = mc.P, mc.val
    for (f, h), o in zip(g["in"]["fe_mul"], g["out"]["fe_mul"]):
        assert val(o) % P == val(f) * val(h) % P
    for (f,), a, b, c in zip(g["in"]["fe_sq"], g["out"]["fe_sq"], g["out"]["fe_sq2"], g["out"]["fe_pow22523"]):
        x = val(f) % P
        assert val(a) % P == x * x % P and val(b) % P == 2 * x * x % P and val(c) % P == pow(x, (P - 5) // 8, P)
    xs = [val(f) % P for (f,) in g["in"]["fe_sq_floor"]]
    for step in g["out"]["fe_sq_floor"]:
        xs = [x * x % P for x in xs]
        assert [val(o) % P for o in step] == xs
