"""Writes carry_chain_golden.json: the limbs fe_mul, fe_sq, fe_sq2,
fe_pow22523 and a run of fe_sq_floor return on the inputs of
tests/carry_chain_cases.py, from a hostcheck library built from the commit
BEFORE the column carries were chained (its edv_math.h adds every carry to the
finished column):

  git worktree add /tmp/parent <that commit> && make -C /tmp/parent/indy-plenum_amd/csrc ../libedv_hostcheck.so
  EDV_HOSTCHECK_OVERRIDE=/tmp/parent/indy-plenum_amd/libedv_hostcheck.so python tests/golden/make_carry_chain_golden.py

Never regenerate it from the code under test: the fixture is what pins the limbs."""
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import carry_chain_cases as cc  # noqa: E402
import hostcheck_lib  # noqa: E402

assert os.environ.get("EDV_HOSTCHECK_OVERRIDE"), "point EDV_HOSTCHECK_OVERRIDE at the earlier commit's library"
hc = hostcheck_lib.load()
V = ctypes.c_int32 * 10


def call(name, *fs):
    out = V()
    getattr(hc, name)(*[V(*f) for f in fs], out)
    return list(out)


ins = cc.inputs()
out = {"fe_mul": [call("hc_fe_mul", f, g) for f, g in ins["fe_mul"]]}
for op in ("fe_sq", "fe_sq2", "fe_pow22523"):
    out[op] = [call("hc_" + op, f) for (f,) in ins["fe_sq"]]
cur, steps = [f for (f,) in ins["fe_sq_floor"]], []
for _ in range(cc.FLOOR_DEPTH):
    cur = [call("hc_fe_sq_floor", f) for f in cur]
    steps.append(cur)
out["fe_sq_floor"] = steps
g = {"in": ins, "out": out}
cc.check_values(g)
with open(cc.GOLDEN, "w") as f:
    json.dump(g, f, separators=(",", ":"))
    f.write("\n")
print("wrote", cc.GOLDEN, os.path.getsize(cc.GOLDEN), "bytes")
