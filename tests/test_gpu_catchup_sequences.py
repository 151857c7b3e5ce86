"""Catch-up across a context history (row f-10), in the manner of
tests/test_gpu_sequences.py: one list of operations on one device context, in a
child process of its own (contexts and settings are process state), checked
after every operation (tests/catchup_history.py).

  catchup_history    host form, device form with null hash outputs (the fold scratch), host form;
                     trim(0); host form of an altered case with null outputs, device form, the tree of
                     2^40 + 5 leaves on the device form with every optional output null; trim(1);
                     device form, host form (altered cases); release; device form in the fresh
                     context (its event and every buffer again), host form, extend_verified's device
                     route, the 2^40 + 5 tree through the host form; trim(0); release

A child that ends by signal, abort, HIP error or time limit fails the test; it
is not run again."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)


def test_catchup_history():
    env = {k: v for k, v in os.environ.items() if k not in ("EDV_SB_TABLES", "EDV_VIRTUAL_DEVICES", "EDV_LIB",
                                                           "EDV_ALLOW_MEASUREMENT_LIB", "EDV_CHUNK")}
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import catchup_history; " \
           "catchup_history.child_main()" % (ROOT, TESTS)
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120, env=env)
    except subprocess.TimeoutExpired:
        pytest.fail("the child ran into its time limit of 120 s")
    assert r.returncode == 0, "the child ended with status %d\n%s" % (r.returncode, r.stderr[-6000:])
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print("catchup_history: %d operations, %d bytes compared, %d booked against the host plan, child %.2f s" % (
        d["operations"], d["comparisons"], d["booked"], d["total_s"]))
    assert d["operations"] == 17 and d["booked"] >= 9 and d["comparisons"] > 100000
