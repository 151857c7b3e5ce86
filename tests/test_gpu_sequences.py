"""Every entry point against its reference across context histories: sequences
of operations on one device context (tests/sequence_cases.py), where what call
B uses depends on what call A left behind -- scratch grown or trimmed, slots
and state sets holding pointers, table sets dropped, settings changed.

  test                         sequence
  ladder[route]                n ascending through the thresholds (1 .. 20,000) on one verify route
                               (pageable, page-locked, asynchronous, device-resident, pipelined); chunks
                               256 -> default -> 1,024 -> 256 between; trims 20,000 / 400 / 1 / 0; latency
                               limits 4,096 and 16,384
  slots                        eight asynchronous batches in flight over the three asynchronous routes,
                               trim / release BUSY, hand-overs out of order, trim(400), the sizes swapped
                               pairwise, a third round that brings the two-walk scratch back smaller and
                               larger, prepare(400, ASYNC), then trim(0) + prepare(64, ASYNC) on the latency
                               and on the batch kernels: 35 covered verifies (n up to k = 64, asynchronous
                               through all eight slots and synchronous) that may allocate nothing
  pipelined                    flags 0 / SPLIT_PREP x length buckets 0 / 1: chunk 1,024, 256, trim(0), default
  two_streams                  two caller streams, no sync between calls: verify, sign, SHA-256, Merkle with
                               66,000 leaves on a; verify of 20,000 (grows the scratch) and pack_bits of a's
                               verdicts on b; trim(0); again
  release_in_the_middle        one operation of every kind (Merkle with null leaf / node outputs,
                               FLAG_UNIFORM_LENGTH, three covered synchronous verifies after prepare(400)
                               among them), release, every kind again; old tickets settled
  table_rotation               COMPACT -> LARGE -> AUTO + trim(400) -> LARGE -> COMPACT + trim(0), 257 and
                               4,097 through every verify route with the latency path on and off
  two_devices                  EDV_VIRTUAL_DEVICES=2: release(0) with a ticket of device 1 outstanding
  random[seed]                 generate(seed, 80): weighted random operations, seeds 41, 42, 65

Every sequence runs in a child process of its own (policy, settings and
contexts are process state), one at a time.  After every operation the runner
checks: outputs equal the references byte for byte and the sentinel bytes past
them are intact; context_memory's parts add up; the total falls only across a
trim or release that returned 0; total == sb_tables (+ the signer's comb
table, which only release frees) after trim(0); context_count and zeros after
release; nothing allocated by a verify that a prepare covers; EDV_E_BUSY exactly
when the model says so, with nothing changed.  A child that ends by signal,
abort or time limit fails its test and skips every later test of this module:
nothing more starts on a card that may have faulted, and no child is rerun.

Operations / bytes compared per test, and wall time of the child on MI355X
(time limit of a child: 120 s, table_rotation's 240 s, about a hundred times
the measured child times):
  test                       operations   bytes compared   test    child   (references)
  ladder[pageable]                   33          175,033   1.24 s  1.00 s  0.21 s
  ladder[pinned3]                    33          175,033   1.11 s  0.85 s  0.21 s
  ladder[async]                      54        2,396,761   1.16 s  0.92 s  0.21 s
  ladder[device]                     33          175,033   1.03 s  0.79 s  0.21 s
  ladder[pipelined]                  54          175,033   1.05 s  0.79 s  0.21 s
  slots                             126        1,485,389   1.11 s  0.84 s  0.21 s
  pipelined                          74          244,952   1.12 s  0.87 s  0.21 s
  two_streams                        22        8,871,012   1.04 s  0.76 s  0.21 s
  release_in_the_middle              69          346,179   1.04 s  0.79 s  0.21 s
  table_rotation                    176          174,440   1.39 s  1.13 s  0.22 s
  two_devices                        26          389,259   1.02 s  0.77 s  0.21 s
  random[41]                         77        4,722,307   1.59 s  1.32 s  0.21 s
  random[42]                         78        6,176,704   1.23 s  0.97 s  0.21 s
  random[65]                         77        5,166,750   1.48 s  1.20 s  0.20 s
These are ABOVE the comparison: in the same run
test_gpu_lifecycle.py::test_release_and_busy took 0.43 s and
test_table_policy_and_trim 0.76 s, and the CPU twin on the same machine
reports 0.22 s for the pool's references plus at most 0.64 s for a list's own,
so the comparison is 0.65-1.29 s (0.98 s for table_rotation) and every test
here exceeds its own by 0.3-0.6 s.  The excess is paid once per child before
its first operation (the 45 MB pool uploaded and page-locked, the model's
trace in the parent), so two children per list would cost more, not less.
"""
import json
import os
import subprocess
import sys

import pytest

import sequence_cases as sc

pytestmark = pytest.mark.gpu
TESTS = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(TESTS)
_card = {"suspect": None}     # set by a child that ended by signal, abort or time limit


def child(name, timeout=120, upto=None):
    if _card["suspect"]:
        pytest.skip("not started: " + _card["suspect"])
    env = {k: v for k, v in os.environ.items() if k not in ("EDV_SB_TABLES", "EDV_VIRTUAL_DEVICES", "EDV_LIB",
                                                           "EDV_ALLOW_MEASUREMENT_LIB", "EDV_CHUNK")}
    env.update(sc.DIRECTED[name][2] if name in sc.DIRECTED else {})
    code = "import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import sequence_cases as sc; " \
           "sc.child_main(%r, %r)" % (ROOT, TESTS, name, upto)
    try:
        r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        _card["suspect"] = "the child of %s ran into its time limit of %d s" % (name, timeout)
        pytest.fail(_card["suspect"])
    hip = r.returncode == sc.HIP_FAULT_STATUS or (r.returncode != 0 and
                                                  any(w in r.stderr for w in sc.HIP_FAULT_WORDS))
    if r.returncode < 0 or r.returncode in (134, 139) or hip:       # a HIP error counts as a fault of the card too
        _card["suspect"] = "the child of %s ended with status %d%s" % (name, r.returncode,
                                                                       ", a HIP error" if hip else "")
        pytest.fail(_card["suspect"] + "\n" + r.stderr[-3000:])
    assert r.returncode == 0, r.stderr[-6000:]
    d = json.loads(r.stdout.strip().splitlines()[-1])
    print("%-28s %3d operations, %9d bytes compared, references %.2f s, run %.2f s, child %.2f s" % (
        name, d["operations"], d["comparisons"], d["references_s"], d["run_s"], d["total_s"]))
    want = sum(1 for t in sc.trace_of(*sc.sequence(name)[:2]) if t["noalloc"])
    assert d["noalloc_checks"] == want, "%d no-allocation checks ran, the model has %d" % (d["noalloc_checks"], want)
    return d


@pytest.mark.parametrize("route", sc.LADDER_ROUTES)
def test_ladder(route):
    d = child("ladder_" + route)
    assert d["operations"] == len(sc.sequence("ladder_" + route)[0]) and d["comparisons"] > 170000


def test_slots():
    d = child("slots")
    # 8 + 3 after prepare(400, ASYNC); 2 x (8 + 4) after trim(0), prepare(64, ASYNC)
    assert d["noalloc_checks"] == 35


def test_pipelined():
    assert child("pipelined")["comparisons"] > 240000


def test_two_streams():
    assert child("two_streams")["comparisons"] > 8000000


def test_release_in_the_middle():
    d = child("release_in_the_middle")
    assert d["operations"] == len(sc.sequence("release_in_the_middle")[0])
    assert d["noalloc_checks"] == 6       # three synchronous verifies after each prepare(400), around the release


def test_table_rotation():
    assert child("table_rotation", timeout=240)["operations"] == len(sc.sequence("table_rotation")[0])


def test_two_devices():
    assert child("two_devices")["operations"] == len(sc.sequence("two_devices")[0])


@pytest.mark.parametrize("seed", sc.SEEDS)
def test_random(seed):
    d = child("random_%d" % seed)
    assert d["operations"] == len(sc.generate(seed, sc.STEPS))
