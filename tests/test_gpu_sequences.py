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
                               FLAG_UNIFORM_LENGTH, three covered synchronous verifies after prepare(400),
                               the batched append, both proof verifications in both forms and a chain step
                               among them), release, every kind again; old tickets settled; the chain goes
                               on from the host copy of its frontier
  table_rotation               COMPACT -> LARGE -> AUTO + trim(400) -> LARGE -> COMPACT + trim(0), 257 and
                               4,097 through every verify route with the latency path on and off
  two_devices                  EDV_VIRTUAL_DEVICES=2: release(0) with a ticket of device 1 outstanding
  random[seed]                 generate(seed, 80): weighted random operations, seeds 41, 42, 65
  merkle_staging               host forms only: inclusion 4,097 with computed roots, consistency 63 without,
                               inclusion by hash 65 with, consistency 257 with, inclusion 1; trim(257); the
                               five backwards; trim(1); all again; between them host appends with all sixteen
                               combinations of the output flags at n = 65 / 1,000 / 64 and extends with null
                               outputs in the same staging; then a capacity kept by trim(257), met smaller
                               and larger
  merkle_fold_streams          append_device with null leaf / node outputs (the fold scratch): 257 on a,
                               66,000 on b (a grow while a's is queued), 63 on a, an extend with all outputs
                               on b, an inclusion verify of the first append's own path and root buffers on a,
                               a consistency verify on the library stream, trim(0) with all of it queued, the
                               syncs; again as b, a; release; once more
  ledger_chain                 ten chained appends (63, 1, 65, 257, 64, 1,000, 66,000, 1, 63, 64) on alternating
                               streams from size 0: d_old_hashes is the frontier buffer of the append before,
                               chain_verify reads the path and root buffers as they are, a consistency proof
                               from the size before with every step; across 128, 256, 512, 1,024 ... 65,536;
                               trim(257) kept, trim / release BUSY, release (restart from the host copy of the
                               frontier), trim(0); a sync only where the next consumer is on another stream
  random_merkle[seed]          generate(seed, 120, merkle=True): the weighted random operations with the new
                               kinds placed between them as motifs, seeds 110, 214

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
The rows above are from the run that added them.  In a later run (the one that added the lists below) the
children of the commit before took 0.85 s (two_streams) and 0.76 s (release_in_the_middle), the comparison for
the new lists; "(own)" is what the list's own Merkle references cost in the child (simulate_appends, simulate,
the proof synthesiser and checker; the 66,000-leaf append is 0.3 s of it), which a list may add to that:
  test                       operations   bytes compared   test    child   (pool)  (own)
  release_in_the_middle              87          529,607   1.17 s  0.91 s  0.20 s  0.02 s
  merkle_staging                     72        2,813,805   1.96 s  1.23 s  0.20 s  0.48 s
  merkle_fold_streams                29       57,318,886   1.33 s  1.06 s  0.20 s  0.36 s
  ledger_chain                       31       25,844,135   1.38 s  1.12 s  0.20 s  0.40 s
  random_merkle[110]                140        8,317,652   1.25 s  0.96 s  0.21 s  0.06 s
  random_merkle[214]                124       10,153,662   1.54 s  1.24 s  0.20 s  0.05 s
merkle_staging (comparison 1.24-1.33 s), merkle_fold_streams (1.12-1.21 s) and ledger_chain (1.16-1.25 s) are
within theirs.  random_merkle[110] is 0.05-0.14 s above (0.82-0.91 s) and random_merkle[214] 0.34-0.43 s above
(0.81-0.90 s): they are 140 and 124 operations of every kind, verifies of 20,000 and signing among them, where
the two compared lists have 22 and 69; random[41] takes 1.41 s for 77.  release_in_the_middle is 0.15 s above
its own earlier form for its 18 new operations.  merkle_staging's test time has 0.7 s on top of its child: the
model's trace in the parent builds the proof batches to size the staging.  The limit stays 120 s.

The earlier rows are ABOVE the comparison: in the same run
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


def _merkle_child(name):
    """a list with the batched append and the proof verification in it: every operation ran, and every device
    verify the model marks was compared with context_memory"""
    d = child(name)
    ops, devices, _seed = sc.sequence(name)
    assert d["operations"] == len(ops)
    assert d["nomem_checks"] == sum(1 for t in sc.trace_of(ops, devices) if t.get("nomem"))
    print("%-28s its own Merkle references %.2f s" % (name, d["merkle_references_s"]))
    return d


def test_merkle_staging():
    assert _merkle_child("merkle_staging")["comparisons"] > 2800000


def test_merkle_fold_streams():
    d = _merkle_child("merkle_fold_streams")
    assert d["comparisons"] > 57000000 and d["nomem_checks"] == 6


def test_ledger_chain():
    d = _merkle_child("ledger_chain")
    assert d["comparisons"] > 25000000 and d["nomem_checks"] >= 6


@pytest.mark.parametrize("seed", sc.MERKLE_SEEDS)
def test_random_merkle(seed):
    _merkle_child("random_merkle_%d" % seed)
