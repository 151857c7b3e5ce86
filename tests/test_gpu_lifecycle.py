"""Context lifecycle on the device (include/edv.h: edv_prepare, edv_self_test,
edv_set_table_policy / edv_table_state, edv_trim, edv_release).  Policy and
contexts are process state, so every scenario runs in a child process of its
own, as test_context_memory_and_table_sets does.  Verdicts are compared with
the oracle's on a 512-request corpus (5 % invalid); the 65,536-request batches
(kLargeTablesMin, the smallest that asks for the large table set) are that
corpus tiled 128 times."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NOVERIFY = os.path.join(ROOT, "indy-plenum_amd", "variants", "libedv_noverify.so")
MiB, GiB = 2**20, 2**30
COMPACT_ONLY = 80 * MiB   # test_context_memory_and_table_sets' bound for "the compact set only"

PRELUDE = r'''
import json, sys, time, numpy as np
sys.path.insert(0, %r); sys.path.insert(0, %r)
import oracle_lib as orc
from indy_plenum_amd import edv
S, P, M, O = orc.corpus(0x11FEC, 0, 512, mode=0, invalid_permille=50)
WANT = np.frombuffer(orc.verify_batch(S.tobytes(), P.tobytes(), M.tobytes(), O, 512, 8), dtype=np.uint8).copy()
assert 0 < int(WANT.sum()) < 512


def head(k):
    """the corpus' first k requests, and their verdicts"""
    return (S[:64 * k], P[:32 * k], M, O[:k + 1]), WANT[:k]


def tiled(times=128):
    """the corpus `times` times over (offsets rebuilt), and the tiled verdicts"""
    lens = np.tile(np.diff(O), times)
    off = np.zeros(len(lens) + 1, np.uint64)
    off[1:] = np.cumsum(lens)
    msgs = np.concatenate([np.tile(M[:int(O[-1])], times), np.zeros(64, np.uint8)])
    return (np.tile(S, times), np.tile(P, times), msgs, off), np.tile(WANT, times)


def check(batch, mask=0):
    args, want = batch
    return bool(np.array_equal(edv.verify_arrays(*args, device_mask=mask), want))


def code_of(call):
    try:
        call()
    except edv.EdvError as ex:
        return [ex.code, str(ex)]
    return [0, ""]


out = {}
''' % (ROOT, os.path.join(ROOT, "tests"))


def child(body, env=None, timeout=300):
    e = {k: v for k, v in os.environ.items() if k not in ("EDV_SB_TABLES", "EDV_VIRTUAL_DEVICES", "EDV_LIB",
                                                          "EDV_ALLOW_MEASUREMENT_LIB", "EDV_CHUNK")}
    e.update(env or {})
    r = subprocess.run([sys.executable, "-c", PRELUDE + body + "\nprint(json.dumps(out))\n"], capture_output=True,
                       text=True, timeout=timeout, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def parts_add_up(m):
    return m["total"] == sum(v for k, v in m.items() if k != "total")


def test_prepare_takes_the_cold_start_off_the_first_verify():
    """edv_prepare(0, 400) in a fresh process creates the context with the
    compact table set only; the first verify of 400 requests then allocates
    nothing (edv_context_memory unchanged), gives the oracle's verdicts and is
    faster than the first verify of a process that did not prepare (the parent
    behaviour: context creation inside the call; two orders of magnitude in
    DESIGN.md section 2).  With EDV_PREPARE_ASYNC the same holds for an
    asynchronous submission."""
    first = r'''
batch = head(400)
t0 = time.perf_counter()
ok = check(batch)
out["first_ms"] = (time.perf_counter() - t0) * 1e3
out["equal"] = ok
out["after"] = edv.context_memory(0)
'''
    prepared = child(r'''
edv.prepare(0, 400)
out["count"] = edv.context_count()
out["before"] = edv.context_memory(0)
out["tables"] = edv.table_state(0)
''' + first + r'''
edv.prepare(0, 400, edv.PREPARE_ASYNC)
out["async_before"] = edv.context_memory(0)
(s, p, m, o), want = batch
acc = np.zeros(400, np.uint8)
edv.wait_async(edv.verify_async(s, p, m, o, acc))
out["async_equal"] = bool(np.array_equal(acc, want))
out["async_after"] = edv.context_memory(0)
''')
    cold = child("out['count0'] = edv.context_count()\n" + first)
    print("first verify of 400: prepared %.3f ms, unprepared %.3f ms" % (prepared["first_ms"], cold["first_ms"]))
    print("footprint after prepare(0, 400):", prepared["before"], "with the asynchronous slots:",
          prepared["async_before"])
    assert prepared["count"] == 1 and cold["count0"] == 0
    m = prepared["before"]
    assert 0 < m["sb_tables"] < COMPACT_ONLY and parts_add_up(m)
    assert prepared["tables"]["compact_bytes"] == m["sb_tables"] and prepared["tables"]["large_bytes"] == 0
    assert prepared["equal"] and cold["equal"]
    assert prepared["after"] == prepared["before"]
    assert prepared["async_equal"] and prepared["async_after"] == prepared["async_before"]
    assert parts_add_up(prepared["async_before"]) and prepared["async_before"]["async_slots"] > 0
    assert prepared["first_ms"] < cold["first_ms"]


def test_prepare_node_pins_the_compact_set():
    """node_integration.prepare_node: compact-only policy, context and slots
    ready; a batch of 65,536 afterwards builds no 3 GiB set."""
    d = child(r'''
from indy_plenum_amd import node_integration
r = node_integration.prepare_node(max_prod=400)
out["r"] = r
out["same"] = r["tables"] == edv.table_state(r["device"]) and r["memory"] == edv.context_memory(r["device"])
out["eq"] = check(tiled(), 1 << r["device"])
out["after"] = edv.table_state(r["device"])
''')
    r = d["r"]
    assert d["same"] and r["tables"]["policy"] == 1 and r["tables"]["large_bytes"] == 0
    assert 0 < r["memory"]["sb_tables"] < COMPACT_ONLY and r["memory"]["async_slots"] > 0
    assert r["memory"]["total"] < 100 * MiB and parts_add_up(r["memory"])
    assert d["eq"] and d["after"]["large_bytes"] == 0 and d["after"]["large_failed"] == 0


def test_self_test_passes_on_the_product_on_either_table_set():
    d = child(r'''
edv.self_test(0, 7)
out["compact"] = edv.table_state(0)
for fam in (edv.SELFTEST_RTL, edv.SELFTEST_TWO_WALK, edv.SELFTEST_BATCH):
    edv.self_test(0, fam)
edv.set_table_policy(0, edv.TABLES_LARGE)
edv.prepare(0, 1)
out["large"] = edv.table_state(0)
edv.self_test(0, 7)
out["mem"] = edv.context_memory(0)
''')
    assert d["compact"]["compact_bytes"] > 0 and d["compact"]["large_bytes"] == 0   # never the 3 GiB set for its own sake
    assert d["large"]["policy"] == 2 and d["large"]["large_bytes"] > 3 * GiB and d["large"]["large_failed"] == 0
    assert d["mem"]["sb_tables"] > 3 * GiB


@pytest.mark.skipif(not os.path.exists(NOVERIFY), reason="variants/libedv_noverify.so is not built")
def test_self_test_fails_the_build_that_skips_verification():
    """The measurement variant reports every request valid: each family's
    self-test, and edv_prepare, return EDV_E_SELFTEST naming family and case."""
    d = child(r'''
out["all"] = code_of(lambda: edv.self_test(0, 7))
out["fam"] = [code_of(lambda: edv.self_test(0, f)) for f in (1, 2, 4)]
out["prepare"] = code_of(lambda: edv.prepare(0, 400))
''', env={"EDV_LIB": NOVERIFY, "EDV_ALLOW_MEASUREMENT_LIB": "1"})
    assert d["all"][0] == -6 and "family RTL" in d["all"][1] and "case 3" in d["all"][1]
    assert [c for c, _t in d["fam"]] == [-6, -6, -6]
    assert ["RTL" in d["fam"][0][1], "TWO_WALK" in d["fam"][1][1], "BATCH" in d["fam"][2][1]] == [True] * 3
    assert d["prepare"][0] == -6


def test_table_policy_and_trim():
    d = child(r'''
edv.set_table_policy(0, edv.TABLES_COMPACT)
out["m0"] = edv.context_memory(0)
big = tiled()
out["eq1"] = check(big); out["m1"] = edv.context_memory(0); out["t1"] = edv.table_state(0)
edv.set_table_policy(0, edv.TABLES_AUTO)
out["eq2"] = check(big); out["m2"] = edv.context_memory(0); out["t2"] = edv.table_state(0)
out["eq3"] = check(head(400)); out["t3"] = edv.table_state(0)
edv.trim(0, 400)
out["m4"] = edv.context_memory(0); out["t4"] = edv.table_state(0); out["count4"] = edv.context_count()
out["eq5"] = check(head(400)); out["m5"] = edv.context_memory(0)
out["eq6"] = check(big); out["m6"] = edv.context_memory(0); out["t6"] = edv.table_state(0)
edv.trim(0, 0)
out["m7"] = edv.context_memory(0)
out["eq7"] = check(head(400))
''')
    assert all(d["eq%d" % k] for k in (1, 2, 3, 5, 6, 7))
    assert d["m1"]["sb_tables"] < COMPACT_ONLY and d["t1"]["large_bytes"] == 0 and d["t1"]["policy"] == 1
    assert d["m2"]["sb_tables"] > 3 * GiB and d["t2"]["large_bytes"] > 3 * GiB and d["t2"]["policy"] == 0
    assert d["t3"] == d["t2"]                                   # the small batch ran on the large set, as today
    assert d["m4"]["sb_tables"] < COMPACT_ONLY and d["t4"]["large_bytes"] == 0 and d["t4"]["compact_bytes"] > 0
    assert d["m4"]["chunk_scratch"] <= d["m0"]["chunk_scratch"] and d["m1"]["chunk_scratch"] > 0
    assert d["count4"] == 1 and parts_add_up(d["m4"])
    assert d["m5"]["sb_tables"] < COMPACT_ONLY                  # a small batch after the trim: no large set
    assert d["m6"]["sb_tables"] > 3 * GiB and d["t6"]["large_bytes"] > 3 * GiB and d["t6"]["large_failed"] == 0
    # trim(0, 0) under auto: every buffer goes, the compact set stays
    m7 = d["m7"]
    assert m7["total"] == m7["sb_tables"] < COMPACT_ONLY


def test_shared_table_sets_go_with_their_last_holder():
    d = child(r'''
full = head(512)
for dev in (0, 1):
    edv.set_table_policy(dev, edv.TABLES_LARGE)
    edv.prepare(dev, 1)
out["t1"] = [edv.table_state(k) for k in (0, 1)]; out["m1"] = [edv.context_memory(k) for k in (0, 1)]
edv.set_table_policy(0, edv.TABLES_AUTO); edv.trim(0, 400)
out["eq2"] = check(full, 2)
out["t2"] = [edv.table_state(k) for k in (0, 1)]; out["m2"] = [edv.context_memory(k) for k in (0, 1)]
edv.set_table_policy(1, edv.TABLES_AUTO); edv.trim(1, 400)
out["t3"] = [edv.table_state(k) for k in (0, 1)]; out["m3"] = [edv.context_memory(k) for k in (0, 1)]
out["eq4"] = [check(full, 1), check(full, 2)]
out["m4"] = [edv.context_memory(k) for k in (0, 1)]
out["devices"] = edv.device_count()
''', env={"EDV_VIRTUAL_DEVICES": "2"})
    assert d["devices"] == 2
    for k in (0, 1):
        assert d["t1"][k]["large_bytes"] > 3 * GiB and d["t1"][k]["compact_bytes"] == 0
        assert 3 * GiB < d["m1"][k]["sb_tables"] < 4 * GiB         # one set in the process, not two
    assert d["eq2"]
    assert d["t2"][0]["large_bytes"] == 0 and d["t2"][1]["large_bytes"] > 3 * GiB
    assert d["m2"][1]["sb_tables"] > 3 * GiB                        # device 1 still holds it
    for k in (0, 1):
        assert d["t3"][k]["large_bytes"] == 0 and d["m3"][k]["sb_tables"] < COMPACT_ONLY
    assert d["eq4"] == [True, True]
    for k in (0, 1):
        assert 0 < d["m4"][k]["sb_tables"] < COMPACT_ONLY           # the compact set, built again by use


def test_release_and_busy():
    d = child(r'''
batch = head(400)
(s, p, m, o), want = batch
out["eq1"] = check(batch)
acc = np.zeros(400, np.uint8)
t = edv.verify_async(s, p, m, o, acc)
before = (edv.context_count(), edv.context_memory(0), edv.table_state(0))
out["busy_release"] = code_of(lambda: edv.release(0))[0]
out["busy_trim"] = code_of(lambda: edv.trim(0, 0))[0]
out["unchanged"] = before == (edv.context_count(), edv.context_memory(0), edv.table_state(0))
edv.wait_async(t)
out["eq4"] = bool(np.array_equal(acc, want))
edv.set_latency_path(0, 8192)
edv.release(0)
out["count5"] = edv.context_count(); out["m5"] = edv.context_memory(0); out["t5"] = edv.table_state(0)
edv.release(0)                      # nothing to release: not an error
out["eq6"] = check(batch); out["count6"] = edv.context_count(); out["m6"] = edv.context_memory(0)
kept = acc.copy()
out["old_wait"] = code_of(lambda: edv.wait_async(t))[0]
out["old_query"] = edv.query_async(t)
out["old_untouched"] = bool(np.array_equal(acc, kept))
acc2 = np.zeros(400, np.uint8)
t2 = edv.verify_async(s, p, m, o, acc2)
out["tickets"] = [t, t2]
out["never_issued"] = code_of(lambda: edv.wait_async(t2 + 1))[0]
edv.wait_async(t2)
out["eq7"] = bool(np.array_equal(acc2, want))
edv.release(0)
out["count8"] = edv.context_count()
''')
    assert d["eq1"] and d["eq4"] and d["eq6"] and d["eq7"]
    assert d["busy_release"] == -5 and d["busy_trim"] == -5 and d["unchanged"]
    assert d["count5"] == 0 and all(v == 0 for v in d["m5"].values())
    assert d["t5"]["compact_bytes"] == 0 and d["t5"]["large_bytes"] == 0
    assert d["count6"] == 1 and d["m6"]["sb_tables"] > 0
    # the old ticket is settled: neither pending nor mistaken for a batch of the new context
    assert d["old_wait"] == 0 and d["old_query"] is True and d["old_untouched"]
    assert d["tickets"][1] == d["tickets"][0] + 1 and d["never_issued"] == -1
    assert d["count8"] == 0


def test_golden_parity_under_either_policy_and_path():
    """The golden set (3,284 cases, verdicts by libsodium) under the compact and
    the large policy, through the latency path (default) and the batch
    kernels (edv_set_latency_path(0, 0))."""
    d = child(r'''
import golden_io
recs = golden_io.load_ed25519_golden()
sigs, pks, msgs, off = golden_io.pack_batch(recs)
want = np.array([r[0] for r in recs], np.uint8)
out["n"] = len(recs)
for name, pol in (("compact", edv.TABLES_COMPACT), ("large", edv.TABLES_LARGE)):
    edv.set_table_policy(0, pol)
    for path, limit in (("latency", edv.LATENCY_PATH_DEFAULT), ("batch", 0)):
        edv.set_latency_path(0, limit)
        out[name + "/" + path] = bool(np.array_equal(edv.verify_arrays(sigs, pks, msgs + b"\0" * 64, off), want))
    out[name] = edv.table_state(0)
''')
    assert d["n"] == 3284
    for k in ("compact/latency", "compact/batch", "large/latency", "large/batch"):
        assert d[k], k
    assert d["compact"]["compact_bytes"] > 0 and d["compact"]["large_bytes"] == 0
    assert d["large"]["large_bytes"] > 3 * GiB
