"""Catch-up in one call (row f-10) without a GPU: the kernel's lane on the CPU
(hc_merkle_catchup) against the model of tests/merkle_catchup_cases.py on every
case and mutation, the model against the reference's recorded outcomes, the
Python host route (CompactMerkleTree.extend_verified, Ledger.applyCatchupReplies)
against the loop it replaces (verify_catchup_txns, then add per transaction),
the host plan, and the C ABI's argument checks."""
import ctypes

import numpy as np
import pytest

import merkle_cases as mc
import merkle_catchup_cases as cc
import merkle_verify_cases as vc
from indy_plenum_amd import Ledger, edv, merkle

CASES = cc.all_cases()
REAL = [c for c in CASES if c.real]
THREE = next(c for c in CASES if c.name == "old5-parts3_0_4-final+37")


# ---- the model itself
def test_model_gives_what_the_reference_recorded():
    g = cc.load_golden()
    assert sorted(g["outcomes"]) == sorted(c.name for c in REAL)
    for c in REAL:
        assert cc.golden_statuses(g, c.name) == list(cc.model(c).status), c.name


def test_intact_cases_are_accepted_whole():
    for c in CASES:
        if ":" not in c.name:
            x = cc.model(c)
            assert set(x.status) == {vc.OK} and x.accepted == len(c.parts) and x.size == c.old + len(c.leaves), c.name


def test_bad_transaction_is_root_or_inconsistent_by_the_size():
    """After a flipped transaction the reply's root is wrong.  Where its size is
    a power of two the walk seeds from that root and arrives at another new
    root (ROOT); where it is not, the proof alone gives the new root and the old
    one differs (INCONSISTENT), as it does for equal sizes."""
    seen = set()
    for c in CASES:
        if ":txn@" not in c.name:
            continue
        j, base = int(c.name[-1]), next(b for b in CASES if b.name == c.name.split(":")[0])
        if c.parts[j] == base.parts[j]:
            continue  # an empty reply: nothing was flipped
        x = cc.model(c)
        assert x.accepted == j
        for k in range(j, len(c.parts)):
            s = c.old + c.ends[k]
            want = vc.ROOT if s & (s - 1) == 0 and s != c.final_size else vc.INCONSISTENT
            assert x.status[k] == want, (c.name, k)
            seen.add(want)
    assert seen == {vc.ROOT, vc.INCONSISTENT}


def test_cases_cover_the_seams():
    sizes = [(c.old + e, c.final_size) for c in CASES if ":" not in c.name for e in c.ends]
    assert any(s == 0 for s, _ in sizes) and any(s == f for s, f in sizes)
    assert any(s & (s - 1) == 0 and 0 < s < f for s, f in sizes)
    assert any(c.ends[k] == c.ends[k - 1] for c in CASES for k in range(1, len(c.ends)))
    assert any(c.old > 2 ** 40 for c in CASES)


# ---- the lane on the CPU
def test_lane_on_every_case_and_mutation():
    for c in CASES:
        cc.check_outputs(c, *cc.hc_catchup(c))


@pytest.mark.parametrize("want", [(False, False, False), (True, False, True), (False, True, False)])
def test_lane_leaves_unwanted_outputs_alone(want):
    for c in CASES[::7]:
        cc.check_outputs(c, *cc.hc_catchup(c, want_leaf=want[0], want_node=want[1], want_roots=want[2]))


def test_harness_rejects_an_end_past_the_call():
    """hc_merkle_catchup makes the host form's argument checks: ends that fall are -1 and nothing is written."""
    a = cc.HostArgs(THREE)
    ends = a.ends.copy()
    ends[1] = a.n + 1
    st = cc.guarded(a.replies)
    rc = cc.hostcheck().hc_merkle_catchup(THREE.old, a.old.ctypes.data, a.blob.ctypes.data, a.off.ctypes.data, a.n,
                                          ends.ctypes.data, a.replies, THREE.final_size, a.root.ctypes.data,
                                          a.proofs.ctypes.data, a.poff.ctypes.data, None, None, None, st.ctypes.data)
    assert rc == -1 and st.tobytes() == bytes([cc.SENTINEL]) * len(st)


# ---- the host plan
def _needs(old, n, mbytes, replies, entries, host, wl, wn, wr):
    out = np.zeros(20, np.uint64)
    cc.hostcheck().hc_merkle_catchup_needs(old, n, mbytes, replies, entries, host, wl, wn, wr, out.ctypes.data)
    return [int(x) for x in out]


def _extend_needs(old, n, mbytes, host, wl, wn):
    lib = mc.hostcheck()
    lib.hc_merkle_extend_needs.argtypes = [ctypes.c_uint64] * 3 + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    lib.hc_merkle_extend_needs.restype = None
    out = np.zeros(15, np.uint64)
    lib.hc_merkle_extend_needs(old, n, mbytes, host, wl, wn, 0, 0, out.ctypes.data)
    return [int(x) for x in out]


@pytest.mark.parametrize("old,n,replies,entries", [(0, 0, 1, 0), (5, 7, 3, 9), (255, 513, 3, 20),
                                                   (2 ** 40 + 5, 5, 2, 40), (0, 70000, 700, 9000)])
def test_host_plan(old, n, replies, entries):
    """MerkleBuf's order: mk_roots, mk_leaves, mk_off, mk_hashes, mk_leafh, mk_nodeh, mk_fleafh, mk_fnodeh,
    mk_aroots, mk_paths, mv_leaves, mv_words, mv_roots, mv_proofs, mv_out, mp_*.  The host form stages the leaves
    where the extend does and the replies where the verify forms do; the lanes' hashes are kept in both forms; the
    new tree's entries, which the passes write, go to the front of mk_fnodeh."""
    mbytes, nodes, new = 100 * n, mc.node_span(old, n), 32 * 63
    for wl in (0, 1):
        for wn in (0, 1):
            for wr in (0, 1):
                host = _needs(old, n, mbytes, replies, entries, 1, wl, wn, wr)
                dev = _needs(old, n, mbytes, replies, entries, 0, wl, wn, wr)
                ext = _extend_needs(old, n, mbytes, 1, 1, 1)
                out_bytes = (32 * replies if wr else 0) + replies
                assert host[:6] == ext[:6] and host[0] == dev[0]
                assert host[4] == 32 * n and host[5] == 32 * nodes            # kept whether wanted or not
                assert host[6:10] == [0, new, 0, 0] and host[10] == 0
                assert host[11:15] == [8 * (2 * replies + 1), 32, 32 * max(entries, 1), out_bytes]
                assert dev[1:6] == [0] * 5 and dev[8:] == [0] * 12
                assert dev[6] == (0 if wl else 32 * n) and dev[7] == new + (0 if wn else 32 * nodes)
                assert host[15:] == [0] * 5


# ---- the Python host route against the loop it replaces
def _replies(case):
    return [(list(part), list(proof)) for part, proof in zip(case.parts, case.proofs)]


def _ledger_at(case):
    led = Ledger(transactionLog=cc._LEAVES[:case.old], on_device=False)
    assert led.size == case.old and list(led.tree.hashes) == case.old_hashes
    return led


def _loop(led, case):
    """What exists without the new call: per reply verify_catchup_txns, then add per transaction; stop at the
    first reply that fails.  Returns the replies applied."""
    count = 0
    for txns, proof in _replies(case):
        if not led.verify_catchup_txns(txns, case.final_size, case.final_root, proof):
            break
        for t in txns:
            led.add(t)
        count += 1
    return count


def _same_ledger(a, b):
    assert a.size == b.size and a.root_hash == b.root_hash and a.tree.hashes == b.tree.hashes
    assert cc.store_bytes(a.tree) == cc.store_bytes(b.tree)
    assert a._transactionLog == b._transactionLog and a.seqNo == b.seqNo


def test_apply_catchup_replies_equals_the_loop():
    for c in REAL:
        a, b = _ledger_at(c), _ledger_at(c)
        count = _loop(a, c)
        res = b.applyCatchupReplies(_replies(c), c.final_size, c.final_root)
        x = cc.model(c)
        assert isinstance(res, merkle.CatchupResult)
        assert res.accepted == count == x.accepted and res.accepted_leaves == x.accepted_leaves, c.name
        assert list(res.status) == list(x.status) and res.roots.tobytes() == b"".join(x.roots), c.name
        _same_ledger(a, b)
        assert b.size == x.size and list(b.tree.hashes) == x.hashes


def test_apply_catchup_replies_takes_base58():
    c = THREE
    a, b = _ledger_at(c), _ledger_at(c)
    reps = [(t, [Ledger.hashToStr(h) for h in p]) for t, p in _replies(c)]
    res = a.applyCatchupReplies(reps, c.final_size, Ledger.hashToStr(c.final_root))
    b.applyCatchupReplies(_replies(c), c.final_size, c.final_root)
    assert res.ok and res.accepted == 3
    _same_ledger(a, b)


def test_extend_verified_host_on_every_case():
    for c in CASES:
        cc.check_extend_verified(c, False)


def test_max_call_splits_at_part_boundaries_host():
    cc.check_max_call_split(False)


def test_extend_verified_checks_its_arguments():
    c, t = THREE, cc.tree_at(THREE)
    with pytest.raises(ValueError):
        t.extend_verified(c.parts, c.final_size, c.final_root, c.proofs[:2], on_device=False)
    with pytest.raises(ValueError):
        t.extend_verified(c.parts, c.final_size, c.final_root[:31], c.proofs, on_device=False)
    with pytest.raises(ValueError):
        t.extend_verified(c.parts, 2 ** 64, c.final_root, c.proofs, on_device=False)
    assert t.tree_size == c.old
    assert merkle.MIN_DEVICE_CATCHUP_LEAVES >= 1
    empty = t.extend_verified([], c.final_size, c.final_root, [], on_device=False)
    assert len(empty) == 0 and empty.accepted == 0 and empty.ok and empty.roots.shape == (0, 32)


# ---- the C ABI's argument checks
def test_library_rejects_bad_arguments_before_any_device():
    """Every EDV_E_ARG case of edv_merkle_catchup returns ahead of any device lookup and writes nothing."""
    lib, c = edv.lib(), THREE
    a = cc.HostArgs(c)
    outs = [cc.guarded(32 * a.n), cc.guarded(32 * a.nodes), cc.guarded(32 * a.replies), cc.guarded(a.replies)]
    good = dict(old_size=c.old, old=a.old.ctypes.data, leaves=a.blob.ctypes.data, off=a.off.ctypes.data, n=a.n,
                ends=a.ends.ctypes.data, replies=a.replies, final_size=c.final_size, root=a.root.ctypes.data,
                proofs=a.proofs.ctypes.data, poff=a.poff.ctypes.data, status=outs[3].ctypes.data)

    def call(**kw):
        k = dict(good, **kw)
        return lib.edv_merkle_catchup(k["old_size"], k["old"], k["leaves"], k["off"], k["n"], k["ends"], k["replies"],
                                      k["final_size"], k["root"], k["proofs"], k["poff"], outs[0].ctypes.data,
                                      outs[1].ctypes.data, outs[2].ctypes.data, k["status"], 0)

    bad_off, bad_ends, short_ends = a.off.copy(), a.ends.copy(), a.ends.copy()
    bad_off[2] = bad_off[1] - 1
    bad_ends[0] = bad_ends[1] + 1
    short_ends[-1] -= 1
    bad_poff = a.poff.copy()
    bad_poff[1] = bad_poff[2] + 1
    many = np.full(a.n + 2, a.n, np.uint64)
    many_poff = np.zeros(a.n + 3, np.uint64)
    cases = [dict(n=edv.MERKLE_MAX_LEAVES + 1), dict(old_size=2 ** 62 + 1), dict(old_size=2 ** 62 - 1),
             dict(old=None), dict(off=None), dict(off=bad_off.ctypes.data), dict(leaves=None),
             dict(replies=0), dict(replies=a.n + 2, ends=many.ctypes.data, poff=many_poff.ctypes.data),
             dict(ends=bad_ends.ctypes.data), dict(ends=short_ends.ctypes.data), dict(poff=bad_poff.ctypes.data),
             dict(root=None), dict(status=None), dict(ends=None), dict(poff=None)]
    for kw in cases:
        assert call(**kw) == edv.EDV_E_ARG, kw
        assert edv.lib().edv_last_error()
    for o in outs:
        assert o.tobytes() == bytes([cc.SENTINEL]) * len(o)
