"""Batched proof generation (row f-8) without a GPU: the checker against the
reference's recorded proofs, the header's lane functions on the CPU
(hc_merkle_prove_*) against the checker byte for byte, the positions function
at sizes no store can have, the offset helpers and the host plan, and the host
route of the Python API against the loops of single calls."""
import ctypes
import hashlib
import os
import random
import re
import subprocess

import numpy as np
import pytest

import merkle_cases as mc
import merkle_prove_cases as pc
import merkle_verify_cases as vc
from indy_plenum_amd import edv, merkle
from indy_plenum_amd.ledger import Ledger

G = pc.load_golden()
LH, LEAFS, NODES = pc.golden_store()
TREE = pc.Tree(LH)
SIZES = list(range(1, 66)) + pc.LARGE


# ---- the checker against the reference's recorded results
def test_checker_reproduces_every_recorded_digest():
    assert [r["n"] for r in G["all_pairs"]] == SIZES
    for r in G["all_pairs"]:
        n = r["n"]
        inc = [TREE.inclusion(m, n) for m in range(n)]
        con = [TREE.consistency(a, n) for a in range(1, n + 1)]
        assert pc.digest(inc) == r["inclusion_sha256"], n
        assert pc.digest(con) == r["consistency_sha256"], n
        assert sum(map(len, inc)) == r["inclusion_entries"] and sum(map(len, con)) == r["consistency_entries"]
    info = G["merkle_info"]
    roots = [TREE.root(s) for s in range(1, 1001)]
    paths = [TREE.inclusion(s - 1, s) for s in range(1, 1001)]
    assert [hashlib.sha256(r + b"".join(p)).hexdigest() for r, p in zip(roots, paths)] == info["per_seq_no_sha256"]
    assert hashlib.sha256(b"".join(roots)).hexdigest() == info["roots_sha256"]
    assert pc.digest(paths) == info["paths_sha256"]


def test_checker_reproduces_the_full_proofs():
    assert len(G["full"]["inclusion"]) + len(G["full"]["consistency"]) >= 40
    for c in G["full"]["inclusion"]:
        assert [h.hex() for h in TREE.inclusion(c["m"], c["n"])] == c["proof"]
        assert TREE.root(c["n"]).hex() == c["root"]
        assert mc.verify_inclusion(LH[c["m"]], c["m"], c["n"], TREE.inclusion(c["m"], c["n"]), TREE.root(c["n"]))
    for c in G["full"]["consistency"]:
        assert [h.hex() for h in TREE.consistency(c["a"], c["b"])] == c["proof"]
        assert (TREE.root(c["a"]).hex(), TREE.root(c["b"]).hex()) == (c["root_a"], c["root_b"])


def test_store_is_the_reference_store():
    g = mc.load_golden()["cases"][-1]
    assert g["size"] == 1000
    assert hashlib.sha256(LEAFS).hexdigest() == g["leaf_store_sha256"]
    assert hashlib.sha256(NODES).hexdigest() == g["node_store_sha256"]


# ---- lengths
def test_lengths():
    hc = pc.hostcheck()
    rng = random.Random(8)
    pairs = [(m, n) for n in range(1, 130) for m in range(n)]
    pairs += [(rng.randrange(n), n) for n in pc.big_sizes() for _ in range(40)]
    pairs += [(i, n) for n in pc.big_sizes() for i in pc.big_indices(n)]
    for m, n in pairs:
        assert hc.hc_merkle_inclusion_length(m, n) == merkle.MerkleVerifier.audit_path_length(m, n), (m, n)
        if m >= 1:
            assert hc.hc_merkle_consistency_length(m, n) == vc.consistency_length(m, n), (m, n)
    for n in (1, 2, 7, 2 ** 62):
        assert hc.hc_merkle_consistency_length(n, n) == 0
    assert max(hc.hc_merkle_inclusion_length(m, 2 ** 62) for m in (0, 2 ** 62 - 1)) == 62
    assert hc.hc_merkle_inclusion_length(0, 2 ** 62 - 1) == 62
    assert max(hc.hc_merkle_consistency_length(a, 2 ** 62 - 1) for a in range(2 ** 62 - 200, 2 ** 62 - 1)) <= pc.MAX_PROOF
    for n in range(1, 130):
        for m in range(n):
            assert len(pc.path_ranges(m, 0, n)) == hc.hc_merkle_inclusion_length(m, n)
            assert len(pc.subproof_ranges(m + 1, 0, n, True)) == hc.hc_merkle_consistency_length(m + 1, n)


# ---- positions
def check_positions(consistency, a, n):
    want, got = pc.positions(consistency, a, n), pc.hc_positions(consistency, a, n)
    assert len(want) == len(got), (consistency, a, n)
    folds = 0
    for (wk, wv), (gk, gv) in zip(want, got):
        assert wk == gk, (consistency, a, n)
        if wk == pc.KIND_FOLD:
            # the height of the cut-off sibling: the range starts at (n >> h) << h
            folds += 1
            assert 0 < gv <= 62 and (n >> gv) << gv == wv and wv < n, (consistency, a, n)
        else:
            assert gv == wv % 2 ** 64, (consistency, a, n, wv, gv)   # byte offsets as 64-bit integers
    assert folds <= 1
    return got


def test_positions_small():
    for n in range(1, 131):
        for m in range(n):
            check_positions(False, m, n)
            check_positions(True, m + 1, n)


def test_positions_at_sizes_no_store_has():
    top = 0
    for n in pc.big_sizes():
        for i in pc.big_indices(n):
            got = check_positions(False, i, n)
            top = max([top] + [v for k, v in got if k != pc.KIND_FOLD])
            if i >= 1:
                check_positions(True, i, n)
        check_positions(True, n, n)
    assert top > 2 ** 63   # byte offsets far above 2^32 went through whole


def test_positions_stay_inside_the_store():
    """Every position of a proof in the tree of n leaves is below the counts of a store of n leaves."""
    rng = random.Random(3)
    sizes = list(range(1, 70)) + [rng.randrange(1, 2 ** 58) for _ in range(60)] + pc.big_sizes()[:4]   # 32 n < 2^64
    for n in sizes:
        nodes = n - mc.popcount(n)
        for i in ([0, n // 2, n - 1] if n > 70 else range(n)):
            for cons, a in ((False, i), (True, i + 1)):
                for kind, v in pc.hc_positions(cons, a, n):
                    if kind == pc.KIND_LEAF:
                        assert v % 32 == 0 and v // 32 < n
                    elif kind == pc.KIND_NODE:
                        assert v % 32 == 0 and v // 32 < nodes


# ---- the lanes against the checker
def run_both(consistency, store_leaves, pairs, off=None, **kw):
    off = pc.exact_offsets(consistency, pairs, store_leaves) if off is None else off
    got = pc.hc_prove(consistency, store_leaves, pairs, off, **kw)
    want = pc.expected(TREE, consistency, pairs, store_leaves, off)
    assert got[0] == want[0]
    assert got[1] == want[1]
    if got[2] is not None:
        assert got[2] == want[2]
    if got[3] is not None:
        assert got[3] == want[3]
    return got


@pytest.mark.parametrize("consistency", [False, True])
def test_lanes_all_pairs_small(consistency):
    pairs = [p for n in range(1, 66) for p in pc.all_pairs(n, consistency)]
    assert len(pairs) == 2145
    st, slots, _, _ = run_both(consistency, 1000, pairs)
    assert set(st) == {pc.OK}
    off = pc.exact_offsets(consistency, pairs, 1000)
    at = 0
    for r in G["all_pairs"][:65]:   # ... and the reference's digests, size by size
        lo, hi = 32 * int(off[at]), 32 * int(off[at + r["n"]])
        key = "consistency_sha256" if consistency else "inclusion_sha256"
        assert hashlib.sha256(slots[lo:hi]).hexdigest() == r[key], r["n"]
        at += r["n"]


@pytest.mark.parametrize("consistency", [False, True])
@pytest.mark.parametrize("n", pc.LARGE)
def test_lanes_all_pairs_large(consistency, n):
    # the store is exactly the tree: a read past either count is outside the harness's blocks
    st, slots, _, _ = run_both(consistency, n, pc.all_pairs(n, consistency))
    assert set(st) == {pc.OK}
    r = next(r for r in G["all_pairs"] if r["n"] == n)
    assert hashlib.sha256(slots).hexdigest() == r["consistency_sha256" if consistency else "inclusion_sha256"]


@pytest.mark.parametrize("consistency", [False, True])
def test_lanes_range_space_and_optional_outputs(consistency):
    for store in (0, 1, 11, 1000):
        pairs = pc.range_cases(consistency, store)
        st, *_ = run_both(consistency, store, pairs)
        assert set(st) == {pc.RANGE}
    pairs, off, short, long_ = pc.one_wave(consistency, 1000)
    st, *_ = run_both(consistency, 1000, pairs, off)
    assert st[short] == pc.SPACE and st[long_] == pc.SPACE
    assert sorted(set(st)) == [pc.OK, pc.RANGE, pc.SPACE]
    for want1, want2 in ((False, False), (True, False), (False, True)):
        run_both(consistency, 1000, pairs, off, want1=want1, want2=want2)


def test_lanes_empty_call_and_bad_arguments():
    hc = pc.hostcheck()
    z = np.zeros(4, np.uint64)
    assert hc.hc_merkle_prove_inclusion(None, None, 0, None, None, None, 0, None, None, None, None) == 0
    dec = np.array([2, 1], np.uint64)
    b = np.zeros(64, np.uint8)
    assert hc.hc_merkle_prove_inclusion(None, None, 0, z.ctypes.data, z.ctypes.data, dec.ctypes.data, 1, b.ctypes.data,
                                        b.ctypes.data, None, None) == -1
    assert hc.hc_merkle_prove_consistency(None, None, 2 ** 62 + 1, z.ctypes.data, z.ctypes.data, z.ctypes.data, 1,
                                          b.ctypes.data, b.ctypes.data, None, None) == -1


# ---- offsets and the host plan
@pytest.mark.parametrize("consistency", [False, True])
def test_offset_helpers(consistency):
    rng = random.Random(11)
    pairs = pc.all_pairs(33, consistency) + pc.range_cases(consistency, 1000) + \
        [(rng.randrange(1, 1000), rng.randrange(1, 1001)) for _ in range(200)] + pc.all_pairs(1, consistency)
    for store in (1000, 40):
        want = pc.exact_offsets(consistency, pairs, store)
        assert pc.hc_offsets(consistency, pairs, store).tolist() == want.tolist()
        a, b = pc.u64(p[0] for p in pairs), pc.u64(p[1] for p in pairs)
        if os.path.exists(edv.LIB_PATH):   # the C-ABI's helper: no device is touched
            fn = edv.merkle_consistency_offsets if consistency else edv.merkle_inclusion_offsets
            assert fn(a, b, store).tolist() == want.tolist()
    assert pc.hc_offsets(consistency, [], 5).tolist() == [0]


def test_host_plan():
    hc = pc.hostcheck()
    consts = (ctypes.c_int32 * 3)()
    hc.hc_merkle_prove_consts(consts)
    assert consts[0] == edv.PROOF_SPACE == pc.SPACE and consts[1] == pc.MAX_PROOF and consts[2] == 20
    names = ["mp_leaves", "mp_nodes", "mp_words", "mp_proofs", "mp_out"]

    def needs(n, prefix, entries, w1, w2):
        out = np.zeros(20, np.uint64)
        hc.hc_merkle_prove_needs(n, prefix, entries, w1, w2, out.ctypes.data)
        assert not out[:15].any()   # nothing of the earlier rows' buffers
        return dict(zip(names, (int(x) for x in out[15:])))

    for n, prefix, entries, w1, w2 in [(1, 1, 0, 0, 0), (64, 1000, 640, 1, 1), (10000, 2 ** 20 + 12345, 200000, 1, 0),
                                       (5, 0, 0, 1, 1)]:
        got = needs(n, prefix, entries, w1, w2)
        assert got["mp_leaves"] >= max(32 * prefix, 1) and got["mp_nodes"] >= max(32 * (prefix - mc.popcount(prefix)), 1)
        assert got["mp_words"] == 8 * (3 * n + 1) and got["mp_proofs"] >= max(32 * entries, 32)
        o = np.zeros(4, np.uint64)
        hc.hc_merkle_prove_out(n, w1, w2, o.ctypes.data)
        first, second, status, total = (int(x) for x in o)
        assert got["mp_out"] == total == status + n and status == 32 * n * (w1 + w2)
        assert (first, second) == (0, 32 * n * w1) and second % 16 == 0
    # the prefix is the largest valid tree size
    a, b = pc.u64([3, 9, 0, 5]), pc.u64([7, 9, 40, 2000])
    assert hc.hc_merkle_prove_prefix(0, a.ctypes.data, b.ctypes.data, 4, 1000) == 40
    assert hc.hc_merkle_prove_prefix(1, a.ctypes.data, b.ctypes.data, 4, 1000) == 9
    assert hc.hc_merkle_prove_prefix(0, a.ctypes.data, b.ctypes.data, 4, 8) == 7
    assert hc.hc_merkle_prove_prefix(1, a.ctypes.data, b.ctypes.data, 0, 8) == 0
    # the trim keeps what keep proofs of 64 entries need, nothing for 0, and leaves the earlier rows as they were
    for keep in (0, 1, 400, 10000):
        lim = np.zeros(20, np.uint64)
        old = np.zeros(15, np.uint64)
        hc.hc_merkle_trim_limits_all(keep, lim.ctypes.data)
        mc.hostcheck().hc_merkle_trim_limits.argtypes = [ctypes.c_uint64, ctypes.c_void_p]
        mc.hostcheck().hc_merkle_trim_limits(keep, old.ctypes.data)
        assert lim[:15].tolist() == old.tolist()
        if keep == 0:
            assert not lim[15:].any()
        else:
            need = needs(keep, 0, 64 * keep, 1, 1)
            for k, name in enumerate(names[2:], 17):
                assert int(lim[k]) >= need[name], (keep, name)


def test_header_constants_match_edv_py():
    hdr = open(os.path.join(mc.ROOT, "include", "edv.h")).read()
    defs = dict(re.findall(r"#define (EDV_PROOF_\w+) (\d+)", hdr))
    assert int(defs["EDV_PROOF_SPACE"]) == edv.PROOF_SPACE == 7
    for name, val in defs.items():
        assert getattr(edv, name[4:]) == int(val)
    for sym in ("edv_merkle_inclusion_offsets", "edv_merkle_consistency_offsets", "edv_merkle_prove_inclusion",
                "edv_merkle_prove_consistency", "edv_merkle_prove_inclusion_dev", "edv_merkle_prove_consistency_dev"):
        assert re.search(r"\bint %s\(" % sym, hdr), sym


# ---- the host route of the Python API
@pytest.fixture(scope="module")
def ledger():
    led = Ledger(tree=merkle.CompactMerkleTree(hashStore=merkle.DeviceHashStore()), on_device=False)
    for leaf in G["leaf_list"]:
        led.add(leaf)
    return led


def pairs_for_api(consistency):
    rng = random.Random(21)
    some = [p for n in (1, 2, 3, 11, 65) for p in pc.all_pairs(n, consistency)]
    return some + [((rng.randrange(1, n + 1) if consistency else rng.randrange(n)), n)
                   for n in (rng.randrange(1, 1001) for _ in range(150))]


def test_device_hash_store_without_a_device(ledger):
    store = ledger.tree.hashStore
    assert isinstance(store, merkle.MemoryHashStore) and store.device_bytes == 0 and store.bytes_uploaded == 0
    assert store.leafCount == 1000 and store.nodeCount == 1000 - mc.popcount(1000)
    assert b"".join(store.readLeafs(1, 1001)) == LEAFS and b"".join(store.readNodes(1, store.nodeCount + 1)) == NODES
    assert store.readLeaf(7) == LH[6]
    with pytest.raises(IndexError):
        store.readLeaf(1001)
    fresh = merkle.DeviceHashStore(device=3)
    fresh.writeLeaf(LH[0])
    assert fresh.leafCount == 1 and fresh.reset() and fresh.leafCount == 0 and fresh.device_bytes == 0


def test_inclusion_proof_batch_host(ledger):
    tree = ledger.tree
    pairs = pairs_for_api(False)
    batch = tree.inclusion_proof_batch(pairs, on_device=False)
    assert batch.kind == "inclusion" and len(batch) == len(pairs) and set(batch.status.tolist()) == {edv.PROOF_OK}
    assert [batch.proof(i) for i in range(len(pairs))] == list(batch) == [tree.inclusion_proof(m, n) for m, n in pairs]
    assert batch.roots.tobytes() == b"".join(tree.merkle_tree_hash(0, n) for _, n in pairs)
    assert batch.leaf_hashes.tobytes() == b"".join(LH[m] for m, _ in pairs)
    assert batch.off.tolist() == pc.exact_offsets(False, pairs, 1000).tolist()
    assert tree.inclusion_proof_batch(pairs, on_device=False, want_roots=False).roots is None
    assert len(tree.inclusion_proof_batch([])) == 0
    assert merkle.MerkleVerifier().verify_proof_batch(batch, on_device=False).ok.all()
    for c in G["full"]["inclusion"]:
        b1 = tree.inclusion_proof_batch([(c["m"], c["n"])])
        assert [h.hex() for h in b1.proof(0)] == c["proof"] and b1.roots[0].tobytes().hex() == c["root"]


def test_consistency_proof_batch_host(ledger):
    tree = ledger.tree
    pairs = pairs_for_api(True)
    batch = tree.consistency_proof_batch(pairs, on_device=False)
    assert list(batch) == [tree.consistency_proof(a, b) for a, b in pairs]
    assert batch.old_roots.tobytes() == b"".join(tree.merkle_tree_hash(0, a) for a, _ in pairs)
    assert batch.new_roots.tobytes() == b"".join(tree.merkle_tree_hash(0, b) for _, b in pairs)
    verdicts = merkle.MerkleVerifier().verify_proof_batch(batch, on_device=False, want_computed=True)
    assert verdicts.ok.all()
    # a proof of the batch altered: the verifier sees it
    batch.proofs = batch.proofs.copy()
    k = next(i for i in range(len(pairs)) if batch.off[i + 1] > batch.off[i])
    batch.proofs[int(batch.off[k]), 3] ^= 1
    assert merkle.MerkleVerifier().verify_proof_batch(batch, on_device=False).ok.tolist().count(False) == 1


def test_merkle_info_batch_and_ledger(ledger):
    seqs = list(range(1, 1001))
    batch = ledger.tree.merkle_info_batch(seqs, on_device=False)
    got = [hashlib.sha256(batch.roots[i].tobytes() + b"".join(p)).hexdigest() for i, p in enumerate(batch)]
    assert got == G["merkle_info"]["per_seq_no_sha256"]
    some = [1, 2, 3, 64, 65, 500, 777, 999, 1000, 65]
    assert ledger.merkleInfoBatch(some) == [ledger.merkleInfo(s) for s in some]
    raw = ledger.merkle_proofs(some)
    assert isinstance(raw, merkle.ProofBatch) and raw.index.tolist() == [s - 1 for s in some]
    cp = [(1, 1), (1, 1000), (512, 777), (999, 1000), (333, 333)]
    assert ledger.consistency_proofs(cp) == [
        {"proof": [ledger.hashToStr(h) for h in ledger.tree.consistency_proof(a, b)],
         "oldRootHash": ledger.hashToStr(ledger.tree.merkle_tree_hash(0, a)),
         "newRootHash": ledger.hashToStr(ledger.tree.merkle_tree_hash(0, b))} for a, b in cp]
    assert ledger.merkleInfoBatch([]) == []


def test_bad_pairs_raise_as_the_single_calls(ledger):
    tree = ledger.tree
    for bad, exc in (((0, 1001), IndexError), ((500, 1001), IndexError), ((0, 0), ValueError)):
        with pytest.raises(exc):
            tree.inclusion_proof(*bad)
        with pytest.raises(exc):
            tree.inclusion_proof_batch([(0, 5), bad, (1, 2)], on_device=False)
    # pairs for which no audit path is defined, or whose tree the store does not hold: the single call
    # answers some of them from the hashes it happens to find; the batch refuses them all
    for bad in ((5, 5), (6, 5), (-1, 5), (0, 2 ** 64)):
        with pytest.raises(ValueError):
            tree.inclusion_proof_batch([bad], on_device=False)
    with pytest.raises(IndexError):
        tree.inclusion_proof_batch([(1000, 1001)], on_device=False)
    for bad, exc in (((0, 5), ValueError), ((1, 1001), IndexError), ((7, 1001), IndexError)):
        with pytest.raises(exc):
            tree.consistency_proof(*bad)
        with pytest.raises(exc):
            tree.consistency_proof_batch([(1, 1), bad], on_device=False)
    with pytest.raises(IndexError):
        tree.consistency_proof_batch([(1001, 1001)], on_device=False)
    with pytest.raises(ValueError):
        tree.consistency_proof_batch([(6, 5)], on_device=False)
    for s in (0, -3):
        with pytest.raises(ValueError):
            ledger.merkleInfo(s)
        with pytest.raises(ValueError):
            ledger.merkleInfoBatch([1, s])
    with pytest.raises(IndexError):
        ledger.merkleInfo(1001)
    with pytest.raises(IndexError):
        ledger.merkleInfoBatch([1001])


def test_routing_defaults(ledger):
    tree = ledger.tree
    assert tree._prove_route(merkle.MIN_DEVICE_PROVE_PROOFS - 1, None) == "host"
    assert tree._prove_route(10 ** 6, False) == "host"
    assert tree._prove_route(1, True) == "store"
    plain = merkle.CompactMerkleTree()
    assert plain._prove_route(10 ** 6, None) == "host" and plain._prove_route(1, True) == "copy"
    other = merkle.CompactMerkleTree(hasher=merkle.TreeHasher(hashlib.sha512), hashStore=merkle.DeviceHashStore())
    with pytest.raises(ValueError):
        other._prove_route(1, True)


# ---- the sanitizer program
def test_asan_program():
    out = subprocess.run(["bash", os.path.join(mc.ROOT, "tools", "asan_merkle_prove.sh")], capture_output=True, text=True,
                         env=dict(os.environ, ASAN_OUT=os.path.join("/tmp", "edv_asan_prove_%d" % os.getpid())))
    assert out.returncode == 0, out.stdout + out.stderr
    assert "asan_merkle_prove ok" in out.stdout
