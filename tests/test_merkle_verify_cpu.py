"""Batched proof verification without a GPU (row f-7): the checker of
tests/merkle_verify_cases.py against the recursive RFC 6962 forms, the recorded
proofs and the reference's recorded outcomes; the kernels' header code on the
CPU (hc_merkle_verify_inclusion / hc_merkle_verify_consistency) against the
checker over the grids; MerkleVerifier's host route, the Ledger's two checks;
and the ASan / UBSan program."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import merkle_cases as mc
import merkle_verify_cases as vc
from indy_plenum_amd import Ledger, MerkleVerifier, STH, edv, merkle, verify_merkle_proofs
from indy_plenum_amd import ledger as ledger_mod


@pytest.fixture(scope="module")
def golden():
    return vc.golden_batches(vc.load_golden())


@pytest.fixture(scope="module")
def trees():
    return mc.load_golden()


# ---- the checker
def test_checker_against_the_recursive_forms_and_the_recorded_proofs(trees):
    leaves = trees["leaves"]
    t = merkle.CompactMerkleTree()
    t.extend(leaves, on_device=False)
    count = 0
    for case in trees["cases"]:
        for p in case["inclusion"]:
            proof = [bytes.fromhex(h) for h in p["proof"]]
            lh, root = mc.leaf_hash(leaves[p["m"]]), t.merkle_tree_hash(0, p["n"])
            assert vc.check_inclusion(lh, p["m"], p["n"], proof, root) == (vc.OK, root)
            assert len(proof) == vc.path_length(p["m"], p["n"]) == MerkleVerifier.audit_path_length(p["m"], p["n"])
            count += 1
        for p in case["consistency"]:
            proof = [bytes.fromhex(h) for h in p["proof"]]
            ra, rb = bytes.fromhex(p["root_a"]), bytes.fromhex(p["root_b"])
            st, comp = vc.check_consistency(p["a"], p["b"], ra, rb, proof)
            assert st == vc.OK and comp == (vc.ZERO * 2 if p["a"] == p["b"] else ra + rb)
            if p["a"] < p["b"]:
                assert len(proof) == vc.consistency_length(p["a"], p["b"])
            count += 1
    assert count > 60
    # every small tree, every leaf and every pair, proofs from the package's tree: the two formulations agree,
    # on good proofs and on broken ones
    for n in range(1, 20):
        root_n = t.merkle_tree_hash(0, n)
        for m in range(n):
            proof = t.inclusion_proof(m, n)
            lh = mc.leaf_hash(leaves[m])
            for pr, root in ((proof, root_n), (proof[:-1], root_n), (proof + [vc.JUNK], root_n), (proof, vc.JUNK)):
                st, _ = vc.check_inclusion(lh, m, n, pr, root)
                assert (st == vc.OK) == bool(mc.verify_inclusion(lh, m, n, pr, root))
        for m in range(1, n):
            proof = t.consistency_proof(m, n)
            root_m = t.merkle_tree_hash(0, m)
            for pr, ra, rb in ((proof, root_m, root_n), (proof[:-1], root_m, root_n), (proof, vc.JUNK, root_n),
                               (proof, root_m, vc.JUNK)):
                st, _ = vc.check_consistency(m, n, ra, rb, pr)
                assert (st == vc.OK) == bool(mc.verify_consistency(m, n, ra, rb, pr))


def test_checker_against_the_reference_outcomes(golden):
    inc, inc_st, con, con_st = golden
    assert inc.expected()[0] == inc_st
    assert con.expected()[0] == con_st
    assert set(inc_st) == {vc.OK, vc.RANGE, vc.SHORT, vc.LONG, vc.ROOT}
    assert set(con_st) == {vc.OK, vc.RANGE, vc.SHORT, vc.ROOT, vc.INCONSISTENT}


def test_the_outcomes_the_issue_names():
    lh, e = mc.leaf_hash(b"x"), vc.JUNK
    assert vc.check_inclusion(lh, 0, 1, [e], lh)[0] == vc.LONG
    assert vc.check_inclusion(lh, 1, 2, [], lh)[0] == vc.SHORT
    assert vc.check_inclusion(lh, 2, 2, [e], lh)[0] == vc.RANGE
    assert vc.check_inclusion(lh, 0, 0, [], lh)[0] == vc.RANGE
    assert vc.check_consistency(3, 3, lh, lh, [e])[0] == vc.OK
    assert vc.check_consistency(3, 3, lh, e, [e])[0] == vc.INCONSISTENT
    assert vc.check_consistency(0, 5, lh, e, [e])[0] == vc.OK
    assert vc.check_consistency(5, 3, lh, e, [e])[0] == vc.RANGE
    assert vc.check_consistency(2, 3, lh, e, [])[0] == vc.SHORT


def test_the_grids_cover_what_they_should():
    pts = vc.inclusion_points()
    lengths = {vc.path_length(i, s) for i, s in pts}
    assert {0, 1, 2, 3, 8, 9, 32, 33, 62, 64} <= lengths and max(lengths) == 64
    assert (2 ** 64 - 2, 2 ** 64 - 1) in pts and (256, 257) in pts      # the no-sibling leaf, one level and many
    assert vc.path_length(256, 257) == 1 and vc.path_length(2 ** 32, 2 ** 32 + 1) == 1
    b = vc.synth_inclusion(vc.interleaved_inclusion_points())
    assert set(b.expected()[0]) == {vc.OK, vc.RANGE, vc.SHORT, vc.LONG, vc.ROOT}
    c = vc.synth_consistency(vc.consistency_points())
    assert set(c.expected()[0]) == {vc.OK, vc.RANGE, vc.SHORT, vc.ROOT, vc.INCONSISTENT}
    assert len(set(c.expected()[0][:64])) == 5 and len(set(b.expected()[0][:64])) == 5   # one wave carries them all
    assert max(vc.consistency_length(a, n) for a, n in vc.consistency_points()) >= 64


# ---- the kernels' code on the CPU
@pytest.mark.parametrize("by_hash", [False, True])
def test_hostcheck_inclusion_over_the_grid(by_hash):
    b = vc.synth_inclusion(vc.inclusion_points(), seed=2)
    assert vc.hc_inclusion(b, by_hash=by_hash) == b.expected()
    good = vc.synth_inclusion(vc.inclusion_points(), seed=3, mutate=False)
    st, comp = vc.hc_inclusion(good, by_hash=by_hash)
    assert st == bytes([vc.OK]) * len(good) and comp == b"".join(good.root)
    assert vc.hc_inclusion(b, by_hash=by_hash, want_computed=False) == (b.expected()[0], None)


def test_hostcheck_consistency_over_the_grid():
    b = vc.synth_consistency(vc.consistency_points(), seed=2)
    assert vc.hc_consistency(b) == b.expected()
    good = vc.synth_consistency(vc.consistency_points(), seed=3, mutate=False)
    st, comp = vc.hc_consistency(good)
    assert st == bytes([vc.OK]) * len(good)
    assert comp == b"".join(o + n for o, n in zip(good.old_root, good.new_root))
    assert vc.hc_consistency(b, want_computed=False, proof_base=3) == (b.expected()[0], None)


@pytest.mark.parametrize("n", vc.BATCH_N)
def test_hostcheck_batch_counts_and_leaf_edges(n):
    pts = [vc.inclusion_points()[(5 * k) % 60] for k in range(n)]
    b = vc.synth_inclusion(pts, seed=n)
    for base in range(4):            # every misalignment of the leaf blob's start
        assert vc.hc_inclusion(b, leaf_base=base, proof_base=base) == b.expected()
    c = vc.synth_consistency([vc.consistency_points()[(3 * k) % 70] for k in range(n)], seed=n)
    assert vc.hc_consistency(c) == c.expected()


def test_hostcheck_golden(golden):
    inc, inc_st, con, con_st = golden
    assert vc.hc_inclusion(inc, by_hash=True) == (inc_st, inc.expected()[1])
    assert vc.hc_consistency(con) == (con_st, con.expected()[1])


def test_hostcheck_argument_errors():
    b = vc.synth_inclusion(vc.inclusion_points()[:5])
    lib = vc.hostcheck()
    blob, loff = mc.pack(b.leaves)
    proofs, poff = vc.pack_proofs(b.proof)
    lh, roots, idx, size = vc.pack_hashes(b.leaf_hashes()), vc.pack_hashes(b.root), vc.u64(b.index), vc.u64(b.size)
    st = np.full(5, vc.SENTINEL, np.uint8)
    p = vc._p

    def call(leaves=p(blob), off=p(loff), hashes=None, n=5, po=p(poff)):
        return lib.hc_merkle_verify_inclusion(leaves, off, hashes, p(idx), p(size), p(roots), p(proofs), po, n, p(st), None)
    bad = np.array([0, 3, 2, 4, 5, 6], np.uint64)
    assert call(hashes=p(lh)) == -1 and call(leaves=None, off=None) == -1 and call(off=None) == -1
    assert call(po=p(bad)) == -1 and call(off=p(bad)) == -1 and call(n=2 ** 22 + 1) == -1
    assert (st == vc.SENTINEL).all()
    assert call(n=0) == 0 and (st == vc.SENTINEL).all()
    assert call() == 0 and st.tobytes() == b.expected()[0]


# ---- the Python surface, host route
def _raises(fn, exc):
    with pytest.raises(exc):
        fn()


def test_single_calls_return_true_or_raise_the_reference_classes(golden):
    inc, inc_st, con, con_st = golden
    v = MerkleVerifier()
    want = {vc.RANGE: ValueError, vc.SHORT: merkle.ProofError, vc.LONG: merkle.ProofError, vc.ROOT: merkle.ProofError,
            vc.INCONSISTENT: merkle.ConsistencyError}
    assert issubclass(merkle.ProofError, merkle.VerifyError) and issubclass(merkle.ConsistencyError, merkle.VerifyError)
    for k in range(len(inc)):
        def call():
            return v.verify_leaf_hash_inclusion(inc.hashes[k], inc.index[k], inc.proof[k], STH(inc.size[k], inc.root[k]))
        if inc_st[k] == vc.OK:
            assert call() is True
        else:
            _raises(call, want[inc_st[k]])
    for k in range(len(con)):
        def call():
            return v.verify_tree_consistency(con.old[k], con.new[k], con.old_root[k], con.new_root[k], con.proof[k])
        if con_st[k] == vc.OK:
            assert call() is True
        else:
            _raises(call, want[con_st[k]])
    with pytest.raises(merkle.ProofError, match="too short"):
        v.verify_leaf_hash_inclusion(vc.JUNK, 1, [], STH(2, vc.JUNK))
    with pytest.raises(merkle.ProofError, match="too long"):
        v.verify_leaf_hash_inclusion(vc.JUNK, 0, [vc.JUNK], STH(1, vc.JUNK))
    leaf = b"a leaf"
    assert v.verify_leaf_inclusion(leaf, 0, [], STH(1, mc.leaf_hash(leaf))) is True
    assert STH(tree_size=1, sha256_root_hash=b"r") == (1, b"r")
    for i, s in vc.inclusion_points():
        assert v.audit_path_length(i, s) == vc.path_length(i, s)


def _check_verdicts(got, status, computed=None):
    assert isinstance(got, merkle.ProofVerdicts) and len(got) == len(status)
    assert got.status.dtype == np.uint8 and got.status.tobytes() == status
    assert got.ok.dtype == np.bool_ and list(got) == [s == vc.OK for s in status] == list(got.ok)
    if computed is not None:
        assert got.computed.tobytes() == computed
    else:
        assert got.computed is None


def test_batched_forms_on_the_host_route(golden):
    inc, inc_st, con, con_st = golden
    v = MerkleVerifier()
    sths = [STH(s, r) for s, r in zip(inc.size, inc.root)]
    got = v.verify_leaf_hash_inclusion_batch(inc.hashes, inc.index, inc.proof, sths, on_device=False, want_computed=True)
    _check_verdicts(got, inc_st, inc.expected()[1])
    items = list(zip(con.old, con.new, con.old_root, con.new_root, con.proof))
    _check_verdicts(v.verify_tree_consistency_batch(items, on_device=False, want_computed=True), con_st,
                    con.expected()[1])
    _check_verdicts(v.verify_tree_consistency_batch(items, on_device=False), con_st)
    b = vc.synth_inclusion(vc.inclusion_points(), seed=5)
    got = v.verify_leaf_inclusion_batch(b.leaves, b.index, b.proof, [STH(s, r) for s, r in zip(b.size, b.root)],
                                        on_device=False, want_computed=True)
    _check_verdicts(got, *b.expected())
    # raise_for raises what the single call raises
    want = {vc.RANGE: ValueError, vc.SHORT: merkle.ProofError, vc.LONG: merkle.ProofError, vc.ROOT: merkle.ProofError}
    for k, st in enumerate(b.expected()[0]):
        if st == vc.OK:
            assert got.raise_for(k) is True
        else:
            _raises(lambda: got.raise_for(k), want[st])
    _raises(lambda: merkle.ProofVerdicts([vc.INCONSISTENT]).raise_for(0), merkle.ConsistencyError)
    _raises(lambda: merkle.ProofVerdicts([vc.UNVERIFIED]).raise_for(0), merkle.VerifyError)
    # integers the C-ABI cannot carry: out of range on the host route as in the shim
    lh = mc.leaf_hash(b"")
    got = v.verify_leaf_hash_inclusion_batch([lh] * 3, [-1, 0, 2 ** 64], [[], [], []],
                                             [STH(1, lh), STH(1, lh), STH(2 ** 64 + 1, lh)], on_device=False)
    assert got.status.tobytes() == bytes([vc.RANGE, vc.OK, vc.RANGE])
    got = v.verify_tree_consistency_batch([(-1, 3, lh, lh, []), (2 ** 64, 2 ** 64, lh, lh, []), (3, 3, lh, lh, [])],
                                          on_device=False)
    assert got.status.tobytes() == bytes([vc.RANGE, vc.RANGE, vc.OK])
    _raises(lambda: v.verify_leaf_hash_inclusion_batch([lh], [0], [[b"short"]], [STH(1, lh)], on_device=False), ValueError)
    empty = v.verify_leaf_inclusion_batch([], [], [], [], on_device=False)
    assert len(empty) == 0 and list(empty) == [] and empty.raise_first() is True


def test_small_batches_stay_on_the_host_by_default(monkeypatch):
    def no_device(*a, **k):
        raise AssertionError("device route taken")
    monkeypatch.setattr(merkle.edv, "merkle_verify_inclusion", no_device)
    monkeypatch.setattr(merkle.edv, "merkle_verify_consistency", no_device)
    n = merkle.MIN_DEVICE_VERIFY_PROOFS - 1
    b = vc.synth_inclusion([vc.inclusion_points()[k % 60] for k in range(n)], mutate=False)
    v = MerkleVerifier()
    got = v.verify_leaf_inclusion_batch(b.leaves, b.index, b.proof, [STH(s, r) for s, r in zip(b.size, b.root)])
    assert got.ok.all() and len(got) == n
    c = vc.synth_consistency(vc.consistency_points()[:20], mutate=False)
    assert v.verify_tree_consistency_batch(zip(c.old, c.new, c.old_root, c.new_root, c.proof)).ok.all()


def test_audit_paths_of_append_are_in_the_verifiers_order(trees):
    """reversed(hashes), smallest subtree first, is the audit path lowest level first: confirmed on the
    recorded appends before verify_append_batch relies on it."""
    leaves = trees["leaves"]
    for case in trees["cases"]:
        for ap in case["audit_paths"]:
            s = ap["leaf"]
            t = merkle.CompactMerkleTree()
            t.extend(leaves[:s], on_device=False)
            path = [bytes.fromhex(h) for h in ap["path"]]
            assert vc.check_inclusion(mc.leaf_hash(leaves[s - 1]), s - 1, s, path, t.root_hash)[0] == vc.OK
            if len(path) > 1:
                assert vc.check_inclusion(mc.leaf_hash(leaves[s - 1]), s - 1, s, path[::-1], t.root_hash)[0] == vc.ROOT


def test_verify_append_batch_on_the_host_route(trees):
    leaves = trees["leaves"]
    for old in (0, 255, 700):
        t = merkle.CompactMerkleTree()
        t.extend(leaves[:old], on_device=False)
        batch = t.append_batch(leaves[old:], on_device=False)
        got = merkle.verify_append_batch(old, leaves[old:], batch, on_device=False)
        assert len(got) == 1000 - old and got.ok.all() and got.raise_first() is True
    # one altered path entry: exactly the proofs that hold it fail
    batch.paths = batch.paths.copy()
    row = merkle.popcount_prefix(700 + 200) - merkle.popcount_prefix(700)
    batch.paths[row, 7] ^= 1
    got = merkle.verify_append_batch(700, leaves[700:], batch, on_device=False)
    assert [k for k, ok in enumerate(got) if not ok] == [200] and got.status[200] == vc.ROOT
    with pytest.raises(ValueError):
        merkle.verify_append_batch(699, leaves[700:], batch, on_device=False)


def _committed(on_device=False):
    leaves = mc.load_golden()["leaves"]
    L = Ledger(serialize_for_tree=lambda txn: txn["payload"], on_device=on_device)
    txns = [{"payload": leaf} for leaf in leaves]
    L.appendTxns(txns)
    L.commitTxns(700)
    L.commitTxns(300)
    return L, [dict(t, seqNo=i + 1) for i, t in enumerate(txns)]


def test_ledger_verify_merkle_proofs_on_the_host_route():
    L, results = _committed()
    ser = L.serialize_for_tree
    assert verify_merkle_proofs(results, ser, on_device=False) is True
    assert ledger_mod.verify_merkle_proofs(results[:3], ser) is True and verify_merkle_proofs([], ser) is True
    bad = [dict(r) for r in results]
    bad[500]["auditPath"] = list(bad[500]["auditPath"])
    bad[500]["auditPath"][1] = bad[499]["auditPath"][0]
    with pytest.raises(merkle.ProofError):
        verify_merkle_proofs(bad, ser, on_device=False)
    bad = [dict(r) for r in results]
    bad[3]["seqNo"] = 0
    with pytest.raises(ValueError):
        verify_merkle_proofs(bad, ser, on_device=False)


def test_ledger_verify_catchup_txns_on_the_host_route():
    L, _ = _committed()
    leaves = mc.load_golden()["leaves"]
    proof = [Ledger.hashToStr(h) for h in L.tree.consistency_proof(800, 1000)]
    behind = Ledger(serialize_for_tree=lambda txn: txn["payload"], on_device=False)
    behind.appendTxns([{"payload": leaf} for leaf in leaves[:600]])
    behind.commitTxns(600)
    txns = [{"payload": leaf} for leaf in leaves[600:800]]
    assert behind.verify_catchup_txns(txns, 1000, L.root_hash, proof) is True
    assert behind.verify_catchup_txns(txns, 1000, Ledger.strToHash(L.root_hash), [Ledger.strToHash(p) for p in proof]) is True
    assert behind.size == 600                                   # the committed tree is left alone
    altered = [dict(t) for t in txns]
    altered[77]["payload"] = altered[77]["payload"] + b"!"
    assert behind.verify_catchup_txns(altered, 1000, L.root_hash, proof) is False
    assert behind.verify_catchup_txns(txns, 1000, L.root_hash, proof[:-1]) is False
    assert behind.verify_catchup_txns(txns, 700, L.root_hash, proof) is False     # 800 > 700: ValueError inside
    assert behind.verify_catchup_txns(txns, 1000, "not base58 0OIl", proof) is False


# ---- the sanitizer program
@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_asan_program_runs_clean(tmp_path):
    r = subprocess.run(["bash", os.path.join(mc.ROOT, "tools", "asan_merkle_verify.sh")], capture_output=True, text=True,
                       env=dict(os.environ, ASAN_OUT=str(tmp_path)), timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "asan_merkle_verify ok" in r.stdout


def test_status_constants_are_the_headers():
    hdr = open(os.path.join(mc.ROOT, "include", "edv.h")).read()
    for name, val in (("UNVERIFIED", 0), ("OK", 1), ("RANGE", 2), ("SHORT", 3), ("LONG", 4), ("ROOT", 5),
                      ("INCONSISTENT", 6)):
        assert "#define EDV_PROOF_%s %d" % (name, val) in hdr
        assert getattr(edv, "PROOF_" + name) == val == getattr(vc, name)
