"""Batched proof verification on the device (row f-7): edv_merkle_verify_inclusion
/ _consistency and their device-resident forms against the checker of
tests/merkle_verify_cases.py (statuses and calculated roots), the reference's
recorded outcomes through the kernels, the append kernel's proofs checked by
the verify kernel with no host copy between them, and the Python surface's
device route against its host route."""
import ctypes

import numpy as np
import pytest

import merkle_cases as mc
import merkle_verify_cases as vc
from indy_plenum_amd import Ledger, MerkleVerifier, STH, edv, merkle, verify_merkle_proofs

pytestmark = pytest.mark.gpu

SENTINEL = vc.SENTINEL
BIG = 2 ** 32 + 2 ** 20 + 24     # a base above 2^32: an offset cut to 32 bits loses it


class _HipStream:
    """A caller-owned HIP stream from the HIP runtime libedv.so uses."""
    _hip = None

    def __init__(self):
        if _HipStream._hip is None:
            _HipStream._hip = ctypes.CDLL("libamdhip64.so.7")
        self._s = ctypes.c_void_p()
        assert _HipStream._hip.hipStreamCreate(ctypes.byref(self._s)) == 0
        self.ptr = self._s.value

    def synchronize(self):
        assert _HipStream._hip.hipStreamSynchronize(self._s) == 0

    def __del__(self):
        if _HipStream._hip is not None and self._s:
            _HipStream._hip.hipStreamDestroy(self._s)


def _dev(host, extra=0):
    b = edv.DeviceBuffer(max(1, host.nbytes) + extra)
    if host.nbytes:
        b.upload(host)
    return b


def _guarded(nbytes):
    """A device buffer of nbytes + 32 sentinel bytes."""
    return _dev(np.full(nbytes + 32, SENTINEL, np.uint8))


class _Outputs:
    """status (n bytes) and computed (cbytes per proof), each followed by 32 sentinel bytes."""

    def __init__(self, n, cbytes, want_computed):
        self.n, self.cbytes, self.want = n, cbytes, want_computed
        self.status, self.computed = _guarded(n), _guarded(cbytes * n)

    def result(self):
        """(statuses, computed | None); the sentinels are intact and a NULL computed is untouched."""
        s, c = self.status.download().tobytes(), self.computed.download().tobytes()
        guard = bytes([SENTINEL]) * 32
        assert s[self.n:] == guard and c[self.cbytes * self.n:] == guard
        if not self.want:
            assert c == bytes([SENTINEL]) * len(c)
        return s[:self.n], (c[:self.cbytes * self.n] if self.want else None)

    def untouched(self):
        s, c = self.status.download().tobytes(), self.computed.download().tobytes()
        return s == bytes([SENTINEL]) * len(s) and c == bytes([SENTINEL]) * len(c)


class IncCall:
    """One edv_merkle_verify_inclusion_dev call's buffers.  leaf_base / proof_base are added to the offsets
    and handed to the call; misalign shifts the leaf blob's first byte inside its allocation."""

    def __init__(self, b, by_hash=False, want_computed=True, leaf_base=0, proof_base=0, misalign=0):
        self.n, self.by_hash, self.leaf_base, self.proof_base = len(b), by_hash, leaf_base, proof_base
        self.misalign = misalign
        if by_hash:
            self.d_lh = _dev(vc.pack_hashes(b.leaf_hashes()))
        else:
            blob, off = mc.pack(b.leaves)
            self.d_leaves = _dev(np.concatenate([np.zeros(misalign, np.uint8), blob]), extra=8)
            self.d_loff = _dev(off + np.uint64(leaf_base))
        proofs, poff = vc.pack_proofs(b.proof)
        self.d_proofs, self.d_poff = _dev(proofs), _dev(poff + np.uint64(proof_base))
        self.d_idx, self.d_size, self.d_roots = _dev(vc.u64(b.index)), _dev(vc.u64(b.size)), _dev(vc.pack_hashes(b.root))
        self.out = _Outputs(self.n, 32, want_computed)

    def args(self):
        leaf = dict(d_leaf_hashes=self.d_lh.ptr) if self.by_hash else dict(d_leaves=self.d_leaves.ptr + self.misalign,
                                                                          d_leaf_off=self.d_loff.ptr)
        return dict(leaf, d_leaf_index=self.d_idx.ptr, d_tree_size=self.d_size.ptr, d_roots=self.d_roots.ptr,
                    d_proofs=self.d_proofs.ptr, d_proof_off=self.d_poff.ptr, n=self.n, d_status=self.out.status.ptr,
                    d_computed=self.out.computed.ptr if self.out.want else None, leaf_base=self.leaf_base,
                    proof_base=self.proof_base)

    def run(self, stream=None):
        edv.merkle_verify_inclusion_device(stream=stream, **self.args())
        return self

    def result(self):
        return self.out.result()


class ConCall:
    def __init__(self, b, want_computed=True, proof_base=0):
        self.n, self.proof_base = len(b), proof_base
        proofs, poff = vc.pack_proofs(b.proof)
        self.d_proofs, self.d_poff = _dev(proofs), _dev(poff + np.uint64(proof_base))
        self.d_old, self.d_new = _dev(vc.u64(b.old)), _dev(vc.u64(b.new))
        self.d_ro, self.d_rn = _dev(vc.pack_hashes(b.old_root)), _dev(vc.pack_hashes(b.new_root))
        self.out = _Outputs(self.n, 64, want_computed)

    def args(self):
        return dict(d_old_size=self.d_old.ptr, d_new_size=self.d_new.ptr, d_old_roots=self.d_ro.ptr,
                    d_new_roots=self.d_rn.ptr, d_proofs=self.d_proofs.ptr, d_proof_off=self.d_poff.ptr, n=self.n,
                    d_status=self.out.status.ptr, d_computed=self.out.computed.ptr if self.out.want else None,
                    proof_base=self.proof_base)

    def run(self, stream=None):
        edv.merkle_verify_consistency_device(stream=stream, **self.args())
        return self

    def result(self):
        return self.out.result()


def host_inclusion(b, by_hash=False, want_computed=True):
    proofs, poff = vc.pack_proofs(b.proof)
    if by_hash:
        kw = dict(leaf_hashes=vc.pack_hashes(b.leaf_hashes()))
    else:
        blob, off = mc.pack(b.leaves)
        kw = dict(leaves=np.concatenate([blob, np.zeros(8, np.uint8)]), leaf_off=off)
    st, comp = edv.merkle_verify_inclusion(vc.u64(b.index), vc.u64(b.size), vc.pack_hashes(b.root), proofs, poff,
                                           want_computed=want_computed, **kw)
    return st.tobytes(), None if comp is None else comp.tobytes()


def host_consistency(b, want_computed=True):
    proofs, poff = vc.pack_proofs(b.proof)
    st, comp = edv.merkle_verify_consistency(vc.u64(b.old), vc.u64(b.new), vc.pack_hashes(b.old_root),
                                             vc.pack_hashes(b.new_root), proofs, poff, want_computed=want_computed)
    return st.tobytes(), None if comp is None else comp.tobytes()


@pytest.fixture(scope="module")
def grid():
    """The two grids, mutated and intact, with what the checker says of them (computed once)."""
    inc = vc.synth_inclusion(vc.inclusion_points(), seed=11)
    good = vc.synth_inclusion(vc.inclusion_points(), seed=12, mutate=False)
    con = vc.synth_consistency(vc.consistency_points(), seed=11)
    cgood = vc.synth_consistency(vc.consistency_points(), seed=12, mutate=False)
    return {"inc": (inc, inc.expected()), "good": (good, good.expected()), "con": (con, con.expected()),
            "cgood": (cgood, cgood.expected())}


@pytest.fixture(scope="module")
def golden():
    return vc.golden_batches(vc.load_golden())


@pytest.mark.parametrize("by_hash", [False, True])
def test_inclusion_both_entry_points_over_the_grid(grid, by_hash):
    for key in ("inc", "good"):
        b, exp = grid[key]
        assert IncCall(b, by_hash).run().result() == exp
        assert host_inclusion(b, by_hash) == exp
    b, exp = grid["good"]
    assert exp == (bytes([vc.OK]) * len(b), b"".join(b.root))
    b, exp = grid["inc"]
    assert IncCall(b, by_hash, want_computed=False).run().result() == (exp[0], None)
    assert host_inclusion(b, by_hash, want_computed=False) == (exp[0], None)


def test_consistency_both_entry_points_over_the_grid(grid):
    for key in ("con", "cgood"):
        b, exp = grid[key]
        assert ConCall(b).run().result() == exp
        assert host_consistency(b) == exp
    b, exp = grid["cgood"]
    assert exp[0] == bytes([vc.OK]) * len(b)
    b, exp = grid["con"]
    assert ConCall(b, want_computed=False).run().result() == (exp[0], None)
    assert host_consistency(b, want_computed=False) == (exp[0], None)


@pytest.mark.parametrize("n", vc.BATCH_N)
def test_batch_counts_leaf_edges_and_misalignment(n):
    """Wave and workgroup boundaries, the SHA-256 padding edges of the leaves, every misalignment of the blob."""
    b = vc.synth_inclusion([vc.inclusion_points()[(5 * k) % 60] for k in range(n)], seed=n)
    exp = b.expected()
    for mis in range(4):
        c = IncCall(b, misalign=mis).run()
        assert c.result() == exp
        if n == 0:
            assert c.out.untouched()
    assert host_inclusion(b) == exp
    c = vc.synth_consistency([vc.consistency_points()[(3 * k) % 70] for k in range(n)], seed=n)
    call = ConCall(c).run()
    assert call.result() == c.expected() and host_consistency(c) == c.expected()
    if n == 0:
        assert call.out.untouched()


def test_one_wave_carries_every_status():
    """64 proofs, one wave: OK, RANGE, SHORT, LONG and ROOT interleaved with walks of 0 to 64 levels side by
    side; and the consistency kernel's five likewise.  Divergence both ways: lanes that leave early beside
    lanes that walk on."""
    b = vc.synth_inclusion(vc.interleaved_inclusion_points(64), seed=21)
    exp = b.expected()
    assert set(exp[0]) == {vc.OK, vc.RANGE, vc.SHORT, vc.LONG, vc.ROOT}
    assert IncCall(b).run().result() == exp and IncCall(b, by_hash=True).run().result() == exp
    c = vc.synth_consistency(vc.consistency_points()[:64], seed=21)
    exp = c.expected()
    assert set(exp[0]) == {vc.OK, vc.RANGE, vc.SHORT, vc.ROOT, vc.INCONSISTENT}
    assert ConCall(c).run().result() == exp


def test_ten_thousand_proofs():
    pts = vc.inclusion_points()
    b = vc.synth_inclusion([pts[(k * 13) % len(pts)] for k in range(10000)], seed=31, lengths=[0, 1, 55, 56, 119, 120])
    exp = b.expected()
    assert IncCall(b).run().result() == exp
    assert host_inclusion(b, by_hash=True) == exp
    cp = vc.consistency_points()
    c = vc.synth_consistency([cp[(k * 7) % len(cp)] for k in range(10000)], seed=31)
    assert ConCall(c).run().result() == c.expected()


def test_reference_outcomes_through_the_device(golden):
    inc, inc_st, con, con_st = golden
    assert IncCall(inc, by_hash=True).run().result() == (inc_st, inc.expected()[1])
    assert host_inclusion(inc, by_hash=True)[0] == inc_st
    assert ConCall(con).run().result() == (con_st, con.expected()[1])
    assert host_consistency(con)[0] == con_st


def test_bases_above_2_32(grid):
    """Offsets that are absolute into a buffer far larger than 4 GiB: truncating one to 32 bits loses the base."""
    b, exp = grid["inc"]
    assert IncCall(b, leaf_base=BIG, proof_base=BIG + 8).run().result() == exp
    assert IncCall(b, by_hash=True, proof_base=2 ** 40 + 3).run().result() == exp
    c, cexp = grid["con"]
    assert ConCall(c, proof_base=BIG).run().result() == cexp


@pytest.mark.parametrize("old", [0, 255, 2 ** 32 - 1])
def test_round_trip_on_the_device(old):
    """edv_merkle_append_batch_dev's roots, audit paths and leaf hashes go straight into
    edv_merkle_verify_inclusion_dev: no host copy of the proofs."""
    n = 513
    fr = mc.frontier(old & 0xFFFF, old)
    leaves = mc.leaves_of(41, n, max_len=100)
    blob, off = mc.pack(leaves)
    entries = edv.merkle_path_entries(old, n)
    d_leaves, d_off = _dev(blob, extra=8), _dev(off)
    d_old = _dev(np.frombuffer(b"".join(fr), np.uint8)) if fr else None
    d_lh, d_roots, d_paths = _guarded(32 * n), _guarded(32 * n), _guarded(32 * entries)
    d_new, d_root = _dev(np.zeros(64 * 32, np.uint8)), _dev(np.zeros(32, np.uint8))
    edv.merkle_append_batch_device(old, d_old.ptr if d_old else None, d_leaves.ptr, d_off.ptr, n, d_lh.ptr, None,
                                   d_new.ptr, d_root.ptr, d_roots.ptr, d_paths.ptr)
    poff = vc.u64(edv.merkle_path_entries(old, i) for i in range(n + 1))
    d_poff = _dev(poff)
    d_idx, d_size = _dev(vc.u64(old + i for i in range(n))), _dev(vc.u64(old + i + 1 for i in range(n)))
    out = _Outputs(n, 32, True)

    def verify(**leaf):
        edv.merkle_verify_inclusion_device(d_idx.ptr, d_size.ptr, d_roots.ptr, d_paths.ptr, d_poff.ptr, n,
                                           out.status.ptr, out.computed.ptr, **leaf)
        return out.result()
    st, comp = verify(d_leaf_hashes=d_lh.ptr)
    assert st == bytes([vc.OK]) * n and comp == d_roots.download(32 * n).tobytes()
    assert verify(d_leaves=d_leaves.ptr, d_leaf_off=d_off.ptr)[0] == bytes([vc.OK]) * n
    # one entry overwritten on the device: exactly the proof that holds it turns ROOT
    row = int(poff[400]) + 1 if old else int(poff[400])
    junk = np.full(32, 0x5A, np.uint8)
    edv._check(edv.lib().edv_h2d(0, d_paths.ptr + 32 * row, junk.ctypes.data, 32))
    hit = [i for i in range(n) if poff[i] <= row < poff[i + 1]]
    assert len(hit) == 1
    st, _ = verify(d_leaf_hashes=d_lh.ptr)
    assert [i for i in range(n) if st[i] != vc.OK] == hit and st[hit[0]] == vc.ROOT


def test_two_caller_streams_back_to_back(grid):
    b, exp = grid["inc"]
    c, cexp = grid["con"]
    s1, s2 = _HipStream(), _HipStream()
    calls = [IncCall(b), ConCall(c), IncCall(b, by_hash=True), ConCall(c)]
    for k, call in enumerate(calls):
        call.run(stream=(s1, s2)[k % 2].ptr)
    s1.synchronize()
    s2.synchronize()
    assert [call.result() for call in calls] == [exp, cexp, exp, cexp]


def test_argument_errors_launch_nothing(grid):
    E = edv.EDV_E_ARG
    lib = edv.lib()
    b = vc.synth_inclusion(vc.inclusion_points()[10:16], seed=51)
    n = len(b)
    ci, ch = IncCall(b), IncCall(b, by_hash=True)

    def dev_inc(call, n=n, **kw):
        a = dict(dict(d_leaves=None, d_leaf_off=None, d_leaf_hashes=None), **call.args())
        a.update(kw, n=n)
        return lib.edv_merkle_verify_inclusion_dev(a["d_leaves"], a["d_leaf_off"], a["leaf_base"], a["d_leaf_hashes"],
                                                   a["d_leaf_index"], a["d_tree_size"], a["d_roots"], a["d_proofs"],
                                                   a["d_proof_off"], a["proof_base"], a["n"], a["d_status"],
                                                   a["d_computed"], 0, None)
    assert dev_inc(ci, n=edv.MERKLE_MAX_LEAVES + 1) == E
    assert dev_inc(ci, d_leaf_hashes=ch.d_lh.ptr) == E                       # both leaf forms
    assert dev_inc(ci, d_leaves=None, d_leaf_off=None) == E                  # neither
    assert dev_inc(ci, d_leaf_off=None) == E
    for k in ("d_leaf_index", "d_tree_size", "d_roots", "d_proofs", "d_proof_off", "d_status"):
        assert dev_inc(ci, **{k: None}) == E
        assert dev_inc(ch, **{k: None}) == E
    for k in ("d_leaf_off", "d_leaf_index", "d_tree_size", "d_proof_off"):   # 64-bit arrays: 8-byte aligned
        assert dev_inc(ci, **{k: ci.args()[k] + 4}) == E
    for k in ("d_roots", "d_proofs", "d_computed"):                          # hash buffers: 16-byte aligned
        assert dev_inc(ci, **{k: ci.args()[k] + 8}) == E
    assert dev_inc(ch, d_leaf_hashes=ch.d_lh.ptr + 8) == E
    assert ci.out.untouched() and ch.out.untouched()
    # d_status may have any alignment, and n = 0 writes nothing
    assert dev_inc(ci, n=0) == 0 and dev_inc(ci, n=0, d_leaf_index=None, d_status=None) == 0 and ci.out.untouched()
    odd = _guarded(n + 3)
    assert dev_inc(ci, d_status=odd.ptr + 3, d_computed=None) == 0
    assert odd.download().tobytes() == bytes([SENTINEL]) * 3 + b.expected()[0] + bytes([SENTINEL]) * 32
    assert ci.out.untouched()

    c = vc.synth_consistency(vc.consistency_points()[10:16], seed=51)
    cc = ConCall(c)

    def dev_con(n=len(c), **kw):
        a = dict(cc.args(), **kw)
        a["n"] = n
        return lib.edv_merkle_verify_consistency_dev(a["d_old_size"], a["d_new_size"], a["d_old_roots"], a["d_new_roots"],
                                                     a["d_proofs"], a["d_proof_off"], a["proof_base"], a["n"],
                                                     a["d_status"], a["d_computed"], 0, None)
    assert dev_con(n=edv.MERKLE_MAX_LEAVES + 1) == E
    for k in ("d_old_size", "d_new_size", "d_old_roots", "d_new_roots", "d_proofs", "d_proof_off", "d_status"):
        assert dev_con(**{k: None}) == E
    for k in ("d_old_size", "d_new_size", "d_proof_off"):
        assert dev_con(**{k: cc.args()[k] + 4}) == E
    for k in ("d_old_roots", "d_new_roots", "d_proofs", "d_computed"):
        assert dev_con(**{k: cc.args()[k] + 8}) == E
    assert cc.out.untouched() and dev_con(n=0) == 0 and cc.out.untouched()

    # the host forms: their own lists, the offsets included
    blob, loff = mc.pack(b.leaves)
    blob = np.concatenate([blob, np.zeros(8, np.uint8)])
    proofs, poff = vc.pack_proofs(b.proof)
    lh, roots, idx, size = vc.pack_hashes(b.leaf_hashes()), vc.pack_hashes(b.root), vc.u64(b.index), vc.u64(b.size)
    status, computed = np.full(n, SENTINEL, np.uint8), np.full(32 * n, SENTINEL, np.uint8)
    p = vc._p
    h = dict(leaves=p(blob), leaf_off=p(loff), leaf_hashes=None, leaf_index=p(idx), tree_size=p(size), roots=p(roots),
             proofs=p(proofs), proof_off=p(poff), status=p(status))

    def host_inc(n=n, **kw):
        a = dict(h, **kw)
        return lib.edv_merkle_verify_inclusion(a["leaves"], a["leaf_off"], a["leaf_hashes"], a["leaf_index"],
                                               a["tree_size"], a["roots"], a["proofs"], a["proof_off"], n, a["status"],
                                               p(computed), 0)
    bad = np.array([0, 2, 1] + [3] * (n - 2), np.uint64)                     # offsets must not decrease
    assert host_inc(n=edv.MERKLE_MAX_LEAVES + 1) == E
    assert host_inc(leaf_hashes=p(lh)) == E and host_inc(leaves=None, leaf_off=None) == E and host_inc(leaf_off=None) == E
    for k in ("leaf_index", "tree_size", "roots", "proofs", "proof_off", "status"):
        assert host_inc(**{k: None}) == E
    assert host_inc(proof_off=p(bad)) == E and host_inc(leaf_off=p(bad)) == E
    assert (status == SENTINEL).all() and (computed == SENTINEL).all()
    assert host_inc(n=0) == 0 and (status == SENTINEL).all()
    cproofs, cpoff = vc.pack_proofs(c.proof)
    olds, news, ro, rn = vc.u64(c.old), vc.u64(c.new), vc.pack_hashes(c.old_root), vc.pack_hashes(c.new_root)
    cstatus = np.full(len(c), SENTINEL, np.uint8)
    hc = dict(old_size=p(olds), new_size=p(news), old_roots=p(ro), new_roots=p(rn), proofs=p(cproofs),
              proof_off=p(cpoff), status=p(cstatus))

    def host_con(n=len(c), **kw):
        a = dict(hc, **kw)
        return lib.edv_merkle_verify_consistency(a["old_size"], a["new_size"], a["old_roots"], a["new_roots"],
                                                 a["proofs"], a["proof_off"], n, a["status"], None, 0)
    assert host_con(n=edv.MERKLE_MAX_LEAVES + 1) == E
    for k in hc:
        assert host_con(**{k: None}) == E
    assert host_con(proof_off=p(bad)) == E and (cstatus == SENTINEL).all()
    # and the same arguments, well formed, go through
    assert host_inc() == 0 and (status.tobytes(), computed.tobytes()) == b.expected()
    assert host_con() == 0 and cstatus.tobytes() == c.expected()[0]
    assert ci.run().result() == b.expected() and cc.run().result() == c.expected()


def test_lifecycle_staging_is_counted_trimmed_and_released(grid):
    pts = vc.inclusion_points()
    big = vc.synth_inclusion([pts[(k * 13) % len(pts)] for k in range(10000)], seed=61, lengths=[0, 55, 120])
    exp = big.expected()
    small, sexp = grid["inc"]
    con, cexp = grid["con"]
    assert host_inclusion(small) == sexp                       # the context exists
    edv.trim(0, 0)
    before = edv.context_memory(0)
    assert IncCall(small).run().result() == sexp               # the device form uses no context memory
    assert edv.context_memory(0) == before
    assert host_inclusion(big) == exp
    mid = edv.context_memory(0)
    staged = sum(len(x) for x in big.leaves) + 32 * sum(len(p) for p in big.proof) + (32 + 32 + 16 + 1) * len(big)
    assert mid["chunk_scratch"] >= before["chunk_scratch"] + staged
    assert mid["total"] > before["total"]
    # a batch of 100 proofs of 64 entries needs far less than this one left behind
    edv.trim(0, 100)
    assert edv.context_memory(0)["chunk_scratch"] < mid["chunk_scratch"]
    assert host_inclusion(small) == sexp and host_consistency(con) == cexp
    edv.trim(0, 0)
    assert edv.context_memory(0)["total"] == before["total"]
    assert host_consistency(con) == cexp and host_inclusion(small, by_hash=True) == sexp
    edv.release(0)
    assert edv.context_memory(0)["total"] == 0
    assert host_inclusion(small) == sexp and host_consistency(con) == cexp


# ---- the Python surface
def _check_verdicts(got, status, computed=None):
    assert isinstance(got, merkle.ProofVerdicts) and got.status.tobytes() == status
    assert list(got) == [s == vc.OK for s in status]
    if computed is not None:
        assert got.computed.tobytes() == computed


def test_verifier_batches_device_equals_host_equals_golden(golden):
    inc, inc_st, con, con_st = golden
    v = MerkleVerifier()
    sths = [STH(s, r) for s, r in zip(inc.size, inc.root)]
    items = list(zip(con.old, con.new, con.old_root, con.new_root, con.proof))
    for on_device in (True, False):
        _check_verdicts(v.verify_leaf_hash_inclusion_batch(inc.hashes, inc.index, inc.proof, sths, on_device=on_device,
                                                           want_computed=True), inc_st, inc.expected()[1])
        _check_verdicts(v.verify_tree_consistency_batch(items, on_device=on_device, want_computed=True), con_st,
                        con.expected()[1])
    b = vc.synth_inclusion(vc.inclusion_points(), seed=71)
    bs = [STH(s, r) for s, r in zip(b.size, b.root)]
    dev = v.verify_leaf_inclusion_batch(b.leaves, b.index, b.proof, bs, on_device=True, want_computed=True)
    host = v.verify_leaf_inclusion_batch(b.leaves, b.index, b.proof, bs, on_device=False, want_computed=True)
    _check_verdicts(dev, *b.expected())
    assert dev.status.tobytes() == host.status.tobytes() and dev.computed.tobytes() == host.computed.tobytes()
    want = {vc.RANGE: ValueError, vc.SHORT: merkle.ProofError, vc.LONG: merkle.ProofError, vc.ROOT: merkle.ProofError}
    for k, st in enumerate(b.expected()[0]):
        if st == vc.OK:
            assert dev.raise_for(k) is True
        else:
            with pytest.raises(want[st]):
                dev.raise_for(k)
    got = v.verify_tree_consistency_batch(items, on_device=True)
    k = con_st.index(bytes([vc.INCONSISTENT]))
    with pytest.raises(merkle.ConsistencyError):
        got.raise_for(k)
    # integers the C-ABI cannot carry never reach the device as they are
    lh = mc.leaf_hash(b"")
    got = v.verify_leaf_hash_inclusion_batch([lh] * 3, [-1, 0, 2 ** 64], [[], [], []],
                                             [STH(1, lh), STH(1, lh), STH(2 ** 64 + 1, lh)], on_device=True)
    assert got.status.tobytes() == bytes([vc.RANGE, vc.OK, vc.RANGE])
    got = v.verify_tree_consistency_batch([(-1, 3, lh, lh, []), (2 ** 64, 2 ** 64, lh, lh, []), (3, 3, lh, lh, [])],
                                          on_device=True)
    assert got.status.tobytes() == bytes([vc.RANGE, vc.RANGE, vc.OK])


def test_verify_append_batch_accepts_what_the_device_appended():
    leaves = mc.load_golden()["leaves"]
    t = merkle.CompactMerkleTree()
    batch = t.append_batch(leaves, on_device=True)
    for kw in ({}, {"max_call": 300}):
        got = merkle.verify_append_batch(0, leaves, batch, on_device=True, **kw)
        assert len(got) == 1000 and got.ok.all() and got.raise_first() is True
    t = merkle.CompactMerkleTree()
    batch = t.append_batch(leaves, on_device=True, max_call=300)
    assert merkle.verify_append_batch(0, leaves, batch, on_device=True).ok.all()
    assert merkle.MIN_DEVICE_VERIFY_PROOFS <= 1000 and merkle.verify_append_batch(0, leaves, batch).ok.all()
    batch.paths = batch.paths.copy()
    batch.paths[merkle.popcount_prefix(900), 7] ^= 1
    got = merkle.verify_append_batch(0, leaves, batch, on_device=True)
    assert [k for k, ok in enumerate(got) if not ok] == [900] and got.status[900] == vc.ROOT


def test_ledger_checks_on_the_device():
    leaves = mc.load_golden()["leaves"]

    def ser(txn):
        return txn["payload"]
    L = Ledger(serialize_for_tree=ser, on_device=True)
    txns = [{"payload": leaf} for leaf in leaves]
    L.appendTxns(txns)
    L.commitTxns(700)
    L.commitTxns(300)
    results = [dict(t, seqNo=i + 1) for i, t in enumerate(txns)]
    assert verify_merkle_proofs(results, ser, on_device=True) is True
    assert verify_merkle_proofs(results, ser) is True
    bad = [dict(r) for r in results]
    bad[500]["auditPath"] = list(bad[500]["auditPath"])
    bad[500]["auditPath"][1] = bad[499]["auditPath"][0]
    with pytest.raises(merkle.ProofError):
        verify_merkle_proofs(bad, ser, on_device=True)
    # catch-up: a ledger 400 behind applies 400 transactions (a device extend) and checks the real proof
    proof = [Ledger.hashToStr(h) for h in L.tree.consistency_proof(900, 1000)]
    behind = Ledger(serialize_for_tree=ser, on_device=True)
    behind.appendTxns([{"payload": leaf} for leaf in leaves[:500]])
    behind.commitTxns(500)
    got = [{"payload": leaf} for leaf in leaves[500:900]]
    assert len(got) >= merkle.MIN_DEVICE_LEAVES
    assert behind.verify_catchup_txns(got, 1000, L.root_hash, proof) is True
    got[123] = {"payload": got[123]["payload"] + b"!"}
    assert behind.verify_catchup_txns(got, 1000, L.root_hash, proof) is False
