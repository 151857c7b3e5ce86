"""Batched proof generation on the device (row f-8): edv_merkle_prove_inclusion /
_consistency and their device-resident forms against the checker of
tests/merkle_prove_cases.py and the reference's recorded digests, the made
proofs checked by the verify kernels with no host copy between them, the
DeviceHashStore's upkeep, context memory, streams and argument errors."""
import ctypes
import hashlib
import random

import numpy as np
import pytest

import merkle_cases as mc
import merkle_prove_cases as pc
from indy_plenum_amd import Ledger, MerkleVerifier, edv, merkle

pytestmark = pytest.mark.gpu

G = pc.load_golden()
LH, LEAFS, NODES = pc.golden_store()
TREE = pc.Tree(LH)
P = pc.PATTERN


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


def _pattern(nbytes):
    """A device buffer of nbytes of PATTERN and 32 more behind them."""
    return _dev(np.full(nbytes + 32, P, np.uint8))


@pytest.fixture(scope="module")
def store():
    """The 1,000 golden leaves' two stores on the device: (leaf buffer, node buffer, 1000)."""
    return (_dev(np.frombuffer(LEAFS, np.uint8)), _dev(np.frombuffer(NODES, np.uint8)), 1000)


class ProveCall:
    """One edv_merkle_prove_*_dev call's buffers.  The slots buffer holds one
    guard entry, the entries [off[0], off[-1]) and 32 guard bytes, all PATTERN;
    the call gets the offsets moved so that entry off[0] lies behind the first
    guard, and PROOF_BASE more, which it hands over as proof_base."""
    PROOF_BASE = 2 ** 32 + 5   # an offset cut to 32 bits loses it

    def __init__(self, consistency, store, pairs, off=None, want1=True, want2=True):
        self.consistency, self.store, self.n = consistency, store, len(pairs)
        self.off = pc.exact_offsets(consistency, pairs, store[2]) if off is None else off
        self.entries = int(self.off[-1]) - int(self.off[0])
        self.koff = self.off - self.off[0] + np.uint64(1 + self.PROOF_BASE)
        self.want1, self.want2 = want1, want2
        self.d_a, self.d_b = _dev(pc.u64(p[0] for p in pairs)), _dev(pc.u64(p[1] for p in pairs))
        self.d_off = _dev(self.koff)
        self.d_slots, self.d_status = _pattern(32 * (self.entries + 1)), _pattern(self.n)
        self.d_1, self.d_2 = _pattern(32 * self.n), _pattern(32 * self.n)

    def args(self):
        return [self.store[0].ptr, self.store[1].ptr, self.store[2], self.d_a.ptr, self.d_b.ptr, self.d_off.ptr,
                self.PROOF_BASE, self.n, self.d_slots.ptr, self.d_status.ptr,
                self.d_1.ptr if self.want1 else None, self.d_2.ptr if self.want2 else None]

    def raw(self, stream=None, **kw):
        """The C call with some arguments replaced (by position name) -> its return code."""
        names = ["leaf_store", "node_store", "store_leaves", "a", "b", "off", "base", "n", "proofs", "status", "o1", "o2"]
        a = dict(zip(names, self.args()))
        a.update(kw)
        fn = edv.lib().edv_merkle_prove_consistency_dev if self.consistency else edv.lib().edv_merkle_prove_inclusion_dev
        return fn(*[a[k] for k in names], 0, stream)

    def run(self, stream=None):
        assert self.raw(stream) == 0
        return self

    def result(self):
        """(status, slots, out1 | None, out2 | None), guards intact, outputs not asked for untouched."""
        guard = bytes([P]) * 32
        slots, status = self.d_slots.download().tobytes(), self.d_status.download().tobytes()
        o1, o2 = self.d_1.download().tobytes(), self.d_2.download().tobytes()
        assert slots[:32] == guard and slots[32 * (self.entries + 1):] == guard
        assert status[self.n:] == guard and o1[32 * self.n:] == guard and o2[32 * self.n:] == guard
        if not self.want1:
            assert o1 == bytes([P]) * len(o1)
        if not self.want2:
            assert o2 == bytes([P]) * len(o2)
        return (status[:self.n], slots[32:32 * (self.entries + 1)], o1[:32 * self.n] if self.want1 else None,
                o2[:32 * self.n] if self.want2 else None)

    def untouched(self):
        return all(b.download().tobytes() == bytes([P]) * b.nbytes for b in (self.d_slots, self.d_status, self.d_1, self.d_2))


def host_form(consistency, pairs, store_leaves=1000, off=None):
    """The host C-ABI form over PATTERN-filled outputs -> (status, slots, out1, out2)."""
    n = len(pairs)
    off = pc.exact_offsets(consistency, pairs, store_leaves) if off is None else off
    entries = int(off[-1]) - int(off[0])
    la, na = np.frombuffer(LEAFS, np.uint8), np.frombuffer(NODES, np.uint8)
    a, b = pc.u64(p[0] for p in pairs), pc.u64(p[1] for p in pairs)
    bufs = pc.run_outputs(n, entries)
    fn = edv.lib().edv_merkle_prove_consistency if consistency else edv.lib().edv_merkle_prove_inclusion
    rc = fn(la.ctypes.data, na.ctypes.data, store_leaves, a.ctypes.data, b.ctypes.data, off.ctypes.data, n,
            bufs[0].ctypes.data - 32 * int(off[0]), bufs[1].ctypes.data, bufs[2].ctypes.data, bufs[3].ctypes.data, 0)
    assert rc == 0, edv.lib().edv_last_error()
    return pc.read_outputs(n, entries, bufs)


def expected(consistency, pairs, off=None, store_leaves=1000):
    off = pc.exact_offsets(consistency, pairs, store_leaves) if off is None else off
    return pc.expected(TREE, consistency, pairs, store_leaves, off)


# ---- small shapes
@pytest.mark.parametrize("consistency", [False, True])
def test_all_pairs_up_to_65_in_one_call(store, consistency):
    pairs = [p for n in range(1, 66) for p in pc.all_pairs(n, consistency)]
    assert len(pairs) == 2145
    exp = expected(consistency, pairs)
    assert set(exp[0]) == {pc.OK}
    got = ProveCall(consistency, store, pairs).run().result()
    assert got == exp
    assert host_form(consistency, pairs) == exp
    off, at = pc.exact_offsets(consistency, pairs, 1000), 0
    key = "consistency_sha256" if consistency else "inclusion_sha256"
    for r in G["all_pairs"][:65]:
        assert hashlib.sha256(got[1][32 * int(off[at]):32 * int(off[at + r["n"]])]).hexdigest() == r[key], r["n"]
        at += r["n"]


@pytest.mark.parametrize("consistency", [False, True])
def test_the_five_larger_sizes(store, consistency):
    key = "consistency_sha256" if consistency else "inclusion_sha256"
    pairs = [p for n in pc.LARGE for p in pc.all_pairs(n, consistency)]
    got = ProveCall(consistency, store, pairs).run().result()
    assert got == expected(consistency, pairs) == host_form(consistency, pairs)
    off, at = pc.exact_offsets(consistency, pairs, 1000), 0
    for n in pc.LARGE:
        r = next(r for r in G["all_pairs"] if r["n"] == n)
        assert hashlib.sha256(got[1][32 * int(off[at]):32 * int(off[at + n])]).hexdigest() == r[key], n
        at += n


@pytest.fixture(scope="module")
def golden_tree():
    tree = merkle.CompactMerkleTree(hashStore=merkle.DeviceHashStore())
    tree.extend(G["leaf_list"], on_device=False)
    return tree


def test_merkle_info_batch_equals_the_recorded_digests(golden_tree):
    batch = golden_tree.merkle_info_batch(range(1, 1001), on_device=True)
    got = [hashlib.sha256(batch.roots[i].tobytes() + b"".join(p)).hexdigest() for i, p in enumerate(batch)]
    assert got == G["merkle_info"]["per_seq_no_sha256"]
    assert batch.leaf_hashes.tobytes() == LEAFS
    assert golden_tree.hashStore.bytes_uploaded == len(LEAFS) + len(NODES)
    # the verifier takes the batch as it is, on the device and on the host
    assert MerkleVerifier().verify_proof_batch(batch, on_device=True).ok.all()
    assert MerkleVerifier().verify_proof_batch(batch, on_device=False).ok.all()
    led = Ledger(tree=golden_tree, transactionLog=G["leaf_list"], on_device=True)
    some = [1, 2, 64, 65, 777, 1000]
    assert led.merkleInfoBatch(some) == [led.merkleInfo(s) for s in some]
    cons = golden_tree.consistency_proof_batch([(a, 1000) for a in range(1, 1001)], on_device=True)
    assert pc.digest(list(cons)) == next(r for r in G["all_pairs"] if r["n"] == 1000)["consistency_sha256"]
    assert MerkleVerifier().verify_proof_batch(cons, on_device=True).ok.all()
    # the host-buffer route (a copy of the store per call) over a plain store gives the same batch
    plain = merkle.CompactMerkleTree()
    plain.extend(G["leaf_list"], on_device=False)
    other = plain.merkle_info_batch(range(1, 1001), on_device=True)
    assert other.proofs.tobytes() == batch.proofs.tobytes() and other.roots.tobytes() == batch.roots.tobytes()
    assert other.off.tolist() == batch.off.tolist()


# ---- one wave holds them all
@pytest.mark.parametrize("consistency", [False, True])
def test_one_wave_carries_every_case(store, consistency):
    pairs, off, short, long_ = pc.one_wave(consistency, 1000)
    assert len(pairs) == 64 and int(off[0]) == 3
    exp = expected(consistency, pairs, off)
    assert exp[0][short] == exp[0][long_] == pc.SPACE and exp[0].count(bytes([pc.RANGE])) == 8
    lens = [int(off[i + 1] - off[i]) for i in range(64) if exp[0][i] == pc.OK]
    assert 0 in lens and max(lens) >= 10
    assert ProveCall(consistency, store, pairs, off).run().result() == exp
    assert host_form(consistency, pairs, off=off) == exp
    for want1, want2 in ((False, False), (True, False), (False, True)):
        got = ProveCall(consistency, store, pairs, off, want1, want2).run().result()
        assert got[:2] == exp[:2]
        assert got[2] == (exp[2] if want1 else None) and got[3] == (exp[3] if want2 else None)
    # every RANGE case against a store of 11 leaves, too
    rng = pc.range_cases(consistency, 11)
    small = (store[0], store[1], 11)
    assert ProveCall(consistency, small, rng).run().result() == expected(consistency, rng, store_leaves=11)


# ---- a deep store
DEEP = 2 ** 20 + 12345


@pytest.fixture(scope="module")
def deep_tree():
    blob = np.arange(DEEP, dtype=np.uint64).view(np.uint8).tobytes()
    tree = merkle.CompactMerkleTree(hashStore=merkle.DeviceHashStore())
    tree.extend([blob[8 * i:8 * i + 8] for i in range(DEEP)], on_device=True)   # one device extend
    return tree


def test_deep_store_proofs_verify_on_the_device(deep_tree):
    tree, hs = deep_tree, deep_tree.hashStore
    d_leafs, d_nodes, leaves, nodes = hs.device_arrays()
    assert (leaves, nodes) == (DEEP, DEEP - mc.popcount(DEEP)) and hs.bytes_uploaded == 32 * (leaves + nodes)
    rng = random.Random(77)
    n = 4096
    sizes = [rng.randrange(1, DEEP + 1) for _ in range(n - 2)] + [DEEP, 2 ** 20]
    inc = [(rng.randrange(s), s) for s in sizes]
    con = [(rng.randrange(1, s + 1), s) for s in sizes]
    dstore = (type("B", (), {"ptr": d_leafs})(), type("B", (), {"ptr": d_nodes})(), DEEP)
    ok = bytes([pc.OK]) * n
    for consistency, pairs in ((False, inc), (True, con)):
        a, b = pc.u64(p[0] for p in pairs), pc.u64(p[1] for p in pairs)
        off = (edv.merkle_consistency_offsets if consistency else edv.merkle_inclusion_offsets)(a, b, DEEP)
        call = ProveCall(consistency, dstore, pairs, off)
        call.run()
        d_vst = _pattern(n)
        proofs, base = call.d_slots.ptr, call.PROOF_BASE
        if consistency:
            edv.merkle_verify_consistency_device(call.d_a.ptr, call.d_b.ptr, call.d_1.ptr, call.d_2.ptr, proofs,
                                                 call.d_off.ptr, n, d_vst.ptr, proof_base=base)
        else:
            edv.merkle_verify_inclusion_device(call.d_a.ptr, call.d_b.ptr, call.d_1.ptr, proofs, call.d_off.ptr, n,
                                               d_vst.ptr, d_leaf_hashes=call.d_2.ptr, proof_base=base)
        assert d_vst.download(n).tobytes() == ok
        st, slots, o1, o2 = call.result()
        assert st == ok
        for i in list(range(0, n, 17)) + [n - 2, n - 1]:   # 243 sampled proofs against the host's single calls
            x, y = pairs[i]
            single = tree.consistency_proof(x, y) if consistency else tree.inclusion_proof(x, y)
            assert slots[32 * int(off[i]):32 * int(off[i + 1])] == b"".join(single), (consistency, x, y)
            if consistency:
                assert o1[32 * i:32 * i + 32] == tree.merkle_tree_hash(0, x)
                assert o2[32 * i:32 * i + 32] == tree.merkle_tree_hash(0, y)
            else:
                assert o1[32 * i:32 * i + 32] == tree.merkle_tree_hash(0, y) and o2[32 * i:32 * i + 32] == hs.readLeaf(x + 1)
    assert o2[32 * (n - 2):32 * (n - 1)] == tree.root_hash
    # and through the tree's own batch call, by its default route
    batch = tree.inclusion_proof_batch(inc[:300], on_device=True)
    assert batch.proofs.tobytes() == b"".join(b"".join(tree.inclusion_proof(x, y)) for x, y in inc[:300])


# ---- the store's upkeep
def test_store_uploads_only_the_tail_grows_and_resets():
    leaves = mc.leaves_of(5, 3000, max_len=40)
    hs = merkle.DeviceHashStore()
    tree, host = merkle.CompactMerkleTree(hashStore=hs), merkle.CompactMerkleTree()
    assert hs.device_bytes == 0
    sent, lo = 0, 0
    for hi in (700, 1500, 2000):   # three appends with proof calls between them: only the new tail goes up
        tree.append_batch(leaves[lo:hi], on_device=True)
        host.extend(leaves[lo:hi], on_device=False)
        pairs = [(m, hi) for m in range(lo, hi, 7)] + [(0, 1), (hi - 1, hi)]
        batch = tree.inclusion_proof_batch(pairs, on_device=True)
        assert list(batch) == [host.inclusion_proof(m, n) for m, n in pairs]
        assert batch.roots[-1].tobytes() == host.root_hash == tree.root_hash
        now = 32 * (hs.leafCount + hs.nodeCount)
        assert hs.bytes_uploaded == now and now > sent   # each byte once
        sent, lo = now, hi
    assert hs._bufs[0].nbytes == hs.MIN_CAPACITY == 65536   # 2,000 leaf hashes still fit the first mirror
    tree.append_batch(leaves[2000:], on_device=True)             # 3,000 do not: it is replaced and filled again
    host.extend(leaves[2000:], on_device=False)
    pairs = [(a, 3000) for a in range(1, 3001, 13)] + [(2049, 2050), (3000, 3000)]
    cons = tree.consistency_proof_batch(pairs, on_device=True)
    assert list(cons) == [host.consistency_proof(a, b) for a, b in pairs]
    assert hs._bufs[0].nbytes >= 32 * 3000 and hs.bytes_uploaded == sent + 32 * (hs.leafCount + hs.nodeCount)
    assert hs.device_bytes > 0
    assert hs.reset() and hs.device_bytes == 0 and hs.leafCount == 0 and hs.bytes_uploaded == 0


# ---- streams and edges
def test_two_caller_streams_interleaved(store):
    inc = [p for n in (64, 65, 777) for p in pc.all_pairs(n, False)]
    con = [p for n in (63, 257) for p in pc.all_pairs(n, True)]
    s1, s2 = _HipStream(), _HipStream()
    calls = [ProveCall(False, store, inc), ProveCall(True, store, con), ProveCall(True, store, con),
             ProveCall(False, store, inc), ProveCall(False, store, inc[::-1])]
    for k, call in enumerate(calls):
        call.run(stream=(s1, s2)[k % 2].ptr)
    s1.synchronize()
    s2.synchronize()
    got = [c.result() for c in calls]
    seq = [ProveCall(False, store, inc).run().result(), ProveCall(True, store, con).run().result()]
    assert got[0] == got[3] == seq[0] == expected(False, inc) and got[1] == got[2] == seq[1] == expected(True, con)
    assert got[4] == expected(False, inc[::-1])


@pytest.mark.parametrize("consistency", [False, True])
def test_argument_errors_and_the_empty_call(store, consistency):
    E = edv.EDV_E_ARG
    pairs = pc.all_pairs(11, consistency)
    c = ProveCall(consistency, store, pairs)
    assert c.raw(n=edv.MERKLE_MAX_LEAVES + 1) == E
    assert c.raw(store_leaves=2 ** 62 + 1) == E
    for k in ("a", "b", "off", "proofs", "status", "leaf_store", "node_store"):
        assert c.raw(**{k: None}) == E, k
    for k in ("a", "b", "off"):                                   # 64-bit arrays: 8-byte aligned
        assert c.raw(**{k: c.args()[["a", "b", "off"].index(k) + 3] + 4}) == E, k
    a = c.args()
    for k, v in (("leaf_store", a[0]), ("node_store", a[1]), ("proofs", a[8]), ("o1", a[10]), ("o2", a[11])):
        assert c.raw(**{k: v + 8}) == E, k                        # hash buffers and both stores: 16-byte aligned
    assert c.untouched()
    assert c.raw(n=0) == 0 and c.raw(n=0, a=None, status=None, proofs=None) == 0 and c.untouched()
    # no store is needed for none, and no node store for a single leaf
    assert c.raw(store_leaves=0, leaf_store=None, node_store=None) == 0
    assert c.result()[0] == bytes([pc.RANGE]) * len(pairs)
    one = ProveCall(consistency, (store[0], store[1], 1), [(1, 1)] if consistency else [(0, 1)])
    assert one.raw(node_store=None) == 0 and one.result() == expected(consistency, [(1, 1)] if consistency else [(0, 1)],
                                                                      store_leaves=1)
    odd = _pattern(len(pairs) + 3)                                # the status may have any alignment
    assert c.raw(status=odd.ptr + 3, o1=None, o2=None) == 0
    assert odd.download().tobytes() == bytes([P]) * 3 + bytes([pc.OK]) * len(pairs) + bytes([P]) * 32

    # the host forms
    lib = edv.lib()
    la, na = np.frombuffer(LEAFS, np.uint8), np.frombuffer(NODES, np.uint8)
    av, bv = pc.u64(p[0] for p in pairs), pc.u64(p[1] for p in pairs)
    off = pc.exact_offsets(consistency, pairs, 1000)
    bufs = pc.run_outputs(len(pairs), int(off[-1]))
    h = dict(leaf_store=la.ctypes.data, node_store=na.ctypes.data, store_leaves=1000, a=av.ctypes.data, b=bv.ctypes.data,
             off=off.ctypes.data, n=len(pairs), proofs=bufs[0].ctypes.data, status=bufs[1].ctypes.data,
             o1=bufs[2].ctypes.data, o2=bufs[3].ctypes.data)
    fn = lib.edv_merkle_prove_consistency if consistency else lib.edv_merkle_prove_inclusion

    def host(**kw):
        x = dict(h, **kw)
        return fn(*[x[k] for k in ("leaf_store", "node_store", "store_leaves", "a", "b", "off", "n", "proofs", "status",
                                   "o1", "o2")], 0)
    bad = np.array([0, 5, 4] + [6] * (len(pairs) - 2), np.uint64)
    assert host(n=edv.MERKLE_MAX_LEAVES + 1) == E and host(store_leaves=2 ** 62 + 1) == E and host(off=bad.ctypes.data) == E
    for k in ("a", "b", "off", "proofs", "status", "leaf_store", "node_store"):
        assert host(**{k: None}) == E, k
    assert all((b == P).all() for b in bufs)
    assert host(n=0) == 0 and all((b == P).all() for b in bufs)
    assert host() == 0 and pc.read_outputs(len(pairs), int(off[-1]), bufs) == expected(consistency, pairs)
    # the offset helpers
    ofn = lib.edv_merkle_consistency_offsets if consistency else lib.edv_merkle_inclusion_offsets
    out = np.zeros(len(pairs) + 1, np.uint64)
    assert ofn(None, bv.ctypes.data, 3, 1000, out.ctypes.data) == E and ofn(av.ctypes.data, bv.ctypes.data, 3, 1000, None) == E
    assert ofn(None, None, 0, 1000, out.ctypes.data) == 0 and ofn(av.ctypes.data, bv.ctypes.data, len(pairs), 1000,
                                                                  out.ctypes.data) == 0
    assert out.tolist() == off.tolist()


# ---- context memory
def test_context_memory(store):
    pairs = [p for n in (1, 2, 65, 1000) for p in pc.all_pairs(n, False)]
    cpairs = [p for n in (1, 65, 777) for p in pc.all_pairs(n, True)]
    exp, cexp = expected(False, pairs), expected(True, cpairs)
    assert host_form(False, pairs[:3]) == expected(False, pairs[:3])   # the context exists
    edv.trim(0, 0)
    before = edv.context_memory(0)
    assert ProveCall(False, store, pairs).run().result() == exp        # the device forms use no context memory
    assert ProveCall(True, store, cpairs).run().result() == cexp
    assert edv.context_memory(0) == before
    assert host_form(False, pairs) == exp
    mid = edv.context_memory(0)
    staged = len(LEAFS) + len(NODES) + 32 * (len(exp[1]) // 32) + (24 + 32 + 32 + 1) * len(pairs)
    assert mid["chunk_scratch"] >= before["chunk_scratch"] + staged and mid["total"] > before["total"]
    assert host_form(True, cpairs) == cexp
    edv.trim(0, 2)   # two proofs of 64 entries need less than the 1,000-leaf store and its 1,068 proofs
    assert edv.context_memory(0)["chunk_scratch"] < mid["chunk_scratch"]
    assert host_form(False, pairs) == exp
    edv.trim(0, 0)
    after = edv.context_memory(0)
    assert (after["total"], after["chunk_scratch"]) == (before["total"], before["chunk_scratch"])
    edv.release(0)
    assert edv.context_memory(0)["total"] == 0
    assert host_form(False, pairs) == exp and host_form(True, cpairs) == cexp
