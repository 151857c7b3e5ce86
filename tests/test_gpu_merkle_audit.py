"""The hash-store audit on the device (row f-9): edv_merkle_audit_nodes /
_leaves and edv_merkle_extend_hashed, host and device-resident forms, against
the checker of tests/merkle_audit_cases.py for every size and mutation; slices
into one summary, the stores' ends, argument errors, context memory, and the
Python route over a DeviceHashStore up to rebuild_nodes.  No test expects a
fault: a damaged store is wrong data inside valid buffers."""
import numpy as np
import pytest

import merkle_audit_cases as ac
import merkle_cases as mc
from indy_plenum_amd import MerkleVerifier, edv, merkle
from indy_plenum_amd.merkle import node_position

pytestmark = pytest.mark.gpu

T = mc.tile()
P, GUARD = ac.PATTERN, ac.GUARD
E = edv.EDV_E_ARG
EMPTY = np.array([0, ac.NONE], np.uint64)


def _dev(host, extra=0):
    b = edv.DeviceBuffer(max(1, host.nbytes) + extra)
    if host.nbytes:
        b.upload(host)
    return b


class DevStore:
    """A store on the device, each part at the end of what the call may read:
    its bytes, then 64 bytes of GUARD that must still be there afterwards."""

    def __init__(self, lh, nodes):
        self.nleaves = len(lh) // 32
        self.lh, self.nodes = bytes(lh), bytes(ac.padded_nodes(nodes, self.nleaves))
        guard = bytes([GUARD]) * 64
        self.d_leafs = _dev(np.frombuffer(self.lh + guard, np.uint8))
        self.d_nodes = _dev(np.frombuffer(self.nodes + guard, np.uint8))

    def intact(self):
        guard = bytes([GUARD]) * 64
        return self.d_leafs.download().tobytes() == self.lh + guard and \
            self.d_nodes.download().tobytes() == self.nodes + guard


class Out:
    """A summary set to empty and `count` status bytes of PATTERN with 32 more behind them."""

    def __init__(self, count, summary=EMPTY):
        self.count = count
        self.d_summary = _dev(np.asarray(summary, np.uint64))
        self.d_status = _dev(np.full(count + 32, P, np.uint8))

    def read(self):
        st = self.d_status.download().tobytes()
        assert st[self.count:] == bytes([P]) * 32
        s = self.d_summary.download(16, np.uint64)
        return (int(s[0]), int(s[1])), st[:self.count]


def dev_nodes(ds, lo, count, out=None, want_status=True, stream=None):
    out = out or Out(count)
    edv.merkle_audit_nodes_device(ds.d_leafs.ptr, ds.d_nodes.ptr, ds.nleaves, lo, count,
                                  out.d_status.ptr if want_status else None, out.d_summary.ptr, stream=stream)
    return out


def host_nodes(lh, nodes, lo, count, want_status=True):
    nleaves = len(lh) // 32
    la, na = ac.arr(lh), ac.arr(ac.padded_nodes(nodes, nleaves))
    st = np.full(count + 32, P, np.uint8)
    summ = np.full(2, 7, np.uint64)
    rc = edv.lib().edv_merkle_audit_nodes(la.ctypes.data, na.ctypes.data, nleaves, lo, count,
                                          st.ctypes.data if want_status else None, summ.ctypes.data, 0)
    assert rc == 0, edv.lib().edv_last_error()
    assert st[count:].tobytes() == bytes([P]) * 32
    return (int(summ[0]), int(summ[1])), st[:count].tobytes()


# ---- the size x mutation table
@pytest.mark.parametrize("size", ac.sizes())
def test_nodes_every_mutation(size):
    for name, lh, nodes, bad in ac.cases(size):
        have = min(len(nodes) // 32, ac.expected_nodes(size))
        ds = DevStore(lh, nodes)
        outs = [(lo, count, dev_nodes(ds, lo, count)) for lo, count in ac.slices(have)]
        for lo, count, out in outs:
            inside = [q for q in bad if lo <= q < lo + count]
            assert out.read() == (ac.summary_of(inside), ac.status_of(bad, lo, count)), (size, name, lo, count)
        quiet = dev_nodes(ds, 0, have, want_status=False)
        assert quiet.read() == (ac.summary_of(bad), bytes([P]) * have)
        assert ds.intact()
        assert host_nodes(lh, nodes, 0, have) == (ac.summary_of(bad), ac.status_of(bad, 0, have)), (size, name)
        if have >= 3:
            lo, count = have // 3, have - have // 3
            inside = [q for q in bad if q >= lo]
            assert host_nodes(lh, nodes, lo, count) == (ac.summary_of(inside), ac.status_of(bad, lo, count))
            assert host_nodes(lh, nodes, lo, count, want_status=False) == (ac.summary_of(inside), bytes([P]) * count)


def test_two_slices_into_one_summary():
    _, lh, nodes, bad = next(c for c in ac.cases(1000) if c[0] == "swap")
    assert len(bad) >= 2
    ds = DevStore(lh, nodes)
    total = len(nodes) // 32
    cut = bad[0] + 1                     # the lowest bad node in the first slice, the others in the second
    out = Out(total)
    edv.merkle_audit_nodes_device(ds.d_leafs.ptr, ds.d_nodes.ptr, 1000, cut, total - cut, out.d_status.ptr + cut,
                                  out.d_summary.ptr)
    assert out.read()[0] == ac.summary_of([q for q in bad if q >= cut])
    edv.merkle_audit_nodes_device(ds.d_leafs.ptr, ds.d_nodes.ptr, 1000, 0, cut, out.d_status.ptr, out.d_summary.ptr)
    assert out.read() == (ac.summary_of(bad), ac.status_of(bad, 0, total))
    # a summary that already holds something keeps it
    more = dev_nodes(ds, 0, total, out=Out(total, summary=[5, 0]))
    assert more.read()[0] == (5 + len(bad), 0)


def test_slice_that_ends_at_the_last_node():
    for size in (T + 1, 2 * T * T + 3):
        _, lh, nodes = ac.store(size)
        total = len(nodes) // 32
        dam = ac.flip(nodes, total - 1, 200)
        ds = DevStore(lh, dam)
        for count in (1, 64, 65, 130):
            out = dev_nodes(ds, total - count, count)
            assert out.read() == ((1, total - 1), ac.status_of([total - 1], total - count, count))
        assert ds.intact()
        # the last leaf's hash has no node above it when the size is odd: nothing reads past the leaf store's end
        leaves = ac.store(size)[0]
        blob, off = mc.pack(leaves[size - 70:], base=3)
        d_blob, d_off = _dev(np.concatenate([blob, np.zeros(8, np.uint8)])), _dev(off)
        out = Out(70)
        edv.merkle_audit_leaves_device(ds.d_leafs.ptr, size, size - 70, d_blob.ptr, d_off.ptr, 70, out.d_status.ptr,
                                       out.d_summary.ptr)
        assert out.read() == ((0, ac.NONE), bytes([ac.OK]) * 70) and ds.intact()


@pytest.mark.parametrize("size", [1, 5, T + 1, 1000])
def test_leaves(size):
    leaves, lh, nodes = ac.store(size)
    flips = sorted({0, size // 2, size - 1})
    dam = lh
    for i in flips:
        dam = ac.flip(dam, i, 3 + i % 200)
    ds = DevStore(dam, nodes)
    for lo, n, base in [(0, size, 0), (0, size, 5), (size // 3, size - size // 3, 1), (size - 1, 1, 2)]:
        part = leaves[lo:lo + n]
        want = [i for i in flips if lo <= i < lo + n]
        assert want == [lo + i for i in ac.expected_bad_leaves(dam[32 * lo:], part)]
        blob, off = mc.pack(part, base)
        blob = np.concatenate([blob, np.zeros(8, np.uint8)])
        # device form: the offsets absolute minus leaf_base, which is far above 2^32; the first leaf `base` bytes in
        big = 2 ** 33 + 8
        d_blob, d_off = _dev(blob), _dev(off + np.uint64(big))
        out = Out(n)
        edv.merkle_audit_leaves_device(ds.d_leafs.ptr, size, lo, d_blob.ptr, d_off.ptr, n, out.d_status.ptr,
                                       out.d_summary.ptr, leaf_base=big)
        assert out.read() == (ac.summary_of(want), ac.status_of(want, lo, n)), (size, lo, n, base)
        bad, first, st = edv.merkle_audit_leaves(dam, size, lo, blob, off)
        assert (bad, first if bad else ac.NONE) == ac.summary_of(want) and st.tobytes() == ac.status_of(want, lo, n)
        assert edv.merkle_audit_leaves(dam, size, lo, blob, off, want_status=False)[:2] == (bad, first)
    assert ds.intact()


def test_golden_store_audits_clean():
    leaves, lh, nodes = ac.store(1000)
    total = len(nodes) // 32
    assert edv.merkle_audit_nodes(lh, nodes, 1000)[:2] == (0, None)
    assert dev_nodes(DevStore(lh, nodes), 0, total).read() == ((0, ac.NONE), bytes([ac.OK]) * total)
    blob, off = mc.pack(leaves)
    assert edv.merkle_audit_leaves(lh, 1000, 0, np.concatenate([blob, np.zeros(8, np.uint8)]), off)[:2] == (0, None)
    tree = merkle.CompactMerkleTree(hashStore=merkle.DeviceHashStore())
    tree.extend(leaves, on_device=True)
    for on_device in (True, None):
        audit = tree.audit_store(leaves, on_device=on_device)
        assert audit.ok and audit.nodes_checked == total and audit.leaves_checked == 1000
    plain = merkle.CompactMerkleTree()
    plain.extend(leaves, on_device=False)
    assert plain.audit_store(leaves, on_device=True).ok        # the host-buffer forms


# ---- extend from hashes
@pytest.mark.parametrize("old", [0, 5, 12345])
def test_extend_hashed_is_extend(old):
    old_hashes = mc.frontier(3, old)
    oh = b"".join(old_hashes)
    for n in (1, T + 1, 2 * T * T + 3):
        leaves = mc.leaves_of(old + 17, n, max_len=20)
        blob, off = mc.pack(leaves)
        lh, nh, new, root = edv.merkle_extend(old, oh, np.concatenate([blob, np.zeros(8, np.uint8)]), off)
        if n <= T + 1:
            assert (lh.tobytes(), nh.tobytes(), [bytes(r) for r in new], root) == mc.simulate(old, old_hashes, leaves)
        gn, gnew, groot = edv.merkle_extend_hashed(old, oh, lh)
        assert (gn.tobytes(), gnew.tobytes(), groot) == (nh.tobytes(), new.tobytes(), root), (old, n)
        gn, gnew, groot = edv.merkle_extend_hashed(old, oh, lh, want_node_hashes=False)
        assert gn is None and (gnew.tobytes(), groot) == (new.tobytes(), root)
        # the device forms, outputs between guards
        d_old, d_lh = _dev(ac.arr(oh)), _dev(lh)
        d_blob, d_off = _dev(np.concatenate([blob, np.zeros(8, np.uint8)])), _dev(off)
        res = []
        for hashed in (False, True):
            d_n, d_new, d_root = (_dev(np.full(k + 32, P, np.uint8)) for k in (nh.nbytes, new.nbytes, 32))
            if hashed:
                edv.merkle_extend_hashed_device(old, d_old.ptr if old else None, d_lh.ptr, n, d_n.ptr, d_new.ptr, d_root.ptr)
            else:
                edv.merkle_extend_device(old, d_old.ptr if old else None, d_blob.ptr, d_off.ptr, n, None, d_n.ptr,
                                         d_new.ptr, d_root.ptr)
            res.append([b.download().tobytes() for b in (d_n, d_new, d_root)])
        assert res[0] == res[1] == [nh.tobytes() + bytes([P]) * 32, new.tobytes() + bytes([P]) * 32, root + bytes([P]) * 32]
        assert d_lh.download().tobytes() == lh.tobytes()


# ---- the Python route over a DeviceHashStore
def test_audit_store_and_rebuild_over_a_device_hash_store():
    leaves = mc.leaves_of(0xF9, 3 * T + 5, max_len=60)
    store = merkle.DeviceHashStore()
    tree = merkle.CompactMerkleTree(hashStore=store)
    tree.extend(leaves[:T], on_device=True)
    tree.append_batch(leaves[T:], on_device=True)
    good_nodes = bytes(store._nodes)
    assert tree.audit_store(on_device=True).ok and tree.audit_store(leaves, on_device=None).ok
    uploaded = store.bytes_uploaded
    assert tree.audit_store(leaves, on_device=True).ok and store.bytes_uploaded == uploaded   # the mirror is up to date
    # one byte of the host copy flipped, the mirror marked stale: exactly that node and its parent
    k = 77
    q = node_position(1, k) - 1
    store._nodes[32 * q + 13] ^= 0x40
    store.mark_stale()
    audit = tree.audit_store(leaves, on_device=True)
    assert audit.bad_nodes == sorted([q + 1, node_position(2, k // 2)]) and audit.bad_leaves == []
    assert audit.counts_ok and not audit.ok
    assert audit.bad_nodes == tree.audit_store(on_device=False).bad_nodes == [p + 1 for p in ac.expected_bad(
        bytes(store._leafs), bytes(store._nodes))]
    assert store.bytes_uploaded == uploaded + len(store._leafs) + len(store._nodes)
    # a leaf hash flipped too: the leaf and its parent
    store._leafs[32 * 9] ^= 1
    store.mark_stale()
    both = tree.audit_store(leaves, on_device=True)
    assert both.bad_leaves == [10] and both.bad_nodes == sorted(audit.bad_nodes + [node_position(1, 4)])
    store._leafs[32 * 9] ^= 1
    store.mark_stale()
    tree.rebuild_nodes(on_device=True)
    assert bytes(store._nodes) == good_nodes and store._sent[1] == 0
    assert tree.audit_store(leaves, on_device=True).ok and store._sent[1] == len(good_nodes)
    fresh = merkle.CompactMerkleTree()
    fresh.extend(leaves, on_device=False)
    assert (tree.tree_size, tree.hashes, tree.root_hash) == (fresh.tree_size, fresh.hashes, fresh.root_hash)
    n = len(leaves)
    pairs = [(m, n) for m in range(0, n, 7)] + [(m, m + 1) for m in range(0, n, 11)]
    batch = tree.inclusion_proof_batch(pairs, on_device=True)
    assert MerkleVerifier().verify_proof_batch(batch, on_device=True).ok.all()
    assert batch.roots[0].tobytes() == fresh.root_hash
    # extend_hashed on the device: tree and store as extend leaves them
    more = mc.leaves_of(0xFA, T + 9, max_len=30)
    tree.extend_hashed([mc.leaf_hash(x) for x in more], on_device=True)
    fresh.extend(more, on_device=False)
    assert (tree.tree_size, tree.hashes, tree.root_hash) == (fresh.tree_size, fresh.hashes, fresh.root_hash)
    assert store._leafs == fresh.hashStore._leafs and store._nodes == fresh.hashStore._nodes
    assert tree.audit_store(leaves + more, on_device=True).ok


# ---- argument errors
def test_argument_errors_and_empty_calls():
    leaves, lh, nodes = ac.store(9)
    ds = DevStore(lh, nodes)
    lib = edv.lib()
    out = Out(16, summary=[7, 7])
    blob, off = mc.pack(leaves)
    d_blob, d_off = _dev(np.concatenate([blob, np.zeros(8, np.uint8)])), _dev(off)
    L, N, S, ST = ds.d_leafs.ptr, ds.d_nodes.ptr, out.d_summary.ptr, out.d_status.ptr

    def untouched():
        return out.read() == ((7, 7), bytes([P]) * 16) and ds.intact()

    nd = lib.edv_merkle_audit_nodes_dev
    for args in ((L, N, 9, 0, 8, ST, S), (L, N, 9, 7, 1, ST, S), (L, N, 9, 8, 0, ST, S), (L, N, 9, 2 ** 64 - 1, 2, ST, S),
                 (L, N, 9, 0, edv.MERKLE_MAX_LEAVES + 1, ST, S), (L, N, 2 ** 62 + 1, 0, 1, ST, S),
                 (None, N, 9, 0, 1, ST, S), (L, None, 9, 0, 1, ST, S), (L, N, 9, 0, 1, ST, None),
                 (L + 8, N, 9, 0, 1, ST, S), (L, N + 8, 9, 0, 1, ST, S), (L, N, 9, 0, 1, ST, S + 4)):
        assert nd(*args, 0, None) == E, args
    lv = lib.edv_merkle_audit_leaves_dev
    for args in ((L, 9, 0, d_blob.ptr, d_off.ptr, 0, 10, ST, S), (L, 9, 9, d_blob.ptr, d_off.ptr, 0, 1, ST, S),
                 (L, 9, 0, d_blob.ptr, d_off.ptr, 0, edv.MERKLE_MAX_LEAVES + 1, ST, S),
                 (L, 2 ** 62 + 1, 0, d_blob.ptr, d_off.ptr, 0, 1, ST, S), (None, 9, 0, d_blob.ptr, d_off.ptr, 0, 1, ST, S),
                 (L, 9, 0, None, d_off.ptr, 0, 1, ST, S), (L, 9, 0, d_blob.ptr, None, 0, 1, ST, S),
                 (L, 9, 0, d_blob.ptr, d_off.ptr, 0, 1, ST, None), (L + 8, 9, 0, d_blob.ptr, d_off.ptr, 0, 1, ST, S),
                 (L, 9, 0, d_blob.ptr, d_off.ptr + 4, 0, 1, ST, S), (L, 9, 0, d_blob.ptr, d_off.ptr, 0, 1, ST, S + 4)):
        assert lv(*args, 0, None) == E, args
    assert untouched()
    # empty calls write nothing, with or without stores
    assert nd(L, N, 9, 7, 0, ST, S, 0, None) == 0 and nd(None, None, 0, 0, 0, None, S, 0, None) == 0
    assert lv(L, 9, 9, None, None, 0, 0, ST, S, 0, None) == 0 and untouched()
    # the status may have any alignment, the leaf bytes too
    odd = Out(16)
    assert nd(L, N, 9, 0, 7, odd.d_status.ptr + 3, odd.d_summary.ptr, 0, None) == 0
    assert odd.read() == ((0, ac.NONE), bytes([P]) * 3 + bytes([ac.OK]) * 7 + bytes([P]) * 6)

    # the host forms
    la, na, ba = ac.arr(lh), ac.arr(nodes), np.concatenate([blob, np.zeros(8, np.uint8)])
    st, summ = np.full(16, P, np.uint8), np.full(2, 7, np.uint64)
    A, B, O, H, M = la.ctypes.data, na.ctypes.data, off.ctypes.data, st.ctypes.data, summ.ctypes.data
    dec = np.array([0, 5, 4], np.uint64)
    hn, hl = lib.edv_merkle_audit_nodes, lib.edv_merkle_audit_leaves
    for args in ((A, B, 9, 0, 8, H, M), (A, B, 9, 8, 0, H, M), (A, B, 9, 0, edv.MERKLE_MAX_LEAVES + 1, H, M),
                 (A, B, 2 ** 62 + 1, 0, 1, H, M), (None, B, 9, 0, 1, H, M), (A, None, 9, 0, 1, H, M),
                 (A, B, 9, 0, 1, H, None)):
        assert hn(*args, 0) == E, args
    for args in ((A, 9, 0, ba.ctypes.data, O, 10, H, M), (A, 9, 9, ba.ctypes.data, O, 1, H, M),
                 (A, 2 ** 62 + 1, 0, ba.ctypes.data, O, 1, H, M), (None, 9, 0, ba.ctypes.data, O, 1, H, M),
                 (A, 9, 0, None, O, 9, H, M), (A, 9, 0, ba.ctypes.data, None, 1, H, M),
                 (A, 9, 0, ba.ctypes.data, O, 1, H, None), (A, 9, 0, ba.ctypes.data, dec.ctypes.data, 2, H, M)):
        assert hl(*args, 0) == E, args
    assert (st == P).all() and summ.tolist() == [7, 7]
    assert hn(A, B, 9, 7, 0, H, M, 0) == 0 and (st == P).all() and summ.tolist() == [0, ac.NONE]   # the initial summary alone
    summ[:] = 7
    assert hl(A, 9, 9, None, None, 0, H, M, 0) == 0 and (st == P).all() and summ.tolist() == [0, ac.NONE]
    # extend from hashes: the extend's checks
    new, root = np.full(64 * 32, P, np.uint8), np.full(32, P, np.uint8)
    eh, ehd = lib.edv_merkle_extend_hashed, lib.edv_merkle_extend_hashed_dev
    assert eh(0, None, None, 1, None, new.ctypes.data, root.ctypes.data, 0) == E
    assert eh(0, None, A, edv.MERKLE_MAX_LEAVES + 1, None, new.ctypes.data, root.ctypes.data, 0) == E
    assert eh(5, None, A, 1, None, new.ctypes.data, root.ctypes.data, 0) == E
    assert eh(2 ** 62, None, A, 1, None, new.ctypes.data, root.ctypes.data, 0) == E
    assert eh(0, None, A, 1, None, None, root.ctypes.data, 0) == E and eh(0, None, A, 1, None, new.ctypes.data, None, 0) == E
    assert (new == P).all() and (root == P).all()
    d_new = _dev(np.full(64 * 32 + 32, P, np.uint8))
    for args in ((0, None, None, 1, None, d_new.ptr, d_new.ptr + 32), (0, None, L + 8, 1, None, d_new.ptr, d_new.ptr + 32),
                 (0, None, L, 1, None, d_new.ptr + 8, d_new.ptr + 32), (0, None, L, 1, None, d_new.ptr, None),
                 (3, None, L, 1, None, d_new.ptr, d_new.ptr + 32)):
        assert ehd(*args, 0, None) == E, args
    assert (d_new.download() == P).all() and ds.intact()


# ---- context memory
def test_context_memory():
    leaves, lh, nodes = ac.store(1000)
    total = len(nodes) // 32
    ds = DevStore(lh, nodes)
    blob, off = mc.pack(leaves)
    blob = np.concatenate([blob, np.zeros(8, np.uint8)])
    d_blob, d_off = _dev(blob), _dev(off)
    assert edv.merkle_audit_nodes(lh, nodes, 1000, 0, 3)[:2] == (0, None)   # the context exists
    edv.trim(0, 0)
    before = edv.context_memory(0)
    assert dev_nodes(ds, 0, total).read()[0] == (0, ac.NONE)                # the device forms use no context memory
    out = Out(1000)
    edv.merkle_audit_leaves_device(ds.d_leafs.ptr, 1000, 0, d_blob.ptr, d_off.ptr, 1000, out.d_status.ptr,
                                   out.d_summary.ptr)
    assert out.read()[0] == (0, ac.NONE) and edv.context_memory(0) == before
    assert edv.merkle_audit_nodes(lh, nodes, 1000)[:2] == (0, None)
    mid = edv.context_memory(0)
    assert mid["chunk_scratch"] >= before["chunk_scratch"] + len(lh) + len(nodes) + total + 16
    assert edv.merkle_audit_leaves(lh, 1000, 0, blob, off)[:2] == (0, None)
    assert edv.context_memory(0)["chunk_scratch"] >= mid["chunk_scratch"] + int(off[-1]) + 8 * 1001
    edv.trim(0, 2)      # what two entries need is less than the 1,000-leaf store
    assert edv.context_memory(0)["chunk_scratch"] < mid["chunk_scratch"]
    assert edv.merkle_audit_nodes(lh, nodes, 1000)[:2] == (0, None)
    gn, _, _ = edv.merkle_extend_hashed(0, b"", lh)
    assert gn.tobytes() == nodes
    edv.trim(0, 0)
    after = edv.context_memory(0)
    assert (after["total"], after["chunk_scratch"]) == (before["total"], before["chunk_scratch"])
    edv.release(0)
    assert edv.context_memory(0)["total"] == 0
    assert edv.merkle_audit_nodes(lh, nodes, 1000)[:2] == (0, None)
