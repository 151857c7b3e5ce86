"""The Merkle-tree extension on the device (row f-5): edv_merkle_extend and
edv_merkle_extend_dev against the sequential checker of tests/merkle_cases.py
(old frontiers are arbitrary bytes, so huge trees need no real tree), and the
Python tree's device path against the reference's recorded trees."""
import ctypes

import numpy as np
import pytest

import merkle_cases as mc
from indy_plenum_amd import edv, merkle

pytestmark = pytest.mark.gpu

SENTINEL = 0xEE


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


class DevCall:
    """One edv_merkle_extend_dev call's buffers.  The leaf blob sits `shift`
    bytes into its allocation, which ends 8 bytes after the last leaf byte."""

    def __init__(self, old, fr, leaves, want_leaf=True, want_node=True, shift=0, leaf_base=0):
        self.old, self.n = old, len(leaves)
        self.want_leaf, self.want_node = want_leaf, want_node
        blob, off = mc.pack(leaves)
        self.d_leaves = _dev(np.concatenate([np.zeros(shift, np.uint8), blob]), extra=8)
        self.shift, self.leaf_base = shift, leaf_base
        self.d_off = _dev(off + np.uint64(leaf_base))
        self.d_old = _dev(np.frombuffer(b"".join(fr), np.uint8)) if fr else None
        self.nodes = mc.node_span(old, self.n)
        self.nnew = mc.popcount(old + self.n)
        self.d_leafh = _dev(np.full(32 * self.n + 32, SENTINEL, np.uint8))
        self.d_nodeh = _dev(np.full(32 * self.nodes + 32, SENTINEL, np.uint8))
        self.d_new = _dev(np.full(32 * 64, SENTINEL, np.uint8))
        self.d_root = _dev(np.full(32, SENTINEL, np.uint8))

    def run(self, stream=None):
        edv.merkle_extend_device(self.old, self.d_old.ptr if self.d_old else None, self.d_leaves.ptr + self.shift,
                                 self.d_off.ptr, self.n, self.d_leafh.ptr if self.want_leaf else None,
                                 self.d_nodeh.ptr if self.want_node else None, self.d_new.ptr, self.d_root.ptr,
                                 leaf_base=self.leaf_base, stream=stream)
        return self

    def result(self):
        """(leaf_hashes | None, nodes | None, new_hashes, root); nothing written past any output's end."""
        lh, nh = self.d_leafh.download().tobytes(), self.d_nodeh.download().tobytes()
        new, root = self.d_new.download().tobytes(), self.d_root.download().tobytes()
        guard = bytes([SENTINEL]) * 32
        assert lh[32 * self.n:] == guard and nh[32 * self.nodes:] == guard
        assert new[32 * self.nnew:] == bytes([SENTINEL]) * (32 * (64 - self.nnew))
        if not self.want_leaf:
            assert lh == bytes([SENTINEL]) * len(lh)
        if not self.want_node:
            assert nh == bytes([SENTINEL]) * len(nh)
        return (lh[:32 * self.n] if self.want_leaf else None, nh[:32 * self.nodes] if self.want_node else None,
                [new[i:i + 32] for i in range(0, 32 * self.nnew, 32)], root)


def dev_extend(old, fr, leaves, **kw):
    return DevCall(old, fr, leaves, **kw).run().result()


def host_extend(old, fr, leaves, want_leaf=True, want_node=True):
    blob, off = mc.pack(leaves)
    blob = np.concatenate([blob, np.zeros(8, np.uint8)])
    lh, nh, new, root = edv.merkle_extend(old, b"".join(fr), blob, off, want_leaf, want_node)
    return (None if lh is None else lh.tobytes(), None if nh is None else nh.tobytes(), [bytes(r) for r in new], root)


def _case(old, n, max_len=300):
    fr = mc.frontier(old & 0xFFFF, old)
    leaves = mc.leaves_of(old % 1000 + n, n, max_len=max_len)
    return fr, leaves, mc.simulate(old, fr, leaves)


@pytest.mark.parametrize("old,n", mc.grid())
def test_both_entry_points_over_the_grid(old, n):
    fr, leaves, want = _case(old, n)
    assert dev_extend(old, fr, leaves) == want
    assert host_extend(old, fr, leaves) == want


@pytest.mark.parametrize("old", [0, 255])
def test_three_passes(old):
    """More than T^2 leaves: tile roots of tile roots."""
    T = mc.tile()
    n = 65537 if T == 256 else T * T + 1
    fr = mc.frontier(7, old)
    rng = np.random.default_rng(old + 1)
    blob = rng.integers(0, 256, 40 * n, dtype=np.uint8).tobytes()
    leaves = [blob[i:i + 40] for i in range(0, 40 * n, 40)]   # 40-byte leaves
    want = mc.simulate(old, fr, leaves)
    assert dev_extend(old, fr, leaves) == want
    assert host_extend(old, fr, leaves) == want


def test_padding_edge_lengths_mixed_in_one_batch():
    leaves = mc.leaves_of(9, 3 * len(mc.EDGE_LENGTHS), lengths=mc.EDGE_LENGTHS)
    fr = mc.frontier(1, 5)
    want = mc.simulate(5, fr, leaves)
    assert dev_extend(5, fr, leaves) == want
    assert host_extend(5, fr, leaves) == want


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_leaf_buffer_at_the_start_of_its_allocation_and_misaligned(shift):
    """shift 0: leaf 0 starts at byte 0 of its device allocation (nothing before
    it may be read); 1-3: the leaf buffer starts inside a word."""
    leaves = mc.leaves_of(11 + shift, 300, max_len=70)
    leaves[0] = b"first leaf, at the very start"
    fr = mc.frontier(2, 3)
    assert dev_extend(3, fr, leaves, shift=shift) == mc.simulate(3, fr, leaves)


def test_output_combinations_agree():
    old, n = 255, 513
    fr, leaves, want = _case(old, n)
    for want_leaf in (True, False):
        for want_node in (True, False):
            exp = (want[0] if want_leaf else None, want[1] if want_node else None, want[2], want[3])
            assert dev_extend(old, fr, leaves, want_leaf=want_leaf, want_node=want_node) == exp
            assert host_extend(old, fr, leaves, want_leaf, want_node) == exp


def test_leaf_base():
    old, n = 65535, 257
    fr, leaves, want = _case(old, n)
    assert dev_extend(old, fr, leaves, leaf_base=123456789) == want
    assert dev_extend(old, fr, leaves, leaf_base=3, shift=1) == want


def test_two_caller_streams_back_to_back():
    """Both calls need the tile-root scratch (more than one pass); issued
    without a sync between them on two streams, both come out right."""
    s1, s2 = _HipStream(), _HipStream()
    fa, la, wa = _case(255, 70000, max_len=16)
    fb, lb, wb = _case(2 ** 32 - 1, 66000, max_len=16)
    a, b = DevCall(255, fa, la), DevCall(2 ** 32 - 1, fb, lb)
    a.run(stream=s1.ptr)
    b.run(stream=s2.ptr)
    s1.synchronize()
    s2.synchronize()
    assert a.result() == wa
    assert b.result() == wb


def test_argument_errors_launch_nothing():
    fr, leaves, _ = _case(3, 4)
    E = edv.EDV_E_ARG
    lib = edv.lib()
    c = DevCall(3, fr, leaves)
    p = dict(old=c.d_old.ptr, leaves=c.d_leaves.ptr, off=c.d_off.ptr, lh=c.d_leafh.ptr, nh=c.d_nodeh.ptr,
             new=c.d_new.ptr, root=c.d_root.ptr)

    def call(old_size=3, n=4, **kw):
        q = dict(p, **kw)
        return lib.edv_merkle_extend_dev(old_size, q["old"], q["leaves"], q["off"], 0, n, q["lh"], q["nh"], q["new"],
                                         q["root"], 0, None)
    assert call(n=edv.MERKLE_MAX_LEAVES + 1) == E
    assert call(old_size=2 ** 62 - 3) == E
    assert call(old=None) == E
    assert call(off=p["off"] + 4) == E
    for k in ("old", "lh", "nh", "new", "root"):
        assert call(**{k: p[k] + 8}) == E
    assert call(new=None) == E and call(root=None) == E
    assert call(leaves=None) == E and call(off=None) == E
    untouched = c.result()
    assert untouched[2] == [bytes([SENTINEL]) * 32] * c.nnew and untouched[3] == bytes([SENTINEL]) * 32
    assert untouched[0] == bytes([SENTINEL]) * 128
    # the host form: its own list, offsets included
    blob, off = mc.pack(leaves)
    new, root = np.full(64 * 32, SENTINEL, np.uint8), np.full(32, SENTINEL, np.uint8)
    lh = np.full(32 * 4, SENTINEL, np.uint8)
    old = np.frombuffer(b"".join(fr), np.uint8)

    def hcall(old_size=3, oldp=old.ctypes.data, offp=off.ctypes.data, n=4, newp=new.ctypes.data,
              rootp=root.ctypes.data):
        return lib.edv_merkle_extend(old_size, oldp, blob.ctypes.data, offp, n, lh.ctypes.data, None, newp, rootp, 0)
    bad = np.array([0, 5, 3, 6, 7], np.uint64)   # offsets must not decrease
    assert hcall(n=edv.MERKLE_MAX_LEAVES + 1) == E
    assert hcall(old_size=2 ** 62 - 3) == E
    assert hcall(oldp=None) == E
    assert hcall(offp=bad.ctypes.data) == E
    assert hcall(offp=None) == E
    assert hcall(newp=None) == E and hcall(rootp=None) == E
    assert (new == SENTINEL).all() and (root == SENTINEL).all() and (lh == SENTINEL).all()
    # and the same arguments, well formed, go through
    assert hcall() == 0 and c.run().result() == mc.simulate(3, fr, leaves)


@pytest.fixture(scope="module")
def golden():
    return mc.load_golden()


def test_python_tree_device_path_against_golden(golden):
    for case in golden["cases"]:
        leaves = golden["leaves"][:case["size"]]
        t = merkle.CompactMerkleTree()
        t.extend(leaves, on_device=True)
        mc.check_tree_against_golden(t, case, leaves)
    # grown in device calls of 300 and by the automatic choice: same tree, same store
    leaves = golden["leaves"][:1000]
    case = [c for c in golden["cases"] if c["size"] == 1000][0]
    t = merkle.CompactMerkleTree()
    t.extend(leaves, on_device=True, max_call=300)
    mc.check_tree_against_golden(t, case, leaves)
    t = merkle.CompactMerkleTree()
    t.extend(leaves[:merkle.MIN_DEVICE_LEAVES - 1])
    t.append(leaves[merkle.MIN_DEVICE_LEAVES - 1])
    t.extend(leaves[merkle.MIN_DEVICE_LEAVES:])
    mc.check_tree_against_golden(t, case, leaves)


def test_lifecycle_scratch_is_counted_trimmed_and_released():
    fr, leaves, want = _case(255, 70000, max_len=16)
    assert host_extend(0, [], leaves[:10])[3] == mc.simulate(0, [], leaves[:10])[3]   # the context exists
    edv.trim(0, 0)
    before = edv.context_memory(0)
    assert host_extend(255, fr, leaves) == want
    after = edv.context_memory(0)
    assert after["chunk_scratch"] > before["chunk_scratch"] and after["total"] > before["total"]
    # a batch of 100 leaves needs far less than this one left behind
    edv.trim(0, 100)
    assert edv.context_memory(0)["chunk_scratch"] < after["chunk_scratch"]
    edv.trim(0, 0)
    assert edv.context_memory(0)["total"] == before["total"]
    assert host_extend(255, fr, leaves) == want
    assert dev_extend(255, fr, leaves[:1000])[3] == mc.simulate(255, fr, leaves[:1000])[3]
    edv.release(0)
    assert edv.context_memory(0)["total"] == 0
    assert host_extend(255, fr, leaves[:300]) == mc.simulate(255, fr, leaves[:300])
