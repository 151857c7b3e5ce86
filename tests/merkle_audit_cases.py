"""Cases and an independent checker for the hash-store audit (row f-9:
edv_merkle_audit_nodes / _leaves, edv_merkle_extend_hashed, hc_merkle_audit_*,
CompactMerkleTree.audit_store / rebuild_nodes / extend_hashed).

expected_bad restates the store's invariant forwards: for every block (h, k)
that a tree of the stored leaf count has, the node at node_position(h, k) must
be the hash of the two stored children.  It uses hashlib and the package's
node_position only; it knows nothing of the inverse position function, the
lanes or the summary of edv_merkle.h, and it reads the stored bytes, damaged as
they are, never what the code under test says about them."""
import ctypes
import hashlib

import numpy as np

import merkle_cases as mc
import merkle_prove_cases as pc
from indy_plenum_amd.merkle import node_position

UNCHECKED, OK, BAD = 0, 1, 2
NONE = 2 ** 64 - 1
PATTERN = 0xC3          # what outputs hold before a call
GUARD = 0x5A            # what lies behind a store's last entry
MUTATIONS = ["clean", "first", "last", "highest", "height1", "leafhash", "swap", "short", "long"]


def sizes():
    """The smallest sizes at which each part can go wrong: no node, one node,
    around a tile of the extend, the reference's recorded store, three extend passes."""
    t = mc.tile()
    return [0, 1, 2, 3, 4, 5, 7, 8, 9, t - 1, t, t + 1, 1000, 2 * t * t + 3]


def expected_nodes(nleaves):
    return nleaves - mc.popcount(nleaves)


def expected_bad(leaf_store, node_store):
    """Sorted 0-based positions of the stored nodes whose stored children do
    not hash to them, among the nodes that are both stored and the leaf count's."""
    nleaves, nnodes = len(leaf_store) // 32, len(node_store) // 32
    have = min(nnodes, expected_nodes(nleaves))
    sha = hashlib.sha256
    bad = []
    h = 1
    while (1 << h) <= nleaves:
        for k in range(nleaves >> h):
            q = node_position(h, k) - 1
            if q >= have:
                continue
            if h == 1:
                children = leaf_store[64 * k:64 * k + 64]
            else:
                pl, pr = node_position(h - 1, 2 * k) - 1, node_position(h - 1, 2 * k + 1) - 1
                children = node_store[32 * pl:32 * pl + 32] + node_store[32 * pr:32 * pr + 32]
            if sha(b"\x01" + children).digest() != node_store[32 * q:32 * q + 32]:
                bad.append(q)
        h += 1
    return sorted(bad)


def expected_bad_leaves(leaf_store, leaves):
    return [i for i, leaf in enumerate(leaves) if mc.leaf_hash(leaf) != leaf_store[32 * i:32 * i + 32]]


# ---- stores
_stores = {}


def store(size):
    """(leaves, leaf store bytes, node store bytes) of `size` leaves: the
    reference's recorded 1,000 leaves, else seeded ones, by merkle_cases.simulate."""
    if size not in _stores:
        if size == 1000:
            leaves = pc.load_golden()["leaf_list"]
            _, lh, nodes = pc.golden_store()
        else:
            leaves = mc.leaves_of(0xA0D17, size, max_len=70 if size < 4096 else 24)
            lh, nodes, _, _ = mc.simulate(0, [], leaves)
        assert len(lh) == 32 * size and len(nodes) == 32 * expected_nodes(size)
        _stores[size] = (leaves, lh, nodes)
    return _stores[size]


def flip(buf, entry, bit):
    b = bytearray(buf)
    b[32 * entry + bit // 8] ^= 1 << (bit % 8)
    return bytes(b)


def mutate(size, name):
    """(leaf store, node store) with one mutation, or None where the store has nothing to apply it to."""
    _, lh, nodes = store(size)
    nn = len(nodes) // 32
    if name == "clean":
        return lh, nodes
    if name == "long":
        return lh, nodes + hashlib.sha256(b"one entry too many").digest()
    if nn == 0:
        return None
    if name == "first":
        return lh, flip(nodes, 0, 5)
    if name == "last":
        return lh, flip(nodes, nn - 1, 255)
    if name == "highest":
        top = size.bit_length() - 1
        return lh, flip(nodes, node_position(top, 0) - 1, 77)
    if name == "height1":
        k = (size // 2) // 2                     # a block in the middle
        return lh, flip(nodes, node_position(1, k) - 1, 130)
    if name == "leafhash":
        return flip(lh, (size // 3) | 1 if size > 3 else 0, 9), nodes
    if name == "swap":
        if nn < 2:
            return None
        b = bytearray(nodes)
        i, j = nn // 3, nn - 1
        b[32 * i:32 * i + 32], b[32 * j:32 * j + 32] = nodes[32 * j:32 * j + 32], nodes[32 * i:32 * i + 32]
        return lh, bytes(b)
    if name == "short":
        return lh, nodes[:-32]
    raise ValueError(name)


_cases = {}


def cases(size):
    """[(name, leaf store, node store, expected bad positions)] for every mutation that applies."""
    if size not in _cases:
        out = []
        for name in MUTATIONS:
            m = mutate(size, name)
            if m is not None:
                out.append((name, m[0], m[1], expected_bad(m[0], m[1])))
        _cases[size] = out
    return _cases[size]


def summary_of(bad):
    return (len(bad), bad[0] if bad else NONE)


def status_of(bad, lo, count):
    st = bytearray([OK]) * count
    for q in bad:
        if lo <= q < lo + count:
            st[q - lo] = BAD
    return bytes(st)


def slices(have):
    """Slices (lo, count) of a store's `have` checkable nodes: the whole, and
    pieces whose starts and lengths are no multiples of 64."""
    out = [(0, have)]
    if have >= 3:
        out += [(1, have - 2), (have // 3, have - have // 3)]
    if have > 200:
        out += [(0, 65), (65, 127), (191, have - 191), (have - 1, 1), (63, 0)]
    return out


def padded_nodes(nodes, nleaves):
    """The node store as a buffer of the leaf count's length: a store cut short
    is filled up with GUARD bytes (never read: the count passed is the store's own)."""
    want = 32 * expected_nodes(nleaves)
    return nodes[:want].ljust(want, bytes([GUARD]))


# ---- hc_merkle_audit_* (the header's code on the CPU)
_bound = False


def hostcheck():
    global _bound
    lib = mc.hostcheck()
    if not _bound:
        vp, u = ctypes.c_void_p, ctypes.c_uint64
        lib.hc_merkle_store_node_at.argtypes = [u, ctypes.POINTER(u), ctypes.POINTER(ctypes.c_int32)]
        lib.hc_merkle_store_node_at.restype = ctypes.c_int
        lib.hc_merkle_audit_nodes.argtypes = [vp, vp, u, u, u, vp, vp]
        lib.hc_merkle_audit_nodes.restype = ctypes.c_int
        lib.hc_merkle_audit_leaves.argtypes = [vp, u, u, vp, vp, u, vp, vp]
        lib.hc_merkle_audit_leaves.restype = ctypes.c_int
        lib.hc_merkle_extend_hashed.argtypes = [u, vp, vp, u, vp, vp, vp]
        lib.hc_merkle_extend_hashed.restype = ctypes.c_int
        lib.hc_merkle_audit_nodes_needs.argtypes = [u, u, vp, vp]
        lib.hc_merkle_audit_nodes_needs.restype = None
        lib.hc_merkle_audit_leaves_needs.argtypes = [u, u, vp]
        lib.hc_merkle_audit_leaves_needs.restype = None
        lib.hc_merkle_extend_hashed_needs.argtypes = [u, u, ctypes.c_int, ctypes.c_int, vp]
        lib.hc_merkle_extend_hashed_needs.restype = None
        lib.hc_merkle_audit_consts.argtypes = [vp]
        lib.hc_merkle_audit_consts.restype = None
        _bound = True
    return lib


def node_at(q):
    s, h = ctypes.c_uint64(0), ctypes.c_int32(0)
    assert hostcheck().hc_merkle_store_node_at(q, ctypes.byref(s), ctypes.byref(h)) == 1
    return int(s.value), int(h.value)


def arr(b):
    return np.frombuffer(bytes(b) or b"\0", np.uint8)


def hc_audit_nodes(lh, nodes, lo, count, want_status=True):
    """-> ((bad, first), status | None); the status buffer's guard is checked."""
    nleaves = len(lh) // 32
    la, na = arr(lh), arr(padded_nodes(nodes, nleaves))
    st = np.full(count + 32, PATTERN, np.uint8)
    summ = np.full(2, 7, np.uint64)
    rc = hostcheck().hc_merkle_audit_nodes(la.ctypes.data, na.ctypes.data, nleaves, lo, count,
                                           st.ctypes.data if want_status else None, summ.ctypes.data)
    assert rc == 0
    assert st[count:].tobytes() == bytes([PATTERN]) * 32
    if not want_status:
        assert st.tobytes() == bytes([PATTERN]) * (count + 32)
    return (int(summ[0]), int(summ[1])), (st[:count].tobytes() if want_status else None)


def hc_audit_leaves(lh, lo, leaves, base=0, want_status=True):
    nleaves, n = len(lh) // 32, len(leaves)
    blob, off = mc.pack(leaves, base)
    blob = np.concatenate([blob, np.zeros(8, np.uint8)])
    la = arr(lh)
    st = np.full(n + 32, PATTERN, np.uint8)
    summ = np.full(2, 7, np.uint64)
    rc = hostcheck().hc_merkle_audit_leaves(la.ctypes.data, nleaves, lo, blob.ctypes.data, off.ctypes.data, n,
                                            st.ctypes.data if want_status else None, summ.ctypes.data)
    assert rc == 0
    assert st[n:].tobytes() == bytes([PATTERN]) * 32
    return (int(summ[0]), int(summ[1])), (st[:n].tobytes() if want_status else None)


def hc_extend_hashed(old, old_hashes, leaf_hashes, want_node=True):
    """hc_merkle_extend_hashed -> (nodes | None, new_hashes list, root)."""
    n = len(leaf_hashes) // 32
    oh = arr(b"".join(old_hashes))
    la = arr(leaf_hashes)
    nh = np.full(32 * mc.node_span(old, n) + 32, PATTERN, np.uint8)
    new = np.zeros(32 * mc.popcount(old + n) + 32, np.uint8)
    root = np.zeros(32, np.uint8)
    rc = hostcheck().hc_merkle_extend_hashed(old, oh.ctypes.data if old_hashes else None, la.ctypes.data if n else None,
                                             n, nh.ctypes.data if want_node else None, new.ctypes.data, root.ctypes.data)
    assert rc == 0
    assert nh[len(nh) - 32:].tobytes() == bytes([PATTERN]) * 32
    nb = new.tobytes()[:32 * mc.popcount(old + n)]
    return (nh[:-32].tobytes() if want_node else None, [nb[i:i + 32] for i in range(0, len(nb), 32)], root.tobytes())
