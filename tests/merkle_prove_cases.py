"""Cases and an independent checker for batched proof generation (row f-8:
edv_merkle_prove_inclusion / _consistency, hc_merkle_prove_*,
CompactMerkleTree.*_batch).

The checker restates PATH and PROOF of RFC 6962 sections 2.1.1 and 2.1.2 as
the recursive definitions they are, over a list of leaf hashes with hashlib
and a memo of MTH; it knows nothing of the walk, the store positions or the
fold of edv_merkle.h.  It is itself checked against the reference's recorded
results (tests/golden/merkle_prove_golden.json).  expected_inclusion /
expected_consistency give what the entry points write for a whole batch:
status, slots (untouched where nothing is to be written), roots, leaf hashes."""
import ctypes
import hashlib
import json
import os

import numpy as np

import merkle_cases as mc
import merkle_verify_cases as vc

GOLDEN = os.path.join(mc.ROOT, "tests", "golden", "merkle_prove_golden.json")
OK, RANGE, SPACE = vc.OK, vc.RANGE, 7
ZERO = b"\0" * 32
PATTERN = 0xC3   # what the outputs hold before a call
LARGE = [255, 256, 257, 777, 1000]
KIND_LEAF, KIND_NODE, KIND_FOLD = 0, 1, 2
MAX_PROOF = 63


# ---- the checker
def split(n):
    """Largest power of two below n >= 2."""
    return 1 << ((n - 1).bit_length() - 1)


def path_ranges(m, lo, hi):
    """PATH(m, D[lo:hi]) as ranges [a, b), lowest level first."""
    n = hi - lo
    if n == 1:
        return []
    k = split(n)
    if m < k:
        return path_ranges(m, lo, lo + k) + [(lo + k, hi)]
    return path_ranges(m - k, lo + k, hi) + [(lo, lo + k)]


def subproof_ranges(m, lo, hi, whole):
    """SUBPROOF(m, D[lo:hi], whole)."""
    n = hi - lo
    if m == n:
        return [] if whole else [(lo, hi)]
    k = split(n)
    if m <= k:
        return subproof_ranges(m, lo, lo + k, whole) + [(lo + k, hi)]
    return subproof_ranges(m - k, lo + k, hi, False) + [(lo, lo + k)]


def proof_ranges(consistency, a, n):
    return subproof_ranges(a, 0, n, True) if consistency else path_ranges(a, 0, n)


class Tree:
    """MTH over a fixed list of leaf hashes, memoized."""

    def __init__(self, leaf_hashes):
        self.lh = list(leaf_hashes)
        self.memo = {}

    def mth(self, a, b):
        if b - a == 1:
            return self.lh[a]
        key = (a, b)
        if key not in self.memo:
            k = split(b - a)
            self.memo[key] = mc.node_hash(self.mth(a, a + k), self.mth(a + k, b))
        return self.memo[key]

    def root(self, n):
        return self.mth(0, n) if n else mc.EMPTY_ROOT

    def inclusion(self, m, n):
        return [self.mth(a, b) for a, b in path_ranges(m, 0, n)]

    def consistency(self, a, n):
        return [self.mth(x, y) for x, y in subproof_ranges(a, 0, n, True)]


def inclusion_status(m, n, store_leaves, slot):
    if m >= n or n > store_leaves:
        return RANGE
    return OK if slot == len(path_ranges(m, 0, n)) else SPACE


def consistency_status(a, n, store_leaves, slot):
    if a == 0 or a > n or n > store_leaves:
        return RANGE
    return OK if slot == len(subproof_ranges(a, 0, n, True)) else SPACE


def expected(tree, consistency, pairs, store_leaves, off):
    """(status, slots, out1, out2) a call over slots of PATTERN bytes leaves
    behind: off in entries, slots covering [off[0], off[-1])."""
    base = int(off[0])
    slots = bytearray([PATTERN]) * (32 * (int(off[-1]) - base))
    status, out1, out2 = [], [], []
    for i, (a, n) in enumerate(pairs):
        slot = int(off[i + 1]) - int(off[i])
        st = (consistency_status if consistency else inclusion_status)(a, n, store_leaves, slot)
        status.append(st)
        if st != OK:
            out1.append(ZERO)
            out2.append(ZERO)
            continue
        proof = tree.consistency(a, n) if consistency else tree.inclusion(a, n)
        lo = 32 * (int(off[i]) - base)
        slots[lo:lo + 32 * len(proof)] = b"".join(proof)
        out1.append(tree.root(a) if consistency else tree.root(n))
        out2.append(tree.root(n) if consistency else tree.lh[a])
    return bytes(status), bytes(slots), b"".join(out1), b"".join(out2)


# ---- positions: what the header's positions function must give
def positions(consistency, a, n):
    """[(kind, value)] per entry: a leaf's or a node's byte offset into its
    store (by the package's node_position), or KIND_FOLD with the range's start."""
    from indy_plenum_amd.merkle import node_position
    out = []
    for lo, hi in proof_ranges(consistency, a, n):
        w = hi - lo
        if w == 1:
            out.append((KIND_LEAF, 32 * lo))
        elif w & (w - 1) == 0 and lo % w == 0:
            h = w.bit_length() - 1
            out.append((KIND_NODE, 32 * (node_position(h, lo >> h) - 1)))
        else:
            assert hi == n, "only a range that ends at the tree size may be cut off"
            out.append((KIND_FOLD, lo))
    return out


def big_sizes():
    return [2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 32 + 12345, 2 ** 62 - 1, 2 ** 62 - 2 ** 31 - 7, 2 ** 61 + 2 ** 33 + 5]


def big_indices(n):
    idx = {0, 1, n - 1}
    for k in range(1, 63):
        idx.update((2 ** k - 1, 2 ** k + 1))
    return sorted(i for i in idx if 0 <= i < n)


# ---- cases
def all_pairs(n, consistency):
    return [(a, n) for a in range(1, n + 1)] if consistency else [(m, n) for m in range(n)]


def range_cases(consistency, store_leaves):
    s = store_leaves
    if consistency:
        return [(0, 5), (0, 0), (6, 5), (s, s + 1), (1, s + 1), (s + 1, s + 1), (2 ** 64 - 1, 3), (1, 2 ** 64 - 1)]
    return [(5, 5), (6, 5), (0, 0), (0, s + 1), (s, s + 1), (2 ** 64 - 1, 2 ** 64 - 1), (3, 2 ** 63), (2 ** 64 - 1, 7)]


def exact_offsets(consistency, pairs, store_leaves, base=0):
    off = [base]
    for a, n in pairs:
        st = (consistency_status if consistency else inclusion_status)(a, n, store_leaves, -1)
        off.append(off[-1] + (0 if st == RANGE else len(proof_ranges(consistency, a, n))))
    return np.array(off, dtype=np.uint64)


def one_wave(consistency, store_leaves):
    """(pairs, off): 64 proofs holding an empty proof, the longest available,
    first == second, every RANGE case, a slot one entry short, one entry long,
    and good proofs between them; off from entry 3 on (a proof_base)."""
    s = store_leaves
    good = [(1, 1), (s, s), (s - 1, s), (1, s), (5, 11), (s // 2, s)] if consistency else \
        [(0, 1), (s - 2, s - 1), (0, s), (s - 1, s), (8, 11), (s // 2, s)]
    rng = range_cases(consistency, s)
    pairs = []
    for k in range(64):
        pairs.append(rng[k // 3 % len(rng)] if k % 3 == 1 and k // 3 < len(rng) else good[k % len(good)])
    off = exact_offsets(consistency, pairs, s, base=3).astype(np.int64)
    fits = [i for i, (a, n) in enumerate(pairs)
            if (consistency_status if consistency else inclusion_status)(a, n, s, -1) != RANGE
            and off[i + 1] - off[i] > 0]
    short, long_ = fits[2], fits[5]
    off[short + 1:] -= 1
    off[long_ + 1:] += 1
    # a RANGE pair with a slot of its own: nothing is written there either
    first_range = next(i for i, p in enumerate(pairs) if p in rng)
    off[first_range + 1:] += 2
    return pairs, off.astype(np.uint64), short, long_


def u64(xs):
    return np.array(list(xs), dtype=np.uint64)


# ---- the golden fixture
def load_golden():
    with open(GOLDEN) as f:
        g = json.load(f)
    g["leaf_list"] = mc.leaves_of(g["seed"], g["leaves"], max_len=g["max_len"])
    return g


_store = None


def golden_store():
    """(leaf hashes as a list, leaf store bytes, node store bytes) of the 1,000
    golden leaves, by merkle_cases.simulate: n appends on a stack."""
    global _store
    if _store is None:
        g = load_golden()
        lh, nodes, _, _ = mc.simulate(0, [], g["leaf_list"])
        _store = ([lh[i:i + 32] for i in range(0, len(lh), 32)], lh, nodes)
    return _store


def store_prefix(n):
    """The two stores of the first n golden leaves: prefixes of the whole."""
    _, lh, nodes = golden_store()
    return lh[:32 * n], nodes[:32 * (n - mc.popcount(n))]


def digest(proofs):
    return hashlib.sha256(b"".join(h for p in proofs for h in p)).hexdigest()


# ---- hc_merkle_prove_* (the kernels' code on the CPU)
_bound = False


def hostcheck():
    global _bound
    lib = mc.hostcheck()
    if not _bound:
        vp, u = ctypes.c_void_p, ctypes.c_uint64
        for f in (lib.hc_merkle_prove_inclusion, lib.hc_merkle_prove_consistency):
            f.argtypes = [vp, vp, u, vp, vp, vp, u, vp, vp, vp, vp]
            f.restype = ctypes.c_int
        lib.hc_merkle_inclusion_length.argtypes = lib.hc_merkle_consistency_length.argtypes = [u, u]
        lib.hc_merkle_inclusion_length.restype = lib.hc_merkle_consistency_length.restype = u
        lib.hc_merkle_proof_positions.argtypes = [ctypes.c_int, u, u, vp, vp]
        lib.hc_merkle_proof_positions.restype = ctypes.c_int
        lib.hc_merkle_prove_offsets.argtypes = [ctypes.c_int, vp, vp, u, u, vp]
        lib.hc_merkle_prove_offsets.restype = None
        lib.hc_merkle_prove_prefix.argtypes = [ctypes.c_int, vp, vp, u, u]
        lib.hc_merkle_prove_prefix.restype = u
        lib.hc_merkle_prove_needs.argtypes = [u, u, u, ctypes.c_int, ctypes.c_int, vp]
        lib.hc_merkle_prove_needs.restype = None
        lib.hc_merkle_trim_limits_all.argtypes = [u, vp]
        lib.hc_merkle_trim_limits_all.restype = None
        lib.hc_merkle_prove_out.argtypes = [u, ctypes.c_int, ctypes.c_int, vp]
        lib.hc_merkle_prove_out.restype = None
        lib.hc_merkle_prove_consts.argtypes = [vp]
        lib.hc_merkle_prove_consts.restype = None
        _bound = True
    return lib


def hc_positions(consistency, a, n):
    kind = np.zeros(MAX_PROOF + 1, np.uint8)
    off = np.zeros(MAX_PROOF + 1, np.uint64)
    cnt = hostcheck().hc_merkle_proof_positions(int(consistency), a, n, kind.ctypes.data, off.ctypes.data)
    assert 0 <= cnt <= MAX_PROOF
    return [(int(kind[i]), int(off[i])) for i in range(cnt)]


def hc_offsets(consistency, pairs, store_leaves):
    a, b = u64(p[0] for p in pairs), u64(p[1] for p in pairs)
    off = np.zeros(len(pairs) + 1, np.uint64)
    hostcheck().hc_merkle_prove_offsets(int(consistency), a.ctypes.data, b.ctypes.data, len(pairs), store_leaves,
                                        off.ctypes.data)
    return off


def run_outputs(n, entries, want1=True, want2=True):
    """Output buffers holding PATTERN, with 32 guard bytes behind each."""
    mk = lambda nbytes: np.full(nbytes + 32, PATTERN, np.uint8)  # noqa: E731
    return mk(32 * entries), mk(n), mk(32 * n), mk(32 * n)


def read_outputs(n, entries, bufs, want1=True, want2=True):
    """(status, slots, out1 | None, out2 | None); guards intact, outputs not asked for untouched."""
    guard = bytes([PATTERN]) * 32
    slots, status, o1, o2 = (b.tobytes() for b in bufs)
    assert slots[32 * entries:] == guard and status[n:] == guard and o1[32 * n:] == guard and o2[32 * n:] == guard
    if not want1:
        assert o1 == bytes([PATTERN]) * len(o1)
    if not want2:
        assert o2 == bytes([PATTERN]) * len(o2)
    return status[:n], slots[:32 * entries], (o1[:32 * n] if want1 else None), (o2[:32 * n] if want2 else None)


def hc_prove(consistency, store_leaves, pairs, off, want1=True, want2=True):
    """hc_merkle_prove_* over the first store_leaves golden leaves.  off may
    start above 0: the slots buffer then starts at entry off[0] (the harness
    reads and writes [off[0], off[-1]) only)."""
    n, base, entries = len(pairs), int(off[0]), int(off[-1]) - int(off[0])
    leafs, nodes = store_prefix(store_leaves)
    la = np.frombuffer(leafs + b"\0", np.uint8)
    na = np.frombuffer(nodes + b"\0", np.uint8)
    a, b = u64(p[0] for p in pairs), u64(p[1] for p in pairs)
    bufs = run_outputs(n, entries)
    slots = bufs[0]
    fn = hostcheck().hc_merkle_prove_consistency if consistency else hostcheck().hc_merkle_prove_inclusion
    rc = fn(la.ctypes.data, na.ctypes.data, store_leaves, a.ctypes.data, b.ctypes.data, off.ctypes.data, n,
            slots.ctypes.data - 32 * base, bufs[1].ctypes.data, bufs[2].ctypes.data if want1 else None,
            bufs[3].ctypes.data if want2 else None)
    assert rc == 0
    return read_outputs(n, entries, bufs, want1, want2)
