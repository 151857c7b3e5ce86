"""Cases and an independent checker for batched proof verification (row f-7:
edv_merkle_verify_inclusion / _consistency, hc_merkle_verify_*,
indy_plenum_amd.merkle.MerkleVerifier).

The checker restates the two walks of RFC 6962 sections 2.1.1 and 2.1.2 in
plain Python over hashlib and returns (status, computed), the pair the entry
points write per proof.  It is itself checked (tests/test_merkle_verify_cpu.py)
against the recursive forms of merkle_cases, against every proof recorded in
merkle_golden.json and against the reference's recorded outcomes in
merkle_verify_golden.json.

Large trees need no tree: for a chosen (leaf_index, tree_size) the path is
audit_path_length arbitrary entries from a seeded generator, and the root the
checker computes from them is the root that makes the proof good."""
import ctypes
import json
import os
import random

import numpy as np

import merkle_cases as mc

GOLDEN = os.path.join(mc.ROOT, "tests", "golden", "merkle_verify_golden.json")

UNVERIFIED, OK, RANGE, SHORT, LONG, ROOT, INCONSISTENT = range(7)
STATUS_NAME = {OK: "True", RANGE: "ValueError", SHORT: "ProofError: too short", LONG: "ProofError: too long",
               ROOT: "ProofError: mismatch", INCONSISTENT: "ConsistencyError"}
ZERO = b"\0" * 32
SENTINEL = 0xEE

# the grids of the issue
SIZES = [1, 2, 3, 7, 8, 255, 256, 257, 2 ** 32 - 1, 2 ** 32, 2 ** 32 + 1, 2 ** 62, 2 ** 63 + 5, 2 ** 64 - 1]
BATCH_N = [0, 1, 63, 64, 65, 257]


# ---- the checker
def check_inclusion(leaf_h, index, size, path, root):
    """(status, calculated root or 32 zero bytes)."""
    if not 0 <= index < size:
        return RANGE, ZERO
    node, last, used, acc = index, size - 1, 0, leaf_h
    while last > 0:
        left = node % 2 == 1
        if left or node < last:
            if used >= len(path):
                return SHORT, ZERO
            acc = mc.node_hash(path[used], acc) if left else mc.node_hash(acc, path[used])
            used += 1
        node //= 2
        last //= 2
    if used < len(path):
        return LONG, acc
    return (OK if acc == root else ROOT), acc


def check_consistency(old, new, old_root, new_root, proof):
    """(status, calculated old root + new root, or 64 zero bytes where no walk is made)."""
    if old > new:
        return RANGE, ZERO + ZERO
    if old == new:
        return (OK if old_root == new_root else INCONSISTENT), ZERO + ZERO
    if old == 0:
        return OK, ZERO + ZERO
    node, last = old - 1, new - 1
    while node % 2 == 1:
        node //= 2
        last //= 2
    it = iter(proof)
    try:
        o = n = next(it) if node else old_root
        while node:
            if node % 2 == 1:
                e = next(it)
                o, n = mc.node_hash(e, o), mc.node_hash(e, n)
            elif node < last:
                n = mc.node_hash(n, next(it))
            node //= 2
            last //= 2
        while last:
            n = mc.node_hash(n, next(it))
            last //= 2
    except StopIteration:
        return SHORT, ZERO + ZERO
    if n != new_root:
        return ROOT, o + n
    return (OK if o == old_root else INCONSISTENT), o + n


def path_length(index, size):
    """Entries the audit path of leaf `index` in a tree of `size` leaves has."""
    length, last = 0, size - 1
    while last > 0:
        if index % 2 == 1 or index < last:
            length += 1
        index //= 2
        last //= 2
    return length


def consistency_length(old, new):
    """Entries PROOF(old, D[new]) has, 0 < old < new."""
    node, last = old - 1, new - 1
    while node % 2 == 1:
        node //= 2
        last //= 2
    length = 1 if node else 0
    while last > 0:
        if node % 2 == 1 or node < last:
            length += 1
        node //= 2
        last //= 2
    return length


# ---- cases
def indices(size):
    return sorted({i for i in (0, 1, size // 2, size - 2, size - 1) if 0 <= i < size})


def inclusion_points():
    """(leaf_index, tree_size) over the grid: first, second, middle and the last two leaves of every size."""
    return [(i, s) for s in SIZES for i in indices(s)]


def consistency_points():
    """(old, new): powers of two (the seed is old_root), odd sizes, (m, m + 1), (1, n), (n - 1, n), old deep in
    the right spine (node == last at several levels) and trees of different heights."""
    pts = []
    for new in SIZES[1:]:
        for old in {1, 2, new // 2, new - 1, (1 << (new.bit_length() - 1)), new - (new & -new), 3, 5}:
            if 0 < old < new:
                pts.append((old, new))
    pts += [(7, 8), (8, 9), (255, 256), (256, 257), (254, 255), (2 ** 32, 2 ** 63 + 5), (2 ** 62 + 2 ** 61, 2 ** 64 - 1),
            (2 ** 64 - 2, 2 ** 64 - 1), (2 ** 63 + 4, 2 ** 63 + 5), (6, 7), (4, 7), (1, 2 ** 64 - 1), (192, 257),
            (2 ** 32 - 2 ** 16, 2 ** 32 + 1)]
    return mc_once(pts)


def mc_once(pairs):
    seen, out = set(), []
    for p in pairs:
        if p not in seen:
            seen.add(p)
            out.append(p)
    return out


def _rand32(rng):
    return bytes(rng.getrandbits(8) for _ in range(32))


def _flip(h, k=5):
    return h[:k] + bytes([h[k] ^ 0x40]) + h[k + 1:]


class InclusionBatch:
    """n proofs as lists: leaves (bytes), index, size, root (bytes), proof (list of 32-byte entries)."""

    def __init__(self):
        self.leaves, self.index, self.size, self.root, self.proof, self.hashes = [], [], [], [], [], []

    def add(self, leaf, index, size, root, proof, leaf_hash=None):
        """leaf None: only its hash is known."""
        self.leaves.append(leaf)
        self.hashes.append(mc.leaf_hash(leaf) if leaf_hash is None else leaf_hash)
        self.index.append(index)
        self.size.append(size)
        self.root.append(root)
        self.proof.append(list(proof))

    def __len__(self):
        return len(self.leaves)

    def leaf_hashes(self):
        return list(self.hashes)

    def expected(self):
        """(statuses, computed): n bytes and n x 32 bytes, by the checker."""
        res = [check_inclusion(*row) for row in zip(self.hashes, self.index, self.size, self.proof, self.root)]
        return bytes(st for st, _ in res), b"".join(c for _, c in res)


class ConsistencyBatch:
    def __init__(self):
        self.old, self.new, self.old_root, self.new_root, self.proof = [], [], [], [], []

    def add(self, old, new, old_root, new_root, proof):
        self.old.append(old)
        self.new.append(new)
        self.old_root.append(old_root)
        self.new_root.append(new_root)
        self.proof.append(list(proof))

    def __len__(self):
        return len(self.old)

    def expected(self):
        res = [check_consistency(*row) for row in zip(self.old, self.new, self.old_root, self.new_root, self.proof)]
        return bytes(st for st, _ in res), b"".join(c for _, c in res)


MUTATIONS = 8


def synth_inclusion(points, seed=1, mutate=True, lengths=mc.EDGE_LENGTHS):
    """A batch over `points` with arbitrary path entries; the good root is the one the checker calculates.
    With mutate, proof k is changed by k % MUTATIONS: 0 and 7 intact, 1 wrong root, 2 last entry dropped (an
    empty path: one appended), 3 one entry appended, 4 leaf_index = tree_size, 5 a bit flipped in the first
    entry, 6 in the last (an empty path: in the leaf)."""
    rng = random.Random(0xF7 * 1000003 + seed)
    b = InclusionBatch()
    for k, (index, size) in enumerate(points):
        ln = lengths[k % len(lengths)]
        leaf = rng.getrandbits(8 * ln).to_bytes(ln, "little") if ln else b""
        path = [_rand32(rng) for _ in range(path_length(index, size))]
        st, root = check_inclusion(mc.leaf_hash(leaf), index, size, path, None)
        assert st == ROOT
        m = k % MUTATIONS if mutate else 0
        if m == 1:
            root = _flip(root)
        elif m == 2 and path:
            path = path[:-1]
        elif m in (2, 3):
            path = path + [_rand32(rng)]
        elif m == 4:
            index = size
        elif m == 5 and path:
            path[0] = _flip(path[0])
        elif m == 6 and path:
            path[-1] = _flip(path[-1], 31)
        elif m in (5, 6):
            leaf = leaf + b"x"
        b.add(leaf, index, size, root, path)
    return b


def synth_consistency(points, seed=1, mutate=True):
    """As synth_inclusion: arbitrary entries of the right count, old_root arbitrary where it is the seed and
    otherwise the calculated one.  Mutation k % MUTATIONS: 0 intact, 1 wrong new root, 2 last entry dropped, 3
    one entry appended (accepted), 4 old and new swapped, 5 wrong old root (inconsistent, unless old_root is
    the seed: then the new root moves too), 6 equal sizes with the old root for both, 7 old = 0 with the proof
    kept."""
    rng = random.Random(0xF7C * 1000003 + seed)
    b = ConsistencyBatch()
    for k, (old, new) in enumerate(points):
        proof = [_rand32(rng) for _ in range(consistency_length(old, new))]
        old_root = _rand32(rng)
        st, comp = check_consistency(old, new, old_root, None, proof)
        assert st == ROOT
        if comp[:32] != old_root:       # old is no power of two: the proof alone gives the old root
            old_root = comp[:32]
        new_root = comp[32:]
        m = k % MUTATIONS if mutate else 0
        if m == 1:
            new_root = _flip(new_root)
        elif m == 2 and proof:
            proof = proof[:-1]
        elif m == 3:
            proof = proof + [_rand32(rng)]
        elif m == 4:
            old, new, old_root, new_root = new, old, new_root, old_root
        elif m == 5:
            old_root = _flip(old_root)
        elif m == 6:
            new, new_root = old, (old_root if k % 16 == 6 else new_root)
        elif m == 7:
            old = 0
        b.add(old, new, old_root, new_root, proof)
    return b


def interleaved_inclusion_points(n=64):
    """n points whose mutated batch carries every inclusion status in one wave, interleaved, with long and
    short walks side by side."""
    pts = inclusion_points()
    return [pts[(k * 7) % len(pts)] for k in range(n)]


# ---- packing
def pack_hashes(hs):
    return np.frombuffer(b"".join(hs), np.uint8).copy() if hs else np.zeros(0, np.uint8)


def pack_proofs(proofs, base=0):
    """(uint8 entries, uint64 offsets in entries starting at `base`, with `base` filler entries in front)."""
    off = np.zeros(len(proofs) + 1, np.uint64)
    if proofs:
        off[1:] = np.cumsum([len(p) for p in proofs], dtype=np.uint64)
    off += np.uint64(base)
    blob = np.frombuffer(b"\xA5" * (32 * base) + b"".join(h for p in proofs for h in p), np.uint8).copy()
    return blob, off


def u64(xs):
    return np.array(list(xs), dtype=np.uint64)


# ---- hc_merkle_verify_* (the kernels' code on the CPU)
_bound = False


def hostcheck():
    global _bound
    lib = mc.hostcheck()
    if not _bound:
        vp = ctypes.c_void_p
        lib.hc_merkle_verify_inclusion.argtypes = [vp] * 8 + [ctypes.c_uint64, vp, vp]
        lib.hc_merkle_verify_inclusion.restype = ctypes.c_int
        lib.hc_merkle_verify_consistency.argtypes = [vp] * 6 + [ctypes.c_uint64, vp, vp]
        lib.hc_merkle_verify_consistency.restype = ctypes.c_int
        _bound = True
    return lib


def _p(a):
    return None if a is None else a.ctypes.data


def _outs(n, cbytes, want_computed):
    status = np.full(n + 32, SENTINEL, np.uint8)
    computed = np.full(cbytes * n + 32, SENTINEL, np.uint8)
    return status, computed


def _read_outs(n, cbytes, status, computed, want_computed):
    """(statuses, computed | None); 32 sentinel bytes after each output are intact, a NULL computed untouched."""
    guard = bytes([SENTINEL]) * 32
    s, c = status.tobytes(), computed.tobytes()
    assert s[n:] == guard and c[cbytes * n:] == guard
    if not want_computed:
        assert c == bytes([SENTINEL]) * len(c)
    return s[:n], (c[:cbytes * n] if want_computed else None)


def hc_inclusion(b, by_hash=False, want_computed=True, leaf_base=0, proof_base=0):
    n = len(b)
    blob = loff = None
    if not by_hash:
        blob, loff = mc.pack(b.leaves, leaf_base)
        blob = np.concatenate([blob, np.zeros(8, np.uint8)])
    lh = pack_hashes(b.leaf_hashes())
    proofs, poff = pack_proofs(b.proof, proof_base)
    roots, idx, size = pack_hashes(b.root), u64(b.index), u64(b.size)
    status, computed = _outs(n, 32, want_computed)
    rc = hostcheck().hc_merkle_verify_inclusion(
        _p(blob), _p(loff), _p(lh) if by_hash else None, _p(idx), _p(size),
        _p(roots), _p(proofs), _p(poff), n, _p(status), _p(computed) if want_computed else None)
    assert rc == 0
    return _read_outs(n, 32, status, computed, want_computed)


def hc_consistency(b, want_computed=True, proof_base=0):
    n = len(b)
    proofs, poff = pack_proofs(b.proof, proof_base)
    status, computed = _outs(n, 64, want_computed)
    old, new, old_roots, new_roots = u64(b.old), u64(b.new), pack_hashes(b.old_root), pack_hashes(b.new_root)
    rc = hostcheck().hc_merkle_verify_consistency(
        _p(old), _p(new), _p(old_roots), _p(new_roots), _p(proofs), _p(poff), n, _p(status),
        _p(computed) if want_computed else None)
    assert rc == 0
    return _read_outs(n, 64, status, computed, want_computed)


# ---- the reference's recorded outcomes
# merkle_verify_golden.json holds every proof of the ten recorded trees once, with the outcome the reference's
# MerkleVerifier gave for it intact and after each of the mutations below (applied here and, identically, by
# tests/golden/make_merkle_verify_golden.py, which imports them).
JUNK = b"\x5a" * 32
INCLUSION_MUTATIONS = ("intact", "drop_last", "append_one", "flip_first", "flip_last", "wrong_root", "index_is_size")
CONSISTENCY_MUTATIONS = ("intact", "drop_last", "append_one", "flip_first", "flip_last", "wrong_root", "wrong_old_root",
                         "swapped", "equal_sizes_equal_roots", "equal_sizes_different_roots", "old_zero_junk")


def _mutate_proof(proof, name):
    proof = list(proof)
    if name == "drop_last":
        return proof[:-1]
    if name == "append_one":
        return proof + [JUNK]
    if name == "flip_first" and proof:
        proof[0] = _flip(proof[0], 0)
    if name == "flip_last" and proof:
        proof[-1] = _flip(proof[-1], 31)
    return proof


def mutate_inclusion(leaf_hash, m, n, proof, root, name):
    """(leaf_hash, m, n, proof, root) after the mutation."""
    assert name in INCLUSION_MUTATIONS
    if name == "wrong_root":
        root = _flip(root)
    if name == "index_is_size":
        m = n
    return leaf_hash, m, n, _mutate_proof(proof, name), root


def mutate_consistency(a, b, root_a, root_b, proof, name):
    """(a, b, root_a, root_b, proof) after the mutation."""
    assert name in CONSISTENCY_MUTATIONS
    if name == "wrong_root":
        root_b = _flip(root_b)
    elif name == "wrong_old_root":
        root_a = _flip(root_a)
    elif name == "swapped":
        a, b, root_a, root_b = b, a, root_b, root_a
    elif name == "equal_sizes_equal_roots":
        b, root_b, proof = a, root_a, list(proof) + [JUNK]
    elif name == "equal_sizes_different_roots":
        b, root_b = a, _flip(root_a)
    elif name == "old_zero_junk":
        a, proof = 0, [JUNK, JUNK]
    return a, b, root_a, root_b, _mutate_proof(proof, name)


def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_batches(g):
    """(InclusionBatch by leaf hash, its recorded statuses, ConsistencyBatch, its recorded statuses): every
    recorded proof under every mutation."""
    name_to_status = {v: k for k, v in STATUS_NAME.items()}
    inc, inc_st, con, con_st = InclusionBatch(), [], ConsistencyBatch(), []
    for c in g["inclusion"]:
        base = (bytes.fromhex(c["leaf_hash"]), c["m"], c["n"], [bytes.fromhex(h) for h in c["proof"]],
                bytes.fromhex(c["root"]))
        for name in INCLUSION_MUTATIONS:
            lh, m, n, proof, root = mutate_inclusion(*base, name)
            inc.add(None, m, n, root, proof, lh)
            inc_st.append(name_to_status[c["outcomes"][name]])
    for c in g["consistency"]:
        base = (c["a"], c["b"], bytes.fromhex(c["root_a"]), bytes.fromhex(c["root_b"]),
                [bytes.fromhex(h) for h in c["proof"]])
        for name in CONSISTENCY_MUTATIONS:
            con.add(*mutate_consistency(*base, name))
            con_st.append(name_to_status[c["outcomes"][name]])
    return inc, bytes(inc_st), con, bytes(con_st)
