"""Cases and an independent model for catch-up in one call (row f-10:
edv_merkle_catchup, hc_merkle_catchup, CompactMerkleTree.extend_verified,
Ledger.applyCatchupReplies).

A case is an old tree (size, frontier), the replies' transactions (`parts`), the
catch-up target (final_size, final_root) and one consistency proof per reply.
The model appends with merkle_cases.simulate (a stack of (height, hash), which
starts from any frontier) and walks with merkle_verify_cases.check_consistency:
per reply the expected status and root, the call's leaf and node hashes, and
the tree and store bytes the accepted prefix leaves behind.

The real cases share one seeded list of leaves and one CompactMerkleTree over
all of them, from which the proofs and roots are read.  The synthetic case has
an old tree of 2^40 + 5 leaves whose frontier is random: its proofs come from
the recursive definition of RFC 6962 section 2.1.2 over the frontier and the new
leaves alone, which is enough because every subtree of the old tree that a
proof from a size at or beyond old_size names is an entry of the frontier."""
import ctypes
import json
import os

import numpy as np

import merkle_cases as mc
import merkle_verify_cases as vc

GOLDEN = os.path.join(mc.ROOT, "tests", "golden", "merkle_catchup_golden.json")
SEED = 0xF10
SENTINEL = vc.SENTINEL
ZERO = vc.ZERO

# the table of the issue: (old sizes, parts as leaves per reply); every one with final = last end and last end + 37
TABLE = [((0,), ([1], [0, 1], [3, 1, 4])),
         ((1, 5, 8), ([1], [3, 0, 4], [8])),
         ((255, 256, 257), ([256, 2, 255],))]
FINAL_EXTRA = (0, 37)
SYNTH_OLD, SYNTH_PARTS, SYNTH_EXTRA = 2 ** 40 + 5, [2, 3], 3
MUTATIONS = ("txn", "proof_flip", "proof_cut", "proof_extra", "final_below")  # per position j; "wrong_root" once

_LEAVES = mc.leaves_of(SEED, 257 + 513 + 37, max_len=120)
_tree = None


def full_tree():
    """The package's CompactMerkleTree over every seeded leaf (host route), built once."""
    global _tree
    if _tree is None:
        from indy_plenum_amd import merkle
        _tree = merkle.CompactMerkleTree()
        _tree.extend(_LEAVES, on_device=False)
    return _tree


class Case:
    def __init__(self, name, old, old_hashes, parts, final_size, final_root, proofs, real=True):
        self.name, self.old, self.old_hashes, self.parts = name, old, list(old_hashes), [list(p) for p in parts]
        self.final_size, self.final_root, self.real = final_size, final_root, real
        self.proofs = [list(p) for p in proofs]

    def copy(self, name):
        return Case(name, self.old, self.old_hashes, self.parts, self.final_size, self.final_root, self.proofs,
                    self.real)

    @property
    def leaves(self):
        return [leaf for p in self.parts for leaf in p]

    @property
    def ends(self):
        return [int(x) for x in np.cumsum([len(p) for p in self.parts])]

    def __repr__(self):
        return self.name


def _name(old, counts, extra):
    return "old%d-parts%s-final+%d" % (old, "_".join(map(str, counts)), extra)


def real_case(old, counts, extra):
    tree, at, parts = full_tree(), old, []
    for c in counts:
        parts.append(_LEAVES[at:at + c])
        at += c
    final = at + extra
    old_hashes = mc.simulate(0, [], _LEAVES[:old])[2]
    ends = [old + e for e in np.cumsum(counts)]
    proofs = [tree.consistency_proof(int(s), final) if 0 < s < final else [] for s in ends]
    root = tree.merkle_tree_hash(0, final) if final else mc.EMPTY_ROOT
    return Case(_name(old, counts, extra), old, old_hashes, parts, final, root, proofs)


def real_cases():
    return [real_case(old, counts, extra) for olds, shapes in TABLE for old in olds for counts in shapes
            for extra in FINAL_EXTRA]


def synthetic_case():
    """old_size 2^40 + 5 with a random frontier: a position or a shift cut to 32 bits shows up."""
    old, counts, extra = SYNTH_OLD, SYNTH_PARTS, SYNTH_EXTRA
    frontier = mc.frontier(SEED, old)
    new = mc.leaves_of(SEED + 1, sum(counts) + extra, max_len=90)
    blocks, at, it = {}, 0, iter(frontier)
    for b in range(old.bit_length() - 1, -1, -1):
        if (old >> b) & 1:
            blocks[(at, at + (1 << b))] = next(it)
            at += 1 << b

    def mth(a, b):
        if (a, b) in blocks:
            return blocks[(a, b)]
        if b - a == 1:
            assert a >= old
            return mc.leaf_hash(new[a - old])
        assert b > old, "a subtree of the old tree that is no entry of its frontier"
        k = 1 << ((b - a - 1).bit_length() - 1)
        return mc.node_hash(mth(a, a + k), mth(a + k, b))

    def subproof(m, a, b, whole):  # RFC 6962 section 2.1.2, SUBPROOF(m, D[a:b], whole)
        if m == b - a:
            return [] if whole else [mth(a, b)]
        k = 1 << ((b - a - 1).bit_length() - 1)
        if m <= k:
            return subproof(m, a, a + k, whole) + [mth(a + k, b)]
        return subproof(m - k, a + k, b, False) + [mth(a, a + k)]

    final, parts, at = old + sum(counts) + extra, [], 0
    for c in counts:
        parts.append(new[at:at + c])
        at += c
    proofs = [subproof(old + int(e), 0, final, True) for e in np.cumsum(counts)]
    return Case(_name(old, counts, extra), old, frontier, parts, final, mth(0, final), proofs, real=False)


def _flip_byte(b, k=0):
    return b[:k] + bytes([b[k] ^ 0x40]) + b[k + 1:]


def mutate(case, name, j=None):
    """The case after one mutation at reply j (None: a target below zero).
    Where there is nothing to change (no byte to flip in an empty reply, no
    entry in an empty proof) the case stays as it was; proof_extra never fails a
    consistency proof and wrong_root does not fail a reply that ends at size 0:
    the model says what each gives."""
    c = case.copy("%s:%s%s" % (case.name, name, "" if j is None else "@%d" % j))
    if name == "txn":
        idx = [i for i, leaf in enumerate(c.parts[j]) if leaf]
        if idx:
            c.parts[j][idx[0]] = _flip_byte(c.parts[j][idx[0]], len(c.parts[j][idx[0]]) // 2)
    elif name == "proof_flip":
        if c.proofs[j]:
            c.proofs[j][-1] = _flip_byte(c.proofs[j][-1], 17)
    elif name == "proof_cut":
        c.proofs[j] = c.proofs[j][:-1]
    elif name == "proof_extra":
        c.proofs[j] = c.proofs[j] + [vc.JUNK]
    elif name == "wrong_root":
        c.final_root = _flip_byte(c.final_root, 5)
    elif name == "final_below":
        if c.old + c.ends[j] == 0:
            return None
        c.final_size = c.old + c.ends[j] - 1
    else:
        raise ValueError(name)
    return c


def mutated_cases(cases=None):
    """Every mutation at every position of every three-reply real case."""
    out = []
    for case in cases if cases is not None else real_cases():
        if len(case.parts) != 3:
            continue
        out.append(mutate(case, "wrong_root"))
        for name in MUTATIONS:
            out.extend(m for m in (mutate(case, name, j) for j in range(3)) if m is not None)
    return out


_all = None


def all_cases():
    """Real cases, their mutations, the synthetic case and its mutations' like: built once, never changed."""
    global _all
    if _all is None:
        real = real_cases()
        synth = synthetic_case()
        extra = [m for m in (mutate(synth, "wrong_root"), mutate(synth, "txn", 0), mutate(synth, "txn", 1),
                             mutate(synth, "proof_flip", 1), mutate(synth, "final_below", 1)) if m is not None]
        _all = real + mutated_cases(real) + [synth] + extra
    return _all


# ---- the model
class Expected:
    """status (bytes), roots (list of 32 bytes; zeros where RANGE), leaf_hashes / nodes (bytes: the whole call's),
    accepted / accepted_leaves, size / hashes (the tree after the accepted prefix) and leaf_store / node_store
    (the bytes that prefix appends to the stores)."""


def model(case):
    size, hashes = case.old, list(case.old_hashes)
    x = Expected()
    x.status, x.roots, x.leaf_hashes, x.nodes = b"", [], b"", b""
    x.accepted = x.accepted_leaves = 0
    x.size, x.hashes, x.leaf_store, x.node_store = size, list(hashes), b"", b""
    good = True
    for part, proof in zip(case.parts, case.proofs):
        lh, nodes, hashes, root = mc.simulate(size, hashes, part)
        size += len(part)
        x.leaf_hashes += lh
        x.nodes += nodes
        if size > case.final_size:
            st, root = vc.RANGE, ZERO
        else:
            st, _ = vc.check_consistency(size, case.final_size, root, case.final_root, proof)
        x.status += bytes([st])
        x.roots.append(root)
        good = good and st == vc.OK
        if good:
            x.accepted += 1
            x.accepted_leaves += len(part)
            x.size, x.hashes, x.leaf_store, x.node_store = size, list(hashes), x.leaf_hashes, x.nodes
    return x


# ---- hc_merkle_catchup (the kernels' code on the CPU)
_bound = False


def hostcheck():
    global _bound
    lib = mc.hostcheck()
    if not _bound:
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        lib.hc_merkle_catchup.argtypes = [u64, vp, vp, vp, u64, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp]
        lib.hc_merkle_catchup.restype = ctypes.c_int
        lib.hc_merkle_catchup_needs.argtypes = [u64] * 5 + [ctypes.c_int] * 4 + [vp]
        lib.hc_merkle_catchup_needs.restype = None
        _bound = True
    return lib


def _p(a):
    return None if a is None else a.ctypes.data


class HostArgs:
    """A case as the arrays both C forms take: leaves, offsets (from leaf_base), old hashes, reply ends, the
    target root, proofs and their offsets (from proof_base, in entries)."""

    def __init__(self, case, leaf_base=0, proof_base=0):
        blob, off = mc.pack(case.leaves)
        self.blob = np.concatenate([blob, np.zeros(8, np.uint8)])
        self.off = off + np.uint64(leaf_base)
        self.old = vc.pack_hashes(case.old_hashes)
        self.ends = vc.u64(case.ends)
        self.root = np.frombuffer(case.final_root, np.uint8).copy()
        proofs, poff = vc.pack_proofs(case.proofs)
        self.proofs = proofs if len(proofs) else np.zeros(32, np.uint8)
        self.poff = poff + np.uint64(proof_base)
        self.n, self.replies = len(case.leaves), len(case.parts)
        self.nodes = mc.node_span(case.old, self.n)


def guarded(nbytes):
    return np.full(nbytes + 32, SENTINEL, np.uint8)


def read_guarded(arr, nbytes, want=True):
    """The first nbytes of an output; 32 sentinel bytes after it are intact, an output not wanted is untouched."""
    b = arr.tobytes()
    assert b[nbytes:] == bytes([SENTINEL]) * 32
    if not want:
        assert b == bytes([SENTINEL]) * len(b)
        return None
    return b[:nbytes]


def hc_catchup(case, want_leaf=True, want_node=True, want_roots=True):
    """hc_merkle_catchup -> (status, roots | None, leaf_hashes | None, nodes | None)."""
    a = HostArgs(case)
    lh, nh, rr, st = guarded(32 * a.n), guarded(32 * a.nodes), guarded(32 * a.replies), guarded(a.replies)
    rc = hostcheck().hc_merkle_catchup(case.old, _p(a.old) if len(a.old) else None, _p(a.blob), _p(a.off), a.n,
                                       _p(a.ends), a.replies, case.final_size, _p(a.root), _p(a.proofs), _p(a.poff),
                                       _p(lh) if want_leaf else None, _p(nh) if want_node else None,
                                       _p(rr) if want_roots else None, _p(st))
    assert rc == 0
    return (read_guarded(st, a.replies), read_guarded(rr, 32 * a.replies, want_roots),
            read_guarded(lh, 32 * a.n, want_leaf), read_guarded(nh, 32 * a.nodes, want_node))


def check_outputs(case, status, roots, leaf_hashes, nodes):
    """A call's outputs (bytes; None: not asked for) against the model."""
    x = model(case)
    assert list(status) == list(x.status), (case.name, list(status), list(x.status))
    if roots is not None:
        assert roots == b"".join(x.roots), case.name
    if leaf_hashes is not None:
        assert leaf_hashes == x.leaf_hashes, case.name
    if nodes is not None:
        assert nodes == x.nodes, case.name
    return x


# ---- CompactMerkleTree.extend_verified on either route
def tree_at(case):
    """A tree without its store's past, as a copied tree is: the frontier alone."""
    from indy_plenum_amd import merkle
    return merkle.CompactMerkleTree(tree_size=case.old, hashes=case.old_hashes)


def store_bytes(tree):
    s = tree.hashStore
    return b"".join(s.readLeafs(1, s.leafCount + 1)), b"".join(s.readNodes(1, s.nodeCount + 1))


def check_extend_verified(case, on_device, **kw):
    """extend_verified from the case's frontier against the model: result, tree and store bytes."""
    t = tree_at(case)
    res = t.extend_verified(case.parts, case.final_size, case.final_root, case.proofs, on_device=on_device, **kw)
    x = model(case)
    assert list(res.status) == list(x.status), case.name
    assert res.roots.tobytes() == b"".join(x.roots), case.name
    assert (res.accepted, res.accepted_leaves) == (x.accepted, x.accepted_leaves), case.name
    assert t.tree_size == x.size and list(t.hashes) == x.hashes, case.name
    assert t.root_hash == mc.fold(x.hashes), case.name
    assert store_bytes(t) == (x.leaf_store, x.node_store), case.name
    return t, res


def case_named(name):
    return next(c for c in all_cases() if c.name == name)


def check_max_call_split(on_device):
    """Calls split at part boundaries; none is made after one with a failure; a part above max_call raises."""
    import pytest
    base = case_named("old0-parts3_1_4-final+37")
    bad = case_named(base.name + ":txn@1")
    # calls of [3, 1] and [4]: the failure is in the first, the second is not made
    t = tree_at(bad)
    res = t.extend_verified(bad.parts, bad.final_size, bad.final_root, bad.proofs, on_device=on_device, max_call=4)
    assert list(res.status) == [vc.OK, vc.ROOT, vc.UNVERIFIED] and res.accepted == 1 and t.tree_size == 3
    assert res.roots[2].tobytes() == ZERO and store_bytes(t) == (model(bad).leaf_store, model(bad).node_store)
    # the failure in the second call: the first call's replies are applied, every status is computed
    bad2 = case_named(base.name + ":txn@2")
    t, res = check_extend_verified(bad2, on_device, max_call=4)
    assert res.accepted == 2 and t.tree_size == 4 and res.status[2] != vc.UNVERIFIED
    # split or not, an intact case ends the same
    for step in (4, 5, 8):
        check_extend_verified(base, on_device, max_call=step)
    t = tree_at(base)
    with pytest.raises(ValueError):
        t.extend_verified(base.parts, base.final_size, base.final_root, base.proofs, on_device=on_device, max_call=3)
    assert t.tree_size == 0 and t.leafCount == 0


# ---- the reference's recorded outcomes
def load_golden():
    with open(GOLDEN) as f:
        return json.load(f)


def golden_statuses(g, name):
    """The recorded outcomes of one case as the statuses they map to (merkle_verify_cases.STATUS_NAME)."""
    to_status = {v: k for k, v in vc.STATUS_NAME.items()}
    return [to_status[g["names"][i]] for i in g["outcomes"][name]]
