"""The ledger's compact Merkle tree with a batched, device-side extend
(SURVEY.md section 8f row f-5).

Same names and call shapes as the reference's ledger package, written from
RFC 6962 (section 2.1) and the append semantics:

  ledger/ledger.py:145-148              Ledger._addToTree: one append per txn
  ledger/ledger.py:95-106               recoverTreeFromTxnLog: the whole log again
  ledger/compact_merkle_tree.py:155-191 CompactMerkleTree.append / extend / extended
  ledger/tree_hasher.py:20-28           hash_leaf, hash_children

`extend` is defined as n appends: same tree_size, hashes, root and hash-store
contents.  (The reference's own extend leaves its hash store in another state,
which Ledger never uses; that state is not reproduced.)  With the device it is
one edv_merkle_extend call per EDV_MERKLE_MAX_LEAVES leaves (gfx950 kernels
edv_merkle_pass_kernel / edv_merkle_finish_kernel); `append` and the single
proofs, which read the store one hash at a time, stay on the host.

The batched reads (row f-8: ledger/ledger.py:197-206 merkleInfo per reply,
plenum/common/ledger_manager.py:448-452 consistency proofs in catch-up) are
`inclusion_proof_batch`, `consistency_proof_batch` and `merkle_info_batch`:
with a `DeviceHashStore`, whose contents are mirrored on the device, one
edv_merkle_prove_*_dev call for the batch (kernels
edv_merkle_prove_inclusion_kernel / edv_merkle_prove_consistency_kernel),
returning a ProofBatch in the layout the batched verification reads.

Nothing in the reference checks the stored hashes those reads copy
(ledger/ledger.py:70-114 recoverTree trusts a store that has leaves;
compact_merkle_tree.py verify_consistency compares two counts).  `audit_store`
(row f-9) checks every stored node against its stored children, and the leaf
hashes against the leaves if given, one lane per entry over a DeviceHashStore
(kernels edv_merkle_audit_nodes_kernel / edv_merkle_audit_leaves_kernel), and
returns a StoreAudit; `rebuild_nodes` recomputes the node store from the leaf
hashes and `extend_hashed` extends a tree from leaf hashes alone
(edv_merkle_extend_hashed: the extend's passes, the first reading hashes).

`append_batch` (row f-6) is `extend` that also returns what each `append`
returns (ledger/ledger.py:145-155: the audit path, and the root hash read after
it), one edv_merkle_append_batch call per batch (kernel
edv_merkle_append_kernel after the extend's): what `Ledger.commitTxns`
(ledger.py) needs for a 3PC batch.

`MerkleVerifier` (row f-7; ledger/merkle_verifier.py) checks such proofs: the
reference's single calls on the host, and batches of audit paths or
consistency proofs in one edv_merkle_verify_inclusion /
edv_merkle_verify_consistency call, one lane per proof, returning a
ProofVerdicts.  `verify_append_batch` hands an AppendBatch's packed paths and
roots to the device as they are.

`extend_verified` (row f-10; plenum/common/ledger_manager.py:505-609, where a
joining node builds a temporary tree per catch-up reply, walks one consistency
proof from it and then appends the reply's transactions one by one) takes the
transactions of a whole pass of in-order replies with their proofs: one
edv_merkle_catchup call hashes every transaction once (the extend's kernels)
and checks every reply's proof against the tree at its end (kernel
edv_merkle_catchup_kernel, one lane per reply); the longest verified prefix is
applied from the call's own outputs and a CatchupResult says which replies
that was.
"""
import hashlib
from binascii import hexlify
from collections import namedtuple

import numpy as np

from . import edv

# extend(on_device=None) takes the device from this many leaves on: the
# smallest measured size at which the host-buffer call beats the host loop
# (profiles/r07/merkle_bench.json, "crossover": 157 us against 234 us at 256
# leaves of 256 bytes; at 64 the host loop wins, 61 us against 131 us)
MIN_DEVICE_LEAVES = 256

# append_batch(on_device=None) takes the device from this many leaves on: the
# smallest measured size at which the host-buffer call with roots and paths
# beats the host loop on both trees (profiles/r08/merkle_append_bench.json,
# "crossover": 234 us against 610 us at 256 leaves of 256 bytes onto an empty
# tree, 354 us against 844 us onto 2^20 + 12,345 leaves; at 100, the next size
# measured, the two are level within the rows' spread, 220 us against 218 us
# and 334 us against 326 us; nothing between 100 and 256 was measured)
MIN_DEVICE_APPEND_LEAVES = 256


# MerkleVerifier.*_batch(on_device=None) takes the device from this many proofs
# on: the smallest size measured, at which verify_append_batch on the device
# already beats the host walk on both trees (profiles/r09/merkle_verify_bench.json,
# "crossover": 153 us against 185 us for the 64 appends onto an empty tree,
# paths of 3 entries, the narrowest margin of the table, and 169 us against
# 332 us onto 2^20 + 12,345 leaves; nothing below 64 was measured)
MIN_DEVICE_VERIFY_PROOFS = 64


# *_proof_batch / merkle_info_batch(on_device=None) over a DeviceHashStore take
# the device from this many proofs on: the smallest size measured, at which the
# route through the store's mirror, outputs copied back, already beats the host
# loop of single calls on both trees (profiles/r10/merkle_prove_bench.json,
# "crossover": 113 us against 187 us for 16 merkleInfo proofs on 10,000
# leaves, 114 us against 205 us on 2^20 + 12,345; nothing below 16 was measured)
MIN_DEVICE_PROVE_PROOFS = 16


# audit_store(on_device=None) over a DeviceHashStore takes the device from this
# many entries (nodes, and leaves if given) on: the smallest measured node count
# at which the route through the store's mirror beats the hashlib loop on both
# stores, the node store alone and the node and leaf stores with 256-byte leaves
# (profiles/r11/merkle_audit_bench.json, "crossover": at 256 nodes 49.3 us
# against 239.2 us, and 149.1 us against 364.3 us with the 258 leaves; at 64
# nodes the node store alone wins, 49.3 us against 61.1 us, and with the 66
# leaves the loop does, 93.7 us against 134.5 us; at 16 the loop wins both)
MIN_DEVICE_AUDIT_ENTRIES = 256


# extend_verified / Ledger.applyCatchupReplies(on_device=None) take the device
# from this many leaves in all on: the smallest measured total at which the one
# device call beats, on both trees and beyond the rows' spread, both the loop it
# replaces and the same pass on the host (profiles/r12/merkle_catchup_bench.json,
# "crossover": at 1,024 transactions of 256 bytes in replies of 100, 679 us
# (600-1,121) against 1,309 us (1,133-1,814) on the host and 8.9 ms for the
# loop onto an empty tree, 740 us against 1,200 us and 10.4 ms onto 2^20 +
# 12,345 leaves; at 256 the host pass wins on the larger tree, 292 us against
# 471 us, and is level on the empty one, 336 us against 351 us; against the
# loop alone the device call wins at every size measured, 64 included;
# nothing between 256 and 1,024 was measured)
MIN_DEVICE_CATCHUP_LEAVES = 1024


class ConsistencyVerificationFailed(Exception):
    pass


STH = namedtuple("STH", ["tree_size", "sha256_root_hash"])


class VerifyError(Exception):
    """A proof did not verify."""


class ProofError(VerifyError):
    """The proof is invalid: too short, too long, or it arrives at another root."""


class ConsistencyError(VerifyError):
    """The proof shows that the two trees are inconsistent."""


def _popcount(x):
    return bin(x).count("1")


def popcount_prefix(x):
    """Sum of popcount(t) over 0 <= t < x: bit b is set in (x >> (b + 1)) 2^b
    numbers below x, plus the part of x's last period past its first half."""
    total = 0
    for b in range(x.bit_length()):
        half = 1 << b
        total += ((x >> (b + 1)) << b) + max(0, (x & (2 * half - 1)) - half)
    return total


class AppendBatch:
    """What the n `append` calls of one append_batch returned: `roots`, an
    (n, 32) uint8 array (the root hash after leaf i), and the audit paths,
    packed in `paths`, an (entries, 32) uint8 array: leaf i's path is the
    popcount(old_size + i) rows from popcount_prefix(old_size + i) -
    popcount_prefix(old_size) on, smallest subtree first.  Iterating yields
    (root, audit_path) per leaf, as bytes and a list of bytes."""

    def __init__(self, old_size, roots, paths):
        self.old_size = old_size
        self.roots = roots
        self.paths = paths
        self._base = popcount_prefix(old_size)

    def __len__(self):
        return len(self.roots)

    def root(self, i):
        return self.roots[i].tobytes()

    def path(self, i):
        if not 0 <= i < len(self.roots):
            raise IndexError(i)
        lo = popcount_prefix(self.old_size + i) - self._base
        blob = self.paths[lo:lo + _popcount(self.old_size + i)].tobytes()
        return [blob[k:k + 32] for k in range(0, len(blob), 32)]

    def __iter__(self):
        roots, blob, lo = self.roots.tobytes(), self.paths.tobytes(), 0
        for i in range(len(self.roots)):
            hi = lo + 32 * _popcount(self.old_size + i)
            yield roots[32 * i:32 * i + 32], [blob[k:k + 32] for k in range(lo, hi, 32)]
            lo = hi


def node_position(height, block):
    """1-based position in the node store of the node of `height` >= 1 over
    leaves [block 2^height, (block + 1) 2^height): appending leaf s (1-based)
    writes heights 1 .. ctz(s), after the (s - 1) - popcount(s - 1) nodes of
    the tree before it."""
    s = (block + 1) << height
    return (s - 1) - _popcount(s - 1) + height


class TreeHasher:
    def __init__(self, hashfunc=hashlib.sha256):
        self.hashfunc = hashfunc

    def __repr__(self):
        return "%s(%r)" % (self.__class__.__name__, self.hashfunc)

    def hash_empty(self):
        return self.hashfunc().digest()

    def hash_leaf(self, data):
        return self.hashfunc(b"\x00" + data).digest()

    def hash_children(self, left, right):
        return self.hashfunc(b"\x01" + left + right).digest()

    def hash_fold(self, hashes):
        """Root of a compact tree's hashes (largest subtree first)."""
        if not hashes:
            return self.hash_empty()
        acc = hashes[-1]
        for h in reversed(hashes[:-1]):
            acc = self.hash_children(h, acc)
        return acc

    def hash_full_tree(self, leaves):
        """MTH of the whole list (RFC 6962 section 2.1)."""
        n = len(leaves)
        if n == 0:
            return self.hash_empty()
        if n == 1:
            return self.hash_leaf(leaves[0])
        k = 1 << ((n - 1).bit_length() - 1)
        return self.hash_children(self.hash_full_tree(leaves[:k]), self.hash_full_tree(leaves[k:]))


class MemoryHashStore:
    """Leaf and node hashes by 1-based position, 32 bytes each, kept as the
    hash alone (as the reference's file store keeps them)."""
    HASH = 32

    def __init__(self):
        self.reset()

    def writeLeaf(self, leafHash):
        self._check(leafHash)
        self._leafs += leafHash

    def writeNode(self, node):
        """node: (start, height, hash), as CompactMerkleTree hands it over."""
        self._check(node[2])
        self._nodes += node[2]

    def writeLeafs(self, hashes):
        """Whole output buffer of a device call: k x 32 bytes, in order."""
        self._leafs += self._bulk(hashes)

    def writeNodes(self, hashes):
        self._nodes += self._bulk(hashes)

    def readLeaf(self, pos):
        return self._read(self._leafs, pos)

    def readNode(self, pos):
        return self._read(self._nodes, pos)

    def readLeafs(self, startpos, endpos):
        return (self._read(self._leafs, p) for p in range(startpos, endpos))

    def readNodes(self, startpos, endpos):
        return (self._read(self._nodes, p) for p in range(startpos, endpos))

    @property
    def leafCount(self):
        return len(self._leafs) // self.HASH

    @property
    def nodeCount(self):
        return len(self._nodes) // self.HASH

    def reset(self):
        self._leafs = bytearray()
        self._nodes = bytearray()
        return True

    def replaceNodes(self, hashes):
        """The node store wholesale: k x 32 bytes, in position order (what
        CompactMerkleTree.rebuild_nodes recomputed from the leaf hashes)."""
        self._nodes = bytearray(self._bulk(hashes))

    def _check(self, h):
        if len(h) != self.HASH:
            raise ValueError("a hash is %d bytes" % self.HASH)

    def _bulk(self, hashes):
        b = hashes.tobytes() if isinstance(hashes, np.ndarray) else bytes(hashes)
        if len(b) % self.HASH:
            raise ValueError("not a whole number of hashes")
        return b

    def _read(self, arr, pos):
        if pos < 1 or pos * self.HASH > len(arr):
            raise IndexError("no hash at position %r" % (pos,))
        return bytes(arr[(pos - 1) * self.HASH:pos * self.HASH])


class DeviceHashStore(MemoryHashStore):
    """A MemoryHashStore whose contents are mirrored in device memory, for the
    batched proofs (row f-8).  The host bytes stay authoritative: every write
    and read is MemoryHashStore's.  device_arrays() brings the mirror up to
    date by uploading the tail not yet sent (the stores only grow) and returns
    (leaf pointer, node pointer, leaf count, node count).  A mirror that has
    become too small is replaced by one of twice the size, at least, and the
    whole store is uploaded again from the host copy.  reset() frees the
    device memory.  Nothing touches the device before the first
    device_arrays(), so without a GPU this is a plain store."""
    MIN_CAPACITY = 1 << 16  # bytes

    def __init__(self, device=0):
        self.device = device
        self._bufs = [None, None]
        self._work = None
        super().__init__()

    def reset(self):
        for b in self._bufs + [self._work]:
            if b is not None:
                b.free()
        self._bufs = [None, None]   # edv.DeviceBuffer of the leaf store, of the node store
        self._sent = [0, 0]         # bytes of each the mirror holds
        self._work = None           # the batch calls' inputs and outputs (work_area)
        self.bytes_uploaded = 0     # in all, since the last reset
        return super().reset()

    @property
    def device_bytes(self):
        """Device memory held: both mirrors and the work area."""
        return sum(b.nbytes for b in self._bufs + [self._work] if b is not None)

    def device_arrays(self):
        for k, host in enumerate((self._leafs, self._nodes)):
            need, buf = len(host), self._bufs[k]
            if buf is None or need > buf.nbytes:
                cap = max(self.MIN_CAPACITY, need, 2 * (buf.nbytes if buf is not None else 0))
                if buf is not None:
                    buf.free()
                buf = self._bufs[k] = edv.DeviceBuffer(cap, self.device)
                self._sent[k] = 0
            sent = self._sent[k]
            if need > sent:
                tail = np.frombuffer(host, dtype=np.uint8, count=need - sent, offset=sent)
                edv._check(edv.lib().edv_h2d(self.device, buf.ptr + sent, tail.ctypes.data, need - sent))
                del tail  # the bytearray may grow again
                self.bytes_uploaded += need - sent
                self._sent[k] = need
        return self._bufs[0].ptr, self._bufs[1].ptr, self.leafCount, self.nodeCount

    def replaceNodes(self, hashes):
        """MemoryHashStore's; the node mirror is uploaded again, whole, by the next device_arrays()."""
        super().replaceNodes(hashes)
        self._sent[1] = 0

    def mark_stale(self):
        """Both mirrors are uploaded again, whole, by the next device_arrays():
        for a caller that changed the host bytes other than by appending."""
        self._sent = [0, 0]

    def work_area(self, nbytes):
        """A device buffer of at least nbytes that the batch calls reuse."""
        if self._work is None or self._work.nbytes < nbytes:
            cap = max(self.MIN_CAPACITY, nbytes, 2 * (self._work.nbytes if self._work is not None else 0))
            if self._work is not None:
                self._work.free()
            self._work = edv.DeviceBuffer(cap, self.device)
        return self._work


class ProofBatch:
    """What a batched proof call returned (row f-8), in the layout the batched
    verification takes as it is: `proofs`, an (entries, 32) uint8 array, proof i
    being rows off[i] .. off[i + 1], lowest level first; `status`, one
    edv.PROOF_* per proof (all PROOF_OK: a pair out of range raises instead).
    kind "inclusion": `index` and `size` (leaf index and tree size per proof),
    `roots` (MTH(D[0:size]), (n, 32), or None if not asked for) and
    `leaf_hashes` (the leaves' stored hashes).  kind "consistency": `index` is
    the older size, `size` the newer one, `old_roots` / `new_roots` their tree
    heads.  proof(i) and iteration give a proof as a list of bytes."""

    def __init__(self, kind, index, size, proofs, off, status, roots=None, leaf_hashes=None, old_roots=None,
                 new_roots=None):
        self.kind = kind
        self.index, self.size = index, size
        self.proofs, self.off, self.status = proofs, off, status
        self.roots, self.leaf_hashes = roots, leaf_hashes
        self.old_roots, self.new_roots = old_roots, new_roots

    def __len__(self):
        return len(self.status)

    def proof(self, i):
        if not 0 <= i < len(self.status):
            raise IndexError(i)
        blob = self.proofs[int(self.off[i]):int(self.off[i + 1])].tobytes()
        return [blob[k:k + 32] for k in range(0, len(blob), 32)]

    def __iter__(self):
        blob = self.proofs.tobytes()
        for i in range(len(self.status)):
            yield [blob[k:k + 32] for k in range(32 * int(self.off[i]), 32 * int(self.off[i + 1]), 32)]


def _hash_rows(hashes):
    return np.frombuffer(b"".join(hashes), dtype=np.uint8).reshape(-1, 32)


class StoreAudit:
    """What CompactMerkleTree.audit_store found (row f-9).  `nodes_checked`
    and `leaves_checked` count the entries compared; `bad_nodes` and
    `bad_leaves` are the sorted 1-based positions, as readNode and readLeaf
    count, of the nodes that are not the hash of their stored children and of
    the leaf hashes that are not the hash of their leaf; `counts_ok`: the node
    store has exactly the nodes its leaf count implies (and, with leaves given,
    there is one leaf per stored hash); `frontier_ok`: the tree's own size and
    hashes are what the store holds for them."""

    def __init__(self, nodes_checked=0, bad_nodes=(), leaves_checked=0, bad_leaves=(), counts_ok=True,
                 frontier_ok=True):
        self.nodes_checked = nodes_checked
        self.bad_nodes = sorted(bad_nodes)
        self.leaves_checked = leaves_checked
        self.bad_leaves = sorted(bad_leaves)
        self.counts_ok = counts_ok
        self.frontier_ok = frontier_ok

    @property
    def ok(self):
        return self.counts_ok and self.frontier_ok and not self.bad_nodes and not self.bad_leaves

    def __repr__(self):
        return "StoreAudit(nodes_checked=%d, bad_nodes=%r, leaves_checked=%d, bad_leaves=%r, counts_ok=%r, " \
            "frontier_ok=%r)" % (self.nodes_checked, self.bad_nodes, self.leaves_checked, self.bad_leaves,
                                 self.counts_ok, self.frontier_ok)


class CatchupResult:
    """What extend_verified / Ledger.applyCatchupReplies did with the replies
    of a catch-up: `status`, a uint8 array of edv.PROOF_* (one per reply; 0,
    PROOF_UNVERIFIED, for a reply of a call that was not made any more);
    `roots`, an (r, 32) uint8 array, the tree head at each reply's end (zeros
    where the status is PROOF_RANGE or PROOF_UNVERIFIED); `accepted`, the
    number of leading PROOF_OK replies, which are the ones that were applied;
    `accepted_leaves`, the leaves in them.

    A status after the first failure is computed over the rejected
    transactions (the tree at that reply's end contains them) and is not a
    judgement of that reply: send the rest again once the failing reply is
    replaced."""

    def __init__(self, status, roots, accepted, accepted_leaves):
        self.status = np.asarray(status, dtype=np.uint8)
        self.roots = roots
        self.accepted = accepted
        self.accepted_leaves = accepted_leaves

    @property
    def ok(self):
        """Was every reply applied?"""
        return self.accepted == len(self.status)

    def __len__(self):
        return len(self.status)

    def __repr__(self):
        return "CatchupResult(accepted=%d of %d replies, accepted_leaves=%d, status=%r)" % (
            self.accepted, len(self.status), self.accepted_leaves, self.status.tolist())


def _leading_ok(status):
    bad = np.flatnonzero(np.asarray(status) != edv.PROOF_OK)
    return int(bad[0]) if len(bad) else len(status)


def _call_frontier(old_size, old_hashes, size, leaf_h, node_h):
    """hashes(size), largest first, out of one call's outputs, old_size <= size
    <= old_size + len(leaf_h): merkle_entry's rule (edv_merkle.h).  The entry
    for set bit b is block k = (size >> b) - 1 at height b; if it ends at or
    before old_size it is the old tree's entry for the same bit, else the call
    made it: a leaf hash (b = 0) or the node at its node-store position."""
    base, out = old_size - _popcount(old_size), []
    for b in reversed(range(size.bit_length())):
        if not (size >> b) & 1:
            continue
        k = (size >> b) - 1
        if ((k + 1) << b) <= old_size:
            out.append(bytes(old_hashes[_popcount(old_size >> (b + 1))]))
        elif b == 0:
            out.append(leaf_h[k - old_size].tobytes())
        else:
            out.append(node_h[node_position(b, k) - 1 - base].tobytes())
    return out


def _carry_chain(hasher, size, stack, leaf_hashes):
    """The appends' carry chain over leaf hashes: (size, stack, node hashes in store order)."""
    nodes = []
    for h in leaf_hashes:
        size += 1
        stack.append(h)
        s = size
        while not s & 1:
            right = stack.pop()
            left = stack.pop()
            stack.append(hasher.hash_children(left, right))
            nodes.append(stack[-1])
            s >>= 1
    return size, stack, nodes


class CompactMerkleTree:
    """(tree_size, hashes): the roots of the full subtrees of the binary
    decomposition of tree_size, largest first; leaf and node hashes go to
    hashStore as they are made."""

    def __init__(self, hasher=None, tree_size=0, hashes=(), hashStore=None):
        self.__hasher = hasher or TreeHasher()
        self.__hashStore = hashStore if hashStore is not None else MemoryHashStore()
        self._update(tree_size, hashes)

    @property
    def hashStore(self):
        return self.__hashStore

    def _update(self, tree_size, hashes):
        hashes = tuple(bytes(h) for h in hashes)
        if tree_size < 0 or len(hashes) != _popcount(tree_size):
            raise ValueError("number of hashes != bits set in tree_size: %s vs %s"
                             % (len(hashes), _popcount(max(tree_size, 0))))
        self.__tree_size = tree_size
        self.__hashes = hashes
        self.__root_hash = None

    def __copy__(self):
        return self.__class__(self.__hasher, self.__tree_size, self.__hashes)

    def __repr__(self):
        return "%s(%r, %r, %r)" % (self.__class__.__name__, self.__hasher, self.__tree_size, self.__hashes)

    def __len__(self):
        return self.__tree_size

    @property
    def tree_size(self):
        return self.__tree_size

    @property
    def hashes(self):
        return self.__hashes

    @property
    def root_hash(self):
        if self.__root_hash is None:
            self.__root_hash = self.__hasher.hash_fold(self.__hashes)
        return self.__root_hash

    @property
    def root_hash_hex(self):
        return hexlify(self.root_hash)

    # ---- growing
    def _append_hashes(self, leaves):
        """The appends' carry chain on the host: leaf hashes, nodes as
        (tree size after the leaf, height, hash), new hashes."""
        size, stack = self.__tree_size, list(self.__hashes)
        leaf_hashes, nodes = [], []
        for leaf in leaves:
            h = self.__hasher.hash_leaf(leaf)
            leaf_hashes.append(h)
            size += 1
            stack.append(h)
            height, s = 1, size
            while not s & 1:
                right = stack.pop()
                left = stack.pop()
                stack.append(self.__hasher.hash_children(left, right))
                nodes.append((size, height, stack[-1]))
                height += 1
                s >>= 1
        return size, stack, leaf_hashes, nodes

    def append(self, new_leaf):
        """Append one leaf; returns its audit path (one leaf is at most 64
        compressions: always on the host)."""
        audit_path = list(reversed(self.__hashes))
        size, hashes, leaf_hashes, nodes = self._append_hashes([new_leaf])
        self.__hashStore.writeLeaf(leaf_hashes[0])
        for node in nodes:
            self.__hashStore.writeNode(node)
        self._update(size, hashes)
        return audit_path

    def extend(self, new_leaves, on_device=None, max_call=None, device=0):
        """Append every leaf of new_leaves: exactly what len(new_leaves) calls
        of append leave behind, hash store included.  on_device True / False
        forces the path; None takes the device from MIN_DEVICE_LEAVES leaves
        on.  Batches above max_call (at most, and by default,
        edv.MERKLE_MAX_LEAVES) leaves go in successive calls."""
        new_leaves = list(new_leaves)
        if on_device is None:
            on_device = len(new_leaves) >= MIN_DEVICE_LEAVES
        step = edv.MERKLE_MAX_LEAVES if max_call is None else int(max_call)
        if step < 1 or step > edv.MERKLE_MAX_LEAVES:
            raise ValueError("max_call must be in [1, %d]" % edv.MERKLE_MAX_LEAVES)
        if self.__tree_size + len(new_leaves) > edv.MERKLE_MAX_SIZE:
            raise ValueError("tree size above 2^62")
        for lo in range(0, len(new_leaves), step):
            part = new_leaves[lo:lo + step]
            if on_device:
                self._extend_device(part, device)
            else:
                size, hashes, leaf_hashes, nodes = self._append_hashes(part)
                self.__hashStore.writeLeafs(b"".join(leaf_hashes))
                self.__hashStore.writeNodes(b"".join(h for _, _, h in nodes))
                self._update(size, hashes)

    def _device_call(self, part, device, per_leaf):
        """One device call over `part`, tree and hash store updated from its
        outputs; with per_leaf the appends' (roots, packed paths), else None."""
        off = np.zeros(len(part) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in part], dtype=np.uint64)
        blob = np.frombuffer(b"".join(part) + b"\0" * 8, dtype=np.uint8)
        call = edv.merkle_append_batch if per_leaf else edv.merkle_extend
        leaf_h, node_h, new_h, root, *rest = call(self.__tree_size, b"".join(self.__hashes), blob, off, device=device)
        self.__hashStore.writeLeafs(leaf_h)
        self.__hashStore.writeNodes(node_h)
        self._update(self.__tree_size + len(part), [bytes(r) for r in new_h])
        self.__root_hash = root
        return tuple(rest) if per_leaf else None

    def _extend_device(self, part, device):
        self._device_call(part, device, False)

    def append_batch(self, new_leaves, on_device=None, max_call=None, device=0):
        """Append every leaf of new_leaves and return what each `append`
        returns, as an AppendBatch: the root hash after every leaf and every
        leaf's audit path.  Tree and hash store end exactly as after
        len(new_leaves) calls of append.  on_device True / False forces the
        path; None takes the device (one edv_merkle_append_batch call per
        max_call leaves) from MIN_DEVICE_APPEND_LEAVES leaves on."""
        new_leaves = list(new_leaves)
        if on_device is None:
            on_device = len(new_leaves) >= MIN_DEVICE_APPEND_LEAVES
        step = edv.MERKLE_MAX_LEAVES if max_call is None else int(max_call)
        if step < 1 or step > edv.MERKLE_MAX_LEAVES:
            raise ValueError("max_call must be in [1, %d]" % edv.MERKLE_MAX_LEAVES)
        if self.__tree_size + len(new_leaves) > edv.MERKLE_MAX_SIZE:
            raise ValueError("tree size above 2^62")
        old_size = self.__tree_size
        roots, paths = [], []
        for lo in range(0, len(new_leaves), step):
            part = new_leaves[lo:lo + step]
            r, p = self._append_batch_device(part, device) if on_device else self._append_batch_host(part)
            roots.append(r)
            paths.append(p)
        if not roots:
            roots, paths = [np.zeros((0, 32), np.uint8)], [np.zeros((0, 32), np.uint8)]
        return AppendBatch(old_size, roots[0] if len(roots) == 1 else np.concatenate(roots),
                           paths[0] if len(paths) == 1 else np.concatenate(paths))

    def _append_batch_host(self, part):
        """The appends one by one in hashlib: stack before, carry chain, fold after."""
        hasher, store = self.__hasher, self.__hashStore
        size, stack = self.__tree_size, list(self.__hashes)
        roots, paths = [], []
        for leaf in part:
            paths.extend(reversed(stack))
            h = hasher.hash_leaf(leaf)
            store.writeLeaf(h)
            size += 1
            stack.append(h)
            height, s = 1, size
            while not s & 1:
                right = stack.pop()
                left = stack.pop()
                stack.append(hasher.hash_children(left, right))
                store.writeNode((size, height, stack[-1]))
                height += 1
                s >>= 1
            roots.append(hasher.hash_fold(stack))
        self._update(size, stack)
        self.__root_hash = roots[-1] if roots else None
        return (np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32),
                np.frombuffer(b"".join(paths), np.uint8).reshape(-1, 32))

    def _append_batch_device(self, part, device):
        return self._device_call(part, device, True)

    def extended(self, new_leaves, on_device=None):
        """A new tree equal to this one extended with new_leaves (its own, empty, hash store)."""
        new_tree = self.__copy__()
        new_tree.extend(new_leaves, on_device=on_device)
        return new_tree

    # ---- catch-up (row f-10)
    def extend_verified(self, parts, final_size, final_root, proofs, on_device=None, max_call=None, device=0):
        """Apply the longest prefix of `parts` (lists of leaves: the
        transactions of in-order catch-up replies) whose consistency proofs all
        verify: proofs[k] must lead from the tree at part k's end to the tree
        of final_size leaves and root final_root.  Tree and hash store end
        byte-identical to `extend` over the accepted parts' leaves; nothing of a
        rejected part is written.  Returns a CatchupResult.

        On the device one edv_merkle_catchup call hashes every leaf once and
        checks the parts' proofs side by side (kernel edv_merkle_catchup_kernel
        after the extend's); on the host the same work goes part by part.
        on_device True / False forces the route; None takes the device from
        MIN_DEVICE_CATCHUP_LEAVES leaves in all on.  Above max_call leaves (at
        most, and by default, edv.MERKLE_MAX_LEAVES) the calls split at part
        boundaries, and none is made after one with a failure; a single part
        above max_call raises ValueError before anything is applied."""
        parts = [list(p) for p in parts]
        proofs = [[_hash32(h, "a proof entry") for h in p] for p in proofs]
        if len(proofs) != len(parts):
            raise ValueError("one proof per part")
        final_size, final_root = int(final_size), _hash32(final_root, "final_root")
        if not _in_u64(final_size):
            raise ValueError("final_size out of range")
        total = sum(len(p) for p in parts)
        if on_device is None:
            on_device = total >= MIN_DEVICE_CATCHUP_LEAVES
        if on_device and self.__hasher.hashfunc is not hashlib.sha256:
            raise ValueError("the device hashes SHA-256 trees only")
        step = edv.MERKLE_MAX_LEAVES if max_call is None else int(max_call)
        if step < 1 or step > edv.MERKLE_MAX_LEAVES:
            raise ValueError("max_call must be in [1, %d]" % edv.MERKLE_MAX_LEAVES)
        if any(len(p) > step for p in parts):
            raise ValueError("a part is larger than max_call")
        if self.__tree_size + total > edv.MERKLE_MAX_SIZE:
            raise ValueError("tree size above 2^62")
        r = len(parts)
        status, roots = np.zeros(r, dtype=np.uint8), np.zeros((r, 32), dtype=np.uint8)
        accepted = accepted_leaves = lo = 0
        while lo < r:
            hi, count = lo + 1, len(parts[lo])
            while hi < r and count + len(parts[hi]) <= step:
                count += len(parts[hi])
                hi += 1
            call = self._catchup_device if on_device else self._catchup_host
            st, rt, ok, ok_leaves = call(parts[lo:hi], proofs[lo:hi], final_size, final_root, device)
            status[lo:hi], roots[lo:hi] = st, rt
            accepted += ok
            accepted_leaves += ok_leaves
            if ok < hi - lo:
                break
            lo = hi
        return CatchupResult(status, roots, accepted, accepted_leaves)

    def _catchup_host(self, parts, proofs, final_size, final_root, device):
        """One call's parts on the host: (statuses, roots, accepted parts,
        accepted leaves), the accepted prefix applied.  Parts after a failure
        are hashed on, as the device call does, and not written."""
        hasher, store = self.__hasher, self.__hashStore
        size, stack = self.__tree_size, list(self.__hashes)
        status, roots, good, ok, ok_leaves = [], [], True, 0, 0
        for part, proof in zip(parts, proofs):
            leaf_hashes = [hasher.hash_leaf(leaf) for leaf in part]
            size, stack, nodes = _carry_chain(hasher, size, stack, leaf_hashes)
            root = hasher.hash_fold(stack)
            if size > final_size:
                st, root = edv.PROOF_RANGE, _ZERO32
            else:
                st, _ = _walk_consistency(hasher, size, final_size, root, final_root, proof)
            status.append(st)
            roots.append(root)
            good = good and st == edv.PROOF_OK
            if good:
                store.writeLeafs(b"".join(leaf_hashes))
                store.writeNodes(b"".join(nodes))
                self._update(size, stack)
                self.__root_hash = root
                ok += 1
                ok_leaves += len(part)
        return status, np.frombuffer(b"".join(roots), np.uint8).reshape(-1, 32), ok, ok_leaves

    def _catchup_device(self, parts, proofs, final_size, final_root, device):
        """One edv_merkle_catchup call over `parts`; as _catchup_host.  The
        accepted size's hashes are read out of the call's own outputs
        (_call_frontier): a copied tree's store is empty."""
        leaves = [leaf for part in parts for leaf in part]
        off = np.zeros(len(leaves) + 1, dtype=np.uint64)
        off[1:] = np.cumsum([len(x) for x in leaves], dtype=np.uint64)
        ends = np.cumsum([len(p) for p in parts], dtype=np.uint64)
        blob = np.frombuffer(b"".join(leaves) + b"\0" * 8, dtype=np.uint8)
        packed, poff = _pack_proofs(proofs)
        old_size, old_hashes = self.__tree_size, self.__hashes
        leaf_h, node_h, roots, status = edv.merkle_catchup(old_size, b"".join(old_hashes), blob, off, ends, final_size,
                                                           final_root, packed, poff, device=device)
        ok = _leading_ok(status)
        ok_leaves = int(ends[ok - 1]) if ok else 0
        if ok:
            size = old_size + ok_leaves
            nodes = edv.merkle_node_span(old_size, ok_leaves)
            self.__hashStore.writeLeafs(leaf_h[:ok_leaves])
            self.__hashStore.writeNodes(node_h[:nodes])
            self._update(size, _call_frontier(old_size, old_hashes, size, leaf_h, node_h))
            self.__root_hash = roots[ok - 1].tobytes()
        return status, roots, ok, ok_leaves

    # ---- reading (host, from the hash store)
    def merkle_tree_hash(self, start, end):
        """MTH(D[start:end]) (RFC 6962 section 2.1) from the stored hashes."""
        if not end > start or start < 0:
            raise ValueError("end must be greater than start")
        n = end - start
        if n == 1:
            return self.__hashStore.readLeaf(end)
        if n & (n - 1) == 0 and start % n == 0:  # a complete aligned subtree: stored
            height = n.bit_length() - 1
            return self.__hashStore.readNode(node_position(height, start >> height))
        k = 1 << ((n - 1).bit_length() - 1)
        return self.__hasher.hash_children(self.merkle_tree_hash(start, start + k),
                                           self.merkle_tree_hash(start + k, end))

    def inclusion_proof(self, start, end):
        """PATH(start, D[0:end]): the audit path of leaf index `start` in the tree of the first `end` leaves."""
        return [self.merkle_tree_hash(a, b) for a, b in self._path(start, 0, end)]

    def consistency_proof(self, first, second):
        """PROOF(first, D[0:second])."""
        return [self.merkle_tree_hash(a, b) for a, b in self._subproof(first, 0, second, True)]

    def _path(self, m, lo, hi):
        n = hi - lo
        if n == 1:
            return []
        k = 1 << ((n - 1).bit_length() - 1)
        if m < k:
            return self._path(m, lo, lo + k) + [(lo + k, hi)]
        return self._path(m - k, lo + k, hi) + [(lo, lo + k)]

    def _subproof(self, m, lo, hi, whole):
        n = hi - lo
        if m == n:
            return [] if whole else [(lo, hi)]
        k = 1 << ((n - 1).bit_length() - 1)
        if m <= k:
            return self._subproof(m, lo, lo + k, whole) + [(lo + k, hi)]
        return self._subproof(m - k, lo + k, hi, False) + [(lo, lo + k)]

    # ---- reading, a batch at a time (row f-8)
    def _store_bytes(self):
        store = self.__hashStore
        if isinstance(store, MemoryHashStore):
            return store._leafs, store._nodes
        return (b"".join(store.readLeafs(1, store.leafCount + 1)), b"".join(store.readNodes(1, store.nodeCount + 1)))

    def _prove_route(self, n, on_device):
        """"host" (the single calls in a loop), "store" (the device forms over
        a DeviceHashStore's mirror) or "copy" (the host-buffer form, which
        copies the store per call)."""
        mirrored = isinstance(self.__hashStore, DeviceHashStore)
        if on_device is None:
            on_device = mirrored and n >= MIN_DEVICE_PROVE_PROOFS
        if not on_device:
            return "host"
        if self.__hasher.hashfunc is not hashlib.sha256:
            raise ValueError("the device proves SHA-256 trees only")
        return "store" if mirrored else "copy"

    def _checked_pairs(self, pairs, consistency):
        """The pairs as two uint64 arrays, after the checks every route makes
        first, so that all of them raise alike: ValueError for a pair that is
        no proof's (leaf index not below the tree size; older size 0 or above
        the newer one), IndexError for a tree larger than the store."""
        if not isinstance(pairs, (list, tuple, np.ndarray)):
            pairs = list(pairs)
        if len(pairs) > edv.MERKLE_MAX_LEAVES:
            raise ValueError("more than %d proofs in one call" % edv.MERKLE_MAX_LEAVES)
        try:   # one conversion for the whole batch: integers below 2^63, which is every real tree's
            both = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
            if (both < 0).any():
                raise ValueError("sizes and indices must be in [0, 2^64)")
            a, b = both[:, 0].astype(np.uint64), both[:, 1].astype(np.uint64)
        except OverflowError:
            pairs = [(int(x), int(y)) for x, y in pairs]
            if any(not (_in_u64(x) and _in_u64(y)) for x, y in pairs):
                raise ValueError("sizes and indices must be in [0, 2^64)")
            a = np.array([p[0] for p in pairs], dtype=np.uint64)
            b = np.array([p[1] for p in pairs], dtype=np.uint64)
        bad = ((a == 0) | (a > b)) if consistency else (a >= b)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            raise ValueError("pair %d: %s" % (i, "the older size must be in [1, newer size]" if consistency
                                              else "the leaf index must be below the tree size"))
        big = b > np.uint64(self.leafCount)
        if big.any():
            raise IndexError("pair %d: the store has no tree of %d leaves" % (int(np.flatnonzero(big)[0]),
                                                                              int(b[np.flatnonzero(big)[0]])))
        return a, b

    def _prove_device(self, consistency, a, b, want1, want2, device):
        """-> (proofs, off, status, out1, out2) through the mirror of a DeviceHashStore."""
        store, n = self.__hashStore, len(a)
        d_leafs, d_nodes, leaves, _ = store.device_arrays()
        off = (edv.merkle_consistency_offsets if consistency else edv.merkle_inclusion_offsets)(a, b, leaves)
        entries = int(off[-1])
        # words | proofs | out1 | out2 | status: every hash buffer on 32 bytes
        wbytes = (8 * (3 * n + 1) + 31) // 32 * 32
        o_proofs, o_1 = wbytes, wbytes + 32 * entries
        o_2 = o_1 + (32 * n if want1 else 0)
        o_st = o_2 + (32 * n if want2 else 0)
        work = store.work_area(o_st + n + 32)
        work.upload(np.concatenate([a, b, off]))
        p = work.ptr
        call = edv.merkle_prove_consistency_device if consistency else edv.merkle_prove_inclusion_device
        call(d_leafs, d_nodes, leaves, p, p + 8 * n, p + 16 * n, n, p + o_proofs, p + o_st,
             p + o_1 if want1 else None, p + o_2 if want2 else None, device=device)
        back = work.download_at(o_proofs, o_st + n - o_proofs)
        proofs = back[:32 * entries].reshape(-1, 32)
        out1 = back[o_1 - o_proofs:o_1 - o_proofs + 32 * n].reshape(-1, 32) if want1 else None
        out2 = back[o_2 - o_proofs:o_2 - o_proofs + 32 * n].reshape(-1, 32) if want2 else None
        return proofs, off, back[o_st - o_proofs:], out1, out2

    def _prove_batch(self, consistency, pairs, on_device, device, want1, want2):
        a, b = self._checked_pairs(pairs, consistency)
        n = len(a)
        route = self._prove_route(n, on_device)
        if n == 0:
            empty = np.zeros((0, 32), np.uint8)
            return a, b, empty, np.zeros(1, np.uint64), np.zeros(0, np.uint8), empty if want1 else None, \
                empty if want2 else None
        if route == "host":
            single = self.consistency_proof if consistency else self.inclusion_proof
            proofs = [single(int(x), int(y)) for x, y in zip(a, b)]
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(p) for p in proofs], dtype=np.uint64)
            out1 = out2 = None
            if consistency:
                if want1:
                    out1 = _hash_rows([self.merkle_tree_hash(0, int(x)) for x in a])
                    out2 = _hash_rows([self.merkle_tree_hash(0, int(y)) for y in b])
            else:
                if want1:
                    out1 = _hash_rows([self.merkle_tree_hash(0, int(y)) for y in b])
                if want2:
                    out2 = _hash_rows([self.__hashStore.readLeaf(int(x) + 1) for x in a])
            return a, b, _hash_rows([h for p in proofs for h in p]), off, np.full(n, edv.PROOF_OK, np.uint8), out1, out2
        if route == "store":
            proofs, off, status, out1, out2 = self._prove_device(consistency, a, b, want1, want2, device)
        else:
            leafs, nodes = self._store_bytes()
            if consistency:
                proofs, off, status, out1, out2 = edv.merkle_prove_consistency(
                    leafs, nodes, self.leafCount, a, b, want_roots=want1, device=device)
            else:
                proofs, off, status, out1, out2 = edv.merkle_prove_inclusion(
                    leafs, nodes, self.leafCount, a, b, want_roots=want1, want_leaf_hashes=want2, device=device)
        if not (status == edv.PROOF_OK).all():   # the pairs were checked and the slots fit: not reachable
            raise RuntimeError("proof %d came back with status %d" % (int(np.flatnonzero(status != edv.PROOF_OK)[0]),
                                                                     int(status[status != edv.PROOF_OK][0])))
        return a, b, proofs, off, status, out1, out2

    def inclusion_proof_batch(self, pairs, on_device=None, device=0, want_roots=True):
        """inclusion_proof(m, n) for every (m, n) of pairs, with the leaves'
        stored hashes and (want_roots) merkle_tree_hash(0, n), as a ProofBatch.
        on_device None: over a DeviceHashStore, the device from
        MIN_DEVICE_PROVE_PROOFS pairs on (edv_merkle_prove_inclusion_dev over
        the store's mirror); over any other store, the host.  True over
        another store is edv_merkle_prove_inclusion, which copies the store
        per call.  A pair with m >= n raises ValueError, a tree larger than the
        store IndexError, before anything is computed."""
        a, b, proofs, off, status, roots, leaf_hashes = self._prove_batch(False, pairs, on_device, device, want_roots,
                                                                          True)
        return ProofBatch("inclusion", a, b, proofs, off, status, roots=roots, leaf_hashes=leaf_hashes)

    def consistency_proof_batch(self, pairs, on_device=None, device=0, want_roots=True):
        """consistency_proof(first, second) for every pair, with both tree
        heads (want_roots), as a ProofBatch; routed as inclusion_proof_batch.
        first == second is the empty proof; first 0 or above second raises
        ValueError, second above the store IndexError."""
        a, b, proofs, off, status, old_roots, new_roots = self._prove_batch(True, pairs, on_device, device, want_roots,
                                                                            want_roots)
        return ProofBatch("consistency", a, b, proofs, off, status, old_roots=old_roots, new_roots=new_roots)

    def merkle_info_batch(self, seq_nos, on_device=None, device=0, want_roots=True):
        """What Ledger.merkleInfo reads for every seqNo: the audit path of leaf
        seqNo - 1 in the tree of seqNo leaves and that tree's head."""
        seq_nos = [int(s) for s in seq_nos]
        for s in seq_nos:
            if s <= 0:
                raise ValueError("seqNo must be > 0, got %r" % (s,))
        return self.inclusion_proof_batch([(s - 1, s) for s in seq_nos], on_device, device, want_roots)

    # ---- auditing and repairing the store (row f-9)
    def _extend_hashed_parts(self, size, hashes, blob, on_device, step, device):
        """(size, hashes) extended by the leaf hashes in blob (n x 32 bytes) ->
        (size, hashes, [node bytes per call])."""
        hashes, parts = list(hashes), []
        for lo in range(0, len(blob), 32 * step):
            part = blob[lo:lo + 32 * step]
            if on_device:
                node_h, new_h, _ = edv.merkle_extend_hashed(size, b"".join(hashes), part, device=device)
                size, hashes = size + len(part) // 32, [bytes(r) for r in new_h]
                parts.append(node_h.tobytes())
            else:
                size, hashes, nodes = _carry_chain(self.__hasher, size, hashes,
                                                   [part[k:k + 32] for k in range(0, len(part), 32)])
                parts.append(b"".join(nodes))
        return size, hashes, parts

    def _hashed_route(self, n, on_device, max_call):
        if on_device is None:
            on_device = n >= MIN_DEVICE_LEAVES
        if on_device and self.__hasher.hashfunc is not hashlib.sha256:
            raise ValueError("the device extends SHA-256 trees only")
        step = edv.MERKLE_MAX_LEAVES if max_call is None else int(max_call)
        if step < 1 or step > edv.MERKLE_MAX_LEAVES:
            raise ValueError("max_call must be in [1, %d]" % edv.MERKLE_MAX_LEAVES)
        return on_device, step

    def extend_hashed(self, leaf_hashes, on_device=None, max_call=None, device=0):
        """extend from the leaves' hashes instead of their bytes (a store
        loaded from disk, a catch-up peer that sends hashes): leaf_hashes is a
        list of 32-byte hashes, their concatenation, or an (n, 32) uint8 array.
        Tree and hash store end byte-identical to extend on the leaves those
        hashes belong to.  on_device as extend (edv_merkle_extend_hashed per
        max_call hashes; None: from MIN_DEVICE_LEAVES hashes on, the extend's
        own threshold)."""
        if isinstance(leaf_hashes, np.ndarray):
            blob = np.ascontiguousarray(leaf_hashes, dtype=np.uint8).tobytes()
        elif isinstance(leaf_hashes, (bytes, bytearray, memoryview)):
            blob = bytes(leaf_hashes)
        else:
            blob = b"".join(_hash32(h, "a leaf hash") for h in leaf_hashes)
        if len(blob) % 32:
            raise ValueError("not a whole number of hashes")
        on_device, step = self._hashed_route(len(blob) // 32, on_device, max_call)
        if self.__tree_size + len(blob) // 32 > edv.MERKLE_MAX_SIZE:
            raise ValueError("tree size above 2^62")
        size, hashes, parts = self._extend_hashed_parts(self.__tree_size, self.__hashes, blob, on_device, step, device)
        self.__hashStore.writeLeafs(blob)
        self.__hashStore.writeNodes(b"".join(parts))
        self._update(size, hashes)

    def rebuild_nodes(self, on_device=None, device=0):
        """Recompute the node store from the leaf store, without the leaves:
        extend_hashed from an empty tree over the stored leaf hashes, in
        edv.MERKLE_MAX_LEAVES slices; the result replaces the node store
        (hashStore.replaceNodes) and the tree's size and hashes."""
        leafs, _ = self._store_bytes()
        blob = bytes(leafs)
        on_device, step = self._hashed_route(len(blob) // 32, on_device, None)
        size, hashes, parts = self._extend_hashed_parts(0, (), blob, on_device, step, device)
        self.__hashStore.replaceNodes(b"".join(parts))
        self._update(size, hashes)

    def _audit_route(self, entries, on_device):
        """"host", "store" or "copy", as _prove_route."""
        mirrored = isinstance(self.__hashStore, DeviceHashStore)
        if on_device is None:
            on_device = mirrored and entries >= MIN_DEVICE_AUDIT_ENTRIES
        if not on_device:
            return "host"
        if self.__hasher.hashfunc is not hashlib.sha256:
            raise ValueError("the device audits SHA-256 trees only")
        return "store" if mirrored else "copy"

    def _stored_frontier(self, size):
        """The hashes of the tree of `size` leaves as the store holds them, largest first (None: not all there)."""
        store, out = self.__hashStore, []
        try:
            for b in reversed(range(size.bit_length())):
                if (size >> b) & 1:
                    k = (size >> b) - 1
                    out.append(store.readLeaf(k + 1) if b == 0 else store.readNode(node_position(b, k)))
        except IndexError:
            return None
        return out

    def _audit_nodes_host(self, leafs, nodes, count):
        """Nodes 0 .. count - 1 in hashlib, in store order: leaf s (1-based) wrote heights 1 .. ctz(s)."""
        bad, q, s, hasher = [], 0, 2, self.__hasher
        while q < count:
            h, t = 1, s
            while not t & 1 and q < count:
                k = (s >> h) - 1
                if h == 1:
                    left, right = leafs[64 * k:64 * k + 32], leafs[64 * k + 32:64 * k + 64]
                else:
                    pl, pr = node_position(h - 1, 2 * k) - 1, node_position(h - 1, 2 * k + 1) - 1
                    left, right = nodes[32 * pl:32 * pl + 32], nodes[32 * pr:32 * pr + 32]
                if hasher.hash_children(bytes(left), bytes(right)) != nodes[32 * q:32 * q + 32]:
                    bad.append(q + 1)
                q += 1
                h += 1
                t >>= 1
            s += 2
        return bad

    def _audit_store_device(self, ncheck, leaves, device):
        """-> (bad node positions, bad leaf positions), 1-based, through the mirror of a DeviceHashStore."""
        store = self.__hashStore
        d_leafs, d_nodes, nleaves, _ = store.device_arrays()
        empty = np.array([0, edv.AUDIT_NONE], dtype=np.uint64)
        bad_nodes, bad_leaves = [], []
        if ncheck:
            # summary | one status byte per node: every slice adds into the one summary, which alone comes back
            work = store.work_area(16 + ncheck)
            work.upload(empty)
            for lo in range(0, ncheck, edv.MERKLE_MAX_LEAVES):
                cnt = min(edv.MERKLE_MAX_LEAVES, ncheck - lo)
                edv.merkle_audit_nodes_device(d_leafs, d_nodes, nleaves, lo, cnt, work.ptr + 16 + lo, work.ptr,
                                              device=device)
            if int(work.download(16, np.uint64)[0]):
                bad_nodes = (np.flatnonzero(work.download_at(16, ncheck) != edv.AUDIT_OK) + 1).tolist()
        for lo in range(0, len(leaves), edv.MERKLE_MAX_LEAVES):
            part = leaves[lo:lo + edv.MERKLE_MAX_LEAVES]
            n = len(part)
            off = np.zeros(n + 1, dtype=np.uint64)
            off[1:] = np.cumsum([len(x) for x in part], dtype=np.uint64)
            part.append(b"\0" * 8)
            blob = np.frombuffer(b"".join(part), dtype=np.uint8)
            # summary | offsets | leaf bytes (8 readable past the end) | statuses
            o_off, o_blob = 16, 16 + 8 * (n + 1)
            o_st = o_blob + len(blob)
            work = store.work_area(o_st + n)
            p = work.ptr
            work.upload(np.concatenate([empty, off]))
            edv._check(edv.lib().edv_h2d(store.device, p + o_blob, blob.ctypes.data, blob.nbytes))
            edv.merkle_audit_leaves_device(d_leafs, nleaves, lo, p + o_blob, p + o_off, n, p + o_st, p, device=device)
            if int(work.download(16, np.uint64)[0]):
                bad_leaves += (np.flatnonzero(work.download_at(o_st, n) != edv.AUDIT_OK) + 1 + lo).tolist()
        return bad_nodes, bad_leaves

    def audit_store(self, leaves=None, on_device=None, device=0):
        """Check the hash store, which recovery otherwise trusts: the node
        count against get_expected_node_count; every node against its two
        stored children; with `leaves` (the leaves' bytes, in order) every
        stored leaf hash against its leaf; the tree's own size and hashes
        against what the store holds for them.  Returns a StoreAudit.

        Routed as the batched proofs: over a DeviceHashStore the device forms
        on its mirror (edv_merkle_audit_nodes_dev / _leaves_dev; 16 bytes come
        back unless something is bad), from MIN_DEVICE_AUDIT_ENTRIES entries on
        with on_device None; on_device True over another store is the
        host-buffer forms, which copy the store per call; otherwise the same
        checks in hashlib."""
        store = self.__hashStore
        nleaves, nnodes = store.leafCount, store.nodeCount
        expected = self.get_expected_node_count(nleaves)
        # a node past the expected count has no children to check; one that is missing is a count error
        ncheck = min(nnodes, expected)
        counts_ok = nnodes == expected
        if leaves is not None:
            leaves = [bytes(x) for x in leaves]
            counts_ok = counts_ok and len(leaves) == nleaves
            leaves = leaves[:nleaves]
        lcheck = len(leaves) if leaves is not None else 0
        frontier_ok = self.__tree_size == nleaves and self._stored_frontier(nleaves) == list(self.__hashes)
        route = self._audit_route(ncheck + lcheck, on_device)
        if route == "store":
            bad_nodes, bad_leaves = self._audit_store_device(ncheck, leaves or [], device)
        elif route == "copy":
            leafs, nodes = self._store_bytes()
            leafs, nodes = bytes(leafs), bytes(nodes)[:32 * expected].ljust(32 * expected, b"\0")
            bad_nodes, bad_leaves = [], []
            for lo in range(0, ncheck, edv.MERKLE_MAX_LEAVES):
                cnt = min(edv.MERKLE_MAX_LEAVES, ncheck - lo)
                bad, _, status = edv.merkle_audit_nodes(leafs, nodes, nleaves, lo, cnt, device=device)
                if bad:
                    bad_nodes += (np.flatnonzero(status != edv.AUDIT_OK) + 1 + lo).tolist()
            for lo in range(0, lcheck, edv.MERKLE_MAX_LEAVES):
                part = leaves[lo:lo + edv.MERKLE_MAX_LEAVES]
                off = np.zeros(len(part) + 1, dtype=np.uint64)
                off[1:] = np.cumsum([len(x) for x in part], dtype=np.uint64)
                bad, _, status = edv.merkle_audit_leaves(leafs, nleaves, lo, b"".join(part) + b"\0" * 8, off,
                                                         device=device)
                if bad:
                    bad_leaves += (np.flatnonzero(status != edv.AUDIT_OK) + 1 + lo).tolist()
        else:
            leafs, nodes = self._store_bytes()
            bad_nodes = self._audit_nodes_host(leafs, nodes, ncheck)
            bad_leaves = [i + 1 for i in range(lcheck)
                          if self.__hasher.hash_leaf(leaves[i]) != leafs[32 * i:32 * i + 32]]
        return StoreAudit(ncheck, bad_nodes, lcheck, bad_leaves, counts_ok, frontier_ok)

    def get_tree_head(self, seq=None):
        if seq is None:
            seq = self.tree_size
        if seq > self.tree_size:
            raise IndexError
        return {"tree_size": seq, "sha256_root_hash": self.merkle_tree_hash(0, seq) if seq else None}

    @property
    def leafCount(self):
        return self.__hashStore.leafCount

    @property
    def nodeCount(self):
        return self.__hashStore.nodeCount

    @staticmethod
    def get_expected_node_count(leaf_count):
        return leaf_count - _popcount(leaf_count)

    def verify_consistency(self, expected_leaf_count):
        if expected_leaf_count != self.leafCount:
            raise ConsistencyVerificationFailed()
        if self.get_expected_node_count(self.leafCount) != self.nodeCount:
            raise ConsistencyVerificationFailed()
        return True

    def reset(self):
        self.__hashStore.reset()
        self._update(0, ())


# ---- proof verification (row f-7)
_U64 = 1 << 64
_ZERO32 = b"\0" * 32


def _walk_inclusion(hasher, leaf_hash, leaf_index, tree_size, path, root):
    """One audit path (RFC 6962 section 2.1.1) -> (status, calculated root or
    32 zero bytes): the walk of edv_merkle.h in hashlib."""
    if not 0 <= leaf_index < tree_size < _U64:
        return edv.PROOF_RANGE, _ZERO32
    node, last, used, acc = leaf_index, tree_size - 1, 0, leaf_hash
    while last > 0:
        if node & 1 or node < last:
            if used == len(path):
                return edv.PROOF_SHORT, _ZERO32
            acc = hasher.hash_children(path[used], acc) if node & 1 else hasher.hash_children(acc, path[used])
            used += 1
        node >>= 1
        last >>= 1
    if used != len(path):
        return edv.PROOF_LONG, acc
    return (edv.PROOF_OK if acc == root else edv.PROOF_ROOT), acc


def _walk_consistency(hasher, old_size, new_size, old_root, new_root, proof):
    """One consistency proof (RFC 6962 section 2.1.2) -> (status, calculated
    old root + new root, or 64 zero bytes where no walk is made)."""
    none = _ZERO32 + _ZERO32
    if old_size < 0 or new_size < 0 or old_size >= _U64 or new_size >= _U64 or old_size > new_size:
        return edv.PROOF_RANGE, none
    if old_size == new_size:
        return (edv.PROOF_OK if old_root == new_root else edv.PROOF_INCONSISTENT), none
    if old_size == 0:
        return edv.PROOF_OK, none
    node, last, used = old_size - 1, new_size - 1, 0
    while node & 1:
        node >>= 1
        last >>= 1
    if node:
        if not proof:
            return edv.PROOF_SHORT, none
        old = new = proof[0]
        used = 1
    else:
        old = new = old_root
    while last > 0:
        if node & 1 or node < last:
            if used == len(proof):
                return edv.PROOF_SHORT, none
            if node & 1:
                old = hasher.hash_children(proof[used], old)
                new = hasher.hash_children(proof[used], new)
            else:
                new = hasher.hash_children(new, proof[used])
            used += 1
        node >>= 1
        last >>= 1
    if new != new_root:
        return edv.PROOF_ROOT, old + new
    return (edv.PROOF_OK if old == old_root else edv.PROOF_INCONSISTENT), old + new


class ProofVerdicts:
    """What a batched verification returned: `status`, a uint8 array of
    edv.PROOF_* (one per proof), `ok`, the same as bools, and `computed`, the
    calculated roots ((n, 32); consistency (n, 64): old, then new) when asked
    for, else None.  len() and iteration (bools) as a list of verdicts;
    raise_for(i) raises what the single call raises for entry i."""

    def __init__(self, status, computed=None):
        self.status = np.asarray(status, dtype=np.uint8)
        self.ok = self.status == edv.PROOF_OK
        self.computed = computed

    def __len__(self):
        return len(self.status)

    def __iter__(self):
        return iter(bool(x) for x in self.ok)

    def raise_for(self, i):
        """True for an accepted proof; else the single call's exception:
        ValueError (sizes out of range), ProofError, ConsistencyError."""
        st = int(self.status[i])
        if st == edv.PROOF_OK:
            return True
        if st == edv.PROOF_RANGE:
            raise ValueError("proof %d: leaf index not below the tree size, or the older tree is the bigger one" % i)
        if st == edv.PROOF_SHORT:
            raise ProofError("proof %d is too short" % i)
        if st == edv.PROOF_LONG:
            raise ProofError("proof %d is too long" % i)
        if st == edv.PROOF_ROOT:
            raise ProofError("proof %d: constructed root hash differs from the provided root hash" % i)
        if st == edv.PROOF_INCONSISTENT:
            raise ConsistencyError("proof %d: inconsistency: first root hash does not match" % i)
        raise VerifyError("proof %d was not verified" % i)

    def raise_first(self):
        """True if every proof is accepted, else the first failing entry's exception."""
        bad = np.flatnonzero(~self.ok)
        return self.raise_for(int(bad[0])) if len(bad) else True


def _hash32(h, what):
    h = bytes(h)
    if len(h) != 32:
        raise ValueError("%s must be 32 bytes" % what)
    return h


def _pack_proofs(proofs):
    """list of lists of 32-byte hashes -> ((entries, 32) uint8 array, n + 1 offsets in entries)."""
    off = np.zeros(len(proofs) + 1, dtype=np.uint64)
    flat = []
    for i, p in enumerate(proofs):
        flat.extend(_hash32(h, "a proof entry") for h in p)
        off[i + 1] = len(flat)
    return np.frombuffer(b"".join(flat), dtype=np.uint8).reshape(-1, 32), off


def _in_u64(x):
    return 0 <= x < _U64


class MerkleVerifier:
    """The reference's ledger/merkle_verifier.py by name, call shape, return
    value and exception, written from RFC 6962 sections 2.1.1 and 2.1.2; and
    the same checks for a batch of proofs in one device call (gfx950 kernels
    edv_merkle_verify_inclusion_kernel / edv_merkle_verify_consistency_kernel).
    A single proof is at most 64 node hashes: always on the host."""

    def __init__(self, hasher=None):
        self.hasher = hasher or TreeHasher()

    def __repr__(self):
        return "%r(hasher: %r)" % (self.__class__.__name__, self.hasher)

    # ---- single proofs (host)
    def verify_tree_consistency(self, old_tree_size, new_tree_size, old_root, new_root, proof):
        st, _ = _walk_consistency(self.hasher, int(old_tree_size), int(new_tree_size), bytes(old_root),
                                  bytes(new_root), [bytes(h) for h in proof])
        return ProofVerdicts([st]).raise_for(0)

    def verify_leaf_hash_inclusion(self, leaf_hash, leaf_index, proof, sth):
        st, _ = _walk_inclusion(self.hasher, bytes(leaf_hash), int(leaf_index), int(sth.tree_size),
                                [bytes(h) for h in proof], bytes(sth.sha256_root_hash))
        return ProofVerdicts([st]).raise_for(0)

    def verify_leaf_inclusion(self, leaf, leaf_index, proof, sth):
        return self.verify_leaf_hash_inclusion(self.hasher.hash_leaf(leaf), leaf_index, proof, sth)

    @classmethod
    def audit_path_length(cls, index, tree_size):
        length, last = 0, tree_size - 1
        while last > 0:
            if index & 1 or index < last:
                length += 1
            index >>= 1
            last >>= 1
        return length

    # ---- batches
    def _device_default(self, n, on_device):
        if on_device is None:
            on_device = n >= MIN_DEVICE_VERIFY_PROOFS
        if on_device and self.hasher.hashfunc is not hashlib.sha256:
            raise ValueError("the device verifies SHA-256 trees only")
        return on_device

    def _inclusion(self, leaves, leaf_hashes, leaf_indices, sizes, roots, paths, off, on_device, device, want_computed,
                   max_call=None):
        """leaves: list of bytes, or None with leaf_hashes an (n, 32) array;
        roots (n, 32), paths (entries, 32) and off (n + 1, in entries) are the
        packed arrays the device call takes as they are."""
        n = len(off) - 1
        idx, size = [int(x) for x in leaf_indices], [int(x) for x in sizes]
        given = len(leaves) if leaf_hashes is None else len(leaf_hashes)
        if not len(idx) == len(size) == len(roots) == given == n:
            raise ValueError("leaves, leaf indices, proofs and tree heads differ in number")
        status = np.zeros(n, dtype=np.uint8)
        computed = np.zeros((n, 32), dtype=np.uint8) if want_computed else None
        if not self._device_default(n, on_device):
            pb, rb = paths.tobytes(), roots.tobytes()
            for i in range(n):
                lo, hi = 32 * int(off[i]), 32 * int(off[i + 1])
                lh = self.hasher.hash_leaf(leaves[i]) if leaf_hashes is None else leaf_hashes[i].tobytes()
                st, comp = _walk_inclusion(self.hasher, lh, idx[i], size[i], [pb[k:k + 32] for k in range(lo, hi, 32)],
                                           rb[32 * i:32 * i + 32])
                status[i] = st
                if want_computed:
                    computed[i] = np.frombuffer(comp, dtype=np.uint8)
            return ProofVerdicts(status, computed)
        # integers the C-ABI cannot carry are out of range whatever the proof says
        fits = [_in_u64(a) and _in_u64(b) for a, b in zip(idx, size)]
        idx_a = np.array([a if f else 0 for a, f in zip(idx, fits)], dtype=np.uint64)
        size_a = np.array([b if f else 0 for b, f in zip(size, fits)], dtype=np.uint64)
        step = edv.MERKLE_MAX_LEAVES if max_call is None else int(max_call)
        if step < 1 or step > edv.MERKLE_MAX_LEAVES:
            raise ValueError("max_call must be in [1, %d]" % edv.MERKLE_MAX_LEAVES)
        for lo in range(0, n, step):
            hi = min(n, lo + step)
            kw = {}
            if leaf_hashes is None:
                loff = np.zeros(hi - lo + 1, dtype=np.uint64)
                loff[1:] = np.cumsum([len(x) for x in leaves[lo:hi]], dtype=np.uint64)
                kw = dict(leaves=np.frombuffer(b"".join(leaves[lo:hi]) + b"\0" * 8, dtype=np.uint8), leaf_off=loff)
            else:
                kw = dict(leaf_hashes=np.ascontiguousarray(leaf_hashes[lo:hi]))
            st, comp = edv.merkle_verify_inclusion(idx_a[lo:hi], size_a[lo:hi], np.ascontiguousarray(roots[lo:hi]),
                                                   paths, off[lo:hi + 1], want_computed=want_computed, device=device,
                                                   **kw)
            status[lo:hi] = st
            if want_computed:
                computed[lo:hi] = comp
        return ProofVerdicts(status, computed)

    @staticmethod
    def _heads(sths):
        sths = list(sths)
        roots = np.frombuffer(b"".join(_hash32(s.sha256_root_hash, "a root hash") for s in sths),
                              dtype=np.uint8).reshape(-1, 32)
        return [s.tree_size for s in sths], roots

    def verify_leaf_inclusion_batch(self, leaves, leaf_indices, proofs, sths, on_device=None, device=0,
                                    want_computed=False):
        """verify_leaf_inclusion for every (leaf, leaf_index, proof, sth), as a
        ProofVerdicts; one edv_merkle_verify_inclusion call from
        MIN_DEVICE_VERIFY_PROOFS proofs on (on_device None), else the same
        walk in hashlib."""
        sizes, roots = self._heads(sths)
        paths, off = _pack_proofs(list(proofs))
        return self._inclusion([bytes(x) for x in leaves], None, list(leaf_indices), sizes, roots, paths, off,
                               on_device, device, want_computed)

    def verify_leaf_hash_inclusion_batch(self, leaf_hashes, leaf_indices, proofs, sths, on_device=None, device=0,
                                         want_computed=False):
        sizes, roots = self._heads(sths)
        paths, off = _pack_proofs(list(proofs))
        lh = np.frombuffer(b"".join(_hash32(h, "a leaf hash") for h in leaf_hashes), dtype=np.uint8).reshape(-1, 32)
        return self._inclusion(None, lh, list(leaf_indices), sizes, roots, paths, off, on_device, device, want_computed)

    def verify_tree_consistency_batch(self, items, on_device=None, device=0, want_computed=False):
        """items: (old_tree_size, new_tree_size, old_root, new_root, proof)
        each, the arguments of verify_tree_consistency."""
        items = [(int(a), int(b), _hash32(ra, "a root hash"), _hash32(rb, "a root hash"), list(p))
                 for a, b, ra, rb, p in items]
        n = len(items)
        if not self._device_default(n, on_device):
            res = [_walk_consistency(self.hasher, a, b, ra, rb, [_hash32(h, "a proof entry") for h in p])
                   for a, b, ra, rb, p in items]
            computed = None
            if want_computed:
                computed = np.frombuffer(b"".join(c for _, c in res), dtype=np.uint8).reshape(-1, 64)
            return ProofVerdicts([st for st, _ in res], computed)
        proofs, off = _pack_proofs([p for *_, p in items])
        fits = [_in_u64(a) and _in_u64(b) for a, b, *_ in items]
        # sizes the C-ABI cannot carry go in as (1, 0): out of range
        old = np.array([it[0] if f else 1 for it, f in zip(items, fits)], dtype=np.uint64)
        new = np.array([it[1] if f else 0 for it, f in zip(items, fits)], dtype=np.uint64)
        status, computed = edv.merkle_verify_consistency(old, new, b"".join(it[2] for it in items),
                                                         b"".join(it[3] for it in items), proofs, off,
                                                         want_computed=want_computed, device=device)
        return ProofVerdicts(status, computed)

    def verify_append_batch(self, old_size, leaves, batch, on_device=None, device=0, max_call=None,
                            want_computed=False):
        """Check what append_batch returned for `leaves` appended to a tree of
        old_size leaves: leaf i has index old_size + i in the tree of
        old_size + i + 1 leaves, whose root is batch.roots[i]; its audit path
        (smallest subtree first: the verifier's order, lowest level first) is
        read where the AppendBatch holds it, packed, with no repacking."""
        leaves = [bytes(x) for x in leaves]
        n = len(leaves)
        if n != len(batch) or int(old_size) != batch.old_size:
            raise ValueError("the AppendBatch is not that of these leaves")
        off = np.zeros(n + 1, dtype=np.uint64)   # leaf i's path has popcount(old_size + i) entries
        off[1:] = np.cumsum([_popcount(batch.old_size + i) for i in range(n)], dtype=np.uint64)
        if int(off[-1]) != len(batch.paths):
            raise ValueError("the AppendBatch's packed paths do not match its sizes")
        idx = [batch.old_size + i for i in range(n)]
        return self._inclusion(leaves, None, idx, [s + 1 for s in idx], np.ascontiguousarray(batch.roots),
                               np.ascontiguousarray(batch.paths), off, on_device, device, want_computed, max_call)

    def verify_proof_batch(self, batch, on_device=None, device=0, want_computed=False):
        """Check a ProofBatch (row f-8) as it is, with no repacking: audit
        paths against the batch's leaf hashes and tree heads, consistency
        proofs against its old and new roots.  The batch must carry them
        (want_roots)."""
        proofs, off = np.ascontiguousarray(batch.proofs), np.ascontiguousarray(batch.off, dtype=np.uint64)
        if batch.kind == "inclusion":
            if batch.roots is None or batch.leaf_hashes is None:
                raise ValueError("the ProofBatch holds no tree heads")
            return self._inclusion(None, np.ascontiguousarray(batch.leaf_hashes), batch.index, batch.size,
                                   np.ascontiguousarray(batch.roots), proofs, off, on_device, device, want_computed)
        if batch.old_roots is None or batch.new_roots is None:
            raise ValueError("the ProofBatch holds no tree heads")
        n = len(batch)
        old_roots, new_roots = np.ascontiguousarray(batch.old_roots), np.ascontiguousarray(batch.new_roots)
        if self._device_default(n, on_device):
            status, computed = edv.merkle_verify_consistency(batch.index, batch.size, old_roots, new_roots, proofs, off,
                                                             want_computed=want_computed, device=device)
            return ProofVerdicts(status, computed)
        res = [_walk_consistency(self.hasher, int(batch.index[i]), int(batch.size[i]), old_roots[i].tobytes(),
                                 new_roots[i].tobytes(), batch.proof(i)) for i in range(n)]
        computed = None
        if want_computed:
            computed = np.frombuffer(b"".join(c for _, c in res), dtype=np.uint8).reshape(-1, 64)
        return ProofVerdicts([st for st, _ in res], computed)


def verify_append_batch(old_size, leaves, batch, on_device=None, device=0, max_call=None):
    """MerkleVerifier().verify_append_batch: the verdicts on an AppendBatch."""
    return MerkleVerifier().verify_append_batch(old_size, leaves, batch, on_device, device, max_call)
