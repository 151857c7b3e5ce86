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
edv_merkle_pass_kernel / edv_merkle_finish_kernel); `append`, the proofs and
everything that reads the store stay on the host.

`append_batch` (row f-6) is `extend` that also returns what each `append`
returns (ledger/ledger.py:145-155: the audit path, and the root hash read after
it), one edv_merkle_append_batch call per batch (kernel
edv_merkle_append_kernel after the extend's): what `Ledger.commitTxns`
(ledger.py) needs for a 3PC batch.
"""
import hashlib
from binascii import hexlify

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


class ConsistencyVerificationFailed(Exception):
    pass


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
