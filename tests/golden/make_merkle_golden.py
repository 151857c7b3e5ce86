#!/usr/bin/env python3
"""Generate tests/golden/merkle_golden.json by running the REFERENCE's own
CompactMerkleTree (ledger/compact_merkle_tree.py) over leaves from
tests/merkle_cases.py.  Run with the reference checkout on PYTHONPATH; only
the outputs (data, hex) are committed, nothing of the reference is copied.

The reference's in-memory hash store keeps the (start, height, hash) tuple it
is handed, and its own proofs then fail on it; the store used here keeps the
hash (as the reference's file store does).  With it the reference's
inclusion_proof / consistency_proof work, and its MerkleVerifier accepts them
(checked below before anything is written).

Per tree size: hashes, root, SHA-256 of the concatenated leaf store and node
store, the audit paths `append` returned for the last three leaves, and
inclusion / consistency proofs for a handful of pairs.
"""
import hashlib
import json
import os
import sys

from ledger.compact_merkle_tree import CompactMerkleTree          # reference modules
from ledger.hash_stores.memory_hash_store import MemoryHashStore
from ledger.merkle_verifier import MerkleVerifier
from ledger.tree_hasher import TreeHasher

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import merkle_cases as mc  # noqa: E402  (own code: the seeded leaves)

SEED = 7
SIZES = [1, 2, 3, 7, 8, 255, 256, 257, 777, 1000]


class HashOnlyStore(MemoryHashStore):
    def writeNode(self, node):
        super().writeNode(node[2])


def pairs(size):
    """(m, n) for inclusion_proof and (a, b) for consistency_proof on a tree of `size` leaves."""
    inc = {(0, size), (size - 1, size), (size // 2, size), (size // 3, max(size - 1, size // 3 + 1)), (0, 1)}
    con = {(size, size), (1, size), (max(1, size // 2), size), (max(1, size - 1), size),
           (max(1, size // 3), max(1, size - 1))}
    return sorted(p for p in inc if p[0] < p[1] <= size), sorted(p for p in con if 0 < p[0] <= p[1] <= size)


def main():
    leaves = mc.leaves_of(SEED, max(SIZES))
    tree = CompactMerkleTree(TreeHasher(), hashStore=HashOnlyStore())
    verifier = MerkleVerifier()
    roots = {0: tree.root_hash}
    audit, cases = [], []
    for s in range(1, max(SIZES) + 1):
        audit.append(tree.append(leaves[s - 1]))
        roots[s] = tree.root_hash
        if s not in SIZES:
            continue
        store = tree.hashStore
        inc, con = pairs(s)
        row = {
            "size": s,
            "hashes": [h.hex() for h in tree.hashes],
            "root": tree.root_hash.hex(),
            "leaf_store_sha256": hashlib.sha256(b"".join(store.readLeafs(1, s + 1))).hexdigest(),
            "node_store_sha256": hashlib.sha256(b"".join(store.readNodes(1, store.nodeCount + 1))).hexdigest(),
            "node_count": store.nodeCount,
            "audit_paths": [{"leaf": i, "path": [h.hex() for h in audit[i - 1]]} for i in range(max(1, s - 2), s + 1)],
            "inclusion": [], "consistency": [],
        }
        for m, n in inc:
            proof = tree.inclusion_proof(m, n)
            assert verifier.verify_leaf_hash_inclusion(store.readLeaf(m + 1), m, proof,
                                                       type("STH", (), {"tree_size": n, "sha256_root_hash": roots[n]})())
            row["inclusion"].append({"m": m, "n": n, "proof": [h.hex() for h in proof]})
        for a, b in con:
            proof = tree.consistency_proof(a, b)
            assert verifier.verify_tree_consistency(a, b, roots[a], roots[b], proof)
            row["consistency"].append({"a": a, "b": b, "root_a": roots[a].hex(), "root_b": roots[b].hex(),
                                       "proof": [h.hex() for h in proof]})
        cases.append(row)
    with open(os.path.join(HERE, "merkle_golden.json"), "w") as f:
        json.dump({"generated_with": "reference ledger.compact_merkle_tree.CompactMerkleTree.append over a hash store "
                                     "that keeps node[2] (python %s)" % sys.version.split()[0],
                   "seed": SEED, "max_len": 300, "cases": cases}, f, indent=1)
    print(len(cases), "merkle cases")


if __name__ == "__main__":
    main()
