#!/usr/bin/env python3
"""Generate tests/golden/merkle_prove_golden.json by running the REFERENCE's own
CompactMerkleTree (ledger/compact_merkle_tree.py: merkle_tree_hash,
inclusion_proof, consistency_proof) over the 1,000 leaves of
tests/merkle_cases.leaves_of(7, 1000), with the hash-only store of
make_merkle_golden.py.  Run with the reference checkout on PYTHONPATH; only
recorded results (data, hex) are committed, nothing of the reference is copied.

Recorded:
  all_pairs     for every n of SMALL (1..65) and LARGE: the SHA-256 of all
                inclusion proofs (m, n), m = 0 .. n - 1, one after another (each
                proof its entries in order), their total entry count, and the
                same for the consistency proofs (a, n), a = 1 .. n
  merkle_info   for s = 1 .. 1000: SHA-256(root of the first s leaves | the
                audit path of leaf s - 1 in that tree), what Ledger.merkleInfo
                reads; and one digest over all roots and one over all paths
  full          about forty proofs entry by entry
"""
import hashlib
import json
import os
import sys

from ledger.compact_merkle_tree import CompactMerkleTree          # reference modules
from ledger.hash_stores.memory_hash_store import MemoryHashStore
from ledger.tree_hasher import TreeHasher

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import merkle_cases as mc  # noqa: E402  (own code: the seeded leaves)

SEED = 7
LEAVES = 1000
SMALL = list(range(1, 66))
LARGE = [255, 256, 257, 777, 1000]
FULL_INCLUSION = [(0, 1), (0, 2), (1, 2), (2, 3), (0, 5), (4, 5), (3, 7), (6, 7), (0, 11), (8, 11), (10, 11), (5, 64),
                  (64, 65), (0, 65), (254, 255), (0, 257), (256, 257), (100, 777), (776, 777), (512, 777), (999, 1000),
                  (0, 1000), (768, 1000)]
FULL_CONSISTENCY = [(1, 1), (1, 2), (2, 3), (3, 5), (4, 7), (6, 7), (7, 8), (8, 11), (5, 11), (10, 11), (64, 65), (33, 65),
                    (255, 256), (256, 257), (192, 257), (1, 777), (776, 777), (512, 777), (1000, 1000), (999, 1000),
                    (1, 1000), (768, 1000), (333, 1000)]


class HashOnlyStore(MemoryHashStore):  # as make_merkle_golden.py: the store keeps the hash alone
    def writeNode(self, node):
        super().writeNode(node[2])


def main():
    leaves = mc.leaves_of(SEED, LEAVES)
    tree = CompactMerkleTree(TreeHasher(), hashStore=HashOnlyStore())
    for leaf in leaves:
        tree.append(leaf)
    all_pairs = []
    for n in SMALL + LARGE:
        inc = [tree.inclusion_proof(m, n) for m in range(n)]
        con = [tree.consistency_proof(a, n) for a in range(1, n + 1)]
        all_pairs.append({
            "n": n,
            "inclusion_sha256": hashlib.sha256(b"".join(h for p in inc for h in p)).hexdigest(),
            "inclusion_entries": sum(len(p) for p in inc),
            "consistency_sha256": hashlib.sha256(b"".join(h for p in con for h in p)).hexdigest(),
            "consistency_entries": sum(len(p) for p in con),
        })
    roots = [tree.merkle_tree_hash(0, s) for s in range(1, LEAVES + 1)]
    paths = [tree.inclusion_proof(s - 1, s) for s in range(1, LEAVES + 1)]
    info = {
        "per_seq_no_sha256": [hashlib.sha256(r + b"".join(p)).hexdigest() for r, p in zip(roots, paths)],
        "roots_sha256": hashlib.sha256(b"".join(roots)).hexdigest(),
        "paths_sha256": hashlib.sha256(b"".join(h for p in paths for h in p)).hexdigest(),
    }
    full = {
        "inclusion": [{"m": m, "n": n, "root": tree.merkle_tree_hash(0, n).hex(),
                       "proof": [h.hex() for h in tree.inclusion_proof(m, n)]} for m, n in FULL_INCLUSION],
        "consistency": [{"a": a, "b": b, "root_a": tree.merkle_tree_hash(0, a).hex(),
                         "root_b": tree.merkle_tree_hash(0, b).hex(),
                         "proof": [h.hex() for h in tree.consistency_proof(a, b)]} for a, b in FULL_CONSISTENCY],
    }
    with open(os.path.join(HERE, "merkle_prove_golden.json"), "w") as f:
        json.dump({"generated_with": "reference ledger.compact_merkle_tree.CompactMerkleTree over a hash store that "
                                     "keeps node[2] (python %s)" % sys.version.split()[0],
                   "seed": SEED, "leaves": LEAVES, "max_len": 300, "all_pairs": all_pairs, "merkle_info": info,
                   "full": full}, f, indent=1)
    print(sum(r["n"] for r in all_pairs) * 2 + LEAVES, "proofs recorded")


if __name__ == "__main__":
    main()
