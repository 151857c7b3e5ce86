#!/usr/bin/env python3
"""Generate tests/golden/merkle_append_golden.json by running the REFERENCE's
own CompactMerkleTree.append (ledger/compact_merkle_tree.py) over the 1,000
seeded leaves of merkle_golden.json.  Run with the reference checkout on
PYTHONPATH, as make_merkle_golden.py; only the outputs (data, hex) are
committed, nothing of the reference is copied.

Per append the reference returns the audit path; the root hash is read after
it (what Ledger._build_merkle_proof puts into the REPLY).  Recorded: SHA-256 of
the 1,000 concatenated roots and of the concatenated audit paths, the entry
count, the full (root, path) of a few leaves, and the same digests for the 300
appends that follow a 700-leaf tree.
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

SEED = 7           # make_merkle_golden.py's
LEAVES = 1000
FULL = [1, 2, 3, 255, 256, 257, 1000]
SPLIT = 700


def digests(roots, paths):
    blob = b"".join(h for p in paths for h in p)
    return {"roots_sha256": hashlib.sha256(b"".join(roots)).hexdigest(),
            "paths_sha256": hashlib.sha256(blob).hexdigest(), "entries": len(blob) // 32}


def main():
    leaves = mc.leaves_of(SEED, LEAVES)
    tree = CompactMerkleTree(TreeHasher(), hashStore=MemoryHashStore())
    roots, paths = [], []
    for leaf in leaves:
        paths.append(list(tree.append(leaf)))
        roots.append(tree.root_hash)
    out = {"generated_with": "reference ledger.compact_merkle_tree.CompactMerkleTree.append (python %s)"
                             % sys.version.split()[0],
           "seed": SEED, "max_len": 300, "leaves": LEAVES,
           "all": digests(roots, paths),
           "full": [{"leaf": i, "root": roots[i - 1].hex(), "path": [h.hex() for h in paths[i - 1]]} for i in FULL],
           "after": dict(digests(roots[SPLIT:], paths[SPLIT:]), old_size=SPLIT, n=LEAVES - SPLIT)}
    with open(os.path.join(HERE, "merkle_append_golden.json"), "w") as f:
        json.dump(out, f, indent=1)
    print(out["all"], out["after"])


if __name__ == "__main__":
    main()
