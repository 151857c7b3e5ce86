#!/usr/bin/env python3
"""Generate tests/golden/merkle_verify_golden.json by running the REFERENCE's
own MerkleVerifier (ledger/merkle_verifier.py) over the proofs of the ten trees
of merkle_golden.json, intact and after each mutation of
tests/merkle_verify_cases.py.  Run with the reference checkout on PYTHONPATH;
only inputs and recorded outcomes (data, hex) are committed, nothing of the
reference is copied.

Per proof: the inputs once, and per mutation the outcome: "True", or the
exception class and, for a ProofError, which of too short / too long /
mismatch it was (read off the reference's message).
"""
import json
import os
import sys

from ledger.compact_merkle_tree import CompactMerkleTree          # reference modules
from ledger.hash_stores.memory_hash_store import MemoryHashStore
from ledger import error
from ledger.merkle_verifier import MerkleVerifier
from ledger.tree_hasher import TreeHasher
from ledger.util import STH

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import merkle_cases as mc  # noqa: E402  (own code: the seeded leaves, the mutations)
import merkle_verify_cases as vc  # noqa: E402


class HashOnlyStore(MemoryHashStore):  # as make_merkle_golden.py: the store keeps the hash alone
    def writeNode(self, node):
        super().writeNode(node[2])


def outcome(call):
    try:
        assert call() is True
        return "True"
    except error.ConsistencyError:
        return "ConsistencyError"
    except error.ProofError as ex:
        msg = str(ex).lower()
        return "ProofError: " + ("too short" if "too short" in msg else "too long" if "too long" in msg else "mismatch")
    except ValueError:
        return "ValueError"


def main():
    g = mc.load_golden()
    leaves = g["leaves"]
    tree = CompactMerkleTree(TreeHasher(), hashStore=HashOnlyStore())
    roots = {0: tree.root_hash}
    for s in range(1, len(leaves) + 1):
        tree.append(leaves[s - 1])
        roots[s] = tree.root_hash
    v = MerkleVerifier()
    inc, con, seen = [], [], set()
    for case in g["cases"]:
        for p in case["inclusion"]:
            key = ("i", p["m"], p["n"])
            if key in seen:
                continue
            seen.add(key)
            base = (tree.hashStore.readLeaf(p["m"] + 1), p["m"], p["n"], [bytes.fromhex(h) for h in p["proof"]],
                    roots[p["n"]])
            row = {"m": p["m"], "n": p["n"], "leaf_hash": base[0].hex(), "root": base[4].hex(), "proof": p["proof"],
                   "outcomes": {}}
            for name in vc.INCLUSION_MUTATIONS:
                lh, m, n, proof, root = vc.mutate_inclusion(*base, name)
                row["outcomes"][name] = outcome(lambda: v.verify_leaf_hash_inclusion(lh, m, proof, STH(n, root)))
            assert row["outcomes"]["intact"] == "True"
            inc.append(row)
        for p in case["consistency"]:
            key = ("c", p["a"], p["b"])
            if key in seen:
                continue
            seen.add(key)
            base = (p["a"], p["b"], bytes.fromhex(p["root_a"]), bytes.fromhex(p["root_b"]),
                    [bytes.fromhex(h) for h in p["proof"]])
            row = dict(p, outcomes={})
            for name in vc.CONSISTENCY_MUTATIONS:
                args = vc.mutate_consistency(*base, name)
                row["outcomes"][name] = outcome(lambda: v.verify_tree_consistency(*args))
            assert row["outcomes"]["intact"] == "True"
            con.append(row)
    with open(os.path.join(HERE, "merkle_verify_golden.json"), "w") as f:
        json.dump({"generated_with": "reference ledger.merkle_verifier.MerkleVerifier over the proofs of "
                                     "merkle_golden.json (python %s)" % sys.version.split()[0],
                   "inclusion": inc, "consistency": con}, f, indent=1)
    print(len(inc), "inclusion and", len(con), "consistency proofs,", len(vc.INCLUSION_MUTATIONS), "and",
          len(vc.CONSISTENCY_MUTATIONS), "mutations")


if __name__ == "__main__":
    main()
