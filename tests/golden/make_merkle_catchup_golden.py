#!/usr/bin/env python3
"""Generate tests/golden/merkle_catchup_golden.json by running the REFERENCE's
own catch-up check (plenum/common/ledger_manager.py:564-609: a temporary tree
over the replies' transactions, CompactMerkleTree.extended, and
MerkleVerifier.verify_tree_consistency from it to the target) over the real
cases of tests/merkle_catchup_cases.py, intact and after each of its mutations.
Run with the reference checkout on PYTHONPATH; only recorded outcomes (data) are
committed, nothing of the reference is copied: the inputs are the seeded cases.

Per case: one outcome per reply, as an index into "names": "True", or the
exception class and, for a ProofError, which of too short / too long / mismatch
it was (read off the reference's message).  Reply k's temporary tree holds the
transactions of replies 0 .. k, whether or not an earlier reply failed: that is
what the statuses of one call are computed over.
"""
import json
import os
import sys

from ledger.compact_merkle_tree import CompactMerkleTree          # reference modules
from ledger.hash_stores.memory_hash_store import MemoryHashStore
from ledger import error
from ledger.merkle_verifier import MerkleVerifier
from ledger.tree_hasher import TreeHasher

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import merkle_catchup_cases as cc  # noqa: E402  (own code: the seeded cases, the mutations)
import merkle_verify_cases as vc  # noqa: E402

NAMES = [vc.STATUS_NAME[s] for s in sorted(vc.STATUS_NAME)]


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
    v, old_trees, out = MerkleVerifier(), {}, {}
    for case in cc.all_cases():
        if not case.real:
            continue
        if case.old not in old_trees:
            t = CompactMerkleTree(TreeHasher(), hashStore=HashOnlyStore())
            for leaf in cc._LEAVES[:case.old]:
                t.append(leaf)
            assert list(t.hashes) == case.old_hashes
            old_trees[case.old] = t
        row, txns = [], []
        for part, proof in zip(case.parts, case.proofs):
            txns = txns + part
            temp = old_trees[case.old].extended(txns)
            row.append(NAMES.index(outcome(lambda: v.verify_tree_consistency(
                temp.tree_size, case.final_size, temp.root_hash, case.final_root, proof))))
        out[case.name] = row
    with open(os.path.join(HERE, "merkle_catchup_golden.json"), "w") as f:
        json.dump({"generated_with": "reference ledger.compact_merkle_tree.CompactMerkleTree.extended and "
                                     "ledger.merkle_verifier.MerkleVerifier.verify_tree_consistency over the real "
                                     "cases of tests/merkle_catchup_cases.py (python %s)" % sys.version.split()[0],
                   "names": NAMES, "outcomes": out}, f, separators=(",", ":"))
    print(len(out), "cases,", sum(len(r) for r in out.values()), "replies")


if __name__ == "__main__":
    main()
