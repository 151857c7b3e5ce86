"""The ledger over the compact Merkle tree, with a 3PC batch committed in one
device call.

Same names, call shapes and return values as the reference's two Ledger
classes, written from their semantics:

  ledger/ledger.py:116-158                add / append -> seqNo, rootHash, auditPath
  ledger/ledger.py:95-114                 recoverTreeFromTxnLog / recoverTreeFromHashStore
  ledger/ledger.py:197-206                merkleInfo
  plenum/common/ledger.py:34-53           appendTxns (uncommittedTree, uncommittedRootHash)
  plenum/common/ledger.py:71-96           commitTxns: txn.update(self.append(txn)) per txn
  plenum/common/ledger.py:98-137          discardTxns, treeWithAppliedTxns
  plenum/client/client.py:846-873         verifyMerkleProof -> verify_merkle_proofs (row f-7)
  plenum/common/ledger_manager.py:564-609 hasValidCatchupReplies -> Ledger.verify_catchup_txns
  plenum/server/node.py:3024-3034         getReplyFromLedger: merkleInfo per reply -> merkleInfoBatch (row f-8)
  plenum/common/ledger_manager.py:995-998 a consistency proof and both roots -> consistency_proofs (row f-8)
  ledger/ledger.py:70-114                 recoverTree trusts a store that has leaves -> auditHashStore,
                                          recoverTreeVerified (row f-9)
  plenum/common/ledger_manager.py:505-609 per reply hasValidCatchupReplies, then _add_txn -> ledger.add per
                                          transaction -> applyCatchupReplies, one call per pass (row f-10)

commitTxns(count) is one CompactMerkleTree.append_batch call
(edv_merkle_append_batch from merkle.MIN_DEVICE_APPEND_LEAVES transactions
on): every committed transaction still gets its own rootHash and auditPath.
applyCatchupReplies(replies, final_size, final_root_hash) is one
CompactMerkleTree.extend_verified call for a pass of in-order catch-up
replies (edv_merkle_catchup from merkle.MIN_DEVICE_CATCHUP_LEAVES transactions
on): the leading replies whose consistency proofs verify are committed, each
transaction hashed once, and a merkle.CatchupResult says which they were.
The transaction log is a list in memory; it holds each transaction as it was
when it was hashed, a copy taken before the committed transaction is updated
with its Merkle info (the reference logs the serialization made before the
update), so recovery from the log hashes what was hashed and getBySeqNo never
shows rootHash / auditPath.  Transaction metadata stays out: the
class never looks inside a transaction, it only `update`s the committed ones
(so neither append_txns_metadata nor appendTxns' seq-no check is here).
"""
from copy import copy

from . import base58
from .merkle import STH, CompactMerkleTree, ConsistencyVerificationFailed, MerkleVerifier

MERKLE_KEYS = ("auditPath", "seqNo", "rootHash")  # what a committed transaction carries beyond what was hashed


def _bytes_as_they_are(txn):
    return txn.encode() if isinstance(txn, str) else bytes(txn)


def _as_hash(h):
    return base58.b58decode(h) if isinstance(h, str) else bytes(h)


def verify_merkle_proofs(results, serialize_for_tree=None, on_device=None, device=0):
    """Check the Merkle proof every result carries, all in one batched call
    (row f-7; plenum/client/client.py:846-873, verifyMerkleProof, one
    verify_leaf_inclusion per reply there).  A result is a dict with `seqNo`,
    `rootHash` and `auditPath`, base58 as Ledger.commitTxns writes them; its
    leaf is serialize_for_tree of the result without those three keys (pass
    the ledger's own serializer: the default, as Ledger's, takes the
    transaction to be the bytes, which a dict is not), at index seqNo - 1 of
    the tree of seqNo leaves.  Returns True, or raises the first failing
    entry's exception (ValueError, ProofError)."""
    results = list(results)
    serialize = serialize_for_tree or _bytes_as_they_are
    leaves, indices, proofs, sths = [], [], [], []
    for r in results:
        seqNo = int(r["seqNo"])
        leaves.append(serialize({k: v for k, v in r.items() if k not in MERKLE_KEYS}))
        indices.append(seqNo - 1)
        proofs.append([_as_hash(a) for a in r["auditPath"]])
        sths.append(STH(tree_size=seqNo, sha256_root_hash=_as_hash(r["rootHash"])))
    return MerkleVerifier().verify_leaf_inclusion_batch(leaves, indices, proofs, sths, on_device=on_device,
                                                        device=device).raise_first()


class Ledger:
    def __init__(self, tree=None, serialize_for_tree=None, transactionLog=None, on_device=None, device=0):
        """serialize_for_tree: transaction -> the bytes the tree hashes (default:
        the transaction is those bytes).  transactionLog: the committed
        transactions so far (a list; default none).  on_device: passed to the
        tree's extend / append_batch (None: by batch size)."""
        self.tree = tree if tree is not None else CompactMerkleTree()
        self.serialize_for_tree = serialize_for_tree or _bytes_as_they_are
        self.on_device = on_device
        self.device = device
        self._transactionLog = list(transactionLog) if transactionLog is not None else []
        self.seqNo = 0
        self.reset_uncommitted()
        self.recoverTree()

    # ---- recovery
    def recoverTree(self):
        """From the hash store if it has leaves and agrees with the log, else from the log."""
        if self.tree.leafCount == 0:
            self.recoverTreeFromTxnLog()
            return
        try:
            self.recoverTreeFromHashStore()
        except ConsistencyVerificationFailed:
            self.recoverTreeFromTxnLog()

    def recoverTreeFromTxnLog(self):
        """The tree again from the whole log: one extend."""
        self.tree.reset()
        self.seqNo = 0
        if self._transactionLog:
            self.tree.extend([self.serialize_for_tree(t) for t in self._transactionLog], on_device=self.on_device,
                             device=self.device)
        self.seqNo = self.tree.tree_size

    def recoverTreeFromHashStore(self):
        treeSize = self.tree.leafCount
        self.seqNo = treeSize
        hashes = list(reversed(self.tree.inclusion_proof(treeSize, treeSize + 1)))
        self.tree._update(treeSize, hashes)
        self.tree.verify_consistency(len(self._transactionLog))

    # ---- auditing the hash store (row f-9)
    def auditHashStore(self, check_leaves=True):
        """CompactMerkleTree.audit_store over the ledger's store, as a
        merkle.StoreAudit: every stored node against its stored children, the
        counts (against the log's length too), the tree's hashes; with
        check_leaves every stored leaf hash against the log's transaction,
        serialised again.  Nothing is changed."""
        leaves = [self.serialize_for_tree(t) for t in self._transactionLog] if check_leaves else None
        audit = self.tree.audit_store(leaves, on_device=self.on_device, device=self.device)
        audit.counts_ok = audit.counts_ok and self.tree.leafCount == len(self._transactionLog)
        return audit

    def recoverTreeVerified(self):
        """recoverTree that does not trust the store (ledger/ledger.py:70-114
        trusts one that has leaves): "store" when the tree is recovered from
        the hash store and the audit, leaves included, passes; "rebuilt" when
        the stored leaf hashes are the log's and only nodes or counts are
        wrong: the node store is recomputed from the leaf hashes
        (CompactMerkleTree.rebuild_nodes), the log is not hashed again; else
        "log": recoverTreeFromTxnLog."""
        try:
            self.recoverTreeFromHashStore()
            recovered = True
        except (ConsistencyVerificationFailed, IndexError):
            recovered = False
        audit = self.auditHashStore(check_leaves=True)
        if recovered and audit.ok:
            return "store"
        n = len(self._transactionLog)
        if self.tree.leafCount == n and audit.leaves_checked == n and not audit.bad_leaves:
            self.tree.rebuild_nodes(on_device=self.on_device, device=self.device)
            self.seqNo = self.tree.tree_size
            return "rebuilt"
        self.recoverTreeFromTxnLog()
        return "log"

    # ---- committed transactions
    def add(self, txn):
        """One transaction into the log and the tree; its seqNo, the root hash
        after it and its audit path."""
        audit_path = self.tree.append(self.serialize_for_tree(txn))
        self._transactionLog.append(copy(txn))  # the caller goes on to update its own object
        self.seqNo += 1
        return {"seqNo": self.seqNo,
                "rootHash": self.hashToStr(self.tree.root_hash),
                "auditPath": [self.hashToStr(h) for h in audit_path]}

    def append(self, txn):
        return self.add(txn)

    def getBySeqNo(self, seqNo):
        seqNo = int(seqNo)
        return self._transactionLog[seqNo - 1] if 0 < seqNo <= len(self._transactionLog) else None

    def __getitem__(self, seqNo):
        return self.getBySeqNo(seqNo)

    def getAllTxn(self, frm=None, to=None):
        lo = 1 if frm is None else max(1, int(frm))
        hi = len(self._transactionLog) if to is None else min(int(to), len(self._transactionLog))
        for seqNo in range(lo, hi + 1):
            yield seqNo, self._transactionLog[seqNo - 1]

    @property
    def size(self):
        return self.tree.tree_size

    def __len__(self):
        return self.size

    @property
    def root_hash(self):
        return self.hashToStr(self.tree.root_hash)

    def merkleInfo(self, seqNo):
        seqNo = int(seqNo)
        if seqNo <= 0:
            raise ValueError("seqNo must be > 0, got %r" % (seqNo,))
        return {"rootHash": self.hashToStr(self.tree.merkle_tree_hash(0, seqNo)),
                "auditPath": [self.hashToStr(h) for h in self.tree.inclusion_proof(seqNo - 1, seqNo)]}

    # ---- reads, a batch at a time (row f-8)
    def merkle_proofs(self, seqNos, on_device=None):
        """The raw ProofBatch behind merkleInfoBatch: audit paths, tree heads
        and leaf hashes as packed arrays, no base58.  on_device None: the
        ledger's own setting, then the tree's routing (the device with a
        merkle.DeviceHashStore, from merkle.MIN_DEVICE_PROVE_PROOFS proofs on)."""
        return self.tree.merkle_info_batch(seqNos, on_device=self.on_device if on_device is None else on_device,
                                           device=self.device)

    def merkleInfoBatch(self, seqNos, on_device=None):
        """[self.merkleInfo(s) for s in seqNos], from one batched proof call
        (plenum/server/node.py:3024-3034 asks once per reply)."""
        batch = self.merkle_proofs(seqNos, on_device)
        return [{"rootHash": self.hashToStr(batch.roots[i].tobytes()),
                 "auditPath": [self.hashToStr(h) for h in path]} for i, path in enumerate(batch)]

    def consistency_proofs(self, pairs, on_device=None):
        """Per (first, second): the consistency proof and both root hashes, as
        catch-up computes them one pair at a time
        (plenum/common/ledger_manager.py:995-998): a list of dicts with
        `proof` (base58 strings), `oldRootHash` and `newRootHash`."""
        batch = self.tree.consistency_proof_batch(pairs, on_device=self.on_device if on_device is None else on_device,
                                                  device=self.device)
        return [{"proof": [self.hashToStr(h) for h in proof],
                 "oldRootHash": self.hashToStr(batch.old_roots[i].tobytes()),
                 "newRootHash": self.hashToStr(batch.new_roots[i].tobytes())} for i, proof in enumerate(batch)]

    def reset(self):
        """Destructive: the log and the hash store are emptied (the tree
        object keeps its size and hashes until it is recovered, as in the
        reference)."""
        self._transactionLog = []
        self.tree.hashStore.reset()

    # ---- uncommitted transactions
    @property
    def uncommitted_size(self):
        return self.size + len(self.uncommittedTxns)

    def appendTxns(self, txns):
        """Applied, not committed: only uncommittedTree and uncommittedRootHash move."""
        txns = list(txns)
        uncommittedSize = self.size + len(self.uncommittedTxns)
        self.uncommittedTree = self.treeWithAppliedTxns(txns, self.uncommittedTree)
        self.uncommittedRootHash = self.uncommittedTree.root_hash
        self.uncommittedTxns.extend(txns)
        if txns:
            return (uncommittedSize + 1, uncommittedSize + len(txns)), txns
        return (uncommittedSize, uncommittedSize), txns

    def commitTxns(self, count):
        """Commit the first `count` uncommitted transactions: one append_batch,
        then every committed transaction is updated with its own rootHash and
        auditPath (a transaction without `update`, such as bytes, is left as it
        is).  Returns ((first seqNo, last seqNo), committed transactions)."""
        committedSize = self.size
        committedTxns = self.uncommittedTxns[:count]
        if committedTxns:
            logged = [copy(t) for t in committedTxns]  # as hashed: before the update
            batch = self.tree.append_batch([self.serialize_for_tree(t) for t in committedTxns],
                                           on_device=self.on_device, device=self.device)
            for txn, (root, audit_path) in zip(committedTxns, batch):
                if hasattr(txn, "update"):
                    txn.update({"rootHash": self.hashToStr(root),
                                "auditPath": [self.hashToStr(h) for h in audit_path]})
            self._transactionLog.extend(logged)
            self.seqNo += len(committedTxns)
        self.uncommittedTxns = self.uncommittedTxns[count:]
        if not self.uncommittedTxns:
            self.uncommittedTree = None
            self.uncommittedRootHash = None
        if committedTxns:
            return (committedSize + 1, committedSize + count), committedTxns
        return (committedSize, committedSize), committedTxns

    def discardTxns(self, count):
        """Drop the last `count` uncommitted transactions."""
        if count == 0:
            return
        self.uncommittedTxns = self.uncommittedTxns[:-count]
        if not self.uncommittedTxns:
            self.uncommittedTree = None
            self.uncommittedRootHash = None
        else:
            self.uncommittedTree = self.treeWithAppliedTxns(self.uncommittedTxns)
            self.uncommittedRootHash = self.uncommittedTree.root_hash

    def treeWithAppliedTxns(self, txns, currentTree=None):
        """A copy of the tree (the committed one unless given) with txns applied."""
        currentTree = currentTree if currentTree is not None else self.tree
        tempTree = copy(currentTree)
        tempTree.extend([self.serialize_for_tree(t) for t in txns], on_device=self.on_device, device=self.device)
        return tempTree

    def verify_catchup_txns(self, txns, final_size, final_root_hash, proof):
        """Do `txns`, applied to the committed tree, lead to a tree consistent
        with the one of final_size leaves and final_root_hash (the check of
        plenum/common/ledger_manager.py:564-609)?  The temporary tree is one
        extend (on the device by batch size); the consistency proof is a
        single one, so it is walked on the host.  final_root_hash and the
        proof's entries are base58 strings or bytes.  Any exception means
        False, as in the reference."""
        try:
            tempTree = self.treeWithAppliedTxns(txns)
            return bool(MerkleVerifier().verify_tree_consistency(
                tempTree.tree_size, int(final_size), tempTree.root_hash, _as_hash(final_root_hash),
                [_as_hash(p) for p in proof]))
        except Exception:
            return False

    def applyCatchupReplies(self, replies, final_size, final_root_hash):
        """Verify and commit in-order catch-up replies in one pass (row f-10;
        plenum/common/ledger_manager.py:505-609 checks one reply at a time with
        a temporary tree and then adds its transactions one by one, hashing
        each twice).  replies: a list of (txns, proof), the transactions in
        seqNo order from size + 1 on, each reply's consistency proof leading
        from the tree at its end to the one of final_size leaves and
        final_root_hash; hashes are base58 strings or bytes, as in
        verify_catchup_txns.  One CompactMerkleTree.extend_verified call
        (edv_merkle_catchup from merkle.MIN_DEVICE_CATCHUP_LEAVES transactions
        on): every transaction is hashed once.  The log, seqNo and the tree
        advance by the leading replies that verify, as the reference's loop
        accepts them; returns the merkle.CatchupResult."""
        replies = [(list(txns), [_as_hash(p) for p in proof]) for txns, proof in replies]
        result = self.tree.extend_verified([[self.serialize_for_tree(t) for t in txns] for txns, _ in replies],
                                           int(final_size), _as_hash(final_root_hash), [p for _, p in replies],
                                           on_device=self.on_device, device=self.device)
        for txns, _ in replies[:result.accepted]:
            self._transactionLog.extend(copy(t) for t in txns)
        self.seqNo += result.accepted_leaves
        return result

    def reset_uncommitted(self):
        self.uncommittedTxns = []
        self.uncommittedRootHash = None
        self.uncommittedTree = None

    @staticmethod
    def hashToStr(h):
        return base58.b58encode(h).decode("utf-8")

    @staticmethod
    def strToHash(s):
        return base58.b58decode(s)
