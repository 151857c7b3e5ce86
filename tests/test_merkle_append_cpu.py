"""The batched append without a GPU (row f-6): the kernel's header code on the
CPU (hc_merkle_path_entries, hc_merkle_append_batch) against Python integers
and the sequential checker of tests/merkle_append_cases.py, and the Python
tree's host route and the Ledger against the reference's recorded appends."""
import itertools
import json

import pytest

import merkle_append_cases as ac
import merkle_cases as mc
from indy_plenum_amd import Ledger, merkle
from indy_plenum_amd import ledger as ledger_mod


# ---- index arithmetic
def test_path_entries_against_python_integers():
    pe = ac.hostcheck().hc_merkle_path_entries
    for old in list(range(0, 70)) + [255, 256, 257, 1023, 65535, 65536]:
        for n in (0, 1, 2, 3, 63, 64, 65, 300):
            assert pe(old, n) == ac.path_entries(old, n) == ac.path_entries_closed(old, n)
    for old in ac.HUGE:
        for n in (0, 1, 2, 257, 599, 600):
            assert pe(old, n) == ac.path_entries(old, n)
        # a maximal call: the closed form in exact integers (P(2^62) itself is above 2^64)
        n = min(2 ** 22, 2 ** 62 - old)
        assert pe(old, n) == ac.path_entries_closed(old, n) < 2 ** 22 * 62
    assert ac.path_entries_closed(0, 2 ** 62) > 2 ** 64


def test_python_prefix_is_the_same_sum():
    for x in list(range(0, 130)) + [2 ** 32 - 1, 2 ** 40 + 2 ** 20 + 5]:
        assert merkle.popcount_prefix(x) == ac.path_entries_closed(0, x)
    assert merkle.popcount_prefix(77) == sum(mc.popcount(t) for t in range(77))


# ---- the kernel's code on the CPU
@pytest.mark.parametrize("old,n", ac.cpu_grid())
def test_hostcheck_over_the_grid(old, n):
    fr, leaves, want, app = ac.case(old, n)
    got = ac.hc_append(old, fr, leaves)
    assert got == ac.expected(want, app)
    if n:
        assert got[4][-32:] == got[3]          # roots[n - 1] == root


@pytest.mark.parametrize("old,n", [(255, 513), (0, 65), (2 ** 32 - 1, 257)])
def test_hostcheck_every_combination_of_outputs(old, n):
    fr, leaves, want, app = ac.case(old, n)
    for combo in itertools.product((True, False), repeat=4):
        assert ac.hc_append(old, fr, leaves, *combo) == ac.expected(want, app, *combo)


def test_hostcheck_multi_pass():
    """More than one tile of tiles: entries that are tile roots of tile roots."""
    old, n = 255, 70000
    fr = mc.frontier(7, old)
    leaves = mc.leaves_of(3, n, max_len=16)
    want, app = mc.simulate(old, fr, leaves), ac.simulate_appends(old, fr, leaves)
    assert ac.hc_append(old, fr, leaves, want_leaf=False, want_node=False) == ac.expected(want, app, True, True,
                                                                                          False, False)


# ---- the Python tree's host route
@pytest.fixture(scope="module")
def golden():
    return ac.load_golden()


def _tree_batch(leaves, **kw):
    t = merkle.CompactMerkleTree()
    return t, t.append_batch(leaves, **kw)


def check_batch_against_golden(batch, g, first=0):
    """An AppendBatch covering leaves first + 1 .. of the golden sequence."""
    rec = g["all"] if first == 0 else g["after"]
    pairs = list(batch)
    assert ac.digest([r for r, _ in pairs], [p for _, p in pairs]) == (rec["roots_sha256"], rec["paths_sha256"],
                                                                      rec["entries"])
    assert batch.roots.shape == (len(pairs), 32) and batch.paths.shape == (rec["entries"], 32)
    for f in g["full"]:
        i = f["leaf"] - 1 - first
        if i < 0:
            continue
        assert batch.root(i).hex() == f["root"] and bytes(batch.roots[i]).hex() == f["root"]
        assert [h.hex() for h in batch.path(i)] == f["path"]
        assert pairs[i] == (bytes.fromhex(f["root"]), [bytes.fromhex(h) for h in f["path"]])


def test_python_host_route_against_golden(golden):
    leaves = golden["leaves"]
    t, batch = _tree_batch(leaves, on_device=False)
    check_batch_against_golden(batch, golden)
    case = [c for c in mc.load_golden()["cases"] if c["size"] == 1000][0]
    mc.check_tree_against_golden(t, case, leaves)          # tree and hash store as n appends leave them
    # the 300 appends after a 700-leaf tree, the first 700 by single appends
    t = merkle.CompactMerkleTree()
    for leaf in leaves[:700]:
        t.append(leaf)
    check_batch_against_golden(t.append_batch(leaves[700:], on_device=False), golden, first=700)
    mc.check_tree_against_golden(t, case, leaves)
    # in calls of 300: the packed layout runs on across calls
    t, batch = _tree_batch(leaves, on_device=False, max_call=300)
    check_batch_against_golden(batch, golden)
    mc.check_tree_against_golden(t, case, leaves)


def test_python_host_route_equals_appends_one_by_one(golden):
    leaves = golden["leaves"][:130]
    a, b = merkle.CompactMerkleTree(), merkle.CompactMerkleTree()
    want = []
    for leaf in leaves:
        path = a.append(leaf)
        want.append((a.root_hash, path))
    batch = b.append_batch(leaves, on_device=False)
    assert list(batch) == want and len(batch) == 130
    assert b.hashes == a.hashes and b.root_hash == a.root_hash
    assert bytes(b.hashStore._leafs) == bytes(a.hashStore._leafs)
    assert bytes(b.hashStore._nodes) == bytes(a.hashStore._nodes)
    empty = b.append_batch([], on_device=False)
    assert len(empty) == 0 and list(empty) == [] and b.tree_size == 130
    with pytest.raises(IndexError):
        batch.path(130)


def test_small_batches_stay_on_the_host_by_default(golden, monkeypatch):
    """Below MIN_DEVICE_APPEND_LEAVES the automatic choice never touches the library."""
    def no_device(*a, **k):
        raise AssertionError("device route taken")
    monkeypatch.setattr(merkle.edv, "merkle_append_batch", no_device)
    n = merkle.MIN_DEVICE_APPEND_LEAVES - 1
    _, batch = _tree_batch(golden["leaves"][:n])
    assert len(batch) == n


# ---- the Ledger
def _txns(leaves):
    return [{"payload": leaf} for leaf in leaves]


def _ledger(**kw):
    return Ledger(serialize_for_tree=lambda txn: txn["payload"], on_device=False, **kw)


def test_ledger_add_against_golden(golden):
    L = Ledger(on_device=False)                # the default: transactions that are already bytes
    roots, paths = [], []
    for i, leaf in enumerate(golden["leaves"]):
        info = L.add(leaf) if i % 2 else L.append(leaf)
        assert info["seqNo"] == i + 1 == L.seqNo == L.size
        roots.append(Ledger.strToHash(info["rootHash"]))
        paths.append([Ledger.strToHash(h) for h in info["auditPath"]])
        assert isinstance(info["rootHash"], str)
    rec = golden["all"]
    assert ac.digest(roots, paths) == (rec["roots_sha256"], rec["paths_sha256"], rec["entries"])
    assert L.root_hash == Ledger.hashToStr(roots[-1]) and len(L) == 1000
    assert L.getBySeqNo(3) == golden["leaves"][2] and L[1000] == golden["leaves"][999] and L[1001] is None


def test_ledger_commit_against_golden(golden):
    L = _ledger()
    txns = _txns(golden["leaves"])
    assert L.appendTxns(txns[:700]) == ((1, 700), txns[:700])
    assert L.commitTxns(700) == ((1, 700), txns[:700])
    assert L.appendTxns(txns[700:]) == ((701, 1000), txns[700:])
    assert L.commitTxns(300) == ((701, 1000), txns[700:])
    for rec, part in ((golden["all"], txns), (golden["after"], txns[700:])):
        roots = [Ledger.strToHash(t["rootHash"]) for t in part]
        paths = [[Ledger.strToHash(h) for h in t["auditPath"]] for t in part]
        assert ac.digest(roots, paths) == (rec["roots_sha256"], rec["paths_sha256"], rec["entries"])
    for f in golden["full"]:
        t = txns[f["leaf"] - 1]
        assert Ledger.strToHash(t["rootHash"]).hex() == f["root"]
        assert [Ledger.strToHash(h).hex() for h in t["auditPath"]] == f["path"]
        assert set(t) == {"payload", "rootHash", "auditPath"}


def test_ledger_commit_equals_an_add_loop(golden):
    leaves = golden["leaves"][:90]
    ref = _ledger()
    infos = [ref.add(t) for t in _txns(leaves)]
    L = _ledger()
    txns = _txns(leaves)
    assert L.uncommittedRootHash is None and L.uncommittedTree is None
    # nothing to commit
    assert L.commitTxns(0) == ((0, 0), []) and L.appendTxns([]) == ((0, 0), []) and L.size == 0
    assert L.appendTxns(txns[:40]) == ((1, 40), txns[:40])
    assert L.appendTxns(txns[40:70]) == ((41, 70), txns[40:70])
    assert L.size == 0 and L.uncommitted_size == 70 and L.seqNo == 0
    assert L.uncommittedRootHash == L.uncommittedTree.root_hash == Ledger.strToHash(infos[69]["rootHash"])
    # a partial commit: 25 of 70, the rest stays applied
    assert L.commitTxns(25) == ((1, 25), txns[:25])
    assert L.size == 25 == L.seqNo and L.root_hash == infos[24]["rootHash"]
    assert len(L.uncommittedTxns) == 45 and L.uncommittedTxns[0] is txns[25]
    assert L.uncommittedRootHash == Ledger.strToHash(infos[69]["rootHash"])
    assert L.commitTxns(0) == ((25, 25), []) and L.size == 25
    # discard the last 30 uncommitted: the uncommitted tree is rebuilt over the 15 left
    L.discardTxns(0)
    assert len(L.uncommittedTxns) == 45
    L.discardTxns(30)
    assert len(L.uncommittedTxns) == 15 and L.uncommitted_size == 40
    assert L.uncommittedRootHash == Ledger.strToHash(infos[39]["rootHash"])
    assert L.uncommittedTree.tree_size == 40
    assert L.appendTxns(txns[40:]) == ((41, 90), txns[40:])
    assert L.commitTxns(65) == ((26, 90), txns[25:])
    assert L.uncommittedTxns == [] and L.uncommittedTree is None and L.uncommittedRootHash is None
    for txn, info in zip(txns, infos):
        assert txn["rootHash"] == info["rootHash"] and txn["auditPath"] == info["auditPath"]
    assert L.size == 90 == L.seqNo and L.root_hash == ref.root_hash and L.tree.hashes == ref.tree.hashes
    assert bytes(L.tree.hashStore._nodes) == bytes(ref.tree.hashStore._nodes)
    logged = _txns(leaves)                 # the log holds the transactions as they were hashed
    assert [t for _, t in L.getAllTxn()] == logged and list(L.getAllTxn(89, 90)) == [(89, logged[88]), (90, logged[89])]
    # discarding everything that is uncommitted
    L.appendTxns(_txns(golden["leaves"][90:95]))
    L.discardTxns(5)
    assert L.uncommittedTxns == [] and L.uncommittedTree is None and L.uncommittedRootHash is None and L.size == 90
    # treeWithAppliedTxns leaves the committed tree alone
    t = L.treeWithAppliedTxns(_txns(golden["leaves"][90:100]))
    assert t.tree_size == 100 and L.size == 90 and t is not L.tree


def test_ledger_log_holds_transactions_as_hashed(golden):
    """A serializer that reads the whole transaction: the Merkle info a
    committed transaction is updated with must not reach the log, or recovery
    hashes other bytes than the commit did."""
    def whole(txn):
        return json.dumps(txn, sort_keys=True).encode()

    def fresh():
        return [{"k": i, "data": leaf.hex()} for i, leaf in enumerate(golden["leaves"][:40])]
    want = merkle.TreeHasher().hash_full_tree([whole(t) for t in fresh()])
    L = Ledger(serialize_for_tree=whole, on_device=False)
    txns = fresh()
    L.appendTxns(txns[:30])
    assert L.commitTxns(30) == ((1, 30), txns[:30])
    for t in txns[30:]:                    # and the per-transaction route, the caller updating its own object
        t.update(L.add(t))
    assert all("rootHash" in t and "auditPath" in t for t in txns)
    root = L.root_hash
    assert Ledger.strToHash(root) == want and txns[29]["rootHash"] == L.merkleInfo(30)["rootHash"]
    assert [L.getBySeqNo(i + 1) for i in range(40)] == fresh() == [t for _, t in L.getAllTxn()]
    L.recoverTreeFromTxnLog()
    assert (L.size, L.seqNo, L.root_hash) == (40, 40, root)
    again = Ledger(serialize_for_tree=whole, transactionLog=[L.getBySeqNo(i + 1) for i in range(40)],
                   on_device=False)
    assert (again.size, again.root_hash, again.tree.hashes) == (40, root, L.tree.hashes)


def test_ledger_merkle_info_agrees_with_add(golden):
    L = _ledger()
    infos = [L.add(t) for t in _txns(golden["leaves"][:70])]
    for i, info in enumerate(infos):
        assert L.merkleInfo(i + 1) == {"rootHash": info["rootHash"], "auditPath": info["auditPath"]}
        assert L.merkleInfo(str(i + 1)) == L.merkleInfo(i + 1)
        assert mc.verify_inclusion(mc.leaf_hash(golden["leaves"][i]), i, i + 1,
                                   [Ledger.strToHash(h) for h in info["auditPath"]],
                                   Ledger.strToHash(info["rootHash"]))
    with pytest.raises(ValueError):
        L.merkleInfo(0)


def test_ledger_recovery_and_reset(golden):
    leaves = golden["leaves"][:300]
    L = Ledger(on_device=False)
    L.appendTxns(leaves)
    L.commitTxns(300)                      # bytes have no `update`: committed as they are
    want_root, want_hashes = L.root_hash, L.tree.hashes
    # from the hash store: the tree object forgets, the store remembers
    L.tree._update(0, ())
    L.recoverTreeFromHashStore()
    assert (L.size, L.seqNo, L.root_hash, L.tree.hashes) == (300, 300, want_root, want_hashes)
    # from the transaction log: the whole log again through extend
    L.recoverTreeFromTxnLog()
    assert (L.size, L.seqNo, L.root_hash, L.tree.hashes) == (300, 300, want_root, want_hashes)
    assert L.tree.leafCount == 300 and L.tree.verify_consistency(300)
    # a new ledger over the same tree and log picks the hash store; over a log that disagrees, the log
    assert Ledger(tree=L.tree, transactionLog=leaves, on_device=False).root_hash == want_root
    shorter = Ledger(tree=L.tree, transactionLog=leaves[:200], on_device=False)
    assert shorter.size == 200 and shorter.root_hash == Ledger.hashToStr(merkle.TreeHasher().hash_full_tree(leaves[:200]))
    L.reset()
    assert L.tree.leafCount == 0 and list(L.getAllTxn()) == []
    L.recoverTreeFromTxnLog()
    assert L.size == 0 and L.seqNo == 0
    assert ledger_mod.Ledger is Ledger
