#!/usr/bin/env python3
"""Times the Merkle-tree extension (row f-5) on the GPU and writes one JSON file
(default profiles/r07/merkle_bench.json).

For 65,536 leaves of 256 bytes, from old = 0 and from old = 2^20 + 12,345
(arbitrary frontier bytes):
  a  edv_merkle_extend_dev            device-resident, all outputs
  b  edv_sha256_batch_dev             the same leaves (the leaf stage's compressions, no tree)
  c  edv_sha256_batch_dev             65,536 messages of 65 bytes (the node stage's compressions,
                                      without the level dependencies)
  d  edv_merkle_extend                the host-buffer call (staging and copies included)
  e  CompactMerkleTree.extend(on_device=False)   the host loop
and (d) against (e) at n = 64 ... 16,384, whose smallest n with d < e is
MIN_DEVICE_LEAVES (indy_plenum_amd/merkle.py).

With --leg append: the batched append (row f-6) instead, written to
profiles/r08/merkle_append_bench.json.  For 100, 256, 1,000, 10,000 and 65,536
leaves of 256 bytes, from old = 0 and from old = 2^20 + 12,345:
  a  edv_merkle_append_batch_dev      device-resident, all outputs
  b  edv_merkle_append_batch          host buffers, roots only (with leaf and node hashes, as the tree asks)
  c  edv_merkle_append_batch          host buffers, roots and audit paths
  d  edv_merkle_extend_dev / edv_merkle_extend   the same leaves without the per-leaf outputs
  e  CompactMerkleTree.append_batch(on_device=False)   the host hashlib loop
with the fold hashes and path entries per leaf and the append kernel's lane
efficiency (mean over the waves of mean / max trip count of the fold, from the
sizes alone).  The smallest size from which (c) beats (e) on both trees is
MIN_DEVICE_APPEND_LEAVES (indy_plenum_amd/merkle.py).

With --leg verify: batched proof verification (row f-7), written to
profiles/r09/merkle_verify_bench.json.  For 64 ... 65,536 proofs, the audit
paths and roots the batched append returns for that many leaves of 256 bytes
onto old = 0 and old = 2^20 + 12,345:
  a  edv_merkle_verify_inclusion_dev  device-resident, on the append's own device outputs: leaf hashes,
                                      and leaf bytes (the lanes hash their leaves)
  b  edv_merkle_verify_inclusion      host buffers, leaf bytes (staging and copies included)
  c  MerkleVerifier.verify_append_batch(on_device=True)    (b) with the Python shim's packing
  e  MerkleVerifier.verify_append_batch(on_device=False)   the host walk in hashlib
with the entries per proof and the lane efficiency of the walk (mean / max
trip count per wave).  The smallest size from which (c) beats (e) on both
trees is MIN_DEVICE_VERIFY_PROOFS.  And 10,000 consistency proofs (m, 4096)
of one real tree, verify_tree_consistency_batch on the device and on the host.

With --leg prove: batched proof generation (row f-8), written to
profiles/r10/merkle_prove_bench.json.  Two trees of 8-byte leaves in a
DeviceHashStore, 10,000 leaves and 2^20 + 12,345, and three sets of 10,000
pairs on each: merkleInfo (the last 10,000 seqNos: leaf s - 1 in the tree of s
leaves), inclusion (random leaves in the whole tree) and consistency (random
first <= random second):
  a  edv_merkle_prove_*_dev           device-resident, all outputs; HIP events on a stream of the bench's own
  v  edv_merkle_verify_*_dev          row f-7 on the proofs (a) made, device-resident, HIP events
  b  CompactMerkleTree.*_batch(on_device=True)   through the DeviceHashStore, outputs copied back
  c  edv_merkle_prove_*               the host-buffer form (copies the store per call)
  e  CompactMerkleTree.*_batch(on_device=False)  the package's host loop of single calls
with the lane efficiency of the fold (mean over waves of mean / max
popcount - 1), (a) again with the pairs sorted by popcount(tree_size), the
base58 encoding of the 10,000 merkleInfo replies on a line of its own, and
(b) against (e) at 16, 64, 256 and 1,024 merkleInfo proofs, whose smallest size
from which (b) wins on both trees is MIN_DEVICE_PROVE_PROOFS.  The routes of a
case are timed interleaved: every repetition visits each route in turn.

With --leg audit: the hash-store audit and repair (row f-9), written to
profiles/r11/merkle_audit_bench.json.  Two ledgers of 256-byte transactions
over a DeviceHashStore, 10,000 leaves and 2^20 + 12,345:
  a  edv_merkle_audit_nodes_dev / _leaves_dev / edv_merkle_extend_hashed_dev   device-resident (copies of the
     store of the bench's own), HIP events; the extend from hashes hashes as many nodes as the node audit checks,
     with coalesced loads; the leaf audit streams its input: both are the node audit's gathers' yardsticks
  b  CompactMerkleTree.audit_store(on_device=True), with and without the leaves, and rebuild_nodes(on_device=True),
     through the DeviceHashStore
  e  the same three in hashlib (on_device=False)
  r  Ledger.recoverTreeFromTxnLog on the device, the remedy there was before, and recoverTreeVerified on a clean store
and (b) against (e) on stores of 16, 64, 256 and 1,024 nodes, alone and with their leaves, whose smallest size from
which (b) wins both ways is MIN_DEVICE_AUDIT_ENTRIES.

With --leg catchup: catch-up in one call (row f-10), written to
profiles/r12/merkle_catchup_bench.json.  A node at old = 0 and at old = 2^20 +
12,345 receives 64, 256, 1,024 and 10,000 transactions of 256 bytes in replies
of 100, each with its consistency proof to the pool's tree:
  b  Ledger.applyCatchupReplies(on_device=True)    one edv_merkle_catchup call for the pass
  h  Ledger.applyCatchupReplies(on_device=False)   the same pass on the host
  e  per reply Ledger.verify_catchup_txns, then Ledger.add per transaction: the loop there was before
The three are timed interleaved; every call starts from a fresh ledger at the
old tree.  The smallest total from which (b) beats (e) and (h) on both trees
beyond the rows' spread is MIN_DEVICE_CATCHUP_LEAVES.

Every figure is wall clock around calls that end in a device synchronise (the
device forms with stream = NULL synchronise the library stream before they
return), the median of 5 repetitions after a warm-up; a repetition repeats
the call until it has run for at least --window seconds.  No time is a
pass/fail gate.  Results of (a) and (d) are compared with (e) before timing.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from indy_plenum_amd import edv, merkle  # noqa: E402

N_BIG = 65536
LEAF_BYTES = 256
OLDS = (0, (1 << 20) + 12345)
SMALL = (64, 256, 1024, 4096, 16384)


def timed(fn, window, reps=5):
    """Median seconds per call over `reps` repetitions of at least `window` seconds each."""
    fn()  # warm-up: code objects, buffers grown
    t0 = time.perf_counter()
    fn()
    one = max(time.perf_counter() - t0, 1e-6)
    inner = max(1, int(window / one))
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        out.append((time.perf_counter() - t0) / inner)
    return {"median_us": statistics.median(out) * 1e6, "min_us": min(out) * 1e6, "max_us": max(out) * 1e6,
            "calls_per_repetition": inner, "repetitions": reps}


def frontier(rng, size):
    return rng.integers(0, 256, 32 * bin(size).count("1"), dtype=np.uint8)


def dev(a, extra=0):
    b = edv.DeviceBuffer(max(1, a.nbytes) + extra)
    if a.nbytes:
        b.upload(a)
    return b


def host_tree(old, fr, leaves):
    t = merkle.CompactMerkleTree(tree_size=old, hashes=[fr[i:i + 32].tobytes() for i in range(0, len(fr), 32)])
    t.extend(leaves, on_device=False)
    return t


APPEND_SIZES = (100, 256, 1000, 10000, 65536)
PROVE_TREES = (10000, (1 << 20) + 12345)
PROVE_N = 10000
PROVE_SMALL = (16, 64, 256, 1024)


class Hip:
    """HIP events on a stream of the bench's own, from the runtime libedv.so uses."""

    def __init__(self):
        import ctypes
        self.c = ctypes
        for name in ("libamdhip64.so.7", "libamdhip64.so"):
            try:
                self.h = ctypes.CDLL(name)
                break
            except OSError:
                continue
        self.stream = ctypes.c_void_p()
        assert self.h.hipStreamCreate(ctypes.byref(self.stream)) == 0
        self.e0, self.e1 = ctypes.c_void_p(), ctypes.c_void_p()
        assert self.h.hipEventCreate(ctypes.byref(self.e0)) == 0 and self.h.hipEventCreate(ctypes.byref(self.e1)) == 0

    def timed(self, launch, inner):
        """Seconds per launch: `inner` launches on the stream between two events."""
        assert self.h.hipEventRecord(self.e0, self.stream) == 0
        for _ in range(inner):
            launch(self.stream.value)
        assert self.h.hipEventRecord(self.e1, self.stream) == 0
        assert self.h.hipEventSynchronize(self.e1) == 0
        ms = self.c.c_float()
        assert self.h.hipEventElapsedTime(self.c.byref(ms), self.e0, self.e1) == 0
        return ms.value * 1e-3 / inner


def timed_interleaved(routes, window, reps=5, hip=None):
    """routes: name -> fn() (wall clock) or fn(stream) (HIP events, names starting with "a_" or "v_").
    Every repetition visits each route in turn; the median over the repetitions per route."""
    inner, out = {}, {k: [] for k in routes}

    def once(name, k):
        fn = routes[name]
        if name[:2] in ("a_", "v_"):
            return hip.timed(fn, k)
        t0 = time.perf_counter()
        for _ in range(k):
            fn()
        return (time.perf_counter() - t0) / k
    for name in routes:
        once(name, 1)   # warm-up
        inner[name] = max(1, min(2000, int(window / max(once(name, 1), 1e-6))))
    for _ in range(reps):
        for name in routes:
            out[name].append(once(name, inner[name]))
    return {k: {"median_us": statistics.median(v) * 1e6, "min_us": min(v) * 1e6, "max_us": max(v) * 1e6,
                "calls_per_repetition": inner[k], "repetitions": reps} for k, v in out.items()}


def fold_efficiency(counts, lanes=64):
    """Mean over waves of mean / max of the lanes' node hashes."""
    c = np.asarray(counts, dtype=np.float64)
    eff = [w.mean() / w.max() if w.max() else 1.0 for w in (c[lo:lo + lanes] for lo in range(0, len(c), lanes))]
    return float(np.mean(eff))


def prove_leg(args, rng):
    """Batched proof generation against the host loop (module docstring)."""
    from indy_plenum_amd.ledger import Ledger
    hip = Hip()
    res = {"window_s": args.window, "version": edv.version(), "proofs": PROVE_N, "rows": [], "crossover": []}
    pc = lambda x: bin(int(x)).count("1")  # noqa: E731
    v = merkle.MerkleVerifier()
    for size in PROVE_TREES:
        blob = np.arange(size, dtype=np.uint64).view(np.uint8).tobytes()
        tree = merkle.CompactMerkleTree(hashStore=merkle.DeviceHashStore(args.device))
        tree.extend([blob[8 * i:8 * i + 8] for i in range(size)], on_device=True, device=args.device)
        store = tree.hashStore
        d_leafs, d_nodes, leaves, _ = store.device_arrays()
        leafs_h, nodes_h = np.frombuffer(bytes(store._leafs), np.uint8), np.frombuffer(bytes(store._nodes), np.uint8)
        seqs = np.arange(size - PROVE_N + 1, size + 1, dtype=np.uint64)
        sec = rng.integers(1, size + 1, PROVE_N).astype(np.uint64)
        cases = {"merkle_info": (False, seqs - np.uint64(1), seqs),
                 "inclusion": (False, rng.integers(0, size, PROVE_N).astype(np.uint64), np.full(PROVE_N, size, np.uint64)),
                 "consistency": (True, (rng.integers(0, 2 ** 62, PROVE_N).astype(np.uint64) % sec) + np.uint64(1), sec)}
        for name, (cons, a, b) in cases.items():
            n = len(a)
            pairs = list(zip(a.tolist(), b.tolist()))
            hashes = [pc(y) - 1 + (pc(x) - 1 if cons else 0) for x, y in pairs]

            def device_call(a, b):
                off = (edv.merkle_consistency_offsets if cons else edv.merkle_inclusion_offsets)(a, b, leaves)
                bufs = dict(a=dev(a), b=dev(b), off=dev(off), proofs=edv.DeviceBuffer(32 * max(1, int(off[-1]))),
                            st=edv.DeviceBuffer(n), o1=edv.DeviceBuffer(32 * n), o2=edv.DeviceBuffer(32 * n),
                            vst=edv.DeviceBuffer(n))
                fn = edv.merkle_prove_consistency_device if cons else edv.merkle_prove_inclusion_device

                def prove(stream):
                    fn(d_leafs, d_nodes, leaves, bufs["a"].ptr, bufs["b"].ptr, bufs["off"].ptr, n, bufs["proofs"].ptr,
                       bufs["st"].ptr, bufs["o1"].ptr, bufs["o2"].ptr, device=args.device, stream=stream)

                def verify(stream):
                    if cons:
                        edv.merkle_verify_consistency_device(bufs["a"].ptr, bufs["b"].ptr, bufs["o1"].ptr, bufs["o2"].ptr,
                                                             bufs["proofs"].ptr, bufs["off"].ptr, n, bufs["vst"].ptr,
                                                             device=args.device, stream=stream)
                    else:
                        edv.merkle_verify_inclusion_device(bufs["a"].ptr, bufs["b"].ptr, bufs["o1"].ptr, bufs["proofs"].ptr,
                                                           bufs["off"].ptr, n, bufs["vst"].ptr, d_leaf_hashes=bufs["o2"].ptr,
                                                           device=args.device, stream=stream)
                return bufs, off, prove, verify

            bufs, off, prove, verify = device_call(a, b)
            order = np.argsort([pc(y) for y in b.tolist()], kind="stable")
            sbufs, _, prove_sorted, _ = device_call(a[order], b[order])
            batch = tree.consistency_proof_batch if cons else tree.inclusion_proof_batch

            def route_b():
                return batch(pairs, on_device=True, device=args.device)

            def route_c():
                if cons:
                    return edv.merkle_prove_consistency(leafs_h, nodes_h, leaves, a, b, device=args.device)
                return edv.merkle_prove_inclusion(leafs_h, nodes_h, leaves, a, b, want_leaf_hashes=True, device=args.device)

            def route_e():
                return batch(pairs, on_device=False)

            # results first: every route gives the host loop's bytes, and the verifier accepts them on the device
            want = route_e()
            prove(None)
            verify(None)
            assert (bufs["st"].download() == edv.PROOF_OK).all() and (bufs["vst"].download() == edv.PROOF_OK).all()
            assert bufs["proofs"].download(32 * int(off[-1])).tobytes() == want.proofs.tobytes()
            got_b, got_c = route_b(), route_c()
            assert got_b.proofs.tobytes() == want.proofs.tobytes() == got_c[0].tobytes()
            w1 = want.old_roots if cons else want.roots
            assert bufs["o1"].download().tobytes() == w1.tobytes() == got_c[3].tobytes()
            assert v.verify_proof_batch(got_b, on_device=True, device=args.device).ok.all()
            t = timed_interleaved({"a_prove_dev": prove, "v_verify_dev": verify, "a_prove_dev_sorted_by_popcount": prove_sorted,
                                   "b_device_hash_store": route_b, "c_prove_host_buffers": route_c,
                                   "e_host_loop": route_e}, args.window, hip=hip)
            row = {"tree": size, "case": name, "n": n, "entries_per_proof": int(off[-1]) / n,
                   "node_hashes_per_proof": float(np.mean(hashes)), "lane_efficiency": fold_efficiency(hashes),
                   "lane_efficiency_sorted": fold_efficiency(np.asarray(hashes)[order])}
            row.update(t)
            row["a_over_v"] = t["a_prove_dev"]["median_us"] / t["v_verify_dev"]["median_us"]
            row["e_over_a"] = t["e_host_loop"]["median_us"] / t["a_prove_dev"]["median_us"]
            row["sorted_wins"] = t["a_prove_dev_sorted_by_popcount"]["median_us"] < t["a_prove_dev"]["median_us"]
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
        # (b) against (e) at small sizes: the last k seqNos
        for k in PROVE_SMALL:
            some = list(range(size - k + 1, size + 1))
            t = timed_interleaved({"b_device_hash_store": lambda: tree.merkle_info_batch(some, on_device=True,
                                                                                         device=args.device),
                                   "e_host_loop": lambda: tree.merkle_info_batch(some, on_device=False)}, args.window)
            row = dict(t, tree=size, n=k)
            row["b_beats_e"] = t["b_device_hash_store"]["median_us"] < t["e_host_loop"]["median_us"]
            res["crossover"].append(row)
            print(json.dumps(row), flush=True)
        if size == PROVE_TREES[0]:
            # base58 for the replies, pure Python, on a line of its own: not part of any route above
            info = tree.merkle_info_batch(seqs.tolist(), on_device=True, device=args.device)
            t0 = time.perf_counter()
            for i, path in enumerate(info):
                Ledger.hashToStr(info.roots[i].tobytes())
                for h in path:
                    Ledger.hashToStr(h)
            res["base58_merkle_info_10000_replies_us"] = (time.perf_counter() - t0) * 1e6
            print(json.dumps({"base58_us": res["base58_merkle_info_10000_replies_us"]}), flush=True)
        store.reset()
    cross = None
    for k in sorted(PROVE_SMALL, reverse=True):
        if all(r["b_beats_e"] for r in res["crossover"] if r["n"] == k):
            cross = k
        else:
            break
    res["min_device_prove_proofs"] = {"value": cross, "rule": "smallest measured n from which b < e on both trees, "
                                      "at n and every larger n measured; null: at none"}
    return res


AUDIT_SMALL = (16, 64, 256, 1024)


def audit_leg(args, rng):
    """The hash-store audit and repair against the hashlib loop and against
    recovery from the log (module docstring)."""
    from indy_plenum_amd.ledger import Ledger
    hip = Hip()
    res = {"window_s": args.window, "version": edv.version(), "leaf_bytes": LEAF_BYTES, "rows": [], "crossover": []}
    empty = np.array([0, edv.AUDIT_NONE], dtype=np.uint64)

    def build(size):
        blob = rng.integers(0, 256, size * LEAF_BYTES + 8, dtype=np.uint8)
        raw = blob.tobytes()
        leaves = [raw[i * LEAF_BYTES:(i + 1) * LEAF_BYTES] for i in range(size)]
        led = Ledger(tree=merkle.CompactMerkleTree(hashStore=merkle.DeviceHashStore(args.device)), on_device=True,
                     device=args.device)
        led._transactionLog = leaves
        led.recoverTreeFromTxnLog()
        return blob, leaves, led

    for size in PROVE_TREES:
        blob, leaves, led = build(size)
        tree, store = led.tree, led.tree.hashStore
        nleaves, nnodes = store.leafCount, store.nodeCount
        good_nodes = bytes(store._nodes)
        # the device-resident routes read copies of their own: recovery from the log resets the store and its mirror
        own = (dev(np.frombuffer(bytes(store._leafs), np.uint8)), dev(np.frombuffer(good_nodes, np.uint8)))
        d_leafs, d_nodes = own[0].ptr, own[1].ptr
        d_blob = dev(blob)
        d_off = dev(np.arange(size + 1, dtype=np.uint64) * np.uint64(LEAF_BYTES))
        d_status, d_summary = edv.DeviceBuffer(max(size, 1)), dev(empty)
        d_out = edv.DeviceBuffer(32 * (nnodes + 130))
        slices = [(lo, min(edv.MERKLE_MAX_LEAVES, nnodes - lo)) for lo in range(0, nnodes, edv.MERKLE_MAX_LEAVES)]

        def audit_nodes(stream):
            for lo, cnt in slices:
                edv.merkle_audit_nodes_device(d_leafs, d_nodes, nleaves, lo, cnt, d_status.ptr, d_summary.ptr,
                                              device=args.device, stream=stream)

        def audit_leaves(stream):
            edv.merkle_audit_leaves_device(d_leafs, nleaves, 0, d_blob.ptr, d_off.ptr, size, d_status.ptr, d_summary.ptr,
                                           device=args.device, stream=stream)

        def extend_hashed(stream):   # the rebuild, device-resident: as many node hashes as the node audit, loads coalesced
            edv.merkle_extend_hashed_device(0, None, d_leafs, size, d_out.ptr, d_out.ptr + 32 * nnodes,
                                            d_out.ptr + 32 * (nnodes + 64), device=args.device, stream=stream)

        # results first: a clean store is clean by every route, a damaged node is found alike, the rebuild restores it
        audit_nodes(None)
        audit_leaves(None)
        extend_hashed(None)
        assert d_summary.download(16, np.uint64).tolist() == empty.tolist()
        assert d_out.download(32 * nnodes).tobytes() == good_nodes
        want = tree.audit_store(leaves if size == PROVE_TREES[0] else None, on_device=False)
        assert want.ok and tree.audit_store(leaves, on_device=True, device=args.device).ok
        q = nnodes // 2
        store._nodes[32 * q + 3] ^= 4
        store.mark_stale()
        got = tree.audit_store(on_device=True, device=args.device)
        assert got.bad_nodes and q + 1 in got.bad_nodes and len(got.bad_nodes) <= 2
        if size == PROVE_TREES[0]:
            assert got.bad_nodes == tree.audit_store(on_device=False).bad_nodes
        tree.rebuild_nodes(on_device=True, device=args.device)
        assert bytes(store._nodes) == good_nodes and led.recoverTreeVerified() == "store"

        routes = {"a_audit_nodes_dev": audit_nodes, "a_audit_leaves_dev": audit_leaves,
                  "a_extend_hashed_dev": extend_hashed,
                  "b_audit_store_nodes": lambda: tree.audit_store(on_device=True, device=args.device),
                  "b_audit_store_nodes_and_leaves": lambda: tree.audit_store(leaves, on_device=True, device=args.device),
                  "b_rebuild_nodes": lambda: tree.rebuild_nodes(on_device=True, device=args.device),
                  "e_hashlib_nodes": lambda: tree.audit_store(on_device=False),
                  "e_hashlib_nodes_and_leaves": lambda: tree.audit_store(leaves, on_device=False),
                  "e_hashlib_rebuild_nodes": lambda: tree.rebuild_nodes(on_device=False),
                  "r_recover_from_txn_log_device": led.recoverTreeFromTxnLog,
                  "r_recover_tree_verified": led.recoverTreeVerified}
        t = timed_interleaved(routes, args.window, reps=5 if size == PROVE_TREES[0] else 3, hip=hip)
        row = {"tree": size, "nodes": nnodes, "leaves": size}
        row.update(t)
        us = lambda k: t[k]["median_us"]  # noqa: E731
        row["ns_per_node_audit_dev"] = 1e3 * us("a_audit_nodes_dev") / nnodes
        row["ns_per_node_extend_hashed_dev"] = 1e3 * us("a_extend_hashed_dev") / nnodes
        row["audit_over_extend_hashed_dev"] = us("a_audit_nodes_dev") / us("a_extend_hashed_dev")
        # the gathering node audit against the streaming leaf audit, per SHA-256 compression: a node is two blocks,
        # a leaf of LEAF_BYTES with its prefix and padding (LEAF_BYTES + 1 + 9 + 63) // 64
        leaf_blocks = (LEAF_BYTES + 1 + 9 + 63) // 64
        row["ns_per_compression_audit_nodes_dev"] = 1e3 * us("a_audit_nodes_dev") / (2 * nnodes)
        row["ns_per_compression_audit_leaves_dev"] = 1e3 * us("a_audit_leaves_dev") / (leaf_blocks * size)
        row["hashlib_nodes_over_b"] = us("e_hashlib_nodes") / us("b_audit_store_nodes")
        row["hashlib_nodes_and_leaves_over_b"] = us("e_hashlib_nodes_and_leaves") / us("b_audit_store_nodes_and_leaves")
        row["recover_from_log_over_b_rebuild"] = us("r_recover_from_txn_log_device") / us("b_rebuild_nodes")
        row["recover_from_log_over_b_audit_nodes"] = us("r_recover_from_txn_log_device") / us("b_audit_store_nodes")
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
        store.reset()
    # (b) against (e) on small stores: trees of n + 2 leaves have n nodes
    for n in AUDIT_SMALL:
        blob, leaves, led = build(n + 2)
        tree = led.tree
        assert tree.nodeCount == n
        for case, lv in (("nodes", None), ("nodes_and_leaves", leaves)):
            t = timed_interleaved({"b_device_hash_store": lambda: tree.audit_store(lv, on_device=True, device=args.device),
                                   "e_hashlib": lambda: tree.audit_store(lv, on_device=False)}, args.window)
            row = dict(t, nodes=n, case=case, entries=n + (n + 2 if lv else 0))
            row["b_beats_e"] = t["b_device_hash_store"]["median_us"] < t["e_hashlib"]["median_us"]
            res["crossover"].append(row)
            print(json.dumps(row), flush=True)
        tree.hashStore.reset()
    cross = None
    for n in sorted(AUDIT_SMALL, reverse=True):
        if all(r["b_beats_e"] for r in res["crossover"] if r["nodes"] == n):
            cross = n
        else:
            break
    res["min_device_audit_entries"] = {"value": cross, "rule": "smallest measured node count from which b < e on both "
                                       "stores (the node store alone, and the node and leaf stores with 256-byte "
                                       "leaves), at that count and every larger one measured; null: at none"}
    return res


def lane_efficiency(old, n, lanes=64):
    """The fold's trip counts (popcount(s) - 1 node hashes for s = old + i + 1) over the append kernel's
    waves of `lanes` consecutive leaves: (mean over waves of mean / max trips, fold hashes per leaf)."""
    trips = np.array([bin(old + i + 1).count("1") - 1 for i in range(n)], dtype=np.float64)
    eff = []
    for lo in range(0, n, lanes):
        w = trips[lo:lo + lanes]
        eff.append(w.mean() / w.max() if w.max() else 1.0)
    return float(np.mean(eff)), float(trips.mean())


def append_leg(args, rng):
    """The batched append against the extend and the host loop (module docstring)."""
    res = {"leaf_bytes": LEAF_BYTES, "window_s": args.window, "version": edv.version(), "rows": []}
    blob = rng.integers(0, 256, N_BIG * LEAF_BYTES + 8, dtype=np.uint8)
    off = np.arange(N_BIG + 1, dtype=np.uint64) * np.uint64(LEAF_BYTES)
    leaves = [blob[i * LEAF_BYTES:(i + 1) * LEAF_BYTES].tobytes() for i in range(N_BIG)]
    d_blob, d_off = dev(blob), dev(off)
    for old in OLDS:
        fr = frontier(rng, old)
        frl = [fr[i:i + 32].tobytes() for i in range(0, len(fr), 32)]
        d_old = dev(fr) if old else None
        for n in APPEND_SIZES:
            nodes = edv.merkle_node_span(old, n)
            entries = edv.merkle_path_entries(old, n)
            d_lh, d_nh = edv.DeviceBuffer(32 * n), edv.DeviceBuffer(32 * max(1, nodes))
            d_new, d_root = edv.DeviceBuffer(32 * 64), edv.DeviceBuffer(32)
            d_roots, d_paths = edv.DeviceBuffer(32 * n), edv.DeviceBuffer(32 * max(1, entries))
            sub_blob, sub_off, sub_leaves = blob[:n * LEAF_BYTES + 8], off[:n + 1], leaves[:n]
            oldp = d_old.ptr if d_old else None

            def a():
                edv.merkle_append_batch_device(old, oldp, d_blob.ptr, d_off.ptr, n, d_lh.ptr, d_nh.ptr, d_new.ptr,
                                               d_root.ptr, d_roots.ptr, d_paths.ptr, device=args.device)

            def b():
                return edv.merkle_append_batch(old, fr, sub_blob, sub_off, want_audit_paths=False, device=args.device)

            def c():
                return edv.merkle_append_batch(old, fr, sub_blob, sub_off, device=args.device)

            def d_dev():
                edv.merkle_extend_device(old, oldp, d_blob.ptr, d_off.ptr, n, d_lh.ptr, d_nh.ptr, d_new.ptr,
                                         d_root.ptr, device=args.device)

            def d_host():
                return edv.merkle_extend(old, fr, sub_blob, sub_off, device=args.device)

            def e():
                t = merkle.CompactMerkleTree(tree_size=old, hashes=frl)
                return t, t.append_batch(sub_leaves, on_device=False)

            # results first: (a) and (c) equal the host loop
            t, batch = e()
            a()
            lh, nh, new, root, roots, paths = c()
            assert root == t.root_hash == roots[-1].tobytes() and d_root.download().tobytes() == root
            assert roots.tobytes() == batch.roots.tobytes() == d_roots.download().tobytes()
            assert paths.tobytes() == batch.paths.tobytes() == d_paths.download(32 * entries).tobytes()
            assert nh.tobytes() == bytes(t.hashStore._nodes) and lh.tobytes() == bytes(t.hashStore._leafs)
            eff, folds = lane_efficiency(old, n)
            row = {"old": old, "n": n, "path_entries_per_leaf": entries / n, "fold_hashes_per_leaf": folds,
                   "lane_efficiency": eff,
                   "a_append_batch_dev": timed(a, args.window),
                   "b_append_batch_host_buffers_roots": timed(b, args.window),
                   "c_append_batch_host_buffers_roots_paths": timed(c, args.window),
                   "d_extend_dev": timed(d_dev, args.window),
                   "d_extend_host_buffers": timed(d_host, args.window),
                   "e_python_host_loop": timed(e, args.window)}
            row["c_beats_e"] = (row["c_append_batch_host_buffers_roots_paths"]["median_us"]
                                < row["e_python_host_loop"]["median_us"])
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    # the crossover: the smallest size from which the host-buffer call with roots and paths wins on every tree
    cross = None
    for n in sorted(APPEND_SIZES, reverse=True):
        if all(r["c_beats_e"] for r in res["rows"] if r["n"] == n):
            cross = n
        else:
            break
    res["crossover"] = {"min_device_append_leaves": cross,
                        "rule": "smallest measured n from which c < e for every old, at n and every larger n"}
    return res


VERIFY_SIZES = (64, 100, 256, 1000, 10000, 65536)


def verify_leg(args, rng):
    """Batched proof verification against the host walk (module docstring)."""
    res = {"leaf_bytes": LEAF_BYTES, "window_s": args.window, "version": edv.version(), "rows": []}
    blob = rng.integers(0, 256, N_BIG * LEAF_BYTES + 8, dtype=np.uint8)
    off = np.arange(N_BIG + 1, dtype=np.uint64) * np.uint64(LEAF_BYTES)
    leaves = [blob[i * LEAF_BYTES:(i + 1) * LEAF_BYTES].tobytes() for i in range(N_BIG)]
    d_blob, d_off = dev(blob), dev(off)
    v = merkle.MerkleVerifier()
    for old in OLDS:
        fr = frontier(rng, old)
        frl = [fr[i:i + 32].tobytes() for i in range(0, len(fr), 32)]
        d_old = dev(fr) if old else None
        for n in VERIFY_SIZES:
            entries = edv.merkle_path_entries(old, n)
            d_lh, d_new, d_root = edv.DeviceBuffer(32 * n), edv.DeviceBuffer(32 * 64), edv.DeviceBuffer(32)
            d_roots, d_paths = edv.DeviceBuffer(32 * n), edv.DeviceBuffer(32 * max(1, entries))
            # the proofs: what the batched append wrote, on the device and (the host loop's) on the host
            edv.merkle_append_batch_device(old, d_old.ptr if d_old else None, d_blob.ptr, d_off.ptr, n, d_lh.ptr, None,
                                           d_new.ptr, d_root.ptr, d_roots.ptr, d_paths.ptr, device=args.device)
            t = merkle.CompactMerkleTree(tree_size=old, hashes=frl)
            sub_leaves = leaves[:n]
            batch = t.append_batch(sub_leaves, on_device=False)
            poff = np.array([merkle.popcount_prefix(old + i) - merkle.popcount_prefix(old) for i in range(n + 1)],
                            dtype=np.uint64)
            idx = np.arange(old, old + n, dtype=np.uint64)
            size = idx + np.uint64(1)
            d_poff, d_idx, d_size = dev(poff), dev(idx), dev(size)
            d_status = edv.DeviceBuffer(n)
            sub_blob, sub_off = blob[:n * LEAF_BYTES + 8], off[:n + 1]
            roots, paths = np.ascontiguousarray(batch.roots), np.ascontiguousarray(batch.paths)

            def a_hashes():
                edv.merkle_verify_inclusion_device(d_idx.ptr, d_size.ptr, d_roots.ptr, d_paths.ptr, d_poff.ptr, n,
                                                   d_status.ptr, d_leaf_hashes=d_lh.ptr, device=args.device)

            def a_leaves():
                edv.merkle_verify_inclusion_device(d_idx.ptr, d_size.ptr, d_roots.ptr, d_paths.ptr, d_poff.ptr, n,
                                                   d_status.ptr, d_leaves=d_blob.ptr, d_leaf_off=d_off.ptr,
                                                   device=args.device)

            def b():
                return edv.merkle_verify_inclusion(idx, size, roots, paths, poff, leaves=sub_blob, leaf_off=sub_off,
                                                   device=args.device)

            def c():
                return v.verify_append_batch(old, sub_leaves, batch, on_device=True, device=args.device)

            def e():
                return v.verify_append_batch(old, sub_leaves, batch, on_device=False)

            # results first: every route accepts every proof
            for fn in (a_hashes, a_leaves):
                d_status.upload(np.zeros(n, np.uint8))
                fn()
                assert (d_status.download() == edv.PROOF_OK).all()
            assert (b()[0] == edv.PROOF_OK).all() and c().ok.all() and e().ok.all()
            trips = np.array([bin(old + i).count("1") for i in range(n)], dtype=np.float64)
            eff = float(np.mean([w.mean() / w.max() if w.max() else 1.0
                                 for w in (trips[lo:lo + 64] for lo in range(0, n, 64))]))
            row = {"old": old, "n": n, "path_entries_per_proof": entries / n, "lane_efficiency": eff,
                   "a_verify_dev_leaf_hashes": timed(a_hashes, args.window),
                   "a_verify_dev_leaf_bytes": timed(a_leaves, args.window),
                   "b_verify_host_buffers": timed(b, args.window),
                   "c_verify_append_batch_device": timed(c, args.window),
                   "e_verify_append_batch_host_walk": timed(e, args.window)}
            row["c_beats_e"] = (row["c_verify_append_batch_device"]["median_us"]
                                < row["e_verify_append_batch_host_walk"]["median_us"])
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    cross = None
    for n in sorted(VERIFY_SIZES, reverse=True):
        if all(r["c_beats_e"] for r in res["rows"] if r["n"] == n):
            cross = n
        else:
            break
    res["crossover"] = {"min_device_verify_proofs": cross,
                        "rule": "smallest measured n from which c < e for every old, at n and every larger n"}
    # consistency: 10,000 proofs (m, 4096) from one real tree, device-resident and host buffers against the host walk
    t = merkle.CompactMerkleTree()
    t.extend(leaves[:4096], on_device=False)
    ms = [1 + (k * 37) % 4095 for k in range(10000)]
    items = [(m, 4096, t.merkle_tree_hash(0, m), t.root_hash, t.consistency_proof(m, 4096)) for m in ms]
    assert v.verify_tree_consistency_batch(items, on_device=True).ok.all()
    assert v.verify_tree_consistency_batch(items, on_device=False).ok.all()
    res["consistency"] = {"n": len(items), "new_size": 4096,
                          "entries_per_proof": sum(len(it[4]) for it in items) / len(items),
                          "batch_device": timed(lambda: v.verify_tree_consistency_batch(
                              items, on_device=True, device=args.device), args.window),
                          "batch_host_walk": timed(lambda: v.verify_tree_consistency_batch(items, on_device=False),
                                                   args.window)}
    print(json.dumps(res["consistency"]), flush=True)
    return res


CATCHUP_TOTALS = (64, 256, 1024, 10000)
CATCHUP_REPLY = 100


def catchup_leg(args, rng):
    """Catch-up in one call against the loop it replaces (module docstring)."""
    from indy_plenum_amd.ledger import Ledger
    res = {"leaf_bytes": LEAF_BYTES, "reply_txns": CATCHUP_REPLY, "window_s": args.window, "version": edv.version(),
           "min_device_catchup_leaves": merkle.MIN_DEVICE_CATCHUP_LEAVES, "rows": [], "crossover": []}
    top = max(CATCHUP_TOTALS)
    blob = rng.integers(0, 256, top * LEAF_BYTES, dtype=np.uint8).tobytes()
    txns = [blob[i * LEAF_BYTES:(i + 1) * LEAF_BYTES] for i in range(top)]
    for old in OLDS:
        # the tree the node has (its leaves' content does not matter: 8 bytes each) and the pool's, top leaves on
        small = rng.integers(0, 256, 8 * old, dtype=np.uint8).tobytes()
        full = merkle.CompactMerkleTree()
        full.extend([small[8 * i:8 * i + 8] for i in range(old)], on_device=old > 0, device=args.device)
        frontier_old = full.hashes
        full.extend(txns, on_device=True, device=args.device)

        def shell(on_device):
            led = Ledger(on_device=on_device, device=args.device)
            led.tree = merkle.CompactMerkleTree(tree_size=old, hashes=frontier_old)
            led.seqNo = old
            return led
        for total in CATCHUP_TOTALS:
            final = old + total
            root = full.merkle_tree_hash(0, final)
            replies = []
            for lo in range(0, total, CATCHUP_REPLY):
                hi = min(total, lo + CATCHUP_REPLY)
                replies.append((txns[lo:hi], full.consistency_proof(old + hi, final) if old + hi < final else []))

            def one_call(on_device):
                led = shell(on_device)
                r = led.applyCatchupReplies(replies, final, root)
                return led, r.accepted

            def loop():
                led, count = shell(None), 0    # the routing that exists: every temporary tree by its batch size
                for t, proof in replies:
                    if not led.verify_catchup_txns(t, final, root, proof):
                        break
                    for txn in t:
                        led.add(txn)
                    count += 1
                return led, count
            for led, count in (one_call(True), one_call(False), loop()):
                assert count == len(replies) and led.size == final and led.tree.root_hash == root
            t = timed_interleaved({"b_apply_catchup_replies_device": lambda: one_call(True),
                                   "h_apply_catchup_replies_host": lambda: one_call(False),
                                   "e_verify_catchup_txns_and_add_loop": loop}, args.window,
                                  reps=5 if total < 10000 else 3)
            row = dict({"old": old, "txns": total, "replies": len(replies)}, **t)
            res["rows"].append(row)
            print(json.dumps(row), flush=True)
    for total in CATCHUP_TOTALS:
        rows = [r for r in res["rows"] if r["txns"] == total]
        res["crossover"].append({"txns": total, "device_wins_beyond_spread_on_both_trees": all(
            r["b_apply_catchup_replies_device"]["max_us"] < min(r["e_verify_catchup_txns_and_add_loop"]["min_us"],
                                                                r["h_apply_catchup_replies_host"]["min_us"])
            for r in rows)})
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("extend", "append", "verify", "prove", "audit", "catchup"), default="extend")
    ap.add_argument("--out", default=None)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.out is None:
        args.out = {"extend": os.path.join(ROOT, "profiles", "r07", "merkle_bench.json"),
                    "append": os.path.join(ROOT, "profiles", "r08", "merkle_append_bench.json"),
                    "verify": os.path.join(ROOT, "profiles", "r09", "merkle_verify_bench.json"),
                    "prove": os.path.join(ROOT, "profiles", "r10", "merkle_prove_bench.json"),
                    "audit": os.path.join(ROOT, "profiles", "r11", "merkle_audit_bench.json"),
                    "catchup": os.path.join(ROOT, "profiles", "r12", "merkle_catchup_bench.json")}[args.leg]
    if edv.device_count() < 1:
        sys.exit("bench_merkle needs a gfx950 GPU")
    rng = np.random.default_rng(0x6962)
    if args.leg in ("append", "verify", "prove", "audit", "catchup"):
        res = {"append": append_leg, "verify": verify_leg, "prove": prove_leg, "audit": audit_leg,
               "catchup": catchup_leg}[args.leg](args, rng)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
        print("wrote", args.out)
        return
    res = {"leaves": N_BIG, "leaf_bytes": LEAF_BYTES, "window_s": args.window, "version": edv.version(),
           "big": [], "crossover": []}

    blob = rng.integers(0, 256, N_BIG * LEAF_BYTES + 8, dtype=np.uint8)
    off = np.arange(N_BIG + 1, dtype=np.uint64) * np.uint64(LEAF_BYTES)
    leaves = [blob[i * LEAF_BYTES:(i + 1) * LEAF_BYTES].tobytes() for i in range(N_BIG)]
    d_blob, d_off = dev(blob), dev(off)
    m65 = rng.integers(0, 256, N_BIG * 65 + 8, dtype=np.uint8)
    o65 = np.arange(N_BIG + 1, dtype=np.uint64) * np.uint64(65)
    d_m65, d_o65 = dev(m65), dev(o65)
    d_dig = edv.DeviceBuffer(32 * N_BIG)
    for old in OLDS:
        fr = frontier(rng, old)
        nodes = edv.merkle_node_span(old, N_BIG)
        nnew = bin(old + N_BIG).count("1")
        d_old = dev(fr) if old else None
        d_lh, d_nh = edv.DeviceBuffer(32 * N_BIG), edv.DeviceBuffer(32 * max(1, nodes))
        d_new, d_root = edv.DeviceBuffer(32 * 64), edv.DeviceBuffer(32)

        def a():
            edv.merkle_extend_device(old, d_old.ptr if d_old else None, d_blob.ptr, d_off.ptr, N_BIG, d_lh.ptr,
                                     d_nh.ptr, d_new.ptr, d_root.ptr, device=args.device)

        def b():
            edv.sha256_device(d_blob.ptr, d_off.ptr, N_BIG, d_dig.ptr, device=args.device)

        def c():
            edv.sha256_device(d_m65.ptr, d_o65.ptr, N_BIG, d_dig.ptr, device=args.device)

        def d():
            return edv.merkle_extend(old, fr, blob, off, device=args.device)

        def e():
            return host_tree(old, fr, leaves)

        # results first: (a) and (d) equal the host loop
        t = e()
        a()
        lh, nh, new, root = d()
        assert root == t.root_hash and d_root.download().tobytes() == root
        assert [bytes(r) for r in new] == list(t.hashes) and d_new.download(32 * nnew).tobytes() == new.tobytes()
        assert nh.tobytes() == bytes(t.hashStore._nodes) == d_nh.download(32 * nodes).tobytes()
        assert lh.tobytes() == bytes(t.hashStore._leafs) == d_lh.download().tobytes()
        row = {"old": old, "a_merkle_extend_dev": timed(a, args.window), "b_sha256_leaves": timed(b, args.window),
               "c_sha256_65B": timed(c, args.window), "d_merkle_extend_host_buffers": timed(d, args.window),
               "e_python_host_loop": timed(e, args.window, reps=5)}
        row["a_over_b_plus_c"] = row["a_merkle_extend_dev"]["median_us"] / (
            row["b_sha256_leaves"]["median_us"] + row["c_sha256_65B"]["median_us"])
        res["big"].append(row)
        print(json.dumps(row), flush=True)

    for n in SMALL:
        sub_blob = blob[:n * LEAF_BYTES + 8]
        sub_off = off[:n + 1]
        sub_leaves = leaves[:n]
        none = np.zeros(0, np.uint8)
        row = {"n": n, "old": 0,
               "d_merkle_extend_host_buffers": timed(lambda: edv.merkle_extend(0, none, sub_blob, sub_off,
                                                                               device=args.device), args.window),
               "e_python_host_loop": timed(lambda: host_tree(0, none, sub_leaves), args.window)}
        row["d_beats_e"] = row["d_merkle_extend_host_buffers"]["median_us"] < row["e_python_host_loop"]["median_us"]
        res["crossover"].append(row)
        print(json.dumps(row), flush=True)
    wins = [r["n"] for r in res["crossover"] if r["d_beats_e"]]
    res["min_device_leaves"] = min(wins) if wins else None
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
    print("wrote", args.out)


if __name__ == "__main__":
    main()
