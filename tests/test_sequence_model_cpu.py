"""The sequence harness of tests/sequence_cases.py without a GPU: a fake
backend returns every operation's reference result and keeps a plain book of
tickets, pipelined batches and memory, so these tests prove the harness -- the
generator, the model's BUSY / OK expectations, replay, the failure message,
that one wrong byte in any kind of output is caught at its operation -- and the
coverage conditions of every directed list and every random seed
(tests/test_gpu_sequences.py runs the same lists on the device)."""
import time

import numpy as np
import pytest

import sequence_cases as sc

MiB = 1 << 20
COMPACT_BYTES, LARGE_BYTES = 64 * MiB, 3200 * MiB


class _H:
    def __init__(self, out, t=None):
        self.out, self.t = out, t
        self.given = None      # chain_append: the frontier and root it left "on the device"


class FakeBackend:
    """Every output is its reference plus the sentinel tail; `corrupt` =
    (operation index, output name) flips one byte of that output ("sentinel":
    the first byte past the verdicts; "<name>.tail": the first byte past that
    output; "untouched_<name>": a byte of an output not asked for;
    "stale_frontier": the chain_append at that index is fed the frontier of
    two steps earlier).  Merkle outputs come from the references; a
    chain_append whose given frontier is not the reference's computes from
    what it was given.  The fifteen Merkle buffers are booked as the model
    books them (sequence_cases.MerkleBufs), within chunk_scratch."""

    def __init__(self, devices=1, corrupt=None):
        self.at, self.corrupt = 0, corrupt
        self.dev = [{"live": False, "slots": {}, "tickets": 0, "pipe": False, "policy": 0, "compact": False,
                     "large": False, "mem": dict.fromkeys(sc.MEMORY_FIELDS[2:], 0), "mk": sc.MerkleBufs()}
                    for _ in range(devices)]
        self.calls = []
        self.op = None
        self.chain = []        # handles of the chain_appends so far

    # -- the book
    def touch(self, dev, field=None, amount=0):
        d = self.dev[dev]
        d["live"] = True
        if d["policy"] == sc.TABLES_LARGE:
            d["large"] = True
        elif d["policy"] == sc.TABLES_COMPACT or not d["large"]:
            d["compact"] = True
        if field:
            d["mem"][field] = max(d["mem"][field], amount)

    def context_count(self):
        return sum(1 for d in self.dev if d["live"])

    def memory(self, dev):
        d = self.dev[dev]
        m = dict(d["mem"], sb_tables=COMPACT_BYTES * d["compact"] + LARGE_BYTES * d["large"]) if d["live"] else \
            dict.fromkeys(sc.MEMORY_FIELDS[1:], 0)
        if d["live"]:
            m["chunk_scratch"] += d["mk"].total()
        m["total"] = sum(m.values())
        return m

    def table_state(self, dev):
        d = self.dev[dev]
        return {"policy": d["policy"], "compact_bytes": COMPACT_BYTES * d["compact"],
                "large_bytes": LARGE_BYTES * d["large"], "large_failed": 0}

    def busy(self, d):
        return bool(d["slots"]) or d["pipe"]

    def lifecycle(self, name, dev, *args):
        d = self.dev[dev]
        self.calls.append((self.at, name))
        if name in ("trim", "release"):
            if not d["live"]:
                return 0
            if self.busy(d):
                return sc.E_BUSY
            if name == "release":
                d.update(live=False, compact=False, large=False, mem=dict.fromkeys(sc.MEMORY_FIELDS[2:], 0))
                d["mk"].release()
                return 0
            d["mk"].trim(args[0])
            keep_large = d["policy"] == sc.TABLES_LARGE or (d["policy"] == sc.TABLES_AUTO and args[0] >= 65536)
            if d["large"] and not keep_large:
                d["large"] = False
            elif d["large"] and keep_large:
                d["compact"] = False
            if args[0] == 0:
                d["mem"].update({f: 0 for f in d["mem"] if f != "signer_comb"})
            return 0
        if name == "set_table_policy":
            d["policy"] = args[0]
        elif name == "set_chunk":
            self.touch(dev)
            d["pipe"] = False
        elif name == "pipeline_sync":
            self.touch(dev)
            d["pipe"] = False
        elif name == "self_test":
            self.touch(dev, "sync_inputs", 4097)
        elif name == "prepare":
            self.touch(dev, "sync_inputs", args[0] * 1000)
            self.touch(dev, "chunk_scratch", args[0] * 1000)
            if args[1] & sc.PREPARE_ASYNC:
                self.touch(dev, "async_slots", args[0] * 8000)
                d["slots"].clear()
                d["tickets"] += 16
        return 0

    # -- outputs
    def out(self, want, t=None, untouched=()):
        got = {k: np.concatenate([np.asarray(v, np.uint8).ravel(), np.full(sc.tail_of(k), sc.SENT, np.uint8)])
               for k, v in want.items()}
        got.update({"untouched_" + k: np.full(64, sc.SENT, np.uint8) for k in untouched})
        if self.corrupt and self.corrupt[0] == self.at and self.corrupt[1] != "stale_frontier":
            name = self.corrupt[1]
            if name == "sentinel":
                got["verdict"][len(want["verdict"])] ^= 1
            elif name.endswith(".tail"):
                got[name[:-5]][len(want[name[:-5]])] ^= 1
            elif name.startswith("untouched_"):
                got[name][5] ^= 1
            else:
                got[name][len(want[name]) // 2] ^= 1
        return _H(got, t)

    def verify_sync(self, dev, lo, n, mem):
        self.touch(dev, "sync_inputs", n)
        return self.out(sc.expect(sc.Op("verify_sync", lo=lo, n=n)))

    def submit_async(self, dev, lo, n, api, digests, mem):
        d = self.dev[dev]
        self.touch(dev, "async_slots", n)
        t = d["tickets"]
        d["tickets"] += 1
        d["slots"][t % sc.K_SLOTS] = t      # a batch still there is handed over by the reuse
        return self.out(sc.expect(sc.Op("verify_async", lo=lo, n=n, digests=digests)), t)

    def ticket(self, h):
        return h.t

    def _settle(self, dev, h):
        self.touch(dev)
        d = self.dev[dev]
        if d["slots"].get(h.t % sc.K_SLOTS) == h.t:
            del d["slots"][h.t % sc.K_SLOTS]
        return 0

    wait = query = _settle

    def verify_device(self, dev, lo, n, stream, flags, shift):
        self.touch(dev, "chunk_scratch", n)
        return self.out(sc.expect(sc.Op("verify_device", lo=lo, n=n)))

    def verify_pipelined(self, dev, lo, n, flags):
        self.touch(dev, "pipelined_sets", n)
        self.dev[dev]["pipe"] = True
        return self.out(sc.expect(sc.Op("verify_pipelined", lo=lo, n=n)))

    def sha256_host(self, dev, lo, n):
        self.touch(dev, "sync_inputs", n)
        return self.out(sc.expect(sc.Op("sha256_host", lo=lo, n=n)))

    def sha256_device(self, dev, lo, n, stream):
        self.touch(dev)
        return self.out(sc.expect(sc.Op("sha256_device", lo=lo, n=n)))

    def sign_device(self, dev, lo, n, seeds, stream):
        self.touch(dev, "signer_comb", 1)
        seed = next(s for s in range(4) if np.array_equal(sc.signed(lo, n, s)[0], seeds))
        return self.out(sc.expect(sc.Op("sign_device", lo=lo, n=n, seed=seed)))

    def _mk(self, dev, step=None):
        """the Merkle buffers the operation at hand grows"""
        self.touch(dev)
        self.dev[dev]["mk"].ensure(sc.merkle_needs(self.op, step))

    def _merkle(self, dev, c, leaf=True, node=True):
        self._mk(dev)
        want = {"leaf": c["leaf"], "node": c["node"], "frontier": c["new"], "root": c["root"]}
        return self.out({k: v for k, v in want.items() if (k != "leaf" or leaf) and (k != "node" or node)})

    def merkle_host(self, dev, c, leaf, node):
        return self._merkle(dev, c, leaf, node)

    def merkle_device(self, dev, c, stream):
        return self._merkle(dev, c)

    def _append(self, dev, c, roots, paths, leaf, node):
        self._mk(dev)
        want = sc.expect(self.op)
        return self.out(want, untouched=[k for k, asked in zip(sc.APPEND_FLAGS, (roots, paths, leaf, node)) if not asked])

    def append_host(self, dev, c, roots, paths, leaf, node):
        return self._append(dev, c, roots, paths, leaf, node)

    def append_device(self, dev, c, stream, roots, paths, leaf, node):
        return self._append(dev, c, roots, paths, leaf, node)

    def _proofs(self, dev, *_args):
        self._mk(dev)
        return self.out(sc.expect(self.op), untouched=() if self.op.computed else ("computed",))

    verify_incl_host = verify_cons_host = verify_incl_device = verify_cons_device = verify_appended = _proofs

    def chain_append(self, dev, prev, step, stream, keep_hashes, restart):
        self._mk(dev, step)
        given = prev
        if self.corrupt == (self.at, "stale_frontier"):
            given = self.chain[-2]
        want = sc.chain_expect(self.op, step)
        fr = b"" if given is None else bytes((given.copy if restart else given.given)["frontier"])
        ref = bytes(step["old_frontier"])
        if fr != ref:       # not the frontier the history leads to: compute from what was given
            old = step["start"]
            have = [fr[i:i + 32] for i in range(0, len(fr), 32)]
            have = [(have or [bytes(32)])[i % max(len(have), 1)] for i in range(sc.mc.popcount(old))]
            roots, paths = sc.ac.simulate_appends(old, have, step["leaves"])
            lh, nodes, new, root = sc.mc.simulate(old, have, step["leaves"])
            want.update(roots=sc._u8(b"".join(roots)), paths=sc._u8(sc.ac.packed(paths)), frontier=sc._u8(b"".join(new)),
                        root=sc._u8(root))
            if keep_hashes:
                want.update(leaf=sc._u8(lh), node=sc._u8(nodes))
        h = self.out(want, untouched=() if keep_hashes else ("leaf", "node"))
        h.n = step["n"]
        h.given = {"frontier": np.array(want["frontier"]), "root": np.array(want["root"])}
        self.chain.append(h)
        return h

    def chain_verify(self, dev, cur, step, stream):
        self.touch(dev)
        return self.out(sc.chain_expect(self.op, step), untouched=("ccomputed",))

    def pack_bits(self, dev, src, n, stream):
        self.touch(dev)
        return self.out({"bitmask": np.packbits(src.out["verdict"][:n], bitorder="little")})

    def stream_sync(self, name):
        pass

    def read(self, h):
        return h.out

    def drop(self, h):
        pass


ALL = list(sc.DIRECTED) + ["random_%d" % s for s in sc.SEEDS] + ["random_merkle_%d" % s for s in sc.MERKLE_SEEDS]
# generate(seed, 80) at the commit before the batched append and the proof verification entered the sequences:
# SHA-256 of repr(list).  The new kinds enter through generate's `merkle` argument only.
FROZEN = {41: "5be5e675066e293e80b219e3ce8480488f3aa3a425bf0f7e53964956d4085e50",
          42: "1c871362aa5e5f10889ccd13d8a4e4b4f8f3ce01bcd30b41dd9238b1466827fc",
          65: "9dbf7ba47f152c910042c6eca494c50eafac0222ec20ef758a1e76141f6d2227"}
# the conditions a directed list is written for (the random seeds and the directed lists together meet all of them)
DIRECTED_COVERS = {
    "ladder_pageable": ("family_sync", "family_latency", "chunk_below", "latency_kernels"),
    "ladder_pinned3": ("family_sync", "family_latency", "chunk_below", "latency_kernels"),
    "ladder_async": ("family_sync", "family_slots", "chunk_below", "async_routes", "latency_kernels"),
    "ladder_device": ("family_sync", "family_latency", "chunk_below", "latency_kernels"),
    "ladder_pipelined": ("family_pipe", "chunk_below", "chunk_above"),
    "slots": ("two_busy", "family_slots", "async_routes", "latency_kernels", "noalloc_sync", "noalloc_async"),
    "pipelined": ("family_pipe", "chunk_below", "chunk_above"),
    "two_streams": ("family_merkle",),
    "release_in_the_middle": ("every_kind", "release_then_four_kinds", "family_merkle", "latency_kernels",
                              "noalloc_sync"),
    "table_rotation": ("family_sync", "family_slots", "family_pipe", "family_latency", "latency_kernels"),
    "two_devices": ("release_then_four_kinds",),
    # the lists of the batched append and the proof verification: each is written for its own conditions of
    # sequence_cases.merkle_coverage (a list of host forms cannot run the fold scratch on two streams); the seeded
    # lists random_merkle_<seed> meet all of them, each alone
    "merkle_staging": ("append_flag_combinations", "kept_stage", "kept_mv", "freed_stage", "freed_mv",
                       "inclusion_consistency_both_orders"),
    "merkle_fold_streams": ("fold_two_streams", "freed_fold", "family_merkle"),
    "ledger_chain": ("kept_fold", "freed_fold", "chain_crosses_power_of_two", "two_busy_then_merkle", "two_busy",
                     "family_merkle"),
}
DIRECTED_COVERS["release_in_the_middle"] += ("every_new_kind",)


@pytest.fixture(scope="module")
def runs():
    """every sequence once on the fake backend"""
    t0 = time.perf_counter()
    p = sc.pool()
    print("references of the pool: %.2f s" % p.build_seconds)
    out = {}
    for name in ALL:
        ops, devices, seed = sc.sequence(name)
        t1, m0 = time.perf_counter(), sc.merkle_seconds()
        out[name] = sc.run(ops, FakeBackend(devices), devices, seed)
        out[name].merkle_s = sc.merkle_seconds() - m0
        print("%-24s %3d operations, %9d bytes compared, references and model %.2f s (the Merkle references' share "
              "%.2f s)" % (name, len(ops), out[name].comparisons, time.perf_counter() - t1, out[name].merkle_s))
    print("all sequences: %.2f s" % (time.perf_counter() - t0))
    return out


def test_generator_is_deterministic_per_seed():
    for seed in sc.SEEDS:
        a, b = sc.generate(seed, sc.STEPS), sc.generate(seed, sc.STEPS)
        assert a == b and sc.STEPS - 3 <= len(a) <= sc.STEPS
        assert a[-1].kind == "release"
    assert sc.generate(sc.SEEDS[0], sc.STEPS) != sc.generate(sc.SEEDS[1], sc.STEPS)
    ops = sc.generate(sc.SEEDS[0], sc.STEPS)
    assert not any(o.kind == "set_table_policy" and o.value == sc.TABLES_LARGE for o in ops)
    assert all(o.get("n", 0) < 65536 for o in ops if not o.kind.startswith("merkle"))     # the 3 GiB set is never built


@pytest.mark.parametrize("name", ALL)
def test_sequence_runs_on_the_fake_backend_and_ends_clean(runs, name):
    """The model's expectations (return codes, hand-overs, slots) agree with the
    fake backend's own book at every operation; nothing is left in flight; the
    sequence ends released."""
    r = runs[name]
    assert r.comparisons > 0 and not r.handles
    assert r.be.context_count() == 0
    assert all(not d.slots and not d.pipe for d in r.model.dev)
    busy = [t for t in r.model.trace if t["rc"] == sc.E_BUSY]
    assert all(t["kind"] in ("trim", "release") for t in busy)
    assert len(r.model.trace) == len(r.ops)          # every operation ran: none skipped


def test_generate_without_the_new_kinds_returns_the_lists_it_returned_before():
    import hashlib
    for seed, digest in FROZEN.items():
        assert hashlib.sha256(repr(sc.generate(seed, sc.STEPS)).encode()).hexdigest() == digest, seed
        assert not any(o.kind in sc.NEW_KINDS for o in sc.generate(seed, sc.STEPS))
    assert len(sc.MERKLE_SEEDS) == 2
    for seed in sc.MERKLE_SEEDS:
        a = sc.generate(seed, sc.MERKLE_STEPS, merkle=True)
        assert a == sc.generate(seed, sc.MERKLE_STEPS, merkle=True) and a[-1].kind == "release"
        assert not any(o.get("n") == 66000 and o.kind not in ("merkle_host", "merkle_device") for o in a)


@pytest.mark.parametrize("name", ALL)
def test_coverage_conditions(runs, name):
    c = sc.coverage(runs[name].model.trace, merkle=name.startswith("random_merkle_"))
    if name.startswith("random_"):
        assert all(c.values()), [k for k, v in c.items() if not v]
    else:
        c = sc.coverage(runs[name].model.trace, merkle=True)
        assert all(c[k] for k in DIRECTED_COVERS[name]), [k for k in DIRECTED_COVERS[name] if not c[k]]


def test_the_new_lists_are_what_the_issue_lists(runs):
    """sizes from the grids, the chain's history, the device verifies compared with context_memory"""
    ops = {name: [t["op"] for t in runs[name].model.trace] for name in sc.DIRECTED}
    st = ops["merkle_staging"]
    assert [(o.kind, o.n, o.computed) for o in st if o.kind.startswith("verify_")][:5] == [
        ("verify_incl_host", 4097, True), ("verify_cons_host", 63, False), ("verify_incl_host", 65, True),
        ("verify_cons_host", 257, True), ("verify_incl_host", 1, False)]
    assert all(o.kind in ("append_host", "merkle_host", "verify_incl_host", "verify_cons_host", "trim", "release")
               for o in st)
    flags = {tuple(o.p[f] for f in sc.APPEND_FLAGS) for o in st if o.kind == "append_host"}
    assert len(flags) == 16 and {o.n for o in st if o.kind == "append_host"} == {65, 1000, 64}
    assert any(a.kind == "append_host" and b.kind == "merkle_host" and not b.leaf and not b.node and c.kind == "append_host"
               for a, b, c in zip(st, st[1:], st[2:]))
    assert {(o.get("leaf_base", 0) != 0, o.proof_base != 0) for o in st if o.kind == "verify_incl_host"} == {
        (False, True), (True, False), (False, False)}
    fs = ops["merkle_fold_streams"]
    assert [o.n for o in fs if o.kind == "append_device"][:3] == [257, 66000, 63]
    assert sum(1 for o in fs if o.kind == "release") == 2 and sum(1 for o in fs if o.kind == "trim" and o.keep == 0) == 3
    ch = ops["ledger_chain"]
    ns = [o.n for o in ch if o.kind == "chain_append"]
    assert len(ns) == 10 and set(ns) <= set(sc.APPEND_SIZES) and 66000 in ns and 1000 in ns
    trace = runs["ledger_chain"].model.trace
    assert any(t.get("restart") for t in trace) and sum(1 for t in trace if t["rc"] == sc.E_BUSY) == 2
    assert any(t["kind"] == "trim" and t["rc"] == 0 for t in trace)
    used = {o.n for name in sc.DIRECTED for o in ops[name] if o.kind in ("append_host", "append_device", "chain_append")}
    assert used == set(sc.APPEND_SIZES)
    olds = {sc.ac.OLD_GRID[o.old] for name in sc.DIRECTED for o in ops[name] if o.kind in ("append_host", "append_device")}
    assert olds == set(sc.APPEND_OLD)
    proofs = {o.n for name in sc.DIRECTED for o in ops[name] if o.kind.startswith("verify_") and "n" in o.p
              and o.get("src") is None and o.kind != "verify_sync" and "seed" in o.p}
    assert proofs == set(sc.PROOF_SIZES)
    for name, r in runs.items():     # every device verify in a live context was compared with context_memory
        assert r.nomem_checks == sum(1 for t in r.model.trace if t.get("nomem")), name
    assert runs["merkle_fold_streams"].nomem_checks >= 6 and runs["ledger_chain"].nomem_checks >= 6


def test_directed_lists_together_meet_every_condition(runs):
    met = set()
    for name in sc.DIRECTED:
        met |= {k for k, v in sc.coverage(runs[name].model.trace).items() if v}
    trace = [t for name in sc.DIRECTED for t in runs[name].model.trace]
    values = {(t["kind"], t["op"].get("value", t["op"].get("keep"))) for t in trace}
    assert all((k, v) in values for k, vs in sc.SETTING_VALUES.items() for v in vs)
    assert {t["op"].flags for t in trace if t["kind"] == "prepare"} >= {0, sc.PREPARE_ASYNC}
    assert met >= set(sc.coverage([])) - {"every_setting_value", "prepare_both"}
    assert runs["slots"].noalloc_checks == 35 and runs["release_in_the_middle"].noalloc_checks == 6
    for name, r in runs.items():       # every check the model plans is one the runner made
        assert r.noalloc_checks == sum(1 for t in r.model.trace if t["noalloc"]), name
    ops = [t["op"] for name in sc.DIRECTED for t in runs[name].model.trace]
    assert any(o.kind == "merkle_host" and not o.leaf for o in ops)
    assert any(o.kind == "merkle_host" and not o.node for o in ops)
    assert any(o.kind == "verify_device" and o.flags & sc.FLAG_UNIFORM_LENGTH and o.n == sc.UNIFORM_N for o in ops)
    two = runs["two_devices"].model.trace
    assert any(t["kind"] == "release" and t["rc"] == 0 and t["dev"] == 0 and
               any(u["dev"] == 1 and u["kind"] == "wait_async" and u["i"] > t["i"] for u in two) for t in two)


def test_replay_reproduces_the_prefix():
    seed = sc.SEEDS[0]
    full = sc.generate(seed, sc.STEPS)
    r = sc.replay(seed, 40, FakeBackend(), sc.STEPS)
    assert r.ops == full[:40] and len(r.model.trace) == 40


def test_failure_message_carries_seed_and_operations():
    seed = sc.SEEDS[0]
    ops = sc.generate(seed, sc.STEPS)
    at = next(i for i, o in enumerate(ops) if o.kind == "verify_sync")
    with pytest.raises(sc.SequenceFailure) as ex:
        sc.run(ops, FakeBackend(corrupt=(at, "verdict")), 1, seed)
    text = str(ex.value)
    assert "seed %d" % seed in text and "operation %d" % at in text
    for i in range(at + 1):
        assert "%4d  %r" % (i, ops[i]) in text
    assert len(text.split("operations up to it:")[1].strip().splitlines()) == at + 1      # the prefix, no more


def _one_of_each_merkle():
    q = sc.Seq()
    q.add("append_host", old=sc._old(255), n=65, roots=True, paths=True, leaf=True, node=True)             # 0
    q.add("verify_incl_host", n=63, seed=1, by_hash=False, computed=True, leaf_base=7, proof_base=5)        # 1
    q.add("verify_cons_device", n=64, seed=1, computed=True, proof_base=sc.BIG_BASE, stream=None)           # 2
    q.add("chain_append", n=63, stream=None, keep_hashes=True)                                              # 3
    q.add("chain_append", n=1, stream="a", keep_hashes=False)                                               # 4
    q.add("chain_append", n=65, stream="a", keep_hashes=False)                                              # 5
    q.add("chain_verify", stream="a")                                                                       # 6
    q.add("sync", stream="a")                                                                               # 7
    q.add("append_device", old=sc._old(0), n=64, stream=None, roots=False, paths=True, leaf=False, node=True)   # 8
    q.add("verify_cons_host", n=65, seed=2, computed=False, proof_base=0)                                   # 9
    q.add("release", final=True)
    return q


@pytest.mark.parametrize("what,at,caught", [
    ("roots", 0, 0), ("paths", 0, 0), ("roots.tail", 0, 0), ("paths.tail", 0, 0), ("leaf.tail", 0, 0),
    ("node.tail", 0, 0), ("frontier.tail", 0, 0), ("root.tail", 0, 0),
    ("status", 1, 1), ("computed", 1, 1), ("status.tail", 1, 1), ("computed.tail", 1, 1),
    ("status", 2, 2), ("computed", 2, 2), ("status.tail", 2, 2), ("computed.tail", 2, 2),
    ("frontier", 3, 3), ("frontier.tail", 3, 3), ("cstatus", 3, 3), ("ccomputed", 3, 3), ("cstatus.tail", 3, 3),
    ("ccomputed.tail", 3, 3), ("roots", 3, 3), ("paths.tail", 3, 3),
    ("frontier", 4, 7), ("untouched_leaf", 4, 7), ("stale_frontier", 5, 7), ("status", 6, 7), ("cstatus.tail", 6, 7),
    ("computed", 6, 7), ("untouched_roots", 8, 8), ("paths", 8, 8), ("untouched_computed", 9, 9), ("status", 9, 9)])
def test_one_wrong_byte_of_a_merkle_output_is_caught_at_its_operation(what, at, caught):
    """A flipped byte of a per-leaf root, a packed path entry, a status, a computed root, a chained frontier and
    of every sentinel tail; an output not asked for written; a chain step fed the frontier of two steps earlier.
    Each is caught where the operation's outputs are checked (at once, or at the sync of its stream), with the
    seed and the operations up to there in the message."""
    ops = _one_of_each_merkle()
    sc.run(ops, FakeBackend(), 1, 7)                          # clean: passes
    with pytest.raises(sc.SequenceFailure) as ex:
        sc.run(ops, FakeBackend(corrupt=(at, what)), 1, 7)
    text = str(ex.value)
    assert "seed 7, operation %d:" % caught in text and "of operation %d " % at in text
    name = what.replace(".tail", "").replace("untouched_", "")
    assert name in text or what == "stale_frontier"
    assert ("sentinel" in text) == what.endswith(".tail") and ("not asked for" in text) == what.startswith("untouched_")
    assert len(text.split("operations up to it:")[1].strip().splitlines()) == caught + 1
    if what == "stale_frontier":      # the first output that depends on the frontier: the per-leaf roots of that step
        assert "roots of operation 5 " in text


def _one_of_each():
    q = sc.Seq()
    q.add("verify_sync", lo=37, n=257, mem="pageable")
    q.add("sha256_host", lo=0, n=17)
    q.add("sign_device", lo=0, n=17, seed=0, stream=None)
    q.add("merkle_host", old=3, n=257)
    q.add("verify_device", lo=0, n=255, stream=None, flags=0, shift=False)
    q.add("pack_bits", lo=0, n=255, stream=None)
    t = q.add("verify_async", lo=1, n=16, api="digest", digests=True, mem="pageable")
    q.add("wait_async", tid=t)
    q.add("release", final=True)
    return q


@pytest.mark.parametrize("what,at", [("verdict", 0), ("digest", 1), ("signature", 2), ("leaf", 3), ("node", 3),
                                     ("root", 3), ("bitmask", 5), ("sentinel", 0)])
def test_one_wrong_byte_is_caught_at_its_operation(what, at):
    ops = _one_of_each()
    sc.run(ops, FakeBackend(), 1, None)                       # clean: passes
    with pytest.raises(sc.SequenceFailure) as ex:
        sc.run(ops, FakeBackend(corrupt=(at, what)), 1, None)
    assert "operation %d:" % at in str(ex.value)
    assert ("sentinel" if what == "sentinel" else what) in str(ex.value)


def test_a_wrong_byte_of_an_asynchronous_batch_is_caught_at_its_hand_over():
    ops = _one_of_each()
    with pytest.raises(sc.SequenceFailure) as ex:
        sc.run(ops, FakeBackend(corrupt=(6, "digest")), 1, None)
    assert "operation 7:" in str(ex.value) and "digest of operation 6" in str(ex.value)


def test_model_flags_a_sequence_it_cannot_place():
    """an operation that cannot be placed is an error, not a skip"""
    with pytest.raises(sc.SequenceFailure):
        sc.run([sc.Op("wait_async", tid=3)], FakeBackend(), 1, None)
    with pytest.raises(sc.SequenceFailure):
        sc.run([sc.Op("verify_device", lo=0, n=257, stream=None, flags=sc.FLAG_UNIFORM_LENGTH, shift=False)],
               FakeBackend(), 1, None)
