"""Operation sequences over one device context (csrc/edv_runtime.hip, DevCtx):
operations, a plain model of the context's history, the references, the
generator and the runner that tests/test_gpu_sequences.py (the device) and
tests/test_sequence_model_cpu.py (a fake backend) share.

An operation is a record of kind and parameters.  The runner executes it on a
backend and compares what came out with references only: verdicts with
test_gpu_runtime.checker (libsodium where present, else the oracle), digests
with hashlib.sha256, signatures and keys with oracle_lib.sign / keypair, Merkle
outputs with merkle_cases.simulate, bitmasks with numpy.packbits.  Every output
buffer is longer than its output and sentinel-filled past it.

The model is plain Python: which tickets are outstanding and in which slot,
which pipelined batches and which caller-stream work is unsynced, the five
settings, and from them what each lifecycle call must return (EDV_E_BUSY with
nothing changed exactly when a ticket is not handed over or a pipelined batch
is not synced).  It also records a trace -- route and buffer family per
operation -- from which the coverage conditions are read.

The comb table of the signer is not a buffer edv_trim frees (include/edv.h), so
"after trim(0) the total is the table set's" is checked as total == sb_tables +
signer_comb, with signer_comb == 0 unless a signing ran since the last release.
"""
import ctypes
import hashlib
import random
import time

import numpy as np

import merkle_cases as mc
import oracle_lib as orc

POOL_N = 20000
POOL_SEED = 0x5EC0DE
HEAD = 64                                   # oracle-signed requests at the pool's start
SPECIAL = (0, 1, 47, 48, 111, 112, 175, 176, 4096)
UNIFORM_LO, UNIFORM_N = 36, 28              # requests [36, 64): one SHA-512 block each
SENT = 0xA5
ROW = 16                                    # sentinel bytes past a verdict row (a digest / hash row: 32)

K_BLOCK, K_RTL_MAX, K_SMALL_ASYNC, K_QUAD_DEFAULT, K_SLOTS = 256, 4096, 8192, 16384, 8
CHUNK_DEFAULT = 1 << 18
SIZES = (1, 16, 17, 255, 256, 257, 4096, 4097, 8192, 8193, 16384, 16385, 20000)
SIGN_SIZES = (1, 17, 256, 257, 1024)
MERKLE_SIZES = (1, 257, 1000, 66000)
MERKLE_MAX_SIZE = 1 << 62                   # include/edv.h: tree sizes up to 2^62
CHUNKS = (256, 1024, 4096, 0)
LATENCY = (0, 4096, K_QUAD_DEFAULT)
TRIMS = (0, 1, 400, 4097, 20000)
E_BUSY = -5
TABLES_AUTO, TABLES_COMPACT, TABLES_LARGE = 0, 1, 2
PREPARE_ASYNC = 1
FLAG_UNIFORM_LENGTH, FLAG_BUCKETS, FLAG_SPLIT_PREP = 1, 2, 4
PREPARE_MSG_BYTES = 512
FAMILIES = ("sync", "slots", "pipe", "latency", "merkle")
MEMORY_FIELDS = ("total", "sb_tables", "chunk_scratch", "async_slots", "pipelined_sets", "sync_inputs", "signer_comb")


class Op:
    """kind and parameters; parameters read as attributes (dev defaults to 0)"""
    __slots__ = ("kind", "p")

    def __init__(self, kind, **p):
        self.kind, self.p = kind, p

    def __getattr__(self, k):
        if k == "dev":
            return self.p.get("dev", 0)
        try:
            return self.p[k]
        except KeyError:
            raise AttributeError(k)

    def get(self, k, d=None):
        return self.p.get(k, d)

    def __eq__(self, o):
        return isinstance(o, Op) and (self.kind, self.p) == (o.kind, o.p)

    def __repr__(self):
        return "%s(%s)" % (self.kind, ", ".join("%s=%r" % kv for kv in self.p.items()))


class SequenceFailure(AssertionError):
    pass


# ------------------------------------------------------------------ the pool
def special_order():
    """The nine special lengths, each starting at every offset mod 4 when laid
    end to end from offset 0: 47, 111, 175 and 1 step the residue (four steps
    come back to it), the multiples of 4 ride along at each residue."""
    out = []
    for step, same in ((47, (0, 48)), (111, (112, 176)), (175, ()), (1, (4096,))):
        for _ in range(4):
            out.extend(same)
            out.append(step)
    return out


class Pool:
    """20,000 requests in the C-ABI layout (msgs ends with 64 spare bytes),
    their verdicts by the checker and their digests by hashlib."""

    def __init__(self):
        from test_gpu_runtime import checker
        t0 = time.perf_counter()
        S, P, M, O = orc.corpus(POOL_SEED, 0, POOL_N, mode=1, invalid_permille=200)
        r = random.Random(POOL_SEED)
        lens = special_order() + [r.randrange(0, 48) for _ in range(UNIFORM_N)]
        assert len(lens) == HEAD
        keys = [orc.keypair(bytes([k, 0x5E]) * 16) for k in range(8)]
        sigs, pks, msgs = [], [], []
        for i, ln in enumerate(lens):
            pk, sk = keys[r.randrange(8)]
            m = r.getrandbits(8 * ln).to_bytes(ln, "little") if ln else b""
            sig = bytearray(orc.sign(m, sk))
            if i % 5 == 2:
                sig[32 + r.randrange(31)] ^= 1 << r.randrange(8)     # a damaged S
            sigs.append(bytes(sig))
            pks.append(pk)
            msgs.append(m)
        head = b"".join(msgs)
        self.sigs = np.concatenate([np.frombuffer(b"".join(sigs), np.uint8), S[64 * HEAD:]])
        self.pks = np.concatenate([np.frombuffer(b"".join(pks), np.uint8), P[32 * HEAD:]])
        self.msgs = np.concatenate([np.frombuffer(head, np.uint8), M[int(O[HEAD]):int(O[-1])], np.zeros(64, np.uint8)])
        self.lens = np.concatenate([np.array(lens, np.uint64), np.diff(O)[HEAD:]])
        self.off = np.zeros(POOL_N + 1, np.uint64)
        self.off[1:] = np.cumsum(self.lens)
        assert self.msgs.nbytes == int(self.off[-1]) + 64
        starts = {(ln, int(o) % 4) for ln, o in zip(lens[:36], self.off[:36])}
        assert starts == {(ln, k) for ln in SPECIAL for k in range(4)}, "a special length misses a start offset mod 4"
        self.want = np.ascontiguousarray(checker(self.sigs, self.pks, self.msgs, self.off), dtype=np.uint8)
        assert 0.7 < self.want.mean() < 0.9 and 0 < int(self.want[:HEAD].sum()) < HEAD
        blob = self.msgs.tobytes()
        self.digests = np.frombuffer(b"".join(hashlib.sha256(blob[int(self.off[i]):int(self.off[i + 1])]).digest()
                                              for i in range(POOL_N)), np.uint8)
        self.blob = blob
        self.build_seconds = time.perf_counter() - t0

    def message(self, i):
        return self.blob[int(self.off[i]):int(self.off[i + 1])]


_cache = {}


def pool():
    if "pool" not in _cache:
        _cache["pool"] = Pool()
    return _cache["pool"]


def pool_lengths():
    """the pool's message lengths without signing or checking anything (the model and the generator need only these)"""
    if "lens" not in _cache:
        r = random.Random(POOL_SEED)
        head = special_order() + [r.randrange(0, 48) for _ in range(UNIFORM_N)]
        _cache["lens"] = np.concatenate([np.array(head, np.uint64),
                                         orc.corpus_lengths(POOL_SEED, HEAD, POOL_N - HEAD, 1)])
    return _cache["lens"]


def average_bytes(lo, n):
    return float(pool_lengths()[lo:lo + n].sum()) / n


def is_uniform(lo, n):
    """one SHA-512 block count over the range (edv_runtime.hip: sha512_blocks)"""
    b = (pool_lengths()[lo:lo + n] + np.uint64(64 + 17 + 127)) >> np.uint64(7)
    return bool((b == b[0]).all())


# ------------------------------------------------------------------ references
def signed(lo, n, seed):
    """seeds, and the oracle's keys, signatures and the checker's verdicts for the pool's messages [lo, lo + n)"""
    key = ("sign", lo, n, seed)
    if key not in _cache:
        from test_gpu_runtime import checker
        p, r = pool(), random.Random(seed)
        seeds = [r.getrandbits(256).to_bytes(32, "little") for _ in range(n)]
        pairs = [orc.keypair(s) for s in seeds]
        sigs = b"".join(orc.sign(p.message(lo + i), sk) for i, (_pk, sk) in enumerate(pairs))
        pks = b"".join(pk for pk, _sk in pairs)
        s8, p8 = np.frombuffer(sigs, np.uint8), np.frombuffer(pks, np.uint8)
        off = p.off[lo:lo + n + 1]
        want = np.ascontiguousarray(checker(s8, p8, p.msgs, off), dtype=np.uint8)
        _cache[key] = (np.frombuffer(b"".join(seeds), np.uint8), p8, s8, want)
    return _cache[key]


def merkle_case(old_index, n):
    """old size (merkle_cases.OLD_GRID), frontier, leaves (16 bytes each at 66,000), merkle_cases.simulate's outputs"""
    key = ("merkle", old_index, n)
    if key not in _cache:
        old = mc.OLD_GRID[old_index]
        assert old + n <= MERKLE_MAX_SIZE
        fr = mc.frontier(0x5EC, old)
        leaves = mc.leaves_of(0x5EC + old_index, n, lengths=[16]) if n == 66000 else mc.leaves_of(0x5EC + old_index, n)
        blob, off = mc.pack(leaves)
        lh, nodes, new, root = mc.simulate(old, fr, leaves)
        assert len(nodes) == 32 * mc.node_span(old, n)
        _cache[key] = {"old": old, "n": n, "frontier": np.frombuffer(b"".join(fr), np.uint8), "blob": blob, "off": off,
                       "leaf": np.frombuffer(lh, np.uint8), "node": np.frombuffer(nodes, np.uint8),
                       "new": np.frombuffer(b"".join(new), np.uint8), "root": np.frombuffer(root, np.uint8)}
    return _cache[key]


def expect(op):
    """name -> expected bytes (uint8 array) of every output of a data operation"""
    k = op.kind
    if k in ("verify_sync", "verify_device", "verify_pipelined"):
        return {"verdict": pool().want[op.lo:op.lo + op.n]}
    if k == "verify_async":
        out = {"verdict": pool().want[op.lo:op.lo + op.n]}
        if op.digests:
            out["digest"] = pool().digests[32 * op.lo:32 * (op.lo + op.n)]
        return out
    if k in ("sha256_host", "sha256_device"):
        return {"digest": pool().digests[32 * op.lo:32 * (op.lo + op.n)]}
    if k == "sign_device":
        _seeds, pks, sigs, want = signed(op.lo, op.n, op.seed)
        return {"key": pks, "signature": sigs, "verdict": want}
    if k in ("merkle_host", "merkle_device"):
        c = merkle_case(op.old, op.n)
        return {"leaf": c["leaf"], "node": c["node"], "frontier": c["new"], "root": c["root"]}
    if k == "pack_bits":
        return {"bitmask": np.packbits(pool().want[op.lo:op.lo + op.n], bitorder="little")}
    raise KeyError(k)


def tail_of(name):
    return ROW if name in ("verdict", "bitmask") else 32


# ------------------------------------------------------------------ the model
def pow2_cap(need, limit):
    """ChunkBufs::ensure: powers of two from 4,096, at most the chunk"""
    c = 4096
    while c < need:
        c <<= 1
    if c > limit:
        c = limit if limit > need else need
    return c


def latency_kernel(n, quad):
    if n <= quad:
        return "rtl" if n <= K_RTL_MAX else "two_walk"
    return None


class DevModel:
    def __init__(self):
        self.live = False
        self.slots = {}            # slot -> index of the submitting operation
        self.issued = 0            # tickets issued to callers (the warm-ups of prepare take whole rounds of 8)
        self.settled = 0
        self.pipe = []             # indices of pipelined batches not synced
        self.chunk, self.quad, self.buckets, self.slices, self.policy = CHUNK_DEFAULT, K_QUAD_DEFAULT, 2, 0, TABLES_AUTO
        self.prepared = None       # (k, async) while nothing it depends on has changed
        self.signed = False
        self.cap = {"st": 0, "pst": 0}
        self.last_dev = None       # (index, lo, n) of the last device-resident verify

    def busy(self):
        return bool(self.slots) or bool(self.pipe)


class Exp:
    """what the model expects of one operation"""

    def __init__(self):
        self.rc = 0
        self.handed = []      # indices of asynchronous submissions handed over by this operation
        self.pipe = []        # pipelined batches synced by it
        self.stream = []      # caller-stream operations synced by it
        self.route = None
        self.noalloc = False
        self.slot = None


class Model:
    def __init__(self, devices=1):
        self.dev = [DevModel() for _ in range(devices)]
        self.streams = {"a": [], "b": []}
        self.trace = []

    def idle_streams(self):
        return not self.streams["a"] and not self.streams["b"]

    def _use(self, t, fam, n):
        t.setdefault("use", []).append((fam, n))

    def apply(self, i, op):
        m, e, k = self.dev[op.dev], Exp(), op.kind
        t = {"i": i, "kind": k, "dev": op.dev, "op": op}
        creates = k not in ("sync", "expect_tables", "set_latency_path", "set_length_buckets", "set_host_slices",
                            "set_table_policy", "trim", "release")
        was_live = m.live
        if creates:
            m.live = True
        n = op.get("n", 0)
        if k == "verify_sync":
            lat = latency_kernel(n, m.quad)
            e.route = lat or ("fields" if n <= m.chunk else "subbatches")
            self._use(t, "latency" if lat else "sync", n)
            if not lat:
                m.cap["st"] = max(m.cap["st"], pow2_cap(min(n, m.chunk), m.chunk))
            t["multi"] = not lat and n > m.chunk
            e.noalloc = bool(m.prepared and n <= m.prepared[0] and average_bytes(op.lo, n) <= PREPARE_MSG_BYTES)
        elif k == "verify_async":
            e.slot = m.issued % K_SLOTS
            m.issued += 1
            if e.slot in m.slots:
                e.handed.append(m.slots[e.slot])
            m.slots[e.slot] = i
            lat = latency_kernel(n, m.quad)
            e.route = lat or ("own" if n <= K_SMALL_ASYNC else "shared")
            self._use(t, "slots", n)
            if e.route == "shared":
                self._use(t, "sync", n)
                m.cap["st"] = max(m.cap["st"], pow2_cap(min(n, m.chunk), m.chunk))
            t["multi"] = not lat and n > m.chunk
            e.noalloc = bool(m.prepared and m.prepared[1] and n <= m.prepared[0] and
                             average_bytes(op.lo, n) <= PREPARE_MSG_BYTES)
        elif k in ("wait_async", "query_async"):
            slot = [s for s, j in m.slots.items() if j == op.tid]
            if not slot:
                raise ValueError("operation %d: no outstanding batch %r" % (i, op.tid))
            del m.slots[slot[0]]
            e.handed.append(op.tid)
        elif k == "verify_device":
            lat = latency_kernel(n, m.quad)
            e.route = lat or "chunks"
            self._use(t, "latency" if lat else "sync", n)
            if not lat:
                m.cap["st"] = max(m.cap["st"], pow2_cap(min(n, m.chunk), m.chunk))
            t["multi"] = not lat and n > m.chunk
            if op.flags & FLAG_UNIFORM_LENGTH and not is_uniform(op.lo, n):
                raise ValueError("operation %d: FLAG_UNIFORM_LENGTH on a range that is not uniform" % i)
            m.last_dev = (i, op.lo, n)
            if op.stream:
                self.streams[op.stream].append(i)
        elif k == "sync":
            e.stream, self.streams[op.stream] = self.streams[op.stream], []
        elif k == "verify_pipelined":
            m.pipe.append(i)
            e.route = "pipelined"
            self._use(t, "pipe", min(n, m.chunk))
            m.cap["pst"] = max(m.cap["pst"], pow2_cap(min(n, m.chunk), m.chunk))
            t["multi"] = n > m.chunk
        elif k == "pipeline_sync":
            e.pipe, m.pipe = m.pipe, []
        elif k in ("sha256_device", "sign_device", "merkle_device", "pack_bits"):
            if k == "sign_device":
                m.signed = True
                if n > 1024:
                    raise ValueError("operation %d: signing is for n <= 1,024" % i)
            if k == "merkle_device":
                self._use(t, "merkle", n)
            if k == "pack_bits":
                if m.last_dev is None or m.last_dev[1:] != (op.lo, n):
                    raise ValueError("operation %d: pack_bits without the device-resident verify it packs" % i)
                t["src"] = m.last_dev[0]
            if op.stream:
                self.streams[op.stream].append(i)
        elif k == "merkle_host":
            self._use(t, "merkle", n)
        elif k == "sha256_host":
            pass
        elif k == "set_chunk":
            e.pipe, m.pipe = m.pipe, []      # edv_set_chunk drains the context
            new = op.value or CHUNK_DEFAULT
            held = max(m.cap.values())
            t["chunk_vs_cap"] = "below" if held and new < held else "above" if held and new > held else "none"
            m.chunk, m.prepared = new, None
        elif k == "set_latency_path":
            m.quad, m.prepared = op.value, None
        elif k == "set_length_buckets":
            m.buckets = op.value
        elif k == "set_host_slices":
            m.slices = op.value
        elif k == "set_table_policy":
            m.policy, m.prepared = op.value, None
        elif k == "prepare":
            if op.flags & PREPARE_ASYNC:     # the warm-ups go through every slot: whole rounds of 8 tickets
                first = m.issued % K_SLOTS
                for s in range(K_SLOTS):
                    if (first + s) % K_SLOTS in m.slots:
                        e.handed.append(m.slots.pop((first + s) % K_SLOTS))
            m.prepared = (op.k, bool(op.flags & PREPARE_ASYNC))
            if not latency_kernel(op.k, m.quad):     # a warm-up of k requests on the batch kernels
                m.cap["st"] = max(m.cap["st"], pow2_cap(min(op.k, m.chunk), m.chunk))
        elif k in ("self_test", "expect_tables"):
            pass
        elif k in ("trim", "release"):
            if not was_live:
                t["idle"] = True
            elif m.busy():
                e.rc = E_BUSY
            else:
                m.prepared = None
                if k == "release":
                    m.live, m.signed, m.cap = False, False, {"st": 0, "pst": 0}
                    t["probes"] = 0 if op.get("final") else min(m.settled, 2)   # the last release leaves nothing behind
                    if t["probes"]:
                        m.live = True       # edv_wait_async on an old ticket makes a fresh context
                else:
                    slots = 0
                    if op.keep:
                        slots = 4096
                        while slots < op.keep and slots < m.chunk:
                            slots <<= 1
                        slots = min(slots, m.chunk)
                    t["freed"] = [fam for fam, name in (("sync", "st"), ("pipe", "pst")) if m.cap[name] > slots]
                    for name in m.cap:
                        if m.cap[name] > slots:
                            m.cap[name] = 0
        else:
            raise ValueError("unknown operation kind %r" % k)
        m.settled += len(e.handed)
        t.update(rc=e.rc, route=e.route, handed=list(e.handed), noalloc=e.noalloc)
        self.trace.append(t)
        return e


# ------------------------------------------------------------------ coverage, read from the trace
SETTING_VALUES = {"set_chunk": CHUNKS, "set_latency_path": LATENCY, "set_length_buckets": (0, 1, 2),
                  "set_host_slices": (0, 2, 8), "set_table_policy": (TABLES_AUTO, TABLES_COMPACT), "trim": TRIMS}
KINDS = ("verify_sync", "verify_async", "wait_async", "query_async", "verify_device", "sync", "verify_pipelined",
         "pipeline_sync", "sha256_host", "sha256_device", "sign_device", "merkle_host", "merkle_device", "pack_bits",
         "prepare", "self_test", "trim", "release", "set_table_policy", "set_chunk", "set_latency_path",
         "set_length_buckets", "set_host_slices")


def freed_by(t, fam, n1):
    """Does this trim / release free the buffers of family `fam` that a use of n1 grew?  For the chunk sets (c.st,
    pst) the model's capacities say so (Model.apply, as trim_buffers computes it); the other families' buffers are
    sized by n: all go with keep 0, and those grown by n1 > 4,096 with a keep of at most half of it."""
    if t["rc"] != 0 or t.get("idle"):
        return False
    if t["kind"] == "release":
        return True
    if fam in ("sync", "pipe"):
        return fam in t.get("freed", ())
    keep = t["op"].keep
    return keep == 0 or (n1 > 4096 and keep <= n1 // 2)


def coverage(trace):
    """name -> bool: the conditions of the issue, over one sequence's trace"""
    c = {}
    kinds = {t["kind"] for t in trace}
    c["every_kind"] = all(k in kinds for k in KINDS)
    vals = {(t["kind"], t["op"].get("value", t["op"].get("keep"))) for t in trace}
    c["every_setting_value"] = all((k, v) in vals for k, vs in SETTING_VALUES.items() for v in vs)
    c["prepare_both"] = {t["op"].flags for t in trace if t["kind"] == "prepare"} >= {0, PREPARE_ASYNC}
    c["two_busy"] = sum(1 for t in trace if t["kind"] in ("trim", "release") and t["rc"] == E_BUSY) >= 2
    rel = [t["i"] for t in trace if t["kind"] == "release" and t["rc"] == 0 and not t.get("idle")]
    c["release_then_four_kinds"] = any(len({t["kind"] for t in trace if t["i"] > r and "use" in t or
                                            t["i"] > r and t["kind"] in ("sha256_host", "sha256_device", "sign_device",
                                                                         "pack_bits")}) >= 4 for r in rel)
    for fam in FAMILIES:
        ok = False
        for a in trace:
            for f, n1 in a.get("use", ()):
                if f != fam or a["dev"] != 0:
                    continue
                for b in trace:
                    if b["i"] > a["i"] and b["dev"] == 0 and b["kind"] in ("trim", "release") and freed_by(b, fam, n1):
                        ok = ok or any(d["i"] > b["i"] and d["dev"] == 0 and any(f2 == fam and n2 > n1
                                                                                  for f2, n2 in d.get("use", ()))
                                       for d in trace)
        c["family_" + fam] = ok
    for rel_ in ("below", "above"):
        c["chunk_" + rel_] = any(a.get("chunk_vs_cap") == rel_ and
                                 any(b["i"] > a["i"] and b.get("multi") for b in trace)
                                 for a in trace if a["kind"] == "set_chunk")
    routes = {t["route"] for t in trace if t["kind"] == "verify_async"}
    c["async_routes"] = {"own", "shared"} <= routes and bool(routes & {"rtl", "two_walk"})
    c["latency_kernels"] = {"rtl", "two_walk"} <= {t["route"] for t in trace}
    # a verify that a prepare covers (at most k requests averaging at most 512 bytes): nothing may be allocated
    c["noalloc_sync"] = any(t["noalloc"] and t["kind"] == "verify_sync" for t in trace)
    c["noalloc_async"] = any(t["noalloc"] and t["kind"] == "verify_async" for t in trace)
    return c


# ------------------------------------------------------------------ the runner
class Runner:
    """Executes operations on a backend, checks every output against its
    reference and the invariants after every operation."""

    def __init__(self, backend, devices=1, seed=None):
        self.be, self.model, self.seed = backend, Model(devices), seed
        self.devices = devices
        self.handles = {}          # operation index -> (operation, backend handle) until its outputs are checked
        self.settled = {}          # device -> its last handed-over asynchronous batches, for the probes after a release
        self.floor = [0] * devices
        self.ops = []
        self.comparisons = 0
        self.noalloc_checks = 0
        self.last_dev = {}         # device -> (index, handle) of the last device-resident verify (pack_bits reads it)

    # -- outputs
    def check(self, i, op, handle):
        got = self.be.read(handle)
        want = expect(op)
        if op.kind in ("merkle_host", "merkle_device"):
            want = {k: v for k, v in want.items() if k in got}
        assert set(got) == set(want), "operation %d %r: outputs %s, expected %s" % (i, op, sorted(got), sorted(want))
        for name, w in want.items():
            g = np.asarray(got[name], np.uint8).ravel()
            w = np.asarray(w, np.uint8).ravel()
            assert g.size == w.size + tail_of(name), "%s of operation %d: %d bytes for %d" % (name, i, g.size, w.size)
            if not np.array_equal(g[:w.size], w):
                bad = int(np.nonzero(g[:w.size] != w)[0][0])
                raise AssertionError("%s of operation %d %r differs from the reference at byte %d of %d "
                                     "(%d, reference %d)" % (name, i, op, bad, w.size, int(g[bad]), int(w[bad])))
            assert (g[w.size:] == SENT).all(), "sentinel past the %s of operation %d %r overwritten" % (name, i, op)
            self.comparisons += int(w.size)

    def finish(self, indices):
        for j in indices:
            op, h = self.handles.pop(j)
            self.check(j, op, h)
            if op.kind == "verify_async":
                self.settled[op.dev] = (self.settled.get(op.dev, []) + [(j, op, h)])[-2:]
            elif self.last_dev.get(op.dev, (None,))[0] != j:
                self.be.drop(h)

    def snapshot(self, dev):
        return self.be.context_count(), self.be.memory(dev), self.be.table_state(dev)

    def step(self, op):
        i = len(self.ops)
        self.ops.append(op)
        try:
            self._step(i, op)
        except SequenceFailure:
            raise
        except Exception as ex:
            raise SequenceFailure("seed %r, operation %d: %s: %s\noperations up to it:\n%s" % (
                self.seed, i, type(ex).__name__, ex, "\n".join("%4d  %r" % kv for kv in enumerate(self.ops)))) from ex

    def _step(self, i, op):
        be, d, k = self.be, op.dev, op.kind
        m = self.model.dev[d]
        be.at = i
        before = self.snapshot(d)
        e = self.model.apply(i, op)
        t = self.model.trace[-1]
        rc = 0
        if k == "verify_sync":
            h = be.verify_sync(d, op.lo, op.n, op.mem)
            self.check(i, op, h)
            be.drop(h)
        elif k == "verify_async":
            h = be.submit_async(d, op.lo, op.n, op.api, op.digests, op.mem)
            assert be.ticket(h) % K_SLOTS == e.slot, "ticket %d, the model expects slot %d" % (be.ticket(h), e.slot)
            self.handles[i] = (op, h)
        elif k == "wait_async":
            rc = be.wait(d, self.handles[op.tid][1])
        elif k == "query_async":
            t0 = time.perf_counter()
            while True:
                rc = be.query(d, self.handles[op.tid][1])
                if rc != 1:
                    break
                assert time.perf_counter() - t0 < 60, "query_async still pending after 60 s"
        elif k in ("verify_device", "verify_pipelined", "sha256_device", "sign_device", "merkle_device", "pack_bits"):
            if k == "pack_bits":
                h = be.pack_bits(d, self.last_dev[d][1], op.n, op.stream)
            elif k == "verify_device":
                old = self.last_dev.get(d)
                h = be.verify_device(d, op.lo, op.n, op.stream, op.flags, op.get("shift", False))
                if old is not None and old[0] not in self.handles:
                    be.drop(old[1])       # checked already, kept only as the source of a pack_bits
                self.last_dev[d] = (i, h)
            elif k == "verify_pipelined":
                h = be.verify_pipelined(d, op.lo, op.n, op.flags)
            elif k == "sha256_device":
                h = be.sha256_device(d, op.lo, op.n, op.stream)
            elif k == "sign_device":
                h = be.sign_device(d, op.lo, op.n, signed(op.lo, op.n, op.seed)[0], op.stream)
            else:
                h = be.merkle_device(d, merkle_case(op.old, op.n), op.stream)
            self.handles[i] = (op, h)
            if k != "verify_pipelined" and not op.get("stream"):
                self.finish([i])
        elif k == "sync":
            be.stream_sync(op.stream)
        elif k == "expect_tables":
            ts = be.table_state(d)
            assert ts["policy"] == op.policy and (ts["large_bytes"] > 3 << 30) == op.large and \
                (not op.large or ts["large_failed"] == 0) and (op.get("compact") is None or
                                                               (ts["compact_bytes"] > 0) == op.compact), \
                "table_state %r where %r is expected" % (ts, op)
        elif k == "pipeline_sync":
            rc = be.lifecycle("pipeline_sync", d)
        elif k == "sha256_host":
            h = be.sha256_host(d, op.lo, op.n)
            self.check(i, op, h)
        elif k == "merkle_host":
            h = be.merkle_host(d, merkle_case(op.old, op.n), op.get("leaf", True), op.get("node", True))
            self.check(i, op, h)
        elif k == "prepare":
            rc = be.lifecycle("prepare", d, op.k, op.flags)
        elif k == "self_test":
            rc = be.lifecycle("self_test", d, op.families)
        elif k == "trim":
            rc = be.lifecycle("trim", d, op.keep)
        elif k == "release":
            rc = be.lifecycle("release", d)
            if rc == 0 and not t.get("idle"):
                self.release_checks(d, before[0])
        else:
            rc = be.lifecycle(k, d, op.value)
        assert rc == e.rc, "%r returned %d, the model expects %d" % (op, rc, e.rc)
        self.finish(e.handed)
        self.finish(e.pipe)
        self.finish(e.stream)
        after = self.snapshot(d)
        # -- invariants
        mem = after[1]
        assert mem["total"] == sum(v for f, v in mem.items() if f != "total"), "context_memory: %r" % mem
        if e.rc == E_BUSY:
            assert after == before, "EDV_E_BUSY changed something: %r -> %r" % (before, after)
        if k in ("trim", "release") and rc == 0 and not t.get("idle"):
            self.floor = [0] * self.devices        # the table sets are shared by the logical devices of a GPU
            if k == "trim" and op.keep == 0 and after[2]["policy"] in (TABLES_AUTO, TABLES_COMPACT):
                assert mem["total"] == mem["sb_tables"] + mem["signer_comb"], "after trim(0): %r" % mem
                assert m.signed or mem["signer_comb"] == 0
        assert mem["total"] >= self.floor[d], "context_memory total fell from %d to %d without a trim or release" % (
            self.floor[d], mem["total"])
        self.floor[d] = mem["total"]
        if e.noalloc:
            assert mem == before[1], "allocation after prepare%r: %r -> %r" % (m.prepared, before[1], mem)
            self.noalloc_checks += 1

    def release_checks(self, d, before_count):
        """after a release that returned 0: the context is gone; older tickets answer as settled"""
        be = self.be
        count, mem, tables = self.snapshot(d)
        assert count == before_count - 1, "context_count %d after release, %d before" % (count, before_count)
        assert all(v == 0 for v in mem.values()), "context_memory after release: %r" % mem
        assert tables["compact_bytes"] == 0 and tables["large_bytes"] == 0, "table_state after release: %r" % tables
        probes = self.model.trace[-1]["probes"]
        for j, op, h in self.settled.get(d, [])[-probes:] if probes else []:
            assert be.wait(d, h) == 0 and be.query(d, h) == 0, "ticket of operation %d not settled" % j
            self.check(j, op, h)     # accept is not rewritten


def run(ops, backend, devices=1, seed=None, complete=True):
    """Runs the operations; returns the runner (trace, counts).  A failure
    carries the seed, the operation index and the operations up to it."""
    r = Runner(backend, devices, seed)
    for op in ops:
        r.step(op)
    if complete:
        assert not r.handles, "outputs never checked: operations %r" % sorted(r.handles)
    return r


def trace_of(ops, devices=1):
    """the model's trace without running anything"""
    m = Model(devices)
    for i, op in enumerate(ops):
        m.apply(i, op)
    return m.trace


# ------------------------------------------------------------------ the generator
WEIGHTS = {"verify_sync": 8, "verify_async": 10, "wait_async": 5, "query_async": 4, "verify_device": 8, "sync": 4,
           "verify_pipelined": 5, "pipeline_sync": 3, "sha256_host": 2, "sha256_device": 2, "sign_device": 2,
           "merkle_host": 2, "merkle_device": 2, "pack_bits": 2, "prepare": 2, "self_test": 1, "trim": 6, "release": 1,
           "set_table_policy": 1, "set_chunk": 4, "set_latency_path": 3, "set_length_buckets": 2, "set_host_slices": 2}
FAMILY_KINDS = {"verify_sync": ("sync", "latency"), "verify_device": ("sync", "latency"), "verify_async": ("slots",),
                "verify_pipelined": ("pipe",), "merkle_host": ("merkle",), "merkle_device": ("merkle",)}


def generate(seed, steps):
    """A random sequence of `steps` operations (or one fewer) for one device:
    weights per kind, raised for kinds, setting values and buffer-family
    stages (use, trim below, use larger) the sequence has not covered yet.
    The large table policy is excluded and no batch reaches 65,536.  It ends
    by handing over and syncing everything, then release."""
    rng = random.Random(seed)
    model = Model(1)
    m = model.dev[0]
    ops = []
    todo = set(KINDS) | {(k, v) for k, vs in SETTING_VALUES.items() for v in vs} | {("prepare", 0), ("prepare", 1)} | \
        {"noalloc_sync", "noalloc_async"}
    stage = {f: [0, 0] for f in FAMILIES}      # family -> [stage, n of the first use]
    released = False

    def closing():
        return len(m.slots) + bool(m.pipe) + sum(1 for s in model.streams.values() if s) + 1

    def lo_for(n):
        return rng.choice([0, 0, 1, 37, HEAD, 4099, POOL_N - n]) % (POOL_N - n + 1)

    def size_for(fams, sizes):
        for f in fams:
            if stage[f][0] == 2:
                big = [s for s in sizes if s > stage[f][1]]
                if big:
                    return rng.choice(big)
        for f in fams:
            if stage[f][0] == 0:
                mid = [s for s in sizes if 4096 < s <= 8193] or [s for s in sizes if 1 < s < max(sizes)]
                return rng.choice(mid)
        return rng.choice(sizes)

    def placeable(k):
        if k in ("wait_async", "query_async"):
            return bool(m.slots)
        if k == "sync":
            return not model.idle_streams()
        if k == "pack_bits":
            return m.last_dev is not None
        if k == "release":     # once in the middle, with room for operations of several kinds after it
            return not released and steps - len(ops) >= 16 and len(ops) >= steps // 3
        if k == "pipeline_sync":
            return bool(m.pipe) or "pipeline_sync" in todo
        return True

    def covered(k):
        """would a verify of this kind, placed now, be one the last prepare covers, with that still to be shown?"""
        if k == "verify_sync":
            return bool(m.prepared) and "noalloc_sync" in todo
        return k == "verify_async" and bool(m.prepared) and m.prepared[1] and "noalloc_async" in todo

    def value_for(k):
        left = [v for v in SETTING_VALUES[k] if (k, v) in todo]
        if k == "trim" and not m.busy():
            adv = [f for f in FAMILIES if stage[f][0] == 1]
            if adv and (not left or rng.random() < 0.6):
                return 0
        return rng.choice(left or SETTING_VALUES[k])

    def make(k):
        stream = rng.choice([None, "a", "b"])
        if k == "verify_sync":
            n = size_for(FAMILY_KINDS[k], SIZES)
            lo = lo_for(n)
            if covered(k):
                lo, n = 0, min(m.prepared[0], HEAD)      # the head averages 308 bytes: the prepare covers it
            return Op(k, lo=lo, n=n, mem=rng.choice(["pageable", "pinned1", "pinned3"]))
        if k == "verify_async":
            n = size_for(FAMILY_KINDS[k], SIZES)
            lo = lo_for(n)
            if covered(k):
                lo, n = 0, min(m.prepared[0], HEAD)
            dig = rng.random() < 0.5
            return Op(k, lo=lo, n=n, api="digest" if dig or rng.random() < 0.5 else "plain", digests=dig,
                      mem=rng.choice(["pageable", "pinned"]))
        if k in ("wait_async", "query_async"):
            return Op(k, tid=rng.choice(sorted(m.slots.values())))
        if k == "verify_device":
            n = size_for(FAMILY_KINDS[k], SIZES)
            flags, lo = rng.choice([0, 0, FLAG_BUCKETS, FLAG_UNIFORM_LENGTH]), lo_for(n)
            if flags == FLAG_UNIFORM_LENGTH:
                n = rng.choice([1, 16, 17])
                lo = UNIFORM_LO + rng.randrange(UNIFORM_N - n + 1)
            return Op(k, lo=lo, n=n, stream=stream, flags=flags, shift=rng.random() < 0.5)
        if k == "sync":
            return Op(k, stream=rng.choice([s for s, v in sorted(model.streams.items()) if v]))
        if k == "verify_pipelined":
            n = size_for(FAMILY_KINDS[k], SIZES)
            return Op(k, lo=lo_for(n), n=n, flags=rng.choice([0, FLAG_SPLIT_PREP]))
        if k in ("sha256_host", "sha256_device"):
            n = rng.choice(SIZES[:8])
            return Op(k, lo=lo_for(n), n=n, **({"stream": stream} if k == "sha256_device" else {}))
        if k == "sign_device":
            n = rng.choice(SIGN_SIZES)
            return Op(k, lo=lo_for(n), n=n, seed=rng.randrange(4), stream=stream)
        if k in ("merkle_host", "merkle_device"):
            n = size_for(("merkle",), MERKLE_SIZES)
            old = rng.choice([j for j, size in enumerate(mc.OLD_GRID) if size + n <= MERKLE_MAX_SIZE])
            if k == "merkle_host":
                return Op(k, old=old, n=n, leaf=rng.random() < 0.7, node=rng.random() < 0.7)
            return Op(k, old=old, n=n, stream=stream)
        if k == "pack_bits":
            return Op(k, lo=m.last_dev[1], n=m.last_dev[2], stream=stream)
        if k == "prepare":
            flags = rng.choice([f for f in (0, 1) if ("prepare", f) in todo] or [0, 1])
            return Op(k, k=rng.choice([1, HEAD, 400, 4097]), flags=flags)
        if k == "self_test":
            return Op(k, families=rng.choice([1, 2, 4, 7]))
        if k == "trim":
            return Op(k, keep=value_for(k))
        if k in ("release", "pipeline_sync"):
            return Op(k)
        return Op(k, value=value_for(k))

    def emit(op):
        i = len(ops)
        e = model.apply(i, op)
        ops.append(op)
        t = model.trace[-1]
        todo.discard(op.kind)
        todo.discard((op.kind, op.get("value", op.get("keep", op.get("flags")))))
        if t["noalloc"]:
            todo.discard("noalloc_sync" if op.kind == "verify_sync" else "noalloc_async")
        for f, n in t.get("use", ()):
            if stage[f][0] == 0:
                stage[f] = [1, n]
            elif stage[f][0] == 2 and n > stage[f][1]:
                stage[f][0] = 3
        if op.kind in ("trim", "release"):
            for f in FAMILIES:
                if stage[f][0] == 1 and freed_by(t, f, stage[f][1]):
                    stage[f][0] = 2
        return e

    def wanted(k):
        if k in todo or any(isinstance(x, tuple) and x[0] == k for x in todo) or covered(k):
            return True
        if any(stage[f][0] in (0, 2) for f in FAMILY_KINDS.get(k, ())):
            return True
        busy_seen = sum(1 for t in model.trace if t["rc"] == E_BUSY)
        if k == "trim":
            return (m.busy() and busy_seen < 2) or (not m.busy() and any(stage[f][0] == 1 for f in FAMILIES))
        if k in ("wait_async", "query_async", "pipeline_sync"):
            return m.busy() and busy_seen >= 2 and any(stage[f][0] == 1 for f in FAMILIES)
        return False

    while len(ops) + closing() + 3 < steps:
        kinds = [k for k in KINDS if placeable(k)]
        if len(m.slots) >= K_SLOTS and rng.random() < 0.7:
            kinds = [k for k in kinds if k != "verify_async"]
        need = [k for k in kinds if wanted(k)]
        if need and rng.random() < 0.85:
            kinds = need
        if not kinds:
            raise ValueError("seed %r: no operation can be placed at %d" % (seed, len(ops)))
        k = rng.choices(kinds, [WEIGHTS[x] for x in kinds])[0]
        if k in ("trim", "set_chunk", "prepare", "release"):
            # with the caller streams idle: what is queued there may still use the scratch these calls free
            for s_ in ("a", "b"):
                if model.streams[s_]:
                    emit(Op("sync", stream=s_))
        if k == "release":
            released = True
        emit(make(k))
    for j, tid in enumerate(sorted(m.slots.values())):
        emit(Op("wait_async" if j % 2 else "query_async", tid=tid))
    for s in ("a", "b"):
        if model.streams[s]:
            emit(Op("sync", stream=s))
    if m.pipe:
        emit(Op("pipeline_sync"))
    emit(Op("release", final=True))
    return ops


def replay(seed, upto, backend=None, steps=80):
    """The first `upto` operations of generate(seed, steps) alone, on the device
    unless a backend is given; outputs still in flight at the cut stay unchecked."""
    return run(generate(seed, steps)[:upto], backend or GpuBackend(), 1, seed, complete=False)


# ------------------------------------------------------------------ the device backend
class _Stream:
    """A caller-owned HIP stream of the runtime libedv.so uses, non-blocking:
    the backend's own synchronous copies do not order it."""
    _hip = None

    def __init__(self):
        if _Stream._hip is None:
            _Stream._hip = ctypes.CDLL("libamdhip64.so.7")
        self._s = ctypes.c_void_p()
        assert _Stream._hip.hipStreamCreateWithFlags(ctypes.byref(self._s), 1) == 0
        self.ptr = self._s.value

    def synchronize(self):
        assert _Stream._hip.hipStreamSynchronize(self._s) == 0


class _H:
    """buffers of one operation on the device backend"""

    def __init__(self, **kw):
        self.__dict__.update(kw)


class GpuBackend:
    """The C-ABI (edv.lib()) on device buffers and page-locked memory of the
    caller's own.  The pool is uploaded once and page-locked once, in the order
    msgs | offsets | keys | signatures (so a range of it is three regions, never
    one sigs | keys | offsets span); "pinned1" packs a range's signatures, keys
    and offsets into one region of its own."""

    def __init__(self):
        from indy_plenum_amd import edv
        self.edv, self.lib, self.p = edv, edv.lib(), pool()
        self.at = 0
        self.streams = {}
        p = self.p
        self.d = {}
        for name, a in (("sigs", p.sigs), ("pks", p.pks), ("msgs", p.msgs), ("off", p.off)):
            b = edv.DeviceBuffer(a.nbytes + 64)
            b.upload(a)
            self.d[name] = b
        pos, self.pin_at = 0, {}
        for name, a in (("msgs", p.msgs), ("off", p.off), ("pks", p.pks), ("sigs", p.sigs)):
            self.pin_at[name] = pos
            pos += (a.nbytes + 255) // 256 * 256
        self.pin = edv.PinnedBuffer(pos)
        for name, a in (("msgs", p.msgs), ("off", p.off), ("pks", p.pks), ("sigs", p.sigs)):
            self.pin.array[self.pin_at[name]:self.pin_at[name] + a.nbytes] = a.view(np.uint8)

    # -- helpers
    def stream(self, name):
        if name is None:
            return None
        if name not in self.streams:
            self.streams[name] = _Stream()
        return self.streams[name].ptr

    def dev_out(self, dev, nbytes, tail):
        b = self.edv.DeviceBuffer(nbytes + tail, dev)
        b.upload(np.full(nbytes + tail, SENT, np.uint8))
        return b

    def dev_in(self, dev, a):
        b = self.edv.DeviceBuffer(max(a.nbytes, 1) + 64, dev)
        if a.nbytes:
            b.upload(a)
        return b

    def host_out(self, nbytes, tail, pinned, keep):
        if pinned:
            pb = self.edv.PinnedBuffer(nbytes + tail)
            keep.append(pb)
            a = pb.array
        else:
            a = np.empty(nbytes + tail, np.uint8)
        a[:] = SENT
        return a

    def host_in(self, lo, n, mem, keep):
        """addresses of sigs, pks, msgs, off for requests [lo, lo + n)"""
        p = self.p
        if mem == "pageable":
            return (p.sigs[64 * lo:].ctypes.data, p.pks[32 * lo:].ctypes.data, p.msgs.ctypes.data,
                    p.off[lo:].ctypes.data)
        base = self.pin.ptr
        if mem in ("pinned", "pinned3"):
            return (base + self.pin_at["sigs"] + 64 * lo, base + self.pin_at["pks"] + 32 * lo,
                    base + self.pin_at["msgs"], base + self.pin_at["off"] + 8 * lo)
        assert mem == "pinned1"
        pb = self.edv.PinnedBuffer(104 * n + 8)
        keep.append(pb)
        pb.array[:64 * n] = p.sigs[64 * lo:64 * (lo + n)]
        pb.array[64 * n:96 * n] = p.pks[32 * lo:32 * (lo + n)]
        pb.array[96 * n:] = p.off[lo:lo + n + 1].view(np.uint8)
        return pb.ptr, pb.ptr + 64 * n, base + self.pin_at["msgs"], pb.ptr + 96 * n

    def ok(self, rc):
        if rc != 0:
            raise AssertionError("edv error %d: %s" % (rc, self.lib.edv_last_error().decode(errors="replace")))

    # -- state
    def context_count(self):
        return self.edv.context_count()

    def memory(self, dev):
        return self.edv.context_memory(dev)

    def table_state(self, dev):
        return self.edv.table_state(dev)

    def lifecycle(self, name, dev, *args):
        lib = self.lib
        if name in ("trim", "prepare", "self_test", "release", "pipeline_sync"):
            return getattr(lib, "edv_" + name)(dev, *args)
        rc = getattr(lib, "edv_" + name)(dev, *args)
        self.ok(rc)
        return rc

    # -- operations
    def verify_sync(self, dev, lo, n, mem):
        keep = []
        s, p, m, o = self.host_in(lo, n, mem, keep)
        acc = self.host_out(n, ROW, mem != "pageable", keep)
        self.ok(self.lib.edv_verify_batch(s, p, m, o, n, acc.ctypes.data, 1 << dev))
        return _H(host={"verdict": acc}, keep=keep)

    def submit_async(self, dev, lo, n, api, digests, mem):
        keep = []
        s, p, m, o = self.host_in(lo, n, mem, keep)
        acc = self.host_out(n, ROW, mem != "pageable", keep)
        out = {"verdict": acc}
        t = ctypes.c_int64(-1)
        if api == "plain":
            assert not digests
            self.ok(self.lib.edv_verify_batch_async(s, p, m, o, n, acc.ctypes.data, dev, ctypes.byref(t)))
        else:
            dig = self.host_out(32 * n, 32, mem != "pageable", keep) if digests else None
            if digests:
                out["digest"] = dig
            self.ok(self.lib.edv_verify_digest_batch_async(s, p, m, o, n, acc.ctypes.data,
                                                           dig.ctypes.data if digests else None, dev, ctypes.byref(t)))
        return _H(host=out, keep=keep, t=t.value)

    def ticket(self, h):
        return h.t

    def wait(self, dev, h):
        return self.lib.edv_wait_async(dev, h.t)

    def query(self, dev, h):
        return self.lib.edv_query_async(dev, h.t)

    def dev_ptrs(self, lo, shift):
        base = int(self.p.off[lo]) if shift else 0     # d_msgs moved on, msg_base says by how much
        return (self.d["sigs"].ptr + 64 * lo, self.d["pks"].ptr + 32 * lo, self.d["msgs"].ptr + base,
                self.d["off"].ptr + 8 * lo, base)

    def verify_device(self, dev, lo, n, stream, flags, shift):
        s, p, m, o, base = self.dev_ptrs(lo, shift)
        acc = self.dev_out(dev, n, ROW)
        self.ok(self.lib.edv_verify_batch_dev_flags(s, p, m, o, base, n, acc.ptr, dev, self.stream(stream), flags))
        return _H(dev={"verdict": acc}, acc=acc)

    def verify_pipelined(self, dev, lo, n, flags):
        s, p, m, o, base = self.dev_ptrs(lo, n % 2 == 1)
        acc = self.dev_out(dev, n, ROW)
        self.ok(self.lib.edv_verify_batch_dev_pipelined(s, p, m, o, base, n, acc.ptr, dev, flags))
        return _H(dev={"verdict": acc})

    def sha256_host(self, dev, lo, n):
        out = np.full(32 * n + 32, SENT, np.uint8)
        self.ok(self.lib.edv_sha256_batch(self.p.msgs.ctypes.data, self.p.off[lo:].ctypes.data, n, out.ctypes.data,
                                          1 << dev))
        return _H(host={"digest": out})

    def sha256_device(self, dev, lo, n, stream):
        _s, _p, m, o, base = self.dev_ptrs(lo, n % 2 == 0)
        out = self.dev_out(dev, 32 * n, 32)
        self.ok(self.lib.edv_sha256_batch_dev(m, o, base, n, out.ptr, dev, self.stream(stream)))
        return _H(dev={"digest": out})

    def sign_device(self, dev, lo, n, seeds, stream):
        _s, _p, m, o, base = self.dev_ptrs(lo, False)
        d_seeds = self.dev_in(dev, seeds)
        pks, sigs, acc = self.dev_out(dev, 32 * n, 32), self.dev_out(dev, 64 * n, 32), self.dev_out(dev, n, ROW)
        st = self.stream(stream)
        self.ok(self.lib.edv_sign_batch_dev(d_seeds.ptr, m, o, base, n, pks.ptr, sigs.ptr, dev, st))
        self.ok(self.lib.edv_verify_batch_dev_flags(sigs.ptr, pks.ptr, m, o, base, n, acc.ptr, dev, st, 0))
        return _H(dev={"key": pks, "signature": sigs, "verdict": acc}, keep=[d_seeds])

    def merkle_host(self, dev, c, leaf, node):
        n, old = c["n"], c["old"]
        out = {"frontier": np.full(c["new"].size + 32, SENT, np.uint8), "root": np.full(64, SENT, np.uint8)}
        if leaf:
            out["leaf"] = np.full(c["leaf"].size + 32, SENT, np.uint8)
        if node:
            out["node"] = np.full(c["node"].size + 32, SENT, np.uint8)
        fr = c["frontier"]
        self.ok(self.lib.edv_merkle_extend(old, fr.ctypes.data if fr.size else None, c["blob"].ctypes.data,
                                           c["off"].ctypes.data, n, out["leaf"].ctypes.data if leaf else None,
                                           out["node"].ctypes.data if node else None, out["frontier"].ctypes.data,
                                           out["root"].ctypes.data, dev))
        return _H(host=out)

    def merkle_device(self, dev, c, stream):
        ins = [self.dev_in(dev, c["frontier"]), self.dev_in(dev, c["blob"]), self.dev_in(dev, c["off"])]
        out = {"leaf": self.dev_out(dev, c["leaf"].size, 32), "node": self.dev_out(dev, c["node"].size, 32),
               "frontier": self.dev_out(dev, c["new"].size, 32), "root": self.dev_out(dev, 32, 32)}
        self.ok(self.lib.edv_merkle_extend_dev(c["old"], ins[0].ptr if c["frontier"].size else None, ins[1].ptr,
                                               ins[2].ptr, 0, c["n"], out["leaf"].ptr, out["node"].ptr,
                                               out["frontier"].ptr, out["root"].ptr, dev, self.stream(stream)))
        return _H(dev=out, keep=ins)

    def pack_bits(self, dev, src, n, stream):
        bits = self.dev_out(dev, (n + 7) // 8, ROW)
        self.ok(self.lib.edv_pack_bits_dev(src.acc.ptr, n, bits.ptr, dev, self.stream(stream)))
        return _H(dev={"bitmask": bits})

    def stream_sync(self, name):
        self.streams[name].synchronize()

    def read(self, h):
        if hasattr(h, "host"):
            return h.host
        return {k: b.download() for k, b in h.dev.items()}

    def drop(self, h):
        for b in list(getattr(h, "dev", {}).values()) + list(getattr(h, "keep", [])):
            b.free()
        h.__dict__.clear()


# ------------------------------------------------------------------ the directed sequences
class Seq(list):
    def add(self, kind, **p):
        self.append(Op(kind, **p))
        return len(self) - 1

    def verify(self, route, n, lo=0, k=0, dev=0):
        """one batch through a verify route, handed over or synced at once"""
        if route in ("pageable", "pinned1", "pinned3"):
            self.add("verify_sync", lo=lo, n=n, mem=route, dev=dev)
        elif route == "async":
            t = self.add("verify_async", lo=lo, n=n, api="digest", digests=k % 2 == 0,
                         mem="pinned" if k % 2 else "pageable", dev=dev)
            self.add("query_async" if k % 2 else "wait_async", tid=t, dev=dev)
        elif route == "device":
            self.add("verify_device", lo=lo, n=n, stream=None, flags=FLAG_BUCKETS if k % 3 == 2 else 0,
                     shift=k % 2 == 1, dev=dev)
        elif route == "stream":
            self.add("verify_device", lo=lo, n=n, stream="a", flags=0, shift=k % 2 == 1, dev=dev)
            self.add("sync", stream="a", dev=dev)
        else:
            assert route == "pipelined"
            self.add("verify_pipelined", lo=lo, n=n, flags=FLAG_SPLIT_PREP if k % 2 else 0, dev=dev)
            self.add("pipeline_sync", dev=dev)


def ladder(route):
    """n ascending through the thresholds on one route, chunks 256 -> default ->
    1,024 -> 256 between (the scratch above the chunk, below the need, regrown),
    trims, and both latency limits"""
    q = Seq()
    q.add("set_latency_path", value=4096)
    steps = ((256, SIZES[:6]), (0, SIZES[6:10]), (1024, SIZES[10:12]), (256, SIZES[12:]))
    k = 0
    for chunk, sizes in steps:
        q.add("set_chunk", value=chunk)
        for n in sizes:
            q.verify(route, n, lo=(0, 37, HEAD)[k % 3] if n < POOL_N - HEAD else 0, k=k)
            k += 1
    q.add("trim", keep=20000)
    q.add("trim", keep=400)
    q.verify(route, SIZES[-1], k=1)
    q.verify(route, SIZES[0], lo=5, k=2)
    q.add("trim", keep=1)
    q.add("trim", keep=0)
    q.verify(route, SIZES[-1], k=3)
    q.add("set_latency_path", value=K_QUAD_DEFAULT)
    q.add("set_chunk", value=0)
    for n in (17, 4097, 16384, 16385, 20000):
        q.verify(route, n, lo=POOL_N - n, k=k)
        k += 1
    q.add("release", final=True)
    return q


SLOT_SIZES = (1, 8193, 17, 4097, 8192, 400, 16384, 257)


def slots():
    q = Seq()
    q.add("set_latency_path", value=4096)      # 1, 17, 400, 257 latency; 4,097, 8,192 own stream; 8,193, 16,384 shared
    t = [q.add("verify_async", lo=(0, 37)[k % 2], n=n, api="digest", digests=k % 2 == 1,
               mem="pageable" if k % 2 else "pinned") for k, n in enumerate(SLOT_SIZES)]
    q.add("trim", keep=0)
    q.add("release")
    for k, j in enumerate((3, 0, 7, 5, 1, 2, 6)):
        q.add("wait_async" if k % 2 == 0 else "query_async", tid=t[j])
        if k in (1, 6):
            q.add("trim", keep=400)
            q.add("release")
    q.add("query_async", tid=t[4])
    q.add("trim", keep=400)
    q.add("set_latency_path", value=K_QUAD_DEFAULT)
    swapped = [SLOT_SIZES[k ^ 1] for k in range(8)]     # the slot that held 8,193 gets 1, and the other way round
    t = [q.add("verify_async", lo=(64, 1)[k % 2], n=n, api="digest", digests=k % 2 == 0,
               mem="pinned" if k % 2 else "pageable") for k, n in enumerate(swapped)]
    for j in t:
        q.add("wait_async", tid=j)
    # the two-walk kernel's table scratch of slots 0, 2, 5, 7 goes, then comes back smaller (slots 0, 7: a kept
    # capacity would pass for enough) and larger (slot 2: sized for 4,097, met by 16,384)
    q.add("trim", keep=400)
    t = [q.add("verify_async", lo=(37, 0)[k % 2], n=n, api="digest", digests=k % 2 == 1,
               mem="pinned" if k % 2 else "pageable") for k, n in enumerate((4097, 1, 16384, 17, 400, 8193, 257, 8192))]
    for k, j in enumerate(reversed(t)):
        q.add("query_async" if k % 2 else "wait_async", tid=j)
    q.add("prepare", k=400, flags=PREPARE_ASYNC)
    for k in range(8):                          # ranges that average at most 512 bytes: nothing may be allocated
        j = q.add("verify_async", lo=(0, 1, UNIFORM_LO, 3)[k % 4], n=(17, 16, 1, 12)[k % 4], api="digest",
                  digests=k % 2 == 0, mem="pinned" if k % 2 else "pageable")
        q.add("wait_async" if k % 2 else "query_async", tid=j)
    for mem in ("pageable", "pinned1", "pinned3"):
        q.add("verify_sync", lo=0, n=HEAD, mem=mem)
    # buffers sized for exactly k: after trim(0), prepare(64, ASYNC) and then the 64 requests of the pool's head
    # (308 bytes on average) through all eight slots and the synchronous call, on the latency kernels and on the
    # batch kernels (the slot's own scratch, c.st)
    for limit in (K_QUAD_DEFAULT, 0):
        q.add("set_latency_path", value=limit)
        q.add("trim", keep=0)
        q.add("prepare", k=HEAD, flags=PREPARE_ASYNC)
        for k in range(8):
            j = q.add("verify_async", lo=0, n=HEAD, api="digest", digests=k % 2 == 0,
                      mem="pinned" if k % 2 else "pageable")
            q.add("wait_async" if k % 2 else "query_async", tid=j)
        for mem in ("pageable", "pinned1", "pinned3"):
            q.add("verify_sync", lo=0, n=HEAD, mem=mem)
        q.add("verify_sync", lo=UNIFORM_LO, n=17, mem="pageable")
    q.add("set_latency_path", value=K_QUAD_DEFAULT)
    q.add("release", final=True)
    return q


def pipelined():
    q = Seq()
    for flags in (0, FLAG_SPLIT_PREP):
        for buckets in (0, 1):
            q.add("set_length_buckets", value=buckets)
            for chunk, sizes in ((1024, (4097, 257, 8193)), (256, (8192, 1, 16385))):
                q.add("set_chunk", value=chunk)
                for k, n in enumerate(sizes):
                    q.add("verify_pipelined", lo=(0, 37, HEAD)[k], n=n, flags=flags)
                q.add("pipeline_sync")
            q.add("trim", keep=0)
            q.add("verify_pipelined", lo=1, n=4096, flags=flags)
            q.add("verify_pipelined", lo=UNIFORM_LO, n=17, flags=flags)
            q.add("pipeline_sync")
            q.add("set_chunk", value=0)
            q.add("verify_pipelined", lo=0, n=POOL_N, flags=flags)
            q.add("pipeline_sync")
    q.add("set_length_buckets", value=2)
    q.add("release", final=True)
    return q


def two_streams():
    q = Seq()
    for _round in range(2):
        q.add("merkle_device", old=4, n=257, stream="a")
        q.add("verify_device", lo=37, n=300, stream="a", flags=0, shift=True)
        q.add("pack_bits", lo=37, n=300, stream="b")              # stream a's verdicts, packed on stream b
        q.add("sign_device", lo=64, n=256, seed=1, stream="a")
        q.add("verify_device", lo=0, n=POOL_N, stream="b", flags=0, shift=False)   # grow_state with a's launches queued
        q.add("sha256_device", lo=1, n=4097, stream="a")
        q.add("merkle_device", old=8, n=66000, stream="a")
        q.add("merkle_device", old=13, n=257, stream="b")
        q.add("sync", stream="a")
        q.add("sync", stream="b")
        if _round == 0:
            q.add("trim", keep=0)
    q.add("release", final=True)
    return q


def every_kind(q, k):
    for route, n in (("pageable", 257), ("pinned1", 4097), ("async", 400), ("stream", 8193), ("pipelined", 8192)):
        q.verify(route, n, lo=37, k=k)
    t = q.add("verify_async", lo=0, n=8193, api="plain", digests=False, mem="pinned")
    q.add("query_async", tid=t)
    q.add("verify_device", lo=HEAD, n=4097, stream=None, flags=0, shift=False)
    q.add("pack_bits", lo=HEAD, n=4097, stream=None)
    q.add("sha256_host", lo=0, n=257)
    q.add("sha256_device", lo=37, n=256, stream="b")
    q.add("sign_device", lo=0, n=256, seed=2, stream=None)
    q.add("verify_device", lo=UNIFORM_LO, n=17, stream=None, flags=FLAG_UNIFORM_LENGTH, shift=False)
    q.add("merkle_host", old=6, n=257, leaf=k != 0, node=k != 1)      # null leaf_hashes, then null node_hashes
    q.add("merkle_device", old=9, n=1000, stream="b")
    q.add("sync", stream="b")
    q.add("prepare", k=400, flags=0)
    q.add("verify_sync", lo=0, n=HEAD, mem="pageable")        # covered by the prepare: nothing may be allocated
    q.add("verify_sync", lo=0, n=HEAD, mem="pinned1")
    q.add("verify_sync", lo=UNIFORM_LO, n=17, mem="pinned3")
    q.add("self_test", families=7)
    for kind, value in (("set_chunk", (1024, 4096)), ("set_latency_path", (4096, 0)), ("set_length_buckets", (1, 0)),
                        ("set_host_slices", (2, 8)), ("set_table_policy", (TABLES_COMPACT, TABLES_AUTO))):
        q.add(kind, value=value[k])
    q.verify("pageable", 8193, k=k)
    q.add("trim", keep=(400, 4097)[k])


def release_in_the_middle():
    q = Seq()
    every_kind(q, 0)
    q.add("release")
    every_kind(q, 1)
    for kind in ("set_chunk", "set_length_buckets", "set_host_slices", "set_table_policy"):
        q.add(kind, value=2 if kind == "set_length_buckets" else 0)
    q.add("set_latency_path", value=K_QUAD_DEFAULT)
    q.add("release", final=True)
    return q


def table_rotation():
    q = Seq()

    def routes():
        k = 0
        for limit in (K_QUAD_DEFAULT, 0):
            q.add("set_latency_path", value=limit)
            for n in (257, 4097):
                for route in ("pageable", "async", "stream", "pipelined"):
                    q.verify(route, n, lo=(0, 37)[k % 2], k=k)
                    k += 1
            # one SHA-512 block count over the range: no length buckets on the batch kernels (limit 0)
            q.add("verify_device", lo=UNIFORM_LO, n=UNIFORM_N, stream=None, flags=FLAG_UNIFORM_LENGTH, shift=limit == 0)
    q.add("set_table_policy", value=TABLES_COMPACT)
    routes()
    q.add("expect_tables", policy=TABLES_COMPACT, large=False, compact=True)
    q.add("set_table_policy", value=TABLES_LARGE)
    routes()
    q.add("expect_tables", policy=TABLES_LARGE, large=True)
    q.add("set_table_policy", value=TABLES_AUTO)
    q.add("trim", keep=400)
    q.add("expect_tables", policy=TABLES_AUTO, large=False, compact=True)
    routes()
    q.add("expect_tables", policy=TABLES_AUTO, large=False, compact=True)
    q.add("set_table_policy", value=TABLES_LARGE)
    routes()
    q.add("expect_tables", policy=TABLES_LARGE, large=True)
    q.add("set_table_policy", value=TABLES_COMPACT)
    q.add("trim", keep=0)
    q.add("expect_tables", policy=TABLES_COMPACT, large=False)
    routes()
    q.add("expect_tables", policy=TABLES_COMPACT, large=False, compact=True)
    q.add("set_latency_path", value=K_QUAD_DEFAULT)
    q.add("release", final=True)
    return q


def two_devices():
    q = Seq()
    for k, (route, n) in enumerate((("pageable", 257), ("pinned3", 4097), ("async", 400), ("device", 8193),
                                    ("pipelined", 4097), ("stream", 16385))):
        q.verify(route, n, lo=37, k=k, dev=k % 2)
    t0 = q.add("verify_async", lo=0, n=400, api="digest", digests=True, mem="pageable", dev=0)
    q.add("wait_async", tid=t0, dev=0)
    t1 = q.add("verify_async", lo=0, n=8193, api="digest", digests=True, mem="pinned", dev=1)
    q.add("release", dev=0)                     # device 1's ticket is outstanding: the BUSY rule is per device
    q.add("wait_async", tid=t1, dev=1)
    q.verify("pageable", 257, k=0, dev=0)       # device 0 recreated by use
    q.verify("async", 4097, k=1, dev=0)
    q.add("trim", keep=0, dev=1)
    for k, dev in enumerate((0, 1, 1, 0)):
        q.verify(("pageable", "async", "device", "pipelined")[k], (8193, 257, 20000, 257)[k], k=k, dev=dev)
    q.add("release", dev=1, final=True)
    q.add("release", dev=0, final=True)
    return q


LADDER_ROUTES = ("pageable", "pinned3", "async", "device", "pipelined")
# name -> (operations, logical devices, environment of the child process)
DIRECTED = {"ladder_" + r: (lambda r=r: ladder(r), 1, {}) for r in LADDER_ROUTES}
DIRECTED.update({
    "slots": (slots, 1, {}),
    "pipelined": (pipelined, 1, {}),
    "two_streams": (two_streams, 1, {}),
    "release_in_the_middle": (release_in_the_middle, 1, {}),
    "table_rotation": (table_rotation, 1, {}),
    "two_devices": (two_devices, 2, {"EDV_VIRTUAL_DEVICES": "2"}),
})
SEEDS = (41, 42, 65)
STEPS = 80


def sequence(name):
    """(operations, devices, seed) of a directed sequence, or of random_<seed>"""
    if name.startswith("random_"):
        seed = int(name[7:])
        return generate(seed, STEPS), 1, seed
    make, devices, _env = DIRECTED[name]
    return make(), devices, None


HIP_FAULT_STATUS = 86
HIP_FAULT_WORDS = ("edv error -3", "returned -3", "illegal memory access", "hipError", "HSA_STATUS_ERROR")


def child_main(name, upto=None):
    """one sequence on the device, in a process of its own; prints one JSON line"""
    import json
    t0 = time.perf_counter()
    ops, devices, seed = sequence(name)
    p = pool()
    t1 = time.perf_counter()
    try:
        r = run(ops if upto is None else ops[:upto], GpuBackend(), devices, seed, complete=upto is None)
    except SequenceFailure as ex:
        if any(w in str(ex) for w in HIP_FAULT_WORDS):
            import sys
            import traceback
            traceback.print_exc()
            sys.stderr.flush()
            import os
            os._exit(HIP_FAULT_STATUS)      # EDV_E_HIP or a HIP fault: the card may be in a bad way
        raise
    print(json.dumps({"name": name, "operations": len(r.ops), "comparisons": r.comparisons,
                      "noalloc_checks": r.noalloc_checks, "references_s": round(p.build_seconds, 2),
                      "run_s": round(time.perf_counter() - t1, 2), "total_s": round(time.perf_counter() - t0, 2)}))
