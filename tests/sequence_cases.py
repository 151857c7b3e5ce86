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

The batched append and the proof verification (edv_merkle_append_batch[_dev],
edv_merkle_verify_inclusion / _consistency[_dev]) are operations too:
append_host / append_device (per-leaf roots, packed paths, leaf and node hashes,
frontier and root against merkle_append_cases.simulate_appends and
merkle_cases.simulate; offsets from path_entries), verify_incl_* / verify_cons_*
(statuses and calculated roots against merkle_verify_cases' checker, batches
from its synthesiser with every status in each) and chain_append / chain_verify,
a ledger that stays on the device: each append's d_old_hashes is the frontier
buffer the append before it wrote, each verify reads the append's path and
per-leaf root buffers as they are, and a consistency proof from the size before
(built here with hashlib, _Tree) is verified against the root buffers of both
appends.  The model books the fifteen Merkle buffers of a context byte for
byte (merkle_needs, merkle_trim_limits, MerkleBufs: what the runtime's ensure
calls and trim_buffers compute from the same arguments): across every Merkle
operation edv_context_memory's chunk_scratch moves by exactly what the model's
buffers grow, and the device verify forms leave context_memory as it was.

The comb table of the signer is not a buffer edv_trim frees (include/edv.h), so
"after trim(0) the total is the table set's" is checked as total == sb_tables +
signer_comb, with signer_comb == 0 unless a signing ran since the last release.
"""
import ctypes
import hashlib
import random
import time

import numpy as np

import merkle_append_cases as ac
import merkle_cases as mc
import merkle_verify_cases as vc
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
# the batched append and the proof verification (their own grids: merkle_append_cases, merkle_verify_cases)
APPEND_SIZES = (1, 63, 64, 65, 257, 1000, 66000)     # 63..65: the append kernel's 64-lane workgroup; 66,000: three passes
APPEND_OLD = (0, 255, 256, 65535, 2 ** 32 - 1, 2 ** 62 - 600)      # sizes of merkle_append_cases.OLD_GRID
PROOF_SIZES = (1, 63, 64, 65, 257, 4097)
PATHS_LIMIT = 32 << 20                      # the packed paths of a 66,000-leaf append stay below this
BIG_BASE = 2 ** 32 + 2 ** 20 + 24           # a device form's base above 2^32, as test_bases_above_2_32
NEW_KINDS = ("append_host", "append_device", "verify_incl_host", "verify_incl_device", "verify_cons_host",
             "verify_cons_device", "chain_append", "chain_verify")
APPEND_FLAGS = ("roots", "paths", "leaf", "node")
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


def _u8(b):
    return np.frombuffer(bytes(b), np.uint8)


def _spent(t0):
    """seconds the references of the batched append and the proof verification took in this process"""
    _cache["merkle_seconds"] = merkle_seconds() + time.perf_counter() - t0


def merkle_seconds():
    return _cache.get("merkle_seconds", 0.0)


def merkle_inputs(old_index, n, grid=mc.OLD_GRID, seed=0x5EC):
    """old size (an index into `grid`), frontier, leaves (16 bytes each at 66,000): the inputs alone, nothing hashed"""
    key = ("merkle_in", old_index, n, seed)
    if key not in _cache:
        old = grid[old_index]
        assert old + n <= MERKLE_MAX_SIZE
        fr = mc.frontier(seed, old)
        leaves = mc.leaves_of(seed + old_index, n, lengths=[16]) if n == 66000 else mc.leaves_of(seed + old_index, n)
        blob, off = mc.pack(leaves)
        _cache[key] = {"old": old, "n": n, "fr": fr, "leaves": leaves, "frontier": _u8(b"".join(fr)), "blob": blob,
                       "off": off, "mbytes": int(off[-1]), "nodes": mc.node_span(old, n)}
    return _cache[key]


def merkle_case(old_index, n):
    """merkle_inputs over merkle_cases.OLD_GRID with merkle_cases.simulate's outputs"""
    key = ("merkle", old_index, n)
    if key not in _cache:
        c = dict(merkle_inputs(old_index, n))
        lh, nodes, new, root = mc.simulate(c["old"], c["fr"], c["leaves"])
        assert len(nodes) == 32 * c["nodes"]
        c.update(leaf=_u8(lh), node=_u8(nodes), new=_u8(b"".join(new)), root=_u8(root))
        _cache[key] = c
    return _cache[key]


def append_inputs(old_index, n):
    """the inputs of a batched append: old size merkle_append_cases.OLD_GRID[old_index]; `entries` is the packed
    paths' length by merkle_append_cases.path_entries (Python integers), never the library's count"""
    key = ("append_in", old_index, n)
    if key not in _cache:
        old = ac.OLD_GRID[old_index]
        assert old in APPEND_OLD and n in APPEND_SIZES, (old, n)
        c = dict(merkle_inputs(old_index, n, ac.OLD_GRID, 0xA90))
        c["entries"] = ac.path_entries(old, n)
        if n == 66000:      # only onto an old size whose popcounts keep the packed paths small
            assert 32 * c["entries"] < PATHS_LIMIT, "66,000 leaves onto %d: %d path entries" % (old, c["entries"])
        _cache[key] = c
    return _cache[key]


def append_case(old_index, n):
    """append_inputs with what merkle_cases.simulate and merkle_append_cases.simulate_appends (hashlib) give: leaf
    and node hashes, the new frontier, the root, the per-leaf roots and the packed audit paths"""
    key = ("append", old_index, n)
    if key not in _cache:
        t0 = time.perf_counter()
        c = dict(append_inputs(old_index, n))
        lh, nodes, new, root = mc.simulate(c["old"], c["fr"], c["leaves"])
        roots, paths = ac.simulate_appends(c["old"], c["fr"], c["leaves"])
        assert roots[-1] == root and len(nodes) == 32 * c["nodes"]
        assert [len(p) for p in paths] == [mc.popcount(c["old"] + i) for i in range(n)]
        packed = ac.packed(paths)
        assert len(packed) == 32 * c["entries"]
        c.update(leaf=_u8(lh), node=_u8(nodes), new=_u8(b"".join(new)), root=_u8(root), roots=_u8(b"".join(roots)),
                 paths=_u8(packed))
        _cache[key] = c
        _spent(t0)
    return _cache[key]


INCLUSION_STATUSES = {vc.OK, vc.RANGE, vc.SHORT, vc.LONG, vc.ROOT}
CONSISTENCY_STATUSES = {vc.OK, vc.RANGE, vc.SHORT, vc.ROOT, vc.INCONSISTENT}


def proof_case(kind, n, seed):
    """n proofs of merkle_verify_cases' synthesiser over its grids (tree sizes up to 2^64 - 1), mutated, with the
    checker's statuses and calculated roots.  A batch of at least MUTATIONS proofs holds every status the
    synthesiser can produce (asserted here); a single proof is mutation 0, intact."""
    key = ("proof", kind, n, seed)
    if key not in _cache:
        t0 = time.perf_counter()
        assert n in PROOF_SIZES
        if kind == "incl":
            pts = vc.inclusion_points()
            b = vc.synth_inclusion([pts[(7 * k + seed) % len(pts)] for k in range(n)], seed=seed)
            every = INCLUSION_STATUSES
        else:
            pts = vc.consistency_points()
            b = vc.synth_consistency([pts[(3 * k + seed) % len(pts)] for k in range(n)], seed=seed)
            every = CONSISTENCY_STATUSES
        st, comp = b.expected()
        assert set(st) == (every if n >= vc.MUTATIONS else {vc.OK}), "%s batch n=%d seed=%d: statuses %s" % (
            kind, n, seed, sorted(set(st)))
        _cache[key] = {"kind": kind, "n": n, "batch": b, "status": _u8(st), "computed": _u8(comp),
                       "entries": sum(len(p) for p in b.proof),
                       "lbytes": sum(len(x) for x in b.leaves) if kind == "incl" else 0}
        _spent(t0)
    return _cache[key]


# -- the chained ledger: one tree from size 0, grown by the pool's bytes
def chain_leaves(start, n):
    """(first request of the pool or None, leaves): n == 66,000 takes 16-byte slices of the pool's messages from
    byte 0, every other n the messages of the n requests from (7 * start) mod (POOL_N - n + 1) on"""
    p = pool()
    if n == 66000:
        return None, [p.blob[16 * i:16 * i + 16] for i in range(n)]
    lo = (7 * start) % (POOL_N - n + 1)
    return lo, [p.message(lo + i) for i in range(n)]


def _largest_pow2_below(n):
    return 1 << ((n - 1).bit_length() - 1)


class _Tree:
    """RFC 6962 over the leaf hashes of the whole history, in hashlib: complete subtrees by level, MTH of any
    range, the frontier of any size and PROOF(m, D[n]) (section 2.1.2), independent of the package's merkle.py"""

    def __init__(self, leaf_hashes):
        self.levels = [leaf_hashes]
        while len(self.levels[-1]) > 1:
            lv = self.levels[-1]
            self.levels.append([mc.node_hash(lv[i], lv[i + 1]) for i in range(0, len(lv) - 1, 2)])

    def mth(self, a, b):
        n = b - a
        if n & (n - 1) == 0 and a % n == 0:
            return self.levels[n.bit_length() - 1][a // n]
        k = _largest_pow2_below(n)
        return mc.node_hash(self.mth(a, a + k), self.mth(a + k, b))

    def frontier(self, size):
        out, pos = [], 0
        for b in range(size.bit_length() - 1, -1, -1):
            if (size >> b) & 1:
                out.append(self.levels[b][pos >> b])
                pos += 1 << b
        return out

    def proof(self, m, n):
        def sub(m, a, b, whole):
            if m == b - a:
                return [] if whole else [self.mth(a, b)]
            k = _largest_pow2_below(b - a)
            if m <= k:
                return sub(m, a, a + k, whole) + [self.mth(a + k, b)]
            return sub(m - k, a + k, b, False) + [self.mth(a, a + k)]
        return sub(m, 0, n, True) if 0 < m < n else []


def chain_reference(ns):
    """The chained ledger's history: one merkle_append_cases.simulate_appends run (and one merkle_cases.simulate
    run, for the leaf and node hashes) over all sum(ns) leaves from size 0.  Returns one record per step: its
    slices of the roots, paths, leaf and node hashes, the frontier and root after it, the offsets of its paths
    (prefix sums of popcounts, in Python) and the consistency proof from the size before it, built by _Tree."""
    key = ("chain", tuple(ns))
    if key not in _cache:
        t0 = time.perf_counter()
        steps, start, leaves = [], 0, []
        for n in ns:
            lo, lv = chain_leaves(start, n)
            steps.append({"start": start, "n": n, "lo": lo})
            leaves += lv
            start += n
        roots, paths = ac.simulate_appends(0, [], leaves)
        lh, nodes, _new, root = mc.simulate(0, [], leaves)
        assert roots[-1] == root
        tree = _Tree([lh[i:i + 32] for i in range(0, len(lh), 32)])
        for st in steps:
            a, n = st["start"], st["n"]
            b = a + n
            fr = tree.frontier(b)
            assert mc.fold(fr) == roots[b - 1], "the level tree and simulate_appends disagree at size %d" % b
            proof = tree.proof(a, b)
            old_root = roots[a - 1] if a else mc.EMPTY_ROOT
            status, computed = vc.check_consistency(a, b, old_root, roots[b - 1], proof)
            assert status == vc.OK and len(proof) == (vc.consistency_length(a, b) if a else 0)
            poff = np.zeros(n + 1, np.uint64)
            poff[1:] = np.cumsum([mc.popcount(a + i) for i in range(n)], dtype=np.uint64)
            n0, n1 = mc.node_span(0, a), mc.node_span(0, b)
            st.update(size=b, old_frontier=_u8(b"".join(tree.frontier(a))), roots=_u8(b"".join(roots[a:b])), paths=_u8(ac.packed(paths[a:b])),
                      leaf=_u8(lh[32 * a:32 * b]), node=_u8(nodes[32 * n0:32 * n1]), nodes=n1 - n0,
                      frontier=_u8(b"".join(fr)), root=_u8(roots[b - 1]), old_root=_u8(old_root), proof=proof,
                      poff=poff, entries=int(poff[-1]), cstatus=_u8(bytes([status])), ccomputed=_u8(computed),
                      leaves=leaves[a:b])
            assert st["paths"].size == 32 * st["entries"]
        _cache[key] = steps
        _spent(t0)
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
    if k in ("append_host", "append_device"):
        c = append_case(op.old, op.n)
        out = {"frontier": c["new"], "root": c["root"]}
        out.update({name: c[name] for name in APPEND_FLAGS if op.p[name]})
        return out
    if k in ("verify_incl_host", "verify_incl_device", "verify_cons_host", "verify_cons_device"):
        if op.get("src") is not None:       # an append's own paths and roots: every proof good, its roots recomputed
            c = append_case(op.old, op.n)
            out = {"status": np.full(op.n, vc.OK, np.uint8), "computed": c["roots"]}
        else:
            c = proof_case("incl" if "incl" in k else "cons", op.n, op.seed)
            out = {"status": c["status"], "computed": c["computed"]}
        if not op.computed:
            del out["computed"]
        return out
    raise KeyError(k)


def chain_expect(op, step):
    """expected outputs of a chain_append / chain_verify at `step`, a record of chain_reference"""
    if op.kind == "chain_append":
        out = {name: step[name] for name in ("roots", "paths", "frontier", "root")}
        if op.keep_hashes:
            out.update(leaf=step["leaf"], node=step["node"])
        out.update(cstatus=step["cstatus"], ccomputed=step["ccomputed"])
        return out
    return {"status": np.full(step["n"], vc.OK, np.uint8), "computed": step["roots"], "cstatus": step["cstatus"]}


def tail_of(name):
    """sentinel bytes past an output: 16 past verdict and status rows, 32 past hash rows"""
    return ROW if name in ("verdict", "bitmask", "status", "cstatus") else 32


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


# -- the fifteen Merkle buffers of a context (MerkleBufs::bytes), as the runtime sizes and trims them
K_MERKLE_LOG_T, K_MERKLE_MAX_HASHES, K_READ_SLACK, K_TRIM_MSG_BYTES = 8, 63, 64, 4096
MERKLE_BUFFERS = ("mk_roots", "mk_leaves", "mk_off", "mk_hashes", "mk_leafh", "mk_nodeh", "mk_fleafh", "mk_fnodeh",
                  "mk_aroots", "mk_paths", "mv_leaves", "mv_words", "mv_roots", "mv_proofs", "mv_out")
# the three sub-families whose capacities the coverage conditions follow: the device append's fold scratch, the
# host append's staging (shared with the host extend) and the host verify's staging
SUBFAMILIES = {"fold": ("mk_fleafh", "mk_fnodeh"), "stage": ("mk_leafh", "mk_nodeh", "mk_aroots", "mk_paths"),
               "mv": ("mv_leaves", "mv_words", "mv_roots", "mv_proofs", "mv_out")}


def merkle_scratch_bytes(old, new):
    """32 x merkle_scratch_hashes (edv_merkle.h): the tile roots every pass after the first reads"""
    def items(h):
        return (new >> h) - (old >> h) if h < 64 else 0
    t, h0 = 0, K_MERKLE_LOG_T
    while h0 < 64 and items(h0 + 1) != 0:
        t += items(h0)
        h0 += K_MERKLE_LOG_T
    return 32 * t


def merkle_needs(op, chain_step=None):
    """(buffer, bytes) for every DevBuf::ensure a Merkle operation reaches, computed from the call's arguments as
    run_merkle_host, launch_merkle and run_verify_*_host compute them.  The device verify forms reach none."""
    k = op.kind
    if k in ("merkle_host", "merkle_device", "append_host", "append_device", "chain_append"):
        if k == "chain_append":
            old, n, nodes = chain_step["start"], op.n, mc.node_span(chain_step["start"], op.n)
            flags = {"roots": True, "paths": True, "leaf": op.keep_hashes, "node": op.keep_hashes}
        else:
            c = append_inputs(op.old, op.n) if k.startswith("append") else merkle_inputs(op.old, op.n)
            old, n, nodes = c["old"], c["n"], c["nodes"]
            if k.startswith("append"):
                flags = {f: op.p[f] for f in APPEND_FLAGS}
            else:
                flags = {"roots": False, "paths": False, "leaf": op.get("leaf", True), "node": op.get("node", True)}
        per_leaf = flags["roots"] or flags["paths"]
        need = []
        if k in ("merkle_host", "append_host"):
            need += [("mk_leaves", c["mbytes"] + 64), ("mk_off", 8 * (n + 1)),
                     ("mk_hashes", 32 * (2 * K_MERKLE_MAX_HASHES + 2)),
                     ("mk_leafh", 32 * n if flags["leaf"] or per_leaf else 0),
                     ("mk_nodeh", 32 * nodes if flags["node"] or per_leaf else 0),
                     ("mk_aroots", 32 * n if flags["roots"] else 0),
                     ("mk_paths", 32 * c["entries"] if flags["paths"] else 0)]
            need.append(("mk_roots", merkle_scratch_bytes(old, old + n)))
        else:
            need += [("mk_roots", merkle_scratch_bytes(old, old + n)),
                     ("mk_fleafh", 32 * n if per_leaf and not flags["leaf"] else 0),
                     ("mk_fnodeh", 32 * nodes if per_leaf and not flags["node"] else 0)]
        return need
    if k in ("verify_incl_host", "verify_cons_host"):
        c = proof_case("incl" if "incl" in k else "cons", op.n, op.seed)
        n, comp = op.n, 1 if op.computed else 0
        proofs = ("mv_proofs", max(32 * c["entries"], 32))
        if k == "verify_incl_host":
            lbytes = 32 * n if op.by_hash else c["lbytes"]
            return [("mv_leaves", lbytes + K_READ_SLACK), ("mv_words", 8 * (4 * n + 2)), ("mv_roots", 32 * n),
                    ("mv_out", 32 * n * comp + n), proofs]
        return [("mv_words", 8 * (4 * n + 2)), ("mv_roots", 64 * n), ("mv_out", 64 * n * comp + n), proofs]
    return []


def merkle_trim_limits(k):
    """what trim_buffers lets each Merkle buffer keep for keep_batch k"""
    msgs = k * K_TRIM_MSG_BYTES + K_READ_SLACK if k else 0
    return {"mk_roots": 32 * (k // ((1 << K_MERKLE_LOG_T) - 1) + 16) if k else 0, "mk_leaves": msgs,
            "mk_off": 8 * (k + 1) if k else 0, "mk_hashes": 32 * (2 * K_MERKLE_MAX_HASHES + 2) if k else 0,
            "mk_leafh": 32 * k, "mk_nodeh": 32 * k, "mk_fleafh": 32 * k, "mk_fnodeh": 32 * k, "mk_aroots": 32 * k,
            "mk_paths": 32 * K_MERKLE_MAX_HASHES * k, "mv_leaves": msgs, "mv_words": 8 * (4 * k + 2) if k else 0,
            "mv_roots": 64 * k, "mv_proofs": 32 * 64 * k, "mv_out": 80 * k}


class MerkleBufs:
    """capacities of the fifteen buffers under DevBuf::ensure, trim_buffers and ctx_destroy"""

    def __init__(self):
        self.cap = dict.fromkeys(MERKLE_BUFFERS, 0)

    def total(self):
        return sum(self.cap.values())

    def ensure(self, needs):
        """-> [(buffer, bytes, capacity before, capacity after)] of the needs above zero"""
        log = []
        for name, need in needs:
            if need:
                log.append((name, need, self.cap[name], max(self.cap[name], need)))
                self.cap[name] = log[-1][3]
        return log

    def trim(self, k):
        """-> {buffer: (capacity, limit)} of the buffers that held something; those above their limit are freed"""
        lim = merkle_trim_limits(k)
        held = {name: (cap, lim[name]) for name, cap in self.cap.items() if cap}
        for name, (cap, limit) in held.items():
            if cap > limit:
                self.cap[name] = 0
        return held

    def release(self):
        self.cap = dict.fromkeys(MERKLE_BUFFERS, 0)


class DevModel:
    def __init__(self):
        self.mk = MerkleBufs()
        self.chain_ns = []         # n of every chain_append so far: the chained ledger's history
        self.chain_at = None       # index of the last chain_append
        self.chain_restart = False # a release since: the next chain_append uploads the host copy of the frontier
        self.appends = {}          # index -> append_device operations whose roots and paths a verify may read
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

    def _pending(self, j):
        return any(j in v for v in self.streams.values())

    def _ordered(self, i, j, stream, what):
        """operation i on `stream` reads what operation j wrote on the device: j is synced, or on the same stream"""
        for s, v in self.streams.items():
            if j in v and s != stream:
                raise ValueError("operation %d on stream %r reads the output of %s %d, queued on stream %r and not "
                                 "synced" % (i, stream, what, j, s))

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
                t["mk"] = m.mk.ensure(merkle_needs(op))
            if k == "pack_bits":
                if m.last_dev is None or m.last_dev[1:] != (op.lo, n):
                    raise ValueError("operation %d: pack_bits without the device-resident verify it packs" % i)
                t["src"] = m.last_dev[0]
            if op.stream:
                self.streams[op.stream].append(i)
        elif k == "merkle_host":
            self._use(t, "merkle", n)
            t["mk"] = m.mk.ensure(merkle_needs(op))
        elif k in ("append_host", "append_device"):
            append_inputs(op.old, n)         # asserts that old size and n are of the grids
            self._use(t, "merkle", n)
            t["mk"] = m.mk.ensure(merkle_needs(op))
            t["fold"] = k == "append_device" and (op.roots or op.paths) and not (op.leaf and op.node)
            if k == "append_device":
                if op.roots and op.paths:
                    m.appends[i] = op
                if op.stream:
                    self.streams[op.stream].append(i)
        elif k in ("verify_incl_host", "verify_cons_host"):
            t["mk"] = m.mk.ensure(merkle_needs(op))
        elif k in ("verify_incl_device", "verify_cons_device"):
            t["nomem"] = was_live          # no context memory: nothing may change in a context that exists
            src = op.get("src")
            if src is not None:
                a = m.appends.get(src)
                if k != "verify_incl_device" or a is None or (a.old, a.n) != (op.old, op.n):
                    raise ValueError("operation %d: no append_device %r with roots and paths to verify" % (i, src))
                self._ordered(i, src, op.stream, "append")
            if op.stream:
                self.streams[op.stream].append(i)
        elif k == "chain_append":
            if n not in APPEND_SIZES:
                raise ValueError("operation %d: chain_append of %d leaves" % (i, n))
            start = sum(m.chain_ns)
            if m.chain_at is not None:
                if m.chain_restart and self._pending(m.chain_at):
                    raise ValueError("operation %d: the frontier to restart from is not synced" % i)
                if not m.chain_restart:
                    self._ordered(i, m.chain_at, op.stream, "chain_append")
            t["chain"], t["restart"], t["prev"] = len(m.chain_ns), m.chain_restart, m.chain_at
            t["chain_cross"] = any(start < (1 << b) < start + n for b in range(63))
            t["fold"] = not op.keep_hashes
            t["mk"] = m.mk.ensure(merkle_needs(op, {"start": start}))
            self._use(t, "merkle", n)
            m.chain_ns.append(n)
            m.chain_at, m.chain_restart = i, False
            if op.stream:
                self.streams[op.stream].append(i)
        elif k == "chain_verify":
            if m.chain_at is None:
                raise ValueError("operation %d: chain_verify before any chain_append" % i)
            self._ordered(i, m.chain_at, op.stream, "chain_append")
            t["chain"], t["prev"], t["nomem"] = len(m.chain_ns) - 1, m.chain_at, was_live
            if op.stream:
                self.streams[op.stream].append(i)
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
                    m.mk.release()
                    m.chain_restart = m.chain_at is not None
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
                    t["mk_trim"] = m.mk.trim(op.keep)
                    t["freed"] = [fam for fam, name in (("sync", "st"), ("pipe", "pst")) if m.cap[name] > slots]
                    for name in m.cap:
                        if m.cap[name] > slots:
                            m.cap[name] = 0
        else:
            raise ValueError("unknown operation kind %r" % k)
        m.settled += len(e.handed)
        t.update(rc=e.rc, route=e.route, handed=list(e.handed), noalloc=e.noalloc, mk_total=m.mk.total())
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
    if fam in SUBFAMILIES:      # the Merkle sub-families: by the model's capacities against trim_buffers' limits
        return any(cap > limit for name, (cap, limit) in t.get("mk_trim", {}).items() if name in SUBFAMILIES[fam])
    if fam in ("sync", "pipe"):
        return fam in t.get("freed", ())
    keep = t["op"].keep
    return keep == 0 or (n1 > 4096 and keep <= n1 // 2)


def kept_then_both(trace, fam):
    """A buffer of the sub-family is grown by a use, survives a trim with its capacity (at most the limit), is then
    used with a smaller need under that kept capacity and, still at that capacity, with a larger one."""
    for name in SUBFAMILIES[fam]:
        for a in trace:
            cap, limit = a.get("mk_trim", {}).get(name, (0, 0))      # mk_trim: of a trim that returned 0
            if not 0 < cap <= limit:
                continue
            smaller = larger = False
            for b in trace[a["i"] + 1:]:        # while the buffer still has that capacity
                for buf, need, before, _after in b.get("mk", ()):
                    if buf == name and before == cap:
                        smaller = smaller or need < cap
                        larger = larger or (need > cap and smaller)
            if smaller and larger:
                return True
    return False


def freed_then_larger(trace, fam):
    """A buffer of the sub-family is grown by a use, freed by a trim (its capacity above the limit) or a release,
    and then used with a larger need than that first use's (the families' condition, for one buffer)."""
    for name in SUBFAMILIES[fam]:
        for a in trace:
            for buf, need, _before, _after in a.get("mk", ()):
                if buf != name:
                    continue
                for b in trace[a["i"] + 1:]:
                    if b["kind"] in ("trim", "release") and freed_by(b, fam, 0) and (
                            b["kind"] == "release" or b["mk_trim"].get(name, (0, 0))[0] > b["mk_trim"].get(name, (0, 0))[1]):
                        if any(buf2 == name and need2 > need for d in trace[b["i"] + 1:]
                               for buf2, need2, _b, _a in d.get("mk", ())):
                            return True
    return False


def merkle_coverage(trace):
    """name -> bool: the conditions the batched append and the proof verification add"""
    c = {}
    kinds = {t["kind"] for t in trace}
    c["every_new_kind"] = all(k in kinds for k in NEW_KINDS)
    combos = {tuple(bool(t["op"].p[f]) for f in APPEND_FLAGS) for t in trace if t["kind"] in ("append_host",
                                                                                              "append_device")}
    c["append_flag_combinations"] = all((r, p, lf, nd) in combos for r in (False, True) for p in (False, True)
                                        for lf in (False, True) for nd in (False, True) if r or p)
    # the fold scratch on two caller streams back to back: nothing between them waits for either stream
    fold, ok = None, False
    for t in trace:
        if t["kind"] in ("sync", "trim", "release", "set_chunk", "prepare", "pipeline_sync"):
            fold = None
        elif t.get("fold") and t["op"].get("stream"):
            ok = ok or (fold is not None and fold != t["op"].stream)
            fold = t["op"].stream
    c["fold_two_streams"] = ok
    for fam in SUBFAMILIES:
        c["kept_" + fam] = kept_then_both(trace, fam)
        c["freed_" + fam] = freed_then_larger(trace, fam)
    pairs = set()
    for a, b in zip(trace, trace[1:]):
        ks = (a["kind"], b["kind"])
        if ks in (("verify_incl_host", "verify_cons_host"), ("verify_cons_host", "verify_incl_host")) and \
                a["op"].n != b["op"].n and a["op"].computed != b["op"].computed:
            pairs.add(ks[0])
    c["inclusion_consistency_both_orders"] = len(pairs) == 2
    c["chain_crosses_power_of_two"] = any(t.get("chain_cross") for t in trace)
    busy = [t["i"] for t in trace if t["kind"] in ("trim", "release") and t["rc"] == E_BUSY]
    c["two_busy_then_merkle"] = sum(1 for i in busy if any(t["i"] > i and t["kind"] in NEW_KINDS for t in trace)) >= 2
    return c


def coverage(trace, merkle=False):
    """name -> bool: the conditions of the issue, over one sequence's trace (merkle: with merkle_coverage's)"""
    c = merkle_coverage(trace) if merkle else {}
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

    def __init__(self, backend, devices=1, seed=None, plan=()):
        self.be, self.model, self.seed = backend, Model(devices), seed
        self.devices = devices
        self.plan = tuple(plan)    # n of every chain_append of the whole list, where known: one reference run for all
        self.chain = {}            # device -> (index, handle) of the last chain_append; chain handles are never
        self.kept = {}             # dropped, nor are append_device's (index -> handle): a later verify reads their
        #                            buffers, and freeing device memory would wait for the streams between calls
        self.handles = {}          # operation index -> (operation, backend handle) until its outputs are checked
        self.settled = {}          # device -> its last handed-over asynchronous batches, for the probes after a release
        self.floor = [0] * devices
        self.ops = []
        self.comparisons = 0
        self.noalloc_checks = 0
        self.nomem_checks = 0      # device verify forms across which context_memory was compared
        self.mk_before = {}        # device -> the model's Merkle bytes after the operation before
        self.last_dev = {}         # device -> (index, handle) of the last device-resident verify (pack_bits reads it)

    # -- outputs
    def chain_step(self, i):
        """the chain_reference record of the chain operation i"""
        t = self.model.trace[i]
        ns = tuple(self.model.dev[t["dev"]].chain_ns)
        if self.plan[:len(ns)] == ns:
            ns = self.plan
        return chain_reference(ns)[t["chain"]]

    def check(self, i, op, handle):
        got = dict(self.be.read(handle))
        if op.kind in ("chain_append", "chain_verify"):
            want = chain_expect(op, self.chain_step(i))
        else:
            want = expect(op)
        if op.kind in ("merkle_host", "merkle_device"):
            want = {k: v for k, v in want.items() if k in got}
        for name in [k for k in got if k.startswith("untouched_")]:      # an output not asked for: sentinels throughout
            assert name[10:] not in want and (np.asarray(got.pop(name)) == SENT).all(), \
                "the %s of operation %d %r was not asked for and was written" % (name[10:], i, op)
        assert set(got) == set(want), "operation %d %r: outputs %s, expected %s" % (i, op, sorted(got), sorted(want))
        if op.kind == "chain_append":       # the host copy a chain restarts from after a release
            handle.copy = {k: np.array(got[k][:want[k].size]) for k in ("frontier", "root")}
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
            elif op.kind in ("append_device", "chain_append", "chain_verify"):
                self.kept[j] = h
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
        be.at, be.op = i, op
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
        elif k in ("append_device", "verify_incl_device", "verify_cons_device", "chain_append", "chain_verify"):
            if k == "append_device":
                h = be.append_device(d, append_inputs(op.old, op.n), op.stream, *[op.p[f] for f in APPEND_FLAGS])
            elif k == "verify_incl_device" and op.get("src") is not None:
                src = self.handles[op.src][1] if op.src in self.handles else self.kept[op.src]
                h = be.verify_appended(d, src, append_inputs(op.old, op.n), op.computed, op.stream)
            elif k == "verify_incl_device":
                h = be.verify_incl_device(d, proof_case("incl", op.n, op.seed), op.by_hash, op.computed, op.leaf_base,
                                          op.proof_base, op.stream)
            elif k == "verify_cons_device":
                h = be.verify_cons_device(d, proof_case("cons", op.n, op.seed), op.computed, op.proof_base, op.stream)
            else:
                step, prev = self.chain_step(i), self.chain.get(d, (None, None))[1]
                if k == "chain_append":
                    h = be.chain_append(d, prev, step, op.stream, op.keep_hashes, t["restart"])
                    self.chain[d] = (i, h)
                else:
                    h = be.chain_verify(d, prev, step, op.stream)
            self.handles[i] = (op, h)
            if not op.get("stream"):
                self.finish([i])
        elif k in ("append_host", "verify_incl_host", "verify_cons_host"):
            if k == "append_host":
                h = be.append_host(d, append_inputs(op.old, op.n), *[op.p[f] for f in APPEND_FLAGS])
            elif k == "verify_incl_host":
                h = be.verify_incl_host(d, proof_case("incl", op.n, op.seed), op.by_hash, op.computed, op.leaf_base,
                                        op.proof_base)
            else:
                h = be.verify_cons_host(d, proof_case("cons", op.n, op.seed), op.computed, op.proof_base)
            self.check(i, op, h)
            be.drop(h)
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
        # the Merkle buffers: chunk_scratch is the chunk set's bytes plus the model's fifteen capacities, and a
        # Merkle operation leaves the chunk set alone (in a context that existed before it)
        if mem["total"]:
            assert mem["chunk_scratch"] >= t["mk_total"], "context_memory %r: the Merkle buffers alone are %d" % (
                mem, t["mk_total"])
        if "mk" in t and before[1]["total"]:
            grown = t["mk_total"] - self.mk_before.get(d, 0)
            assert mem["chunk_scratch"] - before[1]["chunk_scratch"] == grown, \
                "%r: chunk_scratch %d -> %d, the model's buffers grow by %d (%r)" % (
                    op, before[1]["chunk_scratch"], mem["chunk_scratch"], grown, t["mk"])
        if t.get("nomem"):
            assert mem == before[1], "%r uses no context memory: %r -> %r" % (op, before[1], mem)
            self.nomem_checks += 1
        self.mk_before[d] = t["mk_total"]
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
    r = Runner(backend, devices, seed, plan=[op.n for op in ops if op.kind == "chain_append"])
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


def generate(seed, steps, merkle=False):
    """A random sequence of `steps` operations (or one fewer) for one device:
    weights per kind, raised for kinds, setting values and buffer-family
    stages (use, trim below, use larger) the sequence has not covered yet.
    The large table policy is excluded and no batch reaches 65,536.  It ends
    by handing over and syncing everything, then release.

    merkle: the kinds of NEW_KINDS enter as motifs, short runs of operations
    with seeded parameters placed whole at seeded points between the others
    (in seeded order), one per condition of merkle_coverage; the list is then
    longer than `steps` by what the motifs left over at the end take.  Without
    it the list is what it was before these kinds existed, operation for
    operation (tests/test_sequence_model_cpu.py holds the digests)."""
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

    # -- the motifs of the batched append and the proof verification
    small_old = [ac.OLD_GRID.index(x) for x in APPEND_OLD]

    def old_for(n):
        return rng.choice([j for j in small_old if ac.OLD_GRID[j] + n <= MERKLE_MAX_SIZE and
                           (n != 66000 or ac.OLD_GRID[j] == 0)])

    def settle():
        """everything handed over and synced: a trim after it succeeds, and nothing queued uses what it frees"""
        for j, tid in enumerate(sorted(m.slots.values())):
            emit(Op("wait_async" if j % 2 else "query_async", tid=tid))
        if m.pipe:
            emit(Op("pipeline_sync"))
        sync_streams()

    def sync_streams():
        for s_ in ("a", "b"):
            if model.streams[s_]:
                emit(Op("sync", stream=s_))

    def emit_at(op):
        emit(op)
        return len(ops) - 1

    def fold_op(n, stream, leaf=False, node=False, roots=True, paths=True):
        return Op("append_device", old=old_for(n), n=n, stream=stream, roots=roots, paths=paths, leaf=leaf, node=node)

    def m_fold():
        s1, s2 = rng.sample(["a", "b"], 2)
        first = fold_op(rng.choice((63, 64, 65, 257)), s1)
        at = emit_at(first)
        emit(fold_op(rng.choice((1, 63, 257, 1000)), s2, leaf=rng.random() < 0.3))
        emit(Op("verify_incl_device", src=at, old=first.old, n=first.n, computed=rng.random() < 0.5, stream=s1))

    def incl_host(n, computed):
        return Op("verify_incl_host", n=n, seed=rng.randrange(3), by_hash=rng.random() < 0.5, computed=computed,
                  leaf_base=rng.choice((0, 7)), proof_base=rng.choice((0, 5)))

    def cons_host(n, computed):
        return Op("verify_cons_host", n=n, seed=rng.randrange(3), computed=computed, proof_base=rng.choice((0, 5)))

    def m_kept(fam):
        settle()
        emit(Op("trim", keep=0))
        if fam == "fold":
            uses = [fold_op(n, rng.choice([None, "a", "b"])) for n in (257, rng.choice((63, 64, 65)), 1000)]
        elif fam == "stage":
            fl = dict(roots=True, paths=rng.random() < 0.5, leaf=rng.random() < 0.5, node=rng.random() < 0.5)
            uses = [Op("append_host", old=old_for(n), n=n, **fl) for n in (257, rng.choice((63, 64, 65)), 1000)]
        else:
            uses = [incl_host(257, True), cons_host(rng.choice((63, 64, 65)), False), cons_host(257, True)]
        emit(uses[0])
        sync_streams()
        emit(Op("trim", keep=257))
        emit(uses[1])
        emit(uses[2])

    def m_order():
        n1, n2, n3 = rng.sample(PROOF_SIZES[:5], 3)
        c = rng.random() < 0.5
        emit(incl_host(n1, c))
        emit(cons_host(n2, not c))
        emit(incl_host(n3, c))

    def m_flags():
        combos = [(r, p, lf, nd) for r in (False, True) for p in (False, True) for lf in (False, True)
                  for nd in (False, True) if r or p]
        rng.shuffle(combos)
        for r, p, lf, nd in combos:
            n = rng.choice((1, 63, 64, 65, 257))
            if rng.random() < 0.5:
                emit(Op("append_host", old=old_for(n), n=n, roots=r, paths=p, leaf=lf, node=nd))
            else:
                emit(Op("append_device", old=old_for(n), n=n, stream=rng.choice([None, "a", "b"]), roots=r, paths=p,
                        leaf=lf, node=nd))

    def chain_on(kind, stream, **p):
        """a chain operation on `stream`, after the sync its producer needs where that is queued on another one"""
        if m.chain_at is not None:
            for s_, v in model.streams.items():
                if m.chain_at in v and (s_ != stream or (kind == "chain_append" and m.chain_restart)):
                    emit(Op("sync", stream=s_))
        emit(Op(kind, stream=stream, **p))

    def m_chain():
        crossed = False
        for _ in range(5):
            chain_on("chain_append", rng.choice([None, "a", "b"]), n=rng.choice((1, 63, 64, 65, 257)),
                     keep_hashes=rng.random() < 0.5)
            crossed = crossed or model.trace[-1]["chain_cross"]
            if rng.random() < 0.6:
                chain_on("chain_verify", rng.choice([None, "a", "b"]))
            if crossed and rng.random() < 0.5:
                break
        if not crossed:     # 257 more leaves cross a power of two from any size
            chain_on("chain_append", None, n=257, keep_hashes=False)
            chain_on("chain_append", None, n=257, keep_hashes=True)

    def m_busy():
        for k_ in range(2):
            n = rng.choice((17, 257))
            at = emit_at(Op("verify_async", lo=lo_for(n), n=n, api="digest", digests=k_ == 0, mem="pageable"))
            emit(Op("trim", keep=rng.choice((0, 400))) if k_ else Op("release"))
            emit(Op("wait_async", tid=at))
            n = rng.choice(PROOF_SIZES[:5])
            if k_:
                emit(Op("verify_cons_device", n=n, seed=rng.randrange(3), computed=rng.random() < 0.5,
                        proof_base=rng.choice((0, BIG_BASE)), stream=rng.choice([None, "a", "b"])))
            else:
                emit(Op("verify_incl_device", n=n, seed=rng.randrange(3), by_hash=rng.random() < 0.5,
                        computed=rng.random() < 0.5, leaf_base=rng.choice((0, BIG_BASE)),
                        proof_base=rng.choice((0, BIG_BASE + 8)), stream=rng.choice([None, "a", "b"])))

    motifs = []
    if merkle:
        motifs = [m_fold, lambda: m_kept("fold"), lambda: m_kept("stage"), lambda: m_kept("mv"), m_order, m_flags,
                  m_chain, m_busy, m_chain]
        rng.shuffle(motifs)

    while len(ops) + closing() + 3 < steps:
        if motifs and rng.random() < 0.12:
            motifs.pop()()
            continue
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
    while motifs:
        motifs.pop()()
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

    # -- the batched append.  An output not asked for gets a sentinel-filled buffer all the same and a null
    # pointer in the call: read() returns it as untouched_<name>.
    @staticmethod
    def _append_outputs(c, roots, paths, leaf, node):
        """(bytes of every output of an append of c["n"] leaves onto c["old"], which of them the call asks for)"""
        n, new = c["n"], c["old"] + c["n"]
        sizes = {"roots": 32 * n, "paths": 32 * c["entries"], "leaf": 32 * n, "node": 32 * c["nodes"],
                 "frontier": 32 * mc.popcount(new), "root": 32}
        return sizes, {"roots": roots, "paths": paths, "leaf": leaf, "node": node, "frontier": True, "root": True}

    def append_host(self, dev, c, roots, paths, leaf, node):
        sizes, asked = self._append_outputs(c, roots, paths, leaf, node)
        buf = {k: np.full(sizes[k] + 32, SENT, np.uint8) for k in sizes}
        ptr = {k: buf[k].ctypes.data if asked[k] else None for k in sizes}
        fr = c["frontier"]
        self.ok(self.lib.edv_merkle_append_batch(c["old"], fr.ctypes.data if fr.size else None, c["blob"].ctypes.data,
                                                 c["off"].ctypes.data, c["n"], ptr["leaf"], ptr["node"],
                                                 ptr["frontier"], ptr["root"], ptr["roots"], ptr["paths"], dev))
        return _H(host={(k if asked[k] else "untouched_" + k): buf[k] for k in sizes})

    def append_device(self, dev, c, stream, roots, paths, leaf, node):
        ins = [self.dev_in(dev, c["frontier"]), self.dev_in(dev, c["blob"]), self.dev_in(dev, c["off"])]
        sizes, asked = self._append_outputs(c, roots, paths, leaf, node)
        buf = {k: self.dev_out(dev, sizes[k], 32) for k in sizes}
        ptr = {k: buf[k].ptr if asked[k] else None for k in sizes}
        self.ok(self.lib.edv_merkle_append_batch_dev(c["old"], ins[0].ptr if c["frontier"].size else None, ins[1].ptr,
                                                     ins[2].ptr, 0, c["n"], ptr["leaf"], ptr["node"], ptr["frontier"],
                                                     ptr["root"], ptr["roots"], ptr["paths"], dev, self.stream(stream)))
        return _H(dev={(k if asked[k] else "untouched_" + k): buf[k] for k in sizes}, keep=ins, leaves=ins[1],
                  off=ins[2])

    # -- proof verification
    @staticmethod
    def _proof_arrays(c, by_hash, leaf_base, proof_base, filler):
        """the batch's arrays; the bases are added to the offsets, and with `filler` (the host forms, whose
        offsets are absolute into the caller's arrays) that many unused bytes / entries lie in front"""
        b, a = c["batch"], {}
        if c["kind"] == "incl":
            if by_hash:
                a["leaf_hashes"] = vc.pack_hashes(b.leaf_hashes())
            else:
                blob, off = mc.pack(b.leaves, leaf_base if filler else 0)
                a["leaves"] = np.concatenate([blob, np.zeros(8, np.uint8)])
                a["leaf_off"] = off if filler else off + np.uint64(leaf_base)
            a["index"], a["size"], a["roots"] = vc.u64(b.index), vc.u64(b.size), vc.pack_hashes(b.root)
        else:
            a["old"], a["new"] = vc.u64(b.old), vc.u64(b.new)
            a["old_roots"], a["new_roots"] = vc.pack_hashes(b.old_root), vc.pack_hashes(b.new_root)
        proofs, poff = vc.pack_proofs(b.proof, proof_base if filler else 0)
        a["proofs"], a["proof_off"] = proofs, poff if filler else poff + np.uint64(proof_base)
        return a

    def _proof_out(self, n, cbytes, computed, dev=None):
        """status and computed with their sentinel tails, on the host or (dev given) on the device"""
        if dev is None:
            return np.full(n + ROW, SENT, np.uint8), np.full(cbytes * n + 32, SENT, np.uint8)
        return self.dev_out(dev, n, ROW), self.dev_out(dev, cbytes * n, 32)

    def verify_incl_host(self, dev, c, by_hash, computed, leaf_base, proof_base):
        a = self._proof_arrays(c, by_hash, leaf_base, proof_base, True)
        st, comp = self._proof_out(c["n"], 32, computed)
        p = {k: v.ctypes.data for k, v in a.items()}
        self.ok(self.lib.edv_merkle_verify_inclusion(p.get("leaves"), p.get("leaf_off"), p.get("leaf_hashes"), p["index"],
                                                     p["size"], p["roots"], p["proofs"], p["proof_off"], c["n"],
                                                     st.ctypes.data, comp.ctypes.data if computed else None, dev))
        return _H(host={"status": st, ("computed" if computed else "untouched_computed"): comp}, arrays=a)

    def verify_cons_host(self, dev, c, computed, proof_base):
        a = self._proof_arrays(c, False, 0, proof_base, True)
        st, comp = self._proof_out(c["n"], 64, computed)
        p = {k: v.ctypes.data for k, v in a.items()}
        self.ok(self.lib.edv_merkle_verify_consistency(p["old"], p["new"], p["old_roots"], p["new_roots"], p["proofs"],
                                                       p["proof_off"], c["n"], st.ctypes.data,
                                                       comp.ctypes.data if computed else None, dev))
        return _H(host={"status": st, ("computed" if computed else "untouched_computed"): comp}, arrays=a)

    def verify_incl_device(self, dev, c, by_hash, computed, leaf_base, proof_base, stream):
        a = self._proof_arrays(c, by_hash, leaf_base, proof_base, False)
        d = {k: self.dev_in(dev, v) for k, v in a.items()}
        st, comp = self._proof_out(c["n"], 32, computed, dev)
        p = {k: v.ptr for k, v in d.items()}
        self.ok(self.lib.edv_merkle_verify_inclusion_dev(
            p.get("leaves"), p.get("leaf_off"), 0 if by_hash else leaf_base, p.get("leaf_hashes"), p["index"],
            p["size"], p["roots"], p["proofs"], p["proof_off"], proof_base, c["n"], st.ptr,
            comp.ptr if computed else None, dev, self.stream(stream)))
        return _H(dev={"status": st, ("computed" if computed else "untouched_computed"): comp}, keep=list(d.values()))

    def verify_cons_device(self, dev, c, computed, proof_base, stream):
        a = self._proof_arrays(c, False, 0, proof_base, False)
        d = {k: self.dev_in(dev, v) for k, v in a.items()}
        st, comp = self._proof_out(c["n"], 64, computed, dev)
        p = {k: v.ptr for k, v in d.items()}
        self.ok(self.lib.edv_merkle_verify_consistency_dev(
            p["old"], p["new"], p["old_roots"], p["new_roots"], p["proofs"], p["proof_off"], proof_base, c["n"],
            st.ptr, comp.ptr if computed else None, dev, self.stream(stream)))
        return _H(dev={"status": st, ("computed" if computed else "untouched_computed"): comp}, keep=list(d.values()))

    def _verify_paths(self, dev, start, n, poff, d_leaves, d_leaf_off, d_roots, d_paths, computed, stream):
        """edv_merkle_verify_inclusion_dev on an append's path and per-leaf root buffers as they are: leaf i has
        index start + i in the tree of start + i + 1 leaves; the offsets are the caller's own prefix sums"""
        idx = np.arange(start, start + n, dtype=np.uint64)
        ins = [self.dev_in(dev, idx), self.dev_in(dev, idx + np.uint64(1)), self.dev_in(dev, poff)]
        st, comp = self._proof_out(n, 32, computed, dev)
        self.ok(self.lib.edv_merkle_verify_inclusion_dev(d_leaves, d_leaf_off, 0, None, ins[0].ptr, ins[1].ptr, d_roots,
                                                         d_paths, ins[2].ptr, 0, n, st.ptr,
                                                         comp.ptr if computed else None, dev, self.stream(stream)))
        return {"status": st, ("computed" if computed else "untouched_computed"): comp}, ins

    def verify_appended(self, dev, src, c, computed, stream):
        poff = np.zeros(c["n"] + 1, np.uint64)
        poff[1:] = np.cumsum([mc.popcount(c["old"] + i) for i in range(c["n"])], dtype=np.uint64)
        out, ins = self._verify_paths(dev, c["old"], c["n"], poff, src.leaves.ptr, src.off.ptr, src.dev["roots"].ptr,
                                      src.dev["paths"].ptr, computed, stream)
        return _H(dev=out, keep=ins)

    # -- the chained ledger: every buffer stays on the device from one step to the next
    def _consistency_one(self, dev, step, d_old_root, d_new_root, computed, stream):
        """one proof, from the size before the step to the size after it, the roots read where the appends left them"""
        proof = _u8(b"".join(step["proof"])) if step["proof"] else np.zeros(32, np.uint8)
        ins = [self.dev_in(dev, vc.u64([step["start"]])), self.dev_in(dev, vc.u64([step["size"]])),
               self.dev_in(dev, proof), self.dev_in(dev, vc.u64([0, len(step["proof"])]))]
        st, comp = self._proof_out(1, 64, computed, dev)
        self.ok(self.lib.edv_merkle_verify_consistency_dev(ins[0].ptr, ins[1].ptr, d_old_root, d_new_root, ins[2].ptr,
                                                           ins[3].ptr, 0, 1, st.ptr, comp.ptr if computed else None, dev,
                                                           self.stream(stream)))
        return st, comp, ins

    def chain_append(self, dev, prev, step, stream, keep_hashes, restart):
        n, start = step["n"], step["start"]
        keep = []
        if prev is None:
            d_old, old_root = None, self.dev_in(dev, _u8(mc.EMPTY_ROOT))
        elif restart:       # after a release: from the host copy of the frontier and of the root
            d_old, old_root = self.dev_in(dev, prev.copy["frontier"]), self.dev_in(dev, prev.copy["root"])
            keep.append(d_old)
        else:
            d_old, old_root = prev.dev["frontier"], prev.dev["root"]
        if step["lo"] is None:
            off = self.dev_in(dev, np.arange(n + 1, dtype=np.uint64) * np.uint64(16))
            keep.append(off)
            d_off = off.ptr
        else:
            d_off = self.d["off"].ptr + 8 * step["lo"]
        sizes, asked = self._append_outputs({"old": start, "n": n, "entries": step["entries"], "nodes": step["nodes"]},
                                            True, True, keep_hashes, keep_hashes)
        buf = {k: self.dev_out(dev, sizes[k], 32) for k in sizes}
        ptr = {k: buf[k].ptr if asked[k] else None for k in sizes}
        self.ok(self.lib.edv_merkle_append_batch_dev(start, d_old.ptr if d_old else None, self.d["msgs"].ptr, d_off, 0, n,
                                                     ptr["leaf"], ptr["node"], ptr["frontier"], ptr["root"],
                                                     ptr["roots"], ptr["paths"], dev, self.stream(stream)))
        st, comp, ins = self._consistency_one(dev, step, old_root.ptr, buf["root"].ptr, True, stream)
        out = {(k if asked[k] else "untouched_" + k): buf[k] for k in sizes}
        out.update(cstatus=st, ccomputed=comp)
        return _H(dev=out, keep=keep + ins, d_off=d_off, old_root=old_root)

    def chain_verify(self, dev, cur, step, stream):
        out, ins = self._verify_paths(dev, step["start"], step["n"], step["poff"], self.d["msgs"].ptr, cur.d_off,
                                      cur.dev["roots"].ptr, cur.dev["paths"].ptr, True, stream)
        st, comp, ins2 = self._consistency_one(dev, step, cur.old_root.ptr, cur.dev["root"].ptr, False, stream)
        out.update(cstatus=st, untouched_ccomputed=comp)
        return _H(dev=out, keep=ins + ins2)

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
def _old(size):
    """a batched append's old size as its index in merkle_append_cases.OLD_GRID"""
    return ac.OLD_GRID.index(size)


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
    # one operation of every kind of the batched append and the proof verification; the chain goes on from its
    # first step after the release in the middle, restarted from the host copy of the frontier
    q.add("append_host", old=_old(255), n=65, roots=True, paths=k == 0, leaf=k == 1, node=False)
    at = q.add("append_device", old=_old(2 ** 32 - 1), n=257, stream="b", roots=True, paths=True, leaf=False,
               node=k == 1)
    q.add("verify_incl_device", src=at, old=_old(2 ** 32 - 1), n=257, computed=True, stream="b")
    q.add("verify_incl_host", n=63, seed=k, by_hash=k == 1, computed=True, leaf_base=7 * k, proof_base=5 * (1 - k))
    q.add("verify_cons_host", n=65, seed=k, computed=False, proof_base=5 * k)
    q.add("verify_cons_device", n=64, seed=k, computed=True, proof_base=BIG_BASE * k, stream=None)
    q.add("verify_incl_device", n=63, seed=k + 1, by_hash=k == 0, computed=k == 0, leaf_base=BIG_BASE * k,
          proof_base=(BIG_BASE + 8) * (1 - k), stream="b")
    q.add("chain_append", n=(65, 63)[k], stream="b", keep_hashes=k == 0)
    q.add("chain_verify", stream="b")
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


def merkle_staging():
    """The host forms alone, in the staging they share: proof batches of both kinds, sizes and `computed` settings
    one after another in mv_*, and between them host appends with every combination of the four output flags
    and an extend with null outputs, all in mk_leafh / mk_nodeh."""
    q = Seq()
    five = (("verify_incl_host", dict(n=4097, by_hash=False, computed=True)),
            ("verify_cons_host", dict(n=63, computed=False)),
            ("verify_incl_host", dict(n=65, by_hash=True, computed=True)),
            ("verify_cons_host", dict(n=257, computed=True)),
            ("verify_incl_host", dict(n=1, by_hash=False, computed=False)))
    combos = [(r, p, lf, nd) for r in (False, True) for p in (False, True) for lf in (False, True)
              for nd in (False, True)]
    count = [0]

    def proofs(j, k):
        kind, p = five[j]
        bases = dict(proof_base=(0, 5)[(j + k) % 2])
        if kind == "verify_incl_host":
            bases["leaf_base"] = (7, 0)[(j + k) % 2]
        q.add(kind, seed=k, **p, **bases)

    def appends(howmany):
        for _ in range(howmany):
            c = count[0]
            n = (65, 1000, 64)[c % 3]
            r, p, lf, nd = combos[(5 * c) % 16]       # 5 is odd: sixteen in a row are all sixteen
            old = APPEND_OLD[c % 6] if APPEND_OLD[c % 6] + n <= MERKLE_MAX_SIZE else 0
            q.add("append_host", old=_old(old), n=n, roots=r, paths=p, leaf=lf, node=nd)
            if c % 4 == 0:      # an extend with null outputs between two appends: the same staging, nothing copied back
                q.add("merkle_host", old=(6, 4, 10)[c // 4 % 3], n=257, leaf=False, node=False)
            count[0] += 1

    for k in range(2):
        for j in range(5):
            proofs(j, k)
            if j >= 2:          # 1 -> 2 -> 3 follow each other: inclusion and consistency in both orders
                appends(3)
        q.add("trim", keep=257)
        for j in reversed(range(5)):
            proofs(j, k)
            if j in (3, 1):
                appends(3)
        appends(1)
        q.add("trim", keep=1)
    # a kept capacity: grown by 257 (65), left alone by trim(257), then met by a smaller and by a larger need
    q.add("verify_incl_host", n=257, seed=2, by_hash=False, computed=True, leaf_base=0, proof_base=5)
    q.add("append_host", old=_old(256), n=65, roots=True, paths=True, leaf=True, node=True)
    q.add("trim", keep=257)
    q.add("verify_cons_host", n=63, seed=2, computed=False, proof_base=0)
    q.add("append_host", old=_old(65535), n=64, roots=True, paths=True, leaf=False, node=False)
    q.add("verify_incl_host", n=4097, seed=0, by_hash=True, computed=True, leaf_base=0, proof_base=0)
    q.add("append_host", old=_old(0), n=1000, roots=True, paths=False, leaf=False, node=True)
    q.add("release", final=True)
    return q


def merkle_fold_streams():
    """Two caller streams and the library stream with no sync between the calls: the device append's fold
    scratch (null leaf / node outputs) used, grown and used again while the other stream's append is queued."""
    q = Seq()

    def once(s1, s2, k):
        first = dict(old=_old(255), n=257)
        at = q.add("append_device", stream=s1, roots=True, paths=True, leaf=k == 1, node=False, **first)
        q.add("append_device", old=_old(0), n=66000, stream=s2, roots=True, paths=True, leaf=False, node=False)   # a grow
        q.add("append_device", old=_old(2 ** 32 - 1), n=63, stream=s1, roots=k != 1, paths=True, leaf=False,
              node=k == 2)
        q.add("merkle_device", old=7, n=1000, stream=s2)      # two passes: it waits on the tile-root scratch all the same
        q.add("verify_incl_device", src=at, computed=True, stream=s1, **first)
        q.add("verify_cons_device", n=65, seed=k, computed=k == 0, proof_base=BIG_BASE, stream=None)    # library stream
        q.add("trim", keep=0)         # drains through the scratch event: what is queued on a and b stays valid
        q.add("sync", stream="a")
        q.add("sync", stream="b")
    once("a", "b", 0)
    once("b", "a", 1)
    q.add("release")
    once("a", "b", 2)
    q.add("release", final=True)
    return q


def ledger_chain():
    """A device-resident ledger: every append's d_old_hashes is the frontier buffer the append before it wrote,
    every verify reads the append's path and root buffers as they are.  A stream is synced only where the
    next consumer runs on another stream (or, for a release, where the host copy must be complete)."""
    q = Seq()
    q.add("chain_append", n=63, stream="a", keep_hashes=True)
    q.add("chain_verify", stream="a")
    q.add("sync", stream="a")             # needed: the next append, on b, reads a's frontier
    q.add("chain_append", n=1, stream="b", keep_hashes=False)
    q.add("chain_append", n=65, stream="b", keep_hashes=False)      # 64 -> 129: across 128; same stream, no sync
    q.add("chain_verify", stream="b")
    q.add("sync", stream="b")             # needed: a reads b's frontier
    q.add("chain_append", n=257, stream="a", keep_hashes=False)     # 129 -> 386: across 256
    q.add("sync", stream="a")             # needed: b reads a's frontier (the trim drains by itself)
    q.add("trim", keep=257)               # the fold scratch grown by 257 stays
    q.add("chain_append", n=64, stream="b", keep_hashes=False)      # a smaller need under the kept capacity
    q.add("sync", stream="b")             # needed: a reads b's frontier
    q.add("chain_append", n=1000, stream="a", keep_hashes=False)    # a larger one; two passes; across 512 and 1,024
    q.add("chain_verify", stream="a")
    t = q.add("verify_async", lo=37, n=400, api="digest", digests=True, mem="pageable")
    q.add("trim", keep=400)               # BUSY: the ticket is outstanding
    q.add("release")                      # BUSY
    q.add("wait_async", tid=t)
    q.add("sync", stream="a")             # needed: the restart below uploads the host copy of a's frontier
    q.add("release")
    q.add("chain_append", n=66000, stream="b", keep_hashes=True)    # restarted from the host copy; three passes
    q.add("chain_verify", stream="b")
    q.add("sync", stream="b")             # needed: a reads b's frontier
    q.add("chain_append", n=1, stream="a", keep_hashes=False)
    q.add("chain_append", n=63, stream="a", keep_hashes=True)
    q.add("chain_verify", stream="a")
    q.add("sync", stream="a")             # needed: the library stream reads a's frontier
    q.add("trim", keep=0)
    q.add("chain_append", n=64, stream=None, keep_hashes=False)
    q.add("chain_verify", stream=None)
    q.add("release", final=True)
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
    "merkle_staging": (merkle_staging, 1, {}),
    "merkle_fold_streams": (merkle_fold_streams, 1, {}),
    "ledger_chain": (ledger_chain, 1, {}),
})
SEEDS = (41, 42, 65)
STEPS = 80
# random_merkle_<seed> = generate(seed, 120, merkle=True).  Chosen on the CPU: the first two seeds from 100 upward
# whose list alone meets every condition of coverage(trace, merkle=True), the earlier ones and merkle_coverage's
# (every seed tried met the latter, which the motifs see to; 110 and 214 are the first to meet the former in the
# eighty or so operations the motifs leave them).
MERKLE_SEEDS = (110, 214)
MERKLE_STEPS = 120


def sequence(name):
    """(operations, devices, seed) of a directed sequence, or of random_<seed>"""
    if name.startswith("random_merkle_"):
        seed = int(name[14:])
        return generate(seed, MERKLE_STEPS, merkle=True), 1, seed
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
                      "noalloc_checks": r.noalloc_checks, "nomem_checks": r.nomem_checks,
                      "references_s": round(p.build_seconds, 2), "merkle_references_s": round(merkle_seconds(), 2),
                      "run_s": round(time.perf_counter() - t1, 2), "total_s": round(time.perf_counter() - t0, 2)}))
