"""The digests edv_verify_digest_batch_async hands back (a Node's
Request.getDigest: a wrong one is a wrong request identity, and rejects
nothing), on every route of submit_async (csrc/edv_runtime.hip) and every
buffer kind, called through edv.lib() directly:

  route                          reached by                   n
  latency, right-to-left kernel  the default latency limit    1, 16, 17, 400
  latency, two-walk kernel       the default latency limit    4,097, 8,193
  the slot's own stream          set_latency_path(0, 0)       1, 257, 8,192
  the shared copy/kernel streams set_latency_path(0, 0)       8,193

Each (route, n) runs inputs pageable with digests pageable and with digests
page-locked, inputs page-locked in three regions, and inputs page-locked in
ONE region laid out sigs | pks | offsets with gaps of 16 and 8 bytes
(the input stager's single-copy branch, one_span of csrc/edv_hostplan.h), each with off[0] = 0 and off[0] = 5 (the
message pointer unchanged); the latency route once more in a child process
with EDV_QUAD_ZERO_COPY=0 (read once per process).  Every digest byte equals
hashlib.sha256's, every verdict the checker's (libsodium where present, else
the oracle), rejected requests included, and the sentinel bytes past the last
digest and the last verdict stay.  Then slot reuse: twenty batches back to
back on the eight slots, sizes alternating large and small, buffers alternating
page-locked and pageable, every third without digests, handed over by slot
reuse, by edv_wait_async out of order and by edv_query_async; and empty
batches.

The latency route's 8,193 is past kSmallAsync: a latency-path batch runs on its
slot's own stream at every size up to the limit.  Digest comparisons per run (8
buffer/offset combinations per size): latency route 101,792 (+ 25,448 in the
child), own stream 67,600, shared streams 65,544,
slot reuse 2 x 1,801 (and 2 x 2,168 verdicts), empty 2 x 44.  Measured on
MI355X: 14 tests in 2.0 s before [latency-8193] (0.16 s)
was added; the child process 0.9 s (1.2 s with that size), the
first case 0.4 s (it signs the pool's 4,097 requests), [latency-8193] 0.16 s (it
builds the corpus), every other case at most 0.04 s.
"""
import ctypes
import hashlib
import os
import random
import subprocess
import sys
import time

import numpy as np
import pytest

import oracle_lib as orc
from indy_plenum_amd import edv
from test_gpu_runtime import checker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TESTS = os.path.dirname(os.path.abspath(__file__))

SPECIAL_LENS = [0, 1, 3, 54, 55, 56, 57, 63, 64, 65, 119, 120, 121, 127, 128, 129, 4096]
POOL_N = 4097
SENT = 0xA5
SMALL_ORDER_A = bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05")  # order 8
LATENCY = [("latency", n) for n in (1, 16, 17, 400, 4097, 8193)]
ROUTES = LATENCY + [("own", n) for n in (1, 257, 8192)] + [("shared", 8193)]


class Batch:
    """Requests in the C-ABI layout (msgs ends with 64 spare bytes), their
    digests by hashlib and their verdicts by the checker."""

    def __init__(self, sigs, pks, msgs, off):
        self.sigs, self.pks, self.msgs, self.off = sigs, pks, msgs, off
        self.n = len(off) - 1
        assert msgs.nbytes == int(off[-1]) + 64
        self.want = checker(sigs, pks, msgs, off)
        blob = msgs.tobytes()
        self.digests = np.frombuffer(b"".join(hashlib.sha256(blob[int(off[i]):int(off[i + 1])]).digest()
                                              for i in range(self.n)), np.uint8)

    def part(self, lo, n):
        """requests [lo, lo + n): the offsets slice is absolute into the whole message buffer"""
        return (self.sigs[64 * lo:64 * (lo + n)], self.pks[32 * lo:32 * (lo + n)], self.msgs, self.off[lo:lo + n + 1],
                self.want[lo:lo + n], self.digests[32 * lo:32 * (lo + n)])


def signed_pool(n=POOL_N, seed=0xD16E57, lens=None):
    """n requests signed by the oracle over messages of the lengths that cross
    SHA-256's padding and block edges, then a seeded spread of 0..700 B (or of
    the n lengths given); one in five damaged after signing (a flipped message byte, a flipped S bit, a
    small-order A), so a digest is owed for rejected requests too"""
    r = random.Random(seed)
    keys = [orc.keypair(bytes([k, seed & 255]) * 16) for k in range(16)]
    lens = lens or SPECIAL_LENS + [r.randrange(0, 701) for _ in range(n - len(SPECIAL_LENS))]
    sigs, pks, msgs = [], [], []
    for i, ln in enumerate(lens):
        pk, sk = keys[r.randrange(16)]
        m = bytearray(r.getrandbits(8 * ln).to_bytes(ln, "little"))
        sig = bytearray(orc.sign(bytes(m), sk))
        if i % 5 == 2:
            kind = (i // 5) % 3 if ln else 1 + (i // 5) % 2
            if kind == 0:
                m[r.randrange(ln)] ^= 1 << r.randrange(8)
            elif kind == 1:
                sig[32 + r.randrange(31)] ^= 1 << r.randrange(8)
            else:
                pk = SMALL_ORDER_A
        sigs.append(bytes(sig))
        pks.append(pk)
        msgs.append(bytes(m))
    off = np.zeros(n + 1, np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    # non-empty messages start at every offset mod 4 (the kernels read aligned words), within the first 400 already
    assert {int(o) % 4 for o, ln in zip(off[:400], lens) if ln} == {0, 1, 2, 3}
    return Batch(np.frombuffer(b"".join(sigs), np.uint8), np.frombuffer(b"".join(pks), np.uint8),
                 np.frombuffer(b"".join(msgs) + b"\0" * 64, np.uint8), off)


_cache = {}


def pool():
    if "pool" not in _cache:
        b = _cache["pool"] = signed_pool()
        rej = np.nonzero(b.want == 0)[0]
        assert np.array_equal(rej, np.arange(2, POOL_N, 5)), "exactly the damaged requests are rejected"
    return _cache["pool"]


def corpus_batch():
    """the two largest sizes: the seeded corpus, 200..4,096 B, a fifth invalid"""
    if "corpus" not in _cache:
        b = _cache["corpus"] = Batch(*orc.corpus(0xD16E, 0, 8193, mode=1, invalid_permille=200))
        assert 0.7 < b.want.mean() < 0.9
    return _cache["corpus"]


def requests_of(n):
    return (pool() if n <= POOL_N else corpus_batch()).part(0, n)


@pytest.fixture
def route():
    """Selects the route on device 0 for one test; the default limit is restored after."""
    def select(name):
        edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT if name == "latency" else 0)
    yield select
    edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT)


# ------------------------------------------------------------- buffer kinds
def _shifted(msgs, off, off0):
    """off[0] = off0 with the message pointer unchanged: off0 bytes no request owns, then the messages"""
    base = int(off[0])
    body = msgs[base:]
    if off0 == 0 and base == 0:
        return msgs, off
    return np.concatenate([np.full(off0, 0xEE, np.uint8), body]), off - np.uint64(base) + np.uint64(off0)


class Buffers:
    """One submission's buffers of one kind; .sigs .pks .msgs .off are arrays or
    addresses, .acc and .dig sentinel-filled arrays one verdict row / one digest
    longer than the batch."""

    def __init__(self, kind, sigs, pks, msgs, off, n):
        self.pins = []
        inputs, outs = kind
        if inputs == "pageable":
            self.sigs, self.pks, self.msgs, self.off = (np.ascontiguousarray(a) for a in (sigs, pks, msgs, off))
        elif inputs == "pinned3":
            self.sigs, self.pks, self.msgs, self.off = (self._pin(a) for a in (sigs, pks, msgs, off))
        else:
            assert inputs == "pinned1"
            # sigs | 16 | pks | 8 | offsets | up to the next 16 | msgs: the gaps keep (pks - sigs) % 16 == 0
            # and (offsets - sigs) % 8 == 0, what the single-copy branch asks for
            o_p, o_o = 64 * n + 16, 64 * n + 16 + 32 * n + 8
            o_m = (o_o + 8 * (n + 1) + 15) // 16 * 16
            pb = edv.PinnedBuffer(o_m + msgs.nbytes)
            self.pins.append(pb)
            pb.array[:] = 0x3C
            for o, a in ((0, sigs), (o_p, pks), (o_o, off), (o_m, msgs)):
                pb.array[o:o + a.nbytes] = np.ascontiguousarray(a).view(np.uint8)
            assert o_p % 16 == 0 and o_o % 8 == 0
            self.sigs, self.pks, self.off, self.msgs = pb.ptr, pb.ptr + o_p, pb.ptr + o_o, pb.ptr + o_m
        if outs == "pinned":
            pa, pd = edv.PinnedBuffer(n + 16), edv.PinnedBuffer(32 * n + 32)
            self.pins += [pa, pd]
            self.acc, self.dig = pa.array, pd.array
        else:
            self.acc, self.dig = np.empty(n + 16, np.uint8), np.empty(32 * n + 32, np.uint8)
        self.acc[:] = 7
        self.dig[:] = SENT
        self.n = n

    def _pin(self, a):
        a = np.ascontiguousarray(a).view(np.uint8)
        pb = edv.PinnedBuffer(max(a.nbytes, 1))
        self.pins.append(pb)
        pb.array[:a.nbytes] = a
        return pb.ptr

    def submit(self, digests=True, dev=0):
        return edv.verify_digest_async(self.sigs, self.pks, self.msgs, self.off, self.n, self.acc,
                                       self.dig if digests else None, dev)

    def check(self, want, digests, what, asked=True):
        n = self.n
        assert np.array_equal(self.acc[:n], want), (what, "verdicts", np.nonzero(self.acc[:n] != want)[0][:8].tolist())
        assert (self.acc[n:] == 7).all(), (what, "bytes past the last verdict")
        if asked:
            bad = np.nonzero((self.dig[:32 * n] != digests).reshape(n, 32).any(axis=1))[0]
            assert bad.size == 0, (what, "digests of requests", bad[:8].tolist())
            assert (self.dig[32 * n:] == SENT).all(), (what, "the 32 bytes past the last digest")
        else:
            assert (self.dig == SENT).all(), (what, "a digest buffer that was not asked for")

    def free(self):
        self.acc = self.dig = None
        for p in self.pins:
            p.free()


KINDS = [("pageable", "pageable"), ("pageable", "pinned"), ("pinned3", "pageable"), ("pinned1", "pinned")]


def run_route(n, kinds=KINDS):
    """-> digest comparisons made"""
    sigs, pks, msgs, off, want, digests = requests_of(n)
    done = 0
    for off0 in (0, 5):
        m, o = _shifted(msgs, off, off0)
        assert int(o[0]) == off0
        for kind in kinds:
            b = Buffers(kind, sigs, pks, m, o, n)
            edv.wait_async(b.submit())
            b.check(want, digests, (n, kind, off0))
            b.free()
            done += n
    return done


@pytest.mark.parametrize("name,n", ROUTES)
def test_digests_and_verdicts_on_every_route_and_buffer_kind(route, name, n):
    route(name)
    assert run_route(n) == 8 * n


def child_zero_copy_off():
    """(in the child process) the latency route with the pageable inputs DMA'd
    from the staging block instead of read in place"""
    assert os.environ.get("EDV_QUAD_ZERO_COPY") == "0"
    edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT)
    total = sum(run_route(n, kinds=KINDS[:1]) for _, n in LATENCY)
    print("zero-copy off: %d digests compared" % total)


def test_latency_route_with_zero_copy_off_in_a_child_process():
    env = dict(os.environ, EDV_QUAD_ZERO_COPY="0")
    code = "import sys; sys.path[:0] = [%r, %r]; import test_gpu_digest_routes as t; t.child_zero_copy_off()" % (ROOT, TESTS)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "zero-copy off: %d digests compared" % (2 * sum(n for _, n in LATENCY)) in r.stdout


# ------------------------------------------------------------------ slot reuse
REUSE_SIZES = [400, 3, 257, 1, 300, 2, 129, 5, 64, 17, 350, 4, 200, 16, 33, 1, 277, 7, 100, 2]
LAST_EIGHT = (5, 7, 4, 6, 1, 3, 0, 2)


def _poll(dev, t, limit_s=20.0):
    lib = edv.lib()
    t0 = time.time()
    while True:
        rc = lib.edv_query_async(dev, t)
        if rc != edv.EDV_PENDING:
            return rc
        assert time.time() - t0 < limit_s, "batch never completed"


@pytest.mark.parametrize("name", ["latency", "own"])
def test_slot_reuse_keeps_every_batchs_own_digests(route, name):
    """Twenty batches on the eight slots with no wait between submissions: the
    first twelve are handed over when their slot is reused (async_complete's
    copies out of the slot's staging, sized by that batch's n, before a smaller
    or larger batch takes the slot), the last eight by edv_wait_async and
    edv_query_async in another order than they were submitted."""
    route(name)
    lib = edv.lib()
    p = pool()
    assert len(REUSE_SIZES) == 20
    batches, lo = [], 0
    for k, n in enumerate(REUSE_SIZES):
        sigs, pks, msgs, off, want, digests = p.part(lo, n)
        lo += n
        b = Buffers(("pageable", "pinned" if k % 2 == 0 else "pageable"), sigs, pks, msgs, off, n)
        batches.append((b, want, digests, k % 3 != 2))
    tickets = [b.submit(digests=asked) for b, _w, _d, asked in batches]
    assert tickets == list(range(tickets[0], tickets[0] + 20))
    for i, j in enumerate(LAST_EIGHT):
        t = tickets[12 + j]
        assert (_poll(0, t) if i % 2 else lib.edv_wait_async(0, t)) == edv.EDV_OK
    for t in tickets:
        assert lib.edv_wait_async(0, t) == edv.EDV_OK and lib.edv_query_async(0, t) == edv.EDV_OK
    for k, (b, want, digests, asked) in enumerate(batches):
        b.check(want, digests, ("batch", k, "of", b.n), asked=asked)
        b.free()


# --------------------------------------------------------------- empty batches
@pytest.mark.parametrize("name", ["latency", "own"])
def test_empty_batches_and_empty_messages(route, name):
    route(name)
    lib = edv.lib()
    dig = np.full(64, SENT, np.uint8)
    acc = np.full(16, 7, np.uint8)
    one = np.zeros(1, np.uint64)
    t = ctypes.c_int64(-1)
    assert lib.edv_verify_digest_batch_async(None, None, None, one.ctypes.data, 0, acc.ctypes.data, dig.ctypes.data,
                                             0, ctypes.byref(t)) == edv.EDV_OK
    assert t.value >= 0 and lib.edv_wait_async(0, t.value) == edv.EDV_OK
    assert (dig == SENT).all() and (acc == 7).all()
    # n empty messages: n times sha256(b""), signatures over the empty message, one of them damaged
    empty = hashlib.sha256(b"").digest()
    for n in (5, 17):
        keys = [orc.keypair(bytes([k, n]) * 16) for k in range(n)]
        sigs = bytearray(b"".join(orc.sign(b"", sk) for _pk, sk in keys))
        sigs[64 * (n - 2) + 40] ^= 4
        sigs = np.frombuffer(bytes(sigs), np.uint8)
        pks = np.frombuffer(b"".join(pk for pk, _sk in keys), np.uint8)
        msgs, off = np.zeros(64, np.uint8), np.zeros(n + 1, np.uint64)
        want = checker(sigs, pks, msgs, off)
        assert want.tolist() == [1] * (n - 2) + [0, 1]
        for kind in KINDS[:2]:
            b = Buffers(kind, sigs, pks, msgs, off, n)
            edv.wait_async(b.submit())
            b.check(want, np.frombuffer(empty * n, np.uint8), ("empty messages", n, kind))
            b.free()
