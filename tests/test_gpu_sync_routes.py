"""The verdicts of the synchronous edv_verify_batch on every route of
run_shard (csrc/edv_runtime.hip) and every buffer kind: the synchronous
counterpart of test_gpu_digest_routes' table, on its buffers.

  route                      reached by                                    n      requests
  right-to-left kernel       the default latency limit                     1, 17  pool
  two-walk kernel            the default latency limit                     4,097  pool
  field path                 set_latency_path(0, 0)                        257    pool
  field path in slices       ... and set_host_slices(0, 3)                 1,025  one block count
  field path, bucketed       ... and set_host_slices(0, 3)                 1,025  pool
  sub-batch path             ... and set_chunk(0, 512)                     1,025  pool

The sizes are the smallest that reach each branch.  The field path cuts a
shard into slices only when every message has one SHA-512 block count (a
bucketed shard is one slice), and the pool's 0..700 B and 4,096 B messages do
not: the slices route takes 1,025 requests of its own, signed and damaged like
the pool's, with messages of 48..175 B (two blocks each, asserted; starting at
every offset mod 4), so that three slices [0, 256), [256, 512), [512, 1025)
are copied, and staged when pageable, one by one and hashed on three streams.
The same setting on the pool is the bucketed case: one slice, hashed after the
permutation.  With a chunk of 512 the 1,025 are five sub-batches of 256 on two
streams, the last of one request.  Each (route, n) runs inputs pageable with
verdicts pageable and page-locked, inputs page-locked in three regions, and
inputs page-locked in ONE region sigs | 16 | pks | 8 | offsets (the
single-copy branch), each with off[0] = 0 and off[0] = 5.  Every verdict equals
the checker's (the damaged fifth rejected: asserted for both sets of requests
that exactly requests 2, 7, 12, ... are), the sentinel bytes past the last
verdict stay, and the parts of edv_context_memory add up after each route.

Measured on MI355X, run together with test_gpu_digest_routes (22 tests in
2.4 s): the first case here 0.35 s (it signs the pool, which both files share),
[slices-1025] 0.06 s (it signs its 1,025 requests), every other case at most
0.03 s.
"""
import numpy as np
import pytest

from indy_plenum_amd import edv
import random

from test_gpu_digest_routes import KINDS, Buffers, _shifted, pool, signed_pool

pytestmark = pytest.mark.gpu

# (name, n, latency path on, host slices, chunk)
ROUTES = [("rtl", 1, True, 0, 0), ("rtl", 17, True, 0, 0), ("two-walk", 4097, True, 0, 0),
          ("fields", 257, False, 0, 0), ("slices", 1025, False, 3, 0), ("bucketed", 1025, False, 3, 0),
          ("sub-batches", 1025, False, 0, 512)]
_cache = {}


def sha512_blocks(off):
    """SHA-512 blocks of each request's hash input: R, A, the message and the padding"""
    return (64 + np.diff(off.astype(np.int64)) + 17 + 127) // 128


def one_block_count_pool(n=1025):
    """n requests whose messages all hash in two SHA-512 blocks, so the field path does not bucket them"""
    if "uniform" not in _cache:
        r = random.Random(0x51CE5)
        b = _cache["uniform"] = signed_pool(n, seed=0x51CE57, lens=[48 + r.randrange(128) for _ in range(n)])
        assert np.array_equal(np.nonzero(b.want == 0)[0], np.arange(2, n, 5)), "exactly the damaged requests are rejected"
    return _cache["uniform"]


@pytest.fixture
def settings():
    """Selects a route on device 0 for one test; the defaults are restored after."""
    def select(latency, slices, chunk):
        edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT if latency else 0)
        edv.set_host_slices(0, slices)
        edv.set_chunk(0, chunk)
    yield select
    select(True, 0, 0)


def _addr(a):
    return a.ctypes.data if isinstance(a, np.ndarray) else a


@pytest.mark.parametrize("name,n,latency,slices,chunk", ROUTES, ids=["%s-%d" % r[:2] for r in ROUTES])
def test_verdicts_on_every_sync_route_and_buffer_kind(settings, name, n, latency, slices, chunk):
    settings(latency, slices, chunk)
    lib = edv.lib()
    sigs, pks, msgs, off, want, _digests = (one_block_count_pool(n) if name == "slices" else pool()).part(0, n)
    # what decides between slices and buckets on the field path: one SHA-512 block count or several
    assert (len(set(sha512_blocks(off).tolist())) == 1) == (name == "slices") or n < 17
    assert 0 < want.sum() < n or n == 1, "accepted and rejected requests both"
    for off0 in (0, 5):
        m, o = _shifted(msgs, off, off0)
        assert int(o[0]) == off0
        for kind in KINDS:
            b = Buffers(kind, sigs, pks, m, o, n)
            edv._check(lib.edv_verify_batch(_addr(b.sigs), _addr(b.pks), _addr(b.msgs), _addr(b.off), n,
                                            b.acc.ctypes.data, 1))
            b.check(want, None, (name, n, kind, off0), asked=False)
            b.free()
    mem = edv.context_memory(0)
    assert mem["total"] == sum(v for k, v in mem.items() if k != "total") and mem["sync_inputs"] > 0, mem
