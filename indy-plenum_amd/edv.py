"""ctypes binding of the gfx950 batch verifier C-ABI (include/edv.h, libedv.so).

This is the thin shim between Plenum's authenticator layer (client_authn.py,
req_authenticator.py, verifier.py, nacl_wrappers.py in this package) and the
HIP kernels.  There is no CPU fallback here: if libedv.so is missing or no
gfx950 device is visible, every call raises EdvUnavailable, loudly.

Reference behaviour reproduced at this layer:
  stp_core/crypto/nacl_wrappers.py:232-242  Verifier.verify(signature, msg)
      -> crypto_sign_open(signature + msg, pk): the first 64 bytes of the
         CONCATENATION are the signature and the rest is the message, so a
         non-64-byte "signature" re-splits positionally (open_batch below);
         fewer than 64 bytes in total rejects (libsodium: smlen < 64).
"""
import ctypes
import os
import threading

import numpy as np

from . import _edvhost  # native host-side packing (csrc/edv_host.cpp, row f-1)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("EDV_LIB", os.path.join(_HERE, "libedv.so"))
# the benchmark/profiling build (include/edv_measure.h): loaded only by the
# measurement helpers below (bench.py, tools/, the GPU tests' fault hook),
# never by the authenticators
MEASURE_LIB_PATH = os.path.join(_HERE, "libedv_measure.so")
MEASUREMENT_TAG = "MEASUREMENT-ONLY"  # in edv_version() of builds whose verdicts are not libsodium's

EDV_OK = 0
EDV_E_ARG = -1
EDV_E_NODEV = -2
EDV_E_HIP = -3
EDV_E_OOM = -4
EDV_E_BUSY = -5      # trim / release: batches not yet handed over still own caller buffers
EDV_E_SELFTEST = -6  # self_test / prepare: a verdict differs from libsodium's
TABLES_AUTO, TABLES_COMPACT, TABLES_LARGE = 0, 1, 2   # set_table_policy
SELFTEST_RTL, SELFTEST_TWO_WALK, SELFTEST_BATCH = 1, 2, 4
SELFTEST_ALL = 7
PREPARE_ASYNC = 1
FLAG_UNIFORM_LENGTH = 1  # every message has the same SHA-512 block count: no length buckets
FLAG_BUCKETS = 2         # always bucket by SHA-512 block count
FLAG_SPLIT_PREP = 4      # pipelined path: batch k+1's hash side beside batch k's main kernel


class EdvUnavailable(RuntimeError):
    """libedv.so cannot be loaded or no gfx950 device is visible."""


class EdvError(RuntimeError):
    """The C-ABI returned an error code."""

    def __init__(self, code, what):
        super().__init__("edv error {}: {}".format(code, what))
        self.code = code


_lock = threading.Lock()
_lib = None


def lib():
    """The loaded libedv.so (raises EdvUnavailable if it is not built)."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise EdvUnavailable("libedv.so not built at {} (run __graft_entry__.build())".format(LIB_PATH))
        h = ctypes.CDLL(LIB_PATH)
        h.edv_version.restype = ctypes.c_char_p
        ver = h.edv_version().decode(errors="replace")
        if MEASUREMENT_TAG in ver and os.environ.get("EDV_ALLOW_MEASUREMENT_LIB") != "1":
            # a measurement build (e.g. variants/libedv_noverify.so reports every
            # signature valid) must never authenticate requests: fail closed,
            # as the reference's Verifier never returns True without libsodium's
            # check (nacl_wrappers.py:232-242)
            raise EdvUnavailable("{} is a measurement-only build ({}); refusing to load it "
                                 "(EDV_ALLOW_MEASUREMENT_LIB=1 is for benchmarks only)".format(LIB_PATH, ver))
        vp, u64 = ctypes.c_void_p, ctypes.c_uint64
        h.edv_verify_batch.argtypes = [vp, vp, vp, vp, u64, vp, ctypes.c_uint32]
        h.edv_verify_batch.restype = ctypes.c_int
        h.edv_verify_batch_dev.argtypes = [vp, vp, vp, vp, u64, u64, vp, ctypes.c_int, vp]
        h.edv_verify_batch_dev.restype = ctypes.c_int
        h.edv_sha256_batch.argtypes = [vp, vp, u64, vp, ctypes.c_uint32]
        h.edv_sha256_batch.restype = ctypes.c_int
        h.edv_sha256_batch_dev.argtypes = [vp, vp, u64, u64, vp, ctypes.c_int, vp]
        h.edv_sha256_batch_dev.restype = ctypes.c_int
        h.edv_merkle_extend.argtypes = [u64, vp, vp, vp, u64, vp, vp, vp, vp, ctypes.c_int]
        h.edv_merkle_extend.restype = ctypes.c_int
        h.edv_merkle_extend_dev.argtypes = [u64, vp, vp, vp, u64, u64, vp, vp, vp, vp, ctypes.c_int, vp]
        h.edv_merkle_extend_dev.restype = ctypes.c_int
        h.edv_merkle_append_batch.argtypes = [u64, vp, vp, vp, u64, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        h.edv_merkle_append_batch.restype = ctypes.c_int
        h.edv_merkle_append_batch_dev.argtypes = [u64, vp, vp, vp, u64, u64, vp, vp, vp, vp, vp, vp, ctypes.c_int, vp]
        h.edv_merkle_append_batch_dev.restype = ctypes.c_int
        h.edv_merkle_path_entries.argtypes = [u64, u64, ctypes.POINTER(u64)]
        h.edv_merkle_path_entries.restype = ctypes.c_int
        h.edv_merkle_verify_inclusion.argtypes = [vp] * 8 + [u64, vp, vp, ctypes.c_int]
        h.edv_merkle_verify_inclusion.restype = ctypes.c_int
        h.edv_merkle_verify_inclusion_dev.argtypes = [vp, vp, u64, vp, vp, vp, vp, vp, vp, u64, u64, vp, vp,
                                                      ctypes.c_int, vp]
        h.edv_merkle_verify_inclusion_dev.restype = ctypes.c_int
        h.edv_merkle_verify_consistency.argtypes = [vp] * 6 + [u64, vp, vp, ctypes.c_int]
        h.edv_merkle_verify_consistency.restype = ctypes.c_int
        h.edv_merkle_verify_consistency_dev.argtypes = [vp] * 6 + [u64, u64, vp, vp, ctypes.c_int, vp]
        h.edv_merkle_verify_consistency_dev.restype = ctypes.c_int
        for f in (h.edv_merkle_inclusion_offsets, h.edv_merkle_consistency_offsets):
            f.argtypes = [vp, vp, u64, u64, vp]
            f.restype = ctypes.c_int
        for f in (h.edv_merkle_prove_inclusion, h.edv_merkle_prove_consistency):
            f.argtypes = [vp, vp, u64, vp, vp, vp, u64, vp, vp, vp, vp, ctypes.c_int]
            f.restype = ctypes.c_int
        for f in (h.edv_merkle_prove_inclusion_dev, h.edv_merkle_prove_consistency_dev):
            f.argtypes = [vp, vp, u64, vp, vp, vp, u64, u64, vp, vp, vp, vp, ctypes.c_int, vp]
            f.restype = ctypes.c_int
        h.edv_merkle_audit_nodes.argtypes = [vp, vp, u64, u64, u64, vp, vp, ctypes.c_int]
        h.edv_merkle_audit_nodes_dev.argtypes = [vp, vp, u64, u64, u64, vp, vp, ctypes.c_int, vp]
        h.edv_merkle_audit_leaves.argtypes = [vp, u64, u64, vp, vp, u64, vp, vp, ctypes.c_int]
        h.edv_merkle_audit_leaves_dev.argtypes = [vp, u64, u64, vp, vp, u64, u64, vp, vp, ctypes.c_int, vp]
        h.edv_merkle_extend_hashed.argtypes = [u64, vp, vp, u64, vp, vp, vp, ctypes.c_int]
        h.edv_merkle_extend_hashed_dev.argtypes = [u64, vp, vp, u64, vp, vp, vp, ctypes.c_int, vp]
        for f in (h.edv_merkle_audit_nodes, h.edv_merkle_audit_nodes_dev, h.edv_merkle_audit_leaves,
                  h.edv_merkle_audit_leaves_dev, h.edv_merkle_extend_hashed, h.edv_merkle_extend_hashed_dev):
            f.restype = ctypes.c_int
        h.edv_merkle_catchup.argtypes = [u64, vp, vp, vp, u64, vp, u64, u64, vp, vp, vp, vp, vp, vp, vp, ctypes.c_int]
        h.edv_merkle_catchup.restype = ctypes.c_int
        h.edv_merkle_catchup_dev.argtypes = [u64, vp, vp, vp, u64, u64, vp, u64, u64, vp, vp, vp, u64, vp, vp, vp, vp,
                                             ctypes.c_int, vp]
        h.edv_merkle_catchup_dev.restype = ctypes.c_int
        h.edv_verify_batch_dev_flags.argtypes = [vp, vp, vp, vp, u64, u64, vp, ctypes.c_int, vp, ctypes.c_uint32]
        h.edv_verify_batch_dev_flags.restype = ctypes.c_int
        h.edv_verify_batch_dev_pipelined.argtypes = [vp, vp, vp, vp, u64, u64, vp, ctypes.c_int, ctypes.c_uint32]
        h.edv_verify_batch_dev_pipelined.restype = ctypes.c_int
        h.edv_verify_batch_async.argtypes = [vp, vp, vp, vp, u64, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
        h.edv_verify_batch_async.restype = ctypes.c_int
        h.edv_verify_digest_batch_async.argtypes = [vp, vp, vp, vp, u64, vp, vp, ctypes.c_int,
                                                    ctypes.POINTER(ctypes.c_int64)]
        h.edv_verify_digest_batch_async.restype = ctypes.c_int
        h.edv_wait_async.argtypes = [ctypes.c_int, ctypes.c_int64]
        h.edv_wait_async.restype = ctypes.c_int
        h.edv_query_async.argtypes = [ctypes.c_int, ctypes.c_int64]
        h.edv_query_async.restype = ctypes.c_int
        h.edv_pipeline_sync.argtypes = [ctypes.c_int]
        h.edv_pipeline_sync.restype = ctypes.c_int
        h.edv_sign_batch_dev.argtypes = [vp, vp, vp, u64, u64, vp, vp, ctypes.c_int, vp]
        h.edv_sign_batch_dev.restype = ctypes.c_int
        h.edv_stream.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_void_p)]
        h.edv_stream.restype = ctypes.c_int
        h.edv_sync.argtypes = [ctypes.c_int]
        h.edv_sync.restype = ctypes.c_int
        h.edv_set_latency_path.argtypes = [ctypes.c_int, u64]
        h.edv_set_latency_path.restype = ctypes.c_int
        h.edv_set_length_buckets.argtypes = [ctypes.c_int, ctypes.c_int]
        h.edv_set_length_buckets.restype = ctypes.c_int
        h.edv_set_chunk.argtypes = [ctypes.c_int, u64]
        h.edv_set_chunk.restype = ctypes.c_int
        h.edv_set_host_slices.argtypes = [ctypes.c_int, ctypes.c_int]
        h.edv_set_host_slices.restype = ctypes.c_int
        h.edv_shard_split.argtypes = [vp, u64, ctypes.c_uint32, vp]
        h.edv_shard_split.restype = ctypes.c_int
        h.edv_host_alloc.argtypes = [u64, ctypes.POINTER(ctypes.c_void_p)]
        h.edv_host_alloc.restype = ctypes.c_int
        h.edv_host_free.argtypes = [vp]
        h.edv_host_free.restype = ctypes.c_int
        h.edv_device_count.argtypes = []
        h.edv_device_count.restype = ctypes.c_int
        h.edv_context_count.argtypes = []
        h.edv_context_count.restype = ctypes.c_int
        h.edv_pick_device.argtypes = [ctypes.c_uint32]
        h.edv_pick_device.restype = ctypes.c_int
        h.edv_pack_bits_dev.argtypes = [vp, u64, vp, ctypes.c_int, vp]
        h.edv_pack_bits_dev.restype = ctypes.c_int
        h.edv_context_memory.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        h.edv_context_memory.restype = ctypes.c_int
        h.edv_set_table_policy.argtypes = [ctypes.c_int, ctypes.c_int]
        h.edv_set_table_policy.restype = ctypes.c_int
        h.edv_table_state.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_uint64)]
        h.edv_table_state.restype = ctypes.c_int
        h.edv_self_test.argtypes = [ctypes.c_int, ctypes.c_uint32]
        h.edv_self_test.restype = ctypes.c_int
        h.edv_prepare.argtypes = [ctypes.c_int, u64, ctypes.c_uint32]
        h.edv_prepare.restype = ctypes.c_int
        h.edv_trim.argtypes = [ctypes.c_int, u64]
        h.edv_trim.restype = ctypes.c_int
        h.edv_release.argtypes = [ctypes.c_int]
        h.edv_release.restype = ctypes.c_int
        h.edv_dev_alloc.argtypes = [ctypes.c_int, u64, ctypes.POINTER(ctypes.c_void_p)]
        h.edv_dev_free.argtypes = [ctypes.c_int, vp]
        h.edv_h2d.argtypes = [ctypes.c_int, vp, vp, u64]
        h.edv_d2h.argtypes = [ctypes.c_int, vp, vp, u64]
        h.edv_version.restype = ctypes.c_char_p
        h.edv_last_error.restype = ctypes.c_char_p
        _lib = h
        return h


_mlib = None


def measure_lib():
    """libedv_measure.so: the same verifier plus kernel timing and the fault hook
    (include/edv_measure.h).  Its device contexts are its own (a second [S]B
    table set and scratch per GPU in this process); device pointers from either
    library may be passed to the other."""
    global _mlib
    if _mlib is not None:
        return _mlib
    with _lock:
        if _mlib is not None:
            return _mlib
        if not os.path.exists(MEASURE_LIB_PATH):
            raise EdvUnavailable("libedv_measure.so not built at {} (run __graft_entry__.build())"
                                 .format(MEASURE_LIB_PATH))
        h = ctypes.CDLL(MEASURE_LIB_PATH)
        vp, u64, f32p = ctypes.c_void_p, ctypes.c_uint64, ctypes.POINTER(ctypes.c_float)
        h.edv_time_batch_dev.argtypes = [vp, vp, vp, vp, u64, u64, vp, ctypes.c_int, ctypes.c_int, f32p]
        h.edv_profile_batch_dev.argtypes = [vp, vp, vp, vp, u64, u64, vp, ctypes.c_int, ctypes.c_int, f32p, f32p]
        h.edv_profile_batch_dev_flush.argtypes = [vp, vp, vp, vp, u64, u64, vp, ctypes.c_int, ctypes.c_int, u64,
                                                  f32p, f32p, f32p]
        h.edv_profile_prep_sides.argtypes = [vp, vp, vp, vp, u64, u64, vp, ctypes.c_int, ctypes.c_int, f32p]
        h.edv_test_fail_async.argtypes = [ctypes.c_int, ctypes.c_int64]
        h.edv_probe_math.argtypes = [ctypes.c_int, ctypes.c_int, vp, u64, vp, u64, u64]
        h.edv_probe_prep_state.argtypes = [ctypes.c_int, vp, vp, vp, vp, u64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_uint32, vp, vp, vp, vp, vp, vp, ctypes.POINTER(u64)]
        h.edv_probe_main_state.argtypes = [ctypes.c_int, u64, u64, vp, vp, vp, vp, vp, ctypes.c_uint32, vp]
        h.edv_probe_table.argtypes = [ctypes.c_int, ctypes.c_int, vp, u64, vp]
        h.edv_probe_latency_phase1.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_int, vp, vp, vp, vp, u64, vp, vp,
                                               vp, vp]
        h.edv_probe_latency_walk.argtypes = [ctypes.c_int, ctypes.c_int, u64, u64, vp, vp, vp, ctypes.c_uint32, vp]
        h.edv_verify_batch_async.argtypes = [vp, vp, vp, vp, u64, vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int64)]
        h.edv_wait_async.argtypes = [ctypes.c_int, ctypes.c_int64]
        h.edv_last_error.restype = ctypes.c_char_p
        h.edv_version.restype = ctypes.c_char_p
        _mlib = h
        return h


def _mcheck(rc):
    if rc != EDV_OK:
        what = measure_lib().edv_last_error().decode(errors="replace")
        if rc == EDV_E_NODEV:
            raise EdvUnavailable(what)
        raise EdvError(rc, what)


def version() -> str:
    return lib().edv_version().decode()


CONTEXT_MEMORY_FIELDS = ("total", "sb_tables", "chunk_scratch", "async_slots", "pipelined_sets", "sync_inputs",
                         "signer_comb")


def context_memory(device: int = 0) -> dict:
    """Device bytes the library holds for `device` in this process
    (edv_context_memory), by kind; all zero before the context exists."""
    out = (ctypes.c_uint64 * 7)()
    _check(lib().edv_context_memory(device, out))
    return dict(zip(CONTEXT_MEMORY_FIELDS, (int(x) for x in out)))


TABLE_STATE_FIELDS = ("policy", "compact_bytes", "large_bytes", "large_failed")


def set_table_policy(device: int, policy: int):
    """Which [S]B table set the next batches of `device` use: TABLES_AUTO,
    TABLES_COMPACT or TABLES_LARGE (edv_set_table_policy).  Never changes verdicts."""
    _check(lib().edv_set_table_policy(device, policy))


def table_state(device: int = 0) -> dict:
    """The table policy of `device`, the bytes of the compact and of the large
    set its context holds, and whether a build of the large set has failed and
    is not being retried (edv_table_state)."""
    out = (ctypes.c_uint64 * 4)()
    _check(lib().edv_table_state(device, out))
    return dict(zip(TABLE_STATE_FIELDS, (int(x) for x in out)))


def self_test(device: int = 0, families: int = SELFTEST_ALL):
    """Known-answer test of the kernel families in `families` (SELFTEST_*) on
    `device`; raises EdvError(EDV_E_SELFTEST) if a verdict is not libsodium's."""
    _check(lib().edv_self_test(device, families))


def prepare(device: int = 0, max_batch: int = 400, flags: int = 0):
    """Create the context of `device`, build and grow what batches of up to
    max_batch requests need (flags: PREPARE_ASYNC for the asynchronous slots
    too) and self-test the kernels they take (edv_prepare)."""
    _check(lib().edv_prepare(device, max_batch, flags))


def trim(device: int = 0, keep_batch: int = 0):
    """Free what is larger than a batch of keep_batch needs and the table sets
    the policy would not pick for it; EdvError(EDV_E_BUSY) while asynchronous
    batches are not handed over (edv_trim)."""
    _check(lib().edv_trim(device, keep_batch))


def release(device: int = 0):
    """Destroy the context of `device`; its settings stay, the next call makes
    a fresh one; EdvError(EDV_E_BUSY) as for trim (edv_release)."""
    _check(lib().edv_release(device))


def device_count() -> int:
    return lib().edv_device_count()


def context_count() -> int:
    """Devices whose context the library has initialised (placement tests)."""
    return lib().edv_context_count()


def pick_device(device_mask: int = 0) -> int:
    """The device edv_pick_device chooses for a one-device batch (include/edv.h)."""
    d = lib().edv_pick_device(device_mask)
    if d < 0:
        _check(d)
    return d


def batch_device() -> int:
    """Device of the next native asynchronous whole-batch submission: BATCH_DEVICE
    if set, else the library's choice among BATCH_DEVICE_MASK (an idle
    initialised device, else a fresh one), so the Nodes of one process spread
    over the GPUs while a lone caller stays on one context."""
    return BATCH_DEVICE if BATCH_DEVICE is not None else pick_device(BATCH_DEVICE_MASK)


def stream(device: int = 0) -> int:
    """The library's HIP stream of `device` (for asynchronous edv_*_dev calls)."""
    p = ctypes.c_void_p()
    _check(lib().edv_stream(device, ctypes.byref(p)))
    return p.value


def sync(device: int = 0):
    """Wait for everything enqueued on the library stream of `device`."""
    _check(lib().edv_sync(device))


def set_length_buckets(device: int, mode: int):
    """SHA-512 length buckets on the device paths: 0 never, 1 always, 2 auto (default)."""
    _check(lib().edv_set_length_buckets(device, mode))


LATENCY_PATH_DEFAULT = 16384


def set_latency_path(device: int, max_requests: int):
    """Batches of at most max_requests (0 = never) run on the latency kernels:
    sixteen lanes per signature up to 4,096 requests, eight above
    (edv_set_latency_path).  Never changes verdicts."""
    _check(lib().edv_set_latency_path(device, max_requests))


def set_chunk(device: int, chunk: int):
    """Signatures per prep/main kernel pair (0 = default).  Never changes verdicts."""
    _check(lib().edv_set_chunk(device, chunk))


def set_host_slices(device: int, slices: int):
    """Message slices of a synchronous one-chunk shard (edv_set_host_slices; 0 = default)."""
    _check(lib().edv_set_host_slices(device, slices))


def _check(rc):
    if rc != EDV_OK:
        what = lib().edv_last_error().decode(errors="replace")
        if rc == EDV_E_NODEV:
            raise EdvUnavailable(what)
        raise EdvError(rc, what)


def verify_arrays(sigs, pks, msgs, offsets, device_mask: int = 0) -> np.ndarray:
    """Verify n detached 64-byte signatures laid out as the C-ABI expects.

    sigs: n*64 bytes, pks: n*32 bytes, msgs: concatenated messages, offsets:
    n+1 uint64 byte offsets.  Returns a uint8 array of n verdicts (1 = accept),
    bit-exact with libsodium crypto_sign_ed25519_verify_detached.
    """
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(off) - 1
    if n <= 0:
        return np.zeros(0, dtype=np.uint8)
    sigs = np.frombuffer(bytes(sigs), dtype=np.uint8) if not isinstance(sigs, np.ndarray) else sigs
    pks = np.frombuffer(bytes(pks), dtype=np.uint8) if not isinstance(pks, np.ndarray) else pks
    if not isinstance(msgs, np.ndarray):
        msgs = np.frombuffer(bytes(msgs) or b"\0", dtype=np.uint8)
    if sigs.nbytes != 64 * n or pks.nbytes != 32 * n:
        raise ValueError("sigs/pks size does not match offsets")
    if int(off[-1]) > msgs.nbytes:
        raise ValueError("offsets exceed the message buffer")
    accept = np.zeros(n, dtype=np.uint8)
    _check(lib().edv_verify_batch(sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, off.ctypes.data, n,
                                  accept.ctypes.data, device_mask))
    return accept


def verify_async(sigs: np.ndarray, pks: np.ndarray, msgs: np.ndarray, offsets: np.ndarray, accept: np.ndarray,
                 device: int = 0) -> int:
    """Queue one host batch (edv_verify_batch_async) and return its ticket.

    The arrays (uint8 sigs/pks/msgs/accept, uint64 offsets, C-ABI layout) must
    stay alive and unchanged, and `accept` unread, until wait_async(ticket)."""
    off = offsets
    n = len(off) - 1
    if off.dtype != np.uint64 or not off.flags.c_contiguous:
        raise ValueError("offsets must be a contiguous uint64 array")
    if sigs.nbytes != 64 * n or pks.nbytes != 32 * n or accept.nbytes < n:
        raise ValueError("sigs/pks/accept size does not match offsets")
    if n > 0 and int(off[-1]) > msgs.nbytes:
        raise ValueError("offsets exceed the message buffer")
    t = ctypes.c_int64(-1)
    _check(lib().edv_verify_batch_async(sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, off.ctypes.data, n,
                                        accept.ctypes.data, device, ctypes.byref(t)))
    return t.value


def verify_digest_async(sigs, pks, msgs, offsets, n: int, accept, digests=None, device: int = 0) -> int:
    """Queue one host batch with its SHA-256 digests (edv_verify_digest_batch_async)
    and return its ticket.  Every buffer is a numpy array or a raw address (a
    PinnedBuffer's .ptr plus an offset); digests None passes NULL.  No size
    checks: the caller owns the layout, and the buffers until wait_async."""
    def addr(a):
        return a.ctypes.data if isinstance(a, np.ndarray) else a
    t = ctypes.c_int64(-1)
    _check(lib().edv_verify_digest_batch_async(addr(sigs), addr(pks), addr(msgs), addr(offsets), n, addr(accept),
                                               None if digests is None else addr(digests), device,
                                               ctypes.byref(t)))
    return t.value


def wait_async(ticket: int, device: int = 0) -> None:
    """Wait until batch `ticket` has its verdicts in its accept array."""
    _check(lib().edv_wait_async(device, ticket))


EDV_PENDING = 1


def query_async(ticket: int, device: int = 0) -> bool:
    """wait_async without the wait: False while batch `ticket` is still on the
    GPU, True once it is done (its verdicts then handed over, as wait_async
    would); raises as wait_async would for a failed batch."""
    rc = lib().edv_query_async(device, ticket)
    if rc == EDV_PENDING:
        return False
    _check(rc)
    return True


def sha256_arrays(msgs, offsets, device_mask: int = 0) -> np.ndarray:
    """SHA-256 of n messages in the C-ABI layout -> (n, 32) uint8 digests (row f-3)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(off) - 1
    if n <= 0:
        return np.zeros((0, 32), dtype=np.uint8)
    if not isinstance(msgs, np.ndarray):
        msgs = np.frombuffer(bytes(msgs) or b"\0", dtype=np.uint8)
    if int(off[-1]) > msgs.nbytes:
        raise ValueError("offsets exceed the message buffer")
    out = np.zeros((n, 32), dtype=np.uint8)
    _check(lib().edv_sha256_batch(msgs.ctypes.data, off.ctypes.data, n, out.ctypes.data, device_mask))
    return out


def sha256_batch(messages, device_mask: int = 0):
    """list[bytes] -> list[32-byte digest] (hashlib.sha256(m).digest() for each m)."""
    messages = list(messages)
    if not messages:
        return []
    off = np.zeros(len(messages) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in messages])
    d = sha256_arrays(b"".join(messages), off, device_mask)
    return [bytes(r) for r in d]


def pack_bits_device(d_accept, n, d_bits, device=0, stream=None):
    """Device accept bytes -> bitmask (ceil(n/8) bytes, little-endian bit order)."""
    _check(lib().edv_pack_bits_dev(d_accept, n, d_bits, device, stream))


def sha256_device(d_msgs, d_off, n, d_out, device=0, msg_base=0, stream=None):
    """Device-resident batch SHA-256: d_out gets n x 32 bytes."""
    _check(lib().edv_sha256_batch_dev(d_msgs, d_off, msg_base, n, d_out, device, stream))


MERKLE_MAX_LEAVES = 1 << 22  # EDV_MERKLE_MAX_LEAVES: leaves per edv_merkle_extend call
MERKLE_MAX_SIZE = 1 << 62


def merkle_node_span(old_size: int, n: int) -> int:
    """Interior nodes that n appends to a tree of old_size leaves create."""
    new = old_size + n
    return (new - bin(new).count("1")) - (old_size - bin(old_size).count("1"))


def _merkle_call(old_size, old_hashes, leaves, offsets, want_leaf_hashes, want_node_hashes):
    """The checked inputs and the zeroed outputs that merkle_extend and
    merkle_append_batch share: (old_size, n, the C call's first five arguments,
    leaf_h, node_h, new_h, root)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError("offsets must hold n + 1 entries")
    n = len(off) - 1
    old_size = int(old_size)
    if old_size < 0 or old_size + n > MERKLE_MAX_SIZE:
        raise ValueError("tree size out of range")
    if n > MERKLE_MAX_LEAVES:
        raise ValueError("more than MERKLE_MAX_LEAVES leaves in one call")
    if not isinstance(old_hashes, np.ndarray):
        old_hashes = np.frombuffer(bytes(old_hashes), dtype=np.uint8)
    if old_hashes.dtype != np.uint8 or not old_hashes.flags.c_contiguous:
        raise ValueError("old_hashes must be contiguous uint8")
    if old_hashes.nbytes != 32 * bin(old_size).count("1"):
        raise ValueError("old_hashes size does not match old_size")
    if not isinstance(leaves, np.ndarray):
        leaves = np.frombuffer(bytes(leaves) or b"\0", dtype=np.uint8)
    if leaves.dtype != np.uint8 or not leaves.flags.c_contiguous:
        raise ValueError("leaves must be contiguous uint8")
    if int(off[-1]) > leaves.nbytes:
        raise ValueError("offsets exceed the leaf buffer")
    new_size = old_size + n
    leaf_h = np.zeros((n, 32), dtype=np.uint8) if want_leaf_hashes else None
    node_h = np.zeros((merkle_node_span(old_size, n), 32), dtype=np.uint8) if want_node_hashes else None
    new_h = np.zeros((bin(new_size).count("1"), 32), dtype=np.uint8)
    root = np.zeros(32, dtype=np.uint8)
    head = (old_size, old_hashes.ctypes.data if old_hashes.nbytes else None, leaves.ctypes.data, off.ctypes.data, n)
    # old_hashes, leaves and off are returned so that they outlive the call
    return old_size, n, head, (old_hashes, leaves, off), leaf_h, node_h, new_h, root


def _ptr(a):
    return None if a is None else a.ctypes.data


def merkle_extend(old_size: int, old_hashes, leaves, offsets, want_leaf_hashes=True, want_node_hashes=True,
                  device: int = 0):
    """Extend the compact RFC 6962 Merkle tree (old_size, old_hashes) by the n
    leaves laid out as msgs / offsets everywhere else (edv_merkle_extend, row f-5).

    old_hashes: popcount(old_size) x 32 bytes (bytes or uint8 array), largest
    subtree first.  Returns (leaf_hashes, node_hashes, new_hashes, root):
    (n, 32), (nodes, 32) and (popcount(new), 32) uint8 arrays and 32 bytes;
    leaf_hashes / node_hashes are None when not wanted.  Bit-exact with n
    successive appends of the reference's CompactMerkleTree."""
    _, _, head, _keep, leaf_h, node_h, new_h, root = _merkle_call(old_size, old_hashes, leaves, offsets,
                                                                  want_leaf_hashes, want_node_hashes)
    _check(lib().edv_merkle_extend(*head, _ptr(leaf_h), _ptr(node_h), new_h.ctypes.data, root.ctypes.data, device))
    return leaf_h, node_h, new_h, root.tobytes()


def merkle_extend_device(old_size, d_old_hashes, d_leaves, d_off, n, d_leaf_hashes, d_node_hashes, d_new_hashes,
                         d_root, device=0, leaf_base=0, stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_extend_dev(old_size, d_old_hashes, d_leaves, d_off, leaf_base, n, d_leaf_hashes,
                                       d_node_hashes, d_new_hashes, d_root, device, stream))


def merkle_path_entries(old_size: int, n: int) -> int:
    """Audit-path entries of the first n appends to a tree of old_size leaves:
    the sum of popcount(old_size + i) over i < n (edv_merkle_path_entries; no
    device is touched).  Leaf i's path starts at entry merkle_path_entries(old_size, i)."""
    out = ctypes.c_uint64(0)
    _check(lib().edv_merkle_path_entries(old_size, n, ctypes.byref(out)))
    return int(out.value)


def merkle_append_batch(old_size: int, old_hashes, leaves, offsets, want_roots=True, want_audit_paths=True,
                        want_leaf_hashes=True, want_node_hashes=True, device: int = 0):
    """merkle_extend that also returns what each of the n appends returns
    (edv_merkle_append_batch, row f-6).

    Returns (leaf_hashes, node_hashes, new_hashes, root, roots, audit_paths):
    the first four as merkle_extend; roots is (n, 32), the root after leaf i;
    audit_paths is (merkle_path_entries(old_size, n), 32), the paths packed one
    after another, leaf i's being the popcount(old_size + i) rows from
    merkle_path_entries(old_size, i) on (smallest subtree first).  Outputs not
    wanted are None."""
    old_size, n, head, _keep, leaf_h, node_h, new_h, root = _merkle_call(old_size, old_hashes, leaves, offsets,
                                                                         want_leaf_hashes, want_node_hashes)
    roots = np.zeros((n, 32), dtype=np.uint8) if want_roots else None
    paths = np.zeros((merkle_path_entries(old_size, n), 32), dtype=np.uint8) if want_audit_paths else None
    _check(lib().edv_merkle_append_batch(*head, _ptr(leaf_h), _ptr(node_h), new_h.ctypes.data, root.ctypes.data,
                                         _ptr(roots), _ptr(paths), device))
    return leaf_h, node_h, new_h, root.tobytes(), roots, paths


def merkle_append_batch_device(old_size, d_old_hashes, d_leaves, d_off, n, d_leaf_hashes, d_node_hashes, d_new_hashes,
                               d_root, d_roots, d_audit_paths, device=0, leaf_base=0, stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_append_batch_dev(old_size, d_old_hashes, d_leaves, d_off, leaf_base, n, d_leaf_hashes,
                                             d_node_hashes, d_new_hashes, d_root, d_roots, d_audit_paths, device,
                                             stream))


# proof verification (row f-7): one status byte per proof, EDV_PROOF_* of include/edv.h
PROOF_UNVERIFIED = 0   # never written by a kernel: what the host form fills the buffer with first
PROOF_OK = 1
PROOF_RANGE = 2        # leaf_index >= tree_size / old_size > new_size
PROOF_SHORT = 3        # the walk needed an entry past the proof's end
PROOF_LONG = 4         # inclusion only: entries left over after the walk
PROOF_ROOT = 5         # the computed root (inclusion) / new root (consistency) differs
PROOF_INCONSISTENT = 6  # consistency only: the new root matches and the old one does not


def _u8(a, what, nbytes=None):
    if not isinstance(a, np.ndarray):
        a = np.frombuffer(bytes(a) or b"\0", dtype=np.uint8)
    if a.dtype != np.uint8 or not a.flags.c_contiguous:
        raise ValueError(what + " must be contiguous uint8")
    if nbytes is not None and a.nbytes < nbytes:
        raise ValueError(what + " is too small")
    return a


def _u64(a, what, count):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if a.ndim != 1 or len(a) != count:
        raise ValueError("%s must hold %d entries" % (what, count))
    return a


def _proof_offsets(proof_off, proofs):
    off = np.ascontiguousarray(proof_off, dtype=np.uint64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError("proof_off must hold n + 1 entries")
    n = len(off) - 1
    if n > MERKLE_MAX_LEAVES:
        raise ValueError("more than MERKLE_MAX_LEAVES proofs in one call")
    proofs = _u8(proofs, "proofs")
    if 32 * int(off[-1]) > proofs.nbytes and int(off[-1]) > 0:
        raise ValueError("proof_off exceeds the proof buffer")
    return off, n, proofs


def merkle_verify_inclusion(leaf_index, tree_size, roots, proofs, proof_off, leaves=None, leaf_off=None,
                            leaf_hashes=None, want_computed=False, device: int = 0):
    """n audit paths in one call (edv_merkle_verify_inclusion, row f-7).

    proofs: packed 32-byte entries (bytes or uint8 array); proof_off: n + 1
    offsets in entries; roots: n x 32 bytes; leaf_index / tree_size: n
    integers below 2^64.  The leaves come as `leaves` (bytes laid out by the
    n + 1 offsets `leaf_off`; the call stages them with the read-ahead the
    kernel needs) or as `leaf_hashes` (n x 32 bytes), never both.  Returns (status, computed): n
    PROOF_* bytes and the (n, 32) calculated roots (None unless wanted)."""
    off, n, proofs = _proof_offsets(proof_off, proofs)
    if (leaves is None) == (leaf_hashes is None):
        raise ValueError("give leaves or leaf_hashes, not both")
    idx, size = _u64(leaf_index, "leaf_index", n), _u64(tree_size, "tree_size", n)
    roots = _u8(roots, "roots", 32 * n)
    loff = None
    if leaves is not None:
        loff = _u64(leaf_off, "leaf_off", n + 1)
        leaves = _u8(leaves, "leaves")
        if int(loff[-1]) > leaves.nbytes:
            raise ValueError("leaf_off exceeds the leaf buffer")
    else:
        leaf_hashes = _u8(leaf_hashes, "leaf_hashes", 32 * n)
    status = np.zeros(n, dtype=np.uint8)
    computed = np.zeros((n, 32), dtype=np.uint8) if want_computed else None
    _check(lib().edv_merkle_verify_inclusion(_ptr(leaves), _ptr(loff), _ptr(leaf_hashes), idx.ctypes.data,
                                             size.ctypes.data, roots.ctypes.data, proofs.ctypes.data, off.ctypes.data,
                                             n, status.ctypes.data, _ptr(computed), device))
    return status, computed


def merkle_verify_inclusion_device(d_leaf_index, d_tree_size, d_roots, d_proofs, d_proof_off, n, d_status,
                                   d_computed=None, d_leaves=None, d_leaf_off=None, d_leaf_hashes=None, device=0,
                                   leaf_base=0, proof_base=0, stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_verify_inclusion_dev(d_leaves, d_leaf_off, leaf_base, d_leaf_hashes, d_leaf_index,
                                                 d_tree_size, d_roots, d_proofs, d_proof_off, proof_base, n, d_status,
                                                 d_computed, device, stream))


def merkle_verify_consistency(old_size, new_size, old_roots, new_roots, proofs, proof_off, want_computed=False,
                              device: int = 0):
    """n consistency proofs in one call (edv_merkle_verify_consistency).
    Returns (status, computed): n PROOF_* bytes and the (n, 64) calculated
    old and new roots (None unless wanted)."""
    off, n, proofs = _proof_offsets(proof_off, proofs)
    old_size, new_size = _u64(old_size, "old_size", n), _u64(new_size, "new_size", n)
    old_roots, new_roots = _u8(old_roots, "old_roots", 32 * n), _u8(new_roots, "new_roots", 32 * n)
    status = np.zeros(n, dtype=np.uint8)
    computed = np.zeros((n, 64), dtype=np.uint8) if want_computed else None
    _check(lib().edv_merkle_verify_consistency(old_size.ctypes.data, new_size.ctypes.data, old_roots.ctypes.data,
                                               new_roots.ctypes.data, proofs.ctypes.data, off.ctypes.data, n,
                                               status.ctypes.data, _ptr(computed), device))
    return status, computed


def merkle_verify_consistency_device(d_old_size, d_new_size, d_old_roots, d_new_roots, d_proofs, d_proof_off, n,
                                     d_status, d_computed=None, device=0, proof_base=0, stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_verify_consistency_dev(d_old_size, d_new_size, d_old_roots, d_new_roots, d_proofs,
                                                   d_proof_off, proof_base, n, d_status, d_computed, device, stream))


# proof generation (row f-8)
PROOF_SPACE = 7        # proof generation only: the slot's length is not the proof's; nothing else written


def _prove_pairs(a, b, what_a, what_b):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    b = np.ascontiguousarray(b, dtype=np.uint64)
    if a.ndim != 1 or b.ndim != 1 or len(a) != len(b):
        raise ValueError("%s and %s must hold one entry per proof" % (what_a, what_b))
    if len(a) > MERKLE_MAX_LEAVES:
        raise ValueError("more than MERKLE_MAX_LEAVES proofs in one call")
    return a, b, len(a)


def _prove_offsets(call, a, b, store_leaves):
    n = len(a)
    off = np.zeros(n + 1, dtype=np.uint64)
    _check(call(a.ctypes.data, b.ctypes.data, n, int(store_leaves), off.ctypes.data))
    return off


def merkle_inclusion_offsets(leaf_index, tree_size, store_leaves: int) -> np.ndarray:
    """The n + 1 packed slot offsets (in entries, from 0) of the audit paths of
    (leaf_index[i], tree_size[i]) over a store of store_leaves leaves; a pair
    that merkle_prove_inclusion answers with PROOF_RANGE takes no entries
    (edv_merkle_inclusion_offsets; no device is touched)."""
    a, b, _ = _prove_pairs(leaf_index, tree_size, "leaf_index", "tree_size")
    return _prove_offsets(lib().edv_merkle_inclusion_offsets, a, b, store_leaves)


def merkle_consistency_offsets(first, second, store_leaves: int) -> np.ndarray:
    """As merkle_inclusion_offsets, for PROOF(first[i], D[0:second[i]])."""
    a, b, _ = _prove_pairs(first, second, "first", "second")
    return _prove_offsets(lib().edv_merkle_consistency_offsets, a, b, store_leaves)


def _prove_host(call, offsets, leaf_store, node_store, store_leaves, a, b, proof_off, want1, want2, device):
    store_leaves = int(store_leaves)
    if not 0 <= store_leaves <= MERKLE_MAX_SIZE:
        raise ValueError("store_leaves must be in [0, 2^62]")
    leaf_store = _u8(leaf_store, "leaf_store", 32 * store_leaves)
    node_store = _u8(node_store, "node_store", 32 * (store_leaves - bin(store_leaves).count("1")))
    n = len(a)
    off = offsets(a, b, store_leaves) if proof_off is None else _u64(proof_off, "proof_off", n + 1)
    if n and np.any(off[1:] < off[:-1]):
        raise ValueError("proof_off must not decrease")
    proofs = np.zeros((int(off[-1]), 32), dtype=np.uint8)
    status = np.zeros(n, dtype=np.uint8)
    out1 = np.zeros((n, 32), dtype=np.uint8) if want1 else None
    out2 = np.zeros((n, 32), dtype=np.uint8) if want2 else None
    _check(call(leaf_store.ctypes.data, node_store.ctypes.data, store_leaves, a.ctypes.data, b.ctypes.data,
                off.ctypes.data, n, proofs.ctypes.data, status.ctypes.data, _ptr(out1), _ptr(out2), device))
    return proofs, off, status, out1, out2


def merkle_prove_inclusion(leaf_store, node_store, store_leaves, leaf_index, tree_size, proof_off=None,
                           want_roots=True, want_leaf_hashes=False, device: int = 0):
    """n audit paths out of a hash store in host memory (edv_merkle_prove_inclusion,
    row f-8).  The call copies the store prefix it reads to the device every
    time: for small stores and callers without device memory.

    leaf_store / node_store: the store's hashes (bytes or uint8 arrays,
    store_leaves x 32 and (store_leaves - popcount(store_leaves)) x 32 bytes at
    least); leaf_index / tree_size: n integers below 2^64; proof_off: n + 1
    slot offsets in entries (default: merkle_inclusion_offsets, the exact fit).
    Returns (proofs, proof_off, status, roots, leaf_hashes): the packed
    (entries, 32) proofs in the verifier's layout, n PROOF_* bytes (OK, RANGE
    or SPACE), and the (n, 32) tree heads and stored leaf hashes (None unless
    wanted; zeros where the status is not OK)."""
    a, b, _ = _prove_pairs(leaf_index, tree_size, "leaf_index", "tree_size")
    return _prove_host(lib().edv_merkle_prove_inclusion, merkle_inclusion_offsets, leaf_store, node_store,
                       store_leaves, a, b, proof_off, want_roots, want_leaf_hashes, device)


def merkle_prove_consistency(leaf_store, node_store, store_leaves, first, second, proof_off=None, want_roots=True,
                             device: int = 0):
    """n consistency proofs PROOF(first, D[0:second]) out of a hash store in
    host memory (edv_merkle_prove_consistency).  Returns (proofs, proof_off,
    status, old_roots, new_roots), as merkle_prove_inclusion."""
    a, b, _ = _prove_pairs(first, second, "first", "second")
    return _prove_host(lib().edv_merkle_prove_consistency, merkle_consistency_offsets, leaf_store, node_store,
                       store_leaves, a, b, proof_off, want_roots, want_roots, device)


def merkle_prove_inclusion_device(d_leaf_store, d_node_store, store_leaves, d_leaf_index, d_tree_size, d_proof_off, n,
                                  d_proofs, d_status, d_roots=None, d_leaf_hashes_out=None, device=0, proof_base=0,
                                  stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_prove_inclusion_dev(d_leaf_store, d_node_store, store_leaves, d_leaf_index, d_tree_size,
                                                d_proof_off, proof_base, n, d_proofs, d_status, d_roots,
                                                d_leaf_hashes_out, device, stream))


def merkle_prove_consistency_device(d_leaf_store, d_node_store, store_leaves, d_first, d_second, d_proof_off, n,
                                    d_proofs, d_status, d_old_roots=None, d_new_roots=None, device=0, proof_base=0,
                                    stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_prove_consistency_dev(d_leaf_store, d_node_store, store_leaves, d_first, d_second,
                                                  d_proof_off, proof_base, n, d_proofs, d_status, d_old_roots,
                                                  d_new_roots, device, stream))


# auditing a stored tree (row f-9): one status byte per stored entry, EDV_AUDIT_* of include/edv.h
AUDIT_UNCHECKED = 0    # never written by a kernel: what the host forms fill the buffer with first
AUDIT_OK = 1
AUDIT_BAD = 2
AUDIT_NONE = (1 << 64) - 1   # a summary's lowest bad position when nothing is bad


def _store_arrays(leaf_store, node_store, store_leaves):
    store_leaves = int(store_leaves)
    if not 0 <= store_leaves <= MERKLE_MAX_SIZE:
        raise ValueError("store_leaves must be in [0, 2^62]")
    leaf_store = _u8(leaf_store, "leaf_store", 32 * store_leaves)
    if node_store is not None:
        node_store = _u8(node_store, "node_store", 32 * (store_leaves - bin(store_leaves).count("1")))
    return leaf_store, node_store, store_leaves


def merkle_audit_nodes(leaf_store, node_store, store_leaves, node_lo=0, count=None, want_status=True, device: int = 0):
    """Check nodes [node_lo, node_lo + count) of a hash store in host memory
    (0-based positions; default: every node from node_lo on) against their
    stored children (edv_merkle_audit_nodes, row f-9).  The call copies the
    store prefix the slice reads to the device every time.

    leaf_store / node_store as for merkle_prove_inclusion.  Returns (bad,
    first_bad, status): the number of bad nodes, the lowest bad position (None
    if there is none) and the AUDIT_* bytes of the slice (None unless wanted)."""
    leaf_store, node_store, store_leaves = _store_arrays(leaf_store, node_store, store_leaves)
    nodes = store_leaves - bin(store_leaves).count("1")
    node_lo = int(node_lo)
    count = nodes - node_lo if count is None else int(count)
    if node_lo < 0 or count < 0 or node_lo + count > nodes:
        raise ValueError("the slice reaches past the node store")
    if count > MERKLE_MAX_LEAVES:
        raise ValueError("more than MERKLE_MAX_LEAVES entries in one call")
    status = np.zeros(count, dtype=np.uint8) if want_status else None
    summary = np.zeros(2, dtype=np.uint64)
    _check(lib().edv_merkle_audit_nodes(leaf_store.ctypes.data, node_store.ctypes.data, store_leaves, node_lo, count,
                                        _ptr(status), summary.ctypes.data, device))
    return int(summary[0]), (None if int(summary[1]) == AUDIT_NONE else int(summary[1])), status


def merkle_audit_leaves(leaf_store, store_leaves, leaf_lo, leaves, offsets, want_status=True, device: int = 0):
    """Check leaf-store entries leaf_lo .. leaf_lo + n - 1 (0-based) against the
    n leaves laid out as msgs / offsets everywhere else (edv_merkle_audit_leaves).
    Returns (bad, first_bad, status) as merkle_audit_nodes, positions in the
    leaf store."""
    leaf_store, _, store_leaves = _store_arrays(leaf_store, None, store_leaves)
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    if off.ndim != 1 or len(off) < 1:
        raise ValueError("offsets must hold n + 1 entries")
    n, leaf_lo = len(off) - 1, int(leaf_lo)
    if leaf_lo < 0 or leaf_lo + n > store_leaves:
        raise ValueError("the slice reaches past the leaf store")
    if n > MERKLE_MAX_LEAVES:
        raise ValueError("more than MERKLE_MAX_LEAVES entries in one call")
    leaves = _u8(leaves, "leaves", int(off[-1]))
    status = np.zeros(n, dtype=np.uint8) if want_status else None
    summary = np.zeros(2, dtype=np.uint64)
    _check(lib().edv_merkle_audit_leaves(leaf_store.ctypes.data, store_leaves, leaf_lo, leaves.ctypes.data,
                                         off.ctypes.data, n, _ptr(status), summary.ctypes.data, device))
    return int(summary[0]), (None if int(summary[1]) == AUDIT_NONE else int(summary[1])), status


def merkle_audit_nodes_device(d_leaf_store, d_node_store, store_leaves, node_lo, count, d_status, d_summary, device=0,
                              stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream`
    if given.  Adds into d_summary, two uint64 the caller set to (0, AUDIT_NONE)."""
    _check(lib().edv_merkle_audit_nodes_dev(d_leaf_store, d_node_store, store_leaves, node_lo, count, d_status,
                                            d_summary, device, stream))


def merkle_audit_leaves_device(d_leaf_store, store_leaves, leaf_lo, d_leaves, d_leaf_off, n, d_status, d_summary,
                               device=0, leaf_base=0, stream=None):
    """Device-resident form, as merkle_audit_nodes_device."""
    _check(lib().edv_merkle_audit_leaves_dev(d_leaf_store, store_leaves, leaf_lo, d_leaves, d_leaf_off, leaf_base, n,
                                             d_status, d_summary, device, stream))


def merkle_extend_hashed(old_size: int, old_hashes, leaf_hashes, want_node_hashes=True, device: int = 0):
    """merkle_extend from the leaves' hashes instead of their bytes
    (edv_merkle_extend_hashed, row f-9): leaf_hashes is n x 32 bytes (bytes or a
    uint8 array).  Returns (node_hashes, new_hashes, root), byte-identical to
    merkle_extend's on the leaves those hashes belong to."""
    leaf_hashes = _u8(leaf_hashes, "leaf_hashes") if len(leaf_hashes) else np.zeros(0, dtype=np.uint8)
    if leaf_hashes.nbytes % 32:
        raise ValueError("leaf_hashes is not a whole number of hashes")
    n, old_size = leaf_hashes.nbytes // 32, int(old_size)
    if old_size < 0 or old_size + n > MERKLE_MAX_SIZE:
        raise ValueError("tree size out of range")
    if n > MERKLE_MAX_LEAVES:
        raise ValueError("more than MERKLE_MAX_LEAVES leaves in one call")
    if not isinstance(old_hashes, np.ndarray):
        old_hashes = np.frombuffer(bytes(old_hashes), dtype=np.uint8)
    if old_hashes.dtype != np.uint8 or not old_hashes.flags.c_contiguous:
        raise ValueError("old_hashes must be contiguous uint8")
    if old_hashes.nbytes != 32 * bin(old_size).count("1"):
        raise ValueError("old_hashes size does not match old_size")
    node_h = np.zeros((merkle_node_span(old_size, n), 32), dtype=np.uint8) if want_node_hashes else None
    new_h = np.zeros((bin(old_size + n).count("1"), 32), dtype=np.uint8)
    root = np.zeros(32, dtype=np.uint8)
    _check(lib().edv_merkle_extend_hashed(old_size, old_hashes.ctypes.data if old_hashes.nbytes else None,
                                          leaf_hashes.ctypes.data if n else None, n, _ptr(node_h), new_h.ctypes.data,
                                          root.ctypes.data, device))
    return node_h, new_h, root.tobytes()


def merkle_extend_hashed_device(old_size, d_old_hashes, d_leaf_hashes, n, d_node_hashes, d_new_hashes, d_root, device=0,
                                stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_extend_hashed_dev(old_size, d_old_hashes, d_leaf_hashes, n, d_node_hashes, d_new_hashes,
                                              d_root, device, stream))


# catch-up (row f-10)
def merkle_catchup(old_size: int, old_hashes, leaves, offsets, reply_end, final_size: int, final_root, proofs,
                   proof_off, want_leaf_hashes=True, want_node_hashes=True, want_roots=True, device: int = 0):
    """Verify and hash the replies of a catch-up in one call (edv_merkle_catchup,
    row f-10).  The n leaves (leaves / offsets as for merkle_extend) are the
    transactions of len(reply_end) in-order replies: reply k ends at leaf
    reply_end[k] of the call and carries the consistency proof k (proofs /
    proof_off as for merkle_verify_consistency) from the tree at its end to
    (final_size, final_root).  Returns (leaf_hashes, node_hashes, reply_roots,
    status): the first two as merkle_extend's, reply_roots the (replies, 32)
    tree heads at the replies' ends, status one PROOF_* per reply; outputs not
    wanted are None.  A status after the first failure is computed over
    rejected transactions."""
    final_size = int(final_size)
    if not 0 <= final_size < 1 << 64:
        raise ValueError("final_size out of range")
    old_size, n, head, _keep, leaf_h, node_h, _, _ = _merkle_call(old_size, old_hashes, leaves, offsets,
                                                                  want_leaf_hashes, want_node_hashes)
    poff, replies, proofs = _proof_offsets(proof_off, proofs)
    ends = _u64(reply_end, "reply_end", replies)
    final_root = _u8(final_root, "final_root", 32)
    roots = np.zeros((replies, 32), dtype=np.uint8) if want_roots else None
    status = np.zeros(replies, dtype=np.uint8)
    _check(lib().edv_merkle_catchup(*head, ends.ctypes.data, replies, final_size, final_root.ctypes.data,
                                    proofs.ctypes.data, poff.ctypes.data, _ptr(leaf_h), _ptr(node_h), _ptr(roots),
                                    status.ctypes.data, device))
    return leaf_h, node_h, roots, status


def merkle_catchup_device(old_size, d_old_hashes, d_leaves, d_off, n, d_reply_end, replies, final_size, d_final_root,
                          d_proofs, d_proof_off, d_leaf_hashes, d_node_hashes, d_reply_roots, d_status, device=0,
                          leaf_base=0, proof_base=0, stream=None):
    """Device-resident form (pointers are ints, None = NULL); async on `stream` if given."""
    _check(lib().edv_merkle_catchup_dev(old_size, d_old_hashes, d_leaves, d_off, leaf_base, n, d_reply_end, replies,
                                        final_size, d_final_root, d_proofs, d_proof_off, proof_base, d_leaf_hashes,
                                        d_node_hashes, d_reply_roots, d_status, device, stream))


def verify_detached_batch(items, device_mask: int = 0):
    """items: iterable of (sig64: bytes, msg: bytes, pk32: bytes) -> list[bool]."""
    items = list(items)
    if not items:
        return []
    for s, _m, p in items:
        if len(s) != 64 or len(p) != 32:
            raise ValueError("verify_detached_batch needs 64-byte sigs and 32-byte keys")
    off = np.zeros(len(items) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for _s, m, _p in items])
    acc = verify_arrays(b"".join(s for s, _m, _p in items), b"".join(p for _s, _m, p in items),
                        b"".join(m for _s, m, _p in items), off, device_mask)
    return [bool(a) for a in acc]


def open_batch(items, device_mask: int = 0):
    """crypto_sign_open semantics on (signature, msg, pk) triples, batched.

    Mirrors nacl_wrappers.Verifier.verify (nacl_wrappers.py:232-242): the signed
    message is signature + msg and libsodium splits it positionally, so a
    signature of any length is accepted iff (sm[:64], sm[64:]) verifies; sm
    shorter than 64 bytes rejects without reaching the GPU.  pk must be 32 bytes.
    """
    items = list(items)
    if not items:
        return []
    addr = verify_address()
    try:
        out = _edvhost.open_verify(items, addr, device_mask)
    except TypeError:  # bytearray / memoryview / list items: normalise, then pack
        items = [(bytes(s), bytes(m), bytes(p)) for s, m, p in items]
        out = _edvhost.open_verify(items, addr, device_mask)
    if isinstance(out, int):  # the C-ABI's error code
        _check(out)
    return out


_OPEN_BATCH = open_batch        # the genuine entry point (tests may monkeypatch open_batch)
_verify_addr = None
_sha_addr = None
BATCH_DEVICE_MASK = 0          # devices used by the native whole-batch authenticator path
PREP_THREADS = int(os.environ.get("EDV_PREP_THREADS", "0")) or max(1, min(8, (os.cpu_count() or 2) // 2))


def verify_address() -> int:
    """Address of edv_verify_batch (the native whole-batch authenticator calls it
    with the GIL released); also hands edv_host_alloc/free to _edvhost so its
    batch arenas are page-locked."""
    global _verify_addr
    if _verify_addr is None:
        h = lib()
        _edvhost.set_host_allocator(ctypes.cast(h.edv_host_alloc, ctypes.c_void_p).value,
                                    ctypes.cast(h.edv_host_free, ctypes.c_void_p).value)
        _verify_addr = ctypes.cast(h.edv_verify_batch, ctypes.c_void_p).value
    return _verify_addr


_async_addrs = None


def async_addresses():
    """(edv_verify_digest_batch_async, edv_wait_async) addresses for the native
    asynchronous whole-batch path (_edvhost.auth_core_submit / _finish)."""
    global _async_addrs
    if _async_addrs is None:
        verify_address()  # page-locked arenas
        h = lib()
        _async_addrs = (ctypes.cast(h.edv_verify_digest_batch_async, ctypes.c_void_p).value,
                        ctypes.cast(h.edv_wait_async, ctypes.c_void_p).value)
    return _async_addrs


_query_addr = None


def query_address() -> int:
    """Address of edv_query_async (the native batch handles' ready() calls it)."""
    global _query_addr
    if _query_addr is None:
        _query_addr = ctypes.cast(lib().edv_query_async, ctypes.c_void_p).value
    return _query_addr


BATCH_DEVICE = None            # device of the native asynchronous whole-batch path (None: batch_device())


def sha256_address() -> int:
    """Address of edv_sha256_batch (the native request-digest batch calls it with
    the GIL released)."""
    global _sha_addr
    if _sha_addr is None:
        _sha_addr = ctypes.cast(lib().edv_sha256_batch, ctypes.c_void_p).value
    return _sha_addr


def native_batch_enabled() -> bool:
    """The native whole-batch path calls edv_verify_batch itself, so it is used
    only while open_batch is the genuine entry point."""
    return open_batch is _OPEN_BATCH and os.environ.get("EDV_NATIVE_BATCH", "1") != "0"


class DeviceBuffer:
    """A raw device allocation through the C-ABI (no PyTorch needed)."""

    def __init__(self, nbytes: int, device: int = 0):
        self.device = device
        self.nbytes = nbytes
        p = ctypes.c_void_p()
        _check(lib().edv_dev_alloc(device, nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, host):
        a = np.ascontiguousarray(host)
        assert a.nbytes <= self.nbytes
        _check(lib().edv_h2d(self.device, self.ptr, a.ctypes.data, a.nbytes))

    def download(self, nbytes=None, dtype=np.uint8):
        nbytes = self.nbytes if nbytes is None else nbytes
        out = np.empty(nbytes, dtype=np.uint8)
        _check(lib().edv_d2h(self.device, out.ctypes.data, self.ptr, nbytes))
        return out.view(dtype)

    def download_at(self, offset, nbytes, dtype=np.uint8):
        """Bytes [offset, offset + nbytes) of the buffer."""
        assert 0 <= offset and offset + nbytes <= self.nbytes
        out = np.empty(nbytes, dtype=np.uint8)
        if nbytes:
            _check(lib().edv_d2h(self.device, out.ctypes.data, self.ptr + offset, nbytes))
        return out.view(dtype)

    def free(self):
        if self.ptr:
            lib().edv_dev_free(self.device, self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def verify_device(d_sigs, d_pks, d_msgs, d_off, n, d_accept, device=0, msg_base=0, stream=None, flags=0):
    """Device-resident verify (pointers are ints); async on `stream` if given.
    flags: FLAG_UNIFORM_LENGTH / FLAG_BUCKETS (per-call length-bucket hint)."""
    _check(lib().edv_verify_batch_dev_flags(d_sigs, d_pks, d_msgs, d_off, msg_base, n, d_accept, device, stream,
                                            flags))


def verify_device_pipelined(d_sigs, d_pks, d_msgs, d_off, n, d_accept, device=0, msg_base=0, flags=0):
    """Enqueue a device-resident batch on the library's two-stream pipeline (the
    prep kernel of the next batch overlaps the main kernel of this one); the
    verdicts are in d_accept after pipeline_sync(device)."""
    _check(lib().edv_verify_batch_dev_pipelined(d_sigs, d_pks, d_msgs, d_off, msg_base, n, d_accept, device,
                                                flags))


def shard_split(offsets, g: int) -> np.ndarray:
    """The C-ABI's shard split (edv_shard_split; host only, no GPU): g+1 bounds,
    shard k = requests [b[k], b[k+1]).  Equal counts for one SHA-512 block count,
    else equal estimated cost sum(40 + blocks)."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(off) - 1
    b = np.zeros(g + 1, dtype=np.uint64)
    _check(lib().edv_shard_split(off.ctypes.data if n > 0 else None, max(n, 0), g, b.ctypes.data))
    return b


class PinnedBuffer:
    """Page-locked host memory (edv_host_alloc): batches packed here reach the
    device by DMA without the library's staging copy.  `.array` is a uint8 view."""

    def __init__(self, nbytes: int):
        p = ctypes.c_void_p()
        _check(lib().edv_host_alloc(nbytes, ctypes.byref(p)))
        self.ptr, self.nbytes = p.value, nbytes
        self.array = np.ctypeslib.as_array((ctypes.c_uint8 * max(nbytes, 1)).from_address(p.value))[:nbytes]

    def view(self, dtype, offset: int = 0, count: int = -1):
        return np.frombuffer(self.array, dtype=dtype, count=count, offset=offset)

    def free(self):
        if self.ptr:
            self.array = None
            lib().edv_host_free(self.ptr)
            self.ptr = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def pipeline_sync(device: int = 0):
    """Wait for every pipelined batch submitted on `device`."""
    _check(lib().edv_pipeline_sync(device))


def sign_device(d_seeds, d_msgs, d_off, n, d_pks, d_sigs, device=0, msg_base=0, stream=None):
    """Device-resident batch signing (row f-4): seeds -> pks, detached sigs."""
    _check(lib().edv_sign_batch_dev(d_seeds, d_msgs, d_off, msg_base, n, d_pks, d_sigs, device, stream))


def sign_arrays(seeds, msgs, offsets, device=0):
    """Host-array convenience over sign_device -> (pks n*32, sigs n*64) uint8 arrays."""
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(off) - 1
    seeds = np.ascontiguousarray(np.frombuffer(bytes(seeds), np.uint8) if not isinstance(seeds, np.ndarray) else seeds)
    msgs = np.frombuffer(bytes(msgs) + b"\0" * 16, np.uint8) if not isinstance(msgs, np.ndarray) else msgs
    if n <= 0:
        return np.zeros(0, np.uint8), np.zeros(0, np.uint8)
    bufs = [DeviceBuffer(max(a.nbytes, 1) + 64, device) for a in (seeds, msgs, off)]
    for b, a in zip(bufs, (seeds, msgs, off)):
        b.upload(a)
    dp, ds = DeviceBuffer(32 * n, device), DeviceBuffer(64 * n, device)
    sign_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, n, dp.ptr, ds.ptr, device)
    return dp.download(32 * n), ds.download(64 * n)


# ---- measurement helpers: libedv_measure.so (include/edv_measure.h)
def time_device(d_sigs, d_pks, d_msgs, d_off, n, d_accept, device=0, iters=1, msg_base=0) -> float:
    """Milliseconds for `iters` back-to-back kernel launches (HIP events on the kernel's stream)."""
    ms = ctypes.c_float(0)
    _mcheck(measure_lib().edv_time_batch_dev(d_sigs, d_pks, d_msgs, d_off, msg_base, n, d_accept, device, iters,
                                             ctypes.byref(ms)))
    return float(ms.value)


def profile_device(d_sigs, d_pks, d_msgs, d_off, n, d_accept, device=0, iters=1, msg_base=0):
    """(prep_ms, main_ms): average per-launch kernel times from HIP events on the kernels' stream."""
    a, b = ctypes.c_float(0), ctypes.c_float(0)
    _mcheck(measure_lib().edv_profile_batch_dev(d_sigs, d_pks, d_msgs, d_off, msg_base, n, d_accept, device, iters,
                                                ctypes.byref(a), ctypes.byref(b)))
    return float(a.value), float(b.value)


def profile_device_flush(d_sigs, d_pks, d_msgs, d_off, n, d_accept, device=0, iters=1, flush_bytes=0, msg_base=0):
    """(prep_ms, flush_ms, main_ms) with a cache-evicting kernel of flush_bytes between
    prep and main (edv_profile_batch_dev_flush)."""
    a, f, b = ctypes.c_float(0), ctypes.c_float(0), ctypes.c_float(0)
    _mcheck(measure_lib().edv_profile_batch_dev_flush(d_sigs, d_pks, d_msgs, d_off, msg_base, n, d_accept, device,
                                                      iters, flush_bytes, ctypes.byref(a), ctypes.byref(f),
                                                      ctypes.byref(b)))
    return float(a.value), float(f.value), float(b.value)


PREP_SIDE_KEYS = ("hash_side", "a_side", "r_side", "all_three", "point_sides")


def profile_prep_sides(d_sigs, d_pks, d_msgs, d_off, n, d_accept, device=0, iters=1, msg_base=0) -> dict:
    """The prep kernel's sides timed apart (edv_profile_prep_sides), ms per launch."""
    ms = (ctypes.c_float * 5)()
    _mcheck(measure_lib().edv_profile_prep_sides(d_sigs, d_pks, d_msgs, d_off, msg_base, n, d_accept, device, iters,
                                                 ms))
    return dict(zip(PREP_SIDE_KEYS, (float(x) for x in ms)))


# op codes and (input, output) bytes per case of edv_probe_math (include/edv_measure.h)
PROBE_OPS = {
    "fe_mul": (1, 80, 40), "fe_sq": (2, 40, 40), "fe_sq2": (3, 40, 40), "fe_sq_floor": (4, 40, 40),
    "fe_tobytes": (5, 40, 32), "fe_frombytes": (6, 32, 40), "fe_invert_safegcd": (7, 40, 40),
    "fe_pow22523": (8, 40, 40), "sc_reduce": (9, 64, 32), "half_scalars": (10, 32, 68), "recode5": (11, 32, 36),
    "approx_div": (12, 16, 8), "fdiv_floor": (13, 16, 8), "euclid_div": (14, 128, 64),
    "ge_frombytes": (15, 32, 172), "quad_sq_shift": (16, 176, 160), "quad_dbl": (17, 160, 160),
    "quad_add": (18, 320, 160), "quad_cached": (19, 160, 160), "quad_cached_signed": (20, 164, 160),
    "sc_muladd": (21, 96, 32), "recode8": (22, 32, 32), "scalarmult_base": (23, 32, 192),
    "ge_p3_tobytes": (24, 160, 32),
}


def probe_math(op, cases, device=0):
    """Runs the device build of one header function on packed cases
    (edv_probe_math): `cases` is a C-contiguous uint8 array (n, input bytes of
    `op`); returns a uint8 array (n, output bytes)."""
    code, nin, nout = PROBE_OPS[op]
    cases = np.ascontiguousarray(cases, dtype=np.uint8)
    if cases.ndim != 2 or cases.shape[1] != nin:
        raise ValueError("probe {}: cases must be (n, {}) bytes".format(op, nin))
    out = np.zeros((cases.shape[0], nout), np.uint8)
    _mcheck(measure_lib().edv_probe_math(device, code, cases.ctypes.data, nin, out.ctypes.data, nout,
                                         cases.shape[0]))
    return out


# ---- the stage probes (include/edv_measure.h): the product's prep and main
# kernels on a state the caller reads back or writes, and the device tables
STAGE_CAP = 4096
STAGE_SENTINEL = 0xA5
STAGE_BUCKETS, STAGE_SPLIT, STAGE_PRIO = 1, 2, 4
TABLE_SETS = {"compact": 0, "large": 1, "comb": 2}
A_WORDS = 360   # a slot's table: 9 entries x (Y+X, Y-X, Z, 2dT) x 10 limbs
DIG_WORDS = 17


def probe_prep_state(sigs, pks, msgs, offsets, table_set="compact", buckets=False, split=False, side0=0, nsides=3,
                     device=0) -> dict:
    """Runs the bucket kernels (if asked) and the prep kernel on a batch of at
    most STAGE_CAP requests (edv_probe_prep_state) and returns the state they
    wrote: dig (17, cap) uint32, alive (3, cap) uint8, atab / rtab (n, 360)
    int32, perm (n) uint32 or None, accept (n) uint8; bytes no kernel wrote
    hold STAGE_SENTINEL."""
    sigs, pks, msgs = (np.ascontiguousarray(np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray))
                                            else x, dtype=np.uint8) for x in (sigs, pks, msgs))
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(off) - 1
    if sigs.size != 64 * n or pks.size != 32 * n or (n and msgs.size < int(off[-1])):
        raise ValueError("prep probe: sigs n x 64, pks n x 32, msgs at least offsets[n] bytes")
    cap = ctypes.c_uint64(0)
    st = {"dig": np.full((DIG_WORDS, STAGE_CAP), STAGE_SENTINEL * 0x01010101, np.uint32),
          "alive": np.full((3, STAGE_CAP), STAGE_SENTINEL, np.uint8),
          "atab": np.full((n, A_WORDS), STAGE_SENTINEL * 0x01010101, np.uint32).view(np.int32),
          "rtab": np.full((n, A_WORDS), STAGE_SENTINEL * 0x01010101, np.uint32).view(np.int32),
          "perm": np.zeros(n, np.uint32) if buckets else None,
          "accept": np.full(n, STAGE_SENTINEL, np.uint8)}
    flags = (STAGE_BUCKETS if buckets else 0) | (STAGE_SPLIT if split else 0)
    _mcheck(measure_lib().edv_probe_prep_state(
        device, sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, off.ctypes.data, n, TABLE_SETS[table_set], side0,
        nsides, flags, st["dig"].ctypes.data, st["alive"].ctypes.data, st["atab"].ctypes.data, st["rtab"].ctypes.data,
        st["perm"].ctypes.data if buckets else None, st["accept"].ctypes.data, ctypes.byref(cap)))
    assert cap.value == STAGE_CAP
    st["cap"] = STAGE_CAP
    return st


def probe_main_state(n, dig, alive, atab, rtab, perm=None, prio=False, device=0) -> np.ndarray:
    """One launch of the main kernel (prio: edv_main_kernel_prio) on the given
    state of n slots (edv_probe_main_state; dig (17, cap), alive (3, cap), atab
    / rtab (n, 360)); returns accept (n) uint8, STAGE_SENTINEL where the kernel
    wrote nothing."""
    dig = np.ascontiguousarray(dig, dtype=np.uint32)
    alive = np.ascontiguousarray(alive, dtype=np.uint8)
    atab = np.ascontiguousarray(atab, dtype=np.int32)
    rtab = np.ascontiguousarray(rtab, dtype=np.int32)
    cap = dig.shape[1]
    if dig.shape != (DIG_WORDS, cap) or alive.shape != (3, cap) or atab.size < n * A_WORDS or rtab.size < n * A_WORDS:
        raise ValueError("main probe: dig (17, cap), alive (3, cap), atab / rtab n x 360 words")
    if perm is not None:
        perm = np.ascontiguousarray(perm, dtype=np.uint32)
        if perm.size < n:
            raise ValueError("main probe: perm has n entries")
    accept = np.full(n, STAGE_SENTINEL, np.uint8)
    _mcheck(measure_lib().edv_probe_main_state(device, n, cap, dig.ctypes.data, alive.ctypes.data, atab.ctypes.data,
                                               rtab.ctypes.data, None if perm is None else perm.ctypes.data,
                                               STAGE_PRIO if prio else 0, accept.ctypes.data))
    return accept


def probe_table(table_set, pairs, device=0) -> np.ndarray:
    """Entries (t, j) of a device table (edv_probe_table: "compact", "large" or
    "comb"), (n, 32) int32: y+x, y-x, 2dxy limbs and two words of padding."""
    tj = np.ascontiguousarray(pairs, dtype=np.int32).reshape(-1, 2)
    out = np.zeros((len(tj), 32), np.int32)
    _mcheck(measure_lib().edv_probe_table(device, TABLE_SETS[table_set], tj.ctypes.data, len(tj), out.ctypes.data))
    return out


# ---- the latency probes (include/edv_measure.h): the latency kernels cut at
# phase 1's barrier.  Probe kernels that instantiate the header functions the
# product's kernels are made of, not the product's kernel objects.
LAT_KERNELS = {"rtl": (0, 16), "quad": (1, 32)}   # name -> (code, slots per workgroup)
PT_WORDS = 40    # a point: X | Y | Z | T, 10 limbs each


def latency_slots(kernel, n) -> int:
    """n rounded up to the workgroup's 16 or 32 slots"""
    ns = LAT_KERNELS[kernel][1]
    return (n + ns - 1) // ns * ns


def probe_latency_phase1(kernel, sigs, pks, msgs, offsets, table_set="compact", device=0) -> dict:
    """Phase 1 of a latency kernel ("rtl" or "quad") over at most STAGE_CAP
    requests (edv_probe_latency_phase1); returns what each workgroup held in
    LDS at the barrier, by slot: dig (17, slots) uint32, pt (3, 40, slots)
    int32, ok (3, slots) uint8, and accept (n) uint8; bytes no kernel wrote
    hold STAGE_SENTINEL."""
    code, ns = LAT_KERNELS[kernel]
    sigs, pks, msgs = (np.ascontiguousarray(np.frombuffer(bytes(x), np.uint8) if isinstance(x, (bytes, bytearray))
                                            else x, dtype=np.uint8) for x in (sigs, pks, msgs))
    off = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = len(off) - 1
    if sigs.size != 64 * n or pks.size != 32 * n or (n and msgs.size < int(off[-1])):
        raise ValueError("latency phase-1 probe: sigs n x 64, pks n x 32, msgs at least offsets[n] bytes")
    slots = latency_slots(kernel, n)
    g = slots // ns
    dig = np.full((g, DIG_WORDS, ns), STAGE_SENTINEL * 0x01010101, np.uint32)
    pt = np.full((g, 3, PT_WORDS, ns), STAGE_SENTINEL * 0x01010101, np.uint32).view(np.int32)
    ok = np.full((g, 3, ns), STAGE_SENTINEL, np.uint8)
    accept = np.full(n, STAGE_SENTINEL, np.uint8)
    _mcheck(measure_lib().edv_probe_latency_phase1(
        device, code, TABLE_SETS[table_set], sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, off.ctypes.data, n,
        dig.ctypes.data, pt.ctypes.data, ok.ctypes.data, accept.ctypes.data))
    # [workgroup][word][slot] -> [word][slot of the batch]
    return {"dig": np.ascontiguousarray(dig.transpose(1, 0, 2).reshape(DIG_WORDS, slots)),
            "pt": np.ascontiguousarray(pt.transpose(1, 2, 0, 3).reshape(3, PT_WORDS, slots)),
            "ok": np.ascontiguousarray(ok.transpose(1, 0, 2).reshape(3, slots)), "accept": accept, "slots": slots}


def probe_latency_walk(kernel, n, dig, pt, ok, device=0) -> np.ndarray:
    """Everything after phase 1's barrier of a latency kernel ("rtl" or "quad")
    on the given phase-1 state (edv_probe_latency_walk): dig (17, slots), pt
    (3, 40, slots), ok (3, slots) with slots = latency_slots(kernel, n);
    returns accept (slots) uint8, STAGE_SENTINEL where the kernel wrote nothing
    (every slot from n on)."""
    code, ns = LAT_KERNELS[kernel]
    slots = latency_slots(kernel, n)
    dig = np.asarray(dig, dtype=np.uint32)
    pt = np.asarray(pt, dtype=np.int32)
    ok = np.asarray(ok, dtype=np.uint8)
    if dig.shape != (DIG_WORDS, slots) or pt.shape != (3, PT_WORDS, slots) or ok.shape != (3, slots):
        raise ValueError("latency walk probe: dig (17, slots), pt (3, 40, slots), ok (3, slots)")
    g = slots // ns
    # [word][slot of the batch] -> [workgroup][word][slot]
    dig = np.ascontiguousarray(dig.reshape(DIG_WORDS, g, ns).transpose(1, 0, 2))
    pt = np.ascontiguousarray(pt.reshape(3, PT_WORDS, g, ns).transpose(2, 0, 1, 3))
    ok = np.ascontiguousarray(ok.reshape(3, g, ns).transpose(1, 0, 2))
    accept = np.full(slots, STAGE_SENTINEL, np.uint8)
    _mcheck(measure_lib().edv_probe_latency_walk(device, code, n, slots, dig.ctypes.data, pt.ctypes.data,
                                                 ok.ctypes.data, 0, accept.ctypes.data))
    return accept
