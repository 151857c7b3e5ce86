"""The host paths' arithmetic (csrc/edv_hostplan.h) through the CPU build
libedv_hostcheck.so: the packed layout of a batch, the single-copy test, the
capacity rules, the field path's slices, the sub-batch split and the trim
limits, each against a plain Python restatement of its rule written here, and
the same sweeps under UBSan + ASan as a stand-alone program
(tools/ubsan_hostplan.cpp)."""
import ctypes
import os
import shutil
import subprocess

import pytest

import hostcheck_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NS = [0, 1, 255, 256, 257, 511, 512, 513, 4096, 4097, 65535, 65536, 65537, 262144, 2**32 + 1]
CHUNKS = [256, 512, 768, 2**18]
BLOCK, SLICES, MIN_SLICE = 256, 8, 65536
U64 = ctypes.c_uint64


@pytest.fixture(scope="module")
def hc():
    subprocess.check_call(["make", "-s", "-C", hostcheck_lib.CSRC, "../libedv_hostcheck.so"])
    lib = hostcheck_lib.load()
    lib.hc_packed_layout.argtypes = [U64, U64, ctypes.c_void_p]
    lib.hc_one_span.argtypes = [U64, U64, U64, U64, ctypes.c_void_p]
    lib.hc_chunk_capacity.argtypes = [U64, U64]
    lib.hc_chunk_capacity.restype = U64
    lib.hc_pinned_capacity.argtypes = [U64]
    lib.hc_pinned_capacity.restype = U64
    lib.hc_field_slices.argtypes = [U64, ctypes.c_int, ctypes.c_int, U64, ctypes.c_void_p]
    lib.hc_sub_split.argtypes = [U64, U64, U64, ctypes.c_void_p]
    lib.hc_trim_limits.argtypes = [U64, U64, ctypes.c_void_p]
    return lib


def outs(f, k, *args):
    o = (U64 * k)()
    rc = f(*args, o)
    return rc, list(o)


# ------------------------------------------------------------ packed layout
def test_packed_layout(hc):
    for n in NS:
        for mbytes in (0, 1, 64, 700 * n + 3):
            _, got = outs(hc.hc_packed_layout, 5, n, mbytes)
            msgs = 64 * n + 32 * n + 8 * (n + 1)
            assert got == [64 * n, 96 * n, msgs, msgs + mbytes, msgs + mbytes + 64], (n, mbytes)
            assert got[0] % 16 == 0 and got[1] % 8 == 0


# ---------------------------------------------------------------- one span
def span_rule(a_s, a_p, a_o, n):
    """sigs, then pks, then offsets in address order, not overlapping; span at
    most 104 n + 8 + 4096; pks 16-byte and offsets 8-byte aligned to sigs"""
    one = (a_p >= a_s + 64 * n and a_o >= a_p + 32 * n and a_o + 8 * (n + 1) - a_s <= 104 * n + 8 + 4096
           and (a_p - a_s) % 16 == 0 and (a_o - a_s) % 8 == 0)
    if one:
        return 1, [a_p - a_s, a_o - a_s, a_o + 8 * (n + 1) - a_s]
    return 0, [64 * n, 96 * n, 104 * n + 8]  # three copies land in the packed layout


def span_layouts(n, base=0x7F0000001000):
    """(name, sigs, pks, offsets, one copy?) -- None: whatever the rule says (n = 0 has nothing to overlap)"""
    s, p, o = base, base + 64 * n, base + 96 * n
    yield "exact fit", s, p, o, True
    yield "gaps of 16 and 8 (test_gpu_digest_routes)", s, p + 16, o + 16 + 8, True
    yield "gap of 4,096", s, p, o + 4096, True
    yield "gap of 4,104", s, p, o + 4104, False
    yield "gaps of 4,096 in all", s, p + 2048, o + 4096, True
    yield "keys misaligned by 8", s, p + 8, o + 8, False
    yield "offsets misaligned by 4", s, p, o + 4, False
    yield "keys before signatures", p, s, o, False if n else None
    yield "offsets before keys", s, o, p, False if n else None
    yield "offsets first", s + 8 * (n + 1), p + 8 * (n + 1), s, False
    yield "keys overlap the signatures", s, p - 16, o, False if n else None
    yield "offsets overlap the keys", s, p, o - 8, False if n else None
    yield "three far regions", s, s + (1 << 30), s + (2 << 30), False


def test_one_span(hc):
    for n in NS:
        for name, s, p, o, want_one in span_layouts(n):
            rc, got = outs(hc.hc_one_span, 3, s, p, o, n)
            assert (rc, got) == span_rule(s, p, o, n), (n, name)
            if want_one is not None:
                assert rc == int(want_one), (n, name)
            if rc:
                assert got[2] >= 104 * n + 8 and got[0] >= 64 * n and got[1] >= got[0] + 32 * n


# --------------------------------------------------------- capacity rules
def capacity_rule(need, limit):
    """powers of two from 4,096, at most the limit; never below the need"""
    c = 4096
    while c < need:
        c *= 2
    return c if c <= limit else max(limit, need)


def test_chunk_and_pinned_capacity(hc):
    for need in NS:
        for limit in CHUNKS + [8192]:
            got = hc.hc_chunk_capacity(need, limit)
            assert got == capacity_rule(need, limit), (need, limit)
            assert got >= need and (need > limit or got <= limit)
        assert hc.hc_pinned_capacity(need) == need + need // 4 + 4096


# ------------------------------------------------------------ field slices
def slices_rule(n, host_slices, bucketed):
    k = 1 if bucketed else (host_slices if host_slices else n // MIN_SLICE)
    k = min(max(k, 1), SLICES)
    if k * BLOCK > n:
        k = max(n // BLOCK, 1)
    return k, [n if i == k else (n * i // k) // BLOCK * BLOCK for i in range(k + 1)]


def test_field_slices(hc):
    for n in NS:
        for hs in range(10):  # 9 is past what edv_set_host_slices admits: clamped like 8
            for bucketed in (0, 1):
                k, rb = outs(hc.hc_field_slices, SLICES + 1, n, hs, bucketed, BLOCK)
                rb = rb[:k + 1]
                assert (k, rb) == slices_rule(n, hs, bucketed), (n, hs, bucketed)
                assert 1 <= k <= 8 and (k == 1 or not bucketed)
                assert rb[0] == 0 and rb[-1] == n and rb == sorted(rb), "the slices partition [0, n)"
                assert all(b % BLOCK == 0 for b in rb[:-1])
                if hs and not bucketed and n >= hs * BLOCK:
                    assert k == min(hs, SLICES)


# --------------------------------------------------------- sub-batch split
def split_rule(n, chunk):
    q = 2 if n > chunk and chunk >= 2 * BLOCK else 1
    pmax = chunk // q
    p = min((-(-n // q) + 63) // 64 * 64, pmax)
    return [q, pmax, p, -(-n // p) if p else 0]


def test_sub_split(hc):
    for n in NS:
        for chunk in CHUNKS:
            _, got = outs(hc.hc_sub_split, 4, n, chunk, BLOCK)
            assert got == split_rule(n, chunk), (n, chunk)
            q, pmax, p, nsub = got
            assert q * pmax <= chunk and p <= pmax
            if n:
                assert (nsub - 1) * p < n <= nsub * p, "the sub-batches partition [0, n)"
                assert (nsub == 1) == (n <= chunk), "the field path takes exactly the shards of one chunk"
    assert outs(hc.hc_sub_split, 4, 1025, 512, BLOCK)[1] == [2, 256, 256, 5]  # test_gpu_sync_routes' sub-batch route


# -------------------------------------------------------------- trim limits
def trim_rule(k, chunk):
    """the constants of trim_buffers before the limits moved into the header"""
    slots = 0
    if k:
        slots = 4096
        while slots < k and slots < chunk:
            slots *= 2
        slots = min(slots, chunk)
    packed = 104 * k + 8 + 4096 if k else 0
    blob = packed + k * 4096 + 64 if k else 0
    head = 4096 if k else 0
    return [slots, 64 * k, 32 * k, k, 32 * k, k * 4096 + 64, 8 * (k + k // (chunk // 2 or 1) + 2) if k else 0,
            8 * (k + 1) if k else 0, packed, blob, blob + blob // 4 + head, k + k // 4 + head, 32 * k + 8 * k + head]


def test_trim_limits(hc):
    for keep in NS:
        for chunk in CHUNKS:
            _, got = outs(hc.hc_trim_limits, 13, keep, chunk)
            assert got == trim_rule(keep, chunk), (keep, chunk)
            # what a batch of `keep` requests allocates survives the trim
            if keep:
                assert got[0] == hc.hc_chunk_capacity(min(keep, chunk), chunk)
                assert got[10] == hc.hc_pinned_capacity(got[9]) and got[11] == hc.hc_pinned_capacity(keep)
                assert got[8] >= 104 * keep + 8 and got[9] >= outs(hc.hc_packed_layout, 5, keep, keep * 4096)[1][4]


# ---------------------------------------------------- the sanitizer program
def test_sweeps_run_clean_under_ubsan_and_asan(tmp_path):
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx, "the sanitizer program needs the C++ compiler the harness library is built with"
    exe = str(tmp_path / "ubsan_hostplan")
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "ubsan_hostplan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr, (r.returncode, r.stderr[-2000:])
    assert r.stdout.startswith("ok "), r.stdout
