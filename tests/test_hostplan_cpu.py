"""The host paths' arithmetic (csrc/edv_hostplan.h) through the CPU build
libedv_hostcheck.so: the packed layout of a batch, the single-copy test, the
capacity rules, the field path's slices, the sub-batch split and the trim
limits, each against a plain Python restatement of its rule written here, the
sizes and trim limits of the fifteen Merkle buffers against the model of
tests/sequence_cases.py, and the same sweeps under UBSan + ASan as a
stand-alone program (tools/ubsan_hostplan.cpp)."""
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


# ------------------------------------------------------ the Merkle buffers
# The plan (merkle_extend_needs, merkle_verify_needs, merkle_trim_limits) against the model the device sequence
# tests hold edv_context_memory to (sequence_cases.merkle_needs / merkle_trim_limits, written from the arguments
# alone), entry by entry over the fifteen buffers.
MERKLE_OLD = [0, 1, 255, 256, 257, 2**20 + 12345, 2**62 - 300]
MERKLE_N = [0, 1, 255, 256, 257, 300]
MERKLE_KEEP = [0, 1, 254, 255, 256, 400, 2**20]


def model_row(sc, needs):
    want = dict.fromkeys(sc.MERKLE_BUFFERS, 0)
    for name, size in needs:
        assert want[name] == 0, "the model names %s twice" % name
        want[name] = size
    return [want[name] for name in sc.MERKLE_BUFFERS]


def plan_row(hc, sc, op, chain_step=None):
    """the plan's row for a Merkle operation of the sequence tests, from the operation's own parameters and inputs"""
    k = op.kind
    if k in ("verify_incl_host", "verify_cons_host"):
        c = sc.proof_case("incl" if "incl" in k else "cons", op.n, op.seed)
        incl = k == "verify_incl_host"
        lbytes = (32 * op.n if op.by_hash else c["lbytes"]) if incl else 0
        return outs(hc.hc_merkle_verify_needs, 15, int(incl), op.n, lbytes, c["entries"], int(bool(op.computed)))[1]
    if k == "chain_append":
        old, mbytes = chain_step["start"], 0
        flags = {"roots": True, "paths": True, "leaf": op.keep_hashes, "node": op.keep_hashes}
    elif k.startswith("append"):
        c = sc.append_inputs(op.old, op.n)
        old, mbytes, flags = c["old"], c["mbytes"], {f: op.p[f] for f in sc.APPEND_FLAGS}
    else:
        c = sc.merkle_inputs(op.old, op.n)
        old, mbytes = c["old"], c["mbytes"]
        flags = {"roots": False, "paths": False, "leaf": op.get("leaf", True), "node": op.get("node", True)}
    host = k in ("merkle_host", "append_host")
    return outs(hc.hc_merkle_extend_needs, 15, old, op.n, mbytes, int(host), int(bool(flags["leaf"])),
                int(bool(flags["node"])), int(bool(flags["roots"])), int(bool(flags["paths"])))[1]


@pytest.fixture(scope="module")
def mhc(hc):
    hc.hc_merkle_extend_needs.argtypes = [U64, U64, U64] + [ctypes.c_int] * 5 + [ctypes.c_void_p]
    hc.hc_merkle_verify_needs.argtypes = [ctypes.c_int, U64, U64, U64, ctypes.c_int, ctypes.c_void_p]
    hc.hc_merkle_trim_limits.argtypes = [U64, ctypes.c_void_p]
    return hc


MERKLE_LISTS = ("merkle_staging", "merkle_fold_streams", "ledger_chain", "release_in_the_middle", "random_merkle_110",
                "random_merkle_214")


@pytest.mark.parametrize("name", MERKLE_LISTS)
def test_merkle_needs_of_the_sequence_lists(mhc, monkeypatch, name):
    import sequence_cases as sc
    ops, devices, _seed = sc.sequence(name)
    seen, model = [], sc.merkle_needs

    def recording(op, chain_step=None):
        needs = model(op, chain_step)
        seen.append((op, chain_step, needs))
        return needs
    monkeypatch.setattr(sc, "merkle_needs", recording)
    trace = sc.trace_of(ops, devices)
    merkle_ops = [op for op in ops if op.kind in ("merkle_host", "merkle_device", "append_host", "append_device",
                                                  "chain_append", "verify_incl_host", "verify_cons_host")]
    assert [s[0] for s in seen] == merkle_ops and (merkle_ops or name == "release_in_the_middle"), name
    for op, chain_step, needs in seen:
        assert plan_row(mhc, sc, op, chain_step) == model_row(sc, needs), (name, op)
    for t in trace:
        if t["kind"] == "trim":
            k = t["op"].keep
            assert outs(mhc.hc_merkle_trim_limits, 15, k)[1] == model_row(sc, sc.merkle_trim_limits(k).items()), (name, k)


def test_merkle_extend_needs_sweep(mhc, monkeypatch):
    import merkle_append_cases as ac
    import merkle_cases as mc
    import sequence_cases as sc

    def inputs(old, n):  # the sizes alone: `old` is the tree size itself here, no leaves are made
        return {"old": old, "n": n, "nodes": mc.node_span(old, n), "mbytes": 700 * n + 3, "entries": ac.path_entries(old, n)}
    monkeypatch.setattr(sc, "append_inputs", inputs)
    for old in MERKLE_OLD:
        for n in MERKLE_N:
            assert old + n <= 2**62
            for bits in range(16):
                flags = {f: bool(bits >> i & 1) for i, f in enumerate(sc.APPEND_FLAGS)}
                for host in (1, 0):
                    op = sc.Op("append_host" if host else "append_device", old=old, n=n, **flags)
                    got = plan_row(mhc, sc, op)
                    assert got == model_row(sc, sc.merkle_needs(op)), (old, n, flags, host)
                    assert all(g == 0 for g, b in zip(got, sc.MERKLE_BUFFERS) if b.startswith("mv_"))


def test_merkle_verify_needs_sweep(mhc, monkeypatch):
    import sequence_cases as sc
    for n in MERKLE_N[1:] + [4097]:
        for entries in (0, 1, 64 * n):
            monkeypatch.setattr(sc, "proof_case", lambda kind, n_, seed: {"entries": entries, "lbytes": 300 * n_ + 1})
            for kind in ("verify_incl_host", "verify_cons_host"):
                for computed in (False, True):
                    for by_hash in ((False, True) if "incl" in kind else (False,)):
                        op = sc.Op(kind, n=n, seed=0, computed=computed, by_hash=by_hash)
                        got = plan_row(mhc, sc, op)
                        assert got == model_row(sc, sc.merkle_needs(op)), (n, entries, kind, computed, by_hash)
                        assert got[sc.MERKLE_BUFFERS.index("mv_proofs")] >= 32, "mv_proofs is never asked for empty"


def test_merkle_trim_limits(mhc):
    import sequence_cases as sc
    for keep in MERKLE_KEEP + list(sc.TRIMS):
        got = outs(mhc.hc_merkle_trim_limits, 15, keep)[1]
        assert got == model_row(sc, sc.merkle_trim_limits(keep).items()), keep
        if keep:  # what an extend or a verify of `keep` leaves of 4,096 bytes needs survives the trim
            old = 2**20 + 12345
            for host in (1, 0):
                need = outs(mhc.hc_merkle_extend_needs, 15, old, keep, 4096 * keep, host, 0, 0, 1, 1)[1]
                # ... but for the node hashes, limited to 32 keep: n leaves make up to n + popcount(old) - 1 nodes
                slack = [32 * bin(old).count("1") if "nodeh" in b else 0 for b in sc.MERKLE_BUFFERS]
                assert all(n <= g + s for n, g, s in zip(need, got, slack)), (keep, host)
            for incl in (1, 0):
                need = outs(mhc.hc_merkle_verify_needs, 15, incl, keep, 4096 * keep, 64 * keep, 1)[1]
                assert all(n <= g for n, g in zip(need, got)), (keep, incl)


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
