"""GPU parity: the HIP verifier through the C-ABI (libedv.so) against libsodium
1.0.18's own verdicts (committed golden fixtures and corpus bitmasks) and the
oracle.  Bit-exact accept/reject is the bar (integer work, no tolerance).
"""
import hashlib
import json
import os

import numpy as np
import pytest

import golden_io
import oracle_lib as orc
from indy_plenum_amd import edv

pytestmark = pytest.mark.gpu
GOLDEN = golden_io.GOLDEN


@pytest.fixture(scope="module", autouse=True)
def gpu_present():
    assert edv.device_count() >= 1, "no gfx950 device visible: the GPU suite must run on the MI355X box"
    assert edv.version().endswith("gfx950")


def checker(sigs, pks, msgs, off):
    """libsodium 1.0.18 (batch harness) if present, else the oracle, 16 threads."""
    if orc.sodium_batch() is not None:
        return orc.sodium_verify_batch(sigs, pks, msgs, off, 16)
    return np.frombuffer(orc.verify_batch(sigs.tobytes(), pks.tobytes(), msgs.tobytes(), off, len(off) - 1, 16),
                         dtype=np.uint8)


def test_golden_every_category(golden, golden_meta):
    sigs, pks, msgs, off = golden_io.pack_batch(golden)
    got = edv.verify_arrays(sigs, pks, msgs + b"\0" * 16, off)
    want = np.array([g[0] for g in golden], dtype=np.uint8)
    cats = golden_meta["categories"]
    bad = [(int(i), cats[golden[i][1]]) for i in np.nonzero(got != want)[0]]
    assert bad == []
    assert int(got.sum()) == golden_meta["accepted"]


def test_open_positional_split_golden():
    rows = golden_io.load_open_golden()
    got = edv.open_batch([(s, m, p) for s, m, p, _a in rows])
    assert got == [bool(a) for *_x, a in rows]


def test_single_and_empty_batches(golden):
    assert edv.verify_arrays(b"", b"", b"", np.zeros(1, dtype=np.uint64)).size == 0
    for v, _c, sig, pk, msg in golden[:40]:
        assert edv.verify_detached_batch([(sig, msg, pk)]) == [bool(v)]


def test_message_alignment_and_offsets(golden):
    """Messages at every byte offset (unaligned starts) and a non-zero msg_base."""
    recs = [g for g in golden if len(g[4]) > 0][:300]
    sigs = b"".join(r[2] for r in recs)
    pks = b"".join(r[3] for r in recs)
    for pad in range(1, 8):
        # and the raw C-ABI layout with a leading pad (offsets start at `pad`)
        blob2 = b"\xAA" * pad + b"".join(r[4] for r in recs) + b"\0" * 16
        o2 = np.zeros(len(recs) + 1, dtype=np.uint64)
        o2[0] = pad
        o2[1:] = pad + np.cumsum([len(r[4]) for r in recs])
        got2 = edv.verify_arrays(sigs, pks, blob2, o2)
        assert got2.tolist() == [r[0] for r in recs]


def test_random_corpus_c2_vs_libsodium():
    sigs, pks, msgs, off = orc.corpus(0xABCDEF, 0, 40000, mode=0, invalid_permille=100)
    got = edv.verify_arrays(sigs, pks, msgs, off)
    want = checker(sigs, pks, msgs, off)
    assert np.array_equal(got, want)
    assert 0.85 < want.mean() < 0.95


def test_variable_length_c4_vs_libsodium():
    sigs, pks, msgs, off = orc.corpus(0xC4, 0, 6000, mode=1, invalid_permille=50)
    got = edv.verify_arrays(sigs, pks, msgs, off)
    assert np.array_equal(got, checker(sigs, pks, msgs, off))


def _signed_lengths(lens, seed):
    """Requests of the given message lengths, signed by the oracle (libsodium's
    algorithm), a fifth of them damaged: a message bit (often the last byte of a
    long message), an R bit or an S bit."""
    import random
    r = random.Random(seed)
    sigs, pks, msgs = [], [], []
    for i, n in enumerate(lens):
        pk, sk = orc.keypair(bytes([i & 255, i >> 8, seed & 255]) * 10 + b"LM")
        m = bytearray(r.getrandbits(8) for _ in range(min(n, 4096))) * (n // 4096 + 1)
        m = m[:n]
        sig = bytearray(orc.sign(bytes(m), sk))
        k = r.randrange(15)
        if n == 0 and k == 1:
            k = 2
        if k == 1:
            m[n - 1 if r.random() < 0.5 else r.randrange(n)] ^= 1 << r.randrange(8)
        elif k == 2:
            sig[r.randrange(32)] ^= 1 << r.randrange(8)
        elif k == 3:
            sig[32 + r.randrange(31)] ^= 1 << r.randrange(8)
        sigs.append(bytes(sig))
        pks.append(pk)
        msgs.append(bytes(m))
    off = np.zeros(len(lens) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(m) for m in msgs])
    return (np.frombuffer(b"".join(sigs), np.uint8), np.frombuffer(b"".join(pks), np.uint8),
            np.frombuffer(b"".join(msgs) + b"\0" * 16, np.uint8), off)


def test_long_and_skewed_message_lengths():
    """Message lengths far outside C2/C4 (up to 1 MiB, as the reference's verify
    accepts any length) and around SHA-512 block boundaries, with a few very long
    messages among many short ones (one length bucket holding them all, another
    holding the rest), at the batch's start, middle and end, and across chunk
    seams; verdicts equal libsodium's (the oracle where it is absent)."""
    import random
    r = random.Random(0x10C)
    edges = [0, 1, 46, 47, 48, 63, 64, 111, 112, 113, 127, 128, 129, 175, 176, 239, 240, 241, 255, 256, 4096]
    long_ = [1 << 14, (1 << 16) + 3, 1 << 18, 1 << 20]
    lens = [1 << 20] + [r.choice(edges) for _ in range(700)] + long_ + [r.randrange(2000) for _ in range(700)] \
        + [(1 << 20) - 1]
    sigs, pks, msgs, off = _signed_lengths(lens, 0x5A)
    want = checker(sigs, pks, msgs, off)
    assert 0.65 < want.mean() < 0.95
    assert np.array_equal(edv.verify_arrays(sigs, pks, msgs, off), want)   # the latency path (n <= its default limit)
    try:
        edv.set_latency_path(0, 0)   # the batch kernels, across chunk seams
        for chunk in (256, 1024, 0):
            edv.set_chunk(0, chunk)
            assert np.array_equal(edv.verify_arrays(sigs, pks, msgs, off), want), chunk
    finally:
        edv.set_chunk(0, 0)
        edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT)


@pytest.mark.parametrize("mode", [0, 1])
def test_chunk_seams(mode):
    """Batches spanning several prep/main chunk pairs (chunk forced small); mode 1
    (200..4096 B) also exercises the per-chunk SHA length buckets."""
    sigs, pks, msgs, off = orc.corpus(0x5EA + mode, 0, 5000, mode=mode, invalid_permille=200)
    want = checker(sigs, pks, msgs, off)
    edv.set_latency_path(0, 0)   # the batch kernels (5,000 requests would take the latency path)
    try:
        for chunk in (256, 768, 4096):
            edv.set_chunk(0, chunk)
            assert np.array_equal(edv.verify_arrays(sigs, pks, msgs, off), want), chunk
    finally:
        edv.set_chunk(0, 0)  # back to the default
        edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT)


def test_fuzzed_damage_vs_libsodium():
    """Random damage anywhere (tools/parity_live_sodium.py's fuzz corpus, one
    2^16 slice): 1-3 random bit flips over sig || pk || msg, or a random R, S
    or A, on valid C2 requests made by the GPU signer; verdicts equal
    libsodium's (the oracle where it is absent)."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import parity_live_sodium as pl
    if orc.sodium_batch() is None:
        pytest.skip("libsodium batch harness absent")
    out = pl.fuzz(65536, seed=0xF1)
    assert out["requests"] == 65536 and out["mismatches"] == 0, out
    assert 0.4 < out["libsodium_rejected"] / 65536 < 0.8


def test_bench_corpora_vs_libsodium_live():
    """The bench's own generators (tools/parity_live_sodium.py: C3's 256-B
    requests with four damage kinds, C4's 200..4,096-B requests with seven,
    and the fuzz corpus through the synchronous host path in one-slice and
    four-slice calls), verified on the GPU and by libsodium 1.0.18 itself on the
    host, every verdict compared: the bench's corpora are checked against
    libsodium here, not only by construction."""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import parity_live_sodium as pl
    if orc.sodium_batch() is None:
        pytest.skip("libsodium batch harness absent")
    c3 = pl.run("C3", 1 << 20, damage_every=20, damage_kinds=4)
    c4 = pl.run("C4", 1 << 18, seed=0xC4C4, var_range=(200, 4096), damage_every=20, damage_kinds=7)
    assert c3["mismatches"] == 0 and c3["libsodium_rejected"] == len(range(0, 1 << 20, 20)), c3
    assert c4["mismatches"] == 0 and c4["libsodium_rejected"] > 0, c4
    saved = os.environ.get("FUZZ_SLICE")
    try:
        for sl in (1 << 16, 1 << 18):       # one message slice, four
            os.environ["FUZZ_SLICE"] = str(sl)
            out = pl.fuzz(1 << 18, seed=0xF2 + sl)
            assert out["requests"] == 1 << 18 and out["mismatches"] == 0, out
    finally:
        if saved is None:
            os.environ.pop("FUZZ_SLICE", None)
        else:
            os.environ["FUZZ_SLICE"] = saved


def test_full_size_c2_properties():
    """BASELINE configs[1] size (65,536 x 256 B, distinct signers): all valid
    accept; every kind of single-bit/malleation damage rejects exactly where applied."""
    n = 65536
    sigs, pks, msgs, off = orc.corpus(0x5EED2025, 0, n, mode=0, invalid_permille=0)
    assert edv.verify_arrays(sigs, pks, msgs, off).all()
    rng = np.random.default_rng(5)
    bad = np.sort(rng.choice(n, size=4096, replace=False))
    s2, p2, m2 = sigs.copy(), pks.copy(), msgs.copy()
    L = 2**252 + 27742317777372353535851937790883648493
    for k, i in enumerate(bad):
        kind = k % 4
        if kind == 0:
            s2[64 * i + rng.integers(32)] ^= 1 << rng.integers(8)            # R bit
        elif kind == 1:
            m2[int(off[i]) + rng.integers(256)] ^= 1 << rng.integers(8)      # message bit
        elif kind == 2:
            s = int.from_bytes(s2[64 * i + 32:64 * i + 64].tobytes(), "little") + L
            s2[64 * i + 32:64 * i + 64] = np.frombuffer(s.to_bytes(32, "little"), np.uint8)  # S + L
        else:
            p2[32 * i + rng.integers(32)] ^= 1 << rng.integers(8)            # key bit
    got = edv.verify_arrays(s2, p2, m2, off)
    want = np.ones(n, dtype=np.uint8)
    want[bad] = 0
    # a flipped key bit can, rarely, still decode to a point that verifies: never for these seeds
    assert np.array_equal(got, want)


def _bitmask_meta():
    with open(os.path.join(GOLDEN, "corpus_bitmask.json")) as f:
        return json.load(f)


@pytest.mark.slow
@pytest.mark.parametrize("name", ["c2_256B", "c4_var"])
def test_big_corpus_parity(name):
    """Seeded >= 10M-case corpus vs libsodium's committed verdict bitmask: every
    slice (c2_256B: 10 x 1,048,576 = 10,485,760 requests; c4_var: 1,048,576).
    EDV_PARITY_QUICK=1 (local iteration only) runs the middle slice."""
    meta = _bitmask_meta()
    cfg = meta["corpora"][name]
    slice_n = meta["slice"]
    nslices = cfg["count"] // slice_n
    bits = np.fromfile(os.path.join(GOLDEN, "corpus_%s.bits" % name), dtype=np.uint8)
    todo = [nslices // 2] if os.environ.get("EDV_PARITY_QUICK") == "1" else range(nslices)
    for s in todo:
        sigs, pks, msgs, off = orc.corpus(cfg["seed"], s * slice_n, slice_n, cfg["mode"], cfg["invalid_permille"])
        h = hashlib.sha256()
        h.update(sigs.tobytes())
        h.update(pks.tobytes())
        h.update(msgs[:int(off[-1])].tobytes())
        assert h.hexdigest() == cfg["slice_sha256"][s], "corpus regeneration differs from the bitmask's corpus"
        got = edv.verify_arrays(sigs, pks, msgs, off)
        want = np.unpackbits(bits[s * slice_n // 8:(s + 1) * slice_n // 8], bitorder="little")
        assert int(want.sum()) == cfg["slice_accepts"][s]
        mism = np.nonzero(got != want)[0]
        assert mism.size == 0, (s, mism[:10].tolist())


@pytest.mark.slow
def test_big_corpus_split_pipeline():
    """The split pipeline (EDV_FLAG_SPLIT_PREP, the C4 leg's fast mode) on the
    whole c4_var corpus (1,048,576 requests of 200..4,096 B, 5 % invalid) against
    libsodium's committed bitmask, in 65,536-request chunks as at C4: every
    chunk's hash side runs beside the previous chunk's main kernel.
    EDV_PARITY_QUICK=1 runs the first 262,144 requests."""
    meta = _bitmask_meta()
    cfg = meta["corpora"]["c4_var"]
    n = 262144 if os.environ.get("EDV_PARITY_QUICK") == "1" else cfg["count"]
    sigs, pks, msgs, off = orc.corpus(cfg["seed"], 0, n, cfg["mode"], cfg["invalid_permille"])
    bits = np.fromfile(os.path.join(GOLDEN, "corpus_c4_var.bits"), dtype=np.uint8)
    want = np.unpackbits(bits[:n // 8], bitorder="little")
    bufs = [edv.DeviceBuffer(a.nbytes + 64) for a in (sigs, pks, msgs, off)]
    for b, a in zip(bufs, (sigs, pks, msgs, off)):
        b.upload(a)
    acc = edv.DeviceBuffer(n)
    acc.upload(np.full(n, 7, np.uint8))
    try:
        edv.set_chunk(0, 65536)
        for _ in range(2):   # the second pass runs with both state sets already in use
            edv.verify_device_pipelined(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, acc.ptr,
                                        flags=edv.FLAG_SPLIT_PREP)
        edv.pipeline_sync(0)
    finally:
        edv.set_chunk(0, 0)
    got = acc.download(n)
    mism = np.nonzero(got != want)[0]
    assert mism.size == 0, mism[:10].tolist()


def test_device_resident_entry_point():
    sigs, pks, msgs, off = orc.corpus(0xD1, 0, 3000, mode=1, invalid_permille=100)
    want = checker(sigs, pks, msgs, off)
    bufs = [edv.DeviceBuffer(a.nbytes) for a in (sigs, pks, msgs, off)]
    for b, a in zip(bufs, (sigs, pks, msgs, off)):
        b.upload(a)
    acc = edv.DeviceBuffer(3000)
    edv.verify_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 3000, acc.ptr)
    assert np.array_equal(acc.download(3000), want)
    # a shard: items [1000, 3000) with the global offset array slice and msg_base
    o = off[1000:].copy()
    mb = edv.DeviceBuffer(int(o[-1] - o[0]) + 64)
    mb.upload(msgs[int(o[0]):int(o[-1])])
    ob = edv.DeviceBuffer(o.nbytes)
    ob.upload(o)
    sb, pb = edv.DeviceBuffer(2000 * 64), edv.DeviceBuffer(2000 * 32)
    sb.upload(sigs[64000:])
    pb.upload(pks[32000:])
    edv.verify_device(sb.ptr, pb.ptr, mb.ptr, ob.ptr, 2000, acc.ptr, msg_base=int(o[0]))
    assert np.array_equal(acc.download(2000), want[1000:])


MSG_BASES = (0, 2**32 - 1, 2**32 + 5, 2**40 + 3)


def _with_bases(off):
    """The offset array shifted by each msg_base, uploaded; the data pointers stay."""
    out = []
    for base in MSG_BASES:
        o = off + np.uint64(base)
        b = edv.DeviceBuffer(o.nbytes)
        b.upload(o)
        out.append((base, b))
    return out


def test_msg_base_above_2_to_32_on_every_device_entry_point(latency_limit):
    """A C3 shard passes global offsets with its msg_base: 64-bit, and above
    2^32 once 16 M requests carry more than 256 B.  Every device-resident entry
    point computes off[i] - msg_base itself, in every kernel family: one
    600-request batch of varied lengths (200..4,096 B, a fifth damaged) with
    msg_base 0, 2^32 - 1, 2^32 + 5 and 2^40 + 3 (the offsets shifted by as much,
    the message pointer unchanged) through verify_device on the right-to-left
    latency kernel, on the batch kernels (length buckets forced, left to the
    device mode, and off), verify_device_pipelined, sha256_device and
    sign_device; 4,097 requests once for the two-walk latency kernel.  Every
    result equals the checker's, hashlib's and the signing golden's, at every
    base: 600 x 4 x 5 + 4,097 x 4 verdicts, 600 x 4 digests, 600 x 4 signatures."""
    N = 4097
    sigs, pks, msgs, off = orc.corpus(0xB45E, 0, N, mode=1, invalid_permille=200)
    want = checker(sigs, pks, msgs, off)
    assert 0 < want[:600].sum() < 600
    ds, dp, dm = (edv.DeviceBuffer(a.nbytes + 64) for a in (sigs, pks, msgs))
    for b, a in zip((ds, dp, dm), (sigs, pks, msgs)):
        b.upload(a)
    acc = edv.DeviceBuffer(N)
    seven = np.full(N, 7, np.uint8)

    def verdicts(n, run):
        acc.upload(seven)
        run()
        return acc.download(n)

    runs = [("latency, right-to-left", edv.LATENCY_PATH_DEFAULT, 600, 0, False),
            ("latency, two-walk", edv.LATENCY_PATH_DEFAULT, N, 0, False),
            ("batch, buckets", 0, 600, edv.FLAG_BUCKETS, False),
            ("batch, device mode", 0, 600, 0, False),
            ("batch, uniform hint", 0, 600, edv.FLAG_UNIFORM_LENGTH, False),
            ("pipelined", 0, 600, 0, True)]
    for what, limit, n, flags, pipelined in runs:
        latency_limit(limit)
        for base, dob in _with_bases(off[:n + 1]):
            if pipelined:
                def run():
                    edv.verify_device_pipelined(ds.ptr, dp.ptr, dm.ptr, dob.ptr, n, acc.ptr, msg_base=base, flags=flags)
                    edv.pipeline_sync(0)
            else:
                def run():
                    edv.verify_device(ds.ptr, dp.ptr, dm.ptr, dob.ptr, n, acc.ptr, msg_base=base, flags=flags)
            got = verdicts(n, run)
            assert np.array_equal(got, want[:n]), (what, base, np.nonzero(got != want[:n])[0][:8].tolist())
    # SHA-256 of the same 600 messages
    digests = b"".join(hashlib.sha256(msgs[int(off[i]):int(off[i + 1])].tobytes()).digest() for i in range(600))
    dd = edv.DeviceBuffer(32 * 600)
    for base, dob in _with_bases(off[:601]):
        dd.upload(np.full(32 * 600, 7, np.uint8))
        edv.sha256_device(dm.ptr, dob.ptr, 600, dd.ptr, msg_base=base)
        assert dd.download(32 * 600).tobytes() == digests, base
    # the signer, on the first 600 libsodium signing vectors
    vec = golden_io.load_sign_golden()[:600]
    seeds, smsgs, soff = golden_io.pack_sign_batch(vec)
    assert len(vec) == 600 and len({len(r[1]) for r in vec}) > 50
    dseed, dsm = edv.DeviceBuffer(len(seeds) + 64), edv.DeviceBuffer(len(smsgs) + 64)
    dseed.upload(np.frombuffer(seeds, np.uint8))
    dsm.upload(np.frombuffer(smsgs + b"\0" * 16, np.uint8))
    dpk, dsig = edv.DeviceBuffer(32 * 600), edv.DeviceBuffer(64 * 600)
    for base, dob in _with_bases(soff):
        dpk.upload(np.full(32 * 600, 7, np.uint8))
        dsig.upload(np.full(64 * 600, 7, np.uint8))
        edv.sign_device(dseed.ptr, dsm.ptr, dob.ptr, 600, dpk.ptr, dsig.ptr, msg_base=base)
        assert dpk.download(32 * 600).tobytes() == b"".join(r[2] for r in vec), base
        assert dsig.download(64 * 600).tobytes() == b"".join(r[3] for r in vec), base


def test_device_mask_selects_device():
    sigs, pks, msgs, off = orc.corpus(0xE1, 0, 1000, mode=0, invalid_permille=300)
    want = checker(sigs, pks, msgs, off)
    assert np.array_equal(edv.verify_arrays(sigs, pks, msgs, off, device_mask=1), want)
    with pytest.raises(edv.EdvUnavailable):
        edv.verify_arrays(sigs, pks, msgs, off, device_mask=1 << 20)


@pytest.mark.parametrize("flags", [0, edv.FLAG_SPLIT_PREP, edv.FLAG_SPLIT_PREP | edv.FLAG_UNIFORM_LENGTH])
def test_pipelined_submission_matches(flags):
    """edv_verify_batch_dev_pipelined: several different batches in flight on the
    two-stream pipeline (state sets alternate) give each batch its own verdicts;
    also with the split prep (EDV_FLAG_SPLIT_PREP: the hash side of batch k+1
    beside the main kernel of batch k, the point sides on the main stream), with
    and without length buckets."""
    batches = []
    for k in range(5):
        sigs, pks, msgs, off = orc.corpus(0x919 + k, 0, 1500 + 300 * k, mode=k % 2, invalid_permille=150)
        want = checker(sigs, pks, msgs, off)
        bufs = [edv.DeviceBuffer(a.nbytes + 64) for a in (sigs, pks, msgs, off)]
        for b, a in zip(bufs, (sigs, pks, msgs, off)):
            b.upload(a)
        acc = edv.DeviceBuffer(len(want))
        batches.append((bufs, acc, want))
    try:
        edv.set_chunk(0, 1024)  # several chunks per batch: the pipeline alternates within a batch too
        for _ in range(2):
            for bufs, acc, want in batches:
                edv.verify_device_pipelined(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, len(want), acc.ptr,
                                            flags=flags)
            edv.pipeline_sync(0)
            for bufs, acc, want in batches:
                assert np.array_equal(acc.download(len(want)), want)
    finally:
        edv.set_chunk(0, 0)


def test_sha256_batch_vs_hashlib():
    """Row f-3: edv_sha256_batch (gfx950) == hashlib.sha256 for every message of a
    ragged batch (empty, block-boundary and 4 KB lengths, unaligned starts), on
    the host path and the device-resident path."""
    import random
    r = random.Random(12)
    lens = list(range(0, 140)) + [r.randrange(0, 4097) for _ in range(3000)] + [4096, 55, 56, 64]
    msgs = [bytes(r.getrandbits(8) for _ in range(n)) for n in lens]
    got = edv.sha256_batch(msgs)
    assert got == [hashlib.sha256(m).digest() for m in msgs]
    assert edv.sha256_batch([]) == []
    # device-resident, with a msg_base and a leading pad so starts are unaligned
    blob = b"\x11" * 3 + b"".join(msgs) + b"\0" * 16
    off = np.zeros(len(msgs) + 1, dtype=np.uint64)
    off[0] = 3
    off[1:] = 3 + np.cumsum(lens)
    dm, do, dd = edv.DeviceBuffer(len(blob)), edv.DeviceBuffer(off.nbytes), edv.DeviceBuffer(32 * len(msgs))
    dm.upload(np.frombuffer(blob, np.uint8))
    do.upload(off)
    edv.sha256_device(dm.ptr, do.ptr, len(msgs), dd.ptr)
    assert dd.download(32 * len(msgs)).tobytes() == b"".join(hashlib.sha256(m).digest() for m in msgs)


def test_request_digests_and_state_keys():
    """Request.getDigest / nym_to_state_key semantics (request.py:71-72,
    domain_req_handler.py:166-167), pinned by the reference serializer's own
    outputs: for golden requests whose keys are exactly signingState's, the
    digest must be the hex SHA-256 of the reference's serialized bytes."""
    from indy_plenum_amd import digest
    keys = {"identifier", "reqId", "operation", "protocolVersion"}
    cases = [c for c in golden_io.load_serializer_golden() if isinstance(c["msg"], dict) and not c["ignore"]
             and {"identifier", "reqId", "operation"} <= set(c["msg"]) <= keys]
    assert len(cases) >= 3
    reqs = [dict(c["msg"], signature="sig-is-not-hashed") for c in cases]
    want = [hashlib.sha256(c["ser"].encode()).hexdigest() for c in cases]
    assert digest.request_digests(reqs) == want
    nyms = [c["msg"]["identifier"] for c in cases] + ["", "V4SGRU86Z58d6TV7PBUe6f"]
    assert digest.nym_state_keys(nyms) == [hashlib.sha256(n.encode()).digest() for n in nyms]


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_length_bucket_modes_same_verdicts(mode):
    """edv_set_length_buckets never changes verdicts (device path, ragged batch)."""
    sigs, pks, msgs, off = orc.corpus(0xB0C + mode, 0, 3000, mode=1, invalid_permille=120)
    want = checker(sigs, pks, msgs, off)
    bufs = [edv.DeviceBuffer(a.nbytes + 64) for a in (sigs, pks, msgs, off)]
    for b, a in zip(bufs, (sigs, pks, msgs, off)):
        b.upload(a)
    acc = edv.DeviceBuffer(3000)
    try:
        edv.set_latency_path(0, 0)   # the batch kernels, where the buckets apply
        edv.set_length_buckets(0, mode)
        edv.verify_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 3000, acc.ptr)
        assert np.array_equal(acc.download(3000), want)
    finally:
        edv.set_length_buckets(0, 2)
        edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT)


# ---- the latency path (edv_quad.hip): sixteen / eight lanes per signature, one launch
@pytest.fixture
def latency_limit():
    """Set the latency path's batch limit of device 0 for one test, restored after."""
    def setter(limit):
        edv.set_latency_path(0, limit)
    yield setter
    edv.set_latency_path(0, edv.LATENCY_PATH_DEFAULT)


@pytest.mark.parametrize("limit", [0, 16384])
def test_golden_on_both_paths(golden, golden_meta, latency_limit, limit):
    """The 3,284 libsodium golden cases (every strictness category: S + kL,
    torsion and mixed-order A accepted iff 8 | h, small-order and non-canonical
    R / A, off-curve points, ...) on the batch kernels (limit 0) and on the
    latency kernel (limit 16,384: the whole set in one launch), and the
    positional-split cases through open_batch."""
    latency_limit(limit)
    sigs, pks, msgs, off = golden_io.pack_batch(golden)
    got = edv.verify_arrays(sigs, pks, msgs + b"\0" * 16, off)
    want = np.array([g[0] for g in golden], dtype=np.uint8)
    cats = golden_meta["categories"]
    assert [(int(i), cats[golden[i][1]]) for i in np.nonzero(got != want)[0]] == []
    rows = golden_io.load_open_golden()
    assert edv.open_batch([(s, m, p) for s, m, p, _a in rows]) == [bool(a) for *_x, a in rows]


def test_latency_path_batch_sizes_and_entry_points(latency_limit):
    """Batch sizes around the latency kernel's 32-signature workgroups, its
    16-slot padding of tiny batches and its limit, variable message lengths (200..4,096 B) and 20 % damage, through the
    synchronous call, the asynchronous one (pageable and page-locked verdicts)
    and the device-resident one with a non-zero msg_base; verdicts equal
    libsodium's (the oracle where it is absent).  Up to the default limit,
    16,384 requests (the two-walk kernel above 4,096 at two waves per SIMD)."""
    latency_limit(edv.LATENCY_PATH_DEFAULT)
    N = edv.LATENCY_PATH_DEFAULT
    sigs, pks, msgs, off = orc.corpus(0x1A7, 0, N, mode=1, invalid_permille=200)
    want = checker(sigs, pks, msgs, off)
    for n in (1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 400, 1000, 4095, 4096, 4097, 8192,
              8193, 12289, N - 1, N):
        o = off[:n + 1]
        got = edv.verify_arrays(sigs[:64 * n], pks[:32 * n], msgs, o)
        assert np.array_equal(got, want[:n]), n
    pin = edv.PinnedBuffer(N)
    for n, acc in ((400, np.zeros(400, np.uint8)), (8192, pin.array[:8192]), (N, np.zeros(N, np.uint8)),
                   (N, pin.array[:N])):
        ts = [edv.verify_async(sigs[:64 * n], pks[:32 * n], msgs, off[:n + 1], acc) for _ in range(1)]
        for t in ts:
            edv.wait_async(t)
        assert np.array_equal(acc, want[:n]), n
    pin.free()
    # device resident: requests [1000, 3000) with the global offsets and msg_base
    o = off[1000:3001].copy()
    bufs = [edv.DeviceBuffer(x.nbytes + 64) for x in (sigs[64000:192000], pks[32000:96000],
                                                      msgs[int(o[0]):int(o[-1])], o)]
    for b, x in zip(bufs, (sigs[64000:192000], pks[32000:96000], msgs[int(o[0]):int(o[-1])], o)):
        b.upload(x)
    acc = edv.DeviceBuffer(2000)
    acc.upload(np.full(2000, 7, np.uint8))
    edv.verify_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, 2000, acc.ptr, msg_base=int(o[0]))
    assert np.array_equal(acc.download(2000), want[1000:3000])


def test_latency_path_on_corpus_bitmask_slices(latency_limit):
    """The latency kernel against libsodium's committed corpus bitmasks: the
    first 2^18 requests of the C2 corpus (256 B) and of the C4 corpus
    (200..4,096 B, 5 % invalid over every damage kind), in 4,096-request calls
    (the right-to-left kernel) and in 16,384-request calls (the two-walk
    kernel at the default limit), slice hashes checked first."""
    meta = _bitmask_meta()
    for name in ("c2_256B", "c4_var"):
        cfg = meta["corpora"][name]
        n = 262144
        sigs, pks, msgs, off = orc.corpus(cfg["seed"], 0, n, cfg["mode"], cfg["invalid_permille"])
        bits = np.fromfile(os.path.join(GOLDEN, "corpus_%s.bits" % name), dtype=np.uint8)
        want = np.unpackbits(bits[:n // 8], bitorder="little")
        for step in (4096, 16384):   # the right-to-left kernel, then the two-walk kernel at two waves per SIMD
            latency_limit(step)
            got = np.zeros(n, np.uint8)
            for lo in range(0, n, step):
                got[lo:lo + step] = edv.verify_arrays(sigs[64 * lo:64 * (lo + step)], pks[32 * lo:32 * (lo + step)],
                                                      msgs, off[lo:lo + step + 1])
            mism = np.nonzero(got != want)[0]
            assert mism.size == 0, (name, step, mism[:10].tolist())


# ---- the edge batch (tests/golden/prep_edge_golden.json): requests chosen for
# the prep stage's rare paths, verdicts by libsodium 1.0.18, on every product route
def _edge():
    import stage_cases as sc
    b = sc.edge_requests()
    want = np.array([q["valid"] for q in b["reqs"]], np.uint8)
    assert len(want) == 395 and int(want.sum()) == 37
    assert want.tolist() == [int(q["family"] == "accepted") for q in b["reqs"]]
    return b["sigs"], b["pks"], b["msgs"], b["off"], want


def test_edge_batch_on_every_route(latency_limit):
    """S with edge digits of both table sets, Q = [S]B - R the identity or of
    small order, S in [2^252, L) and around L, mixed-order keys, B and -B, and
    37 accepted signatures with a zero or -half digit: the batch kernels, the
    right-to-left latency kernel, the two-walk kernel (the batch tiled to 4,097
    requests), verify_device with EDV_FLAG_BUCKETS and the pipelined entry
    point all give the fixture's libsodium verdicts, and live libsodium (where
    present) gives them too."""
    sigs, pks, msgs, off, want = _edge()
    n = len(want)
    if orc.sodium_batch() is not None:
        assert np.array_equal(orc.sodium_verify_batch(sigs, pks, msgs, off, 16), want)
    assert orc.verify_batch(sigs.tobytes(), pks.tobytes(), msgs.tobytes(), off, n, 8) == want.tobytes()

    def same(got, want, what):
        assert np.array_equal(got, want), (what, np.nonzero(got != want)[0][:10].tolist())

    latency_limit(0)
    same(edv.verify_arrays(sigs, pks, msgs, off), want, "batch kernels")
    latency_limit(edv.LATENCY_PATH_DEFAULT)
    same(edv.verify_arrays(sigs, pks, msgs, off), want, "right-to-left kernel")
    N = 4097
    times = N // n + 1
    lens = np.tile(np.diff(off), times)[:N]
    toff = np.zeros(N + 1, np.uint64)
    toff[1:] = np.cumsum(lens)
    tmsgs = np.concatenate([np.tile(msgs[:int(off[-1])], times), np.zeros(64, np.uint8)])
    same(edv.verify_arrays(np.tile(sigs, times)[:64 * N], np.tile(pks, times)[:32 * N], tmsgs, toff),
         np.tile(want, times)[:N], "two-walk kernel")
    bufs = [edv.DeviceBuffer(a.nbytes + 64) for a in (sigs, pks, msgs, off)]
    for b, a in zip(bufs, (sigs, pks, msgs, off)):
        b.upload(a)
    acc = edv.DeviceBuffer(n)
    latency_limit(0)
    acc.upload(np.full(n, 7, np.uint8))
    edv.verify_device(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, acc.ptr, flags=edv.FLAG_BUCKETS)
    same(acc.download(n), want, "verify_device, buckets")
    for flags in (0, edv.FLAG_SPLIT_PREP):
        acc.upload(np.full(n, 7, np.uint8))
        edv.verify_device_pipelined(bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, bufs[3].ptr, n, acc.ptr, flags=flags)
        edv.pipeline_sync(0)
        same(acc.download(n), want, ("pipelined", flags))


def test_edge_batch_under_either_table_policy():
    """a child process with the compact, then the large table policy set: the
    edge batch through the latency path and through the batch kernels"""
    from test_gpu_lifecycle import GiB, child
    d = child(r'''
import stage_cases as sc
b = sc.edge_requests()
want = np.array([q["valid"] for q in b["reqs"]], np.uint8)
out["n"] = len(want); out["accepted"] = int(want.sum())
for name, pol in (("compact", edv.TABLES_COMPACT), ("large", edv.TABLES_LARGE)):
    edv.set_table_policy(0, pol)
    for path, limit in (("latency", edv.LATENCY_PATH_DEFAULT), ("batch", 0)):
        edv.set_latency_path(0, limit)
        got = edv.verify_arrays(b["sigs"], b["pks"], b["msgs"], b["off"])
        out[name + "/" + path] = np.nonzero(got != want)[0].tolist()
    out[name] = edv.table_state(0)
''')
    assert d["n"] == 395 and d["accepted"] == 37
    for k in ("compact/latency", "compact/batch", "large/latency", "large/batch"):
        assert d[k] == [], (k, d[k][:10])
    assert d["compact"]["compact_bytes"] > 0 and d["compact"]["large_bytes"] == 0
    assert d["large"]["large_bytes"] > 3 * GiB
