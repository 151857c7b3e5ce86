"""Cases and Python-integer checkers for the seam between the batch path's two
kernels: the per-chunk state edv_prep_kernel writes and edv_main_kernel reads
(ChunkState, edv_kernels.h), and the device tables.  Shared by two backends,
like math_cases.py: `host` is the CPU build of the headers behind the same
state layout (libedv_hostcheck.so: hc_stage_prep, hc_stage_main,
hc_btab_entries_of_bits, hc_comb_entries), `device` is the product's kernels
run by the stage probes of libedv_measure.so (include/edv_measure.h).  The
last section does the same for the latency kernels cut at phase 1's barrier
(the latency probes; there `host` is a reference, see that section).

A checker takes its expected values from hashlib, Python integers, the affine
Edwards arithmetic of math_cases and the oracle's scalarmult_base only, never
from the code under test.  Not a conftest.

Limb bounds of a stored cached entry, from edv_math.h: fe_mul returns RED
limbs; ge_p3_to_cached stores Y+X and Y-X (a sum of two reduced values: 2 x
RED) and Z and 2dT (products: RED).  What the main kernel's additions accept
for an entry is the multiply's input bound, BOUND."""
import ctypes
import functools
import hashlib
import json
import os
import random

import numpy as np

import hostcheck_lib
import math_cases as mc
import oracle_lib as orc
from math_cases import BOUND, D, L, N8L, P, RED

CAP = 4096
SENT = 0xA5
SENT32 = 0xA5A5A5A5
A_WORDS = 360
SET_BITS = {"compact": 16, "large": 22}
SET_TABLES = {"compact": 16, "large": 12}
COMB_ROWS, COMB_ENTRIES = 32, 129
M255 = 2**255 - 1
IDENT = (0, 1)


# ------------------------------------------------------------------ backends
def _hc():
    hc = hostcheck_lib.load()
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    hc.hc_stage_prep.argtypes = [vp, vp, vp, vp, u64, ci, ci, ci, ci, u64, vp, vp, vp, vp, vp, vp]
    hc.hc_stage_main.argtypes = [u64, u64, vp, vp, vp, vp, vp, vp]
    hc.hc_comb_entries.argtypes = [vp, ci, vp]
    return hc


def run_prep(backend, batch, n, table_set="compact", buckets=False, split=False, side0=0, nsides=3):
    """The prep stage over the first n requests of `batch` -> the state it
    wrote (edv.probe_prep_state's dict), every byte pre-filled with SENT."""
    sigs, pks, off = batch["sigs"][:64 * n], batch["pks"][:32 * n], batch["off"][:n + 1]
    msgs = batch["msgs"]
    if backend == "device":
        from indy_plenum_amd import edv
        return edv.probe_prep_state(sigs, pks, msgs, off, table_set, buckets, split, side0, nsides)
    assert backend == "host"
    st = {"dig": np.full((17, CAP), SENT32, np.uint32), "alive": np.full((3, CAP), SENT, np.uint8),
          "atab": np.full((n, A_WORDS), SENT32, np.uint32).view(np.int32),
          "rtab": np.full((n, A_WORDS), SENT32, np.uint32).view(np.int32),
          "perm": np.zeros(n, np.uint32) if buckets else None, "accept": np.full(n, SENT, np.uint8), "cap": CAP}
    sigs, pks, off = np.ascontiguousarray(sigs), np.ascontiguousarray(pks), np.ascontiguousarray(off)
    for s0, ns in (((0, 1), (1, 2)) if split else ((side0, nsides),)):   # the split pipeline's two launches
        rc = _hc().hc_stage_prep(sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, off.ctypes.data, n,
                                 SET_BITS[table_set], s0, ns, int(buckets), CAP, st["dig"].ctypes.data,
                                 st["alive"].ctypes.data, st["atab"].ctypes.data, st["rtab"].ctypes.data,
                                 st["perm"].ctypes.data if buckets else None, st["accept"].ctypes.data)
        assert rc == 0
    return st


def run_main(backend, n, dig, alive, atab, rtab, perm=None, prio=False):
    """The main stage on a state of n slots -> accept (n) uint8, SENT where nothing was written."""
    if backend == "device":
        from indy_plenum_amd import edv
        return edv.probe_main_state(n, dig, alive, atab, rtab, perm, prio)
    assert backend == "host"
    dig, alive = np.ascontiguousarray(dig, np.uint32), np.ascontiguousarray(alive, np.uint8)
    atab, rtab = np.ascontiguousarray(atab, np.int32), np.ascontiguousarray(rtab, np.int32)
    perm = None if perm is None else np.ascontiguousarray(perm, np.uint32)
    accept = np.full(n, SENT, np.uint8)
    assert _hc().hc_stage_main(n, dig.shape[1], dig.ctypes.data, alive.ctypes.data, atab.ctypes.data,
                               rtab.ctypes.data, None if perm is None else perm.ctypes.data,
                               accept.ctypes.data) == 0
    return accept


def read_table(backend, table_set, pairs):
    """Entries (t, j) of a table set ("compact", "large", "comb") -> (n, 32) int32"""
    tj = np.ascontiguousarray(pairs, np.int32).reshape(-1, 2)
    if backend == "device":
        from indy_plenum_amd import edv
        return edv.probe_table(table_set, tj)
    assert backend == "host"
    out = np.zeros((len(tj), 32), np.int32)
    if table_set == "comb":
        assert _hc().hc_comb_entries(tj.ctypes.data, len(tj), out.ctypes.data) == 0
        return out
    for t in sorted(set(tj[:, 0].tolist())):
        idx = np.nonzero(tj[:, 0] == t)[0]
        js = np.ascontiguousarray(tj[idx, 1])
        part = np.zeros((len(js), 32), np.int32)
        assert _hc().hc_btab_entries_of_bits(SET_BITS[table_set], t, js.ctypes.data, len(js), part.ctypes.data) == 0
        out[idx] = part
    return out


# ------------------------------------------------------- points and scalars
def ext(pt):
    return (pt[0], pt[1], 1, pt[0] * pt[1] % P)


def ext_add(p, q):
    """extended twisted Edwards addition (a = -1; complete on edwards25519, doubles too)"""
    a = (p[1] - p[0]) * (q[1] - q[0]) % P
    b = (p[1] + p[0]) * (q[1] + q[0]) % P
    c = 2 * D * p[3] * q[3] % P
    d = 2 * p[2] * q[2] % P
    e, f, g, h = b - a, d - c, d + c, b + a
    return (e * f % P, g * h % P, f * g % P, e * h % P)


def affine_all(pts):
    """extended points -> affine (x, y), one inversion for all (Montgomery's trick)"""
    acc, pre = 1, []
    for p in pts:
        pre.append(acc)
        acc = acc * p[2] % P
    inv, out = pow(acc, P - 2, P), [None] * len(pts)
    for k in range(len(pts) - 1, -1, -1):
        zi = inv * pre[k] % P
        inv = inv * pts[k][2] % P
        out[k] = (pts[k][0] * zi % P, pts[k][1] * zi % P)
    return out


def multiples(pt, n=9):
    """0 .. n-1 times the affine point, affine"""
    e, acc, out = ext(pt), ext(IDENT), []
    for _ in range(n):
        out.append(acc)
        acc = ext_add(acc, e)
    return affine_all(out)


def double_and_add(k, pt):
    """[k]pt for any integer k by plain double-and-add, extended coordinates"""
    if k < 0:
        k, pt = -k, ((P - pt[0]) % P, pt[1])
    e, acc = ext(pt), ext(IDENT)
    for bit in bin(k)[2:]:
        acc = ext_add(acc, acc)
        if bit == "1":
            acc = ext_add(acc, e)
    return acc


def base_mult(k):
    """[k]B, affine, by the oracle's fixed-base multiplication"""
    k %= L
    return mc.ed_decode(orc.scalarmult_base(k.to_bytes(32, "little")))


def neg(pt):
    return ((P - pt[0]) % P, pt[1])


T8 = mc.torsion_points()[4]              # a point of order 8 (libsodium's blocklist y, 26e8958f...)
TORSION = multiples(T8, 8)               # i x T8


def recode4(s):
    """Python mirror of recode_signed<4, 64> (edv_verify_core.h): the 64 signed
    digits of s < 2^253 and their packed words"""
    assert 0 <= s < 2**253
    digits, carry = [], 0
    for k in range(64):
        e = ((s >> (4 * k)) & 15) + carry
        carry = 0 if k == 63 else (e + 8) >> 4
        digits.append(e - 16 * carry)
    packed = sum((d & 15) << (4 * k) for k, d in enumerate(digits))
    return digits, [(packed >> (32 * w)) & 0xFFFFFFFF for w in range(8)]


def windows(digits):
    return max([k + 1 for k, d in enumerate(digits) if d], default=0)


def _vals(words40):
    return [mc.val(words40[10 * c:10 * c + 10]) % P for c in range(4)]


# --------------------------------------------------------------- the checkers
def check_cached_table(words, pts, what):
    """A slot's 360 words are entries e = 0..8 of (Y+X, Y-X, Z, 2dT) for the
    affine points pts[e], by cross-multiplication, within the stored bound"""
    words = [int(w) for w in words]
    for e, (x, y) in enumerate(pts):
        w = words[40 * e:40 * e + 40]
        for c in range(4):
            lim = [2 * b for b in RED] if c < 2 else RED
            assert all(abs(w[10 * c + i]) <= lim[i] for i in range(10)), (what, e, c, "limb bound")
        ypx, ymx, z, t2d = _vals(w)
        assert z != 0, (what, e, "Z = 0")
        assert (ypx - ymx) % P == 2 * x * z % P and (ypx + ymx) % P == 2 * y * z % P, (what, e, "point")
        assert t2d == 2 * D * x * y * z % P, (what, e, "T2d")


def oracle_base_mults(scalars):
    """the encodings of [k]B by the oracle's scalarmult_base for every k, on a
    few threads (the call releases the interpreter lock)"""
    from concurrent.futures import ThreadPoolExecutor
    orc.load()
    enc = lambda ks: [orc.scalarmult_base((k % L).to_bytes(32, "little")) for k in ks]      # noqa: E731
    chunks = [scalars[o:o + 256] for o in range(0, len(scalars), 256)]
    with ThreadPoolExecutor(min(16, os.cpu_count() or 1)) as ex:
        return [e for part in ex.map(enc, chunks) for e in part]


def check_precomp_entry(entry, scalar, what, want=None):
    """A shared-table entry (y+x, y-x, 2dxy limbs) encodes to the oracle's
    [scalar]B (want: that encoding, if the caller has it), and its third
    coordinate is 2d x y"""
    e = [int(v) for v in entry]
    ypx, ymx, xy2d = mc.val(e[0:10]) % P, mc.val(e[10:20]) % P, mc.val(e[20:30]) % P
    inv2 = (P + 1) // 2
    y, x = (ypx + ymx) * inv2 % P, (ypx - ymx) * inv2 % P
    assert xy2d == 2 * D * x * y % P, (what, "xy2d")
    enc = int.to_bytes(y | ((x & 1) << 255), 32, "little")
    assert enc == (want or orc.scalarmult_base((scalar % L).to_bytes(32, "little"))), (what, "point")


def table_pairs(table_set, seed=41):
    """The (t, j) a table test reads: per table the edge entries, the first and
    last 256 and 2,048 random ones; the whole comb"""
    if table_set == "comb":
        return [(i, j) for i in range(COMB_ROWS) for j in range(COMB_ENTRIES)]
    r = random.Random(seed)
    last = 2**(SET_BITS[table_set] - 1)
    pairs = []
    for t in range(SET_TABLES[table_set]):
        js = [0, 1, 2, 3, 127, 128, 255, 256, last - 1, last] + list(range(256)) + list(range(last - 255, last + 1))
        js += [r.randrange(last + 1) for _ in range(2048)]
        pairs += [(t, j) for j in js]
    return pairs


def family_tables(backend, table_set):
    pairs = table_pairs(table_set)
    got = read_table(backend, table_set, pairs)
    shift = 8 if table_set == "comb" else SET_BITS[table_set]
    want = oracle_base_mults([j << (shift * t) for t, j in pairs])
    for (t, j), e, w in zip(pairs, got, want):
        check_precomp_entry(e, j << (shift * t), (table_set, t, j), w)
        assert not e[30:].any(), (table_set, t, j, "padding")
    return len(pairs)


# ------------------------------------------------------------ prep state out
SMALL_Y = {0, 1, P - 1, P, P + 1} | set(mc.ORDER8_Y)   # libsodium's blocklist, sign bit masked
SPECIAL_LENS = [0, 1, 46, 47, 48, 111, 112, 175, 176, 303, 304]
PREP_N = 600
PREP_SIZES = (1, 63, 64, 65, 257, 600)
KINDS = ("S + L", "S high bits", "small-order R", "small-order A", "non-canonical R", "non-canonical A",
         "R off the curve", "A off the curve")


def small_order(b):
    return (int.from_bytes(b, "little") & M255) in SMALL_Y


def canonical(b):
    return (int.from_bytes(b, "little") & M255) < P


def point_of(b):
    """libsodium's decoding: y taken mod p, x with the sign bit's parity; None if not on the curve"""
    v = int.from_bytes(b, "little")
    y, sign = (v & M255) % P, v >> 255
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x = pow(u * pow(w, P - 2, P), (P + 3) // 8, P)
    if (w * x * x - u) % P:
        x = x * mc.SQRTM1 % P
    if (w * x * x - u) % P:
        return None
    return ((P - x) % P if (x & 1) != sign else x, y)


def sha_bucket(mlen):
    return min((64 + mlen + 17 + 127) // 128, 63)


def _bad_encodings():
    """the point encodings the rejected requests use, by kind"""
    small = [y | (s << 255) for y in sorted(SMALL_Y) for s in (0, 1)]
    noncanon = [P + y for y in range(2, 19) if point_of((P + y).to_bytes(32, "little")) is not None]
    noncanon += [v | (1 << 255) for v in noncanon]
    r = random.Random(99)
    off = []
    while len(off) < 8:
        y = r.randrange(2, P)
        if point_of(y.to_bytes(32, "little")) is None:
            off.append(y | (r.getrandbits(1) << 255))
    assert len(noncanon) >= 4
    return {"small": [v.to_bytes(32, "little") for v in small], "noncanon": [v.to_bytes(32, "little") for v in noncanon],
            "off": [v.to_bytes(32, "little") for v in off]}


def reject_slots(n=PREP_N):
    """slot -> kind: every kind at scattered slots, at the last slot of a wave,
    at the last slot of each batch size and of the batch"""
    slots = {}
    k = 0
    for s in list(range(63, n, 64)) + [62, 64, 256] + list(range(5, n - 8, 17)) + list(range(n - 8, n)):
        if s not in slots:
            slots[s] = k % len(KINDS)
            k += 1
    return slots


def expect_request(q):
    """what the checkers compare a request's state against: the three sides'
    predicates, h, and the points of both tables"""
    Rp, Ap = point_of(q["R"]), point_of(q["A"])
    q["sides"] = (int(q["S"] < L and not small_order(q["R"]) and canonical(q["A"]) and not small_order(q["A"])),
                  int(canonical(q["A"]) and not small_order(q["A"]) and Ap is not None),
                  int(canonical(q["R"]) and not small_order(q["R"]) and Rp is not None))
    q["h"] = int.from_bytes(hashlib.sha512(q["R"] + q["A"] + q["msg"]).digest(), "little") % L
    q["atab"] = multiples(neg(Ap)) if q["sides"][1] else None
    # the R side cuts S to 253 bits; B has order L
    q["rtab"] = multiples(mc.ed_add(base_mult(q["S"] % 2**253), neg(Rp))) if q["sides"][2] else None


def pack_requests(reqs):
    """the requests' bytes in the C-ABI layout (64 spare bytes after the last message)"""
    off = np.zeros(len(reqs) + 1, np.uint64)
    off[1:] = np.cumsum([len(q["msg"]) for q in reqs])
    return {"off": off,
            "sigs": np.frombuffer(b"".join(q["R"] + q["S"].to_bytes(32, "little") for q in reqs), np.uint8).copy(),
            "pks": np.frombuffer(b"".join(q["A"] for q in reqs), np.uint8).copy(),
            "msgs": np.frombuffer(b"".join(q["msg"] for q in reqs) + bytes(64), np.uint8).copy()}


@functools.lru_cache(maxsize=None)
def prep_batch():
    """The 600-request batch: valid signatures over messages of the block-edge
    lengths, one of 8,100 bytes and a random spread, and rejected ones of every
    kind; with each request's expected sides, hash and table points"""
    r = random.Random(2024)
    lens = SPECIAL_LENS * 3 + [8100]
    lens += [r.randrange(0, 700) for _ in range(PREP_N - len(lens))]
    r.shuffle(lens)
    keys = [orc.keypair(bytes(r.getrandbits(8) for _ in range(32))) for _ in range(8)]
    bad, slots = _bad_encodings(), reject_slots()
    reqs = []
    for i, ln in enumerate(lens):
        msg = bytes(r.getrandbits(8) for _ in range(ln))
        pk, sk = keys[i % len(keys)]
        sig = orc.sign(msg, sk)
        R, S, A = sig[:32], int.from_bytes(sig[32:], "little"), pk
        kind = slots.get(i)
        if kind == 0:
            S += L
        elif kind == 1:
            S |= 1 << 255
        elif kind in (2, 3):
            R, A = (bad["small"][i % len(bad["small"])], A) if kind == 2 else (R, bad["small"][i % len(bad["small"])])
        elif kind in (4, 5):
            e = bad["noncanon"][i % len(bad["noncanon"])]
            R, A = (e, A) if kind == 4 else (R, e)
        elif kind in (6, 7):
            e = bad["off"][i % len(bad["off"])]
            R, A = (e, A) if kind == 6 else (R, e)
        reqs.append({"R": R, "S": S, "A": A, "msg": msg, "kind": kind})
    off = np.zeros(PREP_N + 1, np.uint64)
    off[1:] = np.cumsum([len(q["msg"]) for q in reqs])
    assert set(int(o) % 16 for o in off[:-1]) == set(range(16))       # message starts cover every offset mod 16
    assert sha_bucket(8100) == 63 and all(sha_bucket(a) + 1 == sha_bucket(a + 1) for a in (47, 175, 303))
    for q in reqs:
        expect_request(q)
        q["valid"] = orc.verify(q["R"] + q["S"].to_bytes(32, "little"), q["msg"], q["A"])
    assert sum(q["valid"] for q in reqs) == PREP_N - len(slots) and all(q["kind"] is None or not q["valid"] for q in reqs)
    return dict(pack_requests(reqs), reqs=reqs, off=off)


def uniform_batch(n=65, mlen=100):
    """n requests that share one length bucket (valid signatures)"""
    r = random.Random(7)
    pk, sk = orc.keypair(bytes(range(32)))
    msgs = [bytes(r.getrandbits(8) for _ in range(mlen)) for _ in range(n)]
    off = np.arange(n + 1, dtype=np.uint64) * np.uint64(mlen)
    return {"sigs": np.frombuffer(b"".join(orc.sign(m, sk) for m in msgs), np.uint8).copy(),
            "pks": np.frombuffer(pk * n, np.uint8).copy(), "off": off,
            "msgs": np.frombuffer(b"".join(msgs) + bytes(64), np.uint8).copy()}


def unpack_dig(st, j):
    """slot j's digit words -> (a, b, digits of a, digits of |b|, count)"""
    w = [int(st["dig"][k, j]) for k in range(17)]
    da, db = mc.signed_digits(w[0:8], 4), mc.signed_digits(w[8:16], 4)
    assert w[16] >> 9 == 0, (j, "stray bits in the count word")
    a, u = sum(d << (4 * k) for k, d in enumerate(da)), sum(d << (4 * k) for k, d in enumerate(db))
    return a, (-u if (w[16] >> 8) & 1 else u), da, db, w[16] & 0xff


def check_prep_state(batch, n, st, buckets):
    """Every word the prep stage wrote for the first n requests of the batch
    against Python; -> the (a, b) pairs by request (None where the hash side
    rejected)"""
    reqs, cap = batch["reqs"][:n], st["cap"]
    assert cap == CAP and st["dig"].shape == (17, cap) and st["alive"].shape == (3, cap)
    if buckets:
        perm = [int(x) for x in st["perm"]]
        assert sorted(perm) == list(range(n)), "perm is not a permutation"
        bk = [sha_bucket(len(reqs[i]["msg"])) for i in perm]
        assert bk == sorted(bk), "buckets decrease along the slots"
        if len(set(bk)) == 1:
            assert perm == list(range(n)), "one bucket: the identity order"
    else:
        perm = list(range(n))
    want_acc = [SENT if all(q["sides"]) else 0 for q in reqs]
    assert st["accept"].tolist() == want_acc, [i for i in range(n) if st["accept"][i] != want_acc[i]][:10]
    # nothing written past the batch
    assert (st["alive"][:, n:] == SENT).all() and (st["dig"][:, n:] == SENT32).all()
    ab = [None] * n
    for j, i in enumerate(perm):
        q = reqs[i]
        assert tuple(int(st["alive"][k, j]) for k in range(3)) == q["sides"], (i, j, q["kind"], "alive")
        if q["sides"][0]:
            a, b, da, db, cnt = unpack_dig(st, j)
            assert 0 <= a < 2**253 and abs(b) < 2**192 and b % 2 == 1, (i, "scalar range")
            assert (a - b * q["h"]) % N8L == 0, (i, "a = b h mod 8L")
            assert da[63] >= 0 and db[63] >= 0 and all(-8 <= d <= 7 for d in da + db), (i, "digit range")
            assert cnt == max(windows(da), windows(db)), (i, "window count", cnt)
            ab[i] = (a, b)
        if q["sides"][1]:
            check_cached_table(st["atab"][j], q["atab"], ("atab", i, j))
        if q["sides"][2]:
            check_cached_table(st["rtab"][j], q["rtab"], ("rtab", i, j))
    return ab


def by_request(st, n):
    """the state's slots reordered by request, as bytes per array (split
    against joint, bucketed against unbucketed)"""
    perm = np.arange(n) if st["perm"] is None else st["perm"].astype(np.int64)
    inv = np.empty(n, np.int64)
    inv[perm] = np.arange(n)
    return {"dig": st["dig"][:, :n][:, inv].tobytes(), "alive": st["alive"][:, :n][:, inv].tobytes(),
            "atab": st["atab"][inv].tobytes(), "rtab": st["rtab"][inv].tobytes(), "accept": st["accept"].tobytes()}


def same_rtab_points(batch, n, st1, st2):
    """two runs' rtab entries are the same points (limbs may differ), by request"""
    r1, r2 = (np.frombuffer(by_request(s, n)["rtab"], np.int32).reshape(n, A_WORDS) for s in (st1, st2))
    for i, q in enumerate(batch["reqs"][:n]):
        if not q["sides"][2]:
            continue
        for e in range(9):
            p1, m1, z1, t1 = _vals(r1[i, 40 * e:40 * e + 40].tolist())
            p2, m2, z2, t2 = _vals(r2[i, 40 * e:40 * e + 40].tolist())
            assert (p1 * z2 - p2 * z1) % P == 0 and (m1 * z2 - m2 * z1) % P == 0 and (t1 * z2 - t2 * z1) % P == 0, (i, e)


def round_trip(backend, batch, n, st, prio=False):
    """the prep stage's state through the main stage -> the verdict per request"""
    acc = run_main(backend, n, st["dig"], st["alive"], st["atab"], st["rtab"], st["perm"], prio)
    return [int(p) if p != SENT else int(m) for p, m in zip(st["accept"], acc)]


# ------------------------------------------------------------ chosen state in
def own_count(a, u):
    return max(windows(recode4(a)[0]), windows(recode4(u)[0]))


def expected_verdict(c):
    sb = -c["u"] if c["neg"] else c["u"]
    return int((c["a"] * c["k"] + sb * c["m"]) % L == 0 and (c["a"] * c["i"] + sb * c["j"]) % 8 == 0)


def _solve(r, a, u, negR, residue=0, k_off=0, m=None):
    """(k, m, i, j) with a k + b m = k_off a (mod L) and a i + b j = residue (mod 8), b = -u if negR else u;
    None where no (i, j) exists"""
    sb = -u if negR else u
    if a % L:
        m = r.randrange(1, L) if m is None else m
        k = (-sb * m * pow(a, L - 2, L) + k_off) % L
    else:
        if k_off:
            return None
        m, k = 0, r.randrange(1, L)       # [a]P1 vanishes on the prime-order part: P2 must have none
    opts = [(i, j) for i in range(8) for j in range(8) if (a * i + sb * j) % 8 == residue and (i or j or residue == 0)]
    if not opts:
        return None
    nz = [o for o in opts if o[0] and o[1]] or opts
    i, j = r.choice(nz)
    return k, m, i, j


def _scalar_with_count(r, c, carry_top=False):
    """a scalar < 2^253 whose recoding needs exactly c windows; carry_top: the
    top window holds only the recode's final carry"""
    for _ in range(1000):
        if carry_top:
            s = (0xF8 << (4 * (c - 3))) | r.getrandbits(4 * (c - 3)) if c >= 3 else None
        else:
            s = (1 << 252) | r.getrandbits(252) if c == 64 else (r.randrange(1, 8) << (4 * (c - 1))) | r.getrandbits(4 * (c - 1))
        if s is not None and s < 2**253 and windows(recode4(s)[0]) == c:
            return s
    raise AssertionError(("no scalar with count", c, carry_top))


def special_scalars():
    """the digit families: edges, all-8 and all-7 nibbles, runs of -8 digits
    (0x77..78), alternating patterns, a carry into the top window"""
    vals = [0, 1, 2, 7, 8, 9, 15, 16, 2**252 + 5, 2**252 + 2**128 + 1, 2**253 - 1, 2**253 - 2**200, 2**192 - 1, 2**192 - 2,
            int("8" * 63, 16), int("8" * 48, 16), int("7" * 63, 16), int("7" * 48, 16), int("1" + "8" * 63, 16),
            int("f" * 63, 16), int("f8" + "0" * 60, 16), int("1f8" + "0" * 59, 16)]
    vals += [int("7" * k + "8", 16) for k in (1, 5, 31, 46, 47, 61, 62)]          # digits all -8, then 1
    vals += [v for v in mc.recoding_values()[:12]]
    vals += [int(pat * 31, 16) for pat in ("87", "78", "08", "80", "9f")]
    return [v for v in vals if 0 <= v < 2**253]


def _case(r, a, u, negR, word=None, mode="affine", residue=0, k_off=0, alive=(1, 1, 1), tag=""):
    sol = _solve(r, a, u, negR, residue, k_off)
    if sol is None:
        return None
    k, m, i, j = sol
    own = own_count(a, u)
    c = {"a": a, "u": u, "neg": negR, "k": k, "m": m, "i": i, "j": j, "word": own if word is None else word,
         "mode": mode, "alive": alive, "tag": tag, "own": own}
    assert own <= c["word"] <= 64
    c["expect"] = expected_verdict(c)
    assert c["expect"] == int(residue == 0 and k_off == 0), c
    return c


def _dead(r):
    """a padding lane some side killed: garbage digits, the largest count"""
    return {"dead": True, "alive": r.choice([(0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)]), "tag": "padding",
            "words": [r.getrandbits(32) for _ in range(16)] + [64 | (r.getrandbits(1) << 8)]}


@functools.lru_cache(maxsize=None)
def chosen_cases():
    """The slots of the injected state, wave by wave (64 slots each; the last
    wave is partial)"""
    r = random.Random(515)
    short = lambda: r.randrange(1, 2**12) | 1                                   # noqa: E731
    waves = []

    def add(cases, pad=True, fill=64):
        cases = [c for c in cases if c is not None]
        for o in range(0, len(cases), fill):
            w = cases[o:o + fill]
            waves.append(w + ([_dead(r) for _ in range(64 - len(w))] if pad else []))

    # window counts 1..64 for a, then for |b|, the other scalar short: accepted and off by one; 32
    # cases and 32 dead lanes per wave, so the waves' maxima are 16, 32, 48, 64
    for which in "ab":
        cs = []
        for c in range(1, 65):
            s = _scalar_with_count(r, c)
            tiny = r.randrange(1, 8) if c <= 3 else short() + (c & 1)      # one window, or three
            a, u = (s, tiny) if which == "a" else (tiny, s)
            cs += [_case(r, a, u, c & 1, tag="count %s %d" % (which, c)),
                   _case(r, a, u, c & 1, k_off=1, tag="count %s %d off by one" % (which, c))]
        inter = []
        for o in range(0, len(cs), 32):
            inter += [x for pair in zip(cs[o:o + 32], [_dead(r) for _ in range(32)]) for x in pair]
        add(inter)
    # one long walk among short ones, at lanes 0, 31, 32, 63: the wave-wide maximum
    for lane in (0, 31, 32, 63):
        w = [_case(r, short(), short(), lane & 1, tag="spike short") for _ in range(64)]
        w[lane] = _case(r, _scalar_with_count(r, 64), short(), 0, tag="spike 64")
        w[(lane + 7) % 64] = _case(r, short(), _scalar_with_count(r, 33), 1, tag="spike 33")
        w[(lane + 9) % 64] = _dead(r)
        add(w)
    # a wave of one-window walks (the longest alignment shift)
    add([_case(r, r.randrange(0, 8), r.randrange(1, 8), r.getrandbits(1), k_off=it % 2, tag="one window")
         for it in range(64)])
    # the count word above the lane's own count
    cs = []
    for it in range(64):
        a, u = _scalar_with_count(r, 1 + it % 20), short()
        own = own_count(a, u)
        cs.append(_case(r, a, u, it & 1, word=r.choice([own + 1, max(own, 33), 64]), k_off=(it % 4 == 3),
                        tag="count word above own"))
    add(cs)
    # digit families, carries into the top window
    cs = []
    for s in special_scalars():
        cs += [_case(r, s, short(), 0, tag="digits a"), _case(r, s, short(), 1, k_off=1, tag="digits a off by one")]
        if s:
            cs += [_case(r, short() * 2, s, 1, tag="digits b"), _case(r, short(), s, 0, k_off=1, tag="digits b off by one")]
    for c in (3, 4, 17, 33, 34, 48, 49, 63, 64):
        s = _scalar_with_count(r, c, carry_top=True)
        cs += [_case(r, s, short(), 0, tag="carry top a"), _case(r, short(), s, 1, tag="carry top b"),
               _case(r, s, short(), 1, k_off=1, tag="carry top a off by one")]
    cs += [_case(r, 0, u, s, tag="a = 0") for u in (1, 3, 2**100 + 1, 2**191 + 1) for s in (0, 1)]
    add(cs)
    # the sign: the same |b| with negR 0 and 1, solved for one of them
    cs = []
    for it in range(32):
        a, u = r.getrandbits(130), r.getrandbits(128) | 1
        c0 = _case(r, a, u, it & 1, tag="sign")
        c1 = dict(c0, neg=1 - c0["neg"], tag="sign flipped")
        c1["expect"] = expected_verdict(c1)
        assert c0["expect"] == 1 and c1["expect"] == 0
        cs += [c0, c1]
    add(cs)
    # small-order results: order 2 (X = 0, Y = -Z), order 4, order 8
    cs = []
    for it in range(96):
        a, u = r.getrandbits(128) | (it & 1), r.getrandbits(127) | 1
        res = (4, 2, 6, 1, 3, 7, 5, 4)[it % 8]
        cs.append(_case(r, a, u, it & 1, residue=res, tag="small-order result %d" % res))
    add(cs)
    # the identity in disguise: entries scaled by their own field elements, limbs at the bound
    cs = []
    for it in range(128):
        a, u = r.getrandbits(120 + it), r.getrandbits(100 + it // 2) | 1
        cs.append(_case(r, a, u, it & 1, mode=("scaled", "bound")[it % 2], k_off=(it % 8 == 7),
                        residue=4 * (it % 8 == 5), tag=("scaled", "bound")[it % 2]))
    add(cs)
    # lanes the main kernel must not touch: each side's byte cleared in turn, on states that would be accepted
    cs = []
    for it in range(64):
        al = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0))[it % 4]
        cs.append(_case(r, r.getrandbits(126), r.getrandbits(126) | 1, it & 1, alive=al, tag="alive %s" % (al,)))
    add(cs)
    # a last, partial wave
    add([_case(r, r.getrandbits(128), r.getrandbits(128) | 1, it & 1, k_off=(it % 3 == 0), tag="tail")
         for it in range(37)], pad=False)
    return [c for w in waves for c in w]


def push_to_bound(l):
    """the same value with every limb moved outwards by one limb width (carried
    into the next limb): magnitudes in [0.5, 1.5] x 2^width, inside BOUND"""
    l = list(l)
    for i in range(10):
        w = 26 if i % 2 == 0 else 25
        s = 1 if l[i] >= 0 else -1
        l[i] += s << w
        if i < 9:
            l[i + 1] -= s
        else:
            l[0] -= 19 * s
    return l


def cached_limbs(r, pt, mode):
    """the 40 words of a cached entry for the affine point: Z = 1 ("affine"), a
    random Z ("scaled"), or Z's limbs at +-BOUND and the others pushed outwards ("bound")"""
    x, y = pt
    if mode == "bound":
        zl = mc.rand_limbs(r, extreme=True)
        z = mc.val(zl) % P
        assert z
    else:
        z = 1 if mode == "affine" else r.randrange(1, P)
        zl = mc.signed_limbs(z)
    coords = [mc.signed_limbs(v) for v in ((y + x) * z % P, (y - x) * z % P, 0, 2 * D * x * y * z % P)]
    if mode == "bound":
        coords = [push_to_bound(c) for c in coords]
    coords[2] = zl
    assert all(abs(v) <= BOUND[i] for c in coords for i, v in enumerate(c))
    assert [mc.val(c) % P for c in coords] == [(y + x) * z % P, (y - x) * z % P, z, 2 * D * x * y * z % P]
    return [v for c in coords for v in c]


@functools.lru_cache(maxsize=None)
def chosen_state():
    """-> (cases, dig (17, cap), alive (3, cap), atab, rtab (n, 360)) with cap = n rounded up to 64"""
    cases = chosen_cases()
    n = len(cases)
    cap = (n + 63) // 64 * 64
    r = random.Random(616)
    dig, alive = np.zeros((17, cap), np.uint32), np.zeros((3, cap), np.uint8)
    atab, rtab = np.zeros((n, A_WORDS), np.int32), np.zeros((n, A_WORDS), np.int32)
    for s, c in enumerate(cases):
        alive[:, s] = c["alive"]
        if c.get("dead"):
            dig[:, s] = c["words"]
            continue
        dig[0:8, s] = recode4(c["a"])[1]
        dig[8:16, s] = recode4(c["u"])[1]
        dig[16, s] = c["word"] | (c["neg"] << 8)
        p1 = mc.ed_add(base_mult(c["k"]), TORSION[c["i"]]) if c["k"] % L else TORSION[c["i"]]
        p2 = mc.ed_add(base_mult(c["m"]), TORSION[c["j"]]) if c["m"] % L else TORSION[c["j"]]
        c["p1"], c["p2"] = p1, p2
        atab[s] = [v for pt in multiples(p1) for v in cached_limbs(r, pt, c["mode"])]
        rtab[s] = [v for pt in multiples(p2) for v in cached_limbs(r, pt, c["mode"])]
    return cases, dig, alive, atab, rtab


def expected_accept(cases, n, perm=None):
    """accept after the main stage: the verdict at the slot's request, SENT for every slot a side killed"""
    want = [SENT] * n
    for s, c in enumerate(cases[:n]):
        if all(c["alive"]):
            want[s if perm is None else int(perm[s])] = c["expect"]
    return want


def check_chosen(backend, n=None, prio=False, permute=False, cap=None):
    """Runs the first n slots of the chosen state through the main stage and
    checks every accept byte; cap: the state's slot stride (default: as built)"""
    cases, dig, alive, atab, rtab = chosen_state()
    n = len(cases) if n is None else n
    if cap is not None:
        dig, alive = np.ascontiguousarray(dig[:, :cap]), np.ascontiguousarray(alive[:, :cap])
    perm = None
    if permute:
        perm = np.array(random.Random(n).sample(range(n), n), np.uint32)
        assert n < 2 or perm.tolist() != list(range(n))
    got = run_main(backend, n, dig, alive, atab[:n], rtab[:n], perm, prio).tolist()
    want = expected_accept(cases, n, perm)
    at = (lambda s: s) if perm is None else (lambda s: int(perm[s]))
    bad = [(s, cases[s]["tag"], got[at(s)], want[at(s)]) for s in range(n) if got[at(s)] != want[at(s)]]
    assert bad == [], bad[:12]
    assert got == want
    return n


def check_construction(count=240):
    """The construction itself: for a spread of the chosen cases, [a]P1 + [b]P2
    by plain double-and-add is the identity exactly when the case expects an
    accept, and the small-order cases land on a point of the order they name"""
    cases = [c for c in chosen_state()[0] if not c.get("dead")]
    step = max(1, len(cases) // count)
    seen = set()
    picked = cases[::step] + [c for c in cases if c["tag"].startswith("small-order")][:24]
    for c in picked:
        sb = -c["u"] if c["neg"] else c["u"]
        q = ext_add(double_and_add(c["a"], c["p1"]), double_and_add(sb, c["p2"]))
        x, y = affine_all([q])[0]
        assert ((x, y) == IDENT) == bool(c["expect"]), c["tag"]
        if c["tag"].startswith("small-order"):
            order = next(o for o in (1, 2, 4, 8) if affine_all([double_and_add(o, (x, y))])[0] == IDENT)
            res = int(c["tag"].split()[-1])
            assert order == {4: 2, 2: 4, 6: 4}.get(res, 8), (c["tag"], order)
            if res == 4:
                assert (x, y) == (0, P - 1)        # X = 0 and Y = -Z: what an X == 0 test alone accepts
            seen.add(order)
    assert seen == {2, 4, 8}
    return len(picked)


# ------------------------------------------------------------ the edge batch
# tests/golden/prep_edge_golden.json (make_prep_edge_golden.py): requests built
# for what the 600 honest requests do not reach in the prep stage and in phase
# 1 of the latency kernels -- edge entries of the [S]B tables, Q = [S]B - R the
# identity or of small order, S in [2^252, L), the cut to 253 bits, 32 keys of
# every kind, accepted signatures whose S has an edge digit -- with libsodium's
# verdicts.  Each request names the property it was built for (`want`);
# check_edge_intent asserts it from the request's bytes before anything runs.
EDGE_GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "prep_edge_golden.json")
EDGE_FAMILIES = ("s_digits", "q_special", "s_canonical", "accepted")
NAMED_S = {"L-1": L - 1, "L-2": L - 2, "2^252-1": 2**252 - 1, "2^252": 2**252, "2^252+1": 2**252 + 1,
           "2^253-1": 2**253 - 1}


def recode_sb(s, table_set):
    """The R side's digits of S, from the comment above add_sb (edv_verify_core.h):
    S is cut to 253 bits; below the top table each digit is the balanced
    remainder mod 2^bits, in [-half, half), least significant first; what is
    left over is the top digit, which so keeps the carry from below"""
    bits, tables = SET_BITS[table_set], SET_TABLES[table_set]
    half, v, digits = 1 << (bits - 1), s % 2**253, []
    for _ in range(tables - 1):
        d = (v + half) % (2 * half) - half
        digits.append(d)
        v = (v - d) >> bits
    digits.append(v)
    check_recoding(s, table_set, digits)
    return digits


def check_recoding(s, table_set, digits):
    bits, tables = SET_BITS[table_set], SET_TABLES[table_set]
    half, cut = 1 << (bits - 1), s % 2**253
    assert len(digits) == tables
    assert sum(d << (bits * t) for t, d in enumerate(digits)) == cut, "the digits do not sum back to the value"
    assert all(-half <= d < half for d in digits[:-1]), "a digit below the top outside [-half, half)"
    low = sum(d << (bits * t) for t, d in enumerate(digits[:-1]))
    field = cut >> (bits * (tables - 1))
    assert digits[-1] == field + (low < 0), "the top digit is its field plus the carry from below"
    assert 0 <= digits[-1] <= half, "the top digit outside its table"


def digit_coverage(batch, table_set):
    """(zero digits, digits of magnitude half) the R side gathers over the batch's requests"""
    half = 1 << (SET_BITS[table_set] - 1)
    ds = [d for q in batch["reqs"] if q["sides"][2] for d in recode_sb(q["S"], table_set)]
    return sum(1 for d in ds if d == 0), sum(1 for d in ds if abs(d) == half)


def sqrt_branch(enc):
    """Which square root ge_frombytes_negate (edv_math.h) takes for an encoding:
    with x = u v^3 (u v^7)^((p-5)/8), 0 if v x^2 = u, 1 if v x^2 = -u (x is then
    multiplied by sqrt(-1)), None if neither (no point)"""
    y = (int.from_bytes(enc, "little") & M255) % P
    u, v = (y * y - 1) % P, (D * y * y + 1) % P
    x = u * pow(v, 3, P) * pow(u * pow(v, 7, P), (P - 5) // 8, P) % P
    return 0 if (v * x * x - u) % P == 0 else 1 if (v * x * x + u) % P == 0 else None


def has_torsion(pt):
    """[L]pt is not the identity: the point has a component of small order"""
    return affine_all([double_and_add(L, pt)])[0] != IDENT


def order_of(pt):
    """the order of a point of the torsion subgroup"""
    for o in (1, 2, 4, 8):
        if pt == IDENT:
            return o
        pt = mc.ed_add(pt, pt)
    raise AssertionError("not a torsion point")


def check_edge_intent(q):
    """The property the request was built for holds, from its bytes: the digits
    by recode_sb, ranges and named values by Python integers, Q by affine arithmetic"""
    w, S, what = q["want"], q["S"], q["kind"]
    assert q["family"] in EDGE_FAMILIES, what
    if "digits" in w:
        digits = recode_sb(S, w["set"])
        for t, d in w["digits"].items():
            assert digits[int(t)] == d, (what, "digit", t, digits[int(t)], d)
        if "others" in w:
            assert all(d == w["others"] for t, d in enumerate(digits) if str(t) not in w["digits"]), (what, "other digits")
    if "value" in w:
        assert S == NAMED_S[w["value"]], (what, "value")
        if w["value"] == "2^253-1":               # every top digit at its maximum
            assert all(recode_sb(S, ts)[-1] == 2**253 >> (SET_BITS[ts] * (SET_TABLES[ts] - 1)) for ts in SET_BITS), what
    if "random" in w:
        assert S < L, what
    if "lt_l" in w:
        assert (S < L) == bool(w["lt_l"]) and q["valid"] == 0, (what, "S < L")
    if "ge_2_252" in w:
        assert (S >= 2**252) == bool(w["ge_2_252"]), (what, "S >= 2^252")
    if "r_mixed" in w:
        assert has_torsion(point_of(q["R"])) == bool(w["r_mixed"]), (what, "R's order")
    if "q_order" in w or "q" in w:
        assert S % 2**253 != 0, what
        Q = mc.ed_add(base_mult(S % 2**253), neg(point_of(q["R"])))
        if "q_order" in w:
            assert order_of(Q) == w["q_order"], (what, "Q's order")
        else:
            sb = base_mult(S % 2**253)
            assert w["q"] == "2sb" and Q == mc.ed_add(sb, sb) and Q != IDENT, (what, "Q = 2 [S]B")
    if "a_mixed" in w:
        h = int.from_bytes(hashlib.sha512(q["R"] + q["A"] + q["msg"]).digest(), "little") % L
        assert has_torsion(point_of(q["A"])) and h % 8 == 0, (what, "mixed-order A with 8 | h")
    if q["family"] == "accepted":
        assert q["valid"] == 1 and S < L, (what, "accepted")
    elif q["family"] in ("s_digits", "s_canonical"):
        assert q["valid"] == 0, (what, "verdict")
    assert 0 <= len(q["msg"]) <= 90, (what, "message length")


def check_edge_layout(reqs):
    """the order the fixture promises, and the keys of the s_digits family"""
    fam = [q["family"] for q in reqs]
    assert set(fam[:64]) == set(EDGE_FAMILIES), "a family missing from the first wave"
    assert fam[62] == "q_special" and reqs[62]["want"].get("q_order") == 1, "slot 62: Q the identity"
    assert fam[63] == "accepted", "slot 63: an accepted case"
    assert fam[-1] == "s_canonical" and reqs[-1]["S"] >= L, "the last request: S >= L"
    keys = sorted({q["A"] for q in reqs if q["family"] == "s_digits"})
    assert len(keys) >= 32, "fewer than 32 distinct keys"
    B = base_mult(1)
    assert mc.ed_encode(B) in keys and mc.ed_encode(neg(B)) in keys, "B or -B missing"
    for mixed in (False, True):
        grp = [k for k in keys if has_torsion(point_of(k)) == mixed]
        assert {point_of(k)[0] & 1 for k in grp} == {0, 1}, (mixed, "x parity")
        assert {sqrt_branch(k) for k in grp} == {0, 1}, (mixed, "square-root branch")
    for ts in SET_BITS:                      # every table's entry 0 and last entry, on an R side that runs
        half = 1 << (SET_BITS[ts] - 1)
        seen = {(t, abs(d)) for q in reqs for t, d in enumerate(recode_sb(q["S"], ts)) if abs(d) in (0, half)}
        assert {(t, 0) for t in range(SET_TABLES[ts])} <= seen, (ts, "a zero digit missing")
        assert {(t, half) for t in range(SET_TABLES[ts] - 1)} <= seen, (ts, "an edge digit missing")
    acc = [q for q in reqs if q["family"] == "accepted"]
    for ts, ts_t in (("compact", range(16)), ("large", (0, 5, 10))):
        for d in (0, -(1 << (SET_BITS[ts] - 1))):
            have = {int(t) for q in acc if q["want"]["set"] == ts for t, x in q["want"]["digits"].items() if x == d}
            assert have >= set(t for t in ts_t if d == 0 or t < SET_TABLES[ts] - 1), (ts, d, "accepted digits")
    assert sum(1 for q in acc if "a_mixed" in q["want"]) >= 4


def edge_sha256(requests):
    """the hash the fixture records of its own request list"""
    return hashlib.sha256(json.dumps(requests, sort_keys=True, separators=(",", ":")).encode()).hexdigest()


@functools.lru_cache(maxsize=None)
def edge_requests():
    """The fixture's requests and their bytes in the C-ABI layout, each with its
    family, its intent and libsodium's verdict (`valid`); no expected state yet"""
    with open(EDGE_GOLDEN) as f:
        doc = json.load(f)
    assert doc["sha256"] == edge_sha256(doc["requests"]) and doc["count"] == len(doc["requests"])
    reqs = [{"R": bytes.fromhex(c["R"]), "S": int.from_bytes(bytes.fromhex(c["S"]), "little"), "A": bytes.fromhex(c["A"]),
             "msg": bytes.fromhex(c["msg"]), "family": c["family"], "kind": "%s: %s" % (c["family"], c["tag"]),
             "want": c["want"], "valid": int(c["verdict"])} for c in doc["requests"]]
    assert sum(q["valid"] for q in reqs) == doc["accepted"]
    return dict(pack_requests(reqs), reqs=reqs)


@functools.lru_cache(maxsize=None)
def edge_batch():
    """The fixture in prep_batch()'s shape: every request's intent asserted,
    then its expected sides, hash and table points"""
    b = edge_requests()
    reqs = [dict(q) for q in b["reqs"]]
    for q in reqs:
        check_edge_intent(q)
    check_edge_layout(reqs)
    for q in reqs:
        expect_request(q)
        assert q["family"] != "s_canonical" or q["sides"][0] == int(q["S"] < L), (q["kind"], "the hash side's bit")
        assert q["family"] != "accepted" or q["sides"] == (1, 1, 1), q["kind"]
    return dict(b, reqs=reqs)


BATCHES = {"prep": prep_batch, "edge": edge_batch}


def batch_size(name):
    return len(BATCHES[name]()["reqs"])


# ------------------------------------------------------------------ families
VARIANTS =[(ts, bk, sp) for ts in ("compact", "large") for bk in (False, True) for sp in (False, True)]


@functools.lru_cache(maxsize=None)
def _prep_state(backend, n, table_set, buckets, split, batch):
    return run_prep(backend, BATCHES[batch](), n, table_set, buckets, split)


def prep_state(backend, n, table_set, buckets, split, batch="prep"):
    """the prep stage's state for the first n requests of a batch of BATCHES (run once per variant)"""
    return _prep_state(backend, n, table_set, buckets, split, batch)


def family_prep(backend, table_set, buckets, split, n=None, batch="prep"):
    n = batch_size(batch) if n is None else n
    return check_prep_state(BATCHES[batch](), n, prep_state(backend, n, table_set, buckets, split, batch), buckets)


def family_prep_sizes(backend, n, batch="prep"):
    """a batch size that fills no whole workgroup (or wave), bucketed joint on
    the compact set and unbucketed split on the large one"""
    family_prep(backend, "compact", True, False, n, batch)
    family_prep(backend, "large", False, True, n, batch)


def family_seams(backend, table_set, n=None, batch="prep"):
    """split against joint and bucketed against unbucketed: the same state, byte for byte, by request"""
    n = batch_size(batch) if n is None else n
    ref = by_request(prep_state(backend, n, table_set, False, False, batch), n)
    for bk, sp in ((False, True), (True, False), (True, True)):
        got = by_request(prep_state(backend, n, table_set, bk, sp, batch), n)
        for k in ref:
            assert got[k] == ref[k], (table_set, "buckets" if bk else "", "split" if sp else "", k)


def family_sets(backend, n=None, batch="prep"):
    """the large set and the compact set give the same [S]B - R table points"""
    n = batch_size(batch) if n is None else n
    same_rtab_points(BATCHES[batch](), n, prep_state(backend, n, "compact", False, False, batch),
                     prep_state(backend, n, "large", False, False, batch))


def family_one_bucket(backend):
    b = uniform_batch()
    n = len(b["off"]) - 1
    st = run_prep(backend, b, n, "compact", True, False)
    assert st["perm"].tolist() == list(range(n))
    assert (st["alive"][:, :n] == 1).all() and (st["accept"] == SENT).all()
    acc = run_main(backend, n, st["dig"], st["alive"], st["atab"], st["rtab"], st["perm"])
    assert (acc == 1).all()


def family_round_trip(backend, table_set="compact", buckets=True, split=False, prio=False, batch="prep"):
    """prep state -> main stage: the verdicts the batch records for its requests
    (the oracle's for the 600, libsodium's for the edge batch)"""
    b, n = BATCHES[batch](), batch_size(batch)
    got = round_trip(backend, b, n, prep_state(backend, n, table_set, buckets, split, batch), prio)
    assert got == [int(q["valid"]) for q in b["reqs"]]
    return got


# ====================================================== the latency kernels
# edv_quad.hip's kernels cut at the barrier after their phase 1 (the latency
# probes of include/edv_measure.h): what phase 1 leaves in LDS read back, and
# the walks (rtl_walk, quad_walk) run on chosen phase-1 states.  `device` is the
# probe kernels of libedv_measure.so, which instantiate the product kernels'
# own header functions; `host` is a CPU reference (hc_stage_latency_phase1 /
# _walk: the one-lane header functions and plain signed-digit double-and-add),
# there to prove the cases and checkers, not a build of the code under test.
#
# A phase-1 state of `slots` slots (n rounded up to the workgroup's 16 or 32):
# dig (17, slots), pt (3, 40, slots): -A, -R, [S]B in extended coordinates
# (X | Y | Z | T, 10 limbs each), ok (3, slots).  Limb bound: every coordinate
# phase 1 stores is a product (ge_frombytes_negate's X, Y and T = X Y, with Z =
# 1; add_sb's result through ge_p1p1_to_p3) or the negation of one, and
# edv_math.h states fe_mul's output bound as RED; the quad formulas are proved
# for operands inside RED (math_cases.family_quad_points / quad_bounds).
LAT_NS = {"rtl": 16, "quad": 32}      # slots per workgroup
LAT_UNIT = {"rtl": 16, "quad": 8}     # slots that share a window count: the workgroup, or a wave's 8 signatures
LAT_MIN_LIVE = 16                     # kQMinLive
LAT_P1_SIZES = (1, 15, 16, 17, 33, PREP_N)
LAT_WALK_SIZES = (1, 3, 15, 16, 17, 31, 32, 33)


def lat_slots(kernel, n):
    ns = LAT_NS[kernel]
    return (n + ns - 1) // ns * ns


def _hc_lat():
    hc = hostcheck_lib.load()
    vp, u64, ci = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_int
    hc.hc_stage_latency_phase1.argtypes = [vp, vp, vp, vp, u64, ci, ci, vp, vp, vp]
    hc.hc_stage_latency_walk.argtypes = [u64, ci, vp, vp, vp, vp]
    return hc


def run_lat_phase1(backend, kernel, batch, n, table_set="compact"):
    """phase 1 over the first n requests of `batch` -> dig, pt, ok by slot, accept (n), slots"""
    sigs, pks, off = batch["sigs"][:64 * n], batch["pks"][:32 * n], batch["off"][:n + 1]
    msgs = batch["msgs"]
    if backend == "device":
        from indy_plenum_amd import edv
        return edv.probe_latency_phase1(kernel, sigs, pks, msgs, off, table_set)
    assert backend == "host"
    slots = lat_slots(kernel, n)
    st = {"dig": np.full((17, slots), SENT32, np.uint32), "pt": np.full((3, 40, slots), SENT32, np.uint32).view(np.int32),
          "ok": np.full((3, slots), SENT, np.uint8), "accept": np.full(n, SENT, np.uint8), "slots": slots}
    sigs, pks, off = np.ascontiguousarray(sigs), np.ascontiguousarray(pks), np.ascontiguousarray(off)
    assert _hc_lat().hc_stage_latency_phase1(sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, off.ctypes.data, n,
                                             LAT_NS[kernel], SET_BITS[table_set], st["dig"].ctypes.data,
                                             st["pt"].ctypes.data, st["ok"].ctypes.data) == 0
    return st


def run_lat_walk(backend, kernel, n, dig, pt, ok):
    """the walk on a phase-1 state -> accept (slots) uint8, SENT where nothing was written"""
    if backend == "device":
        from indy_plenum_amd import edv
        return edv.probe_latency_walk(kernel, n, dig, pt, ok)
    assert backend == "host"
    slots = lat_slots(kernel, n)
    dig, pt = np.ascontiguousarray(dig, np.uint32), np.ascontiguousarray(pt, np.int32)
    ok = np.ascontiguousarray(ok, np.uint8)
    assert dig.shape == (17, slots) and pt.shape == (3, 40, slots) and ok.shape == (3, slots)
    accept = np.full(slots, SENT, np.uint8)
    assert _hc_lat().hc_stage_latency_walk(n, LAT_NS[kernel], dig.ctypes.data, pt.ctypes.data, ok.ctypes.data,
                                           accept.ctypes.data) == 0
    return accept


# ------------------------------------------------------------- walk in: cases
def push_to_red(l):
    """the same value with every limb that can cross to the opposite sign inside
    RED moved there (one limb width, carried into the next limb): limbs at the
    outer edge of what phase 1 can emit"""
    l = list(l)
    for i in range(9):
        w = 26 if i % 2 == 0 else 25
        edge = (1 << (w - 1)) - (1 << 20) + 2
        if abs(l[i]) >= edge:
            s = 1 if l[i] > 0 else -1
            l[i] -= s << w
            l[i + 1] += s
    return l


def ext_limbs(r, pt, mode):
    """the 40 words X | Y | Z | T (T = X Y / Z) of the affine point: Z = 1
    ("affine"), a random Z ("scaled"), or Z's limbs at +-RED and the other
    coordinates' limbs pushed outwards where they can be ("bound"); every limb
    inside RED, the bound of what phase 1 stores"""
    x, y = pt
    if mode == "bound":
        zl = mc.red_limbs(r, extreme=True)
        z = mc.val(zl) % P
        assert z
    else:
        z = 1 if mode == "affine" else r.randrange(1, P)
        zl = mc.signed_limbs(z)
    want = [x * z % P, y * z % P, z, x * y * z % P]
    coords = [mc.signed_limbs(v) for v in want]
    if mode == "bound":
        coords = [push_to_red(c) for c in coords]
    coords[2] = zl
    assert all(abs(v) <= RED[i] for c in coords for i, v in enumerate(c)), "a limb outside what phase 1 can emit"
    assert [mc.val(c) % P for c in coords] == want
    return [v for c in coords for v in c]


def _digits_value(digits):
    return sum(d << (4 * k) for k, d in enumerate(digits))


def one_bucket_scalars():
    """(bucket, digit sign, scalar): scalars whose signed digits all have the
    magnitude `bucket` (a run of negative digits needs one positive digit on top:
    the same magnitude, or for -8 the 1 of 0x77..78); bucket 0 is the scalar 0"""
    out = [(0, 1, 0)]
    for d in range(1, 9):
        if d < 8:
            out.append((d, 1, _digits_value([d] * 40)))
            out.append((d, -1, _digits_value([-d] * 40 + [d])))
        else:
            out.append((8, -1, int("7" * 62 + "8", 16)))            # 63 digits of -8, then 1
            out.append((8, -1, int("7" * 20 + "8", 16)))
    for d, sign, s in out:
        dg = recode4(s)[0]
        body = dg[:windows(dg) - (1 if sign < 0 else 0)]           # below the positive digit on top of a negative run
        assert all(x == sign * d for x in body) and len(body) >= 21 * bool(s), (d, sign, hex(s))
        assert {abs(x) for x in dg[:windows(dg)]} <= ({d} if d < 8 else {8, 1}), (d, sign, hex(s))
    return out


EVERY_BUCKET = _digits_value([1, -2, 3, -4, 5, -6, 7, -8, 0, 8 - 16, 6, -5, 4, -3, 2, -1, 0, 1])


def _twin_case(r, a, u, negR):
    """[b]P2 = [a]P1 + T with T = (0, -1), the point of order 2: b m = a k (mod L) and b j - a i = 4 (mod 8)"""
    sb = -u if negR else u
    k = r.randrange(1, L)
    m = a * k * pow(sb, L - 2, L) % L
    i = r.randrange(8)
    j = next(j for j in range(8) if (sb * j - a * i) % 8 == 4)
    own = own_count(a, u)
    c = {"a": a, "u": u, "neg": negR, "k": k, "m": m, "i": i, "j": j, "word": own, "mode": "affine", "alive": (1, 1, 1),
         "tag": "x twin", "own": own}
    c["expect"] = expected_verdict(c)
    assert c["expect"] == 0
    return c


class _Tally:
    """requested and dropped cases per family (a case whose congruences have no solution is dropped)"""
    def __init__(self):
        self.asked, self.dropped = {}, {}

    def __call__(self, family, cases):
        self.asked[family] = self.asked.get(family, 0) + len(cases)
        self.dropped[family] = self.dropped.get(family, 0) + sum(1 for c in cases if c is None)
        out = [c for c in cases if c is not None]
        for c in out:
            c["family"] = family
        return out


@functools.lru_cache(maxsize=None)
def lat_cases(kernel):
    """-> (slots, tally): the slots of the chosen phase-1 state of one latency
    kernel, grouped by the unit that shares a window count (16: the right-to-left
    kernel's workgroup, 8: a wave's signatures in the two-walk kernel); the last
    workgroup is partial"""
    U, ns = LAT_UNIT[kernel], LAT_NS[kernel]
    r = random.Random(1717 + U)
    short = lambda: r.randrange(1, 2**12) | 1                                   # noqa: E731
    tally, units = _Tally(), []

    def add(family, cases, fill=U):
        cases = tally(family, cases)
        for o in range(0, len(cases), fill):
            w = cases[o:o + fill]
            units.append(w + [_dead(r) for _ in range(U - len(w))])

    # every window count 1..64 for a and for |b|, accepted and off by one; half a unit of cases, half dead
    for which in "ab":
        cs = []
        for c in range(1, 65):
            s = _scalar_with_count(r, c)
            tiny = r.randrange(1, 8) if c <= 3 else short() + (c & 1)
            a, u = (s, tiny) if which == "a" else (tiny, s)
            cs += [_case(r, a, u, c & 1, tag="count %s %d" % (which, c)),
                   _case(r, a, u, c & 1, k_off=1, tag="count %s %d off by one" % (which, c))]
        add("count " + which, cs, fill=U // 2)
    # one long walk among short ones, at the first and the last slot of the unit
    for pos in (0, U - 1):
        w = [_case(r, short(), short(), k & 1, k_off=(k % 5 == 4), tag="spike short") for k in range(U)]
        w[pos] = _case(r, _scalar_with_count(r, 64), short(), 0, tag="spike 64")
        w[(pos + 3) % U] = _case(r, short(), _scalar_with_count(r, 33), 1, tag="spike 33")
        w[(pos + 5) % U] = _case(r, short(), short(), 1, alive=(1, 1, 0), tag="spike dead")
        add("spike", w)
    # the count word above the slot's own count
    cs = []
    for it in range(32):
        a, u = _scalar_with_count(r, 1 + it % 20), short()
        own = own_count(a, u)
        cs.append(_case(r, a, u, it & 1, word=(own + 1, max(own, 33), 64)[it % 3], k_off=(it % 4 == 3),
                        tag="count word above own"))
    add("word above own", cs)
    # digit families on a and on |b|, accepted and off by one
    cs = []
    for s in special_scalars():
        cs += [_case(r, s, short(), 0, tag="digits a")]
        if s:
            cs += [_case(r, s, short(), 1, k_off=1, tag="digits a off by one"),
                   _case(r, short() * 2, s, 1, tag="digits b"), _case(r, short(), s, 0, k_off=1, tag="digits b off by one")]
    add("special scalars", cs)
    cs = []
    for c in (3, 4, 17, 33, 34, 48, 49, 63, 64):
        s = _scalar_with_count(r, c, carry_top=True)
        cs += [_case(r, s, short(), 0, tag="carry top a"), _case(r, short(), s, 1, tag="carry top b"),
               _case(r, s, short(), 1, k_off=1, tag="carry top a off by one")]
    add("carry top", cs)
    add("a = 0", [_case(r, 0, u, s, tag="a = 0") for u in (1, 3, 2**100 + 1, 2**191 + 1) for s in (0, 1)])
    # both signs of the same |b|, solved for one of them
    cs = []
    for it in range(16):
        a, u = r.getrandbits(130), r.getrandbits(128) | 1
        c0 = _case(r, a, u, it & 1, tag="sign")
        c1 = dict(c0, neg=1 - c0["neg"], tag="sign flipped")
        c1["expect"] = expected_verdict(c1)
        assert c0["expect"] == 1 and c1["expect"] == 0
        cs += [c0, c1]
    add("sign", cs)
    # results of order 2 (X = 0, Y = -Z), 4 and 8
    cs = []
    for it in range(48):
        a, u = r.getrandbits(128) | (it & 1), r.getrandbits(127) | 1
        res = (4, 2, 6, 1, 3, 7, 5, 4)[it % 8]
        cs.append(_case(r, a, u, it & 1, residue=res, tag="small-order result %d" % res))
    add("small-order result", cs)
    # [b]P2 = [a]P1 + (0, -1): the two results have X_a = -X_b as an accepted pair has, and Y_a = -Y_b;
    # only the final check's Y condition rejects it
    add("x twin", [_twin_case(r, r.getrandbits(120 + it) | 1, r.getrandbits(100 + it) | 1, it & 1) for it in range(8)])
    # each ok byte cleared in turn on states that would be accepted, the digits left in place
    cs = []
    for it in range(2 * U):
        al = ((1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0))[it % 4]
        cs.append(_case(r, r.getrandbits(126), r.getrandbits(126) | 1, it & 1, alive=al, tag="ok %s" % (al,)))
    add("ok cleared", cs)
    if kernel == "rtl":
        # workgroup maxima: the ring's wrap, the running-sum phase from every nwin % kRing
        for top in (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64):
            if top == 0:
                units.append([dict(_dead(r), family="maximum 0") for _ in range(U)])
                tally("maximum 0", units[-1])
                continue
            cs = []
            for k in range(U - 2):
                c = top if k % 4 == 0 else r.randrange(1, top + 1)
                a, u = _scalar_with_count(r, c), (r.randrange(1, 8) if top < 4 else _scalar_with_count(r, min(c, 3))) | 1
                if k % 2:
                    a, u = (u, a | 1) if own_count(u, a | 1) <= top else (a, u)
                cs.append(_case(r, a, u, k & 1, k_off=(k % 3 == 2), tag="maximum %d" % top))
            assert max(c["word"] for c in cs) == top, top
            add("maximum %d" % top, cs)
        # all digits in one bucket, each bucket and digit sign, on a and on |b|, both signs of b
        cs = []
        for d, sign, s in one_bucket_scalars():
            cs += [_case(r, s, short(), 0, tag="bucket %d a" % d), _case(r, s, 1, 1, k_off=(s != 0), tag="bucket %d a x" % d)]
            if s & 1:
                cs += [_case(r, short(), s, ng, k_off=ng, tag="bucket %d b" % d) for ng in (0, 1)]
                cs += [_case(r, 1, s, ng, tag="bucket %d b 1" % d) for ng in (0, 1)]
        cs += [_case(r, EVERY_BUCKET, short(), 0, tag="every bucket a"), _case(r, short(), EVERY_BUCKET, 1, tag="every bucket b"),
               _case(r, EVERY_BUCKET, EVERY_BUCKET, 0, k_off=1, tag="every bucket off by one")]
        add("buckets", cs, fill=U // 2)
    else:
        # the four waves of one workgroup with maxima 1, 16, 33 and 64 at once
        while len(units) % (ns // U):
            units.append([_dead(r) for _ in range(U)])
        for top in (1, 16, 33, 64):
            cs = [_case(r, r.randrange(1, 8), r.randrange(1, 8) | 1, k & 1, k_off=k & 1, tag="waves %d" % top) if top == 1 else
                  _case(r, _scalar_with_count(r, top if k == 3 else r.randrange(1, top + 1)), short(), k & 1,
                        k_off=(k % 3 == 0), tag="waves %d" % top) for k in range(U)]
            assert max(c["word"] for c in cs) == top
            add("waves", cs)
    # a partial last workgroup
    while len(units) % (ns // U):
        units.append([_dead(r) for _ in range(U)])
    tail = tally("tail", [_case(r, r.getrandbits(128), r.getrandbits(128) | 1, it & 1, k_off=(it % 3 == 0), tag="tail")
                          for it in range(5)])
    slots = [c for w in units for c in w] + tail
    # the cap on dropped cases: a condition on the builder, not a measurement
    asked, dropped = sum(tally.asked.values()), sum(tally.dropped.values())
    assert dropped * 50 <= asked, (dropped, asked)
    assert tally.dropped["count a"] == 0 and tally.dropped["count b"] == 0
    want = {"count a", "count b", "spike", "word above own", "special scalars", "carry top", "a = 0", "sign",
            "small-order result", "x twin", "ok cleared", "tail"}
    want |= ({"buckets"} | {"maximum %d" % t for t in (0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64)}) if kernel == "rtl" else {"waves"}
    have = {c.get("family") for c in slots}
    assert want <= have, want - have
    return slots, tally


def _x_point(r, torsion):
    pt = base_mult(r.randrange(1, L))
    return mc.ed_add(pt, TORSION[r.randrange(1, 8)]) if torsion else pt


def lat_state_of(cases, kernel, seed=919):
    """the phase-1 state of the slots `cases`, padded to whole workgroups with
    live-looking accepted states: pt[0] = P1, pt[2] = X = [s]B (half the slots
    with a torsion component), pt[1] = P2 - X, so the kernel's own [S]B + (-R) is
    P2; the three point forms in turn.  A dead slot: garbage digits, count 64,
    arbitrary limbs inside the bound."""
    r = random.Random(seed)
    cases = list(cases)
    while len(cases) % LAT_NS[kernel]:
        cases.append(_case(r, r.getrandbits(100), r.getrandbits(100) | 1, len(cases) & 1, tag="past the batch"))
    slots = len(cases)
    dig, ok = np.zeros((17, slots), np.uint32), np.zeros((3, slots), np.uint8)
    pt = np.zeros((3, 40, slots), np.int32)
    for s, c in enumerate(cases):
        ok[:, s] = c["alive"]
        if c.get("dead"):
            dig[:, s] = c["words"]
            pt[:, :, s] = [[v for _ in range(4) for v in mc.red_limbs(r)] for _ in range(3)]
            continue
        dig[0:8, s] = recode4(c["a"])[1]
        dig[8:16, s] = recode4(c["u"])[1]
        dig[16, s] = c["word"] | (c["neg"] << 8)
        p1 = mc.ed_add(base_mult(c["k"]), TORSION[c["i"]]) if c["k"] % L else TORSION[c["i"]]
        p2 = mc.ed_add(base_mult(c["m"]), TORSION[c["j"]]) if c["m"] % L else TORSION[c["j"]]
        x = _x_point(r, s & 1)
        c["p1"], c["p2"], c["x"], c["mr"] = p1, p2, x, mc.ed_add(p2, neg(x))
        mode = ("affine", "scaled", "bound")[s % 3]
        pt[0, :, s], pt[1, :, s], pt[2, :, s] = ext_limbs(r, p1, mode), ext_limbs(r, c["mr"], mode), ext_limbs(r, x, mode)
    return cases, dig, pt, ok


@functools.lru_cache(maxsize=None)
def lat_state(kernel):
    slots, _ = lat_cases(kernel)
    return (len(slots),) + lat_state_of(slots, kernel)


def lat_expected(cases, n, slots):
    """accept after the walk: 0 for a slot below n with an ok byte cleared, its verdict otherwise; SENT from n on"""
    return [(c["expect"] if all(c["alive"]) else 0) if s < n else SENT for s, c in enumerate(cases[:slots])]


def check_lat_accept(kernel, cases, n, got):
    slots = lat_slots(kernel, n)
    got, want = [int(v) for v in got], lat_expected(cases, n, slots)
    assert len(got) == slots
    bad = [(s, cases[s]["tag"], got[s], want[s]) for s in range(slots) if got[s] != want[s]]
    assert bad == [], (kernel, n, bad[:12])


def check_lat_walk(backend, kernel):
    """the whole chosen state of the kernel through its walk, every accept byte checked"""
    n, cases, dig, pt, ok = lat_state(kernel)
    check_lat_accept(kernel, cases, n, run_lat_walk(backend, kernel, n, dig, pt, ok))
    return n


@functools.lru_cache(maxsize=None)
def _lat_plain(kernel):
    """64 plain slots for the batch sizes: accepted, rejected, one ok byte cleared"""
    r = random.Random(2323)
    cs = []
    for it in range(64):
        al = (1, 1, 1) if it % 7 != 5 else ((0, 1, 1), (1, 0, 1), (1, 1, 0))[it % 3]
        cs.append(_case(r, r.getrandbits(40 + 3 * it), r.getrandbits(30 + 2 * it) | 1, it & 1, k_off=(it % 3 == 1), alive=al,
                        tag="plain"))
    return cs


def check_lat_sizes(backend, kernel, n):
    """A batch of n slots in whole workgroups.  Below kQMinLive the padding slots
    n .. 15 are worked: they carry a live state with count 64 that would be
    accepted, and in a second run one that would be rejected; neither may change
    a verdict below n, and nothing is written from n on."""
    r = random.Random(31 * n)
    slots = lat_slots(kernel, n)
    base = _lat_plain(kernel)[:slots]
    runs = []
    for k_off in ((0, 1) if n < LAT_MIN_LIVE else (0,)):
        cs = list(base)
        for s in range(n, min(slots, LAT_MIN_LIVE)):
            cs[s] = _case(r, _scalar_with_count(r, 64), r.getrandbits(60) | 1, s & 1, k_off=k_off, tag="padding %d" % k_off)
        cases, dig, pt, ok = lat_state_of(cs, kernel, seed=n)
        got = run_lat_walk(backend, kernel, n, dig, pt, ok)
        check_lat_accept(kernel, cases, n, got)
        runs.append(got.tolist())
    assert all(g == runs[0] for g in runs)


def check_lat_construction(kernel, count=120):
    """The construction itself: for a spread of the slots, the injected -R and
    [S]B add up to P2 and [a]P1 + [b]P2 by plain double-and-add is the identity
    exactly when the case expects an accept; the small-order cases land on a
    point of the order they name.  Read back from the limbs that are injected."""
    n, cases, dig, pt, ok = lat_state(kernel)
    live = [s for s, c in enumerate(cases) if not c.get("dead")]
    picked = live[::max(1, len(live) // count)] + [s for s in live if cases[s]["tag"].startswith("small-order")][:16]
    picked += [s for s in live if cases[s]["tag"] == "x twin"]
    seen = set()
    for s in picked:
        c = cases[s]
        p1, mr, x = (mc.affine([[int(v) for v in pt[k, 10 * q:10 * q + 10, s]] for q in range(4)]) for k in range(3))
        assert p1 == c["p1"] and mc.ed_add(x, mr) == c["p2"] and x == c["x"], (s, c["tag"], "the X / P2 - X split")
        sb = -c["u"] if c["neg"] else c["u"]
        q = ext_add(double_and_add(c["a"], p1), double_and_add(sb, mc.ed_add(x, mr)))
        xy = affine_all([q])[0]
        assert (xy == IDENT) == bool(c["expect"]), c["tag"]
        if c["tag"] == "x twin":                     # what the X condition alone accepts
            pa, pb = affine_all([double_and_add(c["a"], p1), double_and_add(sb, c["p2"])])
            assert (pa[0] + pb[0]) % P == 0 and (pa[1] + pb[1]) % P == 0 and pa[1] != pb[1] and pa[0], c["tag"]
            seen.add("twin")
        if c["tag"].startswith("small-order"):
            order = next(o for o in (1, 2, 4, 8) if affine_all([double_and_add(o, xy)])[0] == IDENT)
            res = int(c["tag"].split()[-1])
            assert order == {4: 2, 2: 4, 6: 4}.get(res, 8), (c["tag"], order)
            seen.add(order)
    assert seen == {2, 4, 8, "twin"}
    return len(picked)


# ------------------------------------------------------------ phase 1 out
def _is_identity(words40):
    x, y, z, t = _vals(words40)
    return x == 0 and t == 0 and y == z != 0


def check_lat_phase1(kernel, batch, n, st, sb_enc=None):
    """Every word phase 1 left for the first n requests against Python and the
    oracle; -> the (a, b) pairs by request (None where the hash side rejected)"""
    reqs, slots = batch["reqs"], lat_slots(kernel, n)
    assert st["slots"] == slots and st["dig"].shape == (17, slots) and st["pt"].shape == (3, 40, slots)
    assert st["ok"].shape == (3, slots)
    assert (st["accept"] == SENT).all(), "phase 1 writes no verdict"
    assert not (st["dig"] == SENT32).any() and not (st["pt"].view(np.uint32) == SENT32).any(), "a word left sentinel"
    assert (st["ok"] <= 1).all(), "an ok byte left sentinel"
    assert (np.abs(st["pt"].astype(np.int64)) <= np.array(RED * 4)[None, :, None]).all(), "a limb outside RED"
    if sb_enc is None:
        sb_enc = oracle_base_mults([q["S"] % 2**253 for q in reqs[:n]])
    ab = [None] * n
    for s in range(slots):
        worked = s < n or s < LAT_MIN_LIVE
        w = [int(v) for v in st["dig"][:, s]]
        pts = [[int(v) for v in st["pt"][k, :, s]] for k in range(3)]
        oks = tuple(int(st["ok"][k, s]) for k in range(3))
        if not worked:
            assert oks == (0, 0, 0) and not any(w) and all(_is_identity(p) for p in pts), (s, "a slot past the batch")
            continue
        if s >= n:                                    # padding repeats the last request, word for word
            for key in ("dig", "pt", "ok"):
                assert (st[key][..., s] == st[key][..., n - 1]).all(), (s, key, "padding")
            continue
        q = reqs[s]
        assert oks == q["sides"], (s, q["kind"], oks, "ok")
        if oks[0]:
            a, b, da, db, cnt = unpack_dig(st, s)
            assert 0 <= a < 2**253 and abs(b) < 2**192 and b % 2 == 1, (s, "scalar range")
            assert (a - b * q["h"]) % N8L == 0, (s, "a = b h mod 8L")
            assert da[63] >= 0 and db[63] >= 0 and all(-8 <= d <= 7 for d in da + db), (s, "digit range")
            assert cnt == max(windows(da), windows(db)), (s, "window count", cnt)
            ab[s] = (a, b)
        else:
            assert not any(w), (s, "digits of a rejected request")
        for k, enc in ((0, q["A"]), (1, q["R"])):
            if oks[k + 1]:
                x, y = neg(point_of(enc))
                X, Y, Z, T = _vals(pts[k])
                assert Z and X == x * Z % P and Y == y * Z % P and T * Z % P == X * Y % P, (s, k, "point")
            else:
                assert _is_identity(pts[k]), (s, k, "a rejected point")
        X, Y, Z, T = _vals(pts[2])                     # [S]B whatever the sides say (S cut to 253 bits)
        assert Z and T * Z % P == X * Y % P, (s, "[S]B T")
        zi = pow(Z, P - 2, P)
        x, y = X * zi % P, Y * zi % P
        assert int.to_bytes(y | ((x & 1) << 255), 32, "little") == sb_enc[s], (s, "[S]B")
    return ab


@functools.lru_cache(maxsize=None)
def _lat_phase1_state(backend, kernel, n, table_set, batch):
    return run_lat_phase1(backend, kernel, BATCHES[batch](), n, table_set)


def lat_phase1_state(backend, kernel, n, table_set, batch="prep"):
    return _lat_phase1_state(backend, kernel, n, table_set, batch)


@functools.lru_cache(maxsize=None)
def _sb_encodings(batch="prep"):
    return oracle_base_mults([q["S"] % 2**253 for q in BATCHES[batch]()["reqs"]])


def family_lat_phase1(backend, kernel, table_set, n=None, batch="prep"):
    n = batch_size(batch) if n is None else n
    return check_lat_phase1(kernel, BATCHES[batch](), n, lat_phase1_state(backend, kernel, n, table_set, batch),
                            _sb_encodings(batch)[:n])


def family_lat_sets(backend, kernel, n=None, batch="prep"):
    """the two table sets give the same [S]B (limbs may differ) and the same words otherwise"""
    n = batch_size(batch) if n is None else n
    s1, s2 = (lat_phase1_state(backend, kernel, n, ts, batch) for ts in ("compact", "large"))
    assert (s1["dig"] == s2["dig"]).all() and (s1["ok"] == s2["ok"]).all() and (s1["pt"][:2] == s2["pt"][:2]).all()
    for s in range(s1["slots"]):
        X1, Y1, Z1, _ = _vals([int(v) for v in s1["pt"][2, :, s]])
        X2, Y2, Z2, _ = _vals([int(v) for v in s2["pt"][2, :, s]])
        assert (X1 * Z2 - X2 * Z1) % P == 0 and (Y1 * Z2 - Y2 * Z1) % P == 0 and Z1 and Z2, s


def family_lat_round_trip(backend, kernel, table_set="compact", n=None, batch="prep"):
    """phase-1 out -> walk in: the verdicts the batch records (the oracle's; libsodium's for the edge batch)"""
    n = batch_size(batch) if n is None else n
    st = lat_phase1_state(backend, kernel, n, table_set, batch)
    got = run_lat_walk(backend, kernel, n, st["dig"], st["pt"], st["ok"])
    assert got[:n].tolist() == [int(q["valid"]) for q in BATCHES[batch]()["reqs"][:n]]
    assert (got[n:] == SENT).all()
    return got[:n].tolist()
