#!/usr/bin/env python3
"""Generate tests/golden/prep_edge_golden.json: requests chosen for the paths
of the prep stage (edv_prep_kernel, edv_prep_kernel_compact) and of phase 1 of
the latency kernels that honest signatures do not reach, each with libsodium
1.0.18's own crypto_sign_ed25519_verify_detached verdict.

Run here (the container has /opt/conda/lib/libsodium.so.23); the GPU box only
reads the committed .json.  Inputs are built with Python integers, hashlib, the
affine arithmetic of tests/math_cases.py and the oracle's scalarmult_base; the
digit patterns are asserted with stage_cases.recode_sb (written from the comment
above add_sb, not from its code) by stage_cases.check_edge_intent, the same
assertion edge_batch() makes when it loads the file.  The oracle
(oracle_lib.verify) must agree with libsodium on every verdict.

Families (bits / tables = 16 / 16 for the compact set, 22 / 12 for the large
one; half = 2^(bits-1)):
  s_digits     S with chosen signed digits: 0, 1, half-1, half, half+1,
               2^bits-1, 2^bits; -half at table t alone (and the carry above
               it) for every t below the top; the field of table t all ones
               for every t; every digit -half; every digit half-1; alternating
               extremes (both phases); L-1, L-2, 2^252-1, 2^252, 2^252+1,
               2^253-1; 32 seeded random S.  Each once with R = [r]B and once
               with R = [r]B + T (mixed order); A rotates over 32 keys: prime
               order and mixed order, B, -B, x even and odd, both square-root
               branches of the decompression.  Verdict 0.
  q_special    for 12 non-zero S of that list: R = [S mod 2^253]B (Q = [S]B - R
               is the identity), R = [S]B + i T8 for i = 1..7 (Q of order 8, 4,
               8, 2, 8, 4, 8), R = -[S]B (Q = 2 [S]B).
  s_canonical  S = L - 2^(32w) and L + 2^(32w) for w = 0..7, L, L+1, 2^253,
               2^255+5, 2^256-1, L with its low 64 bits cleared.
  accepted     valid signatures made with a free nonce, R = [r]B, S = r + h a
               mod L, the message ending in a counter ground until the wanted
               digit appears: compact set digit 0 at every t = 0..15 and -half
               at every t = 0..14 (four of them under a mixed-order A with
               8 | h), large set digit 0 and -half at t = 0, 5, 10 (about 2^22
               tries each; the search runs on every core, the smallest counter
               wins, so the result does not depend on the core count).

Order: a case of every family among the first 64; a q_special identity case at
index 62 and an accepted case at index 63 (the last slots of the first wave);
the last request an s_canonical case with S >= L.

The "sha256" field is stage_cases.edge_sha256(requests): the hash of the
request list in canonical JSON.
"""
import ctypes
import hashlib
import json
import os
import random
import sys
from multiprocessing import Pool

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import math_cases as mc  # noqa: E402
import oracle_lib as orc  # noqa: E402
import stage_cases as sc  # noqa: E402
from math_cases import L  # noqa: E402

na = ctypes.CDLL("/opt/conda/lib/libsodium.so.23")
assert na.sodium_init() >= 0
na.sodium_version_string.restype = ctypes.c_char_p
assert na.sodium_version_string() == b"1.0.18", na.sodium_version_string()


def sodium_verify(sig: bytes, msg: bytes, pk: bytes) -> int:
    return 1 if na.crypto_sign_ed25519_verify_detached(sig, msg, ctypes.c_ulonglong(len(msg)), pk) == 0 else 0


def le(x: int) -> bytes:
    return x.to_bytes(32, "little")


def secret_scalar(seed: bytes) -> int:
    h = bytearray(hashlib.sha512(seed).digest()[:32])
    h[0] &= 248
    h[31] &= 127
    h[31] |= 64
    return int.from_bytes(h, "little")


def make_keys(rng):
    """32 keys as (encoding, secret scalar, mixed order): 16 honest ones, 14 with
    a torsion component, B and -B; both x parities and both square-root branches
    among the prime-order and among the mixed-order ones"""
    keys = []
    for _ in range(16):
        seed = bytes(rng.getrandbits(8) for _ in range(32))
        keys.append((orc.keypair(seed)[0], secret_scalar(seed) % L, False))
    for i in range(14):
        a0 = secret_scalar(bytes(rng.getrandbits(8) for _ in range(32))) % L
        keys.append((mc.ed_encode(mc.ed_add(sc.base_mult(a0), sc.TORSION[1 + i % 7])), a0, True))
    B = sc.base_mult(1)
    keys += [(mc.ed_encode(B), 1, False), (mc.ed_encode(sc.neg(B)), L - 1, False)]
    assert len({k[0] for k in keys}) == 32
    return keys


def set_scalars(ts):
    """(tag, S, want) for one table set: the chosen digit patterns"""
    bits, tables = sc.SET_BITS[ts], sc.SET_TABLES[ts]
    half, top = 1 << (bits - 1), tables - 1
    value = lambda digits: sum(d << (bits * t) for t, d in digits.items())      # noqa: E731
    out = []

    def add(tag, digits):
        s = value(digits)
        assert 0 <= s < 2**253, tag
        want = {"set": ts, "digits": {str(t): d for t, d in sorted(digits.items())}, "others": 0}
        out.append(("%s %s" % (ts, tag), s, want))

    add("0", {})
    add("1", {0: 1})
    add("half-1", {0: half - 1})
    add("half", {0: -half, 1: 1})
    add("half+1", {0: -half + 1, 1: 1})
    add("2^bits-1", {0: -1, 1: 1})
    add("2^bits", {1: 1})
    for t in range(top):
        add("-half at %d" % t, {t: -half, t + 1: 1})
    for t in range(top):
        add("ones at %d" % t, {t: -1, t + 1: 1})
    add("ones at %d" % top, {top: (2**253 - 1) >> (bits * top)})
    add("every digit -half", {**{t: -half for t in range(top)}, top: 1})
    add("every digit half-1", {**{t: half - 1 for t in range(top)}, top: (2**252 >> (bits * top)) - 1})
    add("alternating -half, half-1", {**{t: (half - 1 if t & 1 else -half) for t in range(top)}, top: 1})
    add("alternating half-1, -half", {**{t: (-half if t & 1 else half - 1) for t in range(top)}, top: 1})
    # the values the issue names, as integers
    named = {"0": 0, "1": 1, "half-1": half - 1, "half": half, "half+1": half + 1, "2^bits-1": 2**bits - 1, "2^bits": 2**bits}
    for tag, s, _w in out:
        name = tag.split(" ", 1)[1]
        if name in named:
            assert s == named[name], tag
        if name.startswith("-half at "):
            assert s == half << (bits * int(name.split()[-1])), tag
        if name.startswith("ones at "):
            assert s == ((2**bits - 1) << (bits * int(name.split()[-1]))) & (2**253 - 1), tag
    return out


# ---- the search for an accepted signature whose S has a wanted digit
def _grind_chunk(args):
    R, A, a, r, prefix, ts, t, d, need8, lo, hi = args
    bits = sc.SET_BITS[ts]
    mask, half, shift = (1 << bits) - 1, 1 << (bits - 1), bits * t
    fields = (0, mask) if d == 0 else (half, half - 1)       # without and with a carry from below
    base = hashlib.sha512(R + A + prefix)
    for c in range(lo, hi):
        hh = base.copy()
        hh.update(c.to_bytes(8, "little"))
        h = int.from_bytes(hh.digest(), "little") % L
        if need8 and h & 7:
            continue
        s = (r + h * a) % L
        if ((s >> shift) & mask) not in fields:
            continue
        if sc.recode_sb(s, ts)[t] == d:
            return c
    return None


def grind(pool, workers, R, A, a, r, prefix, ts, t, d, need8):
    """the smallest counter c for which S = r + h a mod L, h = SHA-512(R || A || prefix || c), has digit d at table t"""
    step = 1 << (13 if sc.SET_BITS[ts] == 16 and not need8 else 17)
    lo = 0
    while True:
        jobs = [(R, A, a, r, prefix, ts, t, d, need8, lo + k * step, lo + (k + 1) * step) for k in range(workers)]
        for c in pool.map(_grind_chunk, jobs):
            if c is not None:
                return c
        lo += workers * step
        assert lo < 1 << 32, "no counter found"


def main():
    rng = random.Random(0xED6E2026)
    rbytes = lambda n: bytes(rng.getrandbits(8) for _ in range(n))               # noqa: E731
    keys = make_keys(rng)
    prime = [k for k in keys if not k[2]][:16]
    mixed = [k for k in keys if k[2]]
    nk = [0]

    def next_key():
        nk[0] += 1
        return keys[(nk[0] - 1) % len(keys)][0]

    def req(family, tag, R, S, A, msg, want):
        return {"family": family, "tag": tag, "R": R, "S": S, "A": A, "msg": msg, "want": want}

    # ---- s_digits
    shared = [(name, s, {"value": name}) for name, s in sc.NAMED_S.items()]
    shared += [("random %d" % k, rng.randrange(L), {"random": 1}) for k in range(32)]
    per_set = {ts: set_scalars(ts) for ts in ("compact", "large")}
    lists = [per_set["compact"], per_set["large"], shared]
    scalars = [lst[k] for k in range(max(len(x) for x in lists)) for lst in lists if k < len(lst)]   # interleaved
    s_digits = []
    for k, (tag, s, want) in enumerate(scalars):
        for mix in (0, 1):
            Rp = sc.base_mult(rng.randrange(1, L))
            if mix:
                Rp = mc.ed_add(Rp, sc.TORSION[1 + k % 7])
            s_digits.append(req("s_digits", tag + (", mixed-order R" if mix else ", prime-order R"), mc.ed_encode(Rp), s,
                                next_key(), rbytes(rng.randrange(0, 91)), dict(want, r_mixed=mix)))
    by_tag = {tag: s for tag, s, _w in scalars}

    # ---- q_special
    picks = ["compact 1", "compact half", "compact every digit -half", "compact every digit half-1",
             "compact alternating -half, half-1", "large half", "large every digit -half", "large every digit half-1",
             "large alternating half-1, -half", "L-1", "2^252", "2^253-1"]
    q_special = []
    for tag in picks:
        s = by_tag[tag]
        sb = sc.base_mult(s % 2**253)
        cases = [("R = [S]B", sb, {"q_order": 1})]
        cases += [("R = [S]B + %d T8" % i, mc.ed_add(sb, sc.TORSION[i]), {"q_order": sc.order_of(sc.TORSION[i])})
                  for i in range(1, 8)]
        cases += [("R = -[S]B", sc.neg(sb), {"q": "2sb"})]
        for what, Rp, want in cases:
            q_special.append(req("q_special", "%s, %s" % (tag, what), mc.ed_encode(Rp), s, next_key(),
                                 rbytes(rng.randrange(0, 91)), want))
    assert [c["want"].get("q_order") for c in q_special[:9]] == [1, 8, 4, 8, 2, 8, 4, 8, None]

    # ---- s_canonical
    low64_cleared = L >> 64 << 64
    vals = [("L - 2^%d" % (32 * w), L - 2**(32 * w)) for w in range(8)]
    vals += [("L + 2^%d" % (32 * w), L + 2**(32 * w)) for w in range(8)]
    vals += [("L", L), ("L + 1", L + 1), ("2^253", 2**253), ("2^255 + 5", 2**255 + 5),
             ("L with its low 64 bits cleared", low64_cleared), ("2^256 - 1", 2**256 - 1)]
    assert sum(1 for _t, s in vals[:8] if s >= 2**252) >= 3 and low64_cleared >= 2**252
    s_canonical = []
    for tag, s in vals:
        pk, _a, _m = prime[rng.randrange(16)]
        s_canonical.append(req("s_canonical", tag, mc.ed_encode(sc.base_mult(rng.randrange(1, L))), s, pk,
                               rbytes(rng.randrange(0, 91)), {"lt_l": int(s < L), "ge_2_252": int(s >= 2**252)}))

    # ---- accepted
    wanted = [("compact", t, 0, False) for t in range(16)] + [("compact", t, -(1 << 15), False) for t in range(15)]
    for k in (3, 12, 19, 28):                                  # a mixed-order A and 8 | h: digit 0 at 3 and 12, -half at 3 and 12
        wanted[k] = wanted[k][:3] + (True,)
    wanted += [("large", t, d, False) for t in (0, 5, 10) for d in (0, -(1 << 21))]
    accepted = []
    workers = min(16, os.cpu_count() or 1)
    with Pool(workers) as pool:
        for k, (ts, t, d, mix) in enumerate(wanted):
            A, a, _m = (mixed if mix else prime)[k % (14 if mix else 16)]
            r = rng.randrange(1, L)
            R = mc.ed_encode(sc.base_mult(r))
            tag = "%s digit %s at %d%s" % (ts, "0" if d == 0 else "-half", t, ", mixed-order A, 8 | h" if mix else "")
            prefix = tag.encode() + b" #"
            c = grind(pool, workers, R, A, a, r, prefix, ts, t, d, mix)
            msg = prefix + c.to_bytes(8, "little")
            h = int.from_bytes(hashlib.sha512(R + A + msg).digest(), "little") % L
            want = {"set": ts, "digits": {str(t): d}, "accept": 1}
            if mix:
                want["a_mixed"] = 1
            accepted.append(req("accepted", tag, R, (r + h * a) % L, A, msg, want))
            print("accepted: %s after %d tries" % (tag, c + 1), flush=True)

    # ---- the order
    q_ident = [c for c in q_special if c["want"].get("q_order") == 1]
    q_other = [c for c in q_special if c["want"].get("q_order") != 1]
    reqs = s_digits[:50] + s_canonical[:4] + q_other[:8] + q_ident[:1] + accepted[:1]
    assert len(reqs) == 64
    reqs += s_digits[50:] + q_ident[1:] + q_other[8:] + accepted[1:] + s_canonical[4:]

    # ---- verdicts, the intents, the file
    out = []
    for c in reqs:
        sig = c["R"] + le(c["S"])
        verdict = sodium_verify(sig, c["msg"], c["A"])
        assert verdict == int(orc.verify(sig, c["msg"], c["A"])), (c["tag"], "the oracle disagrees with libsodium")
        assert verdict == int(c["family"] == "accepted"), c["tag"]
        sc.check_edge_intent(dict(c, kind=c["tag"], valid=verdict))
        out.append({"family": c["family"], "tag": c["tag"], "R": c["R"].hex(), "S": le(c["S"]).hex(), "A": c["A"].hex(),
                    "msg": c["msg"].hex(), "want": c["want"], "verdict": verdict})
    sc.check_edge_layout([dict(c, kind=c["tag"]) for c in reqs])
    per = {}
    for c in out:
        per.setdefault(c["family"], [0, 0])[c["verdict"]] += 1
    doc = {"generator": "tests/golden/make_prep_edge_golden.py",
           "verdicts_from": "libsodium 1.0.18 crypto_sign_ed25519_verify_detached (/opt/conda/lib/libsodium.so.23)",
           "count": len(out), "accepted": sum(c["verdict"] for c in out), "per_family_reject_accept": per,
           "sha256": sc.edge_sha256(out), "requests": out}
    with open(os.path.join(HERE, "prep_edge_golden.json"), "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: doc[k] for k in ("count", "accepted", "sha256", "per_family_reject_accept")}))


if __name__ == "__main__":
    main()
