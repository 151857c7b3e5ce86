"""Cases and Python-integer checkers for the kernels' arithmetic, shared by the
two builds of the headers: the CPU build (libedv_hostcheck.so) and the device
build (the probe kernels of libedv_measure.so).  A family function takes
`run(op, packed cases) -> packed results` (probe_lib.host or probe_lib.device),
generates its cases, runs them and asserts every result against plain
Python integers (exact rationals for the divisions).  Not a conftest.

Limb bounds used below, from the code:
  BOUND  the input bound fe_mul / fe_sq / fe_sq_cols are specified for
         (edv_math.h): |f_i| <= 1.65 * 2^26 (even i), 1.65 * 2^25 (odd i);
  RED    the output bound of fe_mul / fe_sq / fe_sq2 / fe_carry32 ("reduced",
         out_ok): |h_i| <= 2^25 + 2^20 (even), 2^24 + 2^20 (odd).
The quad arithmetic (edv_quad_math.h) is handed RED limb vectors only: a
distributed point is an fe_mul output (quad_dbl, quad_add, quad_cached), a
decompressed point (fe_carry32 / fe_mul outputs and the constant 1), an [S]B
sum (fe_mul outputs) or the identity (limbs 0 / 1); a cached entry is a
quad_cached output (fe_mul), negated or with two lanes swapped, or the
identity entry (1 | 1 | 0 | 1).  quad_cached multiplies by fe_one() and
fe_d2(), whose limbs are below RED.  So the extremes the callers can reach
are +-RED in every sign pattern; quad_bounds() pushes that bound through the
two stages of quad_dbl and quad_add as written."""
import functools
import random
from fractions import Fraction

import numpy as np

import probe_lib as pl

P = 2**255 - 19
L = 2**252 + 27742317777372353535851937790883648493
N8L = 8 * L
POS = [0, 26, 51, 77, 102, 128, 153, 179, 204, 230]
# input bound the multiply is specified for: |f_i| <= 1.65 * 2^26 (even i), 1.65 * 2^25 (odd i)
BOUND = [int(1.65 * 2**26) if i % 2 == 0 else int(1.65 * 2**25) for i in range(10)]
RED = [2**25 + 2**20 if i % 2 == 0 else 2**24 + 2**20 for i in range(10)]
D = (-121665 * pow(121666, P - 2, P)) % P
D2_LIMBS = [45281625, 27714825, 36363642, 13898781, 229458, 15978800, 54557047, 27058993, 29715967, 9444199]
M256 = 2**256 - 1


def val(l):
    return sum(int(x) << POS[i] for i, x in enumerate(l))


def limbs(x):
    return [(x >> POS[i]) & ((1 << (26 if i % 2 == 0 else 25)) - 1) for i in range(10)]


def rand_limbs(r, extreme=False):
    if extreme:
        return [r.choice([-BOUND[i], BOUND[i], BOUND[i] - 1, -BOUND[i] + 1]) for i in range(10)]
    return [r.randrange(-BOUND[i], BOUND[i] + 1) for i in range(10)]


def out_ok(h):
    # outputs must be reduced enough to feed another multiply after one add/sub
    return all(abs(h[i]) <= (2**25 + 2**20 if i % 2 == 0 else 2**24 + 2**20) for i in range(10))


def red_limbs(r, extreme=False):
    """A limb vector inside RED (what fe_mul returns); extreme: every limb at +-RED or one inside."""
    if extreme:
        return [r.choice([-RED[i], RED[i], RED[i] - 1, -RED[i] + 1]) for i in range(10)]
    return [r.randrange(-RED[i], RED[i] + 1) for i in range(10)]


# ---------------------------------------------------------------- case lists
def fe_mul_sq_cases():
    r = random.Random(5)
    return [(rand_limbs(r, extreme=(it % 3 == 0)), rand_limbs(r, extreme=(it % 5 == 0))) for it in range(3000)]


def fe_sq_floor_starts():
    r = random.Random(9)
    top = [(1 << 26) - 1 if i % 2 == 0 else (1 << 25) - 1 for i in range(10)]
    starts = [[r.randrange(-2**25, 2**25) if i % 2 == 0 else r.randrange(-2**24, 2**24) for i in range(10)]
              for _ in range(300)]
    starts += [[(2**25 if i % 2 == 0 else 2**24) * s for i in range(10)] for s in (1, -1)]
    starts += [top, [t if i != 1 else (1 << 25) + (1 << 17) for i, t in enumerate(top)]]
    return starts


def fe_bytes_values():
    r = random.Random(6)
    specials = [0, 1, P - 1, P, P + 1, 2 * P - 1, 2**255 - 1, 2**255 - 20, 19, 2**255 - 19 - 1]
    xs = specials + [r.randrange(2**255) for _ in range(2000)]
    noncanon = [[r.randrange(-2**25, 2**25) if i % 2 == 0 else r.randrange(-2**24, 2**24) for i in range(10)]
                for _ in range(2000)]
    return xs, noncanon


def fe_invert_cases():
    """canonical values, then arbitrary signed limb vectors within the mul input bounds (half all-extreme)"""
    r = random.Random(17)
    xs = [1, 2, 3, 19, P - 1, P - 2, (P - 1) // 2, 2**254, 2**255 - 20] + [r.randrange(1, P) for _ in range(3000)]
    vecs = [rand_limbs(r, extreme=(it % 2 == 0)) for it in range(3000)]
    return xs, vecs


def sc_reduce_values():
    r = random.Random(8)
    vals = [0, 1, L - 1, L, L + 1, 2 * L - 1, 2 * L, 2**512 - 1, 2**511, 2**253 - 1, 8 * L + 7]
    vals += [k * L + d for k in (1, 2**100, 2**258 - 1) for d in (-1, 0, 1)]
    vals += [r.randrange(2**512) for _ in range(3000)]
    return vals


def half_scalars_edges():
    edge = [0, 1, 2, 3, L - 1, L - 2, 2**128 - 1, 2**128, 2**128 + 1, 2**252, 2**252 - 1, 8, 2**64, 2**64 + 1]
    # large partial quotients (the binary long-division path): h near N8L / 2^k and N8L * j / k
    edge += [N8L >> k for k in (4, 40, 64, 100, 124, 130, 200) if (N8L >> k) < L]
    edge += [(N8L >> k) + 1 for k in (40, 100, 126)]
    edge += [(N8L * j // k) % L for j, k in ((1, 3), (2, 7), (5, 11), (1, 2**33 + 1), (7, 2**61 - 1))]
    edge += [(2**140 * x) % L for x in (1, 3, 5)]
    # a huge quotient after a few ordinary ones (negative cofactor at that point)
    for k in (33, 40, 70, 110):
        for q1 in (1, 2, 3):
            x = N8L * 2**k // (q1 * 2**k + 1)          # N8L / h = q1 + 1/2^k
            edge += [x % L, (x + 12345) % L]
            x = N8L * (2**k + 1) // (2 * 2**k + 3)     # quotients 1, 1, ~2^(k-1), ...
            edge += [x % L]
    return edge


def half_scalars_values():
    r = random.Random(21)
    edge = half_scalars_edges()
    return edge, edge + [r.randrange(L) for _ in range(20000)]


def recoding_values():
    r = random.Random(12)
    # V2 admits every S < 2^252 and canonical S < L; h and signer scalars are < L
    edge = [0, 1, L - 1, 2**252 - 1, 2**252, 2**253 - 1 - (2**253 - L)]
    edge += [int("8000" * 16, 16) % L, int("7fff" * 16, 16) % L, int("ffff" * 15, 16), int("80" * 31, 16)]
    edge += [int("88" * 31, 16), int("77" * 31, 16)]
    return [v for v in edge if 0 <= v < L] + [r.randrange(L) for _ in range(2000)]


def digits_windows_cases():
    r = random.Random(11)
    cases = [[0] * 8, [1] + [0] * 7, [0] * 7 + [0xF0000000], [0] * 7 + [1], [0x80000000] + [0] * 7]
    for _ in range(3000):
        w = [0] * 8
        top = r.randrange(64)
        for k in range(top + 1):
            w[k // 8] |= r.randrange(16) << (4 * (k % 8))
        w[top // 8] |= r.randrange(1, 16) << (4 * (top % 8))
        cases.append(w)
    return cases


def signed_digits(packed, bits):
    """Digit k at bits [bits k, bits k + bits) of the packed 256-bit value."""
    v = sum(w << (32 * i) for i, w in enumerate(packed))
    out = []
    for k in range(256 // bits):
        raw = (v >> (bits * k)) & ((1 << bits) - 1)
        out.append(raw - (1 << bits) if raw >> (bits - 1) else raw)
    return out


# ---------------------------------------------------------------- the curve
def ed_add(p1, p2):
    (x1, y1), (x2, y2) = p1, p2
    t = D * x1 * x2 * y1 * y2 % P
    return ((x1 * y2 + y1 * x2) * pow(1 + t, P - 2, P) % P, (y1 * y2 + x1 * x2) * pow(1 - t, P - 2, P) % P)


def ed_decode(b):
    v = int.from_bytes(b, "little")
    y, sign = v & ((1 << 255) - 1), v >> 255
    if y >= P:
        return None
    u, w = (y * y - 1) % P, (D * y * y + 1) % P
    x = pow(u * pow(w, P - 2, P), (P + 3) // 8, P)
    if (w * x * x - u) % P:
        x = x * pow(2, (P - 1) // 4, P) % P
    if (w * x * x - u) % P:
        return None
    if x == 0 and sign:
        return None
    if (x & 1) != sign:
        x = P - x
    return x, y


def ed_encode(pt):
    x, y = pt
    return int.to_bytes(y | ((x & 1) << 255), 32, "little")


SQRTM1 = pow(2, (P - 1) // 4, P)
# the torsion subgroup: order 1, 2, 4, 4, 8 x 4 (the order-8 points are the
# two y of libsodium's blocklist with either sign of x)
ORDER8_Y = (int.from_bytes(bytes.fromhex("26e8958fc2b227b045c3f489f2ef98f0d5dfac05d3c63339b13802886d53fc05"), "little"),
            int.from_bytes(bytes.fromhex("c7176a703d4dd84fba3c0b760d10670f2a2053fa2c39ccc64ec7fd7792ac037a"), "little"))


def torsion_points():
    pts = [(0, 1), (0, P - 1), (SQRTM1, 0), (P - SQRTM1, 0)]
    for y in ORDER8_Y:
        x, _ = ed_decode(y.to_bytes(32, "little"))
        pts += [(x, y), (P - x, y)]
    return pts


# ------------------------------------------------------------ lane families
def family_fe_mul_sq(run):
    """fe_mul, fe_sq, fe_sq2 at +-1.65 * 2^26 / 2^25: exact mod p, outputs reduced"""
    cases = fe_mul_sq_cases()
    got = pl.unpack_limbs(run("fe_mul", pl.pack_limbs([[f, g] for f, g in cases])))
    for (f, g), h in zip(cases, got):
        assert val(h[0]) % P == val(f) * val(g) % P and out_ok(h[0]), ("fe_mul", f, g)
    fs = pl.pack_limbs([[f] for f, _ in cases])
    for op, k in (("fe_sq", 1), ("fe_sq2", 2)):
        for (f, _), h in zip(cases, pl.unpack_limbs(run(op, fs))):
            assert val(h[0]) % P == k * val(f) ** 2 % P and out_ok(h[0]), (op, f)


def family_fe_sq_floor(run):
    """fe_sq_floor 40 squarings deep from signed reduced and unsigned extreme starts"""
    cur = fe_sq_floor_starts()
    xs = [val(f) % P for f in cur]
    for _ in range(40):
        cur = [h[0] for h in pl.unpack_limbs(run("fe_sq_floor", pl.pack_limbs([[f] for f in cur])))]
        xs = [x * x % P for x in xs]
        for c, x in zip(cur, xs):
            assert val(c) % P == x
            assert all(0 <= c[i] < (1 << (26 if i % 2 == 0 else 25)) for i in range(10) if i != 1)
            assert -(1 << 17) <= c[1] < (1 << 25) + (1 << 17)


def family_fe_bytes(run):
    """fe_frombytes (bit 255 ignored, values >= p) and canonical fe_tobytes"""
    xs, noncanon = fe_bytes_values()
    hs = [h[0] for h in pl.unpack_limbs(run("fe_frombytes", pl.pack_ints([[x] for x in xs], 32)))]
    back = pl.unpack_ints(run("fe_tobytes", pl.pack_limbs([[h] for h in hs])), 32)
    for x, h, b in zip(xs, hs, back):
        y = x & (2**255 - 1)  # bit 255 (the sign bit) is ignored by the decoder
        assert val(h) % P == y % P and out_ok(h), hex(x)
        assert b[0] == y % P, hex(x)
    for f, b in zip(noncanon, pl.unpack_ints(run("fe_tobytes", pl.pack_limbs([[f] for f in noncanon])), 32)):
        assert b[0] == val(f) % P, f


def family_fe_invert_pow(run):
    """fe_invert_safegcd and fe_pow22523 on canonical and bound-extreme limb vectors"""
    xs, vecs = fe_invert_cases()
    ins = [limbs(x) for x in xs] + vecs + [[0] * 10]
    packed = pl.pack_limbs([[f] for f in ins])
    inv = [h[0] for h in pl.unpack_limbs(run("fe_invert_safegcd", packed))]
    pw = [h[0] for h in pl.unpack_limbs(run("fe_pow22523", packed))]
    for f, a, b in zip(ins, inv, pw):
        x = val(f) % P
        assert val(a) % P == pow(x, P - 2, P) and out_ok(a), f
        assert val(b) % P == pow(x, (P - 5) // 8, P) and out_ok(b), f


def family_sc_reduce(run):
    """sc_reduce at k L + {-1, 0, 1}, the 512-bit extremes and random inputs"""
    vals = [v for v in sc_reduce_values() if 0 <= v < 2**512]
    for v, o in zip(vals, pl.unpack_ints(run("sc_reduce", pl.pack_ints([[v] for v in vals], 64)), 32)):
        assert o[0] == v % L, hex(v)


def half_scalars_run(run, hs):
    """-> [(a, b)] with b signed"""
    out = run("half_scalars", pl.pack_ints([[h] for h in hs], 32))
    a_u = pl.unpack_ints(out[:, :64], 32)
    neg = np.ascontiguousarray(out[:, 64:68]).view(np.uint32)[:, 0]
    assert set(neg.tolist()) <= {0, 1}
    return [(a, -u if n else u) for (a, u), n in zip(a_u, neg.tolist())]


def family_half_scalars(run):
    """The lattice reduction: a = b h (mod 8L), b odd, a in [0, 2^253), |b| <
    2^192 for every h < L (adversarial partial quotients among them), both
    about 2^128 for 20,000 hash-like h.  -> the (a, b) pairs, edge cases first."""
    edge, vals = half_scalars_values()
    res = half_scalars_run(run, vals)
    lens = []
    for h, (a, b) in zip(vals, res):
        assert 0 <= a < 2**253 and abs(b) < 2**192, hex(h)
        assert b % 2 == 1, hex(h)
        assert (a - b * h) % N8L == 0, hex(h)
        lens.append(max(a.bit_length(), abs(b).bit_length()))
    rand = sorted(lens[len(edge):])
    assert len(rand) == 20000
    assert rand[len(rand) // 2] <= 128 and rand[-1] <= 142, (rand[len(rand) // 2], rand[-1])
    return res


def recode5_values():
    """scalars < 2^253 (recode5's domain: a < 2^253, u < 2^192): the recoding
    edges, digit-carry runs (all 7s / 8s / fs), every single 4-bit field at 8
    and every power of two"""
    vals = recoding_values() + [2**253 - 1, 2**253 - 2**249, int("7" * 63, 16), int("8" * 62, 16), int("f" * 62, 16)]
    vals += [8 << (4 * k) for k in range(63)] + [1 << k for k in range(253)]
    vals += [(1 << k) - 1 for k in range(1, 254)]
    return vals


def family_recode(run):
    """recode5 + digits5_windows: digits in [-8, 7] (top one >= 0) that sum back
    to the scalar, and the window count 1 + the top nonzero digit's index"""
    vals = recode5_values()
    out = np.ascontiguousarray(run("recode5", pl.pack_ints([[v] for v in vals], 32))).view(np.uint32).tolist()
    for v, o in zip(vals, out):
        d = signed_digits(o[:8], 4)
        assert sum(x << (4 * k) for k, x in enumerate(d)) == v, hex(v)
        assert all(-8 <= x <= 7 for x in d[:-1]) and 0 <= d[-1] <= 7, hex(v)
        assert o[8] == max([k + 1 for k in range(64) if d[k]], default=0), hex(v)


# ------------------------------------------------------------------ division
def approx_div_cases():
    """(a, b) doubles: denominators over the mantissa range (1.0, 2 - ulp,
    1 + ulp, 2^k +- 1, all-ones prefixes and suffixes, 50,000 random) at
    exponents 0..255 (a 256-bit remainder's range), numerators for quotients
    from 1 up to 2^53"""
    r = random.Random(41)
    mants = [0, 2**52 - 1, 1, 2, 3, 2**51, 2**51 + 1, 2**51 - 1]
    mants += [2**k for k in range(52)] + [2**52 - 2**k for k in range(52)] + [2**k - 1 for k in range(1, 52)]
    mants += [(2**k + 1) << (52 - k) & (2**52 - 1) for k in range(1, 52)]   # 2^k + 1
    mants += [((2**k - 1) << (53 - k)) & (2**52 - 1) for k in range(2, 53)]   # 2^k - 1
    dens = [(m, e) for m in sorted(set(mants)) for e in (0, 1, 31, 127, 128, 255)]
    dens += [(r.randrange(2**52), r.randrange(256)) for _ in range(50000)]
    cases = []
    for i, (m, e) in enumerate(dens):
        b = float((2**52 + m) << e) / 2.0**52
        k = (i // 3) % 54                                 # quotient magnitude 2^k .. 2^(k+1), each kind below at each
        if i % 3 == 0:
            a = b * float(r.randrange(2**k, 2**(k + 1)))  # an (almost) integer quotient
        elif i % 3 == 1:
            a = b * (float(r.randrange(2**52, 2**53)) / 2.0**52) * 2.0**k
        else:
            a = float(int(b * 2.0**k) + r.randrange(-1, 2))
        if a < b:
            a = b
        cases.append((a, b))
    # quotient exactly 1, just above, and the largest
    cases += [(1.0, 1.0), (2.0**53, 1.0), (2.0**256, 2.0**203 + 2.0**151), (float(2**53 - 1), 1.0)]
    return cases


def rel_error(got, a, b):
    """|got - a / b| / (a / b), exactly"""
    q = Fraction(a) / Fraction(b)
    return abs(Fraction(got) - q) / q


def family_approx_div(run):
    """approx_div against exact rationals: euclid_div needs the relative error
    below 2^-45 (its operands carry < 2^-49 each and the (1 - 2^-44) factor must
    keep the estimate from exceeding the quotient).  -> the largest error seen."""
    cases = approx_div_cases()
    got = pl.unpack_doubles(run("approx_div", pl.pack_doubles(cases)))[:, 0].tolist()
    worst, where = Fraction(0), None
    for (a, b), g in zip(cases, got):
        e = rel_error(g, a, b)
        if e > worst:
            worst, where = e, (a.hex(), b.hex(), g.hex())
    print("approx_div: %d cases, largest relative error 2^%.2f at %s" %
          (len(cases), float(np.log2(float(worst))) if worst else float("-inf"), where))
    assert worst < Fraction(1, 2**45), where
    return worst


DIV_QUOTIENTS = sorted(set([1, 2, 3] + [2**k + d for k in range(1, 32) for d in (-1, 0, 1)]))
DIV_QUOTIENTS_BIG = [2**40, 2**45, 2**50]


def fdiv_floor_cases():
    """(a, b) exact integers below 2^53 with a in {q b - 1, q b, q b + 1,
    q b + b - 1}: q over 1, 2, 3, 2^k - 1, 2^k, 2^k + 1 (k <= 31), 2^40, 2^45,
    2^50 and their neighbours, and every magnitude 2^k (k < 52) for the measured
    range; b small, a power of two +- 1, random and the largest that fits"""
    r = random.Random(43)
    qs = DIV_QUOTIENTS + [q + d for q in DIV_QUOTIENTS_BIG for d in (-1, 0, 1)]
    qs += [r.randrange(2**k, 2**(k + 1)) for k in range(32, 52) for _ in range(8)]
    cases = []
    for q in qs:
        bmax = (2**53 - 1) // (q + 1)
        bs = {1, 2, 3, 5, 7, bmax, bmax - 1, max(1, bmax // 2), max(1, bmax // 3)}
        bs |= {2**k + d for k in range(1, 53, 3) for d in (-1, 0, 1)}
        bs |= {r.randrange(1, bmax + 1) for _ in range(12)}
        for b in sorted(x for x in bs if 1 <= x <= bmax):
            for a in (q * b - 1, q * b, q * b + 1, q * b + b - 1):
                if a >= 0:
                    cases.append((a, b))
    return cases


def family_fdiv_floor(run):
    """fdiv_floor against integer division: exact for every quotient below 2^31
    (all a Lehmer round accepts before its 2^30 cofactor break) and below 2^45
    (what a relative error under 2^-45 implies: the estimate is then within one
    of the quotient, and the exact remainder test fixes that).  -> the bit
    length up to which every sampled quotient came out exact."""
    cases = fdiv_floor_cases()
    got = pl.unpack_doubles(run("fdiv_floor", pl.pack_doubles([(float(a), float(b)) for a, b in cases])))[:, 0]
    bad_bits = 64
    for (a, b), g in zip(cases, got.tolist()):
        if g != float(a // b):
            assert a // b >= 2**45, ("fdiv_floor", a, b, g)
            bad_bits = min(bad_bits, (a // b).bit_length())
    top = max((a // b).bit_length() for a, b in cases)
    exact_bits = min(bad_bits - 1, top)
    print("fdiv_floor: %d cases, exact for every sampled quotient below 2^%d (largest sampled: 2^%d)" %
          (len(cases), exact_bits, top))
    return exact_bits


def _sx(t):
    """two's complement 256-bit word vector -> signed"""
    return t - 2**256 if t >> 255 else t


def euclid_states(h):
    """The (r0, t0, r1, t1) of every division step of Euclid on (8L, h), cofactors mod 2^256"""
    r0, r1, t0, t1 = N8L, h, 0, 1
    out = []
    while r1:
        out.append((r0, t0 & M256, r1, t1 & M256))
        q = r0 // r1
        r0, r1, t0, t1 = r1, r0 - q * r1, t1, t0 - q * t1
    return out


def euclid_div_cases():
    """Euclid's own steps on (8L, h) for the adversarial h of half_scalars_edges
    (huge partial quotients: the long-division branch) and some hash-like h;
    then synthetic r0 = q r1 + rem with q over the division quotient list
    (below and above 2^31), rem in {0, 1, r1 - 1, random} and r1 from 1 bit to
    as many as fit"""
    r = random.Random(47)
    cases = []
    for h in half_scalars_edges() + [r.randrange(L) for _ in range(40)]:
        if h:
            # half_scalars divides only while r1 >= 2^64 (its quotients stay below 2^192)
            cases += [c for c in euclid_states(h) if c[2] >= 2**64]
    qs = DIV_QUOTIENTS + DIV_QUOTIENTS_BIG + [2**31 + 5, 2**32 - 1, 2**32, 2**32 + 1, 2**63 + 1, 2**100 + 3, 2**127 - 1]
    for q in qs:
        room = 250 - q.bit_length()
        for bits in sorted({1, 2, 31, 32, 33, 53, 54, 64, 65, 127, 128, 129, 140, room - 1, room}):
            if not 1 <= bits <= room:
                continue
            for r1 in (2**(bits - 1), 2**bits - 1, r.randrange(2**(bits - 1), 2**bits)):
                # cofactors as Euclid keeps them: |t1| r0 below 2^255, so t1 2^e never overflows
                tmax = 2**(253 - (q * r1).bit_length())
                for rem in sorted({0, 1 % r1, r1 - 1, r.randrange(r1)}):
                    t1 = r.randrange(-tmax, tmax + 1)
                    t0 = r.randrange(-2**200, 2**200)
                    cases.append((q * r1 + rem, t0 & M256, r1, t1 & M256))
    return cases


def family_euclid_div(run):
    """euclid_div: r0 <- r0 mod r1, t0 <- t0 - floor(r0 / r1) t1 (mod 2^256), on
    both of its branches (double-precision estimate below 2^31, long division)"""
    cases = euclid_div_cases()
    assert sum(1 for c in cases if c[0] // c[2] >= 2**31) >= 200 and sum(1 for c in cases if c[0] // c[2] < 2**31) >= 2000
    out = pl.unpack_ints(run("euclid_div", pl.pack_ints(cases, 32)), 32)
    for (r0, t0, r1, t1), (g0, gt) in zip(cases, out):
        q = r0 // r1
        assert g0 == r0 - q * r1, ("r0", hex(r0), hex(r1))
        assert gt == (_sx(t0) - q * _sx(t1)) & M256, ("t0", hex(r0), hex(r1), hex(t0), hex(t1))


# ------------------------------------------------------------- decompression
def ge_frombytes_encodings(base_points):
    """32-byte strings: valid points (`base_points`: encodings of [k]B), the same
    with the sign bit flipped, torsion-shifted points, the 7 blocklisted small-
    order encodings with both sign bits, non-canonical y (p .. 2^255 - 1), x = 0
    with the sign bit set, and y that are on no curve point"""
    r = random.Random(53)
    enc = list(base_points)
    enc += [bytes(b[:31]) + bytes([b[31] ^ 0x80]) for b in base_points[:8]]
    tors = torsion_points()
    enc += [ed_encode(ed_add(ed_decode(b), t)) for b in base_points[:4] for t in tors]
    small = [0, 1, P - 1, P, P + 1] + list(ORDER8_Y)
    enc += [(y | s << 255).to_bytes(32, "little") for y in small for s in (0, 1)]
    enc += [(y | s << 255).to_bytes(32, "little") for y in range(P, 2**255) for s in (0, 1)]
    enc += [ed_encode(t) for t in tors]
    enc += [(r.randrange(2**256)).to_bytes(32, "little") for _ in range(200)]
    return enc


def family_ge_frombytes(run, base_points):
    """ge_is_canonical, has_small_order and ge_frombytes_negate (-P as reduced
    limbs, Z = 1, T = X Y) against the curve equation in Python integers"""
    enc = ge_frombytes_encodings(base_points)
    out = np.ascontiguousarray(run("ge_frombytes", np.array([list(b) for b in enc], np.uint8))).view(np.int32).tolist()
    small = {0, 1, P - 1, P, P + 1} | set(ORDER8_Y)
    n_ok = 0
    for b, o in zip(enc, out):
        v = int.from_bytes(b, "little")
        y, sign = v & (2**255 - 1), v >> 255
        assert o[0] == int(y < P), b.hex()
        assert o[1] == int(y in small), b.hex()
        yy = y % P
        u, w = (yy * yy - 1) % P, (D * yy * yy + 1) % P
        x2 = u * pow(w, P - 2, P) % P
        on_curve = x2 == 0 or pow(x2, (P - 1) // 2, P) == 1
        assert o[2] == int(on_curve), b.hex()
        if not on_curve:
            continue
        n_ok += 1
        X, Y, Z, T = (o[3 + 10 * k:13 + 10 * k] for k in range(4))
        assert all(out_ok(c) for c in (X, Y, Z, T)), b.hex()
        x = val(X) % P
        assert w * x * x % P == u and val(Y) % P == yy and val(Z) % P == 1 and val(T) % P == x * yy % P, b.hex()
        # -P: the x returned has the parity the sign bit does NOT ask for (x = 0 has only one)
        assert x == 0 or (x & 1) != sign, b.hex()
    assert n_ok >= len(base_points) + 100


# -------------------------------------------------------- the quad arithmetic
# References: each formula as a polynomial map on field elements, written from
# the extended-coordinate formulas (dbl-2008-hwcd, add-2008-hwcd-3 against a
# cached addend), not from the lanes' data movement.
def ref_quad_dbl(p):
    X, Y, Z, _ = p
    XX, YY, B, A = X * X, Y * Y, 2 * Z * Z, (X + Y) ** 2
    Y1, Z1 = YY + XX, YY - XX
    X1, T1 = A - Y1, B - Z1
    return [X1 * T1 % P, Y1 * Z1 % P, Z1 * T1 % P, X1 * Y1 % P]


def ref_quad_cached(p, neg=0):
    X, Y, Z, T = p
    c = [(Y + X) % P, (Y - X) % P, 2 * D * T % P, Z % P]
    return [c[1], c[0], -c[2] % P, c[3]] if neg else c


def ref_quad_add(p, e):
    X, Y, Z, T = p
    YpX, YmX, T2d, Z2 = e
    A, B, C, Dd = (Y + X) * YpX, (Y - X) * YmX, T * T2d, 2 * Z * Z2
    E, F, G, H = A - B, Dd - C, Dd + C, A + B
    return [E * F % P, G * H % P, F * G % P, E * H % P]


# The lanes' data movement as written in edv_quad_math.h (quad_perm indices,
# lane masks, the shift on lane 3), on any values with + - * (Python integers,
# or Mag below for the limb bounds): lane q of the result is coordinate q.
def _perm(v, idx):
    return [v[i] for i in idx]


QUAD_ADD_PERMS = {"x": (0, 0, 0, 0), "u": (1, 1, 3, 2), "uu0": (0, 0, 3, 0), "uu1": (1, 1, 2, 1),
                  "vv0": (3, 3, 3, 0), "vv1": (2, 2, 2, 1)}


def mirror_quad_add(p, e, mul=lambda a, b: a * b, perms=QUAD_ADD_PERMS):
    x0 = _perm(p, perms["x"])
    x = [x0[0], -x0[1], 0 * x0[2], 0 * x0[3]]                       # X | -X | 0 | 0 (m01, s1)
    u = [a + b for a, b in zip(_perm(p, perms["u"]), x)]              # Y+X | Y-X | T | Z
    r = [mul(u[i], e[i]) for i in range(4)]
    r[3] = 2 * r[3]                                                   # sh3
    s03, s02 = (-1, 1, 1, -1), (-1, 1, -1, 1)
    uu = [a + s * b for a, b, s in zip(_perm(r, perms["uu0"]), _perm(r, perms["uu1"]), s03)]
    vv = [a + s * b for a, b, s in zip(_perm(r, perms["vv0"]), _perm(r, perms["vv1"]), s02)]
    return [mul(uu[i], vv[i]) for i in range(4)]


def mirror_quad_dbl(p, mul=lambda a, b: a * b, sq=lambda a, sh: (a * a) << sh):
    y = _perm(p, (1, 1, 1, 1))
    y3 = [0 * y[0], 0 * y[1], 0 * y[2], y[3]]                         # Y on lane 3 (m3)
    u = [a + b for a, b in zip(_perm(p, (0, 1, 2, 0)), y3)]           # X | Y | Z | X + Y
    r = [sq(u[i], int(i == 2)) for i in range(4)]                     # sh2
    a0, a1 = _perm(r, (0, 0, 0, 0)), _perm(r, (1, 1, 1, 1))
    S = [b + a for a, b in zip(a0, a1)]
    Dm = [b - a for a, b in zip(a0, a1)]
    X1 = [a - b for a, b in zip(_perm(r, (3, 3, 3, 3)), S)]
    T1 = [a - b for a, b in zip(_perm(r, (2, 2, 2, 2)), Dm)]
    uu = [X1[0], S[1], Dm[2], X1[3]]                                  # fsel(m1, S, fsel(m2, D, X1))
    vv = [T1[0], Dm[1], T1[2], S[3]]                                  # fsel(m1, D, fsel(m3, S, T1))
    return [mul(uu[i], vv[i]) for i in range(4)]


class Mag:
    """Per-limb magnitude bound of a limb vector (|f_i| <= m_i)."""

    def __init__(self, m):
        self.m = list(m)

    def __add__(self, o):
        return Mag(a + b for a, b in zip(self.m, o.m))

    __sub__ = __add__

    def __neg__(self):
        return self

    def __rmul__(self, k):  # 0 (masked out), +-1 (sign), 2 (the shift by one)
        return Mag(abs(k) * a for a in self.m)

    def ratio(self):
        return max(a / b for a, b in zip(self.m, BOUND))


def quad_bounds():
    """Pushes the reduced bound RED through stages A and B of quad_dbl and
    quad_add as written; -> the largest operand handed to fe_mul / fe_sq_cols,
    as a fraction of BOUND, per operand.  fe_mul / fe_sq / fe_sq2 return RED for
    operands inside BOUND (family_fe_mul_sq proves that); fe_sq_shift's shifted
    columns are fe_sq2's columns, so it returns RED too."""
    seen = {}

    def mul(tag):
        def f(a, b):
            for k, v in ((tag + " lhs", a), (tag + " rhs", b)):
                seen[k] = max(seen.get(k, 0), v.ratio())
            return Mag(RED)
        return f

    def sq(a, sh):
        seen["dbl stage A"] = max(seen.get("dbl stage A", 0), a.ratio())
        return Mag(RED)

    red = [Mag(RED) for _ in range(4)]
    stage = iter(("add stage A", "add stage A", "add stage A", "add stage A",
                  "add stage B", "add stage B", "add stage B", "add stage B"))
    mirror_quad_add(red, red, mul=lambda a, b: mul(next(stage))(a, b))
    mirror_quad_dbl(red, mul=mul("dbl stage B"), sq=sq)
    return seen


def quad_limb_cases(n_vec, n, extra=()):
    """n cases of n_vec coordinates' limb vectors inside RED: a third all-extreme
    (every limb at +-RED or one inside, random signs), then every uniform-sign
    pattern per coordinate (all limbs of a coordinate +RED or -RED: the sums
    Y + X, A + B, D + C at their largest), then `extra`, the rest random"""
    r = random.Random(61 + n_vec)
    cases = [[red_limbs(r, extreme=True) for _ in range(n_vec)] for _ in range(n // 3)]
    for bits in range(min(2**n_vec, 256)):
        cases.append([[RED[i] * (-1 if (bits >> k) & 1 else 1) for i in range(10)] for k in range(n_vec)])
    cases += [list(c) for c in extra]
    while len(cases) < n:
        cases.append([red_limbs(r) for _ in range(n_vec)])
    return cases


IDENT_POINT = [[0] * 10, [1] + [0] * 9, [1] + [0] * 9, [0] * 10]             # X = 0 | Y = 1 | Z = 1 | T = 0
IDENT_CACHED = [[1] + [0] * 9, [1] + [0] * 9, [0] * 10, [1] + [0] * 9]       # YpX = 1 | YmX = 1 | T2d = 0 | Z = 1
QUAD_N = 3000


def _vals(c):
    return [val(f) for f in c]


def _check_quad(op, cases, got, want):
    for c, g, w in zip(cases, got, want):
        for q in range(4):
            assert val(g[q]) % P == w[q] % P, (op, "coordinate", q, c)
            assert out_ok(g[q]), (op, "bound", q, c, g[q])


def family_quad_sq_shift(run):
    """fe_sq_shift: f^2 2^sh per lane, sh in {0, 1} in every pattern over the quad"""
    r = random.Random(71)
    cases = [[rand_limbs(r, extreme=(it % 3 == 0)) for _ in range(4)] for it in range(QUAD_N)]
    shs = [[(it >> q) & 1 for q in range(4)] for it in range(QUAD_N)]
    rows = [[w for f, s in zip(c, sh) for w in f + [s]] for c, sh in zip(cases, shs)]
    got = pl.unpack_limbs(run("quad_sq_shift", pl.pack_words(rows)))
    want = [[val(f) ** 2 << s for f, s in zip(c, sh)] for c, sh in zip(cases, shs)]
    _check_quad("quad_sq_shift", list(zip(cases, shs)), got, want)


def family_quad_poly(run):
    """quad_dbl, quad_add, quad_cached, quad_cached_signed as polynomial maps on
    arbitrary field elements at the limb extremes the callers reach (RED, all
    sign patterns; the identity constants; fe_d2()): every output coordinate
    mod p against the formula in Python integers, and the output bound"""
    d2 = [D2_LIMBS] * 4
    pts = quad_limb_cases(4, QUAD_N, extra=[IDENT_POINT, d2, [[-x for x in D2_LIMBS]] * 4])
    got = pl.unpack_limbs(run("quad_dbl", pl.pack_limbs(pts)))
    _check_quad("quad_dbl", pts, got, [ref_quad_dbl(_vals(c)) for c in pts])
    got = pl.unpack_limbs(run("quad_cached", pl.pack_limbs(pts)))
    _check_quad("quad_cached", pts, got, [ref_quad_cached(_vals(c)) for c in pts])
    negs = [-(i & 1) for i in range(len(pts))]
    rows = [[w for f in c for w in f] + [n] for c, n in zip(pts, negs)]
    got = pl.unpack_limbs(run("quad_cached_signed", pl.pack_words(rows)))
    _check_quad("quad_cached_signed", list(zip(pts, negs)), got,
                [ref_quad_cached(_vals(c), n) for c, n in zip(pts, negs)])
    extra = [IDENT_POINT + IDENT_CACHED, IDENT_POINT + d2, d2 + IDENT_CACHED, d2 + d2]
    extra += [c[:4] + IDENT_CACHED for c in pts[:50]] + [IDENT_POINT + c[:4] for c in pts[:50]]
    adds = quad_limb_cases(8, QUAD_N + 300, extra=extra)
    got = pl.unpack_limbs(run("quad_add", pl.pack_limbs(adds)))
    _check_quad("quad_add", adds, got, [ref_quad_add(_vals(c[:4]), _vals(c[4:])) for c in adds])


def signed_limbs(x):
    """the centred limb vector of x mod p: |l_i| <= 2^25 (even), 2^24 (odd), + a carry (inside RED)"""
    l = limbs(x % P)
    for i in range(10):
        w = 26 if i % 2 == 0 else 25
        if l[i] >= (1 << (w - 1)):
            l[i] -= 1 << w
            if i < 9:
                l[i + 1] += 1
            else:
                l[0] += 19  # 2^255 = 19
    assert val(l) % P == x % P and out_ok(l)
    return l


def extended(r, pt, rand_t=False):
    """affine (x, y) -> X Y Z T limb vectors with a random Z (T = X Y / Z, or garbage)"""
    x, y = pt
    z = r.randrange(1, P)
    t = r.randrange(P) if rand_t else x * y * z % P
    return [signed_limbs(v) for v in (x * z % P, y * z % P, z, t)]


def affine(c):
    X, Y, Z, T = (val(f) % P for f in c)
    zi = pow(Z, P - 2, P)
    assert Z and T * Z % P == X * Y % P, c
    return X * zi % P, Y * zi % P


def quad_point_cases(base_points):
    """Pairs of curve points (affine) for P + Q: [k]B, torsion-shifted [k]B,
    every torsion point, the identity on either side, P + (-P), P + P"""
    pts = [ed_decode(b) for b in base_points]
    tors = torsion_points()
    mixed = [ed_add(p, t) for p in pts[:6] for t in tors[1:]]
    pool = pts + mixed + tors
    r = random.Random(67)
    pairs = [(r.choice(pool), r.choice(pool)) for _ in range(600)]
    pairs += [(p, (0, 1)) for p in pool] + [((0, 1), p) for p in pool]
    pairs += [(p, ((P - p[0]) % P, p[1])) for p in pool]              # P + (-P)
    pairs += [(p, p) for p in pool]                                   # 2P through the addition
    pairs += [(a, b) for a in tors for b in tors]
    return pool, pairs


def family_quad_points(run, base_points):
    """The quad formulas on curve points against the affine group law (ed_add):
    quad_add(P, cached(Q)) with cached(Q) from Python and from quad_cached /
    quad_cached_signed on the device, quad_dbl with a garbage input T; the
    result's T Z = X Y"""
    pool, pairs = quad_point_cases(base_points)
    r = random.Random(73)
    # doubling: T is ignored on input
    ext = [extended(r, p, rand_t=True) for p in pool]
    got = pl.unpack_limbs(run("quad_dbl", pl.pack_limbs(ext)))
    for p, g in zip(pool, got):
        assert affine(g) == ed_add(p, p), ("quad_dbl", p)
        assert all(out_ok(f) for f in g)
    # addition, the addend's cached form from Python
    ext_p = [extended(r, a) for a, _ in pairs]
    ext_q = [extended(r, b) for _, b in pairs]
    cq = [[signed_limbs(v) for v in ref_quad_cached(_vals(c))] for c in ext_q]
    got = pl.unpack_limbs(run("quad_add", pl.pack_limbs([a + b for a, b in zip(ext_p, cq)])))
    for (a, b), g in zip(pairs, got):
        assert affine(g) == ed_add(a, b), ("quad_add", a, b)
        assert all(out_ok(f) for f in g)
    # P - Q: the device's own signed cached form fed back into the device's addition
    rows = [[w for f in c for w in f] + [-1] for c in ext_q]
    cneg = pl.unpack_limbs(run("quad_cached_signed", pl.pack_words(rows)))
    got = pl.unpack_limbs(run("quad_add", pl.pack_limbs([a + b for a, b in zip(ext_p, cneg)])))
    for (a, b), g in zip(pairs, got):
        assert affine(g) == ed_add(a, ((P - b[0]) % P, b[1])), ("quad_add of -Q", a, b)


# ------------------------------------------------------- the signer's arithmetic
# sign_one (edv_verify_core.h) is sc_muladd, two scalarmult_base walks over the
# comb table (recode8 digits, ge_precomp_cneg) and ge_p3_tobytes.
SC_EDGES = [0, 1, 2, L - 1, L, L + 1, 2**252, 2**255 - 8, M256]     # 2^255 - 8: the largest clamped scalar


def sc_muladd_cases():
    """(a, b, c) below 2^256: every triple over SC_EDGES; all words 0xffffffff
    (the largest column sum: the 96-bit accumulator's top word at its maximum,
    and the carry above 2^32 that must survive into the next column); a = 2^(32
    i) - 1, b = 2^(32 j) - 1 with c = 0 and c = 2^256 - 1 (the carries of one
    column at a time); a b + c = 0 (mod L) by construction; 2,000 random
    triples; the signer's shape (h < L, a clamped, r < L)"""
    r = random.Random(91)
    cases = [(a, b, c) for a in SC_EDGES for b in SC_EDGES for c in SC_EDGES]
    cases.append((M256, M256, M256))
    cases += [(2**(32 * i) - 1, 2**(32 * j) - 1, c) for i in range(1, 9) for j in range(1, 9) for c in (0, M256)]
    for _ in range(100):
        a, b = r.randrange(2**256), r.randrange(2**256)
        c = -a * b % L
        cases += [(a, b, c), (a, b, c + L * r.randrange(1, 15))]
    cases += [(0, r.randrange(2**256), 0), (L, r.randrange(2**256), L), (r.randrange(2**256), 8 * L, 15 * L)]
    cases += [(r.randrange(2**256), r.randrange(2**256), r.randrange(2**256)) for _ in range(2000)]
    for _ in range(300):
        clamped = (r.randrange(2**256) & (2**255 - 8) & ~(1 << 255)) | (1 << 254)
        cases.append((r.randrange(L), clamped, r.randrange(L)))
    assert all(0 <= v < 2**256 for t in cases for v in t)
    return cases


def family_sc_muladd(run):
    """sc_muladd: out == (a b + c) mod L and out < L.  -> the number of cases"""
    cases = sc_muladd_cases()
    out = pl.unpack_ints(run("sc_muladd", pl.pack_ints(cases, 32)), 32)
    assert len(out) == len(cases)
    for (a, b, c), o in zip(cases, out):
        assert o[0] < L and o[0] == (a * b + c) % L, ("sc_muladd", hex(a), hex(b), hex(c), hex(o[0]))
    return len(cases)


def py_recode8(k):
    """the unique digits d_i in [-128, 127] (i < 31), d_31 >= 0, with sum d_i 256^i == k"""
    out = []
    for _ in range(31):
        d = k & 255
        if d >= 128:
            d -= 256
        out.append(d)
        k = (k - d) >> 8
    return out + [k]


def recode8_values():
    """scalars below 2^253: the CPU tests' recoding values; 0x7f and 0x80 alone
    in every byte position; 0x80 repeated (a carry through all 31 lower digits);
    0x7f...7f80; 0xff... ; 2^253 - 1"""
    vals = recoding_values()
    vals += [b << (8 * i) for i in range(32) for b in (0x7f, 0x80)]
    vals += [int("80" * 31, 16), int("80" * 31, 16) | 0x10 << 248, int("7f" * 30 + "80", 16),
             int("1f" + "7f" * 30 + "80", 16), int("ff" * 31, 16), int("1f" + "ff" * 31, 16), 2**253 - 1, 2**253 - 2**248]
    return [v for v in vals if 0 <= v < 2**253]


def family_recode8(run):
    """recode8: every digit in [-128, 127], the top one >= 0, sum d_i 256^i == s.  -> the number of cases"""
    vals = recode8_values()
    out = np.ascontiguousarray(run("recode8", pl.pack_ints([[v] for v in vals], 32))).view(np.uint32).tolist()
    for v, o in zip(vals, out):
        d = signed_digits(o, 8)
        assert len(d) == 32 and all(-128 <= x <= 127 for x in d) and d[31] >= 0, hex(v)
        assert sum(x << (8 * i) for i, x in enumerate(d)) == v, hex(v)
        assert d == py_recode8(v), hex(v)
    return len(vals)


def scalarmult_base_digit_cases():
    """Signed radix-256 digit vectors (top digit >= 0, value in [0, 2^253)), so
    the walk's table index and sign are chosen per row: for each row one
    non-zero digit of +1, +127 (row 31: +31, the largest below 2^253), -1, -127
    and -128 (a negative one under +1 in the next row, and in row 31); every
    digit -128 under a top digit of 1; every digit +127; alternating neighbours
    at the two extremes"""
    cases = []
    for i in range(32):
        for d in (1, 127, -1, -127, -128):
            if d > 0:
                v = [0] * 32
                v[i] = d if i < 31 else min(d, 31)
                cases.append(v)
            elif i < 31:
                for j in sorted({i + 1, 31}):
                    v = [0] * 32
                    v[i], v[j] = d, 1
                    cases.append(v)
    cases.append([-128] * 31 + [1])
    cases += [[127] * 31 + [t] for t in (0, 1, 31)]
    cases += [[127 if i % 2 == 0 else -128 for i in range(31)] + [1],
              [-128 if i % 2 == 0 else 127 for i in range(31)] + [1],
              [-127 if i % 2 == 0 else 127 for i in range(31)] + [31],
              [-1] * 31 + [1], [-128] * 31 + [31]]
    return cases


@functools.lru_cache(maxsize=None)
def scalarmult_base_cases():
    """-> (k, digits) per case and the expected affine points by Python
    double-and-add from B (computed once per process)"""
    import stage_cases as sc
    r = random.Random(93)
    digs = scalarmult_base_digit_cases()
    ks = [sum(d << (8 * i) for i, d in enumerate(v)) for v in digs]
    ks += [0, 1, L - 1, L, L + 1, 2**252, 2**253 - 1] + [r.randrange(2**253) for _ in range(300)]
    assert all(0 <= k < 2**253 for k in ks)
    digs = digs + [py_recode8(k) for k in ks[len(digs):]]
    assert all(py_recode8(k) == d for k, d in zip(ks, digs))
    assert sum(1 for d in digs if -128 in d) >= 70 and any(not any(d) for d in digs)
    B = ed_decode(int.to_bytes(4 * pow(5, P - 2, P) % P, 32, "little"))
    want = sc.affine_all([sc.double_and_add(k, B) for k in ks])
    return ks, digs, want


def family_scalarmult_base(run):
    """scalarmult_base over the build's own comb table: the digits recode8 makes
    are the chosen ones; (X / Z, Y / Z) is [k]B by the oracle's fixed-base
    multiplication of k mod L and by Python double-and-add; T Z == X Y; every
    limb inside RED (fe_mul's output bound); ge_p3_tobytes of the point is the
    oracle's encoding.  -> the number of cases"""
    import oracle_lib as orc
    ks, digs, want = scalarmult_base_cases()
    packed = pl.pack_ints([[k] for k in ks], 32)
    got_d = np.ascontiguousarray(run("recode8", packed)).view(np.uint32).tolist()
    out = np.ascontiguousarray(run("scalarmult_base", packed))
    pts = pl.unpack_limbs(out[:, :160])
    for k, d, gd, w, c, enc in zip(ks, digs, got_d, want, pts, out[:, 160:]):
        assert signed_digits(gd, 8) == d, ("recode8", hex(k))
        assert all(out_ok(f) for f in c), ("limb bound", hex(k), c)
        ref = orc.scalarmult_base((k % L).to_bytes(32, "little"))
        assert affine(c) == w == ed_decode(ref), ("scalarmult_base", hex(k), d)
        assert enc.tobytes() == ref, ("ge_p3_tobytes", hex(k))
    return len(ks)


def ge_p3_tobytes_cases(base_points):
    """(affine point, X Y Z T limb vectors): [k]B (`base_points`: encodings) and
    the eight torsion points (x = 0: the identity and the point of order 2, whose
    y is p - 1; x odd and even), each with Z = 1, a random Z, Z's limbs at
    +-RED with the other coordinates' limbs pushed outwards, and every
    coordinate of such a representation multiplied through by one field
    element (2, p - 1: every coordinate negated, random)"""
    import stage_cases as sc
    r = random.Random(97)
    pts = [ed_decode(b) for b in base_points] + torsion_points()
    assert {(0, 1), (0, P - 1)} <= set(pts) and {p[0] & 1 for p in pts if p[0]} == {0, 1}
    cases = []
    for pt in pts:
        reps = [[signed_limbs(v) for v in (pt[0], pt[1], 1, pt[0] * pt[1] % P)], extended(r, pt)]
        for mode in ("scaled", "bound", "bound"):
            w = sc.ext_limbs(r, pt, mode)
            reps.append([w[10 * q:10 * q + 10] for q in range(4)])
        for lam in (2, P - 1, r.randrange(2, P - 1)):
            scaled = [sc.push_to_red(signed_limbs(val(f) * lam)) for f in reps[r.randrange(len(reps))]]
            assert all(abs(v) <= RED[i] for f in scaled for i, v in enumerate(f))
            reps.append(scaled)
        cases += [(pt, c) for c in reps]
    return cases


def family_ge_p3_tobytes(run, base_points):
    """ge_p3_tobytes: the canonical encoding (y, x's parity in bit 255) of the
    affine point, whatever the representation.  -> the number of cases"""
    cases = ge_p3_tobytes_cases(base_points)
    for pt, c in cases:
        assert affine(c) == pt
    out = run("ge_p3_tobytes", pl.pack_limbs([c for _, c in cases]))
    for (pt, c), o in zip(cases, out):
        assert o.tobytes() == ed_encode(pt), ("ge_p3_tobytes", pt, c)
    return len(cases)
