#!/usr/bin/env python3
"""Writes indy-plenum_amd/csrc/edv_selftest_cases.h, the known answers of
edv_self_test, from the committed fixtures: RFC 8032 section 7.1 vectors 1-3
(tests/golden/rfc8032_7_1.json, re-derived here from their seeds) and, from
tests/golden/ed25519_golden.bin (verdicts by libsodium 1.0.18), of each
category below the case with the shortest message that is rejected by the
category's own rule and by no earlier one.  Every case is checked against the
oracle before it is written."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import golden_io  # noqa: E402
import oracle_lib as orc  # noqa: E402

OUT = os.path.join(ROOT, "indy-plenum_amd", "csrc", "edv_selftest_cases.h")
MSG_MAX = 32
# (golden category, verdict, rule name, what it exercises)
PICKS = [
    ("s_plus_kl", 0, "kRuleScalar", "V2: S >= L (S + k L)"),
    ("small_order_r", 0, "kRuleSmallR", "V3: R of small order"),
    ("small_order_r_eq_holds", 0, "kRuleSmallR", "V3: R of small order although the equation holds"),
    ("noncanon_a", 0, "kRuleNoncanonA", "V4: A not canonical (y >= p)"),
    ("small_order_a", 0, "kRuleSmallA", "V4: A of small order"),
    ("offcurve_a", 0, "kRuleOffCurveA", "V5: A does not decompress"),
    ("flip_msg", 0, "kRuleEquation", "a well-formed signature over a changed message"),
    ("mixed_order_a", 1, "kRuleNone", "A of mixed order that libsodium accepts"),
]


def first_rule(sig, pk, msg):
    """The check of oref_verify_detached (libsodium's order) that rejects the case."""
    import ctypes
    lib = orc.load()
    for k in ("oref_sc_is_canonical", "oref_has_small_order", "oref_ge_is_canonical"):
        getattr(lib, k).argtypes = [ctypes.c_char_p]
    if (sig[63] & 0xF0) and not lib.oref_sc_is_canonical(sig[32:]):
        return "kRuleScalar"
    if lib.oref_has_small_order(sig[:32]):
        return "kRuleSmallR"
    if not lib.oref_ge_is_canonical(pk):
        return "kRuleNoncanonA"
    if lib.oref_has_small_order(pk):
        return "kRuleSmallA"
    if orc.point_add(pk, pk) is None:
        return "kRuleOffCurveA"
    return "kRuleNone" if orc.verify(sig, msg, pk) else "kRuleEquation"


def rows(b):
    return "\n".join("     " + ", ".join("0x%02x" % x for x in b[i:i + 16]) + "," for i in range(0, len(b), 16))


def main():
    cases = []
    with open(os.path.join(golden_io.GOLDEN, "rfc8032_7_1.json")) as f:
        for k, v in enumerate(json.load(f)["vectors"]):
            seed, pk, msg, sig = (bytes.fromhex(v[x]) for x in ("seed", "pk", "msg", "sig"))
            opk, osk = orc.keypair(seed)
            assert opk == pk and orc.sign(msg, osk) == sig, "RFC 8032 vector %d" % (k + 1)
            cases.append((sig, pk, msg, 1, "kRuleNone", "RFC 8032 7.1 TEST %d" % (k + 1)))
    recs = golden_io.load_ed25519_golden()
    cats = golden_io.golden_meta()["categories"]
    for cat, verdict, rule, what in PICKS:
        # the shortest message among the category's cases that no earlier check rejects
        best = min((len(m), i) for i, (v, c, sg, p, m) in enumerate(recs)
                   if cats[c] == cat and v == verdict and first_rule(sg, p, m) == rule)
        v, _c, sig, pk, msg = recs[best[1]]
        cases.append((sig, pk, msg, v, rule, "%s (golden case %d, %s)" % (what, best[1], cat)))
    for sig, pk, msg, v, _rule, what in cases:
        assert len(msg) <= MSG_MAX, what
        assert orc.verify(sig, msg, pk) == bool(v), what
    body = []
    for sig, pk, msg, v, rule, what in cases:
        body.append("    // %s\n    {{\n%s\n     },\n     {\n%s\n     },\n     {\n%s\n     },\n     %d, %d, %s},"
                    % (what, rows(sig), rows(pk), rows(msg + bytes(MSG_MAX - len(msg))), len(msg), v, rule))
    with open(OUT, "w") as f:
        f.write(HEAD % {"n": len(cases), "m": MSG_MAX} + "\n".join(body) + TAIL)
    print("%s: %d cases" % (OUT, len(cases)))


HEAD = """// edv_selftest_cases.h -- the known answers of edv_self_test (include/edv.h), as
// data: plain C++, seen by the library and by the CPU test harness alike.
// Written by tools/make_selftest_cases.py from tests/golden/ (RFC 8032 section
// 7.1 vectors 1-3 and cases of ed25519_golden.bin, whose verdicts are libsodium
// 1.0.18's); do not edit by hand.
#pragma once
#include <stdint.h>

namespace edv {

// The rule of libsodium's crypto_sign_ed25519_verify_detached a case is there
// for (SURVEY.md section 8a): the one that rejects it, or none.
enum SelfTestRule {
  kRuleNone = 0,       // accepted
  kRuleScalar = 2,     // V2: S >= L
  kRuleSmallR = 3,     // V3: R in the small-order blocklist
  kRuleNoncanonA = 4,  // V4: A not canonical
  kRuleSmallA = 5,     // V4: A in the small-order blocklist
  kRuleOffCurveA = 6,  // V5: A does not decompress
  kRuleEquation = 7,   // every check passes, the equation does not hold
};

struct SelfTestCase {
  uint8_t sig[64];
  uint8_t pk[32];
  uint8_t msg[%(m)d];  // the first mlen bytes
  uint8_t mlen;
  uint8_t accept;  // libsodium's verdict
  uint8_t rule;
};

constexpr int kSelfTestCases = %(n)d;
inline const SelfTestCase* selftest_cases() {
  static const SelfTestCase k[kSelfTestCases] = {
"""
TAIL = """
  };
  return k;
}

}  // namespace edv
"""

if __name__ == "__main__":
    main()
