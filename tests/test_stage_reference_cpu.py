"""The stage cases and their Python checkers (stage_cases.py) on the CPU build
of the headers behind the kernels' state layout (libedv_hostcheck.so:
hc_stage_prep runs prep_one / prep_point / prep_rpoint per request,
hc_stage_main runs main_one on an injected state): proves the batch, the
chosen states, the packing and the checkers here, before the same families
run on the product's kernels (test_gpu_stage_device.py).  The construction of
the chosen states is itself checked by plain double-and-add, and every checker
is shown to raise on a deliberately wrong value.  The same for the latency
kernels' families (phase-1 state out, walk on chosen phase-1 states) on the
CPU references hc_stage_latency_phase1 / hc_stage_latency_walk, before they
run on the device (test_gpu_latency_device.py).  The edge batch (the fixture
tests/golden/prep_edge_golden.json, verdicts by libsodium) goes through the
same prep and phase-1 families, and every assertion of its builder is shown
to raise on a wrong expectation."""
import numpy as np
import pytest

import stage_cases as sc
from math_cases import L

B = "host"


@pytest.mark.parametrize("table_set,buckets,split", sc.VARIANTS)
def test_prep_state(table_set, buckets, split):
    sc.family_prep(B, table_set, buckets, split)


@pytest.mark.parametrize("n", sc.PREP_SIZES[:-1])
def test_prep_state_batch_sizes(n):
    sc.family_prep_sizes(B, n)


@pytest.mark.parametrize("table_set", ("compact", "large"))
def test_split_and_bucketed_runs_write_the_joint_state(table_set):
    sc.family_seams(B, table_set)


def test_large_and_compact_sets_give_the_same_r_points():
    sc.family_sets(B)


def test_one_bucket_keeps_the_identity_order():
    sc.family_one_bucket(B)


def test_round_trip_matches_the_oracle():
    sc.family_round_trip(B, "compact", True, False)
    sc.family_round_trip(B, "large", False, True)


def test_chosen_state():
    assert sc.check_chosen(B) >= 1500


def test_chosen_state_with_a_permutation():
    sc.check_chosen(B, permute=True)


@pytest.mark.parametrize("n", (1, 63, 65, 257))
def test_chosen_state_partial_waves(n):
    sc.check_chosen(B, n=n, cap=n)
    sc.check_chosen(B, n=n, cap=n, permute=True)


def test_chosen_state_families_are_all_there():
    cases = sc.chosen_cases()
    live = [c for c in cases if not c.get("dead")]
    for which in "ab":
        for accept in (0, 1):
            assert {c["own"] for c in live if c["tag"].startswith("count %s " % which) and c["expect"] == accept} == \
                set(range(1, 65))
    tags = {c["tag"].rstrip("0123456789 ") for c in live}
    assert {"spike", "one window", "count word above own", "digits a", "digits b", "carry top a", "carry top b",
            "a =", "sign", "sign flipped", "small-order result", "scaled", "bound", "tail"} <= tags, tags
    assert any(c["word"] > c["own"] for c in live) and any(c["word"] == 64 and c["own"] < 30 for c in live)
    assert {c["alive"] for c in cases} >= {(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)}
    # digits: a run of -8 across the whole scalar, a top window that is only the carry
    d = sc.recode4(int("7" * 62 + "8", 16))[0]
    assert d[:63] == [-8] * 63 and d[63] == 1
    d = sc.recode4(0xF8 << 240)[0]
    assert d[60:63] == [-8, 0, 1] and sc.windows(d) == 63


def test_chosen_state_construction_by_double_and_add():
    assert sc.check_construction() >= 200


def test_recode_mirror():
    import math_cases as mc
    for s in sc.special_scalars() + mc.recoding_values()[:300]:
        d, words = sc.recode4(s)
        assert sum(x << (4 * k) for k, x in enumerate(d)) == s and all(-8 <= x <= 7 for x in d) and d[63] >= 0
        assert mc.signed_digits(words, 4) == d


@pytest.mark.parametrize("table_set", ("comb", "compact", "large"))
def test_tables(table_set):
    assert sc.family_tables(B, table_set) == {"comb": 32 * 129, "compact": 16 * 2570, "large": 12 * 2570}[table_set]


# ---- the checkers' own tests: a wrong value makes each of them raise
def _copy(st):
    return {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in st.items()}


def _raises(fn):
    with pytest.raises(AssertionError):
        fn()


def test_prep_checker_rejects_wrong_states():
    b, n = sc.prep_batch(), 257
    good = sc.prep_state(B, n, "compact", True, False)
    sc.check_prep_state(b, n, good, True)
    perm = good["perm"].tolist()
    ok_slot = next(j for j in range(n) if all(b["reqs"][perm[j]]["sides"]))
    dead_req = next(i for i in range(n) if not all(b["reqs"][i]["sides"]))

    def tampered(edit):
        st = _copy(good)
        edit(st)
        _raises(lambda: sc.check_prep_state(b, n, st, True))

    def set_(key, idx, value):
        def edit(st):
            st[key][idx] = value
        return edit

    tampered(set_("alive", (0, ok_slot), 0))
    tampered(set_("alive", (2, ok_slot), 0))
    tampered(set_("accept", perm[ok_slot], 1))                               # the sentinel overwritten
    tampered(set_("accept", dead_req, sc.SENT))                              # a rejected request left unmarked
    tampered(set_("dig", (0, ok_slot), int(good["dig"][0, ok_slot]) ^ 16))   # a digit of a
    tampered(set_("dig", (8, ok_slot), int(good["dig"][8, ok_slot]) ^ 1))    # b even
    tampered(set_("dig", (16, ok_slot), int(good["dig"][16, ok_slot]) ^ 0x100))  # the sign
    tampered(set_("dig", (16, ok_slot), int(good["dig"][16, ok_slot]) + 1))  # the count
    tampered(set_("dig", (16, n), 0))                                        # a word past the batch
    tampered(set_("atab", (ok_slot, 40 * 3 + 1), int(good["atab"][ok_slot, 121]) + 1))
    tampered(set_("rtab", (ok_slot, 40 * 8 + 35), int(good["rtab"][ok_slot, 355]) + 1))
    tampered(set_("rtab", (ok_slot, 22), int(good["rtab"][ok_slot, 22]) + (1 << 28)))  # limb bound (and value)

    def swap_perm(st):                                                       # slots no longer hold perm[j]'s state
        j2 = next(j for j in range(n) if j != ok_slot and all(b["reqs"][perm[j]]["sides"])
                  and sc.sha_bucket(len(b["reqs"][perm[j]]["msg"])) == sc.sha_bucket(len(b["reqs"][perm[ok_slot]]["msg"])))
        st["perm"][[ok_slot, j2]] = st["perm"][[j2, ok_slot]]
    tampered(swap_perm)
    tampered(set_("perm", 0, perm[1]))                                       # not a permutation

    def entry_shift(st):                                                     # (e + 1) P stored at entry e
        st["atab"][ok_slot, 120:320] = good["atab"][ok_slot, 160:360]
    tampered(entry_shift)
    # the seams: a state that differs in one byte
    st = _copy(good)
    st["rtab"][5, 7] += 1
    assert sc.by_request(st, n) != sc.by_request(good, n)
    _raises(lambda: sc.same_rtab_points(b, n, st, good))


def test_table_checkers_reject_wrong_entries():
    pts = sc.multiples(sc.base_mult(12345))
    words = [v for pt in pts for v in sc.cached_limbs(None, pt, "affine")]
    sc.check_cached_table(words, pts, "self")
    _raises(lambda: sc.check_cached_table(words, pts[:3] + pts[4:] + pts[:1], "self"))
    _raises(lambda: sc.check_cached_table(words[:355] + [words[355] + 1] + words[356:], pts, "self"))       # T2d
    _raises(lambda: sc.check_cached_table(words[:40] + [0] * 40 + words[80:], pts, "self"))                  # Z = 0
    neg = [v for pt in pts for v in sc.cached_limbs(None, sc.neg(pt), "affine")]
    _raises(lambda: sc.check_cached_table(neg, pts, "self"))
    e = sc.read_table(B, "compact", [(3, 77)])[0]
    sc.check_precomp_entry(e, 77 << 48, "self")
    _raises(lambda: sc.check_precomp_entry(e, (77 << 48) + 1, "self"))
    _raises(lambda: sc.check_precomp_entry(e, L - (77 << 48), "self"))                                       # -P: same y
    bad = e.copy()
    bad[20] += 1
    _raises(lambda: sc.check_precomp_entry(bad, 77 << 48, "self"))


def test_main_checker_rejects_wrong_verdicts(monkeypatch):
    cases = sc.chosen_cases()
    real = sc.run_main
    for pick in (lambda c: all(c["alive"]) and c["expect"] == 1, lambda c: all(c["alive"]) and c["expect"] == 0,
                 lambda c: not all(c["alive"])):
        s = next(k for k, c in enumerate(cases) if pick(c))

        def wrong(*a, _s=s, **kw):
            acc = real(*a, **kw)
            acc[_s] = {1: 0, 0: 1, sc.SENT: 0}[int(acc[_s])]
            return acc
        monkeypatch.setattr(sc, "run_main", wrong)
        _raises(lambda: sc.check_chosen(B))
    monkeypatch.setattr(sc, "run_main", real)
    # an expected verdict is the congruences, not the construction's intent
    c = dict(next(c for c in cases if not c.get("dead") and c["expect"] == 1 and c["a"] % L))
    c["k"] = (c["k"] + 1) % L
    assert sc.expected_verdict(c) == 0


# ---- the edge batch (tests/golden/prep_edge_golden.json, verdicts by libsodium):
# the fixture, its builder's assertions and the generic checkers on the CPU
# build, before the same batch runs on the device
E = "edge"
KERNELS = ("rtl", "quad")


def test_edge_fixture_families_and_coverage():
    """The fixture as the generator promises it, and the digits the R side
    gathers: the 600 honest requests reach 1 / 0 zero digits (compact / large)
    and no digit of magnitude half; the edge batch reaches entry 0 and the
    last entry of every table of both sets."""
    b = sc.edge_batch()
    fam = [q["family"] for q in b["reqs"]]
    assert {f: fam.count(f) for f in sc.EDGE_FAMILIES} == {"s_digits": 228, "q_special": 108, "s_canonical": 22,
                                                           "accepted": 37}
    assert sc.batch_size(E) == 395 and len(b["off"]) == 396 and b["sigs"].size == 64 * 395
    assert [q["valid"] for q in b["reqs"]] == [int(f == "accepted") for f in fam]
    assert {q["sides"] for q in b["reqs"]} == {(1, 1, 1), (0, 1, 1)}
    assert sum(1 for q in b["reqs"] if 2**252 <= q["S"] < L and q["sides"][0]) >= 10
    assert [sc.digit_coverage(sc.prep_batch(), ts) for ts in ("compact", "large")] == [(1, 0), (0, 0)]
    cov = {ts: sc.digit_coverage(b, ts) for ts in ("compact", "large")}
    print("edge batch digit coverage (zero digits, digits of magnitude half):", cov)
    assert all(z >= 16 * 20 and h >= 60 for z, h in cov.values()), cov
    # the recoder: the three properties on every S of both batches, and it raises on a wrong digit
    for q in b["reqs"] + sc.prep_batch()["reqs"]:
        for ts in ("compact", "large"):
            sc.recode_sb(q["S"], ts)
    d = sc.recode_sb(2**252 + 12345, "compact")
    _raises(lambda: sc.check_recoding(2**252 + 12345, "compact", d[:3] + [d[3] + 1] + d[4:]))
    _raises(lambda: sc.check_recoding(0x8000, "compact", [0x8000] + [0] * 15))        # half is not below half
    _raises(lambda: sc.check_recoding(0x8000 << 224, "compact", [0] * 14 + [-0x8000, 0]))


@pytest.mark.parametrize("table_set,buckets,split", sc.VARIANTS)
def test_edge_prep_state(table_set, buckets, split):
    ab = sc.family_prep(B, table_set, buckets, split, batch=E)
    assert sum(1 for x in ab if x is not None) == sum(q["sides"][0] for q in sc.edge_batch()["reqs"])


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_edge_prep_state_batch_sizes(n):
    sc.family_prep_sizes(B, n, batch=E)


def test_edge_prep_seams_and_sets():
    for table_set in ("compact", "large"):
        sc.family_seams(B, table_set, batch=E)
    sc.family_sets(B, batch=E)


def test_edge_round_trip_matches_libsodium():
    got = sc.family_round_trip(B, "compact", True, False, batch=E)
    assert got == sc.family_round_trip(B, "large", False, True, batch=E)
    assert [i for i, v in enumerate(got) if v] == [i for i, q in enumerate(sc.edge_batch()["reqs"]) if q["family"] == "accepted"]


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("table_set", ("compact", "large"))
def test_edge_latency_phase1(kernel, table_set):
    for n in (1, 15, 16, 17, 33, None):
        sc.family_lat_phase1(B, kernel, table_set, n, batch=E)
    sc.family_lat_round_trip(B, kernel, table_set, batch=E)


@pytest.mark.parametrize("kernel", KERNELS)
def test_edge_latency_table_sets_give_the_same_points(kernel):
    sc.family_lat_sets(B, kernel, batch=E)


def test_edge_builder_assertions_fire():
    """Each assertion the edge batch's builder makes raises on a wrong
    expectation: a digit, a value, a range, Q's order, R's and A's order, the
    verdict, the order of the batch; and the generic checker raises on a wrong
    `sides` expectation of an edge request."""
    b = sc.edge_batch()
    reqs = b["reqs"]

    def pick(pred):
        return next(q for q in reqs if pred(q))

    def wrong(q, **want):
        _raises(lambda: sc.check_edge_intent(dict(q, want=dict(q["want"], **want))))

    q = pick(lambda q: q["kind"].startswith("s_digits: compact -half at 7,"))
    sc.check_edge_intent(q)
    wrong(q, digits={"7": -32767, "8": 1})                                # one digit expectation off by one
    wrong(q, digits={"7": -32768})                                        # the carry above it is not "other digits 0"
    wrong(q, set="large")
    wrong(q, r_mixed=1 - q["want"]["r_mixed"])
    _raises(lambda: sc.check_edge_intent(dict(q, S=q["S"] + 1)))
    q = pick(lambda q: q["want"].get("value") == "L-1")
    wrong(q, value="L-2")
    q = pick(lambda q: q["family"] == "s_canonical" and 2**252 <= q["S"] < L)
    wrong(q, lt_l=0)
    wrong(q, ge_2_252=0)
    _raises(lambda: sc.check_edge_intent(dict(q, S=q["S"] + 2**32 * 0x10000000)))
    q = pick(lambda q: q["want"].get("q_order") == 1)
    wrong(q, q_order=2)
    _raises(lambda: sc.check_edge_intent(dict(q, S=q["S"] ^ 1)))
    q = pick(lambda q: q["want"].get("q_order") == 4)
    wrong(q, q_order=8)
    q = pick(lambda q: q["want"].get("q") == "2sb")
    _raises(lambda: sc.check_edge_intent(dict(q, R=reqs[0]["R"])))
    q = pick(lambda q: "a_mixed" in q["want"])
    _raises(lambda: sc.check_edge_intent(dict(q, A=reqs[0]["A"])))
    _raises(lambda: sc.check_edge_intent(dict(q, msg=q["msg"][:-1] + bytes([q["msg"][-1] ^ 1]))))   # 8 no longer divides h
    q = pick(lambda q: q["family"] == "accepted" and q["want"]["set"] == "large")
    wrong(q, digits={k: v + 1 for k, v in q["want"]["digits"].items()})
    _raises(lambda: sc.check_edge_intent(dict(q, valid=0)))
    _raises(lambda: sc.check_edge_intent(dict(reqs[0], valid=1)))
    _raises(lambda: sc.check_edge_intent(dict(reqs[0], msg=bytes(91))))
    sc.check_edge_layout(reqs)
    _raises(lambda: sc.check_edge_layout(reqs[1:] + reqs[:1]))            # slots 62 / 63 and the last request move
    b_enc = sc.mc.ed_encode(sc.base_mult(1))
    _raises(lambda: sc.check_edge_layout([reqs[0] if x["A"] == b_enc else x for x in reqs]))               # no key B
    _raises(lambda: sc.check_edge_layout([reqs[0] if abs(sc.recode_sb(x["S"], "large")[10]) == 2**21 else x
                                          for x in reqs]))                 # the last entry of table 10 never gathered
    # a wrong `sides` expectation: the state checker raises
    n = 65
    good = sc.prep_state(B, n, "compact", False, False, E)
    sc.check_prep_state(b, n, good, False)
    i = next(i for i in range(n) if reqs[i]["family"] == "s_canonical" and reqs[i]["S"] < L)
    bad = dict(b, reqs=reqs[:i] + [dict(reqs[i], sides=(0, 1, 1))] + reqs[i + 1:])
    _raises(lambda: sc.check_prep_state(bad, n, good, False))
    i = next(i for i in range(n) if reqs[i]["want"].get("q_order") == 1)
    shifted = dict(reqs[i], rtab=sc.multiples(sc.base_mult(1)))             # Q expected to be B, not the identity
    _raises(lambda: sc.check_prep_state(dict(b, reqs=reqs[:i] + [shifted] + reqs[i + 1:]), n, good, False))
    lat = sc.lat_phase1_state(B, "rtl", n, "compact", E)
    sc.check_lat_phase1("rtl", b, n, lat)
    _raises(lambda: sc.check_lat_phase1("rtl", bad, n, lat))


# ---- the latency kernels' families (the latency probes) on the CPU references
# (hc_stage_latency_phase1 / _walk: references that prove the cases and the
# checkers, not a build of the quad code, which has none on the CPU)


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_walk_chosen_state(kernel):
    assert sc.check_lat_walk(B, kernel) >= 700


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", sc.LAT_WALK_SIZES)
def test_latency_walk_batch_sizes(kernel, n):
    sc.check_lat_sizes(B, kernel, n)


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_walk_families_are_all_there(kernel):
    slots, tally = sc.lat_cases(kernel)
    live = [c for c in slots if not c.get("dead")]
    for which in "ab":
        for accept in (0, 1):
            assert {c["own"] for c in live if c["tag"].startswith("count %s " % which) and c["expect"] == accept} == \
                set(range(1, 65))
    assert sum(tally.dropped.values()) * 50 <= sum(tally.asked.values())
    assert tally.dropped["count a"] == tally.dropped["count b"] == 0
    U = sc.LAT_UNIT[kernel]
    units = [slots[o:o + U] for o in range(0, len(slots) - len(slots) % U, U)]
    tops = {max([c["word"] for c in u if all(c["alive"])], default=0) for u in units}
    if kernel == "rtl":
        assert {0, 1, 2, 3, 4, 5, 7, 8, 9, 63, 64} <= tops
        assert {t % 4 for t in tops} == {0, 1, 2, 3}
        for d in range(9):
            assert any(c["tag"].startswith("bucket %d a" % d) for c in live)
            assert d in (0, 2, 4, 6, 8) or any(c["tag"].startswith("bucket %d b" % d) for c in live)
        assert sc.recode4(int("7" * 62 + "8", 16))[0][:63] == [-8] * 63
        assert {abs(x) for x in sc.recode4(sc.EVERY_BUCKET)[0]} == set(range(9))
    else:
        ns = sc.LAT_NS[kernel] // U
        assert any([max(c["word"] for c in u if all(c["alive"])) for u in units[o:o + ns]] == [1, 16, 33, 64]
                   for o in range(0, len(units) - ns + 1, ns) if all(any(all(c["alive"]) for c in u) for u in units[o:o + ns]))
    assert any(c["word"] > c["own"] for c in live) and len(slots) % sc.LAT_NS[kernel]
    assert {c["alive"] for c in live} >= {(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0)}
    # the spike sits at the first and at the last slot of a unit
    assert {u.index(c) for u in units for c in u if c["tag"] == "spike 64"} == {0, U - 1}
    # the three point forms, and limbs at the edge of the bound
    n, cases, dig, pt, ok = sc.lat_state(kernel)
    assert n == len(slots) and pt.shape[2] == sc.lat_slots(kernel, n)
    assert (np.abs(pt[:, 20:30].astype(np.int64)).max(axis=(0, 2)) == np.array(sc.RED)).all()


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_walk_construction_by_double_and_add(kernel):
    assert sc.check_lat_construction(kernel) >= 100


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("table_set", ("compact", "large"))
def test_latency_phase1_state(kernel, table_set):
    ab = sc.family_lat_phase1(B, kernel, table_set)
    assert sum(1 for x in ab if x is not None) >= 540


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", sc.LAT_P1_SIZES[:-1])
def test_latency_phase1_batch_sizes(kernel, n):
    sc.family_lat_phase1(B, kernel, "compact", n)
    sc.family_lat_phase1(B, kernel, "large", n)


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_table_sets_give_the_same_points(kernel):
    sc.family_lat_sets(B, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_round_trip_matches_the_oracle(kernel):
    sc.family_lat_round_trip(B, kernel)


def test_latency_checkers_reject_wrong_values(monkeypatch):
    b, n, kernel = sc.prep_batch(), 33, "rtl"
    good = sc.lat_phase1_state(B, kernel, n, "compact")
    sc.check_lat_phase1(kernel, b, n, good)
    ok_slot = next(j for j in range(n) if all(b["reqs"][j]["sides"]))
    dead = next(j for j in range(n) if not b["reqs"][j]["sides"][1])

    def tampered(key, idx, value, st=good, nn=n):
        st = _copy(st)
        st[key][idx] = value
        _raises(lambda: sc.check_lat_phase1(kernel, b, nn, st))

    tampered("ok", (0, ok_slot), 0)
    tampered("ok", (1, dead), 1)
    tampered("ok", (2, 47), 1)                                                 # a slot past the batch marked live
    tampered("accept", 3, 0)
    tampered("dig", (0, ok_slot), int(good["dig"][0, ok_slot]) ^ 16)
    tampered("dig", (16, ok_slot), int(good["dig"][16, ok_slot]) ^ 0x100)
    tampered("dig", (16, ok_slot), int(good["dig"][16, ok_slot]) + 1)
    tampered("dig", (3, 40), sc.SENT32)                                        # a word left sentinel
    tampered("dig", (3, 40), 1)                                                # digits past the batch
    tampered("pt", (0, 1, ok_slot), int(good["pt"][0, 1, ok_slot]) + 1)        # -A
    tampered("pt", (1, 35, ok_slot), int(good["pt"][1, 35, ok_slot]) + 1)      # T of -R
    tampered("pt", (2, 12, ok_slot), int(good["pt"][2, 12, ok_slot]) + 1)      # [S]B
    tampered("pt", (2, 0, ok_slot), int(good["pt"][2, 0, ok_slot]) + (1 << 28))  # limb bound
    tampered("pt", (0, 0, dead), 5)                                            # a rejected point is the identity
    tampered("pt", (2, 10, 45), 0)                                             # past the batch: the identity
    small = sc.lat_phase1_state(B, kernel, 15, "compact")                      # slot 15 repeats request 14
    tampered("dig", (1, 15), int(small["dig"][1, 15]) ^ 1, small, 15)
    tampered("pt", (2, 3, 15), int(small["pt"][2, 3, 15]) + 1, small, 15)
    neg_a = _copy(good)                                                        # +A where -A belongs
    neg_a["pt"][0, 0:10, ok_slot] *= -1
    neg_a["pt"][0, 30:40, ok_slot] *= -1
    _raises(lambda: sc.check_lat_phase1(kernel, b, n, neg_a))
    # the walk's checker: a wrong verdict, a byte written past the batch, a dead slot left unwritten
    real = sc.run_lat_walk
    nn, cases, dig, pt, ok = sc.lat_state(kernel)
    base = real(B, kernel, nn, dig, pt, ok)
    for pick, wrong_value in ((lambda s, c: all(c["alive"]) and c["expect"] == 1, 0),
                              (lambda s, c: all(c["alive"]) and c["expect"] == 0, 1),
                              (lambda s, c: s < nn and not all(c["alive"]), sc.SENT), (lambda s, c: s >= nn, 0)):
        s = next(k for k, c in enumerate(cases) if pick(k, c))

        def wrong(*a, _s=s, _v=wrong_value, **kw):
            acc = base.copy()
            acc[_s] = _v
            return acc
        monkeypatch.setattr(sc, "run_lat_walk", wrong)
        _raises(lambda: sc.check_lat_walk(B, kernel))
    monkeypatch.setattr(sc, "run_lat_walk", real)
    # the reference walk itself tells -R from R and a digit from its neighbour
    s = next(k for k, c in enumerate(cases) if all(c["alive"]) and c.get("expect") == 1 and c["a"] > 16)
    for edit in (lambda d, p: d.__setitem__((0, s), int(d[0, s]) ^ 1), lambda d, p: p.__setitem__((1, slice(0, 10), s), -p[1, 0:10, s])):
        d2, p2 = dig.copy(), pt.copy()
        edit(d2, p2)
        assert base[s] == 1 and real(B, kernel, nn, d2, p2, ok)[s] == 0
