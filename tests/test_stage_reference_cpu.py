"""The stage cases and their Python checkers (stage_cases.py) on the CPU build
of the headers behind the kernels' state layout (libedv_hostcheck.so:
hc_stage_prep runs prep_one / prep_point / prep_rpoint per request,
hc_stage_main runs main_one on an injected state): proves the batch, the
chosen states, the packing and the checkers here, before the same families
run on the product's kernels (test_gpu_stage_device.py).  The construction of
the chosen states is itself checked by plain double-and-add, and every checker
is shown to raise on a deliberately wrong value."""
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
