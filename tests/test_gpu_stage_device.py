"""The seam between the batch path's two kernels, on the device: the state
edv_prep_kernel writes (digits, alive flags, both point tables, the bucket
permutation, the accept bytes it touches) read back word for word, the main
kernels (edv_main_kernel and edv_main_kernel_prio) run on chosen states no
SHA-512 output produces (every window count 1..64, carries into the top window,
runs of -8 digits, a = 0, small-order results, scaled and bound-extreme table
entries, dead lanes), and the device tables read back entry by entry.  The
stage probes of libedv_measure.so (include/edv_measure.h) launch the product's
own kernel objects; the cases and Python-integer checkers are those
test_stage_reference_cpu.py proves on the CPU build (stage_cases.py).

Measured on MI355X (gfx950), recorded in DESIGN.md section 5:
  prep state   600 slots per variant, 8 variants; 0 of 565 device (a, b) pairs
               differ from the CPU build's in each (printed by test_prep_state,
               not asserted: any pair with the lattice property is correct)
  chosen state 1,573 slots (1,183 live walks) through each main kernel
  durations    1.6 s the first chosen-state test (it builds the cases), 1.3 s
               the first prep variant (it builds the batch), 0.5-0.8 s the other
               prep variants and the table sets, the rest below 0.3 s
  edge batch   395 slots per variant (367 pass the hash side); dig, alive and
               accept equal the CPU build's byte for byte, 0 of 142,200 atab and
               of 142,200 rtab words differ in each of the 8 variants; 1.3 s the
               first variant (it builds the expected tables), 0.27-0.33 s the
               others, 0.15 s a batch size, 4.4 s the 17 edge tests"""
import numpy as np
import pytest

import stage_cases as sc

pytestmark = pytest.mark.gpu
B = "device"


def test_stage_probes_reject_bad_arguments():
    from indy_plenum_amd import edv
    m = edv.measure_lib()
    b = sc.uniform_batch(3)
    z = np.zeros(17 * sc.CAP, np.uint32)
    t = np.zeros(3 * sc.A_WORDS, np.int32)
    p = lambda a: a.ctypes.data                                                  # noqa: E731

    def prep(n=3, table_set=0, side0=0, nsides=3, flags=0, sigs=b["sigs"], dig=z, perm=z):
        return m.edv_probe_prep_state(0, None if sigs is None else p(sigs), p(b["pks"]), p(b["msgs"]), p(b["off"]), n,
                                      table_set, side0, nsides, flags, None if dig is None else p(dig), p(z), p(t),
                                      p(t), None if perm is None else p(perm), p(z), None)

    def main(n=3, cap=64, flags=0, dig=z, perm=None):
        return m.edv_probe_main_state(0, n, cap, None if dig is None else p(dig), p(z), p(t), p(t),
                                      None if perm is None else p(perm), flags, p(z))

    tj = np.array([[0, 1]], np.int32)
    out = np.zeros(32, np.int32)
    bad = [lambda: prep(sigs=None), lambda: prep(dig=None), lambda: prep(flags=1, perm=None),
           lambda: prep(n=sc.CAP + 1), lambda: prep(table_set=2), lambda: prep(table_set=-1),
           lambda: prep(nsides=0), lambda: prep(nsides=4), lambda: prep(side0=1, nsides=3), lambda: prep(side0=3, nsides=1),
           lambda: prep(side0=-1), lambda: prep(flags=2, side0=1, nsides=2), lambda: prep(flags=8),
           lambda: main(dig=None), lambda: main(n=65), lambda: main(n=3, cap=sc.CAP + 1), lambda: main(flags=8),
           lambda: main(perm=np.array([0, 1, 3], np.uint32)),
           lambda: m.edv_probe_table(0, 3, p(tj), 1, p(out)), lambda: m.edv_probe_table(0, 0, None, 1, p(out)),
           lambda: m.edv_probe_table(0, 0, p(tj), 1, None),
           lambda: m.edv_probe_table(0, 0, p(np.array([[16, 0]], np.int32)), 1, p(out)),
           lambda: m.edv_probe_table(0, 0, p(np.array([[0, 32769]], np.int32)), 1, p(out)),
           lambda: m.edv_probe_table(0, 2, p(np.array([[0, 129]], np.int32)), 1, p(out))]
    for k, call in enumerate(bad):
        assert call() == edv.EDV_E_ARG, k
        assert b"probe" in m.edv_last_error(), k
    # a live slot whose count word is above 64
    dig, alive = np.zeros((17, 64), np.uint32), np.ones((3, 64), np.uint8)
    dig[16, 1] = 65
    assert m.edv_probe_main_state(0, 3, 64, p(dig), p(alive), p(t), p(t), None, 0, p(z)) == edv.EDV_E_ARG
    # n = 0: fine, nothing launched, nothing read
    assert prep(n=0, sigs=None, dig=None) == edv.EDV_OK and main(n=0, dig=None) == edv.EDV_OK
    assert m.edv_probe_table(0, 0, None, 0, None) == edv.EDV_OK
    assert m.edv_probe_table(0, 0, p(tj), 1, p(out)) == edv.EDV_OK and out[:30].any()


@pytest.mark.parametrize("table_set,buckets,split", sc.VARIANTS)
def test_prep_state(table_set, buckets, split):
    """(the large-set variants build the 3 GiB set in the measurement library's context, once)"""
    dev = sc.family_prep(B, table_set, buckets, split)
    cpu = sc.family_prep("host", table_set, buckets, split)
    print("prep state %s: %d slots, %d of %d device (a, b) differ from the CPU build's" %
          ((table_set, buckets, split), len(dev), sum(1 for x, y in zip(dev, cpu) if x != y),
           sum(1 for x in dev if x is not None)))


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


@pytest.mark.parametrize("prio", (False, True))
def test_round_trip_matches_the_oracle_and_the_product(prio):
    from indy_plenum_amd import edv
    b = sc.prep_batch()
    got = sc.family_round_trip(B, "compact", True, False, prio)
    assert got == sc.family_round_trip(B, "large", False, True, prio)
    assert got == edv.verify_arrays(b["sigs"], b["pks"], b["msgs"], b["off"]).tolist()


@pytest.mark.parametrize("prio", (False, True))
def test_chosen_state(prio):
    print("chosen state: %d slots" % sc.check_chosen(B, prio=prio))


@pytest.mark.parametrize("prio", (False, True))
def test_chosen_state_with_a_permutation(prio):
    sc.check_chosen(B, prio=prio, permute=True)


@pytest.mark.parametrize("n", (1, 63, 65, 257))
def test_chosen_state_partial_waves(n):
    for prio in (False, True):
        sc.check_chosen(B, n=n, cap=n, prio=prio)
        sc.check_chosen(B, n=n, cap=n, prio=prio, permute=True)


@pytest.mark.parametrize("table_set", ("comb", "compact"))
def test_tables(table_set):
    sc.family_tables(B, table_set)


def test_large_table_set():
    """All 12 tables of the large set, entry 2^21 (about one S digit in 2^22
    selects it) among them.  Builds the 3 GiB set in the measurement library's
    context if no earlier test of this process has (test_context_memory_and_table_sets
    builds another in the product's context)."""
    sc.family_tables(B, "large")


# ---- the edge batch (tests/golden/prep_edge_golden.json, verdicts by libsodium;
# proven on the CPU build by test_stage_reference_cpu.py): S whose signed digits
# select entry 0 and the last entry of every [S]B table, Q = [S]B - R the
# identity or of order 2, 4, 8, S in [2^252, L) and around L, 32 keys of every
# kind, accepted signatures with an edge digit
E = "edge"


def _words_differing(dev, cpu, n):
    d, c = sc.by_request(dev, n), sc.by_request(cpu, n)
    return {k: int((np.frombuffer(d[k], np.int32) != np.frombuffer(c[k], np.int32)).sum()) for k in ("atab", "rtab")}


@pytest.mark.parametrize("table_set,buckets,split", sc.VARIANTS)
def test_edge_prep_state(table_set, buckets, split):
    """Every word the prep kernel writes for the 395 edge requests (alive,
    accept, a = b h mod 8L, ranges, the count, every table entry with its limb
    bound, nothing past n).  On the compact joint variant dig, alive and accept
    equal the CPU build's byte for byte; the table words that differ are
    printed, not asserted (any limbs of the same point inside the bound are
    correct)."""
    n = sc.batch_size(E)
    ab = sc.family_prep(B, table_set, buckets, split, batch=E)
    assert sum(1 for x in ab if x is not None) == sum(q["sides"][0] for q in sc.edge_batch()["reqs"])
    dev, cpu = (sc.prep_state(bk, n, table_set, buckets, split, E) for bk in (B, "host"))
    if table_set == "compact" and not split:
        d, c = sc.by_request(dev, n), sc.by_request(cpu, n)
        for k in ("dig", "alive", "accept"):
            assert d[k] == c[k], k
        if not buckets:
            for k in ("dig", "alive", "accept"):
                assert dev[k].tobytes() == cpu[k].tobytes(), k
    print("edge prep state %s: %d slots, table words differing from the CPU build's: %s of %d each" %
          ((table_set, buckets, split), n, _words_differing(dev, cpu, n), n * sc.A_WORDS))


@pytest.mark.parametrize("n", (1, 63, 64, 65))
def test_edge_prep_state_batch_sizes(n):
    """every variant at a size around the wave: slot 62 holds a Q that is the
    identity, slot 63 an accepted signature with a zero digit"""
    for table_set, buckets, split in sc.VARIANTS:
        sc.family_prep(B, table_set, buckets, split, n, batch=E)
    for table_set in ("compact", "large"):
        sc.family_seams(B, table_set, n, batch=E)
    sc.family_sets(B, n, batch=E)
    d, c = (sc.by_request(sc.prep_state(bk, n, "compact", False, False, E), n) for bk in (B, "host"))
    assert all(d[k] == c[k] for k in ("dig", "alive", "accept"))


@pytest.mark.parametrize("table_set", ("compact", "large"))
def test_edge_split_and_bucketed_runs_write_the_joint_state(table_set):
    sc.family_seams(B, table_set, batch=E)


def test_edge_large_and_compact_sets_give_the_same_r_points():
    sc.family_sets(B, batch=E)


@pytest.mark.parametrize("prio", (False, True))
def test_edge_round_trip_matches_libsodium(prio):
    """the prep state through either main kernel: every accepted case accepted, everything else rejected"""
    reqs = sc.edge_batch()["reqs"]
    got = sc.family_round_trip(B, "compact", True, False, prio, batch=E)
    assert got == sc.family_round_trip(B, "large", False, True, prio, batch=E)
    assert got == sc.family_round_trip(B, "compact", False, False, prio, batch=E)
    assert [i for i, v in enumerate(got) if v] == [i for i, q in enumerate(reqs) if q["family"] == "accepted"]
