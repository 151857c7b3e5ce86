"""The latency path's kernels (edv_quad.hip: edv_rtl_kernel, sixteen lanes per
signature, and edv_quad_kernel, eight) cut at the barrier after their phase 1,
on the device: what phase1<BITS, NS> leaves in LDS read back word for word
(digits, both negated decompressions, [S]B, the ok bytes, the padding slots of
a tiny batch), and the walks (rtl_walk: doubler / adder ring, buckets, running
sums; quad_walk: table build, alignment shift, slot pick) run on chosen phase-1
states no SHA-512 output produces: every window count 1..64, workgroup maxima
around the ring size, all digits in one bucket, count words above a slot's own
count, both signs, small-order results, each ok byte cleared, padding slots
that would be accepted or rejected.  The latency probes of libedv_measure.so
(include/edv_measure.h) are probe kernels that instantiate the header
functions the product's kernels are made of (edv_quad_body.h); they are not
the product's kernel objects.  The cases and Python-integer checkers are those
test_stage_reference_cpu.py proves on the CPU references (stage_cases.py).

Measured on MI355X (gfx950), recorded in DESIGN.md section 5:
  walk in      1,269 slots (867 cases) through rtl_walk, 933 (658 cases) through
               quad_walk; 0 of 883 / 658 requested cases dropped; batch sizes 1, 3,
               15, 16, 17, 31, 32, 33 per kernel
  phase 1 out  600 requests (608 slots), both kernels x both table sets; 0 of 565
               digit-word sets differ from edv_probe_prep_state's in each (printed
               by test_latency_phase1_state, not asserted)
  outcome      all 37 tests pass, no defect found; libedv.so's device code hash
               is the parent's
  durations    0.94 s / 0.84 s the chosen-state tests (the first use builds the
               cases), 0.86 s the first phase-1 variant, 0.2-0.3 s the other
               phase-1 variants and the argument rejection, the rest below 0.1 s
  edge batch   395 requests (400 / 416 slots), both kernels x both table sets at
               n = 1, 15, 16, 17, 33, 395; 0 of 367 digit-word sets differ from
               edv_probe_prep_state's; 1.0 s the first test (the oracle's base
               multiplications), 0.18-0.24 s the others, 2.0 s the 6 edge tests"""
import numpy as np
import pytest

import stage_cases as sc

pytestmark = pytest.mark.gpu
B = "device"
KERNELS = ("rtl", "quad")


def test_latency_probes_reject_bad_arguments():
    from indy_plenum_amd import edv
    m = edv.measure_lib()
    b = sc.uniform_batch(3)
    p = lambda a: a.ctypes.data                                                  # noqa: E731
    dig, pt, ok = np.zeros((17, 32), np.uint32), np.zeros((3, 40, 32), np.int32), np.zeros((3, 32), np.uint8)
    acc = np.zeros(32, np.uint8)

    def phase1(kernel=0, table_set=0, n=3, sigs=b["sigs"], dig=dig):
        return m.edv_probe_latency_phase1(0, kernel, table_set, None if sigs is None else p(sigs), p(b["pks"]),
                                          p(b["msgs"]), p(b["off"]), n, None if dig is None else p(dig), p(pt), p(ok),
                                          p(acc))

    def walk(kernel=0, n=3, slots=16, flags=0, dig=dig, ok=ok, accept=acc):
        return m.edv_probe_latency_walk(0, kernel, n, slots, None if dig is None else p(dig), p(pt), p(ok), flags,
                                        None if accept is None else p(accept))

    bad = [lambda: phase1(kernel=2), lambda: phase1(kernel=-1), lambda: phase1(table_set=2), lambda: phase1(sigs=None),
           lambda: phase1(dig=None), lambda: phase1(n=sc.CAP + 1),
           lambda: walk(kernel=2), lambda: walk(flags=1), lambda: walk(dig=None), lambda: walk(accept=None),
           lambda: walk(n=sc.CAP + 1, slots=sc.CAP + 16), lambda: walk(slots=32), lambda: walk(kernel=1, slots=16),
           lambda: walk(n=17, slots=16)]
    for k, call in enumerate(bad):
        assert call() == edv.EDV_E_ARG, k
        assert b"probe" in m.edv_last_error(), k
    # a live slot (a padding slot here) whose count word is above 64: outside the walks' domain
    for kernel, ns in ((0, 16), (1, 32)):
        d2, ok2 = np.zeros((1, 17, ns), np.uint32), np.ones((1, 3, ns), np.uint8)
        d2[0, 16, 5] = 65
        assert walk(kernel=kernel, slots=ns, dig=d2, ok=ok2) == edv.EDV_E_ARG and b"probe" in m.edv_last_error()
        ok2[0, 1, 5] = 0                                  # the same word on a slot a side killed: fine
        assert walk(kernel=kernel, slots=ns, dig=d2, ok=ok2) == edv.EDV_OK
    # n = 0: fine, nothing launched, nothing read
    assert phase1(n=0, sigs=None, dig=None) == edv.EDV_OK and walk(n=0, slots=0, dig=None) == edv.EDV_OK


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_walk_chosen_state(kernel):
    n = sc.check_lat_walk(B, kernel)
    _, tally = sc.lat_cases(kernel)
    print("latency walk %s: %d slots; per family %s; %d of %d requested cases dropped" %
          (kernel, n, {k: v - tally.dropped[k] for k, v in tally.asked.items()}, sum(tally.dropped.values()),
           sum(tally.asked.values())))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", sc.LAT_WALK_SIZES)
def test_latency_walk_batch_sizes(kernel, n):
    sc.check_lat_sizes(B, kernel, n)


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("table_set", ("compact", "large"))
def test_latency_phase1_state(kernel, table_set):
    """(the large-set variants use the 3 GiB set of the measurement library's context)"""
    dev = sc.family_lat_phase1(B, kernel, table_set)
    prep = sc.prep_state(B, sc.PREP_N, table_set, False, False)
    st = sc.lat_phase1_state(B, kernel, sc.PREP_N, table_set)
    live = [i for i, x in enumerate(dev) if x is not None]
    differ = sum(1 for i in live if (st["dig"][:, i] != prep["dig"][:, i]).any())
    print("latency phase 1 %s %s: %d slots, %d of %d (a, b) digit words differ from edv_probe_prep_state's" %
          (kernel, table_set, st["slots"], differ, len(live)))


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("n", sc.LAT_P1_SIZES[:-1])
def test_latency_phase1_batch_sizes(kernel, n):
    sc.family_lat_phase1(B, kernel, "compact", n)
    sc.family_lat_phase1(B, kernel, "large", n)


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_table_sets_give_the_same_points(kernel):
    sc.family_lat_sets(B, kernel)


@pytest.mark.parametrize("kernel", KERNELS)
def test_latency_round_trip_matches_the_oracle_and_the_product(kernel):
    from indy_plenum_amd import edv
    b = sc.prep_batch()
    got = sc.family_lat_round_trip(B, kernel, "compact")
    assert got == sc.family_lat_round_trip(B, kernel, "large")
    assert got == edv.verify_arrays(b["sigs"], b["pks"], b["msgs"], b["off"]).tolist()
    for n in (1, 15, 17, 33):
        assert sc.family_lat_round_trip(B, kernel, "compact", n) == got[:n]


# ---- the edge batch (tests/golden/prep_edge_golden.json, verdicts by libsodium):
# phase 1 gathers entry 0 and the last entry of every [S]B table, cuts S in
# [2^252, L) and above to 253 bits, and pads a tiny batch with an edge request
E = "edge"


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("table_set", ("compact", "large"))
def test_edge_latency_phase1_state(kernel, table_set):
    """n = 1, 15, 16, 17, 33 and the whole batch: [S]B against the oracle for
    every edge S, the padding rule with an edge request repeated, limbs inside
    RED; then phase 1 out -> walk in gives the fixture's verdicts"""
    for n in (1, 15, 16, 17, 33, None):
        sc.family_lat_phase1(B, kernel, table_set, n, batch=E)
    reqs = sc.edge_batch()["reqs"]
    got = sc.family_lat_round_trip(B, kernel, table_set, batch=E)
    assert [i for i, v in enumerate(got) if v] == [i for i, q in enumerate(reqs) if q["family"] == "accepted"]
    for n in (1, 15, 17, 33, 64):
        assert sc.family_lat_round_trip(B, kernel, table_set, n, batch=E) == got[:n]


@pytest.mark.parametrize("kernel", KERNELS)
def test_edge_latency_table_sets_give_the_same_points(kernel):
    sc.family_lat_sets(B, kernel, batch=E)
    n = sc.batch_size(E)
    st, prep = sc.lat_phase1_state(B, kernel, n, "compact", E), sc.prep_state(B, n, "compact", False, False, E)
    live = [i for i, q in enumerate(sc.edge_batch()["reqs"]) if q["sides"][0]]
    print("edge latency phase 1 %s: %d of %d (a, b) digit words differ from edv_probe_prep_state's" %
          (kernel, sum(1 for i in live if (st["dig"][:, i] != prep["dig"][:, i]).any()), len(live)))
