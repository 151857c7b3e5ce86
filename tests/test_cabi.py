"""The product C-ABI library builds, loads without a GPU and exports every
symbol include/edv.h declares and nothing of the measurement header
include/edv_measure.h (that is libedv_measure.so's); without a GPU the shim
fails loudly (no CPU fallback)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HDR = os.path.join(ROOT, "include", "edv.h")
MHDR = os.path.join(ROOT, "include", "edv_measure.h")


def declared(hdr=HDR):
    src = open(hdr).read()
    return sorted(set(re.findall(r"^\s*(?:int|const char \*|void)\s*\**\s*(edv_\w+)\s*\(", src, re.M)))


def exported(path):
    out = subprocess.check_output(["nm", "-D", "--defined-only", path]).decode()
    return set(re.findall(r" T (edv_\w+)$", out, re.M))


def test_header_declares_the_core_entry_points():
    names = declared()
    for need in ("edv_verify_batch", "edv_verify_batch_dev", "edv_version", "edv_last_error", "edv_device_count",
                 "edv_sign_batch_dev", "edv_set_chunk", "edv_context_memory", "edv_verify_batch_async"):
        assert need in names
    meas = declared(MHDR)
    for need in ("edv_profile_batch_dev", "edv_profile_batch_dev_flush", "edv_time_batch_dev",
                 "edv_profile_prep_sides", "edv_test_fail_async", "edv_probe_math", "edv_probe_prep_state",
                 "edv_probe_main_state", "edv_probe_table"):
        assert need in meas and need not in names


def test_library_exports_every_declared_symbol():
    """the product library exports exactly the product
    header's entry points -- no kernel timing, cache flush or fault hook -- and
    the measurement build exports both headers'."""
    from indy_plenum_amd import edv
    lib = edv.lib()
    missing = [n for n in declared() if not hasattr(lib, n)]
    assert missing == []
    prod = exported(edv.LIB_PATH)
    assert prod == set(declared())
    assert not (prod & set(declared(MHDR)))
    meas = exported(edv.MEASURE_LIB_PATH)
    assert meas == set(declared()) | set(declared(MHDR))
    assert edv.version().startswith("edv ") and "gfx950" in edv.version()
    blob = open(edv.LIB_PATH, "rb").read()
    mblob = open(edv.MEASURE_LIB_PATH, "rb").read()
    assert b"edv_flush_kernel" not in blob and b"edv_flush_kernel" in mblob
    # the math probes (edv_probe_math) are the measurement build's alone
    for name in (b"edv_probe_lane_kernel", b"edv_probe_quad_kernel", b"edv_probe_math", b"edv_probe_prep_state",
                 b"edv_probe_main_state", b"edv_probe_table"):
        assert name not in blob and name in mblob
    noverify = os.path.join(os.path.dirname(edv.LIB_PATH), "variants", "libedv_noverify.so")
    if os.path.exists(noverify):
        assert b"edv_probe_" not in open(noverify, "rb").read()


def test_library_contains_gfx950_code_object():
    from indy_plenum_amd import edv
    blob = open(edv.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    assert b"edv_main_kernel" in blob and b"edv_prep_kernel" in blob


@pytest.mark.skipif(os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK), reason="a GPU is present")
def test_no_gpu_means_loud_failure():
    from indy_plenum_amd import edv
    assert edv.device_count() == 0
    with pytest.raises(edv.EdvUnavailable):
        edv.verify_arrays(b"\0" * 64, b"\0" * 32, b"\0" * 16, np.array([0, 0], np.uint64))
    with pytest.raises(edv.EdvUnavailable):
        edv.open_batch([(b"\0" * 64, b"", b"\0" * 32)])


def test_invalid_arguments_are_rejected_before_the_device():
    from indy_plenum_amd import edv
    with pytest.raises(ValueError):
        edv.verify_arrays(b"\0" * 63, b"\0" * 32, b"", np.array([0, 0], np.uint64))
    with pytest.raises(ValueError):
        edv.open_batch([(b"\0" * 64, b"", b"\0" * 31)])
    assert edv.open_batch([(b"\0" * 10, b"\0" * 10, b"\0" * 32)]) == [False]  # sm < 64: no device call


def test_async_entry_points_validate_and_fail_loudly():
    """edv_verify_batch_async / edv_wait_async: size mismatches are rejected in
    the shim, a null ticket pointer and bad offsets in the C-ABI itself (before
    any device is touched), and without a GPU a well-formed submission raises
    EdvUnavailable rather than falling back to the CPU."""
    import ctypes
    from indy_plenum_amd import edv
    sigs, pks = np.zeros(128, np.uint8), np.zeros(64, np.uint8)
    msgs, off, acc = np.zeros(64, np.uint8), np.array([0, 16, 32], np.uint64), np.zeros(2, np.uint8)
    with pytest.raises(ValueError):
        edv.verify_async(sigs[:127], pks, msgs, off, acc)
    with pytest.raises(ValueError):
        edv.verify_async(sigs, pks, msgs, off.astype(np.int64), acc)
    with pytest.raises(ValueError):
        edv.verify_async(sigs, pks, msgs[:16], off, acc)
    lib = edv.lib()
    assert lib.edv_verify_batch_async(sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, off.ctypes.data, 2,
                                      acc.ctypes.data, 0, None) == edv.EDV_E_ARG
    bad = np.array([0, 16, 8], np.uint64)  # offsets must not decrease
    t = ctypes.c_int64(-1)
    assert lib.edv_verify_batch_async(sigs.ctypes.data, pks.ctypes.data, msgs.ctypes.data, bad.ctypes.data, 2,
                                      acc.ctypes.data, 0, ctypes.byref(t)) == edv.EDV_E_ARG
    if not (os.path.exists("/dev/kfd") and os.access("/dev/kfd", os.R_OK)):
        with pytest.raises(edv.EdvUnavailable):
            edv.verify_async(sigs, pks, msgs, off, acc)
        with pytest.raises(edv.EdvUnavailable):
            edv.wait_async(0)


def test_product_library_is_never_the_measurement_build():
    """The measurement-only build (variants/libedv_noverify.so: every request
    reported valid, for bench.py's C5 comparison) is not built by `make all` /
    build(), and the product default is libedv.so, which verifies."""
    env_lib = os.environ.pop("EDV_LIB", None)
    try:
        code = ("import sys; sys.path.insert(0, %r); from indy_plenum_amd import edv; "
                "print(edv.LIB_PATH); print(edv.version())" % ROOT)
        r = subprocess.run(["python3", "-c", code], capture_output=True, text=True, timeout=60,
                           env={k: v for k, v in os.environ.items() if k != "EDV_LIB"})
        assert r.returncode == 0, r.stderr
        path, ver = r.stdout.strip().splitlines()[-2:]
        assert os.path.basename(path) == "libedv.so"
        assert "MEASUREMENT-ONLY" not in ver
    finally:
        if env_lib is not None:
            os.environ["EDV_LIB"] = env_lib
    mk = open(os.path.join(ROOT, "indy-plenum_amd", "csrc", "Makefile")).read()
    all_line = [ln for ln in mk.splitlines() if ln.startswith("all:")][0]
    assert "noverify" not in all_line


def _load_in_child(lib, allow):
    env = {k: v for k, v in os.environ.items() if k not in ("EDV_LIB", "EDV_ALLOW_MEASUREMENT_LIB")}
    env["EDV_LIB"] = lib
    if allow:
        env["EDV_ALLOW_MEASUREMENT_LIB"] = "1"
    code = ("import sys; sys.path.insert(0, %r); from indy_plenum_amd import edv\n"
            "try:\n    edv.lib(); print('LOADED', edv.version())\n"
            "except edv.EdvUnavailable as ex:\n    print('REFUSED', ex)\n" % ROOT)
    r = subprocess.run(["python3", "-c", code], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0, r.stderr
    return r.stdout.strip().splitlines()[-1]


def test_loader_refuses_measurement_builds(tmp_path):
    """Fail closed: a library whose edv_version() says
    MEASUREMENT-ONLY is refused by edv.lib() with EdvUnavailable, wherever
    EDV_LIB points, unless EDV_ALLOW_MEASUREMENT_LIB=1 (set only by
    tools/bench_pool.run_isolated in its child).  Checked on a stand-in
    library with that version string and, when it is built, on the real
    variants/libedv_noverify.so."""
    src = tmp_path / "fake.c"
    src.write_text('const char* edv_version(void) { return "edv 0.2.0 gfx950 MEASUREMENT-ONLY: test"; }\n')
    fake = str(tmp_path / "libfake.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", str(src), "-o", fake])
    assert _load_in_child(fake, allow=False).startswith("REFUSED")
    libs = [os.path.join(ROOT, "indy-plenum_amd", "variants", "libedv_noverify.so")]
    for lib in libs:
        if os.path.exists(lib):
            assert _load_in_child(lib, allow=False).startswith("REFUSED")
            assert _load_in_child(lib, allow=True).startswith("LOADED")
    bp = open(os.path.join(ROOT, "tools", "bench_pool.py")).read()
    assert 'EDV_ALLOW_MEASUREMENT_LIB="1"' in bp



def test_async_ledger_failures_are_sticky():
    """the asynchronous path's ticket ledger (edv_ledger.h,
    the code libedv.so runs, built for the CPU) never reports a failed ticket as
    complete, however many tickets fail after it (the earlier 256-entry list
    dropped the oldest), and reports tickets never issued as unknown."""
    import hostcheck_lib as hc
    E_ARG, E_HIP = -1, -3
    failed = list(range(0, 600))                     # far more than 256 failures
    got = hc.ledger(1000, failed, [0, 1, 255, 256, 599, 600, 999, 1000, -1])
    assert got == [E_HIP, E_HIP, E_HIP, E_HIP, E_HIP, 0, 0, E_ARG, E_ARG]
    # one late failure fails every earlier settled ticket (fail closed), not the later ones
    assert hc.ledger(50, [30], [0, 29, 30, 31, 49]) == [E_HIP, E_HIP, E_HIP, 0, 0]
    assert hc.ledger(10, [], [0, 9, 10]) == [0, 0, E_ARG]
