"""Packing of math-probe cases (include/edv_measure.h, edv_probe_math) and the
two backends that run them: `host` is libedv_hostcheck.so (the headers built
by g++, hc_probe_math), `device` is libedv_measure.so's probe kernels on the
GPU.  Same ops, same packed layout: 32-bit little-endian words, a limb vector
is 10 int32, a scalar 8 or 16 words, a double its raw 64-bit pattern."""
import ctypes

import numpy as np

import hostcheck_lib

QUAD_OPS = ("quad_sq_shift", "quad_dbl", "quad_add", "quad_cached", "quad_cached_signed")


def _ops():
    from indy_plenum_amd import edv
    return edv.PROBE_OPS


def host(op, cases):
    """Run packed cases (n, input bytes) through the CPU build; -> (n, output bytes)."""
    code, nin, nout = _ops()[op]
    cases = np.ascontiguousarray(cases, dtype=np.uint8)
    assert cases.ndim == 2 and cases.shape[1] == nin, (op, cases.shape)
    out = np.zeros((cases.shape[0], nout), np.uint8)
    hc = hostcheck_lib.load()
    hc.hc_probe_math.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_uint64, ctypes.c_void_p, ctypes.c_uint64,
                                 ctypes.c_uint64]
    assert hc.hc_probe_math(code, cases.ctypes.data, nin, out.ctypes.data, nout, cases.shape[0]) == 0, op
    return out


def device(op, cases):
    """Run packed cases through the device build (one probe kernel launch)."""
    from indy_plenum_amd import edv
    return edv.probe_math(op, cases)


# ---- packing
def pack_limbs(vectors):
    """n cases of k limb vectors each, [[limbs, ...], ...] -> (n, 40 k) bytes"""
    a = np.array(vectors, dtype=np.int64)
    assert a.ndim == 3 and a.shape[2] == 10 and np.all(np.abs(a) < 2**31)
    return np.ascontiguousarray(a.astype(np.int32).reshape(a.shape[0], -1)).view(np.uint8)


def unpack_limbs(out, k=None):
    """(n, 40 k) bytes -> n lists of k limb vectors (Python ints)"""
    w = np.ascontiguousarray(out).view(np.int32)
    return w.reshape(w.shape[0], -1, 10).tolist()


def pack_ints(values, nbytes):
    """n cases of j unsigned integers each -> (n, j nbytes) bytes, little-endian"""
    return np.array([list(b"".join(int(v).to_bytes(nbytes, "little") for v in row)) for row in values], np.uint8)


def unpack_ints(out, nbytes):
    """(n, j nbytes) bytes -> n lists of j unsigned integers"""
    raw = np.ascontiguousarray(out)
    return [[int.from_bytes(row[o:o + nbytes].tobytes(), "little") for o in range(0, raw.shape[1], nbytes)]
            for row in raw]


def pack_words(rows):
    """n cases of j signed or unsigned 32-bit words each -> (n, 4 j) bytes"""
    a = np.array(rows, dtype=np.int64) & 0xFFFFFFFF
    return np.ascontiguousarray(a.astype(np.uint32)).view(np.uint8)


def pack_doubles(rows):
    """n cases of j doubles each -> (n, 8 j) bytes (raw IEEE patterns)"""
    return np.ascontiguousarray(np.array(rows, dtype=np.float64)).view(np.uint8)


def unpack_doubles(out):
    return np.ascontiguousarray(out).view(np.float64)
