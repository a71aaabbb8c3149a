"""CPU-side checks of bsgpu_covariance_requests: exported, declared, listed in capi.SYMBOLS, refuses a NULL context."""
import ctypes
import os
import re

from beam_slam_amd import capi, gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_and_declared():
    lib = gpu.lib()
    assert hasattr(lib, "bsgpu_covariance_requests")
    header = open(os.path.join(ROOT, "include", "bsgpu.h")).read()
    assert re.search(r"int bsgpu_covariance_requests\(bsgpu_ctx\* ctx, int32_t n_requests, const int32_t\* block_pairs, int64_t\* offsets, "
                     r"double\* out\);", header)
    assert "covariance_requests" in capi.SYMBOLS
    declared = set(re.findall(r"\b(bsgpu_[a-z0-9_]+)\s*\(", header))
    assert set("bsgpu_" + s for s in capi.SYMBOLS) == declared
    assert hasattr(capi.Solver, "covariance_requests")


def test_null_context_is_invalid():
    fn = gpu.lib().bsgpu_covariance_requests
    fn.restype = ctypes.c_int
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int32, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_double)]
    pairs = (ctypes.c_int32 * 2)(0, 0)
    off = (ctypes.c_int64 * 2)()
    out = (ctypes.c_double * 9)()
    assert fn(None, 1, pairs, off, out) == capi.ERR_INVALID
    assert fn(None, 0, None, None, None) == capi.ERR_INVALID
