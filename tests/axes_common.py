"""Helpers shared by test_oracle_axes.py and test_gpu_committee_axes.py (plain
numpy: importable without torch or a GPU)."""
import numpy as np


def same_bits(a, b):
    """float64 arrays equal as uint64 patterns, NaN matching NaN (ENT_TOL_ULP = 0)."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    return bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def first_diff(a, b):
    """(count, first flat position) of the entries same_bits objects to -- for assertion messages."""
    a = np.ascontiguousarray(a, np.float64).ravel()
    b = np.ascontiguousarray(b, np.float64).ravel()
    bad = ~((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b)))
    w = np.flatnonzero(bad)
    return (int(w.size), int(w[0]), float(a[w[0]]), float(b[w[0]])) if w.size else (0, -1, 0.0, 0.0)


def bf16_bits(x32):
    """float32 -> bfloat16 bit patterns (uint16), round to nearest even."""
    u = np.ascontiguousarray(x32, np.float32).view(np.uint32)
    r = (u + np.uint32(0x7FFF) + ((u >> np.uint32(16)) & np.uint32(1))) >> np.uint32(16)
    r = np.where(np.isnan(x32), np.uint32(0x7FC0), r)
    return r.astype(np.uint16)


def bf16_to_f64(bits):
    """bfloat16 bit patterns -> their exact float64 values."""
    return (np.ascontiguousarray(bits, np.uint16).astype(np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)
