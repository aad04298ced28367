"""Batched sessions, host side (no GPU): the new entry points are exported and
bound, their workspace size is sane, and every argument check answers before
the first HIP call."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "consensus-entropy_amd")
for _p in (ROOT, PKG_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NEW = ("ce_select_batched_excl", "ce_select_batched_mix_workspace_bytes", "ce_select_batched_mix",
       "ce_mark_selected_batched")
P16 = ctypes.c_void_p(16)  # a dummy non-null pointer: never dereferenced, the checks come first


@pytest.fixture(scope="module")
def L():
    from ce_amd import _lib

    return _lib, _lib.load()


def test_new_symbols_exported_and_bound(L):
    _lib, lib = L
    for name in NEW:
        assert name in _lib.SIGNATURES, name
        f = getattr(lib, name)
        assert f.argtypes == _lib.SIGNATURES[name][1] and f.restype == _lib.SIGNATURES[name][0]


def test_mix_workspace_covers_batched_and_grows_with_q(L):
    _, lib = L
    T = 500 * 1608
    assert lib.ce_select_batched_mix_workspace_bytes(T, T, 500, 10) >= lib.ce_select_batched_workspace_bytes(T, 500, 10)
    sizes = [lib.ce_select_batched_mix_workspace_bytes(T, T, 500, q) for q in (1, 10, 64)]
    assert sizes[0] <= sizes[1] <= sizes[2] and sizes[0] < sizes[2]


def _mix(lib, *, C=4, U=3, offsets_h=P16, ld_hc=4, q=10, ws=P16, ws_bytes=1 << 30):
    # p, dt, total_items, M, C, sN, sM, sC, offsets, hc, total_h, ld_hc, offsets_h, U, excl, excl_h, q, ws, ws_bytes, ...
    return lib.ce_select_batched_mix(P16, 0, 100, 4, C, 4 * C, C, 1, P16, P16, 100, ld_hc, offsets_h, U, None, None, q,
                                     ws, ws_bytes, P16, P16, None)


def _excl(lib, *, U=3, q=10, ws=P16, ws_bytes=1 << 30):
    return lib.ce_select_batched_excl(P16, 0, 100, 4, 4, 16, 4, 1, P16, U, P16, q, ws, ws_bytes, P16, P16, None)


def test_argument_errors_before_any_hip_call(L):
    _lib, lib = L

    def refused(rc, code):
        assert rc == code, (rc, code, lib.ce_last_error())
        assert lib.ce_last_error() != b""

    refused(_mix(lib, U=0), _lib.CE_EINVAL)
    refused(_excl(lib, U=0), _lib.CE_EINVAL)
    refused(_mix(lib, offsets_h=None), _lib.CE_EINVAL)
    refused(_mix(lib, ld_hc=3), _lib.CE_EINVAL)
    refused(_mix(lib, q=-1), _lib.CE_EINVAL)
    refused(_excl(lib, q=-1), _lib.CE_EINVAL)
    refused(_mix(lib, ws=ctypes.c_void_p(256), ws_bytes=8), _lib.CE_EWORKSPACE)
    refused(_mix(lib, ws=None, ws_bytes=0), _lib.CE_EWORKSPACE)
    refused(_excl(lib, ws=ctypes.c_void_p(256), ws_bytes=8), _lib.CE_EWORKSPACE)
    refused(_mix(lib, C=8, ld_hc=8), _lib.CE_EUNSUPPORTED)
    refused(_mix(lib, q=65), _lib.CE_EUNSUPPORTED)
    # the batched mark: null idx with q > 0 slots per user; U < 1; a half-given hc side
    refused(lib.ce_mark_selected_batched(None, 3, 10, P16, P16, None, None, None, None, None), _lib.CE_EINVAL)
    refused(lib.ce_mark_selected_batched(P16, 0, 10, P16, P16, None, None, None, None, None), _lib.CE_EINVAL)
    refused(lib.ce_mark_selected_batched(P16, 3, 10, P16, P16, P16, None, None, None, None), _lib.CE_EINVAL)
    # q = 0 selects and marks nothing
    assert _mix(lib, q=0) == _lib.CE_OK
    assert lib.ce_mark_selected_batched(None, 3, 0, P16, P16, None, None, None, None, None) == _lib.CE_OK


def test_session_constructor_errors_before_device_work():
    """rand is refused by name; hc_to_mc is validated per user on the host."""
    pytest.importorskip("torch")
    import ce_amd

    off = np.array([0, 5, 12])
    hc = np.full((12, 4), 0.25)
    with pytest.raises(ValueError, match="SelectionSession"):
        ce_amd.BatchedSelectionSession(10, "rand", off)
    ok = np.concatenate([np.arange(5), np.arange(7)])
    bad = ok.copy()
    bad[3] = 5  # user 0 has items 0..4
    with pytest.raises(ValueError, match=r"\[0, N_u\)"):
        ce_amd.BatchedSelectionSession(10, "mix", off, hc=hc, hc_to_mc=bad)
    bad = ok.copy()
    bad[7] = -2
    with pytest.raises(ValueError, match=r"\[0, N_u\)"):
        ce_amd.BatchedSelectionSession(10, "mix", off, hc=hc, hc_to_mc=bad)
    bad = ok.copy()
    bad[6] = bad[5]  # two rows of user 1 on one item (the same local item in ANOTHER user is fine: `ok` has that)
    with pytest.raises(ValueError, match="two hc rows"):
        ce_amd.BatchedSelectionSession(10, "mix", off, hc=hc, hc_to_mc=bad)
    with pytest.raises(ValueError, match="hc_to_mc"):  # the identity default needs hc_offsets == offsets
        ce_amd.BatchedSelectionSession(10, "mix", off, hc=hc, hc_offsets=np.array([0, 6, 12]))
    with pytest.raises(ValueError, match="negative"):
        ce_amd.BatchedSelectionSession(-1, "mc", off)
