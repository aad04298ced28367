"""Sessions over frame-level members, host side (no GPU): the two new entry
points are declared, exported and bound, every argument check answers before
the first HIP call, and the sessions refuse bad frame geometry on the host."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, "consensus-entropy_amd")
for _p in (ROOT, PKG_DIR):
    if _p not in sys.path:
        sys.path.insert(0, _p)

NEW = ("ce_select_frames_excl", "ce_frames_consensus")
P16 = ctypes.c_void_p(16)  # a dummy non-null pointer: never dereferenced, the checks come first


class Member(ctypes.Structure):
    _fields_ = [("p", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("song_level", ctypes.c_int32),
                ("ld", ctypes.c_int64)]


@pytest.fixture(scope="module")
def L():
    from ce_amd import _lib

    return _lib, _lib.load()


def _members(M, ld=4, dtype=1):
    arr = (Member * max(M, 1))()
    for m in range(max(M, 1)):
        arr[m] = Member(16, dtype, 0, ld)
    return arr


def _sel(lib, *, M=2, C=4, N=1000, excl=P16, q=10, ws=P16, ws_bytes=1 << 30, ld=4, dtype=1, val=P16, idx=P16):
    mem = _members(M, ld, dtype)
    return lib.ce_select_frames_excl(ctypes.cast(mem, ctypes.c_void_p), M, C, P16, None, N, excl, q, 0, ws, ws_bytes,
                                     val, idx, None)


def _cons(lib, *, M=2, C=4, N=1000, excl=None, out=P16, ld_out=4, ld=4, dtype=1):
    mem = _members(M, ld, dtype)
    return lib.ce_frames_consensus(ctypes.cast(mem, ctypes.c_void_p), M, C, P16, None, N, excl, out, ld_out, None)


def test_new_symbols_declared_exported_and_bound(L):
    _lib, lib = L
    with open(os.path.join(ROOT, "include", "ce.h")) as f:
        header = f.read()
    for name in NEW:
        assert re.search(r"\bint\s+%s\s*\(" % name, header), name
        assert name in _lib.SIGNATURES, name
        f = getattr(lib, name)
        assert f.argtypes == _lib.SIGNATURES[name][1] and f.restype == _lib.SIGNATURES[name][0]


def test_argument_errors_before_any_hip_call(L):
    _lib, lib = L

    def refused(rc, code):
        assert rc == code, (rc, code, lib.ce_last_error())
        assert lib.ce_last_error() != b""

    small = lib.ce_select_frames_workspace_bytes(1000, 10)
    refused(_sel(lib, excl=None), _lib.CE_EINVAL)  # a session's selection without its bitmap
    refused(_sel(lib, C=5, ld=5), _lib.CE_EUNSUPPORTED)
    refused(_cons(lib, C=5, ld=5, ld_out=5), _lib.CE_EUNSUPPORTED)
    for M in (0, 33):
        refused(_sel(lib, M=M), _lib.CE_EINVAL)
        refused(_cons(lib, M=M), _lib.CE_EINVAL)
    refused(_sel(lib, ld=3), _lib.CE_EINVAL)
    refused(_cons(lib, ld=3), _lib.CE_EINVAL)
    refused(_cons(lib, ld_out=3), _lib.CE_EINVAL)
    refused(_cons(lib, out=None), _lib.CE_EINVAL)
    refused(_sel(lib, dtype=2), _lib.CE_EUNSUPPORTED)  # bfloat16 members
    refused(_cons(lib, dtype=2), _lib.CE_EUNSUPPORTED)
    refused(_sel(lib, q=-1), _lib.CE_EINVAL)
    refused(_sel(lib, val=None), _lib.CE_EINVAL)
    refused(_sel(lib, ws=ctypes.c_void_p(256), ws_bytes=small - 1), _lib.CE_EWORKSPACE)
    refused(_sel(lib, ws=None, ws_bytes=0), _lib.CE_EWORKSPACE)
    refused(_sel(lib, q=65, ws_bytes=small), _lib.CE_EWORKSPACE)  # q > 64: + the entropies, as ce_select_frames
    # nothing to select / nothing to write
    assert _sel(lib, N=0, q=0, excl=None) == _lib.CE_OK
    assert _sel(lib, q=0) == _lib.CE_OK
    assert _cons(lib, N=0, out=None) == _lib.CE_OK


def test_selection_session_frame_checks_on_the_host():
    pytest.importorskip("torch")
    import ce_amd

    s_id = np.repeat(np.arange(7), 3)  # 7 songs x 3 frames
    with pytest.raises(ValueError, match="n_items"):
        ce_amd.SelectionSession(4, "mc", 8, s_id=s_id, device="cpu")
    hc = np.full((7, 4), 0.25)
    with pytest.raises(ValueError, match="s_id"):
        ce_amd.SelectionSession(4, "hc", 7, hc=hc, s_id=s_id, device="cpu")
    with pytest.raises(ValueError, match="s_id"):
        ce_amd.SelectionSession(4, "rand", 7, s_id=s_id, device="cpu")
    fr = [np.full((21, 4), 0.25)]
    sess = ce_amd.SelectionSession(4, "mc", 7, s_id=s_id[::-1].copy(), device="cpu")
    assert sess.song_ids.tolist() == list(range(7))
    with pytest.raises(ValueError, match="not both"):
        sess.select(committee=np.full((1, 7, 4), 0.25), frames=fr)
    plain = ce_amd.SelectionSession(4, "mc", 7, device="cpu")
    with pytest.raises(ValueError, match="s_id"):
        plain.select(frames=fr)
    with pytest.raises(ValueError, match="neither"):  # 20 rows: neither the 21 frames nor the 7 songs
        sess.select(frames=[np.full((20, 4), 0.25)])


def test_batched_session_frame_checks_on_the_host():
    pytest.importorskip("torch")
    import ce_amd

    off = np.array([0, 5, 12])
    f_off = np.arange(13) * 2
    with pytest.raises(ValueError, match="total_items"):
        ce_amd.BatchedSelectionSession(4, "mc", off, frame_offsets=f_off[:-1], device="cpu")
    bad = f_off.copy()
    bad[4] = bad[3] - 1
    with pytest.raises(ValueError, match="non-decreasing"):
        ce_amd.BatchedSelectionSession(4, "mc", off, frame_offsets=bad, device="cpu")
    with pytest.raises(ValueError, match="frame_perm"):
        ce_amd.BatchedSelectionSession(4, "mc", off, frame_offsets=f_off, frame_perm=np.arange(23), device="cpu")
    with pytest.raises(ValueError, match="frame_offsets"):
        ce_amd.BatchedSelectionSession(4, "mc", off, frame_perm=np.arange(24), device="cpu")
    with pytest.raises(ValueError, match="hc"):
        ce_amd.BatchedSelectionSession(4, "hc", off, hc=np.full((12, 4), 0.25), frame_offsets=f_off, device="cpu")
    fr = [np.full((24, 4), 0.25)]
    sess = ce_amd.BatchedSelectionSession(4, "mc", off, frame_offsets=f_off, device="cpu")
    with pytest.raises(ValueError, match="not both"):
        sess.step(np.full((1, 12, 4), 0.25), frames=fr)
    plain = ce_amd.BatchedSelectionSession(4, "mc", off, device="cpu")
    with pytest.raises(ValueError, match="frame_offsets"):
        plain.select(frames=fr)
