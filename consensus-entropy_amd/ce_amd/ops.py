"""Device-tensor operators over the C-ABI (torch is plumbing: memory + streams).

Every op takes torch tensors resident on a HIP device, launches on torch's
current stream and returns device tensors; nothing is synchronised here.
There is no CPU path: a CPU tensor is an error.
"""
from __future__ import annotations

import ctypes
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import CE_BF16, CE_F32, CE_F64, call
from .xgb import LANE_TABLE_DEPTH, MAX_FEATURES, StackedForests, XgbForest

_DT = {torch.float32: CE_F32, torch.float64: CE_F64, torch.bfloat16: CE_BF16}
LAYOUTS = ("MNC", "NMC")


def _stream(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def _on_gpu(t, what):
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{what} must be a torch.Tensor")
    if t.device.type != "cuda":
        raise ValueError(f"{what} must live on a HIP device (got {t.device}); there is no CPU path")


def _i64(t, what):
    """An index tensor (offsets, perm, picks) as the C-ABI reads it: on the device, int64, contiguous."""
    _on_gpu(t, what)
    if t.dtype == torch.int64 and t.is_contiguous():  # the usual case, without two dispatches
        return t
    return t.to(torch.int64).contiguous()


def _indexed(device):
    """torch.device(device); one without an index becomes the current device."""
    if not isinstance(device, torch.device):
        device = torch.device(device)
    return device if device.index is not None else torch.device("cuda", torch.cuda.current_device())


WS_HEADER_BYTES = 65536 + 256  # include/ce.h: the 64 KiB counter header (+ the 256-B alignment carve)


def new_workspace(nbytes, device, header_only=False):
    """A workspace for the engine, zero-filled as include/ce.h requires (its
    header holds the tiled kernels' arrival counters, which every call leaves
    zero again).  header_only: zero just the header -- for the sort path's
    per-call workspaces, whose body every pass writes before it reads."""
    n = max(int(nbytes), 256)
    if not header_only:
        return torch.zeros(n, dtype=torch.uint8, device=device)
    buf = torch.empty(n, dtype=torch.uint8, device=device)
    buf[:WS_HEADER_BYTES].zero_()
    return buf


class _GraphArena:
    """Zero-filled device memory that captured selections carve their
    workspaces from, one arena per device, filled and synchronised ONCE,
    eagerly, outside any capture.

    A captured call's workspace header (the arrival counters) must be zero at
    the graph's first replay; every call leaves it zero again (include/ce.h).
    Carving from memory zeroed before the capture therefore needs no zero-fill
    node in the graph: each replay runs the selection kernel alone.  A carve is
    never handed out twice, and it is never freed, because a graph may replay
    for the life of the process.  Captures are rare (one per graph) and a small
    pool's workspace is 70-230 KB, so the default 64 MiB lasts hundreds of
    captures.  reserve() adds room before a capture that needs more."""

    ALIGN = 256
    DEFAULT_BYTES = int(os.environ.get("CE_AMD_GRAPH_ARENA_MB", "64")) << 20

    def __init__(self):
        self._free = {}  # device index -> list of [buffer, next offset]

    def reserve(self, device, nbytes):
        """Eager only: make sure `nbytes` can be carved on `device` (adds a
        new zeroed arena when the current ones are short)."""
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("reserve_graph_workspace must run outside HIP-graph capture")
        arenas = self._free.setdefault(device.index, [])
        if any(buf.numel() - off >= nbytes for buf, off in arenas):
            return
        n = max(int(nbytes) + self.ALIGN, self.DEFAULT_BYTES)
        buf = torch.zeros(n, dtype=torch.uint8, device=device)
        # the one synchronisation: the fill must be done before any replay,
        # and a replay may run on any stream
        torch.cuda.current_stream(device).synchronize()
        arenas.append([buf, 0])

    def ensure(self, device):
        if device.index not in self._free:
            self.reserve(device, 0)

    def carve(self, device, nbytes):
        """A zero-filled region of >= nbytes that nothing else uses, or None."""
        nbytes = max(int(nbytes), 256)
        for slot in self._free.get(device.index, ()):
            buf, off = slot
            if buf.numel() - off >= nbytes:
                slot[1] = off + (nbytes + self.ALIGN - 1) // self.ALIGN * self.ALIGN
                return buf[off:off + nbytes]
        return None


def _capture_id(device):
    """The HIP capture id of the device's current stream (unique per capture)."""
    st = ctypes.c_int(0)
    cid = ctypes.c_ulonglong(0)
    rc = _lib.hip_stream_capture_info(torch.cuda.current_stream(device).cuda_stream, st, cid)
    return cid.value if rc == 0 else None


class _WorkspaceCache:
    """Scratch reused across calls, one per (device, stream): include/ce.h
    allows one workspace per stream -- its header holds the arrival counters of
    the folded merges, so two streams sharing one would mix their tickets.  A
    buffer grows (never shrinks), so steady state allocates nothing.

    Bounded: at most MAX_STREAMS buffers, least recently used evicted first (a
    caller cycling through short-lived streams does not pin one buffer per
    stream; an evicted buffer goes back to torch's allocator in its own
    stream's order).  Workspaces of the sort path (q > CE_MAX_Q, ~40 B per
    item: GBs on a 100M pool) are never cached: each such call gets its own,
    released when the call's tensors are, so one large-q call does not keep
    them allocated for the life of the process.

    Under HIP-graph capture a call never uses a cached buffer, so growing the
    cache later cannot free memory a graph still uses, and replays never share
    counters with eager calls.  The workspace is carved from the pre-zeroed
    graph arena (_GraphArena): one carve per (capture, stream), shared by the
    sequential calls on that stream inside that capture, as eager calls share
    their stream's buffer.  The replays then run no zero-fill node.  When the
    arena has no room (or no eager call ever created it), the call falls back
    to a workspace allocated inside the capture with a captured zero fill that
    runs at every replay (correct, one node slower; warned once).  Sort-path
    calls under capture always take that fallback with a header-only fill."""

    MAX_STREAMS = 16

    def __init__(self):
        import collections

        self._ws = collections.OrderedDict()
        self._captured = {}  # (device, stream, capture id) -> carved workspace
        self.arena = _GraphArena()
        self._warned = False

    def get(self, device, nbytes, transient=False):
        device = _indexed(device)
        with torch.cuda.device(device):  # the capture state of THIS device's current stream
            capturing = torch.cuda.is_current_stream_capturing()
        if capturing:
            return self._get_captured(device, nbytes, transient)
        if transient:
            return new_workspace(nbytes, device, header_only=True)
        self.arena.ensure(device)
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        buf = self._ws.get(key)
        if buf is None or buf.numel() < nbytes:
            # the old buffer (if any) is released on this stream: the caching
            # allocator reuses its block only in this stream's order
            buf = new_workspace(nbytes, device)
            self._ws[key] = buf
        self._ws.move_to_end(key)
        while len(self._ws) > self.MAX_STREAMS:
            self._ws.popitem(last=False)
        return buf

    def _get_captured(self, device, nbytes, transient):
        if not transient:
            cid = _capture_id(device)
            key = (device.index, torch.cuda.current_stream(device).cuda_stream, cid)
            buf = self._captured.get(key) if cid is not None else None
            if buf is not None and buf.numel() >= nbytes:
                return buf
            buf = self.arena.carve(device, nbytes) if cid is not None else None
            if buf is not None:
                self._captured[key] = buf
                return buf
            if not self._warned:
                import warnings

                warnings.warn("ce_amd: no pre-zeroed graph workspace left (call ops.reserve_graph_workspace "
                              "before capture); this captured selection replays a zero-fill node", stacklevel=3)
                self._warned = True
        return new_workspace(nbytes, device, header_only=transient)

    def clear(self):
        """Release the cached eager workspaces (the graph arena stays: graphs
        may still replay from it)."""
        self._ws.clear()

    def __len__(self):
        return len(self._ws)


WORKSPACE = _WorkspaceCache()


def reserve_graph_workspace(nbytes, device=None):
    """Before capturing selections into a HIP graph: make sure the graph arena
    can hand out `nbytes` of pre-zeroed workspace on `device` (eager only).
    Size it with the ce_*_workspace_bytes functions, one carve per stream per
    capture."""
    device = _indexed(device if device is not None else "cuda")
    with torch.cuda.device(device):
        WORKSPACE.arena.reserve(device, int(nbytes))


def _committee_args(P, layout):
    """The committee run of the C-ABI's signatures, to splat into a call:
    (p, dtype code, N, M, C, sN, sM, sC) of a committee tensor.  'MNC' is the
    reference's stack np.array(pred_prob) (amg_test.py:441); 'NMC' is the
    item-major [N, M, C] tensor.  Any strides are accepted."""
    _on_gpu(P, "committee")
    if P.dim() != 3:
        raise ValueError(f"committee must be 3-D, got shape {tuple(P.shape)}")
    if P.dtype not in _DT:
        raise TypeError(f"committee dtype {P.dtype} not in float32/float64/bfloat16")
    if layout == "MNC":
        M, N, C = P.shape
        sM, sN, sC = P.stride()
    elif layout == "NMC":
        N, M, C = P.shape
        sN, sM, sC = P.stride()
    else:
        raise ValueError(f"layout must be one of {LAYOUTS}, got {layout!r}")
    if M < 1 or C < 1:
        raise ValueError(f"committee needs M >= 1 members and C >= 1 classes, got M={M}, C={C}")
    return _p(P), _DT[P.dtype], N, M, C, sN, sM, sC


def committee_view(P, layout="MNC"):
    """(N, M, C, sN, sM, sC, dtype code) of a committee tensor ('MNC' / 'NMC', any strides)."""
    _, dt, N, M, C, sN, sM, sC = _committee_args(P, layout)
    return N, M, C, sN, sM, sC, dt


def committee_entropy(P, layout="MNC", return_mean=False):
    """amg_test.py:441+443 per item: f64 entropies [N] (and the [N, C] mean)."""
    comm = _committee_args(P, layout)
    N, C = comm[2], comm[4]
    ent = torch.empty(N, dtype=torch.float64, device=P.device)
    mean = torch.empty((N, C), dtype=torch.float64, device=P.device) if return_mean else None
    call("ce_committee_entropy", *comm, _p(mean), _p(ent), _stream(P.device))
    return (ent, mean) if return_mean else ent


def _map_f64(fn, name, x):
    """y[i] = fn(x[i]) over a float64 device tensor (ce_log_f64 / ce_exp_f64)."""
    _on_gpu(x, "x")
    x = x.contiguous()
    if x.dtype != torch.float64:
        raise ValueError(f"{name} takes float64")
    y = torch.empty_like(x)
    call(fn, _p(x), x.numel(), _p(y), _stream(x.device))
    return y


def log_f64(x):
    """glibc's log(x) as the engine evaluates it inside every entropy
    (ce_log_f64; verification against the C library)."""
    return _map_f64("ce_log_f64", "log_f64", x)


def exp_f64(x):
    """glibc's exp(x) as the engine evaluates it in the GaussianNB member
    (ce_exp_f64; verification against the C library)."""
    return _map_f64("ce_exp_f64", "exp_f64", x)


def _approx_rows(fn, name, rows, dtype=None):
    """(h2 f32 [n], special bool [n]) of rows [n, C] f64 through ce_approx_entropy /
    ce_wide_approx_entropy (dtype: the latter's committee dtype)."""
    _on_gpu(rows, "rows")
    rows = rows.contiguous()
    if rows.dtype != torch.float64 or rows.dim() != 2:
        raise ValueError(f"{name} takes [n, C] float64")
    n, C = rows.shape
    h2 = torch.empty(n, dtype=torch.float32, device=rows.device)
    sp = torch.empty(n, dtype=torch.uint8, device=rows.device)
    call(fn, _p(rows), n, C, *(() if dtype is None else (_DT[dtype],)), _p(h2), _p(sp), _stream(rows.device))
    return h2, sp.bool()


def approx_entropy(rows):
    """The single-block pools' approximate entropy of exact consensus rows
    [n, C] f64 (ce_approx_entropy: log2 units, f32) and their special flags
    (verification of the prefilter's error bound)."""
    return _approx_rows("ce_approx_entropy", "approx_entropy", rows)


def wide_approx_entropy(rows, dtype=torch.bfloat16):
    """The wide stream's approximate prefilter entropy (ce_wide_approx_entropy:
    log2 units, f32) of rows [n, C] f64 -- member sums or means, in the register
    layout k_stream_wide2 uses for a ``dtype`` committee -- and their special
    flags (verification of the margin the C5 prefilter skips items by)."""
    return _approx_rows("ce_wide_approx_entropy", "wide_approx_entropy", rows, dtype)


def row_div_f64(x, s):
    """x / s as the engine divides each consensus row by its sum inside the
    entropy (ce_row_div_f64: one reciprocal per row; verification against
    IEEE division)."""
    _on_gpu(x, "x")
    x = x.contiguous().to(torch.float64)
    s = s.contiguous().to(torch.float64)
    if x.shape != s.shape:
        raise ValueError("x and s must have one shape")
    y = torch.empty_like(x)
    call("ce_row_div_f64", _p(x), _p(s), x.numel(), _p(y), _stream(x.device))
    return y


def vote_table(votes, C=4):
    """amg_test.py:109-117 on int8 votes [N, A] (-1 = missing): (freq [N, C], ent [N])."""
    _on_gpu(votes, "votes")
    if votes.dtype != torch.int8 or votes.dim() != 2:
        raise ValueError("votes must be a 2-D int8 tensor")
    if votes.stride(1) != 1:
        votes = votes.contiguous()
    N, A = votes.shape
    freq = torch.empty((N, C), dtype=torch.float64, device=votes.device)
    ent = torch.empty(N, dtype=torch.float64, device=votes.device)
    call("ce_vote_entropy", _p(votes), N, A, C, votes.stride(0), _p(freq), _p(ent), _stream(votes.device))
    return freq, ent


def va_table(va):
    """amg_test.py:88-117 from raw [N, A, 2] f64 (valence, arousal), NaN = missing."""
    _on_gpu(va, "va")
    if va.dtype != torch.float64 or va.dim() != 3 or va.shape[2] != 2:
        raise ValueError("va must be a [N, A, 2] float64 tensor")
    va = va.contiguous()
    N, A, _ = va.shape
    freq = torch.empty((N, 4), dtype=torch.float64, device=va.device)
    ent = torch.empty(N, dtype=torch.float64, device=va.device)
    call("ce_va_entropy", _p(va), N, A, _p(freq), _p(ent), _stream(va.device))
    return freq, ent


def _csr(offsets, perm):
    """(offsets, perm, N) of a CSR over N songs, as the C-ABI reads them."""
    offsets = _i64(offsets, "offsets")
    if offsets.numel() < 1:
        raise ValueError("offsets must hold N + 1 entries")
    return offsets, (_i64(perm, "perm") if perm is not None else None), offsets.numel() - 1


def segment_mean(frames, offsets, perm=None, out=None):
    """amg_test.py:437 groupby(['s_id']).mean() of one member on the device
    (pandas 1.1.5 group_mean: f64 sequential sums in row order, NaN skipped,
    float32 input -> float32-rounded result).  frames [F, C] f32/f64; song n
    owns rows perm[offsets[n]:offsets[n+1]] (or offsets[n]:offsets[n+1]).
    out: optional [N, C] f32/f64 view with unit column stride (e.g. member m of
    a committee stack); default a new tensor of the frames' dtype."""
    _on_gpu(frames, "frames")
    _on_gpu(offsets, "offsets")  # refused before a bad frames shape is; _csr does the rest
    if frames.dim() != 2 or frames.dtype not in (torch.float32, torch.float64):
        raise ValueError("frames must be a 2-D float32/float64 tensor [F, C]")
    if frames.stride(1) != 1:
        frames = frames.contiguous()
    F, C = frames.shape
    offsets, perm, N = _csr(offsets, perm)
    if out is None:
        out = torch.empty((N, C), dtype=frames.dtype, device=frames.device)
    if out.dim() != 2 or tuple(out.shape) != (N, C) or out.stride(1) != 1 or out.dtype not in _DT:
        raise ValueError(f"out must be an [N={N}, C={C}] float32/float64 view with unit column stride")
    call("ce_segment_mean", _p(frames), _DT[frames.dtype], F, C, frames.stride(0), _p(perm), _p(offsets), N,
         _p(out), _DT[out.dtype], out.stride(0), _stream(frames.device))
    return out


class _Member(ctypes.Structure):
    """include/ce.h ce_member."""
    _fields_ = [("p", ctypes.c_void_p), ("dtype", ctypes.c_int32), ("song_level", ctypes.c_int32),
                ("ld", ctypes.c_int64)]


def _frame_members(members, offsets, perm, song_level):
    """The member and shape rules of the frames entry points: (ce_member array,
    the tensors it points into, C, N, offsets, perm).  ``members``: device
    tensors [F, C] (frame rows) or [N, C] (song-level); ``song_level`` overrides
    the shape rule per member.  With ``perm`` or ``song_level`` given nothing is
    read back from the device."""
    members = list(members)
    if not members:
        raise ValueError("committee has no members")
    offsets, perm, N = _csr(offsets, perm)
    C = members[0].shape[1]
    for m, t in enumerate(members):
        _on_gpu(t, f"member {m}")
        if t.dim() != 2 or t.shape[1] != C or t.dtype not in (torch.float32, torch.float64):
            raise ValueError(f"member {m} must be a float32/float64 [*, {C}] tensor")
    if song_level is not None and len(song_level) != len(members):
        raise ValueError("song_level needs one flag per member")
    # F (frames): the permutation's length, else the row count of the frame-level
    # members (rows other than N, or flagged frame-level), else one device read
    F = perm.numel() if perm is not None else None
    if F is None:
        fr = {t.shape[0] for m, t in enumerate(members)
              if (not bool(song_level[m]) if song_level is not None else t.shape[0] != N)}
        if len(fr) > 1:
            raise ValueError(f"frame-level members disagree on the frame count: {sorted(fr)}")
        F = fr.pop() if fr else None
    if F is None and song_level is not None:  # every member flagged song-level: no frame row is read
        F = 0
    if F is None:  # every member has N rows: only the offsets tell
        F = int(offsets[-1])
    arr = (_Member * len(members))()
    keep = []
    for m, t in enumerate(members):
        if t.stride(1) != 1:
            t = t.contiguous()
        keep.append(t)
        if song_level is not None:
            sl = bool(song_level[m])
        elif t.shape[0] != N:
            sl = False
        else:  # N rows: song-level unless there are exactly N frames too
            sl = F != N
        # the kernel reads row n of a song-level member and rows < F of a frame-level one
        need = N if sl else F
        if t.shape[0] < need:
            raise ValueError(f"member {m} has {t.shape[0]} rows; a {'song' if sl else 'frame'}-level member needs "
                             f">= {need}")
        arr[m] = _Member(t.data_ptr(), _DT[t.dtype], 1 if sl else 0, t.stride(0))
    return arr, keep, C, N, offsets, perm


def select_frames(members, offsets, q, perm=None, base_idx=0, song_level=None, excl=None):
    """amg_test.py:426-445 from the members' FRAME-level outputs in one pass
    (ce_select_frames): per member the groupby(['s_id'])
    mean (:437), the member-sequential mean over the stack, the entropy and the
    top-q over songs -- the [M, N, C] stack is never written.  ``members``:
    device tensors [F, C] (frame rows, song n = rows perm[offsets[n]:
    offsets[n+1]] or offsets[n]:offsets[n+1]) or [N, C] (song-level, e.g. the
    CNN member); ``song_level`` overrides the shape rule per member.  Any q:
    q <= 64 in one pass; larger q through the per-song entropies.  excl: an
    optional exclusion bitmap over the songs (excl_bitmap(N); bit n set = song
    n is out of the pool, whatever base_idx): the selection runs over the
    others inside the same kernels (ce_select_frames_excl) -- a session's
    epoch without rebuilding the offsets.
    Returns (vals [q], idx [q]) over the N sorted songs."""
    arr, keep, C, N, offsets, perm = _frame_members(members, offsets, perm, song_level)
    q = _check_q(q)
    ws, vals, idx = _scratch(offsets.device, q, _lib.load().ce_select_frames_workspace_bytes(N, q))
    _call_excl("ce_select_frames", (ctypes.cast(arr, ctypes.c_void_p), len(keep), C, _p(offsets), _p(perm), N), excl, N,
               (q, int(base_idx), _p(ws), ws.numel(), _p(vals), _p(idx), _stream(offsets.device)))
    return vals, idx


def frames_consensus(members, offsets, perm=None, song_level=None, excl=None, out=None):
    """amg_test.py:426-441 from the members' FRAME-level outputs: the committee
    mean consensus_prob [N, C] float64 (ce_frames_consensus) -- per member the
    groupby(['s_id']) mean (:437), then the member-sequential mean over the
    stack (:441), the [M, N, C] stack never written.  Members, offsets, perm
    and song_level as select_frames.  excl: an optional exclusion bitmap over
    the songs; rows of excluded songs are NOT written (``out`` keeps what it
    held; a new tensor is zero there) and their frames are not read.  out: an
    optional float64 [N, C] view with unit column stride (any row stride).
    Nothing is synchronised when ``perm`` or ``song_level`` is given."""
    arr, keep, C, N, offsets, perm = _frame_members(members, offsets, perm, song_level)
    if out is None:
        out = (torch.zeros if excl is not None else torch.empty)((N, C), dtype=torch.float64, device=offsets.device)
    _on_gpu(out, "out")
    if out.dtype != torch.float64 or out.dim() != 2 or tuple(out.shape) != (N, C) or (C > 1 and out.stride(1) != 1):
        raise ValueError(f"out must be a float64 [N={N}, C={C}] view with unit column stride")
    if excl is not None:
        _check_excl(excl, N)
    call("ce_frames_consensus", ctypes.cast(arr, ctypes.c_void_p), len(keep), C, _p(offsets), _p(perm), N, _p(excl),
         _p(out), out.stride(0) if N > 1 else max(out.stride(0), C), _stream(offsets.device))
    return out


def _f64_dev(t, device, what):
    if not isinstance(t, torch.Tensor):
        t = torch.as_tensor(t)
    t = t.to(device=device, dtype=torch.float64)
    return t.contiguous()


def _check_X(X, dtypes=(torch.float64,)):
    """The frames X of a member's predict_proba: [F, D] of one of `dtypes`, unit column stride.  Returns (F, D)."""
    _on_gpu(X, "X")
    if X.dim() != 2 or X.dtype not in dtypes or X.stride(1) != 1:
        names = "/".join(str(d).split(".")[1] for d in dtypes)
        raise ValueError(f"X must be a {names} [F, D] tensor with unit column stride")
    return X.shape


def gnb_predict_proba(X, theta, var, class_prior, out=None):
    """GaussianNB(...).predict_proba(X) on the device (sklearn 0.24.1 math,
    deam_classifier.py:211; amg_test.py:435).  X [F, D] f64 frames; theta /
    var [C, D] (theta_, var_ -- sigma_ in 0.24), class_prior [C]."""
    F, D = _check_X(X)
    theta = _f64_dev(theta, X.device, "theta")
    var = _f64_dev(var, X.device, "var")
    C = theta.shape[0]
    if tuple(theta.shape) != (C, D) or tuple(var.shape) != (C, D):
        raise ValueError(f"theta/var must be [C, {D}]")
    # np.log(class_prior_[i]) (sklearn 0.24.1 _joint_log_likelihood) with the C
    # library's log, as numpy 1.19.5 evaluates it: a device prior through the
    # restated glibc log (ce_log_f64: no host sync, graph-capturable), a host
    # prior through the C library itself
    if isinstance(class_prior, torch.Tensor) and class_prior.device == X.device:
        log_prior = log_f64(class_prior.to(torch.float64).reshape(-1).contiguous())
    else:
        prior = np.asarray(class_prior.cpu() if isinstance(class_prior, torch.Tensor) else class_prior, np.float64)
        log_prior = torch.tensor([math.log(float(p)) if p > 0 else (-math.inf if p == 0 else math.nan)
                                  for p in prior.reshape(-1)], dtype=torch.float64, device=X.device)
    if out is None:
        out = torch.empty((F, C), dtype=torch.float64, device=X.device)
    call("ce_gnb_predict_proba", _p(X), F, D, X.stride(0), _p(theta), _p(var), _p(log_prior), C, _p(out),
         out.stride(0), _stream(X.device))
    return out


def sgd_predict_proba(X, coef, intercept, out=None):
    """SGDClassifier(loss='log').predict_proba(X) on the device (sklearn
    _predict_proba_lr, deam_classifier.py:214; amg_test.py:435).  coef [K, D],
    intercept [K]; K = C (OvR) or 1 (binary, C = 2)."""
    F, D = _check_X(X)
    coef = _f64_dev(coef, X.device, "coef")
    if coef.dim() == 1:
        coef = coef.unsqueeze(0)
    K = coef.shape[0]
    intercept = _f64_dev(intercept, X.device, "intercept").reshape(-1)
    C = 2 if K == 1 else K
    if coef.shape[1] != D or intercept.numel() != K:
        raise ValueError(f"coef must be [K, {D}] and intercept [K]")
    if out is None:
        out = torch.empty((F, C), dtype=torch.float64, device=X.device)
    call("ce_sgd_predict_proba", _p(X), F, D, X.stride(0), _p(coef), _p(intercept), K, C, _p(out),
         out.stride(0), _stream(X.device))
    return out


def check_users_out(out, F, C, dtypes=(torch.float64,)):
    """``out`` of the users forms: a float64 (or one of ``dtypes``) [F, C] view with unit column stride and rows
    that do not overlap."""
    if not isinstance(out, torch.Tensor) or out.dtype not in dtypes or out.dim() != 2 or \
            tuple(out.shape) != (F, C) or (C > 1 and out.stride(1) != 1) or (F > 1 and out.stride(0) < C):
        names = "/".join(str(d).split(".")[1] for d in dtypes)
        raise ValueError(f"out must be a {names} [F={F}, C={C}] view with unit column stride")


def _users_geom(item_offsets, frame_offsets, frame_perm, excl):
    """The sessions' geometry (frame_geometry) and the songs' bitmap as the C-ABI
    reads them.  Returns (U, item_offsets, frame_offsets, frame_perm)."""
    item_offsets = _i64(item_offsets, "item_offsets").reshape(-1)
    frame_offsets = _i64(frame_offsets, "frame_offsets").reshape(-1)
    U = item_offsets.numel() - 1
    if U < 1 or frame_offsets.numel() < 1:
        raise ValueError("item_offsets must hold U + 1 >= 2 entries and frame_offsets total_items + 1 >= 1")
    if frame_perm is not None:
        frame_perm = _i64(frame_perm, "frame_perm").reshape(-1)
    if excl is not None:
        _check_excl(excl, frame_offsets.numel() - 1)
    return U, item_offsets, frame_offsets, frame_perm


def _users_args(X, C, item_offsets, frame_offsets, frame_perm, excl, out, out_dtype=torch.float64,
                dtypes=(torch.float64,)):
    """The tail the users forms share: the geometry (_users_geom) and ``out``
    (a new one of ``out_dtype``; a given one of one of ``dtypes``).
    Returns (U, item_offsets, frame_offsets, frame_perm, out)."""
    F = X.shape[0]
    U, item_offsets, frame_offsets, frame_perm = _users_geom(item_offsets, frame_offsets, frame_perm, excl)
    if out is None:
        # rows of excluded songs are not written: a new tensor is zero there, the rule of frames_consensus
        if out_dtype not in dtypes:
            raise ValueError(f"out_dtype must be one of {dtypes}")
        out = (torch.zeros if excl is not None else torch.empty)((F, C), dtype=out_dtype, device=X.device)
    _on_gpu(out, "out")
    check_users_out(out, F, C, dtypes)
    return U, item_offsets, frame_offsets, frame_perm, out


def _gnb_users_model(X, theta, var, class_prior):
    """U GaussianNB models over the frames X: theta / var [U, C, D], class_prior
    [U, C] on the device.  Returns (F, D, U, C, theta, var, log_prior): the
    log-prior is one ``log_f64`` over the flat priors."""
    F, D = _check_X(X)
    theta = _f64_dev(theta, X.device, "theta")
    var = _f64_dev(var, X.device, "var")
    if theta.dim() != 3 or theta.shape[2] != D or tuple(var.shape) != tuple(theta.shape):
        raise ValueError(f"theta/var must be [U, C, {D}]")
    Um, C = theta.shape[:2]
    _on_gpu(class_prior, "class_prior")
    if class_prior.numel() != Um * C:
        raise ValueError(f"class_prior must be [U={Um}, C={C}]")
    log_prior = log_f64(class_prior.to(device=X.device, dtype=torch.float64).reshape(-1).contiguous())
    return F, D, Um, C, theta, var, log_prior


def _sgd_users_model(X, coef, intercept):
    """U SGDClassifier models over the frames X: coef [U, K, D], intercept [U, K];
    K = C (OvR) or 1 (binary, C = 2).  Returns (F, D, U, C, K, coef, intercept)."""
    F, D = _check_X(X)
    coef = _f64_dev(coef, X.device, "coef")
    if coef.dim() != 3 or coef.shape[2] != D:
        raise ValueError(f"coef must be [U, K, {D}]")
    Um, K = coef.shape[:2]
    intercept = _f64_dev(intercept, X.device, "intercept").reshape(-1)
    if intercept.numel() != Um * K:
        raise ValueError(f"intercept must be [U={Um}, K={K}]")
    return F, D, Um, 2 if K == 1 else K, K, coef, intercept


def gnb_predict_proba_users(X, theta, var, class_prior, item_offsets, frame_offsets, frame_perm=None, excl=None,
                            out=None):
    """gnb_predict_proba for U models at once (ce_gnb_predict_proba_users): every
    frame row of X [F, D] is predicted by the model of the user who owns it, in
    one launch.  theta / var [U, C, D], class_prior [U, C] (device tensors: the
    log-prior is one ``log_f64`` over the flat priors, as the one-model path
    computes it for a device prior; a zero prior gives -inf).  The geometry is
    a session's ``frame_geometry()``: stacked song g owns the rows
    frame_perm[frame_offsets[g]:frame_offsets[g+1]] (or that range itself),
    user u the stacked songs item_offsets[u]:item_offsets[u+1].  excl: an
    optional exclusion bitmap over the stacked songs; rows of excluded songs
    are NOT written and, eight consecutive frames at a time, not read.  Rows no
    song owns are not written either, and a frame_perm entry outside [0, F) is
    skipped.  out: an optional float64 [F, C] view with unit column stride (a
    new tensor is zero-filled when ``excl`` is given).  Per row the bits are
    gnb_predict_proba's.  Nothing is synchronised."""
    F, D, Um, C, theta, var, log_prior = _gnb_users_model(X, theta, var, class_prior)
    U, item_offsets, frame_offsets, frame_perm, out = _users_args(X, C, item_offsets, frame_offsets, frame_perm, excl, out)
    if U != Um:
        raise ValueError(f"item_offsets names {U} user(s), theta holds {Um} model(s)")
    call("ce_gnb_predict_proba_users", _p(X), F, D, X.stride(0), _p(theta), _p(var), _p(log_prior), C, U,
         _p(item_offsets), _p(frame_offsets), _p(frame_perm), _p(excl), _p(out), max(out.stride(0), C),
         _stream(X.device))
    return out


def sgd_predict_proba_users(X, coef, intercept, item_offsets, frame_offsets, frame_perm=None, excl=None, out=None):
    """sgd_predict_proba for U models at once (ce_sgd_predict_proba_users): coef
    [U, K, D], intercept [U, K]; K = C (OvR) or 1 (binary, C = 2).  Geometry,
    ``excl`` and ``out`` as gnb_predict_proba_users; per row the bits are
    sgd_predict_proba's."""
    F, D, Um, C, K, coef, intercept = _sgd_users_model(X, coef, intercept)
    U, item_offsets, frame_offsets, frame_perm, out = _users_args(X, C, item_offsets, frame_offsets, frame_perm, excl, out)
    if U != Um:
        raise ValueError(f"item_offsets names {U} user(s), coef holds {Um} model(s)")
    call("ce_sgd_predict_proba_users", _p(X), F, D, X.stride(0), _p(coef), _p(intercept), K, C, U,
         _p(item_offsets), _p(frame_offsets), _p(frame_perm), _p(excl), _p(out), max(out.stride(0), C),
         _stream(X.device))
    return out


def _labels_i32(y, F):
    """The labels of a score launch as the C-ABI reads them: one encoded class per ROW of X, int32 [F] on the device."""
    _on_gpu(y, "y")
    if y.dim() != 1 or y.numel() != F or y.dtype not in (torch.int32, torch.int64, torch.int16, torch.int8, torch.uint8):
        raise ValueError(f"y must be an integer [F={F}] tensor: one encoded class per row of X")
    if y.dtype == torch.int32 and y.is_contiguous():
        return y
    return y.to(torch.int32).contiguous()


def _score_args(X, C, score_cols, U_models, item_offsets, frame_offsets, frame_perm, excl, y, return_pred,
                return_scores, scores_dtype=torch.float64):
    """The tail the score launches share.  Returns (U, item_offsets,
    frame_offsets, frame_perm, y, cm, pred, scores): cm a new int64 [U, C, C]
    (the entry point zero-fills it), pred a new int32 [F] of -1 and scores a new
    float64 (``scores_dtype``) [F, score_cols] of NaN where asked for -- what a
    row that is not counted keeps."""
    F = X.shape[0]
    U, item_offsets, frame_offsets, frame_perm = _users_geom(item_offsets, frame_offsets, frame_perm, excl)
    if U != U_models:
        raise ValueError(f"item_offsets names {U} user(s), the member holds {U_models} model(s)")
    y = _labels_i32(y, F)
    cm = torch.empty((U, C, C), dtype=torch.int64, device=X.device)
    pred = torch.full((F,), -1, dtype=torch.int32, device=X.device) if return_pred else None
    scores = torch.full((F, score_cols), math.nan, dtype=scores_dtype, device=X.device) if return_scores else None
    return U, item_offsets, frame_offsets, frame_perm, y, cm, pred, scores


def gnb_score_users(X, theta, var, class_prior, item_offsets, frame_offsets, y, frame_perm=None, excl=None,
                    return_pred=False, return_scores=False):
    """The evaluate step of an epoch for U GaussianNB models in one launch
    (ce_gnb_score_users; amg_test.py:513, ``mod.predict(X_test.values)``, and
    the counts :515's f1_score is formed from).  X [F, D] f64 holds every
    user's TEST frames, ``y`` [F] their encoded classes by row of X; the
    geometry (an EvalSet's ``frame_geometry()``) and the models are those of
    gnb_predict_proba_users.  Every owned row is labelled by the model of its
    user -- np.argmax of the joint log-likelihood, whose bits are the ones
    gnb_predict_proba_users forms before its logsumexp -- and counted in
    cm[u, y, pred].  A row whose label is outside [0, C), whose song is
    excluded or that no song owns is not counted.  Returns (cm int64 [U, C, C],
    pred int32 [F] or None, scores f64 [F, C] or None); rows not counted keep
    -1 in pred and NaN in scores.  Nothing is synchronised."""
    F, D, Um, C, theta, var, log_prior = _gnb_users_model(X, theta, var, class_prior)
    U, item_offsets, frame_offsets, frame_perm, y, cm, pred, scores = _score_args(
        X, C, C, Um, item_offsets, frame_offsets, frame_perm, excl, y, return_pred, return_scores)
    call("ce_gnb_score_users", _p(X), F, D, X.stride(0), _p(theta), _p(var), _p(log_prior), C, U, _p(item_offsets),
         _p(frame_offsets), _p(frame_perm), _p(excl), _p(y), _p(cm), _p(pred), _p(scores), C, _stream(X.device))
    return cm, pred, scores


def sgd_score_users(X, coef, intercept, item_offsets, frame_offsets, y, frame_perm=None, excl=None, return_pred=False,
                    return_scores=False):
    """gnb_score_users for U SGDClassifier models (ce_sgd_score_users): coef
    [U, K, D], intercept [U, K]; K = C (one-vs-rest: np.argmax of the decision
    values) or 1 (binary, C = 2: decision > 0 is class 1).  The decision values
    are the ones sgd_predict_proba_users feeds to expit, bit for bit; scores is
    [F, K]."""
    F, D, Um, C, K, coef, intercept = _sgd_users_model(X, coef, intercept)
    U, item_offsets, frame_offsets, frame_perm, y, cm, pred, scores = _score_args(
        X, C, K, Um, item_offsets, frame_offsets, frame_perm, excl, y, return_pred, return_scores)
    call("ce_sgd_score_users", _p(X), F, D, X.stride(0), _p(coef), _p(intercept), K, C, U, _p(item_offsets),
         _p(frame_offsets), _p(frame_perm), _p(excl), _p(y), _p(cm), _p(pred), _p(scores), K, _stream(X.device))
    return cm, pred, scores


def f1_weighted_users(cm, report=False):
    """sklearn 1.7.2's ``f1_score(y_true, y_pred, average='weighted')`` of every
    user from their counts (ce_f1_weighted_users; amg_test.py:515): cm int64
    [U, C, C], cm[u, true, predicted].  Returns f1 f64 [U] (NaN for a user
    without a counted row), and with report=True (f1, prf [U, C, 4]): every
    class's precision, recall, F1 and support, the numbers of
    classification_report (:514)."""
    _on_gpu(cm, "cm")
    if cm.dim() != 3 or cm.shape[1] != cm.shape[2] or cm.dtype != torch.int64 or cm.shape[0] < 1:
        raise ValueError("cm must be an int64 [U, C, C] tensor")
    cm = cm.contiguous()
    U, C = cm.shape[:2]
    f1 = torch.empty(U, dtype=torch.float64, device=cm.device)
    prf = torch.empty((U, C, 4), dtype=torch.float64, device=cm.device) if report else None
    call("ce_f1_weighted_users", _p(cm), U, C, _p(f1), _p(prf), _stream(cm.device))
    return (f1, prf) if report else f1


def _fit_state(t, what, shape=None):
    """A tensor the partial_fit updates in place: float64, contiguous, on the device (no copy may stand in)."""
    _on_gpu(t, what)
    if t.dtype != torch.float64 or not t.is_contiguous() or (shape is not None and tuple(t.shape) != shape):
        want = f" of shape {list(shape)}" if shape is not None else ""
        raise ValueError(f"{what} must be a contiguous float64 tensor{want} (it is updated in place)")
    return t


def gnb_partial_fit(X, rows, labels, theta, var, class_count, row_offsets=None, var_smoothing=1e-9, *,
                    class_prior=None, epsilon=None):
    """GaussianNB.partial_fit on the device (ce_gnb_partial_fit; amg_test.py:509,
    mod.partial_fit(X_batch.values, y_batch_enc)) for U fitted models at once.
    X [F, D] f64 frames; model u's batch is the rows ``rows[row_offsets[u]:
    row_offsets[u+1]]`` of X, row i of class ``labels[i]`` in [0, C), in
    X_train's order (ascending; ``batch_rows`` builds them from picked songs).
    theta / var [U, C, D] and class_count [U, C] (or [C, D], [C, D], [C] for one
    model) are float64 device tensors UPDATED IN PLACE; row_offsets=None means
    one model owning every row (built on the device: capturable).  Returns
    (class_prior [U, C], epsilon [U]) -- into ``class_prior`` / ``epsilon``
    when given; a model with an empty batch is left untouched, these two slots
    included (NaN in fresh outputs), and with no row at all nothing is launched.
    Bit-identical to sklearn's update; D = 1 is refused."""
    F, D = _check_X(X)
    rows = _i64(rows, "rows").reshape(-1)
    _on_gpu(labels, "labels")
    labels = labels.reshape(-1).to(torch.int32).contiguous()
    if labels.numel() != rows.numel():
        raise ValueError(f"labels must hold one class per row ({rows.numel()}), got {labels.numel()}")
    one = theta.dim() == 2 if isinstance(theta, torch.Tensor) else False
    _fit_state(theta, "theta")
    if theta.dim() not in (2, 3) or theta.shape[-1] != D:
        raise ValueError(f"theta must be [U, C, {D}] (or [C, {D}] for one model)")
    U, C = (1, theta.shape[0]) if one else tuple(theta.shape[:2])
    _fit_state(var, "var", tuple(theta.shape))
    _fit_state(class_count, "class_count", tuple(theta.shape[:-1]))
    if row_offsets is None:
        if U != 1:
            raise ValueError(f"{U} models need row_offsets [U + 1]")
        # [0, n] by two device kernels: no host-to-device copy, so the call stays capturable
        row_offsets = torch.arange(2, dtype=torch.int64, device=X.device) * rows.numel()
    row_offsets = _i64(row_offsets, "row_offsets").reshape(-1)
    if row_offsets.numel() != U + 1:
        raise ValueError(f"row_offsets must hold U + 1 = {U + 1} entries")
    lead = tuple(theta.shape[:-2])
    if class_prior is None:
        class_prior = torch.full(lead + (C,), math.nan, dtype=torch.float64, device=X.device)
    if epsilon is None:
        epsilon = torch.full(lead or (1,), math.nan, dtype=torch.float64, device=X.device)
    _fit_state(class_prior, "class_prior", tuple(theta.shape[:-1]))
    _fit_state(epsilon, "epsilon")
    if epsilon.numel() != U:
        raise ValueError(f"epsilon must hold one value per model ({U})")
    if rows.numel() == 0:  # every batch is empty (an epoch that picked nothing): every model stays as it is
        return class_prior, epsilon
    call("ce_gnb_partial_fit", _p(X), F, D, X.stride(0), _p(rows), _p(labels), _p(row_offsets), U, C,
         float(var_smoothing), _p(theta), _p(var), _p(class_count), _p(class_prior), _p(epsilon), _stream(X.device))
    return class_prior, epsilon


SGD_GRADS = {"half_binomial": 0, "log_dloss": 1}  # sklearn >= 1.x (pinned: 1.7.2) / sklearn 0.24.1's Log.dloss
_INT32_MAX = int(np.iinfo(np.int32).max)


def sgd_chain_seeds(random_state, C):
    """The shuffle seeds of one SGDClassifier.partial_fit call, uint32 [K]
    (K = C one-vs-rest problems, 1 for C = 2) -- the host rule, numpy's legacy
    MT19937 as sklearn draws from it.  An integer random_state re-seeds on
    every call, so the seeds are the same for every call: for C > 2
    ``RandomState(random_state).randint(INT32_MAX, size=C)`` seeds one
    RandomState per problem (C = 2: RandomState(random_state) itself); each
    gives one draw to make_dataset (``randint(1, INT32_MAX)``, discarded) and
    the next, ``randint(INT32_MAX)``, seeds the shuffle.  random_state=None
    cannot be reproduced and is refused."""
    if isinstance(random_state, bool) or not isinstance(random_state, (int, np.integer)):
        raise ValueError("sgd_chain_seeds needs an integer random_state (None or a generator cannot be reproduced)")
    if not 2 <= int(C) <= 8:
        raise ValueError(f"C must be in [2, 8], got {C}")
    if C > 2:
        chains = [np.random.RandomState(int(s))
                  for s in np.random.RandomState(int(random_state)).randint(_INT32_MAX, size=int(C))]
    else:
        chains = [np.random.RandomState(int(random_state))]
    out = []
    for rs in chains:
        rs.randint(1, _INT32_MAX)  # make_dataset's draw
        out.append(rs.randint(_INT32_MAX))
    return np.array(out, dtype=np.uint32)


def sgd_optimal_init(alpha):
    """learning_rate='optimal': the offset of t in eta = 1 / (alpha * (optimal_init + t - 1)),
    computed the way _plain_sgd does (the half-binomial gradient at (1, -typw) is negative for every alpha)."""
    alpha = float(alpha)
    if not (alpha > 0 and math.isfinite(alpha)):
        raise ValueError(f"alpha must be positive and finite, got {alpha}")
    typw = math.sqrt(1.0 / math.sqrt(alpha))
    p = -typw
    if p > -37.0:
        e = math.exp(-p)
        g = ((1.0 - 1.0) - 1.0 * e) / (1.0 + e)
    else:
        g = math.exp(p) - 1.0
    return 1.0 / ((typw / max(1.0, g)) * alpha)


def sgd_partial_fit(X, rows, labels, coef, intercept, t, row_offsets=None, alpha=1e-4, *, seeds,
                    grad="half_binomial", status=None):
    """SGDClassifier(loss='log', penalty='l2').partial_fit on the device
    (ce_sgd_partial_fit; amg_test.py:509 for the 'classifier_sgd' member,
    deam_classifier.py:214-217) for U models at once.  X [F, D] f64 frames;
    model u's batch is the rows ``rows[row_offsets[u]:row_offsets[u+1]]`` of X,
    row i of class ``labels[i]`` in [0, C), in X_train's order (``batch_rows``
    builds them): the shuffle starts from the order given.  coef [U, K, D],
    intercept [U, K] and t [U] (or [K, D], [K], [1] for one model; K = C, or 1
    for C = 2) are float64 device tensors UPDATED IN PLACE; row_offsets=None
    means one model owning every row.  ``seeds``: the shuffle seeds [U, K] (or
    [K]): ``sgd_chain_seeds(random_state, C)`` per model, or a device tensor
    of them (int32; what a captured call needs).  ``grad``: "half_binomial"
    (sklearn >= 1.x; bit-identical to 1.7.2) or "log_dloss" (sklearn 0.24.1's,
    unpinned).  Returns ``status`` int32 [U] (zeroed when not given; only ever
    set): 1 where a model's intercept or a weight is non-finite after the
    update (sklearn raises there), 2 where a model was not run.  A model with
    an empty batch is left untouched, its t included, and with no row at all
    nothing is launched."""
    F, D = _check_X(X)
    rows = _i64(rows, "rows").reshape(-1)
    _on_gpu(labels, "labels")
    labels = labels.reshape(-1).to(torch.int32).contiguous()
    if labels.numel() != rows.numel():
        raise ValueError(f"labels must hold one class per row ({rows.numel()}), got {labels.numel()}")
    if grad not in SGD_GRADS:
        raise ValueError(f"grad must be one of {sorted(SGD_GRADS)}, got {grad!r}")
    one = coef.dim() == 2 if isinstance(coef, torch.Tensor) else False
    _fit_state(coef, "coef")
    if coef.dim() not in (2, 3) or coef.shape[-1] != D:
        raise ValueError(f"coef must be [U, K, {D}] (or [K, {D}] for one model)")
    U, K = (1, coef.shape[0]) if one else tuple(coef.shape[:2])
    if not 1 <= K <= 8 or K == 2:
        raise ValueError(f"coef holds K = {K} binary problems: K = 1 (two classes) or 3 .. 8 (one per class)")
    C = 2 if K == 1 else K
    _fit_state(intercept, "intercept", tuple(coef.shape[:-1]))
    _fit_state(t, "t")
    if t.numel() != U:
        raise ValueError(f"t must hold one step count per model ({U})")
    if row_offsets is None:
        if U != 1:
            raise ValueError(f"{U} models need row_offsets [U + 1]")
        # [0, n] by two device kernels: no host-to-device copy, so the call stays capturable
        row_offsets = torch.arange(2, dtype=torch.int64, device=X.device) * rows.numel()
    row_offsets = _i64(row_offsets, "row_offsets").reshape(-1)
    if row_offsets.numel() != U + 1:
        raise ValueError(f"row_offsets must hold U + 1 = {U + 1} entries")
    if not isinstance(seeds, torch.Tensor):  # host seeds (uint32): their bit patterns, as int32
        seeds = torch.from_numpy(np.ascontiguousarray(seeds).astype(np.uint32).view(np.int32)).to(X.device)
    _on_gpu(seeds, "seeds")
    seeds = seeds.to(torch.int32).contiguous()
    if seeds.numel() != U * K:
        raise ValueError(f"seeds must hold one shuffle seed per model and problem ({U} x {K})")
    if status is None:
        status = torch.zeros(U, dtype=torch.int32, device=X.device)
    _on_gpu(status, "status")
    if status.dtype != torch.int32 or not status.is_contiguous() or status.numel() != U:
        raise ValueError(f"status must be a contiguous int32 tensor of {U} flags")
    optimal_init = sgd_optimal_init(alpha)
    if rows.numel() == 0:  # every batch is empty (an epoch that picked nothing): every model stays as it is
        return status
    ws_bytes = int(_lib.load().ce_sgd_partial_fit_workspace_bytes(rows.numel(), C))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=X.device) if ws_bytes else None  # written before it is read
    call("ce_sgd_partial_fit", _p(X), F, D, X.stride(0), _p(rows), _p(labels), _p(row_offsets), U, C, float(alpha),
         optimal_init, _p(seeds), SGD_GRADS[grad], _p(coef), _p(intercept), _p(t), _p(status), _p(ws), ws_bytes,
         _stream(X.device))
    return status


def batch_rows(songs, frame_offsets, frame_perm=None, song_labels=None, item_offsets=None, n_classes=None,
               max_rows=None):
    """From picked songs to X_batch's rows -- amg_test.py:491,
    ``X_train[X_train.index.isin(q_songs)]``, for one user or U: the frame rows
    of the picked songs in X_train's order (ascending row, not pick order), a
    song picked twice taken once.  ``songs``: picked song positions [q], or
    [U, q] with -1 padding (every -1 is dropped); with ``item_offsets`` [U + 1]
    they are user-local and user u's song s is stacked song item_offsets[u] + s.
    A position outside the user's pool is an error when ``songs`` arrives from
    the host (with host or no ``item_offsets``); on the device it is dropped
    like -1, never mapped onto another user's song.
    Song g owns the rows frame_perm[frame_offsets[g]:frame_offsets[g+1]] (or
    that range itself): the CSR the sessions keep.  ``song_labels``: the class
    of every (stacked) song; from the host it is checked against [0, n_classes).
    Returns (rows int64 [R], labels int32 [R], row_offsets int64 [U + 1]), each
    user's rows ascending, on frame_offsets' device -- torch ops only, so CPU
    tensors work too; R is the one size read back from the device
    (repeat_interleave), everything else is sorts, scans and scatters.
    ``max_rows`` (a host number no batch exceeds, e.g. the pool's frame count):
    nothing is read back -- what a HIP-graph capture needs; rows and labels
    then hold max_rows entries, the R = row_offsets[U] real ones first and
    padding (an in-range row, owned by no model) behind them, which the
    partial_fit kernels never read."""
    if not isinstance(frame_offsets, torch.Tensor):
        frame_offsets = torch.as_tensor(np.asarray(frame_offsets, dtype=np.int64))
    dev = frame_offsets.device
    off = frame_offsets.to(torch.int64).reshape(-1)
    n_songs = off.numel() - 1

    def idx(t):
        return None if t is None else torch.as_tensor(t).to(device=dev, dtype=torch.int64)

    if song_labels is None:
        raise ValueError("batch_rows needs song_labels, the class of every song")
    if not isinstance(song_labels, torch.Tensor):
        host = np.asarray(getattr(song_labels, "values", song_labels))
        if n_classes is not None and host.size and (host.min() < 0 or host.max() >= n_classes):
            raise ValueError(f"song_labels must lie in [0, {n_classes})")
        song_labels = torch.from_numpy(np.ascontiguousarray(host).astype(np.int64))
    lab = song_labels.to(device=dev, dtype=torch.int64).reshape(-1)
    if lab.numel() != n_songs:
        raise ValueError(f"song_labels must hold one class per song ({n_songs}), got {lab.numel()}")
    if not isinstance(songs, torch.Tensor) and not isinstance(item_offsets, torch.Tensor):  # host picks: check them
        hs = np.asarray(songs, dtype=np.int64)
        hs = hs.reshape(1, -1) if hs.ndim < 2 else hs.reshape(hs.shape[0], -1)
        pool = (np.full(hs.shape[0], n_songs) if item_offsets is None
                else np.diff(np.asarray(item_offsets, dtype=np.int64).reshape(-1))[:hs.shape[0]])
        if len(pool) == hs.shape[0] and ((hs < -1) | (hs >= pool[:, None])).any():
            raise ValueError("songs must be positions in the user's pool, or -1")
    S = idx(songs)
    S = S.reshape(1, -1) if S.dim() < 2 else S.reshape(S.shape[0], -1)
    U = S.shape[0]
    row_offsets = torch.zeros(U + 1, dtype=torch.int64, device=dev)
    if item_offsets is not None:
        io = idx(item_offsets).reshape(-1)
        if io.numel() != U + 1:
            raise ValueError(f"item_offsets must hold U + 1 = {U + 1} entries")
        G, pool = S + io[:-1].unsqueeze(1), (io[1:] - io[:-1]).unsqueeze(1)
    else:
        G, pool = S, n_songs
    if n_songs == 0 or S.numel() == 0 or (max_rows is not None and int(max_rows) <= 0):
        return S.new_zeros(0), torch.zeros(0, dtype=torch.int32, device=dev), row_offsets
    # (user, song) keys in user-then-song order; a slot that names no song gets the key past every user
    user = torch.arange(U, device=dev).unsqueeze(1)
    valid = (S >= 0) & (S < pool) & (G < n_songs)
    key, _ = torch.sort(torch.where(valid, user * n_songs + G, U * n_songs).reshape(-1))
    first = key < U * n_songs  # the first slot of every key: a song picked twice is taken once
    first[1:] &= key[1:] != key[:-1]
    uu, g = (key // n_songs).clamp(max=U - 1), key % n_songs
    cnt = torch.where(first, off[g + 1] - off[g], 0)
    slots = torch.arange(key.numel(), device=dev)
    if max_rows is None:
        seg = torch.repeat_interleave(slots, cnt)  # the one size read-back
    else:  # a fixed size: output entry i belongs to the first slot whose running count passes i
        out_i, total = torch.arange(int(max_rows), device=dev), torch.cumsum(cnt, 0)
        real = out_i < total[-1]
        seg = torch.where(real, torch.searchsorted(total, out_i, right=True).clamp(max=key.numel() - 1), 0)
    start = torch.cumsum(cnt, 0) - cnt
    rows = off[g][seg] + (torch.arange(seg.numel(), device=dev) - start[seg])
    ruser, rlab = uu[seg], lab[g][seg]
    if max_rows is not None:  # padding: position 0, past every user
        rows, ruser = torch.where(real, rows, 0), torch.where(real, ruser, U)
    if frame_perm is not None:  # permuted frames: a song's rows are scattered, so order each user's rows again
        rows = idx(frame_perm).reshape(-1)[rows]
        rows, o = torch.sort(rows, stable=True)
        ruser, rlab = ruser[o], rlab[o]
        ruser, o = torch.sort(ruser, stable=True)
        rows, rlab = rows[o], rlab[o]
    row_offsets[1:] = torch.cumsum(torch.zeros(U, dtype=torch.int64, device=dev).index_add_(0, uu, cnt), 0)
    return rows, rlab.to(torch.int32), row_offsets


def xgb_predict_proba(X, forest, out=None, out_dtype=torch.float32):
    """XGBClassifier(...).predict_proba(X) on the device (xgboost 1.3.3
    predictor restated in csrc/ce_xgb.hpp and ce_xgb_walk.hpp;
    xgboost/sklearn.py:991-1029, amg_test.py:435).  X [F, D] f32/f64 frames
    (cast to float32 like DMatrix, NaN = missing); ``forest`` an
    ``ce_amd.xgb.XgbForest`` (or its JSON).  Returns [F, C] ``out_dtype``
    (float32 = what xgboost returns; float64 = its exact upcast, ready for a
    committee stack)."""
    F, D = _check_X(X, (torch.float32, torch.float64))
    if not isinstance(forest, XgbForest):
        forest = XgbForest.from_json(forest)
    if forest.max_feature() >= D:
        raise ValueError(f"the forest splits on feature {forest.max_feature()} but X has {D} columns")
    G, C = forest.n_groups, forest.n_classes
    if out is None:
        out = torch.empty((F, C), dtype=out_dtype, device=X.device)
    if out.dim() != 2 or out.shape[0] != F or out.shape[1] < C or out.stride(1) != 1 or out.dtype not in _DT:
        raise ValueError(f"out must be a float [{F}, >={C}] tensor with unit column stride")
    nodes, leaves, goff, depth = forest.device_arrays(X.device)
    if depth <= LANE_TABLE_DEPTH:  # the reference's max_depth=5: prebuilt per-tree lane tables
        table = forest.lane_table(X.device, D)
        call("ce_xgb_predict_proba_lanes", _p(X), _DT[X.dtype], F, D, X.stride(0), _p(table), table.shape[1],
             _p(goff), G, depth, float(forest.base_margin), C, _p(out), _DT[out.dtype], out.stride(0),
             _stream(X.device))
    else:
        call("ce_xgb_predict_proba", _p(X), _DT[X.dtype], F, D, X.stride(0), _p(nodes), _p(leaves), _p(goff), G,
             depth, float(forest.base_margin), C, _p(out), _DT[out.dtype], out.stride(0), _stream(X.device))
    return out


_XGB_DT = (torch.float32, torch.float64)


def _xgb_users_model(X, stacked):
    """The stacked forests of U users over the frames X.  Returns (F, D, the
    entry points' forest arguments) -- the lane table is built for X's D on
    first use (outside a capture) and cached."""
    F, D = _check_X(X, _XGB_DT)
    if not isinstance(stacked, StackedForests):
        raise TypeError("stacked must be a ce_amd.xgb.StackedForests")
    if stacked.max_feature >= D:
        raise ValueError(f"the forests split on feature {stacked.max_feature} but X has {D} columns")
    table, cap, ids, L, goff, depth = stacked.device_args(X.device, D)
    return F, D, (_p(table), cap, _p(ids), L, _p(goff), stacked.G, depth, stacked.base_margin, stacked.C)


XGB_FIT_MAX_ROWS = 4096  # kXgbFitMaxRows: rows of one user's batch
XGB_FIT_MAX_DEPTH = 5    # kXgbFitMaxDepth
_XGB_FIT_NODES = 63


def xgb_fit_users(X, rows, labels, stacked, row_offsets=None, n_rounds=100, max_depth=5, *, eta=0.3, reg_lambda=1.0,
                  min_child_weight=1.0, gamma=0.0, alpha=0.0, objective="multi:softprob", sample_weight=None,
                  status=None, return_margins=False):
    """``XGBClassifier(max_depth).fit(X[rows], labels, xgb_model=booster)`` on
    the device for U forests at once (ce_xgb_fit_users; amg_test.py:507):
    ``n_rounds`` boosting rounds are grown on every user's batch on top of its
    current forest and appended to ``stacked`` (a ``ce_amd.xgb.StackedForests``),
    whose walks see them from the next call on.  X [F, D] f32/f64 frames (cast
    to float32 like DMatrix; the batch must be dense and finite); user u's
    batch is ``rows[row_offsets[u]:row_offsets[u+1]]`` of class ``labels[i]`` in
    [0, C), in X_train's order (``batch_rows`` builds them); row_offsets=None
    means one forest owning every row.  The arithmetic is the restatement of
    tests/xgb_fit_ref.py, bit for bit (multi:softprob, exact grower, dense
    columns); parity with xgboost 1.3.3 is unpinned.  Refused before any
    launch: gamma or alpha other than 0, any objective but multi:softprob,
    sample weights, max_depth above 5, D > 512, more than 4096 rows of one user.
    ``status`` int32 [U] (zeroed when not given; only ever set): 1 where a
    batch holds a non-finite value (that forest is left unchanged), 2 where it
    was not run.  A user without rows gets no new tree.  Two small copies cross
    the bus (row_offsets before the launch, the flags after it) and none of the
    trees; the call synchronises and is not graph-capturable.  Returns a dict:
    ``status``, ``active`` (host bool [U]: who got trees), ``trees`` (the
    ``ce_amd.xgb.GrownTrees`` appended, its arrays on the device), ``margins``
    (f32 [R, C], the batch's final margins, with return_margins)."""
    from .xgb import GrownTrees

    # what the fit does not take is refused first, from host values alone
    if not isinstance(stacked, StackedForests):
        raise TypeError("stacked must be a ce_amd.xgb.StackedForests")
    if objective != "multi:softprob" or stacked.G < 2 or stacked.G != stacked.C:
        raise ValueError(f"xgb_fit_users grows multi:softprob forests only (objective {objective!r}, "
                         f"{stacked.G} group(s))")
    if float(gamma) != 0.0 or float(alpha) != 0.0:
        raise ValueError(f"gamma and alpha must be 0 (no pruning, no L1 term), got gamma={gamma} alpha={alpha}")
    if sample_weight is not None:
        raise ValueError("sample weights are not supported")
    n_rounds, max_depth = int(n_rounds), int(max_depth)
    if n_rounds < 1:
        raise ValueError(f"n_rounds must be at least 1, got {n_rounds}")
    if not 1 <= max_depth <= XGB_FIT_MAX_DEPTH:
        raise ValueError(f"max_depth must lie in [1, {XGB_FIT_MAX_DEPTH}], got {max_depth}")
    for name, v, lo in (("eta", eta, None), ("reg_lambda", reg_lambda, 0.0), ("min_child_weight", min_child_weight, 0.0)):
        v = float(v)
        if not math.isfinite(v) or (lo is None and v <= 0.0) or (lo is not None and v < lo):
            raise ValueError(f"{name} out of range: {v}")
    F, D = _check_X(X, _XGB_DT)
    if D > MAX_FEATURES:
        raise ValueError(f"X has {D} features: at most {MAX_FEATURES}")
    if stacked.max_feature >= D:
        raise ValueError(f"the forests split on feature {stacked.max_feature} but X has {D} columns")
    U, C = stacked.U, stacked.C
    rows = _i64(rows, "rows").reshape(-1)
    _on_gpu(labels, "labels")
    labels = labels.reshape(-1).to(torch.int32).contiguous()
    if labels.numel() != rows.numel():
        raise ValueError(f"labels must hold one class per row ({rows.numel()}), got {labels.numel()}")
    if row_offsets is None:
        if U != 1:
            raise ValueError(f"{U} forests need row_offsets [U + 1]")
        ro_host = np.array([0, rows.numel()], dtype=np.int64)
        row_offsets = torch.from_numpy(ro_host).to(X.device)
    else:
        row_offsets = _i64(row_offsets, "row_offsets").reshape(-1)
        if row_offsets.numel() != U + 1:
            raise ValueError(f"row_offsets must hold U + 1 = {U + 1} entries")
        ro_host = row_offsets.cpu().numpy()
    counts = np.diff(ro_host)
    if ro_host[0] != 0 or (counts < 0).any() or ro_host[-1] > rows.numel():
        raise ValueError("row_offsets must start at 0, ascend and end within rows")
    R, n_max = int(ro_host[-1]), int(counts.max(initial=0))
    if n_max > XGB_FIT_MAX_ROWS:
        raise ValueError(f"a user's batch holds {n_max} rows: at most {XGB_FIT_MAX_ROWS}")
    if status is None:
        status = torch.zeros(U, dtype=torch.int32, device=X.device)
    _on_gpu(status, "status")
    if status.dtype != torch.int32 or not status.is_contiguous() or status.numel() != U:
        raise ValueError(f"status must be a contiguous int32 tensor of {U} flags")
    out = {"status": status, "active": np.zeros(U, dtype=bool), "trees": None, "margins": None}
    if R == 0:  # every batch is empty (an epoch that picked nothing): every forest stays as it is
        return out
    stacked.ensure_depth(max_depth)  # a deeper fit: the stack is packed again at the new depth, once
    table, cap, ids, L, goff, depth = stacked.device_args(X.device, D)
    dev, T = X.device, U * n_rounds * C
    NI, NL = max((1 << depth) - 1, 1), 1 << depth
    t = {"nodes": torch.zeros((T, NI, 2), dtype=torch.int32, device=dev),
         "leaves": torch.zeros((T, NL), dtype=torch.float32, device=dev),
         "left": torch.full((T, _XGB_FIT_NODES), -1, dtype=torch.int32, device=dev),
         "right": torch.full((T, _XGB_FIT_NODES), -1, dtype=torch.int32, device=dev),
         "split": torch.zeros((T, _XGB_FIT_NODES), dtype=torch.int32, device=dev),
         "cond": torch.zeros((T, _XGB_FIT_NODES), dtype=torch.float32, device=dev),
         "default_left": torch.zeros((T, _XGB_FIT_NODES), dtype=torch.uint8, device=dev),
         "num_nodes": torch.zeros(T, dtype=torch.int32, device=dev)}
    margins = torch.zeros((R, C), dtype=torch.float32, device=dev) if return_margins else None
    flags = torch.zeros(U, dtype=torch.int32, device=dev)
    ws_bytes = int(_lib.load().ce_xgb_fit_workspace_bytes(R, n_max, D, C, n_rounds))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
    call("ce_xgb_fit_users", _p(X), _DT[X.dtype], F, D, X.stride(0), _p(rows), _p(labels), _p(row_offsets), U, R, n_max,
         _p(table), cap, _p(ids), L, _p(goff), C, depth, float(stacked.base_margin), n_rounds, max_depth, float(eta),
         float(reg_lambda), float(min_child_weight), _p(t["nodes"]), _p(t["leaves"]), _p(t["left"]), _p(t["right"]),
         _p(t["split"]), _p(t["cond"]), _p(t["default_left"]), _p(t["num_nodes"]), _p(margins), _p(flags), _p(ws),
         ws_bytes, _stream(dev))
    fl = flags.cpu().numpy()  # the one read-back after the launch: who got trees
    status.copy_(torch.maximum(status, flags))
    out["active"] = (counts > 0) & (fl == 0)
    out["trees"] = GrownTrees(t, U, n_rounds, C, depth, out["active"])
    out["margins"] = margins
    stacked.grow(out["trees"], dev, D, D - 1)
    return out


def xgb_predict_proba_users(X, stacked, item_offsets, frame_offsets, frame_perm=None, excl=None, out=None,
                            out_dtype=torch.float32):
    """xgb_predict_proba for U forests at once (ce_xgb_predict_proba_users):
    every frame row of X [F, D] f32/f64 is predicted by the forest of the user
    who owns it, in one launch.  ``stacked``: a ``ce_amd.xgb.StackedForests``
    (the shared base trees once, every user's own after them; depth <= 5).
    Geometry, ``excl`` and ``out`` as gnb_predict_proba_users, with ``out``
    float32 (what xgboost returns) or float64 (its exact upcast); per row the
    bits are xgb_predict_proba's with that user's full model.  Nothing is
    synchronised."""
    F, D, forest = _xgb_users_model(X, stacked)
    U, item_offsets, frame_offsets, frame_perm, out = _users_args(
        X, stacked.C, item_offsets, frame_offsets, frame_perm, excl, out, out_dtype, _XGB_DT)
    if U != stacked.U:
        raise ValueError(f"item_offsets names {U} user(s), stacked holds {stacked.U} forest(s)")
    call("ce_xgb_predict_proba_users", _p(X), _DT[X.dtype], F, D, X.stride(0), *forest, U, _p(item_offsets),
         _p(frame_offsets), _p(frame_perm), _p(excl), _p(out), _DT[out.dtype], max(out.stride(0), stacked.C),
         _stream(X.device))
    return out


def xgb_score_users(X, stacked, item_offsets, frame_offsets, y, frame_perm=None, excl=None, return_pred=False,
                    return_proba=False):
    """gnb_score_users for U XGBoost forests (ce_xgb_score_users;
    amg_test.py:513): every owned row is labelled by XGBClassifier.predict's
    rule on the float32 probabilities xgb_predict_proba_users forms
    (xgboost/sklearn.py:981-985: np.argmax of the probabilities, or p > 0.5 for
    a binary model) and counted in cm[u, y, pred].  Returns (cm int64 [U, C, C],
    pred int32 [F] or None, proba f32 [F, C] or None); rows not counted keep -1
    in pred and NaN in proba.  Nothing is synchronised."""
    F, D, forest = _xgb_users_model(X, stacked)
    U, item_offsets, frame_offsets, frame_perm, y, cm, pred, proba = _score_args(
        X, stacked.C, stacked.C, stacked.U, item_offsets, frame_offsets, frame_perm, excl, y, return_pred,
        return_proba, torch.float32)
    call("ce_xgb_score_users", _p(X), _DT[X.dtype], F, D, X.stride(0), *forest, U, _p(item_offsets), _p(frame_offsets),
         _p(frame_perm), _p(excl), _p(y), _p(cm), _p(pred), _p(proba), stacked.C, _stream(X.device))
    return cm, pred, proba


def _check_q(q):
    """Any q >= 0, as the reference's -q (amg_test.py:547-553).  Outputs hold q
    slots (padding -- val NaN, idx -1 -- past the pool); q <= CE_MAX_Q runs on
    the list kernels, larger q on the sort path (workspace grows with N)."""
    q = int(q)
    if q < 0:
        raise ValueError(f"q={q} is negative")
    if q > _Q_ABI_MAX:  # every entry point takes q as int32 (ctypes would truncate it silently)
        raise ValueError(f"q={q} exceeds the C-ABI's int32 q; clamp it to the pool size (min(q, N)) first")
    return q


_Q_ABI_MAX = 2**31 - 1


def _sort_path(q):
    """q > CE_MAX_Q runs on the sort path: its workspace is per call (see _WorkspaceCache)."""
    return q > _lib.CE_MAX_Q


def _outs(q, device, lead=()):
    return (torch.empty(lead + (q,), dtype=torch.float64, device=device),
            torch.empty(lead + (q,), dtype=torch.int64, device=device))


def _scratch(device, q, ws_bytes, lead=()):
    """What a selecting call needs besides its inputs: (workspace of ws_bytes, vals, idx)."""
    return (WORKSPACE.get(device, ws_bytes, _sort_path(q)), *_outs(q, device, lead))


def _call_excl(name, head, excl, n, tail):
    """call(name, *head, *tail); with a bitmap over n items, the entry point
    name + "_excl", which takes the bitmap between head and tail."""
    if excl is None:
        call(name, *head, *tail)
    else:
        _check_excl(excl, n)
        call(name + "_excl", *head, _p(excl), *tail)


def topq(ent, q, base_idx=0):
    """np.argsort(ent)[::-1][:q] under the total order (NaN first, desc, lowest
    index).  Returns (vals [q], idx [q]); idx = -1 marks empty slots."""
    _on_gpu(ent, "ent")
    q = _check_q(q)
    ent = ent.contiguous().to(torch.float64)
    N = ent.numel()
    ws, vals, idx = _scratch(ent.device, q, _lib.load().ce_topq_workspace_bytes(N, q))
    call("ce_topq", _p(ent), N, q, int(base_idx), _p(ws), ws.numel(), _p(vals), _p(idx), _stream(ent.device))
    return vals, idx


def topq_merge(vals, idx, q):
    """Merge best-first candidate lists of q slots each (e.g. per-GPU top-q
    after an all-gather) into the global top-q."""
    _on_gpu(vals, "vals")
    q = _check_q(q)
    vals = vals.contiguous().view(-1)
    idx = idx.contiguous().view(-1)
    if q == 0:
        return _outs(0, vals.device)
    if vals.numel() != idx.numel() or vals.numel() == 0 or vals.numel() % q:
        raise ValueError("vals/idx must hold nlists * q entries")
    ov, oi = _outs(q, vals.device)
    call("ce_topq_merge", _p(vals), _p(idx), vals.numel() // q, q, _p(ov), _p(oi), _stream(vals.device))
    return ov, oi


def select_mc(P, q, layout="MNC", base_idx=0, excl=None):
    """Fused amg_test.py:441-445: (vals [q], idx [q]) best-first.  excl: an
    optional exclusion bitmap (int32 [ceil(N/32)], bit i set = item i is out
    of the pool), see excl_bitmap / mark_selected."""
    comm = _committee_args(P, layout)
    N = comm[2]
    q = _check_q(q)
    ws, vals, idx = _scratch(P.device, q, _lib.load().ce_select_mc_workspace_bytes(N, q))
    _call_excl("ce_select_mc", comm, excl, N,
               (q, int(base_idx), _p(ws), ws.numel(), _p(vals), _p(idx), _stream(P.device)))
    return vals, idx


def excl_bitmap(n, device=None):
    """An all-clear exclusion bitmap for n items (int32 words on the device)."""
    words = _lib.load().ce_excl_words(int(n))
    return torch.zeros(max(int(words), 1), dtype=torch.int32, device=device)


def _check_excl(excl, n):
    _on_gpu(excl, "excl")
    if excl.dtype != torch.int32 or not excl.is_contiguous() or excl.numel() * 32 < n:
        raise ValueError(f"excl must be a contiguous int32 bitmap of >= {(n + 31) // 32} words")


def mark_selected(excl, n, idx, base_idx=0):
    """Set the bitmap bits of the selected positions idx (device int64; -1
    slots ignored) -- stream-ordered after the selection that produced them."""
    _check_excl(excl, n)
    idx = _i64(idx, "idx")
    call("ce_mark_selected", _p(excl), int(n), _p(idx), idx.numel(), int(base_idx), _stream(excl.device))


class MCPlan:
    """Pre-bound mc selection with its own workspace and outputs: what the
    bench and the multi-GPU driver launch every step.  step() / step_cands()
    run the whole selection in one launch; partial() + finish() /
    finish_cands() are the two stages as separate launches."""

    def __init__(self, P, q, layout="NMC", base_idx=0):
        self.P = P
        self.comm = _committee_args(P, layout)  # every launch splats it
        _, self.dt, self.N, self.M, self.C, self.sN, self.sM, self.sC = self.comm
        self.q = _check_q(q)
        self.base_idx = int(base_idx)
        lib = _lib.load()
        self.ws_bytes = lib.ce_select_mc_workspace_bytes(self.N, self.q)
        self.ws = new_workspace(self.ws_bytes, P.device)
        self.vals, self.idx = _outs(self.q, P.device)

    def partial(self):
        call("ce_select_mc_partial", *self.comm, self.q, self.base_idx, _p(self.ws), self.ws_bytes,
             _stream(self.P.device))

    def finish(self):
        call("ce_select_finish", self.N, self.q, _p(self.ws), self.ws_bytes, _p(self.vals), _p(self.idx),
             _stream(self.P.device))
        return self.vals, self.idx

    def finish_cands(self, out=None):
        """Stage 2 writing this pool's q candidate records (ce_cand: order key,
        position; as an int64 [q, 2] tensor) -- the all-gather send buffer of
        the multi-GPU merge.  partial() / finish*() need q <= CE_MAX_Q."""
        if out is None:
            out = torch.empty((self.q, 2), dtype=torch.int64, device=self.P.device)
        call("ce_select_finish_cands", self.N, self.q, _p(self.ws), self.ws_bytes, _p(out), _stream(self.P.device))
        return out

    def step(self):
        """The whole selection (ce_select_mc; ONE launch for q <= 64: stage 2
        folded into stage 1's last block): (vals [q], idx [q])."""
        call("ce_select_mc", *self.comm, self.q, self.base_idx, _p(self.ws), self.ws_bytes, _p(self.vals),
             _p(self.idx), _stream(self.P.device))
        return self.vals, self.idx

    def step_cands(self, out=None):
        """This pool's q candidate records (int64 [q, 2], the multi-GPU send
        buffer; ce_select_mc_cands, ONE launch for q <= 64)."""
        if out is None:
            out = torch.empty((self.q, 2), dtype=torch.int64, device=self.P.device)
        call("ce_select_mc_cands", *self.comm, self.q, self.base_idx, _p(self.ws), self.ws_bytes, _p(out),
             _stream(self.P.device))
        return out

    def __call__(self):
        return self.step()


def merge_cands(cands, q):
    """Merge nlists lists of q candidate records (int64 [nlists*q, 2] or
    [nlists, q, 2], each list best-first -- e.g. the all-gather receive buffer)
    into the final (vals [q], idx [q])."""
    _on_gpu(cands, "cands")
    q = _check_q(q)
    if cands.dtype != torch.int64 or cands.shape[-1] != 2 or not cands.is_contiguous():
        raise ValueError("cands must be a contiguous int64 [..., 2] tensor of records")
    n = cands.numel() // 2
    if q == 0 or n == 0 or n % q:
        if q == 0:
            return _outs(0, cands.device)
        raise ValueError("cands must hold nlists * q records")
    ov, oi = _outs(q, cands.device)
    call("ce_merge_cands", _p(cands), n // q, q, _p(ov), _p(oi), _stream(cands.device))
    return ov, oi


class MCChunkJob:
    """amg_test.py:441-445 over a pool larger than HBM (BASELINE configs[4]),
    streamed as consecutive chunks: ``add(P_chunk)`` scores one resident chunk
    (pool positions continue from the previous chunk) and folds its top-q into
    a running list of q candidate records on the device; ``result()`` is the
    selection over everything added -- identical to select_mc on the whole
    pool, ties included (any q)."""

    def __init__(self, q, layout="NMC", device=None):
        self.q = _check_q(q)
        self.layout = layout
        self.device = torch.device(device) if device is not None else None
        self.running = None
        self.n_items = 0
        self._fresh = True
        self._ranges = []  # [lo, hi) position ranges added so far

    def add(self, P, base_idx=None):
        """Score chunk P (layout as constructed); its items are pool positions
        base_idx .. base_idx + N - 1 (default: right after the previous chunk)."""
        comm = _committee_args(P, self.layout)
        N = comm[2]
        if self.running is None:
            if self.device is not None and self.device.index is not None and P.device != self.device:
                raise ValueError(f"chunk on {P.device}, job on {self.device}")
            self.running = torch.empty((self.q, 2), dtype=torch.int64, device=P.device)
        elif P.device != self.running.device:
            raise ValueError(f"chunk on {P.device}, but the job's running list lives on {self.running.device}")
        base = self.n_items if base_idx is None else int(base_idx)
        if base < 0:
            raise ValueError(f"base_idx must be >= 0, got {base}")
        for lo, hi in self._ranges:  # a position scored twice would be merged silently
            if base < hi and lo < base + N:
                raise ValueError(f"chunk positions [{base}, {base + N}) overlap an added chunk [{lo}, {hi})")
        if N > 0:
            self._ranges.append((base, base + N))
        lib = _lib.load()
        ws = WORKSPACE.get(P.device, lib.ce_select_mc_chunk_workspace_bytes(N, self.q), _sort_path(self.q))
        first = 1 if self._fresh else 0
        call("ce_select_mc_chunk", *comm, self.q, base, _p(self.running), first, _p(ws), ws.numel(),
             _stream(P.device))
        self._fresh = False
        self.n_items = max(self.n_items, base + N)
        return self

    def running_records(self, device=None):
        """The running list: q candidate records (int64 [q, 2], best first; an
        empty list -- key 0, idx -1 -- when no chunk was added), e.g. the send
        buffer of the multi-GPU all-gather."""
        if self.running is None:
            dev = device if device is not None else (self.device or torch.device("cuda", torch.cuda.current_device()))
            empty = torch.zeros((self.q, 2), dtype=torch.int64, device=dev)
            empty[:, 1] = -1
            return empty
        return self.running

    def result(self):
        """(vals [q], idx [q]) best-first over every chunk added (idx -1 padding)."""
        if self.running is None:
            raise ValueError("no chunk added")
        return merge_cands(self.running, self.q)


def select_mc_chunks(chunks, q, layout="NMC"):
    """Convenience over MCChunkJob: ``chunks`` yields consecutive device tensors
    (or (tensor, base_idx) pairs) of one pool."""
    job = None
    for ch in chunks:
        P, base = ch if isinstance(ch, tuple) else (ch, None)
        if job is None:
            job = MCChunkJob(q, layout, P.device)
        job.add(P, base)
    if job is None:
        raise ValueError("no chunks")
    return job.result()


def _hc_table(hc, C, rows="N_h"):
    """The hc table as the mix entry points read it: float64 [rows, C], unit column stride."""
    _on_gpu(hc, "hc table")
    if hc.dim() != 2 or hc.shape[1] != C:
        raise ValueError(f"hc table must be [{rows}, {C}]")
    hc = hc.to(torch.float64)
    return hc if hc.stride(1) == 1 else hc.contiguous()


def select_mix(P, hc, q, layout="MNC"):
    """Fused amg_test.py:473-480: top-q over the row stack [mc (N); hc (N_h)]."""
    comm = _committee_args(P, layout)
    N, C = comm[2], comm[4]
    hc = _hc_table(hc, C)
    q = _check_q(q)
    N_h = hc.shape[0]
    ws, vals, idx = _scratch(P.device, q, _lib.load().ce_select_mix_workspace_bytes(N, N_h, q))
    call("ce_select_mix", *comm, _p(hc), N_h, hc.stride(0), q, _p(ws), ws.numel(), _p(vals), _p(idx),
         _stream(P.device))
    return vals, idx


def _user_offsets(offsets, what="offsets", U=None):
    offsets = _i64(offsets, what)
    if offsets.numel() < 2 or (U is not None and offsets.numel() != U + 1):
        raise ValueError(f"{what} must hold U + 1 >= 2 entries" + (f" (U = {U})" if U is not None else ""))
    return offsets


def select_batched(P, offsets, q, layout="MNC", excl=None):
    """U users in one launch; user u owns items offsets[u]:offsets[u+1].
    Returns (vals [U, q], idx [U, q]) with user-local positions.  excl: an
    optional exclusion bitmap over the GLOBAL item index offsets[u] + i (int32
    [ceil(N/32)], see excl_bitmap / mark_selected_batched): each user's
    selection runs over the items whose bit is clear."""
    comm = _committee_args(P, layout)
    N = comm[2]
    offsets = _user_offsets(offsets)
    U = offsets.numel() - 1
    q = _check_q(q)
    ws, vals, idx = _scratch(P.device, q, _lib.load().ce_select_batched_workspace_bytes(N, U, q), (U,))
    _call_excl("ce_select_batched", (*comm, _p(offsets), U), excl, N,
               (q, _p(ws), ws.numel(), _p(vals), _p(idx), _stream(P.device)))
    return vals, idx


def select_batched_mix(P, offsets, hc, hc_offsets, q, layout="MNC", excl=None, excl_h=None):
    """amg_test.py:473-480 for U users in one launch: user u's row stack
    [committee items offsets[u]:offsets[u+1]; rows hc_offsets[u]:hc_offsets[u+1]
    of the stacked tables hc [total_h, C]].  Returns (vals [U, q], idx [U, q]),
    user-local positions: i < N_u a committee item, N_u + j hc row j.  excl /
    excl_h: optional bitmaps over the global item / hc row index.  The engine
    runs C = 4, q <= 64 (CEError otherwise: BatchedSelectionSession composes)."""
    comm = _committee_args(P, layout)
    N, C = comm[2], comm[4]
    hc = _hc_table(hc, C, "total_h")
    offsets = _user_offsets(offsets)
    U = offsets.numel() - 1
    hc_offsets = _user_offsets(hc_offsets, "hc_offsets", U)
    q = _check_q(q)
    Nh = hc.shape[0]
    if excl is not None:
        _check_excl(excl, N)
    if excl_h is not None:
        _check_excl(excl_h, Nh)
    ws, vals, idx = _scratch(P.device, q, _lib.load().ce_select_batched_mix_workspace_bytes(N, Nh, U, q), (U,))
    call("ce_select_batched_mix", *comm, _p(offsets), _p(hc), Nh, hc.stride(0), _p(hc_offsets), U, _p(excl),
         _p(excl_h), q, _p(ws), ws.numel(), _p(vals), _p(idx), _stream(P.device))
    return vals, idx


def mark_selected_batched(idx, offsets, excl, hc_offsets=None, excl_h=None, m2h=None, h2m=None):
    """Set the bits of a batched selection's picks idx [U, q] (user-local
    positions, -1 ignored): a position below N_u marks global item offsets[u] +
    p in excl (and hc row m2h[item] in excl_h), one above it hc row
    hc_offsets[u] + p - N_u in excl_h (and item h2m[row] in excl).  The maps
    hold global indices, -1 = no twin.  Stream-ordered, nothing leaves the GPU."""
    idx = _i64(idx, "idx")
    offsets = _user_offsets(offsets)
    U = offsets.numel() - 1
    if idx.dim() != 2 or idx.shape[0] != U:
        raise ValueError(f"idx must be [U = {U}, q]")
    _check_excl(excl, 0)
    if hc_offsets is not None:
        hc_offsets = _user_offsets(hc_offsets, "hc_offsets", U)
    for name, t in (("excl_h", excl_h), ("m2h", m2h), ("h2m", h2m)):
        if t is not None:
            _on_gpu(t, name)
            if t.dtype != (torch.int32 if name == "excl_h" else torch.int64) or not t.is_contiguous():
                raise ValueError(f"{name} must be a contiguous {'int32 bitmap' if name == 'excl_h' else 'int64 map'}")
    call("ce_mark_selected_batched", _p(idx), U, idx.shape[1], _p(offsets), _p(excl), _p(hc_offsets), _p(excl_h),
         _p(m2h), _p(h2m), _stream(excl.device))
