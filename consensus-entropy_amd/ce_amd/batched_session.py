"""Device-resident multi-epoch selection for U users at once.

The reference's hot loop is users x epochs x mode (amg_test.py:345, :396-397,
:425-489): every user has their own pool, and it shrinks every epoch
(:455/:484 the hc frame, :521-531 X_train).  ``SelectionSession`` keeps ONE
user's full pool on the device with an exclusion bitmap; a
``BatchedSelectionSession`` does the same for all U users, epoch-major: each
epoch is one selection launch over every user's remaining songs and one mark
launch, instead of a Python loop of about five small launches per user.

The users' pools are stacked: user u owns items ``offsets[u]:offsets[u+1]`` of
the committee tensor (and rows ``hc_offsets[u]:hc_offsets[u+1]`` of the stacked
hc tables).  The bitmaps are over the stacked (global) indices.  Positions
returned are positions in each user's FULL pool, stable across epochs, with
the conventions of ``SelectionSession``: in mix mode i in [0, N_u) is committee
item i and N_u + j is row j of the user's table, which keeps its own row order.

Modes:
  mc    one ``ops.select_batched(excl=)`` and one mark per epoch.  Built with
        ``frame_offsets`` (the CSR of the frame rows over the stacked songs,
        optionally ``frame_perm``), ``step(frames=[...])`` takes the members'
        FRAME-level outputs: one ``ops.frames_consensus`` over all users'
        remaining songs writes the committee mean rows (amg_test.py:437-441)
        into a buffer the session owns, and the selection reads them as a
        one-member committee -- three launches per epoch, mix included
  hc    the same over the stacked tables as a one-member f64 committee
  mix   one ``ops.select_batched_mix`` and one mark.  ``hc_to_mc`` is a flat
        [total_h] array: per hc row, the user-local committee item of the same
        song, or -1 (the song is not in that user's committee pool).  A pick
        through either part removes the song from both (:484 + :521-531).
        The engine runs the mix in one launch for C = 4 and q <= 64; any other
        shape is composed from two ``select_batched(excl=)`` calls and a
        per-user ``ops.topq_merge`` -- the same picks, many more launches.
  rand  not offered: the reference draws user by user from ONE global MT19937
        stream (np.random.seed(1987), :55; the user loop, :345), so user u's
        epoch-e draw comes after ALL of user u-1's epochs.  An epoch-major
        batch cannot reproduce that order of draws; run one
        ``SelectionSession("rand")`` per user, user-major, as the reference does.

``select`` reads the picks back (one [U, q] copy per epoch).  ``step`` is the
device half alone -- select + mark, nothing synchronised, capturable in a HIP
graph -- and ``account`` the host half for picks read back later.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .select import MODES, _device, _hc_tensor, frame_member_tensors, stack_committee
from .session import mix_songs, songs_leaving, twin_maps

_MIX_KERNEL_MAX_Q = 64  # include/ce.h: ce_select_batched_mix runs C = 4, q <= 64


def _offsets_host(offsets, what, n=None, count="U + 1 >= 2"):
    """Offsets as an int64 host array: `n` entries when given (at least 2
    otherwise), non-decreasing and >= 0."""
    o = np.asarray(offsets.cpu() if isinstance(offsets, torch.Tensor) else offsets, dtype=np.int64).reshape(-1)
    if n is not None and o.shape[0] != n:
        raise ValueError(f"{what} must hold {count} = {n} entries (got {o.shape[0]})")
    if (n is None and o.shape[0] < 2) or o[0] < 0 or (np.diff(o) < 0).any():
        raise ValueError(f"{what} must hold {count} non-decreasing entries >= 0")
    return o


class BatchedSelectionSession:
    def __init__(self, queries, mode, offsets, *, hc=None, hc_offsets=None, hc_to_mc=None, device=None,
                 frame_offsets=None, frame_perm=None, n_classes=4):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        if mode == "rand":
            raise ValueError("BatchedSelectionSession has no rand mode: the reference draws user by user from one "
                             "global RNG stream, which an epoch-major batch cannot reproduce; use one "
                             "SelectionSession('rand') per user")
        self.q = int(queries)
        if self.q < 0:
            raise ValueError(f"queries = {self.q} is negative")
        self.mode = mode
        # ---- host-side geometry and validation (before any device work)
        off = _offsets_host(offsets, "offsets")
        self.U = off.shape[0] - 1
        off_h = None
        if mode in ("hc", "mix"):
            off_h = off if hc_offsets is None else _offsets_host(hc_offsets, "hc_offsets")
            if off_h.shape[0] != off.shape[0]:
                raise ValueError(f"hc_offsets must hold U + 1 = {self.U + 1} entries")
            if hc is None:
                raise ValueError("hc/mix modes need `hc`, the users' frequency tables stacked [total_h, C]")
            if not hasattr(hc, "shape"):
                hc = np.asarray(hc, dtype=np.float64)
            if len(hc.shape) != 2 or hc.shape[0] != off_h[-1]:
                raise ValueError(f"hc must be [total_h = {off_h[-1]}, C], the users' tables one after the other")
        if mode == "hc":  # the pool IS the table
            off = off_h
        self._off, self._off_h = off, off_h
        self.n_items = np.diff(off)
        self.n_rows = np.diff(off_h) if mode == "mix" else None
        h2m_g = m2h_g = None
        if mode == "mix":
            self._h2m_local, h2m_g, m2h_g = twin_maps(hc_to_mc, off, off_h)
        # frame-level members (step(frames=...)): the CSR of the frame rows over the STACKED songs
        f_off = f_perm = None
        if frame_perm is not None and frame_offsets is None:
            raise ValueError("frame_perm needs frame_offsets")
        if frame_offsets is not None:
            if mode == "hc":
                raise ValueError("frame_offsets (frame-level members) has no use in mode 'hc': it selects from no "
                                 "committee")
            f_off = _offsets_host(frame_offsets, "frame_offsets", int(off[-1]) + 1, "total_items + 1")
            if frame_perm is not None:
                f_perm = np.asarray(frame_perm.cpu() if isinstance(frame_perm, torch.Tensor) else frame_perm,
                                    dtype=np.int64).reshape(-1)
                if f_perm.shape[0] < f_off[-1] or (f_perm < 0).any():
                    raise ValueError(f"frame_perm must hold frame_offsets[-1] = {int(f_off[-1])} row indices >= 0")
            self._F = int(f_off[-1])
            self._song_frames = int(np.diff(f_off).max()) if len(f_off) > 1 else 0  # the longest song
            # rows of X the geometry names (host numbers: a member's predict_proba_session checks X against it)
            self._rows = int(f_perm[:self._F].max()) + 1 if f_perm is not None and self._F else self._F
        self.remaining = self.n_items.copy()
        # ---- device state
        self.dev = _device(device)
        self.offsets = torch.from_numpy(off).to(self.dev)
        self.excl = ops.excl_bitmap(int(off[-1]), self.dev)
        self.H = self.hc_offsets = self.excl_h = self.h2m = self.m2h = None
        if mode in ("hc", "mix"):
            self.H = _hc_tensor(hc, None, None, self.dev).to(torch.float64).contiguous()
        if mode == "mix":
            self.hc_offsets = torch.from_numpy(off_h).to(self.dev)
            self.excl_h = ops.excl_bitmap(self.H.shape[0], self.dev)
            self.h2m = torch.from_numpy(h2m_g).to(self.dev)
            self.m2h = torch.from_numpy(m2h_g).to(self.dev)
            self._n_dev = torch.from_numpy(self.n_items).to(self.dev).unsqueeze(1)
        self.frame_offsets = self.frame_perm = self._cons = None
        if f_off is not None:
            self.frame_offsets = torch.from_numpy(f_off).to(self.dev)
            self.frame_perm = torch.from_numpy(f_perm).to(self.dev) if f_perm is not None else None
            # the consensus rows of every user's remaining songs (ops.frames_consensus writes no row of an
            # excluded song): allocated and zeroed once, so an epoch allocates nothing
            C = self.H.shape[1] if mode == "mix" else int(n_classes)
            self._cons = torch.zeros((int(off[-1]), C), dtype=torch.float64, device=self.dev)

    def _slots(self):
        """Output slots per user: q, but never more than the largest user's
        pools hold, so a huge q costs no huge buffers."""
        n = self.n_items + (self.n_rows if self.mode == "mix" else 0)
        return int(min(self.q, n.max())) if self.U else 0

    def _committee(self, committee, layout):
        if committee is None:
            raise ValueError(f"{self.mode} mode needs `committee`")
        P, lay = stack_committee(committee, self.dev, layout)
        n = P.shape[1] if lay == "MNC" else P.shape[0]
        if n != self._off[-1]:
            raise ValueError(f"committee covers {n} items, the users' pools hold {self._off[-1]}")
        return P, lay

    def _consensus(self, frames):
        """frames -> the consensus rows of the remaining songs of every user
        (one launch), as a one-member committee ((+0.0 + x) / 1 is x)."""
        total = int(self._off[-1])
        ts, sl = frame_member_tensors(frames, total, self._F, self.frame_perm is None, self.dev)
        if ts[0].shape[1] != self._cons.shape[1]:
            raise ValueError(f"members have {ts[0].shape[1]} classes, the session was built for {self._cons.shape[1]}")
        ops.frames_consensus(ts, self.frame_offsets, self.frame_perm, sl, excl=self.excl, out=self._cons)
        return self._cons.unsqueeze(1), "NMC"

    def step(self, committee=None, layout="MNC", *, frames=None, _compose=False):
        """One epoch on the device: selects every user's picks among their
        remaining songs and marks them.  Returns idx [U, slots] (int64 device
        tensor, -1 padding); nothing is synchronised and ``remaining`` is not
        touched -- ``account`` does that once the picks are on the host.
        ``frames`` (a session built with ``frame_offsets``; instead of
        ``committee``): the members' outputs over every user's frame rows,
        [F, C] frame-level or [total_items, C] song-level; three launches
        (consensus rows, select, mark) for any number of users and members."""
        if frames is not None:
            if committee is not None:
                raise ValueError("pass `committee` or `frames`, not both")
            if self._cons is None:
                raise ValueError("`frames` needs a session built with frame_offsets (the frame rows' CSR)")
        qs = self._slots()
        if self.mode == "hc":
            _, idx = ops.select_batched(self.H.unsqueeze(1), self.offsets, qs, "NMC", excl=self.excl)
            ops.mark_selected_batched(idx, self.offsets, self.excl)
            return idx
        P, lay = self._consensus(frames) if frames is not None else self._committee(committee, layout)
        if self.mode == "mc":
            _, idx = ops.select_batched(P, self.offsets, qs, lay, excl=self.excl)
            ops.mark_selected_batched(idx, self.offsets, self.excl)
            return idx
        C = P.shape[2]
        if _compose or qs > _MIX_KERNEL_MAX_Q or C != 4:
            idx = self._mix_composed(P, lay, qs)
        else:
            _, idx = ops.select_batched_mix(P, self.offsets, self.H, self.hc_offsets, qs, lay, excl=self.excl,
                                            excl_h=self.excl_h)
        ops.mark_selected_batched(idx, self.offsets, self.excl, self.hc_offsets, self.excl_h, self.m2h, self.h2m)
        return idx

    def _mix_composed(self, P, lay, qs):
        """The mix epoch from the parts: each part's top-q per user, the hc
        positions shifted by N_u, one merge per user (correct for any C and q;
        U + 2 launches)."""
        vm, im = ops.select_batched(P, self.offsets, qs, lay, excl=self.excl)
        vh, ih = ops.select_batched(self.H.unsqueeze(1), self.hc_offsets, qs, "NMC", excl=self.excl_h)
        ih = torch.where(ih >= 0, ih + self._n_dev, ih)
        idx = torch.empty_like(im)
        if qs:
            for u in range(self.U):
                _, idx[u] = ops.topq_merge(torch.cat([vm[u], vh[u]]), torch.cat([im[u], ih[u]]), qs)
        return idx

    def account(self, idx):
        """The host half of an epoch: idx [U, slots] as ``step`` returned it ->
        a list of U int64 arrays (each user's picks, best first) and the
        ``remaining`` counts updated."""
        rows = np.asarray(idx.cpu() if isinstance(idx, torch.Tensor) else idx, dtype=np.int64).reshape(self.U, -1)
        out = []
        for u in range(self.U):
            r = rows[u][rows[u] >= 0]
            out.append(r)
            if self.mode == "mix":
                self.remaining[u] -= songs_leaving(r, self.n_items[u],
                                                   self._h2m_local[self._off_h[u]:self._off_h[u + 1]])
            else:
                self.remaining[u] -= len(r)
        return out

    def frame_geometry(self):
        """(frame_offsets [total_items + 1], frame_perm [F] or None, offsets
        [U + 1]) on the device: stacked song g owns the rows
        frame_perm[frame_offsets[g]:frame_offsets[g+1]], user u the stacked songs
        offsets[u]:offsets[u+1] (a session built with ``frame_offsets``)."""
        if self.frame_offsets is None:
            raise ValueError("this session was built without frame_offsets: it holds no frame geometry")
        return self.frame_offsets, self.frame_perm, self.offsets

    def songs_of(self, picks):
        """The committee song positions (user-local) behind an epoch's picks,
        i.e. every user's q_songs at amg_test.py:491: in mc mode the picks
        themselves; in mix mode an hc pick N_u + j goes through hc_to_mc and -1
        twins are dropped (session.mix_songs).  ``picks``: the list of U arrays
        ``select`` / ``account`` return -> a list of U int64 arrays, duplicates
        merged; or the device tensor [U, slots] of ``step`` -> a device tensor
        of that shape, -1 where a slot names no song (nothing is read back; a
        song picked through both parts stands twice, ops.batch_rows merges it)."""
        if self.mode == "hc":
            raise ValueError("mode 'hc' selects from no committee: its picks name no committee songs")
        if isinstance(picks, torch.Tensor):
            if self.mode == "mc":
                return picks
            n, lo = self._n_dev, self.offsets[:-1].unsqueeze(1)
            row = (self.hc_offsets[:-1].unsqueeze(1) + picks - n).clamp(0, max(self.H.shape[0] - 1, 0))
            twin = self.h2m[row] if self.H.shape[0] else torch.full_like(picks, -1)
            via_hc = torch.where(twin >= 0, twin - lo, twin)
            return torch.where(picks < 0, picks, torch.where(picks < n, picks, via_hc))
        if len(picks) != self.U:
            raise ValueError(f"picks must hold one array per user ({self.U})")
        out = []
        for u, r in enumerate(picks):
            r = np.asarray(r, dtype=np.int64).reshape(-1)
            out.append(mix_songs(r, self.n_items[u], self._h2m_local[self._off_h[u]:self._off_h[u + 1]])
                       if self.mode == "mix" else r[r >= 0])
        return out

    def select(self, committee=None, layout="MNC", *, frames=None, _compose=False):
        """One epoch: a list of U int64 arrays -- each user's picked positions
        in their full pool, best first, fewer when a pool runs dry -- and the
        picks leave the pools.  _compose (private, tests): force the composed
        mix path."""
        return self.account(self.step(committee, layout, frames=frames, _compose=_compose))
