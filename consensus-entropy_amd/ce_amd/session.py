"""Device-resident multi-epoch selection.

The reference shrinks its pools on the host every epoch: the queried songs
leave X_train / id_tr (amg_test.py:521-531) and the hc frame
(``this_consensus_hc[~index.isin(q_songs)]``, :455, :484), and the next epoch's
``pred_prob`` is computed over what is left.  A ``SelectionSession`` keeps the
FULL pool on the device instead, with one exclusion bitmap per pool: each
epoch the caller hands in the committee's probabilities over the full pool
(e.g. from on-device member inference), the engine selects among the items
whose bit is clear, and marks the picks -- no pool bookkeeping crosses PCIe,
only the q picked positions come back.

Positions returned are positions in the FULL pool (stable across epochs), so
the caller maps them to song ids once.  Selection per epoch equals the
reference's on the shrunken pool (tests/test_gpu_parity.py::test_session_*).

Modes (amg_test.py:425-489):
  mc    committee over the full pool [M, N, C] (or [N, M, C]), excluding queried items;
        or, built with ``s_id`` (the song id of every frame row of the full
        X_train), the members' FRAME-level outputs: ``select(frames=[...])`` runs
        the groupby mean (:437), the committee mean, the entropy and the top-q
        over the remaining songs in one launch (ops.select_frames(excl=)), with
        no [M, N, C] stack and no offsets rebuilt as the pool shrinks.  In mix
        the frames give the consensus rows (ops.frames_consensus) the mix reads.
        Positions then index ``song_ids`` (the sorted unique ids, :437's rows)
  hc    the human-consensus table, fixed at construction, excluding queried rows
  mix   both.  The hc table keeps the reference's OWN row order (annotation
        order, :359/:376), not the committee's (sorted s_id, :437), so the
        lowest-position tie-break inside the hc segment of [mc; hc] (:477) is
        the reference's; ``hc_to_mc[j]`` names the committee item of hc row j
        (-1: the song is not in the committee's pool).  A pick through either
        part removes the song from both, as :484 + :521-531 do by id.
        Positions: i in [0, N) = committee item i, N + j = hc row j (the row
        stack [mc; hc] of select_queries, over the full pools)
  rand  amg_test.py:486-489: ``pos_songs = X_train.index.unique().tolist();
        np.random.shuffle(pos_songs); pos_songs[:q]`` -- the legacy shuffle of
        the REMAINING songs in the order they first appear in X_train.
        ``rand_order`` gives that order as positions (the pool position of the
        first song of X_train, of the second, ...); the remaining songs keep it
        as the pool shrinks (a DataFrame drop keeps row order), so with the
        caller's RandomState (or the global one the reference seeds with
        np.random.seed(1987), :55) the picks are the reference's, draw for
        draw.  Default: ascending positions, i.e. X_train's songs appear in
        position order.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .select import MODES, _device, _hc_tensor, frame_member_tensors, groupby_device, stack_committee


def twin_maps(hc_to_mc, offsets, hc_offsets, pool="N_u"):
    """The mix twin maps of U users, on the host.  ``hc_to_mc``: per hc row the
    user-local committee item of the same song or -1 (None: the identity, only
    when the pools coincide); ``offsets`` / ``hc_offsets``: int64 [U + 1].
    Returns (h2m local [total_h], h2m global [total_h], m2h global
    [total_items]), global = stacked indices, -1 = no twin.  ``pool`` names a
    user's pool size in the range error."""
    n_items, total_h = np.diff(offsets), int(hc_offsets[-1])
    if hc_to_mc is None:
        if not np.array_equal(hc_offsets, offsets):
            raise ValueError("mix: pass hc_to_mc (user-local committee item of each hc row) when the hc pools "
                             "(hc_offsets) differ from the committee pools (offsets)")
        h2m = np.concatenate([np.arange(n) for n in n_items] + [np.zeros(0, np.int64)])
    else:
        h2m = np.asarray(hc_to_mc, dtype=np.int64).reshape(-1)
    if h2m.shape[0] != total_h:
        raise ValueError(f"hc_to_mc must hold one entry per hc row ({total_h})")
    h2m_g = np.full(total_h, -1, np.int64)
    m2h_g = np.full(int(offsets[-1]), -1, np.int64)
    for u in range(len(n_items)):
        rows = np.arange(hc_offsets[u], hc_offsets[u + 1])
        loc = h2m[rows]
        if (loc >= n_items[u]).any() or (loc < -1).any():
            raise ValueError(f"hc_to_mc must give, per hc row, a committee item in [0, {pool}) or -1 (user {u})")
        ok = loc >= 0
        if len(np.unique(loc[ok])) != ok.sum():
            raise ValueError(f"hc_to_mc maps two hc rows to one committee item (user {u})")
        h2m_g[rows[ok]] = offsets[u] + loc[ok]
        m2h_g[offsets[u] + loc[ok]] = rows[ok]
    return h2m, h2m_g, m2h_g


def mix_songs(picks, n_items, h2m_rows):
    """The committee songs behind a user's mix picks, stated once (amg_test.py
    :484 + :491, ``isin(q_songs)``).  ``picks``: the user's picked positions
    (>= 0; i < n_items a committee item, n_items + j hc row j); ``h2m_rows``: the
    user's local hc_to_mc.  A pick through either part counts, a song picked
    through both once, and an hc pick of a song outside the pool (twin -1) names
    no committee song.  Returns the sorted unique positions."""
    picks = np.asarray(picks, dtype=np.int64).reshape(-1)
    picks = picks[picks >= 0]
    via_hc = h2m_rows[picks[picks >= n_items] - n_items]
    return np.unique(np.concatenate([picks[picks < n_items], via_hc[via_hc >= 0]]))


def songs_leaving(picks, n_items, h2m_rows):
    """Songs that leave a user's committee pool after a mix epoch: mix_songs,
    counted (an hc pick whose twin is -1 leaves only the table)."""
    return len(mix_songs(picks, n_items, h2m_rows))


class SelectionSession:
    def __init__(self, queries, mode, n_items, *, hc=None, votes=None, hc_to_mc=None, rng=None, device=None,
                 n_classes=4, rand_order=None, s_id=None):
        if mode not in MODES:
            raise ValueError(f"mode must be one of {MODES}, got {mode!r}")
        self.q = int(queries)
        if self.q < 0:  # any other q, as the reference's -q (amg_test.py:547-553)
            raise ValueError(f"queries = {self.q} is negative")
        self.mode = mode
        self.N = int(n_items)
        self.dev = _device(device)
        # frame-level members (select(frames=...)): the groupby geometry of the FULL X_train, on the device once
        self.song_ids = None
        if s_id is not None:
            if mode in ("hc", "rand"):
                raise ValueError(f"s_id (frame-level members) has no use in mode {mode!r}: it selects from no committee")
            self.song_ids, n, self._F, self._f_off, self._f_perm = groupby_device(s_id, self.dev)
            if n != self.N:
                raise ValueError(f"s_id names {n} songs, n_items is {self.N}")
            self._rows = self._F  # rows of X the geometry names: the grouping permutation covers 0 .. F - 1
            self._song_frames = int(np.unique(np.asarray(getattr(s_id, "values", s_id)), return_counts=True)[1].max()) if n else 0
            self._items = torch.tensor([0, n], dtype=torch.int64).to(self.dev)  # one user owning every song
        self.rng = rng
        self.H = None
        if mode in ("hc", "mix"):
            self.H = _hc_tensor(hc, votes, n_classes, self.dev).to(torch.float64).contiguous()
            if mode == "hc":
                self.N = self.H.shape[0]
        self.excl = ops.excl_bitmap(self.N, self.dev)
        self.n_selected = 0
        if self.song_ids is not None:
            # mix: the consensus rows of the remaining songs, a one-member committee for the mix path
            self._cons = (torch.zeros((self.N, self.H.shape[1]), dtype=torch.float64, device=self.dev)
                          if mode == "mix" else None)
        self.rand_order = None
        if mode == "rand":
            order = np.arange(self.N) if rand_order is None else np.asarray(rand_order, dtype=np.int64).reshape(-1)
            if order.shape[0] != self.N or not np.array_equal(np.sort(order), np.arange(self.N)):
                raise ValueError("rand_order must be a permutation of the n_items pool positions")
            self.rand_order = order
        if mode == "mix":
            self.Nh = self.H.shape[0]
            # one user: the global maps are the local ones; the host copy counts the songs leaving the pool
            self._h2m_host, h2m, m2h = twin_maps(hc_to_mc, np.array([0, self.N]), np.array([0, self.Nh]), "n_items")
            self.h2m = torch.from_numpy(h2m).to(self.dev)
            self.m2h = torch.from_numpy(m2h).to(self.dev)
            self.excl_hc = ops.excl_bitmap(self.Nh, self.dev)

    @property
    def remaining(self):
        return self.N - self.n_selected

    def _mc(self, committee, layout, q):
        P, lay = stack_committee(committee, self.dev, layout)
        n = P.shape[1] if lay == "MNC" else P.shape[0]
        if n != self.N:
            raise ValueError(f"committee covers {n} items, the session's pool has {self.N}")
        return ops.select_mc(P, q, lay, excl=self.excl)

    def _mc_frames(self, frames, q):
        """The committee part from frame-level members.  mc: the fused frames
        selection with the bitmap (one launch, no stack).  mix: the consensus
        rows of the remaining songs into the session's buffer, selected as a
        one-member committee ((+0.0 + x) / 1 is x)."""
        ts, sl = frame_member_tensors(frames, self.N, self._F, self._f_perm is None, self.dev)
        if self.mode == "mc":
            return ops.select_frames(ts, self._f_off, q, perm=self._f_perm, song_level=sl, excl=self.excl)
        if ts[0].shape[1] != self._cons.shape[1]:
            raise ValueError(f"members have {ts[0].shape[1]} classes, the hc table {self._cons.shape[1]}")
        ops.frames_consensus(ts, self._f_off, self._f_perm, sl, excl=self.excl, out=self._cons)
        return ops.select_mc(self._cons.unsqueeze(1), q, "NMC", excl=self.excl)

    def _hc(self, q, excl=None):
        return ops.select_mc(self.H.unsqueeze(1), q, "NMC", excl=self.excl if excl is None else excl)

    def _slots(self):
        """Output slots per part: q, but never more than the pools hold (argsort
        [::-1][:q] returns min(q, N)), so a huge q costs no huge buffers."""
        n = self.N + (self.Nh if self.mode == "mix" else 0)
        return min(self.q, n)

    def select(self, committee=None, layout="MNC", frames=None):
        """One epoch: returns the q picked positions (np.int64; fewer when the
        pool runs dry) and removes them from the pool.  ``frames`` (a session
        built with ``s_id``; instead of ``committee``): the members' outputs
        over the FULL X_train as in select_from_frames -- [F, C] frame rows or
        [N, C] song-level, device tensors or arrays; positions index
        ``song_ids``."""
        if frames is not None:
            if committee is not None:
                raise ValueError("pass `committee` or `frames`, not both")
            if self.song_ids is None:
                raise ValueError("`frames` needs a session built with s_id (the frame rows' song ids)")
        q = self.q
        if self.mode == "rand":  # amg_test.py:487-489 over the remaining songs, in X_train order
            keep = ~self._mask()
            pool = self.rand_order[keep[self.rand_order]].tolist()
            (self.rng if self.rng is not None else np.random).shuffle(pool)
            pick = np.asarray(pool[:q], np.int64)
            ops.mark_selected(self.excl, self.N, torch.from_numpy(pick).to(self.dev))
            self.n_selected += len(pick)
            return pick
        qs = self._slots()
        if self.mode == "mc":
            if committee is None and frames is None:
                raise ValueError("mc mode needs `committee` (or `frames`)")
            _, idx = self._mc_frames(frames, qs) if frames is not None else self._mc(committee, layout, qs)
            ops.mark_selected(self.excl, self.N, idx)
        elif self.mode == "hc":
            _, idx = self._hc(qs)
            ops.mark_selected(self.excl, self.N, idx)
        else:  # mix: top-q of each part over the remaining songs, then the union's top-q
            if committee is None and frames is None:
                raise ValueError("mix mode needs `committee` (or `frames`)")
            vm, im = self._mc_frames(frames, qs) if frames is not None else self._mc(committee, layout, qs)
            vh, ih = self._hc(qs, self.excl_hc)
            ih = torch.where(ih >= 0, ih + self.N, ih)
            _, idx = ops.topq_merge(torch.cat([vm, vh]), torch.cat([im, ih]), qs)
            # a song leaves both pools whichever part picked it (:484, :521-531)
            is_hc = idx >= self.N
            row = (idx - self.N).clamp(0, self.Nh - 1)
            item = idx.clamp(0, self.N - 1)
            song = torch.where(idx < 0, idx, torch.where(is_hc, self.h2m[row], idx))
            hrow = torch.where(idx < 0, idx, torch.where(is_hc, row, self.m2h[item]))
            ops.mark_selected(self.excl, self.N, song)
            ops.mark_selected(self.excl_hc, self.Nh, hrow)
        out = idx.cpu().numpy()
        out = out[out >= 0]
        self.n_selected += songs_leaving(out, self.N, self._h2m_host) if self.mode == "mix" else len(out)
        return out

    def frame_geometry(self):
        """(frame_offsets [N + 1], frame_perm [F] or None, None) on the device:
        song n owns the rows frame_perm[frame_offsets[n]:frame_offsets[n+1]] of
        the full X_train (a session built with ``s_id``); the last entry is the
        users' item offsets, None for one user (BatchedSelectionSession has them)."""
        if self.song_ids is None:
            raise ValueError("this session was built without s_id: it holds no frame geometry")
        return self._f_off, self._f_perm, None

    def songs_of(self, picks):
        """The committee song positions behind an epoch's picks (np.int64), i.e.
        the q_songs that X_train.index.isin selects at amg_test.py:491: in mc
        mode the picks themselves; in mix mode an hc pick N + j goes through
        hc_to_mc, -1 twins are dropped and duplicates merged (mix_songs)."""
        if self.mode in ("hc", "rand"):
            raise ValueError(f"mode {self.mode!r} selects from no committee: its picks name no committee songs")
        picks = np.asarray(picks.cpu() if isinstance(picks, torch.Tensor) else picks, dtype=np.int64).reshape(-1)
        if self.mode == "mix":
            return mix_songs(picks, self.N, self._h2m_host)
        return picks[picks >= 0]

    def _mask(self):
        """The exclusion bitmap as a host bool array [N] (True = queried)."""
        words = self.excl.cpu().numpy().view(np.uint32)
        bits = np.unpackbits(words.view(np.uint8), bitorder="little")
        return bits[: self.N].astype(bool)
