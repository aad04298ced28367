"""Committee members that live on the device across epochs.

The reference's epoch is predict -> select -> retrain -> shrink
(amg_test.py:425-531).  ``DeviceGaussianNB`` holds the parameters of U
GaussianNB members (one per user) on the device and closes the loop there:
``predict_proba`` is ops.gnb_predict_proba, ``partial_fit`` is
ops.gnb_partial_fit -- sklearn's ``mod.partial_fit(X_batch, y_batch)`` of :509,
bit for bit -- and ``partial_fit_picks`` goes from a session's picks to the
batch (``X_train[X_train.index.isin(q_songs)]``, :491) without the host
gathering a frame.
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .select import _device


class DeviceGaussianNB:
    """U fitted GaussianNB models (priors=None) on the device.  theta / var
    [U, C, D] (theta_, var_ -- sigma_ in sklearn 0.24), class_count [U, C]
    (class_count_); [C, D], [C, D], [C] mean U = 1.  class_prior defaults to
    class_count / class_count.sum() as sklearn left it after the last fit."""

    def __init__(self, theta, var, class_count, class_prior=None, var_smoothing=1e-9, device=None):
        self.dev = _device(device)

        def own(a):  # a private float64 copy: the updates are in place
            if isinstance(a, torch.Tensor):
                t = a.detach().to(device=self.dev, dtype=torch.float64, copy=True)
            else:
                t = torch.from_numpy(np.array(a, dtype=np.float64)).to(self.dev)
            return t.contiguous()

        theta = own(theta)
        if theta.dim() == 2:
            theta = theta.unsqueeze(0)
        if theta.dim() != 3:
            raise ValueError("theta must be [U, C, D] or [C, D]")
        self.U, self.C, self.D = theta.shape
        self.theta = theta
        self.var = own(var).reshape(theta.shape)
        self.class_count = own(class_count).reshape(self.U, self.C)
        if class_prior is None:
            cc = self.class_count.cpu().numpy()
            class_prior = np.stack([c / c.sum() for c in cc])  # numpy's own 1-D sum, as sklearn's last fit
        self.class_prior = own(class_prior).reshape(self.U, self.C)
        self.epsilon = torch.full((self.U,), float("nan"), dtype=torch.float64, device=self.dev)
        self.var_smoothing = float(var_smoothing)

    def predict_proba(self, X, u=0, out=None):
        """Model u's predict_proba over the frames X [F, D] (ops.gnb_predict_proba, the device prior)."""
        return ops.gnb_predict_proba(X, self.theta[u], self.var[u], self.class_prior[u], out=out)

    def partial_fit(self, X, rows, labels, row_offsets=None):
        """mod.partial_fit(X[rows], labels) for every model, in place: model u
        takes rows[row_offsets[u]:row_offsets[u+1]] (row_offsets=None: one
        model, every row), given in X_train's order.  A model with no row is
        left untouched.  Returns self."""
        ops.gnb_partial_fit(X, rows, labels, self.theta, self.var, self.class_count, row_offsets, self.var_smoothing,
                            class_prior=self.class_prior, epsilon=self.epsilon)
        return self

    def partial_fit_picks(self, X, session, picks, song_labels):
        """The retrain step of an epoch (amg_test.py:491-509) from a session's
        picks: the picks become committee songs (``session.songs_of``), the
        songs the frame rows of X_batch through the session's own frame
        geometry (ops.batch_rows), and the models are updated.  ``session``: a
        SelectionSession built with ``s_id`` (one model) or a
        BatchedSelectionSession built with ``frame_offsets`` (one model per
        user); ``picks``: what its select / step returned; ``song_labels``: the
        class of every song of the (stacked) pool, in [0, C).  An epoch that
        picked nothing (a dry pool, only -1, only hc picks without a twin)
        leaves the models, class_prior and epsilon as they are."""
        f_off, f_perm, items = session.frame_geometry()
        users = 1 if items is None else items.numel() - 1
        if users != self.U:
            raise ValueError(f"the session has {users} user(s), this member {self.U} model(s)")
        songs = session.songs_of(picks)
        if isinstance(songs, list):  # one array per user: pad to [U, width] with -1
            pad = np.full((self.U, max([len(s) for s in songs] + [1])), -1, np.int64)
            for u, s in enumerate(songs):
                pad[u, :len(s)] = s
            songs = pad
        if not isinstance(songs, torch.Tensor):
            songs = torch.from_numpy(np.ascontiguousarray(songs, dtype=np.int64)).to(self.dev)
        rows, labels, row_offsets = ops.batch_rows(songs, f_off, f_perm, song_labels=song_labels, item_offsets=items,
                                                   n_classes=self.C)
        return self.partial_fit(X, rows, labels, row_offsets)

    def state(self):
        """Host copies: dict of theta [U, C, D], var, class_count [U, C], class_prior, epsilon [U]."""
        return {k: getattr(self, k).cpu().numpy().copy()
                for k in ("theta", "var", "class_count", "class_prior", "epsilon")}
