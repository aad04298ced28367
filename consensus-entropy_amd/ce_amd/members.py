"""Committee members that live on the device across epochs.

The reference's epoch is predict -> select -> retrain -> shrink
(amg_test.py:425-531).  ``DeviceGaussianNB`` holds the parameters of U
GaussianNB members (one per user) on the device and closes the loop there:
``predict_proba`` is ops.gnb_predict_proba, ``partial_fit`` is
ops.gnb_partial_fit -- sklearn's ``mod.partial_fit(X_batch, y_batch)`` of :509,
bit for bit -- and ``partial_fit_picks`` goes from a session's picks to the
batch (``X_train[X_train.index.isin(q_songs)]``, :491) without the host
gathering a frame.  ``DeviceSGDClassifier`` is the same for the other member
type :509 retrains, 'classifier_sgd' (ops.sgd_predict_proba,
ops.sgd_partial_fit).
"""
from __future__ import annotations

import numpy as np
import torch

from . import ops
from .select import _device, groupby_device


def _own_f64(a, dev):
    """A private float64 copy on the device: the updates are in place."""
    if isinstance(a, torch.Tensor):
        t = a.detach().to(device=dev, dtype=torch.float64, copy=True)
    else:
        t = torch.from_numpy(np.array(a, dtype=np.float64)).to(dev)
    return t.contiguous()


def _picks_batch(session, picks, song_labels, U, C, dev):
    """From a session's picks to the batch every model retrains on
    (amg_test.py:484-491): the picks become committee songs
    (``session.songs_of``), the songs the frame rows of X_batch through the
    session's own frame geometry (ops.batch_rows).  Returns (rows, labels,
    row_offsets) for the U models of a member with C classes."""
    f_off, f_perm, items = session.frame_geometry()
    users = 1 if items is None else items.numel() - 1
    if users != U:
        raise ValueError(f"the session has {users} user(s), this member {U} model(s)")
    songs = session.songs_of(picks)
    if isinstance(songs, list):  # one array per user: pad to [U, width] with -1
        pad = np.full((U, max([len(s) for s in songs] + [1])), -1, np.int64)
        for u, s in enumerate(songs):
            pad[u, :len(s)] = s
        songs = pad
    if not isinstance(songs, torch.Tensor):
        songs = torch.from_numpy(np.ascontiguousarray(songs, dtype=np.int64)).to(dev)
    max_rows = None
    if isinstance(songs, torch.Tensor) and songs.is_cuda and torch.cuda.is_current_stream_capturing():
        # a capture cannot read the batch's size back: the rows are padded to a host bound instead --
        # every picked slot a song of the longest kind, and never more than the pool's frames
        max_rows = min(session._F, songs.numel() * session._song_frames)
    return ops.batch_rows(songs, f_off, f_perm, song_labels=song_labels, item_offsets=items, n_classes=C,
                          max_rows=max_rows)


def _session_predict(session, X, U, D, C, out, skip_excluded, out_dtypes=(torch.float64,)):
    """What a member's predict_proba_session hands to the users form of its
    predict_proba: the session's frame geometry and bitmap, checked against the
    member (U models, D features, C classes) and X from host numbers alone --
    nothing is read back.  Returns the keyword arguments of ops.*_predict_proba_users."""
    f_off, f_perm, items = session.frame_geometry()
    users = 1 if items is None else items.numel() - 1
    if users != U:
        raise ValueError(f"the session has {users} user(s), this member {U} model(s)")
    if items is None:
        items = session._items  # a SelectionSession: one model owning every song
    if not isinstance(X, torch.Tensor) or X.dim() != 2 or X.shape[1] != D:
        raise ValueError(f"X must be a float64 [F, D={D}] tensor")
    if X.shape[0] < session._rows:
        raise ValueError(f"X has {X.shape[0]} rows, the session's frame geometry names {session._rows}")
    if out is not None:
        ops.check_users_out(out, X.shape[0], C, out_dtypes)
    return dict(item_offsets=items, frame_offsets=f_off, frame_perm=f_perm,
                excl=session.excl if skip_excluded else None, out=out)


def _host_offsets(a, what):
    """Offsets as host numbers (an int64 array): what the shapes are checked from."""
    o = np.asarray(a.cpu() if isinstance(a, torch.Tensor) else a, dtype=np.int64).reshape(-1)
    if o.shape[0] < 1 or o[0] < 0 or (np.diff(o) < 0).any():
        raise ValueError(f"{what} must hold non-decreasing entries >= 0")
    return o


class EvalSet:
    """Every user's test set on the device (amg_test.py:356-366: X_test /
    y_test, the frame rows of the user's test songs), in the sessions' geometry:
    stacked test song g owns the rows ``frame_perm[frame_offsets[g]:
    frame_offsets[g+1]]`` of X (or that range itself), user u the stacked songs
    ``item_offsets[u]:item_offsets[u+1]`` (None: one user owning every song).
    X [F, D] float64, y [F] the encoded class of every ROW of X, 0 .. C-1 (a row
    with any other label is not counted).  ``excl``: an optional exclusion
    bitmap over the stacked songs (ops.excl_bitmap), None by default."""

    def __init__(self, X, y, frame_offsets, item_offsets=None, frame_perm=None, device=None):
        f_off = _host_offsets(frame_offsets, "frame_offsets")
        T = f_off.shape[0] - 1
        items = np.array([0, T], np.int64) if item_offsets is None else _host_offsets(item_offsets, "item_offsets")
        if items.shape[0] < 2:
            raise ValueError("item_offsets must hold U + 1 >= 2 entries")
        if items[-1] > T:
            raise ValueError(f"item_offsets names {int(items[-1])} songs, frame_offsets holds T + 1 = {T + 1} entries")
        self.U, self.T, n = items.shape[0] - 1, T, int(f_off[-1])
        f_perm = None
        if frame_perm is not None:
            f_perm = np.asarray(frame_perm.cpu() if isinstance(frame_perm, torch.Tensor) else frame_perm,
                                dtype=np.int64).reshape(-1)
            if f_perm.shape[0] < n or (f_perm < 0).any():
                raise ValueError(f"frame_perm must hold frame_offsets[-1] = {n} row indices >= 0")
        self._rows = int(f_perm[:n].max()) + 1 if f_perm is not None and n else n  # rows of X the geometry names
        if not isinstance(X, torch.Tensor):
            X = torch.from_numpy(np.ascontiguousarray(getattr(X, "values", X), dtype=np.float64))
        if X.dim() != 2 or X.dtype != torch.float64:
            raise ValueError("X must be a float64 [F, D] tensor")
        if X.shape[0] < self._rows:
            raise ValueError(f"X has {X.shape[0]} rows, the frame geometry names {self._rows}")
        if not isinstance(y, torch.Tensor):
            y = torch.from_numpy(np.ascontiguousarray(getattr(y, "values", y)))
        if y.dim() != 1 or y.shape[0] != X.shape[0] or y.dtype.is_floating_point or y.dtype == torch.bool:
            raise ValueError(f"y must hold one integer class per row of X ({X.shape[0]})")
        self.dev = _device(device if device is not None or not X.is_cuda else X.device)
        self.X = X.to(self.dev)
        if self.X.stride(1) != 1:
            self.X = self.X.contiguous()
        self.y = y.to(device=self.dev, dtype=torch.int32).contiguous()
        self.F, self.D = self.X.shape
        self.frame_offsets = torch.from_numpy(f_off).to(self.dev)
        self.item_offsets = torch.from_numpy(items).to(self.dev)
        self.frame_perm = torch.from_numpy(f_perm).to(self.dev) if f_perm is not None else None
        self.excl = None

    @classmethod
    def from_s_id(cls, X, y, s_id, item_offsets=None, device=None):
        """The test set of pandas frames: ``s_id`` names the song of every row
        of X.  The songs are the sorted unique ids and a song's rows keep their
        order -- groupby(['s_id']), the same rule as the sessions (groupby_device);
        item_offsets counts those sorted songs per user."""
        dev = _device(device if device is not None or not (isinstance(X, torch.Tensor) and X.is_cuda) else X.device)
        _, _, _, f_off, f_perm = groupby_device(s_id, dev)
        return cls(X, y, f_off, item_offsets, f_perm, device=dev)

    def frame_geometry(self):
        """(frame_offsets [T + 1], frame_perm or None, item_offsets [U + 1]) on the device, as a session's."""
        return self.frame_offsets, self.frame_perm, self.item_offsets


def _evalset_args(evalset, U, D):
    """What a member's ``evaluate`` hands to ops.*_score_users: the set's
    geometry, checked against the member from host numbers alone."""
    if not isinstance(evalset, EvalSet):
        raise TypeError("evaluate needs a ce_amd.EvalSet")
    f_off, f_perm, items = evalset.frame_geometry()
    if evalset.U != U:
        raise ValueError(f"the EvalSet has {evalset.U} user(s), this member {U} model(s)")
    if evalset.D != D:
        raise ValueError(f"the EvalSet has {evalset.D} features, this member {D}")
    return dict(item_offsets=items, frame_offsets=f_off, frame_perm=f_perm, excl=evalset.excl, y=evalset.y)


def mean_f1(f1_list):
    """np.mean(f1_list) of amg_test.py:518 for every user, on the device: the
    members' f1 [U] tensors added one after the other in list order onto 0.0
    and divided by their count -- numpy's bits for fewer than 8 members (its
    pairwise sum adds in order below 8 terms)."""
    f1_list = list(f1_list)
    if not f1_list:
        raise ValueError("mean_f1 needs at least one member's f1")
    if len(f1_list) >= 8:
        raise ValueError("mean_f1 restates np.mean for fewer than 8 members")
    s = torch.zeros_like(f1_list[0])
    for f in f1_list:
        s = s + f
    return s / float(len(f1_list))


def _f1_of(cm, report):
    if report:
        f1, prf = ops.f1_weighted_users(cm, report=True)
        return f1, cm, prf
    return ops.f1_weighted_users(cm), cm


class DeviceGaussianNB:
    """U fitted GaussianNB models (priors=None) on the device.  theta / var
    [U, C, D] (theta_, var_ -- sigma_ in sklearn 0.24), class_count [U, C]
    (class_count_); [C, D], [C, D], [C] mean U = 1.  class_prior defaults to
    class_count / class_count.sum() as sklearn left it after the last fit."""

    def __init__(self, theta, var, class_count, class_prior=None, var_smoothing=1e-9, device=None):
        self.dev = _device(device)

        def own(a):
            return _own_f64(a, self.dev)

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

    def predict_proba_session(self, X, session, out=None, skip_excluded=True):
        """The predict step of an epoch (amg_test.py:435) for every model in
        one launch (ops.gnb_predict_proba_users): every frame row of X [F, D]
        owned by a song of the session is predicted by the model of the user
        who owns it -- bit for bit ``predict_proba(X, u)`` on that row.
        ``session``: a SelectionSession built with ``s_id`` (one model owning
        every song) or a BatchedSelectionSession built with ``frame_offsets``
        (one model per user).  skip_excluded: the rows of the songs already
        picked are not written (and mostly not read) -- the session's
        ``frames=`` epochs read no row of an excluded song; False writes every
        owned row.  ``out``: an optional float64 [F, C] view (unit column
        stride); rows it does not write keep what they held, and a new tensor
        is zero there.  Nothing is synchronised or read back."""
        kw = _session_predict(session, X, self.U, self.D, self.C, out, skip_excluded)
        return ops.gnb_predict_proba_users(X, self.theta, self.var, self.class_prior, **kw)

    def evaluate(self, evalset, report=False):
        """The evaluate step of an epoch (amg_test.py:513-515, and :411-413
        before epoch 0) for every model: one score launch (ops.gnb_score_users:
        ``mod.predict`` of every user's test frames, counted against their
        labels) and one F1 launch (ops.f1_weighted_users: sklearn's
        ``f1_score(average='weighted')``).  ``evalset``: a ce_amd.EvalSet.
        Returns (f1 [U], cm [U, C, C]), or (f1, cm, prf [U, C, 4]) with
        report=True -- the per-class precision, recall, F1 and support of
        classification_report (:514).  Nothing is synchronised or read back."""
        kw = _evalset_args(evalset, self.U, self.D)
        cm, _, _ = ops.gnb_score_users(evalset.X, self.theta, self.var, self.class_prior, **kw)
        return _f1_of(cm, report)

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
        rows, labels, row_offsets = _picks_batch(session, picks, song_labels, self.U, self.C, self.dev)
        return self.partial_fit(X, rows, labels, row_offsets)

    def state(self):
        """Host copies: dict of theta [U, C, D], var, class_count [U, C], class_prior, epsilon [U]."""
        return {k: getattr(self, k).cpu().numpy().copy()
                for k in ("theta", "var", "class_count", "class_prior", "epsilon")}


SGD_OVERFLOW = ("Floating-point under-/overflow occurred at epoch #1. Scaling input data with StandardScaler or "
                "MinMaxScaler might help.")  # sklearn's text (_plain_sgd)


class DeviceSGDClassifier:
    """U SGDClassifier(loss='log', penalty='l2', learning_rate='optimal')
    models on the device: the reference's 'classifier_sgd' member
    (deam_classifier.py:214-217).  coef [U, K, D] (coef_), intercept [U, K]
    (intercept_), t [U] (t_: 1.0 for a model that has seen no row); [K, D],
    [K] and a number mean U = 1.  K = C one-vs-rest problems, or 1 for C = 2.
    ``random_state``: the integer the model was built with (one for all, or one
    per model) -- the shuffle seeds follow from it (ops.sgd_chain_seeds) and are
    the same for every partial_fit.  ``grad``: "half_binomial" (sklearn >= 1.x,
    bit-identical to 1.7.2) or "log_dloss" (sklearn 0.24.1's gradient; unpinned)."""

    def __init__(self, coef, intercept, t, alpha=1e-4, random_state=None, grad="half_binomial", device=None):
        self.dev = _device(device)
        coef = _own_f64(coef, self.dev)
        if coef.dim() == 1:
            coef = coef.unsqueeze(0)
        if coef.dim() == 2:
            coef = coef.unsqueeze(0)
        if coef.dim() != 3:
            raise ValueError("coef must be [U, K, D] or [K, D]")
        self.U, self.K, self.D = coef.shape
        if not 1 <= self.K <= 8 or self.K == 2:
            raise ValueError(f"coef holds K = {self.K} binary problems: K = 1 (two classes) or 3 .. 8 (one per class)")
        self.C = 2 if self.K == 1 else self.K
        self.coef = coef
        self.intercept = _own_f64(intercept, self.dev).reshape(self.U, self.K)
        self.t = _own_f64(np.broadcast_to(np.asarray(t.cpu() if isinstance(t, torch.Tensor) else t, np.float64).reshape(-1),
                                          (self.U,)), self.dev)
        if random_state is None:
            raise ValueError("DeviceSGDClassifier needs the integer random_state of the model (None cannot be reproduced)")
        states = np.asarray(random_state).reshape(-1)
        if states.size not in (1, self.U):
            raise ValueError(f"random_state must be one integer or one per model ({self.U})")
        seeds = np.stack([ops.sgd_chain_seeds(int(r), self.C) for r in np.broadcast_to(states, (self.U,))])
        self.seeds = torch.from_numpy(seeds.view(np.int32)).to(self.dev)  # [U, K]: on the device once, so a fit is capturable
        self.status = torch.zeros(self.U, dtype=torch.int32, device=self.dev)
        self.alpha = float(alpha)
        ops.sgd_optimal_init(self.alpha)  # refuses a bad alpha here
        if grad not in ops.SGD_GRADS:
            raise ValueError(f"grad must be one of {sorted(ops.SGD_GRADS)}, got {grad!r}")
        self.grad = grad

    def predict_proba(self, X, u=0, out=None):
        """Model u's predict_proba over the frames X [F, D] (ops.sgd_predict_proba)."""
        return ops.sgd_predict_proba(X, self.coef[u], self.intercept[u], out=out)

    def predict_proba_session(self, X, session, out=None, skip_excluded=True):
        """The predict step of an epoch for every model in one launch
        (ops.sgd_predict_proba_users), as DeviceGaussianNB.predict_proba_session:
        bit for bit ``predict_proba(X, u)`` on every row user u owns."""
        kw = _session_predict(session, X, self.U, self.D, self.C, out, skip_excluded)
        return ops.sgd_predict_proba_users(X, self.coef, self.intercept, **kw)

    def evaluate(self, evalset, report=False):
        """The evaluate step of an epoch for every model, as
        DeviceGaussianNB.evaluate (ops.sgd_score_users, ops.f1_weighted_users):
        returns (f1 [U], cm [U, C, C]), and prf [U, C, 4] with report=True."""
        kw = _evalset_args(evalset, self.U, self.D)
        cm, _, _ = ops.sgd_score_users(evalset.X, self.coef, self.intercept, **kw)
        return _f1_of(cm, report)

    def partial_fit(self, X, rows, labels, row_offsets=None):
        """mod.partial_fit(X[rows], labels) for every model, in place: model u
        takes rows[row_offsets[u]:row_offsets[u+1]] (row_offsets=None: one
        model, every row), given in X_train's order.  A model with no row is
        left untouched.  Nothing is read back: ``check_finite`` reports where
        sklearn would have raised.  Returns self."""
        ops.sgd_partial_fit(X, rows, labels, self.coef, self.intercept, self.t, row_offsets, self.alpha,
                            seeds=self.seeds, grad=self.grad, status=self.status)
        return self

    def partial_fit_picks(self, X, session, picks, song_labels):
        """The retrain step of an epoch (amg_test.py:491-509) from a session's
        picks, as DeviceGaussianNB.partial_fit_picks: a SelectionSession built
        with ``s_id`` (one model) or a BatchedSelectionSession built with
        ``frame_offsets`` (one model per user).  An epoch that picked nothing
        leaves the models as they are."""
        rows, labels, row_offsets = _picks_batch(session, picks, song_labels, self.U, self.C, self.dev)
        return self.partial_fit(X, rows, labels, row_offsets)

    def check_finite(self):
        """Reads the models' flags (one device-to-host copy).  Raises sklearn's
        ValueError where a partial_fit left an intercept or a weight non-finite,
        a RuntimeError where a model was not run; the flags stay set."""
        st = self.status.cpu().numpy()
        if (st == 2).any():
            raise RuntimeError(f"model(s) {np.flatnonzero(st == 2).tolist()} were not updated: "
                               "a batch of 2^31 rows or more, or no workspace for its permutations")
        if (st != 0).any():
            raise ValueError(f"{SGD_OVERFLOW} (model(s) {np.flatnonzero(st != 0).tolist()})")
        return self

    def state(self):
        """Host copies: dict of coef [U, K, D], intercept [U, K], t [U], status [U]."""
        return {k: getattr(self, k).cpu().numpy().copy() for k in ("coef", "intercept", "t", "status")}


class DeviceXGBClassifier:
    """U XGBClassifier members on the device: the reference's 'classifier_xgb'
    (deam_classifier.py:226-232), one forest per user.  ``base``: the shared
    pretrained model (xgboost JSON or an XgbForest); ``models``: every user's
    full model (None entries, or ``models=None`` with ``U``, mean the base
    itself).  The refit runs on the device: ``fit`` / ``fit_picks`` grow the
    rounds of ``mod.fit(X_batch, y, xgb_model=mod.get_booster())``
    (amg_test.py:507) for every user in one launch and append them to the
    stacked forests the predict and evaluate walks read; nothing of a tree
    comes back to the host unless ``forest(u)``, ``models[u]`` or ``state()``
    asks.  ``status`` (int32 [U], as on DeviceSGDClassifier) flags the users a
    fit left alone.  A model trained elsewhere is still handed over with
    ``set_model(u, ...)``, which compares and packs that one model on the host
    and replaces that user's whole tail, device-grown trees included.  After a
    ``fit`` or a ``set_model`` the device arrays are updated outside a capture:
    neither call, nor the first predict or evaluate after a ``set_model``, is
    graph-capturable.  ``device``: where the tables live; X and the EvalSet
    must be on it.  Depth <= 5."""

    def __init__(self, base, models=None, U=None, device=None):
        from .xgb import StackedForests, XgbForest

        self.dev = _device(device)
        self.base = base if isinstance(base, XgbForest) else XgbForest.from_json(base)
        if models is None:
            models = [None] * (1 if U is None else int(U))
        elif U is not None and int(U) != len(models):
            raise ValueError(f"U={U} but {len(models)} model(s) given")
        if len(models) < 1:
            raise ValueError("DeviceXGBClassifier needs at least one model")
        self._models = [self._forest(m) for m in models]
        self.U, self.C, self.G = len(self._models), self.base.n_classes, self.base.n_groups
        self.D = self.base.num_feature
        self._stacked = StackedForests(self.base, self._models)  # refuses models that disagree with the base
        self._status = None  # on the device from the first use on: the member is built without one

    @property
    def status(self):
        """int32 [U] on the device, only ever set by ``fit``: 1 where a batch held a non-finite value, 2 where
        it was not run."""
        if self._status is None:
            self._status = torch.zeros(self.U, dtype=torch.int32, device=self.dev)
        return self._status

    @property
    def models(self):
        """Every user's full model (None: the base itself) as a NEW list, read-only:
        assigning into it changes nothing (``set_model`` is the way to hand a
        model over), and after a ``fit`` it reads every grown tree of every user
        back from the device.  ``forest(u)`` reads one user's."""
        return [None if self._models[u] is None and not self._stacked.has_grown(u) else self.forest(u)
                for u in range(self.U)]

    def _forest(self, m):
        from .xgb import XgbForest

        return None if m is None else (m if isinstance(m, XgbForest) else XgbForest.from_json(m))

    def stacked(self):
        """The users' forests as one ``ce_amd.xgb.StackedForests``."""
        return self._stacked

    def set_model(self, u, model):
        """User u's forest after a host refit (JSON, an XgbForest, or None for
        the base): checked against the base, compared with it and packed here;
        no other user's trees are touched.  Returns self."""
        if not 0 <= int(u) < self.U:
            raise ValueError(f"user {u} outside [0, {self.U})")
        forest = self._forest(model)
        self._stacked.set(int(u), forest)  # raises before anything changes
        self._models[int(u)] = forest
        return self

    def fit(self, X, rows, labels, row_offsets=None, n_rounds=100, max_depth=5, **params):
        """mod.fit(X[rows], labels, xgb_model=mod.get_booster()) for every
        forest (amg_test.py:507), on the device: forest u grows ``n_rounds``
        rounds of depth <= ``max_depth`` on rows[row_offsets[u]:row_offsets[u+1]]
        (row_offsets=None: one forest, every row), given in X_train's order,
        and the walks see them from the next call on (ops.xgb_fit_users, which
        names the parameters it takes and those it refuses).  A forest with no
        row is left untouched; one whose batch holds a non-finite value too,
        with ``status[u]`` = 1.  If ``max_depth`` is above the stack's common
        depth the stack is packed again at the new depth first.  Not
        graph-capturable.  Returns self."""
        if isinstance(X, torch.Tensor) and X.dim() == 2:
            self._check_D(X.shape[1])
            self._check_dev(X, "X")
        ops.xgb_fit_users(X, rows, labels, self._stacked, row_offsets, n_rounds, max_depth, status=self.status, **params)
        return self

    def fit_picks(self, X, session, picks, song_labels, n_rounds=100, max_depth=5, **params):
        """The retrain step of an epoch (amg_test.py:491-507) from a session's
        picks, as DeviceGaussianNB.partial_fit_picks: the picks become songs,
        the songs the frame rows of X_batch (ops.batch_rows), and every forest
        grows its rounds on its own batch.  An epoch that picked nothing leaves
        the forests as they are."""
        rows, labels, row_offsets = _picks_batch(session, picks, song_labels, self.U, self.C, self.dev)
        return self.fit(X, rows, labels, row_offsets, n_rounds, max_depth, **params)

    def check_finite(self):
        """Reads the flags (one device-to-host copy).  Raises a ValueError where
        a fit met a non-finite value in a batch, a RuntimeError where a batch
        was not run; the flags stay set."""
        st = self.status.cpu().numpy()
        if (st == 2).any():
            raise RuntimeError(f"forest(s) {np.flatnonzero(st == 2).tolist()} were not fitted: too many rows")
        if (st != 0).any():
            raise ValueError(f"the batch of forest(s) {np.flatnonzero(st != 0).tolist()} holds a non-finite value, "
                             "a row outside X or a label outside [0, C): they were left unchanged")
        return self

    def _check_dev(self, t, what):
        d = t.device
        if d.type != self.dev.type or (self.dev.index is not None and d.index != self.dev.index):
            raise ValueError(f"{what} is on {d}, this member's tables on {self.dev}")

    def forest(self, u=0):
        """User u's full forest (an XgbForest); device-grown trees are read back."""
        if not self._stacked.has_grown(u):
            return self.base if self._models[u] is None else self._models[u]
        return self._stacked.forest(u)

    def predict_proba(self, X, u=0, out=None, out_dtype=torch.float32):
        """Model u's predict_proba over the frames X [F, D] (ops.xgb_predict_proba, the one-forest path)."""
        return ops.xgb_predict_proba(X, self.forest(u), out=out, out_dtype=out_dtype)

    def _check_D(self, D):
        if self.D and D != self.D:
            raise ValueError(f"X has {D} features, this member {self.D}")

    def predict_proba_session(self, X, session, out=None, skip_excluded=True, out_dtype=torch.float32):
        """The predict step of an epoch (amg_test.py:435) for every forest in
        one launch (ops.xgb_predict_proba_users), as
        DeviceGaussianNB.predict_proba_session: bit for bit
        ``predict_proba(X, u)`` on every row user u owns.  X float32 or float64;
        the result float32 (xgboost's own; a float32 frame-level member of
        ``select(frames=[...])``) or float64 (its exact upcast)."""
        if isinstance(X, torch.Tensor) and X.dim() == 2:
            self._check_D(X.shape[1])
            self._check_dev(X, "X")
        kw = _session_predict(session, X, self.U, X.shape[1] if isinstance(X, torch.Tensor) and X.dim() == 2 else self.D,
                              self.C, out, skip_excluded, (torch.float32, torch.float64))
        return ops.xgb_predict_proba_users(X, self.stacked(), out_dtype=out_dtype, **kw)

    def evaluate(self, evalset, report=False):
        """The evaluate step of an epoch for every forest, as
        DeviceGaussianNB.evaluate (ops.xgb_score_users, ops.f1_weighted_users):
        returns (f1 [U], cm [U, C, C]), and prf [U, C, 4] with report=True."""
        if isinstance(evalset, EvalSet):
            self._check_D(evalset.D)
            self._check_dev(evalset.X, "the EvalSet")
        kw = _evalset_args(evalset, self.U, evalset.D if isinstance(evalset, EvalSet) else self.D)
        cm, _, _ = ops.xgb_score_users(evalset.X, self.stacked(), **kw)
        return _f1_of(cm, report)

    def state(self):
        """Host copies of the stacked arrays: dict of nodes, leaves, tree_ids, group_offsets, depth."""
        s = self.stacked()
        return {"nodes": s.nodes.copy(), "leaves": s.leaves.copy(), "tree_ids": s.tree_ids.copy(),
                "group_offsets": s.group_offsets.copy(), "depth": s.depth}
