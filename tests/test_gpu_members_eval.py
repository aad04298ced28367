"""The evaluate step of the linear members on the GPU (ce_gnb_score_users,
ce_sgd_score_users, ce_f1_weighted_users; ops.*_score_users,
ops.f1_weighted_users, EvalSet, Device*.evaluate, mean_f1).

Scores: the returned jll / decision values give, through the restated
logsumexp / expit (the C library's exp and log, numpy's order), the bits of
ops.*_predict_proba_users on the same geometry -- kernels that are pinned
already; the GaussianNB scores are also gnb_jll's bits.  Labels: sklearn's rule
over the returned scores on every counted row, the prefill (-1, NaN) on every
other.  Counts: np.add.at over the counted rows, exactly.  F1: f1_weighted
(tests/members_eval_ref.py, pinned to sklearn by tests/test_members_eval.py) in
all 64 bits."""
import numpy as np
import pytest
import torch

from conftest import golden
from gnb_fit_ref import gnb_partial_fit, same_bits
from members_eval_ref import (confusion, f1_weighted, gnb_jll, libm_exp, libm_log, predict_labels, prf,
                              sgd_decision)
from members_proba_ref import sgd_proba_from_decision
from members_users_ref import excl_words, row_owners
from sgd_fit_ref import sgd_partial_fit

pytestmark = pytest.mark.gpu

FILL_BITS = 0x7FF8C0DE00000A5A  # a NaN with a payload of its own (the prefill of predict_proba_users' out)


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def last_kernel(ce):
    return ce._lib.load().ce_last_kernel().decode()


class Pool:
    """U users' stacked songs and their frame rows (the Pool of
    tests/test_gpu_members_users.py).  ``frames``: per user, the frame count of
    each of their songs.  shuffled: the rows in random order (a frame_perm, a
    song's rows ascending); extra: rows of X that no song owns."""

    def __init__(self, rng, frames, shuffled=False, extra=0):
        self.U = len(frames)
        self.off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
        counts = np.concatenate([np.asarray(f, np.int64) for f in frames] + [np.zeros(0, np.int64)])
        self.T = len(counts)
        self.f_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n = int(self.f_off[-1])
        self.F = n + extra
        self.f_perm = None
        if shuffled:
            rows = rng.permutation(self.F)[:n]
            self.f_perm = np.concatenate([np.sort(rows[self.f_off[g]:self.f_off[g + 1]]) for g in range(self.T)]
                                         + [np.zeros(0, np.int64)]).astype(np.int64)
        self.user, self.song = row_owners(self.off, self.f_off, self.f_perm, self.F)

    def geometry(self, f_perm="own"):
        f_perm = self.f_perm if isinstance(f_perm, str) else f_perm
        return dict(item_offsets=dev(self.off), frame_offsets=dev(self.f_off),
                    frame_perm=None if f_perm is None else dev(f_perm))


def gnb_models(rng, U, C, D):
    theta, var = rng.normal(0, 1, (U, C, D)), rng.random((U, C, D)) + 0.1
    return theta, var, rng.dirichlet(np.ones(C) * 3, U)


def sgd_models(rng, U, C, D):
    K = 1 if C == 2 else C
    return rng.normal(0, 0.5, (U, K, D)) / np.sqrt(D / 8), rng.normal(0, 0.5, (U, K))


def labels_for(rng, F, C):
    """One class per row, with some -1 and C among them (rows that are not counted)."""
    y = rng.integers(0, C, F).astype(np.int32)
    y[rng.random(F) < 0.06] = -1
    y[rng.random(F) < 0.06] = C
    return y


def proba_from_scores(kind, s, C):
    """sklearn's predict_proba tail over the kernels' scores: GaussianNB scipy's
    logsumexp (the running max, a non-finite max -> 0, the exps added one after
    the other onto -0.0: numpy's order over the F-ordered jll), SGD expit and
    sklearn's own ``p / p.sum(axis=1)`` over a C-contiguous array (numpy's
    order: 8 classes take the 8-accumulator tree; members_proba_ref), or
    [1 - p, p] for a binary model."""
    with np.errstate(all="ignore"):
        if kind == "gnb":
            mx = s[:, 0].copy()
            for c in range(1, C):
                mx = np.where(s[:, c] > mx, s[:, c], mx)
            mx[~np.isfinite(mx)] = 0.0
            acc = np.full(len(s), -0.0)
            for c in range(C):
                acc = acc + libm_exp(s[:, c] - mx)
            lse = libm_log(0.0 + acc) + mx
            return libm_exp(s - lse[:, None])
        return sgd_proba_from_decision(s)


def score(ce, kind, Xd, models, geom, yd, excl=None):
    f = ce.ops.gnb_score_users if kind == "gnb" else ce.ops.sgd_score_users
    cm, pred, scores = f(Xd, *[dev(m) for m in models], **geom, y=yd, excl=None if excl is None else dev(excl),
                         return_pred=True, return_scores=True)
    return cm.cpu().numpy(), pred.cpu().numpy(), scores.cpu().numpy()


def check(ce, kind, rng, pool, C, D, excluded=None, f_perm="own", ld=None, X=None, models=None, user=None, y=None,
          jll_bits=False, kernel=None):
    """One score launch over `pool` (run twice) and the F1 launch over its
    counts, against the criteria of the module docstring.  Returns (cm, pred, scores, counted)."""
    X = rng.normal(0, 1, (pool.F, D)) if X is None else X
    if ld:
        Xbuf = torch.zeros((pool.F, ld), dtype=torch.float64, device="cuda")
        Xbuf[:, :D] = dev(X)
        Xd = Xbuf[:, :D]
    else:
        Xd = dev(X)
    if models is None:
        models = gnb_models(rng, pool.U, C, D) if kind == "gnb" else sgd_models(rng, pool.U, C, D)
    K = models[0].shape[1]
    y = labels_for(rng, pool.F, C) if y is None else y
    user = pool.user if user is None else user
    owned = np.where(np.isin(pool.song, list(excluded or [])), -1, user)
    counted = (owned >= 0) & (y >= 0) & (y < C)
    geom = pool.geometry(f_perm)
    excl = None if excluded is None else excl_words(excluded, pool.T)
    yd = dev(y)
    cm, pred, scores = score(ce, kind, Xd, models, geom, yd, excl)
    if kernel is not None:
        assert last_kernel(ce) == kernel
    cm2, pred2, scores2 = score(ce, kind, Xd, models, geom, yd, excl)
    assert np.array_equal(cm, cm2) and np.array_equal(pred, pred2) and same_bits(scores, scores2)
    # scores: the pinned predict_proba kernels' bits through their own tail
    out = torch.full((pool.F, C), FILL_BITS, dtype=torch.int64, device="cuda").view(torch.float64)
    fp = ce.ops.gnb_predict_proba_users if kind == "gnb" else ce.ops.sgd_predict_proba_users
    proba = fp(Xd, *[dev(m) for m in models], **geom, excl=None if excl is None else dev(excl), out=out).cpu().numpy()
    assert scores.shape == (pool.F, C if kind == "gnb" else K)
    assert same_bits(proba_from_scores(kind, scores[counted], C), proba[counted])
    assert np.isnan(scores[~counted]).all() and (pred[~counted] == -1).all(), "a row that is not counted was written"
    if jll_bits:
        for u in np.unique(owned[counted]):
            r = counted & (owned == u)
            if kind == "gnb":
                want = gnb_jll(X[r], models[0][u], models[1][u], models[2][u])
            else:
                want = sgd_decision(X[r], models[0][u], models[1][u])
            assert same_bits(scores[r], want), u
    # labels: sklearn's rule over the returned scores; counts: np.add.at, exactly
    assert np.array_equal(pred[counted], predict_labels(scores[counted], binary=K == 1))
    want_cm = confusion(y, pred, C, np.where(counted, owned, -1), pool.U)
    assert cm.dtype == np.int64 and np.array_equal(cm, want_cm)
    assert cm.sum() == counted.sum()
    # F1: the restatement, in all 64 bits
    f1, rep = ce.ops.f1_weighted_users(dev(cm), report=True)
    assert same_bits(f1.cpu().numpy(), np.array([f1_weighted(m) for m in cm]))
    assert np.array_equal(bits(rep.cpu().numpy()), bits(np.stack([prf(m) for m in cm])))
    assert same_bits(ce.ops.f1_weighted_users(dev(cm)).cpu().numpy(), f1.cpu().numpy())
    return cm, pred, scores, counted


def split(rng, n, parts):
    cuts = np.sort(rng.integers(0, n + 1, parts - 1))
    return np.diff(np.concatenate([[0], cuts, [n]]))


STREAMED = "ce::k_gnb_score_users260<4, 3>"


# ---- 1. user edges ------------------------------------------------------------------
@pytest.mark.parametrize("D", [16, 260])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_user_boundaries_inside_groups_and_blocks(ce, kind, shuffled, D):
    """Users of 0, 1, 7, 8, 9, 33 and 257 frames in one pool, a user without a
    song, songs without a frame; D = 260, C = 4 takes the streamed kernel."""
    rng = np.random.default_rng(10 + shuffled)
    counts = [0, 1, 7, 8, 9, 33, 257]
    frames = [split(rng, n, 3) for n in counts]
    frames.insert(4, [])
    frames[1] = np.array([0, counts[1], 0])
    pool = Pool(rng, frames, shuffled)
    assert [int((pool.user == u).sum()) for u in range(pool.U)] == counts[:4] + [0] + counts[4:]
    kernel = (STREAMED if D == 260 else "ce::k_gnb_score_users<8, 0>") if kind == "gnb" else \
        f"ce::k_sgd_score_users<{36 if D == 260 else 8}>"
    cm, _, _, _ = check(ce, kind, rng, pool, 4, D, kernel=kernel, jll_bits=kind == "gnb")
    assert cm[0].sum() == 0 and cm[4].sum() == 0  # the users without a frame: an empty matrix, F1 NaN
    f1 = ce.ops.f1_weighted_users(dev(cm)).cpu().numpy()
    assert np.isnan(f1[[0, 4]]).all() and np.isfinite(f1[[3, 5, 6, 7]]).all()


@pytest.mark.parametrize("D", [24, 260])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_three_hundred_users_of_three_frames(ce, kind, D):
    """A block's share crosses many users: a restage and a flush every three frames."""
    rng = np.random.default_rng(12)
    pool = Pool(rng, [[1, 2]] * 150 + [[3]] * 150, shuffled=True)
    check(ce, kind, rng, pool, 4, D)


@pytest.mark.parametrize("D", [16, 260])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_one_user_over_several_blocks(ce, kind, D):
    """5000 frames of one user (a share is at least 128 positions: some 40
    blocks add into one cm[u]) between two small users."""
    rng = np.random.default_rng(13)
    pool = Pool(rng, [[5, 4], split(rng, 5000, 7), [11]], shuffled=D == 16)
    cm, _, _, counted = check(ce, kind, rng, pool, 4, D)
    assert cm[1].sum() == (counted & (pool.user == 1)).sum() > 4000


@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_scores_against_the_one_model_entry_points(ce, kind):
    """The score and the proba kernel of the 260 form and of SGD are one body, so
    `check` compares only their finishes there.  Here the scores go through the
    proba tail and must equal, in all 64 bits, the ONE-model entry point
    (k_gnb_stream260 / k_sgd_span260: a text of their own) run per user.  Users
    of 5, 0 and 70 positions: a boundary inside an 8-frame group, a user without
    a frame, more than two 32-position passes; C = 4, D = ld = 260."""
    rng = np.random.default_rng(14)
    pool = Pool(rng, [[5], [], [30, 40]])
    C, D = 4, 260
    Xd = dev(rng.normal(0, 1, (pool.F, D)))
    models = gnb_models(rng, pool.U, C, D) if kind == "gnb" else sgd_models(rng, pool.U, C, D)
    y = rng.integers(0, C, pool.F).astype(np.int64)
    _, _, scores = score(ce, kind, Xd, models, pool.geometry(), dev(y))
    assert last_kernel(ce) == (STREAMED if kind == "gnb" else "ce::k_sgd_score_users<36>")
    assert [int((pool.user == u).sum()) for u in range(pool.U)] == [5, 0, 70]
    for u in (0, 2):
        rows = pool.user == u
        m = [dev(a[u]) for a in models]
        one = (ce.ops.gnb_predict_proba if kind == "gnb" else ce.ops.sgd_predict_proba)(Xd, *m).cpu().numpy()
        assert same_bits(proba_from_scores(kind, scores[rows], C), one[rows]), u


# ---- 2. feature and class edges ---------------------------------------------------------
@pytest.mark.parametrize("C", [2, 3, 4, 8])
@pytest.mark.parametrize("D", [8, 9, 64, 260, 512])
def test_gnb_feature_and_class_edges(ce, D, C):
    rng = np.random.default_rng(D * 10 + C)
    pool = Pool(rng, [[3, 30], [17], [9, 0, 41]], shuffled=bool(D & 1))
    check(ce, "gnb", rng, pool, C, D, jll_bits=True, kernel=STREAMED if (D, C) == (260, 4) else None)
    check(ce, "gnb", rng, pool, C, D, ld=D + 3)  # a row pitch above D (D = 260: the general kernel)
    if D == 260:
        assert last_kernel(ce) == "ce::k_gnb_score_users<36, 260>"


@pytest.mark.parametrize("C", [2, 3, 4, 8])
@pytest.mark.parametrize("D", [1, 7, 8, 9, 64, 260, 512])
def test_sgd_feature_and_class_edges(ce, D, C):
    rng = np.random.default_rng(D * 10 + C)
    pool = Pool(rng, [[3, 30], [17], [9, 0, 41]], shuffled=bool(D & 1))
    check(ce, "sgd", rng, pool, C, D, jll_bits=D <= 64)  # C = 2: the binary model, K = 1
    check(ce, "sgd", rng, pool, C, D, ld=D + 3)


# ---- 3. row order and exclusion ---------------------------------------------------------
@pytest.mark.parametrize("D", [33, 260])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_rows_no_song_owns_and_rows_out_of_range(ce, kind, D):
    rng = np.random.default_rng(20)
    frames = [[5, 12, 3], [40], [0, 9]]
    for shuffled in (False, True):
        pool = Pool(rng, frames, shuffled, extra=11)
        assert (pool.user < 0).sum() == 11
        check(ce, kind, rng, pool, 4, D)
    pool = Pool(rng, frames, shuffled=True)
    bad = pool.f_perm.copy()
    lost = [0, 6, 7, 30, len(bad) - 1]
    bad[lost] = [pool.F, pool.F + 1, 1 << 40, -1, -(1 << 35)]
    user, _ = row_owners(pool.off, pool.f_off, bad, pool.F)
    assert (user < 0).sum() == len(lost)
    check(ce, kind, rng, pool, 4, D, f_perm=bad, user=user)


@pytest.mark.parametrize("D", [40, 260])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_excluded_songs_are_not_counted(ce, kind, shuffled, D):
    """Some songs excluded, a whole user excluded, runs of more than 8 excluded
    frames (whole 8-frame groups skipped), excluded songs that straddle a group."""
    rng = np.random.default_rng(30 + shuffled)
    frames = [[3, 5, 20, 4, 1], [6, 6], [2, 40, 9, 0, 7], [13], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]]
    pool = Pool(rng, frames, shuffled, extra=3)
    off = pool.off
    excluded = [int(g) for g in (off[0] + 2, off[1], off[1] + 1, off[2] + 1, off[2] + 3, off[4] + 2, off[4] + 3,
                                 off[4] + 5, off[4] + 11)]
    cm, _, _, _ = check(ce, kind, rng, pool, 4, D, excluded=excluded)
    assert cm[1].sum() == 0 and cm[0].sum() > 0
    check(ce, kind, rng, pool, 4, D, excluded=[])
    cm, pred, _, _ = check(ce, kind, rng, pool, 4, D, excluded=list(range(pool.T)))
    assert cm.sum() == 0 and (pred == -1).all()


# ---- 4. ties and special values ----------------------------------------------------------
@pytest.mark.parametrize("D", [12, 260])
def test_gnb_ties_and_special_values(ce, D):
    """User 0: four classes with identical parameters and priors (the first
    index wins); user 1: classes 1 and 3 identical and nearest (1 wins); user
    2: ordinary models over rows with NaN and +-inf."""
    rng = np.random.default_rng(40)
    C = 4
    pool = Pool(rng, [[9, 14], [30], [5, 5, 15]], shuffled=True)
    X = rng.normal(0, 1, (pool.F, D))
    th, va, pr = gnb_models(rng, pool.U, C, D)
    th[0], va[0], pr[0] = th[0, 0], va[0, 0], 0.25
    th[1, 3], va[1, 3], pr[1] = th[1, 1], va[1, 1], [0.2, 0.3, 0.2, 0.3]
    th[1, 0] += 6.0
    th[1, 2] -= 6.0
    rows2 = np.flatnonzero(pool.user == 2)
    X[rows2[0], 3] = np.nan
    X[rows2[1], 0], X[rows2[2], D - 1] = np.inf, -np.inf
    X[rows2[3], 5], X[rows2[3], 6] = np.inf, -np.inf
    X[rows2[4]] = 1e200
    y = rng.integers(0, C, pool.F).astype(np.int32)
    cm, pred, scores, _ = check(ce, "gnb", rng, pool, C, D, X=X, models=(th, va, pr), y=y)
    r0, r1 = pool.user == 0, pool.user == 1
    assert (bits(scores[r0]) == bits(scores[r0][:, :1])).all() and (pred[r0] == 0).all()
    assert (bits(scores[r1][:, 1]) == bits(scores[r1][:, 3])).all() and (pred[r1] == 1).all()
    assert np.isnan(scores[rows2[0]]).all() and pred[rows2[0]] == 0  # NaN everywhere: its first occurrence
    assert (scores[rows2[1]] == -np.inf).all() and pred[rows2[1]] == 0
    # a zero prior: jll -inf, never the maximum among finite scores
    pr[2] = [0.0, 0.5, 0.25, 0.25]
    _, pred, scores, _ = check(ce, "gnb", rng, pool, C, D, X=X, models=(th, va, pr), y=y)
    fin = np.isfinite(scores[rows2][:, 1])
    assert (scores[rows2][fin, 0] == -np.inf).all() and (pred[rows2][fin] != 0).all()


@pytest.mark.parametrize("D", [12, 260])
def test_sgd_ties_and_special_values(ce, D):
    rng = np.random.default_rng(41)
    C = 4
    pool = Pool(rng, [[9, 14], [30], [5, 5, 15]], shuffled=True)
    X = rng.normal(0, 1, (pool.F, D))
    co, ic = sgd_models(rng, pool.U, C, D)
    co[0], ic[0] = co[0, 0], ic[0, 0]          # four identical problems: the first index wins
    co[1, 3], ic[1, 3] = co[1, 1], ic[1, 1]    # 1 and 3 tie ...
    ic[1, 1] = ic[1, 3] = 50.0                  # ... and are the maximum
    rows2 = np.flatnonzero(pool.user == 2)
    X[rows2[0], 3] = np.nan
    X[rows2[1], 0] = np.inf
    X[rows2[2], D - 1] = -np.inf
    X[rows2[3], 5], X[rows2[3], 6] = np.inf, -np.inf
    y = rng.integers(0, C, pool.F).astype(np.int32)
    _, pred, scores, _ = check(ce, "sgd", rng, pool, C, D, X=X, models=(co, ic), y=y)
    r0, r1 = pool.user == 0, pool.user == 1
    assert (bits(scores[r0]) == bits(scores[r0][:, :1])).all() and (pred[r0] == 0).all()
    assert (bits(scores[r1][:, 1]) == bits(scores[r1][:, 3])).all() and (pred[r1] == 1).all()
    assert np.isnan(scores[rows2[0]]).all() and pred[rows2[0]] == 0
    assert np.isinf(scores[rows2[1]]).all()


def test_binary_sgd_scores_of_plus_and_minus_zero(ce):
    """K = 1: score > 0 is class 1.  A score of exactly +0.0 and of -0.0 (eight
    products that underflow to -0.0, added to an intercept of -0.0) and a NaN
    give class 0; the smallest positive scores class 1."""
    rng = np.random.default_rng(42)
    D = 8
    pool = Pool(rng, [[4], [4]])
    X = np.zeros((pool.F, D))
    X[0], X[1], X[2], X[3] = -1e-200, 1e-200, 1e-100, np.nan
    X[4:] = rng.normal(0, 1, (4, D))
    co = np.stack([np.full((1, D), 1e-200), np.zeros((1, D))])
    ic = np.array([[-0.0], [0.0]])
    y = np.array([0, 1, 1, 0, 1, 0, 1, 0], np.int32)
    cm, pred, scores, counted = check(ce, "sgd", rng, pool, 2, D, X=X, models=(co, ic), y=y)
    assert counted.all()
    assert bits(scores[0, 0]) == bits(-0.0) and bits(scores[1, 0]) == bits(0.0) and scores[2, 0] > 0
    assert (bits(scores[4:, 0]) == bits(0.0)).all()
    assert pred.tolist() == [0, 0, 1, 0, 0, 0, 0, 0]
    assert cm.tolist() == [[[2, 0], [1, 1]], [[2, 0], [2, 0]]]


# ---- 5. F1 ---------------------------------------------------------------------------------
def test_f1_hand_built_matrices(ce):
    rng = np.random.default_rng(50)
    for C in (2, 3, 4, 8):
        cms = [np.zeros((C, C), np.int64) for _ in range(6)]
        cms[0][:, 0] = rng.integers(1, 9, C)                      # only class 0 is ever predicted
        cms[1][0, :] = rng.integers(1, 9, C)                      # only class 0 is ever true
        cms[2][C - 1, C - 1] = 1                                  # a single row
        cms[3] = rng.integers(1, 50, (C, C)) * (1 - np.eye(C, dtype=np.int64))  # all wrong
        cms[4] = rng.integers(1, 1000, (C, C))                    # every class present (C = 8: the tree)
        # cms[5]: an empty user
        cms += [rng.integers(0, 3, (C, C)) * rng.integers(0, 2, (C, 1)) for _ in range(300)]
        cms.append(rng.integers(0, 1 << 40, (C, C)))
        cm = np.stack(cms).astype(np.int64)
        want = np.array([f1_weighted(m) for m in cm])
        assert want[0] < 1 and want[2] == 1.0 and want[3] == 0.0 and np.isnan(want[5])
        f1, rep = ce.ops.f1_weighted_users(dev(cm), report=True)
        assert same_bits(f1.cpu().numpy(), want), C
        assert np.array_equal(bits(rep.cpu().numpy()), bits(np.stack([prf(m) for m in cm]))), C
    with pytest.raises(ValueError, match="int64"):
        ce.ops.f1_weighted_users(torch.zeros((2, 4, 4), dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="int64"):
        ce.ops.f1_weighted_users(torch.zeros((2, 4, 3), dtype=torch.int64, device="cuda"))


def test_sklearn_fixture_end_to_end(ce):
    """The committed sklearn outputs: models -> evaluate -> sklearn's F1 bits,
    GaussianNB, one-vs-rest SGD and binary SGD; the labels are sklearn's too."""
    z = golden("members_eval_sklearn")
    U, C = z["prior"].shape
    es = ce.EvalSet.from_s_id(z["X"], z["y"], z["s_id"], item_offsets=z["item_offsets"])
    es2 = ce.EvalSet.from_s_id(z["X"], z["y2"], z["s_id"], item_offsets=z["item_offsets"])
    assert es.U == U and es.X.is_cuda and es.y.dtype == torch.int32
    nb = ce.DeviceGaussianNB(z["theta"], z["var"], np.ones((U, C)), class_prior=z["prior"])
    sg = ce.DeviceSGDClassifier(z["coef"], z["intercept"], 1.0, random_state=0)
    sg2 = ce.DeviceSGDClassifier(z["coef2"], z["intercept2"], 1.0, random_state=0)
    for m, s, name in ((nb, es, "gnb"), (sg, es, "sgd"), (sg2, es2, "sgd2")):
        f1, cm, rep = m.evaluate(s, report=True)
        assert same_bits(f1.cpu().numpy(), z["f1_" + name]), name
        f1b, cmb = m.evaluate(s)
        assert same_bits(f1b.cpu().numpy(), z["f1_" + name]) and torch.equal(cm, cmb)
        user, _ = row_owners(z["item_offsets"], s.frame_offsets.cpu().numpy(), s.frame_perm.cpu().numpy(), s.F)
        want = confusion(s.y.cpu().numpy(), z["pred_" + name], m.C, user, U)
        assert np.array_equal(cm.cpu().numpy(), want), name
        assert np.array_equal(bits(rep.cpu().numpy()), bits(np.stack([prf(c) for c in want])))
    kw = dict(item_offsets=es.item_offsets, frame_offsets=es.frame_offsets, frame_perm=es.frame_perm, y=es.y,
              return_pred=True)
    assert np.array_equal(ce.ops.gnb_score_users(es.X, nb.theta, nb.var, nb.class_prior, **kw)[1].cpu().numpy(),
                          z["pred_gnb"])
    assert np.array_equal(ce.ops.sgd_score_users(es.X, sg.coef, sg.intercept, **kw)[1].cpu().numpy(), z["pred_sgd"])
    m = ce.mean_f1([nb.evaluate(es)[0], sg.evaluate(es)[0]]).cpu().numpy()
    assert same_bits(m, [np.mean([a, b]) for a, b in zip(z["f1_gnb"], z["f1_sgd"])])
    with pytest.raises(ValueError, match="one encoded class per row"):
        ce.ops.gnb_score_users(es.X, nb.theta, nb.var, nb.class_prior, es.item_offsets, es.frame_offsets, es.y[:-1])
    with pytest.raises(ValueError, match=r"4 user\(s\).*3 model"):
        ce.ops.sgd_score_users(es.X, sg.coef[:3], sg.intercept[:3], es.item_offsets, es.frame_offsets, es.y)


# ---- 6. the loop ---------------------------------------------------------------------------
Q, EPOCHS, C_LOOP, D_LOOP = 4, 3, 4, 20
SONGS = [14, 13, 20, 15, 16, 18]  # six ragged users
SEEDS = [7, 8, 9, 10, 11, 12]


def loop_data(rng, mode):
    U = len(SONGS)
    off = np.concatenate([[0], np.cumsum(SONGS)]).astype(np.int64)
    T = int(off[-1])
    s_id = rng.permutation(np.repeat(np.arange(T), rng.integers(1, 7, T)))
    centers = rng.normal(0, 1, (U, C_LOOP, D_LOOP))
    song_labels = rng.integers(0, C_LOOP, T)
    owner = np.searchsorted(off, s_id, side="right") - 1
    X = centers[owner, song_labels[s_id]] + rng.normal(0, 2.0, (len(s_id), D_LOOP))
    # every user's test songs: a few frames each, rows shuffled
    t_songs = rng.integers(2, 6, U)
    t_off = np.concatenate([[0], np.cumsum(t_songs)]).astype(np.int64)
    t_sid = rng.permutation(np.repeat(np.arange(int(t_off[-1])), rng.integers(2, 9, int(t_off[-1]))))
    t_owner = np.searchsorted(t_off, t_sid, side="right") - 1
    yt = rng.integers(0, C_LOOP, len(t_sid)).astype(np.int32)
    Xt = centers[t_owner, yt] + rng.normal(0, 2.0, (len(t_sid), D_LOOP))
    kw, h2m = {}, [None] * U
    if mode == "mix":
        tabs = []
        for n in SONGS:
            n_rows = int(0.8 * n) + 2
            m = np.concatenate([rng.permutation(n)[:n_rows - 2], np.full(2, -1)])[rng.permutation(n_rows)].astype(np.int64)
            tabs.append((np.round(rng.dirichlet(np.ones(4), n_rows), 1), m))
        off_h = np.concatenate([[0], np.cumsum([len(t[1]) for t in tabs])]).astype(np.int64)
        kw = dict(hc=np.concatenate([t[0] for t in tabs]), hc_offsets=off_h, hc_to_mc=np.concatenate([t[1] for t in tabs]))
        h2m = [t[1] for t in tabs]
    gnb0 = [(rng.normal(0, 0.5, (C_LOOP, D_LOOP)), (rng.random((C_LOOP, D_LOOP)) + 0.5) * 4.0,
             rng.integers(1, 50, C_LOOP).astype(np.float64)) for _ in range(U)]
    sgd0 = [(rng.normal(0, 0.5, (C_LOOP, D_LOOP)), rng.normal(0, 0.5, C_LOOP), float(rng.integers(2, 5000)))
            for _ in range(U)]
    return dict(off=off, s_id=s_id, X=X, song_labels=song_labels, owner=owner, t_off=t_off, t_sid=t_sid,
                t_owner=t_owner, Xt=Xt, yt=yt, kw=kw, h2m=h2m, gnb0=gnb0, sgd0=sgd0)


def loop_build(ce, d, mode):
    _, f_off, f_perm = ce.song_groups(d["s_id"])
    sess = ce.BatchedSelectionSession(Q, mode, d["off"], frame_offsets=f_off, frame_perm=f_perm, **d["kw"])
    nb = ce.DeviceGaussianNB(*[np.stack([s[i] for s in d["gnb0"]]) for i in range(3)])
    sg = ce.DeviceSGDClassifier(*[np.stack([s[i] for s in d["sgd0"]]) for i in range(3)], random_state=SEEDS)
    bufs = [torch.zeros((len(d["s_id"]), C_LOOP), dtype=torch.float64, device="cuda") for _ in range(2)]
    return sess, nb, sg, bufs


def loop_epoch(ce, Xd, labels_d, es, sess, nb, sg, bufs):
    nb.predict_proba_session(Xd, sess, out=bufs[0])
    sg.predict_proba_session(Xd, sess, out=bufs[1])
    idx = sess.step(frames=bufs)
    nb.partial_fit_picks(Xd, sess, idx, labels_d)
    sg.partial_fit_picks(Xd, sess, idx, labels_d)
    f1g, cmg = nb.evaluate(es)
    f1s, cms = sg.evaluate(es)
    return idx, f1g, cmg, f1s, cms, ce.mean_f1([f1g, f1s])


def host_eval(d, u, gnb, sgd):
    rows = d["t_owner"] == u
    th, va, cc = gnb[:3]
    prior = gnb[3] if len(gnb) > 3 else cc / cc.sum()
    out = []
    for s in (gnb_jll(d["Xt"][rows], th, va, prior), sgd_decision(d["Xt"][rows], sgd[0], sgd[1])):
        cm = confusion(d["yt"][rows], predict_labels(s), C_LOOP)[0]
        out.append((cm, f1_weighted(cm)))
    return out


@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_three_epochs_against_the_host_loop(ce, mode):
    """predict -> select -> retrain -> evaluate for 6 ragged users, both
    members: every epoch's f1 [U] and cm equal the host loop's -- the
    restatements of tests/gnb_fit_ref.py / tests/sgd_fit_ref.py retrained on the
    epoch's picks, then members_eval_ref over the user's test frames."""
    rng = np.random.default_rng(60 + len(mode))
    d = loop_data(rng, mode)
    U = len(SONGS)
    Xd, labels_d = dev(d["X"]), dev(d["song_labels"].astype(np.int64))
    es = ce.EvalSet.from_s_id(d["Xt"], d["yt"], d["t_sid"], item_offsets=d["t_off"])
    sess, nb, sg, bufs = loop_build(ce, d, mode)
    gnb, sgd = list(d["gnb0"]), list(d["sgd0"])
    # before epoch 0 (amg_test.py:411-413)
    f1g, cmg = nb.evaluate(es)
    for u in range(U):
        (cm_g, f_g), _ = host_eval(d, u, gnb[u], sgd[u])
        assert np.array_equal(cmg[u].cpu().numpy(), cm_g) and same_bits(f1g[u].cpu().numpy(), f_g)
    for e in range(EPOCHS):
        idx, f1g, cmg, f1s, cms, mean = loop_epoch(ce, Xd, labels_d, es, sess, nb, sg, bufs)
        picks = sess.account(idx)
        got = [t.cpu().numpy() for t in (f1g, cmg, f1s, cms, mean)]
        for u in range(U):
            p = np.asarray(picks[u])
            songs = [int(q) if q < SONGS[u] else int(d["h2m"][u][q - SONGS[u]]) for q in p if q >= 0]
            songs = np.array([s for s in songs if s >= 0], np.int64) + d["off"][u]
            batch = np.isin(d["s_id"], songs)
            if batch.any():
                yb = d["song_labels"][d["s_id"][batch]]
                gnb[u] = gnb_partial_fit(d["X"][batch], yb, *gnb[u][:3])
                sgd[u] = sgd_partial_fit(d["X"][batch], yb, *sgd[u], random_state=SEEDS[u])[:3]
            (cm_g, f_g), (cm_s, f_s) = host_eval(d, u, gnb[u], sgd[u])
            assert np.array_equal(got[1][u], cm_g) and np.array_equal(got[3][u], cm_s), (mode, e, u)
            assert same_bits(got[0][u], f_g) and same_bits(got[2][u], f_s), (mode, e, u)
            assert same_bits(got[4][u], np.mean([f_g, f_s])), (mode, e, u)
    sg.check_finite()


def test_epoch_with_evaluate_in_one_hip_graph(ce):
    """One epoch of both members -- predict, step, retrain, the two evaluates
    and mean_f1 -- captured as ONE HIP graph and replayed while the pools and
    the models change in place: every replay equals the eager epoch."""
    rng = np.random.default_rng(70)
    d = loop_data(rng, "mc")
    Xd, labels_d = dev(d["X"]), dev(d["song_labels"].astype(np.int64))
    es = ce.EvalSet.from_s_id(d["Xt"], d["yt"], d["t_sid"], item_offsets=d["t_off"])
    eager = loop_build(ce, d, "mc")
    want = [[t.cpu().numpy().copy() for t in loop_epoch(ce, Xd, labels_d, es, *eager)] for _ in range(EPOCHS)]
    assert any(not same_bits(want[0][1], w[1]) for w in want[1:])  # the models do change the F1
    torch.cuda.synchronize()
    graphed = loop_build(ce, d, "mc")
    ce.ops.reserve_graph_workspace(ce._lib.load().ce_select_batched_workspace_bytes(int(d["off"][-1]), len(SONGS), Q))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = loop_epoch(ce, Xd, labels_d, es, *graphed)
    for e in range(EPOCHS):
        g.replay()
        got = [t.cpu().numpy().copy() for t in outs]
        assert np.array_equal(got[0], want[e][0]), e
        for k in (1, 3, 5):
            assert same_bits(got[k], want[e][k]), (e, k)
        for k in (2, 4):
            assert np.array_equal(got[k], want[e][k]), (e, k)
    torch.cuda.synchronize()
