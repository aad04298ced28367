"""The evaluate step of the linear members, the parts that need no GPU: the
numpy restatements of tests/members_eval_ref.py pinned to sklearn (where it is
importable) and to the committed sklearn outputs of
tests/golden/members_eval_sklearn.npz, the three entry points' refusals
(ce_gnb_score_users, ce_sgd_score_users, ce_f1_weighted_users) and the Python
validation in front of them (ops.*_score_users, EvalSet, evaluate, mean_f1)."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from members_eval_ref import confusion, f1_weighted, gnb_jll, predict_labels, prf, sgd_decision
from members_users_ref import row_owners


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. f1_weighted against sklearn, all 64 bits -----------------------------------
def label_cases(rng, C, n):
    """(y_true, y_pred) pairs of n rows over C classes: every class drawn;
    classes absent from y_true, from y_pred, from both; one class only."""
    full = np.arange(C)
    some = full[rng.random(C) < 0.6]
    some = some if len(some) else full[:1]
    other = full[rng.random(C) < 0.6]
    other = other if len(other) else full[-1:]
    yield rng.integers(0, C, n), rng.integers(0, C, n)
    yield rng.choice(some, n), rng.integers(0, C, n)          # absent from y_true
    yield rng.integers(0, C, n), rng.choice(some, n)          # absent from y_pred
    yield rng.choice(some, n), rng.choice(some, n)            # absent from both
    yield rng.choice(some, n), rng.choice(other, n)           # each lacks classes of its own
    yield np.full(n, C - 1), np.full(n, rng.integers(0, C))   # one class
    t = rng.integers(0, C, n)
    yield t, np.where(rng.random(n) < 0.8, t, rng.integers(0, C, n))  # mostly right


@pytest.mark.parametrize("C", [2, 3, 4, 7, 8])
def test_f1_weighted_is_sklearns_in_all_bits(C):
    metrics = pytest.importorskip("sklearn.metrics")
    import warnings

    rng = np.random.default_rng(100 + C)
    seen_all_present = False
    for n in (1, 2, 5, 17, 60, 257):
        for rep in range(6):
            for yt, yp in label_cases(rng, C, n):
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    want = metrics.f1_score(yt, yp, average="weighted")
                cm = confusion(yt, yp, C)[0]
                got = f1_weighted(cm)
                assert bits(got) == bits(want), (C, n, rep, got, want, cm.tolist())
                seen_all_present |= len(np.union1d(yt, yp)) == C
                with warnings.catch_warnings():
                    warnings.simplefilter("ignore")
                    p, r, f, s = metrics.precision_recall_fscore_support(yt, yp, labels=np.arange(C), zero_division=0)
                assert np.array_equal(bits(prf(cm)), bits(np.stack([p, r, f, s.astype(np.float64)], 1))), (C, n, rep)
    assert seen_all_present  # C = 8: the 8-term tree order was exercised
    assert np.isnan(f1_weighted(np.zeros((C, C), np.int64)))


def test_f1_weighted_hand_cases():
    assert f1_weighted([[3, 0], [0, 2]]) == 1.0
    assert f1_weighted([[0, 3], [2, 0]]) == 0.0
    assert f1_weighted([[1, 0], [0, 0]]) == 1.0  # a single row; class 1 absent
    # a class never predicted: f = [2*2/(3+2), 0], weights [3, 1]
    assert f1_weighted([[2, 1, 0], [1, 0, 0], [0, 0, 0]]) == ((2.0 * 2 / 6) * 3 + 0.0 * 1) / 4


# ---- 2. the label rules against sklearn ---------------------------------------------
def sk_gnb(theta, var, prior):
    from sklearn.naive_bayes import GaussianNB

    g = GaussianNB()
    g.theta_, g.var_, g.class_prior_, g.classes_ = theta, var, prior, np.arange(len(prior))
    g.n_features_in_ = theta.shape[1]
    return g


def sk_sgd(coef, intercept):
    from sklearn.linear_model import SGDClassifier

    s = SGDClassifier(loss="log_loss")
    s.coef_, s.intercept_ = coef, intercept
    s.classes_ = np.arange(2 if coef.shape[0] == 1 else coef.shape[0])
    s.n_features_in_ = coef.shape[1]
    return s


@pytest.mark.parametrize("C,D", [(2, 8), (4, 260), (8, 33)])
def test_argmax_of_gnb_jll_is_gaussiannb_predict(C, D):
    pytest.importorskip("sklearn")
    rng = np.random.default_rng(C * 1000 + D)
    theta, var, prior = rng.normal(0, 1, (C, D)), rng.random((C, D)) + 0.1, rng.dirichlet(np.ones(C) * 3)
    X = theta[rng.integers(0, C, 300)] + rng.normal(0, 1.5, (300, D))
    got = predict_labels(gnb_jll(X, theta, var, prior))
    want = sk_gnb(theta, var, prior).predict(X)
    assert np.array_equal(got, want)
    assert len(np.unique(want)) == C


def gapped_sgd(rng, C, D, F):
    """Seeded SGD inputs whose top-two decision gap (binary: |score|) is above 1e-9 * max|score| on EVERY row."""
    K = 1 if C == 2 else C
    coef, intercept = rng.normal(0, 0.5, (K, D)), rng.normal(0, 0.5, K)
    X = rng.normal(0, 1, (F, D))
    dec = X @ coef.T + intercept
    top = np.sort(dec, axis=1)
    gap = np.abs(dec[:, 0]) if K == 1 else top[:, -1] - top[:, -2]
    assert (gap > 1e-9 * np.abs(dec).max()).all()
    return X, coef, intercept


@pytest.mark.parametrize("C,D", [(2, 7), (3, 20), (4, 260), (8, 9)])
def test_label_rule_over_sgd_decision_is_sgdclassifier_predict(C, D):
    pytest.importorskip("sklearn")
    X, coef, intercept = gapped_sgd(np.random.default_rng(C * 1000 + D), C, D, 120)
    dec = sgd_decision(X, coef, intercept)
    np.testing.assert_allclose(dec, X @ coef.T + intercept, rtol=1e-10, atol=1e-12)
    got = predict_labels(dec, binary=C == 2)
    assert np.array_equal(got, sk_sgd(coef, intercept).predict(X))
    assert len(np.unique(got)) > 1  # more than one class is predicted


def test_label_rule_edges():
    nan = np.nan
    s = np.array([[1.0, 3.0, 3.0, 2.0], [0.0, 5.0, -1.0, 5.0], [1.0, nan, 7.0, nan], [nan, 9.0, 9.0, 9.0],
                  [-np.inf, -np.inf, -np.inf, -np.inf], [2.0, np.inf, np.inf, nan]])
    assert predict_labels(s).tolist() == [1, 1, 1, 0, 0, 3]
    assert predict_labels(np.array([[0.0], [-0.0], [nan], [1e-300], [-1.0], [np.inf]]), binary=True).tolist() == \
        [0, 0, 0, 1, 0, 1]


# ---- 3. the committed sklearn outputs -------------------------------------------------
def fixture_owner(z):
    import ce_amd

    _, f_off, f_perm = ce_amd.song_groups(z["s_id"])
    user, _ = row_owners(z["item_offsets"], f_off, f_perm, len(z["s_id"]))
    return user


def test_fixture_is_reproduced_by_the_restatements():
    """No sklearn needed: the restatements give the fixture's labels and F1 bits."""
    z = golden("members_eval_sklearn")
    user = fixture_owner(z)
    U, C = z["prior"].shape
    assert (user >= 0).all()
    for name, y, binary in (("gnb", z["y"], False), ("sgd", z["y"], False), ("sgd2", z["y2"], True)):
        pred = np.empty(len(y), np.int32)
        for u in range(U):
            rows = user == u
            if name == "gnb":
                s = gnb_jll(z["X"][rows], z["theta"][u], z["var"][u], z["prior"][u])
            else:
                k = "2" if binary else ""
                s = sgd_decision(z["X"][rows], z["coef" + k][u], z["intercept" + k][u])
            pred[rows] = predict_labels(s, binary)
        assert np.array_equal(pred, z["pred_" + name]), name
        cm = confusion(y, pred, 2 if binary else C, user, U)
        assert np.array_equal(bits([f1_weighted(m) for m in cm]), bits(z["f1_" + name])), name
    assert 3 not in z["y"][user == 2]  # a class absent from one user's test set


def test_fixture_is_sklearns_where_importable():
    pytest.importorskip("sklearn")
    from sklearn.metrics import f1_score

    z = golden("members_eval_sklearn")
    user = fixture_owner(z)
    for u in range(len(z["prior"])):
        rows = user == u
        pg = sk_gnb(z["theta"][u], z["var"][u], z["prior"][u]).predict(z["X"][rows])
        ps = sk_sgd(z["coef"][u], z["intercept"][u]).predict(z["X"][rows])
        assert np.array_equal(pg, z["pred_gnb"][rows]) and np.array_equal(ps, z["pred_sgd"][rows])
        assert bits(f1_score(z["y"][rows], pg, average="weighted")) == bits(z["f1_gnb"][u])
        assert bits(f1_score(z["y"][rows], ps, average="weighted")) == bits(z["f1_sgd"][u])


# ---- 4. refusals without a GPU ---------------------------------------------------------
def test_entry_points_refuse_without_gpu():
    from ce_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)
    for name in ("ce_gnb_score_users", "ce_sgd_score_users", "ce_f1_weighted_users"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)

    def gnb(F=10, D=260, ld=None, C=4, U=2, items=p, frames=p, y=p, cm=p, scores=None, lds=0, X=p):
        return lib.ce_gnb_score_users(X, F, D, D if ld is None else ld, p, p, p, C, U, items, frames, None, None, y, cm,
                                      None, scores, lds, None)

    def sgd(F=10, D=260, ld=None, K=4, C=4, U=2, items=p, frames=p, y=p, cm=p, scores=None, lds=0, X=p):
        return lib.ce_sgd_score_users(X, F, D, D if ld is None else ld, p, p, K, C, U, items, frames, None, None, y, cm,
                                      None, scores, lds, None)

    for f in (gnb, sgd):
        assert f(D=513) == _lib.CE_EINVAL and f(D=0) == _lib.CE_EINVAL
        assert f(C=9, **({"K": 9} if f is sgd else {})) == _lib.CE_EINVAL
        assert f(C=1, **({"K": 1} if f is sgd else {})) == _lib.CE_EINVAL
        assert f(U=0) == _lib.CE_EINVAL and f(U=-1) == _lib.CE_EINVAL
        assert f(items=None) == _lib.CE_EINVAL and f(frames=None) == _lib.CE_EINVAL
        assert b"offsets" in lib.ce_last_error()
        assert f(ld=259) == _lib.CE_EINVAL and f(F=-1) == _lib.CE_EINVAL
        assert f(y=None) == _lib.CE_EINVAL and b"y or cm" in lib.ce_last_error()
        assert f(cm=None) == _lib.CE_EINVAL and f(cm=None, F=0) == _lib.CE_EINVAL
        assert f(X=None) == _lib.CE_EINVAL
        assert f(scores=p, lds=0) == _lib.CE_EINVAL and b"ld_scores" in lib.ce_last_error()
        assert lib.ce_last_kernel() == b""
    assert gnb(scores=p, lds=3) == _lib.CE_EINVAL and sgd(scores=p, lds=3) == _lib.CE_EINVAL
    assert sgd(K=1, C=2, scores=p, lds=0) == _lib.CE_EINVAL
    for D in range(1, 8):
        assert gnb(D=D) == _lib.CE_EUNSUPPORTED
    assert sgd(K=3, C=4) == _lib.CE_EINVAL and sgd(K=1, C=3) == _lib.CE_EINVAL and sgd(K=4, C=3) == _lib.CE_EINVAL
    f1 = lib.ce_f1_weighted_users
    assert f1(p, 0, 4, p, None, None) == _lib.CE_EINVAL and f1(p, 3, 1, p, None, None) == _lib.CE_EINVAL
    assert f1(p, 3, 9, p, None, None) == _lib.CE_EINVAL
    assert f1(None, 3, 4, p, None, None) == _lib.CE_EINVAL and f1(p, 3, 4, None, None, None) == _lib.CE_EINVAL


def test_python_validation_without_gpu():
    torch = pytest.importorskip("torch")
    import ce_amd
    from ce_amd import ops

    rng = np.random.default_rng(1)
    s_id = np.array([2, 0, 1, 2, 0, 3, 3, 1, 4, 5, 5, 4])
    F, C, D = len(s_id), 4, 8
    X, y = rng.normal(0, 1, (F, D)), rng.integers(0, C, F)
    es = ce_amd.EvalSet.from_s_id(X, y, s_id, item_offsets=[0, 2, 2, 6], device="cpu")
    _, f_off, f_perm = ce_amd.song_groups(s_id)
    assert es.U == 3 and es.T == 6 and es.F == F and es.D == D and es._rows == F and es.excl is None
    geo = es.frame_geometry()
    assert geo[0].tolist() == f_off.tolist() and geo[1].tolist() == f_perm.tolist() and geo[2].tolist() == [0, 2, 2, 6]
    assert es.y.dtype == torch.int32 and es.y.tolist() == y.tolist() and es.X.dtype == torch.float64
    one = ce_amd.EvalSet(X, y, [0, 5, 12], device="cpu")  # grouped rows, one user owning every song
    assert one.U == 1 and one.frame_geometry()[1] is None and one.frame_geometry()[2].tolist() == [0, 2]
    assert ce_amd.EvalSet(X, y, [0, 1, 3], frame_perm=[4, 0, 9, 11], device="cpu")._rows == 10
    for bad, match in ((dict(frame_offsets=[0, 5, 13]), "X has 12 rows.*names 13"),
                       (dict(frame_offsets=[0, 5, 4]), "non-decreasing"),
                       (dict(frame_offsets=[0, 5, 12], item_offsets=[0, 3]), "names 3 songs"),
                       (dict(frame_offsets=[0, 5, 12], item_offsets=[0]), "U \\+ 1 >= 2"),
                       (dict(frame_offsets=[0, 5, 12], item_offsets=[0, 2, 1]), "non-decreasing"),
                       (dict(frame_offsets=[0, 5, 12], frame_perm=np.arange(11)), "frame_perm must hold"),
                       (dict(frame_offsets=[0, 5, 12], frame_perm=-np.arange(12)), "frame_perm must hold")):
        with pytest.raises(ValueError, match=match):
            ce_amd.EvalSet(X, y, device="cpu", **bad)
    with pytest.raises(ValueError, match="one integer class per row"):
        ce_amd.EvalSet(X, y[:-1], [0, 5, 12], device="cpu")
    with pytest.raises(ValueError, match="one integer class per row"):
        ce_amd.EvalSet(X, y.astype(np.float64), [0, 5, 12], device="cpu")
    with pytest.raises(ValueError, match="X must be a float64"):
        ce_amd.EvalSet(torch.zeros((F, D), dtype=torch.float32), y, [0, 5, 12], device="cpu")
    nb = {U: ce_amd.DeviceGaussianNB(np.zeros((U, C, D)), np.ones((U, C, D)), np.ones((U, C)), device="cpu")
          for U in (1, 3)}
    sg = {U: ce_amd.DeviceSGDClassifier(np.zeros((U, C, D)), np.zeros((U, C)), 1.0, random_state=0, device="cpu")
          for U in (1, 3)}
    wide = ce_amd.EvalSet(rng.normal(0, 1, (F, D + 1)), y, [0, 5, 12], device="cpu")
    for members in (nb, sg):
        with pytest.raises(ValueError, match=r"3 user\(s\), this member 1 model"):
            members[1].evaluate(es)
        with pytest.raises(ValueError, match=r"1 user\(s\), this member 3 model"):
            members[3].evaluate(one)
        with pytest.raises(ValueError, match="9 features, this member 8"):
            members[1].evaluate(wide)
        with pytest.raises(TypeError, match="EvalSet"):
            members[1].evaluate((X, y))
        # everything the host can check passes: the refusal left is that there is no CPU path
        with pytest.raises(ValueError, match="HIP device"):
            members[3].evaluate(es)
        with pytest.raises(ValueError, match="HIP device"):
            members[1].evaluate(one, report=True)
    with pytest.raises(ValueError, match="HIP device"):
        ops.f1_weighted_users(torch.zeros((2, 4, 4), dtype=torch.int64))
    with pytest.raises(ValueError, match="HIP device"):
        ops.gnb_score_users(es.X, nb[3].theta, nb[3].var, nb[3].class_prior, es.item_offsets, es.frame_offsets, es.y)
    with pytest.raises(ValueError, match="HIP device"):
        ops.sgd_score_users(es.X, sg[3].coef, sg[3].intercept, es.item_offsets, es.frame_offsets, es.y)
    # mean_f1: np.mean of a list of members' F1, bit for bit below 8 members
    for n in (1, 2, 3, 7):
        fs = [rng.random(5) for _ in range(n)]
        got = ce_amd.mean_f1([torch.from_numpy(f) for f in fs]).numpy()
        want = [np.mean([f[u] for f in fs]) for u in range(5)]
        assert np.array_equal(bits(got), bits(want)), n
    with pytest.raises(ValueError, match="at least one"):
        ce_amd.mean_f1([])
    with pytest.raises(ValueError, match="fewer than 8"):
        ce_amd.mean_f1([torch.zeros(2, dtype=torch.float64)] * 8)
