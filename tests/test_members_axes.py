"""The restatements behind tests/test_gpu_members_axes.py, pinned on the CPU to
numpy and to the installed sklearn: numpy's pairwise recursion (pw_shape /
pw_sum), the two orders of a class sum over 8 columns, the tail of
SGDClassifier.predict_proba (sgd_proba), GaussianNB's class sum at 8 near-tied
classes (oracle.ce_oracle.ref_gnb_predict_proba), and what the sweep's feature
counts and data cover (members_axes_cases)."""
import numpy as np
import pytest

import members_axes_cases as A
from members_eval_ref import gnb_jll, libm_exp, libm_log, sgd_decision
from members_proba_ref import (left_to_right, ovr_normalise, pw_shape, pw_sum, row_sums, seq_sum, sgd_proba,
                               sgd_proba_from_decision, tree8_sum)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---- 1. numpy's pairwise recursion ---------------------------------------------------
def test_pairwise_recursion_is_numpys_for_every_feature_count():
    """pw_sum over pw_shape's halves equals np.sum(X, 1) in all 64 bits for
    every D in 1..512, magnitudes over six decades."""
    rng = np.random.default_rng(7)
    differs = 0
    for D in range(1, 513):
        X = rng.normal(0, 1, (5, D)) * 10.0 ** rng.uniform(-3, 3, (5, D))
        want = np.sum(X, 1)
        assert np.array_equal(bits(row_sums(X)), bits(want)), D
        differs += int((bits(left_to_right(X)) != bits(want)).any())
        leaves, height = pw_shape(D)
        assert sum(ln for _, ln in leaves) == D and all(ln <= 128 for _, ln in leaves)
        assert [s for s, _ in leaves] == [int(v) for v in np.cumsum([0] + [ln for _, ln in leaves[:-1]])]
        assert all(s % 8 == 0 for s, _ in leaves), "a leaf starts at lane 0 of an 8-lane group"
        assert height == 0 if D <= 128 else height >= 1
    assert differs > 400  # the order matters on this data: the plain sum has other bits at most D


def test_plan_classes_of_every_feature_count():
    assert {(len(pw_shape(D)[0]), pw_shape(D)[1]) for D in range(8, 513)} == A.PLAN_CLASSES
    assert pw_shape(260) == ([(0, 128), (128, 64), (192, 68)], 2)  # the leaf layout the 260 kernels hard-code
    assert pw_sum([]) == 0.0 and np.signbit(pw_sum([-0.0, -0.0]))


def test_sweep_covers_every_plan_shape():
    """The feature counts of the GPU sweep: every plan class, every tail length
    of a last leaf, both sides of every rung of the kernels' NX ladder."""
    classes, tails, rungs = A.plan_coverage(A.DS)
    assert classes == A.PLAN_CLASSES
    assert tails == set(range(8))
    assert rungs == {(nx, side) for nx in A.NX_LADDER for side in ("last", "next")} - {(64, "next")}  # 513 > kMaxFeat
    assert {pw_shape(D)[1] for D in A.SPECIAL_DS} == {0, 1, 2, 3}
    assert {(len(pw_shape(D)[0]), pw_shape(D)[1]) for D in A.SPECIAL_DS} == A.PLAN_CLASSES
    assert all(pw_shape(D)[0][-1][1] % 8 for D in A.SPECIAL_DS)
    assert set(A.ALL_COUNTS_DS) <= set(A.DS) and set(A.SPECIAL_DS) <= set(A.DS)


def test_sweep_data_has_teeth():
    """On the sweep's own inputs a wrong order changes bits: for D >= 16 the
    pairwise (GaussianNB) / 8-chain (SGD) feature sum differs from the plain
    left-to-right one in at least half the rows, and at 8 classes the tree and
    the sequential class sum differ in at least one row."""
    for D in A.DS + A.SGD_SMALL_DS:
        if D >= 8:
            X, models = A.gnb_case(D)
            for m in models[:1]:
                if D >= 16:
                    assert 2 * A.gnb_sum_teeth(X, m) >= A.F, D
                assert A.class_sum_teeth(A.gnb_class_terms(gnb_jll(X, *A.gnb_model(m, 8)))) >= 1, D
        X, models = A.sgd_case(D)
        if D >= 16:
            assert 2 * A.sgd_sum_teeth(X, models[0]) >= A.F, D
        assert A.class_sum_teeth(A.sgd_class_terms(sgd_decision(X, *models[0]))) >= 1, D


# ---- 2. the order of a class sum ---------------------------------------------------------
@pytest.mark.parametrize("W", range(2, 9))
def test_class_sum_order_follows_the_memory_order(W):
    """np.sum(E, axis=1) of [F, W]: an F-ordered array is added column after
    column (GaussianNB's jll is np.array(jll).T); a C-ordered one row by row,
    each row one pairwise leaf -- sequential below 8 terms, the 8-accumulator
    tree at 8 (SGD's prob.sum(axis=1))."""
    rng = np.random.default_rng(W)
    E = rng.random((4000, W)) * 10.0 ** rng.uniform(-1, 1, (4000, W))
    if W == 8:
        E = E[bits(tree8_sum(E)) != bits(seq_sum(E))]  # the rows on which the two orders differ
        assert len(E) > 500
    Ec, Ef = np.ascontiguousarray(E), np.asfortranarray(E)
    assert Ec.flags.c_contiguous and Ef.flags.f_contiguous and not Ef.flags.c_contiguous
    assert np.array_equal(bits(np.sum(Ef, axis=1)), bits(seq_sum(E)))
    assert np.array_equal(bits(np.sum(Ec, axis=1)), bits(tree8_sum(E) if W == 8 else seq_sum(E)))
    assert np.array_equal(bits(np.sum(np.array(list(E.T)).T, axis=1)), bits(seq_sum(E)))  # sklearn's jll layout
    if W == 8:
        assert (bits(np.sum(Ec, axis=1)) != bits(np.sum(Ef, axis=1))).all()
        assert np.array_equal(bits(np.exp(Ef).sum(axis=1)), bits(seq_sum(np.exp(E))))  # a ufunc keeps the layout


# ---- 3. SGD's tail against sklearn -----------------------------------------------------------
@pytest.mark.parametrize("K", range(1, 9))
def test_sgd_tail_is_sklearns_in_all_bits(K):
    """sklearn's own decision values through ovr_normalise equal
    SGDClassifier.predict_proba bit for bit (scipy's expit on both sides: only
    the normalisation is under test); at K = 8 the sequential sum would not."""
    linear = pytest.importorskip("sklearn.linear_model")
    from scipy.special import expit

    rng = np.random.default_rng(300 + K)
    D, n = 12, 5000
    est = linear.SGDClassifier(loss="log_loss")
    est.coef_ = rng.normal(0, 0.5, (K, D))
    est.intercept_ = rng.normal(0, 0.5, K)
    est.classes_ = np.arange(2 if K == 1 else K)
    X = rng.normal(0, 1, (n, D))
    d = est.decision_function(X).reshape(n, K)
    want = est.predict_proba(X)
    p = expit(d)
    assert np.array_equal(bits(ovr_normalise(p)), bits(want))
    if K > 1:
        off = (bits(p / seq_sum(p)[:, None]) != bits(want)).any(1).sum()
        assert (off > 1000) if K == 8 else (off == 0), off


def test_sgd_proba_against_sklearn_to_tolerance():
    """The whole restatement (the kernels' dot-product order, the C library's
    exp) against sklearn's BLAS order and scipy's expit: rtol 1e-10, the
    tolerance the GPU parity tests state for the one-model kernels."""
    linear = pytest.importorskip("sklearn.linear_model")
    rng = np.random.default_rng(31)
    for K in (1, 3, 8):
        est = linear.SGDClassifier(loss="log_loss")
        est.coef_, est.intercept_ = rng.normal(0, 0.3, (K, 33)), rng.normal(0, 0.5, K)
        est.classes_ = np.arange(2 if K == 1 else K)
        X = rng.normal(0, 1, (40, 33))
        got = sgd_proba(X, est.coef_, est.intercept_)
        assert got.shape == (40, 2 if K == 1 else K)
        np.testing.assert_allclose(got, est.predict_proba(X), rtol=1e-10, atol=1e-300)
        assert np.array_equal(bits(got), bits(sgd_proba_from_decision(sgd_decision(X, est.coef_, est.intercept_))))


# ---- 4. GaussianNB's class sum at 8 classes ---------------------------------------------------------
def near_tied(rng, n, C, D):
    mean, var = rng.normal(0, 1, D), 10.0 ** rng.uniform(-2, 2, D)
    theta = mean + (0.3 / np.sqrt(D)) * np.sqrt(var) * rng.normal(0, 1, (C, D))
    X = mean + np.sqrt(var) * rng.normal(0, 1, (n, D))
    return X, theta, np.tile(var, (C, 1)), rng.dirichlet(np.ones(C) * 5)


def test_ref_gnb_predict_proba_sums_eight_classes_in_sklearns_order():
    """8 near-tied classes (the class means a small perturbation of one mean,
    the variances shared): with numpy's own exp / log the restatement equals
    the installed GaussianNB.predict_proba at the tolerance tests/test_oracle.py
    states for C = 4; the class sum runs column after column, and forcing the
    8-accumulator tree instead changes bits on this data."""
    nb = pytest.importorskip("sklearn.naive_bayes")
    from oracle.ce_oracle import ref_gnb_predict_proba

    rng = np.random.default_rng(8)
    n, C, D = 300, 8, 40
    X, theta, var, prior = near_tied(rng, n, C, D)
    est = nb.GaussianNB()
    est.theta_, est.var_, est.class_prior_, est.classes_, est.n_features_in_ = theta, var, prior, np.arange(C), D
    got = ref_gnb_predict_proba(X, theta, var, prior, exp=np.exp, log=np.log)
    np.testing.assert_allclose(got, est.predict_proba(X), rtol=1e-9, atol=1e-300)
    # the teeth: the same restatement with a C-ordered exp (the 8-accumulator tree) has other bits
    forced = ref_gnb_predict_proba(X, theta, var, prior, exp=lambda a: np.ascontiguousarray(np.exp(a)), log=np.log)
    assert (bits(forced) != bits(got)).any(1).sum() >= 1
    # the default (the C library's exp / log) takes the same, sequential, order: its explicit statement
    jll = gnb_jll(X, theta, var, prior)
    mx = jll.max(1)
    E = libm_exp(jll - mx[:, None])
    assert A.class_sum_teeth(E) >= 1
    want = libm_exp(jll - (libm_log(seq_sum(E)) + mx)[:, None])
    assert np.array_equal(bits(ref_gnb_predict_proba(X, theta, var, prior)), bits(want))
    tree = libm_exp(jll - (libm_log(tree8_sum(E)) + mx)[:, None])
    assert (bits(tree) != bits(want)).any()


@pytest.mark.parametrize("C", [1, 2, 3, 5, 7])
def test_ref_gnb_predict_proba_below_eight_classes(C):
    """Fewer than 8 terms are added one after the other in either layout: the explicit statement's bits."""
    from oracle.ce_oracle import ref_gnb_predict_proba

    rng = np.random.default_rng(80 + C)
    X, theta, var, prior = near_tied(rng, 60, C, 24)
    jll = gnb_jll(X, theta, var, prior)
    mx = jll.max(1)
    want = libm_exp(jll - (libm_log(seq_sum(libm_exp(jll - mx[:, None]))) + mx)[:, None])
    assert np.array_equal(bits(ref_gnb_predict_proba(X, theta, var, prior)), bits(want))
