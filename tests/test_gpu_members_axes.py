"""The linear members at every pairwise-plan shape and class count, against
restatements that share no code with the kernels (ce_gnb_predict_proba,
ce_sgd_predict_proba, their *_users forms and the *_score_users scores):

  GaussianNB  oracle.ce_oracle.ref_gnb_predict_proba (numpy's own pairwise
              np.sum, the C library's exp / log, sklearn's order of the class
              sum) and members_eval_ref.gnb_jll for the scores
  SGD         members_proba_ref.sgd_proba (the documented fma chains and
              butterfly, the C library's exp, numpy's prob.sum(axis=1)) and
              members_eval_ref.sgd_decision for the scores

Every comparison is in all 64 bits; a NaN must be a NaN on both sides.  The
feature counts (members_axes_cases.DS) reach every (leaves, height) class of
numpy's pairwise plan, every tail length of a last leaf and both sides of every
rung of the kernels' NX ladder; the data spreads magnitudes over several decades
and keeps the classes near-tied, and every test measures on the restatements
alone that a wrong order would change bits.  The geometry is trivial (37 rows;
users of 5 and 32 frames): the other member tests cover it."""
import numpy as np
import pytest
import torch

import members_axes_cases as A
from members_eval_ref import gnb_jll, sgd_decision
from members_proba_ref import pw_shape, sgd_proba_from_decision
from test_gpu_members_eval import STREAMED, Pool, dev, last_kernel

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


@pytest.fixture(scope="module")
def pool():
    p = Pool(np.random.default_rng(0), [[n] for n in A.USERS])
    assert p.F == A.F and [int((p.user == u).sum()) for u in range(2)] == list(A.USERS)
    return p


def assert_bits(got, want, what):
    """All 64 bits, NaN for NaN (the sign and payload of a NaN are not values)."""
    got, want = np.ascontiguousarray(got, np.float64), np.ascontiguousarray(want, np.float64)
    assert got.shape == want.shape, what
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), (what, "NaN rows differ")
    bad = (got.view(np.uint64) != want.view(np.uint64)) & ~nan
    assert not bad.any(), (what, np.argwhere(bad)[:6].tolist(), got[bad][:3].tolist(), want[bad][:3].tolist())


def frames(X, ld):
    """X on the device, as a view of row pitch ld when given."""
    if ld is None:
        return dev(X)
    buf = torch.full((X.shape[0], ld), 7.5, dtype=torch.float64, device="cuda")  # the padding is never read
    buf[:, :X.shape[1]] = dev(X)
    return buf[:, :X.shape[1]]


def stack(models):
    """Per-user models (user 0: B, user 1: A) as the users forms take them: [U, ...] arrays."""
    return [np.stack([b, a]) for a, b in zip(*models)]


def per_user(pool, ref, models):
    """[F, cols] rows of user u by ref(rows, model u); models = (A, B), user 0 holds B."""
    parts = [ref(pool.user == u, models[1 - u]) for u in range(2)]
    out = np.empty((pool.F, parts[0].shape[1]))
    for u in range(2):
        out[pool.user == u] = parts[u]
    return out


# ---- GaussianNB ---------------------------------------------------------------------------
def gnb_check(ce, pool, X, models, C, ld=None, what=()):
    """The three entries at C classes against the restatements; models = (A, B) of C classes."""
    from oracle.ce_oracle import ref_gnb_predict_proba

    Xd = frames(X, ld)
    with np.errstate(all="ignore"):
        got = ce.ops.gnb_predict_proba(Xd, *models[0]).cpu().numpy()
        assert_bits(got, ref_gnb_predict_proba(X, *models[0]), (*what, C, "one-model"))
        st = [dev(a) for a in stack(models)]
        got = ce.ops.gnb_predict_proba_users(Xd, *st, **pool.geometry()).cpu().numpy()
        assert_bits(got, per_user(pool, lambda r, m: ref_gnb_predict_proba(X[r], *m), models), (*what, C, "users"))
        y = dev((np.arange(pool.F) % max(C, 2)).astype(np.int32))
        if C == 1:  # the score entry counts into a [C, C] matrix of at least two classes
            with pytest.raises(ValueError, match="bad GaussianNB shapes"):
                ce.ops.gnb_score_users(Xd, *st, **pool.geometry(), y=y, return_scores=True)
            return
        _, _, scores = ce.ops.gnb_score_users(Xd, *st, **pool.geometry(), y=y, return_scores=True)
        assert_bits(scores.cpu().numpy(), per_user(pool, lambda r, m: gnb_jll(X[r], *m), models), (*what, C, "scores"))


@pytest.mark.parametrize("D,ld", [(D, None) for D in A.DS] + [(260, 264)])
def test_gnb_every_plan_shape_and_class_count(ce, pool, D, ld):
    X, models = A.gnb_case(D)
    leaves, height = pw_shape(D)
    if D >= 16:
        assert 2 * A.gnb_sum_teeth(X, models[0]) >= A.F  # a wrong feature order would change bits
    assert A.class_sum_teeth(A.gnb_class_terms(gnb_jll(X, *A.gnb_model(models[0], 8)))) >= 1  # and a wrong class order
    for C in A.gnb_counts(D):
        gnb_check(ce, pool, X, [A.gnb_model(m, C) for m in models], C, ld, what=(D, len(leaves), height))
        if (D, C) == (260, 4):
            assert last_kernel(ce) == (STREAMED if ld is None else "ce::k_gnb_score_users<36, 260>")


def test_gnb_refuses_fewer_than_eight_features(ce, pool):
    """numpy sums fewer than 8 terms sequentially and the 8-lane kernels have no leaf for them: CE_EUNSUPPORTED."""
    X, models = A.gnb_case(8)
    models = [tuple(a[..., :7] if a.ndim == 2 else a for a in A.gnb_model(m, 4)) for m in models]
    Xd = dev(X[:, :7])
    st = [dev(a) for a in stack(models)]
    y = dev(np.zeros(pool.F, np.int32))
    for call in (lambda: ce.ops.gnb_predict_proba(Xd, *models[0]),
                 lambda: ce.ops.gnb_predict_proba_users(Xd, *st, **pool.geometry()),
                 lambda: ce.ops.gnb_score_users(Xd, *st, **pool.geometry(), y=y)):
        with pytest.raises(ce.CEError, match="D >= 8") as e:
            call()
        assert e.value.code == ce._lib.CE_EUNSUPPORTED


@pytest.mark.parametrize("D", A.SPECIAL_DS)
def test_gnb_special_values(ce, pool, D):
    """A NaN in the last feature (a tail lane), +-inf at the ends of the last
    leaf, a row 40 sigma from every class, a zero prior: C = 4 and C = 8."""
    X, models = A.gnb_case(D)
    mean, sd = models[0][0].mean(0), np.sqrt(models[0][1][0])
    for C in (4, 8):
        ms = [A.gnb_model(m, C) for m in models]
        Xs = A.special_rows(X, mean, sd, D)
        Xs[6] = Xs[4]  # the far row for user 1's model too (rows 0..4 are user 0's)
        gnb_check(ce, pool, Xs, ms, C, what=(D, "specials"))
        zero = [(th, va, np.concatenate([[0.0], pr[1:] / pr[1:].sum()])) for th, va, pr in ms]
        gnb_check(ce, pool, Xs, zero, C, what=(D, "zero prior"))
    got = ce.ops.gnb_predict_proba(dev(Xs), *zero[0]).cpu().numpy()
    assert np.isnan(got[[0, 1, 2, 3]]).all() and np.isfinite(got[4:]).all() and (got[4:, 0] == 0).all()
    assert np.array_equal(got[4:].sum(1).round(9), np.ones(A.F - 4))


# ---- SGD ------------------------------------------------------------------------------------
def sgd_check(ce, pool, X, models, dec, K, ld=None, what=()):
    """The three entries with the first K classes of models = (A, B); dec: their
    8-class decision values (A over all rows, B over user 0's), computed once."""
    Xd = frames(X, ld)
    ms = [(co[:K], ic[:K]) for co, ic in models]
    want = [dec[0][:, :K], dec[1][:, :K]]
    with np.errstate(all="ignore"):
        got = ce.ops.sgd_predict_proba(Xd, *ms[0]).cpu().numpy()
        assert_bits(got, sgd_proba_from_decision(want[0]), (*what, K, "one-model"))
        st = [dev(a) for a in stack(ms)]
        d_users = np.concatenate([want[1], want[0][A.USERS[0]:]])  # user 0: model B, user 1: model A
        got = ce.ops.sgd_predict_proba_users(Xd, *st, **pool.geometry()).cpu().numpy()
        assert_bits(got, sgd_proba_from_decision(d_users), (*what, K, "users"))
        y = dev((np.arange(pool.F) % max(K, 2)).astype(np.int32))
        _, _, scores = ce.ops.sgd_score_users(Xd, *st, **pool.geometry(), y=y, return_scores=True)
        assert_bits(scores.cpu().numpy(), d_users, (*what, K, "scores"))


def sgd_decisions(X, models):
    with np.errstate(all="ignore"):
        return sgd_decision(X, *models[0]), sgd_decision(X[:A.USERS[0]], *models[1])


@pytest.mark.parametrize("D,ld", [(D, None) for D in A.SGD_SMALL_DS + A.DS] + [(260, 264)])
def test_sgd_every_plan_shape_and_class_count(ce, pool, D, ld):
    """K = 1 is the binary model ([1 - p, p]); K = 8 takes numpy's 8-accumulator
    tree in the one-vs-rest sum; D = ld = 260, K = 4 is the span kernel."""
    X, models = A.sgd_case(D)
    dec = sgd_decisions(X, models)
    if D >= 16:
        assert 2 * A.sgd_sum_teeth(X, models[0]) >= A.F  # a wrong feature order would change bits
    assert A.class_sum_teeth(A.sgd_class_terms(dec[0])) >= 1  # and the sequential class sum at K = 8
    for K in A.sgd_counts(D):
        sgd_check(ce, pool, X, models, dec, K, ld, what=(D,))


@pytest.mark.parametrize("D", A.SPECIAL_DS)
def test_sgd_special_values(ce, pool, D):
    """A NaN in the last feature, +-inf at the ends of the last leaf, a far row,
    and a saturated model (coef * 50: expits of 0 and 1 among the classes)."""
    X, models = A.sgd_case(D)
    Xs = A.special_rows(X, 0.0, np.abs(X).mean(0), D)
    for scale in (1.0, 50.0):
        ms = [(co * scale, ic) for co, ic in models]
        dec = sgd_decisions(Xs, ms)
        if scale > 1:  # saturated: expits of exactly 1 and of all but 0 among the ordinary rows' classes
            p = A.sgd_class_terms(dec[0][5:])
            assert (p == 1.0).any() and (p < 1e-30).any()
        for K in (1, 4, 8):
            sgd_check(ce, pool, Xs, ms, dec, K, what=(D, "specials", scale))
    got = ce.ops.sgd_predict_proba(dev(Xs), *ms[0]).cpu().numpy()
    assert np.isnan(got[0]).all() and np.isfinite(got[5:]).all()
