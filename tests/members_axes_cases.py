"""The cases of the linear members' axes sweep (tests/test_gpu_members_axes.py;
tests/test_members_axes.py checks the same lists and data on the CPU): the
feature counts, what they cover in terms of numpy's pairwise plan
(members_proba_ref.pw_shape) and of the kernels' NX ladder, and the models and
frames -- magnitudes over several decades and near-tied classes, so that a
wrong order of additions changes bits, which `*_teeth` measure on the
restatements alone."""
import numpy as np

from members_eval_ref import _libm, libm_exp, sgd_decision
from members_proba_ref import left_to_right, pw_shape, seq_sum, tree8_sum

# both sides of every leaf count, tail length and NX rung (plan_coverage)
DS = [8, 9, 10, 11, 13, 14, 15, 16, 64, 65, 127, 128, 129, 130, 131, 133, 134, 135, 136, 192, 193, 248, 249, 251, 253,
      255, 256, 257, 260, 264, 288, 289, 320, 321, 384, 385, 448, 449, 488, 489, 498, 502, 503, 504, 505, 511, 512]
SGD_SMALL_DS = [1, 2, 7]          # SGD alone: GaussianNB refuses fewer than 8 features
ALL_COUNTS_DS = (9, 135, 511)     # every class count runs here
SPECIAL_DS = (15, 135, 255, 289, 511)  # one per plan class, each with a tail in its last leaf
NX_LADDER = (8, 16, 24, 32, 36, 40, 48, 56, 64)  # with_nx: features per lane of the 8-lane kernels
PLAN_CLASSES = {(1, 0), (2, 1), (3, 2), (4, 2), (5, 3)}  # (leaves, height) of every D in 8..512
F = 37            # one-model entries: four full 8-frame groups and a ragged five, one block
USERS = (5, 32)   # users and score forms: user 0 owns rows 0..4, user 1 rows 5..36


def plan_coverage(ds):
    """(plan classes, tail lengths of a last leaf, (NX, side) rungs) the feature counts ds reach."""
    classes, tails, rungs = set(), set(), set()
    for D in ds:
        leaves, height = pw_shape(D)
        classes.add((len(leaves), height))
        tails.add(leaves[-1][1] % 8)
        for nx in NX_LADDER:
            if D == 8 * nx:
                rungs.add((nx, "last"))
            if D == 8 * nx + 1:
                rungs.add((nx, "next"))
    return classes, tails, rungs


def gnb_counts(D):
    return tuple(range(1, 9)) if D in ALL_COUNTS_DS else (1, 2, 3, 4, 5, 8) if D == 260 else (1, 2, 3, 5, 8)


def sgd_counts(D):
    """K: 1 is the binary model (C = 2)."""
    return tuple(range(1, 9)) if D in ALL_COUNTS_DS else (1, 3, 4, 7, 8)


def gnb_case(D, seed=0):
    """X [F, D] and two 8-class GaussianNB models (A: the one-model entries and
    user 1; B: user 0) of near-tied classes: the class means a small
    perturbation of one mean, the variances all but shared and spread over six
    decades, the frames' distances over two and a half."""
    rng = np.random.default_rng(1000 * D + seed)
    mean = rng.normal(0, 1, D) * 10.0 ** rng.uniform(-1, 1, D)
    var = 10.0 ** rng.uniform(-3, 3, D)
    spread = 10.0 ** rng.uniform(-2, 0.5, D)
    X = mean + np.sqrt(var) * spread * rng.normal(0, 1, (F, D))
    models = []
    for _ in range(2):
        theta = mean + (0.3 / np.sqrt(D)) * np.sqrt(var) * rng.normal(0, 1, (8, D))
        v = var * np.exp(0.02 / np.sqrt(D) * rng.normal(0, 1, (8, D)))
        models.append((theta, v, rng.dirichlet(np.ones(8) * 3)))
    return X, models


def gnb_model(model, C):
    theta, var, prior = model
    return theta[:C], var[:C], prior[:C] / prior[:C].sum()


def sgd_case(D, seed=0):
    """X [F, D] and two 8-class SGD models (coef [8, D], intercept [8]): feature
    magnitudes over three decades, the products over two, decision values O(1)."""
    rng = np.random.default_rng(2000 * D + seed)
    scale = 10.0 ** rng.uniform(-2, 1, D)
    X = scale * rng.normal(0, 1, (F, D))
    models = []
    for _ in range(2):
        coef = rng.normal(0, 1, (8, D)) * 10.0 ** rng.uniform(-1, 1, D) / scale / np.sqrt(D)
        models.append((coef, rng.normal(0, 0.5, 8)))
    return X, models


def rows_off(a, b):
    """The number of rows in which the float64 vectors a and b differ in a bit."""
    return int((np.asarray(a, np.float64).view(np.uint64) != np.asarray(b, np.float64).view(np.uint64)).sum())


def gnb_sum_teeth(X, model):
    """Rows whose feature sum for class 0 (numpy's pairwise order) differs from the plain left-to-right sum."""
    theta, var, _ = model
    T = ((X - theta[0]) ** 2) / var[0]
    return rows_off(np.sum(T, 1), left_to_right(T))


def sgd_sum_teeth(X, model):
    """Rows whose decision value for class 0 (sgd_decision: 8 fma chains and the
    butterfly) differs from one left-to-right fma chain over the features."""
    coef, icpt = model
    seq = np.empty(len(X))
    for r in range(len(X)):
        d = 0.0
        for f in range(X.shape[1]):
            d = _libm.fma(float(X[r, f]), float(coef[0, f]), d)
        seq[r] = d + icpt[0]
    return rows_off(sgd_decision(X, coef[:1], icpt[:1])[:, 0], seq)


def class_sum_teeth(E):
    """Rows of E [F, 8] whose sum differs between the 8-accumulator tree and the sequential order."""
    return rows_off(tree8_sum(E), seq_sum(E))


def gnb_class_terms(jll):
    """exp(jll - max) [F, 8]: the terms of GaussianNB's class sum."""
    jll = np.asarray(jll, np.float64)
    return libm_exp(jll - jll.max(1, keepdims=True))


def sgd_class_terms(d):
    """expit(d) [F, 8]: the terms of SGD's one-vs-rest sum."""
    return 1.0 / (1.0 + libm_exp(-np.asarray(d, np.float64)))


def special_rows(X, model_mean, model_sd, D):
    """A copy of X whose first rows hold the special values: row 0 a NaN in the
    last feature (a tail lane of the last leaf); rows 1 and 2 +inf in the last
    leaf's first column and -inf in its last; row 3 both; row 4 forty standard
    deviations from model_mean in every feature."""
    X = np.array(X, np.float64)
    start, length = pw_shape(D)[0][-1]
    assert length % 8, "the last feature must be a tail lane"
    X[0, D - 1] = np.nan
    X[1, start] = np.inf
    X[2, start + length - 1] = -np.inf
    X[3, start], X[3, start + length - 1] = np.inf, -np.inf
    X[4] = model_mean + 40.0 * model_sd * np.where(np.arange(D) & 1, 1.0, -1.0)
    return X
