"""Restatements the linear members' predict_proba is tested against at every
pairwise-plan shape and class count (tests/test_members_axes.py pins them to
numpy and sklearn on the CPU; tests/test_gpu_members_axes.py compares the
kernels with them in all 64 bits):

  pw_shape    numpy's pairwise recursion over n terms: the leaves and the tree
              height, which the tests use to state their coverage
  pw_sum      that recursion summed as numpy sums a leaf (8 strided
              accumulators, their tree, a sequential tail), in Python floats
  seq_sum / tree8_sum
              the two orders np.sum(E, axis=1) takes over 8 columns: one term
              after the other (an F-ordered array, any width below 8) and the
              8-accumulator tree (a C-ordered [F, 8] array)
  sgd_proba   SGDClassifier(loss='log').predict_proba: sgd_decision (the
              kernels' fma chains), expit with the C library's exp, then
              sklearn's own ``p / p.sum(axis=1)`` on a C-contiguous array

GaussianNB's predict_proba is oracle.ce_oracle.ref_gnb_predict_proba."""
import numpy as np

from members_eval_ref import libm_exp, sgd_decision

PW_BLOCK = 128  # numpy's PW_BLOCKSIZE


def pw_shape(n):
    """(leaves, height) of numpy's pairwise sum over n terms: leaves a list of
    (start, length) in order, height the depth of the tree of additions above
    them.  n <= 128 is one leaf; above, n2 = n // 2 - (n // 2) % 8 terms go left."""
    if n <= PW_BLOCK:
        return [(0, n)], 0
    n2 = n // 2
    n2 -= n2 % 8
    left, hl = pw_shape(n2)
    right, hr = pw_shape(n - n2)
    return left + [(n2 + s, ln) for s, ln in right], 1 + max(hl, hr)


def pw_sum(a):
    """numpy's pairwise sum of the Python floats a (DOUBLE_pairwise_sum): fewer
    than 8 one after the other onto -0.0; up to 128 in 8 strided accumulators,
    ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)), then the n % 8 last terms in order;
    above, the two halves of pw_shape."""
    n = len(a)
    if n < 8:
        res = -0.0
        for v in a:
            res += v
        return res
    if n <= PW_BLOCK:
        r = list(a[:8])
        nb = n - n % 8
        for i in range(8, nb, 8):
            for k in range(8):
                r[k] += a[i + k]
        res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]))
        for v in a[nb:]:
            res += v
        return res
    n2 = n // 2
    n2 -= n2 % 8
    return pw_sum(a[:n2]) + pw_sum(a[n2:])


def row_sums(X):
    """np.sum(X, 1) of a [F, D] array by pw_sum: the reduction starts from 0.0."""
    return np.array([0.0 + pw_sum([float(v) for v in row]) for row in np.asarray(X, np.float64)])


def left_to_right(X):
    """The plain sum of every row, one term after the other from the first."""
    X = np.asarray(X, np.float64)
    acc = X[:, 0].copy()
    for f in range(1, X.shape[1]):
        acc = acc + X[:, f]
    return acc


def seq_sum(E):
    """The columns of E [F, W] added one after the other onto -0.0, then onto
    the reduction's 0.0: np.sum(E, axis=1) of an F-ordered array (numpy adds
    whole columns), and of any array narrower than 8."""
    E = np.asarray(E, np.float64)
    acc = np.full(E.shape[0], -0.0)
    for c in range(E.shape[1]):
        acc = acc + E[:, c]
    return 0.0 + acc


def tree8_sum(E):
    """np.sum(E, axis=1) of a C-ordered [F, 8] array: each row is one pairwise
    leaf of 8 terms, ((e0+e1)+(e2+e3))+((e4+e5)+(e6+e7))."""
    E = np.asarray(E, np.float64)
    assert E.shape[1] == 8
    return 0.0 + (((E[:, 0] + E[:, 1]) + (E[:, 2] + E[:, 3])) + ((E[:, 4] + E[:, 5]) + (E[:, 6] + E[:, 7])))


def ovr_normalise(p):
    """sklearn's _predict_proba_lr tail over the expits p [F, K]: [1 - p, p] for
    a binary model (K = 1), else ``p / p.sum(axis=1)`` -- numpy's own sum over a
    C-contiguous array, so 8 classes take the 8-accumulator tree and fewer are
    added one after the other."""
    p = np.ascontiguousarray(p, np.float64)
    if p.shape[1] == 1:
        return np.concatenate([1.0 - p, p], 1)
    with np.errstate(all="ignore"):
        return p / p.sum(axis=1).reshape((p.shape[0], 1))


def sgd_proba_from_decision(d):
    """expit with the C library's exp, then ovr_normalise."""
    with np.errstate(all="ignore"):
        return ovr_normalise(1.0 / (1.0 + libm_exp(-np.asarray(d, np.float64))))


def sgd_proba(X, coef, intercept):
    """[F, C] SGDClassifier(loss='log').predict_proba of one model: coef [K, D],
    intercept [K]; K = 1 is the binary model (C = 2)."""
    return sgd_proba_from_decision(sgd_decision(X, coef, intercept))
