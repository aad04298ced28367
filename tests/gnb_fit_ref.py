"""GaussianNB.partial_fit restated with explicit row loops (no np.sum, so the
bits do not depend on the numpy build): the update the reference runs at
amg_test.py:509 on an already-fitted model, `mod.partial_fit(X_batch, y_batch)`
with priors=None (sklearn _partial_fit + _update_mean_variance).

Every operation below is an elementwise IEEE f64 add, subtract, multiply or true
divide over a row of D features; the only reductions are `colsum` (rows added
one after the other, in row order, onto +0.0) and the running maximum of
`nanmax0`.  tests/test_gnb_partial_fit.py pins it to sklearn bit for bit."""
import numpy as np


def colsum(A):
    """np.add.reduce(A, axis=0) of a C-contiguous [n, D >= 2] block."""
    s = np.zeros(A.shape[1], dtype=np.float64)  # +0.0
    for r in range(A.shape[0]):
        s = s + A[r]
    return s


def mean0(A):
    return colsum(A) / A.shape[0]


def var0(A):
    """np.var(A, axis=0): its own mean, the deviations squared by a multiply."""
    d = A - colsum(A) / A.shape[0]
    return colsum(d * d) / A.shape[0]


def nanmax0(v):
    """np.max of a vector: NaN if any element is NaN."""
    m = v[0]
    for x in v[1:]:
        if np.isnan(m):
            break
        if np.isnan(x) or x > m:
            m = x
    return m


def count_sum(cc):
    """class_count_.sum(): whole numbers far below 2^53, so any order of summation is exact."""
    s = cc[0]
    for x in cc[1:]:
        s = s + x
    return s


def gnb_partial_fit(X, y, theta, var, class_count, var_smoothing=1e-9):
    """One partial_fit of a fitted model on the batch (X [n >= 1, D >= 2] in
    batch order, y [n] in [0, C)).  Returns new (theta, var, class_count,
    class_prior, epsilon); the inputs are left alone."""
    X = np.ascontiguousarray(X, dtype=np.float64)
    y = np.asarray(y)
    theta, var, cc = np.array(theta, np.float64), np.array(var, np.float64), np.array(class_count, np.float64)
    C = theta.shape[0]
    eps = np.float64(var_smoothing) * nanmax0(var0(X))
    var = var - eps
    for c in range(C):
        Xc = X[y == c]
        n_new = Xc.shape[0]
        if n_new == 0:
            continue
        new_var, new_mu = var0(Xc), mean0(Xc)
        n_past = cc[c]
        if n_past == 0:
            theta[c], var[c] = new_mu, new_var
        else:
            n_total = float(n_past + n_new)
            mu = theta[c].copy()
            theta[c] = (float(n_new) * new_mu + n_past * mu) / n_total
            d = mu - new_mu
            ssd = (n_past * var[c] + float(n_new) * new_var) + (float(n_new) * n_past / n_total) * (d * d)
            var[c] = ssd / n_total
        cc[c] = cc[c] + float(n_new)
    var = var + eps
    return theta, var, cc, cc / count_sum(cc), eps


def same_bits(a, b):
    """0 ulp: equal bit patterns, a NaN matching any NaN (numpy fixes neither the
    sign nor the payload of a NaN an operation produces)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb]))
