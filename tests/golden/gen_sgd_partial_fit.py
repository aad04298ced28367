"""Writes tests/golden/sgd_partial_fit.npz: sklearn's own SGDClassifier.partial_fit
(amg_test.py:509 for the 'classifier_sgd' member, deam_classifier.py:214-217) on
chained batches, the reference the device update is held to where sklearn is
absent.  Run with sklearn 1.7.2 installed:

    python tests/golden/gen_sgd_partial_fit.py

`cases` lists the case names; every key of a case is prefixed "<name>_":
  C, alpha, random_state, scale      the model's settings; X is scaled by `scale`
  X [F, D]                           the frames every batch takes its rows from
  coef_init [K, D], intercept_init [K], t_init
                                     the model before the first batch: fitted with
                                     .fit, or fresh (zeros, t = 1: the first batch
                                     goes through partial_fit(..., classes=))
  rows{e}, labels{e}  (e = 0 .. 3)   batch e: ascending rows of X and their classes
                                     (batch 0 is one row; batch 1 lacks class 1)
  coef{e}, intercept{e}, t{e}        coef_, intercept_, t_ after batch e
alpha = 1 and 10 on a fresh model reach the zero shrink factor and the wscale
reset; scale = 1e3 reaches p <= -37.
"""
import os
import warnings

import numpy as np
from sklearn.linear_model import SGDClassifier

HERE = os.path.dirname(os.path.abspath(__file__))

#        name         C  D    F   alpha  fresh  scale
CASES = [("c2_d1",    2, 1,   40, 1e-4,  False, 1.0),
         ("c3_d63",   3, 63,  40, 1e-4,  False, 1.0),
         ("c4_d64",   4, 64,  40, 1e-4,  False, 1.0),
         ("c8_d65",   8, 65,  48, 1e-4,  False, 1.0),
         ("c4_d260",  4, 260, 48, 1e-4,  False, 1.0),
         ("c2_d9_a1", 2, 9,   40, 1.0,   True,  1.0),
         ("c3_d7_a1", 3, 7,   40, 1.0,   True,  1.0),
         ("c4_d12_a10", 4, 12, 40, 10.0, True,  1.0),
         ("c4_d33_big", 4, 33, 40, 1e-4, False, 1e3)]


def case(name, C, D, F, alpha, fresh, scale, seed):
    rng = np.random.default_rng(seed)
    random_state = int(rng.integers(0, 10000))
    K = 1 if C == 2 else C
    X = rng.normal(0, 1, (F, D)) * scale
    m = SGDClassifier(loss="log_loss", penalty="l2", random_state=random_state, warm_start=True, alpha=alpha)
    if fresh:
        init = (np.zeros((K, D)), np.zeros(K), 1.0)
    else:
        m.fit(rng.normal(0, 1, (6 * C, D)) * scale, np.arange(6 * C) % C)
        init = (m.coef_.copy(), m.intercept_.copy(), float(m.t_))
    out = {"C": np.int64(C), "alpha": np.float64(alpha), "random_state": np.int64(random_state),
           "scale": np.float64(scale), "X": X, "coef_init": init[0], "intercept_init": init[1],
           "t_init": np.float64(init[2])}
    for e, n in enumerate((1, 7, 16, F // 2)):
        rows = np.sort(rng.choice(F, n, replace=False)).astype(np.int64)
        labels = rng.integers(0, C, n).astype(np.int32)
        if e == 1:
            labels[labels == 1] = 0
        if fresh and e == 0:
            m.partial_fit(X[rows], labels, classes=np.arange(C))
        else:
            m.partial_fit(X[rows], labels)
        assert m.coef_.shape == (K, D)
        out.update({f"rows{e}": rows, f"labels{e}": labels, f"coef{e}": m.coef_.copy(),
                    f"intercept{e}": m.intercept_.copy(), f"t{e}": np.float64(m.t_)})
    return out


def main():
    warnings.simplefilter("ignore")
    out = {"cases": np.array([c[0] for c in CASES])}
    for i, c in enumerate(CASES):
        out.update({f"{c[0]}_{k}": v for k, v in case(*c, seed=1000 + i).items()})
    path = os.path.join(HERE, "sgd_partial_fit.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
