"""Writes tests/golden/gnb_partial_fit.npz: sklearn's own GaussianNB.partial_fit
(amg_test.py:509) on chained batches, the reference the device update is held
to where sklearn is absent.  Run with sklearn installed:

    python tests/golden/gen_gnb_partial_fit.py

Two cases, D = 12 and D = 260 (C = 4), keys prefixed d12_ / d260_:
  X [F, D]                           the frames every batch takes its rows from
  theta_init, var_init, cc_init      the fitted model before the first batch
                                     (class 3 unseen: cc_init[3] == 0)
  rows{e}, labels{e}  (e = 0, 1, 2)  batch e: ascending rows of X and their classes
                                     (batch 0 lacks class 1; class 3 first shows in batch 1)
  theta{e}, var{e}, cc{e}, prior{e}, eps{e}
                                     theta_, var_, class_count_, class_prior_,
                                     epsilon_ after batch e
"""
import os

import numpy as np
from sklearn.naive_bayes import GaussianNB

HERE = os.path.dirname(os.path.abspath(__file__))


def case(D, F, seed):
    rng = np.random.default_rng(seed)
    C = 4
    X = rng.normal(0, 1, (F, D)) * np.exp(rng.normal(0, 2, D))  # per-feature scales over a few decades
    X0 = rng.normal(0, 1, (9, D)) * 2.0
    y0 = np.arange(9) % 3  # class 3 unseen
    g = GaussianNB().partial_fit(X0, y0, classes=np.arange(C))
    out = {"X": X, "theta_init": g.theta_.copy(), "var_init": g.var_.copy(),
           "cc_init": g.class_count_.copy()}
    for e, n in enumerate((7, 16, F // 2)):
        rows = np.sort(rng.choice(F, n, replace=False)).astype(np.int64)
        labels = rng.integers(0, C, n).astype(np.int32)
        if e == 0:
            labels[labels == 1] = 0
            labels[labels == 3] = 2
        g.partial_fit(X[rows], labels)
        out.update({f"rows{e}": rows, f"labels{e}": labels, f"theta{e}": g.theta_.copy(), f"var{e}": g.var_.copy(),
                    f"cc{e}": g.class_count_.copy(), f"prior{e}": g.class_prior_.copy(),
                    f"eps{e}": np.float64(g.epsilon_)})
    return out


def main():
    out = {}
    for D, F, seed in ((12, 40, 12), (260, 48, 260)):
        out.update({f"d{D}_{k}": v for k, v in case(D, F, seed).items()})
    path = os.path.join(HERE, "gnb_partial_fit.npz")
    np.savez(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
