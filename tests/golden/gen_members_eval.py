"""Writes tests/golden/members_eval_sklearn.npz: sklearn's own evaluate step
(amg_test.py:513-515: mod.predict(X_test), f1_score(average='weighted')) for a
few users' fitted GaussianNB and SGDClassifier(loss='log_loss') models, the
reference the device evaluate is held to where sklearn is absent.  Run with
sklearn installed (written with 1.7.2):

    python tests/golden/gen_members_eval.py

Keys (U = 4 users, C = 4 classes, D = 20 features; every user's test songs one
after the other, a song's frame rows shuffled through s_id):
  X [F, D], y [F] int32        the test frames of every user and their classes
                               (user 2's test set lacks class 3)
  s_id [F]                     the stacked test song of every row
  item_offsets [U + 1]         user u's stacked songs
  theta, var [U, C, D], prior [U, C]     the users' fitted GaussianNB (theta_, var_, class_prior_)
  coef [U, C, D], intercept [U, C]       the users' fitted SGDClassifier (coef_, intercept_)
  pred_gnb, pred_sgd [F] int32           mod.predict of every row by its user's model
  f1_gnb, f1_sgd [U]                     f1_score(y_user, pred_user, average='weighted')
  y2 [F] int32, coef2 [U, 1, D], intercept2 [U, 1], pred_sgd2 [F], f1_sgd2 [U]
                               the same for binary SGD models (classes 0 / 1)
The generator asserts on EVERY row that the top two SGD decision values (binary:
the value and 0) are further apart than 1e-9 * max|decision|: BLAS's dot order
differs from the kernels' by about 1e-13 relative, so the labels do not depend on it.
"""
import os

import numpy as np
from sklearn.linear_model import SGDClassifier
from sklearn.metrics import f1_score
from sklearn.naive_bayes import GaussianNB

HERE = os.path.dirname(os.path.abspath(__file__))
U, C, D = 4, 4, 20


def assert_gap(dec):
    dec = np.asarray(dec, np.float64)
    if dec.ndim == 1:
        gap = np.abs(dec)
    else:
        top = np.sort(dec, axis=1)
        gap = top[:, -1] - top[:, -2]
    assert (gap > 1e-9 * np.abs(dec).max()).all(), "a decision gap below 1e-9 relative: reseed"


def main():
    rng = np.random.default_rng(19870513)
    songs = [5, 3, 6, 4]  # test songs per user
    item_offsets = np.concatenate([[0], np.cumsum(songs)]).astype(np.int64)
    T = int(item_offsets[-1])
    frames = rng.integers(3, 17, T)
    s_id = np.repeat(np.arange(T), frames)
    user = np.searchsorted(item_offsets, s_id, side="right") - 1
    F = len(s_id)
    # rows shuffled within each user's block of X (a user's X_test is their rows, in X's order)
    for u in range(U):
        rows = np.flatnonzero(user == u)
        s_id[rows] = s_id[rows][rng.permutation(len(rows))]
    out = {"s_id": s_id.astype(np.int64), "item_offsets": item_offsets}
    X = np.empty((F, D))
    y, y2 = np.empty(F, np.int32), np.empty(F, np.int32)
    th, va, pr = np.empty((U, C, D)), np.empty((U, C, D)), np.empty((U, C))
    co, ic = np.empty((U, C, D)), np.empty((U, C))
    co2, ic2 = np.empty((U, 1, D)), np.empty((U, 1))
    pg, ps, ps2 = np.empty(F, np.int32), np.empty(F, np.int32), np.empty(F, np.int32)
    f1g, f1s, f1s2 = np.empty(U), np.empty(U), np.empty(U)
    for u in range(U):
        centers = rng.normal(0, 1, (C, D))
        ytr = np.concatenate([np.arange(C), rng.integers(0, C, 200)])
        Xtr = centers[ytr] + rng.normal(0, 2.5, (len(ytr), D))
        rows = np.flatnonzero(user == u)
        yt = rng.integers(0, C if u != 2 else C - 1, len(rows))
        Xt = centers[yt] + rng.normal(0, 2.5, (len(rows), D))
        X[rows], y[rows], y2[rows] = Xt, yt, yt & 1
        g = GaussianNB().fit(Xtr, ytr)
        s = SGDClassifier(loss="log_loss", penalty="l2", random_state=1987 + u, max_iter=20, tol=None).fit(Xtr, ytr)
        s2 = SGDClassifier(loss="log_loss", penalty="l2", random_state=7 + u, max_iter=20, tol=None).fit(Xtr, ytr & 1)
        assert_gap(s.decision_function(Xt))
        assert_gap(s2.decision_function(Xt))
        th[u], va[u], pr[u] = g.theta_, g.var_, g.class_prior_
        co[u], ic[u], co2[u], ic2[u] = s.coef_, s.intercept_, s2.coef_, s2.intercept_
        pg[rows], ps[rows], ps2[rows] = g.predict(Xt), s.predict(Xt), s2.predict(Xt)
        f1g[u] = f1_score(yt, pg[rows], average="weighted")
        f1s[u] = f1_score(yt, ps[rows], average="weighted")
        f1s2[u] = f1_score(yt & 1, ps2[rows], average="weighted")
    out.update(X=X, y=y, y2=y2, theta=th, var=va, prior=pr, coef=co, intercept=ic, coef2=co2, intercept2=ic2,
               pred_gnb=pg, pred_sgd=ps, pred_sgd2=ps2, f1_gnb=f1g, f1_sgd=f1s, f1_sgd2=f1s2)
    np.savez_compressed(os.path.join(HERE, "members_eval_sklearn.npz"), **out)
    print("wrote members_eval_sklearn.npz:", F, "rows;", "f1", f1g, f1s, f1s2)


if __name__ == "__main__":
    main()
