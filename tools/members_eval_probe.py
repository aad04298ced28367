"""The batched evaluate step of profiles/members_eval.json: after the retrain,
every user's model predicts that user's test frames and the labels are scored
(amg_test.py:513-515) -- one score launch and one F1 launch per member for all
users, against the predict_proba launch over the same geometry and against the
host loop it replaces.

  python tools/members_eval_probe.py [out.json]
      per member (gnb, sgd): U = 500 users x 3 test songs x 40 frames, X_test
      [60000, 260], C = 4 -- device time per call from a graph replay (the
      windows of a and b alternate), the eager median next to it:
        a  the evaluate: ce_*_score_users (its memset of cm included) and
           ce_f1_weighted_users; also each of the two on its own
        b  ce_*_predict_proba_users over the same geometry: the same bytes of X
           and of the models, strictly more arithmetic (logsumexp / expit) and
           an [F, C] f64 output
        c  the host loop: 500 x (mod.predict(X_test_u), f1_score(...,
           average='weighted')) with sklearn, the models' parameters already on
           the host (wall time; null where sklearn is absent)
      and the ratios a/b and c/a.
  python tools/members_eval_probe.py pmc gnb|sgd
      5 eager score launches of that member, then 5 predict_proba launches, and
      nothing else: the program to run under rocprofv3 --pmc (one run per
      counter set, no tracing options).
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "consensus-entropy_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ce_amd  # noqa: E402
import ce_amd.ops as ops  # noqa: E402

U, SONGS, FPS, D, C = 500, 3, 40, 260, 4
COMMAND = "python tools/members_eval_probe.py profiles/members_eval.json"


def graph_of(fn, per):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per):
            fn()
    return g


def timed(run, per):
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    run()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3 / per


def device_us_pair(fns, n_win=12, per=20):
    """Device time per call of each of `fns`: `per` calls captured in one HIP
    graph each, the replays timed with device events in alternating windows;
    the eager calls' median next to it."""
    graphs = [graph_of(f, per) for f in fns]
    out, eager = [[] for _ in fns], [[] for _ in fns]
    for _ in range(n_win):
        for i, g in enumerate(graphs):
            out[i].append(timed(g.replay, per))
    for _ in range(n_win):
        for i, f in enumerate(fns):
            eager[i].append(timed(lambda: [f() for _ in range(per)], per))
    return [{"us_min": min(o), "us_median": float(np.median(o)), "us_max": max(o), "windows": n_win,
             "calls_per_window": per, "eager_us_median": float(np.median(e)), "command": COMMAND}
            for o, e in zip(out, eager)]


def host_loop(kind, X, y, models):
    """Wall seconds of the 500 predict + f1_score calls, or None without sklearn."""
    try:
        from sklearn.linear_model import SGDClassifier
        from sklearn.metrics import f1_score
        from sklearn.naive_bayes import GaussianNB
    except ImportError:
        return None
    mods = []
    for u in range(U):
        if kind == "gnb":
            m = GaussianNB()
            m.theta_, m.var_, m.class_prior_ = models[0][u], models[1][u], models[2][u]
        else:
            m = SGDClassifier(loss="log_loss")
            m.coef_, m.intercept_ = models[0][u], models[1][u]
        m.classes_, m.n_features_in_ = np.arange(C), D
        mods.append(m)
    R = SONGS * FPS
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        f1 = [f1_score(y[u * R:(u + 1) * R], mods[u].predict(X[u * R:(u + 1) * R]), average="weighted")
              for u in range(U)]
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    assert len(f1) == U
    return best


def main(out_path, pmc=None):
    ce_amd.load()
    rng = np.random.default_rng(1987)
    F, T = U * SONGS * FPS, U * SONGS
    X = rng.normal(0, 1, (F, D))
    y = rng.integers(0, C, F).astype(np.int32)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    f_off = torch.arange(T + 1, dtype=torch.int64, device="cuda") * FPS
    item_off = torch.arange(U + 1, dtype=torch.int64, device="cuda") * SONGS
    out = torch.zeros((F, C), dtype=torch.float64, device="cuda")
    gnb = (rng.normal(0, 1, (U, C, D)), rng.random((U, C, D)) + 0.5, rng.dirichlet(np.ones(C) * 5, U))
    sgd = (rng.normal(0, 0.1, (U, C, D)), rng.normal(0, 0.5, (U, C)))
    gnb_d, sgd_d = [torch.from_numpy(m).cuda() for m in gnb], [torch.from_numpy(m).cuda() for m in sgd]
    lib = ce_amd._lib.load()

    def evaluate(kind):
        if kind == "gnb":
            return lambda: ops.f1_weighted_users(ops.gnb_score_users(Xd, *gnb_d, item_off, f_off, yd)[0])
        return lambda: ops.f1_weighted_users(ops.sgd_score_users(Xd, *sgd_d, item_off, f_off, yd)[0])

    def score_only(kind):  # the memset of cm and the score kernel, without the F1 launch
        if kind == "gnb":
            return lambda: ops.gnb_score_users(Xd, *gnb_d, item_off, f_off, yd)
        return lambda: ops.sgd_score_users(Xd, *sgd_d, item_off, f_off, yd)

    cm0 = torch.from_numpy(rng.integers(0, 40, (U, C, C))).cuda()

    def f1_only():
        return ops.f1_weighted_users(cm0)

    def proba(kind):
        if kind == "gnb":
            return lambda: ops.gnb_predict_proba_users(Xd, *gnb_d, item_off, f_off, None, None, out)
        return lambda: ops.sgd_predict_proba_users(Xd, *sgd_d, item_off, f_off, None, None, out)

    if pmc is not None:
        for fn in (evaluate(pmc), proba(pmc)):  # two kernels, told apart by name
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return
    res = {"command": COMMAND,
           "shape": {"users": U, "test_songs_per_user": SONGS, "frames_per_song": FPS, "F": F, "D": D, "C": C},
           "bytes_of_X": F * D * 8, "rows": []}
    for kind in ("gnb", "sgd"):
        a, b, a_score, a_f1 = device_us_pair([evaluate(kind), proba(kind), score_only(kind), f1_only])
        evaluate(kind)()
        kernel = lib.ce_last_kernel().decode()
        c = host_loop(kind, X, y, gnb if kind == "gnb" else sgd)
        row = {"member": kind, "score_kernel": kernel, "a": a, "b": b, "a_score_launch_only": a_score,
               "a_f1_launch_only": a_f1,
               "c_host_loop_us": None if c is None else c * 1e6, "a_over_b": a["us_median"] / b["us_median"],
               "c_over_a": None if c is None else c * 1e6 / a["us_median"], "launches": {"a": 2, "b": 1, "c": 0},
               "command": COMMAND}
        res["rows"].append(row)
        print(json.dumps(row), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "pmc":
        main(None, pmc=sys.argv[2])
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
