"""The on-device XGBoost refit of profiles/xgb_fit.json: the retrain step of one
epoch (amg_test.py:507) for every user in one call, at the reference's shape,
and the other steps of the same epoch beside it.

  python tools/bench_xgb_fit.py [out.json] [--users 500] [--rounds 100] [--repeats 3]
      U users x 10 picked songs x 40 frames = 400 batch rows each, X [U * 800,
      260] f64 (20 songs per user), C = 4, max_depth 5, a synthetic base of 100
      rounds (400 trees).  One process, a warm-up fit, then the median of
      ``repeats`` timed calls per figure (device events around synchronised
      calls; a fit is far above the timer's resolution):
        fit_base       ops.xgb_fit_users end to end on base-only forests: the
                       three launches, the lane tables of the new trees and the
                       tree_ids / group_offsets rebuild, flags read back
        fit_tail       the same on forests that already carry one grown tail
        kernels        ce_xgb_fit_users alone (outputs and workspace allocated
                       before): all rounds, one round, and one round of depth-1
                       trees.  `round_ms` is the mean of rounds 2 .. n (the
                       difference over n - 1); `sort_ms` the depth-1 call less
                       the start margins: the finite check, every feature's
                       sort and four stumps, the nearest this gets to the sort
                       alone; `first_round_ms` the one-round call less that
        start_margins  the users walk over the batch rows (predict_proba_users
                       on the batch geometry: the same walk the fit launches)
        lane_tables    ce_xgb_lane_table over the new trees and the copy behind
                       the existing ones
        epoch          predict (three members), evaluate (three members), the
                       GaussianNB and SGD retrain, from the same run
      No host xgboost exists on these machines: there is no baseline, and no
      speed-up is claimed.  row_steps_per_s = rounds * G * depth * D * n * U /
      fit seconds.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "consensus-entropy_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ce_amd  # noqa: E402
import ce_amd.ops as ops  # noqa: E402
from ce_amd.xgb import StackedForests, synthetic_model  # noqa: E402

SONGS, PICKED, FPS, D, C, DEPTH, BASE_ROUNDS, T_SONGS = 20, 10, 40, 260, 4, 5, 100, 3


def timed(fn, repeats):
    """Median, min and max milliseconds of ``repeats`` synchronised calls."""
    ms = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": float(np.median(ms)), "ms_min": min(ms), "ms_max": max(ms), "repeats": repeats}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?", default=os.path.join(ROOT, "profiles", "xgb_fit.json"))
    ap.add_argument("--users", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    a = ap.parse_args()
    U, rounds, rep = a.users, a.rounds, a.repeats
    ce_amd.load()
    rng = np.random.default_rng(1987)
    F, n = U * SONGS * FPS, PICKED * FPS
    X = rng.normal(size=(F, D))
    song_labels = rng.integers(0, C, U * SONGS)
    X[:, :8] += 0.5 * song_labels[np.arange(F) // FPS, None]  # the classes differ: the trees have something to find
    Xd = torch.from_numpy(X).cuda()
    # every user's batch: the frames of its first PICKED songs, in X_train's order
    rows = np.concatenate([np.arange(u * SONGS * FPS, u * SONGS * FPS + n) for u in range(U)]).astype(np.int64)
    labels = song_labels[rows // FPS].astype(np.int32)
    off = (np.arange(U + 1) * n).astype(np.int64)
    rows_d, labels_d, off_d = torch.from_numpy(rows).cuda(), torch.from_numpy(labels).cuda(), torch.from_numpy(off).cuda()
    base = synthetic_model(n_rounds=BASE_ROUNDS, num_class=C, max_depth=DEPTH, num_feature=D, seed=1987)

    def fresh(tails=0):
        st = StackedForests(base, [None] * U)
        for _ in range(tails):
            ops.xgb_fit_users(Xd, rows_d, labels_d, st, off_d, rounds, DEPTH)
        return st

    def fit_on(tails):
        stacks = [fresh(tails) for _ in range(rep + 1)]
        it = iter(stacks)
        ops.xgb_fit_users(Xd, rows_d, labels_d, next(it), off_d, rounds, DEPTH)  # warm-up
        return timed(lambda: ops.xgb_fit_users(Xd, rows_d, labels_d, next(it), off_d, rounds, DEPTH), rep)

    res = {"command": "python tools/bench_xgb_fit.py profiles/xgb_fit.json" + "".join(
               f" --{k} {v}" for k, v, d in (("users", U, 500), ("rounds", rounds, 100), ("repeats", rep, 3)) if v != d),
           "shape": {"users": U, "rows_per_user": n, "D": D, "C": C, "rounds": rounds, "max_depth": DEPTH,
                     "base_trees": BASE_ROUNDS * C, "F": F},
           "baseline": "none: xgboost is not installed on these machines; the host fit this replaces is unmeasured"}
    res["fit_base"] = fit_on(0)
    res["fit_tail"] = fit_on(1)
    secs = res["fit_base"]["ms_median"] * 1e-3
    res["row_steps_per_s"] = rounds * C * DEPTH * D * n * U / secs

    # the entry point alone, everything allocated before
    st = fresh()
    table, cap, ids, L, goff, depth = st.device_args(Xd.device, D)
    p = ops._p

    def raw(r, max_depth=DEPTH):
        T = U * r * C
        o = [torch.zeros((T, 31, 2), dtype=torch.int32, device="cuda"), torch.zeros((T, 32), device="cuda")] + \
            [torch.zeros((T, 63), dtype=torch.int32, device="cuda") for _ in range(3)] + \
            [torch.zeros((T, 63), device="cuda"), torch.zeros((T, 63), dtype=torch.uint8, device="cuda"),
             torch.zeros(T, dtype=torch.int32, device="cuda")]
        flags = torch.zeros(U, dtype=torch.int32, device="cuda")
        wsb = int(ce_amd._lib.load().ce_xgb_fit_workspace_bytes(U * n, n, D, C, r))
        ws = torch.empty(wsb, dtype=torch.uint8, device="cuda")

        def go():
            ce_amd._lib.call("ce_xgb_fit_users", p(Xd), ce_amd._lib.CE_F64, F, D, D, p(rows_d), p(labels_d), p(off_d), U,
                             U * n, n, p(table), cap, p(ids), L, p(goff), C, depth, float(st.base_margin), r, max_depth,
                             0.3, 1.0, 1.0, *[p(t) for t in o], None, p(flags), p(ws), wsb, ops._stream(Xd.device))
        go()
        return timed(go, rep), o

    res["kernels_all_rounds"], o = raw(rounds)
    res["kernels_one_round"], _ = raw(1)
    res["kernels_one_round_depth1"], _ = raw(1, 1)
    if rounds > 1:
        res["round_ms"] = (res["kernels_all_rounds"]["ms_median"] - res["kernels_one_round"]["ms_median"]) / (rounds - 1)
    geo = dict(item_offsets=torch.arange(U + 1, dtype=torch.int64, device="cuda"), frame_offsets=off_d, frame_perm=rows_d)
    out = torch.zeros((F, C), dtype=torch.float32, device="cuda")
    res["start_margins"] = timed(lambda: ops.xgb_predict_proba_users(Xd, st, out=out, **geo), rep)
    res["sort_ms"] = res["kernels_one_round_depth1"]["ms_median"] - res["start_margins"]["ms_median"]
    res["first_round_ms"] = res["kernels_one_round"]["ms_median"] - res["kernels_one_round_depth1"]["ms_median"]
    T = U * rounds * C
    big = torch.zeros((2, 2 * T, 64, 2), dtype=torch.int32, device="cuda")

    def tables():
        big[:, T:2 * T] = st._lane_rows(o[0], o[1], T, depth, D, Xd.device)
    tables()
    res["lane_tables"] = timed(tables, rep)
    del big, o

    # the other steps of the epoch, same run: the members' probe's pool (every user's 20 songs)
    sess_off = (np.arange(U + 1) * SONGS).astype(np.int64)
    f_off = (np.arange(U * SONGS + 1) * FPS).astype(np.int64)
    sess = ce_amd.BatchedSelectionSession(PICKED, "mc", sess_off, frame_offsets=f_off)
    nb = ce_amd.DeviceGaussianNB(rng.normal(size=(U, C, D)), rng.random((U, C, D)) + 0.5,
                                 rng.integers(5, 50, (U, C)).astype(np.float64))
    sgd = ce_amd.DeviceSGDClassifier(rng.normal(size=(U, C, D)) * 0.01, np.zeros((U, C)), np.ones(U), random_state=7)
    xgb = ce_amd.DeviceXGBClassifier(base, U=U, device="cuda")
    xgb.fit(Xd, rows_d, labels_d, off_d, n_rounds=rounds, max_depth=DEPTH)
    Ft = U * T_SONGS * FPS
    es = ce_amd.EvalSet(torch.from_numpy(rng.normal(size=(Ft, D))).cuda(),
                        torch.from_numpy(rng.integers(0, C, Ft).astype(np.int32)).cuda(),
                        frame_offsets=np.arange(U * T_SONGS + 1) * FPS, item_offsets=np.arange(U + 1) * T_SONGS)
    for f in (lambda: nb.predict_proba_session(Xd, sess), lambda: xgb.predict_proba_session(Xd, sess)):
        f()
    res["epoch"] = {
        "predict_gnb": timed(lambda: nb.predict_proba_session(Xd, sess), rep),
        "predict_sgd": timed(lambda: sgd.predict_proba_session(Xd, sess), rep),
        "predict_xgb": timed(lambda: xgb.predict_proba_session(Xd, sess), rep),
        "evaluate_gnb": timed(lambda: nb.evaluate(es), rep),
        "evaluate_sgd": timed(lambda: sgd.evaluate(es), rep),
        "evaluate_xgb": timed(lambda: xgb.evaluate(es), rep),
        "retrain_gnb": timed(lambda: nb.partial_fit(Xd, rows_d, labels_d, off_d), rep),
        "retrain_sgd": timed(lambda: sgd.partial_fit(Xd, rows_d, labels_d, off_d), rep),
        "retrain_xgb": res["fit_tail"],
    }
    tot = sum(v["ms_median"] for v in res["epoch"].values())
    res["epoch"]["xgb_refit_share"] = res["fit_tail"]["ms_median"] / tot
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
    print(json.dumps({k: res[k] for k in ("fit_base", "fit_tail", "row_steps_per_s")}))


if __name__ == "__main__":
    main()
