"""The GaussianNB partial_fit workloads of profiles/gnb_partial_fit.json: the
retrain step of one epoch (amg_test.py:509) for every user of a batched session
in one launch, against the host loop it replaces.

  python tools/gnb_fit_probe.py [out.json]
      batched   U = 500 users x 10 picked songs x 40 frames x 260 features, C = 4:
                one ops.gnb_partial_fit over all users (device time of a graph replay), the
                bytes it must read once (U * B * D * 8) and the fraction of
                8 TB/s that time achieves; the loop of 500 sklearn partial_fit
                calls on the same batches (host wall time)
      one_user  the same two numbers for U = 1 (one workgroup: bound by its own instruction stream)
  python tools/gnb_fit_probe.py pmc batched|one_user
      5 eager updates of that variant and nothing else: the program to run
      under rocprofv3 --pmc (FETCH_SIZE; the SQ counters), reduced with
      tools/pmc_reduce.py into profiles/gnb_partial_fit_pmc_<variant>.json
Every user picks 10 of their 20 songs (40 contiguous frame rows each) of one
X [U * 800, 260]; the models are updated in place call after call.
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

U, SONGS, PICKED, FPS, D, C = 500, 20, 10, 40, 260, 4
HBM_BYTES_PER_S = 8e12


def device_us(fn, n_win=10, per=10):
    """Device time per call: `per` calls captured in one HIP graph, the replay
    timed with device events (eager calls of a kernel this short are bound by
    the host side of the call, reported next to it as eager_us_median)."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per):
            fn()
    out, eager = [], []
    for replay in (True, False):
        for _ in range(n_win):
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            if replay:
                g.replay()
            else:
                for _ in range(per):
                    fn()
            b.record()
            b.synchronize()
            (out if replay else eager).append(a.elapsed_time(b) * 1e3 / per)
    return {"us_min": min(out), "us_median": float(np.median(out)), "us_max": max(out), "windows": n_win,
            "calls_per_window": per, "eager_us_median": float(np.median(eager))}


def sklearn_ms(X, rows, labels, ro, theta, var, cc, users):
    """Wall time of `users` GaussianNB.partial_fit calls on the host (models built from the same state)."""
    try:
        from sklearn.naive_bayes import GaussianNB
    except ImportError:
        return None
    models = []
    for u in range(users):
        g = GaussianNB()
        g.classes_ = np.arange(C)
        g.theta_, g.var_, g.class_count_ = theta[u].copy(), var[u].copy(), cc[u].copy()
        g.class_prior_ = cc[u] / cc[u].sum()
        g.n_features_in_ = D
        models.append(g)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for u, g in enumerate(models):
            r = rows[ro[u]:ro[u + 1]]
            g.partial_fit(X[r], labels[ro[u]:ro[u + 1]])  # X_batch gathered on the host, as :491 does
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def main(out_path, pmc=None):
    ce_amd.load()
    rng = np.random.default_rng(1987)
    F = U * SONGS * FPS
    X = rng.normal(0, 1, (F, D))
    theta, var = rng.normal(0, 1, (U, C, D)), rng.random((U, C, D)) + 0.5
    cc = rng.integers(20, 200, (U, C)).astype(np.float64)
    song_labels = rng.integers(0, C, U * SONGS)
    songs = np.stack([np.sort(rng.choice(SONGS, PICKED, replace=False)) for _ in range(U)])
    f_off = torch.arange(U * SONGS + 1, dtype=torch.int64, device="cuda") * FPS
    item_off = torch.arange(U + 1, dtype=torch.int64, device="cuda") * SONGS
    rows, labels, ro = ops.batch_rows(torch.from_numpy(songs).cuda(), f_off, None, torch.from_numpy(song_labels).cuda(),
                                      item_offsets=item_off)
    Xd = torch.from_numpy(X).cuda()
    res = {"command": "python tools/gnb_fit_probe.py profiles/gnb_partial_fit.json",
           "shape": {"users": U, "songs_picked": PICKED, "frames_per_song": FPS, "D": D, "C": C,
                     "rows_per_user": PICKED * FPS}, "rows": []}
    rows_h, labels_h, ro_h = rows.cpu().numpy(), labels.cpu().numpy(), ro.cpu().numpy()
    for name, users in (("batched", U), ("one_user", 1)):
        st = [torch.from_numpy(a[:users].copy()).cuda() for a in (theta, var, cc)]
        prior = torch.empty((users, C), dtype=torch.float64, device="cuda")
        eps = torch.empty(users, dtype=torch.float64, device="cuda")
        r, lab, o = rows[:int(ro_h[users])], labels[:int(ro_h[users])], ro[:users + 1].contiguous()
        if pmc is not None:  # the counter run: this variant's kernel alone
            if pmc == name:
                for _ in range(5):
                    ops.gnb_partial_fit(Xd, r, lab, *st, row_offsets=o, class_prior=prior, epsilon=eps)
                torch.cuda.synchronize()
            continue
        t = device_us(lambda: ops.gnb_partial_fit(Xd, r, lab, *st, row_offsets=o, class_prior=prior, epsilon=eps))
        nbytes = users * PICKED * FPS * D * 8
        ideal_us = nbytes / HBM_BYTES_PER_S * 1e6
        row = {"variant": name, "users": users, **t, "bytes_read_once": nbytes, "ideal_us_at_8TBps": ideal_us,
               "fraction_of_8TBps_one_read": ideal_us / t["us_median"],
               "note": "the kernel walks each batch twice (sums, then squared deviations): bytes_read_once is the "
                       "floor, not the traffic.  Counter runs (profiles/gnb_partial_fit_pmc_<variant>.json, FETCH_SIZE "
                       "x 2): batched 851 MB per launch = 2.04 x bytes_read_once -- the second walk comes from beyond "
                       "L2 again (500 batches of 832 KB in flight do not fit it), so the traffic rate is about twice "
                       "the fraction given here; one user 0.94 MB = 1.1 x -- its second walk hits L2",
               "sklearn_loop_ms": sklearn_ms(X, rows_h, labels_h, ro_h, theta, var, cc, users)}
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
