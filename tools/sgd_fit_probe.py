"""The SGDClassifier partial_fit workloads of profiles/sgd_partial_fit.json: the
retrain step of one epoch (amg_test.py:509) for the 'classifier_sgd' member of
every user of a batched session in one launch, against the host loop it
replaces.

  python tools/sgd_fit_probe.py [out.json]
      batched   U = 500 users x 10 picked songs x 40 frames x 260 features, C = 4:
                one ops.sgd_partial_fit over all users (device time of a graph
                replay), the dependent f64 adds of one problem's chain
                (rows x D, the floor of a wave's time) and the loop of 500
                sklearn partial_fit calls on the same batches (host wall time)
      one_user  the same for U = 1 (one workgroup of 4 waves)
  python tools/sgd_fit_probe.py pmc batched|one_user
      5 eager updates of that variant and nothing else: the program to run
      under rocprofv3 --pmc (FETCH_SIZE; the SQ counters), reduced with
      tools/pmc_reduce.py into profiles/sgd_partial_fit_pmc_<variant>.json
Every user picks 10 of their 20 songs (40 contiguous frame rows each) of one
X [U * 800, 260]: the GaussianNB probe's shape.  The models are updated in
place call after call.
"""
import json
import os
import sys
import time
import warnings

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "consensus-entropy_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ce_amd  # noqa: E402
import ce_amd.ops as ops  # noqa: E402

U, SONGS, PICKED, FPS, D, C = 500, 20, 10, 40, 260, 4
ALPHA = 1e-4


def device_us(fn, n_win=10, per=10):
    """Device time per call: `per` calls captured in one HIP graph, the replay
    timed with device events; eager calls next to it as eager_us_median."""
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


def sklearn_ms(X, rows, labels, ro, coef, intercept, users):
    """Wall time of `users` SGDClassifier.partial_fit calls on the host (models built from the same state)."""
    try:
        from sklearn.linear_model import SGDClassifier
    except ImportError:
        return None
    warnings.simplefilter("ignore")
    models = []
    for u in range(users):
        m = SGDClassifier(loss="log_loss", penalty="l2", alpha=ALPHA, random_state=u, warm_start=True)
        m.partial_fit(X[:C], np.arange(C), classes=np.arange(C))  # sklearn's own set-up of a fitted model
        m.coef_[:], m.intercept_[:] = coef[u], intercept[u]
        models.append(m)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        for u, m in enumerate(models):
            r = rows[ro[u]:ro[u + 1]]
            m.partial_fit(X[r], labels[ro[u]:ro[u + 1]])  # X_batch gathered on the host, as :491 does
        dt = (time.perf_counter() - t0) * 1e3
        best = dt if best is None else min(best, dt)
    return best


def main(out_path, pmc=None):
    ce_amd.load()
    rng = np.random.default_rng(1987)
    F = U * SONGS * FPS
    X = rng.normal(0, 1, (F, D))
    coef, intercept = rng.normal(0, 0.1, (U, C, D)), rng.normal(0, 0.1, (U, C))
    song_labels = rng.integers(0, C, U * SONGS)
    songs = np.stack([np.sort(rng.choice(SONGS, PICKED, replace=False)) for _ in range(U)])
    f_off = torch.arange(U * SONGS + 1, dtype=torch.int64, device="cuda") * FPS
    item_off = torch.arange(U + 1, dtype=torch.int64, device="cuda") * SONGS
    rows, labels, ro = ops.batch_rows(torch.from_numpy(songs).cuda(), f_off, None, torch.from_numpy(song_labels).cuda(),
                                      item_offsets=item_off)
    Xd = torch.from_numpy(X).cuda()
    res = {"command": "python tools/sgd_fit_probe.py profiles/sgd_partial_fit.json",
           "shape": {"users": U, "songs_picked": PICKED, "frames_per_song": FPS, "D": D, "C": C,
                     "rows_per_user": PICKED * FPS, "alpha": ALPHA}, "rows": []}
    rows_h, labels_h, ro_h = rows.cpu().numpy(), labels.cpu().numpy(), ro.cpu().numpy()
    for name, users in (("batched", U), ("one_user", 1)):
        m = ce_amd.DeviceSGDClassifier(coef[:users], intercept[:users], np.full(users, 1000.0), alpha=ALPHA,
                                       random_state=list(range(users)))
        r, lab, o = rows[:int(ro_h[users])], labels[:int(ro_h[users])], ro[:users + 1].contiguous()
        if pmc is not None:  # the counter run: this variant's kernel alone
            if pmc == name:
                for _ in range(5):
                    m.partial_fit(Xd, r, lab, o)
                torch.cuda.synchronize()
            continue
        t = device_us(lambda: m.partial_fit(Xd, r, lab, o))
        m.check_finite()
        chain = PICKED * FPS * D
        row = {"variant": name, "users": users, **t, "waves": users * C, "chain_adds_per_wave": chain,
               "ns_per_chain_add": t["us_median"] * 1e3 / chain,
               "bytes_read_once": users * PICKED * FPS * D * 8,
               "note": "chain_adds_per_wave = rows x D dependent f64 adds, the serial part of one binary problem; "
                       "ns_per_chain_add is the launch's time over it (every wave runs its chain at once when the "
                       "waves fit the machine: 1024 SIMDs)",
               "sklearn_loop_ms": sklearn_ms(X, rows_h, labels_h, ro_h, coef, intercept, users)}
        if row["sklearn_loop_ms"] is not None:
            row["sklearn_over_device"] = row["sklearn_loop_ms"] * 1e3 / t["us_median"]
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
