"""The batched member inference of profiles/members_users.json: the predict
step of one epoch (amg_test.py:435) for every user of a batched session in one
launch per member, against the per-user launches it replaces and against one
one-model launch over the same rows.

  python tools/members_users_probe.py [out.json]
      per member (gnb, sgd), on the fit probes' pool -- U = 500 users x 20 songs
      x 40 frames, X [400000, 260], C = 4 -- device time per call from a graph
      replay, the eager median next to it:
        a           the batched launch (ce_*_predict_proba_users), grouped rows
        a_shuffled  the same through a random frame_perm
        b           the status quo in its cheapest form: U one-model launches,
                    each over its user's contiguous 800-row slice (no gather;
                    the log-prior computed once, outside)
        c           ONE one-model launch over all 400K rows: the same bytes and
                    arithmetic with one staging -- the floor of a
        d           a with half of every user's songs excluded
      and the ratios a/b, a/c, d/a with the fraction of 8 TB/s that a reaches
      on F * D * 8 bytes.
  python tools/members_users_probe.py pmc gnb|sgd
      5 eager batched launches of that member (a), then 5 one-model launches
      over all rows (c), and nothing else: the program to run under
      rocprofv3 --pmc (one run per counter set, no tracing options), reduced
      with tools/pmc_reduce.py into profiles/members_users_pmc.json
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "consensus-entropy_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import ce_amd  # noqa: E402
import ce_amd.ops as ops  # noqa: E402
from ce_amd._lib import call  # noqa: E402

U, SONGS, FPS, D, C = 500, 20, 40, 260, 4
HBM_BYTES_PER_S = 8e12


def device_us(fn, n_win=10, per=10):
    """Device time per call: `per` calls captured in one HIP graph, the replay
    timed with device events; the eager calls' median next to it."""
    for _ in range(2):
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


def main(out_path, pmc=None):
    ce_amd.load()
    rng = np.random.default_rng(1987)
    F, T, RPU = U * SONGS * FPS, U * SONGS, SONGS * FPS
    Xd = torch.from_numpy(rng.normal(0, 1, (F, D))).cuda()
    f_off = torch.arange(T + 1, dtype=torch.int64, device="cuda") * FPS
    item_off = torch.arange(U + 1, dtype=torch.int64, device="cuda") * SONGS
    perm = torch.from_numpy(rng.permutation(F)).cuda()
    half = ops.excl_bitmap(T, "cuda")
    half.fill_(0x55555555)  # every other song of every user (20 songs per user: 10 excluded)
    out = torch.zeros((F, C), dtype=torch.float64, device="cuda")
    theta = torch.from_numpy(rng.normal(0, 1, (U, C, D))).cuda()
    var = torch.from_numpy(rng.random((U, C, D)) + 0.5).cuda()
    prior = torch.from_numpy(rng.dirichlet(np.ones(C) * 5, U)).cuda()
    log_prior = ops.log_f64(prior.reshape(-1).contiguous()).reshape(U, C)
    coef = torch.from_numpy(rng.normal(0, 0.1, (U, C, D))).cuda()
    icpt = torch.from_numpy(rng.normal(0, 0.5, (U, C))).cuda()
    p = ops._p

    def users(kind, frame_perm=None, excl=None):
        if kind == "gnb":
            return lambda: ops.gnb_predict_proba_users(Xd, theta, var, prior, item_off, f_off, frame_perm, excl, out)
        return lambda: ops.sgd_predict_proba_users(Xd, coef, icpt, item_off, f_off, frame_perm, excl, out)

    def one_model(kind, u, lo, n):
        """The one-model entry point over rows lo .. lo + n with model u (the C-ABI itself: one launch)."""
        xs, os_ = Xd[lo:lo + n], out[lo:lo + n]
        if kind == "gnb":
            args = ("ce_gnb_predict_proba", p(xs), n, D, D, p(theta[u]), p(var[u]), p(log_prior[u]), C, p(os_), C)
        else:
            args = ("ce_sgd_predict_proba", p(xs), n, D, D, p(coef[u]), p(icpt[u]), C, C, p(os_), C)
        return lambda: call(*args, ops._stream(Xd.device))  # torch's current stream: the capture stream in a graph

    if pmc is not None:
        for fn in (users(pmc), one_model(pmc, 0, 0, F)):  # a, then c: two kernels, told apart by name
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return
    res = {"command": "python tools/members_users_probe.py profiles/members_users.json",
           "shape": {"users": U, "songs_per_user": SONGS, "frames_per_song": FPS, "F": F, "D": D, "C": C},
           "bytes_of_X": F * D * 8, "ideal_us_at_8TBps": F * D * 8 / HBM_BYTES_PER_S * 1e6, "rows": []}
    for kind in ("gnb", "sgd"):
        per_user = [one_model(kind, u, u * RPU, RPU) for u in range(U)]

        def loop():
            for f in per_user:
                f()

        lines = {"a": device_us(users(kind)),
                 "a_shuffled": device_us(users(kind, frame_perm=perm)),
                 "b": device_us(loop, n_win=5, per=2),
                 "c": device_us(one_model(kind, 0, 0, F)),
                 "d": device_us(users(kind, excl=half))}
        a = lines["a"]["us_median"]
        row = {"member": kind, **{k: v for k, v in lines.items()},
               "a_over_b": a / lines["b"]["us_median"], "a_over_c": a / lines["c"]["us_median"],
               "d_over_a": lines["d"]["us_median"] / a,
               "a_fraction_of_8TBps": res["ideal_us_at_8TBps"] / a,
               "launches": {"a": 1, "b": U, "c": 1, "d": 1}}
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
