"""The batched XGBoost member of profiles/xgb_users.json: the predict step of
one epoch (amg_test.py:435) after one refit -- every user's forest is the shared
base plus that user's own tail -- in one launch for all users, against the
per-user launches it replaces and against one one-forest launch over the same
rows, and the evaluate step (amg_test.py:513-515).

  python tools/xgb_users_probe.py [out.json]
      the members probe's pool plus one refit: U = 500 users x 20 songs x 40
      frames, X [400000, 260] f64, C = 4, depth 5, a base of 100 rounds and a
      tail of 100 rounds per user (800 trees per user; the packed node / leaf
      arrays are seeded random values made on the device: parity is the tests'
      business).  Device time per call from graph replays, the windows of the
      variants alternating in one run:
        a           the batched launch (ce_xgb_predict_proba_users), grouped rows
        a_shuffled  the same through a random frame_perm
        b           the one-forest interface at its cheapest: U launches of
                    ce_xgb_predict_proba_lanes, each with that user's 800-tree
                    table over its contiguous 800-row slice
        c           ONE one-forest launch of an 800-tree forest over all rows:
                    the floor of a
        d           a with half of every user's songs excluded
        e           the evaluate over 500 x 3 x 40 test frames: memset + score + F1
      and the ratios a/b, a/c, d/a with the fraction of 8 TB/s that a reaches
      on F * D * 8 bytes.
  python tools/xgb_users_probe.py pmc
      5 eager batched launches (a), then 5 one-forest launches over all rows
      (c), and nothing else: the program to run under rocprofv3 --pmc (one run
      per counter set, no tracing options).
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
from ce_amd._lib import CE_F32, CE_F64, call  # noqa: E402

U, SONGS, FPS, D, C, G, DEPTH = 500, 20, 40, 260, 4, 4, 5
ROUNDS, T_SONGS = 100, 3  # rounds of the base and of every tail; test songs per user
HBM_BYTES_PER_S = 8e12
DEV = torch.device("cuda", 0)


def graph_of(fn, per):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(per):
            fn()
    return g


def alternating_us(variants, n_win=10):
    """Device time per call of every variant {name: (fn, calls per graph)}: one
    graph each, the windows alternating over the variants in one run."""
    graphs = {k: (graph_of(fn, per), per) for k, (fn, per) in variants.items()}
    times = {k: [] for k in variants}
    for _ in range(n_win):
        for k, (g, per) in graphs.items():
            torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            g.replay()
            b.record()
            b.synchronize()
            times[k].append(a.elapsed_time(b) * 1e3 / per)
    return {k: {"us_min": min(t), "us_median": float(np.median(t)), "us_max": max(t), "windows": n_win,
                "calls_per_window": graphs[k][1]} for k, t in times.items()}


def main(out_path, pmc=False):
    ce_amd.load()
    torch.manual_seed(1987)
    rng = np.random.default_rng(1987)
    F, T, RPU = U * SONGS * FPS, U * SONGS, SONGS * FPS
    NI, PER = (1 << DEPTH) - 1, ROUNDS * G  # inner nodes per tree; trees per forest part
    TT = PER * (1 + U)
    p, st = ops._p, ops._stream(DEV)
    Xd = torch.from_numpy(rng.normal(0, 1, (F, D))).cuda()
    # the packed arrays, random: {feature | default_left << 31, threshold bits}, leaves
    feat = torch.randint(0, D, (TT, NI), device="cuda", dtype=torch.int32)
    feat |= torch.randint(0, 2, (TT, NI), device="cuda", dtype=torch.int32) << 31
    nodes = torch.stack([feat, torch.randn((TT, NI), device="cuda").view(torch.int32)], 2).contiguous()
    leaves = (torch.randn((TT, NI + 1), device="cuda") * 0.1).contiguous()
    table = torch.empty((2, TT, 64, 2), dtype=torch.int32, device="cuda")
    call("ce_xgb_lane_table", p(nodes), p(leaves), TT, DEPTH, D, p(table), st)
    del nodes, leaves, feat
    # user u's group g: the base's trees of group g, then the user's own (both group-major)
    r = np.arange(ROUNDS)
    ids = np.stack([[np.concatenate([g * ROUNDS + r, PER * (1 + u) + g * ROUNDS + r]) for g in range(G)]
                    for u in range(U)]).astype(np.int32)  # [U, G, 2 ROUNDS]
    tree_ids = torch.from_numpy(ids.reshape(-1)).cuda()
    goff = torch.arange(U * G + 1, dtype=torch.int32, device="cuda") * (2 * ROUNDS)
    f_off = torch.arange(T + 1, dtype=torch.int64, device="cuda") * FPS
    item_off = torch.arange(U + 1, dtype=torch.int64, device="cuda") * SONGS
    perm = torch.from_numpy(rng.permutation(F)).cuda()
    half = ops.excl_bitmap(T, "cuda")
    half.fill_(0x55555555)  # every other song of every user
    out = torch.zeros((F, C), dtype=torch.float32, device="cuda")

    def users(frame_perm=None, excl=None):
        args = ("ce_xgb_predict_proba_users", p(Xd), CE_F64, F, D, D, p(table), TT, p(tree_ids), tree_ids.numel(),
                p(goff), G, DEPTH, 0.5, C, U, p(item_off), p(f_off), p(frame_perm), p(excl), p(out), CE_F32, C)
        return lambda: call(*args, ops._stream(DEV))

    # the one-forest tables: user u's 800 trees, group-major
    one_goff = torch.arange(G + 1, dtype=torch.int32, device="cuda") * (2 * ROUNDS)

    def one_forest(u, lo, n):
        tab = table[:, torch.from_numpy(ids[u].reshape(-1).astype(np.int64)).cuda()].contiguous()
        xs, os_ = Xd[lo:lo + n], out[lo:lo + n]
        args = ("ce_xgb_predict_proba_lanes", p(xs), CE_F64, n, D, D, p(tab), tab.shape[1], p(one_goff), G, DEPTH, 0.5,
                C, p(os_), CE_F32, C)
        return lambda tab=tab: call(*args, ops._stream(DEV))  # the table lives as long as the closure

    floor = one_forest(0, 0, F)
    if pmc:
        for fn in (users(), floor):
            for _ in range(5):
                fn()
        torch.cuda.synchronize()
        return
    per_user = [one_forest(u, u * RPU, RPU) for u in range(U)]

    def loop():
        for f in per_user:
            f()

    # the evaluate step: every user's 3 test songs x 40 frames
    Ft = U * T_SONGS * FPS
    Xt = torch.from_numpy(rng.normal(0, 1, (Ft, D))).cuda()
    yt = torch.from_numpy(rng.integers(0, C, Ft).astype(np.int32)).cuda()
    t_off = torch.arange(U * T_SONGS + 1, dtype=torch.int64, device="cuda") * FPS
    t_items = torch.arange(U + 1, dtype=torch.int64, device="cuda") * T_SONGS
    cm = torch.empty((U, C, C), dtype=torch.int64, device="cuda")
    f1 = torch.empty(U, dtype=torch.float64, device="cuda")

    def evaluate():
        s = ops._stream(DEV)
        call("ce_xgb_score_users", p(Xt), CE_F64, Ft, D, D, p(table), TT, p(tree_ids), tree_ids.numel(), p(goff), G,
             DEPTH, 0.5, C, U, p(t_items), p(t_off), None, None, p(yt), p(cm), None, None, C, s)
        call("ce_f1_weighted_users", p(cm), U, C, p(f1), None, s)

    lines = alternating_us({"a": (users(), 10), "a_shuffled": (users(frame_perm=perm), 10), "b": (loop, 2),
                            "c": (floor, 10), "d": (users(excl=half), 10), "e": (evaluate, 10)})
    a = lines["a"]["us_median"]
    ideal = F * D * 8 / HBM_BYTES_PER_S * 1e6
    res = {"command": "python tools/xgb_users_probe.py profiles/xgb_users.json",
           "shape": {"users": U, "songs_per_user": SONGS, "frames_per_song": FPS, "F": F, "D": D, "C": C, "depth": DEPTH,
                     "base_rounds": ROUNDS, "tail_rounds": ROUNDS, "trees_per_user": 2 * PER, "table_trees": TT,
                     "table_bytes": int(table.numel()) * 4, "test_frames": Ft},
           "bytes_of_X": F * D * 8, "ideal_us_at_8TBps": ideal, **lines,
           "a_over_b": a / lines["b"]["us_median"], "a_over_c": a / lines["c"]["us_median"],
           "d_over_a": lines["d"]["us_median"] / a, "a_fraction_of_8TBps": ideal / a,
           "a_slowest_window_below_b_fastest": lines["a"]["us_max"] < lines["b"]["us_min"],
           "launches": {"a": 1, "b": U, "c": 1, "d": 1, "e": "memset + 2"}}
    print(json.dumps(res), flush=True)
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "pmc":
        main(None, pmc=True)
    else:
        main(sys.argv[1] if len(sys.argv) > 1 else None)
