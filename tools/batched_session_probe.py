"""The batched-session workload of profiles/r07_batched_session.json: 500 users
x (1608 committee items, M = 4, f32) + 1608 hc rows each, q = 10, 30 % of
either pool excluded.

  python tools/batched_session_probe.py time [out.json]
      device-event times: one mix epoch (select + mark) as a HIP-graph replay;
      the same work as a loop of 500 SelectionSession("mix").select calls
  python tools/batched_session_probe.py reduce <prof dir> <time.json> <out.json>
      the kernel traces under <prof dir>/<config>_<rep> and the time JSON -> one JSON
  python tools/batched_session_probe.py mixcold|mccold|mccold_excl [reps]
      plain launches for a rocprofv3 --kernel-trace --stats run of its own,
      rotating 8 distinct 51.5 MB committee pools (412 MB > the 256 MiB
      Infinity Cache, as tools/small_probe.py c3cold): the mix epoch; the
      batched mc without / with a 30 % bitmap
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
from tools.bench_configs import dirichlet  # noqa: E402

U, NU, Q, EXCLUDED = 500, 1608, 10, 0.3


def bitmap(n, g):
    bits = (torch.rand(n + (-n % 32), device="cuda", generator=g) < EXCLUDED).view(-1, 32).to(torch.int64)
    words = (bits << torch.arange(32, device="cuda")).sum(1)
    return torch.where(words >= 2**31, words - 2**32, words).to(torch.int32).contiguous()


def setup(g, pools=1):
    offs = torch.arange(0, U + 1, device="cuda", dtype=torch.int64) * NU
    P = [dirichlet((4, U * NU, 4), torch.float32, g) for _ in range(pools)]
    hc = torch.round(dirichlet((U * NU, 4), torch.float64, g) * 1000) / 1000
    return offs, P, hc, bitmap(U * NU, g), bitmap(U * NU, g)


def probe(cfg, reps):
    g = torch.Generator(device="cuda").manual_seed(1987)
    offs, pools, hc, ex, exh = setup(g, 8)
    ex0, exh0 = ex.clone(), exh.clone()
    for it in range(reps):
        P = pools[it % len(pools)]
        if cfg == "mixcold":  # one epoch: select + mark (the bitmaps restored so every epoch sees 30 %)
            ex.copy_(ex0)
            exh.copy_(exh0)
            _, idx = ops.select_batched_mix(P, offs, hc, offs, Q, "MNC", excl=ex, excl_h=exh)
            ops.mark_selected_batched(idx, offs, ex, offs, exh)
        elif cfg == "mccold":
            ops.select_batched(P, offs, Q, "MNC")
        elif cfg == "mccold_excl":
            ops.select_batched(P, offs, Q, "MNC", excl=ex)
        else:
            raise SystemExit(f"unknown config {cfg}")
    torch.cuda.synchronize()
    print("ok", cfg, reps, ce_amd._lib.load().ce_last_kernel().decode())


def events(fn, windows, per):
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / per)
    return {"us_min": min(out), "us_median": float(np.median(out)), "us_max": max(out), "windows": windows,
            "per_window": per}


def timed(out_path):
    g = torch.Generator(device="cuda").manual_seed(1987)
    offs, (P,), hc, ex, exh = setup(g)
    off_h = np.arange(U + 1) * NU
    sess = ce_amd.BatchedSelectionSession(Q, "mix", off_h, hc=hc)
    ex0, exh0 = ex.clone(), exh.clone()
    sess.excl.copy_(ex0)
    sess.excl_h.copy_(exh0)
    ops.select_mc(P[:, :NU], Q, "MNC")  # creates the graph arena
    ops.reserve_graph_workspace(ce_amd._lib.load().ce_select_batched_mix_workspace_bytes(U * NU, U * NU, U, Q))
    torch.cuda.synchronize()
    gr = torch.cuda.CUDAGraph()
    with torch.cuda.graph(gr):
        idx = sess.step(P)
    kernel = ce_amd._lib.load().ce_last_kernel().decode()

    def replay():
        gr.replay()

    def restore():  # 10 replays mark 100 of a user's ~1125 remaining songs: restore between windows
        sess.excl.copy_(ex0)
        sess.excl_h.copy_(exh0)

    res = {"kernel": kernel, "shape": {"users": U, "items_per_user": NU, "hc_rows_per_user": NU, "M": 4,
                                       "dtype": "float32", "q": Q, "excluded": EXCLUDED}}
    for _ in range(3):
        restore()
        for _ in range(10):
            replay()
    win = []
    for _ in range(30):
        restore()
        torch.cuda.synchronize()
        win.append(events(replay, 1, 10)["us_median"])
    res["graph_replay_mix_epoch_us"] = {"us_min": min(win), "us_median": float(np.median(win)), "us_max": max(win),
                                        "windows": 30, "replays_per_window": 10,
                                        "what": "select + mark, committee resident in the Infinity Cache"}
    picks = idx.cpu().numpy()
    # the parent's way: one SelectionSession per user, a Python loop per epoch
    Hn = hc.cpu().numpy()
    singles = [ce_amd.SelectionSession(Q, "mix", NU, hc=Hn[u * NU:(u + 1) * NU]) for u in range(U)]
    for s in singles:  # 30 % of either pool out, as in the batch
        s.excl.copy_(bitmap(NU, g))
        s.excl_hc.copy_(bitmap(NU, g))
    views = [P[:, u * NU:(u + 1) * NU] for u in range(U)]

    def loop():
        return [s.select(committee=v) for s, v in zip(singles, views)]

    loop()  # warm-up epoch
    import time

    t = []
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        loop()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) * 1e6)
    res["loop_of_500_sessions_epoch_us"] = {"us_min": min(t), "us_median": float(np.median(t)), "us_max": max(t),
                                            "epochs": 3, "what": "500 x SelectionSession('mix').select, host clock "
                                            "around the loop ending in a device synchronise"}
    res["last_replay_picks_user0"] = picks[0].tolist()
    print(json.dumps(res))
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


def reduce(prof, time_json, out):
    """Per config and repetition: every ce:: kernel's device time over the calls (the first 8 dropped: warm-up)."""
    import csv
    import glob

    def kernel_rows(path):  # the engine's kernels: ce::* and the marks
        rows = {}
        for r in csv.DictReader(open(path)):
            name = (r["Kernel_Name"] if "Kernel_Name" in r else r["Name"]).split("(")[0].replace("void ", "")
            if "ce::" in name or name.startswith("k_mark"):
                rows.setdefault(name, []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
        return rows

    res = {"what": "MI355X, one GPU.  kernel_us: device us per kernel call from rocprofv3 kernel traces of plain "
                   "launches rotating 8 committee pools (412 MB > the 256 MiB Infinity Cache: HBM-cold), 60 calls, "
                   "the first 8 dropped, <config>_<repetition>; time: the profiler off",
           "command": "for rep in 1 2; for c in c3cold mixcold mccold mccold_excl: rocprofv3 --kernel-trace --stats "
                      "-d prof/${c}_$rep -o run --output-format csv -- python3 tools/batched_session_probe.py $c 60 "
                      "(c3cold: tools/small_probe.py c3cold 60); python3 tools/batched_session_probe.py time "
                      "time.json; python3 tools/batched_session_probe.py reduce prof time.json "
                      "profiles/r07_batched_session.json",
           "kernel_us": {}, "time": json.load(open(time_json))}
    for d in sorted(glob.glob(os.path.join(prof, "*_[0-9]"))):
        cfg = os.path.basename(d)
        tr = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
        if not tr:
            continue
        for k, v in kernel_rows(tr[0]).items():
            v = v[8:] if len(v) > 16 else v
            sv = sorted(v)
            res["kernel_us"].setdefault(cfg, {})[k[:150]] = {
                "calls": len(v), "mean": sum(v) / len(v) / 1e3, "median": sv[len(v) // 2] / 1e3, "min": sv[0] / 1e3,
                "max": sv[-1] / 1e3}
    json.dump(res, open(out, "w"), indent=1)
    for cfg, ks in res["kernel_us"].items():
        for k, v in ks.items():
            print(f"{cfg:16s} {v['median']:8.2f} us (min {v['min']:.2f}, n {v['calls']})  {k[:80]}")


if __name__ == "__main__":
    if sys.argv[1] == "reduce":
        reduce(*sys.argv[2:5])
    elif sys.argv[1] == "time":
        timed(sys.argv[2] if len(sys.argv) > 2 else None)
    else:
        probe(sys.argv[1], int(sys.argv[2]) if len(sys.argv) > 2 else 50)
