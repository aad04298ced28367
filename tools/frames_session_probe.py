"""The frames-session workloads of profiles/frames_session.json: one epoch of a
session fed with frame-level members (3 frame members + 1 song member, f64,
C = 4, 40 frames per song, q = 10), the fused path against the segment-mean
stack it replaces.

  python tools/frames_session_probe.py mc [out.json]
      one mc epoch at 1608 and 1M songs, grouped and shuffled frames:
        frames_excl   ops.select_frames(excl=) + mark                (2 launches)
        stack_excl    3 x ops.segment_mean + ops.select_mc(excl=) + mark (5 launches)
        frames_plain  ops.select_frames without a bitmap (the existing kernel; the
                      all-clear frames_excl row next to it is the bitmap's own cost)
      at 0 % / 30 % random exclusion (1608 songs), and 0 % / 30 % random / 90 %
      random / 90 % contiguous (1M songs)
  python tools/frames_session_probe.py batched [out.json]
      one batched mix epoch, 500 users x 1608 songs x 40 frames, 30 % excluded:
        frames   ops.frames_consensus + ops.select_batched_mix + mark
        stack    3 x ops.segment_mean into a stack + the same select + mark
  python tools/frames_session_probe.py plain [out.json]
      the four fused (f)1 rows on the existing kernels, no bitmap; with
      CE_AMD_LIB=<another build> the same on that build (A/B against the parent)
Device-event times, the bitmap restored before every epoch (outside the timed
window each 10 epochs: 10 marks of q songs do not change the fill level).
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

FPS, C, Q = 40, 4, 10


def pack(bits):
    """bool [n] on the device -> the engine's bitmap"""
    n = bits.numel()
    b = torch.zeros(n + (-n % 32), dtype=torch.int64, device="cuda")
    b[:n] = bits
    words = (b.view(-1, 32) << torch.arange(32, device="cuda")).sum(1)
    return torch.where(words >= 2**31, words - 2**32, words).to(torch.int32).contiguous()


def fill(kind, n, g):
    if kind == "0%":
        return torch.zeros(n, dtype=torch.bool, device="cuda")
    if kind == "90% contiguous":
        m = torch.zeros(n, dtype=torch.bool, device="cuda")
        m[n // 20:n // 20 + (9 * n) // 10] = True
        return m
    return torch.rand(n, device="cuda", generator=g) < (0.3 if kind == "30% random" else 0.9)


def windows(fn, restore, n_win, per):
    for _ in range(2):
        restore()
        for _ in range(per):
            fn()
    out = []
    for _ in range(n_win):
        restore()
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(per):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / per)
    return {"us_min": min(out), "us_median": float(np.median(out)), "us_max": max(out), "windows": n_win,
            "epochs_per_window": per}


def mc(out_path):
    g = torch.Generator(device="cuda").manual_seed(1987)
    lib = ce_amd._lib.load()
    res = {"shape": {"frames_per_song": FPS, "C": C, "q": Q, "members": "3 frame-level f64 + 1 song-level f64"},
           "rows": []}
    for songs in (1608, 1_000_000):
        F = songs * FPS
        fr = [dirichlet((F, C), torch.float64, g) for _ in range(3)]
        cnn = dirichlet((songs, C), torch.float64, g)
        offs = torch.arange(0, songs + 1, device="cuda", dtype=torch.int64) * FPS
        stack = torch.empty((4, songs, C), device="cuda", dtype=torch.float64)
        stack[3].copy_(cnn)
        sl = [False, False, False, True]
        n_win, per = (20, 10) if songs < 10_000 else (8, 5)
        fills = ("0%", "30% random") if songs < 10_000 else ("0%", "30% random", "90% random", "90% contiguous")
        for perm in (None, torch.randperm(F, device="cuda", generator=g)):
            order = "grouped" if perm is None else "shuffled"
            t = windows(lambda: ops.select_frames(fr + [cnn], offs, Q, perm=perm, song_level=sl), lambda: None,
                        n_win, per)
            res["rows"].append({"songs": songs, "order": order, "variant": "frames_plain", "excluded": "no bitmap",
                                "kernel": lib.ce_last_kernel().decode(), **t})
            print(json.dumps(res["rows"][-1]), flush=True)
            for kind in fills:
                ex0 = pack(fill(kind, songs, g))
                ex = ex0.clone()

                def frames_excl():
                    _, idx = ops.select_frames(fr + [cnn], offs, Q, perm=perm, song_level=sl, excl=ex)
                    ops.mark_selected(ex, songs, idx)
                    return idx

                def stack_excl():
                    for m in range(3):
                        ops.segment_mean(fr[m], offs, perm, out=stack[m])
                    _, idx = ops.select_mc(stack, Q, "MNC", excl=ex)
                    ops.mark_selected(ex, songs, idx)
                    return idx

                ex.copy_(ex0)
                a = frames_excl()
                ka = lib.ce_last_kernel().decode()
                ex.copy_(ex0)
                b = stack_excl()
                same = bool(torch.equal(a, b))
                for name, fn, k in (("frames_excl", frames_excl, ka), ("stack_excl", stack_excl, None)):
                    t = windows(fn, lambda: ex.copy_(ex0), n_win, per)
                    row = {"songs": songs, "order": order, "variant": name, "excluded": kind,
                           "same_picks_both_variants": same, **t}
                    if k:
                        row["kernel"] = k
                    res["rows"].append(row)
                    print(json.dumps(row), flush=True)
        del fr, stack
    dump(res, out_path)


def batched(out_path):
    g = torch.Generator(device="cuda").manual_seed(1987)
    U, NU = 500, 1608
    T, F = U * NU, U * NU * FPS
    off = np.arange(U + 1) * NU
    fr = [dirichlet((F, C), torch.float64, g) for _ in range(3)]
    cnn = dirichlet((T, C), torch.float64, g)
    hc = torch.round(dirichlet((T, C), torch.float64, g) * 1000) / 1000
    f_off = np.arange(T + 1, dtype=np.int64) * FPS
    res = {"shape": {"users": U, "songs_per_user": NU, "hc_rows_per_user": NU, "frames_per_song": FPS, "C": C,
                     "q": Q, "excluded": "30% random of either pool", "members": "3 frame-level f64 + 1 song-level f64",
                     "frames": "grouped"}, "rows": []}
    a = ce_amd.BatchedSelectionSession(Q, "mix", off, hc=hc, frame_offsets=f_off)
    b = ce_amd.BatchedSelectionSession(Q, "mix", off, hc=hc)
    ex0, exh0 = pack(fill("30% random", T, g)), pack(fill("30% random", T, g))
    stack = torch.empty((4, T, C), device="cuda", dtype=torch.float64)
    stack[3].copy_(cnn)
    offs_d = torch.from_numpy(f_off).cuda()

    def restore():
        for s in (a, b):
            s.excl.copy_(ex0)
            s.excl_h.copy_(exh0)

    def frames():
        return a.step(frames=fr + [cnn])

    def stacked():
        for m in range(3):
            ops.segment_mean(fr[m], offs_d, None, out=stack[m])
        return b.step(stack)

    restore()
    same = bool(torch.equal(frames(), stacked()))
    for name, fn in (("frames: frames_consensus + select_batched_mix + mark", frames),
                     ("stack: 3 x segment_mean + select_batched_mix + mark", stacked)):
        t = windows(fn, restore, 8, 5)
        res["rows"].append({"variant": name, "same_picks_both_variants": same, **t})
        print(json.dumps(res["rows"][-1]), flush=True)
    dump(res, out_path)


def plain(out_path):
    """The four fused (f)1 rows of tools/bench_configs.py frames_selection_configs on the existing
    kernels alone (no bitmap): runs on any build of the library (CE_AMD_LIB), for an A/B against
    the parent commit's."""
    g = torch.Generator(device="cuda").manual_seed(1987)
    lib = ce_amd._lib.load()
    res = {"lib": os.path.basename(ce_amd._lib.LIB_PATH), "rows": []}
    for songs in (1608, 1_000_000):
        F = songs * FPS
        fr = [dirichlet((F, C), torch.float64, g) for _ in range(3)]
        cnn = dirichlet((songs, C), torch.float64, g)
        offs = torch.arange(0, songs + 1, device="cuda", dtype=torch.int64) * FPS
        n_win, per = (20, 10) if songs < 10_000 else (8, 5)
        for perm in (None, torch.randperm(F, device="cuda", generator=g)):
            t = windows(lambda: ops.select_frames(fr + [cnn], offs, Q, perm=perm), lambda: None, n_win, per)
            res["rows"].append({"songs": songs, "order": "grouped" if perm is None else "shuffled",
                                "kernel": lib.ce_last_kernel().decode(), **t})
        del fr
    print(json.dumps(res), flush=True)
    dump(res, out_path)


def dump(res, out_path):
    if out_path:
        os.makedirs(os.path.dirname(out_path) or ".", exist_ok=True)
        with open(out_path, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    {"mc": mc, "batched": batched, "plain": plain}[sys.argv[1]](sys.argv[2] if len(sys.argv) > 2 else None)
