"""Where one launch of the streaming selection kernel (k_stream_nmc, item-major
[N,16,4] f32, q = 10: the bench kernel) spends its time, from the diagnostic
build's per-wave stamps (make -C consensus-entropy_amd stamps; run with
CE_AMD_LIB=tools/_diag/libce_amd_stamps.so, or ..._stamps_static.so for the static
grid-cyclic tile order):
  ramp            first to last wave's first DMA issue
  landed          each wave's last tile landed, from the first wave's first issue
  block_merge     a block's last tile landed -> its list written
  fold            the last block: its list written -> the fold's end
  window          lowest to highest tile index in flight over the waves at a few
                  instants, interpolated from each wave's {stamp, tile} samples;
                  a sweep in step spans one tile per wave (W), the excess is drift
Stamps are wall-clock (100 MHz: 10 ns).  One JSON line per pool size.
  python tools/stream_phase_probe.py [--permille S] [--min-rounds R] [n_items ...]
--permille / --min-rounds override the build's claimed share and size gate
(ce_debug_stream_claims); each line reports the launcher's claim_from."""
import ctypes
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-entropy_amd"))
sys.path.insert(0, ROOT)
import ce_amd  # noqa: E402
from bench import make_pool  # noqa: E402
from ce_amd import ops  # noqa: E402

L = ce_amd._lib.load()
SAMPLES = 12


def stamps(waves):
    cols = L.ce_debug_stream_stamp_cols()
    assert cols == 6 + 2 * SAMPLES, cols
    buf = np.zeros((waves, cols), np.uint64)
    assert L.ce_debug_stream_stamps(buf.ctypes.data_as(ctypes.c_void_p), waves) == 0
    return buf.astype(np.int64)


def pct(x):
    return [float(v) for v in np.percentile(x, [0, 50, 99, 100])]


def reduce(b, n_items):
    W = b.shape[0]
    t0 = int(b[:, 0].min())
    us = lambda x: (np.asarray(x, np.float64) - t0) / 100.0  # noqa: E731
    first, landed, merged, folded = us(b[:, 0]), us(b[:, 1]), us(b[:, 2]), us(b[:, 3])
    tiles = b[:, 4]
    blk_landed = landed.reshape(-1, 4).max(1)
    blk_merged = merged.reshape(-1, 4).max(1)
    last = int(folded.reshape(-1, 4).max(1).argmax())
    med = float(np.median(landed))
    out = {
        "n_items": n_items, "waves": W, "tiles_per_wave": pct(tiles),
        "ramp_us": float(first.max()),
        "landed_us": dict(zip(("min", "median", "p99", "max"), pct(landed))),
        "landed_spread_us": float(landed.max() - landed.min()),
        "block_merge_us": dict(zip(("min", "median", "p99", "max"), pct(blk_merged - blk_landed))),
        "last_block": {"block": last, "landed_us": float(blk_landed[last]), "merged_us": float(blk_merged[last]),
                       "fold_us": float(folded.max() - blk_merged[last])},
        "end_us": float(folded.max()),
        "tail_after_median_landed_us": float(folded.max() - med),
        "us_per_tile_per_wave": med / float(np.median(tiles)),
    }
    win = []
    for f in (0.1, 0.25, 0.5, 0.75, 0.9):
        T = f * med
        pos = []
        for r in b:
            n = int(r[5])
            if n < 2:
                continue
            ts, tl = us(r[6:6 + 2 * n:2]), r[7:7 + 2 * n:2].astype(np.float64)
            if ts[0] <= T <= ts[-1]:
                pos.append(np.interp(T, ts, tl))
        if len(pos) > W // 2:
            span = float(max(pos) - min(pos))
            win.append({"at": f, "waves": len(pos), "window_tiles": span, "window_over_W": span / W,
                        "drift_us": (span / W - 1.0) * out["us_per_tile_per_wave"]})
    out["window"] = win
    return out


def main():
    import argparse

    ap = argparse.ArgumentParser()
    ap.add_argument("--permille", type=int, default=-1)
    ap.add_argument("--min-rounds", type=int, default=-1)
    ap.add_argument("sizes", type=int, nargs="*")
    args = ap.parse_args()
    L.ce_debug_stream_claims.argtypes = [ctypes.c_int64, ctypes.c_int64]
    L.ce_debug_stream_claims.restype = None
    L.ce_debug_stream_claim_from.restype = ctypes.c_int64
    L.ce_debug_stream_claims(args.permille, args.min_rounds)
    sizes = args.sizes or [100_000_000, 25_000_000, 12_500_000]
    dev = torch.device("cuda", 0)
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    for n in sizes:
        P = make_pool(0, n, 16, 4, dev)
        plan = ops.MCPlan(P, 10, "NMC")
        for _ in range(3):
            plan.step()
        torch.cuda.synchronize()
        kern = L.ce_last_kernel().decode()
        assert kern.startswith("ce::k_stream_nmc<0, 4, 16, 2, false, 2>"), kern
        waves = 4 * min(cus, (n + 63) // 64)  # one block per CU (two 16-KiB ring slots per wave)
        out = reduce(stamps(waves), n)
        out["kernel"] = kern
        out["lib"] = os.path.basename(os.environ.get("CE_AMD_LIB", "libce_amd.so"))
        out["claim_from"] = L.ce_debug_stream_claim_from()
        print(json.dumps(out), flush=True)
        del plan, P
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
