"""The short-chunk CNN member at the reference's size: 64 users x 136 excerpts
of 59049 samples, nc = 128, shared weights (Uw = 1) and own weights (Uw = U).

  python tools/cnn_member_probe.py run OUT.json
      wall-clock device time (events, median of 3 after a warm-up) of the front
      end alone and of a whole predict_proba_users pass, both forms; and the
      parity ratios |dev - f64| / e32 of the cases of tests/test_gpu_cnn.py
      (tests/cnn_ref.py) and of the front-end edges of
      tests/test_gpu_cnn_edges.py (tests/cnn_exact.py), from which the tests' K
      is set
  python tools/cnn_member_probe.py parity OUT.json
      the parity ratios alone (OUT.json's other entries stay)
  python tools/cnn_member_probe.py torch OUT.json
      on the same box and data: torch.nn.functional float32 forward of the same
      network (tests/cnn_ref.forward, shared weights), median of 3
  python tools/cnn_member_probe.py trace
      one plain pass of either form and nothing else: the program to run under
      rocprofv3 --kernel-trace --output-format csv -d DIR -o run
  python tools/cnn_member_probe.py summarize DIR OUT.json
      per-kernel device time from DIR/**/run_kernel_trace.csv: front end, block
      1, blocks 2-7 one by one, head; the conv kernel's TF/s against the
      157.3 TF/s f32-MFMA peak and the 122 TF/s of an untuned LDS-tiled f32-MFMA
      GEMM
"""
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "consensus-entropy_amd"), os.path.join(ROOT, "tests")]
import torch  # noqa: E402

USERS, PER_USER, L, NC, BATCH, REPS = 64, 136, 59049, 128, 272, 3
PEAK_TFS, GUIDE_GEMM_TFS = 157.3, 122.0
CH = (0, 1, 1, 2, 2, 2, 2, 4)


def conv_flops(T, nc, block):
    """FLOPs of block `block` (2 .. 7) for one excerpt: 2 H W 9 Cin Cout at its input size."""
    H, W = 128 >> (block - 1), T
    for _ in range(block - 1):
        W //= 2
    return 2 * H * W * 9 * CH[block - 1] * nc * CH[block] * nc


def setup(own):
    import ce_amd
    import cnn_ref as R

    ce_amd.load()
    state = R.random_state(NC, seed=1)
    member = ce_amd.DeviceShortChunkCNN(state, U=USERS)
    if own:
        for u in range(USERS):
            member.set_model(u, state)
    g = torch.Generator(device="cuda").manual_seed(1)
    wave = 0.1 * torch.randn((USERS * PER_USER, L), generator=g, device="cuda", dtype=torch.float32)
    items = torch.arange(0, USERS * PER_USER + 1, PER_USER, dtype=torch.int64, device="cuda")
    return R, state, member, wave, items


def timed(fn, reps=REPS):
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return {"ms_median": statistics.median(ms), "ms_all": ms}


def load(path):
    return json.load(open(path)) if os.path.exists(path) else {}


def save(path, d):
    with open(path, "w") as f:
        json.dump(d, f, indent=1)
        f.write("\n")


def parity(R):
    """The tests' cases on this device: |dev - f64| / e32 for every one."""
    import ce_amd

    rows = []

    def row(kind, case, got, f64, f32, floor):
        r, err, e32 = R.ratio(got, f64, f32)
        rows.append({"kind": kind, "case": case, "abs_err": err, "e32": e32, "floor": floor, "ratio": r})

    for nc, S, T in R.BODY_CASES:
        state, mel, f64, f32 = R.body_case(nc, S, T)
        got = ce_amd.DeviceShortChunkCNN(state).predict_proba(mel=mel.cuda()).cpu().numpy()
        row("body", {"nc": nc, "S": S, "T": T}, got, f64, f32, R.FLOOR_P)
    for length in R.FRONT_CASES:
        state, wave, f64, f32 = R.front_case(length)
        got = ce_amd.DeviceShortChunkCNN(state).logmel(wave.cuda()).cpu().numpy()
        row("front_end_dB", {"L": length, "S": 3}, got, f64, f32, R.floor_db(f64))
    import numpy as np

    import cnn_exact as X

    for name in X.FRONT_EDGES:  # the edge inputs of tests/test_gpu_cnn_edges.py, over the HTK bank
        fb, wave, f64, f32 = X.front_edge(name)
        got = ce_amd.DeviceShortChunkCNN(X.exact_state(16, seed=0)).logmel(wave.cuda()).cpu().numpy()
        fin = np.isfinite(f64)  # the "nan" case: the entries off the NaN frames
        row("front_end_edge_dB", {"case": name, "L": int(wave.shape[1]), "S": 3}, got[fin], f64[fin], f32[fin],
            R.floor_db(f64[fin]))
    nc, S, length = R.E2E_CASE
    state, wave, f64, f32 = R.e2e_case(nc, S, length)
    got = ce_amd.DeviceShortChunkCNN(state).predict_proba(wave.cuda()).cpu().numpy()
    row("end_to_end", {"nc": nc, "S": S, "L": length}, got, f64, f32, R.FLOOR_P)
    return rows


def run(out):
    d = load(out)
    d["command"] = "python tools/cnn_member_probe.py run|torch|summarize (see the tool's docstring)"
    d["shape"] = {"users": USERS, "excerpts_per_user": PER_USER, "L": L, "T": L // 256 + 1, "nc": NC, "batch": BATCH,
                  "reps": REPS}
    d["device"] = torch.cuda.get_device_name(0)
    T = L // 256 + 1
    flops = sum(conv_flops(T, NC, b) for b in range(2, 8)) * USERS * PER_USER
    d["conv_flops_per_pass"] = flops
    for own in (False, True):
        R, _, member, wave, items = setup(own)
        key = "own_weights" if own else "shared_weights"
        if not own:
            d["parity"] = parity(R)
            d["front_end_only"] = timed(lambda: [member.logmel(wave[b:b + BATCH]) for b in range(0, wave.shape[0], BATCH)])
        r = timed(lambda: member.predict_proba_users(wave, items, batch=BATCH))
        r["Uw"] = member.Uw
        r["conv_tfs_if_all_time_were_conv"] = flops / (r["ms_median"] * 1e-3) / 1e12
        d[key] = r
        save(out, d)
        del member, wave
        torch.cuda.empty_cache()
    print(json.dumps({k: d[k] for k in ("shared_weights", "own_weights", "front_end_only")}))


def run_parity(out):
    import cnn_ref as R

    d = load(out)
    d["parity"] = parity(R)
    save(out, d)
    print(json.dumps([{**r["case"], "kind": r["kind"], "ratio": round(r["ratio"], 3)} for r in d["parity"]]))


def run_torch(out):
    d = load(out)
    R, state, _, wave, _ = setup(False)
    st = {k: v.cuda() for k, v in R.cast(state, torch.float32).items()}

    def fwd():
        with torch.no_grad():
            for b in range(0, wave.shape[0], BATCH):
                R.forward(wave[b:b + BATCH], st)

    r = timed(fwd)
    r["what"] = "torch.nn.functional float32 forward of the same network (tests/cnn_ref.forward), shared weights, " \
                f"{BATCH} excerpts per call, torch {torch.__version__}"
    d["torch_functional_fp32"] = r
    save(out, d)
    print(json.dumps(r))


def trace():
    for own in (False, True):
        _, _, member, wave, items = setup(own)
        member.predict_proba_users(wave, items, batch=BATCH)
        torch.cuda.synchronize()
        del member, wave
        torch.cuda.empty_cache()


def summarize(tdir, out):
    d = load(out)
    path = glob.glob(os.path.join(tdir, "**", "run_kernel_trace.csv"), recursive=True)[0]
    rows = [r for r in csv.DictReader(open(path)) if "k_cnn_" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    T = L // 256 + 1
    n_batches = (USERS * PER_USER + BATCH - 1) // BATCH
    per_pass = n_batches * 9
    assert len(rows) == 2 * per_pass, (len(rows), per_pass)
    for form, chunk in (("shared_weights", rows[:per_pass]), ("own_weights", rows[per_pass:])):
        ns = {}
        for i, r in enumerate(chunk):
            pos = i % 9
            name = ("front_end", "block1", *[f"block{b}" for b in range(2, 8)], "head")[pos]
            want = "k_cnn_logmel" if pos == 0 else "k_cnn_block1" if pos == 1 else "k_cnn_head" if pos == 8 else "k_cnn_conv"
            assert want in r["Kernel_Name"], (i, r["Kernel_Name"])
            ns[name] = ns.get(name, 0) + int(r["End_Timestamp"]) - int(r["Start_Timestamp"])
        k = {name: {"ms_per_pass": v * 1e-6} for name, v in ns.items()}
        conv_ns = 0
        for b in range(2, 8):
            fl = conv_flops(T, NC, b) * USERS * PER_USER
            k[f"block{b}"]["tfs"] = fl / ns[f"block{b}"] / 1e3
            conv_ns += ns[f"block{b}"]
        tfs = d["conv_flops_per_pass"] / conv_ns / 1e3
        d.setdefault(form, {})["kernels"] = k
        d[form]["conv_kernel"] = {"ms_per_pass": conv_ns * 1e-6, "tfs": tfs, "of_f32_mfma_peak_157.3": tfs / PEAK_TFS,
                                  "of_untuned_gemm_122": tfs / GUIDE_GEMM_TFS}
        d[form]["kernel_time_source"] = "rocprofv3 --kernel-trace, one pass, sum of the dispatches' End - Start"
    save(out, d)
    print(json.dumps({f: d[f]["conv_kernel"] for f in ("shared_weights", "own_weights")}))


if __name__ == "__main__":
    mode = sys.argv[1]
    if mode == "run":
        run(sys.argv[2])
    elif mode == "parity":
        run_parity(sys.argv[2])
    elif mode == "torch":
        run_torch(sys.argv[2])
    elif mode == "trace":
        trace()
    elif mode == "summarize":
        summarize(sys.argv[2], sys.argv[3])
    else:
        raise SystemExit(__doc__)
