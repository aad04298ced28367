"""GPU parity: the HIP path (through the C-ABI) against the golden fixtures and
the CPU oracle on the same seeded inputs.

Bar (BASELINE.json north_star): entropies within 1e-6 relative of the
reference's NumPy/SciPy values (fp32 load, fp64 accumulate) -- we hold them to
BIT EQUALITY (tolerance 0): every sum is in numpy's order and the device log is
glibc's restated (csrc/ce_glibc_log.hpp), so each entropy is the reference's
bit for bit; selected indices bit-exact under the lowest-index tie-break;
frequency tables bit-exact.
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

ENT_TOL_ULP = 0  # written-down tolerance on f64 entropies: none (north star allows 1e-6 relative)

MC_CASES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLDEN, "mc_*.npz")))


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def assert_ent_exact(got, exp):
    """Entropies equal bit for bit (NaN matches NaN; ENT_TOL_ULP = 0)."""
    got = np.ascontiguousarray(got, np.float64)
    exp = np.ascontiguousarray(exp, np.float64)
    assert got.shape == exp.shape
    nan_g, nan_e = np.isnan(got), np.isnan(exp)
    assert np.array_equal(nan_g, nan_e)
    ok = ~nan_e
    ulp = np.abs(got[ok].view(np.int64) - exp[ok].view(np.int64))
    assert ulp.max(initial=0) <= ENT_TOL_ULP, (int(ulp.max()), int((ulp > 0).sum()))


def idx_np(t):
    i = t.cpu().numpy()
    return i[i >= 0]


@pytest.mark.parametrize("case", MC_CASES)
@pytest.mark.parametrize("layout", ["MNC", "NMC"])
def test_mc_golden(ce, case, layout):
    g = golden(case)
    P = g["P"]
    if layout == "NMC":
        P = np.transpose(P, (1, 0, 2))
    Pd = dev(P)
    ent = ce.ops.committee_entropy(Pd, layout).cpu().numpy()
    assert_ent_exact(ent, g["ent"])
    _, idx = ce.ops.select_mc(Pd, int(g["q"]), layout)
    assert np.array_equal(idx_np(idx), g["canon"])


def test_mc_f32_input(ce):
    g = golden("mc_m16_f32")
    Pd = dev(g["P"].astype(np.float32))
    assert_ent_exact(ce.ops.committee_entropy(Pd).cpu().numpy(), g["ent"])
    _, idx = ce.ops.select_mc(Pd, 10)
    assert np.array_equal(idx_np(idx), g["canon"])


def test_mc_bf16_input(ce):
    g = golden("mc_m8_bf16")
    Pd = dev(g["P_bits"].view(np.int16)).view(torch.bfloat16)
    assert_ent_exact(ce.ops.committee_entropy(Pd).cpu().numpy(), g["ent"])
    _, idx = ce.ops.select_mc(Pd, 10)
    assert np.array_equal(idx_np(idx), g["canon"])


def test_mc_mean_output(ce):
    g = golden("mc_m20_mixed_unnorm")
    ent, mean = ce.ops.committee_entropy(dev(g["P"]), return_mean=True)
    assert np.array_equal(mean.cpu().numpy(), g["mean"])


@pytest.mark.parametrize("tag", ["d03", "d100"])
def test_hc_votes(ce, tag):
    g = golden(f"hc_votes_{tag}")
    freq, ent = ce.ops.vote_table(dev(g["votes"]))
    assert np.array_equal(freq.cpu().numpy(), g["freq"])
    assert_ent_exact(ent.cpu().numpy(), g["ent"])
    from ce_amd import select_queries

    assert np.array_equal(select_queries("hc", 10, votes=g["votes"]), g["canon"])
    assert np.array_equal(select_queries("hc", 10, hc=g["freq"]), g["canon"])


def test_hc_va_raw(ce):
    g = golden("hc_va_raw")
    freq, ent = ce.ops.va_table(dev(g["va"]))
    assert np.array_equal(freq.cpu().numpy(), g["freq"])
    assert_ent_exact(ent.cpu().numpy(), g["ent"])


def test_mix(ce):
    g = golden("mix_m4")
    _, idx = ce.ops.select_mix(dev(g["P"]), dev(g["hc"]), 10)
    assert np.array_equal(idx_np(idx), g["canon"])
    from ce_amd import select_queries

    assert np.array_equal(select_queries("mix", 10, committee=list(g["P"]), hc=g["hc"]), g["canon"])


def test_batched_ragged(ce):
    g = golden("batched_u8")
    _, idx = ce.ops.select_batched(dev(g["P"]), dev(g["offsets"]), 10)
    assert np.array_equal(idx.cpu().numpy(), g["canon"])


# ---------------------------------------------------------------------------
# Against the oracle on larger seeded inputs (multi-block + merge paths)
# ---------------------------------------------------------------------------
def synth(rng, N, M, C, dtype=np.float32, unnorm=0.01, quant=None):
    e = -np.log(rng.random((N, M, C)))
    P = e / e.sum(-1, keepdims=True)
    if quant:
        P = np.floor(P * quant) / quant
    if unnorm:
        rows = rng.random((N, M)) < unnorm
        P[rows] *= rng.uniform(0.5, 2.0, size=(rows.sum(), 1))
    return P.astype(dtype)


@pytest.mark.parametrize("N,M,q,quant", [(1_000_000, 16, 10, None), (300_000, 16, 100, None),
                                         (500_000, 4, 10, 8), (200_000, 20, 700, None)])
def test_mc_vs_oracle_large(ce, N, M, q, quant):
    from oracle import ce_oracle as O

    rng = np.random.default_rng(N + M + q)
    P = synth(rng, N, M, 4, quant=quant)
    ent_o = O.oracle_committee_entropy(P, "NMC")
    _, idx_o = O.oracle_topq(ent_o, q)
    Pd = dev(P)
    ent = ce.ops.committee_entropy(Pd, "NMC").cpu().numpy()
    assert_ent_exact(ent, ent_o)
    _, idx = ce.ops.select_mc(Pd, q, "NMC")
    assert np.array_equal(idx_np(idx), idx_o)
    # member-major copy of the same data gives the same answer
    _, idx2 = ce.ops.select_mc(Pd.permute(1, 0, 2).contiguous(), q, "MNC")
    assert np.array_equal(idx_np(idx2), idx_o)


def test_topq_edge_cases(ce):
    from oracle import ce_oracle as O

    rng = np.random.default_rng(3)
    e = rng.random(100_000)
    e[rng.integers(0, e.size, 40)] = np.nan
    e[rng.integers(0, e.size, 2000)] = 0.75
    e[rng.integers(0, e.size, 100)] = -np.inf
    e[5] = -0.0
    for q in (1, 10, 37, 256, 257, 1000, 2048):
        v, i = ce.ops.topq(dev(e), q, base_idx=7)
        vo, io = O.oracle_topq(e, q, base=7)
        assert np.array_equal(idx_np(i), io), q
    # q > N: all items, padding -1
    v, i = ce.ops.topq(dev(np.array([0.2, np.nan, 0.9])), 10)
    assert i.cpu().numpy().tolist() == [1, 2, 0] + [-1] * 7
    # empty pool
    v, i = ce.ops.topq(dev(np.zeros(0)), 5)
    assert (i.cpu().numpy() == -1).all()


def test_all_ties_and_sorted_inputs(ce):
    """Adversarial orders for the LDS buffer: all-equal entropies (index
    tie-break only) and ascending entropies (every item beats the threshold)."""
    from oracle import ce_oracle as O

    N = 300_000
    for e in (np.full(N, 0.5), np.linspace(0.0, 1.0, N), np.linspace(1.0, 0.0, N)):
        for q in (10, 300):
            _, i = ce.ops.topq(dev(e), q)
            assert np.array_equal(idx_np(i), O.oracle_topq(e, q)[1])


def test_merge(ce):
    from oracle import ce_oracle as O

    rng = np.random.default_rng(9)
    q, nl = 10, 8
    vals = rng.random((nl, q))
    vals[2, 3] = np.nan
    vals[4, :] = 0.5  # ties across lists
    idx = rng.permutation(10_000)[: nl * q].reshape(nl, q).astype(np.int64)
    for r in range(nl):  # every list best-first, as the ce_* outputs are (the merge's precondition)
        o = O.canonical_order(vals[r], q)
        vals[r], idx[r] = vals[r][o], idx[r][o]
        ent = np.where(np.isnan(vals[r]), np.inf, vals[r])
        o2 = np.lexsort((idx[r], -ent))
        vals[r], idx[r] = vals[r][o2], idx[r][o2]
    idx[5, 7:] = -1
    v, i = ce.ops.topq_merge(dev(vals.ravel()), dev(idx.ravel()), q)
    vo, io = O.oracle_topq_merge(vals.ravel(), idx.ravel(), q)
    assert np.array_equal(idx_np(i), io)


def test_errors_are_loud(ce):
    with pytest.raises(ValueError):
        ce.ops.select_mc(torch.zeros((4, 10, 4), device="cuda"), -1)
    v, i = ce.ops.select_mc(torch.zeros((4, 10, 4), device="cuda"), 0)  # q = 0: nothing selected
    assert v.numel() == 0 and i.numel() == 0
    with pytest.raises(ValueError):
        ce.ops.select_mc(torch.zeros((4, 10, 4), device="cuda"), 10, layout="XYZ")
    with pytest.raises(ValueError):
        ce.ops.select_mc(torch.zeros((4, 10, 4)), 10)  # CPU tensor: no CPU path
    from ce_amd import select_queries

    with pytest.raises(ValueError):
        select_queries("qbc", 10)


def test_full_size_vs_oracle(ce):
    """The headline workload itself (BASELINE configs[3], bench.py's pool: 100M
    items x 16 members x 4 classes fp32, item-major, 25.6 GB, q = 10): the
    fused selection on the whole resident pool equals the C oracle's, which
    scores the same pool in 10M-item chunks on the host and merges the chunks'
    top-q exactly (the global top-q is a subset of the union)."""
    from bench import make_pool
    from oracle import ce_oracle as O

    N, M, C, q, CH = 100_000_000, 16, 4, 10, 10_000_000
    P = make_pool(0, N, M, C, "cuda")
    vals, idx = ce.ops.select_mc(P, q, "NMC")
    got_v, got_i = vals.cpu().numpy(), idx_np(idx)
    cv, ci = [], []
    for lo in range(0, N, CH):
        ent = O.oracle_committee_entropy(P[lo:lo + CH].cpu().numpy(), "NMC")
        v, i = O.oracle_topq(ent, q, base=lo)
        cv.append(v)
        ci.append(i)
        print(f"oracle chunk {lo // CH}: best {v[0]!r}", flush=True)
    vo, io = O.oracle_topq_merge(np.concatenate(cv), np.concatenate(ci), q)
    assert np.array_equal(got_i, io), (got_i, io)
    assert_ent_exact(got_v[:len(io)], vo)
    del P
    torch.cuda.empty_cache()


def test_device_log_bit_exact(ce):
    """ce_log_f64 (the log inside every device entropy) against libm's log on
    1e8 arguments covering every branch of glibc's algorithm."""
    from oracle import ce_oracle as O

    bad = 0
    for c in range(5):
        x = O.log_test_arguments(20_000_000, 100 + c)
        bad += O.oracle_log_check(x, ce.ops.log_f64(dev(x)).cpu().numpy())
    assert bad == 0


def test_device_exp_bit_exact(ce):
    """ce_exp_f64 (glibc's exp restated: the GaussianNB member's logsumexp and
    expit) against libm's exp on 1e8 arguments covering every branch."""
    from oracle import ce_oracle as O

    bad = 0
    for c in range(5):
        x = O.exp_test_arguments(20_000_000, 200 + c)
        bad += O.oracle_exp_check(x, ce.ops.exp_f64(dev(x)).cpu().numpy())
    assert bad == 0


def test_approx_entropy_bound(ce):
    """The single-block pools' prefilter (csrc/ce_small.hpp) admits every item
    whose approximate entropy is within 2 * kApproxErr2PerClass * C (log2
    units) of the floor; that is a superset of the exact top q only if the
    device's f32 approximation (hardware rcp / log2) stays within
    kApproxErr2PerClass * C of the exact entropy.  Measured here on 1.3e7 rows
    -- Dirichlet rows from very peaked to near-uniform, zeros, classes down to
    1e-300, unnormalised rows with sums across [2^-100, 2^100] -- against the
    exact restatement, with a 4x margin; the special flag (rows the exact path
    takes: negative / -0.0 / non-finite means, f32 sums outside [2^-100,
    2^100]) must match its rule exactly."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(4242)
    worst = {}
    for C in (2, 3, 4, 8):
        parts = []
        for a in (0.02, 0.2, 1.0, 5.0, 100.0):
            parts.append(rng.dirichlet(np.full(C, a), 400_000))
        z = rng.dirichlet(np.ones(C), 300_000)
        z[rng.random(z.shape) < 0.3] = 0.0  # zero classes (and some all-zero rows: special)
        parts.append(z)
        t = rng.dirichlet(np.ones(C), 300_000)
        t[:, 0] = 10.0 ** rng.uniform(-300, -20, len(t))  # tiny classes, f64 and f32-denormal range
        parts.append(t)
        u = rng.dirichlet(np.ones(C), 300_000) * (10.0 ** rng.uniform(-30.5, 30.5, (300_000, 1)))
        parts.append(u)  # unnormalised, sums across (and a little beyond) [2^-100, 2^100]
        v = np.full((200_000, C), 1.0 / C) + rng.normal(0, 1e-7, (200_000, C))
        parts.append(np.abs(v))  # near-uniform
        sp = rng.dirichlet(np.ones(C), 20_000)
        k = rng.integers(0, 5, len(sp))
        sp[k == 0, 0] = -sp[k == 0, 0]
        sp[k == 1, 0] = np.nan
        sp[k == 2, 0] = np.inf
        sp[k == 3, 0] = -0.0
        parts.append(sp)
        R = np.ascontiguousarray(np.concatenate(parts))
        h2, spec = ce.ops.approx_entropy(dev(R))
        h2, spec = h2.cpu().numpy().astype(np.float64), spec.cpu().numpy()
        mf = R.astype(np.float32)
        S = np.zeros(len(R), np.float32)
        for c in range(C):
            S = (S + mf[:, c]).astype(np.float32)
        rule = (np.signbit(R) | ~np.isfinite(R)).any(1) | ~((S >= np.float32(2.0 ** -100)) & (S <= np.float32(2.0 ** 100)))
        assert np.array_equal(spec, rule), C
        ok = ~spec
        exact = O.oracle_table_entropy(R[ok]) / np.log(2.0)
        err = np.abs(h2[ok] - exact)
        bound = 2e-5 * C  # kApproxErr2PerClass * C
        worst[C] = float(err.max())
        assert err.max() <= bound / 4, (C, float(err.max()), bound)
    print("max |approx - exact| (log2 units) per C:", worst)


@pytest.mark.parametrize("dtype", ["bf16", "f32"])
def test_wide_approx_entropy_bound(ce, dtype):
    """The C5 stream's prefilter (csrc/ce_wide.hpp wave_approx_entropy) skips an
    item only when its f32 approximate entropy is more than 2 * kWideApproxErr2
    (log2 units) below the threshold; that never drops a top-q item if the
    device approximation stays within kWideApproxErr2 of the exact entropy.
    Measured here on >= 1.1e6 wide rows per dtype layout -- Dirichlet from very
    peaked to near-uniform, zero classes, classes down to 1e-300, unnormalised
    rows with sums from 2^-90 to 2^90, C in {16, 136, 1000, 2048} (the vector
    stream's row widths; C = 129 has no vector path and never prefilters) --
    against the exact device entropy (glibc log, bit-equal to scipy), with a
    4x margin; rows that must take the exact path (negative, -0.0, NaN, inf,
    sums outside [2^-100, 2^100]) are flagged special."""
    kWideApproxErr2 = 2e-4  # csrc/ce_wide.hpp
    tdt = torch.bfloat16 if dtype == "bf16" else torch.float32
    g = torch.Generator(device="cuda").manual_seed(505)
    worst, n_rows = {}, 0
    for C in (16, 136, 1000, 2048):
        per = 300_000 if C <= 136 else 40_000
        parts = []
        for a in (0.02, 0.2, 1.0, 5.0, 100.0):
            gam = torch._standard_gamma(torch.full((per, C), a, dtype=torch.float64, device="cuda"), generator=g)
            parts.append(gam / gam.sum(1, keepdim=True))
        base = parts[2]
        z = base.clone()
        z[torch.rand(z.shape, generator=g, device="cuda", dtype=torch.float64) < 0.3] = 0.0
        parts.append(z)  # zero classes
        t = base.clone()
        t[:, 0] = 10.0 ** (torch.rand(per, generator=g, device="cuda", dtype=torch.float64) * -280 - 20)
        parts.append(t)  # tiny classes
        u = base * (2.0 ** ((torch.rand((per, 1), generator=g, device="cuda", dtype=torch.float64) - 0.5) * 180))
        parts.append(u)  # unnormalised member sums, 2^-90 .. 2^90
        v = torch.full((per, C), 1.0 / C, dtype=torch.float64, device="cuda")
        v += torch.randn((per, C), generator=g, device="cuda", dtype=torch.float64) * (1e-7 / C)
        parts.append(v.abs())  # near-uniform
        R = torch.cat(parts)
        h2, spec = ce.ops.wide_approx_entropy(R, tdt)
        assert not bool(spec.any()), C
        exact = ce.ops.committee_entropy(R.view(R.shape[0], 1, C), "NMC") / np.log(2.0)
        err = (h2.double() - exact).abs()
        worst[C] = float(err.max())
        n_rows += R.shape[0]
        assert worst[C] <= kWideApproxErr2 / 4, (C, worst[C])
        # rows the approximation does not cover are flagged (the exact path decides them)
        sp = base[:8].clone().repeat(8, 1)
        sp[0:8, 0] = -sp[0:8, 0]
        sp[8:16, 1] = float("nan")
        sp[16:24, 2] = float("inf")
        sp[24:32, 3] = -0.0
        sp[32:40] *= 2.0 ** -110
        sp[40:48] *= 2.0 ** 110
        sp[48:56] = 0.0
        _, spf = ce.ops.wide_approx_entropy(sp, tdt)
        assert bool(spf[:56].all()) and not bool(spf[56:].any()), C
        del parts, R, base, z, t, u, v
    assert n_rows >= 1_100_000
    print(f"{dtype}: max |approx - exact| (log2 units) per C:", worst)


def test_row_division_bit_exact(ce):
    """The entropy's row division (one shared reciprocal per row, exact by
    construction -- DESIGN.md 'Numerics') equals IEEE x / s on 6e7 pairs:
    probabilities over row sums, random exponents across and beyond the fast
    range [2^-300, 2^300), its boundaries +- a few ulps, zeros, signed zeros,
    negatives, subnormals, inf and NaN."""
    rng = np.random.default_rng(77)
    n = 20_000_000
    parts = []
    s = rng.uniform(0.5, 2.0, n)
    parts.append((rng.random(n) * s, s))
    e1, e2 = rng.integers(-1100, 1024, n), rng.integers(-1100, 1024, n)
    parts.append((np.ldexp(rng.uniform(-1, 1, n), e1), np.ldexp(rng.uniform(-1, 1, n), e2)))
    edges = np.array([2.0 ** -300, 2.0 ** 300, 2.0 ** -301, 2.0 ** 299, 5e-324, 2.2250738585072014e-308,
                      1.7976931348623157e308, np.inf, -np.inf, np.nan, 0.0, -0.0, 1.0, -1.0])
    edges = np.concatenate([edges, np.nextafter(edges[:4], np.inf), np.nextafter(edges[:4], -np.inf)])
    xs, ss = np.meshgrid(edges, edges)
    parts.append((xs.ravel(), ss.ravel()))
    k = rng.integers(-320, 320, n)
    parts.append((np.ldexp(rng.random(n), k), np.ldexp(rng.uniform(0.5, 1.0, n), -k // 2)))
    bad = 0
    for p, (x, sv) in enumerate(parts):
        got = ce.ops.row_div_f64(dev(x), dev(sv)).cpu().numpy()
        with np.errstate(all="ignore"):
            exp = x / sv
        same = (got.view(np.int64) == exp.view(np.int64)) | (np.isnan(got) & np.isnan(exp))
        nb = int((~same).sum())
        if nb:
            w = np.flatnonzero(~same)[:12]
            print(f"part {p}: {nb} mismatches, e.g.")
            for i in w:
                print(f"  x={x[i].hex()} s={sv[i].hex()} got={got[i].hex()} ieee={exp[i].hex()}")
        bad += nb
    assert bad == 0


def _bf16_bits(P32):
    """float32 -> bf16 bit patterns (round to nearest even), as uint16."""
    u = P32.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16)


@pytest.mark.parametrize("N,M,C,dt", [(5_000, 32, 1000, "bf16"), (3_001, 5, 1000, "bf16"),
                                      (2_000, 7, 1000, "f32"), (1_500, 3, 2048, "f64"),
                                      (4_000, 9, 136, "bf16")])
def test_wide_stream_vs_oracle(ce, N, M, C, dt):
    """The pipelined wide-class stream (one wave per item, member batches past M
    masked) against the oracle, item-major and member-major, several waves'
    worth of items each."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(N + M + C)
    P = synth(rng, N, M, C, np.float32)
    if dt == "bf16":
        host = _bf16_bits(P)
        Pd = dev(host.view(np.int16)).view(torch.bfloat16)
    else:
        host = P.astype(np.float64) if dt == "f64" else P
        Pd = dev(host)
    ent_o = O.oracle_committee_entropy(host, "NMC")
    for q in (10, 64):
        _, idx_o = O.oracle_topq(ent_o, q)
        _, idx = ce.ops.select_mc(Pd, q, "NMC")
        assert np.array_equal(idx_np(idx), idx_o), (q, "NMC")
    _, idx = ce.ops.select_mc(Pd.permute(1, 0, 2).contiguous(), 10, "MNC")
    assert np.array_equal(idx_np(idx), O.oracle_topq(ent_o, 10)[1])


def test_frames_dma_tiles_vs_oracle():
    """ce_select_frames with the grouped members staged by LDS-DMA tiles
    (k_frames_lanes<C, true>; by default only pools with >= 4 steps per wave
    take them) forced on by CE_AMD_FRAMES_DMA=1 in a child process: the fused
    frame tests against the restated groupby mean + oracle."""
    import subprocess
    import sys

    env = dict(os.environ, CE_AMD_FRAMES_DMA="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu",
                        "-k", "frames_fused_selection or frames_to_selection", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


@pytest.mark.parametrize("sizes", [[1608] * 37, [1, 64, 65, 0, 5000, 127, 20000, 3], [100_000, 70_000]])
def test_batched_segments_vs_oracle(ce, sizes):
    """Per-user selection in one launch (16-wave blocks, one per user): ragged
    users, an empty user, users of 1 item and users spanning many iterations."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(len(sizes))
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    P = synth(rng, int(offs[-1]), 4, 4, np.float32, quant=16)  # quantised: many exact ties
    Pm = np.ascontiguousarray(np.transpose(P, (1, 0, 2)))
    ent_o = O.oracle_committee_entropy(P, "NMC")
    _, idx = ce.ops.select_batched(dev(Pm), dev(offs), 10, "MNC")
    idx = idx.cpu().numpy()
    for u in range(len(sizes)):
        io = O.oracle_topq(ent_o[offs[u]:offs[u + 1]], 10)[1]
        got = idx[u][idx[u] >= 0]
        assert np.array_equal(got, io), u


@pytest.mark.parametrize("q", [10, 1, 64])
def test_batched_500_users_vs_oracle(ce, q):
    """BASELINE configs[2] at its full size: 500 users x 4 members x 1608
    excerpts x 4 classes fp32 in one launch (one block per user), every user's
    top-q against the oracle; the committee is quantised so exact ties cross
    the q-th boundary."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(500 + q)
    U, Nu = 500, 1608
    offs = np.arange(U + 1, dtype=np.int64) * Nu
    P = synth(rng, U * Nu, 4, 4, np.float32, quant=32)
    ent_o = O.oracle_committee_entropy(P, "NMC")
    _, idx = ce.ops.select_batched(dev(np.ascontiguousarray(np.transpose(P, (1, 0, 2)))), dev(offs), q, "MNC")
    idx = idx.cpu().numpy()
    for u in range(U):
        io = O.oracle_topq(ent_o[offs[u]:offs[u + 1]], q)[1]
        assert np.array_equal(idx[u][idx[u] >= 0], io), u


def test_batched_tie_floods(ce):
    """Users whose items tie in masses at the floor (all-equal rows, two-valued
    rows, NaN rows): the single-block survivor list overflows and the kernel
    takes its per-wave fallback -- lowest positions first, NaN first."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(12)
    sizes = [1608, 1608, 2048, 700, 1608, 0, 1]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    P = synth(rng, int(offs[-1]), 4, 4, np.float32)
    P[offs[0]:offs[1]] = 0.25                                  # all equal
    P[offs[1]:offs[2]] = np.where(rng.random((1608, 1, 1)) < 0.5, 0.25, [0.7, 0.1, 0.1, 0.1])
    P[offs[4] + rng.integers(0, 1608, 40)] = np.nan            # NaN rows rank first
    ent_o = O.oracle_committee_entropy(P, "NMC")
    Pm = dev(np.ascontiguousarray(np.transpose(P, (1, 0, 2))))
    for q in (10, 64):
        _, idx = ce.ops.select_batched(Pm, dev(offs), q, "MNC")
        idx = idx.cpu().numpy()
        for u in range(len(sizes)):
            io = O.oracle_topq(ent_o[offs[u]:offs[u + 1]], q)[1]
            assert np.array_equal(idx[u][idx[u] >= 0], io), (q, u)


@pytest.mark.parametrize("nl,q", [(1, 10), (3, 1), (64, 10), (1024, 10), (1024, 64), (5000, 17)])
def test_merge_lists_vs_oracle(ce, nl, q):
    """Stage-2 merge (register lists, 16 waves) over many best-first lists,
    with ties across lists, NaN, empty tails and whole empty lists."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(nl * 100 + q)
    vals = np.round(rng.random((nl, q)), 2)  # coarse: many equal keys
    vals[rng.random((nl, q)) < 0.001] = np.nan
    idx = rng.permutation(nl * q * 3)[: nl * q].reshape(nl, q).astype(np.int64)
    for r in range(nl):
        key = np.where(np.isnan(vals[r]), np.inf, vals[r])
        o = np.lexsort((idx[r], -key))
        vals[r], idx[r] = vals[r][o], idx[r][o]
    cut = rng.integers(0, q + 1, nl)
    for r in range(nl):
        if rng.random() < 0.2:
            idx[r, cut[r]:] = -1
            vals[r, cut[r]:] = np.nan
    v, i = ce.ops.topq_merge(dev(vals.ravel()), dev(idx.ravel()), q)
    vo, io = O.oracle_topq_merge(vals.ravel(), idx.ravel(), q)
    assert np.array_equal(idx_np(i), io)


@pytest.mark.parametrize("nl,q", [(1024, 10), (1000, 16), (700, 3)])
def test_merge_survivor_overflow(ce, nl, q):
    """The floor merge's overflow path: list i holds the values of ranks
    q*i .. q*i+q-1, so the floor (the rank-(q-1) head of 64 group bests of 16
    lists) admits ~16*q*q candidates -- more than its 1024 LDS slots for the
    first two cases -- and the register lists + tree merge take over."""
    from oracle import ce_oracle as O

    n = nl * q
    vals = np.linspace(2.0, 1.0, n).reshape(nl, q)
    idx = np.arange(n, dtype=np.int64)[::-1].copy().reshape(nl, q)
    v, i = ce.ops.topq_merge(dev(vals.ravel()), dev(idx.ravel()), q)
    vo, io = O.oracle_topq_merge(vals.ravel(), idx.ravel(), q)
    assert np.array_equal(idx_np(i), io) and np.array_equal(v.cpu().numpy(), vo)
    # all equal: only the position order decides (lists best-first: ascending positions)
    vals[:] = 0.5
    idx = np.sort(idx, axis=1)
    v, i = ce.ops.topq_merge(dev(vals.ravel()), dev(idx.ravel()), q)
    assert np.array_equal(idx_np(i), O.oracle_topq_merge(vals.ravel(), idx.ravel(), q)[1])


@pytest.mark.parametrize("N", [1, 63, 64, 65, 1608, 4096, 16384])
def test_small_pool_single_launch(ce, N):
    """Pools under kSmallPoolBytes: one 16-wave block scores and selects."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(N)
    P = synth(rng, N, 4, 4, np.float32, quant=8)
    for q in (1, 10, 64):
        _, idx = ce.ops.select_mc(dev(np.transpose(P, (1, 0, 2))), q, "MNC")
        assert np.array_equal(idx_np(idx), O.oracle_select_mc(P, q, "NMC")[1]), q


@pytest.mark.parametrize("C", [2, 3, 4, 8])
@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_small_pool_prefilter_specials(ce, C, dt):
    """The single-block pools rank by an approximate entropy and evaluate the
    exact one for survivors only (csrc/ce_small.hpp): rows outside the
    approximation's domain -- negative, -0.0, NaN, +inf and all-zero means,
    row sums below 2^-100 or above 2^100 -- must always survive and take the
    exact path, and near-ties closer than the approximation's error must be
    ordered by their exact entropies.  One pool, the batched users and (C = 4)
    the mix, against the oracle."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(100 + C)
    N, M = 1608, 4
    P = np.ascontiguousarray(np.transpose(synth(rng, N, M, C, np.float64, quant=0), (1, 0, 2)))  # [M, N, C]
    base = P[:, 0].copy()
    k = rng.permutation(N)
    P[:, k[0:6]] = base[:, None] * (1 + 1e-12 * np.arange(6))[None, :, None]  # near-ties
    P[:, k[6:9]] = 0.0                       # all-zero rows: NaN entropy, ranked first
    P[0, k[9:12], 0] = np.nan                # NaN member value
    P[1, k[12:15], 1 % C] = -0.05            # a negative mean: -inf or NaN entropy
    P[2, k[15:17], 0] = np.inf               # inf: NaN entropy
    P[:, k[17:20]] *= 1e-35                  # sums far below 2^-100
    P[:, k[20:23]] *= 1e35                   # sums far above 2^100
    P[:, k[23:26]] = -0.0                    # -0.0 everywhere
    P[:, k[26:29]] *= 1e-300                 # f64-subnormal-range rows (f32: zero rows)
    P = P.astype(dt)
    Pn = np.ascontiguousarray(np.transpose(P, (1, 0, 2)))  # [N, M, C]
    for q in (1, 10, 64):
        _, idx = ce.ops.select_mc(dev(Pn), q, "NMC")
        assert np.array_equal(idx_np(idx), O.oracle_select_mc(Pn, q, "NMC")[1]), q
    # batched: three users over the same rows (specials in each), plus the mix
    offs = np.array([0, 500, 1100, N], np.int64)
    ent = O.oracle_committee_entropy(P, "MNC")
    for q in (10, 64):
        _, i = ce.ops.select_batched(dev(P), dev(offs), q, "MNC")
        got = i.cpu().numpy()
        for u in range(3):
            exp = O.canonical_order(ent[offs[u]:offs[u + 1]], q)
            assert np.array_equal(got[u][got[u] >= 0], exp), (u, q)
    if C == 4:
        H = Pn[:, 0, :].astype(np.float64).copy()
        H[k[30:33]] = 0.0
        q = 10
        _, i = ce.ops.select_mix(dev(P), dev(H), q, "MNC")
        want = O.canonical_order(np.concatenate([ent, O.oracle_table_entropy(H)]), q)
        assert np.array_equal(idx_np(i), want)


def test_ticket_counters_return_to_zero(ce):
    """The tiled small-pool kernels and the folded stage 2 draw arrival tickets
    from the workspace header (include/ce.h: zero-filled before first use,
    zero again after every call): after a run of every ticketed path, the
    header is all zero and repeated calls keep selecting the same positions."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(4)
    P = synth(rng, 3000, 4, 4, np.float32, quant=8)
    Pm = dev(np.ascontiguousarray(np.transpose(P, (1, 0, 2))))
    big = dev(synth(rng, 400_000, 16, 4))
    hc = dev(np.round(rng.dirichlet(np.ones(4), 1500), 3))
    offs = dev(np.array([0, 1000, 1000, 3000], np.int64))
    exp = O.oracle_select_mc(P, 10, "NMC")[1]
    for _ in range(3):
        assert np.array_equal(idx_np(ce.ops.select_mc(Pm, 10, "MNC")[1]), exp)
        ce.ops.select_mix(Pm, hc, 10)
        ce.ops.select_batched(Pm, offs, 10)
        ce.ops.select_mc(big, 10, "NMC")
    torch.cuda.synchronize()
    ws = ce.ops.WORKSPACE.get(torch.device("cuda", torch.cuda.current_device()), 0)
    off = (-ws.data_ptr()) % 256
    assert int(ws[off:off + 65536].count_nonzero()) == 0


@pytest.mark.parametrize("world", [1, 2, 8])
def test_record_exchange(ce, world):
    """The multi-GPU exchange on one device: each 'rank' scores its shard
    (stage 1 + stage 2 into ce_cand records), the records are concatenated
    rank-major as the all-gather leaves them, and ce_merge_cands gives the
    global top-q."""
    from ce_amd import dist as cdist
    from oracle import ce_oracle as O

    rng = np.random.default_rng(world)
    N, q = 300_001, 10
    P = synth(rng, N, 16, 4, quant=32)
    Pd = dev(P)
    recs = []
    for r in range(world):
        lo, hi = cdist.shard_range(N, r, world)
        plan = ce.ops.MCPlan(Pd[lo:hi], q, "NMC", base_idx=lo)
        plan.partial()
        recs.append(plan.finish_cands())
        # the one-launch form (stage 2 folded into stage 1's last block) writes the same records
        assert torch.equal(plan.step_cands(), recs[-1])
        v1, i1 = plan.step()
        v2, i2 = ce.ops.merge_cands(recs[-1], q)
        assert torch.equal(i1, i2) and torch.equal(v1.view(torch.int64), v2.view(torch.int64))
    vals, idx = ce.ops.merge_cands(torch.cat(recs), q)
    vo, io = O.oracle_select_mc(P, q, "NMC")
    assert np.array_equal(idx_np(idx), io)
    assert_ent_exact(vals.cpu().numpy()[: len(io)], vo)
    with pytest.raises(ValueError):
        ce.ops.merge_cands(torch.cat(recs), 65)


@pytest.mark.parametrize("dt", [np.float64, np.float32])
@pytest.mark.parametrize("grouped", [True, False])
def test_segment_mean_vs_restatement(ce, dt, grouped):
    """groupby(['s_id']).mean() (amg_test.py:437) on the device, bit-exact vs
    the pandas-1.1.5 restatement: frames grouped (CSR only) or shuffled (perm),
    NaN cells, a song whose column is all-NaN, float32 rounding of the result."""
    from oracle.ce_oracle import ref_group_mean

    rng = np.random.default_rng(11 + grouped)
    F, C = 50_000, 4
    s_id = np.sort(rng.integers(0, 1608, F)) if grouped else rng.integers(0, 1608, F)
    vals = rng.random((F, C)).astype(dt)
    vals[rng.random((F, C)) < 0.02] = np.nan
    vals[s_id == s_id[0], 1] = np.nan
    exp, keys = ref_group_mean(vals, s_id)
    uniq, offsets, perm = ce.song_groups(s_id)
    assert np.array_equal(uniq, keys) and (perm is None) == grouped
    got = ce.ops.segment_mean(dev(vals), dev(offsets), None if perm is None else dev(perm))
    assert got.dtype == (torch.float32 if dt == np.float32 else torch.float64)
    assert np.array_equal(got.cpu().numpy(), exp, equal_nan=True)
    # into an f64 stack slot: the float32 result upcast, as np.array(pred_prob) does
    slot = torch.empty((2, len(uniq), C), dtype=torch.float64, device="cuda")
    ce.ops.segment_mean(dev(vals), dev(offsets), None if perm is None else dev(perm), out=slot[1])
    assert np.array_equal(slot[1].cpu().numpy(), exp.astype(np.float64), equal_nan=True)


@pytest.mark.parametrize("C,dt", [(4, np.float64), (2, np.float64), (8, np.float32), (4, np.float32)])
def test_segment_mean_tiles_large(ce, C, dt):
    """The LDS-DMA tile kernel (k_segment_mean_tiles: grouped dense rows, taken
    once every wave runs >= 4 steps) at 300k ragged songs (1..15 frames, 1 % of
    them 40): NaN cells, all-NaN songs, bit-exact vs the restatement, into a
    strided f64 stack slot too.  A step of 64 / C songs of these lengths stays
    inside one 16 KiB tile (TR = 16384 / (C * itemsize) rows), so a dozen songs
    of TR + 1 .. 3 TR rows are added: their steps take two to four tiles (the
    layouts around the tile edge are in test_gpu_frames_tiles.py)."""
    from oracle.ce_oracle import ref_group_mean

    rng = np.random.default_rng(C + (dt == np.float32))
    N = 300_000
    sizes = rng.integers(1, 16, N)
    sizes[rng.random(N) < 0.01] = 40
    TR = 16384 // (C * np.dtype(dt).itemsize)
    sizes[rng.choice(N, 12, replace=False)] = rng.integers(TR + 1, 3 * TR + 1, 12)  # longer than a tile
    assert (sizes > TR).sum() == 12
    s_id = np.repeat(np.arange(N), sizes)
    F = len(s_id)
    vals = rng.random((F, C)).astype(dt)
    vals[rng.random((F, C)) < 0.05] = np.nan
    vals[np.isin(s_id, np.arange(0, N, 997)), 0] = np.nan  # all-NaN columns
    exp, keys = ref_group_mean(vals, s_id)
    uniq, offsets, perm = ce.song_groups(s_id)
    assert perm is None and len(uniq) == N
    got = ce.ops.segment_mean(dev(vals), dev(offsets))
    assert np.array_equal(got.cpu().numpy(), exp, equal_nan=True)
    slot = torch.empty((2, N, C), dtype=torch.float64, device="cuda")
    ce.ops.segment_mean(dev(vals), dev(offsets), out=slot[1])
    assert np.array_equal(slot[1].cpu().numpy(), exp.astype(np.float64), equal_nan=True)


def test_segment_mean_tiles_forced_vs_restatement():
    """test_segment_mean_vs_restatement's small cases (1608 songs, NaN, all-NaN
    songs, f32 rounding) with the tile kernel forced by CE_AMD_FRAMES_DMA=1 in
    a child process; shuffled cases keep the thread-per-cell kernel."""
    import subprocess
    import sys

    env = dict(os.environ, CE_AMD_FRAMES_DMA="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu",
                        "-k", "segment_mean_vs_restatement", "-p", "no:cacheprovider"],
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout


def test_frames_to_selection(ce):
    """amg_test.py:426-445 end to end: three frame-level members (f64, f64,
    f32 -- GNB/SGD/XGB predict_proba over X_train rows) grouped per song on the
    device plus a song-level member (the CNN), stacked, scored and selected --
    against the restatement + oracle on the same inputs."""
    from oracle import ce_oracle as O
    from oracle.ce_oracle import ref_group_mean

    rng = np.random.default_rng(1987)
    F, C = 40_000, 4
    s_id = rng.permutation(np.repeat(np.arange(1608) * 3 + 1, 25))[:F]
    frame_members = []
    for dt in (np.float64, np.float64, np.float32):
        e = -np.log(rng.random((F, C)))
        frame_members.append((e / e.sum(-1, keepdims=True)).astype(dt))
    n_songs = len(np.unique(s_id))
    cnn = rng.random((n_songs, C)).astype(np.float32)  # sigmoid outputs, not normalised
    members = frame_members + [cnn]
    stack, uniq = ce.committee_from_frames(members, s_id)
    assert stack.dtype == torch.float64 and tuple(stack.shape) == (4, n_songs, C)
    pred_prob = [ref_group_mean(m, s_id)[0] for m in frame_members] + [cnn]
    P = np.array(pred_prob)  # the reference's stack (mixed -> float64)
    assert np.array_equal(stack.cpu().numpy(), P)
    _, idx = ce.ops.select_mc(stack, 10, "MNC")
    assert np.array_equal(idx_np(idx), O.oracle_select_mc(P, 10, "MNC")[1])


@pytest.mark.parametrize("grouped", [False, True])
def test_frames_fused_selection(ce, grouped):
    """SURVEY.md §8(f)1 in one kernel (ce_select_frames): frame-level members
    (f64, f64, f32 -- GNB/SGD/XGB over X_train rows, NaN cells included), a
    song-level f32 member (the CNN), shuffled or grouped frame order, a song
    whose frames are all NaN in one member (its mean is NaN: the song's
    entropy is NaN and it ranks first) -- equal to the restated groupby mean
    (amg_test.py:437) stacked like np.array(pred_prob) (:441) and selected by
    the oracle (:443-445), for q = 1, 10, 64."""
    from oracle import ce_oracle as O
    from oracle.ce_oracle import ref_group_mean

    rng = np.random.default_rng(21 + grouped)
    F, C = 60_000, 4
    s_id = rng.integers(0, 2500, F) * 7 + 3
    if grouped:
        s_id = np.sort(s_id)
    frame_members = []
    for dt in (np.float64, np.float64, np.float32):
        e = -np.log(rng.random((F, C)))
        fm = (e / e.sum(-1, keepdims=True))
        fm[rng.random((F, C)) < 0.01] = np.nan
        frame_members.append(fm.astype(dt))
    nan_song = s_id[5]
    frame_members[1][s_id == nan_song] = np.nan
    n_songs = len(np.unique(s_id))
    cnn = rng.random((n_songs, C)).astype(np.float32)
    members = frame_members + [cnn]
    pred_prob = [ref_group_mean(m, s_id)[0] for m in frame_members] + [cnn]
    P = np.array(pred_prob)
    for q in (1, 10, 64):
        got, uniq = ce.select_from_frames(members, s_id, q)
        exp = O.oracle_select_mc(P, q, "MNC")[1]
        assert np.array_equal(got, exp), (q, got[:5], exp[:5])
    assert uniq[got[0]] == nan_song  # NaN entropy first
    # the same through the two-step path (segment means -> stack -> select_mc)
    stack, _ = ce.committee_from_frames(members, s_id)
    assert np.array_equal(idx_np(ce.ops.select_mc(stack, 10, "MNC")[1]), O.oracle_select_mc(P, 10, "MNC")[1])


@pytest.mark.parametrize("C", [4, 8, 2])
def test_frames_large_shuffled_gather(ce, C):
    """A shuffled frame pool large enough (>= 4 steps per wave) for the
    non-temporal gather (k_frames_lanes<C, false, true>, ce_abi_frames.hip):
    300k songs of 1..7 frames, an f64 and an f32 frame member plus a song-level
    member, against the restated groupby mean + oracle; the reference-sized
    pool keeps the plain gather."""
    from oracle import ce_oracle as O
    from oracle.ce_oracle import ref_group_mean

    lib = ce._lib.load()
    rng = np.random.default_rng(300 + C)
    S = 300_000
    s_id = rng.permutation(np.repeat(np.arange(S) * 5 + 2, rng.integers(1, 8, S)))
    F = len(s_id)
    frame_members = []
    for dt in (np.float64, np.float32):
        e = -np.log(rng.random((F, C)))
        frame_members.append((e / e.sum(-1, keepdims=True)).astype(dt))
    song = rng.random((S, C)).astype(np.float32)
    P = np.array([ref_group_mean(m, s_id)[0] for m in frame_members] + [song])
    for q in (1, 10, 64):
        got, _ = ce.select_from_frames(frame_members + [song], s_id, q)
        assert lib.ce_last_kernel().decode() == f"ce::k_frames_lanes<{C}, false, true>"
        assert np.array_equal(got, O.oracle_select_mc(P, q, "MNC")[1]), q
    small = rng.permutation(np.repeat(np.arange(1608) * 5 + 2, 40))
    ce.select_from_frames([np.full((len(small), C), 1.0 / C)], small, 10)
    assert lib.ce_last_kernel().decode() == f"ce::k_frames_lanes<{C}, false, false>"


def _shrinking_reference(mode, epochs, q, committees, hc):
    """The reference's epoch loop on the host: pools shrink by the picks
    (amg_test.py:455, :484, :521-531) and every epoch selects on what is left
    (oracle arithmetic); picks are reported as positions of the full pool."""
    from oracle import ce_oracle as O

    N = committees[0].shape[1] if committees else hc.shape[0]
    alive = np.ones(N, bool)
    out = []
    for e in range(epochs):
        pos = np.flatnonzero(alive)
        if mode == "mc":
            _, i = O.oracle_select_mc(committees[e][:, pos], q, "MNC")
            picks = pos[i]
            songs = picks
        elif mode == "hc":
            _, i = O.oracle_topq(O.oracle_table_entropy(hc[pos]), q)
            picks = pos[i]
            songs = picks
        else:
            ent = np.concatenate([O.oracle_committee_entropy(committees[e][:, pos], "MNC"),
                                  O.oracle_table_entropy(hc[pos])])
            _, i = O.oracle_topq(ent, q)
            n = len(pos)
            picks = np.where(i < n, pos[np.minimum(i, n - 1)], N + pos[np.maximum(i - n, 0)])
            songs = np.where(picks >= N, picks - N, picks)
        alive[songs] = False
        out.append(np.asarray(picks, np.int64))
    return out


@pytest.mark.parametrize("mode", ["mc", "hc", "mix"])
def test_session_equals_shrinking_pools(ce, mode):
    """SelectionSession (full pool on the device + exclusion bitmap) selects,
    epoch after epoch, exactly what the reference's shrinking-pool loop does."""
    rng = np.random.default_rng(len(mode))
    N, q, epochs = 3000, 10, 6
    committees = [np.floor(synth(rng, N, 4, 4, np.float64) * 64).transpose(1, 0, 2) / 64 + 1e-3
                  for _ in range(epochs)]  # coarse: ties across the shrinking pool
    hc = np.round(rng.dirichlet(np.ones(4), N), 3)
    hc[::7] = hc[3]  # exact ties in the table
    exp = _shrinking_reference(mode, epochs, q, committees, hc)
    sess = ce.SelectionSession(q, mode, N, hc=hc if mode != "mc" else None)
    for e in range(epochs):
        got = sess.select(committee=dev(committees[e]) if mode != "hc" else None)
        assert np.array_equal(got, exp[e]), (mode, e, got, exp[e])
    assert sess.remaining == N - len(np.unique(np.concatenate(
        [np.where(x >= N, x - N, x) for x in exp])))


def test_session_mix_hc_in_own_row_order(ce):
    """Session mix with the hc table in the reference's own row order
    (annotation order, amg_test.py:359/:376) while the committee is in sorted
    s_id order (:437): hc rows tie heavily, so the lowest-position rule inside
    the hc segment of [mc; hc] (:477) must follow the TABLE's order.  The table
    covers only part of the pool.  Compared with the reference's shrinking-pool
    loop, where a pick through either segment drops the song from both pools
    (:484, :521-531)."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(77)
    N, Nh, q, epochs = 3000, 2400, 10, 8
    h2m = rng.permutation(N)[:Nh]                       # hc row j is committee item h2m[j]
    m2h = np.full(N, -1)
    m2h[h2m] = np.arange(Nh)
    committees = [np.floor(synth(rng, N, 4, 4, np.float64) * 8).transpose(1, 0, 2) / 8 + 1e-3
                  for _ in range(epochs)]
    hc = np.round(rng.dirichlet(np.ones(4), Nh), 1)     # few distinct rows: ties everywhere
    hc[::5] = [0.25, 0.25, 0.25, 0.25]                   # the maximal entropy, many times
    alive, alive_h = np.ones(N, bool), np.ones(Nh, bool)
    sess = ce.SelectionSession(q, "mix", N, hc=hc, hc_to_mc=h2m)
    hc_picks = 0
    for e in range(epochs):
        pos, hpos = np.flatnonzero(alive), np.flatnonzero(alive_h)
        ent = np.concatenate([O.oracle_committee_entropy(committees[e][:, pos], "MNC"),
                              O.oracle_table_entropy(hc[hpos])])
        _, i = O.oracle_topq(ent, q)
        n = len(pos)
        exp = np.where(i < n, pos[np.minimum(i, n - 1)], N + hpos[np.maximum(i - n, 0)])
        got = sess.select(committee=dev(committees[e]))
        assert np.array_equal(got, exp), (e, got, exp)
        hc_picks += int((exp >= N).sum())
        for p in exp:
            if p < N:
                alive[p] = False
                if m2h[p] >= 0:
                    alive_h[m2h[p]] = False
            else:
                alive_h[p - N] = False
                alive[h2m[p - N]] = False
    assert sess.remaining == alive.sum()
    assert hc_picks > 0  # the hc segment took part


def test_session_rand_and_exhaustion(ce):
    """rand draws only remaining items; a pool smaller than q*epochs runs dry
    without repeats; the exclusion API takes q > 64 too (block lists)."""
    N, q = 45, 10
    sess = ce.SelectionSession(q, "rand", N, rng=np.random.RandomState(1987))
    seen = []
    for _ in range(5):
        seen.extend(sess.select().tolist())
    assert sorted(seen) == list(range(N)) and sess.remaining == 0
    assert len(sess.select()) == 0
    P = dev(np.full((2, 100, 4), 0.25))
    ex = ce.ops.excl_bitmap(100, "cuda")
    ce.ops.mark_selected(ex, 100, torch.arange(0, 100, 2, device="cuda"))
    _, i = ce.ops.select_mc(P, 65, excl=ex)  # all tied: the 50 odd positions, then padding
    assert i.cpu().numpy().tolist() == list(range(1, 100, 2)) + [-1] * 15
    sess = ce.SelectionSession(4, "mc", 100)
    for _ in range(25):
        sess.select(committee=P)
    assert sess.remaining == 0 and len(sess.select(committee=P)) == 0


def test_session_rand_reference_stream(ce):
    """SelectionSession("rand") draws what amg_test.py:486-489 draws, epoch
    after epoch: the reference shuffles X_train.index.unique().tolist() (songs
    in first-appearance order of the frame rows, NOT sorted) with the global
    legacy RNG seeded by np.random.seed(1987) (:55), takes the first q, and
    drops those songs' rows from X_train (:521-531)."""
    import pandas as pd

    rng = np.random.default_rng(5)
    n_songs, q, epochs = 300, 10, 4
    s_ids = rng.permutation(np.arange(1000, 1000 + 3 * n_songs, 3))       # song ids, not positions
    frames = np.repeat(s_ids, rng.integers(1, 6, n_songs))                # frames per song
    X_train = pd.DataFrame({"f": np.arange(len(frames))}, index=pd.Index(rng.permutation(frames), name="s_id"))
    # the reference's loop
    np.random.seed(1987)
    exp, Xr = [], X_train
    for _ in range(epochs):
        pos_songs = Xr.index.unique().tolist()
        np.random.shuffle(pos_songs)
        q_songs = pos_songs[:q]
        exp.append(q_songs)
        Xr = Xr.drop(q_songs)
    # the session: pool positions = sorted song ids (the committee's groupby order, :437)
    uniq = np.unique(frames)
    order = np.searchsorted(uniq, X_train.index.unique().to_numpy())  # first-appearance order as positions
    np.random.seed(1987)
    sess = ce.SelectionSession(q, "rand", len(uniq), rand_order=order)
    for e in range(epochs):
        got = uniq[sess.select()].tolist()
        assert got == exp[e], (e, got, exp[e])
    with pytest.raises(ValueError):
        ce.SelectionSession(q, "rand", len(uniq), rand_order=order[:-1])


@pytest.mark.parametrize("N,M,C,dt", [(2_000_000, 16, 4, np.float32), (1_000_000, 4, 4, np.float64),
                                      (20_000, 3, 1000, np.float32)])
def test_entropy_bit_exact(ce, N, M, C, dt):
    """DESIGN.md 'Numerics': every sum is in numpy's order and the log is
    glibc's, so device and reference entropies are identical bit for bit."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(11)
    e = -np.log(rng.random((N, M, C)))
    P = (e / e.sum(-1, keepdims=True)).astype(dt)
    g = ce.ops.committee_entropy(dev(P), "NMC").cpu().numpy()
    o = O.oracle_committee_entropy(P, "NMC")
    ulp = np.abs(g.view(np.int64) - o.view(np.int64))
    print(f"N={N} M={M} C={C} {np.dtype(dt).name}: max ulp {ulp.max()}")
    assert ulp.max() == 0


def test_randomised_selection_fuzz(ce):
    """Seeded fuzz of the whole selection path against the oracle: random pool
    sizes (single-block, split small-pool, multi-block streaming), q in 1..64,
    member counts, layouts and dtypes, with NaN rows, exact ties, -0.0 and
    all-zero rows sprinkled in."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(20261016)
    for case in range(40):
        N = int(rng.choice([1, 2, 63, 65, 500, 1608, 5000, 70_000, 300_000]))
        M = int(rng.choice([1, 2, 3, 4, 7, 16]))
        C = int(rng.choice([2, 3, 4, 8]))
        q = int(rng.integers(1, 65))
        dt = [np.float32, np.float64][int(rng.integers(0, 2))]
        P = synth(rng, N, M, C, np.float64, quant=int(rng.choice([0, 4, 16])) or None).astype(dt)
        if N > 10:
            P[rng.integers(0, N, 3)] = np.nan
            P[rng.integers(0, N, 3)] = 0.0
            P[rng.integers(0, N, 5)] = P[0]
        lay = ["NMC", "MNC"][int(rng.integers(0, 2))]
        host = P if lay == "NMC" else np.ascontiguousarray(np.transpose(P, (1, 0, 2)))
        _, idx = ce.ops.select_mc(dev(host), q, lay)
        exp = O.oracle_select_mc(P, q, "NMC")[1]
        assert np.array_equal(idx_np(idx), exp), (case, N, M, C, q, dt, lay)


def test_member_inference_vs_restatement(ce):
    """§8(f)4: GaussianNB / SGD(log) predict_proba on the device against the
    restatement of the pinned sklearn 0.24.1 + scipy 1.5.4 + numpy 1.19.5 math.
    GaussianNB: BIT-EXACT (numpy's pairwise sums reproduced, glibc's exp / log
    restated on the device, the restatement evaluating exp / log with libm as
    numpy 1.19.5 does) -- both the feature-streamed kernel (D = 260) and the
    general one (a padded view), a prior of 0 and extreme features included.
    SGD: rtol 1e-10 (its dot products use a fixed wave order, the reference's
    BLAS an unspecified one: parity unpinned there)."""
    from conftest import fitted_members
    from oracle.ce_oracle import ref_gnb_predict_proba, ref_sgd_predict_proba

    gnb, sgd, Xt = fitted_members(n_test=20_000)
    Xt = Xt.copy()
    Xt[::997] *= 40.0  # far from every class: jll ~ -1e4, the logsumexp's shift matters
    Xd = dev(Xt)
    want = ref_gnb_predict_proba(Xt, gnb.theta_, gnb.var_, gnb.class_prior_)
    got = ce.ops.gnb_predict_proba(Xd, gnb.theta_, gnb.var_, gnb.class_prior_).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got != want).sum())
    Xpad = torch.zeros((Xt.shape[0], 264), dtype=torch.float64, device="cuda")
    Xpad[:, :260] = Xd
    got = ce.ops.gnb_predict_proba(Xpad[:, :260], gnb.theta_, gnb.var_, gnb.class_prior_).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    prior = np.array([0.0, 0.5, 0.25, 0.25])  # a class never seen: log(0) = -inf, p = 0
    want = ref_gnb_predict_proba(Xt[:3000], gnb.theta_, gnb.var_, prior)
    got = ce.ops.gnb_predict_proba(Xd[:3000], gnb.theta_, gnb.var_, prior).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # a device prior: log through the restated glibc log on the device (no host
    # sync), the same bits -- and the call replays from a HIP graph
    pd_ = dev(prior)
    got = ce.ops.gnb_predict_proba(Xd[:3000], gnb.theta_, gnb.var_, pd_).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    th, va = dev(gnb.theta_), dev(gnb.var_)
    out = torch.empty((3000, 4), dtype=torch.float64, device="cuda")
    ce.ops.gnb_predict_proba(Xd[:3000], th, va, pd_, out=out)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ce.ops.gnb_predict_proba(Xd[:3000], th, va, pd_, out=out)
    out.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint64), want.view(np.uint64))
    got = ce.ops.sgd_predict_proba(Xd, sgd.coef_, sgd.intercept_).cpu().numpy()
    np.testing.assert_allclose(got, ref_sgd_predict_proba(Xt, sgd.coef_, sgd.intercept_), rtol=1e-10, atol=1e-300)
    # a binary SGD model: [1 - p, p]
    got = ce.ops.sgd_predict_proba(Xd, sgd.coef_[:1], sgd.intercept_[:1]).cpu().numpy()
    np.testing.assert_allclose(got, ref_sgd_predict_proba(Xt, sgd.coef_[:1], sgd.intercept_[:1]), rtol=1e-10)


@pytest.mark.parametrize("F", [1, 7, 33, 20_003])
def test_sgd_span_kernel_matches_general(ce, F):
    """The contiguous-row SGD kernel (k_sgd_span260: D = ld = 260, K = C = 4)
    against the general 8-lane kernel, reached through a padded view (ld =
    264): the same FMA chains, so the same bits, ragged frame counts included."""
    from conftest import fitted_members

    _, sgd, Xt = fitted_members(n_test=F)
    Xd = dev(Xt)
    Xpad = torch.zeros((F, 264), dtype=torch.float64, device="cuda")
    Xpad[:, :260] = Xd
    got = ce.ops.sgd_predict_proba(Xd, sgd.coef_, sgd.intercept_).cpu().numpy()
    want = ce.ops.sgd_predict_proba(Xpad[:, :260], sgd.coef_, sgd.intercept_).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


@pytest.mark.parametrize("F", [1, 7, 33, 20_003])
def test_gnb_stream_kernel_matches_general(ce, F):
    """The feature-streamed GaussianNB kernel (k_gnb_stream260: D = ld = 260,
    C = 4) against the 8-lane kernel, reached through a padded view (ld = 264):
    the same terms, accumulators, butterflies and exp/log, so the same bits,
    ragged frame counts included."""
    from conftest import fitted_members

    gnb, _, Xt = fitted_members(n_test=F)
    Xd = dev(Xt)
    Xpad = torch.zeros((F, 264), dtype=torch.float64, device="cuda")
    Xpad[:, :260] = Xd
    got = ce.ops.gnb_predict_proba(Xd, gnb.theta_, gnb.var_, gnb.class_prior_).cpu().numpy()
    want = ce.ops.gnb_predict_proba(Xpad[:, :260], gnb.theta_, gnb.var_, gnb.class_prior_).cpu().numpy()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    # an infinite feature and a NaN feature: the inf / NaN paths of the terms
    Xt2 = Xt.copy()
    Xt2[0, 3] = np.inf
    if F > 1:
        Xt2[F - 1, 259] = np.nan
    Xpad[:, :260] = dev(Xt2)
    got = ce.ops.gnb_predict_proba(dev(Xt2), gnb.theta_, gnb.var_, gnb.class_prior_).cpu().numpy()
    want = ce.ops.gnb_predict_proba(Xpad[:, :260], gnb.theta_, gnb.var_, gnb.class_prior_).cpu().numpy()
    nan = np.isnan(want)  # NaN rows: NaN in both (the sign of a NaN is not a value)
    assert nan[0].all() and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan].view(np.uint64), want[~nan].view(np.uint64))


def test_frames_inference_to_selection(ce):
    """amg_test.py:426-445 with every step on the device: member inference over
    frames (GNB, SGD), per-song segment mean, stack with a song-level member,
    selection.  The selection equals the oracle's on the device's member
    probabilities (the exact part of the path); the members themselves are
    checked to tolerance above."""
    from conftest import fitted_members
    from oracle import ce_oracle as O
    from oracle.ce_oracle import ref_group_mean

    gnb, sgd, Xt = fitted_members(n_test=16_080)
    s_id = np.repeat(np.arange(1608) * 5, 10)
    Xd = dev(Xt)
    fr_gnb = ce.ops.gnb_predict_proba(Xd, gnb.theta_, gnb.var_, gnb.class_prior_)
    fr_sgd = ce.ops.sgd_predict_proba(Xd, sgd.coef_, sgd.intercept_)
    uniq, offsets, perm = ce.song_groups(s_id)
    assert perm is None
    rng = np.random.default_rng(5)
    cnn = rng.random((1608, 4)).astype(np.float32)
    stack = torch.empty((3, 1608, 4), dtype=torch.float64, device="cuda")
    ce.ops.segment_mean(fr_gnb, dev(offsets), out=stack[0])
    ce.ops.segment_mean(fr_sgd, dev(offsets), out=stack[1])
    stack[2] = dev(cnn).double()
    _, idx = ce.ops.select_mc(stack, 10, "MNC")
    P = np.array([ref_group_mean(fr_gnb.cpu().numpy(), s_id)[0], ref_group_mean(fr_sgd.cpu().numpy(), s_id)[0],
                  cnn])
    assert np.array_equal(stack.cpu().numpy(), P)
    assert np.array_equal(idx_np(idx), O.oracle_select_mc(P, 10, "MNC")[1])


@pytest.mark.parametrize("dt,C,M", [("f32", 4, 16), ("f32", 4, 32), ("bf16", 4, 32), ("bf16", 4, 64), ("f64", 4, 16),
                                    ("f32", 8, 8), ("f32", 8, 16)])
def test_lds_dma_stream_instantiations(ce, dt, C, M):
    """Every k_stream_nmc instantiation (item-major rows of 256 / 512 B staged
    by LDS-DMA) against the oracle, with a ragged tail (N not a multiple of
    64) and exact ties."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(M * 10 + C)
    N = 100_003
    P = synth(rng, N, M, C, np.float32, quant=32)
    if dt == "bf16":
        host = _bf16_bits(P)
        Pd = dev(host.view(np.int16)).view(torch.bfloat16)
    else:
        host = P.astype(np.float64) if dt == "f64" else P
        Pd = dev(host)
    exp = O.oracle_select_mc(host, 10, "NMC")[1]
    _, idx = ce.ops.select_mc(Pd, 10, "NMC")
    assert np.array_equal(idx_np(idx), exp)
    _, idx = ce.ops.select_mc(Pd, 64, "NMC")
    assert np.array_equal(idx_np(idx), O.oracle_select_mc(host, 64, "NMC")[1])


def test_gnb_widest_shape(ce):
    """GaussianNB at the ABI's limits (C = 8 classes, D = 512 features: 96 KB of
    theta / var / 1/var in LDS) against the restatement in all 64 bits, with
    variances spread over 12 decades (the reciprocal-corrected division).  The
    probabilities of this data are one-hot, so the joint log-likelihood itself
    (the scores of ce_gnb_score_users for one user owning every row) is held to
    members_eval_ref.gnb_jll as well: every term's quotient is in those bits."""
    from members_eval_ref import gnb_jll
    from oracle.ce_oracle import ref_gnb_predict_proba

    rng = np.random.default_rng(512)
    C, D = 8, 512
    theta = rng.normal(0, 1, (C, D))
    var = 10.0 ** rng.uniform(-6, 6, (C, D))
    prior = rng.dirichlet(np.ones(C))
    X = theta[rng.integers(0, C, 3000)] + rng.normal(0, 1, (3000, D)) * np.sqrt(var[0])
    got = ce.ops.gnb_predict_proba(dev(X), theta, var, prior).cpu().numpy()
    want = ref_gnb_predict_proba(X, theta, var, prior)
    assert not np.isnan(want).any()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    F = len(X)
    _, _, jll = ce.ops.gnb_score_users(dev(X), dev(theta[None]), dev(var[None]), dev(prior[None]),
                                       dev(np.array([0, 1], np.int64)), dev(np.array([0, F], np.int64)),
                                       dev(np.zeros(F, np.int32)), return_scores=True)
    assert np.array_equal(jll.cpu().numpy().view(np.uint64), gnb_jll(X, theta, var, prior).view(np.uint64))


@pytest.mark.parametrize("C,dt,N,chunk", [(4, "f32", 300_000, 50_000), (1000, "bf16", 6_000, 1_000),
                                          (4, "f64", 70_001, 9_999)])
def test_chunked_pool_vs_oracle(ce, C, dt, N, chunk):
    """ce_select_mc_chunk (pools larger than HBM, BASELINE configs[4]): >= 6
    chunks scored one at a time into a running top-q equal the oracle's
    selection over the whole pool.  Exact ties straddle every chunk boundary
    (the same rows repeated on both sides, the later copy must lose) and the
    pool is quantised so ties cross the q-th place."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(C + N)
    M = 32 if C == 1000 else 16
    P = synth(rng, N, M, C, np.float32, quant=None if C == 1000 else 16)
    for b in range(chunk, N, chunk):  # identical maximal-entropy rows on both sides of each boundary
        P[b - 2:b + 2] = 1.0 / C
    if dt == "bf16":
        host = _bf16_bits(P)
        Pd = dev(host.view(np.int16)).view(torch.bfloat16)
    else:
        host = P.astype(np.float64) if dt == "f64" else P
        Pd = dev(host)
    ent_o = O.oracle_committee_entropy(host, "NMC")
    for q in (10, 64):
        _, idx_o = O.oracle_topq(ent_o, q)
        job = ce.ops.MCChunkJob(q, "NMC")
        for lo in range(0, N, chunk):
            job.add(Pd[lo:lo + chunk])
        _, idx = job.result()
        assert np.array_equal(idx_np(idx), idx_o), q
    # chunks handed in out of order with explicit positions: same answer
    chunks = [(Pd[lo:lo + chunk], lo) for lo in range(0, N, chunk)][::-1]
    _, idx = ce.ops.select_mc_chunks(chunks, 10, "NMC")
    assert np.array_equal(idx_np(idx), O.oracle_topq(ent_o, 10)[1])


def _wide_order_pool(rng, order, N, M, C, chunk):
    """N x M x C f32 rows: item i has K_i classes near 1.0 and the rest near
    2^-10 (entropy grows with K_i), K_i rising / falling with the position, or
    rising and falling chunk by chunk; identical rows across each boundary."""
    k = 1 + (np.arange(N) * (C - 1)) // N
    if order == "falling":
        k = k[::-1]
    elif order == "mixed":
        k = np.concatenate([k[lo:lo + chunk][::(-1) ** (lo // chunk)] for lo in range(0, N, chunk)])
    base = np.where(np.arange(C)[None, :] < k[:, None], np.float32(1.0), np.float32(2.0 ** -10))
    P = rng.random((N, M, C), dtype=np.float32)
    P *= np.float32(0.05)
    P += np.float32(1.0)
    P *= base[:, None, :]
    for b in range(chunk, N, chunk):
        P[b - 1:b + 1] = P[b - 2]  # identical rows across each boundary: the earlier position wins
    return P


@pytest.mark.parametrize("order", ["rising", "falling", "mixed", "iid"])
def test_wide_floor_and_vote_orders(ce, order):
    """The wide stream's sampled floor + grid vote (k_wide_seed / k_wide_seed_pick:
    N / 16 (at most 4096) stratified samples' exact entropies give a floor -- better of their
    q-th and a chunked job's running q-th entry -- the vote sends the launch to
    the deep-ring grid when at most 1/16 of the samples would still be exact,
    else to the occupancy grid; both grids are launched, one exits) on pools
    whose entropies rise, fall or alternate with the position (and i.i.d.),
    10 x 1000 bf16 (20 KB items, >= 16384 items per launch so every launch takes
    the path): chunked jobs with ties on the boundaries and single selections
    equal the oracle, q in {1, 10, 64}."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng({"rising": 61, "falling": 62, "mixed": 63, "iid": 64}[order])
    N, M, C, chunk = 60_000, 10, 1000, 20_000
    if order == "iid":
        P = synth(rng, N, M, C, np.float32)
        for b in range(chunk, N, chunk):
            P[b - 1:b + 1] = P[b - 2]
    else:
        P = _wide_order_pool(rng, order, N, M, C, chunk)
    host = _bf16_bits(P)
    del P
    Pd = dev(host.view(np.int16)).view(torch.bfloat16)
    ent_o = O.oracle_committee_entropy(host, "NMC")
    for q in (1, 10, 64):
        _, idx_o = O.oracle_topq(ent_o, q)
        job = ce.ops.MCChunkJob(q, "NMC")
        for lo in range(0, N, chunk):
            job.add(Pd[lo:lo + chunk])
        _, idx = job.result()
        assert np.array_equal(idx_np(idx), idx_o), (order, q, "job")
        _, idx = ce.ops.select_mc(Pd, q, "NMC")
        assert np.array_equal(idx_np(idx), idx_o), (order, q, "single")


def test_wide_floor_records_shards(ce):
    """The multi-GPU records path on a wide pool (ce_select_mc_cands: every
    shard a folded wide launch with its own sampled floor + grid vote): three
    shards of a rising-entropy pool at their global offsets, their q records
    merged (ce_merge_cands), equal the oracle over the whole pool, q in {1, 10,
    64}; the shard holding the top items and the ones holding none both count."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(81)
    N, M, C, shard = 54_000, 10, 1000, 18_000
    host = _bf16_bits(_wide_order_pool(rng, "rising", N, M, C, shard))
    Pd = dev(host.view(np.int16)).view(torch.bfloat16)
    ent_o = O.oracle_committee_entropy(host, "NMC")
    for q in (1, 10, 64):
        recs = [ce.ops.MCPlan(Pd[lo:lo + shard], q, "NMC", base_idx=lo).step_cands() for lo in range(0, N, shard)]
        _, idx = ce.ops.merge_cands(torch.cat(recs).contiguous(), q)
        assert np.array_equal(idx_np(idx), O.oracle_topq(ent_o, q)[1]), q


def test_wide_floor_near_ties_and_exclusions(ce):
    """Pools the sampled floor cannot prune: near-uniform 1000-class rows whose
    entropies all lie within the approximation's margin of each other (every
    sample stays exact -> the vote picks the occupancy grid), with NaN rows
    (all-zero members) and exact duplicates; then the same pool with an
    exclusion bitmap covering sampled strata (ce_select_mc_excl, the session's
    path): excluded items never enter the floor nor the selection."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(71)
    N, M, C = 40_000, 10, 1000
    P = np.float32(0.5) + np.float32(1e-4) * rng.random((N, M, C), dtype=np.float32)
    k = rng.permutation(N)
    P[k[:3]] = 0.0            # NaN entropies: ranked first
    P[k[3:9]] = P[k[9]]       # exact duplicates
    host = _bf16_bits(P)
    del P
    Pd = dev(host.view(np.int16)).view(torch.bfloat16)
    ent_o = O.oracle_committee_entropy(host, "NMC")
    for q in (1, 10, 64):
        _, idx_o = O.oracle_topq(ent_o, q)
        _, idx = ce.ops.select_mc(Pd, q, "NMC")
        assert np.array_equal(idx_np(idx), idx_o), q
    # exclusions: every other 37-item run plus the NaN rows and the current top 64
    out = np.zeros(N, dtype=bool)
    out[(np.arange(N) // 37) % 2 == 0] = True
    out[k[:3]] = True
    out[O.oracle_topq(ent_o, 64)[1]] = True
    excl = ce.ops.excl_bitmap(N, device="cuda")
    ce.ops.mark_selected(excl, N, torch.from_numpy(np.flatnonzero(out)).cuda())
    ent_x = ent_o.copy()
    ent_x[out] = -np.inf
    for q in (1, 10, 64):
        _, idx = ce.ops.select_mc(Pd, q, "NMC", excl=excl)
        got = idx_np(idx)
        assert not out[got[got >= 0]].any(), q
        assert np.array_equal(got, O.oracle_topq(ent_x, q)[1]), q


@pytest.mark.parametrize("dt", ["f32", "bf16"])
def test_wide_prefilter_specials(ce, dt):
    """The wide stream's approximate prefilter (ce_wide.hpp: items whose f32
    approximate entropy is below the wave's threshold skip the exact entropy;
    a chunked job seeds the threshold with its running list): near-uniform
    1000-class rows (most far below the top, so skipped) with a cluster at the
    top whose entropies differ by far less than the approximation's error,
    exact duplicates across chunks, and rows the approximation does not
    cover -- all-zero (NaN entropy), negative, inf, sums far below / above
    2^+-100 -- in a chunked job and a single call, against the oracle."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(31 if dt == "f32" else 32)
    N, M, C, chunk = 12_000, 8, 1000, 2_000
    P = (-np.log(rng.random((N, M, C)))).astype(np.float32)  # spread entropies: most items are skipped
    k = rng.permutation(N)
    P[k[20:300]] = 0.5 + 0.01 * rng.random((280, M, C))  # a near-uniform cluster: entropies within ~1e-5
    P[k[0:6]] = P[k[6]]                       # exact duplicates (lowest position wins)
    P[k[7:10]] = 0.0                          # NaN entropies: ranked first
    P[k[10:12], 0, 5] = -1.0                  # a negative mean
    P[k[12:14], 1, 7] = np.inf
    P[k[14:16]] *= 1e-32                      # f32 sums below 2^-100
    P[k[16:18]] *= 1e30                       # f32 sums above 2^100
    if dt == "bf16":
        host = _bf16_bits(P)
        Pd = dev(host.view(np.int16)).view(torch.bfloat16)
    else:
        host = P
        Pd = dev(host)
    ent_o = O.oracle_committee_entropy(host, "NMC")
    for q in (1, 10, 64):
        _, idx_o = O.oracle_topq(ent_o, q)
        job = ce.ops.MCChunkJob(q, "NMC")
        for lo in range(0, N, chunk):
            job.add(Pd[lo:lo + chunk])
        _, idx = job.result()
        assert np.array_equal(idx_np(idx), idx_o), q
        _, idx = ce.ops.select_mc(Pd, q, "NMC")
        assert np.array_equal(idx_np(idx), idx_o), q


def test_c5_full_pool_chunk_invariance(ce):
    """BASELINE configs[4] at its FULL size (50M items x 32 x 1000 bf16, 3.2 TB,
    streamed as the bench streams it: device-generated 250K-item chunks): a
    size-independent property the oracle cannot afford at 3.2 TB -- the
    selection must not depend on where the chunk boundaries fall.  Job A adds
    every chunk whole, job B the same bytes as two 125K-item halves (twice as
    many boundaries, every running merge different); both must return the
    same positions and bit-identical entropies, and the same positions as a
    single-launch ce_select_mc over the chunk that holds the winner."""
    items, nc, M, C, q = 50_000_000, 250_000, 32, 1000, 10
    buf = torch.empty((nc, M, C), dtype=torch.bfloat16, device="cuda")
    ja, jb = ce.ops.MCChunkJob(q, "NMC"), ce.ops.MCChunkJob(q, "NMC")
    h = nc // 2
    for c in range(items // nc):
        lo = c * nc
        buf.uniform_(0.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(1987 * 100_003 + c))
        ja.add(buf, lo)
        jb.add(buf[:h], lo)
        jb.add(buf[h:], lo + h)
    va, ia = ja.result()
    vb, ib = jb.result()
    assert torch.equal(ia, ib) and torch.equal(va.view(torch.int64), vb.view(torch.int64))
    assert ia.min().item() >= 0 and ia.max().item() < items
    # the winner's own chunk, re-generated and selected in one launch, ranks it first
    c0 = int(ia[0].item()) // nc
    buf.uniform_(0.0, 1.0, generator=torch.Generator(device="cuda").manual_seed(1987 * 100_003 + c0))
    v1, i1 = ce.ops.select_mc(buf, q, "NMC", base_idx=c0 * nc)
    assert int(i1[0].item()) == int(ia[0].item())
    assert v1[0].view(torch.int64).item() == va[0].view(torch.int64).item()


def _bench_c5_child(lib, items, chunk, q):
    """tools/bench_c5.py in a child process on library build `lib` (None: the
    product library): the job's q positions and entropy bits."""
    import json
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    env.pop("CE_AMD_LIB", None)
    if lib:
        env["CE_AMD_LIB"] = lib
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "bench_c5.py"), "--items", str(items), "--chunk",
                        str(chunk), "--q", str(q), "--quiet"], cwd=root, capture_output=True, text=True, timeout=300,
                       env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    return line["selected"], line["entropy_bits"], line["frac_hbm"]


@pytest.mark.parametrize("items,q", [(50_000_000, 10), (12_000_000, 64)])
def test_c5_prefilter_pinned_full_size(ce, items, q):
    """The C5 job's approximate prefilter (an item whose f32 approximate entropy
    lies more than 2 * kWideApproxErr2 below the running threshold skips its
    exact entropy) pinned at full size against the exact path: the same
    device-generated 2M-item chunks (BASELINE configs[4]: 32 members x 1000
    bf16 classes; at 50M items the whole 3.2 TB pool) scored by the product
    library and by the build without the prefilter
    (tools/_diag/libce_amd_noprefilter.so, `make noprefilter`, built by
    __graft_entry__.build()) -- where nearly every item skips -- must give
    every one of the q positions and their entropy bits identically
    (amg_test.py:441-445)."""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exact_lib = os.path.join(root, "tools", "_diag", "libce_amd_noprefilter.so")
    assert os.path.exists(exact_lib), "build the exact-path reference first: make -C consensus-entropy_amd noprefilter"
    torch.cuda.synchronize()
    ce.ops.WORKSPACE.clear()  # the cached eager workspaces (empty_cache cannot free them)
    torch.cuda.empty_cache()  # the children need a 128 GB chunk each
    free, _ = torch.cuda.mem_get_info()
    need = 2_000_000 * 32 * 1000 * 2 + (8 << 30)  # one chunk + generation / workspace headroom
    if free < need:
        pytest.skip(f"{free / 2**30:.0f} GiB free on the device, a child needs {need / 2**30:.0f} GiB")
    sel_p, bits_p, frac_p = _bench_c5_child(None, items, 2_000_000, q)
    sel_e, bits_e, frac_e = _bench_c5_child(exact_lib, items, 2_000_000, q)
    assert len(sel_p) == q and min(sel_p) >= 0 and max(sel_p) < items
    assert sel_p == sel_e
    assert bits_p == bits_e
    print(f"items={items} q={q}: prefiltered {frac_p:.3f} vs exact path {frac_e:.3f} of HBM")
