"""The streaming kernel's ordered tile claims (k_stream_nmc on folded item-major
launches, csrc/ce_stream.hpp) against the oracle, on [N, 16, 4] f32 pools through
ops.MCPlan / ops.select_mc / ops.MCChunkJob.

Which wave scores a tile is decided at run time by a device counter, so every
test here checks the one thing that must not depend on it: the selection (the
total order NaN first, entropy descending, lowest position).  Sizes sit around
the unit grid: a unit is K adjacent 64-item tiles (K = 2, 4 or 8 by build), the
grid has W waves (4 per CU, one block per CU), so 64 K W items are exactly one
unit per wave.  Positions are compared exactly; entropies to 1e-12 relative
(a dozen f64 operations per item on either side, as smoke() allows).

A pool of <= 4096 items reaches the streaming kernel only through the record
outputs (step_cands / the chunked job); larger ones through step() as well.

The launcher claims only in large pools (CE_STREAM_CLAIM_MIN_ROUNDS tiles per
wave, csrc/ce_launch_stream.hip); ce_debug_stream_claims(500, 0) puts these small
pools on the claimed order, half of each pool claimed, and every test reads the
launcher's decision back (ce_debug_stream_claim_from) so that it knows which
order it checked."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

KERNEL = "ce::k_stream_nmc<0, 4, 16, 2, false, 2>"
HEADER_BYTES = 65536 + 256  # include/ce.h: the counter header (+ the alignment carve)
CLAIM_WORD = 16384 - 1      # csrc/ce_ws.hpp: kWsClaimSlot
M, C = 16, 4
QS = (1, 10, 64)
N_BIG = 1_000_003  # 15 tiles per wave on 1024 waves: the last 8 rounds are claimed


@pytest.fixture(scope="module")
def eng():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ctypes

    import ce_amd
    import ce_amd.ops as ops

    ce_amd.load()
    lib = ce_amd._lib.load()
    lib.ce_debug_stream_claims.argtypes = [ctypes.c_int64, ctypes.c_int64]
    lib.ce_debug_stream_claims.restype = None
    lib.ce_debug_stream_claim_from.argtypes = []
    lib.ce_debug_stream_claim_from.restype = ctypes.c_int64
    lib.ce_debug_stream_claims(500, 0)
    yield ops, lib
    lib.ce_debug_stream_claims(-1, -1)  # the build's share and gate again


def claimed(lib, n):
    """The last launch ran the kernel under test, on the claimed order wherever
    the pool reaches past the static rounds: the launcher's claim_from is
    max(4, rounds - ceil(rounds / 2)) at half the pool claimed."""
    assert lib.ce_last_kernel().decode() == KERNEL
    rounds = ((n + 63) // 64) // grid_waves(n)
    assert lib.ce_debug_stream_claim_from() == max(4, rounds - (rounds + 1) // 2)
    return (n + 63) // 64 > lib.ce_debug_stream_claim_from() * grid_waves(n)


def grid_waves(n):
    """Waves of the grid ce_launch_stream.hip launches for n items: one block
    (4 waves) per CU (two 16-KiB ring slots per wave fill the LDS), at most one
    block per 64 items and 1024 blocks."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return 4 * min(cus, min(1024, (n + 63) // 64))


# sizes: plain item counts, or (K, d) = 64 K W + d items, W read from the device when the test runs
SIZES = [1, 63, 64, 65, 200_001, 1_000_003] + [(k, d) for k in (2, 4, 8) for d in (-1, 0, 1)]


def items(size):
    return size if isinstance(size, int) else 64 * size[0] * grid_waves(1 << 30) + size[1]


def max_items():
    return max(items(s) for s in SIZES)


_POOLS = {}


def pools():
    """Two host pools of the largest size and their oracle entropies, made once:
    `tied` (small-integer rows: the top is a flood of exact ties, so the lowest
    positions must win) and `smooth` (Dirichlet rows, 1 % un-normalised); every
    test slices a prefix."""
    if not _POOLS:
        from oracle import ce_oracle as O

        n = max_items()
        rng = np.random.default_rng(1987)
        tied = (rng.integers(1, 9, size=(n, M, C)) / 32.0).astype(np.float32)
        e = -np.log(rng.random((n, M, C)))
        smooth = (e / e.sum(-1, keepdims=True)).astype(np.float32)
        smooth[rng.random(n) < 0.01] *= np.float32(1.5)
        for name, P in (("tied", tied), ("smooth", smooth)):
            _POOLS[name] = (P, O.oracle_committee_entropy(P, "NMC"), torch.from_numpy(P).cuda())
    return _POOLS


def header_is_zero(ws):
    """The 16384 counters at the workspace's 256-aligned base (csrc/ce_ws.hpp:
    ws_base, kWsHeader), the claim word among them."""
    off = -ws.data_ptr() % 256
    h = ws[off:off + 65536].view(torch.int32)
    return int(h[CLAIM_WORD]) == 0 and not bool(h.any())


def expect(ent, q, base=0):
    from oracle import ce_oracle as O

    return O.oracle_topq(ent, q, base)


def check(vals, idx, ent, q, base=0):
    vo, io = expect(ent, q, base)
    got_i, got_v = idx.cpu().numpy(), vals.cpu().numpy()
    k = len(io)
    assert np.array_equal(got_i[:k], io), (got_i, io)
    assert (got_i[k:] == -1).all()
    np.testing.assert_allclose(got_v[:k], vo, rtol=1e-12, atol=0)


@pytest.mark.parametrize("q", QS)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: str(s).replace(" ", ""))
def test_sizes_around_the_unit_grid(eng, size, q):
    ops, lib = eng
    n = items(size)
    name = "smooth" if n in (200_001, N_BIG) else "tied"
    _, ent, Pd = pools()[name]
    plan = ops.MCPlan(Pd[:n], q, "NMC")
    rec = plan.step_cands()
    assert claimed(lib, n) == (n > 64 * 4 * grid_waves(n))
    check(*ops.merge_cands(rec, q), ent[:n], q)
    assert header_is_zero(plan.ws)
    if n > 4096:  # the final outputs of a larger pool come from the same kernel
        vals, idx = plan.step()
        assert claimed(lib, n) == (n > 64 * 4 * grid_waves(n))
        check(vals, idx, ent[:n], q)
        assert header_is_zero(plan.ws)


def test_base_idx_beyond_32_bits(eng):
    ops, lib = eng
    _, ent, Pd = pools()["smooth"]
    n, base = N_BIG, 12_345_678_901
    plan = ops.MCPlan(Pd[:n], 10, "NMC", base_idx=base)
    vals, idx = plan.step()
    assert claimed(lib, n)
    check(vals, idx, ent[:n], 10, base)
    assert header_is_zero(plan.ws)


@pytest.mark.parametrize("name", ["smooth", "tied"])
def test_exclusion_of_the_whole_top_q(eng, name):
    """The bitmap takes out the true top-q: the next q must come back."""
    ops, lib = eng
    _, ent, Pd = pools()[name]
    n, q = N_BIG, 10
    _, top = expect(ent[:n], 2 * q)
    excl = ops.excl_bitmap(n, Pd.device)
    ops.mark_selected(excl, n, torch.from_numpy(top[:q].copy()).cuda())
    vals, idx = ops.select_mc(Pd[:n], q, "NMC", excl=excl)
    assert claimed(lib, n)
    assert header_is_zero(ops.WORKSPACE.get(Pd.device, 65536 + 256))
    assert np.array_equal(idx.cpu().numpy(), top[q:])
    np.testing.assert_allclose(vals.cpu().numpy(), ent[top[q:]], rtol=1e-12, atol=0)


@pytest.mark.parametrize("q", [10, 64])
def test_tie_flood_takes_the_lowest_positions(eng, q):
    """Every row equal: the q lowest positions win, whichever waves scored them."""
    ops, lib = eng
    n = 64 * 8 * grid_waves(1 << 30) + 1
    P = torch.full((n, M, C), 0.25, dtype=torch.float32, device="cuda")
    plan = ops.MCPlan(P, q, "NMC", base_idx=7)
    _, idx = plan.step()
    assert claimed(lib, n)
    assert torch.equal(idx.cpu(), torch.arange(7, 7 + q))
    assert header_is_zero(plan.ws)


def test_nan_rows_come_first(eng):
    ops, lib = eng
    from oracle import ce_oracle as O

    P, _, _ = pools()["smooth"]
    n = N_BIG
    P = P[:n].copy()
    for i in (0, 63, 64, 800_063, 800_064, n - 1):  # tile edges, deep in the pool, the short last tile
        P[i, 3, 1] = np.nan
    ent = O.oracle_committee_entropy(P, "NMC")
    plan = ops.MCPlan(torch.from_numpy(P).cuda(), 10, "NMC")
    vals, idx = plan.step()
    assert claimed(lib, n)
    assert header_is_zero(plan.ws)
    _, io = expect(ent, 10)
    got = idx.cpu().numpy()
    assert np.array_equal(got, io), (got, io)
    assert np.array_equal(got[:6], [0, 63, 64, 800_063, 800_064, n - 1])
    assert np.isnan(vals.cpu().numpy()[:6]).all()


def test_step_cands_records(eng):
    """The record output: {order key, position} per slot, best first; merged, it
    is step()'s answer."""
    ops, lib = eng
    _, ent, Pd = pools()["smooth"]
    n, q = N_BIG, 10
    plan = ops.MCPlan(Pd[:n], q, "NMC", base_idx=1000)
    rec = plan.step_cands()
    assert claimed(lib, n)
    assert header_is_zero(plan.ws)
    vo, io = expect(ent[:n], q, 1000)
    assert np.array_equal(rec.cpu().numpy()[:, 1], io)
    keys = rec.cpu().numpy()[:, 0].astype(np.uint64)
    assert (keys[:-1] >= keys[1:]).all()  # best first: the order key descends
    mv, mi = ops.merge_cands(rec, q)
    sv, si = plan.step()
    assert torch.equal(mi, si) and torch.equal(mv, sv)


def test_chunked_job_second_chunk(eng):
    """Two chunks on one cached workspace: the second launch merges the running
    list (`extra`) and finds the claim word reset by the first."""
    ops, lib = eng
    _, ent, Pd = pools()["tied"]
    n0, n1, q = 400_001, 600_001, 10
    job = ops.MCChunkJob(q, "NMC")
    job.add(Pd[:n0])
    assert claimed(lib, n0)
    job.add(Pd[n0:n0 + n1])
    assert claimed(lib, n1)
    check(*job.result(), ent[:n0 + n1], q)
    ws = ops.WORKSPACE.get(Pd.device, HEADER_BYTES)
    assert header_is_zero(ws)


def test_three_launches_on_one_workspace(eng):
    ops, lib = eng
    _, ent, Pd = pools()["smooth"]
    n = 64 * 8 * grid_waves(1 << 30) + 1
    plan = ops.MCPlan(Pd[:n], 10, "NMC")
    outs = []
    for _ in range(3):
        vals, idx = plan.step()
        outs.append((vals.clone(), idx.clone()))
        assert header_is_zero(plan.ws)
    assert claimed(lib, n)
    for v, i in outs[1:]:
        assert torch.equal(i, outs[0][1]) and torch.equal(v, outs[0][0])
    check(*outs[0], ent[:n], 10)


def test_shipped_share_and_gate(eng):
    """The build's own share and size gate on a pool large enough to claim (20M
    items, 305 tiles per wave on 1024 waves): the launcher claims, and the answer
    is the one the static order gives on the same pool (share 0: the loop the
    other tests of the suite check against the oracle)."""
    ops, lib = eng
    n = 20_000_003
    g = torch.Generator(device="cuda").manual_seed(7)
    P = torch.rand((n, M, C), device="cuda", generator=g)
    plan = ops.MCPlan(P, 10, "NMC")
    try:
        lib.ce_debug_stream_claims(-1, -1)
        vals, idx = (x.clone() for x in plan.step())
        assert lib.ce_last_kernel().decode() == KERNEL
        r = lib.ce_debug_stream_claim_from()
        assert 4 <= r < ((n + 63) // 64) // grid_waves(n)
        assert header_is_zero(plan.ws)
        lib.ce_debug_stream_claims(0, 0)
        sv, si = plan.step()
        assert lib.ce_debug_stream_claim_from() == 0
        assert torch.equal(idx, si) and torch.equal(vals, sv)
    finally:
        lib.ce_debug_stream_claims(500, 0)
