"""GPU parity of the human-consensus (hc) half of the engine at every class
count, row pitch and edge: the vote and valence/arousal table kernels (k_vote<C>,
k_va), the hc selection (a one-member f64 committee: the register kernels for
C in {2, 3, 4, 8}, the wide kernels' n < 8 leaf for C in {1, 5, 6, 7}) and the
hc segment of the mix (k_partial<TableSrc<C>>), against the CPU oracle, which
tests/test_hc_tables.py pins to numpy / scipy on the same inputs.

Bar: bit for bit, the project's own (ENT_TOL_ULP = 0 in test_gpu_parity.py).
f64 results are compared as uint64 views (-0.0 is not +0.0); a NaN equals any
NaN (a row without a valid vote is 0/0).
"""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

LATTICE_N = list(range(1, 257)) + [500, 665, 1000, 2000]
LATTICE_A = 2000
VA_SPECIALS = np.array([np.nan, -np.inf, -1.0, -5e-324, -0.0, 0.0, 5e-324, 1.0, np.inf])


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


def host(t):
    return t.cpu().numpy()


def assert_bits(got, exp, what=""):
    """Equal bit for bit: NaN equals any NaN, -0.0 differs from +0.0."""
    got = np.ascontiguousarray(got, np.float64)
    exp = np.ascontiguousarray(exp, np.float64)
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    nan_g, nan_e = np.isnan(got), np.isnan(exp)
    assert np.array_equal(nan_g, nan_e), (what, "NaN pattern", np.argwhere(nan_g != nan_e)[:5].tolist())
    bad = (got.view(np.uint64) != exp.view(np.uint64)) & ~nan_e
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5].tolist(), got[bad][:5], exp[bad][:5])


def assert_selection(vals, idx, want_vals, want_idx, what=""):
    """(vals, idx) of a q-slot selection equal the oracle's list, then padding."""
    vals, idx = host(vals), host(idx)
    n = len(want_idx)
    assert np.array_equal(idx[:n], want_idx), (what, idx[:8], want_idx[:8])
    assert (idx[n:] == -1).all(), what
    assert_bits(vals[:n], want_vals, what)


def last_kernel(ce):
    return ce._lib.load().ce_last_kernel().decode()


def planted_votes(rng, N, A, C):
    """Votes in [-1, C] (C itself is out of range: a missing vote) with a row of
    no vote, a row of 127, a row of -128 and a unanimous row."""
    v = rng.integers(-1, C + 1, size=(N, A)).astype(np.int8)
    v[3], v[70], v[129], v[200] = -1, 127, -128, C - 1
    return v


@pytest.fixture(scope="module")
def lattice():
    """Every (c, n), 0 <= c <= n, n in LATTICE_N, as C = 2 vote rows (c votes of
    class 0, n - c of class 1, then -1 up to A = 2000), the oracle's table of
    them, and the rows where rint(x * 1000) rounds an exact tie."""
    from oracle import ce_oracle as O

    n = np.concatenate([np.full(k + 1, k) for k in LATTICE_N])
    c = np.concatenate([np.arange(k + 1) for k in LATTICE_N])
    col = np.arange(LATTICE_A)[None, :]
    votes = np.where(col < c[:, None], np.int8(0), np.where(col < n[:, None], np.int8(1), np.int8(-1)))
    t0, t1 = c / n * 1000.0, (n - c) / n * 1000.0
    halves = (t0 - np.floor(t0) == 0.5) | (t1 - np.floor(t1) == 0.5)
    freq, ent = O.oracle_vote_table(votes, 2)
    return votes, freq, ent, halves


# ---------------------------------------------------------------------------
# k_vote
# ---------------------------------------------------------------------------
def test_vote_count_lattice(ce, lattice):
    """k_vote<2> and round3 (ce_device.hpp) over the whole (count, n) lattice,
    n in 1..256 and {500, 665, 1000, 2000}: 37,321 rows, >= 1,000 of them exact
    ties of rint(x * 1000).  More rows than the 8192 blocks x 4 waves of the
    launch, so the grid-stride loop of the table kernels wraps."""
    votes, freq_o, ent_o, halves = lattice
    N = votes.shape[0]
    assert N == 37321 and N > 8192 * 4  # the wrap
    assert int(halves.sum()) >= 1000
    freq, ent = ce.ops.vote_table(dev(votes), C=2)
    freq, ent = host(freq), host(ent)
    assert_bits(freq[~halves], freq_o[~halves], "freq off the ties")
    assert_bits(freq[halves], freq_o[halves], "freq on the exact ties")
    assert_bits(ent, ent_o, "ent")


@pytest.mark.parametrize("C", range(1, 9))
def test_vote_every_class_count(ce, C):
    """k_vote<C> (and entropy_row<C>) for every instantiated C = 1..8 at
    annotator counts around the 64-lane loop, A in {1, 63, 64, 65, 130}, N = 257
    (a last block of one wave): votes in [-1, C] with a row of no vote, of 127,
    of -128 (bytes outside [0, C) count for nothing; 0/0 rows are NaN) and a
    unanimous row."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(1000 + C)
    for A in (1, 63, 64, 65, 130):
        v = planted_votes(rng, 257, A, C)
        fo, eo = O.oracle_vote_table(v, C)
        assert np.isnan(eo[[3, 70, 129]]).all() and eo[200] == 0.0
        freq, ent = ce.ops.vote_table(dev(v), C=C)
        assert_bits(host(freq), fo, ("freq", C, A))
        assert_bits(host(ent), eo, ("ent", C, A))


@pytest.mark.parametrize("C", range(1, 9))
def test_vote_row_pitch(ce, C):
    """k_vote<C> on a column slice of a wider matrix: votes = big[:, 3:68] of an
    [N, 77] int8 tensor, so the row pitch is ld = 77 > A = 65 and the base
    address is odd.  The columns outside the slice hold valid votes: a kernel
    stepping rows by A, or reading past A, counts them."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(2000 + C)
    N = 257
    big = rng.integers(0, C, size=(N, 77)).astype(np.int8)
    big[:, 3:68] = planted_votes(rng, N, 65, C)
    view = dev(big)[:, 3:68]
    assert view.stride() == (77, 1) and view.data_ptr() % 2 == 1
    fo, eo = O.oracle_vote_table(big[:, 3:68].copy(), C)
    freq, ent = ce.ops.vote_table(view, C=C)
    assert_bits(host(freq), fo, ("freq", C))
    assert_bits(host(ent), eo, ("ent", C))


def test_vote_degenerate_shapes(ce):
    """ce_vote_entropy at the edges of its arguments: no annotator (A = 0: every
    row 0/0, NaN), no row (N = 0: empty outputs, nothing launched), class counts
    outside k_vote<1..8>, a row pitch below A, and no frequency output
    (freq_or_null = NULL) -- the entropies are those of the call with a table."""
    from oracle import ce_oracle as O

    freq, ent = ce.ops.vote_table(torch.empty((5, 0), dtype=torch.int8, device="cuda"), C=3)
    assert tuple(freq.shape) == (5, 3) and tuple(ent.shape) == (5,)
    assert np.isnan(host(freq)).all() and np.isnan(host(ent)).all()
    freq, ent = ce.ops.vote_table(torch.empty((0, 7), dtype=torch.int8, device="cuda"), C=3)
    assert tuple(freq.shape) == (0, 3) and tuple(ent.shape) == (0,)
    rng = np.random.default_rng(5)
    v = planted_votes(rng, 257, 65, 4)
    vd = dev(v)
    for C in (0, 9):
        with pytest.raises(ce.CEError, match="C="):
            ce.ops.vote_table(vd, C=C)
    with pytest.raises(ce.CEError, match="ld="):
        ce.ops.vote_table(vd[0].expand(257, 65), C=4)  # stride(0) == 0: ld < A
    # through the binding, without a table
    lib = ce._lib.load()
    ent = torch.full((257,), -1.0, dtype=torch.float64, device="cuda")
    rc = lib.ce_vote_entropy(ctypes.c_void_p(vd.data_ptr()), 257, 65, 4, 65, None, ctypes.c_void_p(ent.data_ptr()),
                             ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, lib.ce_last_error()
    _, ent_t = ce.ops.vote_table(vd, C=4)
    assert_bits(host(ent), host(ent_t), "ent without a table")
    assert_bits(host(ent), O.oracle_vote_table(v, 4)[1], "ent vs oracle")


# ---------------------------------------------------------------------------
# k_va
# ---------------------------------------------------------------------------
def special_va(rng, N, A):
    """[N, A, 2] (valence, arousal) drawn from NaN, +-inf, +-1, +-denormal,
    +-0.0 and uniform(-1, 1); row 1 all NaN, row 2 NaN valences only, row 4
    NaN arousals only (half-NaN pairs are dropped votes too)."""
    pick = rng.integers(0, len(VA_SPECIALS) + 1, size=(N, A, 2))
    va = np.where(pick < len(VA_SPECIALS), VA_SPECIALS[np.minimum(pick, len(VA_SPECIALS) - 1)],
                  rng.uniform(-1.0, 1.0, size=(N, A, 2)))
    va[1] = np.nan
    va[2, :, 0] = np.nan
    va[4, :, 1] = np.nan
    return np.ascontiguousarray(va, np.float64)


def test_va_edges_and_wrap(ce):
    """k_va (quadrant + finish_counts<4>) on NaN, +-inf, +-denormal and signed
    zeros: N = 33,000 rows of A = 3 (more rows than 8192 blocks x 4 waves: the
    grid-stride loop wraps), then A in {1, 63, 64, 65} around the 64-lane loop
    at N = 64, with all-NaN rows and half-NaN pairs."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(33)
    assert 33_000 > 8192 * 4  # the wrap
    for N, A in ((33_000, 3), (64, 1), (64, 63), (64, 64), (64, 65)):
        va = special_va(rng, N, A)
        fo, eo = O.oracle_va_table(va)
        assert np.isnan(eo[[1, 2, 4]]).all()
        freq, ent = ce.ops.va_table(dev(va))
        assert_bits(host(freq), fo, ("freq", N, A))
        assert_bits(host(ent), eo, ("ent", N, A))


def test_va_alignment_is_loud(ce):
    """k_va reads (valence, arousal) as one 16-byte load: ce_va_entropy refuses
    an array whose base is 8 mod 16 by name instead of returning a table."""
    N, A = 64, 3
    flat = torch.zeros(N * A * 2 + 1, dtype=torch.float64, device="cuda")
    view = flat[1:].view(N, A, 2)
    assert view.is_contiguous() and view.data_ptr() % 16 == 8
    with pytest.raises(ce.CEError, match="16-byte aligned"):
        ce.ops.va_table(view)


# ---------------------------------------------------------------------------
# hc selection and the hc segment of the mix
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("C", range(1, 9))
def test_hc_select_every_class_count(ce, C):
    """select_queries('hc', votes=..., n_classes=C): k_vote<C>, then the table as
    a one-member f64 committee [N_h, 1, C].  C in {2, 3, 4, 8} stays on the
    register kernels; C in {1, 5, 6, 7} is the first run of the wide kernels'
    n < 8 leaf (wave_row_sum, ce_wide.hpp): k_stream_wide / k_stream_wide2 at
    q = 10, k_partial_wide at q = 65, k_wide_entropy_v + the sort at q = 2049.
    N_h = 5000 with 1 % rows of no vote: their NaN entropies rank first, lowest
    index first."""
    from ce_amd import select_queries
    from oracle import ce_oracle as O

    rng = np.random.default_rng(3000 + C)
    N_h = 5000
    v = rng.integers(-1, C, size=(N_h, 30)).astype(np.int8)
    empty = np.sort(rng.choice(N_h, 50, replace=False))
    v[empty] = -1
    ent_o = O.oracle_table_entropy(O.oracle_vote_table(v, C)[0])
    assert np.array_equal(np.flatnonzero(np.isnan(ent_o)), empty)
    for q in (10, 65, 2049):
        got = select_queries("hc", q, votes=v, n_classes=C)
        assert np.array_equal(got, O.canonical_order(ent_o, q)), (C, q)
        assert np.array_equal(got[:min(q, 50)], empty[:q]), (C, q)  # the NaN rows, in index order
        if q == 10 and C in (1, 5, 6, 7):
            want = "ce::k_stream_wide2<" if C == 6 else "ce::k_stream_wide<"  # 48-byte f64 rows take vector loads
            assert last_kernel(ce).startswith(want), last_kernel(ce)


def _bf16_bits(P32):
    """float32 -> bf16 bit patterns (round to nearest even), as uint16."""
    u = P32.astype(np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return u.astype(np.uint16)


@pytest.mark.parametrize("C", [1, 5, 6, 7])
def test_small_class_counts_on_the_wide_path(ce, C):
    """Committees of C in {1, 5, 6, 7} classes have no register kernel: they run
    on the wide kernels, whose row sums take the n < 8 leaf of numpy's pairwise
    sum (wave_row_sum, ce_wide.hpp: sequential, no 8-lane tree).  M in {1, 3, 4}
    (one member, an odd count, a power of two), f32 / f64 / bf16, both layouts,
    N = 3001: k_wide_entropy_v per item and the q = 10 stream.  C = 6 f64 rows
    are 48 bytes and take the vector loads (wide_vec_ok); C = 5 and 7 do not.
    Rows of zeros, of -0.0, with a NaN and with a negative member are planted."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(4000 + C)
    N = 3001
    seen = set()
    for M in (1, 3, 4):
        e = -np.log(rng.random((N, M, C)))
        P = e / e.sum(-1, keepdims=True)
        P[rng.random((N, M)) < 0.01] *= 1.7  # unnormalised members
        P[11] = 0.0
        P[12] = -0.0
        P[13, 0, 0] = np.nan
        P[14, M - 1, C - 1] = -0.05
        for dt in ("f32", "f64", "bf16"):
            if dt == "bf16":
                hostP = _bf16_bits(P)
                Pd = dev(hostP.view(np.int16)).view(torch.bfloat16)
            else:
                hostP = P.astype(np.float32 if dt == "f32" else np.float64)
                Pd = dev(hostP)
            ent_o = O.oracle_committee_entropy(hostP, "NMC")
            vo, io = O.oracle_topq(ent_o, 10)
            for layout in ("NMC", "MNC"):
                T = Pd if layout == "NMC" else Pd.permute(1, 0, 2).contiguous()
                assert_bits(host(ce.ops.committee_entropy(T, layout)), ent_o, ("ent", C, M, dt, layout))
                vals, idx = ce.ops.select_mc(T, 10, layout)
                k = last_kernel(ce)
                assert k.startswith("ce::k_stream_wide"), k
                seen.add(k.split("<")[0])
                assert_selection(vals, idx, vo, io, ("select", C, M, dt, layout))
    assert seen == ({"ce::k_stream_wide", "ce::k_stream_wide2"} if C == 6 else {"ce::k_stream_wide"}), seen


def mix_inputs(rng, N, N_h, M, C, dtype):
    """A committee [M, N, C] and an hc table [N_h, C] of rounded frequencies with
    NaN rows (no vote) and rows of the uniform distribution (the maximal
    entropy, tied) planted."""
    e = -np.log(rng.random((M, N, C)))
    P = (e / e.sum(-1, keepdims=True)).astype(dtype)
    H = np.round(rng.dirichlet(np.ones(C), N_h), 3)
    k = rng.permutation(N_h)
    H[k[:7]] = np.nan
    H[k[7:20]] = 1.0 / C
    return P, np.ascontiguousarray(H)


def table_forms(H):
    """The hc table contiguous (ld_hc = C) and as columns 1..C of an
    [N_h, C + 3] tensor whose outer columns hold 0.5 (ld_hc = C + 3: a kernel
    reading the wrong pitch or width gets other entropies)."""
    N_h, C = H.shape
    wide = np.full((N_h, C + 3), 0.5)
    wide[:, 1:1 + C] = H
    sl = dev(wide)[:, 1:1 + C]
    assert sl.stride() == (C + 3, 1)
    return (("contiguous", dev(H)), ("pitched", sl))


@pytest.mark.parametrize("N,N_h", [(1608, 1300), (5000, 4500)])
@pytest.mark.parametrize("C", [2, 3, 4, 8])
def test_mix_every_table_class_count(ce, C, N, N_h):
    """select_mix with the hc table at C in {2, 3, 4, 8}, contiguous and with
    ld_hc = C + 3: q = 10 is the one-block k_select_tiles (C = 4 at 1608 + 1300)
    or the stream over the table as a one-member committee, q = 65 is
    k_partial<TableSrc<C>> (partial_table, ce_launch_partial.hip -- no streaming
    kernel is noted), q = 2049 the entropies + sort.  (5000, 4500) is past
    kSmallPoolItems for every C.  The order is the oracle's total order over the
    concatenated entropies [mc; hc], values bit for bit."""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(5000 + 10 * C + (N > 2000))
    P, H = mix_inputs(rng, N, N_h, 4, C, np.float32)
    Pd = dev(P)
    for q in (10, 65, 2049):
        vo, io = O.oracle_select_mix(P, H, q)
        assert len(io) == q and (io[:7] >= N).all()  # the table's NaN rows lead
        for form, Hd in table_forms(H):
            vals, idx = ce.ops.select_mix(Pd, Hd, q)
            k = last_kernel(ce)
            assert_selection(vals, idx, vo, io, (C, N, q, form))
            if q == 65:
                assert k == "", k  # neither the stream nor the tiles: the block lists of k_partial
            if q == 10 and C == 4 and N == 1608:
                assert k.startswith("ce::k_select_tiles<"), k


@pytest.mark.parametrize("C", [1, 5, 6, 7])
def test_mix_unsupported_class_counts_are_consistent(ce, C):
    """select_mix at class counts without a TableSrc<C> (C in {1, 5, 6, 7}): the
    hc table is a one-member f64 committee on the wide kernels for every q --
    the stream at q = 10, k_partial_wide at q = 65 (the fallback of
    ce_select_mix when partial_table has no kernel), k_wide_entropy_v + the
    sort at q = 2049 -- so every q answers, and each is the oracle's selection.
    (Before the fallback q = 10 and q = 2049 answered and q = 65 raised
    'mix with C=%d has no kernel in this build'.)"""
    from oracle import ce_oracle as O

    rng = np.random.default_rng(6000 + C)
    N, N_h = 3001, 2500
    P, H = mix_inputs(rng, N, N_h, 3, C, np.float64)
    Pd = dev(P)
    outcome = {}
    for q in (10, 65, 2049):
        vo, io = O.oracle_select_mix(P, H, q)
        for form, Hd in table_forms(H):
            try:
                vals, idx = ce.ops.select_mix(Pd, Hd, q)
            except ce.CEError as e:
                outcome[q, form] = f"CEError: {e}"
                continue
            assert_selection(vals, idx, vo, io, (C, q, form))
            outcome[q, form] = "exact"
    assert set(outcome.values()) == {"exact"}, outcome
