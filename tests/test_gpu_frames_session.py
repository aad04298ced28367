"""Sessions over frame-level members on the GPU: the exclusion bitmap inside the
fused frames kernels (ce_select_frames_excl), the consensus rows
(ce_frames_consensus), SelectionSession(s_id=) and
BatchedSelectionSession(frame_offsets=).

The oracle, the same everywhere: per-song means by oracle.ce_oracle.ref_group_mean
(pandas 1.1.5 group_mean), the stack np.array(pred_prob), the consensus rows
np.mean(stack, axis=0), selection with exclusion = oracle_select_mc on the kept
columns with positions mapped back through np.flatnonzero(keep).  A song's mean
depends only on its own frames and sorted order survives a subset, so this is
the reference's groupby on the shrunken X_train.  Comparisons are bit equality."""
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from test_gpu_batched_session import (_graph_counts, assert_same, bitmap, dev, pad, shrinking_mix_reference,
                                      shrinking_reference)

pytestmark = pytest.mark.gpu

DMA_FORCED = os.environ.get("CE_AMD_FRAMES_DMA") == "1"  # the child run of test_tile_flavour_in_a_child_process


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def frame_pool(rng, N, C, grouped, nan_song=None, lo=1, hi=10, nan_cells=0.01):
    """N songs of lo..hi-1 frames: (s_id [F], members [f64 frames, f32 frames,
    f32 song-level], the reference's stack np.array(pred_prob) [3, N, C]).
    nan_song: a song whose frames are all NaN in the f32 frame member."""
    from oracle.ce_oracle import ref_group_mean

    ids = np.arange(N) * 3 + 5
    s_id = np.repeat(ids, rng.integers(lo, hi, N))
    if not grouped:
        s_id = rng.permutation(s_id)
    F = len(s_id)
    frames = []
    for dt in (np.float64, np.float32):
        e = -np.log(rng.random((F, C)))
        fm = e / e.sum(-1, keepdims=True)
        if nan_cells:
            fm[rng.random((F, C)) < nan_cells] = np.nan
        frames.append(fm.astype(dt))
    if nan_song is not None:
        frames[1][s_id == ids[nan_song]] = np.nan
    song = rng.random((N, C)).astype(np.float32)
    members = frames + [song]
    P = np.array([ref_group_mean(m, s_id)[0] for m in frames] + [song])
    return s_id, members, P


def expected(P, mask, q, base_idx=0):
    """oracle_select_mc on the kept columns, positions mapped back; padded to q slots."""
    from oracle import ce_oracle as O

    pos = np.flatnonzero(~mask)
    if len(pos) == 0 or q == 0:
        return pad(np.zeros(0), np.zeros(0, np.int64), q)
    v, i = O.oracle_select_mc(np.ascontiguousarray(P[:, pos]), q, "MNC")
    return pad(v, pos[i] + base_idx, q)


def bitmaps(rng, N, C, nan_song):
    """name -> bool [N], True = excluded"""
    G = 64 if C == 3 else 64 // C  # songs per wave step
    out = {"clear": np.zeros(N, bool), "all": np.ones(N, bool)}
    m = np.ones(N, bool)
    m[N // 2] = False
    out["all_but_one"] = m
    for name, a, n in (("word", 32 if N >= 64 else 0, 32), ("wave_step", G if N >= 2 * G else 0, G),
                       ("block_step", 4 * G if N >= 8 * G else 0, 4 * G)):
        m = np.zeros(N, bool)
        m[a:a + n] = True
        out[name] = m
    out["alternating"] = np.arange(N) % 2 == 0
    m = np.zeros(N, bool)
    m[[0, N - 1]] = True
    out["first_last"] = m
    out["random30"] = rng.random(N) < 0.3
    m = np.zeros(N, bool)
    m[nan_song] = True
    out["nan_song"] = m
    return out


def geometry(ce, s_id):
    uniq, offsets, perm = ce.song_groups(s_id)
    return len(uniq), dev(offsets), dev(perm) if perm is not None else None


SIZES = [1, 31, 32, 33, 63, 64, 65, 900, 2500]


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("C", [4, 3, 8, 2])
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_select_frames_excl_vs_oracle(ce, order, C, N):
    """ops.select_frames(excl=) on every route (q <= 64 fused, the lists over
    the entropies, the sort path) against the oracle on the kept songs."""
    ops, lib = ce.ops, ce._lib.load()
    rng = np.random.default_rng(1000 * C + N + (order == "grouped"))
    nan_song = N // 3
    s_id, members, P = frame_pool(rng, N, C, order == "grouped", nan_song)
    n, off, perm = geometry(ce, s_id)
    assert n == N
    md = [dev(m) for m in members]
    sl = [False, False, True]
    for name, mask in bitmaps(rng, N, C, nan_song).items():
        ex = bitmap(mask)
        for q in (1, 10, 64) + ((65, 2049) if N == 2500 else ()):
            v, i = ops.select_frames(md, off, q, perm=perm, song_level=sl, excl=ex)
            if q <= 64:
                want = "ce::k_frames_select_excl<3>" if C == 3 else "ce::k_frames_lanes_excl<%d, %s, false>" % (
                    C, "true" if DMA_FORCED and order == "grouped" else "false")
                assert lib.ce_last_kernel().decode() == want
            ev, ei = expected(P, mask, q)
            assert_same(v, i, ev, ei, (name, q))
            if name == "clear":  # the bitmap costs nothing in values: the plain kernels' answer
                v0, i0 = ops.select_frames(md, off, q, perm=perm, song_level=sl)
                assert_same(v, i, v0.cpu().numpy(), i0.cpu().numpy(), ("clear == no bitmap", q))
            if name == "random30" and q == 10:  # bits index the song n, positions are n + base_idx
                v, i = ops.select_frames(md, off, q, perm=perm, song_level=sl, excl=ex, base_idx=1000)
                assert_same(v, i, *expected(P, mask, q, 1000), ("base_idx", q))
    # the song whose f32 frames are all NaN has a NaN entropy, which ranks before every number: it is
    # among the first while it is in the pool and must not leak once excluded
    from oracle import ce_oracle as O

    assert np.isnan(O.oracle_committee_entropy(P, "MNC")[nan_song])
    nans = int(np.isnan(O.oracle_committee_entropy(P, "MNC")).sum())
    if nans <= 64:
        assert nan_song in expected(P, np.zeros(N, bool), 64)[1][:nans]
        _, i = ops.select_frames(md, off, 64, perm=perm, song_level=sl, excl=bitmap(np.arange(N) == nan_song))
        assert nan_song not in i.cpu().numpy()


@pytest.mark.parametrize("N", [1, 33, 65, 900])
@pytest.mark.parametrize("C", [4, 3, 8, 2])
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_frames_consensus_vs_oracle(ce, order, C, N):
    """ops.frames_consensus: rows of the songs in the pool bit-equal to
    np.mean(np.array(pred_prob), 0); rows of excluded songs are not written."""
    ops, lib = ce.ops, ce._lib.load()
    rng = np.random.default_rng(2000 * C + N + (order == "grouped"))
    s_id, members, P = frame_pool(rng, N, C, order == "grouped", N // 3)
    _, off, perm = geometry(ce, s_id)
    md = [dev(m) for m in members]
    rows = np.mean(P, axis=0)
    got = ops.frames_consensus(md, off, perm, [False, False, True])
    want = "ce::k_frames_rows_excl<3, true>" if C == 3 else "ce::k_frames_consensus<%d, %s, false>" % (
        C, "true" if DMA_FORCED and order == "grouped" else "false")
    assert lib.ce_last_kernel().decode() == want
    assert got.dtype == torch.float64 and np.array_equal(got.cpu().numpy(), rows, equal_nan=True)
    for mask in (rng.random(N) < 0.3, np.ones(N, bool), np.arange(N) % 2 == 1):
        buf = torch.full((N, C + 3), -7.0, dtype=torch.float64, device="cuda")  # ld_out = C + 3, a sentinel everywhere
        out = ops.frames_consensus(md, off, perm, [False, False, True], excl=bitmap(mask), out=buf[:, 1:C + 1])
        assert out.data_ptr() == buf[:, 1:C + 1].data_ptr()
        exp = np.full((N, C + 3), -7.0)
        exp[~mask, 1:C + 1] = rows[~mask]
        assert np.array_equal(buf.cpu().numpy(), exp, equal_nan=True)


def test_tile_flavour_in_a_child_process(ce):
    """The grouped cases above with the LDS-DMA tiles forced on
    (CE_AMD_FRAMES_DMA=1, which the library reads once per process): a fresh
    child, as test_frames_dma_tiles_vs_oracle runs the plain kernels' tiles."""
    if DMA_FORCED:
        pytest.skip("this is the child")
    env = dict(os.environ, CE_AMD_FRAMES_DMA="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu",
                        "-k", "(select_frames_excl_vs_oracle or frames_consensus_vs_oracle) and grouped",
                        "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_large_pool_tiles_and_gather(ce, order):
    """300 000 ragged songs (>= 4 steps per wave): the tile kernel for grouped
    frames, the non-temporal gather for shuffled ones, with 30 % of the songs
    excluded at random plus a run of 10 000 consecutive ones (whole wave steps
    and whole tiles skipped); the reference-sized pool keeps the plain kernel."""
    ops, lib = ce.ops, ce._lib.load()
    rng = np.random.default_rng(300 + (order == "grouped"))
    S, C = 300_000, 4
    s_id, members, P = frame_pool(rng, S, C, order == "grouped", lo=1, hi=8, nan_cells=0)
    _, off, perm = geometry(ce, s_id)
    md = [dev(m) for m in members]
    mask = rng.random(S) < 0.3
    mask[123_457:133_457] = True
    ex = bitmap(mask)
    flavour = "true, false" if order == "grouped" else "false, true"
    for q in (1, 10, 64):
        v, i = ops.select_frames(md, off, q, perm=perm, song_level=[False, False, True], excl=ex)
        assert lib.ce_last_kernel().decode() == f"ce::k_frames_lanes_excl<{C}, {flavour}>"
        assert_same(v, i, *expected(P, mask, q), (order, q))
    buf = torch.full((S, C), -7.0, dtype=torch.float64, device="cuda")
    ops.frames_consensus(md, off, perm, [False, False, True], excl=ex, out=buf)
    assert lib.ce_last_kernel().decode() == f"ce::k_frames_consensus<{C}, {flavour}>"
    exp = np.full((S, C), -7.0)
    exp[~mask] = np.mean(P, axis=0)[~mask]
    assert np.array_equal(buf.cpu().numpy(), exp, equal_nan=True)
    small = np.repeat(np.arange(1608), 40)
    small = small if order == "grouped" else rng.permutation(small)
    n, soff, sperm = geometry(ce, small)
    ops.select_frames([dev(np.full((len(small), C), 1.0 / C))], soff, 10, perm=sperm, song_level=[False],
                      excl=ops.excl_bitmap(n, "cuda"))
    assert lib.ce_last_kernel().decode() == f"ce::k_frames_lanes_excl<{C}, false, false>"


# ---------------------------------------------------------------------------
# SelectionSession(s_id=)
# ---------------------------------------------------------------------------
def retrained_members(rng, s_id, N, C=4):
    """One epoch's members over the FULL X_train (values change every epoch, as
    after re-training): coarse values, so entropies tie across songs."""
    from oracle.ce_oracle import ref_group_mean

    F = len(s_id)
    frames = []
    for dt in (np.float64, np.float32):
        e = -np.log(rng.random((F, C)))
        frames.append((np.floor(e / e.sum(-1, keepdims=True) * 8) / 8 + 1e-3).astype(dt))
    frames[0][rng.random((F, C)) < 0.01] = np.nan
    song = (np.floor(rng.random((N, C)) * 8) / 8 + 1e-3).astype(np.float32)
    P = np.array([ref_group_mean(m, s_id)[0] for m in frames] + [song])
    return frames + [song], P


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_selection_session_from_frames(ce, mode, order):
    """Every epoch until the pool is dry: select(frames=) equals the host
    shrinking-pool loop and select(committee=committee_from_frames(...))."""
    rng = np.random.default_rng(len(mode) + (order == "grouped"))
    N, q, epochs = 301, 64, 8
    s_id = np.repeat(np.arange(N) * 2 + 9, rng.integers(1, 10, N))
    if order == "shuffled":
        s_id = rng.permutation(s_id)
    data = [retrained_members(rng, s_id, N) for _ in range(epochs)]
    committees = [P for _, P in data]
    kw = {}
    if mode == "mix":  # the table in its own row order; some rows are songs outside the committee's pool
        h2m = np.concatenate([rng.permutation(N)[:240], np.full(20, -1)])
        h2m = h2m[rng.permutation(len(h2m))].astype(np.int64)
        hc = np.round(rng.dirichlet(np.ones(4), len(h2m)), 1)
        hc[::5] = 0.25
        kw = dict(hc=hc, hc_to_mc=h2m)
        exp = shrinking_mix_reference(epochs, q, committees, hc, h2m)[0]
    else:
        exp = shrinking_reference("mc", epochs, q, committees, None)
    a = ce.SelectionSession(q, mode, N, s_id=s_id, **kw)
    b = ce.SelectionSession(q, mode, N, **kw)
    assert np.array_equal(a.song_ids, np.arange(N) * 2 + 9)
    for e in range(epochs):
        members = data[e][0]
        got = a.select(frames=[dev(m) for m in members] if e % 2 else members)  # device tensors or arrays
        assert got.dtype == np.int64 and np.array_equal(got, exp[e]), (mode, e, got[:8], exp[e][:8])
        stack, uniq = ce.committee_from_frames(members, s_id)
        assert np.array_equal(uniq, a.song_ids)
        assert np.array_equal(got, b.select(committee=stack)), (mode, e)
    assert len(exp[-1]) == 0 and len(exp[0]) == q  # ran dry
    assert a.remaining == b.remaining


# ---------------------------------------------------------------------------
# BatchedSelectionSession(frame_offsets=)
# ---------------------------------------------------------------------------
USERS = [0, 1, 33, 700, 1608]
B_EPOCHS = 3


@pytest.fixture(scope="module", params=["grouped", "perm"])
def batched_case(request):
    rng = np.random.default_rng(31 + (request.param == "perm"))
    off = np.concatenate([[0], np.cumsum(USERS)]).astype(np.int64)
    T = int(off[-1])
    s_id = np.repeat(np.arange(T), rng.integers(1, 8, T))  # the stacked songs' ids: user u owns off[u]:off[u+1]
    if request.param == "perm":
        s_id = rng.permutation(s_id)
    data = [retrained_members(rng, s_id, T) for _ in range(B_EPOCHS)]
    n_rows = [min(n, max(1, int(0.8 * n))) for n in USERS]  # (a single mix session needs a table row)
    off_h = np.concatenate([[0], np.cumsum(n_rows)]).astype(np.int64)
    h2m = np.concatenate([rng.permutation(n)[:nh] for n, nh in zip(USERS, n_rows)] + [np.zeros(0)]).astype(np.int64)
    h2m[rng.random(len(h2m)) < 0.05] = -1
    hc = np.round(rng.dirichlet(np.ones(4), int(off_h[-1])), 1)
    hc[::5] = 0.25
    return off, s_id, data, off_h, h2m, hc


def _batched(ce, case, mode, q):
    off, s_id, _, off_h, h2m, hc = case
    uniq, f_off, f_perm = ce.song_groups(s_id)
    assert len(uniq) == off[-1]
    kw = dict(hc=hc, hc_offsets=off_h, hc_to_mc=h2m) if mode == "mix" else {}
    return ce.BatchedSelectionSession(q, mode, off, frame_offsets=f_off, frame_perm=f_perm, **kw)


def _user_view(case, u, members):
    """user u's own X_train: its frame rows in their order, song ids local"""
    off, s_id = case[0], case[1]
    rows = (s_id >= off[u]) & (s_id < off[u + 1])
    return s_id[rows] - off[u], [members[0][rows], members[1][rows], members[2][off[u]:off[u + 1]]]


@pytest.mark.parametrize("mode,q", [("mc", 20), ("mix", 20), ("mix", 65)])
def test_batched_session_from_frames(ce, batched_case, mode, q):
    """Every user and epoch: step(frames=) equals a per-user
    SelectionSession(s_id=) and the host loop; q = 65 composes the mix."""
    off, s_id, data, off_h, h2m, hc = batched_case
    U = len(USERS)
    sess = _batched(ce, batched_case, mode, q)
    exp, singles = [], []
    for u in range(U):
        cs = [np.ascontiguousarray(P[:, off[u]:off[u + 1]]) for _, P in data]
        hu, mu = hc[off_h[u]:off_h[u + 1]], h2m[off_h[u]:off_h[u + 1]]
        if USERS[u] == 0:
            exp.append([np.zeros(0, np.int64)] * B_EPOCHS)
            singles.append(None)
            continue
        exp.append(shrinking_mix_reference(B_EPOCHS, q, cs, hu, mu)[0] if mode == "mix"
                   else shrinking_reference("mc", B_EPOCHS, q, cs, None))
        sid_u, _ = _user_view(batched_case, u, data[0][0])
        singles.append(ce.SelectionSession(q, mode, USERS[u], s_id=sid_u,
                                           **(dict(hc=hu, hc_to_mc=mu) if mode == "mix" else {})))
    for e in range(B_EPOCHS):
        members = data[e][0]
        got = sess.select(frames=[dev(m) for m in members])
        if mode == "mix":
            k = ce._lib.load().ce_last_kernel()
            assert k.startswith(b"ce::k_select_tiles_mix<") == (q <= 64), k
        for u in range(U):
            assert np.array_equal(got[u], exp[u][e]), (mode, q, e, u, got[u][:8], exp[u][e][:8])
            if singles[u] is not None:
                one = singles[u].select(frames=_user_view(batched_case, u, members)[1])
                assert np.array_equal(got[u], one), (mode, q, e, u)
    assert sess.remaining.tolist() == [0 if s is None else s.remaining for s in singles]


def test_frames_epoch_in_a_hip_graph(ce, batched_case):
    """One mix epoch from frames (consensus rows, select, mark) captured once
    and replayed per epoch, the re-trained members written into the captured
    tensors in place: the picks are the eager session's."""
    off, s_id, data, off_h, _, _ = batched_case
    ops, q = ce.ops, 20
    eager, graphed = _batched(ce, batched_case, "mix", q), _batched(ce, batched_case, "mix", q)
    md = [dev(m) for m in data[0][0]]
    ops.select_mc(dev(data[0][1]), q, "MNC")  # an eager call first: it creates the device's graph arena
    ops.reserve_graph_workspace(ce._lib.load().ce_select_batched_mix_workspace_bytes(
        int(off[-1]), int(off_h[-1]), len(USERS), q))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph(keep_graph=True)
    with warnings.catch_warnings():
        warnings.simplefilter("error")  # the fallback (a captured zero fill) warns
        with torch.cuda.graph(g):
            idx = graphed.step(frames=md)
    g.instantiate()
    assert _graph_counts(g) == (3, 2)  # consensus rows -> select -> mark: linear, no parallel branches
    for e in range(B_EPOCHS):
        for t, m in zip(md, data[e][0]):
            t.copy_(dev(m))
        g.replay()
        torch.cuda.synchronize()
        got = graphed.account(idx)
        exp = eager.select(frames=[dev(m) for m in data[e][0]])
        assert all(np.array_equal(x, y) for x, y in zip(got, exp)), e
        assert any(len(x) for x in got)
    assert graphed.remaining.tolist() == eager.remaining.tolist()
