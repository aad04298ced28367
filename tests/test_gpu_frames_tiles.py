"""The fused frames kernels (k_frames_lanes{,_excl}, k_frames_consensus,
k_segment_mean_tiles and their staging routine tile_song_sum; ce_frames.hpp)
where their suite had not been: songs across and beyond the 16 KiB LDS tile,
several tiles per step and several steps per wave, committees of 1..32 members
with 0..8 frame-level ones, row-strided and mis-aligned members.

The bar is bit equality of values and equality of indices against
oracle.ce_oracle.ref_group_mean -> np.array(pred_prob) -> np.mean(axis=0) ->
oracle_select_mc (NaN matches NaN); no tolerance anywhere.  The geometry (RB, TR,
G per class count and dtype) is restated in frames_tiles_cases.py from the
kernel text, and tests/test_frames_tiles_cases.py asserts on the CPU that the
layouts reach what they claim.  The kernel flavour of every call is asserted
through ce_last_kernel(); the tile flavour is forced at these small sizes by
CE_AMD_FRAMES_DMA=1 in child processes (the library reads it once)."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import frames_tiles_cases as K
from axes_common import first_diff, same_bits
from test_gpu_batched_session import assert_same, bitmap, dev
from test_gpu_frames_session import expected

pytestmark = pytest.mark.gpu

DMA_FORCED = os.environ.get("CE_AMD_FRAMES_DMA") == "1"  # a child of test_forced_tiles_in_a_child_process


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def flavour(what, C, grouped, excl):
    """The kernel a call of these sizes must land on."""
    if C == 3:  # lane per song
        if what == "consensus":
            return "ce::k_frames_rows_excl<3, true>"
        return "ce::k_frames_select_excl<3>" if excl else "ce::k_frames_select<3>"
    dma = "true" if DMA_FORCED and grouped else "false"
    if what == "consensus":
        return "ce::k_frames_consensus<%d, %s, false>" % (C, dma)
    return "ce::k_frames_lanes%s<%d, %s, false>" % ("_excl" if excl else "", C, dma)


def assert_kernel(ce, want):
    got = ce._lib.load().ce_last_kernel().decode()
    print("flavour:", got)
    assert got == want


def check_pool(ce, md, off, perm, sl, P, masks, qs, tag):
    """select_frames (plain and under every bitmap of `masks`) and
    frames_consensus (into a sentinel-filled buffer with ld_out = C + 3) against
    the stack P [M, N, C]."""
    ops = ce.ops
    _, N, C = P.shape
    grouped = perm is None
    rows = np.mean(P, axis=0)
    for q in qs:
        v, i = ops.select_frames(md, off, q, perm=perm, song_level=sl)
        assert_kernel(ce, flavour("select", C, grouped, False))
        assert_same(v, i, *expected(P, np.zeros(N, bool), q), (tag, "plain", q))
        for name, mask in masks.items():
            v, i = ops.select_frames(md, off, q, perm=perm, song_level=sl, excl=bitmap(mask))
            assert_kernel(ce, flavour("select", C, grouped, True))
            assert_same(v, i, *expected(P, mask, q), (tag, name, q))
    for name, mask in [("plain", None)] + list(masks.items()):
        buf = torch.full((N, C + 3), -7.0, dtype=torch.float64, device="cuda")
        ops.frames_consensus(md, off, perm, sl, excl=None if mask is None else bitmap(mask), out=buf[:, 1:C + 1])
        assert_kernel(ce, flavour("consensus", C, grouped, mask is not None))
        exp = np.full((N, C + 3), -7.0)
        keep = np.ones(N, bool) if mask is None else ~mask
        exp[keep, 1:C + 1] = rows[keep]
        got = buf.cpu().numpy()
        assert same_bits(got, exp), (tag, name, first_diff(got, exp))


def random30(N, seed):
    return {"random30": np.random.default_rng(seed).random(N) < 0.3}


# ---------------------------------------------------------------------------
# 1. song layouts around the tile edge
# ---------------------------------------------------------------------------
LAYOUT_CASES = [pytest.param(name, C, "f64" if dt == K.F64 else "f32", id="%s-%s" % (name, K.pair_id(C, dt)))
                for C, dt in K.TILED + [(3, K.F64)] for name in K.LAYOUTS]


@pytest.mark.parametrize("name,C,dtn", LAYOUT_CASES)
def test_tile_layouts(ce, name, C, dtn):
    """Every layout of frames_tiles_cases.layout at the geometry of its (C,
    dtype) pair, grouped frames without perm: select_frames at q = 1, 10, 64
    plain and under the layout's bitmaps (the giant song, the whole step that
    holds the edge, all but the song that crosses it), frames_consensus and
    segment_mean.  This process: the direct flavour (C = 3: the lane-per-song
    kernels).  The child with the tiles forced: every step of these pools that
    is longer than TR rows runs the tile loop more than once."""
    case = K.layout_case(name, C, dtn)
    members, off, P, N = case["members"], dev(case["off"]), case["P"], case["N"]
    md = [dev(m) for m in members]
    check_pool(ce, md, off, None, [False, False, True], P, K.layout_masks(case), (1, 10, 64), name)
    for fm, fd, want in zip(members[:2], md[:2], P[:2]):  # one member alone: k_segment_mean_tiles where it applies
        got = ce.ops.segment_mean(fd, off)
        assert got.dtype == fd.dtype and same_bits(got.cpu().numpy(), want), (name, first_diff(got.cpu().numpy(), want))
        buf = torch.full((N, C + 2), -7.0, dtype=torch.float64, device="cuda")
        ce.ops.segment_mean(fd, off, out=buf[:, 1:C + 1])
        exp = np.full((N, C + 2), -7.0)
        exp[:, 1:C + 1] = want
        assert same_bits(buf.cpu().numpy(), exp), (name, fm.dtype)


# ---------------------------------------------------------------------------
# 2. the dispatch's own choice of the tiles: several steps per wave, several tiles per step
# ---------------------------------------------------------------------------
def test_natural_dispatch_pool(ce):
    """The smallest pool whose waves run >= 4 steps (lanes_flavour then takes the
    tiles by itself): songs of 24..40 frames at C = 4, so about half the steps
    pass the f64 member's 512-row tile while the offsets of the next step are
    in flight; 30 % of the songs and a run of 10 000 excluded.  One song fewer
    keeps the direct flavour."""
    ops, N, C = ce.ops, K.NATURAL_N, 4
    off_h, members, P, mask = K.natural_pool(N, C)
    md, off, ex = [dev(m) for m in members], dev(off_h), bitmap(mask)
    sl = [False, False, True]
    for q in (10, 64):
        v, i = ops.select_frames(md, off, q, song_level=sl, excl=ex)
        assert_kernel(ce, "ce::k_frames_lanes_excl<4, true, false>")
        assert_same(v, i, *expected(P, mask, q), ("natural", q))
    v, i = ops.select_frames(md, off, 10, song_level=sl)
    assert_kernel(ce, "ce::k_frames_lanes<4, true, false>")
    assert_same(v, i, *expected(P, np.zeros(N, bool), 10), ("natural", "plain"))
    buf = torch.full((N, C), -7.0, dtype=torch.float64, device="cuda")
    ops.frames_consensus(md, off, None, sl, excl=ex, out=buf)
    assert_kernel(ce, "ce::k_frames_consensus<4, true, false>")
    exp = np.full((N, C), -7.0)
    exp[~mask] = np.mean(P, axis=0)[~mask]
    got = buf.cpu().numpy()
    assert same_bits(got, exp), first_diff(got, exp)
    # N is the smallest: the first N - 1 songs, same members, same offsets
    ops.select_frames(md, off[:N], 10, song_level=sl, excl=bitmap(mask[:N - 1]))
    assert_kernel(ce, "ce::k_frames_lanes_excl<4, false, false>")


# ---------------------------------------------------------------------------
# 3. member axes
# ---------------------------------------------------------------------------
def pool_geometry(ce, s_id, N):
    uniq, offsets, perm = ce.song_groups(s_id)
    assert len(uniq) == N
    return dev(offsets), (dev(perm) if perm is not None else None)


@pytest.mark.parametrize("N", [65, 900], ids=["N65", "N900"])
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("C", [2, 3, 4, 8], ids=lambda c: "C%d" % c)
@pytest.mark.parametrize("name", list(K.COMMITTEES))
def test_member_axes(ce, name, C, order, N):
    """Committees of frames_tiles_cases.committees(): 0..8 frame-level members
    (past 4 the read-together path gives way to the per-member loop), M = 1..32
    (the power-of-two and the division path of div_members), the song-level
    member first, in the middle, last and twice, every dtype mix."""
    s_id, members, sl, P = K.committee_case(name, N, C, order == "grouped")
    off, perm = pool_geometry(ce, s_id, N)
    assert (perm is None) == (order == "grouped")
    check_pool(ce, [dev(m) for m in members], off, perm, sl, P, random30(N, N + C), (10,), name)


def test_member_count_errors(ce):
    """M = 33 and M = 0 are refused and nothing is written."""
    ops, N, C, q = ce.ops, 65, 4, 10
    s_id, members, _, _ = K.committee_case("nf1", N, C, True)
    off, _ = pool_geometry(ce, s_id, N)
    md = [dev(members[1])] * 33  # 33 song-level members
    with pytest.raises(ValueError):
        ops.select_frames(md, off, q, song_level=[True] * 33)
    buf = torch.full((N, C), -7.0, dtype=torch.float64, device="cuda")
    with pytest.raises(ValueError):
        ops.frames_consensus(md, off, None, [True] * 33, out=buf)
    with pytest.raises(ValueError):
        ops.select_frames([], off, q)
    with pytest.raises(ValueError):
        ops.frames_consensus([], off, None, out=buf)
    # the entry points themselves, outputs in hand
    arr, keep, _, _, _, _ = ops._frame_members(md, off, None, [True] * 33)
    lib = ce._lib.load()
    ws = ops.new_workspace(lib.ce_select_frames_workspace_bytes(N, q), off.device)
    vals = torch.full((q,), -7.0, dtype=torch.float64, device="cuda")
    idx = torch.full((q,), -7, dtype=torch.int64, device="cuda")
    p = ctypes.cast(arr, ctypes.c_void_p)
    for M in (33, 0):
        for excl in (None, ops.excl_bitmap(N, "cuda")):
            head = (p, M, C, ops._p(off), None, N)
            tail = (q, 0, ops._p(ws), ws.numel(), ops._p(vals), ops._p(idx), ops._stream(off.device))
            with pytest.raises(ValueError):
                if excl is None:
                    ce._lib.call("ce_select_frames", *head, *tail)
                else:
                    ce._lib.call("ce_select_frames_excl", *head, ops._p(excl), *tail)
            with pytest.raises(ValueError):
                ce._lib.call("ce_frames_consensus", *head, ops._p(excl) if excl is not None else None, ops._p(buf), C,
                             ops._stream(off.device))
    torch.cuda.synchronize()
    assert bool((vals == -7.0).all()) and bool((idx == -7).all()) and bool((buf == -7.0).all())


# ---------------------------------------------------------------------------
# 4. row layouts
# ---------------------------------------------------------------------------
ROW_CASES = [(how, level, dtn) for how in K.ROW_LAYOUTS for level in ("frame", "song") for dtn in ("f64", "f32")]


def row_layout_committee(N, C, grouped, how, level, dtn):
    """(host member values, device members, song_level, P): the member under test a
    view of a NaN-filled parent, host and device alike; the other frame-level
    member(s) dense and aligned, so a forced-tile launch takes tiles for one
    member and the fallback loads for the next."""
    kind = ("F" if level == "frame" else "S") + dtn[1:]
    v, rows = K.axes_member(N, C, grouped, kind, 0)
    dense = [K.axes_member(N, C, grouped, k, j) for k, j in (("F64", 2), ("F32", 1), ("S32", 3))]
    if how == "dense":
        view_h, view_d = v, dev(v)
    else:
        parent, view_h = K.nan_parent(v, how)
        view_d = K.view_of(dev(parent), how, *v.shape)
        assert view_d.stride(1) == 1 and np.array_equal(view_d.cpu().numpy(), v, equal_nan=True)
        if how == "off8":
            assert view_d.data_ptr() % 16 == 8 and view_d.stride(0) == C
        else:
            assert view_d.stride(0) == C + (1 if how == "ld_plus1" else 4)
    if level == "frame":
        host = [view_h, dense[0][0], dense[2][0]]
        md, sl = [view_d, dev(dense[0][0]), dev(dense[2][0])], [False, False, True]
        P = np.array([rows, dense[0][1], dense[2][1]])
    else:
        host = [dense[0][0], view_h, dense[1][0]]
        md, sl = [dev(dense[0][0]), view_d, dev(dense[1][0])], [False, True, False]
        P = np.array([dense[0][1], rows, dense[1][1]])
    return host, md, sl, P


@pytest.mark.parametrize("N", [65, 900], ids=["N65", "N900"])
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("C", [2, 3, 4, 8], ids=lambda c: "C%d" % c)
@pytest.mark.parametrize("how,level,dtn", ROW_CASES)
def test_row_layouts(ce, how, level, dtn, C, order, N):
    """A member with a row stride of C + 1 or C + 4 elements, or with its base 8
    bytes off a 16-byte boundary (vec = 0), frame-level or song-level: the
    values of the dense member it is a view of.  The parent buffer is NaN
    everywhere else, so a read outside the view reaches the values."""
    grouped = order == "grouped"
    s_id, _ = K.axes_pool(N, C, grouped)
    off, perm = pool_geometry(ce, s_id, N)
    _, md, sl, P = row_layout_committee(N, C, grouped, how, level, dtn)
    check_pool(ce, md, off, perm, sl, P, random30(N, N + C + 1), (10,), (how, level, dtn))


@pytest.mark.parametrize("N", [65, 900], ids=["N65", "N900"])
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_row_layouts_f32_at_two_classes(ce, order, N):
    """A dense f32 member at C = 2 has 8-byte rows and is never tiled: next to a
    tiled f64 member in one launch."""
    grouped = order == "grouped"
    s_id, _ = K.axes_pool(N, 2, grouped)
    off, perm = pool_geometry(ce, s_id, N)
    _, md, sl, P = row_layout_committee(N, 2, grouped, "dense", "frame", "f32")
    assert K.geom(2, K.F32)[1] is None and K.geom(2, K.F64)[1] == 1024
    check_pool(ce, md, off, perm, sl, P, random30(N, N + 3), (10,), "f32 at C = 2")


# ---------------------------------------------------------------------------
# the tile flavour at these sizes: child processes
# ---------------------------------------------------------------------------
CHILDREN = {
    "layouts": "test_tile_layouts and not C3_",
    "members": "test_member_axes and grouped and nf5 and not C3",
    "rows": "test_row_layouts and grouped and not C3",
}


@pytest.mark.parametrize("which", list(CHILDREN))
def test_forced_tiles_in_a_child_process(ce, which):
    """The grouped cases above with the LDS-DMA tiles forced on
    (CE_AMD_FRAMES_DMA=1, read once per process): k_frames_lanes{,_excl}<C, true,
    false>, k_frames_consensus<C, true, false> and k_segment_mean_tiles at C =
    2, 4, 8 -- the layouts (steps of two and three tiles), five frame-level
    members, and a strided or mis-aligned member beside a tiled one."""
    if DMA_FORCED:
        pytest.skip("this is the child")
    env = dict(os.environ, CE_AMD_FRAMES_DMA="1")
    r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-q", "-x", "-m", "gpu",
                        "-k", CHILDREN[which], "-p", "no:cacheprovider"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert " passed" in r.stdout and "skipped" not in r.stdout
