"""The cases of tests/test_gpu_frames_tiles.py checked on the CPU: the tile
table restated from the kernel text, that the layouts put rows where they claim
(so the coverage the GPU module speaks of is itself asserted), and the
position-loop restatement of the groupby mean pinned bit for bit to
oracle.ce_oracle.ref_group_mean."""
import numpy as np
import pytest

import frames_tiles_cases as K
from axes_common import first_diff, same_bits

PAIRS = [pytest.param(C, dt, id=K.pair_id(C, dt)) for C, dt in K.TILED]


def dt_name(dt):
    return "f64" if dt == K.F64 else "f32"


def test_tile_table():
    for (C, dt), row in K.TABLE.items():
        assert K.geom(C, dt) == row
    assert [p for p in K.TABLE if K.TABLE[p][1] is not None] == K.TILED
    assert [K.ragged_rows(rb) for rb in (16, 32, 64)] == [[1, 63, 65], [1, 32, 33], [1, 16, 17]]
    assert K.uniform_length(4, K.F64) * 16 == 640 and K.uniform_length(8, K.F64) * 8 == 264  # the (f)1 step


@pytest.mark.parametrize("C,dt", PAIRS)
def test_layouts_cross_the_tile(C, dt):
    """Every tiled (C, dtype) pair has steps with R1 - R0 > TR, and each layout
    puts its songs where its name says."""
    RB, TR, G = K.geom(C, dt)
    crossing = {}
    for name in K.LAYOUTS:
        case = K.layout_case(name, C, dt_name(dt))
        off, ln, N = case["off"], case["lengths"], case["N"]
        assert N == 12 * G + 5 and N % G == 5 and len(off) == N + 1
        rows = K.step_rows(off, G)
        crossing[name] = int((rows > TR).sum())
        s = case["marks"]["edge_step"]
        rel = off - off[s * G]  # row positions relative to the edge step's first row
        n = case["crosser"]
        assert s * G <= n < (s + 1) * G
        if name == "straddle":
            assert (rel[n], rel[n + 1] - 1) == (TR - 3, TR + 4) and ln[n - 1] == 1 and ln[n + 1] == 1
            r6 = off - off[6 * G]
            assert np.any((r6[:-1] == 2 * TR - 3) & (r6[1:] == 2 * TR + 5))
        if name == "exact":
            assert rel[n] == TR and ln[n - 1] == 9 and ln[n] == 17
            assert rows[6] == TR and rows[7] == 2 * TR
        if name == "giant":
            g = case["marks"]["giant"]
            assert [int(ln[x]) for x in g] == [2 * TR + 37] * 3
            assert g[0] % G == 0 and g[1] % G == G - 1 and g[2] == N - 1
            assert set(np.delete(ln, g)[G:2 * G - 1]) == {1}
        if name == "ragged":
            units = [(int(rows[k]) - TR) * RB // 16 for k in (1, 6, 7)]
            assert units == [-(-u * 16 // RB) * RB // 16 for u in K.RAGGED_UNITS]
            assert all(u % 64 for u in units[::2])  # a clamped source unit, a partial 1 KiB group
        if name == "uniform":
            assert set(ln) == {K.uniform_length(C, dt)} and np.all(rows[:-1] > TR)
        if name == "batch":
            assert list(ln[G:G + 6]) == [7, 8, 9, 15, 16, 17] == list(ln[6 * G + 1:6 * G + 7])
        if name == "empty":
            e = np.flatnonzero(ln == 0)
            assert G in e and N - 1 in e and np.all(ln[6 * G:7 * G] == 0)
            assert np.any(rel[e] == TR)  # one sits on the tile edge
            assert np.all(np.isnan(case["P"][:2, e]))
    assert all(crossing[name] >= 1 for name in K.LAYOUTS), crossing
    assert crossing["giant"] == 3 and crossing["exact"] == 2  # exact: one step IS one tile and crosses nothing


@pytest.mark.parametrize("C,dt", PAIRS + [pytest.param(3, K.F64, id="C3_f64")])
def test_position_loop_is_the_groupby_mean_on_the_layouts(C, dt):
    for name in K.LAYOUTS:
        case = K.layout_case(name, C, dt_name(dt))
        for fm, want in zip(case["members"][:2], case["P"][:2]):
            got = K.position_loop_mean(fm, case["off"])
            assert got.dtype == fm.dtype
            assert same_bits(got, want), (name, first_diff(got, want))


@pytest.mark.parametrize("dt", [K.F64, K.F32], ids=["f64", "f32"])
def test_position_loop_is_the_groupby_mean_on_a_ragged_pool(dt):
    """5 000 songs of 1..60 frames, NaN cells, a song all NaN and one with one
    column all NaN: the same bits as ref_group_mean, and as np.add.at's order."""
    from oracle.ce_oracle import ref_group_mean

    rng = np.random.default_rng(5000 + (dt == K.F32))
    N, C = 5000, 4
    ln = rng.integers(1, 61, N)
    off = K.offsets_of(ln)
    s_id = np.repeat(np.arange(N) * 2 + 1, ln)
    v = (K.prob_rows(rng, len(s_id), C, K.F64, 0.03) * 10.0 ** rng.uniform(-6, 6, (len(s_id), 1))).astype(dt)
    v[off[17]:off[18]] = np.nan
    v[off[400]:off[401], 2] = np.nan
    want, keys = ref_group_mean(v, s_id)
    got = K.position_loop_mean(v, off)
    assert len(keys) == N and got.dtype == want.dtype == dt
    assert np.all(np.isnan(got[17])) and np.isnan(got[400, 2]) and not np.isnan(got[400, 0])
    assert same_bits(got, want), first_diff(got, want)
    assert same_bits(K.ref_means(v, ln), want)
    if dt == K.F64:  # the comparison has teeth: the same rows added in reverse order change bits
        # (float32 results round most such differences away, so only the f64 column can show them)
        rev = K.position_loop_mean(np.concatenate([v[off[n]:off[n + 1]][::-1] for n in range(N)]), off)
        assert not same_bits(rev, want)


def test_natural_pool_steps_pass_the_tile():
    """About half the 16-song steps of the natural-dispatch pool pass the f64
    member's 512 rows, none the f32 member's 1024."""
    ln = K.natural_lengths(K.NATURAL_N)
    assert ln.min() == 24 and ln.max() == 40
    rows = K.step_rows(K.offsets_of(ln), 16)
    frac = float((rows > 512).mean())
    assert 0.35 < frac < 0.65 and rows.max() <= 1024, frac


def test_committees_cover_the_axes():
    c = K.COMMITTEES
    nf = lambda kinds: sum(k[0] == "F" for k in kinds)  # noqa: E731
    assert [nf(c["nf%d" % n]) for n in (0, 1, 2, 4, 5, 8)] == [0, 1, 2, 4, 5, 8]
    assert [len(c["M%d" % m]) for m in (1, 2, 4, 8, 3, 5, 7, 32)] == [1, 2, 4, 8, 3, 5, 7, 32]
    assert nf(c["M32"]) > 4 and all(len(v) <= 32 for v in c.values())
    assert c["song_first"][0][0] == "S" and c["song_last"][-1][0] == "S" and c["song_middle"][1][0] == "S"
    assert [k[0] for k in c["song_two"]].count("S") == 2
    s_id, members, sl, P = K.committee_case("nf5", 65, 4, True)
    assert P.shape == (6, 65, 4) and sl == [False] * 5 + [True] and len(s_id) == len(members[0])
    assert np.all(np.isnan(P[1, 65 // 3]))  # the all-NaN song of the first f32 frame member


@pytest.mark.parametrize("how", K.ROW_LAYOUTS)
@pytest.mark.parametrize("dt", [K.F64, K.F32], ids=["f64", "f32"])
def test_nan_parent_views(how, dt):
    v = np.arange(7 * 4, dtype=dt).reshape(7, 4)
    parent, view = K.nan_parent(v, how)
    assert np.array_equal(view, v) and view.base is not None and np.shares_memory(view, parent)
    assert np.isnan(parent).sum() == parent.size - v.size
    assert np.array_equal(K.view_of(parent, how, 7, 4), v)
    if how == "off8":
        assert view.flags.c_contiguous and (view.ctypes.data - parent.ctypes.data) == 8
    else:
        assert view.strides[0] == (4 + (1 if how == "ld_plus1" else 4)) * v.itemsize
