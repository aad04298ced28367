"""The cases of the frames kernels' tile sweep (tests/test_gpu_frames_tiles.py;
tests/test_frames_tiles_cases.py checks the same lists, data and coverage on the
CPU): the tile geometry restated from the kernel text (tile_song_sum,
ce_frames.hpp), song layouts around the edges of the 16 KiB LDS tile, the
committees of the member-axes sweep, the strided and mis-aligned member views,
and the host restatements they are compared with.  Plain numpy: importable
without torch or a GPU."""
import functools

import numpy as np

from axes_common import same_bits  # noqa: F401  (re-exported for the two test modules)

F64, F32 = np.float64, np.float32
TILE_BYTES = 16384  # the per-wave LDS tile of the DMA flavour (TB)


def geom(C, dt):
    """(RB, TR, G) of a member of dtype dt at C classes: bytes per row, rows per
    tile (None: rows are no multiple of 16 B and are never tiled) and songs per
    wave step."""
    RB = C * np.dtype(dt).itemsize
    return RB, (TILE_BYTES // RB if RB % 16 == 0 else None), 64 // C


# the table of the kernel text, written out: geom() must say the same
TABLE = {(4, F64): (32, 512, 16), (4, F32): (16, 1024, 16), (8, F64): (64, 256, 8), (8, F32): (32, 512, 8),
         (2, F64): (16, 1024, 32), (2, F32): (8, None, 32)}
TILED = [(4, F64), (4, F32), (8, F64), (8, F32), (2, F64)]
LAYOUTS = ["straddle", "exact", "giant", "ragged", "uniform", "batch", "empty"]
FULL_STEPS = 12  # N = 3 * 4 * G + 5: three blocks' worth of wave steps and a ragged one
RAGGED_UNITS = (1, 63, 65)  # 16-B units wanted in the second tile (rounded up to whole rows)


def pair_id(C, dt):
    return "C%d_%s" % (C, "f64" if dt == F64 else "f32")


def uniform_length(C, dt):
    """Frames per song of the uniform layout: the (f)1 shape at C = 4 f64 (40
    frames, 640 rows a step), 33 at C = 8 f64 (264 rows), else the shortest
    song whose step passes the tile."""
    _, TR, G = geom(C, dt)
    return {(4, F64): 40, (8, F64): 33}.get((C, dt), TR // G + 1)


def ragged_rows(RB):
    """Rows in the second tile so that it holds 1, 63 and 65 16-B units, rounded
    up to whole rows (RB = 16: 1, 63, 65 units; 32: 2, 64, 66; 64: 4, 64, 68)."""
    return [-(-u * 16 // RB) for u in RAGGED_UNITS]


def layout(name, G, TR, RB, L_uniform=None, seed=0):
    """(lengths int64 [N], marks) of one layout: N = 12 * G + 5 songs, the wave
    steps of G songs in pool order.  marks: 'edge_step' (the step whose rows
    pass the tile edge in the way the layout is about), 'giant' (song indices)
    and 'nan_rel' (rows relative to edge_step's first row that get NaN cells)."""
    rng = np.random.default_rng(seed + 7 * G + TR)
    steps = [list(rng.integers(1, 4, G)) for _ in range(FULL_STEPS)] + [list(rng.integers(1, 4, 5))]
    ones = lambda k: [1] * k  # noqa: E731
    marks = {"edge_step": 1, "giant": [], "nan_rel": []}
    if name == "straddle":  # a song on rows TR - 3 .. TR + 4, 1-row songs on both sides
        a = (G - 2) // 2
        steps[1] = [TR - 3 - a] + ones(a) + [8] + ones(G - 2 - a)
        steps[6] = [2 * TR - 3 - a] + ones(a) + [8] + ones(G - 2 - a)  # the same at the second edge
        marks["nan_rel"] = [TR - 4, TR - 2, TR - 1, TR, TR + 1, TR + 5]
    elif name == "exact":  # a song ends on row TR - 1, the next starts on row TR
        a = (G - 3) // 2
        steps[1] = ones(a) + [TR - a - 9, 9, 17] + ones(G - a - 3)
        steps[6] = [TR - (G - 1)] + ones(G - 1)  # the step is exactly one tile
        steps[7] = [2 * TR - (G - 1)] + ones(G - 1)  # exactly two
        marks["nan_rel"] = [TR - 1, TR]
    elif name == "giant":  # 2 * TR + 37 rows cross three tiles: first, last in its step, last of the pool
        g = 2 * TR + 37
        steps[1] = [g] + ones(G - 1)
        steps[6] = ones(G - 1) + [g]
        steps[FULL_STEPS] = ones(4) + [g]
        marks["giant"] = [G, 6 * G + G - 1, FULL_STEPS * G + 4]
        marks["nan_rel"] = [TR - 1, TR, 2 * TR - 1, 2 * TR]
    elif name == "ragged":  # the second tile holds 1, 63, 65 units: the source-unit clamp, a partial 1 KiB group
        r1, r2, r3 = ragged_rows(RB)
        steps[1] = ones(G - 1) + [TR + r1 - (G - 1)]
        steps[6] = [TR + r2 - (G - 1)] + ones(G - 1)
        steps[7] = [TR // 2, TR // 2 + r3 - (G - 2)] + ones(G - 2)
        marks["nan_rel"] = [TR - 1, TR]
    elif name == "uniform":
        steps = [[L_uniform] * len(s) for s in steps]
        marks["nan_rel"] = [TR - 1, TR]
    elif name == "batch":  # around the 8-row read batches, inside a tile and across its edge
        lens = [7, 8, 9, 15, 16, 17]
        steps[1] = lens + ones(G - 6)
        steps[6] = [TR - 20] + lens + ones(G - 7)
        marks["edge_step"] = 6
        marks["nan_rel"] = [TR - 1, TR]
    elif name == "empty":  # off[n] == off[n + 1]: at a step's start, at the tile edge, a whole step, last in the pool
        a = (G - 4) // 2
        steps[1] = [0] + ones(a) + [TR - a] + [0] + [5] + ones(G - a - 4)
        steps[6] = [0] * G
        steps[7] = [3, 0, 0, 2] + ones(G - 4)
        steps[FULL_STEPS] = [1, 2, 0, 1, 0]
    else:
        raise ValueError(name)
    assert all(len(s) == G for s in steps[:FULL_STEPS]) and len(steps[FULL_STEPS]) == 5
    lengths = np.array([x for s in steps for x in s], np.int64)
    assert lengths.min() >= 0 and len(lengths) == FULL_STEPS * G + 5
    return lengths, marks


def offsets_of(lengths):
    return np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)


def step_rows(off, G):
    """R1 - R0 of every wave step of G songs."""
    N = len(off) - 1
    t = np.arange(0, N, G)
    return off[np.minimum(t + G, N)] - off[t]


def crosser(off, G, TR, step):
    """The song of wave step `step` that holds the step's row TR (the first row of its second tile)."""
    return int(np.searchsorted(off, off[step * G] + TR, "right") - 1)


def prob_rows(rng, F, C, dt, nan_cells=0.01):
    """[F, C] rows of probabilities of dtype dt, a fraction of the cells NaN: every row
    distinct, the sums sensitive to the order and to any row taken twice or left out."""
    e = -np.log(rng.random((F, C)))
    fm = e / e.sum(-1, keepdims=True)
    if nan_cells:
        fm[rng.random((F, C)) < nan_cells] = np.nan
    return fm.astype(dt)


def ref_means(values, lengths):
    """oracle.ce_oracle.ref_group_mean over grouped rows (song n owns the next
    lengths[n] rows); a song without rows -- which a groupby cannot hold -- is a
    NaN row (count 0)."""
    from oracle.ce_oracle import ref_group_mean

    lengths = np.asarray(lengths, np.int64)
    out = np.full((len(lengths), values.shape[1]), np.nan, values.dtype)
    if lengths.sum():
        m, keys = ref_group_mean(values[:lengths.sum()], np.repeat(np.arange(len(lengths)), lengths))
        out[keys] = m
    return out


def position_loop_mean(values, off):
    """ref_group_mean over grouped rows with explicit offsets, fast enough for
    millions of rows: for j = 0, 1, ... row off[n] + j of every song longer than
    j is added to the song's sums, NaN skipped and counted per cell -- per
    (song, column) the sequential order of np.add.at.  Adding 0.0 for a NaN
    cell changes no bit (a sum that starts at +0.0 is never -0.0)."""
    v = np.asarray(values)
    off = np.asarray(off, np.int64)
    ln = np.diff(off)
    N, C = len(ln), v.shape[1]
    s = np.zeros((N, C))
    cnt = np.zeros((N, C), np.int64)
    for j in range(int(ln.max()) if N else 0):
        sel = np.flatnonzero(ln > j)
        x = v[off[sel] + j].astype(np.float64)
        ok = ~np.isnan(x)
        s[sel] += np.where(ok, x, 0.0)
        cnt[sel] += ok
    with np.errstate(invalid="ignore", divide="ignore"):
        out = np.where(cnt > 0, s / np.maximum(cnt, 1), np.nan)
    return out.astype(np.float32) if v.dtype == np.float32 else out


@functools.lru_cache(maxsize=None)
def layout_case(name, C, dt_name):
    """One layout at a (C, dtype) pair's geometry (C = 3: the lane-per-song
    kernels, long songs at the C = 4 f64 geometry): dict with lengths, off, G,
    TR, marks, members [f64 frames, f32 frames, f32 song-level] and the stack P
    [3, N, C] by ref_means."""
    dt = F64 if dt_name == "f64" else F32
    RB, TR, G = geom(4 if C == 3 else C, dt)
    lengths, marks = layout(name, G, TR, RB, uniform_length(4 if C == 3 else C, dt))
    off = offsets_of(lengths)
    rng = np.random.default_rng(100 * C + len(name) + (dt == F32))
    F, N = int(off[-1]), len(lengths)
    frames = [prob_rows(rng, F, C, F64), prob_rows(rng, F, C, F32)]
    base = int(off[marks["edge_step"] * G])
    for k, rel in enumerate(marks["nan_rel"]):  # NaN cells on the rows next to the edge, in both frame members
        for fm in frames:
            if base + rel < F:
                fm[base + rel, k % C] = np.nan
                if k == 1:
                    fm[base + rel, :] = np.nan
    song = rng.random((N, C)).astype(F32)
    P = np.array([ref_means(fm, lengths) for fm in frames] + [song])
    return dict(lengths=lengths, off=off, G=G, TR=TR, RB=RB, marks=marks, members=frames + [song], P=P, N=N, C=C,
                crosser=crosser(off, G, TR, marks["edge_step"]))


def layout_masks(case):
    """name -> bool [N] (True = excluded) of the exclusion bitmaps over a layout."""
    N, G, s = case["N"], case["G"], case["marks"]["edge_step"]
    out = {}
    if case["marks"]["giant"]:
        m = np.zeros(N, bool)
        m[case["marks"]["giant"]] = True
        out["giant"] = m
    m = np.zeros(N, bool)
    m[s * G:(s + 1) * G] = True  # the wave-uniform skip of the step that holds the edge
    out["edge_step"] = m
    m = np.ones(N, bool)
    m[case["crosser"]] = False
    out["only_crosser"] = m
    return out


# ---------------------------------------------------------------------------
# the natural-dispatch pool
# ---------------------------------------------------------------------------
NATURAL_N = 98_305  # the smallest pool whose waves run 4 steps of 16 songs on the 2 x 256 resident blocks


def natural_lengths(N, seed=2400):
    return np.random.default_rng(seed + 1).integers(24, 41, N)


def natural_pool(N, C=4, seed=2400):
    """N songs of 24..40 frames (about half the 16-song steps pass the f64
    member's 512-row tile): off, members [f64 frames, f32 frames, f32
    song-level], the stack by position_loop_mean, and the exclusion mask (30 % at
    random plus 10 000 consecutive songs)."""
    rng = np.random.default_rng(seed)
    off = offsets_of(natural_lengths(N, seed))
    F = int(off[-1])
    frames = [prob_rows(rng, F, C, F64, 0.001), prob_rows(rng, F, C, F32, 0.001)]
    song = rng.random((N, C)).astype(F32)
    P = np.array([position_loop_mean(fm, off) for fm in frames] + [song])
    mask = rng.random(N) < 0.3
    mask[N // 3:N // 3 + 10_000] = True
    return off, frames + [song], P, mask


# ---------------------------------------------------------------------------
# member axes
# ---------------------------------------------------------------------------
def _alt(n, first="F64"):
    other = "F32" if first == "F64" else "F64"
    return [first if k % 2 == 0 else other for k in range(n)]


def committees():
    """name -> member kinds in member order: 'F64' / 'F32' a frame-level member,
    'S64' / 'S32' a song-level one."""
    out = {}
    for nf in (0, 1, 2, 4, 5, 8):  # frame-level members; 5 and 8 leave the read-together path
        out["nf%d" % nf] = _alt(nf) + (["S32"] if nf else ["S32", "S64"])
    for M in (1, 2, 4, 8, 3, 5, 7, 32):  # power-of-two and division paths of div_members, the cap
        kinds = [("S32" if k % 4 == 3 else ("F64" if k % 2 == 0 else "F32")) for k in range(M)]
        out["M%d" % M] = kinds
    out["song_first"] = ["S32", "F64", "F32", "F64"]
    out["song_middle"] = ["F64", "S32", "F32", "F64"]
    out["song_last"] = ["F64", "F32", "F64", "S32"]
    out["song_two"] = ["F64", "S32", "S64", "F32"]
    out["all_f64"] = ["F64", "F64", "F64", "S64"]
    out["all_f32"] = ["F32", "F32", "F32", "S32"]
    out["alt_f32_first"] = _alt(3, "F32") + ["S32"]
    out["alt_f64_first"] = _alt(3, "F64") + ["S32"]
    return out


COMMITTEES = committees()
BANK = 8  # distinct value sets per kind; member k of a committee takes set k % BANK


@functools.lru_cache(maxsize=None)
def axes_pool(N, C, grouped):
    """N songs of 1..9 frames: (s_id, lengths) -- grouped, or the frame rows shuffled."""
    rng = np.random.default_rng(31 * N + C + grouped)
    lengths = rng.integers(1, 10, N)
    s_id = np.repeat(np.arange(N) * 3 + 5, lengths)
    if not grouped:
        s_id = rng.permutation(s_id)
    return s_id, lengths


@functools.lru_cache(maxsize=None)
def axes_member(N, C, grouped, kind, k):
    """(values, per-song rows [N, C]) of value set k of a kind over axes_pool: the
    rows by ref_group_mean for a frame-level member, the values themselves for a
    song-level one.  The first frame-level f32 set has a song whose frames are all NaN."""
    from oracle.ce_oracle import ref_group_mean

    s_id, _ = axes_pool(N, C, grouped)
    dt = F64 if kind.endswith("64") else F32
    rng = np.random.default_rng([N, C, int(grouped), ord(kind[0]), int(kind[1:]), k])
    if kind[0] == "S":
        v = rng.random((N, C)).astype(dt)
        return v, v
    v = prob_rows(rng, len(s_id), C, dt)
    if kind == "F32" and k == 1:
        v[s_id == (N // 3) * 3 + 5] = np.nan
    return v, ref_group_mean(v, s_id)[0]


def committee_case(name, N, C, grouped):
    """(s_id, member values in member order, song_level flags, the stack P [M, N,
    C] float64).  np.array(pred_prob) of a mixed committee is float64 already;
    an all-float32 one is upcast here, as the engine's contract has it (DESIGN.md
    section 3: f32 load, f64 accumulate -- the reference on the f64 upcast)."""
    kinds = COMMITTEES[name]
    got = [axes_member(N, C, grouped, kind, k % BANK) for k, kind in enumerate(kinds)]
    return (axes_pool(N, C, grouped)[0], [g[0] for g in got], [kind[0] == "S" for kind in kinds],
            np.array([g[1] for g in got]).astype(np.float64))


# ---------------------------------------------------------------------------
# row layouts: views of a NaN-filled parent
# ---------------------------------------------------------------------------
ROW_LAYOUTS = ["ld_plus1", "ld_plus4", "off8"]


def nan_parent(values, how):
    """(parent, view) -- `view` holds `values` inside the NaN-filled flat `parent`
    and is built from it by slicing alone, so the same slicing of the parent's
    device copy is the same view: a row stride of C + 1 or C + 4 elements, or
    dense rows whose first byte lies 8 bytes past a 16-byte boundary (one f64 or
    two f32 elements into a fresh buffer)."""
    rows, C = values.shape
    if how in ("ld_plus1", "ld_plus4"):
        ld = C + (1 if how == "ld_plus1" else 4)
        parent = np.full(rows * ld, np.nan, values.dtype)
        view = view_of(parent, how, rows, C)
    elif how == "off8":
        parent = np.full(rows * C + 16, np.nan, values.dtype)
        view = view_of(parent, how, rows, C)
    else:
        raise ValueError(how)
    view[...] = values
    return parent, view


def view_of(parent, how, rows, C):
    """The slicing of nan_parent, on a numpy array or a torch tensor alike."""
    if how in ("ld_plus1", "ld_plus4"):
        ld = C + (1 if how == "ld_plus1" else 4)
        return parent.reshape(rows, ld)[:, :C]
    e = 8 // parent.element_size() if hasattr(parent, "element_size") else 8 // parent.itemsize
    return parent[e:e + rows * C].reshape(rows, C)
