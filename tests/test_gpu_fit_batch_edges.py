"""The two retrain kernels across the edges of their row staging, at the widths
where the edges matter.

k_gnb_partial_fit stages a batch's row offsets and classes in LDS tiles of 1024
rows (kFitTile) and walks a tile in double-buffered chunks of 16 rows
(kFitAhead), reading past a short tile's end with clamped indices:
batches on both sides of every chunk edge, of the tile edge, of the chunk edges
inside the second tile, and of the second and third tile edge; classes placed
on either side of a tile edge; models with 0, 1, 2 and 3 tile trips in one
launch.  k_sgd_partial_fit fetches the visiting order's rows in blocks of 64
(m_cur / m_next) and visits them in double-buffered chunks of 4: batches around
every block edge up to the fourth and past the 16th, with every lane owning
features and with 8 waves.  Then both through the member classes, with a
batch of more than 1024 rows picked from a session.

The references are the row-loop restatements of sklearn (tests/gnb_fit_ref.py,
tests/sgd_fit_ref.py; the CPU suite pins them to sklearn past 1024 rows too).
Every comparison is 0 ulp on every output; a NaN matches a NaN.  A test loops
its batch sizes and reports every size that differs, so a defect shows as the
list of sizes it breaks."""
import numpy as np
import pytest
import torch

from gnb_fit_ref import gnb_partial_fit, same_bits
from sgd_fit_ref import chain_seeds, sgd_partial_fit
from test_gpu_gnb_partial_fit import NAMES, fitted_state
from test_gpu_gnb_partial_fit import DeviceState as GnbState
from test_gpu_sgd_partial_fit import PERM_LDS, model
from test_gpu_sgd_partial_fit import DeviceState as SgdState

pytestmark = pytest.mark.gpu

TILE = 1024  # kFitTile (csrc/ce_gnb_fit.hpp)
SGD_NAMES = ("coef", "intercept", "t")


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


def differing(got, want, names=NAMES):
    """The names of the outputs that are not equal bit for bit."""
    return [k for k, g, w in zip(names, got, want)
            if not same_bits(np.asarray(g, np.float64).reshape(-1), np.asarray(w, np.float64).reshape(-1))]


def frames(rng, F, D, ld=None, shift=0, spread=1.0):
    """(X on the device as an [F, D] view of row stride ld that starts `shift` elements into its buffer, X on the host)."""
    ld = D if ld is None else ld
    buf = rng.normal(0, 1, F * ld + shift)
    view = buf[shift:].reshape(F, ld)[:, :D]
    view *= np.exp(rng.normal(0, spread, D))  # a scale per feature
    Xd = torch.from_numpy(buf).cuda()[shift:].view(F, ld)[:, :D]
    assert Xd.stride(0) == ld and Xd.data_ptr() % 16 == 8 * shift
    return Xd, np.ascontiguousarray(view)


def report(bad):
    """[(case, outputs that differ)] as one string: every case that differs, and the outputs that do in any of them."""
    return f"{[case for case, _ in bad]} differ in {sorted({str(k) for _, diff in bad for k in diff})}"


# ---------------------------------------------------------------------------
# 1. GaussianNB: batch size x feature layout x class count
# ---------------------------------------------------------------------------
GNB_SIZES = [15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65,  # chunk edges
             1023, 1024, 1025,                                # the tile edge
             1039, 1040, 1041, 1055, 1056, 1057,              # chunk edges inside the second tile
             2047, 2048, 2049, 3073]
# D, ld, elements the view starts into its buffer, the kernel's path (16-byte loads of a lane pair, or 8-byte loads)
LAYOUTS = [(260, 260, 0, True),    # VEC2
           (2, 2, 0, True),        # VEC2, one live lane pair
           (65, 65, 0, False),     # odd D: two waves live, f1 = t + 256 never valid
           (300, 301, 0, False),   # every wave live, f1 valid for t < 44
           (512, 514, 1, False)]   # an 8-byte-aligned base: all of f1 valid


@pytest.mark.parametrize("C", [2, 3, 4, 5, 7, 8])  # 2, 4, 4, 8, 8, 8 accumulators per feature
@pytest.mark.parametrize("D,ld,shift,vec2", LAYOUTS)
def test_gnb_batch_sizes(ce, D, ld, shift, vec2, C):
    """Every size from the same fitted model (its last class unseen), rows drawn
    with replacement and unsorted from 600 frames, so the order and the repeats
    cross the tiles."""
    rng = np.random.default_rng(100000 * C + 100 * D + ld)
    F = 600
    Xd, X = frames(rng, F, D, ld, shift)
    assert vec2 == (D % 2 == 0 and ld % 2 == 0 and Xd.data_ptr() % 16 == 0)
    start = fitted_state(rng, C, D, unseen=(C - 1,))
    bad = []
    for n in GNB_SIZES:
        rows, labels = rng.integers(0, F, n), rng.integers(0, C, n)
        if n >= TILE - 1:
            assert len(np.unique(labels)) == C and (np.diff(rows) < 0).any() and len(np.unique(rows)) < n
        if n >= 2 * TILE - 1:
            assert len(np.unique(labels[TILE:])) == C  # past the first tile too
        st = GnbState(*start)
        st.fit(ce.ops, Xd, rows, labels)
        diff = differing(st.host(), gnb_partial_fit(X[rows], labels, *start))
        if diff:
            bad.append((n, diff))
    assert not bad, f"D={D} ld={ld} shift={shift} C={C}: {report(bad)}"


# ---------------------------------------------------------------------------
# 2. GaussianNB: where a class sits relative to the tile edge
# ---------------------------------------------------------------------------
def labels_around_the_tile_edge(rng, C):
    """name -> labels; class C - 1 has class_count == 0 in the start state.  Every construction is asserted."""
    last, out = C - 1, {}
    lab = rng.integers(0, last, 1030)
    lab[TILE:] = [last, 0, last, 1, last, last]
    assert (lab[:TILE] != last).all() and (lab[TILE:] == last).sum() == 4
    out["unseen_class_only_in_tile_2"] = lab
    lab = rng.integers(0, last, TILE + 1)
    lab[TILE] = last
    assert (lab[:TILE] != last).all() and lab[TILE] == last and len(lab) == 1025
    out["unseen_class_is_the_one_row_of_tile_2"] = lab
    lab = rng.integers(1, C, 1030)
    lab[TILE - 1:TILE + 1] = 0
    assert np.flatnonzero(lab == 0).tolist() == [1023, 1024]
    out["class_holds_rows_1023_and_1024"] = lab
    lab = rng.integers(2, C, 2050)
    lab[rng.choice(TILE, 300, replace=False)] = 0
    lab[2 * TILE:] = 1
    assert (lab[TILE:] != 0).all() and (lab[:TILE] == 0).sum() == 300
    assert (lab[:2 * TILE] != 1).all() and (lab[2 * TILE:] == 1).all() and len(lab) - 2 * TILE == 2
    out["tile_1_only_and_tile_3_only"] = lab
    out["one_class"] = np.full(2 * TILE + 1, 1)
    out["one_class_unseen"] = np.full(2 * TILE + 1, last)
    lab = rng.choice([c for c in range(C) if c != 2], 1500)
    assert (lab != 2).all() and len(np.unique(lab)) == C - 1
    out["class_2_absent"] = lab
    return out


@pytest.mark.parametrize("C", [4, 8])
@pytest.mark.parametrize("D", [260, 65])  # VEC2, scalar
def test_gnb_classes_around_the_tile_edge(ce, D, C):
    rng = np.random.default_rng(10 * D + C)
    F = 600
    Xd, X = frames(rng, F, D)
    start = fitted_state(rng, C, D, unseen=(C - 1,))
    assert start[2][C - 1] == 0
    bad = []
    for name, labels in labels_around_the_tile_edge(rng, C).items():
        rows = rng.integers(0, F, len(labels))
        st = GnbState(*start)
        st.fit(ce.ops, Xd, rows, labels)
        got = st.host()
        want = gnb_partial_fit(X[rows], labels, *start)
        diff = differing(got, want)
        th, va, cc, _, eps = got
        if name == "unseen_class_is_the_one_row_of_tile_2":  # new_var == 0, taken as it is: var = 0 + epsilon
            diff += [k for k, ok in (("theta as is", same_bits(th[C - 1], X[rows[TILE]])),
                                     ("var as is", same_bits(va[C - 1], np.full(D, 0.0 + eps[0]))),
                                     ("count", cc[C - 1] == 1.0)) if not ok]
        if name == "class_2_absent":  # keeps theta and its count, var - eps + eps
            diff += [k for k, ok in (("theta kept", same_bits(th[2], start[0][2])),
                                     ("var - eps + eps", same_bits(va[2], (start[1][2] - eps[0]) + eps[0])),
                                     ("count kept", cc[2] == start[2][2])) if not ok]
        if diff:
            bad.append((name, diff))
    assert not bad, f"D={D} C={C}: {report(bad)}"


@pytest.mark.parametrize("D", [260, 65])
def test_gnb_values_across_tiles(ce, D):
    """n = 1025: a -0.0 column, a column x 1e150 and a column x 1e-150 summed
    across the tile edge; then one NaN cell in the frame at batch position 1024
    only, the single row of tile 2: epsilon and every var are NaN."""
    rng = np.random.default_rng(D)
    F, C, n = 600, 4, TILE + 1
    _, X = frames(rng, F, D)
    X[:, 0] = -0.0
    X[:, 1] = rng.normal(0, 1, F) * 1e150  # squares near 1e300: the sums of 1025 of them stay finite
    X[:, 2] = rng.normal(0, 1, F) * 1e-150
    th, va, cc = fitted_state(rng, C, D, unseen=(C - 1,))
    th[:, 0] = -0.0
    th[:, 1] *= 1e150
    va[:, 1] *= 1e300
    th[:, 2] *= 1e-150
    rows = np.concatenate([rng.integers(0, F - 1, TILE), [F - 1]])  # frame F - 1 at position 1024 only
    labels = rng.integers(0, C, n)
    assert (rows[:TILE] != F - 1).all() and rows[TILE] == F - 1 and len(np.unique(labels)) == C
    st = GnbState(th, va, cc)
    st.fit(ce.ops, dev(X), rows, labels)
    want = gnb_partial_fit(X[rows], labels, th, va, cc)
    assert np.isfinite(want[4]) and np.isfinite(want[1]).all() and want[4] > 1e280  # the 1e150 column's epsilon
    assert not differing(st.host(), want), (D, "finite", differing(st.host(), want))
    X[F - 1, D - 1] = np.nan
    st.fit(ce.ops, dev(X), rows, labels)
    want = gnb_partial_fit(X[rows], labels, *want[:3])
    assert np.isnan(want[4]) and np.isnan(want[1]).all()
    got = st.host()
    assert not differing(got, want), (D, "nan", differing(got, want))
    assert np.isnan(got[4]).all() and np.isnan(got[1]).all()


# ---------------------------------------------------------------------------
# 3. GaussianNB: ragged models in one launch (0, 1, 2 and 3 tile trips)
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("order", ["given", "reversed"])
def test_gnb_ragged_models_in_one_launch(ce, order):
    rng = np.random.default_rng(33 + (order == "given"))
    F, C, D = 600, 4, 260
    n = np.array([1025, 0, 40, 2049, 1, 1024])
    if order == "reversed":
        n = n[::-1]
    U = len(n)
    assert sorted(-(-n // TILE)) == [0, 1, 1, 1, 2, 3]  # tile trips of the launch's blocks
    Xd, X = frames(rng, F, D)
    states = [fitted_state(rng, C, D, unseen=(C - 1,) if u % 2 else ()) for u in range(U)]
    ro = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rows, labels = rng.integers(0, F, ro[-1]), rng.integers(0, C, ro[-1]).astype(np.int32)
    st = GnbState(*[np.stack([s[i] for s in states]) for i in range(3)])
    st.prior.copy_(dev(rng.random(st.prior.shape)))  # the empty model's outputs must keep these
    st.eps.copy_(dev(rng.random(st.eps.shape)))
    before = st.host()
    st.fit(ce.ops, Xd, rows, labels, row_offsets=dev(ro))
    got = st.host()
    bad = []
    for u in range(U):
        mine = [g[u] for g in got]
        if n[u] == 0:
            diff = differing(mine, [b[u] for b in before])
        else:
            r, l = rows[ro[u]:ro[u + 1]], labels[ro[u]:ro[u + 1]]
            diff = differing(mine, gnb_partial_fit(X[r], l, *states[u]))
        if diff:
            bad.append(((u, int(n[u])), diff))
    assert not bad, f"(model, rows) {report(bad)}"


# ---------------------------------------------------------------------------
# 4. SGD: batch size x width x problems
# ---------------------------------------------------------------------------
SGD_SIZES = [4, 5, 7, 8, 9, 12, 13, 127, 128, 129, 191, 192, 193, 255, 256, 257, 1025]


def sgd_one(ce, Xd, X, n, C, start, seeds, rng):
    """One model's partial_fit on n rows drawn from X against the restatement: the outputs that differ."""
    rows, labels = rng.integers(0, len(X), n), rng.integers(0, C, n)
    st = SgdState(*start)
    st.fit(ce.ops, Xd, rows, labels, seeds)
    want = sgd_partial_fit(X[rows], labels, *start, seeds=seeds)
    assert want[3]  # finite
    return differing(st.host(), want[:3], SGD_NAMES) + ([("status", st.status.tolist())] if st.status.tolist() != [0] else [])


@pytest.mark.parametrize("D,C", [(512, 8), (260, 4), (65, 3), (9, 2)])  # 64 / 33 / 9 / 2 lanes own features; 8 / 4 / 3 / 1 waves
def test_sgd_batch_sizes(ce, D, C):
    """The two-chunk loop's tail (n % 8 = 1 .. 7), the first roll of the 64-row
    metadata at row 64 seen from n = 127 .. 129, the second and third at
    191 .. 257, and 16 rolls at n = 1025; fresh seeds for every size."""
    rng = np.random.default_rng(1000 * D + C)
    F, K = 600, 1 if C == 2 else C
    Xd, X = frames(rng, F, D, spread=0.5)
    start = model(rng, C, D)
    bad = []
    for n in SGD_SIZES:
        in_lds = K * n <= PERM_LDS
        assert in_lds == (ce.load().ce_sgd_partial_fit_workspace_bytes(n, C) == 0)
        assert in_lds or (C, n) == (8, 1025)  # 8 x 1025 = 8200 indices: this one size keeps them in the workspace
        diff = sgd_one(ce, Xd, X, n, C, start, chain_seeds(100 * n + C, C), rng)
        if diff:
            bad.append((n, diff))
    assert not bad, f"D={D} C={C}: {report(bad)}"


def test_sgd_workspace_path_at_full_width(ce):
    """D = 260, C = 8, n = 1025: the permutations live in the workspace, every wave of the block runs."""
    rng = np.random.default_rng(2608)
    D, C, n = 260, 8, 1025
    assert ce.load().ce_sgd_partial_fit_workspace_bytes(n, C) == 4 * C * n > 4 * PERM_LDS
    Xd, X = frames(rng, 600, D, spread=0.5)
    diff = sgd_one(ce, Xd, X, n, C, model(rng, C, D), chain_seeds(2608, C), rng)
    assert not diff, diff


def test_sgd_ragged_models_in_one_launch(ce):
    """Blocks of one launch roll the metadata 0, 1, 2 and 4 times; the empty model's coef, intercept and t stay."""
    rng = np.random.default_rng(44)
    F, C, D = 600, 8, 260
    n = np.array([129, 0, 64, 257, 1, 128])
    U = len(n)
    Xd, X = frames(rng, F, D, spread=0.5)
    ro = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rows, labels = rng.integers(0, F, ro[-1]), rng.integers(0, C, ro[-1]).astype(np.int32)
    models =[model(rng, C, D) for _ in range(U)]
    seeds = np.stack([chain_seeds(500 + u, C) for u in range(U)])
    assert len({tuple(s) for s in seeds}) == U
    st = SgdState(*[np.stack([m[i] for m in models]) for i in range(3)])
    st.fit(ce.ops, Xd, rows, labels, seeds, row_offsets=dev(ro))
    got = st.host()
    bad = []
    for u in range(U):
        r, l = rows[ro[u]:ro[u + 1]], labels[ro[u]:ro[u + 1]]
        want = models[u] if n[u] == 0 else sgd_partial_fit(X[r], l, *models[u], seeds=seeds[u])[:3]
        diff = differing([g[u] for g in got], want, SGD_NAMES)
        if diff:
            bad.append(((u, int(n[u])), diff))
    assert not bad, f"(model, rows) {report(bad)}"
    assert st.status.tolist() == [0] * U


# ---------------------------------------------------------------------------
# 5. Through the member classes: a session's picks give more than 1024 rows
# ---------------------------------------------------------------------------
D_M, C_M = 260, 4


def song_pool(rng, frames_per_song):
    """Songs of the given frame counts in shuffled frame order: (s_id [F], X [F, D], song_labels)."""
    n_songs = len(frames_per_song)
    s_id = rng.permutation(np.repeat(np.arange(n_songs), frames_per_song))
    song_labels = rng.permutation(np.arange(n_songs) % C_M)
    centers = rng.normal(0, 1, (C_M, D_M))
    X = centers[song_labels[s_id]] + rng.normal(0, 2.0, (len(s_id), D_M))
    return s_id, X, song_labels


def member_states(s, u):
    return [s[k][u] for k in NAMES]


def test_members_one_user_past_the_tile(ce):
    """One user, 40 songs of 30-40 frames, 32 of them picked: X_batch is X[isin(s_id, picks)], rows in X's order."""
    rng = np.random.default_rng(5)
    N, q = 40, 32
    s_id, X, song_labels = song_pool(rng, rng.integers(30, 41, N))
    picks = rng.permutation(N)[:q].astype(np.int64)
    batch = np.isin(s_id, picks)
    assert batch.sum() > TILE and (np.diff(s_id[batch]) != 0).sum() > TILE // 2  # shuffled: the songs' rows interleave
    y = song_labels[s_id[batch]]
    Xd = dev(X)
    sess = ce.SelectionSession(q, "mc", N, s_id=s_id)
    start = fitted_state(rng, C_M, D_M, unseen=(C_M - 1,))
    nb = ce.DeviceGaussianNB(*start)
    nb.partial_fit_picks(Xd, sess, picks, song_labels)
    diff = differing(member_states(nb.state(), 0), gnb_partial_fit(X[batch], y, *start))
    assert not diff, ("gnb", diff)
    init = model(rng, C_M, D_M)
    m = ce.DeviceSGDClassifier(*init, random_state=12)
    m.partial_fit_picks(Xd, sess, picks, song_labels)
    s = m.state()
    want = sgd_partial_fit(X[batch], y, *init, random_state=12)
    assert want[3]
    diff = differing((s["coef"][0], s["intercept"][0], s["t"]), want[:3], SGD_NAMES)
    assert not diff, ("sgd", diff)
    m.check_finite()


def test_members_batched_users_past_and_below_the_tile(ce):
    """Two users in one launch: one whose picks give more than 1024 rows, one with fewer than 100."""
    rng = np.random.default_rng(6)
    users = [40, 10]
    off = np.array([0, 40, 50], np.int64)
    s_id, X, song_labels = song_pool(rng, np.concatenate([rng.integers(30, 41, 40), rng.integers(1, 10, 10)]))
    picks = [rng.permutation(users[0])[:32].astype(np.int64), rng.permutation(users[1])[:3].astype(np.int64)]  # user-local
    batches = [np.isin(s_id, off[u] + picks[u]) for u in range(2)]
    assert batches[0].sum() > TILE and 0 < batches[1].sum() < 100
    _, f_off, f_perm = ce.song_groups(s_id)
    sess = ce.BatchedSelectionSession(32, "mc", off, frame_offsets=f_off, frame_perm=f_perm)
    Xd = dev(X)
    starts = [fitted_state(rng, C_M, D_M, unseen=(C_M - 1,) if u else ()) for u in range(2)]
    nb = ce.DeviceGaussianNB(*[np.stack([s[i] for s in starts]) for i in range(3)])
    nb.partial_fit_picks(Xd, sess, picks, song_labels)
    inits = [model(rng, C_M, D_M) for _ in range(2)]
    m = ce.DeviceSGDClassifier(*[np.stack([s[i] for s in inits]) for i in range(3)], random_state=[7, 8])
    m.partial_fit_picks(Xd, sess, picks, song_labels)
    gs, ss = nb.state(), m.state()
    bad = []
    for u in range(2):
        Xb, y = X[batches[u]], song_labels[s_id[batches[u]]]
        diff = differing(member_states(gs, u), gnb_partial_fit(Xb, y, *starts[u]))
        want = sgd_partial_fit(Xb, y, *inits[u], random_state=7 + u)
        assert want[3]
        diff += differing((ss["coef"][u], ss["intercept"][u], ss["t"][u]), want[:3], SGD_NAMES)
        if diff:
            bad.append(((u, int(batches[u].sum())), diff))
    assert not bad, f"(user, rows) {report(bad)}"
    m.check_finite()
