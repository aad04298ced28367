"""GPU parity of the XGBoost users form (ce_xgb_predict_proba_users,
ce_xgb_score_users, ce_amd.DeviceXGBClassifier): every owned row equals, BIT
FOR BIT, both the oracle on that user's full JSON model and the one-forest
ops.xgb_predict_proba on the same rows; rows not owned, excluded or out of
range keep the sentinel the test wrote.  The bar is exactness: the traversal
is comparisons and the margins the same float32 chain in model order."""
import numpy as np
import pytest

from ce_amd.xgb import StackedForests, XgbForest, continued_model, synthetic_model
from members_eval_ref import confusion, f1_weighted
from xgb_users_ref import (bits, drop_group, expected_proba, geometry, leaves_model, plant_thresholds, predict_labels,
                           user_models)

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
SENT = np.float32(-7.0)


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


def mk(seed, rounds, depth=5, num_class=4, D=260, **kw):
    return synthetic_model(n_rounds=rounds, num_class=num_class, max_depth=depth, num_feature=D, seed=seed, **kw)


def make_X(F, D, owner, models, seed, nan=0.0):
    rng = np.random.default_rng(seed)
    X = rng.normal(size=(F, D))
    for u, m in enumerate(models):
        plant_thresholds(X, np.flatnonzero(owner == u), m)
    if nan:
        X[rng.random(X.shape) < nan] = np.nan
    return X


def excl_words(songs, n):
    w = np.zeros(max((n + 31) // 32, 1), np.uint32)
    for g in songs:
        w[g >> 5] |= np.uint32(1) << np.uint32(g & 31)
    return dev(w.view(np.int32))


def check(ce, base, models, X, items, f_off, perm, owner, excl=None, written=None, out_dtype=torch.float32, Xd=None,
          ldo=None):
    """One batched launch into a sentinel-filled out against both expected values."""
    C = XgbForest.from_json(base).n_classes
    F = X.shape[0]
    Xd = dev(X) if Xd is None else Xd
    exp = expected_proba(X, owner, models)
    for u, m in enumerate(models):  # the one-forest launch on the same rows
        rows = np.flatnonzero(owner == u)
        if rows.size:
            one = ce.ops.xgb_predict_proba(Xd[dev(rows)].contiguous(), XgbForest.from_json(m)).cpu().numpy()
            assert np.array_equal(bits(one), bits(exp[rows])), u
    full = torch.full((F, ldo or C), float(SENT), dtype=out_dtype, device="cuda")
    out = full[:, :C]
    st = StackedForests(base, models)
    got = ce.ops.xgb_predict_proba_users(Xd, st, dev(items), dev(f_off), None if perm is None else dev(perm),
                                         excl=excl, out=out)
    assert got.data_ptr() == out.data_ptr() and ce._lib.load().ce_last_kernel().startswith(b"ce::k_xgb_users<")
    got = full.cpu().numpy()
    written = (owner >= 0) if written is None else written
    if out_dtype == torch.float64:
        assert np.array_equal(got[written, :C], exp[written].astype(np.float64))
    else:
        assert np.array_equal(bits(got[written, :C]), bits(exp[written])), np.argwhere(
            bits(got[written, :C]) != bits(exp[written]))[:5]
    assert np.all(got[~written] == SENT) and np.all(got[:, C:] == SENT)
    return st, exp


# ---- user geometry ----------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["grouped", "shuffled"])
def test_user_geometry(ce, shuffled):
    """Users of 0, 1, 63, 64, 65, 129 and 257 frames, a user without a song,
    songs without a frame, rows no song owns, frame_perm entries out of range."""
    per_user = [[1], [], [63], [0, 64, 0], [30, 35], [129], [0], [100, 157]]  # frames of every user's songs
    frames_per_song = [f for s in per_user for f in s]
    n, F = sum(frames_per_song), sum(frames_per_song) + 50
    items, f_off, perm, owner, _ = geometry(frames_per_song, [len(s) for s in per_user], F=F if shuffled else None,
                                            shuffled=shuffled, seed=3)
    if not shuffled:  # the tail rows are owned by no song
        owner = np.concatenate([owner, np.full(F - n, -1, np.int64)])
    base = mk(1, 13)
    models = user_models(base, [mk(10 + u, r) for u, r in enumerate([3, 1, 9, 24, 2, 30, 4, 11])])
    X = make_X(F, 260, owner, models, seed=5)
    if shuffled:  # two positions name rows outside [0, F): skipped, and their rows stay unowned
        for pos, bad in ((5, -1), (200, F + 7)):
            owner[perm[pos]] = -1
            perm[pos] = bad
    check(ce, base, models, X, items, f_off, perm, owner)


def test_three_hundred_users_of_three_frames(ce):
    """One block's share crosses many users; six distinct forests."""
    base = mk(2, 3, depth=3, D=20)
    kinds = user_models(base, [mk(20 + k, 1 + k, depth=3, D=20) for k in range(5)]) + [None]
    models = [kinds[u % 6] for u in range(300)]
    items, f_off, perm, owner, _ = geometry([3] * 300, [1] * 300, shuffled=True, seed=4)
    exp_models = [base if m is None else m for m in models]
    X = make_X(900, 20, owner, exp_models[:6], seed=6)
    st, _ = check(ce, base, exp_models, X, items, f_off, perm, owner)
    assert st.U == 300


def test_one_user_over_several_blocks(ce):
    base = mk(3, 5, D=77)
    models = user_models(base, [mk(30, 4, D=77), mk(31, 2, D=77)])
    items, f_off, perm, owner, _ = geometry([700, 301, 40], [2, 1])
    check(ce, base, models, make_X(1041, 77, owner, models, seed=7), items, f_off, perm, owner)


# ---- tree counts at the wave-split edges ----------------------------------------------------
@pytest.mark.parametrize("num_class", [4, 3, 8, 2], ids=["G4", "G3", "G8", "binary"])
def test_tree_counts_per_group(ce, num_class):
    """n trees per group at the edges of split_margins (S = 16 / G waves,
    kXgbChunk = 24) over a base of 13 per group: a batch of 8 straddles base
    and tail rows; tail-only (no continuation), base-only and empty-group users
    in one launch."""
    G = 1 if num_class == 2 else num_class
    S, D = 16 // G, 77
    base = mk(40, 13, num_class=num_class, D=D)
    counts = sorted({1, 7, 8, 9, 24 * (S - 1), 24 * (S - 1) + 1, 100, 137})
    models = []
    for i, n in enumerate(counts):
        if n > 13:
            models.append(continued_model(base, mk(41 + i, n - 13, num_class=num_class, D=D)))
        else:
            models.append(mk(41 + i, n, num_class=num_class, D=D))  # tail-only
    models.append(base)  # base-only
    if G > 1:
        models.append(drop_group(mk(60, 9, num_class=num_class, D=D), 1))  # n = 0 in group 1
        models.append(continued_model(base, drop_group(mk(61, 30, num_class=num_class, D=D), G - 1)))
    U = len(models)
    items, f_off, perm, owner, _ = geometry([70] * U, [1] * U)
    X = make_X(70 * U, D, owner, models, seed=8, nan=0.02)
    check(ce, base, models, X, items, f_off, perm, owner)


@pytest.mark.parametrize("num_class", [2, 4], ids=["binary", "softprob"])
def test_user_without_a_tree(ce, num_class):
    """n = 0 in every group: a user whose model holds no tree predicts the
    objective's transform of the base margin alone -- also in the binary G = 1
    launch.  The oracle cannot read an empty forest, so that user's expected
    rows come from one round of zero leaves (base + 0.0, the same margin bits
    through the same transform); the other users' from their own models."""
    D, G = 30, 1 if num_class == 2 else num_class
    base = mk(65, 13, num_class=num_class, D=D)
    empty = mk(66, 0, num_class=num_class, D=D)
    assert len(empty["learner"]["gradient_booster"]["model"]["trees"]) == 0
    zero = leaves_model([[0.0] * G], num_class, num_feature=D)
    models = [empty, continued_model(base, mk(67, 30, num_class=num_class, D=D)), empty, base]
    items, f_off, perm, owner, _ = geometry([70, 65, 3, 64], [1, 1, 1, 1], shuffled=True, seed=21)
    X = make_X(202, D, owner, [zero, models[1], zero, base], seed=22, nan=0.02)
    exp = expected_proba(X, owner, [zero, models[1], zero, base])
    st = StackedForests(base, models)
    G_off = st.group_offsets
    assert np.all(G_off[:G + 1] == 0) and np.all(G_off[2 * G:3 * G + 1] == G_off[2 * G])  # users 0 and 2 own no tree
    y = np.random.default_rng(23).integers(0, num_class, 202).astype(np.int32)
    out = torch.full((202, num_class), float(SENT), dtype=torch.float32, device="cuda")
    ce.ops.xgb_predict_proba_users(dev(X), st, dev(items), dev(f_off), dev(perm), out=out)
    assert np.array_equal(bits(out.cpu().numpy()), bits(exp))
    want = 0.5 if num_class == 2 else 0.25
    assert np.all(exp[owner == 0] == np.float32(want)) and np.all(exp[owner == 2] == np.float32(want))
    cm, pred, _ = ce.ops.xgb_score_users(dev(X), st, dev(items), dev(f_off), dev(y), dev(perm), return_pred=True)
    labels = predict_labels(exp, binary=num_class == 2)
    assert np.array_equal(pred.cpu().numpy(), labels) and np.all(labels[owner == 0] == 0)  # p == 0.5 / a four-way tie
    assert np.array_equal(cm.cpu().numpy(), confusion(y, labels, num_class, user=owner, U=4))


@pytest.mark.parametrize("db,dt", [(0, 0), (1, 1), (3, 3), (5, 5), (5, 3), (1, 4)],
                         ids=["d0", "d1", "d3", "d5", "d3_tail_over_d5", "d4_tail_over_d1"])
def test_depths(ce, db, dt):
    base = mk(70, 6, depth=db, D=50, p_stop=0.0)
    models = user_models(base, [mk(71, 5, depth=dt, D=50, p_stop=0.0), None, mk(72, 11, depth=dt, D=50)])
    items, f_off, perm, owner, _ = geometry([65, 64, 66], [1, 1, 1])
    st, _ = check(ce, base, models, make_X(195, 50, owner, models, seed=9, nan=0.05), items, f_off, perm, owner)
    assert st.depth == max(db, dt)


@pytest.mark.parametrize("f32", [False, True], ids=["f64", "f32"])
@pytest.mark.parametrize("D", [1, 2, 77, 200, 259, 260, 400, 512])
def test_feature_widths(ce, D, f32):
    """Every staging width (KF 2 / 4 / 5 / 8), the f64 pair loads and their odd-D tail, D = 1."""
    base = mk(80 + D, 4, depth=3, D=D)
    models = user_models(base, [mk(81 + D, 3, depth=3, D=D), mk(82 + D, 2, depth=3, D=D)])
    items, f_off, perm, owner, _ = geometry([70, 59], [1, 1], shuffled=True, seed=D)
    X = make_X(129, D, owner, models, seed=D, nan=0.02)
    if f32:
        X = X.astype(np.float32).astype(np.float64)
        check(ce, base, models, X, items, f_off, perm, owner, Xd=dev(X.astype(np.float32)))
    else:
        check(ce, base, models, X, items, f_off, perm, owner)


def test_missing_values_and_layout(ce):
    """Dense tiles and one user's tile with NaN in one launch; f64 out as the exact upcast; ld > D; ld_out > C."""
    base = mk(90, 20)
    models = user_models(base, [mk(91, 7), mk(92, 9), None])
    items, f_off, perm, owner, _ = geometry([128, 64, 100], [1, 1, 1])
    X = make_X(292, 260, owner, models, seed=10)
    X[130:190:7, 5] = np.nan  # user 1's only tile
    wide = dev(np.concatenate([X, np.full((292, 9), 3.0)], 1))[:, :260]
    assert wide.stride(0) == 269
    check(ce, base, models, X, items, f_off, perm, owner, Xd=wide)
    check(ce, base, models, X, items, f_off, perm, owner, out_dtype=torch.float64, ldo=7)
    check(ce, base, models, X, items, f_off, perm, owner, ldo=6)
    # a new out: float32 by default, float64 on request, zero where excluded
    st = StackedForests(base, models)
    o = ce.ops.xgb_predict_proba_users(dev(X), st, dev(items), dev(f_off), excl=excl_words([1], 3))
    assert o.dtype == torch.float32 and np.all(o.cpu().numpy()[128:192] == 0)
    o64 = ce.ops.xgb_predict_proba_users(dev(X), st, dev(items), dev(f_off), out_dtype=torch.float64)
    assert o64.dtype == torch.float64 and np.array_equal(o64.cpu().numpy()[:128], o.cpu().numpy()[:128].astype(np.float64))
    with pytest.raises(ValueError, match="float32/float64"):
        ce.ops.xgb_predict_proba_users(dev(X), st, dev(items), dev(f_off), out=torch.zeros((292, 4), dtype=torch.int32,
                                                                                       device="cuda"))
    with pytest.raises(ValueError, match=r"2 user\(s\).*3 forest"):
        ce.ops.xgb_predict_proba_users(dev(X), st, dev(items[:3]), dev(f_off))


# ---- exclusion --------------------------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True], ids=["grouped", "shuffled"])
def test_excluded_songs_are_not_written(ce, shuffled):
    """Whole tiles excluded (songs of 64+ frames), partial tiles, every song of a user."""
    songs = [64, 64, 10, 130, 5, 20, 30, 64, 7, 100]
    items, f_off, perm, owner, song = geometry(songs, [3, 2, 3, 2], shuffled=shuffled, seed=11)
    base = mk(100, 6, D=77)
    models = user_models(base, [mk(101 + u, 3 + u, D=77) for u in range(4)])
    X = make_X(sum(songs), 77, owner, models, seed=12)
    gone = [0, 3, 5, 6, 7, 9]  # user 2 keeps nothing, song 0 and 3 cover whole tiles
    check(ce, base, models, X, items, f_off, perm, owner, excl=excl_words(gone, len(songs)),
          written=(owner >= 0) & ~np.isin(song, gone))


def test_session_bitmap_and_skip_excluded(ce):
    """The session's own bitmap after a select: the picked songs' rows are not
    written; skip_excluded=False writes every owned row."""
    rng = np.random.default_rng(13)
    songs_per_user = [6, 5, 7]
    T = sum(songs_per_user)
    s_id = rng.permutation(np.repeat(np.arange(T), rng.integers(20, 90, T)))
    F = len(s_id)
    off = np.concatenate([[0], np.cumsum(songs_per_user)]).astype(np.int64)
    owner = np.searchsorted(off, s_id, side="right") - 1
    base = mk(110, 8, D=40)
    models = user_models(base, [mk(111, 4, D=40), None, mk(112, 6, D=40)])
    X = make_X(F, 40, owner, models, seed=14)
    exp = expected_proba(X, owner, models)
    _, f_off, f_perm = ce.song_groups(s_id)
    sess = ce.BatchedSelectionSession(2, "mc", off, frame_offsets=f_off, frame_perm=f_perm)
    member = ce.DeviceXGBClassifier(base, models)
    Xd = dev(X)
    buf = member.predict_proba_session(Xd, sess)
    assert buf.dtype == torch.float32 and np.array_equal(bits(buf.cpu().numpy()), bits(exp))
    idx = sess.step(frames=[buf])
    picked = np.concatenate([np.asarray(p)[np.asarray(p) >= 0] + off[u] for u, p in enumerate(sess.account(idx))])
    assert picked.size == 6
    out = torch.full((F, 4), float(SENT), dtype=torch.float32, device="cuda")
    member.predict_proba_session(Xd, sess, out=out)
    got, gone = out.cpu().numpy(), np.isin(s_id, picked)
    assert np.array_equal(bits(got[~gone]), bits(exp[~gone])) and np.all(got[gone] == SENT)
    member.predict_proba_session(Xd, sess, out=out, skip_excluded=False)
    assert np.array_equal(bits(out.cpu().numpy()), bits(exp))
    with pytest.raises(ValueError, match="is on cpu"):  # the tables live on the member's device
        member.predict_proba_session(Xd.cpu(), sess)
    for u in range(3):  # predict_proba(X, u): the one-forest path
        rows = np.flatnonzero(owner == u)
        one = member.predict_proba(Xd[dev(rows)].contiguous(), u).cpu().numpy()
        assert np.array_equal(bits(one), bits(exp[rows]))


# ---- score ------------------------------------------------------------------------------------
def run_score(ce, base, models, X, y, items, f_off, perm, excl=None):
    st = StackedForests(base, models)
    cm, pred, proba = ce.ops.xgb_score_users(dev(X), st, dev(items), dev(f_off), dev(y), None if perm is None else dev(perm),
                                             excl=excl, return_pred=True, return_proba=True)
    assert ce._lib.load().ce_last_kernel().startswith(b"ce::k_xgb_score_users<")
    return st, cm.cpu().numpy(), pred.cpu().numpy(), proba.cpu().numpy()


@pytest.mark.parametrize("num_class", [4, 2], ids=["softprob", "binary"])
def test_score_users(ce, num_class):
    """pred = the numpy rule on the expected float32 probabilities, cm = np.add.at,
    proba = the predict launch's bits, labels outside [0, C) and excluded songs
    not counted, f1 = members_eval_ref's restatement."""
    C = num_class
    songs = [40, 64, 25, 70, 3, 90, 12]
    items, f_off, perm, owner, song = geometry(songs, [2, 3, 0, 2], F=sum(songs) + 9, shuffled=True, seed=15)
    base = mk(120, 10, num_class=num_class, D=77)
    models = user_models(base, [mk(121 + u, 2 + 3 * u, num_class=num_class, D=77) for u in range(3)]) + [base]
    F = sum(songs) + 9
    X = make_X(F, 77, owner, models, seed=16, nan=0.01)
    rng = np.random.default_rng(17)
    y = rng.integers(0, C, F).astype(np.int32)
    y[::11] = C
    y[5::13] = -1
    exp = expected_proba(X, owner, models)
    counted = (owner >= 0) & (song != 3) & (y >= 0) & (y < C)
    st, cm, pred, proba = run_score(ce, base, models, X, y, items, f_off, perm, excl=excl_words([3], len(songs)))
    want = predict_labels(exp, binary=C == 2)
    assert np.array_equal(pred[counted], want[counted]) and np.all(pred[~counted] == -1)
    assert np.array_equal(bits(proba[counted]), bits(exp[counted])) and np.all(np.isnan(proba[~counted]))
    assert np.array_equal(cm, confusion(y[counted], want[counted], C, user=owner[counted], U=4))
    out = ce.ops.xgb_predict_proba_users(dev(X), st, dev(items), dev(f_off), dev(perm)).cpu().numpy()
    assert np.array_equal(bits(out[counted]), bits(proba[counted]))
    f1, prf = ce.ops.f1_weighted_users(dev(cm), report=True)
    for u in range(4):
        e = f1_weighted(cm[u])
        assert np.array_equal(np.float64(f1[u].item()).view(np.uint64), np.float64(e).view(np.uint64)) or (
            np.isnan(e) and np.isnan(f1[u].item()))


def test_score_ties_half_and_nan_on_the_device(ce):
    """An exact tie of float32 probabilities (first index), binary p exactly 0.5
    (class 0), NaN probabilities (a NaN wins at its first occurrence; binary: class 0)."""
    items, f_off, perm, owner, _ = geometry([5, 5], [1, 1])
    X, y = np.zeros((10, 4)), np.zeros(10, np.int32)
    tie, nanm = leaves_model([[-1.0, 0.75, 0.75, 0.75]], 4), leaves_model([[np.inf, 0.0, -np.inf, 1.0]], 4)
    _, cm, pred, proba = run_score(ce, tie, [tie, nanm], X, y, items, f_off, perm)
    assert bits(proba)[0, 1] == bits(proba)[0, 2] == bits(proba)[0, 3] and np.all(pred[:5] == 1)
    assert np.all(np.isnan(proba[5:])) and np.all(pred[5:] == 0)  # inf - inf: the whole softmax row is NaN
    assert cm[0, 0, 1] == 5 and cm[1, 0, 0] == 5 and cm.sum() == 10
    half = leaves_model([[0.0]], 2)
    above = leaves_model([[2.0 ** -20]], 2)
    nanb = leaves_model([[np.inf], [-np.inf]], 2)
    items, f_off, perm, owner, _ = geometry([3, 3, 3], [1, 1, 1])
    _, cm, pred, proba = run_score(ce, half, [half, above, nanb], np.zeros((9, 4)), np.ones(9, np.int32), items, f_off,
                                   perm)
    assert np.all(proba[:3, 1] == np.float32(0.5)) and np.all(pred[:3] == 0)
    assert np.all(proba[3:6, 1] > np.float32(0.5)) and np.all(pred[3:6] == 1)
    assert np.all(np.isnan(proba[6:, 1])) and np.all(pred[6:] == 0)
    assert [cm[u, 1].tolist() for u in range(3)] == [[3, 0], [0, 3], [3, 0]]


def test_zero_frames(ce):
    base = mk(130, 2, D=10)
    st = StackedForests(base, [None, None])
    X = torch.empty((0, 10), dtype=torch.float64, device="cuda")
    z = dev(np.zeros(3, np.int64))
    assert tuple(ce.ops.xgb_predict_proba_users(X, st, z, dev(np.zeros(1, np.int64))).shape) == (0, 4)
    cm, _, _ = ce.ops.xgb_score_users(X, st, z, dev(np.zeros(1, np.int64)), torch.empty(0, dtype=torch.int32, device="cuda"))
    assert tuple(cm.shape) == (2, 4, 4) and int(cm.abs().sum()) == 0


# ---- the loop ---------------------------------------------------------------------------------
Q, EPOCHS, C_LOOP, D_LOOP = 3, 3, 4, 20
SONGS = [9, 8, 12, 10]


def loop_data(rng, mode):
    U = len(SONGS)
    off = np.concatenate([[0], np.cumsum(SONGS)]).astype(np.int64)
    T = int(off[-1])
    s_id = rng.permutation(np.repeat(np.arange(T), rng.integers(1, 30, T)))
    owner = np.searchsorted(off, s_id, side="right") - 1
    X = rng.normal(0, 1, (len(s_id), D_LOOP))
    song_labels = rng.integers(0, C_LOOP, T)
    t_off = np.concatenate([[0], np.cumsum(rng.integers(2, 5, U))]).astype(np.int64)
    t_sid = rng.permutation(np.repeat(np.arange(int(t_off[-1])), rng.integers(5, 40, int(t_off[-1]))))
    t_owner = np.searchsorted(t_off, t_sid, side="right") - 1
    Xt, yt = rng.normal(0, 1, (len(t_sid), D_LOOP)), rng.integers(0, C_LOOP, len(t_sid)).astype(np.int32)
    kw = {}
    if mode == "mix":
        tabs = []
        for n in SONGS:
            n_rows = int(0.8 * n) + 2
            m = np.concatenate([rng.permutation(n)[:n_rows - 2], np.full(2, -1)])[rng.permutation(n_rows)].astype(np.int64)
            tabs.append((np.round(rng.dirichlet(np.ones(4), n_rows), 1), m))
        off_h = np.concatenate([[0], np.cumsum([len(t[1]) for t in tabs])]).astype(np.int64)
        kw = dict(hc=np.concatenate([t[0] for t in tabs]), hc_offsets=off_h, hc_to_mc=np.concatenate([t[1] for t in tabs]))
    gnb0 = [np.stack([rng.normal(0, 0.5, (C_LOOP, D_LOOP)) for _ in range(U)]),
            np.stack([(rng.random((C_LOOP, D_LOOP)) + 0.5) * 4.0 for _ in range(U)]),
            np.stack([rng.integers(1, 50, C_LOOP).astype(np.float64) for _ in range(U)])]
    sgd0 = [np.stack([rng.normal(0, 0.5, (C_LOOP, D_LOOP)) for _ in range(U)]),
            np.stack([rng.normal(0, 0.5, C_LOOP) for _ in range(U)]), rng.integers(2, 5000, U).astype(np.float64)]
    return dict(off=off, s_id=s_id, owner=owner, X=X, song_labels=song_labels, t_off=t_off, t_sid=t_sid,
                t_owner=t_owner, Xt=Xt, yt=yt, kw=kw, gnb0=gnb0, sgd0=sgd0)


def loop_build(ce, d, mode, base):
    _, f_off, f_perm = ce.song_groups(d["s_id"])
    sess = ce.BatchedSelectionSession(Q, mode, d["off"], frame_offsets=f_off, frame_perm=f_perm, **d["kw"])
    nb = ce.DeviceGaussianNB(*d["gnb0"])
    sg = ce.DeviceSGDClassifier(*d["sgd0"], random_state=[7, 8, 9, 10])
    xg = ce.DeviceXGBClassifier(base, U=len(SONGS))
    F = len(d["s_id"])
    bufs = [torch.zeros((F, C_LOOP), dtype=torch.float64, device="cuda") for _ in range(2)]
    bufs.append(torch.zeros((F, C_LOOP), dtype=torch.float32, device="cuda"))
    return sess, nb, sg, xg, bufs


def refit(e, u):
    return mk(1000 + 10 * e + u, 2 + (e + u) % 3, depth=3 + (u % 3), D=D_LOOP)


@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_three_epochs_with_three_members(ce, mode):
    """predict (three launches), step(frames=[...]), the linear retrains on the
    device, the XGB refit emulated per user (continued_model + set_model), every
    member evaluated and mean_f1 taken: the batched XGB member against the
    per-user loop through the one-forest entry point, bit for bit."""
    rng = np.random.default_rng(200 + len(mode))
    d = loop_data(rng, mode)
    U = len(SONGS)
    base = mk(140, 6, D=D_LOOP)
    Xd, labels_d = dev(d["X"]), dev(d["song_labels"].astype(np.int64))
    es = ce.EvalSet.from_s_id(d["Xt"], d["yt"], d["t_sid"], item_offsets=d["t_off"])
    runs = [loop_build(ce, d, mode, base) for _ in range(2)]  # 0: batched XGB, 1: the per-user loop
    user_model = [base] * U
    for e in range(EPOCHS):
        res = []
        next_model = [continued_model(user_model[u], refit(e, u)) for u in range(U)]  # the epoch's host refit
        for k, (sess, nb, sg, xg, bufs) in enumerate(runs):
            nb.predict_proba_session(Xd, sess, out=bufs[0])
            sg.predict_proba_session(Xd, sess, out=bufs[1])
            bufs[2].zero_()  # what a row of an excluded song holds in both runs
            if k == 0:
                xg.predict_proba_session(Xd, sess, out=bufs[2])
            else:
                gone = sess.excl.cpu().numpy().view(np.uint32)
                for u in range(U):
                    keep = [g for g in range(int(d["off"][u]), int(d["off"][u + 1])) if not (gone[g >> 5] >> (g & 31)) & 1]
                    rows = dev(np.flatnonzero(np.isin(d["s_id"], keep)))
                    if rows.numel():
                        bufs[2][rows] = ce.ops.xgb_predict_proba(Xd[rows].contiguous(), XgbForest.from_json(user_model[u]))
            idx = sess.step(frames=bufs)
            nb.partial_fit_picks(Xd, sess, idx, labels_d)
            sg.partial_fit_picks(Xd, sess, idx, labels_d)
            f1g, f1s = nb.evaluate(es)[0], sg.evaluate(es)[0]
            if k == 0:
                for u in range(U):
                    xg.set_model(u, next_model[u])
                f1x, cmx = xg.evaluate(es)
                cmx = cmx.cpu().numpy()
            else:
                cmx, f1h = np.zeros((U, C_LOOP, C_LOOP), np.int64), np.zeros(U)
                for u in range(U):
                    rows = np.flatnonzero(d["t_owner"] == u)
                    p = ce.ops.xgb_predict_proba(es.X[dev(rows)].contiguous(), XgbForest.from_json(next_model[u]))
                    cmx[u] = confusion(d["yt"][rows], predict_labels(p.cpu().numpy()), C_LOOP)[0]
                    f1h[u] = f1_weighted(cmx[u])
                f1x = dev(f1h)
            res.append((idx.cpu().numpy(), bufs[2].cpu().numpy().copy(), cmx, f1x.cpu().numpy(),
                        ce.mean_f1([f1g, f1s, f1x]).cpu().numpy()))
        user_model = next_model
        a, b = res
        assert np.array_equal(a[0], b[0]) and np.array_equal(bits(a[1]), bits(b[1])), (mode, e)
        assert np.array_equal(a[2], b[2]), (mode, e)
        assert np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64)), (mode, e)
        assert np.array_equal(a[4].view(np.uint64), b[4].view(np.uint64)), (mode, e)


def test_epoch_in_one_hip_graph(ce):
    """XGB predict, select + mark and XGB evaluate captured as ONE HIP graph:
    every replay equals the eager epoch, also after X changes in place."""
    rng = np.random.default_rng(300)
    d = loop_data(rng, "mc")
    base = mk(150, 5, D=D_LOOP)
    models = user_models(base, [mk(151 + u, 2 + u, D=D_LOOP) for u in range(len(SONGS))])
    es = ce.EvalSet.from_s_id(d["Xt"], d["yt"], d["t_sid"], item_offsets=d["t_off"])
    _, f_off, f_perm = ce.song_groups(d["s_id"])
    X2 = d["X"] + rng.normal(0, 0.5, d["X"].shape)

    def build():
        sess = ce.BatchedSelectionSession(Q, "mc", d["off"], frame_offsets=f_off, frame_perm=f_perm)
        return sess, ce.DeviceXGBClassifier(base, models), torch.zeros((len(d["s_id"]), C_LOOP), dtype=torch.float32,
                                                                       device="cuda")

    def epoch(Xd, sess, xg, buf):
        xg.predict_proba_session(Xd, sess, out=buf)
        idx = sess.step(frames=[buf])
        f1, cm = xg.evaluate(es)
        return idx, f1, cm

    Xe = dev(d["X"])
    eager, want = build(), []
    for e in range(EPOCHS):
        if e == 2:
            Xe.copy_(dev(X2))
        want.append([t.cpu().numpy().copy() for t in epoch(Xe, *eager)] + [eager[2].cpu().numpy().copy()])
    torch.cuda.synchronize()
    Xg = dev(d["X"])
    graphed = build()
    graphed[1].stacked().device(Xg.device, D_LOOP)  # the lane tables are built outside the capture
    ce.ops.reserve_graph_workspace(ce._lib.load().ce_select_batched_workspace_bytes(int(d["off"][-1]), len(SONGS), Q))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        outs = epoch(Xg, *graphed)
    for e in range(EPOCHS):
        if e == 2:
            Xg.copy_(dev(X2))
        g.replay()
        got = [t.cpu().numpy().copy() for t in outs] + [graphed[2].cpu().numpy().copy()]
        assert np.array_equal(got[0], want[e][0]) and np.array_equal(got[2], want[e][2]), e
        assert np.array_equal(got[1].view(np.uint64), want[e][1].view(np.uint64)), e
        assert np.array_equal(bits(got[3]), bits(want[e][3])), e
    torch.cuda.synchronize()
