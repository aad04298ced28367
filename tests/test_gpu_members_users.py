"""The users form of the linear members' predict_proba on the GPU
(ce_gnb_predict_proba_users / ce_sgd_predict_proba_users,
ops.*_predict_proba_users, Device*.predict_proba_session): every frame row is
predicted by the model of the user who owns it, in one launch per member.

The criterion is the one-model entry points on the same row and model, in all
64 bits (ops.gnb_predict_proba with a device prior, ops.sgd_predict_proba);
"who owns row r" is the numpy statement of tests/members_users_ref.py.  Rows the
kernels must not write (rows no song owns, rows of excluded songs, positions
whose row is out of range) are checked against the bit pattern ``out`` was
prefilled with."""
import numpy as np
import pytest
import torch

from gnb_fit_ref import same_bits
from members_users_ref import excl_words, row_owners

pytestmark = pytest.mark.gpu

FILL_BITS = 0x7FF8C0DE00000A5A  # a NaN with a payload of its own
FILL = np.array([FILL_BITS], np.uint64).view(np.float64)[0]


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


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Pool:
    """U users' stacked songs and their frame rows.  ``frames``: per user, the
    frame count of each of their songs.  shuffled: the rows in random order (a
    frame_perm, a song's rows ascending as song_groups gives them); extra: rows
    of X that no song owns (at the end when grouped, anywhere when shuffled)."""

    def __init__(self, rng, frames, shuffled=False, extra=0):
        self.U = len(frames)
        self.off = np.concatenate([[0], np.cumsum([len(f) for f in frames])]).astype(np.int64)
        counts = np.concatenate([np.asarray(f, np.int64) for f in frames] + [np.zeros(0, np.int64)])
        self.T = len(counts)
        self.f_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
        n = int(self.f_off[-1])
        self.F = n + extra
        self.f_perm = None
        if shuffled:
            rows = rng.permutation(self.F)[:n]
            self.f_perm = np.concatenate([np.sort(rows[self.f_off[g]:self.f_off[g + 1]]) for g in range(self.T)]
                                         + [np.zeros(0, np.int64)]).astype(np.int64)
        self.user, self.song = row_owners(self.off, self.f_off, self.f_perm, self.F)

    def geometry(self, f_perm="own"):
        f_perm = self.f_perm if isinstance(f_perm, str) else f_perm
        return dict(item_offsets=dev(self.off), frame_offsets=dev(self.f_off),
                    frame_perm=None if f_perm is None else dev(f_perm))


def gnb_models(rng, U, C, D):
    theta, var = rng.normal(0, 1, (U, C, D)), rng.random((U, C, D)) + 0.1
    return theta, var, rng.dirichlet(np.ones(C) * 3, U)


def sgd_models(rng, U, C, D):
    K = 1 if C == 2 else C
    return rng.normal(0, 0.5, (U, K, D)) / np.sqrt(D / 8), rng.normal(0, 0.5, (U, K))


def one_model_rows(ce, kind, Xd, models, user):
    """[F, C]: row r by the ONE-model entry point with the model of user[r]; FILL where nobody owns r."""
    C = models[0].shape[1] if kind == "gnb" else (2 if models[0].shape[1] == 1 else models[0].shape[1])
    want = np.full((len(user), C), FILL)
    for u in np.unique(user[user >= 0]):
        if kind == "gnb":
            p = ce.ops.gnb_predict_proba(Xd, dev(models[0][u]), dev(models[1][u]), dev(models[2][u]))
        else:
            p = ce.ops.sgd_predict_proba(Xd, dev(models[0][u]), dev(models[1][u]))
        want[user == u] = p.cpu().numpy()[user == u]
    return want


def users_form(ce, kind, Xd, models, geom, excl=None, out=None):
    f = ce.ops.gnb_predict_proba_users if kind == "gnb" else ce.ops.sgd_predict_proba_users
    return f(Xd, *[dev(m) for m in models], **geom, excl=None if excl is None else dev(excl), out=out)


def filled(F, C, ld=None):
    """out [F, C] prefilled with FILL (a view of row stride ld when given)."""
    buf = torch.full((F, ld or C), FILL_BITS, dtype=torch.int64, device="cuda").view(torch.float64)
    return buf[:, :C], buf


def check(ce, kind, rng, pool, C, D, excluded=None, shuffled_perm="own", ld=None, ldo=None, X=None, models=None,
          user=None):
    """The users form over `pool` against the one-model entry points; returns (got, want) on the host."""
    X = rng.normal(0, 1, (pool.F, D)) if X is None else X
    if ld:
        Xbuf = torch.zeros((pool.F, ld), dtype=torch.float64, device="cuda")
        Xbuf[:, :D] = dev(X)
        Xd = Xbuf[:, :D]
    else:
        Xd = dev(X)
    if models is None:
        models = gnb_models(rng, pool.U, C, D) if kind == "gnb" else sgd_models(rng, pool.U, C, D)
    user = pool.user if user is None else user
    written = np.where(np.isin(pool.song, list(excluded or [])), -1, user)
    want = one_model_rows(ce, kind, Xd, models, written)
    out, buf = filled(pool.F, C, ldo)
    got = users_form(ce, kind, Xd, models, pool.geometry(shuffled_perm),
                     excl=None if excluded is None else excl_words(excluded, pool.T), out=out)
    assert got is out
    got, whole = got.cpu().numpy(), buf.cpu().numpy()
    none = written < 0
    assert np.array_equal(bits(got[none]), bits(want[none])), "a row that must not be written was"  # FILL, bit for bit
    assert same_bits(got[~none], want[~none]), np.flatnonzero((bits(got) != bits(want)).any(1))[:8]
    assert np.array_equal(bits(whole[:, C:]), bits(np.full_like(whole[:, C:], FILL))), "wrote past C columns"
    return got, want


def ragged(rng, n_users, max_songs=6, max_frames=12):
    return [rng.integers(0, max_frames + 1, rng.integers(0, max_songs + 1)) for _ in range(n_users)]


# ---- 1. parity --------------------------------------------------------------
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_parity_with_the_one_model_entry_points(ce, kind, shuffled):
    """The reference's shape (D = 260, C = 4): ragged users, more than one block's share."""
    rng = np.random.default_rng(1 + shuffled)
    pool = Pool(rng, ragged(rng, 40, 8, 30), shuffled, extra=5)
    assert pool.F > 2000 and (pool.user >= 0).sum() == pool.F - 5
    check(ce, kind, rng, pool, 4, 260)


def test_gnb_against_the_restatement(ce):
    """One small GaussianNB case against oracle.ce_oracle.ref_gnb_predict_proba, bit for bit."""
    from oracle.ce_oracle import ref_gnb_predict_proba

    rng = np.random.default_rng(3)
    pool = Pool(rng, [[5, 9], [], [1, 0, 20], [8]], shuffled=True)
    X = rng.normal(0, 1, (pool.F, 260))
    models = gnb_models(rng, pool.U, 4, 260)
    got, _ = check(ce, "gnb", rng, pool, 4, 260, X=X, models=models)
    for u in range(pool.U):
        rows = pool.user == u
        if rows.any():
            want = ref_gnb_predict_proba(X[rows], models[0][u], models[1][u], models[2][u])
            assert np.array_equal(bits(got[rows]), bits(want)), u


def test_sgd_against_the_restatement(ce):
    """One small SGD case against ref_sgd_predict_proba at the tolerance
    tests/test_gpu_parity.py states for the one-model kernels (a fixed wave
    order against BLAS's): rtol 1e-10, atol 1e-300."""
    from oracle.ce_oracle import ref_sgd_predict_proba

    rng = np.random.default_rng(4)
    pool = Pool(rng, [[5, 9], [], [1, 0, 20], [8]], shuffled=True)
    X = rng.normal(0, 1, (pool.F, 260))
    models = sgd_models(rng, pool.U, 4, 260)
    got, _ = check(ce, "sgd", rng, pool, 4, 260, X=X, models=models)
    for u in range(pool.U):
        rows = pool.user == u
        if rows.any():
            np.testing.assert_allclose(got[rows], ref_sgd_predict_proba(X[rows], models[0][u], models[1][u]),
                                       rtol=1e-10, atol=1e-300)


# ---- 2. user edges ------------------------------------------------------------
def split(rng, n, parts):
    """n frames over `parts` songs (some may get none)."""
    cuts = np.sort(rng.integers(0, n + 1, parts - 1))
    return np.diff(np.concatenate([[0], cuts, [n]]))


@pytest.mark.parametrize("D", [16, 260])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_user_boundaries_inside_groups_and_blocks(ce, kind, shuffled, D):
    """Per-user frame counts 0, 1, 7, 8, 9, 31, 32, 33 and 257 in one pool (in
    two orders): boundaries fall inside a wave's 8 frames and inside a block's
    share; a user with no song, users whose songs have no frame, songs with no
    frame among others."""
    rng = np.random.default_rng(10 + shuffled)
    for counts in ([0, 1, 7, 8, 9, 31, 32, 33, 257], [257, 33, 0, 32, 31, 9, 8, 7, 1, 0]):
        frames = [split(rng, n, 3) for n in counts]
        frames.insert(4, [])          # a user with no song at all
        frames[1] = np.array([0, counts[1], 0])  # songs with no frame around the one that has them
        pool = Pool(rng, frames, shuffled)
        assert [int((pool.user == u).sum()) for u in range(pool.U)] == counts[:4] + [0] + counts[4:]
        check(ce, kind, rng, pool, 4, D)


@pytest.mark.parametrize("D", [24, 260])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_three_hundred_users_of_three_frames(ce, kind, D):
    rng = np.random.default_rng(12)
    pool = Pool(rng, [[1, 2]] * 150 + [[3]] * 150, shuffled=True)
    check(ce, kind, rng, pool, 4, D)


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_one_user_over_a_selection_session(ce, order):
    """U = 1: a SelectionSession(s_id=) and both members' predict_proba_session
    equal predict_proba(X) on every row; with picked songs their rows keep the
    prefill unless skip_excluded=False."""
    rng = np.random.default_rng(13)
    N, C, D = 30, 4, 260
    s_id = np.repeat(np.arange(N) * 7 + 3, rng.integers(1, 9, N))
    if order == "shuffled":
        s_id = rng.permutation(s_id)
    F = len(s_id)
    Xd = dev(rng.normal(0, 1, (F, D)))
    th, va, pr = gnb_models(rng, 1, C, D)
    nb = ce.DeviceGaussianNB(th[0], va[0], np.ones(C), class_prior=pr[0])
    co, ic = sgd_models(rng, 1, C, D)
    sg = ce.DeviceSGDClassifier(co[0], ic[0], 1.0, random_state=1)
    sess = ce.SelectionSession(5, "mc", N, s_id=s_id)
    for m in (nb, sg):
        want = m.predict_proba(Xd).cpu().numpy()
        assert same_bits(m.predict_proba_session(Xd, sess).cpu().numpy(), want)
    picked = sess.select(frames=[nb.predict_proba(Xd)])
    gone = np.isin(s_id, sess.song_ids[picked])
    assert gone.any() and not gone.all()
    for m in (nb, sg):
        want = m.predict_proba(Xd).cpu().numpy()
        out, _ = filled(F, C)
        got = m.predict_proba_session(Xd, sess, out=out).cpu().numpy()
        assert same_bits(got[~gone], want[~gone]) and (bits(got[gone]) == bits(FILL)).all()
        assert (m.predict_proba_session(Xd, sess).cpu().numpy()[gone] == 0).all()  # a new tensor is zero there
        assert same_bits(m.predict_proba_session(Xd, sess, skip_excluded=False).cpu().numpy(), want)


# ---- 3. feature and class edges ------------------------------------------------
@pytest.mark.parametrize("C", [2, 4, 8])
@pytest.mark.parametrize("D", [8, 9, 63, 64, 65, 260, 511, 512])
def test_gnb_feature_and_class_edges(ce, D, C):
    rng = np.random.default_rng(D * 10 + C)
    pool = Pool(rng, [[3, 30], [17], [9, 0, 41]], shuffled=bool(D & 1))
    check(ce, "gnb", rng, pool, C, D)
    check(ce, "gnb", rng, pool, C, D, ld=D + 3, ldo=C + 3)  # X with ld > D, out with a row stride > C


@pytest.mark.parametrize("C", [2, 3, 4, 8])
@pytest.mark.parametrize("D", [1, 2, 8, 9, 63, 64, 65, 260, 511, 512])
def test_sgd_feature_and_class_edges(ce, D, C):
    rng = np.random.default_rng(D * 10 + C)
    pool = Pool(rng, [[3, 30], [17], [9, 0, 41]], shuffled=bool(D & 1))
    check(ce, "sgd", rng, pool, C, D)  # C = 2: the binary model, K = 1
    check(ce, "sgd", rng, pool, C, D, ld=D + 3, ldo=C + 3)


@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_shape_refusals_on_the_device(ce, kind):
    rng = np.random.default_rng(5)
    pool = Pool(rng, [[4], [6]])
    D = 16
    Xd = dev(rng.normal(0, 1, (pool.F, D)))
    models = gnb_models(rng, 3, 4, D) if kind == "gnb" else sgd_models(rng, 3, 4, D)
    with pytest.raises(ValueError, match=r"2 user\(s\).*3 model"):
        users_form(ce, kind, Xd, models, pool.geometry())
    models = [m[:2] for m in models]
    with pytest.raises(ValueError, match="out must be"):
        users_form(ce, kind, Xd, models, pool.geometry(), out=torch.zeros((pool.F, 5), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="excl must be"):
        users_form(ce, kind, Xd, models, pool.geometry(), excl=np.zeros(1, np.int64))
    if kind == "gnb":
        with pytest.raises(ce.CEError, match="D >= 8"):
            users_form(ce, kind, Xd[:, :7], [m[..., :7] if m.ndim == 3 else m for m in models], pool.geometry())


# ---- 4. row order ---------------------------------------------------------------
@pytest.mark.parametrize("D", [33, 260])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_rows_no_song_owns_and_rows_out_of_range(ce, kind, D):
    """Extra rows of X keep the prefill (grouped: at the end; shuffled:
    anywhere).  A frame_perm entry >= F, or negative, is skipped -- neither read
    nor written -- and its neighbours are correct."""
    rng = np.random.default_rng(20)
    frames = [[5, 12, 3], [40], [0, 9]]
    for shuffled in (False, True):
        pool = Pool(rng, frames, shuffled, extra=11)
        assert (pool.user < 0).sum() == 11
        check(ce, kind, rng, pool, 4, D)
    pool = Pool(rng, frames, shuffled=True)
    bad = pool.f_perm.copy()
    lost = [0, 6, 7, 30, len(bad) - 1]
    bad[lost] = [pool.F, pool.F + 1, 1 << 40, -1, -(1 << 35)]
    user, _ = row_owners(pool.off, pool.f_off, bad, pool.F)
    assert (user < 0).sum() == len(lost)
    check(ce, kind, rng, pool, 4, D, shuffled_perm=bad, user=user)


# ---- 5. exclusion ---------------------------------------------------------------
@pytest.mark.parametrize("D", [40, 260])
@pytest.mark.parametrize("shuffled", [False, True])
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_excluded_songs_are_never_written(ce, kind, shuffled, D):
    """Some songs excluded, a whole user excluded, a run of more than 8 excluded
    frames in the middle of a user (whole 8-frame groups skipped), excluded songs
    that straddle a group; every other row as in the parity test."""
    rng = np.random.default_rng(30 + shuffled)
    frames = [[3, 5, 20, 4, 1], [6, 6], [2, 40, 9, 0, 7], [13], [1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1]]
    pool = Pool(rng, frames, shuffled, extra=3)
    off = pool.off
    excluded = [off[0] + 2,                # 20 frames in the middle of user 0
                off[1], off[1] + 1,        # all of user 1
                off[2] + 1, off[2] + 3,    # 40 frames, and a song with no frame
                off[4] + 2, off[4] + 3, off[4] + 5, off[4] + 11]
    got, want = check(ce, kind, rng, pool, 4, D, excluded=[int(g) for g in excluded])
    assert (bits(got[pool.user == 1]) == bits(FILL)).all() and (pool.user == 1).sum() == 12
    # no bit set: as without a bitmap; every bit set: nothing written
    check(ce, kind, rng, pool, 4, D, excluded=[])
    models = gnb_models(rng, pool.U, 4, D) if kind == "gnb" else sgd_models(rng, pool.U, 4, D)
    out, _ = filled(pool.F, 4)
    users_form(ce, kind, dev(rng.normal(0, 1, (pool.F, D))), models, pool.geometry(),
               excl=excl_words(range(pool.T), pool.T), out=out)
    assert (bits(out.cpu().numpy()) == bits(FILL)).all()
    # a new tensor is zero where nothing is written (the rule of frames_consensus)
    fresh = users_form(ce, kind, dev(rng.normal(0, 1, (pool.F, D))), models, pool.geometry(),
                       excl=excl_words(range(pool.T), pool.T))
    assert (fresh.cpu().numpy() == 0).all()


@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_session_bitmap_and_skip_excluded(ce, kind):
    """predict_proba_session over a BatchedSelectionSession after an epoch: the
    picked songs' rows keep the prefill; skip_excluded=False writes every owned row."""
    rng = np.random.default_rng(33)
    C, D = 4, 20
    pool = Pool(rng, ragged(rng, 6, 9, 10), shuffled=True)
    X = rng.normal(0, 1, (pool.F, D))
    Xd = dev(X)
    sess = ce.BatchedSelectionSession(3, "mc", pool.off, frame_offsets=pool.f_off, frame_perm=pool.f_perm)
    if kind == "gnb":
        models = gnb_models(rng, pool.U, C, D)
        m = ce.DeviceGaussianNB(models[0], models[1], np.ones((pool.U, C)), class_prior=models[2])
    else:
        models = sgd_models(rng, pool.U, C, D)
        m = ce.DeviceSGDClassifier(models[0], models[1], 1.0, random_state=3)
    want = one_model_rows(ce, kind, Xd, models, pool.user)
    first = m.predict_proba_session(Xd, sess)
    assert same_bits(first.cpu().numpy(), want)  # every row is owned; nothing excluded yet
    picks = sess.select(frames=[first])
    gone_songs = np.concatenate([pool.off[u] + np.asarray(p) for u, p in enumerate(picks)])
    gone = np.isin(pool.song, gone_songs)
    assert gone.any() and not gone.all()
    out, _ = filled(pool.F, C)
    got = m.predict_proba_session(Xd, sess, out=out).cpu().numpy()
    assert same_bits(got[~gone], want[~gone]) and (bits(got[gone]) == bits(FILL)).all()
    assert same_bits(m.predict_proba_session(Xd, sess, out=out, skip_excluded=False).cpu().numpy(), want)


# ---- 6. special values ----------------------------------------------------------
@pytest.mark.parametrize("kind", ["gnb", "sgd"])
def test_special_values(ce, kind):
    """A NaN cell, +-inf features, a zero prior (log-prior -inf) and rows 40
    sigma from every class (the logsumexp shift): the one-model path's bits."""
    rng = np.random.default_rng(40)
    C, D = 4, 260
    pool = Pool(rng, [[9, 14], [30], [5, 5, 5]], shuffled=True)
    X = rng.normal(0, 1, (pool.F, D))
    X[3, 17] = np.nan
    X[11, 0], X[12, 259], X[13, 100] = np.inf, -np.inf, np.inf
    X[13, 101] = -np.inf
    X[20:26] *= 40.0
    X[40] = 1e200
    if kind == "gnb":
        models = gnb_models(rng, pool.U, C, D)
        models[2][1] = [0.0, 0.5, 0.25, 0.25]
        models[2][2] = [0.0, 0.0, 0.0, 1.0]
    else:
        models = sgd_models(rng, pool.U, C, D)
        models[0][1] *= 50.0  # saturated expit: 0 and 1 among the classes
    got, want = check(ce, kind, rng, pool, C, D, X=X, models=models)
    assert np.isnan(got[3]).all() and np.isfinite(got[20:26]).all()
    if kind == "gnb":
        r = got[pool.user == 1]
        r = r[np.isfinite(r).all(1)]
        assert len(r) > 20 and (r[:, 0] == 0).all()  # the zero prior: log-prior -inf, p = 0


# ---- 7. end to end ----------------------------------------------------------------
@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_end_to_end_gnb(ce, mode, order):
    """The three-epoch batched loop of test_gpu_gnb_partial_fit.test_end_to_end_batched
    with one predict_proba_session per epoch in place of the per-user loop: the
    picks are the host loop's, and the final states those of the same loop run
    with the per-user predict, bit for bit (host picks and device picks)."""
    import test_gpu_gnb_partial_fit as G

    rng = np.random.default_rng(50 + len(mode) * 2 + (order == "grouped"))
    users = [96, 40, 70]
    U = len(users)
    off = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    s_id, X, song_labels = G.e2e_pool(rng, int(off[-1]), order)
    states = [G.e2e_state(rng) for _ in range(U)]
    user_rows = [np.flatnonzero((s_id >= off[u]) & (s_id < off[u + 1])) for u in range(U)]
    kw, tables = {}, [{} for _ in range(U)]
    if mode == "mix":
        tabs = [G.e2e_table(rng, n) for n in users]
        off_h = np.concatenate([[0], np.cumsum([len(t[1]) for t in tabs])]).astype(np.int64)
        kw = dict(hc=np.concatenate([t[0] for t in tabs]), hc_offsets=off_h, hc_to_mc=np.concatenate([t[1] for t in tabs]))
        tables = [dict(hc=t[0], h2m=t[1]) for t in tabs]
    exp = [G.host_epochs(mode, X[user_rows[u]], s_id[user_rows[u]] - off[u], song_labels[off[u]:off[u + 1]],
                         states[u], **tables[u])[0] for u in range(U)]
    _, f_off, f_perm = ce.song_groups(s_id)
    Xd = dev(X)
    rows_d = [dev(r) for r in user_rows]
    for device_picks in (False, True):
        final = {}
        for batched in (False, True):
            sess = ce.BatchedSelectionSession(G.Q, mode, off, frame_offsets=f_off, frame_perm=f_perm, **kw)
            nb = ce.DeviceGaussianNB(*[np.stack([s[i] for s in states]) for i in range(3)])
            p = torch.empty((len(s_id), G.C_E2E), dtype=torch.float64, device="cuda")
            for e in range(G.EPOCHS):
                if batched:
                    assert nb.predict_proba_session(Xd, sess, out=p) is p
                else:
                    for u in range(U):
                        p[rows_d[u]] = nb.predict_proba(Xd, u)[rows_d[u]]
                if device_picks:
                    idx = sess.step(frames=[p])
                    nb.partial_fit_picks(Xd, sess, idx, song_labels)
                    picks = sess.account(idx)
                else:
                    picks = sess.select(frames=[p])
                    nb.partial_fit_picks(Xd, sess, picks, song_labels)
                for u in range(U):
                    assert np.array_equal(picks[u], exp[u][e]), (mode, order, e, u, batched)
            final[batched] = nb.state()
        for k in G.NAMES:
            assert same_bits(final[True][k], final[False][k]), (mode, order, device_picks, k)


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_end_to_end_sgd(ce, mode, order):
    """The SGD twin (test_gpu_sgd_partial_fit.test_end_to_end_batched): picks and
    states of the loop with predict_proba_session equal those with the per-user
    predict, and every epoch's states the restatement fed those picks."""
    import test_gpu_sgd_partial_fit as S

    rng = np.random.default_rng(50 + len(mode) * 2 + (order == "grouped"))
    users = [80, 30, 55]
    U = len(users)
    off = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    s_id, X, song_labels = S.e2e_pool(rng, int(off[-1]), order)
    user_rows = [np.flatnonzero((s_id >= off[u]) & (s_id < off[u + 1])) for u in range(U)]
    kw, tabs = {}, [(None, None)] * U
    if mode == "mix":
        tabs = [S.e2e_table(rng, n) for n in users]
        off_h = np.concatenate([[0], np.cumsum([len(t[1]) for t in tabs])]).astype(np.int64)
        kw = dict(hc=np.concatenate([t[0] for t in tabs]), hc_offsets=off_h, hc_to_mc=np.concatenate([t[1] for t in tabs]))
    _, f_off, f_perm = ce.song_groups(s_id)
    Xd = dev(X)
    rows_d = [dev(r) for r in user_rows]
    init = [S.model(rng, S.C_E2E, S.D_E2E) for _ in range(U)]
    for device_picks in (False, True):
        seen = {}
        for batched in (False, True):
            states = list(init)
            sess = ce.BatchedSelectionSession(S.Q, mode, off, frame_offsets=f_off, frame_perm=f_perm, **kw)
            m = ce.DeviceSGDClassifier(*[np.stack([s[i] for s in states]) for i in range(3)], random_state=[7, 8, 9])
            p = torch.empty((len(s_id), S.C_E2E), dtype=torch.float64, device="cuda")
            all_picks = []
            for e in range(S.EPOCHS):
                if batched:
                    m.predict_proba_session(Xd, sess, out=p)
                else:
                    for u in range(U):
                        p[rows_d[u]] = m.predict_proba(Xd, u)[rows_d[u]]
                if device_picks:
                    idx = sess.step(frames=[p])
                    m.partial_fit_picks(Xd, sess, idx, song_labels)
                    picks = sess.account(idx)
                else:
                    picks = sess.select(frames=[p])
                    m.partial_fit_picks(Xd, sess, picks, song_labels)
                all_picks.append([np.asarray(x).tolist() for x in picks])
                s = m.state()
                for u in range(U):
                    songs = S.picked_songs(np.asarray(picks[u]), users[u], tabs[u][1])
                    states[u] = S.host_retrain(X[user_rows[u]], s_id[user_rows[u]] - off[u],
                                               song_labels[off[u]:off[u + 1]], songs, states[u], 7 + u)
                    S.assert_state((s["coef"][u], s["intercept"][u], s["t"][u]), states[u], (mode, order, e, u, batched))
            m.check_finite()
            seen[batched] = (all_picks, m.state())
        assert seen[True][0] == seen[False][0], (mode, order, device_picks)
        for k in ("coef", "intercept", "t"):
            assert same_bits(seen[True][1][k], seen[False][1][k]), (mode, order, device_picks, k)


# ---- 8. graph capture ---------------------------------------------------------------
def test_epoch_in_one_hip_graph(ce):
    """One epoch for U = 3 users -- both members' predict_proba_session,
    sess.step(frames=...), both partial_fit_picks on the device picks -- captured
    in ONE HIP graph (a linear chain on the capture stream) and replayed for
    three epochs: the picks and the final states of the eager loop."""
    import test_gpu_sgd_partial_fit as S

    rng = np.random.default_rng(60)
    users, C, D, EPOCHS = [40, 25, 33], 4, 65, 3
    U = len(users)
    off = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    s_id, X, song_labels = S.e2e_pool(rng, int(off[-1]), "shuffled")
    _, f_off, f_perm = ce.song_groups(s_id)
    Xd, labels_d = dev(X), dev(song_labels.astype(np.int64))
    th, va, _ = gnb_models(rng, U, C, D)
    cc = rng.integers(1, 50, (U, C)).astype(np.float64)
    sgd0 = [S.model(rng, C, D) for _ in range(U)]

    def build():
        sess = ce.BatchedSelectionSession(6, "mc", off, frame_offsets=f_off, frame_perm=f_perm)
        nb = ce.DeviceGaussianNB(th * 0.5, va * 4.0, cc)
        sg = ce.DeviceSGDClassifier(*[np.stack([s[i] for s in sgd0]) for i in range(3)], random_state=[7, 8, 9])
        bufs = [torch.zeros((len(s_id), C), dtype=torch.float64, device="cuda") for _ in range(2)]
        return sess, nb, sg, bufs

    def epoch(sess, nb, sg, bufs):
        nb.predict_proba_session(Xd, sess, out=bufs[0])
        sg.predict_proba_session(Xd, sess, out=bufs[1])
        idx = sess.step(frames=bufs)
        nb.partial_fit_picks(Xd, sess, idx, labels_d)
        sg.partial_fit_picks(Xd, sess, idx, labels_d)
        return idx

    eager = build()
    want = [epoch(*eager).cpu().numpy().copy() for _ in range(EPOCHS)]
    assert all((w >= 0).all() for w in want) and len({tuple(w.reshape(-1)) for w in want}) == EPOCHS
    torch.cuda.synchronize()
    graphed = build()
    ce.ops.reserve_graph_workspace(ce._lib.load().ce_select_batched_workspace_bytes(int(off[-1]), U, 6))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        idx = epoch(*graphed)
    got = []
    for _ in range(EPOCHS):
        g.replay()
        got.append(idx.cpu().numpy().copy())
    torch.cuda.synchronize()
    for e in range(EPOCHS):
        assert np.array_equal(got[e], want[e]), e
    for k in ("theta", "var", "class_count", "class_prior", "epsilon"):
        assert same_bits(graphed[1].state()[k], eager[1].state()[k]), k
    for k in ("coef", "intercept", "t", "status"):
        assert same_bits(graphed[2].state()[k].astype(np.float64), eager[2].state()[k].astype(np.float64)), k
