"""GaussianNB.partial_fit on the GPU (ce_gnb_partial_fit, amg_test.py:509):
ops.gnb_partial_fit, DeviceGaussianNB and the predict -> select -> retrain loop
against the row-loop restatement of sklearn (tests/gnb_fit_ref.py, pinned to
sklearn bit for bit by tests/test_gnb_partial_fit.py) and the committed sklearn
fixture.  Every comparison is 0 ulp over all five outputs (theta, var,
class_count, class_prior, epsilon); a NaN matches a NaN."""
import numpy as np
import pytest
import torch

from conftest import golden
from gnb_fit_ref import gnb_partial_fit, same_bits

pytestmark = pytest.mark.gpu

NAMES = ("theta", "var", "class_count", "class_prior", "epsilon")


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


def fitted_state(rng, C, D, unseen=()):
    """A fitted model's (theta, var, class_count); the classes in `unseen` as
    sklearn leaves them before their first sample (zeros, count 0)."""
    theta, var = rng.normal(0, 1, (C, D)), rng.random((C, D)) + 0.1
    cc = rng.integers(1, 50, C).astype(np.float64)
    for c in unseen:
        theta[c], var[c], cc[c] = 0.0, 1e-9, 0.0
    return theta, var, cc


class DeviceState:
    """The three in/out tensors and the two outputs of one or U models, kept on the device."""

    def __init__(self, theta, var, cc):
        self.t = [dev(theta), dev(var), dev(cc)]
        self.prior = torch.full(cc.shape, np.nan, dtype=torch.float64, device="cuda")
        self.eps = torch.full(cc.shape[:-1] or (1,), np.nan, dtype=torch.float64, device="cuda")

    def fit(self, ops, X, rows, labels, row_offsets=None):
        ops.gnb_partial_fit(X, dev(np.asarray(rows, np.int64)), dev(np.asarray(labels, np.int32)), *self.t,
                            row_offsets=row_offsets, class_prior=self.prior, epsilon=self.eps)

    def host(self):
        return [x.cpu().numpy() for x in self.t + [self.prior, self.eps]]


def assert_state(got, want, what):
    for name, g, w in zip(NAMES, got, want):
        g, w = np.asarray(g, np.float64).reshape(-1), np.asarray(w, np.float64).reshape(-1)
        assert same_bits(g, w), (what, name, np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))[:5])


def batch_shapes(rng, C, F):
    """name -> (rows ascending, labels); class C - 1 has class_count == 0 until 'unseen_arrives'."""
    def asc(n):
        return np.sort(rng.choice(F, n, replace=False))

    seen = C - 1
    return [
        ("one_row", asc(1), np.array([0])),                                   # variance 0, epsilon 0
        ("class_absent", asc(9), rng.integers(1, seen, 9) if seen > 1 else np.zeros(9, int)),  # class 0 absent
        ("one_class", asc(7), np.zeros(7, int)),
        ("unseen_arrives", asc(C + 3), np.concatenate([np.arange(C), [C - 1] * 3])),  # class_count == 0 before
        ("row_per_class", asc(C), rng.permutation(C)),
        ("rows400", asc(400), rng.integers(0, C, 400)),
    ]


@pytest.mark.parametrize("C", [2, 4, 8])
@pytest.mark.parametrize("D", [2, 3, 63, 64, 65, 127, 128, 129, 260, 512])
def test_one_model_chained(ce, D, C):
    """Six chained epochs with the state kept on the device, one per batch
    shape, at the lane and lane-pair edges of D and both limits."""
    rng = np.random.default_rng(1000 * D + C)
    F = 500
    X = rng.normal(0, 1, (F, D)) * np.exp(rng.normal(0, 1, D))
    Xd = dev(X)
    th, va, cc = fitted_state(rng, C, D, unseen=(C - 1,))
    st = DeviceState(th, va, cc)
    for name, rows, labels in batch_shapes(rng, C, F):
        st.fit(ce.ops, Xd, rows, labels)
        th, va, cc, prior, eps = gnb_partial_fit(X[rows], labels, th, va, cc)
        if name == "one_row":
            assert eps == 0.0
        assert_state(st.host(), (th, va, cc, prior, eps), (D, C, name))
    assert cc[C - 1] > 0


@pytest.mark.parametrize("D,ld,shift", [(260, 262, 0), (260, 261, 0), (260, 260, 1), (3, 8, 0), (64, 70, 0), (512, 514, 1)])
def test_strides_and_row_order(ce, D, ld, shift):
    """X with ld > D (even: 16-byte loads, odd or an 8-byte-aligned base: 8-byte
    loads), and rows in a non-monotone order: the sums follow the order given."""
    rng = np.random.default_rng(D + ld + shift)
    F, C = 300, 4
    buf = torch.from_numpy(rng.normal(0, 3, F * ld + shift)).cuda()
    Xd = buf[shift:].view(F, ld)[:, :D]
    assert Xd.stride(0) == ld and Xd.data_ptr() % 16 == 8 * shift
    X = Xd.cpu().numpy()
    th, va, cc = fitted_state(rng, C, D)
    st = DeviceState(th, va, cc)
    for e in range(3):
        rows = rng.choice(F, 57, replace=e == 2)  # not ascending; epoch 2 repeats rows
        labels = rng.integers(0, C, len(rows))
        st.fit(ce.ops, Xd, rows, labels)
        th, va, cc, prior, eps = gnb_partial_fit(X[rows], labels, th, va, cc)
        assert_state(st.host(), (th, va, cc, prior, eps), (D, ld, shift, e))
    o = np.argsort(rows, kind="stable")  # the same batch ascending is another result: the order is part of it
    assert not same_bits(gnb_partial_fit(X[rows[o]], labels[o], th, va, cc)[0], gnb_partial_fit(X[rows], labels, th, va, cc)[0])


@pytest.mark.parametrize("D,big", [(9, True), (260, False), (260, True)])
def test_values(ce, D, big):
    """A -0.0 column, a constant column, columns scaled by 1e-150 and (big) 1e150
    -- whose epsilon of ~1e291 swallows every other column's variance, in
    sklearn too; then one NaN cell: epsilon is NaN and var all NaN, as the
    restatement gives."""
    rng = np.random.default_rng(D + big)
    F, C = 64, 4
    X = rng.normal(0, 1, (F, D))
    X[:, 0], X[:, 1] = -0.0, 3.7
    X[:, 2] *= 1e-150
    th, va, cc = fitted_state(rng, C, D, unseen=(2,))
    th[:, 0] = -0.0
    th[:, 2] *= 1e-150
    if big:
        X[:, 3] *= 1e150
        th[:, 3] *= 1e150
        va[:, 3] *= 1e300
    st = DeviceState(th, va, cc)
    for e in range(3):
        if e == 2:
            X[11, D - 1] = np.nan
        rows = np.sort(rng.choice(F, 30, replace=False)) if e < 2 else np.arange(30)
        labels = rng.integers(0, C, 30)
        st.fit(ce.ops, dev(X), rows, labels)
        th, va, cc, prior, eps = gnb_partial_fit(X[rows], labels, th, va, cc)
        assert_state(st.host(), (th, va, cc, prior, eps), (D, big, e))
        if e == 0:
            assert np.signbit(X[rows][:, 0]).all() and not np.signbit(th[labels[0], 0])  # the sums start from +0.0
    assert np.isnan(eps) and np.isnan(va).all() and np.isnan(st.host()[1]).all() and np.isnan(st.host()[4]).all()


@pytest.mark.parametrize("U", [2, 7, 300])
def test_many_models(ce, U):
    """U models in one launch, ragged batches, one user with an empty batch
    (state untouched bit for bit), D = 260: every model equals its own
    one-model call, and (the first models) the restatement."""
    rng = np.random.default_rng(U)
    F, C, D = 2000, 4, 260
    X = rng.normal(0, 1, (F, D))
    Xd = dev(X)
    states = [fitted_state(rng, C, D, unseen=(3,) if u % 3 == 0 else ()) for u in range(U)]
    n = rng.integers(1, 60, U)
    n[U // 2] = 0
    ro = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.choice(F, k, replace=False)) for k in n]).astype(np.int64)
    labels = rng.integers(0, C, len(rows)).astype(np.int32)
    st = DeviceState(*[np.stack([s[i] for s in states]) for i in range(3)])
    st.fit(ce.ops, Xd, rows, labels, row_offsets=dev(ro))
    got = st.host()
    for u in range(U):
        r, l = rows[ro[u]:ro[u + 1]], labels[ro[u]:ro[u + 1]]
        mine = [g[u] for g in got]
        if n[u] == 0:
            assert_state(mine[:3], states[u], (U, u, "untouched"))
            assert np.isnan(mine[3]).all() and np.isnan(mine[4])  # the outputs too: still the caller's fill
            continue
        one = DeviceState(*states[u])
        one.fit(ce.ops, Xd, r, l)
        assert_state(mine, one.host(), (U, u))
        if u < 8:
            assert_state(mine, gnb_partial_fit(X[r], l, *states[u]), (U, u, "restatement"))


@pytest.mark.parametrize("D", [12, 260])
def test_fixture_cases(ce, D):
    """sklearn's own outputs (tests/golden/gnb_partial_fit.npz) through ops.gnb_partial_fit."""
    fx = {k[len(f"d{D}_"):]: v for k, v in golden("gnb_partial_fit").items() if k.startswith(f"d{D}_")}
    Xd = dev(fx["X"])
    st = DeviceState(fx["theta_init"], fx["var_init"], fx["cc_init"])
    for e in range(3):
        st.fit(ce.ops, Xd, fx[f"rows{e}"], fx[f"labels{e}"])
        assert_state(st.host(), [fx[f"{k}{e}"] for k in ("theta", "var", "cc", "prior", "eps")], (D, e))


def test_fresh_outputs_and_shapes(ce):
    """Without out tensors: new (class_prior, epsilon); [C, D] state means one model."""
    rng = np.random.default_rng(8)
    X = rng.normal(0, 1, (50, 10))
    th, va, cc = fitted_state(rng, 3, 10)
    t = [dev(th), dev(va), dev(cc)]
    rows, labels = np.arange(5, 25), rng.integers(0, 3, 20)
    prior, eps = ce.ops.gnb_partial_fit(dev(X), dev(rows), dev(labels), *t)
    assert prior.shape == (3,) and eps.shape == (1,)
    assert_state([x.cpu().numpy() for x in t + [prior, eps]], gnb_partial_fit(X[rows], labels, th, va, cc), "fresh")
    with pytest.raises(ValueError, match="in place"):
        ce.ops.gnb_partial_fit(dev(X), dev(rows), dev(labels), t[0].float(), t[1], t[2])
    with pytest.raises(ce.CEError, match="D >= 2"):
        ce.ops.gnb_partial_fit(dev(X[:, :1]), dev(rows), dev(labels), dev(th[:, :1]), dev(va[:, :1]), t[2])


def test_partial_fit_in_a_hip_graph(ce):
    """One gnb_partial_fit captured in a HIP graph and replayed 3 times equals three eager updates."""
    rng = np.random.default_rng(77)
    U, C, D, F = 3, 4, 260, 400
    X = rng.normal(0, 1, (F, D))
    Xd = dev(X)
    states = [fitted_state(rng, C, D) for _ in range(U)]
    n = np.array([30, 0, 45])
    ro = dev(np.concatenate([[0], np.cumsum(n)]).astype(np.int64))
    rows = dev(np.concatenate([np.sort(rng.choice(F, k, replace=False)) for k in n]).astype(np.int64))
    labels = dev(rng.integers(0, C, int(n.sum())).astype(np.int32))
    stacked = [np.stack([s[i] for s in states]) for i in range(3)]
    eager, graphed = DeviceState(*stacked), DeviceState(*stacked)
    for _ in range(3):
        ce.ops.gnb_partial_fit(Xd, rows, labels, *eager.t, row_offsets=ro, class_prior=eager.prior, epsilon=eager.eps)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        ce.ops.gnb_partial_fit(Xd, rows, labels, *graphed.t, row_offsets=ro, class_prior=graphed.prior,
                               epsilon=graphed.eps)
    assert_state(graphed.host()[:3], stacked, "capture runs nothing")
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    assert_state(graphed.host(), eager.host(), "graph")
    # the one-model form builds its row_offsets on the device: capturable too
    r1, l1 = rows[:30].contiguous(), labels[:30].contiguous()
    one_e, one_g = DeviceState(*states[0]), DeviceState(*states[0])
    for _ in range(2):
        ce.ops.gnb_partial_fit(Xd, r1, l1, *one_e.t, class_prior=one_e.prior, epsilon=one_e.eps)
    torch.cuda.synchronize()
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        ce.ops.gnb_partial_fit(Xd, r1, l1, *one_g.t, class_prior=one_g.prior, epsilon=one_g.eps)
    for _ in range(2):
        g1.replay()
    torch.cuda.synchronize()
    assert_state(one_g.host(), one_e.host(), "graph, one model")


def test_no_rows_at_all(ce):
    """Every batch empty (an epoch that picked nothing): one model with no row
    and three models all empty keep state AND outputs bit for bit."""
    rng = np.random.default_rng(9)
    C, D = 4, 260
    Xd = dev(rng.normal(0, 1, (50, D)))
    none64, none32 = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    for U in (1, 3):
        states = [fitted_state(rng, C, D) for _ in range(U)]
        stacked = [np.stack([s[i] for s in states]) for i in range(3)] if U > 1 else list(states[0])
        st = DeviceState(*stacked)
        st.prior.copy_(dev(rng.random(st.prior.shape)))  # earlier outputs: they must survive
        st.eps.copy_(dev(rng.random(st.eps.shape)))
        before = st.host()
        ro = torch.zeros(U + 1, dtype=torch.int64, device="cuda")
        for offsets in ([ro] if U > 1 else [ro, None]):
            ce.ops.gnb_partial_fit(Xd, none64, none32, *st.t, row_offsets=offsets, class_prior=st.prior, epsilon=st.eps)
            assert_state(st.host(), before, (U, offsets is None))
    prior, eps = ce.ops.gnb_partial_fit(Xd, none64, none32, *st.t, row_offsets=ro)  # fresh outputs: the NaN fill
    assert prior.shape == (3, C) and eps.shape == (3,) and np.isnan(prior.cpu().numpy()).all() and np.isnan(eps.cpu().numpy()).all()


def test_partial_fit_picks_without_a_song(ce):
    """partial_fit_picks after a real update, with picks that name no committee
    song -- all -1, no pick at all, mix picks whose twins are all -1, one user
    and batched: the models and both outputs (the earlier epsilon) stay."""
    rng = np.random.default_rng(21)
    N, C, D = 12, 4, 16
    s_id = np.repeat(np.arange(N), rng.integers(1, 5, N))
    X = rng.normal(0, 1, (len(s_id), D))
    Xd, song_labels = dev(X), rng.integers(0, C, N)
    h2m = np.array([3, -1, -1, 7], np.int64)
    hc = np.full((4, C), 0.25)
    th, va, cc = fitted_state(rng, C, D)
    for mode, empties in (("mc", [np.array([-1, -1]), np.zeros(0, np.int64)]),
                          ("mix", [np.array([N + 1, N + 2]), np.array([-1, N + 1])])):
        kw = dict(hc=hc, hc_to_mc=h2m) if mode == "mix" else {}
        sess = ce.SelectionSession(4, mode, N, s_id=s_id, **kw)
        nb = ce.DeviceGaussianNB(th, va, cc)
        nb.partial_fit_picks(Xd, sess, np.array([2, 5]), song_labels)
        before = nb.state()
        batch = np.isin(s_id, [2, 5])
        assert_state([before[k][0] for k in NAMES], gnb_partial_fit(X[batch], song_labels[s_id[batch]], th, va, cc), mode)
        for picks in empties:
            nb.partial_fit_picks(Xd, sess, picks, song_labels)
            assert_state([nb.state()[k] for k in NAMES], [before[k] for k in NAMES], (mode, picks.tolist()))
        # batched, two users over the same songs twice; picks as host lists and as the device tensor of step
        off = np.array([0, N, 2 * N], np.int64)
        _, f_off, f_perm = ce.song_groups(np.concatenate([s_id, s_id + N]))
        bkw = dict(hc=np.concatenate([hc, hc]), hc_offsets=np.array([0, 4, 8]), hc_to_mc=np.concatenate([h2m, h2m])) if kw else {}
        bs = ce.BatchedSelectionSession(4, mode, off, frame_offsets=f_off, frame_perm=f_perm, **bkw)
        nb2 = ce.DeviceGaussianNB(np.stack([th, th]), np.stack([va, va]), np.stack([cc, cc]))
        X2 = dev(np.concatenate([X, X]))
        nb2.partial_fit_picks(X2, bs, [np.array([2, 5]), np.zeros(0, np.int64)], np.concatenate([song_labels, song_labels]))
        mid = nb2.state()
        assert_state([mid[k][0] for k in NAMES], [before[k][0] for k in NAMES], (mode, "batched user 0"))
        assert same_bits(mid["theta"][1], th) and np.isnan(mid["epsilon"][1])  # user 1 picked nothing yet
        for picks in ([empties[0], empties[1]], torch.full((2, 4), -1, dtype=torch.int64, device="cuda")):
            nb2.partial_fit_picks(X2, bs, picks, np.concatenate([song_labels, song_labels]))
            assert_state([nb2.state()[k] for k in NAMES], [mid[k] for k in NAMES], (mode, "batched empty"))


# ---------------------------------------------------------------------------
# end to end: predict -> select -> retrain, 3 epochs, against the host loop
# ---------------------------------------------------------------------------
Q, EPOCHS, D_E2E, C_E2E = 10, 3, 260, 4


def host_epochs(mode, X, s_id, song_labels, state, hc=None, h2m=None):
    """The reference's loop for one user on the host: every epoch
    ref_gnb_predict_proba over the full X_train, the groupby mean, the
    selection over the songs (and table rows) still in the pool, then the
    restatement's update on X_train[X_train.index.isin(q_songs)] (rows in
    X_train's order).  Returns the picks per epoch and the final state, the
    last update's epsilon included."""
    from oracle import ce_oracle as O

    ids = np.unique(s_id)
    N = len(ids)
    th, va, cc = state
    prior, eps = cc / cc.sum(), np.float64(np.nan)  # the member's epsilon before its first update
    alive = np.ones(N, bool)
    alive_h = np.ones(len(hc), bool) if mode == "mix" else None
    if mode == "mix":
        m2h = np.full(N, -1)
        m2h[h2m[h2m >= 0]] = np.flatnonzero(h2m >= 0)
    out = []
    for _ in range(EPOCHS):
        p = O.ref_gnb_predict_proba(X, th, va, prior)
        P = O.ref_group_mean(p, s_id)[0][None]
        pos = np.flatnonzero(alive)
        if mode == "mc":
            _, i = O.oracle_select_mc(np.ascontiguousarray(P[:, pos]), Q, "MNC")
            picks = pos[i].astype(np.int64)
            songs = picks
        else:
            hpos = np.flatnonzero(alive_h)
            ent = np.concatenate([O.oracle_committee_entropy(np.ascontiguousarray(P[:, pos]), "MNC"),
                                  O.oracle_table_entropy(hc[hpos])])
            _, i = O.oracle_topq(ent, Q)
            picks = np.concatenate([pos, N + hpos])[i].astype(np.int64)
            songs = np.array([s for s in (p_ if p_ < N else h2m[p_ - N] for p_ in picks) if s >= 0], np.int64)
            for p_ in picks:
                if p_ >= N:
                    alive_h[p_ - N] = False
                elif m2h[p_] >= 0:
                    alive_h[m2h[p_]] = False
        alive[songs] = False
        out.append(picks)
        batch = np.isin(s_id, ids[songs])  # X_train.index.isin(q_songs): X_train's row order, a song once
        if batch.any():
            th, va, cc, prior, eps = gnb_partial_fit(X[batch], song_labels[np.searchsorted(ids, s_id[batch])], th, va, cc)
    return out, (th, va, cc, prior, eps)


def e2e_pool(rng, n_songs, order):
    s_id = np.repeat(np.arange(n_songs), rng.integers(1, 10, n_songs))
    if order == "shuffled":
        s_id = rng.permutation(s_id)
    centers = rng.normal(0, 1, (C_E2E, D_E2E))
    song_labels = rng.integers(0, C_E2E, n_songs)
    X = centers[song_labels[s_id]] + rng.normal(0, 2.0, (len(s_id), D_E2E))
    return s_id, X, song_labels


def e2e_table(rng, n_songs):
    n_rows = int(0.8 * n_songs) + 4
    h2m = np.concatenate([rng.permutation(n_songs)[:n_rows - 4], np.full(4, -1)])
    h2m = h2m[rng.permutation(n_rows)].astype(np.int64)
    hc = np.round(rng.dirichlet(np.ones(4), n_rows), 1)
    return hc, h2m


def e2e_state(rng):
    th, va, cc = fitted_state(rng, C_E2E, D_E2E)
    return th * 0.5, va * 4.0, cc


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_end_to_end_one_user(ce, mode, order):
    rng = np.random.default_rng(len(mode) * 2 + (order == "grouped"))
    N = 96
    s_id, X, song_labels = e2e_pool(rng, N, order)
    state = e2e_state(rng)
    kw, hk = {}, {}
    if mode == "mix":
        hc, h2m = e2e_table(rng, N)
        kw, hk = dict(hc=hc, hc_to_mc=h2m), dict(hc=hc, h2m=h2m)
    exp, final = host_epochs(mode, X, s_id, song_labels, state, **hk)
    sess = ce.SelectionSession(Q, mode, N, s_id=s_id, **kw)
    nb = ce.DeviceGaussianNB(*state)
    Xd = dev(X)
    for e in range(EPOCHS):
        picks = sess.select(frames=[nb.predict_proba(Xd)])
        assert np.array_equal(picks, exp[e]), (mode, order, e, picks, exp[e])
        nb.partial_fit_picks(Xd, sess, picks, song_labels)
    s = nb.state()
    assert_state([s[k][0] for k in NAMES], final, (mode, order))


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_end_to_end_batched(ce, mode, order):
    """U = 3 users, one model each: one partial_fit launch per epoch for all of
    them; picks from select (host lists) and from step (the device tensor)."""
    rng = np.random.default_rng(50 + len(mode) * 2 + (order == "grouped"))
    users = [96, 40, 70]
    U = len(users)
    off = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    T = int(off[-1])
    s_id, X, song_labels = e2e_pool(rng, T, order)  # the stacked songs' ids: user u owns off[u]:off[u+1]
    states = [e2e_state(rng) for _ in range(U)]
    user_rows = [np.flatnonzero((s_id >= off[u]) & (s_id < off[u + 1])) for u in range(U)]
    kw, tables = {}, [{} for _ in range(U)]
    if mode == "mix":
        tabs = [e2e_table(rng, n) for n in users]
        off_h = np.concatenate([[0], np.cumsum([len(t[1]) for t in tabs])]).astype(np.int64)
        kw = dict(hc=np.concatenate([t[0] for t in tabs]), hc_offsets=off_h, hc_to_mc=np.concatenate([t[1] for t in tabs]))
        tables = [dict(hc=t[0], h2m=t[1]) for t in tabs]
    exp, finals = zip(*[host_epochs(mode, X[user_rows[u]], s_id[user_rows[u]] - off[u], song_labels[off[u]:off[u + 1]],
                                    states[u], **tables[u]) for u in range(U)])
    _, f_off, f_perm = ce.song_groups(s_id)
    Xd = dev(X)
    rows_d = [dev(r) for r in user_rows]
    for device_picks in (False, True):
        sess = ce.BatchedSelectionSession(Q, mode, off, frame_offsets=f_off, frame_perm=f_perm, **kw)
        nb = ce.DeviceGaussianNB(*[np.stack([s[i] for s in states]) for i in range(3)])
        p = torch.empty((len(s_id), C_E2E), dtype=torch.float64, device="cuda")
        for e in range(EPOCHS):
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
                assert np.array_equal(picks[u], exp[u][e]), (mode, order, e, u)
        s = nb.state()
        for u in range(U):
            assert_state([s[k][u] for k in NAMES], finals[u], (mode, order, u, device_picks))
