"""SGDClassifier.partial_fit on the GPU (ce_sgd_partial_fit, amg_test.py:509 for
the 'classifier_sgd' member): ops.sgd_partial_fit, DeviceSGDClassifier and the
predict -> select -> retrain loop against the row-loop restatement of sklearn
(tests/sgd_fit_ref.py, pinned to sklearn 1.7.2 bit for bit by
tests/test_sgd_partial_fit.py) and the committed sklearn fixture.  Every
comparison is 0 differing bits on coef, intercept and t; a NaN matches a NaN."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import golden
from sgd_fit_ref import chain_seeds, same_bits, sgd_partial_fit

pytestmark = pytest.mark.gpu

PERM_LDS = 8192  # K * n indices up to which a model's permutations stay in shared memory (include/ce.h)


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


def model(rng, C, D, fresh=False):
    """(coef [K, D], intercept [K], t): a fitted model's state, or a fresh one (zeros, t = 1)."""
    K = 1 if C == 2 else C
    if fresh:
        return np.zeros((K, D)), np.zeros(K), 1.0
    return rng.normal(0, 0.5, (K, D)), rng.normal(0, 0.5, K), float(rng.integers(2, 5000))


class DeviceState:
    """coef, intercept, t and status of one or U models, kept on the device."""

    def __init__(self, coef, b, t):
        self.coef, self.b = dev(np.asarray(coef, np.float64)), dev(np.asarray(b, np.float64))
        self.t = dev(np.asarray(t, np.float64).reshape(-1))
        self.status = torch.zeros(self.t.numel(), dtype=torch.int32, device="cuda")

    def fit(self, ops, X, rows, labels, seeds, row_offsets=None, alpha=1e-4, grad="half_binomial"):
        return ops.sgd_partial_fit(X, dev(np.asarray(rows, np.int64)), dev(np.asarray(labels, np.int32)), self.coef,
                                   self.b, self.t, row_offsets, alpha, seeds=seeds, grad=grad, status=self.status)

    def host(self):
        return self.coef.cpu().numpy(), self.b.cpu().numpy(), self.t.cpu().numpy()


def assert_state(got, want, what):
    for name, g, w in zip(("coef", "intercept", "t"), got, want):
        g, w = np.asarray(g, np.float64).reshape(-1), np.asarray(w, np.float64).reshape(-1)
        assert same_bits(g, w), (what, name, np.flatnonzero(g.view(np.uint64) != w.view(np.uint64))[:5])


def fixture_cases():
    fx = golden("sgd_partial_fit")
    return {name: {k[len(name) + 1:]: v for k, v in fx.items() if k.startswith(name + "_")} for name in fx["cases"]}


CASES = fixture_cases()


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_ops(ce, name):
    """sklearn's own outputs (tests/golden/sgd_partial_fit.npz) through ops.sgd_partial_fit."""
    c = CASES[name]
    C, alpha = int(c["C"]), float(c["alpha"])
    seeds = ce.ops.sgd_chain_seeds(int(c["random_state"]), C)
    Xd = dev(c["X"])
    st = DeviceState(c["coef_init"], c["intercept_init"], c["t_init"])
    for e in range(4):
        st.fit(ce.ops, Xd, c[f"rows{e}"], c[f"labels{e}"], seeds, alpha=alpha)
        assert_state(st.host(), (c[f"coef{e}"], c[f"intercept{e}"], c[f"t{e}"]), (name, e))
    assert st.status.tolist() == [0]


@pytest.mark.parametrize("name", sorted(CASES))
def test_fixture_cases_member(ce, name):
    """The same through DeviceSGDClassifier (its own seeds from random_state)."""
    c = CASES[name]
    Xd = dev(c["X"])
    m = ce.DeviceSGDClassifier(c["coef_init"], c["intercept_init"], float(c["t_init"]), alpha=float(c["alpha"]),
                               random_state=int(c["random_state"]))
    assert m.C == int(c["C"])
    for e in range(4):
        m.partial_fit(Xd, dev(c[f"rows{e}"]), dev(c[f"labels{e}"]))
        s = m.state()
        assert_state((s["coef"][0], s["intercept"][0], s["t"]), (c[f"coef{e}"], c[f"intercept{e}"], c[f"t{e}"]), (name, e))
    m.check_finite()
    p = m.predict_proba(Xd)
    assert p.shape == (c["X"].shape[0], m.C)  # the updated model's predict: ops.sgd_predict_proba on the fixture's state
    want = ce.ops.sgd_predict_proba(Xd, dev(c["coef3"]), dev(c["intercept3"]))
    assert same_bits(p.cpu().numpy(), want.cpu().numpy())


@pytest.mark.parametrize("C", [2, 3, 4, 8])
@pytest.mark.parametrize("D", [1, 2, 63, 64, 65, 127, 128, 129, 260, 511, 512])
def test_feature_edges(ce, D, C):
    """Two chained batches at the edges of the lanes' runs of 8 features and of the 64 lanes, every class count."""
    rng = np.random.default_rng(1000 * D + C)
    F = 120
    X = rng.normal(0, 1, (F, D)) * np.exp(rng.normal(0, 0.5, D))
    Xd = dev(X)
    coef, b, t = model(rng, C, D)
    seeds = chain_seeds(int(rng.integers(0, 1000)), C)
    st = DeviceState(coef, b, t)
    for n in (5, 37):
        rows, labels = np.sort(rng.choice(F, n, replace=False)), rng.integers(0, C, n)
        st.fit(ce.ops, Xd, rows, labels, seeds)
        coef, b, t, finite = sgd_partial_fit(X[rows], labels, coef, b, t, seeds=seeds)
        assert finite
        assert_state(st.host(), (coef, b, t), (D, C, n))
    assert st.status.tolist() == [0]


@pytest.mark.parametrize("D,ld,shift", [(260, 262, 0), (260, 261, 0), (260, 260, 1), (3, 8, 0), (64, 70, 1), (512, 514, 1)])
def test_strides_and_row_order(ce, D, ld, shift):
    """X with ld > D and a view that starts one element in (no 16-byte
    alignment); then the same rows in another order: another result, equal to
    the restatement's -- the shuffle starts from the order given."""
    rng = np.random.default_rng(D + ld + shift)
    F, C = 200, 4
    buf = torch.from_numpy(rng.normal(0, 1, F * ld + shift)).cuda()
    Xd = buf[shift:].view(F, ld)[:, :D]
    assert Xd.stride(0) == ld and Xd.data_ptr() % 16 == 8 * shift
    X = Xd.cpu().numpy()
    init = model(rng, C, D)
    seeds = chain_seeds(3, C)
    rows = np.sort(rng.choice(F, 41, replace=False))
    labels = rng.integers(0, C, len(rows))
    o = rng.permutation(len(rows))
    results = []
    for r, l in ((rows, labels), (rows[o], labels[o])):
        st = DeviceState(*init)
        st.fit(ce.ops, Xd, r, l, seeds)
        want = sgd_partial_fit(X[r], l, *init, seeds=seeds)[:3]
        assert_state(st.host(), want, (D, ld, shift))
        results.append(want[0])
    assert not same_bits(results[0], results[1])


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("n", [0, 1, 2, 3, 63, 64, 65, 400])
def test_batch_sizes(ce, n, C):
    """The chunks of 4 rows and the 64-row blocks of the visiting order; n = 0 leaves the model and its t untouched."""
    rng = np.random.default_rng(10 * n + C)
    F, D = 500, 20
    X = rng.normal(0, 1, (F, D))
    coef, b, t = model(rng, C, D)
    seeds = chain_seeds(n, C)
    st = DeviceState(coef, b, t)
    rows, labels = np.sort(rng.choice(F, n, replace=False)), rng.integers(0, C, n)
    st.fit(ce.ops, dev(X), rows, labels, seeds)
    assert_state(st.host(), sgd_partial_fit(X[rows], labels, coef, b, t, seeds=seeds)[:3], (n, C))
    if n == 0:
        assert_state(st.host(), (coef, b, t), "untouched")


@pytest.mark.parametrize("C,n", [(2, PERM_LDS), (2, PERM_LDS + 1), (4, PERM_LDS // 4), (4, PERM_LDS // 4 + 1)])
def test_permutation_threshold(ce, C, n):
    """One n on each side of the threshold between the permutations in shared memory and in the workspace."""
    rng = np.random.default_rng(n + C)
    F, D = 600, 3
    K = 1 if C == 2 else C
    assert (K * n <= PERM_LDS) == (ce.load().ce_sgd_partial_fit_workspace_bytes(n, C) == 0)
    X = rng.normal(0, 1, (F, D))
    coef, b, t = model(rng, C, D)
    seeds = chain_seeds(11, C)
    rows, labels = rng.integers(0, F, n), rng.integers(0, C, n)
    st = DeviceState(coef, b, t)
    st.fit(ce.ops, dev(X), rows, labels, seeds)
    assert_state(st.host(), sgd_partial_fit(X[rows], labels, coef, b, t, seeds=seeds)[:3], (C, n))
    assert st.status.tolist() == [0]


def test_workspace_models_among_others(ce):
    """Models whose permutations need the workspace next to ones that do not and an empty one; then the same
    call without a workspace: those models are flagged 2 and left untouched, the others updated."""
    rng = np.random.default_rng(31)
    F, D, C = 700, 4, 3
    X = rng.normal(0, 1, (F, D))
    Xd = dev(X)
    n = np.array([10, 3000, 0, 2800, 7])
    U = len(n)
    ro = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rows, labels = rng.integers(0, F, ro[-1]), rng.integers(0, C, ro[-1]).astype(np.int32)
    models = [model(rng, C, D) for _ in range(U)]
    seeds = np.stack([chain_seeds(u, C) for u in range(U)])
    stacked = [np.stack([m[i] for m in models]) for i in range(3)]
    want = [sgd_partial_fit(X[rows[ro[u]:ro[u + 1]]], labels[ro[u]:ro[u + 1]], *models[u], seeds=seeds[u])[:3] for u in range(U)]
    st = DeviceState(*stacked)
    st.fit(ce.ops, Xd, rows, labels, seeds, row_offsets=dev(ro))
    got = st.host()
    for u in range(U):
        assert_state([g[u] for g in got], want[u], u)
    assert st.status.tolist() == [0] * U
    # the C-ABI without a workspace
    st = DeviceState(*stacked)
    rd, ld_, rod, sd = dev(rows.astype(np.int64)), dev(labels), dev(ro), dev(seeds.view(np.int32))
    p = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = ce.load().ce_sgd_partial_fit(p(Xd), F, D, D, p(rd), p(ld_), p(rod), U, C, 1e-4, ce.ops.sgd_optimal_init(1e-4), p(sd),
                                      0, p(st.coef), p(st.b), p(st.t), p(st.status), None, 0,
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    torch.cuda.synchronize()
    got = st.host()
    assert st.status.tolist() == [0, 2, 0, 2, 0]
    for u in range(U):
        assert_state([g[u] for g in got], models[u] if n[u] > 2000 else want[u], (u, "no workspace"))


def test_many_models(ce):
    """U = 300 models in one launch, ragged batches, empty batches at the first,
    a middle and the last model, every model its own seeds."""
    rng = np.random.default_rng(300)
    U, F, C, D = 300, 1500, 4, 33
    X = rng.normal(0, 1, (F, D))
    models = [model(rng, C, D) for _ in range(U)]
    seeds = np.stack([chain_seeds(1000 + u, C) for u in range(U)])
    assert len({tuple(s) for s in seeds}) == U
    n = rng.integers(1, 40, U)
    n[0] = n[U // 2] = n[U - 1] = 0
    ro = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    rows = np.concatenate([np.sort(rng.choice(F, k, replace=False)) for k in n]).astype(np.int64)
    labels = rng.integers(0, C, len(rows)).astype(np.int32)
    st = DeviceState(*[np.stack([m[i] for m in models]) for i in range(3)])
    st.fit(ce.ops, dev(X), rows, labels, seeds, row_offsets=dev(ro))
    got = st.host()
    for u in range(U):
        r, l = rows[ro[u]:ro[u + 1]], labels[ro[u]:ro[u + 1]]
        want = sgd_partial_fit(X[r], l, *models[u], seeds=seeds[u])[:3]
        if n[u] == 0:
            assert_state(want, models[u], "the restatement leaves an empty batch alone")
        assert_state([g[u] for g in got], want, u)
    assert st.status.tolist() == [0] * U


@pytest.mark.parametrize("C", [2, 4])
@pytest.mark.parametrize("alpha", [1.0, 10.0])
def test_zero_shrink_factor_and_reset(ce, alpha, C):
    """alpha >= 1 from a fresh model at t = 1: the first rows' factor max(0, 1 - eta * alpha) is exactly 0,
    so wscale drops below 1e-9 and w is reset before the add."""
    from sgd_fit_ref import optimal_init

    assert 1.0 - (1.0 / (alpha * (optimal_init(alpha) + 1.0 - 1.0))) * alpha <= 0.0
    rng = np.random.default_rng(int(alpha) + C)
    F, D = 100, 17
    X = rng.normal(0, 1, (F, D))
    coef, b, t = model(rng, C, D, fresh=True)
    seeds = chain_seeds(5, C)
    st = DeviceState(coef, b, t)
    for n in (3, 50):
        rows, labels = np.sort(rng.choice(F, n, replace=False)), rng.integers(0, C, n)
        st.fit(ce.ops, dev(X), rows, labels, seeds, alpha=alpha)
        coef, b, t, _ = sgd_partial_fit(X[rows], labels, coef, b, t, alpha, seeds=seeds)
        assert_state(st.host(), (coef, b, t), (alpha, C, n))
    assert t == 54.0


@pytest.mark.parametrize("C", [2, 3])
def test_large_rows_and_one_class(ce, C):
    """Rows x 1e3 reach p <= -37 (the gradient's other branch); then a batch made of one class only."""
    from sgd_fit_ref import dot

    rng = np.random.default_rng(C)
    F, D = 80, 12
    X = rng.normal(0, 1, (F, D)) * 1e3
    coef, b, t = model(rng, C, D)
    assert min(dot(w, x) for w in coef for x in X) + b.max() <= -37.0
    seeds = chain_seeds(9, C)
    st = DeviceState(coef, b, t)
    for labels in (rng.integers(0, C, 40), np.full(40, C - 1), np.zeros(40, int)):
        rows = np.sort(rng.choice(F, 40, replace=False))
        st.fit(ce.ops, dev(X), rows, labels, seeds)
        coef, b, t, finite = sgd_partial_fit(X[rows], labels, coef, b, t, seeds=seeds)
        assert finite
        assert_state(st.host(), (coef, b, t), (C, labels[:3]))


def test_overflow_sets_the_flag_of_that_model_only(ce):
    """Rows x 1e300 overflow one model's weights (ordinary inf / NaN arithmetic): its flag is set where sklearn
    would raise, its parameters are what the arithmetic gives, its neighbours are bit-exact and unflagged."""
    rng = np.random.default_rng(6)
    F, D, C, U = 90, 10, 3, 3
    X = rng.normal(0, 1, (F, D))
    X[30:60] *= 1e300
    models = [model(rng, C, D) for _ in range(U)]
    rows = np.concatenate([np.arange(0, 30), np.arange(30, 60), np.arange(60, 90)])
    ro = np.array([0, 30, 60, 90], np.int64)
    labels = rng.integers(0, C, 90)
    m = ce.DeviceSGDClassifier(*[np.stack([mm[i] for mm in models]) for i in range(3)], random_state=[4, 5, 6])
    m.partial_fit(dev(X), dev(rows), dev(labels), dev(ro))
    s = m.state()
    assert s["status"].tolist() == [0, 1, 0]
    for u in range(U):
        want = sgd_partial_fit(X[rows[ro[u]:ro[u + 1]]], labels[ro[u]:ro[u + 1]], *models[u], random_state=4 + u)
        assert want[3] == (u != 1)
        assert_state((s["coef"][u], s["intercept"][u], s["t"][u]), want[:3], u)
    assert not np.isfinite(s["coef"][1]).all()
    with pytest.raises(ValueError, match=r"Floating-point under-/overflow occurred at epoch #1.*\[1\]"):
        m.check_finite()


def test_log_dloss_variant(ce):
    """sklearn 0.24.1's gradient (Log.dloss), against its restatement: both of its tails (|z| > 18) are reached."""
    rng = np.random.default_rng(24)
    F, D, C = 150, 65, 4
    X = rng.normal(0, 1, (F, D)) * 3.0
    coef, b, t = model(rng, C, D)
    seeds = chain_seeds(24, C)
    st = DeviceState(coef, b, t)
    rows, labels = np.sort(rng.choice(F, 100, replace=False)), rng.integers(0, C, 100)
    st.fit(ce.ops, dev(X), rows, labels, seeds, grad="log_dloss")
    want = sgd_partial_fit(X[rows], labels, coef, b, t, seeds=seeds, grad="log_dloss")[:3]
    assert_state(st.host(), want, "log_dloss")
    assert not same_bits(want[0], sgd_partial_fit(X[rows], labels, coef, b, t, seeds=seeds)[0])
    z = X[rows] @ coef.T + b
    assert (z > 18).any() and (z < -18).any()
    with pytest.raises(ValueError, match="grad"):
        st.fit(ce.ops, dev(X), rows, labels, seeds, grad="hinge")


def test_partial_fit_in_a_hip_graph(ce):
    """One sgd_partial_fit captured in a HIP graph and replayed twice equals two eager calls, with and without row_offsets."""
    rng = np.random.default_rng(77)
    U, C, D, F = 3, 4, 260, 400
    X = rng.normal(0, 1, (F, D))
    Xd = dev(X)
    models = [model(rng, C, D) for _ in range(U)]
    n = np.array([30, 0, 45])
    ro = dev(np.concatenate([[0], np.cumsum(n)]).astype(np.int64))
    rows = dev(np.concatenate([np.sort(rng.choice(F, k, replace=False)) for k in n]).astype(np.int64))
    labels = dev(rng.integers(0, C, int(n.sum())).astype(np.int32))
    seeds = dev(np.stack([chain_seeds(u, C) for u in range(U)]).view(np.int32))  # on the device: nothing to copy in the capture
    stacked = [np.stack([m[i] for m in models]) for i in range(3)]

    def run(st, **kw):
        ce.ops.sgd_partial_fit(Xd, kw.get("rows", rows), kw.get("labels", labels), st.coef, st.b, st.t, kw.get("ro", ro),
                               seeds=kw.get("seeds", seeds), status=st.status)

    eager, graphed = DeviceState(*stacked), DeviceState(*stacked)
    for _ in range(2):
        run(eager)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        run(graphed)
    assert_state(graphed.host(), stacked, "capture runs nothing")
    for _ in range(2):
        g.replay()
    torch.cuda.synchronize()
    assert_state(graphed.host(), eager.host(), "graph")
    want = sgd_partial_fit(X[rows[:30].cpu().numpy()], labels[:30].cpu().numpy(), *models[0], seeds=chain_seeds(0, C))
    want = sgd_partial_fit(X[rows[:30].cpu().numpy()], labels[:30].cpu().numpy(), *want[:3], seeds=chain_seeds(0, C))
    assert_state([x[0] for x in eager.host()], want[:3], "two eager calls")
    # the one-model form builds its row_offsets on the device: capturable too
    one = dict(rows=rows[:30].contiguous(), labels=labels[:30].contiguous(), ro=None, seeds=seeds[0].contiguous())
    one_e, one_g = DeviceState(*models[0]), DeviceState(*models[0])
    for _ in range(2):
        run(one_e, **one)
    torch.cuda.synchronize()
    g1 = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        run(one_g, **one)
    for _ in range(2):
        g1.replay()
    torch.cuda.synchronize()
    assert_state(one_g.host(), one_e.host(), "graph, one model")
    assert_state(one_g.host(), want[:3], "graph, one model, restatement")


def test_no_rows_at_all(ce):
    """Every batch empty (an epoch that picked nothing): nothing is launched and nothing changes."""
    rng = np.random.default_rng(9)
    C, D = 4, 16
    Xd = dev(rng.normal(0, 1, (50, D)))
    none64, none32 = torch.zeros(0, dtype=torch.int64, device="cuda"), torch.zeros(0, dtype=torch.int32, device="cuda")
    models = [model(rng, C, D) for _ in range(3)]
    st = DeviceState(*[np.stack([m[i] for m in models]) for i in range(3)])
    before = st.host()
    status = ce.ops.sgd_partial_fit(Xd, none64, none32, st.coef, st.b, st.t, torch.zeros(4, dtype=torch.int64, device="cuda"),
                                    seeds=np.stack([chain_seeds(0, C)] * 3))
    assert status.tolist() == [0, 0, 0]
    assert_state(st.host(), before, "no rows")


# ---------------------------------------------------------------------------
# end to end: predict -> select -> retrain -> shrink, 3 epochs.  After every
# epoch the member equals the restatement fed the picks the device session
# returned (so nothing here depends on the SGD predict's 1e-10 tolerance).
# ---------------------------------------------------------------------------
Q, EPOCHS, D_E2E, C_E2E = 10, 3, 65, 4


def e2e_pool(rng, n_songs, order):
    s_id = np.repeat(np.arange(n_songs), rng.integers(1, 8, n_songs))
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


def picked_songs(picks, N, h2m):
    """q_songs of amg_test.py:484: a committee pick is its song, an hc pick its twin in the pool (if any)."""
    songs = [int(p) if p < N else int(h2m[p - N]) for p in picks if p >= 0]
    return np.array([s for s in songs if s >= 0], np.int64)


def host_retrain(X, s_id, song_labels, songs, state, random_state):
    """mod.partial_fit(X_train[X_train.index.isin(q_songs)], ...): X_train's row order, a song once."""
    batch = np.isin(s_id, songs)
    if not batch.any():
        return state
    return sgd_partial_fit(X[batch], song_labels[s_id[batch]], *state, random_state=random_state)[:3]


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_end_to_end_one_user(ce, mode, order):
    rng = np.random.default_rng(len(mode) * 2 + (order == "grouped"))
    N = 80
    s_id, X, song_labels = e2e_pool(rng, N, order)
    state = model(rng, C_E2E, D_E2E)
    kw, h2m = {}, None
    if mode == "mix":
        hc, h2m = e2e_table(rng, N)
        kw = dict(hc=hc, hc_to_mc=h2m)
    sess = ce.SelectionSession(Q, mode, N, s_id=s_id, **kw)
    m = ce.DeviceSGDClassifier(*state, random_state=12)
    Xd = dev(X)
    seen = set()
    for e in range(EPOCHS):
        picks = np.asarray(sess.select(frames=[m.predict_proba(Xd)]))
        assert len(picks) == Q and not seen & set(picks.tolist())  # the pool shrinks
        seen |= set(picks.tolist())
        m.partial_fit_picks(Xd, sess, picks, song_labels)
        state = host_retrain(X, s_id, song_labels, picked_songs(picks, N, h2m), state, 12)
        s = m.state()
        assert_state((s["coef"][0], s["intercept"][0], s["t"]), state, (mode, order, e))
    m.check_finite()


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
@pytest.mark.parametrize("mode", ["mc", "mix"])
def test_end_to_end_batched(ce, mode, order):
    """U = 3 ragged users, one model each: one partial_fit launch per epoch for
    all of them; picks from select (host lists) and from step (the device tensor)."""
    rng = np.random.default_rng(50 + len(mode) * 2 + (order == "grouped"))
    users = [80, 30, 55]
    U = len(users)
    off = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    s_id, X, song_labels = e2e_pool(rng, int(off[-1]), order)  # the stacked songs' ids: user u owns off[u]:off[u+1]
    user_rows = [np.flatnonzero((s_id >= off[u]) & (s_id < off[u + 1])) for u in range(U)]
    kw, tabs = {}, [(None, None)] * U
    if mode == "mix":
        tabs = [e2e_table(rng, n) for n in users]
        off_h = np.concatenate([[0], np.cumsum([len(t[1]) for t in tabs])]).astype(np.int64)
        kw = dict(hc=np.concatenate([t[0] for t in tabs]), hc_offsets=off_h, hc_to_mc=np.concatenate([t[1] for t in tabs]))
    _, f_off, f_perm = ce.song_groups(s_id)
    Xd = dev(X)
    rows_d = [dev(r) for r in user_rows]
    init = [model(rng, C_E2E, D_E2E) for _ in range(U)]
    for device_picks in (False, True):
        states = list(init)
        sess = ce.BatchedSelectionSession(Q, mode, off, frame_offsets=f_off, frame_perm=f_perm, **kw)
        m = ce.DeviceSGDClassifier(*[np.stack([s[i] for s in states]) for i in range(3)], random_state=[7, 8, 9])
        p = torch.empty((len(s_id), C_E2E), dtype=torch.float64, device="cuda")
        for e in range(EPOCHS):
            for u in range(U):
                p[rows_d[u]] = m.predict_proba(Xd, u)[rows_d[u]]
            if device_picks:
                idx = sess.step(frames=[p])
                m.partial_fit_picks(Xd, sess, idx, song_labels)
                picks = sess.account(idx)
            else:
                picks = sess.select(frames=[p])
                m.partial_fit_picks(Xd, sess, picks, song_labels)
            s = m.state()
            for u in range(U):
                songs = picked_songs(np.asarray(picks[u]), users[u], tabs[u][1])
                assert len(songs) > 0
                states[u] = host_retrain(X[user_rows[u]], s_id[user_rows[u]] - off[u], song_labels[off[u]:off[u + 1]],
                                         songs, states[u], 7 + u)
                assert_state((s["coef"][u], s["intercept"][u], s["t"][u]), states[u], (mode, order, e, u, device_picks))
        m.check_finite()
