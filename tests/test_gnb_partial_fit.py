"""GaussianNB.partial_fit (amg_test.py:509) without a GPU: the row-loop
restatement (tests/gnb_fit_ref.py) against sklearn and the committed fixture,
bit for bit; the C-ABI's refusals; ops.batch_rows and the sessions' songs_of
against the reference's isin rule (:484 / :491) on pandas frames."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from gnb_fit_ref import gnb_partial_fit, same_bits

DS = [2, 3, 7, 8, 9, 260]
BATCHES = [1, 2, 7, 8, 9, 129, 400]


def assert_state(got, want, what):
    for name, g, w in zip(("theta", "var", "class_count", "class_prior", "epsilon"), got, want):
        assert same_bits(g, w), (what, name)


@pytest.mark.parametrize("C", [2, 4, 8])
@pytest.mark.parametrize("D", DS)
def test_restatement_equals_sklearn(D, C):
    """Chained updates: every batch size, a class unseen until a later batch
    (the last class, first in the 9-row batch), a one-class batch, a -0.0 column."""
    pytest.importorskip("sklearn")
    from sklearn.naive_bayes import GaussianNB

    rng = np.random.default_rng(100 * D + C)
    X0, y0 = rng.normal(size=(3 * C, D)), np.arange(3 * C) % (C - 1)  # class C - 1 unseen
    g = GaussianNB().partial_fit(X0, y0, classes=np.arange(C))
    assert g.class_count_[C - 1] == 0
    th, va, cc = g.theta_.copy(), g.var_.copy(), g.class_count_.copy()
    for B in BATCHES + [5]:
        X = rng.normal(size=(B, D)) * rng.choice([1.0, 1e-3, 1e3])
        y = rng.integers(0, C - 1, B) if B < 9 else rng.integers(0, C, B)
        if B == 9:
            y[0] = C - 1
        if B == 5:
            y[:] = 1  # one class
        if B == 8:
            X[:, 0] = -0.0
        g.partial_fit(X, y)
        th, va, cc, prior, eps = gnb_partial_fit(X, y, th, va, cc)
        assert_state((th, va, cc, prior, eps), (g.theta_, g.var_, g.class_count_, g.class_prior_, g.epsilon_), (D, C, B))
    assert g.class_count_[C - 1] > 0


@pytest.mark.parametrize("C", [2, 4, 8])
@pytest.mark.parametrize("D", [2, 65, 260, 512])
def test_restatement_equals_sklearn_past_the_row_tile(D, C):
    """Chained batches of 1024, 1025, 2049 and 3000 rows (the device kernel stages
    1024 rows at a time; tests/test_gpu_fit_batch_edges.py compares it with the
    restatement there): the last class unseen until the second batch, where it
    holds row 1024 alone."""
    pytest.importorskip("sklearn")
    from sklearn.naive_bayes import GaussianNB

    rng = np.random.default_rng(7000 * D + C)
    X0, y0 = rng.normal(size=(3 * C, D)), np.arange(3 * C) % (C - 1)
    g = GaussianNB().partial_fit(X0, y0, classes=np.arange(C))
    assert g.class_count_[C - 1] == 0
    th, va, cc = g.theta_.copy(), g.var_.copy(), g.class_count_.copy()
    for B in (1024, 1025, 2049, 3000):
        X = rng.normal(size=(B, D)) * np.exp(rng.normal(0, 1, D))
        y = rng.integers(0, C - 1, B) if B <= 1025 else rng.integers(0, C, B)
        if B == 1025:
            y[1024] = C - 1
        g.partial_fit(X, y)
        th, va, cc, prior, eps = gnb_partial_fit(X, y, th, va, cc)
        assert_state((th, va, cc, prior, eps), (g.theta_, g.var_, g.class_count_, g.class_prior_, g.epsilon_), (D, C, B))
        if B <= 1025:
            assert cc[C - 1] == B - 1024  # unseen, then its one row
    assert g.class_count_[C - 1] > 1


def test_restatement_nan_cell():
    """One NaN cell: epsilon is NaN and var is all NaN, in sklearn and in the restatement."""
    pytest.importorskip("sklearn")
    from sklearn.naive_bayes import GaussianNB

    rng = np.random.default_rng(5)
    g = GaussianNB().partial_fit(rng.normal(size=(12, 6)), np.arange(12) % 3, classes=np.arange(3))
    th, va, cc = g.theta_.copy(), g.var_.copy(), g.class_count_.copy()
    X, y = rng.normal(size=(10, 6)), np.arange(10) % 2
    X[4, 2] = np.nan
    # sklearn refuses NaN at its door (validate_data); the arithmetic behind the door is what the device follows
    from unittest import mock

    with mock.patch("sklearn.naive_bayes.validate_data", lambda self, X, y, reset: (X, y)):
        g.partial_fit(X, y)
    got = gnb_partial_fit(X, y, th, va, cc)
    assert np.isnan(got[4]) and np.isnan(got[1]).all()
    assert_state(got, (g.theta_, g.var_, g.class_count_, g.class_prior_, g.epsilon_), "nan")


@pytest.mark.parametrize("D", [12, 260])
def test_restatement_equals_fixture(D):
    fx = {k[len(f"d{D}_"):]: v for k, v in golden("gnb_partial_fit").items() if k.startswith(f"d{D}_")}
    th, va, cc = fx["theta_init"], fx["var_init"], fx["cc_init"]
    assert fx["X"].shape[1] == D and cc[3] == 0
    for e in range(3):
        th, va, cc, prior, eps = gnb_partial_fit(fx["X"][fx[f"rows{e}"]], fx[f"labels{e}"], th, va, cc)
        assert_state((th, va, cc, prior, eps), [fx[f"{k}{e}"] for k in ("theta", "var", "cc", "prior", "eps")], (D, e))


def test_fixture_is_small():
    import os

    from conftest import GOLDEN

    assert os.path.getsize(os.path.join(GOLDEN, "gnb_partial_fit.npz")) < 256 * 1024


def test_partial_fit_validates_without_gpu():
    from ce_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)

    def rc(D=4, ld=4, U=1, C=4, theta=p, var=p, cc=p):
        return lib.ce_gnb_partial_fit(p, 10, D, ld, p, p, p, U, C, 1e-9, theta, var, cc, p, p, None)

    assert rc(D=1, ld=1) == _lib.CE_EUNSUPPORTED and b"D >= 2" in lib.ce_last_error()
    assert rc(D=513, ld=513) == _lib.CE_EINVAL
    assert rc(C=9) == _lib.CE_EINVAL and rc(C=1) == _lib.CE_EINVAL
    assert rc(U=0) == _lib.CE_EINVAL
    assert rc(ld=3) == _lib.CE_EINVAL
    for kw in ({"theta": None}, {"var": None}, {"cc": None}):
        assert rc(**kw) == _lib.CE_EINVAL


def test_python_guards_without_gpu():
    torch = pytest.importorskip("torch")
    from ce_amd import ops

    z = torch.zeros((4, 4), dtype=torch.float64)
    with pytest.raises(ValueError, match="HIP device"):
        ops.gnb_partial_fit(z, torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int32), z[:2], z[:2], z[0, :2])
    with pytest.raises(ValueError, match=r"\[0, 4\)"):
        ops.batch_rows(torch.tensor([0]), torch.tensor([0, 2, 3]), song_labels=[0, 4], n_classes=4)
    with pytest.raises(ValueError, match="one class per song"):
        ops.batch_rows(torch.tensor([0]), torch.tensor([0, 2, 3]), song_labels=[0, 1, 2])
    # a position outside the user's pool: refused from the host, dropped (never another user's song) as a tensor
    off, io, lab = torch.tensor([0, 2, 3, 5, 6]), [0, 2, 4], [0, 1, 2, 3]
    with pytest.raises(ValueError, match="positions in the user's pool"):
        ops.batch_rows([[0, 2], [1, -1]], off, song_labels=lab, item_offsets=io)
    with pytest.raises(ValueError, match="positions in the user's pool"):
        ops.batch_rows([4], off, song_labels=lab)
    rows, labels, ro = ops.batch_rows(torch.tensor([[0, 2], [1, 7]]), off, song_labels=lab, item_offsets=torch.tensor(io))
    assert rows.tolist() == [0, 1, 5] and labels.tolist() == [0, 0, 3] and ro.tolist() == [0, 2, 3]
    rows, labels, ro = ops.batch_rows(torch.tensor([[-1, -1], [-1, -1]]), off, song_labels=lab, item_offsets=torch.tensor(io))
    assert rows.numel() == 0 and labels.dtype == torch.int32 and ro.tolist() == [0, 0, 0]


# ---------------------------------------------------------------------------
# batch_rows vs X_train[X_train.index.isin(q_songs)]  (amg_test.py:491)
# ---------------------------------------------------------------------------
def isin_rows(s_id, q_songs):
    """The frame rows of X_batch and their songs, by pandas."""
    import pandas as pd

    X_train = pd.DataFrame({"row": np.arange(len(s_id))}, index=pd.Index(s_id, name="s_id"))
    X_batch = X_train[X_train.index.isin(q_songs)]
    return X_batch["row"].to_numpy(), X_batch.index.to_numpy()


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_batch_rows_one_user(order):
    torch = pytest.importorskip("torch")
    pytest.importorskip("pandas")
    from ce_amd import ops, song_groups

    rng = np.random.default_rng(17 + (order == "grouped"))
    N = 40
    ids = np.arange(N) * 3 + 7
    s_id = np.repeat(ids, rng.integers(1, 10, N))
    if order == "shuffled":
        s_id = rng.permutation(s_id)
    uniq, off, perm = song_groups(s_id)
    assert (perm is None) == (order == "grouped")
    song_labels = rng.integers(0, 4, N)
    for picks in ([5, 0, 39, 17], [3, 3, 12, -1, 3], [-1, -1], list(range(N))[::-1]):
        rows, labels, ro = ops.batch_rows(torch.tensor(picks), torch.from_numpy(off),
                                          None if perm is None else torch.from_numpy(perm), song_labels, n_classes=4)
        want_rows, want_ids = isin_rows(s_id, [ids[p] for p in picks if p >= 0])
        assert rows.dtype == torch.int64 and labels.dtype == torch.int32 and ro.dtype == torch.int64
        assert np.array_equal(rows.numpy(), want_rows), picks
        assert np.array_equal(labels.numpy(), song_labels[np.searchsorted(ids, want_ids)])
        assert ro.tolist() == [0, len(want_rows)]


@pytest.mark.parametrize("order", ["grouped", "shuffled"])
def test_batch_rows_ragged_users(order):
    """U users over the stacked songs (user-local picks, -1 padding, an empty
    user, a user with no pick): each user's rows are its own isin rows."""
    torch = pytest.importorskip("torch")
    pytest.importorskip("pandas")
    from ce_amd import ops, song_groups

    rng = np.random.default_rng(23 + (order == "grouped"))
    users = [6, 0, 11, 1, 9]
    off_u = np.concatenate([[0], np.cumsum(users)]).astype(np.int64)
    T = int(off_u[-1])
    s_id = np.repeat(np.arange(T), rng.integers(1, 6, T))
    if order == "shuffled":
        s_id = rng.permutation(s_id)
    _, off, perm = song_groups(s_id)
    song_labels = rng.integers(0, 4, T)
    picks = np.full((len(users), 5), -1, np.int64)
    picks[0, :4] = [5, 2, 2, 0]
    picks[2] = [10, 0, 3, 3, 7]
    picks[3, 2] = 0  # padding in front of the pick
    rows, labels, ro = ops.batch_rows(torch.from_numpy(picks), torch.from_numpy(off),
                                      None if perm is None else torch.from_numpy(perm),
                                      torch.from_numpy(song_labels), item_offsets=torch.from_numpy(off_u))
    assert ro.shape == (len(users) + 1,) and ro[0] == 0 and ro[-1] == rows.numel()
    for u in range(len(users)):
        q_songs = [off_u[u] + p for p in picks[u] if p >= 0]
        want_rows, want_ids = isin_rows(s_id, q_songs)
        assert np.array_equal(rows[ro[u]:ro[u + 1]].numpy(), want_rows), u
        assert np.array_equal(labels[ro[u]:ro[u + 1]].numpy(), song_labels[want_ids]), u
    assert ro[2] == ro[1] and ro[5] == ro[4]  # the empty user, the user without a pick


# ---------------------------------------------------------------------------
# songs_of vs the isin rule of amg_test.py:484 / :491
# ---------------------------------------------------------------------------
def isin_songs(picks, ids_mc, ids_hc):
    """q_songs as the reference names them (song ids of the mix picks: a
    committee row's or an hc row's), then the committee rows isin keeps."""
    import pandas as pd

    N = len(ids_mc)
    q_songs = [ids_mc[p] if p < N else ids_hc[p - N] for p in picks if p >= 0]
    return np.flatnonzero(pd.Index(ids_mc).isin(q_songs))


def test_songs_of_mix_and_mc():
    pytest.importorskip("torch")
    pytest.importorskip("pandas")
    import ce_amd

    N = 12
    ids_mc = np.arange(N) * 2 + 100
    h2m = np.array([4, -1, 0, 11, -1, 7, 2], np.int64)            # hc rows in their own order; two songs outside the pool
    ids_hc = np.where(h2m >= 0, ids_mc[np.clip(h2m, 0, None)], 9000 + np.arange(len(h2m)))
    hc = np.full((len(h2m), 4), 0.25)
    s = ce_amd.SelectionSession(4, "mix", N, hc=hc, hc_to_mc=h2m, device="cpu")
    for picks in ([3, N + 0, N + 1, 9],        # a twin, a -1 twin
                  [4, N + 0, 7, N + 5],        # songs picked through both parts
                  [N + 4, N + 1, -1, -1],      # only -1 twins, padding
                  [11, 0, 5, 2]):
        got = s.songs_of(np.array(picks))
        assert got.dtype == np.int64 and np.array_equal(got, isin_songs(picks, ids_mc, ids_hc)), picks
    mc = ce_amd.SelectionSession(4, "mc", N, device="cpu")
    assert mc.songs_of(np.array([5, 1, -1, 3])).tolist() == [5, 1, 3]
    with pytest.raises(ValueError, match="no committee"):
        ce_amd.SelectionSession(4, "hc", N, hc=hc, device="cpu").songs_of([0])


def test_batched_songs_of():
    torch = pytest.importorskip("torch")
    pytest.importorskip("pandas")
    import ce_amd

    off = np.array([0, 5, 5, 12], np.int64)
    off_h = np.array([0, 3, 3, 7], np.int64)
    h2m = np.array([2, -1, 4, 6, 0, -1, 3], np.int64)  # user-local twins
    hc = np.full((7, 4), 0.25)
    s = ce_amd.BatchedSelectionSession(4, "mix", off, hc=hc, hc_offsets=off_h, hc_to_mc=h2m, device="cpu")
    picks = [np.array([1, 5 + 0, 5 + 1, 2]), np.zeros(0, np.int64), np.array([7 + 1, 0, 7 + 0, 6])]
    got = s.songs_of(picks)
    for u, p in enumerate(picks):
        n = off[u + 1] - off[u]
        ids_mc = np.arange(n) + 50
        hu = h2m[off_h[u]:off_h[u + 1]]
        ids_hc = np.where(hu >= 0, ids_mc[np.clip(hu, 0, None)] if n else 0, 9000 + np.arange(len(hu)))
        assert np.array_equal(got[u], isin_songs(p, ids_mc, ids_hc)), u
    # the device form (what step returns): the same songs slot by slot, -1 where a slot names none
    idx = torch.tensor([[1, 5, 6, 2], [-1, -1, -1, -1], [8, 0, 7, 6]])
    t = s.songs_of(idx)
    assert t.tolist() == [[1, 2, -1, 2], [-1, -1, -1, -1], [0, 0, 6, 6]]
    for u in range(3):
        assert np.array_equal(np.unique(t[u][t[u] >= 0].numpy()), got[u])
    mc = ce_amd.BatchedSelectionSession(4, "mc", off, device="cpu")
    assert [a.tolist() for a in mc.songs_of([np.array([3, -1, 0]), np.zeros(0, np.int64), np.array([6])])] == [[3, 0], [], [6]]
