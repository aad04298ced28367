"""The users form of the linear members' predict_proba, the parts that need no
GPU: the two entry points' refusals (ce_gnb_predict_proba_users,
ce_sgd_predict_proba_users), the Python validation in front of them, and the
numpy statement of "who owns row r" that the GPU tests compare against."""
import ctypes

import numpy as np
import pytest

from members_users_ref import excl_words, row_owners


def test_entry_points_refuse_without_gpu():
    from ce_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(16)
    for name in ("ce_gnb_predict_proba_users", "ce_sgd_predict_proba_users"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)

    def gnb(F=10, D=260, ld=None, C=4, U=2, items=p, frames=p, perm=None, excl=None, ldo=None):
        return lib.ce_gnb_predict_proba_users(p, F, D, D if ld is None else ld, p, p, p, C, U, items, frames, perm, excl, p,
                                              C if ldo is None else ldo, None)

    def sgd(F=10, D=260, ld=None, K=4, C=4, U=2, items=p, frames=p, perm=None, excl=None, ldo=None):
        return lib.ce_sgd_predict_proba_users(p, F, D, D if ld is None else ld, p, p, K, C, U, items, frames, perm, excl, p,
                                              C if ldo is None else ldo, None)

    for f in (gnb, sgd):
        assert f(D=513) == _lib.CE_EINVAL
        assert f(C=9, **({"K": 9} if f is sgd else {})) == _lib.CE_EINVAL
        assert f(U=0) == _lib.CE_EINVAL and f(U=-1) == _lib.CE_EINVAL
        assert f(items=None) == _lib.CE_EINVAL and f(frames=None) == _lib.CE_EINVAL
        assert b"offsets" in lib.ce_last_error()
        assert f(ld=259) == _lib.CE_EINVAL
        assert f(ldo=3) == _lib.CE_EINVAL
        assert f(F=-1) == _lib.CE_EINVAL
        assert f(F=0) == _lib.CE_OK  # no frame: nothing launched
        assert f(F=0, perm=p, excl=p) == _lib.CE_OK
    for D in range(1, 8):  # fewer than 8 features: numpy's sequential sum, not the 8-lane plan
        assert gnb(D=D) == _lib.CE_EUNSUPPORTED
        assert sgd(D=D, F=0) == _lib.CE_OK  # SGD takes them
    assert sgd(K=3, C=4) == _lib.CE_EINVAL
    assert sgd(K=1, C=3) == _lib.CE_EINVAL and sgd(K=4, C=3) == _lib.CE_EINVAL
    assert sgd(K=1, C=2, F=0) == _lib.CE_OK


def small_sessions(ce_amd):
    """(one-user session, batched session of 3 users, rows) on the CPU: geometry only."""
    s_id = np.array([2, 0, 1, 2, 0, 3, 3, 1, 4, 5, 5, 4])
    one = ce_amd.SelectionSession(2, "mc", 6, s_id=s_id, device="cpu")
    off = np.array([0, 2, 2, 6])
    _, f_off, f_perm = ce_amd.song_groups(s_id)
    bat = ce_amd.BatchedSelectionSession(2, "mc", off, frame_offsets=f_off, frame_perm=f_perm, device="cpu")
    return one, bat, len(s_id)


def test_python_validation_without_gpu():
    torch = pytest.importorskip("torch")
    import ce_amd

    one, bat, F = small_sessions(ce_amd)
    C, D = 4, 8
    assert one._rows == F and bat._rows == F
    grouped = ce_amd.BatchedSelectionSession(2, "mc", [0, 2], frame_offsets=[0, 3, 7], device="cpu")
    assert grouped._rows == 7
    short_perm = ce_amd.BatchedSelectionSession(2, "mc", [0, 2], frame_offsets=[0, 1, 3], frame_perm=[4, 0, 9, 30],
                                                device="cpu")
    assert short_perm._rows == 10  # max over the positions the offsets name, + 1
    nb = {U: ce_amd.DeviceGaussianNB(np.zeros((U, C, D)), np.ones((U, C, D)), np.ones((U, C)), device="cpu")
          for U in (1, 3)}
    sgd = {U: ce_amd.DeviceSGDClassifier(np.zeros((U, C, D)), np.zeros((U, C)), 1.0, random_state=0, device="cpu")
           for U in (1, 3)}
    X = torch.zeros((F, D), dtype=torch.float64)
    for members in (nb, sgd):
        with pytest.raises(ValueError, match=r"3 user\(s\), this member 1 model"):
            members[1].predict_proba_session(X, bat)
        with pytest.raises(ValueError, match=r"1 user\(s\), this member 3 model"):
            members[3].predict_proba_session(X, one)
        for m, sess in ((members[1], one), (members[3], bat)):
            with pytest.raises(ValueError, match=f"X has {F - 1} rows.*names {F}"):
                m.predict_proba_session(X[:F - 1], sess)
            with pytest.raises(ValueError, match="X must be"):
                m.predict_proba_session(torch.zeros((F, D + 1), dtype=torch.float64), sess)
            for bad in (torch.zeros((F, C + 1), dtype=torch.float64), torch.zeros((F + 1, C), dtype=torch.float64),
                        torch.zeros((F, C), dtype=torch.float32), torch.zeros((C, F), dtype=torch.float64).t(),
                        torch.zeros((F, 2 * C), dtype=torch.float64)[:, ::2], torch.zeros(F * C, dtype=torch.float64),
                        np.zeros((F, C))):
                with pytest.raises(ValueError, match="out must be a float64"):
                    m.predict_proba_session(X, sess, out=bad)
            # everything the host can check passes: the refusal left is that there is no CPU path
            with pytest.raises(ValueError, match="HIP device"):
                m.predict_proba_session(X, sess, out=torch.zeros((F, C + 2), dtype=torch.float64)[:, :C])
    with pytest.raises(ValueError, match="without frame_offsets"):
        nb[3].predict_proba_session(X, ce_amd.BatchedSelectionSession(2, "mc", [0, 2, 2, 6], device="cpu"))
    with pytest.raises(ValueError, match="without s_id"):
        sgd[1].predict_proba_session(X, ce_amd.SelectionSession(2, "mc", 6, device="cpu"))


@pytest.mark.parametrize("shuffled", [False, True])
def test_row_owners_matches_pandas_groupby(shuffled):
    pd = pytest.importorskip("pandas")
    import ce_amd

    rng = np.random.default_rng(11 + shuffled)
    users = [5, 0, 9, 3]  # songs per user; user 1 has none
    off = np.concatenate([[0], np.cumsum(users)])
    T = int(off[-1])
    counts = rng.integers(0, 6, T)
    counts[3] = 0  # a song without a frame
    song_of_row = np.repeat(np.arange(T), counts)
    extra = 4  # rows at the end that no song owns
    if shuffled:
        song_of_row = rng.permutation(song_of_row)
    F = len(song_of_row) + extra
    # the CSR over ALL T stacked songs (song_groups drops a song without a frame, a session needs every song)
    f_off = np.concatenate([[0], np.cumsum(np.bincount(song_of_row, minlength=T))])
    f_perm = np.argsort(song_of_row, kind="stable") if shuffled else None
    uniq, so, sp = ce_amd.song_groups(song_of_row)
    assert np.array_equal(np.diff(so), counts[uniq]) and ((sp is None) or np.array_equal(sp, f_perm))
    user, song = row_owners(off, f_off, f_perm, F)
    frame = pd.DataFrame({"song": song_of_row, "row": np.arange(len(song_of_row))})
    frame["user"] = np.searchsorted(off, frame["song"].values, side="right") - 1
    seen = np.zeros(F, bool)
    for (u, g), grp in frame.groupby(["user", "song"]):
        rows = grp["row"].values
        assert (user[rows] == u).all() and (song[rows] == g).all()
        seen[rows] = True
    assert (user[~seen] == -1).all() and (song[~seen] == -1).all() and (~seen).sum() == extra
    assert set(np.unique(user[seen])) == {0, 2, 3}
    # a position whose row lies outside [0, F) names no row; its neighbours keep theirs
    if shuffled:
        bad = f_perm.copy()
        bad[2], bad[7] = F, F + 100
        u2, s2 = row_owners(off, f_off, bad, F)
        lost = np.isin(np.arange(F), f_perm[[2, 7]])
        assert (u2[lost] == -1).all() and np.array_equal(u2[~lost], user[~lost]) and np.array_equal(s2[~lost], song[~lost])


def test_excl_words_layout():
    import ce_amd.ops as ops

    w = excl_words([0, 31, 32, 70], 71)
    assert w.dtype == np.int32 and len(w) == 3 == ops._lib.load().ce_excl_words(71)
    assert w.view(np.uint32).tolist() == [1 | (1 << 31), 1, 1 << 6]


@pytest.mark.parametrize("shuffled", [False, True])
def test_batch_rows_padded_to_a_host_bound(shuffled):
    """batch_rows(max_rows=): what a captured epoch uses -- nothing read back;
    the real rows first, as without the bound, then in-range padding no model owns."""
    torch = pytest.importorskip("torch")
    from ce_amd import ops

    rng = np.random.default_rng(5)
    T = 12
    f_off = np.concatenate([[0], np.cumsum(rng.integers(0, 5, T))])
    n = int(f_off[-1])
    perm = torch.from_numpy(rng.permutation(n)) if shuffled else None
    args = (torch.from_numpy(f_off), perm, torch.from_numpy(rng.integers(0, 4, T)), torch.tensor([0, 5, 5, 12]))
    for songs in ([[0, 3, -1], [-1, -1, -1], [2, 2, 6]], [[-1, -1], [-1, -1], [-1, -1]], [[4], [0], [6]]):
        rows, labels, ro = ops.batch_rows(torch.tensor(songs), *args)
        for bound in (n, n + 7):
            prow, plab, pro = ops.batch_rows(torch.tensor(songs), *args, max_rows=bound)
            R = rows.numel()
            assert pro.tolist() == ro.tolist() and int(ro[-1]) == R and prow.numel() == plab.numel() == bound
            assert prow[:R].tolist() == rows.tolist() and plab[:R].tolist() == labels.tolist()
            assert ((prow >= 0) & (prow < n)).all()
    assert ops.batch_rows(torch.tensor([[1]]), *args[:3], max_rows=0)[0].numel() == 0
