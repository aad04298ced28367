"""GPU tests of the short-chunk CNN member (ce_amd.DeviceShortChunkCNN over
ce_cnn_logmel / ce_cnn_forward_users) against tests/cnn_ref.py.

Tolerance.  e32 is the largest |float32 - float64| of the restatement on the
CPU for the case, computed here; the device must satisfy
|dev - f64| <= K e32 + floor (floor: 2^-22 for a probability, four f32 ulps of
the largest |dB| for the front end).  K is twice the largest ratio
|dev - f64| / e32 measured on the first MI355X run (profiles/cnn_member.json,
"parity"), rounded up to a power of two; only K <= 64 is acceptable.  Measured:
the probabilities (body and end to end) 4.254 at most (nc = 128, K = 2304 terms
in the longest chain; nc = 48, the partial Cout tiles: 2.809), so K = 16.  The
front end 0.87, so K = 2 (the edge inputs of tests/test_gpu_cnn_edges.py have a
K of their own, derived there by the same rule).

The users form, the exclusion and set_model are checked bit for bit against
the one-model call."""
import numpy as np
import pytest
import torch

import cnn_ref as R
import members_eval_ref as E

pytestmark = pytest.mark.gpu

K_BODY = K_E2E = 16
K_FRONT = 2
SENT = np.float32(-7.25)
OFFSETS = np.array([0, 3, 3, 5, 9], np.int64)  # four users, one of them without an excerpt
L_SMALL = 32768  # T = 129: 64, 32, 16, 8, 4, 2, 1


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def check(what, got, f64, f32, floor, k):
    r, err, e32 = R.ratio(got, f64, f32)
    print(f"{what}: |dev - f64| = {err:.3e}, e32 = {e32:.3e}, floor = {floor:.3e}, ratio = {r:.3f} (K = {k})")
    assert e32 > 0 and np.isfinite(got).all()
    assert err <= k * e32 + floor, (what, err, e32, r)


# ---- 1. the network body from a given log-mel ---------------------------------------------------
@pytest.mark.parametrize("nc,S,T", R.BODY_CASES)
def test_body_from_logmel(ce, nc, S, T):
    state, mel, f64, f32 = R.body_case(nc, S, T)
    member = ce.DeviceShortChunkCNN(state)
    assert member.nc == nc and member.Uw == 1
    got = member.predict_proba(mel=dev(mel))
    assert got.dtype == torch.float32 and tuple(got.shape) == (S, 4)
    check(f"body nc={nc} S={S} T={T}", got.cpu().numpy(), f64, f32, R.FLOOR_P, K_BODY)


# ---- 2. the front end ----------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.FRONT_CASES)
def test_front_end(ce, L):
    state, wave, f64, f32 = R.front_case(L)
    got = ce.DeviceShortChunkCNN(state).logmel(dev(wave))
    assert tuple(got.shape) == (3, 128, L // 256 + 1)
    check(f"front end L={L}", got.cpu().numpy(), f64, f32, R.floor_db(f64), K_FRONT)


# ---- 3. end to end from the waveform -------------------------------------------------------------
def test_end_to_end_from_the_waveform(ce):
    state, wave, f64, f32 = R.e2e_case(*R.E2E_CASE)
    got = ce.DeviceShortChunkCNN(state).predict_proba(dev(wave))
    check("end to end", got.cpu().numpy(), f64, f32, R.FLOOR_P, K_E2E)


# ---- 4.-6. users form, exclusion, set_model ------------------------------------------------------
@pytest.fixture(scope="module")
def pool(ce):
    """Nine excerpts of four users, four states, and every state's one-model outputs over all nine."""
    wave = dev(R.noise(9, L_SMALL, seed=40))
    states = [R.random_state(16, seed=50 + u) for u in range(4)]
    for s in states[1:]:
        s["spec.mel_scale.fb"] = states[0]["spec.mel_scale.fb"]  # one front end
    one = [bits(ce.DeviceShortChunkCNN(s).predict_proba(wave)) for s in states]
    owner = np.searchsorted(OFFSETS, np.arange(9), side="right") - 1
    assert len({o.tobytes() for o in one}) == 4  # the models differ
    return wave, states, one, owner


def own_models(ce, states):
    m = ce.DeviceShortChunkCNN(states[0], U=4)
    for u in range(1, 4):
        m.set_model(u, states[u])
    assert m.Uw == 4
    return m


def test_users_form(ce, pool):
    wave, states, one, owner = pool
    items = dev(OFFSETS)
    own = own_models(ce, states)
    exp = np.stack([one[owner[s]][s] for s in range(9)])
    for batch in (2, 9):
        assert np.array_equal(bits(own.predict_proba_users(wave, items, batch=batch)), exp), batch
    for u in (0, 2, 3):  # predict_proba(..., u) of the member itself, on its own rows
        rows = np.flatnonzero(owner == u)
        assert np.array_equal(bits(own.predict_proba(wave[int(rows[0]):int(rows[-1]) + 1], u=u)), exp[rows])
    shared = ce.DeviceShortChunkCNN(states[1], U=4)
    assert shared.Uw == 1
    for batch in (2, 9):
        assert np.array_equal(bits(shared.predict_proba_users(wave, items, batch=batch)), one[1]), batch
    with pytest.raises(ValueError, match=r"3 user\(s\)"):
        own.predict_proba_users(wave, items[:4])


def test_exclusion(ce, pool):
    wave, states, one, owner = pool
    gone = np.array([1, 4, 7])  # one excerpt of every user who has any
    excl = ce.ops.excl_bitmap(9, "cuda")
    ce.ops.mark_selected(excl, 9, dev(gone))
    exp = np.stack([one[owner[s]][s] for s in range(9)])
    keep = ~np.isin(np.arange(9), gone)
    for member in (own_models(ce, states), ce.DeviceShortChunkCNN(states[0], U=4)):
        full = bits(member.predict_proba_users(wave, dev(OFFSETS)))
        for batch in (2, 32):
            out = torch.full((9, 4), float(SENT), dtype=torch.float32, device="cuda")
            assert member.predict_proba_users(wave, dev(OFFSETS), excl=excl, out=out, batch=batch) is out
            got = out.cpu().numpy()
            assert np.all(got[gone] == SENT) and np.array_equal(bits(got[keep]), full[keep])
        new = member.predict_proba_users(wave, dev(OFFSETS), excl=excl).cpu().numpy()
        assert np.all(new[gone] == 0) and np.array_equal(bits(new[keep]), full[keep])
    assert np.array_equal(bits(own_models(ce, states).predict_proba_users(wave, dev(OFFSETS))), exp)


def test_set_model(ce, pool):
    wave, states, one, owner = pool
    member = ce.DeviceShortChunkCNN(states[0], U=4)
    before = bits(member.predict_proba_users(wave, dev(OFFSETS)))
    assert np.array_equal(before, one[0])
    assert member.set_model(2, states[3]) is member and member.Uw == 4
    after = bits(member.predict_proba_users(wave, dev(OFFSETS)))
    assert np.array_equal(after[owner == 2], one[3][owner == 2])
    assert np.array_equal(after[owner != 2], before[owner != 2])
    st = member.state()
    assert len(st) == 4 and np.array_equal(st[2]["dense1.bias"], states[3]["dense1.bias"].numpy())
    assert np.array_equal(st[1]["dense1.bias"], states[0]["dense1.bias"].numpy())
    with pytest.raises(ValueError, match="outside"):
        member.set_model(4, states[1])
    with pytest.raises(ValueError, match=r"nc = 32"):
        member.set_model(1, R.random_state(32, seed=1))
    with pytest.raises(ValueError, match=r"spec\.mel_scale\.fb"):
        member.set_model(1, R.random_state(16, seed=99))


# ---- 7. evaluate ---------------------------------------------------------------------------------
def test_evaluate(ce, pool):
    """User 0's model ties outputs 1 and 2 at the maximum or 0 and 3 (np.argmax:
    the first), user 2's puts a NaN in output 2 (np.argmax: the NaN), both
    through the dense2 weights."""
    wave, states, _, owner = pool
    tie = dict(states[0])
    w, b = tie["dense2.weight"].clone(), tie["dense2.bias"].clone()
    w[2], b[2], w[0], b[0], w[3], b[3] = w[1], b[1], -w[1], -b[1], -w[1], -b[1]
    tie["dense2.weight"], tie["dense2.bias"] = w, b
    nan = dict(states[2])
    w = nan["dense2.weight"].clone()
    w[2, 5] = float("nan")
    nan["dense2.weight"] = w
    member = ce.DeviceShortChunkCNN(states[1], U=4).set_model(0, tie).set_model(2, nan)
    y = np.array([1, 0, 2, 2, 3, 3, 1, -1, 0], np.int32)  # one label outside [0, 4): not counted
    f1, cm, prf = member.evaluate(wave, dev(y), dev(OFFSETS), report=True)
    p = member.last_proba.cpu().numpy()
    assert np.array_equal(bits(p), bits(member.predict_proba_users(wave, dev(OFFSETS))))
    assert np.all((p[owner == 0, 1] == p[owner == 0, 2]) & (p[owner == 0, 0] == p[owner == 0, 3]))
    assert np.isnan(p[owner == 2, 2]).all() and not np.isnan(p[owner != 2]).any()
    pred = np.argmax(p, axis=1)
    assert set(pred[owner == 0]) <= {0, 1} and np.all(pred[owner == 2] == 2)
    exp = E.confusion(y, pred, 4, user=owner, U=4)
    assert cm.dtype == torch.int64 and np.array_equal(cm.cpu().numpy(), exp) and exp.sum() == 8
    want = np.array([E.f1_weighted(exp[u]) for u in range(4)])
    assert np.array_equal(f1.cpu().numpy().view(np.uint64), want.view(np.uint64))  # user 1: NaN, no excerpt
    assert np.array_equal(prf.cpu().numpy(), np.stack([E.prf(exp[u]) for u in range(4)]))
    f1b, cmb = member.evaluate(wave, dev(y), dev(OFFSETS), batch=2)
    assert np.array_equal(cmb.cpu().numpy(), exp)
    one = ce.DeviceShortChunkCNN(states[1])  # item_offsets=None: one user owning all
    _, cm1 = one.evaluate(wave, dev(y))
    assert np.array_equal(cm1.cpu().numpy(), E.confusion(y, np.argmax(one.last_proba.cpu().numpy(), 1), 4))


# ---- 8. a song-level member of a session ----------------------------------------------------------
def test_song_level_member_of_a_batched_session(ce, pool):
    from oracle import ce_oracle as O

    wave, states, _, owner = pool
    rng = np.random.default_rng(8)
    counts = rng.integers(3, 9, 9)
    s_id = np.repeat(np.arange(9), counts)
    f_off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    D, q = 12, 2
    X = rng.normal(size=(len(s_id), D))
    nb = ce.DeviceGaussianNB(rng.normal(size=(4, 4, D)), rng.uniform(0.5, 2.0, (4, 4, D)), rng.integers(5, 50, (4, 4)))
    sess = ce.BatchedSelectionSession(q, "mc", OFFSETS, frame_offsets=f_off)
    member = own_models(ce, states)
    gnb_frames = nb.predict_proba_session(dev(X), sess)
    cnn_songs = member.predict_proba_session(wave, sess)
    assert tuple(cnn_songs.shape) == (9, 4) and cnn_songs.dtype == torch.float32
    idx = sess.step(frames=[gnb_frames, cnn_songs])
    picks = sess.account(idx)
    P = np.stack([O.ref_group_mean(gnb_frames.cpu().numpy(), s_id)[0], cnn_songs.cpu().numpy().astype(np.float64)])
    for u in range(4):
        lo, hi = OFFSETS[u], OFFSETS[u + 1]
        exp = O.oracle_select_mc(np.ascontiguousarray(P[:, lo:hi]), q, "MNC")[1] if hi > lo else np.zeros(0, np.int64)
        assert np.array_equal(picks[u], exp[exp >= 0]), u
    # the next epoch's predict skips the picked songs
    out = torch.full((9, 4), float(SENT), dtype=torch.float32, device="cuda")
    member.predict_proba_session(wave, sess, out=out)
    picked = np.concatenate([np.asarray(p) + OFFSETS[u] for u, p in enumerate(picks)]).astype(np.int64)
    got = out.cpu().numpy()
    assert picked.size == 6 and np.all(got[picked] == SENT)
    keep = ~np.isin(np.arange(9), picked)
    assert np.array_equal(bits(got[keep]), bits(cnn_songs)[keep])
    with pytest.raises(ValueError, match="9 songs"):
        member.predict_proba_session(wave[:5], sess)


def test_one_user_over_a_selection_session(ce, pool):
    """A SelectionSession: one model owning every song; its bitmap skips the picked songs."""
    wave, states, one, _ = pool
    member = ce.DeviceShortChunkCNN(states[2])
    sess = ce.SelectionSession(2, "mc", n_items=9)
    assert np.array_equal(bits(member.predict_proba_session(wave, sess)), one[2])
    gone = np.array([0, 8])
    ce.ops.mark_selected(sess.excl, 9, dev(gone))
    out = torch.full((9, 4), float(SENT), dtype=torch.float32, device="cuda")
    got = member.predict_proba_session(wave, sess, out=out, batch=4).cpu().numpy()
    keep = ~np.isin(np.arange(9), gone)
    assert np.all(got[gone] == SENT) and np.array_equal(bits(got[keep]), one[2][keep])
    assert np.array_equal(bits(member.predict_proba_session(wave, sess, skip_excluded=False)), one[2])
    with pytest.raises(ValueError, match=r"1 user\(s\)"):
        ce.DeviceShortChunkCNN(states[2], U=4).predict_proba_session(wave, sess)
    # a row pitch below L (an expanded view) is refused, not read past its storage
    with pytest.raises(ValueError):
        member.logmel(wave[:1].expand(3, -1))
