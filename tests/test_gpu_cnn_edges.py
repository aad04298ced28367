"""GPU tests of the short-chunk CNN member at the edges its parity cases
(tests/test_gpu_cnn.py) keep away from: the 1e-10 clamp of the front end (the
empty bands of an HTK bank, digital silence), the shortest and the boundary
lengths, a row pitch above L, an `out=` inside a larger buffer, int16-scale
audio, a NaN sample, and the ownership walk and the exclusion bitmap past word 0.

Tolerance of the front end: the rule of tests/test_gpu_cnn.py,
|dev - f64| <= K e32 + floor_db, e32 the largest |float32 torch.stft pipeline -
float64 DFT product| of the case, floor_db four f32 ulps of the largest |dB|.
A value the clamp decides is exactly -100 in the reference and must be within
floor_db of it.  K by that file's rule: twice the largest ratio |dev - f64| /
e32 measured on an MI355X over these inputs (profiles/cnn_member.json, "parity",
kind "front_end_edge_dB"), rounded up to a power of two, 64 at most.  Measured:
3.118 at most (the HTK bank on 4096 samples; 2.399 at L = 2303, 1.522 at 2048,
the others 1.2 and below), so K_FRONT_EDGE = 8; test_gpu_cnn.py's cases keep
their K = 2.  Why more than there: these inputs run over an HTK bank, whose low
bands hold ONE spectrogram bin each.  Where such a bin is weak by chance the dB
error is the bin's absolute error over a small power, and the device's 512-term
DFT chains (16 partial sums of 32) carry a few times the absolute error of the
reference's float32 FFT of nine stages.  The random bank of the parity cases
spreads every band over several bins and hides it.

A NaN goes through, as torch.clamp, relu, max_pool2d and amax pass it on: the
frames that cover a NaN sample are NaN in every band, that excerpt's four
outputs are NaN, no other excerpt changes by a bit, and np.argmax counts the
excerpt as class 0."""
import numpy as np
import pytest
import torch

import cnn_exact as X
import cnn_ref as R
import members_eval_ref as E

pytestmark = pytest.mark.gpu

K_FRONT_EDGE = 8
SENT = np.float32(-7.25)
L_SMALL = 32768  # T = 129


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


@pytest.fixture(scope="module")
def front(ce):
    """A member over the HTK bank (the front end reads nothing else of the state)."""
    return ce.DeviceShortChunkCNN(X.exact_state(16, seed=0))


def dev(a):
    return (a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))).cuda()


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def check_front(what, got, f64, f32):
    """The ordinary bound over the entries that are finite in the reference; returns floor_db."""
    fin = np.isfinite(f64)
    assert np.array_equal(np.isnan(got), ~fin), (what, np.argwhere(np.isnan(got) != ~fin)[:4])
    floor = R.floor_db(f64[fin])
    r, err, e32 = R.ratio(got[fin], f64[fin], f32[fin])
    print(f"{what}: |dev - f64| = {err:.3e}, e32 = {e32:.3e}, floor = {floor:.3e}, ratio = {r:.3f} (K = {K_FRONT_EDGE})")
    assert e32 > 0
    assert err <= K_FRONT_EDGE * e32 + floor, (what, err, e32, r)
    return floor


# ---- the front end ----------------------------------------------------------------------------------
def test_htk_bank_empty_bands_sit_at_the_clamp(front):
    fb, wave, f64, f32 = X.front_edge("htk")
    empty = np.flatnonzero(fb.numpy().sum(0) == 0)
    assert empty.size >= 1
    got = front.logmel(dev(wave)).cpu().numpy()
    floor = check_front("htk bank", got, f64, f32)
    assert np.all(f64[:, empty] == -100.0)
    assert np.abs(got[:, empty].astype(np.float64) + 100.0).max() <= floor, got[:, empty].ravel()[:8]
    assert got[:, np.setdiff1d(np.arange(128), empty)].min() > -90.0  # every other band is off the clamp


def test_silence_sits_at_the_clamp(front):
    fb, wave, f64, f32 = X.front_edge("silence")
    assert not wave[1].any() and not wave[2, X.SILENT_FROM:].any() and wave[2, :X.SILENT_FROM].all()
    got = front.logmel(dev(wave)).cpu().numpy()
    floor = check_front("silence", got, f64, f32)
    t0 = -(-(X.SILENT_FROM + 256) // 256)  # the first frame whose 512 samples (reflected ones too) are all zero
    assert t0 == 7 and np.all(f64[1] == -100.0) and np.all(f64[2, :, t0:] == -100.0) and f64[2, :, t0 - 1].max() > -60
    assert np.abs(got[1].astype(np.float64) + 100.0).max() <= floor
    assert np.abs(got[2, :, t0:].astype(np.float64) + 100.0).max() <= floor


@pytest.mark.parametrize("L", X.EDGE_LENGTHS)
def test_short_and_boundary_lengths(front, L):
    fb, wave, f64, f32 = X.front_edge(f"L{L}")
    T = L // 256 + 1
    assert f64.shape == (3, 128, T) and T == {512: 3, 513: 3, 767: 3, 768: 4, 1792: 8, 2047: 8, 2048: 9, 2303: 9}[L]
    got = front.logmel(dev(wave))
    assert tuple(got.shape) == (3, 128, T)
    check_front(f"L={L}", got.cpu().numpy(), f64, f32)


def test_large_amplitude(front):
    fb, wave, f64, f32 = X.front_edge("loud")
    assert float(wave.abs().max()) > 8192.0
    check_front("int16-scale audio", front.logmel(dev(wave)).cpu().numpy(), f64, f32)


@pytest.mark.parametrize("L", [2303, 4096])
def test_row_pitch_above_L(front, L):
    """The rows of a wider tensor: a pitch above L and a base pointer 20 bytes off any 16-byte line."""
    wave = R.noise(3, L, seed=5 + L)
    big = torch.full((3, L + 16 + 3), 1.0e30, dtype=torch.float32)
    big[:, 5:5 + L] = wave
    big = big.cuda()
    view = big[:, 5:5 + L]
    assert view.stride(0) == L + 19 and view.stride(1) == 1 and view.data_ptr() % 16 == 4
    want = front.logmel(dev(wave))
    assert np.array_equal(bits(front.logmel(view)), bits(want))
    assert float(want.abs().max()) < 200.0  # no sentinel was read


def test_out_inside_a_larger_buffer(front):
    """T = 9: the second frame tile holds one frame and seven past T; nothing lands outside `out`."""
    L, pad = 2048, 4099
    fb, wave, f64, f32 = X.front_edge(f"L{L}")
    n = 3 * 128 * 9
    flat = torch.full((pad + n + pad,), float(SENT), dtype=torch.float32, device="cuda")
    out = flat[pad:pad + n].view(3, 128, 9)
    assert out.is_contiguous() and front.logmel(dev(wave), out=out) is out
    got = flat.cpu().numpy()
    assert np.all(got[:pad] == SENT) and np.all(got[pad + n:] == SENT)
    assert np.array_equal(bits(got[pad:pad + n].reshape(3, 128, 9)), bits(front.logmel(dev(wave))))
    assert not np.any(got[pad:pad + n] == SENT)


# ---- NaN --------------------------------------------------------------------------------------------
def test_nan_sample_in_the_front_end(front):
    fb, wave, f64, f32 = X.front_edge("nan")
    s, at = X.NAN_AT
    mask = np.zeros(f64.shape, bool)
    mask[s, :, [at // 256, at // 256 + 1]] = True  # frames 2 and 3, every band
    assert np.array_equal(np.isnan(f64), mask)
    got = front.logmel(dev(wave)).cpu().numpy()
    print("NaN entries of the device:", int(np.isnan(got).sum()), "of the reference:", int(mask.sum()),
          "device values where the reference is NaN:", np.unique(got[mask])[:4])
    check_front("one NaN sample", got, f64, f32)  # the masks are equal, the finite entries within the bound


def test_nan_sample_end_to_end(ce):
    state = R.random_state(16, seed=21)
    member = ce.DeviceShortChunkCNN(state)
    clean = R.noise(3, L_SMALL, seed=21)
    wave = clean.clone()
    wave[1, 12345] = float("nan")
    want = member.predict_proba(dev(clean)).cpu().numpy()
    got = member.predict_proba(dev(wave)).cpu().numpy()
    assert np.isfinite(want).all()
    assert np.isnan(got[1]).all(), got[1]
    assert np.array_equal(bits(got[[0, 2]]), bits(want[[0, 2]]))
    y = np.array([2, 3, 1], np.int32)
    _, cm = member.evaluate(dev(wave), dev(y))
    pred = np.argmax(got, axis=1)
    assert pred[1] == 0  # np.argmax takes the first NaN
    assert np.array_equal(cm.cpu().numpy(), E.confusion(y, pred, 4)) and cm[0, 3, 0] == 1


def test_nan_pixel_in_the_body(ce):
    state, mel, _, _ = R.body_case(16, 3, 128)
    member = ce.DeviceShortChunkCNN(state)
    want = member.predict_proba(mel=dev(mel)).cpu().numpy()
    bad = mel.clone()
    bad[1, 77, 50] = float("nan")
    got = member.predict_proba(mel=dev(bad)).cpu().numpy()
    assert np.isnan(got[1]).all(), got[1]
    assert np.isfinite(want).all() and np.array_equal(bits(got[[0, 2]]), bits(want[[0, 2]]))
    with torch.no_grad():
        ref = R.body(bad.double(), state).numpy()
    assert np.array_equal(np.isnan(ref), np.isnan(got))


# ---- ownership and the bitmap -------------------------------------------------------------------------
N_POOL = 70
OFFSETS = np.array([0, 0, 1, 1, 33, 64, 70, 70], np.int64)  # users 0, 2 and 6 own nothing; U = 7 is odd
GONE = np.array([0, 31, 32, 33, 63, 64, 69])  # bit 31 of word 0, both ends of word 1, word 2, the pool's ends


@pytest.fixture(scope="module")
def big_pool(ce):
    """70 excerpts of 7 users, 7 states, the owner of every excerpt and its one-model output."""
    wave = dev(R.noise(N_POOL, L_SMALL, seed=60))
    states = [R.random_state(16, seed=70 + u) for u in range(7)]
    for s in states[1:]:
        s["spec.mel_scale.fb"] = states[0]["spec.mel_scale.fb"]
    owner = np.searchsorted(OFFSETS, np.arange(N_POOL), side="right") - 1
    assert sorted(set(owner)) == [1, 3, 4, 5]
    exp = np.zeros((N_POOL, 4), np.uint32)
    for u in sorted(set(owner)):
        rows = np.flatnonzero(owner == u)
        exp[rows] = bits(ce.DeviceShortChunkCNN(states[u]).predict_proba(wave[int(rows[0]):int(rows[-1]) + 1]))
    member = ce.DeviceShortChunkCNN(states[0], U=7)
    for u in range(1, 7):
        member.set_model(u, states[u])
    return wave, member, owner, exp


def bitmap(n, gone):
    words = np.zeros((n + 31) // 32, np.uint32)
    for s in gone:
        words[s >> 5] |= np.uint32(1) << np.uint32(s & 31)
    return dev(words.view(np.int32))


@pytest.mark.parametrize("batch", [7, 32, 70])
def test_ownership_walk_and_bitmap_words(ce, big_pool, batch):
    wave, member, owner, exp = big_pool
    items, excl = dev(OFFSETS), bitmap(N_POOL, GONE)
    assert excl.numel() == 3 and int(excl[0]) < 0  # three words, bit 31 of the first set
    keep = ~np.isin(np.arange(N_POOL), GONE)
    assert np.array_equal(bits(member.predict_proba_users(wave, items, batch=batch)), exp)
    out = torch.full((N_POOL, 4), float(SENT), dtype=torch.float32, device="cuda")
    assert member.predict_proba_users(wave, items, excl=excl, out=out, batch=batch) is out
    got = out.cpu().numpy()
    assert np.all(got[GONE] == SENT), got[GONE]
    assert np.array_equal(bits(got[keep]), exp[keep]), np.flatnonzero((bits(got) != exp).any(1) & keep)
    # evaluate: the labels of the excerpts that left are outside [0, 4), so cm counts the kept ones
    y = (np.arange(N_POOL) % 4).astype(np.int32)
    pred = np.argmax(exp.view(np.float32), axis=1)
    want = E.confusion(y[keep], pred[keep], 4, user=owner[keep], U=7)
    assert want.sum() == N_POOL - len(GONE) and want[[0, 2, 6]].sum() == 0
    y_kept = np.where(keep, y, -1).astype(np.int32)
    _, cm = member.evaluate(wave, dev(y_kept), items, batch=batch)
    assert np.array_equal(cm.cpu().numpy(), want)
    assert np.array_equal(bits(member.last_proba), exp)
    # the bitmap and the labels in one pass: an excluded excerpt is not counted either
    cm2 = torch.zeros((7, 4, 4), dtype=torch.int64, device="cuda")
    out2 = torch.full((N_POOL, 4), float(SENT), dtype=torch.float32, device="cuda")
    member._users(wave, items, 7, excl, dev(y), cm2, out2, batch)
    assert np.array_equal(cm2.cpu().numpy(), want) and np.array_equal(bits(out2), bits(got))


def test_excerpts_no_user_owns(ce, big_pool):
    """item_offsets [2, 5, 9] over 12 excerpts: rows 0-1 and 9-11 belong to nobody and are not written."""
    wave, member7, _, _ = big_pool
    w12 = wave[:12]
    states = member7.state()
    member = ce.DeviceShortChunkCNN(states[3], U=2).set_model(1, states[4])
    one = [bits(ce.DeviceShortChunkCNN(states[u]).predict_proba(w12)) for u in (3, 4)]
    for batch in (5, 12):
        out = torch.full((12, 4), float(SENT), dtype=torch.float32, device="cuda")
        member.predict_proba_users(w12, dev(np.array([2, 5, 9], np.int64)), out=out, batch=batch)
        got = out.cpu().numpy()
        assert np.all(got[[0, 1, 9, 10, 11]] == SENT), got
        assert np.array_equal(bits(got[2:5]), one[0][2:5]) and np.array_equal(bits(got[5:9]), one[1][5:9])
