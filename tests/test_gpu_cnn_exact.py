"""GPU tests of the short-chunk CNN member block by block, with no tolerance:
on the exact states of tests/cnn_exact.py every activation of every block is a
dyadic rational that float32 holds and every sum is exact in any order, so
DeviceShortChunkCNN.activations (ce_cnn_activations: the forward's own launches,
stopped after a block) must equal the float64 restatement to the bit.  A wrong
tap, channel, halo column, pool window or Cout guard shows as a block number and
pixel indices instead of being pooled away in front of four sigmoids.

The head on the same states: the logits are exact, so what is left is the
sigmoid itself, |dev - sigmoid_f64(logit)| <= FLOOR_P = 2^-22 with no e32 term.

The users form on exact states is bit for bit the per-model calls."""
import numpy as np
import pytest
import torch

import cnn_exact as X
import cnn_ref as R

pytestmark = pytest.mark.gpu

CASES = [(nc, S, T, seed) for nc, S, T in X.EXACT_CASES for seed in X.EXACT_SEEDS]


@pytest.fixture(scope="module")
def ce():
    if not torch.cuda.is_available():
        pytest.skip("no HIP device")
    import ce_amd
    import ce_amd.ops

    ce_amd.load()
    return ce_amd


def bits(a):
    return np.ascontiguousarray(a.cpu().numpy() if isinstance(a, torch.Tensor) else a, np.float32).view(np.uint32)


def mismatches(b, got, want):
    """A report of where block b differs: the count and the first few (s, y, x, c) with both values."""
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    lines = [f"block {b}: {len(bad)} of {got.size} values differ, shape [S, H, W, C] = {list(got.shape)}"]
    for s, y, x, c in bad[:8]:
        lines.append(f"  (s, y, x, c) = ({s}, {y}, {x}, {c}): device {got[s, y, x, c]!r}, reference {want[s, y, x, c]!r}")
    return "\n".join(lines)


@pytest.mark.parametrize("nc,S,T,seed", CASES)
def test_every_block_equals_the_reference_bit_for_bit(ce, nc, S, T, seed):
    state, mel, acts, _ = X.exact_case(nc, S, T, seed)
    member = ce.DeviceShortChunkCNN(state)
    mel_d = mel.cuda()
    report = []
    for b in range(1, 8):
        got = member.activations(mel_d, b)
        want = acts[b - 1].astype(np.float32)
        assert got.dtype == torch.float32 and tuple(got.shape) == want.shape == (S, 128 >> b, T >> b, R.CH[b] * nc)
        got = got.cpu().numpy()
        if not np.array_equal(got.view(np.uint32), want.view(np.uint32)):
            report.append(mismatches(b, got, want))
    if report:
        print("\n".join(report))
    assert not report, "\n".join(report)
    with pytest.raises(ValueError, match="block"):
        member.activations(mel_d, 8)


@pytest.mark.parametrize("nc,S,T,seed", CASES)
def test_head_on_exact_logits(ce, nc, S, T, seed):
    state, mel, _, z = X.exact_case(nc, S, T, seed)
    got = ce.DeviceShortChunkCNN(state).predict_proba(mel=mel.cuda()).cpu().numpy()
    want = 1.0 / (1.0 + np.exp(-z))
    err = float(np.abs(got.astype(np.float64) - want).max())
    print(f"head nc={nc} S={S} T={T} seed={seed}: |dev - f64| = {err:.3e} (floor {R.FLOOR_P:.3e}), "
          f"logits {z.min():.3f} .. {z.max():.3f}")
    assert got.dtype == np.float32 and got.shape == (S, 4) and np.isfinite(got).all()
    assert err <= R.FLOOR_P, (err, np.argwhere(np.abs(got - want) > R.FLOOR_P)[:4])


def test_activations_of_a_user_and_of_a_batch_tail(ce):
    """activations(u=...) reads that user's record; the rows of a larger batch
    are the rows of the one-excerpt calls."""
    nc, S, T = 16, 2, 129
    s0, mel, a0, _ = X.exact_case(nc, S, T, 0)
    s1, _, _, _ = X.exact_case(nc, S, T, 1)
    member = ce.DeviceShortChunkCNN(s0, U=3).set_model(2, s1)
    mel_d = mel.cuda()
    with torch.no_grad():
        a1 = [a.permute(0, 2, 3, 1).numpy().astype(np.float32) for a in R.activations(mel.double(), s1)]
    for b in (1, 4, 7):
        assert np.array_equal(bits(member.activations(mel_d, b, u=1)), a0[b - 1].astype(np.float32).view(np.uint32))
        assert np.array_equal(bits(member.activations(mel_d, b, u=2)), a1[b - 1].view(np.uint32))
        assert np.array_equal(bits(member.activations(mel_d[1:], b, u=2)), a1[b - 1][1:].view(np.uint32))
    with pytest.raises(ValueError, match="outside"):
        member.activations(mel_d, 1, u=3)


def test_users_form_on_exact_states(ce):
    """predict_proba_users with one exact state per user equals the per-model calls bit for bit."""
    offsets = np.array([0, 2, 2, 5, 6], np.int64)
    states = [X.exact_state(16, seed=s) for s in range(4)]
    wave = R.noise(6, 32768, seed=77).cuda()
    one = [bits(ce.DeviceShortChunkCNN(s).predict_proba(wave)) for s in states]
    assert len({o.tobytes() for o in one}) == 4
    owner = np.searchsorted(offsets, np.arange(6), side="right") - 1
    exp = np.stack([one[owner[s]][s] for s in range(6)])
    member = ce.DeviceShortChunkCNN(states[0], U=4)
    for u in range(1, 4):
        member.set_model(u, states[u])
    items = torch.from_numpy(offsets).cuda()
    for batch in (1, 4, 6):
        assert np.array_equal(bits(member.predict_proba_users(wave, items, batch=batch)), exp), batch
