"""States and inputs on which the short-chunk CNN is exact in float32, and the
edge inputs of its front end: helpers of tests/test_cnn.py,
tests/test_gpu_cnn_exact.py and tests/test_gpu_cnn_edges.py.

exact_state(nc, seed): a state dict under the reference's key names in which
every value at every block is a dyadic rational and every sum is exact in
float32 whatever the order of its terms, so float32, float64 and the device
agree to the bit and the device is compared with no tolerance at all:

  every BatchNorm   running_var = 1 - 1e-5 and running_mean = 0: the folded
                    scale is the weight itself (1 / sqrt(var + eps) rounds to 1)
  spec_bn           weight 0.5, bias 0.25
  other BatchNorms  weight per channel from {1, -1, 0.5}, bias from
                    {0, 0.25, -0.5}: a negative scale tells a ReLU before the
                    normalisation, or a pool before the ReLU, from the right order
  conv              3 non-zero weights per output channel, +-1, at seeded random
                    (ci, ky, kx); bias from {0, 0.5, -0.25}
  dense1, dense2    3 non-zero +-1 entries per row; bias from {0, 0.5, -0.25}
  exact_mel         randint(-16, 17) / 4

A value after block b is a multiple of 2^-(3 + b) below 2^6 (measured: 62 at
most), 16 significant bits at most, and a sum of three of them stays far inside
float32's 24.  tests/test_cnn.py asserts that float32 equals float64 at every
block of every case below, and that the activations are neither sparse nor few
in values, so the comparison cannot go blind.

htk_bank(): the triangular HTK mel bank the real model carries (16 kHz, 257
bins, 128 bands, no normalisation).  Below about 500 Hz its triangles are
narrower than one 31.25 Hz bin, so some bands hold no bin at all: their power is
0 and the 1e-10 clamp of the front end decides their value.
"""
import numpy as np
import torch

import cnn_ref as R

# (nc, S, T) of the per-block comparison, each with the seeds below.  Widths the
# conv kernel meets (its tile is 8 x 16 pixels): T = 128 -> 64, 32, 16 (one full
# tile), 8, 4, 2; 129 the same after an odd first width; 231 -> 115, 57, 28, 14,
# 7, 3; 300 -> 150, 75, 37, 18 (2 columns into a second tile), 9, 4 and a last
# width of 2; 150 -> 75, 37, 18, 9, 4, 2.  H falls 64 .. 2: below the 8-row tile
# from block 5 on.  nc = 32: exact-fit Cout tiles (32, 64, 128); nc = 48: partial
# ones in every instantiation (48 = 32 + 16, 96 = 64 + 32, 192 = 128 + 64).
EXACT_CASES = [(16, 2, 128), (16, 2, 129), (16, 2, 231), (16, 2, 300), (32, 1, 150), (48, 2, 231)]
EXACT_SEEDS = (0, 1)

BN_W, BN_B, BIAS = (1.0, -1.0, 0.5), (0.0, 0.25, -0.5), (0.0, 0.5, -0.25)


def htk_bank():
    """[257, 128] float64: triangles over 130 points equally spaced in
    mel = 2595 log10(1 + f / 700) from 0 to 8000 Hz."""
    freqs = np.linspace(0.0, 8000.0, R.N_BINS)
    pts = np.linspace(0.0, 2595.0 * np.log10(1.0 + 8000.0 / 700.0), R.N_MELS + 2)
    f_pts = 700.0 * (10.0 ** (pts / 2595.0) - 1.0)
    slopes = f_pts[None, :] - freqs[:, None]  # [257, 130]
    down = -slopes[:, :-2] / np.diff(f_pts)[:-1]
    up = slopes[:, 2:] / np.diff(f_pts)[1:]
    return np.maximum(0.0, np.minimum(down, up))


def _sparse(rng, rows, cols):
    """[rows, cols] with exactly three non-zero entries, +-1, per row."""
    w = np.zeros((rows, cols))
    for r in range(rows):
        w[r, rng.choice(cols, 3, replace=False)] = rng.choice([-1.0, 1.0], 3)
    return w


def exact_state(nc=16, seed=0):
    rng = np.random.default_rng(7000 + 31 * nc + seed)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))  # noqa: E731
    s = {"spec.mel_scale.fb": t(htk_bank())}
    for prefix, c in R.bn_names(nc):
        spec = prefix == "spec_bn"
        s[f"{prefix}.weight"] = t([0.5] if spec else rng.choice(BN_W, c))
        s[f"{prefix}.bias"] = t([0.25] if spec else rng.choice(BN_B, c))
        s[f"{prefix}.running_mean"] = t(np.zeros(c))
        s[f"{prefix}.running_var"] = t(np.full(c, 1.0 - R.EPS))
    for i in range(1, 8):
        cin, cout = (1 if i == 1 else R.CH[i - 1] * nc), R.CH[i] * nc
        s[f"layer{i}.conv.weight"] = t(_sparse(rng, cout, cin * 9).reshape(cout, cin, 3, 3))
        s[f"layer{i}.conv.bias"] = t(rng.choice(BIAS, cout))
    d = 4 * nc
    s["dense1.weight"], s["dense1.bias"] = t(_sparse(rng, d, d)), t(rng.choice(BIAS, d))
    s["dense2.weight"], s["dense2.bias"] = t(_sparse(rng, R.N_CLASS, d)), t(rng.choice(BIAS, R.N_CLASS))
    return s


def exact_mel(S, T, seed=0):
    g = torch.Generator().manual_seed(3000 + seed)
    return (torch.randint(-16, 17, (S, R.N_MELS, T), generator=g).double() / 4.0).float()


_cache = {}


def exact_case(nc, S, T, seed):
    """(state, mel f32, the seven blocks' outputs in float64 as [S, H, W, C]
    arrays, the logits [S, 4] in float64), computed once per process."""
    key = (nc, S, T, seed)
    if key not in _cache:
        state, mel = exact_state(nc, seed), exact_mel(S, T, seed=T + seed)
        with torch.no_grad():
            acts = R.activations(mel.double(), state)
            z = R.logits(acts[-1], state).numpy()
        _cache[key] = (state, mel, [a.permute(0, 2, 3, 1).contiguous().numpy() for a in acts], z)
    return _cache[key]


# ---- the front end's edge inputs (tests/test_gpu_cnn_edges.py and tools/cnn_member_probe.py share them)
EDGE_LENGTHS = [512, 513, 767, 768, 1792, 2047, 2048, 2303]  # T = 3, 3, 3, 4, 8, 8, 9, 9
L_EDGE = 4096  # T = 17: three frame tiles, the last with one frame
SILENT_FROM = 1500  # excerpt 2 of "silence" is zero from here on: frames t >= 7 see zeros only
NAN_AT = (2, 700)  # the "nan" case: one NaN sample, in frames 2 and 3 of excerpt 2
FRONT_EDGES = ["htk", "silence", "loud", "nan"] + [f"L{n}" for n in EDGE_LENGTHS]


def front_edge(name):
    """(fb [257, 128] f64, wave [3, L] f32, dB by the float64 DFT product, dB by
    a float32 torch.stft pipeline) of a named edge case, all over the HTK bank."""
    key = ("edge", name)
    if key not in _cache:
        fb = torch.from_numpy(htk_bank())
        if name.startswith("L"):
            wave = R.noise(3, int(name[1:]), seed=int(name[1:]))
        else:
            wave = R.noise(3, 2048 if name == "nan" else L_EDGE, seed=len(name))
            if name == "silence":
                wave[1] = 0.0
                wave[2, SILENT_FROM:] = 0.0
            elif name == "loud":
                wave = wave * 32768.0  # un-normalised int16-scale audio
            elif name == "nan":
                wave[NAN_AT] = float("nan")
        _cache[key] = (fb, wave, R.logmel(wave.double(), fb).numpy(), R.logmel_stft(wave, fb).numpy())
    return _cache[key]
