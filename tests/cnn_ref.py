"""The short-chunk CNN in eval mode, restated from torch.nn.functional calls:
what the device member (ce_amd.DeviceShortChunkCNN) is tested against, runnable
in float64 and in float32 on the CPU.

  random_state(nc, seed)   a state dict of seeded random tensors (float64) under
                           the reference's key names: BatchNorm running variances
                           in [0.5, 2], means in [-0.5, 0.5], so activations stay
                           alive through seven blocks
  noise(S, L, seed)        Gaussian noise of amplitude 0.1 (no spectrogram bin at
                           the 1e-10 clamp)
  logmel(wave, fb)         the front end from an explicit windowed DFT product
  logmel_stft(wave, fb)    the same through torch.stft
  activations(mel, state)  spec_bn and the seven blocks: every block's output
  body(mel, state)         the blocks and the head: [S, 4]
  forward(wave, state)     both
  ratio(dev, f64, f32)     what the tests bound: max |dev - f64| / e32, e32 = max |f32 - f64|

tests/test_cnn.py pins body() to torch.nn modules and logmel() to torch.stft.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

N_FFT, HOP, N_BINS, N_MELS, N_CLASS = 512, 256, 257, 128, 4
EPS = 1e-5
CH = (0, 1, 1, 2, 2, 2, 2, 4)
BN_KEYS = ("weight", "bias", "running_mean", "running_var")


def bn_names(nc):
    """(prefix, channels) of every BatchNorm of the network."""
    return [("spec_bn", 1)] + [(f"layer{i}.bn", CH[i] * nc) for i in range(1, 8)] + [("bn", 4 * nc)]


def random_state(nc=16, seed=0, with_extras=True):
    g = torch.Generator().manual_seed(seed)

    def rnd(*shape, lo=-1.0, hi=1.0):
        return lo + (hi - lo) * torch.rand(*shape, generator=g, dtype=torch.float64)

    s = {}
    # a non-negative bank with a few bins per band, as a mel bank is (the values are random: the bank is a weight)
    fb = rnd(N_BINS, N_MELS, lo=0.0, hi=1.0)
    centre = torch.linspace(1, N_BINS - 2, N_MELS)[None, :]
    width = 2.0 + 6.0 * torch.arange(N_MELS)[None, :] / N_MELS
    fb = fb * (((torch.arange(N_BINS)[:, None] - centre).abs() <= width).double()) * 0.05
    s["spec.mel_scale.fb"] = fb
    for prefix, c in bn_names(nc):
        s[f"{prefix}.weight"] = rnd(c, lo=0.5, hi=1.5)
        s[f"{prefix}.bias"] = rnd(c, lo=-0.2, hi=0.2)
        s[f"{prefix}.running_mean"] = rnd(c, lo=-0.5, hi=0.5)
        s[f"{prefix}.running_var"] = rnd(c, lo=0.5, hi=2.0)
        if with_extras:
            s[f"{prefix}.num_batches_tracked"] = torch.tensor(7)
    for i in range(1, 8):
        cin, cout = (1 if i == 1 else CH[i - 1] * nc), CH[i] * nc
        a = math.sqrt(6.0 / (9 * cin))  # keeps the variance of the activations from block to block
        s[f"layer{i}.conv.weight"] = rnd(cout, cin, 3, 3, lo=-a, hi=a)
        s[f"layer{i}.conv.bias"] = rnd(cout, lo=-0.1, hi=0.1)
    d = 4 * nc
    a = 0.25 * math.sqrt(3.0 / d)  # outputs away from the sigmoid's flat ends
    s["dense1.weight"], s["dense1.bias"] = rnd(d, d, lo=-a, hi=a), rnd(d, lo=-0.1, hi=0.1)
    s["dense2.weight"], s["dense2.bias"] = rnd(N_CLASS, d, lo=-a, hi=a), rnd(N_CLASS, lo=-0.1, hi=0.1)
    if with_extras:
        s["spec.spectrogram.window"] = torch.hann_window(N_FFT, periodic=True, dtype=torch.float64)
    return s


def cast(state, dtype):
    return {k: (v.to(dtype) if v.is_floating_point() else v) for k, v in state.items()}


def noise(S, L, seed=0):
    g = torch.Generator().manual_seed(1000 + seed)
    return (0.1 * torch.randn(S, L, generator=g, dtype=torch.float64)).float()


def random_mel(S, T, seed=0):
    """A log-mel as the front end makes of the noise: dB values of a few units around 0."""
    g = torch.Generator().manual_seed(2000 + seed)
    return (5.0 * torch.randn(S, N_MELS, T, generator=g, dtype=torch.float64)).float()


def frames_of(wave):
    """[S, T, 512]: the centred, reflect-padded frames."""
    x = F.pad(wave[:, None, :], (N_FFT // 2, N_FFT // 2), mode="reflect")[:, 0, :]
    return x.unfold(1, N_FFT, HOP)


def logmel(wave, fb):
    """wave [S, L], fb [257, 128] -> dB [S, 128, T], in wave's dtype."""
    dt = wave.dtype
    n = torch.arange(N_FFT, dtype=torch.float64, device=wave.device)
    win = 0.5 - 0.5 * torch.cos(2.0 * math.pi * n / N_FFT)
    ang = 2.0 * math.pi * n[:, None] * torch.arange(N_BINS, dtype=torch.float64, device=wave.device)[None, :] / N_FFT
    fr = frames_of(wave)
    re = fr @ (win[:, None] * torch.cos(ang)).to(dt)
    im = fr @ (win[:, None] * torch.sin(ang)).to(dt)
    mel = (re * re + im * im) @ fb.to(dt)
    return (10.0 * torch.log10(torch.clamp(mel, min=1e-10))).transpose(1, 2).contiguous()


def logmel_stft(wave, fb):
    dt = wave.dtype
    win = torch.hann_window(N_FFT, periodic=True, dtype=dt, device=wave.device)
    sp = torch.stft(wave, N_FFT, hop_length=HOP, win_length=N_FFT, window=win, center=True, pad_mode="reflect",
                    normalized=False, onesided=True, return_complex=True)
    power = sp.real * sp.real + sp.imag * sp.imag  # [S, 257, T]
    mel = power.transpose(1, 2) @ fb.to(dt)
    return (10.0 * torch.log10(torch.clamp(mel, min=1e-10))).transpose(1, 2).contiguous()


def _bn(x, s, prefix):
    return F.batch_norm(x, s[f"{prefix}.running_mean"], s[f"{prefix}.running_var"], s[f"{prefix}.weight"],
                        s[f"{prefix}.bias"], training=False, eps=EPS)


def activations(mel, state):
    """mel [S, 128, T] -> what each of the seven blocks writes (after the pool):
    a list of [S, C_b, 128 >> b, T >> b], in mel's dtype."""
    s = cast(state, mel.dtype)
    x = _bn(mel[:, None], s, "spec_bn")
    acts = []
    for i in range(1, 8):
        x = F.conv2d(x, s[f"layer{i}.conv.weight"], s[f"layer{i}.conv.bias"], stride=1, padding=1)
        x = F.max_pool2d(F.relu(_bn(x, s, f"layer{i}.bn")), 2)
        acts.append(x)
    return acts


def logits(feat, state):
    """The last block's output [S, 4nc, 1, Wf] -> dense2's outputs [S, 4], before the sigmoid."""
    s = cast(state, feat.dtype)
    assert feat.shape[2] == 1
    x = feat[:, :, 0, :].amax(dim=2)
    x = F.relu(_bn(F.linear(x, s["dense1.weight"], s["dense1.bias"]), s, "bn"))
    return F.linear(x, s["dense2.weight"], s["dense2.bias"])


def body(mel, state):
    """mel [S, 128, T] -> [S, 4], in mel's dtype."""
    return torch.sigmoid(logits(activations(mel, state)[-1], state))


def forward(wave, state):
    return body(logmel(wave, state["spec.mel_scale.fb"]), state)


def widths(T):
    w = [T]
    for _ in range(7):
        w.append(w[-1] // 2)
    return w


def ratio(dev, f64, f32):
    """(|dev - f64| / e32, |dev - f64|, e32): the largest absolute differences over the case, e32 = |f32 - f64|."""
    f64 = np.asarray(f64, np.float64)
    e32 = float(np.abs(np.asarray(f32, np.float64) - f64).max())
    err = float(np.abs(np.asarray(dev, np.float64) - f64).max())
    return err / e32, err, e32


# ---- the cases the GPU tests and tools/cnn_member_probe.py share (computed once per process)
# (nc, S, T); nc = 48 is the one with partial Cout tiles in every k_cnn_conv instantiation (48, 96, 192)
BODY_CASES = [(16, 3, 128), (16, 3, 231), (16, 3, 255), (16, 3, 300), (128, 2, 231), (48, 2, 150)]
FRONT_CASES = [32768, 59049]  # L, with S = 3
E2E_CASE = (16, 3, 59049)  # (nc, S, L)
FLOOR_P = 2.0 ** -22  # about four f32 ulps of a probability

_cache = {}


def body_case(nc, S, T):
    """(state, mel f32, outputs in float64, outputs in float32)."""
    key = ("body", nc, S, T)
    if key not in _cache:
        state, mel = random_state(nc, seed=nc + T), random_mel(S, T, seed=T)
        with torch.no_grad():
            _cache[key] = (state, mel, body(mel.double(), state).numpy(), body(mel, state).numpy())
    return _cache[key]


def front_case(L, S=3):
    """(state, wave f32, dB by the float64 DFT product, dB by a float32 torch.stft pipeline)."""
    key = ("front", L, S)
    if key not in _cache:
        state, wave = random_state(16, seed=7), noise(S, L, seed=L)
        fb = state["spec.mel_scale.fb"]
        _cache[key] = (state, wave, logmel(wave.double(), fb).numpy(), logmel_stft(wave, fb).numpy())
    return _cache[key]


def e2e_case(nc, S, L):
    """(state, wave f32, outputs in float64, outputs in float32)."""
    key = ("e2e", nc, S, L)
    if key not in _cache:
        state, wave = random_state(nc, seed=11), noise(S, L, seed=11)
        with torch.no_grad():
            _cache[key] = (state, wave, forward(wave.double(), state).numpy(), forward(wave, state).numpy())
    return _cache[key]


def floor_db(f64):
    """Four f32 ulps at the largest |dB| of the case."""
    return 4.0 * float(np.spacing(np.float32(np.abs(f64).max())))
