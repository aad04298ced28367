"""CPU checks of the short-chunk CNN member: the restatement the GPU tests
compare against (tests/cnn_ref.py) is pinned to torch.nn modules and to
torch.stft, the state-dict intake is checked, and the C-ABI's argument errors
come back without a device."""
import ctypes
from collections import OrderedDict

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import cnn_exact as X  # noqa: E402
import cnn_ref as R  # noqa: E402


def module_net(nc):
    """The network body as torch.nn modules in a ModuleDict keyed by the state
    dict's names (what load_state_dict matches on); a block is a Sequential of
    conv, bn, ReLU and the 2 x 2 pool."""
    nn = torch.nn
    mods = {"spec_bn": nn.BatchNorm2d(1)}
    for i in range(1, 8):
        cin, cout = (1 if i == 1 else R.CH[i - 1] * nc), R.CH[i] * nc
        mods[f"layer{i}"] = nn.Sequential(OrderedDict(conv=nn.Conv2d(cin, cout, 3, padding=1), bn=nn.BatchNorm2d(cout),
                                                      act=nn.ReLU(), pool=nn.MaxPool2d(2)))
    d = 4 * nc
    mods.update(dense1=nn.Linear(d, d), bn=nn.BatchNorm1d(d), dense2=nn.Linear(d, R.N_CLASS))
    return nn.ModuleDict(mods)


def run_modules(net, mel):
    x = net["spec_bn"](mel[:, None])
    for i in range(1, 8):
        x = net[f"layer{i}"](x)
    feat = x[:, :, 0, :].amax(-1)  # the height is 1: the maximum over the width left
    hidden = torch.relu(net["bn"](net["dense1"](feat)))
    return torch.sigmoid(net["dense2"](hidden))


@pytest.mark.parametrize("T", [128, 231, 255, 300])
def test_restatement_equals_torch_nn_modules(T):
    """float64, eval mode, to 1e-12: floor pooling at odd sizes (231, 255), a
    final width of 2 (300) and the BatchNorm arithmetic."""
    nc = 16
    state = R.random_state(nc, seed=T)
    net = module_net(nc).double()
    net.load_state_dict({k: v for k, v in state.items() if not k.startswith("spec.")})
    net.eval()
    mel = R.random_mel(2, T, seed=T).double()
    with torch.no_grad():
        want = run_modules(net, mel)
    got = R.body(mel, state)
    assert got.shape == (2, R.N_CLASS)
    assert float((got - want).abs().max()) <= 1e-12
    assert R.widths(T)[-1] == (2 if T == 300 else 1)


def test_folded_batchnorm_equals_the_restatement():
    """The double scale / shift the member packs (conv bias and running
    statistics folded) reproduce the restatement's blocks in float64."""
    import torch.nn.functional as F

    from ce_amd import cnn

    nc, T = 16, 131
    state = R.random_state(nc, seed=5)
    _, s = cnn.read_state(state)
    mel = R.random_mel(1, T, seed=5).double()
    sc, sh = cnn._fold(s, "spec_bn", 0.0)
    x = mel[:, None] * float(sc[0]) + float(sh[0])
    for i in range(1, 8):
        sc, sh = cnn._fold(s, f"layer{i}.bn", s[f"layer{i}.conv.bias"])
        x = F.conv2d(x, torch.from_numpy(s[f"layer{i}.conv.weight"]), None, padding=1)
        x = x * torch.from_numpy(sc)[None, :, None, None] + torch.from_numpy(sh)[None, :, None, None]
        x = F.max_pool2d(F.relu(x), 2)
    x = x[:, :, 0, :].amax(dim=2)
    sc, sh = cnn._fold(s, "bn", s["dense1.bias"])
    x = F.relu((x @ torch.from_numpy(s["dense1.weight"]).T) * torch.from_numpy(sc) + torch.from_numpy(sh))
    got = torch.sigmoid(x @ torch.from_numpy(s["dense2.weight"]).T + torch.from_numpy(s["dense2.bias"]))
    assert float((got - R.body(mel, state)).abs().max()) <= 1e-12


@pytest.mark.parametrize("L", [32768, 59049])
def test_front_end_equals_torch_stft(L):
    state = R.random_state(16, seed=1)
    wave = R.noise(2, L, seed=L).double()
    a, b = R.logmel(wave, state["spec.mel_scale.fb"]), R.logmel_stft(wave, state["spec.mel_scale.fb"])
    assert a.shape == (2, R.N_MELS, L // R.HOP + 1)
    assert float((a - b).abs().max()) <= 1e-9  # dB
    assert float(a.min()) > -60.0  # no band at the 1e-10 clamp (-100 dB)


def test_dft_basis_is_the_windowed_cos_sin():
    from ce_amd import cnn

    b = cnn.dft_basis()
    assert b.shape == (2, R.N_FFT, R.N_BINS) and b.dtype == np.float32
    n = np.arange(R.N_FFT)[:, None]
    f = np.arange(R.N_BINS)[None, :]
    w = np.hanning(R.N_FFT + 1)[:-1][:, None]  # periodic Hann
    assert np.abs(b[0] - w * np.cos(2 * np.pi * n * f / R.N_FFT)).max() < 1e-7
    assert np.abs(b[1] - w * np.sin(2 * np.pi * n * f / R.N_FFT)).max() < 1e-7


def test_state_dict_intake():
    from ce_amd import cnn

    for nc in (16, 48):
        state = R.random_state(nc, seed=3)
        assert any(k.endswith("num_batches_tracked") for k in state)
        got_nc, s = cnn.read_state(state)
        assert got_nc == nc
        assert set(s) == set(cnn.state_shapes(nc))
        assert not any(k.endswith("num_batches_tracked") for k in s)
        rec = cnn.pack_state(nc, s)
        assert rec.dtype == np.float32 and rec.size == cnn._lib.load().ce_cnn_weights_floats(nc)
    # every key the member reads is a key of the reference's state dict (and the rest are the ignored ones)
    state = R.random_state(16, seed=3)
    extra = set(state) - set(cnn.state_shapes(16))
    assert extra and all(k.endswith("num_batches_tracked") or k == "spec.spectrogram.window" for k in extra)
    for key in cnn.state_shapes(16):
        short = {k: v for k, v in state.items() if k != key}
        with pytest.raises(ValueError, match=key.replace(".", r"\.")):
            cnn.read_state(short)
    bad = dict(state)
    bad["layer3.bn.running_var"] = torch.ones(16)
    with pytest.raises(ValueError, match=r"layer3\.bn\.running_var"):
        cnn.read_state(bad)
    bad = dict(state)
    bad["layer1.conv.weight"] = torch.ones(20, 1, 3, 3)
    with pytest.raises(ValueError, match=r"layer1\.conv\.weight"):
        cnn.read_state(bad)


def test_packed_record_layout():
    """Where the engine reads a tensor is where pack_state puts it."""
    from ce_amd import cnn

    nc = 16
    _, s = cnn.read_state(R.random_state(nc, seed=4))
    rec = cnn.pack_state(nc, s)
    sc, sh = cnn._fold(s, "spec_bn", 0.0)
    assert rec[0] == np.float32(sc[0]) and rec[1] == np.float32(sh[0]) and not rec[2:16].any()
    w1 = s["layer1.conv.weight"]
    assert rec[16 + (1 * 3 + 2) * nc + 5] == np.float32(w1[5, 0, 1, 2])
    o2 = 16 + 9 * nc + 2 * nc  # block 2's weights: row (ky 3 + kx) Cin + ci, Cout innermost
    w2 = s["layer2.conv.weight"]
    assert rec[o2 + ((2 * 3 + 0) * nc + 7) * nc + 3] == np.float32(w2[3, 7, 2, 0])
    assert np.array_equal(rec[-16:-12], s["dense2.bias"].astype(np.float32)) and not rec[-12:].any()
    d = 4 * nc
    assert np.array_equal(rec[-16 - 4 * d:-16].reshape(4, d), s["dense2.weight"].astype(np.float32))


def test_argument_errors_without_gpu():
    from ce_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)
    nc, T, n = 16, 231, 2
    ws = lib.ce_cnn_workspace_bytes(n, T, nc)
    assert ws >= 2 * n * 64 * (T // 2) * nc * 4
    assert lib.ce_cnn_workspace_bytes(2 * n, T, nc) > ws
    assert lib.ce_cnn_weights_floats(24) == 0 and lib.ce_cnn_weights_floats(16) > 0

    def fwd(n_mels=128, T=T, nc=nc, Uw=1, U=3, ws_bytes=ws, y=None, cm=None):
        return lib.ce_cnn_forward_users(p, n, n_mels, T, p, nc, Uw, p, U, 0, None, y, cm, p, 4, p, ws_bytes, None)

    assert fwd(T=127) == _lib.CE_EINVAL and b"T=127" in lib.ce_last_error()
    for bad_nc in (0, -16, 24, 8):
        assert fwd(nc=bad_nc) == _lib.CE_EINVAL and b"multiple of 16" in lib.ce_last_error()
    assert fwd(Uw=2, U=3) == _lib.CE_EINVAL and b"Uw=2" in lib.ce_last_error()
    assert fwd(n_mels=96) == _lib.CE_EINVAL and b"96 bands" in lib.ce_last_error()
    assert fwd(ws_bytes=ws - 1) == _lib.CE_EWORKSPACE
    assert fwd(y=p) == _lib.CE_EINVAL  # labels without counts
    assert lib.ce_cnn_logmel(p, 2, 300, 300, p, p, p, None) == _lib.CE_EINVAL  # shorter than one window
    assert lib.ce_cnn_logmel(p, 2, 1024, 512, p, p, p, None) == _lib.CE_EINVAL  # pitch below L
    too_long = 8 * 65535 * 256  # T = 8 * 65535 + 1 frames: one frame tile more than the grid holds
    assert lib.ce_cnn_logmel(p, 2, too_long, too_long, p, p, p, None) == _lib.CE_EINVAL
    assert b"L=" in lib.ce_last_error()


def test_activations_argument_errors_without_gpu():
    from ce_amd import _lib

    lib = _lib.load()
    p = ctypes.c_void_p(256)
    nc, T, n = 16, 231, 2
    ws = lib.ce_cnn_workspace_bytes(n, T, nc)

    def act(n=n, n_mels=128, T=T, nc=nc, block=3, ws_bytes=ws, mel=p, out=p):
        return lib.ce_cnn_activations(mel, n, n_mels, T, p, nc, p, block, out, p, ws_bytes, None)

    for bad in (0, 8, -1):
        assert act(block=bad) == _lib.CE_EINVAL and f"block={bad}".encode() in lib.ce_last_error()
    assert act(T=127) == _lib.CE_EINVAL and b"T=127" in lib.ce_last_error()
    assert act(nc=24) == _lib.CE_EINVAL and b"multiple of 16" in lib.ce_last_error()
    assert act(n_mels=96) == _lib.CE_EINVAL and b"96 bands" in lib.ce_last_error()
    assert act(n=65536) == _lib.CE_EINVAL and b"n=65536" in lib.ce_last_error()
    assert act(n=-1) == _lib.CE_EINVAL
    assert act(ws_bytes=ws - 1) == _lib.CE_EWORKSPACE
    assert act(mel=None) == _lib.CE_EINVAL and act(out=None) == _lib.CE_EINVAL and b"null" in lib.ce_last_error()
    assert act(n=0, mel=None) == _lib.CE_OK  # nothing to run


def test_member_activations_refuses_bad_arguments():
    from ce_amd import cnn

    m = cnn.DeviceShortChunkCNN.__new__(cnn.DeviceShortChunkCNN)
    with pytest.raises(ValueError, match="HIP device"):
        m.activations(torch.zeros(1, 128, 128), 1)


@pytest.mark.parametrize("nc,S,T", X.EXACT_CASES)
def test_exact_states_are_exact_and_alive(nc, S, T):
    """What the bit-for-bit GPU comparison rests on, for every case it uses:
    float32 equals float64 at every block and at the logits; at least 0.4 of a
    block's activations are non-zero and they take at least 50 distinct values;
    the HTK bank of these states has bands that hold no bin."""
    for seed in X.EXACT_SEEDS:
        state, mel, acts, z = X.exact_case(nc, S, T, seed)
        with torch.no_grad():
            a32 = R.activations(mel, state)
            z32 = R.logits(a32[-1], state).numpy()
        assert len(acts) == 7
        for b, (a64, a) in enumerate(zip(acts, a32), start=1):
            a = a.permute(0, 2, 3, 1).numpy()
            assert a.dtype == np.float32 and a64.dtype == np.float64
            assert a64.shape == (S, 128 >> b, T >> b, R.CH[b] * nc)
            assert np.array_equal(a.astype(np.float64), a64), (seed, b)
            assert np.array_equal(a64.astype(np.float32).astype(np.float64), a64), (seed, b)
            assert np.abs(a64).max() <= 128.0
            assert np.count_nonzero(a64) >= 0.4 * a64.size, (seed, b, np.count_nonzero(a64) / a64.size)
            assert np.unique(a64).size >= 50, (seed, b, np.unique(a64).size)
        assert np.array_equal(z32.astype(np.float64), z), seed
    fb = state["spec.mel_scale.fb"].numpy()
    assert fb.shape == (R.N_BINS, R.N_MELS) and (fb >= 0).all() and (fb.sum(0) == 0).any()


def test_packed_exact_state_is_the_state():
    """The record of an exact state holds the weights themselves: the folded
    scales are the BatchNorm weights, the shifts bias + bn.bias, to the bit."""
    from ce_amd import cnn

    nc = 16
    _, s = cnn.read_state(X.exact_state(nc, seed=0))
    rec = cnn.pack_state(nc, s)
    assert rec[0] == np.float32(0.5) and rec[1] == np.float32(0.25)
    o = 16 + 9 * nc
    assert np.array_equal(rec[o:o + nc], s["layer1.bn.weight"].astype(np.float32))
    want = s["layer1.conv.bias"] * s["layer1.bn.weight"] + s["layer1.bn.bias"]
    assert np.array_equal(rec[o + nc:o + 2 * nc].astype(np.float64), want)
    assert set(np.unique(rec[16:16 + 9 * nc])) == {-1.0, 0.0, 1.0}


def test_member_refuses_a_cpu_tensor():
    from ce_amd import cnn

    m = cnn.DeviceShortChunkCNN.__new__(cnn.DeviceShortChunkCNN)
    with pytest.raises(ValueError, match="HIP device"):
        m._check_wave(torch.zeros(2, 1024))
