"""The short-chunk CNN member on the device, inference.

The reference's fifth member type is ``ShortChunkCNN`` (short_cnn.py:278-349),
loaded and run in eval mode by ``predict_cnn`` (amg_test.py:173-201) at :430
and :462.  ``DeviceShortChunkCNN`` holds the weights of one shared model, or of
one model per user, as packed f32 records on the device (include/ce.h,
ce_cnn_forward_users) and predicts every user's excerpts with the owner's
model: ``[total_items, 4]`` float32, a song-level member of
``BatchedSelectionSession.step(frames=[...])``.  Re-training stays on the host:
a user's new weights come back through ``set_model``.

Rows are in session order (stacked songs), not in the order of the reference's
shuffled loader.
"""
from __future__ import annotations

import numpy as np
import torch

from . import _lib, ops
from ._lib import call
from .ops import _p, _stream
from .select import _device

N_FFT, HOP, N_BINS, N_MELS, N_CLASS, N_BLOCKS = 512, 256, 257, 128, 4, 7
BN_EPS = 1e-5  # torch.nn.BatchNorm*'s default, which the reference keeps
_CH = (0, 1, 1, 2, 2, 2, 2, 4)  # channels after block i, in units of nc (block 1 reads one channel)
_BN = ("weight", "bias", "running_mean", "running_var")


def state_shapes(nc):
    """Every key of the reference's state dict this member reads -> its shape."""
    d = 4 * nc
    s = {"spec.mel_scale.fb": (N_BINS, N_MELS)}
    s.update({f"spec_bn.{k}": (1,) for k in _BN})
    for i in range(1, N_BLOCKS + 1):
        cin, cout = (1 if i == 1 else _CH[i - 1] * nc), _CH[i] * nc
        s[f"layer{i}.conv.weight"] = (cout, cin, 3, 3)
        s[f"layer{i}.conv.bias"] = (cout,)
        s.update({f"layer{i}.bn.{k}": (cout,) for k in _BN})
    s["dense1.weight"], s["dense1.bias"] = (d, d), (d,)
    s.update({f"bn.{k}": (d,) for k in _BN})
    s["dense2.weight"], s["dense2.bias"] = (N_CLASS, d), (N_CLASS,)
    return s


def _host(a):
    if isinstance(a, torch.Tensor):
        a = a.detach().cpu().numpy()
    return np.asarray(a)


def read_state(state):
    """The arrays of a state dict as float64 host arrays, checked: nc is read
    from ``layer1.conv.weight``; a missing key or a wrong shape raises a
    ValueError naming the key; other keys (``num_batches_tracked``, the
    spectrogram's window) are ignored.  Returns (nc, {key: array})."""
    key = "layer1.conv.weight"
    if key not in state:
        raise ValueError(f"the state dict lacks {key!r}")
    w = _host(state[key])
    if w.ndim != 4 or w.shape[1:] != (1, 3, 3) or w.shape[0] < 16 or w.shape[0] % 16:
        raise ValueError(f"{key!r} has shape {tuple(w.shape)}: expected (nc, 1, 3, 3) with nc a positive multiple of 16")
    nc = int(w.shape[0])
    out = {}
    for key, shape in state_shapes(nc).items():
        if key not in state:
            raise ValueError(f"the state dict lacks {key!r}")
        a = _host(state[key])
        if tuple(a.shape) != shape:
            raise ValueError(f"{key!r} has shape {tuple(a.shape)}, expected {shape} (nc = {nc})")
        out[key] = a.astype(np.float64)
    return nc, out


def _fold(s, prefix, bias):
    """BatchNorm(x + bias) with running statistics as fma(scale, x, shift), in double."""
    scale = s[f"{prefix}.weight"] / np.sqrt(s[f"{prefix}.running_var"] + BN_EPS)
    return scale, (bias - s[f"{prefix}.running_mean"]) * scale + s[f"{prefix}.bias"]


def pack_state(nc, s):
    """One model's packed f32 record (include/ce.h): the layout of csrc/ce_cnn.hpp's CnnLayout."""
    def pad16(a):
        return np.concatenate([a.reshape(-1), np.zeros(16 - a.size)])

    parts = [pad16(np.concatenate(_fold(s, "spec_bn", 0.0)))]
    for i in range(1, N_BLOCKS + 1):
        w = s[f"layer{i}.conv.weight"]  # [Cout, Cin, ky, kx] -> [(ky, kx, ci), Cout]
        parts.append(w.transpose(2, 3, 1, 0).reshape(-1))
        parts.extend(_fold(s, f"layer{i}.bn", s[f"layer{i}.conv.bias"]))
    parts.append(s["dense1.weight"].T.reshape(-1))
    parts.extend(_fold(s, "bn", s["dense1.bias"]))
    parts.append(s["dense2.weight"].reshape(-1))
    parts.append(pad16(s["dense2.bias"]))
    rec = np.concatenate(parts).astype(np.float32)
    want = int(_lib.load().ce_cnn_weights_floats(nc))
    if rec.size != want:
        raise RuntimeError(f"packed record of {rec.size} floats, the engine's layout holds {want}")
    return rec


def dft_basis():
    """[2, 512, 257] float32: w[n] cos(2 pi f n / 512) and w[n] sin(2 pi f n /
    512), w the periodic Hann window; the angle from f n mod 512, in double."""
    n = np.arange(N_FFT, dtype=np.int64)
    ang = 2.0 * np.pi * ((n[:, None] * np.arange(N_BINS, dtype=np.int64)[None, :]) % N_FFT) / N_FFT
    w = (0.5 - 0.5 * np.cos(2.0 * np.pi * n / N_FFT))[:, None]
    return np.stack([w * np.cos(ang), w * np.sin(ang)]).astype(np.float32)


def n_frames(L):
    return int(L) // HOP + 1


class DeviceShortChunkCNN:
    """U short-chunk CNN members on the device.  ``state``: the reference's
    state dict (key names -> arrays or tensors; ``state_shapes(nc)`` lists the
    keys read).  U users share that one model until the first ``set_model``,
    which gives every user a record of their own.  The filter bank
    (``spec.mel_scale.fb``, a buffer no training touches) and the DFT basis are
    kept once for the member."""

    def __init__(self, state, U=1, device=None):
        self.dev = _device(device)
        self.U = int(U)
        if self.U < 1:
            raise ValueError("DeviceShortChunkCNN needs U >= 1")
        self.nc, s = read_state(state)
        self.C = N_CLASS
        self._fb_host = s["spec.mel_scale.fb"].astype(np.float32)
        self._states = [s]  # host copies: one shared, or one per user
        self.weights = torch.from_numpy(pack_state(self.nc, s)).to(self.dev).unsqueeze(0).contiguous()
        self.fb = torch.from_numpy(self._fb_host).to(self.dev).contiguous()
        self.basis = torch.from_numpy(dft_basis()).to(self.dev).contiguous()
        self._ws = None
        self._one = torch.tensor([0, 1 << 62], dtype=torch.int64).to(self.dev)  # one user owning every excerpt

    @property
    def Uw(self):
        return self.weights.shape[0]

    def set_model(self, u, state):
        """User u's weights after a host retrain.  The first call turns the
        shared model into U own copies.  Returns self."""
        u = int(u)
        if not 0 <= u < self.U:
            raise ValueError(f"user {u} outside [0, {self.U})")
        nc, s = read_state(state)
        if nc != self.nc:
            raise ValueError(f"'layer1.conv.weight' names nc = {nc}, this member holds nc = {self.nc}")
        if not np.array_equal(s["spec.mel_scale.fb"].astype(np.float32), self._fb_host):
            raise ValueError("'spec.mel_scale.fb' differs from the member's filter bank: the front end is shared")
        rec = torch.from_numpy(pack_state(nc, s)).to(self.dev)
        if self.Uw != self.U:
            self.weights = self.weights.expand(self.U, -1).contiguous()
            self._states = [self._states[0]] * self.U
        self.weights[u].copy_(rec)
        self._states[u] = s
        return self

    def state(self):
        """Host copies: a list of Uw dicts (key -> float64 array), one shared or one per user."""
        return [{k: v.copy() for k, v in s.items()} for s in self._states]

    # ---- front end
    def _check_wave(self, wave):
        ops._on_gpu(wave, "wave")
        if wave.dim() != 2 or wave.dtype != torch.float32 or wave.shape[1] < N_FFT or \
                (wave.shape[1] > 1 and wave.stride(1) != 1):
            raise ValueError(f"wave must be a float32 [S, L >= {N_FFT}] tensor with unit sample stride")

    def logmel(self, wave, out=None):
        """wave [S, L] f32 -> the dB log-mel [S, 128, T = L // 256 + 1] f32 (before spec_bn)."""
        self._check_wave(wave)
        S, L = wave.shape
        T = n_frames(L)
        if out is None:
            out = torch.empty((S, N_MELS, T), dtype=torch.float32, device=wave.device)
        elif out.dtype != torch.float32 or tuple(out.shape) != (S, N_MELS, T) or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 [{S}, {N_MELS}, {T}] tensor")
        ld = L if S == 1 else wave.stride(0)  # a row pitch below L (an expanded or overlapping view) is refused
        call("ce_cnn_logmel", _p(wave), S, L, ld, _p(self.basis), _p(self.fb), _p(out),
             _stream(wave.device))
        return out

    # ---- network body
    def _workspace(self, n, T, dev):
        need = int(_lib.load().ce_cnn_workspace_bytes(n, T, self.nc))
        if self._ws is None or self._ws.numel() < need or self._ws.device != dev:
            self._ws = torch.empty(need, dtype=torch.uint8, device=dev)
        return self._ws

    def _forward(self, mel, weights, item_offsets, U, s_base, excl, y, cm, out):
        n, H, T = mel.shape
        ws = self._workspace(max(n, 1), max(T, N_MELS), mel.device)
        call("ce_cnn_forward_users", _p(mel), n, H, T, _p(weights), self.nc, weights.shape[0], _p(item_offsets), U,
             s_base, _p(excl), _p(y), _p(cm), _p(out), out.stride(0), _p(ws), ws.numel(), _stream(mel.device))

    def _check_mel(self, mel):
        ops._on_gpu(mel, "mel")
        if mel.dim() != 3 or mel.dtype != torch.float32 or not mel.is_contiguous():
            raise ValueError("mel must be a contiguous float32 [S, 128, T] tensor")

    def _out(self, out, S, dev, zero):
        if out is None:
            return (torch.zeros if zero else torch.empty)((S, N_CLASS), dtype=torch.float32, device=dev)
        ops._on_gpu(out, "out")
        ops.check_users_out(out, S, N_CLASS, (torch.float32,))
        return out

    def predict_proba(self, wave=None, *, mel=None, u=0, out=None, batch=128):
        """Model u's outputs [S, 4] f32 over the excerpts ``wave`` [S, L] (or
        over their log-mel ``mel`` [S, 128, T], as ``logmel`` returns it)."""
        if (wave is None) == (mel is None):
            raise ValueError("pass `wave` or `mel`")
        u = int(u)
        if not 0 <= u < self.U:
            raise ValueError(f"user {u} outside [0, {self.U})")
        w = self.weights[u if self.Uw > 1 else 0].unsqueeze(0)
        if mel is not None:
            self._check_mel(mel)
        else:
            self._check_wave(wave)
        src = mel if mel is not None else wave
        S = src.shape[0]
        out = self._out(out, S, src.device, False)
        for b in range(0, S, int(batch)):
            e = min(S, b + int(batch))
            m = mel[b:e] if mel is not None else self.logmel(wave[b:e])
            self._forward(m, w, self._one, 1, b, None, None, None, out)
        return out

    def activations(self, mel, block, u=0):
        """What block ``block`` (1 .. 7) of model u writes for the log-mel
        ``mel`` [S, 128, T]: [S, 128 >> block, T >> block, C] f32,
        channel-innermost, after BatchNorm, ReLU and the pool, by the forward's
        own launches (ce_cnn_activations).  For tests and diagnosis."""
        self._check_mel(mel)
        u, block = int(u), int(block)
        if not 0 <= u < self.U:
            raise ValueError(f"user {u} outside [0, {self.U})")
        if not 1 <= block <= N_BLOCKS:
            raise ValueError(f"block {block} outside 1 .. {N_BLOCKS}")
        w = self.weights[u if self.Uw > 1 else 0].unsqueeze(0)
        n, H, T = mel.shape
        act = torch.empty((n, N_MELS >> block, max(T, N_MELS) >> block, _CH[block] * self.nc), dtype=torch.float32,
                          device=mel.device)
        ws = self._workspace(max(n, 1), max(T, N_MELS), mel.device)
        call("ce_cnn_activations", _p(mel), n, H, T, _p(w), self.nc, _p(self._one), block, _p(act), _p(ws), ws.numel(),
             _stream(mel.device))
        return act

    def _users(self, wave, item_offsets, U, excl, y, cm, out, batch):
        self._check_wave(wave)
        S = wave.shape[0]
        batch = int(batch)
        if batch < 1:
            raise ValueError("batch must be >= 1")
        if excl is not None:
            ops._check_excl(excl, S)
        for b in range(0, S, batch):
            e = min(S, b + batch)
            self._forward(self.logmel(wave[b:e]), self.weights, item_offsets, U, b, excl, y, cm, out)
        return out

    def predict_proba_users(self, wave, item_offsets, excl=None, out=None, batch=128):
        """Every excerpt of wave [total_items, L] through the model of the user
        who owns it (item_offsets [U + 1], the sessions' stacked-song order);
        the pool is walked ``batch`` excerpts at a time.  Bit for bit
        ``predict_proba(wave, u=owner)`` whatever the batch.  Excluded excerpts
        (``excl``, a bitmap over the excerpts) are not written and skip the
        network body; the front end (3 % of the work) runs over whole batches,
        excluded excerpts included."""
        item_offsets = ops._i64(item_offsets, "item_offsets").reshape(-1)
        U = item_offsets.numel() - 1
        if U != self.U:
            raise ValueError(f"item_offsets names {U} user(s), this member {self.U} model(s)")
        self._check_wave(wave)
        out = self._out(out, wave.shape[0], wave.device, excl is not None)
        return self._users(wave, item_offsets, U, excl, None, None, out, batch)

    def predict_proba_session(self, wave, session, out=None, skip_excluded=True, batch=128):
        """The predict step of an epoch (amg_test.py:430 / :462) for every
        user: wave [total_items, L], one cropped excerpt per stacked song of the
        session -> [total_items, 4] f32, a song-level member of
        ``step(frames=[...])``.  Rows of excluded songs keep what ``out`` held
        (zero in a new tensor) and cost their front end only (3 % of the
        work; the network body is skipped).  Nothing is read back."""
        offsets = getattr(session, "offsets", None)
        if offsets is None:  # a SelectionSession: one user owning every song
            users, total = 1, int(session.N)
            offsets = torch.tensor([0, total], dtype=torch.int64).to(self.dev)
        else:
            users, total = int(session.U), int(session._off[-1])
        if users != self.U:
            raise ValueError(f"the session has {users} user(s), this member {self.U} model(s)")
        self._check_wave(wave)
        if wave.shape[0] != total:
            raise ValueError(f"wave holds {wave.shape[0]} excerpts, the session's pools {total} songs")
        return self.predict_proba_users(wave, offsets, session.excl if skip_excluded else None, out, batch)

    def evaluate(self, wave_test, y, item_offsets=None, report=False, batch=128):
        """The evaluate step of an epoch for every model: wave_test [S, L] the
        users' test excerpts stacked, y [S] their classes, item_offsets [U + 1]
        (None: one user owning all).  Returns (f1 [U], cm [U, 4, 4]), and prf
        [U, 4, 4] with report=True, as the other members do.  The outputs the
        labels were taken from stay in ``last_proba`` [S, 4]."""
        self._check_wave(wave_test)
        S = wave_test.shape[0]
        if item_offsets is None:
            item_offsets = torch.tensor([0, S], dtype=torch.int64).to(wave_test.device)
        item_offsets = ops._i64(item_offsets, "item_offsets").reshape(-1)
        U = item_offsets.numel() - 1
        if U != self.U:
            raise ValueError(f"item_offsets names {U} user(s), this member {self.U} model(s)")
        y = ops._labels_i32(y, S)
        cm = torch.zeros((U, N_CLASS, N_CLASS), dtype=torch.int64, device=wave_test.device)
        self.last_proba = self._users(wave_test, item_offsets, U, None, y, cm,
                                      self._out(None, S, wave_test.device, True), batch)
        if report:
            f1, prf = ops.f1_weighted_users(cm, report=True)
            return f1, cm, prf
        return ops.f1_weighted_users(cm), cm


__all__ = ["DeviceShortChunkCNN", "state_shapes", "read_state", "pack_state", "dft_basis", "n_frames"]
