"""The spectral front end on the GPU (include/specfe.h): STFT / inverse STFT with autograd, the log-mel spectrogram, and
the spectrogram keys of a batch computed on the device.

Mirrors (does not import) the reference interfaces:
  * ``STFT(n_fft=256, hop_length=128).stft(mix_audio) -> [B, 2, T, F]``      src/encoders/stft.py:14-38
  * ``torch.istft(spec, n_fft, hop_length, window=hann, length=...)``         src/model/rtfsnet.py:843-849  -> ``STFT.istft``
  * ``get_spectrogram``: ``log(MelSpectrogram(sample_rate=16000)(x).clamp(1e-5))``  src/datasets/base_dataset.py:115-123,165
    -> ``LogMelSpectrogram``; the reference computes it per item on loader threads, ``add_spectrogram_keys`` computes the
    keys ``complex_spectrogram`` / ``mix_spectrogram`` / ``s1_spectrogram`` / ``s2_spectrogram`` of a whole batch on the device.
Every call is one launch on the inputs' device and the current stream, with no host synchronisation; outputs come from
torch's allocator.  As everywhere in this package there is no CPU path: a CPU tensor raises RuntimeError.

The mel filterbank follows torchaudio's documented defaults (HTK scale, no norm, f_min 0, f_max sr / 2); torchaudio is
not a dependency and the parity of that one table with it is unpinned.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Optional

import torch

_HANDLES: Dict[tuple, int] = {}                      # (device, n_fft, hop, sample_rate, n_mels) -> specfe handle (kept for the process)


def _device_of(t: torch.Tensor, who: str) -> torch.device:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: expected a torch.Tensor, got {type(t).__name__}")
    if t.device.type != "cuda":
        raise RuntimeError(f"{who} computes only on an AMD GPU through libdptnav (got a {t.device} tensor); "
                           f"there is no CPU/PyTorch fallback")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: expected float32, got {t.dtype}")
    return t.device if t.device.index is not None else torch.device("cuda", torch.cuda.current_device())


def _handle(dev: torch.device, n_fft: int, hop: int, sample_rate: int = 0, n_mels: int = 0) -> int:
    from . import _lib
    key = (dev, int(n_fft), int(hop), int(sample_rate), int(n_mels))
    if key not in _HANDLES:
        lib = _lib.load()
        h = ctypes.c_void_p()
        with torch.cuda.device(dev):
            if n_mels:
                rc = lib.specfe_create_mel(key[1], key[2], key[3], key[4], ctypes.byref(h))
            else:
                rc = lib.specfe_create(key[1], key[2], ctypes.byref(h))
        if rc:
            raise (ValueError if rc == 1 else RuntimeError)(f"specfe_create(n_fft={n_fft}, hop={hop}): {lib.specfe_strerror(rc).decode()}")
        _HANDLES[key] = h.value
    return _HANDLES[key]


def _call(name: str, dev: torch.device, what: str, *args):
    from . import _lib
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise (ValueError if rc == 1 else RuntimeError)(f"{name}({what}): {lib.specfe_strerror(rc).decode()}")


def _check_sizes(n_fft: int, hop: int):
    if n_fft % 16 or not 32 <= n_fft <= 512 or not 1 <= hop <= n_fft // 2:
        raise ValueError(f"n_fft must be a multiple of 16 in [32, 512] and 1 <= hop_length <= n_fft / 2, got n_fft={n_fft}, "
                         f"hop_length={hop}")


def stft_forward(x: torch.Tensor, n_fft: int, hop: int) -> torch.Tensor:
    """specfe_stft: x [B, T] -> [B, 2, 1 + T // hop, n_fft // 2 + 1]; no autograd."""
    dev = _device_of(x, "stft")
    if x.dim() != 2 or x.shape[1] <= n_fft // 2:
        raise ValueError(f"stft takes [batch, samples] with more than n_fft / 2 = {n_fft // 2} samples, got {tuple(x.shape)}")
    x = x.detach().contiguous()
    B, T = x.shape
    with torch.cuda.device(dev):
        out = torch.empty(B, 2, 1 + T // hop, n_fft // 2 + 1, dtype=torch.float32, device=dev)
    if B:
        _call("specfe_stft", dev, f"B={B}, T={T}", _handle(dev, n_fft, hop), x.data_ptr(), B, T, out.data_ptr())
    return out


def stft_backward(g: torch.Tensor, T: int, n_fft: int, hop: int) -> torch.Tensor:
    """specfe_stft_backward: d loss / d X [B, 2, M, F] -> d loss / d x [B, T]."""
    dev = _device_of(g, "stft backward")
    g = g.detach().contiguous()
    B = g.shape[0]
    assert tuple(g.shape[1:]) == (2, 1 + T // hop, n_fft // 2 + 1), tuple(g.shape)
    with torch.cuda.device(dev):
        out = torch.empty(B, T, dtype=torch.float32, device=dev)
    if B:
        _call("specfe_stft_backward", dev, f"B={B}, T={T}", _handle(dev, n_fft, hop), g.data_ptr(), B, T, out.data_ptr())
    return out


def _inverse_length(M: int, n_fft: int, hop: int, length: Optional[int]) -> int:
    L = (M - 1) * hop if length is None else int(length)
    if L < 1:
        raise ValueError(f"istft: output length {L} (frames={M}, hop_length={hop}, length={length}); it must be at least 1")
    return L


def istft_forward(spec: torch.Tensor, n_fft: int, hop: int, length: Optional[int] = None) -> torch.Tensor:
    """specfe_istft: spec [B, 2, M, F] -> [B, length] (the natural (M - 1) hop if `length` is None); no autograd."""
    dev = _device_of(spec, "istft")
    if spec.dim() != 4 or spec.shape[1] != 2 or spec.shape[3] != n_fft // 2 + 1 or spec.shape[2] < 1:
        raise ValueError(f"istft takes [batch, 2, frames, {n_fft // 2 + 1}], got {tuple(spec.shape)}")
    spec = spec.detach().contiguous()
    B, M = spec.shape[0], spec.shape[2]
    L = _inverse_length(M, n_fft, hop, length)
    with torch.cuda.device(dev):
        out = torch.empty(B, L, dtype=torch.float32, device=dev)
    if B:
        _call("specfe_istft", dev, f"B={B}, M={M}, length={L}", _handle(dev, n_fft, hop), spec.data_ptr(), B, M, L, out.data_ptr())
    return out


def istft_backward(g: torch.Tensor, M: int, n_fft: int, hop: int) -> torch.Tensor:
    """specfe_istft_backward: d loss / d y [B, L] -> d loss / d spec [B, 2, M, F]."""
    dev = _device_of(g, "istft backward")
    g = g.detach().contiguous()
    B, L = g.shape
    with torch.cuda.device(dev):
        out = torch.empty(B, 2, M, n_fft // 2 + 1, dtype=torch.float32, device=dev)
    if B:
        _call("specfe_istft_backward", dev, f"B={B}, M={M}, length={L}", _handle(dev, n_fft, hop), g.data_ptr(), B, M, L,
              out.data_ptr())
    return out


def logmel_forward(x: torch.Tensor, sample_rate: int, n_fft: int, hop: int, n_mels: int) -> torch.Tensor:
    """specfe_logmel: x [B, T] -> [B, n_mels, 1 + T // hop]."""
    dev = _device_of(x, "log-mel")
    if x.dim() != 2 or x.shape[1] <= n_fft // 2:
        raise ValueError(f"log-mel takes [batch, samples] with more than n_fft / 2 = {n_fft // 2} samples, got {tuple(x.shape)}")
    x = x.detach().contiguous()
    B, T = x.shape
    with torch.cuda.device(dev):
        out = torch.empty(B, n_mels, 1 + T // hop, dtype=torch.float32, device=dev)
    if B:
        _call("specfe_logmel", dev, f"B={B}, T={T}", _handle(dev, n_fft, hop, sample_rate, n_mels), x.data_ptr(), B, T,
              out.data_ptr())
    return out


class _StftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, n_fft, hop):
        ctx.meta = (x.shape[1], n_fft, hop)
        return stft_forward(x, n_fft, hop)

    @staticmethod
    def backward(ctx, g):
        return stft_backward(g, *ctx.meta), None, None


class _IstftFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, spec, n_fft, hop, length):
        ctx.meta = (spec.shape[2], n_fft, hop)
        return istft_forward(spec, n_fft, hop, length)

    @staticmethod
    def backward(ctx, g):
        return istft_backward(g, *ctx.meta), None, None, None


class STFT:
    """The reference's encoder (src/encoders/stft.py): ``STFT(n_fft, hop_length).stft(mix_audio)`` -> [B, 2, T, F] with
    torch.stft's meaning under a periodic Hann window, center=True / reflect, one-sided, not normalised -- one launch that
    frames, reflects, windows and writes that layout.  ``istft(spec, length=None)`` is torch.istft on the same layout
    (AudioDecoder, src/model/rtfsnet.py:843-849).  Both are differentiable (``loss.backward()`` runs the two adjoint kernels)."""

    def __init__(self, n_fft: int = 256, hop_length: int = 128):
        _check_sizes(int(n_fft), int(hop_length))
        self.n_fft = int(n_fft)
        self.hop_length = int(hop_length)
        self.window = torch.hann_window(self.n_fft)            # as the reference's attribute; the kernels own their copy

    def stft(self, mix_audio: torch.Tensor) -> torch.Tensor:
        _device_of(mix_audio, "STFT.stft")
        return _StftFn.apply(mix_audio, self.n_fft, self.hop_length)

    def istft(self, spec: torch.Tensor, length: Optional[int] = None) -> torch.Tensor:
        _device_of(spec, "STFT.istft")
        return _IstftFn.apply(spec, self.n_fft, self.hop_length, length)


class LogMelSpectrogram:
    """``log(clamp(MelSpectrogram(sample_rate, n_fft, hop_length, n_mels)(x), 1e-5))`` with torchaudio's other defaults
    (power 2, f_min 0, f_max sample_rate / 2, HTK scale, no norm), the reference's get_spectrogram, in one launch:
    [B, T] -> [B, n_mels, 1 + T // hop_length], [B, 1, T] -> [B, 1, n_mels, frames].  No autograd."""

    def __init__(self, sample_rate: int = 16000, n_fft: int = 400, hop_length: int = 200, n_mels: int = 128):
        _check_sizes(int(n_fft), int(hop_length))
        if int(sample_rate) < 2 or not 1 <= int(n_mels) <= 256:
            raise ValueError(f"sample_rate must be at least 2 and n_mels in [1, 256], got {sample_rate}, {n_mels}")
        self.sample_rate, self.n_fft, self.hop_length, self.n_mels = int(sample_rate), int(n_fft), int(hop_length), int(n_mels)

    def __call__(self, audio: torch.Tensor) -> torch.Tensor:
        _device_of(audio, "LogMelSpectrogram")
        if audio.requires_grad:
            raise RuntimeError("LogMelSpectrogram has no backward: detach the input (the reference computes it in the loader)")
        if audio.dim() == 3 and audio.shape[1] == 1:
            return logmel_forward(audio[:, 0], self.sample_rate, self.n_fft, self.hop_length, self.n_mels).unsqueeze(1)
        return logmel_forward(audio, self.sample_rate, self.n_fft, self.hop_length, self.n_mels)


def add_spectrogram_keys(batch: dict, stft: Optional[STFT] = None, logmel: Optional[LogMelSpectrogram] = None) -> dict:
    """Fill the spectrogram keys of a device batch (PinnedBatcher.to_device) in place, as the reference's dataset does per
    item on the host (base_dataset.py:115-130): ``complex_spectrogram`` = stft.stft(mix), ``mix_spectrogram`` /
    ``s1_spectrogram`` / ``s2_spectrogram`` = logmel(mix / s1 / s2).  A key whose waveform is absent (None or missing, as
    s1 / s2 at inference) is left as it is.  Defaults: ``STFT()`` and ``LogMelSpectrogram()``.  Returns the batch."""
    stft = STFT() if stft is None else stft
    logmel = LogMelSpectrogram() if logmel is None else logmel
    with torch.no_grad():
        for src in ("mix", "s1", "s2"):
            wav = batch.get(src)
            if wav is None:
                continue
            batch[f"{src}_spectrogram"] = logmel(wav.detach())
            if src == "mix":
                batch["complex_spectrogram"] = stft.stft(wav.detach())
    return batch
