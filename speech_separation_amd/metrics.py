"""Waveform criteria (forward + backward) and the SI-SNR(i), SI-SDR and STOI / ESTOI metrics computed on the GPU.

Mirrors (does not import) the reference interfaces that consume the model's outputs:
  * ``SiSNRWavLoss()(**batch) -> {"loss": tensor}``          src/loss/ss_losses.py:117-130 (+ BaseSSLoss :21-26)
  * ``MAEWavLoss()`` / ``MSEWavLoss()``, same call            src/loss/ss_losses.py:65-93   (+ BaseSSLoss :21-26)
  * ``MSESpecLoss()`` / ``L1SpecLoss()`` on spectrograms      src/loss/ss_losses.py:29-62   (+ BaseSSLoss :21-26)
  * ``SISNRiMetric(name=..., device=...)(**batch) -> value``  src/metrics/si_snri.py:7-30
  * ``SISNRMetric(name=..., device=...)(**batch) -> value``   src/metrics/si_snr.py:6-12
  * ``SISDRMetric(name=..., device=...)(**batch) -> value``   src/metrics/si_sdr.py
  * ``STOIMetric(fs, extended, name=..., device=...)(**batch) -> value``   src/metrics/stoi.py
All resolve the speaker permutation at BATCH level by default (compare the two batch means), exactly as the reference
does (ss_losses.py:21-25, base_metric.py:57-60) -- this is not per-utterance PIT.  The three criteria take
``pit="utterance"`` for per-utterance PIT (include/wavloss.h: the reference's class on every item alone, averaged); the
metrics stay batch level.

The reference needs >= 6 ``.item()`` syncs per batch for the metrics (base_metric.py:53-56, si_snri.py:25-26); here the
per-item statistics come from ``dptnav_sisnr_pairs`` (one launch) and the 12*B numbers are reduced on the host with ONE
device->host copy.  The LOSS never touches the host: ``dptnav_pit_sisnr_loss`` / ``wavloss_pit_loss`` resolve the
permutation on the device, return the loss as a 0-dim device tensor and leave d loss / d prediction ready for
``loss.backward()`` (two launches instead of ~40 PyTorch kernels and a tensor->bool conversion).
"""
from __future__ import annotations

from typing import Dict

import torch

from .engine import DptnEngine
from .spec import DPTN_AV

_ENGINES: Dict[torch.device, DptnEngine] = {}


def _engine(device: torch.device) -> DptnEngine:
    if device.type != "cuda":
        raise RuntimeError("speech_separation_amd.metrics computes on an AMD GPU through libdptnav; there is no CPU path")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    if device not in _ENGINES:
        _ENGINES[device] = DptnEngine(DPTN_AV, device)   # the statistics kernel needs a handle, not weights
    return _ENGINES[device]


def pair_statistics(s1_pred, s2_pred, s1, s2, mix) -> torch.Tensor:
    """(6,2) CPU tensor of BATCH MEANS: rows = (p1,s1) (p1,s2) (p2,s1) (p2,s2) (mix,s1) (mix,s2);
    columns = (SI-SNR dB, reference loss term).  One launch, one sync."""
    stats = _engine(mix.device).sisnr_pairs(s1_pred, s2_pred, s1, s2, mix)
    return stats.double().mean(0).cpu()


class _PitSisnrFn(torch.autograd.Function):
    """loss = BaseSSLoss(SiSNRLoss) (ss_losses.py:21-26,100-114); the forward launch pair already writes the gradient."""

    @staticmethod
    def forward(ctx, s1_pred, s2_pred, s1, s2):
        d1, d2, out = _engine(s1_pred.device).pit_sisnr_loss(s1_pred, s2_pred, s1, s2)
        ctx.save_for_backward(d1, d2)
        ctx.mark_non_differentiable(out)
        return out[0].clone(), out

    @staticmethod
    def backward(ctx, g, _g_stats):
        d1, d2 = ctx.saved_tensors
        return g * d1, g * d2, None, None


_KINDS = {"mae": 0, "mse": 1, "sisnr": 2}            # WAVLOSS_MAE / _MSE / _SISNR       (include/wavloss.h)
_LEVELS = {"batch": 0, "utterance": 1}               # WAVLOSS_PIT_BATCH / _UTTERANCE


def _check_pit(pit) -> str:
    if pit not in _LEVELS:
        raise ValueError(f"pit must be 'batch' or 'utterance', got {pit!r}")
    return pit


def _wav_inputs(s1_pred, s2_pred, s1, s2):
    """Four fp32 tensors of one 2-D shape on one GPU -> detached, contiguous."""
    named = (("s1_pred", s1_pred), ("s2_pred", s2_pred), ("s1", s1), ("s2", s2))
    for n, t in named:
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{n}: expected a torch.Tensor, got {type(t).__name__}")
    dev = s1_pred.device
    if dev.type != "cuda":
        raise RuntimeError("speech_separation_amd.metrics computes on an AMD GPU through libdptnav; there is no CPU path")
    for n, t in named:
        if tuple(t.shape) != tuple(s1_pred.shape) or t.dim() != 2:
            raise ValueError(f"{n}: shape {tuple(t.shape)} does not match s1_pred's {tuple(s1_pred.shape)}; the criterion takes "
                             f"four [batch, samples] tensors of one shape (the reference would broadcast or fail here)")
        if t.device != dev:
            raise ValueError(f"{n}: lives on {t.device}, s1_pred on {dev}")
        if t.dtype != torch.float32:
            raise TypeError(f"{n}: expected float32, got {t.dtype}")
    return [t.detach().contiguous() for _, t in named]


def wavloss_pit_loss(kind: str, pit: str, s1_pred, s2_pred, s1, s2, grad_scale: float = 1.0):
    """wavloss_pit_loss (include/wavloss.h) on the inputs' device and the current stream
    -> (d loss / d s1_pred, d loss / d s2_pred, out[4] = loss, #items on permutation 1, L0, L1, perm int32 [B]);
    all on the device, no synchronisation; scratch and outputs come from torch's allocator."""
    from . import _lib
    ts = _wav_inputs(s1_pred, s2_pred, s1, s2)
    lib = _lib.load()
    B, T = ts[0].shape
    dev = ts[0].device
    with torch.cuda.device(dev):
        d1, d2 = torch.empty_like(ts[0]), torch.empty_like(ts[0])
        out = torch.empty(4, dtype=torch.float32, device=dev)
        perm = torch.empty(B, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.wavloss_scratch_bytes(max(B, 1))), dtype=torch.uint8, device=dev)
        rc = lib.wavloss_pit_loss(_KINDS[kind], _LEVELS[pit], *[t.data_ptr() for t in ts], B, T, float(grad_scale),
                                  d1.data_ptr(), d2.data_ptr(), out.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.numel(),
                                  torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise RuntimeError(f"wavloss_pit_loss({kind}, {pit}, B={B}, T={T}): {lib.wavloss_strerror(rc).decode()}")
    return d1, d2, out, perm


class _PitWavFn(torch.autograd.Function):
    """loss = BaseSSLoss(element loss) (ss_losses.py:21-26, :65-93, :100-114) or its per-utterance variant; the forward
    launch pair already writes the gradient."""

    @staticmethod
    def forward(ctx, s1_pred, s2_pred, s1, s2, kind, pit):
        d1, d2, out, perm = wavloss_pit_loss(kind, pit, s1_pred, s2_pred, s1, s2)
        ctx.save_for_backward(d1, d2)
        ctx.mark_non_differentiable(out, perm)
        return out[0].clone(), out, perm

    @staticmethod
    def backward(ctx, g, _g_stats, _g_perm):
        d1, d2 = ctx.saved_tensors
        return g * d1, g * d2, None, None, None, None


class _PitWavLoss(torch.nn.Module):
    """``Loss(pit="batch")(**batch) -> {"loss": 0-dim device tensor}``, differentiable w.r.t. s1_pred / s2_pred, no host
    synchronisation.  ``self.last`` keeps the device tensor [loss, #items on permutation 1, loss perm 0, loss perm 1] of
    the latest call for logging, ``self.last_perm`` the int32 [B] permutation of every item."""

    kind: str

    def __init__(self, pit: str = "batch"):
        super().__init__()
        self.pit = _check_pit(pit)
        self.last = self.last_perm = None

    def forward(self, s1_pred, s2_pred, s1, s2, **batch):
        loss, self.last, self.last_perm = _PitWavFn.apply(s1_pred, s2_pred, s1, s2, self.kind, self.pit)
        return {"loss": loss}


class MAEWavLoss(_PitWavLoss):
    """The reference's PIT L1 loss on waveforms (ss_losses.py:65-77), or its per-utterance variant (``pit="utterance"``)."""
    kind = "mae"


class MSEWavLoss(_PitWavLoss):
    """The reference's PIT MSE loss on waveforms (ss_losses.py:80-93), or its per-utterance variant (``pit="utterance"``)."""
    kind = "mse"


class _PitSpecLoss(_PitWavLoss):
    """``Loss(pit="batch")(s1_spec_pred=..., s2_spec_pred=..., s1_spec_true=..., s2_spec_true=..., **batch)``: the MAE /
    MSE criterion of include/wavloss.h on the [B, F * T] view of four spectrograms of one shape (a view, not a copy, for the
    contiguous tensors the models and add_spectrogram_keys produce); the mean over every element is the reference's
    ``reduction="mean"``.  Everything else -- ``{"loss": 0-dim device tensor}``, ``last``, ``last_perm``, ``pit=`` -- as
    the waveform classes."""

    def forward(self, s1_spec_pred, s2_spec_pred, s1_spec_true, s2_spec_true, **batch):
        named = (("s1_spec_pred", s1_spec_pred), ("s2_spec_pred", s2_spec_pred), ("s1_spec_true", s1_spec_true),
                 ("s2_spec_true", s2_spec_true))
        for n, t in named:
            if not isinstance(t, torch.Tensor):
                raise TypeError(f"{n}: expected a torch.Tensor, got {type(t).__name__}")
            if tuple(t.shape) != tuple(s1_spec_pred.shape) or t.dim() < 2:
                raise ValueError(f"{n}: shape {tuple(t.shape)} does not match s1_spec_pred's {tuple(s1_spec_pred.shape)}; the "
                                 f"criterion takes four [batch, ...] spectrograms of one shape")
        return super().forward(*[t.reshape(t.shape[0], -1) for _, t in named])


class MSESpecLoss(_PitSpecLoss):
    """The reference's PIT MSE loss on spectrograms (ss_losses.py:29-44), or its per-utterance variant (``pit="utterance"``)."""
    kind = "mse"


class L1SpecLoss(_PitSpecLoss):
    """The reference's PIT L1 loss on spectrograms (ss_losses.py:47-62), or its per-utterance variant (``pit="utterance"``)."""
    kind = "mae"


class SiSNRWavLoss(_PitWavLoss):
    """The reference's PIT SI-SNR loss: ``SiSNRWavLoss()(**batch) -> {"loss": 0-dim tensor}`` (ss_losses.py:117-130),
    differentiable w.r.t. s1_pred / s2_pred, no host synchronisation.  With the default ``pit="batch"`` the call is
    ``dptnav_pit_sisnr_loss`` and ``self.last`` keeps the device tensor [loss, permutation, loss perm 0, loss perm 1] of
    the latest call for logging (``self.last_perm`` stays None); ``pit="utterance"`` goes through ``wavloss_pit_loss``
    (``self.last`` / ``self.last_perm`` as MAEWavLoss)."""
    kind = "sisnr"

    def forward(self, s1_pred, s2_pred, s1, s2, **batch):
        if self.pit != "batch":
            return super().forward(s1_pred, s2_pred, s1, s2)
        loss, self.last = _PitSisnrFn.apply(s1_pred, s2_pred, s1, s2)
        return {"loss": loss}


class SISNRMetric:
    """``metric(**batch) -> value`` as the reference's (one launch, one device->host copy).  For a loop that must not stall
    on every batch the call is also available in two halves: ``enqueue(**batch)`` launches the statistics kernel and
    returns the (6,2) batch means as a DEVICE tensor without synchronising, ``resolve(means.cpu())`` finishes on the
    host (evaluate.run_inference reads all batches' means once, at the end)."""

    def __init__(self, name=None, device="cuda", lower_better=False, *args, **kwargs):
        self.name = name if name is not None else type(self).__name__
        self.pick = min if lower_better else max

    def _pit(self, m):
        return self.pick(float((m[0] + m[3]) / 2), float((m[1] + m[2]) / 2))

    def enqueue(self, s1_pred, s2_pred, s1, s2, mix=None, **batch) -> torch.Tensor:
        stats = _engine(s1_pred.device).sisnr_pairs(s1_pred, s2_pred, s1, s2, s1_pred if mix is None else mix)
        return stats.double().mean(0)

    def resolve(self, means: torch.Tensor):
        return self._pit(means[:, 0])

    def __call__(self, s1_pred, s2_pred, s1, s2, mix=None, **batch):
        return self.resolve(self.enqueue(s1_pred, s2_pred, s1, s2, mix).cpu())


class SISNRiMetric(SISNRMetric):
    def resolve(self, means: torch.Tensor):
        m = means[:, 0]
        return torch.tensor(self._pit(m) - float((m[4] + m[5]) / 2))   # 0-dim tensor like the reference (float - tensor)

    def __call__(self, s1_pred, s2_pred, s1, s2, mix, **batch):
        return self.resolve(self.enqueue(s1_pred, s2_pred, s1, s2, mix).cpu())


_STOI_HANDLES: Dict[tuple, int] = {}                 # (device, fs, extended) -> wavmetric_stoi handle (kept for the process)


def _pair_device(ts):
    dev = ts[0].device
    return dev if dev.index is not None else torch.device("cuda", torch.cuda.current_device())


def sisdr_pairs(s1_pred, s2_pred, s1, s2) -> torch.Tensor:
    """wavmetric_sisdr_pairs (include/wavmetric.h) on the inputs' device and the current stream -> [B, 4] device tensor, the
    SI-SDR in dB of the pairs (p1,s1) (p1,s2) (p2,s1) (p2,s2); no synchronisation."""
    from . import _lib
    ts = _wav_inputs(s1_pred, s2_pred, s1, s2)
    lib = _lib.load()
    B, T = ts[0].shape
    dev = _pair_device(ts)
    with torch.cuda.device(dev):
        out = torch.empty(B, 4, dtype=torch.float32, device=dev)
        rc = lib.wavmetric_sisdr_pairs(*[t.data_ptr() for t in ts], B, T, out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise RuntimeError(f"wavmetric_sisdr_pairs(B={B}, T={T}): {lib.wavmetric_strerror(rc).decode()}")
    return out


def stoi_pairs(s1_pred, s2_pred, s1, s2, fs: int = 16000, extended: bool = False):
    """wavmetric_stoi_pairs (include/wavmetric.h) on the inputs' device and the current stream
    -> ([B, 4] STOI (ESTOI if `extended`) of the pairs (p1,s1) (p1,s2) (p2,s1) (p2,s2), [B, 2] int32 frames kept under
    target s1 / s2); both on the device, no synchronisation; scratch and outputs come from torch's allocator."""
    import ctypes
    from . import _lib
    ts = _wav_inputs(s1_pred, s2_pred, s1, s2)
    lib = _lib.load()
    B, T = ts[0].shape
    dev = _pair_device(ts)
    key = (dev, int(fs), bool(extended))
    with torch.cuda.device(dev):
        if key not in _STOI_HANDLES:
            h = ctypes.c_void_p()
            rc = lib.wavmetric_stoi_create(int(fs), int(bool(extended)), ctypes.byref(h))
            if rc:
                raise (ValueError if rc == 1 else RuntimeError)(f"wavmetric_stoi_create(fs={fs}): {lib.wavmetric_strerror(rc).decode()}")
            _STOI_HANDLES[key] = h.value
        h = _STOI_HANDLES[key]
        out = torch.empty(B, 4, dtype=torch.float32, device=dev)
        kept = torch.empty(B, 2, dtype=torch.int32, device=dev)
        ws = torch.empty(int(lib.wavmetric_stoi_scratch_bytes(h, max(B, 1), max(T, 1))), dtype=torch.uint8, device=dev)
        rc = lib.wavmetric_stoi_pairs(h, *[t.data_ptr() for t in ts], B, T, out.data_ptr(), kept.data_ptr(), ws.data_ptr(), ws.numel(),
                                      torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise RuntimeError(f"wavmetric_stoi_pairs(fs={fs}, B={B}, T={T}): {lib.wavmetric_strerror(rc).decode()}")
    return out, kept


class _PairMetric:
    """SS2BaseMetric.forward (src/metrics/base_metric.py) over four per-item pair values computed on the device: batch
    means, then the batch-level permutation ``pick((m11 + m22) / 2, (m12 + m21) / 2)``.  ``metric(**batch)`` returns a
    Python float as the reference does (one device->host copy); ``enqueue(**batch)`` launches and returns the four batch
    means as a DEVICE tensor without synchronising, ``resolve(means.cpu())`` finishes on the host
    (evaluate.run_inference reads all batches' means once, at the end)."""

    def __init__(self, name=None, device="cuda", lower_better=False, *args, **kwargs):
        self.name = name if name is not None else type(self).__name__
        self.pick = min if lower_better else max

    def pairs(self, s1_pred, s2_pred, s1, s2) -> torch.Tensor:
        raise NotImplementedError

    def enqueue(self, s1_pred, s2_pred, s1, s2, **batch) -> torch.Tensor:
        return self.pairs(s1_pred, s2_pred, s1, s2).double().mean(0)

    def resolve(self, means: torch.Tensor) -> float:
        m = means
        return self.pick(float((m[0] + m[3]) / 2), float((m[1] + m[2]) / 2))

    def __call__(self, s1_pred, s2_pred, s1, s2, **batch):
        return self.resolve(self.enqueue(s1_pred, s2_pred, s1, s2).cpu())


class SISDRMetric(_PairMetric):
    """The reference's SISDRMetric (src/metrics/si_sdr.py): torchmetrics' ScaleInvariantSignalDistortionRatio() defaults
    (no mean removal), one launch."""

    def pairs(self, s1_pred, s2_pred, s1, s2):
        return sisdr_pairs(s1_pred, s2_pred, s1, s2)


class STOIMetric(_PairMetric):
    """The reference's STOIMetric (src/metrics/stoi.py): STOI, or ESTOI with ``extended=True``, of signals sampled at
    ``fs`` = 8000, 10000 or 16000 Hz, in three or four launches instead of four pystoi calls per item on the host.  The
    definition is the project's fp64 restatement of pystoi's algorithm.  ``self.last_kept`` keeps
    the latest call's [B, 2] device tensor of frames kept under each target."""

    def __init__(self, fs=16000, extended=False, name=None, device="cuda", lower_better=False, *args, **kwargs):
        super().__init__(name, device, lower_better, *args, **kwargs)
        if int(fs) not in (8000, 10000, 16000):
            raise ValueError(f"fs must be 8000, 10000 or 16000, got {fs!r}")
        self.fs, self.extended = int(fs), bool(extended)
        self.last_kept = None

    def pairs(self, s1_pred, s2_pred, s1, s2):
        out, self.last_kept = stoi_pairs(s1_pred, s2_pred, s1, s2, self.fs, self.extended)
        return out
