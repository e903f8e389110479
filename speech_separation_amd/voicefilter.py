"""VoiceFilter on libdptnav (include/vfilt.h): the mixture's magnitude spectrogram and one lip-embedding sequence per speaker
-> one masked spectrogram per speaker.  Replaces the reference's VoiceFilter (src/model/voicefilter.py) in eval mode and
its dataset's get_magnitude (src/datasets/base_dataset.py:167-180); TrainableVoiceFilter adds the training step
(include/vfilt_train.h).  The two waveform ends
(include/vfwave.h): voicefilter_analysis, voicefilter_waveforms, VoiceFilter.separate, VoiceFilterSeparator.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Dict, List, Mapping, Optional, Tuple

import torch
import torch.nn as nn

from .engine import ConvTasNetTrainEngine, DptnEngine, _ConvTasNetEngineBase

EMBED_SIZES = (512, 1024)
MAX_INPUT_SIZE = 257
_HIDDEN, _FC = 400, 600
# the lip reader's test-time preprocessing (src/lipreader/lipreading/dataloaders.py:13-29)
VIDEO_CROP, VIDEO_MEAN, VIDEO_STD = (88, 88), 0.421, 0.165
# (index of the Conv2d in the reference's nn.Sequential, index of its BatchNorm2d, out, in, kernel rows, kernel columns)
_CNN = ((1, 2, 64, 1, 1, 7), (5, 6, 64, 64, 7, 1), (9, 10, 64, 64, 5, 5), (13, 14, 64, 64, 5, 5), (17, 18, 64, 64, 5, 5),
        (21, 22, 64, 64, 5, 5), (25, 26, 64, 64, 5, 5), (28, 29, 8, 64, 1, 1))


def voicefilter_state_dict_spec(input_size: int, embed_size: int = 1024) -> List[Tuple[str, Tuple[int, ...], str]]:
    """[(key, shape, kind)] of VoiceFilter.state_dict() without the lip reader: the reference's 82 keys in its order.
    kind: "param", "buffer" (running_mean / running_var) or "count" (the int64 num_batches_tracked)."""
    F, E = int(input_size), int(embed_size)
    spec = []
    for layer in range(2):
        for suffix in ("", "_reverse"):
            s = f"_l{layer}{suffix}"
            spec += [(f"gru.weight_ih{s}", (3 * F, E if layer == 0 else 2 * F), "param"), (f"gru.weight_hh{s}", (3 * F, F), "param"),
                     (f"gru.bias_ih{s}", (3 * F,), "param"), (f"gru.bias_hh{s}", (3 * F,), "param")]
    spec += [("fc_dvector.weight", (F, 2 * F), "param"), ("fc_dvector.bias", (F,), "param")]
    for ci, bi, cout, cin, kh, kw in _CNN:
        spec += [(f"cnn_layers.{ci}.weight", (cout, cin, kh, kw), "param"), (f"cnn_layers.{ci}.bias", (cout,), "param"),
                 (f"cnn_layers.{bi}.weight", (cout,), "param"), (f"cnn_layers.{bi}.bias", (cout,), "param"),
                 (f"cnn_layers.{bi}.running_mean", (cout,), "buffer"), (f"cnn_layers.{bi}.running_var", (cout,), "buffer"),
                 (f"cnn_layers.{bi}.num_batches_tracked", (), "count")]
    spec += [("lstm.weight_ih_l0", (4 * _HIDDEN, 9 * F), "param"), ("lstm.weight_hh_l0", (4 * _HIDDEN, _HIDDEN), "param"),
             ("lstm.bias_ih_l0", (4 * _HIDDEN,), "param"), ("lstm.bias_hh_l0", (4 * _HIDDEN,), "param"),
             ("fc.1.weight", (_FC, _HIDDEN), "param"), ("fc.1.bias", (_FC,), "param"),
             ("fc.4.weight", (F, _FC), "param"), ("fc.4.bias", (F,), "param")]
    return spec


def _check_sizes(input_size: int, embed_size: int):
    if not 1 <= int(input_size) <= MAX_INPUT_SIZE:
        raise ValueError(f"input_size must be in [1, {MAX_INPUT_SIZE}], got {input_size}")
    if int(embed_size) not in EMBED_SIZES:
        raise ValueError(f"embed_size must be one of {EMBED_SIZES}, got {embed_size}")


class VoiceFilterEngine(_ConvTasNetEngineBase):
    """The VoiceFilter separator's forward (include/vfilt.h).  Same conventions as the other engines: borrowed weights
    (bind / bound_to), a cached workspace taken through the optional `alloc` hook, work on the caller's current stream.
    The library derives its weight copies in every forward, so nothing bound goes stale.  Of the base class only the
    handle, binding and workspace duties apply: this ABI counts cost per item of (W, Tv)."""

    def __init__(self, input_size: int, embed_size: int = 1024, device: torch.device | str = "cuda:0", alloc=None):
        _check_sizes(input_size, embed_size)
        self.input_size, self.embed_size = int(input_size), int(embed_size)
        spec = [(k, s) for k, s, kind in voicefilter_state_dict_spec(input_size, embed_size) if kind != "count"]
        super().__init__("vfilt", "VoiceFilter", spec, device, alloc, self.input_size, self.embed_size)
        for i, (k, s) in enumerate(spec):
            if int(self.lib.vfilt_weight_numel(self._h, i)) != math.prod(s):
                raise RuntimeError(f"libdptnav's VoiceFilter disagrees on the size of {k}")

    def workspace_bytes(self, B: int, W: int, Tv: int) -> int:
        n = int(self.lib.vfilt_workspace_bytes(self._h, B, W, Tv))
        if n == 0:
            raise RuntimeError(f"unsupported shape: {self.lib.vfilt_last_error(self._h).decode()}")
        return n

    def flops_per_item(self, W: int, Tv: int) -> float:
        return float(self.lib.vfilt_flops_per_item(self._h, W, Tv))

    def min_bytes_per_item(self, W: int, Tv: int) -> float:
        return float(self.lib.vfilt_min_bytes_per_item(self._h, W, Tv))

    def _input(self, t, name, shape):
        if not isinstance(t, torch.Tensor):
            raise TypeError(f"{name}: expected a torch.Tensor, got {type(t).__name__}")
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected {tuple(shape)}, got {tuple(t.shape)}")
        if t.device != self.device:
            raise ValueError(f"{name}: lives on {t.device}, engine is on {self.device}")
        if t.dtype != torch.float32:
            raise TypeError(f"{name}: expected float32, got {t.dtype}")
        return t.detach().contiguous()

    def forward(self, mix_magnitude: torch.Tensor, s1_embedding: torch.Tensor, s2_embedding: torch.Tensor,
                out: Optional[Tuple[torch.Tensor, torch.Tensor]] = None, ws: Optional[torch.Tensor] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
        """mix_magnitude (B, F, W), s1/s2_embedding (B, Tv, E) -> (s1_spec_pred, s2_spec_pred), each (B, F, W), enqueued on
        the current stream.  `out` / `ws`: caller-provided results and workspace (workspace_bytes(B, W, Tv) bytes, uint8,
        256-byte aligned)."""
        if not isinstance(mix_magnitude, torch.Tensor) or mix_magnitude.dim() != 3:
            raise ValueError("mix_magnitude: expected a (B, F, W) tensor")
        if not isinstance(s1_embedding, torch.Tensor) or s1_embedding.dim() != 3:
            raise ValueError("s1_embedding: expected a (B, Tv, E) tensor")
        B, F, W = (int(d) for d in mix_magnitude.shape)
        Tv = int(s1_embedding.shape[1])
        if F != self.input_size:
            raise ValueError(f"mix_magnitude: expected {self.input_size} frequency bins, got {F}")
        mix = self._input(mix_magnitude, "mix_magnitude", (B, F, W))
        e1 = self._input(s1_embedding, "s1_embedding", (B, Tv, self.embed_size))
        e2 = self._input(s2_embedding, "s2_embedding", (B, Tv, self.embed_size))
        self._need_bound("forward")
        need = self.workspace_bytes(B, W, Tv)
        if ws is None:
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = self._alloc(need)
            ws = self._ws
        else:
            DptnEngine._check_ws(self, ws, need)
        if out is None:
            o1, o2 = self._empty(B, F, W), self._empty(B, F, W)
        else:
            o1, o2 = out
            for o in (o1, o2):
                if (tuple(o.shape) != (B, F, W) or o.dtype != torch.float32 or o.device != self.device
                        or not o.is_contiguous()):
                    raise ValueError(f"out: expected two contiguous float32 ({B},{F},{W}) tensors on {self.device}")
        rc = self.lib.vfilt_forward(self._h, mix.data_ptr(), e1.data_ptr(), e2.data_ptr(), B, W, Tv, o1.data_ptr(), o2.data_ptr(),
                                    ws.data_ptr(), ws.numel(), self._stream())
        if rc:
            self._raise(rc, "vfilt_forward")
        return o1, o2


class _Node(nn.Module):
    """Container that only names a level of the state_dict keys."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("not callable: VoiceFilter runs on libdptnav")


class VoiceFilter(nn.Module):
    """The reference's VoiceFilter (src/model/voicefilter.py): same constructor arguments, same state_dict keys / shapes /
    order, so the separator's 82 entries of its checkpoints load with strict=True (an attached lip reader adds its own
    entries under `lipreader.`, in front, as in the reference: with the reference's lrw_snv1x_tcn1x.json that is this
    package's ShuffleNetLipreading, 1024 wide; of a reference checkpoint only its lipreader.tcn.* entries have no place).
    forward runs on libdptnav (include/vfilt.h) in eval mode; training (Dropout2d, BatchNorm statistics) is not built and
    raises.  `embed_size` is the lip embedding's width: 1024 in the reference (its ShuffleNet lip reader); this package's
    ResNet-18 lip reader gives 512.
    `lipreader`: a module mapping (S, 1, T, H, W) to (S, T, embed_size); otherwise init_lipreader(lipreader_config,
    lipreader_path) of this package when a config is given; otherwise none, and only forward_embeddings works."""

    def __init__(self, input_size: int, lipreader_path: Optional[str] = None, lipreader_config: Optional[str] = None, *,
                 embed_size: int = 1024, lipreader: Optional[nn.Module] = None):
        super().__init__()
        _check_sizes(input_size, embed_size)
        self.input_size, self.embed_size = int(input_size), int(embed_size)
        if lipreader is None and lipreader_config is not None:
            from .lipreader import init_lipreader
            lipreader = init_lipreader(lipreader_config, lipreader_path)
        if lipreader is not None:
            if getattr(lipreader, "backend_out", self.embed_size) != self.embed_size:
                raise ValueError(f"the lip reader gives {lipreader.backend_out} values per frame: construct VoiceFilter with "
                                 f"embed_size={lipreader.backend_out}")
            self.lipreader = lipreader
            for p in self.lipreader.parameters():
                p.requires_grad = False
            self.lipreader.eval()
        else:
            self.lipreader = None
        self._spec = voicefilter_state_dict_spec(self.input_size, self.embed_size)
        for key, shape, kind in self._spec:
            parts = key.split(".")
            node = self
            for name in parts[:-1]:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            if kind == "param":
                node.register_parameter(parts[-1], nn.Parameter(torch.empty(*shape)))
            elif kind == "buffer":
                node.register_buffer(parts[-1], torch.empty(*shape))
            else:
                node.register_buffer(parts[-1], torch.zeros((), dtype=torch.long))
        self.reset_parameters()
        self._engine: Optional[VoiceFilterEngine] = None

    def reset_parameters(self):
        """PyTorch's defaults for the reference's layers: GRU / LSTM U(+-1/sqrt(hidden)), Linear and Conv2d U(+-1/sqrt(fan_in)),
        BatchNorm weight 1, bias 0, running statistics 0 / 1."""
        with torch.no_grad():
            for key, shape, kind in self._spec:
                t = self._tensor(key)
                if kind == "count" or key.endswith("running_mean"):
                    t.zero_()
                elif key.endswith("running_var"):
                    t.fill_(1.0)
                elif key.startswith("gru."):
                    t.uniform_(-1.0, 1.0).mul_(1.0 / math.sqrt(self.input_size))
                elif key.startswith("lstm."):
                    t.uniform_(-1.0, 1.0).mul_(1.0 / math.sqrt(_HIDDEN))
                elif len(shape) > 1:
                    t.uniform_(-1.0, 1.0).mul_(1.0 / math.sqrt(math.prod(shape[1:])))
                elif key.startswith("cnn_layers.") and int(key.split(".")[1]) in [b for _, b, *_ in _CNN]:
                    t.fill_(1.0) if key.endswith("weight") else t.zero_()
                else:    # bias of a Linear / Conv2d: the bound of its weight
                    w = self._tensor(key[:-4] + "weight")
                    t.uniform_(-1.0, 1.0).mul_(1.0 / math.sqrt(math.prod(w.shape[1:])))

    def _tensor(self, key: str) -> torch.Tensor:
        node = self
        for name in key.split("."):
            node = getattr(node, name)
        return node

    def _float_tensors(self) -> Dict[str, torch.Tensor]:
        return {key: self._tensor(key) for key, _, kind in self._spec if kind != "count"}

    def train(self, mode: bool = True):
        """The lip reader stays in eval mode.  Returns self (the reference's override returns None)."""
        super().train(mode)
        if self.lipreader is not None:
            self.lipreader.eval()
        return self

    def _get_engine(self, device: torch.device) -> VoiceFilterEngine:
        if device.type != "cuda":
            raise RuntimeError(f"VoiceFilter computes only on an AMD GPU through libdptnav (got a {device} tensor); there is no "
                               f"CPU/PyTorch fallback")
        eng = self._engine
        if eng is None or eng.device != device:
            eng = self._engine = VoiceFilterEngine(self.input_size, self.embed_size, device)
        tensors = self._float_tensors()
        for k, t in tensors.items():
            if t.device != device:
                raise RuntimeError(f"{k} is on {t.device} but the input is on {device}: call model.to(device)")
        if not eng.bound_to(tensors):
            eng.bind(tensors)
        return eng

    def _need_eval(self):
        if self.training:
            raise RuntimeError("VoiceFilter: the training step (Dropout2d, BatchNorm batch statistics, backward) is not built; "
                               "call model.eval() for inference")

    def forward_embeddings(self, mix_magnitude, s1_embedding, s2_embedding, out=None, ws=None):
        """The separator alone: mix_magnitude (B, F, W), s1/s2_embedding (B, Tv, embed_size) -> {"s1_spec_pred", "s2_spec_pred"},
        each (B, F, W), without grad."""
        self._need_eval()
        s1, s2 = self._get_engine(mix_magnitude.device).forward(mix_magnitude, s1_embedding, s2_embedding, out=out, ws=ws)
        return {"s1_spec_pred": s1, "s2_spec_pred": s2}

    def _embed(self, video: torch.Tensor) -> torch.Tensor:
        """(S, Tv, H, W) raw mouth frames in [0, 255] -> (S, Tv, embed_size): the reference's test-time pipeline
        (get_preprocessing_pipelines("video")["test"]: x / 255, CenterCrop(88, 88), (x - 0.421) / 0.165) and the lip reader.
        This package's Lipreading takes crop and affine inside its stem's load (forward_window: no cropped or normalised
        copy); any other module gets the preprocessed tensor as (S, 1, Tv, 88, 88)."""
        S, Tv, H, W = (int(d) for d in video.shape)
        th, tw = VIDEO_CROP
        if H < th or W < tw:
            raise ValueError(f"s1_video / s2_video: {H} x {W} frames are smaller than the {th} x {tw} centre crop")
        y0, x0 = (H - th) // 2, (W - tw) // 2
        with torch.no_grad():
            if hasattr(self.lipreader, "forward_window"):
                return self.lipreader.forward_window(video, (y0, x0, th, tw), (1.0 / (255.0 * VIDEO_STD), -VIDEO_MEAN / VIDEO_STD))
            x = ((video / 255.0)[:, :, y0:y0 + th, x0:x0 + tw] - VIDEO_MEAN) / VIDEO_STD
            return self.lipreader(x.unsqueeze(1).contiguous(), lengths=[Tv] * S)

    def forward(self, mix_magnitude, s1_video, s2_video, **batch):
        """mix_magnitude (B, F, W); s1/s2_video (B, Tv, H, W'): RAW mouth frames in [0, 255], at least 88 x 88, as the
        reference's datasets deliver them.  As in the reference, every video goes through the lip reader's test-time
        pipeline (x / 255, centre crop to 88 x 88, (x - 0.421) / 0.165) before the lip reader; both speakers share one
        lip-reader call.  For clips that are already cropped and normalised, compute the embeddings yourself and call
        forward_embeddings."""
        self._need_eval()
        if self.lipreader is None:
            raise RuntimeError(f"VoiceFilter was built without a lip reader (embed_size={self.embed_size}): pass lipreader= or "
                               f"lipreader_config= (a ShuffleNet config gives 1024 values per frame, a ResNet-18 one needs embed_size=512), or call "
                               f"forward_embeddings(mix_magnitude, s1_embedding, s2_embedding) with precomputed embeddings")
        if s1_video.dim() != 4 or s1_video.shape != s2_video.shape:
            raise ValueError(f"s1_video / s2_video: expected two (B,Tv,H,W), got {tuple(s1_video.shape)} and {tuple(s2_video.shape)}")
        B = int(s1_video.shape[0])
        emb = self._embed(torch.cat([s1_video, s2_video], dim=0).float())
        return self.forward_embeddings(mix_magnitude, emb[:B], emb[B:])

    def _separate(self, mix, s1_embedding, s2_embedding, hop_length):
        self._need_eval()
        n_fft = 2 * (self.input_size - 1)
        hop = n_fft // 4 if hop_length is None else int(hop_length)
        if not isinstance(mix, torch.Tensor) or mix.dim() not in (2, 3) or (mix.dim() == 3 and mix.shape[1] != 1):
            raise ValueError("mix: expected a (B, T) or (B, 1, T) tensor")
        wav = mix.detach().reshape(mix.shape[0], mix.shape[-1])
        spec, phasor = voicefilter_analysis(wav, n_fft, hop)
        B, F, W = spec.shape
        stack = torch.empty(2, B, F, W, dtype=torch.float32, device=spec.device)       # both masks' results, one synthesis launch
        out = self.forward_embeddings(spec, s1_embedding, s2_embedding, out=(stack[0], stack[1]))
        y = voicefilter_waveforms(stack, phasor, wav.shape[1], n_fft, hop)
        out.update(s1_pred=y[0].view(mix.shape), s2_pred=y[1].view(mix.shape), mix_magnitude=spec)
        return out

    def separate_embeddings(self, mix, s1_embedding, s2_embedding, hop_length=None):
        """forward_embeddings between the two waveform ends (include/vfwave.h): mix (B, T) or (B, 1, T) waveforms,
        s1/s2_embedding (B, Tv, embed_size) -> {"s1_spec_pred", "s2_spec_pred" (B, F, W), "s1_pred", "s2_pred" (the shape of
        mix), "mix_magnitude" (B, F, W)}.  n_fft is 2 (input_size - 1), hop_length defaults to n_fft / 4 (the reference's
        400 / 100).  Three parts -- voicefilter_analysis, the separator, voicefilter_waveforms -- enqueued back to back on the
        current stream: no host synchronisation and no torch operator between them.  The waveforms carry the convention's
        two clamps (voicefilter_waveforms)."""
        return self._separate(mix, s1_embedding, s2_embedding, hop_length)

    def separate(self, mix, s1_video, s2_video, hop_length=None, **batch):
        """separate_embeddings with the lip reader in front, as forward: s1/s2_video (B, Tv, H, W') raw mouth frames."""
        self._need_eval()
        if self.lipreader is None:
            raise RuntimeError("VoiceFilter was built without a lip reader: call separate_embeddings(mix, s1_embedding, s2_embedding)")
        if s1_video.dim() != 4 or s1_video.shape != s2_video.shape:
            raise ValueError(f"s1_video / s2_video: expected two (B,Tv,H,W), got {tuple(s1_video.shape)} and {tuple(s2_video.shape)}")
        B = int(s1_video.shape[0])
        emb = self._embed(torch.cat([s1_video, s2_video], dim=0).float())
        return self._separate(mix, emb[:B], emb[B:], hop_length)


class VoiceFilterTrainEngine(ConvTasNetTrainEngine):
    """The VoiceFilter training step (include/vfilt_train.h), the counterpart of ConvTasNetTrainEngine: borrowed weights,
    gradient buffers the library writes as views of ONE flat tensor (bind_grads), train_forward -> tape, train_backward, and
    the clip / AdamW step over the flat layout.  Shapes are (B, W, Tv).  The 16 running-statistics slots keep their place in
    the flat layout but are never written and never stepped (no_grad_keys)."""

    TAPE_Z, TAPE_ACT, TAPE_LSTM_H, TAPE_FC1, TAPE_DROP, TAPE_GATES, TAPE_STATS, TAPE_CELL = range(8)

    def __init__(self, input_size: int, embed_size: int = 1024, device: torch.device | str = "cuda:0", alloc=None):
        _check_sizes(input_size, embed_size)
        self.input_size, self.embed_size = int(input_size), int(embed_size)
        full = voicefilter_state_dict_spec(input_size, embed_size)
        self.no_grad_keys = frozenset(k for k, _, kind in full if kind == "buffer")
        self._init_train("vftrain", "VoiceFilter training", [(k, s) for k, s, kind in full if kind != "count"], device, alloc,
                         self.input_size, self.embed_size)

    _input = VoiceFilterEngine._input

    def flops_per_item(self, W: int, Tv: int) -> float:
        return float(self.lib.vftrain_flops_per_item(self._h, W, Tv))

    def _inputs(self, mix_magnitude, s1_embedding, s2_embedding):
        if not isinstance(mix_magnitude, torch.Tensor) or mix_magnitude.dim() != 3:
            raise ValueError("mix_magnitude: expected a (B, F, W) tensor")
        if not isinstance(s1_embedding, torch.Tensor) or s1_embedding.dim() != 3:
            raise ValueError("s1_embedding: expected a (B, Tv, E) tensor")
        B, F, W = (int(d) for d in mix_magnitude.shape)
        Tv = int(s1_embedding.shape[1])
        if F != self.input_size:
            raise ValueError(f"mix_magnitude: expected {self.input_size} frequency bins, got {F}")
        return (self._input(mix_magnitude, "mix_magnitude", (B, F, W)), self._input(s1_embedding, "s1_embedding", (B, Tv, self.embed_size)),
                self._input(s2_embedding, "s2_embedding", (B, Tv, self.embed_size)), B, F, W, Tv)

    def train_forward(self, mix_magnitude, s1_embedding, s2_embedding, dropout_ppm: int = 350000, dropout_seed: int = 0):
        """mix_magnitude (B, F, W), s1/s2_embedding (B, Tv, E) -> (s1_spec_pred, s2_spec_pred, tape): the reference's forward
        in training mode; the tape lives in the engine's workspace until the next train_forward."""
        mix, e1, e2, B, F, W, Tv = self._inputs(mix_magnitude, s1_embedding, s2_embedding)
        self._need_bound("train_forward")
        ws = self._workspace(B, W, Tv)
        o1, o2 = self._empty(B, F, W), self._empty(B, F, W)
        rc = self.lib.vftrain_train_forward(self._h, mix.data_ptr(), e1.data_ptr(), e2.data_ptr(), B, W, Tv, int(dropout_ppm),
                                            int(dropout_seed) & 0xFFFFFFFF, o1.data_ptr(), o2.data_ptr(), ws.data_ptr(), ws.numel(),
                                            self._stream())
        if rc:
            self._raise(rc, "vftrain_train_forward")
        self._tape_id += 1
        return o1, o2, (self._tape_id, B, W, ws.data_ptr(), Tv)

    def tape_tensor(self, tape: tuple, which: int, index: int = 0) -> torch.Tensor:
        """A view of what the forward of `tape` stored (vftrain_tape_offset; the shapes are in include/vfilt_train.h).  Valid
        until the next train_forward."""
        tid, B, W, wsp, Tv = tape
        if tid != self._tape_id or self._ws is None or self._ws.data_ptr() != wsp:
            raise RuntimeError("tape_tensor: the tape was overwritten by a later train_forward")
        off = int(self.lib.vftrain_tape_offset(self._h, B, W, Tv, which, index))
        if off < 0:
            self._raise(1, "vftrain_tape_offset")
        F, pos, rows = self.input_size, B * self.input_size * W, 2 * B * W
        shape = {self.TAPE_Z: (B, W, F, 8) if index == 7 else (pos, 64), self.TAPE_ACT: (pos, 64), self.TAPE_LSTM_H: (rows, _HIDDEN),
                 self.TAPE_FC1: (rows, _FC), self.TAPE_DROP: (2 * B, W), self.TAPE_GATES: (rows, 4 * _HIDDEN),
                 self.TAPE_STATS: (8, 2, 64), self.TAPE_CELL: (rows, _HIDDEN)}[which]
        return self._ws[off:off + 4 * math.prod(shape)].view(torch.float32).view(*shape)

    def train_backward(self, mix_magnitude, s1_embedding, s2_embedding, d_out1, d_out2, tape):
        """d loss / d predictions (B, F, W) -> the bound gradient buffers (overwritten), from the tape of train_forward."""
        if self._grads is None:
            raise RuntimeError("VoiceFilterTrainEngine.train_backward: gradients not bound (call bind_grads first)")
        mix, e1, e2, B, F, W, Tv = self._inputs(mix_magnitude, s1_embedding, s2_embedding)
        tid, tB, tW, tws, tTv = tape
        if tid != self._tape_id or (tB, tW, tTv) != (B, W, Tv) or self._ws is None or self._ws.data_ptr() != tws:
            raise RuntimeError("VoiceFilterTrainEngine.train_backward: the tape was overwritten by a later train_forward (one "
                               "backward per forward, in order)")
        d1 = self._input(d_out1, "d_out1", (B, F, W))
        d2 = self._input(d_out2, "d_out2", (B, F, W))
        ws = self._ws
        rc = self.lib.vftrain_train_backward(self._h, mix.data_ptr(), e1.data_ptr(), e2.data_ptr(), B, W, Tv, d1.data_ptr(),
                                             d2.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        if rc:
            self._raise(rc, "vftrain_train_backward")


class _VoiceFilterTrainFn(torch.autograd.Function):
    """The model part of TrainableVoiceFilter's training step, as model._ConvTasNetTrainFn: forward records the tape
    (vftrain_train_forward) and updates the running statistics, backward turns d loss / d predictions into every
    parameter's gradient (vftrain_train_backward) and hands autograd views of one flat copy."""

    @staticmethod
    def forward(ctx, module, mix, e1, e2, *params):
        eng = module._get_engine(mix.device)
        if eng._grads is None:
            eng.bind_grads()
        ppm, seed = module._arm_dropout()
        o1, o2, tape = eng.train_forward(mix, e1, e2, ppm, seed)
        module._update_running(eng.tape_tensor(tape, eng.TAPE_STATS))
        ctx.module, ctx.tape, ctx.inputs = module, tape, (mix, e1, e2)
        return o1, o2

    @staticmethod
    def backward(ctx, d1, d2):
        module = ctx.module
        eng = module._engine
        mix = ctx.inputs[0]
        zeros = lambda g: torch.zeros_like(mix) if g is None else g.contiguous()
        eng.train_backward(*ctx.inputs, zeros(d1), zeros(d2), ctx.tape)
        ctx.tape = None
        # the library's gradient buffers are reused by the next step: autograd gets its own flat copy, whose views become
        # .grad (train.allreduce_gradients and the fused clip / AdamW find it again through `_flat_grad`)
        flat = eng._grads_flat.clone()
        module._flat_grad = flat
        outs = []
        for key, shape, kind in module._spec:
            if kind == "param":
                o = eng._grad_offsets[key]
                outs.append(flat[o:o + math.prod(shape)].view(*shape))
        return (None, None, None, None) + tuple(outs)


class TrainableVoiceFilter(VoiceFilter):
    """VoiceFilter with the training step on libdptnav (include/vfilt_train.h): same constructor, state_dict keys and order,
    initialisation and parameter-count lines, and checkpoints load strictly either way.  In eval mode or under
    torch.no_grad() the forward is VoiceFilter's inference engine (bitwise the same outputs).  In training mode with grad
    enabled it is the reference's training-mode forward -- BatchNorm on the batch's statistics, Dropout2d(0.35) on whole
    frames -- which records a tape, updates the eight running_mean / running_var buffers (momentum 0.1, from a device block,
    no host synchronisation) and num_batches_tracked, and whose backward computes every parameter's gradient in HIP.  The
    lip reader stays frozen and in eval mode; the embeddings get no gradient (one that requires grad is refused).
    `_get_engine` is the training engine, so optim.clip_grad_norm_ / optim.FusedAdamW(weight_decay=0) / train.train_step take
    their fused paths when the model has no lip reader attached (forward_embeddings, or model(**batch) with s1_embedding /
    s2_embedding in the batch); with one, its frozen parameters send them to the stock paths.  torch.optim.Adam and
    torch.nn.utils.clip_grad_norm_ work either way."""

    DROPOUT = 0.35
    MOMENTUM = 0.1

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self._infer_engine: Optional[VoiceFilterEngine] = None
        self._flat_grad: Optional[torch.Tensor] = None
        for key, _, kind in self._spec:
            if kind == "param":
                self._tensor(key)._dptnav_owner = weakref.ref(self)      # lets optim.FusedAdamW / clip_grad_norm_ find the engine

    def _bound(self, attr: str, make, device: torch.device):
        if device.type != "cuda":
            raise RuntimeError(f"VoiceFilter computes only on an AMD GPU through libdptnav (got a {device} tensor); there is no "
                               f"CPU/PyTorch fallback")
        eng = getattr(self, attr)
        if eng is None or eng.device != device:
            eng = make(self.input_size, self.embed_size, device)
            setattr(self, attr, eng)
        tensors = self._float_tensors()
        for k, t in tensors.items():
            if t.device != device:
                raise RuntimeError(f"{k} is on {t.device} but the input is on {device}: call model.to(device)")
        if not eng.bound_to(tensors):
            eng.bind(tensors)
        return eng

    def _get_engine(self, device: torch.device) -> VoiceFilterTrainEngine:
        return self._bound("_engine", VoiceFilterTrainEngine, device)

    def _get_infer_engine(self, device: torch.device) -> VoiceFilterEngine:
        return self._bound("_infer_engine", VoiceFilterEngine, device)

    def _need_eval(self):
        pass

    def _separate(self, mix, s1_embedding, s2_embedding, hop_length):
        if self.training and torch.is_grad_enabled():
            raise RuntimeError("TrainableVoiceFilter: separate / separate_embeddings reconstruct waveforms from the inference "
                               "forward; call model.eval() or use torch.no_grad()")
        return super()._separate(mix, s1_embedding, s2_embedding, hop_length)

    def _arm_dropout(self):
        """A fresh dropout seed per training forward, model._DPTNBase._arm_dropout's scheme: torch's initial seed, a step
        counter and the data-parallel rank (ranks share torch's seed)."""
        self._drop_step = getattr(self, "_drop_step", 0) + 1
        rank = int(os.environ.get("RANK", "0"))
        seed = (torch.initial_seed() * 2654435761 + self._drop_step * 40503 + rank * 0x632BE5AB) & 0x7FFFFFFF
        return int(round(self.DROPOUT * 1e6)), seed

    def _update_running(self, block: torch.Tensor):
        """block: the tape's [8][2][64] batch means and unbiased variances, on the device"""
        with torch.no_grad():
            for l, (_, bi, cout, *_rest) in enumerate(_CNN):
                node = getattr(self.cnn_layers, str(bi))
                node.running_mean.mul_(1.0 - self.MOMENTUM).add_(block[l, 0, :cout], alpha=self.MOMENTUM)
                node.running_var.mul_(1.0 - self.MOMENTUM).add_(block[l, 1, :cout], alpha=self.MOMENTUM)
                node.num_batches_tracked.add_(1)

    def _own_parameters(self):
        return [self._tensor(key) for key, _, kind in self._spec if kind == "param"]

    def forward_embeddings(self, mix_magnitude, s1_embedding, s2_embedding, out=None, ws=None):
        """The separator alone: mix_magnitude (B, F, W), s1/s2_embedding (B, Tv, embed_size) -> {"s1_spec_pred", "s2_spec_pred"}.
        Training mode with grad enabled: the training step (out / ws do not apply); otherwise VoiceFilter's inference."""
        params = self._own_parameters()
        if self.training and torch.is_grad_enabled() and any(p.requires_grad for p in params):
            for name, e in (("s1_embedding", s1_embedding), ("s2_embedding", s2_embedding)):
                if isinstance(e, torch.Tensor) and e.requires_grad:
                    raise NotImplementedError(f"TrainableVoiceFilter: no gradient is computed for {name} (it comes from a frozen "
                                              f"lip-reader): pass it detached")
            if out is not None or ws is not None:
                raise ValueError("TrainableVoiceFilter: out / ws belong to the inference path")
            s1, s2 = _VoiceFilterTrainFn.apply(self, mix_magnitude, s1_embedding, s2_embedding, *params)
        else:
            s1, s2 = self._get_infer_engine(mix_magnitude.device).forward(mix_magnitude, s1_embedding, s2_embedding, out=out, ws=ws)
        return {"s1_spec_pred": s1, "s2_spec_pred": s2}

    def forward(self, mix_magnitude, s1_video=None, s2_video=None, s1_embedding=None, s2_embedding=None, **batch):
        """VoiceFilter.forward; a batch that carries precomputed s1_embedding / s2_embedding skips the lip reader.  They are
        (B, Tv, embed_size), or (B, embed_size, Tv) as make_embeddings stores them and the loader delivers them (transposed
        here, as VoiceFilterSeparator does)."""
        if s1_embedding is not None and s2_embedding is not None:
            E = self.embed_size
            if s1_embedding.dim() == 3 and s1_embedding.shape[2] != E and s1_embedding.shape[1] == E:
                s1_embedding, s2_embedding = s1_embedding.transpose(1, 2), s2_embedding.transpose(1, 2)
            return self.forward_embeddings(mix_magnitude, s1_embedding, s2_embedding)
        if s1_video is None or s2_video is None:
            raise ValueError("TrainableVoiceFilter: the batch has neither s1_embedding / s2_embedding nor s1_video / s2_video")
        return super().forward(mix_magnitude, s1_video, s2_video)


class VoiceFilterSeparator:
    """``model(**batch)`` of evaluate / run_inference for a VoiceFilter: reads ``mix`` and either ``s1_embedding`` /
    ``s2_embedding`` (precomputed; (B, Tv, E), or (B, E, Tv) as make_embeddings stores them and the loader delivers them) or
    ``s1_video`` / ``s2_video``, and returns VoiceFilter.separate's dict, so that the waveform metrics and the prediction
    writer find ``s1_pred`` / ``s2_pred``.  `n_fft` must be the model's 2 (input_size - 1)."""

    def __init__(self, model: "VoiceFilter", n_fft: Optional[int] = None, hop_length: Optional[int] = None):
        want = 2 * (model.input_size - 1)
        if n_fft is not None and int(n_fft) != want:
            raise ValueError(f"n_fft={n_fft} gives {int(n_fft) // 2 + 1} bins, the model takes {model.input_size} (n_fft={want})")
        self.model, self.n_fft = model, want
        self.hop_length = want // 4 if hop_length is None else int(hop_length)
        _check_transform(self.n_fft, self.hop_length)

    def __call__(self, mix, s1_embedding=None, s2_embedding=None, s1_video=None, s2_video=None, **batch):
        if s1_embedding is not None and s2_embedding is not None:
            E = self.model.embed_size
            if s1_embedding.dim() == 3 and s1_embedding.shape[2] != E and s1_embedding.shape[1] == E:
                s1_embedding, s2_embedding = s1_embedding.transpose(1, 2), s2_embedding.transpose(1, 2)
            return self.model.separate_embeddings(mix, s1_embedding, s2_embedding, self.hop_length)
        if s1_video is not None and s2_video is not None:
            return self.model.separate(mix, s1_video, s2_video, self.hop_length)
        raise ValueError("VoiceFilterSeparator: the batch has neither s1_embedding / s2_embedding nor s1_video / s2_video")


def _check_transform(n_fft: int, hop: int):
    from .spectral import _check_sizes as check
    check(int(n_fft), int(hop))


def _vfwave(name: str, dev: torch.device, what: str, *args):
    from . import _lib
    lib = _lib.load()
    with torch.cuda.device(dev):
        rc = getattr(lib, name)(*args, torch.cuda.current_stream(dev).cuda_stream)
    if rc:
        raise (ValueError if rc == 1 else RuntimeError)(f"{name}({what}): {lib.vfwave_strerror(rc).decode()}")


def _fp32(t, who: str, ranks) -> None:
    if not isinstance(t, torch.Tensor):
        raise TypeError(f"{who}: expected a torch.Tensor, got {type(t).__name__}")
    if t.dtype != torch.float32:
        raise TypeError(f"{who}: expected float32, got {t.dtype}")
    if t.dim() not in ranks:
        raise ValueError(f"{who}: expected {' or '.join(str(r) for r in ranks)} dimensions, got {tuple(t.shape)}")


def _on_gpu(t: torch.Tensor, who: str) -> torch.device:
    if t.device.type != "cuda":
        raise RuntimeError(f"{who} computes only on an AMD GPU through libdptnav (got a {t.device} tensor); there is no "
                           f"CPU/PyTorch fallback")
    return t.device


def voicefilter_analysis(audio: torch.Tensor, n_fft: int = 400, hop_length: int = 100):
    """The reference's get_magnitude (src/datasets/base_dataset.py:167-180) in ONE launch (vfwave_analysis): audio (B, T) or
    (T,), T > n_fft / 2 -> (spec, phasor), (B, F, W) and (B, 2, F, W) with F = n_fft // 2 + 1, W = 1 + T // hop_length (no B
    for a 1-D input).  spec = clamp((20 log10(max(|S|, 1e-5)) - 20) / 100, -1, 0) + 1 in [0, 1], phasor = (Re S, Im S) / |S|,
    (1, 0) where S = 0; the reference's phase is atan2(phasor[:, 1], phasor[:, 0]).  spec keeps |S| only inside
    [1e-4, 10]: smaller bins read 0, larger ones 1 (a full-scale tone at n_fft = 400 reaches about 100).  That is the
    reference's convention, and voicefilter_waveforms inverts exactly this range."""
    _fp32(audio, "voicefilter_analysis: audio", (1, 2))
    _check_transform(n_fft, hop_length)
    one = audio.dim() == 1
    x = audio.detach()[None] if one else audio.detach()
    B, T = x.shape
    if T <= n_fft // 2:
        raise ValueError(f"voicefilter_analysis: needs more than n_fft / 2 = {n_fft // 2} samples, got {T}")
    dev = _on_gpu(x, "voicefilter_analysis")
    from .spectral import _handle
    x = x.contiguous()
    F, W = n_fft // 2 + 1, 1 + T // hop_length
    with torch.cuda.device(dev):
        spec = torch.empty(B, F, W, dtype=torch.float32, device=dev)
        phasor = torch.empty(B, 2, F, W, dtype=torch.float32, device=dev)
    if B:
        _vfwave("vfwave_analysis", dev, f"B={B}, T={T}", _handle(dev, n_fft, hop_length), x.data_ptr(), B, T, spec.data_ptr(),
                phasor.data_ptr())
    return (spec[0], phasor[0]) if one else (spec, phasor)


def voicefilter_waveforms(spec_preds, phasor: torch.Tensor, length: Optional[int] = None, n_fft: int = 400, hop_length: int = 100,
                          out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Predicted maps back to audio on the mixture's phase (vfwave_synthesis): spec_preds (n_src, B, F, W) -- or a sequence
    of n_src (B, F, W) tensors --, phasor (B, 2, F, W) from voicefilter_analysis -> (n_src, B, length), `length` defaulting
    to the natural (W - 1) hop_length.  y = istft(10^(5 clamp(p, 0, 1) - 4) (phasor[0] + i phasor[1])), this package's
    STFT.istft: the inverse of voicefilter_analysis's scaling on [1e-4, 10], outside of which the analysis has already
    clamped.  1 <= n_src <= 4.  One launch for a stack (a sequence that is a stack's slices counts as one); otherwise one
    launch per source, each writing its slice of the result: no map is ever copied.  `out`: a contiguous
    (n_src, B, length) result to fill."""
    maps = [spec_preds] if isinstance(spec_preds, torch.Tensor) else list(spec_preds)
    for t in maps:
        _fp32(t, "voicefilter_waveforms: spec_preds", (4,) if isinstance(spec_preds, torch.Tensor) else (3,))
    _fp32(phasor, "voicefilter_waveforms: phasor", (4,))
    _check_transform(n_fft, hop_length)
    n_src = maps[0].shape[0] if isinstance(spec_preds, torch.Tensor) else len(maps)
    if not 1 <= n_src <= 4:
        raise ValueError(f"voicefilter_waveforms: 1 to 4 sources per item, got {n_src}")
    B, two, F, W = phasor.shape
    if two != 2 or F != n_fft // 2 + 1 or W < 1:
        raise ValueError(f"voicefilter_waveforms: phasor must be (B, 2, {n_fft // 2 + 1}, W), got {tuple(phasor.shape)}")
    for t in maps:
        if tuple(t.shape[-3:]) != (B, F, W):
            raise ValueError(f"voicefilter_waveforms: every map must be ({B}, {F}, {W}) as the phasor, got {tuple(t.shape)}")
    L = (W - 1) * hop_length if length is None else int(length)
    if L < 1:
        raise ValueError(f"voicefilter_waveforms: output length {L}; it must be at least 1")
    dev = _on_gpu(phasor, "voicefilter_waveforms")
    if any(t.device != phasor.device for t in maps) or any(not t.is_contiguous() for t in maps + [phasor]):
        raise ValueError("voicefilter_waveforms: the maps and the phasor must be contiguous and on one device")
    if out is None:
        with torch.cuda.device(dev):
            out = torch.empty(n_src, B, L, dtype=torch.float32, device=dev)
    elif tuple(out.shape) != (n_src, B, L) or out.dtype != torch.float32 or out.device != phasor.device or not out.is_contiguous():
        raise ValueError(f"voicefilter_waveforms: out must be a contiguous float32 ({n_src}, {B}, {L}) tensor on {phasor.device}")
    from .spectral import _handle
    step = 4 * B * F * W
    if all(t.data_ptr() == maps[0].data_ptr() + i * step for i, t in enumerate(maps)):
        calls = [(maps[0].data_ptr(), n_src, out.data_ptr())]
    else:
        calls = [(t.data_ptr(), 1, out[i].data_ptr()) for i, t in enumerate(maps)]
    if B:
        for src, n, dst in calls:
            _vfwave("vfwave_synthesis", dev, f"n_src={n}, B={B}, W={W}, length={L}", _handle(dev, n_fft, hop_length), src,
                    phasor.data_ptr(), n, B, W, L, dst)
    return out


def add_magnitude_keys(batch: dict, n_fft: int = 400, hop_length: int = 100) -> dict:
    """Fill VoiceFilter's spectrogram keys of a device batch in place, as the reference's dataset would per item on the host
    with get_magnitude: ``mix_magnitude`` and ``mix_phase`` (= atan2 of the phasor) from ``mix``, ``s1_spec_true`` /
    ``s2_spec_true`` from ``s1`` / ``s2``.  A key whose waveform is absent (None or missing) stays absent.  The
    counterpart of spectral.add_spectrogram_keys.  Returns the batch."""
    with torch.no_grad():
        for src, key in (("mix", "mix_magnitude"), ("s1", "s1_spec_true"), ("s2", "s2_spec_true")):
            wav = batch.get(src)
            if wav is None:
                continue
            spec, phasor = voicefilter_analysis(wav.detach().reshape(wav.shape[0], wav.shape[-1]), n_fft, hop_length)
            batch[key] = spec
            if src == "mix":
                batch["mix_phase"] = torch.atan2(phasor[:, 1], phasor[:, 0])
    return batch


def magnitude_from_stft(re: torch.Tensor, im: torch.Tensor):
    """(Re S, Im S) -> (spec, phase) of the reference's get_magnitude: spec = clamp((20 log10(max(|S|, 1e-5)) - 20) / 100,
    -1, 0) + 1, phase = angle(S).  Plain torch operators at the inputs' dtype and device."""
    mag = torch.clamp(torch.sqrt(re * re + im * im), min=1e-5)
    spec = torch.clamp((20.0 * torch.log10(mag) - 20.0) / 100.0, min=-1.0, max=0.0) + 1.0
    return spec, torch.atan2(im, re)


def voicefilter_magnitude(audio: torch.Tensor, n_fft: int = 400, hop_length: int = 100):
    """The reference's get_magnitude (src/datasets/base_dataset.py:167-180) on the device: audio (B, T) or (T,) -> (spec, phase),
    each (B, n_fft // 2 + 1, T // hop_length + 1) (no B for a 1-D input): spec = clamp((20 log10(max(|S|, 1e-5)) - 20) / 100,
    -1, 0) + 1 in [0, 1], phase = angle(S), with S the Hann-window STFT of this package (spectral.STFT)."""
    from .spectral import STFT
    one = audio.dim() == 1
    S = STFT(n_fft, hop_length).stft(audio.detach()[None] if one else audio.detach())     # [B, 2, frames, F]
    spec, phase = (t.contiguous() for t in magnitude_from_stft(S[:, 0].transpose(1, 2), S[:, 1].transpose(1, 2)))
    return (spec[0], phase[0]) if one else (spec, phase)
