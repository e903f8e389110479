"""The lip-reading front ends on libdptnav: mouth video -> per-frame embeddings, the input of the audio-visual separators.
Lipreading is the ResNet-18 lip reader (include/lipfe.h, (S, T, 512)), ShuffleNetLipreading the ShuffleNet-v2 one
(include/lipsn.h, (S, T, 1024): the lip reader of the reference's VoiceFilter).  Replaces the reference's
Lipreading(extract_feats=True) (src/lipreader/lipreading/model.py:141-273), init_lipreader (src/utils/init_utils.py:168-207),
profiler.py's VideoSSModel and make_embeddings.py.  Inference only.
"""
from __future__ import annotations

import ctypes as C
import json
import math
import os
from typing import Dict, List, Mapping, Optional, Sequence, Tuple

import numpy as np
import torch
import torch.nn as nn

from . import _lib
from .engine import DptnEngine, _ConvTasNetEngineBase

RELU_TYPES = {"relu": 0, "prelu": 1, "swish": 2}   # LIPFE_RELU / LIPFE_PRELU / LIPFE_SWISH, and the same of LIPSN_*
_PLANES = (64, 128, 256, 512)
SHUFFLENET_WIDTHS = {0.5: (48, 96, 192), 1.0: (116, 232, 464)}   # width_mult -> stage widths (width_x2 of lipsn_create: 1, 2)
_SN_REPEATS = (4, 8, 4)
_SN_STEM, _SN_EMBED = 24, 1024


def lipreader_state_dict_spec(relu_type: str = "swish") -> List[Tuple[str, Tuple[int, ...], str]]:
    """[(key, shape, kind)] of Lipreading.state_dict(): the reference's keys and order without tcn.*.  kind: "param"
    (float parameter), "buffer" (running_mean / running_var) or "count" (the int64 num_batches_tracked)."""
    if relu_type not in RELU_TYPES:
        raise ValueError(f"relu_type must be one of {sorted(RELU_TYPES)}, got {relu_type!r}")

    def bn(p, C_):
        return [(p + "weight", (C_,), "param"), (p + "bias", (C_,), "param"), (p + "running_mean", (C_,), "buffer"),
                (p + "running_var", (C_,), "buffer"), (p + "num_batches_tracked", (), "count")]

    spec, inp = [], 64
    for li, planes in enumerate(_PLANES):
        for b in range(2):
            p = f"trunk.layer{li + 1}.{b}."
            cin = inp if b == 0 else planes
            spec.append((p + "conv1.weight", (planes, cin, 3, 3), "param"))
            spec += bn(p + "bn1.", planes)
            if relu_type == "prelu":
                spec += [(p + "relu1.weight", (planes,), "param"), (p + "relu2.weight", (planes,), "param")]
            spec.append((p + "conv2.weight", (planes, planes, 3, 3), "param"))
            spec += bn(p + "bn2.", planes)
            if b == 0 and li > 0:
                spec.append((p + "downsample.0.weight", (planes, cin, 1, 1), "param"))
                spec += bn(p + "downsample.1.", planes)
        inp = planes
    spec.append(("frontend3D.0.weight", (64, 1, 5, 7, 7), "param"))
    spec += bn("frontend3D.1.", 64)
    if relu_type == "prelu":
        spec.append(("frontend3D.2.weight", (64,), "param"))
    return spec


def _shufflenet_width(width_mult) -> float:
    try:
        w = float(width_mult)
    except (TypeError, ValueError):
        w = None
    if w not in SHUFFLENET_WIDTHS:
        raise NotImplementedError(f"ShuffleNet lip reader: width_mult={width_mult!r} is not built (0.5 or 1.0; no lip-reader "
                                  f"config of the reference uses 1.5 or 2.0)")
    return w


def shufflenet_state_dict_spec(relu_type: str = "prelu", width_mult: float = 1.0) -> List[Tuple[str, Tuple[int, ...], str]]:
    """[(key, shape, kind)] of the reference's Lipreading(backbone_type="shufflenet").state_dict() without tcn.*: the trunk
    Sequential(features, conv_last, globalpool) is registered before the stem.  kind as lipreader_state_dict_spec."""
    if relu_type not in RELU_TYPES:
        raise ValueError(f"relu_type must be one of {sorted(RELU_TYPES)}, got {relu_type!r}")
    stages = SHUFFLENET_WIDTHS[_shufflenet_width(width_mult)]

    def conv_bn(p, i, shape):
        q = f"{p}{i + 1}."
        C_ = shape[0]
        return [(f"{p}{i}.weight", shape, "param"), (q + "weight", (C_,), "param"), (q + "bias", (C_,), "param"),
                (q + "running_mean", (C_,), "buffer"), (q + "running_var", (C_,), "buffer"), (q + "num_batches_tracked", (), "count")]

    spec, inp, bi = [], _SN_STEM, 0
    for width, repeats in zip(stages, _SN_REPEATS):
        ch = width // 2
        for r in range(repeats):
            p = f"trunk.0.{bi}."
            if r == 0:   # the stride-2 form: both branches read the whole input
                spec += conv_bn(p + "banch1.", 0, (inp, 1, 3, 3)) + conv_bn(p + "banch1.", 2, (ch, inp, 1, 1))
            spec += conv_bn(p + "banch2.", 0, (ch, inp if r == 0 else ch, 1, 1))
            spec += conv_bn(p + "banch2.", 3, (ch, 1, 3, 3)) + conv_bn(p + "banch2.", 5, (ch, ch, 1, 1))
            inp = width
            bi += 1
    spec += conv_bn("trunk.1.", 0, (_SN_EMBED, inp, 1, 1))
    spec += conv_bn("frontend3D.", 0, (_SN_STEM, 1, 5, 7, 7))
    if relu_type == "prelu":
        spec.append(("frontend3D.2.weight", (_SN_STEM,), "param"))
    return spec


class LipreadingEngine(_ConvTasNetEngineBase):
    """The lip-reading front end's forward (include/lipfe.h).  Same conventions as the other engines: borrowed weights
    (bind / bound_to), a cached workspace taken through the optional `alloc` hook, work on the caller's current stream.
    The library derives its weight copies in every forward, so nothing bound goes stale.  Of the base class only the
    handle, binding and workspace duties apply: this ABI has no frame arithmetic and counts cost per stream, not per mixture."""

    embed = 512          # values per frame
    _cost_args = ()      # what <prefix>_flops_per_stream / _min_bytes_per_stream take in front of (T, H, W)

    def __init__(self, device: torch.device | str = "cuda:0", relu_type: str = "swish", alloc=None):
        self.relu_type = relu_type
        spec = [(k, s) for k, s, kind in lipreader_state_dict_spec(relu_type) if kind != "count"]
        self._create("lipfe", "lip-reading front end", spec, device, alloc, RELU_TYPES[relu_type])

    def _create(self, prefix, what, spec, device, alloc, *create_args):
        _ConvTasNetEngineBase.__init__(self, prefix, what, spec, device, alloc, *create_args)
        for i, (k, s) in enumerate(spec):
            if int(self._fn("weight_numel")(self._h, i)) != math.prod(s):
                raise RuntimeError(f"libdptnav's {what} disagrees on the size of {k}")

    def workspace_bytes(self, S: int, T: int, H: int, W: int) -> int:
        n = int(self._fn("workspace_bytes")(self._h, S, T, H, W))
        if n == 0:
            raise RuntimeError(f"unsupported shape: {self._fn('last_error')(self._h).decode()}")
        return n

    def weight_pack_bytes(self) -> int:
        return int(self._fn("weight_pack_bytes")(self._h))

    def flops_per_stream(self, T: int, H: int, W: int) -> float:
        return float(self._fn("flops_per_stream")(*self._cost_args, T, H, W))

    def min_bytes_per_stream(self, T: int, H: int, W: int) -> float:
        return float(self._fn("min_bytes_per_stream")(*self._cost_args, T, H, W))

    def forward(self, x: torch.Tensor, window: Optional[Tuple[int, int, int, int]] = None,
                affine: Tuple[float, float] = (1.0, 0.0), out: Optional[torch.Tensor] = None,
                ws: Optional[torch.Tensor] = None) -> torch.Tensor:
        """x (S, 1, T, Hin, Win) or (S, T, Hin, Win) -> (S, T, embed), enqueued on the current stream.  window = (y0, x0, H, W)
        inside the Hin x Win frame (default: all of it); affine = (a, b): the network sees a * x + b.  `out` / `ws`:
        caller-provided result and workspace (workspace_bytes(S, T, H, W) bytes, uint8, 256-byte aligned)."""
        if not isinstance(x, torch.Tensor):
            raise TypeError(f"x: expected a torch.Tensor, got {type(x).__name__}")
        if x.dim() == 5 and x.shape[1] == 1:
            x = x[:, 0]
        if x.dim() != 4:
            raise ValueError(f"x: expected (S,1,T,H,W) or (S,T,H,W), got {tuple(x.shape)}")
        if x.device != self.device:
            raise ValueError(f"x: lives on {x.device}, engine is on {self.device}")
        if x.dtype != torch.float32:
            raise TypeError(f"x: expected float32, got {x.dtype}")
        x = x.contiguous()
        S, T, Hin, Win = (int(d) for d in x.shape)
        y0, x0, H, W = (0, 0, Hin, Win) if window is None else (int(v) for v in window)
        self._need_bound("forward")
        need = self.workspace_bytes(S, T, H, W)
        if ws is None:
            if self._ws is None or self._ws.numel() < need:
                self._ws = None
                self._ws = self._alloc(need)
            ws = self._ws
        else:
            DptnEngine._check_ws(self, ws, need)
        E = self.embed
        if out is None:
            out = self._empty(S, T, E)
        elif (tuple(out.shape) != (S, T, E) or out.dtype != torch.float32 or out.device != self.device
              or not out.is_contiguous()):
            raise ValueError(f"out: expected a contiguous float32 ({S},{T},{E}) tensor on {self.device}")
        rc = self._fn("forward")(self._h, x.data_ptr(), S, T, Hin, Win, y0, x0, H, W, float(affine[0]), float(affine[1]),
                                 out.data_ptr(), ws.data_ptr(), ws.numel(), self._stream())
        if rc:
            self._raise(rc, f"{self._prefix}_forward")
        return out


class ShuffleNetLipreadingEngine(LipreadingEngine):
    """The ShuffleNet-v2 lip reader's forward (include/lipsn.h): x -> (S, T, 1024) for 65 <= H, W <= 160.  Conventions and
    methods as LipreadingEngine; one forward is `launches_per_forward()` kernel launches, one of them per InvertedResidual."""

    embed = _SN_EMBED

    def __init__(self, device: torch.device | str = "cuda:0", relu_type: str = "prelu", width_mult: float = 1.0, alloc=None):
        self.relu_type, self.width_mult = relu_type, _shufflenet_width(width_mult)
        self._cost_args = (int(round(2 * self.width_mult)),)
        spec = [(k, s) for k, s, kind in shufflenet_state_dict_spec(relu_type, self.width_mult) if kind != "count"]
        self._create("lipsn", "ShuffleNet lip reader", spec, device, alloc, RELU_TYPES[relu_type], self._cost_args[0])

    def launches_per_forward(self) -> int:
        return int(self.lib.lipsn_launches_per_forward())


class _Node(nn.Module):
    """Container that only names a level of the state_dict keys."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("not callable: Lipreading runs on libdptnav")


class _LipreaderModule(nn.Module):
    """What the two lip readers share: the reference's state_dict entries as bare tensors (`_build`), its initialisation, and
    a forward on libdptnav through an engine bound to those tensors.  Inference only: train() behaves as eval()."""

    def _build(self, spec):
        self._spec = spec
        for key, shape, kind in self._spec:
            parts = key.split(".")
            node = self
            for name in parts[:-1]:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            if kind == "param":
                node.register_parameter(parts[-1], nn.Parameter(torch.empty(*shape), requires_grad=False))
            elif kind == "buffer":
                node.register_buffer(parts[-1], torch.empty(*shape))
            else:
                node.register_buffer(parts[-1], torch.zeros((), dtype=torch.long))
        self.reset_parameters()
        self._engine: Optional[LipreadingEngine] = None
        self.eval()

    def reset_parameters(self):
        """The reference's _initialize_weights_randomly: conv weights N(0, 2 / (kernel volume * out_channels)), BatchNorm
        weight 1 and bias 0; running statistics 0 / 1; PReLU slopes 0.25."""
        with torch.no_grad():
            for key, shape, kind in self._spec:
                t = self._tensor(key)
                if kind == "count":
                    t.zero_()
                elif len(shape) > 1:
                    t.normal_(0.0, math.sqrt(2.0 / (math.prod(shape[2:]) * shape[0])))
                elif key.endswith(("running_mean", ".bias")):
                    t.zero_()
                elif key.endswith(("relu1.weight", "relu2.weight", "frontend3D.2.weight")):
                    t.fill_(0.25)
                else:
                    t.fill_(1.0)

    def _tensor(self, key: str) -> torch.Tensor:
        node = self
        for name in key.split("."):
            node = getattr(node, name)
        return node

    def _float_tensors(self) -> Dict[str, torch.Tensor]:
        return {key: self._tensor(key) for key, _, kind in self._spec if kind != "count"}

    def train(self, mode: bool = True):
        return super().train(False)

    def _make_engine(self, device: torch.device) -> LipreadingEngine:
        raise NotImplementedError

    def _get_engine(self, device: torch.device) -> LipreadingEngine:
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} computes only on an AMD GPU through libdptnav (got a {device} tensor); "
                               f"there is no CPU/PyTorch fallback")
        eng = self._engine
        if eng is None or eng.device != device:
            eng = self._engine = self._make_engine(device)
        tensors = self._float_tensors()
        for k, t in tensors.items():
            if t.device != device:
                raise RuntimeError(f"{k} is on {t.device} but the input is on {device}: call model.to(device)")
        if not eng.bound_to(tensors):
            eng.bind(tensors)
        return eng

    def forward(self, x, lengths=None, boundaries=None):
        """x (S, 1, T, H, W) -> (S, T, backend_out).  `lengths` is accepted and unused, as in the reference with
        extract_feats=True."""
        return self._get_engine(x.device).forward(x)

    def forward_window(self, x, window, affine=(1.0, 0.0)):
        """x (S, 1, T, Hin, Win) or (S, T, Hin, Win); window = (y0, x0, H, W); the network sees a * x + b on the window: crop
        and normalisation of the reference's test-time pipeline without a copy of the video."""
        return self._get_engine(x.device).forward(x, window=window, affine=affine)


class Lipreading(_LipreaderModule):
    """The reference's Lipreading as a feature extractor (src/lipreader/lipreading/model.py:141-273): same constructor
    keywords, same state_dict keys / shapes / order minus the tcn.* back end, which extract_feats=True never runs and which
    is not built here.  forward runs on libdptnav (include/lipfe.h); inference only: train() behaves as eval() and the
    output carries no grad."""

    def __init__(self, modality="video", hidden_dim=256, backbone_type="resnet", num_classes=500, relu_type="prelu",
                 tcn_options={}, densetcn_options={}, width_mult=1.0, use_boundary=False, extract_feats=False):
        super().__init__()
        if modality != "video":
            raise NotImplementedError(f"Lipreading: modality={modality!r} is not built (only 'video')")
        if backbone_type != "resnet":
            raise NotImplementedError(f"Lipreading: backbone_type={backbone_type!r} is not built (only 'resnet'; "
                                      f"ShuffleNetLipreading is the 'shufflenet' one)")
        if relu_type not in RELU_TYPES:
            raise NotImplementedError(f"Lipreading: relu_type={relu_type!r} is not built (one of {sorted(RELU_TYPES)})")
        if use_boundary:
            raise NotImplementedError("Lipreading: use_boundary=True is not built")
        if not extract_feats:
            raise NotImplementedError("Lipreading: extract_feats=False is not built (the TCN back end); pass extract_feats=True")
        self.modality, self.backbone_type, self.relu_type = modality, backbone_type, relu_type
        self.use_boundary, self.extract_feats = use_boundary, extract_feats
        self.frontend_nout, self.backend_out = 64, 512
        self._build(lipreader_state_dict_spec(relu_type))

    def _make_engine(self, device):
        return LipreadingEngine(device, self.relu_type)


class ShuffleNetLipreading(_LipreaderModule):
    """The reference's Lipreading(backbone_type="shufflenet") as a feature extractor (src/lipreader/lipreading/model.py:141-273,
    models/shufflenetv2.py): the lip reader its VoiceFilter is written for (lrw_snv1x_tcn1x.json).  Same constructor keywords,
    same state_dict keys / shapes / order minus the tcn.* back end, which extract_feats=True never runs.  width_mult 0.5 or
    1.0; relu_type is the stem's activation (the trunk is ReLU).  forward runs on libdptnav (include/lipsn.h) for frames of
    65 .. 160 pixels a side; inference only: train() behaves as eval() and the output carries no grad."""

    def __init__(self, modality="video", hidden_dim=256, backbone_type="shufflenet", num_classes=500, relu_type="prelu",
                 tcn_options={}, densetcn_options={}, width_mult=1.0, use_boundary=False, extract_feats=False):
        super().__init__()
        if modality != "video":
            raise NotImplementedError(f"ShuffleNetLipreading: modality={modality!r} is not built (only 'video')")
        if backbone_type != "shufflenet":
            raise NotImplementedError(f"ShuffleNetLipreading: backbone_type={backbone_type!r} is not built here (only "
                                      f"'shufflenet'; Lipreading is the 'resnet' one)")
        if relu_type not in RELU_TYPES:
            raise NotImplementedError(f"ShuffleNetLipreading: relu_type={relu_type!r} is not built (one of {sorted(RELU_TYPES)})")
        if use_boundary:
            raise NotImplementedError("ShuffleNetLipreading: use_boundary=True is not built")
        if not extract_feats:
            raise NotImplementedError("ShuffleNetLipreading: extract_feats=False is not built (the TCN back end); pass "
                                      "extract_feats=True")
        self.width_mult = _shufflenet_width(width_mult)
        self.modality, self.backbone_type, self.relu_type = modality, backbone_type, relu_type
        self.use_boundary, self.extract_feats = use_boundary, extract_feats
        self.frontend_nout, self.backend_out, self.stage_out_channels = _SN_STEM, _SN_EMBED, _SN_EMBED
        self._build(shufflenet_state_dict_spec(relu_type, self.width_mult))

    def _make_engine(self, device):
        return ShuffleNetLipreadingEngine(device, self.relu_type, self.width_mult)


def init_lipreader(config, path) -> _LipreaderModule:
    """The reference's init_lipreader (src/utils/init_utils.py:168-207): `config` is one of its lip-reader JSON files
    (backbone_type, relu_type, width_mult, ...), `path` a checkpoint with a "model_state_dict" entry, e.g.
    lrw_resnet18_mstcn_video.pth or lrw_snv1x_tcn1x.pth.  backbone_type "resnet" gives a Lipreading, "shufflenet" a
    ShuffleNetLipreading.  As there, entries the model does not have (tcn.*) or has in another shape are left out
    (strict=False)."""
    with open(config) as f:
        args = json.load(f)
    cls = ShuffleNetLipreading if args["backbone_type"] == "shufflenet" else Lipreading
    model = cls(modality="video", num_classes=args.get("num_classes", 500), tcn_options={}, densetcn_options={},
                       backbone_type=args["backbone_type"], relu_type=args["relu_type"], width_mult=args.get("width_mult", 1.0),
                       use_boundary=args.get("use_boundary", False), extract_feats=True)
    if not os.path.isfile(path):
        raise FileNotFoundError(f"lip-reader checkpoint not found: {path}")
    loaded = torch.load(path, map_location="cpu")["model_state_dict"]
    sizes = {k: v.shape for k, v in model.state_dict().items()}
    model.load_state_dict({k: v for k, v in loaded.items() if k in sizes and v.shape == sizes[k]}, strict=False)
    return model


class VideoSSModel(nn.Module):
    """profiler.py's VideoSSModel: lip reader + audio-visual separator in one call.  The batch holds either `video`
    (2B, 1, Tv, H, W) -- the first B rows speaker 1, the next B speaker 2; profiler.py's form at B = 1 -- or `s1_video` /
    `s2_video` (B, Tv, H, W) each.  The lip reader runs once on all 2B streams; the separator gets s1_embedding /
    s2_embedding (B, E, Tv), E the lip reader's width (512 ResNet-18, 1024 ShuffleNet).  Returns the separator's dict with the two embeddings added."""

    def __init__(self, ss: nn.Module, lipreader: nn.Module):
        super().__init__()
        self.ss = ss
        self.lipreader = lipreader
        self.lipreader.eval()

    def forward(self, **batch):
        if "video" in batch:
            video = batch["video"]
            if video.dim() != 5 or video.shape[0] % 2:
                raise ValueError(f"video: expected (2B,1,Tv,H,W), got {tuple(video.shape)}")
        elif "s1_video" in batch and "s2_video" in batch:
            v1, v2 = batch["s1_video"], batch["s2_video"]
            if v1.dim() != 4 or v1.shape != v2.shape:
                raise ValueError(f"s1_video / s2_video: expected two (B,Tv,H,W), got {tuple(v1.shape)} and {tuple(v2.shape)}")
            video = torch.cat([v1, v2], dim=0).unsqueeze(1)
        else:
            raise KeyError("VideoSSModel needs `video` or `s1_video` and `s2_video`")
        B = video.shape[0] // 2
        embed = self.lipreader(video, lengths=[video.shape[2]] * (2 * B)).permute(0, 2, 1)
        batch["s1_embedding"] = embed[:B].contiguous()
        batch["s2_embedding"] = embed[B:].contiguous()
        out = dict(self.ss(**batch))
        out["s1_embedding"], out["s2_embedding"] = batch["s1_embedding"], batch["s2_embedding"]
        return out


def make_embeddings(lipreader: _LipreaderModule, mouths_dir: str, embeds_dir: str, crop: Tuple[int, int] = (88, 88),
                    mean: float = 0.421, std: float = 0.165, streams_per_call: int = 16, device=None) -> List[str]:
    """make_embeddings.py of the reference: every file of `mouths_dir` holds np.load(f)["data"] (T, Hin, Win) in [0, 255];
    its embedding goes to `embeds_dir` under the same name as np.savez_compressed(path, embedding=(backend_out, T) float32), what
    io.load_object and the reference's datasets read.  The test-time pipeline x / 255 -> CenterCrop(crop) -> (x - mean) / std
    is the window and affine of the forward.  Clips of the same shape share a forward (up to `streams_per_call`), and
    each forward's results come back in one device-to-host copy.  Returns the written paths."""
    if device is None:
        device = next(iter(lipreader._float_tensors().values())).device
    device = torch.device(device)
    os.makedirs(embeds_dir, exist_ok=True)
    names = sorted(f for f in os.listdir(mouths_dir) if os.path.isfile(os.path.join(mouths_dir, f)))
    clips: Dict[Tuple[int, ...], List[Tuple[str, np.ndarray]]] = {}
    for name in names:
        with np.load(os.path.join(mouths_dir, name)) as data:
            clip = np.asarray(data["data"], dtype=np.float32)
        if clip.ndim != 3:
            raise ValueError(f"{name}: expected data of shape (T,H,W), got {clip.shape}")
        clips.setdefault(clip.shape, []).append((name, clip))
    a, b = 1.0 / (255.0 * std), -mean / std
    written = []
    for (T, Hin, Win), group in clips.items():
        th, tw = crop
        if Hin < th or Win < tw:
            raise ValueError(f"{group[0][0]}: {Hin} x {Win} frames are smaller than the {th} x {tw} crop")
        window = ((Hin - th) // 2, (Win - tw) // 2, th, tw)
        for i in range(0, len(group), streams_per_call):
            part = group[i:i + streams_per_call]
            x = torch.from_numpy(np.stack([c for _, c in part])).to(device)
            emb = lipreader.forward_window(x, window, (a, b)).permute(0, 2, 1).contiguous().cpu().numpy()
            for (name, _), e in zip(part, emb):
                path = os.path.join(embeds_dir, name)
                np.savez_compressed(path, embedding=e)
                written.append(path if path.endswith(".npz") else path + ".npz")
    return written
