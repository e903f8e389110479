"""Drop-in ``nn.Module``s for the reference's DPTN raw-waveform separators, backed by libdptnav.

Mirrors (does not import) the reference interface for this path:
  * ``DPTNAVWavEncDec(num_features, video_emb_size, hidden_video, kernel_size_enc, hidden_dim, num_blocks,
    chunk_size, step_size, num_heads, dropout, bidir)``            src/model/dptn_wav.py:137-150
  * ``DPTNWavEncDec(num_features, kernel_size_enc, ...)``           src/model/dptn_wav.py:72-83
  * ``DPTNEncDec(num_features, kernel_size_enc, ...)``              src/model/dptn.py:154-165 (masked tail, dptn.py:103-115)
  * ``ConvTasNet(N, L)`` (inference only)                           src/model/convtasnet.py:101-116
  * ``TrainableConvTasNet(N, L)`` (ConvTasNet with the training step) src/model/convtasnet.py:101-116
  * ``DeepConvTasNet(N, L)``, ``DeepAVConvTasNet(N, L, video_emb_size, hidden_video)`` (inference only)
                                                                    src/model/deepconvtasnet.py:122-136, deepavconvtasnet.py:122-156
  * ``TrainableDeepConvTasNet(N, L)`` (DeepConvTasNet with the training step) src/model/deepconvtasnet.py:122-136
  * ``forward(mix, s1_embedding, s2_embedding, **batch) -> {"s1_pred","s2_pred"}``  dptn_wav.py:171,194
    -- called as ``self.model(**batch)`` by src/trainer/trainer.py:40 and inferencer.py:117, so unknown
    batch keys (mix_spectrogram, s1, s2, paths, ...) must be accepted and ignored.
  * ``state_dict()`` keys/shapes == the reference's, so ``model_best.pth`` loads
    through base_trainer.py:539-560 unchanged.
  * ``str(model)`` ends with the two parameter-count lines of dptn_wav.py:196-207.

Select it from the reference's Hydra CLI with ``model._target_=speech_separation_amd.DPTNAVWavEncDec``
(INTEGRATION.md).  The forward AND the backward of the model run ONLY on the HIP library (a torch.autograd.Function
hands autograd the parameter gradients computed by dptnav_train_backward): no PyTorch operators are used for the
model's compute and there is no CPU fallback -- a missing extension or a CPU tensor raises.
"""
from __future__ import annotations

import math
import os
import weakref
from typing import Dict, Optional

import torch
from torch import nn

from .engine import (ConvTasNetEngine, ConvTasNetTrainEngine, DeepAVConvTasNetTrainEngine, DeepConvTasNetEngine,
                     DeepConvTasNetTrainEngine, DptnEngine)
from .spec import DPTNConfig, convtasnet_state_dict_spec, deepconvtasnet_state_dict_spec, state_dict_spec


class _Node(nn.Module):
    """Pure parameter container (never called): gives nested state_dict keys such as
    ``dprnn.model.0.intra_chunk_block.mha.out_proj.weight``."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError("parameter container: compute happens in libdptnav, not in torch")


def _init_like_torch(key: str, p: torch.Tensor, cfg: DPTNConfig) -> None:
    """Default initialisers of the stock modules the reference instantiates (so a from-scratch run
    starts from the same distributions): nn.LSTM U(+-1/sqrt(H)); nn.Linear/Conv kaiming_uniform(a=sqrt 5)
    == U(+-1/sqrt(fan_in)) with the matching bias bound; nn.MultiheadAttention xavier_uniform in_proj,
    zero biases; LayerNorm 1/0; PReLU 0.25; gate ~ N(0,1) (dptn_wav.py:155)."""
    leaf2 = ".".join(key.split(".")[-2:])
    with torch.no_grad():
        if key == "gate":
            p.normal_()
        elif key.endswith("speakers_separation.0.weight"):
            p.fill_(0.25)
        elif ".rnn." in key:
            b = 1.0 / math.sqrt(cfg.hidden_dim)
            p.uniform_(-b, b)
        elif leaf2 in ("ln1.weight", "ln2.weight", "video_ln.weight", "norm1d.weight"):
            p.fill_(1.0)
        elif leaf2 in ("ln1.bias", "ln2.bias", "video_ln.bias", "norm1d.bias", "mha.in_proj_bias", "out_proj.bias"):
            p.zero_()
        elif leaf2 == "mha.in_proj_weight":
            nn.init.xavier_uniform_(p)
        elif key.endswith("weight"):
            fan_in = p[0].numel()
            b = 1.0 / math.sqrt(fan_in)
            p.uniform_(-b, b)
        else:  # biases of Linear / Conv: U(+-1/sqrt(fan_in of the matching weight))
            fan_in = {"visual_compression.bias": cfg.video_emb_size, "ffn.1.bias": None, "fc.bias": None}.get(
                leaf2, cfg.num_features)
            if fan_in is None:
                fan_in = cfg.hidden_dim * (2 if (cfg.bidir or "intra_chunk_block" in key) else 1)
            b = 1.0 / math.sqrt(fan_in)
            p.uniform_(-b, b)


class _SeparateFn(torch.autograd.Function):
    """Model part of the training step: forward records a tape in libdptnav, backward turns d loss / d predictions into
    the gradient of every parameter (dptnav_train_backward).  Loss, clipping and optimizer stay ordinary PyTorch code
    of the caller (the reference's trainer.py:43-51)."""

    @staticmethod
    def forward(ctx, module, mix, e1, e2, *params):
        eng = module._get_engine(mix.device)
        if getattr(eng, "_grads", None) is None:
            eng.bind_grads()
        ppm, seed = module._arm_dropout(eng)
        s1, s2, tape = eng.train_forward(mix, e1, e2)
        ctx.module, ctx.tape, ctx.inputs, ctx.drop = module, tape, (mix, e1, e2), (ppm, seed)
        return s1, s2

    @staticmethod
    def backward(ctx, d_s1, d_s2):
        eng = ctx.module._engine
        mix, e1, e2 = ctx.inputs
        zeros = lambda g: torch.zeros_like(mix) if g is None else g.contiguous()
        eng.set_option("dropout_ppm", ctx.drop[0])
        eng.set_option("dropout_seed", ctx.drop[1])
        eng.train_backward(mix, e1, e2, zeros(d_s1), zeros(d_s2), ctx.tape)
        ctx.tape = None
        # the library's gradient buffers are reused by the next step: hand autograd its own copy -- ONE flat copy whose
        # per-parameter views autograd adopts as .grad without copying (train.allreduce_gradients finds the flat
        # tensor again through `_flat_grad`)
        flat = eng._grads_flat.clone()
        ctx.module._flat_grad = flat
        outs = []
        for k, shape in eng.slots:
            o = eng._grad_offsets[k]
            outs.append(flat[o:o + eng._grads[k].numel()].view(*shape))
        return (None, None, None, None) + tuple(outs)


class _LongTrainingKeyword(type):
    """``Model(..., long_training=True)`` for the classes that set ``_long_training_keyword``: the keyword is taken off by the
    class call and kept as an attribute, so every ``__init__`` keeps exactly the reference's parameters and defaults (the
    drop-in contract; tests/test_mask_variant_host.py pins it) and a Hydra user still writes ``+model.long_training=true``."""

    def __call__(cls, *args, **kwargs):
        if not cls._long_training_keyword:
            return super().__call__(*args, **kwargs)
        long_training = bool(kwargs.pop("long_training", False))
        module = super().__call__(*args, **kwargs)
        module.long_training = long_training
        return module


class _DPTNBase(nn.Module, metaclass=_LongTrainingKeyword):
    # DPTN blocks only: the training step on clips of more than 256 chunks (library option train_long_seq = 1, set on every
    # engine _get_engine makes).  DPRNN blocks have no such limit and take no keyword.
    _long_training_keyword = False
    long_training = False

    def __init__(self, cfg: DPTNConfig):
        super().__init__()
        self.cfg = cfg
        for key, shape in state_dict_spec(cfg):
            parts = key.split(".")
            node: nn.Module = self
            for name in parts[:-1]:
                if name not in node._modules:
                    node.add_module(name, _Node())
                node = node._modules[name]
            p = nn.Parameter(torch.empty(*shape))
            node.register_parameter(parts[-1], p)
            _init_like_torch(key, p, cfg)
            p._dptnav_owner = weakref.ref(self)      # lets optim.FusedAdamW / clip_grad_norm_ find the engine
        self._engine: Optional[DptnEngine] = None

    # -- engine management -------------------------------------------------------------------
    def _params(self) -> Dict[str, torch.Tensor]:
        return dict(self.named_parameters())

    def _get_engine(self, device: torch.device) -> DptnEngine:
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} computes only on an AMD GPU through libdptnav "
                               f"(got a {device} tensor); there is no CPU/PyTorch fallback")
        eng = self._engine
        if eng is None or eng.device != device:
            eng = DptnEngine(self.cfg, device)
            if self.long_training:
                eng.set_option("train_long_seq", 1)
            self._engine = eng
        params = self._params()
        for k, p in params.items():
            if p.device != device:
                raise RuntimeError(f"parameter {k} is on {p.device} but the input is on {device}: call model.to(device)")
        if not eng.bound_to(params):
            eng.bind(params)  # borrows the nn.Parameter storages (optimizer / load_state_dict stay in charge)
        return eng

    def _arm_dropout(self, eng: DptnEngine):
        """Train-mode attention dropout (dptn.py:16-21): a fresh seed per call, kept for this call's backward.  Data-parallel
        ranks share torch's seed, so the rank is mixed in to keep their masks apart."""
        ppm = int(round(self.cfg.dropout * 1e6)) if self.training else 0
        self._drop_step = getattr(self, "_drop_step", 0) + 1
        rank = int(os.environ.get("RANK", "0"))
        seed = (torch.initial_seed() * 2654435761 + self._drop_step * 40503 + rank * 0x632BE5AB) & 0x7FFFFFFF
        eng.set_option("dropout_ppm", ppm)
        eng.set_option("dropout_seed", seed)
        return ppm, seed

    def _train_kernels_built(self) -> bool:
        return self.cfg.num_features in (128, 64)        # DPTN and DPRNN blocks, bidirectional or not

    def _run(self, mix, e1, e2):
        cont = lambda t: None if t is None else t.contiguous()
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            if not self._train_kernels_built():
                raise NotImplementedError("the training step (backward kernels) is built for num_features in {128, 64}; use "
                                          "torch.no_grad() here")
            s1, s2 = _SeparateFn.apply(self, mix.contiguous(), cont(e1), cont(e2), *self.parameters())
            return {"s1_pred": s1, "s2_pred": s2}
        eng = self._get_engine(mix.device)
        # model.train() under torch.no_grad(): the reference still applies attention dropout (nn.MultiheadAttention looks at
        # self.training only).  The dropout lives in the training kernels, so take that path and drop the tape; where it
        # is not built, say so instead of silently returning the eval-mode result.  DPRNN blocks have no dropout.
        if self.training and self.cfg.blocks == "dptn" and self.cfg.dropout > 0:
            if not self._train_kernels_built():
                raise NotImplementedError("train-mode forward (attention dropout) is built for num_features in {128, 64} "
                                          "only: call model.eval() for inference")
            self._arm_dropout(eng)
            s1, s2, _tape = eng.train_forward(mix.contiguous(), cont(e1), cont(e2))
            return {"s1_pred": s1, "s2_pred": s2}
        s1, s2 = eng.forward(mix, e1, e2)
        return {"s1_pred": s1, "s2_pred": s2}

    def __str__(self):
        all_parameters = sum(p.numel() for p in self.parameters())
        trainable_parameters = sum(p.numel() for p in self.parameters() if p.requires_grad)
        return (super().__str__() + f"\nAll parameters: {all_parameters}"
                + f"\nTrainable parameters: {trainable_parameters}")


class DPTNAVWavEncDec(_DPTNBase):
    """Audio-visual DPTN (BASELINE configs 3/4) -- same constructor as the reference class of that name, plus the keyword
    ``long_training`` (training step beyond 256 chunks per mixture)."""
    _long_training_keyword = True

    def __init__(self, num_features=64, video_emb_size=1024, hidden_video=128, kernel_size_enc=2, hidden_dim=32,
                 num_blocks=6, chunk_size=10, step_size=5, num_heads=4, dropout=0.1, bidir=True):
        super().__init__(DPTNConfig(num_features=num_features, video_emb_size=video_emb_size,
                                    hidden_video=hidden_video, kernel_size_enc=kernel_size_enc,
                                    hidden_dim=hidden_dim, num_blocks=num_blocks, chunk_size=chunk_size,
                                    step_size=step_size, num_heads=num_heads, dropout=dropout, bidir=bool(bidir),
                                    audio_only=False))

    def forward(self, mix, s1_embedding, s2_embedding, **batch):
        return self._run(mix, s1_embedding, s2_embedding)


class DPTNWavEncDec(_DPTNBase):
    """Audio-only DPTN (BASELINE config 2) -- same constructor as the reference class of that name, plus the keyword
    ``long_training`` (training step beyond 256 chunks per mixture)."""
    _long_training_keyword = True

    def __init__(self, num_features=64, kernel_size_enc=2, hidden_dim=32, num_blocks=6, chunk_size=10, step_size=5,
                 num_heads=4, dropout=0.1, bidir=True):
        super().__init__(DPTNConfig(num_features=num_features, kernel_size_enc=kernel_size_enc,
                                    hidden_dim=hidden_dim, num_blocks=num_blocks, chunk_size=chunk_size,
                                    step_size=step_size, num_heads=num_heads, dropout=dropout, bidir=bool(bidir),
                                    audio_only=True))

    def forward(self, mix, **batch):
        return self._run(mix, None, None)


class DPTNEncDec(_DPTNBase):
    """Audio-only masked DPTN (src/configs/model/dptn.yaml) -- same constructor as the reference class of that name
    (dptn.py:154-165).  Same blocks and separation conv as DPTNWavEncDec; per speaker the tail is
    ReLU(tanh(output(u)) * sigmoid(output_gate(u))) * encoded instead of postprocessing(u) + encoded (dptn.py:141,189).
    Plus the keyword ``long_training`` (training step beyond 256 chunks per mixture)."""
    _long_training_keyword = True

    def __init__(self, num_features=64, kernel_size_enc=2, hidden_dim=32, num_blocks=6, chunk_size=10, step_size=5,
                 num_heads=4, dropout=0.1, bidir=True):
        super().__init__(DPTNConfig(num_features=num_features, kernel_size_enc=kernel_size_enc,
                                    hidden_dim=hidden_dim, num_blocks=num_blocks, chunk_size=chunk_size,
                                    step_size=step_size, num_heads=num_heads, dropout=dropout, bidir=bool(bidir),
                                    audio_only=True, arch="dptn_mask"))

    def forward(self, mix, **batch):
        return self._run(mix, None, None)


class DPRNNEncDec(_DPTNBase):
    """Audio-only DPRNN (backbone of BASELINE config 5) -- same constructor as the reference class of that name
    (src/model/dprnn.py:238-247); forward(mix, **batch) as dprnn.py:260."""

    def __init__(self, num_features=64, kernel_size_enc=2, hidden_dim=32, num_blocks=6, chunk_size=10, step_size=5,
                 bidir=True):
        super().__init__(DPTNConfig(num_features=num_features, hidden_video=num_features,
                                    kernel_size_enc=kernel_size_enc, hidden_dim=hidden_dim, num_blocks=num_blocks,
                                    chunk_size=chunk_size, step_size=step_size, bidir=bool(bidir), audio_only=True,
                                    arch="dprnn"))

    def forward(self, mix, **batch):
        return self._run(mix, None, None)


class DPRNNAVEncDec(_DPTNBase):
    """"DPRNN-AV" of BASELINE config 5.  The reference has no such class; this is
    DPRNNEncDec plus the lip-embedding fusion head of DPTNAVWavEncDec (dptn_wav.py:173-184) with the same parameter
    names (gate, visual_compression.*, video_ln.*)."""

    def __init__(self, num_features=64, video_emb_size=512, hidden_video=64, kernel_size_enc=2, hidden_dim=32,
                 num_blocks=6, chunk_size=10, step_size=5, bidir=True):
        super().__init__(DPTNConfig(num_features=num_features, video_emb_size=video_emb_size,
                                    hidden_video=hidden_video, kernel_size_enc=kernel_size_enc,
                                    hidden_dim=hidden_dim, num_blocks=num_blocks, chunk_size=chunk_size,
                                    step_size=step_size, bidir=bool(bidir), audio_only=False, arch="dprnn"))

    def forward(self, mix, s1_embedding, s2_embedding, **batch):
        return self._run(mix, s1_embedding, s2_embedding)


def _register_spec_parameters(module: nn.Module, spec):
    """One uninitialised nn.Parameter per (key, shape) of a state_dict spec, in its order, under `_Node` containers named
    by the key's path (so state_dict() has the spec's keys and order)."""
    for key, shape in spec:
        parts = key.split(".")
        node = module
        for name in parts[:-1]:
            if name not in node._modules:
                node.add_module(name, _Node())
            node = node._modules[name]
        node.register_parameter(parts[-1], nn.Parameter(torch.empty(*shape)))


def _bound_engine(module: nn.Module, attr: str, make, device: torch.device):
    """The engine `module` keeps in `attr` for `device` -- made by make(device) at first use and after a device change --
    bound to the module's parameters as they are now."""
    if device.type != "cuda":
        raise RuntimeError(f"{type(module).__name__} computes only on an AMD GPU through libdptnav (got a {device} tensor); "
                           f"there is no CPU/PyTorch fallback")
    eng = getattr(module, attr)
    if eng is None or eng.device != device:
        eng = make(device)
        setattr(module, attr, eng)
    params = dict(module.named_parameters())
    for k, p in params.items():
        if p.device != device:
            raise RuntimeError(f"parameter {k} is on {p.device} but the input is on {device}: call model.to(device)")
    if not eng.bound_to(params):
        eng.bind(params)
    return eng


def _str_with_parameter_counts(module: nn.Module) -> str:
    all_parameters = sum(p.numel() for p in module.parameters())
    trainable_parameters = sum(p.numel() for p in module.parameters() if p.requires_grad)
    return (nn.Module.__str__(module) + f"\nAll parameters: {all_parameters}"
            + f"\nTrainable parameters: {trainable_parameters}")


class ConvTasNet(nn.Module):
    """Conv-TasNet (BASELINE configs[0], src/configs/model/convtasnet.yaml) -- same constructor as the reference class of
    that name (src/model/convtasnet.py:101-116): N and L are accepted and ignored, as there.  Inference only: the forward
    runs on libdptnav (include/ctasnet.h); the training step is not built."""

    def __init__(self, N=512, L=16):
        super().__init__()
        self.N = N
        self.L = L
        _register_spec_parameters(self, convtasnet_state_dict_spec())
        self.reset_parameters()
        self._engine: Optional[ConvTasNetEngine] = None

    def reset_parameters(self):
        """torch's defaults for the reference's modules: Conv1d / ConvTranspose1d weights U(+-1/sqrt(fan_in)) (kaiming_uniform,
        a=sqrt 5) and biases with the matching bound; PReLU 0.25; GlobalNorm / GroupNorm ones and zeros."""
        params = dict(self.named_parameters())
        with torch.no_grad():
            for key, p in params.items():
                if key.endswith(("PReLU_1.weight", "PReLU_2.weight", "seq.0.weight")):
                    p.fill_(0.25)
                elif key.endswith(("gamma", "norm_1.weight", "norm_2.weight")):
                    p.fill_(1.0)
                elif key.endswith(("beta", "norm_1.bias", "norm_2.bias")):
                    p.zero_()
                else:
                    w = params[key[:-len("bias")] + "weight"] if key.endswith("bias") else p
                    b = 1.0 / math.sqrt(w[0].numel())
                    p.uniform_(-b, b)

    def _get_engine(self, device: torch.device) -> ConvTasNetEngine:
        return _bound_engine(self, "_engine", ConvTasNetEngine, device)

    def forward(self, mix, **batch):
        eng = self._get_engine(mix.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError("ConvTasNet: training step not built; use torch.no_grad()")
        s1, s2 = eng.forward(mix)
        return {"s1_pred": s1, "s2_pred": s2}

    __str__ = _str_with_parameter_counts


class _ConvTasNetTrainFn(torch.autograd.Function):
    """The model part of TrainableConvTasNet's / TrainableDeepConvTasNet's / TrainableDeepAVConvTasNet's training step, as
    _SeparateFn: forward records the tape (<prefix>_train_forward), backward turns d loss / d predictions into every
    parameter's gradient (<prefix>_train_backward) and hands autograd views of one flat copy -- None for a parameter the
    forward never reads (the engine's no_grad_keys), as autograd itself leaves it.  e1, e2: the speaker embeddings of the
    audio-visual model (None otherwise); they get no gradient."""

    @staticmethod
    def forward(ctx, module, mix, e1, e2, *params):
        eng = module._get_engine(mix.device)
        if eng._grads is None:
            eng.bind_grads()
        emb = () if e1 is None else (e1, e2)
        s1, s2, tape = eng.train_forward(mix, *emb)
        ctx.module, ctx.tape, ctx.mix, ctx.emb = module, tape, mix, emb
        return s1, s2

    @staticmethod
    def backward(ctx, d_s1, d_s2):
        eng = ctx.module._engine
        mix = ctx.mix
        L = eng.out_len(mix.shape[1])
        zeros = lambda g: torch.zeros(mix.shape[0], L, device=mix.device) if g is None else g.contiguous()
        eng.train_backward(mix, *ctx.emb, zeros(d_s1), zeros(d_s2), ctx.tape)
        ctx.tape = None
        # the library's gradient buffers are reused by the next step: autograd gets its own flat copy, whose views become
        # .grad (train.allreduce_gradients and the fused clip / AdamW find it again through `_flat_grad`)
        flat = eng._grads_flat.clone()
        ctx.module._flat_grad = flat
        outs = []
        for k, shape in eng.slots:
            o = eng._grad_offsets[k]
            outs.append(None if k in eng.no_grad_keys else flat[o:o + eng._grads[k].numel()].view(*shape))
        return (None, None, None, None) + tuple(outs)


class _TrainStep:
    """What the Trainable* classes put in front of their inference class: the inference engine kept beside the training
    one (`_engine`), the flat gradient of the last backward, and the forward that picks between the two."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)            # the inference class's constructor
        self._infer_engine = None
        self._flat_grad: Optional[torch.Tensor] = None
        for p in self.parameters():
            p._dptnav_owner = weakref.ref(self)      # lets optim.FusedAdamW / clip_grad_norm_ find the engine

    def _step(self, mix, *emb):
        """emb: the two speaker embeddings of an audio-visual model, or nothing"""
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            for name, e in zip(("s1_embedding", "s2_embedding"), emb):
                if isinstance(e, torch.Tensor) and e.requires_grad:
                    raise NotImplementedError(f"{type(self).__name__}: no gradient is computed for {name} (it comes from a "
                                              f"frozen lip-reader): pass it detached")
            e1, e2 = emb if emb else (None, None)
            s1, s2 = _ConvTasNetTrainFn.apply(self, mix.contiguous(), e1, e2, *self.parameters())
        else:
            s1, s2 = self._get_infer_engine(mix.device).forward(mix, *emb)
        return {"s1_pred": s1, "s2_pred": s2}

    def forward(self, mix, **batch):
        return self._step(mix)


class TrainableConvTasNet(_TrainStep, ConvTasNet):
    """ConvTasNet with the training step on libdptnav (include/ctasnet_train.h): same constructor, state_dict keys and
    order, initialisation and parameter-count lines as ConvTasNet, and checkpoints load strictly either way.  Under
    torch.no_grad() the forward is ConvTasNet's inference engine (bitwise the same outputs); with grad enabled it records
    a tape and its backward computes every parameter's gradient in HIP.  `_get_engine` is the training engine, so
    optim.clip_grad_norm_ / optim.FusedAdamW / train.train_step take their fused paths; stock torch optimizers work too."""

    def _get_engine(self, device: torch.device) -> ConvTasNetTrainEngine:
        return _bound_engine(self, "_engine", ConvTasNetTrainEngine, device)

    def _get_infer_engine(self, device: torch.device) -> ConvTasNetEngine:
        return _bound_engine(self, "_infer_engine", ConvTasNetEngine, device)


class DeepConvTasNet(nn.Module):
    """Deep encoder / decoder Conv-TasNet (src/configs/model/deepconvtasnet.yaml) -- same constructor as the reference class
    of that name (src/model/deepconvtasnet.py:122-136): N and L are accepted and ignored, as there.  Inference only: the
    forward runs on libdptnav (include/dctasnet.h); TrainableDeepConvTasNet adds the training step."""

    _AV = False

    def __init__(self, N=512, L=16):
        super().__init__()
        self.N = N
        self.L = L
        _register_spec_parameters(self, deepconvtasnet_state_dict_spec(self._AV))
        self.reset_parameters()
        self._engine: Optional[DeepConvTasNetEngine] = None

    def reset_parameters(self):
        """torch's defaults for the reference's modules: Conv1d / ConvTranspose1d / Linear weights U(+-1/sqrt(fan_in))
        (kaiming_uniform, a=sqrt 5, fan_in = weight[0].numel()) and biases with the matching bound; PReLU 0.25; GlobalNorm /
        GroupNorm / LayerNorm ones and zeros."""
        params = dict(self.named_parameters())
        with torch.no_grad():
            for key, p in params.items():
                if p.numel() == 1 and key.endswith(".weight") and not key.startswith("decoder.sequential.8"):
                    p.fill_(0.25)                                   # every PReLU of the model
                elif key.endswith(("gamma", "norm_1.weight", "norm_2.weight", "video_ln.weight")):
                    p.fill_(1.0)
                elif key.endswith(("beta", "norm_1.bias", "norm_2.bias", "video_ln.bias")):
                    p.zero_()
                else:
                    w = params[key[:-len("bias")] + "weight"] if key.endswith("bias") else p
                    b = 1.0 / math.sqrt(w[0].numel())
                    p.uniform_(-b, b)

    def _get_engine(self, device: torch.device) -> DeepConvTasNetEngine:
        return _bound_engine(self, "_engine", lambda dev: DeepConvTasNetEngine(dev, av=self._AV), device)

    def _run(self, mix, s1_embedding=None, s2_embedding=None):
        eng = self._get_engine(mix.device)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters()):
            raise NotImplementedError(f"{type(self).__name__}: training step not built; use torch.no_grad()")
        s1, s2 = eng.forward(mix, s1_embedding, s2_embedding)
        return {"s1_pred": s1, "s2_pred": s2}

    def forward(self, mix, **batch):
        return self._run(mix)

    __str__ = _str_with_parameter_counts


class TrainableDeepConvTasNet(_TrainStep, DeepConvTasNet):
    """DeepConvTasNet with the training step on libdptnav (include/dctasnet_train.h), the counterpart of
    TrainableConvTasNet: same constructor, state_dict keys and order, initialisation and parameter-count lines as
    DeepConvTasNet, and checkpoints load strictly either way.  Under torch.no_grad() the forward is DeepConvTasNet's
    inference engine (bitwise the same outputs); with grad enabled it records a tape and its backward computes every
    parameter's gradient in HIP.  decoder.deconv.weight is a parameter the reference's forward never reads: its .grad stays
    None, as after the reference's loss.backward(), and the fused clip / AdamW leave it out (torch.optim.AdamW skips it too)."""

    def _get_engine(self, device: torch.device) -> DeepConvTasNetTrainEngine:
        return _bound_engine(self, "_engine", DeepConvTasNetTrainEngine, device)

    def _get_infer_engine(self, device: torch.device) -> DeepConvTasNetEngine:
        return _bound_engine(self, "_infer_engine", lambda dev: DeepConvTasNetEngine(dev, av=False), device)


class DeepAVConvTasNet(DeepConvTasNet):
    """Audio-visual deep Conv-TasNet (src/configs/model/deepavconvtasnet.yaml) -- same constructor as the reference class
    (src/model/deepavconvtasnet.py:122-134); N and L are ignored as there.  Only the built sizes video_emb_size = hidden_video
    = 512 exist.  Inference only (include/dctasnet.h); TrainableDeepAVConvTasNet adds the training step."""

    _AV = True

    def __init__(self, N=512, L=16, video_emb_size=512, hidden_video=512):
        if video_emb_size != 512 or hidden_video != 512:
            raise NotImplementedError(f"DeepAVConvTasNet is built for video_emb_size=512, hidden_video=512 only (got "
                                      f"video_emb_size={video_emb_size}, hidden_video={hidden_video})")
        super().__init__(N=N, L=L)

    def forward(self, mix, s1_embedding, s2_embedding, **batch):
        return self._run(mix, s1_embedding, s2_embedding)


class TrainableDeepAVConvTasNet(_TrainStep, DeepAVConvTasNet):
    """DeepAVConvTasNet with the training step on libdptnav (include/davctasnet_train.h), the counterpart of
    TrainableDeepConvTasNet: same constructor, state_dict keys and order, initialisation and parameter-count lines as
    DeepAVConvTasNet, and checkpoints load strictly either way.  Under torch.no_grad() the forward is DeepAVConvTasNet's
    inference engine (bitwise the same outputs); with grad enabled it records a tape and its backward computes every
    parameter's gradient in HIP, the audio-visual head's included.  The speaker embeddings get no gradient (the reference
    feeds them from a frozen lip-reader through the dataset): one that requires grad is refused.  decoder.deconv.weight
    behaves as in TrainableDeepConvTasNet."""

    def _get_engine(self, device: torch.device) -> DeepAVConvTasNetTrainEngine:
        return _bound_engine(self, "_engine", DeepAVConvTasNetTrainEngine, device)

    def _get_infer_engine(self, device: torch.device) -> DeepConvTasNetEngine:
        return _bound_engine(self, "_infer_engine", lambda dev: DeepConvTasNetEngine(dev, av=True), device)

    def forward(self, mix, s1_embedding, s2_embedding, **batch):
        return self._step(mix, s1_embedding, s2_embedding)
