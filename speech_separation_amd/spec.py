"""Shape / checkpoint specification of the DPTN(-AV) raw-waveform separator.

This module is pure host logic (numpy only): it states the hyper-parameters the
hot path is built for, the derived sizes (frames, chunks, tokens) and the exact
``state_dict`` key order + shapes that the reference's checkpoints use, so that
the HIP library, the ``nn.Module`` shim, the oracle and the tests all agree on
one table.

Reference surfaces restated here (never imported):
  * ctor kwargs / defaults ........ src/model/dptn_wav.py:137-169 (AV), :72-103 (audio)
  * Hydra values .................. src/configs/model/dptn_wav_av.yaml:1-12,
                                    src/configs/model/dptn_wav.yaml:1-10
  * parameter registration order .. dptn_wav.py:153-169 -> dptn_wav.py:18-33
                                    -> dptn.py:59-60 -> dptn.py:16-34
  * frame/chunk arithmetic ........ nn.Conv1d(k, stride=k//2) dptn_wav.py:153;
                                    SplitToFolds dprnn.py:122-136
"""
from __future__ import annotations

from dataclasses import dataclass, asdict
from typing import Dict, List, Tuple

import numpy as np


@dataclass(frozen=True)
class DPTNConfig:
    """Constructor arguments of DPTNAVWavEncDec / DPTNWavEncDec (same names)."""

    num_features: int = 128
    video_emb_size: int = 512
    hidden_video: int = 128
    kernel_size_enc: int = 7
    hidden_dim: int = 128
    num_blocks: int = 6
    chunk_size: int = 150
    step_size: int = 75
    num_heads: int = 4
    dropout: float = 0.1
    bidir: bool = True
    audio_only: bool = False  # True -> DPTNWavEncDec / DPRNNEncDec (no video branch)
    arch: str = "dptn"        # "dptn": MHA + bi-LSTM blocks (dptn.py); "dprnn": bi-LSTM + fc blocks (dprnn.py:7-113);
    #                           "dptn_mask": DPTN blocks with the masked tail of DPTNEncDec (dptn.py:82-208, audio only)

    def __post_init__(self):
        if self.arch not in ("dptn", "dprnn", "dptn_mask"):
            raise ValueError(f"arch must be 'dptn', 'dprnn' or 'dptn_mask' (got {self.arch!r})")
        if self.arch == "dptn_mask" and not self.audio_only:
            raise ValueError("arch='dptn_mask' (DPTNEncDec) is audio-only: the reference defines no AV masked variant")

    @property
    def blocks(self) -> str:
        """Block type of the separator: "dptn" (TransformerDPRNN, also for the masked variant) or "dprnn"."""
        return "dprnn" if self.arch == "dprnn" else "dptn"

    @property
    def mask_tail(self) -> bool:
        """True for DPTNEncDec: ReLU(tanh(W_out u + b_out) * sigmoid(W_gate u + b_gate)) * encoded (dptn.py:103-115,141,189)."""
        return self.arch == "dptn_mask"

    # ---- derived sizes -------------------------------------------------
    @property
    def stride_enc(self) -> int:
        return self.kernel_size_enc // 2

    @property
    def head_dim(self) -> int:
        return self.num_features // self.num_heads

    def frames(self, T: int) -> int:
        """Latent length L of Conv1d(k, stride=k//2, no padding)."""
        return (T - self.kernel_size_enc) // self.stride_enc + 1

    def chunks(self, L: int) -> int:
        """Number of 50%-overlap chunks S produced by SplitToFolds."""
        return (L - self.chunk_size) // self.step_size + 1

    def ola_len(self, S: int) -> int:
        return (S - 1) * self.step_size + self.chunk_size

    def tokens(self, B: int, T: int) -> int:
        return B * self.chunks(self.frames(T)) * self.chunk_size

    def to_dict(self) -> dict:
        return asdict(self)


#: BASELINE.json config 3/4 (src/configs/model/dptn_wav_av.yaml)
DPTN_AV = DPTNConfig()
#: BASELINE.json config 2 (src/configs/model/dptn_wav.yaml)
DPTN_AUDIO = DPTNConfig(num_features=64, audio_only=True)
#: BASELINE.json config 5 backbone (src/configs/model/dprnn.yaml): audio-only DPRNNEncDec is the only variant the
#: reference defines; audio_only=False adds this repo's AV fusion head (same as dptn_wav.py:173-184) = "DPRNN-AV"
DPRNN_AUDIO = DPTNConfig(num_features=64, hidden_video=64, kernel_size_enc=2, hidden_dim=128, num_blocks=6,
                         chunk_size=250, step_size=125, audio_only=True, arch="dprnn")
DPRNN_AV = DPTNConfig(**{**DPRNN_AUDIO.__dict__, "audio_only": False})
#: src/configs/model/dptn.yaml (top-level config dptn.yaml): the masked DPTNEncDec (dptn.py:139-208)
DPTN_MASK = DPTNConfig(num_features=64, kernel_size_enc=7, hidden_dim=128, num_blocks=6, chunk_size=150, step_size=75,
                       num_heads=4, audio_only=True, arch="dptn_mask")
#: small shape used by the golden fixtures (fast on every backend)
DPTN_TINY = DPTNConfig(num_features=32, video_emb_size=24, hidden_video=32, kernel_size_enc=7,
                       hidden_dim=32, num_blocks=2, chunk_size=10, step_size=5, num_heads=4)


_DPRNN_PATH_TENSORS: List[Tuple[str, str]] = [
    ("rnn.weight_ih_l0", "4H,N"),
    ("rnn.weight_hh_l0", "4H,H"),
    ("rnn.bias_ih_l0", "4H"),
    ("rnn.bias_hh_l0", "4H"),
    ("rnn.weight_ih_l0_reverse", "4H,N"),
    ("rnn.weight_hh_l0_reverse", "4H,H"),
    ("rnn.bias_ih_l0_reverse", "4H"),
    ("rnn.bias_hh_l0_reverse", "4H"),
    ("fc.weight", "N,DH"),
    ("fc.bias", "N"),
    ("norm1d.weight", "N"),
    ("norm1d.bias", "N"),
]

_PATH_TENSORS: List[Tuple[str, str]] = [
    # (suffix, shape-code)
    ("mha.in_proj_weight", "3N,N"),
    ("mha.in_proj_bias", "3N"),
    ("mha.out_proj.weight", "N,N"),
    ("mha.out_proj.bias", "N"),
    ("ln1.weight", "N"),
    ("ln1.bias", "N"),
    ("rnn.weight_ih_l0", "4H,N"),
    ("rnn.weight_hh_l0", "4H,H"),
    ("rnn.bias_ih_l0", "4H"),
    ("rnn.bias_hh_l0", "4H"),
    ("rnn.weight_ih_l0_reverse", "4H,N"),
    ("rnn.weight_hh_l0_reverse", "4H,H"),
    ("rnn.bias_ih_l0_reverse", "4H"),
    ("rnn.bias_hh_l0_reverse", "4H"),
    ("ffn.1.weight", "N,DH"),
    ("ffn.1.bias", "N"),
    ("ln2.weight", "N"),
    ("ln2.bias", "N"),
]


def state_dict_spec(cfg: DPTNConfig) -> List[Tuple[str, Tuple[int, ...]]]:
    """Ordered (key, shape) list == ``model.state_dict()`` of the reference.

    The order is the slot order of the C-ABI weight table (include/dptnav.h).
    """
    N, H, k = cfg.num_features, cfg.hidden_dim, cfg.kernel_size_enc
    out: List[Tuple[str, Tuple[int, ...]]] = []
    if not cfg.audio_only:
        out.append(("gate", (1,)))
    out.append(("encoder.weight", (N, 1, k)))
    if not cfg.audio_only:
        out.append(("visual_compression.weight", (cfg.hidden_video // 2, cfg.video_emb_size)))
        out.append(("visual_compression.bias", (cfg.hidden_video // 2,)))
        out.append(("video_ln.weight", (cfg.hidden_video,)))
        out.append(("video_ln.bias", (cfg.hidden_video,)))
    for b in range(cfg.num_blocks):
        for path in ("intra_chunk_block", "inter_chunk_block"):
            two_dirs = True if path == "intra_chunk_block" else cfg.bidir
            dims = {"N": N, "3N": 3 * N, "4H": 4 * H, "H": H, "DH": H * (2 if two_dirs else 1)}
            for suffix, code in (_PATH_TENSORS if cfg.blocks == "dptn" else _DPRNN_PATH_TENSORS):
                if suffix.endswith("_reverse") and not two_dirs:
                    continue
                shape = tuple(dims[c] for c in code.split(","))
                out.append((f"dprnn.model.{b}.{path}.{suffix}", shape))
    out.append(("dprnn.speakers_separation.0.weight", (1,)))
    out.append(("dprnn.speakers_separation.1.weight", (2 * N, N, 1, 1)))
    out.append(("dprnn.speakers_separation.1.bias", (2 * N,)))
    if cfg.mask_tail:   # DPTN.__init__ registers output_gate before output (dptn.py:103-111); postprocessing is a bare ReLU
        out.append(("dprnn.output_gate.0.weight", (N, N, 1)))
        out.append(("dprnn.output_gate.0.bias", (N,)))
        out.append(("dprnn.output.0.weight", (N, N, 1)))
        out.append(("dprnn.output.0.bias", (N,)))
    else:
        out.append(("dprnn.postprocessing.0.weight", (N, N, 1)))
        out.append(("dprnn.postprocessing.0.bias", (N,)))
    out.append(("decoder.weight", (N, 1, k)))
    return out


def convtasnet_state_dict_spec() -> List[Tuple[str, Tuple[int, ...]]]:
    """Ordered (key, shape) list == ``ConvTasNet().state_dict()`` of the reference (src/model/convtasnet.py:101-108; the
    model ignores its N / L arguments: Encoder :7-10, GlobalNorm :19-22, Separator :56-63 with N=512, B=128, H=512, X=8,
    P=3, R=3, Conv1D_Block :33-44, Decoder :86-90).  The order is the slot order of include/ctasnet.h's weight table."""
    N, L, B, H, X, P, R = 512, 16, 128, 512, 8, 3, 3
    out: List[Tuple[str, Tuple[int, ...]]] = [
        ("encoder.conv1d.weight", (N, 1, 2 * L)), ("separator.norm_1.gamma", (N, 1)), ("separator.norm_1.beta", (N, 1)),
        ("separator.conv1d.weight", (B, N, 1)), ("separator.conv1d.bias", (B,))]
    for i in range(P * X):
        p = f"separator.separator.{i}."
        out += [(p + "conv1d.weight", (H, B, 1)), (p + "conv1d.bias", (H,)), (p + "PReLU_1.weight", (1,)),
                (p + "norm_1.weight", (H,)), (p + "norm_1.bias", (H,)), (p + "dconv1d.weight", (H, 1, R)),
                (p + "dconv1d.bias", (H,)), (p + "PReLU_2.weight", (1,)), (p + "norm_2.weight", (H,)),
                (p + "norm_2.bias", (H,)), (p + "conv.weight", (B, H, 1)), (p + "conv.bias", (B,)),
                (p + "conv_sc.weight", (B, H, 1)), (p + "conv_sc.bias", (B,))]
    out += [("separator.seq.0.weight", (1,)), ("separator.seq.1.weight", (2 * N, B, 1)), ("separator.seq.1.bias", (2 * N,)),
            ("decoder.deconv.weight", (N, 1, 2 * L))]
    return out


def deepconvtasnet_state_dict_spec(av: bool = False) -> List[Tuple[str, Tuple[int, ...]]]:
    """Ordered (key, shape) list == ``DeepConvTasNet().state_dict()`` (src/model/deepconvtasnet.py:122-129; 372 tensors,
    11 379 386 parameters) or, with ``av``, ``DeepAVConvTasNet().state_dict()`` (src/model/deepavconvtasnet.py:122-134; 376
    tensors, 11 511 738 parameters).  Encoder :7-21, the Separator of ConvTasNet, Decoder :96-112 (``decoder.deconv`` is
    registered but never used by the forward), then the video head.  The order is the slot order of include/dctasnet.h."""
    N, L = 512, 16
    out: List[Tuple[str, Tuple[int, ...]]] = [("encoder.sequential.0.weight", (N, 1, 2 * L)), ("encoder.sequential.0.bias", (N,))]
    for i in (1, 3, 5, 7):
        out += [(f"encoder.sequential.{i}.weight", (N, N, 3)), (f"encoder.sequential.{i}.bias", (N,)),
                (f"encoder.sequential.{i + 1}.weight", (1,))]
    out += [(k, s) for k, s in convtasnet_state_dict_spec() if k.startswith("separator.")]
    for i in (0, 2, 4, 6):
        out += [(f"decoder.sequential.{i}.weight", (N, N, 3)), (f"decoder.sequential.{i}.bias", (N,)),
                (f"decoder.sequential.{i + 1}.weight", (1,))]
    out += [("decoder.sequential.8.weight", (N, 1, 2 * L)), ("decoder.sequential.8.bias", (1,)),
            ("decoder.deconv.weight", (N, 1, 2 * L))]
    if av:
        out += [("visual_compression.weight", (N // 2, N)), ("visual_compression.bias", (N // 2,)),
                ("video_ln.weight", (N,)), ("video_ln.bias", (N,))]
    return out


def num_parameters(cfg: DPTNConfig) -> int:
    return int(sum(int(np.prod(s)) for _, s in state_dict_spec(cfg)))


def synthetic_state_dict(cfg: DPTNConfig, seed: int = 0) -> Dict[str, np.ndarray]:
    """Deterministic, platform-independent random weights (numpy PCG64).

    Used wherever the same weights must exist on two machines without shipping
    them (golden generation here, parity tests / bench on the GPU box).  The
    distributions mimic torch's default init scale (uniform +-1/sqrt(fan_in))
    but make every tensor non-trivial (LayerNorm gains != 1, biases != 0) so a
    dropped parameter shows up in parity.
    """
    rng = np.random.default_rng(seed)
    sd: Dict[str, np.ndarray] = {}
    for key, shape in state_dict_spec(cfg):
        leaf = key.split(".")[-1]
        if key == "gate":
            w = np.array([0.7], dtype=np.float64)
        elif key == "dprnn.speakers_separation.0.weight":
            w = np.array([0.25], dtype=np.float64)
        elif (key.split(".")[-2].startswith(("ln", "video_ln", "norm1d"))) and leaf == "weight":
            w = 1.0 + 0.1 * rng.standard_normal(shape)
        elif (key.split(".")[-2].startswith(("ln", "video_ln", "norm1d"))) and leaf == "bias":
            w = 0.05 * rng.standard_normal(shape)
        else:
            if leaf.startswith("bias") or leaf.endswith("bias"):
                fan_in = {
                    "mha.in_proj_bias": cfg.num_features,
                }.get(".".join(key.split(".")[-2:]), cfg.hidden_dim)
            else:
                fan_in = int(np.prod(shape[1:])) if len(shape) > 1 else shape[0]
            bound = 1.0 / np.sqrt(max(fan_in, 1))
            w = rng.uniform(-bound, bound, size=shape)
        sd[key] = np.ascontiguousarray(w, dtype=np.float32)
    return sd


def synthetic_inputs(cfg: DPTNConfig, B: int, T: int, Tv: int = 50, seed: int = 123) -> Dict[str, np.ndarray]:
    """Seeded inputs of the shapes the trainer hands to ``model(**batch)``.

    mix (B,T) comes from src/datasets/base_dataset.py:144-145 + collate.py:43,
    s*_embedding (B,512,50) from make_embeddings.py:65-69 / base_dataset.py:199-205.
    s1/s2 are only used by loss/metric checks; mix = s1 + s2.
    """
    rng = np.random.default_rng(seed)
    s1 = (0.1 * rng.standard_normal((B, T))).astype(np.float32)
    s2 = (0.1 * rng.standard_normal((B, T))).astype(np.float32)
    out = {"s1": s1, "s2": s2, "mix": (s1 + s2).astype(np.float32)}
    if not cfg.audio_only:
        out["s1_embedding"] = rng.standard_normal((B, cfg.video_emb_size, Tv)).astype(np.float32)
        out["s2_embedding"] = rng.standard_normal((B, cfg.video_emb_size, Tv)).astype(np.float32)
    return out
