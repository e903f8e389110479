"""ctypes binding of libdptnav.so (include/dptnav.h).  No torch types cross this boundary.

The library is looked up next to this file (built in-tree by ``__graft_entry__.build()`` /
``python -m speech_separation_amd.build``).  There is no CPU fallback: if the shared object is
missing or does not export the full ABI, importing callers get a RuntimeError.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

_HERE = os.path.dirname(os.path.abspath(__file__))
# DPTNAV_LIB: another build of the library (same-box A/B of two builds: tools/train_ab.py, tools/ab_option.py)
LIB_PATH = os.environ.get("DPTNAV_LIB") or os.path.join(_HERE, "libdptnav.so")
ABI_VERSION = 4


class DptnavConfig(C.Structure):
    """struct dptnav_config (include/dptnav.h)."""

    _fields_ = [(n, C.c_int32) for n in (
        "num_features", "video_emb_size", "hidden_video", "kernel_size_enc", "hidden_dim", "num_blocks",
        "chunk_size", "step_size", "num_heads", "bidir", "audio_only", "arch", "mask_tail")]


_vp, _fp, _i, _i64, _sz = C.c_void_p, C.c_void_p, C.c_int, C.c_int64, C.c_size_t

#: name -> (restype, argtypes): every symbol include/dptnav.h declares
SYMBOLS = {
    "dptnav_abi_version": (_i, []),
    "dptnav_create": (_i, [C.POINTER(DptnavConfig), C.POINTER(_vp)]),
    "dptnav_destroy": (None, [_vp]),
    "dptnav_last_error": (C.c_char_p, [_vp]),
    "dptnav_num_weights": (_i, [_vp]),
    "dptnav_weight_name": (C.c_char_p, [_vp, _i]),
    "dptnav_weight_numel": (_i64, [_vp, _i]),
    "dptnav_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "dptnav_frames": (_i64, [_vp, _i64]),
    "dptnav_chunks": (_i64, [_vp, _i64]),
    "dptnav_workspace_bytes": (_sz, [_vp, _i, _i64, _i]),
    "dptnav_forward": (_i, [_vp, _fp, _fp, _fp, _i, _i64, _i, _fp, _fp, _vp, _sz, _vp]),
    "dptnav_stage_head": (_i, [_vp, _fp, _fp, _fp, _i, _i64, _i, _fp, _fp, _vp, _sz, _vp]),
    "dptnav_stage_path": (_i, [_vp, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp]),
    "dptnav_stage_tail": (_i, [_vp, _fp, _fp, _i, _i64, _fp, _fp, _vp, _sz, _vp]),
    "dptnav_sisnr_pairs": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, _i64, _fp, _vp]),
    "dptnav_workspace_tap": (_i, [_vp, _i, _i64, _i, C.c_char_p, C.POINTER(_sz), C.POINTER(_sz)]),
    "dptnav_bind_grads": (_i, [_vp, C.POINTER(_fp), _i]),
    "dptnav_train_path_tape_bytes": (_sz, [_vp, _i, _i]),
    "dptnav_train_bwd_workspace_bytes": (_sz, [_vp, _i, _i]),
    "dptnav_train_path_tape_tap": (_i, [_vp, _i, _i, C.c_char_p, C.POINTER(_sz), C.POINTER(_sz)]),
    "dptnav_train_path_forward": (_i, [_vp, _i, _i, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "dptnav_train_path_backward": (_i, [_vp, _i, _i, _fp, _fp, _fp, _i, _i, _vp, _sz, _vp, _sz, _vp]),
    "dptnav_train_tape_bytes": (_sz, [_vp, _i, _i64, _i]),
    "dptnav_train_workspace_bytes": (_sz, [_vp, _i, _i64, _i]),
    "dptnav_train_forward": (_i, [_vp, _fp, _fp, _fp, _i, _i64, _i, _fp, _fp, _vp, _sz, _vp, _sz, _vp]),
    "dptnav_train_backward": (_i, [_vp, _fp, _fp, _fp, _fp, _fp, _i, _i64, _i, _vp, _sz, _vp, _sz, _vp]),
    "dptnav_flat_offset": (_i64, [_vp, _i]),
    "dptnav_flat_numel": (_i64, [_vp]),
    "dptnav_tail_scratch_bytes": (_sz, [_vp, _i]),
    "dptnav_pit_sisnr_loss": (_i, [_vp, _fp, _fp, _fp, _fp, _i, _i64, C.c_float, _fp, _fp, _fp, _vp, _sz, _vp]),
    "dptnav_grad_clip": (_i, [_vp, _fp, _i64, C.c_float, _vp, _sz, _fp, _vp]),
    "dptnav_adamw_step": (_i, [_vp, _fp, _fp, _fp, _i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i, _vp]),
    "dptnav_dropout_mask": (_i, [_vp, _i, _i, _i, _i, _fp, _vp]),
    "dptnav_set_option": (_i, [_vp, C.c_char_p, _i]),
    "dptnav_profile_enable": (_i, [_vp, _i]),
    "dptnav_profile_collect": (_i, [_vp]),
    "dptnav_profile_reset": (_i, [_vp]),
    "dptnav_profile_num": (_i, []),
    "dptnav_profile_name": (C.c_char_p, [_i]),
    "dptnav_profile_ms": (C.c_double, [_vp, _i]),
    "dptnav_profile_count": (_i64, [_vp, _i]),
    "dptnav_flops_per_mixture": (C.c_double, [_vp, _i64]),
    "dptnav_min_bytes_per_mixture": (C.c_double, [_vp, _i64]),
}

CTASNET_ABI_VERSION = 1
DCTASNET_ABI_VERSION = 1
CTTRAIN_ABI_VERSION = 1
DCTTRAIN_ABI_VERSION = 1
DAVTRAIN_ABI_VERSION = 1
WAVLOSS_ABI_VERSION = 1
WAVMETRIC_ABI_VERSION = 1
LIPFE_ABI_VERSION = 1
SPECFE_ABI_VERSION = 1
VFILT_ABI_VERSION = 1
LIPSN_ABI_VERSION = 1
VFWAVE_ABI_VERSION = 1


def _infer_symbols(prefix, create_extra=(), workspace_extra=(), forward_in=(), more=None):
    """The inference boundary of a Conv-TasNet family member: `create_extra` / `workspace_extra` extend the argument
    lists of create / workspace_bytes, `forward_in` follows the mixture in forward, `more` are the member's own entries."""
    d = {
        "abi_version": (_i, []),
        "create": (_i, [C.POINTER(_vp), *create_extra]),
        "destroy": (None, [_vp]),
        "last_error": (C.c_char_p, [_vp]),
        "num_weights": (_i, [_vp]),
        "weight_name": (C.c_char_p, [_vp, _i]),
        "weight_numel": (_i64, [_vp, _i]),
        "bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
        "frames": (_i64, [_i64]),
        "out_len": (_i64, [_i64]),
        "workspace_bytes": (_sz, [_vp, _i, _i64, *workspace_extra]),
        "forward": (_i, [_vp, _fp, *forward_in, _i, _i64, *workspace_extra, _fp, _fp, _vp, _sz, _vp]),
        "flops_per_mixture": (C.c_double, [_vp, _i64]),
        "min_bytes_per_mixture": (C.c_double, [_vp, _i64]),
        **(more or {}),
    }
    return {f"{prefix}_{k}": v for k, v in d.items()}


def _train_symbols(prefix, create_extra=(), shape_extra=(), forward_in=()):
    """The training boundary of a Conv-TasNet family member; `create_extra` extends the argument list of create,
    `shape_extra` follows (B, T) wherever a shape is passed, `forward_in` follows the mixture in train_forward /
    train_backward."""
    d = {
        "abi_version": (_i, []),
        "create": (_i, [C.POINTER(_vp), *create_extra]),
        "destroy": (None, [_vp]),
        "last_error": (C.c_char_p, [_vp]),
        "num_weights": (_i, [_vp]),
        "weight_name": (C.c_char_p, [_vp, _i]),
        "weight_numel": (_i64, [_vp, _i]),
        "bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
        "bind_grads": (_i, [_vp, C.POINTER(_fp), _i]),
        "flat_offset": (_i64, [_vp, _i]),
        "flat_numel": (_i64, [_vp]),
        "frames": (_i64, [_i64]),
        "out_len": (_i64, [_i64]),
        "workspace_bytes": (_sz, [_vp, _i, _i64, *shape_extra]),
        "train_forward": (_i, [_vp, _fp, *forward_in, _i, _i64, *shape_extra, _fp, _fp, _vp, _sz, _vp]),
        "train_backward": (_i, [_vp, _fp, *forward_in, _i, _i64, *shape_extra, _fp, _fp, _vp, _sz, _vp]),
        "tape_offset": (_i64, [_vp, _i, _i64, *shape_extra, _i, _i]),
        "clip_scratch_bytes": (_sz, [_vp]),
        "grad_clip": (_i, [_vp, _fp, _i64, C.c_float, _vp, _sz, _fp, _vp]),
        "adamw_step": (_i, [_vp, _fp, _fp, _fp, _i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i,
                            _vp]),
        "flops_per_mixture": (C.c_double, [_vp, _i64]),
    }
    return {f"{prefix}_{k}": v for k, v in d.items()}


# The six tables below are name -> (restype, argtypes), as SYMBOLS, for entry points of the same shared object.
#: every symbol include/ctasnet.h declares (Conv-TasNet forward)
CTASNET_SYMBOLS = _infer_symbols("ctasnet")
#: every symbol include/dctasnet.h declares (deep Conv-TasNet forward): create takes av, workspace_bytes and forward take Tv,
#: forward takes the two video streams after the mixture, and the weight pack has a size query
DCTASNET_SYMBOLS = _infer_symbols("dctasnet", create_extra=[_i], workspace_extra=[_i], forward_in=[_fp, _fp],
                                  more={"weight_pack_bytes": (_sz, [_vp])})
#: every symbol include/ctasnet_train.h declares (Conv-TasNet training step)
CTTRAIN_SYMBOLS = _train_symbols("cttrain")
#: every symbol include/dctasnet_train.h declares (deep Conv-TasNet training step): create takes av
DCTTRAIN_SYMBOLS = _train_symbols("dcttrain", create_extra=[_i])
#: every symbol include/davctasnet_train.h declares (deep audio-visual Conv-TasNet training step): every shape carries Tv and
#: the two video streams follow the mixture
DAVTRAIN_SYMBOLS = _train_symbols("davtrain", shape_extra=[_i], forward_in=[_fp, _fp])

#: every symbol include/wavloss.h declares (waveform criteria: MAE / MSE / SI-SNR under batch or utterance PIT; stateless)
WAVLOSS_SYMBOLS = {
    "wavloss_abi_version": (_i, []),
    "wavloss_strerror": (C.c_char_p, [_i]),
    "wavloss_scratch_bytes": (_sz, [_i]),
    "wavloss_pit_loss": (_i, [_i, _i, _fp, _fp, _fp, _fp, _i, _i64, C.c_float, _fp, _fp, _fp, _vp, _vp, _sz, _vp]),
}

#: every symbol include/wavmetric.h declares (evaluation metrics: SI-SDR, stateless; STOI / ESTOI behind a handle)
WAVMETRIC_SYMBOLS = {
    "wavmetric_abi_version": (_i, []),
    "wavmetric_strerror": (C.c_char_p, [_i]),
    "wavmetric_sisdr_pairs": (_i, [_fp, _fp, _fp, _fp, _i, _i64, _fp, _vp]),
    "wavmetric_stoi_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "wavmetric_stoi_destroy": (None, [_vp]),
    "wavmetric_stoi_scratch_bytes": (_sz, [_vp, _i, _i64]),
    "wavmetric_stoi_pairs": (_i, [_vp, _fp, _fp, _fp, _fp, _i, _i64, _fp, _vp, _vp, _sz, _vp]),
}

#: every symbol include/lipfe.h declares (lip-reading front end: mouth video -> embeddings)
LIPFE_SYMBOLS = {
    "lipfe_abi_version": (_i, []),
    "lipfe_create": (_i, [C.POINTER(_vp), _i]),
    "lipfe_destroy": (None, [_vp]),
    "lipfe_last_error": (C.c_char_p, [_vp]),
    "lipfe_num_weights": (_i, [_vp]),
    "lipfe_weight_name": (C.c_char_p, [_vp, _i]),
    "lipfe_weight_numel": (_i64, [_vp, _i]),
    "lipfe_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "lipfe_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "lipfe_forward": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, C.c_float, _fp, _vp, _sz, _vp]),
    "lipfe_flops_per_stream": (C.c_double, [_i, _i, _i]),
    "lipfe_min_bytes_per_stream": (C.c_double, [_i, _i, _i]),
    "lipfe_weight_pack_bytes": (_sz, [_vp]),
}

#: every symbol include/specfe.h declares (spectral front end: STFT, inverse STFT, their adjoints, log-mel; behind a handle)
SPECFE_SYMBOLS = {
    "specfe_abi_version": (_i, []),
    "specfe_strerror": (C.c_char_p, [_i]),
    "specfe_create": (_i, [_i, _i, C.POINTER(_vp)]),
    "specfe_create_mel": (_i, [_i, _i, _i, _i, C.POINTER(_vp)]),
    "specfe_destroy": (None, [_vp]),
    "specfe_stft": (_i, [_vp, _fp, _i, _i64, _fp, _vp]),
    "specfe_stft_backward": (_i, [_vp, _fp, _i, _i64, _fp, _vp]),
    "specfe_istft": (_i, [_vp, _fp, _i, _i64, _i64, _fp, _vp]),
    "specfe_istft_backward": (_i, [_vp, _fp, _i, _i64, _i64, _fp, _vp]),
    "specfe_logmel": (_i, [_vp, _fp, _i, _i64, _fp, _vp]),
}

#: every symbol include/vfwave.h declares (VoiceFilter's waveform ends: analysis to magnitude + phasor, synthesis back; on a specfe handle)
VFWAVE_SYMBOLS = {
    "vfwave_abi_version": (_i, []),
    "vfwave_strerror": (C.c_char_p, [_i]),
    "vfwave_analysis": (_i, [_vp, _fp, _i, _i64, _fp, _fp, _vp]),
    "vfwave_synthesis": (_i, [_vp, _fp, _fp, _i, _i, _i64, _i64, _fp, _vp]),
}

#: every symbol include/vfilt.h declares (VoiceFilter separator: magnitude spectrogram + lip embeddings -> two masked spectrograms)
VFILT_SYMBOLS = {
    "vfilt_abi_version": (_i, []),
    "vfilt_create": (_i, [C.POINTER(_vp), _i, _i]),
    "vfilt_destroy": (None, [_vp]),
    "vfilt_last_error": (C.c_char_p, [_vp]),
    "vfilt_num_weights": (_i, [_vp]),
    "vfilt_weight_name": (C.c_char_p, [_vp, _i]),
    "vfilt_weight_numel": (_i64, [_vp, _i]),
    "vfilt_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "vfilt_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "vfilt_forward": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "vfilt_flops_per_item": (C.c_double, [_vp, _i, _i]),
    "vfilt_min_bytes_per_item": (C.c_double, [_vp, _i, _i]),
}

#: every symbol include/vfilt_train.h declares (VoiceFilter training step): _train_symbols' entries with shapes (B, W, Tv), the
#: two embeddings behind the mixture and the dropout's (ppm, seed) in train_forward; costs are counted per item
VFTRAIN_SYMBOLS = {
    "vftrain_abi_version": (_i, []),
    "vftrain_create": (_i, [C.POINTER(_vp), _i, _i]),
    "vftrain_destroy": (None, [_vp]),
    "vftrain_last_error": (C.c_char_p, [_vp]),
    "vftrain_num_weights": (_i, [_vp]),
    "vftrain_weight_name": (C.c_char_p, [_vp, _i]),
    "vftrain_weight_numel": (_i64, [_vp, _i]),
    "vftrain_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "vftrain_bind_grads": (_i, [_vp, C.POINTER(_fp), _i]),
    "vftrain_flat_offset": (_i64, [_vp, _i]),
    "vftrain_flat_numel": (_i64, [_vp]),
    "vftrain_workspace_bytes": (_sz, [_vp, _i, _i, _i]),
    "vftrain_train_forward": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _i, C.c_uint32, _fp, _fp, _vp, _sz, _vp]),
    "vftrain_train_backward": (_i, [_vp, _fp, _fp, _fp, _i, _i, _i, _fp, _fp, _vp, _sz, _vp]),
    "vftrain_tape_offset": (_i64, [_vp, _i, _i, _i, _i, _i]),
    "vftrain_clip_scratch_bytes": (_sz, [_vp]),
    "vftrain_grad_clip": (_i, [_vp, _fp, _i64, C.c_float, _vp, _sz, _fp, _vp]),
    "vftrain_adamw_step": (_i, [_vp, _fp, _fp, _fp, _i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i, _vp]),
    "vftrain_flops_per_item": (C.c_double, [_vp, _i, _i]),
}
VFTRAIN_ABI_VERSION = 1

#: every symbol include/lipsn.h declares (ShuffleNet-v2 lip reader: mouth video -> 1024-wide embeddings)
LIPSN_SYMBOLS = {
    "lipsn_abi_version": (_i, []),
    "lipsn_create": (_i, [C.POINTER(_vp), _i, _i]),
    "lipsn_destroy": (None, [_vp]),
    "lipsn_last_error": (C.c_char_p, [_vp]),
    "lipsn_num_weights": (_i, [_vp]),
    "lipsn_weight_name": (C.c_char_p, [_vp, _i]),
    "lipsn_weight_numel": (_i64, [_vp, _i]),
    "lipsn_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "lipsn_workspace_bytes": (_sz, [_vp, _i, _i, _i, _i]),
    "lipsn_forward": (_i, [_vp, _fp, _i, _i, _i, _i, _i, _i, _i, _i, C.c_float, C.c_float, _fp, _vp, _sz, _vp]),
    "lipsn_launches_per_forward": (_i, []),
    "lipsn_flops_per_stream": (C.c_double, [_i, _i, _i, _i]),
    "lipsn_min_bytes_per_stream": (C.c_double, [_i, _i, _i, _i]),
    "lipsn_weight_pack_bytes": (_sz, [_vp]),
}

_lib: Optional[C.CDLL] = None


def load() -> C.CDLL:
    """Load libdptnav.so and type every entry point; raises RuntimeError if unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    # PyTorch-ROCm ships its own HIP runtime; import it FIRST so that libdptnav resolves libamdhip64 to the
    # runtime torch already loaded -- device pointers and hipStream_t handles are only meaningful inside
    # one runtime instance.
    import torch  # noqa: F401
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built (run `python -c 'import __graft_entry__ as g; "
            f"g.build()'` at the repo root).  speech_separation_amd has no CPU/PyTorch fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in (list(SYMBOLS.items()) + list(CTASNET_SYMBOLS.items()) + list(DCTASNET_SYMBOLS.items())
                      + list(CTTRAIN_SYMBOLS.items()) + list(DCTTRAIN_SYMBOLS.items())
                              + list(DAVTRAIN_SYMBOLS.items()) + list(WAVLOSS_SYMBOLS.items())
                              + list(WAVMETRIC_SYMBOLS.items()) + list(LIPFE_SYMBOLS.items())
                              + list(SPECFE_SYMBOLS.items()) + list(VFILT_SYMBOLS.items())
                              + list(LIPSN_SYMBOLS.items()) + list(VFWAVE_SYMBOLS.items())
                              + list(VFTRAIN_SYMBOLS.items())):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"libdptnav.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    for fn, want, label in ((lib.dptnav_abi_version, ABI_VERSION, "libdptnav"),
                            (lib.ctasnet_abi_version, CTASNET_ABI_VERSION, "ctasnet"),
                            (lib.dctasnet_abi_version, DCTASNET_ABI_VERSION, "dctasnet"),
                            (lib.cttrain_abi_version, CTTRAIN_ABI_VERSION, "cttrain"),
                            (lib.dcttrain_abi_version, DCTTRAIN_ABI_VERSION, "dcttrain"),
                            (lib.davtrain_abi_version, DAVTRAIN_ABI_VERSION, "davtrain"),
                            (lib.wavloss_abi_version, WAVLOSS_ABI_VERSION, "wavloss"),
                            (lib.wavmetric_abi_version, WAVMETRIC_ABI_VERSION, "wavmetric"),
                            (lib.lipfe_abi_version, LIPFE_ABI_VERSION, "lipfe"),
                            (lib.specfe_abi_version, SPECFE_ABI_VERSION, "specfe"),
                            (lib.vfilt_abi_version, VFILT_ABI_VERSION, "vfilt"),
                            (lib.lipsn_abi_version, LIPSN_ABI_VERSION, "lipsn"),
                            (lib.vfwave_abi_version, VFWAVE_ABI_VERSION, "vfwave"),
                            (lib.vftrain_abi_version, VFTRAIN_ABI_VERSION, "vftrain")):
        if fn() != want:
            raise RuntimeError(f"{label} ABI {fn()} != binding {want}: rebuild")
    _lib = lib
    return lib
