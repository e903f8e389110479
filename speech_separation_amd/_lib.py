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

#: name -> (restype, argtypes): every symbol include/ctasnet.h declares (Conv-TasNet forward, same shared object)
CTASNET_SYMBOLS = {
    "ctasnet_abi_version": (_i, []),
    "ctasnet_create": (_i, [C.POINTER(_vp)]),
    "ctasnet_destroy": (None, [_vp]),
    "ctasnet_last_error": (C.c_char_p, [_vp]),
    "ctasnet_num_weights": (_i, [_vp]),
    "ctasnet_weight_name": (C.c_char_p, [_vp, _i]),
    "ctasnet_weight_numel": (_i64, [_vp, _i]),
    "ctasnet_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "ctasnet_frames": (_i64, [_i64]),
    "ctasnet_out_len": (_i64, [_i64]),
    "ctasnet_workspace_bytes": (_sz, [_vp, _i, _i64]),
    "ctasnet_forward": (_i, [_vp, _fp, _i, _i64, _fp, _fp, _vp, _sz, _vp]),
    "ctasnet_flops_per_mixture": (C.c_double, [_vp, _i64]),
    "ctasnet_min_bytes_per_mixture": (C.c_double, [_vp, _i64]),
}

DCTASNET_ABI_VERSION = 1

#: name -> (restype, argtypes): every symbol include/dctasnet.h declares (deep Conv-TasNet forward, same shared object)
DCTASNET_SYMBOLS = {
    "dctasnet_abi_version": (_i, []),
    "dctasnet_create": (_i, [C.POINTER(_vp), _i]),
    "dctasnet_destroy": (None, [_vp]),
    "dctasnet_last_error": (C.c_char_p, [_vp]),
    "dctasnet_num_weights": (_i, [_vp]),
    "dctasnet_weight_name": (C.c_char_p, [_vp, _i]),
    "dctasnet_weight_numel": (_i64, [_vp, _i]),
    "dctasnet_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "dctasnet_frames": (_i64, [_i64]),
    "dctasnet_out_len": (_i64, [_i64]),
    "dctasnet_workspace_bytes": (_sz, [_vp, _i, _i64, _i]),
    "dctasnet_forward": (_i, [_vp, _fp, _fp, _fp, _i, _i64, _i, _fp, _fp, _vp, _sz, _vp]),
    "dctasnet_flops_per_mixture": (C.c_double, [_vp, _i64]),
    "dctasnet_min_bytes_per_mixture": (C.c_double, [_vp, _i64]),
    "dctasnet_weight_pack_bytes": (_sz, [_vp]),
}

CTTRAIN_ABI_VERSION = 1

#: name -> (restype, argtypes): every symbol include/ctasnet_train.h declares (Conv-TasNet training step, same shared object)
CTTRAIN_SYMBOLS = {
    "cttrain_abi_version": (_i, []),
    "cttrain_create": (_i, [C.POINTER(_vp)]),
    "cttrain_destroy": (None, [_vp]),
    "cttrain_last_error": (C.c_char_p, [_vp]),
    "cttrain_num_weights": (_i, [_vp]),
    "cttrain_weight_name": (C.c_char_p, [_vp, _i]),
    "cttrain_weight_numel": (_i64, [_vp, _i]),
    "cttrain_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "cttrain_bind_grads": (_i, [_vp, C.POINTER(_fp), _i]),
    "cttrain_flat_offset": (_i64, [_vp, _i]),
    "cttrain_flat_numel": (_i64, [_vp]),
    "cttrain_frames": (_i64, [_i64]),
    "cttrain_out_len": (_i64, [_i64]),
    "cttrain_workspace_bytes": (_sz, [_vp, _i, _i64]),
    "cttrain_train_forward": (_i, [_vp, _fp, _i, _i64, _fp, _fp, _vp, _sz, _vp]),
    "cttrain_train_backward": (_i, [_vp, _fp, _i, _i64, _fp, _fp, _vp, _sz, _vp]),
    "cttrain_tape_offset": (_i64, [_vp, _i, _i64, _i, _i]),
    "cttrain_clip_scratch_bytes": (_sz, [_vp]),
    "cttrain_grad_clip": (_i, [_vp, _fp, _i64, C.c_float, _vp, _sz, _fp, _vp]),
    "cttrain_adamw_step": (_i, [_vp, _fp, _fp, _fp, _i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i,
                                _vp]),
    "cttrain_flops_per_mixture": (C.c_double, [_vp, _i64]),
}

DCTTRAIN_ABI_VERSION = 1

#: name -> (restype, argtypes): every symbol include/dctasnet_train.h declares (deep Conv-TasNet training step, same shared object)
DCTTRAIN_SYMBOLS = {
    "dcttrain_abi_version": (_i, []),
    "dcttrain_create": (_i, [C.POINTER(_vp), _i]),
    "dcttrain_destroy": (None, [_vp]),
    "dcttrain_last_error": (C.c_char_p, [_vp]),
    "dcttrain_num_weights": (_i, [_vp]),
    "dcttrain_weight_name": (C.c_char_p, [_vp, _i]),
    "dcttrain_weight_numel": (_i64, [_vp, _i]),
    "dcttrain_bind_weights": (_i, [_vp, C.POINTER(_fp), _i]),
    "dcttrain_bind_grads": (_i, [_vp, C.POINTER(_fp), _i]),
    "dcttrain_flat_offset": (_i64, [_vp, _i]),
    "dcttrain_flat_numel": (_i64, [_vp]),
    "dcttrain_frames": (_i64, [_i64]),
    "dcttrain_out_len": (_i64, [_i64]),
    "dcttrain_workspace_bytes": (_sz, [_vp, _i, _i64]),
    "dcttrain_train_forward": (_i, [_vp, _fp, _i, _i64, _fp, _fp, _vp, _sz, _vp]),
    "dcttrain_train_backward": (_i, [_vp, _fp, _i, _i64, _fp, _fp, _vp, _sz, _vp]),
    "dcttrain_tape_offset": (_i64, [_vp, _i, _i64, _i, _i]),
    "dcttrain_clip_scratch_bytes": (_sz, [_vp]),
    "dcttrain_grad_clip": (_i, [_vp, _fp, _i64, C.c_float, _vp, _sz, _fp, _vp]),
    "dcttrain_adamw_step": (_i, [_vp, _fp, _fp, _fp, _i64, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, _i,
                                _vp]),
    "dcttrain_flops_per_mixture": (C.c_double, [_vp, _i64]),
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
                      + list(CTTRAIN_SYMBOLS.items()) + list(DCTTRAIN_SYMBOLS.items())):
        try:
            fn = getattr(lib, name)
        except AttributeError as e:
            raise RuntimeError(f"libdptnav.so does not export {name}") from e
        fn.restype = res
        fn.argtypes = args
    if lib.dptnav_abi_version() != ABI_VERSION:
        raise RuntimeError(f"libdptnav ABI {lib.dptnav_abi_version()} != binding {ABI_VERSION}: rebuild")
    if lib.ctasnet_abi_version() != CTASNET_ABI_VERSION:
        raise RuntimeError(f"ctasnet ABI {lib.ctasnet_abi_version()} != binding {CTASNET_ABI_VERSION}: rebuild")
    if lib.dctasnet_abi_version() != DCTASNET_ABI_VERSION:
        raise RuntimeError(f"dctasnet ABI {lib.dctasnet_abi_version()} != binding {DCTASNET_ABI_VERSION}: rebuild")
    if lib.cttrain_abi_version() != CTTRAIN_ABI_VERSION:
        raise RuntimeError(f"cttrain ABI {lib.cttrain_abi_version()} != binding {CTTRAIN_ABI_VERSION}: rebuild")
    if lib.dcttrain_abi_version() != DCTTRAIN_ABI_VERSION:
        raise RuntimeError(f"dcttrain ABI {lib.dcttrain_abi_version()} != binding {DCTTRAIN_ABI_VERSION}: rebuild")
    _lib = lib
    return lib
