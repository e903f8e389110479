"""CPU checks of the masked DPTN separator (DPTNEncDec, model/dptn.yaml): Python surface, checkpoint spec, C-ABI field,
configuration checks, and the numpy restatement (tests/mask_tail_ref.py) against the reference's own fixtures
(tools/gen_golden_mask.py)."""
from __future__ import annotations

import ctypes as C
import inspect
import os

import numpy as np
import pytest
import torch

from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTN_MASK, DPTNConfig, num_parameters, state_dict_spec
from tests import mask_tail_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ctor_kw(cfg):
    return {k: v for k, v in cfg.to_dict().items() if k not in ("audio_only", "arch", "video_emb_size", "hidden_video")}


def test_import_and_export():
    import speech_separation_amd as pkg
    from speech_separation_amd import DPTNEncDec
    assert "DPTNEncDec" in pkg.__all__ and "DPTN_MASK" in pkg.__all__
    assert DPTNEncDec().cfg.arch == "dptn_mask"


def test_constructor_defaults_match_reference():
    """dptn.py:154-165."""
    from speech_separation_amd import DPTNEncDec
    want = dict(num_features=64, kernel_size_enc=2, hidden_dim=32, num_blocks=6, chunk_size=10, step_size=5, num_heads=4,
                dropout=0.1, bidir=True)
    sig = inspect.signature(DPTNEncDec.__init__)
    assert {k: v.default for k, v in sig.parameters.items() if k != "self"} == want
    assert "mix" in inspect.signature(DPTNEncDec.forward).parameters


def test_dptn_yaml_spec_counts():
    """model/dptn.yaml: 225 state_dict keys, 2 801 537 parameters, the reference's order at the tail."""
    spec = state_dict_spec(DPTN_MASK)
    assert len(spec) == 225
    assert num_parameters(DPTN_MASK) == 2_801_537
    keys = [k for k, _ in spec]
    assert keys[0] == "encoder.weight" and keys[-1] == "decoder.weight"
    assert keys[-8:-1] == ["dprnn.speakers_separation.0.weight", "dprnn.speakers_separation.1.weight",
                           "dprnn.speakers_separation.1.bias", "dprnn.output_gate.0.weight", "dprnn.output_gate.0.bias",
                           "dprnn.output.0.weight", "dprnn.output.0.bias"]
    assert not any("postprocessing" in k for k in keys)
    assert (DPTN_MASK.num_features, DPTN_MASK.kernel_size_enc, DPTN_MASK.hidden_dim, DPTN_MASK.num_blocks,
            DPTN_MASK.chunk_size, DPTN_MASK.step_size, DPTN_MASK.num_heads) == (64, 7, 128, 6, 150, 75, 4)
    assert DPTN_MASK.blocks == "dptn" and DPTN_MASK.mask_tail and DPTN_MASK.audio_only


def test_module_keys_shapes_and_strict_load(golden):
    """The fixture's weights are the reference model's state_dict (tools/gen_golden_mask.py checks the order against the
    imported reference): the module's keys and shapes equal them, and they load strictly."""
    from speech_separation_amd import DPTNEncDec
    cfg, z = golden("mask_tiny")
    sd = {k[2:]: v for k, v in z.items() if k.startswith("w.")}
    model = DPTNEncDec(**_ctor_kw(cfg))
    assert [(k, tuple(v.shape)) for k, v in model.state_dict().items()] == [(k, v.shape) for k, v in sd.items()]
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    full = DPTNEncDec(**_ctor_kw(DPTN_MASK))
    assert [(k, tuple(v.shape)) for k, v in full.state_dict().items()] == state_dict_spec(DPTN_MASK)
    assert sum(p.numel() for p in full.parameters()) == 2_801_537


def test_new_convs_use_conv1d_default_init():
    """output / output_gate: nn.Conv1d(N, N, 1) defaults, U(+-1/sqrt(N)) for weight and bias."""
    from speech_separation_amd import DPTNEncDec
    torch.manual_seed(0)
    model = DPTNEncDec(num_features=64)
    bound = 1.0 / np.sqrt(64)
    for name in ("output", "output_gate"):
        w = getattr(model.dprnn, name)._modules["0"].weight.detach()
        b = getattr(model.dprnn, name)._modules["0"].bias.detach()
        for t in (w, b):
            assert float(t.abs().max()) <= bound and float(t.abs().max()) > 0.8 * bound
            assert abs(float(t.mean())) < 0.1 * bound * (1 + 10 / np.sqrt(t.numel()))


def test_str_ends_with_parameter_counts():
    from speech_separation_amd import DPTNEncDec
    lines = str(DPTNEncDec(**_ctor_kw(DPTN_MASK))).splitlines()
    assert lines[-2:] == ["All parameters: 2801537", "Trainable parameters: 2801537"]


def test_header_and_binding_carry_mask_tail():
    from speech_separation_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dptnav.h")).read()
    assert "int32_t mask_tail;" in hdr
    assert "#define DPTNAV_ABI_VERSION 4" in hdr and _lib.ABI_VERSION == 4
    assert [n for n, _ in _lib.DptnavConfig._fields_][-2:] == ["arch", "mask_tail"]
    assert C.sizeof(_lib.DptnavConfig) == 13 * 4


def test_invalid_combinations_rejected_by_spec():
    with pytest.raises(ValueError, match="audio-only"):
        DPTNConfig(**{**DPTN_MASK.to_dict(), "audio_only": False})
    with pytest.raises(ValueError, match="arch"):
        DPTNConfig(arch="mask")


@pytest.mark.parametrize("arch,audio_only", [(1, 1), (0, 0), (1, 0)])
def test_invalid_combinations_rejected_by_library(arch, audio_only):
    """dptnav_create checks the configuration before it looks for a device: runs on a box without one."""
    from speech_separation_amd import _lib
    lib = _lib.load()
    c = _lib.DptnavConfig(64, 512, 64, 7, 128, 1, 150, 75, 4, 1, audio_only, arch, 1)
    h = C.c_void_p()
    rc = lib.dptnav_create(C.byref(c), C.byref(h))
    assert rc == 1 and not h.value
    assert b"mask_tail" in lib.dptnav_last_error(None)


def test_restatement_reproduces_reference_fixture(golden):
    """tests/mask_tail_ref.py (oracle head / blocks / decoder + the restated masked tail) against the reference's taps and
    outputs, fp64, including the bias-only padded frames."""
    cfg, z = golden("mask_tiny")
    sd = {k[2:]: v for k, v in z.items() if k.startswith("w.")}
    taps = {}
    out = R.forward(cfg, sd, z["in.mix"], dtype=np.float64, taps=taps)
    for k in ("s1_pred", "s2_pred"):
        assert O.agreement_db(out[k], z["tap." + k]) > 100, k
    for k in ("ola", "masks", "masked"):
        assert taps[k].shape == z["tap." + k].shape, k
        assert O.agreement_db(taps[k], z["tap." + k]) > 100, k
    # padded frames: u = 0 there, so m = ReLU(tanh(b_out) sigmoid(b_gate)), the same for every padded frame
    left, L, ola = taps["left"], taps["masks"].shape[-1], taps["ola"].shape[-1]
    pads = [t for t in range(L) if t < left or t >= left + ola]
    assert pads, "the fixture's shape must have padded frames"
    bias_only = np.maximum(np.tanh(sd["dprnn.output.0.bias"].astype(np.float64))
                           * O._sigmoid(sd["dprnn.output_gate.0.bias"].astype(np.float64)), 0.0)
    ref_m = z["tap.masks"]
    for t in pads:
        np.testing.assert_allclose(ref_m[:, :, :, t], np.broadcast_to(bias_only[None, None], ref_m.shape[:3]), rtol=1e-5, atol=1e-6)
    assert np.abs(z["tap.masked"][:, :, :, pads]).max() > 0           # they reach the decoder
    # the tap table the GPU test compares, restated from the fixture
    D = R.decoder_taps(z["tap.masked"].astype(np.float64), sd["decoder.weight"].astype(np.float64))
    assert D.shape == (2, 2, L, 8) and not D[..., cfg.kernel_size_enc:].any()


@pytest.mark.parametrize("name", ["mask_mid", "mask_mid128", "mask_full"])
def test_forward_fixtures_are_consistent(golden, name):
    """Each real-size fixture names its configuration and carries outputs and strided tail taps of the expected shape."""
    cfg, z = golden(name)
    B, T, _ = (int(v) for v in z["shape"])
    assert cfg.arch == "dptn_mask" and cfg.audio_only
    for k in ("s1_pred", "s2_pred"):
        assert z["tap." + k].shape == (B, T) and np.isfinite(z["tap." + k]).all()
    assert sum(k.endswith((".ola", ".masks", ".masked")) for k in z) == 3
