"""Lip-reading front end, host layer (no GPU needed): the C ABI of include/lipfe.h (declared == bound == exported, plain
C99), the module's state_dict against the reference's key list (fixtures written by tools/gen_golden_lipreader.py), the
exports, the refusals, the fp64 restatement (tests/lipreader_ref.py) against the reference's own fp64 outputs, and the
spatial-size / FLOP arithmetic against hand values."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest
import torch

import speech_separation_amd as ssa
from speech_separation_amd import _lib
from tests import lipreader_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lipfe.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(lipfe_\w+)\s*\(", src))
    assert declared == set(_lib.LIPFE_SYMBOLS), declared ^ set(_lib.LIPFE_SYMBOLS)
    m = re.search(r"#define LIPFE_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.LIPFE_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.lipfe_abi_version() == _lib.LIPFE_ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(lipfe_\w+)$", out, re.M))
    assert exported == set(_lib.LIPFE_SYMBOLS), exported ^ set(_lib.LIPFE_SYMBOLS)
    for want in ("lipfe_abi_version", "lipfe_create", "lipfe_destroy", "lipfe_last_error", "lipfe_num_weights",
                 "lipfe_weight_name", "lipfe_weight_numel", "lipfe_bind_weights", "lipfe_workspace_bytes", "lipfe_forward",
                 "lipfe_flops_per_stream", "lipfe_min_bytes_per_stream"):
        assert want in declared, want


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("relu_type,entries", [("swish", 120), ("prelu", 137)])
def test_module_state_dict_is_the_references_without_the_tcn(relu_type, entries):
    z = np.load(os.path.join(GOLDEN, f"lipreader_{relu_type}.npz"))
    keys = [str(k) for k in z["keys"]]
    assert len(keys) == entries and not any(k.startswith("tcn.") for k in keys)
    m = ssa.Lipreading(relu_type=relu_type, extract_feats=True, tcn_options={"ignored": 1}, densetcn_options={"ignored": 1})
    sd = m.state_dict()
    assert list(sd) == keys
    spec = R.lipreader_state_dict_spec(relu_type)      # its shapes were asserted against the reference when the fixture was made
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, s) for k, s, _ in spec]
    for k, v in sd.items():
        assert v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
    w = R.synthetic_lipreader_weights(relu_type, R.WEIGHT_SEED)
    assert R.weights_digest(w) == str(z["digest"])
    # a checkpoint written for the reference: tcn.* entries on top, loaded with strict=False
    ckpt = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    ckpt["tcn.tcn_output.weight"] = torch.zeros(500, 768)
    res = m.load_state_dict(ckpt, strict=False)
    assert res.missing_keys == [] and res.unexpected_keys == ["tcn.tcn_output.weight"]
    assert torch.equal(m.state_dict()["trunk.layer4.1.bn2.running_var"], ckpt["trunk.layer4.1.bn2.running_var"])
    assert not m.training and not m.train().training and not any(p.requires_grad for p in m.parameters())


def test_fresh_module_follows_the_references_initialisation():
    torch.manual_seed(0)
    sd = ssa.Lipreading(relu_type="prelu", extract_feats=True).state_dict()
    assert torch.all(sd["trunk.layer1.0.relu1.weight"] == 0.25) and torch.all(sd["frontend3D.2.weight"] == 0.25)
    assert torch.all(sd["trunk.layer2.0.bn1.weight"] == 1) and torch.all(sd["trunk.layer2.0.bn1.bias"] == 0)
    assert torch.all(sd["frontend3D.1.running_var"] == 1) and torch.all(sd["frontend3D.1.running_mean"] == 0)
    std = float(sd["trunk.layer3.1.conv2.weight"].std())
    assert abs(std / (2.0 / (9 * 256)) ** 0.5 - 1) < 0.02


def test_exports_resolve():
    for name in ("LipreadingEngine", "Lipreading", "init_lipreader", "VideoSSModel", "make_embeddings"):
        assert name in ssa.__all__ and getattr(ssa, name) is not None


@pytest.mark.parametrize("kw,named", [
    (dict(modality="audio"), "modality"), (dict(backbone_type="shufflenet"), "backbone_type"),
    (dict(use_boundary=True), "use_boundary"), (dict(extract_feats=False), "extract_feats"), (dict(), "extract_feats"),
    (dict(relu_type="gelu"), "relu_type")])
def test_unsupported_constructor_arguments_raise(kw, named):
    full = dict(dict(extract_feats=True), **kw) if kw else {}
    with pytest.raises(NotImplementedError, match=named):
        ssa.Lipreading(**full)


def test_cpu_tensors_raise():
    m = ssa.Lipreading(relu_type="swish", extract_feats=True)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(1, 1, 2, 16, 16), lengths=[2])


def test_init_lipreader_reads_the_json_and_the_checkpoint(tmp_path):
    w = R.synthetic_lipreader_weights("prelu", 3)
    ckpt = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    ckpt["tcn.mb_ms_tcn.tcn_output.bias"] = torch.zeros(500)
    torch.save({"model_state_dict": ckpt, "epoch_idx": 7}, tmp_path / "lip.pth")
    (tmp_path / "lip.json").write_text('{"backbone_type": "resnet", "relu_type": "prelu", "width_mult": 1.0, '
                                       '"tcn_num_layers": 4, "tcn_kernel_size": [3, 5, 7], "tcn_dropout": 0.2, '
                                       '"tcn_dwpw": false, "tcn_width_mult": 1}')
    m = ssa.init_lipreader(str(tmp_path / "lip.json"), str(tmp_path / "lip.pth"))
    assert m.relu_type == "prelu" and m.extract_feats
    for k, v in m.state_dict().items():
        assert torch.equal(v, ckpt[k]), k


def _rows_rel(got, ref):
    return float(R.row_rel(got, ref).max())


@pytest.mark.parametrize("relu_type", ["swish", "prelu"])
def test_fp64_restatement_reproduces_the_references_fp64_outputs(relu_type):
    """fp64 against fp64, per (stream, frame) row: pins the restatement, and through it every GPU comparison, to the
    reference's own Lipreading."""
    z = np.load(os.path.join(GOLDEN, f"lipreader_{relu_type}.npz"))
    assert [int(s) for s in z["seeds"]] == [R.WEIGHT_SEED, R.INPUT_SEED]
    w = R.synthetic_lipreader_weights(relu_type, R.WEIGHT_SEED)
    for i, shape in enumerate(R.GOLDEN_SHAPES):
        assert tuple(int(d) for d in z[f"shape{i}"]) == shape
        ref = z[f"out{i}"]
        assert ref.dtype == np.float64 and ref.shape == (shape[0], shape[2], 512)
        got = R.run(w, R.synthetic_video(shape, R.INPUT_SEED + i), torch.float64)
        assert _rows_rel(got, ref) <= 1e-10


def test_fp64_restatement_reproduces_the_preprocessing_fixture():
    z = np.load(os.path.join(GOLDEN, "lipreader_preproc.npz"))
    assert tuple(int(d) for d in z["clip_shape"]) == R.PREPROC_SHAPE == (3, 97, 96)
    clip = R.synthetic_clip(R.PREPROC_SHAPE, R.INPUT_SEED)
    assert clip.min() >= 0 and clip.max() <= 255 and np.array_equal(clip, np.round(clip))
    w = R.synthetic_lipreader_weights("swish", R.WEIGHT_SEED)
    window, affine = R.preproc_window_affine()
    assert window == (4, 4, 88, 88)           # (97 - 88) // 2, (96 - 88) // 2
    got = R.run(w, clip[None, None], torch.float64, window=window, affine=affine)
    assert _rows_rel(got, z["out"]) <= 1e-10


def test_spatial_sizes_and_flops_against_hand_values():
    lib = _lib.load()
    assert R.out_hw(88, 88) == [(44, 44), (22, 22), (11, 11), (6, 6), (3, 3)]
    assert R.out_hw(33, 47) == [(17, 24), (9, 12), (5, 6), (3, 3), (2, 2)]
    # multiply-accumulates per frame, by hand: stem 44*44*64*245; a layer of P planes on p positions with I inputs costs
    # p*P*9*(I + 3P) for its four 3x3 convs and p*P*I for the 1x1 downsample
    stem = 44 * 44 * 64 * 245
    trunk = (484 * 64 * 9 * 256) + (121 * 128 * 64 + 121 * 128 * 9 * 448) + (36 * 256 * 128 + 36 * 256 * 9 * 896) \
        + (9 * 512 * 256 + 9 * 512 * 9 * 1792)
    assert stem == 30_356_480 and trunk == 285_802_496
    assert lib.lipfe_flops_per_stream(50, 88, 88) == 2.0 * 50 * (stem + trunk) == R.flops_per_stream(50, 88, 88)
    assert abs(2 * lib.lipfe_flops_per_stream(50, 88, 88) / 1e9 - 63.2) < 0.1      # the front end's share of profiler.py, 2 streams
    small = 17 * 24 * 64 * 245 + (108 * 64 * 9 * 256) + (30 * 128 * 64 + 30 * 128 * 9 * 448) \
        + (9 * 256 * 128 + 9 * 256 * 9 * 896) + (4 * 512 * 256 + 4 * 512 * 9 * 1792)
    assert lib.lipfe_flops_per_stream(3, 33, 47) == 2.0 * 3 * small == R.flops_per_stream(3, 33, 47)
    for bad in ((50, 7, 88), (50, 88, 257), (0, 88, 88)):
        assert lib.lipfe_flops_per_stream(*bad) == 0.0 and lib.lipfe_min_bytes_per_stream(*bad) == 0.0
    assert lib.lipfe_min_bytes_per_stream(50, 88, 88) > 4.0 * 50 * (88 * 88 + 2 * 44 * 44 * 64)
