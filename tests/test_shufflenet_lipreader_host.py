"""ShuffleNet-v2 lip reader, host layer (no GPU needed): the C ABI of include/lipsn.h (declared == bound == exported, plain
C99), the module's state_dict against the reference's key list (tests/golden/lipreader_shufflenet.npz, written by
tools/gen_golden_shufflenet.py), the fp64 restatement (tests/shufflenet_ref.py) against the reference's own fp64 outputs,
initialisation, init_lipreader's dispatch on the JSON's backbone_type, VoiceFilter with the reference's lip-reader config,
the refusals, the exports and the FLOP arithmetic against hand values."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest
import torch

import speech_separation_amd as ssa
from speech_separation_amd import _lib
from tests import shufflenet_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "lipsn.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "lipreader_shufflenet.npz")
SN_JSON = ('{"backbone_type": "shufflenet", "relu_type": "prelu", "tcn_dropout": 0.2, "tcn_dwpw": false, '
           '"tcn_kernel_size": [3], "tcn_num_layers": 4, "tcn_width_mult": 1, "width_mult": %s}')   # lrw_snv1x_tcn1x.json / snv05x


def _tag(width_mult):
    return "w10" if width_mult == 1.0 else "w05"


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(lipsn_\w+)\s*\(", src))
    assert declared == set(_lib.LIPSN_SYMBOLS), declared ^ set(_lib.LIPSN_SYMBOLS)
    m = re.search(r"#define LIPSN_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.LIPSN_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.lipsn_abi_version() == _lib.LIPSN_ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(lipsn_\w+)$", out, re.M))
    assert exported == set(_lib.LIPSN_SYMBOLS), exported ^ set(_lib.LIPSN_SYMBOLS)
    assert lib.lipsn_launches_per_forward() == 21      # fold, pack, stem, max-pool, 16 blocks, conv_last + pool


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("width_mult", [1.0, 0.5])
@pytest.mark.parametrize("relu_type,entries,floats", [("prelu", 337, 281), ("swish", 336, 280), ("relu", 336, 280)])
def test_module_state_dict_is_the_references_without_the_tcn(relu_type, entries, floats, width_mult):
    z = np.load(GOLDEN)
    keys = [str(k) for k in z[f"keys_{_tag(width_mult)}"]]           # the reference's, with prelu
    assert len(keys) == 337 and not any(k.startswith("tcn.") for k in keys)
    if relu_type != "prelu":
        keys.remove("frontend3D.2.weight")                           # the only entry relu_type adds: the trunk is ReLU
    m = ssa.ShuffleNetLipreading(relu_type=relu_type, width_mult=width_mult, extract_feats=True,
                                 tcn_options={"ignored": 1}, densetcn_options={"ignored": 1})
    assert m.backend_out == 1024 and m.frontend_nout == 24 and m.backbone_type == "shufflenet"
    sd = m.state_dict()
    assert list(sd) == keys and len(sd) == entries
    spec = R.shufflenet_state_dict_spec(relu_type, width_mult)       # its shapes were asserted against the reference
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, s) for k, s, _ in spec]
    assert sum(v.dtype == torch.float32 for v in sd.values()) == floats
    for k, v in sd.items():
        assert v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
    half = {1.0: 58, 0.5: 24}[width_mult]
    assert tuple(sd["trunk.0.0.banch2.5.weight"].shape) == (half, half, 1, 1)
    assert tuple(sd["trunk.1.0.weight"].shape) == (1024, 8 * half, 1, 1)
    if relu_type == "prelu":
        w = R.synthetic_shufflenet_weights(relu_type, width_mult, R.WEIGHT_SEED)
        assert R.weights_digest(w) == str(z[f"digest_{_tag(width_mult)}"])
        ckpt = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
        ckpt["tcn.tcn_output.weight"] = torch.zeros(500, 256)
        res = m.load_state_dict(ckpt, strict=False)
        assert res.missing_keys == [] and res.unexpected_keys == ["tcn.tcn_output.weight"]
        assert torch.equal(m.state_dict()["trunk.0.15.banch2.6.running_var"], ckpt["trunk.0.15.banch2.6.running_var"])
    assert not m.training and not m.train().training and not any(p.requires_grad for p in m.parameters())


def test_fp64_restatement_reproduces_the_references_fp64_outputs():
    """fp64 against fp64, per (stream, frame) row: pins the restatement, and through it every GPU comparison, to the
    reference's own Lipreading(backbone_type="shufflenet")."""
    z = np.load(GOLDEN)
    assert [int(s) for s in z["seeds"]] == [R.WEIGHT_SEED, R.INPUT_SEED]
    for i, (relu_type, width_mult, shape) in enumerate(R.GOLDEN_CASES):
        assert tuple(int(d) for d in z[f"shape{i}"]) == shape and float(z[f"width{i}"]) == width_mult
        ref = z[f"out{i}"]
        assert ref.dtype == np.float64 and ref.shape == (shape[0], shape[2], 1024)
        w = R.synthetic_shufflenet_weights(relu_type, width_mult, R.WEIGHT_SEED)
        got = R.run(w, R.synthetic_video(shape, R.INPUT_SEED + i), torch.float64)
        assert float(R.row_rel(got, ref).max()) <= 1e-10


def test_restatement_refuses_the_sizes_the_reference_cannot_pool():
    w = R.synthetic_shufflenet_weights("relu", 0.5, 0)
    with pytest.raises((ValueError, RuntimeError)):
        R.run(w, np.zeros((1, 1, 1, 64, 88), np.float32), torch.float32, relu_type="relu")
    with pytest.raises(ValueError):
        R.run(w, np.zeros((1, 1, 1, 161, 88), np.float32), torch.float32, relu_type="relu")


def test_fresh_module_follows_the_references_initialisation():
    torch.manual_seed(0)
    sd = ssa.ShuffleNetLipreading(relu_type="prelu", extract_feats=True).state_dict()
    assert torch.all(sd["frontend3D.2.weight"] == 0.25)
    assert torch.all(sd["trunk.0.4.banch2.1.weight"] == 1) and torch.all(sd["trunk.0.4.banch2.1.bias"] == 0)
    assert torch.all(sd["trunk.1.1.running_var"] == 1) and torch.all(sd["trunk.1.1.running_mean"] == 0)
    # N(0, 2 / (kernel volume * out_channels)): conv_last, a depthwise filter bank, the stem
    for key, n in (("trunk.1.0.weight", 1024), ("trunk.0.12.banch1.0.weight", 9 * 232), ("frontend3D.0.weight", 245 * 24)):
        std = float(sd[key].std())
        assert abs(std / (2.0 / n) ** 0.5 - 1) < 0.05, (key, std)
    m = ssa.ShuffleNetLipreading(relu_type="relu", width_mult=0.5, extract_feats=True)
    before = m.state_dict()["trunk.1.0.weight"].clone()
    m.reset_parameters()
    assert not torch.equal(before, m.state_dict()["trunk.1.0.weight"])


def test_exports_resolve():
    for name in ("ShuffleNetLipreadingEngine", "ShuffleNetLipreading", "Lipreading", "init_lipreader"):
        assert name in ssa.__all__ and getattr(ssa, name) is not None
    assert issubclass(ssa.ShuffleNetLipreadingEngine, ssa.LipreadingEngine)
    assert ssa.ShuffleNetLipreadingEngine.embed == 1024 and ssa.LipreadingEngine.embed == 512


@pytest.mark.parametrize("kw,named", [
    (dict(modality="audio"), "modality"), (dict(backbone_type="resnet"), "backbone_type"), (dict(width_mult=1.5), "width_mult"),
    (dict(width_mult=2.0), "width_mult"), (dict(use_boundary=True), "use_boundary"), (dict(extract_feats=False), "extract_feats"),
    (dict(), "extract_feats"), (dict(relu_type="gelu"), "relu_type")])
def test_unsupported_constructor_arguments_raise(kw, named):
    full = dict(dict(extract_feats=True), **kw) if kw else {}
    with pytest.raises(NotImplementedError, match=named):
        ssa.ShuffleNetLipreading(**full)


def test_the_resnet_class_still_refuses_shufflenet_and_names_the_new_class():
    with pytest.raises(NotImplementedError, match="backbone_type.*ShuffleNetLipreading"):
        ssa.Lipreading(backbone_type="shufflenet", extract_feats=True)


def test_cpu_tensors_raise():
    m = ssa.ShuffleNetLipreading(relu_type="swish", width_mult=0.5, extract_feats=True)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(torch.zeros(1, 1, 2, 88, 88), lengths=[2])
    with pytest.raises(RuntimeError, match="no CPU"):
        m.forward_window(torch.zeros(1, 2, 96, 96), (4, 4, 88, 88))


@pytest.mark.parametrize("width_mult", [1.0, 0.5])
def test_init_lipreader_dispatches_on_the_backbone_type(tmp_path, width_mult):
    w = R.synthetic_shufflenet_weights("prelu", width_mult, 3)
    ckpt = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    ckpt["tcn.tcn_trunk.network.0.net.0.weight"] = torch.zeros(256, 1024, 3)
    ckpt["tcn.tcn_output.bias"] = torch.zeros(500)
    torch.save({"model_state_dict": ckpt, "epoch_idx": 7}, tmp_path / "lip.pth")
    (tmp_path / "lip.json").write_text(SN_JSON % width_mult)
    m = ssa.init_lipreader(str(tmp_path / "lip.json"), str(tmp_path / "lip.pth"))
    assert isinstance(m, ssa.ShuffleNetLipreading) and m.relu_type == "prelu" and m.width_mult == width_mult and m.extract_feats
    sd = m.state_dict()
    assert len(sd) == 337 and not any(k.startswith("tcn.") for k in sd)
    for k, v in sd.items():
        assert torch.equal(v, ckpt[k]), k
    with pytest.raises(FileNotFoundError):
        ssa.init_lipreader(str(tmp_path / "lip.json"), str(tmp_path / "absent.pth"))


def test_voicefilter_constructs_with_the_references_lipreader_config(tmp_path):
    w = R.synthetic_shufflenet_weights("prelu", 1.0, 4)
    ckpt = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    torch.save({"model_state_dict": ckpt}, tmp_path / "lrw_snv1x_tcn1x.pth")
    (tmp_path / "lrw_snv1x_tcn1x.json").write_text(SN_JSON % 1.0)
    vf = ssa.VoiceFilter(201, str(tmp_path / "lrw_snv1x_tcn1x.pth"), str(tmp_path / "lrw_snv1x_tcn1x.json"))
    assert vf.embed_size == 1024 and isinstance(vf.lipreader, ssa.ShuffleNetLipreading)
    sd = vf.state_dict()
    keys = list(sd)
    assert len(keys) == 337 + 82
    assert keys[:337] == ["lipreader." + k for k in ckpt] and not any(k.startswith("lipreader.") for k in keys[337:])
    assert tuple(sd["gru.weight_ih_l0"].shape)[1] == 1024
    assert torch.equal(sd["lipreader.trunk.1.0.weight"], ckpt["trunk.1.0.weight"])
    # a checkpoint of the whole model, as the reference saves it, loads strictly
    vf2 = ssa.VoiceFilter(201, str(tmp_path / "lrw_snv1x_tcn1x.pth"), str(tmp_path / "lrw_snv1x_tcn1x.json"))
    vf2.load_state_dict({k: v.clone() for k, v in sd.items()}, strict=True)
    # the ResNet lip reader's width is still refused at the default embed_size
    with pytest.raises(ValueError, match="embed_size=512"):
        ssa.VoiceFilter(201, lipreader=ssa.Lipreading(relu_type="swish", extract_feats=True))


def test_flops_against_hand_values():
    lib = _lib.load()
    assert R.out_hw(88, 88) == [(44, 44), (22, 22), (11, 11), (6, 6), (3, 3)]
    assert R.out_hw(65, 72) == [(33, 36), (17, 18), (9, 9), (5, 5), (3, 3)]
    assert R.out_hw(97, 66)[-1] == (4, 3) and R.out_hw(160, 129)[-1] == (5, 5) and R.out_hw(161, 88)[-1][0] == 6
    # multiply-accumulates per 88 x 88 frame at width 1.0, by hand.  A stride-2 block from I channels on p_in positions to
    # halves of h on p_out: banch1 p_out*I*9 + p_out*I*h, banch2 p_in*I*h + p_out*h*9 + p_out*h*h; a stride-1 block
    # p*(2*h*h + 9*h); conv_last on the whole 3 x 3 map
    stem = 44 * 44 * 24 * 245
    s2 = (121 * 24 * 9 + 121 * 24 * 58) + (484 * 24 * 58 + 121 * 58 * 9 + 121 * 58 * 58) + 3 * 121 * (2 * 58 * 58 + 9 * 58)
    s3 = (36 * 116 * 9 + 36 * 116 * 116) + (121 * 116 * 116 + 36 * 116 * 9 + 36 * 116 * 116) + 7 * 36 * (2 * 116 * 116 + 9 * 116)
    s4 = (9 * 232 * 9 + 9 * 232 * 232) + (36 * 232 * 232 + 9 * 232 * 9 + 9 * 232 * 232) + 3 * 9 * (2 * 232 * 232 + 9 * 232)
    last = 9 * 464 * 1024
    assert stem == 11_383_680
    per_frame = stem + s2 + s3 + s4 + last
    assert lib.lipsn_flops_per_stream(2, 50, 88, 88) == 2.0 * 50 * per_frame == R.flops_per_stream(1.0, 50, 88, 88)
    assert 69e6 < 2 * per_frame < 72e6                         # about a ninth of the ResNet-18 front end's 632 MFLOP
    for wx2, wm in ((1, 0.5), (2, 1.0)):
        for T, H, W in ((3, 65, 72), (2, 97, 66), (1, 160, 129)):
            assert lib.lipsn_flops_per_stream(wx2, T, H, W) == R.flops_per_stream(wm, T, H, W)
    for bad in ((2, 50, 64, 88), (2, 50, 88, 161), (2, 0, 88, 88), (3, 50, 88, 88), (4, 50, 88, 88)):
        assert lib.lipsn_flops_per_stream(*bad) == 0.0 and lib.lipsn_min_bytes_per_stream(*bad) == 0.0
    assert lib.lipsn_min_bytes_per_stream(2, 50, 88, 88) > 4.0 * 50 * (88 * 88 + 2 * 44 * 44 * 24)
