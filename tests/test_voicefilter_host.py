"""VoiceFilter, host layer (no GPU needed): the C ABI of include/vfilt.h (declared == bound == exported, plain C99), the
module's state_dict against the reference's 82 keys (fixture written by tools/gen_golden_voicefilter.py), the fp64
restatement (tests/voicefilter_ref.py) against the reference's own fp64 outputs, that the seeded weights and inputs keep the
network alive, the get_magnitude formula of the restatement against a hand-made DFT and the package's own clamp / log
arithmetic against the restatement, the video preprocessing in front of a caller's lip reader, and the module's mode handling."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest
import torch

import speech_separation_amd as ssa
from speech_separation_amd import _lib
from tests import voicefilter_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vfilt.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "voicefilter_small.npz")


def _torch_sd(w):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(vfilt_\w+)\s*\(", src)) - {"vfilt_ctx"}
    assert declared == set(_lib.VFILT_SYMBOLS), declared ^ set(_lib.VFILT_SYMBOLS)
    m = re.search(r"#define VFILT_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.VFILT_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.vfilt_abi_version() == _lib.VFILT_ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(vfilt_\w+)$", out, re.M))
    assert exported == set(_lib.VFILT_SYMBOLS), exported ^ set(_lib.VFILT_SYMBOLS)
    for want in ("vfilt_abi_version", "vfilt_create", "vfilt_destroy", "vfilt_last_error", "vfilt_num_weights",
                 "vfilt_weight_name", "vfilt_weight_numel", "vfilt_bind_weights", "vfilt_workspace_bytes", "vfilt_forward",
                 "vfilt_flops_per_item", "vfilt_min_bytes_per_item"):
        assert want in declared, want


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_spec_is_the_references_82_keys_and_the_module_loads_them_strictly():
    z = np.load(GOLDEN)
    keys = [str(k) for k in z["keys"]]
    assert len(keys) == 82
    spec = ssa.voicefilter_state_dict_spec(201)
    assert [k for k, _, _ in spec] == keys
    assert [(k, s) for k, s, _ in spec] == [(k, s) for k, s, _ in R.voicefilter_state_dict_spec(201)]   # asserted against the
    assert sum(k.endswith("num_batches_tracked") for k in keys) == 8                                    # reference at generation
    assert sum("_reverse" in k for k in keys) == 8
    assert dict((k, s) for k, s, _ in spec)["cnn_layers.25.weight"] == (64, 64, 5, 5)
    assert dict((k, s) for k, s, _ in ssa.voicefilter_state_dict_spec(40, 512))["gru.weight_ih_l0_reverse"] == (120, 512)
    m = ssa.VoiceFilter(201)
    sd = m.state_dict()
    assert list(sd) == keys
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == [(k, s) for k, s, _ in spec]
    for k, v in sd.items():
        assert v.dtype == (torch.int64 if k.endswith("num_batches_tracked") else torch.float32), k
    w = R.synthetic_voicefilter_weights(201, 1024, R.WEIGHT_SEED)
    assert R.weights_digest(w) == str(z["digest0"])
    m.load_state_dict(_torch_sd(w), strict=True)
    assert torch.equal(m.state_dict()["cnn_layers.29.running_var"], torch.from_numpy(w["cnn_layers.29.running_var"]))
    assert torch.equal(m.state_dict()["gru.weight_hh_l1_reverse"], torch.from_numpy(w["gru.weight_hh_l1_reverse"]))


def test_an_attached_lip_reader_brings_its_keys_first_and_stays_frozen_in_eval():
    lip = ssa.Lipreading(relu_type="swish", extract_feats=True)
    with pytest.raises(ValueError, match="embed_size=512"):
        ssa.VoiceFilter(33, lipreader=lip)
    m = ssa.VoiceFilter(33, embed_size=512, lipreader=lip)
    keys = list(m.state_dict())
    n = len(lip.state_dict())
    assert keys[:n] == ["lipreader." + k for k in lip.state_dict()]
    assert keys[n:] == [k for k, _, _ in ssa.voicefilter_state_dict_spec(33, 512)]
    assert m.train() is m and m.training and not m.lipreader.training
    assert not any(p.requires_grad for p in m.lipreader.parameters())
    assert m.eval() is m and not m.training


def test_exports_resolve():
    for name in ("VoiceFilter", "VoiceFilterEngine", "voicefilter_state_dict_spec", "voicefilter_magnitude"):
        assert name in ssa.__all__ and getattr(ssa, name) is not None


@pytest.mark.parametrize("kw", [dict(input_size=0), dict(input_size=300), dict(input_size=201, embed_size=100)])
def test_unsupported_sizes_raise_at_construction(kw):
    with pytest.raises(ValueError, match="input_size|embed_size"):
        ssa.VoiceFilter(**kw)


def test_train_returns_the_module_and_forward_refuses_training_mode_and_a_missing_lip_reader():
    m = ssa.VoiceFilter(17)
    assert m.training                                   # a fresh nn.Module
    assert m.train() is m and m.train(False) is m and m.eval() is m
    mix, e1, e2 = (torch.from_numpy(a) for a in R.synthetic_inputs(17, 7, 1, 1))
    m.train()
    with pytest.raises(RuntimeError, match="training"):
        m.forward_embeddings(mix, e1, e2)
    with pytest.raises(RuntimeError, match="training"):
        m(mix, torch.zeros(1, 1, 96, 96), torch.zeros(1, 1, 96, 96))
    m.eval()
    with pytest.raises(RuntimeError, match="forward_embeddings"):
        m(mix, torch.zeros(1, 1, 96, 96), torch.zeros(1, 1, 96, 96))
    with pytest.raises(RuntimeError, match="no CPU"):
        m.forward_embeddings(mix, e1, e2)


def test_fp64_restatement_reproduces_the_references_fp64_outputs():
    """fp64 against fp64, per (item, speaker, frame) column: pins the restatement, and through it every GPU comparison, to
    the reference's own VoiceFilter."""
    z = np.load(GOLDEN)
    assert [int(s) for s in z["seeds"]] == [R.WEIGHT_SEED, R.INPUT_SEED] and int(z["embed"]) == R.GOLDEN_EMBED
    for i, (F, W, Tv, B) in enumerate(R.GOLDEN_SHAPES):
        assert tuple(int(d) for d in z[f"shape{i}"]) == (F, W, Tv, B)
        w = R.synthetic_voicefilter_weights(F, R.GOLDEN_EMBED, R.WEIGHT_SEED)
        assert R.weights_digest(w) == str(z[f"digest{i}"])
        ref = (z[f"s1_{i}"], z[f"s2_{i}"])
        assert ref[0].dtype == np.float64 and ref[0].shape == ref[1].shape == (B, F, W)
        got = R.run(w, *R.synthetic_inputs(F, W, Tv, B, R.GOLDEN_EMBED, R.INPUT_SEED + i), torch.float64)
        assert R.worst_col(got, ref) <= 1e-10


@pytest.mark.parametrize("case", range(len(R.GOLDEN_SHAPES)))
def test_seeded_weights_and_inputs_keep_the_network_alive(case):
    F, W, Tv, B = R.GOLDEN_SHAPES[case]
    w = R.synthetic_voicefilter_weights(F, R.GOLDEN_EMBED, R.WEIGHT_SEED)
    mix, e1, e2 = R.synthetic_inputs(F, W, Tv, B, R.GOLDEN_EMBED, R.INPUT_SEED + case)
    assert mix.min() == 0.0 and mix.max() == 1.0 and (mix == 0).sum() > 1 and (mix == 1).sum() > 1
    assert ((mix > 0) & (mix < 1)).mean() > 0.8
    assert not np.array_equal(e1, e2) and np.abs(e1 - e2).min() > 0
    taps = {}
    s1, s2 = R.run(w, mix, e1, e2, torch.float64, taps)
    for l in range(1, 8):                    # every ReLU passes a substantial share and blocks a substantial share
        assert 0.25 <= taps[f"relu{l}"] <= 0.75, (l, taps[f"relu{l}"])
    for k in ("mask1", "mask2"):             # the sigmoid is nowhere saturated, and it is not a constant
        assert float(taps[k].min()) > 0.05 and float(taps[k].max()) < 0.95
        assert float(taps[k].max() - taps[k].min()) > 0.2
    assert float((taps["mask1"] - taps["mask2"]).abs().max()) > 0.01      # the d-vector reaches the mask
    for o in (s1, s2):                       # no reference column is zero: the per-column rule leaves none out
        assert float(o.norm(dim=1).min()) > 0.1
    # BatchNorm: non-trivial and different per channel
    for _, bi, cout, *_ in R.CNN:
        for leaf in ("weight", "bias", "running_mean", "running_var"):
            assert len(np.unique(w[f"cnn_layers.{bi}.{leaf}"])) == cout
    # all GRU tensors of both layers and both directions are distinct
    gru = [k for k in w if k.startswith("gru.")]
    assert len(gru) == 16
    for i, a in enumerate(gru):
        for b in gru[i + 1:]:
            assert w[a].shape != w[b].shape or not np.array_equal(w[a], w[b]), (a, b)


def test_magnitude_formula_against_a_hand_made_dft():
    """R.magnitude (the reference's get_magnitude on torch.stft, here in fp64) against frames cut, reflected and windowed
    by hand and numpy's rfft, at T = 3200: a silent stretch (|S| = 0 -> spec exactly 0), a loud one (|S| >= 10 -> spec
    exactly 1) and noise in between."""
    T, N, H = 3200, 400, 100
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.standard_normal(T) * 0.05
    x[:900] = 0.0
    x[2000:2600] = 0.9 * np.sin(2 * np.pi * 0.06 * np.arange(600))
    spec, phase, mag = R.magnitude(torch.from_numpy(x), N, H)
    assert tuple(spec.shape) == (201, 33)
    xp = np.pad(x, (N // 2, N // 2), mode="reflect")
    win = 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)
    S = np.stack([np.fft.rfft(xp[m * H:m * H + N] * win) for m in range(33)], axis=1)
    want = np.clip((20.0 * np.log10(np.maximum(np.abs(S), 1e-5)) - 20.0) / 100.0, -1.0, 0.0) + 1.0
    assert np.abs(spec.numpy() - want).max() <= 1e-10
    assert float(spec.min()) == 0.0 and float(spec.max()) == 1.0 and ((want > 0.01) & (want < 0.99)).mean() > 0.3
    big = np.abs(S) > 1e-6
    d = np.angle(np.exp(1j * (phase.numpy() - np.angle(S))))
    assert np.abs(d[big]).max() <= 1e-8


def test_magnitude_arithmetic_of_the_package_on_the_cpu():
    """speech_separation_amd.voicefilter.magnitude_from_stft, the plain-torch part of voicefilter_magnitude behind the device
    STFT, on torch.stft's fp64 real and imaginary parts against the restatement: a wrong constant fails here too."""
    from speech_separation_amd.voicefilter import magnitude_from_stft
    rng = np.random.Generator(np.random.PCG64(5))
    x = rng.standard_normal(3200) * 0.05
    x[:900] = 0.0
    x[2000:2600] += 0.9 * np.sin(2 * np.pi * 0.06 * np.arange(600))
    xt = torch.from_numpy(x)
    S = torch.stft(xt, n_fft=400, hop_length=100, win_length=400, window=torch.hann_window(400, dtype=xt.dtype), center=True,
                   return_complex=True)
    spec, phase = magnitude_from_stft(S.real, S.imag)
    want, wphase, mag = R.magnitude(xt, 400, 100)
    assert tuple(spec.shape) == (201, 33) and float((spec - want).abs().max()) <= 1e-12
    assert float(spec.min()) == 0.0 and float(spec.max()) == 1.0
    assert float((phase - wphase).abs()[mag > 1e-6].max()) <= 1e-12


def test_forward_preprocesses_raw_frames_for_a_caller_supplied_lip_reader():
    """A caller's module (no forward_window) gets x / 255 -> CenterCrop(88, 88) -> (x - 0.421) / 0.165 as (S, 1, Tv, 88, 88),
    both speakers in one call; 97 x 96 frames crop at (4, 4) as the reference's CenterCrop does."""
    seen = {}

    class Lip(torch.nn.Module):
        backend_out = 1024

        def forward(self, x, lengths=None):
            seen["x"], seen["lengths"] = x, lengths
            return torch.zeros(x.shape[0], x.shape[2], 1024)

    m = ssa.VoiceFilter(17, lipreader=Lip()).eval()
    rng = np.random.Generator(np.random.PCG64(9))
    v = torch.from_numpy(rng.integers(0, 256, (4, 3, 97, 96)).astype(np.float32))
    emb = m._embed(v)
    assert emb.shape == (4, 3, 1024) and seen["lengths"] == [3, 3, 3, 3]
    want = ((v.double() / 255.0)[:, :, 4:92, 4:92] - 0.421) / 0.165
    assert tuple(seen["x"].shape) == (4, 1, 3, 88, 88) and seen["x"].is_contiguous()
    assert float((seen["x"][:, 0].double() - want).abs().max()) <= 4e-6      # values up to 3.6, a few fp32 roundings
    assert float(seen["x"].min()) < -2.0 and float(seen["x"].max()) > 3.0
    with pytest.raises(ValueError, match="smaller"):
        m._embed(v[:, :, :87])
