"""VoiceFilter training step, host layer (no GPU needed): the training-mode restatement (tests/voicefilter_train_ref.py)
against the reference's own fp64 gradients (fixture written by tools/gen_golden_voicefilter_train.py), the C ABI of
include/vfilt_train.h (declared == bound == exported, plain C99), TrainableVoiceFilter's state_dict and refusals, and the
numpy restatement of the dropout keep mask."""
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
from tests import voicefilter_train_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vfilt_train.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "voicefilter_train_small.npz")


def test_fp64_restatement_reproduces_the_references_fp64_gradients():
    """fp64 against fp64 with free ReLUs and the fixture's dropout mask: per tensor |g - g_ref| <= 1e-9 ||g_ref|| at the
    sampled indices; the loss and the updated running statistics as well.  The eight conv-bias gradients of the reference's
    fp64 run are below 1e-10 x the norm of the same layer's BN-bias gradient: rounding noise around a mathematical zero,
    which is why the library writes exact zeros there."""
    z = np.load(GOLDEN)
    F, W, Tv, B = (int(v) for v in z["shape"])
    assert (F, W, Tv, B) == T.TRAIN_SHAPE
    w = R.synthetic_voicefilter_weights(F, R.GOLDEN_EMBED, R.WEIGHT_SEED)
    assert R.weights_digest(w) == str(z["digest"])
    keep = T.fixture_mask(2 * B, W)
    assert np.array_equal(keep, z["mask"]) and 0 < keep.sum() < keep.size
    x = R.synthetic_inputs(F, W, Tv, B, R.GOLDEN_EMBED, R.INPUT_SEED)
    run = T.forward(w, *x, torch.float64, keep)
    loss, g = run.loss_grads(*T.targets(F, W, B))
    assert abs(float(loss) - float(z["loss64"])) <= 1e-12 * abs(float(z["loss64"]))
    keys = [str(k) for k in z["keys"]]
    assert keys == T.trainable_keys(F) == list(run.params) and len(keys) == 58
    norm = dict(zip(keys, z["norm64"]))
    o = 0
    for k, n in zip(keys, z["count"]):
        idx, ref = z["index"][o:o + n], z["value64"][o:o + n]
        o += n
        got = g[k].reshape(-1).numpy()[idx]
        if k in T.CONV_BIAS:
            bn = T.BN_BIAS[T.CONV_BIAS.index(k)]
            assert norm[k] < 1e-10 * norm[bn], (k, norm[k], norm[bn])
            assert float(g[k].norm()) < 1e-10 * float(g[bn].norm()), k
            continue
        assert np.abs(got - ref).max() <= 1e-9 * norm[k], (k, float(np.abs(got - ref).max()), norm[k])
    assert norm["gru.weight_hh_l1_reverse"] == 0.0 and float(g["gru.weight_hh_l1_reverse"].abs().max()) == 0.0
    running = run.updated_running(w)
    o = 0
    for k in (str(k) for k in z["running_keys"]):
        n = running[k].numel()
        ref = z["running64"][o:o + n]
        o += n
        assert np.abs(running[k].numpy() - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), k


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(vftrain_\w+)\s*\(", src)) - {"vftrain_ctx"}
    assert declared == set(_lib.VFTRAIN_SYMBOLS), declared ^ set(_lib.VFTRAIN_SYMBOLS)
    m = re.search(r"#define VFTRAIN_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.VFTRAIN_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.vftrain_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(vftrain_\w+)$", out, re.M))
    assert exported == set(_lib.VFTRAIN_SYMBOLS), exported ^ set(_lib.VFTRAIN_SYMBOLS)
    for want in ("train_forward", "train_backward", "tape_offset", "bind_grads", "flat_offset", "flat_numel", "grad_clip",
                 "adamw_step", "clip_scratch_bytes", "workspace_bytes", "flops_per_item"):
        assert f"vftrain_{want}" in declared, want


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_trainable_module_has_voicefilters_keys_loads_either_way_and_refuses_embedding_gradients():
    base, m = ssa.VoiceFilter(17), ssa.TrainableVoiceFilter(17)
    assert isinstance(m, ssa.VoiceFilter) and "TrainableVoiceFilter" in ssa.__all__ and "VoiceFilterTrainEngine" in ssa.__all__
    assert list(m.state_dict()) == list(base.state_dict()) and len(m.state_dict()) == 82
    assert [tuple(v.shape) for v in m.state_dict().values()] == [tuple(v.shape) for v in base.state_dict().values()]
    w = {k: torch.from_numpy(np.asarray(v)) for k, v in R.synthetic_voicefilter_weights(17).items()}
    base.load_state_dict(w, strict=True)
    m.load_state_dict(base.state_dict(), strict=True)
    base.load_state_dict(m.state_dict(), strict=True)
    assert all(torch.equal(a, b) for a, b in zip(m.state_dict().values(), base.state_dict().values()))
    assert str(m).splitlines()[-2:] == str(base).splitlines()[-2:]            # the parameter-count lines
    assert m.train() is m and m.training and m.eval() is m
    assert len(list(m.parameters())) == 58 and all(p._dptnav_owner() is m for p in m.parameters())
    m.train()
    mix, e = torch.zeros(1, 17, 5), torch.zeros(1, 2, 1024)
    with pytest.raises(NotImplementedError, match="s2_embedding"):
        m.forward_embeddings(mix, e, e.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match="only on an AMD GPU"):            # no CPU fallback on either path
        m.forward_embeddings(mix, e, e)
    with pytest.raises(ValueError, match="neither"):
        m(mix)


def test_dropout_keep_mask_restatement():
    """One draw per (sequence, frame): over 2^16 draws the keep rate is within 4 sigma of 0.65; ppm 0 keeps everything; the
    mask is a function of the seed."""
    n = 1 << 16
    keep = T.keep_mask(256, 256, 350000, seed=12345)
    assert keep.shape == (256, 256) and set(np.unique(keep)) == {0.0, 1.0}
    sigma = np.sqrt(0.65 * 0.35 / n)
    assert abs(float(keep.mean()) - 0.65) <= 4 * sigma, (float(keep.mean()), sigma)
    assert T.keep_mask(4, 9, 0, seed=1).min() == 1.0
    assert np.array_equal(keep, T.keep_mask(256, 256, 350000, seed=12345))
    assert not np.array_equal(keep, T.keep_mask(256, 256, 350000, seed=12346))
    rows, cols = keep.mean(1), keep.mean(0)                                   # no sequence or frame stands out
    assert abs(rows - 0.65).max() < 6 * np.sqrt(0.65 * 0.35 / 256) and abs(cols - 0.65).max() < 6 * np.sqrt(0.65 * 0.35 / 256)
