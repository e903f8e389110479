"""DeepAVConvTasNet training step, host side (no GPU): the C ABI surface of include/davctasnet_train.h, the stock-PyTorch
restatement (tests/deepavconvtasnet_train_ref.py) against tests/deepconvtasnet_ref.forward and against the reference's own
gradients (tests/golden/deepavconvtasnet_grad_slopes.npz, tools/gen_golden_deepavctasnet_grad.py), and the surface of
speech_separation_amd.TrainableDeepAVConvTasNet."""
from __future__ import annotations

import os
import re
import subprocess

import numpy as np
import pytest
import torch

from speech_separation_amd import _lib
from speech_separation_amd.spec import DPTN_AUDIO, deepconvtasnet_state_dict_spec, synthetic_inputs
from tests import deepavconvtasnet_train_ref as R
from tests import deepconvtasnet_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "davctasnet_train.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "deepavconvtasnet_grad_slopes.npz")


def test_header_declares_exactly_the_bound_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(davtrain_\w+)\s*\(", src))
    assert declared == set(_lib.DAVTRAIN_SYMBOLS), declared ^ set(_lib.DAVTRAIN_SYMBOLS)
    m = re.search(r"#define DAVTRAIN_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.DAVTRAIN_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.davtrain_abi_version() == 1
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(davtrain_\w+)$", out, re.M))
    assert exported == set(_lib.DAVTRAIN_SYMBOLS), exported ^ set(_lib.DAVTRAIN_SYMBOLS)
    # the audio-only unit next to it keeps its surface
    assert set(re.findall(r"\b(dcttrain_\w+)$", out, re.M)) == set(_lib.DCTTRAIN_SYMBOLS)
    assert _lib.DCTTRAIN_SYMBOLS["dcttrain_create"][1][1:] == [_lib._i] and _lib.DCTTRAIN_ABI_VERSION == 1
    # the tape kinds of dctasnet_train.h under the same values, plus VCAT
    kinds = lambda text, p: {k: int(v) for k, v in re.findall(rf"#define {p}_TAPE_(\w+) (\d+)", text)}
    dct = kinds(open(os.path.join(ROOT, "include", "dctasnet_train.h")).read(), "DCTTRAIN")
    assert kinds(src, "DAVTRAIN") == dict(dct, VCAT=5) and len(dct) == 5


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_restatement_forward_is_the_inference_restatement():
    """forward() without masks is tests/deepconvtasnet_ref.forward with embeddings operator by operator (torch.equal, fp32
    and fp64, 2 x 401, Tv = 7); the taps have the tape's shapes and change nothing; masks taken from the taps' own signs
    reproduce F.prelu."""
    sd32 = {k: torch.from_numpy(v) for k, v in R.synthetic_weights(0).items()}
    B, T, Tv = 2, 401, 7
    Fr = D.frames(T)
    mix = torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=1)["mix"])
    e32 = [torch.from_numpy(e) for e in R.synthetic_embeddings(B, Tv, 1)]
    for dt in (torch.float32, torch.float64):
        sd = {k: v.to(dt) for k, v in sd32.items()}
        e = [t.to(dt) for t in e32]
        taps = {}
        with torch.no_grad():
            want = D.forward(sd, mix.to(dt), *e)
            a, b = R.forward(sd, mix.to(dt), *e), R.forward(sd, mix.to(dt), *e, taps=taps)
            masks = {k: [t > 0 for t in v] if isinstance(v, list) else v > 0 for k, v in taps.items() if k != "vcat"}
            c = R.forward(sd, mix.to(dt), *e, masks=masks)
            audio = D.forward(sd, mix.to(dt))
        for k in ("s1_pred", "s2_pred"):
            assert torch.equal(a[k], want[k]) and torch.equal(b[k], want[k]) and torch.equal(c[k], want[k]), (dt, k)
            assert not torch.equal(want[k], audio[k])          # the video head is not a no-op with these weights
        assert len(taps["v1"]) == len(taps["u"]) == 24 and len(taps["ez"]) == len(taps["dz"]) == 4
        assert all(t.shape == (B, 512, Fr) for t in taps["v1"] + taps["u"] + taps["ez"]) and taps["skip"].shape == (B, 128, Fr)
        assert all(t.shape == (2 * B, 512, Fr) for t in taps["dz"])
        assert taps["vcat"].shape == (B, Tv, 512) and float(taps["vcat"].abs().max()) > 0


def test_restatement_reproduces_reference_gradients_distinct_slopes():
    """loss.backward() through the restatement (fp32 and fp64, CPU) against the reference's own DeepAVConvTasNet with 57
    distinct PReLU slopes and a video LayerNorm far from the identity: the loss, the norms and the sampled entries, each
    within the reference's own fp32 / fp64 gap (x4, plus a floor at fp32 resolution), at most 1 in 200 sampled entries off --
    the rule of tests/test_deepconvtasnet_train_host.py."""
    from tests.sisnr_ref import pit_sisnr_loss
    from tools.gen_golden import weights_digest
    z = np.load(GOLDEN)
    seeds = [int(v) for v in z["seeds"]]
    sd = R.synthetic_weights(seeds[0], "distinct", seeds[3])
    assert weights_digest(sd) == str(z["digest"])
    assert float(np.abs(sd["video_ln.weight"] - 1).max()) > 0.3 and float(np.abs(sd["video_ln.bias"]).max()) > 0.3
    keys = [str(k) for k in z["keys"]]
    assert keys == [k for k, _ in deepconvtasnet_state_dict_spec(True)] and len(keys) == 376
    assert [str(k) for k in z["nograd"]] == ["separator.separator.23.conv.weight", "separator.separator.23.conv.bias", R.UNUSED]
    B, T, Tv = (int(v) for v in z["shape"])
    inp = synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=seeds[1])
    s1, s2 = inp["s1"].astype(np.float32), inp["s2"].astype(np.float32)
    mix = torch.from_numpy(s1 + s2)
    e1, e2 = (torch.from_numpy(e) for e in R.synthetic_embeddings(B, Tv, seeds[4]))
    counts, index = z["count"], z["index"]
    starts = np.concatenate([[0], np.cumsum(counts)])
    for k in R.VIDEO:                                   # the four video tensors have real gradients in the fixture
        assert float(z["norm64"][keys.index(k)]) > 0
    for dt, lkey, vkey in ((torch.float64, "loss64", "value64"), (torch.float32, "loss32", "value32")):
        p = {k: torch.from_numpy(v).to(dt).requires_grad_(True) for k, v in sd.items()}
        out = R.forward(p, mix.to(dt), e1.to(dt), e2.to(dt))
        loss = pit_sisnr_loss(out["s1_pred"], out["s2_pred"], torch.from_numpy(s1).to(dt), torch.from_numpy(s2).to(dt))
        loss.backward()
        assert p[R.UNUSED].grad is None
        i_un = keys.index(R.UNUSED)
        assert float(z["norm64"][i_un]) == 0.0 and not np.any(z["value64"][starts[i_un]:starts[i_un + 1]])
        gap_loss = abs(float(z["loss32"]) - float(z["loss64"]))
        assert abs(float(loss.detach()) - float(z[lkey])) <= 4 * gap_loss + 1e-5 * abs(float(z["loss64"]))
        grad = lambda k: p[k].grad if p[k].grad is not None else torch.zeros_like(p[k])
        v_all = np.concatenate([grad(k).detach().double().reshape(-1).numpy()[index[starts[i]:starts[i + 1]]]
                                for i, k in enumerate(keys)])
        ref, ref64, ref32 = z[vkey].astype(np.float64), z["value64"], z["value32"].astype(np.float64)
        scale = np.repeat(np.maximum(z["norm64"], 1e-30) / np.sqrt(np.maximum(counts, 1)), counts)
        tol = 4 * np.abs(ref32 - ref64) + (1e-3 if dt == torch.float32 else 1e-9) * scale
        bad = np.nonzero(np.abs(v_all - ref) > tol)[0]
        print(f"{dt}: {len(bad)} of {len(ref)} sampled entries off (cap {len(ref) // 200})")
        assert len(bad) <= len(ref) // 200, (dt, len(bad), bad[:10])
        if dt == torch.float64:
            norms = np.array([float(grad(k).norm()) for k in keys])
            np.testing.assert_allclose(norms, z["norm64"], rtol=1e-9, atol=1e-12)
    ones = torch.ones(B, 16 * (T // 16))
    g = R.grads({k: torch.from_numpy(v) for k, v in sd.items()}, mix, e1, e2, ones, ones)
    assert not g[R.UNUSED].any() and all(g[k].any() for k in R.VIDEO)


def test_module_surface():
    import speech_separation_amd as pkg
    from speech_separation_amd import DeepAVConvTasNet, TrainableDeepAVConvTasNet
    assert "TrainableDeepAVConvTasNet" in pkg.__all__ and pkg.TrainableDeepAVConvTasNet is TrainableDeepAVConvTasNet
    assert "DeepAVConvTasNetTrainEngine" in pkg.__all__
    from speech_separation_amd.engine import DeepAVConvTasNetTrainEngine, DeepConvTasNetTrainEngine
    assert issubclass(DeepAVConvTasNetTrainEngine, DeepConvTasNetTrainEngine) and DeepAVConvTasNetTrainEngine.TAPE_VCAT == 5
    m = TrainableDeepAVConvTasNet(N=512, L=16, video_emb_size=512, hidden_video=512)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == deepconvtasnet_state_dict_spec(True)
    assert len(m.state_dict()) == 376
    assert str(m).splitlines()[-2:] == str(DeepAVConvTasNet()).splitlines()[-2:]
    with pytest.raises(NotImplementedError):
        TrainableDeepAVConvTasNet(hidden_video=256)
    sd = {k: torch.from_numpy(v) for k, v in R.synthetic_weights(0).items()}
    m.load_state_dict(sd, strict=True)
    c = DeepAVConvTasNet()
    c.load_state_dict(m.state_dict(), strict=True)
    m2 = TrainableDeepAVConvTasNet()
    m2.load_state_dict(c.state_dict(), strict=True)
    for k, v in m2.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert all(p._dptnav_owner() is m for p in m.parameters())
    # initialisation as DeepAVConvTasNet's: the same draws from the same generator state
    torch.manual_seed(3)
    a = TrainableDeepAVConvTasNet().state_dict()
    torch.manual_seed(3)
    b = DeepAVConvTasNet().state_dict()
    assert all(torch.equal(a[k], b[k]) for k in b)
    mix, e = torch.zeros(1, 4000), torch.zeros(1, 512, 5)
    with pytest.raises(RuntimeError, match="no CPU"):
        m(mix=mix, s1_embedding=e, s2_embedding=e)
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU"):
        m(mix=mix, s1_embedding=e, s2_embedding=e)
