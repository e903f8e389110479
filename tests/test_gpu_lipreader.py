"""The lip-reading front end (include/lipfe.h) on the MI355X: parity with the reference's own fp64 outputs
(tests/golden/lipreader_*.npz) and with the fp64 restatement (tests/lipreader_ref.py) for the three activations at square,
non-square and odd sizes and at T in {1, 2}; the windowed forward with the affine fused; determinism, batch independence, a
device-only forward, fresh weights in the same storages, VideoSSModel and make_embeddings.

The rule of every value comparison: per (stream, frame) row r, rel(r) = ||got_r - ref64_r|| / ||ref64_r||; the HIP result's
worst row must be <= 2 x the worst row of the stock-PyTorch fp32 CPU run of the restatement on the same case (2: the MFMA's
K-chunk summation order differs from the CPU library's).  Both figures are printed before the assertion."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests import lipreader_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
ACTS = ("swish", "prelu", "relu")
SHAPES = [(2, 5, 88, 88), (2, 7, 40, 56), (1, 2, 33, 47), (3, 1, 17, 16)]
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


def _weights(relu_type, seed=R.WEIGHT_SEED):
    key = ("w", relu_type, seed)
    if key not in _cache:     # relu shares swish's tensors: the same keys
        _cache[key] = R.synthetic_lipreader_weights("prelu" if relu_type == "prelu" else "swish", seed)
    return _cache[key]


def _load(m, w):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)


def _model(relu_type, dev):
    key = ("m", relu_type)
    if key not in _cache:
        from speech_separation_amd import Lipreading
        m = Lipreading(relu_type=relu_type, extract_feats=True)
        _load(m, _weights(relu_type))
        _cache[key] = m.to(dev).eval()
    return _cache[key]


def _refs(relu_type, x, seed=R.WEIGHT_SEED, **kw):
    """(fp64 restatement, worst row of the fp32 CPU run against it)"""
    w = _weights(relu_type, seed)
    ref64 = R.run(w, x, torch.float64, relu_type=relu_type, **kw)
    cpu32 = R.run(w, x, torch.float32, relu_type=relu_type, **kw)
    return ref64, float(R.row_rel(cpu32, ref64).max())


def _judge(got, ref64, cpu_worst, what):
    got = got.detach().cpu() if torch.is_tensor(got) else torch.as_tensor(got)
    assert tuple(got.shape) == tuple(ref64.shape), what
    assert bool(torch.isfinite(got).all()), what
    rel = float(R.row_rel(got, ref64).max())
    print(f"{what}: HIP worst row {rel:.3e}, fp32 CPU worst row {cpu_worst:.3e}, ratio {rel / cpu_worst:.2f}")
    assert rel <= 2.0 * cpu_worst, (what, rel, cpu_worst)


@pytest.mark.parametrize("relu_type", ["swish", "prelu"])
def test_against_the_references_fp64_outputs(dev, relu_type):
    z = np.load(os.path.join(GOLDEN, f"lipreader_{relu_type}.npz"))
    assert R.weights_digest(_weights(relu_type)) == str(z["digest"])
    m = _model(relu_type, dev)
    for i, shape in enumerate(R.GOLDEN_SHAPES):
        x = R.synthetic_video(shape, R.INPUT_SEED + i)
        ref64 = torch.from_numpy(z[f"out{i}"])
        cpu32 = R.run(_weights(relu_type), x, torch.float32, relu_type=relu_type)
        got = m(torch.from_numpy(x).to(dev), lengths=[shape[2]] * shape[0])
        assert not got.requires_grad
        _judge(got, ref64, float(R.row_rel(cpu32, ref64).max()), f"golden {relu_type} {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("relu_type", ACTS)
def test_against_the_fp64_restatement(dev, relu_type, shape):
    S, T, H, W = shape
    x = R.synthetic_video((S, 1, T, H, W), seed=100 + H)
    ref64, cpu_worst = _refs(relu_type, x)
    got = _model(relu_type, dev)(torch.from_numpy(x).to(dev), lengths=[T] * S)
    _judge(got, ref64, cpu_worst, f"{relu_type} {shape}")


def test_profiler_size(dev):
    x = R.synthetic_video((2, 1, 50, 88, 88), seed=7)
    ref64, cpu_worst = _refs("swish", x)
    got = _model("swish", dev)(torch.from_numpy(x).to(dev), lengths=[50, 50])
    _judge(got, ref64, cpu_worst, "swish (2, 50, 88, 88)")


@pytest.mark.parametrize("hw", [(7, 88), (88, 7), (257, 88), (88, 257)])
def test_unsupported_sizes_are_refused(dev, hw):
    with pytest.raises(RuntimeError, match=r"\[8, 256\]"):
        _model("swish", dev)(torch.zeros(1, 1, 2, *hw, device=dev), lengths=[2])


def test_windowed_forward(dev):
    z = np.load(os.path.join(GOLDEN, "lipreader_preproc.npz"))
    clip = R.synthetic_clip(R.PREPROC_SHAPE, R.INPUT_SEED)
    window, affine = R.preproc_window_affine()
    m = _model("swish", dev)
    got = m.forward_window(torch.from_numpy(clip)[None].to(dev), window, affine)
    # against the reference's own pipeline (CenterCrop / Normalize classes, then the model, fp64)
    ref64 = torch.from_numpy(z["out"])
    cpu32 = R.run(_weights("swish"), clip[None, None], torch.float32, window=window, affine=affine)
    cpu_worst = float(R.row_rel(cpu32, ref64).max())
    _judge(got, ref64, cpu_worst, "windowed vs fixture")
    # against the plain forward on the pre-cropped, pre-normalised tensor (the kernel fuses the affine: value rule)
    y0, x0, H, W = window
    pre = (torch.from_numpy(clip)[:, y0:y0 + H, x0:x0 + W] * np.float32(affine[0]) + np.float32(affine[1])).contiguous()
    plain = m(pre[None, None].to(dev), lengths=[clip.shape[0]])
    _judge(plain, ref64, cpu_worst, "plain on pre-normalised vs fixture")
    _judge(got, plain.detach().cpu().double(), cpu_worst, "windowed vs plain")


def test_two_calls_are_bit_identical_and_streams_do_not_mix(dev):
    m = _model("prelu", dev)
    x = torch.from_numpy(R.synthetic_video((5, 1, 3, 40, 56), seed=11)).to(dev)
    a = m(x, lengths=[3] * 5).clone()
    b = m(x, lengths=[3] * 5)
    assert torch.equal(a, b)
    for i in (0, 2, 4):
        alone = m(x[i:i + 1].contiguous(), lengths=[3])
        assert torch.equal(alone[0], a[i]), i


def test_device_only_forward(dev):
    m = _model("swish", dev)
    x = torch.from_numpy(R.synthetic_video((2, 1, 3, 33, 47), seed=12)).to(dev)
    want = m(x, lengths=[3, 3]).clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = m(x, lengths=[3, 3])
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert torch.equal(got, want)


def test_new_weights_in_the_same_storages(dev):
    from speech_separation_amd import Lipreading
    m = Lipreading(relu_type="prelu", extract_feats=True)
    _load(m, _weights("prelu"))
    m = m.to(dev)
    x = R.synthetic_video((1, 1, 2, 33, 47), seed=13)
    xd = torch.from_numpy(x).to(dev)
    first = m(xd, lengths=[2]).clone()
    ptrs = [t.data_ptr() for t in m.state_dict().values()]
    _load(m, _weights("prelu", seed=1))
    assert ptrs == [t.data_ptr() for t in m.state_dict().values()]
    assert m._engine.bound_to(m._float_tensors())
    got = m(xd, lengths=[2])
    assert not torch.equal(got, first)
    ref64, cpu_worst = _refs("prelu", x, seed=1)
    _judge(got, ref64, cpu_worst, "seed-1 weights in the same storages")


def test_video_ss_model(dev):
    from speech_separation_amd import DPTNAVWavEncDec, VideoSSModel
    torch.manual_seed(0)
    ss = DPTNAVWavEncDec(num_features=128, video_emb_size=512, hidden_video=128, kernel_size_enc=7, hidden_dim=128,
                         num_blocks=2, chunk_size=150, step_size=75).to(dev).eval()
    lip = _model("swish", dev)
    model = VideoSSModel(ss, lip)
    B, T, Tv = 2, 8000, 5
    rng = np.random.Generator(np.random.PCG64(5))
    mix = torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32) * 0.1).to(dev)
    video = torch.from_numpy(R.synthetic_video((2 * B, 1, Tv, 88, 88), seed=14)).to(dev)
    with torch.no_grad():
        out = model(mix=mix, video=video)
        emb = lip(video, lengths=[Tv] * (2 * B)).permute(0, 2, 1)
        e1, e2 = emb[:B].contiguous(), emb[B:].contiguous()
        want = ss(mix=mix, s1_embedding=e1, s2_embedding=e2)
        split = model(mix=mix, s1_video=video[:B, 0].contiguous(), s2_video=video[B:, 0].contiguous())
    assert out["s1_embedding"].shape == (B, 512, Tv)
    assert torch.equal(out["s1_embedding"], e1) and torch.equal(out["s2_embedding"], e2)
    for k in ("s1_pred", "s2_pred"):
        assert out[k].shape[0] == B and bool(torch.isfinite(out[k]).all())
        assert torch.equal(out[k], want[k]), k
        assert torch.equal(split[k], out[k]), k
    assert torch.equal(split["s1_embedding"], e1) and torch.equal(split["s2_embedding"], e2)
    with pytest.raises(KeyError):
        model(mix=mix)


def test_make_embeddings(dev, tmp_path):
    from speech_separation_amd import make_embeddings
    from speech_separation_amd.io import load_object
    mouths, embeds = tmp_path / "mouths", tmp_path / "embeddings"
    mouths.mkdir()
    clips = {}
    for i, T in enumerate((3, 5, 3)):
        clips[f"clip{i}.npz"] = R.synthetic_clip((T, 96, 96), seed=20 + i)
        np.savez_compressed(mouths / f"clip{i}.npz", data=clips[f"clip{i}.npz"].astype(np.uint8))
    m = _model("swish", dev)
    written = make_embeddings(m, str(mouths), str(embeds))
    assert sorted(os.path.basename(p) for p in written) == sorted(clips)
    window, affine = R.preproc_window_affine((0, 96, 96))
    for name, clip in clips.items():
        with np.load(embeds / name) as z:
            assert list(z.files) == ["embedding"]
            e = z["embedding"]
        T = clip.shape[0]
        assert e.shape == (512, T) and e.dtype == np.float32
        direct = m.forward_window(torch.from_numpy(clip)[None].to(dev), window, affine)[0].T.cpu().numpy()
        assert np.array_equal(e, direct), name
        assert tuple(load_object(str(embeds / name)).shape) == (1, 512, T)
