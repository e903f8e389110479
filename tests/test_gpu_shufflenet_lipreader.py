"""The ShuffleNet-v2 lip reader (include/lipsn.h) on the MI355X: parity with the reference's own fp64 outputs
(tests/golden/lipreader_shufflenet.npz) and with the fp64 restatement (tests/shufflenet_ref.py) for the three stem
activations and both widths at sizes with odd maps at every level, final maps of 3 x 3, 4 x 3 and 5 x 5 (AvgPool2d(3) reads
rows / columns 0..2 only) and T in {1, 2, 3}; the windowed forward with the affine fused; the refused sizes; determinism,
batch independence, a device-only forward, fresh weights in the same storages; VoiceFilter from raw video, VideoSSModel and
make_embeddings on top of it.

The rule of every value comparison: per (stream, frame) row r, rel(r) = ||got_r - ref64_r|| / ||ref64_r||; the HIP result's
worst row must be <= 2 x the worst row of the stock-PyTorch fp32 CPU run of the restatement on the same case (2: the MFMA's
K-chunk summation order differs from the CPU library's; a second fp32 order of the CPU library lands at 0.92-1.13 x).  Both
figures are printed before the assertion."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from tests import shufflenet_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "lipreader_shufflenet.npz")
ACTS = ("prelu", "swish", "relu")
WIDTHS = (1.0, 0.5)
# 88 x 88: the shipped crop.  65 x 72: maps 33 x 36 -> 17 x 18 -> 9 x 9 -> 5 x 5 -> 3 x 3.  97 x 66: final map 4 x 3.
# 160 x 129: final map 5 x 5, the upper size limit (stage 2 runs in bands of rows there), T = 1.
SHAPES = [(2, 3, 88, 88), (1, 2, 65, 72), (2, 2, 97, 66), (1, 1, 160, 129)]
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


def _weights(relu_type, width_mult, seed=R.WEIGHT_SEED):
    key = ("w", relu_type == "prelu", width_mult, seed)
    if key not in _cache:     # relu shares swish's tensors: the same keys
        _cache[key] = R.synthetic_shufflenet_weights("prelu" if relu_type == "prelu" else "swish", width_mult, seed)
    return _cache[key]


def _load(m, w):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)


def _model(relu_type, width_mult, dev):
    key = ("m", relu_type, width_mult)
    if key not in _cache:
        from speech_separation_amd import ShuffleNetLipreading
        m = ShuffleNetLipreading(relu_type=relu_type, width_mult=width_mult, extract_feats=True)
        _load(m, _weights(relu_type, width_mult))
        _cache[key] = m.to(dev).eval()
    return _cache[key]


def _refs(relu_type, width_mult, x, seed=R.WEIGHT_SEED, **kw):
    """(fp64 restatement, worst row of the fp32 CPU run against it)"""
    w = _weights(relu_type, width_mult, seed)
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


@pytest.mark.parametrize("case", range(len(R.GOLDEN_CASES)))
def test_against_the_references_fp64_outputs(dev, case):
    relu_type, width_mult, shape = R.GOLDEN_CASES[case]
    z = np.load(GOLDEN)
    tag = "w10" if width_mult == 1.0 else "w05"
    assert R.weights_digest(_weights(relu_type, width_mult)) == str(z[f"digest_{tag}"])
    x = R.synthetic_video(shape, R.INPUT_SEED + case)
    ref64 = torch.from_numpy(z[f"out{case}"])
    cpu32 = R.run(_weights(relu_type, width_mult), x, torch.float32, relu_type=relu_type)
    got = _model(relu_type, width_mult, dev)(torch.from_numpy(x).to(dev), lengths=[shape[2]] * shape[0])
    assert not got.requires_grad
    _judge(got, ref64, float(R.row_rel(cpu32, ref64).max()), f"golden {relu_type} x{width_mult} {shape}")


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("width_mult", WIDTHS)
@pytest.mark.parametrize("relu_type", ACTS)
def test_against_the_fp64_restatement(dev, relu_type, width_mult, shape):
    S, T, H, W = shape
    x = R.synthetic_video((S, 1, T, H, W), seed=100 + H)
    ref64, cpu_worst = _refs(relu_type, width_mult, x)
    got = _model(relu_type, width_mult, dev)(torch.from_numpy(x).to(dev), lengths=[T] * S)
    _judge(got, ref64, cpu_worst, f"{relu_type} x{width_mult} {shape}")


def test_profiler_size(dev):
    x = R.synthetic_video((2, 1, 50, 88, 88), seed=7)
    ref64, cpu_worst = _refs("prelu", 1.0, x)
    got = _model("prelu", 1.0, dev)(torch.from_numpy(x).to(dev), lengths=[50, 50])
    _judge(got, ref64, cpu_worst, "prelu x1.0 (2, 50, 88, 88)")


@pytest.mark.parametrize("hw", [(64, 88), (88, 64), (161, 88), (88, 161)])
def test_unsupported_sizes_are_refused(dev, hw):
    with pytest.raises(RuntimeError, match=r"\[65, 160\]"):
        _model("prelu", 1.0, dev)(torch.zeros(1, 1, 2, *hw, device=dev), lengths=[2])


def test_windowed_forward(dev):
    clip = R.synthetic_clip(R.PREPROC_SHAPE, R.INPUT_SEED)          # (3, 97, 96), uint8-valued
    window, affine = R.preproc_window_affine()
    assert window == (4, 4, 88, 88)
    m = _model("prelu", 1.0, dev)
    got = m.forward_window(torch.from_numpy(clip)[None].to(dev), window, affine)
    ref64, cpu_worst = _refs("prelu", 1.0, clip[None, None], window=window, affine=affine)
    _judge(got, ref64, cpu_worst, "windowed vs restatement")
    # against the plain forward on the pre-cropped, pre-normalised tensor (the kernel fuses the affine: value rule)
    y0, x0, H, W = window
    pre = (torch.from_numpy(clip)[:, y0:y0 + H, x0:x0 + W] * np.float32(affine[0]) + np.float32(affine[1])).contiguous()
    plain = m(pre[None, None].to(dev), lengths=[clip.shape[0]])
    _judge(plain, ref64, cpu_worst, "plain on pre-normalised vs restatement")
    _judge(got, plain.detach().cpu().double(), cpu_worst, "windowed vs plain")


@pytest.mark.parametrize("width_mult", WIDTHS)
def test_two_calls_are_bit_identical_and_streams_do_not_mix(dev, width_mult):
    """Stage 4 and conv_last put several frames into one MFMA tile at 88 x 88 (frames 3k .. 3k + 2 at width 1.0): with
    T = 2 those are frames of two streams, and a stream's rows must not notice."""
    m = _model("prelu", width_mult, dev)
    x = torch.from_numpy(R.synthetic_video((5, 1, 2, 88, 88), seed=11)).to(dev)
    a = m(x, lengths=[2] * 5).clone()
    b = m(x, lengths=[2] * 5)
    assert torch.equal(a, b)
    for i in (0, 2, 4):
        alone = m(x[i:i + 1].contiguous(), lengths=[2])
        assert torch.equal(alone[0], a[i]), i


def test_device_only_forward(dev):
    m = _model("swish", 1.0, dev)
    x = torch.from_numpy(R.synthetic_video((2, 1, 3, 65, 72), seed=12)).to(dev)
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
    from speech_separation_amd import ShuffleNetLipreading
    m = ShuffleNetLipreading(relu_type="prelu", extract_feats=True)
    _load(m, _weights("prelu", 1.0))
    m = m.to(dev)
    x = R.synthetic_video((1, 1, 2, 65, 72), seed=13)
    xd = torch.from_numpy(x).to(dev)
    first = m(xd, lengths=[2]).clone()
    ptrs = [t.data_ptr() for t in m.state_dict().values()]
    _load(m, _weights("prelu", 1.0, seed=1))
    assert ptrs == [t.data_ptr() for t in m.state_dict().values()]
    assert m._engine.bound_to(m._float_tensors())
    got = m(xd, lengths=[2])
    assert not torch.equal(got, first)
    ref64, cpu_worst = _refs("prelu", 1.0, x, seed=1)
    _judge(got, ref64, cpu_worst, "seed-1 weights in the same storages")


def test_voicefilter_from_raw_video(dev):
    """VoiceFilter with its default embed_size = 1024 and the ShuffleNet lip reader, at a small size: forward from raw
    [0, 255] frames equals forward_embeddings on the lip reader's own output of the reference's test-time window."""
    from speech_separation_amd import VoiceFilter
    torch.manual_seed(0)
    lip = _model("prelu", 1.0, dev)
    vf = VoiceFilter(21, lipreader=lip).to(dev).eval()
    assert vf.embed_size == 1024 and list(vf.state_dict())[0].startswith("lipreader.")
    B, F, W, Tv = 2, 21, 9, 3
    rng = np.random.Generator(np.random.PCG64(6))
    mag = torch.from_numpy(np.abs(rng.standard_normal((B, F, W))).astype(np.float32)).to(dev)
    v1 = torch.from_numpy(R.synthetic_clip((B, Tv, 96, 96), seed=40)).to(dev)
    v2 = torch.from_numpy(R.synthetic_clip((B, Tv, 96, 96), seed=41)).to(dev)
    window, affine = R.preproc_window_affine((0, 96, 96))
    with torch.no_grad():
        out = vf(mix_magnitude=mag, s1_video=v1, s2_video=v2)
        e1, e2 = lip.forward_window(v1, window, affine).clone(), lip.forward_window(v2, window, affine).clone()
        want = vf.forward_embeddings(mag, e1, e2)
    assert e1.shape == (B, Tv, 1024)
    for k in ("s1_spec_pred", "s2_spec_pred"):
        assert out[k].shape == (B, F, W) and bool(torch.isfinite(out[k]).all())
        assert torch.equal(out[k], want[k]), k


def test_video_ss_model(dev):
    from speech_separation_amd import DPTNAVWavEncDec, VideoSSModel
    torch.manual_seed(0)
    ss = DPTNAVWavEncDec(num_features=128, video_emb_size=1024, hidden_video=128, kernel_size_enc=7, hidden_dim=128,
                         num_blocks=2, chunk_size=150, step_size=75).to(dev).eval()
    lip = _model("prelu", 0.5, dev)
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
    assert out["s1_embedding"].shape == (B, 1024, Tv)
    assert torch.equal(out["s1_embedding"], e1) and torch.equal(out["s2_embedding"], e2)
    for k in ("s1_pred", "s2_pred"):
        assert out[k].shape[0] == B and bool(torch.isfinite(out[k]).all())
        assert torch.equal(out[k], want[k]), k


def test_make_embeddings(dev, tmp_path):
    from speech_separation_amd import make_embeddings
    from speech_separation_amd.io import load_object
    mouths, embeds = tmp_path / "mouths", tmp_path / "embeddings"
    mouths.mkdir()
    clips = {}
    for i, T in enumerate((3, 5, 3)):
        clips[f"clip{i}.npz"] = R.synthetic_clip((T, 96, 96), seed=20 + i)
        np.savez_compressed(mouths / f"clip{i}.npz", data=clips[f"clip{i}.npz"].astype(np.uint8))
    m = _model("prelu", 1.0, dev)
    written = make_embeddings(m, str(mouths), str(embeds))
    assert sorted(os.path.basename(p) for p in written) == sorted(clips)
    window, affine = R.preproc_window_affine((0, 96, 96))
    for name, clip in clips.items():
        with np.load(embeds / name) as z:
            assert list(z.files) == ["embedding"]
            e = z["embedding"]
        T = clip.shape[0]
        assert e.shape == (1024, T) and e.dtype == np.float32
        direct = m.forward_window(torch.from_numpy(clip)[None].to(dev), window, affine)[0].T.cpu().numpy()
        assert np.array_equal(e, direct), name
        assert tuple(load_object(str(embeds / name)).shape) == (1, 1024, T)
