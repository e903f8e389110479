"""VoiceFilter (include/vfilt.h) on the MI355X: parity with the reference's own fp64 outputs
(tests/golden/voicefilter_small.npz) at the four golden shapes, with the fp64 restatement (tests/voicefilter_ref.py) at
embed_size 512 and at the full size (201, 321, 50, 1); speaker symmetry, determinism, batch independence, fresh weights in
the same storages, caller-provided results and workspace, refusals, the lip reader in front, and voicefilter_magnitude.

The rule of every value comparison: per (item, speaker, frame) column c of F values, rel(c) = ||got_c - ref64_c|| /
||ref64_c||; the HIP result's worst column must be <= 2 x the worst column of the stock-PyTorch fp32 CPU run of the
restatement on the same case (2: the project's standing margin for a different summation order).  No column is left out
(the host test asserts that no reference column is near zero).  Both figures are printed before the assertion."""
from __future__ import annotations

import math
import os

import numpy as np
import pytest
import torch

from tests import spec_ref as SR
from tests import voicefilter_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "voicefilter_small.npz")
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


def _weights(F, E=1024, seed=R.WEIGHT_SEED):
    key = ("w", F, E, seed)
    if key not in _cache:
        _cache[key] = R.synthetic_voicefilter_weights(F, E, seed)
    return _cache[key]


def _load(m, w):
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)


def _model(F, dev, E=1024):
    key = ("m", F, E)
    if key not in _cache:
        from speech_separation_amd import VoiceFilter
        m = VoiceFilter(F, embed_size=E)
        _load(m, _weights(F, E))
        _cache[key] = m.to(dev).eval()
    return _cache[key]


def _on(dev, *arrays):
    return tuple(torch.from_numpy(a).to(dev) for a in arrays)


def _run(m, dev, mix, e1, e2, **kw):
    out = m.forward_embeddings(*_on(dev, mix, e1, e2), **kw)
    assert sorted(out) == ["s1_spec_pred", "s2_spec_pred"] and not out["s1_spec_pred"].requires_grad
    return out["s1_spec_pred"], out["s2_spec_pred"]


def _judge(got, ref64, cpu32, what):
    got = tuple(g.detach().cpu() for g in got)
    for g, r in zip(got, ref64):
        assert tuple(g.shape) == tuple(r.shape), what
        assert bool(torch.isfinite(g).all()), what
        assert float(torch.as_tensor(r).double().norm(dim=1).min()) > 0.1, what       # no column is zero
    rel, cpu_worst = R.worst_col(got, ref64), R.worst_col(cpu32, ref64)
    print(f"{what}: HIP worst column {rel:.3e}, fp32 CPU worst column {cpu_worst:.3e}, ratio {rel / cpu_worst:.2f}")
    assert rel <= 2.0 * cpu_worst, (what, rel, cpu_worst)


@pytest.mark.parametrize("case", range(len(R.GOLDEN_SHAPES)), ids=lambda i: "x".join(map(str, R.GOLDEN_SHAPES[i])))
def test_against_the_references_fp64_outputs(dev, case):
    F, W, Tv, B = R.GOLDEN_SHAPES[case]
    z = np.load(GOLDEN)
    w = _weights(F)
    assert R.weights_digest(w) == str(z[f"digest{case}"])
    x = R.synthetic_inputs(F, W, Tv, B, R.GOLDEN_EMBED, R.INPUT_SEED + case)
    ref64 = (torch.from_numpy(z[f"s1_{case}"]), torch.from_numpy(z[f"s2_{case}"]))
    _judge(_run(_model(F, dev), dev, *x), ref64, R.run(w, *x, torch.float32), f"golden {(F, W, Tv, B)}")


def test_embed_512_against_the_fp64_restatement(dev):
    F, W, Tv, B = 33, 50, 3, 1
    w = _weights(F, 512)
    x = R.synthetic_inputs(F, W, Tv, B, 512, seed=77)
    _judge(_run(_model(F, dev, 512), dev, *x), R.run(w, *x, torch.float64), R.run(w, *x, torch.float32), "E = 512 (33, 50, 3, 1)")


def test_full_size(dev):
    F, W, Tv, B = 201, 321, 50, 1
    w = _weights(F)
    x = R.synthetic_inputs(F, W, Tv, B, 1024, seed=78)
    _judge(_run(_model(F, dev), dev, *x), R.run(w, *x, torch.float64), R.run(w, *x, torch.float32), "full size (201, 321, 50, 1)")


def test_swapped_embeddings_swap_the_outputs_and_two_calls_are_bit_identical(dev):
    F, W, Tv, B = 40, 33, 4, 2
    m = _model(F, dev)
    mix, e1, e2 = R.synthetic_inputs(F, W, Tv, B, 1024, seed=79)
    a1, a2 = (t.clone() for t in _run(m, dev, mix, e1, e2))
    b1, b2 = (t.clone() for t in _run(m, dev, mix, e1, e2))
    assert torch.equal(a1, b1) and torch.equal(a2, b2)
    c1, c2 = _run(m, dev, mix, e2, e1)
    assert torch.equal(c1, a2) and torch.equal(c2, a1)
    assert not torch.equal(a1, a2)


def test_an_item_does_not_depend_on_its_batch(dev):
    F, W, Tv, B = 17, 7, 1, 3
    m = _model(F, dev)
    mix, e1, e2 = R.synthetic_inputs(F, W, Tv, B, 1024, seed=80)
    a1, a2 = (t.clone() for t in _run(m, dev, mix, e1, e2))
    for i in (0, 2):
        s1, s2 = _run(m, dev, mix[i:i + 1], e1[i:i + 1], e2[i:i + 1])
        assert torch.equal(s1[0], a1[i]) and torch.equal(s2[0], a2[i]), i
    # more than one group of eight sequences in the LSTM step: items 0 and 4 of five
    F, W, Tv, B = 33, 9, 2, 5
    m = _model(F, dev)
    mix, e1, e2 = R.synthetic_inputs(F, W, Tv, B, 1024, seed=81)
    a1, a2 = (t.clone() for t in _run(m, dev, mix, e1, e2))
    for i in (0, 4):
        s1, s2 = _run(m, dev, mix[i:i + 1], e1[i:i + 1], e2[i:i + 1])
        assert torch.equal(s1[0], a1[i]) and torch.equal(s2[0], a2[i]), i


def test_new_weights_in_the_same_storages(dev):
    from speech_separation_amd import VoiceFilter
    F, W, Tv, B = 33, 50, 3, 1
    m = VoiceFilter(F)
    _load(m, _weights(F))
    m = m.to(dev).eval()
    x = R.synthetic_inputs(F, W, Tv, B, 1024, seed=82)
    first = tuple(t.clone() for t in _run(m, dev, *x))
    ptrs = [t.data_ptr() for t in m.state_dict().values()]
    w1 = _weights(F, seed=1)
    _load(m, w1)
    assert ptrs == [t.data_ptr() for t in m.state_dict().values()]
    assert m._engine.bound_to(m._float_tensors())
    got = _run(m, dev, *x)
    assert not torch.equal(got[0], first[0])
    _judge(got, R.run(w1, *x, torch.float64), R.run(w1, *x, torch.float32), "seed-1 weights in the same storages")


def test_caller_provided_out_and_workspace(dev):
    F, W, Tv, B = 40, 33, 4, 2
    m = _model(F, dev)
    x = R.synthetic_inputs(F, W, Tv, B, 1024, seed=83)
    want = tuple(t.clone() for t in _run(m, dev, *x))
    need = m._engine.workspace_bytes(B, W, Tv)
    assert need % 256 == 0
    ws = torch.full((need,), 0xFF, dtype=torch.uint8, device=dev)
    out = (torch.full((B, F, W), float("nan"), device=dev), torch.full((B, F, W), float("nan"), device=dev))
    got = _run(m, dev, *x, out=out, ws=ws)
    assert got[0].data_ptr() == out[0].data_ptr() and got[1].data_ptr() == out[1].data_ptr()
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
    with pytest.raises((ValueError, RuntimeError)):
        _run(m, dev, *x, ws=ws[:need - 256])
    assert m._engine.flops_per_item(W, Tv) > 2.0 * F * W * 5 * 64 * 64 * 25
    assert m._engine.min_bytes_per_item(W, Tv) > 4.0 * 14 * F * W * 64


@pytest.mark.parametrize("F,E,named", [(0, 1024, "input_size"), (300, 1024, "input_size"), (201, 100, "embed_size")])
def test_unsupported_sizes_are_refused_without_a_launch(dev, F, E, named):
    import ctypes
    from speech_separation_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.vfilt_create(ctypes.byref(h), F, E) == 1 and not h.value
    assert named in lib.vfilt_last_error(None).decode()


def test_unsupported_shapes_are_refused_with_a_message(dev):
    eng = _model(17, dev)._get_engine(dev)
    for B, W, Tv in ((0, 7, 1), (1, 0, 1), (1, 7, 0), (1 << 20, 1 << 20, 1)):
        with pytest.raises(RuntimeError, match="must"):
            eng.workspace_bytes(B, W, Tv)
    mix, e1, e2 = _on(dev, *R.synthetic_inputs(17, 7, 1, 1))
    with pytest.raises(ValueError):
        eng.forward(mix[:, :16], e1, e2)
    with pytest.raises(ValueError):
        eng.forward(mix, e1[:, :, :512], e2[:, :, :512])


def test_forward_with_videos_through_the_lip_reader(dev):
    """forward on RAW (1, 3, 96, 96) clips in [0, 255] applies the reference's test-time pipeline (x / 255, centre crop to
    88 x 88, (x - 0.421) / 0.165) before the lip reader.  Judged by the rule of this file against the whole chain in fp64 on
    the CPU: the lip reader's restatement on the explicitly cropped and normalised clip (tests/lipreader_ref.py), then the
    separator's; the yardstick is the same chain in fp32.  And bit for bit against forward_embeddings on the lip reader's
    own windowed output, and far from what the unprocessed frames would give."""
    from speech_separation_amd import Lipreading, VoiceFilter
    from tests import lipreader_ref as LR
    lw = LR.synthetic_lipreader_weights("swish", 0)
    lip = Lipreading(relu_type="swish", extract_feats=True)
    lip.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in lw.items()}, strict=True)
    F, W, Tv, B = 33, 50, 3, 1
    w = _weights(F, 512)
    m = VoiceFilter(F, embed_size=512, lipreader=lip)
    res = m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=False)
    assert not res.unexpected_keys and all(k.startswith("lipreader.") for k in res.missing_keys)
    m = m.to(dev).eval()
    mix = R.synthetic_inputs(F, W, Tv, B, 512, seed=84)[0]
    clips = [LR.synthetic_clip((Tv, 96, 96), seed=85 + i) for i in range(2)]          # uint8-valued, as load_video gives
    assert clips[0].max() > 200 and clips[0].min() >= 0
    mixd, v1, v2 = _on(dev, mix, clips[0][None], clips[1][None])
    out = m(mixd, v1, v2, mix_audio=None)        # further batch keys are accepted and unused
    got = (out["s1_spec_pred"], out["s2_spec_pred"])

    def chain(dtype):
        pre = [((torch.from_numpy(c).to(dtype) / 255.0)[:, 4:92, 4:92] - 0.421) / 0.165 for c in clips]
        e = [LR.run(lw, p[None, None], dtype, relu_type="swish") for p in pre]
        return R.run(w, mix, e[0], e[1], dtype)

    _judge(got, chain(torch.float64), chain(torch.float32), "forward on raw 96 x 96 clips")
    # the lip reader's own windowed forward on the raw frames is what forward used
    emb = m.lipreader.forward_window(torch.cat([v1, v2]), (4, 4, 88, 88), (1.0 / (255.0 * 0.165), -0.421 / 0.165))
    assert emb.shape == (2, Tv, 512) and not torch.equal(emb[0], emb[1])
    want = m.forward_embeddings(mixd, emb[:1], emb[1:])
    for k in ("s1_spec_pred", "s2_spec_pred"):
        assert out[k].shape == (B, F, W) and torch.equal(out[k], want[k]), k
    assert not torch.equal(out["s1_spec_pred"], out["s2_spec_pred"])
    # the frames as they are, uncropped and unnormalised, give something else by orders of magnitude more than rounding
    raw = m.lipreader(torch.cat([v1, v2]).unsqueeze(1), lengths=[Tv] * 2)
    off = m.forward_embeddings(mixd, raw[:1], raw[1:])
    far = R.worst_col((off["s1_spec_pred"].cpu(), off["s2_spec_pred"].cpu()), (got[0].cpu(), got[1].cpu()))
    print(f"unprocessed frames: worst column {far:.3e} away")
    assert far > 1e-4
    with pytest.raises(ValueError, match="smaller"):
        m(mixd, v1[:, :, :80], v2[:, :, :80])


def test_magnitude_on_the_device(dev):
    """voicefilter_magnitude against the reference's formula on torch.stft in fp64, T = 3200, n_fft = 400, hop = 100.

    Derivation of the bounds (u = 2^-24).  Every Re / Im of the device STFT is within d of the exact one, d the bound that
    tests/test_gpu_spectral.py holds STFT to (spec_ref.stft_bound, per frame).  So m = |S| is within dm = sqrt(2) d + 4 u m
    (two squares, a sum and a root).  max(., 1e-5) and both clamps are 1-Lipschitz -- a clamp is continuous, so nothing more
    is allowed at the clamp points than next to them -- and spec = 0.2 log10(m) + 0.8 between them, whose slope is
    0.2 / (m ln 10), largest at the lower end of the interval [mc - dm, mc + dm], mc = max(m, 1e-5).  Hence
        |spec - spec64| <= 0.2 / ln 10 * dm / (mc - dm)  +  8 u (|20 log10 mc| + 20) / 100  +  4 u
    (the second term: log10, the product, the difference and the quotient, each rounding a value of at most that size; the
    third: the final clamp, sum and the result).  Where mc <= 2 dm the first term says nothing and the bound is the width
    of the range, 1; such points are counted and must be rare.  Where d = 0 (silence) the bound is rounding only.
    phase is compared where m >= 8 sqrt(2) d: there the exact and the computed S are within an angle asin(sqrt(2) d / m)
    <= 1.01 sqrt(2) d / m, plus 16 u for atan2 itself (3 ulp of a value up to pi); the difference is taken modulo 2 pi."""
    from speech_separation_amd import voicefilter_magnitude
    T, N, H = 3200, 400, 100
    rng = np.random.Generator(np.random.PCG64(6))
    x = (rng.standard_normal((2, T)) * 0.05).astype(np.float32)
    x[0, :900] = 0.0
    x[1, 2000:2600] += (0.9 * np.sin(2 * np.pi * 0.06 * np.arange(600))).astype(np.float32)
    spec, phase = voicefilter_magnitude(torch.from_numpy(x).to(dev), N, H)
    assert tuple(spec.shape) == tuple(phase.shape) == (2, 201, 33) and spec.is_contiguous()
    s1, p1 = voicefilter_magnitude(torch.from_numpy(x[1]).to(dev), N, H)
    assert torch.equal(s1, spec[1]) and torch.equal(p1, phase[1])
    want, wphase, m = R.magnitude(torch.from_numpy(x).double(), N, H)
    u = 2.0 ** -24
    d = SR.stft_bound(x, N, H)[:, None, :]                      # [B][1][frames]
    dm = math.sqrt(2.0) * d + 4 * u * m
    mc = torch.clamp(m, min=1e-5)
    bound = 0.2 / math.log(10.0) * dm / (mc - dm) + 8 * u * ((20 * torch.log10(mc)).abs() + 20) / 100 + 4 * u
    trivial = mc <= 2 * dm
    bound = torch.where(trivial, torch.ones_like(bound), bound)
    err = (spec.cpu().double() - want).abs()
    print(f"magnitude: worst error / bound {float((err / bound).max()):.4f}, trivial bounds {float(trivial.double().mean()):.4f}, "
          f"worst error {float(err.max()):.3e}")
    assert float(trivial.double().mean()) < 0.02
    assert bool((err <= bound).all())
    assert float(spec.min()) == 0.0 and float(spec.max()) == 1.0
    assert bool((spec[0, :, :6] == 0).all())                    # frames that see only the silent stretch
    sel = m >= 8 * math.sqrt(2.0) * d.expand_as(m)
    sel &= m > 0
    assert float(sel.double().mean()) > 0.5
    diff = torch.remainder(phase.cpu().double() - wphase + math.pi, 2 * math.pi) - math.pi
    pb = 1.01 * math.sqrt(2.0) * d.expand_as(m) / torch.clamp(m, min=1e-30) + 16 * u
    print(f"phase: compared {float(sel.double().mean()):.3f} of the bins, worst error / bound {float((diff.abs() / pb)[sel].max()):.4f}")
    assert bool((diff.abs()[sel] <= pb[sel]).all())
