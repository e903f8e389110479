"""VoiceFilter's waveform ends on the MI355X (include/vfwave.h; voicefilter_analysis, voicefilter_waveforms,
VoiceFilter.separate_embeddings, add_magnitude_keys) against the fp64 restatement tests/vf_wave_ref.py, under the bounds
derived in that file's docstring.  Shapes (n_fft, hop) x (B, T): vf_wave_ref.SHAPES -- T just above n_fft / 2 with both ends
reflected inside one frame, the golden VoiceFilter width, a width that is no multiple of a tile, 17 items of odd alignment,
a hop that does not divide n_fft.  The references are computed once per shape and shared.  Every comparison prints its
worst error / bound before it asserts (DESIGN.md section 27 quotes them)."""
from __future__ import annotations

import functools
import math
import os

import numpy as np
import pytest
import torch

from tests import vf_wave_ref as V

pytestmark = pytest.mark.gpu
IDS = ["%dx%d_%dx%d" % s for s in V.SHAPES]
WORST = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(i):
    """fp64 references of shape i, read-only: inputs, analysis, its bounds."""
    N, H, B, T = V.SHAPES[i]
    x = V.noise(N, H, B, T)
    spec, phasor, m = V.analysis(x, N, H)
    bound, trivial, _, _ = V.spec_bound(x, N, H)
    sel, pb = V.phasor_rule(x, N, H)
    return dict(x=x, spec=spec, phasor=phasor, m=m, bound=bound, trivial=trivial, sel=sel, pb=pb)


def _record(what, err, bound):
    live = bound > 0
    assert bool((err[~live] == 0).all()), what                  # a zero bound: nothing reaches the sample, the result is 0
    ratio = float((err[live] / bound[live]).max()) if bool(live.any()) else 0.0
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print(f"vf_wave {what}: worst error {float(err.max()):.3e}, error / bound {ratio:.4f}")
    return ratio


def _analysis(dev, x, N, H):
    from speech_separation_amd import voicefilter_analysis
    spec, phasor = voicefilter_analysis(torch.from_numpy(np.ascontiguousarray(x)).to(dev), N, H)
    return spec, phasor


@pytest.mark.parametrize("i", range(len(V.SHAPES)), ids=IDS)
def test_analysis_against_the_fp64_restatement(dev, i):
    N, H, B, T = V.SHAPES[i]
    c = _case(i)
    spec, phasor = _analysis(dev, c["x"], N, H)
    F, W = N // 2 + 1, 1 + T // H
    assert tuple(spec.shape) == (B, F, W) and tuple(phasor.shape) == (B, 2, F, W)
    assert spec.is_contiguous() and phasor.is_contiguous() and spec.dtype == phasor.dtype == torch.float32
    got, gph = spec.cpu().double(), phasor.cpu().double()
    assert bool(torch.isfinite(got).all()) and bool(torch.isfinite(gph).all())
    assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    assert float(c["trivial"].double().mean()) < 0.02
    r = _record(f"spec {IDS[i]}", (got - c["spec"]).abs(), c["bound"])
    assert r <= 1.0
    share = float(c["sel"].double().mean())
    print(f"vf_wave phasor {IDS[i]}: compared {share:.4f} of the bins")
    assert share >= V.MIN_COMPARED
    sel = c["sel"][:, None].expand_as(gph)
    err = torch.where(sel, (gph - c["phasor"]).abs(), torch.zeros_like(gph))
    r = _record(f"phasor {IDS[i]}", err, c["pb"][:, None].expand_as(gph))
    assert r <= 1.0
    norm = (gph[:, 0] ** 2 + gph[:, 1] ** 2).sqrt()
    assert float((norm - 1).abs().max()) <= 8 * V.U             # a unit vector everywhere, compared or not


def test_hard_values_are_exact(dev):
    N, H, T = 400, 100, 2400
    rng = np.random.Generator(np.random.PCG64(11))
    x = np.zeros((4, T), dtype=np.float32)
    x[1] = rng.standard_normal(T) * 0.3
    x[1, 900:1500] = 0.0                                        # a silent stretch longer than a window inside a loud item
    k = 24
    x[2] = 0.9 * np.cos(2 * np.pi * k * np.arange(T) / N)       # a tone on the centre of bin 24: |S| = 0.9 N / 4 = 90, neighbours 45
    x[3, [0, N // 2, T - 1]] = 1.0                              # unit impulses at n = 0, N / 2, T - 1
    spec, phasor = _analysis(dev, x, N, H)
    spec, phasor = spec.cpu(), phasor.cpu()
    assert bool((spec[0] == 0).all()) and bool((phasor[0, 0] == 1).all()) and bool((phasor[0, 1] == 0).all())
    quiet = slice(11, 14)                                       # frames m with [100 m - 200, 100 m + 200) inside [900, 1500)
    assert bool((spec[1, :, quiet] == 0).all()) and bool((phasor[1, 0, :, quiet] == 1).all()) and bool((phasor[1, 1, :, quiet] == 0).all())
    assert float(spec[1, :, :9].min()) > 0.0
    assert bool((spec[2, k - 1:k + 2, 2:-2] == 1.0).all())
    assert float(spec[2, k + 4:, 2:-2].max()) < 1.0
    # an impulse of height 1 at offset t of a frame gives |S_k| = w[t] for every k: frames that see exactly one impulse
    want, wph, m = V.analysis(x[3:], N, H)
    bound, _, _, _ = V.spec_bound(x[3:], N, H)
    assert _record("spec impulses", (spec[3:].double() - want).abs(), bound) <= 1.0
    sel, pb = V.phasor_rule(x[3:], N, H)
    assert float(sel.double().mean()) > 0.2
    err = torch.where(sel[:, None].expand(1, 2, -1, -1), (phasor[3:].double() - wph).abs(), torch.zeros(1, 2, *sel.shape[1:], dtype=torch.float64))
    assert _record("phasor impulses", err, pb[:, None].expand(1, 2, -1, -1)) <= 1.0
    far = slice(5, 20)                                          # frames no impulse reaches
    assert bool((spec[3, :, far] == 0).all()) and bool((phasor[3, 0, :, far] == 1).all())


@pytest.mark.parametrize("n_src", [1, 2])
@pytest.mark.parametrize("i", range(len(V.SHAPES)), ids=IDS)
def test_synthesis_against_the_fp64_restatement(dev, i, n_src):
    from speech_separation_amd import voicefilter_waveforms
    N, H, B, T = V.SHAPES[i]
    preds, phasor = V.predictions(_case(i)["x"], N, H, n_src)
    ph = phasor.to(dev)
    for kind, p in preds.items():
        pd = p.to(dev)
        for L in V.lengths(N, H, T) + ([(T // H) * H + N // 2 + 10] if i == 0 else []):     # the last: past every frame's reach
            y = voicefilter_waveforms(pd, ph, L, N, H)
            assert tuple(y.shape) == (n_src, B, L) and y.is_contiguous()
            got = y.cpu().double()
            assert bool(torch.isfinite(got).all())
            r = _record(f"synthesis {IDS[i]} {kind}", (got - V.synthesis(p, phasor, N, H, L)).abs(), V.synthesis_bound(p, phasor, N, H, L))
            assert r <= 1.0, (kind, L)
            if L > (T // H) * H + N // 2:
                assert bool((got[..., (T // H) * H + N // 2:] == 0).all())
    nat = voicefilter_waveforms(pd, ph, None, N, H)
    assert nat.shape[-1] == (T // H) * H and torch.equal(nat, voicefilter_waveforms(pd, ph, (T // H) * H, N, H))


@pytest.mark.parametrize("i", range(len(V.SHAPES)), ids=IDS)
def test_round_trip_against_the_fp64_composition(dev, i):
    from speech_separation_amd import voicefilter_waveforms
    N, H, B, T = V.SHAPES[i]
    c = _case(i)
    spec, phasor = _analysis(dev, c["x"], N, H)
    y = voicefilter_waveforms(spec[None], phasor, T, N, H)
    want = V.synthesis(c["spec"][None], c["phasor"], N, H, T)
    assert _record(f"round trip {IDS[i]}", (y.cpu().double() - want).abs(), V.round_trip_bound(c["x"], N, H, T)) <= 1.0


@pytest.mark.parametrize("i", [1, 3, 4], ids=[IDS[1], IDS[3], IDS[4]])
def test_repeatable_and_independent_of_the_batch_and_of_n_src(dev, i):
    from speech_separation_amd import voicefilter_waveforms
    N, H, B, T = V.SHAPES[i]
    x = V.noise(N, H, 3, T)
    a, pa = _analysis(dev, x, N, H)
    b, pb = _analysis(dev, x, N, H)
    assert torch.equal(a, b) and torch.equal(pa, pb)
    for k in (0, 2):
        s, p = _analysis(dev, x[k:k + 1], N, H)
        assert torch.equal(s[0], a[k]) and torch.equal(p[0], pa[k]), k
    preds, phasor = V.predictions(x, N, H, 2)
    ph = phasor.to(dev)
    for L in V.lengths(N, H, T):
        for kind, p in preds.items():
            pd = p.to(dev)
            y = voicefilter_waveforms(pd, ph, L, N, H)
            assert torch.equal(y, voicefilter_waveforms(pd, ph, L, N, H)), (kind, L)
            for s in range(2):
                assert torch.equal(voicefilter_waveforms(pd[s:s + 1], ph, L, N, H)[0], y[s]), (kind, L, s)
            for k in (0, 2):
                one = voicefilter_waveforms(pd[:, k:k + 1].contiguous(), ph[k:k + 1], L, N, H)
                assert torch.equal(one[:, 0], y[:, k]), (kind, L, k)
    # maps that are not one stack's slices: one launch per source into the slices of a caller's result, no copy
    out = torch.full((2, 3, T), float("nan"), device=dev)
    y2 = voicefilter_waveforms([pd[0].clone(), pd[1].clone()], ph, T, N, H, out=out)
    assert y2.data_ptr() == out.data_ptr() and torch.equal(y2, voicefilter_waveforms(pd, ph, T, N, H))
    assert torch.equal(voicefilter_waveforms([pd[0], pd[1]], ph, T, N, H), y2)


def test_c_abi_refuses_without_a_launch(dev):
    import ctypes
    from speech_separation_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.specfe_create(400, 100, ctypes.byref(h)) == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    o = torch.full((4 * 2 * 2 * 201 * 11,), 7.0, device=dev)
    s = torch.zeros(4 * 2 * 2 * 201 * 11, device=dev)
    a, b = o.data_ptr(), s.data_ptr()
    bad = [lib.vfwave_analysis(h, b, 2, 200, a, a, stream), lib.vfwave_analysis(h, b, 0, 1000, a, a, stream),
           lib.vfwave_analysis(None, b, 2, 1000, a, a, stream), lib.vfwave_analysis(h, None, 2, 1000, a, a, stream),
           lib.vfwave_analysis(h, b, 2, 1000, None, a, stream), lib.vfwave_analysis(h, b, 2, 1000, a, None, stream),
           lib.vfwave_analysis(h, b, 1, 1 << 27, a, a, stream),
           lib.vfwave_synthesis(h, b, b, 0, 2, 11, 1000, a, stream), lib.vfwave_synthesis(h, b, b, 5, 2, 11, 1000, a, stream),
           lib.vfwave_synthesis(h, b, b, 2, 0, 11, 1000, a, stream), lib.vfwave_synthesis(h, b, b, 2, 2, 0, 1000, a, stream),
           lib.vfwave_synthesis(h, b, b, 2, 2, 1, 0, a, stream), lib.vfwave_synthesis(h, None, b, 2, 2, 11, 1000, a, stream),
           lib.vfwave_synthesis(h, b, None, 2, 2, 11, 1000, a, stream), lib.vfwave_synthesis(h, b, b, 2, 2, 11, 1000, None, stream),
           lib.vfwave_synthesis(h, b, b, 2, 2, 11, 1 << 27, a, stream), lib.vfwave_synthesis(None, b, b, 2, 2, 11, 1000, a, stream)]
    torch.cuda.synchronize()
    assert bad == [1] * len(bad), bad
    assert bool((o == 7.0).all())
    lib.specfe_destroy(h)
    from speech_separation_amd import voicefilter_waveforms
    with pytest.raises(ValueError, match="1 to 4"):
        voicefilter_waveforms(torch.zeros(5, 2, 201, 11, device=dev), torch.zeros(2, 2, 201, 11, device=dev))


@functools.lru_cache(maxsize=None)
def _separate_case():
    from tests import voicefilter_ref as R
    F, W, Tv, B = 201, 21, 5, 2
    N, H, T = 400, 100, 2000
    rng = np.random.Generator(np.random.PCG64(21))
    s = (rng.standard_normal((2, B, T)) * 0.05).astype(np.float32)
    s[0] *= (0.5 + 0.5 * np.sin(2 * np.pi * np.arange(T) / 700.0)).astype(np.float32)
    mix = s[0] + s[1]
    _, e1, e2 = R.synthetic_inputs(F, W, Tv, B, 1024, seed=91)
    w = R.synthetic_voicefilter_weights(F, 1024, R.WEIGHT_SEED)
    spec, phasor, _ = V.analysis(mix, N, H)
    p1, p2 = (torch.as_tensor(p).double() for p in R.run(w, spec.numpy(), e1, e2, torch.float64))
    y = V.synthesis(torch.stack([p1, p2]), phasor, N, H, T)
    return dict(mix=mix, s1=s[0], s2=s[1], e1=e1, e2=e2, w=w, y64=y.numpy(), shape=(F, W, Tv, B), NHT=(N, H, T))


def test_separate_runs_the_three_parts_and_feeds_the_metrics(dev):
    import speech_separation_amd as S
    from speech_separation_amd.metrics import SISNRiMetric
    from oracle import dptn_oracle as O
    from tests import stoi_ref as SR2
    c = _separate_case()
    F, W, Tv, B = c["shape"]
    N, H, T = c["NHT"]
    m = S.VoiceFilter(F)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["w"].items()}, strict=True)
    m = m.to(dev).eval()
    mix, s1, s2, e1, e2 = (torch.from_numpy(c[k]).to(dev) for k in ("mix", "s1", "s2", "e1", "e2"))
    out = m.separate_embeddings(mix, e1, e2)
    assert sorted(out) == ["mix_magnitude", "s1_pred", "s1_spec_pred", "s2_pred", "s2_spec_pred"]
    spec, phasor = S.voicefilter_analysis(mix, N, H)
    want = m.forward_embeddings(spec, e1, e2)
    assert torch.equal(out["mix_magnitude"], spec)
    for k in ("s1_spec_pred", "s2_spec_pred"):
        assert tuple(out[k].shape) == (B, F, W) and torch.equal(out[k], want[k]), k
    y = S.voicefilter_waveforms([want["s1_spec_pred"], want["s2_spec_pred"]], phasor, T, N, H)
    assert out["s1_pred"].shape == mix.shape and torch.equal(out["s1_pred"], y[0]) and torch.equal(out["s2_pred"], y[1])
    assert not torch.equal(out["s1_pred"], out["s2_pred"])
    # (B, 1, T) mixtures keep their shape; the callable of evaluate / run_inference takes the loader's (B, E, Tv) embeddings
    sep = S.VoiceFilterSeparator(m, N, H)
    o3 = sep(mix=mix[:, None], s1_embedding=e1.transpose(1, 2).contiguous(), s2_embedding=e2.transpose(1, 2).contiguous(), s1=s1, s2=s2)
    assert o3["s1_pred"].shape == (B, 1, T) and torch.equal(o3["s1_pred"][:, 0], out["s1_pred"])
    # the waveform metrics on the resulting batch against the fp64 chain's waveforms, each under its own GPU test's tolerance
    batch = dict(mix=mix, s1=s1, s2=s2, **out)
    y64 = c["y64"]
    p32 = [y64[0].astype(np.float32), y64[1].astype(np.float32)]
    got = float(SISNRiMetric(name="SISNRiMetric")(**batch))
    ref = O.si_snri_metric(p32[0], p32[1], c["s1"], c["s2"], c["mix"])
    print(f"separate: SI-SNRi {got:.6f} dB, from the fp64 chain {ref:.6f} dB")
    assert math.isfinite(got) and abs(got - ref) < 1e-3                       # tests/test_gpu_parity.py
    got = S.SISDRMetric()(**batch)
    ref = SR2.pit(SR2.sisdr_pairs(y64[0], y64[1], c["s1"], c["s2"]))
    print(f"separate: SI-SDR {got:.6f} dB, from the fp64 chain {ref:.6f} dB")
    assert math.isfinite(got) and abs(got - ref) <= 1e-5 * abs(ref)           # tests/test_gpu_wavmetric.py::test_metric_classes
    got = S.STOIMetric(16000)(**batch)
    v64 = SR2.values(SR2.spectra(p32[0], p32[1], c["s1"], c["s2"], 16000, np.float64), False)
    v32 = SR2.values(SR2.spectra(p32[0], p32[1], c["s1"], c["s2"], 16000, np.float32), False)
    bound = (2 * np.abs(v32 - v64) + 32 * V.U).mean(0).max()                  # tests/wavmetric_cases.bound, as test_metric_classes
    print(f"separate: STOI {got:.6e}, from the fp64 chain {SR2.pit(v64):.6e}, bound {bound:.2e}")
    assert math.isfinite(got) and abs(got - SR2.pit(v64)) <= bound


def test_run_inference_carries_a_voicefilter(dev, tmp_path):
    """The tenth model class through the evaluation loop: the loader's batches (embeddings as make_embeddings stores them,
    (E, Tv)), VoiceFilterSeparator, the waveform metrics, the prediction writer; and the files hold what separate_embeddings
    gives for the same items."""
    import speech_separation_amd as S
    from speech_separation_amd.evaluate import run_inference
    from speech_separation_amd.io import collate, load_item
    from speech_separation_amd.metrics import SISNRiMetric
    from tests.dataset_fixture import make_dataset
    c = _separate_case()
    F = c["shape"][0]
    m = S.VoiceFilter(F)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in c["w"].items()}, strict=True)
    m = m.to(dev).eval()
    n, bs, T = 5, 2, 2000
    entries, _ = make_dataset(str(tmp_path / "data"), n=n, T=T, Tv=5, emb=1024, sr=16000)
    mets = [SISNRiMetric(name="SISNRiMetric"), S.SISDRMetric(name="SISDRMetric"), S.STOIMetric(16000, name="STOIMetric")]
    logs, stats = run_inference(S.VoiceFilterSeparator(m, 400, 100), entries, bs, mets, save_dir=str(tmp_path / "out"), device=dev,
                                workers=2, target_sr=16000)
    assert stats["items"] == n and stats["files"] == n
    assert sorted(logs) == ["SISDRMetric", "SISNRiMetric", "STOIMetric"] and all(math.isfinite(v) for v in logs.values()), logs
    b = collate([load_item(e, 16000) for e in entries[:bs]])
    out = m.separate_embeddings(b["mix"].to(dev), b["s1_embedding"].to(dev).transpose(1, 2), b["s2_embedding"].to(dev).transpose(1, 2))
    for j, ap in enumerate(b["audio_path"]):
        saved = torch.load(tmp_path / "out" / (os.path.splitext(os.path.basename(ap))[0] + ".pth"))
        assert saved["s1_pred"].shape == (T,) and torch.equal(saved["s1_pred"], out["s1_pred"][j].cpu()), j
        assert torch.equal(saved["s2_pred"], out["s2_pred"][j].cpu()), j


def test_add_magnitude_keys(dev):
    from speech_separation_amd import add_magnitude_keys
    i = 1
    N, H, B, T = V.SHAPES[i]
    c = _case(i)
    x = torch.from_numpy(c["x"]).to(dev)
    batch = add_magnitude_keys({"mix": x, "s1": x * 0.5, "s2": None, "audio_path": ["a", "b"]}, N, H)
    assert sorted(batch) == ["audio_path", "mix", "mix_magnitude", "mix_phase", "s1", "s1_spec_true", "s2"]
    assert "s2_spec_true" not in batch and batch["s2"] is None
    only = add_magnitude_keys({"mix": x[:, None]}, N, H)
    assert sorted(only) == ["mix", "mix_magnitude", "mix_phase"] and torch.equal(only["mix_magnitude"], batch["mix_magnitude"])
    from speech_separation_amd import voicefilter_analysis
    assert torch.equal(batch["mix_magnitude"], voicefilter_analysis(x, N, H)[0])
    assert torch.equal(batch["s1_spec_true"], voicefilter_analysis(x * 0.5, N, H)[0])
    assert tuple(batch["mix_phase"].shape) == (B, N // 2 + 1, 1 + T // H)
    sel = c["sel"] & (c["m"] > 0)
    want = torch.atan2(c["phasor"][:, 1], c["phasor"][:, 0])
    diff = torch.remainder(batch["mix_phase"].cpu().double() - want + math.pi, 2 * math.pi) - math.pi
    err = torch.where(sel, diff.abs(), torch.zeros_like(diff))
    assert _record("mix_phase", err, c["pb"] + V.ATAN2_ROUNDINGS * V.U) <= 1.0
    assert bool((batch["mix_phase"].cpu()[c["m"] == 0] == 0).all())            # angle(0) = 0


def test_report_worst_ratios(dev):
    """The worst error / bound ratio per map over this session (DESIGN.md section 27 quotes it)."""
    for k in sorted(WORST):
        print(f"vf_wave worst ratio {k}: {WORST[k]:.4f}")
