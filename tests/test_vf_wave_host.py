"""VoiceFilter's waveform ends, host layer (no GPU needed): the C ABI of include/vfwave.h (declared == bound == exported,
plain C99); the fp64 restatement tests/vf_wave_ref.py pinned against torch.stft / abs / angle / istft in fp64 and against the
reference's own get_magnitude (tests/golden/vf_wave_small.npz, tools/gen_golden_vf_wave.py); that the synthesis bound can
tell right from wrong (four mutations, each more than 10 x the bound away); the share of bins the GPU test's phasor rule
compares, on exactly the GPU test's inputs; and the argument refusals of the Python surface."""
from __future__ import annotations

import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import speech_separation_amd as ssa
from speech_separation_amd import _lib
from tests import vf_wave_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "vfwave.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "vf_wave_small.npz")


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(vfwave_\w+)\s*\(", src))
    assert declared == set(_lib.VFWAVE_SYMBOLS), declared ^ set(_lib.VFWAVE_SYMBOLS)
    m = re.search(r"#define VFWAVE_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.VFWAVE_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.vfwave_abi_version() == _lib.VFWAVE_ABI_VERSION
    assert b"n_src" in lib.vfwave_strerror(1)
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(vfwave_\w+)$", out, re.M))
    assert exported == set(_lib.VFWAVE_SYMBOLS), exported ^ set(_lib.VFWAVE_SYMBOLS)


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _torch_chain(x, N, H):
    """get_magnitude's operators in fp64 -> S, |S|, spec, angle, each [B][F][W]"""
    S = torch.stft(x, n_fft=N, hop_length=H, win_length=N, window=torch.hann_window(N, dtype=x.dtype), center=True,
                   return_complex=True)
    mag = torch.abs(S)
    spec = torch.clamp((20.0 * torch.log10(torch.clamp(mag, min=1e-5)) - 20) / 100, min=-1.0, max=0.0) + 1.0
    return S, mag, spec, torch.angle(S)


@pytest.mark.parametrize("N,H,B,T", [V.SHAPES[1], V.SHAPES[4]])        # shapes with wholly silent frames
def test_analysis_restates_torch_in_fp64(N, H, B, T):
    """Away from the clamps to 1e-12; at the clamps (|S| >= 10, |S| <= 1e-4 -- silence included) exactly 1 and 0; the phasor is
    e^{i angle} where S is not zero and (1, 0) where it is."""
    x = torch.from_numpy(V.noise(N, H, B, T)).double()
    S, mag, want, angle = _torch_chain(x, N, H)
    spec, phasor, m = V.analysis(x, N, H)
    assert tuple(spec.shape) == (B, N // 2 + 1, 1 + T // H) and tuple(phasor.shape) == (B, 2, N // 2 + 1, 1 + T // H)
    assert float((m - mag).abs().max()) <= 1e-12 * float(mag.max())
    assert float((spec - want).abs().max()) <= 1e-12
    hi, lo = mag >= 10 * (1 + 1e-9), mag <= 1e-4 * (1 - 1e-9)
    assert int(hi.sum()) > 0 and int(lo.sum()) > 0              # the tone and the silent stretch
    assert bool((spec[hi] == 1.0).all()) and bool((want[hi] == 1.0).all())
    assert bool((spec[lo] == 0.0).all()) and bool((want[lo] == 0.0).all())
    zero = mag == 0
    assert int(zero.sum()) > 0
    assert bool((phasor[:, 0][zero] == 1.0).all()) and bool((phasor[:, 1][zero] == 0.0).all())
    # (torch.angle gives 0 for +0 and pi for a -0 that an FFT may leave; the definition takes angle(0) = 0)
    loud = mag > 1e-9
    assert float((phasor[:, 0] - torch.cos(angle)).abs()[loud].max()) <= 1e-12
    assert float((phasor[:, 1] - torch.sin(angle)).abs()[loud].max()) <= 1e-12


@pytest.mark.parametrize("N,H,B,T", V.SHAPES[:2] + V.SHAPES[4:])
def test_synthesis_restates_torch_istft_in_fp64(N, H, B, T):
    x = V.noise(N, H, B, T)
    preds, phasor = V.predictions(x, N, H, 2)
    window = torch.hann_window(N, dtype=torch.float64)
    for kind, p in preds.items():
        mag = 10.0 ** (5.0 * torch.clamp(p.double(), 0.0, 1.0) - 4.0)
        assert float(mag.min()) >= 1e-4 * (1 - 1e-12) and float(mag.max()) <= 10 * (1 + 1e-12)
        X = torch.complex(mag * phasor[:, 0].double(), mag * phasor[:, 1].double()).reshape(2 * B, *p.shape[2:])
        for L in V.lengths(N, H, T):
            got = V.synthesis(p, phasor, N, H, L).reshape(2 * B, L)
            nat = (T // H) * H
            # torch.istft refuses a length whose tail no frame reaches with a non-zero window; compare what it accepts
            n = min(L, nat + N // 2 - 1)
            want = torch.istft(X, n_fft=N, hop_length=H, win_length=N, window=window, center=True, length=n)
            scale = float(want.abs().max())
            assert float((got[:, :n] - want).abs().max()) <= 1e-12 * max(scale, 1.0), (kind, L)
    if (N, H, T) == (400, 100, 2000):
        p = preds["[-0.5, 1.5]"]
        assert float(p.min()) < -0.4 and float(p.max()) > 1.4


def test_against_the_references_get_magnitude():
    """The fixture holds the reference's fp32 results: held to the bounds the kernel is held to (an fp32 FFT is well inside
    the dot-product bound).  The phase on the compared bins, modulo 2 pi."""
    z = np.load(GOLDEN)
    i = 0
    while f"x{i}" in z:
        N, H, B, T = (int(v) for v in z[f"shape{i}"])
        x = z[f"x{i}"]
        assert np.array_equal(x, V.noise(N, H, B, T))
        spec, phasor, m = V.analysis(x, N, H)
        bound, trivial, _, _ = V.spec_bound(x, N, H)
        assert float(trivial.double().mean()) < 0.02
        err = (torch.from_numpy(z[f"spec{i}"]).double() - spec).abs()
        assert bool((err <= bound).all()), float((err / bound).max())
        sel, pb = V.phasor_rule(x, N, H)
        diff = torch.from_numpy(z[f"phase{i}"]).double() - torch.atan2(phasor[:, 1], phasor[:, 0])
        diff = torch.remainder(diff + math.pi, 2 * math.pi) - math.pi
        assert float(sel.double().mean()) >= V.MIN_COMPARED
        sel &= m > 0                                            # the sign of a zero decides torch.angle there
        assert bool((diff.abs()[sel] <= (pb + V.ATAN2_ROUNDINGS * V.U)[sel]).all())
        i += 1
    assert i == 2


@pytest.mark.parametrize("N,H,B,T", V.SHAPES)
def test_compared_share_of_the_gpu_tests_inputs(N, H, B, T):
    """The fp64 restatement is the same on every machine: the share of bins the phasor rule compares on the GPU test's
    inputs is checked here, once, and the spec bound says something on nearly all of them."""
    x = V.noise(N, H, B, T)
    sel, _ = V.phasor_rule(x, N, H)
    _, trivial, _, _ = V.spec_bound(x, N, H)
    print(f"({N}, {H}) x ({B}, {T}): compared {float(sel.double().mean()):.4f}, trivial spec bounds {float(trivial.double().mean()):.4f}")
    assert float(sel.double().mean()) >= V.MIN_COMPARED
    assert float(trivial.double().mean()) < 0.02


@pytest.mark.parametrize("N,H,B,T", [V.SHAPES[1], V.SHAPES[4]])
def test_the_synthesis_bound_tells_right_from_wrong(N, H, B, T):
    """Each mutation moves the result by more than 10 x the bound somewhere: dropping the clamp, the conjugate phasor,
    4.9 for the factor 5, Im of bin N / 2 let in."""
    x = V.noise(N, H, B, T)
    preds, phasor = V.predictions(x, N, H, 1)
    p = preds["[-0.5, 1.5]"]
    phasor = phasor.clone()
    phasor[:, 1, -1] = 0.5                                      # an Im at bin N / 2 that a correct inverse never reads
    for L in V.lengths(N, H, T):
        ref = V.synthesis(p, phasor, N, H, L)
        bound = V.synthesis_bound(p, phasor, N, H, L)
        live = bound > 0
        for name, kw in (("no clamp", {"clamp": False}), ("conjugate phasor", {"conjugate": True}), ("factor 4.9", {"factor": 4.9}),
                         ("Im of bin N / 2", {"edge_imag": True})):
            off = (V.synthesis(p, phasor, N, H, L, **kw) - ref).abs()
            worst = float((off[live] / bound[live]).max())
            print(f"({N}, {H}) length {L}: {name} lands at {worst:.1f} x the bound")
            assert worst > 10.0, (name, L, worst)


def test_round_trip_bound_is_small_against_the_signal():
    """The composed bound stays a statement about rounding.  It is a worst case: per bin it allows about dm + mag dphasor,
    some 5e-4 on 0.05 rms noise whatever the bin holds, and adds the F bins with absolute values where the signal adds them
    incoherently -- a few per cent of the waveform's rms, not more."""
    N, H, B, T = V.SHAPES[1]
    x = V.noise(N, H, B, T)
    spec, phasor, _ = V.analysis(x, N, H)
    y = V.synthesis(spec[None], phasor, N, H, T)
    b = V.round_trip_bound(x, N, H, T)
    print(f"round trip: bound rms {float(b.pow(2).mean().sqrt()):.3e}, signal rms {float(y.pow(2).mean().sqrt()):.3e}")
    assert float(b.pow(2).mean().sqrt()) < 0.1 * float(y.pow(2).mean().sqrt())
    # and a wrong phase convention is far outside it
    off = (V.synthesis(spec[None], phasor, N, H, T, conjugate=True) - y).abs()
    assert float((off / b).max()) > 10.0


def test_refusals_of_the_python_surface():
    x = torch.zeros(2, 1000)
    with pytest.raises(TypeError, match="float32"):
        ssa.voicefilter_analysis(x.double())
    with pytest.raises(ValueError, match="dimensions"):
        ssa.voicefilter_analysis(x[None, None])
    with pytest.raises(ValueError, match="n_fft / 2"):
        ssa.voicefilter_analysis(x[:, :200])
    with pytest.raises(ValueError, match="n_fft"):
        ssa.voicefilter_analysis(x, n_fft=100)
    with pytest.raises(RuntimeError, match="no CPU"):
        ssa.voicefilter_analysis(x)
    F, W = 201, 11
    ph = torch.zeros(2, 2, F, W)
    with pytest.raises(ValueError, match="1 to 4"):
        ssa.voicefilter_waveforms(torch.zeros(5, 2, F, W), ph)
    with pytest.raises(ValueError, match="1 to 4"):
        ssa.voicefilter_waveforms([], ph)
    with pytest.raises(TypeError, match="float32"):
        ssa.voicefilter_waveforms(torch.zeros(1, 2, F, W, dtype=torch.float16), ph)
    with pytest.raises(ValueError, match="dimensions"):
        ssa.voicefilter_waveforms(torch.zeros(2, F, W), ph)
    with pytest.raises(ValueError, match="as the phasor"):
        ssa.voicefilter_waveforms(torch.zeros(1, 2, F, W + 1), ph)
    with pytest.raises(ValueError, match="phasor must be"):
        ssa.voicefilter_waveforms(torch.zeros(1, 2, F, W), ph, n_fft=256, hop_length=128)
    with pytest.raises(ValueError, match="at least 1"):
        ssa.voicefilter_waveforms(torch.zeros(1, 2, F, 1), torch.zeros(2, 2, F, 1))
    with pytest.raises(RuntimeError, match="no CPU"):
        ssa.voicefilter_waveforms(torch.zeros(1, 2, F, W), ph, 1000)
    with pytest.raises(RuntimeError, match="no CPU"):
        ssa.voicefilter_waveforms([torch.zeros(2, F, W)] * 2, ph)
    m = ssa.VoiceFilter(201).eval()
    with pytest.raises(ValueError, match="n_fft"):
        ssa.VoiceFilterSeparator(m, n_fft=256)
    sep = ssa.VoiceFilterSeparator(m)
    assert (sep.n_fft, sep.hop_length) == (400, 100)
    with pytest.raises(ValueError, match="neither"):
        sep(mix=x, s1=None)
    with pytest.raises(RuntimeError, match="no CPU"):
        sep(mix=x, s1_embedding=torch.zeros(2, 1024, 5), s2_embedding=torch.zeros(2, 1024, 5))
    with pytest.raises(RuntimeError, match="lip reader"):
        m.separate(x, torch.zeros(2, 5, 96, 96), torch.zeros(2, 5, 96, 96))
    with pytest.raises(RuntimeError, match="eval"):
        ssa.VoiceFilter(201).train().separate_embeddings(x, torch.zeros(2, 5, 1024), torch.zeros(2, 5, 1024))
    batch = {"mix": x, "s1": None}
    with pytest.raises(RuntimeError, match="no CPU"):
        ssa.add_magnitude_keys(batch)
    assert sorted(batch) == ["mix", "s1"]


def test_loader_carries_the_videos_an_entry_names(tmp_path):
    """Opt-in: an entry with s1_video_path / s2_video_path gets the `data` array of each .npz as (1, Tv, H, W) float32
    (base_dataset.load_video) and the batcher moves them with the other inputs; an entry without them is as before."""
    from speech_separation_amd.io import PinnedBatcher, collate, load_item
    from tests.dataset_fixture import make_dataset
    entries, _ = make_dataset(str(tmp_path), n=3, T=800, Tv=4, emb=16)
    plain = load_item(entries[0])
    assert plain["s1_video"] is None and plain["s2_video"] is None
    rng = np.random.default_rng(3)
    clips = rng.integers(0, 256, (3, 2, 4, 6, 5)).astype(np.uint8)
    for i, e in enumerate(entries):
        for k in (0, 1):
            path = str(tmp_path / f"utt{i}_s{k + 1}_mouth.npz")
            np.savez_compressed(path, data=clips[i, k])
            e[f"s{k + 1}_video_path"] = path
    items = [load_item(e) for e in entries]
    assert items[1]["s2_video"].shape == (1, 4, 6, 5) and items[1]["s2_video"].dtype == torch.float32
    assert np.array_equal(items[1]["s2_video"][0].numpy(), clips[1, 1].astype(np.float32))
    for batch in (collate(items), PinnedBatcher("cpu").to_device(items)):
        assert batch["s1_video"].shape == (3, 4, 6, 5) and np.array_equal(batch["s2_video"].numpy(), clips[:, 1].astype(np.float32))
        assert batch["mix"].shape == (3, 800) and batch["s1_embedding"].shape == (3, 16, 4)
    assert PinnedBatcher("cpu").to_device([plain])["s1_video"] is None
