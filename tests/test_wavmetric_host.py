"""Evaluation metrics, host layer (no GPU needed): the C ABI of include/wavmetric.h (declared == bound == exported, plain
C99), the argument checks that need no device, the module surface of STOIMetric / SISDRMetric, and the properties of the
definition itself, tests/stoi_ref.py: the resampler's check values and its agreement with scipy.signal.resample_poly, the
band edges from pystoi's argmin rule, STOI(x, x) = 1, the all-zero and the short paths, monotonicity over the SNR, the
sensitivity of every device-test value to one misplaced band edge, and the committed fixture tests/golden/stoi_small.npz
(tools/gen_golden_stoi.py)."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from speech_separation_amd import _lib
from tests import stoi_ref as R
from tests import wavmetric_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wavmetric.h")


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(wavmetric_\w+)\s*\(", src))
    assert declared == set(_lib.WAVMETRIC_SYMBOLS), declared ^ set(_lib.WAVMETRIC_SYMBOLS)
    m = re.search(r"#define WAVMETRIC_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.WAVMETRIC_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.wavmetric_abi_version() == 1
    r = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if " T " in ln and ln.split()[-1].startswith("wavmetric_")}
    assert exported == declared, exported ^ declared


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    assert lib.wavmetric_strerror(0) == b"ok"
    assert len({lib.wavmetric_strerror(c) for c in (0, 1, 4, 99)}) == 4
    h = ctypes.c_void_p(0x1234)
    for fs in (44100, 0, 9999, -8000):
        assert lib.wavmetric_stoi_create(fs, 0, ctypes.byref(h)) == 1 and h.value == 0x1234, fs
    assert lib.wavmetric_stoi_create(16000, 0, None) == 1
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    assert lib.wavmetric_stoi_scratch_bytes(None, 2, 6000) == 0
    assert lib.wavmetric_stoi_pairs(None, p, p, p, p, 1, 4000, p, p, p, 1 << 20, None) == 1
    for B, T, ptr in ((0, 8, p), (1, 0, p), (1, 8, None), (1 << 20, 8, p)):
        assert lib.wavmetric_sisdr_pairs(p, p, p, ptr, B, T, p, None) == 1, (B, T, ptr)
    lib.wavmetric_stoi_destroy(None)                 # a no-op


def test_module_surface():
    import speech_separation_amd as S
    from speech_separation_amd.metrics import SISDRMetric, STOIMetric
    for cls in (STOIMetric, SISDRMetric):
        assert cls.__name__ in S.__all__ and getattr(S, cls.__name__) is cls
        assert cls().name == cls.__name__ and cls(name="x", device="cuda").name == "x"
        assert cls().pick is max and cls(lower_better=True).pick is min
        assert callable(cls.enqueue) and callable(cls.resolve)          # evaluate.run_inference's non-stalling branch
        z = torch.zeros(2, 4000)
        with pytest.raises(RuntimeError, match="no CPU path"):
            cls()(s1_pred=z, s2_pred=z, s1=z, s2=z, mix=z)
    # the reference's constructor (src/metrics/stoi.py): fs, extended first, then SS2BaseMetric's name / lower_better
    assert list(inspect.signature(STOIMetric.__init__).parameters)[:6] == ["self", "fs", "extended", "name", "device", "lower_better"]
    m = STOIMetric()
    assert (m.fs, m.extended) == (16000, False) and STOIMetric(8000, True).extended is True
    with pytest.raises(ValueError, match="8000, 10000 or 16000"):
        STOIMetric(fs=44100)
    assert m.resolve(torch.tensor([0.9, 0.1, 0.2, 0.5], dtype=torch.float64)) == pytest.approx(0.7)
    assert STOIMetric(lower_better=True).resolve(torch.tensor([0.9, 0.1, 0.2, 0.5], dtype=torch.float64)) == pytest.approx(0.15)


def test_resampler_check_values_and_band_edges():
    for fs, p, q, L, taps, T, n_out in ((8000, 5, 4, 182, 365, 1001, 1252), (16000, 5, 8, 290, 581, 1003, 627)):
        pp, qq, LL, g = R.resample_design(fs)
        assert (pp, qq, LL, g.shape[0]) == (p, q, L, taps)
        assert abs(g.sum() - p) < 1e-12 and np.array_equal(g, g[::-1])
        assert R.resample(np.ones(T), fs).shape[0] == n_out
    assert R.EDGES == [(7, 9), (9, 11), (11, 14), (14, 17), (17, 22), (22, 27), (27, 34), (34, 43), (43, 55), (55, 69), (69, 87),
                       (87, 109), (109, 138), (138, 174), (174, 219)]
    assert R.third_octave_edges() == R.EDGES and (R.BIN_LO, R.BIN_HI) == (7, 219)      # from the rule, not a table


@pytest.mark.parametrize("fs,T", [(8000, 1001), (16000, 1003), (16000, 32000), (8000, 32000)])
def test_resampler_equals_scipy_resample_poly(fs, T):
    from scipy.signal import resample_poly
    x = np.random.default_rng(T).standard_normal(T)
    p, q, L, g = R.resample_design(fs)
    want = resample_poly(x, p, q, window=g / p)
    got = R.resample(x, fs)
    assert got.shape == want.shape and np.max(np.abs(got - want)) <= 1e-12
    assert np.array_equal(R.resample(x, 10000), x)


def test_identity_zero_and_short_paths():
    for fs in (8000, 10000, 16000):
        x = R.gated_harmonic(2 * fs, fs, seed=fs)
        for ext in (False, True):
            v, nk, _ = R.stoi(x, x, fs, ext)
            assert nk >= 30 and abs(v - 1) <= 1e-9, (fs, ext, v)
    noise = R.add_noise(np.zeros(12000, dtype=np.float32), 0.0, seed=1)
    for ext in (False, True):
        for dtype in (np.float64, np.float32):
            v, nk, margin = R.stoi(np.zeros(12000), noise, 10000, ext, dtype)
            assert v == 0.0 and not np.isnan(v) and nk == margin.shape[0] == 92          # every frame kept, the value exactly 0
    # n * 128 active samples, then silence: frames 0 .. n - 1 are at least half active and kept, the rest dropped
    for n in (29, 30):
        x = np.concatenate([R.gated_harmonic(128 * n, 10000, seed=3, kind="full"), np.zeros(2560, dtype=np.float32)])
        v, nk, _ = R.stoi(x, R.add_noise(x, 5.0, seed=4), 10000)
        assert nk == n
        assert v == 1e-5 if n == 29 else (v != 1e-5 and 0.1 < v < 1), (n, v)
    assert R.stoi(np.ones(255), np.ones(255), 10000)[:2] == (1e-5, 0)                    # no frame at all
    x = R.gated_harmonic(3967, 10000, seed=5, kind="full")
    assert R.stoi(x, x, 10000)[:2] == (1e-5, 29) and R.stoi(np.append(x, 0), np.append(x, 0), 10000)[1] == 30


def test_stoi_falls_with_the_snr():
    x = R.gated_harmonic(24000, 16000, seed=11)
    for ext in (False, True):
        v = [R.stoi(x, R.add_noise(x, snr, seed=12), 16000, ext)[0] for snr in (20.0, 5.0, -5.0)]
        assert 1 > v[0] > v[1] > v[2] > 0, (ext, v)


def test_sisdr_formula():
    p1, p2, s1, s2 = W.case("8000Hz_2x6000")
    v = R.sisdr_pairs(p1, p2, s1, s2)
    assert v.shape == (2, 4) and np.all(np.abs(v[:, 0] - 5.0) < 0.5) and np.all(np.abs(v[:, 3] + 5.0) < 0.5)     # the SNRs they were built at (the noise's own projection on 6000 samples moves it by a few tenths)
    assert np.allclose(R.sisdr(3.0 * p1, s1), R.sisdr(p1, s1), atol=1e-9)          # scale invariant in the prediction
    assert R.sisdr(s1 + 0.5, s1)[0] < 40                                           # no mean removal: an offset is distortion


@pytest.mark.parametrize("name", W.NAMES)
def test_device_cases_are_decided_and_sensitive_to_a_band_edge(name):
    """Two conditions on the INPUTS of tests/test_gpu_wavmetric.py, checked on the oracle alone.  No frame's energy is
    within 1 dB of the 40 dB threshold, so no keep / drop decision is within reach of fp32 rounding.  And the bound the
    device values are held to would notice a wrong band: with the boundary between bands 6 and 7 moved by one bin (34 ->
    33) every value that takes the full path moves by more than 10 x its bound."""
    assert W.min_margin(name) >= 1.0
    edges = list(R.EDGES)
    edges[6], edges[7] = (edges[6][0], edges[6][1] - 1), (edges[7][0] - 1, edges[7][1])
    for ext in (False, True):
        v = W.values(name, ext)
        live = (v != R.SHORT_VALUE) & (v != 0)
        if name in ("10000Hz_1x3967", "16000Hz_33x4500"):
            assert not live.any() and np.all(v == R.SHORT_VALUE)
            continue
        moved = np.abs(R.values(W.spectra(name, 64), ext, edges) - v)
        ratio = moved[live] / W.bound(name, ext)[live]
        print(f"{name} extended={ext}: a misplaced edge moves the values by {moved[live].min():.2e} .. {moved[live].max():.2e}, "
              f"{ratio.min():.1f} x the bound at least")
        assert live.sum() >= v.size - 4 and np.all(ratio > 10)
    if name == "mixed":
        v, k = W.values(name, False), W.kept(name)
        assert k[2, 0] < 30 and np.all(v[2, [0, 2]] == R.SHORT_VALUE) and np.all(v[3, [0, 2]] == 0) and np.all(k[[0, 1, 3]] >= 30)
        assert k[1, 0] == k[3, 0] == 57                                                # no silence / all zero: every frame kept
    if name == "10000Hz_1x3968":
        assert W.kept(name).tolist() == [[30, 30]]


def test_fixture_is_reproduced():
    z = np.load(os.path.join(ROOT, "tests", "golden", "stoi_small.npz"))
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "stoi_small.npz")) < 200_000
    arrays = [z[k] for k in ("s1_pred", "s2_pred", "s1", "s2")]
    assert all(a.dtype == np.float32 and a.shape == (2, 6000) for a in arrays) and int(z["fs"]) == 8000
    spec = R.spectra(*arrays, 8000)
    assert np.array_equal(R.kept(spec), z["kept"]) and np.array_equal(np.array(R.EDGES), z["edges"])
    for ext, key in ((False, "stoi"), (True, "estoi")):
        assert z[key].dtype == np.float64 and np.max(np.abs(R.values(spec, ext) - z[key])) <= 1e-12
    assert np.max(np.abs(R.sisdr_pairs(*arrays) - z["sisdr"])) <= 1e-12 * np.max(np.abs(z["sisdr"]))
    for got, want in zip(W.case("8000Hz_2x6000"), arrays):                             # the device test runs on the same inputs
        assert np.array_equal(got, want)
