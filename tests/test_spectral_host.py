"""Spectral front end, host layer (no GPU needed): the C ABI of include/specfe.h (declared == bound == exported, plain
C99), the argument checks that need no device, the module surface of STFT / LogMelSpectrogram / add_spectrogram_keys /
MSESpecLoss / L1SpecLoss against the reference's signatures, and the oracle tests/spec_ref.py itself: against torch.stft
and torch.istft in fp64, against fp64 autograd through them, against the committed fixture tests/golden/spec_small.npz
(tools/gen_golden_spec.py, the reference's own classes), the two findings about torch.istft the kernels reproduce, the
mel table's structure, and the sensitivity of the bound the device values are held to.

The mel filterbank is checked for its structure only: torchaudio is not a dependency, its parity with
torchaudio.functional.melscale_fbanks is UNPINNED."""
from __future__ import annotations

import ctypes
import inspect
import os
import re
import subprocess
import warnings

import numpy as np
import pytest
import torch

from speech_separation_amd import _lib, spectral
from tests import spec_ref as R
from tests import wavloss_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "specfe.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "spec_small.npz")
SHAPES = [(256, 128, 1, 129), (256, 128, 3, 1000), (400, 200, 2, 1000), (64, 24, 2, 333), (512, 100, 1, 700)]


def _torch_stft(x, N, H):
    a = torch.stft(x, n_fft=N, hop_length=H, window=torch.hann_window(N, dtype=x.dtype), return_complex=True)
    return torch.stack([a.real, a.imag], dim=1).transpose(2, 3)


def _torch_istft(X, N, H, length):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                          # "shorter than the length parameter": the case under test
        return torch.istft(torch.complex(X[:, 0], X[:, 1]).transpose(1, 2), n_fft=N, hop_length=H,
                           window=torch.hann_window(N, dtype=X.dtype), length=length)


def _lengths(M, N, H):
    nat = (M - 1) * H
    return [None, nat - 24, nat + 76 if 76 < N // 2 else nat + N // 4, nat + N // 2 + 10]


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(specfe_\w+)\s*\(", src))
    assert declared == set(_lib.SPECFE_SYMBOLS), declared ^ set(_lib.SPECFE_SYMBOLS)
    m = re.search(r"#define SPECFE_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.SPECFE_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.specfe_abi_version() == 1
    r = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if " T " in ln and ln.split()[-1].startswith("specfe_")}
    assert exported == declared, exported ^ declared
    assert "UNPINNED" in src                                     # the one table without a pinned parity says so


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_bad_arguments_are_refused_before_any_device_call():
    lib = _lib.load()
    assert lib.specfe_strerror(0) == b"ok"
    assert len({lib.specfe_strerror(c) for c in (0, 1, 4, 99)}) == 4
    h = ctypes.c_void_p(0x1234)
    for n_fft, hop in ((16, 8), (528, 128), (250, 100), (256, 129), (256, 0), (256, -1), (0, 0), (-256, 128)):
        assert lib.specfe_create(n_fft, hop, ctypes.byref(h)) == 1 and h.value == 0x1234, (n_fft, hop)
        assert lib.specfe_create_mel(n_fft, hop, 16000, 128, ctypes.byref(h)) == 1 and h.value == 0x1234, (n_fft, hop)
    for sr, n_mels in ((1, 128), (0, 128), (16000, 0), (16000, 257), (-16000, 128)):
        assert lib.specfe_create_mel(400, 200, sr, n_mels, ctypes.byref(h)) == 1 and h.value == 0x1234, (sr, n_mels)
    assert lib.specfe_create(256, 128, None) == 1 and lib.specfe_create_mel(400, 200, 16000, 128, None) == 1
    buf = np.full(64, 7.0, dtype=np.float64)
    p = buf.ctypes.data
    for fn in (lib.specfe_stft, lib.specfe_stft_backward, lib.specfe_logmel):
        assert fn(None, p, 1, 1000, p, None) == 1
    for fn in (lib.specfe_istft, lib.specfe_istft_backward):
        assert fn(None, p, 1, 9, 0, p, None) == 1
    assert np.all(buf == 7.0)
    lib.specfe_destroy(None)                                     # a no-op


def test_module_surface_and_reference_signatures():
    import speech_separation_amd as S
    from speech_separation_amd.metrics import L1SpecLoss, MAEWavLoss, MSESpecLoss, MSEWavLoss
    for name in ("STFT", "LogMelSpectrogram", "add_spectrogram_keys"):
        assert name in S.__all__ and getattr(S, name) is getattr(spectral, name)
    for cls in (MSESpecLoss, L1SpecLoss):
        assert cls.__name__ in S.__all__ and getattr(S, cls.__name__) is cls
    # src/encoders/stft.py: STFT(n_fft: int = 256, hop_length: int = 128), .stft(mix_audio), attributes n_fft / hop_length / window
    sig = inspect.signature(spectral.STFT.__init__).parameters
    assert list(sig) == ["self", "n_fft", "hop_length"] and (sig["n_fft"].default, sig["hop_length"].default) == (256, 128)
    assert list(inspect.signature(spectral.STFT.stft).parameters) == ["self", "mix_audio"]
    assert list(inspect.signature(spectral.STFT.istft).parameters) == ["self", "spec", "length"]
    e = spectral.STFT()
    assert (e.n_fft, e.hop_length) == (256, 128) and torch.equal(e.window, torch.hann_window(256))
    # torchaudio's MelSpectrogram(sample_rate=16000) defaults (base_dataset.py get_spectrogram)
    m = spectral.LogMelSpectrogram()
    assert (m.sample_rate, m.n_fft, m.hop_length, m.n_mels) == (16000, 400, 200, 128)
    for bad in ((250, 100), (256, 129), (16, 8), (1024, 256), (256, 0)):
        with pytest.raises(ValueError, match="multiple of 16"):
            spectral.STFT(*bad)
    with pytest.raises(ValueError, match="n_mels"):
        spectral.LogMelSpectrogram(n_mels=0)
    # src/loss/ss_losses.py:29-62
    for cls, base, kind in ((MSESpecLoss, MSEWavLoss, "mse"), (L1SpecLoss, MAEWavLoss, "mae")):
        assert list(inspect.signature(cls.forward).parameters) == ["self", "s1_spec_pred", "s2_spec_pred", "s1_spec_true",
                                                                   "s2_spec_true", "batch"]
        assert cls.kind == base.kind == kind and cls().pit == "batch" and cls(pit="utterance").pit == "utterance"
        with pytest.raises(ValueError, match="pit"):
            cls(pit="item")
        z = torch.zeros(2, 9, 7)
        with pytest.raises(RuntimeError, match="no CPU path"):
            cls()(s1_spec_pred=z, s2_spec_pred=z, s1_spec_true=z, s2_spec_true=z, mix=None)
        with pytest.raises(ValueError, match=r"\(2, 9, 6\).*\(2, 9, 7\)"):
            cls()(s1_spec_pred=z, s2_spec_pred=z, s1_spec_true=z[:, :, :6], s2_spec_true=z)
    # no CPU path anywhere: the same kind of error as the models raise
    x = torch.zeros(2, 1000)
    for call in (lambda: e.stft(x), lambda: e.istft(torch.zeros(2, 2, 8, 129)), lambda: m(x),
                 lambda: spectral.add_spectrogram_keys({"mix": x})):
        with pytest.raises(RuntimeError, match="no CPU/PyTorch fallback"):
            call()
    assert spectral.add_spectrogram_keys({"mix": None, "s1": None}) == {"mix": None, "s1": None}      # nothing to fill


@pytest.mark.parametrize("N,H,B,T", SHAPES)
def test_oracle_equals_torch_stft_and_istft_and_their_autograd(N, H, B, T):
    g = torch.Generator().manual_seed(N + T)
    x = torch.randn(B, T, dtype=torch.float64, generator=g, requires_grad=True)
    want = _torch_stft(x, N, H)
    M = 1 + T // H
    assert want.shape == (B, 2, M, N // 2 + 1)
    scale = float(want.detach().abs().max())
    assert float((R.stft(x.detach(), N, H) - want.detach()).abs().max()) <= 1e-13 * scale
    gX = torch.randn(want.shape, dtype=torch.float64, generator=g)
    gx, = torch.autograd.grad(want, x, gX)
    assert float((R.stft_backward(gX, T, N, H) - gx).abs().max()) <= 1e-13 * float(gx.abs().max())
    for length in _lengths(M, N, H):
        X = torch.randn(B, 2, M, N // 2 + 1, dtype=torch.float64, generator=g, requires_grad=True)
        y = _torch_istft(X, N, H, length)
        got = R.istft(X.detach(), N, H, length)
        assert got.shape == y.shape and float((got - y).abs().max()) <= 1e-12 * float(y.abs().max()), length
        gy = torch.randn(y.shape, dtype=torch.float64, generator=g)
        gXi, = torch.autograd.grad(y, X, gy)
        assert float((R.istft_backward(gy, M, N, H) - gXi).abs().max()) <= 1e-12 * float(gXi.abs().max()), length
        assert float(gXi[:, 1, :, 0].abs().max()) == 0 and float(gXi[:, 1, :, -1].abs().max()) == 0
    # round trip: the inverse of the transform of a signal is the signal
    assert float((R.istft(R.stft(x.detach(), N, H), N, H, T)[:, :(M - 1) * H] - x.detach()[:, :(M - 1) * H]).abs().max()) <= 1e-12


def test_findings_about_torch_istft():
    """Im of bins 0 and N / 2 is ignored exactly, and a length beyond the natural one reads into the last half window."""
    g = torch.Generator().manual_seed(5)
    N, H, M = 256, 128, 9
    X = torch.randn(2, 2, M, N // 2 + 1, dtype=torch.float64, generator=g)
    Z = X.clone()
    Z[:, 1, :, 0] = 0
    Z[:, 1, :, -1] = 0
    nat = (M - 1) * H
    for length in (None, nat + 76):
        assert torch.equal(_torch_istft(X, N, H, length), _torch_istft(Z, N, H, length))
        assert torch.equal(R.istft(X, N, H, length), R.istft(Z, N, H, length))
    y = _torch_istft(X, N, H, nat + N // 2 + 10)
    assert float(y[:, nat:nat + N // 2].abs().min()) > 0 and float(y[:, nat + N // 2:].abs().max()) == 0
    assert float((R.istft(X, N, H, nat + N // 2 + 10) - y).abs().max()) <= 1e-12 * float(y.abs().max())


def test_fixture_is_reproduced():
    """tests/golden/spec_small.npz: what the reference's own classes gave (tools/gen_golden_spec.py)."""
    assert os.path.getsize(GOLDEN) < 200_000
    z = np.load(GOLDEN)
    x = torch.from_numpy(z["x"])
    assert z["stft64"].shape == (1, 2, 8, 129) and z["stft32"].dtype == np.float32
    got = R.stft(x, 256, 128)
    assert float((got - torch.from_numpy(z["stft64"])).abs().max()) <= 1e-12
    bound = R.stft_bound(x, 256, 128)[:, None, :, None]
    assert bool(((got - torch.from_numpy(z["stft32"]).double()).abs() <= bound).all())       # the reference's fp32 FFT, far inside
    assert float((R.stft(torch.from_numpy(z["x24"]), 64, 24) - torch.from_numpy(z["stft64_n64_h24"])).abs().max()) <= 1e-12
    X = torch.from_numpy(z["X"])
    assert float(X[:, 1, :, 0].abs().min()) > 0 and float(X[:, 1, :, -1].abs().min()) > 0
    for length in (1000, 1100):
        want = torch.from_numpy(z[f"istft{length}_64"])
        assert float((R.istft(X, 256, 128, length) - want).abs().max()) <= 1e-12 * float(want.abs().max())
    assert float(np.abs(z["istft1100_64"][:, 1024:]).min()) > 0                              # beyond the natural length: not zero
    # the spec losses are the waveform criteria on the [B, F T] view
    arrays = [z["spec." + k].reshape(3, -1) for k in ("p1", "p2", "s1", "s2")]
    for name, kind in (("mse", "mse"), ("l1", "mae")):
        for perm in (0, 1):
            a = [arrays[1], arrays[0], arrays[2], arrays[3]] if perm else arrays
            o = wavloss_ref.evaluate(kind, "batch", *a)
            assert int(o["perm"][0]) == int(z[f"{name}.{perm}.perm"]) == perm
            assert abs(float(o["loss"]) - float(z[f"{name}.{perm}.loss64"])) <= 1e-14
            assert abs(float(z[f"{name}.{perm}.loss32"]) - float(z[f"{name}.{perm}.loss64"])) <= 1e-6 * float(z[f"{name}.{perm}.loss64"])
            for k in ("d1", "d2"):
                assert np.max(np.abs(o[k].reshape(3, 9, 7) - z[f"{name}.{perm}.{k}_64"])) <= 1e-16


def test_mel_table_structure():
    """HTK triangles: non-negative, at most 1, each band one run of bins, and between the centres of the first and the last
    band the triangles sum to 1.  (Structure only: parity with torchaudio is unpinned.)"""
    for sr, N, n_mels in ((16000, 400, 128), (16000, 512, 40), (8000, 256, 64)):
        fb = R.mel_filterbank(sr, N, n_mels)
        F = N // 2 + 1
        assert fb.shape == (F, n_mels) and fb.min() >= 0 and fb.max() <= 1
        top = 2595.0 * np.log10(1.0 + sr / 2 / 700.0)
        f_pts = 700.0 * (10.0 ** (np.arange(n_mels + 2) * top / (n_mels + 1) / 2595.0) - 1.0)
        freqs = np.arange(F) * (sr / 2) / (F - 1)
        inside = (freqs >= f_pts[1]) & (freqs <= f_pts[-2])
        assert np.max(np.abs(fb[inside].sum(1) - 1)) <= 1e-12
        for j in range(n_mels):
            nz = np.flatnonzero(fb[:, j])
            assert nz.size == 0 or (np.all(np.diff(nz) == 1) and f_pts[j] < freqs[nz[0]] and freqs[nz[-1]] < f_pts[j + 2])
    assert R.logmel(torch.zeros(1, 1000)).unique().tolist() == [np.log(1e-5)]


def test_bound_is_loose_for_fp32_and_tight_for_mistakes():
    """The fp32 matrix-product restatement sits far inside the bound; a symmetric window in place of the periodic one, or one
    dropped term, is far outside it."""
    g = torch.Generator().manual_seed(9)
    for N, H, T in ((256, 128, 4099), (400, 200, 2000), (64, 24, 333)):
        x = torch.randn(3, T, generator=g) * torch.tensor([[1.0], [1e-3], [30.0]])
        want, bound = R.stft(x, N, H), R.stft_bound(x, N, H)[:, None, :, None]
        ratio = float(((R.stft(x, N, H, torch.float32).double() - want).abs() / bound).max())
        print(f"stft fp32 restatement ({N}, {H}): worst error / bound {ratio:.4f}")
        assert ratio < 0.1
        w, c, s = R.tables(N)
        fr = R.frames(x.double(), N, H)
        sym = 0.5 - 0.5 * torch.cos(2 * torch.pi * torch.arange(N, dtype=torch.float64) / (N - 1))
        wrong = torch.stack([(fr * sym) @ c, -((fr * sym) @ s)], dim=1)
        assert float(((wrong - want).abs() / bound).max()) > 10
        cut = fr * w
        cut[:, :, N // 3] = 0                                    # one term dropped from every dot product
        wrong = torch.stack([cut @ c, -(cut @ s)], dim=1)
        assert float(((wrong - want).abs() / bound).max()) > 100
