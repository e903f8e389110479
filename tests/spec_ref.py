"""TEST INFRASTRUCTURE: the five maps of include/specfe.h restated as matrix products in stock PyTorch, at any float dtype
(fp64: the oracle of tests/test_gpu_spectral.py; fp32: the "fp32 restatement" whose own distance from fp64 that test
prints next to the kernel's), the mel filterbank, and the forward-error bounds the kernels are held to.

tests/test_spectral_host.py pins this file: stft / istft against torch.stft / torch.istft in fp64, the two adjoints
against fp64 autograd through them, everything against tests/golden/spec_small.npz (tools/gen_golden_spec.py, the
reference's own classes).  The mel table follows torchaudio's documented defaults (HTK scale, no norm); torchaudio is
not a dependency, so its parity with torchaudio.functional.melscale_fbanks is UNPINNED.

Bounds (u = 2^-24, gamma(n) = n u / (1 - n u), the forward error of an n-term fp32 dot product summed in any order):
  stft            |hip - fp64| <= gamma(N + 3) sum_t |w[t] xp[m H + t]|   per element of frame m; N products and additions,
                  3 = rounded window entry, rounded table entry, the product w x
  istft           |dy[n]| <= gamma(N + ceil(N / H) + 6) sum_m |w[n - m H]| (1 / N) sum_k c_k (|Re X| + |Im X|) / env[n]
  stft_backward   the istft form without 1 / N and env: gamma(N + ceil(N / H) + 6) applied to the adjoint of |gX|
                  (overlap-add of |w| sum_k (|gRe| + |gIm|), then the reflect fold)
  istft_backward  the stft form on the enveloped gradient: gamma(N + 8) (c_k / N) sum_t |w[t] gy[m H + t - N / 2] / env|;
                  8 = the 3 of stft + the window's rounding inside env (2) + the division by env + the rounded c_k / N
                  and the product with it
  logmel          the stft bound d propagated: dP <= 2 |X| d + d^2, the non-negative filterbank sum adds gamma(F + 2) of
                  itself, then |log max(a, c) - log max(b, c)| <= |a - b| / max(min(a, b), c), plus 4 u |log| for the
                  fp32 result of logf and the rounded clamp constant (all that is left on a silent frame)
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

U = 2.0 ** -24
CLAMP = 1e-5


def gamma(n):
    return n * U / (1 - n * U)


@functools.lru_cache(maxsize=None)
def tables(N, dtype=torch.float64):
    """-> window [N], cos [N][F], sin [N][F] of 2 pi k t / N: computed in double (the angle reduced in integers), rounded once."""
    t = np.arange(N)
    k = np.arange(N // 2 + 1)
    ang = 2 * np.pi * ((t[:, None] * k[None, :]) % N) / N
    w = 0.5 - 0.5 * np.cos(2 * np.pi * t / N)
    return tuple(torch.from_numpy(a).to(dtype) for a in (w, np.cos(ang), np.sin(ang)))


def reflect_index(T, N):
    """Index into x of every sample of the padded signal, [T + N]."""
    j = np.abs(np.arange(-(N // 2), T + N // 2))
    j = np.where(j >= T, 2 * (T - 1) - j, j)
    assert T > N // 2 and j.min() >= 0 and j.max() < T
    return torch.from_numpy(j)


def frames(x, N, H):
    """x [B][T] -> the M = 1 + T // H frames of the reflect-padded signal, [B][M][N] (not windowed)."""
    T = x.shape[1]
    return x[:, reflect_index(T, N)].unfold(1, N, H)[:, :1 + T // H]


def stft(x, N, H, dtype=torch.float64):
    w, c, s = tables(N, dtype)
    a = frames(torch.as_tensor(x).to(dtype), N, H) * w
    return torch.stack([a @ c, -(a @ s)], dim=1)


def _ck(N, dtype):
    ck = torch.full((N // 2 + 1,), 2.0, dtype=dtype)
    ck[0] = ck[-1] = 1.0
    return ck


def overlap_add(fr, H):
    """fr [B][M][N] -> [B][(M - 1) H + N]"""
    B, M, N = fr.shape
    z = torch.zeros(B, (M - 1) * H + N, dtype=fr.dtype)
    for m in range(M):
        z[:, m * H:m * H + N] += fr[:, m]
    return z


def envelope(N, H, M, dtype=torch.float64):
    w = tables(N, dtype)[0]
    return overlap_add((w * w).expand(1, M, N), H)[0]


def out_length(M, H, length):
    return (M - 1) * H if length is None or length <= 0 else int(length)


def _cut(z, env, N, L):
    """y[j] = z[N / 2 + j] / env[N / 2 + j] for j < L where a frame reaches, 0 beyond"""
    y = torch.zeros(z.shape[0], L, dtype=z.dtype)
    n = min(L, z.shape[1] - N // 2)
    y[:, :n] = z[:, N // 2:N // 2 + n] / env[N // 2:N // 2 + n]
    return y


def istft(X, N, H, length=None, dtype=torch.float64):
    w, c, s = tables(N, dtype)
    X = torch.as_tensor(X).to(dtype)
    ck, ci = _ck(N, dtype), _ck(N, dtype)
    ci[0] = ci[-1] = 0.0                                        # Im of bins 0 and N / 2 does not enter
    r = ((X[:, 0] * ck) @ c.T - (X[:, 1] * ci) @ s.T) / N
    M = X.shape[2]
    return _cut(overlap_add(r * w, H), envelope(N, H, M, dtype), N, out_length(M, H, length))


def stft_backward(gX, T, N, H, dtype=torch.float64):
    w, c, s = tables(N, dtype)
    gX = torch.as_tensor(gX).to(dtype)
    gp = overlap_add((gX[:, 0] @ c.T - gX[:, 1] @ s.T) * w, H)
    gx = torch.zeros(gX.shape[0], T, dtype=dtype)
    return gx.index_add_(1, reflect_index(T, N)[:gp.shape[1]], gp)


def _enveloped(gy, M, N, H, dtype):
    """gy [B][L] -> gz [B][(M - 1) H + N]: gy / env at n = N / 2 + j, 0 elsewhere"""
    env = envelope(N, H, M, dtype)
    gz = torch.zeros(gy.shape[0], env.shape[0], dtype=dtype)
    n = min(gy.shape[1], env.shape[0] - N // 2)
    gz[:, N // 2:N // 2 + n] = gy[:, :n] / env[N // 2:N // 2 + n]
    return gz


def istft_backward(gy, M, N, H, dtype=torch.float64):
    w, c, s = tables(N, dtype)
    gr = _enveloped(torch.as_tensor(gy).to(dtype), M, N, H, dtype).unfold(1, N, H) * w
    ck, ci = _ck(N, dtype) / N, _ck(N, dtype) / N
    ci[0] = ci[-1] = 0.0
    return torch.stack([(gr @ c) * ck, -(gr @ s) * ci], dim=1)


@functools.lru_cache(maxsize=None)
def mel_filterbank(sample_rate=16000, n_fft=400, n_mels=128):
    """[F][n_mels] fp64: HTK mel scale, f_min 0, f_max sample_rate / 2, no norm (torchaudio's MelSpectrogram defaults)."""
    F = n_fft // 2 + 1
    freqs = np.linspace(0.0, sample_rate / 2, F)
    m_pts = np.linspace(0.0, 2595.0 * np.log10(1.0 + (sample_rate / 2) / 700.0), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    slopes = f_pts[None, :] - freqs[:, None]
    down = -slopes[:, :-2] / np.diff(f_pts)[:-1]
    up = slopes[:, 2:] / np.diff(f_pts)[1:]
    return np.maximum(0.0, np.minimum(down, up))


def logmel(x, sample_rate=16000, N=400, H=200, n_mels=128, dtype=torch.float64):
    X = stft(x, N, H, dtype)
    fb = torch.from_numpy(mel_filterbank(sample_rate, N, n_mels)).to(dtype)
    return torch.log(torch.clamp((X[:, 0] ** 2 + X[:, 1] ** 2) @ fb, min=CLAMP)).transpose(1, 2)


# ---- bounds (module docstring), all in fp64 from the fp64 quantities ----

def stft_bound(x, N, H):
    """-> [B][M]: the bound of every element of frame m"""
    w = tables(N)[0]
    return gamma(N + 3) * (frames(torch.as_tensor(x).double(), N, H) * w).abs().sum(-1)


def istft_bound(X, N, H, length=None):
    X = torch.as_tensor(X).double()
    w = tables(N)[0]
    M = X.shape[2]
    a = ((X[:, 0].abs() + X[:, 1].abs()) * _ck(N, torch.float64)).sum(-1) / N                # [B][M]
    z = overlap_add(a[:, :, None] * w.abs(), H)
    return gamma(N + math.ceil(N / H) + 6) * _cut(z, envelope(N, H, M), N, out_length(M, H, length))


def stft_backward_bound(gX, T, N, H):
    gX = torch.as_tensor(gX).double()
    w = tables(N)[0]
    a = (gX[:, 0].abs() + gX[:, 1].abs()).sum(-1)
    gp = overlap_add(a[:, :, None] * w.abs(), H)
    gx = torch.zeros(gX.shape[0], T, dtype=torch.float64)
    return gamma(N + math.ceil(N / H) + 6) * gx.index_add_(1, reflect_index(T, N)[:gp.shape[1]], gp)


def istft_backward_bound(gy, M, N, H):
    """-> [B][M][F] (the same for Re and Im)"""
    w = tables(N)[0]
    s = (_enveloped(torch.as_tensor(gy).double(), M, N, H, torch.float64).unfold(1, N, H) * w).abs().sum(-1)
    return gamma(N + 8) * s[:, :, None] * (_ck(N, torch.float64) / N)


def logmel_bound(x, sample_rate=16000, N=400, H=200, n_mels=128):
    """-> [B][n_mels][M]"""
    X = stft(x, N, H)
    d = stft_bound(x, N, H)[:, :, None]
    mag = torch.sqrt(X[:, 0] ** 2 + X[:, 1] ** 2)
    P = mag ** 2
    dP = 2 * mag * d + d * d
    fb = torch.from_numpy(mel_filterbank(sample_rate, N, n_mels))
    a = P @ fb
    err = dP @ fb + gamma(N // 2 + 3) * ((P + dP) @ fb)
    val = torch.log(torch.clamp(a, min=CLAMP))
    return (err / torch.clamp(a - err, min=CLAMP) + 4 * U * val.abs()).transpose(1, 2)
