"""TEST ORACLE: STOI / ESTOI (Taal et al. 2011, Jensen & Taal 2016) and SI-SDR restated in numpy, at a chosen precision.

pystoi and torchmetrics are not dependencies of this project, so THIS FILE IS THE DEFINITION the HIP kernels of
include/wavmetric.h are held to.  It follows pystoi's algorithm; where pystoi releases differ the
choice is fixed here:
  * frames start at 0, 128, ... <= len - 256, in the silent-frame removal AND in the STFT: the last full frame is included;
  * resampling is the polyphase FIR of `resample_design` (what scipy.signal.resample_poly does with that window), not
    an external resampler;
  * EPS is the double epsilon 2^-52 at every precision.
`dtype=np.float64` may use np.fft.rfft; with `dtype=np.float32` every array is fp32 and the DFT is a matrix product with
twiddles rounded once from double -- the same arithmetic the device does, in another summation order.
"""
from __future__ import annotations

import math

import numpy as np

FS = 10000
N_FRAME = 256
HOP = 128
NFFT = 512
NUM_BANDS = 15
MIN_FREQ = 150.0
N_SEG = 30
BETA = -15.0
DYN_RANGE = 40.0
EPS = 2.0 ** -52
SHORT_VALUE = 1e-5          # pystoi's "not enough frames" value
SDR_EPS = float(np.finfo(np.float32).eps)


def third_octave_edges(fs=FS, nfft=NFFT, num_bands=NUM_BANDS, min_freq=MIN_FREQ):
    """Bins [lo, hi) of every band by pystoi's rule: the bin nearest (argmin of the squared distance) to each band's
    lower and upper edge frequency."""
    f = np.linspace(0, fs, nfft + 1)[:nfft // 2 + 1]
    k = np.arange(num_bands, dtype=np.float64)
    lo_f = min_freq * 2.0 ** ((2 * k - 1) / 6)
    hi_f = min_freq * 2.0 ** ((2 * k + 1) / 6)
    return [(int(np.argmin((f - a) ** 2)), int(np.argmin((f - b) ** 2))) for a, b in zip(lo_f, hi_f)]


EDGES = third_octave_edges()
BIN_LO, BIN_HI = EDGES[0][0], EDGES[-1][1]          # the bins any band reads


def resample_design(fs):
    """(p, q, L, g): fs -> 10 kHz as p / q in lowest terms, half length L and the 2 L + 1 taps g (double)."""
    d = math.gcd(FS, int(fs))
    p, q = FS // d, int(fs) // d
    fc = 1.0 / (2 * max(p, q))
    L = int(math.ceil(52.0 / (28.714 * fc / 10.0)))
    t = np.arange(-L, L + 1, dtype=np.float64)
    h = np.kaiser(2 * L + 1, 0.1102 * 51.3) * 2 * p * fc * np.sinc(2 * fc * t)
    return p, q, L, p * h / h.sum()


def resample(x, fs, dtype=np.float64):
    """y[m] = sum_j g[L + m q - j p] x[j], m < ceil(T p / q); the identity at fs = 10000."""
    x = np.asarray(x, dtype=dtype)
    if int(fs) == FS:
        return x.copy()
    p, q, L, g = resample_design(fs)
    g = g.astype(dtype)
    T = x.shape[0]
    n_out = -(-T * p // q)
    m = np.arange(n_out)
    top = L + m * q                       # tap index of x[0]'s neighbour: k = top - j p
    phase, jmax = top % p, top // p
    y = np.zeros(n_out, dtype=dtype)
    for r in range(p):
        c = np.convolve(x, g[r::p])       # c[n] = sum_i g[r + i p] x[n - i]
        sel = phase == r
        idx = jmax[sel]
        ok = idx < c.shape[0]
        vals = np.zeros(idx.shape[0], dtype=dtype)
        vals[ok] = c[idx[ok]]
        y[sel] = vals
    return y


def window(dtype=np.float64):
    return np.hanning(N_FRAME + 2)[1:-1].astype(dtype)


def _frames(x):
    n = (x.shape[0] - N_FRAME) // HOP + 1 if x.shape[0] >= N_FRAME else 0
    idx = HOP * np.arange(n)[:, None] + np.arange(N_FRAME)[None, :]
    return x[idx] if n else np.zeros((0, N_FRAME), dtype=x.dtype)


def remove_silent_frames(x, ys, dtype=np.float64):
    """The clean signal x decides: -> (compacted x, [compacted y ...], number of kept frames, every frame's margin
    e_k - (max e - 40) in dB as float64)."""
    w = window(dtype)
    xf = _frames(x) * w
    if xf.shape[0] == 0:
        z = np.zeros(0, dtype=dtype)
        return z, [z for _ in ys], 0, np.zeros(0)
    e = (20 * np.log10(np.sqrt(np.sum(xf * xf, axis=1, dtype=dtype)) + dtype(EPS))).astype(dtype)
    margin = e - (e.max() - dtype(DYN_RANGE))
    keep = margin > 0
    nk = int(keep.sum())

    def ola(frames):
        out = np.zeros((nk - 1) * HOP + N_FRAME, dtype=dtype)
        for i, f in enumerate(frames[keep]):
            out[i * HOP:i * HOP + N_FRAME] += f
        return out

    return ola(xf), [ola(_frames(y) * w) for y in ys], nk, margin.astype(np.float64)


_TWIDDLES = {}


def _twiddles(dtype):
    if dtype not in _TWIDDLES:
        ang = 2 * np.pi * np.outer(np.arange(N_FRAME), np.arange(BIN_LO, BIN_HI)) / NFFT
        _TWIDDLES[dtype] = (np.cos(ang).astype(dtype), np.sin(ang).astype(dtype))
    return _TWIDDLES[dtype]


def power_spectrum(z, dtype=np.float64):
    """|STFT|^2 of the bins BIN_LO .. BIN_HI - 1, [frames, bins]."""
    zf = _frames(z) * window(dtype)
    if dtype == np.float64:
        s = np.fft.rfft(zf, NFFT, axis=1)[:, BIN_LO:BIN_HI]
        return s.real ** 2 + s.imag ** 2
    c, s = _twiddles(dtype)
    re, im = zf @ c, zf @ s
    return re * re + im * im


def band_spectrum(pw, edges=None):
    edges = EDGES if edges is None else edges
    return np.stack([np.sqrt(np.sum(pw[:, lo - BIN_LO:hi - BIN_LO], axis=1, dtype=pw.dtype)) for lo, hi in edges], axis=1)


def _segments(X):
    return np.lib.stride_tricks.sliding_window_view(X, N_SEG, axis=0)      # [J, bands, 30]


def _norm(a, axis):
    return np.sqrt(np.sum(a * a, axis=axis, keepdims=True, dtype=a.dtype))


def stoi_from_bands(X, Y, extended):
    """X, Y [frames, 15] band spectra of the clean and the processed signal -> the measure (a Python float)."""
    dt = X.dtype.type
    if X.shape[0] < N_SEG:
        return SHORT_VALUE
    xs, ys = _segments(X), _segments(Y)
    J = xs.shape[0]
    eps = dt(EPS)
    if not extended:
        c = _norm(xs, 2) / (_norm(ys, 2) + eps)
        yp = np.minimum(ys * c, xs * dt(1 + 10 ** (-BETA / 20)))
        yp = yp - np.mean(yp, axis=2, keepdims=True, dtype=dt)
        xc = xs - np.mean(xs, axis=2, keepdims=True, dtype=dt)
        yp = yp / (_norm(yp, 2) + eps)
        xc = xc / (_norm(xc, 2) + eps)
        return float(np.sum(xc * yp, dtype=dt) / dt(J * NUM_BANDS))

    def row_col(a):
        a = a - np.mean(a, axis=2, keepdims=True, dtype=dt)
        a = a / (_norm(a, 2) + eps)
        a = a - np.mean(a, axis=1, keepdims=True, dtype=dt)
        return a / (_norm(a, 1) + eps)

    return float(np.sum(row_col(xs) * row_col(ys), dtype=dt) / dt(N_SEG) / dt(J))


def spectra(s1_pred, s2_pred, s1, s2, fs, dtype=np.float64):
    """Everything up to the power spectra, for a batch [B, T]: per item and target j a dict
    {"kept", "margin", "pw": [clean, prediction 1, prediction 2]} (6 spectra per item)."""
    out = []
    for b in range(np.shape(s1)[0]):
        r = [resample(a[b], fs, dtype) for a in (s1_pred, s2_pred, s1, s2)]
        item = []
        for j in range(2):
            x, ys, nk, margin = remove_silent_frames(r[2 + j], r[:2], dtype)
            item.append({"kept": nk, "margin": margin, "pw": [power_spectrum(z, dtype) for z in [x] + ys]})
        out.append(item)
    return out


def values(spec, extended, edges=None):
    """[B, 4] float64: the measure of the pairs (p1,s1) (p1,s2) (p2,s1) (p2,s2) from `spectra`'s result."""
    out = np.zeros((len(spec), 4))
    for b, item in enumerate(spec):
        for j in range(2):
            X = band_spectrum(item[j]["pw"][0], edges)
            for i in range(2):
                out[b, 2 * i + j] = stoi_from_bands(X, band_spectrum(item[j]["pw"][1 + i], edges), extended)
    return out


def kept(spec):
    return np.array([[item[0]["kept"], item[1]["kept"]] for item in spec], dtype=np.int32)


def stoi(clean, est, fs, extended=False, dtype=np.float64):
    """One (clean, estimate) pair -> (value, kept frames, every frame's margin in dB)."""
    x, y = resample(clean, fs, dtype), resample(est, fs, dtype)
    xc, (yc,), nk, margin = remove_silent_frames(x, [y], dtype)
    v = stoi_from_bands(band_spectrum(power_spectrum(xc, dtype)), band_spectrum(power_spectrum(yc, dtype)), extended)
    return v, nk, margin


def sisdr(p, t, dtype=np.float64):
    """torchmetrics' ScaleInvariantSignalDistortionRatio() default (zero_mean=False) on rows of [.., T]."""
    p, t = np.asarray(p, dtype=dtype), np.asarray(t, dtype=dtype)
    eps = dtype(SDR_EPS)
    a = (np.sum(p * t, axis=-1, keepdims=True, dtype=dtype) + eps) / (np.sum(t * t, axis=-1, keepdims=True, dtype=dtype) + eps)
    ts = a * t
    noise = ts - p
    return (10 * np.log10((np.sum(ts * ts, axis=-1, dtype=dtype) + eps) / (np.sum(noise * noise, axis=-1, dtype=dtype) + eps))).astype(np.float64)


def sisdr_pairs(s1_pred, s2_pred, s1, s2, dtype=np.float64):
    return np.stack([sisdr(s1_pred, s1, dtype), sisdr(s1_pred, s2, dtype), sisdr(s2_pred, s1, dtype), sisdr(s2_pred, s2, dtype)], axis=1)


def pit(vals):
    """SS2BaseMetric.forward on [B, 4] pair values: batch means, then max((m11 + m22) / 2, (m12 + m21) / 2)."""
    m = np.asarray(vals, dtype=np.float64).mean(0)
    return max((m[0] + m[3]) / 2, (m[1] + m[2]) / 2)


# ------------------------------------------------------------------------------------------------ test signals
def gated_harmonic(T, fs, seed, kind="gaps"):
    """Amplitude-gated harmonic signal + a 1e-4 noise floor, fp32 [T].  The gate switches on a grid of 128 samples at
    10 kHz (raised-cosine ramps of 1 ms inside the active side), so that a frame is either fully silent or at least half
    active: no frame's energy sits near the 40 dB threshold.
    kind: "gaps" active runs of 6..14 grid units, silent runs of 2..4;  "full" no silence;  "short" one active run of 20
    units (fewer than 30 kept frames);  "zero" all zeros, no noise floor."""
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(T, dtype=np.float32)
    t = np.arange(T) / fs
    f0 = rng.uniform(110.0, 220.0)
    top = 0.45 * min(fs, FS)
    x = np.zeros(T)
    for k in range(1, int(top / f0) + 1):         # every harmonic has its own slow amplitude modulation: no band is stationary
        am = 1 + 0.6 * np.sin(2 * np.pi * rng.uniform(1.0, 5.0) * t + rng.uniform(0, 2 * np.pi))
        x += am * np.sin(2 * np.pi * k * f0 * t + rng.uniform(0, 2 * np.pi)) / k
    x *= 0.3 * (0.6 + 0.4 * np.sin(2 * np.pi * rng.uniform(3.0, 6.0) * t + rng.uniform(0, 2 * np.pi)))
    units = int(np.ceil(T / fs * FS / HOP)) + 1
    g = np.ones(units)
    if kind == "gaps":
        u = int(rng.integers(3, 8))
        while u < units:
            n = int(rng.integers(2, 5))
            g[u:u + n] = 0
            u += n + int(rng.integers(6, 15))
    elif kind == "short":
        g[:] = 0
        g[4:24] = 1
    elif kind != "full":
        raise ValueError(kind)
    gate = g[np.minimum((t * FS / HOP).astype(np.int64), units - 1)]
    ramp = max(int(fs / 1000), 1)
    k = np.convolve(gate, np.hanning(2 * ramp + 1) / np.hanning(2 * ramp + 1).sum(), mode="same")
    gate = np.minimum(gate, k * gate)     # ramps on the active side only
    return (x * gate + 1e-4 * rng.standard_normal(T)).astype(np.float32)


def add_noise(s, snr_db, seed):
    """s + white noise at `snr_db` over the whole signal (a silent s gets noise of 0.1 RMS), fp32."""
    rng = np.random.default_rng(seed)
    n = rng.standard_normal(s.shape[0])
    ps = float(np.mean(s.astype(np.float64) ** 2))
    scale = math.sqrt(ps / 10 ** (snr_db / 10)) if ps > 0 else 0.1
    return (s.astype(np.float64) + scale * n).astype(np.float32)


def make_batch(fs, B, T, seed, kinds=None, kinds2=None):
    """(s1_pred, s2_pred, s1, s2) fp32 [B, T]: independent gated targets, s1_pred = s1 + noise at 5 dB, s2_pred = s2 +
    noise at -5 dB.  `kinds` / `kinds2`: the first / second target's kind per item (default "gaps")."""
    kinds, kinds2 = kinds or ["gaps"] * B, kinds2 or ["gaps"] * B
    s1 = np.stack([gated_harmonic(T, fs, seed * 1000 + 4 * b, kinds[b]) for b in range(B)])
    s2 = np.stack([gated_harmonic(T, fs, seed * 1000 + 4 * b + 1, kinds2[b]) for b in range(B)])
    p1 = np.stack([add_noise(s1[b], 5.0, seed * 1000 + 4 * b + 2) for b in range(B)])
    p2 = np.stack([add_noise(s2[b], -5.0, seed * 1000 + 4 * b + 3) for b in range(B)])
    return p1, p2, s1, s2
