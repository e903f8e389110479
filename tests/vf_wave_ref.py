"""TEST INFRASTRUCTURE: the two maps of include/vfwave.h restated in stock PyTorch on tests/spec_ref.py's maps, at any
float dtype (fp64: the oracle of tests/test_gpu_vf_wave.py), the inputs both test files share, and the forward-error
bounds the kernels are held to.  tests/test_vf_wave_host.py pins this file against torch.stft / torch.abs / torch.angle /
torch.istft in fp64 and against tests/golden/vf_wave_small.npz (tools/gen_golden_vf_wave.py: the reference's own
get_magnitude).

Definitions, with S = spec_ref.stft (one-sided Hann STFT, n_fft = N, hop = H, F = N / 2 + 1, W = 1 + T // H):
  analysis   spec[b][f][w]   = clamp((20 log10(max(|S|, 1e-5)) - 20) / 100, -1, 0) + 1
             phasor[b][:][f][w] = (Re S, Im S) / |S|, (1, 0) where |S| == 0
  synthesis  mag = 10^(5 clamp(p, 0, 1) - 4), X = mag (phasor[0] + i phasor[1]), y = spec_ref.istft(X, length)
The analysis keeps |S| only inside [1e-4, 10] (the reference's convention): synthesis(analysis(x)) is not x.

Bounds (u = 2^-24, gamma(n) = n u / (1 - n u) as in spec_ref):
  spec       the rule of tests/test_gpu_voicefilter.py::test_magnitude_on_the_device, restated.  d = spec_ref.stft_bound
             (every Re / Im within d).  m = |S| is then within dm = sqrt(2) d + 4 u m (SPEC_MAG_ROUNDINGS = 4: two squares,
             their sum, the root).  max(., 1e-5) and both clamps are 1-Lipschitz; between them spec = 0.2 log10 m + 0.8 with
             slope 0.2 / (m ln 10), largest at the lower end of [mc - dm, mc + dm], mc = max(m, 1e-5):
                 |dspec| <= 0.2 / ln 10 * dm / (mc - dm) + SPEC_LOG_ROUNDINGS u (|20 log10 mc| + 20) / 100 + SPEC_TAIL_ROUNDINGS u
             SPEC_LOG_ROUNDINGS = 8: log10f (2 ulp = 4 u), the product with 20, the difference, the quotient and the rounded
             constant, each on a value of at most |20 log10 mc| + 20; SPEC_TAIL_ROUNDINGS = 4: the clamps' constants, the sum
             with 1, the result.  Where mc <= 2 dm the first term says nothing and the bound is the range's width, 1.
  phasor     compared where m >= 8 sqrt(2) d (PHASOR_MARGIN): there the exact and the computed S subtend an angle
             asin(sqrt(2) d / m) <= 1.01 sqrt(2) d / m, a chord is shorter than its angle and a component's change shorter
             than the chord; plus PHASOR_ROUNDINGS = 8 u for the device's own |S| (4 u relative) and the division, on a
             component of at most 1.  The same bound holds atan2(phasor[1], phasor[0]) against the fp64 angle, plus
             ATAN2_ROUNDINGS = 16 u (3 ulp of a value up to pi), modulo 2 pi.
  synthesis  spec_ref.istft_bound evaluated on |X| = mag (|phasor[0]|, |phasor[1]|), its gamma index N + ceil(N / H) + 6
             raised by what stands between pred and the spectrum the gather sums, each a relative error of X:
                 SYN_CLAMP  = 0    min / max are exact
                 SYN_SCALE  = 10   x = fma(5, c, -4), one rounding of a value of at most 4: |dx| <= 4 u, and 10^x has
                                   condition ln 10 per unit of x: 4 ln 10 u = 9.3 u
                 SYN_EXP10  = 6    exp10f: 3 ulp = 6 u, what OpenCL's full profile requires of exp10 (HIP's own table says 1)
                 SYN_PROD   = 1    mag * phasor[0] and mag * phasor[1], one rounding each, one per element of X
             gamma(a) + gamma(b) + gamma(a) gamma(b) <= gamma(a + b), so the index is N + ceil(N / H) + 6 + 17.
  round trip the analysis' errors carried through the synthesis, which is linear in X, plus the synthesis' own bound at the
             largest spectrum the device can hold: see round_trip_bound.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from tests import spec_ref as SR

U = SR.U
FLOOR = 1e-5
SPEC_MAG_ROUNDINGS, SPEC_LOG_ROUNDINGS, SPEC_TAIL_ROUNDINGS = 4, 8, 4
PHASOR_MARGIN, PHASOR_ROUNDINGS, ATAN2_ROUNDINGS = 8 * math.sqrt(2.0), 8, 16
SYN_CLAMP, SYN_SCALE, SYN_EXP10, SYN_PROD = 0, 10, 6, 1
SYN_RAISE = SYN_CLAMP + SYN_SCALE + SYN_EXP10 + SYN_PROD

#: (n_fft, hop, B, T) of tests/test_gpu_vf_wave.py
SHAPES = [(400, 100, 1, 201), (400, 100, 2, 2000), (400, 100, 3, 4099), (256, 128, 17, 2048), (64, 24, 2, 1000)]
MIN_COMPARED = 0.85


def noise(N, H, B, T):
    """The inputs of tests/test_gpu_voicefilter.py::test_magnitude_on_the_device at another shape: 0.05 rms noise (PCG64),
    fp32; item 0 starts with a silent stretch, the last item carries a 0.9 tone for a while."""
    rng = np.random.Generator(np.random.PCG64(6 + N + T))
    x = (rng.standard_normal((B, T)) * 0.05).astype(np.float32)
    x[0, :min(T // 4, 900)] = 0.0
    lo, hi = (5 * T) // 8, (13 * T) // 16
    x[B - 1, lo:hi] += (0.9 * np.sin(2 * np.pi * 0.06 * np.arange(hi - lo))).astype(np.float32)
    return x


def lengths(N, H, T):
    """Output lengths of the synthesis tests: T, the natural one, one that reads into the last half window."""
    nat = (T // H) * H
    return sorted({T, nat, nat + N // 4 + 3})


def analysis(x, N, H, dtype=torch.float64):
    """x [B][T] -> spec [B][F][W], phasor [B][2][F][W], |S| [B][F][W]"""
    S = SR.stft(x, N, H, dtype).transpose(2, 3).contiguous()                       # [B][2][F][W]
    m = torch.sqrt(S[:, 0] ** 2 + S[:, 1] ** 2)
    spec = torch.clamp((20.0 * torch.log10(torch.clamp(m, min=FLOOR)) - 20.0) / 100.0, min=-1.0, max=0.0) + 1.0
    safe = torch.where(m > 0, m, torch.ones_like(m))
    unit = torch.zeros_like(S)
    unit[:, 0] = 1.0
    phasor = torch.where((m > 0)[:, None], S / safe[:, None], unit)
    return spec, phasor.contiguous(), m


def magnitude_of(pred, dtype=torch.float64, clamp=True, factor=5.0):
    p = torch.as_tensor(pred).to(dtype)
    return 10.0 ** (factor * (torch.clamp(p, 0.0, 1.0) if clamp else p) - 4.0)


def synthesis(pred, phasor, N, H, length=None, dtype=torch.float64, clamp=True, factor=5.0, conjugate=False, edge_imag=False):
    """pred [S][B][F][W], phasor [B][2][F][W] -> y [S][B][L].  The keyword arguments are the mutations of
    tests/test_vf_wave_host.py: no clamp, another factor than 5, the conjugate phasor, Im of bin N / 2 let in."""
    ph = torch.as_tensor(phasor).to(dtype)
    mag = magnitude_of(pred, dtype, clamp, factor)                                 # [S][B][F][W]
    n_src, B = mag.shape[:2]
    X = torch.stack([mag * ph[:, 0], mag * ph[:, 1] * (-1.0 if conjugate else 1.0)], dim=2)      # [S][B][2][F][W]
    X = X.reshape(n_src * B, 2, *X.shape[3:]).transpose(2, 3)
    y = SR.istft(X, N, H, length, dtype)
    if edge_imag:                                               # what Im of bin N / 2 would add: (-1)^t Im X / N per frame
        w = SR.tables(N, dtype)[0]
        sign = torch.tensor([(-1.0) ** t for t in range(N)], dtype=dtype)
        fr = X[:, 1, :, -1:] * sign / N * w
        M = X.shape[2]
        y = y + SR._cut(SR.overlap_add(fr, H), SR.envelope(N, H, M, dtype), N, SR.out_length(M, H, length))
    return y.reshape(n_src, B, -1)


def spec_bound(x, N, H):
    """-> (bound [B][F][W], trivial [B][F][W] bool, d [B][1][W], |S| [B][F][W])"""
    _, _, m = analysis(x, N, H)
    d = SR.stft_bound(x, N, H)[:, None, :]
    dm = math.sqrt(2.0) * d + SPEC_MAG_ROUNDINGS * U * m
    mc = torch.clamp(m, min=FLOOR)
    bound = (0.2 / math.log(10.0) * dm / (mc - dm) + SPEC_LOG_ROUNDINGS * U * ((20 * torch.log10(mc)).abs() + 20) / 100
             + SPEC_TAIL_ROUNDINGS * U)
    trivial = mc <= 2 * dm
    return torch.where(trivial, torch.ones_like(bound), bound), trivial, d, m


def phasor_rule(x, N, H):
    """-> (compared [B][F][W] bool, bound [B][F][W]) for a component of the phasor"""
    _, _, m = analysis(x, N, H)
    d = SR.stft_bound(x, N, H)[:, None, :].expand_as(m)
    sel = (m >= PHASOR_MARGIN * d) & ((m > 0) | (d == 0))          # a silent frame (d = 0) has S = 0 and the phasor (1, 0) exactly
    return sel, 1.01 * math.sqrt(2.0) * d / torch.clamp(m, min=1e-300) + PHASOR_ROUNDINGS * U


def _spectrum_sum(ar, ai, N, H, length):
    """spec_ref.istft_bound's sum without its gamma: ar, ai [S][B][F][W] >= 0 -> [S][B][L]"""
    n_src, B = ar.shape[:2]
    X = torch.stack([ar, ai], dim=2).reshape(n_src * B, 2, *ar.shape[2:]).transpose(2, 3)
    return (SR.istft_bound(X, N, H, length) / SR.gamma(N + math.ceil(N / H) + 6)).reshape(n_src, B, -1)


def synthesis_bound(pred, phasor, N, H, length=None):
    ph = torch.as_tensor(phasor).double().abs()
    mag = magnitude_of(pred)
    return SR.gamma(N + math.ceil(N / H) + 6 + SYN_RAISE) * _spectrum_sum(mag * ph[:, 0], mag * ph[:, 1], N, H, length)


def round_trip_bound(x, N, H, length=None):
    """The bound of synthesis(analysis(x)) with mask 1, both on the device, against the same composition in fp64.  With
    c = 5 ln 10 dspec the device's magnitude is within mag c e^c of the exact one; on a bin whose spec bound is trivial
    (|S| <= 2 dm) both magnitudes lie in [1e-4, max(1e-4, |S| + dm)] instead.  An element of X = mag phasor moves by at most
    dmag + mag dphasor (the device's phasor is a unit vector), and the synthesis' own bound is taken at the largest spectrum
    the device can have got: mag + dmag, components of the phasor at most 1."""
    spec, _, _ = analysis(x, N, H)
    ds, trivial, d, m = spec_bound(x, N, H)
    sel, dp = phasor_rule(x, N, H)
    dp = torch.where(sel, dp, torch.full_like(dp, 2.0))
    mag = magnitude_of(spec)
    c = 5.0 * math.log(10.0) * ds
    dm = math.sqrt(2.0) * d + SPEC_MAG_ROUNDINGS * U * m
    dmag = torch.where(trivial, torch.clamp(m + dm, min=1e-4), mag * c * torch.exp(c))
    move, top = (dmag + mag * dp)[None], (mag + dmag)[None]
    return (SR.gamma(N + math.ceil(N / H) + 6 + SYN_RAISE) * _spectrum_sum(top, top, N, H, length)
            + _spectrum_sum(move, move, N, H, length))


def predictions(x, N, H, n_src, seed=0):
    """The three kinds of fp32 pred [n_src][B][F][W] of the synthesis tests and the fp32 phasor they ride on:
    the spec itself (mask 1), spec x a random mask in [0, 1], values in [-0.5, 1.5] (both clamps are hit)."""
    spec, phasor, _ = analysis(x, N, H)
    spec, phasor = spec.float(), phasor.float()
    g = torch.Generator().manual_seed(seed + N + x.shape[1])
    shape = (n_src,) + tuple(spec.shape)
    preds = {"mask 1": spec.expand(shape), "random mask": spec * torch.rand(shape, generator=g),
             "[-0.5, 1.5]": torch.rand(shape, generator=g) * 2.0 - 0.5}
    return {k: p.contiguous() for k, p in preds.items()}, phasor.contiguous()
