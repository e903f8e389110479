"""The spectral front end on the MI355X (include/specfe.h, speech_separation_amd.spectral): STFT, inverse STFT, their two
adjoints and the log-mel spectrogram against the fp64 oracle tests/spec_ref.py (pinned to torch.stft / torch.istft, their
fp64 autograd and the reference's fixture by tests/test_spectral_host.py), the gradients against fp64 autograd through
torch.stft / torch.istft themselves, and MSESpecLoss / L1SpecLoss under the MAE / MSE rules of tests/test_gpu_wavloss.py.

The bound is NOT the fp32 torch.stft's distance from fp64: an FFT is more accurate than any N-term dot product, and a
"2 x the fp32 reference" rule would fail correct code.  Every value is held to the forward-error bound of a dot product
summed in any order, derived in the docstring of tests/spec_ref.py (u = 2^-24, gamma(n) = n u / (1 - n u)) and never
tuned: stft gamma(N + 3) sum_t |w xp| per frame, istft gamma(N + ceil(N / H) + 6) on the overlap-added absolute inverse
over the envelope, the adjoints the same forms with data and gradient exchanged, log-mel the stft bound propagated
through power, filterbank, clamp and log.  Recorded, not asserted: the worst error / bound per map and the worst ratio
of the kernel's error to the fp32 matrix-product restatement's own error (printed by the last test; DESIGN.md section 24
quotes them).  The mel filterbank's parity with torchaudio is unpinned (tests/spec_ref.py).

Shapes: T = 129 is the smallest legal signal at n_fft 256 (two frames), 255 / 257 / 1000 are no multiples of the hop,
(17, 2048) is a 16-row tile plus one in frames and in items, 4099 gives 33 frames (a 32-frame workgroup plus one),
(16, 32000) is the reference's batch; (64, 24) is a hop that does not divide n_fft.
"""
from __future__ import annotations

import functools
import math
import os
import warnings

import numpy as np
import pytest
import torch

from tests import spec_ref as R
from tests import wavloss_ref

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = R.U
SHAPES = ([(256, 128, B, T) for B, T in ((1, 129), (3, 255), (2, 257), (3, 1000), (17, 2048), (2, 4099))]
          + [(400, 200, B, T) for B, T in ((1, 201), (3, 1000), (2, 4099))]
          + [(64, 24, B, T) for B, T in ((1, 33), (3, 333), (17, 1000))])
BIG = (256, 128, 16, 32000)
SCALES = (1.0, 1e-3, 1e3)            # per-item scales, three decades apart, cycled over the batch
WORST = {}                           # map -> [worst error / bound, worst error / fp32 restatement's error]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _scaled_noise(shape, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    s = torch.tensor([SCALES[i % 3] for i in range(shape[0])]).reshape(-1, *([1] * (len(shape) - 1)))
    return x * s


@functools.lru_cache(maxsize=None)
def signal(B, T, seed=0):
    """Seeded noise [B][T], item i scaled by SCALES[i % 3], the first third of item 0 scaled by 1e-3.  Shared, never modified."""
    x = _scaled_noise((B, T), 1000 * B + T + seed)
    x[0, :T // 3] *= 1e-3
    return x


@functools.lru_cache(maxsize=None)
def spectrogram(B, M, F, seed=0):
    """A random [B][2][M][F] that is no signal's STFT (Im of bins 0 and N / 2 non-zero), item i scaled by SCALES[i % 3]."""
    return _scaled_noise((B, 2, M, F), 77 * B + M + F + seed)


def lengths(M, N, H):
    nat = (M - 1) * H
    return [None, nat - 24, nat + 76 if 76 < N // 2 else nat + N // 4, nat + N // 2 + 10]


def record(name, got, want, bound, fp32=None):
    """Assert |got - want| <= bound everywhere; keep the worst ratios."""
    err = (got.double().cpu() - want).abs()
    assert got.dtype == torch.float32 and got.shape == want.shape and bool(torch.isfinite(got).all()), name
    bound = bound.expand_as(err)
    nz = bound > 0
    ratio = float((err[nz] / bound[nz]).max()) if bool(nz.any()) else 0.0
    rel32 = float("nan")
    if fp32 is not None:
        e32 = float((fp32.double() - want).abs().max())
        rel32 = float(err.max()) / e32 if e32 > 0 else 0.0
    w = WORST.setdefault(name.split()[0], [0.0, 0.0])
    w[0], w[1] = max(w[0], ratio), max(w[1], rel32 if rel32 == rel32 else 0.0)
    print(f"specfe {name}: worst error / bound {ratio:.4f}, max error / fp32 restatement's {rel32:.2f}")
    assert bool((err[~nz] == 0).all()), name                     # a zero bound: every term is zero, the result is exactly 0
    assert ratio <= 1.0, (name, ratio)


def _torch_stft(x, N, H):
    a = torch.stft(x, n_fft=N, hop_length=H, window=torch.hann_window(N, dtype=x.dtype), return_complex=True)
    return torch.stack([a.real, a.imag], dim=1).transpose(2, 3)


def _torch_istft(X, N, H, length):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return torch.istft(torch.complex(X[:, 0], X[:, 1]).transpose(1, 2), n_fft=N, hop_length=H,
                           window=torch.hann_window(N, dtype=X.dtype), length=length)


def check_stft(dev, N, H, x, name, gamma_scale=1.0, fp32=True):
    from speech_separation_amd.spectral import stft_forward
    got = stft_forward(x.to(dev), N, H)
    bound = gamma_scale * R.stft_bound(x, N, H)[:, None, :, None]
    record(name, got, R.stft(x, N, H), bound, R.stft(x, N, H, torch.float32) if fp32 else None)
    return got.cpu()


@pytest.mark.parametrize("N,H,B,T", SHAPES + [BIG])
def test_stft_values(dev, N, H, B, T):
    got = check_stft(dev, N, H, signal(B, T), f"stft ({N}, {H}) {B}x{T}")
    assert got.shape == (B, 2, 1 + T // H, N // 2 + 1)
    assert bool((got[:, 1, :, 0] == 0).all()) and bool((got[:, 1, :, -1] == 0).all())       # Im of bins 0 and N / 2: the table is exact there


@pytest.mark.parametrize("N,H,B,T", SHAPES + [BIG])
def test_istft_values(dev, N, H, B, T):
    from speech_separation_amd.spectral import istft_forward
    M, F = 1 + T // H, N // 2 + 1
    X = spectrogram(B, M, F)
    assert float(X[:, 1, :, 0].abs().min()) > 0 and float(X[:, 1, :, -1].abs().min()) > 0
    for length in lengths(M, N, H) if (N, H, B, T) != BIG else [32000]:
        if length is not None and length < 1:
            continue
        got = istft_forward(X.to(dev), N, H, length)
        record(f"istft ({N}, {H}) {B}x{M} length {length}", got, R.istft(X, N, H, length), R.istft_bound(X, N, H, length),
               R.istft(X, N, H, length, torch.float32))
        if length is not None and length > (M - 1) * H + N // 2:
            assert bool((got[:, (M - 1) * H + N // 2:] == 0).all()) and bool((got[:, (M - 1) * H:(M - 1) * H + N // 2] != 0).all())


@pytest.mark.parametrize("N,H,B,T", SHAPES + [BIG])
def test_adjoints_against_fp64_autograd_through_torch(dev, N, H, B, T):
    from speech_separation_amd.spectral import istft_backward, stft_backward
    M, F = 1 + T // H, N // 2 + 1
    x = signal(B, T).double().requires_grad_(True)
    gX = spectrogram(B, M, F, seed=1)
    want, = torch.autograd.grad(_torch_stft(x, N, H), x, gX.double())
    got = stft_backward(gX.to(dev), T, N, H)
    record(f"stft_backward ({N}, {H}) {B}x{T}", got, want, R.stft_backward_bound(gX, T, N, H), R.stft_backward(gX, T, N, H, torch.float32))
    for length in lengths(M, N, H) if (N, H, B, T) != BIG else [32000]:
        if length is not None and length < 1:
            continue
        X = spectrogram(B, M, F).double().requires_grad_(True)
        y = _torch_istft(X, N, H, length)
        gy = signal(B, y.shape[1], seed=2)
        want, = torch.autograd.grad(y, X, gy.double())
        got = istft_backward(gy.to(dev), M, N, H)
        bound = R.istft_backward_bound(gy, M, N, H)[:, None].expand(B, 2, M, F).clone()
        bound[:, 1, :, 0] = 0                                    # Im of bins 0 and N / 2: the oracle's gradient is exactly 0
        bound[:, 1, :, -1] = 0
        assert float(want[:, 1, :, 0].abs().max()) == 0 and float(want[:, 1, :, -1].abs().max()) == 0
        record(f"istft_backward ({N}, {H}) {B}x{M} length {length}", got, want, bound, R.istft_backward(gy, M, N, H, torch.float32))


@pytest.mark.parametrize("B,T", [(1, 201), (3, 1000), (2, 4099), (3, 32000)])
def test_logmel_values(dev, B, T):
    from speech_separation_amd.spectral import LogMelSpectrogram
    x = signal(B, T, seed=3)
    mel = LogMelSpectrogram()
    got = mel(x.to(dev))
    assert got.shape == (B, 128, 1 + T // 200)
    record(f"logmel {B}x{T}", got, R.logmel(x), R.logmel_bound(x), R.logmel(x, dtype=torch.float32))
    assert torch.equal(mel(x.to(dev)[:, None]), got[:, None])    # [B, 1, T] -> [B, 1, n_mels, frames]
    with pytest.raises(RuntimeError, match="no backward"):
        mel(x.to(dev).requires_grad_(True))
    small = LogMelSpectrogram(sample_rate=8000, n_fft=256, hop_length=64, n_mels=40)
    record(f"logmel 8 kHz 40 bands {B}x{T}", small(x.to(dev)), R.logmel(x, 8000, 256, 64, 40), R.logmel_bound(x, 8000, 256, 64, 40))


@pytest.mark.parametrize("N,H", [(256, 128), (400, 200), (64, 24)])
def test_hard_inputs(dev, N, H):
    from speech_separation_amd.spectral import LogMelSpectrogram, stft_forward
    T = 9 * N + 37
    # an all-zero stretch longer than a frame: its rows are exactly 0, and exactly the clamp's log for log-mel
    x = signal(2, T, seed=4).clone()
    x[:, 3 * N:6 * N] = 0
    got = check_stft(dev, N, H, x, f"stft ({N}, {H}) zero stretch")
    silent = [m for m in range(1 + T // H) if 3 * N <= m * H - N // 2 and m * H + N // 2 <= 6 * N]
    assert len(silent) >= 2 and bool((got[:, :, silent] == 0).all()) and bool((got[:, :, silent[0] - 2].abs().max() > 0))
    if (N, H) == (400, 200):
        S = LogMelSpectrogram()(x.to(dev)).cpu()
        record("logmel zero stretch", S, R.logmel(x), R.logmel_bound(x))
        assert bool((S[:, :, silent] == float(np.float32(math.log(1e-5)))).all())       # exactly log(1e-5), rounded once
    # unit impulses: every output is one w cos product -- two where the reflection doubles the impulse --, so the bound is a
    # few u: the rounded window entry, the rounded table entry, the product, and one addition -> 5 u sum_t |w xp|
    T = 4 * N + 5
    for n in (0, 1, N // 2 - 1, N // 2, T - 2, T - 1):
        x = torch.zeros(1, T)
        x[0, n] = 1.0
        check_stft(dev, N, H, x, f"stft_impulse ({N}, {H}) at {n}", gamma_scale=5 * U / R.gamma(N + 3), fp32=False)
    # a DC offset of 100 under unit noise
    g = torch.Generator().manual_seed(6)
    check_stft(dev, N, H, torch.randn(2, 5 * N + 3, generator=g) + 100.0, f"stft ({N}, {H}) DC offset")


def test_loss_backward_through_a_masked_round_trip(dev):
    """loss.backward() through istft(mask * stft(x)) with a linear loss sum(c y): both gradients against fp64 autograd through
    torch.stft / torch.istft.  The bounds compose the two adjoints' (tests/spec_ref.py): with G = mask * istft_backward(c) and
    e its bound (mask times the istft_backward bound, plus u |G| for the product), d loss / d x is within
    stft_backward_bound(G) + |adjoint|(e) (1 + gamma); d loss / d mask = gRe Re X + gIm Im X is within
    e_i (|Re X| + |Im X|) + (|gRe| + |gIm|) (d + e_i d) + 4 u (|gRe Re X| + |gIm Im X|), e_i the istft_backward bound, d stft's."""
    from speech_separation_amd import STFT
    N, H, B, T = 256, 128, 3, 1000
    M, F = 1 + T // H, N // 2 + 1
    enc = STFT(N, H)
    g = torch.Generator().manual_seed(8)
    x0, mask0, c = signal(B, T, seed=5), torch.rand(B, 1, M, F, generator=g), torch.randn(B, T, generator=g)
    x, mask = x0.to(dev).requires_grad_(True), mask0.to(dev).requires_grad_(True)
    y = enc.istft(mask * enc.stft(x), length=T)
    assert y.shape == (B, T) and y.requires_grad
    (y * c.to(dev)).sum().backward()
    xd, md = x0.double().requires_grad_(True), mask0.double().requires_grad_(True)
    (_torch_istft(md * _torch_stft(xd, N, H), N, H, T) * c.double()).sum().backward()
    gi = R.istft_backward(c, M, N, H)                            # [B, 2, M, F] fp64
    ei = R.istft_backward_bound(c, M, N, H)[:, None].expand(B, 2, M, F)
    G = mask0.double() * gi
    e = mask0.double() * ei + U * G.abs()
    gam = R.gamma(N + math.ceil(N / H) + 6)
    record("roundtrip d/dx", x.grad, xd.grad, R.stft_backward_bound(G, T, N, H) + R.stft_backward_bound(e, T, N, H) / gam * (1 + gam))
    X, d = R.stft(x0, N, H), R.stft_bound(x0, N, H)[:, None, :, None]
    bm = (ei * X.abs()).sum(1, keepdim=True) + (gi.abs() * (d + ei * d)).sum(1, keepdim=True) + 4 * U * (gi * X).abs().sum(1, keepdim=True)
    record("roundtrip d/dmask", mask.grad, md.grad, bm)
    gx, = torch.autograd.grad(enc.stft(x).square().sum(), x)     # torch.autograd.grad works as well
    assert gx.shape == x.shape and bool(torch.isfinite(gx).all())


@pytest.mark.parametrize("N,H,B,T", [(256, 128, 3, 1000), (256, 128, 17, 2048), (64, 24, 3, 333), (400, 200, 3, 1000)])
def test_two_calls_are_bitwise_equal_and_items_do_not_depend_on_the_batch(dev, N, H, B, T):
    from speech_separation_amd import spectral as S
    M, F = 1 + T // H, N // 2 + 1
    x, X = signal(B, T).to(dev), spectrogram(B, M, F).to(dev)
    L = (M - 1) * H + 76 if 76 < N // 2 else (M - 1) * H + N // 4
    gy = signal(B, L, seed=2).to(dev)
    calls = {"stft": (lambda a: S.stft_forward(a, N, H), x), "stft_backward": (lambda a: S.stft_backward(a, T, N, H), X),
             "istft": (lambda a: S.istft_forward(a, N, H, L), X), "istft_backward": (lambda a: S.istft_backward(a, M, N, H), gy)}
    if (N, H) == (400, 200):
        calls["logmel"] = (lambda a: S.logmel_forward(a, 16000, N, H, 128), x)
    for name, (fn, arg) in calls.items():
        a, b = fn(arg), fn(arg)
        assert torch.equal(a, b), name
        for i in (0, B - 1):
            assert torch.equal(fn(arg[i:i + 1].contiguous())[0], a[i]), (name, i)


def test_add_spectrogram_keys_on_a_pinned_batch(dev, tmp_path):
    from dataset_fixture import make_dataset
    from speech_separation_amd import DPTNAVWavEncDec, LogMelSpectrogram, STFT, add_spectrogram_keys
    from speech_separation_amd.io import PinnedBatcher, load_item
    from speech_separation_amd.spec import synthetic_state_dict
    entries, _ = make_dataset(str(tmp_path), n=2, T=32000)
    items = [load_item(e, 8000) for e in entries]
    batch = PinnedBatcher(dev).to_device(items)
    before = dict(batch)
    assert not any(k in batch for k in ("complex_spectrogram", "mix_spectrogram", "s1_spectrogram", "s2_spectrogram"))
    out = add_spectrogram_keys(batch)
    assert out is batch
    assert batch["complex_spectrogram"].shape == (2, 2, 251, 129)
    for k in ("mix", "s1", "s2"):
        assert batch[k + "_spectrogram"].shape == (2, 128, 161) and batch[k + "_spectrogram"].device == dev
        assert torch.equal(batch[k + "_spectrogram"], LogMelSpectrogram()(batch[k]))
        assert not batch[k + "_spectrogram"].requires_grad
    assert torch.equal(batch["complex_spectrogram"], STFT().stft(batch["mix"]))
    record("add_spectrogram_keys complex", batch["complex_spectrogram"], R.stft(batch["mix"].cpu(), 256, 128),
           R.stft_bound(batch["mix"].cpu(), 256, 128)[:, None, :, None])
    assert all(batch[k] is before[k] for k in before)            # nothing else is touched
    # a key whose waveform is absent stays absent
    infer = {"mix": batch["mix"], "s1": None, "audio_path": batch["audio_path"]}
    add_spectrogram_keys(infer, stft=STFT(64, 24))
    assert set(infer) == {"mix", "s1", "audio_path", "mix_spectrogram", "complex_spectrogram"} and infer["s1"] is None
    assert infer["complex_spectrogram"].shape == (2, 2, 1 + 32000 // 24, 33)
    # the separator accepts the batch with the new keys
    model = DPTNAVWavEncDec(num_features=128, video_emb_size=512, hidden_video=128, kernel_size_enc=7, hidden_dim=128,
                            num_blocks=1, chunk_size=150, step_size=75, num_heads=4)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in synthetic_state_dict(model.cfg, seed=0).items()})
    model = model.to(dev).eval()
    with torch.no_grad():
        o = model(**batch)
    assert o["s1_pred"].shape == (2, 32000) and bool(torch.isfinite(o["s1_pred"]).all())


def _spec_case(B, F, T):
    return [a.reshape(B, F, T) for a in wavloss_ref.make_case(B, F * T, seed=B + F + T, swapped=tuple(range(1, B, 2)))]


@pytest.mark.parametrize("cls,kind", [("MSESpecLoss", "mse"), ("L1SpecLoss", "mae")])
@pytest.mark.parametrize("B,F,T", [(2, 129, 3), (5, 201, 17), (3, 9, 7)])
def test_spec_losses(dev, cls, kind, B, F, T):
    """The MAE / MSE rules of tests/test_gpu_wavloss.py (its `check`) on the [B, F T] view, batch level on inputs as built and
    with the predictions exchanged, utterance level on the mixed batch; the choice is decided on the oracle first."""
    import speech_separation_amd as S
    from tests.test_gpu_wavloss import assert_decided, check
    arrays = _spec_case(B, F, T)
    for level, order in (("batch", (0, 1, 2, 3)), ("batch", (1, 0, 2, 3)), ("utterance", (0, 1, 2, 3))):
        a = [arrays[i] for i in order]
        if level == "batch":                                     # every item on one permutation: undo the mixed batch's exchanges
            a = [x.copy() for x in a]
            for i in range(1, B, 2):
                a[0][i], a[1][i] = a[1][i].copy(), a[0][i].copy()
        flat = [x.reshape(B, F * T) for x in a]
        label = f"{cls} {level} {B}x{F}x{T} order {order}"
        o64 = wavloss_ref.evaluate(kind, level, *flat)
        assert_decided(o64, level, label)
        if level == "batch":
            assert int(o64["perm"][0]) == int(order[0] == 1)
        else:
            assert o64["perm"].tolist() == [i & 1 for i in range(B)]
        t = [torch.from_numpy(x).to(dev) for x in a]
        t[0].requires_grad_(True)
        t[1].requires_grad_(True)
        crit = getattr(S, cls)(pit=level)
        loss = crit(s1_spec_pred=t[0], s2_spec_pred=t[1], s1_spec_true=t[2], s2_spec_true=t[3], mix=None)["loss"]
        assert loss.dim() == 0 and loss.device == dev
        loss.backward()
        got = {"d1": t[0].grad.reshape(B, F * T).cpu().numpy(), "d2": t[1].grad.reshape(B, F * T).cpu().numpy(),
               "out": crit.last.cpu().numpy(), "perm": crit.last_perm.cpu().numpy()}
        assert float(loss.detach()) == float(got["out"][0]) and t[0].grad.shape == (B, F, T)
        check(kind, level, flat, got, o64, None, label)


@pytest.mark.parametrize("cls,name", [("MSESpecLoss", "mse"), ("L1SpecLoss", "l1")])
def test_spec_losses_reproduce_the_reference_fixture(dev, cls, name):
    import speech_separation_amd as S
    from tests.test_gpu_wavloss import check
    z = np.load(os.path.join(ROOT, "tests", "golden", "spec_small.npz"))
    arrays = [z["spec." + k] for k in ("p1", "p2", "s1", "s2")]
    for perm in (0, 1):
        a = [arrays[1], arrays[0], arrays[2], arrays[3]] if perm else arrays
        t = [torch.from_numpy(x).to(dev) for x in a]
        t[0].requires_grad_(True)
        t[1].requires_grad_(True)
        crit = getattr(S, cls)()
        crit(s1_spec_pred=t[0], s2_spec_pred=t[1], s1_spec_true=t[2], s2_spec_true=t[3])["loss"].backward()
        o64 = {"perm": np.full(3, int(z[f"{name}.{perm}.perm"])), "loss": z[f"{name}.{perm}.loss64"], "l0": z[f"{name}.{perm}.l0_64"],
               "l1": z[f"{name}.{perm}.l1_64"], "d1": z[f"{name}.{perm}.d1_64"].reshape(3, 63), "d2": z[f"{name}.{perm}.d2_64"].reshape(3, 63)}
        got = {"d1": t[0].grad.reshape(3, 63).cpu().numpy(), "d2": t[1].grad.reshape(3, 63).cpu().numpy(),
               "out": crit.last.cpu().numpy(), "perm": crit.last_perm.cpu().numpy()}
        assert int(o64["perm"][0]) == perm
        check("mse" if name == "mse" else "mae", "batch", [x.reshape(3, 63) for x in a], got, o64, None, f"{cls} fixture perm {perm}")


def test_reference_fixture_values(dev):
    from speech_separation_amd import STFT
    z = np.load(os.path.join(ROOT, "tests", "golden", "spec_small.npz"))
    x = torch.from_numpy(z["x"])
    got = STFT().stft(x.to(dev))
    record("stft_vs_fp32_fft fixture (the last ratio is to the reference's fp32 FFT)", got, torch.from_numpy(z["stft64"]), R.stft_bound(x, 256, 128)[:, None, :, None], torch.from_numpy(z["stft32"]))
    X = torch.from_numpy(z["X"])
    for length in (1000, 1100):
        record(f"istft_vs_fp32_fft fixture length {length}", STFT().istft(X.to(dev), length=length), torch.from_numpy(z[f"istft{length}_64"]),
               R.istft_bound(X, 256, 128, length), torch.from_numpy(z[f"istft{length}_32"]))


def test_argument_errors_launch_nothing(dev):
    import ctypes
    from speech_separation_amd import _lib
    from speech_separation_amd.spectral import _handle
    lib = _lib.load()
    h, hm = _handle(dev, 256, 128), _handle(dev, 400, 200, 16000, 128)
    stream = torch.cuda.current_stream(dev).cuda_stream
    src = torch.ones(1 << 16, device=dev)
    out = torch.full((1 << 16,), 7.0, device=dev)
    s, o = src.data_ptr(), out.data_ptr()
    bad = [lib.specfe_stft(h, s, 2, 128, o, stream), lib.specfe_stft(h, s, 0, 1000, o, stream), lib.specfe_stft(h, None, 2, 1000, o, stream),
           lib.specfe_stft(h, s, 2, 1000, None, stream), lib.specfe_stft(h, s, 1 << 20, 1000, o, stream),
           lib.specfe_stft(h, s, 1, 1 << 27, o, stream), lib.specfe_stft_backward(h, s, 2, 128, o, stream),
           lib.specfe_stft_backward(h, s, -1, 1000, o, stream), lib.specfe_logmel(h, s, 2, 1000, o, stream),
           lib.specfe_logmel(hm, s, 2, 200, o, stream), lib.specfe_istft(h, s, 2, 0, 100, o, stream),
           lib.specfe_istft(h, s, 2, 1, 0, o, stream), lib.specfe_istft(h, s, 0, 9, 0, o, stream),
           lib.specfe_istft(h, s, 2, 9, 1 << 27, o, stream), lib.specfe_istft_backward(h, s, 2, 1, 0, o, stream),
           lib.specfe_istft_backward(h, None, 2, 9, 0, o, stream)]
    torch.cuda.synchronize()
    assert bad == [1] * len(bad), bad
    assert bool((out == 7).all())
    assert lib.specfe_stft(h, s, 2, 1000, o, stream) == 0
    torch.cuda.synchronize()
    assert not bool((out[:2 * 2 * 8 * 129] == 7).any()) and bool((out[2 * 2 * 8 * 129:] == 7).all())
    # a handle of its own is created and destroyed without touching the cached ones
    own = ctypes.c_void_p()
    assert lib.specfe_create(512, 1, ctypes.byref(own)) == 0 and own.value
    lib.specfe_destroy(own)
    with pytest.raises(ValueError, match="more than n_fft / 2"):
        from speech_separation_amd import STFT
        STFT().stft(torch.zeros(2, 128, device=dev))


def test_zz_worst_ratios_are_reported():
    """The worst error / bound and error / fp32-restatement ratios this session saw, per map (DESIGN.md section 24 quotes them)."""
    for k, (a, b) in sorted(WORST.items()):
        print(f"specfe worst {k}: error / bound {a:.4f}, error / fp32 restatement's error {b:.2f}")
    assert all(a <= 1.0 for a, _ in WORST.values())
