"""Waveform criteria on the MI355X (include/wavloss.h, speech_separation_amd.MAEWavLoss / MSEWavLoss / SiSNRWavLoss):
loss, permutation and d loss / d prediction of the six (kind, level) pairs against the fp64 oracle tests/wavloss_ref.py
(pinned to the reference's own classes by tests/test_wavloss_host.py) and against the reference's fixtures.

Tolerances, each from fp32 rounding (u = 2^-24), none tuned to the code:
  MAE gradient    sign pattern == sign(p - s_sigma) at every sample, zeros included (an fp32 difference has the exact
                  sign); magnitude within 2 u relative of grad_scale / (2 B T) (one rounded weight)
  MSE gradient    within 4 u relative, element by element (one subtraction, one rounded weight, one product); absolute
                  floor: the smallest normal fp32
  MAE / MSE loss, L0, L1    within 1e-6 relative of the fp64 value (double accumulation gives ~2^-23; the margin covers a
                  compensated-fp32 implementation)
  SI-SNR          no bound derives through the log of a cancelling ratio: |hip - fp64| <= 2 x |fp32 reference - fp64| on
                  the same inputs + 4 u |value| for the loss values; for a gradient tensor both errors are max-abs errors
                  relative to the fp64 gradient's max-abs, with a 4 u floor.  The fp32 reference is the reference's own
                  class for fixture inputs and tests/wavloss_ref.py run in fp32 otherwise.
The permutation must equal the oracle's on EVERY item; the inputs are built so that no choice is decided by rounding
(asserted on the oracle before the kernel is looked at).  Shapes: T = 1023, 1025, 4099 leave every row after the first
4-byte aligned only, B = 257 is more items than any fixed-size array of a workgroup would hold, (2, 1) is the smallest
MAE / MSE problem, (16, 32000) the reference's real size.
"""
from __future__ import annotations

import functools
import os

import numpy as np
import pytest
import torch

from tests import wavloss_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24
TINY = float(np.finfo(np.float32).tiny)
SHAPES = [(1, 16), (2, 1023), (3, 1025), (5, 4099), (257, 64)]
CASES = [(k, s) for k in R.KINDS for s in SHAPES] + [(k, (2, 1)) for k in ("mae", "mse")]
WORST = {}          # (what) -> worst observed error / bound over this session (SI-SNR), printed by the last test


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _swapped(B, which):
    return {"perm0": (), "perm1": tuple(range(B)), "close": (), "mixed": tuple(range(1, B, 2))}[which]


@functools.lru_cache(maxsize=None)
def case(B, T, which):
    """Seeded inputs (shared, never modified) of one shape and kind of input."""
    arrays = R.make_case(B, T, seed=1000 * B + T + len(which), swapped=_swapped(B, which), mix=0.3 if which == "close" else 0.0)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def oracle(kind, level, B, T, which, bits=64):
    return R.evaluate(kind, level, *case(B, T, which), dtype=torch.float64 if bits == 64 else torch.float32)


def run_hip(dev, kind, level, arrays, grad_scale=1.0):
    from speech_separation_amd.metrics import wavloss_pit_loss
    d1, d2, out, perm = wavloss_pit_loss(kind, level, *[torch.from_numpy(np.array(a)).to(dev) for a in arrays],
                                         grad_scale=grad_scale)
    torch.cuda.synchronize()
    return {"d1": d1.cpu().numpy(), "d2": d2.cpu().numpy(), "out": out.cpu().numpy(), "perm": perm.cpu().numpy()}


def _record(what, err, bound):
    ratio = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print(f"wavloss {what}: error {err:.3e}, bound {bound:.3e}, ratio {ratio:.3f}")


def check(kind, level, arrays, got, o64, o32, label):
    """`got` (the kernel) against `o64` under the rules of the module docstring; `o32`: the fp32 reference (SI-SNR only)."""
    p1, p2, s1, s2 = (a.astype(np.float64) for a in arrays)
    B, T = p1.shape
    perm = np.asarray(o64["perm"]).astype(np.int64)
    assert got["perm"].dtype == np.int32 and np.array_equal(got["perm"], perm), (label, got["perm"], perm)
    assert got["out"][1] == perm.sum()
    vals = {"loss": got["out"][0], "l0": got["out"][2], "l1": got["out"][3]}
    if level == "batch":
        assert got["out"][0] == min(got["out"][2], got["out"][3])
    sw = perm.astype(bool)[:, None]
    t1, t2 = np.where(sw, s2, s1), np.where(sw, s1, s2)          # the chosen target of each prediction
    for k, v in vals.items():
        want = float(o64[k])
        print(f"wavloss {label} {k}: hip {float(v)!r} fp64 {want!r}")
        if kind != "sisnr":
            assert abs(float(v) - want) <= 1e-6 * abs(want), (label, k)
        else:
            bound = 2 * abs(float(o32[k]) - want) + 4 * U * abs(want)
            _record(f"sisnr {k}", abs(float(v) - want), bound)
            assert abs(float(v) - want) <= bound, (label, k)
    for d, p, t, key in ((got["d1"], p1, t1, "d1"), (got["d2"], p2, t2, "d2")):
        want = np.asarray(o64[key], dtype=np.float64)
        assert d.dtype == np.float32 and d.shape == (B, T) and np.all(np.isfinite(d))
        if kind == "mae":
            w = 1.0 / (2.0 * B * T)
            assert np.array_equal(np.sign(d), np.sign(p - t)) and np.array_equal(np.sign(d), np.sign(want)), (label, key)
            nz = d != 0
            assert np.all(np.abs(np.abs(d[nz].astype(np.float64)) - w) <= 2 * U * w), (label, key)
        elif kind == "mse":
            assert np.all(np.abs(d - want) <= 4 * U * np.abs(want) + TINY), (label, key)
        else:
            scale = np.max(np.abs(want))
            err, err32 = np.max(np.abs(d - want)) / scale, np.max(np.abs(np.asarray(o32[key], dtype=np.float64) - want)) / scale
            _record(f"sisnr gradient", err, 2 * err32 + 4 * U)
            assert err <= 2 * err32 + 4 * U, (label, key, err, err32)


def assert_decided(o64, level, label):
    """A condition on the INPUTS, checked on the fp64 oracle: no permutation choice is within reach of rounding."""
    l0, l1 = float(o64["l0"]), float(o64["l1"])
    if level == "batch":
        assert abs(l0 - l1) > 0.05 * max(abs(l0), abs(l1)), (label, l0, l1)      # they differ in their first digits
    else:
        i0, i1 = o64["item0"], o64["item1"]
        assert np.all(np.abs(i0 - i1) > 1e-3 * np.maximum(np.abs(i0), np.abs(i1))), (label, i0, i1)


@pytest.mark.parametrize("which", ["perm0", "perm1", "close"])
@pytest.mark.parametrize("kind,shape", CASES)
def test_batch_level(dev, kind, shape, which):
    B, T = shape
    label = f"{kind} batch {B}x{T} {which}"
    o64 = oracle(kind, "batch", B, T, which)
    assert_decided(o64, "batch", label)
    assert int(o64["perm"][0]) == {"perm0": 0, "perm1": 1, "close": 0}[which]
    o32 = oracle(kind, "batch", B, T, which, 32) if kind == "sisnr" else None
    check(kind, "batch", case(B, T, which), run_hip(dev, kind, "batch", case(B, T, which)), o64, o32, label)


@pytest.mark.parametrize("kind,shape", CASES)
def test_utterance_level_on_a_mixed_batch(dev, kind, shape):
    """The odd items have their predictions exchanged: permutation 1 there, permutation 0 on the even ones."""
    B, T = shape
    label = f"{kind} utterance {B}x{T} mixed"
    o64 = oracle(kind, "utterance", B, T, "mixed")
    assert_decided(o64, "utterance", label)
    assert o64["perm"].tolist() == [i & 1 for i in range(B)]
    o32 = oracle(kind, "utterance", B, T, "mixed", 32) if kind == "sisnr" else None
    got = run_hip(dev, kind, "utterance", case(B, T, "mixed"))
    check(kind, "utterance", case(B, T, "mixed"), got, o64, o32, label)
    if kind == "mae" and T >= 4:             # p == s exactly on a block of item 0: the gradient is exactly 0 there
        assert np.all(got["d1"][0, T // 4:T // 2] == 0) and np.any(got["d1"][0, :T // 4] != 0)


@pytest.mark.parametrize("kind", R.KINDS)
def test_reference_clip_size(dev, kind):
    """16 x 32000, the reference's batch of 2 s clips: both levels on the mixed batch."""
    B, T = 16, 32000
    for level in R.LEVELS:
        label = f"{kind} {level} {B}x{T} mixed"
        o64 = oracle(kind, level, B, T, "mixed")
        assert_decided(o64, level, label)
        o32 = oracle(kind, level, B, T, "mixed", 32) if kind == "sisnr" else None
        check(kind, level, case(B, T, "mixed"), run_hip(dev, kind, level, case(B, T, "mixed")), o64, o32, label)


@pytest.mark.parametrize("name", ["wavloss_b2_t1", "wavloss_mixed_b5_t67", "wavloss_swap_b3_t131"])
def test_reference_fixtures(dev, name):
    """The values and loss.backward() gradients the reference's own classes produced (tools/gen_golden_wavloss.py): the
    fp64 ones are the truth, the fp32 ones give the SI-SNR rule its distance.  Against the fp32 gradients themselves: the
    MAE sign pattern is the same (exact in fp32 on both sides), MSE agrees within 8 u relative (each side is within 4 u
    of fp64)."""
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    arrays = [z[k] for k in ("s1_pred", "s2_pred", "s1", "s2")]
    for kind in z["kinds"]:
        for level in R.LEVELS:
            key = f"{kind}.{level}."
            o64, o32 = ({"perm": z[key + "perm64"], "loss": z[key + f"loss{b}"], "l0": z[key + f"l0_{b}"], "l1": z[key + f"l1_{b}"],
                         "d1": z[key + f"d1_{b}"], "d2": z[key + f"d2_{b}"]} for b in (64, 32))
            got = run_hip(dev, kind, level, arrays)
            check(kind, level, arrays, got, o64, o32, f"{name} {kind} {level}")
            for k in ("d1", "d2"):
                if kind == "mae":
                    assert np.array_equal(np.sign(got[k]), np.sign(o32[k]))
                elif kind == "mse":
                    assert np.all(np.abs(got[k].astype(np.float64) - o32[k]) <= 8 * U * np.abs(o32[k]) + TINY)


def test_cross_checks_with_the_existing_sisnr_loss(dev):
    from speech_separation_amd.metrics import SiSNRWavLoss, _engine, wavloss_pit_loss
    for which in ("perm0", "perm1"):
        t = [torch.from_numpy(np.array(a)).to(dev) for a in case(5, 4099, which)]
        # the new unit, SI-SNR at batch level, against dptnav_pit_sisnr_loss
        d1, d2, out, perm = wavloss_pit_loss("sisnr", "batch", *t)
        e1, e2, eout = _engine(dev).pit_sisnr_loss(*t)
        assert int(eout[1]) == int(perm[0]) == int(which == "perm1") and int(out[1]) == 5 * int(eout[1])
        for a, b in ((out[0], eout[0]), (out[2], eout[2]), (out[3], eout[3])):
            assert abs(float(a) - float(b)) <= 1e-6 * abs(float(b))
        # SiSNRWavLoss(pit="utterance") on one item against SiSNRWavLoss() on the same item
        one = [x[2:3] for x in t]
        cu, cb = SiSNRWavLoss(pit="utterance"), SiSNRWavLoss()
        lu, lb = cu(*one)["loss"], cb(*one)["loss"]
        assert int(cu.last_perm[0]) == int(cb.last[1]) == int(which == "perm1") and cb.last_perm is None
        assert abs(float(lu) - float(lb)) <= 1e-6 * abs(float(lb))


@pytest.mark.parametrize("shape", [(5, 4099), (257, 64)])
def test_two_calls_are_bitwise_equal(dev, shape):
    for kind in R.KINDS:
        for level in R.LEVELS:
            a, b = (run_hip(dev, kind, level, case(*shape, "mixed")) for _ in range(2))
            for k in a:
                assert a[k].tobytes() == b[k].tobytes(), (kind, level, k)


@pytest.mark.parametrize("cls,pit", [("MAEWavLoss", "batch"), ("MSEWavLoss", "utterance"), ("SiSNRWavLoss", "utterance")])
def test_module_call_chaining_and_grad_scale(dev, cls, pit):
    import speech_separation_amd as S
    from speech_separation_amd.metrics import wavloss_pit_loss
    kind = {"MAEWavLoss": "mae", "MSEWavLoss": "mse", "SiSNRWavLoss": "sisnr"}[cls]
    t = dict(zip(("s1_pred", "s2_pred", "s1", "s2"), (torch.from_numpy(np.array(a)).to(dev) for a in case(3, 1025, "mixed"))))
    d1, d2, out, perm = wavloss_pit_loss(kind, pit, **t)
    t["s1_pred"].requires_grad_(True)
    t["s2_pred"].requires_grad_(True)
    t["s2"].requires_grad_(True)                       # a target that requires grad gets None
    crit = getattr(S, cls)(pit=pit)
    loss = crit(**t, mix=None)["loss"]
    assert loss.dim() == 0 and loss.device == dev and loss.requires_grad
    (3.0 * loss).backward()
    assert torch.equal(t["s1_pred"].grad, 3.0 * d1) and torch.equal(t["s2_pred"].grad, 3.0 * d2) and t["s2"].grad is None
    assert torch.equal(crit.last, out) and float(loss.detach()) == float(out[0]) and torch.equal(crit.last_perm, perm)
    assert crit.last_perm.dtype == torch.int32 and crit.last_perm.tolist() == ([0, 1, 0] if pit == "utterance" else [0, 0, 0])
    # grad_scale through the C ABI against 3 x the gradient: each side rounds its weight and its product once (MAE: the
    # weight only), four roundings in all, 4 u + O(u^2) -> 5 u; SI-SNR rounds once per side, relative to the tensor's max
    s1, s2, _, _ = wavloss_pit_loss(kind, pit, *[v.detach() for v in t.values()], grad_scale=3.0)
    for a, b in ((s1, d1), (s2, d2)):
        a, b = a.double(), 3.0 * b.double()
        tol = 5 * U * b.abs() + TINY if kind != "sisnr" else 4 * U * b.abs().max()
        assert bool(torch.all((a - b).abs() <= tol))
    # non-contiguous inputs are made contiguous; mismatched shapes are refused with both shapes named
    nc = {k: torch.stack([v.detach(), v.detach()], dim=2)[:, :, 0] for k, v in t.items()}
    assert not nc["s1"].is_contiguous() and float(getattr(S, cls)(pit=pit)(**nc)["loss"]) == float(loss.detach())
    with pytest.raises(ValueError, match=r"\(3, 1024\).*\(3, 1025\)"):
        crit(**dict(nc, s2=nc["s2"][:, :1024]))
    with pytest.raises(ValueError, match=r"\(1025,\).*\(3, 1025\)"):
        crit(**dict(nc, s1=nc["s1"][0]))


@pytest.fixture(scope="module")
def trainer(dev):
    from oracle import convtasnet_stock as CT
    from speech_separation_amd import FusedAdamW, TrainableConvTasNet
    from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs
    m = TrainableConvTasNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CT.synthetic_convtasnet_weights(seed=0).items()}, strict=True)
    m = m.to(dev)
    inp = synthetic_inputs(DPTN_AUDIO, B=2, T=4000, seed=9)
    return m, FusedAdamW(m.parameters(), lr=1e-3), {k: torch.from_numpy(inp[k]).to(dev) for k in ("mix", "s1", "s2")}


@pytest.mark.parametrize("cls,pit", [("MAEWavLoss", "batch"), ("MAEWavLoss", "utterance"), ("MSEWavLoss", "batch"),
                                     ("MSEWavLoss", "utterance"), ("SiSNRWavLoss", "utterance")])
def test_training_step_runs_without_host_synchronisation(dev, trainer, cls, pit):
    """train.train_step of TrainableConvTasNet (B = 2 x T = 4000) with FusedAdamW under each new criterion: finite loss
    and gradient norm, the parameters move, and the step enqueues under torch's sync debug mode set to "error"."""
    from speech_separation_amd import train
    model, opt, batch = trainer
    crit = getattr(train, cls)(pit=pit)
    first = train.train_step(model, dict(batch), crit, opt, 10.0)                  # allocations happen here
    torch.cuda.synchronize()
    before = [p.detach().clone() for p in model.parameters()]
    torch.cuda.set_sync_debug_mode("error")
    try:
        stats = train.train_step(model, dict(batch), crit, opt, 10.0)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for s in (first, stats):
        assert s["loss"].device.type == "cuda" and np.isfinite(float(s["loss"]))
        assert np.isfinite(float(s["grad_norm"])) and float(s["grad_norm"]) > 0
    assert sum(int(not torch.equal(p.detach(), b)) for p, b in zip(model.parameters(), before)) > len(before) // 2


def test_argument_errors_launch_nothing(dev):
    from speech_separation_amd import _lib
    lib = _lib.load()
    B, T = 2, 8
    inp = [torch.from_numpy(a).to(dev) for a in R.make_case(B, T, seed=1)]
    need = int(lib.wavloss_scratch_bytes(B))
    d1, d2 = torch.full((B, T), 7.0, device=dev), torch.full((B, T), 7.0, device=dev)
    out, perm = torch.full((4,), 7.0, device=dev), torch.full((B,), 7, dtype=torch.int32, device=dev)
    ws = torch.full((need + 8,), 0x5A, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 8 == 0
    good = dict(kind=0, level=0, B=B, T=T, ws=ws.data_ptr(), ws_bytes=need)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for change in (dict(B=0), dict(T=0), dict(kind=7), dict(level=7), dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 4),
                   dict(kind=2, T=1)):
        a = dict(good, **change)
        rc = lib.wavloss_pit_loss(a["kind"], a["level"], *[t.data_ptr() for t in inp], a["B"], a["T"], 1.0, d1.data_ptr(),
                                  d2.data_ptr(), out.data_ptr(), perm.data_ptr(), a["ws"], a["ws_bytes"], stream)
        assert rc == 1, change                                       # WAVLOSS_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((d1 == 7).all()) and bool((d2 == 7).all()) and bool((out == 7).all()) and bool((perm == 7).all()), change
        assert bool((ws == 0x5A).all()), change
    assert lib.wavloss_pit_loss(0, 0, *[t.data_ptr() for t in inp], B, T, 1.0, d1.data_ptr(), d2.data_ptr(), out.data_ptr(),
                                perm.data_ptr(), ws.data_ptr(), need, stream) == 0
    torch.cuda.synchronize()
    assert not bool((d1 == 7).any()) and perm.tolist() == [0, 0]


def test_zz_worst_sisnr_ratio_is_reported():
    """The worst error / bound ratio the SI-SNR checks of this session saw (DESIGN.md section 18 quotes it)."""
    for k, v in sorted(WORST.items()):
        print(f"wavloss worst ratio {k}: {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
