"""Conv-TasNet training step (speech_separation_amd.TrainableConvTasNet, include/ctasnet_train.h) on the MI355X: the
grad-enabled forward is bitwise ConvTasNet's inference forward; gradients agree with fp64 autograd of the stock-PyTorch
restatement (tests/convtasnet_train_ref.py) as closely as the fp32 restatement does; the loss path, the fused and the stock
training steps, determinism, no host synchronisation and guard-page memory safety.  The same with 49 DISTINCT PReLU slopes
(`sd_slopes`: with one common slope no test can tell which slope a kernel read, and TAPE mode applies each slope in its
consumers), the values on the tape against fp64 block by block, and forward and gradients on hard input values
(tests/hard_inputs.py: silence, zero padding, a DC offset).  The B = 16 x 4 s gradient check and the timings live in
tools/convtasnet_train_bench.py."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import convtasnet_stock as CT
from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs
from tests import convtasnet_train_ref as R
from tests import hard_inputs as HI

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False          # the fp32 / fp64 restatements on the GPU: plain fp32 arithmetic
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return {k: torch.from_numpy(v) for k, v in CT.synthetic_convtasnet_weights(seed=0).items()}


@pytest.fixture(scope="module")
def sd_slopes():
    return {k: torch.from_numpy(v) for k, v in CT.synthetic_convtasnet_weights(seed=0, slopes="distinct").items()}


def _model(sd, dev):
    from speech_separation_amd import TrainableConvTasNet
    m = TrainableConvTasNet()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def _mix(B, T, seed=21):
    return torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=seed)["mix"])


def _ratio(g, ref):
    n = float(ref.norm())
    return float((g.double() - ref).norm()) / n if n > 0 else float(g.norm())


def _forward_bitwise_equals_inference(dev, sd):
    from speech_separation_amd import ConvTasNet
    inf = ConvTasNet()
    inf.load_state_dict(sd, strict=True)
    inf = inf.to(dev)
    m = _model(sd, dev)
    for B, T in ((4, 32000), (2, 16), (2, 4001), (2, 12345)):
        mix = _mix(B, T).to(dev)
        out = m(mix=mix)
        assert out["s1_pred"].requires_grad
        with torch.no_grad():
            want = inf(mix=mix)
            nog = m(mix=mix)                          # no_grad: the inference engine
        for k in ("s1_pred", "s2_pred"):
            assert torch.equal(out[k].detach(), want[k]), (B, T, k)
            assert torch.equal(nog[k], want[k]), (B, T, k)


def test_forward_bitwise_equals_inference(dev, sd):
    _forward_bitwise_equals_inference(dev, sd)


def test_forward_bitwise_equals_inference_distinct_slopes(dev, sd_slopes):
    """The tape holds pre-activations, so in the training forward PReLU_1 is applied by the depthwise conv on load and
    PReLU_2 by the res|skip GEMM on load, each with a slope pointer of its own: with distinct slopes a consumer that reads
    another PReLU's slope no longer reproduces the inference forward."""
    _forward_bitwise_equals_inference(dev, sd_slopes)


def check_gradients(named_grads, g64, g32):
    """-> (list of (key, ratio, fp32 ratio) off the bound, worst ratio, worst ratio / fp32 ratio).  Both restatements
    follow this implementation's PReLU branches (R.prelu_masks), so the fp32 restatement's distance to fp64 is the
    rounding noise of the same operations.  Per tensor: ||g - g64|| / ||g64|| < 1e-3 and <= 4 x max(fp32 ratio, 1e-6) (the
    floor is a few fp32 ulps); exactly zero where g64 is zero.  The 49 PReLU slopes are each ONE sum over every activation
    of a layer, whose rounding depends on the summation order alone, so they are judged as one vector the same way; the
    slope whose gradient is furthest off is printed by name (error over the norm of the vector, next to the fp32
    restatement's for the same slope), so that when the vector fails the wrong slope is named."""
    bad, worst, worst_x = [], 0.0, 0.0

    def judge(k, g, ref, ref32):
        nonlocal worst, worst_x
        n = float(ref.norm())
        r, r32 = float((g - ref).norm()), float((ref32 - ref).norm())
        if n == 0.0:
            if r != 0.0:
                bad.append((k, r, r32))
            return
        r, r32 = r / n, r32 / n
        worst, worst_x = max(worst, r), max(worst_x, r / max(r32, 1e-6))
        if not (r < 1e-3 and r <= 4 * max(r32, 1e-6)):
            bad.append((k, r, r32))

    slopes = [k for k, g in named_grads if g.numel() == 1]
    for k, g in named_grads:
        if g.numel() > 1:
            judge(k, g.cpu().double(), g64[k].cpu(), g32[k].cpu().double())
    grads = dict(named_grads)
    cat = lambda d, f: torch.cat([f(d[k]).reshape(-1) for k in slopes])
    v, v64, v32 = cat(grads, lambda t: t.cpu().double()), cat(g64, lambda t: t.cpu()), cat(g32, lambda t: t.cpu().double())
    judge("PReLU slopes", v, v64, v32)
    n = max(float(v64.norm()), 1e-300)
    i = int((v - v64).abs().argmax())
    print(f"PReLU slopes: worst {slopes[i]}: |g - g64| / ||g64 of all slopes|| = {float((v - v64)[i].abs()) / n:.3g} "
          f"(fp32 restatement, same slope: {float((v32 - v64)[i].abs()) / n:.3g}); g = {float(v[i]):.6g}, g64 = {float(v64[i]):.6g}")
    return bad, worst, worst_x


def _gradients_match_fp64(dev, sd, mix, on_gpu_ref, what):
    B, T = mix.shape
    m = _model(sd, dev)
    L = 16 * (T // 16)
    gen = torch.Generator().manual_seed(T)
    d1, d2 = torch.randn(B, L, generator=gen), torch.randn(B, L, generator=gen)
    out = m(mix=mix.to(dev))
    rdev = dev if on_gpu_ref else torch.device("cpu")
    masks = R.prelu_masks(m._engine, B, T)
    masks = {k: [t.to(rdev) for t in v] if isinstance(v, list) else v.to(rdev) for k, v in masks.items()}
    torch.autograd.backward([out["s1_pred"], out["s2_pred"]], [d1.to(dev), d2.to(dev)])
    sdr = {k: v.to(rdev) for k, v in sd.items()}
    g64 = R.grads(sdr, mix.to(rdev), d1.to(rdev), d2.to(rdev), torch.float64, masks)
    g32 = R.grads(sdr, mix.to(rdev), d1.to(rdev), d2.to(rdev), torch.float32, masks)
    bad, worst, worst_x = check_gradients([(k, p.grad) for k, p in m.named_parameters()], g64, g32)
    print(f"{what} B={B} T={T}: worst per-tensor ratio {worst:.3g}, worst ratio / fp32 ratio {worst_x:.3g}")
    for k, p in m.named_parameters():
        assert torch.isfinite(p.grad).all(), k
    assert not bad, f"{len(bad)} tensors off: {bad}"


@pytest.mark.parametrize("B,T,on_gpu_ref", [(2, 4000, False), (3, 12345, False), (4, 32000, True)])
def test_gradients_match_fp64(dev, sd, B, T, on_gpu_ref):
    """Against fp64 autograd of the restatement on the same PReLU branches, as close as the fp32 restatement is
    (check_gradients)."""
    _gradients_match_fp64(dev, sd, _mix(B, T, seed=B + T), on_gpu_ref, "slopes 0.25")


@pytest.mark.parametrize("B,T", [(2, 4000), (3, 12345)])
def test_gradients_match_fp64_distinct_slopes(dev, sd_slopes, B, T):
    """The same with 49 distinct slopes (one 0.0, one 1.0, negative ones, some above 1): the backward reads each slope in
    several launches, and the fp64 reference takes only the BRANCHES from the tape, the slope values from the state dict."""
    _gradients_match_fp64(dev, sd_slopes, _mix(B, T, seed=B + T), False, "distinct slopes")


def test_gradients_on_hard_inputs(dev, sd_slopes):
    """One batch of (plain, silent, padded, dc10) at T = 4000, distinct slopes.  The silent mixture has zero encoder
    variance, so GlobalNorm's backward runs at rstd = 1 / sqrt(eps); every gradient must be finite, and check_gradients'
    rules are those of every other case (measured: worst per-tensor ratio 2.1e-6, 1.5 x the fp32 restatement's)."""
    _, mix = HI.hard_mixtures(4000, seed=3, names=("plain", "silent", "padded", "dc10"))
    _gradients_match_fp64(dev, sd_slopes, torch.from_numpy(mix), False, "hard inputs, distinct slopes")


def test_loss_path_and_determinism(dev, sd):
    from speech_separation_amd import SiSNRWavLoss
    m = _model(sd, dev)
    inp = synthetic_inputs(DPTN_AUDIO, B=2, T=8000, seed=5)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("mix", "s1", "s2")}
    crit = SiSNRWavLoss()
    flats = []
    for _ in range(2):
        m.zero_grad()
        out = m(**batch)
        loss = crit(**batch, **out)["loss"]
        loss.backward()
        flats.append(m._flat_grad.clone())
    assert torch.equal(flats[0], flats[1])           # bitwise-identical gradients, call after call
    for k, p in m.named_parameters():
        o = m._engine._grad_offsets[k]
        assert p.grad.data_ptr() == m._flat_grad.data_ptr() + 4 * o, k
    # the same gradients through an explicit upstream gradient
    out = m(**batch)
    d1, d2 = torch.autograd.grad(crit(**batch, **out)["loss"], [out["s1_pred"], out["s2_pred"]], retain_graph=True)
    g = torch.autograd.grad([out["s1_pred"], out["s2_pred"]], list(m.parameters()), [d1, d2])
    got = torch.cat([x.reshape(-1) for x in g])
    want = torch.cat([p.grad.reshape(-1) for p in m.parameters()])
    assert torch.equal(got, want)


def _mse(**b):
    return {"loss": ((b["s1_pred"] - b["s1"][:, :b["s1_pred"].shape[1]]) ** 2).mean()
            + ((b["s2_pred"] - b["s2"][:, :b["s2_pred"].shape[1]]) ** 2).mean()}


def _train_steps_track_fp64_adamw(dev, sd, what):
    from speech_separation_amd import FusedAdamW, optim
    from speech_separation_amd.train import train_step
    m = _model(sd, dev)
    inp = synthetic_inputs(DPTN_AUDIO, B=2, T=4000, seed=9)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("mix", "s1", "s2")}
    opt = FusedAdamW(m.parameters(), lr=1e-3)
    eng_clip = []
    orig = type(m._get_engine(dev)).grad_clip

    def spy(self, flat, mx):
        eng_clip.append(mx)
        return orig(self, flat, mx)

    refs = {dt: {k: v.to(dev, dt).clone().requires_grad_(True) for k, v in sd.items()} for dt in (torch.float64, torch.float32)}
    ropts = {dt: torch.optim.AdamW(list(r.values()), lr=1e-3) for dt, r in refs.items()}
    type(m._engine).grad_clip = spy
    try:
        for _ in range(3):
            train_step(m, dict(batch), _mse, opt, max_grad_norm=8.0)
            assert optim.flat_grad_or_none(m) is not None
            for dt, ref in refs.items():
                ropts[dt].zero_grad()
                out = R.forward(ref, batch["mix"].to(dt))
                loss = _mse(**{k: v.to(dt) for k, v in batch.items()}, **out)["loss"]
                loss.backward()
                torch.nn.utils.clip_grad_norm_(list(ref.values()), 8.0)
                ropts[dt].step()
    finally:
        type(m._engine).grad_clip = orig
    assert eng_clip == [8.0] * 3                      # the fused clip ran every step
    # the parameter updates, against fp64; AdamW normalises noisy near-zero gradients to lr-sized steps, so the fp32
    # restatement's distance is the yardstick again
    keys = [k for k, _ in m.named_parameters()]
    delta = lambda ps: torch.cat([(ps[k].detach().double() - sd[k].to(dev).double()).reshape(-1) for k in keys])
    d, d64, d32 = delta(dict(m.named_parameters())), delta(refs[torch.float64]), delta(refs[torch.float32])
    r, r32 = float((d - d64).norm() / d64.norm()), float((d32 - d64).norm() / d64.norm())
    print(f"{what}: 3 AdamW steps: update ratio {r:.3g} (fp32 restatement {r32:.3g})")
    assert r <= 4 * r32 + 1e-3


def test_train_steps_track_fp64_adamw(dev, sd):
    """Three train.train_step calls with FusedAdamW (fused clip) against three fp64 torch.optim.AdamW steps of the
    restatement: a stale weight copy anywhere would show in steps 2 and 3."""
    _train_steps_track_fp64_adamw(dev, sd, "slopes 0.25")


def test_train_steps_track_fp64_adamw_distinct_slopes(dev, sd_slopes):
    _train_steps_track_fp64_adamw(dev, sd_slopes, "distinct slopes")


def test_tape_values_match_fp64(dev, sd_slopes):
    """TAPE_V1 and TAPE_U of every block and TAPE_SKIP (cttrain_tape_offset, eng.tape_tensor) against the same tensors of the
    restatement in fp64: VALUES, where the gradient check uses the tape's signs only.  Errors grow through 24 residual
    blocks, so the bound per tensor is no fixed figure: it is the distance of the fp32 restatement's same tensor from fp64,
    times the factor 4 of check_gradients, with the same 1e-6 relative floor.  A failure names the block and the stage."""
    B, T = 3, 4001
    m = _model(sd_slopes, dev)
    mix = _mix(B, T, seed=77)
    m(mix=mix.to(dev))
    got = R.tape_tensors(m._engine, B, T)
    taps = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            taps[dt] = {}
            R.forward({k: v.to(dt) for k, v in sd_slopes.items()}, mix.to(dt), taps=taps[dt])
    flat = lambda d: [(f"v1[{i}]", t) for i, t in enumerate(d["v1"])] + [(f"u[{i}]", t) for i, t in enumerate(d["u"])] + [
        ("skip", d["skip"])]
    bad, worst = [], (0.0, "", 0.0, 0.0)
    for (name, g), (_, t64), (_, t32) in zip(flat(got), flat(taps[torch.float64]), flat(taps[torch.float32])):
        assert g.shape == t64.shape, (name, g.shape, t64.shape)
        n = float(t64.norm())
        assert n > 0 and torch.isfinite(g).all(), name
        r, r32 = float((g.cpu().double() - t64).norm()) / n, float((t32.double() - t64).norm()) / n
        x = r / max(r32, 1e-6)
        if x > worst[0]:
            worst = (x, name, r, r32)
        if not r <= 4 * max(r32, 1e-6):
            bad.append((name, r, r32))
    print(f"tape values: worst {worst[1]}: ratio {worst[2]:.3g}, fp32 restatement {worst[3]:.3g}, ratio / max(fp32 ratio, "
          f"1e-6) = {worst[0]:.3g}")
    assert not bad, f"{len(bad)} tape tensors off (name, ratio, fp32 restatement's ratio): {bad}"


def test_training_forward_on_hard_inputs(dev, sd_slopes):
    """The grad-enabled forward on the nine mixtures of tests/hard_inputs.py in one batch (T = 4001, distinct slopes): bitwise
    the inference forward, and judged per mixture and per frame against fp64 as in tests/test_gpu_ctasnet_values.py."""
    from speech_separation_amd import ConvTasNet
    names, mix = HI.hard_mixtures(4001, seed=0)
    inf = ConvTasNet()
    inf.load_state_dict(sd_slopes, strict=True)
    inf = inf.to(dev)
    m = _model(sd_slopes, dev)
    out = m(mix=torch.from_numpy(mix).to(dev))
    assert out["s1_pred"].requires_grad
    with torch.no_grad():
        want = inf(mix=torch.from_numpy(mix).to(dev))
    for k in ("s1_pred", "s2_pred"):
        assert torch.equal(out[k].detach(), want[k]), k
    got = {k: out[k].detach().cpu().numpy() for k in ("s1_pred", "s2_pred")}
    ref = {dt: {k: v.numpy() for k, v in CT.forward({k: v.to(dt) for k, v in sd_slopes.items()},
                                                    torch.from_numpy(mix).to(dt)).items()}
           for dt in (torch.float64, torch.float32)}
    bad = HI.check_batch("training forward", names, got, ref[torch.float64], ref[torch.float32], 90.0, exact_zero=("silent",))
    assert not bad, bad


def test_stock_optimizer_and_no_host_sync(dev, sd):
    from speech_separation_amd import FusedAdamW
    from speech_separation_amd.train import train_step
    inp = synthetic_inputs(DPTN_AUDIO, B=2, T=4000, seed=13)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("mix", "s1", "s2")}
    # stock torch.optim.AdamW + torch's clip on the same model gives the fused step's parameters
    a, b = _model(sd, dev), _model(sd, dev)
    oa, ob = torch.optim.AdamW(a.parameters(), lr=1e-3), FusedAdamW(b.parameters(), lr=1e-3)
    a.zero_grad()
    _mse(**batch, **a(**batch))["loss"].backward()
    torch.nn.utils.clip_grad_norm_(list(a.parameters()), 8.0)
    oa.step()
    train_step(b, dict(batch), _mse, ob, max_grad_norm=8.0)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), k
    # a full fused step enqueues everything without a host synchronisation
    train_step(b, dict(batch), _mse, ob, max_grad_norm=8.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = train_step(b, dict(batch), _mse, ob, max_grad_norm=8.0)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(r["loss"]) and torch.isfinite(r["grad_norm"])


def test_memory_safety():
    """Poisoned workspace, then every buffer flush against an unmapped page at its end, then at its start
    (tests/ctasnet_train_memsafety_child.py): one child process per mode; each result equals the plain run."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for mode in ("poison", "guard_end", "guard_start"):
        r = subprocess.run([sys.executable, "-m", "tests.ctasnet_train_memsafety_child", mode, "cttrain"], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, f"{mode}: child ended with code {r.returncode}\n{r.stdout[-3000:]}"
        assert f"OK {mode} cttrain" in r.stdout, r.stdout[-3000:]
