"""DeepConvTasNet training step (speech_separation_amd.TrainableDeepConvTasNet, include/dctasnet_train.h) on the MI355X,
with the helpers and rules of tests/test_gpu_convtasnet_train.py: the grad-enabled forward is bitwise DeepConvTasNet's
inference forward; gradients agree with fp64 autograd of the stock-PyTorch restatement (tests/deepconvtasnet_train_ref.py)
on the same PReLU branches as closely as the fp32 restatement does (check_gradients); the tape's values; the loss path,
determinism, the fused and the stock training steps (decoder.deconv.weight, which the forward never reads, keeps .grad None
and its value), no host synchronisation, the rejected paths and guard-page memory safety.  The B = 16 x 2 s gradient check
and the timings live in tools/convtasnet_train_bench.py --model deepconvtasnet."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import pytest
import torch

from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs
from tests import deepconvtasnet_ref as D
from tests import deepconvtasnet_train_ref as R
from tests import hard_inputs as HI
from tests.test_gpu_convtasnet_train import _mix, _mse, check_gradients

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNUSED = R.UNUSED


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False          # the fp32 / fp64 restatements on the GPU: plain fp32 arithmetic
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return {k: torch.from_numpy(v) for k, v in D.synthetic_deepconvtasnet_weights(False, seed=0).items()}


@pytest.fixture(scope="module")
def sd_slopes():
    return {k: torch.from_numpy(v) for k, v in D.synthetic_deepconvtasnet_weights(False, seed=0, slopes="distinct").items()}


def _model(sd, dev):
    from speech_separation_amd import TrainableDeepConvTasNet
    m = TrainableDeepConvTasNet()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


@pytest.mark.parametrize("slopes", ["0.25", "distinct"])
def test_forward_bitwise_equals_inference(dev, sd, sd_slopes, slopes):
    """F = 3 (2 x 16), F = 8 (2 x 100: every d = 8 tap falls outside the sequence), an odd length, and the benchmark's frame
    count.  With distinct slopes a loader that applies another layer's PReLU slope no longer reproduces the inference."""
    from speech_separation_amd import DeepConvTasNet
    w = sd if slopes == "0.25" else sd_slopes
    inf = DeepConvTasNet()
    inf.load_state_dict(w, strict=True)
    inf = inf.to(dev)
    m = _model(w, dev)
    for B, T in ((2, 16), (2, 100), (2, 4001), (4, 32000)):
        mix = _mix(B, T).to(dev)
        out = m(mix=mix)
        assert out["s1_pred"].requires_grad
        with torch.no_grad():
            want = inf(mix=mix)
            nog = m(mix=mix)                          # no_grad: the inference engine
        for k in ("s1_pred", "s2_pred"):
            assert torch.equal(out[k].detach(), want[k]), (B, T, k)
            assert torch.equal(nog[k], want[k]), (B, T, k)


def _to(masks, rdev):
    return {k: [t.to(rdev) for t in v] if isinstance(v, list) else v.to(rdev) for k, v in masks.items()}


def _gradients_match_fp64(dev, sd, mix, what):
    B, T = mix.shape
    m = _model(sd, dev)
    L = 16 * (T // 16)
    gen = torch.Generator().manual_seed(T)
    d1, d2 = torch.randn(B, L, generator=gen), torch.randn(B, L, generator=gen)
    out = m(mix=mix.to(dev))
    masks = _to(R.prelu_masks(m._engine, B, T), dev)
    torch.autograd.backward([out["s1_pred"], out["s2_pred"]], [d1.to(dev), d2.to(dev)])
    sdr = {k: v.to(dev) for k, v in sd.items()}
    g64 = R.grads(sdr, mix.to(dev), d1.to(dev), d2.to(dev), torch.float64, masks)
    g32 = R.grads(sdr, mix.to(dev), d1.to(dev), d2.to(dev), torch.float32, masks)
    params = dict(m.named_parameters())
    assert params[UNUSED].grad is None and not g64[UNUSED].any()
    named = [(k, p.grad) for k, p in params.items() if k != UNUSED]
    bad, worst, worst_x = check_gradients(named, g64, g32)
    print(f"{what} B={B} T={T}: worst per-tensor ratio {worst:.3g}, worst ratio / fp32 ratio {worst_x:.3g}")
    for k, g in named:
        assert torch.isfinite(g).all(), k
    assert not bad, f"{len(bad)} tensors off: {bad}"


@pytest.mark.parametrize("B,T", [(2, 100), (2, 4000), (3, 4001)])
def test_gradients_match_fp64_distinct_slopes(dev, sd_slopes, B, T):
    """Against fp64 autograd of the restatement on the same PReLU branches (check_gradients' rule), 57 distinct slopes.
    B = 3: a tap that read a neighbouring mixture's rows, or on the decoder's 2M rows the other speaker's, would show.
    2 x 100: F = 8, the d = 8 layers have only their centre tap."""
    _gradients_match_fp64(dev, sd_slopes, _mix(B, T, seed=B + T), "distinct slopes")


def test_gradients_match_fp64(dev, sd):
    _gradients_match_fp64(dev, sd, _mix(2, 4000, seed=4002), "slopes 0.25")


def test_gradients_on_hard_inputs(dev, sd_slopes):
    """One batch of (plain, silent, padded, dc10) at T = 4000, distinct slopes: every gradient finite, the same rule."""
    _, mix = HI.hard_mixtures(4000, seed=3, names=("plain", "silent", "padded", "dc10"))
    _gradients_match_fp64(dev, sd_slopes, torch.from_numpy(mix), "hard inputs, distinct slopes")


def test_tape_values_match_fp64(dev, sd_slopes):
    """ENC_Z and DEC_Z of every dense layer, V1 and U of every block and SKIP against the same tensors of the restatement in
    fp64, at 3 x 4001: per tensor within 4 x max(the fp32 restatement's distance, 1e-6), as
    tests/test_gpu_convtasnet_train.py."""
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
    flat = lambda d: ([(f"{n}[{i}]", t) for n in ("ez", "v1", "u", "dz") for i, t in enumerate(d[n])] + [("skip", d["skip"])])
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


def test_loss_path_and_determinism(dev, sd_slopes):
    from speech_separation_amd import SiSNRWavLoss
    m = _model(sd_slopes, dev)
    inp = synthetic_inputs(DPTN_AUDIO, B=2, T=8000, seed=5)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("mix", "s1", "s2")}
    crit = SiSNRWavLoss()
    flats = []
    for _ in range(2):
        m.zero_grad()
        out = m(**batch)
        crit(**batch, **out)["loss"].backward()
        flats.append(m._flat_grad.clone())
    assert torch.equal(flats[0], flats[1])           # bitwise-identical gradients, call after call: no atomics
    eng = m._engine
    for k, p in m.named_parameters():
        o = eng._grad_offsets[k]
        if k == UNUSED:
            assert p.grad is None and not flats[0][o:o + p.numel()].any()      # zero in the clip norm
        else:
            assert p.grad.data_ptr() == m._flat_grad.data_ptr() + 4 * o, k
    # two backward calls on ONE tape
    mix = batch["mix"]
    s1, s2, tape = eng.train_forward(mix)
    d1, d2 = torch.randn_like(s1), torch.randn_like(s2)
    eng.train_backward(mix, d1, d2, tape)
    a = eng._grads_flat.clone()
    eng.train_backward(mix, d1, d2, tape)
    assert torch.equal(a, eng._grads_flat)


def test_train_steps_track_fp64_adamw(dev, sd_slopes):
    """Three train.train_step calls with FusedAdamW (lr 1e-3, fused clip 8.0) against three fp64 torch.optim.AdamW steps of
    the restatement: update ratio <= 4 x the fp32 restatement's + 1e-3.  The backward packs the dense weights anew in every
    step; a stale copy would show in steps 2 and 3.  decoder.deconv.weight keeps its value bit for bit (weight decay 0.01
    included), as under torch.optim.AdamW with .grad None."""
    from speech_separation_amd import FusedAdamW, optim
    from speech_separation_amd.train import train_step
    sd = sd_slopes
    m = _model(sd, dev)
    inp = synthetic_inputs(DPTN_AUDIO, B=2, T=4000, seed=9)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("mix", "s1", "s2")}
    opt = FusedAdamW(m.parameters(), lr=1e-3)
    assert opt.param_groups[0]["weight_decay"] == 0.01
    clipped = []
    orig = type(m._get_engine(dev)).grad_clip

    def spy(self, flat, mx):
        clipped.append(mx)
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
                _mse(**{k: v.to(dt) for k, v in batch.items()}, **out)["loss"].backward()
                torch.nn.utils.clip_grad_norm_([p for p in ref.values() if p.grad is not None], 8.0)
                ropts[dt].step()
    finally:
        type(m._engine).grad_clip = orig
    assert clipped == [8.0] * 3                       # the fused clip ran every step
    params = dict(m.named_parameters())
    assert torch.equal(params[UNUSED].detach().cpu(), sd[UNUSED])
    assert torch.equal(refs[torch.float32][UNUSED].detach().cpu(), sd[UNUSED])      # what stock AdamW does
    keys = [k for k in params]
    delta = lambda ps: torch.cat([(ps[k].detach().double() - sd[k].to(dev).double()).reshape(-1) for k in keys])
    d, d64, d32 = delta(params), delta(refs[torch.float64]), delta(refs[torch.float32])
    r, r32 = float((d - d64).norm() / d64.norm()), float((d32 - d64).norm() / d64.norm())
    print(f"distinct slopes: 3 AdamW steps: update ratio {r:.3g} (fp32 restatement {r32:.3g})")
    assert r <= 4 * r32 + 1e-3


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
    torch.nn.utils.clip_grad_norm_([p for p in a.parameters() if p.grad is not None], 8.0)
    oa.step()
    train_step(b, dict(batch), _mse, ob, max_grad_norm=8.0)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), k
    for mdl in (a, b):
        assert torch.equal(dict(mdl.named_parameters())[UNUSED].detach().cpu(), sd[UNUSED])
    # a full fused step enqueues everything without a host synchronisation
    train_step(b, dict(batch), _mse, ob, max_grad_norm=8.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = train_step(b, dict(batch), _mse, ob, max_grad_norm=8.0)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(r["loss"]) and torch.isfinite(r["grad_norm"])


def test_rejected_paths(dev, sd):
    from speech_separation_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    assert lib.dcttrain_create(ctypes.byref(h), 1) == 1 and not h.value
    assert b"audio-visual training step" in lib.dcttrain_last_error(None) and b"not built" in lib.dcttrain_last_error(None)
    m = _model(sd, dev)
    mix = _mix(2, 400).to(dev)
    out = m(mix=mix)
    m(mix=mix)                                        # a later forward overwrites the tape
    with pytest.raises(RuntimeError, match="overwritten"):
        (out["s1_pred"].sum() + out["s2_pred"].sum()).backward()


def test_memory_safety():
    """Poisoned workspace, then every buffer flush against an unmapped page at its end, then at its start
    (tests/ctasnet_train_memsafety_child.py): one child process per mode; each result equals the plain run."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for mode in ("poison", "guard_end", "guard_start"):
        r = subprocess.run([sys.executable, "-m", "tests.ctasnet_train_memsafety_child", mode, "dcttrain"], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, f"{mode}: child ended with code {r.returncode}\n{r.stdout[-3000:]}"
        assert f"OK {mode} dcttrain" in r.stdout, r.stdout[-3000:]
