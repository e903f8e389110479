"""DeepAVConvTasNet training step (speech_separation_amd.TrainableDeepAVConvTasNet, include/davctasnet_train.h) on the MI355X,
with the helpers and rules of tests/test_gpu_convtasnet_train.py: the grad-enabled forward is bitwise DeepAVConvTasNet's
inference forward; gradients -- the four tensors of the video head judged like any other -- agree with fp64 autograd of the
stock-PyTorch restatement (tests/deepavconvtasnet_train_ref.py) on the same PReLU branches as closely as the fp32 restatement
does (check_gradients); the tape's values, VCAT included; determinism, the fused and the stock training steps, no host
synchronisation, the rejected paths and guard-page memory safety.  Weights: 57 distinct PReLU slopes and a video LayerNorm
far from the identity (R.synthetic_weights).  Shapes (B, T, Tv), the smallest at which each mechanism can go wrong:

  (2, 16, 1)       F = 3    a single video row: every frame puts both interpolation weights on it
  (2, 100, 7)      F = 8    every d = 8 tap outside the sequence
  (3, 4001, 50)    F = 252  three mixtures, upsampling about 5 x
  (2, 400, 50)     F = 27   Tv > F: rows of vcat with zero gradient, the clamp src < 0 at f = 0
  (2, 4000, 252)   F = 252  Tv = F: lam = 0 everywhere

The B = 16 x 2 s gradient check and the timings live in tools/convtasnet_train_bench.py --model deepavconvtasnet."""
from __future__ import annotations

import ctypes
import os
import subprocess
import sys

import pytest
import torch

from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs
from tests import deepavconvtasnet_train_ref as R
from tests import hard_inputs as HI
from tests.test_gpu_convtasnet_train import _mix, _mse, check_gradients

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UNUSED = R.UNUSED
SHAPES = [(2, 16, 1), (2, 100, 7), (3, 4001, 50), (2, 400, 50), (2, 4000, 252)]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.backends.cudnn.allow_tf32 = False          # the fp32 / fp64 restatements on the GPU: plain fp32 arithmetic
    torch.backends.cuda.matmul.allow_tf32 = False
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def sd():
    return {k: torch.from_numpy(v) for k, v in R.synthetic_weights(seed=0).items()}


def _model(sd, dev):
    from speech_separation_amd import TrainableDeepAVConvTasNet
    m = TrainableDeepAVConvTasNet()
    m.load_state_dict(sd, strict=True)
    return m.to(dev)


def _emb(B, Tv, seed=0):
    return tuple(torch.from_numpy(e) for e in R.synthetic_embeddings(B, Tv, seed))


def _batch(B, T, Tv, dev, seed):
    inp = synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=seed)
    batch = {k: torch.from_numpy(inp[k]).to(dev) for k in ("mix", "s1", "s2")}
    batch["s1_embedding"], batch["s2_embedding"] = (e.to(dev) for e in _emb(B, Tv, seed))
    return batch


def test_forward_bitwise_equals_inference(dev, sd):
    from speech_separation_amd import DeepAVConvTasNet
    inf = DeepAVConvTasNet()
    inf.load_state_dict(sd, strict=True)
    inf = inf.to(dev)
    m = _model(sd, dev)
    for B, T, Tv in SHAPES + [(4, 32000, 50)]:
        mix = _mix(B, T).to(dev)
        e1, e2 = (e.to(dev) for e in _emb(B, Tv, seed=T))
        out = m(mix=mix, s1_embedding=e1, s2_embedding=e2)
        assert out["s1_pred"].requires_grad
        with torch.no_grad():
            want = inf(mix=mix, s1_embedding=e1, s2_embedding=e2)
            nog = m(mix=mix, s1_embedding=e1, s2_embedding=e2)      # no_grad: the inference engine
        for k in ("s1_pred", "s2_pred"):
            assert torch.equal(out[k].detach(), want[k]), (B, T, Tv, k)
            assert torch.equal(nog[k], want[k]), (B, T, Tv, k)


def _to(masks, rdev):
    return {k: [t.to(rdev) for t in v] if isinstance(v, list) else v.to(rdev) for k, v in masks.items()}


def _gradients_match_fp64(dev, sd, mix, e1, e2, what):
    B, T = mix.shape
    Tv = e1.shape[-1]
    m = _model(sd, dev)
    L = 16 * (T // 16)
    gen = torch.Generator().manual_seed(T)
    d1, d2 = torch.randn(B, L, generator=gen), torch.randn(B, L, generator=gen)
    mix, e1, e2, d1, d2 = (t.to(dev) for t in (mix, e1, e2, d1, d2))
    out = m(mix=mix, s1_embedding=e1, s2_embedding=e2)
    masks = _to(R.prelu_masks(m._engine, B, T, Tv), dev)
    torch.autograd.backward([out["s1_pred"], out["s2_pred"]], [d1, d2])
    sdr = {k: v.to(dev) for k, v in sd.items()}
    g64 = R.grads(sdr, mix, e1, e2, d1, d2, torch.float64, masks)
    g32 = R.grads(sdr, mix, e1, e2, d1, d2, torch.float32, masks)
    params = dict(m.named_parameters())
    assert params[UNUSED].grad is None and not g64[UNUSED].any()
    named = [(k, p.grad) for k, p in params.items() if k != UNUSED]
    assert len(named) == 375
    bad, worst, worst_x = check_gradients(named, g64, g32)
    print(f"{what} B={B} T={T} Tv={Tv}: worst per-tensor ratio {worst:.3g}, worst ratio / fp32 ratio {worst_x:.3g}")
    ratio = lambda g, ref: float((g.double() - ref).norm() / ref.norm())
    for k in R.VIDEO:
        print(f"  {k}: ratio {ratio(params[k].grad, g64[k]):.3g} (fp32 restatement {ratio(g32[k], g64[k]):.3g})")
        assert float(g64[k].norm()) > 0, k
    for k, g in named:
        assert torch.isfinite(g).all(), k
    assert not bad, f"{len(bad)} tensors off: {bad}"


@pytest.mark.parametrize("B,T,Tv", SHAPES[1:])
def test_gradients_match_fp64(dev, sd, B, T, Tv):
    """All 375 read parameters against fp64 autograd of the restatement on the same PReLU branches (check_gradients' rule:
    per tensor ratio < 1e-3 and <= 4 x max(the fp32 restatement's ratio, 1e-6))."""
    _gradients_match_fp64(dev, sd, _mix(B, T, seed=B + T), *_emb(B, Tv, seed=Tv), "distinct slopes")


def test_gradients_on_hard_inputs(dev, sd):
    """One batch of (plain, silent, padded, dc10) at T = 4000, Tv = 50: every gradient finite, the same rule."""
    _, mix = HI.hard_mixtures(4000, seed=3, names=("plain", "silent", "padded", "dc10"))
    _gradients_match_fp64(dev, sd, torch.from_numpy(mix), *_emb(4, 50, seed=4), "hard inputs")


def test_gradients_with_embeddings_scaled_per_mixture(dev, sd):
    """Mixture b's embeddings scaled by (1, 0, 10)[b]: mixture 1's vcat rows are the bare bias, its interpolated rows are
    constant along time; a vcat row read from the neighbouring mixture, in the recomputation or in the gather, would show."""
    e1, e2 = _emb(3, 50, seed=6)
    s = torch.tensor([1.0, 0.0, 10.0]).view(3, 1, 1)
    _gradients_match_fp64(dev, sd, _mix(3, 4001, seed=8), e1 * s, e2 * s, "scaled embeddings")


def test_tape_values_match_fp64(dev, sd):
    """VCAT, ENC_Z and DEC_Z of every dense layer, V1 and U of every block and SKIP against the same tensors of the
    restatement in fp64, at 3 x 4001 x 50: per tensor within 4 x max(the fp32 restatement's distance, 1e-6), as
    tests/test_gpu_deepconvtasnet_train.py."""
    B, T, Tv = 3, 4001, 50
    m = _model(sd, dev)
    mix = _mix(B, T, seed=77)
    e1, e2 = _emb(B, Tv, seed=78)
    m(mix=mix.to(dev), s1_embedding=e1.to(dev), s2_embedding=e2.to(dev))
    got = R.tape_tensors(m._engine, B, T, Tv)
    taps = {}
    with torch.no_grad():
        for dt in (torch.float64, torch.float32):
            taps[dt] = {}
            R.forward({k: v.to(dt) for k, v in sd.items()}, mix.to(dt), e1.to(dt), e2.to(dt), taps=taps[dt])
    flat = lambda d: ([(f"{n}[{i}]", t) for n in ("ez", "v1", "u", "dz") for i, t in enumerate(d[n])]
                      + [("skip", d["skip"]), ("vcat", d["vcat"])])
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


def test_determinism(dev, sd):
    from speech_separation_amd import SiSNRWavLoss
    m = _model(sd, dev)
    batch = _batch(2, 8000, 50, dev, seed=5)
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
    mix, e1, e2 = batch["mix"], batch["s1_embedding"], batch["s2_embedding"]
    s1, s2, tape = eng.train_forward(mix, e1, e2)
    assert tape[1:3] == (2, 8000) and tape[4] == 50   # Tv is part of the tape's identity
    d1, d2 = torch.randn_like(s1), torch.randn_like(s2)
    eng.train_backward(mix, e1, e2, d1, d2, tape)
    a = eng._grads_flat.clone()
    eng.train_backward(mix, e1, e2, d1, d2, tape)
    assert torch.equal(a, eng._grads_flat)
    with pytest.raises(RuntimeError, match="overwritten"):     # the same forward at another Tv is another tape
        eng.train_backward(mix, e1[..., :49], e2[..., :49], d1, d2, tape)


def test_train_steps_track_fp64_adamw(dev, sd):
    """Three train.train_step calls with FusedAdamW (lr 1e-3, fused clip 8.0) against three fp64 torch.optim.AdamW steps of
    the restatement: update ratio <= 4 x the fp32 restatement's + 1e-3.  decoder.deconv.weight keeps its value bit for bit
    (weight decay 0.01 included), as under torch.optim.AdamW with .grad None."""
    from speech_separation_amd import FusedAdamW, optim
    from speech_separation_amd.train import train_step
    m = _model(sd, dev)
    batch = _batch(2, 4000, 50, dev, seed=9)
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
                b = {k: v.to(dt) for k, v in batch.items()}
                out = R.forward(ref, b["mix"], b["s1_embedding"], b["s2_embedding"])
                _mse(**b, **out)["loss"].backward()
                torch.nn.utils.clip_grad_norm_([p for p in ref.values() if p.grad is not None], 8.0)
                ropts[dt].step()
    finally:
        type(m._engine).grad_clip = orig
    assert clipped == [8.0] * 3                       # the fused clip ran every step
    params = dict(m.named_parameters())
    assert torch.equal(params[UNUSED].detach().cpu(), sd[UNUSED])
    assert torch.equal(refs[torch.float32][UNUSED].detach().cpu(), sd[UNUSED])      # what stock AdamW does
    keys = [k for k in params]
    delta = lambda ps, ks: torch.cat([(ps[k].detach().double() - sd[k].to(dev).double()).reshape(-1) for k in ks])
    d, d64, d32 = (delta(ps, keys) for ps in (params, refs[torch.float64], refs[torch.float32]))
    r, r32 = float((d - d64).norm() / d64.norm()), float((d32 - d64).norm() / d64.norm())
    print(f"3 AdamW steps: update ratio {r:.3g} (fp32 restatement {r32:.3g})")
    assert r <= 4 * r32 + 1e-3
    assert float(delta(params, R.VIDEO).norm()) > 0   # the video head trains


def test_stock_optimizer_and_no_host_sync(dev, sd):
    from speech_separation_amd import FusedAdamW
    from speech_separation_amd.train import train_step
    batch = _batch(2, 4000, 50, dev, seed=13)
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
    m = _model(sd, dev)
    mix = _mix(2, 400).to(dev)
    e1, e2 = (e.to(dev) for e in _emb(2, 5))
    out = m(mix=mix, s1_embedding=e1, s2_embedding=e2)
    eng = m._engine
    # the C boundary: NULL embeddings and Tv = 0
    ws = eng._ws
    s = torch.empty(2, 400, device=dev)
    call = lambda p1, p2, Tv: lib.davtrain_train_forward(eng._h, mix.data_ptr(), p1, p2, 2, 400, Tv, s.data_ptr(), s.data_ptr(),
                                                         ws.data_ptr(), ws.numel(), eng._stream())
    assert call(None, e2.data_ptr(), 5) == 1 and b"embeddings" in lib.davtrain_last_error(eng._h)
    assert call(e1.data_ptr(), None, 5) == 1 and b"embeddings" in lib.davtrain_last_error(eng._h)
    assert call(e1.data_ptr(), e2.data_ptr(), 0) == 1 and b"Tv must be >= 1" in lib.davtrain_last_error(eng._h)
    assert lib.davtrain_workspace_bytes(eng._h, 2, 400, 0) == 0
    bwd = lib.davtrain_train_backward(eng._h, mix.data_ptr(), None, None, 2, 400, 5, s.data_ptr(), s.data_ptr(), ws.data_ptr(),
                                      ws.numel(), eng._stream())
    assert bwd == 1 and b"embeddings" in lib.davtrain_last_error(eng._h)
    # the module: missing / empty embeddings, an embedding that asks for a gradient
    with pytest.raises(ValueError, match="needs s1_embedding and s2_embedding"):
        m(mix=mix, s1_embedding=e1, s2_embedding=None)
    with pytest.raises(RuntimeError, match="Tv must be >= 1"):
        m(mix=mix, s1_embedding=e1[..., :0], s2_embedding=e2[..., :0])
    with pytest.raises(NotImplementedError, match="s2_embedding"):
        m(mix=mix, s1_embedding=e1, s2_embedding=e2.clone().requires_grad_(True))
    # none of the refused calls touched the tape: the first forward's backward still runs
    (out["s1_pred"].sum() + out["s2_pred"].sum()).backward()
    out = m(mix=mix, s1_embedding=e1, s2_embedding=e2)
    m(mix=mix, s1_embedding=e1, s2_embedding=e2)      # a later forward overwrites the tape
    with pytest.raises(RuntimeError, match="overwritten"):
        (out["s1_pred"].sum() + out["s2_pred"].sum()).backward()


def test_memory_safety():
    """Poisoned workspace, then every buffer flush against an unmapped page at its end, then at its start
    (tests/davctasnet_train_memsafety_child.py): one child process per mode; each result equals the plain run."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for mode in ("poison", "guard_end", "guard_start"):
        r = subprocess.run([sys.executable, "-m", "tests.davctasnet_train_memsafety_child", mode], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, f"{mode}: child ended with code {r.returncode}\n{r.stdout[-3000:]}"
        assert f"OK {mode} davtrain" in r.stdout, r.stdout[-3000:]
