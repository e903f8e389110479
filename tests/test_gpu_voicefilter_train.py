"""The VoiceFilter training step (include/vfilt_train.h, TrainableVoiceFilter) on the MI355X.

Gradients: the project's rule unchanged (check_gradients of tests/test_gpu_convtasnet_train.py): per tensor
r = ||g - g64|| / ||g64|| < 1e-3 and r <= 4 max(r32, 1e-6), exactly zero where the fp64 gradient is exactly zero.  g64 / g32
are fp64 / fp32 CPU autograd of tests/voicefilter_train_ref.py, both given this implementation's dropout keep mask and ReLU
keep masks from the tape (as the Conv-TasNet kit does with PReLU branches).  The eight conv biases sit in front of a
batch-statistics BatchNorm: their gradient is mathematically zero, autograd returns rounding noise there (the host test
pins that on the reference's own run), the library writes exact zeros, and that is what is asserted for them; the other 50
trainable tensors go through check_gradients, none left out.

Values: per (item, speaker, frame) column, at most 2 x the fp32 CPU run's own distance to fp64 (the rule of
tests/test_gpu_voicefilter.py).  Every figure is printed before it is asserted.

Shapes (F, W, Tv, B): (17, 7, 1, 3): F below the reach of dilations 8 and 16, W below the 7-tap width, one GRU step,
B F W = 357 fills no chunk; (33, 50, 3, 1): B = 1 statistics, more than one chunk of 1024; (40, 33, 4, 2); (201, 21, 5, 2):
the real feature size, more than one chunk of 4096.  E = 1024, and 512 once."""
from __future__ import annotations

import ctypes
import os

import numpy as np
import pytest
import torch

from tests import voicefilter_ref as R
from tests import voicefilter_train_ref as T
from tests.test_gpu_convtasnet_train import check_gradients

pytestmark = pytest.mark.gpu
SHAPES = ((17, 7, 1, 3), (33, 50, 3, 1), (40, 33, 4, 2), (201, 21, 5, 2))
# (17, 9, 2, 5): 2B = 10 sequences, so the LSTM's step kernels (eight sequences per workgroup) run a second, partly filled group
CASES = [(s, 1024) for s in SHAPES] + [((33, 50, 3, 1), 512), ((17, 9, 2, 5), 1024)]
_cache = {}


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


def _weights(F, E=1024):
    key = ("w", F, E)
    if key not in _cache:
        _cache[key] = R.synthetic_voicefilter_weights(F, E, R.WEIGHT_SEED)
    return _cache[key]


def _model(F, dev, E=1024, cls="TrainableVoiceFilter"):
    """a fresh module with the seeded weights (training forwards change the running statistics)"""
    import speech_separation_amd as ssa
    m = getattr(ssa, cls)(F, embed_size=E)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in _weights(F, E).items()}, strict=True)
    return m.to(dev)


def _on(dev, *arrays):
    return tuple(torch.as_tensor(a).to(dev) for a in arrays)


def _masks(eng, tape, F, W, B):
    """the implementation's ReLU keep masks and dropout keep mask of `tape`, on the CPU"""
    cnn = [(eng.tape_tensor(tape, eng.TAPE_ACT, l) > 0).view(B, F, W, 64).permute(0, 3, 1, 2).cpu() for l in range(7)]
    relu = {"cnn": cnn, "lstm": (eng.tape_tensor(tape, eng.TAPE_LSTM_H) > 0).view(2 * B, W, 400).cpu(),
            "fc1": (eng.tape_tensor(tape, eng.TAPE_FC1) > 0).view(2 * B, W, 600).cpu()}
    return relu, eng.tape_tensor(tape, eng.TAPE_DROP).cpu().numpy().copy()


def _d_out(F, W, B, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, F, W, generator=gen), torch.randn(B, F, W, generator=gen)


def _case(dev, shape, E=1024, ppm=350000, seed=977, d_out="random"):
    """One forward + backward through the engine and both restatements with its masks, computed once per case."""
    key = ("case", shape, E, ppm, seed, d_out)
    if key in _cache:
        return _cache[key]
    F, W, Tv, B = shape
    w = _weights(F, E)
    x = R.synthetic_inputs(F, W, Tv, B, E, R.INPUT_SEED + F)
    m = _model(F, dev, E)
    eng = m._get_engine(dev)
    eng.bind_grads()
    xd = _on(dev, *x)
    o1, o2, tape = eng.train_forward(*xd, ppm, seed)
    relu, keep = _masks(eng, tape, F, W, B)
    assert np.array_equal(keep, T.keep_mask(2 * B, W, ppm, seed))                 # the mask is the host restatement's, bit for bit
    runs = {dt: T.forward(w, *x, dt, keep if ppm else None, relu) for dt in (torch.float64, torch.float32)}
    if d_out == "random":
        d = _d_out(F, W, B, seed=F + W)
        g = {dt: r.grads(*d) for dt, r in runs.items()}
    else:       # the gradient of MSESpecLoss: d loss / d out of the fp64 run, given to all three
        t1, t2 = T.targets(F, W, B)
        r64 = runs[torch.float64]
        a1, a2 = r64.out1.detach().requires_grad_(True), r64.out2.detach().requires_grad_(True)
        d = torch.autograd.grad(T.mse_pit_loss(a1, a2, torch.from_numpy(t1).double(), torch.from_numpy(t2).double()), (a1, a2))
        d = tuple(t.float() for t in d)
        g = {dt: r.grads(*d) for dt, r in runs.items()}
    eng.train_backward(*xd, *_on(dev, *d), tape)
    grads = {k: v.clone() for k, v in eng._grads.items()}
    tapes = {"Z": [eng.tape_tensor(tape, eng.TAPE_Z, l).cpu().clone() for l in range(8)],
             "stats": eng.tape_tensor(tape, eng.TAPE_STATS).cpu().clone(),
             "gates": eng.tape_tensor(tape, eng.TAPE_GATES).cpu().clone()}
    res = dict(m=m, eng=eng, x=x, xd=xd, d=d, tape=tape, out=(o1.cpu(), o2.cpu()), runs=runs, g=g, grads=grads, tapes=tapes, keep=keep)
    _cache[key] = res
    return res


def _judge_gradients(c, F, E, what):
    keys = T.trainable_keys(F, E)
    assert len(keys) == 58 and set(keys) <= set(c["grads"])
    for k in T.CONV_BIAS:
        assert float(c["grads"][k].abs().max()) == 0.0, k                          # exact zeros, see the module docstring
        bn = T.BN_BIAS[T.CONV_BIAS.index(k)]
        assert float(c["g"][torch.float64][k].norm()) < 1e-10 * float(c["g"][torch.float64][bn].norm()), k
    judged = [(k, c["grads"][k]) for k in keys if k not in T.CONV_BIAS]
    assert len(judged) == 50
    # check_gradients gathers one-element tensors (PReLU slopes) into a vector; this model has none, so it gets one empty
    # stand-in whose gradient is zero on every side
    one = ("(no one-element tensors)", torch.zeros(1))
    g64 = dict(c["g"][torch.float64], **{one[0]: torch.zeros(1, dtype=torch.float64)})
    g32 = dict(c["g"][torch.float32], **{one[0]: torch.zeros(1)})
    bad, worst, worst_x = check_gradients(judged + [one], g64, g32)
    print(f"{what}: worst ratio {worst:.3g}, worst ratio / fp32 restatement's {worst_x:.3g}; off the bound: {bad}")
    assert not bad, (what, bad)
    assert float(c["grads"]["gru.weight_hh_l1_reverse"].abs().max()) == 0.0


@pytest.mark.parametrize("shape,E", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_gradients_against_fp64_autograd(dev, shape, E):
    _judge_gradients(_case(dev, shape, E), shape[0], E, f"gradients {shape} E={E}")


def test_gradients_of_the_mse_spec_loss(dev):
    shape = (40, 33, 4, 2)
    _judge_gradients(_case(dev, shape, d_out="mse"), shape[0], 1024, f"gradients of MSESpecLoss {shape}")


def _col_worst(got, ref64, cols):
    """worst ||got - ref|| / ||ref|| over the columns: tensors reshaped to (cols, -1)"""
    got, ref = torch.as_tensor(got).double().reshape(cols, -1), torch.as_tensor(ref64).double().reshape(cols, -1)
    return float(((got - ref).norm(dim=1) / ref.norm(dim=1)).max())


@pytest.mark.parametrize("shape,E", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_tape_values_against_the_fp64_restatement(dev, shape, E):
    F, W, Tv, B = shape
    c = _case(dev, shape, E)
    r64, r32 = c["runs"][torch.float64], c["runs"][torch.float32]
    rows = []
    for l in range(8):                      # Z_l per (item, frame) column over (channel, f)
        z = c["tapes"]["Z"][l]
        z = z.permute(0, 1, 3, 2) if l == 7 else z.view(B, F, W, 64).permute(0, 2, 3, 1)      # -> (B, W, C, F)
        ref = lambda r: r.Z[l].detach().permute(0, 3, 1, 2)
        rows.append((f"Z{l + 1}", _col_worst(z, ref(r64), B * W), _col_worst(ref(r32), ref(r64), B * W)))
    st = c["tapes"]["stats"]
    for l in range(8):                      # batch mean and unbiased variance, a layer's channels as one column each
        C = 8 if l == 7 else 64
        for j, name in enumerate(("mean", "var")):
            rows.append((f"{name}{l + 1}", _col_worst(st[l, j, :C], r64.stats[l][j].detach(), 1),
                         _col_worst(r32.stats[l][j].detach(), r64.stats[l][j].detach(), 1)))
        assert float(st[l, :, C:].abs().max()) == 0.0 if C < 64 else True
    rows.append(("gates", _col_worst(c["tapes"]["gates"], r64.gates.detach(), 2 * B * W),
                 _col_worst(r32.gates.detach(), r64.gates.detach(), 2 * B * W)))
    got = tuple(o.permute(0, 2, 1) for o in c["out"])                                         # (B, W, F): one column per (item, frame)
    o64 = tuple(o.detach().permute(0, 2, 1) for o in (r64.out1, r64.out2))
    o32 = tuple(o.detach().permute(0, 2, 1) for o in (r32.out1, r32.out2))
    for s in range(2):
        assert float(o64[s].norm(dim=2).min()) > 0.1                                          # no column is zero
        rows.append((f"out{s + 1}", _col_worst(got[s], o64[s], B * W), _col_worst(o32[s], o64[s], B * W)))
    for name, rel, cpu in rows:
        print(f"{shape} E={E} {name}: HIP worst column {rel:.3e}, fp32 CPU worst column {cpu:.3e}, ratio {rel / max(cpu, 1e-300):.2f}")
    for name, rel, cpu in rows:
        assert rel <= 2.0 * cpu, (name, rel, cpu)


def test_running_statistics_and_counters(dev):
    F, W, Tv, B = 17, 7, 1, 3
    w = _weights(F)
    x = R.synthetic_inputs(F, W, Tv, B, 1024, R.INPUT_SEED + F)
    m = _model(F, dev).train()
    r64 = T.forward(w, *x, torch.float64, None)
    for steps in (1, 2):
        out = m.forward_embeddings(*_on(dev, *x))
        assert out["s1_spec_pred"].requires_grad and out["s1_spec_pred"].grad_fn is not None
        want = r64.updated_running(w, steps)
        sd = m.state_dict()
        for k, ref in want.items():
            rel = float((sd[k].cpu().double() - ref).norm() / ref.norm())
            assert rel <= 1e-6, (steps, k, rel)
        assert all(int(sd[f"cnn_layers.{bi}.num_batches_tracked"]) == steps for _, bi, *_r in R.CNN)
    m.eval()
    m.forward_embeddings(*_on(dev, *x))
    with torch.no_grad():
        m.train().forward_embeddings(*_on(dev, *x))
    assert all(int(m.state_dict()[f"cnn_layers.{bi}.num_batches_tracked"]) == 2 for _, bi, *_r in R.CNN)


def test_hard_values(dev):
    """Exact zeros and ones in the mixture; dropout off against on; a sequence whose every frame is dropped."""
    shape = F, W, Tv, B = 17, 7, 1, 3
    c = _case(dev, shape)
    mix = torch.from_numpy(c["x"][0])
    assert int((mix == 0).sum()) > 0 and int((mix == 1).sum()) > 0
    for o in c["out"]:
        assert bool((o[mix == 0] == 0).all()) and bool((o[mix == 1] > 0).all()) and bool(torch.isfinite(o).all())
    # an output gradient that lives on zero mixture bins alone reaches no parameter: every gradient is exactly zero
    eng, d = c["eng"], tuple(torch.where(mix == 0, t, torch.zeros(())) for t in c["d"])
    o1, o2, tape = eng.train_forward(*c["xd"], 350000, 977)
    eng.train_backward(*c["xd"], *_on(dev, *d), tape)
    for k in T.trainable_keys(F):
        assert float(eng._grads[k].abs().max()) == 0.0, k
    # dropout off: the mask is all ones and the values follow the restatement without dropout
    off = _case(dev, shape, ppm=0)
    assert off["keep"].min() == 1.0 and 0 < c["keep"].sum() < c["keep"].size
    assert not torch.equal(off["out"][0], c["out"][0])
    _judge_gradients(off, F, 1024, f"gradients {shape}, dropout off")
    # a seed whose mask drops every frame of one sequence, found on the host restatement
    seed = next(s for s in range(1, 200000) if (T.keep_mask(2 * B, W, 350000, s).sum(1) == 0).any())
    gone = _case(dev, shape, seed=seed)
    q = int(np.argmax(gone["keep"].sum(1) == 0))
    assert gone["keep"][q].sum() == 0
    _judge_gradients(gone, F, 1024, f"gradients {shape}, sequence {q} dropped whole (seed {seed})")
    r64 = gone["runs"][torch.float64]
    got = gone["out"][q // B][q % B]
    ref = (r64.out1, r64.out2)[q // B][q % B].detach()
    assert float((got.double() - ref).norm() / ref.norm()) < 1e-5


def test_determinism_and_routing(dev):
    shape = F, W, Tv, B = 40, 33, 4, 2
    c = _case(dev, shape, ppm=0)
    eng, xd, dd = c["eng"], c["xd"], _on(dev, *c["d"])
    # two backwards on one tape, then a second step with the same seed
    o1, o2, tape = eng.train_forward(*xd, 350000, 31)
    eng.train_backward(*xd, *dd, tape)
    a = eng._grads_flat.clone()
    eng.train_backward(*xd, *dd, tape)
    assert torch.equal(a, eng._grads_flat)
    p1, p2, tape = eng.train_forward(*xd, 350000, 31)
    eng.train_backward(*xd, *dd, tape)
    assert torch.equal(o1, p1) and torch.equal(o2, p2) and torch.equal(a, eng._grads_flat)
    # eval mode and no_grad are VoiceFilter's inference, bit for bit
    base = _model(F, dev, cls="VoiceFilter").eval()
    want = base.forward_embeddings(*xd)
    m = _model(F, dev)
    for got in (m.eval().forward_embeddings(*xd), None):
        if got is None:
            with torch.no_grad():
                got = m.train().forward_embeddings(*xd)
        assert not got["s1_spec_pred"].requires_grad
        assert torch.equal(got["s1_spec_pred"], want["s1_spec_pred"]) and torch.equal(got["s2_spec_pred"], want["s2_spec_pred"])
    # model(**batch) takes the embeddings as the loader delivers them, (B, E, Tv), and transposes them
    got = m.eval()(xd[0], s1_embedding=xd[1].transpose(1, 2).contiguous(), s2_embedding=xd[2].transpose(1, 2).contiguous())
    assert torch.equal(got["s1_spec_pred"], want["s1_spec_pred"]) and torch.equal(got["s2_spec_pred"], want["s2_spec_pred"])
    # waveform reconstruction belongs to the inference forward: refused by name in training mode, VoiceFilter's under no_grad
    # (at input_size 17: n_fft = 32 is a transform size the waveform ends take)
    m17, b17 = _model(17, dev).train(), _model(17, dev, cls="VoiceFilter").eval()
    gen = torch.Generator().manual_seed(3)
    wav, e1, e2 = _on(dev, 0.1 * torch.randn(2, 400, generator=gen), torch.randn(2, 3, 1024, generator=gen), torch.randn(2, 3, 1024, generator=gen))
    with pytest.raises(RuntimeError, match=r"model\.eval\(\) or use torch\.no_grad\(\)"):
        m17.separate_embeddings(wav, e1, e2)
    with torch.no_grad():
        sep = m17.separate_embeddings(wav, e1, e2)
    ref = b17.separate_embeddings(wav, e1, e2)
    assert torch.equal(sep["s1_pred"], ref["s1_pred"]) and torch.equal(sep["s2_pred"], ref["s2_pred"])
    # the speakers swapped (embeddings and output gradients, dropout off): the outputs swap bit for bit; the gradients are the
    # same sums with the two speakers' rows in the other order, so they stay within the rule, not bitwise
    s1, s2, tape = eng.train_forward(xd[0], xd[2], xd[1], 0, 0)
    assert torch.equal(s1.cpu(), c["out"][1]) and torch.equal(s2.cpu(), c["out"][0])
    eng.train_backward(xd[0], xd[2], xd[1], dd[1], dd[0], tape)
    swapped = dict(c, grads={k: v.clone() for k, v in eng._grads.items()})
    _judge_gradients(swapped, F, 1024, f"gradients {shape}, speakers swapped")
    same = sum(torch.equal(swapped["grads"][k], c["grads"][k]) for k in T.trainable_keys(F))
    print(f"speakers swapped: {same} of 58 gradients bitwise unchanged")


def _spec_batch(dev, shape):
    F, W, Tv, B = shape
    mix, e1, e2 = R.synthetic_inputs(F, W, Tv, B, 1024, R.INPUT_SEED + F)
    t1, t2 = T.targets(F, W, B)
    return {k: torch.from_numpy(v).to(dev) for k, v in (("mix_magnitude", mix), ("s1_embedding", e1), ("s2_embedding", e2),
                                                        ("s1_spec_true", t1), ("s2_spec_true", t2))}


def test_train_steps_track_fp64_adam(dev):
    """Three train.train_step calls with MSESpecLoss, the fused clip at 2 and FusedAdamW(weight_decay=0) (= Adam, lr 3e-4:
    vf_mse.yaml) against three fp64 torch.optim.Adam steps of the restatement that is given each step's masks from the tape:
    update ratio <= 4 x the fp32 restatement's + 1e-3 (the criterion of test_train_steps_track_fp64_adamw)."""
    from speech_separation_amd import FusedAdamW, MSESpecLoss, optim
    from speech_separation_amd.train import train_step
    shape = F, W, Tv, B = 17, 7, 1, 3
    w = _weights(F)
    m = _model(F, dev).train()
    batch = _spec_batch(dev, shape)
    crit = MSESpecLoss()
    opt = FusedAdamW(m.parameters(), lr=3e-4, weight_decay=0)
    keys = T.trainable_keys(F)
    cpu = {k: v.cpu() for k, v in batch.items()}
    refs = {dt: {k: torch.from_numpy(np.asarray(v)).to(dt).clone() for k, v in w.items() if not k.endswith("num_batches_tracked")}
            for dt in (torch.float64, torch.float32)}
    ropts = {}
    clipped = []
    orig = type(m._get_engine(dev)).grad_clip

    def spy(self, flat, mx):
        clipped.append(mx)
        return orig(self, flat, mx)

    type(m._engine).grad_clip = spy
    try:
        for step in range(3):
            train_step(m, dict(batch), crit, opt, max_grad_norm=2.0)
            assert optim.flat_grad_or_none(m) is not None
            eng = m._engine
            tape = (eng._tape_id, B, W, eng._ws.data_ptr(), Tv)
            relu, keep = _masks(eng, tape, F, W, B)
            for dt, ref in refs.items():
                run = T.forward(ref, cpu["mix_magnitude"], cpu["s1_embedding"], cpu["s2_embedding"], dt, keep, relu)
                _, g = run.loss_grads(cpu["s1_spec_true"], cpu["s2_spec_true"])
                if dt not in ropts:      # the optimizer owns the restatement's values from here on
                    for k in keys:
                        ref[k] = ref[k].clone().requires_grad_(True)
                    ropts[dt] = torch.optim.Adam([ref[k] for k in keys], lr=3e-4)
                for k in keys:
                    ref[k].grad = g[k].clone()
                torch.nn.utils.clip_grad_norm_([ref[k] for k in keys], 2.0)
                ropts[dt].step()
                for kk, v in run.updated_running(ref).items():
                    ref[kk] = v
    finally:
        type(m._engine).grad_clip = orig
    assert clipped == [2.0] * 3
    params = dict(m.named_parameters())
    start = {k: torch.from_numpy(np.asarray(w[k])).double() for k in keys}
    delta = lambda ps: torch.cat([(ps[k].detach().cpu().double() - start[k]).reshape(-1) for k in keys])
    d, d64, d32 = delta(params), delta(refs[torch.float64]), delta(refs[torch.float32])
    r, r32 = float((d - d64).norm() / d64.norm()), float((d32 - d64).norm() / d64.norm())
    print(f"3 Adam steps: update ratio {r:.3g} (fp32 restatement {r32:.3g})")
    assert r <= 4 * r32 + 1e-3
    for k in T.CONV_BIAS:                    # zero gradient, weight_decay 0: the conv biases keep their values
        assert torch.equal(params[k].detach().cpu(), torch.from_numpy(w[k])), k


def test_stock_optimizer_and_no_host_sync(dev):
    from speech_separation_amd import FusedAdamW, MSESpecLoss
    from speech_separation_amd.train import train_step
    shape = F, W, Tv, B = 17, 7, 1, 3
    batch = _spec_batch(dev, shape)
    crit = MSESpecLoss()
    torch.manual_seed(5)
    a, b = _model(F, dev).train(), _model(F, dev).train()          # same torch seed and step counter: the same dropout masks
    oa, ob = torch.optim.Adam(a.parameters(), lr=3e-4), FusedAdamW(b.parameters(), lr=3e-4, weight_decay=0)
    a.zero_grad()
    crit(**batch, **a(**batch))["loss"].backward()
    assert all(p.grad is not None for p in a.parameters())
    torch.nn.utils.clip_grad_norm_(a.parameters(), 2.0)
    oa.step()
    train_step(b, dict(batch), crit, ob, max_grad_norm=2.0)
    for (k, p), q in zip(a.named_parameters(), b.parameters()):
        assert torch.allclose(p, q, rtol=1e-5, atol=1e-6), k
    for k, v in a.state_dict().items():
        assert torch.equal(v, b.state_dict()[k]) or "running" not in k and "num_batches" not in k, k
    # a full fused step enqueues everything without a host synchronisation
    train_step(b, dict(batch), crit, ob, max_grad_norm=2.0)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        r = train_step(b, dict(batch), crit, ob, max_grad_norm=2.0)
    finally:
        torch.cuda.set_sync_debug_mode(0)
    assert torch.isfinite(r["loss"]) and torch.isfinite(r["grad_norm"])


def test_refusals(dev):
    """Refused before any launch: unsupported sizes, a small or misaligned workspace, unbound gradients, a backward without a
    forward on the workspace; and through the module, a tape that a later forward has overwritten."""
    from speech_separation_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p()
    for F, E, named in ((0, 1024, b"input_size"), (300, 1024, b"input_size"), (201, 100, b"embed_size")):
        assert lib.vftrain_create(ctypes.byref(h), F, E) == 1 and not h.value
        assert named in lib.vftrain_last_error(None)
    F, W, Tv, B = 17, 7, 1, 3
    m = _model(F, dev)
    eng = m._get_engine(dev)
    hh, st = eng._h, torch.cuda.current_stream(dev).cuda_stream
    x = _on(dev, *R.synthetic_inputs(F, W, Tv, B, 1024, 3))
    d = _on(dev, *_d_out(F, W, B, 1))
    o = torch.full((2, B, F, W), 7.0, device=dev)
    need = eng.workspace_bytes(B, W, Tv)
    ws = torch.zeros(need + 256, dtype=torch.uint8, device=dev)
    fwd = lambda w, n, b=B, ww=W, tv=Tv: lib.vftrain_train_forward(hh, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), b, ww, tv,
                                                                  350000, 1, o[0].data_ptr(), o[1].data_ptr(), w, n, st)
    bwd = lambda w, n: lib.vftrain_train_backward(hh, x[0].data_ptr(), x[1].data_ptr(), x[2].data_ptr(), B, W, Tv, d[0].data_ptr(),
                                                  d[1].data_ptr(), w, n, st)
    assert lib.vftrain_workspace_bytes(hh, 0, W, Tv) == 0 and b"B must be" in lib.vftrain_last_error(hh)
    assert fwd(ws.data_ptr(), need, b=0) == 1 and fwd(ws.data_ptr(), need, ww=0) == 1 and fwd(ws.data_ptr(), need, tv=0) == 1
    assert fwd(ws.data_ptr(), need - 1) == 2 and b"workspace" in lib.vftrain_last_error(hh)
    assert fwd(ws.data_ptr() + 4, need) == 2
    assert bwd(ws.data_ptr(), need) == 3 and b"gradients not bound" in lib.vftrain_last_error(hh)
    eng.bind_grads()
    assert bwd(ws.data_ptr(), need) == 1 and b"no tape" in lib.vftrain_last_error(hh)
    torch.cuda.synchronize()
    assert bool((o == 7.0).all()) and not ws.any() and not eng._grads_flat.any()             # nothing was launched
    assert fwd(ws.data_ptr(), need) == 0
    other = torch.zeros(need, dtype=torch.uint8, device=dev)
    assert bwd(other.data_ptr(), need) == 1 and b"no tape" in lib.vftrain_last_error(hh)     # a forward, but not on this workspace
    assert bwd(ws.data_ptr(), need) == 0
    torch.cuda.synchronize()
    m.train()
    out = m.forward_embeddings(*x)
    m.forward_embeddings(*x)                          # a later forward overwrites the tape
    with pytest.raises(RuntimeError, match="overwritten"):
        (out["s1_spec_pred"].sum() + out["s2_spec_pred"].sum()).backward()
    with pytest.raises(NotImplementedError, match="s1_embedding"):
        m.forward_embeddings(x[0], x[1].clone().requires_grad_(True), x[2])
