"""VoiceFilter on the MI355X, value tests: every case of tests/voicefilter_cases.py (shapes chosen by the residue of every
tiled dimension, the range ends F = 1 and F = 257, four weight regimes) against the fp64 restatement.

Training values: per column each Z_l and A_l, the 16 statistics, the LSTM's gates, cell and h, Y1 and both outputs, at most
2 x the fp32 CPU restatement's worst column of the same tensor.  Inference values: per output column, the same rule; and
with the running statistics set to a step's batch statistics the inference output stands within 2 x the fp32 restatement
of the training-mode output without dropout (the fold of vfilt_fold_kernel against the training chain).  Gradients: per
tensor the rule of check_gradients, per slice the rule of voicefilter_cases.judge_slices, exact zeros where fp64 has them;
two backwards on one tape are bitwise equal.  Both restatements receive this implementation's ReLU and dropout masks from
the tape; the host test asserts per case that no live pre-activation of the fp64 run is near a kink.  Every figure is
printed before it is asserted; test_zz prints the worst ratio per kernel and regime.

Then the two ends that the training tests left open: L1SpecLoss through the training path (its gradients, and three fused
steps against fp64 Adam), and a training step with a ShuffleNet lip reader in front."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F_

from tests import voicefilter_cases as C
from tests import voicefilter_ref as R
from tests import voicefilter_train_ref as T
from tests import test_gpu_voicefilter_train as TT
from tests.linear_ln_cases import judge_vector

pytestmark = pytest.mark.gpu
_cache = {}
WORST = {}            # (kernel, regime) -> (worst figure over its bound's yardstick, where)
ID = lambda c: c.id


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return torch.device("cuda:0")


def _note(kernel, regime, ratio, where):
    if ratio > WORST.get((kernel, regime), (-1.0, ""))[0]:
        WORST[(kernel, regime)] = (ratio, where)


def _module(case, dev, w, cls):
    import speech_separation_amd as ssa
    m = getattr(ssa, cls)(case.F, embed_size=case.E)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}, strict=True)
    return m.to(dev)


def _train_case(dev, case):
    """One forward, two backwards through the engine, and both restatements with its masks: once per case"""
    if case.id in _cache:
        return _cache[case.id]
    F, W, Tv, B = case.shape
    w, x = C.weights(case), C.inputs(case, C.input_seed(case)[0])
    m = _module(case, dev, w, "TrainableVoiceFilter")
    eng = m._get_engine(dev)
    eng.bind_grads()
    xd = TT._on(dev, *x)
    o1, o2, tape = eng.train_forward(*xd, C.PPM, C.DROP_SEED)
    relu, keep = TT._masks(eng, tape, F, W, B)
    assert np.array_equal(keep, T.keep_mask(2 * B, W, C.PPM, C.DROP_SEED))
    tapes = {"Z": [eng.tape_tensor(tape, eng.TAPE_Z, l).cpu().clone() for l in range(8)],
             "A": [eng.tape_tensor(tape, eng.TAPE_ACT, l).cpu().clone() for l in range(7)],
             "stats": eng.tape_tensor(tape, eng.TAPE_STATS).cpu().clone(),
             "gates": eng.tape_tensor(tape, eng.TAPE_GATES).cpu().clone(), "cell": eng.tape_tensor(tape, eng.TAPE_CELL).cpu().clone(),
             "h": eng.tape_tensor(tape, eng.TAPE_LSTM_H).cpu().clone(), "Y1": eng.tape_tensor(tape, eng.TAPE_FC1).cpu().clone()}
    runs = {dt: T.forward(w, *x, dt, keep, relu) for dt in (torch.float64, torch.float32)}
    d = C.d_out(case)
    g = {dt: r.grads(*d) for dt, r in runs.items()}
    dd = TT._on(dev, *d)
    eng.train_backward(*xd, *dd, tape)
    grads = {k: v.clone() for k, v in eng._grads.items()}
    flat = eng._grads_flat.clone()
    eng.train_backward(*xd, *dd, tape)
    same = torch.equal(flat, eng._grads_flat)
    for r in runs.values():           # the autograd graphs are done with: keep the values alone
        r.params = {}
        r.Z, r.act, r.stats = [t.detach() for t in r.Z], [t.detach() for t in r.act], [(a.detach(), b.detach()) for a, b in r.stats]
        r.gates, r.cell, r.h, r.fc1, r.out1, r.out2 = (t.detach() for t in (r.gates, r.cell, r.h, r.fc1, r.out1, r.out2))
    res = dict(m=m, eng=eng, x=x, out=(o1.cpu(), o2.cpu()), runs=runs, g=g, grads=grads, tapes=tapes, relu=relu, keep=keep, deterministic=same)
    _cache[case.id] = res
    return res


@pytest.mark.parametrize("case", C.TRAIN_CASES, ids=ID)
def test_training_values(dev, case):
    F, W, Tv, B = case.shape
    c = _train_case(dev, case)
    r64, r32, tp = c["runs"][torch.float64], c["runs"][torch.float32], c["tapes"]
    rows = []                                    # (name, got, fp64, fp32, columns, on the RMS column norm)
    cnn = lambda t: t.detach().permute(0, 3, 1, 2)                          # (B, C, F, W) -> (B, W, C, F): a column per (item, frame)
    for l in range(8):
        z = tp["Z"][l]
        z = z.permute(0, 1, 3, 2) if l == 7 else z.view(B, F, W, 64).permute(0, 2, 3, 1)
        rows.append((f"Z{l + 1}", z, cnn(r64.Z[l]), cnn(r32.Z[l]), B * W, False))
    for l in range(7):
        a = tp["A"][l].view(B, F, W, 64).permute(0, 2, 3, 1)
        rows.append((f"A{l + 1}", a, cnn(r64.act[l]), cnn(r32.act[l]), B * W, False))
    for l in range(8):
        Cn = 8 if l == 7 else 64
        for j, name in enumerate(("mean", "var")):
            rows.append((f"{name}{l + 1}", tp["stats"][l, j, :Cn], r64.stats[l][j].detach(), r32.stats[l][j].detach(), 1, False))
        if Cn < 64:
            assert float(tp["stats"][l, :, Cn:].abs().max()) == 0.0
    n = 2 * B * W
    y1 = lambda r: r.fc1.detach() * c["relu"]["fc1"].to(r.fc1.dtype)        # the tape holds Y1 behind its ReLU
    rows += [("gates", tp["gates"], r64.gates.detach(), r32.gates.detach(), n, False),
             ("cell", tp["cell"], r64.cell.detach(), r32.cell.detach(), n, False),
             ("h", tp["h"], r64.h.detach(), r32.h.detach(), n, False), ("Y1", tp["Y1"], y1(r64), y1(r32), n, False)]
    col = lambda o: o.detach().permute(0, 2, 1)                             # (B, W, F)
    for s in range(2):
        rows.append((f"out{s + 1}", col(c["out"][s]), col((r64.out1, r64.out2)[s]), col((r32.out1, r32.out2)[s]), B * W, case.rms_columns))
    bad = []
    for name, got, ref, cpu, cols, rms in rows:
        kernel = C.kernel_of_tensor(name)
        tensor = "out, F = 1" if case.F == 1 and name.startswith("out") else name
        wv, y, off = C.judge_columns(f"{case.id} {name}", got, ref, cpu, cols, rms, C.value_factor(kernel, case.regime, tensor))
        _note(kernel, case.regime, wv / y if y > 0 else (0.0 if wv == 0 else float("inf")), f"{case.id} {name}")
        if off:
            bad.append(off)
    if case.regime == "zerovar":     # the dead channel is exact zeros on the device, the constant channel is constant, everything is finite
        a5 = tp["A"][C.DEAD["layer"]].view(-1, 64)[:, C.DEAD["channel"]]
        a4 = tp["A"][C.ZEROVAR["layer"]].view(-1, 64)[:, C.ZEROVAR["channel"]]
        print(f"{case.id}: dead channel max {float(a5.abs().max())}, constant channel {float(a4.min())} .. {float(a4.max())}, "
              f"its variance on the device {float(tp['stats'][C.ZEROVAR['layer'], 1, C.ZEROVAR['channel']])}")
        assert float(a5.abs().max()) == 0.0 and float(a4.max() - a4.min()) == 0.0
        assert float(tp["stats"][C.ZEROVAR["layer"], 1, C.ZEROVAR["channel"]]) == 0.0
        assert all(bool(torch.isfinite(t).all()) for t in tp["Z"] + tp["A"] + [tp["stats"], tp["gates"], *c["out"]])
    assert not bad, bad


@pytest.mark.parametrize("case", C.TRAIN_CASES, ids=ID)
def test_training_gradients(dev, case):
    c = _train_case(dev, case)
    assert c["deterministic"], "two backwards on one tape differ"
    g64, g32 = c["g"][torch.float64], c["g"][torch.float32]
    bad = []
    for k in T.trainable_keys(case.F, case.E):
        g = c["grads"][k].cpu().numpy()
        assert np.isfinite(g).all(), k
        if k in T.CONV_BIAS:
            continue                  # exact zeros here, rounding noise in autograd: asserted by the per-tensor judge below
        bad += C.exact_zeros(case.id, k, g, g64[k].numpy())
        r, r32, _ = judge_vector(g, g64[k].numpy(), g32[k].numpy())
        print(f"{case.id} {k}: {r:.3g} (fp32 autograd {r32:.3g})")
        if float(g64[k].norm()) > 0:
            _note(C.kernel_of_gradient(k), case.regime, r / min(C.GRAD_BOUND, C.GRAD_FACTOR * max(r32, C.GRAD_FLOOR)), f"{case.id} {k} (tensor over its bound)")
        off, ratio = C.judge_slices(case.id, k, g, g64[k].numpy(), g32[k].numpy())
        _note(C.kernel_of_gradient(k), case.regime, ratio, f"{case.id} {k} (worst slice over its bound)")
        bad += off
    if case.regime == "zerovar":      # what the dead channel makes zero: its d gamma, d beta and the next layer's input-channel slice
        ch = C.DEAD["channel"]
        for k, idx in ((f"cnn_layers.{C.DEAD['bn']}.weight", ch), (f"cnn_layers.{C.DEAD['bn']}.bias", ch), ("cnn_layers.21.weight", (slice(None), ch))):
            assert float(g64[k][idx].abs().max()) == 0.0 and float(c["grads"][k][idx].abs().max()) == 0.0, k
    TT._judge_gradients(c, case.F, case.E, f"gradients {case.id}")
    assert not bad, bad


def _infer_case(dev, case):
    key = ("infer", case.id)
    if key not in _cache:
        w, x = C.weights(case, "infer"), C.inputs(case, C.input_seed(case)[0])
        m = _module(case, dev, w, "VoiceFilter").eval()
        out = m.forward_embeddings(*TT._on(dev, *x))
        _cache[key] = ((out["s1_spec_pred"].cpu(), out["s2_spec_pred"].cpu()), R.run(w, *x, torch.float64), R.run(w, *x, torch.float32))
    return _cache[key]


def _judge_outputs(case, what, got, ref64, ref32, kernel):
    bad = []
    for s in range(2):
        col = lambda o: torch.as_tensor(o).detach().permute(0, 2, 1)
        assert float(col(ref64[s]).double().norm(dim=2).pow(2).mean()) > 0
        wv, y, off = C.judge_columns(f"{case.id} {what} out{s + 1}", col(got[s]), col(ref64[s]), col(ref32[s]), case.B * case.W, case.rms_columns,
                                     C.value_factor(kernel, case.regime, "out"))
        _note(kernel, case.regime, wv / y if y > 0 else (0.0 if wv == 0 else float("inf")), f"{case.id} {what} out{s + 1}")
        bad += [off] if off else []
    assert not bad, bad


@pytest.mark.parametrize("case", C.INFER_CASES, ids=ID)
def test_inference_values(dev, case):
    got, ref64, ref32 = _infer_case(dev, case)
    assert all(bool(torch.isfinite(g).all()) for g in got)
    _judge_outputs(case, "inference", got, ref64, ref32, "vfilt_forward (whole chain)")


@pytest.mark.parametrize("case", C.TIE_CASES, ids=ID)
def test_inference_on_a_steps_batch_statistics_follows_the_training_chain(dev, case):
    """running_mean / running_var := the batch mean and biased variance of the fp64 training-mode run without dropout: the
    inference forward (vfilt_fold_kernel's scale and shift) must then give the training-mode output."""
    x = C.inputs(case, C.input_seed(case)[0])
    w = dict(C.weights(case))
    r64, r32 = (T.forward(w, *x, dt, None) for dt in (torch.float64, torch.float32))
    n = case.pos
    for l, (ci, bi, *_r) in enumerate(R.CNN):
        mean, var = r64.stats[l]
        w[f"cnn_layers.{bi}.running_mean"] = mean.detach().numpy().astype(np.float32)
        w[f"cnn_layers.{bi}.running_var"] = (var.detach().numpy() * (n - 1) / n).astype(np.float32)
    m = _module(case, dev, w, "VoiceFilter").eval()
    out = m.forward_embeddings(*TT._on(dev, *x))
    got = (out["s1_spec_pred"].cpu(), out["s2_spec_pred"].cpu())
    _judge_outputs(case, "inference on batch statistics", got, (r64.out1, r64.out2), (r32.out1, r32.out2), "vfilt_fold_kernel")


def test_lstm_step_instances(dev):
    """Which LSTM step kernel ran, from the launch geometry: <2> at B = 1, <8> in ceil(2B / 8) groups at B > 1; both judged above"""
    one, many = C.BY_ID["41x25x2x1-E1024-plain"], C.BY_ID["8x9x1x9-E1024-plain"]
    assert C.lstm_step_instance(one.B) == ("<2>", (100, 1)) and C.lstm_step_instance(many.B) == ("<8>", (100, 3))
    for case in (one, many):          # every sequence of every group was written: gates, cell and h of the last one too
        c = _train_case(dev, case)
        last = c["tapes"]["gates"].view(2 * case.B, case.W, 1600)[-1]
        assert float(last.abs().min()) > 0 and bool(torch.isfinite(last).all())


def _l1_pit_loss(o1, o2, t1, t2):
    """The reference's L1SpecLoss (ss_losses.py:47-62): batch-level PIT over the mean absolute error"""
    l1 = (F_.l1_loss(o1, t1) + F_.l1_loss(o2, t2)) / 2
    l2 = (F_.l1_loss(o1, t2) + F_.l1_loss(o2, t1)) / 2
    return l2 if bool(l2 < l1) else l1


def _l1_grads(run, t1, t2):
    dt = run.out1.dtype
    loss = _l1_pit_loss(run.out1, run.out2, torch.as_tensor(t1).to(dt), torch.as_tensor(t2).to(dt))
    keys = list(run.params)
    g = torch.autograd.grad(loss, [run.params[k] for k in keys], allow_unused=True)
    return loss.detach(), {k: (torch.zeros_like(run.params[k]) if gi is None else gi.detach()) for k, gi in zip(keys, g)}


def test_l1_spec_loss_gradients(dev):
    """model(**batch) -> L1SpecLoss -> backward in training mode: the parameters' .grad against fp64 autograd of the same loss"""
    from speech_separation_amd import L1SpecLoss
    shape = F, W, Tv, B = 17, 7, 1, 3
    m = TT._model(F, dev).train()
    batch = TT._spec_batch(dev, shape)
    m.zero_grad()
    loss = L1SpecLoss()(**batch, **m(**batch))["loss"]
    loss.backward()
    eng = m._engine
    relu, keep = TT._masks(eng, (eng._tape_id, B, W, eng._ws.data_ptr(), Tv), F, W, B)
    cpu = {k: v.cpu() for k, v in batch.items()}
    runs = {dt: T.forward(TT._weights(F), cpu["mix_magnitude"], cpu["s1_embedding"], cpu["s2_embedding"], dt, keep, relu)
            for dt in (torch.float64, torch.float32)}
    lg = {dt: _l1_grads(r, cpu["s1_spec_true"], cpu["s2_spec_true"]) for dt, r in runs.items()}
    gap = min(float((o.detach() - cpu[t].double()).abs().min()) for o in (runs[torch.float64].out1, runs[torch.float64].out2)
              for t in ("s1_spec_true", "s2_spec_true"))
    l64 = float(lg[torch.float64][0])
    print(f"L1SpecLoss: loss {float(loss):.8g}, fp64 {l64:.8g}; smallest |out - target| {gap:.3g}")
    assert gap > 1e-6 and abs(float(loss) - l64) <= 1e-5 * l64
    c = dict(grads={k: p.grad.detach().clone() for k, p in m.named_parameters()}, g={dt: v[1] for dt, v in lg.items()})
    TT._judge_gradients(c, F, 1024, f"gradients of L1SpecLoss {shape}")


def test_l1_spec_loss_train_steps_track_fp64_adam(dev):
    """test_train_steps_track_fp64_adam with L1SpecLoss: three train_step calls, the fused clip at 2 and
    FusedAdamW(weight_decay=0), against three fp64 Adam steps of the restatement; update ratio <= 4 x the fp32 restatement's + 1e-3."""
    from speech_separation_amd import FusedAdamW, L1SpecLoss, optim
    from speech_separation_amd.train import train_step
    shape = F, W, Tv, B = 17, 7, 1, 3
    w = TT._weights(F)
    m = TT._model(F, dev).train()
    batch = TT._spec_batch(dev, shape)
    crit, opt = L1SpecLoss(), FusedAdamW(m.parameters(), lr=3e-4, weight_decay=0)
    keys = T.trainable_keys(F)
    cpu = {k: v.cpu() for k, v in batch.items()}
    refs = {dt: {k: torch.from_numpy(np.asarray(v)).to(dt).clone() for k, v in w.items() if not k.endswith("num_batches_tracked")}
            for dt in (torch.float64, torch.float32)}
    ropts, clipped = {}, []
    orig = type(m._get_engine(dev)).grad_clip

    def spy(self, flat, mx):
        clipped.append(mx)
        return orig(self, flat, mx)

    type(m._engine).grad_clip = spy
    try:
        for step in range(3):
            res = train_step(m, dict(batch), crit, opt, max_grad_norm=2.0)
            assert optim.flat_grad_or_none(m) is not None and bool(torch.isfinite(res["loss"]))
            eng = m._engine
            relu, keep = TT._masks(eng, (eng._tape_id, B, W, eng._ws.data_ptr(), Tv), F, W, B)
            for dt, ref in refs.items():
                run = T.forward(ref, cpu["mix_magnitude"], cpu["s1_embedding"], cpu["s2_embedding"], dt, keep, relu)
                _, g = _l1_grads(run, cpu["s1_spec_true"], cpu["s2_spec_true"])
                if dt not in ropts:
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
    print(f"L1SpecLoss, 3 Adam steps: update ratio {r:.3g} (fp32 restatement {r32:.3g})")
    assert r <= 4 * r32 + 1e-3


def test_train_step_with_a_lip_reader_in_front(dev, monkeypatch):
    """TrainableVoiceFilter with a ShuffleNet lip reader, training mode, raw 96 x 96 clips of three frames: one train_step with
    torch.optim.Adam.  The reader is frozen, so train_step takes torch's clip; the reader's parameters stay bit for bit; the
    separator's gradients are those of forward_embeddings on the reader's own embeddings, bit for bit; the loss is finite."""
    import speech_separation_amd.train as train
    from speech_separation_amd import MSESpecLoss, TrainableVoiceFilter
    from tests import shufflenet_ref as SR
    from tests.test_gpu_shufflenet_lipreader import _model as lip_model
    torch.manual_seed(0)
    lip = lip_model("prelu", 1.0, dev)
    B, F, W, Tv = 2, 21, 9, 3
    w = R.synthetic_voicefilter_weights(F, 1024, R.WEIGHT_SEED)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
    a = TrainableVoiceFilter(F, lipreader=lip)
    res = a.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.startswith("lipreader.") for k in res.missing_keys)
    a = a.to(dev).train()
    b = TrainableVoiceFilter(F)
    b.load_state_dict(sd, strict=True)
    b = b.to(dev).train()
    assert not a.lipreader.training and not any(p.requires_grad for p in a.lipreader.parameters())
    reader_before = {k: v.detach().clone() for k, v in a.lipreader.state_dict().items()}
    mix, _, _ = R.synthetic_inputs(F, W, Tv, B, 1024, 90)
    t1, t2 = T.targets(F, W, B)
    v1 = torch.from_numpy(SR.synthetic_clip((B, Tv, 96, 96), seed=40)).to(dev)
    v2 = torch.from_numpy(SR.synthetic_clip((B, Tv, 96, 96), seed=41)).to(dev)
    batch = {"mix_magnitude": torch.from_numpy(mix).to(dev), "s1_video": v1, "s2_video": v2, "s1_spec_true": torch.from_numpy(t1).to(dev),
             "s2_spec_true": torch.from_numpy(t2).to(dev)}
    fused, stock = [], []
    monkeypatch.setattr(train, "clip_grad_norm_", lambda *args, **kw: fused.append(args) or torch.zeros(()))
    orig = torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_", lambda ps, mx, *args, **kw: stock.append(mx) or orig(ps, mx, *args, **kw))
    crit = MSESpecLoss()
    opt = torch.optim.Adam([p for p in a.parameters() if p.requires_grad], lr=3e-4)
    own_before = {k: p.detach().clone() for k, p in a.named_parameters() if p.requires_grad}
    out = train.train_step(a, dict(batch), crit, opt, max_grad_norm=1e6)      # a clip that scales by exactly 1
    assert not fused and stock == [1e6]
    assert bool(torch.isfinite(out["loss"])) and bool(torch.isfinite(out["grad_norm"])) and float(out["grad_norm"]) < 1e6
    for k, v in a.lipreader.state_dict().items():
        assert torch.equal(v, reader_before[k]), k
    assert all(p.grad is None for p in a.lipreader.parameters())
    moved = sum(not torch.equal(p.detach(), own_before[k]) for k, p in a.named_parameters() if p.requires_grad)
    assert moved >= 40, moved          # all but the eight conv biases and the reverse W_hh of GRU layer 2, whose gradients are zero
    window, affine = SR.preproc_window_affine((0, 96, 96))
    with torch.no_grad():
        e1, e2 = lip.forward_window(v1, window, affine).clone(), lip.forward_window(v2, window, affine).clone()
    b.zero_grad()
    pred = b.forward_embeddings(batch["mix_magnitude"], e1, e2)
    loss = crit(s1_spec_true=batch["s1_spec_true"], s2_spec_true=batch["s2_spec_true"], **pred)["loss"]
    loss.backward()
    assert torch.equal(loss.detach(), out["loss"])
    ga = {k: p.grad for k, p in a.named_parameters() if p.requires_grad}
    for k, p in b.named_parameters():
        assert torch.equal(p.grad, ga[k]), k
    assert len(ga) == 58


def test_zz_worst_ratio_per_kernel_and_regime():
    """The table of DESIGN.md §32: values as worst column / the fp32 restatement's worst column (bound 2), gradient slices as
    worst slice / its bound (bound 1)."""
    assert WORST, "run with the tests above"
    for (kernel, regime), (ratio, where) in sorted(WORST.items()):
        print(f"WORST {kernel:48s} {regime:10s} {ratio:8.3f}  {where}")
    for key, (reason_factor, why) in C.EXCEPTIONS.items():
        print(f"EXCEPTION {key}: factor {reason_factor}: {why}")
