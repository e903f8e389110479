"""The ends of the DPTN / DPRNN path on the MI355X, per frame and at every geometry (tests/path_ends_cases.py holds the case
table, the restatements and the judges; tests/test_path_ends_host.py proves their conditions on the CPU).

  head   video_linear_kernel, encoder_fuse_kernel                                         (stage_head)
  tail   separation conv, ALoadOla / EpiSkipDecoderTaps (fold_tail 0), fold_decoder_kernel + taps_fold_kernel (fold_tail 1),
         mask_tail.hip, decoder_gather_kernel                                             (stage_tail, tap "taps")
  backward_ends.h and mask_tail.hip's backward                                            (train_forward / train_backward)

The head and tail tests run no path: stage_tail takes a seeded block output and the latent of stage_head, so a failure
points at an end.  1. integer-valued operands, `torch.equal` against the fp64 oracle: a wrong index, a missed or
double-counted chunk or a wrong tap fails at the frame where it happens.  2. Gaussian operands per row (frame, token, tap
row, 16-sample window): worst row <= 2 x the fp32 restatement's worst row, both over the RMS row norm of the fp64 tensor; the
gate at 0.7, -1.3, 0, 1e-4 and 12.  3. every parameter gradient of one-block models by check_gradients (4 x the fp32
restatement / 1e-3 / floor 1e-6), encoder.weight and decoder.weight per tap column too, `gate` on its own too, at gates
0.7, -1.3, 0 and 1e-4."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import path_ends_cases as C
from tests.test_gpu_convtasnet_train import check_gradients

pytestmark = pytest.mark.gpu

LINEAR = [c.name for c in C.STAGE_CASES if not c.masked] + [C.MEMSAFETY_GEOMETRY.name]
ALL = [c.name for c in C.STAGE_CASES] + [C.MEMSAFETY_GEOMETRY.name]
TRAIN = [(c.name, g) for c in C.TRAIN_CASES for g in (C.TRAIN_GATES if c.name == C.GATE_CASE else (0.7,))]


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _engine(cfg, sd, dev):
    from speech_separation_amd.engine import DptnEngine, params_to_device
    eng = DptnEngine(cfg, dev)
    eng.bind(params_to_device(sd, dev))
    return eng


def _dev(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _emb(inp, dev, sl=slice(None)):
    return tuple(_dev(inp[k][sl], dev) if k in inp else None for k in ("s1_embedding", "s2_embedding"))


def _where(got: np.ndarray, want: np.ndarray) -> str:
    bad = np.argwhere(got != want)
    i = tuple(int(v) for v in bad[0])
    return f"{len(bad)} of {got.size} elements differ, first at {i}: got {got[i]!r}, want {want[i]!r}"


def _taps(eng, case, B=None):
    B = case.B if B is None else B
    return eng.tap("taps", B, case.T).view(2, B, case.L, 8).cpu().numpy().copy()


# ------------------------------------------------------------------------------------------------------------------
# 1. exact index tests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", LINEAR)
def test_integer_operands_give_the_oracle_bit_for_bit(dev, name):
    case = C.STAGE[name]
    cfg, sd, mix, x = C.exact_operands(case)
    want = C.exact_truth(name)
    eng = _engine(cfg, sd, dev)
    enc, chk = eng.stage_head(_dev(mix, dev))
    got = {"enc": enc.cpu().numpy(), "chunked": chk.cpu().numpy()}
    for k in ("enc", "chunked"):
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), f"{k}: {_where(got[k], want[k])}"
    xd = _dev(x, dev)
    for fold in (1, 0):
        eng.set_option("fold_tail", fold)
        s1, s2 = eng.stage_tail(xd, enc, case.T)
        torch.cuda.synchronize()
        got = {"taps": _taps(eng, case), "s1_pred": s1.cpu().numpy(), "s2_pred": s2.cpu().numpy()}
        for k in ("taps", "s1_pred", "s2_pred"):
            assert np.array_equal(got[k], want[k]), f"fold_tail {fold} {k}: {_where(got[k], want[k])}"
        assert not got["taps"][..., case.kenc:].any()
        for k in ("s1_pred", "s2_pred"):
            assert not got[k][:, :case.pad_left].any() and not got[k][:, case.pad_left + case.ndec:].any(), (fold, k)


# ------------------------------------------------------------------------------------------------------------------
# 2. per-frame value tests
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_head_rows_match_fp64(dev, name):
    case = C.STAGE[name]
    off = []
    for gate in (C.GATES if case.av else (0.7,)):
        cfg, sd, inp, _ = C.gaussian_operands(case, gate)
        refs = C.value_refs(name, gate)
        eng = _engine(cfg, sd, dev)
        mix, (e1, e2) = _dev(inp["mix"], dev), _emb(inp, dev)
        enc, chk = eng.stage_head(mix, e1, e2)
        got = {"enc": enc.cpu().numpy(), "chunked": chk.cpu().numpy()}
        tag = f"{name} gate {gate:g}" if case.av else name
        for k in ("enc", "chunked"):
            off.append(C.judge_rows(tag, k, got[k], refs["h64"][k], refs["h32"][k])[2])
        if case.av and gate == 0.0:      # tanh(0) = 0: the latent is the encoder conv alone, to the conv's own yardstick
            off.append(C.judge_rows(tag + " against the conv alone", "enc", got["enc"], refs["h64"]["conv"], refs["h32"]["conv"])[2])
        # the tokens are copies of the latent's frames: chunk s holds frames [P s, P s + K)
        idx = case.P * np.arange(case.S)[:, None] + np.arange(case.K)[None, :]
        assert np.array_equal(got["chunked"], got["enc"][:, idx]), f"{tag}: chunked is not a gather of enc"
        # bitwise repeatable, and an item's rows do not depend on the batch it is in
        enc2, chk2 = eng.stage_head(mix, e1, e2)
        assert torch.equal(enc2, enc) and torch.equal(chk2, chk), f"{tag}: not repeatable"
        if case.B > 1:
            b = slice(case.B - 1, case.B)
            e1b, e2b = _emb(inp, dev, b)
            enc1, chk1 = eng.stage_head(_dev(inp["mix"][b], dev), e1b, e2b)
            assert torch.equal(enc1, enc[b]) and torch.equal(chk1, chk[b]), f"{tag}: the last item's rows depend on B"
        eng.close()
    off = [o for o in off if o]
    assert not off, off


@pytest.mark.parametrize("name", ALL)
def test_tail_rows_match_fp64(dev, name):
    case = C.STAGE[name]
    cfg, sd, inp, x = C.gaussian_operands(case)
    eng = _engine(cfg, sd, dev)
    e1, e2 = _emb(inp, dev)
    enc, _ = eng.stage_head(_dev(inp["mix"], dev), e1, e2)
    refs = C.tail_refs(case, enc.cpu().numpy())
    t64 = refs["t64"]
    xd = _dev(x, dev)
    pads = C.padded_frames(case)
    off, got, yard = [], {}, {}
    for fold in ((None,) if case.masked else (1, 0)):
        if fold is not None:
            eng.set_option("fold_tail", fold)
        form, tag = ("t32f", f"{name} fold_tail 1") if fold == 1 else ("t32", f"{name} fold_tail 0" if fold == 0 else name)
        s1, s2 = eng.stage_tail(xd, enc, case.T)
        torch.cuda.synchronize()
        g = {"taps": _taps(eng, case), "s1_pred": s1.cpu().numpy(), "s2_pred": s2.cpu().numpy()}
        got[fold], yard[fold] = g, {}
        for k in ("taps", "s1_pred", "s2_pred"):
            _, yard[fold][k], bad = C.judge_rows(tag, k, g[k], t64[k], refs[form][k])
            off.append(bad)
        assert not g["taps"][..., case.kenc:].any(), f"{tag}: tap columns >= kernel_size_enc are not zero"
        for k in ("s1_pred", "s2_pred"):
            assert not g[k][:, :case.pad_left].any() and not g[k][:, case.pad_left + case.ndec:].any(), (tag, k)
        if len(pads):     # frames outside [left, left + ola): bias + skip (the masked tail: the bias-only mask on the latent)
            want = np.broadcast_to(t64["pad_taps"][None], t64["taps"].shape)[:, :, pads]
            w, i = C.worst_row("taps", g["taps"][:, :, pads], want, scale_of=t64["taps"])
            print(f"{tag} padded frames {pads.tolist()}: worst row {w:.3g}")
            if not w <= C.VALUE_FACTOR * yard[fold]["taps"]:
                off.append(f"{tag}: padded tap row {i} is {w:.3g} from the bias-plus-skip value")
        # bitwise repeatable, and an item's rows do not depend on the batch it is in
        r1, r2 = eng.stage_tail(xd, enc, case.T)
        torch.cuda.synchronize()
        assert torch.equal(r1, s1) and torch.equal(r2, s2) and np.array_equal(_taps(eng, case), g["taps"]), f"{tag}: not repeatable"
        if case.B > 1:
            b = slice(case.B - 1, case.B)
            o1, o2 = eng.stage_tail(xd[b].contiguous(), enc[b].contiguous(), case.T)
            torch.cuda.synchronize()
            assert torch.equal(o1, s1[b]) and torch.equal(o2, s2[b]), f"{tag}: the last item's waveforms depend on B"
            assert np.array_equal(_taps(eng, case, 1), g["taps"][:, b]), f"{tag}: the last item's tap rows depend on B"
    if not case.masked:     # the two linear forms agree within the sum of their two bounds
        for k in ("taps", "s1_pred", "s2_pred"):
            w, i = C.worst_row(k, got[1][k], got[0][k], scale_of=t64[k])
            print(f"{name} fold_tail 1 against 0, {k}: worst row {w:.3g}")
            if not w <= C.VALUE_FACTOR * (yard[1][k] + yard[0][k]):
                off.append(f"{name}: fold_tail 1 and 0 differ by {w:.3g} in row {i} of {k}")
    off = [o for o in off if o]
    assert not off, off


# ------------------------------------------------------------------------------------------------------------------
# 3. gradients of the end parameters
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,gate", TRAIN)
def test_end_gradients_match_fp64_autograd(dev, name, gate):
    """Every tensor of a one-block model by check_gradients; encoder.weight / decoder.weight per tap column as well (one
    wrong tap must not hide behind the kernel_size_enc - 1 others), and `gate` on its own as well as in the vector of
    one-element tensors (where the PReLU slope's gradient, a sum over every token, would outweigh it).

    The gate = 0 case failed before head_bwd_frames_kernel accumulated sum dE . beta itself: d gate was rebuilt as
    sum_i d beta_i / tanh(gate) * beta_i, and the term was dropped at tanh(gate) == 0."""
    case = C.TRAIN[name]
    cfg, sd, inp, d1, d2 = C.train_operands(case, gate)
    eng = _engine(cfg, sd, dev)
    grads = eng.bind_grads()
    mix, (e1, e2) = _dev(inp["mix"], dev), _emb(inp, dev)
    s1, s2, tape = eng.train_forward(mix, e1, e2)
    eng.train_backward(mix, e1, e2, _dev(d1, dev), _dev(d2, dev), tape)
    torch.cuda.synchronize()
    g64 = C.stock_gradients(cfg, sd, inp, d1, d2, torch.float64)
    g32 = C.stock_gradients(cfg, sd, inp, d1, d2, torch.float32)
    assert set(grads) == set(g64) == set(g32), sorted(set(grads) ^ set(g64))
    g64 = {k: v.reshape(grads[k].shape) for k, v in g64.items()}
    g32 = {k: v.reshape(grads[k].shape) for k, v in g32.items()}
    named = [(k, g.cpu()) for k, g in grads.items()]
    bad, worst, worst_x = check_gradients(named, g64, g32)
    slope = "dprnn.speakers_separation.0.weight"
    cols, c64, c32 = [(slope, grads[slope].cpu())], {slope: g64[slope]}, {slope: g32[slope]}
    for key in ("encoder.weight", "decoder.weight"):
        for j in range(case.kenc):
            kj = f"{key}[:, 0, {j}]"
            cols.append((kj, grads[key][:, 0, j].cpu()))
            c64[kj], c32[kj] = g64[key][:, 0, j], g32[key][:, 0, j]
    bad_c, worst_c, worst_cx = check_gradients(cols, c64, c32)
    bad = bad + [b for b in bad_c if b[0] != "PReLU slopes"]
    line = f"{name} gate {gate:g}: worst tensor {worst:.3g} ({worst_x:.2f} x restatement), worst tap column {worst_c:.3g} ({worst_cx:.2f} x)"
    if case.av:
        bad_g, worst_g, worst_gx = check_gradients([("gate", grads["gate"].cpu())], g64, g32)
        bad = bad + [("gate", *b[1:]) for b in bad_g]
        line += f", gate alone {worst_g:.3g} ({worst_gx:.2f} x): d gate {float(grads['gate']):.6g}, fp64 {float(g64['gate']):.6g}"
    print(line)
    ends = [b for b in bad if b[0] == "PReLU slopes" or C.is_end_tensor(b[0])]
    assert not bad, f"(key, ratio, fp32 ratio) off the bound -- end tensors: {ends}; all: {bad[:12]}"
