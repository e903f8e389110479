"""Training attention on the GPU, every instantiation: attention_kernel<DH, NKB> with its softmax and bit-mask tapes and
attention_bwd_kernel<DH, NKB, 0 / 1>, DH = 32 / 16, NKB = 1..8, on both paths, with dropout off and on, against the fp64 formula
of tests/train_attention_cases.py -- judged on EVERY TOKEN of y and dx, where one wrong keep bit stands 10 dB or more below
the floor (tests/test_train_attention_host.py); over whole tensors it would pass from 160 positions on.

One test per case: dptnav_train_path_forward followed by dptnav_train_path_backward on the default kernels."""
import numpy as np
import pytest
import torch

from oracle import dptn_oracle as O
from tests import train_attention_cases as A

pytestmark = pytest.mark.gpu

WORST = {}      # (quantity, DH) -> (dB, case id, the fp32 restatement's figure for that case)
RAN = set()     # (DH, NKB, path, dropout on)
STARTED = set()


def _note(quantity, case, db, restatement):
    key = (quantity, case.features // 4)
    if key not in WORST or db < WORST[key][0]:
        WORST[key] = (db, case.id, restatement)


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_training_attention_matches_the_fp64_formula_on_every_token(case):
    """In this order: the device keep mask equals tests/dropout_ref.keep_mask bit for bit (dropout on); everything is finite
    and the training forward equals the inference forward to 120 dB (dropout off); y and dx reach 80 dB on every token; every
    parameter gradient of the path reaches 70 dB; y is bitwise reproducible (dropout 0.1, len = 32 NKB)."""
    from speech_separation_amd.engine import DptnEngine, params_to_device
    STARTED.add(case)
    A.check_preconditions(case)
    dev = torch.device("cuda:0")
    cfg = A.config(case.features, case.path, case.len, case.chunk)
    B, S, K, N = A.shape(case)
    x, dy = A.inputs(case)
    ref, ref32 = A.reference(case, 64), A.reference(case, 32)
    eng = DptnEngine(cfg, dev)
    try:
        eng.bind(params_to_device({k: np.array(v) for k, v in A.weights(case.features, case.path, case.len, case.chunk).items()}, dev))
        grads = eng.bind_grads()
        eng.set_option("dropout_ppm", case.ppm)
        eng.set_option("dropout_seed", A.DROPOUT_SEED)
        xt, dyt = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(dy)).to(dev)
        y, tape = eng.train_path_forward(0, case.path, xt)
        dx = eng.train_path_backward(0, case.path, xt, dyt, tape)
        torch.cuda.synchronize()
        y_np, dx_np = y.cpu().numpy(), dx.cpu().numpy()
        g_np = {leaf: grads[A.prefix(case) + leaf].cpu().numpy() for leaf in ref["grads"]}
        if case.ppm:
            assert np.array_equal(eng.dropout_mask(0, case.path, B, S).cpu().numpy(), A.mask(case)), "keep mask"
        assert np.isfinite(y_np).all() and np.isfinite(dx_np).all() and all(np.isfinite(g).all() for g in g_np.values())
        if not case.ppm:
            assert O.agreement_db(y_np, eng.stage_path(0, case.path, xt).cpu().numpy()) > 120, "training forward == inference forward"
        RAN.add((case.features // 4, case.nkb, case.path, bool(case.ppm)))

        fig = {k: (A.figures(got, ref[k]), A.figures(ref32[k], ref[k])) for k, got in (("y", y_np), ("dx", dx_np))}
        par = min((O.agreement_db(g_np[leaf], ref["grads"][leaf]), leaf) for leaf in g_np)
        par32 = min((O.agreement_db(ref32["grads"][leaf], ref["grads"][leaf]), leaf) for leaf in g_np)
        print(f"{case.id}: " + "; ".join(
            f"{k} {f[0]:.1f} dB, worst token {f[1]:.1f} dB at {f[2]} (fp32 restatement {r[0]:.1f} / {r[1]:.1f} at {r[2]})"
            for k, (f, r) in fig.items()) + f"; worst parameter {par[1]} {par[0]:.1f} dB (restatement {par32[1]} {par32[0]:.1f})")
        for k, (f, r) in fig.items():
            _note(k, case, f[0], r[0])
            _note(k + " worst token", case, f[1], r[1])
        _note("parameter (the worst of the path)", case, par[0], par32[0])
        for k, (f, r) in fig.items():
            assert f[1] >= A.TOKEN_FLOOR_DB, (case.id, k, "worst token", f[1], f[2], "fp32 restatement", r[1])
        for leaf in g_np:
            assert g_np[leaf].shape == ref["grads"][leaf].shape, leaf
            db = O.agreement_db(g_np[leaf], ref["grads"][leaf])
            assert db >= A.PARAM_FLOOR_DB, (case.id, leaf, db)
        if case.ppm == 100000 and case.len % 32 == 0:      # one length per (features, path, NKB): counter-based mask, no atomics
            y2, _ = eng.train_path_forward(0, case.path, xt)
            torch.cuda.synchronize()
            assert torch.equal(y2, y), "two training forwards with the same dropout seed differ"
    finally:
        eng.close()


def test_zz_worst_figures_are_reported():
    """The worst figures this session's cases reached, per quantity and head width (DESIGN.md quotes them), and: every
    (DH, NKB) instantiation ran on both paths with dropout off and on."""
    for (quantity, dh), (db, cid, r) in sorted(WORST.items()):
        print(f"train attention worst {quantity}, DH = {dh}: {db:.1f} dB at {cid} (fp32 restatement there: {r:.1f} dB)")
    want = {(dh, nkb, path, drop) for dh in (32, 16) for nkb in range(1, 9) for path in (0, 1) for drop in (False, True)}
    if len(STARTED) == len(A.CASES):      # (a selection of cases, -k, reports its figures only)
        assert RAN == want, sorted(want - RAN)
