"""CPU half of the Linear / LayerNorm stage tests (tests/linear_ln_cases.py; the GPU half is tests/test_gpu_linear_ln.py):
every precondition of every case in fp64, the truth pinned to torch's own operators, the fp32 restatement's figures per
regime, the defects the bound must catch, and the coverage table's own arithmetic."""
import os
import re
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import linear_ln_cases as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.id)
def test_preconditions_hold_in_fp64(case):
    """Geometry, regime condition on every row of the shaped LayerNorm input, max |score| <= 4, gate pre-activations within
    +-6, the ReLU kink, exact zeros in h only where `hzero` puts them; `exact`: sum |a b| <= 768 and fp32 == fp64 bit for bit."""
    print(case.id, L.check_preconditions(case))


def _some(regime=None, model=None, stage=None):
    return [c for c in L.CASES if (regime is None or c.base_regime == regime) and (model is None or c.model == model)
            and (stage is None or c.stage == stage)]


def test_truth_is_pinned_to_torch():
    """The fp64 formulas against torch.nn.functional.layer_norm / linear and the stock composition of the path."""
    rng = np.random.default_rng(5)
    z, g, b = rng.standard_normal((37, 128)) * 3 + 7, rng.standard_normal(128), rng.standard_normal(128)
    mine = L.layer_norm_rows(z, g, b)
    want = F.layer_norm(torch.from_numpy(z), (128,), torch.from_numpy(g), torch.from_numpy(b)).numpy()
    assert np.abs(mine["y"] - want).max() < 1e-12
    assert np.abs(mine["rs"] - 1 / np.sqrt(z.var(1) + 1e-5)).max() < 1e-12
    m, v = L.chan_merge(z)
    assert np.abs(m - z.mean(1)).max() < 1e-12 and np.abs(v - z.var(1)).max() < 1e-12
    for model in L.MODELS:
        for case in _some("plain", model)[:2]:
            f = L.host_forward(case, L.input_seed(case))
            x, dy = L.inputs(case, L.input_seed(case))
            ref = L.path_autograd(case, x, dy, torch.float64)
            assert np.abs(f["y"] - ref["y"]).max() < 1e-10, case.id
            if case.arch == "dptn":
                p = L.params(case)
                want = F.linear(torch.from_numpy(f["x"]), torch.from_numpy(p["mha.in_proj_weight"]), torch.from_numpy(p["mha.in_proj_bias"]))
                assert np.abs(f["qkv"] - want.numpy()).max() < 1e-12, case.id


def _restatement_figures(case):
    """{tensor: the fp32 restatement's worst row} on the host's own fp32 inputs."""
    f = L.host_forward(case, L.input_seed(case))
    out = {}
    lstm_in = f["x"]
    if case.arch == "dptn":
        r64, r32 = L.stage_refs(case, "qkv", f["x"])
        out["qkv"] = L.yardstick(r32, r64, "y")
        r64, r32 = L.stage_refs(case, "ln1", f["att"], f["x"])
        out.update({k + "1": L.yardstick(r32, r64, k) for k in ("y", "zn", "rs")})
        lstm_in = f["ln1"]["y"]
    r64, r32 = L.stage_refs(case, "ln2", f["h"], lstm_in, relu=case.arch == "dptn")
    out.update({k + "2": L.yardstick(r32, r64, k) for k in ("y", "zn", "rs")})
    return out


def test_restatement_figures_per_regime():
    """Printed: the worst row of the fp32 restatement per (regime, tensor) over the cases -- the yardstick of the GPU half."""
    worst = {}
    for case in L.CASES:
        if case.regime == "exact" or case.M not in L.TAIL_TOKENS:
            continue
        for k, v in _restatement_figures(case).items():
            assert np.isfinite(v), (case.id, k)
            key = (case.regime, k)
            worst[key] = max(worst.get(key, 0.0), v)
    for (regime, k), v in sorted(worst.items()):
        print(f"fp32 restatement, {regime}, {k}: worst row {v:.3g}")
    assert worst[("zero1", "zn1")] == 0 and worst[("zero2", "zn2")] == 0      # sigma^2 = 0: zn is exactly zero in fp32 too


def test_backward_regimes_leave_fp32_headroom():
    """Every regime in which the fixed half of the gradient rule is asserted: fp32 autograd within FP32_HEADROOM of fp64 on
    every judged tensor and on dx (one case per model and regime); in flat1 it is not, and the relative half is the rule."""
    for model in L.MODELS:
        for regime in L.BACKWARD_REGIMES:
            cases = [c for c in L.CASES if c.model == model and c.regime == regime and c.backward]
            if not cases:
                continue
            g64, g32 = L.gradient_refs(cases[0])
            for leaf in L.linear_ln_leaves(cases[0]):
                r, r32, _ = L.judge_vector(g32["grads"][leaf], g64["grads"][leaf], g32["grads"][leaf])
                assert r <= L.FP32_HEADROOM, (cases[0].id, leaf, r)
            assert L.row_figures(g32["dx"], g64["dx"]).max() <= L.FP32_HEADROOM, cases[0].id
    assert all(c.backward == (c.regime != "exact") for c in L.CASES)
    flat1 = [c for c in L.CASES if c.regime == "flat1" and c.model == "dptn128"][2]
    x, dy = L.inputs(flat1, L.input_seed(flat1))
    a, b = L.path_autograd(flat1, x, dy, torch.float64), L.path_autograd(flat1, x, dy, torch.float32)
    worst = max(L.judge_vector(b["grads"][k], a["grads"][k], b["grads"][k])[0] for k in L.linear_ln_leaves(flat1))
    print(f"{flat1.id}: fp32 autograd's worst tensor {worst:.3g}")
    assert worst > L.FP32_HEADROOM


def test_relu_signs_are_undecided_in_fp32_where_layernorm_1_has_hard_rows():
    """UNDECIDED_RELU: the fp32 restatement's y1 moves h by more than the smallest |h| of the case, so fp32 cannot say which side
    of the ReLU that unit is on; in `plain` and `wide1` it moves h by less."""
    for regime in L.UNDECIDED_RELU + ("plain", "wide1"):
        case = [c for c in L.CASES if c.model == "dptn128" and c.regime == regime and c.M == 65][0]
        f = L.host_forward(case, L.input_seed(case))
        y32 = L.stage_ln1(case, f["att"].astype(np.float32), f["x"].astype(np.float32), np.float32)["y"]
        moved = float(np.abs(L.lstm(case, y32.astype(np.float64))[0] - f["h"]).max())
        print(f"{case.id}: fp32 y1 moves h by {moved:.3g}; smallest |h| {f['kink']:.3g}")
        assert (moved > f["kink"]) == (regime in L.UNDECIDED_RELU), (case.id, moved, f["kink"])


def _ln_inputs(case):
    """(stage, z-producing arguments) of the LayerNorm the case's regime shapes (1 for plain DPTN)."""
    f = L.host_forward(case, L.input_seed(case))
    if case.arch == "dptn" and case.stage in (0, 1):
        return lambda dt, **d: L.stage_ln1(case, f["att"].astype(np.float32).astype(dt), f["x"].astype(np.float32).astype(dt), dt, **d)
    res = f["ln1"]["y"] if case.arch == "dptn" else f["x"]
    return lambda dt, **d: L.stage_ln2(case, f["h"].astype(np.float32).astype(dt), res.astype(np.float32).astype(dt), dt,
                                       case.arch == "dptn", **d)


def _caught(case, defect, rows, dtype=np.float32, tensors=("y", "zn", "rs")):
    """The defect, restated in `dtype` on `rows`, puts at least one judged tensor beyond 2 x the restatement's worst row on
    every row it touches."""
    run = _ln_inputs(case)
    r64, r32, bad = run(np.float64), [run(np.float32, **v) for v in L.LN_VARIANTS], run(dtype, defect=defect, rows=rows)
    out = {}
    for k in tensors:
        bound = L.VALUE_FACTOR * L.yardstick(r32, r64, k)
        with np.errstate(invalid="ignore"):
            fig = L.row_figures(np.nan_to_num(bad[k].astype(np.float64), nan=1e30, posinf=1e30, neginf=-1e30), r64[k])[rows]
        out[k] = (float(fig.min()), bound)
    print(case.id, defect, {k: f"{a:.3g} against {b:.3g}" for k, (a, b) in out.items()})
    assert any(a > b for a, b in out.values()), (case.id, defect, out)


def test_defects_are_caught():
    """Each defect of the issue's list, restated in numpy, exceeds the bound on the rows it touches in its named regime."""
    for case in _some("offset"):
        _caught(case, "one_pass", np.arange(case.M))
    for case in _some("mixed"):
        _caught(case, "neighbour", np.arange(case.M), np.float64)
    for regime in ("flat", "zero"):
        for case in _some(regime):
            _caught(case, "no_eps", np.arange(case.M), np.float64)
    n = 0
    for regime in ("offset", "wide"):
        for case in _some(regime, "dptn128", 1):      # ln_merge serves LayerNorm 1 of the fused 128-feature block
            _caught(case, "chan16", np.arange(case.M), np.float64)
            n += 1
    assert n >= 4
    # tail rows of the last tile taking row M - 1's result, at every M mod tile = 1 case: row M - 1 IS the tail row there, so
    # the defect that shows is the clamp leaking the other way: the last row gets row M - 2's result
    for case in L.CASES:
        if case.regime == "exact" or case.M % 16 != 1:
            continue
        run = _ln_inputs(case)
        r64, r32 = run(np.float64), [run(np.float32, **v) for v in L.LN_VARIANTS]
        bad = r32[0]["y"].copy()
        bad[-1] = bad[-2]
        fig = L.row_figures(bad, r64["y"])[-1]
        bound = L.VALUE_FACTOR * L.yardstick(r32, r64, "y")
        same_rows = case.base_regime == "zero" and case.arch == "dptn"      # (there every row of y is beta: equal rows)
        assert fig > bound or same_rows, (case.id, fig, bound)
        # ... and the clamp one row early: row M - 2, which the previous tile writes, takes row M - 1's result
        bad = r32[0]["y"].copy()
        bad[-2] = bad[-1]
        fig = L.row_figures(bad, r64["y"])[-2]
        assert fig > bound or same_rows, (case.id, fig, bound)


def test_layer_norm_backward_defect_is_caught():
    """LayerNorm backward without the mean(g zn) zn term, in `plain`: dx and the upstream gradients leave the bound."""
    for model in L.MODELS:
        case = _some("plain", model)[3]
        g64, g32 = L.gradient_refs(case)
        x, dy = L.inputs(case, L.input_seed(case))
        bad = L.path_autograd(case, x, dy, torch.float64, defect="no_mean_gzn")
        fig = L.row_figures(bad["dx"], g64["dx"])
        bound = L.VALUE_FACTOR * float(L.row_figures(g32["dx"], g64["dx"]).max())
        assert fig.max() > bound, (case.id, fig.max(), bound)
        leaf = "ffn.1.weight" if case.arch == "dptn" else "fc.weight"
        assert not L.judge_vector(bad["grads"][leaf], g64["grads"][leaf], g32["grads"][leaf])[2], case.id
        # the judge of matrices: a 32-wide slab tile of the weight gradient one block of rows down fails at its rows
        g = np.array(g64["grads"][leaf], np.float32)
        assert not L.judge_gradient(case.id, leaf, g, g64["grads"][leaf], g32["grads"][leaf])
        g[32:64, :32] = np.array(g[0:32, :32])
        assert any("row 3" in m or "row 4" in m or "row 5" in m or "row 6" in m for m in L.judge_gradient(case.id, leaf, g, g64["grads"][leaf], g32["grads"][leaf]))


def test_coverage_table_arithmetic():
    """Residues and tile counts the token set gives each tile height, NBUF against fcln_launch's instantiation list, and the
    grid covers the table."""
    res = {t: {L.residue(M, t) for M in L.TOKENS} for t in (8, 16, 32, 64)}
    assert all({"0", "1", "-1"} <= r for r in res.values()), res
    tiles = {t: {-(-M // t) for M in L.TOKENS} for t in (16, 32, 64)}
    assert {1, 3, 4} <= tiles[16] and {1, 2, 3} <= tiles[32] and {1, 2, 3} <= tiles[64], tiles
    # (no M of the set lies in 17..32: two tiles of 16 tokens are reached by the many-tiles cases alone)
    assert any((-(-M // 8)) % 4 for M in L.TOKENS) and any((-(-M // 16)) % 4 for M in L.TOKENS)      # ln_backward pass counts
    src = open(os.path.join(ROOT, "speech_separation_amd", "csrc", "fcln.hip")).read()
    body = src[src.index("int fcln_launch("):]
    inst = set(re.findall(r"launch<(\d+), (\d+), (\d), (\d), true, (true|false), (true|false)>", body))
    want = {(str(k), str(n), str(nb), str(act), "true" if pre else "false", "true" if save else "false")
            for (k, n, pre, act, save), nbufs in L.FCLN_INSTANCES.items() for nb in nbufs}
    assert inst == want, inst ^ want
    assert len(inst) + 2 == len(re.findall(r"launch<", body))      # seven LayerNorm instantiations (two NBUF of one) + the two plain forms
    missing = L.coverage_table() - L.grid_coverage()
    assert not missing, sorted(missing)
    assert len(L.LEFT_OUT) <= 2
    for case in L.CASES:      # the tick lists exist for every form of every case
        for form in L.infer_forms(case):
            assert L.expected_ticks(case, form, "infer")
        for form in L.train_forms(case):
            assert L.expected_ticks(case, form, "train_forward") and L.expected_ticks(case, form, "train_backward")


def test_many_tiles_geometry_and_reference_time():
    """At 256 CUs: 66 300 tokens; every persistent kernel has a workgroup with more than NBUF tiles; the fp64 + fp32
    references of one such case take a few seconds."""
    for cus in (256, 304, 64):
        case = L.many_tiles_case("dptn128", cus)
        assert case.M >= L.MANY_FACTOR * cus and case.M % 64 != 0, case
        L.stage_geometry(case)
        for kernel, grid in L.many_tiles_grids(case, cus).items():
            tiles, g, nbuf = grid
            assert tiles > nbuf * g, (kernel, cus, grid)
    case = L.many_tiles_case("dprnn64", 256)
    assert case.M == 66300
    t0 = time.time()
    L.check_preconditions(case)
    g64, g32 = L.gradient_refs(case)
    dt = time.time() - t0
    print(f"many-tiles reference ({case.id}, fp64 + fp32 autograd and preconditions): {dt:.1f} s")
    assert np.isfinite(g64["dx"]).all()
