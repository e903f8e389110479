"""CPU only: the cases of tests/voicefilter_cases.py are what they claim.

The coverage table meets every residue class that a shape of the admitted box can reach (UNREACHABLE lists the others with
the reason, LEFT_OUT is empty), the geometry conditions and position edges occur, every regime's precondition holds on the
fp64 restatement, every case has an input draw that keeps the live pre-activations off the ReLU kinks, the draw tells two
exchanged gate blocks or BatchNorm layers apart, the seeded draw is unchanged by the regimes, and the per-slice judge sees
one wrong tap, channel, row, column or gate block that the per-tensor figure accepts."""
from __future__ import annotations

import numpy as np
import pytest
import torch

from tests import voicefilter_cases as C
from tests import voicefilter_ref as R
from tests import voicefilter_train_ref as T


def test_every_reachable_residue_class_is_met():
    assert C.LEFT_OUT == ()
    assert C.uncovered() == []
    table = C.coverage_table()
    assert len(table) == len({(p, k, n, d) for p, k, n, d, _, _ in C.launches()})
    for key, row in sorted(table.items()):
        print(key, {cls: len(ids) for cls, ids in sorted(row.items())})


def test_unreachable_is_exactly_what_the_box_cannot_reach():
    reach = C.reachable()
    for (formula, tile, kind), seen in reach.items():
        want = set(C.wanted_classes(tile, kind if kind != "tile" else ""))
        declared = set(C.UNREACHABLE.get((formula, tile), {})) if kind == "tile" else set()
        assert want - seen == declared, (formula, tile, kind, sorted(want - seen), sorted(declared))
    assert all(why for row in C.UNREACHABLE.values() for why in row.values())
    assert {k for k in C.UNREACHABLE} <= {(f, t) for f, t, _ in reach}


def test_geometry_conditions_and_edges():
    plain = [c for c in C.CASES if c.regime == "plain"]
    for name, cond in C.GEOMETRY.items():
        assert any(cond(c) for c in plain), name
    assert {c.pos for c in plain} >= set(C.POSITION_EDGES)
    assert sum(c.E == 512 for c in plain) >= 2
    assert {(17, 7, 1, 3), (33, 50, 3, 1), (40, 33, 4, 2), (201, 21, 5, 2), (17, 9, 2, 5)} <= {c.shape for c in plain}
    assert max(c.pos for c in C.CASES) <= C.BOX["pos"] and max(c.W for c in C.CASES) <= C.BOX["W"]
    for regime in C.REGIMES[1:]:      # three shapes each, one per residue class of the position tile
        assert sorted(c.pos % 64 for c in C.CASES if c.regime == regime) == [0, 1, 63]
    assert len(C.BY_ID) == len(C.CASES)


def test_lstm_step_instances():
    """<2> at B = 1 alone, <8> in ceil(2B / 8) groups otherwise: the launchers' formula"""
    assert C.lstm_step_instance(1) == ("<2>", (100, 1))
    assert C.lstm_step_instance(2) == ("<8>", (100, 1)) and C.lstm_step_instance(4) == ("<8>", (100, 1))
    assert C.lstm_step_instance(5) == ("<8>", (100, 2)) and C.lstm_step_instance(8) == ("<8>", (100, 2))
    assert C.lstm_step_instance(9) == ("<8>", (100, 3))
    assert {C.lstm_step_instance(c.B)[0] for c in C.CASES} == {"<2>", "<8>"}


def test_the_regimes_leave_the_seeded_draw_alone():
    for F, E in ((17, 1024), (33, 512)):
        before = R.weights_digest(R.synthetic_voicefilter_weights(F, E, R.WEIGHT_SEED))
        for regime in C.REGIMES:
            for mode in ("train", "infer"):
                w = C.weights(C.Case(F, 9, 2, 2, E, regime), mode)
                assert (R.weights_digest(w) == before) == (regime == "plain"), (regime, mode)
        assert R.weights_digest(R.synthetic_voicefilter_weights(F, E, R.WEIGHT_SEED)) == before


@pytest.mark.parametrize("case", C.CASES, ids=lambda c: c.id)
def test_preconditions(case):
    k, margin = C.input_seed(case)
    run = C.forward64(case, k)
    fig = C.check_preconditions(case, run)
    print(case.id, f"input seed {k}, kink margin {margin:.3g}", fig)
    assert margin > C.KINK_MARGIN
    if case.regime == "plain":
        assert k == 0 or case.pos > 4000, (case.id, k)      # the first draw, but for the largest shapes


def test_l1_targets_stay_off_the_kink():
    case = C.Case(17, 7, 1, 3)
    run = C.forward64(case, C.input_seed(case)[0])
    t1, t2 = T.targets(case.F, case.W, case.B)
    gaps = [float((o.detach() - torch.from_numpy(t).double()).abs().min()) for o in (run.out1, run.out2) for t in (t1, t2)]
    print("smallest |out - target| of the fp64 run:", gaps)
    assert min(gaps) > 1e-6


def test_the_restatements_gradient_is_consistent_at_one_frame_and_one_bin():
    """d beta of the last BatchNorm is the channel sum of the gradient that reaches its output: at W = 1 and F = 1 torch's CPU
    batch_norm backward breaks this when it is handed the permuted gradient as it comes (voicefilter_train_ref._PlainGrad)."""
    for shape in ((65, 1, 1, 1), (1, 9, 2, 2), (17, 7, 1, 3)):
        case = C.Case(*shape)
        run = C.forward64(case)
        d = tuple(t.double() for t in C.d_out(case))
        g = torch.autograd.grad((run.out1, run.out2), [run.act[7]], d, retain_graph=True)[0]
        want, got = g.sum((0, 2, 3)), run.grads(*d)["cnn_layers.29.bias"]
        rel = float((got - want).abs().max() / want.abs().max())
        print(shape, f"d beta_8 against the channel sums of d A_8: {rel:.3g}")
        assert rel < 1e-12, (shape, rel)


def test_distinct_order():
    """Two gate blocks or two BatchNorm layers' gamma exchanged move the fp64 output by more than 1e-3"""
    case = C.Case(17, 9, 2, 5)
    base = C.forward64(case, keep=None)
    ref = torch.cat((base.out1, base.out2)).detach()
    for what in C.SWAPS:
        run = C.forward64(case, keep=None, w=C.swapped(C.weights(case), what))
        moved = float((torch.cat((run.out1, run.out2)).detach() - ref).norm() / ref.norm())
        print(f"{what}: output moved by {moved:.3g}")
        assert moved > 1e-3, (what, moved)


def test_the_slice_judge_sees_what_the_tensor_figure_accepts():
    rng = np.random.default_rng(3)
    for key, shape, spoil in (("cnn_layers.9.weight", (64, 64, 5, 5), lambda g: g[:, :, 2, 1]), ("cnn_layers.9.weight", (64, 64, 5, 5), lambda g: g[7]),
                              ("cnn_layers.9.weight", (64, 64, 5, 5), lambda g: g[:, 9]), ("fc.1.weight", (600, 400), lambda g: g[:, 5]),
                              ("lstm.weight_hh_l0", (1600, 400), lambda g: g[400:410])):
        g64 = rng.standard_normal(shape)
        g32 = g64 + 1e-7 * rng.standard_normal(shape)
        g = g64 + 1e-7 * rng.standard_normal(shape)
        assert C.judge_slices("clean", key, g, g64, g32)[0] == []
        spoil(g)[...] *= 1.0 + 1e-5          # one slice off by 1e-5 of itself (basic indexing: a view of g)
        rel = float(np.linalg.norm(g - g64) / np.linalg.norm(g64))
        rel32 = float(np.linalg.norm(g32 - g64) / np.linalg.norm(g64))
        bad, _ = C.judge_slices("spoiled", key, g, g64, g32)
        print(key, shape, f"tensor figure {rel:.3g} (fp32 {rel32:.3g})", bad)
        assert rel < 1e-3 and rel <= 4 * max(rel32, 1e-6) and bad      # the rule of check_gradients accepts it; a slice does not
    # a slice that is zero in fp64 must be zero
    g64 = rng.standard_normal((64, 64, 5, 5));  g64[:, 7] = 0
    g = g64.copy();  g[3, 7, 0, 0] = 1e-12
    assert any("zero in fp64" in b for b in C.judge_slices("zero", "cnn_layers.21.weight", g, g64, g64.copy())[0])
    assert C.exact_zeros("zero", "k", g, g64) and not C.exact_zeros("zero", "k", g64, g64)
    # columns: own norm against the RMS column norm
    ref = np.ones((4, 8));  ref[2] = 0
    got = ref.copy();  got[2, 0] = 1e-9
    assert np.isinf(C.column_figures(got, ref, 4)[2]) and C.column_figures(got, ref, 4, rms=True)[2] < 1e-9
