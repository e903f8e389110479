"""The LSTM recurrence on the GPU, every inference kernel: lstm16x.hip (64 and 128 features), lstm16.hip, lstm4.hip, lstm.hip
(fp32 and split) and lstm16s.hip, on both paths and both architectures, at every tile edge and in every value regime of
tests/recurrence_cases.py -- judged on EVERY UNIT (sequence, position, direction) of the hc tap against the fp64 step loop,
on the input values the recurrence read on the device, with floors taken from the CPU restatement of each form's arithmetic
(tests/test_recurrence_host.py: both defective formulas stand 10 dB or more below every floor).

One test per case; one engine runs every form the case applies to through dptnav_stage_path.

The training forward and the BPTT (lstm16.hip / lstm.hip with the tape, lstm_bptt16.hip / lstm_bptt.hip: option lstm16 = 1 / 0)
go through train_path_forward / train_path_backward on the smaller grid of recurrence_cases.TRAIN_CASES: y and dx on every
token and the eight rnn.* gradients per tensor against fp64 autograd, floors from fp32 autograd of the same formula."""
import numpy as np
import pytest
import torch

from tests import recurrence_cases as R

pytestmark = pytest.mark.gpu

TRAIN_WORST = {}      # (training form, regime, quantity) -> (dB, case id, the fp32 restatement's figure there)
TRAIN_RAN = set()     # (training form, arch, features, path, regime)
TRAIN_STARTED = set()
WORST = {}      # (kernel, regime) -> (dB, case id, form, the restatement's worst unit for that case and form)
RAN = set()     # recurrence_cases.coverage_keys()
STARTED = set()


def _engine(cfg, sd, dev):
    from speech_separation_amd.engine import DptnEngine, params_to_device
    eng = DptnEngine(cfg, dev)
    try:
        eng.bind(params_to_device({k: np.array(v) for k, v in sd.items()}, dev))
    except Exception:
        eng.close()
        raise
    return eng


def _tap(eng, name, g, floats, rows, width):
    """A host copy of the first rows x width floats of a workspace tap, after checking that the plan gives it `floats`."""
    t = eng.tap(name, g["B"], g["T"], g["Tv"])
    assert t.numel() == floats, (name, t.numel(), floats)
    return t[:rows * width].cpu().numpy().reshape(rows, width)


@pytest.mark.parametrize("case", R.CASES, ids=lambda c: c.id)
def test_recurrence_matches_the_fp64_step_loop_on_every_unit(case):
    """In this order: the preconditions on the host's input; every form runs with the launch counts of its route (K4: none
    under lstm16x, one otherwise; the recurrence: one) and leaves a finite hc; on the input each form read on the device the
    defects stay 10 dB under the floors; every unit of hc reaches the floor of its form."""
    STARTED.add(case)
    R.check_preconditions(case)
    g = R.stage_geometry(case)
    dev = torch.device("cuda:0")
    num_cus = torch.cuda.get_device_properties(dev).multi_processor_count
    got = {}
    eng = _engine(R.config(case), R.weights(case), dev)
    try:
        assert eng._path_T(g["S"]) == g["T"] and eng.chunks(g["T"]) == g["S"], (case.id, g)
        xt = torch.from_numpy(np.array(R.inputs(case))).to(dev)
        eng.profile(True)
        outputs = []      # kept alive: no form's output lands in the memory of another's
        for form, opts in R.forms(case).items():
            for k, v in {**R.DEFAULTS, **opts}.items():
                eng.set_option(k, v)
            for name in ("hc", "y1"):      # a form that left one unwritten would otherwise be judged on the previous form's
                eng.tap(name, g["B"], g["T"], g["Tv"]).fill_(float("nan"))
            eng.profile_reset()
            outputs.append(eng.stage_path(0, case.path, xt))
            torch.cuda.synchronize()
            prof = eng.profile_read()
            kernel = R.kernel_for(form, case, num_cus)
            assert prof["lstm_pre_gemm"][1] == R.k4_launches(form, case) and prof["lstm_recurrence"][1] == 1, (case.id, form, kernel, prof)
            lstm_in = _tap(eng, "y1", g, g["y1_floats"], g["M"], g["N"]) if case.arch == "dptn" else R.inputs(case).reshape(g["M"], g["N"])
            got[form] = (kernel, R.LstmInput(lstm_in), _tap(eng, "hc", g, g["hc_floats"], g["M"], g["ldh"]))
            RAN.update(R.coverage_keys(form, case))
    finally:
        eng.close()

    failures = []
    for form, (kernel, lstm_in, hc) in got.items():
        assert np.isfinite(lstm_in.a).all() and np.isfinite(hc).all(), (case.id, form, "not finite")
        R.check_defects(case, lstm_in)
        refs = R.references(case, lstm_in)
        floor = R.floor_db(form, refs)
        fig, r = R.unit_figures(hc, refs["truth"]), R.unit_figures(refs[R.restatement_for(form)], refs["truth"])
        print(f"{case.id} {form} ({kernel}): hc {fig[0]:.1f} dB, worst unit {fig[1]:.1f} dB at {fig[2]}; floor {floor:.1f} "
              f"({R.restatement_for(form)} restatement {r[0]:.1f} / {r[1]:.1f} at {r[2]})")
        key = (kernel, case.regime)
        if key not in WORST or fig[1] < WORST[key][0]:
            WORST[key] = (fig[1], case.id, form, r[1])
        try:
            R.judge(f"{case.id} {form} ({kernel}) hc", hc, refs["truth"], floor)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures


@pytest.mark.parametrize("case", R.TRAIN_CASES, ids=lambda c: c.id)
def test_training_recurrence_and_bptt_match_fp64_autograd(case):
    """For lstm16 = 1 and 0, in this order: the preconditions; everything is finite; the training forward equals the inference
    forward of the same tile height to 120 dB; y and dx reach min(80, restatement - 20) dB on every token; each of the eight
    rnn.* gradients reaches min(70, restatement - 20) dB."""
    from oracle.dptn_oracle import agreement_db
    TRAIN_STARTED.add(case)
    R.check_train_preconditions(case)
    g = R.stage_geometry(case)
    dev = torch.device("cuda:0")
    ref, rest, floors = R.train_reference(case, 64), R.train_restatement(case), R.train_floors(case)
    x, dy = R.train_inputs(case)
    pre = R.prefix(case)
    got = {}
    eng = _engine(R.config(case), R.weights(case), dev)
    try:
        grads = eng.bind_grads()
        xt, dyt = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(dy)).to(dev)
        keep = []      # kept alive: no run's output lands in the memory of another's
        for form, lstm16 in R.TRAIN_FORMS.items():
            for k, v in {**R.DEFAULTS, **R.FORMS[form]}.items():
                eng.set_option(k, v)
            assert eng.options_set["lstm16"] == lstm16
            for t in grads.values():
                t.zero_()
            y, tape = eng.train_path_forward(0, case.path, xt)
            dx = eng.train_path_backward(0, case.path, xt, dyt, tape)
            yi = eng.stage_path(0, case.path, xt)
            torch.cuda.synchronize()
            keep += [y, tape, dx, yi]
            got[form] = {"y": y.cpu().numpy().reshape(g["M"], g["N"]), "dx": dx.cpu().numpy().reshape(g["M"], g["N"]),
                         "inference": yi.cpu().numpy().reshape(g["M"], g["N"]),
                         "grads": {leaf: grads[pre + leaf].cpu().numpy() for leaf in R.RNN_LEAVES}}
            TRAIN_RAN.add((form, case.arch, case.features, case.path, case.regime))
    finally:
        eng.close()

    failures = []
    for form, res in got.items():
        assert all(np.isfinite(a).all() for a in (res["y"], res["dx"], res["inference"], *res["grads"].values())), (case.id, form, "not finite")
        same = agreement_db(res["y"], res["inference"])
        fig = {k: R.figures(res[k], ref[k]) for k in ("y", "dx")}
        par = {leaf: R.param_db(res["grads"][leaf], ref["grads"][leaf]) for leaf in R.RNN_LEAVES}
        print(f"{case.id} lstm16={R.TRAIN_FORMS[form]}: training y against inference y {same:.1f} dB; " + "; ".join(
            f"{k} {f[0]:.1f} dB, worst token {f[1]:.1f} dB at {f[2]} (floor {floors[k]:.1f}, fp32 restatement {rest[k]:.1f})" for k, f in fig.items())
            + "; " + ", ".join(f"{leaf[4:]} {db:.1f} ({rest[leaf]:.1f})" for leaf, db in par.items()))
        worst_leaf = min(par, key=lambda leaf: par[leaf] - floors[leaf])
        for q, db, r in (("y worst token", fig["y"][1], rest["y"]), ("dx worst token", fig["dx"][1], rest["dx"]),
                         ("rnn gradient (the nearest to its floor)", par[worst_leaf], rest[worst_leaf])):
            key = (form, case.regime, q)
            if key not in TRAIN_WORST or db < TRAIN_WORST[key][0]:
                TRAIN_WORST[key] = (db, case.id, r)
        if not same > R.TRAIN_INFERENCE_DB:
            failures.append(f"{case.id} {form}: training forward against inference forward {same:.1f} dB")
        for k, f in fig.items():
            if not f[1] >= floors[k]:
                failures.append(f"{case.id} {form}: {k} worst token {f[1]:.1f} dB at {f[2]}, floor {floors[k]:.1f}, restatement {rest[k]:.1f}")
        for leaf, db in par.items():
            assert res["grads"][leaf].shape == ref["grads"][leaf].shape, leaf
            if not db >= floors[leaf]:
                failures.append(f"{case.id} {form}: {leaf} {db:.1f} dB, floor {floors[leaf]:.1f}, restatement {rest[leaf]:.1f}")
    assert not failures, failures


def test_zz_worst_figures_are_reported():
    """The worst unit this session's cases reached per (kernel, regime) next to the restatement's figure there (DESIGN.md
    quotes them), and: every kernel ran at every tile edge of the coverage table."""
    for (kernel, regime), (db, cid, form, r) in sorted(WORST.items()):
        print(f"recurrence worst unit, {kernel}, {regime}: {db:.1f} dB at {cid} {form} (restatement there: {r:.1f} dB)")
    if len(STARTED) == len(R.CASES):      # (a selection of cases, -k, reports its figures only)
        want = R.coverage_table()
        assert not want - RAN, sorted(want - RAN, key=str)
    for (form, regime, q), (db, cid, r) in sorted(TRAIN_WORST.items()):
        print(f"training recurrence worst {q}, lstm16 = {R.TRAIN_FORMS[form]}, {regime}: {db:.1f} dB at {cid} (fp32 restatement there: {r:.1f} dB)")
    if len(TRAIN_STARTED) == len(R.TRAIN_CASES):
        want = {(form, c.arch, c.features, c.path, c.regime) for c in R.TRAIN_CASES for form in R.TRAIN_FORMS}
        assert TRAIN_RAN == want, sorted(want - TRAIN_RAN)
