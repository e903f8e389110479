"""Inference attention on the GPU, every kernel and length: attn_block2_kernel<NKB, PRO, PERSIST>, attn_block_kernel<NKB, PRO>,
attn_block64_kernel<NB, PRO>, attention_kernel<DH, NKB> with its K1 / K3 GEMMs and attention_long_kernel<DH>, on both paths,
against the fp64 formula of tests/infer_attention_cases.py -- judged on EVERY TOKEN of y1 (and att, and the path output y),
where one wrong key in one query row stands 20 dB (10 dB behind a prologue chain) or more below the floor
(tests/test_infer_attention_host.py); over whole tensors it would pass from about 100 positions on.

One test per case.  A stage case runs every form that applies through dptnav_stage_path on one engine; a PRO case runs
dptnav_forward at B = 1 and reads LN1 of the last inter-chunk path from the workspace."""
import numpy as np
import pytest
import torch

from tests import infer_attention_cases as I

pytestmark = pytest.mark.gpu

WORST = {}      # (quantity, family, DH) -> (dB, case id, form, the fp32 restatement's figure for that case)
RAN = set()     # infer_attention_cases.coverage_key()
STARTED = set()
DEFAULTS = {"fuse_attn": 1, "attn_v2": 1, "attn_persist": 1}


def _note(quantity, case, form, pro, fig, restatement):
    inst = I.instantiation(case.features, form, case.len, pro)
    for q, db, r in ((quantity, fig[0], restatement[0]), (quantity + " worst token", fig[1], restatement[1])):
        key = (q, inst[0] + (" " + inst[3] if inst[3] else ""), case.features // 4)
        if key not in WORST or db < WORST[key][0]:
            WORST[key] = (db, case.id, form, r)


def _engine(cfg, sd, dev):
    from speech_separation_amd.engine import DptnEngine, params_to_device
    eng = DptnEngine(cfg, dev)
    try:
        eng.bind(params_to_device({k: np.array(v) for k, v in sd.items()}, dev))
    except Exception:
        eng.close()
        raise
    return eng


def _select(eng, opts):
    for k, v in {**DEFAULTS, **opts}.items():
        eng.set_option(k, v)


def _poison(eng, g, names):
    """NaN into the taps a run is about to fill: a form that left one unwritten would otherwise be judged on the previous form's."""
    for name in names:
        eng.tap(name, g["B"], g["T"], g["Tv"]).fill_(float("nan"))


def _tap(eng, name, g):
    """A host copy of a workspace tap, after checking that the plan gives it exactly the floats the case reads."""
    t = eng.tap(name, g["B"], g["T"], g["Tv"])
    assert t.numel() == g["tap_floats"], (name, t.numel(), g["tap_floats"])
    return t.cpu().numpy().reshape(g["M"], g["N"])


@pytest.mark.parametrize("case", I.CASES, ids=lambda c: c.id)
def test_stage_path_attention_matches_the_fp64_formula_on_every_token(case):
    """In this order: the preconditions; every form runs and leaves finite results; y1 (every form) and att (the unfused
    forms) reach 100 dB and y reaches 80 dB on every token; beyond 160 positions fuse_attn = 0 changes no bit; up to 160
    positions (len >= 2) the fused and the unfused y1 are not the same bits, so the option selects another kernel."""
    STARTED.add(case)
    I.check_preconditions(case)
    g = I.stage_geometry(case)
    dev = torch.device("cuda:0")
    ref, ref32 = I.reference(case, 64), I.reference(case, 32)
    restatement = {k: I.figures(ref32[k], ref[k]) for k in ("y1", "att", "y")}
    got = {}
    eng = _engine(I.config(case), I.weights(case), dev)
    try:
        assert eng._path_T(g["S"]) == g["T"] and eng.chunks(g["T"]) == g["S"], (case.id, g)
        xt = torch.from_numpy(np.array(I.inputs(case))).to(dev)
        outputs = []      # kept alive: no form's output lands in the memory of another's
        for form, opts in I.forms(case).items():
            _select(eng, opts)
            _poison(eng, g, ("y1", "att"))
            y = eng.stage_path(0, case.path, xt)
            outputs.append(y)
            torch.cuda.synchronize()
            got[form] = {"y": y.cpu().numpy().reshape(g["M"], g["N"]), "y1": _tap(eng, "y1", g)}
            if form in ("unfused", "auto"):
                got[form]["att"] = _tap(eng, "att", g)
            RAN.add(I.coverage_key(case.features, form, case.len, case.path))
    finally:
        eng.close()

    failures = []
    for form, res in got.items():
        for key, floor in (("y1", I.STAGE_FLOOR_DB), ("att", I.STAGE_FLOOR_DB), ("y", I.Y_FLOOR_DB)):
            if key not in res:
                continue
            assert np.isfinite(res[key]).all(), (case.id, form, key, "not finite")
            fig, r = I.figures(res[key], ref[key]), restatement[key]
            print(f"{case.id} {form}: {key} {fig[0]:.1f} dB, worst token {fig[1]:.1f} dB at {fig[2]} "
                  f"(fp32 restatement {r[0]:.1f} / {r[1]:.1f} at {r[2]})")
            _note(key, case, form, False, fig, r)
            try:
                I.judge(f"{case.id} {form} {key}", res[key], ref[key], floor)
            except AssertionError as e:
                failures.append(str(e))
    assert not failures, failures
    if case.len > I.FUSED_MAX:
        for key in ("y1", "att", "y"):
            assert np.array_equal(got["auto"][key], got["unfused"][key]), (case.id, key, "fuse_attn = 0 changes bits beyond 160 positions")
    elif case.len >= 2:
        for form in got:
            if form != "unfused":
                assert not np.array_equal(got[form]["y1"], got["unfused"]["y1"]), (case.id, form, "the same bits as fuse_attn = 0")


@pytest.mark.parametrize("case", [c for c in I.PRO_CASES if c not in I.LEFT_OUT], ids=lambda c: c.id)
def test_prologue_attention_matches_the_fp64_forward_on_every_token(case):
    """The forms with the FFN prologue, which only dptnav_forward runs: the preconditions; the head gives the chunk count the
    case names; both outputs and the final y1 are finite; the final y1 reaches 90 dB on every token against the fp64
    oracle for every form; the persistent form (attn_persist = 3) equals one workgroup per sequence bit for bit."""
    STARTED.add(case)
    I.check_pro_preconditions(case)
    g = I.pro_geometry(case)
    dev = torch.device("cuda:0")
    ref, r = I.pro_reference(case, 64), I.pro_restatement(case)
    got = {}
    eng = _engine(I.pro_config(case), I.pro_weights(case), dev)
    try:
        assert eng.frames(g["T"]) == g["L"] and eng.chunks(g["T"]) == g["S"] and eng.chunks(g["T"] + 1) == g["S"] + 1, (case.id, g)
        t = {k: torch.from_numpy(np.array(v)).to(dev) for k, v in I.pro_inputs(case).items()}
        assert tuple(t["mix"].shape) == (1, g["T"]) and (g["Tv"] == 1 or t["s1_embedding"].shape[-1] == g["Tv"])
        outputs = []
        for form, opts in I.pro_forms(case).items():
            _select(eng, opts)
            _poison(eng, g, ("y1",))
            s1, s2 = eng.forward(t["mix"], t.get("s1_embedding"), t.get("s2_embedding"))
            outputs += [s1, s2]
            torch.cuda.synchronize()
            got[form] = {"y1": _tap(eng, "y1", g), "s1": s1.cpu().numpy(), "s2": s2.cpu().numpy()}
            RAN.add(I.coverage_key(case.features, form, case.len, case.path, pro=True))
    finally:
        eng.close()

    failures = []
    for form, res in got.items():
        assert all(np.isfinite(a).all() for a in res.values()), (case.id, form, "not finite")
        fig = I.figures(res["y1"], ref)
        print(f"{case.id} {form}: final y1 {fig[0]:.1f} dB, worst token {fig[1]:.1f} dB at {fig[2]} "
              f"(fp32 restatement {r[0]:.1f} / {r[1]:.1f} at {r[2]})")
        _note("final y1", case, form, True, fig, r)
        try:
            I.judge(f"{case.id} {form} final y1", res["y1"], ref, I.PRO_FLOOR_DB)
        except AssertionError as e:
            failures.append(str(e))
    assert not failures, failures
    if "persist" in got:
        for key in ("y1", "s1", "s2"):
            assert np.array_equal(got["persist"][key], got["v2"][key]), (case.id, key, "attn_persist = 3 differs from attn_persist = 0")


def test_zz_worst_figures_are_reported():
    """The worst figures this session's cases reached, per quantity, kernel family and head width (DESIGN.md quotes them), and:
    every instantiation of every family ran, with one key and with all keys in its last key block, on both paths."""
    for (quantity, family, dh), (db, cid, form, r) in sorted(WORST.items()):
        print(f"infer attention worst {quantity}, {family}, DH = {dh}: {db:.1f} dB at {cid} {form} (fp32 restatement there: {r:.1f} dB)")
    if len(STARTED) == len(I.CASES) + len(I.PRO_CASES) - len(I.LEFT_OUT):      # (a selection of cases, -k, reports its figures only)
        want = I.instantiations()
        assert not want - RAN, sorted(want - RAN, key=str)
