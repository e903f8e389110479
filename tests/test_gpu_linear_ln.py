"""The token-wise Linear (+ LayerNorm + residual) stages of a DPTN / DPRNN path and their backward on the GPU: every kernel
(fcln.hip's seven LayerNorm instantiations, gemm_t.hip, the engine's row-space epilogues, the LayerNorms inside the fused
attention blocks, dgrad_t.hip, dgrad_r.hip and the engine's rider, the weight-gradient kernels, both LayerNorm backward
forms), at every tail residue of its tile and in every row regime of tests/linear_ln_cases.py.

Each stage is judged PER TOKEN against fp64 on the inputs it read on the device (workspace taps, DptnEngine.tape_tap), with
the bound 2 x the fp32 restatement's worst row; gradients against fp64 autograd of the stock composition per token (dx), per
tensor, and per row and column of every weight matrix.  tests/test_linear_ln_host.py holds the preconditions and shows that
the bound catches the defects it is there for."""
import re
import time

import numpy as np
import pytest
import torch

from tests import linear_ln_cases as L

pytestmark = pytest.mark.gpu

WORST = {}        # (kernel, regime, tensor) -> (ratio to the restatement, worst row, restatement's worst row, case id, form)
RAN = set()
STARTED = set()
# the recurrence between the judged stages is the same kernel in training and inference: K4 GEMM + lstm16.hip
RECURRENCE = {"lstm4": 0, "fuse_pre": 0, "fuse_pre128": 0}


def _engine(case, dev):
    from speech_separation_amd.engine import DptnEngine, params_to_device
    eng = DptnEngine(L.config(case), dev)
    try:
        eng.bind(params_to_device({k: np.array(v) for k, v in L.weights(case).items()}, dev))
    except Exception:
        eng.close()
        raise
    return eng


def _set(eng, opts):
    for k, v in {**L.DEFAULTS, **RECURRENCE, **opts}.items():
        eng.set_option(k, v)


def _np(t, rows, width):
    return t[:rows * width].cpu().numpy().reshape(rows, width)


def _record(case, form, kernel, regime, tensor, w, y):
    ratio = w / y if y > 0 else (0.0 if w == 0 else float("inf"))
    key = (kernel, regime, tensor)
    if key not in WORST or ratio > WORST[key][0]:
        WORST[key] = (ratio, w, y, case.id, form)


def _judge_forward(case, form, train, t, failures):
    """t: {"x", "qkv", "att", "y1", "hc", "y", "zn1", "rs1", "zn2", "rs2"} as read from the device (absent: not left by the form)."""
    M, N = case.M, case.N
    kern = L.forward_kernels(case, form, train)
    tag = f"{case.id} {'train' if train else 'infer'}:{form}"
    dptn = case.arch == "dptn"

    def regime_of(stage):
        return case.base_regime if case.stage in (0, stage) else "plain"

    def judge(stage, name, got, r64, r32s, kernel, regime):
        r32 = r32s[0]      # the plain restatement (bit equality in the zero regime)
        w, y, off = L.judge_rows(f"{tag} {name} ({kernel})", got, r64, r32s, factor=L.value_factor(kernel, regime, name))
        _record(case, form, kernel, regime, name, w, y)
        if off:
            failures.append(off)
        if regime == "zero" and name.startswith(("zn", "y")):      # sigma^2 = 0: zn == 0 and y == beta (+ x), bit for bit
            want = np.zeros_like(r32) if name.startswith("zn") else r32
            if not np.array_equal(np.asarray(got, np.float32).reshape(want.shape), want.astype(np.float32)):
                failures.append(f"{tag} {name} ({kernel}): not bit-equal to {'zero' if name.startswith('zn') else 'beta (+ x)'} in the zero regime")

    if "qkv" in t:
        r64, r32 = L.stage_refs(case, "qkv", t["x"])
        judge(1, "qkv", t["qkv"], r64["y"], [r["y"] for r in r32], kern["qkv"], "exact" if case.regime == "exact" else regime_of(1))
    if case.regime == "exact":
        return
    if dptn:
        if "att" in t:
            r64, r32 = L.stage_refs(case, "ln1", t["att"], t["x"])
        else:
            r64, r32 = L.fused_y1_refs(case, t["x"])
        judge(1, "y1", t["y1"], r64["y"], [r["y"] for r in r32], kern["ln1"], regime_of(1))
        if "zn1" in t:
            judge(1, "zn1", t["zn1"], r64["zn"], [r["zn"] for r in r32], kern["ln1"], regime_of(1))
            judge(1, "rs1", t["rs1"], r64["rs"], [r["rs"] for r in r32], kern["ln1"], regime_of(1))
    r64, r32 = L.stage_refs(case, "ln2", t["hc"], t["y1"] if dptn else t["x"], relu=dptn and train)
    judge(2, "y", t["y"], r64["y"], [r["y"] for r in r32], kern["ln2"], regime_of(2))
    if "zn2" in t:
        judge(2, "zn2", t["zn2"], r64["zn"], [r["zn"] for r in r32], kern["ln2"], regime_of(2))
        judge(2, "rs2", t["rs2"], r64["rs"], [r["rs"] for r in r32], kern["ln2"], regime_of(2))


def _run_case(case, infer_forms, train_forms, failures):
    g = L.stage_geometry(case)
    M, N, ldh = case.M, case.N, g["ldh"]
    dev = torch.device("cuda:0")
    dptn = case.arch == "dptn"
    x, dy = L.inputs(case, L.input_seed(case))
    x2 = x.reshape(M, N)
    pre = L.prefix(case)
    results = {}
    eng = _engine(case, dev)
    try:
        assert eng._path_T(g["S"]) == g["T"] and eng.chunks(g["T"]) == g["S"], (case.id, g)
        xt, dyt = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(dy)).to(dev)
        grads = eng.bind_grads()
        keep = []
        for form, opts in infer_forms.items():
            _set(eng, opts)
            names = ("qkv", "att", "y1", "hc") if dptn else ("hc",)
            for name in names:      # a form that left one unwritten would otherwise be judged on the previous form's
                eng.tap(name, g["B"], g["T"], g["Tv"]).fill_(float("nan"))
            y = eng.stage_path(0, case.path, xt)
            torch.cuda.synchronize()
            keep.append(y)
            t = {"x": x2, "y": _np(y.reshape(-1), M, N), "hc": _np(eng.tap("hc", g["B"], g["T"], g["Tv"]), M, ldh)}
            if dptn:
                t["y1"] = _np(eng.tap("y1", g["B"], g["T"], g["Tv"]), M, N)
                if not L.fused(form):
                    t["qkv"] = _np(eng.tap("qkv", g["B"], g["T"], g["Tv"]), M, 3 * N)
                    t["att"] = _np(eng.tap("att", g["B"], g["T"], g["Tv"]), M, N)
            results[("infer", form)] = t
        for form, opts in train_forms.items():
            _set(eng, opts)
            o = {**L.DEFAULTS, **opts}
            for v in grads.values():
                v.zero_()
            y, tape = eng.train_path_forward(0, case.path, xt)
            t = {"x": x2, "y": _np(y.reshape(-1), M, N), "hc": _np(eng.tape_tap(tape, "hc", g["B"], g["S"]), M, ldh)}
            if dptn:
                for name, w in (("qkv", 3 * N), ("att", N), ("y1", N)):
                    t[name] = _np(eng.tape_tap(tape, name, g["B"], g["S"]), M, w)
            if o["ln_tape"]:
                for name, w in ((("zn1", N), ("rs1", 1)) if dptn else ()) + (("zn2", N), ("rs2", 1)):
                    t[name] = _np(eng.tape_tap(tape, name, g["B"], g["S"]), M, w)
            else:
                with pytest.raises(RuntimeError, match="no LayerNorm rows under ln_tape = 0"):
                    eng.tape_tap(tape, "zn2", g["B"], g["S"])
            if not dptn:
                with pytest.raises(RuntimeError, match="a DPRNN path has no attention half"):
                    eng.tape_tap(tape, "qkv", g["B"], g["S"])
            if case.backward:
                dx = eng.train_path_backward(0, case.path, xt, dyt, tape)
                torch.cuda.synchronize()
                t["dx"] = _np(dx.reshape(-1), M, N)
                t["grads"] = {leaf: grads[pre + leaf].cpu().numpy() for leaf in L.linear_ln_leaves(case)}
                if o["deterministic"]:      # static tile assignment: the gradients repeat bit for bit
                    for v in grads.values():
                        v.zero_()
                    y2, tape2 = eng.train_path_forward(0, case.path, xt)
                    dx2 = eng.train_path_backward(0, case.path, xt, dyt, tape2)
                    torch.cuda.synchronize()
                    keep += [y2, tape2, dx2]
                    if not (np.array_equal(dx2.cpu().numpy().reshape(M, N), t["dx"])
                            and all(np.array_equal(grads[pre + leaf].cpu().numpy(), a) for leaf, a in t["grads"].items())):
                        failures.append(f"{case.id} train:{form}: the gradients do not repeat bit for bit")
                keep.append(dx)
            torch.cuda.synchronize()
            keep += [y, tape]
            results[("train", form)] = t
    finally:
        eng.close()

    for (kind, form), t in results.items():
        _judge_forward(case, form, kind == "train", t, failures)
    # Training forward against the inference forward of the same tile height, 120 dB: wherever an fp32 evaluation can be asked for
    # it -- the fp32 restatement of y (and of y1) on the training run's own inputs stands within 1e-6 of fp64.  Beyond that
    # (offset, flat, mixed: one ulp of a 300-valued y1 is 1e-4 sigma) two correct fp32 evaluations differ by more; printed.
    # DPTN-128 `default` has LayerNorm 1 on 16-token tiles (fcln) where inference has it on the engine's 32: its partner is the
    # nearest inference form, not the same kernels.
    if case.regime != "exact" and not case.many:
        from oracle.dptn_oracle import agreement_db
        pairs = [("default", "sep-fcln" if case.model.startswith("dptn128") else "sep-engine")]
        if "engine" in train_forms:
            pairs.append(("engine", "sep-engine"))
        for tf, inf in pairs:
            if ("train", tf) in results and ("infer", inf) in results:
                tr = results[("train", tf)]
                r64, r32 = L.stage_refs(case, "ln2", tr["hc"], tr["y1"] if dptn else tr["x"], relu=dptn)
                noise = L.yardstick(r32, r64, "y")
                if dptn:
                    r64, r32 = L.stage_refs(case, "ln1", tr["att"], tr["x"])
                    noise = max(noise, L.yardstick(r32, r64, "y"))
                db = agreement_db(tr["y"], results[("infer", inf)]["y"])
                asked = noise <= 1e-6
                print(f"{case.id}: training forward ({tf}) against inference forward ({inf}): {db:.1f} dB (fp32 restatement at {noise:.2g}: {'asserted' if asked else 'not asked for'})")
                if asked and not db > L.TRAIN_INFERENCE_DB:
                    failures.append(f"{case.id}: training forward ({tf}) against inference forward ({inf}) {db:.1f} dB")
    if case.backward:
        g64, g32 = L.gradient_refs(case)
        for form in train_forms:
            t = results[("train", form)]
            tag = f"{case.id} train:{form}"
            fixed = case.regime in L.BACKWARD_REGIMES      # (elsewhere the relative half of the rule; beyond 1e-3 is printed as a FINDING)
            leaves = L.judged_leaves(case)
            if not (np.isfinite(t["dx"]).all() and all(np.isfinite(a).all() for a in t["grads"].values())):
                failures.append(f"{tag}: a gradient is not finite")
            if leaves == L.linear_ln_leaves(case):      # (else: the ReLU's sign is undecided in fp32, see UNDECIDED_RELU)
                w, y, off = L.judge_rows(f"{tag} dx", t["dx"], g64["dx"], g32["dx"], gradient=True, fixed=fixed)
                for kernel in L.backward_kernels(case, form).values():
                    _record(case, form, kernel, case.base_regime, "dx", w, y)
                if off:
                    failures.append(off)
            for leaf in leaves:
                failures += L.judge_gradient(tag, leaf, t["grads"][leaf], g64["grads"][leaf], g32["grads"][leaf], fixed)


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.id)
def test_linear_and_layernorm_stages_match_fp64_on_every_token(case):
    """The preconditions; every inference and training form of the case; every judged tensor finite and within 2 x the fp32
    restatement's worst row on every token; zero regime: bit for bit; gradients per token, tensor, row and column."""
    STARTED.add(case)
    L.check_preconditions(case)
    failures = []
    train = L.train_forms(case)
    if case.regime == "exact":      # qkv from the inference tap and from the tape under gemm_t = 1 and 0
        infer = {"sep-engine": L.INFER_FORMS["sep-engine"]}
        train = {k: train[k] for k in ("default", "engine") if k in train}
    else:
        infer = L.infer_forms(case)
    _run_case(case, infer, train, failures)
    RAN.update(L.coverage_keys(case))
    assert not failures, failures


@pytest.mark.parametrize("model,regime", [(m, "plain") for m in L.MANY_MODELS] + [("dptn128", "hzero"), ("dptn64", "hzero")])
def test_many_tiles(model, regime):
    """258 tokens per CU: every persistent kernel gives some workgroup more than its tiles in flight and others fewer;
    ln_backward_kernel makes more than one trip and its last is partial.  Plain rows, every 5th `offset` (DPTN)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = L.many_tiles_case(model, cus, regime)
    for kernel, (tiles, grid, nbuf) in L.many_tiles_grids(case, cus).items():
        assert tiles > nbuf * grid, (kernel, tiles, grid, nbuf)
    t0 = time.time()
    L.check_preconditions(case)
    failures = []
    infer = {k: v for k, v in L.infer_forms(case).items() if not L.fused(k)}      # (a fused block takes one sequence, not tiles of tokens)
    train = {k: v for k, v in L.train_forms(case).items() if k in ("default", "engine")}
    _run_case(case, infer, train, failures)
    print(f"{case.id}: {time.time() - t0:.1f} s")
    assert not failures, failures[:20]


@pytest.mark.parametrize("model", ("dptn128", "dptn64"))
def test_many_tiles_exact_in_projection(model):
    """Integer operands at the many-tiles size: qkv equals fp64 bit for bit from the inference tap and from the tape under
    gemm_t = 1 and 0."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = L.many_tiles_case(model, cus, "exact")
    L.check_preconditions(case)
    failures = []
    train = {k: v for k, v in L.train_forms(case).items() if k in ("default", "engine")}
    _run_case(case, {"sep-engine": L.INFER_FORMS["sep-engine"]}, train, failures)
    assert not failures, failures[:20]


@pytest.mark.parametrize("case", L.CHAIN_CASES, ids=lambda c: "chain-" + c.id)
def test_chained_ffn_prologue_matches_fp64_on_every_token(case):
    """LayerNorm 2 of path 0 in fragment space inside path 1's fused block (dptnav_forward, fuse_ffn = 1) and as a launch of
    its own (fuse_ffn = 0): the y1 tap of path 1, per token, against the fp64 chain from the mixture; bound 2 x the worst row
    of the same chain in fp32."""
    y64, y32 = L.chain_refs(case)
    g = L.stage_geometry(case)
    dev = torch.device("cuda:0")
    inp = {k: torch.from_numpy(v).to(dev) for k, v in L.chain_inputs(case).items() if k in ("mix", "s1_embedding", "s2_embedding")}
    audio_only = L.config(case).audio_only
    Tv = 1 if audio_only else inp["s1_embedding"].shape[-1]
    failures = []
    eng = _engine(case, dev)
    try:
        for fuse in (1, 0):
            eng.set_option("fuse_ffn", fuse)
            eng.tap("y1", 1, g["T"], Tv).fill_(float("nan"))
            out = eng.forward(inp["mix"], None if audio_only else inp["s1_embedding"], None if audio_only else inp["s2_embedding"])
            torch.cuda.synchronize()
            y1 = _np(eng.tap("y1", 1, g["T"], Tv), case.M, case.N)
            kernel = ("attn_block64" if case.N == 64 else "attn_block2") + (" + FFN prologue" if fuse else "")
            w, y, off = L.judge_rows(f"chain {case.id} fuse_ffn={fuse} y1 ({kernel})", y1, y64, y32)
            _record(case, f"fuse_ffn={fuse}", kernel, case.base_regime, "chain y1", w, y)
            if off:
                failures.append(off)
    finally:
        eng.close()
    assert not failures, failures


def _ticks(eng, call):
    """The launch names `call` ticks, in order: the n-th tick of option inject_fail fails with its launch's name (the
    injection returns before the launch)."""
    names = []
    for n in range(1, 40):
        eng.set_option("inject_fail", n)
        try:
            call()
        except RuntimeError as e:
            m = re.search(r": (.*): injected failure", str(e))
            assert m, str(e)
            names.append(m.group(1))
            torch.cuda.synchronize()
            continue
        eng.set_option("inject_fail", 0)
        torch.cuda.synchronize()
        return names
    raise AssertionError("more than 39 ticks")


@pytest.mark.parametrize("model", list(L.MODELS))
def test_each_form_runs_the_kernels_of_its_route(model):
    """Per (model, form) at the smallest M, both paths: the launch names ticked equal the fixed list of the route -- a
    dedicated kernel that declined its shape would tick its own name and then the engine's."""
    dev = torch.device("cuda:0")
    off = []
    for path in (0, 1):
        case = L.Case(model, path, *L.GEOMETRY[15])
        g = L.stage_geometry(case)
        x, dy = L.inputs(case, 0)
        eng = _engine(case, dev)
        try:
            eng.bind_grads()
            xt, dyt = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(dy)).to(dev)
            for form, opts in L.infer_forms(case).items():
                _set(eng, opts)
                got = _ticks(eng, lambda: eng.stage_path(0, path, xt))
                want = L.expected_ticks(case, form, "infer")
                if got != want:
                    off.append((case.id, "infer", form, got, want))
            for form, opts in L.train_forms(case).items():
                _set(eng, opts)
                got = _ticks(eng, lambda: eng.train_path_forward(0, path, xt))
                if got != L.expected_ticks(case, form, "train_forward"):
                    off.append((case.id, "train_forward", form, got, L.expected_ticks(case, form, "train_forward")))
                y, tape = eng.train_path_forward(0, path, xt)
                got = _ticks(eng, lambda: eng.train_path_backward(0, path, xt, dyt, tape))
                if got != L.expected_ticks(case, form, "train_backward"):
                    off.append((case.id, "train_backward", form, got, L.expected_ticks(case, form, "train_backward")))
        finally:
            eng.close()
    assert not off, off


def test_tape_tap_refuses_what_the_tape_does_not_hold():
    dev = torch.device("cuda:0")
    case = L.Case("dptn128", 0, *L.GEOMETRY[15])
    eng = _engine(case, dev)
    try:
        x = torch.from_numpy(np.array(L.inputs(case, 0)[0])).to(dev)
        y, tape = eng.train_path_forward(0, 0, x)
        with pytest.raises(RuntimeError, match="unknown tape tensor 'gates'"):
            eng.tape_tap(tape, "gates", 1, 3)
        y1 = eng.tape_tap(tape, "y1", 1, 3)
        assert y1.numel() == 15 * 128 and y1.dtype == torch.float32
        assert eng.tape_tap(tape, "rs2", 1, 3).numel() == 15
    finally:
        eng.close()


def test_zz_worst_ratios_and_coverage():
    """The worst kernel-to-restatement ratio per (kernel, regime, tensor) (DESIGN.md section 31 quotes them), and: every
    (kernel instantiation, tail residue, regime) of the coverage table ran."""
    for (kernel, regime, tensor), (ratio, w, y, cid, form) in sorted(WORST.items()):
        print(f"worst ratio, {kernel}, {regime}, {tensor}: {ratio:.2f} ({w:.3g} against the restatement's {y:.3g}) at {cid} {form}")
    if len(STARTED) == len(L.CASES):      # (a selection of cases, -k, reports its figures only)
        want = L.coverage_table()
        assert not want - RAN, sorted(want - RAN)
        assert len(L.LEFT_OUT) <= 2
