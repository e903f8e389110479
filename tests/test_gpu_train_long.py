"""Training attention beyond 256 positions on the GPU (option train_long_seq, attn_long_train.h): the streaming forward with
its softmax tape and dropout, and the two tiled backward launches.

  * train_long_seq = 1, the grid of tests/train_long_cases.py (9 .. 17 key blocks, both widths, dropout off / 0.1 / 0.5)
    against the fp64 formula, judged on EVERY TOKEN of y and dx, with the floors of tests/train_attention_cases.py;
  * train_long_seq = 2 (the streaming trio at every length) on cases of the existing kit, against fp64 and against the
    on-chip kernels' y on the same input;
  * the whole model at S = 257 against fp64 autograd on the stock composition, through the engine and through the nn.Module
    (keyword long_training), deterministic mode, and option 0 left as it was.
"""
import numpy as np
import pytest
import torch

from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTN_AUDIO, DPTN_AV, DPTNConfig, synthetic_inputs, synthetic_state_dict
from tests import train_attention_cases as A
from tests import train_long_cases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    return torch.device("cuda:0")


def _engine(case, dev, long_seq):
    from speech_separation_amd.engine import DptnEngine, params_to_device
    eng = DptnEngine(A.config(case.features, case.path, case.len, case.chunk), dev)
    eng.bind(params_to_device({k: np.array(v) for k, v in A.weights(case.features, case.path, case.len, case.chunk).items()}, dev))
    grads = eng.bind_grads()
    eng.set_option("dropout_ppm", case.ppm)
    eng.set_option("dropout_seed", A.DROPOUT_SEED)
    eng.set_option("train_long_seq", long_seq)
    return eng, grads


def _judge(case, ref, ref32, y_np, dx_np, g_np):
    """Prints every figure, then asserts the per-token floor of y and dx and the floor of every parameter gradient."""
    fig = {k: (A.figures(got, ref[k]), A.figures(ref32[k], ref[k])) for k, got in (("y", y_np), ("dx", dx_np))}
    par = min((O.agreement_db(g_np[leaf], ref["grads"][leaf]), leaf) for leaf in g_np)
    print(f"{case.id}: " + "; ".join(
        f"{k} {f[0]:.1f} dB, worst token {f[1]:.1f} dB at {f[2]} (fp32 restatement {r[0]:.1f} / {r[1]:.1f} at {r[2]})"
        for k, (f, r) in fig.items()) + f"; worst parameter {par[1]} {par[0]:.1f} dB")
    for k, (f, r) in fig.items():
        assert f[1] >= A.TOKEN_FLOOR_DB, (case.id, k, "worst token", f[1], f[2], "fp32 restatement", r[1])
    for leaf in g_np:
        assert g_np[leaf].shape == ref["grads"][leaf].shape, leaf
        db = O.agreement_db(g_np[leaf], ref["grads"][leaf])
        assert db >= A.PARAM_FLOOR_DB, (case.id, leaf, db)


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.id)
def test_long_training_attention_matches_the_fp64_formula_on_every_token(dev, case):
    """train_long_seq = 1.  In this order: the device keep mask equals tests/dropout_ref.keep_mask bit for bit (dropout on);
    everything is finite and the training forward equals the inference forward to 120 dB (dropout off); y and dx reach 80 dB
    on every token; every parameter gradient of the path reaches 70 dB; two forwards and two backwards with the same seed are
    bitwise equal."""
    L.check_preconditions(case)
    B, S, K, N = A.shape(case)
    x, dy = L.inputs(case)
    ref, ref32 = L.reference(case, 64), L.reference(case, 32)
    eng, grads = _engine(case, dev, 1)
    try:
        xt, dyt = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(dy)).to(dev)
        y, tape = eng.train_path_forward(0, 1, xt)
        dx = eng.train_path_backward(0, 1, xt, dyt, tape)
        torch.cuda.synchronize()
        y_np, dx_np = y.cpu().numpy(), dx.cpu().numpy()
        g_np = {leaf: grads[A.prefix(case) + leaf].cpu().numpy() for leaf in ref["grads"]}
        if case.ppm:
            assert np.array_equal(eng.dropout_mask(0, 1, B, S).cpu().numpy(), A.mask(case)), "keep mask"
        assert np.isfinite(y_np).all() and np.isfinite(dx_np).all() and all(np.isfinite(g).all() for g in g_np.values())
        if not case.ppm:
            assert O.agreement_db(y_np, eng.stage_path(0, 1, xt).cpu().numpy()) > 120, "training forward == inference forward"
        _judge(case, ref, ref32, y_np, dx_np, g_np)
        y2, tape2 = eng.train_path_forward(0, 1, xt)
        dx2 = eng.train_path_backward(0, 1, xt, dyt, tape2)
        torch.cuda.synchronize()
        assert torch.equal(y2, y), "two training forwards with the same dropout seed differ"
        assert torch.equal(dx2, dx), "two backwards with the same dropout seed differ"
    finally:
        eng.close()


FORCED_LENGTHS = (1, 2, 33, 160, 255, 256)
FORCED_CASES = [c for c in A.CASES if c.len in FORCED_LENGTHS and c.ppm in (0, 100000) and not c.chunk]


def test_the_forced_cases_cover_both_paths_and_widths():
    assert {(c.path, c.len) for c in FORCED_CASES} == {(1, ln) for ln in FORCED_LENGTHS} | {(0, ln) for ln in (1, 33, 160, 256)}
    assert all({c.ppm for c in FORCED_CASES if (c.features, c.path, c.len) == (f, p, ln)} == {0, 100000}
               for f in (128, 64) for (p, ln) in {(c.path, c.len) for c in FORCED_CASES})


@pytest.mark.parametrize("case", FORCED_CASES, ids=lambda c: c.id)
def test_forced_streaming_kernels_match_fp64_and_the_on_chip_kernels(dev, case):
    """train_long_seq = 2: the streaming trio at a length the on-chip trio takes too, on the existing kit's inputs -- the same
    per-token and parameter floors against fp64, and y > 120 dB against the default kernels' y."""
    A.check_preconditions(case)
    x, dy = A.inputs(case)
    ref, ref32 = A.reference(case, 64), A.reference(case, 32)
    xt, dyt = torch.from_numpy(np.array(x)).to(dev), torch.from_numpy(np.array(dy)).to(dev)
    eng, _ = _engine(case, dev, 0)
    try:
        y_default, _tape = eng.train_path_forward(0, case.path, xt)
        torch.cuda.synchronize()
        y_default = y_default.cpu().numpy()
    finally:
        eng.close()
    eng, grads = _engine(case, dev, 2)
    try:
        y, tape = eng.train_path_forward(0, case.path, xt)
        dx = eng.train_path_backward(0, case.path, xt, dyt, tape)
        torch.cuda.synchronize()
        y_np, dx_np = y.cpu().numpy(), dx.cpu().numpy()
        g_np = {leaf: grads[A.prefix(case) + leaf].cpu().numpy() for leaf in ref["grads"]}
        assert np.isfinite(y_np).all() and np.isfinite(dx_np).all() and all(np.isfinite(g).all() for g in g_np.values())
        _judge(case, ref, ref32, y_np, dx_np, g_np)
        db = O.agreement_db(y_np, y_default)
        print(f"{case.id}: streaming y against on-chip y {db:.1f} dB")
        assert db > 120, (case.id, "streaming y against the on-chip kernels' y", db)
    finally:
        eng.close()


# ---- whole model at S = 257 ---------------------------------------------------------------------------------------------
def _cfg257(features, dropout=0.0):
    """The configuration of tests/test_gpu_backward._chunk_limit_cfg: chunk 20, step 10, one block; T = 7744 samples are 257 chunks."""
    cfg = DPTNConfig(**{**(DPTN_AV if features == 128 else DPTN_AUDIO).to_dict(), "num_blocks": 1, "dropout": dropout,
                        "chunk_size": 20, "step_size": 10})
    assert cfg.chunks(cfg.frames(7744)) == 257
    return cfg


B257, T257 = 2, 7744


def _model_step(eng, t, d1, d2):
    args = (t["mix"], t.get("s1_embedding"), t.get("s2_embedding"))
    s1, s2, tape = eng.train_forward(*args)
    eng.train_backward(*args, d1, d2, tape)
    torch.cuda.synchronize()
    return s1, s2


@pytest.mark.parametrize("features", [128, 64])
def test_whole_model_backward_at_257_chunks_matches_autograd(dev, features):
    """S = 257, one chunk past the on-chip kernels, B = 2: d loss / d every parameter against fp64 autograd on the stock
    composition, to the floor of test_whole_model_backward_at_256_chunks_matches_autograd.  (Input seeds 2 / 8: the smallest
    ReLU input of the fp64 run is 3.0e-7 / 1.7e-7, above that test's 1e-7.)"""
    from speech_separation_amd.engine import DptnEngine, params_to_device
    from tests.test_gpu_fuzz import stock_gradients
    cfg = _cfg257(features)
    sd = synthetic_state_dict(cfg, seed=2)
    eng = DptnEngine(cfg, dev)
    eng.bind(params_to_device(sd, dev))
    grads = eng.bind_grads()
    eng.set_option("train_long_seq", 1)
    assert eng.chunks(T257) == 257
    inp = synthetic_inputs(cfg, B=B257, T=T257, Tv=9, seed=2 if features == 128 else 8)
    t = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    rng = np.random.default_rng(3)
    d1 = rng.standard_normal((B257, T257)).astype(np.float32)
    d2 = rng.standard_normal((B257, T257)).astype(np.float32)
    _model_step(eng, t, torch.from_numpy(d1).to(dev), torch.from_numpy(d2).to(dev))
    want = stock_gradients(cfg, sd, inp, d1, d2)
    kink = want.pop("__smallest_relu_input__")
    assert kink > 1e-7, kink
    missing = [k for k in grads if k not in want]
    assert not missing, missing
    worst = min((O.agreement_db(grads[k].cpu().numpy(), want[k].numpy().reshape(grads[k].shape)), k) for k in grads)
    print(f"{features} features, S = 257: worst parameter {worst[1]} {worst[0]:.1f} dB (smallest ReLU input {kink:.1e})")
    assert worst[0] > 60, worst


@pytest.mark.parametrize("features", [128, 64])
def test_module_trains_at_257_chunks_with_the_keyword_and_raises_without(dev, features):
    """DPTNWavEncDec / DPTNAVWavEncDec(long_training=True), dropout 0.1, model.train(): loss.backward() leaves finite gradients,
    and the step replayed through the engine with the options the module's backward left set -- one seed for forward and
    backward -- gives bit-identical outputs and gradients (deterministic tile order): the module's backward used its forward's
    mask.  Without the keyword the module raises as before."""
    from speech_separation_amd.engine import DptnEngine
    from speech_separation_amd.model import DPTNAVWavEncDec, DPTNWavEncDec
    cfg = _cfg257(features, dropout=0.1)
    kw = dict(num_features=cfg.num_features, kernel_size_enc=cfg.kernel_size_enc, hidden_dim=cfg.hidden_dim, num_blocks=1,
              chunk_size=20, step_size=10, num_heads=cfg.num_heads, dropout=0.1, bidir=cfg.bidir)
    if features == 128:
        make = lambda **more: DPTNAVWavEncDec(video_emb_size=cfg.video_emb_size, hidden_video=cfg.hidden_video, **kw, **more)   # noqa: E731
    else:
        make = lambda **more: DPTNWavEncDec(**kw, **more)   # noqa: E731
    sd = {k: torch.from_numpy(v) for k, v in synthetic_state_dict(cfg, seed=2).items()}
    inp = synthetic_inputs(cfg, B=B257, T=T257, Tv=9, seed=5)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")}
    g = torch.Generator(device="cpu").manual_seed(1)
    d1, d2 = torch.randn(B257, T257, generator=g).to(dev), torch.randn(B257, T257, generator=g).to(dev)

    plain = make()
    assert plain.long_training is False
    plain.load_state_dict(sd)
    plain = plain.to(dev).train()
    with pytest.raises(RuntimeError, match="at most 256 chunks"):
        plain(**batch)
    with torch.no_grad(), pytest.raises(RuntimeError, match="at most 256 chunks"):
        plain(**batch)

    model = make(long_training=True)
    assert model.long_training is True
    model.load_state_dict(sd)
    model = model.to(dev).train()
    eng = model._get_engine(dev)
    assert eng.options_set.get("train_long_seq") == 1
    eng.set_option("deterministic", 1)
    out = model(**batch)
    (out["s1_pred"] * d1 + out["s2_pred"] * d2).sum().backward()
    torch.cuda.synchronize()
    got = {k: p.grad.detach().clone() for k, p in model.named_parameters()}
    assert all(torch.isfinite(v).all() for v in got.values())
    assert any(float(v.abs().max()) > 0 for v in got.values())
    ppm, seed = eng.options_set["dropout_ppm"], eng.options_set["dropout_seed"]
    assert ppm == 100000

    replay = DptnEngine(cfg, dev)
    replay.bind({k: p.detach() for k, p in model.named_parameters()})
    rgrads = replay.bind_grads()
    for k, v in (("train_long_seq", 1), ("deterministic", 1), ("dropout_ppm", ppm), ("dropout_seed", seed)):
        replay.set_option(k, v)
    s1, s2 = _model_step(replay, batch, d1, d2)
    assert torch.equal(s1, out["s1_pred"]) and torch.equal(s2, out["s2_pred"])
    for k in got:
        assert torch.equal(rgrads[k].view_as(got[k]), got[k]), k
    # ... and the mask matters: another seed in the backward alone changes the gradients
    args = (batch["mix"], batch.get("s1_embedding"), batch.get("s2_embedding"))
    s1, s2, tape = replay.train_forward(*args)
    replay.set_option("dropout_seed", seed ^ 1)
    replay.train_backward(*args, d1, d2, tape)
    torch.cuda.synchronize()
    assert any(not torch.equal(rgrads[k].view_as(got[k]), got[k]) for k in got)
    # a train-mode forward under no_grad takes the same path (dropout without a backward)
    with torch.no_grad():
        o2 = model(**batch)
    torch.cuda.synchronize()
    assert torch.isfinite(o2["s1_pred"]).all() and torch.isfinite(o2["s2_pred"]).all()
    # a device move makes a new engine: the option is set on it too
    model._engine = None
    assert model._get_engine(dev).options_set.get("train_long_seq") == 1


def test_dprnn_modules_take_no_long_training_keyword():
    from speech_separation_amd.model import DPRNNEncDec, DPTNEncDec
    with pytest.raises(TypeError):
        DPRNNEncDec(long_training=True)
    assert DPTNEncDec(long_training=True).long_training is True and DPTNEncDec().long_training is False


@pytest.mark.parametrize("features", [128, 64])
def test_whole_model_step_at_257_chunks_is_deterministic(dev, features):
    """deterministic = 1, dropout 0.1: the whole-model step at S = 257 run twice gives bit-identical outputs and flat gradients."""
    from speech_separation_amd.engine import DptnEngine, params_to_device
    cfg = _cfg257(features)
    eng = DptnEngine(cfg, dev)
    eng.bind(params_to_device(synthetic_state_dict(cfg, seed=1), dev))
    eng.bind_grads()
    for k, v in (("train_long_seq", 1), ("deterministic", 1), ("dropout_ppm", 100000), ("dropout_seed", 2024)):
        eng.set_option(k, v)
    t = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_inputs(cfg, B=B257, T=T257, Tv=9, seed=2).items()}
    g = torch.Generator(device="cpu").manual_seed(0)
    d1, d2 = torch.randn(B257, T257, generator=g).to(dev), torch.randn(B257, T257, generator=g).to(dev)
    runs = []
    for _ in range(2):
        s1, s2 = _model_step(eng, t, d1, d2)
        runs.append((s1.clone(), s2.clone(), eng._grads_flat.clone()))
    assert torch.isfinite(runs[0][2]).all()
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    assert torch.equal(runs[0][2], runs[1][2])


@pytest.mark.parametrize("features", [128, 64])
def test_option_zero_is_inert(dev, features):
    """train_long_seq = 0 (the default, and set back after 1): at S = 257 the size queries, the whole-model forward and the
    path-level entry point refuse with the text they had, dropout armed.  (The attention launcher's own "dropout needs sequence
    length <= 256" sits behind these checks at every entry point: with option 0 nothing reaches it, which is what
    tests/test_gpu_backward.py pins; its wording is unchanged up to the clause naming the option.)"""
    from speech_separation_amd.engine import DptnEngine, params_to_device
    cfg = _cfg257(features)
    eng = DptnEngine(cfg, dev)
    eng.bind(params_to_device(synthetic_state_dict(cfg, seed=1), dev))
    eng.bind_grads()
    eng.set_option("dropout_ppm", 100000)
    eng.set_option("dropout_seed", 7)
    t = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_inputs(cfg, B=B257, T=T257, Tv=9, seed=2).items()}
    args = (t["mix"], t.get("s1_embedding"), t.get("s2_embedding"))
    x = torch.randn(1, 257, cfg.chunk_size, cfg.num_features, device=dev)
    for value in (None, 1, 0):
        if value is not None:
            eng.set_option("train_long_seq", value)
        if value == 1:
            s1, s2, _tape = eng.train_forward(*args)
            torch.cuda.synchronize()
            assert torch.isfinite(s1).all() and torch.isfinite(s2).all()
            continue
        with pytest.raises(RuntimeError, match="at most 256 chunks"):
            eng.train_forward(*args)
        with pytest.raises(RuntimeError, match="at most 256 chunks"):
            eng.train_path_forward(0, 1, x)
    with pytest.raises(RuntimeError):
        eng.set_option("train_long_seq", 3)
