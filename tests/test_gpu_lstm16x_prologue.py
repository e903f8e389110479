"""lstm16x.hip: the prologue that fetches its weights in one burst from a packed, pre-scaled copy (engine option
lstm_prologue = 1, the default) against the prologue before it (0: every lane reads its rows of the nn.LSTM tensors and scales
them).  The packed copy holds the products of the same fp32 multiplies, the kernels keep them in the same registers and the step
loops are the same code, so a forward must agree BIT FOR BIT on both outputs.

Shapes and model are those of tests/test_gpu_lstm16x_sched.py (2-block DPTN-AV, lstm4 = 0, fuse_pre128 = 2: the fused kernel runs
for both paths of both blocks, both directions, recurrences of length 150 and S = 38, 1, 2, 3, 5, padded last tiles); the
64-feature kernel runs in a 2-block DPTN audio-only model (fuse_pre, on by default; lstm4 = 0 keeps small launches on it).

The copy is made by a launch of its own at the first fused recurrence of every pass, from the weights as they are then: a
parameter changed in place between two calls must show in the second (test_weights_are_read_per_call)."""
import pytest
import torch

from speech_separation_amd.spec import DPTN_AUDIO, DPTN_AV, DPTNConfig, synthetic_inputs, synthetic_state_dict

pytestmark = pytest.mark.gpu

CFG = DPTNConfig(**{**DPTN_AV.to_dict(), "num_blocks": 2})
CFG64 = DPTNConfig(**{**DPTN_AUDIO.to_dict(), "num_blocks": 2})


def _engine(cfg):
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from speech_separation_amd.engine import DptnEngine, params_to_device
    dev = torch.device("cuda:0")
    eng = DptnEngine(cfg, dev)
    params = params_to_device(synthetic_state_dict(cfg, seed=0), dev)
    eng.bind(params)
    eng.set_option("lstm4", 0)
    return eng, dev, params


@pytest.fixture(scope="module")
def engine():
    eng, dev, params = _engine(CFG)
    eng.set_option("fuse_pre128", 2)      # the fused kernel whatever the batch (the default starts at B = 12)
    return eng, dev, params


@pytest.fixture(scope="module")
def engine64():
    assert CFG64.num_features == 64
    return _engine(CFG64)


def _inputs(cfg, dev, B, T):
    t = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_inputs(cfg, B=B, T=T, Tv=50, seed=71).items()}
    return (t["mix"], t.get("s1_embedding"), t.get("s2_embedding"))


def _forward(eng, args, prologue):
    eng.set_option("lstm_prologue", prologue)
    try:
        s1, s2 = eng.forward(*args)
        torch.cuda.synchronize()
        return s1.clone(), s2.clone()
    finally:
        eng.set_option("lstm_prologue", 1)


def _assert_identical(a, b):
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and x.abs().max() > 0
        assert torch.equal(x, y)


# B, T -> recurrence lengths (intra 150, inter S) and sequence counts (intra B S, inter 150 B; tiles of 16)
CASES = [(5, 9000), (1, 454), (2, 679), (3, 904), (3, 1354)]


@pytest.mark.parametrize("B,T", CASES, ids=[f"B{b}_T{t}" for b, t in CASES])
def test_prologue_0_and_1_are_bit_identical(engine, B, T):
    eng, dev, _ = engine
    assert CFG.chunks(CFG.frames(T)) == {9000: 38, 454: 1, 679: 2, 904: 3, 1354: 5}[T]
    args = _inputs(CFG, dev, B, T)
    _assert_identical(_forward(eng, args, 0), _forward(eng, args, 1))


def test_prologue_0_and_1_are_bit_identical_with_the_loop_before(engine):
    eng, dev, _ = engine
    args = _inputs(CFG, dev, 3, 904)
    eng.set_option("lstm_sched", 0)
    try:
        _assert_identical(_forward(eng, args, 0), _forward(eng, args, 1))
    finally:
        eng.set_option("lstm_sched", 1)


@pytest.mark.parametrize("B,T", [(1, 454), (5, 9000)], ids=["B1_T454", "B5_T9000"])
def test_prologue_0_and_1_are_bit_identical_64_features(engine64, B, T):
    eng, dev, _ = engine64
    args = _inputs(CFG64, dev, B, T)
    _assert_identical(_forward(eng, args, 0), _forward(eng, args, 1))


def test_weights_are_read_per_call(engine):
    eng, dev, params = engine
    args = _inputs(CFG, dev, 2, 679)
    first = _forward(eng, args, 1)
    k_hh = sorted(k for k in params if k.endswith("rnn.weight_hh_l0"))[0]
    k_ih = sorted(k for k in params if k.endswith("rnn.weight_ih_l0_reverse"))[-1]
    saved = {k: params[k].clone() for k in (k_hh, k_ih)}
    try:
        params[k_hh].mul_(1.25)
        params[k_ih].mul_(0.75)
        second = _forward(eng, args, 1)
        reference = _forward(eng, args, 0)
    finally:
        for k, v in saved.items():
            params[k].copy_(v)
        torch.cuda.synchronize()
    for a, b in zip(first, second):
        assert not torch.equal(a, b)
    _assert_identical(reference, second)
