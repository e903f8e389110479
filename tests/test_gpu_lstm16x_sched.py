"""lstm16x128_kernel: the step loop with hand-issued LDS reads (engine option lstm_sched = 1, the default) against the loop before
that (0).  The two issue the same MFMAs per accumulator in the same order, so a forward must agree BIT FOR BIT on both outputs.

The fused kernel is forced at any batch as tests/test_gpu_parity.py does (lstm4 = 0, fuse_pre128 = 2) on a 2-block DPTN-AV
model: every forward runs the kernel for both paths of both blocks and in both directions (the model is bidirectional), on
recurrences of length K = 150 (intra-chunk path) and S (inter-chunk path: S chunks of 150 frames at step 75, L = (T - 7) // 3 + 1
frames).  The engine needs L >= chunk_size, i.e. T >= 454; the smallest inputs it accepts for S = 1, 2, 3 are T = 454, 679, 904.

(The first version of the new loop missed this test by 1.9e-6: not the schedule, but `c = f * c + i * g` contracted to another
FMA for accumulator rows 2 and 3 once the cell update stood in a lambda.  Both loops now compute fma(f, c, i * g), written out.)"""
import pytest
import torch

from speech_separation_amd.spec import DPTN_AV, DPTNConfig, synthetic_inputs, synthetic_state_dict

pytestmark = pytest.mark.gpu

CFG = DPTNConfig(**{**DPTN_AV.to_dict(), "num_blocks": 2})


@pytest.fixture(scope="module")
def engine():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    from speech_separation_amd.engine import DptnEngine, params_to_device
    dev = torch.device("cuda:0")
    eng = DptnEngine(CFG, dev)
    eng.bind(params_to_device(synthetic_state_dict(CFG, seed=0), dev))
    eng.set_option("lstm4", 0)
    eng.set_option("fuse_pre128", 2)      # the fused kernel whatever the batch (the default starts at B = 12)
    return eng, dev


# B, T -> recurrence lengths (intra 150, inter S) and sequence counts (intra B S, inter 150 B; tiles of 16)
CASES = [
    (5, 9000),      # S = 38; 190 and 750 sequences: neither a multiple of 16, the last tile is padded
    (1, 454),       # S = 1: the single step is the one written out behind the loop; the x prefetch of step + 2 clamps twice
    (2, 679),       # S = 2: one trip through the loop, then the last step; the h / x buffers change places once
    (3, 904),       # S = 3: two trips: both buffer parities inside the loop
    (3, 1354),      # S = 5: a length >= 5, odd
]


@pytest.mark.parametrize("B,T", CASES, ids=[f"B{b}_T{t}" for b, t in CASES])
def test_sched_0_and_1_are_bit_identical(engine, B, T):
    eng, dev = engine
    assert CFG.chunks(CFG.frames(T)) == {9000: 38, 454: 1, 679: 2, 904: 3, 1354: 5}[T]
    t = {k: torch.from_numpy(v).to(dev) for k, v in synthetic_inputs(CFG, B=B, T=T, Tv=50, seed=71).items()}
    out = {}
    for sched in (0, 1):
        eng.set_option("lstm_sched", sched)
        s1, s2 = eng.forward(t["mix"], t["s1_embedding"], t["s2_embedding"])
        torch.cuda.synchronize()
        out[sched] = (s1.clone(), s2.clone())
    eng.set_option("lstm_sched", 1)
    for a, b in zip(out[0], out[1]):
        assert torch.isfinite(a).all() and a.abs().max() > 0
        assert torch.equal(a, b)
