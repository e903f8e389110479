"""The inference-attention grid on the CPU (tests/infer_attention_cases.py): the grid reaches every kernel instantiation, the
preconditions that make the GPU test's per-token floors meaningful hold for every case, the gap those floors close is on
record, and the GPU test's own judging code rejects a result with one wrong key in one query row.

No GPU: everything here is the explicit formula of a TransformerDPRNN half and the numpy oracle at fp64 and fp32."""
import pytest

from tests import infer_attention_cases as I


def test_the_grid_covers_every_instantiation():
    """Every (family, NKB or NB, plain / prologue / persistent) of the five kernel families runs with one key and with all keys
    in its last key block, on both paths where the path exists (attention_long_kernel: the inter-chunk path only)."""
    assert len(I.FUSED) == 33 and I.FUSED[:4] == [1, 2, 15, 16] and I.FUSED[-1] == 160 and 141 in I.FUSED and 150 in I.FUSED
    assert I.MID == [161, 191, 192, 193, 223, 224, 225, 255, 256]
    assert [(ln + 31) // 32 for ln in I.LONG] == [9, 9, 9, 10, 10, 12, 13]
    assert len(I.PATH0_LENGTHS) == 27 and max(I.PATH0_LENGTHS) == 256
    assert len(I.CASES) == 2 * (33 + 9 + 7 + 27) and len(set(I.CASES)) == len(I.CASES)
    assert len(I.PRO_CASES) == 2 * (14 + 22) and not I.LEFT_OUT
    want, have = I.instantiations(), I.grid_coverage()
    assert len(want) == 2 * 2 * (5 * 3 + 5 * 2 + 10 * 2 + 2 * 8) + 4
    assert not want - have, sorted(want - have, key=str)
    assert not have - want, sorted(have - want, key=str)
    assert all(k in set(map(tuple, I.PRO_CASES)) for k in I.PRO_SEED_OVERRIDES)


@pytest.mark.parametrize("case", I.CASES + I.PRO_CASES, ids=lambda c: c.id)
def test_launch_geometry(case):
    """Before anything runs on a device: the sample count gives the chunk count the case names (and one more sample gives one
    more chunk, for the PRO cases), the sequence length under test is the case's, the fused forms stay at 160 positions or
    fewer, chunk_size at 256 or fewer, and the floats read from a tap are the M * N the plan gives it."""
    g = I.stage_geometry(case) if isinstance(case, I.Case) else I.pro_geometry(case)
    assert g["B"] == 1 and g["M"] == g["S"] * g["K"] and g["tap_floats"] == g["M"] * case.features
    assert case.len == (g["S"] if case.path == 1 else g["K"]) and 3 == (g["K"] if case.path == 1 else g["S"])
    assert g["T"] >= 7 and g["M"] <= 3 * 385


@pytest.mark.parametrize("case", I.CASES, ids=lambda c: c.id)
def test_stage_preconditions_hold(case):
    """The fp32 restatement at 130 dB or better on every token of y1, 120 dB on every token of att (fp32 cannot reach 130 there:
    the kit's header) and 90 dB on every token of y; with len >= 2 either defect leaves the worst token of y1 at 80 dB or below."""
    f = I.check_preconditions(case)
    print(case.id, " ".join(f"{k} {v:.1f}" for k, v in f.items()))


@pytest.mark.parametrize("case", I.PRO_CASES, ids=lambda c: c.id)
def test_pro_preconditions_hold(case):
    """The fp32 restatement of the whole forward at 100 dB or better on every token of the final y1; the recomputation from the
    defective path's input tap reproduces the oracle; with len >= 2 either defect in the attention under test -- for the
    intra kind block 1's intra-chunk attention, one attention half before the judged one -- reaches the final y1 at 80 dB or
    below on its worst token: THE CHAIN carries it below the PRO floor."""
    f = I.check_pro_preconditions(case)
    print(case.id, " ".join(f"{k} {v:.1f}" for k, v in f.items()))
    if case.len >= 2:
        assert max(f[f"{d}.y1.token"] for d in I.DEFECTS) < I.PRO_FLOOR_DB


@pytest.mark.parametrize("features", I.FEATURES)
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("ln", [160, 256])
def test_one_wrong_key_passes_the_whole_tensor_floor_and_fails_the_token_floor(ln, path, features):
    """The gap on record: at 160 and 256 positions y1 with ONE wrong key in ONE softmax row clears the 80 dB whole-tensor bar that
    guarded these kernels (the better hidden of the two defects: 82.2 dB or more; the other one too except at 64 features /
    path 1 / len 160, where key 0 counted twice stands at 79.7 dB), and both defects miss the per-token floor by 30 dB or more.
    If this stops being true the kit's shapes have drifted."""
    case = I.Case(features, path, ln)
    assert case in I.CASES
    fig = {d: I.figures(I.reference(case, 64, d)["y1"], I.reference(case, 64)["y1"]) for d in I.DEFECTS}
    print(f"{case.id}: " + "; ".join(f"{d}: y1 {f[0]:.1f} dB over the whole tensor, {f[1]:.1f} dB at token {f[2]}" for d, f in fig.items()))
    assert max(f[0] for f in fig.values()) > I.OLD_FLOOR_DB
    assert all(f[1] <= I.DEFECT_CEILING_DB < I.STAGE_FLOOR_DB for f in fig.values())


@pytest.mark.parametrize("case", [c for c in I.CASES if c.len >= 2], ids=lambda c: c.id)
def test_the_judging_code_fails_a_result_with_one_wrong_key(case):
    """The tests can fail: the formula with the one-key defect, handed to the GPU test's judging code in place of a kernel
    result, misses the floor at every length >= 2; the fp32 restatement handed to it passes."""
    ref = I.reference(case, 64)
    with pytest.raises(AssertionError, match="worst token"):
        I.judge("y1", I.reference(case, 64, "key0_twice")["y1"], ref["y1"], I.STAGE_FLOOR_DB)
    with pytest.raises(AssertionError, match="worst token"):
        I.judge("att", I.reference(case, 64, "key0_twice")["att"], ref["att"], I.STAGE_FLOOR_DB)
    for key, floor in (("y1", I.STAGE_FLOOR_DB), ("att", I.STAGE_FLOOR_DB), ("y", I.Y_FLOOR_DB)):
        I.judge(key, I.reference(case, 32)[key], ref[key], floor)


@pytest.mark.parametrize("case", [c for c in I.PRO_CASES if c.len >= 2], ids=lambda c: c.id)
def test_the_judging_code_fails_a_chain_with_one_wrong_key(case):
    ref = I.pro_reference(case, 64)
    with pytest.raises(AssertionError, match="worst token"):
        I.judge("y1", I.pro_defective(case, "key0_twice"), ref, I.PRO_FLOOR_DB)
    I.judge("y1", I.pro_reference(case, 32), ref, I.PRO_FLOOR_DB)
