"""The training-attention grid on the CPU (tests/train_attention_cases.py): the preconditions that make the GPU test's
per-token floor meaningful hold for every case, and the gap that floor closes is on record.

No GPU: everything here is the explicit formula of one TransformerDPRNN half under torch.autograd at fp64 and fp32."""
import pytest

from tests import train_attention_cases as A

OLD_Y_FLOOR_DB, OLD_DX_FLOOR_DB = 80.0, 70.0     # test_dropout_forward_and_backward_match_autograd_with_the_same_mask, whole tensors


def test_the_grid_covers_every_instantiation():
    """Every (features, NKB) runs on both paths with dropout off and on, once with a full last key block (len = 32 NKB) and once
    with one key in it (len = 32 (NKB - 1) + 1); the inter-chunk path also runs 32 NKB - 1, and lengths 1, 2 and 256 exist."""
    assert len(A.LENGTHS) == 25 and A.LENGTHS[:5] == [1, 2, 31, 32, 33] and A.LENGTHS[-2:] == [255, 256]
    assert len(A.PATH0_LENGTHS) == 16
    have = {tuple(c)[:4] for c in A.CASES if not c.chunk}
    assert sum(1 for c in A.CASES if c.chunk) == 2 and all(c.chunk == 1 and c.path == 1 and not c.ppm for c in A.CASES if c.chunk)
    assert len(have) + 2 == len(A.CASES) == 2 * (2 * 25 + 1 + 2 * 16 + 1 + 1)
    for features in A.FEATURES:
        for path in (0, 1):
            for nkb in range(1, 9):
                for ppm in (0, 100000):
                    assert (features, path, 32 * nkb, ppm) in have and (features, path, 32 * (nkb - 1) + 1, ppm) in have
                    assert path == 0 or (features, path, 32 * nkb - 1, ppm) in have
            assert (features, path, 256, 500000) in have
    assert all(k in have for k in A.SEED_OVERRIDES)


@pytest.mark.parametrize("case", A.CASES, ids=lambda c: c.id)
def test_preconditions_hold(case):
    """No ReLU input within 4e-7 of the kink, the fp32 restatement at 90 dB or better on every token of y and dx, and (dropout
    on, len >= 2) one inverted keep bit at 70 dB or worse on its worst token of y and of dx."""
    f = A.check_preconditions(case)
    print(case.id, " ".join(f"{k} {v:.3g}" if k == "min_relu" else f"{k} {v:.1f}" for k, v in f.items()))


@pytest.mark.parametrize("features", A.FEATURES)
@pytest.mark.parametrize("path", [0, 1])
@pytest.mark.parametrize("ln", [160, 256])
def test_one_inverted_keep_bit_passes_the_whole_tensor_floors_and_fails_the_token_floor(ln, path, features):
    """The gap on record: at 160 and 256 positions a result with one wrong keep bit clears the whole-tensor floors the dropout
    test of tests/test_gpu_backward.py applies to y (80 dB) and dx (70 dB), and misses the per-token floor of
    tests/test_gpu_train_attention.py.  If this stops being true the kit's shapes have drifted."""
    case = A.Case(features, path, ln, 100000)
    assert case in A.CASES
    ref, flipped = A.reference(case, 64), A.one_bit_flipped(case)
    y, dx = A.figures(flipped["y"], ref["y"]), A.figures(flipped["dx"], ref["dx"])
    param = min((A.O.agreement_db(flipped["grads"][k], ref["grads"][k]), k) for k in ref["grads"])
    print(f"{case.id}: one inverted keep bit: y {y[0]:.1f} dB, dx {dx[0]:.1f} dB, worst parameter {param[0]:.1f} dB ({param[1]}), "
          f"worst token y {y[1]:.1f} dB, dx {dx[1]:.1f} dB")
    assert y[0] > OLD_Y_FLOOR_DB and dx[0] > OLD_DX_FLOOR_DB
    assert y[1] < A.TOKEN_FLOOR_DB and dx[1] < A.TOKEN_FLOOR_DB
