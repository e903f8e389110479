"""The inputs of the long-sequence training-attention tests (tests/train_long_cases.py), checked on the CPU before any kernel
result is looked at: the three preconditions of tests/train_attention_cases.check_preconditions with its bounds, on every
case of the new grid with the new seeds, and the grid's coverage."""
import pytest

from tests import train_attention_cases as A
from tests import train_long_cases as L


def test_the_grid_covers_the_block_counts_both_widths_and_dropout():
    assert {c.len: c.nkb for c in L.CASES} == {257: 9, 288: 9, 289: 10, 385: 13, 513: 17}
    assert all(c.path == 1 and not c.chunk and A.shape(c) == (1, c.len, 3, c.features) for c in L.CASES)
    for features in (128, 64):
        for ln in L.LENGTHS:
            ppms = {c.ppm for c in L.CASES if c.features == features and c.len == ln}
            assert ppms == ({0, 100000, 500000} if ln == 385 else {0, 100000}), (features, ln, ppms)
    assert len(L.CASES) == 22 and set(L.SEEDS) == {(c.features, c.len, c.ppm) for c in L.CASES}
    # every seed follows the search rule: 1000 + len, + 10000, ...
    assert all((seed - 1000 - ln) % 10000 == 0 and seed >= 1000 + ln for (_, ln, _), seed in L.SEEDS.items())
    # beyond what the on-chip kernels are instantiated for, and past a 16-block or 512-row assumption
    assert min(c.nkb for c in L.CASES) > 8 and max(c.nkb for c in L.CASES) > 16 and max(c.len for c in L.CASES) > 512
    # the existing kit's seed table is not touched
    assert not any(k[2] > 256 for k in A.SEED_OVERRIDES)


@pytest.mark.parametrize("case", L.CASES, ids=lambda c: c.id)
def test_preconditions_hold_for_every_long_case(case):
    fig = L.check_preconditions(case)
    print(f"{case.id} seed {L.input_seed(case)}: " + ", ".join(f"{k} {v:.3g}" for k, v in fig.items()))
