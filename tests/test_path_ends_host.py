"""Host-side conditions of the path-ends tests (tests/path_ends_cases.py; the GPU half is tests/test_gpu_path_ends.py):
the case table says what it claims, the integer-valued operands are exact in fp32 in ANY summation order (a condition,
not a measurement: it is what makes `torch.equal` against the fp64 oracle a fair demand on a kernel), the fp32 restatements
give a non-zero yardstick for every judged tensor, and headtail.h's fast_div is floor division for every numerator it can
meet (its comment says so; nothing checked it)."""
from __future__ import annotations

import numpy as np
import pytest

from tests import path_ends_cases as C

LINEAR = [c.name for c in C.STAGE_CASES if not c.masked]
ALL = [c.name for c in C.STAGE_CASES + [C.MEMSAFETY_GEOMETRY]]


def test_the_table_covers_what_it_claims():
    every = C.STAGE_CASES + C.TRAIN_CASES
    for c in every:
        cfg = c.cfg()
        assert cfg.frames(c.T) == c.L and cfg.chunks(c.L) == c.S, c.name
        assert 0 <= c.left and c.left + c.ola <= c.L and c.pad_left >= 0, c.name
    for cases, kps in ((C.STAGE_CASES, {(20, 5), (21, 10), (20, 10), (20, 13), (20, 20), (9, 2), (5, 1), (150, 75)}),
                       (C.TRAIN_CASES, {(20, 5), (21, 10), (20, 13), (20, 20), (9, 2), (5, 1)})):
        assert {(c.K, c.P) for c in cases} == kps
        assert {c.N for c in cases} == {128, 64} and {c.B for c in cases} == {1, 2, 3}
        assert {c.arch for c in cases} == {"dptn", "dprnn", "dptn_mask"}
    assert {c.kenc for c in C.STAGE_CASES} == set(range(2, 9)) and {c.kenc for c in C.TRAIN_CASES} == set(range(2, 9))
    assert any(c.kenc == 7 and (c.K, c.P) == (150, 75) for c in C.STAGE_CASES)
    assert all(c.arch == "dprnn" for c in C.TRAIN_CASES if (c.K, c.P) in ((9, 2), (5, 1)))
    # both staging forms and the generic loop's odd K, per tail
    for masked in (False, True):
        sel = [c for c in C.STAGE_CASES if c.masked == masked]
        assert any(c.K > 2 * c.P and c.K % 2 for c in sel) and any(c.K > 2 * c.P and c.K % 2 == 0 for c in sel)
        assert any(c.K == 2 * c.P for c in sel) and any(c.K / 2 < c.P < c.K for c in sel) and any(c.P == c.K for c in sel)
        assert any(c.S == 1 for c in sel) and any(c.left > 0 for c in sel)
    # the kernels' own boundaries
    for N, frames in ((128, 64), (64, 128)):
        sel = [c for c in C.STAGE_CASES if c.N == N]
        assert any(c.L == c.K for c in sel) and any(c.L == 131 and c.L > frames for c in sel)
        assert any(c.B == 3 and (2 * c.B * c.L) % 32 for c in sel)
    assert any(c.L == 515 and c.B == 3 for c in C.TRAIN_CASES)                # past encoder_wgrad_kernel's 512-frame slab
    assert {(c.Cv, c.Tv) for c in C.STAGE_CASES if c.av} >= {(5, 1), (30, 2), (512, 65), (24, 70)}
    assert any(c.av and c.K == 20 and c.S == 1 and c.Tv == 50 for c in C.STAGE_CASES)          # Tv > L
    assert any(c.av and c.Tv == 256 for c in C.TRAIN_CASES) and any(c.av and c.Tv > c.L for c in C.TRAIN_CASES)
    m = C.MEMSAFETY_GEOMETRY
    assert (m.K, m.P, m.kenc, m.B, m.av) == (21, 5, 8, 3, True)
    from tests.memsafety_child import VARIANTS
    cfg, options, Bbig, T, Tv, Btrain = VARIANTS["path_ends"]
    assert cfg == m.cfg() and (options, Bbig, T, Tv, Btrain) == ({}, m.B, m.T, m.Tv, 2)


@pytest.mark.parametrize("name", LINEAR + [C.MEMSAFETY_GEOMETRY.name])
def test_integer_operands_are_exact_in_any_order(name):
    case = C.STAGE[name]
    sums = C.exactness(case)
    print(name, {k: v for k, v in sums.items()})
    assert all(v < C.EXACT_LIMIT for v in sums.values()), sums
    # the fp32 oracle equals the fp64 oracle bit for bit, in the reference's association and in the folded one
    cfg, sd, mix, x = C.exact_operands(case)
    want = C.exact_truth(name)
    h32 = C.head(cfg, sd, {"mix": mix}, np.float32)
    assert h32["enc"].dtype == np.float32
    for k in ("enc", "chunked"):
        assert np.array_equal(h32[k].astype(np.float64), want[k]), k
    for folded in (False, True):
        t32 = C.tail(cfg, sd, x, h32["enc"], case.T, np.float32, folded=folded)
        assert t32["taps"].dtype == np.float32
        for k in ("taps", "s1_pred", "s2_pred"):
            assert np.array_equal(t32[k].astype(np.float64), want[k]), (k, folded)
    # and the test has something to see: values of every size, few zeros, exact zeros where the geometry says so
    assert float(np.abs(want["taps"][..., :case.kenc]).max()) > 1000 and np.count_nonzero(want["taps"][..., :case.kenc]) > 0.9 * want["taps"][..., :case.kenc].size
    assert not want["taps"][..., case.kenc:].any()
    for k in ("s1_pred", "s2_pred"):
        assert not want[k][:, :case.pad_left].any() and not want[k][:, case.pad_left + case.ndec:].any()


@pytest.mark.parametrize("name", ALL)
def test_every_judged_tensor_has_a_yardstick(name):
    """The fp32 restatement's worst row is non-zero for every tensor the GPU tests judge (no row rule of `2 x 0`)."""
    case = C.STAGE[name]
    refs = C.value_refs(name)
    for k in ("enc", "chunked"):
        w, _ = C.worst_row(k, refs["h32"][k], refs["h64"][k])
        assert 0 < w < 1e-5, (k, w)
    t = C.tail_refs(case, refs["h32"]["enc"])
    for form in ("t32",) + (() if case.masked else ("t32f",)):
        for k in ("taps", "s1_pred", "s2_pred"):
            w, _ = C.worst_row(k, t[form][k], t["t64"][k])
            assert 0 < w < 1e-5, (form, k, w)
    pads = C.padded_frames(case)
    assert (len(pads) > 0) == (case.rL > 0)
    if len(pads):       # a padded frame's tap row is the bias-plus-skip value (the masked tail: the bias-only mask on the latent)
        assert np.allclose(t["t64"]["taps"][:, :, pads], t["t64"]["pad_taps"][None][:, :, pads], rtol=0, atol=1e-12)


@pytest.mark.parametrize("name", [c.name for c in C.TRAIN_CASES])
def test_training_inputs_stay_clear_of_the_ffn_relu_kink(name):
    case = C.TRAIN[name]
    for gate in (C.TRAIN_GATES if name == C.GATE_CASE else (0.7,)):
        m = C.ffn_kink_margin(case, gate)
        print(name, gate, m)
        assert m > C.KINK_MARGIN, (name, gate, m)


def test_gate_zero_is_the_encoder_conv_alone():
    name = next(c.name for c in C.STAGE_CASES if c.av)
    r = C.value_refs(name, 0.0)
    assert np.array_equal(r["h64"]["enc"], r["h64"]["conv"])


# ------------------------------------------------------------------------------------------------------------------
# fast_div
# ------------------------------------------------------------------------------------------------------------------
def test_fast_div_is_floor_division_below_2_to_23():
    """Every n < 2^23 for every divisor 1..256 (the float path of fast_div; larger n take the hardware division): the
    corrected quotient q satisfies 0 <= n - q d < d, which only floor(n / d) does; and the raw estimate is within one of it,
    which is what ONE correction step each way presumes."""
    block = 1 << 16                                      # numerators in cache-sized blocks, every divisor per block
    for n0 in range(0, 1 << 23, block):
        n = np.arange(n0, n0 + block, dtype=np.int32)
        nf = n.astype(np.float32)
        for d in range(1, 257):
            q = C.fast_div(n, d, nf)
            r = n - q * np.int32(d)
            assert int(r.min()) >= 0 and int(r.max()) < d, (n0, d)
    n = np.arange(1 << 23, dtype=np.int32)
    for d in (1, 3, 7, 75, 150, 255, 256):               # the same against // itself, on a few
        assert np.array_equal(C.fast_div(n, d), n // d), d


def test_fast_div_on_the_divisors_and_numerators_in_use():
    """Divisors are L and step_size; numerators are below 2 B L.  The table's L and P, and the BASELINE shapes' (L = 10665 at
    4 s / 8 kHz with kernel_size_enc 7, step_size 75; L = 15999 / step_size 125 for the DPRNN configuration), B up to 64."""
    pairs = {(c.L, c.B) for c in C.STAGE_CASES + C.TRAIN_CASES} | {(10665, 64), (15999, 64)}
    for L, B in sorted(pairs):
        n = np.arange(min(2 * B * L, 1 << 23), dtype=np.int32)
        assert np.array_equal(C.fast_div(n, L), n // L), L
    for P in sorted({c.P for c in C.STAGE_CASES + C.TRAIN_CASES} | {75, 125}):
        n = np.arange(16000, dtype=np.int32)
        assert np.array_equal(C.fast_div(n, P), n // P), P
