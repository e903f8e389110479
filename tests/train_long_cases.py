"""TEST INFRASTRUCTURE: the cases of the long-sequence training-attention tests (option train_long_seq) and their CPU
references, computed once per process and shared, read-only, by tests/test_train_long_host.py and
tests/test_gpu_train_long.py.  Built on tests/train_attention_cases.py (formula, mask, figures, floors); the seed table is
this module's own.

The streaming trio of attn_long_train.h walks 32-key blocks at run time, four query blocks per workgroup in the backward
and query blocks w, w + 4, ... per wave in the forward:

  len   key blocks
  257   9    one key in the last block, odd count
  288   9    nine full blocks
  289   10   even count, one key in the last
  385   13   uneven query blocks per wave
  513   17   past any 512-row or 16-block assumption

Inter-chunk path only (chunk_size 3, step 1, B = 1: 3 sequences of `len` positions, token stride 3; the intra-chunk
sequence is a chunk, at most 256).  Features 128 and 64; dropout off and 0.1, plus 0.5 at len 385.

Input seeds: the first of 1000 + len, + 10000, ... at which the three preconditions of A.check_preconditions hold
(searched on the CPU; `python -m tests.train_long_cases --search` walks the same rule and prints the table).
"""
from __future__ import annotations

import functools
from typing import Dict, Tuple

import numpy as np
import torch

from oracle import dptn_oracle as O
from tests import train_attention_cases as A

LENGTHS = (257, 288, 289, 385, 513)
FEATURES = (128, 64)

# (features, len, ppm) -> input seed
SEEDS: Dict[Tuple[int, int, int], int] = {
    (128, 257, 0): 41257, (128, 257, 100000): 31257, (128, 288, 0): 1288, (128, 288, 100000): 11288,
    (128, 289, 0): 11289, (128, 289, 100000): 1289, (128, 385, 0): 1385, (128, 385, 100000): 11385,
    (128, 385, 500000): 1385, (128, 513, 0): 1513, (128, 513, 100000): 1513,
    (64, 257, 0): 1257, (64, 257, 100000): 11257, (64, 288, 0): 1288, (64, 288, 100000): 1288,
    (64, 289, 0): 1289, (64, 289, 100000): 1289, (64, 385, 0): 1385, (64, 385, 100000): 11385,
    (64, 385, 500000): 1385, (64, 513, 0): 21513, (64, 513, 100000): 21513,
}


def _grid():
    return [A.Case(features, 1, ln, ppm) for features in FEATURES for ln in LENGTHS
            for ppm in (0, 100000) + ((500000,) if ln == 385 else ())]


CASES = _grid()


def input_seed(case: A.Case) -> int:
    return SEEDS[(case.features, case.len, case.ppm)]


@functools.lru_cache(maxsize=None)
def inputs(case: A.Case) -> Tuple[np.ndarray, np.ndarray]:
    """(x, dy) fp32 [B, S, K, N], read-only."""
    x, dy = A.inputs_for_seed(case, input_seed(case))
    x.setflags(write=False)
    dy.setflags(write=False)
    return x, dy


@functools.lru_cache(maxsize=None)
def reference(case: A.Case, bits: int = 64) -> Dict[str, object]:
    """A.formula at fp64 (the truth) or fp32 (the restatement) on the case's inputs and mask; read-only."""
    x, dy = inputs(case)
    return A.formula(case, x, dy, A.mask(case), torch.float64 if bits == 64 else torch.float32)


@functools.lru_cache(maxsize=None)
def one_bit_flipped(case: A.Case) -> Dict[str, object]:
    """The fp64 formula with the keep bit at A.flip_index(case) inverted."""
    assert case.ppm
    m = A.mask(case).copy()
    i = A.flip_index(case)
    m[i] = 1.0 - m[i]
    x, dy = inputs(case)
    return A.formula(case, x, dy, m, torch.float64)


def check_preconditions(case: A.Case) -> Dict[str, float]:
    """The three input preconditions of A.check_preconditions, with A's bounds, on this grid's inputs; -> the figures."""
    r64, r32 = reference(case, 64), reference(case, 32)
    out = {"min_relu": r64["min_relu"]}
    assert r64["min_relu"] >= A.MIN_RELU_INPUT, (case.id, "smallest ReLU input in fp64", r64["min_relu"])
    for key in ("y", "dx"):
        whole, worst, tok = A.figures(r32[key], r64[key])
        out[f"restatement.{key}"], out[f"restatement.{key}.token"] = whole, worst
        assert worst >= A.RESTATEMENT_FLOOR_DB, (case.id, key, "fp32 restatement, worst token", worst, tok)
    if case.ppm:
        f = one_bit_flipped(case)
        for key in ("y", "dx"):
            whole, worst, tok = A.figures(f[key], r64[key])
            out[f"one_bit.{key}"], out[f"one_bit.{key}.token"] = whole, worst
            assert worst <= A.ONE_BIT_CEILING_DB, (case.id, key, "one inverted keep bit, worst token", worst, tok)
        out["one_bit.param"] = min(O.agreement_db(f["grads"][k], r64["grads"][k]) for k in r64["grads"])
    return out


def _holds(case: A.Case, seed: int) -> bool:
    x, dy = A.inputs_for_seed(case, seed)
    r64 = A.formula(case, x, dy, A.mask(case), torch.float64)
    if r64["min_relu"] < A.MIN_RELU_INPUT:
        return False
    r32 = A.formula(case, x, dy, A.mask(case), torch.float32)
    if any(A.figures(r32[k], r64[k])[1] < A.RESTATEMENT_FLOOR_DB for k in ("y", "dx")):
        return False
    if case.ppm:
        m = A.mask(case).copy()
        i = A.flip_index(case)
        m[i] = 1.0 - m[i]
        f = A.formula(case, x, dy, m, torch.float64)
        if any(A.figures(f[k], r64[k])[1] > A.ONE_BIT_CEILING_DB for k in ("y", "dx")):
            return False
    return True


def _search():      # python -m tests.train_long_cases --search: the table above
    for case in CASES:
        seed = 1000 + case.len
        while not _holds(case, seed):
            seed += 10000
        print(f"    ({case.features}, {case.len}, {case.ppm}): {seed},", flush=True)


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        _search()
