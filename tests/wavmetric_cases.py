"""TEST INFRASTRUCTURE: the inputs of the STOI / ESTOI / SI-SDR device tests and their oracle values, computed once per
process (tests/stoi_ref.py at fp64 and fp32) and shared, read-only, by tests/test_wavmetric_host.py and
tests/test_gpu_wavmetric.py.

Cases (fs, B, T):
  (10000, 1, 3968)   exactly 30 frames, one segment, nothing removed (both targets without silence)
  (10000, 1, 3967)   29 frames: every pair exactly 1e-5
  (10000, 3, 9001)   odd T: rows after the first are 4-byte aligned only
  (8000, 2, 6000), (16000, 5, 12003)   both resamplers
  (16000, 33, 4500)  more items than half a wavefront; 20 frames after resampling: every pair 1e-5
  (16000, 16, 32000) the reference's batch of 2 s clips
  "mixed"            (16000, 4, 12003): a first target with gaps, one without silence, one whose active part leaves fewer
                     than 30 kept frames (1e-5 for that item's pairs with it), one all-zero (0)
Predictions are target + white noise at 5 dB (first) and -5 dB (second); the second target is an independent signal.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import stoi_ref as R

U = 2.0 ** -24
SHAPES = [(10000, 1, 3968), (10000, 1, 3967), (10000, 3, 9001), (8000, 2, 6000), (16000, 5, 12003), (16000, 33, 4500),
          (16000, 16, 32000)]
MIXED = (16000, 4, 12003)
MIXED_KINDS = ["gaps", "full", "short", "zero"]
NAMES = ["%dHz_%dx%d" % s for s in SHAPES] + ["mixed"]


def shape(name):
    return MIXED if name == "mixed" else SHAPES[NAMES.index(name)]


@functools.lru_cache(maxsize=None)
def case(name):
    """(s1_pred, s2_pred, s1, s2) fp32 [B, T], read-only."""
    fs, B, T = shape(name)
    if name == "mixed":
        arrays = R.make_batch(fs, B, T, seed=99, kinds=MIXED_KINDS)
    elif T < 4000:
        arrays = R.make_batch(fs, B, T, seed=fs // 1000 + B, kinds=["full"] * B, kinds2=["full"] * B)
    else:
        arrays = R.make_batch(fs, B, T, seed=fs // 1000 + B)
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def spectra(name, bits):
    return R.spectra(*case(name), shape(name)[0], np.float64 if bits == 64 else np.float32)


@functools.lru_cache(maxsize=None)
def values(name, extended, bits=64):
    v = R.values(spectra(name, bits), extended)
    v.setflags(write=False)
    return v


def bound(name, extended):
    """[B, 4]: 2 x |fp32 restatement - fp64| + 32 u, the bound a device value is held to."""
    return 2 * np.abs(values(name, extended, 32) - values(name, extended, 64)) + 32 * U


def kept(name):
    return R.kept(spectra(name, 64))


def min_margin(name):
    """The smallest distance in dB of any frame's energy from the 40 dB threshold, over every (item, target)."""
    m = [np.abs(t["margin"]).min() for item in spectra(name, 64) for t in item if t["margin"].size]
    return min(m) if m else np.inf
