"""Writes tests/golden/stoi_small.npz: inputs and fp64 values of the project's STOI / ESTOI restatement (tests/stoi_ref.py)
at fs = 8000, B = 2, T = 6000, so that later drift of the restatement shows up (tests/test_wavmetric_host.py reproduces
the file to 1e-12).  pystoi is not a dependency of this project: the restatement is the definition.

    python tools/gen_golden_stoi.py
"""
from __future__ import annotations

import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from tests import stoi_ref as R  # noqa: E402

FS, B, T, SEED = 8000, 2, 6000, 10


def main():
    p1, p2, s1, s2 = R.make_batch(FS, B, T, seed=SEED)
    spec = R.spectra(p1, p2, s1, s2, FS)
    out = os.path.join(ROOT, "tests", "golden", "stoi_small.npz")
    np.savez_compressed(out, fs=np.int64(FS), s1_pred=p1, s2_pred=p2, s1=s1, s2=s2, stoi=R.values(spec, False),
                        estoi=R.values(spec, True), kept=R.kept(spec), edges=np.array(R.EDGES, dtype=np.int64),
                        sisdr=R.sisdr_pairs(p1, p2, s1, s2))
    print(out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
