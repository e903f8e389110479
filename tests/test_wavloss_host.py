"""Waveform criteria, host layer (no GPU needed): the C ABI of include/wavloss.h (declared == bound == exported, plain C99),
the scratch size, the module surface of MAEWavLoss / MSEWavLoss / SiSNRWavLoss, and the test oracle tests/wavloss_ref.py
against the values and gradients the reference's own classes produced (tests/golden/wavloss_*.npz, written by
tools/gen_golden_wavloss.py)."""
from __future__ import annotations

import glob
import inspect
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from speech_separation_amd import _lib
from tests import wavloss_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "wavloss.h")
FIXTURES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "wavloss_*.npz")))


def test_header_declares_exactly_the_bound_and_exported_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(wavloss_\w+)\s*\(", src))
    assert declared == set(_lib.WAVLOSS_SYMBOLS), declared ^ set(_lib.WAVLOSS_SYMBOLS)
    m = re.search(r"#define WAVLOSS_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.WAVLOSS_ABI_VERSION == 1
    lib = _lib.load()
    assert lib.wavloss_abi_version() == 1
    r = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    exported = {ln.split()[-1] for ln in r.stdout.splitlines() if " T " in ln and ln.split()[-1].startswith("wavloss_")}
    assert exported == declared, exported ^ declared


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_scratch_bytes_and_error_strings():
    lib = _lib.load()
    sizes = [lib.wavloss_scratch_bytes(B) for B in (1, 2, 16, 257)]
    assert all(s > 0 and s % 8 == 0 for s in sizes) and sizes == sorted(sizes) and sizes[0] < sizes[-1]
    assert lib.wavloss_scratch_bytes(0) == 0
    assert lib.wavloss_strerror(0) == b"ok"
    assert len({lib.wavloss_strerror(c) for c in (0, 1, 2, 4, 99)}) == 5


def test_bad_arguments_are_refused_before_any_launch():
    """No device is needed to be told no: every one of these returns WAVLOSS_ERR_INVALID without touching a pointer."""
    lib = _lib.load()
    buf = np.zeros(64, dtype=np.float64)
    p = buf.ctypes.data
    ok = dict(kind=0, level=0, B=1, T=4, ws=p, ws_bytes=int(lib.wavloss_scratch_bytes(1)))
    for change in (dict(B=0), dict(T=0), dict(kind=7), dict(level=7), dict(ws_bytes=ok["ws_bytes"] - 1), dict(ws=p + 4),
                   dict(kind=2, T=1), dict(ws=None)):
        a = dict(ok, **change)
        rc = lib.wavloss_pit_loss(a["kind"], a["level"], p, p, p, p, a["B"], a["T"], 1.0, p, p, p, p, a["ws"], a["ws_bytes"], None)
        assert rc == 1, change


def test_module_surface():
    import speech_separation_amd as S
    from speech_separation_amd import train
    from speech_separation_amd.metrics import MAEWavLoss, MSEWavLoss, SiSNRWavLoss
    for cls in (MAEWavLoss, MSEWavLoss, SiSNRWavLoss):
        assert cls.__name__ in S.__all__ and getattr(S, cls.__name__) is cls and getattr(train, cls.__name__) is cls
        assert cls().pit == "batch" and cls(pit="utterance").pit == "utterance" and cls("utterance").pit == "utterance"
        for bad in ("item", None, 1, "Batch"):
            with pytest.raises(ValueError, match="pit"):
                cls(pit=bad)
        z = torch.zeros(2, 8)
        for crit in (cls(), cls(pit="utterance")):
            with pytest.raises(RuntimeError, match="no CPU path"):
                crit(s1_pred=z, s2_pred=z, s1=z, s2=z, mix=z)
    # the call of the reference's classes (ss_losses.py:69-77): four tensors by name or position, the rest of the batch ignored
    sig = inspect.signature(SiSNRWavLoss.forward)
    assert list(sig.parameters) == ["self", "s1_pred", "s2_pred", "s1", "s2", "batch"]
    assert sig.parameters["batch"].kind is inspect.Parameter.VAR_KEYWORD
    assert inspect.signature(MAEWavLoss.forward) == inspect.signature(MSEWavLoss.forward)
    assert list(inspect.signature(MAEWavLoss.forward).parameters) == list(sig.parameters)


def test_fixtures_are_there():
    assert FIXTURES == ["wavloss_b2_t1", "wavloss_mixed_b5_t67", "wavloss_swap_b3_t131"]


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_reference_fixtures(name):
    """tests/wavloss_ref.py in fp64 against the reference's own fp64 loss, permutation and loss.backward() gradients, to
    fp64 rounding (1e-12 relative to the tensor's largest magnitude: the two sum in different orders); in fp32 the
    permutations agree as well."""
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    arrays = [z[k] for k in ("s1_pred", "s2_pred", "s1", "s2")]
    assert all(a.dtype == np.float32 for a in arrays)
    for kind in z["kinds"]:
        for level in R.LEVELS:
            got = R.evaluate(kind, level, *arrays)
            key = f"{kind}.{level}."
            assert np.array_equal(got["perm"], z[key + "perm64"]) and np.array_equal(z[key + "perm32"], z[key + "perm64"])
            for mine, theirs in (("loss", "loss64"), ("l0", "l0_64"), ("l1", "l1_64"), ("d1", "d1_64"), ("d2", "d2_64")):
                want = z[key + theirs]
                assert want.dtype == np.float64 and np.all(np.isfinite(want))
                assert np.max(np.abs(got[mine] - want)) <= 1e-12 * np.max(np.abs(want)), (kind, level, mine)
    if name == "wavloss_mixed_b5_t67":      # the mixed batch: items 1 and 3 on permutation 1, at both precisions
        for kind in R.KINDS:
            assert z[f"{kind}.utterance.perm64"].tolist() == [0, 1, 0, 1, 0] and z[f"{kind}.batch.perm64"].tolist() == [0] * 5
