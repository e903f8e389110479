"""Deep Conv-TasNet host layer (no GPU needed): state_dict spec against the reference's key list (fixtures written by
tools/gen_golden_deepctasnet.py), module surface, the C ABI of include/dctasnet.h (declared == bound == exported, plain C99),
frame / output-length arithmetic, the refusals, the restatement against the reference's own outputs, and the engine
instantiations' ticket waits."""
from __future__ import annotations

import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dptn_oracle as O
from speech_separation_amd import _lib
from speech_separation_amd.spec import DPTN_AV, deepconvtasnet_state_dict_spec, synthetic_inputs
from tests import deepconvtasnet_ref as DR
from tools.gen_golden import weights_digest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "dctasnet.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = [("deepconvtasnet", False, 372, 11_379_386), ("deepavconvtasnet", True, 376, 11_511_738)]


def _models(av):
    from speech_separation_amd import DeepAVConvTasNet, DeepConvTasNet
    return DeepAVConvTasNet if av else DeepConvTasNet


@pytest.mark.parametrize("name,av,ntensors,nparams", CASES)
def test_spec_matches_the_reference_key_list(name, av, ntensors, nparams):
    z = np.load(os.path.join(GOLDEN, f"{name}.npz"))
    spec = deepconvtasnet_state_dict_spec(av)
    assert [k for k, _ in spec] == [str(k) for k in z["keys"]]
    assert len(spec) == ntensors
    assert sum(int(np.prod(s)) for _, s in spec) == nparams


@pytest.mark.parametrize("name,av,ntensors,nparams", CASES)
def test_module_keys_init_and_strict_load(name, av, ntensors, nparams):
    cls = _models(av)
    torch.manual_seed(0)
    m = cls()
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == deepconvtasnet_state_dict_spec(av)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in DR.synthetic_deepconvtasnet_weights(av, 0).items()}, strict=True)
    assert [(k, tuple(v.shape)) for k, v in cls(N=256, L=8).state_dict().items()] == deepconvtasnet_state_dict_spec(av)
    assert str(cls()).splitlines()[-2:] == [f"All parameters: {nparams}", f"Trainable parameters: {nparams}"]
    fresh = {k: p.detach() for k, p in cls().named_parameters()}
    prelus = {f"encoder.sequential.{i}.weight" for i in (2, 4, 6, 8)} | {f"decoder.sequential.{i}.weight" for i in (1, 3, 5, 7)}
    for k, p in fresh.items():
        if k in prelus or k.endswith(("PReLU_1.weight", "PReLU_2.weight", "seq.0.weight")):
            assert torch.all(p == 0.25), k
        elif k.endswith(("gamma", "norm_1.weight", "norm_2.weight", "video_ln.weight")):
            assert torch.all(p == 1.0), k
        elif k.endswith(("beta", "norm_1.bias", "norm_2.bias", "video_ln.bias")):
            assert torch.all(p == 0.0), k
        else:
            w = fresh[k[:-4] + "weight"] if k.endswith("bias") else p
            bound = 1.0 / math.sqrt(w[0].numel())
            if p.numel() > 1:
                assert float(p.abs().max()) <= bound and float(p.abs().max()) > 0.5 * bound, k
            else:
                assert float(p.abs().max()) <= bound, k
    # ConvTranspose1d's fan_in is weight.size(1) * k (torch's rule), i.e. weight[0].numel() as for Conv1d
    assert float(fresh["decoder.sequential.0.weight"].abs().max()) <= 1 / math.sqrt(1536)
    assert float(fresh["decoder.sequential.8.weight"].abs().max()) > 1 / math.sqrt(1536)


def test_non_default_video_sizes_are_refused():
    from speech_separation_amd import DeepAVConvTasNet
    with pytest.raises(NotImplementedError, match="video_emb_size=512, hidden_video=512"):
        DeepAVConvTasNet(video_emb_size=256)
    with pytest.raises(NotImplementedError, match="video_emb_size=512, hidden_video=512"):
        DeepAVConvTasNet(hidden_video=128)


def test_header_declares_exactly_the_bound_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(dctasnet_\w+)\s*\(", src))
    assert declared == set(_lib.DCTASNET_SYMBOLS), declared ^ set(_lib.DCTASNET_SYMBOLS)
    m = re.search(r"#define DCTASNET_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.DCTASNET_ABI_VERSION == 1
    lib = _lib.load()
    for name in _lib.DCTASNET_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.dctasnet_abi_version() == _lib.DCTASNET_ABI_VERSION
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(ROOT, "speech_separation_amd", "libdptnav.so")],
                         capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(dctasnet_\w+)$", out, re.M))
    assert exported == set(_lib.DCTASNET_SYMBOLS), exported ^ set(_lib.DCTASNET_SYMBOLS)


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("T", [16, 17, 400, 4000, 4001])
def test_frames_and_output_length_match_the_restatement(T):
    lib = _lib.load()
    assert lib.dctasnet_frames(T) == DR.frames(T)
    inp = synthetic_inputs(DPTN_AV, B=1, T=T, Tv=3, seed=1)
    sd = DR.synthetic_deepconvtasnet_weights(True, 0)
    out = DR.run_numpy(sd, inp["mix"], inp["s1_embedding"], inp["s2_embedding"], dtype=torch.float32)
    assert lib.dctasnet_out_len(T) == out["s1_pred"].shape[-1] == 16 * (T // 16)
    assert lib.dctasnet_frames(15) == 0 and lib.dctasnet_out_len(15) == 0


def test_cpu_tensors_are_refused():
    from speech_separation_amd import DeepAVConvTasNet, DeepConvTasNet
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU"):
        DeepConvTasNet()(mix=torch.zeros(1, 400))
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU"):
        DeepAVConvTasNet()(mix=torch.zeros(1, 400), s1_embedding=torch.zeros(1, 512, 5), s2_embedding=torch.zeros(1, 512, 5))
    from speech_separation_amd.engine import DeepConvTasNetEngine
    with pytest.raises(RuntimeError):
        DeepConvTasNetEngine("cpu")


def _restatement_reproduces_the_reference(fixture, av, slopes):
    z = np.load(os.path.join(GOLDEN, f"{fixture}.npz"))
    wseed, iseed = (int(v) for v in z["seeds"])
    B, T, Tv = (int(v) for v in z["shape"])
    sd = DR.synthetic_deepconvtasnet_weights(av, seed=wseed, slopes=slopes)
    assert weights_digest(sd) == str(z["digest"])
    inp = synthetic_inputs(DPTN_AV, B=B, T=T, Tv=Tv, seed=iseed)
    emb = (inp["s1_embedding"], inp["s2_embedding"]) if av else (None, None)
    torch.set_num_threads(min(8, os.cpu_count() or 1))
    out32 = DR.run_numpy(sd, inp["mix"], *emb, dtype=torch.float32)
    out64 = DR.run_numpy(sd, inp["mix"], *emb)
    for k in ("s1_pred", "s2_pred"):
        assert out32[k].shape == z[k].shape == (B, 16 * (T // 16))
        assert O.agreement_db(out32[k], z[k]) >= 120.0, (k, O.agreement_db(out32[k], z[k]))
        assert O.agreement_db(out64[k], z[k]) >= 90.0, (k, O.agreement_db(out64[k], z[k]))


@pytest.mark.parametrize("name,av,ntensors,nparams", CASES)
def test_restatement_reproduces_the_reference(name, av, ntensors, nparams):
    """tests/deepconvtasnet_ref.py in fp32 against the reference's own outputs (same weights, same inputs)."""
    _restatement_reproduces_the_reference(name, av, "0.25")


@pytest.mark.parametrize("name,av,ntensors,nparams", CASES)
def test_restatement_reproduces_the_reference_distinct_slopes(name, av, ntensors, nparams):
    """The same with 57 distinct PReLU slopes (deep encoder, Separator, deep decoder; tests/golden/*_slopes.npz): shows that the
    restatement gives each PReLU the slope the reference gives it, which one common slope cannot."""
    _restatement_reproduces_the_reference(name + "_slopes", av, "distinct")


def test_engine_reaches_no_ticket_wait_in_deepctasnet():
    """tools/ticket_waits.py on csrc/deepctasnet.hip: its instantiations of the GEMM engine keep the tile-loop ticket atomic
    free of waits, as ctasnet.hip's do."""
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ticket_waits.py"), "deepctasnet.hip"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert re.search(r"\d+ kernels with ticket atomics, 0 wait for the one inside their tile loop", r.stdout), r.stdout
