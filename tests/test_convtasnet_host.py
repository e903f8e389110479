"""Conv-TasNet host layer (no GPU needed): state_dict spec and module surface against the oracle's restatement of the
reference, the C ABI of include/ctasnet.h (declared == bound == exported, plain C99), frame / output-length arithmetic,
and the no-CPU-path behaviour."""
from __future__ import annotations

import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from oracle import convtasnet_stock as CT
from speech_separation_amd import _lib
from speech_separation_amd.spec import DPTN_AUDIO, convtasnet_state_dict_spec, synthetic_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ctasnet.h")


def test_spec_matches_the_oracle():
    spec = convtasnet_state_dict_spec()
    assert spec == CT.convtasnet_spec()
    assert sum(int(np.prod(s)) for _, s in spec) == 5_066_929


def test_module_keys_init_and_strict_load():
    from speech_separation_amd import ConvTasNet
    torch.manual_seed(0)
    m = ConvTasNet()
    sd = m.state_dict()
    assert [(k, tuple(v.shape)) for k, v in sd.items()] == CT.convtasnet_spec()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in CT.synthetic_convtasnet_weights(0).items()}, strict=True)
    assert [(k, tuple(v.shape)) for k, v in ConvTasNet(N=256, L=8).state_dict().items()] == CT.convtasnet_spec()
    lines = str(ConvTasNet()).splitlines()
    assert lines[-2:] == ["All parameters: 5066929", "Trainable parameters: 5066929"]
    # torch's defaults: PReLU 0.25, norms ones / zeros, conv weights and biases U(+-1/sqrt(fan_in))
    fresh = {k: p.detach() for k, p in ConvTasNet().named_parameters()}
    for k, p in fresh.items():
        if k.endswith(("PReLU_1.weight", "PReLU_2.weight", "seq.0.weight")):
            assert torch.all(p == 0.25), k
        elif k.endswith(("gamma", "norm_1.weight", "norm_2.weight")):
            assert torch.all(p == 1.0), k
        elif k.endswith(("beta", "norm_1.bias", "norm_2.bias")):
            assert torch.all(p == 0.0), k
        else:
            w = fresh[k[:-4] + "weight"] if k.endswith("bias") else p
            bound = 1.0 / math.sqrt(w[0].numel())
            assert float(p.abs().max()) <= bound and float(p.abs().max()) > 0.5 * bound, k
    assert float(fresh["separator.seq.1.weight"].std()) == pytest.approx(1 / math.sqrt(128) / math.sqrt(3), rel=0.05)


def test_header_declares_exactly_the_bound_symbols():
    src = open(HEADER).read()
    declared = set(re.findall(r"\b(ctasnet_\w+)\s*\(", src))
    assert declared == set(_lib.CTASNET_SYMBOLS), declared ^ set(_lib.CTASNET_SYMBOLS)
    m = re.search(r"#define CTASNET_ABI_VERSION (\d+)", src)
    assert int(m.group(1)) == _lib.CTASNET_ABI_VERSION == 1
    lib = _lib.load()
    for name in _lib.CTASNET_SYMBOLS:
        assert getattr(lib, name) is not None
    assert lib.ctasnet_abi_version() == _lib.CTASNET_ABI_VERSION


def test_header_is_plain_c99():
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-fsyntax-only", "-x", "c", HEADER],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("T", [16, 17, 400, 4000, 4001, 12345, 32000])
def test_frames_and_output_length_match_the_oracle(T):
    lib = _lib.load()
    mix = synthetic_inputs(DPTN_AUDIO, B=1, T=T, seed=1)["mix"]
    sd = {k: torch.from_numpy(v) for k, v in CT.synthetic_convtasnet_weights(0).items()}
    enc = torch.nn.functional.conv1d(torch.nn.functional.pad(torch.from_numpy(mix).unsqueeze(1), (16, 32)),
                                     sd["encoder.conv1d.weight"], stride=16)
    assert lib.ctasnet_frames(T) == enc.shape[-1]
    if T <= 4001:
        out = CT.forward(sd, torch.from_numpy(mix))
        assert lib.ctasnet_out_len(T) == out["s1_pred"].shape[-1]
    assert lib.ctasnet_out_len(T) == 16 * (T // 16)


@pytest.mark.skipif(torch.cuda.is_available(), reason="only meaningful on a box without a GPU")
def test_no_cpu_path_without_gpu():
    lib = _lib.load()
    h = C.c_void_p()
    assert lib.ctasnet_create(C.byref(h)) != 0
    assert b"no CPU path" in lib.ctasnet_last_error(None)
    from speech_separation_amd import ConvTasNet
    with torch.no_grad(), pytest.raises(RuntimeError):
        ConvTasNet()(mix=torch.zeros(1, 400))


def test_cpu_tensors_are_refused():
    from speech_separation_amd import ConvTasNet
    with torch.no_grad(), pytest.raises(RuntimeError, match="no CPU"):
        ConvTasNet()(mix=torch.zeros(1, 400))
    with pytest.raises(RuntimeError):
        from speech_separation_amd.engine import ConvTasNetEngine
        ConvTasNetEngine("cpu")


def test_engine_reaches_no_ticket_wait_in_ctasnet():
    """tools/ticket_waits.py on csrc/ctasnet.hip: the Conv-TasNet instantiations of the GEMM engine keep the tile-loop ticket
    atomic free of waits, as dptnav.hip's do (test_build_checks.py)."""
    import sys
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "ticket_waits.py"), "ctasnet.hip"], capture_output=True,
                       text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert "4 kernels with ticket atomics, 0 wait for the one inside their tile loop" in r.stdout
