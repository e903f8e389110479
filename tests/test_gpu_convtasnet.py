"""Conv-TasNet inference (speech_separation_amd.ConvTasNet, include/ctasnet.h) on the MI355X: parity with the reference's own
outputs (tests/golden/convtasnet.npz) and with the fp64 oracle (oracle/convtasnet_stock.py) at the config sizes and at
awkward lengths, determinism and batch independence, a device-only forward, guard-page memory safety and the module's
behaviour (no training step, train() == eval(), the model-agnostic inference loop)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import convtasnet_stock as CT
from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return CT.synthetic_convtasnet_weights(seed=0)


@pytest.fixture(scope="module")
def model(dev, weights):
    from speech_separation_amd import ConvTasNet
    m = ConvTasNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
    return m.to(dev).eval()


def _run(model, mix_np, dev):
    with torch.no_grad():
        out = model(mix=torch.from_numpy(mix_np).to(dev))
    return {k: out[k].cpu().numpy() for k in ("s1_pred", "s2_pred")}


def _oracle64(weights, mix_np):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    out = CT.forward({k: torch.from_numpy(v).double() for k, v in weights.items()}, torch.from_numpy(mix_np).double())
    return {k: v.numpy() for k, v in out.items()}


def _sisnri(out, inp):
    return O.si_snri_metric(out["s1_pred"].astype(np.float32), out["s2_pred"].astype(np.float32), inp["s1"], inp["s2"],
                            inp["mix"])


def test_matches_reference_outputs(dev, model):
    """B=2, T=4000, the oracle's seeded weights: against the reference's own ConvTasNet outputs."""
    from tests.conftest import GOLDEN
    z = np.load(os.path.join(GOLDEN, "convtasnet.npz"))
    inp = synthetic_inputs(DPTN_AUDIO, B=2, T=4000, seed=21)
    got = _run(model, inp["mix"], dev)
    for k in ("s1_pred", "s2_pred"):
        assert got[k].shape == z[k].shape == (2, 4000)
        assert O.agreement_db(got[k], z[k]) >= 90.0, (k, O.agreement_db(got[k], z[k]))
    ref = {k: z[k] for k in ("s1_pred", "s2_pred")}
    assert abs(_sisnri(got, inp) - _sisnri(ref, inp)) <= 1e-3


@pytest.mark.parametrize("B", [4, 16])
def test_config_sizes_match_the_fp64_oracle(dev, weights, model, B):
    """4 s mixtures (T = 32000) at B = 4 (config 1) and B = 16."""
    inp = synthetic_inputs(DPTN_AUDIO, B=B, T=32000, seed=100 + B)
    got = _run(model, inp["mix"], dev)
    ref = _oracle64(weights, inp["mix"])
    for k in ("s1_pred", "s2_pred"):
        assert got[k].shape == ref[k].shape == (B, 32000)
        agree = O.agreement_db(got[k], ref[k])
        print(f"B={B} {k}: {agree:.1f} dB")
        assert agree >= 90.0, (k, agree)
    assert abs(_sisnri(got, inp) - _sisnri(ref, inp)) <= 1e-3


def test_lengths(dev, weights, model):
    """T not a multiple of 16, T = 16 / 17 (F = 3, every dilation beyond 2 reaches past the mixture), T = 400 (F = 27 < 32, 64,
    128): the reference's output shapes and values; T < 16 is refused with a message."""
    for T in (16, 17, 400, 4001, 12345):
        inp = synthetic_inputs(DPTN_AUDIO, B=2, T=T, seed=T)
        got = _run(model, inp["mix"], dev)
        ref = _oracle64(weights, inp["mix"])
        for k in ("s1_pred", "s2_pred"):
            assert got[k].shape == ref[k].shape == (2, 16 * (T // 16)), (T, k)
            assert O.agreement_db(got[k], ref[k]) >= 90.0, (T, k, O.agreement_db(got[k], ref[k]))
    with torch.no_grad(), pytest.raises(RuntimeError, match="T must be >= 16"):
        model(mix=torch.zeros(2, 15, device=dev))


def test_deterministic_and_batch_independent(dev, model):
    inp = synthetic_inputs(DPTN_AUDIO, B=8, T=8001, seed=5)
    mix = torch.from_numpy(inp["mix"]).to(dev)
    with torch.no_grad():
        a = model(mix=mix)
        b = model(mix=mix)
        for k in ("s1_pred", "s2_pred"):
            assert torch.equal(a[k], b[k]), k
        for i in (0, 3, 7):
            one = model(mix=mix[i:i + 1].contiguous())
            for k in ("s1_pred", "s2_pred"):
                assert torch.equal(one[k][0], a[k][i]), (i, k)


def test_device_only_forward_and_side_stream(dev, model):
    mix = torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=3, T=6000, seed=9)["mix"]).to(dev)
    with torch.no_grad():
        want = model(mix=mix)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = model(mix=mix)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        s = torch.cuda.Stream(dev)
        s.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(s):
            side = model(mix=mix)
        torch.cuda.current_stream(dev).wait_stream(s)
        torch.cuda.synchronize()
    for k in ("s1_pred", "s2_pred"):
        assert torch.equal(got[k], want[k]) and torch.equal(side[k], want[k]), k


def test_memory_safety():
    """Poisoned workspace, then every buffer flush against an unmapped page at its end, then at its start
    (tests/ctasnet_memsafety_child.py): one child process per mode, in sequence; each result equals the plain run."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for mode in ("poison", "guard_end", "guard_start"):
        r = subprocess.run([sys.executable, "-m", "tests.ctasnet_memsafety_child", mode], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, f"{mode}: child ended with code {r.returncode}\n{r.stdout[-3000:]}"
        assert f"OK {mode} convtasnet" in r.stdout, r.stdout[-3000:]


def test_module_behaviour(dev, weights, model, tmp_path):
    from speech_separation_amd import ConvTasNet
    from speech_separation_amd.evaluate import run_inference
    from speech_separation_amd.io import collate, load_item
    from speech_separation_amd.metrics import SISNRiMetric
    from tests.dataset_fixture import make_dataset

    m = ConvTasNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights.items()}, strict=True)
    m = m.to(dev)
    mix = torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=2, T=4000, seed=21)["mix"]).to(dev)
    with pytest.raises(NotImplementedError, match="training step not built"):
        m(mix=mix)
    with torch.no_grad():
        tr = m.train()(mix=mix)
        ev = m.eval()(mix=mix)
    for k in ("s1_pred", "s2_pred"):
        assert torch.equal(tr[k], ev[k]), k

    n, bs = 10, 4
    entries, _ = make_dataset(str(tmp_path / "data"), n=n, T=4000)
    logs, stats = run_inference(model, entries, bs, [SISNRiMetric(name="SISNRiMetric")], save_dir=str(tmp_path / "out"),
                                device=dev, workers=2, target_sr=8000)
    assert stats["items"] == n and np.isfinite(logs["SISNRiMetric"])
    with torch.no_grad():
        for i in range(0, n, bs):
            b = collate([load_item(e, 8000) for e in entries[i:i + bs]])
            out = model(mix=b["mix"].to(dev))
            for j, ap in enumerate(b["audio_path"]):
                saved = torch.load(tmp_path / "out" / (os.path.splitext(os.path.basename(ap))[0] + ".pth"))
                assert torch.equal(saved["s1_pred"], out["s1_pred"][j].cpu()), (i + j)
                assert torch.equal(saved["s2_pred"], out["s2_pred"][j].cpu()), (i + j)
