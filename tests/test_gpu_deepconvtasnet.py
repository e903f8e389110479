"""DeepConvTasNet / DeepAVConvTasNet inference (include/dctasnet.h) on the MI355X: parity with the reference's own outputs
(tests/golden/deepconvtasnet.npz, deepavconvtasnet.npz) and with the fp64 restatement (tests/deepconvtasnet_ref.py) at the
config sizes, at awkward lengths and video lengths, dilations reaching past short sequences, batch independence,
determinism, a device-only forward, fresh weights in the same storages, guard-page memory safety and the module's
behaviour (no training step, train() == eval(), the model-agnostic inference loop with embeddings)."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTN_AV, synthetic_inputs
from tests import deepconvtasnet_ref as DR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return {av: DR.synthetic_deepconvtasnet_weights(av, seed=0) for av in (False, True)}


@pytest.fixture(scope="module")
def models(dev, weights):
    from speech_separation_amd import DeepAVConvTasNet, DeepConvTasNet
    out = {}
    for av, cls in ((False, DeepConvTasNet), (True, DeepAVConvTasNet)):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights[av].items()}, strict=True)
        out[av] = m.to(dev).eval()
    return out


def _inputs(av, B, T, Tv=50, seed=0):
    inp = synthetic_inputs(DPTN_AV, B=B, T=T, Tv=Tv, seed=seed)
    if not av:
        inp.pop("s1_embedding"), inp.pop("s2_embedding")
    return inp


def _run(model, inp, dev):
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")}
    with torch.no_grad():
        out = model(**batch)
    return {k: out[k].cpu().numpy() for k in ("s1_pred", "s2_pred")}


def _ref64(weights, inp):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    return DR.run_numpy(weights, inp["mix"], inp.get("s1_embedding"), inp.get("s2_embedding"))


def _sisnri(out, inp):
    return O.si_snri_metric(out["s1_pred"].astype(np.float32), out["s2_pred"].astype(np.float32), inp["s1"], inp["s2"],
                            inp["mix"])


def _check64(got, ref, what, floor=100.0):
    for k in ("s1_pred", "s2_pred"):
        assert got[k].shape == ref[k].shape, (what, k)
        agree = O.agreement_db(got[k], ref[k])
        print(f"{what} {k}: {agree:.1f} dB")
        assert agree >= floor, (what, k, agree)


@pytest.mark.parametrize("av", [False, True])
def test_matches_reference_outputs(dev, models, av):
    """B=2, T=4000, Tv=13, the restatement's seeded weights: against the reference's own outputs."""
    z = np.load(os.path.join(GOLDEN, "deepavconvtasnet.npz" if av else "deepconvtasnet.npz"))
    wseed, iseed = (int(v) for v in z["seeds"])
    B, T, Tv = (int(v) for v in z["shape"])
    assert wseed == 0
    inp = _inputs(av, B, T, Tv, seed=iseed)
    got = _run(models[av], inp, dev)
    for k in ("s1_pred", "s2_pred"):
        assert got[k].shape == z[k].shape == (B, T)
        assert O.agreement_db(got[k], z[k]) >= 90.0, (k, O.agreement_db(got[k], z[k]))
    assert abs(_sisnri(got, inp) - _sisnri({k: z[k] for k in ("s1_pred", "s2_pred")}, inp)) <= 1e-3


@pytest.mark.parametrize("av", [False, True])
@pytest.mark.parametrize("B", [4, 16])
def test_config_sizes_match_the_fp64_restatement(dev, weights, models, av, B):
    """4 s mixtures (T = 32000, Tv = 50) at B = 4 and B = 16."""
    inp = _inputs(av, B, 32000, 50, seed=100 + B)
    got = _run(models[av], inp, dev)
    ref = _ref64(weights[av], inp)
    _check64(got, ref, f"av={av} B={B}")
    assert abs(_sisnri(got, inp) - _sisnri(ref, inp)) <= 1e-3


@pytest.mark.parametrize("av", [False, True])
def test_lengths(dev, weights, models, av):
    """T = 16 / 17 (F = 3: every dilation above 2 reaches past the sequence), 400, 4001, 12345; T < 16 is refused."""
    for T in (16, 17, 400, 4001, 12345):
        inp = _inputs(av, 2, T, 50, seed=T)
        _check64(_run(models[av], inp, dev), _ref64(weights[av], inp), f"av={av} T={T}")
    with torch.no_grad(), pytest.raises(RuntimeError, match="T must be >= 16"):
        _run(models[av], _inputs(av, 2, 15, 5), dev)


def test_video_lengths(dev, weights, models):
    """Tv = 1, 2, 7, 50, 400 against F = 26 (T = 400) and F = 252 (T = 4001): Tv above and below F.  At Tv = 400 the fp32
    source position ((f + 0.5) Tv / F - 0.5, as torch computes it in fp32) carries an absolute error of a few 1e-5 into the
    interpolation weight, which limits the agreement with the fp64 restatement to about 100 dB (measured 100.4)."""
    for T in (400, 4001):
        for Tv in (1, 2, 7, 50, 400):
            inp = _inputs(True, 2, T, Tv, seed=Tv)
            _check64(_run(models[True], inp, dev), _ref64(weights[True], inp), f"T={T} Tv={Tv}", 95.0 if Tv > 100 else 100.0)


@pytest.mark.parametrize("av", [False, True])
def test_sequence_edges_and_batch_independence(dev, weights, models, av):
    """F < 9 (T = 100: F = 8, the d = 8 taps fall entirely outside every sequence), and each mixture of a B = 16 batch
    equals the same mixture run alone, bit for bit: no tap crosses into a neighbouring mixture or speaker."""
    inp = _inputs(av, 3, 100, 5, seed=3)
    _check64(_run(models[av], inp, dev), _ref64(weights[av], inp), f"av={av} F=8")
    inp = _inputs(av, 16, 4001, 50, seed=5)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")}
    with torch.no_grad():
        a = models[av](**batch)
        b = models[av](**batch)
        for k in ("s1_pred", "s2_pred"):
            assert torch.equal(a[k], b[k]), k
        for i in (0, 7, 15):
            one = models[av](**{k: v[i:i + 1].contiguous() for k, v in batch.items()})
            for k in ("s1_pred", "s2_pred"):
                assert torch.equal(one[k][0], a[k][i]), (i, k)


@pytest.mark.parametrize("av", [False, True])
def test_device_only_forward(dev, models, av):
    inp = _inputs(av, 3, 6000, 50, seed=9)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")}
    with torch.no_grad():
        want = models[av](**batch)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            got = models[av](**batch)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
    for k in ("s1_pred", "s2_pred"):
        assert torch.equal(got[k], want[k]), k


@pytest.mark.parametrize("av", [False, True])
def test_new_weights_in_the_same_storages(dev, weights, av):
    """load_state_dict copies into the bound storages (same pointers, so no re-bind): the next forward must use the new
    values, including the dense convs' weights the library repacks."""
    from speech_separation_amd import DeepAVConvTasNet, DeepConvTasNet
    m = (DeepAVConvTasNet if av else DeepConvTasNet)()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights[av].items()}, strict=True)
    m = m.to(dev).eval()
    inp = _inputs(av, 2, 4001, 50, seed=77)
    _run(m, inp, dev)
    ptrs = [p.data_ptr() for p in m.parameters()]
    other = DR.synthetic_deepconvtasnet_weights(av, seed=1)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in other.items()}, strict=True)
    assert [p.data_ptr() for p in m.parameters()] == ptrs
    _check64(_run(m, inp, dev), _ref64(other, inp), f"av={av} reloaded")


def test_memory_safety():
    """Poisoned workspace, then every buffer flush against an unmapped page at its end, then at its start
    (tests/deepctasnet_memsafety_child.py): one child process per mode, in sequence; each result equals the plain run."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    for mode in ("poison", "guard_end", "guard_start"):
        r = subprocess.run([sys.executable, "-m", "tests.deepctasnet_memsafety_child", mode], cwd=ROOT, env=env,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
        assert r.returncode == 0, f"{mode}: child ended with code {r.returncode}\n{r.stdout[-3000:]}"
        assert f"OK {mode} deepconvtasnet" in r.stdout, r.stdout[-3000:]


@pytest.mark.parametrize("av", [False, True])
def test_module_behaviour(dev, weights, models, av, tmp_path):
    from speech_separation_amd import DeepAVConvTasNet, DeepConvTasNet
    from speech_separation_amd.evaluate import run_inference
    from speech_separation_amd.io import collate, load_item
    from speech_separation_amd.metrics import SISNRiMetric
    from tests.dataset_fixture import make_dataset

    m = (DeepAVConvTasNet if av else DeepConvTasNet)()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in weights[av].items()}, strict=True)
    m = m.to(dev)
    inp = _inputs(av, 2, 4000, 50, seed=21)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")}
    with pytest.raises(NotImplementedError, match="training step not built"):
        m(**batch)
    with torch.no_grad():
        tr = m.train()(**batch)
        ev = m.eval()(**batch)
    for k in ("s1_pred", "s2_pred"):
        assert torch.equal(tr[k], ev[k]), k

    n, bs = 10, 4
    entries, _ = make_dataset(str(tmp_path / "data"), n=n, T=4000)
    logs, stats = run_inference(models[av], entries, bs, [SISNRiMetric(name="SISNRiMetric")], save_dir=str(tmp_path / "out"),
                                device=dev, workers=2, target_sr=8000)
    assert stats["items"] == n and np.isfinite(logs["SISNRiMetric"])
    with torch.no_grad():
        for i in range(0, n, bs):
            b = collate([load_item(e, 8000) for e in entries[i:i + bs]])
            kw = {"mix": b["mix"].to(dev)}
            if av:
                kw.update(s1_embedding=b["s1_embedding"].to(dev), s2_embedding=b["s2_embedding"].to(dev))
            out = models[av](**kw)
            for j, ap in enumerate(b["audio_path"]):
                saved = torch.load(tmp_path / "out" / (os.path.splitext(os.path.basename(ap))[0] + ".pth"))
                assert torch.equal(saved["s1_pred"], out["s1_pred"][j].cpu()), (i + j)
                assert torch.equal(saved["s2_pred"], out["s2_pred"][j].cpu()), (i + j)
