"""The masked DPTN separator (DPTNEncDec, model/dptn.yaml) on the MI355X: forward and gradients against the reference's own
fixtures (tools/gen_golden_mask.py), the tail's tap table against the numpy restatement (tests/mask_tail_ref.py), a full
training step through the module, determinism, guard-page memory safety, and the dptn.yaml shape at B = 16."""
from __future__ import annotations

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTN_MASK, DPTNConfig, synthetic_inputs, synthetic_state_dict
from tests import mask_tail_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _model(cfg, sd, dev):
    from speech_separation_amd import DPTNEncDec
    kw = {k: v for k, v in cfg.to_dict().items() if k not in ("audio_only", "arch", "video_emb_size", "hidden_video")}
    model = DPTNEncDec(**kw)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()}, strict=True)
    return model.to(dev)


@pytest.mark.parametrize("name", ["mask_mid", "mask_mid128", "mask_full"])
def test_forward_matches_reference(dev, golden, name):
    """dptnav_forward (through the module) and the stage entry points against the reference's outputs; the stage run's
    decoder tap table ("taps") against the restated tail applied to the library's own block output."""
    from tools.gen_golden import weights_digest
    cfg, z = golden(name)
    B, T, Tv = (int(v) for v in z["shape"])
    sd = synthetic_state_dict(cfg, seed=0)
    assert weights_digest(sd) == str(z["digest"])
    inp = synthetic_inputs(cfg, seed=123, B=B, T=T, Tv=Tv)
    model = _model(cfg, sd, dev).eval()
    mix = torch.from_numpy(inp["mix"]).to(dev)
    with torch.no_grad():
        out = model(mix=mix, mix_spectrogram=torch.zeros(1, device=dev))
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy() for k in ("s1_pred", "s2_pred")}
    for k in got:
        assert O.agreement_db(got[k], z["tap." + k]) >= 80, (k, O.agreement_db(got[k], z["tap." + k]))
    d = abs(O.si_snri_metric(got["s1_pred"], got["s2_pred"], inp["s1"], inp["s2"], inp["mix"])
            - O.si_snri_metric(z["tap.s1_pred"], z["tap.s2_pred"], inp["s1"], inp["s2"], inp["mix"]))
    assert d <= 1e-3, d
    # the same through the stage entry points
    eng = model._get_engine(dev)
    enc, x = eng.stage_head(mix)
    for block in range(cfg.num_blocks):
        for path in (0, 1):
            x = eng.stage_path(block, path, x)
    s1, s2 = eng.stage_tail(x, enc, T)
    torch.cuda.synchronize()
    L = eng.frames(T)
    D = eng.tap("taps", B, T).view(2, B, L, 8).cpu().numpy().astype(np.float64)
    for k, s in (("s1_pred", s1), ("s2_pred", s2)):
        assert O.agreement_db(s.cpu().numpy(), z["tap." + k]) >= 80, k
    # restated tail on the library's block output (fp64): the tap table, and the fixture's strided tail taps
    p64 = {k: v.astype(np.float64) for k, v in sd.items()}
    xb = x.cpu().numpy().astype(np.float64).transpose(0, 3, 1, 2)          # (B,S,K,N) -> (B,N,S,K)
    e = enc.cpu().numpy().astype(np.float64).transpose(0, 2, 1)             # (B,L,N) -> (B,N,L)
    taps = {}
    m = R.masked_tail(xb, L, p64, cfg.step_size, taps)
    q = m * e[None]
    want = R.decoder_taps(q, p64["decoder.weight"])
    assert O.agreement_db(D, want) >= 90, O.agreement_db(D, want)
    left, ola = taps["left"], taps["ola"].shape[-1]
    pads = [t for t in range(L) if t < left or t >= left + ola]
    assert pads and O.agreement_db(D[:, :, pads], want[:, :, pads]) >= 90          # the bias-only padded frames
    step = next(int(k.split(".")[1][7:]) for k in z if k.startswith("tap.strided"))
    for k, v in (("masks", m), ("masked", q)):
        assert O.agreement_db(v.reshape(-1)[::step], z[f"tap.strided{step}.{k}"]) >= 75, k


@pytest.mark.parametrize("name", ["grad_mask_mid", "grad_mask_mid128"])
def test_training_step_matches_reference_gradients(dev, golden, name):
    """The reference's loss.backward() (fp64 truth, tools/gen_golden_mask.py) against dptnav_train_forward / _backward
    through the module; same floor and margin as test_gpu_backward.py's test of that name."""
    from speech_separation_amd.train import SiSNRWavLoss
    from tests.test_oracle_golden import reference_gradient_report
    from tools.gen_golden import weights_digest
    cfg, z = golden(name)
    B, T, Tv = (int(v) for v in z["shape"])
    wseed, iseed = (int(v) for v in z["seeds"])
    sd = synthetic_state_dict(cfg, seed=wseed)
    assert weights_digest(sd) == str(z["digest"])
    model = _model(cfg, sd, dev).train()
    inp = synthetic_inputs(cfg, B=B, T=T, Tv=Tv, seed=iseed)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    batch.update(model(mix_spectrogram=torch.zeros(1, device=dev), **batch))
    loss = SiSNRWavLoss()(**batch)["loss"]
    loss.backward()
    torch.cuda.synchronize()
    assert abs(float(loss.detach()) - float(z["val.loss64"])) < 1e-5 * abs(float(z["val.loss64"]))
    for k in ("s1_pred", "s2_pred"):
        assert O.agreement_db(batch[k].detach().cpu().numpy(), z["tap." + k]) > 80, k
    grads = {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}
    fails, worst_db, worst_norm = reference_gradient_report(z, grads, floor_db=60.0, margin_db=10.0)
    print(f"{name}: worst parameter {worst_db[1]} {worst_db[0]:.1f} dB, worst norm error {worst_norm[0]:.2e} ({worst_norm[1]})")
    assert not fails, fails[:8]
    assert worst_norm[0] < 3e-3, worst_norm
    total = float(np.sqrt(sum(float((g.astype(np.float64) ** 2).sum()) for g in grads.values())))
    assert abs(total - float(z["val.grad_norm"])) < 1e-4 * float(z["val.grad_norm"])


def test_full_training_step_through_the_module(dev):
    """model.train() (dropout 0.1 as in dptn.yaml), SiSNRWavLoss, clip_grad_norm_, FusedAdamW: no host synchronisation,
    a finite loss, every parameter moves."""
    from speech_separation_amd.optim import FusedAdamW, clip_grad_norm_
    from speech_separation_amd.train import SiSNRWavLoss
    cfg = DPTNConfig(**{**DPTN_MASK.to_dict(), "num_blocks": 2})
    model = _model(cfg, synthetic_state_dict(cfg, seed=3), dev).train()
    opt = FusedAdamW(model.parameters(), lr=1e-3)
    inp = synthetic_inputs(cfg, B=4, T=16000, seed=5)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    before = [p.detach().clone() for p in model.parameters()]

    def step():
        out = model(**batch)
        loss = SiSNRWavLoss()(**{**batch, **out})["loss"]
        opt.zero_grad()
        loss.backward()
        clip_grad_norm_(model.parameters(), 10.0)
        opt.step()
        return loss.detach()

    first = step()                     # allocations (engine, tape, optimizer state) happen here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        loss = step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    assert np.isfinite(float(first)) and np.isfinite(float(loss))
    for (k, p), b in zip(model.named_parameters(), before):
        assert torch.isfinite(p).all(), k
        assert not torch.equal(p.detach(), b), k


def test_deterministic_gradients_are_bit_identical(dev):
    from speech_separation_amd.train import SiSNRWavLoss
    cfg = DPTNConfig(**{**DPTN_MASK.to_dict(), "num_blocks": 2, "dropout": 0.0})
    model = _model(cfg, synthetic_state_dict(cfg, seed=4), dev).train()
    model._get_engine(dev).set_option("deterministic", 1)
    inp = synthetic_inputs(cfg, B=3, T=12000, seed=6)
    batch = {k: torch.from_numpy(v).to(dev) for k, v in inp.items()}
    runs = []
    for _ in range(2):
        model.zero_grad(set_to_none=True)
        out = model(**batch)
        SiSNRWavLoss()(**{**batch, **out})["loss"].backward()
        torch.cuda.synchronize()
        runs.append({k: p.grad.detach().clone() for k, p in model.named_parameters()})
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
        assert float(runs[0][k].abs().max()) > 0, k


@pytest.mark.parametrize("mode", ["guard_end", "guard_start"])
def test_memory_safety(mode):
    """Forward, stage entry points and training step of a 2-block DPTNEncDec with every buffer against an unmapped page
    (tests/mask_memsafety_child.py), in a child process of its own."""
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tests.mask_memsafety_child", mode, "mask64"], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    assert r.returncode == 0, f"{mode}: child ended with code {r.returncode}\n{r.stdout[-3000:]}"
    assert f"OK {mode} mask64" in r.stdout, r.stdout[-3000:]


def test_dptn_yaml_shape_at_batch_16(dev):
    """The dptn.yaml model at B = 16, T = 32000: finite outputs, and a second call gives the same bits."""
    model = _model(DPTN_MASK, synthetic_state_dict(DPTN_MASK, seed=0), dev).eval()
    inp = synthetic_inputs(DPTN_MASK, B=16, T=32000, seed=9)
    mix = torch.from_numpy(inp["mix"]).to(dev)
    with torch.no_grad():
        a = model(mix=mix)
        a = {k: v.clone() for k, v in a.items()}
        b = model(mix=mix)
    torch.cuda.synchronize()
    for k in ("s1_pred", "s2_pred"):
        assert torch.isfinite(a[k]).all() and float(a[k].abs().max()) > 0, k
        assert torch.equal(a[k], b[k]), k
