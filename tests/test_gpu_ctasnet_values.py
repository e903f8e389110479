"""The Conv-TasNet family's inference forwards (ConvTasNet, DeepConvTasNet, DeepAVConvTasNet) on the MI355X at VALUES the other
files never feed them.  Those files are thorough about shapes, but all their weights have one PReLU slope (0.25) and all their
inputs are white noise of standard deviation 0.14:

* distinct slopes (`slopes="distinct"`: pairwise different, one exactly 0, one exactly 1, negative ones, some above 1): the
  slopes reach the kernels as bare pointers picked out of a flat table by index, so a swapped or stale index is invisible
  while all slopes are equal.  Parity with the reference's own outputs (tests/golden/*_slopes.npz) and with the fp64 oracle;
* hard inputs (tests/hard_inputs.py: silence, int16-scaled audio, a very quiet clip, DC offsets, zero padding, an impulse, a
  tone) in ONE batch, judged per mixture and per 16-sample frame, where the hand-written normalisation (eps 5e-6 against
  1e-10, variance as a sum of centred squares) can go wrong without the whole-batch agreement moving.

The training forward and the gradients on the same values are in tests/test_gpu_convtasnet_train.py."""
from __future__ import annotations

import os

import numpy as np
import pytest
import torch

from oracle import convtasnet_stock as CT
from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTN_AV, synthetic_inputs
from tests import deepconvtasnet_ref as DR
from tests import hard_inputs as HI
from tools.gen_golden import weights_digest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
MODELS = ("convtasnet", "deepconvtasnet", "deepavconvtasnet")
FLOOR = {"convtasnet": 90.0, "deepconvtasnet": 100.0, "deepavconvtasnet": 100.0}   # tests/test_gpu_{,deep}convtasnet.py's
KEYS = ("s1_pred", "s2_pred")
EMB = ("s1_embedding", "s2_embedding")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


@pytest.fixture(scope="module")
def weights():
    return {"convtasnet": CT.synthetic_convtasnet_weights(seed=0, slopes="distinct"),
            "deepconvtasnet": DR.synthetic_deepconvtasnet_weights(False, seed=0, slopes="distinct"),
            "deepavconvtasnet": DR.synthetic_deepconvtasnet_weights(True, seed=0, slopes="distinct")}


@pytest.fixture(scope="module")
def models(dev, weights):
    from speech_separation_amd import ConvTasNet, DeepAVConvTasNet, DeepConvTasNet
    out = {}
    for name, cls in zip(MODELS, (ConvTasNet, DeepConvTasNet, DeepAVConvTasNet)):
        m = cls()
        m.load_state_dict({k: torch.from_numpy(v) for k, v in weights[name].items()}, strict=True)
        out[name] = m.to(dev).eval()
    return out


def _inputs(name, B, T, Tv, seed):
    inp = synthetic_inputs(DPTN_AV, B=B, T=T, Tv=Tv, seed=seed)
    return {k: v for k, v in inp.items() if k == "mix" or (name == "deepavconvtasnet" and k in EMB)}


def _run(model, inp, dev, rows=slice(None)):
    with torch.no_grad():
        out = model(**{k: torch.from_numpy(np.ascontiguousarray(v[rows])).to(dev) for k, v in inp.items()})
    return {k: out[k].cpu().numpy() for k in KEYS}


def _ref(name, weights, inp, dtype=torch.float64):
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    if name == "convtasnet":
        out = CT.forward({k: torch.from_numpy(v).to(dtype) for k, v in weights.items()}, torch.from_numpy(inp["mix"]).to(dtype))
        return {k: v.numpy() for k, v in out.items()}
    return DR.run_numpy(weights, inp["mix"], inp.get(EMB[0]), inp.get(EMB[1]), dtype=dtype)


@pytest.mark.parametrize("name", MODELS)
def test_distinct_slopes_match_reference_outputs(dev, weights, models, name):
    """B = 2, T = 4000 (Tv = 13): against the reference's own outputs for the distinct-slope weights."""
    z = np.load(os.path.join(GOLDEN, f"{name}_slopes.npz"))
    assert weights_digest(weights[name]) == str(z["digest"])
    Tv = 13 if name == "convtasnet" else int(z["shape"][2])
    inp = _inputs(name, 2, 4000, Tv, seed=21)
    got = _run(models[name], inp, dev)
    for k in KEYS:
        assert got[k].shape == z[k].shape == (2, 4000)
        agree = O.agreement_db(got[k], z[k])
        print(f"{name} distinct slopes vs the reference {k}: {agree:.1f} dB")
        assert agree >= 90.0, (name, k, agree)


@pytest.mark.parametrize("B,T,Tv", [(4, 32000, 50), (3, 4001, 7)])
@pytest.mark.parametrize("name", MODELS)
def test_distinct_slopes_match_the_fp64_oracle(dev, weights, models, name, B, T, Tv):
    inp = _inputs(name, B, T, Tv, seed=B + T)
    got = _run(models[name], inp, dev)
    ref = _ref(name, weights[name], inp)
    for k in KEYS:
        assert got[k].shape == ref[k].shape == (B, 16 * (T // 16))
        agree = O.agreement_db(got[k], ref[k])
        print(f"{name} distinct slopes B={B} T={T} {k}: {agree:.1f} dB")
        assert agree >= FLOOR[name], (name, B, T, k, agree)


@pytest.mark.parametrize("name", MODELS)
def test_hard_inputs_per_mixture_and_per_frame(dev, weights, models, name):
    """The nine mixtures of tests/hard_inputs.py in one call at T = 4001 (a silent mixture shares GEMM tiles with one at
    int16 scale), distinct slopes, Tv = 7.  Per mixture and speaker against fp64: the whole signal and EVERY 16-sample frame
    (error RMS of the frame over the RMS of that mixture's whole reference output) at the floor the model's own file uses
    for whole tensors (90 dB ConvTasNet, 100 dB the deep models); exact zeros wherever the fp64 reference is exactly zero
    (ConvTasNet's encoder has no bias, so silence stays silence: all of `silent`, the tail of `padded`, everything away
    from the `impulse`; this also shows nothing leaks across zero padding); every output finite; each mixture run alone
    equals its row of the batch bit for bit.  The deep models' encoder has a bias, so their `silent` output is not zero
    and is judged in dB like the others.  Masks are invariant to the input's scale only up to eps, so no f(k x) = k f(x).

    The floors are bounds the fp32 restatement (stock PyTorch on the CPU) holds against fp64 on every one of these cases,
    measured before any kernel ran (whole mixture; worst frame, dB): ConvTasNet 121.6-124.2; 112.9-119.3 and 99.1 for
    `impulse`, whose output energy sits in three frames.  DeepConvTasNet 117.2-126.4; 113.1-121.5.  DeepAVConvTasNet
    117.4-122.5; 112.8-118.1.  The restatement's figures are computed again here, printed next to the kernel's and held to
    the same floor."""
    names, mix = HI.hard_mixtures(4001, seed=0)
    inp = {"mix": mix}
    if name == "deepavconvtasnet":
        emb = synthetic_inputs(DPTN_AV, B=len(names), T=4001, Tv=7, seed=0)
        inp.update({k: emb[k] for k in EMB})
    got = _run(models[name], inp, dev)
    ref64, ref32 = _ref(name, weights[name], inp), _ref(name, weights[name], inp, torch.float32)
    bad = HI.check_batch(name, names, got, ref64, ref32, FLOOR[name], exact_zero=("silent",) if name == "convtasnet" else ())
    for i, n in enumerate(names):
        alone = _run(models[name], inp, dev, rows=slice(i, i + 1))
        for k in KEYS:
            if not np.array_equal(alone[k][0], got[k][i]):
                bad.append((n, k, "alone differs from its row in the batch"))
    assert not bad, bad


MEAN_OFFSET = 50.0


def test_large_mean_in_front_of_the_block_norms(dev, weights):
    """ctasnet_kernels.h promises a variance of the form sum M2_i + sum n (m_i - mean)^2 and never E[x^2] - E[x]^2.  The
    hard INPUTS cannot test that: GlobalNorm and the blocks' GroupNorm(1, H) take their statistics over channels and time,
    the synthetic encoder and conv weights have zero mean, so even a DC of 1000 at the input leaves mean^2 of the order of
    the variance at every norm, where the cancelling formula loses a bit or two (measured: a library whose statistics
    kernel computes E[x^2] - E[x]^2 passes every other test of this file).  What makes a mean large against the deviation
    at a norm is a bias: here block 3's conv1d bias (in front of norm_1) and block 17's dconv1d bias (in front of norm_2)
    are raised by 50, about a hundred deviations; the cancelling formula then loses three to four digits of the variance
    (measured with such a library: 75.2-89.9 dB on `plain` and `padded`), the shifted one none (108.3 dB on every frame).  Per mixture and per frame at the file's floor of 90 dB; the fp32 restatement on the CPU
    holds 103.8-105.9 dB per mixture and 97.5 dB on every frame with these weights (with +100 it would hold 91.4 only, as the
    conv outputs themselves then carry the rounding of the large mean)."""
    from speech_separation_amd import ConvTasNet
    w = dict(weights["convtasnet"])
    for k in ("separator.separator.3.conv1d.bias", "separator.separator.17.dconv1d.bias"):
        w[k] = w[k] + np.float32(MEAN_OFFSET)
    m = ConvTasNet()
    m.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()}, strict=True)
    m = m.to(dev).eval()
    names, mix = HI.hard_mixtures(4001, seed=0, names=("plain", "dc10", "padded", "tone"))
    inp = {"mix": mix}
    got = _run(m, inp, dev)
    bad = HI.check_batch("convtasnet, mean 50 at two norms", names, got, _ref("convtasnet", w, inp),
                         _ref("convtasnet", w, inp, torch.float32), FLOOR["convtasnet"])
    assert not bad, bad
