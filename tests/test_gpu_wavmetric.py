"""STOI / ESTOI and SI-SDR on the MI355X (include/wavmetric.h, speech_separation_amd.STOIMetric / SISDRMetric) against the
fp64 restatement tests/stoi_ref.py, which is the definition (pystoi is not a dependency).

Inputs and shapes: tests/wavmetric_cases.py.  Precondition, asserted on the fp64 oracle before the kernel is looked at:
every frame's energy is at least 1 dB away from the 40 dB threshold of the silent-frame removal (a condition on the
inputs, not a tolerance: no frame is excused).  Then
  kept    equals the oracle's on every (item, target)
  STOI / ESTOI   |hip - fp64| <= 2 |fp32 restatement - fp64| + 32 u, u = 2^-24.  The first term is the project's rule for
          values no bound derives through (tests/test_gpu_wavloss.py); the fp32 restatement's own distance is 0.1 .. 3 u
          because its rounding errors average out, so alone it is too small to be a bound.  The floor is the worst-case
          bound n u of one 30-term normalised correlation: every value is a mean of such terms, all within [-1, 1].
          tests/test_wavmetric_host.py shows that one band edge off by one bin moves every such value by > 10 x this bound.
  SI-SDR  |hip - fp64| <= 2 |fp32 formula - fp64| + 4 u |value|
The short path gives exactly 1e-5 and an all-zero target exactly 0.
"""
from __future__ import annotations

import ctypes
import functools

import numpy as np
import pytest
import torch

from tests import stoi_ref as R
from tests import wavmetric_cases as W

pytestmark = pytest.mark.gpu
U = W.U
WORST = {}          # what -> worst observed error / bound over this session, printed by the last test


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def to_dev(arrays, dev):
    return [torch.from_numpy(np.array(a)).to(dev) for a in arrays]


@functools.lru_cache(maxsize=None)
def run_stoi(name, extended):
    """(out [B, 4], kept [B, 2]) of the device for a case, computed once."""
    from speech_separation_amd.metrics import stoi_pairs
    out, kept = stoi_pairs(*to_dev(W.case(name), torch.device("cuda:0")), fs=W.shape(name)[0], extended=extended)
    torch.cuda.synchronize()
    return out.cpu().numpy(), kept.cpu().numpy()


def _record(what, err, bound):
    ratio = float(np.max(err / bound))
    WORST[what] = max(WORST.get(what, 0.0), ratio)
    print(f"wavmetric {what}: worst error {float(np.max(err)):.3e}, error / bound {ratio:.3f}")


@pytest.mark.parametrize("extended", [False, True])
@pytest.mark.parametrize("name", W.NAMES)
def test_stoi_pairs(dev, name, extended):
    assert W.min_margin(name) >= 1.0, "a frame within 1 dB of the threshold: the inputs do not decide the mask"
    want, bound = W.values(name, extended), W.bound(name, extended)
    got, kept = run_stoi(name, extended)
    B = W.shape(name)[1]
    assert got.dtype == np.float32 and got.shape == (B, 4) and kept.dtype == np.int32 and kept.shape == (B, 2)
    assert np.array_equal(kept, W.kept(name)), (kept.tolist(), W.kept(name).tolist())
    short, zero = want == R.SHORT_VALUE, want == 0
    assert np.all(got[short] == np.float32(1e-5)) and np.all(got[zero] == 0)
    if name in ("10000Hz_1x3967", "16000Hz_33x4500"):
        assert short.all()
    if name == "10000Hz_1x3968":
        assert kept.tolist() == [[30, 30]] and not short.any()
    if name == "mixed":
        assert short[2, [0, 2]].all() and zero[3, [0, 2]].all() and short.sum() == 2 and zero.sum() == 2
    err = np.abs(got.astype(np.float64) - want)
    print(f"{name} extended={extended}: hip {got[0].tolist()} fp64 {want[0].tolist()}")
    _record("estoi" if extended else "stoi", err, bound)
    assert np.all(err <= bound), (name, extended, err.max(), (err / bound).max())


@pytest.mark.parametrize("name", W.NAMES)
def test_sisdr_pairs(dev, name):
    from speech_separation_amd.metrics import sisdr_pairs
    arrays = W.case(name)
    want, f32 = R.sisdr_pairs(*arrays), R.sisdr_pairs(*arrays, dtype=np.float32)
    got = sisdr_pairs(*to_dev(arrays, dev)).cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape and np.all(np.isfinite(got))
    err, bound = np.abs(got.astype(np.float64) - want), 2 * np.abs(f32 - want) + 4 * U * np.abs(want)
    _record("sisdr", err, bound)
    assert np.all(err <= bound), (name, err.max(), (err / bound).max())


def test_sisdr_agrees_with_the_sisnr_kernel_on_centred_inputs(dev):
    """Independent check: on inputs centred in fp64 and rounded once, the zero-mean SI-SNR of dptnav_sisnr_pairs is the
    SI-SDR (the eps terms are 1e-9 of the energies)."""
    from speech_separation_amd.metrics import _engine, sisdr_pairs
    arrays = [(a.astype(np.float64) - a.astype(np.float64).mean(axis=1, keepdims=True)).astype(np.float32)
              for a in W.case("16000Hz_5x12003")]
    t = to_dev(arrays, dev)
    got = sisdr_pairs(*t).cpu().numpy().astype(np.float64)
    other = _engine(dev).sisnr_pairs(*t, t[0])[:, :4, 0].cpu().numpy().astype(np.float64)
    want = R.sisdr_pairs(*arrays)
    bound = 2 * np.abs(R.sisdr_pairs(*arrays, dtype=np.float32) - want) + 4 * U * np.abs(want)
    _record("sisdr vs sisnr kernel", np.abs(got - other), bound)
    assert np.all(np.abs(got - other) <= bound)


@pytest.mark.parametrize("name", ["10000Hz_3x9001", "16000Hz_5x12003", "mixed"])
def test_two_calls_are_bitwise_equal(dev, name):
    from speech_separation_amd.metrics import sisdr_pairs, stoi_pairs
    t = to_dev(W.case(name), dev)
    for ext in (False, True):
        a, b = (stoi_pairs(*t, fs=W.shape(name)[0], extended=ext) for _ in range(2))
        assert a[0].cpu().numpy().tobytes() == b[0].cpu().numpy().tobytes() and torch.equal(a[1], b[1])
        assert a[0].cpu().numpy().tobytes() == run_stoi(name, ext)[0].tobytes()
    assert sisdr_pairs(*t).cpu().numpy().tobytes() == sisdr_pairs(*t).cpu().numpy().tobytes()


def test_metric_classes(dev):
    import speech_separation_amd as S
    name = "8000Hz_2x6000"
    keys = ("s1_pred", "s2_pred", "s1", "s2")
    batch = dict(zip(keys, to_dev(W.case(name), dev)), mix=None, audio_path=["a", "b"])
    swapped = dict(batch, s1_pred=batch["s2_pred"], s2_pred=batch["s1_pred"])
    for ext in (False, True):
        met = S.STOIMetric(fs=8000, extended=ext, name="stoi")
        v = met(**batch)
        assert isinstance(v, float) and met.name == "stoi" and met.last_kept.device == dev
        means = met.enqueue(**batch)
        assert means.device == dev and means.shape == (4,) and means.dtype == torch.float64
        assert v == met.resolve(means.cpu())
        want, bound = W.values(name, ext), W.bound(name, ext).mean(0).max()
        assert abs(v - R.pit(want)) <= bound and R.pit(want) == (want[:, 0].mean() + want[:, 3].mean()) / 2
        # speakers exchanged: the batch-level permutation is the other one, the value the same
        sw = want[:, [2, 3, 0, 1]]
        assert R.pit(sw) == (sw[:, 1].mean() + sw[:, 2].mean()) / 2 > (sw[:, 0].mean() + sw[:, 3].mean()) / 2 + 0.1
        assert abs(met(**swapped) - R.pit(sw)) <= bound
        low = S.STOIMetric(fs=8000, extended=ext, lower_better=True)(**batch)
        assert abs(low - (want[:, 1].mean() + want[:, 2].mean()) / 2) <= bound
    met = S.SISDRMetric()
    v = met(**batch)
    want = R.sisdr_pairs(*W.case(name))
    assert isinstance(v, float) and v == met.resolve(met.enqueue(**batch).cpu()) and abs(v - R.pit(want)) <= 1e-5 * abs(R.pit(want))
    assert abs(met(**swapped) - R.pit(want[:, [2, 3, 0, 1]])) <= 1e-5 * abs(R.pit(want))
    # arguments as the criteria's: four fp32 [B, T] tensors of one shape on one GPU
    with pytest.raises(ValueError, match=r"\(2, 5999\).*\(2, 6000\)"):
        met(**dict(batch, s2=batch["s2"][:, :5999]))
    with pytest.raises(TypeError, match="float32"):
        S.STOIMetric(fs=8000)(**dict(batch, s1=batch["s1"].double()))
    nc = {k: torch.stack([batch[k], batch[k]], dim=2)[:, :, 0] for k in keys}
    assert not nc["s1"].is_contiguous() and S.STOIMetric(fs=8000)(**nc) == S.STOIMetric(fs=8000)(**batch)


def test_enqueue_does_not_synchronise(dev):
    import speech_separation_amd as S
    batch = dict(zip(("s1_pred", "s2_pred", "s1", "s2"), to_dev(W.case("16000Hz_5x12003"), dev)))
    mets = [S.STOIMetric(), S.STOIMetric(extended=True), S.SISDRMetric()]
    first = [m.enqueue(**batch) for m in mets]                      # handles and allocations happen here
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        again = [m.enqueue(**batch) for m in mets]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    torch.cuda.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b)


def test_run_inference_takes_the_metrics_on_its_non_stalling_branch(dev, tmp_path):
    """evaluate.run_inference with [SISNRiMetric, STOIMetric] on the synthetic dataset returns the mean of per-batch calls."""
    from speech_separation_amd.evaluate import run_inference
    from speech_separation_amd.io import collate, load_item
    from speech_separation_amd.metrics import SISNRiMetric, STOIMetric
    from tests.dataset_fixture import make_dataset

    def model(mix, s1=None, s2=None, **batch):       # a stand-in separator: the targets with some of the mixture left in
        return {"s1_pred": 0.8 * s1 + 0.2 * mix, "s2_pred": 0.6 * s2 + 0.4 * mix}

    n, bs = 10, 4
    entries, _ = make_dataset(str(tmp_path / "data"), n=n, T=6000)
    mets = [SISNRiMetric(name="SISNRiMetric"), STOIMetric(fs=8000, name="STOIMetric")]
    assert all(hasattr(m, "enqueue") and hasattr(m, "resolve") for m in mets)
    logs, stats = run_inference(model, entries, bs, mets, save_dir=None, device=dev, workers=2, target_sr=8000)
    assert stats["items"] == n
    sums = [0.0, 0.0]
    nb = 0
    for i in range(0, n, bs):
        b = collate([load_item(e, 8000) for e in entries[i:i + bs]])
        b = {k: (v.to(dev) if isinstance(v, torch.Tensor) else v) for k, v in b.items()}
        b.update(model(**b))
        for j, m in enumerate(mets):
            sums[j] += float(m(**b))
        nb += 1
    assert logs["STOIMetric"] == pytest.approx(sums[1] / nb, abs=1e-12) and 0 < logs["STOIMetric"] <= 1
    assert logs["SISNRiMetric"] == pytest.approx(sums[0] / nb, abs=1e-9)


def test_argument_errors_launch_nothing(dev):
    from speech_separation_amd import _lib
    lib = _lib.load()
    h = ctypes.c_void_p(0x1234)
    assert lib.wavmetric_stoi_create(44100, 0, ctypes.byref(h)) == 1 and h.value == 0x1234
    assert lib.wavmetric_stoi_create(8000, 0, ctypes.byref(h)) == 0 and h.value not in (None, 0x1234)
    fs, B, T = 8000, 2, 6000
    inp = to_dev(W.case("8000Hz_2x6000"), dev)
    need = int(lib.wavmetric_stoi_scratch_bytes(h, B, T))
    assert need > 0 and need % 16 == 0 and lib.wavmetric_stoi_scratch_bytes(h, 0, T) == 0
    out, kept = torch.full((B, 4), 7.0, device=dev), torch.full((B, 2), 7, dtype=torch.int32, device=dev)
    ws = torch.full((need + 16,), 0x5A, dtype=torch.uint8, device=dev)
    assert ws.data_ptr() % 16 == 0
    stream = torch.cuda.current_stream(dev).cuda_stream
    good = dict(h=h, p=inp[2].data_ptr(), B=B, T=T, out=out.data_ptr(), kept=kept.data_ptr(), ws=ws.data_ptr(), ws_bytes=need)
    for change in (dict(h=None), dict(p=None), dict(B=0), dict(T=0), dict(out=None), dict(kept=None), dict(ws=None),
                   dict(ws_bytes=need - 1), dict(ws=ws.data_ptr() + 4), dict(ws=ws.data_ptr() + 8)):
        a = dict(good, **change)
        rc = lib.wavmetric_stoi_pairs(a["h"], inp[0].data_ptr(), inp[1].data_ptr(), a["p"], inp[3].data_ptr(), a["B"], a["T"],
                                      a["out"], a["kept"], a["ws"], a["ws_bytes"], stream)
        assert rc == 1, change                                       # WAVMETRIC_ERR_INVALID
        torch.cuda.synchronize()
        assert bool((out == 7).all()) and bool((kept == 7).all()) and bool((ws == 0x5A).all()), change
    for change in (dict(p=None), dict(B=0), dict(T=0), dict(out=None)):
        a = dict(good, **change)
        rc = lib.wavmetric_sisdr_pairs(inp[0].data_ptr(), inp[1].data_ptr(), a["p"], inp[3].data_ptr(), a["B"], a["T"], a["out"], stream)
        assert rc == 1, change
        torch.cuda.synchronize()
        assert bool((out == 7).all()), change
    assert lib.wavmetric_stoi_pairs(h, *[t.data_ptr() for t in inp], B, T, out.data_ptr(), kept.data_ptr(), ws.data_ptr(), need,
                                    stream) == 0
    torch.cuda.synchronize()
    assert not bool((out == 7).any()) and not bool((kept == 7).any()) and bool((ws[need:] == 0x5A).all())
    assert np.array_equal(out.cpu().numpy(), run_stoi("8000Hz_2x6000", False)[0])
    lib.wavmetric_stoi_destroy(h)


def test_zz_worst_ratio_is_reported():
    """The worst error / bound ratio the checks of this session saw (DESIGN.md section 19 quotes it)."""
    for k, v in sorted(WORST.items()):
        print(f"wavmetric worst ratio {k}: {v:.3f}")
    assert all(v <= 1.0 for v in WORST.values())
