"""tests/hard_inputs.py itself (no GPU): the mixtures are what their names say, and the judge sees what it is there to see."""
from __future__ import annotations

import numpy as np

from tests import hard_inputs as HI


def test_mixtures_are_what_their_names_say():
    names, mix = HI.hard_mixtures(4001, seed=0)
    assert tuple(names) == HI.NAMES and mix.shape == (9, 4001) and mix.dtype == np.float32 and np.isfinite(mix).all()
    m = dict(zip(names, mix))
    assert 0.12 < m["plain"].std() < 0.16 and abs(m["plain"].mean()) < 0.01
    assert not m["silent"].any()
    assert np.abs(m["int16"]).max() > 32768 and 0.12 * 65536 < m["int16"].std() < 0.16 * 65536
    assert 0.12e-4 < m["quiet"].std() < 0.16e-4
    assert abs(m["dc10"].mean() - 10) < 0.01 and abs(m["dc1000"].mean() - 1000) < 0.01 and 0.12 < m["dc1000"].std() < 0.16
    assert m["padded"][:HI.PADDED_FROM].std() > 0.12 and not m["padded"][HI.PADDED_FROM:].any()
    assert m["impulse"][2000] == 1.0 and np.count_nonzero(m["impulse"]) == 1
    assert abs(np.abs(m["tone"]).max() - 0.3) < 1e-3 and abs(np.argmax(np.abs(np.fft.rfft(m["tone"][:4000]))) - 220) <= 1
    # seeded, and a mixture does not depend on its place in the batch
    again = HI.hard_mixtures(4001, seed=0, names=("dc10", "plain"))[1]
    assert np.array_equal(again[0], m["dc10"]) and np.array_equal(again[1], m["plain"])
    assert not np.array_equal(HI.hard_mixtures(4001, seed=1)[1][0], m["plain"])


def test_judge_sees_one_wrong_frame_and_leaks_into_silence():
    rng = np.random.default_rng(0)
    ref = rng.standard_normal(4000)
    ref[2000:] = 0.0                                    # zero padding
    got = ref.copy()
    got[16:32] += 1e-4                                  # one frame off by -80 dB; diluted to about -101 dB over the signal
    j = HI.judge(got, ref)
    assert j["db"] > 95 and 76 < j["worst"][0] < 80 and j["worst"][1] == 1 and j["edges"][1] == j["worst"][0]
    assert j["edges"][0] == float("inf") and j["n_zero_frames"] == 125 and j["zero_frames_exact"] and j["finite"]
    both = {"s1_pred": got[None], "s2_pred": ref[None]}
    refs = {"s1_pred": ref[None], "s2_pred": ref[None]}
    bad = HI.check_batch("t", ["x"], both, refs, refs, 90.0)
    assert [b[:3] for b in bad] == [("x", "s1_pred", "worst frame")]
    leak = ref.copy()
    leak[3000] = 1e-30
    j = HI.judge(leak, ref)
    assert not j["zero_frames_exact"] and not j["zero"]
    nan = ref.copy()
    nan[5] = np.nan
    j = HI.judge(nan, ref)
    assert not j["finite"] and j["db"] == float("-inf")
    z = HI.judge(np.zeros(64), np.zeros(64))
    assert z["zero"] and z["zero_frames_exact"] and z["db"] == float("inf")
    bad = HI.check_batch("t", ["silent"], {k: np.full((1, 64), 1e-20) for k in both}, {k: np.zeros((1, 64)) for k in both},
                         {k: np.zeros((1, 64)) for k in both}, 90.0, exact_zero=("silent",))
    assert len(bad) == 4
