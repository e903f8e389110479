"""TEST INFRASTRUCTURE (not product code): mixtures whose VALUES are hard for hand-written normalisation (the other
generators draw white noise of standard deviation 0.14 only), and the figures they are judged by: one agreement per mixture
and speaker rather than one over the batch (where only the loudest mixture counts), and one per 16-sample output frame
(where an error confined to a sequence edge is not diluted by the rest of the signal)."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

NAMES = ("plain", "silent", "int16", "quiet", "dc10", "dc1000", "padded", "impulse", "tone")
PADDED_FROM = 1500        # `padded`: silence from this sample on (a batch zero-padded by the collate function)
FRAME = 16                # output samples per decoder frame (the models' L)


def hard_mixtures(T: int, seed: int = 0, names: Sequence[str] = NAMES) -> Tuple[List[str], np.ndarray]:
    """-> (names, mix [len(names)][T] float32).  Every noise-like mixture has a draw of its own of the usual noise
    (0.1 N(0, 1) per speaker, two speakers); the draws depend on `seed` and on the mixture's name, not on its place."""
    out = np.zeros((len(names), T), np.float32)
    t = np.arange(T)
    for i, name in enumerate(names):
        rng = np.random.default_rng([seed, NAMES.index(name)])
        plain = (0.1 * rng.standard_normal(T)).astype(np.float32) + (0.1 * rng.standard_normal(T)).astype(np.float32)
        if name == "plain":
            x = plain
        elif name == "silent":
            x = np.zeros(T, np.float32)
        elif name == "int16":           # audio a loader did not normalise: peaks beyond +-32768
            x = plain * np.float32(65536.0)
        elif name == "quiet":           # the encoder's variance is of the order of GlobalNorm's eps
            x = plain * np.float32(1e-4)
        elif name == "dc10":
            x = plain + np.float32(10.0)
        elif name == "dc1000":          # the mean is 10^4 times the deviation
            x = plain + np.float32(1000.0)
        elif name == "padded":
            x = plain.copy()
            x[PADDED_FROM:] = 0.0
        elif name == "impulse":
            x = np.zeros(T, np.float32)
            x[T // 2] = 1.0
        elif name == "tone":            # 440 Hz at 8 kHz
            x = (0.3 * np.sin(2 * np.pi * 440.0 * t / 8000.0)).astype(np.float32)
        else:
            raise KeyError(name)
        out[i] = x
    return list(names), out


def _db(ref_power: float, err_power: float) -> float:
    if err_power == 0:
        return float("inf")
    return float("-inf") if ref_power == 0 else float(10 * np.log10(ref_power / err_power))


def judge(got: np.ndarray, ref: np.ndarray) -> Dict[str, object]:
    """One mixture and speaker, got / ref [16 n] (ref: fp64).  -> {"zero": the reference is exactly zero everywhere,
    "db": agreement over the whole signal (10 log10 |ref|^2 / |got - ref|^2), "frame_db": per 16-sample frame, the RMS of
    the reference's WHOLE signal over the error RMS of that frame (inf where the frame is exact), "worst": (frame_db, frame)
    of the worst frame, "edges": frame_db of the first two and last two frames, "zero_frames_exact": got is exactly zero in
    every frame where the reference is exactly zero, "finite": got is finite}."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    assert got.shape == ref.shape and got.ndim == 1 and got.size % FRAME == 0 and got.size >= 4 * FRAME
    finite = bool(np.isfinite(got).all())
    gf, rf = got.reshape(-1, FRAME), ref.reshape(-1, FRAME)
    zero_ref = ~rf.any(axis=1)
    with np.errstate(invalid="ignore", over="ignore"):
        err = ((gf - rf) ** 2).mean(axis=1)
        power = float((ref ** 2).mean())
        frame_db = np.array([_db(power, e) if np.isfinite(e) else -np.inf for e in err])
        total = float(err.mean())
    worst = int(np.argmin(frame_db))
    return {"zero": bool(zero_ref.all()), "db": _db(power, total) if np.isfinite(total) else -np.inf, "frame_db": frame_db,
            "worst": (float(frame_db[worst]), worst), "edges": [float(frame_db[i]) for i in (0, 1, -2, -1)],
            "zero_frames_exact": bool((gf[zero_ref] == 0.0).all()), "n_zero_frames": int(zero_ref.sum()), "finite": finite}


def report(tag: str, name: str, key: str, k: Dict[str, object], r: Dict[str, object]) -> str:
    """One printed line: the kernel's figures (k) next to the fp32 restatement's (r)."""
    e = lambda d: "/".join(f"{v:.1f}" for v in d["edges"])
    return (f"{tag} {name:8s} {key}: {k['db']:.1f} dB (fp32 restatement {r['db']:.1f}); worst frame {k['worst'][0]:.1f} dB at "
            f"{k['worst'][1]} (restatement {r['worst'][0]:.1f} at {r['worst'][1]}); first two / last two frames {e(k)} "
            f"(restatement {e(r)}); {k['n_zero_frames']} exactly-zero reference frames")


def check_batch(tag: str, names: Sequence[str], got: Dict[str, np.ndarray], ref64: Dict[str, np.ndarray],
                ref32: Dict[str, np.ndarray], floor: float, exact_zero: Sequence[str] = ()) -> List[tuple]:
    """got / ref64 / ref32: {"s1_pred", "s2_pred"} [len(names)][16 n] of the implementation under test, the fp64 reference and
    the fp32 restatement.  Prints report() per mixture and speaker and returns what is off: every output finite; exactly zero
    in every frame where the fp64 reference is exactly zero (and everywhere for the mixtures in `exact_zero`, whose reference
    must be zero too); otherwise the whole mixture AND its worst 16-sample frame at least `floor` dB.  The restatement's
    own figures are held to the same floor, so a floor the reference arithmetic cannot reach shows as such."""
    bad = []
    for i, name in enumerate(names):
        for key in ("s1_pred", "s2_pred"):
            k, r = judge(got[key][i], ref64[key][i]), judge(ref32[key][i], ref64[key][i])
            print(report(tag, name, key, k, r))
            if not k["finite"]:
                bad.append((name, key, "not finite"))
            if name in exact_zero and not (k["zero"] and np.all(got[key][i] == 0.0)):
                bad.append((name, key, "not exactly zero", k["zero"]))
            if not k["zero_frames_exact"]:
                bad.append((name, key, "nonzero where the reference is exactly zero"))
            if k["zero"]:
                continue                # no signal to relate an error to: judged by equality above
            for what, kv, rv in (("whole mixture", k["db"], r["db"]), ("worst frame", k["worst"][0], r["worst"][0])):
                if not kv >= floor:
                    bad.append((name, key, what, round(kv, 1), "fp32 restatement", round(rv, 1)))
                if not rv >= floor:
                    bad.append((name, key, what, "the fp32 restatement itself is below the floor", round(rv, 1)))
    return bad
