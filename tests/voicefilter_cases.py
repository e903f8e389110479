"""Cases, regimes, references, judgement and the coverage table of the VoiceFilter value tests
(tests/test_voicefilter_values_host.py, tests/test_gpu_voicefilter_values.py).

A case is (F, W, Tv, B, E, regime).  The shapes are chosen by residue: coverage_table() restates the launchers' formulas of
csrc/vfilt.hip (forward) and csrc/vfilt_train.hip (train_forward, train_backward): for every kernel launch the tiled
dimensions, their tile, and for each case the residue class (0, 1, tile - 1, other) of the dimension.  reachable() walks the
box of shapes the tests admit (F in [1, 257], E in {512, 1024}, B <= 9, W <= 65, Tv <= 5, at most 8500 positions) and says
which classes can occur at all; the others stand in UNREACHABLE with the reason.  The host test asserts that the cases meet
every reachable class.

The regimes are named edits of the seeded draw (voicefilter_ref.synthetic_voicefilter_weights, unchanged): `plain`,
`bigmean` (|mean| / sigma >= 50 in front of two BatchNorms), `zerovar` (a channel of variance exactly 0 and a channel that
ReLU kills), `saturated` (LSTM / GRU gates and mask bins at 0 and 1, a mask pre-activation of -100).  Their preconditions
are asserted on the fp64 restatement by the host test.

Judgement: values per column, at most VALUE_FACTOR x the fp32 CPU restatement's worst column of the same tensor; gradients
per tensor under the rule of check_gradients and per slice (out channel / in channel / tap; row / column; gate block) on
the scale of the tensor's RMS slice norm (linear_ln_cases.row_figures), at most GRAD_FACTOR x max(fp32 autograd's worst
slice of the same tensor and kind, GRAD_FLOOR) and below GRAD_BOUND, exact zeros where fp64 has them."""
from __future__ import annotations

from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from tests import voicefilter_ref as R
from tests import voicefilter_train_ref as T
from tests.linear_ln_cases import GRAD_BOUND, GRAD_FACTOR, GRAD_FLOOR, KINK_MARGIN, VALUE_FACTOR, row_figures

HIDDEN, FC = R.HIDDEN, R.FC
PPM, DROP_SEED = 350000, 977
INPUT_SEEDS = (0, 1000, 2000, 3000, 4000, 5000, 6000, 7000)      # offsets on voicefilter_ref.INPUT_SEED + F: the first that meets the kink precondition
REGIMES = ("plain", "bigmean", "zerovar", "saturated")
TRAIN_ONLY = ("zerovar",)            # its preconditions concern batch statistics


class Case(NamedTuple):
    F: int
    W: int
    Tv: int
    B: int
    E: int = 1024
    regime: str = "plain"

    @property
    def shape(self):
        return (self.F, self.W, self.Tv, self.B)

    @property
    def pos(self):
        return self.B * self.F * self.W

    @property
    def id(self):
        return f"{self.F}x{self.W}x{self.Tv}x{self.B}-E{self.E}-{self.regime}"

    @property
    def rms_columns(self):
        """F = 1 (a column is one bin, and the mixture has exact zeros) and `saturated` (bins at -40 and -100) have output
        columns that are zero or denormal: there a column is judged on the RMS column norm of its output, not on its own."""
        return self.F == 1 or self.regime == "saturated"


# (F, W, Tv, B, E): what each shape is there for
SHAPES: Tuple[Tuple[Tuple[int, int, int, int, int], str], ...] = (
    ((17, 7, 1, 3, 1024), "the five shapes of tests/test_gpu_voicefilter_train.py: `other` in most classes; F <= 2 dil for 8 and 16"),
    ((33, 50, 3, 1, 1024), ""),
    ((40, 33, 4, 2, 1024), ""),
    ((201, 21, 5, 2, 1024), "F > 64: all five rows of dilation 16 inside; Tv = 5"),
    ((17, 9, 2, 5, 1024), "2B = 10"),
    ((33, 50, 3, 1, 512), "E = 512"),
    ((16, 8, 2, 8, 1024), "1024 positions exactly, 2B = 16, 2F = 32"),
    ((41, 25, 2, 1, 1024), "1025 positions"),
    ((33, 31, 3, 1, 1024), "1023 positions"),
    ((64, 16, 1, 4, 1024), "4096 positions exactly, 2B = 8, every GEMM dimension in F a tile multiple"),
    ((241, 17, 1, 1, 512), "4097 positions; E = 512"),
    ((63, 65, 2, 1, 1024), "4095 positions, W = 65"),
    ((257, 7, 2, 1, 1024), "the range end: 3F = 771 threads of 1024, VF_FMAX-sized LDS arrays full"),
    ((1, 9, 2, 2, 1024), "the other range end: F = 1, 2B = 4"),
    ((8, 9, 1, 9, 1024), "8F = 64, 2B = 18: a third group of eight sequences"),
    ((43, 3, 5, 1, 1024), "W = 3 < 5: narrower than every kernel; 3F = 129"),
    ((21, 4, 4, 8, 1024), "W = 4; 3F = 63; B W = 32; 2 B Tv = 64"),
    ((11, 31, 1, 1, 1024), "3F = 33 as a K; B W = 31"),
    ((2, 64, 1, 1, 1024), "W = 64; F mod 4 = 2; F <= 2 dil for dilation 4"),
    ((65, 1, 1, 1, 1024), "W = 1; F = 65; B W = 1"),
    ((31, 33, 2, 1, 1024), "F = 31 as a K and an N; W = 33; F mod 4 = 3"),
    ((32, 32, 1, 1, 1024), "3F = 96 as a K; W = 32"),
    ((127, 2, 1, 2, 1024), "F = 127: 63 as an N residue; 2B W = 8"),
    ((107, 63, 1, 1, 1024), "3F = 321 = 1 mod 64; W = 63"),
)
REGIME_SHAPES = ((16, 8, 2, 8), (41, 25, 2, 1), (33, 31, 3, 1))       # positions = 0, 1, 63 mod 64 (1024, 1025, 1023); Tv >= 2
# bigmean's precondition (|mean| / sigma >= 50 on every channel behind a bias of + 50) needs sigma <= 1 on every channel of
# Z_3 and Z_6: at (41, 25) and (33, 31) one channel stands at 49.6, so its residues 1 and 63 come from 4097 and 1023 = 31 x 33
BIGMEAN_SHAPES = ((16, 8, 2, 8), (241, 17, 2, 1), (31, 33, 2, 1))


def _grid() -> List[Case]:
    cases = [Case(*s) for s, _ in SHAPES]
    for regime in REGIMES[1:]:
        cases += [Case(*s, 1024, regime) for s in (BIGMEAN_SHAPES if regime == "bigmean" else REGIME_SHAPES)]
    return cases


CASES = _grid()
BY_ID = {c.id: c for c in CASES}
TRAIN_CASES = list(CASES)
INFER_CASES = [c for c in CASES if c.regime not in TRAIN_ONLY]
TIE_CASES = [Case(*s, 1024, regime) for regime in ("plain", "saturated") for s in REGIME_SHAPES]      # fold against the training chain


# ---------------------------------------------------------------------------------------------------------------------
# coverage: every kernel launch, its tiled dimensions as formulas in F, W, Tv, B, E
# ---------------------------------------------------------------------------------------------------------------------
GEMM_TILES = (("M", 64), ("N", 64), ("K", 32))


def _gemm(phase, name, M, N, K):
    return [(phase, "vfilt_gemm_kernel", name, d, tile, f) for (d, tile), f in zip(GEMM_TILES, (M, N, K))]


def launches() -> List[Tuple[str, str, str, str, int, str]]:
    """[(phase, kernel, launch, dimension, tile, formula)]: phase `infer` is vfilt_forward, `fwd` / `bwd` are
    vftrain_train_forward / vftrain_train_backward.  Formulas are in F, W, Tv, B, E."""
    pos, rows, vrows = "B*F*W", "2*B*W", "2*B*Tv"
    out = []
    for phase in ("infer", "fwd"):
        out += [(phase, "lipfe_conv_kernel", "conv 2..7", "positions", 64, pos)]
        out += _gemm(phase, "gru input 1", "B*Tv" if phase == "infer" else vrows, "3*F", "E")
        out += _gemm(phase, "gru input 2", vrows, "3*F", "2*F")
        out += _gemm(phase, "gru input 2 reverse", "2*B", "3*F", "2*F")
        out += _gemm(phase, "fc_dvector", "2*B", "F", "2*F")
        out += _gemm(phase, "lstm d-vector", "2*B", "1600", "F")
        out += _gemm(phase, "lstm projection", "W", "1600", "8*F")
        out += _gemm(phase, "fc 1", rows, "600", "400")
        out += _gemm(phase, "fc 2", "W" if phase == "infer" else rows, "F", "600")
        step = "vfilt_lstm_step_kernel" if phase == "infer" else "vftrain_lstm_step_kernel"
        gru = "vfilt_gru_kernel" if phase == "infer" else "vftrain_gru_kernel"
        out += [(phase, step, "lstm step", "sequences", 0, "2*B"), (phase, gru, "gru", "F mod 4", 4, "F"), (phase, gru, "gru", "steps", 0, "Tv")]
    out += [("fwd", "vftrain_stat_part_kernel", "batch statistics", "positions", 1024, pos)]
    out += [("bwd", "vftrain_bn_bwd_part_kernel", "BatchNorm backward", "positions", 1024, pos),
            ("bwd", "vftrain_conv8_wgrad_kernel", "conv8 wgrad", "positions", 1024, pos),
            ("bwd", "vftrain_conv1_wgrad_kernel", "conv1 wgrad", "positions", 1024, pos),
            ("bwd", "lipfe_conv_kernel", "conv dgrad 7..2", "positions", 64, pos),
            ("bwd", "vftrain_wgrad_kernel", "conv wgrad 7..2", "K step", 32, pos),
            ("bwd", "vftrain_wgrad_kernel", "conv wgrad 7..2", "chunk", 4096, pos),
            ("bwd", "vftrain_view_t_kernel", "view transpose", "W", 32, "W"),
            ("bwd", "vftrain_view_t_kernel", "view transpose", "8F", 32, "8*F"),
            ("bwd", "vftrain_lstm_bwd_step_kernel", "lstm backward step", "sequences", 0, "2*B"),
            ("bwd", "vftrain_gru_bwd_kernel", "gru backward", "F mod 4", 4, "F"),
            ("bwd", "vftrain_gru_bwd_kernel", "gru backward", "steps", 0, "Tv")]
    out += _gemm("bwd", "fc 2 wgrad", "F", "600", rows)
    out += _gemm("bwd", "fc 2 dgrad", rows, "600", "F")
    out += _gemm("bwd", "fc 1 wgrad", "400", "600", rows)
    out += _gemm("bwd", "fc 1 dgrad", rows, "400", "600")
    out += _gemm("bwd", "lstm W_hh wgrad", "1600", "400", rows)
    out += _gemm("bwd", "lstm W_ih wgrad (map)", "1600", "8*F", "B*W")
    out += _gemm("bwd", "lstm W_ih wgrad (d-vector)", "1600", "F", "2*B")
    out += _gemm("bwd", "d view", "W", "8*F", "1600")
    out += _gemm("bwd", "d dvector", "2*B", "F", "1600")
    out += _gemm("bwd", "fc_dvector wgrad", "F", "2*F", "2*B")
    out += _gemm("bwd", "fc_dvector dgrad", "2*B", "2*F", "F")
    out += _gemm("bwd", "gru 2 W_ih wgrad", "3*F", "2*F", vrows)
    out += _gemm("bwd", "gru 2 W_hh wgrad", "3*F", "F", vrows)
    out += _gemm("bwd", "gru 2 dgrad", vrows, "2*F", "3*F")
    out += _gemm("bwd", "gru 2 reverse W_ih wgrad", "3*F", "2*F", "2*B")
    out += _gemm("bwd", "gru 2 reverse dgrad", "2*B", "2*F", "3*F")
    out += _gemm("bwd", "gru 1 W_ih wgrad", "3*F", "E", vrows)
    out += _gemm("bwd", "gru 1 W_hh wgrad", "3*F", "F", vrows)
    for name, C, r in (("fc.4.bias", "F", rows), ("fc.1.bias", "600", rows), ("lstm gates over time", "1600", "W"),
                       ("lstm biases", "1600", "2*B"), ("fc_dvector.bias", "F", "2*B"), ("gru biases", "3*F", vrows),
                       ("gru 2 reverse biases", "3*F", "2*B")):
        out += [("bwd", "vftrain_colsum_kernel", name, "columns", 64, C), ("bwd", "vftrain_colsum_kernel", name, "rows", 4, r)]
    return out


SEQUENCES = (2, 4, 8, 10, 16, 18)      # 2B: <2> once, then one partly filled group of eight, one full, a second partly filled, two full, a third
STEPS = (1, 2, 5)                      # Tv of the GRU kernels: no recurrence, one recurrent step, several


def residue_class(n: int, tile: int, dim: str) -> str:
    if dim == "sequences":
        return str(n) if n in SEQUENCES else "other"
    if dim == "steps":
        return str(n) if n in STEPS else "other"
    if dim == "F mod 4":
        return str(n % 4)
    r = n % tile
    return str(r) if r in (0, 1, tile - 1) else "other"


def wanted_classes(tile: int, dim: str) -> Tuple[str, ...]:
    if dim == "sequences":
        return tuple(map(str, SEQUENCES))
    if dim == "steps":
        return tuple(map(str, STEPS))
    if dim == "F mod 4":
        return ("0", "1", "2", "3")
    return ("0", "1", str(tile - 1))


def lstm_step_instance(B: int) -> Tuple[str, Tuple[int, int]]:
    """The launchers' choice (vfilt.hip / vfilt_train.hip, forward and backward alike): <2> at two sequences, else <8> in
    groups of eight -> (template argument, grid)."""
    nseq = 2 * B
    return ("<2>", (HIDDEN // 4, 1)) if nseq == 2 else ("<8>", (HIDDEN // 4, (nseq + 7) // 8))


def _value(formula: str, case) -> int:
    return int(eval(formula, {}, dict(F=case.F, W=case.W, Tv=case.Tv, B=case.B, E=case.E)))


def coverage_table(cases=None, phases=("infer", "fwd", "bwd")) -> Dict[Tuple[str, str, str, str], Dict[str, List[str]]]:
    """{(phase, kernel, launch, dimension): {class: [case ids]}}; inference launches count the INFER_CASES only."""
    cases = CASES if cases is None else cases
    table = {}
    for phase, kernel, name, dim, tile, formula in launches():
        if phase not in phases:
            continue
        row = table.setdefault((phase, kernel, name, dim), {})
        for c in cases:
            if phase == "infer" and c.regime in TRAIN_ONLY:
                continue
            row.setdefault(residue_class(_value(formula, c), tile, dim), []).append(c.id)
    return table


BOX = dict(F=257, B=9, W=65, Tv=5, pos=8500)


def reachable() -> Dict[Tuple[str, int, str], set]:
    """{(formula, tile, dimension kind): classes that occur somewhere in the box}"""
    F, B, W, Tv = np.meshgrid(np.arange(1, BOX["F"] + 1), np.arange(1, BOX["B"] + 1), np.arange(1, BOX["W"] + 1),
                              np.arange(1, BOX["Tv"] + 1), indexing="ij")
    ok = (B * F * W <= BOX["pos"]) & (B * F * W >= 2)
    out = {}
    for _, _, _, dim, tile, formula in launches():
        kind = dim if dim in ("sequences", "steps", "F mod 4") else "tile"
        if (formula, tile, kind) in out:
            continue
        seen = set()
        for E in (512, 1024):
            v = np.broadcast_to(np.asarray(eval(formula, {}, dict(F=F, W=W, Tv=Tv, B=B, E=E))), ok.shape)[ok]
            if kind == "sequences":
                seen |= {str(n) for n in SEQUENCES if (v == n).any()}
            elif kind == "steps":
                seen |= {str(n) for n in STEPS if (v == n).any()}
            else:
                r = v % tile
                seen |= {str(k) for k in ((0, 1, 2, 3) if kind == "F mod 4" else (0, 1, tile - 1)) if (r == k).any()}
        out[(formula, tile, kind)] = seen
    return out


_EVEN = "the dimension is even"
_FIXED = "the dimension is fixed by the model"
# (formula, tile) -> {class: why no shape of the box reaches it}
UNREACHABLE: Dict[Tuple[str, int], Dict[str, str]] = {
    ("1600", 64): {"1": _FIXED + ": 1600 = 25 x 64", "63": _FIXED + ": 1600 = 25 x 64"},
    ("1600", 32): {"1": _FIXED + ": 1600 = 50 x 32", "31": _FIXED + ": 1600 = 50 x 32"},
    ("600", 64): {"0": _FIXED + ": 600 = 9 x 64 + 24", "1": _FIXED + ": 600 = 9 x 64 + 24", "63": _FIXED + ": 600 = 9 x 64 + 24"},
    ("600", 32): {"0": _FIXED + ": 600 = 18 x 32 + 24", "1": _FIXED + ": 600 = 18 x 32 + 24", "31": _FIXED + ": 600 = 18 x 32 + 24"},
    ("400", 64): {"0": _FIXED + ": 400 = 6 x 64 + 16", "1": _FIXED + ": 400 = 6 x 64 + 16", "63": _FIXED + ": 400 = 6 x 64 + 16"},
    ("400", 32): {"0": _FIXED + ": 400 = 12 x 32 + 16", "1": _FIXED + ": 400 = 12 x 32 + 16", "31": _FIXED + ": 400 = 12 x 32 + 16"},
    ("E", 64): {"1": "embed_size is 512 or 1024", "63": "embed_size is 512 or 1024"},
    ("E", 32): {"1": "embed_size is 512 or 1024", "31": "embed_size is 512 or 1024"},
    ("2*B", 64): {"0": "2B <= 18 in the box", "1": _EVEN, "63": _EVEN},
    ("2*B", 32): {"0": "2B <= 18 in the box", "1": _EVEN, "31": _EVEN},
    ("2*B", 4): {"1": _EVEN, "3": _EVEN},
    ("2*B*W", 64): {"1": _EVEN, "63": _EVEN},
    ("2*B*W", 32): {"1": _EVEN, "31": _EVEN},
    ("2*B*W", 4): {"1": _EVEN, "3": _EVEN},
    ("2*B*Tv", 64): {"1": _EVEN, "63": _EVEN},
    ("2*B*Tv", 32): {"1": _EVEN, "31": _EVEN},
    ("2*B*Tv", 4): {"1": _EVEN, "3": _EVEN},
    ("B*Tv", 64): {"0": "B Tv <= 45 in the box", "63": "B Tv <= 45 in the box"},
    ("2*F", 64): {"1": _EVEN, "63": _EVEN},
    ("2*F", 32): {"1": _EVEN, "31": _EVEN},
    ("8*F", 64): {"1": "a multiple of 8", "63": "a multiple of 8"},
    ("8*F", 32): {"1": "a multiple of 8", "31": "a multiple of 8"},
}
LEFT_OUT: Tuple[Tuple[str, str, str, str, str], ...] = ()      # (phase, kernel, launch, dimension, class) left out by name: none


def uncovered(cases=None) -> List[Tuple[str, str, str, str, str]]:
    """Reachable classes that no case meets."""
    reach, table, miss = reachable(), coverage_table(cases), []
    for phase, kernel, name, dim, tile, formula in launches():
        kind = dim if dim in ("sequences", "steps", "F mod 4") else "tile"
        for cls in wanted_classes(tile, dim):
            if cls in reach[(formula, tile, kind)] and cls not in table[(phase, kernel, name, dim)]:
                miss.append((phase, kernel, name, dim, cls))
    return miss


GEOMETRY = {      # conditions that must each occur in some case
    "W < 7": lambda c: c.W < 7, "W < 5": lambda c: c.W < 5,
    "F <= 2 dil, dil = 4": lambda c: c.F <= 8, "F <= 2 dil, dil = 8": lambda c: c.F <= 16, "F <= 2 dil, dil = 16": lambda c: c.F <= 32,
    "F > 64": lambda c: c.F > 64,
}
POSITION_EDGES = (1023, 1024, 1025, 4095, 4096, 4097)      # each the position count of some case


# ---------------------------------------------------------------------------------------------------------------------
# weights and inputs
# ---------------------------------------------------------------------------------------------------------------------
_wcache: Dict[tuple, Dict[str, np.ndarray]] = {}
GRU_KEYS = tuple(f"gru.bias_ih_l{l}{s}" for l in range(2) for s in ("", "_reverse"))
DEAD = {"bn": 18, "layer": 4, "channel": 7}            # cnn_layers.18.bias[7] = -50: channel 7 of A_5 is dead
ZEROVAR = {"conv": 13, "layer": 3, "channel": 5}       # cnn_layers.13.weight[5] = 0: channel 5 of Z_4 is its bias


def weights(case: Case, mode: str = "train") -> Dict[str, np.ndarray]:
    """The seeded draw of the case's (F, E) with the regime's named edit; mode: `train` or `infer` (bigmean differs)."""
    key = (case.F, case.E, case.regime, mode if case.regime == "bigmean" else "")
    if key in _wcache:
        return _wcache[key]
    w = {k: np.array(v, copy=True) for k, v in R.synthetic_voicefilter_weights(case.F, case.E, R.WEIGHT_SEED).items()}
    if case.regime == "bigmean":
        for ci, bi in ((9, 10), (21, 22)):
            w[f"cnn_layers.{ci}.bias"] += np.float32(50.0)
            if mode == "infer":
                w[f"cnn_layers.{bi}.running_mean"] += np.float32(50.0)
    elif case.regime == "zerovar":
        w[f"cnn_layers.{ZEROVAR['conv']}.weight"][ZEROVAR["channel"]] = 0.0
        w[f"cnn_layers.{DEAD['bn']}.bias"][DEAD["channel"]] = -50.0
    elif case.regime == "saturated":
        b = w["lstm.bias_ih_l0"]
        for block, every in ((0, 7), (1, 5), (3, 9)):       # i, f, o
            rows = np.arange(0, HIDDEN, every)
            b[block * HIDDEN + rows] += np.where(np.arange(rows.size) % 2 == 0, 30.0, -30.0).astype(np.float32)
        for k in GRU_KEYS:
            w[k][::6] += np.float32(30.0)
        f4 = w["fc.4.bias"]
        f4[0::4] += np.float32(40.0)
        f4[1::4] -= np.float32(40.0)
        assert case.F >= 4
        f4[[2, 3]] = -100.0                                  # two bins the +-40 leave alone: expf(100) overflows in fp32
    elif case.regime != "plain":
        raise ValueError(case.regime)
    _wcache[key] = w
    return w


def inputs(case: Case, k: int = 0):
    return R.synthetic_inputs(case.F, case.W, case.Tv, case.B, case.E, R.INPUT_SEED + case.F + INPUT_SEEDS[k])


def forward64(case: Case, k: int = 0, keep="case", w=None):
    """The fp64 restatement in training mode with its own ReLUs; keep: the case's dropout mask, or None"""
    if isinstance(keep, str):
        keep = T.keep_mask(2 * case.B, case.W, PPM, DROP_SEED)
    return T.forward(weights(case) if w is None else w, *inputs(case, k), torch.float64, keep)


def kink_margin(case: Case, run, keep=None) -> float:
    """The smallest |pre-activation| in front of a ReLU over its layer's RMS, exact zeros aside (a zero-variance channel's
    normalised value and a dropped frame are exact on every side).  The ReLU behind the LSTM sees h = o tanh(c) with o > 0:
    it opens on the sign of c = f c' + i g alone.  Gates of 1e-13 (`saturated`) scale c, h and their rounding alike, so no
    distance from zero on the layer's scale can hold there; what decides the sign is how far the two terms cancel, and the
    margin of that ReLU is |c| / (|f c'| + |i g|), in every regime."""
    worst = np.inf
    pre = []
    for l in range(7):
        p = T.CNN[l][1]
        z, (mean, var) = run.Z[l].detach(), run.stats[l]
        n = z.numel() // z.shape[1]
        xh = (z - mean.detach()[None, :, None, None]) / torch.sqrt(var.detach() * (n - 1) / n + R.BN_EPS)[None, :, None, None]
        g = torch.as_tensor(np.asarray(weights(case)[f"cnn_layers.{p}.weight"])).double()[None, :, None, None]
        b = torch.as_tensor(np.asarray(weights(case)[f"cnn_layers.{p}.bias"])).double()[None, :, None, None]
        pre.append(xh * g + b)
    pre.append(run.fc1.detach())
    n = run.cell.shape[0]
    g, cell = run.gates.detach().view(n, case.W, 4, HIDDEN), run.cell.detach().view(n, case.W, HIDDEN)
    before = torch.cat((torch.zeros_like(cell[:, :1]), cell[:, :-1]), dim=1)
    terms = (g[:, :, 1] * before).abs() + (g[:, :, 0] * g[:, :, 2]).abs()
    live = terms > 0
    worst = min(worst, float((cell.abs()[live] / terms[live]).min()))
    for t in pre:
        a = t.abs()
        rms = float(torch.sqrt((t ** 2).mean()))
        live = a[a > 0]
        if live.numel():
            worst = min(worst, float(live.min()) / rms)
    return worst


_seed_cache: Dict[str, Tuple[int, float]] = {}


def input_seed(case: Case) -> Tuple[int, float]:
    """-> (index into INPUT_SEEDS, its kink margin): the first input draw whose fp64 run keeps every live pre-activation
    further than KINK_MARGIN (relative to its layer's RMS) from a ReLU's kink."""
    if case.id not in _seed_cache:
        for k in range(len(INPUT_SEEDS)):
            m = kink_margin(case, forward64(case, k))
            if m > KINK_MARGIN:
                _seed_cache[case.id] = (k, m)
                break
        else:
            raise AssertionError(f"{case.id}: no input seed keeps the pre-activations off the kink")
    return _seed_cache[case.id]


def d_out(case: Case):
    gen = torch.Generator().manual_seed(case.F + case.W)
    return torch.randn(case.B, case.F, case.W, generator=gen), torch.randn(case.B, case.F, case.W, generator=gen)


# ---------------------------------------------------------------------------------------------------------------------
# preconditions of the regimes, on an fp64 run
# ---------------------------------------------------------------------------------------------------------------------
def check_preconditions(case: Case, run) -> Dict[str, float]:
    """Asserts what the regime claims on `run` (forward64 of the case) and returns the figures."""
    fig = {}
    for s, o in enumerate((run.out1, run.out2)):
        col = o.detach().norm(dim=1)                                   # (B, W): one column per (item, frame)
        fig[f"rms column norm {s + 1}"] = float(torch.sqrt((col ** 2).mean()))
        assert fig[f"rms column norm {s + 1}"] > 0
        if not case.rms_columns:
            assert float(col.min()) > 1e-3, (case.id, float(col.min()))           # judged on their own norm: none near zero
    if case.regime == "bigmean":
        for l in (2, 5):
            mean, var = run.stats[l]
            fig[f"|mean|/sigma Z{l + 1}"] = float((mean.detach().abs() / var.detach().sqrt()).min())
            assert fig[f"|mean|/sigma Z{l + 1}"] >= 50.0, (case.id, l, fig)
        wi = weights(case, "infer")
        for ci, bi in ((9, 10), (21, 22)):      # the fold's cb - running_mean cancels: the difference is a 1/50 of either
            cb, rm = wi[f"cnn_layers.{ci}.bias"].astype(np.float64), wi[f"cnn_layers.{bi}.running_mean"].astype(np.float64)
            assert float(np.abs(cb - rm).max()) < 2.0 and float(np.abs(cb).min()) > 49.0
    elif case.regime == "zerovar":
        l, ch = ZEROVAR["layer"], ZEROVAR["channel"]
        fig["variance of the constant channel"] = float(run.stats[l][1][ch].detach())
        assert fig["variance of the constant channel"] == 0.0, fig
        assert float(run.stats[l][1].detach()[np.arange(64) != ch].min()) > 1e-3
        dead = [int((run.act[k].detach().amax(dim=(0, 2, 3)) <= 0).sum()) for k in range(7)]
        fig["dead channels"] = float(sum(dead))
        assert dead[DEAD["layer"]] == 1 and float(run.act[DEAD["layer"]].detach()[:, DEAD["channel"]].abs().max()) == 0.0, dead
        a = run.act[l].detach()[:, ch]
        assert float(a.max() - a.min()) == 0.0                       # the constant channel: relu(beta) everywhere
    elif case.regime == "saturated":
        assert case.Tv >= 2
        g = run.gates.detach().view(-1, 4, HIDDEN)[:, (0, 1, 3)]
        fig["saturated share of i / f / o"] = float(((g < 1e-4) | (g > 1 - 1e-4)).double().mean())
        assert fig["saturated share of i / f / o"] >= 0.10, fig
        mix = torch.from_numpy(inputs(case, 0)[0]).double()
        mask = torch.where(mix > 0, run.out1.detach() / mix.clamp_min(1e-30), torch.zeros(()).double())
        fig["mask values that are 1 in fp32"] = float((mask.float() == 1.0).sum())
        assert fig["mask values that are 1 in fp32"] >= 1
        fig["smallest live mask value"] = float(mask[mask > 0].min())
        assert fig["smallest live mask value"] < 1e-40               # the bins at -100: below fp32's normal range
    return fig


def swapped(w: Dict[str, np.ndarray], what: str) -> Dict[str, np.ndarray]:
    """`distinct-order`: the draw with two gate blocks or two BatchNorm layers' gamma exchanged, as a mis-indexed pointer would"""
    w = {k: np.array(v, copy=True) for k, v in w.items()}
    if what == "gru r<->z":
        for k in ("gru.weight_hh_l0", "gru.bias_hh_l0", "gru.weight_hh_l1", "gru.bias_hh_l1"):
            F = w[k].shape[0] // 3
            w[k][:F], w[k][F:2 * F] = w[k][F:2 * F].copy(), w[k][:F].copy()
    elif what == "lstm i<->f":
        for k in ("lstm.weight_hh_l0", "lstm.bias_hh_l0"):
            w[k][:HIDDEN], w[k][HIDDEN:2 * HIDDEN] = w[k][HIDDEN:2 * HIDDEN].copy(), w[k][:HIDDEN].copy()
    elif what == "gamma 2<->3":
        w["cnn_layers.6.weight"], w["cnn_layers.10.weight"] = w["cnn_layers.10.weight"], w["cnn_layers.6.weight"]
    else:
        raise ValueError(what)
    return w


SWAPS = ("gru r<->z", "lstm i<->f", "gamma 2<->3")


# ---------------------------------------------------------------------------------------------------------------------
# judgement
# ---------------------------------------------------------------------------------------------------------------------
OUT_KERNEL = "vfilt_gemm_kernel (fc 2) + vftrain_out_kernel"
# (kernel, regime, tensor) -> (asserted factor, the arithmetic behind it)
EXCEPTIONS: Dict[Tuple[str, str, str], Tuple[float, str]] = {
    (OUT_KERNEL, "plain", "out, F = 1"): (
        4.0, "At F = 1 a column is ONE fp32 value, so a tensor's figure is the largest of B W = 18 single rounding draws on "
             "either side, not a norm over F draws.  The standing factor 2 allows the draws of another summation order (600 "
             "products in 32s on MFMA against torch's blocked sum) twice the restatement's sigma; the largest of 18 draws over "
             "the largest of 18 others then passes 2 in half of all cases and 4 in 1.4 % (200 000 simulated pairs of "
             "half-normal maxima).  4 = 2 (sigma) x 2 (the ratio of two maxima of 18, passed in 1.4 % at equal sigma).  The "
             "inference forward, without the dropout scale, gives the restatement's values there bit for bit (ratio 1.00)."),
}


def value_factor(kernel: str, regime: str, tensor: str) -> float:
    return EXCEPTIONS.get((kernel, regime, tensor), (VALUE_FACTOR, ""))[0]


def column_figures(got, ref64, cols: int, rms: bool = False) -> np.ndarray:
    """Per column (the tensors reshaped to (cols, -1)): ||got - ref|| / ||ref||, or over the RMS column norm"""
    g, r = (np.asarray(torch.as_tensor(a).detach().double().reshape(cols, -1)) for a in (got, ref64))
    if rms:
        return row_figures(g, r)
    n = np.sqrt((r ** 2).sum(1))
    e = np.sqrt(((g - r) ** 2).sum(1))
    return np.where(n > 0, e / np.where(n > 0, n, 1.0), np.where(e > 0, np.inf, 0.0))


def judge_columns(tag: str, got, ref64, ref32, cols: int, rms: bool = False, factor: float = VALUE_FACTOR):
    """-> (worst column, the fp32 restatement's worst column, None or what is off); the figures are printed first"""
    if not bool(torch.isfinite(torch.as_tensor(got)).all()):
        return float("inf"), 0.0, f"{tag}: not finite"
    f, y = column_figures(got, ref64, cols, rms), float(column_figures(ref32, ref64, cols, rms).max())
    i = int(np.argmax(f))
    w = float(f[i])
    print(f"{tag}: HIP worst column {w:.3e} (column {i} of {cols}), fp32 CPU worst column {y:.3e}, ratio {w / y if y > 0 else (0.0 if w == 0 else float('inf')):.2f}"
          + (" [on the RMS column norm]" if rms else ""))
    if not w <= factor * y:
        return w, y, f"{tag}: worst column {w:.3g} at column {i} > {factor} x {y:.3g}"
    return w, y, None


RECURRENT_BLOCKS = {"gru.": 3, "lstm.": 4}


def slice_views(key: str, a: np.ndarray) -> Dict[str, np.ndarray]:
    """{slice kind: the tensor as (slices, -1)} of a gradient of two or more dimensions"""
    a = np.asarray(a, np.float64)
    if a.ndim < 2:
        return {}
    if a.ndim == 4:
        co, ci = a.shape[:2]
        t = a.reshape(co, ci, -1)
        out = {"out channel": t.reshape(co, -1), "in channel": np.moveaxis(t, 1, 0).reshape(ci, -1), "tap": np.moveaxis(t, 2, 0).reshape(t.shape[2], -1)}
    else:
        out = {"row": a, "column": a.T}
    for prefix, nb in RECURRENT_BLOCKS.items():
        if key.startswith(prefix):
            out["gate block"] = a.reshape(nb, -1)
    return out


def judge_slices(tag: str, key: str, g, g64, g32) -> Tuple[List[str], float]:
    """Per slice kind: every slice's ||g - g64|| over the RMS slice norm of g64 is < GRAD_BOUND and <= GRAD_FACTOR x
    max(fp32 autograd's worst slice of that kind, GRAD_FLOOR); a slice that is zero in fp64 is zero here.
    -> (what is off, worst figure / bound)"""
    bad, worst = [], 0.0
    v, v64, v32 = slice_views(key, g), slice_views(key, g64), slice_views(key, g32)
    for kind in v64:
        if not np.isfinite(v[kind]).all():
            bad.append(f"{tag} {key} per {kind}: not finite")
            continue
        zero = (v64[kind] == 0).all(1)
        nz = np.flatnonzero(zero & (v[kind] != 0).any(1))
        if nz.size:
            bad.append(f"{tag} {key}: {kind} {int(nz[0])} is zero in fp64 and not here ({nz.size} such)")
        if zero.all():
            continue
        f, f32 = row_figures(v[kind], v64[kind]), row_figures(v32[kind], v64[kind])
        lim = min(GRAD_BOUND, GRAD_FACTOR * max(float(f32.max()), GRAD_FLOOR))
        i = int(np.argmax(f))
        worst = max(worst, float(f[i]) / lim)
        print(f"{tag} {key} per {kind}: worst {float(f[i]):.3g} at {i} of {len(f)}, fp32 autograd {float(f32.max()):.3g}, bound {lim:.3g}")
        if not float(f[i]) <= lim:
            bad.append(f"{tag} {key}: {kind} {i} off by {float(f[i]):.3g} of the RMS {kind} norm (bound {lim:.3g}; {int((f > lim).sum())} off)")
    return bad, worst


def exact_zeros(tag: str, key: str, g, g64) -> List[str]:
    """Every element that is exactly zero in fp64 autograd is exactly zero here"""
    g, g64 = np.asarray(g, np.float64), np.asarray(g64, np.float64)
    off = (g64 == 0) & (g != 0)
    return [f"{tag} {key}: {int(off.sum())} elements are zero in fp64 and not here"] if off.any() else []


# which kernel(s) a judged tensor speaks for: the worst-ratio table is kept per (kernel, regime)
TENSOR_KERNEL = {"Z1": "vftrain_conv1_kernel", "Z8": "vfilt_conv8_kernel", "A": "vftrain_norm_kernel", "mean": "vftrain_stat_*", "var": "vftrain_stat_*",
                 "Z": "lipfe_conv_kernel", "gates": "vftrain_lstm_step_kernel", "cell": "vftrain_lstm_step_kernel", "h": "vftrain_lstm_step_kernel",
                 "Y1": "vfilt_gemm_kernel (fc 1)", "out": OUT_KERNEL}


def kernel_of_tensor(name: str) -> str:
    if name in TENSOR_KERNEL:
        return TENSOR_KERNEL[name]
    return TENSOR_KERNEL[name.rstrip("0123456789")]


def kernel_of_gradient(key: str) -> str:
    if key.startswith("gru."):
        return "vftrain_gru_bwd_kernel + GEMM / colsum"
    if key.startswith("lstm."):
        return "vftrain_lstm_bwd_step_kernel + GEMM / colsum"
    if key.startswith("fc"):
        return "FC tail backward (GEMM / colsum / dsig)"
    idx = int(key.split(".")[1])
    if idx in (1, 28):
        return "conv1 / conv8 wgrad"
    if key.endswith(".weight") and idx in (5, 9, 13, 17, 21, 25):
        return "vftrain_wgrad_kernel"
    return "vftrain_bn_bwd_*"
