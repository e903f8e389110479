"""TEST INFRASTRUCTURE: the cases of the recurrence tests and their CPU references, computed once per process and shared,
read-only, by tests/test_recurrence_host.py and tests/test_gpu_recurrence.py.

The LSTM recurrence of a DPTN / DPRNN path runs through six inference kernels, chosen in route_path (kernel_for() restates
the rule), here named by the FORMS that select them:

  form  options on top of the defaults           kernel                                  tile of sequences
  16x   lstm4 = 0, fuse_pre = 1, fuse_pre128 = 2  lstm16x.hip (input projection inside)   16
  16    lstm4 = 0, fuse_pre = 0, fuse_pre128 = 0  K4 GEMM + lstm16.hip                    16
  4     lstm4 = 2                                 K4 GEMM + lstm4.hip                     4
  32    lstm16 = 0                                K4 GEMM + lstm.hip, fp32                32
  16s   split_bf16 = 1                            split K4 + lstm16s.hip                  16
  32s   split_bf16 = 1, lstm16 = 0                split K4 + lstm.hip, split              32

A case is (arch, features, path, nseq, len, regime, B, bidir): one block, hidden 128, weights synthetic_state_dict(cfg, 9).
  path 0    intra-chunk, tokens contiguous: S = nseq, chunk_size = len               -> B * nseq sequences of len positions
  path 1    inter-chunk, tokens strided:    chunk_size = nseq, step_size 1, S = len  -> B * nseq sequences, token stride nseq
  x         standard normal [B, S, K, N], seeded per shape

JUDGED is the "hc" workspace tap after DptnEngine.stage_path: [tokens][ndir * 128], ReLU(h) for DPTN and raw h for DPRNN.
The LSTM's input is taken from the device -- the "y1" tap of the same run for DPTN, x itself for DPRNN -- so nothing in front of
the recurrence enters the figure; the host test uses the fp64 formula's y1, rounded to fp32, in its place.  Every reference is
computed on exactly those fp32 values (references()):

  truth   an explicit step loop at fp64 with torch.sigmoid / torch.tanh (pinned to torch.nn.LSTM and the numpy oracle)
  k32     the same loop at fp32 with the kernels' gate formulas (common.h): sigmoid = 1 / (1 + exp2(-log2e a)),
          tanh = 2 / (1 + exp2(-2 log2e a)) - 1, also for tanh(c)
  split   k32 with every product A W^T (input projection and recurrent) taken as Ah Wh + Ah Wl + Al Wh, hi = bf16(v),
          lo = bf16(v - hi), fp32 accumulation: the three-MFMA scheme of mfma3 (the restatement of the 16s / 32s forms)

The figure is per UNIT = one (sequence, position, direction), 128 values: the reference's mean power over the whole tensor
divided by that unit's mean squared error (train_attention_cases.figures on the tensor as [units, 128]).

REGIMES.  A regime changes the path's rnn.* tensors before they are bound, or x for DPRNN:
  plain      nothing
  saturated  W_ih x 8, W_hh x 4: gates at their rails, max |h| = 1.000
  open       bias_ih + 3 on the input gate and + 6 on the forget gate, W_ih x 4: the cell accumulates
  quiet      the LSTM's input x 1e-4.  DPRNN: x itself.  DPTN reads LayerNorm output, which no scaling of x changes, so W_ih
             x 1e-4 there -- the same pre-activations
  loud       DPRNN: x x 1000; exp2 overflows to inf, which the formula turns into 0 or 1
  silent     DPRNN: the last sequence all zeros (its units are judged like any other: the bias keeps h != 0)
  mixed      DPRNN: sequence q x 10^(q mod 7 - 3): one tile holds quiet and overflowing rows side by side
The split forms are left out of loud and mixed: their own arithmetic restated here reaches only 59 dB there.
Left out of the regimes because no fp32 evaluation can be judged there: W_hh x 8 (chaotic; the fp32 restatement falls to -5 dB
at 150 positions) and the open bias without W_ih x 4 (drifts to 78.6 dB at 257).

FLOORS come from the restatement, never from a kernel:  floor = min(100 dB, worst unit of the form's restatement - 20 dB), k32
for the fp32 forms and split for the split forms.  100 dB is STAGE_FLOOR_DB of the attention grid; 20 dB is the distance that
grid keeps between its bars, here the allowance for 1-ulp v_exp_f32 / v_rcp_f32 against libm and another order of summation.

PRECONDITIONS (asserted on the CPU before a kernel result is looked at):
  * the restatement's worst unit is at or above the regime's bar (RESTATEMENT_BARS: what the generator was measured to give);
  * either DEFECT in the fp64 formula, at the last sequence of the last tile, leaves the worst unit at or below every floor
    of the case - 10 dB:
      skip  the last direction (reverse where there are two) skips its first step: that position stays zero and the state
            starts one step late -- a loop bound off by one
      row   at the last step of that direction the recurrent product reads the previous sequence's h (the zero state where
            there is one sequence) -- a tile row off by one.  Not at len = 1, where every row of h is the zero state and the
            defect changes nothing.
  * the launch geometry (stage_geometry) and the route (kernel_for, launch counts from profile_read).
"""
from __future__ import annotations

import functools
import hashlib
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from speech_separation_amd.spec import DPRNN_AUDIO, DPTN_AUDIO, DPTN_AV, DPTNConfig, synthetic_state_dict
from tests.infer_attention_cases import STAGE_FLOOR_DB, _params, _to_seqs, _to_tokens, half
from tests.train_attention_cases import WEIGHT_SEED, figures

H = 128
ARCHS = (("dptn", 128), ("dptn", 64), ("dprnn", 64), ("dprnn", 128))
NSEQ = (1, 4, 5, 16, 17, 32, 33, 49)      # one tile or fewer; full and one over for tiles of 4, 16, 32; four tiles of 16
LENGTHS = (1, 2, 33)                      # 1 and 2: nothing for the double-buffered h and the operand read-ahead to read ahead of
LONG = 150                                # at nseq 17 only
SPAN_CHUNKS = (9, 17)                     # path 1, B = 2: a tile of 16 / of 32 holds sequences of two mixtures
VALUE_NSEQ, VALUE_LENGTHS = 17, (33, 150)
WEIGHT_REGIMES = ("saturated", "open")
INPUT_REGIMES = ("quiet", "loud", "silent", "mixed")
DPTN_REGIMES = ("plain", "saturated", "open", "quiet")
DPRNN_REGIMES = DPTN_REGIMES + ("loud", "silent", "mixed")
NO_SPLIT = ("loud", "mixed")

FORMS: Dict[str, Dict[str, int]] = {
    "16x": {"lstm4": 0, "fuse_pre": 1, "fuse_pre128": 2},
    "16": {"lstm4": 0, "fuse_pre": 0, "fuse_pre128": 0},
    "4": {"lstm4": 2},
    "32": {"lstm16": 0},
    "16s": {"split_bf16": 1},
    "32s": {"split_bf16": 1, "lstm16": 0},
}
DEFAULTS = {"lstm16": 1, "lstm4": 1, "fuse_pre": 1, "fuse_pre128": 1, "split_bf16": 0}      # dptnav.hip's own
SPLIT_FORMS = ("16s", "32s")
KERNELS = {"lstm16x": 16, "lstm16": 16, "lstm4": 4, "lstm32": 32, "lstm16s": 16, "lstm32s": 32}      # -> its tile of sequences
# (form, regime) pairs left out by name beyond the split x {loud, mixed} pairs of NO_SPLIT (the issue allows two): none
LEFT_OUT: Tuple[Tuple[str, str], ...] = ()

MARGIN_DB = 20.0
DEFECT_MARGIN_DB = 10.0
DEFECTS = ("skip", "row")
# the worst unit of the restatement, at least: the k32 bar per regime, and the split bar
RESTATEMENT_BARS = {"plain": 115.0, "saturated": 115.0, "open": 115.0, "quiet": 115.0, "silent": 115.0, "loud": 85.0,
                    "mixed": 85.0}      # (mixed holds the loud rows)
SPLIT_BAR = 88.0
PIN_DB = 250.0      # truth against torch.nn.LSTM and the numpy oracle, both fp64

# tuple(case) -> input seed of the cases whose first seed, 0, missed a precondition: the first of 1, 2, ... that meets them all,
# searched on the CPU (python -m tests.recurrence_cases --search prints this table with what seed 0 missed)
SEED_OVERRIDES: Dict[tuple, int] = {
    ("dptn", 128, 0, 17, 150, "open", 1, True): 1,       # seed 0: k32 restatement 114.7 dB under its 115 dB bar
    ("dprnn", 128, 0, 17, 33, "loud", 1, True): 1,       # seed 0: the row defect at 79.8 dB, lowest floor 69.3 (every gate
    ("dprnn", 128, 0, 17, 150, "loud", 1, True): 2,      # seed 0: ... at 93.0 dB, 65.4   of the last step driven to a rail)
    ("dprnn", 128, 0, 17, 150, "mixed", 1, True): 1,     # seed 0: k32 restatement 84.6 dB under its 85 dB bar
}


class Case(NamedTuple):
    arch: str
    features: int
    path: int
    nseq: int            # sequences per mixture: S on path 0, chunk_size on path 1
    len: int
    regime: str = "plain"
    B: int = 1
    bidir: bool = True

    @property
    def id(self) -> str:
        return (f"{self.arch}{self.features}-path{self.path}-nseq{self.nseq}-len{self.len}-{self.regime}"
                + (f"-B{self.B}" if self.B != 1 else "") + ("" if self.bidir else "-unidir"))

    @property
    def ndir(self) -> int:
        return 2 if self.bidir or self.path == 0 else 1      # (the intra-chunk LSTM always has both directions)

    @property
    def total(self) -> int:
        return self.B * self.nseq


def _grid() -> Tuple[List[Case], List[Case]]:
    geometry, value = [], []
    for arch, f in ARCHS:
        for path in (0, 1):
            for nseq in NSEQ:
                for ln in LENGTHS + ((LONG,) if nseq == VALUE_NSEQ else ()):
                    geometry.append(Case(arch, f, path, nseq, ln))
        for chunk in SPAN_CHUNKS:
            for ln in LENGTHS:
                geometry.append(Case(arch, f, 1, chunk, ln, B=2))
        geometry.append(Case(arch, f, 1, VALUE_NSEQ, 33, bidir=False))
        for regime in (DPTN_REGIMES if arch == "dptn" else DPRNN_REGIMES):
            if regime == "plain":
                continue      # (the geometry grid has nseq 17 at both lengths)
            for path in (0, 1):
                for ln in VALUE_LENGTHS:
                    value.append(Case(arch, f, path, VALUE_NSEQ, ln, regime))
    return geometry, value


GEOMETRY_CASES, VALUE_CASES = _grid()
CASES = GEOMETRY_CASES + VALUE_CASES


# ---------------------------------------------------------------------------------------------------------------------
# the route, restated
# ---------------------------------------------------------------------------------------------------------------------
def forms(case: Case) -> Dict[str, Dict[str, int]]:
    """form -> the options that select it, for the forms the case runs."""
    return {f: o for f, o in FORMS.items()
            if not (f in SPLIT_FORMS and case.regime in NO_SPLIT) and (f, case.regime) not in LEFT_OUT}


def kernel_for(form: str, case: Case, num_cus: int = 256) -> str:
    """route_path / lstm_use16 of dptnav.hip for an inference stage_path call with the form's options.  The rule also reads
    the diagnostic option lstm_stamps (it rules out lstm4 and lstm16x); no test here sets it, so it is taken at its default 0."""
    o = {**DEFAULTS, **FORMS[form]}
    B, S, K = shape(case)[:3]
    M, ndir = B * S * K, case.ndir
    nst16, nst4 = (case.total + 15) // 16, (case.total + 3) // 4
    fits32 = (M + S * K) * ndir * H * 4 < 2 ** 32
    use16 = bool(o["lstm16"]) and nst16 * ndir <= num_cus and fits32
    split = bool(o["split_bf16"])
    rounds20 = 30 if 0 < B <= 10 else 23
    lstm_stamps = 0
    use4 = use16 and not split and not lstm_stamps and (o["lstm4"] == 2 or (o["lstm4"] == 1 and 20 * nst4 * ndir <= rounds20 * num_cus))
    fuse128 = o["fuse_pre128"] == 2 or (o["fuse_pre128"] == 1 and B >= 12)
    usex = bool(o["fuse_pre"] if case.features == 64 else fuse128 and fits32) and bool(o["lstm16"]) and not split and not use4 and not lstm_stamps
    return ("lstm16x" if usex else "lstm16s" if use16 and split else "lstm4" if use4 else "lstm16" if use16
            else "lstm32s" if split else "lstm32")


def k4_launches(form: str, case: Case) -> int:
    """Launches of the lstm_pre_gemm category: the input projection runs inside lstm16x.hip."""
    return 0 if kernel_for(form, case) == "lstm16x" else 1


def tile_edges(case: Case, tile: int) -> List[str]:
    """Which edges of a tile of `tile` sequences the case's sequence count is at."""
    n, out = case.total, []
    if case.B > 1:
        return ["spans"] if case.path == 1 and case.nseq % tile else []
    if n < tile:
        out.append("below")
    if n % tile == 0:
        out.append("full")
    if n > tile and n % tile == 1:
        out.append("over")
    return out


def coverage_keys(form: str, case: Case) -> set:
    k = kernel_for(form, case)
    return {(k, case.features, case.arch, case.path, e) for e in tile_edges(case, KERNELS[k])}


def coverage_table() -> set:
    """Every (kernel, features, arch, path, tile edge): below, full and one over on both paths, two mixtures in one tile on
    the strided path."""
    return {(k, f, arch, path, e) for k in KERNELS for arch, f in ARCHS
            for path, edges in ((0, ("below", "full", "over")), (1, ("below", "full", "over", "spans"))) for e in edges}


def grid_coverage(cases=None) -> set:
    have = set()
    for c in (GEOMETRY_CASES if cases is None else cases):
        for form in forms(c):
            have |= coverage_keys(form, c)
    return have


# ---------------------------------------------------------------------------------------------------------------------
# configuration, weights, inputs
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def config(case: Case) -> DPTNConfig:
    base = {("dptn", 128): DPTN_AV, ("dptn", 64): DPTN_AUDIO, ("dprnn", 64): DPRNN_AUDIO,
            ("dprnn", 128): DPTNConfig(**{**DPRNN_AUDIO.to_dict(), "num_features": 128, "hidden_video": 128})}[case[:2]]
    chunk, step = (case.len, max(case.len // 2, 1)) if case.path == 0 else (case.nseq, 1)
    return DPTNConfig(**{**base.to_dict(), "num_blocks": 1, "chunk_size": chunk, "step_size": step, "hidden_dim": H,
                         "num_heads": 4, "bidir": case.bidir})


def shape(case: Case) -> Tuple[int, int, int, int]:
    """(B, S, K, N) of x."""
    return (case.B, case.nseq, case.len, case.features) if case.path == 0 else (case.B, case.len, case.nseq, case.features)


def prefix(case: Case) -> str:
    return "dprnn.model.0.%s." % ("intra_chunk_block" if case.path == 0 else "inter_chunk_block")


def stage_geometry(case: Case) -> Dict[str, int]:
    """What the GPU test hands to the library, restated on the host: T as DptnEngine._path_T derives it, the chunk count it
    gives back, the tokens, the row width of hc and the floats of the taps (the plan sizes hc for two directions always)."""
    cfg = config(case)
    B, S, K, N = shape(case)
    L = (S - 1) * cfg.step_size + cfg.chunk_size
    T = (L - 1) * cfg.stride_enc + cfg.kernel_size_enc
    assert cfg.chunk_size == K <= 256 and cfg.frames(T) == L and cfg.chunks(L) == S, case.id
    assert (case.nseq, case.len) == ((S, K) if case.path == 0 else (K, S)), case.id
    M = B * S * K
    assert (B + 1) * S * K * max(3 * N, 2 * H) < 2 ** 31, case.id      # make_plan's 32-bit token indexing bound
    return {"B": B, "S": S, "K": K, "N": N, "T": T, "Tv": 1, "M": M, "ldh": case.ndir * H, "y1_floats": M * N,
            "hc_floats": M * 2 * H}


@functools.lru_cache(maxsize=None)
def weights(case: Case) -> Dict[str, np.ndarray]:
    """The whole model's state_dict with the regime applied to the path's rnn.* tensors; read-only."""
    sd = synthetic_state_dict(config(case), seed=WEIGHT_SEED)
    pre = prefix(case) + "rnn."
    for k in [k for k in sd if k.startswith(pre)]:
        leaf, v = k[len(pre):], sd[k]
        if case.regime == "saturated":
            v = v * 8 if leaf.startswith("weight_ih") else v * 4 if leaf.startswith("weight_hh") else v
        elif case.regime == "open":
            if leaf.startswith("weight_ih"):
                v = v * 4
            elif leaf.startswith("bias_ih"):
                v = v.copy()
                v[:H] += 3
                v[H:2 * H] += 6
        elif case.regime == "quiet" and case.arch == "dptn" and leaf.startswith("weight_ih"):
            v = v * 1e-4
        sd[k] = np.ascontiguousarray(v, dtype=np.float32)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def input_seed(case: Case) -> int:
    return SEED_OVERRIDES.get(tuple(case), 0)


@functools.lru_cache(maxsize=None)
def inputs(case: Case, seed: Optional[int] = None) -> np.ndarray:
    """x fp32 [B, S, K, N] with the regime applied (DPRNN), read-only.  seed: another than input_seed(case) (the seed search)."""
    B, S, K, N = shape(case)
    seed = input_seed(case) if seed is None else seed
    x = np.random.default_rng([case.path, case.nseq, case.len, case.B, case.features, seed]).standard_normal((B, S, K, N))
    if case.arch == "dprnn" and case.regime in INPUT_REGIMES:
        seqs = _to_seqs(torch.from_numpy(x), case.path).clone()      # [R, len, N]
        if case.regime == "quiet":
            seqs *= 1e-4
        elif case.regime == "loud":
            seqs *= 1000.0
        elif case.regime == "silent":
            seqs[-1] = 0
        elif case.regime == "mixed":
            seqs *= torch.tensor([10.0 ** (q % 7 - 3) for q in range(seqs.shape[0])], dtype=seqs.dtype)[:, None, None]
        x = np.array(_to_tokens(seqs, case.path, B, S, K)).reshape(B, S, K, N)
    else:
        assert case.regime not in INPUT_REGIMES or (case.arch == "dptn" and case.regime == "quiet"), case.id
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


class LstmInput:
    """The fp32 values the recurrence reads, [tokens, N], hashable by content (references() is cached on it)."""

    def __init__(self, a: np.ndarray):
        self.a = np.ascontiguousarray(a, dtype=np.float32)
        self.a.setflags(write=False)
        self._digest = hashlib.sha1(self.a.tobytes()).digest()

    def __hash__(self):
        return hash(self._digest)

    def __eq__(self, other):
        return isinstance(other, LstmInput) and self._digest == other._digest and self.a.shape == other.a.shape


@functools.lru_cache(maxsize=None)
def host_lstm_input(case: Case, seed: Optional[int] = None) -> LstmInput:
    """DPRNN: x.  DPTN: y1 = LN1(MHA(x) + x) by the fp64 formula, rounded to fp32 (the GPU test reads the y1 tap instead)."""
    B, S, K, N = shape(case)
    x = inputs(case, seed)
    if case.arch == "dprnn":
        return LstmInput(x.reshape(-1, N))
    P = _params(weights(case), prefix(case), torch.float64)
    y1 = half(_to_seqs(torch.from_numpy(np.array(x)).double(), case.path), P, upto="y1")["y1"]
    return LstmInput(_to_tokens(y1, case.path, B, S, K))


# ---------------------------------------------------------------------------------------------------------------------
# the recurrence by explicit step loops
# ---------------------------------------------------------------------------------------------------------------------
LOG2E = 1.4426950408889634


def _bf16_split(v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    hi = v.to(torch.bfloat16).to(torch.float32)
    return hi, (v - hi).to(torch.bfloat16).to(torch.float32)


class _Arith:
    """How one reference multiplies and squashes: "truth" (fp64, torch's functions), "k32" (fp32, the kernels' gate
    formulas), "split" (k32 with three-term bf16 hi / lo products)."""

    def __init__(self, mode: str):
        assert mode in ("truth", "k32", "split")
        self.mode = mode
        self.dtype = torch.float64 if mode == "truth" else torch.float32

    def weight(self, w: torch.Tensor):
        """W [J, K] -> what prod() takes."""
        wt = w.to(self.dtype).t().contiguous()
        return _bf16_split(wt) if self.mode == "split" else wt

    def prod(self, a: torch.Tensor, wt) -> torch.Tensor:
        if self.mode != "split":
            return a @ wt
        (ah, al), (wh, wl) = _bf16_split(a), wt
        return ah @ wh + ah @ wl + al @ wh

    def sigmoid(self, a: torch.Tensor) -> torch.Tensor:
        return torch.sigmoid(a) if self.mode == "truth" else 1.0 / (1.0 + torch.exp2(a * -LOG2E))

    def tanh(self, a: torch.Tensor) -> torch.Tensor:
        return torch.tanh(a) if self.mode == "truth" else 2.0 / (1.0 + torch.exp2(a * (-2.0 * LOG2E))) - 1.0


def lstm_direction(x: torch.Tensor, w: Dict[str, torch.Tensor], reverse: bool, mode: str = "truth",
                   defect: Optional[str] = None, cells: bool = False):
    """One direction of nn.LSTM(batch_first = True) from the zero state: x [R, len, N] -> h [R, len, H].
    w: weight_ih [4H, N], weight_hh [4H, H], bias_ih, bias_hh, gate rows in the order i | f | g | o.
    defect (the LAST row of x only): "skip" / "row" of the header.  cells: -> (h, c), c [R, len, H] the cell states."""
    ar = _Arith(mode)
    x = x.to(ar.dtype)
    R, L, N = x.shape
    w_ih, w_hh = ar.weight(w["weight_ih"]), ar.weight(w["weight_hh"])
    bias = w["bias_ih"].to(ar.dtype) + w["bias_hh"].to(ar.dtype)
    with torch.no_grad():
        pre = (ar.prod(x.reshape(R * L, N), w_ih) + bias).reshape(R, L, 4 * H)
        h = torch.zeros(R, H, dtype=ar.dtype)
        c = torch.zeros(R, H, dtype=ar.dtype)
        out = torch.zeros(R, L, H, dtype=ar.dtype)
        cs = torch.zeros(R, L, H, dtype=ar.dtype)
        order = list(range(L - 1, -1, -1) if reverse else range(L))
        for n, t in enumerate(order):
            hr = h
            if defect == "row" and n == L - 1:
                hr = h.clone()
                hr[-1] = h[-2] if R > 1 else 0.0
            g = pre[:, t] + ar.prod(hr, w_hh)
            c = ar.sigmoid(g[:, H:2 * H]) * c + ar.sigmoid(g[:, :H]) * ar.tanh(g[:, 2 * H:3 * H])
            h = ar.sigmoid(g[:, 3 * H:]) * ar.tanh(c)
            if defect == "skip" and n == 0:
                h[-1] = 0.0
                c[-1] = 0.0
            out[:, t] = h
            cs[:, t] = c
    return (out, cs) if cells else out


def _rnn_weights(case: Case) -> List[Dict[str, torch.Tensor]]:
    """[direction] -> {weight_ih, weight_hh, bias_ih, bias_hh} fp32 of the case's path."""
    sd, pre = weights(case), prefix(case) + "rnn."
    return [{leaf: torch.from_numpy(np.array(sd[f"{pre}{leaf}_l0{suffix}"])) for leaf in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")}
            for suffix in ("", "_reverse")[:case.ndir]]


def _seqs_of(case: Case, lstm_in: np.ndarray) -> torch.Tensor:
    B, S, K, N = shape(case)
    return _to_seqs(torch.from_numpy(np.array(lstm_in)).reshape(B, S, K, N), case.path)


def _hc(case: Case, dirs: List[torch.Tensor]) -> np.ndarray:
    """[direction] of h [R, len, H] -> the hc tap: [tokens, ndir * H] at fp64, ReLU for DPTN; read-only."""
    B, S, K, _ = shape(case)
    h = torch.cat(dirs, -1).double()
    return _to_tokens(torch.relu(h) if case.arch == "dptn" else h, case.path, B, S, K)


def recurrence(case: Case, lstm_in: np.ndarray, mode: str) -> np.ndarray:
    seqs, W = _seqs_of(case, lstm_in), _rnn_weights(case)
    return _hc(case, [lstm_direction(seqs, W[d], d == 1, mode) for d in range(case.ndir)])


@functools.lru_cache(maxsize=None)
def references(case: Case, lstm_in: LstmInput) -> Dict[str, np.ndarray]:
    """{"truth", "k32", "split" where a split form runs}: hc [tokens, ndir * H] on the given input values; read-only."""
    modes = ("truth", "k32") + (("split",) if any(f in SPLIT_FORMS for f in forms(case)) else ())
    return {m: recurrence(case, lstm_in.a, m) for m in modes}


@functools.lru_cache(maxsize=None)
def defective(case: Case, lstm_in: LstmInput, defect: str) -> np.ndarray:
    """The fp64 formula with the defect at the last sequence of the last tile, in the last direction.  Rows of a batch do not
    meet in the recurrence, so only the last two sequences are recomputed and the last one replaced in the truth."""
    assert defect in DEFECTS
    seqs, W = _seqs_of(case, lstm_in.a), _rnn_weights(case)
    R, d = seqs.shape[0], case.ndir - 1
    B, S, K, _ = shape(case)
    truth = torch.from_numpy(np.array(references(case, lstm_in)["truth"]))
    hs = _to_seqs(truth.reshape(B, S, K, case.ndir * H), case.path).clone()      # [R, len, ndir H]
    bad = lstm_direction(seqs[-2:], W[d], d == 1, "truth", defect)[-1]
    hs[R - 1, :, d * H:(d + 1) * H] = torch.relu(bad) if case.arch == "dptn" else bad
    return _to_tokens(hs, case.path, B, S, K)


# ---------------------------------------------------------------------------------------------------------------------
# figures, floors, judging
# ---------------------------------------------------------------------------------------------------------------------
def unit_figures(got: np.ndarray, ref: np.ndarray) -> Tuple[float, float, int]:
    """(whole-tensor dB, worst unit dB, that unit = token * ndir + direction)."""
    return figures(np.asarray(got).reshape(-1, H), np.asarray(ref).reshape(-1, H))


def restatement_for(form: str) -> str:
    return "split" if form in SPLIT_FORMS else "k32"


def floor_db(form: str, refs: Dict[str, np.ndarray]) -> float:
    """min(100, worst unit of the form's restatement on these inputs - 20)."""
    return min(STAGE_FLOOR_DB, unit_figures(refs[restatement_for(form)], refs["truth"])[1] - MARGIN_DB)


def floors(case: Case, refs: Dict[str, np.ndarray]) -> Dict[str, float]:
    return {form: floor_db(form, refs) for form in forms(case)}


def check_restatements(case: Case, refs: Dict[str, np.ndarray]) -> Dict[str, float]:
    """Every restatement's worst unit at or above its bar."""
    out: Dict[str, float] = {}
    for m in refs:
        if m == "truth":
            continue
        whole, worst, unit = unit_figures(refs[m], refs["truth"])
        out[m], out[m + ".unit"] = whole, worst
        bar = SPLIT_BAR if m == "split" else RESTATEMENT_BARS[case.regime]
        assert worst >= bar, (case.id, m, "restatement, worst unit", worst, unit, "bar", bar)
    return out


def check_defects(case: Case, lstm_in: LstmInput) -> Dict[str, float]:
    """Either defect at or below the lowest floor of the case - 10 dB."""
    refs = references(case, lstm_in)
    lowest = min(floors(case, refs).values())
    out = {"floor.min": lowest}
    for d in DEFECTS:
        if d == "row" and case.len == 1:
            continue      # (every row of h is the zero state at the only step)
        whole, worst, unit = unit_figures(defective(case, lstm_in, d), refs["truth"])
        out[d], out[d + ".unit"] = whole, worst
        assert worst <= lowest - DEFECT_MARGIN_DB, (case.id, d, "defect, worst unit", worst, unit, "lowest floor", lowest)
    return out


def check_preconditions(case: Case, lstm_in: Optional[LstmInput] = None) -> Dict[str, float]:
    """Asserts the preconditions of the case on the given input of the recurrence (default: the host's); -> the figures."""
    stage_geometry(case)
    lstm_in = host_lstm_input(case) if lstm_in is None else lstm_in
    return {**check_restatements(case, references(case, lstm_in)), **check_defects(case, lstm_in)}


def judge(what: str, got: np.ndarray, ref: np.ndarray, floor: float) -> Tuple[float, float, int]:
    """Finite, the reference's shape, every unit at `floor` dB or better -> unit_figures(); AssertionError otherwise."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    whole, worst, unit = unit_figures(got, ref)
    assert worst >= floor, (what, "worst unit", round(worst, 1), "dB at unit", unit, "floor", round(floor, 1), "whole tensor", round(whole, 1))
    return whole, worst, unit


# ---------------------------------------------------------------------------------------------------------------------
# training forward and BPTT: lstm16.hip / lstm.hip with the tape, lstm_bptt16.hip / lstm_bptt.hip (option lstm16 = 1 / 0)
# ---------------------------------------------------------------------------------------------------------------------
# A training case is a Case run through train_path_forward / train_path_backward, once per entry of TRAIN_FORMS.  Judged: y
# (every token; and against the inference forward of the same tile height, 120 dB), dx (every token) and the eight rnn.*
# gradients (per tensor), against fp64 autograd of the explicit half -- DPTN: attention, LN1, bi-LSTM, ReLU, FFN, LN2; DPRNN:
# bi-LSTM, fc, LayerNorm, + x -- with fp32 autograd of the same formula as the restatement:
#   floor = min(80, restatement's worst token - 20) for y and dx, min(70, restatement - 20) per parameter tensor.
# PRECONDITION (DPTN): the ReLU behind the LSTM reads the sign of h = o tanh(c).  Where fp32 and fp64 disagree on it the
# gradient of that unit differs by a finite amount with every kernel right, so the smallest |h| must be >= MIN_RELU_INPUT in
# fp64 (the attention grid's precondition; TRAIN_SEED_OVERRIDES).
# LEFT OUT BY NAME (TRAIN_LEFT_OUT): DPTN x saturated, for both training forms -- the two (form, regime) pairs the grid may
# drop.  No input meets the precondition there: gates at their rail put hundreds of |h| near 1e-12 at every seed, and the
# smallest |tanh(c)| is no better (i and f both at the low rail leave c = f c + i g near zero); measured on 17 sequences of 33
# positions, seeds 0..3: smallest |h| 2.4e-13 .. 9.1e-11, 659 .. 894 values below 4e-7 (tests/test_recurrence_host.py asserts
# that no seed below TRAIN_SEED_LIMIT meets it).  The saturated BPTT, where the gate derivatives i - i i cancel, is judged
# on DPRNN, which has no ReLU.
TRAIN_ARCHS = (("dptn", 128), ("dptn", 64), ("dprnn", 64))
TRAIN_NSEQ = (5, 16, 17, 33)
TRAIN_LENGTHS = (2, 33)
TRAIN_FORMS = {"16": 1, "32": 0}      # the inference form of the same tile height (FORMS) -> option lstm16 of the training step
RNN_LEAVES = tuple(f"rnn.{leaf}_l0{sfx}" for sfx in ("", "_reverse") for leaf in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
TRAIN_INFERENCE_DB = 120.0
TRAIN_SEED_LIMIT = 32
TRAIN_LEFT_OUT = (("16", "saturated"), ("32", "saturated"))      # DPTN only; (training form, regime)


def train_regimes(arch: str) -> Tuple[str, ...]:
    return ("plain", "saturated", "open") + (("loud",) if arch == "dprnn" else ())


def _train_grid() -> List[Case]:
    """plain at every sequence count, both lengths, both paths; the other regimes at 17 sequences; 150 positions once per
    architecture (17 sequences, the strided path)."""
    out = []
    for arch, f in TRAIN_ARCHS:
        for path in (0, 1):
            for ln in TRAIN_LENGTHS:
                out += [Case(arch, f, path, nseq, ln) for nseq in TRAIN_NSEQ]
                out += [Case(arch, f, path, VALUE_NSEQ, ln, regime) for regime in train_regimes(arch)[1:]
                        if not (arch == "dptn" and all((form, regime) in TRAIN_LEFT_OUT for form in TRAIN_FORMS))]
        out.append(Case(arch, f, 1, VALUE_NSEQ, LONG))
    return out


TRAIN_CASES = _train_grid()

# tuple(case) -> input seed of the DPTN training cases whose first seed, 0, missed the ReLU precondition in fp64: the first of
# 1, 2, ... that meets it (python -m tests.recurrence_cases --search prints this table)
TRAIN_SEED_OVERRIDES: Dict[tuple, int] = {
    ("dptn", 128, 0, 33, 2, "plain", 1, True): 1, ("dptn", 128, 0, 16, 33, "plain", 1, True): 1,
    ("dptn", 128, 1, 16, 33, "plain", 1, True): 1, ("dptn", 128, 1, 17, 150, "plain", 1, True): 1,
    ("dptn", 64, 0, 5, 2, "plain", 1, True): 1, ("dptn", 64, 0, 33, 33, "plain", 1, True): 1,
    ("dptn", 64, 1, 16, 33, "plain", 1, True): 1, ("dptn", 64, 1, 33, 33, "plain", 1, True): 1,
    ("dptn", 64, 1, 17, 33, "open", 1, True): 1, ("dptn", 64, 1, 17, 150, "plain", 1, True): 17,
}


def train_seed(case: Case) -> int:
    return TRAIN_SEED_OVERRIDES.get(tuple(case), 0)


def train_inputs(case: Case, seed: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(x, dy) fp32 [B, S, K, N], read-only: x as the inference cases make it (the regime applied), dy standard normal."""
    seed = train_seed(case) if seed is None else seed
    dy = np.random.default_rng([7, case.path, case.nseq, case.len, case.features, seed]).standard_normal(shape(case)).astype(np.float32)
    dy.setflags(write=False)
    return inputs(case, seed), dy


def train_formula(case: Case, x: np.ndarray, dy: np.ndarray, dtype=torch.float64) -> Dict[str, object]:
    """One half of a block, forward and backward, under torch.autograd on the CPU.
    -> {"y", "dx": [tokens, N], "grads": {rnn leaf: numpy}, "y1": the LSTM's input [R, len, N] (DPTN; else None),
        "min_relu": smallest |h| that meets the ReLU (DPTN; else inf)}."""
    import torch.nn.functional as F
    B, S, K, N = shape(case)
    sd, pre = weights(case), prefix(case)
    P = {k[len(pre):]: torch.from_numpy(np.array(v)).to(dtype).requires_grad_(True) for k, v in sd.items() if k.startswith(pre)}
    rnn = torch.nn.LSTM(N, H, bidirectional=True, batch_first=True).to(dtype)
    rnn.load_state_dict({k[4:]: v.detach() for k, v in P.items() if k.startswith("rnn.")})
    seqs = _to_seqs(torch.from_numpy(np.array(x)).to(dtype), case.path).clone().requires_grad_(True)
    y1 = None
    with torch.enable_grad():
        if case.arch == "dptn":
            R_, Ls, heads, dh = seqs.shape[0], seqs.shape[1], 4, N // 4
            qkv = F.linear(seqs, P["mha.in_proj_weight"], P["mha.in_proj_bias"])
            q, k, v = (t.reshape(R_, Ls, heads, dh).transpose(1, 2) for t in qkv.split(N, -1))
            att = (torch.softmax(q @ k.transpose(-1, -2) / dh ** 0.5, -1) @ v).transpose(1, 2).reshape(R_, Ls, N)
            y1 = F.layer_norm(F.linear(att, P["mha.out_proj.weight"], P["mha.out_proj.bias"]) + seqs, (N,), P["ln1.weight"], P["ln1.bias"])
            h = rnn(y1)[0]
            out = F.layer_norm(F.linear(F.relu(h), P["ffn.1.weight"], P["ffn.1.bias"]) + y1, (N,), P["ln2.weight"], P["ln2.bias"])
            min_relu = float(h.detach().abs().min())
        else:
            h = rnn(seqs)[0]
            out = F.layer_norm(F.linear(h, P["fc.weight"], P["fc.bias"]), (N,), P["norm1d.weight"], P["norm1d.bias"]) + seqs
            min_relu = float("inf")
        out.backward(_to_seqs(torch.from_numpy(np.array(dy)).to(dtype), case.path))
    grads = {"rnn." + k: np.array(p.grad.numpy()) for k, p in rnn.named_parameters()}
    assert tuple(sorted(grads)) == tuple(sorted(RNN_LEAVES))
    res = {"y": np.array(_to_tokens(out.detach(), case.path, B, S, K)), "dx": np.array(_to_tokens(seqs.grad, case.path, B, S, K)),
           "grads": grads, "min_relu": min_relu, "y1": None if y1 is None else y1.detach()}
    for a in (res["y"], res["dx"], *grads.values()):
        a.setflags(write=False)
    return res


def relu_margin(case: Case, r64: Dict[str, object]) -> float:
    """The smallest |h| that meets the ReLU in fp64; inf for DPRNN, which has no ReLU."""
    return r64["min_relu"] if case.arch == "dptn" else float("inf")


def saturated_relu_inputs(features: int, path: int, seed: int, ln: int = 33) -> Tuple[float, float, int]:
    """(smallest |h|, smallest |tanh(c)|, values of |h| below MIN_RELU_INPUT) of the left-out DPTN x saturated case at fp64."""
    from tests.train_attention_cases import MIN_RELU_INPUT
    case = Case("dptn", features, path, VALUE_NSEQ, ln, "saturated")
    y1, W = train_formula(case, *train_inputs(case, seed))["y1"], _rnn_weights(case)
    hc = [lstm_direction(y1, W[d], d == 1, cells=True) for d in range(2)]
    h, c = torch.cat([a for a, _ in hc], -1), torch.cat([b for _, b in hc], -1)
    return float(h.abs().min()), float(torch.tanh(c).abs().min()), int((h.abs() < MIN_RELU_INPUT).sum())


@functools.lru_cache(maxsize=None)
def train_reference(case: Case, bits: int = 64) -> Dict[str, object]:
    x, dy = train_inputs(case)
    return train_formula(case, x, dy, torch.float64 if bits == 64 else torch.float32)


def param_db(got: np.ndarray, ref: np.ndarray) -> float:
    from oracle.dptn_oracle import agreement_db
    return agreement_db(got, ref)


@functools.lru_cache(maxsize=None)
def train_restatement(case: Case) -> Dict[str, float]:
    """{"y", "dx": worst token, each rnn leaf: whole tensor} of fp32 autograd against fp64 autograd, dB."""
    r64, r32 = train_reference(case, 64), train_reference(case, 32)
    out = {k: figures(r32[k], r64[k])[1] for k in ("y", "dx")}
    out.update({leaf: param_db(r32["grads"][leaf], r64["grads"][leaf]) for leaf in RNN_LEAVES})
    return out


def train_floors(case: Case) -> Dict[str, float]:
    """{"y", "dx", each rnn leaf} -> the floor the kernels must meet."""
    from tests.train_attention_cases import PARAM_FLOOR_DB, TOKEN_FLOOR_DB
    return {k: min(TOKEN_FLOOR_DB if k in ("y", "dx") else PARAM_FLOOR_DB, v - MARGIN_DB) for k, v in train_restatement(case).items()}


def check_train_preconditions(case: Case) -> Dict[str, float]:
    from tests.train_attention_cases import MIN_RELU_INPUT
    stage_geometry(case)
    r64 = train_reference(case, 64)
    margin = relu_margin(case, r64)
    assert margin >= MIN_RELU_INPUT, (case.id, "ReLU precondition in fp64", margin)
    assert all(np.isfinite(a).all() for a in (r64["y"], r64["dx"], *r64["grads"].values())), case.id
    fl = train_floors(case)
    assert all(np.isfinite(v) for v in fl.values()), (case.id, fl)
    return {"relu_margin": margin, **{"floor." + k: v for k, v in fl.items()}}


def _search():      # python -m tests.recurrence_cases --search: the table above
    for case in CASES:
        seed, missed = 0, None
        while True:
            try:
                check_preconditions(case, host_lstm_input(case, seed))
                break
            except AssertionError as e:
                missed = missed or e.args[0][1:]
                seed += 1
                assert seed < 32, (case.id, "no seed meets the preconditions", missed)
        if seed:
            print(f"    {tuple(case)}: {seed},      # seed 0: {missed}", flush=True)
    from tests.train_attention_cases import MIN_RELU_INPUT
    print("TRAIN_SEED_OVERRIDES")
    for case in (c for c in TRAIN_CASES if c.arch == "dptn"):
        seed = 0
        while relu_margin(case, train_formula(case, *train_inputs(case, seed))) < MIN_RELU_INPUT:
            seed += 1
            assert seed < TRAIN_SEED_LIMIT, (case.id, "no seed meets the ReLU precondition")
        if seed:
            print(f"    {tuple(case)}: {seed},", flush=True)


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        _search()
