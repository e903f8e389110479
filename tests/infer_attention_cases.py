"""TEST INFRASTRUCTURE: the cases of the inference-attention tests and their CPU references, computed once per process and
shared, read-only, by tests/test_infer_attention_host.py and tests/test_gpu_infer_attention.py.

The inference forward runs the attention half of a TransformerDPRNN through five kernel families (instantiations() below):

  attn_block2_kernel<NKB, PRO, PERSIST>   128 features, len <= 160, the default       NKB 1..5 x {plain, pro, persist}
  attn_block_kernel<NKB, PRO>             128 features, option attn_v2 = 0            NKB 1..5 x {plain, pro}
  attn_block64_kernel<NB, PRO>            64 features, len <= 160                     NB = ceil(len / 16) = 1..10 x {plain, pro}
  attention_kernel<DH, NKB> + K1 / K3     option fuse_attn = 0, or 160 < len <= 256   DH 32 / 16 x NKB 1..8
  attention_long_kernel<DH>               len > 256 (inter-chunk path only)           DH 32 / 16

Two kinds of case, all with hidden_dim 128, 4 heads, both LSTM directions, weights synthetic_state_dict(cfg, WEIGHT_SEED):

STAGE cases (features, path, len) go through dptnav_stage_path: one engine runs every form that applies (forms()).
  path 1    inter-chunk, tokens strided: chunk_size 3, step_size 1, B = 1, S = len -> 3 sequences; FUSED + MID + LONG
  path 0    intra-chunk, tokens contiguous: chunk_size = len, step = max(len // 2, 1), B = 1, S = 3; PATH0_LENGTHS
  x         standard normal [B, S, K, N], seed 1000 * path + len
  judged    y1 = LN1(MHA(x) + x) (the "y1" workspace tap), att (the "att" tap, unfused forms only), y (the path output)
  reference the explicit formula of one half (half()) at fp64 (the truth) and fp32 (the restatement)

PRO cases (features, kind, len) go through dptnav_forward with B = 1 and synthetic_inputs waveforms: the forms whose attention
block computes the previous path's FFN half as its prologue exist only there.
  inter     one block, chunk_size 3, step_size 1, S = len: the inter-chunk block carries the prologue
  intra     two blocks, chunk_size = len, step = max(len // 2, 1), S = 3: block 1's intra-chunk block carries it
  T         the largest number of samples that gives S chunks (samples_for_chunks)
  judged    the "y1" tap after the forward: LN1 of the LAST inter-chunk path (nothing behind it writes y1: the tail aliases
            qkv and att only; at B = 1 the forward runs the one unsliced plan that dptnav_workspace_tap reports)
  reference oracle.dptn_oracle.forward with taps at fp64 / fp32, y1 of the last path from the blk*_intra tap by half()

The figure is train_attention_cases.figures / token_db: the reference's overall power over ONE token's error.

Preconditions (conditions on the INPUTS, asserted on the CPU before any kernel result is looked at):
  * the fp32 restatement reaches STAGE_RESTATEMENT_DB on every token of y1, ATT_RESTATEMENT_DB on every token of att,
    Y_RESTATEMENT_DB on every token of y, PRO_RESTATEMENT_DB on every token of the final y1 of a PRO chain (pro_seed:
    PRO_SEED_OVERRIDES).  att has a bar of its own because fp32 cannot reach 130 dB there: an element of att is a
    softmax-weighted mean of V rows, which cancels most of their magnitude while keeping the rounding of every term, and
    every fp32 evaluation tried (explicit exp, torch.softmax, scaled_dot_product_attention, normalising after P V) lands
    at 130 .. 131.5 dB over the WHOLE att tensor and 126.5 .. 130 dB on its worst token from 17 positions on; only fp64
    inside the attention lifts it.  120 dB keeps the restatement 20 dB clear of the 100 dB floor, the distance the grid
    keeps between its floors and the defect ceiling.  The floor the kernels must meet on att is the same 100 dB as for y1;
  * len >= 2: the fp64 formula with either DEFECT at (last sequence, last head, last query) of the attention under test has
    the worst token of the judged y1 at or below DEFECT_CEILING_DB -- the floors then see one wrong key in one query row
    with 20 dB (stage) or 10 dB (PRO) to spare;
  * the launch geometry: samples -> frames -> chunks, the (B, T, Tv) handed to the tap and the floats read from it.
"""
from __future__ import annotations

import functools
from typing import Dict, List, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTN_AUDIO, DPTN_AV, DPTNConfig, synthetic_inputs, synthetic_state_dict
from tests.train_attention_cases import WEIGHT_SEED, config as stage_config, figures, weights as stage_weights

FEATURES = (128, 64)
FUSED_MAX = 160                # ATTN_BLOCK_MAX_LEN
FUSED = sorted({2, 141, 150} | {v for n in range(1, 11) for v in (16 * (n - 1) + 1, 16 * n - 1, 16 * n)})
MID = sorted({v for n in (6, 7, 8) for v in (32 * (n - 1) + 1, 32 * n - 1, 32 * n)})
LONG = [257, 287, 288, 289, 320, 384, 385]
PATH1_LENGTHS = FUSED + MID + LONG
PATH0_LENGTHS = sorted({v for n in range(1, 11) for v in (16 * (n - 1) + 1, 16 * n)} | {150} | {161, 192, 193, 224, 225, 256})
PRO_LENGTHS = {128: [1, 2, 32, 33, 64, 65, 96, 97, 128, 129, 141, 150, 159, 160],
               64: sorted({v for n in range(1, 11) for v in (16 * (n - 1) + 1, 16 * n)} | {2, 150})}
PRO_TV = 50

DEFECTS = ("key0_twice", "last_key_dropped")   # a padded key read unmasked / a length mask off by one
STAGE_FLOOR_DB = 100.0         # y1 and att through stage_path, every token: "the same sums in another order"
STAGE_RESTATEMENT_DB = 130.0    # y1 (measured: 135.2 or better)
ATT_RESTATEMENT_DB = 120.0      # att (measured: 126.5 or better; see the header)
Y_FLOOR_DB = 80.0              # y through stage_path, every token (TOKEN_FLOOR_DB of the training grid)
Y_RESTATEMENT_DB = 90.0
PRO_FLOOR_DB = 90.0            # the final y1 of a PRO chain, every token
PRO_RESTATEMENT_DB = 100.0
DEFECT_CEILING_DB = 80.0
OLD_FLOOR_DB = 80.0            # agreement_db > 80 over whole tensors: what guarded these kernels before


class Case(NamedTuple):
    features: int
    path: int
    len: int

    @property
    def id(self) -> str:
        return f"n{self.features}-path{self.path}-len{self.len}"


class ProCase(NamedTuple):
    features: int
    kind: str       # "inter" / "intra": which path's attention block carries the prologue under test
    len: int

    @property
    def id(self) -> str:
        return f"n{self.features}-pro-{self.kind}-len{self.len}"

    @property
    def path(self) -> int:
        return 1 if self.kind == "inter" else 0


CASES = [Case(f, p, ln) for f in FEATURES for p, lengths in ((1, PATH1_LENGTHS), (0, PATH0_LENGTHS)) for ln in lengths]
PRO_CASES = [ProCase(f, kind, ln) for f in FEATURES for kind in ("inter", "intra") for ln in PRO_LENGTHS[f]]
LEFT_OUT: List[ProCase] = []   # PRO cases without a sample count the head accepts (none: test_launch_geometry checks every case)

# (features, kind, len) -> input seed of the PRO cases whose first seed, 7000 + len, missed PRO_RESTATEMENT_DB:
# the first of seed + 10000, seed + 20000, ... that reaches it (python -m tests.infer_attention_cases --search prints this table)
PRO_SEED_OVERRIDES: Dict[Tuple[int, str, int], int] = {
}


# ---------------------------------------------------------------------------------------------------------------------
# which template a form of a case runs
# ---------------------------------------------------------------------------------------------------------------------
def _edge(ln: int, block: int) -> str:
    """'one': one key in the last block of `block` keys, 'full': all of them, '': neither."""
    return "one" if (ln - 1) % block == 0 else "full" if ln % block == 0 else ""


def forms(case: Case) -> Dict[str, Dict[str, int]]:
    """form -> the options that select it (set on top of the defaults, which every form starts from)."""
    if case.len > FUSED_MAX:
        return {"auto": {}, "unfused": {"fuse_attn": 0}}
    if case.features == 128:
        return {"v2": {}, "v1": {"attn_v2": 0}, "unfused": {"fuse_attn": 0}}
    return {"fused64": {}, "unfused": {"fuse_attn": 0}}


def pro_forms(case: ProCase) -> Dict[str, Dict[str, int]]:
    if case.features == 128:
        return {"v2": {"attn_persist": 0}, "persist": {"attn_persist": 3}, "v1": {"attn_v2": 0}}
    return {"fused64": {}}


def instantiation(features: int, form: str, ln: int, pro: bool = False) -> Tuple:
    """(family, DH or '', NKB / NB or '', 'plain' / 'pro' / 'persist' or '') of the kernel the form runs at this length."""
    if form in ("v2", "persist"):
        return ("attn_block2", "", (ln + 31) // 32, "persist" if form == "persist" else "pro" if pro else "plain")
    if form == "v1":
        return ("attn_block", "", (ln + 31) // 32, "pro" if pro else "plain")
    if form == "fused64":
        return ("attn_block64", "", (ln + 15) // 16, "pro" if pro else "plain")
    assert form in ("unfused", "auto") and not pro
    if ln > 256:
        return ("attention_long", features // 4, "", "")
    return ("attention", features // 4, (ln + 31) // 32, "")


def coverage_key(features: int, form: str, ln: int, path: int, pro: bool = False) -> Optional[Tuple]:
    """instantiation + (path, edge), None where the length is neither edge of its last key block."""
    inst = instantiation(features, form, ln, pro)
    edge = _edge(ln, 16 if inst[0] == "attn_block64" else 32)
    return inst + (path, edge) if edge else None


def instantiations() -> set:
    """Every (instantiation, path, edge) the table in the header names."""
    want = set()
    for path in (0, 1):
        for edge in ("one", "full"):
            for nkb in range(1, 6):
                want |= {("attn_block2", "", nkb, f, path, edge) for f in ("plain", "pro", "persist")}
                want |= {("attn_block", "", nkb, f, path, edge) for f in ("plain", "pro")}
            want |= {("attn_block64", "", nb, f, path, edge) for nb in range(1, 11) for f in ("plain", "pro")}
            want |= {("attention", dh, nkb, "", path, edge) for dh in (32, 16) for nkb in range(1, 9)}
    want |= {("attention_long", dh, "", "", 1, edge) for dh in (32, 16) for edge in ("one", "full")}
    return want


def grid_coverage() -> set:
    """The (instantiation, path, edge) keys the grid runs."""
    have = set()
    for c in CASES:
        for form in forms(c):
            have.add(coverage_key(c.features, form, c.len, c.path))
    for c in PRO_CASES:
        if c in LEFT_OUT:
            continue
        for form in pro_forms(c):
            have.add(coverage_key(c.features, form, c.len, c.path, pro=True))
    have.discard(None)
    return have


# ---------------------------------------------------------------------------------------------------------------------
# the formula of one TransformerDPRNN half
# ---------------------------------------------------------------------------------------------------------------------
def _params(sd: Dict[str, np.ndarray], pre: str, dtype) -> Dict[str, torch.Tensor]:
    return {k[len(pre):]: torch.from_numpy(np.array(v)).to(dtype) for k, v in sd.items() if k.startswith(pre)}


def half(seqs, P: Dict[str, torch.Tensor], heads: int = 4, defect: Optional[str] = None, upto: str = "y") -> Dict[str, torch.Tensor]:
    """seqs [R, len, N] (torch, the dtype the formula runs in) -> {"att", "y1", "y"} in the same layout ("y" only with
    upto == "y").  defect: key 0 counted twice / the last key left out of the softmax of (last sequence, last head, last query)."""
    R, Ls, N = seqs.shape
    dh = N // heads
    with torch.no_grad():
        qkv = F.linear(seqs, P["mha.in_proj_weight"], P["mha.in_proj_bias"])
        q, k, v = (t.reshape(R, Ls, heads, dh).transpose(1, 2) for t in qkv.split(N, -1))
        s = q @ k.transpose(-1, -2) / dh ** 0.5
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        if defect == "key0_twice":
            e[-1, -1, -1, 0] *= 2
        elif defect == "last_key_dropped":
            assert Ls >= 2
            e[-1, -1, -1, -1] = 0
        else:
            assert defect is None
        prob = e / e.sum(-1, keepdim=True)
        att = (prob @ v).transpose(1, 2).reshape(R, Ls, N)
        y1 = F.layer_norm(F.linear(att, P["mha.out_proj.weight"], P["mha.out_proj.bias"]) + seqs, (N,), P["ln1.weight"], P["ln1.bias"])
        out = {"att": att, "y1": y1}
        if upto == "y":
            H = P["rnn.weight_hh_l0"].shape[1]
            rnn = torch.nn.LSTM(N, H, bidirectional=True, batch_first=True).to(seqs.dtype)
            rnn.load_state_dict({k[4:]: t for k, t in P.items() if k.startswith("rnn.")})
            z = F.linear(F.relu(rnn(y1)[0]), P["ffn.1.weight"], P["ffn.1.bias"]) + y1
            out["y"] = F.layer_norm(z, (N,), P["ln2.weight"], P["ln2.bias"])
    return out


def _to_seqs(a: torch.Tensor, path: int) -> torch.Tensor:
    """[B, S, K, N] -> the path's sequences [R, len, N]."""
    B, S, K, N = a.shape
    return a.reshape(B * S, K, N) if path == 0 else a.transpose(1, 2).reshape(B * K, S, N)


def _to_tokens(a: torch.Tensor, path: int, B: int, S: int, K: int) -> np.ndarray:
    """The path's sequences [R, len, N] -> [tokens = B * S * K, N], token (b, s, k) (the layout of the workspace taps); read-only."""
    N = a.shape[-1]
    a = a.reshape(B, S, K, N) if path == 0 else a.reshape(B, K, S, N).transpose(1, 2)
    out = a.contiguous().reshape(B * S * K, N).numpy()
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# stage cases
# ---------------------------------------------------------------------------------------------------------------------
def shape(case: Case) -> Tuple[int, int, int, int]:
    """(B, S, K, N) of x."""
    return (1, case.len, 3, case.features) if case.path == 1 else (1, 3, case.len, case.features)


def config(case: Case) -> DPTNConfig:
    return stage_config(case.features, case.path, case.len)


def weights(case: Case) -> Dict[str, np.ndarray]:
    return stage_weights(case.features, case.path, case.len)


def prefix(path: int, block: int = 0) -> str:
    return "dprnn.model.%d.%s." % (block, "intra_chunk_block" if path == 0 else "inter_chunk_block")


@functools.lru_cache(maxsize=None)
def inputs(case: Case) -> np.ndarray:
    """x fp32 [B, S, K, N], read-only."""
    x = np.random.default_rng(1000 * case.path + case.len).standard_normal(shape(case)).astype(np.float32)
    x.setflags(write=False)
    return x


def stage_geometry(case: Case) -> Dict[str, int]:
    """What the GPU test hands to the library for this case, restated on the host: T as DptnEngine._path_T derives it,
    the chunk count that T gives back, M tokens and the floats of the y1 / att taps."""
    cfg = config(case)
    B, S, K, N = shape(case)
    L = (S - 1) * cfg.step_size + cfg.chunk_size
    T = (L - 1) * cfg.stride_enc + cfg.kernel_size_enc
    assert cfg.chunk_size == K and cfg.chunk_size <= 256 and cfg.frames(T) == L and cfg.chunks(L) == S, case.id
    return {"B": B, "S": S, "K": K, "N": N, "T": T, "Tv": 1, "M": B * S * K, "tap_floats": B * S * K * N}


@functools.lru_cache(maxsize=None)
def reference(case: Case, bits: int = 64, defect: Optional[str] = None) -> Dict[str, np.ndarray]:
    """{"att", "y1", "y"} as [tokens, N] of the formula at fp64 / fp32; with a defect: {"att", "y1"} only."""
    dtype = torch.float64 if bits == 64 else torch.float32
    B, S, K, N = shape(case)
    P = _params(weights(case), prefix(case.path), dtype)
    seqs = _to_seqs(torch.from_numpy(np.array(inputs(case))).to(dtype), case.path)
    r = half(seqs, P, defect=defect, upto="y1" if defect else "y")
    return {k: _to_tokens(v, case.path, B, S, K) for k, v in r.items()}


def check_preconditions(case: Case) -> Dict[str, float]:
    """Asserts the preconditions of a stage case; -> the measured figures."""
    stage_geometry(case)
    r64, r32 = reference(case, 64), reference(case, 32)
    out = {}
    for key, floor in (("y1", STAGE_RESTATEMENT_DB), ("att", ATT_RESTATEMENT_DB), ("y", Y_RESTATEMENT_DB)):
        whole, worst, tok = figures(r32[key], r64[key])
        out[f"restatement.{key}"], out[f"restatement.{key}.token"] = whole, worst
        assert worst >= floor, (case.id, key, "fp32 restatement, worst token", worst, tok)
    if case.len >= 2:
        for d in DEFECTS:
            whole, worst, tok = figures(reference(case, 64, d)["y1"], r64["y1"])
            out[f"{d}.y1"], out[f"{d}.y1.token"] = whole, worst
            assert worst <= DEFECT_CEILING_DB, (case.id, d, "worst token of y1", worst, tok)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# PRO cases
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pro_config(case: ProCase) -> DPTNConfig:
    base = DPTN_AV if case.features == 128 else DPTN_AUDIO
    blocks, chunk, step = (1, 3, 1) if case.kind == "inter" else (2, case.len, max(case.len // 2, 1))
    return DPTNConfig(**{**base.to_dict(), "num_blocks": blocks, "chunk_size": chunk, "step_size": step, "hidden_dim": 128,
                         "num_heads": 4, "bidir": True})


@functools.lru_cache(maxsize=None)
def pro_weights(case: ProCase) -> Dict[str, np.ndarray]:
    sd = synthetic_state_dict(pro_config(case), seed=WEIGHT_SEED)
    for v in sd.values():
        v.setflags(write=False)
    return sd


def samples_for_chunks(cfg: DPTNConfig, S: int) -> int:
    """The largest T that gives S chunks: the last frame count before chunk S + 1 starts, the last sample before the next frame."""
    L = cfg.ola_len(S) + cfg.step_size - 1
    return (L - 1) * cfg.stride_enc + cfg.kernel_size_enc + cfg.stride_enc - 1


def pro_geometry(case: ProCase) -> Dict[str, int]:
    """The launch geometry of a PRO case, checked on the host: samples -> frames -> chunks, the (B, T, Tv) of the forward and of
    the tap, the tokens and the floats read from the tap (the plan's y1 holds exactly M * N)."""
    cfg = pro_config(case)
    S, K = (case.len, 3) if case.kind == "inter" else (3, case.len)
    T = samples_for_chunks(cfg, S)
    L = cfg.frames(T)
    assert T >= cfg.kernel_size_enc and cfg.chunk_size == K <= 256, case.id
    assert cfg.chunks(L) == S and cfg.chunks(cfg.frames(T + 1)) == S + 1, (case.id, T, L)
    assert cfg.ola_len(S) <= L < cfg.ola_len(S) + cfg.step_size, (case.id, L)       # frames = (S - 1) step + chunk, + < one step
    assert (S if case.kind == "inter" else K) == case.len <= FUSED_MAX                # the sequence length under test
    M = S * K
    assert 2 * M * max(3 * cfg.num_features, 2 * cfg.hidden_dim) < 2 ** 31          # make_plan's 32-bit token indexing bound
    return {"B": 1, "S": S, "K": K, "N": cfg.num_features, "T": T, "Tv": 1 if cfg.audio_only else PRO_TV, "L": L, "M": M,
            "tap_floats": M * cfg.num_features, "blocks": cfg.num_blocks}


def pro_seed(case: ProCase) -> int:
    return PRO_SEED_OVERRIDES.get(tuple(case), 7000 + case.len)


def pro_inputs_for_seed(case: ProCase, seed: int) -> Dict[str, np.ndarray]:
    g = pro_geometry(case)
    inp = synthetic_inputs(pro_config(case), B=1, T=g["T"], Tv=g["Tv"], seed=seed)
    return {k: v for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")}


@functools.lru_cache(maxsize=None)
def pro_inputs(case: ProCase) -> Dict[str, np.ndarray]:
    inp = pro_inputs_for_seed(case, pro_seed(case))
    for v in inp.values():
        v.setflags(write=False)
    return inp


def _last_y1(case: ProCase, intra_tap: np.ndarray, dtype) -> np.ndarray:
    """y1 of the last inter-chunk path from the oracle's blk*_intra tap ((B S, K, N), the intra-chunk path's output)."""
    g = pro_geometry(case)
    B, S, K, N = 1, g["S"], g["K"], g["N"]
    P = _params(pro_weights(case), prefix(1, g["blocks"] - 1), dtype)
    seqs = _to_seqs(torch.from_numpy(np.ascontiguousarray(intra_tap)).to(dtype).reshape(B, S, K, N), 1)
    return _to_tokens(half(seqs, P, upto="y1")["y1"], 1, B, S, K)


def _pro_chain(case: ProCase, inp: Dict[str, np.ndarray], bits: int):
    g = pro_geometry(case)
    taps: dict = {}
    O.forward(pro_config(case), pro_weights(case), dtype=np.float64 if bits == 64 else np.float32, taps=taps, **inp)
    y1 = _last_y1(case, taps[f"blk{g['blocks'] - 1}_intra"], torch.float64 if bits == 64 else torch.float32)
    return y1, taps


@functools.lru_cache(maxsize=None)
def pro_reference(case: ProCase, bits: int = 64) -> np.ndarray:
    """The final y1 [tokens, N] of the whole forward at fp64 / fp32; read-only."""
    return _pro_chain(case, pro_inputs(case), bits)[0]


@functools.lru_cache(maxsize=None)
def _pro_taps64(case: ProCase) -> dict:
    return _pro_chain(case, pro_inputs(case), 64)[1]


@functools.lru_cache(maxsize=None)
def pro_defective(case: ProCase, defect: Optional[str]) -> np.ndarray:
    """The final y1 at fp64 with the defect in the attention under test, recomputed from the fp64 input tap of that path onward
    (defect None: the same recomputation without one, which must reproduce pro_reference)."""
    g = pro_geometry(case)
    B, S, K, N = 1, g["S"], g["K"], g["N"]
    taps, sd, dt = _pro_taps64(case), pro_weights(case), torch.float64
    if case.kind == "inter":      # the last path itself: its input is the intra-chunk output of the only block
        seqs = _to_seqs(torch.from_numpy(np.ascontiguousarray(taps["blk0_intra"])).reshape(B, S, K, N), 1)
        return _to_tokens(half(seqs, _params(sd, prefix(1, 0), dt), defect=defect, upto="y1")["y1"], 1, B, S, K)
    x = torch.from_numpy(np.ascontiguousarray(taps["blk0_out"].transpose(0, 2, 3, 1)))       # (B, N, S, K) -> (B, S, K, N)
    intra = half(_to_seqs(x, 0), _params(sd, prefix(0, 1), dt), defect=defect)["y"].reshape(B, S, K, N)
    return _to_tokens(half(_to_seqs(intra, 1), _params(sd, prefix(1, 1), dt), upto="y1")["y1"], 1, B, S, K)


def pro_restatement(case: ProCase, seed: Optional[int] = None) -> Tuple[float, float, int]:
    """figures() of the fp32 chain against the fp64 chain (for another input seed: uncached, the seed search)."""
    if seed is None:
        return figures(pro_reference(case, 32), pro_reference(case, 64))
    inp = pro_inputs_for_seed(case, seed)
    return figures(_pro_chain(case, inp, 32)[0], _pro_chain(case, inp, 64)[0])


def check_pro_preconditions(case: ProCase) -> Dict[str, float]:
    pro_geometry(case)
    r64 = pro_reference(case, 64)
    whole, worst, tok = pro_restatement(case)
    out = {"restatement.y1": whole, "restatement.y1.token": worst}
    assert worst >= PRO_RESTATEMENT_DB, (case.id, "fp32 restatement of the chain, worst token", worst, tok)
    whole, worst, tok = figures(pro_defective(case, None), r64)      # half() against the oracle's own formulas, fp64
    out["recomputed.y1.token"] = worst
    assert worst >= 200.0, (case.id, "the recomputation from the tap does not reproduce the oracle", worst, tok)
    if case.len >= 2:
        for d in DEFECTS:
            whole, worst, tok = figures(pro_defective(case, d), r64)
            out[f"{d}.y1"], out[f"{d}.y1.token"] = whole, worst
            assert worst <= DEFECT_CEILING_DB, (case.id, d, "worst token of the final y1", worst, tok)
    return out


# ---------------------------------------------------------------------------------------------------------------------
# judging (the GPU test's assertions; the host test runs defective formulas through the same code)
# ---------------------------------------------------------------------------------------------------------------------
def judge(what: str, got: np.ndarray, ref: np.ndarray, floor: float) -> Tuple[float, float, int]:
    """Finite, the reference's shape, every token at `floor` dB or better -> figures(); AssertionError otherwise."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), (what, "not finite")
    whole, worst, tok = figures(got, ref)
    assert worst >= floor, (what, "worst token", round(worst, 1), "dB at token", tok, "floor", floor, "whole tensor", round(whole, 1))
    return whole, worst, tok


def _search():      # python -m tests.infer_attention_cases --search: the table above
    for case in PRO_CASES:
        seed = 7000 + case.len
        while pro_restatement(case, seed)[1] < PRO_RESTATEMENT_DB:
            seed += 10000
        if seed != 7000 + case.len:
            print(f"    {tuple(case)}: {seed},", flush=True)


if __name__ == "__main__":
    import sys
    if "--search" in sys.argv:
        _search()
