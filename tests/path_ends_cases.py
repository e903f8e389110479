"""TEST INFRASTRUCTURE (not product code): the case table, input builders, restatements and judges of the path-ends tests
(tests/test_path_ends_host.py on the CPU, tests/test_gpu_path_ends.py on the MI355X).  No GPU is needed to import it.

The ends of the DPTN / DPRNN path are the head (video_linear_kernel, encoder_fuse_kernel), the tail (separation conv,
ALoadOla / EpiSkipDecoderTaps or fold_decoder_kernel + taps_fold_kernel, mask_tail.hip, decoder_gather_kernel) and their
backward (backward_ends.h).  A case fixes the geometry exactly:

    L = (S - 1) P + K + r_L,  r_L in {0, P - 1}      trailing frames that no chunk holds (left >= 0, padded rows exist)
    T = (L - 1) stride + kenc + r_T,  r_T in {0, stride - 1}      pad_left and the zero tail of the waveform

(K, P) covers both staging forms of taps_fold_kernel / mask_tail.hip: K > 2P (the generic chunk loop: (20, 5), the odd
(21, 10), (9, 2), (5, 1)), K = 2P, K/2 < P < K (20, 13) and P = K (20, 20).  L crosses the kernels' own boundaries: L = K
(one chunk), 131 / 134 (past one encoder_fuse_kernel workgroup of 64 frames at 128 features, 128 at 64), 515 (past
encoder_wgrad_kernel's 512-frame slab), and 2 B L is no multiple of taps_fold_kernel's 32 rows at B = 3.  kernel_size_enc
takes every value 2..8 (7 on the reference's (150, 75)).  Video: video_emb_size 5 / 30 (no multiple of 4: the quartering of
Cv in video_linear_kernel), Tv 65 / 70 (second pass of its frame loop), Tv > L (the interpolation shrinks), Tv = 256 (the
limit of video_linear_bwd_kernel's LDS column).

Judges.  Values: per ROW (a frame of the latent, a token, a (speaker, item, frame) row of the tap table, a 16-sample
window of a waveform) the error norm over the RMS row norm of the WHOLE fp64 tensor (tests/hard_inputs.judge's
convention: near-zero and padded rows are judged on the signal's scale); the bound is 2 x the same figure of the fp32
restatement (the numpy oracle in fp32 against itself in fp64, written in the association the kernel uses).  Integer-valued
operands: exact equality (every partial sum of every contraction is an integer multiple of 0.25 below 2^22, so any
summation order gives the same fp32 bits: `exactness`)."""
from __future__ import annotations

import functools
from dataclasses import dataclass
from typing import Dict, List, Optional, Tuple

import numpy as np

from oracle import dptn_oracle as O
from speech_separation_amd.spec import DPTNConfig, synthetic_inputs, synthetic_state_dict
from tests import mask_tail_ref as MR

WINDOW = 16              # waveform samples per judged row
VALUE_FACTOR = 2.0       # a kernel's worst row <= 2 x the fp32 restatement's worst row
GATES = (0.7, -1.3, 0.0, 1e-4, 12.0)       # value tests
TRAIN_GATES = (0.7, -1.3, 0.0, 1e-4)       # gradient tests


@dataclass(frozen=True)
class Case:
    name: str
    arch: str                # "dptn" | "dprnn" | "dptn_mask"
    N: int
    K: int
    P: int
    kenc: int
    S: int
    rL: int                  # 0 or P - 1
    rT: int                  # 0 or stride - 1
    B: int
    Cv: int = 0              # > 0: audio-visual head
    Tv: int = 1

    def __post_init__(self):
        assert self.rL in (0, self.P - 1) and self.rT in (0, self.kenc // 2 - 1), self.name
        assert self.B in (1, 2, 3) and self.B * self.L <= 3 * 515, self.name
        assert (self.Cv == 0) or (self.N == 128 and self.arch == "dptn"), self.name

    @property
    def stride(self) -> int:
        return self.kenc // 2

    @property
    def L(self) -> int:
        return (self.S - 1) * self.P + self.K + self.rL

    @property
    def T(self) -> int:
        return (self.L - 1) * self.stride + self.kenc + self.rT

    @property
    def ola(self) -> int:
        return (self.S - 1) * self.P + self.K

    @property
    def left(self) -> int:
        return (self.L - self.ola) // 2

    @property
    def ndec(self) -> int:
        return (self.L - 1) * self.stride + self.kenc

    @property
    def pad_left(self) -> int:
        return (self.T - self.ndec) // 2

    @property
    def av(self) -> bool:
        return self.Cv > 0

    @property
    def masked(self) -> bool:
        return self.arch == "dptn_mask"

    def cfg(self, audio_only: Optional[bool] = None) -> DPTNConfig:
        ao = (not self.av) if audio_only is None else audio_only
        return DPTNConfig(num_features=self.N, video_emb_size=self.Cv or 512, hidden_video=self.N, kernel_size_enc=self.kenc,
                          hidden_dim=128, num_blocks=1, chunk_size=self.K, step_size=self.P, num_heads=4, dropout=0.0,
                          bidir=True, audio_only=ao, arch=self.arch)


def _c(*a, **kw) -> Case:
    return Case(*a, **kw)


# ---- stage-level cases: head and tail without a path in between (the arch only selects the tail)
STAGE_CASES: List[Case] = [
    #  name                 arch         N    K    P  kenc  S  rL rT  B
    _c("av128_k20p5_e2",    "dptn",     128,  20,   5, 2,   1,  0, 0, 3, Cv=512, Tv=50),     # L = K = 20 < Tv
    _c("av128_k21p10_e3",   "dptn",     128,  21,  10, 3,  12,  0, 0, 3, Cv=5, Tv=1),        # L = 131, 6 L = 18 mod 32
    _c("av128_k20p10_e5",   "dptn",     128,  20,  10, 5,   4,  9, 1, 2, Cv=30, Tv=2),       # L = 59
    _c("av128_k20p13_e6",   "dptn",     128,  20,  13, 6,   3, 12, 2, 1, Cv=512, Tv=65),     # L = 58 < Tv
    _c("av128_k20p20_e8",   "dptn",     128,  20,  20, 8,   3, 19, 3, 2, Cv=24, Tv=70),      # L = 79
    _c("av128_k150p75_e7",  "dptn",     128, 150,  75, 7,   2, 74, 2, 1, Cv=512, Tv=7),      # the reference geometry, L = 299
    _c("a128_k9p2_e4",      "dprnn",    128,   9,   2, 4,  62,  0, 1, 3),                    # L = 131
    _c("a128_k5p1_e7",      "dprnn",    128,   5,   1, 7,   8,  0, 2, 2),                    # L = 12
    _c("a64_k20p5_e3",      "dptn",      64,  20,   5, 3,  23,  4, 0, 3),                    # L = 134, 6 L = 4 mod 32
    _c("a64_k21p10_e8",     "dptn",      64,  21,  10, 8,  12,  0, 3, 3),                    # L = 131
    _c("a64_k20p10_e6",     "dptn",      64,  20,  10, 6,   1,  0, 2, 2),                    # L = K = 20
    _c("a64_k20p13_e2",     "dptn",      64,  20,  13, 2,   4, 12, 0, 1),                    # L = 71
    _c("a64_k20p20_e5",     "dptn",      64,  20,  20, 5,   2,  0, 0, 2),                    # L = 40, no padded row at all
    _c("a64_k9p2_e7",       "dprnn",     64,   9,   2, 7,   5,  1, 0, 3),                    # L = 18
    _c("a64_k5p1_e4",       "dprnn",     64,   5,   1, 4, 127,  0, 1, 1),                    # L = 131
    _c("m64_k20p5_e5",      "dptn_mask", 64,  20,   5, 5,  23,  4, 1, 3),                    # L = 134
    _c("m64_k21p10_e2",     "dptn_mask", 64,  21,  10, 2,   2,  9, 0, 2),                    # L = 40
    _c("m64_k20p13_e8",     "dptn_mask", 64,  20,  13, 8,   1, 12, 3, 1),                    # one chunk, L = 32
    _c("m64_k20p10_e7",     "dptn_mask", 64,  20,  10, 7,   3,  0, 2, 2),                    # L = 40
    _c("m128_k20p20_e3",    "dptn_mask", 128, 20,  20, 3,   3, 19, 0, 2),                    # L = 79
    _c("m128_k9p2_e6",      "dptn_mask", 128,  9,   2, 6,  62,  0, 2, 3),                    # L = 131
]

# ---- training cases: one-block models through train_forward / train_backward.  (S >= 2: a one-step inter-chunk recurrence
# is the recurrence suite's subject, not an end's; the ends' own S = 1 branches are in the stage cases.)
TRAIN_CASES: List[Case] = [
    _c("t_av128_k20p5_e2_L515", "dptn",     128, 20,  5, 2, 100,  0, 0, 3, Cv=30, Tv=2),     # L = 515: second encoder_wgrad slab
    _c("t_av128_k21p10_e5",     "dptn",     128, 21, 10, 5,   3,  9, 1, 2, Cv=24, Tv=70),    # L = 50 < Tv; the gate cases
    _c("t_av128_k20p13_e8",     "dptn",     128, 20, 13, 8,   2, 12, 3, 2, Cv=5, Tv=256),    # Tv = 256: the LDS column's limit
    _c("t_av128_k20p20_e3",     "dptn",     128, 20, 20, 3,   3, 19, 0, 1, Cv=512, Tv=65),   # L = 79
    _c("t_a64_k20p5_e6",        "dptn",      64, 20,  5, 6,  23,  4, 2, 3),                  # L = 134
    _c("t_a64_k21p10_e7",       "dptn",      64, 21, 10, 7,   2,  0, 2, 2),                  # L = 31
    _c("t_a64_k20p20_e8",       "dptn",      64, 20, 20, 8,   2,  0, 3, 2),                  # L = 40
    _c("t_r64_k9p2_e4",         "dprnn",     64,  9,  2, 4,  62,  0, 1, 2),                  # L = 131
    _c("t_r64_k5p1_e2",         "dprnn",     64,  5,  1, 2,   4,  0, 0, 3),                  # L = 8
    _c("t_m64_k20p5_e3",        "dptn_mask", 64, 20,  5, 3,   4,  4, 0, 2),                  # L = 39
    _c("t_m64_k20p13_e6",       "dptn_mask", 64, 20, 13, 6,   3,  0, 2, 1),                  # L = 46
]
GATE_CASE = "t_av128_k21p10_e5"
#: the geometry of the memory-safety variant "path_ends" (tests/memsafety_child.py): chunk 21, step 5, kernel 8
MEMSAFETY_GEOMETRY = _c("av128_k21p5_e8", "dptn", 128, 21, 5, 8, 9, 4, 3, 3, Cv=512, Tv=13)      # L = 65

STAGE = {c.name: c for c in STAGE_CASES + [MEMSAFETY_GEOMETRY]}
TRAIN = {c.name: c for c in TRAIN_CASES}


# ------------------------------------------------------------------------------------------------------------------
# operands
# ------------------------------------------------------------------------------------------------------------------
def _seed(case: Case, salt: int) -> List[int]:
    return [salt, case.N, case.K, case.P, case.kenc, case.S, case.B]


def gaussian_operands(case: Case, gate: float = 0.7) -> Tuple[DPTNConfig, Dict[str, np.ndarray], Dict[str, np.ndarray], np.ndarray]:
    """-> (cfg, state dict, inputs, block output x [B][S][K][N]) of the value tests: the project's seeded weights and
    inputs, `gate` set by hand, and a seeded Gaussian in place of the last block's output."""
    cfg = case.cfg()
    sd = synthetic_state_dict(cfg, seed=7)
    if case.av:
        sd["gate"] = np.array([gate], np.float32)
    inp = synthetic_inputs(cfg, B=case.B, T=case.T, Tv=case.Tv, seed=31)
    x = np.random.default_rng(_seed(case, 1)).standard_normal((case.B, case.S, case.K, case.N)).astype(np.float32)
    return cfg, sd, inp, x


END_INT_KEYS = ("encoder.weight", "dprnn.speakers_separation.1.weight", "dprnn.speakers_separation.1.bias",
                "dprnn.postprocessing.0.weight", "dprnn.postprocessing.0.bias", "decoder.weight")


def exact_operands(case: Case) -> Tuple[DPTNConfig, Dict[str, np.ndarray], np.ndarray, np.ndarray]:
    """-> (audio-only cfg, state dict, mix [B][T], x [B][S][K][N]): the end parameters are integers in [-2, 2], the PReLU
    slope is 0.25, mix holds integers in [-3, 3] and x integers in [-4, 4] (see `exactness`)."""
    assert not case.masked
    cfg = case.cfg(audio_only=True)
    sd = synthetic_state_dict(cfg, seed=7)
    rng = np.random.default_rng(_seed(case, 2))
    for k in END_INT_KEYS:
        sd[k] = rng.integers(-2, 3, size=sd[k].shape).astype(np.float32)
    sd["dprnn.speakers_separation.0.weight"] = np.array([0.25], np.float32)
    mix = rng.integers(-3, 4, size=(case.B, case.T)).astype(np.float32)
    x = rng.integers(-4, 5, size=(case.B, case.S, case.K, case.N)).astype(np.float32)
    return cfg, sd, mix, x


# ------------------------------------------------------------------------------------------------------------------
# restatements (numpy, any dtype)
# ------------------------------------------------------------------------------------------------------------------
def head(cfg: DPTNConfig, sd, inp, dtype) -> Dict[str, np.ndarray]:
    """-> {"conv": encoder conv alone, "enc": fused latent [B][L][N], "chunked": [B][S][K][N]}"""
    p = {k: np.asarray(v, dtype) for k, v in sd.items()}
    conv = O.encoder_conv(np.asarray(inp["mix"], dtype), p["encoder.weight"], cfg.stride_enc)
    enc = conv
    if not cfg.audio_only:
        enc = O.video_fusion(conv, np.asarray(inp["s1_embedding"], dtype), np.asarray(inp["s2_embedding"], dtype), p)
    x = O.split_to_folds(enc, cfg.chunk_size, cfg.step_size)
    return {"conv": conv.transpose(0, 2, 1), "enc": enc.transpose(0, 2, 1), "chunked": x.transpose(0, 2, 3, 1)}


def waves_from_taps(D: np.ndarray, kenc: int, stride: int, T: int) -> np.ndarray:
    """tap table (2,B,L,8) -> (2,B,T): y[stride i + j] += D[i][j], centred in T (O.decoder_deconv's second half)."""
    L = D.shape[2]
    n = (L - 1) * stride + kenc
    y = np.zeros(D.shape[:2] + (n,), D.dtype)
    for j in range(kenc):
        y[..., j:j + stride * L:stride] += D[..., j]
    out = np.zeros(D.shape[:2] + (T,), D.dtype)
    out[..., (T - n) // 2:(T - n) // 2 + n] = y
    return out


def tail(cfg: DPTNConfig, sd, x: np.ndarray, enc: np.ndarray, T: int, dtype, folded: bool = False) -> Dict[str, np.ndarray]:
    """x [B][S][K][N], enc [B][L][N] -> {"taps": (2,B,L,8), "s1_pred", "s2_pred": (B,T), "pad_taps": the tap rows of a padded
    frame, (B,L,8) (what a frame outside [left, left + ola) must hold: its u is zero)}.  folded (linear tail only): the
    association of fold_decoder_kernel / taps_fold_kernel, D = [u | E] . [G | W_dec] + bd with G = W_dec^T W_post."""
    p = {k: np.asarray(v, dtype) for k, v in sd.items()}
    xb = np.asarray(x, dtype).transpose(0, 3, 1, 2)
    e = np.asarray(enc, dtype).transpose(0, 2, 1)                        # (B,N,L)
    L, P, wdec = e.shape[-1], cfg.step_size, p["decoder.weight"]
    taps: dict = {}
    if cfg.mask_tail:
        m = MR.masked_tail(xb, L, p, P, taps)
        q = m * e[None]
        D = MR.decoder_taps(q, wdec)
        m0 = np.maximum(np.tanh(p["dprnn.output.0.bias"]) * O._sigmoid(p["dprnn.output_gate.0.bias"]), 0.0)
        pad = MR.decoder_taps((m0[None, :, None] * e)[None], wdec)[0]
    else:
        Wp, bp = p["dprnn.postprocessing.0.weight"][:, :, 0], p["dprnn.postprocessing.0.bias"]
        masks = O.separation_tail(xb, L, p, P, taps)
        pad = MR.decoder_taps((bp[None, :, None] + e)[None], wdec)[0]
        if folded:
            B, N = e.shape[0], e.shape[1]
            left, ola = (L - taps["ola"].shape[-1]) // 2, taps["ola"].shape[-1]
            u = np.zeros((B, 2 * N, L), dtype)
            u[:, :, left:left + ola] = taps["ola"]
            u = u.reshape(B, 2, N, L).transpose(1, 0, 2, 3)              # (2,B,N,L)
            G = wdec[:, 0, :].T @ Wp                                     # (k,N)
            bd = wdec[:, 0, :].T @ bp                                    # (k,)
            ue = np.concatenate([u, np.broadcast_to(e[None], u.shape)], 2)          # (2,B,2N,L)
            Wf = np.concatenate([G, wdec[:, 0, :].T], 1)                 # (k,2N)
            D = np.zeros(u.shape[:2] + (L, 8), dtype)
            D[..., :wdec.shape[-1]] = np.einsum("jbcl,kc->jblk", ue, Wf) + bd
        else:
            D = MR.decoder_taps(masks + e[None], wdec)
    w = waves_from_taps(D, cfg.kernel_size_enc, cfg.stride_enc, T)
    return {"taps": D, "s1_pred": w[0], "s2_pred": w[1], "pad_taps": pad}


def tail_truth(cfg, sd, x, enc, T) -> Dict[str, np.ndarray]:
    """fp64, the reference's own association, and the waveforms by the oracle's decoder (not through the tap table)."""
    out = tail(cfg, sd, x, enc, T, np.float64)
    p = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    xb = np.asarray(x, np.float64).transpose(0, 3, 1, 2)
    e = np.asarray(enc, np.float64).transpose(0, 2, 1)
    if cfg.mask_tail:
        q = MR.masked_tail(xb, e.shape[-1], p, cfg.step_size) * e[None]
    else:
        q = O.separation_tail(xb, e.shape[-1], p, cfg.step_size) + e[None]
    for j, k in enumerate(("s1_pred", "s2_pred")):
        w = O.decoder_deconv(q[j], p["decoder.weight"], cfg.stride_enc, T)
        assert np.allclose(w, out[k], rtol=0, atol=1e-9 * max(1.0, float(np.abs(w).max())))
        out[k] = w
    return out


# ------------------------------------------------------------------------------------------------------------------
# judges
# ------------------------------------------------------------------------------------------------------------------
def as_rows(name: str, a: np.ndarray) -> np.ndarray:
    """A tensor as its judged rows [rows][width]: the last axis for enc / conv / chunked / taps / pad_taps, 16-sample
    windows (the last one zero-filled) for a waveform."""
    a = np.asarray(a, np.float64)
    if name in ("s1_pred", "s2_pred"):
        B, T = a.shape
        n = -(-T // WINDOW) * WINDOW
        z = np.zeros((B, n))
        z[:, :T] = a
        return z.reshape(-1, WINDOW)
    return a.reshape(-1, a.shape[-1])


def row_figures(name: str, got: np.ndarray, ref64: np.ndarray, scale_of: Optional[np.ndarray] = None) -> np.ndarray:
    """Per row: ||got - ref|| / RMS over all rows of ||ref|| (`scale_of`: the tensor whose rows give that scale, where
    `ref64` is only a selection of its rows)."""
    g, r = as_rows(name, got), as_rows(name, ref64)
    assert g.shape == r.shape, (name, g.shape, r.shape)
    s = r if scale_of is None else as_rows(name, scale_of)
    scale = float(np.sqrt((s ** 2).sum(1).mean()))
    assert scale > 0, name
    return np.sqrt(((g - r) ** 2).sum(1)) / scale


def worst_row(name, got, ref64, scale_of=None) -> Tuple[float, int]:
    f = row_figures(name, got, ref64, scale_of)
    assert np.isfinite(f).all(), f"{name}: not finite"
    i = int(np.argmax(f))
    return float(f[i]), i


def judge_rows(tag: str, name: str, got, ref64, ref32, scale_of=None) -> Tuple[float, float, Optional[str]]:
    """-> (worst row, the restatement's worst row, None or what is off).  Prints worst / restatement's worst."""
    w, i = worst_row(name, got, ref64, scale_of)
    y, _ = worst_row(name, ref32, ref64, scale_of)
    print(f"{tag} {name}: worst row {w:.3g} at row {i}, restatement {y:.3g}, ratio {w / y if y > 0 else float('inf'):.2f}")
    if y <= 0:
        return w, y, f"{name}: the fp32 restatement equals fp64 bit for bit: no yardstick"
    if not w <= VALUE_FACTOR * y:
        return w, y, f"{name}: worst row {w:.3g} at row {i} > {VALUE_FACTOR} x {y:.3g} (the fp32 restatement's worst row)"
    return w, y, None


# ------------------------------------------------------------------------------------------------------------------
# the exactness condition of the integer-valued operands
# ------------------------------------------------------------------------------------------------------------------
EXACT_LIMIT = float(2 ** 22)      # quantum 0.25: every partial sum is k / 4 with |k| < 2^24, exact in fp32 in any order


def exactness(case: Case) -> Dict[str, float]:
    """-> {contraction: max over its outputs of sum |a b|} for every contraction of the head and of both linear tails on
    `exact_operands(case)` (the operands a, b are the exact values themselves, from the fp64 oracle), all of which must stay
    below EXACT_LIMIT.  The sum of absolute products bounds every partial sum of that contraction in any order and with any
    split (an MFMA's k blocks, four interleaved accumulators, the folded form's two halves).  Overlap-add, the bias / skip
    additions and the decoder's tap gather are sums too and are bounded the same way."""
    cfg, sd, mix, x = exact_operands(case)
    q = {k: np.asarray(v, np.float64) for k, v in sd.items()}
    A = np.abs
    ein = np.einsum
    enc = O.encoder_conv(mix.astype(np.float64), q["encoder.weight"], cfg.stride_enc)          # (B,N,L)
    out = {"encoder": float(O.encoder_conv(A(mix.astype(np.float64)), A(q["encoder.weight"]), cfg.stride_enc).max())}
    L, P = enc.shape[-1], cfg.step_size
    xb = x.astype(np.float64).transpose(0, 3, 1, 2)
    y = np.where(xb >= 0, xb, q["dprnn.speakers_separation.0.weight"] * xb)
    Ws, bs = q["dprnn.speakers_separation.1.weight"][:, :, 0, 0], q["dprnn.speakers_separation.1.bias"]
    out["separation conv + bias"] = float((ein("bnsk,on->bosk", A(y), A(Ws)) + A(bs)[None, :, None, None]).max())
    taps: dict = {}
    masks = O.separation_tail(xb, L, q, P, taps)                          # (2,B,N,L)
    out["overlap-add"] = float(O.overlap_add(A(taps["sep"]), P).max())
    B, N = enc.shape[0], enc.shape[1]
    left, ola = (L - taps["ola"].shape[-1]) // 2, taps["ola"].shape[-1]
    u = np.zeros((B, 2 * N, L))
    u[:, :, left:left + ola] = taps["ola"]
    u = u.reshape(B, 2, N, L).transpose(1, 0, 2, 3)                       # (2,B,N,L)
    Wp, bp, wd = q["dprnn.postprocessing.0.weight"][:, :, 0], q["dprnn.postprocessing.0.bias"], q["decoder.weight"][:, 0, :]
    out["post-processing conv + bias + skip"] = float((ein("jbnl,on->jbol", A(u), A(Wp)) + A(bp)[None, None, :, None]
                                                       + A(enc)[None]).max())
    qq = masks + enc[None]                                                # what the decoder consumes
    D = ein("jbcl,ck->jblk", A(qq), A(wd))
    out["decoder taps"] = float(D.max())
    G, bd = wd.T @ Wp, wd.T @ bp
    out["fold G = W_dec^T W_post"] = float((A(wd).T @ A(Wp)).max())
    out["fold bd = W_dec^T b_post"] = float((A(wd).T @ A(bp)).max())
    out["folded contraction [u|E].[G|W_dec] + bd"] = float((ein("jbcl,kc->jblk", A(u), A(G)) + ein("bcl,ck->blk", A(enc), A(wd))[None]
                                                            + A(bd)).max())
    Dt = A(ein("jbcl,ck->jblk", qq, wd))
    Dt = np.concatenate([Dt, np.zeros(Dt.shape[:3] + (8 - Dt.shape[3],))], 3)
    out["decoder gather"] = float(waves_from_taps(Dt, cfg.kernel_size_enc, cfg.stride_enc, case.T).max())
    return out


@functools.lru_cache(maxsize=None)
def exact_truth(name: str) -> Dict[str, np.ndarray]:
    """The fp64 oracle on `exact_operands` -> enc, chunked, taps, s1_pred, s2_pred (shared, read-only)."""
    case = STAGE[name]
    cfg, sd, mix, x = exact_operands(case)
    h = head(cfg, sd, {"mix": mix}, np.float64)
    t = tail_truth(cfg, sd, x, h["enc"], case.T)
    out = {"enc": h["enc"], "chunked": h["chunked"], "taps": t["taps"], "s1_pred": t["s1_pred"], "s2_pred": t["s2_pred"]}
    for v in out.values():
        v.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------------------------
# the value tests' references: fp64 truth and fp32 restatements, computed once per (case, gate)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def value_refs(name: str, gate: float = 0.7) -> Dict[str, Dict[str, np.ndarray]]:
    """-> {"h64", "h32"}: head() in fp64 (the truth) and in fp32 (the yardstick); shared, read-only."""
    case = STAGE[name]
    cfg, sd, inp, x = gaussian_operands(case, gate)
    out = {"h64": head(cfg, sd, inp, np.float64), "h32": head(cfg, sd, inp, np.float32)}
    for d in out.values():
        for v in d.values():
            v.setflags(write=False)
    return out


def tail_refs(case: Case, enc: np.ndarray, gate: float = 0.7) -> Dict[str, Dict[str, np.ndarray]]:
    """stage_tail takes the block output x and a latent: both are INPUTS of the tail, so the truth and the restatements are
    evaluated on the very fp32 latent the tail is handed (`enc`, [B][L][N]).  -> {"t64", "t32" (GEMM association), "t32f"
    (folded association; linear tails only)}."""
    cfg, sd, _, x = gaussian_operands(case, gate)
    out = {"t64": tail_truth(cfg, sd, x, enc, case.T), "t32": tail(cfg, sd, x, enc, case.T, np.float32)}
    if not case.masked:
        out["t32f"] = tail(cfg, sd, x, enc, case.T, np.float32, folded=True)
    return out


def padded_frames(case: Case) -> np.ndarray:
    t = np.arange(case.L)
    return t[(t < case.left) | (t >= case.left + case.ola)]


# ------------------------------------------------------------------------------------------------------------------
# fast_div (headtail.h): the float estimate with one correction each way, restated in numpy float32
# ------------------------------------------------------------------------------------------------------------------
def fast_div(n: np.ndarray, d: int, nf: Optional[np.ndarray] = None) -> np.ndarray:
    """n: int32 array, 0 <= n < 2^23 -> floor(n / d) as headtail.h computes it.  nf: float32(n), if the caller has it."""
    inv = np.float32(1.0) / np.float32(d)
    nf = n.astype(np.float32) if nf is None else nf
    q = (nf * inv).astype(np.int32)              # C's (int) of a non-negative float: truncation
    r = n - q * np.int32(d)
    q += (r >= d)
    q -= (r < 0)
    return q


# ------------------------------------------------------------------------------------------------------------------
# gradient references (torch autograd on the stock-PyTorch composition)
# ------------------------------------------------------------------------------------------------------------------
# The FFN's ReLU (dptn.py:51) has a kink at h = 0: a one-block model has 10^5..10^6 hidden values, the smallest |h| of a draw
# can lie below what fp32 resolves, fp32 and fp64 then disagree on the sign of that one unit and every gradient upstream of
# it differs by a finite amount, about 1 / sqrt(number of units) of its norm (tests/test_gpu_backward.py picks its seeds for
# the same reason and keeps |h| above 4e-7).  A property of the function at those inputs, decided on the CPU in fp64 alone
# (`ffn_kink_margin`, asserted for every case by tests/test_path_ends_host.py): with the default seed the 1.5 million hidden
# values of t_av128_k20p5_e2_L515 come as close as 3.5e-8 to zero (on the MI355X its intra-chunk gradients were then 2e-4 off,
# the tail's were not), and the fp32 restatement of t_a64_k20p5_e6 is at 1e-3 of fp64; a case whose default draw comes
# closer than KINK_MARGIN at any of its gates gets the first seed after 41 that does not.
TRAIN_INPUT_SEED = {"t_av128_k20p5_e2_L515": 81, "t_av128_k21p10_e5": 44, "t_a64_k20p5_e6": 43, "t_m64_k20p5_e3": 42}
KINK_MARGIN = 4e-7


def ffn_kink_margin(case: Case, gate: float = 0.7) -> float:
    """Smallest |input of the FFN's ReLU| over both paths of the case's model in fp64 (inf for DPRNN blocks: no ReLU)."""
    import torch
    from unittest import mock
    import oracle.torch_stock as TS
    cfg, sd, inp, _, _ = train_operands(case, gate)
    seen = [float("inf")]
    relu = TS.F.relu

    def spy(x, *a, **k):
        seen.append(float(x.detach().abs().min()))
        return relu(x, *a, **k)

    plain = DPTNConfig(**{**cfg.to_dict(), "arch": cfg.blocks, "audio_only": cfg.audio_only})
    ref = TS.StockDPTN(plain, sd)
    ref.sd = {k: v.double() for k, v in ref.sd.items()}
    ref.paths = [(pre, m.double() if m is not None else None, r.double()) for pre, m, r in ref.paths]
    with mock.patch.object(TS.F, "relu", spy):
        try:
            ref(**{k: torch.from_numpy(v).double() for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")})
        except KeyError:      # the masked model: its head and paths are StockDPTN's own and have run; its tail is not
            assert cfg.mask_tail and len(seen) == 3
    return min(seen)


def train_operands(case: Case, gate: float = 0.7):
    """-> (cfg, state dict, inputs, d1, d2): seeded weights (non-zero video_ln.bias), inputs and output gradients."""
    cfg = case.cfg()
    sd = synthetic_state_dict(cfg, seed=11)
    if case.av:
        sd["gate"] = np.array([gate], np.float32)
        assert np.abs(sd["video_ln.bias"]).min() > 0
    inp = synthetic_inputs(cfg, B=case.B, T=case.T, Tv=case.Tv, seed=TRAIN_INPUT_SEED.get(case.name, 41))
    rng = np.random.default_rng(_seed(case, 3))
    d1 = rng.standard_normal((case.B, case.T)).astype(np.float32)
    d2 = rng.standard_normal((case.B, case.T)).astype(np.float32)
    return cfg, sd, inp, d1, d2


def stock_gradients(cfg: DPTNConfig, sd, inp, d1, d2, dtype) -> Dict[str, "object"]:
    """d (sum s1_pred d1 + s2_pred d2) / d every parameter by torch.autograd on oracle.torch_stock.StockDPTN in `dtype`
    (torch.float64: the reference; torch.float32: the yardstick).  The masked model (DPTNEncDec) takes StockDPTN's head and
    paths and the tail of tests/mask_tail_ref.py restated with torch operators."""
    import torch
    import torch.nn.functional as F
    from oracle.torch_stock import StockDPTN

    plain = DPTNConfig(**{**cfg.to_dict(), "arch": cfg.blocks})
    ref = StockDPTN(plain, sd)
    ref.sd = {k: v.to(dtype).requires_grad_(True) for k, v in ref.sd.items()}
    ref.paths = [(pre, m.to(dtype) if m is not None else None, r.to(dtype)) for pre, m, r in ref.paths]
    mods = [m for _, m, r in ref.paths if m is not None] + [r for _, m, r in ref.paths]
    for m in mods:
        for q in m.parameters():
            q.requires_grad_(True)
    t = {k: torch.from_numpy(v).to(dtype) for k, v in inp.items() if k in ("mix", "s1_embedding", "s2_embedding")}
    g1, g2 = torch.from_numpy(d1).to(dtype), torch.from_numpy(d2).to(dtype)
    with torch.enable_grad():
        if not cfg.mask_tail:
            out = StockDPTN.__call__.__wrapped__(ref, **t)
            s1, s2 = out["s1_pred"], out["s2_pred"]
        else:
            w, N, K, P = ref.sd, cfg.num_features, cfg.chunk_size, cfg.step_size
            mix = t["mix"]
            B, T = mix.shape
            enc = F.conv1d(mix.unsqueeze(1), w["encoder.weight"], stride=cfg.stride_enc)
            L = enc.shape[-1]
            x = F.unfold(enc.unsqueeze(-1), kernel_size=(K, 1), stride=(P, 1)).view(B, N, K, -1).permute(0, 1, 3, 2)
            S = x.shape[2]
            x = x.permute(0, 2, 3, 1).reshape(B * S, K, N)
            (pre0, m0, r0), (pre1, m1, r1) = ref.paths
            x = ref._path(x, pre0, m0, r0).view(B, S, K, N).transpose(1, 2).reshape(B * K, S, N)
            x = ref._path(x, pre1, m1, r1).view(B, K, S, N).transpose(1, 2).reshape(B * S, K, N)
            x = x.view(B, S, K, N).permute(0, 3, 1, 2)
            x = F.prelu(x, w["dprnn.speakers_separation.0.weight"])
            x = F.conv2d(x, w["dprnn.speakers_separation.1.weight"], w["dprnn.speakers_separation.1.bias"])
            ola = (S - 1) * P + K
            x = F.fold(x.permute(0, 1, 3, 2).reshape(B, 2 * N * K, S), output_size=(ola, 1), kernel_size=(K, 1),
                       stride=(P, 1)).squeeze(3)
            pad = L - ola
            x = F.pad(x, (pad // 2, pad - pad // 2)).view(B, 2, N, L).transpose(0, 1)
            preds = []
            for j in range(2):
                m = F.relu(torch.tanh(F.conv1d(x[j], w["dprnn.output.0.weight"], w["dprnn.output.0.bias"]))
                           * torch.sigmoid(F.conv1d(x[j], w["dprnn.output_gate.0.weight"], w["dprnn.output_gate.0.bias"])))
                y = F.conv_transpose1d(m * enc, w["decoder.weight"], stride=cfg.stride_enc)
                padn = T - y.shape[-1]
                preds.append(F.pad(y, (padn // 2, padn - padn // 2)).squeeze(1))
            s1, s2 = preds
        ((s1 * g1).sum() + (s2 * g2).sum()).backward()
    want = {}
    for pre, m, r in ref.paths:
        if m is not None:
            want[pre + "mha.in_proj_weight"], want[pre + "mha.in_proj_bias"] = m.in_proj_weight.grad, m.in_proj_bias.grad
            want[pre + "mha.out_proj.weight"], want[pre + "mha.out_proj.bias"] = m.out_proj.weight.grad, m.out_proj.bias.grad
        for k, v in r.named_parameters():
            want[pre + "rnn." + k] = v.grad
    for k, v in ref.sd.items():
        if k not in want and v.grad is not None:
            want[k] = v.grad
    return {k: v.detach() for k, v in want.items()}


END_PREFIXES = ("encoder.weight", "decoder.weight", "visual_compression.", "video_ln.", "gate", "dprnn.speakers_separation.",
                "dprnn.postprocessing.", "dprnn.output")


def is_end_tensor(key: str) -> bool:
    return key.startswith(END_PREFIXES)
