"""TEST INFRASTRUCTURE: numpy restatement of the masked DPTN separator (DPTNEncDec, the reference's src/model/dptn.py:82-208),
composed with the head, block and decoder functions of oracle/dptn_oracle.py (which it leaves as they are).

The tail, per speaker (dptn.py:122-141, 185-193):
    u      = pad(OverlapAdd(Conv2d_1x1(PReLU(x))))[spk]           (B,N,L), zero frames outside [left, left + ola)
    m      = ReLU(tanh(W_out u + b_out) * sigmoid(W_gate u + b_gate))
    s_pred = pad(ConvTranspose1d(m * encoded))
The padding comes BEFORE the two 1x1 convs, so the padded frames are not zero in m: there m = ReLU(tanh(b_out) *
sigmoid(b_gate)), which multiplies a nonzero encoded frame.
"""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np

from oracle import dptn_oracle as O


def masked_tail(x: np.ndarray, L: int, p: Dict[str, np.ndarray], P: int, taps: Optional[dict] = None) -> np.ndarray:
    """x (B,N,S,K) = last block's output -> m (2,B,N,L)."""
    B, N, S, K = x.shape
    a = p["dprnn.speakers_separation.0.weight"]
    y = np.where(x >= 0, x, a * x)
    W = p["dprnn.speakers_separation.1.weight"][:, :, 0, 0]
    sep = np.einsum("bnsk,on->bosk", y, W) + p["dprnn.speakers_separation.1.bias"][None, :, None, None]
    ola = O.overlap_add(sep, P)
    left = (L - ola.shape[-1]) // 2
    padded = np.zeros((B, 2 * N, L), dtype=x.dtype)
    padded[:, :, left:left + ola.shape[-1]] = ola
    u = padded.reshape(B, 2, N, L).transpose(1, 0, 2, 3)                 # (2,B,N,L)
    a_out = np.einsum("jbnl,on->jbol", u, p["dprnn.output.0.weight"][:, :, 0]) + p["dprnn.output.0.bias"][None, None, :, None]
    a_gate = (np.einsum("jbnl,on->jbol", u, p["dprnn.output_gate.0.weight"][:, :, 0])
              + p["dprnn.output_gate.0.bias"][None, None, :, None])
    m = np.maximum(np.tanh(a_out) * O._sigmoid(a_gate), 0.0)
    if taps is not None:
        taps["sep"], taps["ola"], taps["masks"], taps["left"] = sep, ola, m, left
    return m


def decoder_taps(q: np.ndarray, w: np.ndarray) -> np.ndarray:
    """q (2,B,N,L) decoder input -> (2,B,L,8) tap products D[spk][b][l][j] = sum_c q[c,l] w[c,0,j] (columns >= k: 0),
    the table the library leaves in its workspace ("taps")."""
    k = w.shape[-1]
    D = np.zeros(q.shape[:2] + (q.shape[-1], 8), dtype=q.dtype)
    D[..., :k] = np.einsum("jbcl,ck->jblk", q, w[:, 0, :])
    return D


def forward(cfg, params: Dict[str, np.ndarray], mix: np.ndarray, dtype=np.float64,
            taps: Optional[dict] = None, **_ignored) -> Dict[str, np.ndarray]:
    """DPTNEncDec.forward (dptn.py:185-197) -> {"s1_pred", "s2_pred"} (B,T)."""
    p = {k: np.asarray(v, dtype=dtype) for k, v in params.items()}
    mix = np.asarray(mix, dtype=dtype)
    B, T = mix.shape
    enc = O.encoder_conv(mix, p["encoder.weight"], cfg.stride_enc)
    L = enc.shape[-1]
    x = O.split_to_folds(enc, cfg.chunk_size, cfg.step_size)
    for b in range(cfg.num_blocks):
        x = O.dptn_block(x, p, b, cfg.num_heads, taps)
    m = masked_tail(x, L, p, cfg.step_size, taps)
    q = m * enc[None]
    if taps is not None:
        taps["encoded"], taps["masked"] = enc, q
    preds = [O.decoder_deconv(q[j], p["decoder.weight"], cfg.stride_enc, T) for j in range(2)]
    return {"s1_pred": preds[0], "s2_pred": preds[1]}
