"""VoiceFilter (src/model/voicefilter.py:108-145, eval mode, from the lip embeddings on) restated on stock PyTorch CPU
operators, the reference's get_magnitude formula, and the seeded weights and inputs the tests and
tools/gen_golden_voicefilter.py share.

synthetic_voicefilter_weights(input_size, embed_size, seed) -> {key: numpy array} in the reference's state_dict() order
synthetic_inputs(input_size, W, Tv, B, embed_size, seed) -> (mix_magnitude, s1_embedding, s2_embedding)
run(weights, mix, e1, e2, dtype, taps=None) -> (s1_spec_pred, s2_spec_pred), each (B, F, W) of `dtype`
"""
from __future__ import annotations

import hashlib

import numpy as np
import torch
import torch.nn.functional as F_

HIDDEN, FC = 400, 600
BN_EPS = 1e-5
# (Conv2d index, BatchNorm2d index, out, in, kernel rows, kernel columns, row dilation) in the reference's nn.Sequential
CNN = ((1, 2, 64, 1, 1, 7, 1), (5, 6, 64, 64, 7, 1, 1), (9, 10, 64, 64, 5, 5, 1), (13, 14, 64, 64, 5, 5, 2),
       (17, 18, 64, 64, 5, 5, 4), (21, 22, 64, 64, 5, 5, 8), (25, 26, 64, 64, 5, 5, 16), (28, 29, 8, 64, 1, 1, 1))
# (input_size, W, Tv, B): the real feature size with few frames; F below the reach of dilations 8 and 16; W below the 7-tap
# width and Tv = 1; an even input_size that is no multiple of 16
GOLDEN_SHAPES = ((201, 21, 5, 2), (33, 50, 3, 1), (17, 7, 1, 3), (40, 33, 4, 2))
GOLDEN_EMBED = 1024
WEIGHT_SEED, INPUT_SEED = 0, 41


def voicefilter_state_dict_spec(input_size, embed_size=1024):
    """[(key, shape, kind)]: the 82 entries of the reference's state_dict() (lip reader stubbed), in its order."""
    F, E = input_size, embed_size
    spec = []
    for layer in range(2):
        for suffix in ("", "_reverse"):
            s = f"_l{layer}{suffix}"
            spec += [(f"gru.weight_ih{s}", (3 * F, E if layer == 0 else 2 * F), "gru_ih"), (f"gru.weight_hh{s}", (3 * F, F), "rnn"),
                     (f"gru.bias_ih{s}", (3 * F,), "rnn"), (f"gru.bias_hh{s}", (3 * F,), "rnn")]
    spec += [("fc_dvector.weight", (F, 2 * F), "lin"), ("fc_dvector.bias", (F,), "bias")]
    for ci, bi, cout, cin, kh, kw, _ in CNN:
        spec += [(f"cnn_layers.{ci}.weight", (cout, cin, kh, kw), "conv"), (f"cnn_layers.{ci}.bias", (cout,), "bias"),
                 (f"cnn_layers.{bi}.weight", (cout,), "bn_w"), (f"cnn_layers.{bi}.bias", (cout,), "bn_b"),
                 (f"cnn_layers.{bi}.running_mean", (cout,), "bn_m"), (f"cnn_layers.{bi}.running_var", (cout,), "bn_v"),
                 (f"cnn_layers.{bi}.num_batches_tracked", (), "nbt")]
    spec += [("lstm.weight_ih_l0", (4 * HIDDEN, 9 * F), "lstm_ih"), ("lstm.weight_hh_l0", (4 * HIDDEN, HIDDEN), "lstm"),
             ("lstm.bias_ih_l0", (4 * HIDDEN,), "lstm"), ("lstm.bias_hh_l0", (4 * HIDDEN,), "lstm"),
             ("fc.1.weight", (FC, HIDDEN), "lin"), ("fc.1.bias", (FC,), "bias"),
             ("fc.4.weight", (F, FC), "lin"), ("fc.4.bias", (F,), "bias")]
    return spec


def synthetic_voicefilter_weights(input_size, embed_size=1024, seed=WEIGHT_SEED):
    """Seeded, non-degenerate weights (numpy PCG64).  Conv N(0, 2 / fan_in); BN weight and running_var U(0.5, 1.5), BN bias
    and running_mean N(0, 0.2^2), all different per channel; Linear weights N(0, 2 / fan_in) (the FC tail sees ReLU'd inputs)
    and biases N(0, 0.1^2); recurrent weights and biases U(+-1 / sqrt(hidden)) as PyTorch initialises them, input weights
    N(0, 1 / fan_in) so that the gates see unit-size sums and are neither linear nor saturated throughout."""
    rng = np.random.Generator(np.random.PCG64(seed))
    F = input_size
    sd = {}
    for key, shape, kind in voicefilter_state_dict_spec(input_size, embed_size):
        if kind == "conv" or kind == "lin":
            v = rng.standard_normal(shape) * np.sqrt(2.0 / int(np.prod(shape[1:])))
        elif kind in ("gru_ih", "lstm_ih"):
            v = rng.standard_normal(shape) * np.sqrt(1.0 / shape[1])
        elif kind == "rnn":
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(F)
        elif kind == "lstm":
            v = rng.uniform(-1.0, 1.0, shape) / np.sqrt(HIDDEN)
        elif kind == "bias":
            v = rng.standard_normal(shape) * 0.1
        elif kind in ("bn_w", "bn_v"):
            v = rng.uniform(0.5, 1.5, shape)
        elif kind in ("bn_b", "bn_m"):
            v = rng.standard_normal(shape) * 0.2
        else:
            sd[key] = np.array(0, dtype=np.int64)
            continue
        sd[key] = np.ascontiguousarray(v, dtype=np.float32)
    return sd


def synthetic_inputs(input_size, W, Tv, B, embed_size=1024, seed=INPUT_SEED):
    """mix_magnitude (B, F, W) in [0, 1] with exact zeros and exact ones (about 5 % each, as get_magnitude's clamps give) and
    two different N(0, 1) embedding sequences (B, Tv, E)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    mix = rng.uniform(0.0, 1.0, (B, input_size, W))
    kind = rng.uniform(0.0, 1.0, mix.shape)
    mix[kind < 0.05] = 0.0
    mix[kind > 0.95] = 1.0
    mix.reshape(-1)[:2] = (0.0, 1.0)
    e1 = rng.standard_normal((B, Tv, embed_size))
    e2 = rng.standard_normal((B, Tv, embed_size))
    return mix.astype(np.float32), e1.astype(np.float32), e2.astype(np.float32)


def weights_digest(sd) -> str:
    h = hashlib.sha256()
    for k, v in sd.items():
        h.update(k.encode())
        h.update(np.ascontiguousarray(v).tobytes())
    return h.hexdigest()


def run(weights, mix, e1, e2, dtype=torch.float64, taps=None, modules=None):
    """weights: {key: array}; mix (B, F, W); e1, e2 (B, Tv, E); computed on the device of `mix`.  taps: a dict that receives
    "relu<l>" (share of non-zero outputs of ReLU l = 1..7) and "mask1" / "mask2" (the sigmoid outputs).  modules: a dict
    that keeps the nn.GRU / nn.LSTM built from the weights for the next call with the same weights (timing loops)."""
    def tensor(v):
        return (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).to(dtype)

    w = {k: tensor(v) for k, v in weights.items() if not k.endswith("num_batches_tracked")}
    mix, e1, e2 = tensor(mix), tensor(e1), tensor(e2)
    B, F, W = mix.shape
    E = e1.shape[2]
    with torch.no_grad():
        if modules is not None and "gru" in modules:
            gru, lstm = modules["gru"], modules["lstm"]
        else:
            gru = torch.nn.GRU(E, F, num_layers=2, bidirectional=True, batch_first=True).to(device=mix.device, dtype=dtype)
            gru.load_state_dict({k[4:]: v for k, v in w.items() if k.startswith("gru.")}, strict=True)
            lstm = torch.nn.LSTM(9 * F, HIDDEN, batch_first=True).to(device=mix.device, dtype=dtype)
            lstm.load_state_dict({k[5:]: v for k, v in w.items() if k.startswith("lstm.")}, strict=True)
            if modules is not None:
                modules["gru"], modules["lstm"] = gru, lstm
        dvecs = [F_.linear(gru(e)[0][:, -1, :], w["fc_dvector.weight"], w["fc_dvector.bias"]) for e in (e1, e2)]
        x = mix.unsqueeze(1)
        for l, (ci, bi, cout, cin, kh, kw, dil) in enumerate(CNN):
            x = F_.conv2d(x, w[f"cnn_layers.{ci}.weight"], w[f"cnn_layers.{ci}.bias"], 1, ((kh // 2) * dil, kw // 2), (dil, 1))
            p = f"cnn_layers.{bi}."
            x = F_.batch_norm(x, w[p + "running_mean"], w[p + "running_var"], w[p + "weight"], w[p + "bias"], False, 0.0, BN_EPS)
            if l < 7:
                x = F_.relu(x)
                if taps is not None:
                    taps[f"relu{l + 1}"] = float((x > 0).double().mean())
        x = x.permute(0, 3, 2, 1).contiguous().view(B, 8 * F, W)
        outs = []
        for i, dv in enumerate(dvecs):
            cat = torch.cat((x, dv.unsqueeze(-1).expand(-1, -1, W)), dim=1)
            h = lstm(cat.transpose(1, 2))[0]
            h = F_.relu(F_.linear(F_.relu(h), w["fc.1.weight"], w["fc.1.bias"]))
            mask = torch.sigmoid(F_.linear(h, w["fc.4.weight"], w["fc.4.bias"])).transpose(1, 2)
            if taps is not None:
                taps[f"mask{i + 1}"] = mask
            outs.append(mask * mix)
    return outs[0], outs[1]


def col_rel(got, ref64):
    """Per (item, frame) column of F values of one speaker's (B, F, W) output: ||got - ref||_2 / ||ref||_2, in fp64."""
    got = torch.as_tensor(got).double()
    ref = torch.as_tensor(ref64).double()
    return ((got - ref).norm(dim=1) / ref.norm(dim=1)).numpy()


def worst_col(got_pair, ref_pair):
    """The worst column over both speakers."""
    return max(float(col_rel(g, r).max()) for g, r in zip(got_pair, ref_pair))


def magnitude(audio, n_fft=400, hop_length=100):
    """The reference's get_magnitude formula (src/datasets/base_dataset.py:167-180) on torch.stft, at the dtype of `audio`:
    -> (spec, phase, |S|)."""
    S = torch.stft(audio, n_fft=n_fft, hop_length=hop_length, win_length=n_fft, window=torch.hann_window(n_fft, dtype=audio.dtype),
                   center=True, return_complex=True)
    mag = torch.abs(S)
    spec = 20.0 * torch.log10(torch.clamp(mag, min=1e-5)) - 20
    return torch.clamp(spec / 100, min=-1.0, max=0.0) + 1.0, torch.angle(S), mag
