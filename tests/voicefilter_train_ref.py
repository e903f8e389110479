"""VoiceFilter in TRAINING mode (src/model/voicefilter.py:108-145 from the lip embeddings on: BatchNorm on the batch's
statistics, Dropout2d(0.35) on whole frames) restated on stock PyTorch CPU operators with autograd, the numpy restatement
of the library's dropout keep mask, and what the tests and tools/gen_golden_voicefilter_train.py share.

forward(weights, mix, e1, e2, dtype, keep, relu_masks=None) -> Run: outputs, batch statistics, taps, leaf parameters
Run.grads(d_out1, d_out2) -> {key: gradient} of the 58 trainable tensors
keep_mask(nseq, W, ppm, seed) -> (nseq, W) float32, 1 = kept: csrc/vfilt_train_kernels.h's vftrain_drop_mask_kernel

Sequences are speaker-major: q = speaker * B + item, rows (q, t).  An imposed ReLU keep mask replaces relu(x) by x * mask
(the Conv-TasNet kit's way with PReLU branches): both restatements then differentiate the same piecewise-linear function
as the implementation whose masks they were given.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F_

from tests import dropout_ref as D
from tests.voicefilter_ref import BN_EPS, CNN, FC, HIDDEN, voicefilter_state_dict_spec

P_DROP = 0.35
MOMENTUM = 0.1
TRAIN_SHAPE = (17, 7, 1, 3)            # (F, W, Tv, B) of tests/golden/voicefilter_train_small.npz
MASK_SEED, TARGET_SEED, INDEX_SEED, SAMPLES = 5, 43, 7, 64
CONV_BIAS = tuple(f"cnn_layers.{ci}.bias" for ci, *_ in CNN)
BN_BIAS = tuple(f"cnn_layers.{bi}.bias" for _, bi, *_ in CNN)


def keep_mask(nseq, W, ppm, seed):
    """keep[q][t] = drop_rand_q(drop_qseed(seed, q W + t), 0) >= p 2^24, p = ppm 1e-6; ppm 0 keeps everything."""
    thresh = int(ppm * 1e-6 * 16777216.0)
    ctr = np.arange(nseq * W, dtype=np.uint64)
    r = D.drop_rand_q(D.drop_qseed(int(seed) & 0xFFFFFFFF, ctr), np.zeros_like(ctr))
    return (r >= np.uint64(thresh)).astype(np.float32).reshape(nseq, W)


def fixture_mask(nseq, W, seed=MASK_SEED):
    """The seeded keep mask of the golden run (numpy PCG64 Bernoulli(0.65))."""
    rng = np.random.Generator(np.random.PCG64(seed))
    return (rng.uniform(0.0, 1.0, (nseq, W)) >= P_DROP).astype(np.float32)


def targets(F, W, B, seed=TARGET_SEED):
    """s1_spec_true, s2_spec_true (B, F, W) in [0, 1]"""
    rng = np.random.Generator(np.random.PCG64(seed))
    return rng.uniform(0.0, 1.0, (B, F, W)).astype(np.float32), rng.uniform(0.0, 1.0, (B, F, W)).astype(np.float32)


def trainable_keys(input_size, embed_size=1024):
    return [k for k, _, kind in voicefilter_state_dict_spec(input_size, embed_size) if kind not in ("bn_m", "bn_v", "nbt")]


def sample_indices(spec):
    """{key: sorted flat indices}: every entry of small tensors, else SAMPLES distinct seeded ones (tools/gen_golden_ctasnet_grad.py)"""
    rng = np.random.default_rng(INDEX_SEED)
    out = {}
    for k, shape in spec:
        n = int(np.prod(shape))
        out[k] = np.arange(n) if n <= SAMPLES else np.sort(rng.choice(n, SAMPLES, replace=False))
    return out


def mse_pit_loss(o1, o2, t1, t2):
    """The reference's MSESpecLoss (ss_losses.py:5-44): batch-level PIT over the mean squared error."""
    mse = F_.mse_loss
    l1 = (mse(o1, t1) + mse(o2, t2)) / 2
    l2 = (mse(o1, t2) + mse(o2, t1)) / 2
    return l2 if bool(l2 < l1) else l1


class Run:
    def __init__(self):
        self.params = {}
        self.Z, self.act, self.stats = [], [], []       # per CNN layer: raw conv output, BN(+ReLU), (mean, unbiased variance)
        self.gates = self.cell = self.h = self.fc1 = None
        self.out1 = self.out2 = None

    def grads(self, d_out1, d_out2):
        keys = list(self.params)
        dt = self.out1.dtype
        g = torch.autograd.grad((self.out1, self.out2), [self.params[k] for k in keys],
                                (torch.as_tensor(d_out1).to(dt), torch.as_tensor(d_out2).to(dt)), allow_unused=True, retain_graph=True)
        return {k: (torch.zeros_like(self.params[k]) if gi is None else gi.detach()) for k, gi in zip(keys, g)}

    def loss_grads(self, t1, t2):
        """(MSESpecLoss, {key: gradient}) against the targets t1, t2"""
        dt = self.out1.dtype
        loss = mse_pit_loss(self.out1, self.out2, torch.as_tensor(t1).to(dt), torch.as_tensor(t2).to(dt))
        keys = list(self.params)
        g = torch.autograd.grad(loss, [self.params[k] for k in keys], allow_unused=True, retain_graph=True)
        return loss.detach(), {k: (torch.zeros_like(self.params[k]) if gi is None else gi.detach()) for k, gi in zip(keys, g)}

    def updated_running(self, weights, steps=1):
        """{key: running_mean / running_var after `steps` identical forwards from the weights' buffers} (momentum 0.1)"""
        out = {}
        for l, (ci, bi, *_rest) in enumerate(CNN):
            for name, new in zip(("running_mean", "running_var"), self.stats[l]):
                k = f"cnn_layers.{bi}.{name}"
                r = torch.as_tensor(np.asarray(weights[k])).to(new.dtype)
                for _ in range(steps):
                    r = (1.0 - MOMENTUM) * r + MOMENTUM * new.detach()
                out[k] = r
        return out


class _PlainGrad(torch.autograd.Function):
    """Identity whose backward hands on a gradient in plain contiguous strides.  The map leaves the CNN through
    permute(0, 3, 2, 1).contiguous(), whose backward returns strides (8 F W, 1, 8, 8 F) for a (B, 8, F, W) tensor; at W = 1 or
    F = 1 those are exactly channels-last strides, and torch's CPU batch_norm backward then reads the gradient in one layout
    and its input in the other: d beta is no longer the channel sum of the incoming gradient, and every CNN gradient behind
    it is wrong, in fp32 and fp64 alike (tests/test_voicefilter_values_host.py shows it).  The values are untouched."""

    @staticmethod
    def forward(ctx, x):
        return x.view_as(x)

    @staticmethod
    def backward(ctx, g):
        return g.clone(memory_format=torch.contiguous_format)


def _relu(x, mask):
    return F_.relu(x) if mask is None else x * mask.to(x.dtype)


def forward(weights, mix, e1, e2, dtype=torch.float64, keep=None, relu_masks=None, leaves=False, stock_lstm=False, modules=None):
    """weights: {key: array}; mix (B, F, W); e1, e2 (B, Tv, E); keep: (2B, W) dropout keep mask (None: no dropout).
    relu_masks: None, or {"cnn": 7 x (B, 64, F, W), "lstm": (2B, W, 400), "fc1": (2B, W, 600)} of 0 / 1.
    Computed on the device of `mix` when it is a tensor.  leaves: `weights` are the caller's own leaf tensors of `dtype` on
    that device and are used as they are (a training loop).  stock_lstm: nn.LSTM instead of the step loop (timing; no gate
    taps).  modules: a dict that keeps the nn.GRU / nn.LSTM shells for the next call (timing loops: a training script builds
    its modules once; their own values are never read, functional_call puts the weights in)."""
    dev = mix.device if torch.is_tensor(mix) else torch.device("cpu")

    def tensor(v):
        return (v if torch.is_tensor(v) else torch.as_tensor(np.asarray(v))).detach().to(device=dev, dtype=dtype)

    run = Run()
    w = {}
    for k, v in weights.items():
        if k.endswith("num_batches_tracked"):
            continue
        t = v if leaves else tensor(v).clone()
        if not k.endswith(("running_mean", "running_var")):
            if not leaves:
                t.requires_grad_(True)
            run.params[k] = t
        w[k] = t
    mix, e1, e2 = tensor(mix), tensor(e1), tensor(e2)
    B, F, W = mix.shape
    E = e1.shape[2]
    def shell(name, make):
        if modules is None:
            return make().to(device=dev, dtype=dtype)
        if name not in modules:
            modules[name] = make().to(device=dev, dtype=dtype)
        return modules[name]

    gru = shell("gru", lambda: torch.nn.GRU(E, F, num_layers=2, bidirectional=True, batch_first=True))
    gru_w = {k[4:]: v for k, v in w.items() if k.startswith("gru.")}
    dvecs = [F_.linear(torch.func.functional_call(gru, gru_w, (e,))[0][:, -1, :], w["fc_dvector.weight"], w["fc_dvector.bias"])
             for e in (e1, e2)]
    x = mix.unsqueeze(1)
    for l, (ci, bi, cout, cin, kh, kw, dil) in enumerate(CNN):
        z = F_.conv2d(x, w[f"cnn_layers.{ci}.weight"], w[f"cnn_layers.{ci}.bias"], 1, ((kh // 2) * dil, kw // 2), (dil, 1))
        run.Z.append(z)
        run.stats.append((z.mean((0, 2, 3)), z.var((0, 2, 3), unbiased=True)))
        p = f"cnn_layers.{bi}."
        x = _PlainGrad.apply(F_.batch_norm(z, None, None, w[p + "weight"], w[p + "bias"], True, MOMENTUM, BN_EPS))
        if l < 7:
            x = _relu(x, None if relu_masks is None else relu_masks["cnn"][l])
        run.act.append(x)
    x = x.permute(0, 3, 2, 1).contiguous().view(B, 8 * F, W)
    wih, whh = w["lstm.weight_ih_l0"], w["lstm.weight_hh_l0"]
    bias = w["lstm.bias_ih_l0"] + w["lstm.bias_hh_l0"]
    outs, gates, cells, hs, fc1s = [], [], [], [], []
    for s, dv in enumerate(dvecs):
        cat = torch.cat((x, dv.unsqueeze(-1).expand(-1, -1, W)), dim=1).transpose(1, 2)        # (B, W, 9F)
        if stock_lstm:
            lstm = shell("lstm", lambda: torch.nn.LSTM(9 * F, HIDDEN, batch_first=True))
            h = torch.func.functional_call(lstm, {k[5:]: v for k, v in w.items() if k.startswith("lstm.")}, (cat,))[0]
            hs.append(h);  gates.append(h);  cells.append(h)                                   # no taps on this path
        else:
            gin = F_.linear(cat, wih, bias)
            h = torch.zeros(B, HIDDEN, dtype=dtype, device=dev)
            c = torch.zeros(B, HIDDEN, dtype=dtype, device=dev)
            hh, gg, cc = [], [], []
            for t in range(W):
                a = gin[:, t] + F_.linear(h, whh)
                i, f, g, o = a.split(HIDDEN, dim=1)
                i, f, g, o = torch.sigmoid(i), torch.sigmoid(f), torch.tanh(g), torch.sigmoid(o)
                c = f * c + i * g
                h = o * torch.tanh(c)
                hh.append(h);  gg.append(torch.cat((i, f, g, o), dim=1));  cc.append(c)
            h = torch.stack(hh, dim=1)                                                         # (B, W, 400)
            hs.append(h);  gates.append(torch.stack(gg, dim=1));  cells.append(torch.stack(cc, dim=1))
        rows = slice(s * B, (s + 1) * B)
        y = F_.linear(_relu(h, None if relu_masks is None else relu_masks["lstm"][rows]), w["fc.1.weight"], w["fc.1.bias"])
        fc1s.append(y)
        if keep is not None:     # Dropout2d on (B, W, 600): whole frames
            y = y * (torch.as_tensor(keep)[rows].to(device=dev, dtype=dtype) / (1.0 - P_DROP)).unsqueeze(-1)
        y = _relu(y, None if relu_masks is None else relu_masks["fc1"][rows])
        mask = torch.sigmoid(F_.linear(y, w["fc.4.weight"], w["fc.4.bias"])).transpose(1, 2)
        outs.append(mask * mix)
    run.out1, run.out2 = outs
    run.h, run.gates, run.cell, run.fc1 = (torch.cat(v, dim=0) for v in (hs, gates, cells, fc1s))
    return run
