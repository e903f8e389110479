"""TEST INFRASTRUCTURE: one memory-safety run of the long-sequence training attention (option train_long_seq = 1) in a process
of its own (tests/test_gpu_train_long_memsafety.py spawns it; a GPU memory access fault kills only this child, and its last
"BEGIN ..." line names what was running).  Same modes and allocator as tests/memsafety_child.py:

    python -m tests.train_long_memsafety_child <mode>

mode  poison       every buffer the engine allocates starts as 0xFF bytes instead of zeros
      guard_end    weights, inputs, outputs, workspaces, tapes and per-slot gradient buffers each END flush against an unmapped
                   page (tests/guardmem): an access beyond a buffer is a GPU fault
      guard_start  the same with each buffer STARTING right behind an unmapped page

One variant: chunk 20, step 10, one block, 128 features, B = 2, T = 7744 (S = 257 chunks: nine key blocks with one key in the
last, the last workgroup of a sequence with three of its four waves beyond it), dropout 0.1.  The whole-model training step
(deterministic tile order) and the path-level entry points on the inter-chunk path; the training forward's outputs and every
gradient must be bit-identical to the plain run's.
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from speech_separation_amd.engine import DptnEngine  # noqa: E402
from speech_separation_amd.spec import DPTN_AV, DPTNConfig, synthetic_inputs, synthetic_state_dict  # noqa: E402

CFG = DPTNConfig(**{**DPTN_AV.to_dict(), "num_blocks": 1, "dropout": 0.1, "chunk_size": 20, "step_size": 10})
OPTIONS = {"train_long_seq": 1, "dropout_ppm": 100000, "dropout_seed": 2024, "deterministic": 1}
B, T, TV = 2, 7744, 9


def say(msg):
    print(msg, flush=True)


def run_sequence(eng, inputs, place):
    res = {}
    rng = np.random.default_rng(11)
    d1 = place(torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32)))
    d2 = place(torch.from_numpy(rng.standard_normal((B, T)).astype(np.float32)))
    args = (inputs["mix"], inputs["s1_embedding"], inputs["s2_embedding"])
    say("BEGIN training forward")
    s1, s2, tape = eng.train_forward(*args)
    torch.cuda.synchronize()
    say("BEGIN training backward")
    eng.train_backward(*args, d1, d2, tape)
    torch.cuda.synchronize()
    res["train.s1"], res["train.s2"] = s1.cpu().numpy(), s2.cpu().numpy()
    for k, g in eng._grads.items():
        res[f"train.grad.{k}"] = g.cpu().numpy()
    del tape
    S = eng.chunks(T)
    assert S == 257
    rng = np.random.default_rng(12)
    x = place(torch.from_numpy(rng.standard_normal((B, S, CFG.chunk_size, CFG.num_features)).astype(np.float32)))
    dy = place(torch.from_numpy(rng.standard_normal((B, S, CFG.chunk_size, CFG.num_features)).astype(np.float32)))
    say("BEGIN path-level training forward (inter-chunk)")
    y, tape = eng.train_path_forward(0, 1, x)
    torch.cuda.synchronize()
    say("BEGIN path-level training backward (inter-chunk)")
    dx = eng.train_path_backward(0, 1, x, dy, tape)
    torch.cuda.synchronize()
    res["path1.y"], res["path1.dx"] = y.cpu().numpy(), dx.cpu().numpy()
    for k, g in eng._grads.items():
        res[f"path1.grad.{k}"] = g.cpu().numpy()
    return res


def main(mode):
    dev = torch.device("cuda:0")
    sd = synthetic_state_dict(CFG, seed=5)
    host_inputs = synthetic_inputs(CFG, B=B, T=T, Tv=TV, seed=79)

    def make(alloc, place, per_slot):
        eng = DptnEngine(CFG, dev, alloc=alloc)
        eng.bind({k: place(torch.from_numpy(v)) for k, v in sd.items()})
        eng.bind_grads(per_slot=per_slot)
        for k, v in OPTIONS.items():
            eng.set_option(k, v)
        return eng, {k: place(torch.from_numpy(v)) for k, v in host_inputs.items() if k in ("mix", "s1_embedding", "s2_embedding")}

    def plain_run():
        say(f"== {mode}: plain run")
        eng, inputs = make(lambda n: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev), False)
        res = run_sequence(eng, inputs, lambda t: t.to(dev))
        eng.close()
        del eng, inputs
        torch.cuda.empty_cache()
        return res

    def run_under_test():
        say(f"== {mode}: run under test")
        arena = None
        if mode == "poison":
            place = lambda t: t.to(dev)   # noqa: E731
            eng, inputs = make(lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device=dev), place, False)
        else:
            from tests.guardmem import GuardArena
            arena = GuardArena(0, flush="end" if mode == "guard_end" else "start", fill=0xFF)
            place = lambda t: arena.like(t.contiguous())   # noqa: E731
            eng, inputs = make(lambda n: arena.bytes(n, 256), place, True)
        res = run_sequence(eng, inputs, place)
        eng.close()
        del eng, inputs, place
        if arena is not None:
            say(f"guard arena: {len(arena.handles)} allocations, {arena.total / 2**20:.1f} MiB")
            arena.close()
        torch.cuda.empty_cache()
        return res

    got = run_under_test()      # first, as tests/memsafety_child.py: the arena reserves its ranges in a fresh process
    want = plain_run()
    bad = []
    for k in want:
        a, b = want[k], got[k]
        if not np.all(np.isfinite(b)):
            bad.append(f"{k}: non-finite values ({int(np.sum(~np.isfinite(b)))} of {b.size})")
        elif not np.array_equal(a, b):
            bad.append(f"{k}: not bit-identical (max |d| {float(np.abs(a - b).max()):.3e}, {int(np.sum(a != b))} of {a.size} elements)")
    if bad:
        say(f"FAILED {mode}\n  " + "\n  ".join(bad[:40]))
        return 1
    say(f"OK {mode} train_long: {len(want)} results identical")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
