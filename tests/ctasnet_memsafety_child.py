"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_convtasnet.py (as tests/mask_memsafety_child.py is for
DPTNEncDec).  One mode per process:

mode  poison       the workspace and the outputs the engine allocates start filled with 0xFF bytes
      guard_end    every buffer (weights, inputs, workspace, outputs) ENDS flush against an unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

The call sequence (a big batch, then smaller shapes on the cached workspace) runs under test first, then with plain
zero-filled buffers; the results must be bit-identical (the forward has a fixed reduction order).

    python -m tests.ctasnet_memsafety_child <mode>
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from oracle.convtasnet_stock import synthetic_convtasnet_weights  # noqa: E402
from speech_separation_amd.engine import ConvTasNetEngine  # noqa: E402
from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs  # noqa: E402

SHAPES = [(3, 4001), (1, 400), (2, 17), (2, 8000)]


def say(msg):
    print(msg, flush=True)


def run(dev, alloc, place):
    eng = ConvTasNetEngine(dev, alloc=alloc)
    sd = synthetic_convtasnet_weights(seed=3)
    eng.bind({k: place(torch.from_numpy(v)) for k, v in sd.items()})
    res = {}
    for B, T in SHAPES:
        mix = place(torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=B * 7 + T)["mix"]))
        s1, s2 = eng.forward(mix)
        torch.cuda.synchronize()
        res[f"{B}x{T}.s1"], res[f"{B}x{T}.s2"] = s1.cpu().numpy(), s2.cpu().numpy()
    eng.close()
    return res


def main(mode, label="convtasnet", run=run):
    """`run(dev, alloc, place) -> {name: array}` under `mode`, then plainly; 0 if every array is finite and bit-identical.
    tests/deepctasnet_memsafety_child.py and tests/ctasnet_train_memsafety_child.py pass their own label and run."""
    dev = torch.device("cuda:0")
    arena = None
    say(f"== {mode} {label}: run under test")
    if mode == "poison":
        got = run(dev, lambda n: torch.full((n,), 0xFF, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    elif mode in ("guard_end", "guard_start"):
        from tests.guardmem import GuardArena
        arena = GuardArena(0, flush="end" if mode == "guard_end" else "start", fill=0xFF)
        got = run(dev, lambda n: arena.bytes(n, 256), lambda t: arena.like(t.contiguous()))
    else:
        raise SystemExit(f"unknown mode {mode}")
    torch.cuda.synchronize()
    if arena is not None:
        say(f"guard arena: {len(arena.handles)} allocations, {arena.total / 2**20:.1f} MiB")
        arena.close()
    torch.cuda.empty_cache()
    say(f"== {mode} {label}: plain run")
    want = run(dev, lambda n: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    bad = [k for k in want if not (np.all(np.isfinite(got[k])) and np.array_equal(got[k], want[k]))]
    for k in bad:
        say(f"MISMATCH {k}")
    if bad:
        return 1
    say(f"OK {mode} {label}")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
