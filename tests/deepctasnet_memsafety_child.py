"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_deepconvtasnet.py (as tests/ctasnet_memsafety_child.py is
for ConvTasNet).  One mode per process:

mode  poison       the workspace and the outputs the engine allocates start filled with 0xFF bytes
      guard_end    every buffer (weights, inputs, workspace, outputs) ENDS flush against an unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

Both models run a call sequence (a big batch, then smaller shapes on the cached workspace; for the audio-visual one Tv
below, equal to and above F) under test first, then with plain zero-filled buffers; the results must be bit-identical.

    python -m tests.deepctasnet_memsafety_child <mode>
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from speech_separation_amd.engine import DeepConvTasNetEngine  # noqa: E402
from speech_separation_amd.spec import DPTN_AV, synthetic_inputs  # noqa: E402
from tests.deepconvtasnet_ref import synthetic_deepconvtasnet_weights  # noqa: E402
from tests.ctasnet_memsafety_child import main  # noqa: E402  (the mode harness)

SHAPES = [(3, 4001, 50), (1, 400, 1), (2, 17, 7), (2, 400, 50)]


def run(dev, alloc, place):
    res = {}
    for av in (False, True):
        eng = DeepConvTasNetEngine(dev, av=av, alloc=alloc)
        sd = synthetic_deepconvtasnet_weights(av, seed=3)
        eng.bind({k: place(torch.from_numpy(v)) for k, v in sd.items()})
        for B, T, Tv in SHAPES:
            inp = synthetic_inputs(DPTN_AV, B=B, T=T, Tv=Tv, seed=B * 7 + T)
            emb = [place(torch.from_numpy(inp[k])) for k in ("s1_embedding", "s2_embedding")] if av else [None, None]
            s1, s2 = eng.forward(place(torch.from_numpy(inp["mix"])), *emb)
            torch.cuda.synchronize()
            res[f"{int(av)}.{B}x{T}x{Tv}.s1"], res[f"{int(av)}.{B}x{T}x{Tv}.s2"] = s1.cpu().numpy(), s2.cpu().numpy()
        eng.close()
    return res


if __name__ == "__main__":
    rc = main(sys.argv[1], "deepconvtasnet", run)
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
