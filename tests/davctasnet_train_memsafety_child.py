"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_deepavconvtasnet_train.py, covering davtrain_train_forward
and davtrain_train_backward (DeepAVConvTasNet) with the mode harness of tests/ctasnet_memsafety_child.main -- the same three
modes as tests/ctasnet_train_memsafety_child.py, one per process:

mode  poison       the workspace, gradients and outputs the engine allocates start filled with 0xFF bytes
      guard_end    every buffer (weights, mixture, both embeddings, upstream gradients, workspace, gradients, outputs) ENDS
                   flush against an unmapped page (tests/guardmem); vcat is the last region of the workspace, so its end
                   is the workspace's
      guard_start  every buffer STARTS flush against an unmapped page

The shapes cover Tv = 1, Tv > F, a Tv that is no multiple of the Linear kernels' frame tiles, and Tv = F.

    python -m tests.davctasnet_train_memsafety_child <mode>
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from speech_separation_amd.engine import DeepAVConvTasNetTrainEngine  # noqa: E402
from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs  # noqa: E402
from tests.ctasnet_memsafety_child import main  # noqa: E402  (the mode harness)
from tests.deepavconvtasnet_train_ref import synthetic_embeddings, synthetic_weights  # noqa: E402

SHAPES = [(3, 4001, 50), (1, 400, 50), (2, 17, 1), (2, 1104, 71)]


def run(dev, alloc, place):
    eng = DeepAVConvTasNetTrainEngine(dev, alloc=alloc)
    eng.bind({k: place(torch.from_numpy(v)) for k, v in synthetic_weights(seed=3).items()})
    eng.bind_grads()
    res = {}
    for B, T, Tv in SHAPES:
        mix = place(torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=B * 7 + T)["mix"]))
        e1, e2 = (place(torch.from_numpy(e)) for e in synthetic_embeddings(B, Tv, seed=T))
        s1, s2, tape = eng.train_forward(mix, e1, e2)
        g = torch.Generator().manual_seed(B * 11 + T)
        L = eng.out_len(T)
        d1, d2 = (place(torch.randn(B, L, generator=g)) for _ in range(2))
        eng.train_backward(mix, e1, e2, d1, d2, tape)
        torch.cuda.synchronize()
        tag = f"{B}x{T}x{Tv}"
        res[tag + ".s1"], res[tag + ".s2"] = s1.cpu().numpy(), s2.cpu().numpy()
        res[tag + ".grad"] = eng._grads_flat.cpu().numpy()
        res[tag + ".vcat"] = eng.tape_tensor(tape, eng.TAPE_VCAT).cpu().numpy()
    eng.close()
    return res


if __name__ == "__main__":
    rc = main(sys.argv[1], "davtrain", run)
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
