"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_convtasnet_train.py and
tests/test_gpu_deepconvtasnet_train.py (as tests/ctasnet_memsafety_child.py is for the inference forward), covering
<model>_train_forward and <model>_train_backward for model cttrain (Conv-TasNet) or dcttrain (DeepConvTasNet).  One mode per
process:

mode  poison       the workspace, gradients and outputs the engine allocates start filled with 0xFF bytes
      guard_end    every buffer (weights, inputs, upstream gradients, workspace, gradients, outputs) ENDS flush against an
                   unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

The call sequence (a big batch, then smaller shapes on the cached workspace) runs under test first, then with plain
zero-filled buffers; predictions and gradients must be bit-identical (fixed reduction order everywhere).

    python -m tests.ctasnet_train_memsafety_child <mode> <model>
"""
from __future__ import annotations

import functools
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from oracle.convtasnet_stock import synthetic_convtasnet_weights  # noqa: E402
from speech_separation_amd.engine import ConvTasNetTrainEngine, DeepConvTasNetTrainEngine  # noqa: E402
from speech_separation_amd.spec import DPTN_AUDIO, synthetic_inputs  # noqa: E402
from tests.ctasnet_memsafety_child import main  # noqa: E402  (the mode harness)
from tests.deepconvtasnet_ref import synthetic_deepconvtasnet_weights  # noqa: E402

SHAPES = [(3, 4001), (1, 400), (2, 17)]
#: model -> (engine, its synthetic weights)
MODELS = {"cttrain": (ConvTasNetTrainEngine, lambda: synthetic_convtasnet_weights(seed=3)),
          "dcttrain": (DeepConvTasNetTrainEngine, lambda: synthetic_deepconvtasnet_weights(False, seed=3, slopes="distinct"))}


def run(model, dev, alloc, place):
    engine, weights = MODELS[model]
    eng = engine(dev, alloc=alloc)
    sd = weights()
    eng.bind({k: place(torch.from_numpy(v)) for k, v in sd.items()})
    eng.bind_grads()
    res = {}
    for B, T in SHAPES:
        mix = place(torch.from_numpy(synthetic_inputs(DPTN_AUDIO, B=B, T=T, seed=B * 7 + T)["mix"]))
        s1, s2, tape = eng.train_forward(mix)
        g = torch.Generator().manual_seed(B * 11 + T)
        L = eng.out_len(T)
        d1, d2 = (place(torch.randn(B, L, generator=g)) for _ in range(2))
        eng.train_backward(mix, d1, d2, tape)
        torch.cuda.synchronize()
        res[f"{B}x{T}.s1"], res[f"{B}x{T}.s2"] = s1.cpu().numpy(), s2.cpu().numpy()
        res[f"{B}x{T}.grad"] = eng._grads_flat.cpu().numpy()
    eng.close()
    return res


if __name__ == "__main__":
    rc = main(sys.argv[1], sys.argv[2], functools.partial(run, sys.argv[2]))
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
