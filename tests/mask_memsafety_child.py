"""TEST INFRASTRUCTURE: the memory-safety child of tests/memsafety_child.py for the masked DPTN separator (DPTNEncDec):
the same modes and the same call sequence (forward big batch then small, stage entry points, training step with and
without option deterministic, path-level training entry points), on a 2-block model/dptn.yaml configuration.

    python -m tests.mask_memsafety_child <mode> <variant>
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from speech_separation_amd.spec import DPTN_MASK  # noqa: E402
from tests import memsafety_child as M  # noqa: E402

# name -> (config, options, big batch, T, Tv, train batch), as memsafety_child.VARIANTS
VARIANTS = {
    "mask64": (M._cfg(DPTN_MASK, num_blocks=2), {}, 5, 8000, 1, 3),
    "mask128": (M._cfg(DPTN_MASK, num_blocks=1, num_features=128, hidden_video=128), {}, 3, 6000, 1, 2),
}

if __name__ == "__main__":
    M.VARIANTS.update(VARIANTS)
    rc = M.main(sys.argv[1], sys.argv[2])
    sys.stdout.flush()
    os._exit(rc)      # as memsafety_child: no interpreter teardown with guard mappings still referenced by tensors
