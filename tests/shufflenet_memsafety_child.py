"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_shufflenet_lipreader_memsafety.py (as
tests/lipreader_memsafety_child.py is for the ResNet-18 lip reader).  One mode per process:

mode  poison       output and workspace start filled with 0xFF bytes
      guard_end    every buffer (input, output, workspace, each bound weight) ENDS flush against an unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

lipsn_forward (PReLU form, width 1.0: 281 bound tensors) runs through the C ABI at (S, T, H, W) = (1, 2, 65, 72) and
(2, 1, 88, 88), plain and as a window at (4, 4) of a frame 9 rows and 8 columns larger with the reference's affine -- under test first,
then with plain zero-filled buffers: every output element must have been written (no 0xFF pattern left) and the results
must be bit-identical.

    python -m tests.shufflenet_memsafety_child <mode>
"""
from __future__ import annotations

import ctypes
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from speech_separation_amd import _lib  # noqa: E402
from tests import shufflenet_ref as R  # noqa: E402

SHAPES = [(1, 2, 65, 72), (2, 1, 88, 88)]
AFFINE = (1.0 / (255.0 * 0.165), -0.421 / 0.165)


def say(msg):
    print(msg, flush=True)


def run(dev, alloc, place):
    """`alloc(nbytes, align)` -> uint8 device tensor, `place(host tensor)` -> device copy: where every buffer of the calls
    lives.  Float buffers ask for 4-byte alignment and the workspace for 256, so that each is EXACTLY flush with its guard."""
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    h = ctypes.c_void_p()
    rc = lib.lipsn_create(ctypes.byref(h), 1, 2)
    assert rc == 0, lib.lipsn_last_error(None)
    sd = R.synthetic_shufflenet_weights("prelu", 1.0, 0)
    n = lib.lipsn_num_weights(h)
    names = [lib.lipsn_weight_name(h, i).decode() for i in range(n)]
    assert names == [k for k in sd if not k.endswith("num_batches_tracked")]
    weights = [place(torch.from_numpy(sd[k]).reshape(-1)) for k in names]
    for i, t in enumerate(weights):
        assert t.numel() == lib.lipsn_weight_numel(h, i), names[i]
    ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in weights])
    rc = lib.lipsn_bind_weights(h, ptrs, n)
    assert rc == 0, lib.lipsn_last_error(h)
    res = {}
    for S, T, H, W in SHAPES:
        for form in ("plain", "window"):
            if form == "plain":
                Hin, Win, y0, x0, a, b = H, W, 0, 0, 1.0, 0.0
                x = R.synthetic_video((S, T, Hin, Win), seed=S + H)
            else:
                Hin, Win, y0, x0, (a, b) = H + 9, W + 8, 4, 4, AFFINE
                x = R.synthetic_clip((S, T, Hin, Win), seed=S + H)
            xd = place(torch.from_numpy(x).reshape(-1))
            need = int(lib.lipsn_workspace_bytes(h, S, T, H, W))
            assert need > 0 and need % 256 == 0
            out = alloc(4 * S * T * 1024, 4).view(torch.float32)
            ws = alloc(need, 256)
            say(f"BEGIN {form} {S}x{T}x{H}x{W} workspace {need}")
            rc = lib.lipsn_forward(h, xd.data_ptr(), S, T, Hin, Win, y0, x0, H, W, a, b, out.data_ptr(), ws.data_ptr(), need,
                                   stream)
            assert rc == 0, lib.lipsn_last_error(h)
            torch.cuda.synchronize()
            res[f"{form}.{S}x{T}x{H}x{W}"] = out.cpu().numpy()
    lib.lipsn_destroy(h)
    return res


def main(mode):
    dev = torch.device("cuda:0")
    arena = None
    say(f"== {mode} lipsn: run under test")
    if mode == "poison":
        got = run(dev, lambda n, align: torch.full((n,), 0xFF, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    elif mode in ("guard_end", "guard_start"):
        from tests.guardmem import GuardArena
        arena = GuardArena(0, flush="end" if mode == "guard_end" else "start", fill=0xFF)
        got = run(dev, arena.bytes, lambda t: arena.like(t.contiguous(), align=4))
    else:
        raise SystemExit(f"unknown mode {mode}")
    torch.cuda.synchronize()
    if arena is not None:
        say(f"guard arena: {len(arena.handles)} allocations, {arena.total / 2**20:.1f} MiB")
        arena.close()
    say(f"== {mode} lipsn: plain run")
    want = run(dev, lambda n, align: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    bad = []
    for k in want:
        if not (np.all(np.isfinite(got[k])) and np.array_equal(got[k], want[k])):     # 0xFF.. is NaN
            bad.append(k)
            say(f"MISMATCH {k}: {got[k].ravel()[:8]} vs {want[k].ravel()[:8]}")
    if bad:
        return 1
    say(f"OK {mode} lipsn")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
