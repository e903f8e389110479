"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_voicefilter_memsafety.py (as
tests/lipreader_memsafety_child.py is for the lip reader).  One mode per process:

mode  poison       outputs and workspace start filled with 0xFF bytes
      guard_end    every buffer (inputs, outputs, workspace, each bound weight) ENDS flush against an unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

vfilt_forward (74 bound tensors) runs through the C ABI at (input_size, W, Tv, B) = (17, 7, 1, 3) -- F below the reach of
dilations 8 and 16, W below the 7-tap width, one video frame --, (33, 50, 3, 1), (257, 7, 2, 1) -- the end of the range -- and (16, 8, 2, 8) -- exactly 1024 positions,
16 sequences --, under test first, then with plain
zero-filled buffers: every output element must have been written (no 0xFF pattern left) and the results must be
bit-identical.

    python -m tests.voicefilter_memsafety_child <mode>
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
from tests import voicefilter_ref as R  # noqa: E402

SHAPES = [(17, 7, 1, 3), (33, 50, 3, 1), (257, 7, 2, 1), (16, 8, 2, 8)]
EMBED = 1024


def say(msg):
    print(msg, flush=True)


def run(dev, alloc, place):
    """`alloc(nbytes, align)` -> uint8 device tensor, `place(host tensor)` -> device copy: where every buffer of the calls
    lives.  Float buffers ask for 4-byte alignment and the workspace for 256, so that each is EXACTLY flush with its guard."""
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    for F, W, Tv, B in SHAPES:
        h = ctypes.c_void_p()
        rc = lib.vfilt_create(ctypes.byref(h), F, EMBED)
        assert rc == 0, lib.vfilt_last_error(None)
        sd = R.synthetic_voicefilter_weights(F, EMBED, 0)
        n = lib.vfilt_num_weights(h)
        names = [lib.vfilt_weight_name(h, i).decode() for i in range(n)]
        assert n == 74 and names == [k for k in sd if not k.endswith("num_batches_tracked")]
        weights = [place(torch.from_numpy(sd[k]).reshape(-1)) for k in names]
        for i, t in enumerate(weights):
            assert t.numel() == lib.vfilt_weight_numel(h, i), names[i]
        ptrs = (ctypes.c_void_p * n)(*[t.data_ptr() for t in weights])
        rc = lib.vfilt_bind_weights(h, ptrs, n)
        assert rc == 0, lib.vfilt_last_error(h)
        mix, e1, e2 = (place(torch.from_numpy(a).reshape(-1)) for a in R.synthetic_inputs(F, W, Tv, B, EMBED, seed=F))
        need = int(lib.vfilt_workspace_bytes(h, B, W, Tv))
        assert need > 0 and need % 256 == 0
        out1 = alloc(4 * B * F * W, 4).view(torch.float32)
        out2 = alloc(4 * B * F * W, 4).view(torch.float32)
        ws = alloc(need, 256)
        say(f"BEGIN {F}x{W}x{Tv}x{B} workspace {need}")
        rc = lib.vfilt_forward(h, mix.data_ptr(), e1.data_ptr(), e2.data_ptr(), B, W, Tv, out1.data_ptr(), out2.data_ptr(),
                               ws.data_ptr(), need, stream)
        assert rc == 0, lib.vfilt_last_error(h)
        torch.cuda.synchronize()
        res[f"s1.{F}x{W}x{Tv}x{B}"] = out1.cpu().numpy()
        res[f"s2.{F}x{W}x{Tv}x{B}"] = out2.cpu().numpy()
        lib.vfilt_destroy(h)
    return res


def main(mode):
    dev = torch.device("cuda:0")
    arena = None
    say(f"== {mode} vfilt: run under test")
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
    say(f"== {mode} vfilt: plain run")
    want = run(dev, lambda n, align: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    bad = []
    for k in want:
        if not (np.all(np.isfinite(got[k])) and np.array_equal(got[k], want[k])):     # 0xFF.. is NaN
            bad.append(k)
            say(f"MISMATCH {k}: {got[k].ravel()[:8]} vs {want[k].ravel()[:8]}")
    if bad:
        return 1
    say(f"OK {mode} vfilt")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
