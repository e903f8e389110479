"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_wavloss_memsafety.py (as tests/ctasnet_memsafety_child.py
is for Conv-TasNet).  One mode per process:

mode  poison       outputs and scratch start filled with 0xFF bytes
      guard_end    every buffer (inputs, gradients, loss_out, perm_out, scratch) ENDS flush against an unmapped page
                   (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

wavloss_pit_loss runs through the C ABI for every kind and level at (3, 1025) -- rows after the first are 4-byte aligned
only -- and (2, 1), under test first, then with plain zero-filled buffers; the results must be bit-identical.

    python -m tests.wavloss_memsafety_child <mode>
"""
from __future__ import annotations

import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from speech_separation_amd import _lib  # noqa: E402
from tests.wavloss_ref import make_case  # noqa: E402

SHAPES = [(3, 1025), (2, 1)]


def say(msg):
    print(msg, flush=True)


def run(dev, alloc, place):
    """`alloc(nbytes, align)` -> uint8 device tensor, `place(host tensor)` -> device copy: where every buffer of the calls
    lives.  Float buffers ask for 4-byte alignment and the scratch for 8, so that each is EXACTLY flush with its guard."""
    lib = _lib.load()
    res = {}
    for B, T in SHAPES:
        inp = [place(torch.from_numpy(a)) for a in make_case(B, T, seed=B * 7 + T, swapped=(1,))]
        for kind in range(3 if T >= 2 else 2):
            for level in range(2):
                d1, d2 = (alloc(4 * B * T, 4).view(torch.float32).view(B, T) for _ in range(2))
                out = alloc(16, 4).view(torch.float32)
                perm = alloc(4 * B, 4).view(torch.int32)
                ws = alloc(int(lib.wavloss_scratch_bytes(B)), 8)
                say(f"BEGIN kind {kind} level {level} {B}x{T}")
                rc = lib.wavloss_pit_loss(kind, level, *[t.data_ptr() for t in inp], B, T, 1.0, d1.data_ptr(), d2.data_ptr(),
                                          out.data_ptr(), perm.data_ptr(), ws.data_ptr(), ws.numel(),
                                          torch.cuda.current_stream(dev).cuda_stream)
                assert rc == 0, lib.wavloss_strerror(rc)
                torch.cuda.synchronize()
                key = f"{kind}.{level}.{B}x{T}"
                res[key + ".d1"], res[key + ".d2"] = d1.cpu().numpy(), d2.cpu().numpy()
                res[key + ".out"], res[key + ".perm"] = out.cpu().numpy(), perm.cpu().numpy().astype("float32")
    return res


def main(mode):
    dev = torch.device("cuda:0")
    arena = None
    say(f"== {mode} wavloss: run under test")
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
        say(f"guard arena: {len(arena.handles)} allocations, {arena.total / 2**10:.1f} KiB")
        arena.close()
    say(f"== {mode} wavloss: plain run")
    want = run(dev, lambda n, align: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    bad = [k for k in want if not (np.all(np.isfinite(got[k])) and np.array_equal(got[k], want[k]))]
    for k in bad:
        say(f"MISMATCH {k}")
    if bad:
        return 1
    say(f"OK {mode} wavloss")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
