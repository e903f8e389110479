"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_wavmetric_memsafety.py (as tests/wavloss_memsafety_child.py
is for the waveform criteria).  One mode per process:

mode  poison       outputs and scratch start filled with 0xFF bytes
      guard_end    every buffer (inputs, out, kept, scratch) ENDS flush against an unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

wavmetric_stoi_pairs (STOI and ESTOI) and wavmetric_sisdr_pairs run through the C ABI at (8000, 2, 6000) and
(16000, 3, 12003) -- rows after the first are 4-byte aligned only --, under test first, then with plain zero-filled
buffers: every element of out and kept must have been written (no 0xFF pattern left) and the results must be
bit-identical.

    python -m tests.wavmetric_memsafety_child <mode>
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
from tests.stoi_ref import make_batch  # noqa: E402

SHAPES = [(8000, 2, 6000), (16000, 3, 12003)]


def say(msg):
    print(msg, flush=True)


def run(dev, alloc, place):
    """`alloc(nbytes, align)` -> uint8 device tensor, `place(host tensor)` -> device copy: where every buffer of the calls
    lives.  Float and int buffers ask for 4-byte alignment and the scratch for 16, so that each is EXACTLY flush with its
    guard."""
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    for fs, B, T in SHAPES:
        inp = [place(torch.from_numpy(a)) for a in make_batch(fs, B, T, seed=fs // 1000 + B)]
        ptrs = [t.data_ptr() for t in inp]
        out = alloc(16 * B, 4).view(torch.float32)
        say(f"BEGIN sisdr {fs} {B}x{T}")
        rc = lib.wavmetric_sisdr_pairs(*ptrs, B, T, out.data_ptr(), stream)
        assert rc == 0, lib.wavmetric_strerror(rc)
        torch.cuda.synchronize()
        res[f"sisdr.{fs}.{B}x{T}"] = out.cpu().numpy()
        for ext in (0, 1):
            h = ctypes.c_void_p()
            rc = lib.wavmetric_stoi_create(fs, ext, ctypes.byref(h))
            assert rc == 0, lib.wavmetric_strerror(rc)
            need = int(lib.wavmetric_stoi_scratch_bytes(h, B, T))
            assert need > 0 and need % 16 == 0
            out = alloc(16 * B, 4).view(torch.float32)
            kept = alloc(8 * B, 4).view(torch.int32)
            ws = alloc(need, 16)
            say(f"BEGIN stoi extended {ext} {fs} {B}x{T} scratch {need}")
            rc = lib.wavmetric_stoi_pairs(h, *ptrs, B, T, out.data_ptr(), kept.data_ptr(), ws.data_ptr(), need, stream)
            assert rc == 0, lib.wavmetric_strerror(rc)
            torch.cuda.synchronize()
            key = f"stoi{ext}.{fs}.{B}x{T}"
            res[key + ".out"], res[key + ".kept"] = out.cpu().numpy(), kept.cpu().numpy()
            lib.wavmetric_stoi_destroy(h)
    return res


def main(mode):
    dev = torch.device("cuda:0")
    arena = None
    say(f"== {mode} wavmetric: run under test")
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
    say(f"== {mode} wavmetric: plain run")
    want = run(dev, lambda n, align: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    bad = []
    for k in want:
        written = np.all(np.isfinite(got[k])) if got[k].dtype == np.float32 else np.all(got[k] >= 0)   # 0xFF.. is NaN / -1
        if not (written and np.array_equal(got[k], want[k])):
            bad.append(k)
            say(f"MISMATCH {k}: {got[k].ravel()[:8]} vs {want[k].ravel()[:8]}")
    if bad:
        return 1
    say(f"OK {mode} wavmetric")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
