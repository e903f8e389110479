"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_specfe_memsafety.py (as tests/wavmetric_memsafety_child.py
is for the evaluation metrics).  One mode per process:

mode  poison       outputs start filled with 0xFF bytes
      guard_end    every buffer (inputs and outputs) ENDS flush against an unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page

The five entry points of include/specfe.h run through the C ABI at (n_fft, hop, B, T) = (256, 128, 1, 129),
(256, 128, 17, 2048) and (400, 200, 2, 1000) -- rows after the first are 4-byte aligned only; the inverse and its adjoint
at the natural length and at one that reads into the last half window; log-mel on the (400, 200) handle --, under test
first, then with plain zero-filled buffers: every output element must have been written (no 0xFF pattern left) and the
results must be bit-identical.

    python -m tests.specfe_memsafety_child <mode>
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

SHAPES = [(256, 128, 1, 129), (256, 128, 17, 2048), (400, 200, 2, 1000)]
N_MELS = 128


def say(msg):
    print(msg, flush=True)


def run(dev, alloc, place):
    """`alloc(nbytes, align)` -> uint8 device tensor, `place(host tensor)` -> device copy: where every buffer of the calls
    lives.  Every buffer asks for 4-byte alignment, so that each is EXACTLY flush with its guard."""
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    for N, H, B, T in SHAPES:
        M, F = 1 + T // H, N // 2 + 1
        g = torch.Generator().manual_seed(N + T)
        x, X = place(torch.randn(B, T, generator=g)), place(torch.randn(B, 2, M, F, generator=g))
        h = ctypes.c_void_p()
        rc = lib.specfe_create_mel(N, H, 16000, N_MELS, ctypes.byref(h)) if N == 400 else lib.specfe_create(N, H, ctypes.byref(h))
        assert rc == 0, lib.specfe_strerror(rc)
        tag = f"{N}.{H}.{B}x{T}"

        def call(name, fn, numel, *args):
            out = alloc(4 * numel, 4).view(torch.float32)
            say(f"BEGIN {name} {tag}")
            rc = fn(h, *args, out.data_ptr(), stream)
            assert rc == 0, lib.specfe_strerror(rc)
            torch.cuda.synchronize()
            res[f"{name}.{tag}"] = out.cpu().numpy()

        call("stft", lib.specfe_stft, B * 2 * M * F, x.data_ptr(), B, T)
        call("stft_backward", lib.specfe_stft_backward, B * T, X.data_ptr(), B, T)
        for L in ((M - 1) * H, (M - 1) * H + N // 2 + 10):
            gy = place(torch.randn(B, L, generator=g))
            call(f"istft{L}", lib.specfe_istft, B * L, X.data_ptr(), B, M, L)
            call(f"istft_backward{L}", lib.specfe_istft_backward, B * 2 * M * F, gy.data_ptr(), B, M, L)
        if N == 400:
            call("logmel", lib.specfe_logmel, B * N_MELS * M, x.data_ptr(), B, T)
        lib.specfe_destroy(h)
    return res


def main(mode):
    dev = torch.device("cuda:0")
    arena = None
    say(f"== {mode} specfe: run under test")
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
    say(f"== {mode} specfe: plain run")
    want = run(dev, lambda n, align: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev))
    bad = []
    for k in want:
        if not (np.all(np.isfinite(got[k])) and np.array_equal(got[k], want[k])):          # 0xFF.. is NaN
            bad.append(k)
            say(f"MISMATCH {k}: {got[k].ravel()[:8]} vs {want[k].ravel()[:8]}")
    if bad:
        return 1
    say(f"OK {mode} specfe")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
