"""TEST INFRASTRUCTURE: the memory-safety child of tests/test_gpu_vf_wave_memsafety.py (as tests/specfe_memsafety_child.py
is for the spectral front end).  One (mode, variant) per process:

mode  poison       outputs start filled with 0xFF bytes
      guard_end    every buffer (inputs and outputs) ENDS flush against an unmapped page (tests/guardmem)
      guard_start  every buffer STARTS flush against an unmapped page
variant            index into SHAPES: (n_fft, hop, B, T) = (400, 100, 1, 201) or (256, 128, 17, 2048) -- rows after the
                   first are 4-byte aligned only

The two entry points of include/vfwave.h run through the C ABI: the analysis, then the synthesis with n_src = 1 and 2 at
the natural length and at one that reads past the last half window; under test first, then with plain zero-filled
buffers: every output element must have been written (no 0xFF pattern left) and the results must be bit-identical.

    python -m tests.vf_wave_memsafety_child <mode> <variant>
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

SHAPES = [(400, 100, 1, 201), (256, 128, 17, 2048)]


def say(msg):
    print(msg, flush=True)


def run(dev, alloc, place, shape):
    """`alloc(nbytes, align)` -> uint8 device tensor, `place(host tensor)` -> device copy: where every buffer of the calls
    lives.  Every buffer asks for 4-byte alignment, so that each is EXACTLY flush with its guard."""
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    res = {}
    N, H, B, T = shape
    W, F = 1 + T // H, N // 2 + 1
    g = torch.Generator().manual_seed(N + T)
    x = place(torch.randn(B, T, generator=g))
    pred = place(torch.rand(2, B, F, W, generator=g) * 2.0 - 0.5)
    angle = torch.rand(B, F, W, generator=g) * 6.283
    phasor = place(torch.stack([torch.cos(angle), torch.sin(angle)], dim=1))
    h = ctypes.c_void_p()
    rc = lib.specfe_create(N, H, ctypes.byref(h))
    assert rc == 0, lib.specfe_strerror(rc)
    tag = f"{N}.{H}.{B}x{T}"
    spec, ph = alloc(4 * B * F * W, 4).view(torch.float32), alloc(4 * B * 2 * F * W, 4).view(torch.float32)
    say(f"BEGIN analysis {tag}")
    rc = lib.vfwave_analysis(h, x.data_ptr(), B, T, spec.data_ptr(), ph.data_ptr(), stream)
    assert rc == 0, lib.vfwave_strerror(rc)
    torch.cuda.synchronize()
    res[f"spec.{tag}"], res[f"phasor.{tag}"] = spec.cpu().numpy(), ph.cpu().numpy()
    for n_src in (1, 2):
        for L in ((W - 1) * H, (W - 1) * H + N // 2 + 10):
            y = alloc(4 * n_src * B * L, 4).view(torch.float32)
            p = pred if n_src == 2 else place(pred[:1].cpu())
            say(f"BEGIN synthesis n_src={n_src} length={L} {tag}")
            rc = lib.vfwave_synthesis(h, p.data_ptr(), phasor.data_ptr(), n_src, B, W, L, y.data_ptr(), stream)
            assert rc == 0, lib.vfwave_strerror(rc)
            torch.cuda.synchronize()
            res[f"synthesis{n_src}.{L}.{tag}"] = y.cpu().numpy()
    lib.specfe_destroy(h)
    return res


def main(mode, variant):
    dev = torch.device("cuda:0")
    shape = SHAPES[int(variant)]
    arena = None
    say(f"== {mode} vfwave {variant}: run under test")
    if mode == "poison":
        got = run(dev, lambda n, align: torch.full((n,), 0xFF, dtype=torch.uint8, device=dev), lambda t: t.to(dev), shape)
    elif mode in ("guard_end", "guard_start"):
        from tests.guardmem import GuardArena
        arena = GuardArena(0, flush="end" if mode == "guard_end" else "start", fill=0xFF)
        got = run(dev, arena.bytes, lambda t: arena.like(t.contiguous(), align=4), shape)
    else:
        raise SystemExit(f"unknown mode {mode}")
    torch.cuda.synchronize()
    if arena is not None:
        say(f"guard arena: {len(arena.handles)} allocations, {arena.total / 2**10:.1f} KiB")
        arena.close()
    say(f"== {mode} vfwave {variant}: plain run")
    want = run(dev, lambda n, align: torch.zeros(n, dtype=torch.uint8, device=dev), lambda t: t.to(dev), shape)
    bad = []
    for k in want:
        if not (np.all(np.isfinite(got[k])) and np.array_equal(got[k], want[k])):          # 0xFF.. is NaN
            bad.append(k)
            say(f"MISMATCH {k}: {got[k].ravel()[:8]} vs {want[k].ravel()[:8]}")
    if bad:
        return 1
    say(f"OK {mode} vfwave {variant}")
    return 0


if __name__ == "__main__":
    rc = main(sys.argv[1], sys.argv[2])
    sys.stdout.flush()
    os._exit(rc)      # no interpreter teardown with guard mappings still referenced by tensors
