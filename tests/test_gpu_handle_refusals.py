"""The refusals that csrc/handle.h and csrc/lipfront.h serve for the three video-side handles (include/lipfe.h, lipsn.h,
vfilt.h), through the C ABI itself: return code and last_error text of a short, NULL or misaligned pointer table, a forward
before any bind, a workspace that is short or misaligned and, for the two lip readers, a window that leaves the frame.
Nothing is launched: every call is refused before its first kernel.  The expected strings are those of the three units
before they shared their scaffolding."""
from __future__ import annotations

import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

OK, INVALID, WORKSPACE, WEIGHTS = 0, 1, 2, 3
ENGINES = ("lipfe", "lipsn", "vfilt")
_cache = {}


class _Case:
    """One engine with the smallest shape it accepts, and a forward call whose every argument can be replaced."""

    def __init__(self, prefix):
        from speech_separation_amd.lipreader import LipreadingEngine, ShuffleNetLipreadingEngine
        from speech_separation_amd.voicefilter import VoiceFilterEngine
        dev = torch.device("cuda:0")
        self.prefix = prefix
        if prefix == "lipfe":
            self.eng, self.shape = LipreadingEngine(dev), (1, 1, 8, 8)          # S, T, H, W
        elif prefix == "lipsn":
            self.eng, self.shape = ShuffleNetLipreadingEngine(dev), (1, 1, 65, 65)
        else:
            self.eng, self.shape = VoiceFilterEngine(8, 512, dev), (1, 1, 1)     # B, W, Tv
        self.n = len(self.eng.slots)
        self.names = [k for k, _ in self.eng.slots]
        self.need = self.eng.workspace_bytes(*self.shape)
        # device memory that is only pointed at: the weight table's entries, the inputs and results, the workspace
        self.mem = torch.empty(4 * self.n + 4096 + self.need + 512, dtype=torch.uint8, device=dev)
        base = (self.mem.data_ptr() + 255) & ~255
        self.weights = [base + 4 * i for i in range(self.n)]
        self.io = (base + 4 * self.n + 255) & ~255
        self.ws = self.io + 4096

    def bind(self, ptrs):
        table = (C.c_void_p * len(ptrs))(*ptrs)
        return self.eng._fn("bind_weights")(self.eng._h, table, len(ptrs))

    def forward(self, ws=None, ws_bytes=None, window=None):
        ws = self.ws if ws is None else ws
        ws_bytes = self.need if ws_bytes is None else ws_bytes
        h, io = self.eng._h, self.io
        if self.prefix == "vfilt":
            B, W, Tv = self.shape
            return self.eng._fn("forward")(h, io, io, io, B, W, Tv, io, io, ws, ws_bytes, None)
        S, T, H, W = self.shape
        Hin, Win, y0, x0 = window or (H, W, 0, 0)
        return self.eng._fn("forward")(h, io, S, T, Hin, Win, y0, x0, H, W, 1.0, 0.0, io, ws, ws_bytes, None)

    def error(self):
        return self.eng._fn("last_error")(self.eng._h).decode()


def _case(prefix, bound):
    """A fresh engine for the tests that need it unbound, one bound engine per prefix for the rest."""
    if not bound:
        return _Case(prefix)
    if prefix not in _cache:
        c = _Case(prefix)
        assert c.bind(c.weights) == OK, c.error()
        _cache[prefix] = c
    return _cache[prefix]


@pytest.mark.parametrize("prefix", ENGINES)
def test_bind_refuses_a_short_table(prefix):
    c = _case(prefix, bound=False)
    assert c.bind(c.weights[:-1]) == WEIGHTS
    assert c.error() == f"expected {c.n} weight pointers, got {c.n - 1}"


@pytest.mark.parametrize("prefix", ENGINES)
def test_bind_refuses_a_null_entry(prefix):
    c = _case(prefix, bound=False)
    i = c.n // 2
    assert c.bind(c.weights[:i] + [None] + c.weights[i + 1:]) == WEIGHTS
    assert c.error() == f"weight {i} ({c.names[i]}) is NULL"


@pytest.mark.parametrize("prefix", ENGINES)
def test_bind_refuses_a_misaligned_entry(prefix):
    c = _case(prefix, bound=False)
    i = c.n - 1
    assert c.bind(c.weights[:i] + [c.weights[i] + 2]) == WEIGHTS
    assert c.error() == f"weight {i} ({c.names[i]}) is not 4-byte aligned"


@pytest.mark.parametrize("prefix", ENGINES)
def test_forward_refuses_before_any_bind(prefix):
    c = _case(prefix, bound=False)
    assert c.forward() == WEIGHTS
    assert c.error() == f"weights not bound ({prefix}_bind_weights)"
    c.bind(c.weights[:-1])      # a refused bind binds nothing
    assert c.forward() == WEIGHTS
    assert c.error() == f"weights not bound ({prefix}_bind_weights)"


@pytest.mark.parametrize("prefix", ENGINES)
def test_forward_refuses_a_short_workspace(prefix):
    c = _case(prefix, bound=True)
    assert c.forward(ws_bytes=c.need - 1) == WORKSPACE
    assert c.error() == f"workspace: need {c.need} bytes, 256-byte aligned (got {c.need - 1} at {c.ws:#x})"


@pytest.mark.parametrize("prefix", ENGINES)
def test_forward_refuses_a_misaligned_workspace(prefix):
    c = _case(prefix, bound=True)
    assert c.forward(ws=c.ws + 128) == WORKSPACE
    assert c.error() == f"workspace: need {c.need} bytes, 256-byte aligned (got {c.need} at {c.ws + 128:#x})"


@pytest.mark.parametrize("prefix", ("lipfe", "lipsn"))
@pytest.mark.parametrize("dy, dx", [(1, 0), (0, 1), (-1, 0), (0, -1)])
def test_forward_refuses_a_window_outside_the_frame(prefix, dy, dx):
    c = _case(prefix, bound=True)
    S, T, H, W = c.shape
    Hin, Win = H + 2, W + 3
    y0, x0 = (Hin - H + 1 if dy > 0 else dy), (Win - W + 1 if dx > 0 else dx)      # one row / column past an edge
    assert c.forward(window=(Hin, Win, y0, x0)) == INVALID
    assert c.error() == f"window {H} x {W} at ({y0}, {x0}) does not lie inside the {Hin} x {Win} frame"
