"""Memory safety of VoiceFilter's waveform ends (include/vfwave.h) on the GPU: poisoned outputs, then every input and
output buffer flush against an unmapped page at its end, then at its start (tests/vf_wave_memsafety_child.py over
tests/guardmem).  One child process per (mode, shape), so that a fault kills the child, not the suite; every output
element is written and each result equals the plain run bit for bit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("variant", [0, 1], ids=["400x100_1x201", "256x128_17x2048"])
@pytest.mark.parametrize("mode", ["poison", "guard_end", "guard_start"])
def test_memory_safety(mode, variant):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tests.vf_wave_memsafety_child", mode, str(variant)], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    begins = [ln for ln in r.stdout.splitlines() if ln.startswith(("BEGIN", "=="))]
    last = " / ".join(begins[-2:]) if begins else "(nothing started)"
    assert r.returncode == 0, f"{mode}: child ended with code {r.returncode} during [{last}]\n{r.stdout[-3000:]}"
    assert f"OK {mode} vfwave {variant}" in r.stdout, r.stdout[-3000:]
