"""Memory safety of the VoiceFilter training step (include/vfilt_train.h) on the GPU: poisoned outputs, workspace and
gradient buffers, then every input, output, gradient buffer, bound weight and the workspace flush against an unmapped page
at its end, then at its start (tests/voicefilter_train_memsafety_child.py over tests/guardmem), at a shape where whole
dilated taps fall outside the map, the map is narrower than the 7-tap kernel and B F W = 357 fills no chunk, and at one
with more frames.  One child process per mode, so that a fault kills the child, not the suite; every written element is
written, the running-statistics slots stay untouched, and each result equals the plain run bit for bit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ["poison", "guard_end", "guard_start"])
def test_memory_safety(mode):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tests.voicefilter_train_memsafety_child", mode], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    begins = [ln for ln in r.stdout.splitlines() if ln.startswith(("BEGIN", "=="))]
    last = " / ".join(begins[-2:]) if begins else "(nothing started)"
    assert r.returncode == 0, f"{mode}: child ended with code {r.returncode} during [{last}]\n{r.stdout[-3000:]}"
    assert f"OK {mode} vftrain" in r.stdout, r.stdout[-3000:]
