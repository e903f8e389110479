"""Memory-safety harness for the long-sequence training attention (option train_long_seq = 1): poisoned buffers and guard
pages, one spawned child per mode (tests/train_long_memsafety_child.py, the pattern of tests/test_gpu_memsafety.py with the
allocator of tests/guardmem).  A fault kills the child, not the suite; the failure message carries the child's last
"BEGIN ..." line."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ["poison", "guard_end", "guard_start"])
def test_long_training_memory_safety(mode):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tests.train_long_memsafety_child", mode], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
    out = r.stdout
    begins = [ln for ln in out.splitlines() if ln.startswith(("BEGIN", "=="))]
    last = " / ".join(begins[-2:]) if begins else "(nothing started)"
    assert r.returncode == 0, f"{mode}: child ended with code {r.returncode} during [{last}]\n{out[-3000:]}"
    assert f"OK {mode} train_long" in out, out[-3000:]
