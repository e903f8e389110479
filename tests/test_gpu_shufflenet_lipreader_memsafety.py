"""Memory safety of the ShuffleNet-v2 lip reader (include/lipsn.h) on the GPU: poisoned output and workspace, then the input,
the output, the workspace and every bound weight flush against an unmapped page at its end, then at its start
(tests/shufflenet_memsafety_child.py over tests/guardmem), for the plain and the windowed forward.  One child process per
mode, so that a fault kills the child, not the suite; every output element is written and each result equals the plain
run bit for bit."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("mode", ["poison", "guard_end", "guard_start"])
def test_memory_safety(mode):
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    r = subprocess.run([sys.executable, "-m", "tests.shufflenet_memsafety_child", mode], cwd=ROOT, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    begins = [ln for ln in r.stdout.splitlines() if ln.startswith(("BEGIN", "=="))]
    last = " / ".join(begins[-2:]) if begins else "(nothing started)"
    assert r.returncode == 0, f"{mode}: child ended with code {r.returncode} during [{last}]\n{r.stdout[-3000:]}"
    assert f"OK {mode} lipsn" in r.stdout, r.stdout[-3000:]
