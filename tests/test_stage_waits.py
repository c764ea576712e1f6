"""The off-diagonal GEMM1 stage loop keeps its B-operand prefetch in flight: tools/stage_waits.py
--check on k_chol.hip (no vmcnt wait below 7 between a stage's barrier and its last MFMA, no scratch
access, in the 64-MFMA loops of k_chol_offdiag<...>).

CPU only, skipped where hipcc is absent.  It costs one device-only compile of k_chol.hip, about
25 s."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="hipcc not found")
def test_gemm1_stage_loop_waits():
    env = dict(os.environ)
    if not os.path.exists(HIPCC):
        env["HIPCC"] = shutil.which("hipcc")   # the Makefile's HIPCC ?= default is overridden from the environment
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "stage_waits.py"), "--check",
                        os.path.join(ROOT, "tblup_amd", "csrc", "k_chol.hip")], capture_output=True, text=True, env=env)
    print(r.stdout[-4000:], r.stderr[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "check ok:" in r.stdout
