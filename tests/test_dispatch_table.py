"""The dispatch table of the point-function kernels (mrhyde_amd/csrc/kernels/engine_dispatch.hpp), checked on the host:
tests/dispatch_table_check.cpp drives dispatch_module and dispatch_expr with a recording functor and compares with a
table written out there -- the 19 (dimension, module) pairs, pairs that do not exist, and for every module the EXPR
variant or the refusal text of each situation.  A correct kernel reached for the wrong case is what no comparison of the
kernels themselves can show.  Built host-only; no GPU, no HIP runtime call."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


@pytest.mark.skipif(shutil.which(HIPCC) is None, reason="hipcc not installed")
def test_dispatch_table(tmp_path):
    exe = tmp_path / "dispatch_table_check"
    build = subprocess.run([HIPCC, "-std=c++17", "-O0", "-Wall", "-Wextra", "-Wno-unused-parameter", "-x", "hip",
                            "--cuda-host-only", os.path.join(HERE, "dispatch_table_check.cpp"), "-o", str(exe)],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    run = subprocess.run([str(exe)], capture_output=True, text=True)
    assert run.returncode == 0 and run.stdout.strip() == "ok", run.stdout + run.stderr
