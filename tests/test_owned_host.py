"""The library's owning resources (convofusion_amd/csrc/owned.hpp: DBuf, GraphExec) on the host: tests/host/owned_test.cpp is a stand-alone
program with counting stubs of hipMalloc / hipFree / hipGraph(Exec)Destroy.  It is compiled with the host g++ under AddressSanitizer and
UBSan and run as a child process, nothing preloaded: a leak, a double free, a use after move or a failed case makes it exit non-zero.  No GPU, no HIP runtime."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "owned_test.cpp")


def _rocm_include():
    for root in (os.environ.get("ROCM_PATH"), "/opt/rocm"):
        if root and os.path.exists(os.path.join(root, "include", "hip", "hip_runtime_api.h")):
            return os.path.join(root, "include")
    return None


def test_owned_resources_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("no ROCm headers (hip/hip_runtime_api.h) on this machine")
    exe = str(tmp_path / "owned_test")
    # (the sanitizers' runtimes are linked into the program, so it runs the same whatever else the loader brings in)
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + inc, SRC, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
