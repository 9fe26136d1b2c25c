"""The host-side tables of the key-pose guide call: the inverse tie table (convofusion_amd/csrc/guide_tables.hpp: guide_build_tie_csr)
and the row limit a caller hands to the forward-path decision (convofusion_amd/csrc/forward_path.hpp: PathAsk::max_rows).
tests/host/guide_tables_test.cpp is a stand-alone program that checks both against values written out by hand.  It is compiled with the
host g++ under AddressSanitizer and UBSan and run as a child process, nothing preloaded: a failed check makes it exit non-zero.  No GPU,
no HIP runtime, no HIP header."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "guide_tables_test.cpp")


def test_guide_tables_under_sanitizers(tmp_path):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    exe = str(tmp_path / "guide_tables_test")
    # (the sanitizers' runtimes are linked into the program, so it runs the same whatever else the loader brings in)
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", SRC, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout
