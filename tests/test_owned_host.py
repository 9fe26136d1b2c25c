"""The library's owning resources (convofusion_amd/csrc/owned.hpp: DBuf, GraphExec) on the host: tests/host/owned_test.cpp is a stand-alone
program with counting stubs of hipMalloc / hipFree / hipDeviceSynchronize / hipGraph(Exec)Destroy.  It is compiled with the host g++ under AddressSanitizer and
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


@pytest.fixture(scope="module")
def owned_test_run(tmp_path_factory):
    """The program, built and run once: its CompletedProcess."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++ on this machine")
    inc = _rocm_include()
    if inc is None:
        pytest.skip("no ROCm headers (hip/hip_runtime_api.h) on this machine")
    exe = str(tmp_path_factory.mktemp("owned") / "owned_test")
    # (the sanitizers' runtimes are linked into the program, so it runs the same whatever else the loader brings in)
    cmd = [gxx, "-std=c++17", "-g", "-O1", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
           "-static-libasan", "-static-libubsan", "-D__HIP_PLATFORM_AMD__", "-I" + inc, SRC, "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stdout + built.stderr
    return subprocess.run([exe], capture_output=True, text=True, timeout=120)


def test_owned_resources_under_sanitizers(owned_test_run):
    run = owned_test_run
    assert run.returncode == 0, run.stdout + run.stderr
    assert "all checks passed" in run.stdout


def test_arena_layout_sizes_exactly_what_it_carves(owned_test_run):
    """ArenaLayout (owned.hpp), the one statement of a workspace's buffers behind wegrt::prepare, wegrt::prepare_mem_grad and
    cfd_vae_decode_vjp: for three field lists whose counts are no multiples of the granule, at granule 4 and at granule 64, the sizing
    pass (null base) returns exactly the bytes the carving pass consumes, and the carved addresses are granule-aligned, in call order and
    disjoint (test_arena_layout of the program; under AddressSanitizer every element of every buffer is written)."""
    run = owned_test_run
    assert run.returncode == 0, run.stdout + run.stderr
    assert "ArenaLayout: 6 layouts sized and carved alike" in run.stdout


def test_carve_grows_by_one_rule(owned_test_run):
    """carve and DBuf::grow (owned.hpp), how every one-call unit sizes, grows and carves its workspace, at granule 4 and at granule 64
    against a counting stub of hipDeviceSynchronize (test_carve of the program): the first carve of an empty buffer allocates once and
    waits for nothing, and every field equals a hand-run ArenaLayout's; the same layout again and a smaller one allocate nothing, wait
    for nothing and move nothing; a larger one waits exactly once, before the free; a failing hipMalloc returns the error and leaves the
    buffer empty, the live counters consistent and every field null; a buffer of 0 floats in a non-empty layout has an address."""
    run = owned_test_run
    assert run.returncode == 0, run.stdout + run.stderr
    assert "carve: 2 granules grown by one rule, the wait before the free" in run.stdout
