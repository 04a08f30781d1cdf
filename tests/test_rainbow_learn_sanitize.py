"""The Rainbow learning entry points' host code under AddressSanitizer and UndefinedBehaviorSanitizer: the
library's source and tests/native/rainbow_learn_sanitize.cpp (its own main) built into one stand-alone program,
as tests/test_rainbow_sanitize.py builds rainbow_sanitize. mg_host_rainbow_learn (two updates at batch 33 on a
partly filled ring, every optional output), mg_host_rainbow_project and mg_host_rainbow_log run there on exactly
sized heap buffers; the device entry points only refuse. No GPU is touched and nothing is loaded into Python."""

import os
import shutil
import subprocess

import pytest

from conftest import ROOT

NATIVE = os.path.join(ROOT, "tests", "native")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def _hipcc():
    for cand in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    return None


@pytest.mark.skipif(_hipcc() is None, reason="hipcc not found")
def test_rainbow_learn_host_code_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "rainbow_learn_sanitize")
    b = subprocess.run([_hipcc(), "--offload-arch=gfx950", "-O1", "-g", "-std=c++17", "-ffp-contract=off",
                        "-fno-omit-frame-pointer", "-Xarch_host", "-fsanitize=address", "-Xarch_host",
                        "-fsanitize=undefined", "-I", os.path.join(ROOT, "include"), "-o", exe,
                        os.path.join(ROOT, "merging-gym_amd", "csrc", "merging_hip.hip"),
                        os.path.join(NATIVE, "rainbow_learn_sanitize.cpp")], capture_output=True, text=True, timeout=300)
    assert b.returncode == 0, b.stderr[-2000:]
    r = subprocess.run([exe], env=ENV, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "rainbow learn sanitizer run: 0 failures" in r.stdout
