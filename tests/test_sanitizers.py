"""Host-code sanitizer runs ("race detection / sanitizers"): the C oracle and
the host side of libmerging_hip (argument validation, launch set-up) built with AddressSanitizer
and UndefinedBehaviorSanitizer and driven by tests/native/*. No GPU is touched: device-side
sanitizers (xnack+) are not available on the GPU pool, and the kernels are one thread per env
with no shared writes besides the LDS staging tiles."""

import os
import shutil
import subprocess

import pytest

from conftest import ROOT
from native_build import hipcc, run_sanitized_driver

NATIVE = os.path.join(ROOT, "tests", "native")
ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:abort_on_error=1",
           UBSAN_OPTIONS="halt_on_error=1:print_stacktrace=1")


def _run(cmd, **kw):
    return subprocess.run(cmd, capture_output=True, text=True, timeout=300, **kw)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="gcc not found")
def test_oracle_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "oracle_sanitize")
    b = _run(["gcc", "-O1", "-g", "-std=c11", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
              "-fno-omit-frame-pointer", "-ffp-contract=off", "-Wall", "-Wno-unknown-pragmas", "-o", exe,
              os.path.join(ROOT, "oracle", "merge_oracle.c"), os.path.join(NATIVE, "oracle_sanitize.c"), "-lm"])
    assert b.returncode == 0, b.stderr
    r = _run([exe], env=ENV)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "oracle sanitizer run ok" in r.stdout


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_library_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("abi_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "abi sanitizer run: 0 failures" in r.stdout
