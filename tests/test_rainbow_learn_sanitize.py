"""The Rainbow learning entry points' host code under AddressSanitizer and UndefinedBehaviorSanitizer: the
library's source and tests/native/rainbow_learn_sanitize.cpp (its own main) built into one stand-alone program,
as tests/test_rainbow_sanitize.py builds rainbow_sanitize. mg_host_rainbow_learn (two updates at batch 33 on a
partly filled ring, every optional output), mg_host_rainbow_project and mg_host_rainbow_log run there on exactly
sized heap buffers; the device entry points only refuse. No GPU is touched and nothing is loaded into Python."""

import pytest

from native_build import hipcc, run_sanitized_driver


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_rainbow_learn_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("rainbow_learn_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "rainbow learn sanitizer run: 0 failures" in r.stdout
