"""The prioritized population's host code under AddressSanitizer and UndefinedBehaviorSanitizer: the library's
source and tests/native/per_many_sanitize.cpp (its own main) built into one stand-alone program, as
tests/test_rainbow_learn_many_sanitize.py builds its driver. mg_host_per_store_many and
mg_host_rainbow_learn_prioritized_many run there with three members at batch 33 on exactly sized heap buffers and
are compared with the lone host calls; the device entry points only refuse. No GPU is touched and nothing is
loaded into Python."""

import pytest

from native_build import hipcc, run_sanitized_driver


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_prioritized_population_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("per_many_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "prioritized population sanitizer run: 0 failures" in r.stdout
