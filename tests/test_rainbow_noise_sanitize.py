"""The device-noise entry points' host code under AddressSanitizer and UndefinedBehaviorSanitizer: the library's
source and tests/native/rainbow_noise_sanitize.cpp (its own main) built into one stand-alone program, as
tests/test_per_sanitize.py builds per_sanitize. The host twins mg_host_rainbow_noise (U = 0, 1, 3) and
mg_host_rainbow_ndtri (n = 0, 1, 65) run there on exactly sized heap buffers; the device entry points only
refuse. No GPU is touched and nothing is loaded into Python."""

import pytest

from native_build import hipcc, run_sanitized_driver


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_rainbow_noise_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("rainbow_noise_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "rainbow noise sanitizer run: 0 failures" in r.stdout
