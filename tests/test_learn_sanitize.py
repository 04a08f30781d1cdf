"""DQN.learn's host code under AddressSanitizer and UndefinedBehaviorSanitizer: the library's source
and tests/native/learn_sanitize.cpp (its own main) built into one stand-alone program, as
tests/test_sanitizers.py builds abi_sanitize. mg_host_dqn_learn runs there on exactly sized heap
buffers for (10, 5, 96) and (11, 5, 32); the device entry points only refuse. No GPU is touched and
nothing is loaded into Python."""

import pytest

from native_build import hipcc, run_sanitized_driver


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_learn_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("learn_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "learn sanitizer run: 0 failures" in r.stdout
