"""The prioritized replay entry points' host code under AddressSanitizer and UndefinedBehaviorSanitizer: the
library's source and tests/native/per_sanitize.cpp (its own main) built into one stand-alone program, as
tests/test_rainbow_learn_sanitize.py builds rainbow_learn_sanitize. The host twins mg_host_per_* (stores that
wrap and exceed the ring, samples, updates with duplicates and rejected entries, at capacities 1, 13 and 3000)
and mg_host_rainbow_learn_prioritized run there on exactly sized heap buffers; the device entry points only
refuse. No GPU is touched and nothing is loaded into Python."""

import pytest

from native_build import hipcc, run_sanitized_driver


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_prioritized_replay_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("per_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "prioritized replay sanitizer run: 0 failures" in r.stdout
