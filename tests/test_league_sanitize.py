"""The league's host code under AddressSanitizer and UndefinedBehaviorSanitizer: the library's source and
tests/native/league_sanitize.cpp (its own main) built into one stand-alone program, as
tests/test_per_many_sanitize.py builds its driver. Every refusal of mg_rollout_qnet_league and mg_stats_reduce_many
runs there, the mg_league_net list an exactly sized heap block of 1 and of 64 entries, and
mg_stats_reduce_many_scratch_bytes at the edges of its block count; both entry points only refuse or return with
nothing to do. No GPU is touched and nothing is loaded into Python."""

import pytest

from native_build import hipcc, run_sanitized_driver


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_league_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("league_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "league sanitizer run: 0 failures" in r.stdout
