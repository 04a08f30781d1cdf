"""The host code of the Rainbow rollouts against another net under AddressSanitizer and
UndefinedBehaviorSanitizer: the library's source and tests/native/rainbow_vs_sanitize.cpp (its own main) built into
one stand-alone program, as tests/test_league_sanitize.py builds its driver. Every refusal of mg_rollout_rainbow_vs
and mg_rollout_rainbow_vs_many runs there -- NULL and misaligned nets and opponents, members 0 and 65, n_member 96,
num_steps -1 and 65536 -- with the members' nets and opponents as exactly sized heap blocks of 1, 3 and 64 entries;
both entry points only refuse or return with nothing to do. No GPU is touched and nothing is loaded into Python."""

import pytest

from native_build import hipcc, run_sanitized_driver


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_rainbow_vs_host_code_under_asan_ubsan(tmp_path):
    r = run_sanitized_driver("rainbow_vs_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "rainbow vs sanitizer run: 0 failures" in r.stdout
