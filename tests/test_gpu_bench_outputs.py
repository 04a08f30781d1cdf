"""bench.py --dump-outputs on the GPU: one plain run of the benchmark's main() on a small batch. The
arrays it writes must be what the same sequence of launches (stagger, burn-in, warm-up, K timed
steps with the same seed) leaves in a second MergeVecEnv stepped here, value for value: the inputs
are fixed by the arguments, so the dump compares two builds output for output. The result line must
report the K it was given and an ms_per_step consistent with its value, and carry no --full leg."""

import json
import os
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

ENVS, STEPS, WARMUP, STAGGER, BURN, SEED = 4099, 7, 3, 5, 11, 77


def test_plain_run_dumps_the_last_timed_steps_outputs(tmp_path, monkeypatch, capsys):
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from merging_gym import MergeVecEnv

    out = tmp_path / "dump"
    # in this process (a benchmark process of its own would spend the test's time starting up);
    # --sync-spin 0: the device flags of a process whose HIP context exists are left alone
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", str(WARMUP),
                                      "--envs", str(ENVS), "--stagger", str(STAGGER), "--burn-in-launches", str(BURN),
                                      "--seed", str(SEED), "--sync-spin", "0", "--dump-outputs", str(out)])
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    bench.main()
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    assert line["steps"] == STEPS and line["warmup"] == WARMUP and line["full"] is False
    assert line["unit"] == "env-steps/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and np.isclose(line["value"], ENVS / (line["ms_per_step"] * 1e-3), rtol=1e-6)
    assert line["legs"] == {} and "cpu_baseline" not in line

    env = MergeVecEnv(ENVS, device="cuda:0", autoreset=True, final_observation=True, episode_stats=True)
    k = bench.stagger(env, STAGGER, SEED, 0, torch)
    env.clear_statistics()
    for k in range(k, k + BURN + WARMUP + STEPS):
        result = env.step_random(SEED, opponent_random=True, step_idx=k)
    torch.cuda.synchronize()
    want = bench.snapshot_outputs(env, result, torch)
    assert sorted(os.listdir(out)) == sorted(name + ".npy" for name in want)
    assert np.array_equal(want["env_index"], np.arange(ENVS))  # below DUMP_ROWS: every env
    total = 0
    for name, w in want.items():
        got = np.load(out / (name + ".npy"))
        total += got.nbytes
        assert got.dtype == w.dtype and got.dtype in (np.float32, np.float64), name
        assert np.array_equal(got, w), name
    assert total <= 64e6
    assert np.isfinite(want["obs"]).all() and want["obs"].any()
