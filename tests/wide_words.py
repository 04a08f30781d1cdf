"""Shared by tests/test_wide_words_host.py and tests/test_gpu_wide_words.py: the 64-bit seeds, draws, step indices
and counters those tests run (every 32-bit half non-zero), the Random123 vectors, a ring that stores its own
row numbers, and the random store inputs of test_gpu_replay.py's test_mixed_size_stores_share_scratch."""

from __future__ import annotations

import numpy as np

from test_philox import KATS  # noqa: F401  (re-exported: counter, key, output of the three Random123 vectors)

U64 = (1 << 64) - 1
SEED_W = 0xA4093822299F31D0    # the key words of the third Random123 vector
SEED_TOP = 0xFFFFFFFF00000001
SEED_MAX = U64
DRAW_W = (1 << 40) + 3
DRAW_MAX = U64 - 1             # two updates draw at 2^64 - 2 and 2^64 - 1
DRAW_WRAP = U64                # two updates draw at 2^64 - 1 and 0: first_draw + u wraps
STEP_W = (1 << 36) + 11        # odd (the second draw of a word pair), above 2^35 (step div 8 and div 2 keep a high word)
ENV_OFF_W = (1 << 33) + 5
COUNTER_CROSS = (1 << 32) - 100  # a store of more than 100 rows crosses 2^32
COUNTER_ABOVE = (1 << 32) + 17
PROBE_CAP = 1 << 16            # slot = (x 2^16) >> 32 = the top 16 bits of Philox word x


def probe_ring(row_floats, capacity=PROBE_CAP):
    """[capacity, row_floats] fp32, row i = [i, 0, ...] (rainbow_learn_ref.ring_of_chosen_rows' trick): a sampled
    row's first column is the slot it was read from."""
    ring = np.zeros((capacity, row_floats), np.float32)
    ring[:, 0] = np.arange(capacity)
    return ring


def unpack_won(words, n):
    """[T, ceil(n/64)] int64 words -> [T, n] bool (bit j of word w = env 64 w + j)."""
    m = np.ascontiguousarray(words).view(np.uint64)
    bits = (m[..., :, None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)
    return bits.reshape(*m.shape[:-1], -1)[..., :n].astype(bool)


def store_inputs(rng, n, T, goal=False):
    """Random inputs of one store: won words with about a quarter of the bits set, bits past n included (they
    must be ignored); 10 % done rows, which take s' from final_obs. goal: also the goal, next_goal and reward
    columns of a goal ring's rows."""
    d = dict(obs0=rng.standard_normal((n, 10)).astype(np.float32),
             obs=rng.standard_normal((T, n, 10)).astype(np.float32),
             fobs=rng.standard_normal((T, n, 10)).astype(np.float32),
             a1=rng.integers(0, 5, (T, n)).astype(np.int8),
             rew=rng.standard_normal((T, n, 2)).astype(np.float32),
             done=(rng.random((T, n)) < 0.1).astype(np.uint8))
    words = rng.integers(0, 2**63, (T, (n + 63) // 64), dtype=np.int64)
    words &= rng.integers(0, 2**63, words.shape, dtype=np.int64)
    d["words"] = words
    if goal:
        d["goal"] = rng.integers(0, 3, (T, n)).astype(np.float32)
        d["goal2"] = rng.integers(0, 3, (T, n)).astype(np.float32)
        d["r_int"] = (rng.random((T, n)) < 0.3).astype(np.float32)
    return d
