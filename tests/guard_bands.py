"""Guard bands around everything a rollout writes (a plain helper, not a conftest; tests/test_gpu_guard_bands.py).

MergeVecEnv._traj and rollout_hdqn's _hdqn_bufs hand the kernels exact-size torch allocations, and torch's
allocator rounds those up: a ragged last wave that stores one row too many, or a wave with no live env that
writes a mask word, lands in slack no test can see. install() builds the same dicts with every tensor in the
middle of a larger allocation -- BAND bytes on either side (a multiple of 256 B, so obs keeps its 16-byte
alignment), the whole allocation filled with byte 0xA5 -- and sets them as env._traj_bufs / env._hdqn_bufs, which
the next rollout with the same T and output choices reuses.
"""

from __future__ import annotations

import numpy as np

BAND = 4096
FILL = 0xA5
OBS_DIM = 10


class Guarded:
    """The guarded tensors by name, each with the allocation it sits in."""

    def __init__(self, torch, device):
        self.torch, self.device = torch, device
        self.raw = {}  # name -> (allocation [BAND + padded bytes + BAND] uint8, the tensor's bytes)

    def tensor(self, name, shape, dtype):
        torch = self.torch
        nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        padded = (nbytes + 255) // 256 * 256
        raw = torch.full((BAND + padded + BAND,), FILL, dtype=torch.uint8, device=self.device)
        assert raw.data_ptr() % 256 == 0
        self.raw[name] = (raw, nbytes)
        return raw[BAND:BAND + nbytes].view(dtype).view(shape)

    def assert_bands_intact(self):
        """Every byte before and after every tensor is still FILL."""
        for name, (raw, nbytes) in self.raw.items():
            lo, hi = raw[:BAND], raw[BAND + nbytes:]
            assert hi.numel() >= BAND
            for side, band in (("before", lo), ("after", hi)):
                bad = (band != FILL).nonzero().flatten()
                assert bad.numel() == 0, (f"{name}: {bad.numel()} bytes written {side} the tensor, the first at "
                                          f"offset {int(bad[0]) - (BAND if side == 'before' else 0)}")


def prefill_bits(torch, t):
    """A guarded fp32 tensor's prefill, as int32 bits (every byte FILL)."""
    return torch.full_like(t.view(torch.int32), int(np.array([FILL] * 4, np.uint8).view(np.int32)[0]))


def install(env, T, final_observation=True, won_mask=True, hdqn=False):
    """Guarded twins of env._traj(T, final_observation, won_mask)'s dict and (hdqn) of rollout_hdqn's buffers,
    installed on env. Returns the Guarded holding them."""
    torch, nat, n = env._torch, env._nat, env.num_envs
    g = Guarded(torch, env.device)
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    flags = g.tensor("flags", (T, n, 4), torch.uint8)
    buf = {"T": T,
           "obs": g.tensor("obs", (T, n, OBS_DIM), torch.float32),
           "rew": g.tensor("rew", (T, n, 2), torch.float32),
           "flags": flags,
           "final_observation": g.tensor("final_observation", (T, n, OBS_DIM), torch.float32) if final_observation else None,
           "won_mask": g.tensor("won_mask", (T, (n + 63) // 64), torch.int64) if won_mask else None}
    buf["_traj"] = nat.Traj(ptr(buf["obs"]), ptr(buf["rew"]), None, None, None, None, ptr(buf["final_observation"]),
                            ptr(buf["won_mask"]), ptr(flags))
    buf["_result"] = {"obs": buf["obs"], "rew": buf["rew"], "done": flags[..., 2].view(torch.bool),
                      "collision": flags[..., 3].view(torch.bool), "a1": flags[..., 0].view(torch.int8),
                      "a2": flags[..., 1].view(torch.int8), "final_observation": buf["final_observation"],
                      "won_mask": buf["won_mask"], "flags": flags}
    env._traj_bufs = buf
    if hdqn:
        hb = {k: g.tensor(k, (T, n), torch.float32) for k in ("goal", "next_goal", "reward", "goal_op", "ext_reward")}
        hb["no_break"] = g.tensor("no_break", (T, (n + 63) // 64), torch.int64)
        hb["_h"] = nat.HdqnTraj(*(hb[k].data_ptr() for k in ("goal", "next_goal", "reward", "goal_op")))
        hb["_hm"] = nat.HdqnTraj(*(hb[k].data_ptr() for k in ("goal", "next_goal", "reward", "goal_op", "ext_reward",
                                                               "no_break")))
        env._hdqn_bufs = hb
    return g


def assert_no_bits_past_n(words, n):
    """[T, ceil(n/64)] int64 mask words: every bit at or past n in the last word is 0."""
    if n % 64:
        last = words[:, -1].cpu().numpy().view(np.uint64)
        assert not (last >> np.uint64(n % 64)).any(), [hex(int(w)) for w in last]
