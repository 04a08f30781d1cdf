"""ReplayRing: the DQN replay memory kept on the GPU.

Device twin of the reference's memory (scripts/main.py:91-92 `np.zeros((MEMORY_CAPACITY,
NUM_STATES * 2 + 2))`, :115-119 store_transition, :129-135 the minibatch draw in learn(); the
same structure in scripts/hdqn.py:157-158, :180-184, :194-199). Rows are
[s(10), a, r, s'(10)] fp32 -- the reference keeps fp64 rows and reads them back through
torch.FloatTensor, so the values learn() sees are the same. `ReplayRing(cap, goal=True)` holds
hdqn.py's lower-level rows [goal, s(10), a, r, next_goal, s'(10)] (goal_state = [goal] + state,
:291 and :304; intrinsic reward :314): store() then takes the per-transition goals and the
reward column.

Transitions go in straight from a MergeVecEnv's trajectory buffers (one batched store per
rollout, three kernel launches from libmerging_hip.so) instead of one store_transition call
per env step; the order is (step, env), i.e. what stepping env 0..N-1 and storing each in
turn would give. The ring position lives on the device; reading `memory_counter`
synchronises.

    ring = ReplayRing(capacity=2000, device="cuda:0")
    obs0 = env.observe().clone()
    traj = env.rollout_qnet(16, qnet, seed)
    ring.store_rollout(obs0, traj)                       # main.py:209 filter by default
    s, a, r, s2 = ring.sample(128, seed=1, draw=step)    # main.py:130-135
"""

from __future__ import annotations

import ctypes

from . import _native
from ._base import MAX_MEMBERS, RingBase
from ._device import ptr

_OBS_DIM = 10
ROW = 2 * _OBS_DIM + 2        # main.py:91: NUM_STATES * 2 + 2
ROW_GOAL = 2 * _OBS_DIM + 4   # hdqn.py:158: (NUM_STATES + 1) * 2 + 2


class ReplayRing(RingBase):
    def __init__(self, capacity: int = 2000, device=None, goal: bool = False):
        self.goal = bool(goal)
        self._s0 = 1 if self.goal else 0  # column of s[0]
        super().__init__(capacity, ROW_GOAL if self.goal else ROW, device)
        self._scratch = self._torch.empty(0, dtype=self._torch.int64, device=self.device)
        self._sample_bufs = {}

    # ------------------------------------------------------------------ helpers
    def _scratch_for(self, nbytes):
        """The ring's scratch, grown to `nbytes` (the library's mg_replay_scratch*_bytes of the store)."""
        if self._scratch.numel() * 8 < nbytes:
            self._scratch = self._torch.empty((nbytes + 7) // 8, dtype=self._torch.int64, device=self.device)
        return self._scratch

    def _batch_f32(self, T, n, obs_first, obs, rew, final_obs):
        """The float tensors of a [T, n, ...] batch, as contiguous fp32 on the ring's device."""
        return (self._f32(obs_first, (n, _OBS_DIM)), self._f32(obs, (T, n, _OBS_DIM)), self._f32(rew, (T, n, 2)),
                None if final_obs is None else self._f32(final_obs, (T, n, _OBS_DIM)))

    def _transitions(self, **tensors):
        """mg_transitions of the named tensors (None or unnamed: absent); the ring keeps them alive until its next
        store has been enqueued."""
        self._keepalive = tuple(tensors.values())
        return _native.Transitions(**{k: ptr(t) for k, t in tensors.items()})

    # ------------------------------------------------------------------ stores
    @property
    def memory_counter(self) -> int:
        """Transitions stored so far (main.py:119). Synchronises the stream."""
        return int(self._counter.item())

    def store(self, obs_first, obs, a1, rew, done=None, final_obs=None, won_mask=None,
              skip_ego_won: bool = True, goal=None, next_goal=None, reward=None, flags=None, meta_goal=None):
        """Append T steps of N envs ([T, N, ...] tensors; obs_first [N, 10] = observation
        before step 0). skip_ego_won drops the transitions whose won bit is set (main.py:209;
        hdqn.py:316 stores all: pass False). A goal ring needs goal / next_goal [T, N] (the goal
        columns of s and s'); reward [T, N] replaces the ego's env reward rew[..., 0] as the r
        column (hdqn.py:314's intrinsic reward). flags: a rollout's interleaved [T, N, 4] buffer
        (a1, a2, done, collision), read in place of a1 / done. Stream-ordered; nothing is
        synchronised. meta_goal [T, N]: Goal_DQN's memory instead (hdqn.py:97-101 at :325, a plain
        22-float ring): rows [s', meta_goal, reward, s'] for the steps whose won_mask bit is clear,
        the mask then being the rollout's no_break and reward its ext_reward (store_meta)."""
        torch = self._torch
        if self.goal != (goal is not None) or (goal is None) != (next_goal is None):
            raise ValueError("a goal ring takes goal and next_goal; a plain ring takes neither")
        if meta_goal is not None:
            if self.goal or reward is None or won_mask is None:
                raise ValueError("Goal_DQN rows need a plain ring, reward (ext_reward) and won_mask (no_break)")
            skip_ego_won = True
        a1 = torch.as_tensor(a1, device=self.device)
        if a1.dim() == 1:  # one step: every [N, ...] tensor becomes [1, N, ...]
            a1, obs, rew, done, final_obs, won_mask, flags, goal, next_goal, reward, meta_goal = (
                None if t is None else torch.as_tensor(t, device=self.device)[None]
                for t in (a1, obs, rew, done, final_obs, won_mask, flags, goal, next_goal, reward, meta_goal))
        T, n = a1.shape
        if flags is not None:
            flags = torch.as_tensor(flags, device=self.device)
            if flags.dtype != torch.uint8 or tuple(flags.shape) != (T, n, 4) or not flags.is_contiguous():
                raise ValueError(f"flags must be a contiguous [{T}, {n}, 4] uint8 tensor")
            a1, done = None, None  # read from flags
        elif a1.dtype != torch.int8:
            a1 = a1.to(torch.int8)
        if a1 is not None:
            a1 = a1.contiguous()
        obs_first, obs, rew, final_obs = self._batch_f32(T, n, obs_first, obs, rew, final_obs)
        if goal is not None:
            goal, next_goal = self._f32(goal, (T, n)), self._f32(next_goal, (T, n))
        if reward is not None:
            reward = self._f32(reward, (T, n))
        if meta_goal is not None:
            meta_goal = self._f32(meta_goal, (T, n))
        if done is not None:
            done = torch.as_tensor(done, device=self.device)
            if done.dtype == torch.bool:
                done = done.view(torch.uint8)
            done = done.to(torch.uint8).contiguous()
            if tuple(done.shape) != (T, n):
                raise ValueError(f"done must have shape {(T, n)}")
        if skip_ego_won and won_mask is not None:
            won_mask = torch.as_tensor(won_mask, device=self.device).to(torch.int64).contiguous()
            if tuple(won_mask.shape) != (T, (n + 63) // 64):
                raise ValueError(f"won_mask must have shape {(T, (n + 63) // 64)}")
        elif skip_ego_won:
            raise ValueError("skip_ego_won needs the won_mask of the step(s) (main.py:209): roll out "
                             "with won_mask=True / MergeVecEnv(won_mask=True), or pass skip_ego_won=False")
        tr = self._transitions(obs_first=obs_first, obs=obs, final_obs=final_obs, a1=a1, rew=rew, done=done,
                               won_mask=won_mask if skip_ego_won else None, goal=goal, next_goal=next_goal,
                               reward=reward, flags=flags, meta_goal=meta_goal)
        scratch = self._scratch_for(int(_native.lib.mg_replay_scratch_bytes(n, T)))
        rc = _native.lib.mg_replay_store(
            self.memory.data_ptr(), self._counter.data_ptr(), self.capacity, self.row, ctypes.byref(tr), n,
            T, 1 if skip_ego_won else 0, scratch.data_ptr(), scratch.numel() * 8, self._stream())
        _native.check(rc, "mg_replay_store")

    def store_rollout(self, obs_first, traj, skip_ego_won: bool = True, goal=None, next_goal=None,
                      reward=None):
        """Append a MergeVecEnv rollout (the dict rollout_random / rollout_qnet return). With
        autoreset the obs row of a finished env is already the reset observation, so the
        terminal one must come from final_observation (roll out with final_observation=True)."""
        self.store(obs_first, traj["obs"], traj["a1"], traj["rew"], traj["done"], self._final_observation(traj),
                   traj.get("won_mask"), skip_ego_won, goal, next_goal, reward, traj.get("flags"))

    def store_meta(self, traj):
        """Append Goal_DQN's rows of an h-DQN rollout (MergeVecEnv.rollout_hdqn(...,
        goal_memory=True)): upper.store_transition(state, goal, extrinsic_reward, next_state) at
        every inner-loop break or episode end (hdqn.py:325; state is already next_state and goal
        the :303 choice), in (t, i) order, into a plain ring (GOAL_MEMORY_CAPACITY = 200, :22,
        :75)."""
        if traj.get("final_observation") is None or traj.get("no_break") is None:
            raise ValueError("roll out with final_observation=True and goal_memory=True")
        self.store(traj["obs"][0], traj["obs"], traj["a1"], traj["rew"], traj["done"], traj["final_observation"],
                   traj["no_break"], True, None, None, traj["ext_reward"], traj.get("flags"),
                   meta_goal=traj["next_goal"])

    def store_transition(self, state, action, reward, next_state):
        """The reference's single-transition call (main.py:115-119; hdqn.py:180-184 for a goal
        ring, where state / next_state are the 11-value goal states [goal] + state), through the
        same kernels."""
        if not self.goal:
            self.store(*self._single(state, action, reward, next_state), skip_ego_won=False)
            return
        gs, gs2 = [float(x) for x in state], [float(x) for x in next_state]
        g = self._torch.as_tensor([[gs[0]]], dtype=self._torch.float32)
        g2 = self._torch.as_tensor([[gs2[0]]], dtype=self._torch.float32)
        self.store(*self._single(gs[1:], action, reward, gs2[1:]), skip_ego_won=False, goal=g.to(self.device),
                   next_goal=g2.to(self.device))

    # ------------------------------------------------------------------ checkpoint / resume
    def state_dict(self):
        """memory (copy) and memory_counter -- what DQN's memory and counter hold."""
        return dict(super().state_dict(), goal=self.goal)

    def load_state_dict(self, sd):
        mem = self._torch.as_tensor(sd["memory"])
        if tuple(mem.shape) != tuple(self.memory.shape) or bool(sd.get("goal", False)) != self.goal:
            raise ValueError(f"expected a {tuple(self.memory.shape)} ring (goal={self.goal})")
        super().load_state_dict(sd)

    # ------------------------------------------------------------------ sampling
    def sample_rows(self, batch_size: int = 128, seed: int = 0, draw: int = 0,
                    filled_only: bool = False, return_index: bool = False):
        """[B, 22] (goal ring: [B, 24]) rows at Philox-drawn slots: np.random.choice(MEMORY_CAPACITY, BATCH_SIZE)
        (main.py:130-131); filled_only draws from the stored rows only. The returned tensor is
        reused by the next call with the same batch size."""
        torch = self._torch
        B = int(batch_size)
        buf = self._sample_bufs.get(B)
        if buf is None:
            buf = (torch.empty((B, self.row), dtype=torch.float32, device=self.device),
                   torch.empty(B, dtype=torch.int64, device=self.device))
            self._sample_bufs[B] = buf
        rows, idx = buf
        self._sample_into(rows, idx, seed, draw, filled_only)
        return (rows, idx) if return_index else rows

    def sample(self, batch_size: int = 128, seed: int = 0, draw: int = 0, filled_only: bool = False):
        """(batch_state [B,10] f32, batch_action [B,1] int64, batch_reward [B,1] f32,
        batch_next_state [B,10] f32) -- the slices of main.py:131-135; for a goal ring the
        states are the 11-value goal states, as hdqn.py:196-199 slices them."""
        rows = self.sample_rows(batch_size, seed, draw, filled_only)
        k = _OBS_DIM + self._s0  # state width
        return (rows[:, :k], rows[:, k:k + 1].to(self._torch.int64), rows[:, k + 1:k + 2], rows[:, -k:])


def store_rollout_many(rings, obs_first, traj, skip_ego_won: bool = True):
    """Append one rollout of N = M n envs (MergeVecEnv.rollout_qnet_many's dict; obs_first [N, 10] = the
    observation before step 0) to M rings, member m's slice [m n, (m + 1) n) to rings[m]: exactly what
    rings[m].store_rollout leaves when given a contiguous copy of the slice, in three launches for all members
    (mg_replay_store_many). The rings are plain (not goal), distinct, of one capacity and on one device; n is a
    multiple of 64. traj["flags"] and traj["won_mask"] are read in place; like store_rollout it needs the
    rollout's final_observation. Nothing is copied and nothing is synchronised."""
    rings = list(rings)
    M = len(rings)
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"store_rollout_many takes 1..{MAX_MEMBERS} rings, got {M}")
    r0 = rings[0]
    torch = r0._torch
    if any(r.goal for r in rings):
        raise ValueError("the member store writes 22-float rows: goal rings are refused")
    if any(r.capacity != r0.capacity or r.device != r0.device for r in rings):
        raise ValueError("the rings share one capacity and one device")
    if len({id(r) for r in rings}) != M:
        raise ValueError("a ring is listed twice: two members' appends to one ring have no defined order")
    final_obs = RingBase._final_observation(traj)
    flags = traj.get("flags")
    if flags is None or flags.dtype != torch.uint8 or flags.dim() != 3 or not flags.is_contiguous():
        raise ValueError("the member store reads the rollout's interleaved [T, N, 4] uint8 flags buffer")
    T, N = int(flags.shape[0]), int(flags.shape[1])
    if N % M or (N // M) % 64:
        raise ValueError(f"N = {N} must be {M} slices of a multiple of 64 envs")
    obs_first, obs, rew, final_obs = r0._batch_f32(T, N, obs_first, traj["obs"], traj["rew"], final_obs)
    won_mask = traj.get("won_mask")
    if skip_ego_won:
        if won_mask is None:
            raise ValueError("skip_ego_won needs the rollout's won_mask (main.py:209): roll out with won_mask=True, "
                             "or pass skip_ego_won=False")
        if (won_mask.dtype != torch.int64 or tuple(won_mask.shape) != (T, (N + 63) // 64)
                or not won_mask.is_contiguous() or won_mask.device != r0.device):
            raise ValueError(f"won_mask must be a contiguous [{T}, {(N + 63) // 64}] int64 tensor on {r0.device}")
    tr = r0._transitions(obs_first=obs_first, obs=obs, final_obs=final_obs, rew=rew,
                         won_mask=won_mask if skip_ego_won else None, flags=flags)
    scratch = r0._scratch_for(int(_native.lib.mg_replay_scratch_many_bytes(N // M, T, M)))
    rows = (ctypes.c_void_p * M)(*(r.memory.data_ptr() for r in rings))
    counters = (ctypes.c_void_p * M)(*(r._counter.data_ptr() for r in rings))
    rc = _native.lib.mg_replay_store_many(rows, counters, M, r0.capacity, r0.row, ctypes.byref(tr), N // M, T,
                                          1 if skip_ego_won else 0, scratch.data_ptr(), scratch.numel() * 8,
                                          r0._stream())
    _native.check(rc, "mg_replay_store_many")
