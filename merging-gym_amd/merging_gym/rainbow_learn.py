"""RainbowReplay and RainbowLearner: the reference's Rainbow training step on the device.

Device twins of ReplayBuffer (scripts/ranbowdqn.py:265-323, the buffer main() builds at :647) and of
compute_td_loss (:584-609) with projection_distribution (:554-582): a minibatch from the replay rows, the C51
projection of the target net's distribution, the cross-entropy against the current net's, Adam(lr 0.001), and
a fresh draw of both nets' noise. One call enqueues any number of updates on the current stream (seven kernel
launches each, libmerging_hip.so's mg_rainbow_learn) and repacks the current net for the acting kernels, so
the loop of ranbowdqn.py:662-691 closes without leaving the device:

    replay = RainbowReplay(10000, device="cuda:0")
    learner = RainbowLearner(RainbowNet.from_state_dict(sd, device="cuda:0"), replay)
    obs0 = env.observe().clone()
    traj = env.rollout_rainbow(16, learner.net)            # act + act on the rotated view + env.step
    replay.store_rollout(obs0, traj)                       # replay_buffer.push, every transition
    learner.learn(4)                                       # compute_td_loss, four times
    traj = env.rollout_rainbow(16, learner.net)            # acts with the new weights and the new noise
    learner.sync_target()                                  # update_target, every 20 episodes (:690-691)

The arithmetic is fp32 in the fixed order include/merging_hip.h documents, so a run is reproducible bit for
bit, also across a state_dict() / load_state_dict() resume. The noise is torch's: every update consumes the
draws of two RainbowNet.reset_noise calls (the current model's, then the target's) from `generator`. With
generator=DeviceNoise(noise_seed) a kernel draws the factors instead, from a counter-based stream keyed by
(noise_seed, update index) that include/merging_hip.h documents at mg_rainbow_noise: learn() then does no host
work and no upload, and the distribution, not the numbers, is torch's:

    learner = RainbowLearner(sd, replay, generator=DeviceNoise(7))
    learner.learn(4)                                       # enqueued behind the rollout and the store
    actor = RainbowNet.from_state_dict(sd); actor.reset_noise(seed=7, draw=3)   # the current model's noise now

PrioritizedRainbowReplay and PrioritizedRainbowLearner are the same pair over the script's
PrioritizedReplayBuffer (:326-437) and its sum / min segment trees (:130-262), which the script defines and
never runs: transitions enter with max_priority ** alpha, every update draws its minibatch from the tree,
weights the rows' losses and writes their new priorities back (nine launches, mg_rainbow_learn_prioritized):

    replay = PrioritizedRainbowReplay(10000, alpha=0.6, device="cuda:0")
    learner = PrioritizedRainbowLearner(sd, replay, beta=0.4, prio_eps=1e-5)
    replay.store_rollout(obs0, traj)
    learner.learn(4, beta=0.5)                             # beta per call: an annealing schedule
"""

from __future__ import annotations

import ctypes

from ._base import MAX_MEMBERS, LearnerBase, RingBase
from ._device import U64, ptr
from .rainbow import NOISY, NUM_ATOMS, PLAIN, SHAPES, RainbowNet

ROW = 24  # [s(10), a, r, s'(10), done, 0]: 8-byte aligned rows mg_replay_sample copies as they are
_OBS = 10

# RainbowDQN.named_parameters() order, and the noise buffers per noisy layer
PARAM_KEYS = tuple(f"{n}.{leaf}" for n in PLAIN for leaf in ("weight", "bias")) + tuple(
    f"{n}.{leaf}" for n in NOISY for leaf in ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma"))
EPS_KEYS = tuple(f"{n}.{leaf}" for n in NOISY for leaf in ("weight_epsilon", "bias_epsilon"))


def _shape(key):
    name, leaf = key.split(".")
    return SHAPES[name] if leaf.startswith("weight") else SHAPES[name][:1]


def _numel(key):
    s = _shape(key)
    return s[0] * (s[1] if len(s) == 2 else 1)


NUM_PARAMS = sum(_numel(k) for k in PARAM_KEYS)      # 58,884
NUM_EPS = sum(_numel(k) for k in EPS_KEYS)           # 28,210
NUM_FACTORS = sum(SHAPES[n][1] + 2 * SHAPES[n][0] for n in NOISY)  # 1,124 per model and update
OFF_M, OFF_V, OFF_EPS = 2 * NUM_PARAMS, 3 * NUM_PARAMS, 4 * NUM_PARAMS
OFF_Z = OFF_EPS + 2 * NUM_EPS
LEARNER_FLOATS = OFF_Z + NUM_ATOMS + 1


def learner_array(current, target=None):
    """The learner buffer (a flat fp32 CPU tensor) from RainbowDQN state dicts: current, target (default: a
    copy of current, noise included -- update_target, :551-552), zero Adam moments, both noise blocks, the
    support."""
    import torch

    target = current if target is None else target
    flat = lambda sd, keys: torch.cat([  # noqa: E731
        torch.as_tensor(sd[k]).detach().to("cpu", torch.float32).reshape(-1) for k in keys])
    buf = torch.cat([flat(current, PARAM_KEYS), flat(target, PARAM_KEYS), torch.zeros(2 * NUM_PARAMS),
                     flat(current, EPS_KEYS), flat(target, EPS_KEYS), torch.linspace(-10, 10, NUM_ATOMS),
                     torch.zeros(1)])
    assert buf.numel() == LEARNER_FLOATS
    return buf.contiguous()


def model_state_dict(buf, model):
    """RainbowDQN.state_dict() of model 0 (current) or 1 (target) of a learner buffer: copies, the reference's
    keys, the epsilon buffers included."""
    out = {}
    at = model * NUM_PARAMS
    for k in PARAM_KEYS:
        out[k] = buf[at:at + _numel(k)].reshape(_shape(k)).clone()
        at += _numel(k)
    at = OFF_EPS + model * NUM_EPS
    for k in EPS_KEYS:
        out[k] = buf[at:at + _numel(k)].reshape(_shape(k)).clone()
        at += _numel(k)
    order = [f"{n}.{leaf}" for n in PLAIN for leaf in ("weight", "bias")] + [
        f"{n}.{leaf}" for n in NOISY
        for leaf in ("weight_mu", "weight_sigma", "bias_mu", "bias_sigma", "weight_epsilon", "bias_epsilon")]
    return {k: out[k] for k in order}


def noise_factors(num_updates, generator=None):
    """[num_updates, 2, 1124] fp32: per update the factors of current_model.reset_noise() then
    target_model.reset_noise() (:606-607) -- per noisy layer epsilon_in, epsilon_out, the bias noise (:486-491) --
    the same stream as that many RainbowNet.reset_noise(generator) calls."""
    import torch

    out = torch.empty((int(num_updates), 2, NUM_FACTORS), dtype=torch.float32)
    flat, at = out.view(-1), 0
    sizes = [size for name in NOISY for size in (SHAPES[name][1], SHAPES[name][0], SHAPES[name][0])]
    for _ in range(2 * int(num_updates)):  # one randn per draw, as _scale_noise makes them: the same stream
        for size in sizes:
            torch.randn(size, generator=generator, out=flat[at:at + size])
            at += size
    return out.sign().mul_(out.abs().sqrt_())  # _scale_noise's x.sign().mul(x.abs().sqrt()), elementwise


class DeviceNoise:
    """The noise source of a learner that draws its factors on the device: pass it where a learner takes its
    `generator`. seed: the stream's key (None: the learner's minibatch seed). The stream is counter-based and
    has no state, so one DeviceNoise may serve several learners."""

    def __init__(self, seed=None):
        self.seed = None if seed is None else int(seed) & U64

    def __repr__(self):
        return f"DeviceNoise(seed={self.seed})"


def device_noise_factors(num_updates, noise_seed, first_update=0):
    """[num_updates, 2, 1124] fp32 on the CPU, in noise_factors' layout: the factors a DeviceNoise learner with
    this noise_seed draws for its updates first_update, first_update + 1, ... (libmerging_hip.so's
    mg_host_rainbow_noise, the host twin of the kernel: the same bits). The stream is counter-based -- element
    (u, model, factor) depends on (noise_seed, first_update + u, model, factor) alone -- so there is no state."""
    import torch

    from . import _native

    U = int(num_updates)
    if U < 0:
        raise ValueError("num_updates must be >= 0")
    out = torch.empty((U, 2, NUM_FACTORS), dtype=torch.float32)
    if U > 0:  # an empty tensor has no storage to point at
        rc = _native.lib.mg_host_rainbow_noise(int(noise_seed) & U64, int(first_update) & U64, U, out.data_ptr())
        _native.check(rc, "mg_host_rainbow_noise")
    return out


class RainbowReplay(RingBase):
    """ReplayBuffer(capacity) (:265-323) as a ring of [capacity, 24] fp32 rows on the device; the position is
    a device counter, so stores are stream-ordered and len() synchronises."""

    def __init__(self, capacity: int = 10000, device=None):
        super().__init__(capacity, ROW, device)

    def __len__(self):
        """len(replay_buffer) (:278-279). Synchronises the stream."""
        return min(int(self._counter.item()), self.capacity)

    def store(self, obs_first, obs, a1, rew, done=None, final_obs=None, flags=None):
        """Append T steps of N envs ([T, N, ...] tensors; obs_first [N, 10] = the observation before step 0) in
        (step, env) order, as pushing env 0..N-1 of each step in turn would. flags: a rollout's interleaved
        [T, N, 4] buffer, read in place of a1 / done. One launch; nothing is synchronised."""
        torch = self._torch
        if flags is not None:
            flags = torch.as_tensor(flags, device=self.device)
            if flags.dtype != torch.uint8 or flags.dim() != 3 or flags.shape[2] != 4 or not flags.is_contiguous():
                raise ValueError("flags must be a contiguous [T, N, 4] uint8 tensor")
            T, n = flags.shape[:2]
            a1, done = None, None
        else:
            a1 = torch.as_tensor(a1, device=self.device).to(torch.int8).contiguous()
            T, n = a1.shape
            if done is not None:
                done = torch.as_tensor(done, device=self.device).to(torch.uint8).contiguous()
                if tuple(done.shape) != (T, n):
                    raise ValueError(f"done must have shape {(T, n)}")
        obs_first = self._f32(obs_first, (n, _OBS))
        obs = self._f32(obs, (T, n, _OBS))
        rew = self._f32(rew, (T, n, 2))
        if final_obs is not None:
            final_obs = self._f32(final_obs, (T, n, _OBS))
        tr = self._nat.Transitions(ptr(obs_first), ptr(obs), ptr(final_obs), ptr(a1), ptr(rew), ptr(done), None,
                                   None, None, None, ptr(flags), None)
        self._store_call(tr, n, T)
        self._keepalive = (obs_first, obs, a1, rew, done, final_obs, flags)

    def _store_call(self, tr, n, T):
        rc = self._nat.lib.mg_rainbow_replay_store(self.memory.data_ptr(), self._counter.data_ptr(), self.capacity,
                                                   ctypes.byref(tr), n, T, self._stream())
        self._nat.check(rc, "mg_rainbow_replay_store")

    def store_rollout(self, obs_first, traj):
        """Append a MergeVecEnv rollout (the dict rollout_rainbow returns): every transition (:673). With
        autoreset the obs row of a finished env is already the reset observation, so the terminal one comes
        from final_observation."""
        self.store(obs_first, traj["obs"], traj["a1"], traj["rew"], traj["done"], self._final_observation(traj),
                   traj.get("flags"))

    def push(self, state, action, reward, next_state, done):
        """replay_buffer.push (:281-288), the reference's single call, through the same kernel."""
        d = self._torch.as_tensor([[1 if done else 0]], dtype=self._torch.uint8)
        self.store(*self._single(state, action, reward, next_state), d.to(self.device))

    def sample_rows(self, batch_size: int = 32, seed: int = 0, draw: int = 0):
        """[B, 24] rows at mg_replay_sample's Philox slots among the rows stored so far (the reference draws
        from len(storage), :322)."""
        rows = self._torch.empty((int(batch_size), ROW), dtype=self._torch.float32, device=self.device)
        return self._sample_into(rows, None, seed, draw, True)

    def sample(self, batch_size: int = 32, seed: int = 0, draw: int = 0):
        """(state [B, 10], action [B] int64, reward [B], next_state [B, 10], done [B]) -- ReplayBuffer.sample's
        five arrays (:302-323)."""
        rows = self.sample_rows(batch_size, seed, draw)
        return (rows[:, :_OBS], rows[:, _OBS].to(self._torch.int64), rows[:, _OBS + 1],
                rows[:, _OBS + 2:2 * _OBS + 2], rows[:, 2 * _OBS + 2])


def store_rainbow_rollout_many(replays, obs_first, traj):
    """Append one rollout of N = M n envs (MergeVecEnv.rollout_rainbow_many's dict; obs_first [N, 10] = the
    observation before step 0) to M RainbowReplays, member m's slice [m n, (m + 1) n) to replays[m]: exactly what
    replays[m].store_rollout leaves when given a contiguous copy of the slice, in two launches for all members
    (mg_rainbow_replay_store_many). The replays are distinct, of one capacity and on one device; a
    PrioritizedRainbowReplay is refused (its trees need store_prioritized_rollout_many). traj["flags"] is read in
    place; like store_rollout it needs the rollout's final_observation. Nothing is copied and nothing is
    synchronised."""
    _store_rollout_many("store_rainbow_rollout_many", list(replays), obs_first, traj, False)


def store_prioritized_rollout_many(replays, obs_first, traj):
    """store_rainbow_rollout_many for M PrioritizedRainbowReplays (mg_per_store_many): member m's rows, counter and
    trees are exactly what replays[m].store_rollout leaves when given a contiguous copy of its slice -- every stored
    transition enters with that replay's max_priority ** alpha. The trees' launches are the lone store's with the
    member in the grid, between the rows' launch and the counters'. The replays are distinct, of one capacity and on
    one device, each with its own alpha; a plain RainbowReplay is refused."""
    _store_rollout_many("store_prioritized_rollout_many", list(replays), obs_first, traj, True)


def _store_rollout_many(what, replays, obs_first, traj, prioritized):
    from . import _native

    M = len(replays)
    if not 1 <= M <= MAX_MEMBERS:
        raise ValueError(f"{what} takes 1..{MAX_MEMBERS} replays, got {M}")
    for r in replays:
        if isinstance(r, PrioritizedRainbowReplay) and not prioritized:
            raise ValueError("the member store writes rows only: a PrioritizedRainbowReplay's trees need its own "
                             "store_rollout")
        if not isinstance(r, PrioritizedRainbowReplay if prioritized else RainbowReplay):
            raise ValueError(f"expected {'Prioritized' if prioritized else ''}RainbowReplays, got a "
                             f"{type(r).__name__}")
    r0 = replays[0]
    torch = r0._torch
    if any(r.capacity != r0.capacity or r.device != r0.device for r in replays):
        raise ValueError("the replays share one capacity and one device")
    if len({id(r) for r in replays}) != M:
        raise ValueError("a replay is listed twice: two members' appends to one replay have no defined order")
    final_obs = RingBase._final_observation(traj)
    flags = traj.get("flags")
    if (flags is None or flags.dtype != torch.uint8 or flags.dim() != 3 or flags.shape[2] != 4
            or not flags.is_contiguous() or flags.device != r0.device):
        raise ValueError(f"the member store reads the rollout's interleaved [T, N, 4] uint8 flags buffer on {r0.device}")
    T, N = int(flags.shape[0]), int(flags.shape[1])
    if N % M:
        raise ValueError(f"N = {N} is not {M} equal slices")
    obs_first, obs = r0._f32(obs_first, (N, _OBS)), r0._f32(traj["obs"], (T, N, _OBS))
    rew, final_obs = r0._f32(traj["rew"], (T, N, 2)), r0._f32(final_obs, (T, N, _OBS))
    tr = _native.Transitions(ptr(obs_first), ptr(obs), ptr(final_obs), None, ptr(rew), None, None, None, None, None,
                             ptr(flags), None)
    rows = (ctypes.c_void_p * M)(*(r.memory.data_ptr() for r in replays))
    counters = (ctypes.c_void_p * M)(*(r._counter.data_ptr() for r in replays))
    if prioritized:
        trees = (ctypes.c_void_p * M)(*(r._tree.data_ptr() for r in replays))
        alphas = (ctypes.c_double * M)(*(r.alpha for r in replays))
        rc = _native.lib.mg_per_store_many(rows, counters, M, r0.capacity, ctypes.byref(tr), N // M, T, trees,
                                           r0._tree_bytes, alphas, r0._stream())
        _native.check(rc, "mg_per_store_many")
        return
    rc = _native.lib.mg_rainbow_replay_store_many(rows, counters, M, r0.capacity, ctypes.byref(tr), N // M, T,
                                                  r0._stream())
    _native.check(rc, "mg_rainbow_replay_store_many")


class PrioritizedRainbowReplay(RainbowReplay):
    """PrioritizedReplayBuffer(capacity, alpha) (:326-437): RainbowReplay's rows with the sum and min segment
    trees (:130-262) beside them, one fp64 device buffer (include/merging_hip.h, mg_per_bytes). A stored
    transition enters with max_priority ** alpha (:353-358); store, sample and update_priorities are
    stream-ordered launches and nothing is synchronised. The script defines the class and never builds one;
    this twin is pinned to the class itself."""

    def __init__(self, capacity: int = 10000, alpha: float = 0.6, device=None):
        super().__init__(capacity, device)
        if not alpha > 0:
            raise ValueError("alpha must be > 0")  # :342
        torch, lib = self._torch, self._nat.lib
        self.alpha = float(alpha)
        self._tree_bytes = int(lib.mg_per_bytes(self.capacity))
        self._tree = torch.empty(self._tree_bytes // 8, dtype=torch.float64, device=self.device)
        self._nat.check(lib.mg_per_init(self._tree.data_ptr(), self._tree_bytes, self.capacity, self._stream()),
                        "mg_per_init")

    def _store_call(self, tr, n, T):
        rc = self._nat.lib.mg_per_store(self.memory.data_ptr(), self._counter.data_ptr(), self.capacity,
                                        ctypes.byref(tr), n, T, self._tree.data_ptr(), self._tree_bytes, self.alpha,
                                        self._stream())
        self._nat.check(rc, "mg_per_store")

    def sample_indices(self, batch_size: int = 32, beta: float = 0.4, seed: int = 0, draw: int = 0):
        """(idxes [B] int64, weights [B] fp32) of _sample_proportional (:360-367) and the importance weights
        (:405-412), on the device; draw b takes its uniform from mg_replay_sample's Philox block (seed, draw).
        The prefix the reference draws from ends one slot short (sum(0, len - 1), :364), so the newest slot
        len - 1 is never drawn; this twin keeps that. Nothing is synchronised; fewer than two stored
        transitions give slot 0 with weight 1 (sample() refuses them)."""
        torch = self._torch
        idx = torch.empty(int(batch_size), dtype=torch.int64, device=self.device)
        w = torch.empty(int(batch_size), dtype=torch.float32, device=self.device)
        rc = self._nat.lib.mg_per_sample(self._tree.data_ptr(), self._tree_bytes, self._counter.data_ptr(),
                                         self.capacity, float(beta), seed & U64, draw & U64, int(batch_size),
                                         idx.data_ptr(), w.data_ptr(), self._stream())
        self._nat.check(rc, "mg_per_sample")
        return idx, w

    def sample(self, batch_size: int = 32, beta: float = 0.4, seed: int = 0, draw: int = 0):
        """(state, action, reward, next_state, done, weights [B] fp32, idxes [B] int64) --
        PrioritizedReplayBuffer.sample (:369-415). The newest slot is never drawn, as in the reference (see
        sample_indices). With fewer than two stored transitions the reference recurses out of its tree; this
        raises ValueError after reading the length, which synchronises."""
        if not beta > 0:
            raise ValueError("beta must be > 0")  # :401
        if len(self) < 2:
            raise ValueError("PrioritizedRainbowReplay.sample needs at least two stored transitions")
        idx, w = self.sample_indices(batch_size, beta, seed, draw)
        rows = self.memory[idx]
        return (rows[:, :_OBS], rows[:, _OBS].to(self._torch.int64), rows[:, _OBS + 1],
                rows[:, _OBS + 2:2 * _OBS + 2], rows[:, 2 * _OBS + 2], w, idx)

    def update_priorities(self, idxes, priorities):
        """update_priorities (:417-437): leaf idxes[b] := priorities[b] ** alpha, the last of a repeated index
        winning; max_priority takes every priority. Up to 1024 entries per call; an entry the reference's
        asserts reject (priority <= 0, an index outside the stored slots) is left out."""
        torch = self._torch
        idx = torch.as_tensor(idxes, device=self.device).to(torch.int64).contiguous().reshape(-1)
        pr = torch.as_tensor(priorities, device=self.device).to(torch.float32).contiguous().reshape(-1)
        if idx.numel() != pr.numel():
            raise ValueError("idxes and priorities must have the same length")  # :430
        rc = self._nat.lib.mg_per_update(self._tree.data_ptr(), self._tree_bytes, self._counter.data_ptr(),
                                         self.capacity, self.alpha, idx.data_ptr(), pr.data_ptr(), idx.numel(),
                                         self._stream())
        self._nat.check(rc, "mg_per_update")
        self._keepalive_update = (idx, pr)

    @property
    def max_priority(self):
        """_max_priority (:351, :437). Synchronises."""
        return float(self._tree[-2].item())

    def state_dict(self):
        return dict(super().state_dict(), tree=self._tree.clone(), alpha=self.alpha)

    def load_state_dict(self, sd):
        tree = self._torch.as_tensor(sd["tree"])
        if tree.numel() != self._tree.numel():
            raise ValueError(f"expected a tree of {self._tree.numel()} doubles")
        super().load_state_dict(sd)
        self._tree.copy_(tree.to(self._torch.float64).reshape(-1))
        self.alpha = float(sd["alpha"])


class _LearnerNet(RainbowNet):
    """The RainbowNet a learner owns: `packed` is the buffer mg_rainbow_learn rewrites, and the host-side
    `state` is read back from the learner's device buffer whenever a learn, a sync or a load has changed it."""

    _learner = None
    _stale = False

    @property
    def state(self):
        if self._stale and self._learner is not None:
            self._stale = False
            for k, v in self._learner.current_state_dict().items():
                self._state[k].copy_(v)
        return self._state

    @state.setter
    def state(self, value):
        self._state = value

    @property
    def packed(self):
        return self._learner._packed

    def reset_noise(self, generator=None, *, seed=None, draw=0):
        raise RuntimeError("the learner owns this net's noise: RainbowLearner.learn() redraws it")


class RainbowLearner(LearnerBase):
    _state_of = "a RainbowLearner"
    _entry, _prioritized = "mg_rainbow_learn", False

    def __init__(self, net, replay, lr: float = 0.001, gamma: float = 0.99, batch_size: int = 32, seed: int = 0,
                 generator=None, device=None, betas=(0.9, 0.999), eps: float = 1e-8):
        """net: a RainbowNet, or a RainbowDQN.state_dict(); the current and the target model both start from
        it, noise included (update_target, :648). replay: the RainbowReplay learn() draws from. lr, gamma,
        batch_size: ranbowdqn.py:645, :569, :652. seed: the key of the minibatch draws (update u draws what
        replay.sample(batch_size, seed, draw=u) returns). generator: the source of the noise draws -- a
        torch.Generator (None: torch's global one, as the reference), drawn from on the host, or a
        DeviceNoise(noise_seed), drawn by a kernel on the stream. A PrioritizedRainbowReplay takes the subclass
        PrioritizedRainbowLearner."""
        super().__init__(replay, "replay memory", device)
        torch, _native = self._torch, self._nat
        self.replay = replay
        sd = net.state if isinstance(net, RainbowNet) else net
        if isinstance(generator, DeviceNoise):  # self.noise: "torch" or "device", the mode a state dict names
            self.noise, self.generator = "device", None
            self.noise_seed = (int(seed) if generator.seed is None else generator.seed) & U64
        else:
            self.noise, self.noise_seed, self.generator = "torch", None, generator
        assert int(_native.lib.mg_rainbow_learner_bytes()) == 4 * LEARNER_FLOATS
        self._buf = learner_array(sd).to(self.device)
        if isinstance(replay, PrioritizedRainbowReplay) != self._prioritized:
            raise ValueError("a PrioritizedRainbowReplay takes a PrioritizedRainbowLearner, a RainbowReplay a "
                             "RainbowLearner")
        sbytes = int(getattr(_native.lib, self._entry + "_scratch_bytes")(int(batch_size)))
        self._setup(batch_size, seed, sbytes, lr, gamma, betas, eps)
        self._packed = torch.empty(int(_native.lib.mg_rainbow_packed_bytes()), dtype=torch.uint8, device=self.device)
        self.net = _LearnerNet(model_state_dict(self._buf, 0), training=True, device=self.device)
        self.net._learner = self
        self._call(0)

    def _call(self, U, noise=None, loss=None, rows=None, proj=None, grads=None, extra=()):
        """One call of the library's learner; extra: what the prioritized entry point takes behind the scratch."""
        rc = getattr(self._nat.lib, self._entry)(
            self._buf.data_ptr(), self.replay.memory.data_ptr(), self.replay._counter.data_ptr(),
            self.replay.capacity, self.batch_size, U, self.learn_step_counter, self.seed, self.draw_counter,
            ctypes.byref(self.hyper), ptr(noise), ptr(loss), ptr(rows), ptr(proj), ptr(grads),
            self._packed.data_ptr(), self._scratch.data_ptr(), self._scratch_bytes, *(extra or self._extra()),
            self._stream())
        self._nat.check(rc, self._entry)
        self.net._stale = True

    def _extra(self):
        return ()

    def learn(self, num_updates: int = 1, return_loss: bool = False, return_rows: bool = False,
              return_proj: bool = False, return_grads: bool = False):
        """num_updates times compute_td_loss (:584-609), enqueued back to back on the current stream, then the
        acting net repacked; nothing is synchronised. Returns None, the one requested device tensor, or a
        tuple of the requested ones in the order loss [U], rows [U, B, 24], proj [U, B, 51], grads [U, P]
        (the gradients in named_parameters() order)."""
        return self._learn(num_updates, return_loss, return_rows, return_proj, return_grads)

    def _learn(self, num_updates, return_loss, return_rows, return_proj, return_grads, more=(), extra=()):
        """more: further optional output tensors, returned behind the four; extra: see _call."""
        torch = self._torch
        U = int(num_updates)
        if U < 0:
            raise ValueError("num_updates must be >= 0")
        B = self.batch_size
        new = lambda want, *shape: torch.empty(shape, dtype=torch.float32, device=self.device) if want else None  # noqa: E731
        loss, rows = new(return_loss, U), new(return_rows, U, B, ROW)
        proj, grads = new(return_proj, U, B, NUM_ATOMS), new(return_grads, U, NUM_PARAMS)
        if U > 0:
            noise = self._noise(U)
            self._call(U, noise, loss, rows, proj, grads, extra)
            self._keepalive = noise
            self.learn_step_counter += U
            self.draw_counter += U
        out = tuple(t for t in (loss, rows, proj, grads, *more) if t is not None)
        return None if not out else out[0] if len(out) == 1 else out

    def _noise(self, U):
        """The [U, 2, 1124] factors of the next U updates on the device: torch's draws uploaded, or in device
        mode mg_rainbow_noise's on the current stream (nothing drawn or copied on the host)."""
        if self.noise == "torch":
            return noise_factors(U, self.generator).to(self.device)
        out = self._torch.empty((U, 2, NUM_FACTORS), dtype=self._torch.float32, device=self.device)
        rc = self._nat.lib.mg_rainbow_noise(self.noise_seed, self.learn_step_counter & U64, U, out.data_ptr(),
                                            self._stream())
        self._nat.check(rc, "mg_rainbow_noise")
        return out

    def sync_target(self):
        """update_target (:551-552, :690-691): target := current, noise included."""
        b = self._buf
        b[NUM_PARAMS:2 * NUM_PARAMS].copy_(b[:NUM_PARAMS])
        b[OFF_EPS + NUM_EPS:OFF_EPS + 2 * NUM_EPS].copy_(b[OFF_EPS:OFF_EPS + NUM_EPS])

    def current_state_dict(self):
        """current_model.state_dict() as ranbowdqn.py:699 saves it (copies, torch-loadable)."""
        return model_state_dict(self._buf, 0)

    def target_state_dict(self):
        return model_state_dict(self._buf, 1)

    def state_dict(self):
        """Both models with their noise, Adam's moments, the counters and the noise generator's state: a run
        resumed from it continues bit for bit. In device mode the noise needs no state beyond the counters: the
        dict carries "noise": "device" and "noise_seed" in the generator's place."""
        if self.noise == "device":
            return dict(super().state_dict(), noise="device", noise_seed=self.noise_seed)
        return dict(super().state_dict(),
                    generator=None if self.generator is None else self.generator.get_state())

    def load_state_dict(self, sd):
        theirs = sd.get("noise", "torch")
        if theirs != self.noise:
            raise ValueError(f'the state is of a learner with "{theirs}" noise, this learner draws "{self.noise}" '
                             'noise ("torch": a torch.Generator on the host, "device": a DeviceNoise): build the '
                             "learner in the state's mode")
        super().load_state_dict(sd)
        if self.noise == "device":
            self.noise_seed = int(sd["noise_seed"]) & U64
        if sd.get("generator") is not None:
            if self.generator is None:
                self.generator = self._torch.Generator()
            self.generator.set_state(sd["generator"])
        self._call(0)


class PrioritizedRainbowLearner(RainbowLearner):
    """RainbowLearner on a PrioritizedRainbowReplay (libmerging_hip.so's mg_rainbow_learn_prioritized): every
    update draws its minibatch from the tree (the draw of replay.sample_indices(batch_size, beta, seed, draw=u)),
    multiplies each row's loss by its importance weight -- loss = (loss_b * weights).mean() -- and writes
    loss_b + prio_eps back as the rows' priorities: nine launches per update, the sample before and the priority
    update behind RainbowLearner's seven, nothing synchronised. The script defines PrioritizedReplayBuffer and
    never runs it, so this use of it is the convention of the notebooks the script was taken from, not the
    script's. A row whose loss_b + prio_eps is not positive (Rainbow's loss can be negative: the gathered target
    row stays support-scaled) keeps its priority, as update_priorities' assert would refuse it."""

    _state_of = "a PrioritizedRainbowLearner"
    _entry, _prioritized = "mg_rainbow_learn_prioritized", True

    def __init__(self, net, replay, lr: float = 0.001, gamma: float = 0.99, batch_size: int = 32, seed: int = 0,
                 generator=None, device=None, betas=(0.9, 0.999), eps: float = 1e-8, beta: float = 0.4,
                 prio_eps: float = 1e-5):
        """RainbowLearner's arguments (generator: a torch.Generator or a DeviceNoise), then beta: the importance
        weights' exponent (learn() may override it per call), prio_eps: added to a row's loss to give its new
        priority."""
        if not (beta > 0 and prio_eps >= 0):
            raise ValueError("beta must be > 0 and prio_eps >= 0")
        self.beta, self.prio_eps = float(beta), float(prio_eps)
        super().__init__(net, replay, lr, gamma, batch_size, seed, generator, device, betas, eps)

    def _extra(self, beta=None, idx=None, weights=None):
        r = self.replay
        return (r._tree.data_ptr(), r._tree_bytes, r.alpha, self.beta if beta is None else float(beta), self.prio_eps,
                ptr(idx), ptr(weights))

    def learn(self, num_updates: int = 1, return_loss: bool = False, return_rows: bool = False,
              return_proj: bool = False, return_grads: bool = False, return_idx: bool = False,
              return_weights: bool = False, beta=None):
        """RainbowLearner.learn with, behind its four outputs, idx [U, B] int64 (the sampled slots) and weights
        [U, B] fp32. beta: this call's importance exponent, for an annealing schedule (default: the
        constructor's). loss [U] is the weighted mean; the rows' priorities are updated from the unweighted
        row losses."""
        if beta is not None and not beta > 0:
            raise ValueError("beta must be > 0")
        torch, U, B = self._torch, max(int(num_updates), 0), self.batch_size
        idx = torch.empty((U, B), dtype=torch.int64, device=self.device) if return_idx else None
        weights = torch.empty((U, B), dtype=torch.float32, device=self.device) if return_weights else None
        return self._learn(num_updates, return_loss, return_rows, return_proj, return_grads, (idx, weights),
                           self._extra(beta, idx, weights))
