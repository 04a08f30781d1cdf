"""RainbowPopulation: M independent RainbowLearners trained by one set of launches.

Rainbow's users sweep seeds, lr, gamma and opponents as DQN's do, and one RainbowLearner.learn() is a dependent
chain of seven small launches that leaves most of the device idle. A population runs M learners through the
same seven launches (libmerging_hip.so's mg_rainbow_learn_many), each on its own nets, replay, minibatch seed,
noise seed, counters and hyperparameters; the noise is always drawn on the device (mg_rainbow_noise_many, one
launch for all members and updates of a call), so learn() does no host work and no upload. The members act the
same way: collect() is one observe, one rollout (mg_rollout_rainbow_many, member m on its slice of one env batch
with its own net) and one store of two launches (mg_rainbow_replay_store_many) for the whole population:

    replays = [RainbowReplay(10000, device="cuda:0") for _ in range(8)]
    pop = RainbowPopulation([sd] * 8, replays, lr=[0.001, 0.0005, 0.002] + [0.001] * 5, seed=range(8))
    env = MergeVecEnv(8 * 1024, device="cuda:0")            # member m owns envs [1024 m, 1024 (m + 1))
    pop.collect(env, 16)                                    # every member acts with its own net and stores
    pop.learn(4)                                            # into its own replay; four updates of all eight
    env.member_summaries(8)                                 # each member's episode summary
    pop.sync_target([0, 3])                                 # update_target for members 0 and 3, one launch
    pop.copy_member(best, worst)                            # population-based training's exploit step

Member m is bit for bit the lone RainbowLearner(net, replay, ..., generator=DeviceNoise(noise_seed[m])) built from
the same net, replay, seeds and hyperparameters, acting through rollout_rainbow and store_rollout on a lone env
that holds its slice: member_state_dict(m) is that learner's state_dict() and loads into one, and back.

PrioritizedRainbowPopulation is the same over M PrioritizedRainbowReplays: every member draws its minibatches from
its own sum / min trees with its own alpha, beta and prio_eps, nine launches per update of the whole population
(mg_rainbow_learn_prioritized_many), and collect() stores through mg_per_store_many. Member m is bit for bit the
lone PrioritizedRainbowLearner(..., generator=DeviceNoise(noise_seed[m])):

    replays = [PrioritizedRainbowReplay(10000, alpha=a, device="cuda:0") for a in (0.4, 0.6, 0.8, 1.0)]
    pop = PrioritizedRainbowPopulation([sd] * 4, replays, seed=range(4), beta=[0.4, 0.4, 0.6, 0.6])
    pop.collect(env, 16)
    pop.learn(4, beta=0.5)                                  # beta per call: one value, or one per member

Members may meet each other or a frozen checkpoint: collect(env, T, opponent=[1, 0, checkpoint, ...]) gives member
m the current acting net of the member named by an index, or the RainbowNet given, as its opponent
(mg_rollout_rainbow_vs_many); the stored rows stay the ego's.

Not part of these classes: a league (a K x K grid of pairings in one launch), an epsilon mixture on top of the
noisy nets, storing the opponent's view of the transitions, appending to the replays from inside the rollout
kernel, and a target sync by episode count (the caller reads env.member_summaries and calls sync_target).
"""

from __future__ import annotations

import ctypes

from . import _native
from ._base import MAX_MEMBERS, per_member
from ._device import U64, cuda_device, ptr, raw_stream, require_gpu
from .rainbow import NUM_ATOMS, RainbowNet
from .rainbow_learn import (LEARNER_FLOATS, NUM_FACTORS, NUM_PARAMS, ROW, PrioritizedRainbowReplay, RainbowReplay,
                            _LearnerNet, learner_array, model_state_dict, store_prioritized_rollout_many,
                            store_rainbow_rollout_many)


class _Member:
    """What a _LearnerNet asks of its learner, for member m of a population."""

    def __init__(self, pop, m):
        self._pop, self._m = pop, m

    @property
    def _packed(self):
        return self._pop._packed[self._m]

    def current_state_dict(self):
        return self._pop.current_state_dict(self._m)


class RainbowPopulation:
    def __init__(self, nets, replays, lr=0.001, gamma=0.99, batch_size: int = 32, seed=0, noise_seed=None,
                 betas=(0.9, 0.999), eps=1e-8, device=None):
        """nets: M RainbowNets or RainbowDQN.state_dict()s; every member's current and target model both start
        from its net, noise included. replays: M RainbowReplays of one capacity on one device; the same replay may
        appear more than once (learn() only reads it). lr, gamma, betas, eps, seed and noise_seed are each one
        value applied to every member or a sequence of M; noise_seed=None gives each member its minibatch seed
        (DeviceNoise(None)'s rule). batch_size is shared."""
        torch = require_gpu(type(self).__name__)
        self._torch, self._nat = torch, _native
        nets, replays = list(nets), list(replays)
        M = len(nets)
        if not 1 <= M <= MAX_MEMBERS:
            raise ValueError(f"a population has 1..{MAX_MEMBERS} members, got {M}")
        if len(replays) != M:
            raise ValueError(f"{M} nets need {M} replays (one replay may appear more than once), got {len(replays)}")
        self._check_replays(replays)
        self.device = cuda_device(torch, device, replays[0].device)
        for r in replays:
            if r.device != self.device:
                raise ValueError(f"a replay lives on {r.device}, the population on {self.device}")
            if r.capacity != replays[0].capacity:
                raise ValueError("the replays of a population share one capacity")
        self.replays = replays
        lib = _native.lib
        self.batch_size = int(batch_size)
        one = int(getattr(lib, self._scratch_entry)(self.batch_size))
        if one == 0:
            raise ValueError("batch_size must be in 1..1024")
        lrs, gammas, epss = (per_member(v, M, n) for v, n in ((lr, "lr"), (gamma, "gamma"), (eps, "eps")))
        seeds, pairs = per_member(seed, M, "seed"), per_member(betas, M, "betas", pair=True)
        nseeds = seeds if noise_seed is None else per_member(noise_seed, M, "noise_seed")
        self._members = (_native.DqnMember * M)()
        for m in range(M):
            self._members[m] = _native.DqnMember(
                replays[m].memory.data_ptr(), replays[m]._counter.data_ptr(), int(seeds[m]) & U64, 0, 0,
                _native.DqnHyper(float(lrs[m]), float(gammas[m]), float(pairs[m][0]), float(pairs[m][1]),
                                 float(epss[m]), 1, 0))
        self._noise_seeds = (ctypes.c_uint64 * M)(*(int(s) & U64 for s in nseeds))
        assert int(lib.mg_rainbow_learner_bytes()) == 4 * LEARNER_FLOATS
        states = [n.state if isinstance(n, RainbowNet) else n for n in nets]
        self._buf = torch.stack([learner_array(sd) for sd in states]).to(self.device)
        self._scratch_bytes = one * M
        self._scratch = torch.empty(self._scratch_bytes // 4, dtype=torch.float32, device=self.device)
        self._stride = int(lib.mg_rainbow_packed_bytes())
        self._packed = torch.empty((M, self._stride), dtype=torch.uint8, device=self.device)
        self._table_bytes = int(lib.mg_rainbow_learn_many_table_bytes(M))
        self._table = torch.empty(self._table_bytes, dtype=torch.uint8, device=self.device)
        self._write_table()
        # the acting nets: `packed` is row m of the one buffer every learn() rewrites, `state` is read back lazily
        self.nets = []
        for m in range(M):
            net = _LearnerNet(model_state_dict(self._buf[m], 0), training=True, device=self.device)
            net._learner = _Member(self, m)
            self.nets.append(net)
        self._call(0)

    # ------------------------------------------------------------------ helpers
    _scratch_entry = "mg_rainbow_learn_scratch_bytes"  # the library's size of one member's scratch
    _store_many = staticmethod(store_rainbow_rollout_many)  # collect()'s store

    @staticmethod
    def _check_replays(replays):
        for r in replays:
            if isinstance(r, PrioritizedRainbowReplay):
                raise ValueError("a RainbowPopulation has no prioritized members: a PrioritizedRainbowReplay takes a "
                                 "PrioritizedRainbowPopulation, or a PrioritizedRainbowLearner of its own")
            if not isinstance(r, RainbowReplay):
                raise ValueError(f"expected RainbowReplays, got a {type(r).__name__}")

    def __len__(self):
        return len(self._members)

    def _stream(self):
        return raw_stream(self._torch, self.device)

    def _index(self, m):
        """Member index m as an int in 0 .. M - 1; anything else (a negative one too) is an IndexError."""
        M = len(self._members)
        if not 0 <= int(m) < M:
            raise IndexError(f"member {m} of a population of {M}")
        return int(m)

    def _write_table(self):
        """The device's member table (replays, seeds, gamma, Adam's constants) from the member list."""
        _native.check(_native.lib.mg_rainbow_learn_many_init(self._table.data_ptr(), self._table_bytes, self._members,
                                                             len(self._members), self._stream()),
                      "mg_rainbow_learn_many_init")

    def _call(self, U, noise=None, loss=None, rows=None, proj=None, grads=None):
        """One call of mg_rainbow_learn_many (U == 0: the effective weights and the pack alone); on success it
        has advanced the members' counters."""
        rc = _native.lib.mg_rainbow_learn_many(
            self._buf.data_ptr(), self._table.data_ptr(), self._table_bytes, self._members, len(self._members),
            self.replays[0].capacity, self.batch_size, U, ptr(noise), ptr(loss), ptr(rows), ptr(proj), ptr(grads),
            self._packed.data_ptr(), self._stride, self._scratch.data_ptr(), self._scratch_bytes, self._stream())
        _native.check(rc, "mg_rainbow_learn_many")
        for net in self.nets:
            net._stale = True

    @property
    def learn_step_counter(self):
        """Per member, the updates made so far (Adam's step count, the noise stream's update index)."""
        return [int(e.first_update) for e in self._members]

    @property
    def draw_counter(self):
        """Per member, the minibatches drawn so far."""
        return [int(e.first_draw) for e in self._members]

    @property
    def seed(self):
        return [int(e.seed) for e in self._members]

    @property
    def noise_seed(self):
        return [int(s) for s in self._noise_seeds]

    # ------------------------------------------------------------------ act and store
    def collect(self, env, num_steps: int, opponent="self"):
        """The acting half of the loop for every member at once: env.observe(), one
        env.rollout_rainbow_many(num_steps, self.nets, opponent) -- member m on its slice of env's batch -- and one
        store_rainbow_rollout_many into self.replays: four launches beside the 4 M of the members in turn, each
        member's slice, replay and counter bit for bit the lone loop's. opponent: "self" or "none" for every
        member, or a list of M items, item m a member index (member m plays against that member's current acting
        net: cross-play) or a RainbowNet (a frozen checkpoint); an index outside 0 .. M - 1 is a ValueError. The
        stored rows are the ego's either way. Returns the trajectory. Refuses a population whose replays are
        shared."""
        if len({id(r) for r in self.replays}) != len(self.replays):
            raise ValueError("collect() appends each member's transitions to its own ring: this population's "
                             "rings are shared")
        if not isinstance(opponent, str):
            M = len(self.nets)
            opponent = list(opponent)
            if len(opponent) != M:
                raise ValueError(f"{M} members need {M} opponents (one per member), got {len(opponent)}")
            for m, o in enumerate(opponent):
                if isinstance(o, RainbowNet):
                    continue
                if isinstance(o, bool) or not isinstance(o, int) or not 0 <= o < M:
                    raise ValueError(f"opponent[{m}] = {o!r}: a member index in 0..{M - 1} or a RainbowNet")
                opponent[m] = self.nets[o]
        obs0 = env.observe()
        traj = env.rollout_rainbow_many(num_steps, self.nets, opponent)
        self._store_many(self.replays, obs0, traj)
        return traj

    # ------------------------------------------------------------------ learn
    def learn(self, num_updates: int = 1, return_loss: bool = False, return_rows: bool = False,
              return_proj: bool = False, return_grads: bool = False):
        """num_updates times compute_td_loss for every member, enqueued back to back on the current stream: one
        launch for all the noise factors, seven per update of the whole population, one for the acting nets;
        nothing is synchronised and nothing is drawn or uploaded by the host. Returns None, the one requested
        device tensor, or a tuple of the requested ones in the order loss [U, M], rows [U, M, B, 24], proj
        [U, M, B, 51], grads [U, M, P]."""
        return self._learn(num_updates, return_loss, return_rows, return_proj, return_grads)

    def _learn(self, num_updates, return_loss, return_rows, return_proj, return_grads, more=(), **extra):
        """more: further optional output tensors, returned behind the four; extra: what _call takes besides."""
        torch = self._torch
        U, M, B = int(num_updates), len(self._members), self.batch_size
        if U < 0:
            raise ValueError("num_updates must be >= 0")
        new = lambda want, *shape: torch.empty(shape, dtype=torch.float32, device=self.device) if want else None  # noqa: E731
        loss, rows = new(return_loss, U, M), new(return_rows, U, M, B, ROW)
        proj, grads = new(return_proj, U, M, B, NUM_ATOMS), new(return_grads, U, M, NUM_PARAMS)
        if U > 0:
            noise = torch.empty((U, M, 2, NUM_FACTORS), dtype=torch.float32, device=self.device)
            first = (ctypes.c_uint64 * M)(*(e.first_update for e in self._members))
            rc = _native.lib.mg_rainbow_noise_many(self._noise_seeds, first, M, U, noise.data_ptr(), self._stream())
            _native.check(rc, "mg_rainbow_noise_many")
            self._call(U, noise, loss, rows, proj, grads, **extra)  # `noise` may go: the allocator is stream-ordered
        out = tuple(t for t in (loss, rows, proj, grads, *more) if t is not None)
        return None if not out else out[0] if len(out) == 1 else out

    def sync_target(self, members=None):
        """update_target (:551-552, :690-691) -- target := current, noise included -- for all members or for an
        iterable of member indices, in one launch."""
        M = len(self._members)
        mask = 0
        for m in range(M) if members is None else members:
            mask |= 1 << self._index(m)
        rc = _native.lib.mg_rainbow_sync_target_many(self._buf.data_ptr(), M, mask, self._stream())
        _native.check(rc, "mg_rainbow_sync_target_many")

    # ------------------------------------------------------------------ checkpoints
    def current_state_dict(self, m):
        """Member m's current_model.state_dict() as ranbowdqn.py:699 saves it (copies, torch-loadable)."""
        return model_state_dict(self._buf[self._index(m)], 0)

    def target_state_dict(self, m):
        return model_state_dict(self._buf[self._index(m)], 1)

    def member_state_dict(self, m):
        """Exactly the state_dict() of the lone RainbowLearner(..., generator=DeviceNoise(noise_seed[m])) member m
        equals: it loads into one."""
        m = self._index(m)
        e = self._members[m]
        return {"learner": self._buf[m].clone(), "learn_step_counter": int(e.first_update),
                "draw_counter": int(e.first_draw), "seed": int(e.seed), "noise": "device",
                "noise_seed": int(self._noise_seeds[m])}

    @staticmethod
    def _device_noise_state(sd):
        if sd.get("noise", "torch") != "device":
            raise ValueError('the state is of a learner with "torch" noise; a population draws "device" noise '
                             "(a RainbowLearner built with generator=DeviceNoise(...))")

    def _take_member(self, m, buf, step, draw, seed, noise_seed):
        self._buf[m].copy_(self._torch.as_tensor(buf).to(self._torch.float32).reshape(-1))
        e = self._members[m]
        e.first_update, e.first_draw, e.seed = int(step), int(draw), int(seed) & U64
        self._noise_seeds[m] = int(noise_seed) & U64

    def load_member_state_dict(self, m, sd):
        """A device-noise RainbowLearner's state_dict() (or member_state_dict()) into member m: nets, noise,
        moments, counters and seeds."""
        m = self._index(m)
        self._device_noise_state(sd)
        if self._torch.as_tensor(sd["learner"]).numel() != LEARNER_FLOATS:
            raise ValueError("expected the state of a RainbowLearner")
        self._take_member(m, sd["learner"], sd["learn_step_counter"], sd["draw_counter"], sd["seed"],
                          sd["noise_seed"])
        self._write_table()
        self._call(0)

    def state_dict(self):
        """Every member's models with their noise, moments, counters and seeds: a run resumed from it continues
        bit for bit."""
        return {"learners": self._buf.clone(), "learn_step_counter": self.learn_step_counter,
                "draw_counter": self.draw_counter, "seed": self.seed, "noise": "device",
                "noise_seed": self.noise_seed}

    def load_state_dict(self, sd):
        self._device_noise_state(sd)
        buf = self._torch.as_tensor(sd["learners"])
        if tuple(buf.shape) != tuple(self._buf.shape):
            raise ValueError(f"expected the state of {len(self)} Rainbow learners")
        for m in range(len(self)):
            self._take_member(m, buf[m], sd["learn_step_counter"][m], sd["draw_counter"][m], sd["seed"][m],
                              sd["noise_seed"][m])
        self._write_table()
        self._call(0)

    def copy_member(self, src, dst):
        """Population-based training's exploit step: dst takes src's nets, noise blocks, Adam moments and counters
        (a device-side copy) and is repacked for acting; it keeps its own seeds, replay and hyperparameters."""
        src, dst = self._index(src), self._index(dst)
        if src == dst:
            return
        self._buf[dst].copy_(self._buf[src])
        self._members[dst].first_update = self._members[src].first_update
        self._members[dst].first_draw = self._members[src].first_draw
        self._call(0)


class PrioritizedRainbowPopulation(RainbowPopulation):
    """RainbowPopulation over M PrioritizedRainbowReplays (libmerging_hip.so's mg_rainbow_learn_prioritized_many):
    every update draws each member's minibatch from its own tree, weights its rows' losses and writes loss_b +
    prio_eps back as their priorities -- PrioritizedRainbowLearner's nine launches, for all members at once, nothing
    synchronised. The trees belong to the replays, as in the lone class: copy_member copies no tree, and a
    checkpoint of the population holds none (the replays' state_dict() does)."""

    _scratch_entry = "mg_rainbow_learn_prioritized_scratch_bytes"
    _store_many = staticmethod(store_prioritized_rollout_many)

    def __init__(self, nets, replays, lr=0.001, gamma=0.99, batch_size: int = 32, seed=0, noise_seed=None,
                 betas=(0.9, 0.999), eps=1e-8, device=None, beta=0.4, prio_eps=1e-5):
        """RainbowPopulation's arguments, with replays M distinct PrioritizedRainbowReplays of one capacity on one
        device, each with its own alpha (learning writes a member's tree, so a shared replay has no defined order);
        then beta -- the importance weights' exponent, which learn() may override per call -- and prio_eps, each
        one value or a sequence of M."""
        replays = list(replays)
        self.beta = self._betas(beta, len(replays))
        self.prio_eps = [float(v) for v in per_member(prio_eps, len(replays), "prio_eps")]
        if not all(v >= 0 for v in self.prio_eps):
            raise ValueError("prio_eps must be >= 0")
        super().__init__(nets, replays, lr, gamma, batch_size, seed, noise_seed, betas, eps, device)

    @staticmethod
    def _betas(beta, M):
        out = [float(v) for v in per_member(beta, M, "beta")]
        if not all(v > 0 for v in out):
            raise ValueError("beta must be > 0")
        return out

    @staticmethod
    def _check_replays(replays):
        for r in replays:
            if not isinstance(r, PrioritizedRainbowReplay):
                raise ValueError(f"expected PrioritizedRainbowReplays, got a {type(r).__name__} (a RainbowReplay "
                                 "takes a RainbowPopulation)")
        if len({id(r) for r in replays}) != len(replays):
            raise ValueError("a replay is listed twice: learning writes a member's tree, so two members on one "
                             "replay have no defined order")

    def _call(self, U, noise=None, loss=None, rows=None, proj=None, grads=None, beta=None, idx=None, weights=None):
        """One call of mg_rainbow_learn_prioritized_many (see RainbowPopulation._call)."""
        M = len(self._members)
        per = (_native.PerMember * M)(*(
            _native.PerMember(r._tree.data_ptr(), r.alpha, b, e)
            for r, b, e in zip(self.replays, self.beta if beta is None else beta, self.prio_eps)))
        rc = _native.lib.mg_rainbow_learn_prioritized_many(
            self._buf.data_ptr(), self._table.data_ptr(), self._table_bytes, self._members, M,
            self.replays[0].capacity, self.batch_size, U, ptr(noise), ptr(loss), ptr(rows), ptr(proj), ptr(grads),
            self._packed.data_ptr(), self._stride, self._scratch.data_ptr(), self._scratch_bytes, per,
            self.replays[0]._tree_bytes, ptr(idx), ptr(weights), self._stream())
        _native.check(rc, "mg_rainbow_learn_prioritized_many")
        for net in self.nets:
            net._stale = True

    def learn(self, num_updates: int = 1, return_loss: bool = False, return_rows: bool = False,
              return_proj: bool = False, return_grads: bool = False, return_idx: bool = False,
              return_weights: bool = False, beta=None):
        """RainbowPopulation.learn with, behind its four outputs, idx [U, M, B] int64 (the sampled slots) and
        weights [U, M, B] fp32. beta: this call's importance exponents, one value or a sequence of M (default:
        the constructor's). loss [U, M] is each member's weighted mean; the priorities are updated from the
        unweighted row losses."""
        torch, M, B = self._torch, len(self._members), self.batch_size
        beta = None if beta is None else self._betas(beta, M)
        U = max(int(num_updates), 0)
        idx = torch.empty((U, M, B), dtype=torch.int64, device=self.device) if return_idx else None
        weights = torch.empty((U, M, B), dtype=torch.float32, device=self.device) if return_weights else None
        return self._learn(num_updates, return_loss, return_rows, return_proj, return_grads, (idx, weights),
                           beta=beta, idx=idx, weights=weights)
