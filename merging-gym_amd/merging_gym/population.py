"""DQNPopulation: M independent DQNLearners trained by one set of launches.

What the reference's users do with its scripts is train many agents -- sweeps over the reward parameters,
L1 against L0 and then against L1, hdqn.py's two nets -- and one DQNLearner.learn() is a dependent chain
of seven small launches that leaves most of the device idle. A population runs M learners of one shape
through the same seven launches (libmerging_hip.so's mg_dqn_learn_many), each on its own net, replay
ring, seed, counters and hyperparameters:

    rings = [ReplayRing(2000, device="cuda:0") for _ in range(8)]
    pop = DQNPopulation([sd] * 8, rings, lr=[0.01, 0.005, 0.02, 0.01, 0.01, 0.01, 0.01, 0.01], seed=range(8))
    env = MergeVecEnv(8 * 1024, device="cuda:0")            # member m owns envs [1024 m, 1024 (m + 1))
    pop.collect(env, 16)                                    # every member acts with its own net and stores
    pop.learn(4)                                            # into its own ring; four updates of all eight
    pay = pop.cross_play(league_env, 64)                    # [8, 8] payoff matrices: ego i against opponent j
    pop.copy_member(best, worst)                            # population-based training's exploit step

Member m is bit for bit the lone DQNLearner built from the same net, ring, seed and hyperparameters:
member_state_dict(m) is that learner's state_dict() and loads into one, and back.
"""

from __future__ import annotations

from . import _native
from ._base import MAX_MEMBERS, DQNNets, per_member
from ._device import U64, cuda_device, ptr, raw_stream, require_gpu

class DQNPopulation(DQNNets):
    def __init__(self, nets, rings, lr=0.01, gamma=0.9, batch_size: int = 128, target_period=100,
                 betas=(0.9, 0.999), eps=1e-8, seed=0, device=None):
        """nets: M QNets or state dicts with the reference's keys (fc1.weight ... out.bias), all of one
        shape. rings: M ReplayRings of one capacity and row width on one device; the same ring may appear
        more than once (learn() only reads it). lr, gamma, target_period, betas, eps and seed are each one
        value applied to every member -- the seed too, so members on one ring with one seed draw the same
        minibatches -- or a sequence of M. batch_size is shared."""
        torch = require_gpu(type(self).__name__)
        self._torch, self._nat = torch, _native
        nets, rings = list(nets), list(rings)
        M = len(nets)
        if not 1 <= M <= MAX_MEMBERS:
            raise ValueError(f"a population has 1..{MAX_MEMBERS} members, got {M}")
        if len(rings) != M:
            raise ValueError(f"{M} nets need {M} rings (one ring may appear more than once), got {len(rings)}")
        self.device = cuda_device(torch, device, rings[0].device)
        ring0 = rings[0]
        for r in rings:
            if r.device != self.device:
                raise ValueError(f"a ring lives on {r.device}, the population on {self.device}")
            if (r.capacity, r.row) != (ring0.capacity, ring0.row):
                raise ValueError("the rings of a population share one capacity and row width")
        self.rings = rings
        tensors = [self._net_tensors(net, "a", "population") for net in nets]
        if len({(int(ts[0].shape[1]), int(ts[4].shape[0])) for ts in tensors}) != 1:
            raise ValueError("the nets of a population share one shape")
        self._set_shape(tensors[0], ring0.row, "rings'")
        lib = _native.lib
        self.batch_size = int(batch_size)
        one = int(lib.mg_dqn_learn_scratch_bytes(self.batch_size, self.in_dim, self.out_dim))
        if one == 0:
            raise ValueError("batch_size must be in 1..1024")
        lrs, gammas, epss = (per_member(v, M, n) for v, n in ((lr, "lr"), (gamma, "gamma"), (eps, "eps")))
        periods, seeds = per_member(target_period, M, "target_period"), per_member(seed, M, "seed")
        pairs = per_member(betas, M, "betas", pair=True)
        self._members = (_native.DqnMember * M)()
        for m in range(M):
            self._members[m] = _native.DqnMember(
                rings[m].memory.data_ptr(), rings[m]._counter.data_ptr(), int(seeds[m]) & U64, 0, 0,
                _native.DqnHyper(float(lrs[m]), float(gammas[m]), float(pairs[m][0]), float(pairs[m][1]),
                                 float(epss[m]), int(periods[m]), 0))
        self._buf = torch.empty((M, 4 * self._P), dtype=torch.float32, device=self.device)
        self._scratch_bytes = one * M
        self._scratch = torch.empty(self._scratch_bytes // 4, dtype=torch.float32, device=self.device)
        self._stride = int(lib.mg_qnet_packed_bytes())
        self._packed = torch.empty((M, self._stride), dtype=torch.uint8, device=self.device)
        self._table_bytes = int(lib.mg_dqn_learn_many_table_bytes(M))
        self._table = torch.empty(self._table_bytes, dtype=torch.uint8, device=self.device)
        self._write_table()
        # the acting nets: their fp32 tensors are views of the members' eval blocks, their packed
        # buffers rows of one buffer that every learn() rewrites
        self.qnets = [self._init_learner(self._buf[m], nets[m], tensors[m], self._packed[m]) for m in range(M)]

    # ------------------------------------------------------------------ helpers
    def __len__(self):
        return len(self._members)

    def _stream(self):
        return raw_stream(self._torch, self.device)

    def _write_table(self):
        """The device's member table (rings, seeds, gamma, Adam's constants) from the member list."""
        _native.check(_native.lib.mg_dqn_learn_many_init(self._table.data_ptr(), self._table_bytes, self._members,
                                                         len(self._members), self._stream()),
                      "mg_dqn_learn_many_init")

    def _repack(self, m):
        self._pack(self._buf[m], self.qnets[m])  # into qnets[m].packed, row m of _packed

    @property
    def learn_step_counter(self):
        """Per member, the updates made so far (Adam's step count, the target copy's clock)."""
        return [int(e.first_update) for e in self._members]

    @property
    def draw_counter(self):
        """Per member, the minibatches drawn so far."""
        return [int(e.first_draw) for e in self._members]

    @property
    def seed(self):
        return [int(e.seed) for e in self._members]

    # ------------------------------------------------------------------ act and store
    def collect(self, env, num_steps: int, seed=None, opponent="none", episilo=0.7, opp_episilo=0.7,
                skip_ego_won: bool = True):
        """The acting half of the loop for every member at once: env.observe(), one
        env.rollout_qnet_many(num_steps, self.qnets, ...) -- member m on its slice of env's batch -- and one
        replay.store_rollout_many into self.rings: four launches beside the M rollouts and 3 M stores of the
        members in turn, each member's slice, ring and counter bit for bit the lone loop's. seed: one value or
        M (None: the members' own seeds); opponent, episilo, opp_episilo as rollout_qnet_many takes them.
        Returns the trajectory. Refuses a population whose rings are shared."""
        from .replay import store_rollout_many

        if len({id(r) for r in self.rings}) != len(self.rings):
            raise ValueError("collect() appends each member's transitions to its own ring: this population's "
                             "rings are shared")
        obs0 = env.observe()
        traj = env.rollout_qnet_many(num_steps, self.qnets, self.seed if seed is None else seed, opponent, episilo,
                                     opp_episilo)
        store_rollout_many(self.rings, obs0, traj, skip_ego_won)
        return traj

    # ------------------------------------------------------------------ evaluate
    def cross_play(self, env, num_steps: int, seed=None, episilo=0.7):
        """The league's payoff matrices: every member as ego against every member as opponent, K = len(self).
        Exactly env.clear_statistics(), env.rollout_qnet_league(num_steps, self.qnets, seed, episilo,
        trajectory=False) and env.league_summary(K): three launches (the rollout of all K^2 pairings, the two of
        the segmented reduction) and one host copy, whatever K is. env holds K^2 slices of a multiple of 64
        envs; pairing (i, j) plays on slice i K + j. seed: one value or K (None: the members' own seeds);
        episilo: one value or K, each net's exploration on either side. Nothing is stored in the rings and the
        learners are untouched; env's earlier statistics are cleared, and its envs move on num_steps steps.

        Returns a dict with episode_summary()'s keys, each a [K, K] float64 CPU tensor (`completed`: int64):
        entry [i, j] is that quantity over the episodes ego i completed against opponent j. Row i is how member
        i fares as the ego, column i what the others achieve against it. A fitness for the exploit step:

            pay = pop.cross_play(env, 64)
            win, ret = pay["win_rate_main"], pay["mean_return_ego"]
            fitness = win.mean(1) - win.mean(0) + 0.01 * (ret.mean(1) - ret.mean(0))   # [K]
            pop.copy_member(int(fitness.argmax()), int(fitness.argmin()))

        The diagonal is a member against a copy of itself (the other-net path, not opponent="self"). Frozen
        checkpoints are evaluated by env.rollout_qnet_league(num_steps, self.qnets + frozen_qnets, ...) on an
        env of (K + F)^2 slices and reading the sub-block of env.league_summary(K + F); there is no
        rectangular form."""
        env.clear_statistics()
        env.rollout_qnet_league(num_steps, self.qnets, self.seed if seed is None else seed, episilo, trajectory=False)
        return env.league_summary(len(self))

    # ------------------------------------------------------------------ learn
    def learn(self, num_updates: int = 1, filled_only: bool = False, return_loss: bool = False,
              return_rows: bool = False):
        """num_updates updates of every member, enqueued back to back on the current stream: seven launches
        per update of the whole population (eight when a member's target copy is due), two per call for
        the acting nets; nothing is synchronised. filled_only draws from the rows each member's ring has
        stored so far. return_loss: the [num_updates, M] fp32 device tensor of the MSE losses; return_rows:
        also the [num_updates, M, B, row] minibatches."""
        torch = self._torch
        U, M = int(num_updates), len(self._members)
        if U < 0:
            raise ValueError("num_updates must be >= 0")
        row = self.rings[0].row
        loss = torch.empty((U, M), dtype=torch.float32, device=self.device) if return_loss else None
        rows = torch.empty((U, M, self.batch_size, row), dtype=torch.float32,
                           device=self.device) if return_rows else None
        if U > 0:
            rc = _native.lib.mg_dqn_learn_many(
                self._buf.data_ptr(), self._table.data_ptr(), self._table_bytes, self._members, M,
                self.rings[0].capacity, row, self.in_dim, self.out_dim, self.batch_size, U, 1 if filled_only else 0,
                ptr(loss), ptr(rows), self._packed.data_ptr(), self._stride, self._scratch.data_ptr(),
                self._scratch_bytes, self._stream())
            _native.check(rc, "mg_dqn_learn_many")  # the call advanced the members' counters
            for q in self.qnets:
                self._new_weights(q)
        if return_loss and return_rows:
            return loss, rows
        return loss if return_loss else rows

    # ------------------------------------------------------------------ checkpoints
    def eval_state_dict(self, m):
        """Member m's eval_net.state_dict() as main.py:244 saves it (copies, torch-loadable)."""
        return self._net_state_dict(self._buf[m], 0)

    def target_state_dict(self, m):
        """Member m's target_net.state_dict() as main.py:245 saves it."""
        return self._net_state_dict(self._buf[m], 1)

    def member_state_dict(self, m):
        """Exactly the state_dict() of the lone DQNLearner member m equals: it loads into one."""
        e = self._members[m]
        return {"learner": self._buf[m].clone(), "learn_step_counter": int(e.first_update),
                "draw_counter": int(e.first_draw), "seed": int(e.seed), "in_dim": self.in_dim,
                "out_dim": self.out_dim}

    def load_member_state_dict(self, m, sd):
        """A DQNLearner's state_dict() (or member_state_dict()) into member m: nets, moments, counters, seed."""
        self._buf[m].copy_(self._learner_state(sd).to(self._torch.float32).reshape(-1))
        e = self._members[m]
        e.first_update, e.first_draw = int(sd["learn_step_counter"]), int(sd["draw_counter"])
        e.seed = int(sd["seed"]) & U64
        self._write_table()
        self._repack(m)

    def state_dict(self):
        """Every member's nets, moments, counters and seed: a run resumed from it continues bit for bit."""
        return {"learners": self._buf.clone(), "learn_step_counter": self.learn_step_counter,
                "draw_counter": self.draw_counter, "seed": self.seed, "in_dim": self.in_dim,
                "out_dim": self.out_dim}

    def load_state_dict(self, sd):
        buf = self._torch.as_tensor(sd["learners"])
        if (int(sd["in_dim"]), int(sd["out_dim"])) != (self.in_dim, self.out_dim) or \
                tuple(buf.shape) != tuple(self._buf.shape):
            raise ValueError(f"expected the state of {len(self)} {self.in_dim} -> {self.out_dim} learners")
        self._buf.copy_(buf.to(self._torch.float32))
        for m, e in enumerate(self._members):
            e.first_update, e.first_draw = int(sd["learn_step_counter"][m]), int(sd["draw_counter"][m])
            e.seed = int(sd["seed"][m]) & U64
        self._write_table()
        for m in range(len(self)):
            self._repack(m)

    def copy_member(self, src, dst):
        """Population-based training's exploit step: dst takes src's nets, Adam moments and counters (a
        device-side copy) and is repacked for acting; it keeps its own seed, ring and hyperparameters."""
        src, dst = int(src), int(dst)
        if src == dst:
            return
        self._buf[dst].copy_(self._buf[src])
        self._members[dst].first_update = self._members[src].first_update
        self._members[dst].first_draw = self._members[src].first_draw
        self._repack(dst)
