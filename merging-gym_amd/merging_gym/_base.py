"""What the two replay rings (ReplayRing, RainbowReplay) and the two learners (DQNLearner, RainbowLearner)
share: the device buffers, the stream, the sample call, the counters and the checkpoint code; and what
DQNLearner and DQNPopulation share of a DQN net's handling (DQNNets)."""

from ._device import U64, cuda_device, raw_stream, require_gpu
from .policy import QNet

MAX_MEMBERS = 64  # the members one call takes: actors of a rollout, rings of a store, learners of a population


def per_member(value, members, name, pair=False):
    """`value` for every member: a scalar (a pair, for betas) applied to all, or a sequence of `members`."""
    shared = not hasattr(value, "__len__") and not hasattr(value, "__iter__")
    if pair:
        value = list(value)
        shared = len(value) == 2 and not hasattr(value[0], "__len__")
    if shared:
        return [value] * members
    value = list(value)
    if len(value) != members:
        raise ValueError(f"{name}: expected one value or {members}, got {len(value)}")
    return value


class RingBase:
    """[capacity, row] fp32 rows on the device; the position is a device counter, so stores are stream-ordered."""

    def __init__(self, capacity, row, device):
        torch = require_gpu(type(self).__name__)
        from . import _native

        if capacity < 1:
            raise ValueError("capacity must be >= 1")
        self._torch, self._nat = torch, _native
        self.capacity, self.row = int(capacity), row
        self.device = cuda_device(torch, device)
        self.memory = torch.zeros((self.capacity, row), dtype=torch.float32, device=self.device)
        self._counter = torch.zeros(1, dtype=torch.int64, device=self.device)

    def _stream(self):
        return raw_stream(self._torch, self.device)

    def _f32(self, t, shape):
        torch = self._torch
        t = torch.as_tensor(t, device=self.device)
        if t.dtype != torch.float32 or not t.is_contiguous():
            t = t.to(torch.float32).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _single(self, state, action, reward, next_state):
        """One transition as store()'s first four arguments: obs_first [1, 10], obs [1, 1, 10], a1, rew."""
        torch = self._torch
        s = torch.as_tensor([list(map(float, state))], dtype=torch.float32)
        s2 = torch.as_tensor([[list(map(float, next_state))]], dtype=torch.float32)
        a = torch.as_tensor([[int(action)]], dtype=torch.int8)
        r = torch.as_tensor([[[float(reward), 0.0]]], dtype=torch.float32)
        return s.to(self.device), s2.to(self.device), a.to(self.device), r.to(self.device)

    @staticmethod
    def _final_observation(traj):
        if traj.get("final_observation") is None:
            raise ValueError("the rollout has no final_observation: episode ends would store the "
                             "reset observation as next_state; roll out with final_observation=True")
        return traj["final_observation"]

    def _sample_into(self, rows, idx, seed, draw, filled_only):
        """mg_replay_sample's draw of len(rows) rows into `rows`, their slots into `idx` (or None)."""
        rc = self._nat.lib.mg_replay_sample(
            self.memory.data_ptr(), self._counter.data_ptr(), self.capacity, self.row, seed & U64, draw & U64,
            1 if filled_only else 0, rows.data_ptr(), None if idx is None else idx.data_ptr(), rows.shape[0],
            self._stream())
        self._nat.check(rc, "mg_replay_sample")
        return rows

    def state_dict(self):
        return {"memory": self.memory.clone(), "counter": self._counter.clone()}

    def load_state_dict(self, sd):
        mem = self._torch.as_tensor(sd["memory"])
        if tuple(mem.shape) != tuple(self.memory.shape):
            raise ValueError(f"expected a {tuple(self.memory.shape)} replay memory")
        self.memory.copy_(mem)
        self._counter.copy_(self._torch.as_tensor(sd["counter"]))


class LearnerBase:
    """The learner buffer `_buf` (the subclass fills it), the scratch, Adam's hyperparameters, the counters."""

    def __init__(self, ring, ring_name, device):
        torch = require_gpu(type(self).__name__)
        from . import _native

        self._torch, self._nat = torch, _native
        self.device = cuda_device(torch, device, ring.device)
        if self.device != ring.device:
            raise ValueError(f"the {ring_name} lives on {ring.device}, the learner on {self.device}")

    def _setup(self, batch_size, seed, scratch_bytes, lr, gamma, betas, eps, target_period=1):
        """scratch_bytes: the library's mg_*_learn_scratch_bytes for this batch size (0: refused)."""
        self.batch_size = int(batch_size)
        self.hyper = self._nat.DqnHyper(float(lr), float(gamma), float(betas[0]), float(betas[1]), float(eps),
                                        int(target_period), 0)
        self.seed = int(seed) & U64
        self.learn_step_counter = 0  # Adam's step count (main.py:90, :127) -- a Python int: no device round trip
        self.draw_counter = 0        # minibatches drawn so far
        if scratch_bytes == 0:
            raise ValueError("batch_size must be in 1..1024")
        self._scratch = self._torch.empty(scratch_bytes // 4, dtype=self._torch.float32, device=self.device)
        self._scratch_bytes = scratch_bytes

    def _stream(self):
        return raw_stream(self._torch, self.device)

    def state_dict(self):
        return {"learner": self._buf.clone(), "learn_step_counter": self.learn_step_counter,
                "draw_counter": self.draw_counter, "seed": self.seed}

    def load_state_dict(self, sd):
        buf = self._torch.as_tensor(sd["learner"])
        if buf.numel() != self._buf.numel():
            raise ValueError(f"expected the state of {self._state_of}")  # the subclass names itself
        self._buf.copy_(buf.to(self._torch.float32).reshape(-1))
        self.learn_step_counter = int(sd["learn_step_counter"])
        self.draw_counter = int(sd["draw_counter"])
        self.seed = int(sd["seed"]) & U64


DQN_KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "out.weight", "out.bias")


class DQNNets:
    """What DQNLearner and DQNPopulation share: a net's intake, the shape checks, the views of a flat [4 P]
    learner buffer, its repack for acting and the check of a learner's state. Uses _torch, _nat, device, _stream()."""

    def _net_tensors(self, net, a, owner):
        """A QNet or a state dict with the reference's keys as six contiguous fp32 tensors on the device."""
        torch = self._torch
        if isinstance(net, QNet):
            if torch.device(net.device.type, net.device.index or 0) != self.device:
                raise ValueError(f"{a} QNet lives on {net.device}, the {owner} on {self.device}")
            return list(net.fp32)
        return [torch.as_tensor(net[k], dtype=torch.float32).to(self.device).contiguous() for k in DQN_KEYS]

    def _set_shape(self, tensors, row, rings):
        """in_dim, out_dim and _P (the floats of one block) of a net, which must fit the rows it learns from."""
        self.in_dim, self.out_dim = int(tensors[0].shape[1]), int(tensors[4].shape[0])
        if row != 2 * self.in_dim + 2:
            raise ValueError(f"a net on {self.in_dim} inputs learns from rows of {2 * self.in_dim + 2} floats; "
                             f"the {rings} have {row}")
        nbytes = int(self._nat.lib.mg_dqn_learner_bytes(self.in_dim, self.out_dim))
        if nbytes == 0:
            raise ValueError("expected the reference Net with 1 <= in <= 13 and 1 <= out <= 8")
        self._P = nbytes // 16

    def _block_views(self, learner, block):
        """The six tensors of a learner's block 0 (eval), 1 (target), 2 (Adam's m) or 3 (v): views, no copies."""
        shapes = ((200, self.in_dim), (200,), (100, 200), (100,), (self.out_dim, 100), (self.out_dim,))
        parts = learner[block * self._P:(block + 1) * self._P].split([s[0] * (s[1:] or (1,))[0] for s in shapes])
        return [p.view(s) for p, s in zip(parts, shapes)]

    def _init_learner(self, learner, net, tensors, packed=None):
        """Fills a learner buffer from a net's tensors (eval = target, zero moments) and returns its acting net:
        `net` itself if it is a QNet, its fp32 tensors now views of the eval block; with `packed`, packing there."""
        rc = self._nat.lib.mg_dqn_learner_init(learner.data_ptr(), *(t.data_ptr() for t in tensors), self.in_dim,
                                               self.out_dim, self._stream())
        self._nat.check(rc, "mg_dqn_learner_init")
        qnet = net if isinstance(net, QNet) else QNet(*self._block_views(learner, 0), device=self.device)
        qnet.fp32 = self._block_views(learner, 0)
        if packed is not None:
            qnet.packed = packed
            self._pack(learner, qnet)
        self._new_weights(qnet)
        return qnet

    def _net_state_dict(self, learner, block):
        return {k: t.clone() for k, t in zip(DQN_KEYS, self._block_views(learner, block))}

    @staticmethod
    def _new_weights(qnet):
        """The acting net's weights changed: what it derived from the old ones goes."""
        qnet.__dict__.pop("_reset_argmax", None)

    def _pack(self, learner, qnet):
        """The learner's eval block into qnet's packed buffer, for the acting kernels."""
        rc = self._nat.lib.mg_qnet_pack(*(t.data_ptr() for t in self._block_views(learner, 0)), self.in_dim,
                                        self.out_dim, qnet.packed.data_ptr(), self._stream())
        self._nat.check(rc, "mg_qnet_pack")
        self._new_weights(qnet)

    def _learner_state(self, sd):
        """The learner buffer in a DQNLearner's state dict, as a tensor; another shape's is refused."""
        buf = self._torch.as_tensor(sd["learner"])
        if (int(sd["in_dim"]), int(sd["out_dim"])) != (self.in_dim, self.out_dim) or buf.numel() != 4 * self._P:
            raise ValueError(f"expected the state of a {self.in_dim} -> {self.out_dim} learner")
        return buf
