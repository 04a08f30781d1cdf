"""DQNLearner: the reference's learn() on the device.

Device twin of DQN.learn (scripts/main.py:122-157), HDQN.learn (scripts/hdqn.py:186-221) and
Goal_DQN.learn (hdqn.py:104-139) -- the same code on nets of 10 -> 5, 11 -> 5 and 10 -> 3: a minibatch
drawn from the replay memory, the Double-DQN target, nn.MSELoss, torch.optim.Adam(lr 0.01) and the
target net copied from the eval net every Q_NETWORK_ITERATION = 100 learns. One call enqueues any
number of updates on the current stream (seven kernel launches each, libmerging_hip.so's
mg_dqn_learn) and repacks the eval net for the acting kernels, so the loop of main.py:189-220 closes
without leaving the device:

    ring = ReplayRing(2000, device="cuda:0")
    learner = DQNLearner(QNet.from_state_dict(sd, device="cuda:0"), ring)
    traj = env.rollout_qnet(16, learner.qnet, seed)       # choose_action + env.step
    ring.store_rollout(obs0, traj)                         # store_transition
    learner.learn(4)                                       # learn(), four times
    traj = env.rollout_qnet(16, learner.qnet, seed, ...)   # acts with the new weights

The arithmetic is fp32 in the fixed order include/merging_hip.h documents, so a run is reproducible
bit for bit, also across a state_dict() / load_state_dict() resume.
"""

from __future__ import annotations

import ctypes

from . import _native
from ._base import DQNNets, LearnerBase
from ._device import ptr


class DQNLearner(DQNNets, LearnerBase):
    def __init__(self, net, ring, lr: float = 0.01, gamma: float = 0.9, batch_size: int = 128,
                 target_period: int = 100, betas=(0.9, 0.999), eps: float = 1e-8, seed: int = 0, device=None):
        """net: a QNet, or a state dict with the reference's keys (fc1.weight ... out.bias); both
        eval_net and target_net start from it. ring: the ReplayRing learn() draws from; a goal ring
        (24-float rows) implies in_dim 11. lr, gamma, batch_size, target_period: main.py:13-18's LR,
        GAMMA, BATCH_SIZE, Q_NETWORK_ITERATION; betas, eps: Adam's. seed: the key of the minibatch
        draws (update u of the run draws what ring.sample_rows(batch_size, seed, draw=u) returns)."""
        super().__init__(ring, "ring", device)
        torch = self._torch
        self.ring = ring
        tensors = self._net_tensors(net, "the", "learner")
        self._set_shape(tensors, ring.row, "ring's")
        self.target_period = int(target_period)
        sbytes = int(_native.lib.mg_dqn_learn_scratch_bytes(int(batch_size), self.in_dim, self.out_dim))
        self._setup(batch_size, seed, sbytes, lr, gamma, betas, eps, self.target_period)
        self._buf = torch.empty(4 * self._P, dtype=torch.float32, device=self.device)
        # the acting net: its fp32 tensors are views of the eval block, its packed buffer is
        # rewritten by every learn()
        self.qnet = self._init_learner(self._buf, net, tensors)

    def _repack(self):
        self._pack(self._buf, self.qnet)

    # ------------------------------------------------------------------ learn
    def learn(self, num_updates: int = 1, filled_only: bool = False, return_loss: bool = False, return_rows: bool = False):
        """num_updates times learn() (main.py:122-157), enqueued back to back on the current stream;
        nothing is synchronised. filled_only draws from the rows stored so far instead of the whole
        memory (the reference learns only once the memory is full, main.py:211). return_loss: the
        [num_updates] fp32 device tensor of the updates' MSE losses; return_rows: also the
        [num_updates, B, row] minibatches."""
        torch = self._torch
        U = int(num_updates)
        if U < 0:
            raise ValueError("num_updates must be >= 0")
        loss = torch.empty(U, dtype=torch.float32, device=self.device) if return_loss else None
        rows = torch.empty((U, self.batch_size, self.ring.row), dtype=torch.float32,
                           device=self.device) if return_rows else None
        if U > 0:
            rc = _native.lib.mg_dqn_learn(
                self._buf.data_ptr(), self.ring.memory.data_ptr(), self.ring._counter.data_ptr(), self.ring.capacity,
                self.ring.row, self.in_dim, self.out_dim, self.batch_size, U, self.learn_step_counter, self.seed,
                self.draw_counter, 1 if filled_only else 0, ctypes.byref(self.hyper),
                ptr(loss), ptr(rows), self.qnet.packed.data_ptr(), self._scratch.data_ptr(), self._scratch_bytes,
                self._stream())
            _native.check(rc, "mg_dqn_learn")
            self.learn_step_counter += U
            self.draw_counter += U
            self._new_weights(self.qnet)
        if return_loss and return_rows:
            return loss, rows
        return loss if return_loss else rows

    # ------------------------------------------------------------------ checkpoints
    def eval_state_dict(self):
        """eval_net.state_dict() as main.py:244 saves it (copies, torch-loadable)."""
        return self._net_state_dict(self._buf, 0)

    def target_state_dict(self):
        """target_net.state_dict() as main.py:245 saves it."""
        return self._net_state_dict(self._buf, 1)

    def state_dict(self):
        """Both nets, Adam's moments and the counters: a run resumed from it continues bit for bit."""
        return dict(super().state_dict(), in_dim=self.in_dim, out_dim=self.out_dim)

    def load_state_dict(self, sd):
        self._learner_state(sd)  # another shape's is refused
        super().load_state_dict(sd)
        self._repack()
