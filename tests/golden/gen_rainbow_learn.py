"""Golden vectors for Rainbow's learning step, from the reference's own compute_td_loss.

Test infrastructure only: run in the build container, never on the GPU box. Imports scripts/ranbowdqn.py
through gen_rainbow.load_reference_module() and calls its compute_td_loss (:584-609) with a stand-in buffer
whose sample() returns chosen rows. Nothing of the reference's text is copied: only what its functions compute
is recorded.

For the two net families of gen_rainbow.py ("default": the net as constructed, whose softmax saturates on raw
observations so the clamp and the exp cut-off are live; "soft": linear1.weight / 1024) and two consecutive
updates u = 0, 1 of torch.manual_seed(1)'s RainbowDQN pair after update_target:
  rainbow_learn_{fam}_u{u}_state.npz
      rows          the minibatch [32, 24] fp32 = [s, a, r, s', done, 0]
      cur/<key>     the current model's state dict before the update (parameters and noise buffers)
      tgt/<key>     the target model's noise buffers before the update (its parameters never change: they are
                    u0's cur/ parameters, update_target's copy)
      next_dist     the gathered, support-scaled target distribution [32, 51] (:560-563)
      proj_dist     projection_distribution's result [32, 51]
      loss32, loss64
  rainbow_learn_{fam}_u{u}_grads.npz
      g64/<key>     the gradients of the fp64 run of the same function (model.double(), float64 default dtype,
                    the module's `torch` name replaced by a proxy whose FloatTensor makes doubles). Its
                    projection_distribution is the reference's own on fp32 tensors, fed the fp64 target
                    model's output rounded to fp32: the projection is discontinuous where b is integral (the
                    mass is dropped, :579-580), which happens in fp32 arithmetic and not in fp64, so a
                    projection in fp64 would be the target of another loss
      d32/<key>     fp32(g32 - g64): the reference's own fp32 run minus the fp64 one
Each file stays under the repository's 1 MiB limit.

The minibatch is accepted only if every row's two best target q-values differ by more than 1e-3 (about 30
times the worst-case fp32 error of a 51-term sum of values <= 10, so no rounding flips the argmax) and no hidden
pre-activation of either forward is within 1e-6 of zero; otherwise the next row seed is tried.

Usage:  python tests/golden/gen_rainbow_learn.py
"""

from __future__ import annotations

import copy
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
B = 32
REWARDS = np.array([-10.0, 10.0, 0.0, 0.4, 1.2, 2.0, -0.001, 1.0, 25.0, -0.37, -30.0, 9.6], np.float32)


class Chosen:
    """Stand-in for ReplayBuffer: sample() returns the chosen rows."""

    def __init__(self, rows):
        self.rows = rows

    def sample(self, batch_size):
        r = self.rows
        assert batch_size == len(r)
        return r[:, :10].copy(), r[:, 10].astype(np.int64), r[:, 11].copy(), r[:, 12:22].copy(), r[:, 22].copy()


class Torch64:
    """The module's `torch` name for the fp64 run: FloatTensor makes doubles, everything else is torch's."""

    def __init__(self, torch):
        self._torch = torch

    def __getattr__(self, name):
        return getattr(self._torch, name)

    def FloatTensor(self, data):
        return self._torch.as_tensor(np.asarray(data), dtype=self._torch.float64)


def make_rows(obs, seed):
    rng = np.random.default_rng(seed)
    at = rng.integers(0, len(obs) - 1, B)
    rows = np.zeros((B, 24), dtype=np.float32)
    rows[:, :10] = obs[at]
    rows[:, 12:22] = obs[at + 1]
    rows[:, 10] = np.arange(B) % 5
    rows[:, 11] = REWARDS[rng.integers(0, len(REWARDS), B)]
    rows[:, 22] = rng.integers(0, 2, B)
    rows[:len(REWARDS), 11] = REWARDS  # every special reward at least once
    rows[:4, 22] = (0, 1, 0, 1)
    return rows


def margins(torch, model, target, rows, support):
    """(smallest gap between the two best target q-values, smallest |hidden pre-activation|) in fp64."""
    m, t = copy.deepcopy(model).double(), copy.deepcopy(target).double()
    with torch.no_grad():
        s, s2 = torch.as_tensor(rows[:, :10], dtype=torch.float64), torch.as_tensor(rows[:, 12:22], dtype=torch.float64)
        q = (t(s2) * support.double()).sum(2)
        top = q.topk(2, dim=1).values
        small = []
        for net, x in ((m, s), (t, s2)):
            p1 = net.linear1(x)
            p2 = net.linear2(torch.relu(p1))
            h = torch.relu(p2)
            small += [p1.abs().min(), p2.abs().min(), net.noisy_value1(h).abs().min(), net.noisy_advantage1(h).abs().min()]
    return float((top[:, 0] - top[:, 1]).min()), float(min(small))


def main():
    import torch

    sys.path.insert(0, HERE)
    from gen_rainbow import load_reference_module

    mod = load_reference_module()
    mod.USE_CUDA = False
    warnings.simplefilter("ignore")
    obs = np.asarray(np.load(os.path.join(HERE, "reference_golden.npz"))["katB_obs"], dtype=np.float32)
    support = torch.linspace(mod.Vmin, mod.Vmax, mod.num_atoms)
    real_torch, real_proj = mod.torch, mod.projection_distribution
    for fam in ("default", "soft"):
        torch.manual_seed(1)
        current = mod.RainbowDQN(10, 5, mod.num_atoms, mod.Vmin, mod.Vmax)
        target = mod.RainbowDQN(10, 5, mod.num_atoms, mod.Vmin, mod.Vmax)
        if fam == "soft":
            current.linear1.weight.data.div_(1024.0)
        mod.update_target(current, target)
        optimizer = torch.optim.Adam(current.parameters(), 0.001)
        for u in range(2):
            for seed in range(100 * u + 1, 100 * u + 100):
                rows = make_rows(obs, seed)
                gap, small = margins(torch, current, target, rows, support)
                if gap > 1e-3 and small > 1e-6:
                    break
            else:
                raise SystemExit("no acceptable minibatch")
            state = {"rows": rows}
            for k, v in current.state_dict().items():
                state[f"cur/{k}"] = v.detach().clone().numpy()
            for k, v in target.state_dict().items():
                if k.endswith("epsilon"):
                    state[f"tgt/{k}"] = v.detach().clone().numpy()
            before = copy.deepcopy(current), copy.deepcopy(target)
            # the reference's own run, its projection recorded on the way
            seen = {}

            def recording(next_state, rewards, dones, target_model):
                with torch.no_grad():
                    nd = target_model(next_state).data * support
                    seen["next_dist"] = nd[torch.arange(nd.size(0)), nd.sum(2).max(1)[1]].clone().numpy()
                seen["proj_dist"] = real_proj(next_state, rewards, dones, target_model)
                return seen["proj_dist"]

            mod.projection_distribution = recording
            try:
                loss32 = mod.compute_td_loss(B, Chosen(rows), target, current, optimizer)
            finally:
                mod.projection_distribution = real_proj
            # the fp64 run on copies of the same before-state (the global generator put back afterwards)
            rng_state = torch.get_rng_state()
            c64, t64 = before[0].double(), before[1].double()
            torch.set_default_dtype(torch.float64)
            mod.torch = Torch64(real_torch)
            proxy = mod.torch

            def projection64(next_state, rewards, dones, target_model):
                mod.torch = real_torch
                torch.set_default_dtype(torch.float32)
                try:
                    return real_proj(next_state.float(), rewards.float(), dones.float(),
                                     lambda x: target_model(x.double()).float()).double()
                finally:
                    mod.torch = proxy
                    torch.set_default_dtype(torch.float64)

            mod.projection_distribution = projection64
            try:
                loss64 = mod.compute_td_loss(B, Chosen(rows), t64, c64, torch.optim.Adam(c64.parameters(), 0.001))
            finally:
                mod.torch = real_torch
                mod.projection_distribution = real_proj
                torch.set_default_dtype(torch.float32)
                torch.set_rng_state(rng_state)
            state["next_dist"] = seen["next_dist"]
            state["proj_dist"] = seen["proj_dist"].clone().numpy()
            state["loss32"] = np.float32(loss32.item())
            state["loss64"] = np.float64(loss64.item())
            grads = {}
            worst = 0.0
            for (k, p32), (_, p64) in zip(current.named_parameters(), c64.named_parameters()):
                g64 = p64.grad.detach().numpy()
                grads[f"g64/{k}"] = g64
                grads[f"d32/{k}"] = (p32.grad.detach().double().numpy() - g64).astype(np.float32)
                worst = max(worst, float(np.abs(grads[f"d32/{k}"]).max() / np.abs(g64).max()))
            print(f"{fam} u{u}: row seed {seed}, q gap {gap:.3g}, smallest pre-activation {small:.3g}, loss32 "
                  f"{float(state['loss32']):.7g}, loss64 {float(state['loss64']):.12g}, integral b "
                  f"{np.mean(state['proj_dist'] != 0):.2f} non-zero proj, worst fp32 gradient error {worst:.3g}")
            for tag, d in (("state", state), ("grads", grads)):
                path = os.path.join(HERE, f"rainbow_learn_{fam}_u{u}_{tag}.npz")
                np.savez_compressed(path, **d)
                print("wrote", path, os.path.getsize(path), "bytes")
                assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
