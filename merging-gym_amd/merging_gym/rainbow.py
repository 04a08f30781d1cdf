"""The reference's Rainbow policy on the device: RainbowDQN (scripts/ranbowdqn.py:498-548) -- a noisy
dueling C51 net -- as its act() evaluates it, packed for the fused bf16 MFMA kernels.

    net = RainbowNet.from_state_dict(torch.load(path, weights_only=True), device="cuda:0")
    q, action = net.forward(obs)                      # [N, 5] fp32, [N] int8
    traj = env.rollout_rainbow(T, net, opponent="self")   # act + act on the rotated view + env step, fused
    net.reset_noise()                                 # after a learn, as compute_td_loss does (:606)

The noisy layers act through their effective weights mu + sigma * epsilon (:468-470); the reference never
calls .eval() and redraws epsilon only inside compute_td_loss, so between two learns the policy is a fixed
function of those weights. Learning (compute_td_loss) is merging_gym.rainbow_learn's RainbowLearner.
"""

from __future__ import annotations

PLAIN = ("linear1", "linear2")
NOISY = ("noisy_value1", "noisy_value2", "noisy_advantage1", "noisy_advantage2")  # reset_noise's order, :537-541
SHAPES = {"linear1": (32, 10), "linear2": (64, 32), "noisy_value1": (64, 64), "noisy_value2": (51, 64),
          "noisy_advantage1": (64, 64), "noisy_advantage2": (5 * 51, 64)}
NUM_ACTIONS, NUM_ATOMS = 5, 51


def _scale_noise(size, generator):
    """NoisyLinear._scale_noise (:493-496)."""
    import torch

    x = torch.randn(size, generator=generator)
    return x.sign().mul(x.abs().sqrt())


class RainbowNet:
    """RainbowDQN(10, 5) with 51 atoms. The parameters and noise buffers live on the host (fp32 torch
    tensors, `state`); `packed` is the kernels' layout on the device, built on first use and again after
    reset_noise()."""

    def __init__(self, state, training=True, device=None):
        import torch

        self.state = {}
        for name in PLAIN:
            for leaf in ("weight", "bias"):
                self.state[f"{name}.{leaf}"] = self._take(state, f"{name}.{leaf}", name, leaf)
        for name in NOISY:
            for leaf in ("weight_mu", "weight_sigma", "weight_epsilon", "bias_mu", "bias_sigma", "bias_epsilon"):
                self.state[f"{name}.{leaf}"] = self._take(state, f"{name}.{leaf}", name, leaf)
        extra = set(state) - set(self.state)
        if extra:
            raise ValueError(f"unexpected keys for RainbowDQN.state_dict(): {sorted(extra)}")
        self.training = bool(training)
        self.device = device
        self.support = torch.linspace(-10, 10, NUM_ATOMS)  # Vmin, Vmax, num_atoms: :32-34, :546
        self._packed = None

    @staticmethod
    def _take(state, key, name, leaf):
        import torch

        if key not in state:
            raise ValueError(f"missing key {key} (expected RainbowDQN.state_dict())")
        t = torch.as_tensor(state[key]).detach().to("cpu", torch.float32).contiguous().clone()
        want = SHAPES[name] if leaf.startswith("weight") else SHAPES[name][:1]
        if tuple(t.shape) != want:
            raise ValueError(f"{key}: expected shape {want} of RainbowDQN(10, 5) with 51 atoms, got {tuple(t.shape)}")
        return t

    @classmethod
    def from_state_dict(cls, sd, training=True, device=None):
        return cls(sd, training=training, device=device)

    def effective(self):
        """The twelve fp32 tensors a forward uses, in layer order: NoisyLinear.forward's weight_mu +
        weight_sigma.mul(weight_epsilon) and its bias twin in training mode (:468-470), mu otherwise."""
        s, out = self.state, {}
        for name in PLAIN:
            out[f"{name}.weight"], out[f"{name}.bias"] = s[f"{name}.weight"], s[f"{name}.bias"]
        for name in NOISY:
            for leaf in ("weight", "bias"):
                mu = s[f"{name}.{leaf}_mu"]
                out[f"{name}.{leaf}"] = (mu + s[f"{name}.{leaf}_sigma"].mul(s[f"{name}.{leaf}_epsilon"])
                                         if self.training else mu)
        return out

    def reset_noise(self, generator=None, *, seed=None, draw=0):
        """RainbowDQN.reset_noise (:537-541): per noisy layer epsilon_in, epsilon_out, then the bias noise, each
        one torch.randn (:486-496). generator=None draws from torch's global generator, so after the same
        torch.manual_seed and the same earlier draws the buffers equal the reference's.

        seed: take the factors from the counter-based stream of a DeviceNoise learner instead
        (rainbow_learn.device_noise_factors): the current model's block of update `draw`, so the buffers equal
        those of a learner with generator=DeviceNoise(seed) after its update number `draw` (counted from 0)."""
        if seed is not None and generator is not None:
            raise ValueError("reset_noise takes a generator or a seed, not both")
        if seed is not None:
            from .rainbow_learn import device_noise_factors

            factors, at = device_noise_factors(1, seed, draw)[0, 0], 0

            def take(size, _generator):
                nonlocal at
                at += size
                return factors[at - size:at]
        else:
            take = _scale_noise
        for name in NOISY:
            out_f, in_f = SHAPES[name]
            eps_in = take(in_f, generator)
            eps_out = take(out_f, generator)
            self.state[f"{name}.weight_epsilon"].copy_(eps_out.ger(eps_in))
            self.state[f"{name}.bias_epsilon"].copy_(take(out_f, generator))
        self._packed = None

    # ---- device side
    def _device(self):
        import torch

        return torch.device(self.device if self.device is not None else "cuda")

    @property
    def packed(self):
        """The packed net on the device (mg_rainbow_pack), from the current effective weights."""
        if self._packed is None:
            import torch

            from . import _native

            dev = self._device()
            eff = self.effective()
            ts = [eff[f"{name}.{leaf}"].to(dev).contiguous()
                  for name in ("linear1", "linear2", "noisy_value1", "noisy_value2", "noisy_advantage1",
                               "noisy_advantage2") for leaf in ("weight", "bias")]
            z = self.support.to(dev).contiguous()
            packed = torch.empty(_native.lib.mg_rainbow_packed_bytes(), dtype=torch.uint8, device=dev)
            stream = torch.cuda.current_stream(dev).cuda_stream
            _native.check(_native.lib.mg_rainbow_pack(*(t.data_ptr() for t in ts), z.data_ptr(), 10, 32, 64, 64,
                                                      NUM_ACTIONS, NUM_ATOMS, packed.data_ptr(), stream),
                          "mg_rainbow_pack")
            self._packed = packed
        return self._packed

    def forward(self, obs, rotate: int = 0, logits: bool = False):
        """(q [N, 5] fp32, action [N] int8) of observations [N, 10] on the device: sum_i softmax_i z_i per
        action and its first maximum, as act() computes them (:543-548). rotate feeds obs[(j + rotate) % 10]
        (3: the opponent's view, :669). logits=True also returns the head's inputs [N, 306] (value [51], then
        advantage [5][51])."""
        import torch

        from . import _native

        dev = self._device()
        obs = obs.to(dev, torch.float32).contiguous()
        if obs.dim() != 2 or obs.shape[1] != 10:
            raise ValueError(f"expected observations [N, 10], got {tuple(obs.shape)}")
        n = obs.shape[0]
        q = torch.empty((n, NUM_ACTIONS), dtype=torch.float32, device=dev)
        act = torch.empty(n, dtype=torch.int8, device=dev)
        lg = torch.empty((n, NUM_ATOMS * (1 + NUM_ACTIONS)), dtype=torch.float32, device=dev) if logits else None
        stream = torch.cuda.current_stream(dev).cuda_stream
        _native.check(_native.lib.mg_rainbow_forward(self.packed.data_ptr(), obs.data_ptr(), int(rotate),
                                                     None if lg is None else lg.data_ptr(), q.data_ptr(),
                                                     act.data_ptr(), n, stream), "mg_rainbow_forward")
        return (q, act, lg) if logits else (q, act)

    def act(self, obs, rotate: int = 0):
        """RainbowDQN.act (:543-548) for a batch: the chosen actions [N] int8."""
        return self.forward(obs, rotate)[1]
