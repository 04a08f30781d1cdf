"""Golden vectors for Rainbow's acting path, from the reference's own RainbowDQN.

Test infrastructure only: run in the build container, never on the GPU box. Imports scripts/ranbowdqn.py
from the reference checkout (read-only; gen_golden.REFERENCE) with stand-ins in sys.modules for tensorboardX
and merging_gym (both absent here; only main() uses them) and tests/stubs/gym for gym. Nothing of the
reference's text is copied: only what its classes compute is recorded.

For torch.manual_seed(s), s = 1, 2, 3, then RainbowDQN(10, 5) (ranbowdqn.py:498-515):
  s{s}/sd/<key>       the state dict as constructed (parameters and the weight_epsilon / bias_epsilon buffers)
  s{s}/noise2/<key>   the noise buffers after one more reset_noise() (:537-541), the RNG continuing
  s{s}/{fam}/act0     act(state) (:543-548) on every katB_obs row of reference_golden.npz (as a Python list)
  s{s}/{fam}/act3     act(state[3:] + state[:3]), the literal expression of :669
  s{s}/soft/q0, q3    (forward(x) * linspace(Vmin, Vmax, 51)).sum(2), act()'s q, on every row (soft nets only:
                      no q bound applies to the saturated default nets)
  s1/{fam}/dist0      forward(x) itself, [256, 5, 51], on the 256-row subset `rows` (seed 1 only: the
                      file-size limit)
fam "default": the net as constructed; fam "soft": the same net with linear1.weight / 1024 (an exact scaling).
On raw observations (positions up to +-9,800) the default nets' softmax saturates to one-hot, which hides every
error of exp, the sums and the division; the soft nets' largest atom probability is about 0.03.
The act() results are taken with the state dict's noise (before the second reset_noise).

Two files, each under the repository's 1 MiB limit: rainbow_golden.npz (state dicts, actions) and
rainbow_golden_noise.npz (noise2, q and dist0).

Usage:  python tests/golden/gen_rainbow.py
"""

from __future__ import annotations

import contextlib
import io
import os
import sys
import types
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "rainbow_golden.npz")
OUT_NOISE = os.path.join(HERE, "rainbow_golden_noise.npz")
SEEDS = (1, 2, 3)
SUBSET = 256


def load_reference_module():
    sys.path.insert(0, HERE)
    from gen_golden import REFERENCE

    if not os.path.isdir(REFERENCE):
        raise SystemExit(f"{REFERENCE} not found: golden vectors are generated only in the build container")
    os.environ.setdefault("MPLBACKEND", "Agg")
    sys.dont_write_bytecode = True
    tb = types.ModuleType("tensorboardX")
    tb.SummaryWriter = object
    sys.modules.setdefault("tensorboardX", tb)
    sys.modules.setdefault("merging_gym", types.ModuleType("merging_gym"))
    sys.path[:0] = [os.path.join(os.path.dirname(HERE), "stubs"), os.path.join(REFERENCE, "scripts")]
    with contextlib.redirect_stdout(io.StringIO()):
        import ranbowdqn
    return ranbowdqn


def main():
    import torch

    mod = load_reference_module()
    mod.USE_CUDA = False
    obs = np.load(os.path.join(HERE, "reference_golden.npz"))["katB_obs"]
    states = [[float(v) for v in row] for row in obs]
    rows = np.linspace(0, len(states) - 1, SUBSET).astype(np.int64)
    support = torch.linspace(mod.Vmin, mod.Vmax, mod.num_atoms)
    out, noise = {"rows": rows}, {}
    warnings.simplefilter("ignore")
    for s in SEEDS:
        torch.manual_seed(s)
        model = mod.RainbowDQN(10, 5, mod.num_atoms, mod.Vmin, mod.Vmax)
        sd = {k: v.detach().clone() for k, v in model.state_dict().items()}
        for k, v in sd.items():
            out[f"s{s}/sd/{k}"] = v.numpy()
        for fam in ("default", "soft"):
            if fam == "soft":
                model.linear1.weight.data.div_(1024.0)
            out[f"s{s}/{fam}/act0"] = np.array([model.act(st) for st in states], np.int8)
            out[f"s{s}/{fam}/act3"] = np.array([model.act(st[3:] + st[:3]) for st in states], np.int8)
            for r, view in ((0, lambda st: st), (3, lambda st: st[3:] + st[:3])):
                x = torch.FloatTensor([view(st) for st in states])
                with torch.no_grad():
                    dist = model.forward(x).data.cpu()
                if fam == "soft":
                    noise[f"s{s}/{fam}/q{r}"] = (dist * support).sum(2).numpy()
                if s == 1 and r == 0:
                    noise[f"s{s}/{fam}/dist0"] = dist[torch.from_numpy(rows)].numpy()
            print(f"seed {s} {fam}: actions", np.bincount(out[f"s{s}/{fam}/act0"], minlength=5),
                  "largest p", float(dist.max()))
        model.linear1.weight.data.mul_(1024.0)
        assert torch.equal(model.linear1.weight.data, sd["linear1.weight"])
        model.reset_noise()
        for k, v in model.state_dict().items():
            if k.endswith("epsilon"):
                noise[f"s{s}/noise2/{k}"] = v.detach().clone().numpy()
    np.savez_compressed(OUT, **out)
    np.savez_compressed(OUT_NOISE, **noise)
    for p in (OUT, OUT_NOISE):
        print("wrote", p, os.path.getsize(p), "bytes")
        assert os.path.getsize(p) < (1 << 20)


if __name__ == "__main__":
    main()
