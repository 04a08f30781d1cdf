"""The Rainbow learner's noise drawn on the GPU: mg_rainbow_noise and mg_rainbow_ndtri against their host twins
bit for bit, a DeviceNoise learner against the plain-C restatements of the learner and of the stream, one
call against several, a resume, the stand-alone acting net's noise, and the prioritized learner."""
import numpy as np
import pytest

import rainbow_learn_ref as R
import rainbow_noise_ref as N
from learn_ref import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NOISE_SEED = 7


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _stream(torch):
    return torch.cuda.current_stream(torch.device(DEV)).cuda_stream


@pytest.mark.parametrize("noise_seed,first_update,U", N.CASES, ids=["zero", "low-word-crossing", "64-bit-seed"])
def test_draw_kernel_equals_the_host_twin(torch, noise_seed, first_update, U):
    from merging_gym import _native

    out = torch.full((U * 2 * N.NF + 64,), 9.0, dtype=torch.float32, device=DEV)
    _native.check(_native.lib.mg_rainbow_noise(noise_seed, first_update, U, out.data_ptr(), _stream(torch)),
                  "mg_rainbow_noise")
    got = out.cpu().numpy()
    assert (got[U * 2 * N.NF:] == 9.0).all()  # nothing past the last factor
    assert N.same_bits(got[:U * 2 * N.NF].reshape(U, 2, N.NF), N.noise_host(noise_seed, first_update, U))


def test_inverse_cdf_kernel_equals_the_host_twin(torch):
    """The edge list (all three branches, the far tail among them), 4,096 stream uniforms, and what gives NaN."""
    from merging_gym import _native

    u = np.concatenate([N.edge_uniforms(), N.stream_uniforms(), [0.0, 1.0, -0.25, 1.5, np.nan, 5e-324, 0.5]])
    du = torch.from_numpy(u).to(DEV)
    dz = torch.full((u.size + 8,), 9.0, dtype=torch.float64, device=DEV)
    _native.check(_native.lib.mg_rainbow_ndtri(du.data_ptr(), dz.data_ptr(), u.size, _stream(torch)), "mg_rainbow_ndtri")
    got = dz.cpu().numpy()
    assert (got[u.size:] == 9.0).all()
    assert N.same_bits(got[:u.size], N.ndtri_host(u))
    assert np.isnan(got[u.size - 7:u.size - 1]).all() and got[u.size - 1] == 0.0


def _replay(torch, ring, counter):
    from merging_gym import RainbowReplay

    rp = RainbowReplay(len(ring), device=DEV)
    rp.memory.copy_(torch.from_numpy(ring))
    rp._counter.fill_(counter)
    return rp


def _learner(torch, ring, counter, batch, noise_seed=NOISE_SEED, fam="default"):
    from merging_gym import DeviceNoise, RainbowLearner

    return RainbowLearner(R.golden_state(1, fam), _replay(torch, ring, counter), batch_size=batch, seed=3,
                          generator=DeviceNoise(noise_seed), device=DEV)


def _all(learner, U):
    return [t.cpu().numpy() for t in learner.learn(U, return_loss=True, return_rows=True, return_proj=True,
                                                   return_grads=True)]


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


@pytest.mark.parametrize("capacity,counter", ((64, 40), (64, 200)), ids=["partly-filled", "wrapped"])
@pytest.mark.parametrize("batch", (1, 33))
def test_device_mode_learner_equals_the_restatements(torch, batch, capacity, counter):
    """learn(2), sync_target(), learn(1): the learner's restatement fed the stream's restatement."""
    ring, c = R.ring_case(capacity, counter)
    nf = N.noise_ref(NOISE_SEED, 0, 3)
    L, *out1 = R.run_ref(R.learner_numpy(R.golden_state(1, "default")), ring, c, batch, 2, 0, 3, 0, nf[:2])
    R.sync_target(L)
    L, *out2 = R.run_ref(L, ring, c, batch, 1, 2, 3, 2, nf[2:])
    lr = _learner(torch, ring, c, batch)
    out = _all(lr, 2)
    lr.sync_target()
    out += _all(lr, 1)
    R.assert_same((lr._buf.cpu().numpy(), out), (L, out1 + out2))
    assert (lr.learn_step_counter, lr.draw_counter) == (3, 3)


def test_one_call_of_three_equals_three_calls_of_one(torch):
    ring, c = R.ring_case(64, 200)
    one, many, other = _learner(torch, ring, c, 33), _learner(torch, ring, c, 33), _learner(torch, ring, c, 33,
                                                                                           NOISE_SEED + 1)
    a = one.learn(3, return_loss=True)
    b = torch.cat([many.learn(1, return_loss=True) for _ in range(3)])
    d = other.learn(3, return_loss=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(one._buf.view(torch.int32), many._buf.view(torch.int32))
    assert torch.equal(one.net.packed, many.net.packed)
    assert not torch.equal(one._buf.view(torch.int32), other._buf.view(torch.int32))
    assert not torch.equal(one.net.packed, other.net.packed)
    assert not torch.equal(a.view(torch.int32), d.view(torch.int32))  # from update 1 on the nets differ


def test_device_mode_never_draws_on_the_host(torch, monkeypatch):
    from merging_gym import rainbow_learn

    def refuse(*a, **k):
        raise AssertionError("noise_factors called in device mode")

    monkeypatch.setattr(rainbow_learn, "noise_factors", refuse)
    monkeypatch.setattr(rainbow_learn, "device_noise_factors", refuse)
    ring, c = R.ring_case(64, 40)
    lr = _learner(torch, ring, c, 8)
    assert torch.isfinite(lr.learn(2, return_loss=True)).all()
    assert lr.noise == "device" and lr.noise_seed == NOISE_SEED and lr.generator is None
    # the stream's key defaults to the minibatch seed; the default mode is torch's generator
    from merging_gym import DeviceNoise, RainbowLearner

    by_default = RainbowLearner(R.golden_state(1, "default"), _replay(torch, ring, c), seed=5, generator=DeviceNoise(),
                                device=DEV)
    assert (by_default.noise, by_default.noise_seed) == ("device", 5)
    plain = RainbowLearner(R.golden_state(1, "default"), _replay(torch, ring, c), seed=5, device=DEV)
    assert (plain.noise, plain.noise_seed, plain.generator) == ("torch", None, None)


def test_resume_is_bit_identical_and_refuses_the_other_mode(torch):
    from merging_gym import RainbowLearner

    ring, c = R.ring_case(64, 200)
    straight = _learner(torch, ring, c, 32)
    a = straight.learn(4, return_loss=True)
    first = _learner(torch, ring, c, 32)
    b0 = first.learn(2, return_loss=True)
    ck = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in first.state_dict().items()}
    assert ck["noise"] == "device" and ck["noise_seed"] == NOISE_SEED and "generator" not in ck
    resumed = _learner(torch, ring, c, 32, noise_seed=99, fam="soft")
    resumed.load_state_dict(ck)
    assert resumed.noise_seed == NOISE_SEED
    b1 = resumed.learn(2, return_loss=True)
    assert torch.equal(a.view(torch.int32), torch.cat([b0, b1]).view(torch.int32))
    assert torch.equal(straight._buf.view(torch.int32), resumed._buf.view(torch.int32))
    assert torch.equal(straight.net.packed, resumed.net.packed)
    assert (resumed.learn_step_counter, resumed.draw_counter) == (4, 4)
    torch_mode = RainbowLearner(R.golden_state(1, "default"), _replay(torch, ring, c), batch_size=32, device=DEV)
    assert set(torch_mode.state_dict()) == {"learner", "learn_step_counter", "draw_counter", "seed", "generator"}
    with pytest.raises(ValueError, match='with "device" noise, this learner draws "torch" noise'):
        torch_mode.load_state_dict(ck)
    with pytest.raises(ValueError, match='with "torch" noise, this learner draws "device" noise'):
        resumed.load_state_dict(torch_mode.state_dict())


def test_stand_alone_net_reproduces_the_learners_noise(torch):
    from merging_gym import RainbowNet

    ring, c = R.ring_case(64, 40)
    lr = _learner(torch, ring, c, 32, noise_seed=21)
    lr.learn(1)
    sd = lr.current_state_dict()
    net = RainbowNet.from_state_dict(R.golden_state(1, "default"))
    net.reset_noise(seed=21, draw=0)
    keys = [k for k in sd if k.endswith("epsilon")]
    assert len(keys) == 8
    for k in keys:
        assert torch.equal(sd[k].cpu().view(torch.int32), net.state[k].view(torch.int32)), k
    lr.learn(2)
    net.reset_noise(seed=21, draw=2)
    sd = lr.current_state_dict()
    assert all(torch.equal(sd[k].cpu().view(torch.int32), net.state[k].view(torch.int32)) for k in keys)
    with pytest.raises(RuntimeError):
        lr.net.reset_noise(seed=21)


def test_prioritized_learner_in_device_mode(torch, monkeypatch):
    """Against a torch-mode PrioritizedRainbowLearner whose host draws are replaced by the stream's host twin."""
    import per_ref as P
    from merging_gym import DeviceNoise, PrioritizedRainbowLearner, PrioritizedRainbowReplay, rainbow_learn

    def replay():
        rp = PrioritizedRainbowReplay(13, 0.6, device=DEV)
        tr = P.transitions(9, 2)
        dev = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
        rp.store(dev(tr["obs_first"]), dev(tr["obs"]), dev(tr["a1"]), dev(tr["rew"]), dev(tr["done"]), dev(tr["final_obs"]))
        idx, _ = rp.sample_indices(8, 0.4, 1, 0)
        rp.update_priorities(idx, torch.linspace(0.1, 3.0, 8))
        return rp

    def run(lr):
        out = lr.learn(2, return_loss=True, return_idx=True, return_weights=True)
        return [lr._buf.cpu().numpy(), lr.replay._tree.cpu().numpy()] + [t.cpu().numpy() for t in out]

    sd = R.golden_state(1, "soft")
    got = run(PrioritizedRainbowLearner(sd, replay(), batch_size=8, seed=3, generator=DeviceNoise(5), device=DEV))
    calls = []

    def stream_factors(num_updates, generator=None):
        calls.append(num_updates)
        return rainbow_learn.device_noise_factors(num_updates, 5, 0)

    monkeypatch.setattr(rainbow_learn, "noise_factors", stream_factors)
    want = run(PrioritizedRainbowLearner(sd, replay(), batch_size=8, seed=3, device=DEV))
    assert calls == [2]
    for name, g, w in zip(("learner", "tree", "loss", "idx", "weights"), got, want):
        g, w = (g[1:], w[1:]) if name == "tree" else (g, w)  # sum's node 0 is unused
        assert _same(g, w), name
    assert bits(got[2]).size == 2 and np.isfinite(got[2]).all()
