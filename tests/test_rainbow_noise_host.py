"""The Rainbow learner's device noise stream on the CPU: the host twins mg_host_rainbow_noise and
mg_host_rainbow_ndtri against the plain-C restatement bit for bit, the inverse CDF against the standard
library's, the stream's symmetry, addressing and distribution, RainbowNet.reset_noise(seed=, draw=), the host
learner fed from both, and the four entry points' refusals. No GPU is touched."""
import math
import statistics

import numpy as np
import pytest

import rainbow_learn_ref as L
import rainbow_noise_ref as R

NF = R.NF


@pytest.mark.parametrize("noise_seed,first_update,U", R.CASES, ids=["zero", "low-word-crossing", "64-bit-seed"])
def test_host_factors_equal_the_restatement(noise_seed, first_update, U):
    got, want = R.noise_host(noise_seed, first_update, U), R.noise_ref(noise_seed, first_update, U)
    assert R.same_bits(got, want)
    assert np.isfinite(got).all() and (got != 0).all()


def _ndtri_inputs():
    return np.concatenate([R.edge_uniforms(), R.stream_uniforms()])


def test_host_inverse_cdf_equals_the_restatement():
    u = _ndtri_inputs()
    got = R.ndtri_host(u)
    assert R.same_bits(got, R.ndtri_ref(u))
    assert np.isfinite(got).all()
    # all three branches are in the list
    r = np.sqrt(-np.log(np.minimum(u, 1 - u)))
    central = np.abs(u - 0.5) <= 0.425
    assert central.any() and (~central & (r <= 5)).any() and (~central & (r > 5)).any()


def test_inverse_cdf_outside_the_open_interval_is_nan():
    z = R.ndtri_host(np.array([0.0, 1.0, -0.25, 1.5, np.nan, np.inf, 5e-324]))
    assert np.isnan(z).all()
    assert R.same_bits(z, R.ndtri_ref(np.array([0.0, 1.0, -0.25, 1.5, np.nan, np.inf, 5e-324])))


def test_inverse_cdf_agrees_with_the_standard_library():
    """statistics.NormalDist().inv_cdf is the same AS 241 with the C library's log: a shared typo in a
    coefficient would show, a bit-level pin it is not. Largest difference seen on the edge list and the 4,096
    stream uniforms (an x86-64 CPU, glibc's log): 3.0 ulp, at u = 0.0415... in the r <= 5 tail, where the two logs' last
    bit goes through the square root and a degree-7 rational. The bound is 4x that."""
    u = _ndtri_inputs()
    got = R.ndtri_host(u)
    inv = statistics.NormalDist().inv_cdf
    want = np.array([inv(float(x)) for x in u])
    ulps = np.abs(got - want) / np.spacing(np.abs(want))
    print(f"largest difference to statistics.NormalDist().inv_cdf: {ulps.max()} ulp at u = {u[ulps.argmax()]!r}")
    assert ulps.max() <= 12.0


def test_inverse_cdf_is_odd_about_one_half():
    """Wherever 1 - u is exact, as for every uniform of the stream (a multiple of 2^-53)."""
    grid = lambda x: round(x * 2.0 ** 53) * 2.0 ** -53  # noqa: E731  -- the nearest multiple of 2^-53
    u = np.concatenate([R.stream_uniforms(), [2.0 ** -53, 3 * 2.0 ** -53, 0.25, grid(0.075), grid(0.075) - 2.0 ** -53,
                                              grid(math.exp(-25.0)), grid(math.exp(-25.0)) + 2.0 ** -53]])
    assert (u * 2.0 ** 53 == np.rint(u * 2.0 ** 53)).all() and ((u > 0) & (u < 0.5) | (u > 0.5) & (u < 1)).all()
    z = R.ndtri_host(u)
    assert R.same_bits(R.ndtri_host(1.0 - u), -z)
    assert ((z < 0) == (u < 0.5)).all()


def test_any_update_is_addressable_on_its_own():
    whole = R.noise_host(11, 5, 3)
    for i, t in enumerate((5, 6, 7)):
        assert R.same_bits(whole[i:i + 1], R.noise_host(11, t, 1))


def test_blocks_and_seeds_are_independent_streams():
    a, b = R.noise_host(11, 0, 1), R.noise_host(12, 0, 1)
    assert (a[0, 0] != a[0, 1]).mean() > 0.99  # current against target
    assert (a != b).mean() > 0.99
    assert (R.noise_host(11, 1, 1) != a).mean() > 0.99


def test_device_noise_factors_has_noise_factors_shape():
    import torch

    from merging_gym import rainbow_learn

    want = rainbow_learn.noise_factors(2, torch.Generator().manual_seed(0))
    got = rainbow_learn.device_noise_factors(2, 11, 4)
    assert got.shape == want.shape == (2, 2, NF) and got.dtype == want.dtype == torch.float32
    assert got.device.type == "cpu" and got.is_contiguous()
    assert R.same_bits(got.numpy(), R.noise_host(11, 4, 2))
    assert R.same_bits(rainbow_learn.device_noise_factors(1, -1, 0).numpy(), R.noise_host(2 ** 64 - 1, 0, 1))
    assert tuple(rainbow_learn.device_noise_factors(0, 11).shape) == (0, 2, NF)


def _normal_cdf(v):
    import torch

    return (0.5 * (1.0 + torch.erf(torch.from_numpy(v) / math.sqrt(2.0)))).numpy()


@pytest.mark.parametrize("noise_seed,first_update", [c[:2] for c in R.CASES],
                         ids=["zero", "low-word-crossing", "64-bit-seed"])
def test_distribution_of_200_updates(noise_seed, first_update):
    """The 449,600 pre-transform values x |x| of 200 updates are standard normal draws: mean, variance,
    Kolmogorov-Smirnov distance, lag-1 correlation across updates, current against target, no repeated uniform."""
    U = 200
    f = R.noise_host(noise_seed, first_update, U)
    assert R.same_bits(f, R.noise_ref(noise_seed, first_update, U))
    f = f.astype(np.float64)
    x = f * np.abs(f)  # [U, 2, 1124]
    v = x.reshape(-1)
    N = v.size
    assert N == 449600
    mean, var = v.mean(), v.var()
    cdf = _normal_cdf(np.sort(v))
    i = np.arange(1, N + 1)
    ks = max((i / N - cdf).max(), (cdf - (i - 1) / N).max())
    a, b = x[:-1].reshape(-1), x[1:].reshape(-1)
    lag1 = np.corrcoef(a, b)[0, 1] * math.sqrt(a.size)
    cross = np.corrcoef(x[:, 0].reshape(-1), x[:, 1].reshape(-1))[0, 1] * math.sqrt(N / 2)
    u = R.uniforms_ref(noise_seed, first_update, U).reshape(-1)
    print(f"mean {mean * math.sqrt(N):.3f} se, variance {(var - 1) / math.sqrt(2 / N):.3f} sd, KS sqrt(N) "
          f"{ks * math.sqrt(N):.3f}, lag-1 {lag1:.3f} sigma, current/target {cross:.3f} sigma")
    assert abs(mean) * math.sqrt(N) < 4
    assert abs(var - 1) < 4 * math.sqrt(2 / N)
    assert ks * math.sqrt(N) < 1.95
    assert abs(lag1) < 4
    assert abs(cross) < 4
    assert np.unique(u).size == N
    assert ((u > 0) & (u < 1) & (u != 0.5)).all()


def test_reset_noise_from_the_stream():
    import torch

    from merging_gym import RainbowNet, rainbow_learn
    from merging_gym.rainbow import NOISY, SHAPES

    net = RainbowNet.from_state_dict(L.golden_state())
    before = {k: v.clone() for k, v in net.state.items()}
    net.reset_noise(seed=3, draw=2)
    factors, at = rainbow_learn.device_noise_factors(3, 3)[2, 0], 0
    for name in NOISY:
        out_f, in_f = SHAPES[name]
        eps_in, eps_out, eps_b = factors[at:at + in_f], factors[at + in_f:at + in_f + out_f], \
            factors[at + in_f + out_f:at + in_f + 2 * out_f]
        at += in_f + 2 * out_f
        assert torch.equal(net.state[f"{name}.weight_epsilon"].view(torch.int32), eps_out.ger(eps_in).view(torch.int32))
        assert torch.equal(net.state[f"{name}.bias_epsilon"].view(torch.int32), eps_b.view(torch.int32))
        assert not torch.equal(net.state[f"{name}.weight_epsilon"], before[f"{name}.weight_epsilon"])
    assert at == NF
    again = RainbowNet.from_state_dict(L.golden_state())
    again.reset_noise(seed=3, draw=2)
    other = RainbowNet.from_state_dict(L.golden_state())
    other.reset_noise(seed=3, draw=1)
    for k, v in net.state.items():
        assert torch.equal(v, again.state[k])
        assert torch.equal(v, before[k]) == ("epsilon" not in k)
    assert not torch.equal(other.state["noisy_value1.bias_epsilon"], net.state["noisy_value1.bias_epsilon"])
    with pytest.raises(ValueError):
        net.reset_noise(torch.Generator().manual_seed(0), seed=3)


@pytest.mark.parametrize("batch", [1, 33])
def test_host_learner_on_host_factors_equals_the_restatement_on_restated_factors(batch):
    ring, c = L.ring_case(64, 40)
    L0 = L.learner_numpy(L.golden_state(1, "default"))
    got = L.run_host(L0, ring, c, batch, 2, 0, 3, 0, R.noise_host(7, 0, 2))
    want = L.run_ref(L0, ring, c, batch, 2, 0, 3, 0, R.noise_ref(7, 0, 2))
    L.assert_same((got[0], got[1:]), (want[0], want[1:]))


def _refused(rc, *needles):
    from merging_gym import _native

    msg = _native.lib.mg_last_error().decode()
    assert rc != 0 and all(n in msg for n in needles), (rc, msg)


def test_refusals_name_the_entry_point():
    from merging_gym import _native

    lib = _native.lib
    buf = np.zeros(2 * NF + 2, np.float32)
    d = np.zeros(8, np.float64)
    p, q = buf.ctypes.data, d.ctypes.data
    assert p % 4 == 0 and q % 8 == 0
    for name, call in (("mg_rainbow_noise", lambda *a: lib.mg_rainbow_noise(*a, None)),
                       ("mg_host_rainbow_noise", lib.mg_host_rainbow_noise)):
        _refused(call(1, 0, 1, None), name + ":", "NULL pointer")
        _refused(call(1, 0, -1, p), name + ":", "num_updates < 0")
        _refused(call(1, 0, 1, p + 2), name + ":", "noise_out must be 4-byte aligned")
        assert call(1, 0, 0, p) == 0
    for name, call in (("mg_rainbow_ndtri", lambda *a: lib.mg_rainbow_ndtri(*a, None)),
                       ("mg_host_rainbow_ndtri", lib.mg_host_rainbow_ndtri)):
        _refused(call(None, q, 4), name + ":", "NULL pointer")
        _refused(call(q, None, 4), name + ":", "NULL pointer")
        _refused(call(q, q + 32, -1), name + ":", "n < 0")
        _refused(call(q + 4, q + 32, 2), name + ":", "u and z must be 8-byte aligned")
        _refused(call(q, q + 36, 2), name + ":", "u and z must be 8-byte aligned")
        assert call(q, q + 32, 0) == 0
    assert not buf.any() and not d.any()  # a refused or empty call writes nothing
    assert lib.mg_abi_version() == 21
