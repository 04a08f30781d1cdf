"""Rainbow acting, the CPU side: the head's host twin against the plain-C restatement bit for bit, the
library's exp against glibc, RainbowNet's effective weights and noise against the reference's recorded buffers,
and the restatement of the whole forward (tests/rainbow_ref.py) against the reference's own act()
(tests/golden/rainbow_golden.npz, from tests/golden/gen_rainbow.py)."""

import ctypes
import ctypes.util
import math

import numpy as np
import pytest

import rainbow_ref as R

NETS = [(s, soft) for s in R.SEEDS for soft in (False, True)]
FAM = {False: "default", True: "soft"}

# Measured with this restatement on the fixture (seeds 1-3, both views), then doubled for the assertions:
MAX_TIE_GAP = 0.0024864078   # largest reference top-2 gap among differing choices of the soft nets (seed 1, view 3)
MAX_Q_ERROR = 0.00812912     # largest |q - q_ref| of the soft nets (seed 3, view 3)
MAX_DIFFERING = 0.02         # share of differing choices per net and view (measured 0 - 0.92 %)


# ---- the head
def _crafted_rows():
    """Logit rows [306] that meet the head's corners."""
    rng = np.random.default_rng(4)
    rows = []
    rows.append(np.full(R.LOGITS, 0.375, np.float32))                      # all logits equal: q = mean(z) five times
    tie = rng.normal(0, 1, R.LOGITS).astype(np.float32)
    tie[R.ATOMS:] = np.tile(tie[R.ATOMS:2 * R.ATOMS], R.ACTIONS)            # five equal advantages: an exact q tie
    rows.append(tie)
    tie2 = tie.copy()
    tie2[R.ATOMS + 50] += 3.0                                               # action 0 ahead ...
    tie2[R.ATOMS * 4 + 50] += 3.0                                           # ... and action 3 the same: first wins
    rows.append(tie2)
    for atom in (0, 50, 12, 13, 38, 39):                                    # the maximum at the ends and at chain edges
        r = rng.normal(0, 1, R.LOGITS).astype(np.float32)
        r[atom] += 9.0
        rows.append(r)
    far = rng.normal(0, 1, R.LOGITS).astype(np.float32)
    far[:R.ATOMS] += np.linspace(0, 200, R.ATOMS, dtype=np.float32)         # a spread past the exp cut-off (87)
    rows.append(far)
    edge = np.zeros(R.LOGITS, np.float32)
    edge[1], edge[2] = -87.0, np.nextafter(np.float32(-87.0), np.float32(-100))  # on and just below the cut-off
    rows.append(edge)
    hot = np.full(R.LOGITS, -1000.0, np.float32)                            # saturated one-hot rows
    hot[:R.ATOMS] = 0.0
    hot[R.ATOMS + 51 * np.arange(R.ACTIONS) + np.array([3, 50, 0, 25, 26])] = 4000.0
    rows.append(hot)
    return np.stack(rows)


def test_host_head_equals_the_c_restatement_on_crafted_rows():
    rows = _crafted_rows()
    q_ref, a_ref = R.head_ref(rows)
    q, a = R.head_host(rows)
    np.testing.assert_array_equal(R.bits(q), R.bits(q_ref))
    np.testing.assert_array_equal(a, a_ref)
    z = R.support()
    assert (q[0] == q[0][0]).all() and abs(q[0][0] - z.mean()) < 1e-6 and a[0] == 0   # equal logits
    assert (q[1] == q[1][0]).all() and a[1] == 0                                      # exact tie: first index
    assert q[2][0] == q[2][3] and q[2][0] > q[2][1] and a[2] == 0
    assert np.isfinite(q).all()
    # the one-hot row: q is the support point of each action's atom
    np.testing.assert_array_equal(q[-1], z[[3, 50, 0, 25, 26]])
    assert a[-1] == 1


@pytest.mark.parametrize("seed,soft", NETS)
def test_host_head_equals_the_c_restatement_on_the_fixture_logits(seed, soft):
    for rotate in (0, 3):
        lg, q_ref, a_ref = R.forward_fixture(seed, soft, rotate)
        q, a = R.head_host(lg)
        np.testing.assert_array_equal(R.bits(q), R.bits(q_ref))
        np.testing.assert_array_equal(a, a_ref)


def test_host_head_outputs_are_optional():
    from merging_gym import _native

    lg = np.ascontiguousarray(R.forward_fixture(1, True, 0)[0][:7])
    z = R.support()
    q = np.zeros((7, 5), np.float32)
    a = np.zeros(7, np.int8)
    assert _native.lib.mg_host_rainbow_head(lg.ctypes.data, z.ctypes.data, q.ctypes.data, None, 7) == 0
    assert _native.lib.mg_host_rainbow_head(lg.ctypes.data, z.ctypes.data, None, a.ctypes.data, 7) == 0
    q2, a2 = R.head_host(lg)
    np.testing.assert_array_equal(q, q2)
    np.testing.assert_array_equal(a, a2)


# ---- exp
def test_exp_against_glibc_expf():
    """Sample: the 2,000,001 points of np.linspace(-87, 0, 2000001) rounded to fp32, and the end points -87,
    -0.0 and 0 themselves. Measured: the library's exp differs from glibc's expf (correctly rounded in all but
    rare cases) by at most 1 ulp -- 123,128 of the points by one, none by more -- which is the assertion. Below
    the cut-off the result is +0."""
    from merging_gym import _native

    x = np.concatenate([np.linspace(-87, 0, 2_000_001).astype(np.float32), np.float32([-87.0, -0.0, 0.0])])
    y = np.empty_like(x)
    assert _native.lib.mg_host_rainbow_exp(x.ctypes.data, y.ctypes.data, x.size) == 0
    np.testing.assert_array_equal(R.bits(y), R.bits(R.exp_ref(x)))  # the C restatement's exp: the same bits
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.expf.restype, libm.expf.argtypes = ctypes.c_float, [ctypes.c_float]
    g = np.fromiter((libm.expf(float(v)) for v in x), np.float32, x.size)
    ulp = np.abs(y.view(np.int32).astype(np.int64) - g.view(np.int32).astype(np.int64))
    print("worst error against expf:", int(ulp.max()), "ulp; points off by one:", int((ulp == 1).sum()))
    assert int(ulp.max()) == 1
    assert y[-1] == 1.0 and y[-2] == 1.0 and y[-3] > 0
    below = np.float32([np.nextafter(np.float32(-87), np.float32(-100)), -88, -1000, -np.inf, np.nan])
    out = np.ones_like(below)
    assert _native.lib.mg_host_rainbow_exp(below.ctypes.data, out.ctypes.data, below.size) == 0
    np.testing.assert_array_equal(R.bits(out), np.zeros(below.size, np.uint32))  # +0, not -0


# ---- effective weights and noise
@pytest.mark.parametrize("seed", R.SEEDS)
def test_effective_weights_equal_the_fixture(seed):
    import torch

    from merging_gym.rainbow import RainbowNet

    sd = R.state_dict(seed)
    net = RainbowNet.from_state_dict(sd)
    eff, ref = net.effective(), R.effective_ref(sd)
    assert list(eff) == list(ref)
    for k in ref:
        np.testing.assert_array_equal(R.bits(eff[k].numpy()), R.bits(ref[k]), err_msg=k)
    mu = RainbowNet.from_state_dict(sd, training=False).effective()
    for name in R.NOISY:
        assert torch.equal(mu[f"{name}.weight"], sd[f"{name}.weight_mu"]) and torch.equal(mu[f"{name}.bias"],
                                                                                         sd[f"{name}.bias_mu"])
    with pytest.raises(ValueError):
        RainbowNet.from_state_dict({k: v for k, v in sd.items() if k != "noisy_value2.bias_epsilon"})
    with pytest.raises(ValueError):
        RainbowNet.from_state_dict(dict(sd, extra=torch.zeros(1)))
    with pytest.raises(ValueError):
        RainbowNet.from_state_dict(dict(sd, **{"linear1.weight": torch.zeros(200, 10)}))


@pytest.mark.parametrize("seed", R.SEEDS)
def test_reset_noise_reproduces_the_reference_buffers(seed):
    """torch.manual_seed(s), then the draws RainbowDQN(10, 5)'s construction makes (ranbowdqn.py:508-515:
    two nn.Linear, then per NoisyLinear the two uniform_ of reset_parameters and the three randn of
    reset_noise), replayed here in the tests' own words -- the replayed parameters and first noise equal the
    recorded state dict, so the generator stands where the reference's stood -- then RainbowNet.reset_noise():
    its buffers equal the reference's after one more reset_noise(), bit for bit."""
    import torch

    from merging_gym.rainbow import SHAPES, RainbowNet

    sd = R.state_dict(seed)
    torch.manual_seed(seed)
    for name in ("linear1", "linear2"):
        out_f, in_f = SHAPES[name]
        lin = torch.nn.Linear(in_f, out_f)
        assert torch.equal(lin.weight.data, sd[f"{name}.weight"]) and torch.equal(lin.bias.data, sd[f"{name}.bias"])

    def scale(size):
        x = torch.randn(size)
        return x.sign() * x.abs().sqrt()

    for name in R.NOISY:
        out_f, in_f = SHAPES[name]
        rng = 1 / math.sqrt(in_f)
        assert torch.equal(torch.empty(out_f, in_f).uniform_(-rng, rng), sd[f"{name}.weight_mu"]), name
        assert torch.equal(torch.empty(out_f).uniform_(-rng, rng), sd[f"{name}.bias_mu"]), name
        e_in, e_out = scale(in_f), scale(out_f)
        assert torch.equal(torch.outer(e_out, e_in), sd[f"{name}.weight_epsilon"]), name
        assert torch.equal(scale(out_f), sd[f"{name}.bias_epsilon"]), name
    net = RainbowNet.from_state_dict(sd)
    net.reset_noise()
    zn = R.golden("rainbow_golden_noise.npz")
    for name in R.NOISY:
        for leaf in ("weight_epsilon", "bias_epsilon"):
            np.testing.assert_array_equal(R.bits(net.state[f"{name}.{leaf}"].numpy()),
                                          R.bits(zn[f"s{seed}/noise2/{name}.{leaf}"]), err_msg=f"{name}.{leaf}")
    # a generator of its own gives the same stream
    gen = torch.Generator().manual_seed(99)
    a = RainbowNet.from_state_dict(sd)
    a.reset_noise(generator=gen)
    torch.manual_seed(99)
    b = RainbowNet.from_state_dict(sd)
    b.reset_noise()
    assert all(torch.equal(a.state[k], b.state[k]) for k in a.state)


# ---- the restatement against the reference's own act()
@pytest.mark.parametrize("rotate", [0, 3])
@pytest.mark.parametrize("seed,soft", NETS)
def test_restatement_against_the_reference_act(seed, soft, rotate):
    """At most 2 % of the choices differ per net and view (bf16 operands and the MFMA's accumulation against
    the reference's fp32). For the soft nets, whose softmax is not saturated, every differing choice is a
    near-tie of the reference's own q, and q itself is close: both bounds are twice the worst value measured
    with this restatement over seeds 1-3 and both views (MAX_TIE_GAP 0.0024864, MAX_Q_ERROR 0.0081291). No q
    bound applies to the saturated default nets: there q jumps between support points."""
    _, q, act = R.forward_fixture(seed, soft, rotate)
    ref = R.golden()[f"s{seed}/{FAM[soft]}/act{rotate}"]
    differ = np.nonzero(act != ref)[0]
    print(f"seed {seed} {FAM[soft]} view {rotate}: {len(differ)} of {len(ref)} choices differ")
    assert len(differ) <= MAX_DIFFERING * len(ref)
    if soft:
        q_ref = R.golden("rainbow_golden_noise.npz")[f"s{seed}/soft/q{rotate}"]
        np.testing.assert_array_equal(q_ref.argmax(1), ref)  # the recorded q is act()'s own
        gap = q_ref[differ, ref[differ]] - q_ref[differ, act[differ]]
        err = np.abs(q - q_ref).max()
        print(f"  largest top-2 gap among them {gap.max() if len(gap) else 0.0:.7f}, largest |q - q_ref| {err:.7f}")
        assert (gap <= 2 * MAX_TIE_GAP).all()
        assert err <= 2 * MAX_Q_ERROR


def test_soft_nets_are_not_saturated():
    """What makes the soft nets' q bound meaningful: the default net's distributions are one-hot, the soft
    net's largest atom probability stays within five times the uniform 1 / 51 (a property of the fixture, not of
    the code under test)."""
    zn = R.golden("rainbow_golden_noise.npz")
    assert zn["s1/default/dist0"].max() == 1.0
    assert zn["s1/soft/dist0"].max() < 5 / 51
    np.testing.assert_allclose(zn["s1/soft/dist0"].sum(2), 1.0, atol=1e-5)


@pytest.mark.parametrize("seed,soft", NETS)
def test_the_opponent_view_is_a_rotation_by_three(seed, soft):
    """ranbowdqn.py:669 feeds state[3:] + state[:3], not the DQN's swap of halves: the restatement at rotate = 3
    meets the 2 % cap against the recorded act(state[3:] + state[:3]); at rotate = 5 it does not (measured:
    15 - 99 % of the choices differ)."""
    ref = R.golden()[f"s{seed}/{FAM[soft]}/act3"]
    three = (R.forward_fixture(seed, soft, 3)[2] != ref).mean()
    five = (R.forward_fixture(seed, soft, 5)[2] != ref).mean()
    print(f"seed {seed} {FAM[soft]}: rotate 3 differs on {three:.4f}, rotate 5 on {five:.4f}")
    assert three <= MAX_DIFFERING < five
