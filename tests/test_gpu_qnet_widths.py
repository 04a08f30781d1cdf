"""mg_qnet_pack and mg_qnet_forward at every accepted width (tests/width_cases.py WIDTHS: the corners of
1 <= in_dim <= 13, 1 <= out_dim <= 8 and five points between): every bit of every Q-value against the oracle's
model of the matrix cores (oracle.merge_oracle.qnet_reference_mfma, pinned to recorded MI355X outputs by
tests/test_oracle_mfma.py), the padding columns and the rows past n, and the swapped view's refusal."""

import numpy as np
import pytest

import merge_oracle as mo
import width_cases as wc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NS = (1, 63, 64, 65, 577)  # one row; both sides of a wave's 64-row tile; a ragged tail over three blocks
SENTINEL = -12345.0


def ties(in_dim):
    """in_dim fp32 values halfway between two bf16 neighbours, in sign pairs: 1 + 2^-8, 1 + 3 2^-8,
    -(1 + 2^-8), -(1 + 3 2^-8), 1 + 5 2^-8, ... -- round to nearest even sends the first of a pair down and
    the second up."""
    k = np.arange(in_dim)
    mag = 1.0 + (4 * (k // 4) + 2 * (k % 2) + 1) * 2.0 ** -8
    return (np.where(k // 2 % 2 == 0, mag, -mag)).astype(np.float32)


def inputs(in_dim, out_dim):
    """[577, in_dim] fp32 uniform in [-2, 2); row 0 all zeros, row 1 the bf16 ties. No subnormals and nothing
    non-finite: the MFMA model has no recorded probe for them."""
    x = np.random.default_rng(1000 + 10 * in_dim + out_dim).uniform(-2.0, 2.0, (max(NS), in_dim)).astype(np.float32)
    x[0] = 0.0
    x[1] = ties(in_dim)
    nz = np.abs(x[x != 0])
    assert np.isfinite(x).all() and (nz >= np.finfo(np.float32).tiny).all() and (np.abs(x) <= 2.0).all()
    return x


def test_the_tie_row_is_made_of_bf16_ties():
    t = ties(13).astype(np.float64)
    assert t[:4].tolist() == [1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8)]
    steps = np.abs(t) * 2.0 ** 8  # bf16's spacing in [1, 2) is 2^-7: a tie is an odd multiple of 2^-8
    assert (steps == np.round(steps)).all() and (steps.astype(np.int64) % 2 == 1).all() and (np.abs(t) < 2).all()


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("in_dim,out_dim", wc.WIDTHS)
def test_qnet_forward_equals_the_mfma_model_at_every_width(in_dim, out_dim, n):
    import torch

    from merging_gym.policy import QNet

    sd, x = wc.width_net(in_dim, out_dim), inputs(in_dim, out_dim)
    qnet = QNet.from_state_dict(sd, device=DEV)
    assert (qnet.in_dim, qnet.out_dim) == (in_dim, out_dim)
    # one row: the zero row, the tie row and a uniform row, each as a launch of its own
    for xs in ([x[r:r + 1] for r in range(3)] if n == 1 else [x[:n]]):
        q = qnet.forward(torch.from_numpy(xs).to(DEV)).cpu().numpy()
        ref = mo.qnet_reference_mfma(sd, xs)
        assert q.shape == ref.shape == (len(xs), out_dim)
        same = q.view(np.uint32) == ref.view(np.uint32)
        assert same.all(), (int((~same.all(1)).sum()), "rows differ; first", np.flatnonzero(~same.all(1))[:4].tolist())
        assert np.isfinite(q).all()


@pytest.mark.parametrize("in_dim,out_dim", wc.WIDTHS)
def test_qnet_forward_padding_columns_and_rows_past_n(in_dim, out_dim):
    """mg_qnet_forward itself at n = 65 into a [65 + 64, 8] buffer: the columns >= out_dim ("padding" in
    include/merging_hip.h: the packed weight rows and bias parts there are zero) are exactly +0.0, the rows
    >= n are not written."""
    import torch

    from merging_gym import _native
    from merging_gym.policy import QNet

    n = 65
    sd, x = wc.width_net(in_dim, out_dim), inputs(in_dim, out_dim)[:n]
    qnet = QNet.from_state_dict(sd, device=DEV)
    xd = torch.from_numpy(x).to(DEV).contiguous()
    q = torch.full((n + 64, 8), SENTINEL, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    _native.check(_native.lib.mg_qnet_forward(qnet.packed.data_ptr(), xd.data_ptr(), in_dim, 0, q.data_ptr(), n, stream),
                  "mg_qnet_forward")
    q = q.cpu().numpy()
    ref = mo.qnet_reference_mfma(sd, x)
    assert np.array_equal(q[:n, :out_dim].view(np.uint32), ref.view(np.uint32))
    assert (q[:n, out_dim:].view(np.uint32) == 0).all()
    assert (q[n:] == np.float32(SENTINEL)).all()


@pytest.mark.parametrize("in_dim,out_dim", [(13, 8), (11, 2), (1, 1)])
def test_swapped_view_is_refused_off_ten_inputs(in_dim, out_dim):
    import torch

    from merging_gym import _native
    from merging_gym.policy import QNet

    qnet = QNet.from_state_dict(wc.width_net(in_dim, out_dim), device=DEV)
    x = torch.zeros((4, in_dim), dtype=torch.float32, device=DEV)
    with pytest.raises(ValueError, match="swap_halves"):
        qnet.forward(x, swap_halves=True)
    q = torch.full((4, 8), SENTINEL, dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream(torch.device(DEV)).cuda_stream
    rc = _native.lib.mg_qnet_forward(qnet.packed.data_ptr(), x.data_ptr(), in_dim, 1, q.data_ptr(), 4, stream)
    assert rc != 0
    assert _native.lib.mg_last_error() == b"mg_qnet_forward: need 1 <= in_dim <= 13 (swap_halves: in_dim 10)"
    torch.cuda.synchronize()
    assert bool((q == SENTINEL).all())  # refused before anything ran
