"""The neural scene-flow prior's kernels -- csrc/ndp_nsfp.inc, and through it k_level_bwd2 and k_grad_reduce of csrc/ndp_level_f32.inc --
on the GPU against the float64 restatement of tests/_nsfp_ref.py, at the sizes where a tile or a strided loop ends: every tensor at the
project's bar -- max(4 x the eager float32 restatement's error, 16 float32 ulps of the largest magnitude) --, bit for bit where the
arithmetic promises it.  Every accuracy case prints error / bar before it asserts (profiles/nsfp_level_accuracy.txt is that output).
What the inputs are built to satisfy (no ReLU within the kink margin, loud weights, gradients that feel their last row) is asserted in
tests/test_nsfp_edges_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from deformationpyramid_amd import nsfp as NS
from tests import _nsfp_ref as B
from tests._nsfp_ref import check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return None if a is None else a.contiguous().to(DEV)


def check_out_and_flow(tag, out, x, r64, r32):
    """out at the bar, and out - x (exact in float64) at the bar of the FLOW: its magnitude, the eager flow's error.  The kernel forms
    x + flow once in float32, so its flow shows only through an output rounded to the grid of |out|: at most half a float32 spacing
    at |out| <= 1.3, 6e-8, which the 16 ulps of the flow's magnitude cover from a flow of 0.03 up (the flows here: 0.047 to 0.8).
    So the subtraction is given no allowance of its own."""
    out = out.cpu()
    check(f"{tag} out", out, r64.out, r32.out)
    check(f"{tag} out - x", out.double() - x.double(), r64.flow, r32.flow)


@functools.lru_cache(maxsize=None)
def refs(kind, n):
    """inputs and both restatements, computed once and shared; nothing below writes to them"""
    x = B.default_points() if kind == "default" else B.kink_free_points(kind, n)[0]
    gy = B.upstream_gradient(n) if kind == "loud" else None
    return (x, gy) + B.nsfp_pair(B.nsfp_flat(kind), x, gy)


# ------------------------------------------------------------------------------------------ forward
def forward_case(kind, n):
    x, _, r64, r32 = refs(kind, n)
    flat, xd = dev(B.nsfp_flat(kind)), dev(x)
    out, act = NS.nsfp_fwd(flat, xd, save=True)
    tag = f"nsfp fwd {kind} n={n}"
    assert out.shape == (n, 3) and act.shape == (8, (n + 63) // 64 * 64, 128)
    check_out_and_flow(tag, out, x, r64, r32)
    check(f"{tag} h1", act[0, :n], torch.relu(r64.zs[0]), torch.relu(r32.zs[0]))
    assert torch.equal(NS.nsfp_fwd(flat, xd), out)                              # inference form: two ping-pong planes
    out3, act3 = NS.nsfp_fwd(flat, xd, save=True)
    assert torch.equal(out3, out) and torch.equal(act3[:, :n], act[:, :n])


@pytest.mark.parametrize("n", B.NSFP_FWD_N)
def test_nsfp_forward_loud_weights(n):
    forward_case("loud", n)


def test_nsfp_forward_default_init():
    """The workload's regime: the flow is nearly the same for every point."""
    forward_case("default", B.NSFP_DEFAULT_N)


def test_nsfp_forward_grid_stride():
    """514 tiles on k_nsfp_dense's grid of 512: the tiles reached by the second trip of its loop (what the final all-point flow of
    optimize_neural_SFlow runs from 32769 points on)."""
    x, rows, _, _ = B.stride_case()
    n, flat = x.shape[0], B.nsfp_flat("loud")
    out = NS.nsfp_fwd(dev(flat), dev(x))
    assert out.shape == (n, 3) and bool(torch.isfinite(out).all())
    r64, r32 = B.nsfp_pair(flat, x[rows])
    check_out_and_flow(f"nsfp fwd loud n={n} ({len(rows)} rows)", out.cpu()[rows], x[rows], r64, r32)


# ------------------------------------------------------------------------------------------ backward
def backward(kind, n, n_part, poison=None):
    x, gy, _, _ = refs(kind, n)
    flat, xd, gd = dev(B.nsfp_flat(kind)), dev(x), dev(gy)
    act = NS.nsfp_fwd(flat, xd, save=True)[1]
    if poison is not None:
        act[:, n:] = poison
    return NS.nsfp_bwd(flat, xd, act, gd, n_part=n_part)


@pytest.mark.parametrize("n,n_part", B.NSFP_BWD_CASES)
def test_nsfp_backward(n, n_part):
    _, _, r64, r32 = refs("loud", n)
    got = backward("loud", n, n_part)
    assert got.shape == (NS.PARAM_COUNT,) == r64.grad.shape
    for name, g, g64, g32 in zip(B.names(), B.split(got), B.split(r64.grad), B.split(r32.grad)):
        check(f"nsfp bwd n={n} n_part={n_part} {name}", g, g64, g32)
    assert torch.equal(backward("loud", n, n_part), got)
    if (n, n_part) == (257, None):                                               # the C oracle stays tied in: its error is of the kernel's class
        from oracle import ndp_oracle as O
        x, gy = refs("loud", n)[:2]
        want = torch.from_numpy(O.nsfp_bwd(B.nsfp_flat("loud").numpy(), x.numpy(), gy.numpy()))
        for name, g, g64, g32 in zip(B.names(), B.split(want), B.split(r64.grad), B.split(r32.grad)):
            check(f"nsfp bwd n={n} C oracle {name}", g, g64, g32)


@pytest.mark.parametrize("n", B.NSFP_PADDING_N)
def test_nsfp_backward_padding_does_not_contribute(n):
    """Rows n: of the eight saved planes overwritten with a large finite value of either sign.  The kernels DO multiply those rows
    into their MFMA operands; what multiplies them is dO / dz of a padding row, an exact zero, so the product is an exact zero for
    any finite value (a NaN would not tell a read from a contribution: 0 * NaN is NaN)."""
    clean = backward("loud", n, None)
    assert bool(torch.isfinite(clean).all()) and bool(clean.any())
    for poison in B.POISON:
        assert torch.equal(backward("loud", n, None, poison=poison), clean), poison
