"""The stand-alone level operators -- ops.level_fwd / ops.level_bwd: k_level_fwd, k_level_bwd2, k_level_bwd1(_dx) and k_grad_reduce of
csrc/ndp_level_f32.inc, k_gen_level_fwd of csrc/ndp_generic.inc -- on the GPU against the float64 restatement of tests/_level_ref.py, at
the sizes where a tile or a strided loop ends: every tensor at the project's bar -- max(4 x the eager float32 restatement's error,
16 float32 ulps of the largest magnitude) --, bit for bit where the arithmetic promises it.  Every accuracy case prints error / bar
before it asserts (profiles/nsfp_level_accuracy.txt is that output).  What the inputs are built to satisfy is asserted in
tests/test_level_edges_cpu.py."""
import functools

import numpy as np
import pytest
import torch

from deformationpyramid_amd import ops
from tests import _level_ref as L
from tests._nsfp_ref import check

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return None if a is None else a.contiguous().to(DEV)


@functools.lru_cache(maxsize=None)
def refs(n, k0):
    """inputs and both restatements, computed once and shared; nothing below writes to them"""
    d, flat = L.level_params()
    x, g = L.kink_free_points(n, k0)[0], L.upstream_gradient(n)
    return (x, g) + L.level_pair(d, flat, x, k0, g)


def check_out_and_move(tag, out, x, r64, r32):
    """x_out at the bar, and x_out - x (exact in float64, for the kernel's output and for the eager one alike) at the bar of the
    movement: its magnitude is a hundredth of |x_out|, so this is the check that sees how the warp depends on x."""
    out, x = out.cpu(), x.double()
    check(f"{tag} x_out", out, r64.x_out, r32.x_out)
    check(f"{tag} x_out - x", out.double() - x, r64.x_out - x, r32.x_out.double() - x)


# ------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("k0", L.LEVEL_K0)
@pytest.mark.parametrize("n", L.LEVEL_FWD_N)
def test_level_forward(n, k0):
    d, flat = L.level_params()
    x, _, r64, r32 = refs(n, k0)
    p, xd = dev(flat), dev(x)
    out, act, heads = ops.level_fwd(d, p, L.LEVEL, k0, xd, save=True)
    tag = f"level fwd se3aa k0={k0} n={n}"
    assert out.shape == (n, 3) and act.shape == (3, ops.cap(n), 128) and heads.shape[0] == ops.cap(n)
    check_out_and_move(tag, out, x, r64, r32)
    for i in range(3):
        check(f"{tag} h{i}", act[i, :n], torch.relu(r64.zs[i]), torch.relu(r32.zs[i]))
    assert torch.equal(ops.level_fwd(d, p, L.LEVEL, k0, xd), out)


@pytest.mark.parametrize("k0", L.LEVEL_K0)
@pytest.mark.parametrize("tag", L.LEVEL_STRIDE_TAGS)
def test_level_forward_grid_stride(tag, k0):
    """1026 tiles on a grid of 1024 workgroups: the tiles reached by the second trip of the tile loop, in k_level_fwd and in
    k_gen_level_fwd (width 64, depth 2), whose cap is the same line of ndp_level_fwd."""
    d, flat = L.level_params(tag)
    x, rows = L.stride_case()
    n = x.shape[0]
    out = ops.level_fwd(d, dev(flat), L.LEVEL, k0, dev(x))
    assert out.shape == (n, 3) and bool(torch.isfinite(out).all())
    r64, r32 = L.level_pair(d, flat, x[rows], k0)
    check_out_and_move(f"level fwd {tag} k0={k0} n={n} ({len(rows)} rows)", out.cpu()[rows], x[rows], r64, r32)


# ------------------------------------------------------------------------------------------ backward
def backward(n, k0, n_part, want_dx=False, poison=None):
    d, flat = L.level_params()
    x, g, _, _ = refs(n, k0)
    p, xd, gd = dev(flat), dev(x), dev(g)
    _, act, heads = ops.level_fwd(d, p, L.LEVEL, k0, xd, save=True)
    if poison is not None:
        act[:, n:] = poison
        heads[n:] = poison
    return ops.level_bwd(d, p, L.LEVEL, k0, xd, act, heads, gd, n_part=n_part, want_dx=want_dx)


@pytest.mark.parametrize("k0", L.LEVEL_K0)
@pytest.mark.parametrize("n,n_part", L.LEVEL_BWD_CASES)
def test_level_backward(n, n_part, k0):
    d, _ = L.level_params()
    _, _, r64, r32 = refs(n, k0)
    got = backward(n, k0, n_part)
    assert got.shape == (d.param_count,) == r64.grad.shape
    tag = f"level bwd se3aa k0={k0} n={n} n_part={n_part}"
    for name, off, shape in d.named_slices():
        s = slice(off, off + int(np.prod(shape)))
        check(f"{tag} {name}", got[s], r64.grad[s], r32.grad[s])
    assert torch.equal(backward(n, k0, n_part), got)
    with_dx, dx = backward(n, k0, n_part, want_dx=True)
    assert torch.equal(with_dx, got) and dx.shape == (n, 3)
    check(f"{tag} dx", dx, r64.dx, r32.dx)


@pytest.mark.parametrize("k0", L.LEVEL_K0)
@pytest.mark.parametrize("n", L.LEVEL_PADDING_N)
def test_level_backward_padding_does_not_contribute(n, k0):
    """Rows n: of the three saved planes and of the saved head rows (head outputs and positional encoding) overwritten with a large
    finite value of either sign.  The kernels DO multiply those rows into their MFMA operands; what multiplies them is dO / dz of a
    padding row, an exact zero, so the product is an exact zero for any finite value (a NaN would not tell a read from a
    contribution: 0 * NaN is NaN)."""
    clean, clean_dx = backward(n, k0, None, want_dx=True)
    assert bool(torch.isfinite(clean).all()) and bool(clean.any()) and bool(torch.isfinite(clean_dx).all())
    for poison in L.POISON:
        grads, dx = backward(n, k0, None, want_dx=True, poison=poison)
        assert torch.equal(grads, clean) and torch.equal(dx, clean_dx), poison
        assert torch.equal(backward(n, k0, None, poison=poison), clean), poison
