"""Preconditions of tests/test_level_edges.py, checked without a GPU: the restatement of tests/_level_ref.py is the level of
oracle/ndp_torch_ref (and, at the width the torch oracle does not have, of the C oracle), and the inputs it builds meet the conditions
the float32 / float64 comparison rests on: no ReLU within the kink margin, few candidates left out, gradients in which one dropped tail
row would show far above the bar, and strided tiles whose rows differ from the rows a wrong tile would deliver."""
import numpy as np
import pytest
import torch

from oracle import ndp_oracle as O
from oracle import ndp_torch_ref as R
from tests import _level_ref as L

MAX_DROPPED_SHARE = 0.05
LEVEL_INPUTS = sorted({(n, k0) for n in L.LEVEL_FWD_N + tuple(n for n, _ in L.LEVEL_BWD_CASES) for k0 in L.LEVEL_K0})


def test_case_lists():
    assert L.LEVEL_K0 == (-8, 0) and L.LEVEL_FWD_N == (1, 63, 64, 65, 257) and (L.LEVEL, L.HEAD_SCALE, L.SEED) == (4, 30.0, 6)
    assert L.LEVEL_BWD_CASES == [(1, None), (1, 3), (64, 1), (65, 1), (65, 2), (65, 5), (257, 1), (257, 3), (257, 7), (257, None)]
    assert L.LEVEL_STRIDE_N == 1024 * 64 + 65 == 65601 and L.LEVEL_STRIDE_TAGS == ("se3aa", "w64d2_se3aa")
    assert L.LEVEL_PADDING_N == (65, 257) and L.POISON == (3.0e4, -3.0e4) and L.KINK_MARGIN == 1e-5
    d, flat = L.level_params()
    assert (d.width, d.n_hidden, d.param_count) == (128, 2, 34694) and len(d.named_slices()) == 10 and flat.shape[0] >= d.param_count
    g, _ = L.level_params("w64d2_se3aa")
    assert (g.width, g.n_hidden, g.motion, g.rotfmt) == (64, 1, "SE3", "axis_angle")


# ------------------------------------------------------------------------------------------ the restatement is the oracle's level
@pytest.mark.parametrize("k0", L.LEVEL_K0)
def test_float64_restatement_is_the_torch_oracle(k0):
    d, flat = L.level_params()
    n = 65
    x, g = L.kink_free_points(n, k0)[0].double(), L.upstream_gradient(n).double()
    mine = L.level(d, flat.double(), x, k0, g)
    p = R.split_level(flat[:d.param_count].double())
    xr = x.clone().requires_grad_(True)
    out = R.level_forward(p, xr, L.LEVEL, k0=k0, mlp_scale=L.head_scale(d))
    (out * g).sum().backward()
    assert (mine.x_out - out.detach()).abs().max() <= 1e-15 and (mine.dx - xr.grad).abs().max() <= 1e-13 * xr.grad.abs().max()
    theirs = torch.cat([t.grad.reshape(-1) for t in p])
    assert theirs.shape == mine.grad.shape and (mine.grad - theirs).abs().max() <= 1e-13 * theirs.abs().max()
    plain = R.level_forward(p, x, L.LEVEL, k0=k0)                                # the double 0.001 next to the kernels' float32(0.001)
    assert (plain.detach() - mine.x_out).abs().max() < 1e-7 * (mine.x_out - x).abs().max()


@pytest.mark.parametrize("tag", L.LEVEL_STRIDE_TAGS)
@pytest.mark.parametrize("k0", L.LEVEL_K0)
def test_float32_restatement_agrees_with_the_c_oracle(tag, k0):
    """oracle/ndp_oracle.c is another float32 evaluation of the level, at any width: within the project's bar of float64."""
    d, flat = L.level_params(tag)
    x, rows = L.stride_case()
    x = x[rows]
    r64, r32 = L.level_pair(d, flat, x, k0)
    cd = O.make_desc(d.width, d.n_hidden, d.motion, d.rotfmt, d.nonrigidity, d.mlp_scale)
    out = torch.from_numpy(O.level_fwd(cd, flat[:d.param_count].numpy(), L.LEVEL, k0, x.numpy(), nthreads=4))
    err32, mag = float((r32.x_out.double() - r64.x_out).abs().max()), float(r64.x_out.abs().max())
    assert float((out.double() - r64.x_out).abs().max()) <= L.bar(err32, mag)


# ------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("n,k0", LEVEL_INPUTS)
def test_level_inputs_are_kink_free(n, k0):
    d, flat = L.level_params()
    x, candidates, dropped = L.kink_free_points(n, k0)
    print(f"level se3aa n={n} k0={k0}: {dropped} of {candidates} candidates dropped ({100.0 * dropped / candidates:.2f} %)")
    assert x.shape == (n, 3) and x.dtype == torch.float32 and x.abs().max() <= 0.5 and candidates >= 1024
    assert dropped <= MAX_DROPPED_SHARE * candidates
    r64, r32 = L.level_pair(d, flat, x, k0)
    assert len(r64.zs) == 3 and all(z.shape == (n, 128) for z in r64.zs)
    for z64, z32 in zip(r64.zs, r32.zs):
        assert z64.abs().min() > L.KINK_MARGIN
        assert torch.equal(z64 > 0, z32 > 0)
        assert (z32.double() - z64).abs().max() < L.KINK_MARGIN / 10             # the margin is an order above float32's own z error


def test_the_warp_depends_on_x_more_at_k0_0_than_at_the_shipped_k0():
    """Measured with these parameters: the warp moves points by 0.0004 to 0.013 at k0 = 0 and by 0.0025 to 0.007 at k0 = -8, and the
    movement's standard deviation ACROSS points is 2.4e-3 to 2.9e-3 per coordinate at k0 = 0 against 5e-4 to 9e-4 at k0 = -8.  Either is
    thousands of bars of x_out - x (about 1e-7), so a forward wrong in how the warp depends on x cannot hide in that check."""
    d, flat = L.level_params()
    x = L.uniform_points(4096, 1).double()
    move = {k0: L.level(d, flat.double(), x, k0).x_out - x for k0 in L.LEVEL_K0}
    for k0, m in move.items():
        print(f"level se3aa k0={k0}: |x_out - x| {m.norm(dim=1).min():.4f} .. {m.norm(dim=1).max():.4f}  std across points {m.std(dim=0).tolist()}")
    assert move[0].std(dim=0).min() >= 2e-3 and move[-8].std(dim=0).min() >= 4e-4
    assert move[0].std(dim=0).min() > 2 * move[-8].std(dim=0).max()


def slices(d, flat_grad):
    return [(name, flat_grad[off:off + int(np.prod(shape))]) for name, off, shape in d.named_slices()]


@pytest.mark.parametrize("k0", L.LEVEL_K0)
@pytest.mark.parametrize("n", sorted({n for n, _ in L.LEVEL_BWD_CASES}))
def test_gradients_are_nonzero_and_feel_the_last_point(n, k0):
    """Every checked tensor has a non-zero maximum; from n = 64 on, leaving the LAST point out moves every tensor by more than ten
    bars: a backward that dropped a tail row, or a partial, could not pass."""
    d, flat = L.level_params()
    x, g = L.kink_free_points(n, k0)[0], L.upstream_gradient(n)
    r64, r32 = L.level_pair(d, flat, x, k0, g)
    assert r64.grad.shape == (d.param_count,) and float(r64.dx.abs().max()) > 0
    assert all(float(t.abs().max()) > 0 for _, t in slices(d, r64.grad))
    if n >= 64:
        less = L.level(d, flat.double(), x[:-1].double(), k0, g[:-1].double())
        for (name, full), (_, part), (_, g32) in zip(slices(d, r64.grad), slices(d, less.grad), slices(d, r32.grad)):
            bar = L.bar(float((g32.double() - full).abs().max()), float(full.abs().max()))
            assert float((full - part).abs().max()) > 10 * bar, (name, float((full - part).abs().max()), bar)


@pytest.mark.parametrize("tag", L.LEVEL_STRIDE_TAGS)
@pytest.mark.parametrize("k0", L.LEVEL_K0)
def test_stride_case_rows_tell_their_tiles_apart(tag, k0):
    d, flat = L.level_params(tag)
    x, rows = L.stride_case()
    n = x.shape[0]
    assert n == 1024 * 64 + 65 and (n + 63) // 64 == 1026                                  # two tiles past a grid of 1024, the last of one row
    assert torch.equal(rows, torch.cat([torch.arange(64), torch.arange(1024 * 64, n)])) and len(rows) == 64 + 65
    r64, r32 = L.level_pair(d, flat, x[rows], k0)
    move = r64.x_out - x[rows].double()
    bar = L.bar(float(((r32.x_out.double() - x[rows].double()) - move).abs().max()), float(move.abs().max()))
    assert (move[1:] - move[:-1]).abs().max(dim=1)[0].min() > 10 * bar                     # a row is not its neighbour ...
    late = torch.arange(1024 * 64, n)
    earlier = L.level(d, flat.double(), x[late - 1024 * 64].double(), k0).x_out - x[late - 1024 * 64].double()
    assert (move[64:] - earlier).abs().max(dim=1)[0].min() > 10 * bar                      # ... nor the row its workgroup saw a trip earlier
