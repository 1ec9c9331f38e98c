"""Plain-torch restatement of one SE3 / axis-angle level as ops.level_fwd / ops.level_bwd compute it (k_level_fwd, k_level_bwd2,
k_level_bwd1, k_grad_reduce of csrc/ndp_level_f32.inc; k_gen_level_fwd for other widths), with the inputs and the case lists of
tests/test_level_edges.py.  It is oracle/ndp_torch_ref.level_forward with the width and the number of layers taken from the
descriptor, returning the pre-activations too; it follows the dtype of its input: float64 is the yardstick, float32 the eager
arithmetic whose own error sets the project's bar (tests/_kpconv_ref.bar).  tests/test_level_edges_cpu.py holds it to
oracle/ndp_torch_ref and the inputs to their preconditions.

The head scale is the float32 the kernels hold (the descriptor's C struct carries a float), cast up: float32(0.001) and the double
0.001 differ by 4.7e-8 of every head output, which is the function's definition and not an error of its evaluation.
Inputs as in tests/_nsfp_ref.py: points whose 3 x 128 (depth x width) float64 pre-activations all have |z| > KINK_MARGIN, a seeded
uniform upstream gradient of sum(x_out * g), seed-6 pyramid, level 4, head weights and biases x 30, at k0 = -8 (shipped: the warp
is nearly one rigid motion) and k0 = 0 (the warp's dependence on x is loud).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F

from ._helpers import GENERIC_SHAPES, VARIANTS, generic_pyramid, scale_heads, seeded_pyramid
from ._kpconv_ref import ULP, bar  # noqa: F401  (re-exported: the tests take them from here)
from ._nsfp_ref import NSFP_BWD_CASES, POISON, TILE, stride_rows, uniform_points, upstream_gradient  # noqa: F401

KINK_MARGIN = 1e-5
LEVEL, HEAD_SCALE, SEED = 4, 30.0, 6
LEVEL_K0 = (-8, 0)
LEVEL_FWD_N = (1, 63, 64, 65, 257)
LEVEL_BWD_CASES = list(NSFP_BWD_CASES)                              # (n, n_part)
LEVEL_STRIDE_N = 1024 * 64 + 65                                     # 1026 tiles: the forward kernels' grid of 1024 strides once
LEVEL_STRIDE_TAGS = ("se3aa", "w64d2_se3aa")                        # k_level_fwd, k_gen_level_fwd
LEVEL_PADDING_N = (65, 257)


@functools.lru_cache(maxsize=None)
def level_params(tag="se3aa"):
    """-> (descriptor, float32 parameter block of level LEVEL padded to the pyramid's stride), heads x HEAD_SCALE."""
    pyr = generic_pyramid(SEED, tag, m=5) if tag in GENERIC_SHAPES else seeded_pyramid(SEED, **VARIANTS[tag])
    scale_heads(pyr, LEVEL, HEAD_SCALE)
    d = pyr.descs[LEVEL]
    assert d.motion == "SE3" and d.rotfmt == "axis_angle" and not d.nonrigidity
    return d, pyr.store[LEVEL].clone().contiguous()


def split(d, flat):
    """flat block -> [W0, b0, W1, b1, ..., Wh, bh] views (Wh: 3 rotation rows, 3 translation rows)."""
    out = []
    for i in range(d.n_hidden + 1):
        cols = 6 if i == 0 else d.width
        out.append(flat[d.off_W(i):d.off_W(i) + d.width * cols].reshape(d.width, cols))
        out.append(flat[d.off_b(i):d.off_b(i) + d.width])
    out.append(flat[d.off_Wh:d.off_bh].reshape(d.n_heads, d.width))
    out.append(flat[d.off_bh:d.off_bh + d.n_heads])
    return out


def head_scale(d):
    return float(np.float32(d.mlp_scale))


def level(d, flat, x, k0, g=None, lvl=LEVEL):
    """flat [>= P], x [n,3] of one dtype -> zs (pre-activations [n,width], one per layer), x_out and, with g [n,3], the gradient of
    sum(x_out * g) in the parameters (flat layout, [P]) and in x."""
    flat = flat[:d.param_count].detach().clone().requires_grad_(g is not None)
    x = x.detach().clone().requires_grad_(g is not None)
    p = split(d, flat)
    fx = 2.0 ** (lvl + 1 + k0) * x
    h = torch.stack([fx.sin(), fx.cos()], dim=-1).reshape(x.shape[0], 6)        # [sin fx0, cos fx0, sin fx1, ...]
    zs = []
    for i in range(d.n_hidden + 1):
        zs.append(F.linear(h, p[2 * i], p[2 * i + 1]))
        h = F.relu(zs[-1])
    o = head_scale(d) * F.linear(h, p[-2], p[-1])
    r, t = o[:, :3], o[:, 3:]
    theta = r.norm(dim=1, keepdim=True)
    w = r / theta
    z = torch.zeros_like(w[:, 0])
    K = torch.stack([z, -w[:, 2], w[:, 1], w[:, 2], z, -w[:, 0], -w[:, 1], w[:, 0], z], dim=1).reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=x.dtype).expand_as(K)
    R = eye + theta.sin()[..., None] * K + ((1.0 - theta.cos())[..., None] * K) @ K
    x_out = (R @ x[..., None])[..., 0] + t
    grad = dx = None
    if g is not None:
        (x_out * g).sum().backward()
        grad, dx = flat.grad.detach(), x.grad.detach()
    return SimpleNamespace(zs=[v.detach() for v in zs], x_out=x_out.detach(), grad=grad, dx=dx)


def level_pair(d, flat32, x32, k0, g32=None):
    """The float64 yardstick and the eager float32 restatement on the same float32 inputs."""
    c = lambda a: None if a is None else a.double()
    return level(d, c(flat32), c(x32), k0, c(g32)), level(d, flat32, x32, k0, g32)


def kink_margin(d, flat32, x32, k0):
    """min over the depth x width float64 pre-activations of |z|, per point."""
    zs = level(d, flat32.double(), x32.double(), k0).zs
    return torch.stack([z.abs().min(dim=1)[0] for z in zs]).min(dim=0)[0]


@functools.lru_cache(maxsize=None)
def kink_free_points(n, k0, seed=41):
    """-> (x [n,3] float32: the first n candidates, uniform in [-0.5, 0.5]^3, whose margin on the shipped shape exceeds KINK_MARGIN;
    candidates examined; candidates dropped).  At least 1024 candidates are examined."""
    d, flat = level_params()
    c = max(1024, int(math.ceil(1.3 * n)))
    cand = uniform_points(c, seed + n + 1000 * (k0 + 8))
    keep = kink_margin(d, flat, cand, k0) > KINK_MARGIN
    assert int(keep.sum()) >= n
    return cand[keep][:n].contiguous(), c, int((~keep).sum())


@functools.lru_cache(maxsize=None)
def stride_case():
    """x [LEVEL_STRIDE_N, 3] uniform and the rows to compare: 0..63 and every row from 65536 on (the two tiles past the grid of 1024).
    Unfiltered: only the forward runs on them, and the forward is continuous across a ReLU's kink."""
    return uniform_points(LEVEL_STRIDE_N, 79), stride_rows(LEVEL_STRIDE_N, 1024)
