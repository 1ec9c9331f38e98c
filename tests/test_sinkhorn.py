"""Sinkhorn baseline on the GPU: the kernels of csrc/ndp_sinkhorn.inc against the float64 restatement of tests/_sinkhorn_ref.py.

The bar is measured per case and per tensor (the four potentials, the loss, the gradient): the kernels' max-abs error against
float64 may be at most the larger of
    4 x the error of the SAME restatement run eagerly in float32 on the same inputs   (tiled summation order, hardware exp2), and
    16 float32 ulps of the tensor's largest magnitude                                 (where the eager error happens to be ~0).
Every case prints its ratios (error / bar) before it asserts; profiles/sinkhorn_accuracy.txt is that output."""
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _sinkhorn_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n, m, blur, reach, scaling)
CASES = [(1, 1, .1, 1, .5), (1, 65, .1, 1, .5), (63, 1, .1, 1, .5), (64, 64, .1, 1, .5), (65, 129, .1, 1, .5), (257, 300, .1, None, .5),
         (500, 400, .01, 1, .5), (300, 300, .1, .3, .9), (2000, 1999, .1, 1, .5)]
# the kernel's own boundaries: 16 rows per workgroup and 16 lanes per row (15 / 17), 128 columns per chunk round (127; 129 is above),
# 1024 columns per LDS tile (1023 / 1025), on the y side and -- the x cloud is the column set of two softmins -- on the x side
EDGES = [(15, 17, .1, 1, .5), (17, 15, .1, None, .5), (33, 127, .1, 1, .5), (20, 1023, .1, 1, .5), (24, 1025, .1, None, .5),
         (1025, 31, .1, 1, .5), (1023, 1024, .1, 1, .5)]


def ulps16(t):
    return 16.0 * float(np.spacing(np.float32(float(t.abs().max()))))


def bar(r64, r32):
    """(name, float64 tensor, bound) for the four potentials, the loss and the gradient."""
    out = []
    for name, a, b in [(k, r64.potentials[i], r32.potentials[i]) for i, k in enumerate(("F_ba", "F_aa", "G_ab", "G_bb"))] + \
                      [("loss", r64.loss.reshape(1), r32.loss.reshape(1)), ("grad", r64.grad, r32.grad)]:
        out.append((name, a, max(4.0 * float((b.double() - a).abs().max()), ulps16(a))))
    return out


@functools.lru_cache(maxsize=None)
def case(n, m, blur, reach, scaling):
    """Inputs and both restatements of one case, computed once and shared (never modified)."""
    x, y = R.box_clouds(n, m, 1000 * n + m)
    return x, y, R.sinkhorn_ref(x, y, blur, reach, scaling), R.sinkhorn_ref(x, y, blur, reach, scaling, dtype=torch.float32)


def run(x, y, blur, reach, scaling=0.5, **kw):
    from deformationpyramid_amd import ops
    return ops.sinkhorn_divergence(x.cuda().contiguous(), y.cuda().contiguous(), blur, reach, scaling, want_potentials=True, **kw)


def check(tag, got, r64, r32):
    loss, grad, pot = got
    n, m = r64.grad.shape[0], r64.potentials[2].shape[0]
    mine = dict(zip(("F_ba", "F_aa", "G_ab", "G_bb"), torch.split(pot.cpu().double(), [n, n, m, m])), loss=loss.cpu().double(), grad=grad.cpu().double())
    worst = []
    for name, ref, bound in bar(r64, r32):
        err = float((mine[name] - ref).abs().max())
        assert np.isfinite(err), (tag, name)
        worst.append((name, err, bound))
    print(f"sinkhorn_accuracy {tag} eps_entries={r64.n_eps} " + " ".join(f"{k}={e / b:.3f}({e:.2e}/{b:.2e})" for k, e, b in worst))
    for name, err, bound in worst:
        assert err <= bound, (tag, name, err, bound)


@pytest.mark.parametrize("n,m,blur,reach,scaling", CASES + EDGES)
def test_against_float64(n, m, blur, reach, scaling):
    x, y, r64, r32 = case(n, m, blur, reach, scaling)
    check(f"n={n} m={m} blur={blur} reach={reach} scaling={scaling}", run(x, y, blur, reach, scaling), r64, r32)


@pytest.mark.parametrize("reach", [None, 1])
def test_equal_clouds(reach):
    x, _ = R.box_clouds(300, 1, 7)
    r64 = R.sinkhorn_ref(x, x.clone(), .1, reach)
    r32 = R.sinkhorn_ref(x, x.clone(), .1, reach, dtype=torch.float32)
    loss, grad, pot = run(x, x.clone(), .1, reach)
    floor = ulps16(r64.potentials[0])                           # the loss and the gradient are differences of terms of this size
    assert abs(float(loss)) <= floor and float(grad.abs().max()) <= floor
    F = torch.split(pot.cpu().double(), [300] * 4)
    for i, (name, ref, bound) in enumerate(bar(r64, r32)[:4]):
        assert float((F[i] - ref).abs().max()) <= bound, (name, reach)
    other = R.sinkhorn_ref(x, x.clone(), .1, None if reach else 1)
    gap = float((other.potentials[0] - r64.potentials[0]).abs().max())
    assert gap > 1e-3                                           # balanced and unbalanced potentials differ, by what the restatement says:
    assert float((F[0] - other.potentials[0]).abs().max()) > gap / 2


def test_run_to_run_bits():
    from deformationpyramid_amd import ops
    x, y, _, _ = case(2000, 1999, .1, 1, .5)
    xd, yd = x.cuda(), y.cuda()
    a = ops.sinkhorn_divergence(xd, yd, .1, 1, want_potentials=True)
    b = ops.sinkhorn_divergence(xd, yd, .1, 1, want_potentials=True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    loss, grad, pot = ops.sinkhorn_divergence(xd, yd, .1, 1, want_grad=False)
    assert grad is None and pot is None and torch.equal(loss, a[0])


def sinkhorn_registration(src, tgt, samples, nsteps=11):
    from deformationpyramid_amd.config import Config
    from deformationpyramid_amd.registration import Registration
    cfg = Config(deformation_model="Sinkhorn", device=torch.device("cuda:0"), samples=samples, blur=0.1, reach=1, Nsteps=nsteps, lr=1)
    model = Registration(cfg)
    model.load_pcds(src, tgt)
    return model


def test_run_optimal_transport_follows_the_float64_euler_loop():
    src, tgt = R.box_clouds(600, 590, 11)
    tgt = tgt - 0.05                                            # 0.1 apart
    model = sinkhorn_registration(src, tgt, samples=1000)       # more samples than points: every point is used
    torch.manual_seed(5)
    warped, select_ind = model.register()
    state = torch.get_rng_state()
    with pytest.raises(NotImplementedError):
        model.register(visualize=True)
    torch.manual_seed(5)
    perm_s, perm_t = torch.randperm(600), torch.randperm(590)
    assert torch.equal(torch.get_rng_state(), state)            # the generator is left where two randperms leave it
    assert warped.is_cuda and select_ind.is_cuda and warped.shape == (600, 3)
    assert torch.equal(select_ind.cpu(), perm_s)
    # the float64 loop on the same samples; the per-step bound is the gradient's bar (above) at that step's clouds, and the Euler
    # update multiplies a gradient error by lr * n, so after Nsteps the bound is  Nsteps x lr x n x (largest per-step bound)
    x, y = src[perm_s].double(), tgt[perm_t]
    per_step = 0.0
    for _ in range(11):
        r64 = R.sinkhorn_ref(x.float(), y, .1, 1)
        r32 = R.sinkhorn_ref(x.float(), y, .1, 1, dtype=torch.float32)
        per_step = max(per_step, bar(r64, r32)[5][2])
        x = x - 1 * len(x) * R.sinkhorn_ref(x, y, .1, 1).grad
    bound = 11 * 1 * 600 * per_step
    err = float((warped.cpu().double() - x).abs().max())
    print(f"sinkhorn_accuracy euler n=600 m=590 steps=11 err={err:.2e} bound={bound:.2e} ratio={err / bound:.3f}")
    assert err <= bound
    assert float((warped.cpu().mean(0) - tgt.mean(0)).norm()) < 0.2 * float((src.mean(0) - tgt.mean(0)).norm())   # and it registers


def test_run_optimal_transport_samples():
    src, tgt = R.box_clouds(700, 650, 12)
    model = sinkhorn_registration(src, tgt, samples=256, nsteps=2)
    torch.manual_seed(3)
    warped, select_ind = model.register()
    torch.manual_seed(3)
    assert warped.shape == (256, 3) and torch.equal(select_ind.cpu(), torch.randperm(700)[:256])
    assert torch.isfinite(warped).all()


def test_driver_runs_the_shipped_config(tmp_path):
    out = subprocess.run([sys.executable, os.path.join(ROOT, "eval_nolearned.py"), "--config",
                          os.path.join(ROOT, "config", "baselines", "Sinkhorn.yaml"), "--synthetic", "2"],
                         capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    line = re.search(r"2/2: (.*)", out.stdout)
    assert line, out.stdout[-800:]
    vals = re.findall(r"(\S+): (\S+)", line.group(1))           # "key: value" for every metric of every subset
    assert len(vals) >= 4 and all(np.isfinite(float(v)) for _, v in vals), line.group(1)
