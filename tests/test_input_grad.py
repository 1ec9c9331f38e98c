"""GPU tests of the gradients with respect to the input POINTS: ndp_level_bwd's dx, Deformation_Pyramid.warp through
torch.autograd (several trainable levels, points through a frozen pyramid), the Chamfer loss in its target cloud, and
Registration.fitted_pyramid().

References: fixture F17 (tests/golden/make_golden_input_grad.py: the reference's own float32 autograd) and float64 autograd of
oracle/ndp_torch_ref.level_forward.  Bars are the project's for level gradients (tests/test_hip_parity.py): rel_err < 1e-4 against
a float64 restatement, < 2e-4 against the reference's float32 goldens (rel_err of tests/_helpers.py: max |a - b| / max |b|).  The
reference's float32 against its own float64 is at most 3.4e-6 over F17's cases (tests/test_input_grad_cpu.py keeps that below a
tenth of the bar).  dx = direct term + network term, and the network term carries the level's frequency 2^(level + 1 + k0): at the
shipped k0 = -8 it is a few percent of dx at most, so every case is also checked at k0 = 0, where F17 guarantees that it is at
least a tenth of the direct term (up to 70 times it).
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests._helpers import GENERIC_SHAPES, VARIANTS, generic_pyramid, rel_err, scale_heads, seeded_pyramid, wsum

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAR_F64, BAR_REF32 = 1e-4, 2e-4
GATED = {"se3quat_nr": dict(rotation_format="quaternion", motion="SE3", nonrigidity_est=True)}


def _cases():
    out = []
    for tag in list(VARIANTS) + list(GATED):
        out += [(tag, 4, -8), (tag, 4, 0)]
        if tag in ("se3aa", "sim3eu"):
            out += [(tag, 0, -8), (tag, 8, -8)]
    for tag in GENERIC_SHAPES:
        out += [(tag, 4, -8), (tag, 4, 0)]
    return out


CASES = _cases()                                  # (the CPU tests hold the fixture to exactly this list)


def case_key(tag, lvl, k0):
    return f"{tag}.L{lvl}.k{k0}"


def case_pyramid(tag, seed):
    if tag in GENERIC_SHAPES:
        return generic_pyramid(seed, tag, m=5)
    return seeded_pyramid(seed, **(VARIANTS[tag] if tag in VARIANTS else GATED[tag]))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


def cloud(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, 3, generator=g) - 0.5) * scale).contiguous()


def level_dx(d, p, lvl, k0, x, g, n_part=None):
    from deformationpyramid_amd import ops
    _, act, heads = ops.level_fwd(d, p, lvl, k0, x, save=True)
    return ops.level_bwd(d, p, lvl, k0, x, act, heads, g, n_part=n_part, want_dx=True)


# ------------------------------------------------------------------------------------------------ 1. dx against the reference
@pytest.mark.parametrize("tag,lvl,k0", CASES, ids=[case_key(*c) for c in CASES])
def test_level_dx_golden_from_reference(dev, golden, tag, lvl, k0):
    g = golden("F17_input_grad")
    f2 = golden("F2_layer_forward")
    key = case_key(tag, lvl, k0)
    pyr = case_pyramid(tag, int(g["seed"]))
    scale_heads(pyr, lvl, float(g["head_scale"]))
    assert abs(wsum(pyr, lvl) - float(g[f"{key}.wsum"])) < 1e-6 * float(g[f"{key}.wsum"])      # the seeded replay is the fixture's
    x = torch.from_numpy(f2["x"]).to(dev)
    coef = torch.linspace(-1.0, 1.0, 256 * 3).reshape(256, 3).to(dev)
    d = pyr.descs[lvl]
    grads, dx = level_dx(d, pyr.store[lvl].to(dev), lvl, k0, x, coef)
    e = rel_err(dx.cpu().numpy(), g[f"{key}.dx"])
    print(f"{key}: rel_err dx {e:.3e}  (network / direct {float(g[f'{key}.share']):.3g})")
    assert e < BAR_REF32, (key, e)
    if k0 == -8 and tag in ("se3aa", "sim3eu", "sflow") and lvl == 4:                          # the parameter gradients are F2's still
        got = grads.cpu().numpy()
        for name, off, shape in d.named_slices():
            ref = f2[f"{tag}.L{lvl}.grad.{name}"]
            assert rel_err(got[off:off + ref.size].reshape(ref.shape), ref) < BAR_REF32, (key, name)


# ------------------------------------------------------------------------------------------------ 2. sizes, partials, bounds
@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2000])
def test_level_dx_sizes_partials_and_bounds(dev, n):
    """dx against float64 autograd of the torch restatement at k0 = 0; bit for bit the same for every n_part; and through the C
    entry with dx inside a larger poisoned buffer nothing but its 3 n floats is written."""
    from deformationpyramid_amd import _native as N, ops
    from oracle import ndp_torch_ref as R
    lvl, k0 = 4, 0
    pyr = seeded_pyramid(6, **VARIANTS["se3aa"])
    scale_heads(pyr, lvl, 30.0)
    d = pyr.descs[lvl]
    flat = pyr.store[lvl, :d.param_count].clone()
    x, gsrc = cloud(n, 23), cloud(n, 29, scale=2.0)
    x64 = x.double().requires_grad_(True)
    out = R.level_forward(R.split_level(flat.double()), x64, lvl, k0=k0)
    (out * gsrc.double()).sum().backward()
    ref = x64.grad.numpy()
    p, xd, gd = pyr.store[lvl].to(dev), x.to(dev), gsrc.to(dev)
    got = {}
    for n_part in (1, 3, 16):
        _, dx = level_dx(d, p, lvl, k0, xd, gd, n_part=n_part)
        got[n_part] = dx.cpu()
        e = rel_err(got[n_part].numpy(), ref)
        print(f"n {n} n_part {n_part}: rel_err dx {e:.3e}")
        assert e < BAR_F64, (n, n_part, e)
    assert torch.equal(got[1], got[3]) and torch.equal(got[1], got[16])
    # the C entry, dx in the middle of a poisoned buffer
    pad, poison = 4099, -7.25e5
    big = torch.full((2 * pad + 3 * n,), poison, device=dev)
    _, act, heads = ops.level_fwd(d, p, lvl, k0, xd, save=True)
    stride = (d.param_count + 3) // 4 * 4
    n_part = 3
    part = torch.empty(n_part, stride, device=dev)
    work = torch.empty(ops.cap(n), N.NHMAX, device=dev)
    cd = d.c_struct()
    V = ctypes.c_void_p
    rc = N.lib().ndp_level_bwd(ctypes.byref(cd), V(p.data_ptr()), lvl, k0, V(xd.data_ptr()), n, V(act.data_ptr()), V(heads.data_ptr()),
                               V(gd.data_ptr()), None, V(work.data_ptr()), V(part.data_ptr()), n_part, stride, N.stream_ptr(dev),
                               V(big.data_ptr() + 4 * pad))
    assert rc == 0
    big = big.cpu()
    assert torch.equal(big[pad:pad + 3 * n].view(n, 3), got[3])
    assert bool((big[:pad] == poison).all()) and bool((big[pad + 3 * n:] == poison).all())


# ------------------------------------------------------------------------------------------------ 3. parameter gradients untouched
@pytest.mark.parametrize("tag", ["se3aa", "sim3quat", "se3quat_nr", "w64d2_se3aa", "w100d3_se3quat_nr"])
def test_parameter_gradients_are_the_same_bits_with_dx(dev, tag):
    from deformationpyramid_amd import ops
    lvl, k0, n = 4, -8, 1000
    pyr = case_pyramid(tag, 6)
    scale_heads(pyr, lvl, 30.0)
    d = pyr.descs[lvl]
    p, x, g = pyr.store[lvl].to(dev), cloud(n, 23).to(dev), cloud(n, 29, scale=2.0).to(dev)
    for n_part in (1, 5):
        _, act, heads = ops.level_fwd(d, p, lvl, k0, x, save=True)
        plain = ops.level_bwd(d, p, lvl, k0, x, act, heads, g, n_part=n_part)
        with_dx, dx = level_dx(d, p, lvl, k0, x, g, n_part=n_part)
        assert torch.equal(plain, with_dx), (tag, n_part)
        assert bool(torch.isfinite(dx).all())


# ------------------------------------------------------------------------------------------------ 4. several levels at once
def test_joint_levels_through_warp_and_autograd(dev, golden):
    """warp(x, 4, 2) with levels 2..4 trainable and x requiring a gradient: level 2 receives the loss gradient through levels 3
    and 4, and x through all three."""
    g = golden("F17_input_grad")
    f2 = golden("F2_layer_forward")
    pyr = seeded_pyramid(int(g["seed"]), device=dev, **VARIANTS["se3aa"])
    for lvl in (2, 3, 4):
        scale_heads(pyr, lvl, float(g["head_scale"]))
        assert abs(wsum(pyr, lvl) - float(g[f"joint.wsum.L{lvl}"])) < 1e-6 * float(g[f"joint.wsum.L{lvl}"])
    for i, layer in enumerate(pyr.pyramid):
        for q in layer.parameters():
            q.requires_grad = i in (2, 3, 4)
    x = torch.from_numpy(f2["x"]).to(dev).requires_grad_(True)
    coef = torch.linspace(-1.0, 1.0, 256 * 3).reshape(256, 3).to(dev)
    y, _ = pyr.warp(x, max_level=4, min_level=2)
    (y * coef).sum().backward()
    e = rel_err(x.grad.cpu().numpy(), g["joint.dx"])
    print(f"joint: rel_err dx {e:.3e}")
    assert e < BAR_REF32, e
    for name, q in pyr.pyramid[2].named_parameters():
        assert q.grad is not None, name
        e = rel_err(q.grad.cpu().numpy(), g[f"joint.L2.grad.{name}"])
        print(f"joint: level 2 {name}: rel_err {e:.3e}")
        assert e < BAR_REF32, (name, e)
    assert all(q.grad is not None for lvl in (3, 4) for q in pyr.pyramid[lvl].parameters())
    assert all(q.grad is None for lvl in (0, 1, 5) for q in pyr.pyramid[lvl].parameters())


def test_second_derivatives_raise(dev):
    pyr = seeded_pyramid(3, m=2, device=dev, **VARIANTS["se3aa"])
    x = cloud(100, 5).to(dev).requires_grad_(True)
    y, _ = pyr.warp(x)
    (gx,) = torch.autograd.grad((y ** 2).sum(), x, create_graph=True)          # dL/dy = 2 y carries a graph into the level backward
    with pytest.raises(RuntimeError, match="differentiate twice"):
        gx.sum().backward()


# ------------------------------------------------------------------------------------------------ 5. Chamfer in the target cloud
def test_chamfer_gradient_of_the_target_cloud(dev, golden):
    from deformationpyramid_amd import ops
    from deformationpyramid_amd.loss import compute_truncated_chamfer_distance as cd
    g = golden("F17_input_grad")
    for tag, trunc in (("full", 1e9), ("trunc", 0.01)):
        x0, y0 = torch.from_numpy(g["cd.x"]).to(dev), torch.from_numpy(g["cd.y"]).to(dev)
        x, y = x0.clone().requires_grad_(True), y0.clone().requires_grad_(True)
        L = cd(x[None], y[None], trunc=trunc)
        L.backward()
        assert abs(L.item() - float(g[f"cd.{tag}.loss"])) < 2e-6 * float(g[f"cd.{tag}.loss"])      # (the bar of test_hip_parity.py for F3's loss)
        e = rel_err(y.grad.cpu().numpy(), g[f"cd.{tag}.grad_y"])
        print(f"cd.{tag}: rel_err dy {e:.3e}")
        assert e < BAR_REF32, (tag, e)
        # asking for y.grad leaves the loss and x.grad as they were
        x1 = x0.clone().requires_grad_(True)
        L1 = cd(x1[None], y0[None], trunc=trunc)
        L1.backward()
        assert torch.equal(L1.detach(), L.detach()) and torch.equal(x1.grad, x.grad)
        # symmetry: dL/dy (x, y) is dL/dx (y, x), bit for bit
        y2 = y0.clone().requires_grad_(True)
        ops.chamfer_distance(y2, x0, trunc).backward()
        assert torch.equal(y2.grad, y.grad)
        # only y requires a gradient
        y3 = y0.clone().requires_grad_(True)
        cd(x0[None], y3[None], trunc=trunc).backward()
        assert torch.equal(y3.grad, y.grad)


# ------------------------------------------------------------------------------------------------ 6. points through a frozen pyramid
def test_points_are_optimised_through_a_frozen_pyramid(dev):
    pyr = seeded_pyramid(11, m=5, device=dev, **VARIANTS["se3aa"])
    for lvl in range(5):
        scale_heads(pyr, lvl, 30.0)
    pyr.gradient_setup(optimized_level=-1)                          # every level frozen
    known = cloud(500, 41).to(dev)
    with torch.no_grad():
        target, _ = pyr.warp(known)
    x = (known + cloud(500, 43, scale=0.1).to(dev)).requires_grad_(True)
    opt = torch.optim.Adam([x], lr=0.001)
    dist = []
    for _ in range(20):
        w, _ = pyr.warp(x)
        dist.append((w.detach() - target).norm(dim=1).mean().item())
        loss = ((w - target) ** 2).sum(dim=-1).mean()
        opt.zero_grad()
        loss.backward()
        assert x.grad is not None and bool(torch.isfinite(x.grad).all())
        opt.step()
    with torch.no_grad():
        w, _ = pyr.warp(x)
    dist.append((w - target).norm(dim=1).mean().item())
    print(f"|warp(x) - target|: {dist[0]:.5f} -> {dist[-1]:.5f}")
    assert dist[-1] < dist[0]
    assert all(q.grad is None for layer in pyr.pyramid for q in layer.parameters())


# ------------------------------------------------------------------------------------------------ 7. the fitted pyramid as an object
def _cfg():
    from deformationpyramid_amd.config import Config, load_config
    return Config(load_config(os.path.join(ROOT, "config", "NDP.yaml"), device=0), samples=256, m=4, iters=40)


@pytest.mark.parametrize("mode", ["bitwise", "split"])
def test_fitted_pyramid_reproduces_register(dev, golden, mode):
    from deformationpyramid_amd.registration import Registration
    g = golden("F7_end_to_end")
    kw = dict(gemm_mode=0, nn_matrix=False) if mode == "bitwise" else {}            # {}: the defaults a user gets (split arithmetic)
    model = Registration(_cfg(), **kw)
    with pytest.raises(RuntimeError, match="register"):
        model.fitted_pyramid()
    model.load_pcds(g["src"], g["tgt"])
    torch.manual_seed(0)
    warped, _, _ = model.register()
    pyr, src_mean, tgt_mean = model.fitted_pyramid()
    assert pyr.n_hierarchy == 4 and pyr.store.shape[0] == 4 and src_mean.shape == tgt_mean.shape == (3,)
    src = model.src_pcd
    again = pyr.warp(src - src_mean)[0].detach() + tgt_mean
    if mode == "bitwise":
        assert torch.equal(again, warped)
    else:
        d = (again - warped).abs().max().item()
        print(f"fitted pyramid (fp32 level chain) against register()'s split final warp: max |diff| {d:.3e}")
        assert d < 1e-4
    # the store is a copy: writing into it changes nothing a following register() computes
    with torch.no_grad():
        pyr.store.zero_()
    torch.manual_seed(0)
    warped2, _, _ = model.register()
    assert torch.equal(warped2, warped)
    pyr2, _, _ = model.fitted_pyramid()
    assert pyr2.store.abs().sum().item() > 0
    # ... and its levels are trainable modules: one joint step on all levels
    for q in pyr2.pyramid[0].parameters():
        assert q.requires_grad
    y, _ = pyr2.warp(src - src_mean)
    (y ** 2).sum().backward()
    assert all(q.grad is not None for layer in pyr2.pyramid for q in layer.parameters())
