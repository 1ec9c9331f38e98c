"""GPU tests of the pyramid warp's per-point Jacobian (ndp_pyramid_jac), of the transport of normals and of the inverse warp
(ndp_pyramid_inverse), up to Deformation_Pyramid.warp_jacobian / warp_normals / inverse_warp and Registration.inverse_warp.

References: fixture F18 (tests/golden/make_golden_jacobian.py: the reference's own float32 autograd, its float64 beside it), float64
autograd of oracle/ndp_torch_ref.level_forward, and the dx of ndp_level_bwd.  Bars are the project's for derivatives of a level
(tests/test_input_grad.py: rel_err < 1e-4 against float64, < 2e-4 against the reference's float32) and for a level's forward against
the oracle (tests/test_hip_parity.py: 2e-6 absolute, 1e-5 for quaternion / 6D), which is also the Newton tolerance.  J = direct part +
network part, and the network part carries the level's frequency: every per-level case is also checked at k0 = 0, where F18 guarantees
that it is at least a tenth of the direct part (tests/test_jacobian_cpu.py).

The inverse case (gated quaternion, m = 5, k0 = 0) is refused by the fixture's qualification rule (sigma_min = 0.000 at every head
scale, float64 Newton diverges: tests/test_jacobian_cpu.py); it is run with the folded field, where only honest statuses are asked.
The converging inverse through the gate and at the 1e-5 bar, which it was there for, are the cases se3aa_nr.m5.k0 and se3quat.m5.k-8.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests._helpers import GENERIC_SHAPES, VARIANTS, generic_pyramid, rel_err, scale_heads, seeded_pyramid, wsum
from tests.test_input_grad import BAR_F64, BAR_REF32, CASES, GATED, case_key, case_pyramid, cloud

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_TAGS = list(VARIANTS) + list(GATED) + list(GENERIC_SHAPES)
MORE_GATED = {"se3aa_nr": dict(rotation_format="axis_angle", motion="SE3", nonrigidity_est=True)}      # (an inverse case of F18)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


def bar_fwd(tag):
    return 1e-5 if ("quat" in tag or "6d" in tag) else 2e-6


def pyramid_at(tag, seed, k0, m, levels, scale, dev):
    """The seeded pyramid of a variant on the device, heads of `levels` x scale, every level at frequency offset k0."""
    if tag in GENERIC_SHAPES:
        pyr = generic_pyramid(seed, tag, m=m, device=dev)
    else:
        pyr = seeded_pyramid(seed, m=m, device=dev, **{**VARIANTS, **GATED, **MORE_GATED}[tag])
    for lvl in levels:
        scale_heads(pyr, lvl, scale)
    pyr.k0 = k0
    for layer in pyr.pyramid:
        layer.k0 = k0
    pyr.gradient_setup(optimized_level=-1)                          # every level frozen
    return pyr


def level_jac(pyr, lvl, k0, x):
    from deformationpyramid_amd import ops
    return ops.pyramid_jacobian(pyr.descs[-1], pyr.n_hierarchy, k0, pyr.store, x, min_level=lvl, max_level=lvl)


# ------------------------------------------------------------------------------------------------ 1. against the reference
@pytest.mark.parametrize("tag,lvl,k0", CASES, ids=[case_key(*c) for c in CASES])
def test_level_jacobian_golden_from_reference(dev, golden, tag, lvl, k0):
    g = golden("F18_jacobian")
    key = case_key(tag, lvl, k0)
    pyr = pyramid_at(tag, int(g["seed"]), k0, 5 if tag in GENERIC_SHAPES else 9, [lvl], float(g["head_scale"]), dev)
    assert abs(wsum(pyr, lvl) - float(g[f"{key}.wsum"])) < 1e-6 * float(g[f"{key}.wsum"])      # the seeded replay is the fixture's
    x = torch.from_numpy(golden("F2_layer_forward")["x"]).to(dev)
    _, J = level_jac(pyr, lvl, k0, x)
    e = rel_err(J.cpu().numpy(), g[f"{key}.J"])
    print(f"{key}: rel_err J {e:.3e}  (network / direct {float(g[f'{key}.share']):.3g})")
    assert e < BAR_REF32, (key, e)


CHAINS = {"L2_4": ("se3aa", 2, 4), "se3aa": ("se3aa", 0, 8), "sim3eu": ("sim3eu", 0, 8), "se3quat_nr": ("se3quat_nr", 0, 8)}


@pytest.mark.parametrize("name", list(CHAINS))
def test_chained_jacobian_golden_from_reference(dev, golden, name):
    g = golden("F18_jacobian")
    assert list(g["chains"]) == list(CHAINS)
    tag, lo, hi = CHAINS[name]
    pyr = pyramid_at(tag, int(g["seed"]), -8, 9, range(lo, hi + 1), float(g["head_scale"]), dev)
    for i, lvl in enumerate(range(lo, hi + 1)):
        assert abs(wsum(pyr, lvl) - float(g[f"chain.{name}.wsum"][i])) < 1e-6 * float(g[f"chain.{name}.wsum"][i])
    x = torch.from_numpy(golden("F2_layer_forward")["x"]).to(dev)
    _, J = pyr.warp_jacobian(x, max_level=hi, min_level=lo)
    e = rel_err(J.cpu().numpy(), g[f"chain.{name}.J"])
    print(f"chain.{name}: rel_err J {e:.3e}  (network / direct {float(g[f'chain.{name}.share']):.3g})")
    assert e < BAR_REF32, (name, e)


# ------------------------------------------------------------------------------------------------ 2. float64, odd sizes, bounds
def _f64_case(n_max=2000):
    lvl, k0 = 4, 0
    pyr = seeded_pyramid(6, **VARIANTS["se3aa"])
    scale_heads(pyr, lvl, 30.0)
    return pyr, lvl, k0, cloud(n_max, 23)


def _jac64(pyr, lvl, k0, x):
    from oracle import ndp_torch_ref as R
    d = pyr.descs[lvl]
    flat = pyr.store[lvl, :d.param_count].clone()
    x64 = x.double().requires_grad_(True)
    out = R.level_forward(R.split_level(flat.double()), x64, lvl, k0=k0)
    rows = [torch.autograd.grad(out[:, a].sum(), x64, retain_graph=a < 2)[0] for a in range(3)]
    return torch.stack(rows, dim=1).numpy()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1000, 2000])
def test_level_jacobian_sizes_and_bounds(dev, n):
    """J against float64 autograd of the torch restatement at k0 = 0, and through the C entry with J, x_out and the normals in the
    middle of poisoned buffers: nothing outside them is written."""
    from deformationpyramid_amd import _native as N
    pyr, lvl, k0, xs = _f64_case()
    x = xs[:n].contiguous()
    ref = _jac64(pyr, lvl, k0, x)
    store, xd = pyr.store.to(dev), x.to(dev)
    pyr_d = pyr.descs[-1]
    from deformationpyramid_amd import ops
    xo, J = ops.pyramid_jacobian(pyr_d, 9, k0, store, xd, min_level=lvl, max_level=lvl)
    e = rel_err(J.cpu().numpy(), ref)
    print(f"n {n}: rel_err J {e:.3e}")
    assert e < BAR_F64, (n, e)
    nrm = torch.nn.functional.normalize(cloud(n, 31), dim=1).to(dev)
    _, _, nref = ops.pyramid_jacobian(pyr_d, 9, k0, store, xd, min_level=lvl, max_level=lvl, normals=nrm)
    pad, poison = 4099, -7.25e5
    bufs = {k: torch.full((2 * pad + w * n,), poison, device=dev) for k, w in (("x", 3), ("J", 9), ("n", 3))}
    cd = pyr_d.c_struct()
    V = ctypes.c_void_p
    rc = N.lib().ndp_pyramid_jac(ctypes.byref(cd), 9, k0, V(store.data_ptr()), store.stride(0), lvl, lvl, V(xd.data_ptr()), n,
                                 V(bufs["x"].data_ptr() + 4 * pad), V(bufs["J"].data_ptr() + 4 * pad), V(nrm.data_ptr()),
                                 V(bufs["n"].data_ptr() + 4 * pad), N.stream_ptr(dev))
    assert rc == 0
    for k, w, want in (("x", 3, xo), ("J", 9, J), ("n", 3, nref)):
        big = bufs[k].cpu()
        assert torch.equal(big[pad:pad + w * n], want.cpu().reshape(-1)), k
        assert bool((big[:pad] == poison).all()) and bool((big[pad + w * n:] == poison).all()), k


def test_rows_do_not_depend_on_n_or_tile_boundaries(dev):
    from deformationpyramid_amd import ops
    pyr, lvl, k0, xs = _f64_case(1000)
    store = pyr.store.to(dev)
    big = ops.pyramid_jacobian(pyr.descs[-1], 9, k0, store, xs.to(dev), min_level=lvl, max_level=lvl)
    small = ops.pyramid_jacobian(pyr.descs[-1], 9, k0, store, xs[:63].contiguous().to(dev), min_level=lvl, max_level=lvl)
    assert torch.equal(big[0][:63], small[0]) and torch.equal(big[1][:63], small[1])


# ------------------------------------------------------------------------------------------------ 3. against the level backward
@pytest.mark.parametrize("tag", ALL_TAGS)
def test_jacobian_transposed_is_the_dx_of_the_level_backward(dev, tag):
    """J^T g from the new J against ndp_level_bwd's dx: two float32 evaluations of one derivative, each held to BAR_F64 against
    float64 elsewhere, so they differ by less than twice that.  No fixture; every head format."""
    from deformationpyramid_amd import ops
    lvl, k0, n = 4, 0, 1000
    pyr = pyramid_at(tag, 6, k0, 5 if tag in GENERIC_SHAPES else 9, [lvl], 30.0, dev)
    x, gsrc = cloud(n, 23).to(dev), cloud(n, 29, scale=2.0).to(dev)
    _, J = level_jac(pyr, lvl, k0, x)
    d, p = pyr.descs[lvl], pyr.store[lvl]
    _, act, heads = ops.level_fwd(d, p, lvl, k0, x, save=True)
    _, dx = ops.level_bwd(d, p, lvl, k0, x, act, heads, gsrc, want_dx=True)
    jtg = torch.einsum("pa,pab->pb", gsrc.double(), J.double())
    e = rel_err(jtg.cpu().numpy(), dx.cpu().numpy())
    print(f"{tag}: rel_err J^T g against level_bwd dx {e:.3e}   max |J - I| {(J - torch.eye(3, device=dev)).abs().max().item():.3g}")
    assert e < 2 * BAR_F64, (tag, e)


# ------------------------------------------------------------------------------------------------ 4. primal bits
@pytest.mark.parametrize("tag", ["se3aa", "sim3quat", "w100d3_se3quat_nr", "w256d4_sim3eu"])
def test_primal_rows_are_the_bits_of_the_forward(dev, tag):
    from deformationpyramid_amd import ops
    m = 5 if tag in GENERIC_SHAPES else 9
    pyr = pyramid_at(tag, 11, -8, m, range(m), 30.0, dev)
    x = cloud(777, 37).to(dev)
    xj, _ = pyr.warp_jacobian(x)
    assert torch.equal(xj, ops.pyramid_fwd(pyr.descs[-1], m, -8, pyr.store, x))
    with torch.no_grad():
        assert torch.equal(xj, pyr.warp(x)[0])
        xj2, _ = pyr.warp_jacobian(x, max_level=4, min_level=2)
        assert torch.equal(xj2, pyr.warp(x, max_level=4, min_level=2)[0])
    assert not xj.requires_grad


# ------------------------------------------------------------------------------------------------ 5. normals
@pytest.mark.parametrize("tag", ["se3aa", "w64d2_se3aa"])
def test_normals_follow_the_cofactor_matrix(dev, tag):
    m = 5
    pyr = pyramid_at(tag, 11, 0, m, range(m), 30.0, dev)
    x = cloud(1000, 37).to(dev)
    nrm = torch.nn.functional.normalize(cloud(1000, 39), dim=1).to(dev)
    xw, J = pyr.warp_jacobian(x)
    xn, nw = pyr.warp_normals(x, nrm)
    assert torch.equal(xn, xw)
    J64 = J.double()
    cof = torch.linalg.det(J64)[:, None, None] * torch.linalg.inv(J64).transpose(1, 2)
    want = torch.nn.functional.normalize(torch.einsum("pab,pb->pa", cof, nrm.double()), dim=1)
    d = (nw.double() - want).abs().max().item()
    unit = (nw.double().norm(dim=1) - 1).abs().max().item()
    print(f"{tag}: max |n' - normalize(cof(J) n)| {d:.3e}   max | |n'| - 1 | {unit:.3e}   det J in [{torch.linalg.det(J64).min().item():.3f}, {torch.linalg.det(J64).max().item():.3f}]")
    assert d < 1e-6 and unit < 1e-6


def test_identity_warp_returns_the_normals_bit_for_bit(dev):
    """sflow with zeroed head weights and biases is the identity: J = I exactly, cof(J) n = n exactly, and a vector that is unit to
    fp32 accuracy is not renormalised: every fp32-normalised normal comes back bit for bit."""
    pyr = pyramid_at("sflow", 11, -8, 3, [], 1.0, dev)
    for lvl, d in enumerate(pyr.descs):
        with torch.no_grad():
            pyr.store[lvl, d.off_Wh:d.param_count] = 0.0
    axes = torch.tensor([[1.0, 0, 0], [0, -1.0, 0], [0, 0, 1.0]])
    nrm = torch.cat([torch.nn.functional.normalize(cloud(2000, 39), dim=1), axes]).contiguous().to(dev)
    x = cloud(nrm.shape[0], 37).to(dev)
    xw, J = pyr.warp_jacobian(x)
    assert torch.equal(xw, x) and torch.equal(J, torch.eye(3, device=dev).expand_as(J))
    _, nw = pyr.warp_normals(x, nrm)
    assert torch.equal(nw, nrm)
    _, n2 = pyr.warp_normals(x, (3.0 * nrm).contiguous())            # (anything else is normalised)
    assert (n2 - nrm).abs().max().item() <= 2.0 ** -22


# ------------------------------------------------------------------------------------------------ 6. inverse
INVERSE = {"se3aa.m5.k0": ("se3aa", 5, 0), "se3aa.m9.k-8": ("se3aa", 9, -8), "sim3eu.m5.k0": ("sim3eu", 5, 0),
           "se3quat_nr.m5.k0": ("se3quat_nr", 5, 0), "se3aa_nr.m5.k0": ("se3aa_nr", 5, 0), "se3quat.m5.k-8": ("se3quat", 5, -8)}
INVERSE_REFUSED = ["se3quat_nr.m5.k0"]


def _inverse_pyramid(g, name, dev):
    tag, m, k0 = INVERSE[name]
    pyr = pyramid_at(tag, int(g["seed"]), k0, m, range(m), float(g[f"inv.{name}.head_scale"]), dev)
    for lvl in range(m):
        assert abs(wsum(pyr, lvl) - float(g[f"inv.{name}.wsum"][lvl])) < 1e-6 * float(g[f"inv.{name}.wsum"][lvl])
    return pyr, tag


def _recomputed_residual(pyr, x, y):
    with torch.no_grad():
        return (pyr.warp(x)[0] - y).abs().amax(dim=1)


@pytest.mark.parametrize("name", [k for k in INVERSE if k not in INVERSE_REFUSED])
def test_inverse_warp_solves_the_fixture_cases(dev, golden, name):
    """Newton inside one launch.  Iterations: float32 needs at most one pass more than float64 to reach its floor, plus one of slack
    for the last-bit plateau.  Preimage: |x - known| <= 2 bar / sigma_min (first-order propagation of a residual <= bar, the factor
    2 for the second-order term and for the fixture's y being the float32 rounding of a float64 warp)."""
    g = golden("F18_jacobian")
    assert name in list(g["inverse_cases"])
    pyr, tag = _inverse_pyramid(g, name, dev)
    bar = bar_fwd(tag)
    known = cloud(500, 41).to(dev)
    y = torch.from_numpy(g[f"inv.{name}.y"]).to(dev)
    x, info = pyr.inverse_warp(y, iters=8, tol=bar)
    its64, smin = int(g[f"inv.{name}.iters64"]), float(g[f"inv.{name}.sigma_min"])
    res = _recomputed_residual(pyr, x, y)
    err = (x - known).abs().max().item()
    print(f"{name}: converged {int(info.converged.sum())}/500  iterations max {int(info.iterations.max())} (float64: {its64})  "
          f"residual max {res.max().item():.3e} (bar {bar:.1e})  max |x - known| {err:.3e} (bound {2 * bar / smin:.3e})")
    assert bool(info.converged.all())
    assert int(info.iterations.max()) <= its64 + 2
    assert res.max().item() <= bar and torch.equal(res, info.residual)
    assert err <= 2 * bar / smin
    assert not x.requires_grad and info.iterations.dtype == torch.int32
    x1, info1 = pyr.inverse_warp(y, x0=known, iters=8, tol=bar)
    assert bool((info1.iterations == 0).all()) and torch.equal(x1, known)


# ------------------------------------------------------------------------------------------------ 7. folds are reported, not hidden
@pytest.mark.parametrize("name", ["fold", "se3quat_nr.m5.k0"])
def test_folded_fields_are_reported_not_hidden(dev, golden, name):
    g = golden("F18_jacobian")
    known = cloud(500, 41).to(dev)
    if name == "fold":
        pyr = pyramid_at("se3aa", int(g["seed"]), 0, 9, range(9), float(g["head_scale"]), dev)
        for lvl in range(9):
            assert abs(wsum(pyr, lvl) - float(g["fold.wsum"][lvl])) < 1e-6 * float(g["fold.wsum"][lvl])
        y, tol = torch.from_numpy(g["fold.y"]).to(dev), 2e-6
    else:
        assert name in list(g["inverse_refused"])
        pyr, tag = _inverse_pyramid(g, name, dev)
        y, tol = torch.from_numpy(g[f"inv.{name}.y"]).to(dev), bar_fwd(tag)
    x, info = pyr.inverse_warp(y, iters=8, tol=tol)                 # does not raise
    res = _recomputed_residual(pyr, x, y)
    conv = info.converged
    print(f"{name}: converged {int(conv.sum())}/500, not converged {int((info.iterations == -1).sum())}, singular {int((info.iterations == -2).sum())}")
    assert bool((res[conv] <= tol).all()) and torch.equal(res[conv], info.residual[conv])
    assert bool((~conv).any())
    assert bool(((info.iterations >= -2) & (info.iterations <= 8)).all())
    if name == "fold":
        det = torch.linalg.det(pyr.warp_jacobian(known)[1].double()).cpu().numpy()
        ref = g["fold.det64"]
        big = np.abs(ref) > 1e-3
        print(f"fold: det J in [{det.min():.3f}, {det.max():.3f}] (float64 [{ref.min():.3f}, {ref.max():.3f}]), {int(big.sum())} points compared")
        assert (np.sign(det[big]) == np.sign(ref[big])).all()


# ------------------------------------------------------------------------------------------------ 8. through Registration
def test_registration_inverse_warp_returns_the_source(dev, golden):
    from deformationpyramid_amd.config import Config, load_config
    from deformationpyramid_amd.registration import Registration
    g = golden("F7_end_to_end")
    cfg = Config(load_config(os.path.join(ROOT, "config", "NDP.yaml"), device=0), samples=256, m=4, iters=40)
    model = Registration(cfg, gemm_mode=0, nn_matrix=False)
    with pytest.raises(RuntimeError, match="register"):
        model.inverse_warp(g["src"])
    model.load_pcds(g["src"], g["tgt"])
    torch.manual_seed(0)
    warped, _, _ = model.register()
    tol = 2e-6
    p, info = model.inverse_warp(warped, tol=tol)
    conv = info.converged
    print(f"registration: {int(conv.sum())} of {conv.numel()} points converged ({100.0 * conv.float().mean().item():.2f} %), "
          f"iterations max {int(info.iterations.max())}")
    assert bool(conv.any())
    pyr, src_mean, _ = model.fitted_pyramid()
    _, J = pyr.warp_jacobian((p - src_mean).contiguous())
    smin = torch.linalg.svdvals(J.double()).amin(dim=1)
    err = (p - model.src_pcd).abs().amax(dim=1).double()
    worst = (err[conv] * smin[conv] / (2 * tol)).max().item()
    print(f"registration: max |p - src| {err[conv].max().item():.3e}, sigma_min in [{smin[conv].min().item():.3f}, {smin[conv].max().item():.3f}], "
          f"worst error / bound {worst:.3f}")
    assert bool((err[conv] <= 2 * tol / smin[conv]).all())
    # x0 is taken in the frame of the x returned: a solution fed back in is (within a rounding of the two centrings) already one
    p2, info2 = model.inverse_warp(warped, tol=tol, x0=p)
    assert bool(info2.converged[conv].all()) and int(info2.iterations[conv].max()) <= 1
    assert (p2 - p)[conv].abs().max().item() <= 2 * tol / smin[conv].min().item()
