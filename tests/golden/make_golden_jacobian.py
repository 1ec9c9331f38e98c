#!/usr/bin/env python3
"""Generate tests/golden/F18_jacobian.npz by RUNNING THE REFERENCE's autograd: the per-point Jacobian J = d warp(x) / d x of single
levels and of level chains, inverse-warp cases (y = warp(known) with the float64 Newton iteration count and the smallest singular
value of J) and one folded field.

Build-container tooling like make_golden_input_grad.py (whose stubs, seeded pyramids, head scale and 256 points of F2 it uses):
numbers only go into the fixture, it never runs on the GPU box and nothing in the product imports it.

  cases                       the keys of the per-level cases: tests.test_input_grad.CASES (imported, not restated)
  <key>.J                     J [256, 3, 3], J[p, a, b] = d x'_a / d x_b: the reference's float32 autograd
  <key>.J64_minus_J           its float64 autograd as the float32 difference to .J (J64 = J + J64_minus_J to about 1e-14: half the
                              bytes of a float64 array, which would put the file over its 900 KB ceiling)
  <key>.wsum                  sum |parameter| of the level (catches a drift of the seeded replay)
  <key>.rel64                 rel_err(J, J64)  (max |a - b| / max |b|, tests/_helpers.py)
  <key>.share                 max |J64 - J_direct| / max |J_direct|, J_direct the Jacobian with the network outputs detached (the
                              positional encoding's output cut from the graph): what a comparison relative to max |J| can see of
                              the tangent code.  A k0 = 0 case below 0.1 is refused (F17's rule, for F17's reason).
  chain.<name>.*              the same for level chains at k0 = -8, heads x 30 on the chained levels: L2_4 (se3aa, levels 2..4) and
                              the whole m = 9 pyramid of se3aa, sim3eu and the gated quaternion variant; .wsum per chained level
  inv.<name>.*                inverse cases, seed 11, 500 points `known` = cloud(500, 41) of tests/test_input_grad.py:
                              y = float32(float64 warp(known)), iters64 = float64 Newton steps from x0 = y until max |r| <= 1e-15
                              (or 16 ulp of the largest |y| where that is more: the quaternion case moves points by more than 1),
                              sigma_min = smallest singular value of the float64 J over the points, head_scale as used, wsum [m].
                              A case with iters64 > 6 or sigma_min < 0.5 does not qualify (8 float32 iterations are a safe ceiling
                              only for one that does): the head scale is dropped until it does.  se3quat_nr.m5.k0 never does --
                              a quaternion head is normalised, so its rotation is the same at every head scale, and at k0 = 0 it
                              turns by whole rotations between neighbouring points (sigma_min 0.000 at every scale from 30 to 1;
                              even at k0 = -8 the gate's 0.5 (I + R) leaves sigma_min 0.244) -- and is REFUSED: it is listed in
                              `inverse_refused`, not in `inverse_cases`, with its figures at x 30 (iters64 = -1) and its y, on
                              which the GPU tests only ask for honest statuses, as on the folded field.  What that case was
                              there for is covered by two further cases under the same rule: se3aa_nr.m5.k0 (the gate, axis-angle,
                              k0 = 0) and se3quat.m5.k-8 (a quaternion head, the 1e-5 bar).
  fold.*                      se3aa, m = 9, k0 = 0, heads x 30: y = warp(known), det64 = float64 det J at `known`, wsum [m]

Usage:  python tests/golden/make_golden_jacobian.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from make_golden import install_stubs, save                                                    # noqa: E402
from make_golden_input_grad import GATED, GENERIC_SHAPES, HEAD_SCALE, SEED, VARIANTS, rel_err    # noqa: E402

MIN_SHARE_K0_0 = 0.1
MAX_ITERS64, MIN_SIGMA = 6, 0.5


def build(nets, kw, k0, m, levels, scale=HEAD_SCALE):
    """The seeded pyramid of the tests (generator seed 11, the heads of `levels` x scale)."""
    kw = dict(dict(depth=3, width=128), **kw)
    torch.manual_seed(SEED)
    pyr = nets.Deformation_Pyramid(device="cpu", k0=k0, m=m, **kw)
    with torch.no_grad():
        for lvl in levels:
            for k, v in pyr.pyramid[lvl].named_parameters():
                if "branch" in k or "brach" in k:
                    v.mul_(scale)
    return pyr


def wsum(pyr, lvl):
    return sum(v.double().abs().sum().item() for v in pyr.pyramid[lvl].parameters())


def cloud(n, seed, scale=1.0):                                  # tests/test_input_grad.py: cloud
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, 3, generator=g) - 0.5) * scale).contiguous()


def warp_and_jac(pyr, x, lo, hi, dtype, direct=False):
    """-> (warp(x, hi, lo), J [n,3,3]) by three autograd passes in `dtype`; direct: with every level's encoding cut from the graph."""
    for layer in pyr.pyramid:
        layer.to(dtype)
    saved = []
    if direct:
        for layer in pyr.pyramid[lo:hi + 1]:
            orig = layer.posenc
            layer.posenc = (lambda pos, f=orig: f(pos).detach())
            saved.append(layer)
    try:
        xx = x.to(dtype).clone().requires_grad_(True)
        y, _ = pyr.warp(xx, max_level=hi, min_level=lo)
        rows = [torch.autograd.grad(y[:, a].sum(), xx, retain_graph=a < 2)[0] for a in range(3)]
    finally:
        for layer in saved:
            del layer.posenc
    return y.detach(), torch.stack(rows, dim=1)


def jac_case(pyr, x, lo, hi, key, out, need_share=None):
    _, J32 = warp_and_jac(pyr, x, lo, hi, torch.float32)
    _, J64 = warp_and_jac(pyr, x, lo, hi, torch.float64)
    _, Jd = warp_and_jac(pyr, x, lo, hi, torch.float64, direct=True)
    share = float((J64 - Jd).abs().max() / Jd.abs().max())
    r = rel_err(J32.numpy(), J64.numpy())
    assert torch.isfinite(J32).all() and torch.isfinite(J64).all(), key
    if need_share is not None and not share >= need_share:
        raise SystemExit(f"{key}: network term is {share:.3g} of the direct Jacobian (< {need_share}): not a test of the tangents; not written")
    out[f"{key}.J"], out[f"{key}.J64_minus_J"] = J32.numpy(), (J64 - J32.double()).float().numpy()
    out[f"{key}.rel64"], out[f"{key}.share"] = np.float64(r), np.float64(share)
    print(f"  {key:30s} max|J - I| {(J64 - torch.eye(3)).abs().max():.3e}  share {share:.3e}  rel64 {r:.2e}", flush=True)


def newton64(pyr, y, lo, hi, floor=1e-15, cap=30):
    """float64 Newton on warp(x) = y from x0 = y -> (steps until every point has max |r| <= floor, or None; x; last residuals)."""
    x = y.double().clone()
    floor = max(floor, 16 * 2.0 ** -52 * float(y.abs().max()))      # (a residual cannot fall below a few ulp of the coordinates)
    for it in range(cap + 1):
        w, J = warp_and_jac(pyr, x, lo, hi, torch.float64)
        r = w - y.double()
        res = r.abs().amax(dim=1)
        if bool((res <= floor).all()):
            return it, x, res
        if it == cap or not torch.isfinite(res).all():
            break
        x = x - torch.linalg.solve(J, r[..., None])[..., 0]
    return None, x, res


def main():
    install_stubs()
    torch.set_num_threads(8)
    import model.nets as nets
    from tests.test_input_grad import CASES, case_key
    out = {}
    g = torch.Generator().manual_seed(7)
    x = torch.rand(256, 3, generator=g) - 0.5                       # F2's x
    out["head_scale"], out["seed"] = np.float32(HEAD_SCALE), np.int64(SEED)
    kws = {**VARIANTS, **GATED, **GENERIC_SHAPES, "se3aa_nr": dict(rotation_format="axis_angle", motion="SE3", nonrigidity_est=True)}
    names = []
    for tag, lvl, k0 in CASES:
        key = case_key(tag, lvl, k0)
        pyr = build(nets, kws[tag], k0, 5 if tag in GENERIC_SHAPES else 9, [lvl])
        out[f"{key}.wsum"] = np.float64(wsum(pyr, lvl))
        jac_case(pyr, x, lvl, lvl, key, out, need_share=MIN_SHARE_K0_0 if k0 == 0 else None)
        names.append(key)
    out["cases"] = np.array(names)
    # ---- chains (k0 = -8)
    chains = [("L2_4", "se3aa", 2, 4), ("se3aa", "se3aa", 0, 8), ("sim3eu", "sim3eu", 0, 8), ("se3quat_nr", "se3quat_nr", 0, 8)]
    for name, tag, lo, hi in chains:
        pyr = build(nets, kws[tag], -8, 9, range(lo, hi + 1))
        out[f"chain.{name}.wsum"] = np.array([wsum(pyr, l) for l in range(lo, hi + 1)])
        jac_case(pyr, x, lo, hi, f"chain.{name}", out)
    out["chains"] = np.array([c[0] for c in chains])
    # ---- inverse cases
    known = cloud(500, 41)
    inv = [("se3aa.m5.k0", "se3aa", 5, 0), ("se3aa.m9.k-8", "se3aa", 9, -8), ("sim3eu.m5.k0", "sim3eu", 5, 0), ("se3quat_nr.m5.k0", "se3quat_nr", 5, 0),
           # what the refused case was there for, each under the same rule: the nonrigidity gate at k0 = 0, and a rotation format of the 1e-5 bar
           ("se3aa_nr.m5.k0", "se3aa_nr", 5, 0), ("se3quat.m5.k-8", "se3quat", 5, -8)]
    refused = []
    for name, tag, m, k0 in inv:
        tried = []
        for scale in (30.0, 20.0, 15.0, 10.0, 7.0, 5.0, 3.0, 1.0):
            pyr = build(nets, kws[tag], k0, m, range(m), scale=scale)
            y64, J64 = warp_and_jac(pyr, known, 0, m - 1, torch.float64)
            smin = float(torch.linalg.svdvals(J64).min())
            y = y64.float()
            its, x64, res = newton64(pyr, y, 0, m - 1)
            print(f"  inv.{name}: head scale {scale}: float64 Newton steps {its}  sigma_min {smin:.3f}  max|x - known| {(x64 - known.double()).abs().max():.2e}", flush=True)
            ok = its is not None and its <= MAX_ITERS64 and smin >= MIN_SIGMA
            tried.append((scale, y, its, smin, [wsum(pyr, l) for l in range(m)]))
            if ok:
                break
            if tag == "se3aa":
                raise SystemExit(f"inv.{name}: float64 Newton needs {its} steps, sigma_min {smin:.3f}: not written")
        if not ok:
            # No head scale qualifies (a quaternion head is normalised: its rotation does not depend on the scale): REFUSED as an
            # inverse case.  Its name goes into `inverse_refused` with the figures of the first scale (iters64 = -1) and its y,
            # which the GPU tests use like the folded field: the statuses must be honest, nothing is asked of convergence.
            print(f"  inv.{name}: NO head scale qualifies -- refused (listed in inverse_refused, iters64 = -1)", flush=True)
            tried = tried[:1]
            refused.append(name)
        scale, y, its, smin, ws = tried[-1]
        out[f"inv.{name}.y"], out[f"inv.{name}.iters64"] = y.numpy(), np.int64(-1 if its is None else its)
        out[f"inv.{name}.sigma_min"], out[f"inv.{name}.head_scale"] = np.float64(smin), np.float32(scale)
        out[f"inv.{name}.wsum"] = np.array(ws)
    out["inverse_cases"] = np.array([c[0] for c in inv if c[0] not in refused])
    out["inverse_refused"] = np.array(refused, dtype="U32")
    # ---- the folded field
    pyr = build(nets, kws["se3aa"], 0, 9, range(9))
    y64, J64 = warp_and_jac(pyr, known, 0, 8, torch.float64)
    det = torch.linalg.det(J64)
    its, _, res = newton64(pyr, y64.float(), 0, 8)
    print(f"  fold: det J in [{det.min():.3f}, {det.max():.3f}], {(det <= 0).sum().item()} of 500 points with det <= 0; float64 Newton from y: "
          f"{'all converged in ' + str(its) if its is not None else str(int((~(res <= 1e-15)).sum())) + ' points not converged'}", flush=True)
    assert bool((det <= 0).any())
    out["fold.y"], out["fold.det64"] = y64.float().numpy(), det.numpy()
    out["fold.wsum"] = np.array([wsum(pyr, l) for l in range(9)])
    save("F18_jacobian", **out)
    size = os.path.getsize(os.path.join(HERE, "F18_jacobian.npz"))
    if size > 900 * 1024:
        raise SystemExit(f"F18_jacobian.npz is {size} bytes (> 900 KB)")


if __name__ == "__main__":
    main()
