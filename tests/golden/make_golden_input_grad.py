#!/usr/bin/env python3
"""Generate tests/golden/F17_input_grad.npz by RUNNING THE REFERENCE's autograd: gradients of warp() and of the truncated
Chamfer loss with respect to their input POINTS.

Build-container tooling like make_golden.py (whose stubs and reference path it uses): numbers only go into the fixture, it
never runs on the GPU box and nothing in the product imports it.

Inputs are F2's (x of 256 points from generator seed 7, pyramid seed 11, head weights x 30) and the linspace(-1, 1)
coefficient cloud g of test_level_bwd_golden_from_reference: L = sum(g * warp(x)).

  <tag>.L<l>.k<k0>.dx        dL/dx, float32 autograd of the reference                         [256, 3]
  <tag>.L<l>.k<k0>.wsum      sum |parameter| of the level (catches a drift of the seeded replay)
  <tag>.L<l>.k<k0>.rel64     rel_err(float32 dx, float64 dx) of the reference itself (max |a - b| / max |b|)
  <tag>.L<l>.k<k0>.share     max |network term| / max |direct term| of dx in float64, where the network term is what arrives through
                             the positional encoding, f (cos . dpe_sin - sin . dpe_cos) with dpe the gradient the encoding's OUTPUT
                             receives (the layer's posenc is wrapped so that its output retains its gradient), and the direct term
                             is dx minus that
  joint.*                    se3aa, warp(x, 4, 2) with levels 2..4 trainable and x requiring a gradient: level 2's parameter
                             gradients and dL/dx
  cd.<full|trunc>.grad_y     F3's clouds with y.requires_grad: dL/dy

dx is the sum of a direct term of the size of g and the network term, which carries the factor f = 2^(level + 1 + k0).  At the
shipped k0 = -8 the network term is a few percent of the direct one at best, so that a relative-to-maximum comparison of dx would
pass a wrong network term; every case is therefore ALSO captured at k0 = 0 (f = 32 at level 4), and this script refuses to write a
k0 = 0 case whose network term is below a tenth of the direct one.

Usage:  python tests/golden/make_golden_input_grad.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import install_stubs, save          # noqa: E402

HEAD_SCALE = 30.0
SEED = 11
MIN_SHARE_K0_0 = 0.1

# tests/_helpers.py: VARIANTS, one gated 128 / 3 variant, GENERIC_SHAPES (kept separate on purpose: this file does not import the product)
VARIANTS = {
    "se3aa": dict(rotation_format="axis_angle", motion="SE3"),
    "sim3eu": dict(rotation_format="euler", motion="Sim3"),
    "sflow": dict(rotation_format="axis_angle", motion="sflow"),
    "se3eu": dict(rotation_format="euler", motion="SE3"),
    "sim3aa": dict(rotation_format="axis_angle", motion="Sim3"),
    "se3quat": dict(rotation_format="quaternion", motion="SE3"),
    "se36d": dict(rotation_format="6D", motion="SE3"),
    "sim3quat": dict(rotation_format="quaternion", motion="Sim3"),
}
GATED = {"se3quat_nr": dict(rotation_format="quaternion", motion="SE3", nonrigidity_est=True)}
GENERIC_SHAPES = {
    "w64d2_se3aa": dict(width=64, depth=2, rotation_format="axis_angle", motion="SE3"),
    "w256d4_sim3eu": dict(width=256, depth=4, rotation_format="euler", motion="Sim3"),
    "w32d1_sflow": dict(width=32, depth=1, rotation_format="axis_angle", motion="sflow"),
    "w100d3_se3quat_nr": dict(width=100, depth=3, rotation_format="quaternion", motion="SE3", nonrigidity_est=True),
}


def rel_err(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-30))


def build(nets, kw, k0, m, levels):
    """The seeded pyramid of the tests (generator seed 11, the heads of `levels` x 30)."""
    kw = dict(dict(depth=3, width=128), **kw)
    torch.manual_seed(SEED)
    pyr = nets.Deformation_Pyramid(device="cpu", k0=k0, m=m, **kw)
    with torch.no_grad():
        for lvl in levels:
            for k, v in pyr.pyramid[lvl].named_parameters():
                if "branch" in k or "brach" in k:
                    v.mul_(HEAD_SCALE)
    return pyr


def input_grad(pyr, x, coef, lo, hi, dtype):
    """dL/dx of L = sum(coef * warp(x, hi, lo)) in `dtype`; with lo == hi also the network term of it."""
    for layer in pyr.pyramid:
        layer.to(dtype)
    xx = x.to(dtype).clone().requires_grad_(True)
    kept = {}
    layer = pyr.pyramid[lo]
    orig = layer.posenc

    def posenc(pos):
        pe = orig(pos)
        pe.retain_grad()
        kept["pe"] = pe
        return pe

    if lo == hi:
        layer.posenc = posenc
    try:
        for l in pyr.pyramid:
            for p in l.parameters():
                p.grad = None
        y, _ = pyr.warp(xx, max_level=hi, min_level=lo)
        (y * coef.to(dtype)).sum().backward()
    finally:
        if lo == hi:
            del layer.posenc
    dx = xx.grad.detach()
    net = None
    if lo == hi:
        pe, dpe = kept["pe"].detach(), kept["pe"].grad
        f = 2.0 ** (layer.m + layer.k0)
        net = torch.stack([f * (pe[:, 2 * k + 1] * dpe[:, 2 * k] - pe[:, 2 * k] * dpe[:, 2 * k + 1]) for k in range(3)], dim=1)
    return dx, net


def main():
    install_stubs()
    torch.set_num_threads(8)
    import model.nets as nets
    import model.loss as loss_mod
    out = {}
    g = torch.Generator().manual_seed(7)
    x = torch.rand(256, 3, generator=g) - 0.5                       # F2's x
    coef = torch.linspace(-1.0, 1.0, 256 * 3).reshape(256, 3)
    out["head_scale"], out["seed"] = np.float32(HEAD_SCALE), np.int64(SEED)
    cases = []
    for tag, kw in {**VARIANTS, **GATED}.items():
        cases += [(tag, kw, 9, 4, -8), (tag, kw, 9, 4, 0)]
        if tag in ("se3aa", "sim3eu"):
            cases += [(tag, kw, 9, 0, -8), (tag, kw, 9, 8, -8)]
    for tag, kw in GENERIC_SHAPES.items():
        cases += [(tag, kw, 5, 4, -8), (tag, kw, 5, 4, 0)]
    names = []
    for tag, kw, m, lvl, k0 in cases:
        key = f"{tag}.L{lvl}.k{k0}"
        pyr = build(nets, kw, k0, m, [lvl])
        wsum = sum(v.double().abs().sum().item() for v in pyr.pyramid[lvl].parameters())
        dx32, _ = input_grad(pyr, x, coef, lvl, lvl, torch.float32)
        dx64, net64 = input_grad(pyr, x, coef, lvl, lvl, torch.float64)
        direct64 = dx64 - net64
        share = float(net64.abs().max() / direct64.abs().max())
        r = rel_err(dx32.numpy(), dx64.numpy())
        assert torch.isfinite(dx32).all() and torch.isfinite(dx64).all(), key
        if k0 == 0 and not share >= MIN_SHARE_K0_0:
            raise SystemExit(f"{key}: network term is {share:.3g} of the direct term (< {MIN_SHARE_K0_0}): not a test of dpe; not written")
        out[f"{key}.dx"] = dx32.numpy()
        out[f"{key}.wsum"] = np.float64(wsum)
        out[f"{key}.rel64"] = np.float64(r)
        out[f"{key}.share"] = np.float64(share)
        names.append(key)
        print(f"  {key:28s} max|dx| {dx32.abs().max():.4f}  share {share:.3e}  rel64 {r:.2e}", flush=True)
    out["cases"] = np.array(names)
    # ---- joint: levels 2..4 trainable, x requires a gradient
    for dtype, sfx in ((torch.float32, ""), (torch.float64, "64")):
        pyr = build(nets, VARIANTS["se3aa"], -8, 9, [2, 3, 4])
        if dtype == torch.float32:
            for lvl in (2, 3, 4):
                out[f"joint.wsum.L{lvl}"] = np.float64(sum(v.double().abs().sum().item() for v in pyr.pyramid[lvl].parameters()))
        for i, layer in enumerate(pyr.pyramid):
            for p in layer.parameters():
                p.requires_grad = i in (2, 3, 4)
        dx, _ = input_grad(pyr, x, coef, 2, 4, dtype)
        if dtype == torch.float32:
            out["joint.dx"] = dx.numpy()
            for k, v in pyr.pyramid[2].named_parameters():
                out[f"joint.L2.grad.{k}"] = v.grad.numpy().copy()
            g32 = {k: v.grad.numpy().copy() for k, v in pyr.pyramid[2].named_parameters()}
            dx32 = dx
        else:
            out["joint.rel64"] = np.float64(rel_err(dx32.numpy(), dx.numpy()))
            out["joint.L2.rel64"] = np.float64(max(rel_err(g32[k], v.grad.numpy()) for k, v in pyr.pyramid[2].named_parameters()))
    print(f"  joint: max|dx| {np.abs(out['joint.dx']).max():.4f}  max|grad L2 W1| {np.abs(out['joint.L2.grad.mlp.pts_linears.0.weight']).max():.3e}"
          f"  rel64 dx {out['joint.rel64']:.2e}  L2 {out['joint.L2.rel64']:.2e}", flush=True)
    # ---- Chamfer: F3's clouds, gradient of the TARGET side
    g = torch.Generator().manual_seed(3)
    cx = torch.rand(300, 3, generator=g) - 0.5
    cy = (torch.rand(257, 3, generator=g) - 0.5) * 1.1 + 0.02
    out["cd.x"], out["cd.y"] = cx.numpy(), cy.numpy()
    for tag, trunc in (("full", 1e9), ("trunc", 0.01)):
        res = {}
        for dtype in (torch.float32, torch.float64):
            yy = cy.to(dtype).clone().requires_grad_(True)
            L = loss_mod.compute_truncated_chamfer_distance(cx.to(dtype)[None], yy[None], trunc=trunc)
            L.backward()
            res[dtype] = (L.item(), yy.grad.numpy().copy())
        out[f"cd.{tag}.loss"] = np.float32(res[torch.float32][0])
        out[f"cd.{tag}.grad_y"] = res[torch.float32][1]
        out[f"cd.{tag}.rel64"] = np.float64(rel_err(res[torch.float32][1], res[torch.float64][1]))
        print(f"  cd.{tag}: loss {res[torch.float32][0]:.6f}  max|dy| {np.abs(res[torch.float32][1]).max():.3e}  rel64 {out[f'cd.{tag}.rel64']:.2e}", flush=True)
    save("F17_input_grad", **out)


if __name__ == "__main__":
    main()
