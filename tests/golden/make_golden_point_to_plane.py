#!/usr/bin/env python3
"""Generate tests/golden/F19_point_to_plane.npz by RUNNING THE REFERENCE: model.loss.point_2_plane_distance (loss.py:61-92) and its
autograd gradients in both clouds.

Build-container tooling like make_golden.py (whose stubs, reference path and surface_pair it uses): numbers only go into the fixture,
it never runs on the GPU box and nothing in the product imports it.

Inputs: surface_pair(1, n_total=600), 300 source and 246 target points; the normals are the points' unit radial directions
(p / |p|, float32), stored in the file.

  x, y, nx, ny            the inputs, float32
  f32.values / f64.values (p2plane, x_2_plane, y_2_plane) of the reference run in that dtype
  f32.gx, f32.gy / f64.*  d p2plane / dx, d p2plane / dy from the reference's autograd
  idx_x                   float64 nearest y point of every x point (int64); the reference's x_ref_normal is checked to be ny[idx_x]

Usage:  python tests/golden/make_golden_point_to_plane.py
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import install_stubs, save, surface_pair          # noqa: E402


def main():
    install_stubs()
    torch.set_num_threads(8)
    import model.loss as loss_mod
    src, tgt, _, _ = surface_pair(1, n_total=600)
    assert src.shape == (300, 3) and tgt.shape == (246, 3), (src.shape, tgt.shape)
    nx = (src / src.norm(dim=1, keepdim=True)).contiguous()
    ny = (tgt / tgt.norm(dim=1, keepdim=True)).contiguous()
    out = dict(x=src.numpy(), y=tgt.numpy(), nx=nx.numpy(), ny=ny.numpy())
    for dtype, tag in ((torch.float32, "f32"), (torch.float64, "f64")):
        x = src.to(dtype).clone().requires_grad_(True)
        y = tgt.to(dtype).clone().requires_grad_(True)
        total, px, py, ref_n = loss_mod.point_2_plane_distance(x[None], y[None], x_normals=nx.to(dtype)[None], y_normals=ny.to(dtype)[None])
        gx, gy = torch.autograd.grad(total, [x, y])
        assert torch.isfinite(gx).all() and torch.isfinite(gy).all()
        out[f"{tag}.values"] = np.array([total.item(), px.item(), py.item()], dtype=np.float64 if dtype == torch.float64 else np.float32)
        out[f"{tag}.gx"], out[f"{tag}.gy"] = gx.numpy(), gy.numpy()
        if dtype == torch.float64:
            d = ((src.double()[:, None, :] - tgt.double()[None, :, :]) ** 2).sum(-1)
            out["idx_x"] = d.argmin(dim=1).numpy()
            assert torch.equal(ny.double()[out["idx_x"]], ref_n), "x_ref_normal is not y_normals at the float64 nearest neighbours"
        print(f"  {tag}: p2plane {total.item():.8f} = {px.item():.8f} + {py.item():.8f}   max|gx| {gx.abs().max():.3e}  max|gy| {gy.abs().max():.3e}")
    save("F19_point_to_plane", **out)


if __name__ == "__main__":
    main()
