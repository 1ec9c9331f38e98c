#!/usr/bin/env python3
"""Drop-in counterpart of the reference's shape_transfer.py (/root/reference/shape_transfer.py:25-170): Sim(3) /
euler deformation pyramid fitted between two meshes, then applied to every vertex of the source mesh.

    python shape_transfer.py -s sim3_demo/AlienSoldier.ply -t sim3_demo/Ortiz.ply [-o warped.ply]
                             [--jacobian-stats] [--pull-back pulled.ply] [--plane-stats] [--voxel-size DL]

Same hard-wired settings as upstream (:27-52): 6000 surface samples per mesh, ALL of them used as Chamfer samples,
m = 9, k0 = -8, lr 0.01, 500 iterations with the early-stop rule, Sim3 + euler; like upstream the target mean is
NOT added back to the warped vertices (:164-167).  The optimisation loop is the device-resident engine (the same
level/Adam/early-stop semantics the upstream script spells out inline, :116-157); open3d mesh I/O and viewers are
replaced by an ASCII-PLY reader/writer and an area-weighted sampler (deformationpyramid_amd/meshio.py).

Three optional extras on top of upstream (without them the output is unchanged): --jacobian-stats prints det J of the fitted warp at
the mesh vertices (local volume change; det J <= 0 marks where the field folded over), --pull-back FILE maps the TARGET mesh's
vertices into the source frame through the inverse warp (Registration.inverse_warp) and writes them with the target's faces,
--plane-stats prints the mean point-to-plane residual |(x - p) . n| of the source samples against the target samples and their face
normals before and after the fit (both clouds centred as the fit sees them): a quality figure that needs no ground truth.
--voxel-size DL fits on the voxel-grid barycentres (edge DL) of the two meshes' vertices instead of the surface samples -- an even
cover whatever the tessellation -- and still warps every source vertex; without it nothing changes.
"""
import argparse

import numpy as np
import torch

from deformationpyramid_amd import ops
from deformationpyramid_amd.config import Config
from deformationpyramid_amd.meshio import read_ply_ascii, sample_surface, write_ply_ascii
from deformationpyramid_amd.registration import Registration
from deformationpyramid_amd.utils import setup_seed

setup_seed(0)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("-s", type=str, required=True, help="Path to the src mesh.")
    ap.add_argument("-t", type=str, required=True, help="Path to the tgt mesh.")
    ap.add_argument("-o", type=str, default="", help="write the warped source mesh here (ASCII PLY)")
    ap.add_argument("--jacobian-stats", action="store_true", help="print min / median / max of det J at the warped vertices and the folded share")
    ap.add_argument("--pull-back", type=str, default="", metavar="FILE",
                    help="write the target mesh's vertices mapped into the source frame (inverse warp) here (ASCII PLY)")
    ap.add_argument("--plane-stats", action="store_true",
                    help="print the mean point-to-plane residual of the source samples against the target samples' normals before and after the fit")
    ap.add_argument("--voxel-size", type=float, default=0.0, metavar="DL",
                    help="fit on the voxel barycentres (edge DL, ops.voxel_subsample) of both meshes' vertices instead of 6000 surface "
                         "samples per mesh; every vertex of the source is still warped (default 0: off)")
    args = ap.parse_args()
    if args.voxel_size < 0:
        ap.error("--voxel-size must be positive (0: off)")
    config = Config({
        "gpu_mode": True, "deformation_model": "NDP",
        "iters": 500, "lr": 0.01, "max_break_count": 15, "break_threshold_ratio": 0.001,
        "samples": 6000, "motion_type": "Sim3", "rotation_format": "euler",
        "m": 9, "k0": -8, "depth": 3, "width": 128, "act_fn": "relu",
        "w_reg": 0, "w_ldmk": 0, "w_cd": 0.1,
    })
    config.device = torch.cuda.current_device()

    rng = np.random.default_rng(0)
    src_v, src_f = read_ply_ascii(args.s)
    tgt_v, tgt_f = read_ply_ascii(args.t)
    src_pcd = sample_surface(src_v, src_f, config.samples, rng)
    tgt_pcd, tgt_nrm = sample_surface(tgt_v, tgt_f, config.samples, rng, return_normals=True)     # (the same draws and points as without)
    if args.voxel_size > 0:
        if args.plane_stats:
            ap.error("--plane-stats needs the surface samples' normals: not together with --voxel-size")
        thin = lambda v: ops.voxel_subsample(torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda(), [len(v)], args.voxel_size)[0].cpu().numpy()
        src_pcd, tgt_pcd = thin(src_v), thin(tgt_v)
        print("fitting on", len(src_pcd), "and", len(tgt_pcd), "voxel barycentres of", len(src_v), "and", len(tgt_v), "vertices")

    model = Registration(config)
    model.load_pcds(src_pcd, tgt_pcd)
    warped_samples, iter_cnt, _ = model.register()          # samples == all points: randperm only reorders them
    print("loss evaluations per level:", [iter_cnt[l] for l in range(config.m)], " final loss:", model.last_state.loss)

    # warp the original mesh vertices with the optimised pyramid (shape_transfer.py:160-166)
    dev = torch.device("cuda", config.device)
    src_mean = torch.from_numpy(src_pcd).to(dev).mean(dim=0, keepdim=True)
    verts = torch.from_numpy(src_v).to(dev) - src_mean
    eng = model._engines[0]
    warped_vert = ops.pyramid_fwd(eng.desc, config.m, config.k0, eng.params[0], verts.contiguous()).cpu().numpy()
    print("warped", warped_vert.shape[0], "vertices; bbox", warped_vert.min(0), warped_vert.max(0))
    if args.o:
        write_ply_ascii(args.o, warped_vert, src_f)
        print("wrote", args.o)
    if args.jacobian_stats:
        _, J = ops.pyramid_jacobian(eng.desc, config.m, config.k0, eng.params[0], verts.contiguous())
        det = torch.linalg.det(J.double().cpu())
        print(f"det J at {det.numel()} vertices: min {det.min().item():.6g}  median {det.median().item():.6g}  max {det.max().item():.6g}"
              f"  folded (det J <= 0): {100.0 * (det <= 0).double().mean().item():.3f} %")
    if args.plane_stats:
        src_c = (torch.from_numpy(src_pcd).to(dev) - src_mean).contiguous()
        tgt_c = torch.from_numpy(tgt_pcd).to(dev)
        tgt_c = (tgt_c - tgt_c.mean(dim=0, keepdim=True)).contiguous()
        ny = torch.from_numpy(tgt_nrm).to(dev).contiguous()
        moved = ops.pyramid_fwd(eng.desc, config.m, config.k0, eng.params[0], src_c)
        fig = [float(ops.point_to_plane(c, tgt_c, torch.zeros_like(c), ny, mode=1, want_grad=False)[0][1]) for c in (src_c, moved)]
        print(f"point-to-plane residual of {src_c.shape[0]} source samples against the target samples' normals: "
              f"before {fig[0]:.6g}  after {fig[1]:.6g}")
    if args.pull_back:
        pulled, info = model.inverse_warp(tgt_v)
        write_ply_ascii(args.pull_back, pulled.cpu().numpy(), tgt_f)
        print("wrote", args.pull_back, "--", int((~info.converged).sum().item()), "of", pulled.shape[0], "vertices did not converge")
