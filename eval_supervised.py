#!/usr/bin/env python3
"""Drop-in counterpart of the reference's eval_supervised.py (/root/reference/eval_supervised.py:40-190) for the
LNDP path (landmark-guided deformation pyramid) on the MI355X engine.

    python eval_supervised.py --config config/LNDP.yaml [--batched] [--synthetic N] [--landmarks DIR]

Upstream predicts the landmark correspondences with the Lepard matcher (`Landmark_Model.inference`, :102), which
is outside this repository's scope.  Here they are *precomputed*: `--landmarks DIR` holds one
`<pair stem>.npz` per 4DMatch pair with `ldmk_s [K,3]`, `ldmk_t [K,3]` (un-centred coordinates, what
`ldmk_model.inference` returns); without it -- or without the dataset -- seeded synthetic pairs get K = 500 landmarks
`(src[idx], GT-warped src[idx] + N(0, 0.005^2))`.  Everything after the matcher
is upstream's flow: GT scene flow and overlap mask (:111-124), `load_pcds(src, tgt, landmarks=(ldmk_s, ldmk_t))`,
`register()`, `compute_flow_metrics`, `AverageMeter`, timers.

`--descriptors DIR [--match-type dual_softmax|sinkhorn|mutual_nn]` (off by default; without it the output is unchanged) matches
the landmarks from per-point descriptors on the GPU (deformationpyramid_amd/matching.py): each `<stem>.npz` holds `pts_s, pts_t,
feat_s, feat_t`; without the dataset seeded descriptors are planted on the synthetic pairs' landmark points.  It composes with:
`--rigid-landmarks THR` (off by default; without it the output is unchanged) also runs RANSAC on every pair's landmarks
(`deformationpyramid_amd/rigid.py`) and prints a `rigid-*` row -- how much of the ground-truth flow one rigid motion explains -- with
the mean inlier ratio; `--rigid-landmarks-filter` then registers on the inlier landmarks only.
`--outlier-weights FILE [--outlier-thr 0.5]` (off by default; without it the output is unchanged) passes every pair's landmarks --
precomputed, matched from descriptors or synthetic -- through the reference's learned outlier filter (`Landmark_Model.inference`'s
`vec_6d[inlier_conf > inlier_thr]`, deformationpyramid_amd/outlier.py) before anything else sees them, and prints the mean kept share;
FILE is the reference's `{'state_dict': ...}` checkpoint of `Outlier_Rejection` at configs/outlier_rejection.yaml.
"""
import argparse
import os

import numpy as np
import torch

from deformationpyramid_amd.config import load_config
from deformationpyramid_amd.loss import compute_flow_metrics
from deformationpyramid_amd.registration import Registration
from deformationpyramid_amd.synthetic import synthetic_descriptors, synthetic_landmarks, synthetic_pair
from deformationpyramid_amd.utils import AverageMeter, Logger, Timers, setup_seed
from deformationpyramid_amd.parallel import shard_range
from eval_nolearned import FourDMatchPairs, dist_setup, reduce_meters


def make_parser():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", type=str, default="config/LNDP.yaml", help="Path to the config file.")
    ap.add_argument("--visualize", action="store_true", help="(upstream flag; mayavi is out of scope here)")
    ap.add_argument("--batched", action="store_true", help="register all pairs through register_batch")
    ap.add_argument("--slots", type=int, default=64)
    ap.add_argument("--synthetic", type=int, default=32, help="pairs to generate when the dataset is absent")
    ap.add_argument("--landmarks", type=str, default="", help="directory of precomputed <stem>.npz (ldmk_s, ldmk_t)")
    ap.add_argument("--K", type=int, default=500, help="synthetic landmarks per pair")
    ap.add_argument("--rigid-landmarks", type=float, default=0.0, metavar="THR",
                    help="RANSAC a rigid motion through each pair's landmarks (inlier distance THR): adds a rigid-* metric row and the mean inlier ratio")
    ap.add_argument("--rigid-landmarks-filter", action="store_true", help="with --rigid-landmarks: register on the inlier landmarks only")
    ap.add_argument("--descriptors", type=str, default=None, metavar="DIR",
                    help="match landmarks from per-point descriptors: directory of <stem>.npz (pts_s, pts_t, feat_s, feat_t); "
                         "without the dataset, seeded descriptors planted on the synthetic pairs' landmark points")
    ap.add_argument("--match-type", type=str, default="dual_softmax", choices=["dual_softmax", "sinkhorn", "mutual_nn"],
                    help="with --descriptors: the matcher (deformationpyramid_amd/matching.py)")
    ap.add_argument("--outlier-weights", type=str, default=None, metavar="FILE",
                    help="filter every pair's landmarks with the learned outlier rejection network: its {'state_dict': ...} checkpoint")
    ap.add_argument("--outlier-thr", type=float, default=0.5, help="with --outlier-weights: keep the landmarks whose inlier confidence exceeds this")
    return ap


def outlier_rows(items, weights, thr):
    """The learned outlier filter on every pair's landmarks (deformationpyramid_amd/outlier.py) -> (kept shares, items with the
    landmarks filtered; a pair that would keep fewer than 3 keeps all of them)."""
    from deformationpyramid_amd import outlier
    dev = torch.device("cuda", torch.cuda.current_device())
    model = outlier.Outlier_Rejection(outlier.DEFAULT_CONFIG)
    model.load_state_dict(torch.load(weights, map_location="cpu")["state_dict"], strict=True)
    model = model.to(dev).eval()
    shares, out = [], []
    for src, tgt, flow_gt, overlap, (ls, lt) in items:
        keep, _ = outlier.reject_landmarks(model, ls, lt, thr)
        keep = keep.cpu()
        shares.append(float(keep.float().mean()) if keep.numel() else 0.0)
        if int(keep.sum()) >= 3:
            ls, lt = ls[keep].contiguous(), lt[keep].contiguous()
        out.append((src, tgt, flow_gt, overlap, (ls, lt)))
    return shares, out


def descriptor_landmarks(d, match_type):
    """pts_s, pts_t, feat_s, feat_t -> (ldmk_s, ldmk_t) on the CPU, matched on the GPU (deformationpyramid_amd/matching.py)."""
    from deformationpyramid_amd.matching import landmarks_from_descriptors
    dev = torch.device("cuda", torch.cuda.current_device())
    ls, lt = landmarks_from_descriptors(*(torch.as_tensor(np.asarray(d[k])).float().to(dev) for k in ("pts_s", "pts_t", "feat_s", "feat_t")),
                                        match_type=match_type)
    return ls.cpu(), lt.cpu()


def rigid_rows(items, thr, keep_inliers):
    """RANSAC on every pair's landmarks (deformationpyramid_amd/rigid.py) -> (rigid flows R src + t - src, inlier ratios, items with
    the landmarks filtered when keep_inliers)."""
    from deformationpyramid_amd.rigid import reject_landmarks
    flows, ratios, out = [], [], []
    for src, tgt, flow_gt, overlap, (ls, lt) in items:
        mask, R, t = reject_landmarks(ls, lt, thr)
        mask, R, t = mask.cpu(), R.cpu(), t.cpu()
        flows.append(src @ R.T + t - src)
        ratios.append(float(mask.float().mean()))
        if keep_inliers and int(mask.sum()) >= 3:
            ls, lt = ls[mask].contiguous(), lt[mask].contiguous()
        out.append((src, tgt, flow_gt, overlap, (ls, lt)))
    return flows, ratios, out


def main():
    args = make_parser().parse_args()
    world, rank, local_rank, backend = dist_setup()              # torchrun: pairs sharded over ranks (BASELINE config 5)
    setup_seed(rank)
    config = load_config(args.config, make_dirs=rank == 0, device=local_rank)
    if config.deformation_model != "NDP":
        raise KeyError(config.deformation_model)
    model = Registration(config)
    timer = Timers()
    for benchmark in ["4DMatch-F", "4DLoMatch-F"]:
        config.split["test"] = benchmark
        root = os.path.join(config.data_root, benchmark)
        items = []
        have_data = os.path.isdir(root) and bool(args.landmarks or args.descriptors)
        if have_data:
            data = FourDMatchPairs(config.data_root, benchmark)
            n_total = len(data)
            for i in range(*shard_range(n_total, rank, world)):
                src, tgt, flow_gt, overlap = data[i]
                stem = os.path.splitext(os.path.basename(data.files[i]))[0]
                if args.descriptors:
                    ldmk = descriptor_landmarks(np.load(os.path.join(args.descriptors, stem + ".npz")), args.match_type)
                else:
                    lm = np.load(os.path.join(args.landmarks, stem + ".npz"))
                    ldmk = (torch.from_numpy(lm["ldmk_s"]).float(), torch.from_numpy(lm["ldmk_t"]).float())
                items.append((src, tgt, flow_gt, overlap, ldmk))
        else:
            if rank == 0:
                print(f"[{benchmark}] dataset or --landmarks missing: {args.synthetic} synthetic pairs, K = {args.K} landmarks")
            n_total = args.synthetic
            for p in range(*shard_range(n_total, rank, world)):
                src, tgt, flow_gt, overlap = synthetic_pair(p)
                ldmk = synthetic_landmarks(p, src, flow_gt, k=args.K)
                if args.descriptors:
                    ps, pt, fs, ft, _ = synthetic_descriptors(p, *ldmk)
                    if args.match_type == "sinkhorn":               # it has no temperature: the 1 / 0.1 goes into the descriptors' length
                        fs, ft = fs * 10 ** 0.5, ft * 10 ** 0.5
                    ldmk = descriptor_landmarks(dict(pts_s=ps, pts_t=pt, feat_s=fs, feat_t=ft), args.match_type)
                items.append((src, tgt, flow_gt, overlap, ldmk))
            if rank == 0 and args.descriptors:
                print(f"landmarks matched from descriptors ({args.match_type}): {sum(l[4][0].shape[0] for l in items) / max(len(items), 1):.1f} per pair")
        if args.outlier_weights:
            kept, items = outlier_rows(items, args.outlier_weights, args.outlier_thr)
            meters = {"outlier-kept_share": AverageMeter()}
            for share in kept:
                meters["outlier-kept_share"].update(share)
            keys, avgs = reduce_meters(meters, len(items), world, local_rank, backend)
            if rank == 0:
                print("learned outlier rejection of the landmarks, thr =", args.outlier_thr, "\n",
                      f"{n_total}/{n_total}: " + "".join(f"{k}: {avgs[k]:.3f}\t" for k in keys))
        rigid_flows = None
        if args.rigid_landmarks > 0:
            rigid_flows, inlier_ratios, items = rigid_rows(items, args.rigid_landmarks, args.rigid_landmarks_filter)
        if args.batched:
            timer.tic("registration")
            results = model.register_batch([(s, t, l) for s, t, _, _, l in items], slots=args.slots)
            torch.cuda.synchronize()
            timer.toc("registration")
            flows = [w.cpu() - s for (w, _), (s, _, _, _, _) in zip(results, items)]
        else:
            flows = []
            for src, tgt, _, _, ldmk in items:
                model.load_pcds(src, tgt, landmarks=ldmk)
                timer.tic("registration")
                warped, iter_cnt, timer = model.register(visualize=args.visualize, timer=timer)
                timer.toc("registration")
                flows.append((warped - model.src_pcd).cpu())
        meters = None
        for flow, (_, _, flow_gt, overlap, _) in zip(flows, items):
            info = compute_flow_metrics(flow, flow_gt, overlap=overlap)
            if meters is None:
                meters = {k: AverageMeter() for k in info}
            for k, v in info.items():
                meters[k].update(v)
        keys, avgs = reduce_meters(meters, len(items), world, local_rank, backend)
        if rank == 0:
            message = f"{n_total}/{n_total}: " + "".join(f"{k}: {avgs[k]:.3f}\t" for k in keys)
            Logger(os.path.join(config.snapshot_dir, benchmark + ".log")).write(message + "\n")
            print("score on ", benchmark, "\n", message)
        if rigid_flows is not None:
            meters = {}
            for flow, ratio, (_, _, flow_gt, overlap, _) in zip(rigid_flows, inlier_ratios, items):
                info = dict(compute_flow_metrics(flow, flow_gt, overlap=overlap), inlier_ratio=ratio)
                for k, v in info.items():
                    meters.setdefault("rigid-" + k, AverageMeter()).update(v)
            keys, avgs = reduce_meters(meters, len(items), world, local_rank, backend)
            if rank == 0:
                print("rigid motion through the landmarks, thr =", args.rigid_landmarks, "\n",
                      f"{n_total}/{n_total}: " + "".join(f"{k}: {avgs[k]:.3f}\t" for k in keys))
        if not have_data:
            break
    if rank == 0:
        print("time cost average")
        for line in timer.get_strings():
            print(line)
    if world > 1:
        import torch.distributed as dist
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
