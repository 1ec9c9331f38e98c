"""Rigid alignment from correspondences on the HIP path (csrc/ndp_rigid.inc; DESIGN.md "Rigid alignment"): the reference's weighted
Procrustes (correspondence/lepard/procrustes.py:18-44) and its RANSAC pose helper (correspondence/lepard/loss.py:13-24) with their
signatures, the inlier ratio, and a landmark filter for the LNDP driver.

The hypotheses are drawn here, on the host, from a seeded generator; the kernels contain no random numbers.  Unlike open3d's
registration_ransac_based_on_correspondence there is no early termination at a confidence bound: all `max_iteration` hypotheses
are scored.  Parity with open3d is unverified (the library is not available to this repository)."""
import numpy as np
import torch

from . import ops


def draw_triples(K, H, seed):
    """H triples of indices into K correspondences -> [H,3] int32 (CPU); a list of K gives [B,H,3], problem b drawn in [0, K[b]).
    torch.randint on a CPU generator seeded with `seed`: the same arguments always give the same triples.  A triple may repeat an
    index; the kernel refuses such a hypothesis."""
    g = torch.Generator().manual_seed(int(seed))
    if isinstance(K, (list, tuple)):
        return torch.stack([torch.randint(0, int(k), (int(H), 3), generator=g, dtype=torch.int32) for k in K])
    return torch.randint(0, int(K), (int(H), 3), generator=g, dtype=torch.int32)


def weighted_procrustes(X, Y, w, eps=1e-4):
    """The reference's batch_weighted_procrustes: X, Y [B,N,3], w [B,N,1] -> (R [B,3,3], t [B,3,1], condition [B])."""
    B, n = X.shape[0], X.shape[1]
    R, t, cond, _ = ops.rigid_fit(X.reshape(B * n, 3).contiguous(), Y.reshape(B * n, 3).contiguous(), w=w.reshape(B * n).contiguous(), eps=eps,
                                  offsets=[b * n for b in range(B + 1)])
    return R, t[:, :, None], cond


def _device(*ts):
    for t in ts:
        if isinstance(t, torch.Tensor) and t.is_cuda:
            return t.device
    return torch.device("cuda", torch.cuda.current_device())


def _f32(a, dev):
    return torch.as_tensor(np.asarray(a) if not isinstance(a, torch.Tensor) else a).to(device=dev, dtype=torch.float32).contiguous()


def ransac_rigid(src, tgt, thr, max_iteration=50000, seed=0, edge_ratio=0.9, refine_iters=2):
    """RANSAC on one set of correspondences src [K,3] -> tgt [K,3] with `max_iteration` seeded hypotheses: ops.ransac_rigid's dict."""
    triples = draw_triples(src.shape[0], max_iteration, seed).to(src.device)
    return ops.ransac_rigid(src, tgt, triples, thr, edge_ratio=edge_ratio, refine_iters=refine_iters)


def ransac_pose_estimation(src_pcd, tgt_pcd, corrs=None, distance_threshold=0.05, ransac_n=3, max_iteration=50000, seed=0, src_feat=None,
                           tgt_feat=None):
    """The reference's helper (correspondence/lepard/loss.py:13): corrs = [s_ind, t_ind] pairs src_pcd[s_ind[i]] with tgt_pcd[t_ind[i]]
    -> the 4 x 4 pose (float64 numpy) that takes the source onto the target.  Edge-length check 0.9 and distance check at
    distance_threshold, as there; every one of the max_iteration hypotheses is scored (no confidence-bound early exit).
    corrs = None with src_feat [S,C] and tgt_feat [T,C]: the correspondences are the descriptors' mutual matches
    (matching.mutual_selection), the `mutual=True` branch of utils/benchmark_utils.py:251-274."""
    if ransac_n != 3:
        raise ValueError(f"ransac_n = {ransac_n}: only ransac_n = 3 is served (a hypothesis is a three-point fit)")
    if corrs is None and (src_feat is None or tgt_feat is None):
        raise ValueError("ransac_pose_estimation needs corrs, or src_feat and tgt_feat to match")
    dev = _device(src_pcd, tgt_pcd)
    if corrs is None:
        from . import matching
        corrs = matching.mutual_selection(_f32(src_feat, dev), _f32(tgt_feat, dev))
    s_ind, t_ind = (c.long().to(dev) if isinstance(c, torch.Tensor) else torch.as_tensor(np.asarray(c)).long().to(dev) for c in corrs[:2])
    src, tgt = _f32(src_pcd, dev)[s_ind].contiguous(), _f32(tgt_pcd, dev)[t_ind].contiguous()
    out = ransac_rigid(src, tgt, distance_threshold, max_iteration=max_iteration, seed=seed)
    pose = np.eye(4)
    pose[:3, :3] = out["R"][0].double().cpu().numpy()
    pose[:3, 3] = out["t"][0].double().cpu().numpy()
    return pose


def inlier_ratio(src, tgt, R, t, thr):
    """Share of correspondences with |R src + t - tgt| < thr (the reference's get_inlier_ratio) -> float."""
    T = torch.cat([R.reshape(9), t.reshape(3)]).to(device=src.device, dtype=torch.float32).reshape(1, 12).contiguous()
    count, _ = ops.rigid_score(T, src, tgt, thr)
    return float(count[0, 0].item()) / src.shape[0]


def reject_landmarks(ldmk_s, ldmk_t, thr, max_iteration=4096, seed=0, edge_ratio=0.9, refine_iters=2):
    """Landmarks that one rigid motion explains to within thr -> (mask [K] bool, R [3,3], t [3]) on the landmarks' device (moved to
    the GPU when they are not there).  All True with the identity when no hypothesis finds an inlier."""
    dev = _device(ldmk_s, ldmk_t)
    s, y = _f32(ldmk_s, dev), _f32(ldmk_t, dev)
    out = ransac_rigid(s, y, thr, max_iteration=max_iteration, seed=seed, edge_ratio=edge_ratio, refine_iters=refine_iters)
    mask = out["mask"].bool()
    if int(out["status"][0].item()) != 0:
        mask = torch.ones_like(mask)
    return mask, out["R"][0], out["t"][0]
