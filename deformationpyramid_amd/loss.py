"""Loss and metric surface of the reference's model/loss.py, backed by the HIP Chamfer kernels.

    compute_truncated_chamfer_distance(x, y, ..., trunc=0.2)   (/root/reference/model/loss.py:94-258)
    point_2_plane_distance(x, y, ..., x_normals, y_normals)    (loss.py:61-92)
    compute_flow_metrics(flow, flow_gt, overlap=None)          (loss.py:431-471)
    scene_flow_metrics(pred, labels, strict=0.025, relax=0.05) (loss.py:382-403)
    landmark_cost(x, y)                                        (loss.py:348-351)

The nearest-neighbour search and the L1 reduction run in libndp_hip.so (no pytorch3d, no torch
fallback for GPU tensors).  Pointclouds inputs are not part of any caller of the hot path and are
rejected; normals are taken by point_2_plane_distance only.
"""
import torch

from . import ops


def _lengths(points, lengths, name):
    if not torch.is_tensor(points):
        raise ValueError("The input pointclouds should be torch.Tensor of shape (minibatch, num_points, 3).")
    if points.ndim != 3:
        raise ValueError("Expected points to be of shape (N, P, D)")
    n, p = points.shape[0], points.shape[1]
    if lengths is None:
        return [p] * n
    if lengths.ndim != 1 or lengths.shape[0] != n:
        raise ValueError("Expected lengths to be of shape (N,)")
    return [int(v) for v in lengths.tolist()]


def compute_truncated_chamfer_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None,
                                       weights=None, trunc=0.2, batch_reduction="mean", point_reduction="mean"):
    """Bidirectional L1 Chamfer on exact 1-NN with truncation in SQUARED units.  Differentiable (first derivatives) in x -- the
    only use on the hot path: registration.py:195,212 -- and in y: whichever of the two requires a gradient receives one, from the
    one nearest-neighbour search."""
    if batch_reduction is not None and batch_reduction not in ["mean", "sum"]:
        raise ValueError('batch_reduction must be one of ["mean", "sum"] or None')
    if point_reduction not in ["mean", "sum"]:
        raise ValueError('point_reduction must be one of ["mean", "sum"]')
    if x_normals is not None or y_normals is not None:
        raise NotImplementedError("normals are not used by the NDP path and are not supported")
    xl = _lengths(x, x_lengths, "x")
    yl = _lengths(y, y_lengths, "y")
    N, _, D = x.shape
    if y.shape[0] != N or y.shape[2] != D:
        raise ValueError("y does not have the correct shape.")
    if D != 3:
        raise ValueError("only 3-D point clouds are supported")
    if weights is not None:
        if weights.size(0) != N:
            raise ValueError("weights must be of shape (N,).")
        if not (weights >= 0).all():
            raise ValueError("weights cannot be negative.")
        if weights.sum() == 0.0:
            z = (x.sum((1, 2)) * weights).sum() * 0.0
            return z if batch_reduction in ["mean", "sum"] else (x.sum((1, 2)) * weights) * 0.0
    per_batch = []
    for b in range(N):
        xb, yb = x[b, :xl[b]], y[b, :yl[b]]
        v = ops.chamfer_distance(xb, yb, trunc, point_sum=point_reduction == "sum")   # sum_x[/len_x] + sum_y[/len_y] (loss.py:233-235)
        if weights is not None:
            v = v * weights[b]
        per_batch.append(v)
    out = torch.stack(per_batch)
    if batch_reduction is None:
        return out
    out = out.sum()
    if batch_reduction == "mean":
        out = out / (weights.sum() if weights is not None else N)
    return out


def point_2_plane_distance(x, y, x_lengths=None, y_lengths=None, x_normals=None, y_normals=None, *, trunc=None, true_plane=False):
    """model/loss.py:61-92 on the HIP kernels: x [1,P1,3], y [1,P2,3] with their normals -> (p2plane, x_2_plane, y_2_plane,
    x_ref_normal [P1,3] = y_normals at every x point's nearest y point).  The defaults are the reference's arithmetic as written,
    sqrt(sum_a ((x_a - p_a) n_a)^2): the norm of the elementwise product, which is not a plane distance; true_plane=True gives
    |(x - p) . n|.  trunc (squared units, None: none) drops pairs as the Chamfer does.  p2plane is differentiable (first derivatives)
    in x and in y with the normals and the nearest-neighbour indices held constant; x_2_plane and y_2_plane are its two parts as
    values."""
    if x_normals is None or y_normals is None:
        raise ValueError("point_2_plane_distance needs x_normals and y_normals")
    xl = _lengths(x, x_lengths, "x")
    yl = _lengths(y, y_lengths, "y")
    assert x.shape[0] == 1                                            # as the reference (loss.py:76)
    if y.shape[0] != 1 or x.shape[2] != 3 or y.shape[2] != 3:
        raise ValueError("expected x [1, P1, 3] and y [1, P2, 3]")
    if x_normals.shape != x.shape or y_normals.shape != y.shape:
        raise ValueError("normals must have the shapes of their clouds")
    xb, yb = x[0, :xl[0]].float(), y[0, :yl[0]].float()
    nxb, nyb = x_normals[0, :xl[0]].float().contiguous(), y_normals[0, :yl[0]].float().contiguous()
    total, parts, idx_x = ops.point_to_plane_distance(xb, yb, nxb, nyb, float("inf") if trunc is None else trunc, 1 if true_plane else 0)
    return total, parts[0], parts[1], y_normals[0][idx_x.long()]


def landmark_cost(x, y):
    return torch.mean(torch.sum((x - y) ** 2, dim=-1))


def scene_flow_metrics(pred, labels, strict=0.025, relax=0.05):
    """EPE3D (x100 -> cm), AccS, AccR, Outlier (x100 -> %) on CPU, as upstream."""
    pred, labels = pred.detach().float().cpu(), labels.detach().float().cpu()
    err = torch.linalg.vector_norm(pred - labels, dim=1)
    rel = err / (torch.linalg.vector_norm(labels, dim=1) + 1e-20)
    epe = err.mean().item()
    acc_s = ((err < strict) | (rel < strict)).float().mean().item()
    acc_r = ((err < relax) | (rel < relax)).float().mean().item()
    outlier = (rel > 0.3).float().mean().item()
    return epe * 100, acc_s * 100, acc_r * 100, outlier * 100


def _metrics_on_device(flow, flow_gt, overlap):
    sums = ops.flow_metrics(flow.detach().float().contiguous(), flow_gt.detach().float().contiguous(), overlap)
    info = {}
    for tag, row in zip(("full", "vis", "occ") if overlap is not None else ("full",), sums):
        cnt = row[4].item()
        if cnt == 0:                                              # upstream: mean over an empty selection
            vals = [float("nan")] * 4
        else:
            vals = [float(torch.tensor(row[0].item() / cnt, dtype=torch.float32)) * 100] + [100.0 * row[k].item() / cnt for k in (1, 2, 3)]
        info.update({f"{tag}-epe": vals[0], f"{tag}-AccS": vals[1], f"{tag}-AccR": vals[2], f"{tag}-outlier": vals[3]})
    return info


def compute_flow_metrics(flow, flow_gt, overlap=None):
    """loss.py:431-471.  GPU tensors are reduced on the device (k_flow_metrics: one launch, 15 sums back); CPU tensors take
    the torch path upstream takes."""
    if torch.is_tensor(flow) and flow.is_cuda and flow.shape[0] > 0:
        return _metrics_on_device(flow, flow_gt.to(flow.device), overlap)
    info = {}
    subsets = [("full", None)]
    if overlap is not None:
        subsets += [("vis", overlap), ("occ", ~overlap)]
    for tag, mask in subsets:
        f, g = (flow, flow_gt) if mask is None else (flow[mask], flow_gt[mask])
        epe, acc_s, acc_r, outlier = scene_flow_metrics(f, g)
        info.update({f"{tag}-epe": epe, f"{tag}-AccS": acc_s, f"{tag}-AccR": acc_r, f"{tag}-outlier": outlier})
    return info
