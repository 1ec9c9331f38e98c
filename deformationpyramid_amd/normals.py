"""Normals for bare point clouds (4DMatch scans carry none): exact k nearest neighbours of the cloud against itself, then PCA of each
neighbourhood, both in libndp_hip.so (csrc/ndp_normals.inc).  What the reference's mesh driver gets from open3d for meshes
(shape_transfer.py:70,79); for a mesh see meshio.vertex_normals."""
import numpy as np
import torch

from . import ops


def estimate_normals(points, k=16, viewpoint=None, return_curvature=False):
    """points [n,3] (numpy array or tensor; moved to the current GPU if it is not on one) -> unit normals [n,3] on the device, with
    return_curvature (normals, curvature [n]).  A point's neighbourhood is its k nearest points, itself included (3 <= k <= 32,
    k <= n).  viewpoint (3 values): the normals face it; None: each normal's component of largest magnitude is positive.  Orientation
    is per point: there is no propagation along the surface."""
    p = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)) if isinstance(points, np.ndarray) else points
    if not p.is_cuda:
        p = p.cuda()
    p = p.detach().float().contiguous()
    _, idx = ops.knn(p, p, k)
    return ops.normals_from_knn(p, idx, viewpoint=viewpoint, want_curvature=return_curvature)
