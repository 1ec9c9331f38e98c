"""The input pyramid of KPConv-style backbones (KPFCN / Lepard) on the device: voxel-grid subsampling, fixed-radius neighbour tables,
the per-level lists a collate function hands to the network, the neighbourhood-size calibration, and the coarse labels of the
4DMatch collate.  The two operators are ops.voxel_subsample and ops.radius_search (csrc/ndp_kpconv.inc); this module is the
reference-shaped surface around them (correspondence/datasets/dataloader.py).  Everything takes and returns CUDA tensors; lengths
are small and live on the host."""
import math

import numpy as np
import torch

from . import ops


def grid_subsample(points, batches_len, features=None, labels=None, sampleDl=0.1, max_p=0, verbose=0, random_grid_orient=True):
    """batch_grid_subsampling_kpconv: (s_points, s_len) or (s_points, s_len, s_features).  Barycentres per voxel of edge sampleDl,
    in a defined order (per cloud ascending (iz, iy, ix); the reference's is its hash map's).  Class labels (majority vote per voxel)
    are not served; `verbose` and `random_grid_orient` are accepted and, as in the reference, do nothing."""
    if labels is not None:
        raise NotImplementedError("grid_subsample: class labels (majority vote per voxel) are not served")
    s_points, s_len, s_feat, _ = ops.voxel_subsample(points, batches_len, sampleDl, features=features, max_p=max_p)
    return (s_points, s_len) if features is None else (s_points, s_len, s_feat)


def radius_neighbors(queries, supports, q_batches, s_batches, radius, max_neighbors):
    """batch_neighbors_kpconv: int64 [Nq, K] stacked support indices, nearest first, padded with the shadow index len(supports).
    max_neighbors > 0: the `[:, :max_neighbors]` cut of the reference, except that a table whose fullest row is shorter is that
    narrow, as the reference's is; max_neighbors <= 0: every neighbour (at most 64 per query)."""
    if max_neighbors > 0:
        idx, counts = ops.radius_search(queries, supports, q_batches, s_batches, radius, min(int(max_neighbors), ops.RADIUS_MAX_K))
        fullest = int(counts.max().item())
        if int(max_neighbors) > ops.RADIUS_MAX_K and fullest > ops.RADIUS_MAX_K:
            raise ops.N.NdpError(f"radius_neighbors: a neighbourhood holds {fullest} supports; rows wider than "
                                 f"{ops.RADIUS_MAX_K} are not served (see radius_count)")
        return idx[:, :min(idx.shape[1], fullest)].long()
    idx, _ = ops.radius_search(queries, supports, q_batches, s_batches, radius, 0)
    return idx.long()


def radius_count(queries, supports, q_batches, s_batches, radius):
    """Number of supports within `radius` of every query [Nq] int32: the count pass alone, no limit on the neighbourhood size."""
    return ops.radius_search(queries, supports, q_batches, s_batches, radius, None)[1]


def _layers(architecture):
    """The reference's reading of the block names (dataloader.py:441-516): blocks up to the first `global` / `upsample`; a `pool` or
    `strided` block ends a layer; a layer's convolution radius widens if one of its blocks before the last is `deformable`, its
    pooling radius if the pooling block itself is.  -> [(has_conv, conv_deformable, pools, pool_deformable)]"""
    out, blocks = [], []
    for i, block in enumerate(architecture):
        if "global" in block or "upsample" in block:
            break
        pools = "pool" in block or "strided" in block
        if not pools:
            blocks.append(block)
            if i < len(architecture) - 1 and "upsample" not in architecture[i + 1]:
                continue
        out.append((bool(blocks), any("deformable" in b for b in blocks[:-1]), pools, "deformable" in block))
        blocks = []
    return out


def build_pyramid(points, lengths, first_subsampling_dl, conv_radius, deform_radius, architecture, neighborhood_limits):
    """The per-level inputs of the KPFCN collate for stacked clouds `points` [N,3] / `lengths` [B] -> dict of lists, one entry per
    layer: points [n_l,3] float32, neighbors / pools / upsamples int64 tables (empty [0,1] where the layer has none), stack_lengths
    int32 on the host.  Level l has conv radius r_l = first_subsampling_dl * conv_radius * 2^l (deformable: * deform_radius /
    conv_radius), is pooled onto a voxel grid of edge 2 r_l / conv_radius, and is upsampled from it with radius 2 r_l."""
    dev = points.device
    empty_i = lambda: torch.zeros((0, 1), dtype=torch.int64, device=dev)
    lengths = torch.as_tensor(lengths, dtype=torch.int32).cpu()
    r_normal = first_subsampling_dl * conv_radius
    out = {"points": [], "neighbors": [], "pools": [], "upsamples": [], "stack_lengths": []}
    for layer, (has_conv, conv_deform, pools, pool_deform) in enumerate(_layers(architecture)):
        limit = neighborhood_limits[layer]
        wide = r_normal * deform_radius / conv_radius
        conv_i = radius_neighbors(points, points, lengths, lengths, wide if conv_deform else r_normal, limit) if has_conv else empty_i()
        if pools:
            pool_p, pool_b = grid_subsample(points, lengths, sampleDl=2 * r_normal / conv_radius)
            pool_i = radius_neighbors(pool_p, points, pool_b, lengths, wide if pool_deform else r_normal, limit)
            up_i = radius_neighbors(points, pool_p, lengths, pool_b, 2 * r_normal, limit)
        else:
            pool_p, pool_b = torch.zeros((0, 3), device=dev), torch.zeros((0,), dtype=torch.int32)
            pool_i, up_i = empty_i(), empty_i()
        out["points"].append(points.float())
        out["neighbors"].append(conv_i)
        out["pools"].append(pool_i)
        out["upsamples"].append(up_i)
        out["stack_lengths"].append(lengths)
        points, lengths = pool_p, pool_b
        r_normal *= 2
    return out


def calibrate_neighbors(clouds, first_subsampling_dl, conv_radius, deform_radius, architecture, keep_ratio=0.8, samples_threshold=2000):
    """Per-layer neighbourhood limits (dataloader.py:609-637): the keep_ratio percentile of the conv neighbourhood sizes, gathered over
    `clouds` -- an iterable of (points [N,3], lengths) -- until every layer has more than samples_threshold samples.  The reference
    reads the sizes off index tables hist_n = ceil(4/3 pi (deform_radius + 1)^3) wide; here they are the search's `counts`, cut at
    hist_n the same way."""
    hist_n = int(math.ceil(4 / 3 * math.pi * (deform_radius + 1) ** 3))
    layers = _layers(architecture)
    hists = np.zeros((len(layers), hist_n), dtype=np.int64)
    for points, lengths in clouds:
        lengths = torch.as_tensor(lengths, dtype=torch.int32).cpu()
        r_normal = first_subsampling_dl * conv_radius
        for layer, (has_conv, conv_deform, pools, _) in enumerate(layers):
            if has_conv:
                c = radius_count(points, points, lengths, lengths, r_normal * deform_radius / conv_radius if conv_deform else r_normal)
                c = torch.clamp(c, max=hist_n).cpu().numpy()
                hists[layer] += np.bincount(c, minlength=hist_n)[:hist_n]
            if pools:
                points, lengths = grid_subsample(points, lengths, sampleDl=2 * r_normal / conv_radius)
            r_normal *= 2
        if hists.sum(axis=1).min() > samples_threshold:
            break
    cumsum = np.cumsum(hists.T, axis=0)
    return np.sum(cumsum < keep_ratio * cumsum[hist_n - 1, :], axis=0)


def blend_scene_flow(query, ref, ref_flow, knn=3):
    """Flow at `query` [m,3] blended from its `knn` nearest points of `ref` [n,3] with flows `ref_flow` [n,3] (datasets/utils.py:42-58):
    inverse-distance weights, distances floored at 1e-10.  The neighbours are ops.knn's."""
    d2, idx = ops.knn(query, ref, knn)
    w = 1.0 / torch.sqrt(d2).clamp_min(1e-10)
    w = w / w.sum(-1, keepdim=True)
    return (ref_flow[idx.long()] * w.unsqueeze(-1)).sum(1)


def mutual_nn_correspondence(src, tgt, search_radius=0.3):
    """[2, M] int64 (source index, target index) of the pairs that are each other's nearest neighbour and closer than search_radius
    (datasets/utils.py:61-79), ascending in the source index.  The neighbours are ops.chamfer_nn's."""
    d2x, ix, _, iy = ops.chamfer_nn(src, tgt)
    ix, iy = ix.long(), iy.long()
    src_idx = torch.arange(src.shape[0], device=src.device)
    keep = (iy[ix] == src_idx) & (torch.sqrt(d2x) < search_radius)
    return torch.stack([src_idx[keep], ix[keep]], 0)
