"""Descriptor matching on the HIP path (csrc/ndp_match.inc; DESIGN.md "Descriptor matching"): from per-point descriptors to
correspondences.  The reference's coarse matcher (correspondence/lepard/matching.py:118-173: dual-softmax or Sinkhorn with a
dustbin, then the mutual-maximum test of `get_match`) and its feature-matching helpers (utils/benchmark_utils.py:251-359:
`mutual_selection`, `get_inlier_ratio`), without their S x T matrices: the kernels keep row and column statistics only.

The inputs are the feature matrices the reference hands to its matcher AFTER `src_proj` and the positional embedding; the learned
layers in front of them (the repositioning transformer, `src_proj`, the rotary embedding) are deformationpyramid_amd/lepard.py, whose
`Matching` also returns the dense confidence matrix (ops.feat_conf).  Scores follow the reference: <fs_i, ft_j> / C (its `feat / C ** .5` on both sides), so
unit-norm descriptors (FCGF, Predator, FPFH after normalisation) want a factor sqrt(C) first to make `temperature` act on cosines.

Ties: where the reference's `conf == conf.max()` test accepts every column that attains a row's maximum, the kernels take the lowest
index.  Sinkhorn is defined on the unpadded problems (the reference's padded rows leak mass into the dustbin).
Parity with a trained Lepard checkpoint is unverified: no weights are available to this repository."""
import math

import torch

from . import ops


def _rows(feats, mask, name):
    """feats [B,N,C] or [N,C], mask [B,N] bool prefix mask or None -> (the valid rows concatenated [sum N_b, C], [N_b])."""
    if not isinstance(feats, torch.Tensor) or feats.ndim not in (2, 3):
        raise ValueError(f"{name}_feats must be a tensor [B, N, C] or [N, C], got {getattr(feats, 'shape', type(feats))}")
    if feats.ndim == 2:
        feats = feats[None]
    B, n = feats.shape[0], feats.shape[1]
    if mask is None:
        return feats.reshape(B * n, feats.shape[2]).float().contiguous(), [n] * B
    mask = torch.as_tensor(mask)
    if mask.ndim == 1:
        mask = mask[None]
    if tuple(mask.shape) != (B, n):
        raise ValueError(f"{name}_mask must be [{B}, {n}], got {tuple(mask.shape)}")
    mask = mask.bool()
    lens = mask.sum(1)
    if not torch.equal(mask, torch.arange(n, device=mask.device)[None, :] < lens[:, None]):
        raise ValueError(f"{name}_mask must be a prefix mask (the valid rows first, as a padded batch has them)")
    lens = [int(v) for v in lens.tolist()]
    return torch.cat([feats[b, :k] for b, k in enumerate(lens)]).float().contiguous(), lens


def _offsets(lens):
    off = [0]
    for k in lens:
        off.append(off[-1] + k)
    return off


def _match(src_feats, tgt_feats, src_mask, tgt_mask, **kw):
    fs, ls = _rows(src_feats, src_mask, "src")
    ft, lt = _rows(tgt_feats, tgt_mask, "tgt")
    if len(ls) != len(lt):
        raise ValueError(f"src_feats and tgt_feats must hold the same number of problems, got {len(ls)} and {len(lt)}")
    if fs.shape[1] != ft.shape[1]:
        raise ValueError(f"both sides need the same descriptor length C, got {fs.shape[1]} and {ft.shape[1]}")
    off_s = _offsets(ls)
    match_t, conf = ops.feat_match(fs, ft, offsets_s=off_s, offsets_t=_offsets(lt), **kw)
    rows = (match_t >= 0).nonzero()[:, 0]                        # the one compaction, as the reference's `mask.nonzero()`
    bounds = torch.tensor(off_s, device=rows.device)
    b = torch.bucketize(rows, bounds[1:], right=True)
    index = torch.stack([b, rows - bounds[b], match_t[rows].long()], 1)
    return index, conf[rows]


def dual_softmax_match(src_feats, tgt_feats, temperature=0.1, confidence_threshold=0.1, src_mask=None, tgt_mask=None, mutual=True):
    """The reference's dual-softmax branch followed by `Matching.get_match` (matching.py:144-157, 73-88): conf_ij = softmax over i
    times softmax over j of <fs_i, ft_j> / (C temperature) -> (index [M,3] int64 rows (b, s, t) in ascending (b, s), mconf [M])."""
    return _match(src_feats, tgt_feats, src_mask, tgt_mask, mode="dual_softmax", temperature=temperature, thr=confidence_threshold,
                  mutual=mutual)


def sinkhorn_match(src_feats, tgt_feats, bin_score=1.0, iters=3, confidence_threshold=0.1, src_mask=None, tgt_mask=None, mutual=True):
    """The reference's `log_optimal_transport` branch (matching.py:6-38, 159-170) on each unpadded problem -> as dual_softmax_match."""
    return _match(src_feats, tgt_feats, src_mask, tgt_mask, mode="sinkhorn", bin_score=bin_score, iters=iters, thr=confidence_threshold,
                  mutual=mutual)


def mutual_selection(src_feat, tgt_feat):
    """Pairs (i, j) whose score <src_i, tgt_j> is the maximum of both its row and its column (benchmark_utils.mutual_selection on
    the score matrix, `np.where` of its result) -> (row_sel [M], col_sel [M]) int64, ascending rows."""
    index, _ = _match(src_feat, tgt_feat, None, None, mode="mutual_nn", temperature=1.0, thr=-math.inf, mutual=True)
    return index[:, 1], index[:, 2]


def inlier_ratio_of_features(src_pcd, tgt_pcd, src_feat, tgt_feat, rot, trans, thr=0.1):
    """The two ratios of the reference's get_inlier_ratio: the share of feature matches that (rot, trans) brings within thr, with
    every source point matched to its best target ("wo") and with the mutual matches only ("w") -> (ratio_wo, ratio_w) floats;
    ratio_w is nan without a mutual match, as the reference's mean of nothing."""
    from . import rigid
    dev = rigid._device(src_feat, tgt_feat, src_pcd, tgt_pcd)
    ps, pt = rigid._f32(src_pcd, dev), rigid._f32(tgt_pcd, dev)
    fs, ft = rigid._f32(src_feat, dev), rigid._f32(tgt_feat, dev)
    R, t = rigid._f32(rot, dev).reshape(3, 3), rigid._f32(trans, dev).reshape(3)
    best, _ = ops.feat_match(fs, ft, mode="mutual_nn", temperature=1.0, thr=-math.inf, mutual=False)
    wo = rigid.inlier_ratio(ps, pt[best.long()].contiguous(), R, t, thr)
    rows, cols = mutual_selection(fs, ft)
    w = rigid.inlier_ratio(ps[rows].contiguous(), pt[cols].contiguous(), R, t, thr) if rows.numel() else math.nan
    return wo, w


def landmarks_from_descriptors(pts_s, pts_t, feat_s, feat_t, match_type="dual_softmax", temperature=0.1, confidence_threshold=0.1,
                               bin_score=1.0, iters=3, mutual=True, want_conf=False):
    """Points pts_s [S,3], pts_t [T,3] with descriptors feat_s [S,C], feat_t [T,C] -> (ldmk_s [K,3], ldmk_t [K,3]) of the matched
    pairs, in ascending source order: what Registration.load_pcds(..., landmarks=) and rigid.reject_landmarks take.  want_conf adds
    the matches' confidences [K]."""
    from . import rigid
    dev = rigid._device(feat_s, feat_t, pts_s, pts_t)
    ps, pt, fs, ft = (rigid._f32(a, dev) for a in (pts_s, pts_t, feat_s, feat_t))
    if ps.shape[0] != fs.shape[0] or pt.shape[0] != ft.shape[0]:
        raise ValueError(f"one descriptor per point: {tuple(ps.shape)} / {tuple(fs.shape)} and {tuple(pt.shape)} / {tuple(ft.shape)}")
    if match_type == "dual_softmax":
        index, conf = dual_softmax_match(fs, ft, temperature, confidence_threshold, mutual=mutual)
    elif match_type == "sinkhorn":
        index, conf = sinkhorn_match(fs, ft, bin_score, iters, confidence_threshold, mutual=mutual)
    elif match_type == "mutual_nn":
        index, conf = _match(fs, ft, None, None, mode="mutual_nn", temperature=1.0, thr=-math.inf, mutual=mutual)
    else:
        raise ValueError(f"match_type must be dual_softmax, sinkhorn or mutual_nn, got {match_type!r}")
    out = (ps[index[:, 1]].contiguous(), pt[index[:, 2]].contiguous())
    return out + (conf,) if want_conf else out
