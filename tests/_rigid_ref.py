"""Plain-torch restatements of what csrc/ndp_rigid.inc computes (DESIGN.md "Rigid alignment"), on the CPU in float64 -- the yardstick
of tests/test_rigid.py -- or in float32 -- the eager arithmetic the kernels' error is measured against.  Nothing here imports the
package.  The functions run on the device of their inputs (tools/rigid_bench.py times them on the GPU)."""
import math
from types import SimpleNamespace

import numpy as np
import torch

COND_MAX = 1e6                                                    # a triple whose D[0] / D[1] exceeds this is collinear
FLAG_INDEX, FLAG_EDGE, FLAG_DEGENERATE = 1, 2, 4


# ------------------------------------------------------------------------------------------ clouds
def lattice_cloud(n, seed):
    """Coordinates k / 64 with integer |k| <= 32: differences, squares and their sums are exact in float32, and ties are everywhere."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-32, 33, (n, 3), generator=g).float() / 64.0).contiguous()


def random_cloud(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, generator=g) - 0.5).contiguous()


def rotation(axis, angle):
    """Rodrigues: rotation by `angle` about `axis`, [3,3] float64."""
    a = torch.tensor(axis, dtype=torch.float64)
    a = a / a.norm()
    Kx = torch.tensor([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]], dtype=torch.float64)
    return torch.eye(3, dtype=torch.float64) + math.sin(angle) * Kx + (1 - math.cos(angle)) * (Kx @ Kx)


PLANTED_R = rotation((0.3, -0.5, 0.8), 1.1)
PLANTED_T = torch.tensor([0.2, -0.1, 0.05], dtype=torch.float64)


def planted(K, inlier_share, seed):
    """K correspondences of which the first int(K * inlier_share) in a seeded shuffle follow PLANTED_R, PLANTED_T up to per-axis noise
    uniform in +-0.004; the other targets are uniform in the cube.  -> (src [K,3], tgt [K,3] float32, inlier [K] bool)."""
    g = torch.Generator().manual_seed(seed)
    src = (torch.rand(K, 3, generator=g) - 0.5).float()
    n_in = int(K * inlier_share)
    noise = (torch.rand(K, 3, generator=g, dtype=torch.float64) - 0.5) * 0.008
    tgt = src.double() @ PLANTED_R.T + PLANTED_T + noise
    other = torch.rand(K, 3, generator=g, dtype=torch.float64) - 0.5
    inlier = torch.zeros(K, dtype=torch.bool)
    inlier[torch.randperm(K, generator=g)[:n_in]] = True
    tgt = torch.where(inlier[:, None], tgt, other).float()
    return src.contiguous(), tgt.contiguous(), inlier


def signed_permutations(H, seed):
    """H transforms [H,12] float32: R a signed axis permutation, t on the lattice k / 64."""
    g = torch.Generator().manual_seed(seed)
    T = torch.zeros(H, 12)
    for h in range(H):
        p = torch.randperm(3, generator=g)
        sg = torch.randint(0, 2, (3,), generator=g).float() * 2 - 1
        R = torch.zeros(3, 3)
        R[torch.arange(3), p] = sg
        T[h, :9] = R.reshape(9)
        T[h, 9:] = torch.randint(-16, 17, (3,), generator=g).float() / 64.0
    return T.contiguous()


# ------------------------------------------------------------------------------------------ Procrustes
def procrustes_ref(X, Y, w, eps=1e-4, dtype=torch.float64, three_points=False):
    """The reference's batch_weighted_procrustes (procrustes.py:18-44) as written: X, Y [B,N,3], w [B,N,1]; the sums in `dtype`, the
    3 x 3 SVD in double as there.  -> (R [B,3,3], t [B,3,1] in `dtype`, condition [B] float64 = D.max / D.min; three_points:
    D[0] / D[1], the ratio that is finite for a centred triple)."""
    X, Y, w = X.to(dtype), Y.to(dtype), w.to(dtype)
    W1 = torch.abs(w).sum(dim=1, keepdim=True)
    w_norm = w / (W1 + eps)
    mean_X = (w_norm * X).sum(dim=1, keepdim=True)
    mean_Y = (w_norm * Y).sum(dim=1, keepdim=True)
    Sxy = torch.matmul((Y - mean_Y).transpose(1, 2), w_norm * (X - mean_X)).cpu().double()        # (the SVD on the CPU, as there)
    U, D, Vh = torch.linalg.svd(Sxy)
    V = Vh.transpose(1, 2)
    condition = D[:, 0] / (D[:, 1] if three_points else D[:, 2])
    S = torch.eye(3, dtype=torch.float64)[None].repeat(X.shape[0], 1, 1)
    S[:, 2, 2] = torch.linalg.det(U) * torch.linalg.det(V)
    R = (U @ S @ V.transpose(1, 2)).to(dtype).to(X.device)
    t = mean_Y.transpose(1, 2) - R @ mean_X.transpose(1, 2)
    return R, t, condition.to(X.device)


def weights_of(n, w=None, mask=None):
    return (w if w is not None else mask.to(torch.float64) if mask is not None else torch.ones(n, dtype=torch.float64)).reshape(1, n, 1)


# ------------------------------------------------------------------------------------------ residuals
def residual2(T, src, tgt, dtype=torch.float64):
    """|R s + t - y|^2 of every (transform, correspondence): T [H,12], src, tgt [K,3] -> [H,K] in `dtype`.  (The kernel's chain is
    d_a = fmaf(R[a][0], sx, fmaf(R[a][1], sy, fmaf(R[a][2], sz, t[a]))) - y_a, d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)); on lattice
    inputs every product and sum is exact and the order does not matter.)"""
    T, s, y = T.to(dtype), src.to(dtype), tgt.to(dtype)
    R, t = T[:, :9].reshape(-1, 3, 3), T[:, 9:]
    d = torch.einsum("hab,kb->hka", R, s) + t[:, None, :] - y[None]
    return (d * d).sum(-1)


def score_ref(T, src, tgt, thr, dtype=torch.float64):
    """-> (count [H] int64, sse [H] in `dtype`): strict `<` against thr^2."""
    d2 = residual2(T, src, tgt, dtype)
    inl = d2 < torch.tensor(thr, dtype=dtype) ** 2
    return inl.sum(1), torch.where(inl, d2, torch.zeros_like(d2)).sum(1)


# ------------------------------------------------------------------------------------------ RANSAC
def hypotheses_ref(src, tgt, triples, edge_ratio=0.9, dtype=torch.float64):
    """The rejection rules and the three-point fits of every hypothesis: -> namespace(flags [H] int, T [H,12] (identity where refused),
    ratio [H,3] the min / max edge-length ratios, cond [H] D[0] / D[1]; NaN where the indices are refused)."""
    K, H = src.shape[0], triples.shape[0]
    tri = triples.long()
    bad = ((tri < 0) | (tri >= K)).any(1) | (tri[:, 0] == tri[:, 1]) | (tri[:, 0] == tri[:, 2]) | (tri[:, 1] == tri[:, 2])
    safe = torch.where(bad[:, None], torch.tensor([0, 1, 2], device=tri.device).expand(H, 3), tri)
    X, Y = src.to(dtype)[safe], tgt.to(dtype)[safe]                # [H,3,3]
    ratio = torch.empty(H, 3, dtype=dtype, device=src.device)
    for e, (a, b) in enumerate(((0, 1), (0, 2), (1, 2))):
        ls, ly = (X[:, a] - X[:, b]).norm(dim=1), (Y[:, a] - Y[:, b]).norm(dim=1)
        hi = torch.maximum(ls, ly)
        ratio[:, e] = torch.where(hi > 0, torch.minimum(ls, ly) / torch.where(hi > 0, hi, torch.ones_like(hi)), torch.ones_like(hi))
    R, t, cond = procrustes_ref(X, Y, torch.ones(H, 3, 1, dtype=dtype, device=src.device), 1e-4, dtype, three_points=True)
    flags = torch.zeros(H, dtype=torch.int64, device=src.device)
    edge = (ratio < edge_ratio).any(1) if edge_ratio > 0 else torch.zeros(H, dtype=torch.bool, device=src.device)
    flags[edge] = FLAG_EDGE
    flags[~edge & ~(cond <= COND_MAX)] = FLAG_DEGENERATE
    flags[bad] = FLAG_INDEX
    T = torch.cat([R.reshape(H, 9), t.reshape(H, 3)], dim=1)
    ident = torch.tensor([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0], dtype=dtype, device=src.device)
    T = torch.where((flags != 0)[:, None], ident, T)
    nan = torch.full_like(cond, float("nan"))
    return SimpleNamespace(flags=flags, T=T, ratio=torch.where(bad[:, None], nan[:, None].to(dtype), ratio), cond=torch.where(bad, nan, cond))


def refine_ref(T0, src, tgt, thr, refine_iters=2, dtype=torch.float64):
    """The refinement loop from the transform T0 [12]: mask under the current transform, Procrustes over the mask (eps 1e-4); fewer
    than 3 inliers keep the transform.  -> namespace(R, t, mask, count, rmse, masks = the mask of every pass)."""
    T = T0.to(dtype).reshape(1, 12)
    thr2 = torch.tensor(thr, dtype=dtype) ** 2
    masks = []
    left = refine_iters
    while True:
        d2 = residual2(T, src, tgt, dtype)[0]
        mask = d2 < thr2
        masks.append(mask)
        if left == 0 or int(mask.sum()) < 3:
            break
        left -= 1
        R, t, _ = procrustes_ref(src[None], tgt[None], weights_of(src.shape[0], mask=mask), 1e-4, dtype)
        T = torch.cat([R.reshape(1, 9), t.reshape(1, 3)], dim=1)
    n = int(mask.sum())
    rmse = float((d2[mask].sum() / n).sqrt()) if n else 0.0
    return SimpleNamespace(R=T[0, :9].reshape(3, 3), t=T[0, 9:], mask=mask, count=n, rmse=rmse, masks=masks, d2=d2)


def ransac_ref(src, tgt, triples, thr, edge_ratio=0.9, refine_iters=2, best=None, dtype=torch.float64):
    """The whole of ndp_ransac_rigid: rejection, three-point fits, scores of the accepted hypotheses, the best one (largest count, lowest
    index), refinement.  best: refine from this hypothesis instead of the restatement's own choice."""
    hyp = hypotheses_ref(src, tgt, triples, edge_ratio, dtype)
    ok = hyp.flags == 0
    count = torch.zeros(triples.shape[0], dtype=torch.int64, device=src.device)
    if ok.any():
        count[ok] = score_ref(hyp.T[ok], src, tgt, thr, dtype)[0]
    own = int(torch.argmax(count))                                # (argmax returns the first of equal maxima)
    out = SimpleNamespace(flags=hyp.flags, h_T=hyp.T, h_count=count, ratio=hyp.ratio, cond=hyp.cond, own_best=own, accepted=int(ok.sum()))
    b = own if best is None else int(best)
    if int(count[b]) == 0:
        out.status, out.best, out.count, out.rmse = 1, -1, 0, 0.0
        out.R, out.t, out.mask = torch.eye(3, dtype=dtype), torch.zeros(3, dtype=dtype), torch.zeros(src.shape[0], dtype=torch.bool, device=src.device)
        return out
    r = refine_ref(hyp.T[b], src, tgt, thr, refine_iters, dtype)
    out.status, out.best = 0, b
    out.R, out.t, out.mask, out.count, out.rmse, out.masks, out.d2 = r.R, r.t, r.mask, r.count, r.rmse, r.masks, r.d2
    return out


# ------------------------------------------------------------------------------------------ bars
def ulps16(scale):
    return 16.0 * float(np.spacing(np.float32(float(scale))))


def bar(ref64, ref32, scale):
    """The bound of a tensor: the larger of 4 x the eager float32 restatement's error and 16 float32 ulps of `scale`."""
    return max(4.0 * float((ref32.double() - ref64.double()).abs().max()), ulps16(scale))
