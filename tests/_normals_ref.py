"""Plain-torch restatements of what csrc/ndp_normals.inc computes (DESIGN.md "Surface normals"), on the CPU in float64 -- the yardstick
of tests/test_normals.py -- or in float32 -- the eager arithmetic the kernels' error is measured against.  Nothing here imports the
package."""
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn.functional as F


# ------------------------------------------------------------------------------------------ clouds
def lattice_cloud(n, seed):
    """Coordinates k / 64 with integer |k| <= 32: differences, squares and their sums are exact in float32, and ties are everywhere."""
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(-32, 33, (n, 3), generator=g).float() / 64.0).contiguous()


def random_cloud(n, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(n, 3, generator=g) - 0.5).contiguous()


def icosphere(subdiv=2, radius=1.0):
    """-> (verts [V,3] float64 on the sphere, faces [F,3] int64, outward winding)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, dtype=np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(subdiv):
        mid, nf = {}, []

        def m(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[key] = len(v) - 1
            return mid[key]

        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v) * radius, np.asarray(f, dtype=np.int64)


# ------------------------------------------------------------------------------------------ k nearest neighbours
def knn_ref(q, r, K):
    """Float64 brute force with a stable sort: -> (d2 [nq,K] float64, idx [nq,K] int64), rows ascending in (d2, index)."""
    q, r = q.double(), r.double()
    d2s, idxs = [], []
    for s in range(0, q.shape[0], 1024):
        d = ((q[s:s + 1024, None, :] - r[None, :, :]) ** 2).sum(-1)
        v, i = torch.sort(d, dim=1, stable=True)
        d2s.append(v[:, :K]); idxs.append(i[:, :K])
    return torch.cat(d2s), torch.cat(idxs)


def pair_d2(q, r, idx):
    """Float64 squared distance of every listed (query, reference) pair: [nq, K]."""
    return ((q.double()[:, None, :] - r.double()[idx.long()]) ** 2).sum(-1)


# ------------------------------------------------------------------------------------------ PCA normals
def pca_ref(p, idx, dtype=torch.float64):
    """-> namespace(normal [n,3], curvature [n], gap [n] = (l1 - l0) / l2, cov [n,3,3]) of the neighbourhoods idx [n,K] of p, in
    `dtype`: mean, covariance of the differences, eigh.  The normal's sign is eigh's (compare up to sign)."""
    nb = p.to(dtype)[idx.long()]
    d = nb - nb.mean(dim=1, keepdim=True)
    cov = d.transpose(1, 2) @ d / idx.shape[1]
    w, v = torch.linalg.eigh(cov)
    tot = w.sum(dim=1)
    curv = torch.where(tot > 0, w[:, 0].clamp_min(0) / torch.where(tot > 0, tot, torch.ones_like(tot)), torch.zeros_like(tot))
    gap = (w[:, 1] - w[:, 0]) / torch.where(w[:, 2] > 0, w[:, 2], torch.ones_like(tot))
    return SimpleNamespace(normal=v[:, :, 0], curvature=curv, gap=gap, cov=cov)


def sin_angle(a, b):
    """sin of the angle between unit vectors, sign-blind: |a x b|."""
    return torch.linalg.cross(a.double(), b.double(), dim=1).norm(dim=1)


# ------------------------------------------------------------------------------------------ point to plane
def _direction(a, b, n_a, n_b, d2, idx, trunc, mode):
    """Direction a -> b: value, consistency figure, d value / da [na,3], d value / db [nb,3] (indices and normals constant)."""
    idx = idx.long()
    diff, n = a - b[idx], n_b[idx]
    keep = (d2 < trunc)[:, None]
    if mode == 0:
        e = diff * n
        r = e.pow(2).sum(1).sqrt()
        g = e * n / r[:, None]
    else:
        dot = (diff * n).sum(1)
        r = dot.abs()
        g = torch.sign(dot)[:, None] * n
    zero = torch.zeros_like(g)
    val = torch.where(keep[:, 0], r, zero[:, 0]).sum() / a.shape[0]
    ga = torch.where(keep, g, zero) / a.shape[0]
    gb = torch.zeros_like(b).index_add_(0, idx, -ga)
    cons = (1 - F.cosine_similarity(n_a, n, dim=1, eps=1e-6).abs()).mean()
    return val, cons, ga, gb


def point_to_plane_ref(x, y, nx, ny, nn, trunc=float("inf"), mode=0, dtype=torch.float64):
    """-> namespace(out [4], gx [S,3], gy [T,3]) in `dtype` from explicit formulas.  nn = (d2x, idx_x, d2y, idx_y): the truncation
    compares the GIVEN float32 distances with float32(trunc), as the kernel does; nothing else of d2 is used."""
    d2x, ix, d2y, iy = nn
    tr = torch.tensor(trunc, dtype=torch.float32)
    x, y, nx, ny = (t.to(dtype) for t in (x, y, nx, ny))
    vx, cx, gxx, gyx = _direction(x, y, nx, ny, d2x.float(), ix, tr, mode)
    vy, cy, gyy, gxy = _direction(y, x, ny, nx, d2y.float(), iy, tr, mode)
    return SimpleNamespace(out=torch.stack([vx + vy, vx, vy, cx + cy]), gx=gxx + gxy, gy=gyy + gyx)


def point_to_plane_autograd(x, y, nx, ny, nn, trunc=float("inf"), mode=0, dtype=torch.float64):
    """The same value written as the reference writes it (loss.py:81-90, plus the truncation mask), differentiated by autograd."""
    d2x, ix, d2y, iy = nn
    tr = torch.tensor(trunc, dtype=torch.float32)
    x, y = x.to(dtype).clone().requires_grad_(True), y.to(dtype).clone().requires_grad_(True)
    nx, ny = nx.to(dtype), ny.to(dtype)

    def side(a, b, n_b, d2, idx):
        prod = (a - b[idx.long()]) * n_b[idx.long()]
        r = prod.pow(2).sum(1).sqrt() if mode == 0 else prod.sum(1).abs()
        return r[d2.float() < tr].sum() / a.shape[0]

    total = side(x, y, ny, d2x, ix) + side(y, x, nx, d2y, iy)
    gx, gy = torch.autograd.grad(total, [x, y])
    return SimpleNamespace(total=total.detach(), gx=gx, gy=gy)


def nn_ref(x, y):
    """Float64 1-NN in both directions in the layout of ops.chamfer_nn: (d2x float32, idx_x int32, d2y float32, idx_y int32)."""
    dx, ix = knn_ref(x, y, 1)
    dy, iy = knn_ref(y, x, 1)
    return dx[:, 0].float(), ix[:, 0].int(), dy[:, 0].float(), iy[:, 0].int()


def ulps16(t):
    return 16.0 * float(np.spacing(np.float32(float(t.abs().max()))))


def bar(ref64, ref32):
    """The bound of a tensor: the larger of 4 x the eager float32 restatement's error and 16 float32 ulps of its largest magnitude."""
    return max(4.0 * float((ref32.double() - ref64).abs().max()), ulps16(ref64))
