"""numpy restatements of the KPConv input operators (csrc/ndp_kpconv.inc, deformationpyramid_amd/kpconv.py): the yardstick of
tests/test_kpconv.py.  Voxel membership is the fp32 expression of the reference (origin = floor(min * (1 / dl)) * dl,
i = floor((p - origin) / dl), numpy float32 is IEEE single); barycentres are float64 sums in ascending input index (dtype=float32:
the reference's own fp32 accumulation, the eager error of the bar); output order per cloud is ascending (iz, iy, ix).  Radius rows
are brute force over the cloud, d2 < r2 strictly with r2 = fl32(radius * radius), sorted by (d2, index) and padded with the shadow
index.  Nothing here imports the package."""
import math
from types import SimpleNamespace

import numpy as np

ULP = 2.0 ** -23                                                  # float32 spacing at 1
F32, F64 = np.float32, np.float64
KPFCN = ["simple", "resnetb", "resnetb_strided", "resnetb", "resnetb", "resnetb_strided", "resnetb", "resnetb", "resnetb_strided",
         "resnetb", "resnetb", "nearest_upsample", "unary", "nearest_upsample", "unary", "nearest_upsample", "unary"]
LEPARD = dict(first_subsampling_dl=0.01, conv_radius=2.5, deform_radius=5.0)       # configs/lepard.yaml


def bar(err32, magnitude):
    """The project's bar: the larger of 4 x the eager float32 restatement's error and 16 float32 ulps of the largest magnitude."""
    return max(4.0 * float(err32), 16.0 * ULP * float(magnitude))


def offsets(lengths):
    return np.concatenate([[0], np.cumsum(np.asarray(lengths, np.int64))])


# ------------------------------------------------------------------------------------------ generators
def lattice_cloud(n, seed, lo=-64, hi=64, step=1.0 / 64):
    """n points whose coordinates are integer multiples of `step` in [lo, hi) * step: differences, squares and their sums are exact."""
    g = np.random.default_rng(seed)
    return (g.integers(lo, hi, size=(n, 3)) * step).astype(F32)


def surface_cloud(n, seed, density=10000.0, shift=(0.0, 0.0, 0.0)):
    """n points of a gently curved, slightly noisy height field whose side grows with n so that the density per unit area stays put
    (about one point per 0.01-voxel: what the first subsampling of a scan leaves)."""
    g = np.random.default_rng(seed)
    side = math.sqrt(n / density)
    xy = g.random((n, 2)) * side
    z = 0.05 * np.sin(8 * xy[:, 0]) * np.cos(6 * xy[:, 1]) + 0.002 * g.standard_normal(n)
    return (np.concatenate([xy, z[:, None]], 1) + np.asarray(shift)).astype(F32)


# ------------------------------------------------------------------------------------------ voxel subsampling
def voxel_cells(p, dl):
    """One cloud: int64 [n,3] voxel indices (ix, iy, iz) and the float64 quotients they are the floors of."""
    p, dl = np.asarray(p, F32), F32(dl)
    origin = np.floor(p.min(0) * (F32(1) / dl)) * dl
    assert origin.dtype == F32
    quo = (p - origin) / dl
    assert quo.dtype == F32
    return np.floor(quo).astype(np.int64), (p.astype(F64) - origin.astype(F64)) / F64(dl)


def voxel_subsample(points, lengths, dl, features=None, max_p=0, dtype=F64):
    points = np.asarray(points, F32)
    n_all = points.shape[0]
    out_p, out_f, out_len, keys = [], [], [], []
    inverse = np.full(n_all, -1, np.int64)
    base = obase = 0
    for n in [int(v) for v in lengths]:
        p = points[base:base + n]
        c, _ = voxel_cells(p, dl)
        order = np.lexsort((c[:, 0], c[:, 1], c[:, 2]))
        cs = c[order]
        head = np.ones(n, bool)
        head[1:] = (cs[1:] != cs[:-1]).any(1)
        vid = np.empty(n, np.int64)
        vid[order] = np.cumsum(head) - 1
        nv = int(head.sum())
        keep = nv if max_p <= 0 else min(nv, int(max_p))
        cnt = np.bincount(vid, minlength=nv).astype(dtype)
        acc = np.zeros((nv, 3), dtype)
        np.add.at(acc, vid, p.astype(dtype))                      # unbuffered: ascending input index
        out_p.append((acc / cnt[:, None])[:keep])
        if features is not None:
            f = np.asarray(features, F32)[base:base + n]
            accf = np.zeros((nv, f.shape[1]), dtype)
            np.add.at(accf, vid, f.astype(dtype))
            out_f.append((accf / cnt[:, None])[:keep])
        inverse[base:base + n] = np.where(vid < keep, vid + obase, -1)
        keys.append(cs[head][:keep][:, ::-1])                     # (iz, iy, ix) per kept voxel
        out_len.append(keep)
        base += n
        obase += keep
    return SimpleNamespace(points=np.concatenate(out_p), lengths=np.asarray(out_len, np.int32), inverse=inverse,
                           features=np.concatenate(out_f) if features is not None else None, keys=keys)


def face_clearance(points, lengths, dl):
    """Smallest distance of a voxel quotient (p - origin) / dl to an integer, in float32 ulps of that quotient."""
    worst, base = math.inf, 0
    for n in [int(v) for v in lengths]:
        _, u = voxel_cells(np.asarray(points, F32)[base:base + n], dl)
        gap = np.abs(u - np.round(u)) / np.spacing(np.maximum(np.abs(u), 1.0).astype(F32)).astype(F64)
        worst = min(worst, float(gap.min()))
        base += n
    return worst


# ------------------------------------------------------------------------------------------ radius search
def _r32(x):
    return x.astype(F32).astype(F64)


def cloud_d2(q, s):
    """(float32 d2 of the kernels' chain fmaf(dz, dz, fmaf(dy, dy, dx * dx)) with d = q - s, emulated through float64 -- exact
    whenever the products are, as on lattice clouds --, float64 d2 of the same float32 inputs)."""
    d64 = np.asarray(q, F32).astype(F64)[:, None, :] - np.asarray(s, F32).astype(F64)[None, :, :]
    d = _r32(d64)
    t = _r32(d[..., 0] * d[..., 0])
    t = _r32(d[..., 1] * d[..., 1] + t)
    return (d[..., 2] * d[..., 2] + t).astype(F32), (d64 * d64).sum(-1)


def radius_search(q, s, q_lengths, s_lengths, radius, K=None):
    """-> idx [nq, K] int64 (stacked-global, (d2, index) order, shadow-padded), counts [nq], d2 [nq, K] float32 (+inf padded),
    clearance: the smallest |d2_64 - r2| over all pairs of a cloud in float32 ulps of r2.  K None: the largest count."""
    r2 = F32(radius) * F32(radius)
    qo, so = offsets(q_lengths), offsets(s_lengths)
    shadow = int(so[-1])
    rows, dists, clearance = [], [], math.inf
    for b in range(len(qo) - 1):
        d2, d64 = cloud_d2(np.asarray(q)[qo[b]:qo[b + 1]], np.asarray(s)[so[b]:so[b + 1]])
        clearance = min(clearance, float(np.abs(d64 - F64(r2)).min() / np.spacing(r2)))
        for i in range(d2.shape[0]):
            js = np.nonzero(d2[i] < r2)[0]
            js = js[np.lexsort((js, d2[i, js]))]
            rows.append(js + so[b])
            dists.append(d2[i, js])
    counts = np.asarray([len(r) for r in rows], np.int64)
    K = int(counts.max()) if K is None else int(K)
    idx = np.full((len(rows), K), shadow, np.int64)
    dd = np.full((len(rows), K), np.inf, F32)
    for i, (r, d) in enumerate(zip(rows, dists)):
        idx[i, :min(K, len(r))] = r[:K]
        dd[i, :min(K, len(r))] = d[:K]
    return SimpleNamespace(idx=idx, counts=counts, d2=dd, clearance=clearance, r2=r2)


def neighbors(q, s, ql, sl, radius, limit):
    """The reference's wrapper: width min(largest count, limit) for limit > 0."""
    r = radius_search(q, s, ql, sl, radius)
    return (r.idx[:, :limit] if limit > 0 else r.idx), r


# ------------------------------------------------------------------------------------------ pyramid
def layers(architecture):
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


def build_pyramid(points, lengths, first_subsampling_dl, conv_radius, deform_radius, architecture, limits):
    """The collate's lists; points64 holds the unrounded float64 barycentres of each level (level 0: the input), and clearance the
    smallest face / r2 clearance met on the way, in float32 ulps."""
    points, lengths = np.asarray(points, F32), np.asarray(lengths, np.int32)
    out = SimpleNamespace(points=[], points64=[], points32=[], neighbors=[], pools=[], upsamples=[], stack_lengths=[], counts=[],
                          clearance=math.inf)
    p64 = points.astype(F64)
    p32 = points
    r_normal = first_subsampling_dl * conv_radius
    empty = np.zeros((0, 1), np.int64)
    for layer, (has_conv, conv_deform, pools, pool_deform) in enumerate(layers(architecture)):
        wide = r_normal * deform_radius / conv_radius
        conv_i, pool_i, up_i, cnt = empty, empty, empty, None
        if has_conv:
            conv_i, r = neighbors(points, points, lengths, lengths, wide if conv_deform else r_normal, limits[layer])
            out.clearance, cnt = min(out.clearance, r.clearance), r.counts
        if pools:
            dl = 2 * r_normal / conv_radius
            out.clearance = min(out.clearance, face_clearance(points, lengths, dl))
            sub = voxel_subsample(points, lengths, dl)
            sub32 = voxel_subsample(points, lengths, dl, dtype=F32)
            pool_p = sub.points.astype(F32)
            pool_i, r1 = neighbors(pool_p, points, sub.lengths, lengths, wide if pool_deform else r_normal, limits[layer])
            up_i, r2 = neighbors(points, pool_p, lengths, sub.lengths, 2 * r_normal, limits[layer])
            out.clearance = min(out.clearance, r1.clearance, r2.clearance)
        out.points.append(points); out.points64.append(p64); out.points32.append(p32)
        out.neighbors.append(conv_i); out.pools.append(pool_i); out.upsamples.append(up_i)
        out.stack_lengths.append(lengths); out.counts.append(cnt)
        if not pools:
            break
        points, lengths, p64, p32 = pool_p, sub.lengths, sub.points, sub32.points
        r_normal *= 2
    return out


def calibrate_neighbors(clouds, first_subsampling_dl, conv_radius, deform_radius, architecture, keep_ratio=0.8, samples_threshold=2000):
    hist_n = int(math.ceil(4 / 3 * math.pi * (deform_radius + 1) ** 3))
    n_layers = len(layers(architecture))
    hists = np.zeros((n_layers, hist_n), np.int64)
    for points, lengths in clouds:
        pyr = build_pyramid(points, lengths, first_subsampling_dl, conv_radius, deform_radius, architecture, [0] * n_layers)
        for layer, c in enumerate(pyr.counts):
            hists[layer] += np.bincount(np.minimum(c, hist_n), minlength=hist_n)[:hist_n]
        if hists.sum(axis=1).min() > samples_threshold:
            break
    cumsum = np.cumsum(hists.T, axis=0)
    return np.sum(cumsum < keep_ratio * cumsum[hist_n - 1, :], axis=0)


def pyramid_input(seed0=0, sizes=(1700, 1300), need=16.0):
    """The (1700, 1300) surface pair of the pyramid test: reseeded until no level has a point within `need` ulps of a voxel face or a
    pair within `need` ulps of r2.  -> (points, lengths, restated pyramid, seed)"""
    limits = PYRAMID_LIMITS
    for seed in range(seed0, seed0 + 64):
        pts = np.concatenate([surface_cloud(n, 1000 * seed + k, shift=(0.3 * k, -0.2 * k, 0.1 * k)) for k, n in enumerate(sizes)])
        pyr = build_pyramid(pts, sizes, architecture=KPFCN, limits=limits, **LEPARD)
        if pyr.clearance > need:
            return pts, np.asarray(sizes, np.int32), pyr, seed
    raise AssertionError("no seed gave the clearance")


PYRAMID_LIMITS = [24, 28, 32, 36]


# ------------------------------------------------------------------------------------------ coarse labels
def blend_scene_flow(query, ref, ref_flow, knn=3, dtype=F64):
    q, r = np.asarray(query, F32).astype(dtype), np.asarray(ref, F32).astype(dtype)
    d2 = ((q[:, None, :] - r[None, :, :]) ** 2).sum(-1)
    idx = np.argsort(d2, axis=1, kind="stable")[:, :knn]
    d = np.sqrt(np.take_along_axis(d2, idx, 1))
    d[d < 1e-10] = 1e-10
    w = 1.0 / d
    w = w / w.sum(-1, keepdims=True)
    return (np.asarray(ref_flow, F32).astype(dtype)[idx] * w[..., None]).sum(1), np.sort(d2, axis=1)[:, :knn + 1]


def mutual_nn_correspondence(src, tgt, search_radius):
    d2 = cloud_d2(src, tgt)[1]
    s2t, t2s = d2.argmin(1), d2.argmin(0)
    i = np.arange(d2.shape[0])
    keep = (t2s[s2t] == i) & (np.sqrt(d2[i, s2t]) < search_radius)
    return np.stack([i[keep], s2t[keep]], 0)


# ------------------------------------------------------------------------------------------ the cases of tests/test_kpconv.py
def _case(q, s, ql, sl, radius, lattice=False):
    return SimpleNamespace(q=np.ascontiguousarray(q, F32), s=np.ascontiguousarray(s, F32), ql=list(ql), sl=list(sl), radius=radius,
                           lattice=lattice)


def _lattice_case():
    """Coordinates are multiples of 1/64 in [-0.5, 0.5), radius 0.25: every d2 is an exact multiple of 2^-12, r2 = 2^-4 is hit
    exactly (planted pairs 16/64 apart along an axis, and more by chance), supports are duplicated, queries include supports."""
    s = lattice_cloud(380, 7, -32, 32)
    s = np.concatenate([s, s[:20], s[5:6] + np.asarray([[0.25, 0, 0]], F32), s[9:10] + np.asarray([[0, -0.25, 0]], F32)])
    q = np.concatenate([lattice_cloud(65, 8, -40, 40), s[:40]])
    return _case(q, s, [len(q)], [len(s)], 0.25, lattice=True)


def _random_case(nq, ns, seed, radius=0.03, extra_q=None):
    def make(sd):
        s = surface_cloud(ns, 31 * sd + 1)
        q = surface_cloud(nq, 31 * sd + 2, density=10000.0 * nq / ns)      # the same patch
        if extra_q is not None:
            q = np.concatenate([q, extra_q(s)]).astype(F32)
        return _case(q, s, [len(q)], [len(s)], radius)
    return _cleared(make, seed)


def _cleared(make, seed, need=16.0):
    for sd in range(seed, seed + 64):
        c = make(sd)
        if radius_search(c.q, c.s, c.ql, c.sl, c.radius).clearance > need:
            return c
    raise AssertionError("no seed gave the clearance")


def _outside(s):
    """queries outside the supports' box by less and by more than the radius (0.03), on every side, and one very far away"""
    lo, hi = s.min(0), s.max(0)
    mid = (lo + hi) / 2
    out = []
    for a in range(3):
        for d in (0.01, 0.02, 0.05, 0.5):
            for end, sign in ((lo, -1), (hi, 1)):
                p = mid.copy()
                p[a] = end[a] + sign * d
                out.append(p)
    out.append(mid + 1e6)
    out.append(lo - 0.01)
    return np.asarray(out, F32)


def _batch_case(sd):
    sizes_s, sizes_q = [300, 1, 64, 129], [65, 3, 1, 200]
    s = [surface_cloud(n, 100 * sd + k, density=10000.0 * n / 300) for k, n in enumerate(sizes_s)]    # all on the patch of 300 points: the clouds overlap
    q = [surface_cloud(n, 100 * sd + 50 + k, density=10000.0 * n / 300) for k, n in enumerate(sizes_q)]
    q[1][0] = s[1][0]                                             # the 1-point cloud is asked about itself
    return _case(np.concatenate(q), np.concatenate(s), sizes_q, sizes_s, 0.03)


def _twins_case(sd):
    s, q = surface_cloud(200, 9 * sd), surface_cloud(70, 9 * sd + 1, density=10000.0 * 70 / 200)
    return _case(np.concatenate([q, q]), np.concatenate([s, s]), [70, 70], [200, 200], 0.03)


def _outlier_case(sd):
    s = surface_cloud(400, 5 * sd)
    s = np.concatenate([s, np.asarray([[300.0, -300.0, 300.0]], F32)])     # 10^4 cells of one radius away
    q = np.concatenate([surface_cloud(65, 5 * sd + 1, density=10000.0 * 65 / 400), s[-1:], s[-1:] + F32(0.01)])
    return _case(q, s, [len(q)], [len(s)], 0.03)


RADIUS_CASES = {
    "lattice": _lattice_case,
    "nq1": lambda: _random_case(1, 300, 1),
    "nq63": lambda: _random_case(63, 300, 2),
    "nq64": lambda: _random_case(64, 300, 3),
    "nq65": lambda: _random_case(65, 300, 4),
    "nq1025": lambda: _random_case(1025, 700, 5),
    "outside": lambda: _random_case(10, 500, 6, extra_q=_outside),
    "self": lambda: _cleared(lambda sd: (lambda s: _case(s, s, [len(s)], [len(s)], 0.03))(surface_cloud(500, 77 * sd)), 7),
    "batch": lambda: _cleared(_batch_case, 8),
    "twins": lambda: _cleared(_twins_case, 9),
    "whole": lambda: _cleared(lambda sd: _case(surface_cloud(40, 3 * sd), surface_cloud(50, 3 * sd + 1), [40], [50], 10.0), 10),
    "outlier": lambda: _cleared(_outlier_case, 11),
    "sparse": lambda: _cleared(lambda sd: _case(surface_cloud(100, 2 * sd, density=100.0), surface_cloud(60, 2 * sd + 1, density=100.0),
                                                [100], [60], 0.03), 12),
}
RADIUS_KS = (1, 15, 16, 17, 32, 33, 64)


def subsample_cases():
    """name -> (points, lengths, dl, features or None, max_p)"""
    g = np.random.default_rng(3)
    feat = lambda n, F: g.standard_normal((n, F)).astype(F32)
    grid = np.stack(np.meshgrid(*[np.arange(5.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    batch = [surface_cloud(n, 40 + k, shift=(0.1 * k, 0, -0.2 * k)) for k, n in enumerate((1, 300, 64, 1025))]
    twin = surface_cloud(257, 50)
    out = {
        "one_point": (np.asarray([[0.3, -0.2, 5.0]], F32), [1], 0.02, None, 0),
        "n63": (surface_cloud(63, 41), [63], 0.02, None, 0),
        "n64": (surface_cloud(64, 42), [64], 0.02, None, 0),
        "n65": (surface_cloud(65, 43), [65], 0.02, None, 0),
        "one_voxel": ((0.5 + 0.01 * g.random((200, 3))).astype(F32), [200], 1.0, feat(200, 3), 0),
        "own_voxel": (g.permutation(grid).astype(F32), [125], 0.5, None, 0),
        "faces_negative": (lattice_cloud(300, 44, -24, 8, 0.125), [300], 0.125, None, 0),
        "batch": (np.concatenate(batch), [1, 300, 64, 1025], 0.02, None, 0),
        "twins": (np.concatenate([twin, twin]), [257, 257], 0.02, feat(514, 1), 0),
        "outlier": (np.concatenate([surface_cloud(500, 45), np.asarray([[200.0, 0.1, -200.0]], F32)]), [501], 0.02, None, 0),
        "max_p_below": (np.concatenate(batch), [1, 300, 64, 1025], 0.02, feat(1390, 3), 40),
        "max_p_above": (surface_cloud(300, 46), [300], 0.02, None, 100000),
        "F1": (surface_cloud(300, 47), [300], 0.03, feat(300, 1), 0),
        "F3": (surface_cloud(300, 48), [300], 0.03, feat(300, 3), 0),
        "F32": (np.concatenate([surface_cloud(300, 49), surface_cloud(200, 51)]), [300, 200], 0.03, feat(500, 32), 0),
    }
    out["twins"][3][257:] = out["twins"][3][:257]
    return out


def lattice_voxels(seed=0):
    """dl = 0.125, coordinates multiples of 1/64, every voxel holds a power of two of points (1 .. 64): float64 means are exact and
    fit float32."""
    g = np.random.default_rng(seed)
    clouds = []
    for _ in range(2):
        pts = []
        for v in g.permutation(np.stack(np.meshgrid(*[np.arange(-3, 3)] * 3, indexing="ij"), -1).reshape(-1, 3))[:20]:
            k = 2 ** int(g.integers(0, 7))
            pts.append((v * 8 + g.integers(0, 8, size=(k, 3))) / 64.0)
        clouds.append(g.permutation(np.concatenate(pts)).astype(F32))
    return np.concatenate(clouds), [len(c) for c in clouds], 0.125
