"""Surface normals on the GPU: the kernels of csrc/ndp_normals.inc against the float64 restatements of tests/_normals_ref.py.

k nearest neighbours are exact: bitwise on lattice clouds, ordered by (d2, index), no closer point left out.  The PCA normals and
the point-to-plane figures are held to a bar measured per case and per tensor: the kernels' max-abs error against float64 may be at
most the larger of
    4 x the error of the SAME restatement run eagerly in float32 on the same inputs, and
    16 float32 ulps (of 1 for normals and curvature, of the tensor's largest magnitude otherwise).
Every case prints its ratios (error / bar) before it asserts; profiles/normals_accuracy.txt is that output."""
import functools
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import _normals_ref as R
from tests._helpers import VARIANTS, scale_heads, seeded_pyramid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ULPS16_OF_1 = 16.0 * float(np.spacing(np.float32(1.0)))


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


def gpu_knn(q, r, K):
    from deformationpyramid_amd import ops
    d2, idx = ops.knn(q.cuda().contiguous(), r.cuda().contiguous(), K)
    assert d2.shape == (q.shape[0], K) and idx.shape == (q.shape[0], K) and idx.dtype == torch.int32
    return d2.cpu(), idx.cpu()


# ================================================================================================ k nearest neighbours
# 64 queries per workgroup (63 / 64 / 65), 2048 references per LDS tile (2047 / 2048 / 2049 and several tiles), the list capacities
# 8 / 16 / 32 with every K of the issue's list and the K beside a capacity (8, 9, 16, 17), nr == K, nq == 1
KNN_SHAPES = [(63, 2047, 1), (64, 2048, 3), (65, 2049, 8), (1, 2049, 16), (257, 4100, 31), (300, 32, 32), (130, 5000, 32), (5, 3, 3),
              (1, 1, 1), (129, 2050, 9), (127, 300, 17), (64, 16, 16)]


@pytest.mark.parametrize("nq,nr,K", KNN_SHAPES)
def test_knn_lattice_is_bitwise_float64(dev, nq, nr, K):
    q, r = R.lattice_cloud(nq, 100 + nq), R.lattice_cloud(nr, 200 + nr)
    d2, idx = gpu_knn(q, r, K)
    rd2, ridx = R.knn_ref(q, r, K)
    assert torch.equal(idx.long(), ridx)
    assert torch.equal(d2.double(), rd2)                        # every operation of the chain is exact on this lattice
    if nr >= 2047 and K > 1 and nq > 1:                         # (at most 12288 distinct distances: the rows do hold ties)
        assert bool((rd2[:, 1:] == rd2[:, :-1]).any())


def test_knn_of_a_cloud_concatenated_with_itself(dev):
    c = R.random_cloud(1100, 7)
    n = c.shape[0]
    d2, idx = gpu_knn(c[:300], torch.cat([c, c]), 8)
    assert torch.equal(d2[:, 0::2], d2[:, 1::2])                # equal-d2 pairs (j, j + n), the lower index first
    assert torch.equal(idx[:, 0::2] + n, idx[:, 1::2]) and bool((idx[:, 0::2] < n).all())
    assert torch.equal(idx[:, 0], torch.arange(300, dtype=torch.int32)) and bool((d2[:, :2] == 0).all())


@pytest.mark.parametrize("nq,nr,K", KNN_SHAPES)
def test_knn_random_clouds_are_exact(dev, nq, nr, K):
    q, r = R.random_cloud(nq, 300 + nq), R.random_cloud(nr, 400 + nr) * 1.1 + 0.02
    d2, idx = gpu_knn(q, r, K)
    assert bool((idx >= 0).all()) and bool((idx < nr).all())
    assert all(len(set(row)) == K for row in idx.tolist())      # no reference twice
    ordered = (d2[:, 1:] > d2[:, :-1]) | ((d2[:, 1:] == d2[:, :-1]) & (idx[:, 1:] > idx[:, :-1]))
    assert bool(ordered.all())                                  # rows ascending in (d2, index)
    ulps4 = 4.0 * torch.from_numpy(np.spacing(d2.numpy())).double()
    exact = R.pair_d2(q, r, idx)
    assert bool(((d2.double() - exact).abs() <= ulps4).all())   # the distance of the named pair
    full = ((q.double()[:, None, :] - r.double()[None, :, :]) ** 2).sum(-1)
    full.scatter_(1, idx.long(), math.inf)                      # what the row does not list
    if nr > K:
        assert bool((full.min(dim=1).values >= d2[:, -1].double() - ulps4[:, -1]).all())


@pytest.mark.parametrize("S,T", [(127, 2049), (2049, 128), (1, 1), (600, 500)])
def test_knn_first_column_is_bitwise_chamfer_nn(dev, S, T):
    from deformationpyramid_amd import ops
    x, y = R.random_cloud(S, 500 + S).cuda(), (R.random_cloud(T, 600 + T) * 1.1).cuda()
    d2x, ix, d2y, iy = ops.chamfer_nn(x, y)
    a, b = ops.knn(x, y, 1), ops.knn(y, x, 1)
    assert torch.equal(a[0][:, 0], d2x) and torch.equal(a[1][:, 0], ix) and torch.equal(b[0][:, 0], d2y) and torch.equal(b[1][:, 0], iy)
    lx, ly = R.lattice_cloud(S, 1).cuda(), R.lattice_cloud(T, 2).cuda()            # ties: the lowest index on both
    nn = ops.chamfer_nn(lx, ly)
    a = ops.knn(lx, ly, 1)
    assert torch.equal(a[0][:, 0], nn[0]) and torch.equal(a[1][:, 0], nn[1])
    K = min(8, T)
    one, two = ops.knn(x, y, K), ops.knn(x, y, K)               # run to run
    assert torch.equal(one[0], two[0]) and torch.equal(one[1], two[1])


# ================================================================================================ PCA normals
PCA_CASES = [(600, 16), (2048, 16), (4096, 16), (4096, 32)]    # (n_total of surface_pair, K): no neighbourhood below the gap of 0.05


@functools.lru_cache(maxsize=None)
def pca_case(n_total, K):
    """The cloud, the kernel's own neighbour lists and outputs, and both restatements on those lists (computed once, never modified)."""
    from deformationpyramid_amd import ops
    from deformationpyramid_amd.synthetic import surface_pair
    p = surface_pair(0, n_total, partial=False)[0].contiguous()
    pd = p.cuda()
    _, idx = ops.knn(pd, pd, K)
    normals, curv = ops.normals_from_knn(pd, idx, want_curvature=True)
    idx = idx.cpu()
    return p, idx, normals.cpu(), curv.cpu(), R.pca_ref(p, idx), R.pca_ref(p, idx, torch.float32)


@pytest.mark.parametrize("n_total,K", PCA_CASES)
def test_pca_against_float64_eigh(dev, n_total, K):
    p, idx, normals, curv, r64, r32 = pca_case(n_total, K)
    keep = r64.gap >= 0.05                                      # below it the eigenvector is ill-defined
    left_out = int((~keep).sum())
    assert left_out <= 0.01 * p.shape[0]
    assert torch.isfinite(normals).all() and torch.isfinite(curv).all()
    assert float((normals.double().norm(dim=1) - 1).abs().max()) <= ULPS16_OF_1
    e_n, e32_n = float(R.sin_angle(normals, r64.normal)[keep].max()), float(R.sin_angle(r32.normal, r64.normal)[keep].max())
    e_c, e32_c = float((curv.double() - r64.curvature)[keep].abs().max()), float((r32.curvature.double() - r64.curvature)[keep].abs().max())
    b_n, b_c = max(4 * e32_n, ULPS16_OF_1), max(4 * e32_c, ULPS16_OF_1)
    print(f"normals_accuracy pca n={p.shape[0]} K={K} left_out={left_out} min_gap={float(r64.gap.min()):.3f} "
          f"sin={e_n / b_n:.3f}({e_n:.2e}/{b_n:.2e}, eager32 {e32_n:.2e}) curvature={e_c / b_c:.3f}({e_c:.2e}/{b_c:.2e}, eager32 {e32_c:.2e})")
    assert e_n <= b_n and e_c <= b_c


def test_pca_planar_patch_and_coincident_points(dev):
    from deformationpyramid_amd import ops
    g = torch.arange(8, dtype=torch.float32) / 8.0
    u, v = torch.meshgrid(g, g, indexing="ij")
    for axis in range(3):                                       # the plane coordinate[axis] = 1 / 4: an exact axis normal
        cols = [u.reshape(-1), v.reshape(-1)]
        cols.insert(axis, torch.full((64,), 0.25))
        p = torch.stack(cols, dim=1).contiguous().cuda()
        _, idx = ops.knn(p, p, 9)
        n, c = ops.normals_from_knn(p, idx, want_curvature=True)
        want = torch.zeros(64, 3)
        want[:, axis] = 1.0
        assert torch.equal(n.cpu(), want) and bool((c == 0).all())
        below = torch.zeros(3)
        below[axis] = -5.0
        assert torch.equal(ops.normals_from_knn(p, idx, viewpoint=below).cpu(), -want)
    p = R.random_cloud(40, 3)
    p[:8] = p[0]                                                # eight coincident points, K = 8: their neighbourhoods are one point
    pd = p.cuda()
    d2, idx = ops.knn(pd, pd, 8)
    assert bool((d2[:8] == 0).all())
    n, c = ops.normals_from_knn(pd, idx, want_curvature=True)
    assert bool((n[:8] == 0).all()) and bool((c[:8] == 0).all())
    assert torch.isfinite(n).all() and torch.isfinite(c).all() and bool((n[8:].norm(dim=1) > 0.99).all())
    bad = idx.clone()
    bad[5, 2] = 40                                              # not an index into p: that row is marked, nothing else changes
    nb = ops.normals_from_knn(pd, bad)
    assert torch.isnan(nb[5]).all() and torch.equal(nb[torch.arange(40) != 5], n[torch.arange(40) != 5])


def test_pca_sign_rules(dev):
    from deformationpyramid_amd import ops
    p, idx, normals, _, _, _ = pca_case(600, 16)
    big = normals.abs().argmax(dim=1)                           # the first axis of largest magnitude
    assert bool((normals[torch.arange(len(p)), big] > 0).all())
    inside = torch.tensor([0.01, -0.02, 0.015])                 # the surface is star-shaped about the origin: these face inward
    nv = ops.normals_from_knn(p.cuda(), idx.cuda(), viewpoint=inside).cpu()
    dots = (nv.double() * (inside.double() - p.double())).sum(1)
    assert bool((dots >= 0).all())
    assert bool(((nv == normals).all(dim=1) | (nv == -normals).all(dim=1)).all())     # only the sign differs
    assert 0 < int((nv == -normals).all(dim=1).sum()) < len(p)
    assert float(((nv.double() * torch.nn.functional.normalize(p.double(), dim=1)).sum(1) < 0).double().mean()) > 0.99


def test_estimate_normals_is_the_composition(dev):
    from deformationpyramid_amd import ops
    from deformationpyramid_amd.normals import estimate_normals
    p, idx, normals, curv, _, _ = pca_case(600, 16)
    n1 = estimate_normals(p.numpy())                            # numpy in, device out
    assert n1.is_cuda and torch.equal(n1.cpu(), normals)
    n2, c2 = estimate_normals(p.cuda(), k=16, return_curvature=True)
    assert torch.equal(n2.cpu(), normals) and torch.equal(c2.cpu(), curv)
    vp = (0.0, 0.0, 2.0)
    n3 = estimate_normals(p, k=8, viewpoint=vp)
    assert torch.equal(n3, ops.normals_from_knn(p.cuda(), ops.knn(p.cuda(), p.cuda(), 8)[1], viewpoint=vp))


# ================================================================================================ point to plane
P2P_SIZES = [(1, 1), (63, 65), (300, 246), (2000, 1999)]


@functools.lru_cache(maxsize=None)
def p2p_inputs(S, T):
    x, y = R.random_cloud(S, 700 + S), R.random_cloud(T, 800 + T) * 1.1 + 0.02
    nx = torch.nn.functional.normalize(R.random_cloud(S, 900 + S), dim=1).contiguous()
    ny = torch.nn.functional.normalize(R.random_cloud(T, 1000 + T), dim=1).contiguous()
    return x, y, nx, ny


def gpu_p2p(x, y, nx, ny, **kw):
    from deformationpyramid_amd import ops
    return ops.point_to_plane(x.cuda(), y.cuda(), nx.cuda(), ny.cuda(), **kw)


def check_p2p(tag, got, r64, r32):
    worst = []
    for name, mine, a, b in (("values", got[0][:3], r64.out[:3], r32.out[:3]), ("consistency", got[0][3:], r64.out[3:], r32.out[3:]),
                             ("gx", got[1], r64.gx, r32.gx), ("gy", got[3], r64.gy, r32.gy)):
        err, bound = float((mine.cpu().double() - a).abs().max()), R.bar(a, b)
        assert np.isfinite(err), (tag, name)
        worst.append((name, err, bound))
    print(f"normals_accuracy point_to_plane {tag} " + " ".join(f"{k}={e / b:.3f}({e:.2e}/{b:.2e})" for k, e, b in worst))
    for name, err, bound in worst:
        assert err <= bound, (tag, name, err, bound)


@pytest.mark.parametrize("cut", ["inf", "median"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("S,T", P2P_SIZES)
def test_point_to_plane_against_float64(dev, S, T, mode, cut):
    from deformationpyramid_amd import ops
    x, y, nx, ny = p2p_inputs(S, T)
    nn = ops.chamfer_nn(x.cuda(), y.cuda())
    trunc = math.inf if cut == "inf" else float(nn[0].median())          # some pairs are cut ((1, 1): the only one)
    got = gpu_p2p(x, y, nx, ny, trunc=trunc, mode=mode, nn=nn, want_grad_y=True)
    cpu_nn = tuple(t.cpu() for t in nn)
    if cut == "median":
        assert int((cpu_nn[0] < trunc).sum()) < S
    r64 = R.point_to_plane_ref(x, y, nx, ny, cpu_nn, trunc, mode)
    r32 = R.point_to_plane_ref(x, y, nx, ny, cpu_nn, trunc, mode, dtype=torch.float32)
    assert abs(float(got[0][0]) - float(got[0][1] + got[0][2])) <= R.ulps16(r64.out[:1])
    check_p2p(f"S={S} T={T} mode={mode} trunc={cut}", got, r64, r32)


def test_point_to_plane_against_the_reference_fixture(dev, golden):
    from deformationpyramid_amd import loss
    g = golden("F19_point_to_plane")
    x, y, nx, ny = (torch.from_numpy(g[k]) for k in ("x", "y", "nx", "ny"))
    got = gpu_p2p(x, y, nx, ny, want_grad_y=True)
    assert np.array_equal(got[2][1].cpu().numpy(), g["idx_x"])
    worst = []
    for name, mine, key in (("values", got[0][:3], "values"), ("gx", got[1], "gx"), ("gy", got[3], "gy")):
        a, b = torch.from_numpy(g[f"f64.{key}"]), torch.from_numpy(g[f"f32.{key}"])
        worst.append((name, float((mine.cpu().double() - a).abs().max()), R.bar(a, b)))
    print("normals_accuracy point_to_plane F19 " + " ".join(f"{k}={e / b:.3f}({e:.2e}/{b:.2e})" for k, e, b in worst))
    for name, err, bound in worst:
        assert err <= bound, (name, err, bound)
    # the loss-module surface: the reference's signature, its four results, gradients in both clouds
    xd, yd = x.cuda().requires_grad_(True), y.cuda().requires_grad_(True)
    total, px, py, ref_n = loss.point_2_plane_distance(xd[None], yd[None], x_normals=nx.cuda()[None], y_normals=ny.cuda()[None])
    total.backward()
    assert torch.equal(total.detach(), got[0][0]) and torch.equal(px, got[0][1]) and torch.equal(py, got[0][2])
    assert torch.equal(xd.grad, got[1]) and torch.equal(yd.grad, got[3])
    assert torch.equal(ref_n.cpu(), ny[torch.from_numpy(g["idx_x"])])
    plane = loss.point_2_plane_distance(xd[None], yd[None], x_normals=nx.cuda()[None], y_normals=ny.cuda()[None], true_plane=True, trunc=0.01)
    assert torch.equal(plane[0].detach(), gpu_p2p(x, y, nx, ny, mode=1, trunc=0.01)[0][0])


def test_normal_consistency_with_a_zero_normal(dev):
    x, y, nx, ny = p2p_inputs(300, 246)
    nx = nx.clone()
    nx[0] = 0.0
    ny = ny.clone() * 3.0                                       # cosine_similarity does not need unit normals
    out, gx, nn = gpu_p2p(x, y, nx, ny, want_grad=False)
    assert gx is None
    ix, iy = nn[1].cpu().long(), nn[3].cpu().long()
    cs = torch.nn.functional.cosine_similarity

    def figure(dt):
        a, b = nx.to(dt), ny.to(dt)
        return (1 - cs(a, b[ix], dim=1, eps=1e-6).abs()).mean() + (1 - cs(b, a[iy], dim=1, eps=1e-6).abs()).mean()

    want = [figure(torch.float64), figure(torch.float32)]
    assert float(cs(nx[:1].double(), ny[ix[:1]].double(), dim=1, eps=1e-6)) == 0.0
    err, bound = abs(float(out[3]) - float(want[0])), R.bar(want[0].reshape(1), want[1].reshape(1))
    print(f"normals_accuracy consistency zero-normal {err / bound:.3f}({err:.2e}/{bound:.2e})")
    assert err <= bound


@pytest.mark.parametrize("mode", [0, 1])
def test_point_to_plane_bits(dev, mode):
    """want_grad_y is the exchanged call, nn= reuse is the internal search, and two runs give the same bits."""
    from deformationpyramid_amd import ops
    x, y, nx, ny = (t.cuda() for t in p2p_inputs(2000, 1999))
    trunc = 0.002
    out, gx, nn, gy = ops.point_to_plane(x, y, nx, ny, trunc=trunc, mode=mode, want_grad_y=True)
    ex = ops.point_to_plane(y, x, ny, nx, trunc=trunc, mode=mode)
    assert torch.equal(ex[1], gy) and torch.equal(ex[0][1], out[2]) and torch.equal(ex[0][2], out[1])
    shared = ops.chamfer_nn(x, y)
    assert all(torch.equal(a, b) for a, b in zip(shared, nn))
    re_use = ops.point_to_plane(x, y, nx, ny, trunc=trunc, mode=mode, nn=shared, want_grad_y=True)
    again = ops.point_to_plane(x, y, nx, ny, trunc=trunc, mode=mode, want_grad_y=True)
    for other in (re_use, again):
        assert torch.equal(other[0], out) and torch.equal(other[1], gx) and torch.equal(other[3], gy)
    value_only = ops.point_to_plane(x, y, nx, ny, trunc=trunc, mode=mode, want_grad=False)
    assert value_only[1] is None and torch.equal(value_only[0], out)
    assert 0 < int((nn[0] < trunc).sum()) < 2000 and bool(torch.isfinite(gx).all()) and bool(torch.isfinite(gy).all())


def test_mode0_reproduces_the_reference_nan_at_zero_residual(dev):
    from deformationpyramid_amd import ops
    x, y, nx, ny = (t.clone() for t in p2p_inputs(63, 65))
    y[7] = x[3]                                                 # x_3 lies on its nearest point: sqrt's backward at 0
    out, gx, nn = gpu_p2p(x, y, nx, ny, mode=0)
    assert int(nn[1][3]) == 7 and torch.isnan(gx[3]).all() and torch.isfinite(out).all()
    assert torch.isfinite(gx[torch.arange(63) != 3]).all()
    out1, gx1, _ = gpu_p2p(x, y, nx, ny, mode=1)                # the plane distance: sign(0) = 0
    assert torch.isfinite(gx1).all()


def test_gradient_flows_into_a_pyramid_level(dev):
    """loss.backward() through Deformation_Pyramid.warp(x, max_level=0): the parameter gradients are bitwise ops.level_bwd fed the
    operator's gx."""
    from deformationpyramid_amd import ops
    pyr = seeded_pyramid(11, m=2, device=dev, **VARIANTS["se3aa"])
    scale_heads(pyr, 0, 30.0)
    x, y, nx, ny = (t.to(dev) for t in p2p_inputs(300, 246))
    for mode in (0, 1):
        for q in pyr.pyramid[0].parameters():
            q.grad = None
        warped, _ = pyr.warp(x, max_level=0)
        total, parts, _ = ops.point_to_plane_distance(warped, y, nx, ny, mode=mode)
        total.backward()
        layer = pyr.pyramid[0]
        wd = warped.detach().contiguous()
        out, gx, _ = ops.point_to_plane(wd, y, nx, ny, mode=mode)
        assert torch.equal(total.detach(), out[0]) and torch.equal(parts, out[1:])
        _, act, heads = ops.level_fwd(layer.desc, layer.flat.detach(), 0, layer.k0, x, save=True)
        grads = ops.level_bwd(layer.desc, layer.flat.detach(), 0, layer.k0, x, act, heads, gx)
        seen = 0
        for (name, off, shape), q in zip(layer.desc.named_slices(), layer.parameters()):
            n = int(np.prod(shape))
            assert q.grad is not None and torch.equal(q.grad.reshape(-1), grads[off:off + n]), (mode, name)
            seen += int((q.grad != 0).sum())
        assert seen > 0


# ================================================================================================ driver
def test_shape_transfer_plane_stats(dev, tmp_path):
    from deformationpyramid_amd.meshio import write_ply_ascii
    v, f = R.icosphere(3, radius=0.5)
    write_ply_ascii(str(tmp_path / "src.ply"), v, f)
    write_ply_ascii(str(tmp_path / "tgt.ply"), v * np.array([1.1, 1.0, 0.9]) + 0.05, f)
    cmd = [sys.executable, os.path.join(ROOT, "shape_transfer.py"), "-s", str(tmp_path / "src.ply"), "-t", str(tmp_path / "tgt.ply")]
    out = subprocess.run(cmd + ["--plane-stats"], capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    hit = re.search(r"point-to-plane residual of 6000 source samples.*before (\S+)\s+after (\S+)", out.stdout)
    assert hit, out.stdout[-800:]
    before, after = float(hit.group(1)), float(hit.group(2))
    assert np.isfinite(before) and np.isfinite(after) and 0 <= after < before
    plain = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=str(tmp_path))
    assert plain.returncode == 0, plain.stderr[-2000:]
    assert plain.stdout == "".join(l for l in out.stdout.splitlines(keepends=True) if not l.startswith("point-to-plane residual"))
