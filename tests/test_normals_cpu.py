"""Surface normals, everything that needs no GPU: the ABI's host side (version, header, every refusal of ndp_knn / ndp_normals_from_knn
/ ndp_point_to_plane), meshio's vertex and face normals, and the float64 restatement (tests/_normals_ref.py) that
tests/test_normals.py holds the kernels to -- pinned against hand-made cases, torch autograd and the reference's fixture F19."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native as N
from deformationpyramid_amd import meshio
from tests import _normals_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndp_knn", "ndp_normals_from_knn", "ndp_point_to_plane")
INVALID, UNSUPPORTED = -1, -2
P = ctypes.c_void_p(64)                                         # never dereferenced: every call below is refused on the host


def last_error():
    return N.lib().ndp_last_error().decode()


def test_abi_carries_the_normals_entries():
    L = N.lib()
    assert L.ndp_version() >= 210
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*\*?(ndp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    assert declared == set(N.EXPORTS)
    for name in NAMES:
        assert name in declared and name in N._SIGS
        assert getattr(L, name) is not None
    assert "ndp_normals.inc" in N.HEADERS                       # part of the build id


def knn(nq=8, nr=40, K=4, q=P, r=P, d2=P, idx=P):
    return N.lib().ndp_knn(q, nq, r, nr, K, d2, idx, None)


@pytest.mark.parametrize("kw,code,text", [
    (dict(K=0), INVALID, "K must lie in 1..32"), (dict(K=33), INVALID, "K must lie in 1..32"), (dict(K=-1), INVALID, "K must lie in 1..32"),
    (dict(K=5, nr=4), INVALID, "K must not exceed nr"), (dict(nq=0), INVALID, "nq, nr >= 1"), (dict(nr=0, K=1), INVALID, "nq, nr >= 1"),
    (dict(q=None), INVALID, "null pointer"), (dict(r=None), INVALID, "null pointer"), (dict(d2=None), INVALID, "null pointer"),
    (dict(idx=None), INVALID, "null pointer"), (dict(nq=(1 << 24) + 1), UNSUPPORTED, "16777216"), (dict(nr=(1 << 24) + 1), UNSUPPORTED, "16777216")])
def test_knn_refusals(kw, code, text):
    assert knn(**kw) == code
    assert last_error().startswith("ndp_knn: ") and text in last_error()


def pca(n=8, K=4, p=P, idx=P, normals=P, curvature=None, viewpoint=None):
    return N.lib().ndp_normals_from_knn(p, n, idx, K, viewpoint, normals, curvature, None)


@pytest.mark.parametrize("kw,code,text", [
    (dict(K=2), INVALID, "K must be at least 3"), (dict(K=0), INVALID, "K must be at least 3"), (dict(n=0), INVALID, "n >= 1"),
    (dict(p=None), INVALID, "null pointer"), (dict(idx=None), INVALID, "null pointer"), (dict(normals=None), INVALID, "null pointer"),
    (dict(n=(1 << 24) + 1), UNSUPPORTED, "16777216")])
def test_normals_from_knn_refusals(kw, code, text):
    assert pca(**kw) == code
    assert last_error().startswith("ndp_normals_from_knn: ") and text in last_error()


def p2p(S=8, T=9, mode=0, trunc=math.inf, **ptr):
    a = dict(x=P, y=P, nx=P, ny=P, d2x=P, idx_x=P, d2y=P, idx_y=P, out=P, gx=None)
    a.update(ptr)
    return N.lib().ndp_point_to_plane(a["x"], S, a["y"], T, a["nx"], a["ny"], trunc, a["d2x"], a["idx_x"], a["d2y"], a["idx_y"], mode,
                                      a["out"], a["gx"], None)


@pytest.mark.parametrize("kw,text", [(dict(mode=2), "mode must be 0"), (dict(mode=-1), "mode must be 0"), (dict(S=0), "S, T >= 1"),
                                     (dict(T=0), "S, T >= 1"), (dict(trunc=math.nan), "trunc must not be NaN")] +
                         [({k: None}, "null pointer") for k in ("x", "y", "nx", "ny", "d2x", "idx_x", "d2y", "idx_y", "out")])
def test_point_to_plane_refusals(kw, text):
    assert p2p(**kw) == INVALID
    assert last_error().startswith("ndp_point_to_plane: ") and text in last_error()


def test_operators_refuse_cpu_tensors_and_bad_shapes():
    from deformationpyramid_amd import loss, ops
    x = torch.zeros(5, 3)
    with pytest.raises(N.NdpError):
        ops.knn(x, x, 3)
    with pytest.raises(N.NdpError):
        ops.normals_from_knn(x, torch.zeros(5, 3, dtype=torch.int32))
    with pytest.raises(N.NdpError):
        ops.point_to_plane(x, x, x, x)
    with pytest.raises(ValueError):
        loss.point_2_plane_distance(x[None], x[None])            # no normals
    with pytest.raises(NotImplementedError):                     # the Chamfer is as it was
        loss.compute_truncated_chamfer_distance(x[None], x[None], x_normals=x[None], y_normals=x[None])


# ---------------------------------------------------------------------------------- meshio
CUBE_V = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], dtype=np.float32)
CUBE_F = np.array([[0, 1, 3], [0, 3, 2], [4, 6, 7], [4, 7, 5], [0, 4, 5], [0, 5, 1], [2, 3, 7], [2, 7, 6], [0, 2, 6], [0, 6, 4], [1, 5, 7], [1, 7, 3]])


def test_vertex_normals_cube():
    n = meshio.vertex_normals(CUBE_V, CUBE_F)
    assert n.dtype == np.float64 and n.shape == (8, 3)
    want = np.zeros((8, 3))
    for a, b, c in CUBE_F:                                       # one face at a time, by hand
        fn = np.cross(CUBE_V[b].astype(np.float64) - CUBE_V[a], CUBE_V[c].astype(np.float64) - CUBE_V[a])
        assert np.dot(fn, CUBE_V[a] + CUBE_V[b] + CUBE_V[c]) > 0  # outward winding: every face's normal is its axis
        for v in (a, b, c):
            want[v] += fn
    want /= np.linalg.norm(want, axis=1, keepdims=True)
    np.testing.assert_allclose(n, want, atol=1e-15)
    np.testing.assert_allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-15)
    assert (np.sign(n) == np.sign(CUBE_V)).all()                 # every corner's normal points into its own octant
    # area weighting: corner 0 touches two triangles of each of its three faces, corner 1 two, one and one
    np.testing.assert_allclose(n[0], -np.ones(3) / math.sqrt(3), atol=1e-15)
    assert sorted(np.abs(n[1]).round(12)) == sorted((np.array([1, 1, 2]) / math.sqrt(6)).round(12))
    lone = meshio.vertex_normals(np.vstack([CUBE_V, [[5, 5, 5]]]), CUBE_F)
    assert (lone[8] == 0).all() and np.array_equal(lone[:8], n)  # a vertex of no face


def test_vertex_normals_icosphere_are_radial():
    """Within 1e-6 of the radial direction wherever the mesh is symmetric about the vertex: every vertex of the icosahedron (the
    icosphere without subdivision), and the twelve five-fold vertices of a subdivided one.  At the other vertices of a subdivided
    icosphere the surrounding triangles differ in shape, and an area-weighted sum then leaves the radius by a term of second order
    in the edge length: those are held to edge^2."""
    v, f = R.icosphere(0, radius=0.7)
    assert np.abs(meshio.vertex_normals(v, f) - v / 0.7).max() <= 1e-6
    v, f = R.icosphere(3, radius=0.7)
    n, radial = meshio.vertex_normals(v, f), v / np.linalg.norm(v, axis=1, keepdims=True)
    assert np.abs(n[:12] - radial[:12]).max() <= 1e-6
    edge = np.linalg.norm(radial[f[:, 0]] - radial[f[:, 1]], axis=1).max()
    assert 1e-6 < np.abs(n - radial).max() <= edge ** 2


def test_sample_surface_normals_leave_the_points_alone():
    v, f = R.icosphere(1)
    v = (v * np.array([1.0, 0.8, 1.3])).astype(np.float32)
    r0, r1 = np.random.default_rng(5), np.random.default_rng(5)
    pts = meshio.sample_surface(v, f, 500, r0)
    pts_n, nrm = meshio.sample_surface(v, f, 500, r1, return_normals=True)
    assert pts.dtype == np.float32 and pts.tobytes() == pts_n.tobytes()
    assert r0.random() == r1.random()                            # the stream is where it was either way
    assert nrm.dtype == np.float32 and nrm.shape == (500, 3)
    np.testing.assert_allclose(np.linalg.norm(nrm.astype(np.float64), axis=1), 1.0, atol=2e-7)
    a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
    fn = np.cross(b - a, c - a)
    fn /= np.linalg.norm(fn, axis=1, keepdims=True)
    hit = (np.abs(nrm.astype(np.float64)[:, None, :] - fn[None]).max(-1) <= 1e-7)       # the triangle(s) with this normal
    assert hit.any(axis=1).all()
    for i in range(500):                                         # orthogonal to the edges of its triangle, which holds the sample
        t = int(np.argmax(hit[i]))
        assert abs(np.dot(nrm[i], b[t] - a[t])) <= 1e-6 and abs(np.dot(nrm[i], c[t] - a[t])) <= 1e-6
        assert abs(np.dot(fn[t], pts[i] - a[t])) <= 1e-6
    assert (np.einsum("ij,ij->i", nrm, pts_n) > 0).all()         # outward on a star-shaped mesh


# ---------------------------------------------------------------------------------- the float64 restatement pins itself
def test_knn_ref_orders_ties_by_index():
    r = torch.tensor([[1., 0, 0], [0, 1, 0], [0, 0, 0], [-1, 0, 0], [0, 0, 0], [2, 0, 0]])
    d2, idx = R.knn_ref(torch.zeros(1, 3), r, 5)
    assert idx.tolist() == [[2, 4, 0, 1, 3]] and d2.tolist() == [[0, 0, 1, 1, 1]]
    assert torch.equal(R.pair_d2(torch.zeros(1, 3), r, idx), d2)


def test_pca_ref_on_a_plane_and_a_point():
    g = torch.Generator().manual_seed(0)
    p = torch.rand(30, 3, generator=g)
    p[:, 1] = 0.25                                               # the plane y = 1 / 4
    p[20:] = p[20]                                               # and ten coincident points
    idx = torch.stack([torch.arange(0, 10), torch.arange(20, 30)])
    r = R.pca_ref(p, idx)
    assert torch.equal(r.normal[0].abs(), torch.tensor([0., 1, 0], dtype=torch.float64)) and float(r.curvature[0]) == 0.0
    assert float(r.gap[0]) > 0.05 and float(r.curvature[1]) == 0.0 and not torch.isnan(r.normal).any()
    assert float(R.sin_angle(r.normal[:1], -r.normal[:1])) == 0.0


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("trunc", [math.inf, 0.004])
def test_point_to_plane_ref_gradient_is_autograd(mode, trunc):
    x, y = R.random_cloud(70, 1), R.random_cloud(55, 2) * 1.1 + 0.02
    nx, ny = torch.nn.functional.normalize(R.random_cloud(70, 3), dim=1), torch.nn.functional.normalize(R.random_cloud(55, 4), dim=1)
    nn = R.nn_ref(x, y)
    assert trunc == math.inf or 0 < int((nn[0] < trunc).sum()) < 70
    r, a = R.point_to_plane_ref(x, y, nx, ny, nn, trunc, mode), R.point_to_plane_autograd(x, y, nx, ny, nn, trunc, mode)
    assert abs(float(r.out[0] - a.total)) <= 1e-15 and float(r.out[0]) == float(r.out[1] + r.out[2])
    assert float((r.gx - a.gx).abs().max()) <= 1e-15 and float((r.gy - a.gy).abs().max()) <= 1e-15
    assert float(r.gx.abs().max()) > 1e-4 and float(r.gy.abs().max()) > 1e-4
    ex = R.point_to_plane_ref(y, x, ny, nx, (nn[2], nn[3], nn[0], nn[1]), trunc, mode)      # exchanged: the same numbers
    assert torch.equal(ex.gx, r.gy) and torch.equal(ex.gy, r.gx) and float(ex.out[1]) == float(r.out[2])


def test_point_to_plane_ref_mode0_is_the_reference(golden):
    g = golden("F19_point_to_plane")
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "F19_point_to_plane.npz")) < 900 * 1024
    x, y, nx, ny = (torch.from_numpy(g[k]) for k in ("x", "y", "nx", "ny"))
    assert x.shape == (300, 3) and y.shape == (246, 3)
    from deformationpyramid_amd.synthetic import surface_pair
    src, tgt, _, _ = surface_pair(1, n_total=600)
    # (to an ulp, not bitwise: the generator's matrix product and the norm are not bit-stable from one host CPU to the next)
    assert float((src - x).abs().max()) <= 1e-7 and float((tgt - y).abs().max()) <= 1e-7
    assert float((nx - x / x.norm(dim=1, keepdim=True)).abs().max()) <= 2e-7 and float((ny - y / y.norm(dim=1, keepdim=True)).abs().max()) <= 2e-7
    nn = R.nn_ref(x, y)
    assert np.array_equal(nn[1].numpy(), g["idx_x"])
    for dtype, tag, tol in ((torch.float64, "f64", 1e-13), (torch.float32, "f32", 2e-7)):        # (summation order is the host's)
        r = R.point_to_plane_ref(x, y, nx, ny, nn, dtype=dtype)
        assert np.abs(r.out[:3].double().numpy() - g[f"{tag}.values"]).max() <= tol
        assert np.abs(r.gx.double().numpy() - g[f"{tag}.gx"]).max() <= tol and np.abs(r.gy.double().numpy() - g[f"{tag}.gy"]).max() <= tol
    assert g["f32.values"].dtype == np.float32 and g["f64.gx"].dtype == np.float64
