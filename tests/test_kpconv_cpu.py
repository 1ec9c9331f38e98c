"""KPConv inputs without a GPU: the ABI carries the entries, every host-side refusal (through the C entries and through Python), the
workspace queries, the numpy restatement against the reference's own extensions (fixture F22), and the input preconditions of the
GPU tests of tests/test_kpconv.py."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native, kpconv, ops
from tests import _kpconv_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndp_voxel_subsample_workspace", "ndp_voxel_subsample", "ndp_radius_search_workspace", "ndp_radius_search")


@pytest.fixture(scope="module")
def L():
    return _native.lib()


def ints(*v):
    return (ctypes.c_int * len(v))(*v)


def test_abi_carries_the_entries(L):
    assert L.ndp_version() >= 213
    for name in ENTRIES:
        assert name in _native._SIGS and name in _native.EXPORTS and getattr(L, name)
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    for name in ENTRIES:
        assert f"int {name}(" in header
    assert "ndp_kpconv.inc" in " ".join(_native.HEADERS)


def test_workspace_queries(L):
    nb = ctypes.c_longlong()
    sizes = []
    for n in (1, 1000, 30000, 320000):
        assert L.ndp_voxel_subsample_workspace(n, 1, ctypes.byref(nb)) == 0
        sizes.append(nb.value)
        assert nb.value % 16 == 0 and nb.value >= 36 * n
    assert sizes == sorted(sizes) and sizes[-1] < 64 * 320000 + (1 << 20)          # O(N), not a bounding box
    assert L.ndp_radius_search_workspace(5000, 60000, 2, ctypes.byref(nb)) == 0
    big = nb.value
    assert L.ndp_radius_search_workspace(60000, 5000, 2, ctypes.byref(nb)) == 0
    assert 0 < nb.value <= big and big < 100 * 60000 + (1 << 20)
    for args in ((0, 1), (5, 0), (5, 6), (5, 65536), ((1 << 30) + 1, 1)):
        assert L.ndp_voxel_subsample_workspace(args[0], args[1], ctypes.byref(nb)) != 0
        assert b"ndp_voxel_subsample_workspace" in L.ndp_last_error()
    assert L.ndp_voxel_subsample_workspace(5, 1, None) != 0
    for args in ((0, 5, 1), (5, 0, 1), (5, 5, 0), (5, 5, 6), ((1 << 30) + 1, 5, 1)):
        assert L.ndp_radius_search_workspace(*args, ctypes.byref(nb)) != 0
        assert b"ndp_radius_search_workspace" in L.ndp_last_error()
    assert L.ndp_radius_search_workspace(5, 5, 1, None) != 0


def test_c_entries_refuse_bad_arguments(L):
    """every refusal that needs no device happens before the first HIP call: the pointers are never read"""
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    out_len = ints(0, 0)
    S = None

    def voxel(pts=p, feat=None, F=0, lengths=ints(3, 2), B=2, dl=0.1, max_p=0, ws=p, ws_bytes=1 << 40, out=p, out_f=None, inv=p, ol=out_len):
        return L.ndp_voxel_subsample(pts, feat, F, lengths, B, dl, max_p, ws, ws_bytes, out, out_f, inv, ol, S)

    for kw, word in ((dict(lengths=ints(3, 0)), b"length"), (dict(lengths=ints(-1, 6)), b"length"), (dict(B=0), b"B must"),
                     (dict(B=65536), b"B must"), (dict(lengths=None), b"null"), (dict(dl=0.0), b"dl must"), (dict(dl=-1.0), b"dl must"),
                     (dict(dl=float("nan")), b"dl must"), (dict(dl=float("inf")), b"dl must"), (dict(F=-1), b"F must"),
                     (dict(F=3), b"null"), (dict(pts=None), b"null"), (dict(out=None), b"null"), (dict(ws=None), b"null"),
                     (dict(ol=None), b"null"), (dict(ws=odd), b"aligned"), (dict(ws_bytes=64), b"workspace smaller")):
        assert voxel(**kw) != 0, kw
        assert word in L.ndp_last_error(), (kw, L.ndp_last_error())

    def radius(q=p, s=p, ql=ints(3, 2), sl=ints(4, 4), B=2, r=0.1, K=8, ws=p, ws_bytes=1 << 40, idx=p, d2=None, counts=p):
        return L.ndp_radius_search(q, s, ql, sl, B, r, K, ws, ws_bytes, idx, d2, counts, S)

    for kw, word in ((dict(ql=ints(0, 5)), b"length"), (dict(sl=ints(4, 0)), b"length"), (dict(B=0), b"B must"), (dict(ql=None), b"null"),
                     (dict(r=0.0), b"radius must"), (dict(r=-0.5), b"radius must"), (dict(r=float("nan")), b"radius must"),
                     (dict(r=float("inf")), b"radius must"), (dict(r=1e-30), b"radius * radius"), (dict(r=1e30), b"radius * radius"),
                     (dict(K=-1), b"K must"), (dict(K=65), b"K must"), (dict(q=None), b"null"), (dict(s=None), b"null"),
                     (dict(idx=None), b"null"), (dict(counts=None), b"null"), (dict(ws=None), b"null"), (dict(ws=odd), b"aligned"),
                     (dict(ws_bytes=64), b"workspace smaller")):
        assert radius(**kw) != 0, kw
        assert word in L.ndp_last_error(), (kw, L.ndp_last_error())


def test_python_refuses_bad_arguments():
    pts = torch.zeros(5, 3)
    for kw in (dict(lengths=[5, 0]), dict(lengths=[3, 1]), dict(lengths=[]), dict(dl=0.0), dict(dl=-1.0), dict(dl=float("nan")),
               dict(features=torch.zeros(4, 2)), dict(points=torch.zeros(5, 2)), dict(points=torch.zeros(0, 3))):
        a = dict(points=pts, lengths=[3, 2], dl=0.1)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.voxel_subsample(**a)
    for kw in (dict(q_lengths=[5, 0]), dict(s_lengths=[4]), dict(s_lengths=[1, 1, 3]), dict(radius=0.0), dict(radius=float("inf")),
               dict(max_neighbors=65), dict(q=torch.zeros(5)), dict(s=torch.zeros(0, 3))):
        a = dict(q=pts, s=pts, q_lengths=[3, 2], s_lengths=[2, 3], radius=0.1, max_neighbors=8)
        a.update(kw)
        with pytest.raises(ValueError):
            ops.radius_search(**a)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):            # valid arguments on the CPU: no quiet fallback
        ops.voxel_subsample(pts, [3, 2], 0.1)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.radius_search(pts, pts, [3, 2], [2, 3], 0.1, 8)
    with pytest.raises(NotImplementedError):
        kpconv.grid_subsample(pts, [5], labels=torch.zeros(5))


def test_layers_follow_the_reference_rules():
    assert kpconv._layers(R.KPFCN) == R.layers(R.KPFCN) == [(True, False, True, False)] * 3 + [(True, False, False, False)]
    arch = ["simple", "resnetb_deformable", "resnetb", "resnetb_deformable_strided", "resnetb", "global_average", "resnetb_strided"]
    assert kpconv._layers(arch) == R.layers(arch) == [(True, True, True, True)]       # a layer is emitted by its pooling block, or ahead of an upsample
    assert kpconv._layers(arch[:5] + ["nearest_upsample"]) == [(True, True, True, True), (True, False, False, False)]
    assert kpconv._layers(["simple", "max_pool", "resnetb_strided"])[1] == (False, False, True, False)


def test_restatement_reproduces_fixture_f22(golden):
    """the numpy restatement against the reference's own C++ on the reference's inputs of every level"""
    g = golden("F22_kpconv")
    K = int(g["columns"])
    assert int(g["levels"]) == 4
    for l in range(4):
        pts, lengths, radius = g[f"l{l}.points"], g[f"l{l}.lengths"], float(g[f"l{l}.radius"])
        assert pts.dtype == np.float32 and g[f"l{l}.radius"].dtype == np.float32
        r = R.radius_search(pts, pts, lengths, lengths, radius)
        assert r.clearance > 16
        rows_match(r.idx[:, :K], g[f"l{l}.conv"], pts, pts, len(pts))
        if f"l{l}.sub_points" not in g:
            assert l == 3
            continue
        dl = float(g[f"l{l}.dl"])
        sub = R.voxel_subsample(pts, lengths, dl)
        want_p, want_l = g[f"l{l}.sub_points"], g[f"l{l}.sub_lengths"]
        assert sub.lengths.tolist() == want_l.tolist()
        base = 0
        for n in want_l:
            a, b = sub.points[base:base + n], want_p[base:base + n].astype(np.float64)
            a, b = a[np.lexsort((a[:, 0], a[:, 1], a[:, 2]))], b[np.lexsort((b[:, 0], b[:, 1], b[:, 2]))]
            assert np.abs(a - b).max() <= 16 * R.ULP * np.abs(a).max()         # the reference sums in fp32
            base += n
        r = R.radius_search(want_p, pts, want_l, lengths, radius)
        assert r.clearance > 16
        rows_match(r.idx[:, :K], g[f"l{l}.pool"], want_p, pts, len(pts))
        r = R.radius_search(pts, want_p, lengths, want_l, 2 * radius)
        assert r.clearance > 16
        rows_match(r.idx[:, :K], g[f"l{l}.up"], pts, want_p, len(want_p))


def rows_match(got, want, q, s, shadow):
    w = min(got.shape[1], want.shape[1])
    got, want = got[:, :w], want[:, :w].astype(np.int64)
    assert np.array_equal((got != shadow).sum(1), (want != shadow).sum(1))
    for i in np.nonzero((got != want).any(1))[0]:
        k = np.nonzero(got[i] != want[i])[0]
        da = ((q[i].astype(np.float64) - s[got[i, k]].astype(np.float64)) ** 2).sum(-1)
        db = ((q[i].astype(np.float64) - s[want[i, k]].astype(np.float64)) ** 2).sum(-1)
        assert np.all(np.abs(da - db) < 4 * np.spacing(np.float32(np.maximum(da, db))))


@pytest.mark.parametrize("name", [n for n in R.RADIUS_CASES if n != "lattice"])
def test_radius_inputs_clear_r2(name):
    c = R.RADIUS_CASES[name]()
    assert R.radius_search(c.q, c.s, c.ql, c.sl, c.radius).clearance > 16


def test_case_preconditions():
    c = R.RADIUS_CASES["lattice"]()
    d2 = R.cloud_d2(c.q, c.s)[0]
    assert (d2 == np.float32(0.0625)).sum() >= 2 and np.array_equal(d2 * 4096, np.round(d2 * 4096))
    c = R.RADIUS_CASES["outside"]()
    full = R.radius_search(c.q, c.s, c.ql, c.sl, c.radius)
    assert full.counts.min() == 0 and full.counts[10:].max() > 0
    lo, hi = c.s.min(0), c.s.max(0)
    out_by = np.maximum(lo - c.q, c.q - hi).max(1)
    assert (out_by[10:] > 0).all() and (out_by[10:] < c.radius).any() and (out_by[10:] > c.radius).any()
    pts, lengths, dl = R.lattice_voxels()
    assert np.array_equal(pts * 64, np.round(pts * 64))
    cnt = np.bincount(R.voxel_subsample(pts, lengths, dl).inverse)
    assert np.all(cnt & (cnt - 1) == 0) and cnt.max() >= 8
    p, l, dl, _, _ = R.subsample_cases()["faces_negative"]
    assert np.array_equal(p / dl, np.round(p / dl)) and p.min() < -1
    p, l, dl, _, _ = R.subsample_cases()["outlier"]
    assert (p.max() - p.min()) / dl >= 1e4


def test_pyramid_input_clears_faces_and_r2():
    pts, lengths, pyr, seed = R.pyramid_input()
    assert pyr.clearance > 16 and lengths.tolist() == [1700, 1300] and len(pyr.points) == 4
    assert all(t.shape[0] > 0 for t in pyr.pools[:3]) and pyr.pools[3].shape == (0, 1)


def test_shape_transfer_flag_parses():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "shape_transfer.py"), "--help"], capture_output=True, text=True, cwd=ROOT)
    assert out.returncode == 0 and "--voxel-size" in out.stdout
