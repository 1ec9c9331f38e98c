"""Rigid alignment, everything that needs no GPU: the ABI's host side, the refusals of the ops and of the public functions, the seeded
hypothesis draw, and the float64 restatement (tests/_rigid_ref.py) that tests/test_rigid.py holds the kernels to -- pinned against
the reference's fixture F20 and against the planted inputs, whose preconditions are asserted here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native as N
from deformationpyramid_amd import ops, rigid
from tests import _rigid_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndp_rigid_fit", "ndp_rigid_score", "ndp_ransac_rigid")
INVALID = -1
P = ctypes.c_void_p(64)                                         # never dereferenced: every call below is refused on the host
PLANTED = [(1000, 0.3, 4096, 1), (2049, 0.5, 1024, 2)]          # K, inlier share, H, seed; thr = 0.05


def last_error():
    return N.lib().ndp_last_error().decode()


def test_abi_carries_the_rigid_entries():
    L = N.lib()
    assert L.ndp_version() >= 211
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    declared = set(re.findall(r"^(?:int|const char \*)\s*\*?(ndp_[a-z0-9_]+)\s*\(", header, flags=re.M))
    for name in NAMES + ("ndp_ransac_rigid_workspace",):
        assert name in declared and name in N._SIGS
        assert getattr(L, name) is not None
    assert "ndp_rigid.inc" in N.HEADERS                         # part of the build id


def off(*v):
    return (ctypes.c_int * len(v))(*v)


def ransac(o=off(0, 10), B=1, H=8, thr=0.05, edge=0.9, iters=2, src=P, ws=P):
    return N.lib().ndp_ransac_rigid(src, P, P, o, B, P, H, thr, edge, iters, ws, P, P, P, P, P, P, P, None, None, None, None)


@pytest.mark.parametrize("kw,text", [
    (dict(o=off(0, 2)), "K >= 3"), (dict(o=off(0, 5, 4), B=2), "monotone"), (dict(H=0), "H >= 1"), (dict(thr=0.0), "positive and finite"),
    (dict(thr=float("inf")), "positive and finite"), (dict(thr=float("nan")), "positive and finite"), (dict(edge=1.5), "edge_ratio"),
    (dict(iters=-1), "refine_iters"), (dict(src=None), "null pointer"), (dict(ws=None), "null pointer"), (dict(B=0), "B must lie"),
    (dict(ws=ctypes.c_void_p(66)), "aligned")])
def test_ransac_refusals(kw, text):
    assert ransac(**kw) == INVALID
    assert last_error().startswith("ndp_ransac_rigid: ") and text in last_error()


def test_fit_and_score_refusals():
    L = N.lib()
    assert L.ndp_rigid_fit(P, P, P, P, P, off(0, 10), 1, 1e-4, P, P, P, P, None) == INVALID and "not both" in last_error()
    assert L.ndp_rigid_fit(P, P, None, None, P, off(0, 10, 5), 2, 1e-4, P, P, P, P, None) == INVALID and "monotone" in last_error()
    assert L.ndp_rigid_fit(P, P, None, None, P, off(0, 10), 1, -1.0, P, P, P, P, None) == INVALID and "eps" in last_error()
    assert L.ndp_rigid_fit(P, P, None, None, P, off(0, 10), 1, 1e-4, None, P, P, P, None) == INVALID and "null pointer" in last_error()
    assert L.ndp_rigid_score(P, P, P, P, off(0, 0), 1, 4, 0.1, P, P, None) == INVALID and "K >= 1" in last_error()
    assert L.ndp_rigid_score(P, P, P, P, off(0, 9), 1, 0, 0.1, P, P, None) == INVALID and "H >= 1" in last_error()
    assert L.ndp_rigid_score(P, P, P, P, off(0, 9), 1, 4, -0.1, P, P, None) == INVALID and "positive and finite" in last_error()
    nb = ctypes.c_longlong()
    assert L.ndp_ransac_rigid_workspace(3, 257, ctypes.byref(nb)) == 0 and nb.value == 4 * (14 * 3 * 257 + 2 * 3 * 2)


def test_ops_refuse_cpu_tensors():
    s, y = R.random_cloud(16, 1), R.random_cloud(16, 2)
    with pytest.raises(N.NdpError):
        ops.rigid_fit(s, y)
    with pytest.raises(N.NdpError):
        ops.rigid_score(torch.zeros(1, 1, 12), s, y, 0.1)
    with pytest.raises(N.NdpError):
        ops.ransac_rigid(s, y, rigid.draw_triples(16, 8, 0), 0.1)


def test_draw_triples():
    a, b = rigid.draw_triples(500, 4096, 7), rigid.draw_triples(500, 4096, 7)
    assert a.shape == (4096, 3) and a.dtype == torch.int32 and torch.equal(a, b)
    assert int(a.min()) >= 0 and int(a.max()) < 500
    assert not torch.equal(a, rigid.draw_triples(500, 4096, 8))
    c = rigid.draw_triples([3, 40, 500], 64, 7)
    assert c.shape == (3, 64, 3) and c.dtype == torch.int32 and torch.equal(c, rigid.draw_triples([3, 40, 500], 64, 7))
    for k, row in zip((3, 40, 500), c):
        assert int(row.min()) >= 0 and int(row.max()) < k


def test_only_three_point_hypotheses_are_served():
    with pytest.raises(ValueError, match="ransac_n = 3"):
        rigid.ransac_pose_estimation(np.zeros((8, 3)), np.zeros((8, 3)), [np.arange(8), np.arange(8)], ransac_n=4)


def test_restatement_reproduces_the_reference_fixture():
    f = np.load(os.path.join(ROOT, "tests", "golden", "F20_procrustes.npz"))
    X, Y, w = (torch.from_numpy(f[k]) for k in ("X", "Y", "w"))
    assert X.shape == (4, 257, 3) and w.shape == (4, 257, 1) and int((w[1] == 0).sum()) == 64
    Rr, t, cond = R.procrustes_ref(X, Y, w)
    assert float((Rr - torch.from_numpy(f["R"]).double()).abs().max()) < 1e-6
    assert float((t - torch.from_numpy(f["t"]).double()).abs().max()) < 1e-6
    assert float(((cond - torch.from_numpy(f["condition"])) / cond).abs().max()) < 1e-5
    assert f["R"].dtype == np.float32 and f["t"].shape == (4, 3, 1)
    det = torch.linalg.det(Rr)
    assert float((det - 1).abs().max()) < 1e-12                   # the mirrored problem included: a rotation, not a reflection
    U, D, Vh = torch.linalg.svd((Y[2] - Y[2].mean(0)).double().T @ (X[2] - X[2].mean(0)).double())
    assert float(torch.linalg.det(U) * torch.linalg.det(Vh)) < 0  # ... and that problem does need the fix
    assert float(cond[3]) > 1e3                                   # the nearly planar one


@pytest.mark.parametrize("K,share,H,seed", PLANTED)
def test_planted_inputs_and_their_preconditions(K, share, H, seed):
    thr = 0.05
    s, y, inl = R.planted(K, share, seed)
    assert s.dtype == torch.float32 and int(inl.sum()) == int(K * share + 1e-9)
    tri = rigid.draw_triples(K, H, seed)
    o = R.ransac_ref(s, y, tri, thr)
    assert o.status == 0 and o.accepted >= 100
    assert int(o.h_count.max()) == int(inl.sum())                 # the best hypothesis already finds exactly the planted ones
    assert o.count == int(inl.sum()) and torch.equal(o.mask, inl)
    assert float((o.R - R.PLANTED_R).abs().max()) < 2e-3 and float((o.t - R.PLANTED_T).abs().max()) < 2e-3
    for it in (1, 2):                                             # no residual near the threshold after a refit: fp32 decides alike
        d = R.refine_ref(o.h_T[o.best], s, y, thr, it).d2.sqrt()
        assert not bool(((d > thr * (1 - 1e-3)) & (d < thr * (1 + 1e-3))).any())
    band = ((o.ratio - 0.9).abs() < 0.9e-4).any(1) | ((o.cond / R.COND_MAX - 1).abs() < 1e-4)
    assert int(band.sum()) <= H // 100                            # and next to no rejection decision near its limit


def test_driver_accepts_the_rigid_flags(monkeypatch):
    sys.path.insert(0, ROOT)
    import eval_supervised
    ap = eval_supervised.make_parser()
    a = ap.parse_args([])
    assert a.rigid_landmarks == 0.0 and a.rigid_landmarks_filter is False
    a = ap.parse_args(["--rigid-landmarks", "0.05", "--rigid-landmarks-filter"])
    assert a.rigid_landmarks == 0.05 and a.rigid_landmarks_filter is True
