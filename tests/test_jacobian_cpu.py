"""CPU-side tests of the warp Jacobian / inverse warp: the ABI (version, header, ctypes signatures), every refusal of the two entries
without a device, the conditions fixture F18 must meet for the GPU comparisons to mean something, and Registration.inverse_warp()
before any register().

Of the four inverse cases the capture script is given, one is REFUSED by its qualification rule (float64 Newton <= 6 steps and
sigma_min >= 0.5 at some head scale): (gated quaternion, m = 5, k0 = 0).  Measured by tests/golden/make_golden_jacobian.py:
sigma_min = 0.000 and float64 Newton diverging at every head scale from 30 down to 1 -- a quaternion head is normalised, so the
rotation does not depend on the head scale, and at k0 = 0 it turns by whole rotations between neighbouring points; even at k0 = -8
the gate's 0.5 (I + R) leaves sigma_min = 0.244.  The fixture lists it under `inverse_refused` with those figures, and the GPU
tests run it like the folded field (honest statuses, nothing asked of convergence).  What it was there for -- a converging inverse
through the nonrigidity gate, and one at the 1e-5 bar of the quaternion / 6D formats -- is covered by two further cases captured under
the same rule: se3aa_nr.m5.k0 (gated axis-angle, k0 = 0) and se3quat.m5.k-8 (quaternion).
"""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests.test_input_grad import BAR_F64, CASES, case_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVERSE_NAMED = ["se3aa.m5.k0", "se3aa.m9.k-8", "sim3eu.m5.k0", "se3quat_nr.m5.k0"]      # the four the feature request names
INVERSE_ADDED = ["se3aa_nr.m5.k0", "se3quat.m5.k-8"]                                     # for what the refused one was there for
INVERSE_CASES = INVERSE_NAMED[:3] + INVERSE_ADDED                                        # ... what qualified


def test_abi_version_header_and_signatures_agree():
    from deformationpyramid_amd import _native
    assert _native.lib().ndp_version() >= 206
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    for name in ("ndp_pyramid_jac", "ndp_pyramid_inverse"):
        assert name in _native._SIGS and name in _native.EXPORTS
        decl = header[header.index(f"int {name}("):]
        decl = re.sub(r"/\*.*?\*/", "", decl[:decl.index(";")], flags=re.S)
        args = [a.strip() for a in decl[decl.index("(") + 1:decl.rindex(")")].split(",")]
        sig = _native._SIGS[name]
        assert len(args) == len(sig), (name, args)
        for a, t in zip(args, sig):                                   # pointers <-> void* / struct pointer, int <-> c_int, float <-> c_float
            want = "ptr" if "*" in a else a.split()[0]
            got = {ctypes.c_int: "int", ctypes.c_float: "float"}.get(t, "ptr")
            assert want == got, (name, a, t)
        assert args[-1] == "void *stream"
        getattr(_native.lib(), name)


def test_jacobian_and_inverse_reject_bad_arguments_without_a_gpu():
    """Every refusal happens before any launch: the pointers are made-up addresses (non-null, aligned) that are never followed."""
    from deformationpyramid_amd import _native
    from deformationpyramid_amd.layout import LayerDesc
    L = _native.lib()
    V = ctypes.c_void_p
    a, odd = V(4096), V(4098)
    for desc in (LayerDesc(), LayerDesc(width=64, n_hidden=1), LayerDesc(rotfmt="quaternion", nonrigidity=True)):
        cd = desc.c_struct()
        stride = (desc.param_count + 63) // 64 * 64

        def jac(m=5, k0=-8, params=a, p_stride=stride, lo=0, hi=4, x=a, n=100, x_out=a, J=a, nin=None, nout=None):
            return L.ndp_pyramid_jac(ctypes.byref(cd), m, k0, params, p_stride, lo, hi, x, n, x_out, J, nin, nout, None)

        def inv(m=5, k0=-8, params=a, p_stride=stride, lo=0, hi=4, y=a, n=100, x=a, iters=8, tol=2e-6, res=a, status=a):
            return L.ndp_pyramid_inverse(ctypes.byref(cd), m, k0, params, p_stride, lo, hi, y, n, x, iters, tol, res, status, None)

        for f, who in ((jac, b"ndp_pyramid_jac"), (inv, b"ndp_pyramid_inverse")):
            assert f(n=0) == -1 and who in L.ndp_last_error() and b"n must be positive" in L.ndp_last_error()
            assert f(n=-3) == -1
            assert f(lo=-1) == -1 and b"levels" in L.ndp_last_error()
            assert f(hi=5) == -1 and b"levels" in L.ndp_last_error()
            assert f(lo=3, hi=2) == -1 and b"levels" in L.ndp_last_error()
            assert f(m=0, lo=0, hi=0) == -1 and f(m=17, hi=16) == -1
            assert f(k0=200) == -1 and b"float range" in L.ndp_last_error()
            assert f(p_stride=desc.param_count - 1) == -1 and b"p_stride" in L.ndp_last_error()
            assert f(params=None) == -1 and b"params_all" in L.ndp_last_error()
            assert f(params=V(4100)) == -1 and b"16-byte" in L.ndp_last_error()
        assert jac(x=None) == -1 and jac(x_out=None) == -1 and jac(J=None) == -1 and b"non-null" in L.ndp_last_error()
        assert jac(x_out=odd) == -1 and jac(J=odd) == -1 and b"4-byte aligned" in L.ndp_last_error()
        assert jac(nin=a) == -1 and b"go together" in L.ndp_last_error()
        assert jac(nout=a) == -1 and b"go together" in L.ndp_last_error()
        assert jac(nin=a, nout=odd) == -1 and b"normals" in L.ndp_last_error()
        assert inv(y=None) == -1 and inv(x=None) == -1 and inv(res=None) == -1 and inv(status=None) == -1
        assert inv(x=odd) == -1 and inv(res=odd) == -1 and inv(status=odd) == -1 and b"4-byte aligned" in L.ndp_last_error()
        assert inv(iters=0) == -1 and b"iters" in L.ndp_last_error()
        for tol in (0.0, -1e-6, float("inf"), float("nan")):
            assert inv(tol=tol) == -1 and b"tol" in L.ndp_last_error(), tol
    for bad in (LayerDesc(width=257), LayerDesc(width=0), LayerDesc(n_hidden=4)):
        cd = bad.c_struct()
        assert L.ndp_pyramid_jac(ctypes.byref(cd), 5, -8, a, 1 << 20, 0, 4, a, 100, a, a, None, None, None) == -2
        assert L.ndp_pyramid_inverse(ctypes.byref(cd), 5, -8, a, 1 << 20, 0, 4, a, 100, a, 8, 2e-6, a, a, None) == -2
        assert b"width" in L.ndp_last_error()


def fixture_j64(g, key):
    return g[f"{key}.J"].astype(np.float64) + g[f"{key}.J64_minus_J"].astype(np.float64)


def test_fixture_cases_shares_and_size(golden):
    """F18 holds exactly the cases the GPU test walks; at k0 = 0 the network's part of J is at least a tenth of the direct part (at
    the shipped k0 = -8 it is about 1e-2 of it or less: a comparison relative to max |J| ~ 1 would pass wrong tangents there); the
    reference's float32 J sits within a tenth of the tighter bar of its float64; and the file stays below its ceiling."""
    g = golden("F18_jacobian")
    assert list(g["cases"]) == [case_key(*c) for c in CASES]
    worst = 0.0
    for c in CASES:
        key = case_key(*c)
        J = g[f"{key}.J"]
        assert J.shape == (256, 3, 3) and J.dtype == np.float32 and np.isfinite(J).all()
        share, rel64 = float(g[f"{key}.share"]), float(g[f"{key}.rel64"])
        if c[2] == 0:
            assert share >= 0.1, (key, share)
        d = np.abs(J - fixture_j64(g, key)).max() / np.abs(fixture_j64(g, key)).max()
        assert abs(d - rel64) <= 1e-3 * rel64 + 1e-12, (key, d, rel64)          # (the float64 J is really beside the float32 one)
        worst = max(worst, rel64)
    for name in g["chains"]:
        assert g[f"chain.{name}.J"].shape == (256, 3, 3)
        worst = max(worst, float(g[f"chain.{name}.rel64"]))
    assert list(g["chains"]) == ["L2_4", "se3aa", "sim3eu", "se3quat_nr"]
    print(f"worst rel64 {worst:.3e}")
    assert worst < 0.1 * BAR_F64, worst
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "F18_jacobian.npz")) <= 900 * 1024
    det = g["fold.det64"]
    assert det.shape == (500,) and (det <= 0).any() and (det > 0).any() and g["fold.y"].shape == (500, 3)


def test_fixture_inverse_cases_are_the_four_named(golden):
    """Every named case is either stored as qualified or listed as refused with figures that do not qualify (module docstring)."""
    g = golden("F18_jacobian")
    assert sorted(list(g["inverse_cases"]) + list(g["inverse_refused"])) == sorted(INVERSE_NAMED + INVERSE_ADDED)
    assert list(g["inverse_cases"]) == INVERSE_CASES and list(g["inverse_refused"]) == INVERSE_NAMED[3:]
    for name in g["inverse_refused"]:
        its, smin = int(g[f"inv.{name}.iters64"]), float(g[f"inv.{name}.sigma_min"])
        print(f"refused {name}: float64 Newton steps {its}, sigma_min {smin:.3e}")
        assert not (0 <= its <= 6 and smin >= 0.5)
        assert g[f"inv.{name}.y"].shape == (500, 3)


@pytest.mark.parametrize("name", INVERSE_CASES)
def test_fixture_inverse_case_qualifies(golden, name):
    """float64 Newton from x0 = y needs at most 6 steps and the smallest singular value of J is at least 0.5: only then are 8 float32
    iterations a safe ceiling."""
    g = golden("F18_jacobian")
    its, smin = int(g[f"inv.{name}.iters64"]), float(g[f"inv.{name}.sigma_min"])
    print(f"{name}: float64 Newton steps {its}, sigma_min {smin:.3f}, head scale {float(g[f'inv.{name}.head_scale'])}")
    assert g[f"inv.{name}.y"].shape == (500, 3)
    assert 0 <= its <= 6, (name, its)
    assert smin >= 0.5, (name, smin)


def test_registration_inverse_warp_needs_a_register_first():
    from deformationpyramid_amd.config import Config
    from deformationpyramid_amd.registration import Registration
    cfg = Config(deformation_model="NDP", device=torch.device("cpu"), depth=3, width=128, k0=-8, m=2, w_reg=0.0,
                 rotation_format="axis_angle", motion_type="SE3", samples=10, iters=5, lr=0.01, max_break_count=15,
                 break_threshold_ratio=0.001)
    model = Registration(cfg)
    with pytest.raises(RuntimeError, match="register"):
        model.inverse_warp(np.zeros((4, 3), np.float32))
    model.load_pcds(np.zeros((20, 3), np.float32), np.zeros((20, 3), np.float32))
    with pytest.raises(RuntimeError, match="register"):
        model.inverse_warp(torch.zeros(4, 3))
