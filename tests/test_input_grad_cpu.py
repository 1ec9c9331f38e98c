"""CPU-side tests of the input-point gradients: argument validation of ndp_level_bwd's dx without a device, the ABI version, the
two conditions fixture F17 must meet for the GPU comparisons to mean something, and fitted_pyramid() before any register()."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests.test_input_grad import BAR_F64, CASES, case_key

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_abi_version_carries_the_dx_argument():
    from deformationpyramid_amd import _native
    assert _native.lib().ndp_version() >= 205
    assert len(_native._SIGS["ndp_level_bwd"]) == 16
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    decl = header[header.index("int ndp_level_bwd("):]
    assert decl[:decl.index(";")].rstrip().endswith("void *stream, float *dx)")


def test_level_bwd_with_dx_rejects_bad_arguments_without_a_gpu():
    """Every refusal happens before any launch: the pointers are made-up addresses (non-null, aligned) that are never followed."""
    from deformationpyramid_amd import _native
    from deformationpyramid_amd.layout import LayerDesc
    L = _native.lib()
    V = ctypes.c_void_p
    a = V(4096)
    for desc in (LayerDesc(), LayerDesc(width=64, n_hidden=1)):
        cd = desc.c_struct()
        stride = (desc.param_count + 3) // 4 * 4

        def call(level=4, k0=-8, n=100, n_part=2, p_stride=stride, dx=a, x=a):
            return L.ndp_level_bwd(ctypes.byref(cd), a, level, k0, x, n, a, a, a, None, a, a, n_part, p_stride, None, dx)

        assert call(n=0) == -1 and call(n=-5) == -1                               # bad sizes
        assert call(n_part=0) == -1
        assert call(p_stride=desc.param_count - 1) == -1 and b"p_stride" in L.ndp_last_error()
        assert call(x=None) == -1
        assert call(level=-1) == -1 and b"dx needs" in L.ndp_last_error()         # dx needs the level's frequency
        assert call(level=16) == -1
        assert call(level=4, k0=200) == -1 and call(level=0, k0=-200) == -1
        assert call(dx=V(4098)) == -1 and b"4-byte aligned" in L.ndp_last_error()
    bad = LayerDesc(width=257).c_struct()
    assert L.ndp_level_bwd(ctypes.byref(bad), a, 4, -8, a, 100, a, a, a, None, a, a, 2, 1 << 20, None, a) == -2


def test_fixture_network_term_is_visible_at_k0_0(golden):
    """dx = direct term + network term.  A comparison relative to max |dx| only tests the network term (the new device code) where
    that term is a sizeable part of dx: every k0 = 0 case of F17 has max |network| >= 0.1 max |direct| (the capture script refuses
    to write one that does not), and the fixture holds exactly the cases the GPU test walks."""
    g = golden("F17_input_grad")
    assert list(g["cases"]) == [case_key(*c) for c in CASES]
    at0 = [c for c in CASES if c[2] == 0]
    assert len(at0) == 13
    for c in CASES:
        key = case_key(*c)
        share = float(g[f"{key}.share"])
        assert np.isfinite(g[f"{key}.dx"]).all() and g[f"{key}.dx"].shape == (256, 3)
        if c[2] == 0:
            assert share >= 0.1, (key, share)
        else:
            assert 0.0 < share < 0.2, (key, share)         # (the shipped k0: why k0 = 0 is captured at all)


def test_fixture_float32_reference_sits_well_inside_the_bar(golden):
    """The reference's own float32 autograd against its float64, in the measure the GPU tests use: below a tenth of the tighter bar
    (1e-4), so that the fixture's rounding cannot eat the margin of a comparison at 2e-4."""
    g = golden("F17_input_grad")
    worst = max(float(g[f"{case_key(*c)}.rel64"]) for c in CASES)
    worst = max(worst, float(g["joint.rel64"]), float(g["cd.full.rel64"]), float(g["cd.trunc.rel64"]))
    assert worst < 0.1 * BAR_F64, worst
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "F17_input_grad.npz")) <= 900 * 1024


def test_fitted_pyramid_needs_a_register_first():
    from deformationpyramid_amd.config import Config
    from deformationpyramid_amd.registration import Registration
    cfg = Config(deformation_model="NDP", device=torch.device("cpu"), depth=3, width=128, k0=-8, m=2, w_reg=0.0,
                 rotation_format="axis_angle", motion_type="SE3", samples=10, iters=5, lr=0.01, max_break_count=15,
                 break_threshold_ratio=0.001)
    model = Registration(cfg)
    with pytest.raises(RuntimeError, match="register"):
        model.fitted_pyramid()
    model.load_pcds(np.zeros((20, 3), np.float32), np.zeros((20, 3), np.float32))
    with pytest.raises(RuntimeError, match="register"):
        model.fitted_pyramid()


def test_pyramid_from_store_draws_no_random_numbers_and_shares_the_block():
    from deformationpyramid_amd.nets import Deformation_Pyramid
    torch.manual_seed(3)
    a = Deformation_Pyramid(depth=3, width=128, device="cpu", k0=-8, m=3, rotation_format="axis_angle", motion="SE3")
    before = torch.get_rng_state().clone()
    b = Deformation_Pyramid.from_store(a.store.clone(), 3, 128, -8, "axis_angle")
    assert torch.equal(torch.get_rng_state(), before)
    assert b.n_hierarchy == 3 and b.p_stride == a.p_stride and [d for d in b.descs] == [d for d in a.descs]
    for la, lb in zip(a.pyramid, b.pyramid):
        for (na, pa), (nb, pb) in zip(la.named_parameters(), lb.named_parameters()):
            assert na == nb and torch.equal(pa, pb) and pb.data_ptr() != pa.data_ptr()
    with torch.no_grad():
        b.store[1, 7] = 42.0
    assert next(iter(b.pyramid[1].parameters())).reshape(-1)[7].item() == 42.0 and a.store[1, 7].item() != 42.0
    with pytest.raises(ValueError):
        Deformation_Pyramid.from_store(a.store[:, :100].contiguous(), 3, 128, -8, "axis_angle")
