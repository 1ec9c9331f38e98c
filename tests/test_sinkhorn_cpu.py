"""Sinkhorn baseline, everything that needs no GPU: the ABI's host side (schedule, workspace, argument checks), the shipped config,
the dispatch, and the float64 restatement (tests/_sinkhorn_ref.py) that tests/test_sinkhorn.py holds the kernels to."""
import ctypes
import math
import os

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native as N
from tests import _sinkhorn_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("ndp_sinkhorn_schedule", "ndp_sinkhorn_workspace", "ndp_sinkhorn_divergence")
# (diameter, blur, scaling) -> entries of the epsilon schedule
SCHEDULES = [(1.668, 0.1, 0.5, 7), (0.377, 0.1, 0.5, 4), (1.663, 0.01, 0.5, 10), (1.660, 0.1, 0.9, 29)]


def c_schedule(diameter, blur, scaling, cap=256):
    out = (ctypes.c_double * max(cap, 1))()
    cnt = N.lib().ndp_sinkhorn_schedule(diameter, blur, scaling, out, cap)
    return cnt, list(out[:max(0, min(cnt, cap))])


def test_abi_carries_the_sinkhorn_entries():
    L = N.lib()
    assert L.ndp_version() >= 209
    for name in NAMES:
        assert name in N._SIGS and name in N.EXPORTS
        assert getattr(L, name) is not None
    assert "ndp_sinkhorn.inc" in N.HEADERS                      # part of the build id


@pytest.mark.parametrize("diameter,blur,scaling,entries", SCHEDULES)
def test_schedule_lengths_and_ends(diameter, blur, scaling, entries):
    from deformationpyramid_amd.sinkhorn import epsilon_schedule
    py = epsilon_schedule(diameter, blur, scaling)
    cnt, c = c_schedule(diameter, blur, scaling)
    assert cnt == entries == len(py)
    assert c == py                                              # both in double, the same operations
    assert py[0] == diameter * diameter and py[-1] == blur * blur
    assert all(a > b for a, b in zip(py[1:-1], py[2:-1]))       # the arange part decreases
    np.testing.assert_allclose(py, R.schedule(diameter, blur, scaling), rtol=1e-14)     # the helper's numpy arange


def test_schedule_edges():
    from deformationpyramid_amd.sinkhorn import epsilon_schedule
    for diameter in (0.1, 0.05):                                # diameter <= blur: the arange part is empty
        assert epsilon_schedule(diameter, 0.1, 0.5) == [diameter * diameter, 0.1 * 0.1]
        assert c_schedule(diameter, 0.1, 0.5) == (2, [diameter * diameter, 0.1 * 0.1])
    cnt, head = c_schedule(1.668, 0.1, 0.5, cap=3)              # a short buffer gets the head, the count is the whole schedule's
    assert cnt == 7 and head == epsilon_schedule(1.668, 0.1, 0.5)[:3]
    assert N.lib().ndp_sinkhorn_schedule(1.668, 0.1, 0.5, None, 0) == 7
    for bad in ((0.0, 0.1, 0.5), (-1.0, 0.1, 0.5), (math.inf, 0.1, 0.5), (math.nan, 0.1, 0.5), (1.0, 0.0, 0.5), (1.0, 0.1, 0.0),
                (1.0, 0.1, 1.0), (1.0, 0.1, 1.5)):
        assert c_schedule(*bad)[0] == -1
        with pytest.raises(ValueError):
            epsilon_schedule(*bad)


def test_workspace_formula():
    L = N.lib()
    nf = ctypes.c_longlong()
    for n, m in ((1, 1), (16, 17), (2000, 1999), (63, 4000), (1 << 20, 3)):
        assert L.ndp_sinkhorn_workspace(n, m, ctypes.byref(nf)) == 0
        assert nf.value == 4 * ((max(n, m) + 15) // 16) + 4 * (n + m)
    assert L.ndp_sinkhorn_workspace(0, 5, ctypes.byref(nf)) == -1
    assert L.ndp_sinkhorn_workspace(5, 0, ctypes.byref(nf)) == -1
    assert L.ndp_sinkhorn_workspace(5, 5, None) == -1


def test_divergence_refuses_bad_arguments_before_touching_the_device():
    L = N.lib()
    p = ctypes.c_void_p(64)                                     # never dereferenced: every call below is refused on the host

    def call(n=8, m=8, blur=0.1, reach=1.0, scaling=0.5, diameter=1.0, x=p, y=p, ws=p, loss=p):
        return L.ndp_sinkhorn_divergence(x, n, y, m, blur, reach, scaling, diameter, ws, loss, None, None, None)

    for kw in (dict(n=0), dict(m=0), dict(n=-3), dict(blur=0.0), dict(blur=-0.1), dict(blur=math.nan), dict(scaling=0.0),
               dict(scaling=1.0), dict(scaling=-0.5), dict(scaling=math.nan), dict(diameter=0.0), dict(diameter=-1.0),
               dict(diameter=math.inf), dict(diameter=math.nan), dict(reach=math.nan), dict(reach=math.inf),
               dict(x=None), dict(y=None), dict(ws=None), dict(loss=None), dict(ws=ctypes.c_void_p(68))):
        assert call(**kw) == -1, kw
        assert b"ndp_sinkhorn" in L.ndp_last_error()
    assert call(blur=1e-3, scaling=0.99, diameter=1e3) == -2    # 2 ln(1e6) / (2 |ln 0.99|) entries: beyond the cap of 256
    assert b"256" in L.ndp_last_error()


def test_shipped_config_and_dispatch():
    from deformationpyramid_amd.config import Config, load_config
    from deformationpyramid_amd.registration import Registration
    c = load_config(os.path.join(ROOT, "config", "baselines", "Sinkhorn.yaml"), device=torch.device("cpu"))
    assert c.deformation_model == "Sinkhorn" and c.gpu_mode is True
    assert (c.samples, c.blur, c.reach, c.Nsteps, c.lr) == (2000, 0.1, 1, 11, 1)
    assert c.folder == "Sinkhron" and c.exp_dir == "blur_0.1_reach_1" and c.snapshot_dir == "snapshot/Sinkhron/blur_0.1_reach_1"
    model = Registration(c)
    model.load_pcds(np.zeros((20, 3), np.float32), np.ones((20, 3), np.float32))
    with pytest.raises(N.NdpError, match="Sinkhorn.*GPU only"):  # served, on the GPU only: the package's error, which names the reason,
        model.register()                                        # not a bare KeyError("Sinkhorn")
    with pytest.raises(N.NdpError, match="GPU only"):           # the same before any cloud is loaded
        Registration(c).register()
    with pytest.raises(NotImplementedError):
        model.register(visualize=True)
    with pytest.raises(KeyError, match="not served"):           # an unknown model: a failed lookup, as ever, and an NdpError too
        Registration(Config(c, deformation_model="Lepard+NICP")).register()
    assert issubclass(N.NdpUnservedError, N.NdpError) and issubclass(N.NdpUnservedError, KeyError)
    assert str(N.NdpUnservedError("plain message")) == "plain message"
    from deformationpyramid_amd import ops
    with pytest.raises(N.NdpError):
        ops.sinkhorn_divergence(torch.zeros(4, 3), torch.ones(4, 3), 0.1)


# ---------------------------------------------------------------------------------- the float64 restatement pins itself
def test_reference_vanishes_on_equal_clouds():
    x, _ = R.box_clouds(50, 1, 0)
    for reach in (None, 1.0):
        r = R.sinkhorn_ref(x, x.clone(), 0.1, reach)
        assert abs(float(r.loss)) <= 1e-15 and float(r.grad.abs().max()) <= 1e-15      # float64 round-off of potentials of order 0.1


@pytest.mark.parametrize("reach", [None, 0.3])
def test_reference_gradient_is_autograd_through_the_extrapolation(reach):
    x, y = R.box_clouds(40, 55, 1)
    r = R.sinkhorn_ref(x, y, 0.1, reach)
    xg = x.double().requires_grad_(True)
    loss = R.extrapolation_loss(xg, y.double(), r)
    assert abs(float(loss.detach()) - float(r.loss)) <= 1e-15
    (g,) = torch.autograd.grad(loss, [xg])
    assert float((g * r.backward_scale - r.grad).abs().max()) <= 1e-15
    assert (r.backward_scale == 1.0) == (reach is None)


def test_reference_euler_loop_registers_a_shifted_cloud():
    x, _ = R.box_clouds(200, 1, 2)
    y = x + 0.1
    out = R.euler(x, y, 0.1, 1.0, nsteps=11, lr=1)
    assert float((out - y.double()).norm(dim=1).mean()) < 0.01
