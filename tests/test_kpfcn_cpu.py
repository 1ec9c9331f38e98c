"""KPConv convolution and KPFCN without a GPU: the ABI carries the two entries, the workspace query and every refusal that needs no
device, the numpy restatement (tests/_kpfcn_ref.py) against the reference's own modules (fixture F23), the default kernel points, and
the input preconditions of the GPU cases of tests/test_kpfcn.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native
from tests import _kpconv_ref as R
from tests import _kpfcn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndp_kpconv_forward_workspace", "ndp_kpconv_forward")
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    return _native.lib()


@pytest.fixture(scope="module")
def f23():
    return K.load_f23()


def test_abi_carries_the_entries(L):
    assert L.ndp_version() >= 214
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    for name in ENTRIES:
        assert name in _native._SIGS and name in _native.EXPORTS and getattr(L, name)
        assert f"int {name}(" in header
    assert "ndp_kpconv_conv.inc" in " ".join(_native.HEADERS)


def test_workspace_query_needs_no_device(L):
    nb = ctypes.c_longlong()
    assert L.ndp_kpconv_forward_workspace(20000, 20000, 32, 15, 64, 64, ctypes.byref(nb)) == 0
    assert nb.value % 16 == 0 and 4 * 20000 <= nb.value <= 4 * 20000 + 16          # the row flags, nothing that grows with Nq, H, K or C
    assert L.ndp_kpconv_forward_workspace(1, 1, 1, 1, 1, 1, ctypes.byref(nb)) == 0 and nb.value == 16
    assert L.ndp_kpconv_forward_workspace(1 << 30, 1 << 30, 64, 32, 1024, 1024, ctypes.byref(nb)) == 0
    assert L.ndp_kpconv_forward_workspace(5, 5, 4, 15, 8, 8, None) == E_INVALID
    for args in ((0, 5, 4, 15, 8, 8), (5, 0, 4, 15, 8, 8), (5, 5, 0, 15, 8, 8), (5, 5, 4, 0, 8, 8), (5, 5, 4, 15, 0, 8), (5, 5, 4, 15, 8, -1)):
        assert L.ndp_kpconv_forward_workspace(*args, ctypes.byref(nb)) == E_INVALID, args
    for args in (((1 << 30) + 1, 5, 4, 15, 8, 8), (5, (1 << 30) + 1, 4, 15, 8, 8), (5, 5, 65, 15, 8, 8), (5, 5, 4, 33, 8, 8),
                 (5, 5, 4, 15, 1025, 8), (5, 5, 4, 15, 8, 1025)):
        assert L.ndp_kpconv_forward_workspace(*args, ctypes.byref(nb)) == E_UNSUPPORTED, args
        assert b"ndp_kpconv_forward_workspace" in L.ndp_last_error()


def test_c_entry_refuses_bad_arguments(L):
    """every refusal that needs no device happens before the first HIP call: the pointers are never read"""
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    odd4, odd1 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 1)

    def fwd(q=p, s=p, idx=p, x=p, W=p, kp=p, nq=5, ns=6, H=4, K=15, cin=8, cout=8, extent=0.02, influence=1, aggregation=0,
            normalize=1, ws=p, ws_bytes=1 << 40, y=p):
        return L.ndp_kpconv_forward(q, s, idx, x, W, kp, nq, ns, H, K, cin, cout, extent, influence, aggregation, normalize, ws, ws_bytes, y, None)

    invalid = [(dict(extent=0.0), b"extent"), (dict(extent=-1.0), b"extent"), (dict(extent=float("nan")), b"extent"),
               (dict(extent=float("inf")), b"extent"), (dict(influence=-1), b"influence"), (dict(influence=3), b"influence"),
               (dict(aggregation=2), b"aggregation"), (dict(aggregation=-1), b"aggregation"), (dict(normalize=2), b"normalize"),
               (dict(ws=odd4), b"aligned"), (dict(ws_bytes=16), b"workspace smaller"), (dict(nq=0), b">= 1"), (dict(H=0), b">= 1"),
               (dict(K=0), b">= 1"), (dict(cin=0), b">= 1"), (dict(cout=0), b">= 1")]
    invalid += [(dict([(name, None)]), b"null") for name in ("q", "s", "idx", "x", "W", "kp", "ws", "y")]
    invalid += [(dict([(name, odd1)]), b"aligned") for name in ("q", "s", "idx", "x", "W", "kp", "y")]
    for kw, word in invalid:
        assert fwd(**kw) == E_INVALID, kw
        assert word in L.ndp_last_error(), (kw, L.ndp_last_error())
    for kw in (dict(nq=(1 << 30) + 1), dict(ns=(1 << 30) + 1), dict(H=65), dict(K=33), dict(cin=1025), dict(cout=1025)):
        assert fwd(**kw) == E_UNSUPPORTED, kw
        assert b"served are" in L.ndp_last_error()


def test_wrapper_refuses_bad_arguments():
    from deformationpyramid_amd import kpfcn, ops
    q, s = torch.zeros(5, 3), torch.zeros(6, 3)
    idx, x, W, kp = torch.zeros(5, 4, dtype=torch.int64), torch.zeros(6, 8), torch.zeros(15, 8, 8), torch.zeros(15, 3)
    for kw in (dict(idx=idx[:4]), dict(idx=idx.float()), dict(idx=idx[:, :0]), dict(x=x[:5]), dict(x=x[0]), dict(W=W[:, :7]), dict(W=W[0]),
               dict(kp=kp[:14]), dict(extent=0.0), dict(extent=float("nan")), dict(influence="cubic"), dict(aggregation="max"),
               dict(idx=torch.zeros(5, 65, dtype=torch.int64)), dict(W=torch.zeros(33, 8, 8), kp=torch.zeros(33, 3)),
               dict(x=torch.zeros(6, 1025), W=torch.zeros(15, 1025, 8)), dict(W=torch.zeros(15, 8, 1025)), dict(q=torch.zeros(5, 2))):
        a = dict(q=q, s=s, idx=idx, x=x, W=W, kp=kp, extent=0.02, influence="linear", aggregation="sum")
        a.update(kw)
        with pytest.raises(ValueError):
            ops.kpconv(a["q"], a["s"], a["idx"], a["x"], a["W"], a["kp"], a["extent"], a["influence"], a["aggregation"])
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.kpconv(q, s, idx, x, W, kp, 0.02)
    cfg = dict(K.F23_CONFIG)
    for bad in (dict(deformable=True), dict(modulated=True), dict(architecture=["simple", "resnetb_deformable"]),
                dict(architecture=["simple_equivariant"]), dict(architecture=["simple", "resnetb_invariant_strided"])):
        with pytest.raises(NotImplementedError):
            kpfcn.KPFCN({**cfg, **bad})
    with pytest.raises(NotImplementedError):
        kpfcn.KPConv(15, 3, 8, 8, 0.02, 0.025, deformable=True)
    with pytest.raises(NotImplementedError):
        kpfcn.KPFCN(cfg)({"features": torch.ones(3, 1)}, phase="fine")
    with pytest.raises(ValueError):
        kpfcn.block_decider("global_median", 0.025, 8, 16, 0, cfg)


def test_default_kernel_points():
    from deformationpyramid_amd import kpfcn
    for Kn, radius in ((1, 0.025), (2, 0.05), (15, 0.025), (16, 0.1), (32, 1.0)):
        a, b = kpfcn.default_kernel_points(Kn, radius), kpfcn.default_kernel_points(Kn, radius)
        assert a.dtype == torch.float32 and tuple(a.shape) == (Kn, 3) and torch.equal(a, b)             # deterministic
        assert torch.equal(a[0], torch.zeros(3))                                                          # the centre
        np.testing.assert_allclose(a.numpy(), K.default_kernel_points(Kn, radius), rtol=0, atol=2e-7 * radius)
        if Kn > 1:
            r = a[1:].double().norm(dim=1)
            assert abs(float(r.mean()) - 0.66 * radius) <= 1e-6 * radius
            assert float(torch.cdist(a.double(), a.double()).fill_diagonal_(1e9).min()) > 0.2 * radius      # no two coincide
    assert sum(p.numel() for p in kpfcn.KPFCN(K.F23_CONFIG).parameters()) == 96571


def test_fixture_is_small_and_complete(f23):
    assert os.path.getsize(K.F23) <= 900 * 1024
    batch, z = f23
    assert [p.shape[0] for p in batch["points"]] == [1200, 388, 113, 31]
    assert z["c.out"].shape == (113, 12) and z["c.out"].dtype == np.float32
    pyr = R.build_pyramid(batch["points"][0], batch["stack_lengths"][0], architecture=R.KPFCN, limits=R.PYRAMID_LIMITS, **R.LEPARD)
    for l in range(4):
        for key in ("neighbors", "pools", "upsamples"):
            assert np.array_equal(getattr(pyr, key)[l], batch[key][l]), (l, key)


def _report(what, got, ref64, ref32):
    err, err32, mag = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max()), float(np.abs(ref64).max())
    bar = R.bar(err32, mag)
    print(f"{what}: error {err:.3e}  eager float32 {err32:.3e}  magnitude {mag:.3e}  bar {bar:.3e}")
    return err, bar


def test_restatement_reproduces_the_reference_convs(f23):
    """The reference's float32 output against the float64 restatement, at the bar set by the float32 restatement."""
    batch, z = f23
    x = z["x8"].astype(np.float32)
    for i, (influence, aggregation, strided) in enumerate(K.F23_CONVS):
        q, s, inds = K._tables(batch, 0, strided)
        a = (q, s, inds, x, z[f"a{i}.weights"], z[f"a{i}.kernel_points"], K.EXTENT, influence, aggregation, True)
        err, bar = _report(f"F23 a{i} {influence}/{aggregation}{' strided' if strided else ''}", z[f"a{i}.out"], K.kpconv(*a, np.float64), K.kpconv(*a, np.float32))
        assert err <= bar


def test_restatement_reproduces_the_reference_blocks(f23):
    batch, z = f23
    for i, (name, cin, cout) in enumerate(K.F23_BLOCKS):
        sd, x = K.state_dict(z, f"b{i}.sd."), z[f"x{cin}"].astype(np.float32)
        fn = K.simple_block if "simple" in name else K.resnet_block
        y64, y32 = (fn(sd, "", x, batch, 0, "strided" in name, K.F23_CONFIG, dt) for dt in (np.float64, np.float32))
        assert y64.shape == z[f"b{i}.out"].shape
        err, bar = _report(f"F23 b{i} {name}", z[f"b{i}.out"], y64, y32)
        assert err <= bar


def test_restatement_reproduces_the_reference_network(f23):
    batch, z = f23
    sd = K.state_dict(z, "c.sd.")
    y64, y32 = (K.kpfcn_coarse(sd, batch, K.F23_CONFIG, dt) for dt in (np.float64, np.float32))
    assert y64.shape == (113, 12)
    assert float(np.abs(y64 - z["c.out64"]).max()) <= 1e-9 * float(np.abs(y64).max())          # double against the reference in double
    err, bar = _report("F23 coarse forward", z["c.out"], y64, y32)
    assert err <= bar


@pytest.mark.parametrize("name", sorted(K.CASES))
def test_gpu_case_preconditions(name):
    c = K.make_case(name)
    nq, ns, H, Kn, cin, cout = K.CASES[name][:6]
    assert c.q.shape == (nq, 3) and c.s.shape == (ns, 3) and c.idx.shape == (nq, H) and c.x.shape == (ns, cin) and c.W.shape == (Kn, cin, cout)
    assert c.idx.min() >= 0 and c.idx.max() <= ns and (c.idx < ns).any()
    if name == "exact":
        assert np.array_equal(c.x, np.round(c.x)) and np.abs(c.x).max() <= 4 and np.array_equal(c.W * 8, np.round(c.W * 8)) and np.abs(c.W).max() <= 2
        return
    x64 = c.x.astype(np.float64)
    assert (np.abs(x64.sum(1)) >= K.ROW_CLEARANCE * np.abs(x64).sum(1)).all()              # fp32 summation error at C <= 1024 is below 2^-13 of sum |x|
    if c.aggregation == "closest":
        _, d2, valid, _ = K.kpconv(c.q, c.s, c.idx, c.x, c.W, c.kp, c.extent, c.influence, c.aggregation, c.normalize, np.float32, want=True)
        assert K.closest_clearance(d2, valid) > K.CLOSEST_ULPS
