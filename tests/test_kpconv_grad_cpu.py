"""The KPConv backward without a GPU: the closed-form gradient of tests/_kpconv_grad_ref.py agrees with torch-double autograd of the
reference's op sequence, the ABI carries the new entries and their refusals, the workspace query keeps the slab bound, the
preconditions of the GPU cases of tests/test_kpconv_grad.py hold, and fixture F27 (the reference's own gradients) is reproduced."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native, kpfcn, ops
from tests import _kpconv_grad_ref as G
from tests import _kpfcn_ref as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndp_kpconv_backward_workspace", "ndp_kpconv_backward")
E_INVALID, E_UNSUPPORTED = -1, -2
MIB = 1 << 20


@pytest.fixture(scope="module")
def L():
    return _native.lib()


# ------------------------------------------------------------------------------------------ the restatement
def _autograd(c, idx, dy, normalize=None):
    T = lambda a: torch.from_numpy(np.asarray(a)).double()
    x, W = T(c.x).requires_grad_(True), T(c.W).requires_grad_(True)
    ns = c.s.shape[0]
    clean = torch.from_numpy(np.where((idx >= 0) & (idx < ns), idx, ns).astype(np.int64))
    y = G.t_kpconv(T(c.q), T(c.s), clean, x, W, T(c.kp), c.extent, c.influence, c.aggregation, c.normalize if normalize is None else normalize)
    (y * T(dy)).sum().backward()
    return y.detach().numpy(), x.grad.numpy(), W.grad.numpy()


@pytest.mark.parametrize("name", G.GRAD_CASES + ["exact", "c4_shadows"])
def test_closed_form_agrees_with_torch_double_autograd(name):
    c = K.make_case(name.replace("c4_shadows", "c4"))
    idx = G.shadow_table(c)[0] if name == "c4_shadows" else np.asarray(c.idx, np.int64)
    dy = G.case_dy(c)
    y, dx_t, dW_t = _autograd(c, idx, dy)
    dx, dW = G.kpconv_grad(c.q, c.s, idx, c.x, c.W, c.kp, c.extent, dy, c.influence, c.aggregation, c.normalize, np.float64)
    y64 = K.kpconv(c.q, c.s, idx, c.x, c.W, c.kp, c.extent, c.influence, c.aggregation, c.normalize, np.float64)
    for what, mine, theirs in (("y", y64, y), ("dx", dx, dx_t), ("dW", dW, dW_t)):
        err, mag = float(np.abs(mine - theirs).max()), float(np.abs(theirs).max())
        assert err <= 1e-12 * max(mag, 1.0), (name, what, err, mag)


# ------------------------------------------------------------------------------------------ the ABI
def test_abi_carries_the_entries(L):
    assert L.ndp_version() == 219 and _native.ABI_VERSION == 215
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    versions = open(os.path.join(_native.CSRC, "ndp_abi_common.inc")).read()
    assert "//   219: " + ", ".join(ENTRIES) in versions
    for entry in ENTRIES:
        assert entry in _native._SIGS and entry in _native.EXPORTS and getattr(L, entry)
        decl = re.search(r"\bint " + entry + r"\(([^;]*?)\);", header, re.S)
        assert decl, entry
        assert len(decl.group(1).split(",")) == len(_native._SIGS[entry]), entry          # header and ctypes table agree on the arity
    names = list(_native._SIGS)
    assert names.index(ENTRIES[0]) == names.index("ndp_kpconv_forward") + 1 and names.index(ENTRIES[1]) == names.index(ENTRIES[0]) + 1


def _buffers():
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    return buf, p, ctypes.c_void_p(p.value + 1)


def test_entries_refuse_bad_arguments(L):
    """every refusal is decided before the first HIP call: the made-up device pointers are never followed"""
    buf, p, odd = _buffers()
    big = 1 << 40

    def bwd(q=p, s=p, idx=p, x=p, W=p, kp=p, dy=p, nq=65, ns=70, H=17, K=15, cin=65, cout=33, extent=0.02, influence=1, aggregation=0,
            normalize=1, slab=0, ws=p, ws_bytes=big, dx=p, dW=p):
        return L.ndp_kpconv_backward(q, s, idx, x, W, kp, dy, nq, ns, H, K, cin, cout, extent, influence, aggregation, normalize, slab, ws,
                                     ws_bytes, dx, dW, None)

    def size(nq=65, ns=70, H=17, K=15, cin=65, cout=33, slab=0, **_):
        n = ctypes.c_longlong(-1)
        return L.ndp_kpconv_backward_workspace(nq, ns, H, K, cin, cout, slab, ctypes.byref(n))

    need = ctypes.c_longlong()
    assert L.ndp_kpconv_backward_workspace(65, 70, 17, 15, 65, 33, 0, ctypes.byref(need)) == 0 and need.value % 16 == 0
    invalid = [(dict([(name, None)]), b"null") for name in ("q", "s", "idx", "x", "W", "kp", "dy", "ws")]
    invalid += [(dict([(name, odd)]), b"aligned") for name in ("q", "s", "idx", "x", "W", "kp", "dy", "dx", "dW", "ws")]
    invalid += [(dict(dx=None, dW=None), b"both null"), (dict(slab=8), b"slab_queries"), (dict(slab=-16), b"slab_queries"),
                (dict(slab=24), b"slab_queries"), (dict(slab=1 << 20), b"slab_queries"), (dict(ws_bytes=need.value - 1), b"workspace smaller"),
                (dict(extent=0.0), b"extent"), (dict(extent=float("nan")), b"extent"), (dict(influence=3), b"influence"),
                (dict(aggregation=2), b"aggregation"), (dict(normalize=2), b"normalize")]
    invalid += [(dict([(name, 0)]), b">= 1") for name in ("nq", "ns", "H", "K", "cin", "cout")]
    for kw, word in invalid:
        assert bwd(**kw) == E_INVALID, kw
        assert word in L.ndp_last_error() and b"ndp_kpconv_backward" in L.ndp_last_error(), (kw, L.ndp_last_error())
    for kw in (dict(K=33), dict(H=65), dict(cin=1025), dict(cout=1025), dict(nq=(1 << 30) + 1), dict(ns=(1 << 30) + 1), dict(nq=1 << 30, H=2)):
        assert bwd(**kw) == E_UNSUPPORTED and b"served are" in L.ndp_last_error(), (kw, L.ndp_last_error())
        assert size(**kw) == E_UNSUPPORTED, kw
    assert size(slab=8) == E_INVALID and size(nq=0) == E_INVALID
    assert L.ndp_kpconv_backward_workspace(65, 70, 17, 15, 65, 33, 0, None) == E_INVALID


def test_workspace_keeps_the_slab_bound(L):
    """the slab buffer is at most 64 MiB; next to it only O(Nq H + Ns) integers (flags, counts, keys, values, sort storage, row starts)"""
    for nq, H, cin in ((20000, 32, 64), (1000000, 64, 1024)):
        n = ctypes.c_longlong()
        assert L.ndp_kpconv_backward_workspace(nq, nq, H, 15, cin, cin, 0, ctypes.byref(n)) == 0
        edges = nq * H
        integers = 4 * (10 * edges + 2 * nq + nq + 1) + MIB                               # 4 E keys / values, 6 E + 256 KiB sort storage, flags, row starts, counts
        assert n.value <= 64 * MIB + integers, (nq, H, cin, n.value)
        assert n.value >= min(64 * MIB, nq * H * cin * 4) // 2                            # and the slab is there
        small = ctypes.c_longlong()
        assert L.ndp_kpconv_backward_workspace(nq, nq, H, 15, cin, cin, 16, ctypes.byref(small)) == 0 and small.value <= n.value


def test_wrappers_refuse_bad_arguments():
    q, x, W, kp = torch.zeros(5, 3), torch.zeros(5, 4), torch.zeros(15, 4, 6), torch.zeros(15, 3)
    idx, dy = torch.zeros(5, 7, dtype=torch.int64), torch.zeros(5, 6)
    for a in (dict(dy=torch.zeros(5, 5)), dict(dy=None), dict(need_dx=False, need_dw=False), dict(slab_queries=8), dict(slab_queries=-16),
              dict(influence="cubic"), dict(x=torch.zeros(4, 4)), dict(idx=idx.float())):
        kw = dict(q=q, s=q, idx=idx, x=x, weights=W, kernel_points=kp, extent=0.02, dy=dy)
        kw.update(a)
        with pytest.raises(ValueError):
            ops.kpconv_bwd(**kw)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.kpconv_bwd(q, q, idx, x, W, kp, 0.02, dy)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.kpconv_fn(q, q, idx, x.requires_grad_(True), W, kp, 0.02)
    for cls in (kpfcn.KPConv, kpfcn.SimpleBlock, kpfcn.ResnetBottleneckBlock, kpfcn.KPFCN):
        assert callable(cls.forward_grad)
    assert callable(kpfcn.train_step)


def test_trainable_parameters_freeze_what_the_coarse_phase_never_reaches():
    torch.manual_seed(0)
    net = kpfcn.KPFCN(K.F23_CONFIG)
    kept = kpfcn.trainable_parameters(net)
    frozen = [n for n, p in net.named_parameters() if not p.requires_grad]
    assert any(n.startswith("coarse_in.") for n in frozen) and any(n.startswith("fine_out.") for n in frozen)
    assert all(n.endswith("kernel_points") or n.startswith(("coarse_in.", "fine_out.", "decoder_blocks.")) for n in frozen)
    assert all(not n.startswith("decoder_blocks.1.") for n in frozen)
    assert len(kept) == sum(p.requires_grad for p in net.parameters()) and any(p is net.coarse_out.weight for p in kept)


# ------------------------------------------------------------------------------------------ the GPU cases' preconditions
def test_gpu_cases_meet_their_preconditions():
    c = K.make_case("c6_strided")
    idx, ns = np.asarray(c.idx, np.int64), c.s.shape[0]
    holes = G.holes_table(c)                                                              # as generated the case references all of its supports
    assert sorted(G.unreferenced_rows(holes, ns).tolist()) == sorted(G.HOLE_ROWS)         # rows nobody references: dx must be +0 there
    assert (np.isin(idx, G.HOLE_ROWS).sum(1) > 0).sum() >= 2 and ((holes != idx).sum() < idx.size // 20)
    tiles = [set((np.nonzero((idx == r).any(1))[0] // 16).tolist()) for r in range(ns)]
    assert max(len(t) for t in tiles) >= 2                                                # a row with edges from two or more query tiles
    assert idx.shape[0] > 64                                                              # slab_queries = 16 and 64 both cut it
    c5 = K.make_case("c5")
    assert c5.q.shape[0] == 129                                                           # 129 queries: nine tiles, slabs of 16 and 64 end inside
    c4 = K.make_case("c4")
    bad, clean = G.shadow_table(c4)
    ns4 = c4.s.shape[0]
    shadow = (bad < 0) | (bad >= ns4)
    assert shadow[2].all() and bad[3, 0] == bad[3, 1] and 0 <= bad[3, 0] < ns4
    assert shadow.mean() >= 1 / 3 and {int(v) for v in np.unique(bad[shadow])} == {ns4, -1, 2 ** 31 - 1}
    assert np.array_equal(clean[~shadow], bad[~shadow]) and (clean[shadow] == ns4).all()
    assert G.unreferenced_rows(bad, ns4).size >= 1                                        # rows only shadows "reference"
    ex = K.make_case("exact")
    dy = G.case_dy(ex, integer=True)
    dx64, dW64 = G.kpconv_grad(ex.q, ex.s, ex.idx, ex.x, ex.W, ex.kp, ex.extent, dy, ex.influence, ex.aggregation, False, np.float64)
    assert np.array_equal(dx64, dx64.astype(np.float32)) and np.array_equal(dW64, dW64.astype(np.float32))    # the exact case is exact in float32
    assert np.abs(dx64).max() < 2 ** 20 and np.abs(dW64).max() < 2 ** 20


# ------------------------------------------------------------------------------------------ fixture F27
def test_fixture_f27_is_reproduced_by_the_restatement():
    """the reference's own KPConv under torch double autograd against the closed form, to 1e-12 relative"""
    z = G.load_f27()
    batch, f23 = K.load_f23()
    assert os.path.getsize(G.F27) <= os.path.getsize(K.F23)
    r0 = K.F23_CONFIG["first_subsampling_dl"] * K.F23_CONFIG["conv_radius"]
    extent = r0 * K.F23_CONFIG["KP_extent"] / K.F23_CONFIG["conv_radius"]
    for i, (influence, aggregation, strided) in enumerate(K.F23_CONVS):
        q, s, idx = K._tables(batch, 0, strided)
        x, W, kp, dy = (z[f"a{i}.{k}"].astype(np.float32) for k in ("x", "weights", "kernel_points", "dy"))
        dx, dW = G.kpconv_grad(q, s, idx, x, W, kp, extent, dy, influence, aggregation, True, np.float64)
        for what, mine in (("dx", dx), ("dW", dW)):
            ref = z[f"a{i}.{what}64"]
            assert np.abs(mine - ref).max() <= 1e-12 * max(1.0, np.abs(ref).max()), (i, what)
            assert np.abs(z[f"a{i}.{what}32"] - ref).max() <= 1e-3 * max(1.0, np.abs(ref).max())
    sd = K.state_dict(z, "b2.sd.")
    P = G.t_params(sd, torch.float64)
    x = torch.from_numpy(z["b2.x"].astype(np.float64)).requires_grad_(True)
    out = G.t_resnet_block(P, "", x, G.t_batch(batch, torch.float64), 0, True, K.F23_CONFIG)
    (out * torch.from_numpy(z["b2.dy"].astype(np.float64))).sum().backward()
    names = sorted(k[len("b2.grad64."):] for k in z.files if k.startswith("b2.grad64."))
    assert names == sorted(["x"] + [k for k, v in P.items() if v.requires_grad])
    for name in names:
        mine = (x.grad if name == "x" else P[name].grad).numpy()
        ref = z[f"b2.grad64.{name}"]
        assert np.abs(mine - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), name
