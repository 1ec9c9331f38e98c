"""The three comparison baselines' kernels -- csrc/ndp_nerfies.inc, csrc/ndp_ed.inc, csrc/ndp_flow_metrics.inc -- on the GPU against the
float64 restatements of tests/_baselines_ref.py, at the sizes where a tile, a block or a strided loop ends: every tensor at the project's
bar -- max(4 x the eager float32 restatement's error, 16 float32 ulps of the largest magnitude) --, bit for bit where the arithmetic
promises it.  Every accuracy case prints error / bar before it asserts (profiles/baselines_accuracy.txt is that output).  What the inputs
are built to satisfy (no ReLU within the kink margin, no row at a threshold, -1 slots and every phi class present) is asserted in
tests/test_baselines_cpu.py.

Two cases of the issue are narrower here because they cannot exist: an ED batch of S = 0 points has no anchor slot, so only its -1 edge
slots are made loud; a flow case of n = 1 is one ordinary row, without the ten special rows (they are in every case of n >= 1023)."""
import functools

import numpy as np
import pytest
import torch

from deformationpyramid_amd import nerfies as NF
from deformationpyramid_amd import ops
from deformationpyramid_amd.ed import EDGraph
from deformationpyramid_amd.loss import compute_flow_metrics
from tests import _baselines_ref as B

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return None if a is None else a.contiguous().to(DEV)


def check(what, got, ref64, ref32):
    got, ref64, ref32 = (np.asarray(torch.as_tensor(a).detach().cpu().double()) for a in (got, ref64, ref32))
    assert got.shape == ref64.shape == ref32.shape and np.isfinite(got).all() and np.isfinite(ref64).all(), what
    err, err32, mag = (float(np.abs(a).max()) if a.size else 0.0 for a in (got - ref64, ref32 - ref64, ref64))
    bar = B.bar(err32, mag)
    print(f"{what}: error {err:.3e}  bar {bar:.3e}  (eager float32 {err32:.3e}, magnitude {mag:.3e})  error / bar {err / bar if bar else 0.0:.3f}")
    assert err <= bar, what


# ------------------------------------------------------------------------------------------ Nerfies
@functools.lru_cache(maxsize=None)
def nerfies_refs(kind, n, it):
    """inputs and both restatements, computed once and shared; nothing below writes to them"""
    x, gy = B.kink_free_points(kind, n, it)[0], B.upstream_gradient(n)
    return (x, gy) + B.nerfies_pair(B.nerfies_flat(kind), x, it, gy)


def forward_case(kind, n, it):
    x, _, r64, r32 = nerfies_refs(kind, n, it)
    flat, xd = dev(B.nerfies_flat(kind)), dev(x)
    warped, J, reg, saved = NF.nerfies_fwd(flat, xd, it, B.MAX_ITER, save=True)
    tag = f"nerfies fwd {kind} n={n} it={it}"
    check(f"{tag} pe", saved[1][:n, :39], r64.pe, r32.pe)
    check(f"{tag} warped", warped, r64.warped, r32.warped)
    check(f"{tag} J", J, r64.J, r32.J)
    check(f"{tag} reg", reg[0], r64.reg, r32.reg)
    w2, J2, reg2 = NF.nerfies_fwd(flat, xd, it, B.MAX_ITER)                     # inference form: two ping-pong planes
    assert torch.equal(w2, warped) and torch.equal(J2, J) and torch.equal(reg2, reg)
    w3, J3, reg3, _ = NF.nerfies_fwd(flat, xd, it, B.MAX_ITER, save=True)
    assert torch.equal(w3, warped) and torch.equal(J3, J) and torch.equal(reg3, reg)


@pytest.mark.parametrize("n,it", B.NERFIES_FWD_CASES)
def test_nerfies_forward_loud_weights(n, it):
    forward_case("loud", n, it)


def test_nerfies_forward_default_init():
    """The workload's regime: J is within 0.2 of the identity."""
    forward_case("default", *B.NERFIES_DEFAULT_CASE)


def test_nerfies_forward_grid_stride():
    """514 tiles on k_nrf_dense's grid of 512: the tiles reached by the second trip of its loop, and the mean of 32833 terms."""
    x, rows = B.stride_case()
    n, flat = x.shape[0], B.nerfies_flat("loud")
    warped, J, reg = NF.nerfies_fwd(dev(flat), dev(x), 2999, B.MAX_ITER)
    r64, r32 = B.nerfies_pair(flat, x[rows], 2999)
    check(f"nerfies fwd loud n={n} it=2999 warped ({len(rows)} rows)", warped.cpu()[rows], r64.warped, r32.warped)
    check(f"nerfies fwd loud n={n} it=2999 J ({len(rows)} rows)", J.cpu()[rows], r64.J, r32.J)
    assert torch.isfinite(J).all() and torch.isfinite(warped).all()
    ref = B.regularization(J.cpu()).item()                                       # float64, on the kernel's own J: every row
    err, bound = abs(reg.item() - ref), 4 * B.ULP * ref
    print(f"nerfies fwd loud n={n} reg on the kernel's J: error {err:.3e}  bound {bound:.3e} (4 ulps of {ref:.6e})  error / bound {err / bound:.3f}")
    assert err <= bound


def test_nerfies_regulariser_on_a_pure_rotation():
    """J^T J = I up to rounding: a triple eigenvalue, where the closed form's p1 vanishes or its r is clamped."""
    n, flat = 65, B.nerfies_flat("rotation")
    x = B.upstream_gradient(n, seed=1)
    warped, J, reg = NF.nerfies_fwd(dev(flat), dev(x), 2999, B.MAX_ITER)
    r64, r32 = B.nerfies_pair(flat, x, 2999)
    check("nerfies fwd rotation n=65 warped", warped, r64.warped, r32.warped)
    check("nerfies fwd rotation n=65 J", J, r64.J, r32.J)
    print(f"nerfies fwd rotation n=65 reg {reg.item():.3e} (float64 on the kernel's J {B.regularization(J.cpu()).item():.3e})")
    assert np.isfinite(reg.item()) and 0.0 <= reg.item() <= 1e-10


@pytest.mark.parametrize("n,n_part", B.NERFIES_BWD_CASES)
def test_nerfies_backward(n, n_part):
    it = B.NERFIES_BWD_IT
    x, gy, r64, r32 = nerfies_refs("loud", n, it)
    flat, xd, gd = dev(B.nerfies_flat("loud")), dev(x), dev(gy)
    net = NF.Nerfies_Deformation(max_iter=B.MAX_ITER)

    def run(poison=False):
        saved = NF.nerfies_fwd(flat, xd, it, B.MAX_ITER, save=True)[3]
        if poison:                                                               # the saved posenc's padding rows: the forward leaves posenc(0)
            saved[1][n:] = float("nan")                                          # there, and upstream's dz rows of padding are zero, so only
        return NF.nerfies_bwd(flat, xd, saved, gd, n_part=n_part)               # a NaN shows a padding row that was multiplied in

    got = run()
    assert got.shape == (NF.PARAM_COUNT,) == r64.grad.shape
    for (name, _), g, g64, g32 in zip(net.named_parameters(), net.split_like(got), net.split_like(r64.grad), net.split_like(r32.grad)):
        check(f"nerfies bwd n={n} n_part={n_part} {name}", g, g64, g32)
    assert torch.equal(run(), got)
    assert torch.equal(run(poison=True), got)                                    # a row of padding does not contribute


# ------------------------------------------------------------------------------------------ embedded deformation
def ed_graph_on_device(c):
    return EDGraph(dev(c.nodes), dev(c.edges), dev(c.edge_w))


@pytest.mark.parametrize("S", B.ED_S)
@pytest.mark.parametrize("loud", [False, True], ids=["zero_slots", "loud_slots"])
@pytest.mark.parametrize("tag", B.ED_GRAPHS)
def test_ed_warp_arap_and_gradients(tag, loud, S):
    c = B.ed_case(tag, S, loud)
    graph = ed_graph_on_device(c)
    params = dev(torch.cat([c.phi.reshape(-1), c.t.reshape(-1)]))
    x, a, w, gy = dev(c.x), dev(c.anchors.to(torch.int32)), dev(c.weights), dev(c.gy)
    y = graph.warp(params, x, a, w)
    arap = graph.arap(params).clone()
    for w_arap in B.ED_W_ARAP:
        r64, r32 = B.ed(torch.float64, c, w_arap), B.ed(torch.float32, c, w_arap)
        tagline = f"ed {tag} ({c.n} nodes) S={S} {'loud' if loud else 'zero'} slots w_arap={w_arap}"
        gr = graph.grads(params, x, a, w, gy, w_arap)
        assert y.shape == (S, 3) and gr.shape == (6 * c.n,)
        check(f"{tagline} y", y, r64[0], r32[0])
        check(f"{tagline} arap", arap[0], r64[1], r32[1])
        check(f"{tagline} dphi", gr[:3 * c.n].view(c.n, 3), r64[2], r32[2])
        check(f"{tagline} dt", gr[3 * c.n:].view(c.n, 3), r64[3], r32[3])
        if S == 0 and w_arap == 0:
            assert not gr.any()
        assert torch.equal(graph.grads(params, x, a, w, gy, w_arap), gr)


@pytest.mark.parametrize("tag", B.ED_GRAPHS)
def test_ed_keep_R_warps_with_the_old_rotations_and_the_new_translations(tag):
    c = B.ed_case(tag, 257, True)
    graph = ed_graph_on_device(c)
    x, a, w = dev(c.x), dev(c.anchors.to(torch.int32)), dev(c.weights)
    phi2, t2 = B.ed_state(c.n, seed=4)
    assert not torch.equal(phi2, c.phi) and not torch.equal(t2, c.t)
    graph.warp(dev(torch.cat([c.phi.reshape(-1), c.t.reshape(-1)])), x, a, w)
    y = graph.warp(dev(torch.cat([phi2.reshape(-1), t2.reshape(-1)])), x, a, w, keep_R=True)
    r64, r32 = B.ed(torch.float64, c, 0.0, t=t2), B.ed(torch.float32, c, 0.0, t=t2)
    check(f"ed {tag} keep_R y", y, r64[0], r32[0])
    fresh = B.ed(torch.float64, c, 0.0, phi=phi2, t=t2)[0]
    assert (fresh - r64[0]).abs().max() > 1e-3                                   # the two states are told apart by far more than a bar


# ------------------------------------------------------------------------------------------ flow metrics
@pytest.mark.parametrize("mode", B.FLOW_OVERLAPS)
@pytest.mark.parametrize("n", B.FLOW_N)
def test_flow_metrics(n, mode):
    flow, gt, ov, _, _ = B.flow_case(n, mode)
    s64, s32 = B.flow_sums(flow.double(), gt.double(), ov), B.flow_sums(flow, gt, ov)
    sums = ops.flow_metrics(dev(flow), dev(gt), dev(ov))
    assert sums.shape == (3, 5) and sums.dtype == torch.float64
    assert torch.equal(sums[:, 1:], s64[:, 1:]), (sums, s64)                     # the twelve counts
    for s, name in enumerate(("all", "overlap", "rest")):
        check(f"flow metrics n={n} {mode} sum of errors ({name})", sums[s, 0], s64[s, 0], s32[s, 0])
    got, cpu = compute_flow_metrics(dev(flow), dev(gt), dev(ov)), compute_flow_metrics(flow, gt, ov)
    assert list(got) == list(cpu) and len(got) == (4 if ov is None else 12)
    for k, v in cpu.items():
        if np.isnan(v):
            assert np.isnan(got[k]), k
        else:
            assert abs(got[k] - v) < 1e-4 * max(1.0, abs(v)), k
    if mode == "all_true" or (mode == "mixed" and n == 1 and bool(ov[0])):
        assert np.isnan(got["occ-epe"]) and got["vis-epe"] == got["full-epe"]
    if mode == "all_false" or (mode == "mixed" and n == 1 and not bool(ov[0])):
        assert np.isnan(got["vis-epe"]) and got["occ-epe"] == got["full-epe"]
