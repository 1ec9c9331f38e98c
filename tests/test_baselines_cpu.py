"""Preconditions of tests/test_baselines_edges.py, checked without a GPU: the restatements of tests/_baselines_ref.py reproduce the
fixtures and the oracles they restate, and the inputs they build meet the conditions the float32 / float64 comparison rests on
(no ReLU within the kink margin, no row at a metric's threshold, every class of edge input present).

Two conditions of the issue cannot hold at the smallest sizes and are asserted from the first size at which they can: an ED batch of
S = 0 points has no anchor slot at all (the -1 edge slots are still there), and a flow case of one row cannot hold twenty rows of each
outcome nor the ten special rows -- both are asserted for n >= 1023."""
import numpy as np
import pytest
import torch

from oracle import ed_ref as E
from oracle import nerfies_ref as O
from tests import _baselines_ref as B

NERFIES_INPUTS = sorted({("loud", n, it) for n, it in B.NERFIES_FWD_CASES} | {("loud", n, B.NERFIES_BWD_IT) for n, _ in B.NERFIES_BWD_CASES}
                        | {("default",) + B.NERFIES_DEFAULT_CASE})


def default_net():
    from deformationpyramid_amd.nerfies import Nerfies_Deformation
    torch.manual_seed(23)
    return Nerfies_Deformation(max_iter=5000)


# ------------------------------------------------------------------------------------------ Nerfies
@pytest.mark.parametrize("it", [0, 700, 2999])
def test_float32_restatement_reproduces_the_nerfies_fixture(golden, it):
    """F14 at the bounds tests/test_nerfies.py holds the oracle to.  The fixture's gradients are those of cd + 0.001 reg, reg constant:
    the Chamfer gradient in the warped points is taken from the oracle's Chamfer and handed to the restatement as gy."""
    g = golden("F14_nerfies")
    net = default_net()
    x, y = torch.from_numpy(g["fb.x"]), torch.from_numpy(g["fb.y"])
    leaf = B.nerfies(net.flat, x, it).warped.clone().requires_grad_(True)
    cd = O.chamfer_l1(leaf, y)
    cd.backward()
    r = B.nerfies(net.flat, x, it, gy=leaf.grad)
    np.testing.assert_allclose(r.pe.numpy(), g[f"fb{it}.pe"], rtol=0, atol=2e-6)
    np.testing.assert_allclose(r.warped.numpy(), g[f"fb{it}.warped"], rtol=0, atol=2e-5)
    np.testing.assert_allclose(r.J.numpy(), g[f"fb{it}.J"], rtol=0, atol=2e-4)
    assert abs(r.reg.item() - float(g[f"fb{it}.reg"])) < 1e-3 * float(g[f"fb{it}.reg"]) + 1e-9
    assert abs(cd.item() - float(g[f"fb{it}.cd"])) < 2e-6 * float(g[f"fb{it}.cd"])
    flat_grad = torch.zeros_like(net.flat)
    flat_grad[:B.P_COUNT] = r.grad
    for (k, _), gr in zip(net.named_parameters(), net.split_like(flat_grad)):
        ref = g[f"fb{it}.grad.{k}"].reshape(-1)
        got = gr.numpy().reshape(-1)
        got = got if got.size <= 4992 else got[::37]
        assert np.abs(got - ref).max() < 2e-4 * (np.abs(ref).max() + 1e-12) + 1e-9, k
        assert abs(gr.numpy().astype(np.float64).sum() - float(g[f"fb{it}.gsum.{k}"])) < 1e-3 * float(g[f"fb{it}.gabs.{k}"]) + 1e-9, k


@pytest.mark.parametrize("kind,n,it", [("default", 200, 2999), ("default", 200, 700), ("loud", 65, 2999)])
def test_float32_restatement_agrees_with_the_oracle(golden, kind, n, it):
    """oracle/nerfies_ref.forward is another float32 evaluation of the same network: it is held to the project's bar around float64."""
    flat = B.nerfies_flat(kind)
    x = torch.from_numpy(golden("F14_nerfies")["fb.x"]) if kind == "default" else B.kink_free_points(kind, n, it)[0]
    r64, r32 = B.nerfies_pair(flat, x, it)
    warped, J, pe = O.forward(flat[:O.P_COUNT], x, it, 5000)
    assert O.P_COUNT == B.P_COUNT
    for what, mine, theirs, ref in (("pe", r32.pe, pe, r64.pe), ("warped", r32.warped, warped.detach(), r64.warped), ("J", r32.J, J, r64.J)):
        err32, mag = float((mine.double() - ref).abs().max()), float(ref.abs().max())
        assert float((theirs.double() - ref).abs().max()) <= B.bar(err32, mag), what
        assert float((theirs - mine).abs().max()) <= B.bar(err32, mag), what
    assert abs(O.regularization(J).item() - r32.reg.item()) <= 1e-5 * r32.reg.item()


@pytest.mark.parametrize("kind,n,it", NERFIES_INPUTS, ids=lambda v: str(v))
def test_nerfies_inputs_are_kink_free(kind, n, it):
    x, candidates, dropped = B.kink_free_points(kind, n, it)
    assert x.shape == (n, 3) and x.dtype == torch.float32 and x.abs().max() <= 0.5
    assert dropped <= 0.15 * candidates
    r64, r32 = B.nerfies_pair(B.nerfies_flat(kind), x, it)
    assert len(r64.zs) == 7 and all(z.shape == (n, 128) for z in r64.zs)
    for z64, z32 in zip(r64.zs, r32.zs):
        assert z64.abs().min() > B.KINK_MARGIN
        assert torch.equal(z64 > 0, z32 > 0)
        assert (z32.double() - z64).abs().max() < B.KINK_MARGIN / 10            # the margin is an order above float32's own z error


def test_nerfies_loud_weights_are_loud():
    """What the stated factors buy: rotations of about half a radian and a Jacobian far from the identity."""
    x, _, _ = B.kink_free_points("loud", 257, 2999)
    r = B.nerfies(B.nerfies_flat("loud").double(), x.double(), 2999)
    angle = r.o[:, :3].norm(dim=1)
    assert angle.min() > 0.4 and angle.max() < 0.8
    assert (r.J - torch.eye(3, dtype=torch.float64)).abs().median() > 0.3
    quiet = B.nerfies(B.nerfies_flat("default").double(), x.double(), 2999)
    assert (quiet.J - torch.eye(3, dtype=torch.float64)).abs().median() < 0.05


def test_nerfies_stride_case_rows_are_kink_free():
    x, rows = B.stride_case()
    assert x.shape[0] == 512 * 64 + 65 and (x.shape[0] + 63) // 64 == 514                # two tiles past a grid of 512, the last partial
    assert (rows < 64).sum() >= 48 and (rows >= 512 * 64).sum() >= 48 and (rows >= 513 * 64).any()
    r64, r32 = B.nerfies_pair(B.nerfies_flat("loud"), x[rows], 2999)
    assert all(torch.equal(a > 0, b > 0) for a, b in zip(r64.zs, r32.zs))


def test_nerfies_rotation_weights_give_a_pure_rotation():
    x = B.upstream_gradient(65, seed=1)
    r = B.nerfies(B.nerfies_flat("rotation").double(), x.double(), 2999)
    assert abs(float(r.o[0, :3].norm()) - 0.7) < 1e-6
    assert (r.J.transpose(1, 2) @ r.J - torch.eye(3, dtype=torch.float64)).abs().max() < 1e-14 and r.reg.item() < 1e-24


# ------------------------------------------------------------------------------------------ embedded deformation
def test_ed_wrapper_agrees_with_the_oracle():
    c = B.ed_case("g", 600, False)
    phi_r, t_r = c.phi.clone().requires_grad_(True), c.t.clone().requires_grad_(True)
    Rm = E.axis_angle_to_matrix(phi_r)
    y = E.ed_warp(c.x, c.anchors, c.weights, c.nodes, Rm, t_r)
    ar = E.arap(Rm, t_r, c.nodes, c.edges, c.edge_w)
    ((y * c.gy).sum() + 0.5 * ar).backward()
    got = B.ed(torch.float32, c, 0.5)
    for a, b in zip(got, (y.detach(), ar.detach(), phi_r.grad, t_r.grad)):
        assert a.dtype == torch.float32 and torch.equal(a, b)
    assert all(v.dtype == torch.float64 for v in B.ed(torch.float64, c, 0.5))


@pytest.mark.parametrize("tag", B.ED_GRAPHS)
def test_ed_cases_hold_every_class_of_input(golden, tag):
    g = golden("F15_embedded_deformation")
    G = B.ed_graph(tag)
    n = G.nodes.shape[0]
    np.testing.assert_array_equal(G.nodes.numpy(), g[f"{tag}.graph_nodes"])
    assert n == {"g": 129, "gr": 378}[tag] and (G.edges < 0).any() and (G.edge_w[G.edges < 0] == 0).all()
    assert (G.weights[G.anchors < 0] == 0).all() and G.anchors.max() < n and G.edges.max() < n and G.anchors.min() == -1 == G.edges.min()
    for S in B.ED_S:
        for loud in (False, True):
            c = B.ed_case(tag, S, loud)
            assert c.x.shape == (S, 3) and (S == 0 or (c.anchors < 0).any())
            if loud:
                assert (c.weights[c.anchors < 0] == B.ED_LOUD_ANCHOR).all() and (c.edge_w[c.edges < 0] == B.ED_LOUD_EDGE).all()
            norm = c.phi.double().norm(dim=1)
            for k, mag in B.ED_PHI_CLASSES.items():
                assert len(norm[k::7]) >= 18 and (norm[k::7] - mag).abs().max() <= 1e-6 * mag
            assert (c.phi[0::7] == 0).all() and (norm[1::7] < 1e-6).all() and (norm[2::7] > 1e-6).all() and (norm[2::7] < 1e-5).all()
            rest = torch.cat([c.phi[5::7], c.phi[6::7]])
            assert len(rest) >= 36 and rest.abs().max() <= 0.3 and rest.abs().max() > 0.25 and c.t.abs().max() <= 0.025
            for w_arap in B.ED_W_ARAP:
                assert all(torch.isfinite(v).all() for v in B.ed(torch.float64, c, w_arap))


def test_ed_loud_slots_make_the_last_node_observable():
    """With upstream's zero weights the node a -1 slot indexes cannot matter; with the loud weights it does."""
    c = B.ed_case("gr", 257, True)
    y, ar, _, _ = B.ed(torch.float64, c, 0.5)
    moved = c.t.clone()
    moved[-1] += 0.01
    y2, ar2, _, _ = B.ed(torch.float64, c, 0.5, t=moved)
    assert (y2 - y).abs().max() > 1e-4 and abs(ar2 - ar) > 1e-7


# ------------------------------------------------------------------------------------------ flow metrics
def test_flow_restatement_reproduces_the_metrics_fixture(golden):
    g = golden("F8_metrics")
    flow, gt, ov = torch.from_numpy(g["flow"]), torch.from_numpy(g["flow_gt"]), torch.from_numpy(g["overlap"])
    sums = B.flow_sums(flow.double(), gt.double(), ov)
    assert sums.dtype == torch.float64 and B.flow_sums(flow, gt, ov).dtype == torch.float32
    got = {}
    for tag, row in zip(("full", "vis", "occ"), sums):
        got.update({f"{tag}-epe": 100 * row[0] / row[4], f"{tag}-AccS": 100 * row[1] / row[4], f"{tag}-AccR": 100 * row[2] / row[4],
                    f"{tag}-outlier": 100 * row[3] / row[4]})
    assert sorted(got) == sorted(str(k) for k in g["keys"])
    for k, v in zip(g["keys"], g["vals"]):
        assert abs(float(got[str(k)]) - float(v)) < 1e-4 * max(1.0, abs(float(v))), k


@pytest.mark.parametrize("n", B.FLOW_N)
@pytest.mark.parametrize("mode", B.FLOW_OVERLAPS)
def test_flow_cases_have_both_outcomes_and_keep_off_the_thresholds(n, mode):
    flow, gt, ov, candidates, dropped = B.flow_case(n, mode)
    assert flow.shape == gt.shape == (n, 3) and flow.dtype == torch.float32
    assert dropped <= 0.01 * candidates and not B.near_threshold(flow, gt).any()
    assert {"none": ov is None, "mixed": ov is not None and 0 < ov.sum() < n or n == 1, "all_true": ov is not None and ov.all(),
            "all_false": ov is not None and not ov.any()}[mode]
    s64, s32 = B.flow_sums(flow.double(), gt.double(), ov), B.flow_sums(flow, gt, ov)
    assert torch.equal(s64[:, 1:], s32[:, 1:].double())                          # float32 decides every row as float64 does
    if n >= B.FLOW_SPECIAL_N:
        for k in (1, 2, 3):
            assert s64[0, k] >= 20 and n - s64[0, k] >= 20
        zero_gt = (gt == 0).all(dim=1)
        assert int(zero_gt.sum()) == 10 and int((zero_gt & (flow == 0).all(dim=1)).sum()) == 5 and zero_gt[0] and zero_gt[n - 1]
