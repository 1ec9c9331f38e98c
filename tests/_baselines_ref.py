"""Plain-torch restatements of what csrc/ndp_nerfies.inc, csrc/ndp_ed.inc and csrc/ndp_flow_metrics.inc compute, with the inputs
of tests/test_baselines_edges.py.  Every function follows the dtype of its input: float64 is the yardstick, float32 is the eager
arithmetic whose own error sets the project's bar (tests/_kpconv_ref.bar).  The preconditions the inputs are built to meet are
asserted in tests/test_baselines_cpu.py.

Nerfies.  oracle/nerfies_ref.py builds float32 tensors whatever it is given; this is the same network, dtype-generic, and it also
returns every layer's pre-activation z.  Two choices keep a float32 / float64 comparison meaningful:
  * loud weights -- with the default init J - I is 1e-3 .. 0.1, so a tangent path wrong by 1e-3 of its own scale hides below any
    float32 bar.  LOUD scales the six 128x128 matrices by 1.7 and the head weights and biases by 6 (seed-23 init).
  * kink-free inputs -- a pre-activation that is +1e-8 in float64 and -1e-8 in float32 switches a ReLU off and moves J by O(1):
    a discontinuity of the function, not an error of either evaluation.  Points are kept only if every one of their 7 x 128
    float64 pre-activations has |z| > KINK_MARGIN.
Gradients are those of sum(warped * gy) with a random upstream gy: Chamfer's argmin would be a second discontinuity.
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import torch

from ._kpconv_ref import ULP, bar  # noqa: F401  (bar is re-exported: the tests take it from here)

# ------------------------------------------------------------------------------------------ Nerfies
W, M_FREQ, K0, DIM_PE, N_HID = 128, 6, -3, 39, 6
PI32 = float(np.float32(3.14))                                   # the kernel's constant: float32(3.14), cast up
P_COUNT = W * DIM_PE + W + N_HID * (W * W + W) + 6 * W + 6
MAX_ITER = 5000
KINK_MARGIN = 1e-5
LOUD_HIDDEN, LOUD_HEAD = 1.7, 6.0

NERFIES_FWD_CASES = [(1, 2999), (63, 2999), (64, 2999), (65, 2999), (257, 2999), (257, 0), (257, 700)]     # (n, it), loud weights
NERFIES_DEFAULT_CASE = (65, 2999)                                                                          # default init
NERFIES_BWD_CASES = [(1, None), (64, 1), (65, 1), (65, 2), (65, 5), (257, 1), (257, 3), (257, None)]       # (n, n_part), it = 2999
NERFIES_BWD_IT = 2999
NERFIES_STRIDE_N = 512 * 64 + 65                                 # 514 tiles: k_nrf_dense's grid of 512 strides once


def split(flat):
    """[W_in 128x39 | b_in | (W_l 128x128 | b_l) x 6 | W_h 6x128 | b_h 6] -> 16 views."""
    o, out = 0, []
    for shape in [(W, DIM_PE), (W,)] + [(W, W), (W,)] * N_HID + [(6, W), (6,)]:
        n = math.prod(shape)
        out.append(flat[o:o + n].reshape(shape))
        o += n
    return out


def window(it, max_iter, dtype):
    a = M_FREQ * it / (0.6 * max_iter)
    return (1 - torch.cos(torch.clamp(a - torch.arange(M_FREQ, dtype=dtype), min=0, max=1) * PI32)) / 2


def posenc(x, it, max_iter):
    """-> pe [n,39] = [x | sin_x(6) cos_x(6) | sin_y cos_y | sin_z cos_z] (windowed) and dpe [n,3,39] = d pe / d x."""
    n, dt = x.shape[0], x.dtype
    w = window(it, max_iter, dt)
    f = (2.0 ** (torch.arange(M_FREQ, dtype=dt) + K0)) * PI32
    pe, dpe = torch.zeros(n, DIM_PE, dtype=dt), torch.zeros(n, 3, DIM_PE, dtype=dt)
    pe[:, :3] = x
    for a in range(3):
        arg = x[:, a:a + 1] * f[None]
        s, c = torch.sin(arg) * w, torch.cos(arg) * w
        pe[:, 3 + 12 * a:9 + 12 * a], pe[:, 9 + 12 * a:15 + 12 * a] = s, c
        dpe[:, a, a] = 1.0
        dpe[:, a, 3 + 12 * a:9 + 12 * a], dpe[:, a, 9 + 12 * a:15 + 12 * a] = c * f, -s * f
    return pe, dpe


def skew(w):
    z = torch.zeros_like(w[..., 0])
    return torch.stack([z, -w[..., 2], w[..., 1], w[..., 2], z, -w[..., 0], -w[..., 1], w[..., 0], z], -1).reshape(*w.shape[:-1], 3, 3)


def se3_warp(o, x):
    """o [n,6] = (w, v) raw head outputs -> R(w) x + P(w) v / |w|  (the SE(3) exponential of the screw (w, v))."""
    w, v = o[..., :3], o[..., 3:]
    th = w.norm(dim=-1, keepdim=True)
    K, vh, th = skew(w / th), v / th, th[..., None]
    eye = torch.eye(3, dtype=o.dtype).expand_as(K)
    R = eye + torch.sin(th) * K + (1 - torch.cos(th)) * (K @ K)
    P = eye + (1 - torch.cos(th)) * K + (th - torch.sin(th)) * (K @ K)
    return (R @ x[..., None] + P @ vh[..., None])[..., 0]


def preactivations(flat, x, it, max_iter=MAX_ITER):
    """-> (pe, dpe, [z_0 .. z_6] each [n,128], h_6)."""
    p = split(flat)
    pe, dpe = posenc(x, it, max_iter)
    zs, h = [], pe
    for l in range(N_HID + 1):
        zs.append(h @ p[2 * l].T + p[2 * l + 1])
        h = torch.relu(zs[-1])
    return pe, dpe, zs, h


def regularization(J, eps=1e-6):
    """mean over points of log(largest singular value of J)^2, in double, singular values clamped at eps."""
    sv = torch.clamp(torch.linalg.svdvals(J.double()), min=eps)
    return (torch.log(sv.max(dim=1)[0]) ** 2).mean()


def nerfies(flat, x, it, max_iter=MAX_ITER, gy=None):
    """flat [>= P_COUNT], x [n,3] of one dtype -> pe, zs, o (heads), warped, J (forward tangents, masked by the primal's z > 0),
    reg, and with gy [n,3] the gradient of sum(warped * gy) in the parameters (flat layout)."""
    flat = flat[:P_COUNT].detach().clone().requires_grad_(gy is not None)
    p = split(flat)
    pe, dpe, zs, h = preactivations(flat, x, it, max_iter)
    o = h @ p[14].T + p[15]
    warped = se3_warp(o, x)
    with torch.no_grad():
        t = dpe
        for l in range(N_HID + 1):
            t = (t @ p[2 * l].T) * (zs[l] > 0)[:, None, :]
        D = t @ p[14].T                                                         # [n,3,6] = d o / d x_k
        cols = []
        for k in range(3):
            e = torch.zeros_like(x)
            e[:, k] = 1.0
            cols.append(torch.func.jvp(se3_warp, (o.detach(), x), (D[:, k], e))[1])
        J = torch.stack(cols, dim=-1)                                           # J[n, a, k] = d warped_a / d x_k
    grad = None
    if gy is not None:
        (warped * gy).sum().backward()
        grad = flat.grad.detach()
    return SimpleNamespace(pe=pe.detach(), zs=[z.detach() for z in zs], o=o.detach(), warped=warped.detach(), J=J, reg=regularization(J),
                           grad=grad)


def nerfies_pair(flat32, x32, it, gy32=None):
    """The float64 yardstick and the eager float32 restatement on the same float32 inputs."""
    d = lambda a: None if a is None else a.double()
    return nerfies(d(flat32), d(x32), it, gy=d(gy32)), nerfies(flat32, x32, it, gy=gy32)


@functools.lru_cache(maxsize=None)
def nerfies_flat(kind):
    """float32 parameters in the product's flat layout (padded to its stride): 'default' = the seed-23 Nerfies_Deformation init,
    'loud' = its six hidden matrices x 1.7 and head weights and biases x 6, 'rotation' = everything zero but a head bias (w, v)
    with |w| = 0.7, so that the warp is one rigid motion and J a pure rotation."""
    from deformationpyramid_amd import nerfies as NF
    torch.manual_seed(23)
    flat = NF.Nerfies_Deformation(max_iter=MAX_ITER).flat.clone()
    if kind == "loud":
        for l in range(1, N_HID + 1):
            flat[NF.off_W(l):NF.off_b(l)] *= LOUD_HIDDEN
        flat[NF.OFF_WH:NF.OFF_BH + 6] *= LOUD_HEAD
    elif kind == "rotation":
        flat.zero_()
        flat[NF.OFF_BH:NF.OFF_BH + 6] = torch.tensor([0.2, -0.3, 0.6, 0.1, -0.2, 0.3])       # |w| = 0.7
    else:
        assert kind == "default"
    return flat


def kink_margin(flat32, x32, it):
    """min over the 7 x 128 float64 pre-activations of |z|, per point."""
    _, _, zs, _ = preactivations(flat32[:P_COUNT].double(), x32.double(), it)
    return torch.stack([z.abs().min(dim=1)[0] for z in zs]).min(dim=0)[0]


@functools.lru_cache(maxsize=None)
def kink_free_points(kind, n, it, seed=5):
    """-> (x [n,3] float32: the first n candidates, uniform in [-0.5, 0.5]^3, whose margin exceeds KINK_MARGIN; candidates examined;
    candidates dropped).  At least 1024 candidates are examined so that the dropped share means something at n = 1."""
    c = max(1024, int(math.ceil(1.3 * n)))
    cand = (torch.rand(c, 3, generator=torch.Generator().manual_seed(seed + 1000 * it + n)) - 0.5).contiguous()
    keep = kink_margin(nerfies_flat(kind), cand, it) > KINK_MARGIN
    assert int(keep.sum()) >= n
    return cand[keep][:n].contiguous(), c, int((~keep).sum())


def upstream_gradient(n, seed=11):
    return (torch.rand(n, 3, generator=torch.Generator().manual_seed(seed + n)) - 0.5).contiguous()


def stride_case():
    """x [NERFIES_STRIDE_N, 3] uniform (unfiltered: only some rows are compared) and the rows to compare: 0..63 and every row from
    32768 on (the two tiles past k_nrf_dense's grid), those of them that pass the kink margin."""
    n = NERFIES_STRIDE_N
    x = (torch.rand(n, 3, generator=torch.Generator().manual_seed(77)) - 0.5).contiguous()
    rows = torch.cat([torch.arange(64), torch.arange(512 * 64, n)])
    rows = rows[kink_margin(nerfies_flat("loud"), x[rows], 2999) > KINK_MARGIN]
    return x, rows


# ------------------------------------------------------------------------------------------ embedded deformation
ED_S = (0, 1, 255, 256, 257, 600)
ED_W_ARAP = (0.0, 0.5)
ED_GRAPHS = ("g", "gr")                                           # fixture F15: 129 nodes, 378 nodes (a second block of k_ed_rot)
ED_PHI_CLASSES = {0: 0.0, 1: 3e-7, 2: 3e-6, 3: 3.1, 4: 4.0}       # |phi| by node index mod 7; 5 and 6: components in +-0.3
ED_LOUD_ANCHOR, ED_LOUD_EDGE = 0.05, 0.3                          # weights given to the -1 slots in the second run


@functools.lru_cache(maxsize=None)
def ed_graph(tag):
    """Graph and anchored points of the F15 depth map as Registration.load_raw_pcds_from_depth builds them.  Points are ordered so that
    every prefix of length >= 1 holds a point with a -1 anchor slot: those points first, in their own order, interleaved one to one
    with the others."""
    import os
    from deformationpyramid_amd.config import Config
    from deformationpyramid_amd.geometry import get_deformation_graph_from_depthmap
    BASE = dict(deformation_model="ED", max_triangle_distance=0.06, node_coverage=0.09, USE_ONLY_VALID_VERTICES=True, num_neighbors=8,
                ENFORCE_TOTAL_NUM_NEIGHBORS=False, SAMPLE_RANDOM_SHUFFLE=False, REMOVE_NODES_WITH_NOT_ENOUGH_NEIGHBORS=False)   # tests/test_ed.py
    g = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F15_embedded_deformation.npz"), allow_pickle=False))
    cfg = Config(dict(BASE, REMOVE_NODES_WITH_NOT_ENOUGH_NEIGHBORS=tag == "gr", node_coverage=float(g[f"{tag}.coverage"])))
    data = get_deformation_graph_from_depthmap(g["depth_src"].copy(), g["K"], cfg)
    valid = torch.sum(data["pixel_anchors"], dim=-1) > -4
    x, a, w = data["point_image"][valid].float(), data["pixel_anchors"][valid].long(), data["pixel_weights"][valid].float()
    has = (a < 0).any(dim=1)
    i_has, i_not = torch.nonzero(has)[:, 0], torch.nonzero(~has)[:, 0]
    m = min(len(i_has), len(i_not))
    order = torch.cat([torch.stack([i_has[:m], i_not[:m]], 1).reshape(-1), i_has[m:], i_not[m:]])
    return SimpleNamespace(nodes=data["graph_nodes"].float().contiguous(), edges=data["graph_edges"].long().contiguous(),
                           edge_w=data["graph_edges_weights"].float().contiguous(), x=x[order].contiguous(), anchors=a[order].contiguous(),
                           weights=w[order].contiguous())


def ed_state(n, seed=3):
    """phi, t [n,3] float32: phi by class (ED_PHI_CLASSES) in a random direction, t with components in +-0.025."""
    gen = torch.Generator().manual_seed(seed + n)
    phi = (torch.rand(n, 3, generator=gen) - 0.5) * 0.6
    d = torch.randn(n, 3, generator=gen, dtype=torch.float64)
    d = d / d.norm(dim=1, keepdim=True)
    for k, mag in ED_PHI_CLASSES.items():
        phi[k::7] = (d[k::7] * mag).float()
    t = (torch.rand(n, 3, generator=gen) - 0.5) * 0.05
    return phi.contiguous(), t.contiguous()


def ed_case(tag, S, loud_slots):
    """-> graph data with the first S points, phi, t, gy.  loud_slots: the -1 anchor and edge slots carry ED_LOUD_ANCHOR / ED_LOUD_EDGE
    instead of upstream's 0, which makes the node they index observable."""
    G = ed_graph(tag)
    n = G.nodes.shape[0]
    phi, t = ed_state(n)
    x, a, w = G.x[:S].contiguous(), G.anchors[:S].contiguous(), G.weights[:S].clone()
    ew = G.edge_w.clone()
    if loud_slots:
        w[a < 0] = ED_LOUD_ANCHOR
        ew[G.edges < 0] = ED_LOUD_EDGE
    gy = (torch.rand(S, 3, generator=torch.Generator().manual_seed(17 + S)) - 0.5).contiguous()
    return SimpleNamespace(tag=tag, S=S, n=n, nodes=G.nodes, edges=G.edges, edge_w=ew.contiguous(), x=x, anchors=a, weights=w.contiguous(),
                           phi=phi, t=t, gy=gy)


def ed(dtype, c, w_arap, phi=None, t=None):
    """oracle/ed_ref (which follows its input's dtype; -1 slots by Python negative indexing) on case c in `dtype`
    -> (y [S,3], arap, dphi [n,3], dt [n,3]) of  sum(y * gy) + w_arap * arap."""
    from oracle import ed_ref as E
    f = lambda a: a.to(dtype)
    phi_r = f(c.phi if phi is None else phi).clone().requires_grad_(True)
    t_r = f(c.t if t is None else t).clone().requires_grad_(True)
    Rm = E.axis_angle_to_matrix(phi_r)
    y = E.ed_warp(f(c.x), c.anchors, f(c.weights), f(c.nodes), Rm, t_r)
    ar = E.arap(Rm, t_r, f(c.nodes), c.edges, f(c.edge_w))
    ((y * f(c.gy)).sum() + w_arap * ar).backward()
    return y.detach(), ar.detach(), phi_r.grad, t_r.grad


# ------------------------------------------------------------------------------------------ flow metrics
FLOW_N = (1, 1023, 1024, 1025, 3000)
FLOW_OVERLAPS = ("none", "mixed", "all_true", "all_false")
FLOW_THRESHOLDS = (0.025, 0.05, 0.3)
FLOW_SPECIAL_N = 1023                                             # cases of at least this many rows carry the ten special rows
_SPECIAL_FLOW = [[0.01, 0.0, 0.0], [0.0, -0.03, 0.0], [0.02, 0.02, -0.03], [0.0, 0.06, 0.0], [-0.1, 0.0, 0.0]]


def flow_errors(flow, gt):
    err = torch.linalg.vector_norm(flow - gt, dim=1)
    return err, err / (torch.linalg.vector_norm(gt, dim=1) + 1e-20)


def flow_sums(flow, gt, overlap=None):
    """[3,5] in the inputs' dtype: per subset {all, overlap, ~overlap} {sum err, #AccS, #AccR, #outlier, #rows}."""
    err, rel = flow_errors(flow, gt)
    cols = torch.stack([err, ((err < 0.025) | (rel < 0.025)).to(err.dtype), ((err < 0.05) | (rel < 0.05)).to(err.dtype),
                        (rel > 0.3).to(err.dtype), torch.ones_like(err)], 1)
    z = torch.zeros(5, dtype=err.dtype)
    return torch.stack([cols.sum(0), cols[overlap].sum(0) if overlap is not None else z, cols[~overlap].sum(0) if overlap is not None else z])


def near_threshold(flow, gt, tol=1e-5):
    """rows whose float64 err or rel lies within tol (relative) of a threshold it is compared with."""
    err, rel = flow_errors(flow.double(), gt.double())
    near = torch.zeros_like(err, dtype=torch.bool)
    for v, ths in ((err, (0.025, 0.05)), (rel, FLOW_THRESHOLDS)):
        for th in ths:
            near |= (v - th).abs() <= tol * th
    return near


@functools.lru_cache(maxsize=None)
def flow_case(n, overlap_mode, seed=9):
    """gt ~ U(-0.2, 0.2)^3, flow = gt + N(0, 0.03), rows near a threshold filtered out; with n >= FLOW_SPECIAL_N ten rows spread from
    row 0 to row n - 1 alternate (gt = 0, flow != 0) and (both 0).  -> flow, gt float32, overlap (bool or None), candidates, dropped."""
    gen = torch.Generator().manual_seed(seed + n)
    c = n + max(16, n // 50)
    gt = (torch.rand(c, 3, generator=gen) - 0.5) * 0.4
    flow = gt + torch.randn(c, 3, generator=gen) * 0.03
    keep = ~near_threshold(flow, gt)
    assert int(keep.sum()) >= n
    flow, gt = flow[keep][:n].clone(), gt[keep][:n].clone()
    if n >= FLOW_SPECIAL_N:
        for k, row in enumerate(np.linspace(0, n - 1, 10).astype(int)):
            gt[row] = 0.0
            flow[row] = torch.tensor(_SPECIAL_FLOW[k // 2]) if k % 2 == 0 else 0.0
    ov = {"none": None, "mixed": torch.rand(n, generator=gen) < 0.5, "all_true": torch.ones(n, dtype=torch.bool),
          "all_false": torch.zeros(n, dtype=torch.bool)}[overlap_mode]
    return flow.contiguous(), gt.contiguous(), ov, c, int((~keep).sum())
