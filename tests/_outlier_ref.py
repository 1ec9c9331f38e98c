"""numpy restatements of the compatibility-modulated ops.attention and of the modules of deformationpyramid_amd/outlier.py, written
from the maths: the yardstick of tests/test_outlier.py and tests/test_outlier_cpu.py.  Everything is parameterised by dtype: float64
is the yardstick, the float32 run is the "eager float32" of the project's bar (_kpconv_ref.bar).  Problems are unpadded and
independent, so every function here takes ONE problem.  Nothing here imports the package.

    c[i, j] = max(0, 1 - (|s_i - s_j| - |t_i - t_j|)^2 / sigma_spat^2),   pos = (s_xyz, t_xyz) per row
    o[i, h D + d] = sum_j softmax_j(scale <q'_i,h, k'_j,h> c[i, j]) v[j, h D + d]
    6-D position code: each side the code of xyz / voxel_size on feature_dim / 2 channels, the sides concatenated
    inlier: |R (s + flow) + t - target end|^2 < inlier_thr^2"""
import os
from types import SimpleNamespace

import numpy as np

from . import _lepard_ref as P

F32, F64 = np.float32, np.float64
F25 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F25_outlier.npz")
SIGMA, VOXEL = 0.1, 0.08                                              # configs/outlier_rejection.yaml
Cfg = P.Cfg


def config(C, H, pe_type="rotary", num_layers=2, check=True, sigma_spat=SIGMA, voxel_size=VOXEL):
    return Cfg(in_dim=6, num_layers=num_layers, feature_dim=C, n_head=H, pe_type=pe_type, voxel_size=voxel_size, sigma_spat=sigma_spat,
               spatial_consistency_check=check)


# ------------------------------------------------------------------------------------------ the operator
def position_code(vec6d, C, pe_type, voxel_size=VOXEL, dtype=F64):
    """vec6d [N, 6] -> rotary [N, C, 2] or sinusoidal [N, C]: lepard's code of each side on C / 2 channels without an origin."""
    vec6d = np.asarray(vec6d)
    sides = [P.position_code(vec6d[:, a:a + 3], C // 2, pe_type, voxel_size, vol_origin=[0.0, 0.0, 0.0], dtype=dtype) for a in (0, 3)]
    return np.concatenate(sides, 1)


def compat(pos_q, pos_k, sigma_spat=SIGMA, dtype=F64):
    """[L, S]: in the reference's order -- two norms, their difference squared, divided by dtype(sigma^2), 1 minus, clamp at 0."""
    pq, pk = np.asarray(pos_q).astype(dtype), np.asarray(pos_k).astype(dtype)
    ds = np.sqrt(((pq[:, None, :3] - pk[None, :, :3]) ** 2).sum(-1))
    dt = np.sqrt(((pq[:, None, 3:] - pk[None, :, 3:]) ** 2).sum(-1))
    c = np.maximum(dtype(1) - (ds - dt) ** 2 / dtype(float(sigma_spat) ** 2), dtype(0))
    assert c.dtype == dtype
    return c


def attention(q, k, v, H, pe_q=None, pe_k=None, pos_q=None, pos_k=None, sigma_spat=None, scale=None, dtype=F64):
    """The plain attention of _lepard_ref when sigma_spat is None."""
    if sigma_spat is None:
        return P.attention(q, k, v, H, pe_q, pe_k, scale, dtype)
    D = np.asarray(q).shape[1] // H
    a = P.scores(q, k, H, pe_q, pe_k, 1.0, dtype) * compat(pos_q, pos_k, sigma_spat, dtype)[:, :, None]
    a = a * dtype(D ** -0.5 if scale is None else scale)
    a = np.exp(a - a.max(1, keepdims=True))
    a = a / a.sum(1, keepdims=True)
    o = np.einsum("lsh,shd->lhd", a, np.asarray(v).astype(dtype).reshape(-1, H, D)).reshape(np.asarray(q).shape[0], -1)
    assert o.dtype == dtype
    return o


# ------------------------------------------------------------------------------------------ the modules
def layer(sd, prefix, x, source, x_pe, source_pe, H, pe_type, pos_x=None, pos_s=None, sigma_spat=None, dtype=F64):
    W = lambda name: sd[prefix + name].astype(dtype)
    x, source = np.asarray(x).astype(dtype), np.asarray(source).astype(dtype)
    q, k, v, pe_q, pe_k = x, source, source, None, None
    if x_pe is not None:
        if pe_type == "sinusoidal":
            q, k = q + np.asarray(x_pe).astype(dtype), k + np.asarray(source_pe).astype(dtype)
        elif pe_type == "rotary":
            pe_q, pe_k = x_pe, source_pe
    o = attention(q @ W("q_proj.weight").T, k @ W("k_proj.weight").T, v @ W("v_proj.weight").T, H, pe_q, pe_k, pos_x, pos_s, sigma_spat, None, dtype)
    m = P.layer_norm(o @ W("merge.weight").T, W("norm1.weight"), W("norm1.bias"))
    m = np.concatenate([x, m], 1) @ W("mlp.0.weight").T
    m = np.maximum(m, 0) @ W("mlp.2.weight").T
    return x + P.layer_norm(m, W("norm2.weight"), W("norm2.bias"))


def network(sd, cfg, vec6d, dtype=F64):
    """Outlier_Rejection on one pair's vec6d [M, 6] -> (logit [M], confidence [M])."""
    W = lambda name: sd[name].astype(dtype)
    v6 = np.asarray(vec6d).astype(dtype)
    pe = None if cfg["pe_type"] == "none" else position_code(v6, cfg["feature_dim"], cfg["pe_type"], cfg["voxel_size"], dtype)
    sigma = cfg["sigma_spat"] if cfg["spatial_consistency_check"] else None
    feat = v6 @ W("in_proj.weight").T + W("in_proj.bias")
    for i in range(cfg["num_layers"]):
        feat = layer(sd, f"_6D_geometry_layers.{i}.", feat, feat, pe, pe, cfg["n_head"], cfg["pe_type"], v6, v6, sigma, dtype)
    h = np.maximum(feat @ W("classification.0.weight").T + W("classification.0.bias"), 0)
    h = np.maximum(h @ W("classification.2.weight").T + W("classification.2.bias"), 0)
    z = (h @ W("classification.4.weight").T + W("classification.4.bias"))[:, 0]
    return z, dtype(1) / (dtype(1) + np.exp(-z))


def inlier_residual(s_pcd, flow, rot, trn, ind_s, tgt_ends, dtype=F64):
    """|R (s + flow) + t - target end|^2 of every match of one pair."""
    warped = (np.asarray(rot).astype(dtype) @ (np.asarray(s_pcd).astype(dtype) + np.asarray(flow).astype(dtype)).T + np.asarray(trn).astype(dtype).reshape(3, 1)).T
    return ((warped[np.asarray(ind_s)] - np.asarray(tgt_ends).astype(dtype)) ** 2).sum(1)


# ------------------------------------------------------------------------------------------ the cases of tests/test_outlier.py
#        (L, S, C, H): the smallest shapes at each tile edge (16 query rows, 64 keys), D = 6, 12 and 18 (the shipped head width, on
# the unvectorised staging path: 18 is no multiple of 4), and the shipped C = 144 / H = 8 past one key tile on either side
COMPAT_SHAPES = [(1, 1, 6, 1), (1, 17, 12, 2), (17, 1, 12, 2), (15, 16, 48, 4), (63, 65, 48, 4), (64, 64, 72, 4), (65, 129, 144, 8),
                 (129, 65, 144, 8)]
COMPAT_BATCH = [(1, 1), (67, 31), (40, 67)]                           # three unequal problems in one call, C = 48, H = 4
_made = {}


def matches(n, seed, outlier_share=0.4, noise=0.01):
    """n correspondences in the reference's metre range -> vec6d [n, 6] float32: the target end of an inlier is its source end under
    a smooth deformation and a rigid motion plus noise, that of an outlier a random point.  Inside one problem c is then both
    positive (inlier pairs keep their distances to within sigma) and exactly zero."""
    g = np.random.default_rng(seed)
    s = g.uniform(-0.6, 0.6, (n, 3))
    ang = 0.4
    Rm = np.array([[np.cos(ang), -np.sin(ang), 0], [np.sin(ang), np.cos(ang), 0], [0, 0, 1.0]])
    t = (s + 0.03 * np.sin(3.0 * s[:, ::-1])) @ Rm.T + np.array([0.2, -0.1, 0.05]) + noise * g.standard_normal((n, 3))
    out = g.uniform(0, 1, n) < outlier_share
    t[out] = g.uniform(-0.6, 0.6, (int(out.sum()), 3))
    return np.concatenate([s, t], 1).astype(F32)


def compat_inputs(L, S, C, H, rotary, seed=None, spread=1.0):
    """_lepard_ref.attention_inputs plus positions: the query rows' and the key rows' correspondences are drawn from one cloud of
    matches (the first min(L, S) rows are the same correspondences, as in the network's self-attention)."""
    key = (L, S, C, H, rotary, seed, spread)
    if key not in _made:
        c = P.attention_inputs(L, S, C, H, rotary, seed, spread)
        pos = matches(max(L, S), 7919 * L + 31 * S + C if seed is None else seed)
        _made[key] = SimpleNamespace(q=c.q, k=c.k, v=c.v, pe_q=c.pe_q, pe_k=c.pe_k, H=H, pos_q=pos[:L].copy(), pos_k=pos[:S].copy())
    return _made[key]


def compat_refs(c, sigma_spat=SIGMA):
    """(float64, float32) outputs of a case, computed once."""
    if not hasattr(c, "refs"):
        c.refs = {}
    if sigma_spat not in c.refs:
        c.refs[sigma_spat] = tuple(attention(c.q, c.k, c.v, c.H, c.pe_q, c.pe_k, c.pos_q, c.pos_k, sigma_spat, None, dt) for dt in (F64, F32))
    return c.refs[sigma_spat]


def positive_share(c):
    m = compat(c.pos_q, c.pos_k)
    return float((m > 0).mean())


# ------------------------------------------------------------------------------------------ fixture F25
F25_LAYER_VARIANTS = ["rotary", "sinusoidal", "none"]                  # (a): C = 48, H = 4, B = 2 with prefix masks
F25_LAYER_LENS = [21, 9]
F25_NETS = {"b": dict(C=48, H=4, num_layers=2, lens=[37, 21]), "b1": dict(C=72, H=4, num_layers=1, lens=[37, 21])}       # b1: the issue's (b')
F25_POINTS = 48                                                        # coarse points a side of every pair of (b) / (b')
F25_THR = 0.5                                                          # the recorded confidence threshold
F25_INLIER_THR = 0.04                                                  # (c)


def load_f25():
    return np.load(F25)


def net_config(name):
    n = F25_NETS[name]
    return config(n["C"], n["H"], num_layers=n["num_layers"])


def net_vec6d(z, name):
    """The stacked vec_6d of a network case, per pair, from the recorded clouds and matches."""
    p = name + "."
    out = []
    for b, _ in enumerate(F25_NETS[name]["lens"]):
        rows = z[p + "match"][z[p + "match"][:, 0] == b]
        out.append(np.concatenate([z[p + "s_pcd"][b][rows[:, 1]], z[p + "t_pcd"][b][rows[:, 2]]], 1))
    return out


def run_net(z, name, dtype=F64):
    sd, cfg = P.sub_dict(z, name + ".sd."), net_config(name)
    return [network(sd, cfg, v6, dtype) for v6 in net_vec6d(z, name)]


def net_preconditions(z, name):
    """(ok, why): the positive share of c in 0.1 .. 0.9; every row's float64 confidence more than twice the bar away from the
    threshold, at least a quarter of the rows on each side of it; the reference's float32 confidences inside the bar with the same
    rows above the threshold."""
    from ._kpconv_ref import bar
    p = name + "."
    r64, r32 = run_net(z, name, F64), run_net(z, name, F32)
    for b, ((_, c64), (_, c32), v6) in enumerate(zip(r64, r32, net_vec6d(z, name))):
        share = float((compat(v6, v6) > 0).mean())
        if not 0.1 <= share <= 0.9 or abs(share - float(z[p + "positive_share"][b])) > 1e-12:
            return False, f"pair {b}: positive share of c {share:.3f} (recorded {float(z[p + 'positive_share'][b]):.3f})"
        bb = bar(np.abs(c32.astype(F64) - c64).max(), np.abs(c64).max())
        gap = float(np.abs(c64 - F25_THR).min())
        if not gap > 2 * bb:
            return False, f"pair {b}: a confidence {gap:.3e} from the threshold against bar {bb:.3e}"
        above = float((c64 > F25_THR).mean())
        if not 0.25 <= above <= 0.75:
            return False, f"pair {b}: {above:.2f} of the rows above the threshold"
        n = len(c64)
        got = np.asarray(z[p + "conf"])[b, :n]
        err = float(np.abs(got.astype(F64) - c64).max())
        if not err <= bb:
            return False, f"pair {b}: reference float32 confidence error {err:.3e} above bar {bb:.3e}"
        if not np.array_equal(got > F25_THR, c64 > F25_THR):
            return False, f"pair {b}: the reference's float32 rows above the threshold differ from float64's"
    return True, ""


def inlier_preconditions(z):
    """(ok, why): no float64 residual of (c) within 1e-5 (relative) of inlier_thr^2, and both kinds of match present."""
    v6 = net_vec6d(z, "b")
    for b in range(len(v6)):
        rows = z["b.match"][z["b.match"][:, 0] == b]
        res = inlier_residual(z["b.s_pcd"][b], z["c.flow"][b], z["c.rot"][b], z["c.trn"][b], rows[:, 1], v6[b][:, 3:])
        if float(np.abs(res / F25_INLIER_THR ** 2 - 1).min()) < 1e-5:
            return False, f"pair {b}: a residual within 1e-5 of inlier_thr^2"
        if not 0 < (res < F25_INLIER_THR ** 2).sum() < len(res):
            return False, f"pair {b}: the matches are all inliers or all outliers"
    return True, ""
