"""numpy restatements of ops.attention, ops.feat_conf and of the modules of deformationpyramid_amd/lepard.py, written from the maths:
the yardstick of tests/test_lepard.py and tests/test_lepard_cpu.py.  Everything is parameterised by dtype: float64 is the yardstick,
the float32 run is the "eager float32" of the project's bar (_kpconv_ref.bar).  Problems are unpadded and independent, so every
function here takes ONE problem.  Nothing here imports the package.

    q' = q cos + rot(q) sin,  rot(x)[2m] = -x[2m+1],  rot(x)[2m+1] = x[2m]
    o[i, h D + d] = sum_j softmax_j(scale <q'_i,h, k'_j,h>) v[j, h D + d]
    conf_ij = softmax_i(a) softmax_j(a),  a = <fs_i, ft_j> / (C temperature)
    soft-Procrustes: the n = int(max(S, T) sample_rate) largest conf entries weigh their point pairs in a weighted Kabsch fit whose
    3 x 3 SVD runs in double whatever the dtype (the reference's own), condition = largest / smallest singular value."""
import math
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _kpfcn_ref as K

F32, F64 = np.float32, np.float64
F24 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F24_lepard.npz")
VOL_BNDS = [[-3.6, -2.4, 1.14], [1.093, 0.78, 2.92]]                 # configs/lepard.yaml
LAYER_TYPES = ["self", "cross", "positioning", "self", "cross"]
MAX_CONDITION = 40.0


class Cfg(dict):
    """A dict with attribute access: the reference reads config['x'] and config.x alike."""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def transformer_config(C, H, pe_type="rotary", voxel_size=0.04, sample_rate=1.0, entangled=False, layer_types=LAYER_TYPES,
                       positioning_type="procrustes"):
    """configs/lepard.yaml's coarse_transformer (and its coarse_matching) at C channels and H heads."""
    matching = Cfg(feature_dim=C, confidence_threshold=0.1, dsmax_temperature=0.1, match_type="dual_softmax", entangled=entangled,
                   skh_init_bin_score=1.0, skh_iters=3, skh_prefilter=False)
    return Cfg(feature_dim=C, n_head=H, layer_types=list(layer_types), positioning_type=positioning_type, pe_type=pe_type,
               entangled=entangled, vol_bnds=VOL_BNDS, voxel_size=voxel_size, feature_matching=matching,
               procrustes=Cfg(max_condition_num=MAX_CONDITION, sample_rate=sample_rate))


def pipeline_config(C=12, H=2):
    """Fixture F24 (c): F23's backbone config with a transformer of C = coarse_feature_dim channels."""
    t = transformer_config(C, H)
    return Cfg(kpfcn_config=Cfg(K.F23_CONFIG), coarse_transformer=t, coarse_matching=t.feature_matching)


# ------------------------------------------------------------------------------------------ position codes
def position_code(xyz, C, pe_type, voxel_size, vol_origin=VOL_BNDS[0], dtype=F64):
    """xyz [N, 3] -> rotary [N, C, 2] (cos, sin) or sinusoidal [N, C].  The frequencies are the reference's float32 numbers, from torch's own
    float32 exp (libraries differ in its last bit, and a bit of a frequency is 1e-6 of a code at 25 voxels)."""
    third = C // 3
    div = torch.exp(torch.arange(0, third, 2, dtype=torch.float) * (-math.log(10000.0) / third)).numpy().astype(dtype)      # torch's float32 exp, to the bit
    vox = (np.asarray(xyz).astype(dtype) - np.asarray(vol_origin, F32).astype(dtype)) / dtype(voxel_size)
    ang = vox[:, :, None] * div[None, None, :]                                       # [N, 3, C / 6]
    sin, cos = np.sin(ang), np.cos(ang)
    n = ang.shape[0]
    if pe_type == "sinusoidal":
        return np.stack([sin, cos], 2).reshape(n, -1)
    return np.stack([np.repeat(cos, 2, axis=2).reshape(n, -1), np.repeat(sin, 2, axis=2).reshape(n, -1)], -1)


def rotate(x, pe):
    x2 = np.stack([-x[:, 1::2], x[:, ::2]], -1).reshape(x.shape)
    return x * pe[..., 0] + x2 * pe[..., 1]


def embed_pos(pe_type, x, pe):
    return rotate(x, pe) if pe_type == "rotary" else x + pe


# ------------------------------------------------------------------------------------------ the operators
def scores(q, k, H, pe_q=None, pe_k=None, scale=None, dtype=F64):
    """[L, S, H] scaled scores of one problem."""
    q, k = np.asarray(q).astype(dtype), np.asarray(k).astype(dtype)
    if pe_q is not None:
        q, k = rotate(q, np.asarray(pe_q).astype(dtype)), rotate(k, np.asarray(pe_k).astype(dtype))
    D = q.shape[1] // H
    scale = dtype(D ** -0.5 if scale is None else scale)
    return np.einsum("lhd,shd->lsh", q.reshape(-1, H, D), k.reshape(-1, H, D)) * scale


def attention(q, k, v, H, pe_q=None, pe_k=None, scale=None, dtype=F64):
    a = scores(q, k, H, pe_q, pe_k, scale, dtype)
    a = np.exp(a - a.max(1, keepdims=True))
    a = a / a.sum(1, keepdims=True)
    D = q.shape[1] // H
    o = np.einsum("lsh,shd->lhd", a, np.asarray(v).astype(dtype).reshape(-1, H, D)).reshape(q.shape[0], -1)
    assert o.dtype == dtype
    return o


def _softmax(a, axis):
    e = np.exp(a - a.max(axis, keepdims=True))
    return e / e.sum(axis, keepdims=True)


def feat_conf(fs, ft, temperature=0.1, dtype=F64):
    fs, ft = np.asarray(fs).astype(dtype), np.asarray(ft).astype(dtype)
    a = (fs @ ft.T) * dtype(1.0 / (fs.shape[1] * temperature))
    return _softmax(a, 0) * _softmax(a, 1)


def get_match(conf, thr=0.1):
    """[M, 2] rows (s, t): conf > thr and the maximum of both its row and its column."""
    mask = (conf > thr) & (conf == conf.max(1, keepdims=True)) & (conf == conf.max(0, keepdims=True))
    return np.argwhere(mask)


# ------------------------------------------------------------------------------------------ the modules
def layer_norm(x, w, b, eps=1e-5):
    mean = x.mean(1, keepdims=True)
    var = ((x - mean) ** 2).mean(1, keepdims=True)
    return (x - mean) / np.sqrt(var + x.dtype.type(eps)) * w.astype(x.dtype) + b.astype(x.dtype)


def attention_layer(sd, prefix, x, source, x_pe, source_pe, H, pe_type, dtype=F64):
    W = lambda name: sd[prefix + name].astype(dtype)
    x, source = np.asarray(x).astype(dtype), np.asarray(source).astype(dtype)
    q, k, v, pe_q, pe_k = x, source, source, None, None
    if x_pe is not None:
        if pe_type == "sinusoidal":
            q, k = q + np.asarray(x_pe).astype(dtype), k + np.asarray(source_pe).astype(dtype)
        else:
            pe_q, pe_k = x_pe, source_pe
    o = attention(q @ W("q_proj.weight").T, k @ W("k_proj.weight").T, v @ W("v_proj.weight").T, H, pe_q, pe_k, None, dtype)
    m = layer_norm(o @ W("merge.weight").T, W("norm1.weight"), W("norm1.bias"))
    m = np.concatenate([x, m], 1) @ W("mlp.0.weight").T
    m = np.maximum(m, 0) @ W("mlp.2.weight").T
    return x + layer_norm(m, W("norm2.weight"), W("norm2.bias"))


def matching(sd, prefix, src, tgt, src_pe, tgt_pe, pe_type, entangled=False, temperature=0.1, thr=0.1, dtype=F64):
    """-> (conf [S, T], match [M, 2]); src_proj on both sides."""
    W = sd[prefix + "src_proj.weight"].astype(dtype)
    fs, ft = np.asarray(src).astype(dtype) @ W.T, np.asarray(tgt).astype(dtype) @ W.T
    if not entangled:
        fs, ft = embed_pos(pe_type, fs, np.asarray(src_pe).astype(dtype)), embed_pos(pe_type, ft, np.asarray(tgt_pe).astype(dtype))
    conf = feat_conf(fs, ft, temperature, dtype)
    return conf, get_match(conf, thr)


def weighted_procrustes(X, Y, w, eps=1e-4, dtype=F64):
    """procrustes.py:18-44 on one problem: means and covariance in dtype, the 3 x 3 SVD in double -> (R [3,3], t [3,1], condition)."""
    X, Y, w = np.asarray(X).astype(dtype), np.asarray(Y).astype(dtype), np.asarray(w).astype(dtype)[:, None]
    wn = w / (np.abs(w).sum() + dtype(eps))
    mx, my = (wn * X).sum(0, keepdims=True), (wn * Y).sum(0, keepdims=True)
    Sxy = ((Y - my).T @ (wn * (X - mx))).astype(F64)
    U, D, Vt = np.linalg.svd(Sxy)
    S = np.diag([1.0, 1.0, np.linalg.det(U) * np.linalg.det(Vt)])
    R = (U @ S @ Vt).astype(dtype)
    return R, my.T - R @ mx.T, float(D.max() / D.min())


def soft_procrustes(conf, s_pcd, t_pcd, sample_rate=1.0, max_condition=MAX_CONDITION, dtype=F64):
    """The project's per-problem rule -> namespace(R, t, R_forwd, t_forwd, condition, mask, n, gap): gap is the difference between
    the last confidence taken and the first one left out (inf when nothing is left out)."""
    S, T = conf.shape
    n = min(int(max(S, T) * sample_rate), S * T)
    flat = conf.reshape(-1)
    order = np.argsort(-flat, kind="stable")
    idx = order[:n]
    gap = float(flat[order[n - 1]] - flat[order[n]]) if 0 < n < flat.size else np.inf
    R, t, cond = weighted_procrustes(np.asarray(s_pcd)[idx // T], np.asarray(t_pcd)[idx % T], flat[idx], dtype=dtype)
    ok = cond < max_condition
    return SimpleNamespace(R=R, t=t, R_forwd=R if ok else np.eye(3, dtype=dtype), t_forwd=t if ok else np.zeros((3, 1), dtype), condition=cond,
                           mask=bool(ok), n=n, gap=gap)


def transformer(sd, cfg, src, tgt, s_pcd, t_pcd, dtype=F64, prefix=""):
    """RepositioningTransformer on one problem -> (src_feat, tgt_feat, src_pe, tgt_pe, position_layers [namespace(conf, match, fit)])."""
    C, H, pe_type, vs = cfg["feature_dim"], cfg["n_head"], cfg["pe_type"], cfg["voxel_size"]
    code = lambda p: position_code(p, C, pe_type, vs, cfg["vol_bnds"][0], dtype)
    s_pcd, t_pcd = np.asarray(s_pcd).astype(dtype), np.asarray(t_pcd).astype(dtype)
    src, tgt = np.asarray(src).astype(dtype), np.asarray(tgt).astype(dtype)
    src_pe, tgt_pe = code(s_pcd), code(t_pcd)
    layers = []
    if cfg["entangled"]:
        src, tgt = embed_pos(pe_type, src, src_pe), embed_pos(pe_type, tgt, tgt_pe)
    for i, name in enumerate(cfg["layer_types"]):
        p = f"{prefix}layers.{i}."
        ps, pt = (None, None) if cfg["entangled"] else (src_pe, tgt_pe)
        if name == "self":
            src = attention_layer(sd, p, src, src, ps, ps, H, pe_type, dtype)
            tgt = attention_layer(sd, p, tgt, tgt, pt, pt, H, pe_type, dtype)
        elif name == "cross":
            src = attention_layer(sd, p, src, tgt, ps, pt, H, pe_type, dtype)
            tgt = attention_layer(sd, p, tgt, src, pt, ps, H, pe_type, dtype)
        elif not cfg["entangled"]:
            m = cfg["feature_matching"]
            conf, match = matching(sd, p + "0.", src, tgt, src_pe, tgt_pe, pe_type, False, m["dsmax_temperature"], m["confidence_threshold"], dtype)
            fit = soft_procrustes(conf, s_pcd, t_pcd, cfg["procrustes"]["sample_rate"], cfg["procrustes"]["max_condition_num"], dtype)
            layers.append(SimpleNamespace(conf=conf, match=match, fit=fit))
            src_pe = code((fit.R_forwd @ s_pcd.T + fit.t_forwd).T)
    return src, tgt, src_pe, tgt_pe, layers


def pipeline(sd, cfg, batch, dtype=F64):
    """Pipeline on a one-pair batch (tests/_kpfcn_ref.load_f23's) -> namespace(feats, s_pcd, t_pcd, layers, conf, match, fit)."""
    kcfg, tcfg, mcfg = cfg["kpfcn_config"], cfg["coarse_transformer"], cfg["coarse_matching"]
    feats = K.kpfcn_coarse({k[len("backbone."):]: v for k, v in sd.items() if k.startswith("backbone.")}, batch, dict(kcfg), dtype)
    level = kcfg["coarse_level"]
    pts, lens = np.asarray(batch["points"][level]).astype(dtype), [int(v) for v in batch["stack_lengths"][level]]
    assert len(lens) == 2 and sum(lens) == feats.shape[0]
    n = lens[0]
    src, tgt, src_pe, tgt_pe, layers = transformer(sd, tcfg, feats[:n], feats[n:], pts[:n], pts[n:], dtype, "coarse_transformer.")
    conf, match = matching(sd, "coarse_matching.", src, tgt, src_pe, tgt_pe, tcfg["pe_type"], mcfg["entangled"], mcfg["dsmax_temperature"],
                           mcfg["confidence_threshold"], dtype)
    fit = soft_procrustes(conf, pts[:n], pts[n:], tcfg["procrustes"]["sample_rate"], tcfg["procrustes"]["max_condition_num"], dtype)
    return SimpleNamespace(feats=feats, s_pcd=pts[:n], t_pcd=pts[n:], src=src, tgt=tgt, layers=layers, conf=conf, match=match, fit=fit)


# ------------------------------------------------------------------------------------------ the cases of tests/test_lepard.py
#          (L, S, C, H, rotary): the smallest shapes at each tile edge (16 query rows, 64 keys, 16-channel output tiles, D up to 264)
# (65, 129, 66, 2) has D = 33: a rotary code pairs the channels (2m, 2m + 1) inside a head, so an odd D is refused (tested in
# tests/test_lepard_cpu.py) and that shape runs without codes; (65, 129, 68, 2), D = 34, is the rotary case on the same unvectorised path.
ATTENTION_CASES = [(1, 1, 6, 1, True), (1, 17, 12, 2, True), (17, 1, 12, 2, True), (15, 16, 48, 4, True), (63, 65, 48, 4, True),
                   (64, 64, 64, 4, True), (65, 129, 66, 2, False), (65, 129, 68, 2, True), (129, 257, 132, 1, True), (33, 300, 528, 4, True),
                   (16, 40, 1056, 4, True), (63, 65, 48, 4, False)]
ATTENTION_BATCH = [(1, 1), (67, 31), (40, 67)]                       # three unequal problems in one call, C = 48, H = 4
CONF_SHAPES = [(1, 1), (31, 33), (257, 300)]
CONF_CS = [3, 48, 528]
_made = {}


def attention_inputs(L, S, C, H, rotary, seed=None, spread=1.0):
    """q, k, v float32 (q and k scaled so that the scaled scores are of order `spread`) and rotary codes of random angles."""
    key = (L, S, C, H, rotary, seed, spread)
    if key not in _made:
        g = np.random.default_rng(1000003 * L + 1009 * S + C if seed is None else seed)
        q, k, v = (g.standard_normal((n, C)).astype(F32) for n in (L, S, S))
        q = (q * np.sqrt(spread)).astype(F32)
        k = (k * np.sqrt(spread)).astype(F32)
        pe_q = pe_k = None
        if rotary:
            pts_q, pts_k = g.uniform(-1, 1, (L, C // 2)) * 3, g.uniform(-1, 1, (S, C // 2)) * 3
            pe_q = np.stack([np.repeat(np.cos(pts_q), 2, 1), np.repeat(np.sin(pts_q), 2, 1)], -1).astype(F32)
            pe_k = np.stack([np.repeat(np.cos(pts_k), 2, 1), np.repeat(np.sin(pts_k), 2, 1)], -1).astype(F32)
        _made[key] = SimpleNamespace(q=q, k=k, v=v, pe_q=pe_q, pe_k=pe_k, H=H)
    return _made[key]


def attention_refs(c):
    """(float64, float32) outputs of a case, computed once."""
    if not hasattr(c, "refs"):
        c.refs = tuple(attention(c.q, c.k, c.v, c.H, c.pe_q, c.pe_k, None, dt) for dt in (F64, F32))
    return c.refs


# ------------------------------------------------------------------------------------------ fixture F24
F24_LAYER_VARIANTS = ["rotary", "sinusoidal", "none"]                  # (a): C = 48, H = 4, B = 2 with prefix masks
F24_LAYER_LENS = [(21, 17), (9, 30)]                                   # (L_b, S_b) of the two problems
F24_B_CASES = ["below", "above", "batch"]                              # (b): C = 24, H = 4
F24_B_LENS = {"below": [(45, 38)], "above": [(45, 38)], "batch": [(67, 31), (40, 67)]}


def load_f24():
    return np.load(F24)


def _keys(z):
    return z.files if hasattr(z, "files") else list(z)


def sub_dict(z, prefix):
    return {k[len(prefix):]: z[k] for k in _keys(z) if k.startswith(prefix)}


def b_config():
    return transformer_config(24, 4)


def run_b(z, case, dtype=F64):
    """Fixture (b) through the restatement: one namespace(src, tgt, layers, conf, match, fit) per problem of the case."""
    cfg, p = b_config(), f"b.{case}."
    tsd, msd = sub_dict(z, p + "t.sd."), sub_dict(z, p + "m.sd.")
    res = []
    for b, (S, T) in enumerate(np.asarray(z[p + "lens"]).tolist()):
        s_pcd, t_pcd = z[p + "s_pcd"][b, :S], z[p + "t_pcd"][b, :T]
        src, tgt, src_pe, tgt_pe, layers = transformer(tsd, cfg, z[p + "src"][b, :S], z[p + "tgt"][b, :T], s_pcd, t_pcd, dtype)
        m = cfg["feature_matching"]
        conf, match = matching(msd, "", src, tgt, src_pe, tgt_pe, cfg["pe_type"], False, m["dsmax_temperature"], m["confidence_threshold"], dtype)
        fit = soft_procrustes(conf, s_pcd, t_pcd, cfg["procrustes"]["sample_rate"], cfg["procrustes"]["max_condition_num"], dtype)
        res.append(SimpleNamespace(src=src, tgt=tgt, layers=layers, conf=conf, match=match, fit=fit))
    return res


def quantities(r):
    """The compared numbers of one problem's run, by name."""
    pl = r.layers[0]
    return {"src": r.src, "tgt": r.tgt, "pl.conf": pl.conf, "pl.R": pl.fit.R, "pl.t": pl.fit.t, "pl.condition": np.asarray([pl.fit.condition]),
            "conf": r.conf, "R": r.fit.R, "t": r.fit.t, "condition": np.asarray([r.fit.condition])}


def recorded(z, prefix, b, S, T):
    """The same numbers as the fixture recorded them for problem b (valid rows only)."""
    g = lambda k: np.asarray(z[prefix + k])
    return {"src": g("out.src")[b, :S], "tgt": g("out.tgt")[b, :T], "pl.conf": g("pl.conf")[b, :S, :T], "pl.R": g("pl.R")[b], "pl.t": g("pl.t")[b],
            "pl.condition": g("pl.condition")[b:b + 1], "conf": g("conf")[b, :S, :T], "R": g("R")[b], "t": g("t")[b], "condition": g("condition")[b:b + 1]}


def bars(r64, r32):
    from ._kpconv_ref import bar
    q64, q32 = quantities(r64), quantities(r32)
    return {k: bar(np.abs(q32[k].astype(F64) - q64[k]).max(), np.abs(q64[k]).max()) for k in q64}


def b_preconditions(z, case):
    """(ok, why): every condition number at least 10 % away from max_condition_num (and, for `below` / `above`, the positioning
    layer's on that side), the confidence gap at every top-n cut above twice the bar, and the recorded float32 reference
    inside the bar of the float64 restatement with the same mask and match lists."""
    p = f"b.{case}."
    r64, r32 = run_b(z, case, F64), run_b(z, case, F32)
    lens = np.asarray(z[p + "lens"]).tolist()
    for b, (a, c) in enumerate(zip(r64, r32)):
        bb = bars(a, c)
        for name, fit, key in (("positioning", a.layers[0].fit, "pl.conf"), ("final", a.fit, "conf")):
            if abs(fit.condition / MAX_CONDITION - 1.0) < 0.1:
                return False, f"problem {b}: {name} condition {fit.condition:.2f} within 10 % of {MAX_CONDITION}"
            if not fit.gap > 2 * bb[key]:
                return False, f"problem {b}: {name} gap {fit.gap:.3e} at the cut against bar {bb[key]:.3e}"
        if case == "below" and not a.layers[0].fit.mask:
            return False, f"positioning condition {a.layers[0].fit.condition:.2f} is not below {MAX_CONDITION}"
        if case == "above" and a.layers[0].fit.mask:
            return False, f"positioning condition {a.layers[0].fit.condition:.2f} is not above {MAX_CONDITION}"
        if True:                                                     # at B = 2 as well: the fixture's problems have equal n_b
            got, want = recorded(z, p, b, *lens[b]), quantities(a)
            for k in want:
                err = float(np.abs(got[k].astype(F64) - want[k]).max())
                if not err <= bb[k]:
                    return False, f"reference float32 {k}: error {err:.3e} above bar {bb[k]:.3e}"
            if bool(np.asarray(z[p + "pl.mask"])[b]) != a.layers[0].fit.mask:
                return False, "solution_mask differs"
            for key, m in (("pl.match", a.layers[0].match), ("match", a.match)):
                rows = np.asarray(z[p + key])
                if not np.array_equal(rows[rows[:, 0] == b][:, 1:], m):
                    return False, f"{key} differs"
    return True, ""
