"""Lepard's repositioning transformer, coarse matcher, soft-Procrustes layer and pipeline (correspondence/lepard/transformer.py,
position_encoding.py, matching.py, procrustes.py, pipeline.py) on the HIP operators: the link between kpfcn.KPFCN's coarse descriptors
and the landmarks that Registration.load_pcds(..., landmarks=) and rigid.reject_landmarks take.  The modules carry the reference's
parameter names, so the state dict of its `Pipeline` loads with load_state_dict(strict=True).  Inference calls are no_grad;
GeometryAttentionLayer.forward_grad is the layer recorded for autograd (ops.attention_fn); the rest of the pipeline is forward only.

What runs where: every attention is one ops.attention call (csrc/ndp_attention.inc: the rotary code is applied while q and k are
staged, the L x S x H scores are never stored); the confidence matrix is ops.feat_conf and the match list ops.feat_match
(csrc/ndp_match.inc); the weighted Procrustes is ops.rigid_fit (csrc/ndp_rigid.inc, double).  The Linear and LayerNorm layers, the
position codes and the top-n selection of the soft-Procrustes layer are torch ops on the device.

Problems are UNPADDED: a batch is the problems' rows stacked, [sum S, C], with their lengths.  On valid rows that equals the
reference's masked batch; a padded row never reaches a valid row's soft-max, LayerNorm or Linear.  pad() / unpad() convert.

Two deliberate deviations (DESIGN.md "Attention"): the soft-Procrustes layer takes the n_b = int(max(S_b, T_b) * sample_rate) most
confident entries of EACH problem, where the reference takes the batch mean of that number for all of them (equal at B = 1 and for
equal n_b); and torch.topk, like the reference's unstable sort, is free among equal confidences.

Not served: `match_type: sinkhorn` as a confidence matrix (matching.sinkhorn_match gives its match list), `positioning_type:
randSO3` (a training augmentation), the backward of ops.feat_conf and ops.rigid_fit (so the pipeline as a whole is not trainable).  Parity with a trained Lepard checkpoint is unverified: none is available."""
import math

import torch
import torch.nn as nn

from . import kpconv, kpfcn, ops
from .matching import _offsets


def _get(config, key):
    """The reference reads its config as config['x'] and as config.x; take either."""
    return config[key] if isinstance(config, dict) else getattr(config, key)


def unpad(x, mask):
    """x [B, N, ...] with a prefix mask [B, N] -> (the valid rows stacked [sum N_b, ...], [N_b])."""
    lens = [int(n) for n in mask.sum(1).tolist()]
    return torch.cat([x[b, :n] for b, n in enumerate(lens)]).contiguous(), lens


def pad(rows, lens):
    """Stacked rows [sum N_b, ...] -> [B, max N_b, ...] with zeros behind every problem."""
    out = rows.new_zeros((len(lens), max(lens)) + tuple(rows.shape[1:]))
    off = _offsets(lens)
    for b, n in enumerate(lens):
        out[b, :n] = rows[off[b]:off[b + 1]]
    return out


def _row_problem(lens, device):
    """[sum N_b] int64: the problem of every stacked row."""
    return torch.repeat_interleave(torch.arange(len(lens), device=device), torch.tensor(lens, device=device))


class VolumetricPositionEncoding(nn.Module):
    """xyz [..., 3] -> the position code of the voxel coordinates (xyz - vol_bnds[0]) / voxel_size, a third of the channels per axis
    with frequencies 10000 ** (-2 m / (C / 3)): "sinusoidal" [..., C] = (sin x, cos x, sin y, cos y, sin z, cos z); "rotary"
    [..., C, 2] = (cos, sin) with every angle on two neighbouring channels, x then y then z."""

    def __init__(self, config):
        super().__init__()
        self.feature_dim, self.vol_bnds, self.voxel_size = _get(config, "feature_dim"), _get(config, "vol_bnds"), _get(config, "voxel_size")
        self.vol_origin, self.pe_type = self.vol_bnds[0], _get(config, "pe_type")
        if self.pe_type not in ("rotary", "sinusoidal"):
            raise KeyError(f"pe_type must be rotary or sinusoidal, got {self.pe_type!r}")
        if self.feature_dim % 6 != 0:
            raise ValueError(f"a volumetric position code needs feature_dim % 6 == 0 (a sine and a cosine per axis), got {self.feature_dim}")

    def voxelize(self, xyz):
        origin = torch.tensor(self.vol_origin, dtype=torch.float32, device=xyz.device)        # the reference's FloatTensor, whatever xyz is
        return (xyz - origin.to(xyz.dtype)) / self.voxel_size

    @staticmethod
    def embed_rotary(x, cos, sin):
        x2 = torch.stack([-x[..., 1::2], x[..., ::2]], dim=-1).reshape(x.shape)
        return x * cos + x2 * sin

    @staticmethod
    def embed_pos(pe_type, x, pe):
        if pe_type == "rotary":
            return VolumetricPositionEncoding.embed_rotary(x, pe[..., 0], pe[..., 1])
        if pe_type == "sinusoidal":
            return x + pe
        raise KeyError(pe_type)

    def forward(self, xyz):
        third = self.feature_dim // 3
        div = torch.exp(torch.arange(0, third, 2, dtype=torch.float, device=xyz.device) * (-math.log(10000.0) / third)).to(xyz.dtype)
        ang = self.voxelize(xyz)[..., :, None] * div                                 # [..., 3, C / 6]
        sin, cos = torch.sin(ang), torch.cos(ang)
        lead = xyz.shape[:-1]
        if self.pe_type == "sinusoidal":
            return torch.stack([sin, cos], dim=-2).reshape(*lead, -1).detach()       # per axis: its sines, then its cosines
        sin2 = torch.stack([sin, sin], dim=-1).reshape(*lead, -1)                    # every angle twice, x | y | z
        cos2 = torch.stack([cos, cos], dim=-1).reshape(*lead, -1)
        return torch.stack([cos2, sin2], dim=-1).detach()


class GeometryAttentionLayer(nn.Module):
    """forward(x [sum L, C], source [sum S, C], x_pe, source_pe, x_lens, source_lens): attention of x's rows over source's rows of
    the same problem, merge, LayerNorm, the two-layer MLP on (x, message), LayerNorm, residual."""

    def __init__(self, config):
        super().__init__()
        d_model, nhead = _get(config, "feature_dim"), _get(config, "n_head")
        if d_model % nhead != 0:
            raise ValueError(f"feature_dim {d_model} must be a multiple of n_head {nhead}")
        self.dim, self.nhead, self.pe_type = d_model // nhead, nhead, _get(config, "pe_type")
        if self.pe_type not in ("rotary", "sinusoidal"):
            raise KeyError(f"pe_type must be rotary or sinusoidal, got {self.pe_type!r}")
        if self.pe_type == "rotary" and self.dim % 2 != 0:
            raise ValueError(f"a rotary code needs an even head dimension, got feature_dim / n_head = {self.dim}")
        self.q_proj = nn.Linear(d_model, d_model, bias=False)
        self.k_proj = nn.Linear(d_model, d_model, bias=False)
        self.v_proj = nn.Linear(d_model, d_model, bias=False)
        self.merge = nn.Linear(d_model, d_model, bias=False)
        self.mlp = nn.Sequential(nn.Linear(d_model * 2, d_model * 2, bias=False), nn.ReLU(True), nn.Linear(d_model * 2, d_model, bias=False))
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    @torch.no_grad()
    def forward(self, x, source, x_pe, source_pe, x_lens=None, source_lens=None):
        return self._run(ops.attention, x, source, x_pe, source_pe, x_lens, source_lens)

    def forward_grad(self, x, source, x_pe, source_pe, x_lens=None, source_lens=None):
        """forward's value, recorded for autograd: differentiable in x, source and the layer's parameters (ops.attention_fn)."""
        with torch.enable_grad():
            return self._run(ops.attention_fn, x, source, x_pe, source_pe, x_lens, source_lens)

    def _run(self, attention, x, source, x_pe, source_pe, x_lens, source_lens):
        q, k, v = x, source, source
        pe_q = pe_k = None
        if self.pe_type == "sinusoidal":
            if x_pe is not None:
                q, k = q + x_pe, k + source_pe
        elif x_pe is not None:
            pe_q, pe_k = x_pe, source_pe
        o = attention(self.q_proj(q), self.k_proj(k), self.v_proj(v), self.nhead, pe_q=pe_q, pe_k=pe_k,
                      offsets_q=None if x_lens is None else _offsets(x_lens), offsets_k=None if source_lens is None else _offsets(source_lens))
        message = self.norm1(self.merge(o))
        message = self.norm2(self.mlp(torch.cat([x, message], dim=1)))
        return x + message


class Matching(nn.Module):
    """forward(src_feats [sum S, C], tgt_feats [sum T, C], src_pe, tgt_pe, src_lens, tgt_lens, data, pe_type) ->
    (conf_matrix [B, Smax, Tmax], index [M, 3] int64 rows (b, s, t)).  `src_proj` is applied to BOTH sides, as the reference does
    (matching.py:127-128); `tgt_proj` exists so that checkpoints load."""

    def __init__(self, config):
        super().__init__()
        self.match_type, self.confidence_threshold = _get(config, "match_type"), _get(config, "confidence_threshold")
        d_model = _get(config, "feature_dim")
        self.src_proj = nn.Linear(d_model, d_model, bias=False)
        self.tgt_proj = nn.Linear(d_model, d_model, bias=False)
        self.entangled = _get(config, "entangled")
        if self.match_type == "dual_softmax":
            self.temperature = _get(config, "dsmax_temperature")
        elif self.match_type == "sinkhorn":
            raise NotImplementedError("match_type sinkhorn: its confidence MATRIX is not served (matching.sinkhorn_match gives the match list)")
        else:
            raise NotImplementedError(f"match_type {self.match_type!r}")

    @torch.no_grad()
    def forward(self, src_feats, tgt_feats, src_pe, tgt_pe, src_lens=None, tgt_lens=None, data=None, pe_type="rotary"):
        src_lens = [src_feats.shape[0]] if src_lens is None else src_lens
        tgt_lens = [tgt_feats.shape[0]] if tgt_lens is None else tgt_lens
        src_feats, tgt_feats = self.src_proj(src_feats), self.src_proj(tgt_feats)
        if data is not None:
            data["src_feats_nopos"], data["tgt_feats_nopos"] = src_feats, tgt_feats
        if not self.entangled:
            src_feats = VolumetricPositionEncoding.embed_pos(pe_type, src_feats, src_pe)
            tgt_feats = VolumetricPositionEncoding.embed_pos(pe_type, tgt_feats, tgt_pe)
        src_feats, tgt_feats = src_feats.contiguous(), tgt_feats.contiguous()
        if data is not None:
            data["src_feats"], data["tgt_feats"] = src_feats, tgt_feats
        off_s, off_t = _offsets(src_lens), _offsets(tgt_lens)
        conf = ops.feat_conf(src_feats, tgt_feats, self.temperature, offsets_s=off_s, offsets_t=off_t)
        match_t, _ = ops.feat_match(src_feats, tgt_feats, mode="dual_softmax", temperature=self.temperature, thr=self.confidence_threshold,
                                    mutual=True, offsets_s=off_s, offsets_t=off_t)
        rows = (match_t >= 0).nonzero()[:, 0]                     # matching._match's compaction: rows (b, s, t) in ascending (b, s)
        bounds = torch.tensor(off_s, device=rows.device)
        b = torch.bucketize(rows, bounds[1:], right=True)
        return conf, torch.stack([b, rows - bounds[b], match_t[rows].long()], 1)


class SoftProcrustesLayer(nn.Module):
    """forward(conf_matrix [B, Smax, Tmax], src_pcd [sum S, 3], tgt_pcd [sum T, 3], src_lens, tgt_lens) ->
    (R [B,3,3], t [B,3,1], R_forwd, t_forwd, condition [B], solution_mask [B]): the weighted Procrustes of each problem's n_b most
    confident pairs, and identity / zero in R_forwd, t_forwd where the condition number is not below max_condition_num or the fit
    reports a status."""

    def __init__(self, config):
        super().__init__()
        self.sample_rate, self.max_condition_num = _get(config, "sample_rate"), _get(config, "max_condition_num")

    @torch.no_grad()
    def forward(self, conf_matrix, src_pcd, tgt_pcd, src_lens=None, tgt_lens=None):
        src_lens = [src_pcd.shape[0]] if src_lens is None else src_lens
        tgt_lens = [tgt_pcd.shape[0]] if tgt_lens is None else tgt_lens
        B, _, M = conf_matrix.shape
        off_s, off_t = _offsets(src_lens), _offsets(tgt_lens)
        xs, ys, ws, off = [], [], [], [0]
        for b in range(B):
            n = min(int(max(src_lens[b], tgt_lens[b]) * self.sample_rate), src_lens[b] * tgt_lens[b])
            w, idx = torch.topk(conf_matrix[b, :src_lens[b], :tgt_lens[b]].reshape(-1), n)
            xs.append(src_pcd[off_s[b] + idx // tgt_lens[b]])
            ys.append(tgt_pcd[off_t[b] + idx % tgt_lens[b]])
            ws.append(w)
            off.append(off[-1] + n)
        R, t, condition, status = ops.rigid_fit(torch.cat(xs).float().contiguous(), torch.cat(ys).float().contiguous(),
                                                w=torch.cat(ws).float().contiguous(), eps=1e-4, offsets=off)
        solution_mask = (condition < self.max_condition_num) & (status == 0)
        t = t[:, :, None]
        R_forwd, t_forwd = R.clone(), t.clone()
        R_forwd[~solution_mask] = torch.eye(3, device=R.device, dtype=R.dtype)
        t_forwd[~solution_mask] = 0.0
        return R, t, R_forwd, t_forwd, condition, solution_mask


def _transform(R, t, pcd, lens):
    """Per problem R_b p + t_b on stacked points."""
    b = _row_problem(lens, pcd.device)
    return (R[b] @ pcd[:, :, None] + t[b])[:, :, 0]


class RepositioningTransformer(nn.Module):
    """forward(src_feat [sum S, C], tgt_feat [sum T, C], s_pcd [sum S, 3], t_pcd [sum T, 3], src_lens, tgt_lens, data, T=None) ->
    (src_feat, tgt_feat, src_pe, tgt_pe); fills data["position_layers"][1, 2, ..] with conf_matrix, match_pred, R_s2t_pred,
    t_s2t_pred, solution_mask, condition of every positioning layer."""

    def __init__(self, config):
        super().__init__()
        self.d_model, self.nhead = _get(config, "feature_dim"), _get(config, "n_head")
        self.layer_types, self.positioning_type = list(_get(config, "layer_types")), _get(config, "positioning_type")
        self.pe_type, self.entangled = _get(config, "pe_type"), _get(config, "entangled")
        if self.positioning_type == "randSO3":
            raise NotImplementedError("positioning_type randSO3 is a training augmentation and is not served")
        if self.positioning_type not in ("procrustes", "oracle"):
            raise KeyError(f"{self.positioning_type} undefined positional encoding type")
        self.positional_encoding = VolumetricPositionEncoding(config)
        self.layers = nn.ModuleList()
        for l_type in self.layer_types:
            if l_type in ("self", "cross"):
                self.layers.append(GeometryAttentionLayer(config))
            elif l_type == "positioning":
                if self.positioning_type == "procrustes":
                    self.layers.append(nn.ModuleList([Matching(_get(config, "feature_matching")), SoftProcrustesLayer(_get(config, "procrustes"))]))
                else:
                    self.layers.append(None)
            else:
                raise KeyError(f"layer type {l_type!r}")
        for p in self.parameters():
            if p.dim() > 1:
                nn.init.xavier_uniform_(p)

    @torch.no_grad()
    def forward(self, src_feat, tgt_feat, s_pcd, t_pcd, src_lens=None, tgt_lens=None, data=None, T=None):
        src_lens = [src_feat.shape[0]] if src_lens is None else src_lens
        tgt_lens = [tgt_feat.shape[0]] if tgt_lens is None else tgt_lens
        data = {} if data is None else data
        if self.d_model != src_feat.shape[1]:
            raise ValueError(f"the transformer was built for {self.d_model} channels, the features have {src_feat.shape[1]}")
        src_pe = self.positional_encoding(s_pcd if T is None else _transform(T[0], T[1], s_pcd, src_lens))
        tgt_pe = self.positional_encoding(t_pcd)
        data["position_layers"] = {}
        if self.entangled:
            src_feat = VolumetricPositionEncoding.embed_pos(self.pe_type, src_feat, src_pe)
            tgt_feat = VolumetricPositionEncoding.embed_pos(self.pe_type, tgt_feat, tgt_pe)
        position_layer = 0
        for layer, name in zip(self.layers, self.layer_types):
            pe_s, pe_t = (None, None) if self.entangled else (src_pe, tgt_pe)
            if name == "self":
                src_feat = layer(src_feat, src_feat, pe_s, pe_s, src_lens, src_lens)
                tgt_feat = layer(tgt_feat, tgt_feat, pe_t, pe_t, tgt_lens, tgt_lens)
            elif name == "cross":
                src_feat = layer(src_feat, tgt_feat, pe_s, pe_t, src_lens, tgt_lens)
                tgt_feat = layer(tgt_feat, src_feat, pe_t, pe_s, tgt_lens, src_lens)
            elif self.entangled:
                continue                                             # the reference's entangled branch skips positioning
            elif self.positioning_type == "procrustes":
                conf_matrix, match_pred = layer[0](src_feat, tgt_feat, src_pe, tgt_pe, src_lens, tgt_lens, data, pe_type=self.pe_type)
                position_layer += 1
                R, t, R_forwd, t_forwd, condition, solution_mask = layer[1](conf_matrix, s_pcd, t_pcd, src_lens, tgt_lens)
                data["position_layers"][position_layer] = {"conf_matrix": conf_matrix, "match_pred": match_pred, "R_s2t_pred": R,
                                                           "t_s2t_pred": t, "solution_mask": solution_mask, "condition": condition}
                src_pe = self.positional_encoding(_transform(R_forwd, t_forwd, s_pcd, src_lens))
                tgt_pe = self.positional_encoding(t_pcd)
            else:                                                    # oracle: the ground-truth pose, for the position code only
                src_pe = self.positional_encoding(_transform(data["batched_rot"], data["batched_trn"], s_pcd, src_lens))
                tgt_pe = self.positional_encoding(t_pcd)
        return src_feat, tgt_feat, src_pe, tgt_pe


class Pipeline(nn.Module):
    """pipeline.py's Pipeline: backbone (kpfcn.KPFCN), coarse_transformer, coarse_matching, soft_procrustes.  forward(batch) takes a
    kpconv.build_pyramid batch with `features`; the clouds alternate (src_0, tgt_0, src_1, tgt_1, ..), as the reference's collate
    stacks them, and the split is read from stack_lengths at kpfcn_config.coarse_level.  It adds s_pcd / t_pcd (stacked), src_lengths
    / tgt_lengths, position_layers, conf_matrix_pred [B, Smax, Tmax], coarse_match_pred [M, 3], R_s2t_pred, t_s2t_pred to the batch."""

    def __init__(self, config):
        super().__init__()
        self.config = config
        kcfg, tcfg = _get(config, "kpfcn_config"), _get(config, "coarse_transformer")
        self.coarse_level = _get(kcfg, "coarse_level")
        self.backbone = kpfcn.KPFCN(kcfg)
        self.pe_type, self.positioning_type = _get(tcfg, "pe_type"), _get(tcfg, "positioning_type")
        self.coarse_transformer = RepositioningTransformer(tcfg)
        self.coarse_matching = Matching(_get(config, "coarse_matching"))
        self.soft_procrustes = SoftProcrustesLayer(_get(tcfg, "procrustes"))

    def split_feats(self, feats, data):
        pcd = data["points"][self.coarse_level]
        lens = [int(v) for v in data["stack_lengths"][self.coarse_level]]
        if len(lens) % 2 != 0 or sum(lens) != feats.shape[0]:
            raise ValueError(f"the coarse level must hold (src, tgt) pairs of {feats.shape[0]} points in all, got lengths {lens}")
        off = _offsets(lens)
        src = torch.cat([torch.arange(off[i], off[i + 1]) for i in range(0, len(lens), 2)]).to(feats.device)
        tgt = torch.cat([torch.arange(off[i], off[i + 1]) for i in range(1, len(lens), 2)]).to(feats.device)
        return feats[src].contiguous(), feats[tgt].contiguous(), pcd[src].contiguous(), pcd[tgt].contiguous(), lens[0::2], lens[1::2]

    @torch.no_grad()
    def forward(self, data):
        feats = self.backbone(data, phase="coarse")
        src_feats, tgt_feats, s_pcd, t_pcd, src_lens, tgt_lens = self.split_feats(feats, data)
        data.update({"s_pcd": s_pcd, "t_pcd": t_pcd, "src_lengths": src_lens, "tgt_lengths": tgt_lens})
        src_feats, tgt_feats, src_pe, tgt_pe = self.coarse_transformer(src_feats, tgt_feats, s_pcd, t_pcd, src_lens, tgt_lens, data)
        conf, match = self.coarse_matching(src_feats, tgt_feats, src_pe, tgt_pe, src_lens, tgt_lens, data, pe_type=self.pe_type)
        data.update({"conf_matrix_pred": conf, "coarse_match_pred": match})
        R, t, _, _, _, _ = self.soft_procrustes(conf, s_pcd, t_pcd, src_lens, tgt_lens)
        data.update({"R_s2t_pred": R, "t_s2t_pred": t})
        return data


@torch.no_grad()
def run_pair(pipeline, src, tgt, neighborhood_limits):
    """Two clouds src [N,3], tgt [M,3] on the device -> the pipeline's batch of that one pair (Pipeline.forward's keys)."""
    kcfg = _get(pipeline.config, "kpfcn_config")
    points = torch.cat([src, tgt]).float().contiguous()
    batch = kpconv.build_pyramid(points, [src.shape[0], tgt.shape[0]], _get(kcfg, "first_subsampling_dl"), _get(kcfg, "conv_radius"),
                                 _get(kcfg, "deform_radius"), _get(kcfg, "architecture"), neighborhood_limits)
    batch["features"] = torch.ones(points.shape[0], 1, device=points.device)
    return pipeline(batch)


@torch.no_grad()
def predict_landmarks(pipeline, src, tgt, neighborhood_limits):
    """Two clouds src [N,3], tgt [M,3] on the device -> (ldmk_s [K,3], ldmk_t [K,3], conf [K], R [3,3], t [3]): the coarse points of
    the pipeline's mutual matches in ascending source order with their confidences, and the soft-Procrustes pose.  The landmarks are
    what Registration.load_pcds(..., landmarks=), rigid.reject_landmarks and outlier.reject_landmarks take."""
    out = run_pair(pipeline, src, tgt, neighborhood_limits)
    index = out["coarse_match_pred"]
    i, j = index[:, 1], index[:, 2]
    return (out["s_pcd"][i].contiguous(), out["t_pcd"][j].contiguous(), out["conf_matrix_pred"][0, i, j], out["R_s2t_pred"][0],
            out["t_s2t_pred"][0, :, 0])
