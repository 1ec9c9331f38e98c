"""The reference's learned outlier filter (correspondence/outlier_rejection/pipeline.py, geometry_attention.py, position_encoding.py,
loss.py) and its Landmark_Model (correspondence/landmark_estimator.py) on the HIP operators: the link between lepard.Pipeline's
match list and the landmarks that Registration.load_pcds(..., landmarks=) takes.  The modules carry the reference's parameter
names, so the state dict of its `Outlier_Rejection` loads with load_state_dict(strict=True).  forward / confidence are inference
calls (no_grad); forward_grad / confidence_grad are the same values recorded for autograd on ops.attention_fn, and NeCoLoss,
synthetic_matches and train_step are what tools/outlier_train.py trains the filter with.

What runs where: every one of the network's layers is one ops.attention call with pos_q = pos_k = vec_6d and sigma_spat
(csrc/ndp_attention.inc, ndp_attention_compat_forward): the spatial compatibility c[i, j] = max(0, 1 - (|s_i - s_j| - |t_i - t_j|)^2 /
sigma_spat^2) of two correspondences is taken on the chip between the score product and the soft-max, so neither the reference's
[B, M, M, 3] differences, its [B, M, M] distances and c, nor a [B, M, M, H] score tensor exists.  The Linear and LayerNorm layers,
the position code and the classification head are torch ops on the device.

Problems are UNPADDED, as in lepard.py: vec_6d is the pairs' matches stacked, [sum M_b, 6], with their lengths.  On valid rows
that equals the reference's padded batch (_3D_to_6D): a padded row never reaches a valid row's soft-max, LayerNorm or Linear.  A
pair without matches is left out of the kernel call and gets an empty confidence.

Parity with the reference's own trained checkpoint is unverified: none is available."""
import copy
import math

import numpy as np
import torch
import torch.nn as nn

from . import lepard, ops, synthetic
from .lepard import _get
from .matching import _offsets

DEFAULT_CONFIG = {"in_dim": 6, "num_layers": 9, "feature_dim": 144, "n_head": 8, "pe_type": "rotary", "voxel_size": 0.08,
                  "sigma_spat": 0.1, "spatial_consistency_check": True}       # correspondence/configs/outlier_rejection.yaml
PE_TYPES = ("rotary", "sinusoidal", "none")


class VolumetricPositionEncoding(nn.Module):
    """vec_6d [..., 6] = (s_xyz, t_xyz) -> the 6-D position code: each side gets feature_dim // 2 channels, the code of its voxel
    coordinates xyz / voxel_size (no volume origin) with a third of a side's channels per axis and the frequencies
    10000 ** (-2 m / (feature_dim // 2 // 3)); the two sides are concatenated along the channel.  "sinusoidal" [..., C] = per side
    (sin x, cos x, sin y, cos y, sin z, cos z); "rotary" [..., C, 2] = (cos, sin) with every angle on two neighbouring channels.
    With pe_type "none" there is no code: forward returns None."""

    def __init__(self, config):
        super().__init__()
        full = _get(config, "feature_dim")
        self.feature_dim, self.voxel_size, self.pe_type = full // 2, _get(config, "voxel_size"), _get(config, "pe_type")
        if self.pe_type not in PE_TYPES:
            raise KeyError(f"pe_type must be one of {PE_TYPES}, got {self.pe_type!r}")
        if self.pe_type != "none" and full % 12 != 0:
            raise ValueError(f"a 6-D position code needs feature_dim % 12 == 0 (two sides, three axes, a sine and a cosine), got {full}")

    embed_rotary = staticmethod(lepard.VolumetricPositionEncoding.embed_rotary)
    embed_pos = staticmethod(lepard.VolumetricPositionEncoding.embed_pos)

    def voxelize(self, xyz):
        return xyz / self.voxel_size

    def pe(self, xyz):
        third = self.feature_dim // 3
        div = torch.exp(torch.arange(0, third, 2, dtype=torch.float, device=xyz.device) * (-math.log(10000.0) / third)).to(xyz.dtype)
        ang = self.voxelize(xyz)[..., :, None] * div                                 # [..., 3, C / 12]
        sin, cos = torch.sin(ang), torch.cos(ang)
        lead = xyz.shape[:-1]
        if self.pe_type == "sinusoidal":
            return torch.stack([sin, cos], dim=-2).reshape(*lead, -1)                # per axis: its sines, then its cosines
        sin2 = torch.stack([sin, sin], dim=-1).reshape(*lead, -1)                    # every angle twice, x | y | z
        cos2 = torch.stack([cos, cos], dim=-1).reshape(*lead, -1)
        return torch.stack([cos2, sin2], dim=-1)

    def forward(self, vec6d):
        if self.pe_type == "none":
            return None
        if vec6d.shape[-1] != 6:
            raise ValueError(f"vec_6d must be [..., 6] (source xyz, target xyz), got {tuple(vec6d.shape)}")
        s_pe, t_pe = self.pe(vec6d[..., :3]), self.pe(vec6d[..., 3:])
        return torch.cat([s_pe, t_pe], dim=-1 if self.pe_type == "sinusoidal" else -2).detach().contiguous()


class CorrespondenceAttentionLayer(nn.Module):
    """forward(x [sum L, C], source [sum S, C], x_pe, source_pe, x_lens, source_lens, x_pos [sum L, 6], source_pos [sum S, 6]):
    lepard.GeometryAttentionLayer's structure -- attention, merge, LayerNorm, the two-layer MLP on (x, message), LayerNorm, residual
    -- with every score multiplied by the compatibility of the rows' positions when config.spatial_consistency_check is on (the
    positions are needed then), and the plain attention when it is off."""

    def __init__(self, config):
        super().__init__()
        d_model, nhead = _get(config, "feature_dim"), _get(config, "n_head")
        if d_model % nhead != 0:
            raise ValueError(f"feature_dim {d_model} must be a multiple of n_head {nhead}")
        self.dim, self.nhead, self.pe_type = d_model // nhead, nhead, _get(config, "pe_type")
        if self.pe_type not in PE_TYPES:
            raise KeyError(f"pe_type must be one of {PE_TYPES}, got {self.pe_type!r}")
        if self.pe_type == "rotary" and self.dim % 2 != 0:
            raise ValueError(f"a rotary code needs an even head dimension, got feature_dim / n_head = {self.dim}")
        self.spatial_consistency_check, self.sigma_spat = bool(_get(config, "spatial_consistency_check")), float(_get(config, "sigma_spat"))
        if self.spatial_consistency_check and not self.sigma_spat > 0:
            raise ValueError(f"sigma_spat must be positive, got {self.sigma_spat}")
        self.q_proj = nn.Linear(d_model, d_model, bias=False)
        self.k_proj = nn.Linear(d_model, d_model, bias=False)
        self.v_proj = nn.Linear(d_model, d_model, bias=False)
        self.merge = nn.Linear(d_model, d_model, bias=False)
        self.mlp = nn.Sequential(nn.Linear(d_model * 2, d_model * 2, bias=False), nn.ReLU(True), nn.Linear(d_model * 2, d_model, bias=False))
        self.norm1 = nn.LayerNorm(d_model)
        self.norm2 = nn.LayerNorm(d_model)

    @torch.no_grad()
    def forward(self, x, source, x_pe, source_pe, x_lens=None, source_lens=None, x_pos=None, source_pos=None):
        return self._run(ops.attention, x, source, x_pe, source_pe, x_lens, source_lens, x_pos, source_pos)

    def forward_grad(self, x, source, x_pe, source_pe, x_lens=None, source_lens=None, x_pos=None, source_pos=None):
        """forward's value, recorded for autograd: differentiable in x, source and the layer's parameters (ops.attention_fn)."""
        with torch.enable_grad():
            return self._run(ops.attention_fn, x, source, x_pe, source_pe, x_lens, source_lens, x_pos, source_pos)

    def _run(self, attention, x, source, x_pe, source_pe, x_lens, source_lens, x_pos, source_pos):
        q, k, v = x, source, source
        pe_q = pe_k = None
        if x_pe is not None:
            if self.pe_type == "sinusoidal":
                q, k = q + x_pe, k + source_pe
            elif self.pe_type == "rotary":
                pe_q, pe_k = x_pe, source_pe
        compat = {}
        if self.spatial_consistency_check:
            if x_pos is None or source_pos is None:
                raise ValueError("spatial_consistency_check is on: the layer needs the rows' 6-D positions")
            compat = {"pos_q": x_pos, "pos_k": source_pos, "sigma_spat": self.sigma_spat}
        o = attention(self.q_proj(q), self.k_proj(k), self.v_proj(v), self.nhead, pe_q=pe_q, pe_k=pe_k,
                      offsets_q=None if x_lens is None else _offsets(x_lens), offsets_k=None if source_lens is None else _offsets(source_lens),
                      **compat)
        message = self.norm1(self.merge(o))
        message = self.norm2(self.mlp(torch.cat([x, message], dim=1)))
        return x + message


class Outlier_Rejection(nn.Module):
    """pipeline.py's Outlier_Rejection: in_proj, num_layers CorrespondenceAttentionLayers, the 64 -> 32 -> 1 classification head.
    forward(data) takes the matcher's batch -- s_pcd [sum S, 3], t_pcd [sum T, 3] stacked, src_lengths, tgt_lengths,
    coarse_match_pred [M, 3] int64 rows (b, s, t) -- adds vec_6d [sum M_b, 6], vec_6d_lengths [M_b], vec_6d_ind [sum M_b, 2] and
    inlier_conf to it and returns (confidence [sum M_b], [M_b])."""

    def __init__(self, config):
        super().__init__()
        self.num_layers, self.pe_type = _get(config, "num_layers"), _get(config, "pe_type")
        self.in_proj = nn.Linear(_get(config, "in_dim"), _get(config, "feature_dim"), bias=True)
        sa_layer = CorrespondenceAttentionLayer(config)
        self._6D_geometry_layers = nn.ModuleList()
        self.positional_encoding = VolumetricPositionEncoding(config)
        self.sigma_spat, self.spatial_consistency_check = _get(config, "sigma_spat"), _get(config, "spatial_consistency_check")
        for _ in range(self.num_layers):
            self._6D_geometry_layers.append(copy.deepcopy(sa_layer))
        self.classification = nn.Sequential(nn.Linear(_get(config, "feature_dim"), 64, bias=True), nn.ReLU(), nn.Linear(64, 32, bias=True),
                                            nn.ReLU(), nn.Linear(32, 1, bias=True), nn.Sigmoid())

    @staticmethod
    def _3D_to_6D(data):
        """The reference's _3D_to_6D without the padding: the matches grouped by pair in their given order."""
        src_lens, tgt_lens = list(data["src_lengths"]), list(data["tgt_lengths"])
        ind = data["coarse_match_pred"]
        if ind.ndim != 2 or ind.shape[1] != 3:
            raise ValueError(f"coarse_match_pred must be [M, 3] rows (b, s, t), got {tuple(ind.shape)}")
        B = len(src_lens)
        order = torch.argsort(ind[:, 0], stable=True)
        bi, si, ti = ind[order, 0], ind[order, 1], ind[order, 2]
        lens = torch.bincount(bi, minlength=B).tolist() if ind.shape[0] else [0] * B
        if len(lens) != B:
            raise ValueError(f"coarse_match_pred names pair {len(lens) - 1} of a batch of {B}")
        off_s = torch.tensor(_offsets(src_lens), device=ind.device)
        off_t = torch.tensor(_offsets(tgt_lens), device=ind.device)
        vec_6d = torch.cat([data["s_pcd"][off_s[bi] + si], data["t_pcd"][off_t[bi] + ti]], dim=1).contiguous()
        data.update({"vec_6d": vec_6d, "vec_6d_lengths": lens, "vec_6d_ind": torch.stack([si, ti], dim=-1)})
        return vec_6d, lens

    @torch.no_grad()
    def confidence(self, vec_6d, lens):
        """vec_6d [sum M_b, 6] stacked with its per-pair lengths (zeros allowed) -> the inlier confidence of every row [sum M_b]."""
        return self._confidence(vec_6d, lens, False)

    def confidence_grad(self, vec_6d, lens):
        """confidence's value, recorded for autograd: differentiable in every parameter of the network (training)."""
        with torch.enable_grad():
            return self._confidence(vec_6d, lens, True)

    def _confidence(self, vec_6d, lens, grad):
        if vec_6d.shape[0] != sum(lens):
            raise ValueError(f"the lengths {lens} must sum to the {vec_6d.shape[0]} rows of vec_6d")
        if vec_6d.shape[0] == 0:
            return vec_6d.new_zeros(0)                                                # no matches at all: nothing is launched
        lens = [n for n in lens if n > 0]                                             # a pair without matches is no problem of the call
        vec_6d = vec_6d.float().contiguous()
        pe_6d = self.positional_encoding(vec_6d)
        feat = self.in_proj(vec_6d)
        for layer in self._6D_geometry_layers:
            feat = (layer.forward_grad if grad else layer)(feat, feat, pe_6d, pe_6d, lens, lens, vec_6d, vec_6d)
        return self.classification(feat).squeeze(-1)

    @torch.no_grad()
    def forward(self, data):
        vec_6d, lens = self._3D_to_6D(data)
        data["inlier_conf"] = self.confidence(vec_6d, lens)
        return data["inlier_conf"], lens


@torch.no_grad()
def compute_inlier_mask(data, inlier_thr, s2t_flow, rot, trn):
    """NeCoLoss.compute_inlier_mask on the stacked layout: s2t_flow [sum S, 3] on data["s_pcd"], rot [B, 3, 3], trn [B, 3, 1]; a
    match is an inlier when its warped source end rot (s + flow) + trn lies within inlier_thr of its target end.  Needs the
    vec_6d, vec_6d_lengths and vec_6d_ind of Outlier_Rejection.forward -> ([mask_b [M_b] bool], [rate_b]); the rate of a pair
    without matches is NaN, the reference's 0 / 0."""
    src_lens = list(data["src_lengths"])
    s_pcd = data["s_pcd"]
    warped = lepard._transform(rot.to(s_pcd.dtype), trn.to(s_pcd.dtype).reshape(-1, 3, 1), s_pcd + s2t_flow, src_lens)
    lens, off_s = data["vec_6d_lengths"], _offsets(src_lens)
    off_m = _offsets(lens)
    masks, rates = [], []
    for b, n in enumerate(lens):
        rows = slice(off_m[b], off_m[b + 1])
        diff = warped[off_s[b] + data["vec_6d_ind"][rows, 0]] - data["vec_6d"][rows, 3:]
        inlier = torch.sum(diff ** 2, dim=1) < inlier_thr ** 2
        masks.append(inlier)
        rates.append(inlier.sum().float() / n if n else inlier.new_tensor(float("nan"), dtype=torch.float32))
    return masks, rates


class NeCoLoss(nn.Module):
    """loss.py's NeCoLoss on the stacked layout.  forward(data) takes what Outlier_Rejection.forward left in data (vec_6d,
    vec_6d_lengths, vec_6d_ind; inlier_conf [sum M_b] -- from confidence_grad when the loss is to be differentiated) and the ground
    truth: coarse_flow, a list of [S_b, 3] flows on the pairs' coarse source points, batched_rot [B, 3, 3], batched_trn [B, 3, 1]
    -> {"loss", "IR Lepard", "IR NeCo"}: the class-weighted BCE against compute_inlier_mask's labels, the matcher's inlier rate
    and the inlier rate of the matches with confidence above 0.5 (the mean over the pairs that keep any; 0 when none does)."""

    def __init__(self, config):
        super().__init__()
        self.inlier_thr = _get(config, "inlier_thr")
        self.mutual_nearest, self.dataset, self.balanced = (_get(config, key) for key in ("mutual_nearest", "dataset", "balanced_bce"))

    def forward(self, data):
        masks, rates = compute_inlier_mask(data, self.inlier_thr, torch.cat(list(data["coarse_flow"])), data["batched_rot"], data["batched_trn"])
        info = {"IR Lepard": torch.stack(rates).mean()}
        conf = data["inlier_conf"].reshape(-1)
        loss = self.get_weighted_bce_loss(conf, torch.cat(masks).float())
        off = _offsets(data["vec_6d_lengths"])
        ir = []
        for b, mask in enumerate(masks):
            kept = mask[conf[off[b]:off[b + 1]] > 0.5]
            if kept.shape[0] > 0:
                ir.append(kept.sum() / kept.shape[0])
        info["IR NeCo"] = torch.stack(ir).mean() if ir else 0
        info["loss"] = loss
        return info

    @staticmethod
    def get_weighted_bce_loss(prediction, gt):
        """The reference's weighting, as written: an inlier weighs the outliers' share of the labels, an outlier the inliers', and
        the weighted terms are averaged over all rows."""
        class_loss = nn.functional.binary_cross_entropy(prediction, gt, reduction="none")
        weights = torch.ones_like(gt)
        w_negative = gt.sum() / gt.size(0)
        w_positive = 1 - w_negative
        weights[gt >= 0.5] = w_positive
        weights[gt < 0.5] = w_negative
        return torch.mean(weights * class_loss)


def synthetic_matches(n_inlier, n_outlier, seed, device="cpu"):
    """A seeded pair's putative matches -> (vec_6d [M, 6] float32, labels [M] bool), M = n_inlier + n_outlier.  The source ends
    are samples of synthetic.surface_pair's star-shaped surface (synthetic.surface_radius); an inlier's target end is its own image
    under that pair's motion (synthetic.surface_deform, then the rotation by SURFACE_ROT_Z about z and the translation SURFACE_TRN),
    an outlier's the image of another, uniformly drawn sample; the rows are shuffled.  Drawn with numpy's seeded MT19937 and computed
    in float64 on the host, so the batch is the same on every machine."""
    rs = np.random.RandomState(seed)
    M = n_inlier + n_outlier
    d = rs.standard_normal((M, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ph = rs.uniform(0.0, 2.0 * math.pi, 4)
    src = d * synthetic.surface_radius(d, ph, np)[:, None]
    c, s = math.cos(synthetic.SURFACE_ROT_Z), math.sin(synthetic.SURFACE_ROT_Z)
    Rz = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])
    image = synthetic.surface_deform(src, ph[3], np) @ Rz.T + np.array(synthetic.SURFACE_TRN)
    wrong = (np.arange(M) + rs.randint(1, M, size=M)) % M if M > 1 else np.zeros(M, np.int64)     # never the row itself
    labels = np.arange(M) < n_inlier
    tgt = np.where(labels[:, None], image, image[wrong])
    order = rs.permutation(M)
    vec_6d = np.concatenate([src, tgt], 1)[order].astype(np.float32)
    return torch.from_numpy(vec_6d).to(device), torch.from_numpy(labels[order]).to(device)


def train_step(model, optimizer, vec_6d, lens, labels):
    """One optimiser step of the filter on stacked matches with their inlier labels [sum M_b] bool -> the loss before the step."""
    optimizer.zero_grad(set_to_none=True)
    loss = NeCoLoss.get_weighted_bce_loss(model.confidence_grad(vec_6d, lens), labels.float())
    loss.backward()
    optimizer.step()
    return loss.detach()


@torch.no_grad()
def reject_landmarks(model, ldmk_s, ldmk_t, thr=0.5):
    """One pair's landmarks from any source, ldmk_s, ldmk_t [K, 3] -> (keep mask [K] bool, confidence [K]) on the model's device:
    the landmarks whose learned inlier confidence exceeds thr."""
    dev = next(model.parameters()).device
    if ldmk_s.ndim != 2 or ldmk_s.shape[1] != 3 or ldmk_s.shape != ldmk_t.shape:
        raise ValueError(f"ldmk_s and ldmk_t must both be [K, 3], got {tuple(ldmk_s.shape)} and {tuple(ldmk_t.shape)}")
    vec_6d = torch.cat([ldmk_s.to(dev).float(), ldmk_t.to(dev).float()], dim=1)
    conf = model.confidence(vec_6d, [vec_6d.shape[0]])
    return conf > thr, conf


class LandmarkModel:
    """landmark_estimator.py's Landmark_Model on lepard.Pipeline and Outlier_Rejection: two clouds in, filtered landmarks out."""

    def __init__(self, matcher, outlier_model):
        self.matcher, self.outlier_model = matcher.eval(), outlier_model.eval()

    @classmethod
    def from_checkpoints(cls, matcher_cfg, matcher_ckpt, outlier_cfg, outlier_ckpt, device="cuda"):
        """The reference's {'state_dict': ...} checkpoint files, loaded strictly."""
        matcher, outlier_model = lepard.Pipeline(matcher_cfg), Outlier_Rejection(outlier_cfg)
        matcher.load_state_dict(torch.load(matcher_ckpt, map_location="cpu")["state_dict"], strict=True)
        outlier_model.load_state_dict(torch.load(outlier_ckpt, map_location="cpu")["state_dict"], strict=True)
        return cls(matcher.to(device), outlier_model.to(device))

    @torch.no_grad()
    def inference(self, src, tgt, neighborhood_limits, reject_outliers=True, inlier_thr=0.5, coarse_flow=None, rot=None, trn=None):
        """src [N, 3], tgt [M, 3] on the device -> (ldmk_s [K, 3], ldmk_t [K, 3], confidence [K]): the matcher's coarse matches
        with their learned inlier confidence, only those above inlier_thr when reject_outliers.  With the ground truth --
        coarse_flow [S, 3] on the coarse source points, rot [3, 3], trn [3] -- the inlier rates of the matches before and after
        the filter are appended, as the reference returns them."""
        data = lepard.run_pair(self.matcher, src, tgt, neighborhood_limits)
        conf, _ = self.outlier_model(data)
        vec_6d = data["vec_6d"]
        keep = conf > inlier_thr
        out = (vec_6d[keep], conf[keep]) if reject_outliers else (vec_6d, conf)
        res = (out[0][:, :3].contiguous(), out[0][:, 3:].contiguous(), out[1])
        if coarse_flow is None:
            return res
        masks, rates = compute_inlier_mask(data, inlier_thr, coarse_flow, rot.reshape(1, 3, 3), trn.reshape(1, 3, 1))
        filtered = masks[0][keep]
        return res + (rates[0], filtered.sum() / filtered.shape[0])
