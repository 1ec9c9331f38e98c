"""The KPFCN backbone of Lepard (correspondence/lepard/blocks.py, backbone.py) up to its coarse descriptors, on ops.kpconv: the step
between kpconv.build_pyramid (the collate's tables) and matching.* (per-point descriptors).  The modules carry the reference's
parameter and buffer names, so the `backbone.*` part of a Lepard checkpoint loads with load_state_dict(strict=True).

What runs where: every KPConv is one ops.kpconv call (csrc/ndp_kpconv_conv.inc); the unary layers, the instance norm, LeakyReLU(0.1)
and the two shadow-row gathers (max_pool, closest_pool) are torch ops on the device.  `forward` is the inference path: its KPConv
outputs carry no grad_fn.  `forward_grad` (KPConv, SimpleBlock, ResnetBottleneckBlock, KPFCN) is the same computation on
ops.kpconv_fn, whose backward is csrc/ndp_kpconv_bwd.inc: gradients reach every KPConv's weights and the input features, the torch
ops around it are autograd's.  train_step is one optimiser step on a descriptor loss over synthetic surface pairs.  The points and
the kernel points get no gradient.

Not served: deformable / modulated convolutions, the `equivariant` / `invariant` block names, any `phase` but "coarse" (the
reference's fine decoder is commented out upstream; `fine_out` is kept as unused parameters so that checkpoints load).  Lepard's
repositioning transformer between this backbone and the matching is deformationpyramid_amd/lepard.py (lepard.Pipeline holds this
backbone); descriptors from here go to matching.* as they are only when that is what the caller wants.  Parity with a trained
Lepard checkpoint is unverified: none is available."""
import math
from types import SimpleNamespace

import numpy as np
import torch
import torch.nn as nn
from torch.nn.init import kaiming_uniform_
from torch.nn.parameter import Parameter

from . import kpconv, ops

KP_RADIUS_RATIO = 0.66                       # the reference's: kernel points are optimised inside 0.66 x the convolution radius


def default_kernel_points(K, radius):
    """[K, 3] float32 kernel points for a model built WITHOUT a checkpoint: the centre, then a Fibonacci-sphere lattice of K - 1
    points at 0.66 * radius.  Closed form and deterministic.  NOT the reference's disposition -- that one comes out of an
    optimisation it caches on disk and is a saved parameter, so a checkpoint brings its own."""
    K = int(K)
    if K < 1:
        raise ValueError(f"K must be >= 1, got {K}")
    pts = torch.zeros(K, 3, dtype=torch.float64)
    m = K - 1
    if m > 0:
        i = torch.arange(m, dtype=torch.float64)
        z = 1.0 - (2.0 * i + 1.0) / m
        rho = torch.sqrt(torch.clamp(1.0 - z * z, min=0.0))
        phi = i * (math.pi * (3.0 - math.sqrt(5.0)))
        pts[1:] = torch.stack([rho * torch.cos(phi), rho * torch.sin(phi), z], 1) * (KP_RADIUS_RATIO * float(radius))
    return pts.float()


def _cfg(config):
    return SimpleNamespace(**config) if isinstance(config, dict) else config


def _refuse(block_name, config=None):
    for word in ("deformable", "equivariant", "invariant"):
        if word in block_name:
            raise NotImplementedError(f"block {block_name!r}: {word} blocks are not served (rigid KPConv only)")
    if config is not None and (getattr(config, "deformable", False) or getattr(config, "modulated", False)):
        raise NotImplementedError("deformable / modulated convolutions are not served (rigid KPConv only)")


def max_pool(x, inds):
    """[n2, d]: per row of inds [n2, m] the channel-wise maximum of x's rows; the shadow index len(x) is a row of zeros."""
    x = torch.cat((x, torch.zeros_like(x[:1, :])), 0)
    return x[inds].max(1).values


def closest_pool(x, inds):
    """[n2, d]: x's row named by the first column of inds (the nearest neighbour); the shadow index len(x) is a row of zeros."""
    x = torch.cat((x, torch.zeros_like(x[:1, :])), 0)
    return x[inds[:, 0]]


class KPConv(nn.Module):
    def __init__(self, kernel_size, p_dim, in_channels, out_channels, KP_extent, radius, fixed_kernel_points="center",
                 KP_influence="linear", aggregation_mode="sum", deformable=False, modulated=False):
        super().__init__()
        if deformable or modulated:
            raise NotImplementedError("deformable / modulated convolutions are not served (rigid KPConv only)")
        if p_dim != 3:
            raise NotImplementedError(f"points of dimension {p_dim} are not served")
        if KP_influence not in ops.KPCONV_INFLUENCE or aggregation_mode not in ops.KPCONV_AGGREGATION:
            raise ValueError(f"unknown KP_influence {KP_influence!r} or aggregation_mode {aggregation_mode!r}")
        self.K, self.p_dim, self.in_channels, self.out_channels = kernel_size, p_dim, in_channels, out_channels
        self.radius, self.KP_extent = radius, KP_extent
        self.fixed_kernel_points, self.KP_influence, self.aggregation_mode = fixed_kernel_points, KP_influence, aggregation_mode
        self.deformable, self.modulated = False, False
        self.weights = Parameter(torch.zeros((self.K, in_channels, out_channels), dtype=torch.float32), requires_grad=True)
        kaiming_uniform_(self.weights, a=math.sqrt(5))
        self.kernel_points = Parameter(default_kernel_points(self.K, radius), requires_grad=False)

    def forward(self, q_pts, s_pts, neighb_inds, x):
        return ops.kpconv(q_pts, s_pts, neighb_inds, x, self.weights, self.kernel_points, self.KP_extent,
                          influence=self.KP_influence, aggregation=self.aggregation_mode, normalize=True)

    def forward_grad(self, q_pts, s_pts, neighb_inds, x):
        """forward's bits, differentiable in x and self.weights (ops.kpconv_fn)."""
        return ops.kpconv_fn(q_pts, s_pts, neighb_inds, x, self.weights, self.kernel_points, self.KP_extent,
                             influence=self.KP_influence, aggregation=self.aggregation_mode, normalize=True)

    def __repr__(self):
        return f"KPConv(radius: {self.radius:.2f}, extent: {self.KP_extent:.2f}, in_feat: {self.in_channels:d}, out_feat: {self.out_channels:d})"


class BatchNormBlock(nn.Module):
    """use_bn: the reference's InstanceNorm1d over all stacked points per channel (biased variance, eps 1e-5, no parameters);
    otherwise a bias."""

    def __init__(self, in_dim, use_bn, bn_momentum):
        super().__init__()
        self.bn_momentum, self.use_bn, self.in_dim = bn_momentum, use_bn, in_dim
        if self.use_bn:
            self.batch_norm = nn.InstanceNorm1d(in_dim, momentum=bn_momentum)
        else:
            self.bias = Parameter(torch.zeros(in_dim, dtype=torch.float32), requires_grad=True)

    def forward(self, x):
        if self.use_bn:
            return self.batch_norm(x.t().unsqueeze(0)).squeeze(0).t()     # [N, C] -> [1, C, N] and back; no bare squeeze(): N = 1 and C = 1 keep their axes
        return x + self.bias


class UnaryBlock(nn.Module):
    def __init__(self, in_dim, out_dim, use_bn, bn_momentum, no_relu=False):
        super().__init__()
        self.bn_momentum, self.use_bn, self.no_relu, self.in_dim, self.out_dim = bn_momentum, use_bn, no_relu, in_dim, out_dim
        self.mlp = nn.Linear(in_dim, out_dim, bias=False)
        self.batch_norm = BatchNormBlock(out_dim, self.use_bn, self.bn_momentum)
        if not no_relu:
            self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, x, batch=None):
        x = self.batch_norm(self.mlp(x))
        return x if self.no_relu else self.leaky_relu(x)


def _conv_tables(block_name, layer_ind, batch):
    if "strided" in block_name:
        return batch["points"][layer_ind + 1], batch["points"][layer_ind], batch["pools"][layer_ind]
    return batch["points"][layer_ind], batch["points"][layer_ind], batch["neighbors"][layer_ind]


def _make_conv(block_name, in_dim, out_dim, radius, config):
    return KPConv(config.num_kernel_points, config.in_points_dim, in_dim, out_dim, radius * config.KP_extent / config.conv_radius, radius,
                  fixed_kernel_points=config.fixed_kernel_points, KP_influence=config.KP_influence,
                  aggregation_mode=config.aggregation_mode, deformable="deform" in block_name, modulated=config.modulated)


class SimpleBlock(nn.Module):
    def __init__(self, block_name, in_dim, out_dim, radius, layer_ind, config):
        super().__init__()
        config = _cfg(config)
        _refuse(block_name, config)
        self.bn_momentum, self.use_bn = config.batch_norm_momentum, config.use_batch_norm
        self.layer_ind, self.block_name, self.in_dim, self.out_dim = layer_ind, block_name, in_dim, out_dim
        self.KPConv = _make_conv(block_name, in_dim, out_dim // 2, radius, config)
        self.batch_norm = BatchNormBlock(out_dim // 2, self.use_bn, self.bn_momentum)
        self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, x, batch):
        return self._run(x, batch, self.KPConv)

    def forward_grad(self, x, batch):
        return self._run(x, batch, self.KPConv.forward_grad)

    def _run(self, x, batch, conv):
        q_pts, s_pts, inds = _conv_tables(self.block_name, self.layer_ind, batch)
        return self.leaky_relu(self.batch_norm(conv(q_pts, s_pts, inds, x)))


class ResnetBottleneckBlock(nn.Module):
    def __init__(self, block_name, in_dim, out_dim, radius, layer_ind, config):
        super().__init__()
        config = _cfg(config)
        _refuse(block_name, config)
        self.bn_momentum, self.use_bn = config.batch_norm_momentum, config.use_batch_norm
        self.block_name, self.layer_ind, self.in_dim, self.out_dim = block_name, layer_ind, in_dim, out_dim
        self.unary1 = UnaryBlock(in_dim, out_dim // 4, self.use_bn, self.bn_momentum) if in_dim != out_dim // 4 else nn.Identity()
        self.KPConv = _make_conv(block_name, out_dim // 4, out_dim // 4, radius, config)
        self.batch_norm_conv = BatchNormBlock(out_dim // 4, self.use_bn, self.bn_momentum)
        self.unary2 = UnaryBlock(out_dim // 4, out_dim, self.use_bn, self.bn_momentum, no_relu=True)
        self.unary_shortcut = (UnaryBlock(in_dim, out_dim, self.use_bn, self.bn_momentum, no_relu=True) if in_dim != out_dim
                               else nn.Identity())
        self.leaky_relu = nn.LeakyReLU(0.1)

    def forward(self, features, batch):
        return self._run(features, batch, self.KPConv)

    def forward_grad(self, features, batch):
        return self._run(features, batch, self.KPConv.forward_grad)

    def _run(self, features, batch, conv):
        q_pts, s_pts, inds = _conv_tables(self.block_name, self.layer_ind, batch)
        x = self.unary1(features)
        x = self.leaky_relu(self.batch_norm_conv(conv(q_pts, s_pts, inds, x)))
        x = self.unary2(x)
        shortcut = max_pool(features, inds) if "strided" in self.block_name else features
        return self.leaky_relu(x + self.unary_shortcut(shortcut))


class NearestUpsampleBlock(nn.Module):
    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind

    def forward(self, x, batch):
        return closest_pool(x, batch["upsamples"][self.layer_ind - 1])


class MaxPoolBlock(nn.Module):
    def __init__(self, layer_ind):
        super().__init__()
        self.layer_ind = layer_ind

    def forward(self, x, batch):
        return max_pool(x, batch["pools"][self.layer_ind + 1])


def block_decider(block_name, radius, in_dim, out_dim, layer_ind, config):
    config = _cfg(config)
    _refuse(block_name)
    if block_name == "unary":
        return UnaryBlock(in_dim, out_dim, config.use_batch_norm, config.batch_norm_momentum)
    if block_name in ("simple", "simple_strided"):
        return SimpleBlock(block_name, in_dim, out_dim, radius, layer_ind, config)
    if block_name in ("resnetb", "resnetb_strided"):
        return ResnetBottleneckBlock(block_name, in_dim, out_dim, radius, layer_ind, config)
    if block_name in ("max_pool", "max_pool_wide"):
        return MaxPoolBlock(layer_ind)
    if block_name == "nearest_upsample":
        return NearestUpsampleBlock(layer_ind)
    raise ValueError("Unknown block name in the architecture definition : " + block_name)


class KPFCN(nn.Module):
    """backbone.py's KPFCN: the same modules under the same names in the same order.  forward(batch, phase="coarse") takes the
    collate's dict (features [N, in_feats_dim], points / neighbors / pools / upsamples lists as kpconv.build_pyramid returns them)
    and returns the coarse descriptors [n_coarse, coarse_feature_dim]: the encoder, the first upsampling, its unary, coarse_out."""

    def __init__(self, config):
        super().__init__()
        config = _cfg(config)
        _refuse("", config)
        layer, r = 0, config.first_subsampling_dl * config.conv_radius
        in_dim, out_dim = config.in_feats_dim, config.first_feats_dim
        self.encoder_blocks = nn.ModuleList()
        self.encoder_skip_dims, self.encoder_skips = [], []
        for block_i, block in enumerate(config.architecture):
            if any(tmp in block for tmp in ("pool", "strided", "upsample", "global")):
                self.encoder_skips.append(block_i)
                self.encoder_skip_dims.append(in_dim)
            if "upsample" in block:
                break
            self.encoder_blocks.append(block_decider(block, r, in_dim, out_dim, layer, config))
            in_dim = out_dim // 2 if "simple" in block else out_dim
            if "pool" in block or "strided" in block:
                layer += 1
                r *= 2
                out_dim *= 2
        self.coarse_out = nn.Conv1d(in_dim // 2, config.coarse_feature_dim, kernel_size=1, bias=True)
        self.coarse_in = nn.Conv1d(config.coarse_feature_dim, in_dim // 2, kernel_size=1, bias=True)
        self.decoder_blocks = nn.ModuleList()
        self.decoder_concats = []
        start_i = next((i for i, block in enumerate(config.architecture) if "upsample" in block), 0)
        for block_i, block in enumerate(config.architecture[start_i:]):
            if block_i > 0 and "upsample" in config.architecture[start_i + block_i - 1]:
                in_dim += self.encoder_skip_dims[layer]
                self.decoder_concats.append(block_i)
            self.decoder_blocks.append(block_decider(block, r, in_dim, out_dim, layer, config))
            in_dim = out_dim
            if "upsample" in block:
                layer -= 1
                r *= 0.5
                out_dim = out_dim // 2
        self.fine_out = nn.Conv1d(out_dim, config.fine_feature_dim, kernel_size=1, bias=True)      # unused: the reference's fine phase is commented out

    def forward(self, batch, phase="coarse"):
        return self._run(batch, phase, False)

    def forward_grad(self, batch, phase="coarse"):
        """forward's computation with every KPConv on ops.kpconv_fn: differentiable in the parameters and in batch["features"]
        (which is used as it is, not detached)."""
        return self._run(batch, phase, True)

    def _run(self, batch, phase, grad):
        if phase != "coarse":
            raise NotImplementedError(f"phase {phase!r}: only the coarse descriptors are served")
        x = batch["features"] if grad else batch["features"].clone().detach()
        call = (lambda op: getattr(op, "forward_grad", op)) if grad else (lambda op: op)
        skip_x = []
        for block_i, block_op in enumerate(self.encoder_blocks):
            if block_i in self.encoder_skips:
                skip_x.append(x)
            x = call(block_op)(x, batch)
        for block_i, block_op in enumerate(self.decoder_blocks):
            if block_i in self.decoder_concats:
                x = torch.cat([x, skip_x.pop()], dim=1)
            x = call(block_op)(x, batch)
            if block_i == 1:
                return self.coarse_out(x.t().unsqueeze(0)).squeeze(0).t().contiguous()       # [N, C] -> [1, C, N] -> [N, C2]
        raise ValueError("the architecture has no unary block behind its first upsampling: no coarse descriptors")


@torch.no_grad()
def coarse_features(model, points, lengths, config, neighborhood_limits):
    """Stacked clouds -> (coarse points [n_coarse, 3], their lengths [B] int32 on the host, descriptors [n_coarse, coarse_feature_dim]):
    kpconv.build_pyramid with the config's numbers, ones [N, 1] as input features, model's coarse forward.  Cut per cloud by the
    lengths, the descriptors are what matching.* and matching.landmarks_from_descriptors take.  Lepard's repositioning transformer
    between the backbone and the matching is NOT applied here: lepard.Pipeline / lepard.predict_landmarks apply it."""
    config = _cfg(config)
    batch = kpconv.build_pyramid(points, lengths, config.first_subsampling_dl, config.conv_radius, config.deform_radius,
                                 config.architecture, neighborhood_limits)
    batch["features"] = torch.ones(points.shape[0], 1, device=points.device)
    feats = model(batch, phase="coarse")
    level = len(batch["points"]) - 2                               # one upsampling above the encoder's last level
    return batch["points"][level], batch["stack_lengths"][level], feats


# ------------------------------------------------------------------------------------------ training the coarse descriptors
TRAIN_LIMITS = (24, 28, 32, 36, 40)          # neighbourhood limits of synthetic_batch's pyramid, one per level
TRAIN_TEMPERATURE = 0.1


def trainable_parameters(model):
    """The parameters the coarse phase reaches, for an optimiser.  What it does not reach -- coarse_in, fine_out and the decoder
    behind the first unary -- is frozen (requires_grad_(False)): it would get no gradient and an optimiser would carry it unmoved."""
    for name, p in model.named_parameters():
        unused = name.startswith(("coarse_in.", "fine_out.")) or (name.startswith("decoder_blocks.") and int(name.split(".")[1]) > 1)
        if unused:
            p.requires_grad_(False)
    return [p for p in model.parameters() if p.requires_grad]


def synthetic_batch(seed, config, n_points=2048, device="cuda", match_radius=None):
    """A seeded training pair as KPFCN's batch dict.  Both clouds are samples of synthetic.surface_pair's star-shaped surface
    (synthetic.surface_radius), drawn independently with numpy's MT19937 in float64 (the same numbers on every machine); the target
    is the surface rotated by synthetic.SURFACE_ROT_Z about z and translated by synthetic.SURFACE_TRN -- a known rigid motion.  On top
    of kpconv.build_pyramid's lists and features = ones [N, 1]: "coarse_lengths" (source, target) at the level of the descriptors,
    and "matches" [2, M] int64 -- the ground-truth coarse matches: the mutual nearest neighbours of the moved source coarse points
    among the target's within match_radius (default: the coarse voxel edge), as indices into either side."""
    from . import synthetic
    config = _cfg(config)
    rs = np.random.RandomState(seed)
    d = rs.standard_normal((2 * n_points, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ph = rs.uniform(0.0, 2.0 * math.pi, 4)
    x = d * synthetic.surface_radius(d, ph, np)[:, None]
    c, s = math.cos(synthetic.SURFACE_ROT_Z), math.sin(synthetic.SURFACE_ROT_Z)
    Rz, t = np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]]), np.array(synthetic.SURFACE_TRN)
    src, tgt = x[:n_points], x[n_points:] @ Rz.T + t
    points = torch.from_numpy(np.concatenate([src, tgt]).astype(np.float32)).to(device)
    n_layers = len(kpconv._layers(config.architecture))
    batch = kpconv.build_pyramid(points, [n_points, n_points], config.first_subsampling_dl, config.conv_radius, config.deform_radius,
                                 config.architecture, TRAIN_LIMITS[:n_layers])
    batch["features"] = torch.ones(points.shape[0], 1, device=points.device)
    level = len(batch["points"]) - 2
    n_s, n_t = (int(v) for v in batch["stack_lengths"][level])
    coarse = batch["points"][level]
    moved = coarse[:n_s] @ torch.from_numpy(Rz.T.astype(np.float32)).to(coarse.device) + torch.from_numpy(t.astype(np.float32)).to(coarse.device)
    radius = match_radius if match_radius is not None else config.first_subsampling_dl * 2 ** level
    batch["coarse_lengths"] = (n_s, n_t)
    batch["matches"] = kpconv.mutual_nn_correspondence(moved.contiguous(), coarse[n_s:].contiguous(), radius)
    return batch


def descriptor_scores(feats, batch, temperature=TRAIN_TEMPERATURE):
    """a [n_s, n_t] = <f_s, f_t> / (C temperature) of a batch's coarse descriptors: ops.feat_conf's scores, in eager torch."""
    n_s, n_t = batch["coarse_lengths"]
    return feats[:n_s] @ feats[n_s:n_s + n_t].t() / (feats.shape[1] * temperature)


def descriptor_loss(feats, batch, temperature=TRAIN_TEMPERATURE):
    """The mean negative log dual-softmax likelihood of the batch's ground-truth matches: -mean_m (log softmax_j a[i_m, :][j_m] + log
    softmax_i a[:, j_m][i_m]).  Eager torch: ops.feat_conf has no backward."""
    a = descriptor_scores(feats, batch, temperature)
    i, j = batch["matches"]
    return -(torch.log_softmax(a, 1)[i, j] + torch.log_softmax(a, 0)[i, j]).mean()


@torch.no_grad()
def match_recall(feats, batch):
    """The share of the ground-truth matches that the descriptors' mutual nearest neighbours (by score) recover."""
    a = descriptor_scores(feats, batch)
    i, j = batch["matches"]
    return float(((a.argmax(1)[i] == j) & (a.argmax(0)[j] == i)).float().mean())


def train_step(model, batches, optimizer):
    """One optimiser step on the mean descriptor_loss of `batches` (synthetic_batch's dicts) through forward_grad -> the loss before
    the step.  Every KPConv gradient is csrc/ndp_kpconv_bwd.inc's; the loss and everything between the convolutions is eager torch."""
    optimizer.zero_grad(set_to_none=True)
    loss = torch.stack([descriptor_loss(model.forward_grad(b, phase="coarse"), b) for b in batches]).mean()
    loss.backward()
    optimizer.step()
    return loss.detach()
