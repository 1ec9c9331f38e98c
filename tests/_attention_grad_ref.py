"""Restatements of the gradient of ops.attention and of what is trained on it, written from the maths: the yardstick of
tests/test_attention_grad.py and tests/test_attention_grad_cpu.py.  Everything is parameterised by dtype: float64 is the yardstick,
the float32 run is the "eager float32" of the project's bar (_kpconv_ref.bar).  Nothing here imports the package.

The operator, closed form in numpy (one problem; the forward is _lepard_ref.scores and _outlier_ref.compat):
    x = scale c a,  a = <q'_i,h, k'_j,h>,  p = softmax_j x,  o = p v,  lse = log sum_j exp x
    dv = p^T do,  dp = do v^T,  delta_i = <o_i, do_i> per head,  ds = p (dp - delta),  t = ds scale c
    dq' = t k',  dk' = t^T q',  dq = dq' cos + rot^T(dq' sin),  rot^T(y)[2m] = y[2m + 1],  rot^T(y)[2m + 1] = -y[2m]
c and the codes are data.  The modules (a layer, the network, the class-weighted BCE) are restated as torch functions of a dict of
parameters and differentiated by torch autograd on the CPU in the asked dtype; the same functions on the GPU in float32 are the
"eager float32 torch sequence" that the differentiable operator is compared with and timed against."""
import os
from types import SimpleNamespace

import numpy as np
import torch

from . import _kpconv_ref as R
from . import _lepard_ref as P
from . import _outlier_ref as O

F32, F64 = np.float32, np.float64
F26 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F26_attention_grad.npz")
SIGMA = O.SIGMA


# ------------------------------------------------------------------------------------------ the operator, numpy
def unrotate(y, pe):
    """The transpose of _lepard_ref.rotate: y cos + rot^T(y sin)."""
    z = y * pe[..., 1]
    zt = np.stack([z[:, 1::2], -z[:, ::2]], -1).reshape(y.shape)
    return y * pe[..., 0] + zt


def attention_grad(q, k, v, do, H, pe_q=None, pe_k=None, pos_q=None, pos_k=None, sigma_spat=None, scale=None, dtype=F64):
    """-> SimpleNamespace(o, lse [L, H], dq, dk, dv, p [L, S, H]) of one problem."""
    q, k, v, do = (np.asarray(a).astype(dtype) for a in (q, k, v, do))
    L, S, D = q.shape[0], k.shape[0], q.shape[1] // H
    qr, kr = q, k
    if pe_q is not None:
        pe_q, pe_k = np.asarray(pe_q).astype(dtype), np.asarray(pe_k).astype(dtype)
        qr, kr = P.rotate(q, pe_q), P.rotate(k, pe_k)
    c = np.ones((L, S), dtype) if sigma_spat is None else O.compat(pos_q, pos_k, sigma_spat, dtype)
    scale = dtype(D ** -0.5 if scale is None else scale)
    qh, kh, vh, gh = qr.reshape(L, H, D), kr.reshape(S, H, D), v.reshape(S, H, D), do.reshape(L, H, D)
    x = np.einsum("lhd,shd->lsh", qh, kh) * c[:, :, None] * scale
    m = x.max(1, keepdims=True)
    e = np.exp(x - m)
    s = e.sum(1, keepdims=True)
    p = e / s
    lse = (m + np.log(s))[:, 0, :]
    o = np.einsum("lsh,shd->lhd", p, vh)
    dv = np.einsum("lsh,lhd->shd", p, gh)
    dp = np.einsum("lhd,shd->lsh", gh, vh)
    delta = (o * gh).sum(-1)
    t = p * (dp - delta[:, None, :]) * scale * c[:, :, None]
    dq, dk = np.einsum("lsh,shd->lhd", t, kh).reshape(L, -1), np.einsum("lsh,lhd->shd", t, qh).reshape(S, -1)
    if pe_q is not None:
        dq, dk = unrotate(dq, pe_q), unrotate(dk, pe_k)
    out = SimpleNamespace(o=o.reshape(L, -1), lse=lse, dq=dq, dk=dk, dv=dv.reshape(S, -1), p=p)
    assert all(a.dtype == dtype for a in (out.o, out.lse, out.dq, out.dk, out.dv))
    return out


# ------------------------------------------------------------------------------------------ the operator and the modules, torch
def t_rotate(x, pe):
    x2 = torch.stack([-x[..., 1::2], x[..., ::2]], dim=-1).reshape(x.shape)
    return x * pe[..., 0] + x2 * pe[..., 1]


def t_compat(pos_q, pos_k, sigma_spat):
    ds = torch.norm(pos_q[:, None, :3] - pos_k[None, :, :3], dim=-1)
    dt = torch.norm(pos_q[:, None, 3:] - pos_k[None, :, 3:], dim=-1)
    return torch.clamp(1.0 - (ds - dt) ** 2 / sigma_spat ** 2, min=0)


def t_attention(q, k, v, H, pe_q=None, pe_k=None, pos_q=None, pos_k=None, sigma_spat=None, scale=None):
    """The reference's sequence of operations on one unpadded problem (geometry_attention.py): rotation, einsum to [L, S, H], times
    c, scale, soft-max over the keys, einsum with v.  Differentiable; any dtype and device."""
    L, S, D = q.shape[0], k.shape[0], q.shape[1] // H
    if pe_q is not None:
        q, k = t_rotate(q, pe_q), t_rotate(k, pe_k)
    a = torch.einsum("lhd,shd->lsh", q.view(L, H, D), k.view(S, H, D))
    if sigma_spat is not None:
        a = a * t_compat(pos_q, pos_k, sigma_spat).detach()[..., None]
    a = torch.softmax(a * (D ** -0.5 if scale is None else scale), dim=1)
    return torch.einsum("lsh,shd->lhd", a, v.view(S, H, D)).reshape(L, H * D)


def t_attention_stacked(q, k, v, H, pe_q, pe_k, offq, offk, pos_q=None, pos_k=None, sigma_spat=None):
    cut = lambda t, off, b: None if t is None else t[off[b]:off[b + 1]]
    return torch.cat([t_attention(cut(q, offq, b), cut(k, offk, b), cut(v, offk, b), H, cut(pe_q, offq, b), cut(pe_k, offk, b),
                                  cut(pos_q, offq, b), cut(pos_k, offk, b), sigma_spat) for b in range(len(offq) - 1)])


def t_layer(W, prefix, x, source, x_pe, source_pe, H, pe_type, x_lens, source_lens, x_pos=None, source_pos=None, sigma_spat=None, pre=None):
    """An attention layer (lepard's, or the outlier filter's with positions and sigma_spat) as a function of the parameter dict W.
    pre: a list that receives the MLP's pre-ReLU values."""
    F = torch.nn.functional
    g = lambda name: W[prefix + name]
    q, k, pe_q, pe_k = x, source, None, None
    if x_pe is not None:
        if pe_type == "sinusoidal":
            q, k = q + x_pe, k + source_pe
        elif pe_type == "rotary":
            pe_q, pe_k = x_pe, source_pe
    offq, offk = R.offsets(x_lens).tolist(), R.offsets(source_lens).tolist()
    o = t_attention_stacked(q @ g("q_proj.weight").T, k @ g("k_proj.weight").T, source @ g("v_proj.weight").T, H, pe_q, pe_k, offq, offk,
                            x_pos, source_pos, sigma_spat)
    C = x.shape[1]
    m = F.layer_norm(o @ g("merge.weight").T, (C,), g("norm1.weight"), g("norm1.bias"))
    h = torch.cat([x, m], dim=1) @ g("mlp.0.weight").T
    if pre is not None:
        pre.append(h.detach())
    m = torch.relu(h) @ g("mlp.2.weight").T
    return x + F.layer_norm(m, (C,), g("norm2.weight"), g("norm2.bias"))


def t_network(W, cfg, vec6d, lens):
    """Outlier_Rejection.confidence on stacked pairs as a function of the parameter dict W (dtype and device of vec6d)."""
    np_dtype = F64 if vec6d.dtype == torch.float64 else F32
    pe = None
    if cfg["pe_type"] != "none":
        pe = torch.from_numpy(O.position_code(vec6d.detach().cpu().numpy(), cfg["feature_dim"], cfg["pe_type"], cfg["voxel_size"], np_dtype)).to(vec6d.device)
    sigma = cfg["sigma_spat"] if cfg["spatial_consistency_check"] else None
    feat = vec6d @ W["in_proj.weight"].T + W["in_proj.bias"]
    for i in range(cfg["num_layers"]):
        feat = t_layer(W, f"_6D_geometry_layers.{i}.", feat, feat, pe, pe, cfg["n_head"], cfg["pe_type"], lens, lens, vec6d, vec6d, sigma)
    h = torch.relu(feat @ W["classification.0.weight"].T + W["classification.0.bias"])
    h = torch.relu(h @ W["classification.2.weight"].T + W["classification.2.bias"])
    return torch.sigmoid(h @ W["classification.4.weight"].T + W["classification.4.bias"])[:, 0]


def weighted_bce(conf, labels):
    """loss.py's get_weighted_bce_loss, directly: w_i = 1 - mean(labels) on an inlier, mean(labels) on an outlier;
    mean_i w_i (-(y_i log p_i + (1 - y_i) log(1 - p_i))) with torch's clamp of the logarithms at -100."""
    share = labels.mean()
    w = torch.where(labels >= 0.5, 1 - share, share)
    bce = -(labels * torch.log(conf).clamp(min=-100) + (1 - labels) * torch.log(1 - conf).clamp(min=-100))
    return (w * bce).mean()


def params_of(sd, dtype, device="cpu", requires_grad=True):
    return {k: torch.as_tensor(np.asarray(v)).to(device=device, dtype=dtype).clone().requires_grad_(requires_grad) for k, v in sd.items()}


def layer_grads(sd, x, source, x_pe, source_pe, w, H, pe_type, x_lens, source_lens, x_pos=None, source_pos=None, sigma_spat=None, dtype=torch.float64):
    """d(sum w out) in x, source and every parameter, torch autograd on the CPU in dtype -> (dict of numpy arrays with the keys "x",
    "source" and the parameter names, out, the MLP's pre-ReLU values)."""
    T = lambda a: None if a is None else torch.as_tensor(np.asarray(a)).to(dtype)
    W = params_of(sd, dtype)
    xt, st = T(x).requires_grad_(True), T(source).requires_grad_(True)
    pre = []
    out = t_layer(W, "", xt, st, T(x_pe), T(source_pe), H, pe_type, x_lens, source_lens, T(x_pos), T(source_pos), sigma_spat, pre)
    (out * T(w)).sum().backward()
    grads = {"x": xt.grad.numpy(), "source": st.grad.numpy()}
    grads.update({k: p.grad.numpy() for k, p in W.items()})
    return grads, out.detach().numpy(), pre[0].numpy()


def train_grads(sd, cfg, vec6d, lens, labels, dtype=torch.float64):
    """-> (loss, {parameter: gradient}) of the weighted BCE of the network's confidences, torch autograd on the CPU in dtype."""
    W = params_of(sd, dtype)
    loss = weighted_bce(t_network(W, cfg, torch.as_tensor(np.asarray(vec6d)).to(dtype), list(lens)), torch.as_tensor(np.asarray(labels)).to(dtype))
    loss.backward()
    return float(loss), {k: p.grad.numpy() for k, p in W.items()}


def train_init(net):
    """The seeded initialisation the training tests start from: torch's default with in_proj's weight times 4.  The issue asks for
    a seed at which the eager double path's 20-step ratio is below 0.7, so that 1.5 x the ratio stays below 1.  At the default
    initialisation none was found: over synthetic_matches(64, 32, seed) for seed 1 .. 80 times torch.manual_seed(0 .. 24) -- 2 000
    runs of the eager double path at this configuration (2 layers, C = 48, H = 4) -- the smallest ratio is 0.756 (init 16, seed 47)
    and the next are 0.764, 0.770, 0.775 and 0.778; 500 more runs (inits 0 .. 119 at the seeds 3, 15 and 17) end at 0.759, and 4 to 9 layers
    at C = 48 .. 144 at 0.80 or above.  The coordinates are of the order of 0.3 (metres), so at the default scale of the first layer
    the features start small and Adam at lr 1e-3 needs more than 20 steps to leave the plateau.  With the weight times 4 the same
    seed 3 gives 0.2852."""
    with torch.no_grad():
        net.in_proj.weight *= 4
    return net


def eager_training(model, cfg, vec6d, lens, labels, steps, lr=1e-3):
    """`steps` Adam steps on one batch with the eager sequence in the model's dtype on its device -> the losses before every step."""
    opt = torch.optim.Adam(model.parameters(), lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad(set_to_none=True)
        loss = weighted_bce(t_network(dict(model.named_parameters()), cfg, vec6d, list(lens)), labels.to(vec6d.dtype))
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


# ------------------------------------------------------------------------------------------ the cases of tests/test_attention_grad.py
#        (L, S, C, H, rotary or None for both): tile edges of either sweep (16 owned rows, walked tiles of 64, or 48 above D = 144)
GRAD_CASES = [(1, 1, 4, 1, None), (15, 63, 8, 2, None), (16, 64, 48, 4, None), (17, 65, 48, 4, None), (65, 129, 72, 4, None),
              (33, 130, 144, 8, None),             # D = 18, the shipped outlier head
              (20, 70, 528, 4, None),              # D = 132, Lepard's
              (17, 65, 264, 1, None),              # D = 264, the LDS limit: walked tiles of 48
              (5, 70, 3, 1, False), (9, 33, 68, 4, False),         # odd / unvectorised, no code
              (40, 40, 16, 16, False)]             # H = 16, D = 1, no code
GRAD_BATCH = [(1, 1), (16, 64), (37, 20), (20, 70)]                   # four unequal problems in one call, C = 48, H = 4
TRAIN_CFG = dict(C=48, H=4, num_layers=2)
TRAIN_SEED = 3                                                        # of outlier.synthetic_matches(64, 32, seed)
TRAIN_INIT = 217                                                      # torch.manual_seed of the network's initialisation
# The eager double path on the CPU, measured by tests/test_attention_grad_cpu.py: the loss after 20 Adam steps at lr 1e-3 on
# synthetic_matches(64, 32, TRAIN_SEED) over the first loss.  The bound asked of the float32 paths is that ratio times 1.5.
TRAIN_RATIO_DOUBLE = 0.2852
TRAIN_BOUND = 1.5 * TRAIN_RATIO_DOUBLE
_made = {}


def positions(L, S, seed):
    """Distinct correspondences for the query and the key rows, on the scale of sigma_spat = 0.1: c is exactly 0 on a sizeable share
    of the pairs and strictly inside (0, 1) on the rest (no query is any key, so no pair has c = 1)."""
    pos = O.matches(L + S, seed, outlier_share=0.3)
    return pos[:L].copy(), pos[L:].copy()


def grad_inputs(L, S, C, H, rotary, seed=None, spread=1.0):
    key = (L, S, C, H, rotary, seed, spread)
    if key not in _made:
        c = P.attention_inputs(L, S, C, H, rotary, seed, spread)
        sd = 104729 * L + 7919 * S + 31 * C + H if seed is None else seed
        pos_q, pos_k = positions(L, S, sd)
        do = np.random.default_rng(sd + 1).standard_normal((L, C)).astype(F32)
        _made[key] = SimpleNamespace(q=c.q, k=c.k, v=c.v, pe_q=c.pe_q, pe_k=c.pe_k, H=H, pos_q=pos_q, pos_k=pos_k, do=do, refs={})
    return _made[key]


def grad_refs(c, sigma_spat=None):
    """(float64, float32) closed-form gradients of a case, computed once."""
    if sigma_spat not in c.refs:
        c.refs[sigma_spat] = tuple(attention_grad(c.q, c.k, c.v, c.do, c.H, c.pe_q, c.pe_k, c.pos_q, c.pos_k, sigma_spat, None, dt) for dt in (F64, F32))
    return c.refs[sigma_spat]


def zero_share(c):
    """(share of the pairs with c = 0, whether every other pair lies strictly inside (0, 1))."""
    m = O.compat(c.pos_q, c.pos_k)
    return float((m == 0).mean()), bool(((m[m != 0] > 0) & (m[m != 0] < 1)).all())


def lonely_row_case():
    """(17, 65, 48, 4) with query 3 = key 3 a correspondence whose target end lies 5 m off: c[3, j] = 0 for every key but itself."""
    key = "lonely"
    if key not in _made:
        b = grad_inputs(17, 65, 48, 4, True, seed=4242)
        pos_q, pos_k = b.pos_q.copy(), b.pos_k.copy()
        pos_q[3, 3:] += np.asarray([5.0, 0.0, 0.0], F32)
        pos_k[3] = pos_q[3]
        _made[key] = SimpleNamespace(q=b.q, k=b.k, v=b.v, pe_q=b.pe_q, pe_k=b.pe_k, H=b.H, pos_q=pos_q, pos_k=pos_k, do=b.do, refs={})
    return _made[key]


def load_f26():
    return np.load(F26)
