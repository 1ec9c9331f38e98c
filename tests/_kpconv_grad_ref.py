"""The KPConv backward (csrc/ndp_kpconv_bwd.inc, ops.kpconv_bwd) restated in numpy from its formulas, in the notation of
tests/_kpfcn_ref.py, and the same forward restated in torch so that autograd can be asked: the yardsticks of
tests/test_kpconv_grad.py and tests/test_kpconv_grad_cpu.py.  Parameterised by dtype: float64 is the yardstick, the float32 run is
the "eager float32" of the project's bar (_kpconv_ref.bar).  Nothing here imports the package.

    g[n,o]     = dy[n,o] / count[n]          (normalize; else dy)         dW[k,c,o] = sum_n wf[n,k,c] g[n,o]
    dwf[n,k,c] = sum_o g[n,o] W[k,c,o]       dx[r,c] = sum over valid (n,h) with idx[n,h] == r of sum_k w(n,h,k) dwf[n,k,c]
count and the `closest` one-hot are constants; the points and the kernel points get no gradient."""
import os

import numpy as np

from . import _kpfcn_ref as K

F32, F64 = np.float32, np.float64
F27 = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "F27_kpconv_grad.npz")
GRAD_CASES = [name for name in K.CASES if name != "exact"]


def influence_weights(d2, valid, extent, influence, aggregation, dtype):
    """w [N,H,K] of _kpfcn_ref.kpconv from its d2 and valid, the same expressions."""
    if influence == "constant":
        w = np.ones_like(d2)
    elif influence == "linear":
        w = np.maximum(dtype(1) - np.sqrt(d2) / dtype(extent), dtype(0))
    else:
        w = np.exp(-d2 / dtype(2.0 * (0.3 * float(extent)) ** 2 + 1e-9))
    if aggregation == "closest":
        w = w * (np.arange(d2.shape[2])[None, None, :] == d2.argmin(2)[:, :, None])
    return (w * valid[:, :, None]).astype(dtype)


def kpconv_grad(q, s, idx, x, W, kp, extent, dy, influence="linear", aggregation="sum", normalize=True, dtype=F64):
    """-> (dx [Ns,Cin], dW [K,Cin,Cout]) in `dtype`."""
    _, d2, valid, count = K.kpconv(q, s, idx, x, W, kp, extent, influence, aggregation, normalize, dtype, want=True)
    x, W, dy = (np.asarray(a).astype(dtype) for a in (x, W, dy))
    idx = np.asarray(idx, np.int64)
    safe = np.where(valid, idx, 0)
    w = influence_weights(d2, valid, extent, influence, aggregation, dtype)
    g = dy / count[:, None].astype(dtype) if normalize else dy
    wf = np.matmul(w.transpose(0, 2, 1), x[safe] * valid[:, :, None])            # [N,K,C]
    dW = np.einsum("nkc,no->kco", wf, g, optimize=True).astype(dtype)
    dwf = np.einsum("no,kco->nkc", g, W, optimize=True).astype(dtype)
    e = np.matmul(w, dwf)                                                        # [N,H,C]
    dx = np.zeros(x.shape, dtype)
    np.add.at(dx, safe[valid], e[valid])                                         # unbuffered: ascending (n, h)
    assert dx.dtype == dtype and dW.dtype == dtype
    return dx, dW


def case_dy(c, integer=False):
    """dy [Nq,Cout] of a case: seeded standard normal (integer: whole numbers in -3 .. 3), float32."""
    g = np.random.default_rng(c.seed + 77)
    shape = (c.q.shape[0], c.W.shape[2])
    return g.integers(-3, 4, size=shape).astype(F32) if integer else g.standard_normal(shape).astype(F32)


_refs = {}


def case_refs(name, idx=None, tag="", normalize=None, integer=False):
    """(case, dy, (dx64, dW64), (dx32, dW32)) of a case of _kpfcn_ref.CASES, computed once and shared."""
    key = (name, tag)
    if key not in _refs:
        c = K.make_case(name)
        dy = case_dy(c, integer)
        table = c.idx if idx is None else idx
        norm = c.normalize if normalize is None else normalize
        run = lambda dt: kpconv_grad(c.q, c.s, table, c.x, c.W, c.kp, c.extent, dy, c.influence, c.aggregation, norm, dt)
        _refs[key] = (c, dy, run(F64), run(F32))
    return _refs[key]


def shadow_table(c):
    """Case c's table (int64) with every third entry turned into a shadow -- Ns, -1 and 2^31 - 1 in turn --, query 2 all shadows
    query 3 naming its first support twice and the support row behind that one named by nobody; and the cleaned table (every shadow Ns) the float64 yardstick is computed on."""
    ns = c.s.shape[0]
    idx = np.asarray(c.idx, np.int64).copy()
    flat = idx.reshape(-1)
    hit = np.arange(0, flat.size, 3)
    flat[hit] = np.asarray([ns, -1, 2 ** 31 - 1], np.int64)[np.arange(hit.size) % 3]
    idx[2, :] = np.asarray([ns, -1, 2 ** 31 - 1], np.int64)[np.arange(idx.shape[1]) % 3]
    first = int(np.asarray(c.idx)[3, 0])
    idx[3, 0], idx[3, 1] = first, first
    idx[idx == (first + 1) % ns] = -1                                            # a support row that only shadows "reference"
    clean = np.where((idx >= 0) & (idx < ns), idx, ns)
    return idx, clean


HOLE_ROWS = (5, 77)


def holes_table(c, rows=HOLE_ROWS):
    """Case c's table (int64) with every entry that names one of `rows` turned into the shadow Ns: those support rows lose all their
    incoming edges.  (c6_strided as _kpfcn_ref generates it references every one of its 200 supports.)"""
    idx = np.asarray(c.idx, np.int64).copy()
    idx[np.isin(idx, rows)] = c.s.shape[0]
    return idx


def unreferenced_rows(idx, ns):
    idx = np.asarray(idx, np.int64)
    seen = np.zeros(ns, bool)
    seen[idx[(idx >= 0) & (idx < ns)]] = True
    return np.nonzero(~seen)[0]


# ------------------------------------------------------------------------------------------ torch restatements (autograd's side)
def t_kpconv(q, s, idx, x, W, kp, extent, influence="linear", aggregation="sum", normalize=True):
    """The reference's op sequence (blocks.py KPConv.forward, rigid) on torch tensors of one dtype; idx an int64 tensor whose
    shadows are all Ns.  Differentiable in x and W."""
    import torch
    ns = s.shape[0]
    s_pad = torch.cat((s, torch.zeros_like(s[:1]) + 1e6), 0)
    neighbors = s_pad[idx] - q[:, None, :]
    d2 = ((neighbors[:, :, None, :] - kp[None, None, :, :]) ** 2).sum(3)              # [N,H,K]
    if influence == "constant":
        w = torch.ones_like(d2)
    elif influence == "linear":
        w = torch.clamp(1 - torch.sqrt(d2) / extent, min=0.0)
    else:
        w = torch.exp(-d2 / (2.0 * (0.3 * float(extent)) ** 2 + 1e-9))
    if aggregation == "closest":
        w = w * torch.nn.functional.one_hot(d2.argmin(2), d2.shape[2]).to(w.dtype)
    valid = (idx < ns)
    w = (w * valid[:, :, None]).transpose(1, 2)                                       # [N,K,H]; a far shadow's influence is 0 anyway
    x_pad = torch.cat((x, torch.zeros_like(x[:1])), 0)
    nx = x_pad[idx]                                                                   # [N,H,C]
    wf = torch.matmul(w, nx).permute(1, 0, 2)                                         # [K,N,C]
    y = torch.matmul(wf, W).sum(0)                                                    # [N,O]
    if normalize:
        count = torch.clamp(((nx.sum(2) > 0) & valid).sum(1), min=1)
        y = y / count[:, None].to(y.dtype)
    return y


def t_instance_norm(x, eps=1e-5):
    mean = x.mean(0, keepdim=True)
    var = ((x - mean) ** 2).mean(0, keepdim=True)
    return (x - mean) / (var + eps).sqrt()


def t_leaky(x):
    import torch
    return torch.where(x > 0, x, x * 0.1)


def _t_norm(sd, prefix, x):
    return x + sd[prefix + "bias"] if prefix + "bias" in sd else t_instance_norm(x)


def t_unary(sd, prefix, x, relu=True):
    x = _t_norm(sd, prefix + "batch_norm.", x @ sd[prefix + "mlp.weight"].t())
    return t_leaky(x) if relu else x


def _t_pad(x):
    import torch
    return torch.cat((x, torch.zeros_like(x[:1])), 0)


def _t_conv(sd, prefix, x, batch, layer, strided, cfg):
    q, s, inds = K._tables(batch, layer, strided)
    radius = cfg["first_subsampling_dl"] * cfg["conv_radius"] * 2 ** layer
    return t_kpconv(q, s, inds, x, sd[prefix + "weights"], sd[prefix + "kernel_points"], radius * cfg["KP_extent"] / cfg["conv_radius"],
                    cfg["KP_influence"], cfg["aggregation_mode"], True)


def t_simple_block(sd, prefix, x, batch, layer, strided, cfg):
    return t_leaky(_t_norm(sd, prefix + "batch_norm.", _t_conv(sd, prefix + "KPConv.", x, batch, layer, strided, cfg)))


def t_resnet_block(sd, prefix, features, batch, layer, strided, cfg):
    x = t_unary(sd, prefix + "unary1.", features) if prefix + "unary1.mlp.weight" in sd else features
    x = t_leaky(_t_norm(sd, prefix + "batch_norm_conv.", _t_conv(sd, prefix + "KPConv.", x, batch, layer, strided, cfg)))
    x = t_unary(sd, prefix + "unary2.", x, relu=False)
    shortcut = _t_pad(features)[K._tables(batch, layer, True)[2]].max(1).values if strided else features
    if prefix + "unary_shortcut.mlp.weight" in sd:
        shortcut = t_unary(sd, prefix + "unary_shortcut.", shortcut, relu=False)
    return t_leaky(x + shortcut)


def t_kpfcn_coarse(sd, batch, cfg):
    """_kpfcn_ref.kpfcn_coarse on torch tensors: batch holds tensors (tables int64 with shadows at the level's size)."""
    import torch
    arch = cfg["architecture"]
    x = batch["features"]
    layer, skips = 0, []
    start = next(i for i, b in enumerate(arch) if "upsample" in b)
    for i, block in enumerate(arch[:start]):
        if "pool" in block or "strided" in block:
            skips.append(x)
        fn = t_simple_block if "simple" in block else t_resnet_block
        x = fn(sd, f"encoder_blocks.{i}.", x, batch, layer, "strided" in block, cfg)
        if "pool" in block or "strided" in block:
            layer += 1
    x = _t_pad(x)[batch["upsamples"][layer - 1][:, 0]]
    x = t_unary(sd, "decoder_blocks.1.", torch.cat([x, skips.pop()], 1))
    return x @ sd["coarse_out.weight"][:, :, 0].t() + sd["coarse_out.bias"]


def t_batch(batch, dtype):
    """_kpfcn_ref.load_f23's batch (numpy) -> the same dict of torch tensors, floats in dtype."""
    import torch
    out = {"points": [torch.from_numpy(np.asarray(p)).to(dtype) for p in batch["points"]]}
    for key in ("neighbors", "pools", "upsamples"):
        out[key] = [torch.from_numpy(np.asarray(t, np.int64)) for t in batch[key]]
    out["features"] = torch.from_numpy(np.asarray(batch["features"])).to(dtype)
    return out


def t_params(sd, dtype, device="cpu"):
    """state dict of arrays / tensors -> {name: leaf tensor in dtype}; every floating entry but the kernel points requires grad."""
    import torch
    out = {}
    for k, v in sd.items():
        t = (torch.from_numpy(np.asarray(v)) if not isinstance(v, torch.Tensor) else v.detach().cpu()).to(dtype).to(device)
        out[k] = t.requires_grad_(not k.endswith("kernel_points"))
    return out


def load_f27():
    return np.load(F27)

