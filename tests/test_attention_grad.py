"""The backward of ops.attention (csrc/ndp_attention.inc, ndp_attention_forward_lse / ndp_attention_backward), ops.attention_fn under
autograd, the layers' forward_grad and outlier.train_step on the GPU against tests/_attention_grad_ref.py: float64 at the project's
bar -- max(4 x the float32 restatement's error, 16 float32 ulps of the largest magnitude), per tensor --, bit-for-bit where the
arithmetic promises it, and the reference's own gradients (fixture F26).  Every accuracy case prints error / bar before it asserts
(profiles/attention_grad_accuracy.txt is that output).  torch.autograd.gradcheck is not used: the kernels are fp32."""
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deformationpyramid_amd import lepard, ops, outlier
from tests import _attention_grad_ref as G
from tests import _kpconv_ref as R
from tests import _lepard_ref as P
from tests import _outlier_ref as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(what, got, ref64, ref32):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got)
    ref64 = np.asarray(ref64)
    err, err32, mag = float(np.abs(got - ref64).max()), float(np.abs(np.asarray(ref32).astype(np.float64) - ref64).max()), float(np.abs(ref64).max())
    bar = R.bar(err32, mag)
    print(f"{what}: error {err:.3e}  bar {bar:.3e}  (eager float32 {err32:.3e}, magnitude {mag:.3e})  error / bar {err / bar if bar else 0.0:.3f}")
    assert got.shape == ref64.shape and np.isfinite(got).all()
    assert err <= bar


def compat_kw(c, sigma, rows=None):
    if sigma is None:
        return {}
    return {"pos_q": dev(c.pos_q if rows is None else c.pos_q[rows]), "pos_k": dev(c.pos_k), "sigma_spat": sigma}


def backward(c, sigma=None, rows=None):
    """(dq, dk, dv, o, lse) of a case through the raw calls, as numpy; rows: only these query rows."""
    cut = lambda a: a if rows is None or a is None else a[rows]
    q, pe_q, kw = dev(cut(c.q)), dev(cut(c.pe_q)), compat_kw(c, sigma, rows)
    o, lse = ops.attention(q, dev(c.k), dev(c.v), c.H, pe_q, dev(c.pe_k), want_lse=True, **kw)
    grads = ops.attention_bwd(q, dev(c.k), dev(c.v), o, lse, dev(cut(c.do)), c.H, pe_q, dev(c.pe_k), **kw)
    return tuple(t.cpu().numpy() for t in grads + (o, lse))


def check_grads(what, got, c, sigma):
    r64, r32 = G.grad_refs(c, sigma)
    for name, g in zip(("dq", "dk", "dv"), got):
        check(f"{what} {name}", g, getattr(r64, name), getattr(r32, name))


CASES = [(s[:4], rot) for s in G.GRAD_CASES for rot in ((True, False) if s[4] is None else (s[4],))]


# ------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("variant", ["plain", "compat"])
@pytest.mark.parametrize("shape,rotary", CASES, ids=lambda s: "x".join(str(int(v)) for v in s) if isinstance(s, tuple) else ("rotary" if s else "nocode"))
def test_backward_against_float64(shape, rotary, variant):
    c = G.grad_inputs(*shape, rotary)
    sigma = G.SIGMA if variant == "compat" else None
    if sigma is not None:
        share, inside = G.zero_share(c)
        print(f"attention backward {shape}: c = 0 on {100 * share:.1f} % of the pairs")
        assert inside                                                              # every other pair strictly inside (0, 1)
        if shape[0] * shape[1] >= 256:                                             # (one pair has no share between 20 % and 80 %)
            assert 0.2 <= share <= 0.8
    got = backward(c, sigma)
    check_grads(f"attention backward {variant} {shape} {'rotary' if rotary else 'no code'}", got, c, sigma)
    r64, r32 = G.grad_refs(c, sigma)
    check(f"attention forward {variant} {shape} lse", got[4], r64.lse, r32.lse)


def test_compat_positions_over_all_cases():
    """Pooled over the cases: c is exactly 0 on a share between 20 % and 80 % of all pairs and strictly inside (0, 1) elsewhere."""
    zero = total = 0
    for shape, rotary in CASES:
        m = O.compat(*(lambda c: (c.pos_q, c.pos_k))(G.grad_inputs(*shape, rotary)))
        zero, total = zero + int((m == 0).sum()), total + m.size
        assert ((m[m != 0] > 0) & (m[m != 0] < 1)).all()
    assert 0.2 <= zero / total <= 0.8


def test_backward_row_with_no_compatible_key_but_itself():
    c = G.lonely_row_case()
    m = O.compat(c.pos_q, c.pos_k)
    assert m[3, 3] == 1 and (np.delete(m[3], 3) == 0).all() and 0.2 <= float((m == 0).mean()) <= 0.8
    check_grads("attention backward compat (17, 65, 48, 4), row 3 compatible with itself only", backward(c, G.SIGMA), c, G.SIGMA)


def test_backward_wide_logits():
    """modulated, scaled scores spread over +-200: p = exp(x - lse) stays in [0, 1] and the gradients finite"""
    for sigma in (None, G.SIGMA):
        c = G.grad_inputs(63, 65, 48, 4, True, seed=7, spread=60.0)
        a = P.scores(c.q, c.k, c.H, c.pe_q, c.pe_k) * (1.0 if sigma is None else O.compat(c.pos_q, c.pos_k)[:, :, None])
        assert a.max() > 200 and a.min() < -200
        got = backward(c, sigma)
        assert all(np.isfinite(g).all() for g in got)
        check_grads(f"attention backward {'plain' if sigma is None else 'compat'} (63, 65, 48, 4) logits over +-200", got, c, sigma)


def test_backward_non_contiguous_inputs():
    c = G.grad_inputs(17, 65, 48, 4, True)
    wide = lambda a: torch.stack([dev(a), torch.zeros_like(dev(a))], -1)[..., 0]
    q, k, v, do = wide(c.q), wide(c.k), wide(c.v), wide(c.do)
    assert not q.is_contiguous() and not k.is_contiguous() and not v.is_contiguous() and not do.is_contiguous()
    kw = compat_kw(c, G.SIGMA)
    o, lse = ops.attention(q, k, v, c.H, dev(c.pe_q), dev(c.pe_k), want_lse=True, **kw)
    got = tuple(t.cpu().numpy() for t in ops.attention_bwd(q, k, v, o, lse, do, c.H, dev(c.pe_q), dev(c.pe_k), **kw))
    check_grads("attention backward compat (17, 65, 48, 4) strided q, k, v, do", got, c, G.SIGMA)
    assert all(np.array_equal(a, b) for a, b in zip(got, backward(c, G.SIGMA)))


# ------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("variant", ["plain", "compat"])
def test_backward_batched_call(variant):
    sigma = G.SIGMA if variant == "compat" else None
    cs = [G.grad_inputs(L, S, 48, 4, True) for L, S in G.GRAD_BATCH]
    cat = lambda name: dev(np.concatenate([getattr(c, name) for c in cs]))
    offq, offk = R.offsets([c.q.shape[0] for c in cs]).tolist(), R.offsets([c.k.shape[0] for c in cs]).tolist()
    kw = {} if sigma is None else {"pos_q": cat("pos_q"), "pos_k": cat("pos_k"), "sigma_spat": sigma}
    o, lse = ops.attention(cat("q"), cat("k"), cat("v"), 4, cat("pe_q"), cat("pe_k"), offsets_q=offq, offsets_k=offk, want_lse=True, **kw)
    dq, dk, dv = (t.cpu().numpy() for t in ops.attention_bwd(cat("q"), cat("k"), cat("v"), o, lse, cat("do"), 4, cat("pe_q"), cat("pe_k"),
                                                             offsets_q=offq, offsets_k=offk, **kw))
    for b, c in enumerate(cs):
        alone = backward(c, sigma)
        mine = (dq[offq[b]:offq[b + 1]], dk[offk[b]:offk[b + 1]], dv[offk[b]:offk[b + 1]])
        check_grads(f"attention backward {variant} batched problem {b} {G.GRAD_BATCH[b]}", mine, c, sigma)
        assert all(np.array_equal(a, b_) for a, b_ in zip(mine, alone[:3]))        # the bits of the same problem alone


@pytest.mark.parametrize("shape", [(17, 65, 48, 4), (65, 129, 72, 4), (17, 65, 264, 1)], ids=["vector", "scalar", "d264"])
def test_backward_same_call_twice_and_infinite_sigma(shape):
    c = G.grad_inputs(*shape, True)
    first, again = backward(c, G.SIGMA), backward(c, G.SIGMA)
    assert all(np.array_equal(a, b) for a, b in zip(first, again))
    plain, inf = backward(c), backward(c, float("inf"))
    assert all(np.array_equal(a, b) for a, b in zip(plain, inf))


@pytest.mark.parametrize("variant", ["plain", "compat"])
def test_dq_does_not_depend_on_the_other_query_rows(variant):
    sigma = G.SIGMA if variant == "compat" else None
    c = G.grad_inputs(65, 129, 72, 4, True)
    whole = backward(c, sigma)[0]
    for i in (0, 17, 64):
        assert np.array_equal(backward(c, sigma, rows=[i])[0][0], whole[i])


@pytest.mark.parametrize("shape,rotary", [((17, 65, 48, 4), True), ((33, 130, 144, 8), True), ((9, 33, 68, 4), False), ((17, 65, 264, 1), True)],
                         ids=["vector", "d18", "scalar", "d264"])
def test_want_lse_returns_the_default_calls_bits(shape, rotary):
    c = G.grad_inputs(*shape, rotary)
    for sigma in (None, G.SIGMA):
        kw = compat_kw(c, sigma)
        args = (dev(c.q), dev(c.k), dev(c.v), c.H, dev(c.pe_q), dev(c.pe_k))
        o, lse = ops.attention(*args, want_lse=True, **kw)
        assert torch.equal(o, ops.attention(*args, **kw)) and lse.shape == (shape[0], shape[3])
        r64, r32 = G.grad_refs(c, sigma)
        check(f"attention {'plain' if sigma is None else 'compat'} {shape} lse", lse, r64.lse, r32.lse)


# ------------------------------------------------------------------------------------------ under autograd
@pytest.mark.parametrize("variant", ["plain", "compat"])
def test_attention_fn_through_the_projections(variant):
    """ops.attention_fn behind two Linear projections a side against the eager float32 torch sequence on the same GPU and against
    the same sequence in double on the CPU: gradients in the inputs and in the projections' weights."""
    sigma = G.SIGMA if variant == "compat" else None
    c = G.grad_inputs(33, 130, 144, 8, True)
    g = np.random.default_rng(5)
    Ws = {n: (g.standard_normal((144, 144)) / 12).astype(np.float32) for n in ("q", "k", "v")}

    def run(attn, dtype, device):
        T = lambda a: None if a is None else torch.from_numpy(a).to(device=device, dtype=dtype)
        leaves = {n: T(a).requires_grad_(True) for n, a in (("x", c.q), ("s", c.k), ("Wq", Ws["q"]), ("Wk", Ws["k"]), ("Wv", Ws["v"]))}
        kw = {} if sigma is None else {"pos_q": T(c.pos_q), "pos_k": T(c.pos_k), "sigma_spat": sigma}
        o = attn(leaves["x"] @ leaves["Wq"].T, leaves["s"] @ leaves["Wk"].T, leaves["s"] @ leaves["Wv"].T, 8, T(c.pe_q), T(c.pe_k), **kw)
        (o * T(c.do)).sum().backward()
        return {n: t.grad.cpu().numpy() for n, t in leaves.items()}

    ours, eager32, ref64 = run(ops.attention_fn, torch.float32, DEV), run(G.t_attention, torch.float32, DEV), run(G.t_attention, torch.float64, "cpu")
    for n in ours:
        check(f"attention_fn {variant} through the projections, d/d{n}", ours[n], ref64[n], eager32[n])


def test_attention_fn_contract():
    c = G.grad_inputs(17, 65, 48, 4, True)
    q, k, v = (dev(a).requires_grad_(True) for a in (c.q, c.k, c.v))
    pe_q, pe_k, pos_q, pos_k = (dev(a).requires_grad_(True) for a in (c.pe_q, c.pe_k, c.pos_q, c.pos_k))
    o = ops.attention_fn(q, k, v, 4, pe_q, pe_k, pos_q=pos_q, pos_k=pos_k, sigma_spat=G.SIGMA)
    assert o.requires_grad and torch.equal(o.detach(), ops.attention(q.detach(), k.detach(), v.detach(), 4, pe_q.detach(), pe_k.detach(),
                                                                     pos_q=pos_q.detach(), pos_k=pos_k.detach(), sigma_spat=G.SIGMA))
    do = torch.stack([dev(c.do).requires_grad_(True), torch.zeros_like(dev(c.do))], -1)[..., 0]      # a strided do is made contiguous
    assert not do.is_contiguous()
    o.backward(do, create_graph=True)
    check_grads("attention_fn compat (17, 65, 48, 4) strided do", (q.grad, k.grad, v.grad), c, G.SIGMA)
    assert all(t.grad is None for t in (pe_q, pe_k, pos_q, pos_k))                 # the codes and positions are data
    with pytest.raises(RuntimeError, match="once_differentiable"):
        q.grad.sum().backward()


# ------------------------------------------------------------------------------------------ the layers
LAYER_SEEDS = {"outlier": 16, "lepard": 13}      # the first seeds from 11 on at which the float64 pre-ReLU values keep 2e-3 from 0


def layer_case(kind, seed=None):
    """A layer at C = 48, H = 4 with drawn LayerNorm weights and the first MLP weight times 8, at a seed for which, in float64, every
    pre-ReLU value of the MLP is at least 1e-3 away from 0 (asserted by the caller) -> SimpleNamespace."""
    seed = LAYER_SEEDS[kind] if seed is None else seed
    g = np.random.default_rng(seed)
    torch.manual_seed(seed)
    if kind == "outlier":
        L = S = 33
        cfg = O.config(48, 4)
        mod = outlier.CorrespondenceAttentionLayer(cfg)
        pos = O.matches(L, seed)
        pe_x = pe_s = O.position_code(pos, 48, "rotary", dtype=np.float32)
        pos_x = pos_s = pos
        sigma = G.SIGMA
    else:
        L, S = 17, 65
        mod = lepard.GeometryAttentionLayer(P.transformer_config(48, 4))
        pts_x, pts_s = g.uniform(-1, 1, (L, 3)), g.uniform(-1, 1, (S, 3))
        pe_x, pe_s = (P.position_code(p, 48, "rotary", 0.04, dtype=np.float32) for p in (pts_x, pts_s))
        pos_x = pos_s = sigma = None
    for m in mod.modules():
        if isinstance(m, torch.nn.LayerNorm):
            m.weight.data = 1 + 0.2 * torch.randn(m.weight.shape)
            m.bias.data = 0.2 * torch.randn(m.bias.shape)
    mod.mlp[0].weight.data *= 8                                                        # spreads the pre-ReLU values
    x = g.standard_normal((L, 48)).astype(np.float32)
    source = x if kind == "outlier" else g.standard_normal((S, 48)).astype(np.float32)
    w = g.standard_normal((L, 48)).astype(np.float32)
    sd = {k: v.numpy() for k, v in mod.state_dict().items()}
    return SimpleNamespace(kind=kind, mod=mod, sd=sd, x=x, source=source, pe_x=pe_x, pe_s=pe_s, pos_x=pos_x, pos_s=pos_s, sigma=sigma, w=w,
                           lens=([L], [S]))


def hip_layer_grads(mod, x, source, pe_x, pe_s, lens, pos_x, pos_s, w):
    """d(sum w forward_grad(...)) in x, source and every parameter on the GPU.  On the way: under enabled grad, with inputs and
    parameters that require grad, forward itself returns a tensor without grad_fn, bit for bit forward_grad's value."""
    mod = mod.to(DEV)
    mod.zero_grad()
    xt, st = dev(x).requires_grad_(True), dev(source).requires_grad_(True)
    args = (xt, st, dev(pe_x), dev(pe_s), lens[0], lens[1]) + ((dev(pos_x), dev(pos_s)) if pos_x is not None else ())
    with torch.enable_grad():
        assert torch.is_grad_enabled() and all(p.requires_grad for p in mod.parameters())
        out, plain = mod.forward_grad(*args), mod(*args)
    assert out.grad_fn is not None and plain.grad_fn is None and not plain.requires_grad and torch.equal(out.detach(), plain)
    (out * dev(w)).sum().backward()
    grads = {"x": xt.grad, "source": st.grad}
    grads.update({k: p.grad for k, p in mod.named_parameters()})
    return grads


@pytest.mark.parametrize("kind", ["outlier", "lepard"])
def test_layer_gradients_against_float64(kind):
    c = layer_case(kind)
    run = lambda dt: G.layer_grads(c.sd, c.x, c.source, c.pe_x, c.pe_s, c.w, 4, "rotary", c.lens[0], c.lens[1], c.pos_x, c.pos_s, c.sigma, dt)
    (g64, _, pre), (g32, _, _) = run(torch.float64), run(torch.float32)
    assert np.abs(pre).min() >= 1e-3, f"a pre-ReLU value lies {np.abs(pre).min():.2e} from 0: the gradient is not smooth there"
    ours = hip_layer_grads(c.mod, c.x, c.source, c.pe_x, c.pe_s, c.lens, c.pos_x, c.pos_s, c.w)
    for name in g64:
        check(f"{kind} layer forward_grad, d/d{name}", ours[name], g64[name], g32[name])


@pytest.mark.parametrize("kind", ["outlier", "lepard"])
def test_layer_gradients_against_the_references_own(kind):
    z = G.load_f26()
    f = lambda name: z[f"{kind}.{name}"]
    cfg = O.config(48, 4) if kind == "outlier" else P.transformer_config(48, 4)
    mod = (outlier.CorrespondenceAttentionLayer if kind == "outlier" else lepard.GeometryAttentionLayer)(cfg)
    mod.load_state_dict({k[len(kind) + 4:]: torch.from_numpy(z[k]) for k in z.files if k.startswith(f"{kind}.sd.")}, strict=True)
    pos = (f("vec6d"), f("vec6d")) if kind == "outlier" else (None, None)
    x, source = f("x"), f("source")
    ours = hip_layer_grads(mod, x, source, f("x_pe"), f("source_pe"), ([x.shape[0]], [source.shape[0]]), pos[0], pos[1], f("w"))
    assert np.abs(f("pre64")).min() >= 1e-3
    for k in z.files:
        if k.startswith(f"{kind}.grad64."):
            name = k[len(kind) + 8:]
            check(f"{kind} layer forward_grad against the reference's own gradient, d/d{name}", ours[name], z[k], z[f"{kind}.grad32.{name}"])


# ------------------------------------------------------------------------------------------ the network and training
def train_case():
    cfg = O.config(G.TRAIN_CFG["C"], G.TRAIN_CFG["H"], num_layers=G.TRAIN_CFG["num_layers"])
    torch.manual_seed(G.TRAIN_INIT)
    return cfg, G.train_init(outlier.Outlier_Rejection(cfg))


def test_confidence_is_the_no_grad_value_of_confidence_grad():
    cfg, net = train_case()
    net = net.to(DEV)
    v6 = torch.cat([outlier.synthetic_matches(30, 18, s, DEV)[0] for s in (1, 2)])
    with torch.enable_grad():
        plain, rec = net.confidence(v6, [48, 48]), net.confidence_grad(v6, [48, 48])
    assert plain.grad_fn is None and rec.grad_fn is not None and torch.equal(plain, rec.detach())


def test_one_train_step_against_float64():
    cfg, net = train_case()
    batches = [outlier.synthetic_matches(30, 18, s) for s in (1, 2)]                   # M = 96 in two stacked pairs
    v6, labels, lens = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches]), [48, 48]
    sd = {k: v.numpy().copy() for k, v in net.state_dict().items()}
    (l64, g64), (l32, g32) = (G.train_grads(sd, cfg, v6.numpy(), lens, labels.numpy(), dt) for dt in (torch.float64, torch.float32))
    net = net.to(DEV)
    opt = torch.optim.SGD(net.parameters(), lr=0.0)                                    # the step keeps the gradients to look at
    loss = outlier.train_step(net, opt, v6.to(DEV), lens, labels.to(DEV))
    check("train_step loss", loss.reshape(1), np.asarray([l64]), np.asarray([l32]))
    for name, p in net.named_parameters():
        check(f"train_step d/d{name}", p.grad, g64[name], g32[name])


def test_twenty_train_steps_lower_the_loss():
    """The loss falls below G.TRAIN_BOUND of its first value: 1.5 x the eager double path's measured 20-step ratio 0.2852 (0.4278).
    Measured on an MI355X: eager float32 0.2854, the HIP path 0.3600.  The gap is not a gradient error: along one shared trajectory
    the two paths' gradients agree to 1e-6 of each tensor's maximum at every one of the 21 steps, and run freely the two
    trajectories' parameters agree to 1.4e-6 through step 7.  From step 8 on Adam's m / sqrt(v) turns that noise into steps of the
    size of lr on the elements whose gradients are near zero, and the loss falls by 10-15 % a step at the end, so a fraction of a
    step's lag is a tenth of the ratio: eager float32 with Gaussian noise of 1e-7 of each gradient's maximum ends between 0.27 and
    0.34.  The margin under the bound is therefore thinner for the HIP path (0.36 of 0.43) than the figures of one run suggest."""
    v6, labels = outlier.synthetic_matches(64, 32, G.TRAIN_SEED, DEV)
    cfg, net = train_case()
    net = net.to(DEV)
    opt = torch.optim.Adam(net.parameters(), lr=1e-3)
    ours = [float(outlier.train_step(net, opt, v6, [96], labels)) for _ in range(20)]
    ours.append(float(outlier.NeCoLoss.get_weighted_bce_loss(net.confidence(v6, [96]), labels.float())))
    cfg, net = train_case()
    eager = G.eager_training(net.to(DEV), cfg, v6, [96], labels, 21)
    print(f"20 Adam steps: HIP path loss {ours[0]:.5f} -> {ours[20]:.5f} (ratio {ours[20] / ours[0]:.4f}), eager float32 {eager[0]:.5f} -> {eager[20]:.5f} "
          f"(ratio {eager[20] / eager[0]:.4f}); bound {G.TRAIN_BOUND:.4f} = 1.5 x the eager double path's {G.TRAIN_RATIO_DOUBLE}")
    assert eager[20] <= G.TRAIN_BOUND * eager[0]
    assert ours[20] <= G.TRAIN_BOUND * ours[0]
