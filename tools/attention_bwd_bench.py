"""Forward + backward of the differentiable attention (ops.attention_fn: ndp_attention_forward_lse, then ndp_attention_backward) next
to the reference's sequence of operations in eager float32 torch under autograd on the same GPU, and one training step of the
nine-layer Outlier_Rejection both ways:
    python tools/attention_bwd_bench.py [runs [output file]]
Device events around one call, every shape warmed up first, the median of `runs` calls (tools/outlier_bench.py's counts).  A call is
the forward from leaf q, k, v, then backward of sum(o * do), with its allocations.  The eager side is the rotation of q and k, einsum
to [B, L, S, H] scores, times the compatibility c (given: the reference takes it once per forward), scale, soft-max, einsum with v;
the shapes have equal problems, so the eager batch carries no padding.  For the plain variant F.scaled_dot_product_attention in
float32 on the rotated q and k is timed as well.  Peak memory is torch.cuda.max_memory_allocated over one call above what was
allocated before it.  The training step is outlier.train_step at outlier.DEFAULT_CONFIG against the same modules with their
attention replaced by the eager sequence (c taken once per step).
Output: profiles/attention_bwd_bench.txt unless another file is named."""
import os, statistics, sys
import numpy as np
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import ops, outlier
from tests import _outlier_ref as O

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
SIGMA = 0.1
OUTLIER_SHAPES = ((256, 1), (1000, 1), (2000, 1), (700, 8))           # (M, B) at C = 144, H = 8: tools/outlier_bench.py's
LEPARD_SHAPES = ((500, 1), (2000, 1))                                 # (L = S, B) at C = 528, H = 4


def timed(fn, runs):
    """(median device milliseconds of fn() over `runs` calls, peak bytes of one call above the standing allocation)."""
    fn(); fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    ms = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms), peak


def rot(x, pe):
    x2 = torch.stack([-x[..., 1::2], x[..., ::2]], dim=-1).reshape(x.shape)
    return x * pe[..., 0] + x2 * pe[..., 1]


def eager_compat(pos6d, sigma):
    src, tgt = pos6d[..., :3], pos6d[..., 3:]
    src_dist = torch.norm(src[:, :, None, :] - src[:, None, :, :], dim=-1)
    tgt_dist = torch.norm(tgt[:, :, None, :] - tgt[:, None, :, :], dim=-1)
    return torch.clamp(1.0 - (src_dist - tgt_dist) ** 2 / sigma ** 2, min=0)


def eager_attention(q, k, v, H, pe_q, pe_k, comp):
    B, D = q.shape[0], q.shape[2] // H
    q, k = rot(q, pe_q), rot(k, pe_k)
    a = torch.einsum("nlhd,nshd->nlsh", q.view(B, -1, H, D), k.view(B, -1, H, D))
    if comp is not None:
        a = a * comp[..., None]
    a = torch.softmax(a / D ** 0.5, dim=2)
    return torch.einsum("nlsh,nshd->nlhd", a, v.view(B, -1, H, D)).reshape(B, -1, H * D)


def sdpa(q, k, v, H, pe_q, pe_k):
    B, D = q.shape[0], q.shape[2] // H
    heads = lambda t: t.view(B, -1, H, D).transpose(1, 2)
    return F.scaled_dot_product_attention(heads(rot(q, pe_q)), heads(rot(k, pe_k)), heads(v)).transpose(1, 2).reshape(B, -1, H * D)


def mark(ours, other):
    return f"{other / ours:5.2f}x" if ours <= other else f"**{other / ours:5.2f}x (slower)**"


def fwd_bwd(fn, leaves, do):
    def call():
        for t in leaves:
            t.grad = None
        (fn() * do).sum().backward()
    return call


lines = []
for C, H, shapes, compat in ((144, 8, OUTLIER_SHAPES, True), (528, 4, LEPARD_SHAPES, False)):
    for M, B in shapes:
        g = torch.Generator().manual_seed(M + B)
        q, k, v, do = (torch.randn(B * M, C, generator=g).to(dev) for _ in range(4))
        q, k, v = (t.requires_grad_(True) for t in (q, k, v))
        pos = torch.from_numpy(np.concatenate([O.matches(M, 1000 * M + b) for b in range(B)])).to(dev)
        if compat:
            pe = outlier.VolumetricPositionEncoding(outlier.DEFAULT_CONFIG)(pos)
        else:
            ang = torch.rand(B * M, C // 2, generator=g).to(dev) * 6 - 3
            pe = torch.stack([torch.cos(ang).repeat_interleave(2, 1), torch.sin(ang).repeat_interleave(2, 1)], -1).contiguous()
        off = [b * M for b in range(B + 1)]
        bat = lambda x: x.view(B, M, *x.shape[1:])
        kw = {"pos_q": pos, "pos_k": pos, "sigma_spat": SIGMA} if compat else {}
        comp = eager_compat(bat(pos), SIGMA) if compat else None
        ours = fwd_bwd(lambda: ops.attention_fn(q, k, v, H, pe, pe, offsets_q=off, offsets_k=off, **kw), (q, k, v), do)
        eager = fwd_bwd(lambda: eager_attention(bat(q), bat(k), bat(v), H, bat(pe), bat(pe), comp).reshape(B * M, C), (q, k, v), do)
        ms, mem = timed(ours, runs)
        mine = [t.grad.clone() for t in (q, k, v)]
        ems, emem = timed(eager, runs)
        err = max(float((a - t.grad).abs().max()) for a, t in zip(mine, (q, k, v)))
        lines.append(f"{'compatibility ' if compat else 'plain '}attention forward + backward, B = {B} x (L = S = {M}, C = {C}, H = {H})")
        lines.append(f"  ops.attention_fn     {ms:8.3f} ms  peak {mem / 2**20:8.2f} MiB")
        lines.append(f"  eager float32        {ems:8.3f} ms  peak {emem / 2**20:8.2f} MiB  {mark(ms, ems)}   max |gradient difference| {err:.2e}" + ("   (c given)" if compat else ""))
        if not compat:
            sms, smem = timed(fwd_bwd(lambda: sdpa(bat(q), bat(k), bat(v), H, bat(pe), bat(pe)).reshape(B * M, C), (q, k, v), do), runs)
            lines.append(f"  F.sdpa float32       {sms:8.3f} ms  peak {smem / 2**20:8.2f} MiB  {mark(ms, sms)}")
        print("\n".join(lines[-(3 if compat else 4):]), flush=True)
        del comp


class EagerLayer(outlier.CorrespondenceAttentionLayer):
    comp = None

    def forward_grad(self, x, source, x_pe, source_pe, x_lens=None, source_lens=None, x_pos=None, source_pos=None):
        B = len(x_lens)
        bat = lambda t: t.view(B, -1, *t.shape[1:])
        o = eager_attention(bat(self.q_proj(x)), bat(self.k_proj(source)), bat(self.v_proj(source)), self.nhead, bat(x_pe), bat(source_pe),
                            EagerLayer.comp).reshape(x.shape)
        message = self.norm1(self.merge(o))
        return x + self.norm2(self.mlp(torch.cat([x, message], dim=1)))


for M in (256, 1000, 2000):
    torch.manual_seed(0)
    net = outlier.Outlier_Rejection(outlier.DEFAULT_CONFIG).to(dev)
    opt = torch.optim.Adam(net.parameters(), lr=0.0)                   # the step is taken and leaves the weights: both ways time the same net
    n_out = int(0.4 * M)
    v6, labels = outlier.synthetic_matches(M - n_out, n_out, M, dev)
    ours = lambda: outlier.train_step(net, opt, v6, [M], labels)
    ms, mem = timed(ours, runs)
    loss = float(ours())
    for layer in net._6D_geometry_layers:
        layer.__class__ = EagerLayer

    def eager():
        EagerLayer.comp = eager_compat(v6.view(1, M, 6), SIGMA)
        out = outlier.train_step(net, opt, v6, [M], labels)
        EagerLayer.comp = None
        return out
    ems, emem = timed(eager, runs)
    lines.append(f"Outlier_Rejection training step (forward, loss, backward, Adam), {M} matches, {outlier.DEFAULT_CONFIG['num_layers']} layers, C = 144, H = 8")
    lines.append(f"  HIP attention        {ms:8.3f} ms  peak {mem / 2**20:8.2f} MiB")
    lines.append(f"  eager attention      {ems:8.3f} ms  peak {emem / 2**20:8.2f} MiB  {mark(ms, ems)}   |loss difference| {abs(loss - float(eager())):.2e}")
    print("\n".join(lines[-3:]), flush=True)

out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "attention_bwd_bench.txt")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(f"tools/attention_bwd_bench.py, {torch.cuda.get_device_name(0)}, median of {runs} calls, device events\n" + "\n".join(lines) + "\n")
