"""Attention, the dense confidence matrix and one whole repositioning-transformer forward on the HIP path next to eager float32 torch
on the same GPU:
    python tools/lepard_bench.py [runs [output file]]
Device events around one call, every shape warmed up first, the median of `runs` calls.  A call is ops.attention / ops.feat_conf
with its allocations and offset copies.  The eager side is (a) the reference's own sequence of operations in float32 (the rotation
of q and k, einsum to [L, S, H] scores, scale, soft-max, einsum with v; per problem, one after the other, which is what an unpadded
batch costs it) and (b) F.scaled_dot_product_attention in float32 on the rotated operands where it runs.  Peak memory is
torch.cuda.max_memory_allocated over one call above what was allocated before it.  The transformer forward is
lepard.RepositioningTransformer at configs/lepard.yaml's layer types against the same modules with their attention, confidence
matrix and Procrustes fit replaced by the eager sequence.
Output: profiles/lepard_bench.txt unless another file is named."""
import os, statistics, sys
import torch
import torch.nn.functional as F
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import lepard, ops
from tests import _lepard_ref as P

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
PEAK = 157e12


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


def eager_attention(q, k, v, H, pe_q, pe_k):
    """transformer.py:59-82 on one problem."""
    q, k = rot(q, pe_q), rot(k, pe_k)
    D = q.shape[1] // H
    a = torch.einsum("lhd,shd->lsh", q.view(-1, H, D), k.view(-1, H, D)) / D ** 0.5
    a = torch.softmax(a, dim=1)
    return torch.einsum("lsh,shd->lhd", a, v.view(-1, H, D)).reshape(q.shape[0], -1)


def sdpa(q, k, v, H, pe_q, pe_k):
    q, k = rot(q, pe_q), rot(k, pe_k)
    D = q.shape[1] // H
    h = lambda x: x.view(-1, H, D).transpose(0, 1)[None]
    return F.scaled_dot_product_attention(h(q), h(k), h(v))[0].transpose(0, 1).reshape(q.shape[0], -1)


def mark(ours, other):
    return f"{other / ours:5.2f}x" if ours <= other else f"**{other / ours:5.2f}x (slower than eager)**"


lines = []
for L, S, C, H, B in ((500, 500, 528, 4, 1), (2000, 2000, 528, 4, 1), (800, 700, 528, 4, 8), (500, 500, 48, 4, 1), (2000, 2000, 48, 4, 1)):
    g = torch.Generator().manual_seed(L + S + C)
    q, k, v = (torch.randn(B * n, C, generator=g).to(dev) for n in (L, S, S))
    ang_q, ang_k = torch.rand(B * L, C // 2, generator=g) * 6, torch.rand(B * S, C // 2, generator=g) * 6
    code = lambda a: torch.stack([a.cos(), a.sin()], -1).repeat_interleave(2, dim=1).contiguous().to(dev)
    pe_q, pe_k = code(ang_q), code(ang_k)
    oq, ok = [b * L for b in range(B + 1)], [b * S for b in range(B + 1)]
    ours = lambda: ops.attention(q, k, v, H, pe_q, pe_k, offsets_q=oq, offsets_k=ok)
    per = lambda fn: (lambda: [fn(q[oq[b]:oq[b + 1]], k[ok[b]:ok[b + 1]], v[ok[b]:ok[b + 1]], H, pe_q[oq[b]:oq[b + 1]], pe_k[ok[b]:ok[b + 1]]) for b in range(B)])
    ms, mem = timed(ours, runs)
    ems, emem = timed(per(eager_attention), runs)
    err = float((ours() - torch.cat(per(eager_attention)())).abs().max())
    flop = 4.0 * B * L * S * C
    lines.append(f"attention B = {B} x (L = {L}, S = {S}, C = {C}, H = {H}): {B * H * ((L + 15) // 16)} workgroups")
    lines.append(f"  ops.attention        {ms:8.3f} ms  peak {mem / 2**20:8.2f} MiB  {flop / ms / 1e9:7.2f} TFLOP/s = {100 * flop / ms / 1e9 / (PEAK / 1e12):5.2f} % of the f32 MFMA peak")
    lines.append(f"  eager float32        {ems:8.3f} ms  peak {emem / 2**20:8.2f} MiB  {mark(ms, ems)}   max |difference| {err:.2e}")
    try:
        sms, smem = timed(per(sdpa), runs)
        lines.append(f"  F.sdpa float32       {sms:8.3f} ms  peak {smem / 2**20:8.2f} MiB  {mark(ms, sms)}")
    except Exception as e:                                          # no float32 backend on this build: say so
        lines.append(f"  F.sdpa float32       does not run here: {type(e).__name__}: {str(e)[:80]}")
    print("\n".join(lines[-4:]), flush=True)

for S, T, C, B in ((500, 500, 528, 1), (2000, 2000, 528, 1), (800, 700, 528, 8)):
    g = torch.Generator().manual_seed(S + T)
    fs, ft = torch.randn(B * S, C, generator=g).to(dev), torch.randn(B * T, C, generator=g).to(dev)
    os_, ot = [b * S for b in range(B + 1)], [b * T for b in range(B + 1)]
    ours = lambda: ops.feat_conf(fs, ft, 0.1, offsets_s=os_, offsets_t=ot)

    def eager():
        out = []
        for b in range(B):
            sim = (fs[os_[b]:os_[b + 1]] @ ft[ot[b]:ot[b + 1]].T) / (C * 0.1)
            out.append(torch.softmax(sim, 0) * torch.softmax(sim, 1))
        return out
    ms, mem = timed(ours, runs)
    ems, emem = timed(eager, runs)
    err = float((ours() - torch.stack(eager())).abs().max())
    lines.append(f"feat_conf B = {B} x (S = {S}, T = {T}, C = {C})")
    lines.append(f"  ops.feat_conf        {ms:8.3f} ms  peak {mem / 2**20:8.2f} MiB  (the matrix itself is {4 * B * S * T / 2**20:.2f} MiB)")
    lines.append(f"  eager float32        {ems:8.3f} ms  peak {emem / 2**20:8.2f} MiB  {mark(ms, ems)}   max |difference| {err:.2e}")
    print("\n".join(lines[-3:]), flush=True)


class EagerLayer(lepard.GeometryAttentionLayer):
    def forward(self, x, source, x_pe, source_pe, x_lens=None, source_lens=None):
        o = eager_attention(self.q_proj(x), self.k_proj(source), self.v_proj(source), self.nhead, x_pe, source_pe)
        message = self.norm1(self.merge(o))
        return x + self.norm2(self.mlp(torch.cat([x, message], dim=1)))


for n, C in ((500, 528), (2000, 528)):
    cfg = P.transformer_config(C, 4)
    torch.manual_seed(0)
    net = lepard.RepositioningTransformer(cfg).to(dev)
    g = torch.Generator().manual_seed(n)
    src, tgt = torch.randn(n, C, generator=g).to(dev), torch.randn(n, C, generator=g).to(dev)
    s_pcd = (torch.rand(n, 3, generator=g) + torch.tensor(P.VOL_BNDS[0])).to(dev)
    t_pcd = (torch.rand(n, 3, generator=g) + torch.tensor(P.VOL_BNDS[0])).to(dev)
    ours = lambda: net(src, tgt, s_pcd, t_pcd)
    ms, mem = timed(ours, runs)
    for layer in net.layers:
        if isinstance(layer, lepard.GeometryAttentionLayer):
            layer.__class__ = EagerLayer
    with torch.no_grad():
        ems, emem = timed(ours, runs)
    lines.append(f"RepositioningTransformer forward, one pair of {n} + {n} coarse points, C = {C}, H = 4, layers {cfg.layer_types}")
    lines.append(f"  HIP attention        {ms:8.3f} ms  peak {mem / 2**20:8.2f} MiB")
    lines.append(f"  eager attention      {ems:8.3f} ms  peak {emem / 2**20:8.2f} MiB  {mark(ms, ems)}   (positioning layer unchanged: ops.feat_conf, topk, ops.rigid_fit)")
    print("\n".join(lines[-3:]), flush=True)

out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "lepard_bench.txt")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(f"tools/lepard_bench.py, {torch.cuda.get_device_name(0)}, median of {runs} calls, device events\n" + "\n".join(lines) + "\n")
