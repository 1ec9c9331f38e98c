"""The compatibility-modulated attention and one whole nine-layer Outlier_Rejection forward on the HIP path next to the reference's
sequence of operations in eager float32 torch on the same GPU:
    python tools/outlier_bench.py [runs [output file]]
Device events around one call, every shape warmed up first, the median of `runs` calls.  A call is ops.attention with positions and
sigma_spat, with its allocations and offset copies.  The eager side is the reference's own sequence (pipeline.py:52-58,
geometry_attention.py:56-97) on the [B, M, ...] batch: the compatibility matrix c from the [B, M, M, 3] differences -- timed on its
own line, because the reference takes it once per forward and hands it to all nine layers --, then the rotation of q and k, einsum to
[B, M, M, H] scores, times c, scale, soft-max, einsum with v.  The shapes have equal problems, so the eager batch carries no padding.
Peak memory is torch.cuda.max_memory_allocated over one call above what was allocated before it.  The network forward is
outlier.Outlier_Rejection at outlier.DEFAULT_CONFIG against the same modules with their attention replaced by the eager sequence and
c taken once.
Output: profiles/outlier_bench.txt unless another file is named."""
import os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import ops, outlier
from tests import _outlier_ref as O

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
C, H, SIGMA = 144, 8, 0.1
SHAPES = ((256, 1), (1000, 1), (2000, 1), (700, 8))                   # (M, B)


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
    """pipeline.py:54-58 on [B, M, 6]."""
    src, tgt = pos6d[..., :3], pos6d[..., 3:]
    src_dist = torch.norm(src[:, :, None, :] - src[:, None, :, :], dim=-1)
    tgt_dist = torch.norm(tgt[:, :, None, :] - tgt[:, None, :, :], dim=-1)
    return torch.clamp(1.0 - (src_dist - tgt_dist) ** 2 / sigma ** 2, min=0)


def eager_attention(q, k, v, H, pe_q, pe_k, comp):
    """geometry_attention.py:56-97 on [B, M, C] (no padding, so no mask)."""
    B, D = q.shape[0], q.shape[2] // H
    if pe_q is not None:
        q, k = rot(q, pe_q), rot(k, pe_k)
    a = torch.einsum("nlhd,nshd->nlsh", q.view(B, -1, H, D), k.view(B, -1, H, D))
    a = a * comp[..., None]
    a = torch.softmax(a / D ** 0.5, dim=2)
    return torch.einsum("nlsh,nshd->nlhd", a, v.view(B, -1, H, D)).reshape(B, -1, H * D)


def mark(ours, other):
    return f"{other / ours:5.2f}x" if ours <= other else f"**{other / ours:5.2f}x (slower than eager)**"


def clouds(M, B):
    return torch.from_numpy(np.concatenate([O.matches(M, 1000 * M + b) for b in range(B)])).to(dev)


lines = []
for M, B in SHAPES:
    g = torch.Generator().manual_seed(M + B)
    q, k, v = (torch.randn(B * M, C, generator=g).to(dev) for _ in range(3))
    pos = clouds(M, B)
    pe = outlier.VolumetricPositionEncoding(outlier.DEFAULT_CONFIG)(pos)
    off = [b * M for b in range(B + 1)]
    bat = lambda x: x.view(B, M, *x.shape[1:])
    ours = lambda: ops.attention(q, k, v, H, pe, pe, offsets_q=off, offsets_k=off, pos_q=pos, pos_k=pos, sigma_spat=SIGMA)
    comp = eager_compat(bat(pos), SIGMA)
    eager = lambda: eager_attention(bat(q), bat(k), bat(v), H, bat(pe), bat(pe), comp)
    ms, mem = timed(ours, runs)
    pms, pmem = timed(lambda: ops.attention(q, k, v, H, pe, pe, offsets_q=off, offsets_k=off), runs)
    ems, emem = timed(eager, runs)
    cms, cmem = timed(lambda: eager_compat(bat(pos), SIGMA), runs)
    err = float((ours() - eager().reshape(B * M, C)).abs().max())
    share = float((comp > 0).float().mean())
    lines.append(f"compatibility attention B = {B} x (M = {M}, C = {C}, H = {H}): {B * H * ((M + 15) // 16)} workgroups, c > 0 on {100 * share:.1f} % of the pairs")
    lines.append(f"  ops.attention + c    {ms:8.3f} ms  peak {mem / 2**20:8.2f} MiB   (the plain ops.attention: {pms:.3f} ms)")
    lines.append(f"  eager float32        {ems:8.3f} ms  peak {emem / 2**20:8.2f} MiB  {mark(ms, ems)}   max |difference| {err:.2e}   (c given)")
    lines.append(f"  eager c itself       {cms:8.3f} ms  peak {cmem / 2**20:8.2f} MiB  once per forward; with it {mark(ms, ems + cms)}")
    print("\n".join(lines[-4:]), flush=True)
    del comp


class EagerLayer(outlier.CorrespondenceAttentionLayer):
    comp = None

    def forward(self, x, source, x_pe, source_pe, x_lens=None, source_lens=None, x_pos=None, source_pos=None):
        B = len(x_lens)
        bat = lambda t: t.view(B, -1, *t.shape[1:])
        o = eager_attention(bat(self.q_proj(x)), bat(self.k_proj(source)), bat(self.v_proj(source)), self.nhead, bat(x_pe), bat(source_pe),
                            EagerLayer.comp).reshape(x.shape)
        message = self.norm1(self.merge(o))
        return x + self.norm2(self.mlp(torch.cat([x, message], dim=1)))


for M, B in SHAPES:
    torch.manual_seed(0)
    net = outlier.Outlier_Rejection(outlier.DEFAULT_CONFIG).to(dev).eval()
    pos, lens = clouds(M, B), [M] * B
    ours = lambda: net.confidence(pos, lens)
    ms, mem = timed(ours, runs)
    mine = ours()
    for layer in net._6D_geometry_layers:
        layer.__class__ = EagerLayer

    def eager():
        EagerLayer.comp = eager_compat(pos.view(B, M, 6), SIGMA)
        out = net.confidence(pos, lens)
        EagerLayer.comp = None
        return out
    with torch.no_grad():
        ems, emem = timed(eager, runs)
        err = float((mine - eager()).abs().max())
    lines.append(f"Outlier_Rejection forward, {B} x {M} matches, {outlier.DEFAULT_CONFIG['num_layers']} layers, C = {C}, H = {H}")
    lines.append(f"  HIP attention        {ms:8.3f} ms  peak {mem / 2**20:8.2f} MiB")
    lines.append(f"  eager attention      {ems:8.3f} ms  peak {emem / 2**20:8.2f} MiB  {mark(ms, ems)}   max |confidence difference| {err:.2e}")
    print("\n".join(lines[-3:]), flush=True)

out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "outlier_bench.txt")
os.makedirs(os.path.dirname(out), exist_ok=True)
with open(out, "w") as f:
    f.write(f"tools/outlier_bench.py, {torch.cuda.get_device_name(0)}, median of {runs} calls, device events\n" + "\n".join(lines) + "\n")
