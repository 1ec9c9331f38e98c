"""ops.kpconv and the KPFCN coarse forward on the HIP path next to an eager float32 torch restatement of the reference's op sequence
on the same GPU:
    python tools/kpfcn_bench.py [runs [output file]]
Operator shapes (N = Nq = Ns, H, Cin -> Cout), K = 15, linear / sum / normalised: (20 000, 32, 64), (6 000, 32, 128), (2 000, 32, 256),
(600, 32, 512) and the first layer (20 000, 24, 1 -> 128).  Points are tests/_kpconv_ref.surface_cloud, tables ops.radius_search at
r = 0.025 * 2^level cut to H, so rows carry shadows as real tables do.  The eager side is KPConv.forward of the reference written
out in torch (the [N,H,K,3] differences, the [N,K,H] influences, the gathered [N,H,Cin] features, two matmuls, the normalisation):
the yardstick for time.  Device events around one call, every shape warmed up first, the median of `runs` calls; peak memory is
torch.cuda.max_memory_allocated over one call, inputs excluded.  The fraction of the 157.3 TFLOP/s f32-MFMA peak counts
2 Nq K Cin (Cout + mean valid H) FLOP.  Then one coarse forward at first_feats_dim 256 on a 2 x 10 000-point pair, with the share of
its device time spent inside ops.kpconv (the rest: unary GEMMs, instance norm, gathers).
Output: profiles/kpfcn_bench.txt unless another file is named."""
import os, statistics, sys
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import kpconv, kpfcn, ops
from tests import _kpconv_ref as R
from tests import _kpfcn_ref as K

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
PEAK = 157.3e12


def timed(fn, runs):
    """Median device milliseconds of fn() over `runs` calls, each between its own pair of events (two warm-up calls first)."""
    fn(); fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(runs):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return statistics.median(ms)


def peak_mb(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    out = fn()
    torch.cuda.synchronize()
    del out
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def eager_kpconv(q, s, idx, x, W, kp, extent):
    """blocks.py KPConv.forward, linear / sum, not deformable, op for op"""
    s = torch.cat((s, torch.zeros_like(s[:1]) + 1e6), 0)
    neighbors = s[idx] - q.unsqueeze(1)
    sq = ((neighbors.unsqueeze(2) - kp) ** 2).sum(3)
    w = torch.clamp(1 - torch.sqrt(sq) / extent, min=0.0).transpose(1, 2)
    x = torch.cat((x, torch.zeros_like(x[:1])), 0)
    nx = x[idx]
    out = torch.matmul(torch.matmul(w, nx).permute(1, 0, 2), W).sum(0)
    num = torch.gt(nx.sum(-1), 0.0).sum(-1)
    return out / torch.max(num, torch.ones_like(num)).unsqueeze(1)


lines = []
g = torch.Generator().manual_seed(0)
for n, H, cin, cout, level in ((20000, 32, 64, 64, 0), (6000, 32, 128, 128, 1), (2000, 32, 256, 256, 2), (600, 32, 512, 512, 3), (20000, 24, 1, 128, 0)):
    radius = K.RADIUS * 2 ** level
    pts = torch.from_numpy(R.surface_cloud(n, 700 + level, density=10000.0 / 4 ** level)).to(dev)
    idx, counts = ops.radius_search(pts, pts, [n], [n], radius, H)
    idx64 = idx.long()
    x = torch.ones(n, 1, device=dev) if cin == 1 else torch.randn(n, cin, generator=g).to(dev)
    W = (torch.randn(15, cin, cout, generator=g) / (15 * cin) ** 0.5).to(dev)
    kp = kpfcn.default_kernel_points(15, radius).to(dev)
    extent = radius * 2.0 / 2.5
    hip = lambda: ops.kpconv(pts, pts, idx, x, W, kp, extent)
    eager = lambda: eager_kpconv(pts, pts, idx64, x, W, kp, extent)
    diff = float((hip() - eager()).abs().max())
    ms, ms_eager = timed(hip, runs), timed(eager, runs)
    valid = float(counts.clamp(max=H).float().mean())
    flop = 2.0 * n * 15 * cin * (cout + valid)
    note = "" if ms <= ms_eager else "   SLOWER than eager"
    lines.append(f"kpconv N = {n:5d} H = {H} {cin:3d} -> {cout:3d} (mean valid H {valid:4.1f}): {ms:8.4f} ms   eager float32 torch {ms_eager:8.4f} ms "
                 f"({ms_eager / ms:5.2f} x)   {flop / ms / 1e9:7.2f} TFLOP/s = {100 * flop / (ms * 1e-3) / PEAK:4.1f} % of the f32-MFMA peak   "
                 f"peak memory {peak_mb(hip):7.1f} MB, eager {peak_mb(eager):7.1f} MB   max |hip - eager| {diff:.1e}{note}")
    print(lines[-1], flush=True)

# one coarse forward at Lepard's width
cfg = dict(K.F23_CONFIG, first_feats_dim=256, coarse_feature_dim=528, fine_feature_dim=264)
torch.manual_seed(0)
model = kpfcn.KPFCN(cfg).to(dev).eval()
pts = torch.from_numpy(np.concatenate([R.surface_cloud(10000, 800 + k, shift=(0.2 * k, 0.0, 0.1 * k)) for k in range(2)])).to(dev)
batch = kpconv.build_pyramid(pts, [10000, 10000], cfg["first_subsampling_dl"], cfg["conv_radius"], cfg["deform_radius"], cfg["architecture"], R.PYRAMID_LIMITS)
batch["features"] = torch.ones(pts.shape[0], 1, device=dev)
spent, real = [], ops.kpconv


def clocked(*a, **kw):
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    y = real(*a, **kw)
    t1.record()
    spent.append((t0, t1))
    return y


with torch.no_grad():
    fwd = lambda: model(batch, phase="coarse")
    ms = timed(fwd, runs)
    mem = peak_mb(fwd)
    ops.kpconv = clocked
    try:
        fwd()
        torch.cuda.synchronize()
    finally:
        ops.kpconv = real
    inside = sum(a.elapsed_time(b) for a, b in spent)
    real_eager = kpfcn.KPConv.forward
    kpfcn.KPConv.forward = lambda self, q, s, i, x: eager_kpconv(q, s, i, x, self.weights, self.kernel_points, self.KP_extent)
    try:
        ms_eager = timed(fwd, max(3, runs // 3))
        mem_eager = peak_mb(fwd)
    finally:
        kpfcn.KPConv.forward = real_eager
levels = [int(p.shape[0]) for p in batch["points"]]
note = "" if ms <= ms_eager else "   SLOWER than eager"
lines.append(f"KPFCN coarse forward, first_feats_dim 256, 2 x 10000 points (levels {levels}): {ms:8.3f} ms, {len(spent)} ops.kpconv calls take "
             f"{inside:8.3f} ms = {100 * inside / ms:4.1f} % of it; with the eager convolution {ms_eager:8.3f} ms ({ms_eager / ms:5.2f} x)   "
             f"peak memory {mem:7.1f} MB, eager {mem_eager:7.1f} MB{note}")
print(lines[-1], flush=True)

text = (f"tools/kpfcn_bench.py on {torch.cuda.get_device_name(0)}: median of {runs} calls, device events around one call "
        "(allocations and launches included), K = 15, linear / sum / normalised\n" + "\n".join(lines) + "\n")
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "kpfcn_bench.txt")
with open(out_path, "w") as f:
    f.write(text)
print(text)
