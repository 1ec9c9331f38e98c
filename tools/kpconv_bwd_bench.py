"""Forward + backward of ops.kpconv_fn (csrc/ndp_kpconv_conv.inc, csrc/ndp_kpconv_bwd.inc) next to the reference's op sequence in
eager float32 torch under autograd on the same GPU:
    python tools/kpconv_bwd_bench.py [runs [output file]]
The five operator shapes of tools/kpfcn_bench.py (N = Nq = Ns, H, Cin -> Cout), K = 15, linear / sum / normalised, the same points and
tables.  One timed call is y = conv(x, W); y.backward(dy) with both x and W requiring a gradient (the first layer's features are ones
and need none: there only W does).  Device events around one call, every shape warmed up first, the median of `runs` calls;
peak memory is torch.cuda.max_memory_allocated over one call, inputs excluded.  There is no speed threshold: a shape that is slower
than eager says so.  Not measured here: a kernel trace or hardware counters of the backward kernels.
Output: profiles/kpconv_bwd_bench.txt unless another file is named."""
import os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import kpfcn, ops
from tests import _kpconv_ref as R
from tests import _kpfcn_ref as K

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")


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
    want_dx = cin != 1
    x = (torch.ones(n, 1, device=dev) if cin == 1 else torch.randn(n, cin, generator=g).to(dev)).requires_grad_(want_dx)
    W = (torch.randn(15, cin, cout, generator=g) / (15 * cin) ** 0.5).to(dev).requires_grad_(True)
    dy = torch.randn(n, cout, generator=g).to(dev)
    kp = kpfcn.default_kernel_points(15, radius).to(dev)
    extent = radius * 2.0 / 2.5

    def step(conv, table):
        x.grad = W.grad = None
        conv(pts, pts, table, x, W, kp, extent).backward(dy)
        return (x.grad, W.grad)

    hip = lambda: step(ops.kpconv_fn, idx)
    eager = lambda: step(eager_kpconv, idx64)
    gh, ge = hip(), eager()
    diff = [float((a - b).abs().max() / b.abs().max()) for a, b in zip(gh, ge) if a is not None]
    ms, ms_eager = timed(hip, runs), timed(eager, runs)
    ms_fwd = timed(lambda: ops.kpconv(pts, pts, idx, x.detach(), W.detach(), kp, extent), runs)
    note = "" if ms <= ms_eager else "   SLOWER than eager"
    lines.append(f"kpconv_fn forward + backward N = {n:5d} H = {H} {cin:3d} -> {cout:3d} ({'dx and dW' if want_dx else 'dW only'}): {ms:8.4f} ms "
                 f"(its forward alone {ms_fwd:8.4f} ms)   eager float32 torch autograd {ms_eager:8.4f} ms ({ms_eager / ms:5.2f} x)   "
                 f"peak memory {peak_mb(hip):7.1f} MB, eager {peak_mb(eager):7.1f} MB   max |hip - eager| / max |eager| "
                 f"{' '.join(f'{d:.1e}' for d in diff)}{note}")
    print(lines[-1], flush=True)

text = (f"tools/kpconv_bwd_bench.py on {torch.cuda.get_device_name(0)}: median of {runs} calls, device events around one forward + backward "
        "(allocations and launches included), K = 15, linear / sum / normalised\n" + "\n".join(lines) + "\n")
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "kpconv_bwd_bench.txt")
with open(out_path, "w") as f:
    f.write(text)
print(text)
