"""The KPConv input operators' timing on the HIP path next to an eager float32 torch restatement on the same GPU and the numpy
restatement (tests/_kpconv_ref.py) on the host:
    python tools/kpconv_bench.py [runs [output file]]
Synthetic surface clouds (tests/_kpconv_ref.surface_cloud: about one point per 0.01-voxel) of 2 x 5 000, 2 x 30 000 and 16 x 20 000
points; the numbers of configs/lepard.yaml (first_subsampling_dl 0.01, conv_radius 2.5, deform_radius 5.0), four levels.
  voxel_subsample   ops.voxel_subsample at dl = 0.02 (the first pooling)
  radius_search     ops.radius_search of the cloud against itself at r = 0.025, K = 24 (the first convolution table)
  build_pyramid     kpconv.build_pyramid: 4 conv tables, 3 subsamplings, 3 pool and 3 upsample tables
Device events around one call (both operators end in a synchronise of their own: the time is a call's wall time on the device
clock, allocations and the host-side part included), every shape warmed up first, the median of `runs` calls.
The eager side is what one writes in torch without this library: per cloud, voxel keys + unique + index_add_ for the barycentres;
for the neighbours the |q|^2 + |s|^2 - 2 q.s distance matrix in chunks of 4096 queries, a mask and topk.  Its distances are not
the kernels' chain, so its tables can differ in the last neighbour; it is a clock, not a yardstick.  The numpy side is the test
restatement, brute force in float64 with Python loops: timed once, and only where its n x n matrices fit (2 x 5 000).
Output: profiles/kpconv_bench.txt unless another file is named."""
import os, statistics, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import kpconv, ops
from tests import _kpconv_ref as R

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
LIMITS = R.PYRAMID_LIMITS
CFG = R.LEPARD


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


def eager_voxel(p, lengths, dl):
    out, out_l, a = [], [], 0
    for n in lengths:
        c = p[a:a + n]
        origin = torch.floor(c.min(0).values * (1.0 / dl)) * dl
        i = torch.floor((c - origin) / dl).long()
        _, inv = torch.unique((i[:, 2] << 32) + (i[:, 1] << 16) + i[:, 0], return_inverse=True)
        m = int(inv.max()) + 1
        acc = torch.zeros(m, 3, device=p.device).index_add_(0, inv, c)
        out.append(acc / torch.bincount(inv, minlength=m)[:, None])
        out_l.append(m)
        a += n
    return torch.cat(out), out_l


def eager_radius(q, s, ql, sl, radius, K):
    r2 = float(np.float32(radius) * np.float32(radius))
    shadow, rows, qa, sa = s.shape[0], [], 0, 0
    for nq, ns in zip(ql, sl):
        sc = s[sa:sa + ns]
        s2 = (sc * sc).sum(1)[None, :]
        for c0 in range(qa, qa + nq, 4096):
            qc = q[c0:min(c0 + 4096, qa + nq)]
            d2 = (qc * qc).sum(1)[:, None] + s2 - 2.0 * (qc @ sc.T)
            d2 = torch.where(d2 < r2, d2, torch.full_like(d2, float("inf")))
            val, idx = torch.topk(d2, min(K, ns), dim=1, largest=False)
            rows.append(torch.where(torch.isinf(val), torch.full_like(idx, shadow), idx + sa))
        qa += nq
        sa += ns
    width = max(r.shape[1] for r in rows)
    return torch.cat([torch.nn.functional.pad(r, (0, width - r.shape[1]), value=shadow) for r in rows])


def eager_pyramid(p, lengths):
    r, out = CFG["first_subsampling_dl"] * CFG["conv_radius"], []
    for layer in range(4):
        out.append(eager_radius(p, p, lengths, lengths, r, LIMITS[layer]))
        if layer == 3:
            break
        sub, sub_l = eager_voxel(p, lengths, 2 * r / CFG["conv_radius"])
        out.append(eager_radius(sub, p, sub_l, lengths, r, LIMITS[layer]))
        out.append(eager_radius(p, sub, lengths, sub_l, 2 * r, LIMITS[layer]))
        p, lengths, r = sub, sub_l, 2 * r
    return out


def host_once(fn):
    t = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t)


lines = []
for B, n in ((2, 5000), (2, 30000), (16, 20000)):
    pts_np = np.concatenate([R.surface_cloud(n, 900 + b, shift=(0.1 * b, 0.0, 0.05 * b)) for b in range(B)])
    lengths = [n] * B
    pts = torch.from_numpy(pts_np).to(dev)
    dl, r0, K = 0.02, 0.025, LIMITS[0]
    small = B * n <= 10000
    lines.append(f"B = {B} x {n} points")
    rows = (
        ("voxel_subsample", lambda: ops.voxel_subsample(pts, lengths, dl), lambda: eager_voxel(pts, lengths, dl),
         lambda: R.voxel_subsample(pts_np, lengths, dl)),
        ("radius_search", lambda: ops.radius_search(pts, pts, lengths, lengths, r0, K), lambda: eager_radius(pts, pts, lengths, lengths, r0, K),
         (lambda: R.radius_search(pts_np, pts_np, lengths, lengths, r0, K)) if small else None),
        ("build_pyramid", lambda: kpconv.build_pyramid(pts, lengths, architecture=R.KPFCN, neighborhood_limits=LIMITS, **CFG),
         lambda: eager_pyramid(pts, lengths),
         (lambda: R.build_pyramid(pts_np, lengths, architecture=R.KPFCN, limits=LIMITS, **CFG)) if small else None),
    )
    for name, hip, eager, host in rows:
        ms = timed(hip, runs)
        ms_eager = timed(eager, max(3, runs // 3))
        ms_host = f"{host_once(host):10.1f} ms" if host is not None else "not measured"
        note = "" if ms <= ms_eager else "   SLOWER than eager"
        lines.append(f"  {name:16s} {ms:9.4f} ms   eager float32 torch {ms_eager:9.3f} ms ({ms_eager / ms:6.1f} x)   numpy on the host {ms_host}{note}")
        print(lines[-1], flush=True)
    sub = ops.voxel_subsample(pts, lengths, dl)
    idx, counts = ops.radius_search(pts, pts, lengths, lengths, r0, K)
    lines.append(f"  ({int(sub[1].sum())} voxels at dl = {dl}; neighbours within {r0}: mean {float(counts.float().mean()):.1f}, largest {int(counts.max())}, K = {K})")

text = (f"tools/kpconv_bench.py on {torch.cuda.get_device_name(0)}: median of {runs} calls (eager side: {max(3, runs // 3)}; numpy: one call), "
        "device events, wall time of one call including its allocations, launches and final synchronise\n" + "\n".join(lines) + "\n")
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "kpconv_bench.txt")
with open(out_path, "w") as f:
    f.write(text)
print(text)
