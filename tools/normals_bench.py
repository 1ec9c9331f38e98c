"""Surface-normal operators' timing on the HIP path next to the eager float32 restatement on the same GPU:
    python tools/normals_bench.py [reps]
Device events around work that ends in a synchronise; every shape is warmed up first."""
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import ops
from deformationpyramid_amd.normals import estimate_normals
from deformationpyramid_amd.synthetic import surface_pair
from tests import _normals_ref as R

reps = int(sys.argv[1]) if len(sys.argv) > 1 else 20
dev = torch.device("cuda:0")


def timed(fn, reps):
    """Mean device milliseconds of fn() over `reps` back-to-back calls (one warm-up call first)."""
    fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps


def eager_normals(p, K):
    """k nearest neighbours by topk over 2048-row blocks of the distance matrix, then the restatement's covariance and eigh, in float32."""
    idx = torch.cat([((p[s:s + 2048, None, :] - p[None, :, :]) ** 2).sum(-1).topk(K, dim=1, largest=False).indices for s in range(0, len(p), 2048)])
    return R.pca_ref(p, idx, torch.float32).normal


def eager_nn(x, y):
    d = ((x[:, None, :] - y[None, :, :]) ** 2).sum(-1)
    a, b = d.min(dim=1), d.min(dim=0)
    return a.values, a.indices.int(), b.values, b.indices.int()


K = 16
for n in (8192, 30000):
    p = surface_pair(2, 2 * n, partial=False)[0].contiguous().to(dev)
    ms_knn = timed(lambda: ops.knn(p, p, K), reps)
    idx = ops.knn(p, p, K)[1]
    ms_pca = timed(lambda: ops.normals_from_knn(p, idx), reps)
    ms_all = timed(lambda: estimate_normals(p, k=K), reps)
    ms_eager = timed(lambda: eager_normals(p, K), max(2, reps // 10))
    print(f"estimate_normals, {n} points, K = {K}: {ms_all:.3f} ms (knn {ms_knn:.3f} ms = {n * n / ms_knn / 1e9:.3f} T distances/s, "
          f"PCA {ms_pca:.4f} ms); eager float32 restatement on the same GPU {ms_eager:.3f} ms ({ms_eager / ms_all:.1f} x)")

for n in (2000, 6000):
    x, y = R.random_cloud(n, 1).to(dev), (R.random_cloud(n, 2) * 1.1 + 0.02).to(dev)
    nx = torch.nn.functional.normalize(R.random_cloud(n, 3), dim=1).contiguous().to(dev)
    ny = torch.nn.functional.normalize(R.random_cloud(n, 4), dim=1).contiguous().to(dev)
    nn = ops.chamfer_nn(x, y)
    for mode in (0, 1):
        ms_k = timed(lambda: ops.point_to_plane(x, y, nx, ny, mode=mode, nn=nn), reps)
        ms_op = timed(lambda: ops.point_to_plane(x, y, nx, ny, mode=mode), reps)
        ms_eager = timed(lambda: R.point_to_plane_autograd(x, y, nx, ny, eager_nn(x, y), mode=mode, dtype=torch.float32), max(2, reps // 10))
        print(f"point_to_plane, {n} x {n}, mode {mode}, values + gradient in x: {ms_k:.4f} ms on a given search, {ms_op:.4f} ms with its own search; "
              f"eager float32 restatement (search + autograd, gradients in x and y) {ms_eager:.3f} ms ({ms_eager / ms_op:.1f} x)")
