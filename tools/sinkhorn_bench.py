"""Sinkhorn baseline timing on the HIP path next to the eager float32 restatement on the same GPU:
    python tools/sinkhorn_bench.py [n] [reps]
Device events around work that ends in a synchronise; every shape is warmed up first."""
import ctypes
import os, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import _native as N
from deformationpyramid_amd import ops
from deformationpyramid_amd.config import load_config
from deformationpyramid_amd.registration import Registration
from deformationpyramid_amd.sinkhorn import epsilon_schedule
from deformationpyramid_amd.synthetic import synthetic_pair
from tests import _sinkhorn_ref as R

n = int(sys.argv[1]) if len(sys.argv) > 1 else 2000
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 200
cfg = load_config(os.path.join(ROOT, "config", "baselines", "Sinkhorn.yaml"), device=0)
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


x, y = R.box_clouds(n, n, 0)
xd, yd = x.to(dev), y.to(dev)
L = len(epsilon_schedule(R.diameter(x, y), cfg.blur, 0.5))
launches = L + 1                                            # initialisation + one step per epsilon, four soft-minima each
pairs = (launches + 1) * (2 * n * n + 2 * n * n)            # + the final kernel; one exponential per (row, column) pair
blocks = (n + 15) // 16
print(f"shape {n} x {n}, blur {cfg.blur}, reach {cfg.reach}: {L} epsilons, {launches} step launches of {4 * blocks} workgroups, "
      f"final kernel {2 * blocks} workgroups (256 threads each)")

# the kernels alone: the C entry with the diameter and the workspace in hand (no host read, no allocation)
nf = ctypes.c_longlong()
N.check(N.lib().ndp_sinkhorn_workspace(n, n, ctypes.byref(nf)), "workspace")
ws = torch.empty(nf.value // 2 + 1, device=dev, dtype=torch.float64)
loss, gx = torch.empty(1, device=dev), torch.empty_like(xd)
diam = R.diameter(x, y)
entry = lambda: N.check(N.lib().ndp_sinkhorn_divergence(ops._p(xd), n, ops._p(yd), n, float(cfg.blur), float(cfg.reach), 0.5, diam, ops._p(ws),
                                                        ops._p(loss), ops._p(gx), None, N.stream_ptr(dev)), "ndp_sinkhorn_divergence")
ms_entry = timed(entry, reps)
print(f"HIP kernels (ndp_sinkhorn_divergence, loss + gradient): {ms_entry:.4f} ms per call; {pairs / ms_entry / 1e9:.3f} T exponentials/s over the "
      f"whole call ({launches + 2} launches, gaps included)")
ms_op = timed(lambda: ops.sinkhorn_divergence(xd, yd, cfg.blur, cfg.reach), reps)
print(f"HIP operator (ops.sinkhorn_divergence: + diameter read, allocations): {ms_op:.4f} ms per call")
ms_eager = timed(lambda: R.sinkhorn_ref(xd, yd, cfg.blur, cfg.reach, dtype=torch.float32, device=dev), max(3, reps // 20))
print(f"eager float32 restatement on the same GPU (loss + gradient): {ms_eager:.4f} ms per call  ({ms_eager / ms_op:.1f} x the operator)")

# the 11-step registration of the shipped config on a synthetic pair (8192 source points, 2000 samples)
model = Registration(cfg)
src, tgt, _, _ = synthetic_pair(1)
model.load_pcds(src, tgt)
torch.manual_seed(0)
ms_reg = timed(lambda: model.register(), max(3, reps // 20))
print(f"Registration.register(), {cfg.Nsteps} Euler steps at {cfg.samples} samples: {ms_reg:.3f} ms per pair")
torch.manual_seed(0)
s = src[torch.randperm(src.shape[0])[: cfg.samples]].to(dev)
t = tgt[torch.randperm(tgt.shape[0])[: cfg.samples]].to(dev)


def eager_loop():
    xi = s
    for _ in range(cfg.Nsteps):
        xi = xi - cfg.lr * len(xi) * R.sinkhorn_ref(xi, t, cfg.blur, cfg.reach, dtype=torch.float32, device=dev).grad
    return xi


ms_loop = timed(eager_loop, 3)
print(f"the same loop on the eager float32 restatement: {ms_loop:.3f} ms per pair  ({ms_loop / ms_reg:.1f} x)")
