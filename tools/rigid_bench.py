"""Rigid-alignment operators' timing on the HIP path next to the eager float32 restatement (tests/_rigid_ref.py) on the same GPU:
    python tools/rigid_bench.py [runs [output file]]
Device events around one call, every shape warmed up first, the median of `runs` calls.  The hypotheses are drawn once, outside the
timed region, for both sides.  The eager RANSAC scores only the hypotheses its own checks accept, in one [accepted, K] matrix; its
3 x 3 SVDs run on the CPU, where the reference runs them.  Output: profiles/rigid_bench.txt unless another file is named."""
import os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import ops, rigid
from tests import _rigid_ref as R

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
THR = 0.05


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


def eager_score(T, s, y, thr):
    out = [R.score_ref(T[h:h + 8192], s, y, thr, torch.float32) for h in range(0, T.shape[0], 8192)]
    return torch.cat([o[0] for o in out]), torch.cat([o[1] for o in out])


lines = []
for K, H, B in ((500, 4096, 1), (1000, 50000, 1), (5000, 50000, 1), (500, 4096, 64)):
    probs = [R.planted(K, 0.3, 1 + b)[:2] for b in range(B)]
    s, y = torch.cat([p[0] for p in probs]).to(dev), torch.cat([p[1] for p in probs]).to(dev)
    offs = [b * K for b in range(B + 1)]
    tri = rigid.draw_triples([K] * B, H, 1).to(dev)
    ms_ransac = timed(lambda: ops.ransac_rigid(s, y, tri, THR, offsets=offs), runs)
    out = ops.ransac_rigid(s, y, tri, THR, offsets=offs, want_hypotheses=True)
    accepted = float((out["h_flags"] == 0).float().mean())
    ms_score = timed(lambda: ops.rigid_score(out["h_T"], s, y, THR, offsets=offs), runs)
    ms_fit = timed(lambda: ops.rigid_fit(s, y, mask=out["mask"], offsets=offs), runs)
    few = max(3, runs // 3)
    ms_eager = timed(lambda: [R.ransac_ref(s[offs[b]:offs[b + 1]], y[offs[b]:offs[b + 1]], tri[b], THR, dtype=torch.float32) for b in range(B)], few)
    ms_eager_score = timed(lambda: [eager_score(out["h_T"][b], s[offs[b]:offs[b + 1]], y[offs[b]:offs[b + 1]], THR) for b in range(B)], few)
    ms_eager_fit = timed(lambda: [R.procrustes_ref(s[None, offs[b]:offs[b + 1]], y[None, offs[b]:offs[b + 1]],
                                                   R.weights_of(K, mask=out["mask"][offs[b]:offs[b + 1]]).float(), dtype=torch.float32)
                                  for b in range(B)], few)
    lines.append(f"B = {B} x (K = {K}, H = {H}), {100 * accepted:.1f} % of the hypotheses accepted, inliers found {out['count'].tolist()[:4]}\n"
                 f"  ransac_rigid (3 launches, refine_iters 2) {ms_ransac:9.4f} ms   eager float32 restatement {ms_eager:10.3f} ms  ({ms_eager / ms_ransac:8.1f} x)\n"
                 f"  rigid_score of all B x H transforms       {ms_score:9.4f} ms   eager float32 restatement {ms_eager_score:10.3f} ms  ({ms_eager_score / ms_score:8.1f} x)\n"
                 f"  rigid_fit over the inlier mask            {ms_fit:9.4f} ms   eager float32 restatement {ms_eager_fit:10.3f} ms  ({ms_eager_fit / ms_fit:8.1f} x)")
    print(lines[-1], flush=True)

text = (f"tools/rigid_bench.py on {torch.cuda.get_device_name(0)}: median of {runs} calls (eager: {max(3, runs // 3)}), device events, "
        "wall time of one call including its allocations and launches\n" + "\n".join(lines) + "\n")
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "rigid_bench.txt")
with open(out_path, "w") as f:
    f.write(text)
