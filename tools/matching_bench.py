"""Descriptor matching's timing on the HIP path next to the eager float32 restatement (tests/_matching_ref.py) on the same GPU:
    python tools/matching_bench.py [runs [output file]]
Device events around one call, every shape warmed up first, the median of `runs` calls.  A call is ops.feat_match with its
allocations and all of its launches.  The eager side writes the S x T matrix out (per problem, one after the other), twice: `lean`
is the reference's own sequence of operations in float32 (soft-max or log-sum-exp, two `max`, the equality mask, stopping at the
dense mask without its `nonzero`), `yardstick` is the test restatement tests/_matching_ref.mode_ref, which also takes top-two gaps
and is heavier.  The k_feat_rowstats line is NOT a kernel time from a trace: it is the device-event time of one ndp_feat_rowstats
call through the C entry with outputs and offsets allocated beforehand (one launch and its launch overhead), next to the time of one
ops.feat_rowstats call (the same plus three allocations and two offset copies); the rate 2 S T C flop over the former, as a share of
the 157 TFLOP/s f32-input MFMA peak, is therefore a call's share and understates the kernel's.
Output: profiles/matching_bench.txt unless another file is named."""
import ctypes, math, os, statistics, sys
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from deformationpyramid_amd import _native as N, ops
from tests import _matching_ref as R

runs = int(sys.argv[1]) if len(sys.argv) > 1 else 9
dev = torch.device("cuda:0")
PEAK = 157e12


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


def lean_eager(mode, fs, ft, thr=0.1, bin_score=1.0, iters=3):
    """The reference's sequence of float32 operations for one problem, up to the dense mask of matches."""
    C = fs.shape[1]
    if mode == "mutual_nn":
        scores = fs @ ft.T
        r, c = scores.argmax(1), scores.argmax(0)
        return c[r] == torch.arange(fs.shape[0], device=fs.device)
    if mode == "dual_softmax":
        sim = (fs @ ft.T) / (C * R.TEMPERATURE)
        conf = torch.softmax(sim, 0) * torch.softmax(sim, 1)
    else:
        conf = R.sinkhorn_ref(fs, ft, bin_score, iters, dtype=torch.float32).exp()
    return (conf > thr) & (conf == conf.max(1, keepdim=True).values) & (conf == conf.max(0, keepdim=True).values)


lines = []
for S, T, C, B in ((2000, 2000, 528, 1), (5000, 5000, 32, 1), (800, 700, 528, 8)):
    probs = [R.planted_features(S, T, C, 1 + b)[:2] for b in range(B)]
    fs, ft = torch.cat([p[0] for p in probs]).to(dev), torch.cat([p[1] for p in probs]).to(dev)
    os_, ot = [b * S for b in range(B + 1)], [b * T for b in range(B + 1)]
    k = math.sqrt(1.0 / R.TEMPERATURE)
    feats = {"dual_softmax": (fs, ft), "sinkhorn": ((fs * k).contiguous(), (ft * k).contiguous()), "mutual_nn": (fs, ft)}
    lines.append(f"B = {B} x (S = {S}, T = {T}, C = {C})")
    for mode in R.MODES:
        a, b = feats[mode]
        thr = -math.inf if mode == "mutual_nn" else 0.1
        temp = 1.0 if mode == "mutual_nn" else R.TEMPERATURE
        call = lambda: ops.feat_match(a, b, mode=mode, temperature=temp, thr=thr, offsets_s=os_, offsets_t=ot)
        ms = timed(call, runs)
        n_match = int((call()[0] >= 0).sum())
        lean = lambda: [lean_eager(mode, a[os_[p]:os_[p + 1]], b[ot[p]:ot[p + 1]]) for p in range(B)]
        heavy = lambda: [R.mode_ref(mode, a[os_[p]:os_[p + 1]], b[ot[p]:ot[p + 1]], dtype=torch.float32) for p in range(B)]
        ms_lean, ms_heavy = timed(lean, max(3, runs // 3)), timed(heavy, max(3, runs // 3))
        note = "" if ms <= ms_lean else "   SLOWER than eager"
        lines.append(f"  feat_match {mode:12s} {ms:9.4f} ms   eager float32: lean {ms_lean:8.3f} ms ({ms_lean / ms:5.1f} x)  yardstick {ms_heavy:8.3f} ms "
                     f"({ms_heavy / ms:5.1f} x)   {n_match} matches{note}")
    alpha = 1.0 / (C * R.TEMPERATURE)
    ms_call = timed(lambda: ops.feat_rowstats(fs, ft, alpha, offsets_a=os_, offsets_b=ot), runs)
    oa, ob = torch.tensor(os_, dtype=torch.int32, device=dev), torch.tensor(ot, dtype=torch.int32, device=dev)
    ha, hb = (ctypes.c_int * len(os_))(*os_), (ctypes.c_int * len(ot))(*ot)
    lse, mx, arg = torch.empty(B * S, device=dev), torch.empty(B * S, device=dev), torch.empty(B * S, device=dev, dtype=torch.int32)
    P = lambda t: ctypes.c_void_p(t.data_ptr())
    entry = lambda: N.check(N.lib().ndp_feat_rowstats(P(fs), P(ft), P(oa), P(ob), ha, hb, B, C, alpha, None, None, P(lse), P(mx), P(arg),
                                                      N.stream_ptr(dev)), "ndp_feat_rowstats")
    ms_rows = timed(entry, runs)
    ms_mm = timed(lambda: [fs[os_[p]:os_[p + 1]] @ ft[ot[p]:ot[p + 1]].T for p in range(B)], runs)
    flop = 2.0 * B * S * T * C
    lines.append(f"  one ndp_feat_rowstats call, buffers preallocated (events, not a kernel trace) {ms_rows:9.4f} ms = {flop / ms_rows / 1e9:7.2f} TFLOP/s = "
                 f"{100 * flop / (ms_rows * 1e-3) / PEAK:5.1f} % of the 157 TFLOP/s f32-MFMA peak; one ops.feat_rowstats call {ms_call:9.4f} ms   "
                 f"(eager: the fp32 product alone, no statistics {ms_mm:9.4f} ms)")
    print("\n".join(lines[-5:]), flush=True)

text = (f"tools/matching_bench.py on {torch.cuda.get_device_name(0)}: median of {runs} calls (eager sides: {max(3, runs // 3)}), device events, "
        "wall time of one call including its allocations and launches\n" + "\n".join(lines) + "\n")
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "profiles", "matching_bench.txt")
with open(out_path, "w") as f:
    f.write(text)
