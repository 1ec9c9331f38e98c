"""Plain-torch restatements of what csrc/ndp_match.inc computes (DESIGN.md "Descriptor matching"), on the CPU in float64 -- the
yardstick of tests/test_matching.py -- or in float32 -- the eager arithmetic the kernels' error is measured against.  Unlike the
kernels they write the S x T matrix out.  Nothing here imports the package.  The functions run on the device of their inputs
(tools/matching_bench.py times them on the GPU)."""
import math
from types import SimpleNamespace

import torch

ULP = 2.0 ** -23                                                  # float32 spacing at 1
SHAPES = [(1, 1), (1, 300), (31, 33), (32, 32), (127, 129), (128, 128), (300, 257), (513, 640)]
CS = [1, 3, 32, 33, 528]
BIG = (2049, 1999, 32)
BATCH = [(70, 45), (1, 1), (33, 130)]                             # three unequal problems in one launch, C = 33
TEMPERATURE = 0.1


# ------------------------------------------------------------------------------------------ inputs
def planted_features(S, T, C, seed, noise=0.3):
    """Unit-normalised Gaussian rows, half of the smaller side planted: target row perm_t[k] is source row perm_s[k] plus `noise`
    per component before normalisation.  Scaled by sqrt(C), so that <fs_i, ft_j> / C is the cosine and `temperature` acts on unit
    rows.  -> (fs [S,C], ft [T,C] float32, pairs [K,2] the planted (s, t))."""
    g = torch.Generator().manual_seed(seed)
    fs = torch.randn(S, C, generator=g, dtype=torch.float64)
    ft = torch.randn(T, C, generator=g, dtype=torch.float64)
    K = min(S, T) // 2
    ps, pt = torch.randperm(S, generator=g)[:K], torch.randperm(T, generator=g)[:K]
    ft[pt] = fs[ps] + noise * torch.randn(K, C, generator=g, dtype=torch.float64)
    fs = fs / fs.norm(dim=1, keepdim=True) * math.sqrt(C)
    ft = ft / ft.norm(dim=1, keepdim=True) * math.sqrt(C)
    return fs.float().contiguous(), ft.float().contiguous(), torch.stack([ps, pt], 1)


def lattice_features(S, T, C, seed, dup=0):
    """Integer components in -4 .. 4: every product and partial sum is an exact float32 integer (C * 16 < 2^24), ties are
    everywhere.  dup > 0: the last `dup` target rows repeat the first ones, so every maximum they attain is attained twice."""
    g = torch.Generator().manual_seed(seed)
    fs = torch.randint(-4, 5, (S, C), generator=g).float()
    ft = torch.randint(-4, 5, (T, C), generator=g).float()
    if dup:
        ft[T - dup:] = ft[:dup].clone()
    return fs.contiguous(), ft.contiguous()


# ------------------------------------------------------------------------------------------ restatements
def logits(a, b, alpha, v=None, dtype=torch.float64):
    z = alpha * (a.to(dtype) @ b.to(dtype).T)
    return z if v is None else z + v.to(dtype)[None, :]


def rowstats_ref(a, b, alpha, v=None, e=None, dtype=torch.float64):
    """-> lse [S], max [S], arg [S] (the lowest index that attains max), gap [S] (max minus the runner-up, inf with one column)."""
    z = logits(a, b, alpha, v, dtype)
    zz = z if e is None else torch.cat([z, torch.full((z.shape[0], 1), float(e), dtype=dtype, device=z.device)], 1)
    top = z.topk(min(2, z.shape[1]), dim=1).values
    mx = top[:, 0]
    arg = (z == mx[:, None]).int().argmax(1)
    gap = top[:, 0] - top[:, 1] if z.shape[1] > 1 else torch.full_like(mx, math.inf)
    return SimpleNamespace(lse=torch.logsumexp(zz, 1), max=mx, arg=arg, gap=gap)


def dual_softmax_ref(fs, ft, temperature=TEMPERATURE, dtype=torch.float64):
    """log of matching.py:144-157's conf_matrix on one unpadded problem, [S,T]."""
    s = logits(fs, ft, 1.0 / (fs.shape[1] * temperature), None, dtype)
    return 2 * s - torch.logsumexp(s, 1, keepdim=True) - torch.logsumexp(s, 0, keepdim=True)


def sinkhorn_ref(fs, ft, bin_score=1.0, iters=3, dtype=torch.float64):
    """log of matching.py:159-170's conf_matrix (log_optimal_transport, :6-38) on one unpadded problem, [S,T]."""
    s = logits(fs, ft, 1.0 / fs.shape[1], None, dtype)
    m, n = s.shape
    Z = torch.full((m + 1, n + 1), float(bin_score), dtype=dtype, device=s.device)
    Z[:m, :n] = s
    norm = -math.log(m + n)
    log_mu = torch.full((m + 1,), norm, dtype=dtype, device=s.device)
    log_nu = torch.full((n + 1,), norm, dtype=dtype, device=s.device)
    log_mu[m] = math.log(n) + norm
    log_nu[n] = math.log(m) + norm
    u, v = torch.zeros_like(log_mu), torch.zeros_like(log_nu)
    for _ in range(iters):
        u = log_mu - torch.logsumexp(Z + v[None, :], 1)
        v = log_nu - torch.logsumexp(Z + u[:, None], 0)
    return (Z + u[:, None] + v[None, :] - norm)[:m, :n]


def match_ref(logc, thr, mutual=True, exp=True):
    """The kernels' rule on a [S,T] matrix of (log) confidences: row i matches its lowest-index best column j iff conf > thr and
    (mutual) i is the lowest-index best row of column j.  -> match_t [S] (-1: none), conf [S] of the best column, and the top-two
    gaps of every row and column (the quantity whose argmax is taken)."""
    top_r = logc.topk(min(2, logc.shape[1]), dim=1).values
    top_c = logc.topk(min(2, logc.shape[0]), dim=0).values
    arg_r = (logc == top_r[:, :1]).int().argmax(1)
    arg_c = (logc == top_c[:1, :]).int().argmax(0)
    best = top_r[:, 0]
    conf = best.exp() if exp else best
    ok = conf > thr
    if mutual:
        ok = ok & (arg_c[arg_r] == torch.arange(logc.shape[0], device=logc.device))
    inf = torch.full_like(best, math.inf)
    gap_r = top_r[:, 0] - top_r[:, 1] if logc.shape[1] > 1 else inf
    gap_c = top_c[0] - top_c[1] if logc.shape[0] > 1 else torch.full_like(top_c[0], math.inf)
    return SimpleNamespace(match_t=torch.where(ok, arg_r, torch.full_like(arg_r, -1)), conf=conf, logc=best, arg_r=arg_r, arg_c=arg_c,
                           gap_r=gap_r, gap_c=gap_c)


def mode_ref(mode, fs, ft, dtype=torch.float64, temperature=TEMPERATURE, bin_score=1.0, iters=3, thr=0.1, mutual=True):
    if mode == "dual_softmax":
        return match_ref(dual_softmax_ref(fs, ft, temperature, dtype), thr, mutual)
    if mode == "sinkhorn":
        return match_ref(sinkhorn_ref(fs, ft, bin_score, iters, dtype), thr, mutual)
    return match_ref(logits(fs, ft, 1.0, None, dtype), -math.inf, mutual, exp=False)


# ------------------------------------------------------------------------------------------ the bar
def bar(err32, magnitude):
    """The project's bar: the larger of 4 x the error of the eager float32 restatement on the same inputs and 16 float32 ulps of the
    logits' magnitude."""
    return max(4.0 * float(err32), 16.0 * ULP * float(magnitude))


# ------------------------------------------------------------------------------------------ the cases of tests/test_matching.py
ROWSTATS_CASES = [(S, T, C) for C in CS for S, T in SHAPES] + [BIG]
MODES = ("dual_softmax", "sinkhorn", "mutual_nn")
# every mode at every named C and (S, T), and the large case
MODE_CASES = [(S, T, C) for C in CS for S, T in SHAPES] + [BIG]


def float64_leaves_open(mode, S, T, C):
    """The mode cases in which float64 itself cannot say which index is the maximum, so `preconditions` fails on the reference
    alone (tests/test_matching_cpu.py asserts that it fails for exactly these and holds for all others):
      C = 1 with more than one source row: unit rows of length 1 are +-1, every logit is +-1 / temperature, and every row and
        every column attains its maximum many times over -- all S + T top-two gaps are exactly 0;
      dual_softmax at (31, 33, 528): one row's top-two gap is below twice the bar, and one row is more than 1 % of 31 + 33.
    In these cases `conf` (a value, not an index) is still held to the bar on every row, and the match list is compared on the
    entries float64 does settle (none at C = 1, 30 of 31 rows in the other case); only the 1 % condition is not asserted."""
    return (C == 1 and S > 1) or (mode, S, T, C) == ("dual_softmax", 31, 33, 528)


def seed_of(S, T, C):
    return 1000003 * S + 1009 * T + C


def mode_features(mode, S, T, C):
    """The planted features of a mode case.  Sinkhorn has no temperature, so its rows are scaled to length sqrt(C / temperature):
    its scores <fs_i, ft_j> / C are then the cosines over `temperature`, the logits the other two modes see."""
    fs, ft, _ = planted_features(S, T, C, seed_of(S, T, C))
    k = math.sqrt(1.0 / TEMPERATURE) if mode == "sinkhorn" else 1.0
    return (fs * k).contiguous(), (ft * k).contiguous()


def rowstats_case(S, T, C):
    """Inputs and float64 / float32 results of one row-statistics case: planted features, alpha = 1 / (C temperature), a potential
    uniform in +-1 and a dustbin value 0.5.  ambiguous [S]: rows whose float64 top-two gap is below twice the bar."""
    fs, ft, _ = planted_features(S, T, C, seed_of(S, T, C))
    g = torch.Generator().manual_seed(seed_of(S, T, C) + 1)
    v = (torch.rand(T, generator=g) * 2 - 1).contiguous()
    e, alpha = 0.5, 1.0 / (C * TEMPERATURE)
    r64 = rowstats_ref(fs, ft, alpha, v, e, torch.float64)
    r32 = rowstats_ref(fs, ft, alpha, v, e, torch.float32)
    mag = max(float(logits(fs, ft, alpha, v).abs().max()), abs(e))          # the dustbin column is a logit as well
    b = bar(max(float((r32.lse.double() - r64.lse).abs().max()), float((r32.max.double() - r64.max).abs().max())), mag)
    return SimpleNamespace(fs=fs, ft=ft, v=v, e=e, alpha=alpha, r64=r64, bar=b, ambiguous=r64.gap < 2 * b)


def mode_case(mode, fs, ft, thr=0.1):
    """float64 result of one mode on one problem with its bar and what float64 itself leaves open: ambiguous rows / columns (top-two
    gap of the maximised quantity below twice the bar) and ambiguous pairs (conf within the relative bar, expm1(bar) on its
    logarithm, of the threshold).  The bar's float32 error is that of the eager restatement's whole matrix."""
    kw = dict(thr=thr)
    full = {"dual_softmax": dual_softmax_ref, "sinkhorn": sinkhorn_ref}.get(mode)
    if full is None:
        l64, l32 = logits(fs, ft, 1.0), logits(fs, ft, 1.0, None, torch.float32)
        alpha = 1.0
    else:
        l64, l32 = full(fs, ft), full(fs, ft, dtype=torch.float32)
        alpha = 1.0 / (fs.shape[1] * (TEMPERATURE if mode == "dual_softmax" else 1.0))
    mag = float(logits(fs, ft, alpha).abs().max())
    b = bar(float((l32.double() - l64).abs().max()), mag)
    r64 = mode_ref(mode, fs, ft, **kw)
    amb_r, amb_c = r64.gap_r < 2 * b, r64.gap_c < 2 * b
    rel = math.expm1(b)
    amb_pair = ((r64.conf / thr - 1).abs() <= rel) if mode != "mutual_nn" else torch.zeros_like(amb_r)
    return SimpleNamespace(r64=r64, bar=b, rel=rel, amb_r=amb_r, amb_c=amb_c, amb_pair=amb_pair, n_match=int((r64.match_t >= 0).sum()))


def preconditions(c, S, T):
    """The condition under which a mode case may be asserted: float64 leaves at most 1 % of the rows plus columns and at most 1 % of
    its matches open."""
    return int(c.amb_r.sum()) + int(c.amb_c.sum()) <= 0.01 * (S + T) and int((c.amb_pair & (c.r64.arg_r >= 0)).sum()) <= 0.01 * max(c.n_match, 1)
