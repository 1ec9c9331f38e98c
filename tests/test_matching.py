"""Descriptor matching kernels (csrc/ndp_match.inc) against the float64 restatement of tests/_matching_ref.py.  The project's bar: a
kernel may err by at most the larger of 4 x the error of the eager float32 restatement on the same inputs and 16 float32 ulps of
the logits' magnitude; `conf` is held relatively, to expm1 of the bar on its logarithm.  Argmax and match lists must equal float64's
except where float64 itself is ambiguous (top-two gap below twice the bar, conf within the relative bar of the threshold), and
that such entries are rare is asserted on the reference values before the kernel's output is looked at (in the few named cases where
they are not rare, _matching_ref.float64_leaves_open, `conf` is still held on every row and the lists on what float64 settles).  What is exact in fp32
(lattice logits, the tie rule, batch against single, run against run, rows against columns) is compared bit for bit.  Every
accuracy case prints error / bar before it asserts (profiles/matching_accuracy.txt is that output)."""
import functools
import math

import numpy as np
import pytest
import torch

from deformationpyramid_amd import matching, ops, rigid
from deformationpyramid_amd.synthetic import synthetic_descriptors, synthetic_landmarks, synthetic_pair
from tests import _matching_ref as R
from tests import _rigid_ref as RG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TINY = 1e-37


def dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def bits(t):
    return t.cpu().contiguous().view(torch.int32)


def f32(t):
    """float32 of exact float64 values, a zero as +0 (the kernel's chain starts from +0 and never leaves a -0 behind)."""
    return t.float() + 0.0


def offsets(sizes):
    return [0] + [int(v) for v in np.cumsum(sizes)]


# ------------------------------------------------------------------------------------------ 1. row statistics
@pytest.mark.parametrize("S,T,C", R.ROWSTATS_CASES)
def test_rowstats_against_float64(S, T, C):
    c = R.rowstats_case(S, T, C)
    assert int(c.ambiguous.sum()) <= 0.01 * S                     # on the reference alone
    fs, ft, v = dev(c.fs, c.ft, c.v)
    lse, mx, arg = ops.feat_rowstats(fs, ft, c.alpha, v=v, e=torch.tensor([c.e], device=DEV))
    assert lse.shape == (S,) and mx.dtype == torch.float32 and arg.dtype == torch.int32
    e_lse = float((lse.double().cpu() - c.r64.lse).abs().max())
    e_max = float((mx.double().cpu() - c.r64.max).abs().max())
    print(f"rowstats S={S} T={T} C={C}: lse {e_lse:.3e} max {e_max:.3e} / bar {c.bar:.3e} = {max(e_lse, e_max) / c.bar:.3f}  "
          f"ambiguous rows {int(c.ambiguous.sum())}")
    assert np.isfinite(e_lse) and e_lse <= c.bar and e_max <= c.bar
    arg = arg.long().cpu()
    assert bool(((arg >= 0) & (arg < T)).all())
    assert torch.equal(arg[~c.ambiguous], c.r64.arg[~c.ambiguous])


def test_rowstats_outputs_without_potential_or_dustbin():
    S, T, C = 70, 300, 33
    fs, ft, _ = R.planted_features(S, T, C, 3)
    r64, r32 = R.rowstats_ref(fs, ft, 0.3), R.rowstats_ref(fs, ft, 0.3, dtype=torch.float32)
    b = R.bar(float((r32.lse.double() - r64.lse).abs().max()), float(R.logits(fs, ft, 0.3).abs().max()))
    lse, mx, arg = ops.feat_rowstats(*dev(fs, ft), 0.3)
    assert float((lse.double().cpu() - r64.lse).abs().max()) <= b and float((mx.double().cpu() - r64.max).abs().max()) <= b
    keep = r64.gap >= 2 * b
    assert torch.equal(arg.long().cpu()[keep], r64.arg[keep])


# ------------------------------------------------------------------------------------------ 2. the three modes
def check_mode(tag, mode, fs, ft, match_t, conf, c, S, T, thr=0.1):
    """match_t, conf [S] of the kernel (mutual) for one problem against the float64 case c."""
    r = c.r64
    conf, match_t = conf.double().cpu(), match_t.long().cpu()
    if mode == "mutual_nn":
        err, lim = float((conf - r.conf).abs().max()), c.bar
    else:
        err, lim = float(((conf - r.conf).abs() / (r.conf + TINY)).max()), c.rel
    col_open = c.amb_c[r.arg_r]                                   # the mutual test of row i reads the column of its best target
    settled = ~(c.amb_r | col_open | c.amb_pair)
    print(f"{mode} {tag}: conf {err:.3e} / {lim:.3e} = {err / lim:.3f}  matches {c.n_match}  open rows {int((~settled).sum())}")
    assert np.isfinite(err) and err <= lim
    assert match_t.shape == (S,) and bool(((match_t >= -1) & (match_t < T)).all())
    assert torch.equal(match_t[settled], r.match_t[settled])
    return settled


def run_mode(mode, fs, ft, mutual=True, **kw):
    thr = -math.inf if mode == "mutual_nn" else 0.1
    return ops.feat_match(fs, ft, mode=mode, temperature=1.0 if mode == "mutual_nn" else R.TEMPERATURE, thr=thr, mutual=mutual, **kw)


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("S,T,C", R.MODE_CASES)
def test_modes_against_float64(S, T, C, mode):
    fs, ft = R.mode_features(mode, S, T, C)
    c = R.mode_case(mode, fs, ft)
    # on the reference alone; where float64 cannot name the maxima (_matching_ref.float64_leaves_open says which cases and why) conf
    # is still held on every row and the lists on the entries float64 settles, only the 1 % condition does not hold
    assert R.preconditions(c, S, T) == (not R.float64_leaves_open(mode, S, T, C))
    fsd, ftd = dev(fs, ft)
    match_t, conf = run_mode(mode, fsd, ftd)
    assert match_t.dtype == torch.int32 and conf.dtype == torch.float32
    check_mode(f"S={S} T={T} C={C}", mode, fs, ft, match_t, conf, c, S, T)
    one_way, conf1 = run_mode(mode, fsd, ftd, mutual=False)       # without the mutual test: the row argmax wherever conf > thr
    assert torch.equal(bits(conf1), bits(conf))
    want = R.mode_ref(mode, fs, ft, mutual=False, thr=-math.inf if mode == "mutual_nn" else 0.1).match_t
    keep = ~(c.amb_r | c.amb_pair)
    assert torch.equal(one_way.long().cpu()[keep], want[keep])


@pytest.mark.parametrize("mode", R.MODES)
def test_batch_of_unequal_problems(mode):
    C = 33
    feats = [R.mode_features(mode, S, T, C) for S, T in R.BATCH]
    cases = [R.mode_case(mode, fs, ft) for fs, ft in feats]
    assert all(R.preconditions(c, S, T) for c, (S, T) in zip(cases, R.BATCH))
    fs, ft = dev(torch.cat([f[0] for f in feats]), torch.cat([f[1] for f in feats]))
    os_, ot = offsets([s for s, _ in R.BATCH]), offsets([t for _, t in R.BATCH])
    match_t, conf = run_mode(mode, fs, ft, offsets_s=os_, offsets_t=ot)
    lse, mx, arg = ops.feat_rowstats(fs, ft, 0.3, offsets_a=os_, offsets_b=ot)
    for b, ((S, T), (f_s, f_t), c) in enumerate(zip(R.BATCH, feats, cases)):
        rows = slice(os_[b], os_[b + 1])
        check_mode(f"batch[{b}] S={S} T={T}", mode, f_s, f_t, match_t[rows], conf[rows], c, S, T)
        alone_t, alone_c = run_mode(mode, *dev(f_s, f_t))         # the same problem alone: the same bits
        assert torch.equal(alone_t.cpu(), match_t[rows].cpu()) and torch.equal(bits(alone_c), bits(conf[rows]))
        l1, m1, a1 = ops.feat_rowstats(*dev(f_s, f_t), 0.3)
        assert torch.equal(bits(l1), bits(lse[rows])) and torch.equal(bits(m1), bits(mx[rows])) and torch.equal(a1.cpu(), arg[rows].cpu())


# ------------------------------------------------------------------------------------------ 3. bitwise
@pytest.mark.parametrize("S,T,C", [(127, 129, 1), (300, 257, 3), (127, 129, 33), (300, 257, 528), (31, 65, 1056)])
def test_lattice_logits_are_exact_and_ties_take_the_lowest_index(S, T, C):
    fs, ft = R.lattice_features(S, T, C, S + C, dup=20)
    r = R.rowstats_ref(fs, ft, 0.25)                              # float64 of exact integers / 4: the integer computation
    assert bool((r.gap == 0).any()) and not bool((r.arg >= T - 20).any())
    lse, mx, arg = ops.feat_rowstats(*dev(fs, ft), 0.25)
    assert torch.equal(bits(mx), bits(f32(r.max))) and torch.equal(arg.long().cpu(), r.arg)
    lse2, mx2, arg2 = ops.feat_rowstats(*dev(fs, ft), 0.25)       # run to run
    assert torch.equal(bits(lse), bits(lse2)) and torch.equal(bits(mx), bits(mx2)) and torch.equal(arg.cpu(), arg2.cpu())
    rc = R.rowstats_ref(ft, fs, 0.25)                             # the column statistics: operands exchanged
    _, mxc, argc = ops.feat_rowstats(*dev(ft, fs), 0.25)
    assert torch.equal(bits(mxc), bits(f32(rc.max))) and torch.equal(argc.long().cpu(), rc.arg)
    match_t, conf = ops.feat_match(*dev(fs, ft), mode="mutual_nn", temperature=0.25, thr=-math.inf)
    want = R.match_ref(R.logits(fs, ft, 0.25), -math.inf, exp=False)
    assert torch.equal(match_t.long().cpu(), want.match_t) and torch.equal(bits(conf), bits(f32(want.conf)))


@pytest.mark.parametrize("S,T,C", [(31, 33, 33), (40, 17, 528)])
def test_exchanged_operands_give_the_transposed_statistics_bit_for_bit(S, T, C):
    """Every logit's bits, read through S T problems of one row and one column each, once with the source as rows and once with the
    target as rows: the two must agree, and the statistics of the whole problem must be the maxima of exactly these values."""
    fs, ft, _ = R.planted_features(S, T, C, 17)
    alpha = 1.0 / (C * R.TEMPERATURE)
    fsd, ftd = dev(fs, ft)
    a, b = fsd.repeat_interleave(T, 0).contiguous(), ftd.repeat(S, 1).contiguous()          # pair (i, j) at row i T + j
    one = list(range(S * T + 1))
    z_rows = ops.feat_rowstats(a, b, alpha, offsets_a=one, offsets_b=one)[1]
    z_cols = ops.feat_rowstats(b, a, alpha, offsets_a=one, offsets_b=one)[1]
    assert torch.equal(bits(z_rows), bits(z_cols))
    Z = z_rows.reshape(S, T)
    assert float((Z.double().cpu() - R.logits(fs, ft, alpha)).abs().max()) <= 16 * R.ULP * float(R.logits(fs, ft, alpha).abs().max())
    lse_r, mx_r, arg_r = ops.feat_rowstats(fsd, ftd, alpha)
    lse_c, mx_c, arg_c = ops.feat_rowstats(ftd, fsd, alpha)
    assert torch.equal(bits(mx_r), bits(Z.max(1).values)) and torch.equal(bits(mx_c), bits(Z.max(0).values))
    assert torch.equal(arg_r.long(), (Z == Z.max(1, keepdim=True).values).int().argmax(1))
    assert torch.equal(arg_c.long(), (Z == Z.max(0, keepdim=True).values).int().argmax(0))


# ------------------------------------------------------------------------------------------ 4. the reference's fixture
@pytest.mark.parametrize("case", ["dsm", "skh"])
def test_reference_fixture_through_the_public_functions(golden, case):
    f = golden("F21_matching")
    cfg = f[case + ".config"]
    fs, ft = torch.from_numpy(f[case + ".src_feats"]), torch.from_numpy(f[case + ".tgt_feats"])
    sm, tm = torch.from_numpy(f[case + ".src_mask"]), torch.from_numpy(f[case + ".tgt_mask"])
    conf64 = torch.from_numpy(f[case + ".conf_matrix64"])
    rel = 0.0
    for b in range(fs.shape[0]):                                 # the bar of every problem, from the reference side alone
        s, t = int(sm[b].sum()), int(tm[b].sum())
        mode = "dual_softmax" if case == "dsm" else "sinkhorn"
        full = R.dual_softmax_ref if case == "dsm" else R.sinkhorn_ref
        args = (float(cfg[1]),) if case == "dsm" else (float(cfg[1]), int(cfg[2]))
        l64, l32 = full(fs[b, :s], ft[b, :t], *args), full(fs[b, :s], ft[b, :t], *args, dtype=torch.float32)
        alpha = 1.0 / (fs.shape[2] * (float(cfg[1]) if case == "dsm" else 1.0))
        rel = max(rel, math.expm1(R.bar(float((l32.double() - l64).abs().max()), float(R.logits(fs[b, :s], ft[b, :t], alpha).abs().max()))))
    if case == "dsm":
        index, mconf = matching.dual_softmax_match(fs.to(DEV), ft.to(DEV), float(cfg[1]), float(cfg[0]), src_mask=sm.to(DEV), tgt_mask=tm.to(DEV))
    else:
        index, mconf = matching.sinkhorn_match(fs.to(DEV), ft.to(DEV), float(cfg[1]), int(cfg[2]), float(cfg[0]), src_mask=sm.to(DEV), tgt_mask=tm.to(DEV))
    assert index.dtype == torch.int64 and index.ndim == 2 and index.shape[1] == 3 and mconf.dtype == torch.float32 and mconf.shape == (index.shape[0],)
    want = torch.from_numpy(f[case + ".coarse_match"])
    assert torch.equal(index.cpu(), want)
    ref = conf64[want[:, 0], want[:, 1], want[:, 2]]
    err = float(((mconf.double().cpu() - ref).abs() / ref).max())
    print(f"fixture {case}: {index.shape[0]} matches, conf {err:.3e} / {rel:.3e} = {err / rel:.3f}")
    assert err <= rel


# ------------------------------------------------------------------------------------------ 5. end to end at small size
@functools.lru_cache(maxsize=None)
def planted_pair():
    src, tgt, flow_gt, overlap = synthetic_pair(0)
    ls, lt = synthetic_landmarks(0, src, flow_gt, k=300)
    return synthetic_descriptors(0, ls, lt, impostors=0.3)


def test_landmarks_from_descriptors_feed_the_rigid_filter():
    thr = 0.1                                                     # the pair deforms: its true matches lie within 0.1 of one rigid motion
    ps, pt, fs, ft, perm = planted_pair()
    c = R.mode_case("dual_softmax", fs, ft)
    assert R.preconditions(c, 300, 300) and not bool((c.amb_r | c.amb_c | c.amb_pair).any()) and c.n_match >= 200
    rows = (c.r64.match_t >= 0).nonzero()[:, 0]
    ls64, lt64 = ps[rows].contiguous(), pt[c.r64.match_t[rows]].contiguous()
    tri = rigid.draw_triples(rows.numel(), 4096, 0)
    o = RG.ransac_ref(ls64, lt64, tri, thr)
    assert o.status == 0 and 150 <= o.count <= 0.75 * rows.numel()  # the impostors are out
    # float64 leaves the best hypothesis open among equals and near-equals; every one of them must refine to the same set, with no
    # residual at the threshold: then fp32 decides alike whichever of them it starts from
    for h in (o.h_count >= o.h_count.max() - 2).nonzero()[:, 0].tolist():
        r = RG.refine_ref(o.h_T[h], ls64, lt64, thr, 2)
        d = r.d2.sqrt()
        assert torch.equal(r.mask, o.mask) and not bool(((d > thr * (1 - 1e-3)) & (d < thr * (1 + 1e-3))).any())
    ls, lt = matching.landmarks_from_descriptors(*dev(ps, pt, fs, ft))
    assert torch.equal(ls.cpu(), ls64) and torch.equal(lt.cpu(), lt64)
    mask, Rm, t = rigid.reject_landmarks(ls, lt, thr)
    assert torch.equal(mask.cpu(), o.mask)


def test_ransac_pose_estimation_matches_the_descriptors_itself():
    ps, pt, fs, ft, perm = planted_pair()
    want = R.mode_ref("mutual_nn", fs, ft)
    c = R.mode_case("mutual_nn", fs, ft)
    assert not bool((c.amb_r | c.amb_c).any())
    row_sel, col_sel = matching.mutual_selection(*dev(fs, ft))
    rows = (want.match_t >= 0).nonzero()[:, 0]
    assert row_sel.dtype == torch.int64 and torch.equal(row_sel.cpu(), rows) and torch.equal(col_sel.cpu(), want.match_t[rows])
    explicit = rigid.ransac_pose_estimation(ps.numpy(), pt.numpy(), [row_sel.cpu().numpy(), col_sel.cpu().numpy()], 0.05, max_iteration=4096, seed=2)
    own = rigid.ransac_pose_estimation(ps.numpy(), pt.numpy(), distance_threshold=0.05, max_iteration=4096, seed=2, src_feat=fs.numpy(), tgt_feat=ft.numpy())
    assert own.shape == (4, 4) and np.array_equal(own, explicit) and not np.array_equal(own, np.eye(4))
    wo, w = matching.inlier_ratio_of_features(ps, pt, fs, ft, torch.from_numpy(own[:3, :3]), torch.from_numpy(own[:3, 3]), thr=0.05)
    best = R.mode_ref("mutual_nn", fs, ft, mutual=False).match_t
    moved = ps.double() @ torch.from_numpy(own[:3, :3]).T + torch.from_numpy(own[:3, 3])
    d_wo, d_w = (moved - pt[best].double()).norm(dim=1), (moved[rows] - pt[want.match_t[rows]].double()).norm(dim=1)
    near = lambda d: int(((d - 0.05).abs() < 1e-5).sum())
    assert abs(wo - float((d_wo < 0.05).double().mean())) <= near(d_wo) / 300 + 1e-12
    assert abs(w - float((d_w < 0.05).double().mean())) <= near(d_w) / rows.numel() + 1e-12
