"""The compatibility-modulated ops.attention (csrc/ndp_attention.inc, ndp_attention_compat_forward) and deformationpyramid_amd/outlier.py
on the GPU against the numpy restatement of tests/_outlier_ref.py: float64 at the project's bar -- max(4 x the float32 restatement's
error, 16 float32 ulps of the largest magnitude) --, bit-for-bit where the arithmetic promises it, and the reference's own numbers
(fixture F25).  Every accuracy case prints error / bar before it asserts (profiles/outlier_accuracy.txt is that output).  The
fixture's preconditions are asserted in tests/test_outlier_cpu.py."""
import numpy as np
import pytest
import torch

from deformationpyramid_amd import lepard, ops, outlier
from tests import _kpconv_ref as R
from tests import _kpfcn_ref as K
from tests import _lepard_ref as P
from tests import _outlier_ref as O

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def check(what, got, ref64, ref32):
    got, ref64 = np.asarray(got), np.asarray(ref64)
    err, err32, mag = float(np.abs(got - ref64).max()), float(np.abs(np.asarray(ref32).astype(np.float64) - ref64).max()), float(np.abs(ref64).max())
    bar = R.bar(err32, mag)
    print(f"{what}: error {err:.3e}  bar {bar:.3e}  (eager float32 {err32:.3e}, magnitude {mag:.3e})  error / bar {err / bar:.3f}")
    assert got.shape == ref64.shape and np.isfinite(got).all()
    assert err <= bar


def run(c, rows=None, sigma=O.SIGMA, **kw):
    q, pe_q, pos_q = (c.q, c.pe_q, c.pos_q) if rows is None else (c.q[rows], None if c.pe_q is None else c.pe_q[rows], c.pos_q[rows])
    return ops.attention(dev(q), dev(c.k), dev(c.v), c.H, dev(pe_q), dev(c.pe_k), pos_q=dev(pos_q), pos_k=dev(c.pos_k), sigma_spat=sigma, **kw).cpu().numpy()


def plain(c):
    return ops.attention(dev(c.q), dev(c.k), dev(c.v), c.H, dev(c.pe_q), dev(c.pe_k)).cpu().numpy()


# ------------------------------------------------------------------------------------------ against float64
@pytest.mark.parametrize("rotary", [True, False], ids=["rotary", "nocode"])
@pytest.mark.parametrize("shape", O.COMPAT_SHAPES, ids=lambda s: "x".join(str(int(v)) for v in s))
def test_compat_attention_against_float64(shape, rotary):
    c = O.compat_inputs(*shape, rotary)
    if min(shape[:2]) >= 15:
        assert 0.1 <= O.positive_share(c) <= 0.9                                   # c is both positive and exactly zero in the problem
    check(f"compat attention {shape} {'rotary' if rotary else 'no code'}", run(c), *O.compat_refs(c))


def test_compat_attention_batched_call():
    cs = [O.compat_inputs(L, S, 48, 4, True) for L, S in O.COMPAT_BATCH]
    cat = lambda name: dev(np.concatenate([getattr(c, name) for c in cs]))
    offq, offk = R.offsets([c.q.shape[0] for c in cs]).tolist(), R.offsets([c.k.shape[0] for c in cs]).tolist()
    got = ops.attention(cat("q"), cat("k"), cat("v"), 4, cat("pe_q"), cat("pe_k"), offsets_q=offq, offsets_k=offk, pos_q=cat("pos_q"),
                        pos_k=cat("pos_k"), sigma_spat=O.SIGMA).cpu().numpy()
    for b, c in enumerate(cs):
        mine = got[offq[b]:offq[b + 1]]
        check(f"compat attention batched problem {b} {O.COMPAT_BATCH[b]}", mine, *O.compat_refs(c))
        assert np.array_equal(mine, run(c))                                        # the bits of the same problem alone


def test_compat_attention_wide_logits():
    """modulated, scaled scores spread over +-200: the running maximum keeps every term in (0, 1]"""
    c = O.compat_inputs(63, 65, 48, 4, True, seed=7, spread=60.0)
    a = P.scores(c.q, c.k, c.H, c.pe_q, c.pe_k) * O.compat(c.pos_q, c.pos_k)[:, :, None]
    assert a.max() > 200 and a.min() < -200
    check("compat attention (63, 65, 48, 4) logits over +-200", run(c), *O.compat_refs(c))


def test_compat_attention_non_contiguous_inputs():
    c = O.compat_inputs(63, 65, 48, 4, True)
    wide = lambda a: torch.stack([dev(a), torch.zeros_like(dev(a))], -1)[..., 0]
    q, k, v, pos_q, pos_k = wide(c.q), wide(c.k), wide(c.v), wide(c.pos_q), wide(c.pos_k)
    assert not q.is_contiguous() and not pos_q.is_contiguous() and not pos_k.is_contiguous()
    got = ops.attention(q, k, v, 4, dev(c.pe_q), dev(c.pe_k), pos_q=pos_q, pos_k=pos_k, sigma_spat=O.SIGMA).cpu().numpy()
    check("compat attention (63, 65, 48, 4) strided q, k, v, pos", got, *O.compat_refs(c))
    assert np.array_equal(got, run(c))


# ------------------------------------------------------------------------------------------ bit for bit
@pytest.mark.parametrize("shape", [(63, 65, 48, 4), (65, 129, 72, 4)], ids=["vector", "scalar"])
def test_infinite_sigma_is_the_plain_attention(shape):
    c = O.compat_inputs(*shape, True)
    assert np.array_equal(run(c, sigma=float("inf")), plain(c))


@pytest.mark.parametrize("shape", [(63, 65, 48, 4), (65, 129, 72, 4)], ids=["vector", "scalar"])
def test_a_translated_lattice_is_the_plain_attention(shape):
    """positions on a lattice with t = s + an integer translation: both differences are the same exact numbers, so c == 1 exactly"""
    c = O.compat_inputs(*shape, True)
    n = max(shape[:2])
    s = R.lattice_cloud(n, 5).astype(np.float32)
    pos = np.concatenate([s, s + np.array([3.0, -2.0, 1.0], np.float32)], 1)
    assert np.array_equal(pos[:, 3:] - pos[:, :3], np.broadcast_to(np.array([3.0, -2.0, 1.0], np.float32), (n, 3)))
    assert (O.compat(pos, pos, dtype=np.float32) == 1).all()
    got = ops.attention(dev(c.q), dev(c.k), dev(c.v), c.H, dev(c.pe_q), dev(c.pe_k), pos_q=dev(pos[:shape[0]]), pos_k=dev(pos[:shape[1]]),
                        sigma_spat=O.SIGMA).cpu().numpy()
    assert np.array_equal(got, plain(c))


def test_zero_compatibility_scores_zero_not_minus_infinity():
    """sources pairwise further than sigma apart, all targets equal: c = 1 on the diagonal and 0 off it; a c = 0 key takes part in the
    soft-max with score 0"""
    n = 70
    c = O.compat_inputs(n, n, 48, 4, True)
    g = np.random.default_rng(11)
    cells = g.permutation(6 ** 3)[:n]
    s = 0.5 * np.stack([cells // 36, (cells // 6) % 6, cells % 6], 1).astype(np.float32)
    pos = np.concatenate([s, np.full((n, 3), 0.25, np.float32)], 1)
    assert np.array_equal(O.compat(pos, pos, dtype=np.float32), np.eye(n, dtype=np.float32))
    z = SimpleCase(c, pos)
    got = run(z)
    assert np.isfinite(got).all()
    check("compat attention (70, 70, 48, 4) c = identity", got, *O.compat_refs(z))
    # the maths of it: every off-diagonal key weighs exp(0 - max), so no row is its own value row alone
    assert not np.array_equal(got, c.v)


class SimpleCase:
    """an attention case with other positions"""

    def __init__(self, c, pos):
        self.q, self.k, self.v, self.pe_q, self.pe_k, self.H = c.q, c.k, c.v, c.pe_q, c.pe_k, c.H
        self.pos_q, self.pos_k = pos[:c.q.shape[0]].copy(), pos[:c.k.shape[0]].copy()


def test_rows_do_not_depend_on_the_other_queries():
    c = O.compat_inputs(129, 65, 144, 8, True)
    assert np.array_equal(run(c)[10:21], run(c, rows=slice(10, 21)))


def test_same_call_same_bits():
    c = O.compat_inputs(65, 129, 144, 8, True)
    assert np.array_equal(run(c), run(c))


# ------------------------------------------------------------------------------------------ modules against fixture F25
@pytest.fixture(scope="module")
def f25():
    return O.load_f25()


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.mark.parametrize("variant", O.F25_LAYER_VARIANTS)
def test_correspondence_attention_layer(f25, variant):
    p = f"a.{variant}."
    cfg, sd = O.config(48, 4, variant), P.sub_dict(f25, p + "sd.")
    layer = outlier.CorrespondenceAttentionLayer(cfg)
    layer.load_state_dict(tensors(sd), strict=True)
    layer = layer.to(DEV)
    lens = f25[p + "lens"].tolist()
    stack = lambda key: dev(np.concatenate([f25[p + key][b, :n] for b, n in enumerate(lens)]))
    x, s, v6 = stack("x"), stack("source"), stack("vec6d")
    pe = outlier.VolumetricPositionEncoding(cfg)(v6)
    got = lepard.pad(layer(x, s, pe, pe, lens, lens, v6, v6), lens).cpu().numpy()
    for b, n in enumerate(lens):
        outs = []
        for dt in (np.float64, np.float32):
            code = None if variant == "none" else O.position_code(f25[p + "vec6d"][b, :n], 48, variant, dtype=dt)
            outs.append(O.layer(sd, "", f25[p + "x"][b, :n], f25[p + "source"][b, :n], code, code, 4, variant, f25[p + "vec6d"][b, :n],
                                f25[p + "vec6d"][b, :n], O.SIGMA, dt))
        check(f"layer {variant} problem {b} against float64", got[b, :n], *outs)
        check(f"layer {variant} problem {b} against the reference's double", got[b, :n], f25[p + "out64"][b, :n], outs[1] + (f25[p + "out64"][b, :n] - outs[0]))
        check(f"layer {variant} problem {b} against the reference's float32", got[b, :n], f25[p + "out"][b, :n].astype(np.float64), outs[1] + (f25[p + "out"][b, :n] - outs[0]))
    # with the check off the layer is the plain attention layer: lepard's, on the same weights
    off = outlier.CorrespondenceAttentionLayer(O.config(48, 4, variant, check=False))
    off.load_state_dict(tensors(sd), strict=True)
    if variant != "none":
        twin = lepard.GeometryAttentionLayer(P.transformer_config(48, 4, variant))
        twin.load_state_dict(tensors(sd), strict=True)
        assert torch.equal(off.to(DEV)(x, s, pe, pe, lens, lens), twin.to(DEV)(x, s, pe, pe, lens, lens))


def _net_data(f25, name):
    n, p = O.F25_POINTS, name + "."
    B = len(O.F25_NETS[name]["lens"])
    return {"s_pcd": dev(f25[p + "s_pcd"].reshape(-1, 3)), "t_pcd": dev(f25[p + "t_pcd"].reshape(-1, 3)), "src_lengths": [n] * B,
            "tgt_lengths": [n] * B, "coarse_match_pred": dev(f25[p + "match"].astype(np.int64))}


@pytest.mark.parametrize("name", list(O.F25_NETS))
def test_outlier_rejection_network(f25, name):
    p = name + "."
    net = outlier.Outlier_Rejection(O.net_config(name))
    net.load_state_dict(tensors(P.sub_dict(f25, p + "sd.")), strict=True)
    net = net.to(DEV).eval()
    data = _net_data(f25, name)
    conf, lens = net(data)
    assert lens == O.F25_NETS[name]["lens"] and tuple(conf.shape) == (sum(lens),) and conf.data_ptr() == data["inlier_conf"].data_ptr()
    conf = conf.cpu().numpy()
    r64, r32 = O.run_net(f25, name, np.float64), O.run_net(f25, name, np.float32)
    off = R.offsets(lens).tolist()
    for b, n in enumerate(lens):
        mine, c64, c32 = conf[off[b]:off[b + 1]], r64[b][1], r32[b][1]
        check(f"({name}) pair {b} confidence against float64", mine, c64, c32)
        check(f"({name}) pair {b} confidence against the reference's double", mine, f25[p + "conf64"][b, :n], c32 + (f25[p + "conf64"][b, :n] - c64))
        check(f"({name}) pair {b} confidence against the reference's float32", mine, f25[p + "conf"][b, :n].astype(np.float64), c32 + (f25[p + "conf"][b, :n] - c64))
        assert np.array_equal(np.flatnonzero(mine > O.F25_THR), np.flatnonzero(c64 > O.F25_THR))          # no row is left out
        alone = net.confidence(data["vec_6d"][off[b]:off[b + 1]], [n]).cpu().numpy()
        assert np.array_equal(alone, mine)                                         # a pair's bits do not depend on the batch
    # a pair without matches between the two: left out of the call, the others' bits unchanged
    m = data["coarse_match_pred"].clone()
    m[m[:, 0] == 1, 0] = 2
    wide = dict(_net_data(f25, name), coarse_match_pred=m)
    for key in ("s_pcd", "t_pcd"):
        wide[key] = torch.cat([wide[key], wide[key][:O.F25_POINTS]])
    wide["src_lengths"], wide["tgt_lengths"] = [O.F25_POINTS] * 3, [O.F25_POINTS] * 3
    wide["s_pcd"][2 * O.F25_POINTS:], wide["t_pcd"][2 * O.F25_POINTS:] = data["s_pcd"][O.F25_POINTS:], data["t_pcd"][O.F25_POINTS:]
    conf3, lens3 = net(wide)
    assert lens3 == [lens[0], 0, lens[1]] and np.array_equal(conf3.cpu().numpy(), conf)


def test_compute_inlier_mask(f25):
    data = _net_data(f25, "b")
    _, lens = outlier.Outlier_Rejection._3D_to_6D(data)
    masks, rates = outlier.compute_inlier_mask(data, O.F25_INLIER_THR, dev(f25["c.flow"].reshape(-1, 3)), dev(f25["c.rot"]), dev(f25["c.trn"]))
    for b, n in enumerate(lens):
        assert np.array_equal(masks[b].cpu().numpy(), f25["c.mask"][b, :n])
        assert abs(float(rates[b]) - float(f25["c.rate"][b])) < 1e-6


# ------------------------------------------------------------------------------------------ end to end
@pytest.fixture(scope="module")
def default_net():
    torch.manual_seed(216)
    return outlier.Outlier_Rejection(outlier.DEFAULT_CONFIG).to(DEV).eval()


def test_landmark_model_inference(default_net):
    f24 = P.load_f24()
    batch, z23 = K.load_f23()
    sd = {"backbone." + k: v for k, v in K.state_dict(z23, "c.sd.").items()}
    sd.update(P.sub_dict(f24, "c.sd."))
    pipe = lepard.Pipeline(P.pipeline_config())
    pipe.load_state_dict(tensors(sd), strict=True)
    pipe = pipe.to(DEV).eval()
    n0 = int(batch["stack_lengths"][0][0])
    pts = dev(batch["points"][0])
    src, tgt = pts[:n0], pts[n0:]
    ldmk_s, ldmk_t, _, _, _ = lepard.predict_landmarks(pipe, src, tgt, R.PYRAMID_LIMITS)
    K_ = ldmk_s.shape[0]
    assert K_ == f24["c.match"].shape[0] and K_ > 4
    model = outlier.LandmarkModel(pipe, default_net)
    ls, lt, conf = model.inference(src, tgt, R.PYRAMID_LIMITS, reject_outliers=False)
    assert torch.equal(ls, ldmk_s) and torch.equal(lt, ldmk_t) and tuple(conf.shape) == (K_,)
    assert bool(((conf > 0) & (conf < 1)).all())
    thr = float(conf.sort().values[K_ // 2 - 1] + conf.sort().values[K_ // 2]) / 2       # a threshold that a seeded model's confidences straddle
    keep = conf > thr
    assert 0 < int(keep.sum()) < K_
    fs, ft, fc = model.inference(src, tgt, R.PYRAMID_LIMITS, reject_outliers=True, inlier_thr=thr)
    assert torch.equal(fs, ldmk_s[keep]) and torch.equal(ft, ldmk_t[keep]) and torch.equal(fc, conf[keep])
    # with the ground truth the two inlier rates are appended: identity flow and pose, every match within thr = 10 m
    res = model.inference(src, tgt, R.PYRAMID_LIMITS, reject_outliers=False, inlier_thr=10.0, coarse_flow=torch.zeros(69, 3, device=DEV),
                          rot=torch.eye(3, device=DEV), trn=torch.zeros(3, device=DEV))
    assert len(res) == 5 and float(res[3]) == 1.0


def test_reject_landmarks(default_net):
    v6 = O.matches(300, 99)
    keep, conf = outlier.reject_landmarks(default_net, torch.from_numpy(v6[:, :3]), torch.from_numpy(v6[:, 3:]), thr=0.5)
    assert tuple(keep.shape) == tuple(conf.shape) == (300,) and keep.dtype == torch.bool and keep.device.type == "cuda"
    assert bool(torch.isfinite(conf).all()) and bool(((conf >= 0) & (conf <= 1)).all())
    assert torch.equal(keep, conf > 0.5)
    keep2, conf2 = outlier.reject_landmarks(default_net, dev(v6[:, :3]), dev(v6[:, 3:]), thr=float(conf.median()))
    assert torch.equal(conf2, conf) and 0 < int(keep2.sum()) < 300
