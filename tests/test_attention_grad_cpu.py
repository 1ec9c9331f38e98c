"""The attention backward without a GPU: the ABI carries the new entries and their refusals, the closed-form gradient of
tests/_attention_grad_ref.py agrees with torch-double autograd of the same forward, the un-rotation identity, the reproducible
synthetic matches, the class-weighted BCE against a direct restatement, fixture F26's preconditions, and the training condition of
tests/test_attention_grad.py on the eager double path (its 20-step ratio is measured and pinned here)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native, outlier
from tests import _attention_grad_ref as G
from tests import _lepard_ref as P
from tests import _outlier_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndp_attention_forward_lse", "ndp_attention_backward")
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    return _native.lib()


def test_abi_carries_the_entries(L):
    assert L.ndp_version() >= 217
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    versions = open(os.path.join(_native.CSRC, "ndp_abi_common.inc")).read()
    assert "//   217: " + ", ".join(ENTRIES) in versions
    for entry in ENTRIES:
        assert entry in _native._SIGS and entry in _native.EXPORTS and getattr(L, entry)
        assert f"int {entry}(" in header
    assert list(_native._SIGS)[-2:] == list(ENTRIES)                                   # appended, nothing renumbered


def _buffers():
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    return buf, p, ctypes.c_void_p(p.value + 1)


def _off(*v):
    return (ctypes.c_int * len(v))(*v)


def test_entries_refuse_bad_arguments(L):
    """every refusal is decided before the first HIP call: the device pointers are never read"""
    buf, p, odd = _buffers()

    def fwd(q=p, k=p, v=p, pe_q=None, pe_k=None, pos_q=p, pos_k=p, offQ=p, offK=p, hq=_off(0, 5), hk=_off(0, 7), B=1, C=48, H=4, scale=0.25,
            sigma=0.1, o=p, lse=p, **_):
        return L.ndp_attention_forward_lse(q, k, v, pe_q, pe_k, pos_q, pos_k, offQ, offK, hq, hk, B, C, H, scale, sigma, o, lse, None)

    def bwd(q=p, k=p, v=p, pe_q=None, pe_k=None, pos_q=p, pos_k=p, offQ=p, offK=p, hq=_off(0, 5), hk=_off(0, 7), B=1, C=48, H=4, scale=0.25,
            sigma=0.1, o=p, lse=p, do=p, delta=p, dq=p, dk=p, dv=p):
        return L.ndp_attention_backward(q, k, v, pe_q, pe_k, pos_q, pos_k, o, lse, do, offQ, offK, hq, hk, B, C, H, scale, sigma, delta, dq, dk, dv, None)

    shared = [(dict(pos_q=None), b"both or neither"), (dict(pos_k=None), b"both or neither"), (dict(pos_q=odd), b"aligned"), (dict(pos_k=odd), b"aligned"),
              (dict(sigma=float("nan")), b"sigma_spat"), (dict(sigma=0.0), b"sigma_spat"), (dict(sigma=-0.1), b"sigma_spat"), (dict(sigma=1e-30), b"sigma_spat"),
              (dict(B=0), b"B must"), (dict(B=65536), b"B must"), (dict(hq=None), b"null"), (dict(hk=None), b"null"),
              (dict(hq=_off(0, 0)), b"non-empty"), (dict(hk=_off(3, 3)), b"non-empty"), (dict(hq=_off(-1, 5)), b"start at 0"),
              (dict(hq=_off(0, 5, 3), hk=_off(0, 3, 7), B=2), b"monotone"), (dict(pe_q=p), b"both or neither"), (dict(pe_k=p), b"both or neither"),
              (dict(pe_q=p, pe_k=p, C=66, H=2), b"even head dimension"), (dict(scale=float("nan")), b"scale"), (dict(scale=float("inf")), b"scale")]
    shared += [(dict([(name, None)]), b"null") for name in ("q", "k", "v", "offQ", "offK", "o", "lse")]
    shared += [(dict([(name, odd)]), b"aligned") for name in ("q", "k", "v", "offQ", "offK", "lse")]
    for fn, entry, more in ((fwd, ENTRIES[0], [(dict(o=odd), b"aligned")]),
                            (bwd, ENTRIES[1], [(dict([(name, None)]), b"null") for name in ("do", "delta", "dq", "dk", "dv")] +
                             [(dict([(name, odd)]), b"aligned") for name in ("o", "do", "delta", "dq", "dk", "dv")])):
        for kw, word in shared + more:
            assert fn(**kw) == E_INVALID, (entry, kw)
            assert word in L.ndp_last_error() and entry.encode() in L.ndp_last_error(), (kw, L.ndp_last_error())
        for kw in (dict(C=0), dict(C=1057, H=1), dict(H=0), dict(H=17, C=17 * 6), dict(C=50, H=4), dict(C=265, H=1),
                   dict(hq=_off(0, (1 << 30) + 1)), dict(hk=_off(0, (1 << 30) + 1))):
            assert fn(**kw) == E_UNSUPPORTED, (entry, kw)
            assert b"served are" in L.ndp_last_error()


def test_wrappers_refuse_bad_arguments():
    from deformationpyramid_amd import ops
    q, k = torch.zeros(5, 48), torch.zeros(7, 48)
    lse = torch.zeros(5, 4)
    for a in (dict(o=k), dict(do=k), dict(lse=torch.zeros(5, 3)), dict(lse=None), dict(pos_q=torch.zeros(5, 6)), dict(n_head=5)):
        kw = dict(q=q, k=k, v=k, o=q, lse=lse, do=q, n_head=4)
        kw.update(a)
        with pytest.raises(ValueError):
            ops.attention_bwd(**kw)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.attention_bwd(q, k, k, q, lse, q, 4)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.attention_fn(q.requires_grad_(True), k, k, 4)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.attention(q, k, k, 4, want_lse=True)


# ------------------------------------------------------------------------------------------ the restatement
CASES = [(s[:4], rot) for s in G.GRAD_CASES for rot in ((True, False) if s[4] is None else (s[4],))]


@pytest.mark.parametrize("sigma", [None, G.SIGMA], ids=["plain", "compat"])
def test_closed_form_agrees_with_torch_double_autograd(sigma):
    for shape, rotary in CASES + [((63, 65, 48, 4), True)]:
        c = G.grad_inputs(*shape, rotary) if shape != (63, 65, 48, 4) else G.grad_inputs(*shape, True, seed=7, spread=60.0)
        r64, _ = G.grad_refs(c, sigma)
        T = lambda a: None if a is None else torch.from_numpy(a).double()
        q, k, v = (T(a).requires_grad_(True) for a in (c.q, c.k, c.v))
        o = G.t_attention(q, k, v, c.H, T(c.pe_q), T(c.pe_k), T(c.pos_q), T(c.pos_k), sigma)
        (o * T(c.do)).sum().backward()
        for name, mine, theirs in (("o", r64.o, o.detach()), ("dq", r64.dq, q.grad), ("dk", r64.dk, k.grad), ("dv", r64.dv, v.grad)):
            err, mag = float(np.abs(mine - theirs.numpy()).max()), float(np.abs(mine).max())
            assert err <= 1e-12 * max(mag, 1.0), (shape, rotary, name, err)
        x = P.scores(c.q, c.k, c.H, c.pe_q, c.pe_k, 1.0) * (1.0 if sigma is None else O.compat(c.pos_q, c.pos_k, sigma)[:, :, None]) * (shape[2] // shape[3]) ** -0.5
        assert np.allclose(r64.lse, torch.logsumexp(torch.from_numpy(x), 1).numpy(), rtol=1e-12, atol=1e-12)
        assert np.allclose(r64.p.sum(1), 1.0, atol=1e-12)


def test_cases_have_the_compatibility_spread_asked_of_them():
    zero = total = 0
    for shape, rotary in CASES:
        share, inside = G.zero_share(G.grad_inputs(*shape, rotary))
        m = O.compat(G.grad_inputs(*shape, rotary).pos_q, G.grad_inputs(*shape, rotary).pos_k)
        zero, total = zero + int((m == 0).sum()), total + m.size
        assert inside and (shape[0] * shape[1] < 256 or 0.2 <= share <= 0.8), (shape, share)
    assert 0.2 <= zero / total <= 0.8
    c = G.lonely_row_case()
    m = O.compat(c.pos_q, c.pos_k)
    assert m[3, 3] == 1 and (np.delete(m[3], 3) == 0).all()


def test_unrotation_is_the_transpose_of_the_rotation():
    g = np.random.default_rng(3)
    x, y = g.standard_normal((7, 12)), g.standard_normal((7, 12))
    ang = g.uniform(-3, 3, (7, 6))
    pe = np.stack([np.repeat(np.cos(ang), 2, 1), np.repeat(np.sin(ang), 2, 1)], -1)
    assert abs((P.rotate(x, pe) * y).sum() - (x * G.unrotate(y, pe)).sum()) < 1e-12      # <R x, y> = <x, R^T y>
    assert np.allclose(G.unrotate(P.rotate(x, pe), pe), x, atol=1e-12)                  # a rotation: R^T R = 1
    # the element-wise form the kernels write: dq[2m] = y[2m] cos[2m] + y[2m+1] sin[2m+1], dq[2m+1] = y[2m+1] cos[2m+1] - y[2m] sin[2m]
    pe = g.standard_normal((7, 12, 2))                                                  # any (cos, sin) per channel: the map is linear
    u = G.unrotate(y, pe)
    assert np.allclose(u[:, ::2], y[:, ::2] * pe[:, ::2, 0] + y[:, 1::2] * pe[:, 1::2, 1], atol=1e-15)
    assert np.allclose(u[:, 1::2], y[:, 1::2] * pe[:, 1::2, 0] - y[:, ::2] * pe[:, ::2, 1], atol=1e-15)
    assert abs((P.rotate(x, pe) * y).sum() - (x * u).sum()) < 1e-12


# ------------------------------------------------------------------------------------------ data, loss, modules
def test_synthetic_matches_are_reproducible():
    a, la = outlier.synthetic_matches(64, 32, 3)
    b, lb = outlier.synthetic_matches(64, 32, 3)
    c, _ = outlier.synthetic_matches(64, 32, 4)
    assert torch.equal(a, b) and torch.equal(la, lb) and not torch.equal(a, c)
    assert a.shape == (96, 6) and a.dtype == torch.float32 and la.dtype == torch.bool and int(la.sum()) == 64
    assert not la[:64].all()                                                            # shuffled
    # an inlier's target end is its source end's image; an outlier's is another sample's, far on the scale of sigma_spat
    s, t = a[:, :3].double().numpy(), a[:, 3:].double().numpy()
    cs, sn = np.cos(0.25), np.sin(0.25)
    back = (t - np.array([0.08, -0.03, 0.05])) @ np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1.0]])          # R^T applied to rows
    resid = np.abs(back - s).max(1)                                                     # |phi(s) - s| <= 0.05 on an inlier
    assert (resid[la.numpy()] <= 0.05 + 1e-6).all()
    first = np.asarray([-0.31294382, 0.14079854, -0.02348976, -0.21789624, -0.14365625, -0.02955137], np.float32)
    assert np.abs(a[0].numpy() - first).max() < 1e-6                                    # the same numbers on every machine


def test_synthetic_matches_share_surface_pairs_surface_and_motion():
    """the numpy and the torch evaluation of the shared formulas agree on the same points, and surface_pair still is what it was"""
    from deformationpyramid_amd import synthetic
    g = np.random.default_rng(0)
    d = g.standard_normal((50, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    ph = g.uniform(0, 6.28, 4)
    r_np, r_t = synthetic.surface_radius(d, ph, np), synthetic.surface_radius(torch.from_numpy(d), torch.from_numpy(ph)).numpy()
    assert np.abs(r_np - r_t).max() < 1e-14
    x = d * r_np[:, None]
    assert np.abs(synthetic.surface_deform(x, ph[3], np) - synthetic.surface_deform(torch.from_numpy(x), float(ph[3])).numpy()).max() < 1e-14
    src, tgt, flow, overlap = synthetic.surface_pair(0, n_total=64, partial=False)       # the pair's own motion, from the shared constants
    cs, sn = np.cos(synthetic.SURFACE_ROT_Z), np.sin(synthetic.SURFACE_ROT_Z)
    back = ((src + flow).double().numpy() - np.asarray(synthetic.SURFACE_TRN)) @ np.array([[cs, -sn, 0], [sn, cs, 0], [0, 0, 1.0]])
    assert np.abs(back - src.double().numpy()).max() <= 0.05 + 1e-6                       # |phi(x) - x| <= 0.05
    assert (synthetic.SURFACE_ROT_Z, synthetic.SURFACE_TRN) == (0.25, (0.08, -0.03, 0.05))


def test_weighted_bce_equals_a_direct_restatement():
    g = torch.Generator().manual_seed(0)
    for n_in, n in ((5, 17), (17, 17), (0, 9), (40, 96)):
        conf = torch.rand(n, generator=g, dtype=torch.float64).clamp(1e-6, 1 - 1e-6)
        labels = torch.zeros(n, dtype=torch.float64)
        labels[torch.randperm(n, generator=g)[:n_in]] = 1
        mine, direct = outlier.NeCoLoss.get_weighted_bce_loss(conf, labels), G.weighted_bce(conf, labels)
        assert abs(float(mine) - float(direct)) <= 1e-14 * max(1.0, abs(float(direct)))
        by_hand = sum(((1 - n_in / n) if y else n_in / n) * -(np.log(p) if y else np.log(1 - p)) for p, y in zip(conf.tolist(), labels.tolist())) / n
        assert abs(float(mine) - by_hand) <= 1e-12
    loss = outlier.NeCoLoss({"inlier_thr": 0.04, "mutual_nearest": False, "dataset": "4dmatch", "balanced_bce": True})
    assert loss.inlier_thr == 0.04 and abs(float(loss.get_weighted_bce_loss(conf, labels)) - float(direct)) <= 1e-14


def test_neco_loss_on_the_stacked_layout():
    """two pairs: labels from compute_inlier_mask, the loss of the stacked confidences, both inlier rates"""
    g = np.random.default_rng(0)
    s_pcd = torch.from_numpy(g.uniform(-0.5, 0.5, (11, 3)).astype(np.float32))
    flow = [torch.from_numpy(g.uniform(-0.02, 0.02, (n, 3)).astype(np.float32)) for n in (6, 5)]
    rot, trn = torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3, 1)
    ind = torch.tensor([[0, 0], [1, 1], [2, 2], [3, 3], [0, 0], [1, 1], [4, 4]])
    rows = torch.tensor([0, 1, 2, 3, 6, 7, 10])
    tgt = (s_pcd + torch.cat(flow))[rows]
    tgt[1] += 0.5
    tgt[5] += 0.5                                                                       # two outliers
    conf = torch.tensor([0.9, 0.2, 0.8, 0.4, 0.7, 0.6, 0.3], requires_grad=True)
    data = {"s_pcd": s_pcd, "src_lengths": [6, 5], "coarse_flow": flow, "batched_rot": rot, "batched_trn": trn, "vec_6d": torch.cat([s_pcd[rows], tgt], 1),
            "vec_6d_lengths": [4, 3], "vec_6d_ind": ind, "inlier_conf": conf}
    info = outlier.NeCoLoss({"inlier_thr": 0.04, "mutual_nearest": False, "dataset": "4dmatch", "balanced_bce": True})(data)
    labels = torch.tensor([1, 0, 1, 1, 1, 0, 1.0])
    assert abs(float(info["loss"]) - float(G.weighted_bce(conf.detach(), labels))) < 1e-7 and info["loss"].requires_grad
    assert abs(float(info["IR Lepard"]) - (3 / 4 + 2 / 3) / 2) < 1e-6
    assert abs(float(info["IR NeCo"]) - (2 / 2 + 1 / 2) / 2) < 1e-6                     # kept: rows 0, 2 of pair 0; rows 0, 1 of pair 1


def test_modules_keep_their_inference_contract():
    """forward / confidence stay no_grad wrappers; the new methods exist; the restated network agrees with _outlier_ref's numpy one"""
    cfg = O.config(48, 4)
    torch.manual_seed(1)
    net = outlier.Outlier_Rejection(cfg)
    from deformationpyramid_amd import lepard
    for cls in (outlier.CorrespondenceAttentionLayer, lepard.GeometryAttentionLayer):
        assert callable(cls.forward_grad) and callable(cls._run)
    assert callable(net.confidence_grad) and callable(outlier.train_step)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        net.confidence_grad(torch.zeros(4, 6), [4])
    v6, _ = outlier.synthetic_matches(20, 10, 1)
    sd = {k: v.numpy() for k, v in net.state_dict().items()}
    mine = G.t_network(G.params_of(sd, torch.float64, requires_grad=False), cfg, v6.double(), [30]).numpy()
    assert np.abs(mine - O.network(sd, cfg, v6.numpy())[1]).max() < 1e-12


def test_fixture_f26_preconditions():
    """the reference's own double gradients agree with the restatement's, and no pre-ReLU value lies within 1e-3 of 0"""
    z = G.load_f26()
    for kind in ("outlier", "lepard"):
        f = lambda name: z[f"{kind}.{name}"]
        sd = {k[len(kind) + 4:]: z[k] for k in z.files if k.startswith(f"{kind}.sd.")}
        x, source = f("x"), f("source")
        assert x.shape[0] <= 40 and source.shape[0] <= 40 and x.shape[1] <= 48
        pos = f("vec6d") if kind == "outlier" else None
        g64, out, pre = G.layer_grads(sd, x, source, f("x_pe"), f("source_pe"), f("w"), 4, "rotary", [x.shape[0]], [source.shape[0]], pos, pos,
                                      G.SIGMA if kind == "outlier" else None)
        assert np.abs(pre).min() >= 1e-3 and np.abs(f("pre64")).min() >= 1e-3
        assert np.abs(out - f("out64")).max() < 1e-10
        names = [k[len(kind) + 8:] for k in z.files if k.startswith(f"{kind}.grad64.")]
        assert sorted(names) == sorted(g64)
        for name in names:
            ref = z[f"{kind}.grad64.{name}"]
            assert np.abs(g64[name] - ref).max() <= 1e-10 * max(1.0, np.abs(ref).max()), (kind, name)


# ------------------------------------------------------------------------------------------ the training condition
def test_twenty_eager_double_steps_lower_the_loss():
    """What tests/test_attention_grad.py asks of the float32 paths, on the eager double path: this run fixes G.TRAIN_RATIO_DOUBLE."""
    cfg = O.config(G.TRAIN_CFG["C"], G.TRAIN_CFG["H"], num_layers=G.TRAIN_CFG["num_layers"])
    torch.manual_seed(G.TRAIN_INIT)
    net = G.train_init(outlier.Outlier_Rejection(cfg)).double()
    v6, labels = outlier.synthetic_matches(64, 32, G.TRAIN_SEED)
    losses = G.eager_training(net, cfg, v6.double(), [96], labels, 21)
    ratio = losses[20] / losses[0]
    print(f"eager double: loss {losses[0]:.5f} -> {losses[20]:.5f} after 20 Adam steps, ratio {ratio:.4f}")
    assert ratio < 0.7                                                                  # the seed leaves a margin that means something
    assert abs(ratio - G.TRAIN_RATIO_DOUBLE) < 5e-4                                     # the recorded figure is this run's
    assert losses[20] <= G.TRAIN_BOUND * losses[0]
