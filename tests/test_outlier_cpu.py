"""The compatibility-modulated attention entry and deformationpyramid_amd/outlier.py without a GPU: the ABI carries the entry, every
refusal that needs no device, the numpy restatement (tests/_outlier_ref.py) against the reference's own modules (fixture F25), the
fixture's preconditions, the module-level refusals, the strict state-dict load and the empty-match handling."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native
from tests import _kpconv_ref as R
from tests import _lepard_ref as P
from tests import _outlier_ref as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "ndp_attention_compat_forward"
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    return _native.lib()


@pytest.fixture(scope="module")
def f25():
    return O.load_f25()


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


def test_abi_carries_the_entry(L):
    assert L.ndp_version() >= 216
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    assert ENTRY in _native._SIGS and ENTRY in _native.EXPORTS and getattr(L, ENTRY)
    assert f"int {ENTRY}(" in header
    versions = open(os.path.join(_native.CSRC, "ndp_abi_common.inc")).read()
    assert f"//   216: {ENTRY}" in versions
    assert len(_native._SIGS[ENTRY]) == len(_native._SIGS["ndp_attention_forward"]) + 3          # pos_q, pos_k, sigma_spat


def _buffers():
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    return buf, p, ctypes.c_void_p(p.value + 1)


def _off(*v):
    return (ctypes.c_int * len(v))(*v)


def test_entry_refuses_bad_arguments(L):
    """every refusal is decided before the first HIP call: the device pointers are never read"""
    buf, p, odd = _buffers()

    def fwd(q=p, k=p, v=p, pe_q=None, pe_k=None, pos_q=p, pos_k=p, offQ=p, offK=p, hq=_off(0, 5), hk=_off(0, 7), B=1, C=48, H=4, scale=0.25,
            sigma=0.1, o=p):
        return L.ndp_attention_compat_forward(q, k, v, pe_q, pe_k, pos_q, pos_k, offQ, offK, hq, hk, B, C, H, scale, sigma, o, None)

    invalid = [(dict(pos_q=None), b"null"), (dict(pos_k=None), b"null"), (dict(pos_q=None, pos_k=None), b"null"), (dict(pos_q=odd), b"aligned"),
               (dict(pos_k=odd), b"aligned"), (dict(sigma=float("nan")), b"sigma_spat"), (dict(sigma=0.0), b"sigma_spat"),
               (dict(sigma=-0.1), b"sigma_spat"), (dict(sigma=float("-inf")), b"sigma_spat"), (dict(sigma=1e-30), b"sigma_spat")]
    # everything ndp_attention_forward refuses
    invalid += [(dict(B=0), b"B must"), (dict(B=65536), b"B must"), (dict(hq=None), b"null"), (dict(hk=None), b"null"),
                (dict(hq=_off(0, 0)), b"non-empty"), (dict(hk=_off(3, 3)), b"non-empty"), (dict(hq=_off(-1, 5)), b"start at 0"),
                (dict(hq=_off(0, 5, 3), hk=_off(0, 3, 7), B=2), b"monotone"), (dict(pe_q=p), b"both or neither"), (dict(pe_k=p), b"both or neither"),
                (dict(pe_q=p, pe_k=p, C=66, H=2), b"even head dimension"), (dict(pe_q=p, pe_k=p, C=33, H=1), b"even head dimension"),
                (dict(scale=float("nan")), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("-inf")), b"scale")]
    invalid += [(dict([(name, None)]), b"null") for name in ("q", "k", "v", "offQ", "offK", "o")]
    invalid += [(dict([(name, odd)]), b"aligned") for name in ("q", "k", "v", "offQ", "offK", "o")]
    invalid += [(dict(pe_q=odd, pe_k=p), b"aligned"), (dict(pe_q=p, pe_k=odd), b"aligned")]
    for kw, word in invalid:
        assert fwd(**kw) == E_INVALID, kw
        assert word in L.ndp_last_error() and ENTRY.encode() in L.ndp_last_error(), (kw, L.ndp_last_error())
    for kw in (dict(C=0), dict(C=1057, H=1), dict(H=0), dict(H=17, C=17 * 6), dict(C=50, H=4), dict(C=265, H=1), dict(C=1060, H=4),
               dict(hq=_off(0, (1 << 30) + 1)), dict(hk=_off(0, (1 << 30) + 1))):
        assert fwd(**kw) == E_UNSUPPORTED, kw
        assert b"served are" in L.ndp_last_error()


def test_wrapper_refuses_bad_arguments():
    from deformationpyramid_amd import ops
    q, k = torch.zeros(5, 48), torch.zeros(7, 48)
    pos_q, pos_k = torch.zeros(5, 6), torch.zeros(7, 6)
    for a in (dict(pos_k=None), dict(pos_q=None), dict(sigma_spat=None), dict(pos_q=None, pos_k=None), dict(pos_q=pos_q[:4]), dict(pos_k=pos_k[:, :3]),
              dict(pos_q=pos_k), dict(sigma_spat=0.0), dict(sigma_spat=-1.0), dict(sigma_spat=float("nan")), dict(pos_q=[[0.0] * 6] * 5)):
        kw = dict(q=q, k=k, v=k, n_head=4, pos_q=pos_q, pos_k=pos_k, sigma_spat=0.1)
        kw.update(a)
        with pytest.raises(ValueError):
            ops.attention(**kw)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.attention(q, k, k, 4, pos_q=pos_q, pos_k=pos_k, sigma_spat=0.1)


# ------------------------------------------------------------------------------------------ the restatement against fixture F25
def _report(what, got, ref64, ref32):
    err, err32, mag = float(np.abs(got - ref64).max()), float(np.abs(ref32.astype(np.float64) - ref64).max()), float(np.abs(ref64).max())
    bar = R.bar(err32, mag)
    print(f"{what}: error {err:.3e}  eager float32 {err32:.3e}  magnitude {mag:.3e}  bar {bar:.3e}")
    return err, bar


def test_fixture_is_small(f25):
    assert os.path.getsize(O.F25) <= 900 * 1024
    assert all(f25[k].dtype.kind in "fiub" for k in f25.files)                     # numbers only


@pytest.mark.parametrize("variant", O.F25_LAYER_VARIANTS)
def test_restatement_reproduces_the_reference_layer(f25, variant):
    p = f"a.{variant}."
    sd = P.sub_dict(f25, p + "sd.")
    for b, n in enumerate(f25[p + "lens"].tolist()):
        v6 = f25[p + "vec6d"][b, :n]
        share = float((O.compat(v6, v6) > 0).mean())
        assert 0.1 <= share <= 0.9 and abs(share - float(f25[p + "positive_share"][b])) < 1e-12
        assert (O.compat(v6, v6) == 0).any() and (np.diag(O.compat(v6, v6)) == 1).all()
        outs = []
        for dt in (np.float64, np.float32):
            pe = None if variant == "none" else O.position_code(v6, 48, variant, dtype=dt)
            outs.append(O.layer(sd, "", f25[p + "x"][b, :n], f25[p + "source"][b, :n], pe, pe, 4, variant, v6, v6, O.SIGMA, dt))
        assert float(np.abs(outs[0] - f25[p + "out64"][b, :n]).max()) <= 1e-9 * float(np.abs(outs[0]).max())      # double against the reference in double
        err, bar = _report(f"F25 (a) {variant} problem {b}", f25[p + "out"][b, :n], *outs)
        assert err <= bar


@pytest.mark.parametrize("name", list(O.F25_NETS))
def test_fixture_preconditions_and_the_reference_network(f25, name):
    ok, why = O.net_preconditions(f25, name)
    assert ok, why
    p = name + "."
    r64, r32 = O.run_net(f25, name, np.float64), O.run_net(f25, name, np.float32)
    for b, n in enumerate(O.F25_NETS[name]["lens"]):
        c64, c32 = r64[b][1], r32[b][1]
        assert len(c64) == n                                                       # no row is left out of the comparison
        assert float(np.abs(c64 - f25[p + "conf64"][b, :n]).max()) <= 1e-9         # double against the reference in double
        err, bar = _report(f"F25 ({name}) pair {b} confidence", f25[p + "conf"][b, :n].astype(np.float64), c64, c32)
        assert err <= bar
        assert float(np.abs(c64 - O.F25_THR).min()) > 2 * bar
        assert 0.25 <= float((c64 > O.F25_THR).mean()) <= 0.75
        assert np.array_equal(f25[p + "conf"][b, :n] > O.F25_THR, c64 > O.F25_THR)


def test_inlier_mask_preconditions_and_restatement(f25):
    ok, why = O.inlier_preconditions(f25)
    assert ok, why
    v6 = O.net_vec6d(f25, "b")
    for b, n in enumerate(O.F25_NETS["b"]["lens"]):
        rows = f25["b.match"][f25["b.match"][:, 0] == b]
        res = O.inlier_residual(f25["b.s_pcd"][b], f25["c.flow"][b], f25["c.rot"][b], f25["c.trn"][b], rows[:, 1], v6[b][:, 3:])
        mask = res < O.F25_INLIER_THR ** 2
        assert np.array_equal(mask, f25["c.mask"][b, :n])
        assert abs(float(mask.mean()) - float(f25["c.rate"][b])) < 1e-6


# ------------------------------------------------------------------------------------------ the modules
def test_position_codes_are_the_reference_layout():
    """the torch module against the restatement, both kinds, float64 on the CPU"""
    from deformationpyramid_amd import outlier
    v6 = O.matches(9, 3).astype(np.float64)
    for pe_type in ("rotary", "sinusoidal"):
        got = outlier.VolumetricPositionEncoding(O.config(48, 4, pe_type))(torch.from_numpy(v6)).numpy()
        want = O.position_code(v6, 48, pe_type)
        assert got.shape == want.shape == ((9, 48, 2) if pe_type == "rotary" else (9, 48))
        assert float(np.abs(got - want).max()) <= 1e-12
    assert outlier.VolumetricPositionEncoding(O.config(48, 4, "none"))(torch.from_numpy(v6)) is None


def test_module_refusals_and_state_dict(f25):
    from deformationpyramid_amd import outlier
    for pe_type in ("rotary", "sinusoidal"):
        for C in (6, 18, 30, 66):
            with pytest.raises(ValueError, match="% 12"):
                outlier.VolumetricPositionEncoding(O.config(C, 1, pe_type))
    with pytest.raises(ValueError, match="even head dimension"):
        outlier.CorrespondenceAttentionLayer(O.config(36, 4))                      # D = 9
    for cls in (outlier.VolumetricPositionEncoding, outlier.CorrespondenceAttentionLayer, outlier.Outlier_Rejection):
        with pytest.raises(KeyError):
            cls(O.config(48, 4, "learned"))
    with pytest.raises(ValueError, match="multiple of n_head"):
        outlier.CorrespondenceAttentionLayer(O.config(48, 5))
    cfg = outlier.DEFAULT_CONFIG
    assert (cfg["in_dim"], cfg["num_layers"], cfg["feature_dim"], cfg["n_head"], cfg["pe_type"], cfg["voxel_size"], cfg["sigma_spat"],
            cfg["spatial_consistency_check"]) == (6, 9, 144, 8, "rotary", 0.08, 0.1, True)
    net = outlier.Outlier_Rejection(cfg)
    assert len(net._6D_geometry_layers) == 9 and net._6D_geometry_layers[0].dim == 18
    for name in O.F25_NETS:                                                        # the reference's state dict, every key of it
        net = outlier.Outlier_Rejection(O.net_config(name))
        sd = P.sub_dict(f25, name + ".sd.")
        assert "classification.4.bias" in sd and "_6D_geometry_layers.0.norm2.bias" in sd and "in_proj.bias" in sd
        net.load_state_dict(tensors(sd), strict=True)
    for variant in O.F25_LAYER_VARIANTS:
        outlier.CorrespondenceAttentionLayer(O.config(48, 4, variant)).load_state_dict(tensors(P.sub_dict(f25, f"a.{variant}.sd.")), strict=True)
    layer = outlier.CorrespondenceAttentionLayer(O.config(48, 4))
    with pytest.raises(ValueError, match="6-D positions"):
        layer(torch.zeros(3, 48), torch.zeros(3, 48), None, None)


def test_no_matches_need_no_launch():
    """everything here runs on the CPU, where a launch would raise: an empty batch returns empty"""
    from deformationpyramid_amd import outlier
    net = outlier.Outlier_Rejection(O.net_config("b"))
    data = {"s_pcd": torch.rand(9, 3), "t_pcd": torch.rand(7, 3), "src_lengths": [5, 4], "tgt_lengths": [3, 4],
            "coarse_match_pred": torch.zeros(0, 3, dtype=torch.long)}
    conf, lens = net(data)
    assert tuple(conf.shape) == (0,) and lens == [0, 0] and tuple(data["vec_6d"].shape) == (0, 6) and tuple(data["vec_6d_ind"].shape) == (0, 2)
    keep, conf = outlier.reject_landmarks(net, torch.zeros(0, 3), torch.zeros(0, 3))
    assert tuple(keep.shape) == (0,) and keep.dtype == torch.bool and tuple(conf.shape) == (0,)
    masks, rates = outlier.compute_inlier_mask(data, 0.04, torch.zeros(9, 3), torch.eye(3).repeat(2, 1, 1), torch.zeros(2, 3, 1))
    assert [tuple(m.shape) for m in masks] == [(0,), (0,)] and all(torch.isnan(r) for r in rates)
    # matches of one pair only: the other is left out of the call (which then needs the GPU), its rows are grouped by pair
    data["coarse_match_pred"] = torch.tensor([[1, 2, 3], [1, 0, 1]])
    vec_6d, lens = net._3D_to_6D(data)
    assert lens == [0, 2] and torch.equal(vec_6d[0], torch.cat([data["s_pcd"][5 + 2], data["t_pcd"][3 + 3]]))
    assert torch.equal(data["vec_6d_ind"], torch.tensor([[2, 3], [0, 1]]))
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        net(data)


def test_driver_accepts_the_outlier_flags():
    import sys
    sys.path.insert(0, ROOT)
    import eval_supervised
    ap = eval_supervised.make_parser()
    a = ap.parse_args([])
    assert a.outlier_weights is None and a.outlier_thr == 0.5
    a = ap.parse_args(["--outlier-weights", "w.pth", "--outlier-thr", "0.3"])
    assert a.outlier_weights == "w.pth" and a.outlier_thr == 0.3


def test_inlier_mask_module_matches_the_fixture(f25):
    from deformationpyramid_amd import outlier
    n = O.F25_POINTS
    T = lambda a: torch.from_numpy(np.ascontiguousarray(a))
    data = {"s_pcd": T(f25["b.s_pcd"].reshape(-1, 3)), "t_pcd": T(f25["b.t_pcd"].reshape(-1, 3)), "src_lengths": [n, n], "tgt_lengths": [n, n],
            "coarse_match_pred": T(f25["b.match"].astype(np.int64))}
    _, lens = outlier.Outlier_Rejection._3D_to_6D(data)
    assert lens == O.F25_NETS["b"]["lens"]
    for b, v6 in enumerate(O.net_vec6d(f25, "b")):
        assert np.array_equal(data["vec_6d"][sum(lens[:b]):sum(lens[:b + 1])].numpy(), v6)
    masks, rates = outlier.compute_inlier_mask(data, O.F25_INLIER_THR, T(f25["c.flow"].reshape(-1, 3)), T(f25["c.rot"]), T(f25["c.trn"]))
    for b, m in enumerate(lens):
        assert np.array_equal(masks[b].numpy(), f25["c.mask"][b, :m])
        assert abs(float(rates[b]) - float(f25["c.rate"][b])) < 1e-6
