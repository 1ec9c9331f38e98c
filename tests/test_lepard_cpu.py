"""Attention, the dense confidence matrix and the Lepard modules without a GPU: the ABI carries the entries, every refusal that needs
no device, the workspace query, the numpy restatement (tests/_lepard_ref.py) against the reference's own modules (fixture F24), the
preconditions of the fixture's cases, and the module-level refusals and the strict state-dict load of deformationpyramid_amd/lepard.py."""
import ctypes
import os

import numpy as np
import pytest
import torch

from deformationpyramid_amd import _native
from tests import _kpconv_ref as R
from tests import _kpfcn_ref as K
from tests import _lepard_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("ndp_attention_forward", "ndp_feat_conf_workspace", "ndp_feat_conf")
E_INVALID, E_UNSUPPORTED = -1, -2


@pytest.fixture(scope="module")
def L():
    return _native.lib()


@pytest.fixture(scope="module")
def f24():
    return P.load_f24()


def test_abi_carries_the_entries(L):
    assert L.ndp_version() >= 215 and _native.ABI_VERSION == 215
    header = open(os.path.join(ROOT, "include", "ndp_hip.h")).read()
    for name in ENTRIES:
        assert name in _native._SIGS and name in _native.EXPORTS and getattr(L, name)
        assert f"int {name}(" in header
    assert "ndp_attention.inc" in " ".join(_native.HEADERS)


def test_workspace_query_needs_no_device(L):
    nb = ctypes.c_longlong()
    assert L.ndp_feat_conf_workspace(3, 2000, 1900, ctypes.byref(nb)) == 0 and nb.value == 4 * 3900
    assert L.ndp_feat_conf_workspace(1, 1, 1, ctypes.byref(nb)) == 0 and nb.value == 8
    assert L.ndp_feat_conf_workspace(1, 5, 5, None) == E_INVALID
    for args in ((0, 5, 5), (65536, 5, 5), (1, 0, 5), (1, 5, 0), (1, 1 << 31, 5), (1, 5, 1 << 31)):
        assert L.ndp_feat_conf_workspace(*args, ctypes.byref(nb)) == E_INVALID, args


def _buffers():
    buf = (ctypes.c_char * 4096)()
    p = ctypes.cast(ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16, ctypes.c_void_p)
    return buf, p, ctypes.c_void_p(p.value + 1)


def _off(*v):
    return (ctypes.c_int * len(v))(*v)


def test_attention_entry_refuses_bad_arguments(L):
    """every refusal is decided before the first HIP call: the device pointers are never read"""
    buf, p, odd = _buffers()

    def fwd(q=p, k=p, v=p, pe_q=None, pe_k=None, offQ=p, offK=p, hq=_off(0, 5), hk=_off(0, 7), B=1, C=48, H=4, scale=0.25, o=p):
        return L.ndp_attention_forward(q, k, v, pe_q, pe_k, offQ, offK, hq, hk, B, C, H, scale, o, None)

    invalid = [(dict(B=0), b"B must"), (dict(B=65536), b"B must"), (dict(hq=None), b"null"), (dict(hk=None), b"null"),
               (dict(hq=_off(0, 0)), b"non-empty"), (dict(hk=_off(3, 3)), b"non-empty"), (dict(hq=_off(-1, 5)), b"start at 0"),
               (dict(hq=_off(0, 5, 3), hk=_off(0, 3, 7), B=2), b"monotone"), (dict(pe_q=p), b"both or neither"), (dict(pe_k=p), b"both or neither"),
               (dict(pe_q=p, pe_k=p, C=66, H=2), b"even head dimension"), (dict(pe_q=p, pe_k=p, C=33, H=1), b"even head dimension"),
               (dict(scale=float("nan")), b"scale"), (dict(scale=float("inf")), b"scale"), (dict(scale=float("-inf")), b"scale")]
    invalid += [(dict([(name, None)]), b"null") for name in ("q", "k", "v", "offQ", "offK", "o")]
    invalid += [(dict([(name, odd)]), b"aligned") for name in ("q", "k", "v", "offQ", "offK", "o")]
    invalid += [(dict(pe_q=odd, pe_k=p), b"aligned"), (dict(pe_q=p, pe_k=odd), b"aligned")]
    for kw, word in invalid:
        assert fwd(**kw) == E_INVALID, kw
        assert word in L.ndp_last_error(), (kw, L.ndp_last_error())
    for kw in (dict(C=0), dict(C=1057, H=1), dict(H=0), dict(H=17, C=17 * 6), dict(C=50, H=4), dict(C=265, H=1), dict(C=1060, H=4),
               dict(hq=_off(0, (1 << 30) + 1)), dict(hk=_off(0, (1 << 30) + 1))):
        assert fwd(**kw) == E_UNSUPPORTED, kw
        assert b"served are" in L.ndp_last_error()


def test_feat_conf_entry_refuses_bad_arguments(L):
    buf, p, odd = _buffers()

    def conf(fs=p, ft=p, offS=p, offT=p, hs=_off(0, 5), ht=_off(0, 7), B=1, C=8, temperature=0.1, ws=p, out=p, Smax=5, Tmax=7):
        return L.ndp_feat_conf(fs, ft, offS, offT, hs, ht, B, C, temperature, ws, out, Smax, Tmax, None)

    invalid = [(dict(B=0), b"B must"), (dict(hs=None), b"null"), (dict(C=0), b"C must"), (dict(C=1057), b"C must"), (dict(hs=_off(0, 0)), b"non-empty"),
               (dict(ht=_off(2, 1)), b"monotone"), (dict(temperature=0.0), b"temperature"), (dict(temperature=-1.0), b"temperature"),
               (dict(temperature=float("nan")), b"temperature"), (dict(temperature=float("inf")), b"temperature"), (dict(Smax=4), b"Smax"),
               (dict(Tmax=6), b"Tmax")]
    invalid += [(dict([(name, None)]), b"null") for name in ("fs", "ft", "offS", "offT", "ws", "out")]
    invalid += [(dict([(name, odd)]), b"aligned") for name in ("fs", "ft", "offS", "offT", "ws", "out")]
    for kw, word in invalid:
        assert conf(**kw) == E_INVALID, kw
        assert word in L.ndp_last_error(), (kw, L.ndp_last_error())


def test_wrappers_refuse_bad_arguments():
    from deformationpyramid_amd import ops
    q, k = torch.zeros(5, 48), torch.zeros(7, 48)
    pe_q, pe_k = torch.zeros(5, 48, 2), torch.zeros(7, 48, 2)
    for a in (dict(q=q[:, :47]), dict(v=k[:6]), dict(n_head=5), dict(n_head=0), dict(pe_q=pe_q), dict(pe_q=pe_q, pe_k=pe_k[:6]),
              dict(pe_q=pe_q[:, :, :1], pe_k=pe_k), dict(scale=float("nan")), dict(q=torch.zeros(5, 66), k=torch.zeros(7, 66), v=torch.zeros(7, 66),
                                                                                    n_head=2, pe_q=torch.zeros(5, 66, 2), pe_k=torch.zeros(7, 66, 2))):
        kw = dict(q=q, k=k, v=k, n_head=4)
        kw.update(a)
        with pytest.raises(ValueError):
            ops.attention(**kw)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.attention(q, k, k, 4)
    with pytest.raises(_native.NdpError, match="no CPU fallback"):
        ops.feat_conf(q, k)
    with pytest.raises(ValueError):
        ops.feat_conf(q, k[:, :40])


def test_module_refusals_and_state_dict(f24):
    from deformationpyramid_amd import lepard
    with pytest.raises(NotImplementedError, match="randSO3"):
        lepard.RepositioningTransformer(P.transformer_config(24, 4, positioning_type="randSO3"))
    sink = P.transformer_config(24, 4).feature_matching
    with pytest.raises(NotImplementedError, match="sinkhorn"):
        lepard.Matching({**sink, "match_type": "sinkhorn"})
    for pe_type in ("rotary", "sinusoidal"):
        with pytest.raises(ValueError, match="% 6"):
            lepard.VolumetricPositionEncoding(P.transformer_config(16, 4, pe_type))
    with pytest.raises(ValueError, match="even head dimension"):
        lepard.GeometryAttentionLayer(P.transformer_config(66, 2))                 # D = 33
    with pytest.raises(KeyError):
        lepard.GeometryAttentionLayer(P.transformer_config(24, 4, "learned"))
    lepard.RepositioningTransformer(P.transformer_config(24, 4, positioning_type="oracle", entangled=True))
    # the reference's Pipeline state dict, every key of it: backbone.* is F23's, the rest F24 (c)'s
    _, z23 = K.load_f23()
    sd = {"backbone." + k: v for k, v in K.state_dict(z23, "c.sd.").items()}
    sd.update(P.sub_dict(f24, "c.sd."))
    assert any(k.startswith("coarse_transformer.layers.2.0.tgt_proj") for k in sd) and any(k.startswith("coarse_matching.src_proj") for k in sd)
    pipe = lepard.Pipeline(P.pipeline_config())
    pipe.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    net = lepard.RepositioningTransformer(P.b_config())
    net.load_state_dict({k: torch.from_numpy(v) for k, v in P.sub_dict(f24, "b.below.t.sd.").items()}, strict=True)


def test_position_codes_are_the_reference_layout():
    """the torch module against the restatement, both kinds, float64 on the CPU"""
    from deformationpyramid_amd import lepard
    pts = np.random.default_rng(0).uniform(0, 1, (9, 3)) + np.asarray(P.VOL_BNDS[0])
    for pe_type in ("rotary", "sinusoidal"):
        got = lepard.VolumetricPositionEncoding(P.transformer_config(24, 4, pe_type))(torch.from_numpy(pts)).numpy()
        want = P.position_code(pts, 24, pe_type, 0.04)
        assert got.shape == want.shape == ((9, 24, 2) if pe_type == "rotary" else (9, 24))
        assert float(np.abs(got - want).max()) <= 1e-12
    x = torch.arange(12.0).reshape(2, 6)
    r = lepard.VolumetricPositionEncoding.embed_rotary(x, torch.zeros(2, 6), torch.ones(2, 6))
    assert torch.equal(r[0], torch.tensor([-1.0, 0.0, -3.0, 2.0, -5.0, 4.0]))


def _report(what, got, ref64, ref32):
    err, err32, mag = float(np.abs(got - ref64).max()), float(np.abs(ref32.astype(np.float64) - ref64).max()), float(np.abs(ref64).max())
    bar = R.bar(err32, mag)
    print(f"{what}: error {err:.3e}  eager float32 {err32:.3e}  magnitude {mag:.3e}  bar {bar:.3e}")
    return err, bar


def test_fixture_is_small(f24):
    assert os.path.getsize(P.F24) <= 900 * 1024
    assert all(f24[k].dtype.kind in "fiub" for k in f24.files)                     # numbers only


@pytest.mark.parametrize("variant", P.F24_LAYER_VARIANTS)
def test_restatement_reproduces_the_reference_layer(f24, variant):
    p = f"a.{variant}."
    pe_type = "sinusoidal" if variant == "sinusoidal" else "rotary"
    sd = P.sub_dict(f24, p + "sd.")
    for b, (Lb, Sb) in enumerate(f24[p + "lens"].tolist()):
        outs = []
        for dt in (np.float64, np.float32):
            x_pe = s_pe = None
            if variant != "none":
                x_pe, s_pe = (P.position_code(f24[p + k][b, :n], 48, pe_type, 0.04, dtype=dt) for k, n in (("x_pts", Lb), ("source_pts", Sb)))
            outs.append(P.attention_layer(sd, "", f24[p + "x"][b, :Lb], f24[p + "source"][b, :Sb], x_pe, s_pe, 4, pe_type, dt))
        assert float(np.abs(outs[0] - f24[p + "out64"][b, :Lb]).max()) <= 1e-9 * float(np.abs(outs[0]).max())      # double against the reference in double
        err, bar = _report(f"F24 (a) {variant} problem {b}", f24[p + "out"][b, :Lb], *outs)
        assert err <= bar


@pytest.mark.parametrize("case", P.F24_B_CASES)
def test_fixture_preconditions_and_the_reference_transformer(f24, case):
    """conditions away from the threshold, the top-n cuts open, and (B = 1) the reference's float32 numbers inside the bar"""
    ok, why = P.b_preconditions(f24, case)
    assert ok, why
    p = f"b.{case}."
    r64, r32 = P.run_b(f24, case, np.float64), P.run_b(f24, case, np.float32)
    side = {"below": True, "above": False}
    for b, (S, T) in enumerate(f24[p + "lens"].tolist()):
        if case in side:
            assert r64[b].layers[0].fit.mask is side[case] and bool(f24[p + "pl.mask"][b]) is side[case]
        bb, got, want = P.bars(r64[b], r32[b]), P.recorded(f24, p, b, S, T), P.quantities(r64[b])
        for k in want:                                                             # at B = 2 as well: the problems' n_b are equal
            err = float(np.abs(got[k].astype(np.float64) - want[k]).max())
            print(f"F24 (b) {case} problem {b} {k}: error {err:.3e}  bar {bb[k]:.3e}")
            assert err <= bb[k]
        assert f24[p + "conf"][b, S:].max(initial=0) == 0 and f24[p + "conf"][b, :, T:].max(initial=0) == 0       # the reference's padding is exactly 0


def test_restatement_reproduces_the_reference_pipeline(f24):
    batch, z23 = K.load_f23()
    sd = {"backbone." + k: v for k, v in K.state_dict(z23, "c.sd.").items()}
    sd.update(P.sub_dict(f24, "c.sd."))
    cfg = P.pipeline_config()
    r64, r32 = P.pipeline(sd, cfg, batch, np.float64), P.pipeline(sd, cfg, batch, np.float32)
    assert r64.feats.shape == (113, 12) and r64.conf.shape == f24["c.conf"].shape[1:]
    pl64, pl32 = r64.layers[0], r32.layers[0]
    for what, got, a, b in (("conf_matrix_pred", f24["c.conf"][0], r64.conf, r32.conf), ("R", f24["c.R"][0], r64.fit.R, r32.fit.R),
                            ("t", f24["c.t"][0], r64.fit.t, r32.fit.t), ("position conf", f24["c.pl.conf"][0], pl64.conf, pl32.conf),
                            ("position R", f24["c.pl.R"][0], pl64.fit.R, pl32.fit.R), ("position t", f24["c.pl.t"][0], pl64.fit.t, pl32.fit.t),
                            ("position condition", f24["c.pl.condition"], np.asarray([pl64.fit.condition]), np.asarray([pl32.fit.condition]))):
        err, bar = _report(f"F24 (c) {what}", got.astype(np.float64), a, b)
        assert err <= bar
    assert abs(pl64.fit.condition / P.MAX_CONDITION - 1) >= 0.1 and bool(f24["c.pl.mask"][0]) == pl64.fit.mask
    assert np.array_equal(f24["c.match"][:, 1:], r64.match) and np.array_equal(f24["c.pl.match"][:, 1:], pl64.match)
