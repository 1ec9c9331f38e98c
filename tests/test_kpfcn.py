"""ops.kpconv (csrc/ndp_kpconv_conv.inc) and deformationpyramid_amd/kpfcn.py on the GPU against the numpy restatement of
tests/_kpfcn_ref.py: float64 at the project's bar -- max(4 x the float32 restatement's error, 16 float32 ulps of the largest
magnitude) --, exactness where the arithmetic is exact, and the reference's own numbers (fixture F23).  Every accuracy case prints
error / bar before it asserts (profiles/kpfcn_accuracy.txt is that output).  The cases' preconditions are asserted in
tests/test_kpfcn_cpu.py."""
import numpy as np
import pytest
import torch

from deformationpyramid_amd import kpconv, kpfcn, matching, ops
from tests import _kpconv_ref as R
from tests import _kpfcn_ref as K

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def run(c, idx=None, normalize=None, x=None, rows=None):
    """ops.kpconv on a case (int32 table unless `idx` is given as a tensor) -> numpy."""
    q = c.q if rows is None else c.q[rows]
    if idx is None:
        idx = dev((c.idx if rows is None else c.idx[rows]).astype(np.int32))
    y = ops.kpconv(dev(q), dev(c.s), idx, dev(c.x) if x is None else x, dev(c.W), dev(c.kp), c.extent, c.influence, c.aggregation,
                   c.normalize if normalize is None else normalize)
    return y.cpu().numpy()


def check(what, got, ref64, ref32):
    err, err32, mag = float(np.abs(got - ref64).max()), float(np.abs(ref32 - ref64).max()), float(np.abs(ref64).max())
    bar = R.bar(err32, mag)
    print(f"{what}: error {err:.3e}  bar {bar:.3e}  (eager float32 {err32:.3e}, magnitude {mag:.3e})  error / bar {err / bar:.3f}")
    assert got.shape == ref64.shape and np.isfinite(got).all()
    assert err <= bar


_refs = {}


def refs(name):
    if name not in _refs:
        c = K.make_case(name)
        _refs[name] = (K.run_case(c, np.float64), K.run_case(c, np.float32))
    return _refs[name]


# ------------------------------------------------------------------------------------------ the operator against float64
@pytest.mark.parametrize("name", [n for n in sorted(K.CASES) if n != "exact"])
def test_operator_against_float64(name):
    c = K.make_case(name)
    check(f"kpconv {name} {K.CASES[name][:6]}", run(c), *refs(name))


def test_int64_table_and_strided_features():
    """case 12: the reference's int64 tables and a non-contiguous x through the wrapper give the bits of the plain call"""
    c = K.make_case("c3")
    wide = torch.zeros(c.x.shape[0], 2 * c.x.shape[1], device=DEV)
    wide[:, ::2] = dev(c.x)
    x = wide[:, ::2]
    assert not x.is_contiguous()
    got = run(c, idx=dev(c.idx), x=x)
    check("kpconv c3 int64 idx, strided x", got, *refs("c3"))
    assert np.array_equal(got, run(c))


# ------------------------------------------------------------------------------------------ exactness and determinism
def test_shadows():
    c = K.make_case("c3")
    ns = c.s.shape[0]
    idx = c.idx.copy()
    idx[5] = ns
    idx[17] = ns                                                                  # rows whose neighbours are all shadows
    some = np.random.default_rng(0).random(idx.shape) < 0.3
    idx[some] = ns
    base = run(c, idx=dev(idx.astype(np.int32)))
    assert (base[5] == 0).all() and (base[17] == 0).all()
    check("kpconv c3 with shadows", base, K.run_case(c, np.float64, idx=idx), K.run_case(c, np.float32, idx=idx))
    for bad in (-1, ns + 5, 2 ** 31 - 1, -2 ** 31):
        other = idx.copy()
        other[idx == ns] = bad
        assert np.array_equal(run(c, idx=dev(other.astype(np.int32))), base), bad
    other = idx.copy()
    other[idx == ns] = 2 ** 40 + 3                                                # through the int64 path of the wrapper
    assert np.array_equal(run(c, idx=dev(other)), base)


def test_bitwise_on_exact_inputs():
    """constant influence, integer features, weights in eighths: every sum is exact in float32 whatever its order"""
    c = K.make_case("exact")
    y64 = K.run_case(c, np.float64, normalize=False)
    plain = run(c, normalize=False)
    assert np.abs(y64).max() < 2 ** 21 and np.array_equal(plain.astype(np.float64), y64)
    _, _, _, count = K.kpconv(c.q, c.s, c.idx, c.x, c.W, c.kp, c.extent, c.influence, c.aggregation, True, np.float64, want=True)
    assert count.max() > 1 and (c.x.sum(1) <= 0).any()
    assert np.array_equal(run(c, normalize=True), y64.astype(np.float32) / count[:, None].astype(np.float32))
    g = np.random.default_rng(1)
    perm = np.stack([row[g.permutation(len(row))] for row in c.idx])
    assert np.array_equal(run(c, idx=dev(perm.astype(np.int32)), normalize=False), plain)


def test_same_call_same_bits():
    c = K.make_case("c5")
    assert np.array_equal(run(c), run(c))


def test_rows_do_not_depend_on_the_other_queries():
    c = K.make_case("c5")
    assert c.q.shape[0] == 129
    assert np.array_equal(run(c)[10:21], run(c, rows=slice(10, 21)))


# ------------------------------------------------------------------------------------------ blocks and network
@pytest.fixture(scope="module")
def f23():
    batch, z = K.load_f23()
    tbatch = {k: [dev(a) for a in v] if k != "stack_lengths" else [torch.from_numpy(a) for a in v] for k, v in batch.items() if k != "features"}
    tbatch["features"] = dev(batch["features"])
    return batch, tbatch, z


def tensors(sd):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}


@pytest.mark.parametrize("i", range(len(K.F23_BLOCKS)))
def test_blocks(f23, i):
    batch, tbatch, z = f23
    name, cin, cout = K.F23_BLOCKS[i]
    sd, x = K.state_dict(z, f"b{i}.sd."), z[f"x{cin}"].astype(np.float32)
    block = kpfcn.block_decider(name, K.RADIUS, cin, cout, 0, K.F23_CONFIG)
    block.load_state_dict(tensors(sd), strict=True)
    with torch.no_grad():
        got = block.to(DEV)(dev(x), tbatch).cpu().numpy()
    fn = K.simple_block if "simple" in name else K.resnet_block
    y64, y32 = (fn(sd, "", x, batch, 0, "strided" in name, K.F23_CONFIG, dt) for dt in (np.float64, np.float32))
    check(f"block {name} {cin} -> {cout}", got, y64, y32)


@pytest.fixture(scope="module")
def network(f23):
    batch, tbatch, z = f23
    sd = K.state_dict(z, "c.sd.")
    model = kpfcn.KPFCN(K.F23_CONFIG)
    model.load_state_dict(tensors(sd), strict=True)                                # the reference's names, every one of them
    model = model.to(DEV).eval()
    with torch.no_grad():
        got = model(tbatch, phase="coarse")
    return model, sd, got


def test_coarse_forward(f23, network):
    batch, tbatch, z = f23
    model, sd, got = network
    y64, y32 = (K.kpfcn_coarse(sd, batch, K.F23_CONFIG, dt) for dt in (np.float64, np.float32))
    assert tuple(got.shape) == (batch["points"][2].shape[0], K.F23_CONFIG["coarse_feature_dim"]) == (113, 12)
    got = got.cpu().numpy()
    check("KPFCN coarse forward against float64", got, y64, y32)
    err, err32, mag = float(np.abs(got - z["c.out"]).max()), float(np.abs(y32 - y64).max()), float(np.abs(y64).max())
    print(f"KPFCN coarse forward against the reference's float32 output: error {err:.3e}  bar {R.bar(err32, mag):.3e}")
    assert err <= R.bar(err32, mag)


def test_coarse_features_end_to_end(f23, network):
    batch, tbatch, z = f23
    model, sd, got = network
    cfg = K.F23_CONFIG
    pts, lengths = tbatch["points"][0], batch["stack_lengths"][0]
    cpts, clen, feats = kpfcn.coarse_features(model, pts, lengths, cfg, R.PYRAMID_LIMITS)
    pyr = kpconv.build_pyramid(pts, lengths, cfg["first_subsampling_dl"], cfg["conv_radius"], cfg["deform_radius"], cfg["architecture"], R.PYRAMID_LIMITS)
    assert torch.equal(cpts, pyr["points"][2]) and [int(v) for v in clen] == [int(v) for v in pyr["stack_lengths"][2]]
    seen = {}
    forward = model.forward
    model.forward = lambda b, phase="coarse": (seen.update(b), forward(b, phase))[1]
    try:
        cpts, clen, feats = kpfcn.coarse_features(model, pts, lengths, cfg, R.PYRAMID_LIMITS)
    finally:
        del model.forward
    for key in ("points", "neighbors", "pools", "upsamples"):                     # the tables it ran on are build_pyramid's
        for l in range(4):
            assert torch.equal(pyr[key][l], seen[key][l]), (key, l)
    assert torch.equal(seen["features"], torch.ones(1200, 1, device=DEV))
    pyr["features"] = tbatch["features"]
    with torch.no_grad():
        assert torch.equal(feats, model(pyr, phase="coarse"))
    assert tuple(feats.shape) == (113, 12) and sum(int(v) for v in clen) == 113
    n0 = int(clen[0])
    fs, ft = feats[:n0].contiguous(), feats[n0:].contiguous()
    index, mconf = matching.dual_softmax_match(fs, ft, confidence_threshold=0.0)
    assert index.ndim == 2 and index.shape[1] == 3 and index.shape[0] == mconf.shape[0]
    assert (index[:, 1] < n0).all() and (index[:, 2] < feats.shape[0] - n0).all()


def test_refusals():
    cfg = dict(K.F23_CONFIG)
    for bad in (dict(deformable=True), dict(modulated=True), dict(architecture=["simple", "resnetb_deformable"]),
                dict(architecture=["simple_equivariant"]), dict(architecture=["simple_invariant"])):
        with pytest.raises(NotImplementedError):
            kpfcn.KPFCN({**cfg, **bad})
    with pytest.raises(NotImplementedError):
        kpfcn.KPFCN(cfg).to(DEV)({"features": torch.ones(3, 1, device=DEV)}, phase="fine")
