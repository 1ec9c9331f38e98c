"""Pins the CPU oracle (oracle/ndp_oracle.c) and the host-side init replay against golden
vectors captured FROM THE REFERENCE (tests/golden/make_golden.py, run in the build container).

These are `not gpu` tests.  Tolerances are float32 round-off class: the reference's sgemm and
the oracle's fmaf chains sum in different orders.
"""
import os

import numpy as np
import pytest
import torch

from oracle import ndp_oracle as O
from tests._helpers import VARIANTS, seeded_pyramid, scale_heads, flat_from_named, wsum, rel_err

K0 = -8


def cdesc(d):
    return O.make_desc(d.width, d.n_hidden, d.motion, d.rotfmt, d.nonrigidity, d.mlp_scale)


# ----------------------------------------------------------------------------- F1: init replay
@pytest.mark.parametrize("tag,kw", [
    ("se3aa_m9", dict(m=9, rotation_format="axis_angle", motion="SE3")),
    ("sim3eu_m9", dict(m=9, rotation_format="euler", motion="Sim3")),
    ("se3aa_m10", dict(m=10, rotation_format="axis_angle", motion="SE3")),
    ("se3quat_nr_m3", dict(m=3, rotation_format="quaternion", motion="SE3", nonrigidity_est=True)),
    ("sflow6d_m2", dict(m=2, rotation_format="6D", motion="sflow")),
])
def test_F1_init_replays_reference_rng(golden, tag, kw):
    g = golden("F1_init")
    pyr = seeded_pyramid(0, **kw)
    names, sums, asums, heads = [], [], [], []
    for li, layer in enumerate(pyr.pyramid):
        for k, v in layer.named_parameters():
            a = v.detach().double().numpy().ravel()
            names.append(f"{li}.{k}")
            sums.append(a.sum())
            asums.append(np.abs(a).sum())
            h = np.zeros(8)
            h[:min(8, a.size)] = a[:8]
            heads.append(h)
    assert names == list(g[f"{tag}.names"])
    np.testing.assert_array_equal(np.array(heads), g[f"{tag}.head8"])          # bit-exact
    np.testing.assert_allclose(np.array(sums), g[f"{tag}.sum"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(asums), g[f"{tag}.abssum"], rtol=1e-12)
    # the RNG stream continues identically after construction (registration.py:156-157)
    np.testing.assert_array_equal(torch.randperm(8192)[:16].numpy(), g[f"{tag}.perm8192"])
    np.testing.assert_array_equal(torch.randperm(6100)[:16].numpy(), g[f"{tag}.perm6100"])


def test_param_counts_match_survey():
    assert seeded_pyramid(0, m=1, **VARIANTS["se3aa"]).descs[0].param_count == 34694
    assert seeded_pyramid(0, m=1, **VARIANTS["sim3eu"]).descs[0].param_count == 34823


# ------------------------------------------------------------------- F2: level forward + grads
def _f2_pyramid(g, tag):
    pyr = seeded_pyramid(int(g["seed"]), **VARIANTS[tag])
    levels = (0, 4, 8) if tag in ("se3aa", "sim3eu") else (4,)
    for lvl in levels:
        scale_heads(pyr, lvl, float(g["head_scale"]))
        assert abs(wsum(pyr, lvl) - float(g[f"{tag}.L{lvl}.wsum"])) < 1e-6 * float(g[f"{tag}.L{lvl}.wsum"])
    return pyr, levels


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_F2_level_forward_and_grads(golden, tag):
    g = golden("F2_layer_forward")
    pyr, levels = _f2_pyramid(g, tag)
    x = g["x"]
    coef = np.linspace(-1.0, 1.0, 256 * 3, dtype=np.float32).reshape(256, 3)
    coef = torch.linspace(-1.0, 1.0, 256 * 3).reshape(256, 3).numpy()
    for lvl in levels:
        d = pyr.descs[lvl]
        params = pyr.store[lvl, :d.param_count].numpy()
        out = O.level_fwd(cdesc(d), params, lvl, K0, x)
        np.testing.assert_allclose(out, g[f"{tag}.L{lvl}.out"], rtol=0, atol=2e-6)
        grads = O.level_bwd(cdesc(d), params, lvl, K0, x, coef)
        for name, off, shape in d.named_slices():
            ref = g[f"{tag}.L{lvl}.grad.{name}"]
            got = grads[off:off + ref.size].reshape(ref.shape)
            assert rel_err(got, ref) < 1e-4, (tag, lvl, name, rel_err(got, ref))  # cancelling sums, fp32 order


@pytest.mark.parametrize("tag", list(VARIANTS))
def test_F2_full_pyramid_inference(golden, tag):
    g = golden("F2_layer_forward")
    pyr, _ = _f2_pyramid(g, tag)
    descs = [cdesc(d) for d in pyr.descs]
    params_all = np.concatenate([pyr.store[i, :d.param_count].numpy() for i, d in enumerate(pyr.descs)])
    out = O.pyramid_fwd(descs, K0, params_all, g["x"])
    # nine chained levels; the quaternion / 6D heads normalise a 1e-4-sized vector, which amplifies round-off
    np.testing.assert_allclose(out, g[f"{tag}.full_out"], rtol=0, atol=5e-6 if "quat" not in tag and "6d" not in tag else 2e-5)


# ------------------------------------------------------------------------------- F3: Chamfer
@pytest.mark.parametrize("tag,trunc", [("full", 1e9), ("trunc", 0.01)])
def test_F3_chamfer(golden, tag, trunc):
    g = golden("F3_chamfer")
    r = O.chamfer(g["x"], g["y"], trunc=trunc)
    np.testing.assert_array_equal(r["idx_x"], g[f"{tag}.idx_x"])              # bit-exact indices
    np.testing.assert_array_equal(r["idx_y"], g[f"{tag}.idx_y"])
    np.testing.assert_allclose(r["d2x"], g[f"{tag}.d2_x"], rtol=3e-7, atol=0)
    np.testing.assert_allclose(r["d2y"], g[f"{tag}.d2_y"], rtol=3e-7, atol=0)
    assert abs(float(r["loss"]) - float(g[f"{tag}.loss"])) < 2e-6 * float(g[f"{tag}.loss"])
    np.testing.assert_allclose(r["gx"], g[f"{tag}.grad_x"], rtol=0, atol=2e-6 * np.abs(g[f"{tag}.grad_x"]).max())
    if tag == "trunc":
        assert (g["trunc.d2_x"] >= trunc).any() and (g["trunc.d2_x"] < trunc).any()


# ---------------------------------------------------------- F4/F5: one iteration, 20 iterations
ITER_CASES = [("se3aa.L0", "se3aa", 0), ("se3aa.L5", "se3aa", 5), ("sim3eu.L2", "sim3eu", 2), ("sflow.L3", "sflow", 3)]


def _run_level(g, tag, var, lvl, n_iter, landmarks=False, fixture_prefix=None):
    pre = fixture_prefix or tag
    pyr = seeded_pyramid(int(g[f"{pre}.seed"]), **VARIANTS[var])
    assert abs(wsum(pyr, lvl) - float(g[f"{pre}.wsum"])) < 1e-6 * float(g[f"{pre}.wsum"])
    d = pyr.descs[lvl]
    cd = cdesc(d)
    p = pyr.store[lvl, :d.param_count].numpy().copy()
    m = np.zeros_like(p)
    v = np.zeros_like(p)
    x, y = g[f"{pre}.x"], g[f"{pre}.y"]
    rec = dict(losses=[])
    for it in range(n_iter):
        w = O.level_fwd(cd, p, lvl, K0, x)
        if landmarks:
            L, gx = O.landmark(w, y)
        else:
            r = O.chamfer(w, y)
            L, gx = r["loss"], r["gx"]
        rec["losses"].append(float(L))
        grads = O.level_bwd(cd, p, lvl, K0, x, gx)
        if it == 0:
            rec["warp0"], rec["grad0"] = w, grads.copy()
        O.adam(p, grads, m, v, it + 1)
        if it in (0, 2):
            rec[f"step{it + 1}"] = p.copy()
    rec["warp_final"] = O.level_fwd(cd, p, lvl, K0, x)
    return d, rec


@pytest.mark.parametrize("tag,var,lvl", ITER_CASES)
def test_F4_one_iteration(golden, tag, var, lvl):
    g = golden("F4F5_iteration")
    d, rec = _run_level(g, tag, var, lvl, n_iter=3)
    np.testing.assert_allclose(rec["warp0"], g[f"{tag}.warp0"], rtol=0, atol=1e-6)
    assert abs(rec["losses"][0] - g[f"{tag}.losses"][0]) < 2e-6 * g[f"{tag}.losses"][0]
    for name, off, shape in d.named_slices():
        ref = g[f"{tag}.grad0.{name}"]
        got = rec["grad0"][off:off + ref.size].reshape(ref.shape)
        assert rel_err(got, ref) < 1e-4, (name, rel_err(got, ref))
        # Adam: step 1 moves every parameter by ~lr*sign(g) whatever |g| is, so parameters whose
        # gradient is round-off noise can legitimately differ by 2*lr; compare where |g| is material.
        ref3 = g[f"{tag}.step3.{name}"]
        got3 = rec["step3"][off:off + ref3.size].reshape(ref3.shape)
        mask = np.abs(ref) > 1e-3 * np.abs(ref).max()
        assert np.abs(got3 - ref3)[mask].max() < 2e-4, name
        if tag == "se3aa.L0":
            ref1 = g[f"{tag}.step1.{name}"]
            got1 = rec["step1"][off:off + ref1.size].reshape(ref1.shape)
            assert np.abs(got1 - ref1)[mask].max() < 1e-5, name


@pytest.mark.parametrize("tag,var,lvl", ITER_CASES)
def test_F5_short_trajectory(golden, tag, var, lvl):
    g = golden("F4F5_iteration")
    _, rec = _run_level(g, tag, var, lvl, n_iter=20)
    ref = g[f"{tag}.losses"]
    got = np.array(rec["losses"])
    assert abs(got[1] - ref[1]) < 1e-4 * ref[1]
    assert np.abs(got - ref).max() < 1e-2 * ref.max()          # loosens to 1e-2 by step 20
    assert np.abs(rec["warp_final"] - g[f"{tag}.warp_final"]).mean() < 5e-3


def test_F9_landmark_iterations(golden):
    g = golden("F9_landmarks")
    d, rec = _run_level(g, "ldmk.L0", "se3aa", 0, n_iter=8, landmarks=True)
    ref = g["ldmk.L0.losses"]
    assert abs(rec["losses"][0] - ref[0]) < 2e-6 * ref[0]
    assert np.abs(np.array(rec["losses"]) - ref).max() < 1e-2 * ref.max()
    for name, off, shape in d.named_slices():
        r0 = g[f"ldmk.L0.grad0.{name}"]
        got = rec["grad0"][off:off + r0.size].reshape(r0.shape)
        assert rel_err(got, r0) < 1e-4, name


def test_F9c_mixed_landmark_plus_truncated_chamfer(golden):
    """registration.py:189-197 (landmarks and samples warped together, landmark MSE + w_cd * truncated Chamfer) as the
    reference computes it: loss trace of 8 forced iterations, gradients of step 0, parameters after step 3."""
    g = golden("F9c_mixed")
    K, w_cd, trunc = g["src_ldmk"].shape[0], float(g["w_cd"]), float(g["trunc"])
    pyr = seeded_pyramid(int(g["seed"]), **VARIANTS["se3aa"])
    assert abs(wsum(pyr, 0) - float(g["wsum"])) < 1e-6 * float(g["wsum"])
    d = pyr.descs[0]
    cd = cdesc(d)
    p0 = pyr.store[0, :d.param_count].numpy().copy()
    pts = np.concatenate([g["src_ldmk"], g["s_sample"]])
    # one step by hand: the two gradient parts combine as the reference's autograd does
    w = O.level_fwd(cd, p0, 0, K0, pts)
    np.testing.assert_allclose(w, g["warp0"], rtol=0, atol=1e-6)
    L_l, g_l = O.landmark(w[:K], g["tgt_ldmk"])
    r = O.chamfer(w[K:], g["t_sample"], trunc=trunc)
    assert 0 < (r["d2x"] >= trunc).sum() < r["d2x"].size           # the truncation really cuts some terms, not all
    assert abs(float(L_l) - g["losses_ldmk"][0]) < 2e-6 * g["losses_ldmk"][0]
    assert abs(float(r["loss"]) - g["losses_cd"][0]) < 2e-6 * g["losses_cd"][0]
    grads = O.level_bwd(cd, p0, 0, K0, pts, np.concatenate([g_l, w_cd * r["gx"]]))
    for name, off, shape in d.named_slices():
        ref = g[f"grad0.{name}"]
        assert rel_err(grads[off:off + ref.size].reshape(ref.shape), ref) < 1e-4, name
    # the whole loop through the oracle's optimiser (what the engine tests compare against)
    out = O.optimize([cd], p0, pts, K, pts.shape[0] - K, g["tgt_ldmk"], g["t_sample"], k0=K0, iters=8, w_cd=w_cd,
                     trunc=trunc, early_stop=False, nthreads=4)
    ref = g["losses"]
    assert abs(out["loss_trace"][0] - ref[0]) < 2e-6 * ref[0]
    assert np.abs(out["loss_trace"] - ref).max() < 1e-3 * ref.max()
    out3 = O.optimize([cd], p0, pts, K, pts.shape[0] - K, g["tgt_ldmk"], g["t_sample"], k0=K0, iters=3, w_cd=w_cd,
                      trunc=trunc, early_stop=False, nthreads=4)
    for name, off, shape in d.named_slices():
        ref3, r0 = g[f"step3.{name}"], g[f"grad0.{name}"]
        mask = np.abs(r0) > 1e-3 * np.abs(r0).max()
        got3 = out3["params_all"][off:off + ref3.size].reshape(ref3.shape)
        assert np.abs(got3 - ref3)[mask].max() < 2e-4, name


def _f13_setup(g):
    pyr = seeded_pyramid(0, **VARIANTS["sim3eu"])
    assert abs(wsum(pyr, 0) - float(g["wsum"])) < 1e-6 * float(g["wsum"])
    return pyr, pyr.descs[0]


def test_F13_shape_transfer_loop_and_vertex_warp(golden):
    """shape_transfer.py:116-166 on 6000 seeded vertices of each demo mesh (Sim3 / euler): the oracle follows the
    reference's first ten iterations of level 0 and reproduces the 24 856-vertex inference warp."""
    g = golden("F13_shape_transfer")
    pyr, d = _f13_setup(g)
    cd = cdesc(d)
    p0 = pyr.store[0, :d.param_count].numpy().copy()
    S = g["s_sample"].shape[0]
    out = O.optimize([cd], p0, g["s_sample"], 0, S, None, g["t_sample"], k0=K0, iters=10, early_stop=False, nthreads=8)
    ref = g["losses"]
    assert abs(out["loss_trace"][0] - ref[0]) < 2e-6 * ref[0]
    assert np.abs(out["loss_trace"] - ref).max() < 2e-3 * ref.max()
    # gradients of step 0 (checksums + strided slices of the big matrices)
    w = O.level_fwd(cd, p0, 0, K0, g["s_sample"], nthreads=8)
    r = O.chamfer(w, g["t_sample"], nthreads=8)
    grads = O.level_bwd(cd, p0, 0, K0, g["s_sample"], r["gx"], nthreads=8)
    for name, off, shape in d.named_slices():
        n = int(np.prod(shape))
        got = grads[off:off + n]
        assert abs(got.astype(np.float64).sum() - float(g[f"gsum0.{name}"])) < 2e-4 * float(g[f"gabs0.{name}"]) + 1e-9, name
        refv = g[f"grad0.{name}"].reshape(-1)
        gotv = got if n <= 1024 else got[::37]
        assert rel_err(gotv, refv) < 2e-4, name
    # inference warp of all source vertices with the reference's trained level 0 and the untouched levels 1..8
    params_all = np.concatenate([pyr.store[i, :d.param_count].numpy() for i in range(9)])
    named = {name: g[f"final.{name}"] for name, _, _ in d.named_slices()}
    params_all[:d.param_count] = flat_from_named(d, named)
    got = O.pyramid_fwd([cd] * 9, K0, params_all, g["mesh_vert"], nthreads=8)
    assert got.shape == (24856, 3)
    assert np.abs(got - g["warped_vert"]).max() < 1e-5


def test_ply_reader_reproduces_the_demo_mesh_numbers(golden, tmp_path):
    """meshio.read_ply_ascii against numbers captured from sim3_demo/*.ply (counts, bounding box, total area, checksums).
    The two demo meshes are kept xz-compressed under tests/golden/ and read back as the ASCII files they are."""
    import lzma
    import shutil
    from deformationpyramid_amd.meshio import read_ply_ascii
    g = golden("F13_shape_transfer")
    for tag, name in (("src", "AlienSoldier.ply"), ("tgt", "Ortiz.ply")):
        path = tmp_path / name
        with lzma.open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sim3_demo_" + name + ".xz")) as fin, open(path, "wb") as fout:
            shutil.copyfileobj(fin, fout)
        v, f = read_ply_ascii(str(path))
        assert [v.shape[0], f.shape[0]] == list(g[f"mesh.{tag}.counts"])
        np.testing.assert_array_equal(np.stack([v.min(0), v.max(0)]), g[f"mesh.{tag}.bbox"])
        a, b, c = (v[f[:, k]].astype(np.float64) for k in range(3))
        area = 0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum()
        assert abs(area - float(g[f"mesh.{tag}.area"])) < 1e-9 * area
        np.testing.assert_allclose(v.astype(np.float64).sum(0), g[f"mesh.{tag}.vsum"], rtol=1e-12)
        assert int(f.sum()) == int(g[f"mesh.{tag}.fsum"])


def test_torch_cpu_restatement_follows_the_reference_trace(golden):
    """oracle/ndp_torch_ref.py (the BLAS-backed baseline bench.py times beside the C port) against the reference's F4/F5
    loss traces at two levels, and against the C oracle's warp: the same algorithm, stated on plain torch ops."""
    from oracle import ndp_torch_ref as T
    g = golden("F4F5_iteration")
    for tag, lvl in (("se3aa.L0", 0), ("se3aa.L5", 5)):
        pyr = seeded_pyramid(int(g[f"{tag}.seed"]), **VARIANTS["se3aa"])
        d = pyr.descs[lvl]
        x, y = torch.from_numpy(g[f"{tag}.x"]), torch.from_numpy(g[f"{tag}.y"])
        p = T.split_level(pyr.store[lvl, :d.param_count])
        w0 = T.level_forward(p, x, lvl).detach().numpy()
        np.testing.assert_allclose(w0, g[f"{tag}.warp0"], rtol=0, atol=1e-6)
        np.testing.assert_allclose(w0, O.level_fwd(cdesc(d), pyr.store[lvl, :d.param_count].numpy(), lvl, K0, g[f"{tag}.x"]),
                                   rtol=0, atol=1e-6)
        opt = torch.optim.Adam(p, lr=0.01)
        losses = []
        for _ in range(20):
            loss = T.chamfer_l1(T.level_forward(p, x, lvl), y)
            losses.append(loss.item())
            opt.zero_grad(); loss.backward(); opt.step()
        ref = g[f"{tag}.losses"]
        assert abs(losses[0] - ref[0]) < 2e-6 * ref[0]
        assert np.abs(np.array(losses) - ref).max() < 1e-2 * ref.max()


# ------------------------------------------------------------------- F6/F7: early stop + end to end
def test_F6_stop_rule_replays_reference_iteration_counts(golden):
    """Feed the reference's own loss trace to the oracle's stop rule: the per-level evaluation
    counts must come out exactly (registration.py:226-232)."""
    for fx in ("F7_end_to_end", "F9b_lndp_end_to_end"):
        g = golden(fx)
        trace, counts = g["loss_trace"], g["iters_per_level"]
        pos = 0
        for c in counts:
            seg = trace[pos:pos + c]
            brk, _, _ = O.stop_trace(seg)
            if c < 500:
                assert brk == c - 1, (fx, brk, c)        # the breaking evaluation is the last one
            else:
                assert brk == c
            pos += c
        assert pos == len(trace)


def test_stop_rule_edges():
    assert O.stop_trace([5e-5])[0] == 0                           # loss < 1e-4 -> immediate break
    brk, bc, _ = O.stop_trace([1.0] * 40)
    assert brk == 15 and bc == 15                                 # first eval vs 1e6 is not "small"
    brk, bc, _ = O.stop_trace([1.0, 0.5] * 30)
    assert brk == 60 and bc == 0
    # the counter is cumulative, never reset by a good step
    seq = [1.0] + [1.0] * 7 + [0.5] + [0.5] * 8
    assert O.stop_trace(seq)[0] == len(seq) - 1


# ------------------------------------------------------------- F11: nonrigidity gate + BCE (w_reg > 0)
F11_VARIANTS = {"se3aa": VARIANTS["se3aa"], "sim3quat": VARIANTS["sim3quat"], "sflow": VARIANTS["sflow"]}


def _bce_zero_target(nr, w_reg):
    """value and d/dnr of w_reg * BCELoss(nr, 0) with torch's clamps (registration.py:216-220)."""
    nr = nr.astype(np.float32)
    l1 = np.maximum(np.log(np.float32(1.0) - nr), np.float32(-100.0))
    val = np.float32(w_reg) * np.float32((-l1).sum(dtype=np.float32) / np.float32(nr.size))
    den = np.maximum((np.float32(1.0) - nr) * nr, np.float32(1e-12))
    g = np.float32(w_reg) * (np.float32(1.0 / nr.size) * (nr / den))
    return val, g.astype(np.float32)


@pytest.mark.parametrize("tag", list(F11_VARIANTS))
def test_F11_gate_forward_and_grads(golden, tag):
    g = golden("F11_nonrigidity")
    pyr = seeded_pyramid(int(g["seed"]), m=6, nonrigidity_est=True, **F11_VARIANTS[tag])
    lvl = 4
    assert not pyr.descs[0].nonrigidity and pyr.descs[lvl].nonrigidity            # nets.py:26: no gate at level 0
    scale_heads(pyr, lvl, float(g["head_scale"]))
    assert abs(wsum(pyr, lvl) - float(g[f"{tag}.wsum"])) < 1e-6 * float(g[f"{tag}.wsum"])
    d = pyr.descs[lvl]
    params = pyr.store[lvl, :d.param_count].numpy()
    out, nr = O.level_fwd(cdesc(d), params, lvl, K0, g["x"], want_nonrig=True)
    np.testing.assert_allclose(out, g[f"{tag}.out"], rtol=0, atol=1e-5 if "quat" in tag else 2e-6)
    np.testing.assert_allclose(nr, g[f"{tag}.nonrig"], rtol=0, atol=1e-6)
    coef = torch.linspace(-1.0, 1.0, 256 * 3).reshape(256, 3).numpy()
    c2 = torch.linspace(0.5, -0.25, 256).numpy()
    grads = O.level_bwd(cdesc(d), params, lvl, K0, g["x"], coef, g_nr=c2)
    for name, off, shape in d.named_slices():
        ref = g[f"{tag}.grad.{name}"]
        got = grads[off:off + ref.size].reshape(ref.shape)
        assert rel_err(got, ref) < 1e-4, (tag, name, rel_err(got, ref))
    descs = [cdesc(x) for x in pyr.descs]
    params_all = np.concatenate([pyr.store[i, :x.param_count].numpy() for i, x in enumerate(pyr.descs)])
    full = O.pyramid_fwd(descs, K0, params_all, g["x"])
    np.testing.assert_allclose(full, g[f"{tag}.full_out"], rtol=0, atol=2e-5)


def test_F11_iterations_with_bce(golden):
    g = golden("F11_nonrigidity")
    pyr = seeded_pyramid(int(g["it.seed"]), m=4, nonrigidity_est=True, **VARIANTS["se3aa"])
    lvl, w_reg = 2, float(g["it.w_reg"])
    assert abs(wsum(pyr, lvl) - float(g["it.wsum"])) < 1e-6 * float(g["it.wsum"])
    d = pyr.descs[lvl]
    cd = cdesc(d)
    p = pyr.store[lvl, :d.param_count].numpy().copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    losses = []
    for it in range(12):
        w, nr = O.level_fwd(cd, p, lvl, K0, g["it.x"], want_nonrig=True)
        r = O.chamfer(w, g["it.y"])
        reg, gnr = _bce_zero_target(nr, w_reg)
        losses.append(float(np.float32(r["loss"]) + reg))
        grads = O.level_bwd(cd, p, lvl, K0, g["it.x"], r["gx"], g_nr=gnr)
        if it == 0:
            np.testing.assert_allclose(w, g["it.warp0"], rtol=0, atol=1e-6)
            np.testing.assert_allclose(nr, g["it.nonrig0"], rtol=0, atol=1e-6)
            for name, off, shape in d.named_slices():
                ref = g[f"it.grad0.{name}"]
                assert rel_err(grads[off:off + ref.size].reshape(ref.shape), ref) < 1e-4, name
        O.adam(p, grads, m, v, it + 1)
    ref = g["it.losses"]
    assert abs(losses[0] - ref[0]) < 2e-6 * ref[0]
    assert np.abs(np.array(losses) - ref).max() < 1e-2 * ref.max()


def test_F11_oracle_level_loop_matches_hand_rolled_bce(golden):
    """ndp_o_optimize with w_reg > 0 equals the step-by-step composition above (same C pieces)."""
    g = golden("F11_nonrigidity")
    pyr = seeded_pyramid(int(g["it.seed"]), m=3, nonrigidity_est=True, **VARIANTS["se3aa"])
    descs = [cdesc(x) for x in pyr.descs]
    params_all = np.concatenate([pyr.store[i, :x.param_count].numpy() for i, x in enumerate(pyr.descs)])
    r = O.optimize(descs, params_all, g["it.x"], 0, g["it.x"].shape[0], None, g["it.y"], iters=4, early_stop=False, w_reg=0.5)
    assert r["steps"] == 12 and list(r["iters_per_level"]) == [4, 4, 4]
    # level 0 carries no gate: its first loss is the plain Chamfer value
    w0 = O.level_fwd(descs[0], params_all[:pyr.descs[0].param_count], 0, K0, g["it.x"])
    assert abs(r["loss_trace"][0] - float(O.chamfer(w0, g["it.y"])["loss"])) < 1e-7
    # at level 1 the BCE term is present (loss > Chamfer alone)
    assert r["loss_trace"][4] > 0.5 * 0.6                        # w_reg * -log(1 - 0.5) = 0.35 at init, plus Chamfer


# ------------------------------------------------- F16: width / depth other than 128 / 3 (model/nets.py:65-110,295-304)
from tests._helpers import GENERIC_SHAPES, generic_pyramid


@pytest.mark.parametrize("tag", list(GENERIC_SHAPES))
def test_F16_generic_width_init_forward_grads_and_pyramid(golden, tag):
    """The init replay, the oracle's level forward / backward and its pyramid at other widths and depths, against the reference."""
    g = golden("F16_generic_width")
    pyr = generic_pyramid(int(g["seed"]), tag)
    names, sums, asums, heads = [], [], [], []
    for li, layer in enumerate(pyr.pyramid):
        for k, v in layer.named_parameters():
            a = v.detach().double().numpy().ravel()
            names.append(f"{li}.{k}")
            sums.append(a.sum())
            asums.append(np.abs(a).sum())
            h = np.zeros(8)
            h[:min(8, a.size)] = a[:8]
            heads.append(h)
    assert names == list(g[f"{tag}.names"])
    np.testing.assert_array_equal(np.array(heads), g[f"{tag}.head8"])          # bit-exact RNG replay at this width / depth
    np.testing.assert_allclose(np.array(sums), g[f"{tag}.sum"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(np.array(asums), g[f"{tag}.abssum"], rtol=1e-12)
    np.testing.assert_array_equal(torch.randperm(4096)[:16].numpy(), g[f"{tag}.perm4096"])
    lvl, x = int(g["level"]), g["x"]
    scale_heads(pyr, lvl, float(g["head_scale"]))
    d = pyr.descs[lvl]
    assert d.width == GENERIC_SHAPES[tag]["width"] and d.n_hidden == GENERIC_SHAPES[tag]["depth"] - 1
    params = pyr.store[lvl, :d.param_count].numpy()
    out = O.level_fwd(cdesc(d), params, lvl, K0, x)
    np.testing.assert_allclose(out, g[f"{tag}.out"], rtol=0, atol=1e-5 if "quat" in tag else 2e-6)
    coef = torch.linspace(-1.0, 1.0, x.shape[0] * 3).reshape(-1, 3).numpy()
    grads = O.level_bwd(cdesc(d), params, lvl, K0, x, coef)
    for name, off, shape in d.named_slices():
        ref = g[f"{tag}.grad.{name}"]
        got = grads[off:off + ref.size].reshape(ref.shape)
        assert rel_err(got, ref) < 1e-4, (tag, name, rel_err(got, ref))
    descs = [cdesc(dd) for dd in pyr.descs]
    params_all = np.concatenate([pyr.store[i, :dd.param_count].numpy() for i, dd in enumerate(pyr.descs)])
    full = O.pyramid_fwd(descs, K0, params_all, x)
    np.testing.assert_allclose(full, g[f"{tag}.full_out"], rtol=0, atol=2e-5 if "quat" in tag else 5e-6)


def test_F16_stop_rule_replays_the_reference_at_width_64(golden):
    g = golden("F16_generic_width")
    trace, counts = g["reg.loss_trace"], g["reg.iters_per_level"]
    pos = 0
    for c in counts:
        brk, _, _ = O.stop_trace(trace[pos:pos + c])
        assert brk == (c - 1 if c < 60 else c), (brk, c)
        pos += c
    assert pos == len(trace) and len(counts) == 5
