"""The loss stage's float64 reference (tests/_loss_ref.py) pinned without a GPU: against the CPU oracle's Chamfer and landmark terms,
the crafted-index builders' ranges, the early-stop restatement against the oracle's rule, and ndp_engine_load's refusal of a pair with
samples, a Chamfer weight and no target (the loss would be 0/0, and the stage's scatter had no target to bring its head rows in)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deformationpyramid_amd.layout import LayerDesc
from tests import _loss_ref as R
from tests import _tick_ref as TR

BAR = 2e-6                       # test_chamfer_loss_and_grad's, relative to the loss / to max |grad|


def O():
    from oracle import ndp_oracle
    return ndp_oracle


def _snap(K, S, T, trunc, w_cd, seed, motion="SE3", rotfmt="axis_angle"):
    """A stage input with real nearest neighbours: head outputs of O(0.01), the oracle's NN on the float32 warped samples."""
    d = LayerDesc(motion=motion, rotfmt=rotfmt)
    pts, lt, tgt = R.clouds(K, S, T, seed)
    g = torch.Generator().manual_seed(seed)
    heads = torch.zeros(K + S, 24)
    heads[:, :d.n_heads] = (torch.rand(K + S, d.n_heads, generator=g) - 0.5) * 0.04
    snap = SimpleNamespace(desc=d, level=0, K=K, S=S, T=T, w_cd=w_cd, trunc=trunc, w_reg=0.0, heads=heads, x_in=pts,
                           ldmk_t=lt, tgt=tgt, d2x=None, idx_x=None, d2y=None, idx_y=None)
    xw, _ = R.head_warp(d, heads[:, :d.n_heads].double(), pts.double())
    xw32 = xw.float().numpy()
    r = O().chamfer(xw32[K:], tgt.numpy(), trunc=trunc, want_grad=True)
    snap.d2x, snap.idx_x = torch.from_numpy(r["d2x"]), torch.from_numpy(r["idx_x"])
    snap.d2y, snap.idx_y = torch.from_numpy(r["d2y"]), torch.from_numpy(r["idx_y"])
    return snap, xw32, r


@pytest.mark.parametrize("trunc", [1e9, 0.004])
def test_reference_without_landmarks_is_the_oracles_chamfer(trunc):
    snap, xw32, r = _snap(0, 300, 333, trunc, 0.5, 1)          # (w_cd must NOT scale the term when K == 0)
    n_cut = int((r["d2x"] >= np.float32(trunc)).sum()) + int((r["d2y"] >= np.float32(trunc)).sum())
    assert (n_cut > 50) == (trunc < 1) and (r["d2x"] > 0).all() and (r["d2y"] > 0).all()
    ref = R.evaluate(snap)
    assert np.abs(ref.xw.numpy() - xw32).max() < 1e-7
    assert abs(ref.loss - float(r["loss"])) < BAR * float(r["loss"])
    assert np.abs(ref.gx.numpy() - r["gx"]).max() < BAR * np.abs(r["gx"]).max()
    f32 = R.evaluate(snap, torch.float32)                       # the yardstick evaluation is the same function
    assert abs(f32.loss - ref.loss) < BAR * ref.loss and (f32.dO.double() - ref.dO).abs().max() < 1e-5 * ref.dO.abs().max()


@pytest.mark.parametrize("trunc", [1e9, 0.004])
def test_reference_with_landmarks_is_landmark_plus_w_cd_chamfer(trunc):
    K, w_cd = 70, 0.5
    snap, xw32, r = _snap(K, 200, 230, trunc, w_cd, 2, motion="Sim3", rotfmt="euler")
    l_ld, g_ld = O().landmark(xw32[:K], snap.ldmk_t.numpy())
    want = float(l_ld) + w_cd * float(r["loss"])
    gx = np.concatenate([g_ld, w_cd * r["gx"]])
    ref = R.evaluate(snap)
    assert abs(ref.loss - want) < BAR * want
    assert np.abs(ref.gx.numpy() - gx).max() < BAR * np.abs(gx).max()
    assert np.abs(ref.gx.numpy()[:K] - g_ld).max() < BAR * np.abs(g_ld).max()          # (each part on its own scale, too)
    assert np.abs(ref.gx.numpy()[K:] - w_cd * r["gx"]).max() < BAR * np.abs(w_cd * r["gx"]).max()


def _layout_desc(tag):
    """The descriptor of a level that carries every row of the layout (a gated layout: a level >= 1)."""
    kw = TR.LAYOUTS[tag]
    return LayerDesc(motion=kw["motion"], rotfmt=kw["rotation_format"], nonrigidity=bool(kw.get("nonrigidity_est", False)))


def test_reference_head_backward_is_the_chain_rule_of_its_own_warp():
    """dO = mlp_scale J^T gx for every head layout the GPU cases use (finite differences of head_warp in float64), at head outputs of
    the size those cases see (5e-3).  The quaternion and 6D heads divide by norms of that size, so the warp's higher derivatives grow
    like norm^-k: the differences are the five-point stencil (error h^4 f^(5) / 30) at h = 3e-7 -- at 1e-6 the three-point stencil's
    own h^2 f''' / 6 is 1e-6 for these heads, a hundred times the bar."""
    for tag in TR.LAYOUTS:
        d = _layout_desc(tag)
        assert d.n_heads == TR.HEAD_ROWS[tag][1]
        g = torch.Generator().manual_seed(5)
        o = ((torch.rand(6, d.n_heads, generator=g) - 0.5) * 0.01).double()
        x = R.cloud(6, 9).double()
        gx = torch.rand(6, 3, generator=g).double()
        mg = TR.rotation_margins(d, o)
        assert all(v > 1.5e-3 for v in mg.values()), mg             # the stencil's error estimate above rests on it
        oo = o.clone().requires_grad_()
        (R.head_warp(d, oo, x)[0] * gx).sum().backward()
        f = lambda q: (R.head_warp(d, q, x)[0] * gx).sum(-1)
        h = 3e-7
        for j in range(d.n_heads):
            e = torch.zeros_like(o)
            e[:, j] = h
            fd = (-f(o + 2 * e) + 8 * f(o + e) - 8 * f(o - e) + f(o - 2 * e)) / (12 * h)
            assert (fd - oo.grad[:, j]).abs().max() < 1e-8, (tag, j, float((fd - oo.grad[:, j]).abs().max()))
            assert float(oo.grad[:, j].abs().max()) > 1e-3, (tag, j)              # every row of the layout moves the warp


@pytest.mark.parametrize("tag", list(TR.LAYOUTS))
def test_restated_warp_is_the_oracles_level_forward(tag):
    """head_warp on float64 head outputs (MLP + mlp_scale from the level's parameters) against the CPU oracle's level forward -- which is
    pinned to the reference's own outputs by fixtures F2 / F11 -- at test_level_fwd_matches_oracle's tolerances.  Levels 0, 1, 2 of a
    pyramid with the heads x 20: a gated layout's level 0 has no gate row."""
    pyr = TR.tick_pyramid(tag, 3)
    x = R.cloud(200, 17)
    tol = 1e-5 if ("6d" in tag or "quat" in tag) else 2e-6
    for level in (0, 1, 2):
        d = R.level_desc(pyr.descs[-1], level)
        assert d == pyr.descs[level]
        params = pyr.store[level, :d.param_count]
        xw, nr = R.head_warp(d, TR.level_heads(d, params, level, x), x.double())
        cd = O().make_desc(d.width, d.n_hidden, d.motion, d.rotfmt, d.nonrigidity, d.mlp_scale)
        ref, ref_nr = O().level_fwd(cd, params.numpy(), level, TR.K0, x.numpy(), want_nonrig=True)
        err = float(np.abs(xw.numpy() - ref).max())
        print(f"{tag} level {level}: |restated warp - oracle| = {err:.3e}, largest displacement {float((xw - x.double()).abs().max()):.3e}")
        assert err < tol, (tag, level, err)
        assert float((xw - x.double()).abs().max()) > 5e-4             # a warp that moves the points, not the identity
        assert (nr is not None) == (tag in TR.GATED and level > 0)
        if nr is not None:
            assert float(np.abs(nr.numpy() - ref_nr).max()) < 2e-6, (tag, level)


def test_crafted_indices_stay_inside_their_range():
    K, S, T = 70, 600, 2049
    gens = {
        "all_one:first": lambda: R.craft_all_one(K, S, T, 0),
        "all_one:thread255": lambda: R.craft_all_one(K, S, T, R.sample_of_point(K, S, 255)),
        "all_one:block1": lambda: R.craft_all_one(K, S, T, R.sample_of_point(K, S, 256)),
        "all_one:last": lambda: R.craft_all_one(K, S, T, S - 1),
        "alternate": lambda: R.craft_alternate(K, S, T, 3, R.sample_of_point(K, S, 300)),
        "block1": lambda: R.craft_block(K, S, T, 1),
        "block2": lambda: R.craft_block(K, S, T, 2),
        "permutation": lambda: R.craft_permutation(0, 512, 512, 7),
    }
    for name, gen in gens.items():
        idx = gen()
        s = 512 if name == "permutation" else S
        assert idx.dtype == torch.int32 and idx.numel() == (512 if name == "permutation" else T), name
        assert int(idx.min()) >= 0 and int(idx.max()) < s, name
    assert sorted(gens["permutation"]().tolist()) == list(range(512))
    b1 = gens["block1"]()
    assert int(b1.min()) + K == 256 and int(b1.max()) + K == 511 and len(set(b1.tolist())) == 256
    assert R.sample_of_point(K, S, 255) == 185 and R.sample_of_point(K, S, 256) == 186
    for bad in (lambda: R.craft_all_one(K, S, T, S), lambda: R.craft_all_one(K, S, T, -1), lambda: R.craft_alternate(K, S, T, 0, S),
                lambda: R.craft_block(K, S, T, 3), lambda: R.craft_permutation(0, 512, 511, 1), lambda: R.sample_of_point(K, S, 69),
                lambda: R.sample_of_point(K, S, K + S), lambda: R.checked(np.zeros(5, np.int64), 4, 6)):
        with pytest.raises(ValueError):
            bad()


def test_next_state_follows_the_oracles_stop_rule():
    """The restated early stop against the oracle's (ndp_o_stop_check) on loss sequences that end each way."""
    cfg = SimpleNamespace(m=3, iters=6, early_stop=True, max_break_count=2, break_threshold_ratio=0.01)
    for losses in ([1.0, 0.5, 0.4999, 0.3, 0.2999, 0.2998], [1.0, 0.9999, 0.9998, 0.5], [1.0, 5e-5, 1.0], [1.0, 0.8, 0.6, 0.4, 0.3, 0.2, 0.1]):
        losses = [float(np.float32(v)) for v in losses]         # the stage's loss is a float32
        st = SimpleNamespace(level=1, iter=0, break_counter=0, adam_t=0, cur=1, total_steps=4, total_evals=5, loss_prev=1e6,
                             evals_per_level=[5, 0, 0] + [0] * 13, step_level=0, step_t=0, loss=0.0, decision=0)
        end, bc, lp = O().stop_trace(losses, cfg.max_break_count, cfg.break_threshold_ratio)
        for i, L in enumerate(losses):
            nxt = R.next_state(st, L, cfg)
            if nxt["decision"] != R.DEC_STEP:
                break
            assert nxt["iter"] == i + 1 and nxt["total_steps"] == 4 + i + 1 and nxt["level"] == 1
            st = SimpleNamespace(**dict(nxt, step_level=1, step_t=0, loss=L))
        if end < len(losses) and end < cfg.iters:               # the oracle's rule broke the level at evaluation `end`: no step there
            assert i == end and nxt["decision"] == R.DEC_ADVANCE and nxt["total_steps"] == 4 + end
            assert st.loss_prev == lp and (losses[end] < 1e-4 or (bc == cfg.max_break_count and st.break_counter == bc - 1))
        else:
            assert i == cfg.iters - 1 and nxt["decision"] == R.DEC_STEP_ADVANCE and nxt["total_steps"] == 4 + cfg.iters
        assert nxt["level"] == 2 and nxt["iter"] == 0 and nxt["break_counter"] == 0 and nxt["loss_prev"] == 1e6 and nxt["cur"] == 0
        assert nxt["evals_per_level"][1] == i + 1 and nxt["total_evals"] == 5 + i + 1
    idle = R.next_state(SimpleNamespace(level=3, iter=0, break_counter=0, adam_t=0, cur=1, total_steps=9, total_evals=9, loss_prev=1e6,
                                        evals_per_level=[3] * 16, step_level=2, step_t=3, loss=0.25, decision=2), 0.0, cfg)
    assert idle["decision"] == R.DEC_IDLE and idle["level"] == 3 and idle["total_evals"] == 9 and idle["loss"] == 0.25


def _fake_engine(N, desc, w_cd, n_cap=512, t_cap=512, B=2):
    """An engine descriptor whose buffers are made-up addresses (non-null, aligned): every refusal below happens before any launch."""
    e = N.Engine()
    e.desc = desc.c_struct()
    e.m, e.k0, e.P, e.p_stride = 3, -8, desc.param_count, (desc.param_count + 63) // 64 * 64
    e.iters, e.max_break_count, e.early_stop = 5, 2, 1
    e.B, e.G, e.n_cap, e.t_cap = B, 1, n_cap, t_cap
    e.break_threshold_ratio, e.w_cd, e.trunc = 0.01, w_cd, 1e9
    for name in ("geom", "state", "pts", "ldmk_t", "tgt", "params", "gpart", "adam_m", "adam_v", "act", "heads", "d2x", "idx_x", "d2y",
                 "idx_y", "adam_tab", "dO", "nn_row", "gmax"):
        setattr(e, name, 4096)
    return e


def test_engine_load_refuses_samples_without_targets_under_a_chamfer_term():
    from deformationpyramid_amd import _native as N
    L = N.lib()
    e = _fake_engine(N, LayerDesc(), 0.5)

    def load(**kw):
        job = N.LoadJob()
        job.slot, job.params, job.src, job.tgt, job.ldmk_s, job.ldmk_t = 0, 4096, 4096, 4096, 4096, 4096
        for k, v in kw.items():
            setattr(job, k, v)
        arr = (N.LoadJob * 2)(N.LoadJob(), job)                  # (a park job in front: the refusal covers the whole group)
        arr[0].slot = 1
        return L.ndp_engine_load(ctypes.byref(e), 0, arr, 2, None)

    for K in (0, 40):
        assert load(K=K, S=100, T=0) == -1
        msg = L.ndp_last_error()
        assert b"ndp_engine_load" in msg and b"S > 0, T == 0" in msg and b"w_cd" in msg, msg
    e.w_cd = -0.25                                               # any non-zero weight switches the Chamfer term on
    assert load(K=0, S=1, T=0) == -1 and b"T == 0" in L.ndp_last_error()
    # the older refusals still come first and keep their messages
    e.w_cd = 0.5
    assert load(K=0, S=600, T=0) == -1 and b"capacities" in L.ndp_last_error()
    assert load(K=0, S=100, T=0, src=None) == -1 and b"null cloud pointer" in L.ndp_last_error()
    assert load(K=0, S=100, T=0, params=4100) == -1 and b"16-byte" in L.ndp_last_error()
    assert N.lib().ndp_version() >= 207                          # nothing in the ABI moved for it
