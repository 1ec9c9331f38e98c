"""The tick's loss stage (k_eng_loss) on its own, against float64 autograd of the same inputs.

The stage computes the loss, takes the early-stop / hand-over decision, turns dL/dx' (own nearest-neighbour term + an LDS counting-sort
scatter of the targets that chose each source) into dO through the head backward, and leaves the pair's max |dO| in gmax.  Every case
below runs stages 0-1 of a tick, optionally overwrites the stage's INPUTS in the engine's own tensors (crafted nearest-source
assignments, pair-state fields), fills dO with NaN, snapshots every input, runs stage 2 alone and holds what it wrote against
tests/_loss_ref.py evaluated on the snapshot:

  (a) dO rows < n against the reference, columns nh..15 exactly 0;      (b) rows n .. end of the last live 256-point block exactly 0,
  nothing of another slot's dO touched;      (c) gmax bit-equal to max |dO| of what was written;      (d) the loss;      (e) every
  field of the next pair state against registration.py:226-249 restated in Python.

Head layouts: the reference restates all four rotation formats (axis-angle, Euler, quaternion, 6D) under SE3 and Sim3, scene flow, and
the nonrigidity gate behind any of them; test_head_variants and test_gated_engine run every layout of tests/_tick_ref.py's table, 3 to 11
head rows.  Every other case runs se3aa.

The bar has no constant: the SAME reference evaluated in float32 on the CPU is the yardstick of each case and tensor; the kernel's max
error must stay within 4 yardsticks (floor 2^-22 max|ref|: a float32 run can happen to be exact).  No point is excluded anywhere.
Measured figures of every case: build/reports/loss_stage_errors.json and .txt (untracked; a copy of the table is kept as
profiles/loss_stage_f64_errors.txt).

Out of scope (asserted not to occur): a source exactly on its nearest target (d2 == 0 -> 0 * inf, in the reference's autograd too).
"""
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deformationpyramid_amd._native import DEC_ADVANCE, DEC_IDLE, DEC_STEP, DEC_STEP_ADVANCE          # (loads no library)
from tests import _loss_ref as R
from tests import _tick_ref as TR
from tests._helpers import VARIANTS, engine_modes, scale_heads, seeded_pyramid

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEAD_SCALE = 20.0                 # head outputs of O(0.01): rotations, scales and gates that matter
FACTOR = 4.0
STATE_FIELDS = ("level", "iter", "break_counter", "adam_t", "cur", "decision", "total_steps", "total_evals", "step_level", "step_t",
                "loss_prev")
_REPORT = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


def _write_report():
    out_dir = os.path.join(ROOT, "build", "reports")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "loss_stage_errors.json"), "w") as f:
        json.dump(_REPORT, f, indent=1, sort_keys=True)
    with open(os.path.join(out_dir, "loss_stage_errors.txt"), "w") as f:
        f.write("k_eng_loss against float64 autograd of its own inputs (tests/test_loss_stage.py); yardstick = the same reference in\n"
                "float32 on the CPU; allowed = max(4 yardsticks, 2^-22 max|ref|); ratio = err / (allowed / 4), the bar is ratio <= 4\n\n")
        f.write(f"{'case':<58}{'K':>5}{'S':>5}{'T':>6}  {'tensor':<5}{'kernel err':>12}{'yardstick':>12}{'floor':>12}{'ratio':>8}\n")
        for case in sorted(_REPORT):
            for r in _REPORT[case]:
                for what in ("dO", "loss"):
                    q = r[what]
                    f.write(f"{case + ' [' + str(r['slot']) + ']':<58}{r['K']:>5}{r['S']:>5}{r['T']:>6}  {what:<5}{q['err']:>12.3e}"
                            f"{q['yardstick']:>12.3e}{q['floor']:>12.3e}{q['ratio']:>8.2f}\n")


# ------------------------------------------------------------------------------------------------ the harness
def _pyramid(variant, gated, m, seed):
    """variant: a tag of VARIANTS, or one of the layout table's (tests/_tick_ref.py: LAYOUTS) that VARIANTS does not have; the gate comes
    from `gated` alone."""
    kw = VARIANTS[variant] if variant in VARIANTS else {k: v for k, v in TR.LAYOUTS[variant].items() if k != "nonrigidity_est"}
    pyr = seeded_pyramid(seed, m=m, nonrigidity_est=True, **kw) if gated else seeded_pyramid(seed, m=m, **kw)
    for lvl in range(m):
        scale_heads(pyr, lvl, HEAD_SCALE)
    return pyr


def _state(eng, parity, b):
    from deformationpyramid_amd import _native as N
    return N.PairState.from_buffer_copy(eng.state[parity, b].cpu().numpy().tobytes())


def _put_state(eng, parity, b, st):
    eng.state[parity, b].copy_(torch.frombuffer(bytearray(bytes(st)), dtype=torch.uint8).to(eng.device))


def run_stage(dev, case, pairs, *, variant="se3aa", gated=False, level=0, m=None, B=None, cfg=None, eng_kw=None, n_cap=None, t_cap=None,
              craft=None, state_edit=None, ldmk_from_warp=False, finished=None, folded=False, seed=0):
    """One engine, the pairs {slot: (K, S, T)} loaded (every other slot parked), brought to `level` by whole ticks, stages 0-1 run,
    inputs overwritten as asked, stage 2 run alone and EVERYTHING it wrote checked; -> {slot: SimpleNamespace of what was seen}.
      craft(slot, K, S, T) -> int32 [T] nearest-source assignment (rows final: nn_mode 1) | None
      state_edit(slot, PairState) edits the current record in place
      ldmk_from_warp: after stage 0 the landmark targets become the warped landmarks themselves
      finished: (slot, (K, S, T)) a pair that runs to its end before the others are loaded
      folded: the stage itself folds the one-pass kernels' row partials and stores d2x / idx_x"""
    from deformationpyramid_amd import ops
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    m = m or max(level + 1, 2 if gated else 1)
    kw = dict(m=m, iters=1 if level > 0 else 3, early_stop=False, w_cd=0.5, trunc=1e9)
    kw.update(cfg or {})
    assert level == 0 or kw["iters"] == 1                         # whole ticks bring a pair to its level: one iteration per level
    cfg = OptConfig(**kw)
    pyr = _pyramid(variant, gated, m, 11 + seed)
    desc = pyr.descs[m - 1]
    B = B or max(pairs) + 1
    everyone = dict(pairs)
    if finished:
        everyone[finished[0]] = finished[1]
    n_cap = n_cap or max(K + S for K, S, _ in everyone.values())
    t_cap = t_cap or max(T for _, _, T in everyone.values())
    eng = BatchedEngine(desc, cfg, B, n_cap=n_cap, t_cap=t_cap, device=dev, **(eng_kw or {}))
    eng.park_all()
    held = {}

    def load(slot, shape, k):
        K, S, T = shape
        pts, lt, tgt = R.clouds(K, S, T, seed + 7 * k)
        eng.load(slot, pts, K, S, lt, tgt, pyr.store)
        held[slot] = eng._keep

    if finished:
        load(finished[0], finished[1], 50)
        eng.run_ticks(m * cfg.iters)
        assert _state(eng, eng.tick & 1, finished[0]).level == m
    for k, (slot, shape) in enumerate(sorted(pairs.items())):
        load(slot, shape, k)
    if level:
        eng.run_ticks(level)
    par = eng.tick & 1
    eng.run_stages(0, 0)
    if ldmk_from_warp:
        for slot, (K, S, T) in pairs.items():
            cur = _state(eng, par, slot).cur
            eng.ldmk_t[slot, :K].copy_(eng.pts[slot, cur ^ 1, :K])
    eng.run_stages(1, 1)
    torch.cuda.synchronize()
    for slot, (K, S, T) in pairs.items():
        st = _state(eng, par, slot)
        assert st.level == level, (slot, st.level)
        if craft is not None and craft(slot, K, S, T) is not None:
            assert eng.nn_mode == 1 and not eng.nn_cells          # final rows: nothing folds over what is written here
            idx = R.checked(craft(slot, K, S, T).numpy(), S, T)   # inside [0, S): the kernel dereferences it
            xs = eng.pts[slot, st.cur ^ 1, K:K + S].cpu()
            eng.idx_y[slot, :T].copy_(idx.to(dev))
            eng.d2y[slot, :T].copy_(R.crafted_d2y(xs, eng.tgt[slot, :T].cpu(), idx).to(dev))
        if state_edit is not None:
            state_edit(slot, st)
            _put_state(eng, par, slot, st)
    eng.dO.fill_(float("nan"))
    names = ("pts", "heads", "ldmk_t", "tgt", "d2x", "idx_x", "d2y", "idx_y", "geom")
    before = {k: getattr(eng, k).clone() for k in names}
    before["state"] = eng.state[par].clone()
    eng.run_stages(2, 2)
    torch.cuda.synchronize()
    for k in names:                                               # the stage's inputs are inputs
        if not (folded and k in ("d2x", "idx_x")):
            assert torch.equal(before[k].view(torch.int32), getattr(eng, k).view(torch.int32)), (case, k)
    assert torch.equal(before["state"], eng.state[par]), case
    dO, gmax = eng.dO.cpu(), eng.gmax.view(torch.float32).cpu()
    rows = {k: (getattr(eng, k) if folded and k in ("d2x", "idx_x") else before[k]).cpu() for k in names}
    seen, report = {}, []
    for slot in range(B):
        st, nst = _state(eng, par, slot), _state(eng, par ^ 1, slot)
        K, S, T = (int(v) for v in rows["geom"][slot, :3]) if slot in everyone else (0, 0, 0)
        if slot in everyone:
            assert (K, S, T) == tuple(everyone[slot])
        want = R.next_state(st, nst.loss, cfg)
        if st.level >= m:                                         # parked / finished: dO untouched, the record copied with IDLE
            assert slot not in pairs and torch.isnan(dO[slot]).all(), (case, slot)
            assert nst.decision == DEC_IDLE and want["decision"] == DEC_IDLE
            a, b = bytearray(bytes(st)), bytearray(bytes(nst))
            a[type(st).decision.offset:type(st).decision.offset + 4] = b[type(st).decision.offset:type(st).decision.offset + 4]
            assert a == b, (case, slot)
            continue
        d = R.level_desc(desc, level)
        n, nh = K + S, d.n_heads
        snap = SimpleNamespace(desc=desc, level=level, K=K, S=S, T=T, w_cd=eng.c_engine.w_cd, trunc=eng.c_engine.trunc,
                               w_reg=eng.c_engine.w_reg, heads=rows["heads"][slot], x_in=rows["pts"][slot, st.cur],
                               ldmk_t=rows["ldmk_t"][slot], tgt=rows["tgt"][slot], d2x=rows["d2x"][slot], idx_x=rows["idx_x"][slot],
                               d2y=rows["d2y"][slot], idx_y=rows["idx_y"][slot])
        if S > 0 and T > 0 and cfg.w_cd != 0:
            assert (snap.d2x[:S] > 0).all() and (snap.d2y[:T] > 0).all(), (case, slot)          # out of scope: a source ON its target
        r64, r32 = R.evaluate(snap), R.evaluate(snap, torch.float32)
        # the restated warp against the forward's own output, before anything rests on it
        x_in = snap.x_in[:n].double()
        extent = float((x_in.max(0).values - x_in.min(0).values).max())
        fwd = rows["pts"][slot, st.cur ^ 1, :n].double()
        assert float((r64.xw - fwd).abs().max()) <= 1e-6 * extent, (case, slot, float((r64.xw - fwd).abs().max()), extent)
        if folded:                                                # the rows the stage folded and stored, bit for bit
            xs = eng.pts[slot, st.cur ^ 1, K:n].contiguous()
            d2x, ix, d2y, iy = ops.chamfer_nn(xs, eng.tgt[slot, :T].contiguous())
            assert torch.equal(d2x.cpu().view(torch.int32), snap.d2x[:S].view(torch.int32)) and torch.equal(ix.cpu(), snap.idx_x[:S])
            assert torch.equal(d2y.cpu().view(torch.int32), snap.d2y[:T].view(torch.int32)) and torch.equal(iy.cpu(), snap.idx_y[:T])
        end = min((n + 255) // 256 * 256, eng.n_cap)
        got = dO[slot]
        q_dO = R.bar(got[:n, :nh], r64.dO, r32.dO, FACTOR)
        q_L = R.bar(torch.tensor([nst.loss]), torch.tensor([r64.loss]), torch.tensor([r32.loss]), FACTOR)
        report.append(dict(slot=slot, K=K, S=S, T=T, level=level, dO=q_dO, loss=q_L, loss_kernel=nst.loss, loss_f64=r64.loss))
        print(f"{case} slot {slot} (K, S, T) = {(K, S, T)}: dO err {q_dO['err']:.3e} yardstick {q_dO['yardstick']:.3e} ratio "
              f"{q_dO['ratio']:.2f} | loss {nst.loss:.9g} f64 {r64.loss:.12g} err {q_L['err']:.3e} yardstick {q_L['yardstick']:.3e} "
              f"ratio {q_L['ratio']:.2f}")
        seen[slot] = SimpleNamespace(st=st, nst=nst, dO=got, gmax=float(gmax[slot]), r64=r64, r32=r32, snap=snap, q_dO=q_dO, q_L=q_L,
                                     K=K, S=S, T=T, n=n, nh=nh, want=want, eng=eng)
    _REPORT[case] = report
    _write_report()
    for slot, s in seen.items():
        n, nh, got = s.n, s.nh, s.dO
        end = min((n + 255) // 256 * 256, eng.n_cap)
        assert torch.isfinite(got[:end]).all(), (case, slot)
        assert s.q_dO["err"] <= s.q_dO["allowed"], (case, slot, "dO", s.q_dO)                                   # (a)
        assert (got[:n, nh:] == 0).all(), (case, slot)
        assert (got[n:end] == 0).all(), (case, slot)                                                          # (b)
        assert np.float32(s.gmax).tobytes() == np.float32(float(got[:end].abs().max())).tobytes(), (case, slot, s.gmax)   # (c)
        assert s.q_L["err"] <= s.q_L["allowed"], (case, slot, "loss", s.q_L)                                    # (d)
        for f in STATE_FIELDS:                                                                                # (e)
            assert getattr(s.nst, f) == s.want[f], (case, slot, f, getattr(s.nst, f), s.want[f])
        assert list(s.nst.evals_per_level) == s.want["evals_per_level"], (case, slot)
    for slot in range(B):                                         # nothing of a slot without a live pair was written
        if slot not in seen:
            assert torch.isnan(dO[slot]).all(), (case, slot)
    return seen


def _nn_kw(arith, nn):
    """BatchedEngine arguments of (arithmetic, way the rows reach the stage) -> (kwargs, does the stage fold the rows itself)."""
    if nn == "cells":
        return dict(engine_modes(arith, None, nn_mode=1), nn_mode=None, nn_cells=True), False
    mode = {"nn0": 0, "nn1": 1, "nn2": 2}[nn]
    return dict(engine_modes(arith, None, nn_mode=mode), nn_cells=False), mode != 1


LAT = dict(nn_mode=1, nn_cells=False)            # final rows in d2x / idx_x (what every crafted case needs)


# ------------------------------------------------------------------------------------------------ natural cases
@pytest.mark.parametrize("nn", ["nn0", "nn2", "nn1", "cells"])
def test_every_way_the_rows_reach_the_stage(dev, arith, nn):
    kw, folded = _nn_kw(arith, nn)
    seen = run_stage(dev, f"rows/{nn}/{arith}", {0: (0, 300, 333)}, eng_kw=kw, folded=folded, cfg=dict(w_cd=0.5))
    eng = seen[0].eng
    assert bool(eng.nn_cells) == (nn == "cells") and (nn == "cells" or eng.nn_mode == int(nn[2]))
    assert seen[0].nst.decision == DEC_STEP and seen[0].gmax > 0


@pytest.mark.parametrize("shape,w_cd", [((70, 200, 233), 0.5), ((256, 100, 133), 0.5), ((300, 250, 283), 0.5), ((150, 0, 0), 0.0)],
                         ids=["K70_S200", "K256_S100", "K300_S250", "K150_only"])
def test_landmark_and_sample_layouts(dev, shape, w_cd):
    """One straddling block | a block of landmarks only and the first sample on thread 0 of the next | i_lo > 0 with the straddle in
    block 1 | landmarks alone."""
    seen = run_stage(dev, f"layout/K{shape[0]}_S{shape[1]}", {0: shape}, cfg=dict(w_cd=w_cd), eng_kw=dict(gemm_mode=0, **LAT), t_cap=320)
    assert seen[0].r64.loss > 1e-4 and seen[0].gmax > 0


@pytest.mark.parametrize("T", [2048, 2049, 4100])
def test_targets_across_the_scatter_chunk(dev, T):
    """LG_CHUNK = 2048 targets per pass of the counting sort: exactly one pass, one pass + 1 target, three passes (the last of 4)."""
    seen = run_stage(dev, f"chunk/T{T}", {0: (0, 300, T)}, eng_kw=dict(gemm_mode=0), t_cap=T + 64)
    assert seen[0].eng.nn_mode == 1 and seen[0].eng.t_cap > 2048 and not seen[0].eng.nn_cells


@pytest.mark.parametrize("which", ["d2y", "d2x"])
def test_truncation_exactly_on_a_stored_distance(dev, which):
    """trunc = the median stored distance of a first run of the same pair: that element and every larger one contribute nothing, the
    next smaller one does (`>=`, not `>`)."""
    shape, kw = {0: (0, 300, 333)}, dict(gemm_mode=0, **LAT)
    first = run_stage(dev, f"trunc/{which}/first", shape, eng_kw=kw)[0]
    vals = getattr(first.snap, which)[:300 if which == "d2x" else 333]
    trunc = float(vals.sort().values[vals.numel() // 2])
    s = run_stage(dev, f"trunc/{which}/median", shape, eng_kw=kw, cfg=dict(trunc=trunc))[0]
    vals2 = getattr(s.snap, which)[:vals.numel()]
    assert torch.equal(vals2, vals) and np.float32(s.eng.c_engine.trunc) == np.float32(trunc)
    assert int((vals2 == trunc).sum()) >= 1 and int((vals2 < trunc).sum()) == vals.numel() // 2
    # the element ON the bound is worth far more than the bar: with `>` in the kernel the loss alone would move by sqrt(trunc) / n
    assert float(np.sqrt(trunc)) / vals.numel() > 100 * s.q_L["allowed"] and s.r64.loss < first.r64.loss


def test_truncation_below_every_distance_leaves_the_landmarks_alone(dev):
    s = run_stage(dev, "trunc/all", {0: (70, 200, 233)}, eng_kw=dict(gemm_mode=0, **LAT), cfg=dict(trunc=1e-12))[0]
    assert (s.snap.d2x[:200] >= 1e-12).all() and (s.snap.d2y[:233] >= 1e-12).all()
    assert s.n == 270 and (s.dO[70:270] == 0).all() and s.dO[:70].abs().max() > 0 and s.gmax > 0
    lt = s.snap.ldmk_t[:70].double()
    assert abs(s.r64.loss - float(((s.r64.xw[:70] - lt) ** 2).sum(-1).mean())) == 0


def _assert_margins(s, d):
    """The quaternion and 6D heads of the case are far from their clamps (1e-12 in the kernel) and from 0 / 0; no axis-angle rotation
    vector is near theta = 0 -- on the head outputs the forward kernel wrote (tests/test_tick_layouts_cpu.py: the same on the CPU)."""
    mg = TR.rotation_margins(d, s.snap.heads[:s.n, :s.nh])
    for k, v in mg.items():
        assert v >= (1e-6 if k == "aa_norm" else 5e-4), (k, v)


@pytest.mark.parametrize("variant", ["sim3eu", "sflow"] + [t for t in TR.UNGATED if t not in ("sim3eu", "sflow")])
def test_head_variants(dev, variant):
    """Every ungated layout of the table, 3 to 10 head rows: the row offsets of head_warp_bwd (scale, translation) behind 3, 4 and 6
    rotation rows, and the 6D backward, which reads the raw rotation outputs out of the row it then overwrites with their gradient."""
    s = run_stage(dev, f"variant/{variant}", {0: (40, 300, 333)}, variant=variant, eng_kw=dict(gemm_mode=0, **LAT))[0]
    assert s.nh == TR.HEAD_ROWS[variant][0]
    d = R.level_desc(s.snap.desc, 0)
    _assert_margins(s, d)
    for j in range(s.nh):                                        # no row of the layout is without a gradient
        assert float(s.r64.dO[:, j].abs().max()) > 0, (variant, j)


@pytest.mark.parametrize("tag,level", [pytest.param("se3aa", 1, id="1"), pytest.param("se3aa", 0, id="0")]
                         + [pytest.param(t, lvl, id=f"{t}-{lvl}") for t in TR.GATED for lvl in (1, 0)])
def test_gated_engine(dev, tag, level):
    """A layout with the nonrigidity gate, w_reg > 0: level 1 carries the BCE value and g_nr, level 0 of the same engine carries no gate
    -- the shorter layout next to a parameter block sized for the longer one.  se3aa (7 | 6 head rows) and the table's gated layouts:
    the gate row behind a lone translation (4 | 3), behind a quaternion (8 | 7), and behind 6D rows, a Sim3 scale row and the
    translation (11 | 10)."""
    variant = tag[:-3] if tag.endswith("_nr") else tag
    s = run_stage(dev, f"gated/level{level}" if tag == "se3aa" else f"gated/{tag}/level{level}", {0: (40, 300, 333)}, variant=variant,
                  gated=True, level=level, m=2, cfg=dict(w_reg=0.5, iters=1), eng_kw=dict(gemm_mode=0, **LAT))[0]
    d = R.level_desc(s.snap.desc, level)
    rows = (6, 7) if tag == "se3aa" else TR.HEAD_ROWS[tag]
    assert s.snap.desc.nonrigidity and s.eng.c_engine.w_reg == 0.5 and s.nh == rows[1 if level else 0] == d.n_heads
    _assert_margins(s, d)
    plain = R.evaluate(SimpleNamespace(**dict(vars(s.snap), w_reg=0.0)))
    if level:
        assert d.row_nr == s.nh - 1
        assert s.r64.loss - plain.loss > 0.1 and s.dO[:340, d.row_nr].abs().max() > 0    # ~ 0.5 * log 2, and a gradient on the gate row
    else:
        assert s.r64.loss == plain.loss and s.st.cur == 0
    assert s.nst.decision == DEC_STEP_ADVANCE


def test_nine_slots_with_a_parked_and_a_finished_one(dev):
    """A full XCD group of eight plus a remainder slot (both branches of xcd_pair_block), every pair of another size."""
    pairs = {0: (0, 300, 333), 1: (70, 200, 233), 2: (256, 100, 133), 4: (0, 65, 63), 6: (300, 212, 283), 7: (20, 0, 0), 8: (7, 120, 130)}
    seen = run_stage(dev, "placement/B9", pairs, B=9, m=1, cfg=dict(iters=1), finished=(5, (30, 100, 90)), n_cap=512, t_cap=512,
                     eng_kw=dict(gemm_mode=0))
    assert sorted(seen) == sorted(pairs) and seen[0].eng.B == 9
    for s in seen.values():
        assert s.nst.decision == DEC_STEP_ADVANCE and s.nst.level == 1


def test_one_slot(dev):
    run_stage(dev, "placement/B1", {0: (70, 200, 233)}, B=1, eng_kw=dict(gemm_mode=0))


# ------------------------------------------------------------------------------------------------ crafted assignments
CRAFT_K, CRAFT_S, CRAFT_T = 70, 600, 2049


@pytest.mark.parametrize("where", ["first", "thread255", "block1", "last"])
def test_all_targets_name_one_source(dev, where):
    """A bucket of 2048 in the first pass + 1 in the second, the insertion sort's long path, 2049 fused adds in ascending order; the
    named sample at thread 70 of block 0 (the first one), thread 255 of block 0, thread 0 of block 1, and the last one."""
    K, S, T = CRAFT_K, CRAFT_S, CRAFT_T
    i = {"first": 0, "thread255": R.sample_of_point(K, S, 255), "block1": R.sample_of_point(K, S, 256), "last": S - 1}[where]
    s = run_stage(dev, f"craft/one/{where}", {0: (K, S, T)}, eng_kw=dict(gemm_mode=0, **LAT), t_cap=T + 64,
                  craft=lambda slot, K, S, T: R.craft_all_one(K, S, T, i))[0]
    assert (s.snap.idx_y[:T] == i).all()
    assert s.dO[K + i].abs().max() == s.dO[K:K + S].abs().max()           # the one row that collects every target


def test_targets_alternate_between_two_blocks(dev):
    K, S, T = CRAFT_K, CRAFT_S, CRAFT_T
    run_stage(dev, "craft/alternate", {0: (K, S, T)}, eng_kw=dict(gemm_mode=0, **LAT), t_cap=T + 64,
              craft=lambda slot, K, S, T: R.craft_alternate(K, S, T, 3, R.sample_of_point(K, S, 300)))


def test_only_sources_of_block_one_are_named(dev):
    K, S, T = CRAFT_K, CRAFT_S, CRAFT_T
    s = run_stage(dev, "craft/block1", {0: (K, S, T)}, eng_kw=dict(gemm_mode=0, **LAT), t_cap=T + 64,
                  craft=lambda slot, K, S, T: R.craft_block(K, S, T, 1))[0]
    assert int(s.snap.idx_y[:T].min()) + K == 256 and int(s.snap.idx_y[:T].max()) + K == 511


def test_every_source_is_named_once(dev):
    s = run_stage(dev, "craft/permutation", {0: (0, 512, 512)}, eng_kw=dict(gemm_mode=0, **LAT),
                  craft=lambda slot, K, S, T: R.craft_permutation(K, S, T, 7))[0]
    assert sorted(s.snap.idx_y[:512].tolist()) == list(range(512))


# ------------------------------------------------------------------------------------------------ the state machine
STOP = dict(iters=6, early_stop=True, max_break_count=3, break_threshold_ratio=0.001)


def _edit(**fields):
    def edit(slot, st):
        for k, v in fields.items():
            setattr(st, k, v)
    return edit


def test_last_iteration_steps_and_hands_over(dev):
    s = run_stage(dev, "state/step_advance", {0: (0, 300, 333)}, m=2, cfg=STOP, eng_kw=dict(gemm_mode=0),
                  state_edit=_edit(iter=5, adam_t=5, break_counter=1, loss_prev=123.0, total_steps=5, total_evals=5))[0]
    n = s.nst
    assert (n.decision, n.level, n.iter, n.adam_t, n.break_counter, n.loss_prev) == (DEC_STEP_ADVANCE, 1, 0, 0, 0, 1e6)
    assert n.cur == s.st.cur ^ 1 and n.evals_per_level[0] == 6 and n.total_steps == 6 and n.total_evals == 6
    assert (n.step_level, n.step_t) == (0, 6)


def test_break_counter_reaching_its_limit_advances_without_a_step(dev):
    first = run_stage(dev, "state/first", {0: (0, 300, 333)}, m=2, cfg=STOP, eng_kw=dict(gemm_mode=0))[0]
    assert first.nst.decision == DEC_STEP and first.nst.loss_prev == first.nst.loss and first.nst.break_counter == 0
    s = run_stage(dev, "state/advance", {0: (0, 300, 333)}, m=2, cfg=STOP, eng_kw=dict(gemm_mode=0),
                  state_edit=_edit(iter=2, adam_t=2, break_counter=2, loss_prev=float(first.nst.loss), total_steps=2, total_evals=2))[0]
    n = s.nst
    assert n.loss == first.nst.loss
    assert (n.decision, n.level, n.iter, n.adam_t, n.break_counter, n.loss_prev) == (DEC_ADVANCE, 1, 0, 0, 0, 1e6)
    assert n.total_steps == 2 and n.total_evals == 3 and n.evals_per_level[0] == 3 and n.cur == s.st.cur ^ 1


def test_a_moving_loss_steps_and_keeps_the_break_counter(dev):
    s = run_stage(dev, "state/step", {0: (0, 300, 333)}, m=2, cfg=STOP, eng_kw=dict(gemm_mode=0),
                  state_edit=_edit(iter=2, adam_t=2, break_counter=2, loss_prev=50.0, total_steps=2, total_evals=2))[0]
    n = s.nst
    assert (n.decision, n.level, n.iter, n.adam_t, n.break_counter) == (DEC_STEP, 0, 3, 3, 2)
    assert n.loss_prev == float(n.loss) and n.total_steps == 3 and n.cur == s.st.cur and n.evals_per_level[0] == 0


def test_landmarks_already_on_their_targets(dev):
    s = run_stage(dev, "state/zero_loss", {0: (150, 0, 0)}, m=2, cfg=dict(STOP, w_cd=0.0), eng_kw=dict(gemm_mode=0), ldmk_from_warp=True,
                  state_edit=_edit(iter=1, adam_t=1, total_steps=1, total_evals=1, loss_prev=0.3))[0]
    # (the float64 warp of the reference sits a float32 rounding away from the stored points: its loss is ~1e-15, not 0 -- what
    #  the generic bar holds the kernel's exact 0 against)
    assert s.nst.loss == 0.0 and s.r64.loss < 1e-12 and s.nst.decision == DEC_ADVANCE and s.nst.total_steps == 1
    assert torch.equal(s.snap.ldmk_t[:150], s.eng.pts[0, s.st.cur ^ 1, :150].cpu())
    assert (s.dO[:192] == 0).all() and s.gmax == 0.0


# ------------------------------------------------------------------------------------------------ the refused job
def test_load_jobs_refuses_samples_without_targets_under_a_chamfer_term(dev):
    """Raised before anything is launched: nothing of the engine changes (ndp_engine_load's own refusal: test_loss_stage_cpu.py)."""
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    pyr = _pyramid("se3aa", False, 1, 11)
    eng = BatchedEngine(pyr.descs[0], OptConfig(m=1, iters=2, w_cd=0.5), 1, n_cap=64, t_cap=64, device=dev)
    eng.park_all()
    torch.cuda.synchronize()
    before = (eng.state.clone(), eng.geom.clone(), eng.pts.clone())
    pts, lt, _ = R.clouds(5, 20, 0, 3)
    with pytest.raises(ValueError, match="no target"):
        eng.load(0, pts, 5, 20, lt, None, pyr.store)
    with pytest.raises(ValueError, match="no target"):
        eng.load(0, pts[5:], 0, 20, None, None, pyr.store)
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(before, (eng.state, eng.geom, eng.pts)))
    eng.load(0, pts[:5], 5, 0, lt, None, pyr.store)              # its landmarks alone are a valid pair
    eng.run_ticks(1)
    st = eng.read_states()[0]
    assert st.level == 0 and st.iter == 1 and np.isfinite(st.loss)
