"""The level kernels of the 128 / 3 engine's tick under every head layout and at the tile loop's edges, each kernel against float64.

k_eng_fwd8, k_eng_bwd_f, k_eng_bwd2_8 + k_eng_bwd1_8 and the fp32 chain specialise on the head-row count (dO staged in groups of four
rows, the head matrix loaded at a clamped index and zero-filled above nh x 128, dWh accumulators of three lane groups); the suite ran
them with 3, 6 and 7 head rows only.  Here one tick of a one-pair engine runs stage by stage (tests/_tick_ref.py) for every layout of
the table -- 3, 4, 6, 7, 8, 9, 10 and 11 head rows; gated layouts at level 0, where the shorter layout lives in a parameter block sized
for the longer one, and at level 1 -- and every output tensor of every kernel (h0, h1, h2, head outputs, dWh, dbh, dW2, db2, dz1, dW1,
db1, dW0, db0) is held against a float64 evaluation of that kernel from its own inputs, in three arithmetics: gemm_mode 0 (the fp32
chain), 7 (the fused split backward) and 7 | 16 (the two-launch split backward).

The bar, per tensor (tests/_tick_ref.py: allowed): the yardstick is the SAME reference evaluated in float32 on the CPU, never a kernel;
the fp32 chain may be 4 yardsticks off (floor: 16 float32 ulps of max |ref|), the split kernels 4 r yardsticks with r what
tests/test_split_accuracy.py grants the split over the chain in maximum error (2 from 10 000 elements on: 8 yardsticks; 3 below: 12).
On top of it every tensor stays within 5e-6 of its own scale.  Every case prints error / yardstick per tensor before it asserts; the
table of a whole run is written to build/reports/tick_layouts_accuracy.txt (a copy is kept as profiles/tick_layouts_accuracy.txt).

The buffers the kernels fill (act, heads, dO, the gradient partials) are NaN before the tick: what a kernel reads without its having
been written this tick, or leaves unwritten, shows.

Edges (se3aa at level 0, six head rows; sim36d_nr at level 1, eleven): pairs of 1, 63, 64 and 65 points; more workgroups than tiles
(their partials are exactly zero); an engine two tiles larger than the pair (bit for bit the gradients of a tight engine); the fused
against the two-launch backward on every shape.

Out of scope: whole trajectories with quaternion / 6D heads (chaotic for every arithmetic: tests/test_generic_width.py), generic widths,
the NN stage, the axis-angle head at theta = 0.
"""
import functools
import os

import pytest
import torch

from tests import _tick_ref as TR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S_TICK, T_TICK = 130, 120                  # three tiles: 64 + 64 + 2 points
T_EDGE = 70
MODES = {"chain": 0, "fused": 7, "two_launch": 7 | 16}
KERNEL_OF = {"h0": "fwd", "h1": "fwd", "h2": "fwd", "heads": "fwd", "dWh": "bwd2", "dbh": "bwd2", "dW2": "bwd2", "db2": "bwd2", "dz1": "bwd2",
             "dW1": "bwd1", "db1": "bwd1", "dW0": "bwd1", "db0": "bwd1"}
GRADS = ("dWh", "dbh", "dW2", "db2", "dz1", "dW1", "db1", "dW0", "db0")
_REPORT = {}


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _run(tag, level, mode, S, T, G, n_cap=None, warm_mode=None):
    """One tick by stages, shared by every assertion on it (the results are read, never changed)."""
    return TR._run_tick_by_stages(torch.device("cuda:0"), tag, mode, S, T, level, TR.HEAD_SCALE, G=G, n_cap=n_cap, poison=True,
                                  warm_mode=warm_mode)


def _bits(t):
    return t.contiguous().view(torch.int32)                     # bit for bit, the NaN of a never-written element included


def _write_report():
    out_dir = os.path.join(ROOT, "build", "reports")
    os.makedirs(out_dir, exist_ok=True)
    worst = {}
    with open(os.path.join(out_dir, "tick_layouts_accuracy.txt"), "w") as f:
        f.write("level kernels of one engine tick against float64 of their own inputs (tests/test_tick_layouts.py); yardstick = the same\n"
                "reference in float32 on the CPU; allowed = max(factor x yardstick, 16 float32 ulps of max|ref|), factor 4 for the fp32 chain,\n"
                "8 (>= 10 000 elements) / 12 for the split kernels; ratio = err / (allowed / factor), the bar is ratio <= factor\n\n")
        f.write(f"{'case':<44}{'tensor':<7}{'elements':>9}{'kernel err':>12}{'yardstick':>12}{'max|ref|':>12}{'allowed':>12}{'ratio':>8}{'factor':>7}\n")
        for case in sorted(_REPORT):
            arith, rows = _REPORT[case]
            for k, q, a, rt, fac in rows:
                f.write(f"{case:<44}{k:<7}{q['elements']:>9}{q['err']:>12.3e}{q['yardstick']:>12.3e}{q['scale']:>12.3e}{a:>12.3e}{rt:>8.2f}{fac:>7.0f}\n")
                key = (KERNEL_OF[k], arith)
                if key not in worst or rt / fac > worst[key][0] / worst[key][3]:
                    worst[key] = (rt, case, k, fac)
        f.write("\nlargest ratio per kernel and arithmetic (ratio, factor, case, tensor)\n")
        for (kern, arith), (rt, case, k, fac) in sorted(worst.items()):
            f.write(f"{kern:<6}{arith:<12}{rt:>8.2f}{fac:>6.0f}  {case}  {k}\n")


def _check_accuracy(case, arith, r):
    """finite, within the bar and the cap, per tensor; prints error / yardstick first."""
    mode = MODES[arith]
    got = TR._kernel_outputs(r)
    qs = TR.yardsticks(r)
    rows = []
    for k in TR.TENSORS:
        q = qs[k]
        a, rt, fac = TR.allowed(q, mode), TR.ratio(q, mode), TR.factor_of(mode, q["elements"])
        rows.append((k, q, a, rt, fac))
        print(f"{case} {k:<6} n={q['elements']:<6} err {q['err']:.3e} yardstick {q['yardstick']:.3e} err/yardstick "
              f"{q['err'] / q['yardstick'] if q['yardstick'] > 0 else float('nan'):.2f} scale {q['scale']:.3e} ratio {rt:.2f} / {fac:.0f}")
    _REPORT[case] = (arith, rows)
    _write_report()
    for k in TR.TENSORS:
        assert bool(torch.isfinite(got[k]).all()), (case, k)
    for k, q, a, rt, fac in rows:
        assert q["err"] <= a, (case, k, "error over the bar", q, a, rt)
        assert q["err"] <= TR.CAP * q["scale"], (case, k, "error over 5e-6 of the scale", q)


def _check_forward_record(case, r):
    """What the forward documents for a point's record: head outputs in columns < nh, zero in columns nh .. 15 (rows of the head matrix
    above nh are zero-filled, their bias is zero), the six encoding values sin / cos (2^(level + 1 + k0) x) in columns 16 .. 21."""
    d, n = r["desc"], r["n"]
    nh = d.n_heads
    rec = r["heads"][:n]
    assert bool(torch.isfinite(rec[:, :22]).all()), case
    assert bool((rec[:, nh:16] == 0).all()), (case, "head columns >= nh")
    a = r["x_in"].double() * 2.0 ** (r["level"] + 1 + TR.K0)
    want = torch.stack([torch.sin(a[:, 0]), torch.cos(a[:, 0]), torch.sin(a[:, 1]), torch.cos(a[:, 1]), torch.sin(a[:, 2]), torch.cos(a[:, 2])], -1)
    assert float((rec[:, 16:22].double() - want).abs().max()) <= 16 * TR.ULP, (case, "encoding columns")
    assert bool(torch.isfinite(r["dO"][:n]).all()) and bool((r["dO"][:n, nh:] == 0).all()), (case, "dO")
    for k, v in TR.rotation_margins(d, rec[:, :nh]).items():          # tests/test_tick_layouts_cpu.py, on what the kernel wrote
        assert v >= (1e-6 if k == "aa_norm" else 5e-4), (case, k, v)


def _check_partials(case, r):
    """The G gradient partials as the backward left them: every parameter of the LEVEL's layout written by every workgroup (finite; a
    workgroup without a tile: exactly zero, the whole partial); beyond the level's parameter count -- the rows of Wh / bh above nh,
    where a gated engine's level 0 has no gate row -- untouched (still the NaN it was filled with) or zero, as the update stage expects."""
    d, ed, n = r["desc"], r["engine_desc"], r["n"]
    gp = r["gpart"]
    Pl, P = d.param_count, ed.param_count
    n_tiles = (n + 63) // 64
    assert gp.shape[0] == r["G"]
    for g in range(gp.shape[0]):
        if g < n_tiles:
            assert bool(torch.isfinite(gp[g, :Pl]).all()), (case, "partial", g)
            rest = gp[g, Pl:]
            assert bool((torch.isnan(rest) | (rest == 0)).all()), (case, "partial beyond the level's parameters", g)
        else:
            assert bool((gp[g, :P] == 0).all()), (case, "partial of a workgroup without a tile", g)
            rest = gp[g, P:]
            assert bool((torch.isnan(rest) | (rest == 0)).all()), (case, "padding of an idle partial", g)
    if ed.nonrigidity and r["level"] == 0:
        # the gate row's place in the gated layout, [off_Wh + nh0 W, + W): at level 0 it holds dbh (nh0 values, compared with float64
        # by the accuracy check) and nothing else
        nh0 = d.n_heads
        lo = d.off_Wh + nh0 * d.width
        assert lo == d.off_bh and Pl == lo + nh0 and P == Pl + d.width + 1
        place = gp[:, lo + nh0:lo + d.width]
        assert bool((torch.isnan(place) | (place == 0)).all()), (case, "gate row's place at level 0")
        folded = r["g_all"][lo + nh0:P]
        assert bool((torch.isnan(folded) | (folded == 0)).all()), (case, "gate row's place at level 0, folded")


# ------------------------------------------------------------------------------------------------ every layout
@pytest.mark.parametrize("arith", list(MODES))
@pytest.mark.parametrize("G", [None, 1], ids=["Gtiles", "G1"])
@pytest.mark.parametrize("tag,level", TR.TICK_CASES, ids=[f"{t}-L{lvl}" for t, lvl in TR.TICK_CASES])
def test_level_kernels_meet_float64_under_every_head_layout(dev, tag, level, G, arith):
    """S = 130 (tiles of 64 + 64 + 2 points), T = 120; G: one workgroup per tile | one for the pair (the benchmark's shape)."""
    case = f"layout/{tag}/L{level}/G{G or 'tiles'}/{arith}"
    r = _run(tag, level, MODES[arith], S_TICK, T_TICK, G)
    assert r["desc"].n_heads == TR.HEAD_ROWS[tag][min(level, 1)] and r["G"] == (G or 3)
    _check_forward_record(case, r)
    _check_partials(case, r)
    _check_accuracy(case, arith, r)


# ------------------------------------------------------------------------------------------------ tile and workgroup edges
def _edge_params():
    out = []
    for tag, level in TR.EDGE_CASES:
        for S in (1, 63, 64, 65):
            for G in (None, 1, 3):
                for arith in ("fused", "two_launch") + (("chain",) if G == 3 else ()):       # the chain at one G per shape: the one with idle workgroups
                    out.append(pytest.param(tag, level, S, G, arith, id=f"{tag}-L{level}-S{S}-G{G or 'tiles'}-{arith}"))
    return out


@pytest.mark.parametrize("tag,level,S,G,arith", _edge_params())
def test_tile_and_workgroup_edges(dev, tag, level, S, G, arith):
    """One point, a tile less one, a full tile, a tile and one; G = 3 at one or two tiles: workgroups without a tile, whose partials
    are exactly zero.  The folded gradient (and every other output) meets the bar."""
    case = f"edge/{tag}/L{level}/S{S}/G{G or 'tiles'}/{arith}"
    r = _run(tag, level, MODES[arith], S, T_EDGE, G)
    n_tiles = (S + 63) // 64
    assert r["G"] == (G or n_tiles) and r["n"] == S
    if G == 3:
        assert r["gpart"].shape[0] == 3 > n_tiles
    _check_forward_record(case, r)
    _check_partials(case, r)
    _check_accuracy(case, arith, r)


@pytest.mark.parametrize("S", [1, 63, 64, 65])
@pytest.mark.parametrize("tag,level", TR.EDGE_CASES, ids=[f"{t}-L{lvl}" for t, lvl in TR.EDGE_CASES])
def test_fused_and_two_launch_backward_agree_at_the_edges(dev, tag, level, S):
    """Same forward state, two summation orders: every gradient tensor within 2e-6 of its own scale
    (tests/test_split_accuracy.py: test_fused_backward_agrees_with_the_two_launch_backward), for each G.  The ticks that bring the pair
    to level 1 run on the fp32 chain in both engines, so that both see the same parameters and points there."""
    for G in (None, 1, 3):
        a, b = _run(tag, level, 7, S, T_EDGE, G, None, 0), _run(tag, level, 7 | 16, S, T_EDGE, G, None, 0)
        assert torch.equal(a["params"], b["params"]) and torch.equal(a["x_in"], b["x_in"])
        assert torch.equal(a["dO"][:S], b["dO"][:S]) and torch.equal(a["act_fwd"][0, :S], b["act_fwd"][0, :S])
        assert torch.equal(a["g_bwd2"][:a["desc"].param_count], a["g_all"][:a["desc"].param_count])       # the fused stage 3 is the whole backward
        ka, kb = TR._kernel_outputs(a), TR._kernel_outputs(b)
        for k in GRADS:
            err = float((ka[k] - kb[k]).abs().max() / kb[k].abs().max().clamp_min(1e-300))
            print(f"agree/{tag}/L{level}/S{S}/G{G or 'tiles'} {k}: {err:.3e}")
            assert err < 2e-6, (tag, level, S, G, k, err)


@pytest.mark.parametrize("arith", list(MODES))
@pytest.mark.parametrize("tag,level", TR.EDGE_CASES, ids=[f"{t}-L{lvl}" for t, lvl in TR.EDGE_CASES])
def test_capacity_beyond_the_pair_changes_no_bit(dev, tag, level, arith):
    """S = 65 in an engine of n_cap = 256: two tiles beyond the pair are never walked (act, heads and dO there stay the NaN they were
    filled with), no NaN reaches a gradient, and every partial is bit for bit what an engine of n_cap = 128 computes.  G is passed
    explicitly: left to the engine it is the capacity's tile count (engine.py), 4 against 2."""
    for G in (1, 2):
        wide, tight = _run(tag, level, MODES[arith], 65, T_EDGE, G, 256), _run(tag, level, MODES[arith], 65, T_EDGE, G, 128)
        assert (wide["n_cap"], tight["n_cap"], wide["G"], tight["G"]) == (256, 128, G, G)
        case = f"capacity/{tag}/L{level}/G{G}/{arith}"
        Pl = wide["desc"].param_count
        assert bool(torch.isfinite(wide["gpart"][:, :Pl]).all()) and bool(torch.isfinite(wide["g_all"][:Pl]).all()), case
        assert bool(torch.isnan(wide["heads"][128:]).all()) and bool(torch.isnan(wide["dz1"][128:]).all()), case    # never walked
        assert bool((wide["dO"][65:] == 0).all()), case              # (the loss stage zeroes the rest of its 256-point block)
        for k in ("gpart_bwd2", "gpart"):
            assert torch.equal(_bits(wide[k]), _bits(tight[k])), (case, k)
        for k in ("heads", "dO", "dz1"):
            assert torch.equal(_bits(wide[k][:65]), _bits(tight[k][:65])), (case, k)
        assert torch.equal(_bits(wide["act_fwd"][:, :65]), _bits(tight["act_fwd"][:, :65])), case
        _check_partials(case, wide)
