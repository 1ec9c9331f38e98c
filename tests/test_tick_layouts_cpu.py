"""The table of head layouts tests/test_tick_layouts.py and tests/test_loss_stage.py run (tests/_tick_ref.py), checked on the reference
alone -- no GPU, no native library:

  * the (tag, level) cases reach every head-row count the engine kernels can meet, 3, 4 and 6 .. 11;
  * for every case the GPU tests run, the normalisations of the quaternion and 6D heads are far from their clamps and from 0 / 0:
    the quaternion's norm, the 6D head's |a1| and |a2 - (b1.a2) b1| are at least 5e-4 at every point (the kernel clamps at 1e-12);
  * no axis-angle case has a rotation vector shorter than 1e-6 (theta = 0 is the reference's own NaN and out of scope).

The head outputs are evaluated in float64 from the seeded pyramid and the case's points; a level >= 1 sees the points warped by the
levels below it (tests/_loss_ref.py: head_warp).  The GPU tests assert the same margins again on the head outputs the kernels wrote.
"""
import pytest
import torch

from tests import _loss_ref as R
from tests import _tick_ref as TR

MARGIN = 5e-4
TICK_S = 130
EDGE_S = (1, 63, 64, 65)


def _level_input(pyr, desc, level, x):
    """The points level `level` reads: x through the seeded levels below it, float64."""
    x = x.double()
    for lvl in range(level):
        d = R.level_desc(desc, lvl)
        x = R.head_warp(d, TR.level_heads(d, pyr.store[lvl], lvl, x), x)[0]
    return x


def _margins(tag, level, S):
    """S: sources of a tick case (tests/test_tick_layouts.py), or "loss": the 40 landmarks + 300 samples of tests/test_loss_stage.py's
    layout cases."""
    m = TR.levels_of(tag, level)
    pyr = TR.tick_pyramid(tag, m)
    desc = pyr.descs[m - 1]
    d = R.level_desc(desc, level)
    x = _level_input(pyr, desc, level, R.clouds(40, 300, 333, 0)[0] if S == "loss" else TR.tick_clouds(S, 120)[0])
    return d, TR.rotation_margins(d, TR.level_heads(d, pyr.store[level], level, x))


def test_the_table_reaches_every_head_row_count():
    seen = set()
    for tag, kw in TR.LAYOUTS.items():
        pyr = TR.tick_pyramid(tag, 3)
        desc = pyr.descs[-1]
        assert bool(desc.nonrigidity) == (tag in TR.GATED), tag
        rows = tuple(R.level_desc(desc, lvl).n_heads for lvl in (0, 1, 2))
        assert rows == (TR.HEAD_ROWS[tag][0], TR.HEAD_ROWS[tag][1], TR.HEAD_ROWS[tag][1]), (tag, rows)
        assert pyr.descs[0].n_heads == rows[0] and pyr.descs[1].n_heads == rows[1]          # the pyramid's own per-level descriptors
    for tag, level in TR.TICK_CASES + TR.EDGE_CASES:
        seen.add(TR.HEAD_ROWS[tag][min(level, 1)])
    assert seen == {3, 4, 6, 7, 8, 9, 10, 11}
    assert set(TR.LAYOUTS) == set(TR.HEAD_ROWS) and set(TR.GATED) == {"sflow_nr", "se3quat_nr", "sim36d_nr"}
    assert all(tag in TR.LAYOUTS for tag, _ in TR.TICK_CASES + TR.EDGE_CASES)
    assert {t for t, lvl in TR.TICK_CASES if lvl == 0} == set(TR.LAYOUTS)
    # gate row behind a Sim3 scale row, gate row behind a quaternion, gate row with no rotation at all
    d = R.level_desc(TR.tick_pyramid("sim36d_nr", 2).descs[-1], 1)
    assert (d.row_scale, d.row_trn, d.row_nr, d.n_heads) == (6, 7, 10, 11)
    d = R.level_desc(TR.tick_pyramid("se3quat_nr", 2).descs[-1], 1)
    assert (d.row_trn, d.row_nr, d.n_heads) == (4, 7, 8)
    d = R.level_desc(TR.tick_pyramid("sflow_nr", 2).descs[-1], 1)
    assert (d.row_trn, d.row_nr, d.n_heads) == (0, 3, 4)


def _cases():
    out = [(tag, level, TICK_S) for tag, level in TR.TICK_CASES]
    out += [(tag, level, S) for tag, level in TR.EDGE_CASES for S in EDGE_S]
    out += [(tag, 0, "loss") for tag in TR.LAYOUTS] + [(tag, 1, "loss") for tag in TR.GATED]
    return out


@pytest.mark.parametrize("tag,level,S", _cases())
def test_normalisations_are_far_from_their_clamps(tag, level, S):
    d, mg = _margins(tag, level, S)
    print(f"{tag} level {level} S {S}: " + ", ".join(f"{k} {v:.3e}" for k, v in mg.items()))
    if d.motion != "sflow" and d.rotfmt == "quaternion":
        assert mg["quat_norm"] >= MARGIN, (tag, level, S, mg)
    if d.motion != "sflow" and d.rotfmt == "6D":
        assert mg["a1_norm"] >= MARGIN and mg["u_norm"] >= MARGIN, (tag, level, S, mg)
    if d.motion != "sflow" and d.rotfmt == "axis_angle":
        assert mg["aa_norm"] >= 1e-6, (tag, level, S, mg)


def test_margins_are_what_the_restated_warp_divides_by():
    """rotation_margins names the denominators of tests/_loss_ref.py's rotations: scaling a quaternion or a 6D pair leaves the rotation
    alone (so only these norms can make it ill-conditioned), and the 6D rows are orthonormal."""
    g = torch.Generator().manual_seed(2)
    for tag in ("se3quat", "se36d"):
        d = TR.tick_pyramid(tag, 1).descs[0]
        o = ((torch.rand(9, d.n_heads, generator=g) - 0.5) * 0.01).double()
        o2 = o.clone()
        o2[:, :d.n_rot] *= 3.0
        Ra, Rb = R._rotation(d, o), R._rotation(d, o2)
        assert float((Ra - Rb).abs().max()) < 1e-12
        eye = torch.eye(3, dtype=torch.float64).expand(9, 3, 3)
        assert float((Ra @ Ra.transpose(1, 2) - eye).abs().max()) < 1e-12 and float((torch.linalg.det(Ra) - 1).abs().max()) < 1e-12
