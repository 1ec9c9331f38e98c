"""CPU test of the wave-step model of the cell search's walk (tools/nn_wave_steps.py): on a hand-made case of 64 queries -- one wave --
the modelled steps, the row part and the ideal equal a count done by hand."""
import importlib.util
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model():
    spec = importlib.util.spec_from_file_location("nn_wave_steps", os.path.join(ROOT, "tools", "nn_wave_steps.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def _case():
    """A 4 x 2 x 2 grid over the box [0, 4] x [0, 2] x [0, 2] (cells of side 1) and ten references; records per cell, x = 0 .. 3:
         row (y 0, z 0): 2, 0, 2, 0      row (y 1, z 0): 0, 3, 0, 0      row (y 0, z 1): 0, 0, 0, 1      row (y 1, z 1): 0, 0, 0, 2
       64 queries, one wave, each with the seed that fixes its radius:
         lanes 0 .. 61 at (0.5, 0.5, 0.5), seed 1 at distance 0.25: the one cell (0, 0, 0)                  -> 1 row of 2 records
         lane  62      at (1.5, 1.0, 0.4), seed 4 at distance 0.51: cells x 0 .. 2, y 0 .. 1, z 0           -> 2 rows of 4 and 3 records
         lane  63      at (2.0, 1.0, 1.0), seed 0 at distance 2.45: the whole grid                          -> 4 rows of 4, 3, 1 and 2 records
       By hand: the wave's row iterations cost max(2, 4, 4), max(3, 3), 1 and 2 = 10 record steps, its longest lane has 4 rows: 14 steps.
       Ideal: (62 (1 + 2) + (2 + 7) + (4 + 10)) / 64 = 209 / 64."""
    ref = np.array([[0.0, 0.0, 0.0], [0.25, 0.5, 0.5],
                    [2.2, 0.5, 0.5], [2.8, 0.2, 0.4],
                    [1.5, 1.5, 0.5], [1.2, 1.3, 0.2], [1.8, 1.7, 0.9],
                    [3.5, 0.5, 1.5],
                    [3.5, 1.5, 1.5], [4.0, 2.0, 2.0]], np.float32)
    q = np.tile(np.array([[0.5, 0.5, 0.5]], np.float32), (64, 1))
    seed = np.ones(64, np.int64)
    q[62] = (1.5, 1.0, 0.4); seed[62] = 4
    q[63] = (2.0, 1.0, 1.0); seed[63] = 0
    return q, ref, seed


def test_wave_steps_equal_a_count_done_by_hand():
    W = _model()
    dims = (4, 2, 2)
    q, ref, seed = _case()
    o, ih = W.geometry(ref, dims)
    assert o.tolist() == [0, 0, 0] and ih.tolist() == [1, 1, 1]
    cells = W.cell1(ref, o, ih, dims)
    per_cell = np.zeros((2, 2, 4), int)
    np.add.at(per_cell, (cells[:, 2], cells[:, 1], cells[:, 0]), 1)
    assert per_cell.tolist() == [[[2, 0, 2, 0], [0, 3, 0, 0]], [[0, 0, 0, 1], [0, 0, 0, 2]]]
    lo, hi = W.boxes(q, ref, seed, o, ih, dims)
    assert lo[0].tolist() == [0, 0, 0] and hi[0].tolist() == [0, 0, 0]
    assert lo[62].tolist() == [0, 0, 0] and hi[62].tolist() == [2, 1, 0]
    assert lo[63].tolist() == [0, 0, 0] and hi[63].tolist() == [3, 1, 1]
    nrow, rec = W.row_records(cells, dims, lo, hi)
    assert nrow.tolist() == [1] * 62 + [2, 4]
    assert rec[0].tolist() == [2, 0, 0, 0] and rec[62].tolist() == [4, 3, 0, 0] and rec[63].tolist() == [4, 3, 1, 2]
    steps, rows, ideal = W.wave_steps(nrow, rec)
    assert steps.tolist() == [14] and rows.tolist() == [4]
    assert ideal.tolist() == [209 / 64]
    st, rw, idl, nr, nc = W.direction(q, ref, seed, o, ih, dims)
    assert (st.tolist(), rw.tolist(), idl.tolist(), nr, nc) == ([14], [4], [209 / 64], 62 + 2 + 4, 62 * 2 + 7 + 10)


def test_boxes_follow_the_kernels_radius_and_clamp():
    """boxes(): the ball of a query around its seed, with the kernel's margins, in cells; a query outside the box clamps into border cells."""
    W = _model()
    dims = (4, 2, 2)
    _, ref, _ = _case()
    o, ih = W.geometry(ref, dims)
    q = np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [9.0, 0.5, 0.5], [2.2, 0.5, 0.5]], np.float32)
    seed = np.array([1, 1, 9, 2])                     # distances 0.25, 1.25, 5.4 from outside the box, 0 (the query IS its seed)
    lo, hi = W.boxes(q, ref, seed, o, ih, dims)
    assert lo.tolist() == [[0, 0, 0], [0, 0, 0], [3, 0, 0], [2, 0, 0]]
    assert hi.tolist() == [[0, 0, 0], [2, 1, 1], [3, 1, 1], [2, 0, 0]]


def test_lane_mapping_is_t_plus_1024_u():
    """1100 queries: u = 0 holds 16 full waves, u = 1 two waves of 64 and 12 lanes; a wave's steps come from ITS queries only."""
    W = _model()
    nrow = np.ones(1100, np.int64)
    rec = np.ones((1100, 1), np.int64)
    nrow[1024 + 70] = 3                                # query 1094 = thread 70, u 1: wave 1 of the second pass
    rec = np.concatenate([rec, np.zeros((1100, 2), np.int64)], 1)
    rec[1094] = (1, 5, 2)
    steps, rows, ideal = W.wave_steps(nrow, rec)
    assert len(steps) == 16 + 2
    assert steps.tolist() == [2] * 17 + [1 + 5 + 2 + 3] and rows.tolist() == [1] * 17 + [3]
    assert ideal[16] == 2.0 and ideal[17] == (11 * 2 + 3 + 8) / 64
