"""CPU-side checks of the wide cell search's plumbing (clouds of up to 8192 points, csrc/ndp_nn_cells_wide.inc): ABI version and struct
mirror, the fits query, the workspace formula, the selection rule -- and that the rule of the <= 2048 search answers as before."""
import ctypes

import pytest


def test_abi_208_carries_the_wide_cell_search():
    from deformationpyramid_amd import _native as N
    L = N.lib()
    assert L.ndp_version() >= 208
    for name in ("ndp_chamfer_nn_cells_wide", "ndp_chamfer_nn_cells_wide_workspace", "ndp_engine_nn_cells_wide_fits"):
        assert name in N._SIGS and name in N.EXPORTS
        getattr(L, name)
    assert "ndp_nn_cells_wide.inc" in N.HEADERS                 # part of the build id
    assert "ndp_nn_cells.inc" in N.HEADERS
    assert (N.NNC_MAX, N.NNW_MAX) == (2048, 8192)


def test_wide_fits_and_workspace():
    from deformationpyramid_amd import _native as N
    L = N.lib()
    fits = L.ndp_engine_nn_cells_wide_fits
    assert fits(8192, 8192) == 1 and fits(2048, 2048) == 1 and fits(1, 1) == 1
    assert fits(8256, 64) == 0 and fits(64, 8256) == 0 and fits(0, 64) == 0 and fits(64, 0) == 0
    # [geometry 8 | two cell_start tables | the targets' and the sources' records, four floats each]
    nf = ctypes.c_longlong()
    for S, T in ((8192, 8192), (1, 1), (5000, 777), (0, 0)):
        assert L.ndp_chamfer_nn_cells_wide_workspace(S, T, ctypes.byref(nf)) == 0
        assert nf.value == 8 + 2 * N.NNC_START + 4 * T + 4 * S
    assert nf.value % 4 == 0
    assert L.ndp_chamfer_nn_cells_wide_workspace(-1, 4, ctypes.byref(nf)) == -1          # NDP_E_INVALID
    assert L.ndp_chamfer_nn_cells_wide_workspace(4, 4, None) == -1


def test_the_old_engine_fields_stay_put_and_the_new_ones_follow():
    from deformationpyramid_amd import _native as N
    E = N.Engine
    sizes = (ctypes.c_int * 6)()
    assert N.lib().ndp_abi_sizes(sizes) == 0 and sizes[3] == ctypes.sizeof(E)
    # what ABI 207 pinned (tests/test_nn_cells_cpu.py) ...
    assert E.nn_cells.offset == E.gmax.offset + 8 and E.nnc_geom.offset == E.nn_cells.offset + 8
    assert E.nnc_start.offset == E.nnc_geom.offset + 8 and E.nnc_rec.offset == E.nnc_start.offset + 8
    # ... and the new fields behind the last of them, 8-byte aligned, nothing behind; no new pointer: the wide search keeps its
    # grids in nnc_geom / nnc_start / nnc_rec, in a layout of its own
    assert E.nn_cells_wide.offset == E.nnc_rec.offset + 8 and E.nn_cells_wide.offset % 8 == 0
    assert E.pad_w.offset == E.nn_cells_wide.offset + 4 and ctypes.sizeof(E) == E.nn_cells_wide.offset + 8
    assert [n for n, _ in E._fields_][-5:] == ["nnc_geom", "nnc_start", "nnc_rec", "nn_cells_wide", "pad_w"]
    header = open(N.os.path.join(N.CSRC, "..", "..", "include", "ndp_hip.h")).read()
    assert header.index("int nn_cells, pad_i;") < header.index("int nn_cells_wide, pad_w;") < header.index("} ndp_engine;")


def test_wide_selection_rule():
    from deformationpyramid_amd import _native as N
    from deformationpyramid_amd import engine
    r = engine.resolve_nn_cells_wide
    assert engine.DEFAULT_NN_CELLS_WIDE in (True, False)
    D = bool(engine.DEFAULT_NN_CELLS_WIDE)
    # None: the default, where the engine chose a one-pass shape itself, nn_cells resolved false and the capacities fit
    assert r(4096, 4096, None, 2, False) is D and r(8192, 6144, None, 0, False) is D
    assert r(4096, 4096, None, 1, False) is False                # the engine chose the latency shape: few pairs
    assert r(4096, 4096, 2, 2, False) is False                   # an explicit nn_mode keeps its kernel
    assert r(2048, 2048, None, 2, True) is False                 # the <= 2048 search has the stage
    assert r(8256, 4096, None, 2, False) is False and r(4096, 8256, None, 2, False) is False
    # explicit
    assert r(4096, 4096, None, 2, False, True) is True and r(4096, 4096, None, 2, False, False) is False
    assert r(4096, 4096, 2, 2, False, True) is True              # with an explicit nn_mode: allowed, as for nn_cells
    assert r(4096, 4096, None, 1, False, True) is True
    assert r(2048, 2048, 2, 2, False, True) is True              # small capacities fit as well
    assert r(2048, 2048, None, 2, True, False) is False
    with pytest.raises(N.NdpError, match="nn_cells_wide"):
        r(8256, 8192, None, 2, False, True)
    with pytest.raises(N.NdpError, match="nn_cells_wide"):
        r(2048, 2048, None, 2, True, True)
    # the default constant off: None never selects it, True still does
    saved = engine.DEFAULT_NN_CELLS_WIDE
    try:
        engine.DEFAULT_NN_CELLS_WIDE = False
        assert r(4096, 4096, None, 2, False) is False and r(4096, 4096, None, 2, False, True) is True
        engine.DEFAULT_NN_CELLS_WIDE = True
        assert r(4096, 4096, None, 2, False) is True and r(4096, 4096, None, 1, False) is False
    finally:
        engine.DEFAULT_NN_CELLS_WIDE = saved


def test_the_2048_rule_answers_as_before():
    from deformationpyramid_amd import _native as N
    from deformationpyramid_amd.engine import resolve_nn_cells
    L = N.lib()
    assert L.ndp_engine_nn_cells_fits(2048, 2048) == 1 and L.ndp_engine_nn_cells_fits(2112, 2048) == 0
    assert L.ndp_engine_nn_cells_fits(2048, 2112) == 0 and L.ndp_engine_nn_cells_fits(4096, 4096) == 0
    assert resolve_nn_cells(2048, 2048, None, 2) and resolve_nn_cells(2048, 2048, None, 0)
    assert not resolve_nn_cells(2048, 2048, None, 1) and not resolve_nn_cells(2048, 2048, 2, 2)
    assert not resolve_nn_cells(4096, 2048, None, 2) and not resolve_nn_cells(4096, 4096, None, 2)
    assert resolve_nn_cells(2048, 2048, 2, 2, True) and not resolve_nn_cells(2048, 2048, None, 2, False)
    with pytest.raises(N.NdpError, match="nn_cells"):
        resolve_nn_cells(4096, 4096, None, 2, True)
    nf = ctypes.c_longlong()
    assert L.ndp_chamfer_nn_cells_workspace(2048, ctypes.byref(nf)) == 0 and nf.value == 8 + N.NNC_START + 4 * 2048
