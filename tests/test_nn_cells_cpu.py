"""CPU-side checks of the cell search's plumbing: ABI version and struct mirror, the fits query, the default selection rule."""
import ctypes

import pytest


def test_abi_207_carries_the_cell_search():
    from deformationpyramid_amd import _native as N
    L = N.lib()
    assert L.ndp_version() >= 207
    for name in ("ndp_chamfer_nn_cells", "ndp_chamfer_nn_cells_workspace", "ndp_engine_nn_cells_fits"):
        assert name in N._SIGS and name in N.EXPORTS
    sizes = (ctypes.c_int * 6)()
    assert L.ndp_abi_sizes(sizes) == 0 and sizes[3] == ctypes.sizeof(N.Engine)
    assert N.Engine.nn_cells.offset == N.Engine.gmax.offset + 8 and N.Engine.nnc_geom.offset % 8 == 0
    header = open(N.os.path.join(N.CSRC, "..", "..", "include", "ndp_hip.h")).read()
    assert f"#define NDP_NNC_START {N.NNC_START}" in header
    nf = ctypes.c_longlong()
    assert L.ndp_chamfer_nn_cells_workspace(2048, ctypes.byref(nf)) == 0 and nf.value == 8 + N.NNC_START + 4 * 2048
    assert "ndp_nn_cells.inc" in N.HEADERS                      # part of the build id


def test_cell_search_default_selection_rule():
    from deformationpyramid_amd import _native as N
    from deformationpyramid_amd.engine import resolve_nn_cells
    L = N.lib()
    assert L.ndp_engine_nn_cells_fits(2048, 2048) == 1 and L.ndp_engine_nn_cells_fits(64, 64) == 1
    assert L.ndp_engine_nn_cells_fits(2112, 2048) == 0 and L.ndp_engine_nn_cells_fits(2048, 4096) == 0
    # None: on where the engine chose a one-pass shape itself and the capacities fit
    assert resolve_nn_cells(2048, 2048, None, 2) and resolve_nn_cells(2048, 2048, None, 0)
    assert not resolve_nn_cells(2048, 2048, None, 1)            # the engine chose the latency shape: few pairs
    assert not resolve_nn_cells(2048, 2048, 2, 2)               # an explicit nn_mode keeps its kernel
    assert not resolve_nn_cells(4096, 2048, None, 2)
    # explicit
    assert resolve_nn_cells(2048, 2048, 2, 2, True) and not resolve_nn_cells(2048, 2048, None, 2, False)
    with pytest.raises(N.NdpError, match="nn_cells"):
        resolve_nn_cells(4096, 4096, None, 2, True)
