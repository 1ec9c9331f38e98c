"""The tick plan without a GPU: ndp_engine_plan reports, for hand-built engine records, the launches ndp_engine_run would make.

The expected names, grids, block sizes, LDS bytes and third arguments are literals, worked out from the launcher's formulas as they
stood before the plan existed (ABI 217: engine_launch_ticks, nn1_lds_floats, nn2_lds_floats, NNC_LDS_BYTES, NNW_*, upd_rest_count and
the kSmem* totals of the level kernels) -- not read back from the library.  Shared shape unless a test says otherwise:
n_cap = t_cap = 512, m = 1, the default descriptor (128 / 3, SE3, axis-angle: P = 34694)."""
import ctypes
import os

import pytest

from deformationpyramid_amd import _native as N
from deformationpyramid_amd.engine import tick_plan
from deformationpyramid_amd.layout import LayerDesc

E_INVALID, E_UNSUPPORTED = -1, -2
# dynamic LDS of the level kernels: fp32 forward / backward, split forward, fused backward, split bwd2 / bwd1; generic at width 64
FWD, BWD, FWD8, BWD_F, BWD2_8, BWD1_8, GEN_FWD_64, GEN_BWD_64 = 80640, 77056, 145984, 162944, 119808, 90112, 44032, 39000
NN_512 = (3 * 256 + 4 * 256 + 3 * 4 * 129) * 4                    # k_eng_nn: target chunk, column table of 4 blocks, staged sources = 13360
MX8_512 = (4 * 64 * 8 + 4 * 64 * 8 + 3 * 4 * 129 + 8 * 32 * 33 + 8 + 2 * 8 * 2 * 64 * 4) * 4        # k_eng_nn_mx8 = 89168
LAT16, LAT8 = (3 * 2048 + 2 * 1024) * 4, (3 * 2048 + 2 * 512) * 4
NNC_LDS, NNW_LDS, NNW_SORT_LDS = 49312, 147488, 16544
POINTERS = ("geom", "state", "pts", "ldmk_t", "tgt", "params", "gpart", "adam_m", "adam_v", "act", "heads", "d2x", "idx_x", "d2y", "idx_y",
            "adam_tab", "dO", "nn_row", "gmax")
GRID_POINTERS = ("nnc_geom", "nnc_start", "nnc_rec")


def engine(gemm_mode=7, nn_mode=2, G=1, B=4, n_cap=512, t_cap=512, w_cd=1.0, nn_cells=0, nn_cells_wide=0, desc=LayerDesc(), null=()):
    """An engine record whose buffers are dummy 16-byte aligned addresses: the plan dereferences none of them."""
    e = N.Engine()
    e.desc = desc.c_struct()
    e.m, e.k0, e.P, e.p_stride = 1, -8, desc.param_count, (desc.param_count + 63) // 64 * 64
    e.iters, e.max_break_count, e.early_stop = 10, 15, 1
    e.B, e.G, e.n_cap, e.t_cap = B, G, n_cap, t_cap
    e.w_cd, e.trunc = w_cd, 1e9
    e.gemm_mode, e.nn_mode, e.nn_cells, e.nn_cells_wide = gemm_mode, nn_mode, nn_cells, nn_cells_wide
    names = POINTERS + (GRID_POINTERS if nn_cells or nn_cells_wide else ())
    for i, name in enumerate(names):
        setattr(e, name, None if name in null else 0x10000 + 16 * i)
    return e


def refused(e, code, phrase):
    out, n = (N.StageLaunch * 12)(), ctypes.c_int(-7)
    L = N.lib()
    assert L.ndp_engine_plan(ctypes.byref(e), out, ctypes.byref(n)) == code
    assert phrase in L.ndp_last_error().decode() and n.value == -7
    with pytest.raises(N.NdpError, match=phrase):
        tick_plan(e)


LOSS_512 = ("k_eng_loss", (3, 4, 1), 256, 0, None)                  # two workgroups of 256 points and the loss / decision workgroup
UPDATE = ("k_eng_update", (136, 4, 1), 256, 0, None)              # ceil(34694 / 256)
UPDATE_REST = ("k_eng_update_rest", (8, 4, 1), 256, 0, None)      # W0 and b0, b1, and everything behind W2: 1926 parameters


def test_abi_218_carries_the_plan():
    L = N.lib()
    assert L.ndp_version() >= 218
    assert "ndp_engine_plan" in N._SIGS and "ndp_engine_plan" in N.EXPORTS
    versions = open(os.path.join(N.CSRC, "ndp_abi_common.inc")).read()
    assert "//   218: ndp_engine_plan" in versions
    assert ctypes.sizeof(N.StageLaunch) == 40


def test_row1_fused_split_tick_at_one_workgroup_per_pair():
    want = [[("k_eng_fwd8", (1, 4, 1), 512, FWD8, 1)], [("k_eng_nn_mx8", (1, 4, 1), 512, MX8_512, None)], [LOSS_512],
            [("k_eng_bwd_f", (1, 4, 1), 512, BWD_F, None)], [], [UPDATE_REST]]
    assert tick_plan(engine(gemm_mode=7, G=1, B=4, nn_mode=2)) == want
    assert MX8_512 == 89168
    want[5] = [UPDATE]                                               # bit 1024: the whole Adam step in the update stage
    assert tick_plan(engine(gemm_mode=7 | 1024, G=1, B=4, nn_mode=2)) == want


def test_row2_the_warp_rides_in_the_tile_loop_only_with_one_tile_per_workgroup_and_few_of_them():
    assert tick_plan(engine(gemm_mode=7, G=8, B=4))[0] == [("k_eng_fwd8", (8, 4, 1), 512, FWD8, 0)]        # G = n_cap / 64
    assert tick_plan(engine(gemm_mode=7, G=4, B=4))[0] == [("k_eng_fwd8", (4, 4, 1), 512, FWD8, 1)]
    assert tick_plan(engine(gemm_mode=7, G=8, B=64))[0] == [("k_eng_fwd8", (8, 64, 1), 512, FWD8, 1)]      # B G = 512 > 256
    assert tick_plan(engine(gemm_mode=7, G=8, B=32))[0] == [("k_eng_fwd8", (8, 32, 1), 512, FWD8, 0)]      # B G = 256


def test_row3_two_launch_split_backward():
    plan = tick_plan(engine(gemm_mode=7 | 16, G=2))
    assert plan[0] == [("k_eng_fwd8", (2, 4, 1), 512, FWD8, 1)]
    assert plan[3] == [("k_eng_bwd2_8", (2, 4, 1), 512, BWD2_8, None)]
    assert plan[4] == [("k_eng_bwd1_8", (2, 4, 1), 512, BWD1_8, None)]
    assert plan[5] == [UPDATE]


@pytest.mark.parametrize("G,g8", [(2, 1), (1, 1), (6, 3)])
def test_row4_mixed_masks_put_the_split_kernels_on_half_the_grid(G, g8):
    plan = tick_plan(engine(gemm_mode=5, G=G))
    assert plan[0] == [("k_eng_fwd8", (g8, 4, 1), 512, FWD8, 1)]
    assert plan[3] == [("k_eng_bwd2_8", (g8, 4, 1), 512, BWD2_8, None)]
    assert plan[4] == [("k_eng_bwd1", (G, 4, 1), 256, BWD, None)]
    assert plan[5] == [UPDATE]


def test_row5_fp32_tick_with_the_one_pass_vector_search():
    want = [[("k_eng_fwd", (2, 4, 1), 256, FWD, None)], [("k_eng_nn", (2, 4, 1), 256, NN_512, 1)], [LOSS_512],
            [("k_eng_bwd2", (2, 4, 1), 256, BWD, None)], [("k_eng_bwd1", (2, 4, 1), 256, BWD, None)], [UPDATE]]
    assert tick_plan(engine(gemm_mode=0, nn_mode=0, G=2)) == want
    assert NN_512 == 13360
    # the largest table that fits 160 KB leaves no room to stage the sources: 157 blocks of 128
    assert tick_plan(engine(gemm_mode=0, nn_mode=0, G=2, n_cap=20096))[1] == [("k_eng_nn", (2, 4, 1), 256, 163840, 0)]


def test_row6_latency_shape_has_a_16_wave_form_for_one_or_two_pairs():
    assert tick_plan(engine(nn_mode=1, B=2))[1] == [("k_eng_nn_lat16", (16, 2, 1), 1024, LAT16, None)]
    assert tick_plan(engine(nn_mode=1, B=3))[1] == [("k_eng_nn_lat8", (16, 3, 1), 512, LAT8, None)]
    assert (LAT16, LAT8) == (32768, 28672)


def test_row7_cell_searches_take_the_stage_whatever_nn_mode_names():
    for nn_mode in (0, 1, 2):
        assert tick_plan(engine(nn_mode=nn_mode, nn_cells=1))[1] == [("k_eng_nn_cells", (2, 4, 1), 1024, NNC_LDS, None)]
    plan = tick_plan(engine(nn_cells_wide=1, n_cap=4096, t_cap=4096))
    assert plan[1] == [("k_eng_nnw_sort", (4, 1, 1), 1024, NNW_SORT_LDS, None), ("k_eng_nn_cells_wide", (4, 4, 1), 1024, NNW_LDS, 2)]
    assert plan[2] == [("k_eng_loss", (17, 4, 1), 256, 0, None)]
    refused(engine(nn_cells=1, nn_cells_wide=1), E_INVALID, "nn_cells and nn_cells_wide together")


def test_row8_other_widths_run_the_generic_kernels_whatever_gemm_mode_says():
    desc = LayerDesc(width=64)
    assert desc.param_count == 9158
    want = [[("k_eng_fwd_gen", (2, 4, 1), 256, GEN_FWD_64, None)], [("k_eng_nn_mx8", (1, 4, 1), 512, MX8_512, None)], [LOSS_512],
            [("k_eng_bwd_gen", (2, 4, 1), 256, GEN_BWD_64, None)], [], [("k_eng_update", (36, 4, 1), 256, 0, None)]]
    for gemm_mode in (0, 7):
        assert tick_plan(engine(gemm_mode=gemm_mode, G=2, desc=desc)) == want
    assert tick_plan(engine(gemm_mode=7, G=1, desc=desc))[5] == [("k_eng_update", (36, 4, 1), 256, 0, None)]


def test_row9_no_chamfer_term_no_search():
    plan = tick_plan(engine(w_cd=0.0, null=("nn_row", "d2x", "d2y", "idx_x", "idx_y", "tgt")))
    assert plan[1] == [] and [len(s) for s in plan] == [1, 0, 1, 1, 0, 1]
    assert tick_plan(engine(w_cd=0.0, nn_mode=3, nn_cells=1, n_cap=4096))[1] == []        # nothing of the search is looked at


def test_row10_refusals_keep_their_codes_and_messages():
    refused(engine(gemm_mode=7 | 64), E_INVALID, "gemm_mode is a mask of 1")
    refused(engine(nn_mode=3), E_INVALID, "nn_mode must be 0")
    refused(engine(gemm_mode=0, nn_mode=0, n_cap=20160), E_UNSUPPORTED, "n_cap too large for the one-pass nearest-neighbour kernel")
    refused(engine(null=("nn_row",)), E_INVALID, "Chamfer term without nearest-neighbour buffers")
    refused(engine(nn_cells=1, n_cap=4096), E_UNSUPPORTED, "nn_cells needs n_cap and t_cap <= 2048")
    refused(engine(nn_cells_wide=1, n_cap=8256), E_UNSUPPORTED, "nn_cells_wide needs n_cap and t_cap <= 8192")
    refused(engine(nn_cells=1, null=("nnc_rec",)), E_INVALID, "nn_cells without its grid buffers")
    refused(engine(gemm_mode=7, null=("gmax",)), E_INVALID, "needs the gmax buffer")
    # wrong in two ways: the earlier check wins, as it did when the checks stood in the launcher
    refused(engine(gemm_mode=7 | 64, nn_mode=3), E_INVALID, "gemm_mode is a mask of 1")
    refused(engine(nn_mode=3, null=("nn_row",)), E_INVALID, "Chamfer term without nearest-neighbour buffers")
    refused(engine(gemm_mode=0, nn_mode=0, n_cap=20160, nn_cells=1), E_UNSUPPORTED, "n_cap too large for the one-pass")
    L = N.lib()
    assert L.ndp_engine_plan(None, (N.StageLaunch * 12)(), ctypes.byref(ctypes.c_int())) == E_INVALID
    assert L.ndp_engine_plan(ctypes.byref(engine()), None, None) == E_INVALID


@pytest.mark.parametrize("gemm_mode", [0, 7, 7 | 1024])
@pytest.mark.parametrize("nn_mode", [0, 1, 2])
@pytest.mark.parametrize("G", [1, 2])
def test_row11_bench_stage_kernels_names_the_plans_kernels(gemm_mode, nn_mode, G):
    import bench
    plan = tick_plan(engine(gemm_mode=gemm_mode, nn_mode=nn_mode, G=G, B=4))
    table = bench.stage_kernels(gemm_mode, nn_mode, G)
    assert list(table) == list(N.TICK_KERNELS)
    assert [[launch[0] for launch in stage] for stage in plan] == [table[k] for k in N.TICK_KERNELS]


def test_the_matrix_search_fits_every_capacity():
    """k_eng_nn_mx8 keeps at most 2048 sources resident: the LDS it asks for stops growing there, below 160 KB."""
    L = N.lib()
    worst = (4 * 64 * 8 + 16 * 64 * 8 + 3 * 16 * 129 + 8 * 32 * 33 + 8 + 2 * 8 * 2 * 64 * 4) * 4
    assert worst == 132320
    for n_cap in (2048, 2112, 8192, 65536):
        assert L.ndp_engine_nn_matrix_fits(n_cap) == 1
        assert tick_plan(engine(n_cap=n_cap))[1] == [("k_eng_nn_mx8", (1, 4, 1), 512, worst, None)]
