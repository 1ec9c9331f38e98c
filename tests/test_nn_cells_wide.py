"""GPU tests of the grid ball search for clouds of up to 8192 points (csrc/ndp_nn_cells_wide.inc): the standalone entry against the
oracle's brute force for ANY seed indices, an engine with nn_cells_wide against the same engine without, a slot's independence of
its history, the default selection and the public API.

Everything here is bit-exact: d2 and index, both directions (assert_array_equal / torch.equal).

The kernels' boundaries that the sizes below straddle: a search workgroup answers 2048 queries (chunks end at 2048, 4096, 6144), its
1024 threads take two each (1024), every copy and sort loop strides by 1024 threads, a wave is 64 lanes, the scope ends at 8192."""
import contextlib

import numpy as np
import pytest
import torch

from tests import test_nn_cells as small
from tests import test_slot_history as hist
from tests._helpers import VARIANTS, seeded_pyramid
from tests.test_hip_parity import _nn_case, cloud

pytestmark = pytest.mark.gpu

# the wide search keeps its grids in the engine's three grid buffers (include/ndp_hip.h: nnc_start [B][2][.], nnc_rec [B][t_cap + n_cap][4]):
# they are on test_slot_history's poison list, so its poison() overwrites them in a wide engine as it does in an nn_cells engine
GRID_BUFFERS = ("nnc_geom", "nnc_start", "nnc_rec")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


@contextlib.contextmanager
def _wide_entry():
    """test_nn_cells._check_all_seeds (the five seed sets: none, all -1, the exact answer, in-range garbage, values >= the reference
    count, each compared with the oracle's brute force bit for bit) calls ops.chamfer_nn_cells: here that name is the wide entry."""
    from deformationpyramid_amd import ops
    saved = ops.chamfer_nn_cells
    ops.chamfer_nn_cells = ops.chamfer_nn_cells_wide
    try:
        yield
    finally:
        ops.chamfer_nn_cells = saved


def _check_all_seeds(dev, key, x, y):
    with _wide_entry():
        small._check_all_seeds(dev, ("wide",) + tuple(key), x, y)


# ------------------------------------------------------------------------------------------------ standalone entry
SIZES = [(1, 8192), (8192, 1), (8192, 8192), (1, 1), (63, 65), (65, 63), (64, 64),
         (2049, 2047), (2047, 2049), (2048, 2048),              # the old limit = the first chunk's end
         (1023, 1025), (1025, 1023), (1024, 1024),              # threads of a workgroup / stride of the copy and sort loops
         (4095, 4097), (4097, 4095), (4096, 4096),              # second chunk's end
         (6143, 6145), (6145, 6143), (6144, 6144),              # third chunk's end
         (8191, 8192), (8192, 8191)]                            # one below the scope's end


@pytest.mark.parametrize("S,T", SIZES)
def test_wide_cell_search_sizes(dev, S, T):
    x, y = cloud(S, 900 + S), cloud(T, 1900 + T, 1.3)
    _check_all_seeds(dev, ("size", S, T), x, y)


@pytest.mark.parametrize("name", ["many_sources", "cross_pass_ties", "lattice_ties", "identical", "single_ref"])
def test_wide_cell_search_is_exact_on_adversarial_layouts(dev, name):
    x, y = _nn_case(name)
    _check_all_seeds(dev, (name,), x, y)


def _own_case(name):
    g = torch.Generator().manual_seed(8192)
    u = lambda n, s=1.0: (torch.rand(n, 3, generator=g) - 0.5) * s
    if name == "boundaries":
        # 17 x 17 x 28 = 8092 targets: x and y on the lattice k / 16 of the unit cube -- exactly on the cell boundaries of the 16^3 grid, k = 16
        # on the box's max face -- and z on 28 of the values k / 32 (all 17 boundaries and 11 cell centres).  Queries as in
        # test_nn_cells._own_case("boundaries"): lattice mid-points (the ball ends EXACTLY on boundaries on either side), points shifted by
        # 1 / 32 along one axis only, copies of targets (distance 0), and random points.
        k = torch.arange(17, dtype=torch.float32) / 16
        kz = torch.cat([torch.arange(17, dtype=torch.float32) * 2, torch.tensor([1.0, 3, 7, 9, 15, 17, 21, 25, 27, 29, 31])]) / 32
        y = torch.stack(torch.meshgrid(k, k, kz, indexing="ij"), -1).reshape(-1, 3)
        assert y.shape[0] == 8092
        y = y[torch.randperm(y.shape[0], generator=g)].contiguous()
        mid = y[:2400] + 1.0 / 32
        one = y[2400:4000].clone(); one[:, 0] += 1.0 / 32
        x = torch.cat([mid, one, y[4000:5600], u(2400) + 0.5])
    elif name == "outside_box":          # every source outside the targets' box, on all sides: all of them clamp into border cells
        y = u(6000)
        side = torch.randint(0, 2, (5000, 3), generator=g).float() * 2 - 1
        x = u(5000) * 0.3 + side * torch.tensor([1.5, 4.0, 0.8])
    elif name == "outlier":              # one target at 1e3 stretches the box: all the others share one cell
        y = torch.cat([u(7000), torch.full((1, 3), 1e3)])
        y = y[torch.randperm(y.shape[0], generator=g)].contiguous()
        x = torch.cat([u(4500), torch.full((3, 3), 600.0), torch.full((2, 3), 1e3)])
    elif name == "duplicates":           # every target four times, 2000 indices apart (one copy per chunk of the columns): the lowest index wins
        b = u(2000)
        y = torch.cat([b, b, b, b])
        c = u(2000)
        x = torch.cat([c, c, b[:1000] + 1e-3, c])
    return x.contiguous(), y.contiguous()


@pytest.mark.parametrize("name", ["boundaries", "outside_box", "outlier", "duplicates"])
def test_wide_cell_search_is_exact_at_its_own_edges(dev, name):
    x, y = _own_case(name)
    _check_all_seeds(dev, ("own", name), x, y)


def test_wide_cell_search_refuses_more_than_8192_points(dev):
    from deformationpyramid_amd import _native as N, ops
    x, y = _nn_case("large")
    assert y.shape[0] == 9000
    with pytest.raises(N.NdpError, match=r"rc=-2"):                      # NDP_E_UNSUPPORTED
        ops.chamfer_nn_cells_wide(x.to(dev), y.to(dev))
    with pytest.raises(N.NdpError, match=r"rc=-2"):
        ops.chamfer_nn_cells_wide(y.to(dev), x.to(dev))


# ------------------------------------------------------------------------------------------------ engine level
@pytest.mark.parametrize("trunc", [1e9, 0.01])
def test_engine_with_wide_cell_search_is_bit_identical(dev, arith, trunc):
    """Two engines that differ in nn_cells_wide only (same explicit nn_mode: the one-pass kernel of the arithmetic), B = 3 pairs of
    different sizes above 2048 points, m = 2 levels of 6 iterations: parameters, Adam moments and pair states are the same BITS after
    every tick -- across the level hand-over, and after slot 1 is refilled in mid-flight with a smaller pair (the slot's index buffers
    then hold the old pair's indices: some >= the new T / S, the others in range but meaningless)."""
    from deformationpyramid_amd import _native as N
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    m, iters = 2, 6
    sizes = [(4100, 3900), (2100, 4160), (3000, 2049)]
    small_pair = (1900, 1500)
    cfg = OptConfig(m=m, iters=iters, early_stop=False, w_cd=1.0, trunc=trunc)
    modes = dict(gemm_mode=7, nn_mode=2) if arith == "split" else dict(gemm_mode=0, nn_mode=0)
    pairs = [small._engine_pair(7 + b, S, T, m) for b, (S, T) in enumerate(sizes)]
    refill = small._engine_pair(31, *small_pair, m)
    d = pairs[0][0].descs[0]
    engs = [BatchedEngine(d, cfg, 3, n_cap=4160, t_cap=4160, device=dev, nn_cells_wide=flag, **modes) for flag in (True, False)]
    assert engs[0].c_engine.nn_cells_wide == 1 and engs[1].c_engine.nn_cells_wide == 0
    assert engs[0].nn_cells_wide and not engs[1].nn_cells_wide
    assert not engs[0].nn_cells and not engs[1].nn_cells and engs[0].c_engine.nn_cells == engs[1].c_engine.nn_cells == 0
    assert engs[0].c_engine.nn_mode == engs[1].c_engine.nn_mode == modes["nn_mode"]
    assert not hasattr(engs[1], "nnc_rec")                  # the buffers exist only where a search is on
    assert tuple(engs[0].nnc_start.shape) == (3, 2, N.NNC_START) and tuple(engs[0].nnc_rec.shape) == (3, 2 * 4160, 4)
    for eng in engs:
        for b, (pyr, src, tgt) in enumerate(pairs):
            eng.load(b, src, 0, src.shape[0], None, tgt, pyr.store)

    def same(tick):
        a, b = engs
        for name in ("params", "adam_m", "adam_v"):
            assert torch.equal(getattr(a, name), getattr(b, name)), (name, tick)
        assert torch.equal(a.state[a.tick & 1], b.state[b.tick & 1]), ("state", tick)

    levels_seen = set()
    for tick in range(2 * iters + 9):
        if tick == iters + 2:                              # slot 1 is in its second level: refill it with another, smaller pair
            for eng in engs:
                pyr, src, tgt = refill
                eng.load(1, src, 0, src.shape[0], None, tgt, pyr.store)
        for eng in engs:
            eng.run_ticks(1)
        same(tick)
        levels_seen.add(engs[0].read_states()[0].level)
    assert levels_seen == {0, 1, 2}                        # the hand-over and the end were both crossed
    for st in engs[0].read_states():
        assert st.level == m and st.total_steps == m * iters
    a, b = engs
    for slot, (S, T) in ((0, sizes[0]), (1, small_pair), (2, sizes[2])):
        assert torch.equal(a.idx_y[slot, :T], b.idx_y[slot, :T]) and torch.equal(a.d2y[slot, :T], b.d2y[slot, :T])
        assert torch.equal(a.idx_x[slot, :S], b.idx_x[slot, :S]) and torch.equal(a.d2x[slot, :S], b.d2x[slot, :S])
        assert bool((a.idx_y[slot, T:] == -1).all())


def test_engine_refuses_both_searches_and_missing_wide_buffers(dev):
    from deformationpyramid_amd import _native as N
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    pyr, src, tgt = small._engine_pair(5, 300, 280, 1)
    cfg = OptConfig(m=1, iters=2, early_stop=False)
    with pytest.raises(N.NdpError, match="nn_cells_wide"):
        BatchedEngine(pyr.descs[0], cfg, 2, n_cap=512, t_cap=512, device=dev, nn_cells=True, nn_cells_wide=True)
    eng = BatchedEngine(pyr.descs[0], cfg, 2, n_cap=512, t_cap=512, device=dev, nn_mode=2, nn_cells_wide=True)
    eng.park_all()
    eng.c_engine.nn_cells = 1                               # both flags in the C struct
    with pytest.raises(N.NdpError, match=r"rc=-1.*nn_cells_wide"):        # NDP_E_INVALID
        eng.run_ticks(1)
    with pytest.raises(N.NdpError, match=r"rc=-1.*nn_cells_wide"):
        eng.load(0, src, 0, src.shape[0], None, tgt, pyr.store)
    eng.c_engine.nn_cells = 0
    for name in GRID_BUFFERS:
        keep = getattr(eng.c_engine, name)
        setattr(eng.c_engine, name, None)                   # a missing buffer
        with pytest.raises(N.NdpError, match=r"rc=-1.*grid buffers"):
            eng.run_ticks(1)
        if name != "nnc_geom":                              # (eight floats per pair: no alignment asked, as for nn_cells)
            setattr(eng.c_engine, name, keep + 4)           # a misaligned one
            with pytest.raises(N.NdpError, match=r"rc=-1.*grid buffers"):
                eng.run_ticks(1)
        setattr(eng.c_engine, name, keep)
    eng.run_ticks(1)                                        # the intact struct runs
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ a slot's history
def _assert_poison_reaches_the_grids(eng):
    """test_slot_history.poison names the buffers it overwrites; the wide engine's grids must be among those it finds."""
    for name in GRID_BUFFERS:
        assert name in hist.ENGINE_POISONED and getattr(eng, name).data_ptr() == getattr(eng.c_engine, name), name
        t = getattr(eng, name)
        bad = torch.isnan(t).all() if t.dtype == torch.float32 else (t.view(-1)[3::4] == 0x7fffffff).all()
        assert bool(bad), name


WIDE_NN = dict(nn_cells=False, nn_cells_wide=True)


@pytest.mark.parametrize("arith_name", ["fp32", "split_fused"])
def test_a_pairs_trace_in_a_wide_engine_does_not_depend_on_the_slots_history(dev, arith_name):
    """The matrix of test_slot_history (its engines, pairs, histories and trace, imported) with the wide search in the NN slot: every
    history -- all engine buffers INCLUDING the wide search's grids (they are on that file's poison list) overwritten with NaN / 0x7f7f7f7f / out-of-range integers, a larger
    pair in mid-flight at either parity or finished -- reproduces the pair's trace in a fresh engine, bit for bit and tick by tick."""
    kind = hist.ARITH[arith_name][0]
    lived = {h: hist._engine(dev, arith_name, None, WIDE_NN) for h in hist.FULL_HISTORIES}
    for k, shape in enumerate(hist.PAIRS[:2] + hist.PAIRS[4:]):
        it = hist._item(dev, kind, shape, 11 + k)
        eng, want = hist.fresh_trace(dev, arith_name, None, WIDE_NN, it)
        assert eng.c_engine.nn_cells_wide == 1 and eng.c_engine.nn_cells == 0 and eng.nn_cells_wide and not eng.nn_cells
        sts = hist.states_of(eng, hist.SLOT, want)
        assert sts[-1].level == hist.M and sts[-1].decision == hist.DEC_IDLE, (shape, sts[-1].level)
        for h in hist.FULL_HISTORIES:
            got = hist.run_history(h, lived[h], dev, it, k)
            hist.assert_same_trace(want, got, eng, hist.SLOT, f"wide {arith_name} pair {shape} after {h}")


def test_a_pairs_trace_across_query_chunks_does_not_depend_on_the_slots_history(dev):
    """The same property where a direction's queries span two workgroups (capacity 2176, pair of 2100 / 2060 points): fresh engine
    against poisoned buffers and against a slot that held a larger pair (2176 / 2176, every head x 20) in mid-flight."""
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    m, iters, n_ticks, CAP = 2, 4, 10, 2176
    kind, modes, _ = hist.ARITH["split_fused"]
    desc = hist._pyramid(kind, 0, m, None, 1.0).descs[m - 1]
    cfg = OptConfig(m=m, iters=iters, early_stop=True, w_cd=0.5, trunc=0.05, break_threshold_ratio=hist.RATIO, max_break_count=hist.BREAKS)

    def engine():
        eng = BatchedEngine(desc, cfg, 2, n_cap=CAP, t_cap=CAP, device=dev, **modes, **WIDE_NN)
        assert eng.c_engine.nn_cells_wide == 1
        eng.park_all()
        return eng

    it = hist._item(dev, kind, (0, 2100, 2060), 21, m=m)
    prev = hist._item(dev, kind, (0, CAP, CAP), 22, m=m, scale_level=-1)
    eng = engine()
    hist._load(eng, hist.SLOT, it)
    want = hist.trace(eng, hist.SLOT, n_ticks)
    assert hist.states_of(eng, hist.SLOT, want)[-1].level == m
    for kind_ in ("nan", "big"):
        e2 = engine()
        hist.poison(e2, kind_)
        if kind_ == "nan":
            _assert_poison_reaches_the_grids(e2)
        e2.park_all()
        hist._load(e2, hist.SLOT, it)
        hist.assert_same_trace(want, hist.trace(e2, hist.SLOT, n_ticks), eng, hist.SLOT, f"two chunks after poison {kind_}")
    e3 = engine()
    hist._load(e3, hist.SLOT, prev)
    hist._run_until(e3, hist.SLOT, lambda s: s.level == 1 and s.iter >= 1, 3 * iters)      # the larger pair is inside its second level
    hist._load(e3, hist.SLOT, it)
    hist.assert_same_trace(want, hist.trace(e3, hist.SLOT, n_ticks), eng, hist.SLOT, "two chunks after a larger pair in mid-flight")


# ------------------------------------------------------------------------------------------------ selection, public API
def test_wide_cell_search_selection(dev):
    from deformationpyramid_amd import _native as N
    from deformationpyramid_amd import engine
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    d = seeded_pyramid(3, m=1, **VARIANTS["se3aa"]).descs[0]
    cfg = OptConfig(m=1, iters=2, early_stop=False)
    eng = BatchedEngine(d, cfg, 32, n_cap=4096, t_cap=4096, device=dev)
    assert eng.nn_mode in (0, 2) and eng.nn_cells_wide == engine.DEFAULT_NN_CELLS_WIDE and not eng.nn_cells
    assert eng.c_engine.nn_cells == 0 and eng.c_engine.nn_cells_wide == int(engine.DEFAULT_NN_CELLS_WIDE)
    del eng
    eng = BatchedEngine(d, cfg, 32, n_cap=4096, t_cap=4096, device=dev, nn_mode=2)         # an explicit nn_mode switches it off
    assert eng.nn_mode == 2 and not eng.nn_cells_wide and eng.c_engine.nn_cells_wide == 0
    del eng
    eng = BatchedEngine(d, cfg, 2, n_cap=4096, t_cap=4096, device=dev)                     # few pairs: the latency shape, no search
    assert eng.nn_mode == 1 and not eng.nn_cells_wide and not eng.nn_cells
    del eng
    eng = BatchedEngine(d, cfg, 256, n_cap=256, t_cap=256, device=dev)                     # <= 2048: the old search keeps the stage
    assert eng.nn_cells and eng.c_engine.nn_cells == 1 and not eng.nn_cells_wide and eng.c_engine.nn_cells_wide == 0
    del eng
    with pytest.raises(N.NdpError, match="nn_cells_wide"):
        BatchedEngine(d, cfg, 2, n_cap=8256, t_cap=8256, device=dev, nn_cells_wide=True)


def test_register_batch_with_and_without_the_wide_search_gives_the_same_bits(dev):
    import os

    from deformationpyramid_amd.config import Config, load_config
    from deformationpyramid_amd.registration import Registration
    from deformationpyramid_amd.synthetic import synthetic_pair
    c = Config(load_config(os.path.join(hist.ROOT, "config", "NDP.yaml"), device=0), samples=2500, m=3, iters=30)
    pairs = [synthetic_pair(70 + p)[:2] for p in range(3)]
    out = []
    for flag in (True, False):
        torch.manual_seed(9)
        model = Registration(c, nn_cells_wide=flag)
        out.append(model.register_batch(pairs, slots=3, prefetch=False))
        e = model._engines[0]
        assert bool(e.nn_cells_wide) is flag and e.c_engine.nn_cells_wide == int(flag) and not e.nn_cells
        assert e.n_cap > 2048
    hist._assert_same_results(out[0], out[1])
