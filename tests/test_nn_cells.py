"""GPU tests of the exact grid ball search of the nearest-neighbour stage (csrc/ndp_nn_cells.inc): the standalone entry against the
oracle's brute force for ANY seed indices, an engine with nn_cells against the same engine without, and the default selection.

Everything here is bit-exact: d2 and index, both directions (assert_array_equal / torch.equal)."""
import numpy as np
import pytest
import torch

from tests._helpers import VARIANTS, seeded_pyramid
from tests.test_hip_parity import O, _nn_case, cloud

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


_REF = {}


def _ref(key, x, y):
    """The oracle's answer for a case, computed once and shared."""
    if key not in _REF:
        _REF[key] = O().chamfer(x.numpy(), y.numpy(), want_grad=False, nthreads=8)
    return _REF[key]


def _check_all_seeds(dev, key, x, y):
    """The cell search must give the brute force's bits whatever the previous indices are: none, all -1, the exact answer, seeded
    random in-range garbage, values >= the reference count."""
    from deformationpyramid_amd import ops
    r = _ref(key, x, y)
    S, T = x.shape[0], y.shape[0]
    g = torch.Generator().manual_seed(1234 + S + 7 * T)
    i32 = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.int32).to(dev)
    beyond_x = torch.full((S,), T, dtype=torch.int32); beyond_x[1::2] = T + 5; beyond_x[2::3] = 2 ** 30
    beyond_y = torch.full((T,), S, dtype=torch.int32); beyond_y[1::2] = S + 5; beyond_y[2::3] = 2 ** 30
    seeds = {"null": (None, None),
             "minus_one": (torch.full((S,), -1, dtype=torch.int32).to(dev), torch.full((T,), -1, dtype=torch.int32).to(dev)),
             "exact": (i32(r["idx_x"]), i32(r["idx_y"])),
             "garbage": (torch.randint(0, T, (S,), generator=g, dtype=torch.int32).to(dev), torch.randint(0, S, (T,), generator=g, dtype=torch.int32).to(dev)),
             "beyond": (beyond_x.to(dev), beyond_y.to(dev))}
    xd, yd = x.to(dev), y.to(dev)
    for name, (px, py) in seeds.items():
        d2x, ix, d2y, iy = [t.cpu().numpy() for t in ops.chamfer_nn_cells(xd, yd, px, py)]
        np.testing.assert_array_equal(d2x, r["d2x"], err_msg=f"{key} / {name}")
        np.testing.assert_array_equal(d2y, r["d2y"], err_msg=f"{key} / {name}")
        np.testing.assert_array_equal(ix, r["idx_x"], err_msg=f"{key} / {name}")
        np.testing.assert_array_equal(iy, r["idx_y"], err_msg=f"{key} / {name}")


def _near_ties():
    g = torch.Generator().manual_seed(5)
    d = torch.randn(1500, 3, generator=g); d = d / d.norm(dim=1, keepdim=True)
    y = (torch.tensor([3.0, -2.0, 1.0]) + d * (0.25 + 1e-7 * torch.arange(1500)[:, None])).contiguous()
    x = (torch.tensor([3.0, -2.0, 1.0]) + (torch.rand(900, 3, generator=g) - 0.5) * 1e-3).contiguous()
    return [(x, y), (y[:1100].contiguous(), x)]


def _ragged():
    g = torch.Generator().manual_seed(77)
    x, y = torch.rand(1, 3, generator=g), torch.rand(1, 3, generator=g)
    return [(x, y)] + [(torch.rand(s, 3, generator=g) - 0.5, torch.rand(t, 3, generator=g) - 0.5)
                       for s, t in ((65, 17), (129, 513), (700, 1025), (2000, 1490), (513, 2047))]


@pytest.mark.parametrize("name", ["clusters", "far_queries", "plane", "line", "lattice_ties", "single_ref", "identical", "skewed",
                                  "near_ties", "ragged"])
def test_cell_search_is_exact_on_adversarial_layouts(dev, name):
    """The layouts of test_onepass_nn_is_exact_on_adversarial_layouts that fit the cell search's scope (S, T <= 2048), each with
    every kind of previous indices."""
    cases = _near_ties() if name == "near_ties" else _ragged() if name == "ragged" else [_nn_case(name)]
    for k, (x, y) in enumerate(cases):
        _check_all_seeds(dev, (name, k), x, y)


@pytest.mark.parametrize("name", ["large", "many_sources", "cross_pass_ties"])
def test_cell_search_refuses_more_than_2048_points(dev, name):
    from deformationpyramid_amd import _native as N, ops
    x, y = _nn_case(name)
    assert max(x.shape[0], y.shape[0]) > 2048
    with pytest.raises(N.NdpError, match=r"rc=-2"):                      # NDP_E_UNSUPPORTED
        ops.chamfer_nn_cells(x.to(dev), y.to(dev))
    assert N.lib().ndp_engine_nn_cells_fits(2048, 2048) == 1
    assert N.lib().ndp_engine_nn_cells_fits(2112, 2048) == 0 and N.lib().ndp_engine_nn_cells_fits(2048, 2112) == 0


def _own_case(name):
    g = torch.Generator().manual_seed(4242)
    u = lambda n, s=1.0: (torch.rand(n, 3, generator=g) - 0.5) * s
    if name == "boundaries":
        # Targets on the lattice k / 16 of the unit cube: every coordinate sits exactly on a cell boundary of the 16^3 grid, those with
        # k = 16 on the box's max face.  Queries: lattice mid-points (their ball ends EXACTLY on the boundaries k / 16 on either side),
        # points shifted by 1 / 32 along one axis only, copies of targets (distance 0), and random points.
        k = torch.arange(17, dtype=torch.float32) / 16
        kz = torch.tensor([0.0, 1.0, 2.0, 5.0, 8.0, 15.0, 16.0]) / 16
        y = torch.stack(torch.meshgrid(k, k, kz, indexing="ij"), -1).reshape(-1, 3)                 # 17 * 17 * 7 = 2023
        y = y[torch.randperm(y.shape[0], generator=g)].contiguous()
        mid = y[:600] + 1.0 / 32
        one = y[600:1000].clone(); one[:, 0] += 1.0 / 32
        x = torch.cat([mid, one, y[1000:1400], u(600) + 0.5])
    elif name == "outside_box":          # every source outside the targets' box, on all sides: all of them clamp into border cells
        y = u(1500)
        side = torch.randint(0, 2, (1200, 3), generator=g).float() * 2 - 1
        x = u(1200) * 0.3 + side * torch.tensor([1.5, 4.0, 0.8])
    elif name == "outlier":              # one target at 1e3 stretches the box: all the others share one cell
        y = torch.cat([u(1400), torch.full((1, 3), 1e3)])
        y = y[torch.randperm(y.shape[0], generator=g)].contiguous()
        x = torch.cat([u(900), torch.full((3, 3), 600.0), torch.full((2, 3), 1e3)])
    elif name == "duplicates":           # every point four (three) times, 500 (600) indices apart: equal distances, the lowest index wins
        b = u(500)
        y = torch.cat([b, b, b, b])
        c = u(600)
        x = torch.cat([c, c, b[:200] + 1e-3, c])
    return x.contiguous(), y.contiguous()


@pytest.mark.parametrize("name", ["boundaries", "outside_box", "outlier", "duplicates"])
def test_cell_search_is_exact_at_its_own_edges(dev, name):
    x, y = _own_case(name)
    _check_all_seeds(dev, ("own", name), x, y)


@pytest.mark.parametrize("S,T", [(1, 2048), (2048, 1), (63, 65), (65, 63), (64, 64), (2048, 2048), (1, 1)])
def test_cell_search_sizes(dev, S, T):
    """S or T = 1, 63, 64, 65, 2048: one point, the ends of a wave, the scope's limit."""
    x, y = cloud(S, 900 + S), cloud(T, 1900 + T, 1.3)
    _check_all_seeds(dev, ("size", S, T), x, y)


# ------------------------------------------------------------------------------------------------ engine level
def _engine_pair(seed, S, T, m):
    pyr = seeded_pyramid(seed, m=m, **VARIANTS["se3aa"])
    src = cloud(S, 100 + seed)
    c, s_ = np.cos(0.2), np.sin(0.2)
    Rz = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    tgt = (cloud(T, 200 + seed) @ Rz.T + torch.tensor([0.03, -0.02, 0.01])).contiguous()
    return pyr, src, tgt


@pytest.mark.parametrize("trunc", [1e9, 0.01])
def test_engine_with_cell_search_is_bit_identical(dev, arith, trunc):
    """Two engines that differ in nn_cells only (same nn_mode: the one-pass kernel of the arithmetic), B = 3 pairs of different
    sizes, m = 2 levels of 6 iterations: parameters, Adam moments and pair states are the same BITS after every tick -- across the
    level hand-over, and after slot 1 is refilled in mid-flight with a pair of a smaller T and S (the slot's index buffers then hold
    the old pair's indices: some >= the new T / S, the others in range but meaningless)."""
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    m, iters = 2, 6
    sizes = [(450, 480), (500, 390), (310, 333)]
    cfg = OptConfig(m=m, iters=iters, early_stop=False, w_cd=1.0, trunc=trunc)
    modes = dict(gemm_mode=7, nn_mode=2) if arith == "split" else dict(gemm_mode=0, nn_mode=0)
    pairs = [_engine_pair(7 + b, S, T, m) for b, (S, T) in enumerate(sizes)]
    refill = _engine_pair(31, 290, 260, m)
    d = pairs[0][0].descs[0]
    engs = [BatchedEngine(d, cfg, 3, n_cap=512, t_cap=512, device=dev, nn_cells=flag, **modes) for flag in (True, False)]
    assert engs[0].c_engine.nn_cells == 1 and engs[1].c_engine.nn_cells == 0
    assert engs[0].c_engine.nn_mode == engs[1].c_engine.nn_mode == modes["nn_mode"]
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
    # the cell search's own rows and columns against the dense kernel's (slot 1: the refilled pair)
    a, b = engs
    for slot, (S, T) in ((0, sizes[0]), (1, (290, 260)), (2, sizes[2])):
        assert torch.equal(a.idx_y[slot, :T], b.idx_y[slot, :T]) and torch.equal(a.d2y[slot, :T], b.d2y[slot, :T])
        assert torch.equal(a.idx_x[slot, :S], b.idx_x[slot, :S]) and torch.equal(a.d2x[slot, :S], b.d2x[slot, :S])
        assert bool((a.idx_y[slot, T:] == -1).all())


def test_cell_search_is_the_default_where_the_engine_picks_a_one_pass_shape(dev):
    from deformationpyramid_amd import _native as N
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    d = seeded_pyramid(3, m=1, **VARIANTS["se3aa"]).descs[0]
    cfg = OptConfig(m=1, iters=2, early_stop=False)
    eng = BatchedEngine(d, cfg, 256, n_cap=256, t_cap=256, device=dev)
    assert eng.nn_mode in (0, 2) and eng.nn_cells and eng.c_engine.nn_cells == 1
    del eng
    eng = BatchedEngine(d, cfg, 256, n_cap=256, t_cap=256, device=dev, nn_mode=2)
    assert eng.nn_mode == 2 and not eng.nn_cells and eng.c_engine.nn_cells == 0
    del eng
    eng = BatchedEngine(d, cfg, 32, n_cap=4096, t_cap=4096, device=dev)
    assert eng.nn_mode in (0, 2) and not eng.nn_cells and eng.c_engine.nn_cells == 0
    del eng
    with pytest.raises(N.NdpError, match="nn_cells"):
        BatchedEngine(d, cfg, 32, n_cap=4096, t_cap=4096, device=dev, nn_cells=True)
