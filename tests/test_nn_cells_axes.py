"""The cell search (csrc/ndp_nn_cells.inc) with its own cell count per axis and its one-key (d2, index) minimum, against the brute force
k_nn (ops.chamfer_nn) on the same device: d2 and index of both directions with torch.equal, for every kind of seed -- none, the exact
answer, stale indices in range, indices >= the reference count.  The inputs sit where a per-axis grid or the key could go wrong: box
extents 1 : 1e-3 : 0, a flat cloud, all targets in one cell, fewer targets than the fine axis has cells, sources far outside the box on
both sides of the fine axis, duplicated targets (ties -> the lowest index), a NaN query coordinate (never wins: d2 = +inf, index -1) and
a query at 3e38 from everything (d2 = +inf, index -1).

test_inputs_contain_their_cases needs no GPU: a float32 brute force on the CPU shows that each input really holds its tie, NaN or inf."""
import numpy as np
import pytest
import torch

from tests._helpers import VARIANTS, seeded_pyramid

FINE = 64                                             # cells of the fine axis (x) of the search's grid


def _u(g, n, s=1.0):
    return (torch.rand(n, 3, generator=g) - 0.5) * s


def _case(name):
    g = torch.Generator().manual_seed(977)
    if name == "s70_t130":
        x, y = _u(g, 70), _u(g, 130, 1.2)
    elif name == "s2048_t2047":
        x, y = _u(g, 2048), _u(g, 2047, 1.1) + 0.02
    elif name == "extents_1_1e-3_0":                  # the targets' box is 1 x 1e-3 x 0
        y = _u(g, 1500) * torch.tensor([1.0, 1e-3, 0.0]) + torch.tensor([0.1, -0.2, 0.3])
        x = torch.cat([_u(g, 700) * torch.tensor([1.0, 1e-3, 0.0]) + torch.tensor([0.1, -0.2, 0.3]), _u(g, 300, 1.5)])
    elif name == "flat":                              # y is constant over the targets AND the sources
        y = _u(g, 1300); y[:, 1] = 0.25
        x = _u(g, 1100, 1.2); x[:, 1] = 0.25
    elif name == "one_cell":                          # one target far away stretches the box: all the others share cell (0, 0, 0)
        y = torch.cat([_u(g, 999, 1e-3), torch.full((1, 3), 100.0)])
        x = torch.cat([_u(g, 600, 2e-3), _u(g, 200, 50.0) + 50.0])
    elif name == "one_point":                         # every target the same point: extent 0 on every axis, one cell, ties everywhere
        y = torch.tensor([[0.3, -0.1, 0.7]]).repeat(300, 1)
        x = _u(g, 400)
    elif name == "t_below_fine":                      # fewer targets than the fine axis has cells
        x, y = _u(g, 900), _u(g, 5)
        assert y.shape[0] < FINE
    elif name == "outside_fine_axis":                 # sources far beyond the box on both sides of x (the fine axis), inside it in y and z
        y = _u(g, 1400)
        x = _u(g, 1000)
        x[:500, 0] -= 40.0
        x[500:, 0] += 40.0
    elif name == "duplicates":                        # every target three times, 400 indices apart
        b = _u(g, 400)
        y = torch.cat([b, b, b])
        x = torch.cat([_u(g, 500), b[:100]])
    elif name == "nan_query":                         # one source coordinate is NaN
        x, y = _u(g, 800), _u(g, 1000)
        x[411, 1] = float("nan")
    elif name == "inf_distance":                      # one source at 3e38 from everything: its squared distance overflows
        x, y = _u(g, 800), _u(g, 1000)
        x[123] = torch.tensor([3e38, 0.0, 0.0])
    else:
        raise KeyError(name)
    return x.contiguous(), y.contiguous()


CASES = ["s70_t130", "s2048_t2047", "extents_1_1e-3_0", "flat", "one_cell", "one_point", "t_below_fine", "outside_fine_axis", "duplicates",
         "nan_query", "inf_distance"]


def _brute(q, r):
    """float32 chain fmaf(dz, dz, fmaf(dy, dy, dx * dx)) through float64 (each product of two float32 is exact in float64; the sums round
    once more than the chain does only where that cannot change a tie, an inf or a NaN) -> d2 [nq][nr]"""
    d = (q[:, None, :] - r[None, :, :]).astype(np.float32).astype(np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        t = (d[..., 0] * d[..., 0]).astype(np.float32).astype(np.float64)
        t = (d[..., 1] * d[..., 1] + t).astype(np.float32).astype(np.float64)
        return (d[..., 2] * d[..., 2] + t).astype(np.float32)


def test_inputs_contain_their_cases():
    f = lambda name: [t.numpy() for t in _case(name)]
    x, y = f("duplicates")
    d = _brute(x, y)
    assert ((d == d.min(1, keepdims=True)).sum(1) >= 3).all()           # every source: at least a three-way tie for the minimum
    assert (d[500:].min(1) == 0).all() and (d[500:].argmin(1) < 400).all()
    x, y = f("one_point")
    d = _brute(x, y)
    assert (d == d[:, :1]).all() and np.ptp(y, 0).max() == 0
    x, y = f("nan_query")
    d = _brute(x, y)
    assert np.isnan(d[411]).all() and np.isfinite(np.delete(d, 411, 0)).all()
    x, y = f("inf_distance")
    d = _brute(x, y)
    assert np.isposinf(d[123]).all() and np.isfinite(np.delete(d, 123, 0)).all()
    x, y = f("extents_1_1e-3_0")
    e = np.ptp(y, 0)
    assert 0.9 < e[0] <= 1 and 0.9e-3 < e[1] <= 1e-3 and e[2] == 0
    x, y = f("flat")
    assert np.ptp(y, 0)[1] == 0 and np.ptp(x, 0)[1] == 0
    x, y = f("one_cell")
    lo, e = y.min(0), np.ptp(y, 0)
    assert (np.floor((y[:-1] - lo) * (np.array([FINE, 8, 8], np.float32) / e)) == 0).all()   # whatever the axis' count up to 64: cell 0
    x, y = f("outside_fine_axis")
    assert (x[:500, 0] < y[:, 0].min() - 30).all() and (x[500:, 0] > y[:, 0].max() + 30).all()
    assert (np.abs(x[:, 1:]) <= 0.5).all()


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


def _seeds(S, T, ref, dev):
    g = torch.Generator().manual_seed(31 + S + 7 * T)
    beyond_x = torch.full((S,), T, dtype=torch.int32); beyond_x[1::2] = T + 5; beyond_x[2::3] = 2 ** 30
    beyond_y = torch.full((T,), S, dtype=torch.int32); beyond_y[1::2] = S + 5; beyond_y[2::3] = 2 ** 30
    # (the exact answer holds -1 where there is no neighbour: a negative seed is "no seed")
    return {"none": (None, None),
            "exact": (ref[1].clone(), ref[3].clone()),
            "stale_in_range": (torch.randint(0, T, (S,), generator=g, dtype=torch.int32).to(dev),
                               torch.randint(0, S, (T,), generator=g, dtype=torch.int32).to(dev)),
            "beyond": (beyond_x.to(dev), beyond_y.to(dev))}


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_cell_search_equals_the_brute_force(dev, name):
    from deformationpyramid_amd import ops
    x, y = [t.to(dev) for t in _case(name)]
    S, T = x.shape[0], y.shape[0]
    ref = ops.chamfer_nn(x, y)                                          # k_nn: computed once per case
    if name == "nan_query":
        assert ref[1][411].item() == -1 and ref[0][411].item() == float("inf")
    if name == "inf_distance":
        assert ref[1][123].item() == -1 and ref[0][123].item() == float("inf")
    if name == "duplicates":
        assert int(ref[1].max()) < 400                                  # the lowest of the three equal indices
    for seed, (px, py) in _seeds(S, T, ref, dev).items():
        out = ops.chamfer_nn_cells(x, y, px, py)
        for what, a, b in zip(("d2x", "idx_x", "d2y", "idx_y"), out, ref):
            assert torch.equal(a, b), (name, seed, what)


@pytest.mark.gpu
def test_engine_ticks_with_the_cell_search_equal_the_brute_force(dev):
    """Three pairs in an engine with nn_cells, the forward and the NN stage of three ticks (the first without seeds, the others seeded by
    the tick before): the stage's rows and columns are k_nn's of the warped sources the forward left, bit for bit."""
    from deformationpyramid_amd import ops
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    m = 1
    cfg = OptConfig(m=m, iters=6, early_stop=False, w_cd=1.0)
    pyr = seeded_pyramid(11, m=m, **VARIANTS["se3aa"])
    pairs = [_case("s70_t130"), _case("s2048_t2047"), _case("extents_1_1e-3_0")]
    eng = BatchedEngine(pyr.descs[0], cfg, 3, n_cap=2048, t_cap=2048, device=dev, nn_cells=True)
    assert eng.c_engine.nn_cells == 1
    for b, (x, y) in enumerate(pairs):
        eng.load(b, x, 0, x.shape[0], None, y, pyr.store)
    seen = []
    for tick in range(3):
        cur = [st.cur for st in eng.read_states()]
        eng.run_stages(0, 1)
        for b, (x, y) in enumerate(pairs):
            S, T = x.shape[0], y.shape[0]
            xw = eng.pts[b, cur[b] ^ 1, :S].contiguous()
            ref = ops.chamfer_nn(xw, y.to(dev))
            if b == 0:
                seen.append(xw.clone())
            got = (eng.d2x[b, :S], eng.idx_x[b, :S], eng.d2y[b, :T], eng.idx_y[b, :T])
            for what, a, r in zip(("d2x", "idx_x", "d2y", "idx_y"), got, ref):
                assert torch.equal(a, r), (tick, b, what)
            assert bool((eng.idx_y[b, T:] == -1).all())
        eng.run_stages(2, 5)
    assert not torch.equal(seen[0], seen[2])                            # the warped sources did move between the ticks
