"""Preconditions of tests/test_nsfp_edges.py, checked without a GPU: the restatement of tests/_nsfp_ref.py is the reference's network
(the C oracle and fixture F12 say so), and the inputs it builds meet the conditions the float32 / float64 comparison rests on: no ReLU
within the kink margin, few candidates left out, weights loud enough that the flow depends on x, and gradients in which one dropped
tail row or one misplaced tile would show far above the bar."""
import numpy as np
import pytest
import torch

from oracle import ndp_oracle as O
from tests import _nsfp_ref as B

MAX_DROPPED_SHARE = 0.05
NSFP_INPUTS = sorted({("loud", n) for n in B.NSFP_FWD_N} | {("loud", n) for n, _ in B.NSFP_BWD_CASES})


def test_case_lists():
    assert B.NSFP_FWD_N == (1, 63, 64, 65, 257)
    assert B.NSFP_BWD_CASES == [(1, None), (1, 3), (64, 1), (65, 1), (65, 2), (65, 5), (257, 1), (257, 3), (257, 7), (257, None)]
    assert B.NSFP_STRIDE_N == 512 * 64 + 65 == 32833 and B.NSFP_DEFAULT_N == 65
    assert B.NSFP_PADDING_N == (65, 257) and B.POISON == (3.0e4, -3.0e4) and B.KINK_MARGIN == 1e-5
    tiles = lambda n: (n + 63) // 64
    assert [c for c in B.NSFP_BWD_CASES if c[1] is not None and c[1] > tiles(c[0])] == [(1, 3), (65, 5), (257, 7)]
    assert B.P_COUNT == O.NSFP_P == 116483 and len(B.names()) == 18


# ------------------------------------------------------------------------------------------ the restatement is the reference's network
def f12_model(g):
    from deformationpyramid_amd.nsfp import Neural_Prior
    torch.manual_seed(21)
    m = Neural_Prior()
    for k, v in m.named_parameters():
        if k.endswith("weight"):
            v.mul_(float(g["fb.scale"]))                                         # as tests/test_nsfp.py builds it
    return m


def test_float32_restatement_reproduces_the_nsfp_fixture(golden):
    """F12 at the bounds tests/test_nsfp.py holds the oracle to; the Chamfer gradient in the warped points is the oracle's."""
    g = golden("F12_nsfp")
    m = f12_model(g)
    assert [k for k, _ in m.named_parameters()] == B.names() == list(g["names"])
    x, y = torch.from_numpy(g["fb.x"]), g["fb.y"]
    out = B.nsfp(m.flat, x).out
    r = O.chamfer(out.numpy(), y, trunc=1e9)
    assert abs(r["loss"] - g["fb.loss"]) < 2e-6 * g["fb.loss"]
    res = B.nsfp(m.flat, x, torch.from_numpy(r["gx"]))
    assert np.abs(res.flow.numpy() - g["fb.flow"]).max() < 2e-6
    assert np.abs((res.out - x).numpy() - g["fb.flow"]).max() < 2e-6
    for name, gr in zip(B.names(), B.split(res.grad)):
        ref = g[f"fb.grad.{name}"].reshape(-1)
        got = gr.numpy().reshape(-1)
        got = got if ref.size == got.size else got[::37]
        assert np.abs(got - ref).max() < 2e-4 * np.abs(ref).max() + 1e-9, name
        assert abs(gr.numpy().astype(np.float64).sum() - g[f"fb.gsum.{name}"]) < 1e-3 * g[f"fb.gabs.{name}"] + 1e-9, name


@pytest.mark.parametrize("kind,n", [("default", 200), ("loud", 65), ("loud", 257)])
def test_float32_restatement_agrees_with_the_oracle(kind, n):
    """oracle/ndp_oracle.c is another float32 evaluation of the same network: output and gradients within the project's bar of float64,
    and of the eager restatement."""
    flat = B.nsfp_flat(kind)
    x = B.uniform_points(n, 3) if kind == "default" else B.kink_free_points(kind, n)[0]
    gy = B.upstream_gradient(n)
    r64, r32 = B.nsfp_pair(flat, x, gy)
    out = torch.from_numpy(O.nsfp_fwd(flat.numpy(), x.numpy(), nthreads=4))
    assert float((out - r32.out).abs().max()) < 2e-6
    pairs = [("out", out, r32.out, r64.out), ("flow", out.double() - x.double(), r32.flow, r64.flow)]
    if kind == "loud":                                                           # (gradients need the kink-free points)
        grads = torch.from_numpy(O.nsfp_bwd(flat.numpy(), x.numpy(), gy.numpy()))
        pairs += [(k, a, b, c) for k, a, b, c in zip(B.names(), B.split(grads), B.split(r32.grad), B.split(r64.grad))]
    for what, theirs, mine, ref in pairs:
        B.check(f"C oracle {kind} n={n} {what}", theirs, ref, mine)


# ------------------------------------------------------------------------------------------ the inputs
@pytest.mark.parametrize("kind,n", NSFP_INPUTS, ids=lambda v: str(v))
def test_nsfp_inputs_are_kink_free(kind, n):
    x, candidates, dropped = B.kink_free_points(kind, n)
    print(f"nsfp {kind} n={n}: {dropped} of {candidates} candidates dropped ({100.0 * dropped / candidates:.2f} %)")
    assert x.shape == (n, 3) and x.dtype == torch.float32 and x.abs().max() <= 0.5 and candidates >= 1024
    assert dropped <= MAX_DROPPED_SHARE * candidates
    r64, r32 = B.nsfp_pair(B.nsfp_flat(kind), x)
    assert len(r64.zs) == 8 and all(z.shape == (n, 128) for z in r64.zs)
    for z64, z32 in zip(r64.zs, r32.zs):
        assert z64.abs().min() > B.KINK_MARGIN
        assert torch.equal(z64 > 0, z32 > 0)
        assert (z32.double() - z64).abs().max() < B.KINK_MARGIN / 10             # the margin is an order above float32's own z error


def test_default_case_is_the_workload_regime():
    """Unfiltered points (tests/_nsfp_ref.default_points says why): the flow is nearly constant, and the eager float32 forward is as
    accurate on them as on filtered ones."""
    x = B.default_points()
    r64, r32 = B.nsfp_pair(B.nsfp_flat("default"), x)
    assert x.shape == (B.NSFP_DEFAULT_N, 3) and x.abs().max() <= 0.5
    assert r64.flow.abs().max() < 0.1 and r64.flow.std(dim=0).max() < 1e-3
    assert (r32.out.double() - r64.out).abs().max() < 4 * B.ULP


def test_loud_weights_are_loud():
    """What the stated factors buy: a flow whose variation across points is a tenth of its size, not a thousandth."""
    x = B.uniform_points(4096, 1)
    loud = B.nsfp(B.nsfp_flat("loud").double(), x.double())
    quiet = B.nsfp(B.nsfp_flat("default").double(), x.double())
    print(f"loud: flow max {loud.flow.abs().max():.3f}  std across points {loud.flow.std(dim=0).tolist()}  "
          f"largest activation {max(float(z.max()) for z in loud.zs):.3f}")
    print(f"default: flow max {quiet.flow.abs().max():.3f}  std across points {quiet.flow.std(dim=0).tolist()}")
    assert loud.flow.abs().max() >= 0.25 and loud.flow.std(dim=0).min() >= 0.02
    assert max(float(z.abs().max()) for z in loud.zs) < 10.0                     # and nowhere near a range where float32 would strain
    assert quiet.flow.std(dim=0).max() < 1e-3


def tensor_bars(r64, r32):
    return [B.bar(float((b.double() - a).abs().max()), float(a.abs().max())) for a, b in zip(B.split(r64.grad), B.split(r32.grad))]


@pytest.mark.parametrize("n", sorted({n for n, _ in B.NSFP_BWD_CASES}))
def test_gradients_are_nonzero_and_feel_the_last_point(n):
    """Every checked tensor has a non-zero maximum; from n = 64 on, leaving the LAST point out moves every tensor by more than ten
    bars: a backward that dropped a tail row, or a partial, could not pass."""
    x, gy = B.kink_free_points("loud", n)[0], B.upstream_gradient(n)
    r64, r32 = B.nsfp_pair(B.nsfp_flat("loud"), x, gy)
    assert r64.grad.shape == (B.P_COUNT,)
    assert all(float(t.abs().max()) > 0 for t in B.split(r64.grad))
    if n >= 64:
        less = B.nsfp(B.nsfp_flat("loud").double(), x[:-1].double(), gy[:-1].double())
        for name, full, part, bar in zip(B.names(), B.split(r64.grad), B.split(less.grad), tensor_bars(r64, r32)):
            assert float((full - part).abs().max()) > 10 * bar, (name, float((full - part).abs().max()), bar)


def test_stride_case_rows_are_kink_free_and_tell_their_tiles_apart():
    x, rows, candidates, dropped = B.stride_case()
    n = x.shape[0]
    print(f"nsfp stride: {dropped} of {candidates} compared rows dropped ({100.0 * dropped / candidates:.2f} %)")
    assert n == 512 * 64 + 65 and (n + 63) // 64 == 514 and candidates == 64 + 65          # two tiles past a grid of 512, the last of one row
    assert dropped <= MAX_DROPPED_SHARE * candidates
    assert (rows < 64).sum() >= 48 and (rows >= 512 * 64).sum() >= 48 and rows[-1] == n - 1
    r64, r32 = B.nsfp_pair(B.nsfp_flat("loud"), x[rows])
    assert all(torch.equal(a > 0, b > 0) for a, b in zip(r64.zs, r32.zs))
    bar = B.bar(float((r32.flow.double() - r64.flow).abs().max()), float(r64.flow.abs().max()))
    assert (r64.flow[1:] - r64.flow[:-1]).abs().max(dim=1)[0].min() > 10 * bar              # a row is not its neighbour ...
    flow = B.nsfp(B.nsfp_flat("loud").double(), x.double()).flow
    late = torch.arange(512 * 64, n)
    assert (flow[late] - flow[late - 512 * 64]).abs().max(dim=1)[0].min() > 10 * bar        # ... nor the row its workgroup saw a trip earlier
