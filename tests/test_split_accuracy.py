"""What justifies `dtype: f32` for the split level kernels (engine gemm_mode 7).

Every kernel of one tick is run on its own (ndp_engine_run_stages) in both arithmetic configurations -- the fp32-MFMA
kernels, bitwise the oracle's fma chain, and the kernels that form the 128x128 contractions from two-way fp16 splits
(x = hi + 2^-11 lo, three products; rounds 2-3: three-way bf16 splits, six products) on the 16-bit MFMA -- and each output (activations, head outputs, weight / bias gradients, the data gradient dz1) is
compared with a FLOAT64 evaluation of the same kernel on the SAME inputs (the kernel's own input buffers, cast up).
The split path's maximum error must not exceed 1.5x the fp32 chain's: it is fp32 arithmetic in everything but the
summation order.  (/root/reference/model/nets.py:111-140 forward; its autograd for the gradients.)
"""
import numpy as np
import pytest
import torch

from tests._helpers import VARIANTS, seeded_pyramid, scale_heads
from tests._tick_ref import _errors, _f64_reference, _kernel_outputs, _run_tick_by_stages       # (moved there: tests/test_tick_layouts.py shares them)

pytestmark = pytest.mark.gpu
K0 = -8
RATIO = 1.5


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()
    return torch.device("cuda:0")


@pytest.mark.parametrize("G", [None, 2, 1])
@pytest.mark.parametrize("tag,level", [("se3aa", 0), ("se3aa", 3), ("sim3eu", 1), ("sflow", 2)])
def test_split_kernels_are_as_close_to_float64_as_the_fp32_chain(dev, tag, level, G):
    """Bar, per output tensor of every kernel, split path vs fp32 chain, both against float64:
      * tensors of >= 10 000 elements (the activations h1, h2, the head outputs, the data gradient dz1, the 128x128 weight
        gradients): RMS error at most 1.5x the chain's (measured over the cases below: 0.7-1.2x), maximum error at most 2x (the
        maximum of 256 000 elements is a tail statistic: measured 0.4-1.6x);
      * small tensors (768-896 elements of dWh / dW0, 128 of a bias gradient, 6-7 of dbh): too few elements for a ratio to be
        more than noise (dbh is a plain fp32 sum in both kernels and still lands anywhere in 0.3-2.4x): at most 3x, RMS and max.
        One of them is systematically on the high side and is reported rather than hidden: dW0 / db0 with ONE tile per
        accumulator come out at 1.5-2.2x the chain's RMS (3-4e-7 of the tensor's scale instead of 1.5-2.5e-7) -- they sum
        dz0 = (dz1 . W1) * [h0 > 0], a split contraction the kernel never writes out, over the points with heavy cancellation;
        with the bench's 16 tiles per accumulator (G = 2) the same tensors are at 0.5-0.75x.
    Everything stays below 5e-6 of its tensor's scale in absolute terms (the north-star budget is 1e-4 on warped coordinates).
    The per-tensor numbers of every case are written to gpurun_out/split_accuracy_*.json (kept under profiles/).
    G: workgroups per pair -- None: one per tile (the latency shape), 2: a 128-slot engine's shape (16 tiles per accumulator), 1: the shape
    bench.py runs since round 4 (256 slots per engine: ONE workgroup and one accumulator per pair, 32 tiles;
    the same G for both arithmetics, so that the comparison is between arithmetics, not between partial counts)."""
    import json
    import os
    S, T = 2000, 2000
    e_chain = _errors(_run_tick_by_stages(dev, tag, 0, S, T, level, 20.0, G=G))      # the same tiles per accumulator in both
    e_split = _errors(_run_tick_by_stages(dev, tag, 7, S, T, level, 20.0, G=G))
    report = {k: {"chain_max": e_chain[k][0], "split_max": e_split[k][0], "chain_rms": e_chain[k][1], "split_rms": e_split[k][1],
                  "elements": e_chain[k][2]} for k in e_chain}
    out_dir = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"split_accuracy_{tag}_L{level}_G{G or 'tiles'}.json"), "w") as f:      # kept under profiles/ by hand
        json.dump(report, f, indent=1)
    for k, r in report.items():
        # relative to the tensor's own scale both sit at a few fp32 ulps of a 128- (or 2000-) term sum
        assert r["chain_max"] < 5e-6 and r["split_max"] < 5e-6, (k, r)
        large = r["elements"] >= 10000
        if r["elements"] < 16:
            continue                                  # dbh: three to seven plain fp32 sums in both kernels -- a ratio of two such errors is noise
        assert r["split_rms"] <= (RATIO if large else 3.0) * r["chain_rms"] + 1e-9, (k, "rms ratio", r["split_rms"] / max(r["chain_rms"], 1e-30), report)
        assert r["split_max"] <= (2.0 if large else 3.0) * r["chain_max"] + 2e-8, (k, "max ratio", r["split_max"] / max(r["chain_max"], 1e-30), report)


GRAD_TENSORS = ("dW2", "db2", "dz1", "dW1", "db1", "dW0", "db0")


@pytest.mark.parametrize("w_cd", [1e-7, 3e4])
def test_gradient_scale_keeps_the_split_backward_exact_over_the_range_of_gradients(dev, w_cd):
    """The split backward multiplies its gradient operands by S = 2^k (k from the pair's max |dO| of the tick, left in e.gmax by
    k_eng_loss) so that they sit in fp16's range, and the results by 1 / S.  With the loss weighted 1e-7 (|dO| ~ 1e-11: every
    unscaled fp16 part would be zero) and 3e4 (|dO| ~ 10: an unscaled hi x 2^11 lo would be at fp16's ceiling) the gradient tensors
    are as close to float64 as the fp32 chain's, by the bars of the test above."""
    e_chain = _errors(_run_tick_by_stages(dev, "se3aa", 0, 2000, 2000, 1, 20.0, G=2, w_cd=w_cd))
    e_split = _errors(_run_tick_by_stages(dev, "se3aa", 7, 2000, 2000, 1, 20.0, G=2, w_cd=w_cd))
    for k in GRAD_TENSORS:
        (cm, cr, n), (sm, sr, _) = e_chain[k], e_split[k]
        large = n >= 10000
        assert sm < 5e-6 and cm < 5e-6, (k, sm, cm)
        assert sr <= (RATIO if large else 3.0) * cr + 1e-9, (k, "rms ratio", sr / max(cr, 1e-30))
        assert sm <= (2.0 if large else 3.0) * cm + 2e-8, (k, "max ratio", sm / max(cm, 1e-30))


def test_relu_masks_of_the_split_backward_see_activations_below_fp16s_range(dev):
    """The ReLU masks of the split backward are read from the hi plane of the activation.  With h0 = 1e-9 everywhere (and elements
    of h1 of the same size) a plain fp16 conversion would make every hi zero and mask the whole gradient away; the split keeps
    hi > 0 exactly where the activation is.  dz1 (masked by h1), dW0 / db0 (dz0 masked by h0) against float64 with the true masks."""
    r = _run_tick_by_stages(dev, "se3aa", 7, 2000, 2000, 0, 20.0, G=2, tiny_h0=True)
    h0, h1 = r["act_fwd"][0, :2000], r["act_fwd"][1, :2000]
    assert float(h0.max()) < 3e-8 and float(h0.min()) > 0.0                       # below fp16's smallest subnormal, all positive
    assert int(((h1 > 0) & (h1 < 3e-8)).sum()) > 1000
    e = _errors(r)
    ref = _f64_reference(r)
    assert float(ref["db0"].abs().max()) > 0 and float(ref["dz1"].abs().max()) > 0
    for k in ("dz1", "dW0", "db0", "db1"):
        assert e[k][0] < 5e-6, (k, e[k])
    # dW1 = dz1^T h0 is built from the VALUES of those activations.  The fused backward splits 2^6 h (one accumulator per product,
    # lo unscaled): its absolute floor per operand element is half an fp16 subnormal step over 2^6 = 2^-31 = 4.7e-10 -- nothing
    # beside O(1) activations, but 2^6 x 1e-9 = 6.4e-8 is ONE subnormal step of hi and a lo that rounds to zero: 7 % off.  (The
    # two-launch backward, lo scaled by 2^11: floor 2^-36, 1.5 % of 1e-9.)
    assert e["dW1"][0] < 0.08, e["dW1"]


def test_activations_beyond_fp16s_range_saturate(dev):
    """fp16 ends at 65504.  An operand beyond it enters a contraction saturated: layer 0's output at 65504; h1 and every activation
    and weight of the fused backward, which are split as 2^6 x, at 65504 / 64 = 1023.5 (the h1 plane image IS that split; the fp32
    rows the forward stores -- h2, and h1 for the two-launch backward -- carry the same bound since round 5).  The results are then no longer the fp32 chain's, but they stay finite -- no
    inf, no NaN anywhere in the tick.  (This network's activations are O(1): its inputs are sines and cosines, its weights O(0.1).)"""
    for mode in (7, 23):
        r = _run_tick_by_stages(dev, "se3aa", mode, 2000, 2000, 0, 20.0, G=2, b1=1.0e5)
        h1 = r["act_fwd"][1, :2000]
        # every h1 is out of range: the image holds the bound -- and so do the fp32 rows of the two-launch configuration since round 5
        # (the forward's epilogue bounds the accumulator ONCE, for the planes and for the rows: one v_med3 per element)
        assert float(h1.min()) == float(h1.max()) == 65504.0 / 64.0
        for k in ("act_fwd", "heads", "dO", "dz1"):
            assert bool(torch.isfinite(r[k][..., :2000, :] if r[k].dim() == 3 else r[k][:2000]).all()), (mode, k)
        assert bool(torch.isfinite(r["g_all"]).all())


def test_h0_is_recomputed_by_the_split_backward_not_read_back(dev):
    """With forward and bwd1 on the splits the forward does not store h0 -- act[0] keeps whatever was there -- and bwd1 recomputes it
    from the saved encoding with the forward's own two MFMAs per point group: every gradient and dz1 are BITWISE what they are when
    the forward is told to store h0 as well (gemm_mode bit 8, which bwd1 ignores), and the h0 that bit stores is what layer 1 saw."""
    a = _run_tick_by_stages(dev, "se3aa", 7, 2000, 2000, 1, 20.0, G=2, keep_h0=True)
    b = _run_tick_by_stages(dev, "se3aa", 7, 2000, 2000, 1, 20.0, G=2, keep_h0=False)
    assert bool(torch.isnan(b["act_fwd"][0]).all())                               # never written (the test pre-fills act with NaN)
    assert bool(torch.isfinite(a["act_fwd"][0, :2000]).all())
    for k in ("heads", "dO", "dz1", "g_bwd2", "g_all"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["act_fwd"][1:], b["act_fwd"][1:])


def test_loss_stage_leaves_the_pairs_largest_dO_for_the_gradient_scale(dev):
    """e.gmax[b] after the loss stage = the bit pattern of max |dO| over the pair's points (wave maxima folded per workgroup, one
    atomicMax of the non-negative float's bits per workgroup); the forward stage of the next tick starts it from zero again."""
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    pyr = seeded_pyramid(11, m=1, **VARIANTS["se3aa"])
    scale_heads(pyr, 0, 20.0)
    eng = BatchedEngine(pyr.descs[0], OptConfig(m=1, iters=4, early_stop=False), 2, n_cap=1024, t_cap=1024, device=dev, gemm_mode=7, nn_mode=1)
    g = torch.Generator().manual_seed(5)
    for b, S in enumerate((1000, 700)):
        src = (torch.rand(S, 3, generator=g) - 0.5).contiguous()
        tgt = ((torch.rand(900, 3, generator=g) - 0.5) * 1.05).contiguous()
        eng.load(b, src, 0, S, None, tgt, pyr.store)
    for tick in range(2):
        eng.run_stages(0, 0)
        torch.cuda.synchronize()
        assert eng.gmax[:2].cpu().tolist() == [0, 0]
        eng.run_stages(1, 2)
        torch.cuda.synchronize()
        got = eng.gmax[:2].cpu().view(torch.float32)
        want = eng.dO.abs().amax(dim=(1, 2)).cpu()
        assert torch.equal(got, want), (got, want)
        assert float(want.min()) > 0
        eng.run_stages(3, 5)


@pytest.mark.parametrize("tag,level", [("se3aa", 0), ("sim3eu", 0)])       # level 0: the two engines have seen the same ticks
def test_fused_backward_agrees_with_the_two_launch_backward(dev, tag, level):
    """The one-launch backward (k_eng_bwd_f: both layers per tile, dz1 in LDS, one accumulator per product on pre-scaled splits)
    against the two round-3 launches (k_eng_bwd2_8 + k_eng_bwd1_8, gemm_mode bit 16: main + correction accumulators) on the same
    forward state: the two arithmetics differ in how the three partial products are summed, so the bar is the one both hold against
    float64 -- every gradient tensor within 2e-6 of its own scale -- not bit equality.  Stage 4 of the fused tick launches nothing."""
    a = _run_tick_by_stages(dev, tag, 7, 2000, 2000, level, 20.0, G=2)          # fused (+ dz1 dump)
    b = _run_tick_by_stages(dev, tag, 7 | 16, 2000, 2000, level, 20.0, G=2)     # two launches
    assert torch.equal(a["dO"], b["dO"]) and torch.equal(a["act_fwd"][0], b["act_fwd"][0])
    # h1, h2: the fused backward's forward leaves the split it fed to layer 2 / to the heads (22 bits of 2^6 h, as a plane image), the
    # other the fp32 value
    for k in (1, 2):
        ha, hb = a["act_fwd"][k, :2000].double(), b["act_fwd"][k, :2000].double()
        assert bool(((ha - hb).abs() <= 2.0 ** -21 * hb.abs() + 2.0 ** -31).all()) and bool(((ha > 0) == (hb > 0)).all()), k
    assert torch.equal(a["g_bwd2"], a["g_all"])                                  # the fused stage 3 is the whole backward
    ka, kb = _kernel_outputs(a), _kernel_outputs(b)
    for k in ("dWh", "dbh", "dW2", "db2", "dz1", "dW1", "db1", "dW0", "db0"):
        err = float((ka[k] - kb[k]).abs().max() / kb[k].abs().max().clamp_min(1e-300))
        assert err < 2e-6, (k, err)
