"""A slot's bits must not depend on what it held before.

register_batch keeps `slots` pairs resident and refills a finished slot while the others are mid-flight, and the engine cache hands
the same engine to the next call: almost every pair runs in a slot another pair has just left.  k_eng_load rewrites only part of a
slot (point plane 0, landmark / target rows below K / T, parameters, Adam moments, geometry, one state parity); the rest -- the other
point plane, activations, head records, dO, gradient partials, nearest-neighbour results and workspaces, gmax, the other state
parity -- keeps what the previous pair (possibly a larger or a diverged one) left there.  The tick kernels work on whole 64-point
tiles and fold all G partials, so each of them relies on "whoever ran before me left this clean, or I clean it myself".

The property pinned here needs no tolerance: for a fixed engine geometry and configuration, the bits a pair produces TICK BY TICK --
parameters, Adam moments, its state record, its points, its nearest-neighbour results -- depend on that pair alone: not on what the slot
held before (garbage, a larger pair in mid-flight or finished, a landmark-only pair), not on the tick parity it was loaded at, not on
its neighbours.  Every history below must reproduce the trace of the same pair in a FRESH engine with parked neighbours; the
fresh-engine-against-oracle tests of test_hip_parity.py / test_generic_width.py / test_split_accuracy.py then carry over to the slots
the production path really uses.  (The only tolerances in this file are the oracle tie-in's, which are those of
test_engine_fixed_work_matches_oracle.)

A trace record also holds BOTH point planes of the pair (not only the current one): after the pair's first tick the other plane's
rows below K + S are this tick's warped points.  Of a finished slot the tick kernels write one thing only: k_eng_loss copies its state
record into the other parity with decision = IDLE, the same bytes every tick; everything else of the slot is left
alone.  So its records repeat, and comparing a fixed number of ticks compares nothing less than "until both read as finished" -- it
also holds the idle ticks to the same bits -- and needs no host round trip per tick."""
import functools
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from deformationpyramid_amd._native import DEC_ADVANCE, DEC_IDLE, DEC_STEP_ADVANCE          # (importing _native loads no library)
from tests._helpers import (ENGINE_POISONED, VARIANTS, engine_modes, generic_pyramid, registration_modes, scale_heads, seeded_pyramid)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K0 = -8

B, CAP, M, SLOT = 3, 512, 3, 1
# Early stop: 5 iterations per level at most, a level ends early once the loss has moved by less than 1 % twice (so after 3 evaluations
# at the soonest).  One level of every pair under test carries head weights x 20 (SCALED_LEVEL), so the loss keeps moving there and
# settles at once on the others: levels end both ways, and the break counter / loss_prev reset at a hand-over matter.  That is asserted
# on the fresh trace of each of the two tile-tail pairs (BOTH_WAYS) in every configuration, and over the five pairs together: the
# one-point pair and the full slot do not end levels both ways under every arithmetic whichever level is scaled.
ITERS, RATIO, BREAKS = 5, 0.01, 2
SCALED_LEVEL = {"w64d2_se3aa": 2}             # (pyramid kind -> the level with x 20 heads; every other kind: level 1)
N_TICKS = M * ITERS + 2                       # a pair needs at most M * ITERS ticks

# (K landmarks, S samples, T targets): the smallest shapes at which tile tails and idle workgroups occur
PAIRS = [(0, 65, 63),        # two tiles, the second holding one point
         (7, 120, 130),      # 127 points: one short of two full tiles, landmarks and samples in one tile
         (0, 1, 1),
         (20, 0, 0),         # landmark-only: the NN stage must not touch it
         (0, 512, 512)]      # a full slot
BOTH_WAYS = PAIRS[:2]
PREV = (40, 472, 512)        # the full-size previous tenant (every head weight x 20: large activations and gradients)
LDMK_ONLY = (20, 0, 0)
NEIGHBOURS = [(0, 300, 280), (30, 100, 90), (0, 200, 410)]               # slot 0, slot 2, slot 0's refill while slot 1 runs

# arithmetic of the level kernels: (pyramid kind, BatchedEngine arguments, w_reg)
ARITH = {
    "fp32": ("w128", dict(gemm_mode=0), 0.0),
    "split_fused": ("w128", dict(gemm_mode=7), 0.0),
    "split_two_launch": ("w128", dict(gemm_mode=7 | 16), 0.0),
    "w64d2_se3aa": ("w64d2_se3aa", {}, 0.0),
    "w100d3_se3quat_nr": ("w100d3_se3quat_nr", {}, 0.5),                 # the gate row; level 0's shorter layout against stale gate moments
    "w128_gated": ("w128nr", dict(gemm_mode=7), 0.5),                    # shipped width with the nonrigidity head and the BCE term
}
# NN stage.  "default": with B = 3 the engine picks the latency shape (nn_mode 1, no cell search) -- asserted below, so the full matrix
# under "default" IS the full matrix under nn_mode = 1; "cells" is what the engine picks at the batch sizes bench.py runs.
NN = {
    "default": {},
    "cells": dict(nn_cells=True),
    "nn0": dict(nn_mode=0, nn_cells=False),
    "nn2": dict(nn_mode=2, nn_cells=False),
}
GS = [None, 2, 1]             # None: one workgroup per tile of the capacity (8); 1 with split_fused: Adam behind the backward + k_eng_update_rest


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from deformationpyramid_amd import _native
    _native.lib()            # must load: no fallback
    return torch.device("cuda:0")


def O():
    from oracle import ndp_oracle
    return ndp_oracle


def cdesc(d):
    return O().make_desc(d.width, d.n_hidden, d.motion, d.rotfmt, d.nonrigidity, d.mlp_scale)


# ------------------------------------------------------------------------------------------------ inputs (built once, never modified)
def cloud(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, 3, generator=g) - 0.5) * scale).contiguous()


@functools.lru_cache(maxsize=None)
def _pyramid(kind, seed, m, scale_level, factor):
    """scale_level: a level whose head weights are multiplied by `factor`, -1: every level, None: none."""
    if kind == "w128":
        pyr = seeded_pyramid(seed, m=m, **VARIANTS["se3aa"])
    elif kind == "w128nr":
        pyr = seeded_pyramid(seed, m=m, nonrigidity_est=True, **VARIANTS["se3aa"])
    else:
        pyr = generic_pyramid(seed, kind, m=m)
    for lvl in range(m):
        if scale_level == -1 or scale_level == lvl:
            scale_heads(pyr, lvl, factor)
    return pyr


@functools.lru_cache(maxsize=None)
def _clouds(K, S, T, seed):
    """-> (pts [K + S, 3] landmarks first, ldmk_t [K, 3] | None, tgt [T, 3] | None): the clouds of test_hip_parity's engine tests."""
    if (K, S, T) == (0, 1, 1):                    # one sample 0.12 away from its target: inside the truncation radius
        return torch.tensor([[0.1, -0.2, 0.05]]), None, torch.tensor([[0.15, -0.1, 0.0]])
    src = cloud(K + S, 100 + seed)
    c, s_ = np.cos(0.2), np.sin(0.2)
    Rz = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    tgt = (cloud(T, 200 + seed) @ Rz.T + torch.tensor([0.03, -0.02, 0.01])).contiguous() if T else None
    lt = ((src[:K] + 0.04 * torch.sin(4 * src[:K])) @ Rz.T).contiguous() if K else None
    return src, lt, tgt


@functools.lru_cache(maxsize=None)
def _item(dev, kind, shape, seed, m=M, scale_level="kind", factor=20.0):
    """One pair ready for BatchedEngine.load: device tensors, parameters padded to the engine's stride."""
    K, S, T = shape
    if scale_level == "kind":
        scale_level = SCALED_LEVEL.get(kind, 1)
    pyr = _pyramid(kind, seed, m, scale_level, factor)
    P = pyr.descs[m - 1].param_count
    stride = (P + 63) // 64 * 64
    params = torch.zeros(m, stride)
    params[:, :P] = pyr.store[:, :P]
    pts, lt, tgt = _clouds(K, S, T, seed)
    up = lambda t: None if t is None else t.to(dev)
    return SimpleNamespace(K=K, S=S, T=T, pyr=pyr, params=params.to(dev), pts=up(pts), lt=up(lt), tgt=up(tgt), host=(pts, lt, tgt))


def _load(eng, slot, it):
    eng.load(slot, it.pts, it.K, it.S, it.lt, it.tgt, it.params)


def _engine(dev, arith, G, nn, m=M, iters=ITERS, early_stop=True):
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    kind, modes, w_reg = ARITH[arith] if isinstance(arith, str) else arith
    desc = _pyramid(kind, 0, m, None, 1.0).descs[m - 1]          # (gated shapes: the engine's "levels > 0 gated" descriptor)
    cfg = OptConfig(m=m, iters=iters, early_stop=early_stop, w_cd=0.5, trunc=0.05, break_threshold_ratio=RATIO, max_break_count=BREAKS,
                    w_reg=w_reg)
    kw = dict(modes)
    kw.update(NN[nn] if isinstance(nn, str) else nn)
    eng = BatchedEngine(desc, cfg, B, n_cap=CAP, t_cap=CAP, device=dev, G=G, **kw)
    eng.park_all()                                               # (a new engine's zero states read as live pairs without points)
    eng.kind = kind
    return eng


# ------------------------------------------------------------------------------------------------ trace
def _fields(eng, slot):
    """(name, tensor view) of what a pair's trace records after a tick."""
    K, S, T = (int(v) for v in eng._geom_h[slot][:3])
    out = [("params", eng.params[slot]), ("adam_m", eng.adam_m[slot]), ("adam_v", eng.adam_v[slot]),
           ("state", eng.state[eng.tick & 1, slot]), ("pts", eng.pts[slot, :, :K + S])]
    if S > 0 and T > 0:
        out += [("d2x", eng.d2x[slot, :S]), ("idx_x", eng.idx_x[slot, :S]), ("d2y", eng.d2y[slot, :T]), ("idx_y", eng.idx_y[slot, :T])]
    return out


def trace(eng, slot, n_ticks):
    """One tick at a time; after each, the raw bytes of everything the pair in `slot` owns -> uint8 [n_ticks, L] (on the device:
    nothing here waits for the GPU).  Bytes, not floats: a NaN equals itself."""
    recs = []
    for _ in range(n_ticks):
        eng.run_ticks(1)
        recs.append(torch.cat([t.contiguous().view(torch.uint8).reshape(-1) for _, t in _fields(eng, slot)]))
    return torch.stack(recs)


def _layout(eng, slot):
    return [(name, t.numel() * t.element_size()) for name, t in _fields(eng, slot)]


def states_of(eng, slot, tr):
    """The slot's PairState after every traced tick."""
    from deformationpyramid_amd import _native as N
    off = 0
    for name, nb in _layout(eng, slot):
        if name == "state":
            raw = tr[:, off:off + nb].cpu().numpy()
            return [N.PairState.from_buffer_copy(raw[i].tobytes()) for i in range(raw.shape[0])]
        off += nb
    raise AssertionError("no state in the trace")


def ended_both_ways(sts):
    """Did levels of this trace end by early stop (ADVANCE: no step taken) AND by their iteration count (STEP_ADVANCE)?"""
    dec = {s.decision for s in sts}
    return DEC_ADVANCE in dec and DEC_STEP_ADVANCE in dec


def assert_same_trace(want, got, eng, slot, what):
    assert want.shape == got.shape, (what, want.shape, got.shape)
    if torch.equal(want, got):
        return
    diff = (want != got)
    tick = int(torch.nonzero(diff.any(dim=1))[0])
    col = int(torch.nonzero(diff[tick])[0])
    off = 0
    for name, nb in _layout(eng, slot):
        if col < off + nb:
            n_bad = int(diff[tick, off:off + nb].view(-1, 4).any(dim=1).sum()) if nb % 4 == 0 else -1
            raise AssertionError(f"{what}: the trace leaves the fresh engine's at tick {tick} in `{name}` (first byte {col - off} of {nb}, "
                                 f"{n_bad} words differ in that field at that tick)")
        off += nb


# ------------------------------------------------------------------------------------------------ histories
def poison(eng, kind):
    """Overwrites every buffer of ENGINE_POISONED.  kind "nan": floats NaN, "big": floats 0x7f7f7f7f (3.4e38, finite); integer buffers a
    mix of negative, in-range and >= capacity values; the state records garbage bytes in both parities."""
    d = eng.device
    cap_ = max(eng.n_cap, eng.t_cap)
    for name in ENGINE_POISONED:
        t = getattr(eng, name, None)
        if t is None:
            assert name.startswith("nnc_") and not eng.nn_cells, name        # the only buffers an engine may lack
            continue
        assert getattr(eng.c_engine, name) == t.data_ptr(), name               # the memory the kernels are handed, not a namesake
        if t.dtype == torch.float32:
            if kind == "nan":
                t.fill_(float("nan"))
            else:
                t.view(torch.int32).fill_(0x7f7f7f7f)
        elif t.dtype == torch.int32:
            i = torch.arange(t.numel(), device=d, dtype=torch.int64)
            v = torch.where(i % 4 == 0, -1 - (i % 977), torch.where(i % 4 == 1, i % cap_, torch.where(i % 4 == 2, cap_ + (i % 100003),
                                                                                                  torch.full_like(i, 0x7fffffff))))
            t.view(-1).copy_(v.to(torch.int32))
        else:
            assert t.dtype == torch.uint8, (name, t.dtype)
            if kind == "nan":
                g = torch.Generator().manual_seed(1234)
                t.copy_(torch.randint(0, 256, tuple(t.shape), generator=g, dtype=torch.uint8).to(d))
            else:
                t.fill_(0x7f)


def _run_until(eng, slot, cond, limit):
    for _ in range(limit):
        st = eng.read_states()[slot]
        if cond(st):
            return st
        eng.run_ticks(1)
    raise AssertionError(f"slot {slot} never reached the wanted state within {limit} ticks")


def _neighbours(eng, dev, k):
    """Slots 0 and 2 get other pairs of other sizes (they finish at ticks of their own)."""
    _load(eng, 0, _item(dev, eng.kind, NEIGHBOURS[0], 40 + k))
    _load(eng, 2, _item(dev, eng.kind, NEIGHBOURS[1], 50 + k))


def _trace_with_refilled_neighbour(eng, dev, k):
    first = trace(eng, SLOT, 4)
    _load(eng, 0, _item(dev, eng.kind, NEIGHBOURS[2], 60 + k))              # slot 0 is refilled while slot 1 runs
    return torch.cat([first, trace(eng, SLOT, N_TICKS - 4)])


def run_history(hist, eng, dev, it, k):
    """Brings slot 1 of `eng` into the state the history names, loads `it` there and returns its trace."""
    kind = eng.kind
    if hist in ("poison_nan", "poison_big"):
        poison(eng, hist[7:])
        eng.park_all()
        _load(eng, SLOT, it)
        return trace(eng, SLOT, N_TICKS)
    prev = _item(dev, kind, LDMK_ONLY, 70, scale_level=-1) if hist == "mid_after_landmarks" else _item(dev, kind, PREV, 9, scale_level=-1)
    _neighbours(eng, dev, k)
    _load(eng, SLOT, prev)
    if hist.startswith("mid"):                                              # the previous tenant is inside level 1 (cur == 1)
        want = {"mid_odd": 1, "mid_even": 0}.get(hist)
        st = _run_until(eng, SLOT, lambda s: s.level == 1 and s.iter >= 1 and (want is None or (eng.tick & 1) == want), 3 * ITERS)
        assert st.cur == 1 and st.level == 1
    else:                                                                   # ... has finished and idled for three ticks
        _run_until(eng, SLOT, lambda s: s.level >= M, M * ITERS + 2)
        eng.run_ticks(3)
        if hist == "done_parked":
            eng.park(SLOT)
    _load(eng, SLOT, it)
    return _trace_with_refilled_neighbour(eng, dev, k)


FULL_HISTORIES = ("poison_nan", "poison_big", "mid_odd", "mid_even", "mid_after_landmarks", "done_idle", "done_parked")


def fresh_trace(dev, arith, G, nn, it):
    eng = _engine(dev, arith, G, nn)
    _load(eng, SLOT, it)
    return eng, trace(eng, SLOT, N_TICKS)


# ------------------------------------------------------------------------------------------------ the matrix
@pytest.mark.parametrize("nn", ["default", "cells"])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("arith", list(ARITH))
def test_a_pairs_trace_does_not_depend_on_the_slots_history(dev, arith, G, nn):
    """Every pair x every history against the pair's trace in a fresh engine, bit for bit and tick by tick."""
    kind = ARITH[arith][0]
    lived = {h: _engine(dev, arith, G, nn) for h in FULL_HISTORIES}         # one engine per history: it gets more lived-in pair by pair
    decisions = set()
    for k, shape in enumerate(PAIRS):
        it = _item(dev, kind, shape, 11 + k)
        eng, want = fresh_trace(dev, arith, G, nn, it)
        if nn == "default":
            assert eng.nn_mode == 1 and not eng.nn_cells                    # what "default" means at B = 3 (see NN above)
        else:
            assert eng.c_engine.nn_cells == 1
        assert eng.G == (G or CAP // 64)
        sts = states_of(eng, SLOT, want)
        assert sts[-1].level == M and sts[-1].decision == DEC_IDLE, (shape, sts[-1].level)     # finished inside the traced ticks
        decisions |= {s.decision for s in sts}
        if shape in BOTH_WAYS:
            assert ended_both_ways(sts), (shape, list(sts[-1].evals_per_level[:M]))
        for hist in FULL_HISTORIES:
            got = run_history(hist, lived[hist], dev, it, k)
            assert_same_trace(want, got, eng, SLOT, f"{arith} G={G} nn={nn} pair {shape} after {hist}")
    # over the five fresh runs, too, levels ended by early stop AND by their iteration count
    assert DEC_ADVANCE in decisions and DEC_STEP_ADVANCE in decisions, decisions


@pytest.mark.parametrize("nn", ["nn0", "nn2"])
@pytest.mark.parametrize("G", GS)
@pytest.mark.parametrize("arith", list(ARITH))
def test_a_pairs_trace_under_the_one_pass_nn_kernels(dev, arith, G, nn):
    """The dense one-pass kernels (row partials in nn_row, folded by the loss stage): the mid-flight refill at both parities and the
    NaN-poisoned engine (nn_row is read in these modes only), first two pairs."""
    kind = ARITH[arith][0]
    hists = ("mid_odd", "mid_even", "poison_nan")
    lived = {h: _engine(dev, arith, G, nn) for h in hists}
    for k, shape in enumerate(PAIRS[:2]):
        it = _item(dev, kind, shape, 11 + k)
        eng, want = fresh_trace(dev, arith, G, nn, it)
        assert eng.nn_mode == NN[nn]["nn_mode"] and not eng.nn_cells
        sts = states_of(eng, SLOT, want)
        assert sts[-1].level == M and sts[-1].decision == DEC_IDLE
        assert shape in BOTH_WAYS and ended_both_ways(sts), (shape, list(sts[-1].evals_per_level[:M]))
        for hist in hists:
            got = run_history(hist, lived[hist], dev, it, k)
            assert_same_trace(want, got, eng, SLOT, f"{arith} G={G} nn={nn} pair {shape} after {hist}")


# ------------------------------------------------------------------------------------------------ oracle tie-in
@pytest.mark.parametrize("shape", PAIRS[:2])
def test_a_refilled_slot_matches_the_oracle(dev, arith, shape):
    """History mid_odd, early stop off (2 levels x 6 iterations): the refilled slot's final loss and points against O().optimize of
    that pair, at the budgets of test_engine_fixed_work_matches_oracle (loss 1e-4 relative, points 1e-4)."""
    m, iters = 2, 6
    K, S, T = shape
    modes = engine_modes(arith, CAP)
    eng = _engine(dev, ("w128", modes, 0.0), None, {}, m=m, iters=iters, early_stop=False)
    _load(eng, 0, _item(dev, "w128", NEIGHBOURS[0], 40, m=m))
    _load(eng, 2, _item(dev, "w128", NEIGHBOURS[1], 50, m=m))
    _load(eng, SLOT, _item(dev, "w128", PREV, 9, m=m, scale_level=-1))
    st = _run_until(eng, SLOT, lambda s: s.level == 1 and s.iter >= 1 and (eng.tick & 1) == 1, 3 * iters)
    assert st.cur == 1
    it = _item(dev, "w128", shape, 11 + PAIRS.index(shape), m=m, scale_level=None)      # (initial heads as the parity tests have them)
    _load(eng, SLOT, it)
    states = eng.run_until_done(chunk=4)
    st = states[SLOT]
    assert st.level == m and list(st.evals_per_level[:m]) == [iters] * m and st.total_steps == m * iters
    pyr = it.pyr
    pts, lt, tgt = it.host
    pa = np.concatenate([pyr.store[i, :dd.param_count].numpy() for i, dd in enumerate(pyr.descs)])
    ref = O().optimize([cdesc(dd) for dd in pyr.descs], pa, pts.numpy(), K, S, lt.numpy() if K else None, tgt.numpy(), k0=K0,
                       iters=iters, w_cd=0.5, trunc=0.05, early_stop=False, nthreads=4)
    loss_ref = ref["loss_trace"][-1]
    got = eng.final_points(SLOT, st).cpu().numpy()
    print(f"refilled slot vs oracle {arith} {shape}: loss {st.loss} vs {loss_ref}, points {np.abs(got - ref['pts']).max()}")
    assert abs(st.loss - loss_ref) < 1e-4 * abs(loss_ref)
    assert np.abs(got - ref["pts"]).max() < 1e-4


# ------------------------------------------------------------------------------------------------ registration level
def _engine_facts(model):
    e = model._engines[0]
    return dict(n_cap=e.n_cap, t_cap=e.t_cap, G=e.G, gemm_mode=e.gemm_mode, nn_mode=e.nn_mode, nn_cells=e.nn_cells)


def _log_loads(monkeypatch):
    """Records (slot, K, S, T) of every pair a BatchedEngine is given, in load order."""
    from deformationpyramid_amd.engine import BatchedEngine
    log, real = [], BatchedEngine.load_jobs

    def load_jobs(self, jobs):
        log.extend((j["slot"], int(j["K"]), int(j["S"]), int(j["T"])) for j in jobs if j.get("params") is not None)
        return real(self, jobs)

    monkeypatch.setattr(BatchedEngine, "load_jobs", load_jobs)
    return log


def _assert_same_results(a, b):
    assert len(a) == len(b)
    for i, ((wa, ca), (wb, cb)) in enumerate(zip(a, b)):
        assert wa.shape == wb.shape and torch.equal(wa.view(torch.int32), wb.view(torch.int32)), f"pair {i}: warped points differ"
        assert ca == cb, (i, ca, cb)


@pytest.fixture(scope="module")
def ndp_cfg(dev):
    from deformationpyramid_amd.config import load_config
    return load_config(os.path.join(ROOT, "config", "NDP.yaml"), device=0)


def _ndp_pairs():
    from deformationpyramid_amd.synthetic import synthetic_pair
    pairs = []
    for p, n_total in enumerate((1500, 1564, 400, 1628, 1692, 410, 1756)):      # pairs 2 and 5: clouds smaller than `samples`
        src, tgt, _, _ = synthetic_pair(20 + p, n_total=n_total)
        pairs.append((src, tgt))
    return pairs


def test_register_batch_two_slots_equal_one_slot_per_pair(ndp_cfg, arith, monkeypatch):
    """Seven pairs through two slots (five refills into lived-in slots) against the same pairs with a slot each, same seed: warped
    points and iteration counts bit-identical per pair.  Pairs 2 and 5 have fewer points than `samples` (S, T < 300) and each follows a
    full-size pair in its slot.  (prefetch=False: pairs are prepared on the calling thread, so which slot a pair lands in does not
    depend on thread timing; test_register_batch_equals_sequential_register holds prefetch on and off to the same bits.)"""
    from deformationpyramid_amd.config import Config
    from deformationpyramid_amd.registration import Registration
    c = Config(ndp_cfg, samples=300, m=3, iters=40)
    pairs = _ndp_pairs()
    kw = registration_modes(arith)
    log = _log_loads(monkeypatch)
    torch.manual_seed(3)
    two = Registration(c, **kw)
    a = two.register_batch(pairs, slots=2, prefetch=False)
    loads_two = list(log)
    del log[:]
    torch.manual_seed(3)
    each = Registration(c, **kw)
    b = each.register_batch(pairs, slots=len(pairs), prefetch=False)
    assert _engine_facts(two) == _engine_facts(each), (_engine_facts(two), _engine_facts(each))     # else bit equality is not expected
    assert two._engines[0].B == 2 and each._engines[0].B == len(pairs)
    small = [i for i, (_, _, S, T) in enumerate(loads_two) if S < 300 and T < 300]
    assert len(loads_two) == len(pairs) and len(small) == 2, loads_two
    for i in small:                                                # the tenant before each small pair was a full-size one
        before = [l for l in loads_two[:i] if l[0] == loads_two[i][0]]
        assert before and before[-1][2] == 300 and before[-1][3] == 300, (i, loads_two)
    _assert_same_results(a, b)


def test_register_batch_landmark_sets_of_different_sizes_two_slots_equal_four(dev, arith, monkeypatch):
    """The LNDP configuration with K = 20, 150, 400, 90 landmarks (the pairs of
    test_register_batch_sizes_engines_for_the_largest_landmark_set): two slots against four, bit-identical per pair.  With two
    slots the last two pairs are refills: each runs where a pair with another number of landmarks has just been."""
    from deformationpyramid_amd.config import Config, load_config
    from deformationpyramid_amd.registration import Registration
    from deformationpyramid_amd.synthetic import synthetic_landmarks, synthetic_pair
    c = Config(load_config(os.path.join(ROOT, "config", "LNDP.yaml"), device=0), samples=200, m=3, iters=30, w_cd=0.5, trunc_cd=0.05)
    pairs = []
    for p, k in enumerate((20, 150, 400, 90)):
        src, tgt, flow_gt, _ = synthetic_pair(40 + p, n_total=1200)
        pairs.append((src, tgt, synthetic_landmarks(p, src, flow_gt, k=k)))
    kw = registration_modes(arith)
    log = _log_loads(monkeypatch)
    torch.manual_seed(5)
    two = Registration(c, **kw)
    a = two.register_batch(pairs, slots=2, prefetch=False)
    loads_two = list(log)
    torch.manual_seed(5)
    four = Registration(c, **kw)
    b = four.register_batch(pairs, slots=4, prefetch=False)
    assert _engine_facts(two) == _engine_facts(four), (_engine_facts(two), _engine_facts(four))
    assert two._engines[0].n_cap >= 200 + 400
    assert sorted(l[1] for l in loads_two) == [20, 90, 150, 400], loads_two
    for i in (2, 3):                                               # a refill: another landmark set lived in that slot before
        before = [l for l in loads_two[:i] if l[0] == loads_two[i][0]]
        assert before and before[-1][1] != loads_two[i][1], (i, loads_two)
    _assert_same_results(a, b)


def test_a_second_register_batch_call_runs_in_the_cached_engines_and_gives_the_same_bits(ndp_cfg, arith):
    """(prefetch=False as above: which slot a pair lands in does not depend on thread timing, so a failure reproduces.  The call in
    between only changes what the slots hold: a pair's samples and initial weights come from the generator's position, which depends on
    the pair's place in the list, so the reversed list's results are not comparable with the first call's.)"""
    from deformationpyramid_amd.config import Config
    from deformationpyramid_amd.registration import Registration
    c = Config(ndp_cfg, samples=300, m=3, iters=40)
    pairs = _ndp_pairs()
    model = Registration(c, **registration_modes(arith))
    torch.manual_seed(3)
    a = model.register_batch(pairs, slots=2, prefetch=False)
    eng = model._engines[0]
    torch.manual_seed(3)
    model.register_batch(list(reversed(pairs)), slots=2, prefetch=False)    # other tenants in between
    torch.manual_seed(3)
    c2 = model.register_batch(pairs, slots=2, prefetch=False)
    assert model._engines[0] is eng                                         # the lived-in engine, not a new one
    _assert_same_results(a, c2)
