"""One tick of a one-pair 128 / 3 engine, stage by stage, and the float64 evaluation of each of its level kernels from that kernel's own
inputs -- shared by tests/test_split_accuracy.py (the split arithmetic against the fp32 chain at S = T = 2000), tests/test_tick_layouts.py
(every head layout and tile edge at small sizes) and tests/test_tick_layouts_cpu.py (the table below and its preconditions, no GPU).

Nothing here is a transcription of a kernel: the forward is nets.py:111-140 (MLP, mlp_scale) and the backward its autograd, written out
as the five matrix products they are.  `_f64_reference(r, dtype)` runs the same lines in float64 (the reference) or float32 (the yardstick).
"""
import numpy as np
import torch

from tests import _loss_ref as R
from tests._helpers import scale_heads, seeded_pyramid

K0 = -8
ULP = 2.0 ** -23                                   # float32 spacing at 1

# tag -> Deformation_Pyramid arguments.  Head rows: rotation (3 | 4 quaternion | 6 for 6D; none for sflow), Sim3 scale, 3 translation,
# gate (levels >= 1 of a gated pyramid only: nets.py:26).
LAYOUTS = {
    "sflow": dict(rotation_format="axis_angle", motion="sflow"),
    "sflow_nr": dict(rotation_format="axis_angle", motion="sflow", nonrigidity_est=True),
    "se3aa": dict(rotation_format="axis_angle", motion="SE3"),
    "se3eu": dict(rotation_format="euler", motion="SE3"),
    "sim3aa": dict(rotation_format="axis_angle", motion="Sim3"),
    "sim3eu": dict(rotation_format="euler", motion="Sim3"),
    "se3quat": dict(rotation_format="quaternion", motion="SE3"),
    "sim3quat": dict(rotation_format="quaternion", motion="Sim3"),
    "se3quat_nr": dict(rotation_format="quaternion", motion="SE3", nonrigidity_est=True),
    "se36d": dict(rotation_format="6D", motion="SE3"),
    "sim36d": dict(rotation_format="6D", motion="Sim3"),
    "sim36d_nr": dict(rotation_format="6D", motion="Sim3", nonrigidity_est=True),
}
# tag -> (head rows at level 0, head rows at every later level)
HEAD_ROWS = {"sflow": (3, 3), "sflow_nr": (3, 4), "se3aa": (6, 6), "se3eu": (6, 6), "sim3aa": (7, 7), "sim3eu": (7, 7), "se3quat": (7, 7),
             "sim3quat": (8, 8), "se3quat_nr": (7, 8), "se36d": (9, 9), "sim36d": (10, 10), "sim36d_nr": (10, 11)}
GATED = tuple(t for t, kw in LAYOUTS.items() if kw.get("nonrigidity_est"))
UNGATED = tuple(t for t in LAYOUTS if t not in GATED)
# what tests/test_tick_layouts.py runs: every tag at level 0, the gated ones at level 1 (their gate row), two wide heads at level 2
TICK_CASES = tuple((t, 0) for t in LAYOUTS) + tuple((t, 1) for t in GATED) + (("sim3quat", 2), ("se36d", 2))
EDGE_CASES = (("se3aa", 0), ("sim36d_nr", 1))     # nh = 6 and nh = 11 at the tile and workgroup edges
TENSORS = ("h0", "h1", "h2", "heads", "dWh", "dbh", "dW2", "db2", "dz1", "dW1", "db1", "dW0", "db0")
SEED, HEAD_SCALE = 11, 20.0


def levels_of(tag, level):
    """Depth of the pyramid a case needs: a gated pyramid has at least two levels (level 0 of it carries no gate but lives in a
    parameter block sized for the gated layout)."""
    return max(level + 1, 2) if tag in GATED else level + 1


def tick_pyramid(tag, m, head_scale=HEAD_SCALE, seed=SEED):
    pyr = seeded_pyramid(seed, m=m, **LAYOUTS[tag])
    for lvl in range(m):
        scale_heads(pyr, lvl, head_scale)              # head outputs of O(0.01): rotations / translations that matter
    return pyr


def tick_clouds(S, T):
    g = torch.Generator().manual_seed(3)
    src = (torch.rand(S, 3, generator=g) - 0.5).contiguous()
    tgt = ((torch.rand(T, 3, generator=g) - 0.5) * 1.05 + 0.02).contiguous()
    return src, tgt


def level_heads(d, params, level, x, dtype=torch.float64, k0=K0):
    """Scaled head outputs [n, nh] of one level from its flat parameter block (nets.py:111-117, :164-177): positional encoding at
    2^(level + 1 + k0), three ReLU layers, the head matrix, mlp_scale.  d: the LEVEL's descriptor."""
    W, nh = d.width, d.n_heads
    P = params.to(dtype)
    x = x.to(dtype)
    a = x * 2.0 ** (level + 1 + k0)
    h = torch.stack([torch.sin(a[:, 0]), torch.cos(a[:, 0]), torch.sin(a[:, 1]), torch.cos(a[:, 1]), torch.sin(a[:, 2]), torch.cos(a[:, 2])], -1)
    h = torch.relu(h @ P[d.off_W(0):d.off_W(0) + W * 6].view(W, 6).T + P[d.off_b(0):d.off_b(0) + W])
    for i in range(1, d.n_hidden + 1):
        h = torch.relu(h @ P[d.off_W(i):d.off_W(i) + W * W].view(W, W).T + P[d.off_b(i):d.off_b(i) + W])
    return d.mlp_scale * (h @ P[d.off_Wh:d.off_Wh + nh * W].view(nh, W).T + P[d.off_bh:d.off_bh + nh])


def rotation_margins(d, o):
    """What keeps a head's normalisations away from their clamps and 0/0, from scaled head outputs o [n, nh] of the level descriptor d:
    -> dict of the smallest value over the points of  quat_norm | a1_norm, u_norm (6D: |a1|, |a2 - (b1.a2) b1|) | aa_norm."""
    o = o.double()
    if d.motion == "sflow":
        return {}
    if d.rotfmt == "quaternion":
        return {"quat_norm": float(o[:, :4].norm(dim=-1).min())}
    if d.rotfmt == "6D":
        a1, a2 = o[:, 0:3], o[:, 3:6]
        b1 = a1 / a1.norm(dim=-1, keepdim=True)
        u = a2 - (b1 * a2).sum(-1, keepdim=True) * b1
        return {"a1_norm": float(a1.norm(dim=-1).min()), "u_norm": float(u.norm(dim=-1).min())}
    if d.rotfmt == "axis_angle":
        return {"aa_norm": float(o[:, :3].norm(dim=-1).min())}
    return {}


def _run_tick_by_stages(dev, tag, gemm_mode, S, T, level, head_scale, G=None, w_cd=1.0, tiny_h0=False, b1=None, keep_h0=True,  # noqa: C901
                        n_cap=None, t_cap=None, poison=False, warm_mode=None):
    """One tick of a one-pair engine at `level`, stage by stage; returns every buffer a kernel consumed or produced (CPU, fp32).
    tag: a layout of LAYOUTS; a gated engine is built from the pyramid's last descriptor, and the LEVEL's descriptor (head rows and
    offsets of that level: `desc`) is what the comparisons use.
    w_cd: weight of the loss (every gradient scales with it).  tiny_h0: layer 0 of the level = (W0 = 0, b0 = 1e-9), i.e. every
    h0 is positive and below fp16's smallest subnormal (and h1 = relu(1e-9 W1 1 + b1) has such elements too).
    n_cap, t_cap: engine capacities (default: the pair's sizes).  poison: heads, dO and the gradient partials are pre-filled with NaN as
    act always is -- whatever a kernel reads without having been written this tick, or leaves unwritten, shows.  warm_mode: the
    gemm_mode of the ticks BEFORE the one taken apart (default: the same) -- with 0, the fp32 chain, two arithmetics arrive at a level
    >= 1 with bit-identical parameters and points."""
    from deformationpyramid_amd.engine import BatchedEngine, OptConfig
    m = levels_of(tag, level)
    pyr = tick_pyramid(tag, m, head_scale)
    edesc = pyr.descs[m - 1]                                  # nonrigidity = True: "every level but the first is gated"
    d = R.level_desc(edesc, level)
    if tiny_h0:
        with torch.no_grad():
            pyr.store[level, d.off_W(0):d.off_W(0) + d.width * 6] = 0.0
            pyr.store[level, d.off_b(0):d.off_b(0) + d.width] = 1e-9
            pyr.store[level, d.off_b(1):d.off_b(1) + d.width] = 0.0
    if b1 is not None:
        with torch.no_grad():
            pyr.store[level, d.off_b(1):d.off_b(1) + d.width] = b1
    cfg = OptConfig(m=m, iters=2, early_stop=False, w_cd=w_cd)
    # gemm_mode 7: the split forward does not store h0 (bwd1 recomputes it); bit 8 makes it store h0 for the comparisons below --
    # test_h0_is_recomputed... pins that the bit changes nothing else
    # + 32: the fused backward (one launch for both layers, dz1 in LDS) also writes dz1 to HBM, where the two-launch form leaves it
    # + 1024: the whole Adam step in the update stage -- at G = 1 the default steps the two 128 x 128 matrices behind the fused backward's
    # tile loop and writes no partial of them (bitwise the same state: test_adam_behind_the_backward_is_bitwise_the_update_stage)
    mode = gemm_mode if (gemm_mode & 7) != 7 else (gemm_mode | 1024 | (0 if gemm_mode & 16 else 32) | (8 if keep_h0 else 0))
    eng = BatchedEngine(edesc, cfg, 1, n_cap=n_cap or S, t_cap=t_cap or T, device=dev, gemm_mode=mode, nn_mode=1, G=G)
    src, tgt = tick_clouds(S, T)
    eng.load(0, src, 0, S, None, tgt, pyr.store)
    if warm_mode is not None:
        eng.c_engine.gemm_mode = warm_mode                    # (the engine record goes to every call by value)
    for _ in range(2 * level):                               # iters = 2 per level: arrive at `level` with trained lower levels
        eng.run_ticks(1)
    eng.c_engine.gemm_mode = mode
    st = eng.read_states()[0]
    assert st.level == level
    P = edesc.param_count
    out = {"desc": d, "engine_desc": edesc, "n": S, "level": level, "G": eng.G, "n_cap": eng.n_cap, "mode": mode,
           "params": eng.params[0, level, :P].cpu().clone(), "x_in": eng.pts[0, st.cur, :S].cpu().clone()}
    eng.act.fill_(float("nan"))                           # whatever a kernel does not write must not look like data
    if poison:
        eng.heads.fill_(float("nan"))
        eng.dO.fill_(float("nan"))
        eng.gpart.fill_(float("nan"))
    eng.run_stages(0, 2)                                      # forward, nearest neighbours, loss / dL/dx'
    torch.cuda.synchronize()
    out["act_fwd"] = eng.act[0].cpu().clone()                 # h0, h1, h2
    if (mode & 7) == 7 and not mode & 16:                     # the fused backward reads h1 and (round 6) h2 as the forward's plane images, not as fp32 rows
        out["act_fwd"][1] = _decode_plane_image(out["act_fwd"][1])
        out["act_fwd"][2] = _decode_plane_image(out["act_fwd"][2])
    out["heads"] = eng.heads[0].cpu().clone()
    out["dO"] = eng.dO[0].cpu().clone()
    eng.run_stages(3, 3)                                      # bwd2
    torch.cuda.synchronize()
    out["dz1"] = eng.act[0, 2].cpu().clone()
    out["gpart_bwd2"] = eng.gpart[0].cpu().clone()            # [G, p_stride] as the kernels left them
    out["g_bwd2"] = eng.gpart[0].double().sum(0)[:P].cpu().clone()
    eng.run_stages(4, 4)                                      # bwd1
    torch.cuda.synchronize()
    out["gpart"] = eng.gpart[0].cpu().clone()
    out["g_all"] = eng.gpart[0].double().sum(0)[:P].cpu().clone()
    eng.run_stages(5, 5)
    torch.cuda.synchronize()
    return out


def _decode_plane_image(act1):
    """A plane image (h1; since round 6 also h2) the split forward leaves for the FUSED backward (gemm_mode 7): per 64-point tile 32 KB -- the footprint of the
    fp32 rows it replaces -- holding two fp16 planes [64][128], hi = fp16(2^6 h1) and lo = fp16(2^6 h1 - hi), each row's sixteen
    16-byte granules XOR-swizzled (ndp_fwd_split.inc: bf_swz).  -> [rows][128] float32 (hi + lo carries 22 bits: exact in fp32)."""
    rows = act1.shape[0] // 64 * 64
    img = act1[:rows].contiguous().view(torch.float16).view(rows // 64, 2, 64, 128).float()
    p = torch.arange(64)
    g = torch.tensor([0, 2, 3, 1])
    swz = ((((p & 3) << 2) | g[(p >> 2) & 3]) << 3)[:, None]
    idx = (torch.arange(128)[None, :] ^ swz).expand(rows // 64, 2, 64, 128)
    planes = torch.gather(img, 3, idx)
    out = torch.full_like(act1, float("nan"))
    val = (planes[:, 0] + planes[:, 1]) / 64.0
    # the ReLU mask is the HI plane's SIGN BIT (round 6: hi = -0 where the pre-activation is <= 0, hi >= +0 where it is positive -- a
    # positive activation below fp16's range has hi = +0 and its value in lo, or nothing at all): a positive element whose parts sum to
    # zero decodes to a positive value below everything else
    val = torch.where(~torch.signbit(planes[:, 0]) & (val <= 0), torch.full_like(val, 2.0 ** -40), val)
    out[:rows] = val.reshape(rows, 128)
    return out


def _f64_reference(r, dtype=torch.float64):
    """float64 evaluation of each kernel from that kernel's own inputs (dtype = torch.float32: the same lines in float32, the yardstick)."""
    d, n, P = r["desc"], r["n"], r["params"].to(dtype)
    W = d.width
    nh = d.n_heads
    W0 = P[d.off_W(0):d.off_W(0) + W * 6].view(W, 6); b0 = P[d.off_b(0):d.off_b(0) + W]
    W1 = P[d.off_W(1):d.off_W(1) + W * W].view(W, W); b1 = P[d.off_b(1):d.off_b(1) + W]
    W2 = P[d.off_W(2):d.off_W(2) + W * W].view(W, W); b2 = P[d.off_b(2):d.off_b(2) + W]
    Wh = P[d.off_Wh:d.off_Wh + nh * W].view(nh, W); bh = P[d.off_bh:d.off_bh + nh]
    pe = r["heads"][:n, 16:22].to(dtype)                      # the forward's own layer-0 input
    ref = {}
    # ---- forward: pe -> h0, h1, h2, scaled head outputs
    h0 = torch.relu(pe @ W0.T + b0); h1 = torch.relu(h0 @ W1.T + b1); h2 = torch.relu(h1 @ W2.T + b2)
    ref["h0"], ref["h1"], ref["h2"] = h0, h1, h2
    ref["heads"] = torch.tensor(np.float32(d.mlp_scale).item(), dtype=dtype) * (h2 @ Wh.T + bh)
    # ---- bwd2 from ITS inputs: dO, h2, h1 as the forward kernel left them
    dO = r["dO"][:n, :nh].to(dtype)
    g_h0, g_h1, g_h2 = (r["act_fwd"][k, :n].to(dtype) for k in range(3))
    dz2 = (dO @ Wh) * (g_h2 > 0)
    ref["dWh"], ref["dbh"] = dO.T @ g_h2, dO.sum(0)
    ref["dW2"], ref["db2"] = dz2.T @ g_h1, dz2.sum(0)
    ref["dz1"] = (dz2 @ W2) * (g_h1 > 0)
    # ---- bwd1 from ITS inputs: dz1 as bwd2 left it, h0, pe
    dz1 = r["dz1"][:n].to(dtype)
    ref["dW1"], ref["db1"] = dz1.T @ g_h0, dz1.sum(0)
    dz0 = (dz1 @ W1) * (g_h0 > 0)
    ref["dW0"], ref["db0"] = dz0.T @ pe, dz0.sum(0)
    return ref


def _kernel_outputs(r):
    d, n, W, nh = r["desc"], r["n"], r["desc"].width, r["desc"].n_heads
    ga, g2 = r["g_all"], r["g_bwd2"]
    return {
        "h0": r["act_fwd"][0, :n].double(), "h1": r["act_fwd"][1, :n].double(), "h2": r["act_fwd"][2, :n].double(),
        "heads": r["heads"][:n, :nh].double(),
        "dWh": g2[d.off_Wh:d.off_Wh + nh * W].view(nh, W), "dbh": g2[d.off_bh:d.off_bh + nh],
        "dW2": g2[d.off_W(2):d.off_W(2) + W * W].view(W, W), "db2": g2[d.off_b(2):d.off_b(2) + W],
        "dz1": r["dz1"][:n].double(),
        "dW1": ga[d.off_W(1):d.off_W(1) + W * W].view(W, W), "db1": ga[d.off_b(1):d.off_b(1) + W],
        "dW0": ga[d.off_W(0):d.off_W(0) + W * 6].view(W, 6), "db0": ga[d.off_b(0):d.off_b(0) + W],
    }


def _errors(r):
    """per tensor: (max |error| / max |reference|, rms error / rms reference, number of elements)."""
    ref, got = _f64_reference(r), _kernel_outputs(r)
    out = {}
    for k in ref:
        e = got[k] - ref[k]
        out[k] = (float(e.abs().max() / ref[k].abs().max().clamp_min(1e-300)),
                  float(e.pow(2).mean().sqrt() / ref[k].pow(2).mean().sqrt().clamp_min(1e-300)), ref[k].numel())
    return out


# ------------------------------------------------------------------------------------------------ the bar
def yardsticks(r):
    """per tensor: dict(err, yardstick, scale, elements) -- the kernel's max error against float64, the float32 evaluation's max error
    against the same float64 values, max |reference|."""
    ref64, ref32, got = _f64_reference(r), _f64_reference(r, torch.float32), _kernel_outputs(r)
    return {k: dict(err=float((got[k] - ref64[k]).abs().max()), yardstick=float((ref32[k].double() - ref64[k]).abs().max()),
                    scale=float(ref64[k].abs().max()), elements=ref64[k].numel()) for k in TENSORS}


def factor_of(gemm_mode, elements):
    """How many yardsticks an arithmetic may be off by: 4 for the fp32 chain; for the split kernels 4 r, r being what
    tests/test_split_accuracy.py grants the split over the chain in maximum error (2 from 10 000 elements on, 3 below)."""
    if (gemm_mode & 7) != 7:
        return 4.0
    return 4.0 * (2.0 if elements >= 10000 else 3.0)


CAP = 5e-6                                         # on top of the bar: every tensor within 5e-6 of its own scale


def allowed(q, gemm_mode):
    """The bar of one tensor: max(factor x yardstick, 16 float32 ulps of max |ref|)."""
    return max(factor_of(gemm_mode, q["elements"]) * q["yardstick"], 16.0 * ULP * q["scale"])


def ratio(q, gemm_mode):
    """The error in yardsticks (or in floors, where the floor is the bar): a tensor passes at ratio <= factor_of(...)."""
    unit = allowed(q, gemm_mode) / factor_of(gemm_mode, q["elements"])
    return q["err"] / unit if unit > 0 else (0.0 if q["err"] == 0 else float("inf"))
