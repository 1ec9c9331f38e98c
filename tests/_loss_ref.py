"""Reference of the tick's loss stage (k_eng_loss) for tests/test_loss_stage.py and tests/test_loss_stage_cpu.py -- torch on the CPU,
no GPU and no native library needed.

What the stage computes from its inputs, restated in torch and differentiated by autograd (it is not a transcription of the kernel:
no scatter, no buckets, no chunks):

    x'  = head warp of the level input x with the scaled head outputs o        (nets.py:117-135)
    L   = [K > 0] mean_k |x'_k - ldmk_t_k|^2
        + c ( (1/S) sum_i m_i |x'_{K+i} - y_{idx_x[i]}| + (1/T) sum_j n_j |x'_{K+idx_y[j]} - y_j| )      c = w_cd if K > 0 else 1
        + w_reg mean_p( -max(log(1 - nr_p), -100) )                                                     gated levels only
    dO  = mlp_scale dL/do

The nearest-neighbour indices and the truncation masks m_i = !(d2x[i] >= trunc), n_j = !(d2y[j] >= trunc) come from the STORED float32
results: that decision is the NN stage's arithmetic, not this stage's.  `evaluate(snap, dtype)` runs in float64 (the reference) or in
float32 (the yardstick the kernel's error is measured against).
"""
import dataclasses
from types import SimpleNamespace

import numpy as np
import torch

DEC_STEP, DEC_ADVANCE, DEC_STEP_ADVANCE, DEC_IDLE = 0, 1, 2, 3


def level_desc(desc, level):
    """An engine's descriptor carries nonrigidity = True for "every level but the first is gated" (nets.py:26)."""
    return dataclasses.replace(desc, nonrigidity=bool(desc.nonrigidity and level > 0))


def _skew(w):
    z = torch.zeros_like(w[:, 0])
    return torch.stack([torch.stack([z, -w[:, 2], w[:, 1]], -1), torch.stack([w[:, 2], z, -w[:, 0]], -1),
                        torch.stack([-w[:, 1], w[:, 0], z], -1)], -2)


def _rotation(d, o):
    r = o[:, :3]
    if d.rotfmt == "axis_angle":                       # nets.py:150-153, rigid_body.py:113-119 (Rodrigues)
        theta = r.norm(dim=-1, keepdim=True)
        K = _skew(r / theta)
        eye = torch.eye(3, dtype=o.dtype).expand(o.shape[0], 3, 3)
        return eye + torch.sin(theta)[:, :, None] * K + (1 - torch.cos(theta))[:, :, None] * (K @ K)
    if d.rotfmt == "euler":                            # rigid_body.py:19-56, convention X, Y, Z: R = Mx My Mz
        s, c = torch.sin(r), torch.cos(r)
        one, z = torch.ones_like(s[:, 0]), torch.zeros_like(s[:, 0])
        m3 = lambda rows: torch.stack([torch.stack(q, -1) for q in rows], -2)
        Mx = m3([[one, z, z], [z, c[:, 0], -s[:, 0]], [z, s[:, 0], c[:, 0]]])
        My = m3([[c[:, 1], z, s[:, 1]], [z, one, z], [-s[:, 1], z, c[:, 1]]])
        Mz = m3([[c[:, 2], -s[:, 2], z], [s[:, 2], c[:, 2], z], [z, z, one]])
        return Mx @ My @ Mz
    if d.rotfmt == "quaternion":                       # nets.py:154-157, rigid_body.py:58-85
        raw = o[:, :4]
        norm = raw.norm(dim=-1, keepdim=True)
        q = raw / torch.where(raw[:, :1] < 0, -norm, norm)      # unit length, real part >= 0 (the norm carries component 0's sign)
        w, x, y, z = q.unbind(-1)
        k = 2.0 / (q * q).sum(-1)                      # 2 / |q|^2 of the normalised quaternion, as the reference forms it again
        rows = [[1 - k * (y * y + z * z), k * (x * y - z * w), k * (x * z + y * w)],
                [k * (x * y + z * w), 1 - k * (x * x + z * z), k * (y * z - x * w)],
                [k * (x * z - y * w), k * (y * z + x * w), 1 - k * (x * x + y * y)]]
        return torch.stack([torch.stack(q3, -1) for q3 in rows], -2)
    if d.rotfmt == "6D":                               # rigid_body.py:5-16: Gram-Schmidt, rows b1, b2, b1 x b2
        a1, a2 = o[:, 0:3], o[:, 3:6]
        unit = lambda v: v / v.norm(dim=-1, keepdim=True).clamp_min(1e-12)         # (F.normalize's own floor)
        b1 = unit(a1)
        b2 = unit(a2 - (b1 * a2).sum(-1, keepdim=True) * b1)
        return torch.stack([b1, b2, torch.linalg.cross(b1, b2, dim=-1)], -2)
    raise NotImplementedError(d.rotfmt)


def head_warp(d, o, x):
    """d: the LEVEL's descriptor (level_desc); o [n, nh] scaled head outputs; x [n, 3] -> (x' [n, 3], nr [n] | None)."""
    t = o[:, d.row_trn:d.row_trn + 3]
    if d.motion == "sflow":
        xw = x + t
    else:
        rx = (_rotation(d, o) @ x[:, :, None])[:, :, 0]
        xw = (o[:, d.row_scale:d.row_scale + 1] + 1) * rx + t if d.motion == "Sim3" else rx + t
    if not d.nonrigidity:
        return xw, None
    nr = torch.sigmoid(o[:, d.row_nr])
    return x + nr[:, None] * (xw - x), nr


def evaluate(snap, dtype=torch.float64):
    """snap: the stage's inputs of ONE pair as CPU tensors / numbers --
        desc (engine descriptor), level, K, S, T, w_cd, trunc, w_reg,
        heads [>= n, >= nh] f32, x_in [>= n, 3] f32, ldmk_t [>= K, 3], tgt [>= T, 3], d2x [>= S] f32, idx_x [>= S], d2y [>= T] f32, idx_y [>= T]
    -> SimpleNamespace(loss (python float), dO [n, nh], xw [n, 3], gx [n, 3] = dL/dx')  in `dtype`."""
    d = level_desc(snap.desc, snap.level)
    K, S, T = snap.K, snap.S, snap.T
    n, nh = K + S, d.n_heads
    o = snap.heads[:n, :nh].to(dtype).clone().requires_grad_()
    xw, nr = head_warp(d, o, snap.x_in[:n].to(dtype))
    xw.retain_grad()
    loss = torch.zeros((), dtype=dtype)
    if K > 0:
        loss = loss + ((xw[:K] - snap.ldmk_t[:K].to(dtype)) ** 2).sum(-1).mean()
    if S > 0 and snap.w_cd != 0.0 and T > 0:
        trunc = float(np.float32(snap.trunc))                  # (a float32 value: the comparison below runs in float32)
        xs, y = xw[K:], snap.tgt[:T].to(dtype)
        keep_x = ~(snap.d2x[:S] >= trunc)                      # float32 against float32, as stored
        keep_y = ~(snap.d2y[:T] >= trunc)
        ix, iy = snap.idx_x[:S].long(), snap.idx_y[:T].long()
        assert 0 <= int(ix.min()) and int(ix.max()) < T and 0 <= int(iy.min()) and int(iy.max()) < S
        dx = (xs[keep_x] - y[ix[keep_x]]).norm(dim=-1)
        dy = (xs[iy[keep_y]] - y[keep_y]).norm(dim=-1)
        cd = dx.sum() / S + dy.sum() / T
        loss = loss + (float(np.float32(snap.w_cd)) * cd if K > 0 else cd)
    if nr is not None and snap.w_reg > 0:
        loss = loss + float(np.float32(snap.w_reg)) * (-torch.clamp(torch.log(1 - nr), min=-100.0)).mean()
    if loss.requires_grad:
        loss.backward()
    go = o.grad if o.grad is not None else torch.zeros_like(o)
    gx = xw.grad if xw.grad is not None else torch.zeros_like(xw)
    scale = torch.tensor(np.float32(d.mlp_scale).item(), dtype=dtype)
    return SimpleNamespace(loss=float(loss.detach()), dO=(scale * go).detach(), xw=xw.detach(), gx=gx.detach())


# ------------------------------------------------------------------------------------------------ the bar
def bar(kernel, ref64, ref32, factor=4.0):
    """-> dict(err, yardstick, allowed, ratio): the kernel's max error against the float64 reference, the float32 evaluation's max
    error against the same (the yardstick), and the bar  max(factor * yardstick, 2^-22 max|ref|).  ratio = err / (allowed / factor),
    i.e. "how many yardsticks (or floors)": the case passes at ratio <= factor."""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64).reshape(-1)
    err = float((torch.as_tensor(kernel).double().reshape(-1) - ref64).abs().max()) if ref64.numel() else 0.0
    yard = float((torch.as_tensor(ref32).double().reshape(-1) - ref64).abs().max()) if ref64.numel() else 0.0
    floor = 2.0 ** -22 * (float(ref64.abs().max()) if ref64.numel() else 0.0)
    allowed = max(factor * yard, floor)
    unit = allowed / factor
    return dict(err=err, yardstick=yard, floor=floor, allowed=allowed, ratio=(err / unit if unit > 0 else (0.0 if err == 0 else float("inf"))))


# ------------------------------------------------------------------------------------------------ the next pair state
def next_state(st, loss, cfg):
    """registration.py:226-249 (+ :179-180) on a pair-state record.  st: anything with the PairState fields; loss: the float32 loss the
    stage stored; cfg: m, iters, early_stop, max_break_count, break_threshold_ratio -> dict of the fields of the next record."""
    out = {f: getattr(st, f) for f in ("level", "iter", "break_counter", "adam_t", "cur", "total_steps", "total_evals", "loss_prev")}
    out["evals_per_level"] = list(st.evals_per_level)
    if st.level >= cfg.m:                                       # finished / parked: a copy with decision IDLE
        out.update(decision=DEC_IDLE, step_level=st.step_level, step_t=st.step_t, loss=st.loss)
        return out
    bc, lp, stop = st.break_counter, st.loss_prev, False
    if cfg.early_stop:
        L = float(np.float32(loss))
        if L < 1e-4:
            stop = True
        else:
            if abs(lp - L) < lp * cfg.break_threshold_ratio:
                bc += 1
            if bc >= cfg.max_break_count:
                stop = True
            else:
                lp = L
    decision = DEC_ADVANCE if stop else (DEC_STEP_ADVANCE if st.iter + 1 >= cfg.iters else DEC_STEP)
    out.update(decision=decision, total_evals=st.total_evals + 1, step_level=st.level, step_t=st.adam_t + 1)
    if decision != DEC_ADVANCE:                                 # an Adam step follows this evaluation
        out["total_steps"] = st.total_steps + 1
    if decision == DEC_STEP:
        out.update(iter=st.iter + 1, adam_t=st.adam_t + 1, break_counter=bc, loss_prev=lp)
    else:                                                       # level hand-over: fresh counters, the other point plane
        out.update(level=st.level + 1, iter=0, adam_t=0, break_counter=0, loss_prev=1e6, cur=st.cur ^ 1)
        out["evals_per_level"][st.level] = st.iter + 1
    return out


# ------------------------------------------------------------------------------------------------ inputs
def cloud(n, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return ((torch.rand(n, 3, generator=g) - 0.5) * scale).contiguous()


def clouds(K, S, T, seed):
    """-> (pts [K + S, 3] landmarks first, ldmk_t [K, 3] | None, tgt [T, 3] | None): random clouds in general position (no source on a
    target), the target rotated and shifted against the source."""
    src = cloud(K + S, 100 + seed)
    c, s_ = np.cos(0.2), np.sin(0.2)
    Rz = torch.tensor([[c, -s_, 0.0], [s_, c, 0.0], [0.0, 0.0, 1.0]], dtype=torch.float32)
    tgt = (cloud(T, 200 + seed) @ Rz.T + torch.tensor([0.03, -0.02, 0.01])).contiguous() if T else None
    lt = ((src[:K] + 0.04 * torch.sin(4 * src[:K])) @ Rz.T).contiguous() if K else None
    return src, lt, tgt


# ------------------------------------------------------------------------------------------------ crafted target -> source assignments
# Each generator returns int32 [T] with every entry inside [0, S): the kernel dereferences them.  `checked` is the one way out.
def checked(idx, S, T):
    idx = np.asarray(idx)
    if idx.shape != (T,) or idx.dtype.kind != "i" or T < 1 or int(idx.min()) < 0 or int(idx.max()) >= S:
        raise ValueError(f"crafted index outside [0, {S}) or of the wrong shape {idx.shape} for T = {T}")
    return torch.from_numpy(idx.astype(np.int32))


def sample_of_point(K, S, p):
    """Sample index of engine point p (thread p % 256 of gradient block p // 256)."""
    i = p - K
    if not 0 <= i < S:
        raise ValueError(f"point {p} is not a sample of a pair with K = {K}, S = {S}")
    return i


def craft_all_one(K, S, T, i):
    """Every target names sample i."""
    return checked(np.full(T, i, dtype=np.int64), S, T)


def craft_alternate(K, S, T, i, j):
    """Even targets name sample i, odd ones sample j."""
    return checked(np.where(np.arange(T) % 2 == 0, i, j), S, T)


def craft_block(K, S, T, block):
    """Only samples whose point lies in gradient block `block` (points 256 block .. 256 block + 255) are named, round robin."""
    lo, hi = max(256 * block - K, 0), min(256 * (block + 1) - K, S)
    if hi <= lo:
        raise ValueError(f"block {block} holds no sample of a pair with K = {K}, S = {S}")
    return checked(lo + np.arange(T) % (hi - lo), S, T)


def craft_permutation(K, S, T, seed):
    """Every sample is named exactly once (S == T)."""
    if S != T:
        raise ValueError("a permutation needs S == T")
    return checked(np.random.default_rng(seed).permutation(S), S, T)


def crafted_d2y(xs32, tgt32, idx):
    """float32 squared distance of target j to the sample it now names, from float32 coordinates (differences, squares and the
    three-term sum each rounded to float32: the values a float32 NN stage would store)."""
    e = (xs32[idx.long()] - tgt32).float()
    return ((e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]) + e[:, 2] * e[:, 2]).contiguous()
