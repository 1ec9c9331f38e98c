"""torch-tensor wrappers around the single-pair operators of libndp_hip.so.

Torch is plumbing here: it owns device memory and the stream; all arithmetic is in the HIP
library.  Every function requires CUDA(HIP) float32 contiguous tensors and raises otherwise --
there is no CPU / eager fallback.
"""
import ctypes
import math

import torch
from torch.autograd.function import once_differentiable

from . import _native as N
from .layout import LayerDesc

TILE = N.TILE


def _chk(t, name, dtype=torch.float32):
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise N.NdpError(f"{name}: the HIP path needs a tensor on the GPU (got {getattr(t, 'device', type(t))}); "
                         "there is no CPU fallback")
    if t.dtype != dtype:
        raise N.NdpError(f"{name}: expected {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise N.NdpError(f"{name}: tensor must be contiguous")
    return t


def _p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def cap(n):
    return max(TILE, (n + TILE - 1) // TILE * TILE)


def _workspace(entry, dims, dev, dtype=torch.float32, per=1):
    """Ask the library's size query `entry`(*dims, &size) and allocate that workspace on dev: a tensor of `dtype`, one element of
    which holds `per` of the query's units (floats or bytes; the count is rounded up).  Every entry accepts a workspace at least as
    large as its query asked for, so a caller that must name the size passes the tensor's own (4 * ws.numel() bytes: the KPConv
    queries answer in multiples of 16 bytes, so that is their figure)."""
    size = ctypes.c_longlong()
    N.check(getattr(N.lib(), entry)(*dims, ctypes.byref(size)), entry)
    return torch.empty((size.value + per - 1) // per, device=dev, dtype=dtype)


def _nn_result(S, T, dev):
    """The tensors of a nearest-neighbour result, unfilled: (d2x [S], ix [S] int32, d2y [T], iy [T] int32)."""
    return (torch.empty(S, device=dev), torch.empty(S, device=dev, dtype=torch.int32),
            torch.empty(T, device=dev), torch.empty(T, device=dev, dtype=torch.int32))


def _check_prev_idx(prev_idx_x, S, prev_idx_y, T):
    for p, n, name in ((prev_idx_x, S, "prev_idx_x"), (prev_idx_y, T, "prev_idx_y")):
        if p is not None and (p.dtype != torch.int32 or not p.is_cuda or not p.is_contiguous() or p.numel() != n):
            raise ValueError(f"{name} must be a contiguous int32 device tensor with one entry per query")


def _host_offsets(n, offsets, name, dev):
    """offsets over n rows (None: one problem; else B + 1 ascending ints, host side) -> (device int32 tensor, ctypes host copy).  The
    entries check the host copy; the kernels read the device one."""
    off = [0, n] if offsets is None else [int(v) for v in (offsets.tolist() if isinstance(offsets, torch.Tensor) else offsets)]
    if len(off) < 2 or off[0] != 0 or off[-1] != n:
        raise ValueError(f"{name} must run from 0 to {n} in B + 1 entries, got {off[:4]}{'...' if len(off) > 4 else ''}")
    return torch.tensor(off, dtype=torch.int32).to(dev), (ctypes.c_int * len(off))(*off)


def level_fwd(desc: LayerDesc, params, level, k0, x, save=False, want_nonrig=False):
    """x [n,3] -> x_out [n,3]; with save also (act [depth,cap,width], heads [cap,24]; [3,cap,128] for the shipped 128 / 3); with
    want_nonrig the gate values [n] of a level that carries the nonrigidity head are appended.  width / depth other than 128 / 3 run on
    the generic fp32 kernels (csrc/ndp_generic.inc), bitwise the oracle's chain."""
    _chk(params, "params"); _chk(x, "x")
    n = x.shape[0]
    out = torch.empty_like(x)
    act = heads = nr = None
    if save:
        c = cap(n)
        act = torch.empty(desc.n_hidden + 1, c, desc.width, device=x.device, dtype=torch.float32)
        heads = torch.empty(c, N.HROW, device=x.device, dtype=torch.float32)
    if want_nonrig and desc.nonrigidity:
        nr = torch.empty(n, device=x.device, dtype=torch.float32)
    cd = desc.c_struct()
    N.check(N.lib().ndp_level_fwd(ctypes.byref(cd), _p(params), int(level), int(k0), _p(x), n, _p(out),
                                  _p(act), _p(heads), _p(nr), N.stream_ptr(x.device)), "ndp_level_fwd")
    res = (out, act, heads) if save else (out,)
    if want_nonrig:
        res = res + (nr,)
    return res if len(res) > 1 else res[0]


def level_bwd(desc: LayerDesc, params, level, k0, x, act, heads, g, n_part=None, g_nr=None, want_dx=False):
    """-> grads [P] (partials folded in index order on the device).  `act` is consumed.
    want_dx: -> (grads, dx [n,3]) with dx = dL/dx of the level's input points (the warp's own dependence on x plus the path
    through the positional encoding and the network); grads are the same bits with and without."""
    _chk(params, "params"); _chk(x, "x"); _chk(act, "act"); _chk(heads, "heads"); _chk(g, "g")
    if g_nr is not None:
        _chk(g_nr, "g_nr")
    n = x.shape[0]
    if tuple(act.shape) != (desc.n_hidden + 1, cap(n), desc.width) or tuple(heads.shape) != (cap(n), N.HROW):
        raise N.NdpError(f"level_bwd: act must be [{desc.n_hidden + 1}, {cap(n)}, {desc.width}] and heads [{cap(n)}, {N.HROW}] as level_fwd(save=True) left them")
    P = desc.param_count
    stride = (P + 3) // 4 * 4
    tiles = (n + TILE - 1) // TILE
    if n_part is None:
        n_part = min(tiles, 256)
    part = torch.empty(n_part, stride, device=x.device, dtype=torch.float32)
    work = torch.empty(cap(n), N.NHMAX, device=x.device, dtype=torch.float32)
    cd = desc.c_struct()
    st = N.stream_ptr(x.device)
    dx = torch.empty_like(x) if want_dx else None
    N.check(N.lib().ndp_level_bwd(ctypes.byref(cd), _p(params), int(level), int(k0), _p(x), n, _p(act), _p(heads),
                                  _p(g), _p(g_nr), _p(work), _p(part), n_part, stride, st, _p(dx)), "ndp_level_bwd")
    grads = torch.empty(P, device=x.device, dtype=torch.float32)
    N.check(N.lib().ndp_grad_reduce(_p(part), n_part, stride, P, _p(grads), st), "ndp_grad_reduce")
    return (grads, dx) if want_dx else grads


def pyramid_fwd(desc: LayerDesc, m, k0, store, x):
    """store [m, p_stride] (level l in row l) ; x [n,3] -> [n,3]."""
    _chk(store, "store"); _chk(x, "x")
    out = torch.empty_like(x)
    cd = desc.c_struct()
    N.check(N.lib().ndp_pyramid_fwd(ctypes.byref(cd), int(m), int(k0), _p(store), store.stride(0), _p(x), x.shape[0],
                                    _p(out), N.stream_ptr(x.device)), "ndp_pyramid_fwd")
    return out


def _levels(m, min_level, max_level):
    max_level = int(m) - 1 if max_level is None else int(max_level)
    return int(min_level), max_level


def pyramid_jacobian(desc: LayerDesc, m, k0, store, x, min_level=0, max_level=None, normals=None):
    """The warp of levels min_level..max_level and its per-point Jacobian in one launch (csrc/ndp_jacobian.inc).
    store [m, p_stride], x [n,3] -> (x' [n,3], J [n,3,3]) with J[p, a, b] = d x'_a / d x_b; with normals [n,3] also
    n' = cof(J) n / |cof(J) n| (J^-T n up to the factor det J; its sign follows the cofactor matrix where det J < 0).
    x' is bit for bit pyramid_fwd's.  desc.nonrigidity means "every level but the first is gated", as for pyramid_fwd."""
    _chk(store, "store"); _chk(x, "x")
    if normals is not None:
        _chk(normals, "normals")
        if normals.shape != x.shape:
            raise N.NdpError("pyramid_jacobian: normals must have the shape of x")
    lo, hi = _levels(m, min_level, max_level)
    n = x.shape[0]
    out = torch.empty_like(x)
    J = torch.empty(n, 3, 3, device=x.device, dtype=torch.float32)
    nout = torch.empty_like(x) if normals is not None else None
    cd = desc.c_struct()
    N.check(N.lib().ndp_pyramid_jac(ctypes.byref(cd), int(m), int(k0), _p(store), store.stride(0), lo, hi, _p(x), n, _p(out), _p(J),
                                    _p(normals), _p(nout), N.stream_ptr(x.device)), "ndp_pyramid_jac")
    return (out, J) if normals is None else (out, J, nout)


def pyramid_inverse(desc: LayerDesc, m, k0, store, y, min_level=0, max_level=None, x0=None, iters=8, tol=2e-6):
    """Newton on warp(x) = y for levels min_level..max_level, every iteration inside one launch.  y [n,3]; x0 [n,3] the first guess
    (None: y) -> (x [n,3], residual [n] = max |warp(x) - y| of the x returned, status [n] int32: Newton steps taken when converged,
    -1 not converged within iters, -2 stopped on a singular Jacobian or non-finite values)."""
    _chk(store, "store"); _chk(y, "y")
    lo, hi = _levels(m, min_level, max_level)
    n = y.shape[0]
    if x0 is not None:
        _chk(x0, "x0")
        if x0.shape != y.shape:
            raise N.NdpError("pyramid_inverse: x0 must have the shape of y")
    x = (y if x0 is None else x0).clone()
    res = torch.empty(n, device=y.device, dtype=torch.float32)
    status = torch.empty(n, device=y.device, dtype=torch.int32)
    cd = desc.c_struct()
    N.check(N.lib().ndp_pyramid_inverse(ctypes.byref(cd), int(m), int(k0), _p(store), store.stride(0), lo, hi, _p(y), n, _p(x), int(iters),
                                        float(tol), _p(res), _p(status), N.stream_ptr(y.device)), "ndp_pyramid_inverse")
    return x, res, status


def pyramid_fwd_batch(desc: LayerDesc, m, k0, jobs, device=None, split=False, tiles=None):
    """jobs: [(store [m,p_stride], x [n,3], shift_in [>=3] | None, shift_out [>=3] | None)] -> [x_out [n,3]]: every
    cloud through its whole pyramid in ONE launch per 32 jobs; x_out = pyramid(x - shift_in) + shift_out.
    split: the engine's fp16-split arithmetic (k_pyramid_fwd8) instead of the fp32 MFMA (bitwise the level chain).
    tiles (split only): 64-point tiles per workgroup, 1..8 (default 4; the batched engine passes 8: half the weight prologues)."""
    if not jobs:
        return []
    arr = (N.WarpJob * len(jobs))()
    outs = []
    stride = None
    for q, (store, x, s_in, s_out) in zip(arr, jobs):
        _chk(store, "store"); _chk(x, "x")
        if s_in is not None:
            _chk(s_in, "shift_in")
        if s_out is not None:
            _chk(s_out, "shift_out")
        if stride is None:
            stride = store.stride(0)
        elif stride != store.stride(0):
            raise N.NdpError("pyramid_fwd_batch: all stores must share one row stride")
        out = torch.empty_like(x)
        outs.append(out)
        q.params, q.x, q.x_out = store.data_ptr(), x.data_ptr(), out.data_ptr()
        q.shift_in = s_in.data_ptr() if s_in is not None else None
        q.shift_out = s_out.data_ptr() if s_out is not None else None
        q.n = x.shape[0]
    cd = desc.c_struct()
    dev = device if device is not None else jobs[0][1].device
    if split and tiles is not None:
        N.check(N.lib().ndp_pyramid_fwd_batch_split_tiles(ctypes.byref(cd), int(m), int(k0), int(stride), arr, len(jobs), int(tiles),
                                                          N.stream_ptr(dev)), "ndp_pyramid_fwd_batch_split_tiles")
        return outs
    fn = N.lib().ndp_pyramid_fwd_batch_split if split else N.lib().ndp_pyramid_fwd_batch
    N.check(fn(ctypes.byref(cd), int(m), int(k0), int(stride), arr, len(jobs), N.stream_ptr(dev)), "ndp_pyramid_fwd_batch")
    return outs


def pair_means(src, tgt, out=None):
    """-> means [8] on the device: [0:3] mean of src, [4:7] mean of tgt (registration.py:150-153)."""
    _chk(src, "src"); _chk(tgt, "tgt")
    if out is None:
        out = torch.empty(8, device=src.device, dtype=torch.float32)
    N.check(N.lib().ndp_pair_means(_p(src), src.shape[0], _p(tgt), tgt.shape[0], _p(out), N.stream_ptr(src.device)),
            "ndp_pair_means")
    return out


def chamfer_nn(x, y):
    _chk(x, "x"); _chk(y, "y")
    S, T = x.shape[0], y.shape[0]
    d2x, ix, d2y, iy = _nn_result(S, T, x.device)
    N.check(N.lib().ndp_chamfer_nn_fwd(_p(x), S, _p(y), T, _p(d2x), _p(ix), _p(d2y), _p(iy), N.stream_ptr(x.device)),
            "ndp_chamfer_nn_fwd")
    return d2x, ix, d2y, iy


def chamfer_nn_onepass(x, y, matrix=False):
    """Same result as chamfer_nn from one pass over the S x T distances (the engine's per-tick kernels as an operator);
    matrix: the variant that forms the distances on the bf16 matrix pipe and re-evaluates the candidates exactly (engine nn_mode 2)."""
    _chk(x, "x"); _chk(y, "y")
    S, T = x.shape[0], y.shape[0]
    ws_row = _workspace("ndp_engine_nn_workspace", (cap(S), cap(T)), x.device)
    d2x, ix, d2y, iy = _nn_result(S, T, x.device)
    fn = N.lib().ndp_chamfer_nn_matrix if matrix else N.lib().ndp_chamfer_nn_onepass
    N.check(fn(_p(x), S, _p(y), T, _p(d2x), _p(ix), _p(d2y), _p(iy), _p(ws_row), N.stream_ptr(x.device)),
            "ndp_chamfer_nn_matrix" if matrix else "ndp_chamfer_nn_onepass")
    return d2x, ix, d2y, iy


def chamfer_nn_cells(x, y, prev_idx_x=None, prev_idx_y=None):
    """Same result as chamfer_nn from the exact grid ball search (the NN stage of an engine with nn_cells, as an operator; S, T <= 2048).
    prev_idx_x [S] / prev_idx_y [T] (int32, optional): seed indices, e.g. the previous call's; ANY values give the same result."""
    _chk(x, "x"); _chk(y, "y")
    S, T = x.shape[0], y.shape[0]
    _check_prev_idx(prev_idx_x, S, prev_idx_y, T)
    ws = _workspace("ndp_chamfer_nn_cells_workspace", (T,), x.device)
    d2x, ix, d2y, iy = _nn_result(S, T, x.device)
    N.check(N.lib().ndp_chamfer_nn_cells(_p(x), S, _p(y), T, _p(prev_idx_x), _p(prev_idx_y), _p(d2x), _p(ix), _p(d2y), _p(iy), _p(ws),
                                         N.stream_ptr(x.device)), "ndp_chamfer_nn_cells")
    return d2x, ix, d2y, iy


def chamfer_nn_cells_wide(x, y, prev_idx_x=None, prev_idx_y=None):
    """chamfer_nn_cells for clouds of up to 8192 points (the NN stage of an engine with nn_cells_wide, as an operator): same result as
    chamfer_nn for ANY prev_idx_x [S] / prev_idx_y [T] (int32, optional)."""
    _chk(x, "x"); _chk(y, "y")
    S, T = x.shape[0], y.shape[0]
    _check_prev_idx(prev_idx_x, S, prev_idx_y, T)
    ws = _workspace("ndp_chamfer_nn_cells_wide_workspace", (S, T), x.device)
    d2x, ix, d2y, iy = _nn_result(S, T, x.device)
    N.check(N.lib().ndp_chamfer_nn_cells_wide(_p(x), S, _p(y), T, _p(prev_idx_x), _p(prev_idx_y), _p(d2x), _p(ix), _p(d2y), _p(iy), _p(ws),
                                              N.stream_ptr(x.device)), "ndp_chamfer_nn_cells_wide")
    return d2x, ix, d2y, iy


def chamfer_l1(x, y, trunc, nn=None, want_grad=True, point_sum=False, want_grad_y=False):
    """-> (loss [1], gx [S,3] | None, nn tuple).  point_sum: point_reduction="sum" of loss.py:233-235.
    want_grad_y: -> (loss, gx, nn, gy [T,3]).  The loss is symmetric in its clouds, so gy is the same kernel with the two clouds and
    their halves of the ONE nearest-neighbour result exchanged: the bits of chamfer_l1(y, x)'s gx."""
    if nn is None:
        nn = chamfer_nn(x, y)
    d2x, ix, d2y, iy = nn
    loss = torch.empty(1, device=x.device)
    gx = torch.empty_like(x) if want_grad else None
    N.check(N.lib().ndp_chamfer_l1_bwd(_p(x), x.shape[0], _p(y), y.shape[0], float(trunc), _p(d2x), _p(ix), _p(d2y),
                                       _p(iy), _p(loss), _p(gx), 1 if point_sum else 0, N.stream_ptr(x.device)), "ndp_chamfer_l1_bwd")
    if not want_grad_y:
        return loss, gx, nn
    gy = torch.empty_like(y)
    loss_y = torch.empty(1, device=x.device)                         # (the exchanged call's own copy of the value: not used)
    N.check(N.lib().ndp_chamfer_l1_bwd(_p(y), y.shape[0], _p(x), x.shape[0], float(trunc), _p(d2y), _p(iy), _p(d2x),
                                       _p(ix), _p(loss_y), _p(gy), 1 if point_sum else 0, N.stream_ptr(x.device)), "ndp_chamfer_l1_bwd")
    return loss, gx, nn, gy


def sinkhorn_divergence(x, y, blur, reach=None, scaling=0.5, want_grad=True, want_potentials=False):
    """Debiased Sinkhorn divergence of two uniformly weighted clouds x [n,3], y [m,3], cost |u - v|^2 / 2 (the arithmetic of
    geomloss.SamplesLoss("sinkhorn", p=2, blur, reach, scaling) as restated in DESIGN.md; reach None: balanced).
    -> (loss [1], grad_x [n,3] | None, potentials [2n + 2m] = (F_ba, F_aa, G_ab, G_bb) | None).  grad_x is dloss/dx with y and the
    dual potentials held fixed.  One host read: the diameter of the joint bounding box, as the library's `.item()`."""
    _chk(x, "x"); _chk(y, "y")                                      # both devices before either shape
    _cloud(x, "x"); _cloud(y, "y")
    n, m = x.shape[0], y.shape[0]
    lo = torch.minimum(x.min(dim=0).values, y.min(dim=0).values).double()
    hi = torch.maximum(x.max(dim=0).values, y.max(dim=0).values).double()
    diameter = float((hi - lo).norm().item())
    ws = _workspace("ndp_sinkhorn_workspace", (n, m), x.device, torch.float64, per=2)      # (in floats; float64: 8-byte aligned)
    loss = torch.empty(1, device=x.device)
    gx = torch.empty_like(x) if want_grad else None
    pot = torch.empty(2 * n + 2 * m, device=x.device) if want_potentials else None
    N.check(N.lib().ndp_sinkhorn_divergence(_p(x), n, _p(y), m, float(blur), 0.0 if reach is None else float(reach), float(scaling),
                                            diameter, _p(ws), _p(loss), _p(gx), _p(pot), N.stream_ptr(x.device)),
            "ndp_sinkhorn_divergence")
    return loss, gx, pot


def _cloud(t, name):
    _chk(t, name)
    if t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"{name} must be a [N, 3] tensor with N >= 1, got {tuple(t.shape)}")
    return t


def knn(q, r, K):
    """The K nearest points of r [nr,3] for every point of q [nq,3], exact (csrc/ndp_normals.inc: k_knn)
    -> (d2 [nq,K] squared distances, idx [nq,K] int32), every row ascending in (d2, index).  1 <= K <= 32, K <= nr; column 0 at
    K = 1 is bitwise chamfer_nn's d2x / idx_x."""
    _cloud(q, "q"); _cloud(r, "r")
    nq, nr, K = q.shape[0], r.shape[0], int(K)
    d2 = torch.empty(nq, max(K, 0), device=q.device)
    idx = torch.empty(nq, max(K, 0), device=q.device, dtype=torch.int32)
    N.check(N.lib().ndp_knn(_p(q), nq, _p(r), nr, K, _p(d2), _p(idx), N.stream_ptr(q.device)), "ndp_knn")
    return d2, idx


def normals_from_knn(p, idx, viewpoint=None, want_curvature=False):
    """PCA normals of p [n,3] from neighbour lists idx [n,K] (int32, K >= 3, e.g. knn(p, p, K)[1]) -> normals [n,3], with
    want_curvature (normals, curvature [n] = l0 / (l0 + l1 + l2)).  viewpoint (3 values): normals face it; None: the component of
    largest magnitude is positive."""
    _cloud(p, "p"); _chk(idx, "idx", torch.int32)
    if idx.ndim != 2 or idx.shape[0] != p.shape[0]:
        raise ValueError(f"idx must be [{p.shape[0]}, K], got {tuple(idx.shape)}")
    vp = None
    if viewpoint is not None:
        vp = torch.as_tensor(viewpoint, dtype=torch.float32).reshape(3).to(p.device).contiguous()
    normals = torch.empty_like(p)
    curv = torch.empty(p.shape[0], device=p.device) if want_curvature else None
    N.check(N.lib().ndp_normals_from_knn(_p(p), p.shape[0], _p(idx), idx.shape[1], _p(vp), _p(normals), _p(curv), N.stream_ptr(p.device)),
            "ndp_normals_from_knn")
    return (normals, curv) if want_curvature else normals


def point_to_plane(x, y, nx, ny, trunc=math.inf, mode=0, nn=None, want_grad=True, want_grad_y=False):
    """Point-to-plane residuals of both directions on one nearest-neighbour result -> (out [4], gx [S,3] | None, nn tuple), with
    want_grad_y (out, gx, nn, gy [T,3]).  out = (sum, x part, y part, normal consistency); mode 0: the reference's formula
    (model/loss.py:87-88, the norm of the elementwise product), mode 1: the plane distance |(x - p) . n|; trunc in squared units.
    nn: chamfer_nn's tuple, so that a Chamfer term and a plane term share one search.  gy is the same entry with the clouds, the
    normals and the halves of nn exchanged."""
    _cloud(x, "x"); _cloud(y, "y"); _chk(nx, "nx"); _chk(ny, "ny")
    if nx.shape != x.shape or ny.shape != y.shape:
        raise ValueError("nx / ny must have the shapes of x / y")
    if nn is None:
        nn = chamfer_nn(x, y)
    d2x, ix, d2y, iy = nn
    S, T = x.shape[0], y.shape[0]
    out = torch.empty(4, device=x.device)
    gx = torch.empty_like(x) if want_grad else None
    N.check(N.lib().ndp_point_to_plane(_p(x), S, _p(y), T, _p(nx), _p(ny), float(trunc), _p(d2x), _p(ix), _p(d2y), _p(iy), int(mode),
                                       _p(out), _p(gx), N.stream_ptr(x.device)), "ndp_point_to_plane")
    if not want_grad_y:
        return out, gx, nn
    gy = torch.empty_like(y)
    out_y = torch.empty(4, device=x.device)                          # (the exchanged call's own copy of the values: not used)
    N.check(N.lib().ndp_point_to_plane(_p(y), T, _p(x), S, _p(ny), _p(nx), float(trunc), _p(d2y), _p(iy), _p(d2x), _p(ix), int(mode),
                                       _p(out_y), _p(gy), N.stream_ptr(x.device)), "ndp_point_to_plane")
    return out, gx, nn, gy


def _rigid_problems(src, tgt, offsets):
    """src, tgt [sum K,3] and their row offsets (_host_offsets) -> (B, device offsets, host offsets)."""
    _cloud(src, "src"); _cloud(tgt, "tgt")
    if tgt.shape != src.shape:
        raise ValueError(f"src and tgt must list the same correspondences, got {tuple(src.shape)} and {tuple(tgt.shape)}")
    off, host = _host_offsets(src.shape[0], offsets, "offsets", src.device)
    return len(host) - 1, off, host


def rigid_fit(src, tgt, w=None, mask=None, eps=1e-4, offsets=None):
    """Weighted Procrustes (Kabsch) of correspondences src [K,3] -> tgt [K,3], the reference's arithmetic (procrustes.py:18-44) in
    double on the device (csrc/ndp_rigid.inc: k_rigid_fit) -> (R [B,3,3], t [B,3], condition [B], status [B] int32).  w [K]: weights;
    mask [K] uint8: non-zero rows weigh 1; neither: all ones.  offsets: B + 1 ascending row offsets for B problems in one call.
    status 1 (fewer than 3 weighted rows, zero weight sum) or 2 (rows on a line): identity, zero, condition inf."""
    B, off, host = _rigid_problems(src, tgt, offsets)
    if w is not None and mask is not None:
        raise ValueError("rigid_fit takes weights or a mask, not both")
    if w is not None:
        _chk(w, "w")
        if w.numel() != src.shape[0]:
            raise ValueError(f"w must hold {src.shape[0]} weights, got {tuple(w.shape)}")
    if mask is not None:
        _chk(mask, "mask", torch.uint8)
        if mask.numel() != src.shape[0]:
            raise ValueError(f"mask must hold {src.shape[0]} entries, got {tuple(mask.shape)}")
    R = torch.empty(B, 3, 3, device=src.device)
    t = torch.empty(B, 3, device=src.device)
    cond = torch.empty(B, device=src.device)
    status = torch.empty(B, device=src.device, dtype=torch.int32)
    N.check(N.lib().ndp_rigid_fit(_p(src), _p(tgt), _p(w), _p(mask), _p(off), host, B, float(eps), _p(R), _p(t), _p(cond), _p(status),
                                  N.stream_ptr(src.device)), "ndp_rigid_fit")
    return R, t, cond, status


def rigid_score(T, src, tgt, thr, offsets=None):
    """Residuals of given transforms: T [B,H,12] (or [H,12] for one problem; R row-major then t) -> (count [B,H] int32 of rows with
    |R s + t - y|^2 < thr^2, sse [B,H] the fp32 sum of those squared residuals in row order) (csrc/ndp_rigid.inc: k_rigid_score).
    With H = 1 count / K is the reference's inlier ratio."""
    B, off, host = _rigid_problems(src, tgt, offsets)
    _chk(T, "T")
    if T.ndim == 2:
        T = T[None]
    if T.ndim != 3 or T.shape[0] != B or T.shape[2] != 12 or T.shape[1] < 1:
        raise ValueError(f"T must be [{B}, H, 12] with H >= 1, got {tuple(T.shape)}")
    H = T.shape[1]
    count = torch.empty(B, H, device=src.device, dtype=torch.int32)
    sse = torch.empty(B, H, device=src.device)
    N.check(N.lib().ndp_rigid_score(_p(T), _p(src), _p(tgt), _p(off), host, B, H, float(thr), _p(count), _p(sse), N.stream_ptr(src.device)),
            "ndp_rigid_score")
    return count, sse


def ransac_rigid(src, tgt, triples, thr, edge_ratio=0.9, refine_iters=2, offsets=None, want_hypotheses=False):
    """RANSAC over given hypotheses (csrc/ndp_rigid.inc): triples [B,H,3] int32 (or [H,3]) index each problem's own rows
    (rigid.draw_triples).  -> dict(R [B,3,3], t [B,3], mask [K] uint8, count [B], rmse [B], best [B], status [B]); with
    want_hypotheses also h_count [B,H], h_flags [B,H] (1 bad index, 2 edge length, 4 collinear) and h_T [B,H,12]."""
    B, off, host = _rigid_problems(src, tgt, offsets)
    _chk(triples, "triples", torch.int32)
    if triples.ndim == 2:
        triples = triples[None]
    if triples.ndim != 3 or triples.shape[0] != B or triples.shape[2] != 3 or triples.shape[1] < 1:
        raise ValueError(f"triples must be [{B}, H, 3] with H >= 1, got {tuple(triples.shape)}")
    H, dev = triples.shape[1], src.device
    ws = _workspace("ndp_ransac_rigid_workspace", (B, H), dev, torch.int32, per=4)
    out = dict(R=torch.empty(B, 3, 3, device=dev), t=torch.empty(B, 3, device=dev), mask=torch.empty(src.shape[0], device=dev, dtype=torch.uint8),
               count=torch.empty(B, device=dev, dtype=torch.int32), rmse=torch.empty(B, device=dev),
               best=torch.empty(B, device=dev, dtype=torch.int32), status=torch.empty(B, device=dev, dtype=torch.int32))
    hc = hf = hT = None
    if want_hypotheses:
        hc = torch.empty(B, H, device=dev, dtype=torch.int32)
        hf = torch.empty(B, H, device=dev, dtype=torch.int32)
        hT = torch.empty(B, H, 12, device=dev)
        out.update(h_count=hc, h_flags=hf, h_T=hT)
    N.check(N.lib().ndp_ransac_rigid(_p(src), _p(tgt), _p(off), host, B, _p(triples), H, float(thr), float(edge_ratio), int(refine_iters),
                                     _p(ws), _p(out["R"]), _p(out["t"]), _p(out["mask"]), _p(out["count"]), _p(out["rmse"]), _p(out["best"]),
                                     _p(out["status"]), _p(hc), _p(hf), _p(hT), N.stream_ptr(dev)), "ndp_ransac_rigid")
    return out


FEAT_MODES = {"dual_softmax": 0, "sinkhorn": 1, "mutual_nn": 2}


def _feat_problems(a, b, offsets_a, offsets_b):
    """a [sum S,C], b [sum T,C] and their B + 1 host-side row offsets (None: one problem) -> (B, C, device offsets a / b, host a / b)."""
    if not isinstance(a, torch.Tensor) or not isinstance(b, torch.Tensor) or a.ndim != 2 or b.ndim != 2:
        raise ValueError(f"descriptors must be tensors [rows, C], got {getattr(a, 'shape', type(a))} and {getattr(b, 'shape', type(b))}")
    if a.shape[1] != b.shape[1]:
        raise ValueError(f"both sides need the same descriptor length C, got {a.shape[1]} and {b.shape[1]}")
    _chk(a, "a"); _chk(b, "b")
    oa, ha = _host_offsets(a.shape[0], offsets_a, "offsets_a", a.device)
    ob, hb = _host_offsets(b.shape[0], offsets_b, "offsets_b", a.device)
    if len(ha) != len(hb):
        raise ValueError(f"both sides must list the same problems, got {len(ha) - 1} and {len(hb) - 1}")
    return len(ha) - 1, a.shape[1], oa, ob, ha, hb


def feat_rowstats(a, b, alpha=1.0, v=None, e=None, offsets_a=None, offsets_b=None):
    """Row statistics of the logits alpha <a_i, b_j> + v_j, which are never stored (csrc/ndp_match.inc: k_feat_rowstats, exact fp32 on
    the f32-input MFMA) -> (lse [sum S], max [sum S], arg [sum S] int32: the lowest j, local to the problem, that attains max).
    v [sum T]: a potential per column; e [B]: one extra dustbin column per problem, which enters lse only.  Exchange a and b for the
    column statistics: a logit has the same bits either way."""
    B, C, oa, ob, ha, hb = _feat_problems(a, b, offsets_a, offsets_b)
    if v is not None:
        _chk(v, "v")
        if v.numel() != b.shape[0]:
            raise ValueError(f"v must hold one potential per row of b ({b.shape[0]}), got {tuple(v.shape)}")
    if e is not None:
        _chk(e, "e")
        if e.numel() != B:
            raise ValueError(f"e must hold one value per problem ({B}), got {tuple(e.shape)}")
    n, dev = a.shape[0], a.device
    lse, mx, arg = torch.empty(n, device=dev), torch.empty(n, device=dev), torch.empty(n, device=dev, dtype=torch.int32)
    N.check(N.lib().ndp_feat_rowstats(_p(a), _p(b), _p(oa), _p(ob), ha, hb, B, C, float(alpha), _p(v), _p(e), _p(lse), _p(mx), _p(arg),
                                      N.stream_ptr(dev)), "ndp_feat_rowstats")
    return lse, mx, arg


def feat_match(fs, ft, mode="dual_softmax", temperature=0.1, bin_score=1.0, iters=3, thr=0.1, mutual=True, offsets_s=None, offsets_t=None):
    """Matches between descriptors fs [sum S,C] and ft [sum T,C] (csrc/ndp_match.inc: ndp_feat_match, one sequence of launches) ->
    (match_t [sum S] int32: the matched target row local to the problem or -1, conf [sum S]: the confidence of each row's best
    column).  mode "dual_softmax" (temperature), "sinkhorn" (bin_score, iters) or "mutual_nn" (temperature is the score's scale,
    thr may be -inf)."""
    if mode not in FEAT_MODES:
        raise ValueError(f"mode must be one of {sorted(FEAT_MODES)}, got {mode!r}")
    B, C, os_, ot, hs, ht = _feat_problems(fs, ft, offsets_s, offsets_t)
    dev = fs.device
    ws = _workspace("ndp_feat_match_workspace", (B, fs.shape[0], ft.shape[0]), dev, torch.int32, per=4)
    match_t, conf = torch.empty(fs.shape[0], device=dev, dtype=torch.int32), torch.empty(fs.shape[0], device=dev)
    N.check(N.lib().ndp_feat_match(_p(fs), _p(ft), _p(os_), _p(ot), hs, ht, B, C, FEAT_MODES[mode], float(temperature), float(bin_score),
                                   int(iters), float(thr), int(bool(mutual)), _p(ws), _p(match_t), _p(conf), N.stream_ptr(dev)),
            "ndp_feat_match")
    return match_t, conf


def feat_conf(fs, ft, temperature=0.1, offsets_s=None, offsets_t=None):
    """The dense dual-softmax confidence matrix of descriptors fs [sum S,C] and ft [sum T,C] (csrc/ndp_match.inc: ndp_feat_conf, two
    k_feat_rowstats launches and one dense pass) -> conf [B, Smax, Tmax]: softmax over i times softmax over j of
    <fs_i, ft_j> / (C temperature) inside each problem's S x T, exactly 0 in the padding (the reference's masked batch,
    matching.py:144-157).  Does not synchronise."""
    B, C, os_, ot, hs, ht = _feat_problems(fs, ft, offsets_s, offsets_t)
    dev = fs.device
    smax = max(hs[b + 1] - hs[b] for b in range(B))
    tmax = max(ht[b + 1] - ht[b] for b in range(B))
    ws = _workspace("ndp_feat_conf_workspace", (B, fs.shape[0], ft.shape[0]), dev, torch.float32, per=4)
    conf = torch.empty(B, smax, tmax, device=dev)
    N.check(N.lib().ndp_feat_conf(_p(fs), _p(ft), _p(os_), _p(ot), hs, ht, B, C, float(temperature), _p(ws), _p(conf), smax, tmax,
                                  N.stream_ptr(dev)), "ndp_feat_conf")
    return conf


def _attention_args(q, k, v, n_head, pe_q, pe_k, scale, offsets_q, offsets_k, pos_q, pos_k, sigma_spat, more=()):
    """The checks that attention and attention_bwd share -> (q, k, v, pe_q, pe_k, pos_q, pos_k contiguous and checked, C, n_head, scale,
    sigma_spat, (device offsets, host copy) of either side).  more: (name, tensor, "C" or "H") triples of further tensors that must be
    [sum L, C] or [sum L, n_head], checked with the shapes, ahead of the device checks."""
    for t, name in ((q, "q"), (k, "k"), (v, "v")):
        if not isinstance(t, torch.Tensor) or t.ndim != 2:
            raise ValueError(f"{name} must be a tensor [rows, C], got {getattr(t, 'shape', type(t))}")
    C, n_head = q.shape[1], int(n_head)
    if k.shape[1] != C or v.shape[1] != C or k.shape[0] != v.shape[0]:
        raise ValueError(f"q [L,C], k [S,C] and v [S,C] must agree, got {tuple(q.shape)}, {tuple(k.shape)} and {tuple(v.shape)}")
    if n_head < 1 or C < 1 or C % n_head != 0:
        raise ValueError(f"C = {C} must be a positive multiple of n_head = {n_head}")
    D = C // n_head
    if (pe_q is None) != (pe_k is None):
        raise ValueError("pe_q and pe_k are passed as both or neither")
    if pe_q is not None:
        if D % 2 != 0:
            raise ValueError(f"a rotary code needs an even head dimension, got C / n_head = {D}")
        for t, ref, name in ((pe_q, q, "pe_q"), (pe_k, k, "pe_k")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (ref.shape[0], C, 2):
                raise ValueError(f"{name} must be [{ref.shape[0]}, {C}, 2], got {getattr(t, 'shape', type(t))}")
    scale = D ** -0.5 if scale is None else float(scale)
    if not math.isfinite(scale):
        raise ValueError(f"scale must be finite, got {scale}")
    compat = pos_q is not None or pos_k is not None or sigma_spat is not None
    if compat:
        if pos_q is None or pos_k is None or sigma_spat is None:
            raise ValueError("pos_q, pos_k and sigma_spat are passed all together or not at all")
        for t, ref, name in ((pos_q, q, "pos_q"), (pos_k, k, "pos_k")):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != (ref.shape[0], 6):
                raise ValueError(f"{name} must be [{ref.shape[0]}, 6] (source xyz, target xyz), got {getattr(t, 'shape', type(t))}")
        sigma_spat = float(sigma_spat)
        if not sigma_spat > 0:
            raise ValueError(f"sigma_spat must be positive (inf: no compatibility), got {sigma_spat}")
    for name, t, width in more:
        cols = C if width == "C" else n_head
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != (q.shape[0], cols):
            raise ValueError(f"{name} must be [{q.shape[0]}, {cols}], got {getattr(t, 'shape', type(t))}")
    q, k, v = (_chk(t.contiguous() if isinstance(t, torch.Tensor) and t.is_cuda else t, name) for t, name in ((q, "q"), (k, "k"), (v, "v")))
    if pe_q is not None:
        pe_q, pe_k = _chk(pe_q.contiguous() if pe_q.is_cuda else pe_q, "pe_q"), _chk(pe_k.contiguous() if pe_k.is_cuda else pe_k, "pe_k")
    dev = q.device
    oq, hq = _host_offsets(q.shape[0], offsets_q, "offsets_q", dev)
    ok, hk = _host_offsets(k.shape[0], offsets_k, "offsets_k", dev)
    if len(hq) != len(hk):
        raise ValueError(f"both sides must list the same problems, got {len(hq) - 1} and {len(hk) - 1}")
    if compat:
        pos_q, pos_k = _chk(pos_q.contiguous() if pos_q.is_cuda else pos_q, "pos_q"), _chk(pos_k.contiguous() if pos_k.is_cuda else pos_k, "pos_k")
    return q, k, v, pe_q, pe_k, pos_q, pos_k, C, n_head, scale, sigma_spat, (oq, hq), (ok, hk)


def attention(q, k, v, n_head, pe_q=None, pe_k=None, scale=None, offsets_q=None, offsets_k=None, pos_q=None, pos_k=None, sigma_spat=None,
              want_lse=False):
    """Multi-head soft-max attention of stacked, unpadded problems (csrc/ndp_attention.inc: one fused launch, scores and P V on the
    f32-input MFMA, the L x S x H scores are never stored) -> o [sum L, C].  q [sum L,C], k, v [sum S,C] already projected (made
    contiguous if they are not); head h owns the channels h D .. h D + D - 1, D = C / n_head.  pe_q [sum L,C,2], pe_k [sum S,C,2]:
    the (cos, sin) of a rotary code per channel (lepard.VolumetricPositionEncoding), both or neither; q and k are rotated while they
    are staged, v is not.  scale defaults to D ** -0.5.  offsets_*: B + 1 ascending row offsets for B problems in one call.
    pos_q [sum L,6], pos_k [sum S,6] float32 and sigma_spat, all three or none: every score is multiplied by the spatial compatibility
    max(0, 1 - (|s_i - s_j| - |t_i - t_j|)^2 / sigma_spat^2) of the rows' (s_xyz, t_xyz) before the scale and the soft-max
    (ndp_attention_compat_forward, outlier.CorrespondenceAttentionLayer); sigma_spat = inf is the plain call's bits.
    want_lse: -> (o, lse [sum L, n_head]), the same o and the log-sum-exp of every row's scaled scores (ndp_attention_forward_lse),
    which attention_bwd takes.  This call itself records nothing for autograd: attention_fn is the differentiable form.  Does not
    synchronise."""
    q, k, v, pe_q, pe_k, pos_q, pos_k, C, n_head, scale, sigma_spat, (oq, hq), (ok, hk) = _attention_args(
        q, k, v, n_head, pe_q, pe_k, scale, offsets_q, offsets_k, pos_q, pos_k, sigma_spat)
    dev = q.device
    out = torch.empty_like(q)
    if want_lse:
        lse = torch.empty(q.shape[0], n_head, device=dev)
        N.check(N.lib().ndp_attention_forward_lse(_p(q), _p(k), _p(v), _p(pe_q), _p(pe_k), _p(pos_q), _p(pos_k), _p(oq), _p(ok), hq, hk,
                                                  len(hq) - 1, C, n_head, scale, sigma_spat if pos_q is not None else math.inf, _p(out),
                                                  _p(lse), N.stream_ptr(dev)), "ndp_attention_forward_lse")
        return out, lse
    if pos_q is not None:
        N.check(N.lib().ndp_attention_compat_forward(_p(q), _p(k), _p(v), _p(pe_q), _p(pe_k), _p(pos_q), _p(pos_k), _p(oq), _p(ok), hq, hk,
                                                     len(hq) - 1, C, n_head, scale, sigma_spat, _p(out), N.stream_ptr(dev)),
                "ndp_attention_compat_forward")
        return out
    N.check(N.lib().ndp_attention_forward(_p(q), _p(k), _p(v), _p(pe_q), _p(pe_k), _p(oq), _p(ok), hq, hk, len(hq) - 1, C, n_head, scale,
                                          _p(out), N.stream_ptr(dev)), "ndp_attention_forward")
    return out


def attention_bwd(q, k, v, o, lse, do, n_head, pe_q=None, pe_k=None, scale=None, offsets_q=None, offsets_k=None, pos_q=None, pos_k=None,
                  sigma_spat=None):
    """The gradient of attention's o in the unrotated q, k and v -> (dq [sum L,C], dk [sum S,C], dv [sum S,C]), given do [sum L,C] and
    the (o, lse) that attention(..., want_lse=True) returned for the same arguments (ndp_attention_backward: two launches that
    recompute the scores -- no L x S array exists -- fp32 on the f32-input MFMA, no atomics, the same bits run to run).  pe_* and
    pos_* are data: they get no gradient and the compatibility is not differentiated.  Takes attention's checks; q, k, v, o, lse
    and do are made contiguous if they are not.  Does not synchronise."""
    q, k, v, pe_q, pe_k, pos_q, pos_k, C, n_head, scale, sigma_spat, (oq, hq), (ok, hk) = _attention_args(
        q, k, v, n_head, pe_q, pe_k, scale, offsets_q, offsets_k, pos_q, pos_k, sigma_spat,
        more=(("o", o, "C"), ("do", do, "C"), ("lse", lse, "H")))
    o, lse, do = (_chk(t.contiguous() if t.is_cuda else t, name) for t, name in ((o, "o"), (lse, "lse"), (do, "do")))
    dev = q.device
    dq, dk, dv = torch.empty_like(q), torch.empty_like(k), torch.empty_like(v)
    delta = torch.empty(q.shape[0], n_head, device=dev)          # sum_d o do per (row, head): the dq sweep writes it, the dk / dv sweep reads it
    N.check(N.lib().ndp_attention_backward(_p(q), _p(k), _p(v), _p(pe_q), _p(pe_k), _p(pos_q), _p(pos_k), _p(o), _p(lse), _p(do), _p(oq),
                                           _p(ok), hq, hk, len(hq) - 1, C, n_head, scale, sigma_spat if pos_q is not None else math.inf,
                                           _p(delta), _p(dq), _p(dk), _p(dv), N.stream_ptr(dev)), "ndp_attention_backward")
    return dq, dk, dv


RADIUS_MAX_K = 64


def _stack_lengths(lengths, n, name):
    """lengths (tensor, array or list, every entry >= 1, summing to n) -> ctypes int array for the C entries."""
    ls = [int(v) for v in (lengths.tolist() if hasattr(lengths, "tolist") else lengths)]
    if not ls or min(ls) < 1:
        raise ValueError(f"{name}: every cloud needs at least one point, got lengths {ls[:8]}{'...' if len(ls) > 8 else ''}")
    if sum(ls) != n:
        raise ValueError(f"{name} must sum to the number of stacked points ({n}), got {sum(ls)}")
    if len(ls) > 65535:
        raise ValueError(f"{name}: at most 65535 clouds in a batch, got {len(ls)}")
    return (ctypes.c_int * len(ls))(*ls)


def _stacked(t, name):
    if not isinstance(t, torch.Tensor) or t.ndim != 2 or t.shape[1] != 3 or t.shape[0] < 1:
        raise ValueError(f"{name} must be a [N, 3] tensor with N >= 1, got {getattr(t, 'shape', type(t))}")
    return t


def voxel_subsample(points, lengths, dl, features=None, max_p=0):
    """Voxel-grid barycentre subsampling of stacked clouds (csrc/ndp_kpconv.inc: k_voxel_keys, sort, k_voxel_reduce) ->
    (s_points [M,3], s_lengths [B] int32 on the host, s_features [M,F] or None, inverse [N] int32: the output row of every input
    point, -1 where max_p dropped its voxel).  Voxel membership is the reference's fp32 expression; a barycentre is a float64 sum in
    input order rounded once; output order per cloud is ascending (iz, iy, ix); max_p > 0 keeps the first max_p voxels per cloud.
    Class labels (the reference's majority vote) are not served.  Synchronises: the output size is data."""
    _stacked(points, "points")
    n, dl = points.shape[0], float(dl)
    hl = _stack_lengths(lengths, n, "lengths")
    if not (dl > 0 and math.isfinite(dl)):
        raise ValueError(f"dl must be positive and finite, got {dl}")
    F = 0
    if features is not None:
        if not isinstance(features, torch.Tensor) or features.ndim != 2 or features.shape[0] != n or features.shape[1] < 1:
            raise ValueError(f"features must be [N, F] with N = {n} and F >= 1, got {getattr(features, 'shape', type(features))}")
        F = features.shape[1]
    _chk(points, "points")
    if features is not None:
        _chk(features, "features")
    B, dev = len(hl), points.device
    ws = _workspace("ndp_voxel_subsample_workspace", (n, B), dev, torch.int32, per=4)
    out = torch.empty(n, 3, device=dev)
    out_f = torch.empty(n, F, device=dev) if F else None
    inverse = torch.empty(n, device=dev, dtype=torch.int32)
    out_len = (ctypes.c_int * B)()
    N.check(N.lib().ndp_voxel_subsample(_p(points), _p(features), F, hl, B, dl, int(max_p), _p(ws), 4 * ws.numel(), _p(out), _p(out_f), _p(inverse),
                                        out_len, N.stream_ptr(dev)), "ndp_voxel_subsample")
    m = sum(out_len)
    return out[:m], torch.tensor(list(out_len), dtype=torch.int32), (out_f[:m] if F else None), inverse


def radius_search(q, s, q_lengths, s_lengths, radius, max_neighbors, want_d2=False):
    """Fixed-radius neighbours of stacked queries among the supports of their own cloud (csrc/ndp_kpconv.inc: k_radius_grid, sort,
    k_radius_search) -> (idx [Nq,K] int32, counts [Nq] int32[, d2 [Nq,K]]).  A support is listed iff d2 < radius^2 (fp32, strict, the
    chain of ops.knn); a row holds the K = max_neighbors nearest in (d2, index) order, stacked-global indices, padded with the shadow
    index Ns (d2: +inf); counts is the number within the radius before the cut.  max_neighbors <= 0: all of them -- K is the largest
    count, which must not exceed 64 (see kpconv.radius_count for the counts alone).  max_neighbors = None: counts only, idx is None."""
    _stacked(q, "q"); _stacked(s, "s")
    nq, ns, radius = q.shape[0], s.shape[0], float(radius)
    hq, hs = _stack_lengths(q_lengths, nq, "q_lengths"), _stack_lengths(s_lengths, ns, "s_lengths")
    if len(hq) != len(hs):
        raise ValueError(f"queries and supports must list the same clouds, got {len(hq)} and {len(hs)}")
    if not (radius > 0 and math.isfinite(radius)):
        raise ValueError(f"radius must be positive and finite, got {radius}")
    if max_neighbors is not None and int(max_neighbors) > RADIUS_MAX_K:
        raise ValueError(f"max_neighbors must not exceed {RADIUS_MAX_K}, got {max_neighbors}")
    _chk(q, "q"); _chk(s, "s")
    B, dev = len(hq), q.device
    ws = _workspace("ndp_radius_search_workspace", (nq, ns, B), dev, torch.int32, per=4)
    counts = torch.empty(nq, device=dev, dtype=torch.int32)

    def run(K, idx, d2):
        N.check(N.lib().ndp_radius_search(_p(q), _p(s), hq, hs, B, radius, K, _p(ws), 4 * ws.numel(), _p(idx), _p(d2), _p(counts),
                                          N.stream_ptr(dev)), "ndp_radius_search")

    K = 0 if max_neighbors is None else int(max_neighbors)
    if K <= 0:
        run(0, None, None)
        if max_neighbors is None:
            return (None, counts, None) if want_d2 else (None, counts)
        K = int(counts.max().item())
        if K > RADIUS_MAX_K:
            raise N.NdpError(f"radius_search: max_neighbors <= 0 asks for every neighbour, and the fullest neighbourhood holds {K} > "
                             f"{RADIUS_MAX_K}: pass a limit, or read the sizes with kpconv.radius_count")
    idx = torch.empty(nq, K, device=dev, dtype=torch.int32)
    d2 = torch.empty(nq, K, device=dev) if want_d2 else None
    if K > 0:
        run(K, idx, d2)
    return (idx, counts, d2) if want_d2 else (idx, counts)


KPCONV_INFLUENCE = {"constant": 0, "linear": 1, "gaussian": 2}
KPCONV_AGGREGATION = {"sum": 0, "closest": 1}
KPCONV_MAX_K, KPCONV_MAX_C = 32, 1024


def _kpconv_args(q, s, idx, x, weights, kernel_points, extent, influence, aggregation, dy=None):
    """ops.kpconv's argument checks, shared with ops.kpconv_bwd (which passes dy, checked against [Nq, Cout] before the tensors are
    asked to be on the device) -> (idx int32 contiguous, x contiguous, extent, (nq, ns, H, K, cin, cout))."""
    _stacked(q, "q"); _stacked(s, "s")
    nq, ns, extent = q.shape[0], s.shape[0], float(extent)
    if not isinstance(idx, torch.Tensor) or idx.ndim != 2 or idx.shape[0] != nq or idx.shape[1] < 1 or idx.dtype not in (torch.int32, torch.int64):
        raise ValueError(f"idx must be an int32 or int64 tensor [Nq, H] with Nq = {nq} and H >= 1, got {getattr(idx, 'shape', type(idx))} "
                         f"{getattr(idx, 'dtype', '')}")
    if not isinstance(x, torch.Tensor) or x.ndim != 2 or x.shape[0] != ns or x.shape[1] < 1:
        raise ValueError(f"x must be [Ns, Cin] with Ns = {ns} and Cin >= 1, got {getattr(x, 'shape', type(x))}")
    cin = x.shape[1]
    if not isinstance(weights, torch.Tensor) or weights.ndim != 3 or weights.shape[1] != cin or weights.shape[0] < 1 or weights.shape[2] < 1:
        raise ValueError(f"weights must be [K, Cin, Cout] with Cin = {cin}, got {getattr(weights, 'shape', type(weights))}")
    K, cout, H = weights.shape[0], weights.shape[2], idx.shape[1]
    if not isinstance(kernel_points, torch.Tensor) or tuple(kernel_points.shape) != (K, 3):
        raise ValueError(f"kernel_points must be [K, 3] with K = {K}, got {getattr(kernel_points, 'shape', type(kernel_points))}")
    if influence not in KPCONV_INFLUENCE:
        raise ValueError(f"influence must be one of {sorted(KPCONV_INFLUENCE)}, got {influence!r}")
    if aggregation not in KPCONV_AGGREGATION:
        raise ValueError(f"aggregation must be one of {sorted(KPCONV_AGGREGATION)}, got {aggregation!r}")
    if not (extent > 0 and math.isfinite(extent)):
        raise ValueError(f"extent must be positive and finite, got {extent}")
    if H > RADIUS_MAX_K or K > KPCONV_MAX_K or cin > KPCONV_MAX_C or cout > KPCONV_MAX_C:
        raise ValueError(f"served are H <= {RADIUS_MAX_K}, K <= {KPCONV_MAX_K}, Cin, Cout <= {KPCONV_MAX_C}; got H = {H}, K = {K}, "
                         f"Cin = {cin}, Cout = {cout}")
    if dy is not None and (not isinstance(dy, torch.Tensor) or tuple(dy.shape) != (nq, cout)):
        raise ValueError(f"dy must be [Nq, Cout] = [{nq}, {cout}], got {getattr(dy, 'shape', type(dy))}")
    _chk(q, "q"); _chk(s, "s")
    if idx.dtype == torch.int64:                                   # the reference's tables; a value beyond int32 is a shadow either way
        idx = idx.clamp(-1, ns).to(torch.int32)
    idx, x = idx.contiguous(), x.contiguous()
    _chk(idx, "idx", torch.int32); _chk(x, "x"); _chk(weights.detach(), "weights"); _chk(kernel_points.detach(), "kernel_points")
    return idx, x, extent, (nq, ns, H, K, cin, cout)


def kpconv(q, s, idx, x, weights, kernel_points, extent, influence="linear", aggregation="sum", normalize=True):
    """Rigid KPConv forward (csrc/ndp_kpconv_conv.inc: k_kpc_forward, both products on the f32-input MFMA) -> y [Nq, Cout].
    q [Nq,3] queries, s [Ns,3] supports, idx [Nq,H] int32 or int64 stacked support rows (radius_search's; every value outside
    0 .. Ns-1 is a shadow and contributes nothing), x [Ns,Cin] features (made contiguous if they are not), weights [K,Cin,Cout],
    kernel_points [K,3].  y[n] = sum_k sum_c (sum_h w(n,h,k) x[idx[n,h],c]) W[k,c,:] with the kernel-point influence w of the
    squared distance between s[idx[n,h]] - q[n] and kernel_points[k]: "constant" 1, "linear" max(0, 1 - d / extent), "gaussian"
    exp(-d^2 / (2 (0.3 extent)^2 + 1e-9)); aggregation "closest" keeps, per neighbour, only its nearest kernel point; normalize
    divides by max(1, number of neighbours whose feature row sums to a positive number), the reference's term.  K <= 32, H <= 64,
    Cin, Cout <= 1024.  The result carries no grad_fn: kpconv_fn is the differentiable form and kpconv_bwd the gradient itself.
    Does not synchronise."""
    idx, x, extent, dims = _kpconv_args(q, s, idx, x, weights, kernel_points, extent, influence, aggregation)
    nq, ns, H, K, cin, cout = dims
    dev = q.device
    ws = _workspace("ndp_kpconv_forward_workspace", dims, dev, torch.int32, per=4)
    y = torch.empty(nq, cout, device=dev)
    N.check(N.lib().ndp_kpconv_forward(_p(q), _p(s), _p(idx), _p(x), _p(weights), _p(kernel_points), nq, ns, H, K, cin, cout, extent,
                                       KPCONV_INFLUENCE[influence], KPCONV_AGGREGATION[aggregation], int(bool(normalize)), _p(ws),
                                       4 * ws.numel(), _p(y), N.stream_ptr(dev)), "ndp_kpconv_forward")
    return y


def kpconv_bwd(q, s, idx, x, weights, kernel_points, extent, dy, influence="linear", aggregation="sum", normalize=True, need_dx=True,
               need_dw=True, slab_queries=0):
    """The gradient of sum(kpconv(...) * dy) in x and in weights -> (dx [Ns,Cin] or None, dW [K,Cin,Cout] or None), given dy [Nq,Cout]
    (csrc/ndp_kpconv_bwd.inc: fp32 on the f32-input MFMA, no atomics, every sum in one fixed order, the same bits run to run; the
    influences are recomputed from the points, nothing of the forward is kept).  The normalisation count and the `closest` choice are
    constants; the points and kernel_points get no gradient.  dx[r] is one chain over the incoming edges of r in ascending (n, h);
    the per-edge gradients pass through memory in slabs of slab_queries queries (0: as many as 64 MiB hold; else a multiple of 16),
    and the bits of dx do not depend on that.  need_dx / need_dw = False skips that gradient and its launches.  Takes kpconv's
    checks; dy is made contiguous if it is not.  Does not synchronise."""
    if not (need_dx or need_dw):
        raise ValueError("need_dx and need_dw are both False: nothing to compute")
    slab_queries = int(slab_queries)
    if slab_queries < 0 or slab_queries % 16:
        raise ValueError(f"slab_queries must be 0 or a positive multiple of 16, got {slab_queries}")
    if dy is None:
        raise ValueError("dy must be [Nq, Cout], got None")
    idx, x, extent, dims = _kpconv_args(q, s, idx, x, weights, kernel_points, extent, influence, aggregation, dy)
    nq, ns, H, K, cin, cout = dims
    dy = _chk(dy.contiguous() if dy.is_cuda else dy, "dy")
    dev = q.device
    ws = _workspace("ndp_kpconv_backward_workspace", dims + (slab_queries,), dev, torch.int32, per=4)
    dx = torch.empty(ns, cin, device=dev) if need_dx else None
    dw = torch.empty(K, cin, cout, device=dev) if need_dw else None
    N.check(N.lib().ndp_kpconv_backward(_p(q), _p(s), _p(idx), _p(x), _p(weights.detach()), _p(kernel_points.detach()), _p(dy), nq, ns, H, K,
                                        cin, cout, extent, KPCONV_INFLUENCE[influence], KPCONV_AGGREGATION[aggregation],
                                        int(bool(normalize)), slab_queries, _p(ws), 4 * ws.numel(), _p(dx), _p(dw), N.stream_ptr(dev)),
            "ndp_kpconv_backward")
    return dx, dw


def landmark_mse(x, t):
    _chk(x, "x"); _chk(t, "t")
    loss = torch.empty(1, device=x.device)
    gx = torch.empty_like(x)
    N.check(N.lib().ndp_landmark_mse_fwd_bwd(_p(x), _p(t), x.shape[0], _p(loss), _p(gx), N.stream_ptr(x.device)),
            "ndp_landmark_mse_fwd_bwd")
    return loss, gx


def adam_scalars(t, lr=0.01, b1=0.9, b2=0.999):
    """(neg_step, bc2_sqrt) of torch.optim.Adam's single-tensor path, computed in Python doubles."""
    bc1 = 1 - b1 ** t
    bc2 = 1 - b2 ** t
    return -(lr / bc1), math.sqrt(bc2)


def adam_step(p, g, m, v, t, lr=0.01, b1=0.9, b2=0.999, eps=1e-8):
    for a, nm in ((p, "p"), (g, "g"), (m, "m"), (v, "v")):
        _chk(a, nm)
    ns, bc2s = adam_scalars(t, lr, b1, b2)
    N.check(N.lib().ndp_adam_step(_p(p), _p(g), _p(m), _p(v), p.numel(), 1 - b1, b2, 1 - b2, ns, bc2s, eps,
                                  N.stream_ptr(p.device)), "ndp_adam_step")


# ------------------------------------------------------------------------------ autograd wrappers
class _LevelWarpFn(torch.autograd.Function):
    """NDPLayer.forward (nets.py:111-140) for callers that own their optimisation loop
    (shape_transfer.py:116-157).  Differentiable in the level's parameters AND in x, like the reference's autograd code: levels
    chained by Deformation_Pyramid.warp pass the gradient down, and points can be optimised through a frozen pyramid.  When x does
    not require a gradient the launches are those of a detached x (the reference's hot path).  First derivatives only.
    Returns (x', nonrigidity) -- the gate tensor is empty for levels without the nonrigidity head."""

    @staticmethod
    def forward(ctx, x, layer, *params):
        need_p = any(p.requires_grad for p in params)
        need = need_p or x.requires_grad
        flat = layer.flat.detach()
        xd = x.detach().contiguous()
        gate = layer.desc.nonrigidity
        if need:
            res = level_fwd(layer.desc, flat, layer.level, layer.k0, xd, save=True, want_nonrig=True)
            out, act, heads, nr = res
            ctx.save_for_backward(xd, act, heads)
            ctx.layer = layer
            ctx.need_p = need_p
        else:
            out, nr = level_fwd(layer.desc, flat, layer.level, layer.k0, xd, want_nonrig=True)
        if not gate:
            nr = torch.empty(0, device=x.device)
            ctx.mark_non_differentiable(nr)
        return out, nr

    @staticmethod
    @once_differentiable
    def backward(ctx, g, g_nr):
        x, act, heads = ctx.saved_tensors
        layer = ctx.layer
        gnr = g_nr.contiguous() if (layer.desc.nonrigidity and g_nr is not None) else None
        want_dx = ctx.needs_input_grad[0]
        res = level_bwd(layer.desc, layer.flat.detach(), layer.level, layer.k0, x, act, heads, g.contiguous(), g_nr=gnr, want_dx=want_dx)
        grads, dx = res if want_dx else (res, None)
        outs = []
        for name, off, shape in layer.desc.named_slices():
            if not ctx.need_p:
                outs.append(None)
                continue
            n = 1
            for s in shape:
                n *= s
            outs.append(grads[off:off + n].view(shape))
        return (dx, None) + tuple(outs)


def level_warp(layer, x):
    """-> (x', nonrigidity | None).  Squeeze semantics of nets.py:140 are not reproduced (n >= 2)."""
    if x.dim() != 2 or x.shape[-1] != 3:
        raise ValueError("expected points of shape [n, 3]")
    params = tuple(layer.parameters())
    out, nr = _LevelWarpFn.apply(x.float(), layer, *params)
    return out, (nr if layer.desc.nonrigidity else None)


def _save_pair_grads(ctx, gx, gy, dev):
    """What the two pair losses keep for their backward: dloss/dx and dloss/dy as the forward's kernels left them (empty: not asked for)."""
    none = torch.empty(0, device=dev)
    ctx.save_for_backward(gx if gx is not None else none, gy if gy is not None else none)


def _pair_grads(ctx, g, n_inputs):
    """... and their backward: the saved gradients scaled by g for x and y, None for the other inputs."""
    gx, gy = ctx.saved_tensors
    return ((gx * g if gx.numel() else None), (gy * g if gy.numel() else None)) + (None,) * (n_inputs - 2)


class _ChamferFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, trunc, point_sum=False):
        xd, yd = x.detach().contiguous(), y.detach().contiguous()
        res = chamfer_l1(xd, yd, trunc, want_grad=x.requires_grad, point_sum=point_sum, want_grad_y=y.requires_grad)
        _save_pair_grads(ctx, res[1], res[3] if y.requires_grad else None, x.device)
        return res[0][0]

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return _pair_grads(ctx, g, 4)


def chamfer_distance(x, y, trunc, point_sum=False):
    """Differentiable (in x and in y, first derivatives) truncated L1 Chamfer of two [n,3] clouds."""
    return _ChamferFn.apply(x, y, float(trunc), bool(point_sum))


class _PointToPlaneFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, nx, ny, trunc, mode):
        xd, yd = x.detach().contiguous(), y.detach().contiguous()
        res = point_to_plane(xd, yd, nx.detach().contiguous(), ny.detach().contiguous(), trunc, mode,
                             want_grad=x.requires_grad, want_grad_y=y.requires_grad)
        out = res[0]
        _save_pair_grads(ctx, res[1], res[3] if y.requires_grad else None, x.device)
        parts = out[1:].clone()
        ctx.mark_non_differentiable(parts, res[2][1])
        return out[0], parts, res[2][1]

    @staticmethod
    @once_differentiable
    def backward(ctx, g, g_parts, g_idx):
        return _pair_grads(ctx, g, 6)


def point_to_plane_distance(x, y, nx, ny, trunc=math.inf, mode=0):
    """-> (total, parts [3] = (x part, y part, normal consistency), idx_x [S] int32).  `total` is differentiable (first derivatives)
    in x and in y; the normals and the nearest-neighbour indices are constants; `parts` are values only."""
    return _PointToPlaneFn.apply(x, y, nx, ny, float(trunc), int(mode))


class _AttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, n_head, pe_q, pe_k, scale, offsets_q, offsets_k, pos_q, pos_k, sigma_spat):
        det = lambda t: None if t is None else t.detach()
        qd, kd, vd = q.detach().contiguous(), k.detach().contiguous(), v.detach().contiguous()
        ctx.args = dict(n_head=n_head, pe_q=det(pe_q), pe_k=det(pe_k), scale=scale, offsets_q=offsets_q, offsets_k=offsets_k,
                        pos_q=det(pos_q), pos_k=det(pos_k), sigma_spat=sigma_spat)
        o, lse = attention(qd, kd, vd, want_lse=True, **ctx.args)
        ctx.save_for_backward(qd, kd, vd, o, lse)
        return o

    @staticmethod
    @once_differentiable
    def backward(ctx, do):
        q, k, v, o, lse = ctx.saved_tensors
        return attention_bwd(q, k, v, o, lse, do.contiguous(), **ctx.args) + (None,) * 9


def attention_fn(q, k, v, n_head, pe_q=None, pe_k=None, scale=None, offsets_q=None, offsets_k=None, pos_q=None, pos_k=None, sigma_spat=None):
    """attention, differentiable (first derivatives) in q, k and v: the forward keeps (q, k, v, o, lse) and the backward is one
    attention_bwd call.  The codes, the positions and everything else are constants."""
    return _AttentionFn.apply(q, k, v, n_head, pe_q, pe_k, scale, offsets_q, offsets_k, pos_q, pos_k, sigma_spat)


class _KPConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, s, idx, x, weights, kernel_points, extent, influence, aggregation, normalize):
        xd, wd = x.detach().contiguous(), weights.detach()
        ctx.args = dict(influence=influence, aggregation=aggregation, normalize=normalize)
        ctx.extent = extent
        ctx.save_for_backward(q.detach(), s.detach(), idx, xd, wd, kernel_points.detach())
        return kpconv(q.detach(), s.detach(), idx, xd, wd, kernel_points.detach(), extent, **ctx.args)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        q, s, idx, x, w, kp = ctx.saved_tensors
        need_dx, need_dw = ctx.needs_input_grad[3], ctx.needs_input_grad[4]
        dx = dw = None
        if need_dx or need_dw:
            dx, dw = kpconv_bwd(q, s, idx, x, w, kp, ctx.extent, dy.contiguous(), need_dx=need_dx, need_dw=need_dw, **ctx.args)
        return None, None, None, dx, dw, None, None, None, None, None


def kpconv_fn(q, s, idx, x, weights, kernel_points, extent, influence="linear", aggregation="sum", normalize=True):
    """kpconv, differentiable (first derivatives) in x and in weights: the forward is kpconv's, bit for bit, and keeps only its inputs;
    the backward is one kpconv_bwd call for what needs_input_grad asks.  The points, the table and kernel_points are constants."""
    return _KPConvFn.apply(q, s, idx, x, weights, kernel_points, float(extent), influence, aggregation, bool(normalize))


def flow_metrics(flow, flow_gt, overlap=None):
    """Device-side sums behind compute_flow_metrics -> [3,5] float64 on the host: per subset {all, overlap, ~overlap}
    {sum err, #AccS, #AccR, #outlier, #points}."""
    _chk(flow, "flow"); _chk(flow_gt, "flow_gt")
    n = flow.shape[0]
    ov = None
    if overlap is not None:
        ov = overlap.to(device=flow.device, dtype=torch.uint8).contiguous()
    out = torch.empty(15, device=flow.device, dtype=torch.float64)
    N.check(N.lib().ndp_flow_metrics(_p(flow), _p(flow_gt), _p(ov), n, _p(out), N.stream_ptr(flow.device)), "ndp_flow_metrics")
    return out.cpu().view(3, 5)
