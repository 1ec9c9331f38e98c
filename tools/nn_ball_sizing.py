"""Sizing of an exact grid ball search for the nearest-neighbour stage (CPU only, no GPU involved).
Runs the torch port of the oracle's optimisation (oracle/ndp_torch_ref.optimize, NDP.yaml unchanged) on two pairs and, at every
loss evaluation and for both directions, takes each query's exact distance to LAST evaluation's neighbour as the radius of a
ball and counts the reference points inside the ball and inside the uniform cells that the ball's bounding box touches, as a
fraction of all S x T (query, reference) combinations.
    python tools/nn_ball_sizing.py [A | surface] [cell size]        (A: synthetic_pair, cell 0.0625; surface: surface_pair, try 0.05)
The committed output is profiles/nn_ball_sizing.txt.
    python tools/nn_ball_sizing.py [C | D] [G ...]                  (C: synthetic_pair, samples 8192; D: surface_pair, Sim3/euler, samples 6000)
counts with the cell search's REAL geometry instead of a fixed cell size -- a G^3 grid over the targets' bounding box and the kernel's own
float32 cell expression (nnc_cell1 of csrc/ndp_nn_cells.inc), warped sources clamped into border cells -- at every evaluation of levels 0, 4
and 8 of the oracle's own optimisation loop (level forward / backward, Chamfer, Adam of oracle/ndp_oracle.py, bench.py's clouds and sampling).
The committed output is profiles/nn_ball_sizing_wide.txt.
    python tools/nn_ball_sizing.py steps [x | y | z] [GXxGYxGZ ...] [by_cell]
replays config A's trajectories (the oracle's loop, NDP.yaml's 2000 samples, every evaluation and both directions) through the wave-step
model of tools/nn_wave_steps.py: the kernel's lane mapping (query t + 1024 u, 64 lanes per wave), per wave and tick the modelled steps
(sum over row iterations of the busiest lane's records, plus the longest lane's rows) and the ideal (rows + records over lanes), for grids of
Gx x Gy x Gz <= 4096 cells whose row axis runs along the given geometric axis; by_cell deals the queries to the lanes in the order of their
own cells.  The committed output is profiles/nn_wave_steps.txt."""
import sys, os, torch, numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wide(kind, grids, levels=(0, 4, 8), n_pairs=2, nthreads=16):
    import ctypes
    from oracle import ndp_oracle as O
    from deformationpyramid_amd.synthetic import synthetic_pair, surface_pair
    from deformationpyramid_amd.config import Config, load_config
    from deformationpyramid_amd.nets import Deformation_Pyramid
    f32 = np.float32
    cfg = load_config(os.path.join(ROOT, "config", "NDP.yaml"), device=0)
    if kind == "C":
        cfg.samples = 8192
        make_pair = lambda i: synthetic_pair(i)
    else:
        cfg = Config(cfg, motion_type="Sim3", rotation_format="euler", samples=6000)
        make_pair = lambda i: surface_pair(i, n_total=2 * 24856, partial=False)

    def geometry(y, G):                      # nnc_build_global: origin = the box's minimum, inv_h = G / extent (0 where that is not finite)
        lo, hi = y.min(0), y.max(0)
        ext = (hi - lo).astype(f32)
        with np.errstate(divide="ignore", invalid="ignore"):
            ih = np.where(ext > 0, f32(G) / ext, f32(0)).astype(f32)
        ih[~np.isfinite(ih)] = 0
        return lo.astype(f32), ih

    def cell1(p, o, ih, G):                  # nnc_cell1, float32 throughout
        return np.minimum(np.maximum(np.floor(((p - o).astype(f32) * ih).astype(f32)), f32(0)), f32(G - 1)).astype(np.int64)

    def touched(q, ref, seed, o, ih, G):
        """per query: references in the cells that the ball around q (radius: chain distance to ref[seed], with the kernel's margins) touches"""
        d = (q - ref[seed]).astype(f32)
        b2 = ((d[:, 2] * d[:, 2]).astype(f32) + ((d[:, 1] * d[:, 1]).astype(f32) + (d[:, 0] * d[:, 0]).astype(f32)).astype(f32)).astype(f32)
        rs = (np.sqrt(b2).astype(f32) * f32(1 + 2.0 ** -10) + f32(1e-18)).astype(f32)
        r = (rs[:, None] + np.abs(q) * f32(2.0 ** -20)).astype(f32)
        lo, hi = cell1((q - r).astype(f32), o, ih, G), cell1((q + r).astype(f32), o, ih, G)
        c = cell1(ref, o, ih, G)
        cnt = np.zeros((G + 1, G + 1, G + 1), np.int64)
        np.add.at(cnt, (c[:, 2] + 1, c[:, 1] + 1, c[:, 0] + 1), 1)
        P = cnt.cumsum(0).cumsum(1).cumsum(2)                               # integral image: box sums by inclusion / exclusion
        z0, y0, x0, z1, y1, x1 = lo[:, 2], lo[:, 1], lo[:, 0], hi[:, 2] + 1, hi[:, 1] + 1, hi[:, 0] + 1
        return (P[z1, y1, x1] - P[z0, y1, x1] - P[z1, y0, x1] - P[z1, y1, x0] + P[z0, y0, x1] + P[z0, y1, x0] + P[z1, y0, x0] - P[z0, y0, x0])

    for k in range(n_pairs):
        src, tgt, _, _ = make_pair(k)
        torch.manual_seed(k)
        pyr = Deformation_Pyramid(depth=cfg.depth, width=cfg.width, device="cpu", k0=cfg.k0, m=cfg.m, rotation_format=cfg.rotation_format, motion=cfg.motion_type)
        sc = src - src.mean(0, keepdim=True); tc = tgt - tgt.mean(0, keepdim=True)
        x = sc[torch.randperm(sc.shape[0])[:cfg.samples]].contiguous().numpy()
        y = tc[torch.randperm(tc.shape[0])[:cfg.samples]].contiguous().numpy()
        S, T = x.shape[0], y.shape[0]
        geo = {G: geometry(y, G) for G in grids}
        stats = {(G, lv): [] for G in grids for lv in levels}
        prev, ticks = None, 0
        for level in range(cfg.m):
            d = pyr.descs[level]
            cd = O.make_desc(d.width, d.n_hidden, d.motion, d.rotfmt, d.nonrigidity, d.mlp_scale)
            p = pyr.store[level, :d.param_count].numpy().copy()
            am, av = np.zeros_like(p), np.zeros_like(p)
            bc, lp = ctypes.c_int(0), ctypes.c_double(1e6)
            warped = x
            for it in range(cfg.iters):
                warped = O.level_fwd(cd, p, level, cfg.k0, x, nthreads=nthreads)
                r = O.chamfer(warped, y, want_grad=True, nthreads=nthreads)
                ticks += 1
                if prev is not None and level in levels:
                    for G in grids:
                        o, ih = geo[G]
                        rows = touched(warped, y, prev[0], o, ih, G) / T
                        cols = touched(y, warped, prev[1], o, ih, G) / S
                        stats[G, level].append((rows.mean(), np.quantile(rows, 0.99), rows.max(), cols.mean(), np.quantile(cols, 0.99), cols.max(),
                                                (prev[0] == r["idx_x"]).mean(), (prev[1] == r["idx_y"]).mean()))
                prev = (r["idx_x"].astype(np.int64), r["idx_y"].astype(np.int64))
                if O.lib().ndp_o_stop_check(ctypes.c_double(float(r["loss"])), ctypes.byref(bc), ctypes.byref(lp), int(cfg.max_break_count),
                                            ctypes.c_double(cfg.break_threshold_ratio)):
                    break
                g = O.level_bwd(cd, p, level, cfg.k0, x, r["gx"], nthreads=nthreads)
                O.adam(p, g, am, av, it + 1, lr=cfg.lr)
            x = warped
        print(f"{kind} pair {k}: S {S} T {T}, {ticks} evaluations, last loss {float(r['loss']):.5f}")
        for G in grids:
            allv = []
            for lv in levels:
                a = np.array(stats[G, lv])
                if not len(a):
                    continue
                allv.append(a)
                print(f" G {G:2d} level {lv} ({len(a):3d} evaluations): rows mean {a[:,0].mean():.5f} p99 {a[:,1].mean():.4f} worst {a[:,2].max():.3f} | "
                      f"cols mean {a[:,3].mean():.5f} p99 {a[:,4].mean():.4f} worst {a[:,5].max():.3f} | same idx {a[:,6].mean():.3f} / {a[:,7].mean():.3f}")
            a = np.concatenate(allv)
            print(f" G {G:2d} levels {levels} together: rows mean {a[:,0].mean():.5f} | cols mean {a[:,3].mean():.5f} | both directions {(a[:,0].mean() + a[:,3].mean()) / 2:.5f} of S*T")


def steps(fine, shapes, n_pairs=2, nthreads=8, by_cell=False):
    """The wave-step model of tools/nn_wave_steps.py over config A's own trajectories (the oracle's loop, every evaluation that has a previous
    one, both directions).  fine: the geometric axis (0, 1, 2) that the grid's row axis runs along; shapes: (Gx, Gy, Gz) with Gx on that axis."""
    import ctypes
    import nn_wave_steps as W
    from oracle import ndp_oracle as O
    from deformationpyramid_amd.synthetic import synthetic_pair
    from deformationpyramid_amd.config import load_config
    from deformationpyramid_amd.nets import Deformation_Pyramid
    cfg = load_config(os.path.join(ROOT, "config", "NDP.yaml"), device=0)
    perm = [fine] + [a for a in range(3) if a != fine]         # the fine axis becomes the model's x
    acc = {s: [] for s in shapes}                              # per tick and direction: (sum of steps, sum of row parts, sum of ideals, max steps, waves, rows, records, queries)
    for k in range(n_pairs):
        src, tgt, _, _ = synthetic_pair(k)
        torch.manual_seed(k)
        pyr = Deformation_Pyramid(depth=cfg.depth, width=cfg.width, device="cpu", k0=cfg.k0, m=cfg.m, rotation_format=cfg.rotation_format, motion=cfg.motion_type)
        sc = src - src.mean(0, keepdim=True); tc = tgt - tgt.mean(0, keepdim=True)
        x = sc[torch.randperm(sc.shape[0])[:cfg.samples]].contiguous().numpy()
        y = tc[torch.randperm(tc.shape[0])[:cfg.samples]].contiguous().numpy()
        yp = np.ascontiguousarray(y[:, perm])
        geo = {s: W.geometry(yp, s) for s in shapes}
        prev, ticks = None, 0
        for level in range(cfg.m):
            d = pyr.descs[level]
            cd = O.make_desc(d.width, d.n_hidden, d.motion, d.rotfmt, d.nonrigidity, d.mlp_scale)
            p = pyr.store[level, :d.param_count].numpy().copy()
            am, av = np.zeros_like(p), np.zeros_like(p)
            bc, lp = ctypes.c_int(0), ctypes.c_double(1e6)
            warped = x
            for it in range(cfg.iters):
                warped = O.level_fwd(cd, p, level, cfg.k0, x, nthreads=nthreads)
                r = O.chamfer(warped, y, want_grad=True, nthreads=nthreads)
                ticks += 1
                if prev is not None:
                    wp = np.ascontiguousarray(warped[:, perm])
                    for s in shapes:
                        o, ih = geo[s]
                        for q, ref, seed in ((wp, yp, prev[0]), (yp, wp, prev[1])):
                            st, rows, ideal, nr, nc = W.direction(q, ref, seed, o, ih, s, by_cell)
                            acc[s].append((st.sum(), rows.sum(), ideal.sum(), st.max(), len(st), nr, nc, q.shape[0]))
                prev = (r["idx_x"].astype(np.int64), r["idx_y"].astype(np.int64))
                if O.lib().ndp_o_stop_check(ctypes.c_double(float(r["loss"])), ctypes.byref(bc), ctypes.byref(lp), int(cfg.max_break_count),
                                            ctypes.c_double(cfg.break_threshold_ratio)):
                    break
                g = O.level_bwd(cd, p, level, cfg.k0, x, r["gx"], nthreads=nthreads)
                O.adam(p, g, am, av, it + 1, lr=cfg.lr)
            x = warped
        print(f"A pair {k}: S {x.shape[0]} T {y.shape[0]}, {ticks} evaluations, last loss {float(r['loss']):.5f}")
    print(f"fine axis {'xyz'[fine]}{', queries dealt to the lanes in the order of their cells' if by_cell else ''}; per wave (64 lanes, one of a thread's two queries) and tick, mean over both directions of {n_pairs} pairs:")
    print("   Gx  Gy  Gz | steps = rows + records | ideal | worst wave || per query: rows  records")
    for s in shapes:
        a = np.array(acc[s], np.float64)
        w = a[:, 4].sum()
        print(f"  {s[0]:3d} {s[1]:3d} {s[2]:3d} | {a[:,0].sum() / w:6.1f} = {a[:,1].sum() / w:5.1f} + {(a[:,0].sum() - a[:,1].sum()) / w:5.1f} | {a[:,2].sum() / w:5.1f} | "
              f"{a[:,3].mean():6.1f}     ||   {a[:,5].sum() / a[:,7].sum():6.2f} {a[:,6].sum() / a[:,7].sum():7.2f}")


if len(sys.argv) > 1 and sys.argv[1] == "steps":
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    by_cell = "by_cell" in sys.argv
    args = [a for a in sys.argv[2:] if a != "by_cell"]
    fine = "xyz".index(args[0]) if args else 0
    grids = [tuple(int(v) for v in a.split("x")) for a in args[1:]] or \
            [(16, 16, 16), (32, 16, 8), (32, 8, 16), (64, 8, 8), (64, 16, 4), (64, 4, 16), (128, 8, 4), (128, 4, 8), (256, 4, 4), (8, 16, 16), (16, 32, 8)]
    assert all(len(g) == 3 and g[0] * g[1] * g[2] <= 4096 for g in grids), "Gx x Gy x Gz <= 4096 (the cell_start table stays 16 KB)"
    steps(fine, grids, by_cell=by_cell)
    sys.exit(0)
if len(sys.argv) > 1 and sys.argv[1] in ("C", "D"):
    wide(sys.argv[1], [int(v) for v in sys.argv[2:]] or [16])
    sys.exit(0)
from oracle import ndp_torch_ref as T
from deformationpyramid_amd.synthetic import synthetic_pair, surface_pair
from deformationpyramid_amd.config import load_config
from deformationpyramid_amd.nets import Deformation_Pyramid
torch.set_num_threads(16)
cfg = load_config(os.path.join(ROOT, "config", "NDP.yaml"), device=0)
CELL = float(sys.argv[2]) if len(sys.argv) > 2 else 0.0625
stats = []
last = {}
def counts(a, b, key):
    d = ((a[:, None, :] - b[None, :, :]) ** 2).sum(-1)
    idx = d.argmin(1)
    prev = last.get(key)
    last[key] = idx
    if prev is None or prev.shape != idx.shape:
        return None
    r2 = d.gather(1, prev[:, None])[:, 0]            # exact distance to last tick's neighbour: an upper bound
    ball = (d <= r2[:, None]).sum(1).float()
    r = r2.sqrt()
    lo = torch.floor((a - r[:, None]) / CELL) * CELL
    hi = (torch.floor((a + r[:, None]) / CELL) + 1) * CELL
    inb = ((b[None] >= lo[:, None]) & (b[None] < hi[:, None])).all(-1).sum(1).float()
    same = (prev == idx).float().mean().item()
    return ball.mean().item() / b.shape[0], inb.mean().item() / b.shape[0], inb.max().item() / b.shape[0], same, torch.quantile(inb, 0.99).item() / b.shape[0]
orig = T.chamfer_l1
def patched(x, y, trunc=1e9):
    with torch.no_grad():
        r = counts(x.detach(), y, "x"); c = counts(y, x.detach(), "y")
        if r and c: stats.append(r + c)
    return orig(x, y, trunc)
T.chamfer_l1 = patched
kind = sys.argv[1] if len(sys.argv) > 1 else "A"
for k in range(2):
    src, tgt, _, _ = (synthetic_pair(k) if kind == "A" else surface_pair(k))
    torch.manual_seed(k)
    pyr = Deformation_Pyramid(depth=cfg.depth, width=cfg.width, device="cpu", k0=cfg.k0, m=cfg.m, rotation_format=cfg.rotation_format, motion=cfg.motion_type)
    d = pyr.descs[0]
    sc = src - src.mean(0, keepdim=True); tc = tgt - tgt.mean(0, keepdim=True)
    s = sc[torch.randperm(sc.shape[0])[:cfg.samples]].contiguous(); t = tc[torch.randperm(tc.shape[0])[:cfg.samples]].contiguous()
    last.clear(); n0 = len(stats)
    T.optimize(pyr.store[:, :d.param_count], s, t, m=cfg.m, k0=cfg.k0, iters=cfg.iters, lr=cfg.lr, max_break_count=cfg.max_break_count, ratio=cfg.break_threshold_ratio)
    a = np.array(stats[n0:])
    print(kind, "pair", k, "ticks", len(a), "cell", CELL)
    print(" rows (source->target): ball %.4f  cells %.4f  worst query %.3f  p99 %.3f  same idx %.3f" % (a[:,0].mean(), a[:,1].mean(), a[:,2].max(), a[:,4].mean(), a[:,3].mean()))
    print(" cols (target->source): ball %.4f  cells %.4f  worst query %.3f  p99 %.3f  same idx %.3f" % (a[:,5].mean(), a[:,6].mean(), a[:,7].max(), a[:,9].mean(), a[:,8].mean()))
    print(" first 3 ticks cells rows/cols:", a[:3,1], a[:3,6])
