"""Wave-step model of the cell search's walk (csrc/ndp_nn_cells.inc), CPU only.  Importable; tools/nn_ball_sizing.py steps drives it.

The search gives thread t of a 1024-thread workgroup the queries t + 1024 u (u = 0, 1), one after the other; 64 consecutive threads are
a wave.  A query walks the (y, z) ROWS of its box of cells -- y fastest -- and in every row the records of the cells lo_x .. hi_x, which
lie contiguously.  The lanes of a wave run in lock step, so a wave issues for one u
    steps = sum over row iterations r of  max over lanes (records of that lane's r-th row)   +   max over lanes (rows)
and the least any lane mapping could issue is the IDEAL (sum over lanes of rows + records) / lanes.
The grid has (Gx, Gy, Gz) cells per axis over the references' geometry (the targets' bounding box), cell(p) per axis is the kernel's own
float32 expression (nnc_cell1), the radius carries the kernel's margins."""
import numpy as np

f32 = np.float32
LANES, THREADS = 64, 1024


def geometry(y, dims):
    """nnc_build_global: origin = the box's minimum, inv_h = G_axis / extent (0 where that is not finite)"""
    lo, hi = y.min(0), y.max(0)
    ext = (hi - lo).astype(f32)
    g = np.asarray(dims, f32)
    with np.errstate(divide="ignore", invalid="ignore"):
        ih = np.where(ext > 0, g / ext, f32(0)).astype(f32)
    ih[~np.isfinite(ih)] = 0
    return lo.astype(f32), ih


def cell1(p, o, ih, dims):
    """nnc_cell1 per axis, float32 throughout; p [n][3]"""
    top = (np.asarray(dims) - 1).astype(f32)
    return np.minimum(np.maximum(np.floor(((p - o).astype(f32) * ih).astype(f32)), f32(0)), top).astype(np.int64)


def boxes(q, ref, seed, o, ih, dims):
    """per query the cells lo .. hi [nq][3] its ball around q touches (radius: chain distance to ref[seed] with the kernel's margins)"""
    d = (q - ref[seed]).astype(f32)
    b2 = ((d[:, 2] * d[:, 2]).astype(f32) + ((d[:, 1] * d[:, 1]).astype(f32) + (d[:, 0] * d[:, 0]).astype(f32)).astype(f32)).astype(f32)
    rs = (np.sqrt(b2).astype(f32) * f32(1 + 2.0 ** -10) + f32(1e-18)).astype(f32)
    r = (rs[:, None] + np.abs(q) * f32(2.0 ** -20)).astype(f32)
    return cell1((q - r).astype(f32), o, ih, dims), cell1((q + r).astype(f32), o, ih, dims)


def row_records(ref_cells, dims, lo, hi):
    """nrow [nq] and rec [nq][max nrow]: the records of each query's rows in the kernel's order (y fastest, then z), 0 behind its last row"""
    gx, gy, gz = dims
    cnt = np.zeros((gz, gy, gx + 1), np.int64)
    np.add.at(cnt, (ref_cells[:, 2], ref_cells[:, 1], ref_cells[:, 0] + 1), 1)
    px = cnt.cumsum(2)                                             # px[z, y, x]: records of row (y, z) in the cells < x
    ny = hi[:, 1] - lo[:, 1] + 1
    nrow = ny * (hi[:, 2] - lo[:, 2] + 1)
    r = np.arange(max(int(nrow.max()), 1))[None, :]
    on = r < nrow[:, None]
    cy = np.where(on, lo[:, 1:2] + r % ny[:, None], 0)
    cz = np.where(on, lo[:, 2:3] + r // ny[:, None], 0)
    rec = np.where(on, px[cz, cy, hi[:, 0:1] + 1] - px[cz, cy, lo[:, 0:1]], 0)
    return nrow, rec


def wave_steps(nrow, rec, threads=THREADS, lanes=LANES):
    """The modelled steps of every (wave, u) that holds a query, and the ideal.  Returns (steps, row_part, ideal): arrays over those
    waves; steps = row_part + the record part."""
    nq = nrow.shape[0]
    steps, rows, ideal = [], [], []
    for u in range((nq + threads - 1) // threads):
        for w in range(threads // lanes):
            a = u * threads + w * lanes
            b = min(a + lanes, nq)
            if a >= b:
                continue
            mr = int(nrow[a:b].max())
            steps.append(int(rec[a:b, :mr].max(0).sum()) + mr)
            rows.append(mr)
            ideal.append((int(nrow[a:b].sum()) + int(rec[a:b].sum())) / lanes)
    return np.array(steps), np.array(rows), np.array(ideal)


def direction(q, ref, seed, o, ih, dims, by_cell=False):
    """one direction of one tick -> (steps, row_part, ideal) per wave and (rows, records) per query, summed.  by_cell: the queries are
    dealt to the threads in the order of their own cells (x fastest) instead of their index -- what a wave would issue if its lanes held
    neighbours"""
    lo, hi = boxes(q, ref, seed, o, ih, dims)
    nrow, rec = row_records(cell1(ref, o, ih, dims), dims, lo, hi)
    if by_cell:
        c = cell1(q, o, ih, dims)
        order = np.argsort((c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0], kind="stable")
        nrow, rec = nrow[order], rec[order]
    return wave_steps(nrow, rec) + (int(nrow.sum()), int(rec.sum()))
