// ------------------------------------------------------------------------------------------------
// Exact nearest neighbours by a grid ball search (engine flag nn_cells; ndp_chamfer_nn_cells).
//   The dense kernels evaluate all S x T distances every tick although the answer changes for a few percent of the queries from
//   one tick to the next.  Here the references of a direction are sorted into a uniform grid of NNC_NGX x NNC_NGY x NNC_NGZ cells; a query takes the
//   EXACT distance to a seed reference (last tick's neighbour) as the radius of a ball, evaluates only the references in the cells
//   that the ball's bounding box touches and keeps the lexicographic minimum of (d2, index) -- the minimum distance with the lowest
//   index among equals, which is what k_nn reports.  Every distance is nn_exact_d2, the brute force's own fma chain, and the minimum
//   of a set does not depend on the order of its elements: the records of a cell may lie in any order (they are placed by integer
//   atomics) and no float atomic is used.
//
//   Geometry (per pair, from the TARGETS' bounding box, fixed while the pair lives in its slot): origin o = the box's minimum,
//   inv_h = NG_a / extent per axis a, NG_a that axis' cell count -- 0 where the extent is 0 or the quotient is not finite, which puts the
//   whole axis into cell 0.
//       cell(p) = (int) min(max(floor((p - o) * inv_h), 0), NG_a - 1)                                                (nnc_cell1)
//   per axis, the SAME float expression for references and for the bounds of a query.  It is MONOTONE in p: a rounded subtraction, a
//   rounded product with a non-negative factor, floor and the clamp are each non-decreasing (a NaN goes to cell 0 in every case:
//   max(NaN, 0) = 0).  Points outside the box -- the warped sources, which are sorted into the targets' geometry -- fall into
//   border cells.  The targets' grid is built once when the slot is filled, the sources' grid in LDS every tick.
//
//   WHY THE RANGE IS CONSERVATIVE.  Let b2 be the chain distance of the query q to the seed and t any reference whose chain
//   distance d2c(q, t) <= b2 (the answer is one of them, because the seed itself is a reference).  Per axis a:
//     1. the chain: d2c = fl(dz^2 + fl(dy^2 + fl(dx^2))) with da = fl(q_a - t_a) sums non-negative terms, so da^2 <= d2c (1 + u)^3
//        with u = 2^-24, and |q_a - t_a| <= |da| / (1 - u): |q_a - t_a| <= sqrt(d2c) (1 + 4 u).  Where a square underflows the relative
//        bound fails, but then |da| < 2^-63: |q_a - t_a| <= sqrt(d2c) (1 + 4 u) + 2^-62 always.
//     2. the radius: rs = fl(sqrt(b2)) * (1 + 2^-10) + 1e-18 covers 1. and the rounding of the square root with a factor of a
//        thousand to spare; r' = rs + 2^-20 |q_a| adds an ABSOLUTE margin in |q_a|, 8 ulp of q_a.
//     3. the bounds: fl(q_a - r') differs from q_a - r' by at most 2^-24 (|q_a| + r'), less than the margin 2^-20 |q_a| + 2^-10 sqrt(b2)
//        that r' carries above |q_a - t_a|.  So fl(q_a - r') <= t_a <= fl(q_a + r') as REAL numbers.
//     4. the cell expression needs no margin of its own: it is monotone and applied to fl(q_a - r'), t_a and fl(q_a + r') alike, so
//        cell(fl(q_a - r')) <= cell(t_a) <= cell(fl(q_a + r')) whatever its roundings are.
//   Hence every reference at chain distance <= b2 lies in the enumerated cells, whatever the seed: correctness never rests on
//   coherence between ticks; a poor seed only costs candidates.  A bound that is not finite (inf or NaN) enumerates the whole grid.
//   The argument is per axis and never compares two axes: it holds for any cell count per axis.
//
//   CELLS PER AXIS.  The records of a cell row (fixed y and z cell, x cells lo .. hi) lie contiguously, so a box costs one ROW step per
//   (y, z) cell -- two cell_start reads, the address arithmetic, a loop set-up -- and one RECORD step per record.  The lanes of a wave
//   walk in lock step: a wave issues, per row iteration, as many record steps as its busiest lane has records in that row.  At config A
//   the ball's radius is about one cell of a 16^3 grid; 64 x 8 x 8 cells (x, the row axis, fine; y and z coarse) halve the rows of a box
//   (5.3 -> 2.6 per query) for a third more records (8.4 -> 11.4), and the modelled steps of a wave (tools/nn_wave_steps.py over the
//   oracle's own trajectories, profiles/nn_wave_steps.txt) fall from 70.7 to 61.0, a row step costing about 1.4 record steps on top.
//   Measured (profiles/nn_loss_tick_ab.txt): 16^3 0.048 ms, 32 x 16 x 8 0.042, 64 x 8 x 8 0.041, 64 x 16 x 4 0.044, 128 x 8 x 4 0.048,
//   256 x 4 x 4 0.059.  The wide search (ndp_nn_cells_wide.inc) keeps 16^3 (NNC_NG): the functions below take the counts as template
//   parameters.
//
//   THE MINIMUM AS ONE KEY.  A chain distance is +0, positive, +inf or NaN (squares and sums of squares: never -0, never negative), so
//   its bit pattern orders as its value does, and (d2, index) is kept as the unsigned 64-bit key d2-bits : index with ONE compare and
//   two selects per record (eleven vector instructions per record step; the record is {index, x, y, z} so that the loaded index and the
//   distance computed over x form the key's register pair without a move).  The three corners come out as with two compares:
//     * a NaN distance never wins: its bits (0x7f800001 .. 0x7fffffff, or with the sign bit set) are ABOVE +inf's, and the running key
//       starts at (+inf, 0) and is replaced only by a strictly smaller one;
//     * d2 = +inf leaves index -1: a key (+inf, j) is not strictly below the start (+inf, 0) for any j >= 0, so the start survives, and a
//       final key whose distance is +inf reports index -1 (no finite distance was seen);
//     * equal distances take the lowest index: the index is the key's low word.
//
//   SEEDS.  The seed is last tick's index of the query when there is one: not on a pair's first evaluation (total_evals == 0: the
//   slot's index buffers survive a refill and belong to ANOTHER pair), and not where it is negative or >= the reference count
//   (a stale index of a larger pair).  A stale index IN range is a valid seed like any other.  Without a seed the bound comes from
//   the grid: the smallest chain distance to the records of the nearest non-empty cells, found by growing a Chebyshev cube -- a cube in
//   space: an axis with more cells takes proportionally more of them per step -- around the query's own (clamped) cell until it holds a
//   record.  ANY record's chain distance is a valid bound, so the region's shape is a matter of cost only.
//
//   Launch: one 1024-thread workgroup per pair and DIRECTION (blockIdx.x: 0 sources -> targets, 1 targets -> sources), each thread up
//   to two queries: the stage lasts as long as ONE workgroup (512 of them on 256 CUs), so a workgroup's own chain is what counts.
//   Measured at 256 pairs on the 16^3 grid with two compares per record (profiles/nn_cells_variants.txt): 512 threads x four queries
//   0.076 ms, 1024 x two 0.060 ms.  The walk is bound
//   by the NUMBER of record reads and evaluations a wave issues -- as many as its busiest lane needs -- not by their latency: reading
//   2 / 4 / 8 records of a cell row together (the surplus re-reads the last one) measured 0.065 / 0.073 / 0.102 ms and was not kept; nor
//   were queries taken in cell order (0.060) or a first look into the query's own cell to tighten a stale seed's bound (0.062).
//   LDS per workgroup: records 32 KB + cell_start 16 KB.  Scope: S, T <= NNC_MAX (configs A and B); up to 8192: ndp_nn_cells_wide.inc.
// ------------------------------------------------------------------------------------------------
#ifndef NNC_NGX                                /* cells per axis of this file's search (x: the axis a row runs along) */
#define NNC_NGX 64
#define NNC_NGY 8
#define NNC_NGZ 8
#endif
#define NNC_NG 16                             /* cells per axis of the wide search (ndp_nn_cells_wide.inc): 16^3 */
#define NNC_NC 4096                           /* cells of either grid: the cell_start table is 16 KB */
static_assert(NNC_NGX * NNC_NGY * NNC_NGZ == NNC_NC && NNC_NG * NNC_NG * NNC_NG == NNC_NC, "both grids fill the same cell_start table");
#define NNC_MAX 2048                          /* references / queries per cloud */
#define NNC_NT 1024
#define NNC_NW (NNC_NT / 64)
#define NNC_QPT (NNC_MAX / NNC_NT)            /* queries (and references to sort) per thread */
#define NNC_CS (NNC_NC + 8)                   /* ints per cell_start table: NNC_NC + 1 entries, padded to 16 bytes */
#define NNC_GEOM 8                            /* floats per geometry record: origin[3], inv_h[3], 2 pad */
#define NNC_LDS_BYTES (NNC_MAX * 16 + NNC_CS * 4 + 8 * NNC_NW)

__host__ __device__ inline bool nnc_fits(int n_cap, int t_cap) { return n_cap >= 1 && t_cap >= 1 && n_cap <= NNC_MAX && t_cap <= NNC_MAX; }

struct NncGeom { float o[3], ih[3]; };

__device__ __forceinline__ int nnc_cell1(float p, float o, float ih, int ng) {
    return (int)fminf(fmaxf(floorf((p - o) * ih), 0.f), (float)(ng - 1));
}
// the cell of a point, x fastest
template <int GX, int GY, int GZ>
__device__ __forceinline__ int nnc_cell3(const float (&v)[3], const NncGeom &g) {
    return (nnc_cell1(v[2], g.o[2], g.ih[2], GZ) * GY + nnc_cell1(v[1], g.o[1], g.ih[1], GY)) * GX + nnc_cell1(v[0], g.o[0], g.ih[0], GX);
}
// inv_h of an axis of ng cells and the given extent: 0 for a zero (or vanishing) extent -- one cell on this axis
__device__ __forceinline__ float nnc_inv_h(float ext, int ng) {
    const float ih = ext > 0.f ? (float)ng / ext : 0.f;
    return ih < INFINITY ? ih : 0.f;
}
__device__ __forceinline__ NncGeom nnc_load_geom(const float *g) {
    NncGeom r;
#pragma unroll
    for (int a = 0; a < 3; ++a) { r.o[a] = g[a]; r.ih[a] = g[3 + a]; }
    return r;
}

// exclusive prefix sum of one int per thread over the workgroup's NNC_NT threads (tmp: 2 NNC_NW ints of LDS)
__device__ __forceinline__ int nnc_block_excl_scan(int v, int *tmp, int t) {
    const int lane = t & 63, wv = t >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o);
        if (lane >= o) inc += up;
    }
    if (lane == 63) tmp[wv] = inc;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 0; w < NNC_NT / 64; ++w) base += w < wv ? tmp[w] : 0;
    __syncthreads();
    return base + inc - v;
}

// Counting sort of n <= NNC_MAX points [n][3] into the grid: rec[k] = {index, x, y, z} grouped by cell (x fastest), cs[c] .. cs[c + 1]
// the records of cell c.  In place: cs[c + 1] counts, then holds the cell's first slot, and the scatter's own cursor moves it to the
// cell's end -- which is the next cell's first slot.  All NNC_NT threads call this.
__device__ __forceinline__ void nnc_build_lds(const float *pts, int n, const NncGeom &g, float4 *rec, int *cs, int *tmp, int t) {
    for (int c = t; c < NNC_NC + 1; c += NNC_NT) cs[c] = 0;
    float v[NNC_QPT][3];
    int cell[NNC_QPT];
#pragma unroll
    for (int u = 0; u < NNC_QPT; ++u) {
        const int i = t + NNC_NT * u;
        const float *rp = pts + 3 * (size_t)(i < n ? i : 0);
        v[u][0] = rp[0]; v[u][1] = rp[1]; v[u][2] = rp[2];
        cell[u] = nnc_cell3<NNC_NGX, NNC_NGY, NNC_NGZ>(v[u], g);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NNC_QPT; ++u)
        if (t + NNC_NT * u < n) atomicAdd(&cs[cell[u] + 1], 1);
    __syncthreads();
    constexpr int CPT = NNC_NC / NNC_NT;                      // consecutive cells per thread
    int cnt[CPT], sum = 0;
#pragma unroll
    for (int k = 0; k < CPT; ++k) { cnt[k] = cs[1 + t * CPT + k]; sum += cnt[k]; }
    int run = nnc_block_excl_scan(sum, tmp, t);
#pragma unroll
    for (int k = 0; k < CPT; ++k) { cs[1 + t * CPT + k] = run; run += cnt[k]; }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NNC_QPT; ++u) {
        const int i = t + NNC_NT * u;
        if (i < n) {
            const int pos = atomicAdd(&cs[cell[u] + 1], 1);
            rec[pos] = make_float4(__int_as_float(i), v[u][0], v[u][1], v[u][2]);
        }
    }
    __syncthreads();
}

// lexicographic minimum of (d2, index) over the records of the cells [lo, hi] (per axis, inclusive) of a GX x GY x . grid, from
// (+inf, -1); returns whether a record was seen.  The minimum is kept as ONE unsigned key, d2's bits above the index (see the header).
template <int GX, int GY>
__device__ __forceinline__ bool nnc_scan_box(const float4 *rec, const int *cs, const float (&q)[3], const int (&lo)[3], const int (&hi)[3],
                                             float &bd, int &bj) {
    bool seen = false;
    unsigned long long best = (unsigned long long)0x7f800000u << 32;           // (+inf, 0): no record with d2 = +inf or NaN is below it
    const int ny = hi[1] - lo[1] + 1, nrow = ny * (hi[2] - lo[2] + 1);
    // a row's segment is cs[c0] .. cs[c0 + w]; c0 moves by GX from row to row and by zstep more where y wraps
    const int w = hi[0] - lo[0] + 1, zstep = (GY - ny) * GX;
    int c0 = (lo[2] * GY + lo[1]) * GX + lo[0], left = ny;
    int k0 = cs[c0], k1 = cs[c0 + w];
    for (int r = 0; r < nrow; ++r) {
        // the next row's segment is requested before this row's records are walked (a chain of dependent LDS round trips otherwise)
        int n0 = 0, n1 = 0;
        if (r + 1 < nrow) {
            c0 += GX;
            if (--left == 0) { left = ny; c0 += zstep; }
            n0 = cs[c0]; n1 = cs[c0 + w];
        }
        seen |= k1 > k0;
        for (const float4 *p = rec + k0, *pe = rec + k1; p < pe; ++p) {     // (one cursor: no record index to step beside the address)
            const float4 c = *p;
            const float d = nn_exact_d2(q[0], q[1], q[2], c.y, c.z, c.w);
            const unsigned long long key = ((unsigned long long)__float_as_uint(d) << 32) | __float_as_uint(c.x);
            best = key < best ? key : best;
        }
        k0 = n0; k1 = n1;
    }
    bd = __uint_as_float((unsigned)(best >> 32));
    bj = (best >> 32) == 0x7f800000u ? -1 : (int)(unsigned)best;
    return seen;
}

// One query against the grid in LDS.  b2: the chain distance to the seed, or a negative value when there is no seed.
template <int GX, int GY, int GZ>
__device__ __forceinline__ void nnc_query(const float4 *rec, const int *cs, const NncGeom &g, const float (&q)[3], float b2, float &bd, int &bj) {
    constexpr int ng[3] = {GX, GY, GZ};
    // The growing region of a query without a seed is a cube IN SPACE, not in cells: an axis with sc times the cells of the coarsest axis
    // takes sc cells per step (and sc / 2 at step 0), so that the first record found is near in every direction and the ball it bounds stays
    // small.  (In cells -- one per step on every axis -- a 64 x 8 x 8 grid found its first record up to a coarse cell away in y or z and
    // walked a ball of that radius: 13 fine cells either way in x.)  Step gmin reaches every cell of every axis.
    constexpr int gmin = GX < GY ? (GX < GZ ? GX : GZ) : (GY < GZ ? GY : GZ);
    constexpr int sc[3] = {GX / gmin, GY / gmin, GZ / gmin};
    static_assert(sc[0] * gmin == GX && sc[1] * gmin == GY && sc[2] * gmin == GZ, "cells per axis: multiples of the coarsest axis' count");
    int lo[3], hi[3];
    if (b2 < 0.f) {                                   // no seed: the nearest non-empty cells give the bound
        int c[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) c[a] = nnc_cell1(q[a], g.o[a], g.ih[a], ng[a]);
        b2 = INFINITY;
#pragma unroll 1                                       // (nine copies of the scan tripled the kernel's code: 0.039 -> 0.044 ms at 256 pairs)
        for (int r = 0; r <= gmin; ++r) {
#pragma unroll
            for (int a = 0; a < 3; ++a) { lo[a] = max(c[a] - r * sc[a] - sc[a] / 2, 0); hi[a] = min(c[a] + r * sc[a] + sc[a] / 2, ng[a] - 1); }
            float sd;
            int sj;
            if (nnc_scan_box<GX, GY>(rec, cs, q, lo, hi, sd, sj)) { b2 = sd; break; }
        }
    }
    if (b2 < INFINITY) {
        const float rs = sqrtf(b2) * (1.0f + 0x1p-10f) + 1e-18f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float r = rs + fabsf(q[a]) * 0x1p-20f;
            lo[a] = nnc_cell1(q[a] - r, g.o[a], g.ih[a], ng[a]);
            hi[a] = nnc_cell1(q[a] + r, g.o[a], g.ih[a], ng[a]);
        }
    } else {                                          // inf or NaN: the whole grid
#pragma unroll
        for (int a = 0; a < 3; ++a) { lo[a] = 0; hi[a] = ng[a] - 1; }
    }
    nnc_scan_box<GX, GY>(rec, cs, q, lo, hi, bd, bj);
}

// One direction of one pair: queries qs [nq][3] against references rs [nr][3] (both <= NNC_MAX).
//   grec / gcs: the references' grid in global memory (the targets', built when the slot was filled), or NULL: built here from rs.
//   prev: last tick's indices [nq] or NULL.  Writes d2 / idx [nq]; idx = -1 for [nq, pad_to).
__device__ __forceinline__ void nnc_body(const float *qs, int nq, const float *rs, int nr, const float *geom, const float4 *grec, const int *gcs,
                                         const int *prev, float *d2, int *idx, int pad_to, unsigned char *smem) {
    float4 *rec = reinterpret_cast<float4 *>(smem);
    int *cs = reinterpret_cast<int *>(smem + NNC_MAX * 16);
    int *tmp = cs + NNC_CS;
    const int t = threadIdx.x;
    const NncGeom g = nnc_load_geom(geom);
    // queries, their seeds and the seeds' coordinates are requested before the grid is staged
    float q[NNC_QPT][3], b2[NNC_QPT];
#pragma unroll
    for (int u = 0; u < NNC_QPT; ++u) {
        const int i = t + NNC_NT * u;
        const float *qp = qs + 3 * (size_t)(i < nq ? i : 0);
        q[u][0] = qp[0]; q[u][1] = qp[1]; q[u][2] = qp[2];
        const int s = (prev && i < nq) ? prev[i] : -1;
        const bool ok = s >= 0 && s < nr;
        const float *sp = rs + 3 * (size_t)(ok ? s : 0);
        const float s0 = sp[0], s1 = sp[1], s2 = sp[2];
        b2[u] = ok ? nn_exact_d2(q[u][0], q[u][1], q[u][2], s0, s1, s2) : -1.f;
        if (b2[u] != b2[u]) b2[u] = INFINITY;                  // a NaN bound: the whole grid (and not "no seed")
    }
    if (grec) {
        for (int k = t; k < nr; k += NNC_NT) rec[k] = grec[k];
        const int4 *src = reinterpret_cast<const int4 *>(gcs);
        int4 *dst = reinterpret_cast<int4 *>(cs);
        for (int k = t; k < NNC_CS / 4; k += NNC_NT) dst[k] = src[k];
        __syncthreads();
    } else nnc_build_lds(rs, nr, g, rec, cs, tmp, t);
#pragma unroll                                     // (q / b2 indexed by constants: registers, no scratch)
    for (int u = 0; u < NNC_QPT; ++u) {
        const int i = t + NNC_NT * u;
        if (i < nq) {
            float bd;
            int bj;
            nnc_query<NNC_NGX, NNC_NGY, NNC_NGZ>(rec, cs, g, q[u], b2[u], bd, bj);
            d2[i] = bd; idx[i] = bj;
        } else if (i < pad_to) idx[i] = -1;
    }
}

// the targets' bounding box -> geometry, their grid -> global memory (one workgroup; all NNC_NT threads)
__device__ __forceinline__ void nnc_build_global(const float *ys, int T, float *geom, float4 *grec, int *gcs, unsigned char *smem) {
    float4 *rec = reinterpret_cast<float4 *>(smem);
    int *cs = reinterpret_cast<int *>(smem + NNC_MAX * 16);
    int *tmp = cs + NNC_CS;
    float *red = reinterpret_cast<float *>(tmp);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = t; i < T; i += NNC_NT)
#pragma unroll
        for (int a = 0; a < 3; ++a) { const float v = ys[3 * (size_t)i + a]; mn[a] = fminf(mn[a], v); mx[a] = fmaxf(mx[a], v); }
    NncGeom g;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int o = 32; o; o >>= 1) { mn[a] = fminf(mn[a], __shfl_xor(mn[a], o)); mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], o)); }
        if (lane == 0) { red[wv] = mn[a]; red[NNC_NW + wv] = mx[a]; }
        __syncthreads();
        float lo = red[0], hi = red[NNC_NW];
#pragma unroll
        for (int w = 1; w < NNC_NW; ++w) { lo = fminf(lo, red[w]); hi = fmaxf(hi, red[NNC_NW + w]); }
        __syncthreads();
        const float ih = nnc_inv_h(hi - lo, a == 0 ? NNC_NGX : a == 1 ? NNC_NGY : NNC_NGZ);
        g.o[a] = lo; g.ih[a] = ih;
        if (t == 0) { geom[a] = lo; geom[3 + a] = ih; }
    }
    if (t == 0) { geom[6] = 0.f; geom[7] = 0.f; }
    nnc_build_lds(ys, T, g, rec, cs, tmp, t);
    for (int k = t; k < T; k += NNC_NT) grec[k] = rec[k];
    for (int k = t; k < NNC_CS; k += NNC_NT) gcs[k] = k <= NNC_NC ? cs[k] : 0;
}

// engine: the grid of the targets of the slots a load call has just filled, behind k_eng_load on the same stream
extern "C" __global__ void __launch_bounds__(NNC_NT)
k_eng_nn_cells_build(ndp_engine e, LoadJobs jobs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnc_sm[];
    const ndp_load_job jb = jobs.j[blockIdx.x];
    if (!jb.params || jb.T < 1 || jb.S < 1) return;
    const int b = jb.slot;
    nnc_build_global(e.tgt + (size_t)b * e.t_cap * 3, jb.T, e.nnc_geom + (size_t)b * NNC_GEOM,
                     reinterpret_cast<float4 *>(e.nnc_rec) + (size_t)b * e.t_cap, e.nnc_start + (size_t)b * NNC_CS, nnc_sm);
}

// engine: the NN stage of a tick.  Writes FINAL rows d2x / idx_x and columns d2y / idx_y (idx_y padded with -1 up to t_cap).
extern "C" __global__ void __launch_bounds__(NNC_NT)
k_eng_nn_cells(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnc_sm[];
    const int b = blockIdx.y, dir = blockIdx.x;
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    struct { int level, cur, evals; } st;
    st.level = stp->level; st.cur = stp->cur; st.evals = stp->total_evals;
    const ndp_pair_geom gm = e.geom[b];
    if ((st.level >= e.m) | (gm.S == 0) | (st.cur < 0) | (e.w_cd == 0.f)) return;
    const float *xw = e.pts + ((size_t)b * 2 + (st.cur ^ 1)) * e.n_cap * 3 + 3 * gm.K;
    const float *y = e.tgt + (size_t)b * e.t_cap * 3;
    const float *geom = e.nnc_geom + (size_t)b * NNC_GEOM;
    int *ix = e.idx_x + (size_t)b * e.n_cap, *iy = e.idx_y + (size_t)b * e.t_cap;
    const bool seeded = st.evals != 0;               // a fresh pair: the slot's indices belong to the pair it held before
    if (gm.T < 1) {                                   // no targets: no neighbour (what the dense kernels leave)
        for (int i = threadIdx.x; i < (dir ? e.t_cap : gm.S); i += NNC_NT) {
            if (dir) iy[i] = -1;
            else { e.d2x[(size_t)b * e.n_cap + i] = INFINITY; ix[i] = -1; }
        }
        return;
    }
    if (dir == 0)
        nnc_body(xw, gm.S, y, gm.T, geom, reinterpret_cast<const float4 *>(e.nnc_rec) + (size_t)b * e.t_cap, e.nnc_start + (size_t)b * NNC_CS,
                 seeded ? ix : nullptr, e.d2x + (size_t)b * e.n_cap, ix, gm.S, nnc_sm);
    else
        nnc_body(y, gm.T, xw, gm.S, geom, nullptr, nullptr, seeded ? iy : nullptr, e.d2y + (size_t)b * e.t_cap, iy, e.t_cap, nnc_sm);
}

// standalone: ws = [geometry NNC_GEOM floats | cell_start NNC_CS ints | records T x 4 floats]
__host__ __device__ inline long long nnc_ws_floats(int T) { return NNC_GEOM + NNC_CS + 4LL * T; }
extern "C" __global__ void __launch_bounds__(NNC_NT)
k_nn_cells_build(const float *y, int T, float *ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnc_sm[];
    nnc_build_global(y, T, ws, reinterpret_cast<float4 *>(ws + NNC_GEOM + NNC_CS), reinterpret_cast<int *>(ws + NNC_GEOM), nnc_sm);
}
extern "C" __global__ void __launch_bounds__(NNC_NT)
k_nn_cells(const float *x, int S, const float *y, int T, const int *prev_x, const int *prev_y, float *d2x, int *idx_x, float *d2y, int *idx_y,
           const float *ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnc_sm[];
    if (blockIdx.x == 0)
        nnc_body(x, S, y, T, ws, reinterpret_cast<const float4 *>(ws + NNC_GEOM + NNC_CS), reinterpret_cast<const int *>(ws + NNC_GEOM),
                 prev_x, d2x, idx_x, S, nnc_sm);
    else nnc_body(y, T, x, S, ws, nullptr, nullptr, prev_y, d2y, idx_y, T, nnc_sm);
}
