// ------------------------------------------------------------------------------------------------
// The exact grid ball search for clouds of up to NNW_MAX = 8192 points (engine flag nn_cells_wide; ndp_chamfer_nn_cells_wide).
//   Same algorithm, same geometry and same exactness argument as ndp_nn_cells.inc (its header's WHY THE RANGE IS CONSERVATIVE and SEEDS
//   hold here word for word): per query the radius is the chain distance nn_exact_d2 to a seed, every cell the ball's bounding box touches
//   is enumerated (nnc_query / nnc_scan_box / nnc_cell1 are that file's own functions, called with NNC_NG = 16 cells on every axis -- the
//   per-axis counts of the 2048-point search were chosen for ITS ball sizes and are not measured here) and the result is the
//   lexicographic minimum of (d2, index) -- the brute force's bits for ANY seed values.  What differs is the kernels' shape:
//
//   * A reference grid of 8192 records is 128 KB of LDS, so a workgroup holds ONE grid and nothing else of that size: the grids are sorted
//     in global memory and only COPIED into LDS by the search.  The targets' grid is built once per pair behind k_eng_load
//     (k_eng_nnw_build), the warped sources' grid once per pair and tick by a launch of its own in front of the search (k_eng_nnw_sort:
//     one workgroup per pair; the search of that tick starts behind it on the same stream, so no grid-wide barrier is needed).  The
//     counting sort keeps its counters in LDS (integer atomics, order-free result) and scatters the records straight to global memory.
//   * The queries of one pair and direction are split over Q = ceil(max(n_cap, t_cap) / NNW_CH) workgroups: blockIdx.x = direction * Q +
//     chunk, blockIdx.y = pair.  Each stages the whole reference grid of its direction and answers the queries [chunk * NNW_CH,
//     (chunk + 1) * NNW_CH) -- two per thread, as k_eng_nn_cells does, so a workgroup's own chain is that kernel's.  The chunks partition
//     [0, nq) and, for the columns, the -1 padding of idx_y up to t_cap: every element has exactly one writer.  A chunk that starts
//     behind both ends returns before it stages anything.
//
//   LDS per search workgroup: records 128 KB + cell_start 16 416 B = 147 488 B (one workgroup per CU); per sort / build workgroup:
//   cell_start + the scan's scratch.  Scope: 1 <= S, T <= NNW_MAX.
// ------------------------------------------------------------------------------------------------
#define NNW_MAX 8192                          /* references / queries per cloud */
#define NNW_NT NNC_NT                         /* (nnc_block_excl_scan is written for NNC_NT threads) */
#define NNW_QPT 2                             /* queries per thread of a search workgroup */
#define NNW_CH (NNW_NT * NNW_QPT)             /* queries per search workgroup */
#define NNW_SPT (NNW_MAX / NNW_NT)            /* references to sort per thread */
#define NNW_LDS_BYTES (NNW_MAX * 16 + NNC_CS * 4)
#define NNW_SORT_LDS_BYTES (NNC_CS * 4 + 8 * NNC_NW)

__host__ __device__ inline bool nnw_fits(int n_cap, int t_cap) { return n_cap >= 1 && t_cap >= 1 && n_cap <= NNW_MAX && t_cap <= NNW_MAX; }
__host__ __device__ inline int nnw_chunks(int n_cap, int t_cap) { return ((n_cap > t_cap ? n_cap : t_cap) + NNW_CH - 1) / NNW_CH; }

// Counting sort of n <= NNW_MAX points [n][3] into the grid g: grec[k] = {index, x, y, z} grouped by cell in GLOBAL memory, gcs[0 .. NNC_CS)
// the cell_start table there.  The counters live in LDS (cs: NNC_CS ints, tmp: 2 NNC_NW ints) exactly as in nnc_build_lds.  All NNW_NT threads.
__device__ __forceinline__ void nnw_sort_global(const float *pts, int n, const NncGeom &g, float4 *grec, int *gcs, int *cs, int *tmp, int t) {
    for (int c = t; c < NNC_NC + 1; c += NNW_NT) cs[c] = 0;
    float v[NNW_SPT][3];
    int cell[NNW_SPT];
#pragma unroll
    for (int u = 0; u < NNW_SPT; ++u) {
        const int i = t + NNW_NT * u;
        const float *rp = pts + 3 * (size_t)(i < n ? i : 0);
        v[u][0] = rp[0]; v[u][1] = rp[1]; v[u][2] = rp[2];
        cell[u] = nnc_cell3<NNC_NG, NNC_NG, NNC_NG>(v[u], g);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NNW_SPT; ++u)
        if (t + NNW_NT * u < n) atomicAdd(&cs[cell[u] + 1], 1);
    __syncthreads();
    constexpr int CPT = NNC_NC / NNW_NT;                      // consecutive cells per thread
    int cnt[CPT], sum = 0;
#pragma unroll
    for (int k = 0; k < CPT; ++k) { cnt[k] = cs[1 + t * CPT + k]; sum += cnt[k]; }
    int run = nnc_block_excl_scan(sum, tmp, t);
    // the table as the search reads it (cs[c] = first record of cell c, cs[NNC_NC] = n), written before the scatter moves the cursors
    if (t == 0) gcs[0] = 0;
#pragma unroll
    for (int k = 0; k < CPT; ++k) { cs[1 + t * CPT + k] = run; run += cnt[k]; gcs[1 + t * CPT + k] = run; }
    for (int c = NNC_NC + 1 + t; c < NNC_CS; c += NNW_NT) gcs[c] = 0;
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NNW_SPT; ++u) {
        const int i = t + NNW_NT * u;
        if (i < n) {
            const int pos = atomicAdd(&cs[cell[u] + 1], 1);
            grec[pos] = make_float4(__int_as_float(i), v[u][0], v[u][1], v[u][2]);
        }
    }
}

// the targets' bounding box -> geometry (as nnc_build_global computes it), their grid -> global memory (one workgroup; all NNW_NT threads)
__device__ __forceinline__ void nnw_build_global(const float *ys, int T, float *geom, float4 *grec, int *gcs, unsigned char *smem) {
    int *cs = reinterpret_cast<int *>(smem);
    int *tmp = cs + NNC_CS;
    float *red = reinterpret_cast<float *>(tmp);
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = t; i < T; i += NNW_NT)
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
        const float ih = nnc_inv_h(hi - lo, NNC_NG);
        g.o[a] = lo; g.ih[a] = ih;
        if (t == 0) { geom[a] = lo; geom[3 + a] = ih; }
    }
    if (t == 0) { geom[6] = 0.f; geom[7] = 0.f; }
    nnw_sort_global(ys, T, g, grec, gcs, cs, tmp, t);
}

// One chunk of one direction of one pair: the queries [q0, q0 + NNW_CH) of qs [nq][3] against the references rs [nr][3], whose grid
// (grec [nr], gcs [NNC_CS]) lies sorted in global memory.  prev: last tick's indices [nq] or NULL.  Writes d2 / idx of its queries;
// idx = -1 for its share of [nq, pad_to).
__device__ __forceinline__ void nnw_body(const float *qs, int nq, const float *rs, int nr, const float *geom, const float4 *grec, const int *gcs,
                                         const int *prev, float *d2, int *idx, int pad_to, int q0, unsigned char *smem) {
    float4 *rec = reinterpret_cast<float4 *>(smem);
    int *cs = reinterpret_cast<int *>(smem + NNW_MAX * 16);
    const int t = threadIdx.x;
    const NncGeom g = nnc_load_geom(geom);
    // queries, their seeds and the seeds' coordinates are requested before the grid is staged
    float q[NNW_QPT][3], b2[NNW_QPT];
#pragma unroll
    for (int u = 0; u < NNW_QPT; ++u) {
        const int i = q0 + t + NNW_NT * u;
        const float *qp = qs + 3 * (size_t)(i < nq ? i : 0);
        q[u][0] = qp[0]; q[u][1] = qp[1]; q[u][2] = qp[2];
        const int s = (prev && i < nq) ? prev[i] : -1;
        const bool ok = s >= 0 && s < nr;
        const float *sp = rs + 3 * (size_t)(ok ? s : 0);
        const float s0 = sp[0], s1 = sp[1], s2 = sp[2];
        b2[u] = ok ? nn_exact_d2(q[u][0], q[u][1], q[u][2], s0, s1, s2) : -1.f;
        if (b2[u] != b2[u]) b2[u] = INFINITY;                  // a NaN bound: the whole grid (and not "no seed")
    }
    for (int k = t; k < nr; k += NNW_NT) rec[k] = grec[k];
    const int4 *src = reinterpret_cast<const int4 *>(gcs);
    int4 *dst = reinterpret_cast<int4 *>(cs);
    for (int k = t; k < NNC_CS / 4; k += NNW_NT) dst[k] = src[k];
    __syncthreads();
#pragma unroll                                     // (q / b2 indexed by constants: registers, no scratch)
    for (int u = 0; u < NNW_QPT; ++u) {
        const int i = q0 + t + NNW_NT * u;
        if (i < nq) {
            float bd;
            int bj;
            nnc_query<NNC_NG, NNC_NG, NNC_NG>(rec, cs, g, q[u], b2[u], bd, bj);
            d2[i] = bd; idx[i] = bj;
        } else if (i < pad_to) idx[i] = -1;
    }
}

// Engine buffers.  The wide search keeps its grids in the engine's three grid buffers, in a layout of its own (an engine runs one of the two
// searches, never both): nnc_geom [B][8] as for nn_cells; nnc_start [B][2][NNC_CS]: the targets' cell_start table, then the warped
// sources'; nnc_rec [B][t_cap + n_cap][4]: the targets' records, then the warped sources'.
__device__ __forceinline__ int *nnw_start_tgt(const ndp_engine &e, int b) { return e.nnc_start + (size_t)b * 2 * NNC_CS; }
__device__ __forceinline__ int *nnw_start_src(const ndp_engine &e, int b) { return nnw_start_tgt(e, b) + NNC_CS; }
__device__ __forceinline__ float4 *nnw_rec_tgt(const ndp_engine &e, int b) { return reinterpret_cast<float4 *>(e.nnc_rec) + (size_t)b * (e.t_cap + e.n_cap); }
__device__ __forceinline__ float4 *nnw_rec_src(const ndp_engine &e, int b) { return nnw_rec_tgt(e, b) + e.t_cap; }

// engine: the grid of the targets of the slots a load call has just filled, behind k_eng_load on the same stream
extern "C" __global__ void __launch_bounds__(NNW_NT)
k_eng_nnw_build(ndp_engine e, LoadJobs jobs) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnw_sm[];
    const ndp_load_job jb = jobs.j[blockIdx.x];
    if (!jb.params || jb.T < 1 || jb.S < 1) return;
    const int b = jb.slot;
    nnw_build_global(e.tgt + (size_t)b * e.t_cap * 3, jb.T, e.nnc_geom + (size_t)b * NNC_GEOM, nnw_rec_tgt(e, b), nnw_start_tgt(e, b), nnw_sm);
}

// what the two tick kernels below do with a pair: the early-outs of k_eng_nn_cells, in its order
struct NnwJob { bool run; int S, T; const float *xw, *y, *geom; };
__device__ __forceinline__ NnwJob nnw_job(const ndp_engine &e, int parity, int b, bool &seeded) {
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    const int level = stp->level, cur = stp->cur, evals = stp->total_evals;
    const ndp_pair_geom gm = e.geom[b];
    NnwJob j;
    j.run = !((level >= e.m) | (gm.S == 0) | (cur < 0) | (e.w_cd == 0.f));
    j.S = gm.S; j.T = gm.T;
    j.xw = e.pts + ((size_t)b * 2 + ((cur < 0 ? 0 : cur) ^ 1)) * e.n_cap * 3 + 3 * gm.K;
    j.y = e.tgt + (size_t)b * e.t_cap * 3;
    j.geom = e.nnc_geom + (size_t)b * NNC_GEOM;
    seeded = evals != 0;                                  // a fresh pair: the slot's indices belong to the pair it held before
    return j;
}

// engine: this tick's warped sources sorted into the targets' geometry, one workgroup per pair, in front of k_eng_nn_cells_wide
extern "C" __global__ void __launch_bounds__(NNW_NT)
k_eng_nnw_sort(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnw_sm[];
    const int b = blockIdx.x;
    bool seeded;
    const NnwJob j = nnw_job(e, parity, b, seeded);
    if (!j.run || j.T < 1) return;                        // (no targets: the search writes "no neighbour" and reads no grid)
    int *cs = reinterpret_cast<int *>(nnw_sm);
    nnw_sort_global(j.xw, j.S, nnc_load_geom(j.geom), nnw_rec_src(e, b), nnw_start_src(e, b), cs, cs + NNC_CS, threadIdx.x);
}

// engine: the NN stage of a tick.  Writes FINAL rows d2x / idx_x and columns d2y / idx_y (idx_y padded with -1 up to t_cap).
extern "C" __global__ void __launch_bounds__(NNW_NT)
k_eng_nn_cells_wide(ndp_engine e, int parity, int Q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnw_sm[];
    const int b = blockIdx.y, dir = (int)blockIdx.x >= Q ? 1 : 0, q0 = ((int)blockIdx.x - dir * Q) * NNW_CH;
    bool seeded;
    const NnwJob j = nnw_job(e, parity, b, seeded);
    if (!j.run) return;
    int *ix = e.idx_x + (size_t)b * e.n_cap, *iy = e.idx_y + (size_t)b * e.t_cap;
    if (q0 >= (dir ? e.t_cap : j.S)) return;              // a chunk behind the queries and the padding: nothing to write
    if (j.T < 1) {                                        // no targets: no neighbour (what the dense kernels leave)
        const int end = min(dir ? e.t_cap : j.S, q0 + NNW_CH);
        for (int i = q0 + threadIdx.x; i < end; i += NNW_NT) {
            if (dir) iy[i] = -1;
            else { e.d2x[(size_t)b * e.n_cap + i] = INFINITY; ix[i] = -1; }
        }
        return;
    }
    if (dir == 0)
        nnw_body(j.xw, j.S, j.y, j.T, j.geom, nnw_rec_tgt(e, b), nnw_start_tgt(e, b), seeded ? ix : nullptr, e.d2x + (size_t)b * e.n_cap, ix, j.S, q0, nnw_sm);
    else
        nnw_body(j.y, j.T, j.xw, j.S, j.geom, nnw_rec_src(e, b), nnw_start_src(e, b), seeded ? iy : nullptr, e.d2y + (size_t)b * e.t_cap, iy, e.t_cap, q0, nnw_sm);
}

// standalone: ws = [geometry NNC_GEOM floats | targets' cell_start NNC_CS ints | sources' cell_start NNC_CS ints | targets' records T x 4
//                   floats | sources' records S x 4 floats]
__host__ __device__ inline long long nnw_ws_floats(int S, int T) { return NNC_GEOM + 2 * NNC_CS + 4LL * T + 4LL * S; }
extern "C" __global__ void __launch_bounds__(NNW_NT)
k_nnw_build(const float *y, int T, float *ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnw_sm[];
    nnw_build_global(y, T, ws, reinterpret_cast<float4 *>(ws + NNC_GEOM + 2 * NNC_CS), reinterpret_cast<int *>(ws + NNC_GEOM), nnw_sm);
}
extern "C" __global__ void __launch_bounds__(NNW_NT)
k_nnw_sort(const float *x, int S, int T, float *ws) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnw_sm[];
    int *cs = reinterpret_cast<int *>(nnw_sm);
    nnw_sort_global(x, S, nnc_load_geom(ws), reinterpret_cast<float4 *>(ws + NNC_GEOM + 2 * NNC_CS + 4 * (size_t)T),
                    reinterpret_cast<int *>(ws + NNC_GEOM + NNC_CS), cs, cs + NNC_CS, threadIdx.x);
}
extern "C" __global__ void __launch_bounds__(NNW_NT)
k_nn_cells_wide(const float *x, int S, const float *y, int T, const int *prev_x, const int *prev_y, float *d2x, int *idx_x, float *d2y, int *idx_y,
                const float *ws, int Q) {
    extern __shared__ __attribute__((aligned(16))) unsigned char nnw_sm[];
    const int dir = (int)blockIdx.x >= Q ? 1 : 0, q0 = ((int)blockIdx.x - dir * Q) * NNW_CH;
    if (q0 >= (dir ? T : S)) return;
    const float4 *rec_t = reinterpret_cast<const float4 *>(ws + NNC_GEOM + 2 * NNC_CS);
    const int *cs_t = reinterpret_cast<const int *>(ws + NNC_GEOM);
    if (dir == 0) nnw_body(x, S, y, T, ws, rec_t, cs_t, prev_x, d2x, idx_x, S, q0, nnw_sm);
    else nnw_body(y, T, x, S, ws, rec_t + T, cs_t + NNC_CS, prev_y, d2y, idx_y, T, q0, nnw_sm);
}
