// ndp_nn_onepass.inc -- one-pass nearest neighbours on the vector pipe: k_eng_nn, the latency shapes k_eng_nn_lat8 / 16, k_nn1, k_nn1_rows.
// ------------------------------------------------------------------------------------------------
// One-pass exact 1-NN for the engine: every squared distance d2(x_i, y_j) is evaluated ONCE and serves both
// directions (loss.py:177-178 calls knn_points twice; SURVEY 8(d) counts 8 S T FLOP for one pass).
//   workgroup = ALL sources x NN1_YCH consecutive targets (SoA in LDS, broadcast ds_read_b128, packed fp32).  The
//   sources are walked in rounds of 512: a thread keeps two of them in registers, wave w of round r owns the 128-source
//   block 4r + w.
//   ROW minimum (nearest target of a source): thread-private, tracked per 16-target sub-chunk, the winning sub-chunk
//   re-scanned exactly at the end of the round; one partial {d2, idx} per (source, target chunk) goes to HBM and is
//   folded by whoever reads it (first chunk wins ties = lowest index).
//   COLUMN minimum (nearest source of a target): over the 128 sources of a wave it is a cross-lane reduction -- a
//   transposed butterfly over the 16 column registers of a sub-chunk (v_permlane32_swap, v_permlane16_swap, DPP
//   row_mirror / row_half_mirror / quad_perm: 35 instructions per 16 targets x 128 sources) -- into an LDS table
//   [block][target]; when all rounds are done the workgroup folds the blocks in order (first block wins ties) and
//   re-scans the winning block for the exact lowest index with the same arithmetic, from a copy of the sources in LDS.
//   d2 and idx are bit-identical to the two-pass brute force (k_nn); nothing but the row partials needs a second look.
// ------------------------------------------------------------------------------------------------
#define NN1_XW 128                    /* sources per wave and round: granularity of the column table */
#define NN1_XB (4 * NN1_XW)           /* sources per round */
#define NN1_YCH 256                   /* targets per workgroup (512: 0.138 ms, 128: 0.137 + a slower row fold, 1024: 0.197) */
#define NN1_XLD (NN1_XW + 1)          /* LDS stride of a 128-source block (the re-scan reads different blocks per lane) */

// v_min_f32 / v_min3_f32 without the canonicalising v_max the compiler puts in front of every fminf operand it cannot
// prove quiet (30 of them per 16-target sub-chunk): the instruction itself returns the other operand for a quiet NaN,
// which is all the NaN padding needs
__device__ __forceinline__ float vmin(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float vmin3(float a, float b, float c) {
    float r;
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float dpp_row_mirror(float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x140, 0xf, 0xf, false));
}
__device__ __forceinline__ float dpp_row_half_mirror(float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), 0x141, 0xf, 0xf, false));
}
template <int CTRL>
__device__ __forceinline__ float dpp_quad(float v) {
    return __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(v), CTRL, 0xf, 0xf, false));
}

// c[16]: per-lane values of 16 columns -> minimum over the 64 lanes of every column; lane L returns column L >> 2
__device__ __forceinline__ float wave_colmin16(const float (&c)[16], int lane) {
    float d[8], e[4], f[2];
#pragma unroll
    for (int r = 0; r < 8; ++r) {                  // lanes L and L ^ 32: lower half keeps column r, upper half column r + 8
        const auto s = __builtin_amdgcn_permlane32_swap(__float_as_uint(c[r]), __float_as_uint(c[r + 8]), false, false);
        d[r] = vmin(__uint_as_float(s[0]), __uint_as_float(s[1]));
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {                  // rows of 16 lanes: even rows keep column r, odd rows column r + 4
        const auto s = __builtin_amdgcn_permlane16_swap(__float_as_uint(d[r]), __float_as_uint(d[r + 4]), false, false);
        e[r] = vmin(__uint_as_float(s[0]), __uint_as_float(s[1]));
    }
    const bool b3 = lane & 8, b2 = lane & 4;
#pragma unroll
    for (int r = 0; r < 2; ++r) {                  // lane l and 15 - l of a row: bit 3 clear keeps r, set keeps r + 2
        const float keep = b3 ? e[r + 2] : e[r], give = b3 ? e[r] : e[r + 2];
        f[r] = vmin(keep, dpp_row_mirror(give));
    }
    const float keep = b2 ? f[1] : f[0], give = b2 ? f[0] : f[1];
    float g = vmin(keep, dpp_row_half_mirror(give));           // lane l and 7 - l of a half row
    g = vmin(g, dpp_quad<0xB1>(g));                            // the four lanes of a quad hold the same column:
    g = vmin(g, dpp_quad<0x4E>(g));                            // fold them (quad_perm [1,0,3,2] then [2,3,0,1])
    return g;
}

struct NnPart { float d2; int idx; };

__host__ __device__ inline int nn1_row_chunks(int t_cap) { return (t_cap + NN1_YCH - 1) / NN1_YCH; }
__host__ __device__ constexpr int nn1_col_blocks(int n_cap) { return (n_cap + NN1_XW - 1) / NN1_XW; }
// dynamic LDS of the one-pass kernel (floats): target chunk, column table, re-scan results, (optionally) the sources
__host__ __device__ inline int nn1_lds_floats(int n_cap, bool stage_x) {
    const int nb = nn1_col_blocks(n_cap);
    return 3 * NN1_YCH + nb * NN1_YCH + (stage_x ? 3 * nb * NN1_XLD : 0);
}
__host__ __device__ inline bool nn1_stage_x(int n_cap) { return nn1_lds_floats(n_cap, true) * 4 <= 80 * 1024; }

// nearest target of NS sources (i[0..NS-1]; i < 0: skipped) from the row partials of the live target chunks (strict <: the
// first chunk keeps ties).  The partials of up to 8 chunks x NS sources are requested together: with one load in flight per
// thread the fold of S = 8192 x 24 chunks by the loss workgroup was a 0.2 ms latency chain.  cstep: the partials are indexed by
// 256-target chunk; a producer whose workgroups cover 512 targets (k_eng_nn_mx8) writes every SECOND slot only -- cstep = 2.
template <int NS>
__device__ __forceinline__ void nn_row_fold_n(const NnPart *rowpart /*[chunks][n_cap]*/, int n_cap, int T, const int (&i)[NS],
                                              NnPart (&r)[NS], int cstep = 1) {
#pragma unroll
    for (int s = 0; s < NS; ++s) { r[s].d2 = INFINITY; r[s].idx = -1; }
    if (!rowpart) return;
    const int live = ((T + NN1_YCH - 1) / NN1_YCH + cstep - 1) / cstep;
    n_cap *= cstep;                                                  // (slot c of the producer is chunk c * cstep)
    for (int c0 = 0; c0 < live; c0 += 8) {
        NnPart q[NS][8];
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                q[s][k].d2 = INFINITY; q[s][k].idx = -1;
                if (c0 + k < live && i[s] >= 0) q[s][k] = rowpart[(size_t)(c0 + k) * n_cap + i[s]];
            }
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int k = 0; k < 8; ++k)
                if (q[s][k].d2 < r[s].d2) r[s] = q[s][k];
    }
}
__device__ __forceinline__ NnPart nn_row_fold(const NnPart *rowpart, int n_cap, int T, int i, int cstep = 1) {
    const int ii[1] = {i};
    NnPart r[1];
    nn_row_fold_n<1>(rowpart, n_cap, T, ii, r, cstep);
    return r[0];
}

// sources [S][3] at xs, targets [T][3] at ys; this workgroup: all sources x targets y0 .. y0 + NN1_YCH - 1.
// rowpart: [n_cap] partials of THIS target chunk; d2y / idx_y: final results for the chunk's targets (idx_y = -1 for
// y0 + j in [T, t_out)).
template <bool STAGE_X>
__device__ __forceinline__ void nn1_body(const float *xs, int S, const float *ys, int T, int y0, int t_out,
                                         NnPart *rowpart, float *d2y, int *idx_y, float *sm) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int nb = (S + NN1_XW - 1) / NN1_XW;      // live source blocks
    float *lx = sm, *ly = sm + NN1_YCH, *lz = sm + 2 * NN1_YCH;
    float *colp = sm + 3 * NN1_YCH;                // [nb][NN1_YCH]
    float *sx = colp + nb * NN1_YCH;               // STAGE_X: [3][nb * NN1_XLD] sources, SoA per block
    const float nanv = __builtin_nanf("");
    const int cn = min(NN1_YCH, T - y0);           // >= 1
    const int cpad = (cn + 15) & ~15;
    for (int j = t; j < NN1_YCH; j += 256) {       // stage the target chunk (NaN padding: never wins a minimum nor an equality)
        float v0 = nanv, v1 = nanv, v2 = nanv;
        if (j < cn) { const float *rp = ys + 3 * (size_t)(y0 + j); v0 = rp[0]; v1 = rp[1]; v2 = rp[2]; }
        lx[j] = v0; ly[j] = v1; lz[j] = v2;
    }
    if (STAGE_X) {
        const int sn = nb * NN1_XLD;
        for (int i = t; i < nb * NN1_XW; i += 256) {
            float v0 = nanv, v1 = nanv, v2 = nanv;
            if (i < S) { v0 = xs[3 * (size_t)i]; v1 = xs[3 * (size_t)i + 1]; v2 = xs[3 * (size_t)i + 2]; }
            const int o = (i >> 7) * NN1_XLD + (i & 127);
            sx[o] = v0; sx[sn + o] = v1; sx[2 * sn + o] = v2;
        }
    }
    __syncthreads();
    for (int xw = wv; xw < nb; xw += 4) {          // this wave's source blocks; no barrier inside
        float qc[2][3];
        f32x2 qx[2], qy[2], qz[2];
        float best[2];
        int sc_best[2];
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int i = xw * NN1_XW + 64 * w + lane;
            qc[w][0] = qc[w][1] = qc[w][2] = nanv;                 // a missing source never wins a minimum
            if (i < S) { qc[w][0] = xs[3 * (size_t)i]; qc[w][1] = xs[3 * (size_t)i + 1]; qc[w][2] = xs[3 * (size_t)i + 2]; }
            qx[w] = f32x2{qc[w][0], qc[w][0]}; qy[w] = f32x2{qc[w][1], qc[w][1]}; qz[w] = f32x2{qc[w][2], qc[w][2]};
            best[w] = INFINITY;
            sc_best[w] = -1;
        }
        float *cp = colp + xw * NN1_YCH + (lane >> 2);
        // (reading the NEXT sub-chunk's 12 broadcast ds_read_b128 ahead of the arithmetic measured slower: 0.141 vs 0.133 ms,
        //  132 registers instead of 70)
        for (int sc = 0; sc < cpad / 16; ++sc) {
            float c[16], m[2] = {INFINITY, INFINITY};
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int o = 16 * sc + 4 * u;
                const float4 X = *reinterpret_cast<const float4 *>(lx + o);
                const float4 Y = *reinterpret_cast<const float4 *>(ly + o);
                const float4 Z = *reinterpret_cast<const float4 *>(lz + o);
                const f32x2 X0 = {X.x, X.y}, X1 = {X.z, X.w}, Y0 = {Y.x, Y.y}, Y1 = {Y.z, Y.w}, Z0 = {Z.x, Z.y}, Z1 = {Z.z, Z.w};
                const f32x2 a0 = pk_dist2(X0, Y0, Z0, qx[0], qy[0], qz[0]), a1 = pk_dist2(X1, Y1, Z1, qx[0], qy[0], qz[0]);
                const f32x2 b0 = pk_dist2(X0, Y0, Z0, qx[1], qy[1], qz[1]), b1 = pk_dist2(X1, Y1, Z1, qx[1], qy[1], qz[1]);
                m[0] = vmin3(m[0], a0.x, a0.y); m[0] = vmin3(m[0], a1.x, a1.y);
                m[1] = vmin3(m[1], b0.x, b0.y); m[1] = vmin3(m[1], b1.x, b1.y);
                c[4 * u] = vmin(a0.x, b0.x); c[4 * u + 1] = vmin(a0.y, b0.y);
                c[4 * u + 2] = vmin(a1.x, b1.x); c[4 * u + 3] = vmin(a1.y, b1.y);
            }
#pragma unroll
            for (int w = 0; w < 2; ++w)
                if (m[w] < best[w]) { best[w] = m[w]; sc_best[w] = sc; }
            const float g = wave_colmin16(c, lane);
            if ((lane & 3) == 0) cp[16 * sc] = g;
        }
        // exact lowest index inside the winning sub-chunk (same arithmetic -> bitwise equality is safe)
#pragma unroll
        for (int w = 0; w < 2; ++w) {
            const int i = xw * NN1_XW + 64 * w + lane;
            if (i >= S) continue;
            int bi = -1;
            if (sc_best[w] >= 0) {
                const int j0 = 16 * sc_best[w];
                for (int j = j0 + 15; j >= j0; --j) {
                    const float dx = qc[w][0] - lx[j], dy = qc[w][1] - ly[j], dz = qc[w][2] - lz[j];
                    const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    if (dd == best[w]) bi = y0 + j;               // descending j: the last hit is the lowest index
                }
            }
            NnPart r; r.d2 = best[w]; r.idx = bi;
            rowpart[i] = r;
        }
    }
    __syncthreads();
    // ---- columns: fold the blocks in order (the first block keeps ties), then the exact lowest index inside the winning
    //      block, one thread per target, candidates from the LDS copy of the sources
    for (int jj = t; jj < NN1_YCH; jj += 256) {
        if (y0 + jj >= t_out) break;
        if (jj >= cn) { idx_y[y0 + jj] = -1; continue; }
        float cbest = INFINITY;
        int blk = -1;
        for (int k = 0; k < nb; ++k) {
            const float v = colp[k * NN1_YCH + jj];
            if (v < cbest) { cbest = v; blk = k; }
        }
        int r = -1;
        if (blk >= 0) {
            const float q0 = lx[jj], q1 = ly[jj], q2 = lz[jj];
            const int k0 = blk * NN1_XW;
            if (STAGE_X) {
                const int sn = nb * NN1_XLD;
                const float *bx = sx + blk * NN1_XLD;
                for (int k = NN1_XW - 1; k >= 0; --k) {               // padding beyond S is NaN: never equal
                    const float dx = bx[k] - q0, dy = bx[sn + k] - q1, dz = bx[2 * sn + k] - q2;
                    const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    if (dd == cbest) r = k0 + k;                      // descending k: the last hit is the lowest index
                }
            } else {
                for (int k = min(k0 + NN1_XW, S) - 1; k >= k0; --k) {
                    const float dx = xs[3 * (size_t)k] - q0, dy = xs[3 * (size_t)k + 1] - q1, dz = xs[3 * (size_t)k + 2] - q2;
                    const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                    if (dd == cbest) r = k;
                }
            }
        }
        d2y[y0 + jj] = cbest;
        idx_y[y0 + jj] = r;
    }
}

// few pairs resident: blockIdx.x < ceil(n_cap/64): 64 source samples -> targets;  else 64 targets -> source samples.
// Writes the final d2x / idx_x / d2y / idx_y (no partials): e.nn_mode = 1 tells the loss kernel to read them.
template <int NW>
__device__ __forceinline__ void eng_nn_lat_stage(const ndp_engine &e, int parity, float *sm) {
    const int b = blockIdx.y;
    // (level, buffer parity and geometry requested side by side, ONE test: see eng_nn_mx_body)
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    struct { int level, cur; } st;
    st.level = stp->level; st.cur = stp->cur;
    const ndp_pair_geom gm = e.geom[b];
    if ((st.level >= e.m) | (gm.S == 0) | (st.cur < 0) | (e.w_cd == 0.f)) return;
    const float *xw = e.pts + ((size_t)b * 2 + (st.cur ^ 1)) * e.n_cap * 3 + 3 * gm.K;
    const float *y = e.tgt + (size_t)b * e.t_cap * 3;
    const int bx = e.n_cap / 64;
    if ((int)blockIdx.x < bx) {
        const int qb = blockIdx.x * 64;
        if (qb >= gm.S) return;
        nn_lat_body<NW>(xw, gm.S, y, gm.T, e.d2x + (size_t)b * e.n_cap, e.idx_x + (size_t)b * e.n_cap, qb, sm);
    } else {
        const int qb = (blockIdx.x - bx) * 64;
        int *iy = e.idx_y + (size_t)b * e.t_cap;
        if (qb < gm.T) nn_lat_body<NW>(y, gm.T, xw, gm.S, e.d2y + (size_t)b * e.t_cap, iy, qb, sm);
        if (threadIdx.x < 64 && qb + (int)threadIdx.x >= gm.T && qb + (int)threadIdx.x < e.t_cap) iy[qb + threadIdx.x] = -1;
    }
}
// eight waves per 64 queries (each scans an eighth of every stage): what the engine launches (round 4; four waves were measured and
// retired as gemm_mode bit 128) -- at batch 1 the stage is one workgroup's latency (the fold over the waves keeps the lowest index)
extern "C" __global__ void __launch_bounds__(512)
k_eng_nn_lat8(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    eng_nn_lat_stage<8>(e, parity, sm);
}
// sixteen waves per 64 queries (each scans a sixteenth of every stage): the engine's launch since round 6 when the pair count is small
// enough for the stage to be ONE workgroup's latency (B <= 2: the scan of a stage is half as long; same fold, same results)
extern "C" __global__ void __launch_bounds__(1024)
k_eng_nn_lat16(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    eng_nn_lat_stage<16>(e, parity, sm);
}

extern "C" __global__ void __launch_bounds__(256)
k_eng_nn(ndp_engine e, int parity, int stage_x) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.y;
    const ndp_pair_state st = e.state[parity * e.B + b];
    if (st.level >= e.m) return;
    const ndp_pair_geom gm = e.geom[b];
    if (gm.S == 0 || e.w_cd == 0.f) return;
    const int y0 = blockIdx.x * NN1_YCH;
    int *iy = e.idx_y + (size_t)b * e.t_cap;
    if (y0 >= gm.T) {                               // keep the -1 padding beyond T
        for (int j = y0 + threadIdx.x; j < min(y0 + NN1_YCH, e.t_cap); j += 256) iy[j] = -1;
        return;
    }
    const float *xw = e.pts + ((size_t)b * 2 + (st.cur ^ 1)) * e.n_cap * 3 + 3 * gm.K;
    const float *y = e.tgt + (size_t)b * e.t_cap * 3;
    NnPart *rowpart = reinterpret_cast<NnPart *>(e.nn_row) + ((size_t)b * nn1_row_chunks(e.t_cap) + blockIdx.x) * e.n_cap;
    if (stage_x) nn1_body<true>(xw, gm.S, y, gm.T, y0, e.t_cap, rowpart, e.d2y + (size_t)b * e.t_cap, iy, sm);
    else nn1_body<false>(xw, gm.S, y, gm.T, y0, e.t_cap, rowpart, e.d2y + (size_t)b * e.t_cap, iy, sm);
}

// the same kernel as a standalone operator on one pair, plus the fold of its row partials
extern "C" __global__ void __launch_bounds__(256)
k_nn1(const float *x, int S, const float *y, int T, int n_cap, float *ws_row, float *d2y, int *idx_y, int stage_x) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int y0 = blockIdx.x * NN1_YCH;
    if (y0 >= T) return;
    NnPart *rowpart = reinterpret_cast<NnPart *>(ws_row) + (size_t)blockIdx.x * n_cap;
    if (stage_x) nn1_body<true>(x, S, y, T, y0, T, rowpart, d2y, idx_y, sm);
    else nn1_body<false>(x, S, y, T, y0, T, rowpart, d2y, idx_y, sm);
}
extern "C" __global__ void __launch_bounds__(256)
k_nn1_rows(int S, int T, int n_cap, const float *ws_row, float *d2x, int *idx_x) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const NnPart r = nn_row_fold(reinterpret_cast<const NnPart *>(ws_row), n_cap, T, i);
    d2x[i] = r.d2;
    idx_x[i] = r.idx;
}
