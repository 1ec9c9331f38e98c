// ------------------------------------------------------------------------------------------------
// One-pass nearest neighbours with the S x T distances on the bf16 MATRIX pipe (engine nn_mode 2).
//   The vector kernel (nn1_body) spends 8 lane-operations per distance and runs at ~90 % of the vector rate.  Here
//   |x - y|^2 = |x|^2 + |y|^2 - 2 x.y is ONE contraction per 32 x 32 tile of (source, target) pairs: every coordinate, -2 y and the
//   two squared norms as THREE-WAY bf16 SPLITS (hi + mid + lo = 24 mantissa bits), six partial products per coordinate, three per
//   norm = 24 of the 32 slots of two v_mfma_f32_32x32x16_bf16 -- 64 matrix-pipe cycles per 1024 distances; the vector pipe only
//   takes minima: half a v_min3 per distance for the row direction, half for the column direction.  (Vector instructions BEHIND a
//   block of MFMAs are paid in full by an in-order wave -- rounds 4 and 5 measured the distance loop at the SUM, ~30 ns of MFMA and
//   ~32 ns of v_min3 per 1024 distances and wave; placed BETWEEN the MFMAs they ride in the matrix pipe's shadow, coexec2.hip:
//   since round 6 the loop is a software pipeline, see "ORDER" below.)  That value is APPROXIMATE (cancellation: absolute error a few 2^-22 R^2 for points of norm <= R), so
//   it only SELECTS candidates; every reported distance and index is then recomputed with the exact fma chain of the brute force
//   ((x - y)^2, z last) -- results stay bit-identical to k_nn:
//     rows    a lane of the 32 x 32 tile owns one target CLASS (j mod 32) of every source row; the element-wise minimum over the
//             chunk's 8 tiles leaves, per source, 32 class minima.  They are transposed through a wave-private LDS
//             scratch, the best class (tagged in the 4 low mantissa bits) and the runner-up VALUE are found in-lane, the 8
//             targets of the best class are evaluated exactly, and if the runner-up lies within the error bound
//             (thr = n1 + 2^-16 R^2 + 2^-17 |n1|) every class below thr is evaluated too -- about a percent of the sources.
//     columns the minimum over a wave's 128 sources goes to the LDS table [block][target] as in the vector kernel; a target
//             re-scans, in descending order, every block whose table entry is within the bound of the best one (usually one).
//   Ties: all candidates within the bound are compared exactly and the lowest index wins, as in k_nn.
//   (The same scheme on the fp32 MFMA measured SLOWER than the vector kernel, 0.149 vs 0.131 ms: 256 matrix-pipe cycles per 1024
//    distances instead of 64, and every one of them shuts the vector pipe of its SIMD out.)
// ------------------------------------------------------------------------------------------------
#define NN2_TS 33                     /* row stride of the transposition scratch: [32 sources][32 classes] per wave */
#define NN2_NB_MAX 16                 /* 128-source blocks resident in LDS at a time (2048 sources: 78.6 KB, two workgroups per CU); more
                                         sources are walked in PASSES of that many, highest indices first (round 3) */
// NW waves per workgroup (4: 256 targets per chunk, two workgroups per CU; 8: 512 targets per chunk, one workgroup per CU -- the same
// eight waves per CU, but the per-workgroup set-up (sources -> LDS, norms), the A operands of a source block and the row stage
// (transposition + exact evaluation per source block and CHUNK) are paid once per 512 targets instead of once per 256)
__host__ __device__ constexpr int nn2_nb(int n_cap) { return nn1_col_blocks(n_cap) < NN2_NB_MAX ? nn1_col_blocks(n_cap) : NN2_NB_MAX; }
__host__ __device__ constexpr int nb_cap_floats(int nb, int nw) { return nb * 64 * nw + 3 * nb * NN1_XLD + nw * 32 * NN2_TS + 8; }
__host__ __device__ constexpr int nn2_lds_floats(int n_cap, int nw = 4) {
    return ((4 * 64 * nw + nb_cap_floats(nn2_nb(n_cap), nw) + 3) & ~3) + 2 * nw * 2 * 64 * 4;
}
// nn2_nb caps the resident blocks, so both carves have a worst case whatever n_cap is: no engine and no S is refused for its size
static_assert(nn2_lds_floats(NN2_NB_MAX * NN1_XW, 4) * 4 <= 80 * 1024, "4 waves (k_nn2): two workgroups per CU");
static_assert(nn2_lds_floats(NN2_NB_MAX * NN1_XW, 8) * 4 <= 160 * 1024, "8 waves (k_eng_nn_mx8): one workgroup per CU");

// x = hi + mid + lo in bf16; a non-finite x (padding: +inf) stays in hi alone
__device__ __forceinline__ void nn2_split3(float x, __bf16 &hi, __bf16 &mid, __bf16 &lo) {
    hi = (__bf16)x;
    const float r1 = x - (float)hi;
    const bool fin = x < INFINITY;
    mid = (__bf16)(fin ? r1 : 0.f);
    lo = (__bf16)(fin ? r1 - (float)mid : 0.f);
}

__device__ __forceinline__ float vmed3(float a, float b, float c) {
    float r;
    asm("v_med3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}
__device__ __forceinline__ float vmax(float a, float b) {
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ float nn_exact_d2(float s0, float s1, float s2, float t0, float t1, float t2) {
    const float dx = s0 - t0, dy = s1 - t1, dz = s2 - t2;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}
__device__ __forceinline__ float dpp_swap1(float v) { return dpp_quad<0xB1>(v); }        // lane l <-> l ^ 1
__device__ __forceinline__ int dpp_swap1(int v) { return __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xf, 0xf, false); }

template <int NW>
__device__ __forceinline__ void nn2_body(const float *xs, int S, const float *ys, int T, int y0, int t_out,
                                         NnPart *rowpart, float *d2y, int *idx_y, float *sm) {
    static_assert(NN1_XW == 128 && (NW == 4 || NW == 8), "thread t stages target t; a wave's block is four 32-row tiles");
    constexpr int YCH = 64 * NW, NT = 64 * NW, NTL = 2 * NW;           // targets per chunk, threads, 32-target tiles per chunk
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int nb_all = (S + NN1_XW - 1) / NN1_XW;
    const int nb = nb_all < NN2_NB_MAX ? nb_all : NN2_NB_MAX;                     // blocks resident per pass (the LDS carve)
    const int npass = (nb_all + nb - 1) / nb;
    float *lx = sm, *ly = sm + YCH, *lz = sm + 2 * YCH, *ny = sm + 3 * YCH;
    float *colp = sm + 4 * YCH;                   // [nb][YCH] approximate column minima per source block
    float *sx = colp + nb * YCH;              // [3][nb * NN1_XLD] sources, SoA per block
    const int sn = nb * NN1_XLD;
    float *scr = sx + 3 * sn + wv * (32 * NN2_TS);
    float *red = sx + 3 * sn + NW * 32 * NN2_TS;
    // [NTL tiles][2 instructions][64 lanes] B operands of the chunk's targets, 16-byte aligned (3 nb NN1_XLD floats are not a multiple of 4 for every nb)
    bf16x8 *bop = reinterpret_cast<bf16x8 *>(sm + ((4 * YCH + nb_cap_floats(nb, NW) + 3) & ~3));
    const float nanv = __builtin_nanf("");
    const int cn = min(YCH, T - y0);              // >= 1
    PT_INIT;
    PT_DECL;
    float r2t = 0.f;
    {   // targets (NaN coordinates beyond cn: never equal in an exact comparison; |y|^2 = inf: never a minimum on the matrix pipe)
        float v0 = nanv, v1 = nanv, v2 = nanv, nn = INFINITY;
        if (t < cn) {
            const float *rp = ys + 3 * (size_t)(y0 + t);
            v0 = rp[0]; v1 = rp[1]; v2 = rp[2];
            nn = fmaf(v2, v2, fmaf(v1, v1, v0 * v0));
            r2t = nn;
        }
        lx[t] = v0; ly[t] = v1; lz[t] = v2; ny[t] = nn;
        // the 24 (of 32) contraction slots of this target: per coordinate c, u = -2 y_c against the source's x_c as
        //   A (xh, xh, xm, xh, xl, xm) . B (uh, um, uh, ul, uh, um);  then A (nxh, nxm, nxl) . B (1, 1, 1);  A (1, 1, 1) . B (nyh, nym, nyl)
        const bool lv = t < cn;
        const float u[3] = {lv ? -2.0f * v0 : 0.f, lv ? -2.0f * v1 : 0.f, lv ? -2.0f * v2 : 0.f};
        __bf16 sb[32];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            __bf16 a, m, l;
            nn2_split3(u[c], a, m, l);
            sb[6 * c] = a; sb[6 * c + 1] = m; sb[6 * c + 2] = a; sb[6 * c + 3] = l; sb[6 * c + 4] = a; sb[6 * c + 5] = m;
        }
        {
            __bf16 a, m, l;
            nn2_split3(nn, a, m, l);
            sb[18] = (__bf16)1.0f; sb[19] = (__bf16)1.0f; sb[20] = (__bf16)1.0f; sb[21] = a; sb[22] = m; sb[23] = l;
        }
#pragma unroll
        for (int q = 24; q < 32; ++q) sb[q] = (__bf16)0.f;
        bf16x8 *bo = bop + (size_t)(t >> 5) * 128 + (t & 31);
#pragma unroll
        for (int blk = 0; blk < 4; ++blk) {                          // slots 8 blk .. + 7 -> instruction blk >> 1, lane half blk & 1
            bf16x8 v;
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = sb[8 * blk + e];
            bo[64 * (blk >> 1) + 32 * (blk & 1)] = v;
        }
    }
    // per-target running answer across the passes (thread t <-> target t)
    const bool live = t < cn;
    float best = INFINITY;
    int rr = -1;
    const float relc = 7.62939453125e-06f;                        // 2^-17: the exact chain's own rounding (5 u d) twice + 16 ulp of tag
    const int ntile = (cn + 31) >> 5;
    f32x16 zero16;
#pragma unroll
    for (int r = 0; r < 16; ++r) zero16[r] = 0.f;
    // Sources beyond the LDS carve: passes of nb blocks, HIGHEST source indices first, so that the exact comparisons of the column
    // direction (candidates descending, `<=`) still end on the lowest index of the smallest distance.  A source belongs to exactly one
    // pass: its row partial is complete when its pass is.  The error bound of a pass uses the norms of THAT pass's sources and the
    // chunk's targets (every approximate distance involves one of each).
  for (int pass = npass - 1; pass >= 0; --pass) {
    const int s0 = pass * nb * NN1_XW, Sp = min(S - s0, nb * NN1_XW), nbp = (Sp + NN1_XW - 1) / NN1_XW;
    if (pass != npass - 1) __syncthreads();                       // the previous pass's column stage is done with sx / colp / red
    float r2 = r2t;
    // Staging: FOUR items per thread requested together, then stored (2048 sources on 512 threads: the whole pass in one global round
    // trip; until round 6 one round trip per item, in the open at the top of every workgroup).  Same values, same maximum.
    for (int i0 = t; i0 < nb * NN1_XW; i0 += 4 * NT) {
        float sv[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * NT;
            const bool ok = i < Sp;
            const float *rp = xs + 3 * (size_t)(s0 + (ok ? i : 0));
            const float a0 = rp[0], a1 = rp[1], a2 = rp[2];
            sv[u][0] = ok ? a0 : nanv; sv[u][1] = ok ? a1 : nanv; sv[u][2] = ok ? a2 : nanv;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int i = i0 + u * NT;
            if (i < nb * NN1_XW) {
                const float v0 = sv[u][0], v1 = sv[u][1], v2 = sv[u][2];
                if (i < Sp) r2 = fmaxf(r2, fmaf(v2, v2, fmaf(v1, v1, v0 * v0)));
                const int o = (i >> 7) * NN1_XLD + (i & 127);
                sx[o] = v0; sx[sn + o] = v1; sx[2 * sn + o] = v2;
            }
        }
    }
#pragma unroll
    for (int o = 32; o; o >>= 1) r2 = fmaxf(r2, __shfl_xor(r2, o));
    if (lane == 0) red[wv] = r2;
    __syncthreads();
    float R2 = red[0];
#pragma unroll
    for (int w2 = 1; w2 < NW; ++w2) R2 = fmaxf(R2, red[w2]);
    PT(0);
    // 2^-18 R^2: twice the approximation error (24 fp32 accumulations of terms <= 4 R^2 plus the dropped split terms; measured on random
    // tiles: 2^-22.7 R^2, tools/experiments/probe_nn_slots.hip)
#ifndef NN2_ERRC
#define NN2_ERRC 3.814697265625e-06f
#endif
    const float errc = R2 * NN2_ERRC;

    for (int xw = wv; xw < nbp; xw += NW) {         // this wave's source blocks; no workgroup barrier inside
        bf16x8 A[4][2];                            // [tile][instruction]: this lane's eight slots (lane half h) of its source row l31
#pragma unroll
        for (int a = 0; a < 4; ++a) {
            const int o = xw * NN1_XLD + 32 * a + l31;
            const bool lsrc = xw * NN1_XW + 32 * a + l31 < Sp;
            const float x[3] = {lsrc ? sx[o] : 0.f, lsrc ? sx[sn + o] : 0.f, lsrc ? sx[2 * sn + o] : 0.f};
            const float nx = lsrc ? fmaf(x[2], x[2], fmaf(x[1], x[1], x[0] * x[0])) : INFINITY;
            __bf16 sa[32];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                __bf16 p, m, l;
                nn2_split3(x[c], p, m, l);
                sa[6 * c] = p; sa[6 * c + 1] = p; sa[6 * c + 2] = m; sa[6 * c + 3] = p; sa[6 * c + 4] = l; sa[6 * c + 5] = m;
            }
            {
                __bf16 p, m, l;
                nn2_split3(nx, p, m, l);
                sa[18] = p; sa[19] = m; sa[20] = l; sa[21] = (__bf16)1.0f; sa[22] = (__bf16)1.0f; sa[23] = (__bf16)1.0f;
            }
#pragma unroll
            for (int q = 24; q < 32; ++q) sa[q] = (__bf16)0.f;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                A[a][0][e] = h ? sa[8 + e] : sa[e];
                A[a][1][e] = h ? sa[24 + e] : sa[16 + e];
            }
        }
        PT(1);
        f32x16 rmin[4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int r = 0; r < 16; ++r) rmin[a][r] = 3.0e38f;       // (not +inf: a class without a live target must stay finite -- inf | tag would be a NaN --
                                                                     //  and starting the minima there saves the clamp per class in the row stage; same bits)
        float *cp = colp + xw * YCH;
        // Two target tiles x two source tiles per step: every v_min3 then folds TWO fresh distances -- the row minima take one
        // distance of either target tile (same class), the column minima one of either source tile -- 1.0 instead of 1.5 vector
        // instructions per distance (a tile beyond the chunk's last target holds |y|^2 = inf: its distances never win).
        // ORDER (round 6): a software pipeline over the steps s = (jp, ap).  Until round 5 a step was eight MFMAs, 24 wait states, then
        // its 64 v_min3 in a block BEHIND them -- where an in-order wave pays them in full (the two pipes added: ~570 clocks per step and
        // wave).  Vector instructions placed BETWEEN MFMAs ride in their shadow (tools/experiments/micro/coexec2.hip), so each of a
        // step's eight MFMAs is followed by eight v_min3 on accumulators that are already complete:
        //     MFMA         acc0.k0      acc0.k1      acc1.k0      acc1.k1      acc2.k0      acc2.k1      acc3.k0      acc3.k1
        //     gap behind   rows(1,3)'   rows(1,3)'   cols(2,3)'   cols(2,3)'   cols(0,1)    cols(0,1)    rows(0,2)    rows(0,2)
        // (' = the previous step's accumulators, which this step's MFMAs of the same number overwrite only after their gap).  No second
        // accumulator set: four are live, as before.  The first step's "previous" accumulators are +inf (its minima are no-ops), the
        // last step's are drained behind the loop.  Reading acc1 / acc2 one MFMA after their last product needs three more wait states
        // (an 8-pass MFMA's result is readable 11 wait states after issue; its successor occupies 8 of them).  Per accumulator and per
        // minimum the operands are what they were: bit-identical results.
        f32x16 p1, p2, p3;                                           // the previous step's acc1, acc2, acc3
#pragma unroll
        for (int r = 0; r < 16; ++r) { p1[r] = INFINITY; p2[r] = INFINITY; p3[r] = INFINITY; }
        float cm[2][2][4];                                           // [source-tile pair ap][target tile ja / jb][partial] of the CURRENT jp
#pragma unroll
        for (int q = 0; q < 16; ++q) cm[q >> 3][(q >> 2) & 1][q & 3] = INFINITY;
        // Column minima per HALF block (source tiles 0-1 / 2-3), folded into ONE table entry per block and target whose two low
        // mantissa bits say where to look: bit 0 = the half that holds the minimum, bit 1 = the other half lies within the error
        // bound of it (then the whole block is re-scanned, as until round 4; otherwise 64 exact evaluations instead of 128).
        auto col_finish = [&](int jpf) {
#pragma unroll
            for (int jt = 0; jt < 2; ++jt) {
                float c2[2];
#pragma unroll
                for (int ap = 0; ap < 2; ++ap) {
                    const float cmf = vmin(vmin(cm[ap][jt][0], cm[ap][jt][1]), vmin(cm[ap][jt][2], cm[ap][jt][3]));
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(cmf), __float_as_uint(cmf), false, false);
                    const float c = vmin(vmin(__uint_as_float(sw[0]), __uint_as_float(sw[1])), 3.0e38f);      // rows 4h.. of both halves; (inf | tag would be a NaN)
                    c2[ap] = __uint_as_float((__float_as_uint(c) & ~3u) | (unsigned)ap);
                }
                const float m1 = vmin(c2[0], c2[1]), m2 = vmax(c2[0], c2[1]);
                const bool amb = !(m2 > fmaf(fabsf(m1), relc, m1 + errc));
                if (h == 0) cp[64 * jpf + 32 * jt + l31] = __uint_as_float(__float_as_uint(m1) | (amb ? 2u : 0u));
            }
        };
        // eight row minima (elements lo .. lo + 7) / eight steps of a column minimum, pinned between two MFMAs; WAIT: the newer operand's
        // last product is one MFMA back
        auto gap_rows = [&](f32x16 &rm, f32x16 &x, f32x16 &y, int lo, bool wait) {
            __builtin_amdgcn_sched_barrier(0);
            if (wait) asm volatile("s_nop 3" : "+v"(x), "+v"(y));
#pragma unroll
            for (int r = lo; r < lo + 8; ++r) rm[r] = vmin3(rm[r], x[r], y[r]);
            __builtin_amdgcn_sched_barrier(0);
        };
        // (a column minimum is a chain: FOUR rotating partial minima, folded in col_finish -- the minimum of a set does not depend on the
        //  order -- so that an instruction's input is four instructions old: the compiler puts a wait state in front of an inline-asm
        //  reader of a register written less than three instructions earlier)
        // (lo == 0 STARTS the four partials -- a two-operand minimum of the first elements -- so that nobody has to reset them to +inf
        //  behind col_finish: sixteen v_mov per target-tile pair less; a set's lo == 0 call always precedes its lo == 8 call)
        auto gap_cols = [&](float (&c)[4], f32x16 &x, f32x16 &y, int lo, bool wait) {
            __builtin_amdgcn_sched_barrier(0);
            if (wait) asm volatile("s_nop 3" : "+v"(x), "+v"(y));
#pragma unroll
            for (int r = lo; r < lo + 8; ++r) c[r & 3] = (lo == 0 && r < 4) ? vmin(x[r], y[r]) : vmin3(c[r & 3], x[r], y[r]);
            __builtin_amdgcn_sched_barrier(0);
        };
        for (int jp = 0; 2 * jp < ntile; ++jp) {
            const bf16x8 B0a = bop[(2 * jp) * 128 + lane], B1a = bop[(2 * jp) * 128 + 64 + lane];
            const bf16x8 B0b = bop[(2 * jp + 1) * 128 + lane], B1b = bop[(2 * jp + 1) * 128 + 64 + lane];
#pragma unroll
            for (int ap = 0; ap < 2; ++ap) {
                const int pa = ap ^ 1;                               // the previous step's source-tile pair
                f32x16 a0, a1, a2, a3;                               // (a0, ja), (a1, ja), (a0, jb), (a1, jb)
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap][0], B0a, zero16, 0, 0, 0);
                gap_rows(rmin[2 * pa + 1], p1, p3, 0, false);
                a0 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap][1], B1a, a0, 0, 0, 0);
                gap_rows(rmin[2 * pa + 1], p1, p3, 8, false);
                a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap + 1][0], B0a, zero16, 0, 0, 0);
                gap_cols(cm[pa][1], p2, p3, 0, false);
                a1 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap + 1][1], B1a, a1, 0, 0, 0);
                gap_cols(cm[pa][1], p2, p3, 8, false);
                if (ap == 0 && jp > 0) col_finish(jp - 1);           // the previous target-tile pair's column minima are complete
                a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap][0], B0b, zero16, 0, 0, 0);
                gap_cols(cm[ap][0], a0, a1, 0, true);
                a2 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap][1], B1b, a2, 0, 0, 0);
                gap_cols(cm[ap][0], a0, a1, 8, false);
                a3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap + 1][0], B0b, zero16, 0, 0, 0);
                gap_rows(rmin[2 * ap], a0, a2, 0, true);
                a3 = __builtin_amdgcn_mfma_f32_32x32x16_bf16(A[2 * ap + 1][1], B1b, a3, 0, 0, 0);
                gap_rows(rmin[2 * ap], a0, a2, 8, false);
                p1 = a1; p2 = a2; p3 = a3;
            }
        }
        {   // drain: the last step's rows(1,3) and cols(2,3) (its source-tile pair is 1), then the last target-tile pair's column entry
            asm volatile("s_nop 15\n\ts_nop 7" : "+v"(p1), "+v"(p2), "+v"(p3));
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                rmin[3][r] = vmin3(rmin[3][r], p1[r], p3[r]);
                cm[1][1][r & 3] = r < 4 ? vmin(p2[r], p3[r]) : vmin3(cm[1][1][r & 3], p2[r], p3[r]);
            }
            col_finish((ntile - 1) >> 1);
        }
        PT(2);
        // ---- rows: per 32-source tile, class minima -> best class + runner-up -> exact evaluation
#pragma unroll
        for (int a = 0; a < 4; ++a) {
#pragma unroll
            for (int r = 0; r < 16; ++r) scr[mfma_row(r, h) * NN2_TS + l31] = rmin[a][r];
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");                  // wave-private scratch, in-order LDS
            const int rho = lane >> 1, q = lane & 1;                             // two lanes per source: 16 classes each
            float v[16], m1 = INFINITY, m2 = INFINITY;
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                v[k] = __uint_as_float((__float_as_uint(scr[rho * NN2_TS + 16 * q + k]) & ~15u) | (unsigned)k);      // (<= 3.0e38: rmin starts there)
                m2 = vmed3(m1, m2, v[k]);
                m1 = vmin(m1, v[k]);
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const float o1 = dpp_swap1(m1), o2 = dpp_swap1(m2);
            const float n1 = vmin(m1, o1), n2 = vmin(vmax(m1, o1), vmin(m2, o2));
            const bool mine = q == 0 ? m1 <= o1 : m1 < o1;                       // a tie goes to the even lane: both lanes agree
            const int kw = (int)(__float_as_uint(mine ? m1 : o1) & 15u);
            const int cw = 16 * (mine ? q : q ^ 1) + kw;                         // winning class
            const int i = s0 + xw * NN1_XW + 32 * a + rho;                       // global source index
            const int so = xw * NN1_XLD + 32 * a + rho;
            const float q0 = sx[so], q1 = sx[sn + so], q2 = sx[2 * sn + so];     // NaN beyond S
            float e = INFINITY;
            int jb = -1;
#pragma unroll
            for (int jt = NTL - 2; jt >= 0; jt -= 2) {                           // this lane's half of the class, descending
                const int j = 32 * (jt + q) + cw;
                const float dd = nn_exact_d2(q0, q1, q2, lx[j], ly[j], lz[j]);
                if (dd <= e) { e = dd; jb = j; }
            }
            const float thr = fmaf(fabsf(n1), relc, n1 + errc);
            const bool amb = i < S && !(n2 > thr);
            if (__builtin_amdgcn_ballot_w64(amb) != 0) {                         // rare: evaluate every class within the bound
                unsigned cmask = 0;                                              // this lane's candidate classes (of its 16)
#pragma unroll
                for (int k = 0; k < 16; ++k) cmask |= v[k] <= thr ? 1u << k : 0u;
                if (!amb) cmask = 0;
                else if (mine) cmask &= ~(1u << kw);                             // the winning class has been evaluated above
                while (__builtin_amdgcn_ballot_w64(cmask != 0) != 0) {           // every lane takes ITS next candidate: 1-2 rounds
                    const bool has = cmask != 0;
                    const int k = has ? __builtin_ctz(cmask) : 0;
                    cmask &= cmask - 1;
                    // (the class's targets requested together and compared without branches: as a chain of sixteen read - wait - compare
                    //  blocks this path -- taken by a quarter of the tile stages, for one or two lanes -- was half of the row stage: round 6)
                    float tx[NTL], ty[NTL], tz[NTL];
#pragma unroll
                    for (int jt = 0; jt < NTL; ++jt) {
                        const int j = 32 * jt + 16 * q + k;
                        tx[jt] = lx[j]; ty[jt] = ly[j]; tz[jt] = lz[j];
                    }
#pragma unroll
                    for (int jt = NTL - 1; jt >= 0; --jt) {
                        const int j = 32 * jt + 16 * q + k;
                        const float dd = nn_exact_d2(q0, q1, q2, tx[jt], ty[jt], tz[jt]);
                        const bool take = has && (dd < e || (dd == e && j < jb));
                        e = take ? dd : e;
                        jb = take ? j : jb;
                    }
                }
            }
            const float oe = dpp_swap1(e);
            const int oj = dpp_swap1(jb);
            if (oe < e || (oe == e && oj < jb)) { e = oe; jb = oj; }
            if (q == 0 && i < S) {
                NnPart r; r.d2 = e; r.idx = y0 + jb;
                rowpart[i] = r;
            }
        }
        PT(3);
    }
    __syncthreads();
    PT(4);
    // ---- columns: thread t <-> target t.  Blocks whose table entry is within the bound of the pass's best one are re-scanned
    //      exactly, highest block first, candidates descending: the last hit of the smallest distance is the lowest index.  (A source
    //      at the smallest exact distance is always within the bound of the pass's best APPROXIMATE value, so its block is a candidate;
    //      a pass whose best approximate value cannot reach the running exact minimum is skipped.)
    // (Round 6: the target's table entries are read ONCE, all sixteen requested together, and the candidates kept as a bit mask --
    //  until then a fold loop and, per round, a search loop of nbp dependent LDS round trips each: a third of this stage.  The re-scan
    //  takes sixteen sources per step, their 48 LDS reads requested together, instead of four.)
    float ce[NN2_NB_MAX];
#pragma unroll
    for (int k = 0; k < NN2_NB_MAX; ++k) ce[k] = k < nbp ? colp[k * YCH + t] : INFINITY;
    float cb = INFINITY;
#pragma unroll
    for (int k = 0; k < NN2_NB_MAX; ++k) cb = vmin(cb, ce[k]);
    const float thr = fmaf(fabsf(cb), relc, cb + errc);
    const bool may = cb <= fmaf(fabsf(best), relc, best + errc);                   // (best = inf in the first pass: always)
    const float q0 = lx[t], q1 = ly[t], q2 = lz[t];
    unsigned cand = 0;
#pragma unroll
    for (int k = 0; k < NN2_NB_MAX; ++k) cand |= (k < nbp && ce[k] <= thr) ? 1u << k : 0u;
    if (!live || !may) cand = 0;
    while (__builtin_amdgcn_ballot_w64(cand != 0) != 0) {
        const int kn = cand != 0 ? 31 - __builtin_clz(cand) : -1;                  // highest block first; -1: this lane is done
        if (kn >= 0) cand &= ~(1u << kn);
        const unsigned tg = kn >= 0 ? __float_as_uint(colp[kn * YCH + t]) & 3u : 0u;
        const bool both = (tg & 2u) != 0u;                                         // the other half is within the bound: scan both, upper half first
        const float *bx = sx + (kn >= 0 ? kn : 0) * NN1_XLD + ((both || (tg & 1u)) ? NN1_XW / 2 : 0);
        const int k0 = s0 + kn * NN1_XW + ((both || (tg & 1u)) ? NN1_XW / 2 : 0);
        int rl = -1;
#pragma unroll 1
        for (int kb = NN1_XW / 2 - 16; kb >= 0; kb -= 16) {                        // padding beyond the pass's sources is NaN: never <=
            float c0[16], c1[16], c2[16];
#pragma unroll
            for (int u = 0; u < 16; ++u) { c0[u] = bx[kb + u]; c1[u] = bx[sn + kb + u]; c2[u] = bx[2 * sn + kb + u]; }
#pragma unroll
            for (int u = 15; u >= 0; --u) {
                const float dd = nn_exact_d2(c0[u], c1[u], c2[u], q0, q1, q2);
                if (kn >= 0 && dd <= best) { best = dd; rl = kb + u; }
            }
        }
        if (rl >= 0) rr = k0 + rl;
        if (__builtin_amdgcn_ballot_w64(kn >= 0 && both) != 0) {
            const float *bl = bx - NN1_XW / 2;
            rl = -1;
#pragma unroll 1
            for (int kb = NN1_XW / 2 - 16; kb >= 0; kb -= 16) {
                float c0[16], c1[16], c2[16];
#pragma unroll
                for (int u = 0; u < 16; ++u) { c0[u] = bl[kb + u]; c1[u] = bl[sn + kb + u]; c2[u] = bl[2 * sn + kb + u]; }
#pragma unroll
                for (int u = 15; u >= 0; --u) {
                    const float dd = nn_exact_d2(c0[u], c1[u], c2[u], q0, q1, q2);
                    if (kn >= 0 && both && dd <= best) { best = dd; rl = kb + u; }
                }
            }
            if (rl >= 0) rr = k0 - NN1_XW / 2 + rl;
        }
    }
  }   // passes
    if (y0 + t < t_out) {
        if (live) { d2y[y0 + t] = best; idx_y[y0 + t] = rr; }
        else idx_y[y0 + t] = -1;
    }
    PT(5);
    PT_FLUSH(64);
}

// (two workgroups per CU is what the 4-wave LDS carve allows anyway; the 256-register budget also makes the compiler keep the MFMA
//  results in VGPRs -- with AGPR accumulators every element costs an extra v_accvgpr_read per use)
template <int NW>
__device__ __forceinline__ void eng_nn_mx_body(const ndp_engine &e, int parity, float *sm) {
    constexpr int YCH = 64 * NW, NT = 64 * NW;
    int b, bx;                                    // the pair's workgroups on ONE XCD: they all read the pair's sources (xcd_pair_block)
    xcd_pair_block(gridDim.x, gridDim.y, b, bx);
    // (state and geometry requested side by side -- behind the test on the state the geometry was one more global round trip in the
    //  open at the top of every workgroup; only the two scalar fields of the state are read)
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    struct { int level, cur; } st;
    st.level = stp->level; st.cur = stp->cur;
    const ndp_pair_geom gm = e.geom[b];
    // (ONE test on all three requests: the compiler sinks a load below every branch that does not need it, which made the state's level,
    //  the geometry and the state's buffer parity three dependent round trips; cur is 0 or 1)
    if ((st.level >= e.m) | (gm.S == 0) | (st.cur < 0) | (e.w_cd == 0.f)) return;
    const int y0 = bx * YCH;
    int *iy = e.idx_y + (size_t)b * e.t_cap;
    // row partials are indexed by 256-target chunk (nn1_row_chunks); an 8-wave workgroup covers two of them: its partial goes to the
    // first, and the loss stage's fold visits every second slot (nn_row_fold_n, cstep = 2: eng_nn_mx8)
    const int slot = bx * (YCH / NN1_YCH);
    NnPart *rowpart = reinterpret_cast<NnPart *>(e.nn_row) + ((size_t)b * nn1_row_chunks(e.t_cap) + slot) * e.n_cap;
    if (y0 >= gm.T) {                               // keep the -1 padding beyond T
        for (int j = y0 + threadIdx.x; j < min(y0 + YCH, e.t_cap); j += NT) iy[j] = -1;
        return;
    }
    const float *xw = e.pts + ((size_t)b * 2 + (st.cur ^ 1)) * e.n_cap * 3 + 3 * gm.K;
    const float *y = e.tgt + (size_t)b * e.t_cap * 3;
    nn2_body<NW>(xw, gm.S, y, gm.T, y0, e.t_cap, rowpart, e.d2y + (size_t)b * e.t_cap, iy, sm);
}
// 512 targets per workgroup, one 8-wave workgroup per CU (round 4): the engine's kernel of nn_mode 2
extern "C" __global__ void __launch_bounds__(512, 1)
k_eng_nn_mx8(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    eng_nn_mx_body<8>(e, parity, sm);
}

extern "C" __global__ void __launch_bounds__(256, 2)
k_nn2(const float *x, int S, const float *y, int T, int n_cap, float *ws_row, float *d2y, int *idx_y) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int y0 = blockIdx.x * NN1_YCH;
    if (y0 >= T) return;
    nn2_body<4>(x, S, y, T, y0, T, reinterpret_cast<NnPart *>(ws_row) + (size_t)blockIdx.x * n_cap, d2y, idx_y, sm);
}
