// ndp_match.inc -- descriptor matching: row statistics of the never-stored S x T logit matrix on the f32-input MFMA (k_feat_rowstats),
// the 1-D kernels around it (k_feat_neg, k_feat_ot_init, k_feat_ot_update, k_feat_match_finish), and ndp_feat_rowstats /
// ndp_feat_match_workspace / ndp_feat_match, which compose dual-softmax, dustbin optimal transport and mutual nearest neighbours
// from them.  DESIGN.md "Descriptor matching".  fp32 throughout, no atomics, every output element has one writer and every sum one
// fixed order.  All entries are batched: problem b owns the rows offA[b] .. offA[b + 1] of A and offB[b] .. offB[b + 1] of B; the
// entries check the host's copies of both with check_offsets (ndp_abi_common.inc).
// ------------------------------------------------------------------------------------------------
// k_feat_rowstats.  a_ij = alpha * <A_i, B_j> + v_j.  A workgroup (4 waves) owns FM_BM = 32 rows of A and walks the columns in
// tiles of FM_BN = 256; wave w owns the columns 64 w .. 64 w + 63 of a tile as two 32 x 32 accumulators.  The product is taken
// TRANSPOSED, D = B_tile A_block^T (the MFMA's A operand is a row of B, its B operand a row of A): in the 32x32 C/D map the column
// of D lies on the lane (lane & 31) and its rows in the 16 registers, so every lane keeps the running max / sum-exp / argmax of ONE
// row of A over the columns it meets, in registers, with no lane traffic inside the walk.  Products commute and the chain runs over
// ascending k from C = 0 whichever operand is which, so <A_i, B_j> has the same bits with the operands exchanged.
// Both operands pass through LDS in chunks of FM_KC = 32 of k; the next chunk is fetched into registers while the current one is
// multiplied.  An LDS row holds its chunk's even k first, then the odd ones (k at word (k & 1) * 16 + k / 2): the 32x32x2 MFMA wants
// k = 2 kk + (lane >> 5) from a lane, so a lane's sixteen operands of a chunk are contiguous and arrive in four 16-byte reads.  Rows beyond S, columns beyond T and k beyond C are
// zeros in LDS (fma(0, 0, acc) = acc); a column beyond T gets v = -inf, so it adds exp(-inf) = 0 and never wins the max.
// The eight partial results of a row (4 waves x 2 lane halves) are folded in one fixed order at the end, then the dustbin term e[b].
#define FM_BM 32
#define FM_BN 256
#define FM_KC 32
#define FM_LD 36                       // LDS row stride in words: 16-byte aligned rows, 4 words of padding
#define FM_NLOAD ((FM_BM + FM_BN) * FM_KC / 256)
#define FM_MAX_C 1056
#define FM_MODE_DUAL_SOFTMAX 0
#define FM_MODE_SINKHORN 1
#define FM_MODE_MUTUAL_NN 2

// One chunk of both operands, global memory -> registers.  VEC (C a multiple of 4, 16-byte aligned operands): a thread loads nine
// float4, row e * 32 + t / 8, k = 4 (t & 7) ..; otherwise 36 floats, row e * 8 + t / 32, k = t & 31.  fm_stage writes them to LDS.
template <bool VEC>
__device__ __forceinline__ void fm_fetch(float (&pre)[FM_NLOAD], float &pv, const float *A, const float *Bm, const float *v, int C, int S, int T,
                                         int r0, int jt, int kc) {
    const int t = threadIdx.x;
    if (VEC) {
        const int k = kc * FM_KC + 4 * (t & 7), rr = t >> 3;
        const bool kin = k < C;
#pragma unroll
        for (int e = 0; e < FM_NLOAD / 4; ++e) {
            float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
            if (e == 0) {
                const int gi = r0 + rr;
                if (kin && gi < S) q = *reinterpret_cast<const float4 *>(A + (size_t)gi * C + k);
            } else {
                const int gj = jt * FM_BN + (e - 1) * 32 + rr;
                if (kin && gj < T) q = *reinterpret_cast<const float4 *>(Bm + (size_t)gj * C + k);
            }
            pre[4 * e] = q.x; pre[4 * e + 1] = q.y; pre[4 * e + 2] = q.z; pre[4 * e + 3] = q.w;
        }
    } else {
        const int k = kc * FM_KC + (t & 31), rr = t >> 5;
        const bool kin = k < C;
#pragma unroll
        for (int e = 0; e < FM_NLOAD; ++e) {
            const int row = e * 8 + rr;                          // 0 .. 31: the block's rows of A; 32 .. 287: the tile's rows of B
            if (e < FM_BM / 8) {
                const int gi = r0 + row;
                pre[e] = (kin && gi < S) ? A[(size_t)gi * C + k] : 0.f;
            } else {
                const int gj = jt * FM_BN + row - FM_BM;
                pre[e] = (kin && gj < T) ? Bm[(size_t)gj * C + k] : 0.f;
            }
        }
    }
    if (kc == 0) {
        const int gj = jt * FM_BN + t;
        pv = gj < T ? (v ? v[gj] : 0.f) : -INFINITY;
    }
}

template <bool VEC>
__device__ __forceinline__ void fm_stage(const float (&pre)[FM_NLOAD], float *sm) {
    const int t = threadIdx.x;
    if (VEC) {                                                   // k = 4 kq .. 4 kq + 3: the even pair to word 2 kq, the odd pair to 16 + 2 kq
#pragma unroll
        for (int e = 0; e < FM_NLOAD / 4; ++e) {
            float *row = sm + (e * 32 + (t >> 3)) * FM_LD + 2 * (t & 7);
            *reinterpret_cast<float2 *>(row) = make_float2(pre[4 * e], pre[4 * e + 2]);
            *reinterpret_cast<float2 *>(row + 16) = make_float2(pre[4 * e + 1], pre[4 * e + 3]);
        }
    } else {
        const int k = t & 31, pos = (k & 1) * 16 + (k >> 1);
#pragma unroll
        for (int q = 0; q < FM_NLOAD; ++q) sm[(q * 8 + (t >> 5)) * FM_LD + pos] = pre[q];
    }
}

template <bool VEC>
__device__ __forceinline__ void feat_rowstats_body(const float *A, const float *Bm, const int *offA, const int *offB, int C, float alpha,
                                                   const float *v, const float *e, float *lse, float *mx, int *arg) {
    __shared__ __attribute__((aligned(16))) float sm[(FM_BM + FM_BN) * FM_LD];
    __shared__ float sv[FM_BN];
    const int t = threadIdx.x, b = blockIdx.y;
    const int a0 = offA[b], S = offA[b + 1] - a0, b0 = offB[b], T = offB[b + 1] - b0;
    const int r0 = blockIdx.x * FM_BM;
    if (r0 >= S) return;                                         // (uniform: the grid is sized by the largest problem)
    A += (size_t)a0 * C; Bm += (size_t)b0 * C;
    if (v) v += b0;
    const int lane = t & 63, w = t >> 6, li = lane & 31, h = lane >> 5;
    const int n_kc = (C + FM_KC - 1) / FM_KC, n_jt = (T + FM_BN - 1) / FM_BN, total = n_kc * n_jt;
    const float4 *pi = reinterpret_cast<const float4 *>(sm + li * FM_LD + 16 * h);
    const float4 *pj0 = reinterpret_cast<const float4 *>(sm + (FM_BM + w * 64 + li) * FM_LD + 16 * h), *pj1 = pj0 + 32 * FM_LD / 4;
    float pre[FM_NLOAD], pv = 0.f;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    float m = -INFINITY, s = 0.f, bm = -INFINITY;                // this lane's row over the columns it has met
    int bj = 0x7fffffff;
    fm_fetch<VEC>(pre, pv, A, Bm, v, C, S, T, r0, 0, 0);
    int jt = 0, kc = 0;
    for (int it = 0; it < total; ++it) {
        fm_stage<VEC>(pre, sm);
        if (kc == 0) sv[t] = pv;
        __syncthreads();
        int jn = jt, kn = kc + 1;
        if (kn == n_kc) { kn = 0; ++jn; }
        if (it + 1 < total) fm_fetch<VEC>(pre, pv, A, Bm, v, C, S, T, r0, jn, kn);
        const int kp = (min(FM_KC, C - kc * FM_KC) + 1) >> 1;    // k pairs of this chunk; beyond them LDS holds zeros: fma(0, 0, acc) = acc
#pragma unroll
        for (int q = 0; q < 4; ++q) {                            // four pairs a step, ascending k
            if (4 * q < kp) {
                const float4 bi = pi[q], a0q = pj0[q], a1q = pj1[q];
                acc0 = MFMA32(a0q.x, bi.x, acc0); acc1 = MFMA32(a1q.x, bi.x, acc1);
                acc0 = MFMA32(a0q.y, bi.y, acc0); acc1 = MFMA32(a1q.y, bi.y, acc1);
                acc0 = MFMA32(a0q.z, bi.z, acc0); acc1 = MFMA32(a1q.z, bi.z, acc1);
                acc0 = MFMA32(a0q.w, bi.w, acc0); acc1 = MFMA32(a1q.w, bi.w, acc1);
            }
        }
        if (kn == 0) {                                           // the tile's last chunk: its 32 logits of this lane's row
            float x[32];
            float tm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 32; ++r) {
                const int jl = w * 64 + (r >> 4) * 32 + (r & 3) + 8 * ((r & 15) >> 2) + 4 * h;
                const float a = alpha * (r < 16 ? acc0[r & 15] : acc1[r & 15]) + sv[jl];
                x[r] = a;
                tm = fmaxf(tm, a);
                if (a > bm) { bm = a; bj = jt * FM_BN + jl; }   // ascending columns: the lowest index among equals stays
            }
            if (tm > m) { s *= expf(m - tm); m = tm; }
            if (m > -INFINITY) {
#pragma unroll
                for (int r = 0; r < 32; ++r) s += expf(x[r] - m);
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
        }
        jt = jn; kc = kn;
        __syncthreads();
    }
    float *cm = sm, *cs = sm + 256, *cb = sm + 512;              // [8][32] each: part p = 2 w + h of row li
    int *cj = reinterpret_cast<int *>(sm + 768);
    const int p = 2 * w + h;
    cm[p * 32 + li] = m; cs[p * 32 + li] = s; cb[p * 32 + li] = bm; cj[p * 32 + li] = bj;
    __syncthreads();
    if (t >= FM_BM || r0 + t >= S) return;
    float M = -INFINITY;
    for (int q = 0; q < 8; ++q) M = fmaxf(M, cm[q * 32 + t]);
    float sum = 0.f;
    bm = -INFINITY; bj = 0x7fffffff;
    for (int q = 0; q < 8; ++q) {
        const float mq = cm[q * 32 + t];
        if (mq > -INFINITY) sum += cs[q * 32 + t] * expf(mq - M);
        const float aq = cb[q * 32 + t];
        const int jq = cj[q * 32 + t];
        if (aq > bm || (aq == bm && jq < bj)) { bm = aq; bj = jq; }
    }
    if (e) {
        const float eb = e[b], M2 = fmaxf(M, eb);
        sum = sum * expf(M - M2) + expf(eb - M2);
        M = M2;
    }
    const size_t o = (size_t)a0 + r0 + t;
    if (lse) lse[o] = M + logf(sum);
    if (mx) mx[o] = bm;
    if (arg) arg[o] = bj;
}

extern "C" __global__ void __launch_bounds__(256)
k_feat_rowstats(const float *A, const float *Bm, const int *offA, const int *offB, int C, float alpha, const float *v, const float *e,
                float *lse, float *mx, int *arg) {
    feat_rowstats_body<false>(A, Bm, offA, offB, C, alpha, v, e, lse, mx, arg);
}

// the same kernel with 16-byte loads: C a multiple of 4 and both operands 16-byte aligned (every row then is); the same bits
extern "C" __global__ void __launch_bounds__(256)
k_feat_rowstats_v4(const float *A, const float *Bm, const int *offA, const int *offB, int C, float alpha, const float *v, const float *e,
                   float *lse, float *mx, int *arg) {
    feat_rowstats_body<true>(A, Bm, offA, offB, C, alpha, v, e, lse, mx, arg);
}

// ------------------------------------------------------------------------------------------------
// 1-D kernels.  fm_block_lse: log-sum-exp of x[0 .. n) and one extra term by a 256-thread workgroup, a thread's share in ascending
// order, the shares folded by block_fold's tree (ndp_device.h); every thread receives the result.  scratch [256].
__device__ __forceinline__ float fm_block_lse(const float *x, int n, float extra, float *scratch) {
    const int t = threadIdx.x;
    float mm = t == 0 ? extra : -INFINITY;
    for (int i = t; i < n; i += 256) mm = fmaxf(mm, x[i]);
    const float M = block_fold_one(mm, scratch, FoldMax());
    float ss = t == 0 ? expf(extra - M) : 0.f;
    for (int i = t; i < n; i += 256) ss += expf(x[i] - M);
    return M + logf(block_fold_one(ss, scratch, FoldSum()));
}

extern "C" __global__ void __launch_bounds__(256) k_feat_neg(float *x, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = -x[i];
}

// u = v = 0 (the dustbin entries included); eu = ev = bin_score + 0: the dustbin column value the first row-statistics pass adds
extern "C" __global__ void __launch_bounds__(256)
k_feat_ot_init(float *u, int nS, float *v, int nT, float *ubin, float *vbin, float *eu, float *ev, int B, float bin) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < nS) u[i] = 0.f;
    if (i < nT) v[i] = 0.f;
    if (i < B) { ubin[i] = 0.f; vbin[i] = 0.f; eu[i] = bin; ev[i] = bin; }
}

// One Sinkhorn half step of log_optimal_transport (matching.py:24-32) for side X against side Y, one workgroup per problem:
//   potX_i = norm - lseX_i,  lseX_i = LSE_j(Z_ij + potY_j) with the dustbin column already folded in by k_feat_rowstats (e = eY);
//   potbinX = log nY + norm - (bin + LSE(potY_0 .. potY_{nY - 1}, potbinY))   -- the dustbin row of X: every Z entry is bin;
//   eX = bin + potbinX, the dustbin term of the NEXT row-statistics pass (rows Y, columns X).        norm = -log(nX + nY).
extern "C" __global__ void __launch_bounds__(256)
k_feat_ot_update(const float *lseX, float *potX, const int *offX, const float *potY, const int *offY, const float *potbinY, float *potbinX,
                 float *eX, float bin) {
    __shared__ float scratch[256];
    const int t = threadIdx.x, b = blockIdx.x;
    const int x0 = offX[b], nX = offX[b + 1] - x0, y0 = offY[b], nY = offY[b + 1] - y0;
    const float norm = -logf((float)(nX + nY));
    for (int i = t; i < nX; i += 256) potX[x0 + i] = norm - lseX[x0 + i];
    const float L = fm_block_lse(potY + y0, nY, potbinY[b], scratch);
    if (t == 0) {
        const float pb = (logf((float)nY) + norm) - (bin + L);
        potbinX[b] = pb;
        eX[b] = bin + pb;
    }
}

// Per source row i: j = arg_row[i]; conf = exp(max_row + add) (dual-softmax: add = -lse_row), exp((max_row + add) - norm) (sinkhorn:
// add = u, norm = -log(S + T)) or max_row itself (mutual_nn).  match_t = j when conf > thr and (mutual: arg_col[j] == i), else -1.
// A j outside the problem (a row of NaNs has no maximum) never matches and is never used as an index.
extern "C" __global__ void __launch_bounds__(256)
k_feat_match_finish(int mode, const float *max_row, const float *add, const int *arg_row, const int *arg_col, const int *offS, const int *offT,
                    float thr, int mutual, int *match_t, float *conf) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int s0 = offS[b], S = offS[b + 1] - s0, t0 = offT[b], T = offT[b + 1] - t0;
    if (i >= S) return;
    const int j = arg_row[s0 + i];
    float c = max_row[s0 + i];
    if (mode == FM_MODE_DUAL_SOFTMAX) c = expf(c + add[s0 + i]);
    else if (mode == FM_MODE_SINKHORN) c = expf((c + add[s0 + i]) + logf((float)(S + T)));
    bool ok = (unsigned)j < (unsigned)T && c > thr;
    if (ok && mutual) ok = arg_col[t0 + j] == i;
    match_t[s0 + i] = ok ? j : -1;
    conf[s0 + i] = c;
}

// ------------------------------------------------------------------------------------------------
// host entries
// ------------------------------------------------------------------------------------------------
struct FmShape {
    long long nA, nB;
    int maxA, maxB;
};

static int fm_check(const char *who, const int *offA_host, const int *offB_host, int B, int C, FmShape *sh) {
    if (int rc = check_batch(who, offA_host && offB_host ? offA_host : nullptr, B)) return rc;      // B, both pointers, C, then the contents
    if (C < 1 || C > FM_MAX_C) return failf(NDP_E_INVALID, "%s: C must lie in 1..%d", who, FM_MAX_C);
    if (int rc = check_offsets(who, offA_host, B, 1, "a non-empty side, S and T", &sh->maxA)) return rc;
    if (int rc = check_offsets(who, offB_host, B, 1, "a non-empty side, S and T", &sh->maxB)) return rc;
    sh->nA = offA_host[B]; sh->nB = offB_host[B];
    return 0;
}

static bool fm_aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }

static int fm_rowstats_launch(const float *A, const float *Bm, const int *offA, const int *offB, int maxA, int B, int C, float alpha,
                              const float *v, const float *e, float *lse, float *mx, int *arg, hipStream_t s) {
    const dim3 grid((maxA + FM_BM - 1) / FM_BM, B);
    if (C % 4 == 0 && aligned16(A) && aligned16(Bm))
        hipLaunchKernelGGL(k_feat_rowstats_v4, grid, dim3(256), 0, s, A, Bm, offA, offB, C, alpha, v, e, lse, mx, arg);
    else
        hipLaunchKernelGGL(k_feat_rowstats, grid, dim3(256), 0, s, A, Bm, offA, offB, C, alpha, v, e, lse, mx, arg);
    HIP_TRY(hipGetLastError(), "k_feat_rowstats launch");
    return 0;
}

extern "C" int ndp_feat_rowstats(const float *A, const float *Bm, const int *offA, const int *offB, const int *offA_host, const int *offB_host,
                                 int B, int C, float alpha, const float *v, const float *e, float *lse, float *mx, int *arg, void *stream) {
    FmShape sh;
    if (int rc = fm_check("ndp_feat_rowstats", offA_host, offB_host, B, C, &sh)) return rc;
    if (!A || !Bm || !offA || !offB || (!lse && !mx && !arg)) return fail(NDP_E_INVALID, "ndp_feat_rowstats: null pointer");
    if (!fm_aligned4(A) || !fm_aligned4(Bm) || !fm_aligned4(offA) || !fm_aligned4(offB) || !fm_aligned4(v) || !fm_aligned4(e) ||
        !fm_aligned4(lse) || !fm_aligned4(mx) || !fm_aligned4(arg))
        return fail(NDP_E_INVALID, "ndp_feat_rowstats: pointers must be 4-byte aligned");
    if (!std::isfinite(alpha)) return fail(NDP_E_INVALID, "ndp_feat_rowstats: alpha must be finite");
    return fm_rowstats_launch(A, Bm, offA, offB, sh.maxA, B, C, alpha, v, e, lse, mx, arg, (hipStream_t)stream);
}

// words (4 bytes): per source row f0, f1, arg; per target row g0, g1, arg; per problem ubin, vbin, eu, ev
extern "C" int ndp_feat_match_workspace(int B, long long nS, long long nT, long long *nbytes) {
    if (B < 1 || B > NDP_MAX_B || nS < 1 || nT < 1 || nS > 0x7fffffffLL || nT > 0x7fffffffLL || !nbytes)
        return fail(NDP_E_INVALID, "ndp_feat_match_workspace: B in 1..65535, 1 <= nS, nT < 2^31, nbytes not NULL");
    *nbytes = 4 * (3 * (nS + nT) + 4 * (long long)B);
    return 0;
}

extern "C" int ndp_feat_match(const float *fs, const float *ft, const int *offS, const int *offT, const int *offS_host, const int *offT_host,
                              int B, int C, int mode, float temperature, float bin_score, int iters, float thr, int mutual, void *ws,
                              int *match_t, float *conf, void *stream) {
    FmShape sh;
    if (int rc = fm_check("ndp_feat_match", offS_host, offT_host, B, C, &sh)) return rc;
    if (mode < FM_MODE_DUAL_SOFTMAX || mode > FM_MODE_MUTUAL_NN)
        return fail(NDP_E_INVALID, "ndp_feat_match: mode must be 0 (dual_softmax), 1 (sinkhorn) or 2 (mutual_nn)");
    if (mode != FM_MODE_SINKHORN && (!(temperature > 0.f) || !std::isfinite(temperature)))
        return fail(NDP_E_INVALID, "ndp_feat_match: temperature (mutual_nn: alpha) must be positive and finite");
    if (mode == FM_MODE_SINKHORN && !std::isfinite(bin_score)) return fail(NDP_E_INVALID, "ndp_feat_match: bin_score must be finite");
    if (iters < 0) return fail(NDP_E_INVALID, "ndp_feat_match: iters >= 0");
    if (thr != thr) return fail(NDP_E_INVALID, "ndp_feat_match: thr must not be NaN");
    if (!fs || !ft || !offS || !offT || !ws || !match_t || !conf) return fail(NDP_E_INVALID, "ndp_feat_match: null pointer");
    if (!fm_aligned4(fs) || !fm_aligned4(ft) || !fm_aligned4(offS) || !fm_aligned4(offT) || !fm_aligned4(ws) || !fm_aligned4(match_t) ||
        !fm_aligned4(conf))
        return fail(NDP_E_INVALID, "ndp_feat_match: pointers and the workspace must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const long long nS = sh.nA, nT = sh.nB;
    float *f0 = (float *)ws, *f1 = f0 + nS;
    int *ar = (int *)(f1 + nS);
    float *g0 = (float *)(ar + nS), *g1 = g0 + nT;
    int *ac = (int *)(g1 + nT);
    float *ubin = (float *)(ac + nT), *vbin = ubin + B, *eu = vbin + B, *ev = eu + B;
    const float *none = nullptr;
    float *no_out = nullptr;
    int *no_arg = nullptr;
#define FM_ROWS(alpha, v, e, lse, mx, arg)                                                                                      \
    if (int rc = fm_rowstats_launch(fs, ft, offS, offT, sh.maxA, B, C, alpha, v, e, lse, mx, arg, s)) return rc
#define FM_COLS(alpha, v, e, lse, mx, arg)                                                                                      \
    if (int rc = fm_rowstats_launch(ft, fs, offT, offS, sh.maxB, B, C, alpha, v, e, lse, mx, arg, s)) return rc
    if (mode == FM_MODE_DUAL_SOFTMAX) {
        const float alpha = 1.f / ((float)C * temperature);
        FM_ROWS(alpha, none, none, f0, no_out, no_arg);         // pass 1: lse_row, lse_col
        FM_COLS(alpha, none, none, g0, no_out, no_arg);
        hipLaunchKernelGGL(k_feat_neg, dim3((unsigned)((nS + 255) / 256)), dim3(256), 0, s, f0, (int)nS);
        hipLaunchKernelGGL(k_feat_neg, dim3((unsigned)((nT + 255) / 256)), dim3(256), 0, s, g0, (int)nT);
        HIP_TRY(hipGetLastError(), "k_feat_neg launch");
        FM_ROWS(2.f * alpha, (const float *)g0, none, no_out, f1, ar);       // pass 2: max_j (2 s_ij - lse_col_j), max_i (2 s_ij - lse_row_i)
        if (mutual) FM_COLS(2.f * alpha, (const float *)f0, none, no_out, g1, ac);
    } else if (mode == FM_MODE_SINKHORN) {
        const float alpha = 1.f / (float)C;
        const long long nmax = std::max(std::max(nS, nT), (long long)B);
        hipLaunchKernelGGL(k_feat_ot_init, dim3((unsigned)((nmax + 255) / 256)), dim3(256), 0, s, f0, (int)nS, g0, (int)nT, ubin, vbin, eu, ev, B, bin_score);
        HIP_TRY(hipGetLastError(), "k_feat_ot_init launch");
        for (int it = 0; it < iters; ++it) {                    // u = f0, v = g0
            FM_ROWS(alpha, (const float *)g0, (const float *)ev, f1, no_out, no_arg);
            hipLaunchKernelGGL(k_feat_ot_update, dim3(B), dim3(256), 0, s, (const float *)f1, f0, offS, (const float *)g0, offT, (const float *)vbin, ubin, eu, bin_score);
            FM_COLS(alpha, (const float *)f0, (const float *)eu, g1, no_out, ac);      // its argmax is the final one: u does not change again
            hipLaunchKernelGGL(k_feat_ot_update, dim3(B), dim3(256), 0, s, (const float *)g1, g0, offT, (const float *)f0, offS, (const float *)ubin, vbin, ev, bin_score);
            HIP_TRY(hipGetLastError(), "k_feat_ot_update launch");
        }
        FM_ROWS(alpha, (const float *)g0, none, no_out, f1, ar);
        if (mutual && iters == 0) FM_COLS(alpha, (const float *)f0, none, no_out, g1, ac);
    } else {
        FM_ROWS(temperature, none, none, no_out, f1, ar);
        if (mutual) FM_COLS(temperature, none, none, no_out, g1, ac);
    }
#undef FM_ROWS
#undef FM_COLS
    hipLaunchKernelGGL(k_feat_match_finish, dim3((sh.maxA + 255) / 256, B), dim3(256), 0, s, mode, (const float *)f1, (const float *)f0,
                       (const int *)ar, (const int *)ac, offS, offT, thr, mutual, match_t, conf);
    HIP_TRY(hipGetLastError(), "k_feat_match_finish launch");
    return 0;
}

// ------------------------------------------------------------------------------------------------
// The dense dual-softmax confidence matrix (ABI 215), for the callers that need the matrix itself: Lepard's soft-Procrustes layer and
// its conf_matrix_pred.  conf[b, i, j] = exp(a_ij - lse_row_i) exp(a_ij - lse_col_j), a_ij = <fs_i, ft_j> / (C temperature), into
// [B, Smax, Tmax]; everything outside a problem's S x T is exactly 0, what the reference's masked soft-maxes give its padding.
// lse_row / lse_col come from two launches of k_feat_rowstats.  k_feat_conf walks the matrix as k_feat_rowstats does -- the same
// staging (fm_fetch / fm_stage), the same MFMA chain over ascending k, a_ij = alpha * acc -- so a logit has the bits both statistics
// passes saw; where that kernel folds a tile's 32 logits of a lane's row into its statistics, this one writes their confidences.
// The grid covers Smax rows: a block beyond the problem's rows only writes zeros.
template <bool VEC>
__device__ __forceinline__ void feat_conf_body(const float *A, const float *Bm, const int *offA, const int *offB, int C, float alpha,
                                               const float *lse_r, const float *lse_c, float *conf, int Smax, int Tmax) {
    __shared__ __attribute__((aligned(16))) float sm[(FM_BM + FM_BN) * FM_LD];
    __shared__ float sv[FM_BN];
    const int t = threadIdx.x, b = blockIdx.y;
    const int a0 = offA[b], S = offA[b + 1] - a0, b0 = offB[b], T = offB[b + 1] - b0;
    const int r0 = blockIdx.x * FM_BM;
    conf += (size_t)b * Smax * Tmax;
    if (r0 >= S) {                                               // (uniform) padding rows
        const int nr = min(FM_BM, Smax - r0);
        for (int i = 0; i < nr; ++i)
            for (int j = t; j < Tmax; j += 256) conf[(size_t)(r0 + i) * Tmax + j] = 0.f;
        return;
    }
    A += (size_t)a0 * C; Bm += (size_t)b0 * C;
    lse_r += a0; lse_c += b0;
    const int lane = t & 63, w = t >> 6, li = lane & 31, h = lane >> 5;
    const int n_kc = (C + FM_KC - 1) / FM_KC, n_jt = (T + FM_BN - 1) / FM_BN, total = n_kc * n_jt;
    const float4 *pi = reinterpret_cast<const float4 *>(sm + li * FM_LD + 16 * h);
    const float4 *pj0 = reinterpret_cast<const float4 *>(sm + (FM_BM + w * 64 + li) * FM_LD + 16 * h), *pj1 = pj0 + 32 * FM_LD / 4;
    float pre[FM_NLOAD], pv = 0.f;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
    const int gi = r0 + li;
    const float lr = gi < S ? lse_r[gi] : 0.f;
    float *crow = conf + (size_t)gi * Tmax;
    fm_fetch<VEC>(pre, pv, A, Bm, lse_c, C, S, T, r0, 0, 0);     // v = lse_col: sv holds the tile's column statistics (-inf beyond T)
    int jt = 0, kc = 0;
    for (int it = 0; it < total; ++it) {
        fm_stage<VEC>(pre, sm);
        if (kc == 0) sv[t] = pv;
        __syncthreads();
        int jn = jt, kn = kc + 1;
        if (kn == n_kc) { kn = 0; ++jn; }
        if (it + 1 < total) fm_fetch<VEC>(pre, pv, A, Bm, lse_c, C, S, T, r0, jn, kn);
        const int kp = (min(FM_KC, C - kc * FM_KC) + 1) >> 1;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            if (4 * q < kp) {
                const float4 bi = pi[q], a0q = pj0[q], a1q = pj1[q];
                acc0 = MFMA32(a0q.x, bi.x, acc0); acc1 = MFMA32(a1q.x, bi.x, acc1);
                acc0 = MFMA32(a0q.y, bi.y, acc0); acc1 = MFMA32(a1q.y, bi.y, acc1);
                acc0 = MFMA32(a0q.z, bi.z, acc0); acc1 = MFMA32(a1q.z, bi.z, acc1);
                acc0 = MFMA32(a0q.w, bi.w, acc0); acc1 = MFMA32(a1q.w, bi.w, acc1);
            }
        }
        if (kn == 0) {                                           // the tile's last chunk: the 32 confidences of this lane's row
            if (gi < Smax) {
#pragma unroll
                for (int r = 0; r < 32; ++r) {
                    const int jl = w * 64 + (r >> 4) * 32 + (r & 3) + 8 * ((r & 15) >> 2) + 4 * h, j = jt * FM_BN + jl;
                    const float a = alpha * (r < 16 ? acc0[r & 15] : acc1[r & 15]);
                    if (j < Tmax) crow[j] = (gi < S && j < T) ? expf(a - lr) * expf(a - sv[jl]) : 0.f;
                }
            }
#pragma unroll
            for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
        }
        jt = jn; kc = kn;
        __syncthreads();
    }
    const int nr = min(FM_BM, Smax - r0);                        // the columns behind the last tile
    for (int i = 0; i < nr; ++i)
        for (int j = n_jt * FM_BN + t; j < Tmax; j += 256) conf[(size_t)(r0 + i) * Tmax + j] = 0.f;
}

extern "C" __global__ void __launch_bounds__(256)
k_feat_conf(const float *A, const float *Bm, const int *offA, const int *offB, int C, float alpha, const float *lse_r, const float *lse_c,
            float *conf, int Smax, int Tmax) {
    feat_conf_body<false>(A, Bm, offA, offB, C, alpha, lse_r, lse_c, conf, Smax, Tmax);
}

extern "C" __global__ void __launch_bounds__(256)
k_feat_conf_v4(const float *A, const float *Bm, const int *offA, const int *offB, int C, float alpha, const float *lse_r, const float *lse_c,
               float *conf, int Smax, int Tmax) {
    feat_conf_body<true>(A, Bm, offA, offB, C, alpha, lse_r, lse_c, conf, Smax, Tmax);
}

// floats: lse_row [nS], lse_col [nT]
extern "C" int ndp_feat_conf_workspace(int B, long long nS, long long nT, long long *nbytes) {
    if (B < 1 || B > NDP_MAX_B || nS < 1 || nT < 1 || nS > 0x7fffffffLL || nT > 0x7fffffffLL || !nbytes)
        return fail(NDP_E_INVALID, "ndp_feat_conf_workspace: B in 1..65535, 1 <= nS, nT < 2^31, nbytes not NULL");
    *nbytes = 4 * (nS + nT);
    return 0;
}

extern "C" int ndp_feat_conf(const float *fs, const float *ft, const int *offS, const int *offT, const int *offS_host, const int *offT_host,
                             int B, int C, float temperature, void *ws, float *conf, int Smax, int Tmax, void *stream) {
    FmShape sh;
    if (int rc = fm_check("ndp_feat_conf", offS_host, offT_host, B, C, &sh)) return rc;
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(NDP_E_INVALID, "ndp_feat_conf: temperature must be positive and finite");
    if (Smax < sh.maxA || Tmax < sh.maxB)
        return failf(NDP_E_INVALID, "ndp_feat_conf: conf is [B, Smax, Tmax] with Smax >= %d and Tmax >= %d, the largest problem", sh.maxA, sh.maxB);
    if (!fs || !ft || !offS || !offT || !ws || !conf) return fail(NDP_E_INVALID, "ndp_feat_conf: null pointer");
    if (!fm_aligned4(fs) || !fm_aligned4(ft) || !fm_aligned4(offS) || !fm_aligned4(offT) || !fm_aligned4(ws) || !fm_aligned4(conf))
        return fail(NDP_E_INVALID, "ndp_feat_conf: pointers and the workspace must be 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    float *lr = (float *)ws, *lc = lr + sh.nA;
    const float alpha = 1.f / ((float)C * temperature);          // ndp_feat_match's
    if (int rc = fm_rowstats_launch(fs, ft, offS, offT, sh.maxA, B, C, alpha, nullptr, nullptr, lr, nullptr, nullptr, s)) return rc;
    if (int rc = fm_rowstats_launch(ft, fs, offT, offS, sh.maxB, B, C, alpha, nullptr, nullptr, lc, nullptr, nullptr, s)) return rc;
    const dim3 grid((Smax + FM_BM - 1) / FM_BM, B);
    if (C % 4 == 0 && aligned16(fs) && aligned16(ft))
        hipLaunchKernelGGL(k_feat_conf_v4, grid, dim3(256), 0, s, fs, ft, offS, offT, C, alpha, (const float *)lr, (const float *)lc, conf, Smax, Tmax);
    else
        hipLaunchKernelGGL(k_feat_conf, grid, dim3(256), 0, s, fs, ft, offS, offT, C, alpha, (const float *)lr, (const float *)lc, conf, Smax, Tmax);
    HIP_TRY(hipGetLastError(), "k_feat_conf launch");
    return 0;
}
