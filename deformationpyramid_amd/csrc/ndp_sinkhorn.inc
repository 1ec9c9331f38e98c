// ndp_sinkhorn.inc -- Sinkhorn divergence baseline (optimal-transport registration): the streamed soft-minimum kernels, the fixed-order
// loss reduce, and ndp_sinkhorn_schedule / ndp_sinkhorn_workspace / ndp_sinkhorn_divergence.  DESIGN.md "Sinkhorn baseline".
// ------------------------------------------------------------------------------------------------
// softmin(eps, U, V, h)_i = -eps log sum_j exp(h_j - |U_i - V_j|^2 / (2 eps)),   h_j = log w + pot_j / eps,   w = 1 / #V
//
// With u_ij = pot_j - |U_i - V_j|^2 / 2 the sum is  w exp(M_i / eps) S_i,  M_i = max_j u_ij,  S_i = sum_j exp2((u_ij - M_i) k),
// k = log2(e) / eps, so  softmin_i = -M_i - eps (log w + ln S_i).  The maximum is taken on u (values of order one), not on the
// exponent argument (up to 1e4 at blur 0.01): the difference u - M is formed before the multiplication by k, which keeps its
// rounding error relative.  The N x M matrix is never stored: columns stream through LDS in tiles, every row keeps (M, S) and, in
// the final kernel, the three weighted sums  sum_j exp2(..) (U_i - V_j)  under the same rescale.
//
// Shape: a workgroup of 256 threads owns SK_ROWS = 16 rows; the SK_SPLIT = 16 lanes of a row (consecutive lanes of one wave) take
// the columns j = c (mod 16) of every tile and merge their (M, S) by a four-round xor butterfly -- a fixed tree, and both partners
// of a round form the same two products, so every lane ends with the same bits.  2000 rows give 125 workgroups per softmin.
// No atomics: every output element has one writer and the loss is folded in a fixed order.
#define SK_ROWS 16
#define SK_SPLIT 16
#define SK_TILE 1024                   // columns staged per pass: 16 KiB of (x, y, z, pot) records
#define SK_CHUNK 8                     // columns per lane between two rescales
#define SK_MAX_EPS 256                 // longest epsilon schedule ndp_sinkhorn_divergence accepts
#define SK_EMPTY (-3.402823466e38f)    // running maximum of a lane that has seen no column (finite: never inf - inf)

struct SkAcc { float M, S, ax, ay, az; };

__device__ __forceinline__ float sk_exp2(float v) { return __builtin_amdgcn_exp2f(v); }     // v <= 0 here; exp2(-inf) = 0

// One row's soft-minimum statistics over all ncols columns, for the row point (px, py, pz) of this thread; every thread of the
// workgroup must call it (it stages tiles and shuffles).  colpot == nullptr: all potentials zero.  The 16 lanes of a row return
// the same merged accumulator.
template <bool GRAD>
__device__ __forceinline__ SkAcc sk_softmin(const float *cols, int ncols, const float *colpot, float k, float px, float py, float pz,
                                            float4 *tile) {
    const int t = threadIdx.x, c = t & (SK_SPLIT - 1);
    SkAcc a = {SK_EMPTY, 0.f, 0.f, 0.f, 0.f};
    for (int base = 0; base < ncols; base += SK_TILE) {
        const int cnt = ncols - base < SK_TILE ? ncols - base : SK_TILE;
        const int nq = (cnt + SK_SPLIT * SK_CHUNK - 1) / (SK_SPLIT * SK_CHUNK);           // chunks holding a live column (<= 8)
        __syncthreads();                                                                    // the previous tile is read out
        for (int j = t; j < nq * SK_SPLIT * SK_CHUNK; j += 256) {
            const size_t g = (size_t)base + j;
            float4 r = make_float4(0.f, 0.f, 0.f, -INFINITY);                               // padding: weight exp2(-inf) = 0
            if (j < cnt) r = make_float4(cols[3 * g], cols[3 * g + 1], cols[3 * g + 2], colpot ? colpot[g] : 0.f);
            tile[j] = r;
        }
        __syncthreads();
        for (int q = 0; q < nq; ++q) {
            float u[SK_CHUNK], dx[SK_CHUNK], dy[SK_CHUNK], dz[SK_CHUNK];
            float cm = -INFINITY;
#pragma unroll
            for (int e = 0; e < SK_CHUNK; ++e) {
                const float4 v = tile[(q * SK_CHUNK + e) * SK_SPLIT + c];
                dx[e] = px - v.x; dy[e] = py - v.y; dz[e] = pz - v.z;
                const float d2 = fmaf(dz[e], dz[e], fmaf(dy[e], dy[e], dx[e] * dx[e]));
                u[e] = fmaf(d2, -0.5f, v.w);
                cm = fmaxf(cm, u[e]);
            }
            const float Mn = fmaxf(a.M, cm);                                                // finite: a.M >= SK_EMPTY
            const float sc = sk_exp2((a.M - Mn) * k);
            a.S *= sc;
            if (GRAD) { a.ax *= sc; a.ay *= sc; a.az *= sc; }
#pragma unroll
            for (int e = 0; e < SK_CHUNK; ++e) {
                const float w = sk_exp2((u[e] - Mn) * k);
                a.S += w;
                if (GRAD) { a.ax = fmaf(w, dx[e], a.ax); a.ay = fmaf(w, dy[e], a.ay); a.az = fmaf(w, dz[e], a.az); }
            }
            a.M = Mn;
        }
    }
#pragma unroll
    for (int off = 1; off < SK_SPLIT; off <<= 1) {                                          // partners stay inside the row's 16 lanes
        const float Mo = __shfl_xor(a.M, off), So = __shfl_xor(a.S, off);
        const float Mn = fmaxf(a.M, Mo);
        const float s1 = sk_exp2((a.M - Mn) * k), s2 = sk_exp2((Mo - Mn) * k);
        a.S = a.S * s1 + So * s2;
        if (GRAD) {
            const float xo = __shfl_xor(a.ax, off), yo = __shfl_xor(a.ay, off), zo = __shfl_xor(a.az, off);
            a.ax = a.ax * s1 + xo * s2; a.ay = a.ay * s1 + yo * s2; a.az = a.az * s1 + zo * s2;
        }
        a.M = Mn;
    }
    return a;
}

// The row's damped soft-minimum from its merged statistics.  Once per row, so in double: the value is rounded to fp32 once, where
// it is stored, instead of at each of these operations.
__device__ __forceinline__ double sk_value(const SkAcc &a, double eps, int ncols, double damp) {
    return damp * (-(double)a.M - eps * (log((double)a.S) - log((double)ncols)));
}

// Potentials live as [f_ba n | f_aa n | g_ab m | g_bb m]; softmin z writes block z and reads the block of its columns' potentials.
struct SkStep {
    const float *x, *y, *pin;          // pin == nullptr: the initialisation (zero potentials, no averaging)
    float *pout;
    int n, m;
    float k;                           // log2(e) / eps
    double eps, damp;
};

__device__ __forceinline__ size_t sk_block_off(int z, int n, int m) {
    return z == 0 ? 0 : z == 1 ? (size_t)n : z == 2 ? 2 * (size_t)n : 2 * (size_t)n + m;
}

// One Sinkhorn step: blockIdx.y = softmin (0 f_ba: rows x, columns y, g_ab; 1 f_aa: x, x, f_aa; 2 g_ab: y, x, f_ba; 3 g_bb: y, y, g_bb),
// all four from the old potentials `pin`, written averaged with their old value to `pout`.
extern "C" __global__ void __launch_bounds__(256)
k_sinkhorn_step(SkStep p) {
    __shared__ __attribute__((aligned(16))) float4 tile[SK_TILE];
    const int z = blockIdx.y;
    const bool rows_x = z < 2, cols_x = z == 1 || z == 2;
    const float *rows = rows_x ? p.x : p.y, *cols = cols_x ? p.x : p.y;
    const int nrows = rows_x ? p.n : p.m, ncols = cols_x ? p.n : p.m;
    const int row0 = blockIdx.x * SK_ROWS;
    if (row0 >= nrows) return;                                                              // whole workgroup: before any barrier
    const int row = row0 + (threadIdx.x >> 4), rr = row < nrows ? row : nrows - 1;          // rows past the end repeat the last, unwritten
    const int zc = z == 0 ? 2 : z == 2 ? 0 : z;
    const float *colpot = p.pin ? p.pin + sk_block_off(zc, p.n, p.m) : nullptr;
    const SkAcc a = sk_softmin<false>(cols, ncols, colpot, p.k, rows[3 * (size_t)rr], rows[3 * (size_t)rr + 1], rows[3 * (size_t)rr + 2], tile);
    if ((threadIdx.x & (SK_SPLIT - 1)) == 0 && row < nrows) {
        const size_t o = sk_block_off(z, p.n, p.m) + row;
        const double v = sk_value(a, p.eps, ncols, p.damp);
        p.pout[o] = (float)(p.pin ? 0.5 * ((double)p.pin[o] + v) : v);
    }
}

struct SkFinal {
    const float *x, *y, *pin;
    float *grad_x, *potentials;        // either may be NULL
    double *partials;                  // [2][gridDim.x]: per-workgroup sums of the loss terms of the x rows, then of the y rows
    int n, m;
    float k;
    double eps, damp, rho;             // rho == 0: balanced
};

// The extrapolation: blockIdx.y = 0 the x rows (F_ba then F_aa, and grad_x), 1 the y rows (G_ab then G_bb).
template <bool GRAD>
__device__ __forceinline__ void sk_final_side(const SkFinal &p, float4 *tile, double *red) {
    const float *rows = GRAD ? p.x : p.y, *other = GRAD ? p.y : p.x;
    const int nrows = GRAD ? p.n : p.m, nother = GRAD ? p.m : p.n;
    const int z1 = GRAD ? 0 : 2, z2 = z1 + 1;                                               // potentials written; columns' potentials:
    const size_t c1 = sk_block_off(GRAD ? 2 : 0, p.n, p.m), c2 = sk_block_off(z2, p.n, p.m); // g_ab / f_ba across, f_aa / g_bb within
    const int r = threadIdx.x >> 4, row = blockIdx.x * SK_ROWS + r, rr = row < nrows ? row : nrows - 1;
    const float px = rows[3 * (size_t)rr], py = rows[3 * (size_t)rr + 1], pz = rows[3 * (size_t)rr + 2];
    const SkAcc a1 = sk_softmin<GRAD>(other, nother, p.pin + c1, p.k, px, py, pz, tile);
    const SkAcc a2 = sk_softmin<GRAD>(rows, nrows, p.pin + c2, p.k, px, py, pz, tile);
    const bool writer = (threadIdx.x & (SK_SPLIT - 1)) == 0 && row < nrows;
    double term = 0.0;
    if (writer) {                                                                           // one lane per row; double, like sk_value
        const double F1 = sk_value(a1, p.eps, nother, p.damp), F2 = sk_value(a2, p.eps, nrows, p.damp);
        double e1 = 1.0, e2 = 1.0;
        if (p.rho > 0.0) { e1 = exp(-F1 / p.rho); e2 = exp(-F2 / p.rho); }
        // the row's loss term: F1 - F2, or exp(-F2 / rho) - exp(-F1 / rho) formed without the cancellation
        term = p.rho > 0.0 ? -e2 * expm1(-(F1 - F2) / p.rho) : F1 - F2;
        if (p.potentials) {
            p.potentials[sk_block_off(z1, p.n, p.m) + row] = (float)F1;
            p.potentials[sk_block_off(z2, p.n, p.m) + row] = (float)F2;
        }
        if (GRAD && p.grad_x) {
            // dF = damp (x_i - sum_j W_ij v_j) = damp A / S;  balanced: (dF_ba - dF_aa) / n;  unbalanced: the library's backward
            // weight (1 + eps / rho) on exp(-F / rho) dF
            const double w = (p.rho > 0.0 ? 1.0 + p.eps / p.rho : 1.0) / p.n * p.damp;
            const double i1 = e1 / a1.S, i2 = e2 / a2.S;
            p.grad_x[3 * (size_t)row]     = (float)(w * (a1.ax * i1 - a2.ax * i2));
            p.grad_x[3 * (size_t)row + 1] = (float)(w * (a1.ay * i1 - a2.ay * i2));
            p.grad_x[3 * (size_t)row + 2] = (float)(w * (a1.az * i1 - a2.az * i2));
        }
    }
    if ((threadIdx.x & (SK_SPLIT - 1)) == 0) red[r] = term;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < SK_ROWS; ++i) s += red[i];
        p.partials[(size_t)(GRAD ? 0 : 1) * gridDim.x + blockIdx.x] = s;
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_sinkhorn_final(SkFinal p) {
    __shared__ __attribute__((aligned(16))) float4 tile[SK_TILE];
    __shared__ double red[SK_ROWS];
    const int side = blockIdx.y;
    if (blockIdx.x * SK_ROWS >= (side == 0 ? p.n : p.m)) {                                  // no row of this side: its partial reads as zero
        if (threadIdx.x == 0) p.partials[(size_t)side * gridDim.x + blockIdx.x] = 0.0;
        return;
    }
    if (side == 0) sk_final_side<true>(p, tile, red);
    else sk_final_side<false>(p, tile, red);
}

// loss = scale (sum_x / n + sum_y / m) over the per-workgroup partials, each side folded in one fixed order
extern "C" __global__ void __launch_bounds__(256)
k_sinkhorn_loss(const double *partials, int nb, int n, int m, double scale, float *loss) {
    __shared__ double scratch[2 * 256];
    double s[2] = {0.0, 0.0};
    for (int i = threadIdx.x; i < nb; i += 256) { s[0] += partials[i]; s[1] += partials[(size_t)nb + i]; }
    block_fold<2>(s, scratch, FoldSum());
    if (threadIdx.x == 0) *loss = (float)(scale * (s[0] / n + s[1] / m));
}

// ------------------------------------------------------------------------------------------------
// host entries
// ------------------------------------------------------------------------------------------------
static int sk_blocks(int n, int m) { return ((n > m ? n : m) + SK_ROWS - 1) / SK_ROWS; }

extern "C" int ndp_sinkhorn_schedule(double diameter, double blur, double scaling, double *eps_out, int cap) {
    if (!(diameter > 0.0) || !std::isfinite(diameter) || !(blur > 0.0) || !std::isfinite(blur) || !(scaling > 0.0 && scaling < 1.0) ||
        cap < 0 || (cap > 0 && !eps_out))
        return fail(NDP_E_INVALID, "ndp_sinkhorn_schedule: diameter and blur must be positive and finite, 0 < scaling < 1, cap >= 0");
    const double start = 2.0 * log(diameter), stop = 2.0 * log(blur), step = 2.0 * log(scaling);
    const double cnt = ceil((stop - start) / step);                                         // numpy.arange: empty when diameter <= blur
    if (cnt > 1e6) return fail(NDP_E_UNSUPPORTED, "ndp_sinkhorn_schedule: more than a million entries");
    const int mid = cnt > 0.0 ? (int)cnt : 0, total = mid + 2;
    for (int i = 0; i < total && i < cap; ++i)
        eps_out[i] = i == 0 ? diameter * diameter : i == total - 1 ? blur * blur : exp(start + (i - 1) * step);
    return total;
}

extern "C" int ndp_sinkhorn_workspace(int n, int m, long long *nfloats) {
    if (n < 1 || m < 1 || !nfloats) return fail(NDP_E_INVALID, "ndp_sinkhorn_workspace: n, m >= 1 and a result pointer");
    *nfloats = 4LL * sk_blocks(n, m) + 4LL * ((long long)n + m);
    return 0;
}

extern "C" int ndp_sinkhorn_divergence(const float *x, int n, const float *y, int m, float blur, float reach, float scaling, double diameter,
                                       float *ws, float *loss_out, float *grad_x, float *potentials, void *stream) {
    if (n < 1 || m < 1) return fail(NDP_E_INVALID, "ndp_sinkhorn_divergence: n, m >= 1");
    if (!(blur > 0.f) || !std::isfinite(blur)) return fail(NDP_E_INVALID, "ndp_sinkhorn_divergence: blur must be positive and finite");
    if (!(scaling > 0.f && scaling < 1.f)) return fail(NDP_E_INVALID, "ndp_sinkhorn_divergence: scaling must lie in (0, 1)");
    if (!(diameter > 0.0) || !std::isfinite(diameter)) return fail(NDP_E_INVALID, "ndp_sinkhorn_divergence: diameter must be positive and finite");
    if (std::isnan(reach) || std::isinf(reach)) return fail(NDP_E_INVALID, "ndp_sinkhorn_divergence: reach must be finite (<= 0: balanced)");
    if (!x || !y || !ws || !loss_out) return fail(NDP_E_INVALID, "ndp_sinkhorn_divergence: null pointer");
    if (((uintptr_t)ws & 7) != 0) return fail(NDP_E_INVALID, "ndp_sinkhorn_divergence: the workspace must be 8-byte aligned");
    double eps_list[SK_MAX_EPS];
    const int L = ndp_sinkhorn_schedule(diameter, (double)blur, (double)scaling, eps_list, SK_MAX_EPS);
    if (L < 0) return L;
    if (L > SK_MAX_EPS) return fail(NDP_E_UNSUPPORTED, "ndp_sinkhorn_divergence: the epsilon schedule has more than 256 entries");
    hipStream_t s = (hipStream_t)stream;
    const int nb = sk_blocks(n, m);
    const size_t npot = 2 * ((size_t)n + m);
    double *partials = reinterpret_cast<double *>(ws);
    float *pot[2] = {ws + 4 * (size_t)nb, ws + 4 * (size_t)nb + npot};
    const double rho = reach > 0.f ? (double)reach * reach : 0.0;
    SkStep st;
    st.x = x; st.y = y; st.n = n; st.m = m;
    int cur = 0;                                                                            // pot[cur] holds the current potentials
    double eps = eps_list[0];
    for (int i = -1; i < L; ++i) {                                                          // -1: the initialisation at eps_list[0]
        eps = eps_list[i < 0 ? 0 : i];
        st.eps = eps; st.k = (float)(1.4426950408889634 / eps); st.damp = rho > 0.0 ? 1.0 / (1.0 + eps / rho) : 1.0;
        st.pin = i < 0 ? nullptr : pot[cur];
        st.pout = i < 0 ? pot[cur] : pot[cur ^ 1];
        hipLaunchKernelGGL(k_sinkhorn_step, dim3(nb, 4), dim3(256), 0, s, st);
        if (i >= 0) cur ^= 1;
    }
    SkFinal f;
    f.x = x; f.y = y; f.pin = pot[cur]; f.grad_x = grad_x; f.potentials = potentials; f.partials = partials; f.n = n; f.m = m;
    f.eps = st.eps; f.k = st.k; f.damp = st.damp; f.rho = rho;
    hipLaunchKernelGGL(k_sinkhorn_final, dim3(nb, 2), dim3(256), 0, s, f);
    hipLaunchKernelGGL(k_sinkhorn_loss, dim3(1), dim3(256), 0, s, (const double *)partials, nb, n, m, rho > 0.0 ? rho + 0.5 * eps : 1.0, loss_out);
    HIP_TRY(hipGetLastError(), "sinkhorn launch");
    return 0;
}
