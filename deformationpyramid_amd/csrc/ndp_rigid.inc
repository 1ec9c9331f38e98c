// ndp_rigid.inc -- rigid alignment from correspondences: weighted Procrustes (k_rigid_fit), residual counts of given transforms
// (k_rigid_score), and RANSAC over caller-drawn triples (k_rigid_hyp + k_rigid_score + k_ransac_finish), with ndp_rigid_fit /
// ndp_rigid_score / ndp_ransac_rigid_workspace / ndp_ransac_rigid.  DESIGN.md "Rigid alignment".  No atomics, no random numbers:
// every output element has one writer and every sum one fixed order (block_fold, ndp_device.h).  All entries are batched: problem b
// owns the rows off[b] .. off[b + 1] of src / tgt; the entries check the host's copy of off with check_offsets (ndp_abi_common.inc).
// ------------------------------------------------------------------------------------------------
// The 3 x 3 decomposition: one-sided (Hestenes) Jacobi in double on one lane.  The columns of A = S V are rotated in pairs until they
// are orthogonal; then A = U Sigma, the column norms are the singular values (to RELATIVE accuracy: S^T S is never formed) and
// S = U Sigma V^T.  Every element is a named scalar, nothing is indexed at run time.  With the singular values sorted descending the
// reference's R = U diag(1, 1, det U det V) V^T is
//     R = u1 v1^T + u2 v2^T + (u1 x u2)(v1 x v2)^T:
// (u1, u2, u1 x u2) and (v1, v2, v1 x v2) are right-handed, u3 = det U (u1 x u2), v3 = det V (v1 x v2), and the two signs meet their
// own product in diag(1, 1, det U det V).  So neither u3 nor sigma3 is divided by, and a rank-2 S (three points; a planar cloud) needs
// no special case.
#define RIGID_HPB 256                  // hypotheses per workgroup, one per lane
#define RIGID_TILE 2048                // correspondences per LDS tile: 2 x 3 x 2048 floats = 48 KB
#define RIGID_SWEEPS 12                // cyclic one-sided Jacobi on 3 columns: double is reached in 4-6 sweeps
#define RIGID_COND_MAX 1e6             // a triple whose sigma1 / sigma2 exceeds this is collinear
#define RIGID_RANK2_MIN 1e-10          // sigma2 <= this * sigma1: the rotation is not determined (a line, a point)
#define RIGID_FLAG_INDEX 1             // k_rigid_hyp flags: two indices equal, or one outside the problem
#define RIGID_FLAG_EDGE 2              //   an edge of the two triangles differs by more than edge_ratio
#define RIGID_FLAG_DEGENERATE 4        //   collinear triple
#define RIGID_ST_FEW 1                 // ndp_rigid_fit status: fewer than 3 non-zero weights, or a zero weight sum
#define RIGID_ST_RANK 2                //   rank of Sxy below 2

__device__ __forceinline__ bool svd_rotate(double &a0p, double &a1p, double &a2p, double &a0q, double &a1q, double &a2q,
                                           double &v0p, double &v1p, double &v2p, double &v0q, double &v1q, double &v2q) {
    const double alpha = a0p * a0p + a1p * a1p + a2p * a2p, beta = a0q * a0q + a1q * a1q + a2q * a2q;
    const double gamma = a0p * a0q + a1p * a1q + a2p * a2q;
    if (gamma == 0.0 || gamma * gamma <= 1e-34 * (alpha * beta)) return false;      // orthogonal to double already
    double c, s, x, y;
    jacobi_cs((beta - alpha) / (2.0 * gamma), c, s);
    x = c * a0p - s * a0q; y = s * a0p + c * a0q; a0p = x; a0q = y;
    x = c * a1p - s * a1q; y = s * a1p + c * a1q; a1p = x; a1q = y;
    x = c * a2p - s * a2q; y = s * a2p + c * a2q; a2p = x; a2q = y;
    x = c * v0p - s * v0q; y = s * v0p + c * v0q; v0p = x; v0q = y;
    x = c * v1p - s * v1q; y = s * v1p + c * v1q; v1p = x; v1q = y;
    x = c * v2p - s * v2q; y = s * v2p + c * v2q; v2p = x; v2q = y;
    return true;
}

__device__ __forceinline__ void svd_swap(bool sw, double &n_p, double &n_q, double &a0p, double &a1p, double &a2p, double &a0q, double &a1q,
                                         double &a2q, double &v0p, double &v1p, double &v2p, double &v0q, double &v1q, double &v2q) {
    double x;
    x = n_p; n_p = sw ? n_q : n_p; n_q = sw ? x : n_q;
    x = a0p; a0p = sw ? a0q : a0p; a0q = sw ? x : a0q;
    x = a1p; a1p = sw ? a1q : a1p; a1q = sw ? x : a1q;
    x = a2p; a2p = sw ? a2q : a2p; a2q = sw ? x : a2q;
    x = v0p; v0p = sw ? v0q : v0p; v0q = sw ? x : v0q;
    x = v1p; v1p = sw ? v1q : v1p; v1q = sw ? x : v1q;
    x = v2p; v2p = sw ? v2q : v2p; v2q = sw ? x : v2q;
}

// S (row-major, S[i][j] = sum (y_i - my_i) wn (x_j - mx_j)), the two means -> out[0..8] R row-major, out[9..11] t = my - R mx,
// out[12] the condition number sigma1 / sigma3 (three_points: sigma1 / sigma2 -- the third singular value of a centred triple is
// eps-sized rounding: its Sxy has rank 2), rounded to fp32 once.  Returns 0 or RIGID_ST_RANK, where out is identity, zero and inf.
__device__ __forceinline__ int rigid_solve(double a00, double a01, double a02, double a10, double a11, double a12, double a20, double a21,
                                           double a22, double mx0, double mx1, double mx2, double my0, double my1, double my2,
                                           bool three_points, float *out) {
    double v00 = 1.0, v01 = 0.0, v02 = 0.0, v10 = 0.0, v11 = 1.0, v12 = 0.0, v20 = 0.0, v21 = 0.0, v22 = 1.0;
    for (int sweep = 0; sweep < RIGID_SWEEPS; ++sweep) {         // columns (0, 1), (0, 2), (1, 2); a?c is row ?, column c
        bool moved = svd_rotate(a00, a10, a20, a01, a11, a21, v00, v10, v20, v01, v11, v21);
        moved |= svd_rotate(a00, a10, a20, a02, a12, a22, v00, v10, v20, v02, v12, v22);
        moved |= svd_rotate(a01, a11, a21, a02, a12, a22, v01, v11, v21, v02, v12, v22);
        if (!moved) break;
    }
    double n0 = a00 * a00 + a10 * a10 + a20 * a20, n1 = a01 * a01 + a11 * a11 + a21 * a21, n2 = a02 * a02 + a12 * a12 + a22 * a22;
    // descending; a swap needs `<`, so equal singular values keep their column order
    svd_swap(n0 < n1, n0, n1, a00, a10, a20, a01, a11, a21, v00, v10, v20, v01, v11, v21);
    svd_swap(n1 < n2, n1, n2, a01, a11, a21, a02, a12, a22, v01, v11, v21, v02, v12, v22);
    svd_swap(n0 < n1, n0, n1, a00, a10, a20, a01, a11, a21, v00, v10, v20, v01, v11, v21);
    const double s0 = sqrt(n0), s1 = sqrt(n1), s2 = sqrt(n2);
    if (!(s0 > 0.0) || !(s1 > RIGID_RANK2_MIN * s0)) {
        out[0] = 1.f; out[1] = 0.f; out[2] = 0.f; out[3] = 0.f; out[4] = 1.f; out[5] = 0.f; out[6] = 0.f; out[7] = 0.f; out[8] = 1.f;
        out[9] = 0.f; out[10] = 0.f; out[11] = 0.f; out[12] = INFINITY;
        return RIGID_ST_RANK;
    }
    const double u00 = a00 / s0, u10 = a10 / s0, u20 = a20 / s0, u01 = a01 / s1, u11 = a11 / s1, u21 = a21 / s1;
    const double u02 = u10 * u21 - u20 * u11, u12 = u20 * u01 - u00 * u21, u22 = u00 * u11 - u10 * u01;        // u1 x u2
    const double w0 = v10 * v21 - v20 * v11, w1 = v20 * v01 - v00 * v21, w2 = v00 * v11 - v10 * v01;            // v1 x v2
    const double r00 = u00 * v00 + u01 * v01 + u02 * w0, r01 = u00 * v10 + u01 * v11 + u02 * w1, r02 = u00 * v20 + u01 * v21 + u02 * w2;
    const double r10 = u10 * v00 + u11 * v01 + u12 * w0, r11 = u10 * v10 + u11 * v11 + u12 * w1, r12 = u10 * v20 + u11 * v21 + u12 * w2;
    const double r20 = u20 * v00 + u21 * v01 + u22 * w0, r21 = u20 * v10 + u21 * v11 + u22 * w1, r22 = u20 * v20 + u21 * v21 + u22 * w2;
    out[0] = (float)r00; out[1] = (float)r01; out[2] = (float)r02;
    out[3] = (float)r10; out[4] = (float)r11; out[5] = (float)r12;
    out[6] = (float)r20; out[7] = (float)r21; out[8] = (float)r22;
    out[9] = (float)(my0 - (r00 * mx0 + r01 * mx1 + r02 * mx2));
    out[10] = (float)(my1 - (r10 * mx0 + r11 * mx1 + r12 * mx2));
    out[11] = (float)(my2 - (r20 * mx0 + r21 * mx1 + r22 * mx2));
    const double small = three_points ? s1 : s2;
    out[12] = small > 0.0 ? (float)(s0 / small) : INFINITY;
    return 0;
}

// The residual of one correspondence under T = (R row-major, t): a fixed chain, the one tests/_rigid_ref.py restates.
//   d_a = fmaf(R[a][0], sx, fmaf(R[a][1], sy, fmaf(R[a][2], sz, t[a]))) - y_a;   d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx))
__device__ __forceinline__ float rigid_d2(const float (&T)[12], float sx, float sy, float sz, float yx, float yy, float yz) {
    const float dx = fmaf(T[0], sx, fmaf(T[1], sy, fmaf(T[2], sz, T[9]))) - yx;
    const float dy = fmaf(T[3], sx, fmaf(T[4], sy, fmaf(T[5], sz, T[10]))) - yy;
    const float dz = fmaf(T[6], sx, fmaf(T[7], sy, fmaf(T[8], sz, T[11]))) - yz;
    return fmaf(dz, dz, fmaf(dy, dy, dx * dx));
}

// Weighted Procrustes of the rows [k0, k1) by one 256-thread workgroup, the reference's arithmetic (procrustes.py:30-43) in double:
// wn = w / (sum |w| + eps), the two weighted means, Sxy from differences against them -- three passes, a thread's share of each sum
// in ascending row order, the shares folded by block_fold's tree: nothing depends on which lane runs when.  w NULL: mask
// (non-zero = 1) or, with both NULL, all ones.  Thread 0 solves; res [13] (LDS) = R, t, condition and *st (LDS) the status reach
// every thread behind the closing barrier.
__device__ __forceinline__ void rigid_fit_block(const float *src, const float *tgt, const float *w, const unsigned char *mask, int k0, int k1,
                                                double eps, double *scratch, float *res, int *st) {
    const int t = threadIdx.x;
    double a[2] = {0.0, 0.0};                                    // sum |w|, number of non-zero weights
    for (int k = k0 + t; k < k1; k += 256) {
        const double wk = w ? (double)w[k] : mask ? (mask[k] ? 1.0 : 0.0) : 1.0;
        a[0] += fabs(wk); a[1] += wk != 0.0 ? 1.0 : 0.0;
    }
    block_fold<2>(a, scratch, FoldSum());
    if (!(a[1] >= 3.0) || !(a[0] > 0.0)) {                       // (uniform: every thread holds the same totals)
        if (t == 0) {
            for (int i = 0; i < 12; ++i) res[i] = (i == 0 || i == 4 || i == 8) ? 1.f : 0.f;
            res[12] = INFINITY; *st = RIGID_ST_FEW;
        }
        __syncthreads();
        return;
    }
    const double inv = 1.0 / (a[0] + eps);
    double m[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = k0 + t; k < k1; k += 256) {
        const double wn = (w ? (double)w[k] : mask ? (mask[k] ? 1.0 : 0.0) : 1.0) * inv;
        const float *sp = src + 3 * (size_t)k, *yp = tgt + 3 * (size_t)k;
        m[0] += wn * (double)sp[0]; m[1] += wn * (double)sp[1]; m[2] += wn * (double)sp[2];
        m[3] += wn * (double)yp[0]; m[4] += wn * (double)yp[1]; m[5] += wn * (double)yp[2];
    }
    block_fold<6>(m, scratch, FoldSum());
    double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = k0 + t; k < k1; k += 256) {
        const double wn = (w ? (double)w[k] : mask ? (mask[k] ? 1.0 : 0.0) : 1.0) * inv;
        const float *sp = src + 3 * (size_t)k, *yp = tgt + 3 * (size_t)k;
        const double x0 = wn * ((double)sp[0] - m[0]), x1 = wn * ((double)sp[1] - m[1]), x2 = wn * ((double)sp[2] - m[2]);
        const double y0 = (double)yp[0] - m[3], y1 = (double)yp[1] - m[4], y2 = (double)yp[2] - m[5];
        s[0] += y0 * x0; s[1] += y0 * x1; s[2] += y0 * x2;
        s[3] += y1 * x0; s[4] += y1 * x1; s[5] += y1 * x2;
        s[6] += y2 * x0; s[7] += y2 * x1; s[8] += y2 * x2;
    }
    block_fold<9>(s, scratch, FoldSum());
    if (t == 0) *st = rigid_solve(s[0], s[1], s[2], s[3], s[4], s[5], s[6], s[7], s[8], m[0], m[1], m[2], m[3], m[4], m[5], false, res);
    __syncthreads();
}

extern "C" __global__ void __launch_bounds__(256)
k_rigid_fit(const float *src, const float *tgt, const float *w, const unsigned char *mask, const int *off, float eps,
            float *R, float *tr, float *cond, int *status) {
    __shared__ double scratch[9 * 256];
    __shared__ float res[13];
    __shared__ int st;
    const int b = blockIdx.x;
    rigid_fit_block(src, tgt, w, mask, off[b], off[b + 1], (double)eps, scratch, res, &st);
    const int t = threadIdx.x;
    if (t < 9) R[9 * (size_t)b + t] = res[t];
    else if (t < 12) tr[3 * (size_t)b + t - 9] = res[t];
    else if (t == 12) cond[b] = res[12];
    else if (t == 13) status[b] = st;
}

// ------------------------------------------------------------------------------------------------
// k_rigid_hyp: one lane, one hypothesis.  The checks (indices, then open3d's edge-length rule in fp32: an edge is refused when
// min(|s_a - s_b|, |y_a - y_b|) < edge_ratio * max(...)), then the three-point fit with rigid_fit_block's arithmetic (w = 1: wn =
// 1 / (3 + eps)) on the lane.  A refused hypothesis gets the identity and its flag bits; the scoring kernel does not score it.
__device__ __forceinline__ bool rigid_edge_bad(const float *sa, const float *sb, const float *ya, const float *yb, float edge_ratio) {
    const float sx = sa[0] - sb[0], sy = sa[1] - sb[1], sz = sa[2] - sb[2], yx = ya[0] - yb[0], yy = ya[1] - yb[1], yz = ya[2] - yb[2];
    const float ls = sqrtf(fmaf(sz, sz, fmaf(sy, sy, sx * sx))), ly = sqrtf(fmaf(yz, yz, fmaf(yy, yy, yx * yx)));
    return fminf(ls, ly) < edge_ratio * fmaxf(ls, ly);
}

extern "C" __global__ void __launch_bounds__(RIGID_HPB)
k_rigid_hyp(const float *src, const float *tgt, const int *off, const int *triples, int H, float edge_ratio, float eps, float *T, int *flags) {
    const int h = blockIdx.x * RIGID_HPB + threadIdx.x, b = blockIdx.y;
    if (h >= H) return;
    const int k0 = off[b], K = off[b + 1] - k0;
    const size_t e = (size_t)b * H + h;
    const int ia = triples[3 * e], ib = triples[3 * e + 1], ic = triples[3 * e + 2];
    float out[13] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, INFINITY};
    int flag = 0;
    if ((unsigned)ia >= (unsigned)K || (unsigned)ib >= (unsigned)K || (unsigned)ic >= (unsigned)K || ia == ib || ia == ic || ib == ic) {
        flag = RIGID_FLAG_INDEX;                                // nothing is read through such an index
    } else {
        const float *sa = src + 3 * (size_t)(k0 + ia), *sb = src + 3 * (size_t)(k0 + ib), *sc = src + 3 * (size_t)(k0 + ic);
        const float *ya = tgt + 3 * (size_t)(k0 + ia), *yb = tgt + 3 * (size_t)(k0 + ib), *yc = tgt + 3 * (size_t)(k0 + ic);
        if (edge_ratio > 0.f && (rigid_edge_bad(sa, sb, ya, yb, edge_ratio) || rigid_edge_bad(sa, sc, ya, yc, edge_ratio) ||
                                 rigid_edge_bad(sb, sc, yb, yc, edge_ratio))) {
            flag = RIGID_FLAG_EDGE;
        } else {
            const double wn = 1.0 / (3.0 + (double)eps);
            const double ax = sa[0], ay = sa[1], az = sa[2], bx = sb[0], by = sb[1], bz = sb[2], cx = sc[0], cy = sc[1], cz = sc[2];
            const double px = ya[0], py = ya[1], pz = ya[2], qx = yb[0], qy = yb[1], qz = yb[2], rx = yc[0], ry = yc[1], rz = yc[2];
            const double mx0 = wn * ax + wn * bx + wn * cx, mx1 = wn * ay + wn * by + wn * cy, mx2 = wn * az + wn * bz + wn * cz;
            const double my0 = wn * px + wn * qx + wn * rx, my1 = wn * py + wn * qy + wn * ry, my2 = wn * pz + wn * qz + wn * rz;
            const double xa0 = wn * (ax - mx0), xa1 = wn * (ay - mx1), xa2 = wn * (az - mx2);
            const double xb0 = wn * (bx - mx0), xb1 = wn * (by - mx1), xb2 = wn * (bz - mx2);
            const double xc0 = wn * (cx - mx0), xc1 = wn * (cy - mx1), xc2 = wn * (cz - mx2);
            const double ya0 = px - my0, ya1 = py - my1, ya2 = pz - my2, yb0 = qx - my0, yb1 = qy - my1, yb2 = qz - my2;
            const double yc0 = rx - my0, yc1 = ry - my1, yc2 = rz - my2;
            const int st = rigid_solve(ya0 * xa0 + yb0 * xb0 + yc0 * xc0, ya0 * xa1 + yb0 * xb1 + yc0 * xc1, ya0 * xa2 + yb0 * xb2 + yc0 * xc2,
                                       ya1 * xa0 + yb1 * xb0 + yc1 * xc0, ya1 * xa1 + yb1 * xb1 + yc1 * xc1, ya1 * xa2 + yb1 * xb2 + yc1 * xc2,
                                       ya2 * xa0 + yb2 * xb0 + yc2 * xc0, ya2 * xa1 + yb2 * xb1 + yc2 * xc1, ya2 * xa2 + yb2 * xb2 + yc2 * xc2,
                                       mx0, mx1, mx2, my0, my1, my2, true, out);
            if (st != 0 || !(out[12] <= (float)RIGID_COND_MAX)) {
                flag = RIGID_FLAG_DEGENERATE;
                out[0] = 1.f; out[1] = 0.f; out[2] = 0.f; out[3] = 0.f; out[4] = 1.f; out[5] = 0.f; out[6] = 0.f; out[7] = 0.f; out[8] = 1.f;
                out[9] = 0.f; out[10] = 0.f; out[11] = 0.f;
            }
        }
    }
    float *Tp = T + 12 * e;
#pragma unroll
    for (int i = 0; i < 12; ++i) Tp[i] = out[i];
    flags[e] = flag;
}

// ------------------------------------------------------------------------------------------------
// k_rigid_score: one lane, one transform; a workgroup owns RIGID_HPB of them and streams the problem's correspondences through LDS in
// tiles of RIGID_TILE, src rows and tgt rows as they lie in memory.  Every lane reads the same LDS address (a broadcast: no bank
// conflict), four correspondences per step as three 16-byte reads per cloud.  count = number of d2 < thr2, sse = their fp32 sum in
// correspondence order.  The padding of the last tile is NaN, which never passes the `<`.  flags (may be NULL): a lane whose flag
// is non-zero reports count 0, sse 0; a wave with no live lane skips the arithmetic, a workgroup with none the whole loop.
// partial (may be NULL) [gridDim.y][gridDim.x][2]: the workgroup's best (count, hypothesis) -- the largest count, the lowest
// hypothesis among equals -- for k_ransac_finish.
extern "C" __global__ void __launch_bounds__(RIGID_HPB)
k_rigid_score(const float *T, const int *flags, const float *src, const float *tgt, const int *off, int H, float thr2,
              int *count, float *sse, int *partial) {
    __shared__ __attribute__((aligned(16))) float sm[6 * RIGID_TILE];
    __shared__ int s_any;
    float *ss = sm, *sy = sm + 3 * RIGID_TILE;
    const int t = threadIdx.x, b = blockIdx.y;
    const int h = blockIdx.x * RIGID_HPB + t;
    const size_t e = (size_t)b * H + min(h, H - 1);              // a lane beyond H scores the last transform and writes nothing
    const bool live = h < H && (!flags || flags[e] == 0);
    float Tl[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Tl[i] = T[12 * e + i];
    if (t == 0) s_any = 0;
    __syncthreads();
    if (live) s_any = 1;
    __syncthreads();
    int cnt = 0;
    float sum = 0.f;
    if (s_any) {
        const bool wave_live = __any(live);
        const int k0 = off[b], K = off[b + 1] - k0;
        for (int c0 = 0; c0 < K; c0 += RIGID_TILE) {
            const int cn = min(RIGID_TILE, K - c0);
            const int cpad = (cn + 3) / 4 * 4;
            const float *sp = src + 3 * (size_t)(k0 + c0), *yp = tgt + 3 * (size_t)(k0 + c0);
            __syncthreads();
            for (int j = t; j < 3 * cpad; j += RIGID_HPB) {
                const bool in = j < 3 * cn;
                ss[j] = in ? sp[j] : __builtin_nanf("");
                sy[j] = in ? yp[j] : __builtin_nanf("");
            }
            __syncthreads();
            if (!wave_live) continue;
            for (int o = 0; o < cpad; o += 4) {
                const float4 a0 = *reinterpret_cast<const float4 *>(ss + 3 * o), a1 = *reinterpret_cast<const float4 *>(ss + 3 * o + 4),
                             a2 = *reinterpret_cast<const float4 *>(ss + 3 * o + 8);
                const float4 b0 = *reinterpret_cast<const float4 *>(sy + 3 * o), b1 = *reinterpret_cast<const float4 *>(sy + 3 * o + 4),
                             b2 = *reinterpret_cast<const float4 *>(sy + 3 * o + 8);
                const float d0 = rigid_d2(Tl, a0.x, a0.y, a0.z, b0.x, b0.y, b0.z);
                const float d1 = rigid_d2(Tl, a0.w, a1.x, a1.y, b0.w, b1.x, b1.y);
                const float d2 = rigid_d2(Tl, a1.z, a1.w, a2.x, b1.z, b1.w, b2.x);
                const float d3 = rigid_d2(Tl, a2.y, a2.z, a2.w, b2.y, b2.z, b2.w);
                if (d0 < thr2) { ++cnt; sum += d0; }
                if (d1 < thr2) { ++cnt; sum += d1; }
                if (d2 < thr2) { ++cnt; sum += d2; }
                if (d3 < thr2) { ++cnt; sum += d3; }
            }
        }
    }
    if (!live) { cnt = 0; sum = 0.f; }
    if (h < H) {
        count[e] = cnt;
        if (sse) sse[e] = sum;
    }
    if (!partial) return;
    // FoldBestCount's tree (ndp_device.h) in this kernel's own words: through block_fold the compiler schedules the scoring loop above
    // differently, and rigid_score measured 1 % slower at K = 5000 in three calls out of three (profiles/operator_refactor_ab.txt).
    int *pc = reinterpret_cast<int *>(sm), *pi = pc + RIGID_HPB;
    __syncthreads();                                             // (the last tile is no longer read)
    pc[t] = h < H ? cnt : -1;
    pi[t] = h;
    __syncthreads();
    for (int s = RIGID_HPB / 2; s > 0; s >>= 1) {
        if (t < s && (pc[t + s] > pc[t] || (pc[t + s] == pc[t] && pi[t + s] < pi[t]))) { pc[t] = pc[t + s]; pi[t] = pi[t + s]; }
        __syncthreads();
    }
    if (t == 0) {
        int *pp = partial + 2 * ((size_t)b * gridDim.x + blockIdx.x);
        pp[0] = pc[0]; pp[1] = pi[0];
    }
}

// ------------------------------------------------------------------------------------------------
// k_ransac_finish: one workgroup per problem.  Folds the scoring workgroups' partials (a thread's share in ascending order, then a
// tree; the largest count wins, the lowest hypothesis among equals), then refines: the mask under the current transform (rigid_d2
// < thr2, the scoring kernel's arithmetic), rigid_fit_block over the mask, refine_iters times; a mask of fewer than 3 inliers or a
// fit that reports a status keeps the transform and ends the loop.  The last pass leaves the mask under the final transform, its
// count and rmse = sqrt(sum d2 / count), the sum in double in the fixed tree.  A best count of 0: status 1, identity, zero mask.
struct RansacOut {
    float *R, *t, *rmse;
    unsigned char *mask;
    int *count, *best, *status;
};

extern "C" __global__ void __launch_bounds__(256)
k_ransac_finish(const float *src, const float *tgt, const int *off, const float *hT, const int *partial, int n_part, int H, float thr2,
                float eps, int refine_iters, RansacOut o) {
    __shared__ double scratch[9 * 256];
    __shared__ float res[13];
    __shared__ int st;
    const int t = threadIdx.x, b = blockIdx.x;
    const int k0 = off[b], k1 = off[b + 1];
    int bc = -1, bi = 0x7fffffff;
    for (int i = t; i < n_part; i += 256) {
        const int c = partial[2 * ((size_t)b * n_part + i)], j = partial[2 * ((size_t)b * n_part + i) + 1];
        if (c > bc || (c == bc && j < bi)) { bc = c; bi = j; }
    }
    const CountIdx best = block_fold_one(CountIdx{bc, bi}, reinterpret_cast<CountIdx *>(scratch), FoldBestCount());
    bc = best.count; bi = best.idx;
    if (bc <= 0) {
        for (int k = k0 + t; k < k1; k += 256) o.mask[k] = 0;
        if (t < 9) o.R[9 * (size_t)b + t] = (t == 0 || t == 4 || t == 8) ? 1.f : 0.f;
        else if (t < 12) o.t[3 * (size_t)b + t - 9] = 0.f;
        else if (t == 12) { o.count[b] = 0; o.rmse[b] = 0.f; o.best[b] = -1; o.status[b] = 1; }
        return;
    }
    float Tl[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) Tl[i] = hT[12 * ((size_t)b * H + bi) + i];
    double a[2];
    for (int left = refine_iters;; --left) {
        a[0] = 0.0; a[1] = 0.0;                                  // inliers under Tl, the sum of their d2
        for (int k = k0 + t; k < k1; k += 256) {
            const float *sp = src + 3 * (size_t)k, *yp = tgt + 3 * (size_t)k;
            const float d2 = rigid_d2(Tl, sp[0], sp[1], sp[2], yp[0], yp[1], yp[2]);
            const bool in = d2 < thr2;
            o.mask[k] = in ? 1 : 0;
            if (in) { a[0] += 1.0; a[1] += (double)d2; }
        }
        block_fold<2>(a, scratch, FoldSum());                      // (its barriers also publish the mask to the workgroup)
        if (left == 0 || a[0] < 3.0) break;                     // uniform; the mask and the sums are those of Tl
        rigid_fit_block(src, tgt, nullptr, o.mask, k0, k1, (double)eps, scratch, res, &st);
        const int fit_st = st;
        if (fit_st == 0) {
#pragma unroll
            for (int i = 0; i < 12; ++i) Tl[i] = res[i];
        }
        __syncthreads();                                         // res and st are read before the next fit rewrites them
        if (fit_st != 0) break;                                  // the transform stays, and the mask above is its mask
    }
    if (t == 0) {
#pragma unroll
        for (int i = 0; i < 9; ++i) o.R[9 * (size_t)b + i] = Tl[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) o.t[3 * (size_t)b + i] = Tl[9 + i];
        o.count[b] = (int)a[0];
        o.rmse[b] = a[0] > 0.0 ? (float)sqrt(a[1] / a[0]) : 0.f;
        o.best[b] = bi; o.status[b] = 0;
    }
}

// ------------------------------------------------------------------------------------------------
// host entries
// ------------------------------------------------------------------------------------------------
extern "C" int ndp_rigid_fit(const float *src, const float *tgt, const float *w, const unsigned char *mask, const int *off,
                             const int *off_host, int B, float eps, float *R, float *t, float *condition, int *status, void *stream) {
    if (int rc = check_offsets("ndp_rigid_fit", off_host, B, 0, "K", nullptr)) return rc;
    if (!src || !tgt || !off || !R || !t || !condition || !status) return fail(NDP_E_INVALID, "ndp_rigid_fit: null pointer");
    if (w && mask) return fail(NDP_E_INVALID, "ndp_rigid_fit: weights or a mask, not both");
    if (!(eps >= 0.f) || !std::isfinite(eps)) return fail(NDP_E_INVALID, "ndp_rigid_fit: eps must be finite and >= 0");
    hipLaunchKernelGGL(k_rigid_fit, dim3(B), dim3(256), 0, (hipStream_t)stream, src, tgt, w, mask, off, eps, R, t, condition, status);
    HIP_TRY(hipGetLastError(), "k_rigid_fit launch");
    return 0;
}

extern "C" int ndp_rigid_score(const float *T, const float *src, const float *tgt, const int *off, const int *off_host, int B, int H,
                               float thr, int *count, float *sse, void *stream) {
    if (int rc = check_offsets("ndp_rigid_score", off_host, B, 1, "K", nullptr)) return rc;
    if (H < 1) return fail(NDP_E_INVALID, "ndp_rigid_score: H >= 1");
    if (!(thr > 0.f) || !std::isfinite(thr)) return fail(NDP_E_INVALID, "ndp_rigid_score: thr must be positive and finite");
    if (!T || !src || !tgt || !off || !count) return fail(NDP_E_INVALID, "ndp_rigid_score: null pointer");
    const float thr2 = thr * thr;
    hipLaunchKernelGGL(k_rigid_score, dim3((H + RIGID_HPB - 1) / RIGID_HPB, B), dim3(RIGID_HPB), 0, (hipStream_t)stream,
                       T, (const int *)nullptr, src, tgt, off, H, thr2, count, sse, (int *)nullptr);
    HIP_TRY(hipGetLastError(), "k_rigid_score launch");
    return 0;
}

extern "C" int ndp_ransac_rigid_workspace(int B, int H, long long *nbytes) {
    if (B < 1 || B > NDP_MAX_B || H < 1 || !nbytes) return fail(NDP_E_INVALID, "ndp_ransac_rigid_workspace: B in 1..65535, H >= 1, nbytes not NULL");
    const long long bh = (long long)B * H, parts = (long long)B * ((H + RIGID_HPB - 1) / RIGID_HPB);
    *nbytes = 4 * (12 * bh + bh + bh + 2 * parts);
    return 0;
}

extern "C" int ndp_ransac_rigid(const float *src, const float *tgt, const int *off, const int *off_host, int B, const int *triples, int H,
                                float thr, float edge_ratio, int refine_iters, void *ws, float *R, float *t, unsigned char *mask, int *count,
                                float *rmse, int *best, int *status, int *h_count, int *h_flags, float *h_T, void *stream) {
    if (int rc = check_offsets("ndp_ransac_rigid", off_host, B, 3, "K", nullptr)) return rc;
    if (H < 1) return fail(NDP_E_INVALID, "ndp_ransac_rigid: H >= 1");
    if (!(thr > 0.f) || !std::isfinite(thr)) return fail(NDP_E_INVALID, "ndp_ransac_rigid: thr must be positive and finite");
    if (!(edge_ratio >= 0.f) || !(edge_ratio <= 1.f)) return fail(NDP_E_INVALID, "ndp_ransac_rigid: edge_ratio must lie in 0..1 (0: no edge check)");
    if (refine_iters < 0) return fail(NDP_E_INVALID, "ndp_ransac_rigid: refine_iters >= 0");
    if (!src || !tgt || !off || !triples || !ws || !R || !t || !mask || !count || !rmse || !best || !status)
        return fail(NDP_E_INVALID, "ndp_ransac_rigid: null pointer");
    if (((uintptr_t)ws & 3) != 0) return fail(NDP_E_INVALID, "ndp_ransac_rigid: the workspace must be 4-byte aligned");
    const long long bh = (long long)B * H;
    const int n_part = (H + RIGID_HPB - 1) / RIGID_HPB;
    float *wT = (float *)ws;                                     // [B][H][12] | count [B][H] | flags [B][H] | partials [B][n_part][2]
    int *wcount = (int *)(wT + 12 * bh), *wflags = wcount + bh, *wpart = wflags + bh;
    float *hT = h_T ? h_T : wT;
    int *hc = h_count ? h_count : wcount, *hf = h_flags ? h_flags : wflags;
    hipStream_t s = (hipStream_t)stream;
    const float thr2 = thr * thr, eps = 1e-4f;
    const dim3 grid(n_part, B), block(RIGID_HPB);
    hipLaunchKernelGGL(k_rigid_hyp, grid, block, 0, s, src, tgt, off, triples, H, edge_ratio, eps, hT, hf);
    HIP_TRY(hipGetLastError(), "k_rigid_hyp launch");
    hipLaunchKernelGGL(k_rigid_score, grid, block, 0, s, (const float *)hT, (const int *)hf, src, tgt, off, H, thr2, hc, (float *)nullptr, wpart);
    HIP_TRY(hipGetLastError(), "k_rigid_score launch");
    RansacOut o;
    o.R = R; o.t = t; o.rmse = rmse; o.mask = mask; o.count = count; o.best = best; o.status = status;
    hipLaunchKernelGGL(k_ransac_finish, dim3(B), dim3(256), 0, s, src, tgt, off, (const float *)hT, (const int *)wpart, n_part, H, thr2, eps,
                       refine_iters, o);
    HIP_TRY(hipGetLastError(), "k_ransac_finish launch");
    return 0;
}
