// ndp_ops.inc -- the single-pair operators: brute-force and latency-shape nearest neighbours (k_nn), k_chamfer_bwd, k_landmark, k_adam.
// ---- brute-force 1-NN.  Two queries per thread; references staged in LDS as SoA (x[], y[], z[]) so that
// one ds_read_b128 feeds four references; distances in packed fp32 (v_pk_add/mul/fma: two references per
// instruction, same fma chain and therefore the same bits as the scalar form); the running minimum is
// tracked per 16-reference sub-chunk with v_min3 and the exact (lowest) index is recovered by re-scanning
// the winning sub-chunk.  ~3.7 VALU instructions per distance instead of ~10.
#define NN_STAGE 2048
#ifndef NN_SUB
#define NN_SUB 16
#endif
#define NN_QPB 512                    /* queries per workgroup (standalone operator: two per thread) */
typedef float f32x2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ f32x2 pk_dist2(f32x2 X, f32x2 Y, f32x2 Z, f32x2 qx, f32x2 qy, f32x2 qz) {
    const f32x2 dx = qx - X, dy = qy - Y, dz = qz - Z;
    f32x2 dd = dx * dx;
    dd = __builtin_elementwise_fma(dy, dy, dd);
    dd = __builtin_elementwise_fma(dz, dz, dd);
    return dd;
}

// NQ queries per thread (queries qbase + t + 256*w): the reference tile read from LDS is shared by NQ queries
template <int NQ>
__device__ __forceinline__ void nn_body(const float *q, int nq, const float *r, int nr, float *d2, int *idx,
                                        int qbase, float *sm /*[3][NN_STAGE]*/) {
    const int t = threadIdx.x;
    float *xs = sm, *ys = sm + NN_STAGE, *zs = sm + 2 * NN_STAGE;
    float qc[NQ][3];
    f32x2 qx[NQ], qy[NQ], qz[NQ];
    float best[NQ];
    int sc_best[NQ];                                       // winning sub-chunk (global index)
#pragma unroll
    for (int w = 0; w < NQ; ++w) {
        const int i = qbase + 256 * w + t;
        qc[w][0] = qc[w][1] = qc[w][2] = 0.f;
        if (i < nq) { qc[w][0] = q[3 * (size_t)i]; qc[w][1] = q[3 * (size_t)i + 1]; qc[w][2] = q[3 * (size_t)i + 2]; }
        qx[w] = f32x2{qc[w][0], qc[w][0]}; qy[w] = f32x2{qc[w][1], qc[w][1]}; qz[w] = f32x2{qc[w][2], qc[w][2]};
        best[w] = INFINITY;
        sc_best[w] = -1;
    }
    for (int c0 = 0; c0 < nr; c0 += NN_STAGE) {
        const int cn = min(NN_STAGE, nr - c0);
        const int cpad = (cn + NN_SUB - 1) / NN_SUB * NN_SUB;
        __syncthreads();
        {   // stage: all loads first, then the LDS stores (one exposed latency, not eight)
            float v[NN_STAGE / 256][3];
#pragma unroll
            for (int k = 0; k < NN_STAGE / 256; ++k) {
                const int j = t + 256 * k;
                const float nanv = __builtin_nanf("");
                v[k][0] = v[k][1] = v[k][2] = nanv;       // padding never wins a minimum nor an equality
                if (j < cn) {
                    const float *rp = r + 3 * (size_t)(c0 + j);
                    v[k][0] = rp[0]; v[k][1] = rp[1]; v[k][2] = rp[2];
                }
            }
#pragma unroll
            for (int k = 0; k < NN_STAGE / 256; ++k) {
                const int j = t + 256 * k;
                if (j < cpad) { xs[j] = v[k][0]; ys[j] = v[k][1]; zs[j] = v[k][2]; }
            }
        }
        __syncthreads();
        const int nsub = cpad / NN_SUB;
        for (int sc = 0; sc < nsub; ++sc) {
            float m[NQ];
#pragma unroll
            for (int w = 0; w < NQ; ++w) m[w] = INFINITY;
#pragma unroll
            for (int u = 0; u < NN_SUB / 4; ++u) {
                const int o = sc * NN_SUB + 4 * u;
                const float4 X = *reinterpret_cast<const float4 *>(xs + o);
                const float4 Y = *reinterpret_cast<const float4 *>(ys + o);
                const float4 Z = *reinterpret_cast<const float4 *>(zs + o);
                const f32x2 X0 = {X.x, X.y}, X1 = {X.z, X.w}, Y0 = {Y.x, Y.y}, Y1 = {Y.z, Y.w}, Z0 = {Z.x, Z.y}, Z1 = {Z.z, Z.w};
#pragma unroll
                for (int w = 0; w < NQ; ++w) {
                    const f32x2 a0 = pk_dist2(X0, Y0, Z0, qx[w], qy[w], qz[w]), a1 = pk_dist2(X1, Y1, Z1, qx[w], qy[w], qz[w]);
                    m[w] = fminf(fminf(m[w], a0.x), a0.y);
                    m[w] = fminf(fminf(m[w], a1.x), a1.y);
                }
            }
            const int gsc = (c0 / NN_SUB) + sc;
#pragma unroll
            for (int w = 0; w < NQ; ++w)
                if (m[w] < best[w]) { best[w] = m[w]; sc_best[w] = gsc; }
        }
    }
    // exact lowest index inside the winning sub-chunk (same arithmetic -> bitwise equality is safe)
#pragma unroll
    for (int w = 0; w < NQ; ++w) {
        const int i = qbase + 256 * w + t;
        if (i >= nq) continue;
        int bi = -1;
        if (sc_best[w] >= 0) {
            const int j0 = sc_best[w] * NN_SUB, j1 = min(j0 + NN_SUB, nr);
            for (int j = j1 - 1; j >= j0; --j) {
                const float dx = qc[w][0] - r[3 * (size_t)j], dy = qc[w][1] - r[3 * (size_t)j + 1], dz = qc[w][2] - r[3 * (size_t)j + 2];
                const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
                if (dd == best[w]) bi = j;                // descending j: the last hit is the lowest index
            }
        }
        d2[i] = best[w];
        idx[i] = bi;
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_nn(const float *x, int S, const float *y, int T, float *d2x, int *idx_x, float *d2y, int *idx_y) {
    __shared__ __attribute__((aligned(16))) float sm[3 * NN_STAGE];
    const int bx = (S + NN_QPB - 1) / NN_QPB;
    if ((int)blockIdx.x < bx) nn_body<2>(x, S, y, T, d2x, idx_x, blockIdx.x * NN_QPB, sm);
    else nn_body<2>(y, T, x, S, d2y, idx_y, (blockIdx.x - bx) * NN_QPB, sm);
}

// Latency shape of the exact 1-NN (few pairs resident: one pair must spread over the chip).  A workgroup owns 64
// queries, one per lane; its NW waves each scan an NW-th of every 2048-reference stage (LDS, broadcast reads, the
// same packed arithmetic and sub-chunk bookkeeping as nn_body), then the NW candidates of a query are folded in
// reference order (strict <: the earliest part keeps ties).  S/64 + T/64 workgroups per pair instead of S/512 + T/512.
template <int NW>
__device__ __forceinline__ void nn_lat_body(const float *q, int nq, const float *r, int nr, float *d2, int *idx,
                                            int qbase, float *sm /*[3][NN_STAGE] + [NW][64] + [NW][64]*/) {
    constexpr int NT = 64 * NW;                                     // threads of the workgroup: NW waves share the 64 queries
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    float *xs = sm, *ys = sm + NN_STAGE, *zs = sm + 2 * NN_STAGE;
    float *cb = sm + 3 * NN_STAGE;
    int *ci = reinterpret_cast<int *>(cb + NT);
    const int i = qbase + lane;
    // (the query is requested unconditionally at a clamped index, next to the stage's references: behind `if (i < nq)` it was a global
    //  round trip of its own in front of them; a lane beyond nq scans with the last query and writes nothing)
    float qc[3];
    {
        const float *qp = q + 3 * (size_t)min(i, nq - 1);
        qc[0] = qp[0]; qc[1] = qp[1]; qc[2] = qp[2];
    }
    const f32x2 qx = {qc[0], qc[0]}, qy = {qc[1], qc[1]}, qz = {qc[2], qc[2]};
    float best = INFINITY;
    int sc_best = -1;
    for (int c0 = 0; c0 < nr; c0 += NN_STAGE) {
        const int cn = min(NN_STAGE, nr - c0);
        const int cpad = (cn + NN_SUB - 1) / NN_SUB * NN_SUB;
        __syncthreads();
        {
            float v[NN_STAGE / NT][3];
#pragma unroll
            for (int k = 0; k < NN_STAGE / NT; ++k) {
                const int j = t + NT * k;
                const float nanv = __builtin_nanf("");
                v[k][0] = v[k][1] = v[k][2] = nanv;
                if (j < cn) { const float *rp = r + 3 * (size_t)(c0 + j); v[k][0] = rp[0]; v[k][1] = rp[1]; v[k][2] = rp[2]; }
            }
#pragma unroll
            for (int k = 0; k < NN_STAGE / NT; ++k) {
                const int j = t + NT * k;
                if (j < cpad) { xs[j] = v[k][0]; ys[j] = v[k][1]; zs[j] = v[k][2]; }
            }
        }
        __syncthreads();
        const int nsub = cpad / NN_SUB, per = (nsub + NW - 1) / NW;           // sub-chunks of this stage, per wave
        for (int sc = wv * per; sc < min(nsub, (wv + 1) * per); ++sc) {
            float m = INFINITY;
#pragma unroll
            for (int u = 0; u < NN_SUB / 4; ++u) {
                const int o = sc * NN_SUB + 4 * u;
                const float4 X = *reinterpret_cast<const float4 *>(xs + o);
                const float4 Y = *reinterpret_cast<const float4 *>(ys + o);
                const float4 Z = *reinterpret_cast<const float4 *>(zs + o);
                const f32x2 X0 = {X.x, X.y}, X1 = {X.z, X.w}, Y0 = {Y.x, Y.y}, Y1 = {Y.z, Y.w}, Z0 = {Z.x, Z.y}, Z1 = {Z.z, Z.w};
                const f32x2 a0 = pk_dist2(X0, Y0, Z0, qx, qy, qz), a1 = pk_dist2(X1, Y1, Z1, qx, qy, qz);
                m = fminf(fminf(m, a0.x), a0.y);
                m = fminf(fminf(m, a1.x), a1.y);
            }
            if (m < best) { best = m; sc_best = c0 / NN_SUB + sc; }
        }
    }
    // Which reference of the winning sub-chunk: its NN_SUB candidates are requested TOGETHER -- from the LDS stage when there was only
    // one (the references are still there: the same values), from global memory at a clamped index otherwise -- and compared from the
    // last to the first (the lowest index of the minimum stays).  Until round 6 a loop of one global round trip per candidate: sixteen
    // dependent round trips, a third of the batch-1 stage.
    int bi = -1;
    if (sc_best >= 0 && i < nq) {
        const int j0 = sc_best * NN_SUB;
        float rx[NN_SUB], ry[NN_SUB], rz[NN_SUB];
        if (nr <= NN_STAGE) {
#pragma unroll
            for (int u = 0; u < NN_SUB; ++u) { rx[u] = xs[j0 + u]; ry[u] = ys[j0 + u]; rz[u] = zs[j0 + u]; }   // (NaN beyond nr: never equal)
        } else {
#pragma unroll
            for (int u = 0; u < NN_SUB; ++u) {
                const float *rp = r + 3 * (size_t)min(j0 + u, nr - 1);
                rx[u] = rp[0]; ry[u] = rp[1]; rz[u] = rp[2];
            }
        }
#pragma unroll
        for (int u = NN_SUB - 1; u >= 0; --u) {
            const float dx = qc[0] - rx[u], dy = qc[1] - ry[u], dz = qc[2] - rz[u];
            const float dd = fmaf(dz, dz, fmaf(dy, dy, dx * dx));
            if (j0 + u < nr && dd == best) bi = j0 + u;
        }
    }
    // The quarters of one stage are in reference order, but a later stage's quarter w precedes nothing of an earlier
    // stage: a wave's running best is over ITS quarters of all stages, so ties across waves must be broken by index.
    cb[64 * wv + lane] = best;
    ci[64 * wv + lane] = bi;
    __syncthreads();
    if (wv == 0 && i < nq) {
        float b = cb[lane];
        int k = ci[lane];
#pragma unroll
        for (int w = 1; w < NW; ++w) {
            const float v = cb[64 * w + lane];
            const int kv = ci[64 * w + lane];
            if (v < b || (v == b && kv >= 0 && (k < 0 || kv < k))) { b = v; k = kv; }
        }
        d2[i] = b;
        idx[i] = k;
    }
}

// sum_i sqrt(d2_i) [d2_i < trunc], deterministic block reduction (all 256 threads get the value)
__device__ __forceinline__ float l1_sum(const float *d2, int n, float trunc, float *scratch) {
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        const float v = d2[i];
        s += (v >= trunc) ? 0.f : sqrtf(v);
    }
    return block_fold_one(s, scratch, FoldSum());
}
__device__ __forceinline__ float sq_sum(const float *x, const float *tt, int K, float *scratch) {
    float s = 0.f;
    for (int k = threadIdx.x; k < K; k += 256) {
        const float e0 = x[3 * k] - tt[3 * k], e1 = x[3 * k + 1] - tt[3 * k + 1], e2 = x[3 * k + 2] - tt[3 * k + 2];
        s += fmaf(e2, e2, fmaf(e1, e1, e0 * e0));
    }
    return block_fold_one(s, scratch, FoldSum());
}

extern "C" __global__ void __launch_bounds__(256)
k_chamfer_bwd(const float *x, int S, const float *y, int T, float trunc, const float *d2x, const int *idx_x,
              const float *d2y, const int *idx_y, float *loss, float *gx, int point_sum) {
    __shared__ float scratch[256];
    // point_reduction (loss.py:233-235): "mean" divides each direction's sum by its point count, "sum" does not
    const float Sdiv = point_sum ? 1.0f : (float)S, Tdiv = point_sum ? 1.0f : (float)T;
    if (blockIdx.x == 0) {
        const float sx = l1_sum(d2x, S, trunc, scratch);
        const float sy = l1_sum(d2y, T, trunc, scratch);
        if (threadIdx.x == 0) loss[0] = sx / Sdiv + sy / Tdiv;
    }
    if (!gx) return;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= S) return;
    const float xi[3] = {x[3 * i], x[3 * i + 1], x[3 * i + 2]};
    float g[3] = {0.f, 0.f, 0.f};
    if (!(d2x[i] >= trunc)) {
        const float *yy = y + 3 * idx_x[i];
        const float inv = 1.0f / (Sdiv * sqrtf(d2x[i]));
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = (xi[a] - yy[a]) * inv;
    }
    for (int j = 0; j < T; ++j) {           // ascending j: same order as the oracle / the CPU reference
        if (idx_y[j] == i && !(d2y[j] >= trunc)) {
            const float inv = 1.0f / (Tdiv * sqrtf(d2y[j]));
#pragma unroll
            for (int a = 0; a < 3; ++a) g[a] = fmaf(xi[a] - y[3 * j + a], inv, g[a]);
        }
    }
    gx[3 * i] = g[0]; gx[3 * i + 1] = g[1]; gx[3 * i + 2] = g[2];
}

extern "C" __global__ void __launch_bounds__(256)
k_landmark(const float *x, const float *tt, int K, float *loss, float *gx) {
    __shared__ float scratch[256];
    const float invK = 1.0f / (float)K;
    if (blockIdx.x == 0) {
        const float s = sq_sum(x, tt, K, scratch);
        if (threadIdx.x == 0) loss[0] = s * invK;
    }
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k < K && gx) {
#pragma unroll
        for (int a = 0; a < 3; ++a) gx[3 * k + a] = 2.0f * (x[3 * k + a] - tt[3 * k + a]) * invK;
    }
}

// torch.optim.Adam single-tensor update, op for op (see oracle ndp_o_adam)
__device__ __forceinline__ void adam_update(float &p, float g, float &m, float &v, float w1, float b2, float w2,
                                            float neg_step, float bc2s, float eps) {
    const float mi = m + w1 * (g - m);
    float vi = v * b2;
    vi = vi + (w2 * g) * g;
    const float denom = sqrtf(vi) / bc2s + eps;
    p = p + (neg_step * mi) / denom;
    m = mi;
    v = vi;
}

extern "C" __global__ void k_adam(float *p, const float *g, float *m, float *v, int P, float w1, float b2, float w2,
                                  float neg_step, float bc2s, float eps) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float pi = p[i], mi = m[i], vi = v[i];
    adam_update(pi, g[i], mi, vi, w1, b2, w2, neg_step, bc2s, eps);
    p[i] = pi; m[i] = mi; v[i] = vi;
}
