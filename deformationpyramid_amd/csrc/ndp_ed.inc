// ndp_ed.inc -- embedded-deformation N-ICP comparison baseline (SURVEY section 8 f4), included at the end of ndp_kernels.hip.
//
//   ED_warp                        model/geometry.py:37-49       y = sum_k w_k (R_k (x - g_k) + g_k + t_k),  6 anchors per point
//   arap_cost                      model/loss.py:261-285         mean_{i, slot} w_ij |R_i (g_j - g_i) + g_i + t_i - g_j - t_j|^2
//   axis_angle_to_matrix           pytorch3d.transforms (absent, un-pinned upstream): through the unit quaternion, Taylor branch
//                                  below 1e-6 rad; written once on the value+derivative scalar so that d R / d phi is three
//                                  forward-mode passes per node
//   gradients of  w_cd cd + w_arap arap + w_ldmk ldmk  wrt the node rotations phi and translations t
//                                  (autograd of registration.py:376-440), one workgroup per node, fixed summation order, no atomics
// Upstream's -1 anchor / edge slots index the LAST node (python negative indexing) with weight 0: reproduced.
// Problem sizes are tiny (a few hundred nodes, 2000 samples): these kernels are latency bound, not roofline material.

__device__ __forceinline__ void ed_aa_to_matrix(const Dualf (&a)[3], Dualf (&R)[9]) {
    const Dualf s2 = a[0] * a[0] + a[1] * a[1] + a[2] * a[2];
    Dualf ang = s2.v > 0.f ? dsqrt(s2) : Dualf{0.f, 0.f};               // torch.norm's subgradient at 0 is 0
    const Dualf half = dconst(0.5f) * ang;
    const Dualf s = fabsf(ang.v) < 1e-6f ? dconst(0.5f) - ang * ang / dconst(48.f) : dsin(half) / ang;
    const Dualf q[4] = {dcos(half), a[0] * s, a[1] * s, a[2] * s};
    const Dualf two_s = dconst(2.f) / (((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    const Dualf r = q[0], i = q[1], j = q[2], k = q[3], one = dconst(1.f);
    R[0] = one - two_s * (j * j + k * k); R[1] = two_s * (i * j - k * r);       R[2] = two_s * (i * k + j * r);
    R[3] = two_s * (i * j + k * r);       R[4] = one - two_s * (i * i + k * k); R[5] = two_s * (j * k - i * r);
    R[6] = two_s * (i * k - j * r);       R[7] = two_s * (j * k + i * r);       R[8] = one - two_s * (i * i + j * j);
}

extern "C" __global__ void __launch_bounds__(256)
k_ed_rot(const float *phi, int n, float *R) {
    const int a = blockIdx.x * 256 + threadIdx.x;
    if (a >= n) return;
    const Dualf p[3] = {{phi[3 * a], 0.f}, {phi[3 * a + 1], 0.f}, {phi[3 * a + 2], 0.f}};
    Dualf M[9];
    ed_aa_to_matrix(p, M);
#pragma unroll
    for (int q = 0; q < 9; ++q) R[9 * a + q] = M[q].v;
}

extern "C" __global__ void __launch_bounds__(256)
k_ed_warp(const float *x, const int *anchors, const float *weights, const float *nodes, const float *R, const float *t,
          int n_nodes, int S, float *y) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= S) return;
    const float xv[3] = {x[3 * (size_t)p], x[3 * (size_t)p + 1], x[3 * (size_t)p + 2]};
    float acc[3] = {0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        int a = anchors[6 * (size_t)p + k];
        if (a < 0) a += n_nodes;
        const float w = weights[6 * (size_t)p + k];
        const float *g = nodes + 3 * a, *Ra = R + 9 * a, *ta = t + 3 * a;
        const float d[3] = {xv[0] - g[0], xv[1] - g[1], xv[2] - g[2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float rot = (Ra[3 * c] * d[0] + Ra[3 * c + 1] * d[1]) + Ra[3 * c + 2] * d[2];
            acc[c] += ((rot + g[c]) + ta[c]) * w;
        }
    }
    y[3 * (size_t)p] = acc[0]; y[3 * (size_t)p + 1] = acc[1]; y[3 * (size_t)p + 2] = acc[2];
}

// residual of one graph edge slot: r = R_i (g_j - g_i) + g_i + t_i - g_j - t_j
__device__ __forceinline__ void ed_edge_residual(const float *nodes, const float *R, const float *t, int i, int j, float (&r)[3], float (&dg)[3]) {
    const float *gi = nodes + 3 * i, *gj = nodes + 3 * j, *Ri = R + 9 * i;
#pragma unroll
    for (int c = 0; c < 3; ++c) dg[c] = gj[c] - gi[c];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float rot = (Ri[3 * c] * dg[0] + Ri[3 * c + 1] * dg[1]) + Ri[3 * c + 2] * dg[2];
        r[c] = (((rot + gi[c]) + t[3 * i + c]) - gj[c]) - t[3 * j + c];
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_ed_arap(const float *nodes, const float *R, const float *t, const int *edges, const float *ew, int n, int K, float *out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int idx = threadIdx.x; idx < n * K; idx += 256) {
        const int i = idx / K;
        int j = edges[idx];
        if (j < 0) j += n;
        float r[3], dg[3];
        ed_edge_residual(nodes, R, t, i, j, r, dg);
        s += ew[idx] * ((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    }
    const float tot = block_fold_one(s, red, FoldSum());
    if (threadIdx.x == 0) out[0] = tot / (float)(n * K);
}

// one workgroup per node a: dL/dR_a, dL/dt_a from the warped points anchored to it (gy = dL/dy [S][3]) and from the ARAP term
// (scale = w_arap), then dL/dphi_a through the axis-angle map.  grads: [phi (3n) | t (3n)].
extern "C" __global__ void __launch_bounds__(256)
k_ed_grad(const float *x, const int *anchors, const float *weights, const float *gy, int S, const float *nodes, const float *R,
          const float *t, const float *phi, const int *edges, const float *ew, int n, int K, float w_arap, float *grads) {
    __shared__ float red[256];
    const int a = blockIdx.x;
    float acc[12];                                                       // dR (9), dt (3)
#pragma unroll
    for (int q = 0; q < 12; ++q) acc[q] = 0.f;
    const float *ga = nodes + 3 * a;
    for (int idx = threadIdx.x; idx < S * 6; idx += 256) {
        int b = anchors[idx];
        if (b < 0) b += n;
        if (b != a) continue;
        const int p = idx / 6;
        const float w = weights[idx];
        const float g[3] = {w * gy[3 * (size_t)p], w * gy[3 * (size_t)p + 1], w * gy[3 * (size_t)p + 2]};
        const float d[3] = {x[3 * (size_t)p] - ga[0], x[3 * (size_t)p + 1] - ga[1], x[3 * (size_t)p + 2] - ga[2]};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            acc[3 * c] += g[c] * d[0]; acc[3 * c + 1] += g[c] * d[1]; acc[3 * c + 2] += g[c] * d[2];
            acc[9 + c] += g[c];
        }
    }
    const float sc = 2.0f * w_arap / (float)(n * K);
    for (int idx = threadIdx.x; idx < n * K; idx += 256) {
        const int i = idx / K;
        int j = edges[idx];
        if (j < 0) j += n;
        if (i != a && j != a) continue;
        float r[3], dg[3];
        ed_edge_residual(nodes, R, t, i, j, r, dg);
        const float c0 = sc * ew[idx];
        if (i == a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[3 * c] += c0 * r[c] * dg[0]; acc[3 * c + 1] += c0 * r[c] * dg[1]; acc[3 * c + 2] += c0 * r[c] * dg[2];
                acc[9 + c] += c0 * r[c];
            }
        }
        if (j == a) {
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[9 + c] -= c0 * r[c];
        }
    }
    float tot[12];
#pragma unroll
    for (int q = 0; q < 12; ++q) tot[q] = block_fold_one(acc[q], red, FoldSum());
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {                                    // dL/dphi_k = <dL/dR, dR/dphi_k>: one forward-mode pass per component
            Dualf p[3], M[9];
#pragma unroll
            for (int c = 0; c < 3; ++c) p[c] = {phi[3 * a + c], c == k ? 1.f : 0.f};
            ed_aa_to_matrix(p, M);
            float s = 0.f;
#pragma unroll
            for (int q = 0; q < 9; ++q) s += tot[q] * M[q].d;
            grads[3 * a + k] = s;
            grads[3 * n + 3 * a + k] = tot[9 + k];
        }
    }
}

extern "C" int ndp_ed_warp(const float *x, int S, const int *anchors, const float *weights, const float *nodes, int n_nodes,
                           const float *phi, const float *t, float *R_work, float *y, void *stream) {
    if (S < 0 || n_nodes < 1 || !nodes || !t || !R_work || (S > 0 && (!x || !anchors || !weights || !y)))
        return fail(NDP_E_INVALID, "ndp_ed_warp: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    // phi == NULL: warp with the rotations R_work already holds (upstream's final warp uses the R of the last loop iteration,
    // one Adam step behind phi -- registration.py:376, 449-453)
    if (phi) hipLaunchKernelGGL(k_ed_rot, dim3((n_nodes + 255) / 256), dim3(256), 0, s, phi, n_nodes, R_work);
    if (S > 0) hipLaunchKernelGGL(k_ed_warp, dim3((S + 255) / 256), dim3(256), 0, s, x, anchors, weights, nodes, R_work, t, n_nodes, S, y);
    HIP_TRY(hipGetLastError(), "k_ed_warp launch");
    return 0;
}

extern "C" int ndp_ed_arap(const float *nodes, int n_nodes, const float *R, const float *t, const int *edges, const float *edge_w,
                           int K, float *out, void *stream) {
    if (n_nodes < 1 || K < 1 || !nodes || !R || !t || !edges || !edge_w || !out) return fail(NDP_E_INVALID, "ndp_ed_arap: bad arguments");
    hipLaunchKernelGGL(k_ed_arap, dim3(1), dim3(256), 0, (hipStream_t)stream, nodes, R, t, edges, edge_w, n_nodes, K, out);
    HIP_TRY(hipGetLastError(), "k_ed_arap launch");
    return 0;
}

extern "C" int ndp_ed_grad(const float *x, int S, const int *anchors, const float *weights, const float *gy, const float *nodes,
                           int n_nodes, const float *R, const float *t, const float *phi, const int *edges, const float *edge_w,
                           int K, float w_arap, float *grads, void *stream) {
    if (S < 0 || n_nodes < 1 || K < 1 || !nodes || !R || !t || !phi || !edges || !edge_w || !grads || (S > 0 && (!x || !anchors || !weights || !gy)))
        return fail(NDP_E_INVALID, "ndp_ed_grad: bad arguments");
    hipLaunchKernelGGL(k_ed_grad, dim3(n_nodes), dim3(256), 0, (hipStream_t)stream, x, anchors, weights, gy, S, nodes, R, t, phi,
                       edges, edge_w, n_nodes, K, w_arap, grads);
    HIP_TRY(hipGetLastError(), "k_ed_grad launch");
    return 0;
}
