// ndp_nerfies.inc -- Nerfies comparison baseline (SURVEY section 8 f3, second half), included at the end of ndp_kernels.hip
// (it shares the tile helpers and the layer-generic backward of the NDP / NSFP paths).
//
//   Nerfies_Deformation.forward   model/nets.py:187-253  (windowed posenc :218-240, 39->128, six 128x128 ReLU layers, w / v
//                                 heads, SE(3) exponential warp :242-253 + rigid_body.py:97-110, per-point Jacobian :209-216)
//   nerfies_regularization        model/loss.py:373-379
//
// The Jacobian d warp / d x is carried FORWARD: every point drags three tangent rows through the network
// (t_out = (W t_in) * [primal z > 0]); rows are laid out as four planes [primal | d/dx0 | d/dx1 | d/dx2] of `cap` rows each.
// Upstream's Jacobian is built with create_graph=False, so the regulariser has no gradient: the backward is the Chamfer
// gradient through the primal plane only, on bwd2_body (shared with NDP / NSFP) plus a 39-wide input-layer kernel.
//
// Flat parameters: [W_in 128x39 | b_in 128 | (W_l 128x128 | b_l 128) l = 1..6 | W_h 6x128 (w rows, v rows) | b_h 6].
#define NRF_PE 39
#define NRF_PES 40                      /* row stride of the saved posenc */
#define NRF_HID 6
__host__ __device__ inline int nrf_off_W(int l /*1..6*/) { return NDP_W * NRF_PE + NDP_W + (l - 1) * (NDP_W * NDP_W + NDP_W); }
__host__ __device__ inline int nrf_off_b(int l) { return nrf_off_W(l) + NDP_W * NDP_W; }
__host__ __device__ inline int nrf_off_Wh() { return nrf_off_W(NRF_HID + 1); }
__host__ __device__ inline int nrf_off_bh() { return nrf_off_Wh() + 6 * NDP_W; }
__host__ __device__ inline int nrf_param_count() { return nrf_off_bh() + 6; }

struct NrfWindow { float w[6]; };

// ---- forward-mode scalar: value + one directional derivative ------------------------------------------------------
struct Dualf {
    float v, d;
};
__device__ __forceinline__ Dualf operator+(Dualf a, Dualf b) { return {a.v + b.v, a.d + b.d}; }
__device__ __forceinline__ Dualf operator-(Dualf a, Dualf b) { return {a.v - b.v, a.d - b.d}; }
__device__ __forceinline__ Dualf operator*(Dualf a, Dualf b) { return {a.v * b.v, a.d * b.v + a.v * b.d}; }
__device__ __forceinline__ Dualf operator/(Dualf a, Dualf b) {
    const float q = a.v / b.v;
    return {q, (a.d - q * b.d) / b.v};
}
__device__ __forceinline__ Dualf dconst(float c) { return {c, 0.f}; }
__device__ __forceinline__ Dualf dsqrt(Dualf a) {
    const float s = sqrtf(a.v);
    return {s, a.d / (2.0f * s)};
}
__device__ __forceinline__ Dualf dsin(Dualf a) { return {sinf(a.v), cosf(a.v) * a.d}; }
__device__ __forceinline__ Dualf dcos(Dualf a) { return {cosf(a.v), -sinf(a.v) * a.d}; }

// nets.py:242-253 + rigid_body.py:97-110 on duals: o = (w, v) raw head outputs, x the point; out = R(w) x + P(w) v/|w|
__device__ __forceinline__ void nrf_se3_warp(const Dualf (&o)[6], const Dualf (&x)[3], Dualf (&out)[3]) {
    const Dualf th = dsqrt(o[0] * o[0] + o[1] * o[1] + o[2] * o[2]);
    const Dualf w[3] = {o[0] / th, o[1] / th, o[2] / th}, v[3] = {o[3] / th, o[4] / th, o[5] / th};
    const Dualf z = dconst(0.f);
    const Dualf K[9] = {z, z - w[2], w[1], w[2], z, z - w[0], z - w[1], w[0], z};
    Dualf K2[9];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) K2[3 * i + j] = K[3 * i] * K[j] + K[3 * i + 1] * K[3 + j] + K[3 * i + 2] * K[6 + j];
    const Dualf s = dsin(th), c1 = dconst(1.f) - dcos(th), ts = th - s;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        Dualf r = z;
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const Dualf eye = dconst(i == j ? 1.f : 0.f);
            const Dualf Rij = eye + s * K[3 * i + j] + c1 * K2[3 * i + j];
            const Dualf Pij = eye + c1 * K[3 * i + j] + ts * K2[3 * i + j];
            r = r + Rij * x[j] + Pij * v[j];
        }
        out[i] = r;
    }
}

// ---- input layer: windowed posenc (nets.py:218-240) -> h0 = relu(W_in pe + b_in), tangents (W_in dpe_k) * [z > 0] --------
// one workgroup = 64 points; thread = (point t & 63, output block t >> 6 of 32 outputs)
extern "C" __global__ void __launch_bounds__(256)
k_nrf_in(const float *params, const float *x, int n, int cap, NrfWindow win, float *pe_out /*[cap][40]*/, float *h0 /*[4cap][128]*/) {
    __shared__ float pes[64][NRF_PES + 1];
    const int t = threadIdx.x, pt = t & 63, part = t >> 6, p = blockIdx.x * 64 + pt;
    const float PI = 3.14f;                                                    // (sic) nets.py:220
    if (part < 3) {
        const float xa = p < n ? x[3 * (size_t)p + part] : 0.f;
        pes[pt][part] = xa;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const float f = ldexpf(1.0f, j - 3) * PI;                          // 2^(j + k0) * pi, k0 = -3
            pes[pt][3 + 12 * part + j] = sinf(xa * f) * win.w[j];
            pes[pt][9 + 12 * part + j] = cosf(xa * f) * win.w[j];
        }
    } else pes[pt][NRF_PE] = 0.f;
    __syncthreads();
    for (int c = part; c < NRF_PES; c += 4) pe_out[(size_t)p * NRF_PES + c] = pes[pt][c];
    const float *W = params, *b = params + NDP_W * NRF_PE;
    const size_t row = (size_t)p * NDP_W, plane = (size_t)cap * NDP_W;
    for (int oo = 0; oo < 32; ++oo) {
        const int o = 32 * part + oo;
        const float *wr = W + o * NRF_PE;
        float z = b[o];
#pragma unroll
        for (int c = 0; c < NRF_PE; ++c) z = fmaf(wr[c], pes[pt][c], z);
        const bool on = z > 0.f && p < n;
        h0[row + o] = on ? z : 0.f;
#pragma unroll
        for (int a = 0; a < 3; ++a) {                                          // d pe / d x_a: e_a, f cos w, -f sin w on axis a's block
            float tz = wr[a];
#pragma unroll
            for (int j = 0; j < 6; ++j) {
                const float f = ldexpf(1.0f, j - 3) * PI;
                tz = fmaf(wr[3 + 12 * a + j], f * pes[pt][9 + 12 * a + j], tz);
                tz = fmaf(wr[9 + 12 * a + j], -f * pes[pt][3 + 12 * a + j], tz);
            }
            h0[(a + 1) * plane + row + o] = on ? tz : 0.f;
        }
    }
}

// ---- hidden layer with tangents: primal y = relu(W h + b); tangent planes t_out = (W t_in) * [y > 0] ---------------------
extern "C" __global__ void __launch_bounds__(256, 2)
k_nrf_dense(const float *W, const float *b, const float *hin /*[4cap][128]*/, float *hout /*[4cap][128]*/, int cap, int n_tiles) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    float *bufA = sm, *bufB = sm + 64 * NDP_LD;
    float w[64];
    load_w_fwd(W, sm, wv, l31, h, w);
    __syncthreads();                               // the weight image shares the tile buffers
    const float bias = b[32 * wv + l31];
    const size_t plane = (size_t)cap * NDP_W;
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const size_t off = (size_t)tile * NDP_TILE * NDP_W;
        load_tile_to_lds(hin + off, bufA);
        __syncthreads();
        {
            f32x16 acc0, acc1;
            acc_init_bias(bias, h, acc0, acc1);
            tile_gemm_64x32(bufA, w, l31, h, acc0, acc1);
            epilogue_relu(acc0, acc1, bufB, wv, l31, h);
        }
        __syncthreads();
        store_tile_from_lds(bufB, hout + off);                                 // bufB stays: the ReLU pattern of the three tangents
        for (int k = 1; k < 4; ++k) {
            load_tile_to_lds(hin + k * plane + off, bufA);
            __syncthreads();
            f32x16 d0, d1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { d0[r] = 0.f; d1[r] = 0.f; }
            tile_gemm_64x32(bufA, w, l31, h, d0, d1);
            __syncthreads();                                                   // every wave is done reading the tangent tile
            epilogue_mask(d0, d1, bufB, bufA, wv, l31, h);
            __syncthreads();
            store_tile_from_lds(bufA, hout + k * plane + off);
            __syncthreads();
        }
    }
}

// ---- heads: o = W_h h6 + b_h for the primal rows, D_k = W_h t6_k for the tangent rows: [4cap][8] (6 used) ----------------
extern "C" __global__ void __launch_bounds__(256)
k_nrf_heads(const float *params, const float *h6 /*[4cap][128]*/, float *heads /*[4cap][8]*/, int cap) {
    __shared__ __attribute__((aligned(16))) float tile[64 * NDP_LD];
    __shared__ __attribute__((aligned(16))) float wh[6 * NDP_W];
    const int t = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * NDP_TILE;                         // row of the 4cap-row matrix
    load_tile_to_lds(h6 + base * NDP_W, tile);
    for (int i = t; i < 6 * NDP_W; i += 256) wh[i] = params[nrf_off_Wh() + i];
    __syncthreads();
    const bool primal = base < (size_t)cap;
    const int r = t & 63;
    for (int j = t >> 6; j < 6; j += 4) {
        const float *hr = tile + r * NDP_LD, *wr = wh + j * NDP_W;
        float a0 = primal ? params[nrf_off_bh() + j] : 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
        for (int k4 = 0; k4 < 32; ++k4) {
            const float4 hv = *reinterpret_cast<const float4 *>(hr + 4 * k4);
            const float4 wv4 = *reinterpret_cast<const float4 *>(wr + 4 * k4);
            a0 = fmaf(wv4.x, hv.x, a0); a1 = fmaf(wv4.y, hv.y, a1);
            a2 = fmaf(wv4.z, hv.z, a2); a3 = fmaf(wv4.w, hv.w, a3);
        }
        heads[(base + r) * 8 + j] = (a0 + a1) + (a2 + a3);
    }
}

// largest eigenvalue of a symmetric 3x3 matrix (closed form, double): a = [a00 a01 a02 a11 a12 a22]
__device__ __forceinline__ double sym3_lambda_max(const double (&a)[6]) {
    const double p1 = a[1] * a[1] + a[2] * a[2] + a[4] * a[4];
    const double q = (a[0] + a[3] + a[5]) / 3.0;
    if (p1 == 0.0) return fmax(a[0], fmax(a[3], a[5]));
    const double b0 = a[0] - q, b3 = a[3] - q, b5 = a[5] - q;
    const double p = sqrt((b0 * b0 + b3 * b3 + b5 * b5 + 2.0 * p1) / 6.0);
    const double B0 = b0 / p, B1 = a[1] / p, B2 = a[2] / p, B3 = b3 / p, B4 = a[4] / p, B5 = b5 / p;
    double r = 0.5 * (B0 * (B3 * B5 - B4 * B4) - B1 * (B1 * B5 - B4 * B2) + B2 * (B1 * B4 - B3 * B2));
    r = r < -1.0 ? -1.0 : (r > 1.0 ? 1.0 : r);
    return q + 2.0 * p * cos(acos(r) / 3.0);
}

// ---- warp + Jacobian + regulariser term per point -------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256)
k_nrf_warp(const float *heads /*[4cap][8]*/, const float *x, int n, int cap, float *x_out, float *J /*[n][9]*/, double *regp /*[cap]*/) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    float o[6], xv[3];
#pragma unroll
    for (int j = 0; j < 6; ++j) o[j] = heads[(size_t)p * 8 + j];
#pragma unroll
    for (int a = 0; a < 3; ++a) xv[a] = x[3 * (size_t)p + a];
    float Jm[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {                                              // column k: d/d eps warp(o + eps D_k, x + eps e_k)
        Dualf od[6], xd[3], out[3];
        const float *D = heads + ((size_t)(k + 1) * cap + p) * 8;
#pragma unroll
        for (int j = 0; j < 6; ++j) od[j] = {o[j], D[j]};
#pragma unroll
        for (int a = 0; a < 3; ++a) xd[a] = {xv[a], a == k ? 1.f : 0.f};
        nrf_se3_warp(od, xd, out);
#pragma unroll
        for (int a = 0; a < 3; ++a) Jm[3 * a + k] = out[a].d;
        if (k == 0) { x_out[3 * (size_t)p] = out[0].v; x_out[3 * (size_t)p + 1] = out[1].v; x_out[3 * (size_t)p + 2] = out[2].v; }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) J[(size_t)p * 9 + i] = Jm[i];
    // loss.py:373-379: log of the largest singular value (double, clamped at 1e-6), squared
    double A[6];
    int q = 0;
    for (int i = 0; i < 3; ++i)
        for (int j = i; j < 3; ++j)
            A[q++] = (double)Jm[i] * Jm[j] + (double)Jm[3 + i] * Jm[3 + j] + (double)Jm[6 + i] * Jm[6 + j];   // (J^T J)_ij
    double lam = sym3_lambda_max(A);
    double sv = sqrt(lam > 0.0 ? lam : 0.0);
    if (sv < 1e-6) sv = 1e-6;
    const double lg = log(sv);
    regp[p] = lg * lg;
}
extern "C" __global__ void __launch_bounds__(256)
k_nrf_reg_mean(const double *regp, int n, float *reg) {                        // fixed-order mean (one workgroup)
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += regp[i];
    s = block_fold_one(s, red, FoldSum());
    if (threadIdx.x == 0) reg[0] = (float)(s / (double)n);
}

// ---- backward of the head stage per point: dO[p][i] = <g, d warp / d o_i>  (six forward-mode passes; zero rows beyond n) ----
extern "C" __global__ void __launch_bounds__(256)
k_nrf_head_bwd(const float *heads, const float *x, const float *g, int n, int plane, float *dO /*[plane][16]*/) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    float4 *o4 = reinterpret_cast<float4 *>(dO + (size_t)p * NDP_NHMAX);
    const float4 z4 = make_float4(0.f, 0.f, 0.f, 0.f);
    float r[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (p < n) {
        float o[6];
#pragma unroll
        for (int j = 0; j < 6; ++j) o[j] = heads[(size_t)p * 8 + j];
        const Dualf xd[3] = {{x[3 * (size_t)p], 0.f}, {x[3 * (size_t)p + 1], 0.f}, {x[3 * (size_t)p + 2], 0.f}};
        const float gv[3] = {g[3 * (size_t)p], g[3 * (size_t)p + 1], g[3 * (size_t)p + 2]};
#pragma unroll
        for (int i = 0; i < 6; ++i) {
            Dualf od[6], out[3];
#pragma unroll
            for (int j = 0; j < 6; ++j) od[j] = {o[j], j == i ? 1.f : 0.f};
            nrf_se3_warp(od, xd, out);
            r[i] = gv[0] * out[0].d + gv[1] * out[1].d + gv[2] * out[2].d;
        }
    }
    o4[0] = make_float4(r[0], r[1], r[2], r[3]);
    o4[1] = make_float4(r[4], r[5], 0.f, 0.f);
    o4[2] = z4; o4[3] = z4;
}

// ---- input layer backward: dW_in[o][c] += sum_p dz0[p][o] pe[p][c] ; db_in[o] += sum_p dz0[p][o] -------------------------
// thread = (output o = t & 127, half of the tile's points t >> 7); one partial per workgroup
extern "C" __global__ void __launch_bounds__(256)
k_nrf_in_bwd(const float *dz0 /*[cap][128]*/, const float *pe /*[cap][40]*/, int n, int n_tiles, float *gpart, int p_stride) {
    __shared__ __attribute__((aligned(16))) float pes[64 * NRF_PES];
    __shared__ float comb[NDP_W * (NRF_PES + 1)];
    const int t = threadIdx.x, o = t & 127, half = t >> 7;
    float acc[NRF_PES];
#pragma unroll
    for (int c = 0; c < NRF_PES; ++c) acc[c] = 0.f;                            // acc[39]: the bias gradient
    for (int tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int base = tile * NDP_TILE;
        __syncthreads();
        for (int i = t; i < 64 * NRF_PES; i += 256) pes[i] = pe[(size_t)base * NRF_PES + i];
        __syncthreads();
        for (int q = 0; q < 32; ++q) {
            const int pl = 32 * half + q;
            if (base + pl >= n) break;
            const float z = dz0[(size_t)(base + pl) * NDP_W + o];
            const float4 *pr = reinterpret_cast<const float4 *>(pes + pl * NRF_PES);
#pragma unroll
            for (int c4 = 0; c4 < NRF_PES / 4; ++c4) {
                const float4 v = pr[c4];
                acc[4 * c4] = fmaf(z, v.x, acc[4 * c4]); acc[4 * c4 + 1] = fmaf(z, v.y, acc[4 * c4 + 1]);
                acc[4 * c4 + 2] = fmaf(z, v.z, acc[4 * c4 + 2]);
                if (4 * c4 + 3 < NRF_PE) acc[4 * c4 + 3] = fmaf(z, v.w, acc[4 * c4 + 3]);
                else acc[NRF_PE] += z;                                         // slot 39 of the saved row is padding: use it for db
            }
        }
    }
    __syncthreads();
    if (half == 1) {
#pragma unroll
        for (int c = 0; c < NRF_PES; ++c) comb[o * (NRF_PES + 1) + c] = acc[c];
    }
    __syncthreads();
    if (half == 0) {
        float *G = gpart + (size_t)blockIdx.x * p_stride;
#pragma unroll
        for (int c = 0; c < NRF_PE; ++c) G[o * NRF_PE + c] = acc[c] + comb[o * (NRF_PES + 1) + c];
        G[NDP_W * NRF_PE + o] = acc[NRF_PE] + comb[o * (NRF_PES + 1) + NRF_PE];
    }
}

static constexpr int kSmemNrfDenseBytes = 2 * 64 * NDP_LD * 4;

extern "C" int ndp_nerfies_fwd(const float *params, const float *x, int n, const float *window6, float *x_out, float *J,
                               float *reg, float *act, int save, float *pe, float *heads, double *work, void *stream) {
    if (n <= 0 || !params || !x || !window6 || !x_out || !J || !reg || !act || !pe || !heads || !work)
        return fail(NDP_E_INVALID, "ndp_nerfies_fwd: null pointer / bad n");
    if (!aligned16(params) || !aligned16(act) || !aligned16(pe) || !aligned16(heads))
        return fail(NDP_E_INVALID, "ndp_nerfies_fwd: params/act/pe/heads must be 16-byte aligned");
    if (int rc = set_smem((const void *)k_nrf_dense, kSmemNrfDenseBytes)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int n_tiles = (n + NDP_TILE - 1) / NDP_TILE, cap = n_tiles * NDP_TILE;
    const size_t psz = 4 * (size_t)cap * NDP_W;                               // one activation buffer: four planes
    NrfWindow win;
    for (int j = 0; j < 6; ++j) win.w[j] = window6[j];
    float *cur = act;
    hipLaunchKernelGGL(k_nrf_in, dim3(n_tiles), dim3(256), 0, s, params, x, n, cap, win, pe, cur);
    const int grid = n_tiles < 512 ? n_tiles : 512;
    for (int l = 1; l <= NRF_HID; ++l) {
        float *nxt = save ? act + (size_t)l * psz : (cur == act ? act + psz : act);
        hipLaunchKernelGGL(k_nrf_dense, dim3(grid), dim3(256), kSmemNrfDenseBytes, s, params + nrf_off_W(l), params + nrf_off_b(l),
                           cur, nxt, cap, n_tiles);
        cur = nxt;
    }
    hipLaunchKernelGGL(k_nrf_heads, dim3(4 * n_tiles), dim3(256), 0, s, params, cur, heads, cap);
    hipLaunchKernelGGL(k_nrf_warp, dim3((n + 255) / 256), dim3(256), 0, s, heads, x, n, cap, x_out, J, work);
    hipLaunchKernelGGL(k_nrf_reg_mean, dim3(1), dim3(256), 0, s, work, n, reg);
    HIP_TRY(hipGetLastError(), "nerfies forward launch");
    return 0;
}

extern "C" int ndp_nerfies_bwd(const float *params, const float *x, int n, float *act, const float *pe, const float *heads,
                               const float *g, float *dO_work, float *grads_part, int n_part, int p_stride, void *stream) {
    if (n <= 0 || !params || !x || !act || !pe || !heads || !g || !dO_work || !grads_part || n_part < 1)
        return fail(NDP_E_INVALID, "ndp_nerfies_bwd: null pointer / bad sizes");
    if (p_stride < nrf_param_count()) return fail(NDP_E_INVALID, "ndp_nerfies_bwd: p_stride < P");
    if (!aligned16(params) || !aligned16(act) || !aligned16(dO_work) || !aligned16(pe))
        return fail(NDP_E_INVALID, "ndp_nerfies_bwd: params/act/dO_work/pe must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    BwdJob job;
    memset(&job, 0, sizeof job);
    job.params = params; job.dO = dO_work; job.gpart = grads_part;
    job.n = n; job.n_tiles = (n + NDP_TILE - 1) / NDP_TILE; job.plane = job.n_tiles * NDP_TILE;
    const size_t psz = 4 * (size_t)job.plane * NDP_W;
    if (n_part > job.n_tiles) {                                  // partials with no tile must read as zero
        HIP_TRY(hipMemsetAsync(grads_part + (size_t)job.n_tiles * p_stride, 0,
                               sizeof(float) * (size_t)(n_part - job.n_tiles) * p_stride, s), "memset");
        n_part = job.n_tiles;
    }
    if (int rc = set_smem((const void *)k_level_bwd2, kSmemBwdBytes)) return rc;
    ndp_layer_desc d3 = {NDP_W, 2, NDP_MOTION_SFLOW, NDP_ROT_AXIS_ANGLE, 0, 1.0f};
    const HeadCfg hc = make_head_cfg(d3);
    hipLaunchKernelGGL(k_nrf_head_bwd, dim3((job.plane + 255) / 256), dim3(256), 0, s, heads, x, g, n, job.plane, dO_work);
    // hidden layers 6..1 on the PRIMAL plane (rows 0 .. cap of every activation buffer): layer 6 recomputes its dz from dO
    // through the six head rows, the layers below read the dz the layer above left in the plane (h6's buffer, in place)
    float *dz = act + (size_t)NRF_HID * psz;
    job.dz_plane = dz;
    for (int l = NRF_HID; l >= 1; --l) {
        job.h_plane = act + (size_t)(l - 1) * psz;
        job.w_off = nrf_off_W(l); job.b_off = nrf_off_b(l);
        job.from_dO = l == NRF_HID; job.wh_off = nrf_off_Wh(); job.nh = 6;
        hipLaunchKernelGGL(k_level_bwd2, dim3(n_part), dim3(256), kSmemBwdBytes, s, hc, job, p_stride);
    }
    hipLaunchKernelGGL(k_nrf_in_bwd, dim3(n_part), dim3(256), 0, s, dz, pe, n, job.n_tiles, grads_part, p_stride);
    HIP_TRY(hipGetLastError(), "nerfies backward launch");
    return 0;
}
