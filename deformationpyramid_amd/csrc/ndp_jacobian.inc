// ndp_jacobian.inc -- the pyramid warp together with its per-point Jacobian J = d x' / d x (3 x 3), the inverse warp (Newton on
// W(x) = y, all iterations of a tile inside ONE launch) and the transport of normals n' ~ J^-T n.
//
// A workgroup carries one 64-point tile through levels min_level .. max_level without intermediate HBM traffic, like k_pyramid_fwd
// and k_gen_pyramid_fwd.  Per level the network is walked FOUR times -- the four-plane layout [primal | d/dx0 | d/dx1 | d/dx2] of
// ndp_nerfies.inc, one plane after another so that two activation buffers serve all of them (at width 256 the two buffers are 133 KB
// of the 160 KB of LDS):
//   primal   : the operations of fwd_tile_core (128 / 3) resp. gen_tile_core (every other shape), in their order -- the x' produced
//              here is bit for bit the x' of ndp_pyramid_fwd.  Behind every ReLU layer its mask [pre-activation > 0] is packed into one
//              bit per feature (at most 4 layers x 8 words x 64 points = 8 KB);
//   tangent a: layer 0 is W0 applied to f (cos, -sin) of the primal encoding of coordinate a (ONE k-step of the fp32 MFMA: the level's
//              tangents are seeded with the identity), every later layer (W t_in) . mask with no bias, the head rows mlp_scale Wh t.
// All contractions on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation); no fp16 split here: J feeds a solver.
// Then one wave, lane = point:  J_level = D + A T,  T [heads][3] from the tangent planes, and row a of D (3 x 3, the warp's direct
// dependence on x) and of A (3 x heads, d x' / d heads) from head_warp_bwd of ndp_device.h called with g = e_a -- the head maths of
// every rotation format, motion and the nonrigidity gate that the level backward already uses.  Running product J <- J_level J.
// Every point is written by one thread in a fixed order: results do not depend on n or on tile boundaries.
#define JAC_HO4 (4 * 64 * NDP_NHMAX)          /* head outputs of the four planes */
#define JAC_MKW_GEN 8                          /* mask words per point and layer: 256 features */
#define JAC_MKW_MFMA 4

struct JacLds {
    float *pe, *xs, *ho4, *rows;               // encoding [64][9]; points [64][4]; [4][64][16]; [64][16] private rows of head_warp_bwd
    unsigned *mk;                              // [layer][word][64]
    int *flag;
};
// generic carve (floats): the two activation buffers (rows aliases them: it is only used when every plane is done), pe, xs, ho4, mk, flag
__host__ __device__ inline int jac_gen_bufs(int W) { const int b = 2 * gen_buf(W); return b > 64 * NDP_NHMAX ? b : 64 * NDP_NHMAX; }
__host__ __device__ inline int jac_gen_floats(int W) { return jac_gen_bufs(W) + 64 * 9 + 64 * 4 + JAC_HO4 + (GEN_HMAX + 1) * JAC_MKW_GEN * 64 + 4; }
static constexpr int kSmemJacGenMax = (2 * GEN_WMAX * GEN_PS + 64 * 9 + 64 * 4 + JAC_HO4 + (GEN_HMAX + 1) * JAC_MKW_GEN * 64 + 4) * 4;
static constexpr int kSmemJacBytes = (L_FWD_TOTAL + JAC_HO4 + 3 * JAC_MKW_MFMA * 64 + 4) * 4;
static_assert(kSmemJacGenMax <= 160 * 1024 && kSmemJacBytes <= 160 * 1024, "Jacobian kernels: LDS carve");

template <bool GEN>
__device__ __forceinline__ JacLds jac_lds(float *sm, int W) {
    JacLds L;
    if (GEN) {
        L.pe = sm + jac_gen_bufs(W);
        L.xs = L.pe + 64 * 9;
        L.ho4 = L.xs + 64 * 4;
        L.mk = reinterpret_cast<unsigned *>(L.ho4 + JAC_HO4);
        L.flag = reinterpret_cast<int *>(L.mk + (GEN_HMAX + 1) * JAC_MKW_GEN * 64);
    } else {
        L.pe = sm + L_PE;
        L.xs = sm + L_XS;
        L.ho4 = sm + L_FWD_TOTAL;
        L.mk = reinterpret_cast<unsigned *>(L.ho4 + JAC_HO4);
        L.flag = reinterpret_cast<int *>(L.mk + 3 * JAC_MKW_MFMA * 64);
    }
    L.rows = sm;
    return L;
}

// d pe[2 a + h] / d x_a of point p from the primal encoding: f cos (h = 0), -f sin (h = 1)
__device__ __forceinline__ float jac_dpe(const float *pe, int p, int a, int h, float freq) {
    return h == 0 ? freq * pe[p * 9 + 2 * a + 1] : -(freq * pe[p * 9 + 2 * a]);
}

// ---- 128 / 3 ---------------------------------------------------------------------------------------------------------------------------
// mask word of (point, 32-feature block) from a [64][NDP_LD] tile of post-ReLU activations
__device__ __forceinline__ void jac_pack_mfma(const float *buf, unsigned *mkl /* [4][64] */) {
    const int p = threadIdx.x >> 2, w = threadIdx.x & 3;
    const float *src = buf + p * NDP_LD + 32 * w;
    unsigned bits = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 v = *reinterpret_cast<const float4 *>(src + 4 * i);
        bits |= (v.x > 0.f ? 1u : 0u) << (4 * i) | (v.y > 0.f ? 2u : 0u) << (4 * i) | (v.z > 0.f ? 4u : 0u) << (4 * i) | (v.w > 0.f ? 8u : 0u) << (4 * i);
    }
    mkl[w * 64 + p] = bits;
}
// epilogue of tile_gemm_64x32 for a tangent plane: [p][32 wv + 8 g + 4 h .. + 3] <- acc where the primal's bit is set
__device__ __forceinline__ void jac_epilogue_bits(const f32x16 &acc0, const f32x16 &acc1, const unsigned *mkl, float *out, int wv, int l31, int h) {
    const unsigned m0 = mkl[wv * 64 + l31] >> (4 * h), m1 = mkl[wv * 64 + l31 + 32] >> (4 * h);
    float *o0 = out + l31 * NDP_LD + 32 * wv + 4 * h, *o1 = o0 + 32 * NDP_LD;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const unsigned b0 = m0 >> (8 * g), b1 = m1 >> (8 * g);
        *reinterpret_cast<float4 *>(o0 + 8 * g) = make_float4(b0 & 1 ? acc0[4 * g] : 0.f, b0 & 2 ? acc0[4 * g + 1] : 0.f,
                                                                b0 & 4 ? acc0[4 * g + 2] : 0.f, b0 & 8 ? acc0[4 * g + 3] : 0.f);
        *reinterpret_cast<float4 *>(o1 + 8 * g) = make_float4(b1 & 1 ? acc1[4 * g] : 0.f, b1 & 2 ? acc1[4 * g + 1] : 0.f,
                                                                b1 & 4 ? acc1[4 * g + 2] : 0.f, b1 & 8 ? acc1[4 * g + 3] : 0.f);
    }
}
// One plane of the tile through the level's network -> ho4[a + 1] (a = -1: the primal plane, the arithmetic of fwd_tile_core, which
// also leaves the three masks; a = 0..2: the tangent d/dx_a).  Ends with a barrier.
__device__ __forceinline__ void jac_mfma_plane(const HeadCfg &hc, const FwdWeights &fw, float *sm, const JacLds &L, int a, float freq) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    float *bufA = sm + L_BUFA, *bufB = sm + L_BUFB;
    const float *whs = sm + L_WH, *bhs = sm + L_BH;
    float *ho = L.ho4 + (a + 1) * 64 * NDP_NHMAX;
    const bool tan = a >= 0;
    {
        f32x16 acc0, acc1;
        acc_init_bias(tan ? 0.f : fw.bias0, h, acc0, acc1);
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            float b0 = L.pe[l31 * 9 + 2 * ks + h], b1 = L.pe[(l31 + 32) * 9 + 2 * ks + h];
            if (tan) {
                b0 = ks == a ? jac_dpe(L.pe, l31, ks, h, freq) : 0.f;
                b1 = ks == a ? jac_dpe(L.pe, l31 + 32, ks, h, freq) : 0.f;
            }
            acc0 = MFMA32(fw.w0b[ks], b0, acc0);
            acc1 = MFMA32(fw.w0b[ks], b1, acc1);
        }
        if (tan) jac_epilogue_bits(acc0, acc1, L.mk, bufA, wv, l31, h);
        else epilogue_relu(acc0, acc1, bufA, wv, l31, h);
    }
    __syncthreads();
    {
        f32x16 acc0, acc1;
        acc_init_bias(tan ? 0.f : fw.bias1, h, acc0, acc1);
        if (!tan) jac_pack_mfma(bufA, L.mk);
        tile_gemm_64x32(bufA, fw.w1, l31, h, acc0, acc1);
        if (tan) jac_epilogue_bits(acc0, acc1, L.mk + JAC_MKW_MFMA * 64, bufB, wv, l31, h);
        else epilogue_relu(acc0, acc1, bufB, wv, l31, h);
    }
    __syncthreads();
    {
        f32x16 acc0, acc1;
        acc_init_bias(tan ? 0.f : fw.bias2, h, acc0, acc1);
        if (!tan) jac_pack_mfma(bufB, L.mk + JAC_MKW_MFMA * 64);
        tile_gemm_64x32(bufB, fw.w2, l31, h, acc0, acc1);
        if (tan) jac_epilogue_bits(acc0, acc1, L.mk + 2 * JAC_MKW_MFMA * 64, bufA, wv, l31, h);
        else epilogue_relu(acc0, acc1, bufA, wv, l31, h);
    }
    __syncthreads();
    if (!tan) jac_pack_mfma(bufA, L.mk + 2 * JAC_MKW_MFMA * 64);
    {   // heads on the 16x16x4 MFMA as in fwd_tile_core; a tangent plane has no bias
        const int l15 = lane & 15, lk = lane >> 4;
        f32x4 acc;
        const float bj = tan ? 0.f : bhs[l15];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = bj;
        const float *arow = bufA + (16 * wv + l15) * NDP_LD + 4 * lk;
        const float *brow = whs + (l15 < NDP_WHROWS ? l15 : 0) * NDP_LD + 4 * lk;
        const bool live = l15 < NDP_WHROWS;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 av = *reinterpret_cast<const float4 *>(arow + 16 * q);
            float4 b = *reinterpret_cast<const float4 *>(brow + 16 * q);
            if (!live) b = make_float4(0.f, 0.f, 0.f, 0.f);
            acc = MFMA16(av.x, b.x, acc);
            acc = MFMA16(av.y, b.y, acc);
            acc = MFMA16(av.z, b.z, acc);
            acc = MFMA16(av.w, b.w, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ho[(16 * wv + 4 * lk + r) * NDP_NHMAX + l15] = hc.mlp_scale * acc[r];
    }
    __syncthreads();
}

// ---- every other width / depth -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void jac_pack_gen(const float *buf /*[feature][GEN_PS]*/, int W, unsigned *mkl /* [8][64] */) {
    const int nw = (W + 31) >> 5;
    for (int idx = threadIdx.x; idx < nw * 64; idx += 256) {
        const int p = idx & 63, w = idx >> 6;
        const int nb = W - 32 * w < 32 ? W - 32 * w : 32;
        unsigned bits = 0;
        for (int j = 0; j < nb; ++j) bits |= (buf[(32 * w + j) * GEN_PS + p] > 0.f ? 1u : 0u) << j;
        mkl[w * 64 + p] = bits;
    }
}
// gen_dense without a bias: out[o] = sum_k W[o][k] in[k] (k ascending from zero), times the primal's mask bit (mkl) or times `scale`
// (mkl == nullptr: the head rows)
__device__ __forceinline__ void jac_gen_dense(const float *Wm, int n_out, int n_in, const float *in /*[k][GEN_PS]*/, float *out, int out_os,
                                              int out_ps, const unsigned *mkl, float scale) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    for (int ob = 32 * wv; ob < n_out; ob += 128) {
        const int o = ob + l31 < n_out ? ob + l31 : n_out - 1;
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
        const float *wr = Wm + (size_t)o * n_in + h;
        const float *i0 = in + h * GEN_PS + l31, *i1 = i0 + 32;
        const int n2 = n_in & ~1;
#pragma unroll 8
        for (int k = 0; k < n2; k += 2) {
            const float a = wr[k];
            acc0 = MFMA32(a, i0[k * GEN_PS], acc0);
            acc1 = MFMA32(a, i1[k * GEN_PS], acc1);
        }
        if (n_in & 1) {
            const float a = h == 0 ? wr[n2] : 0.f, b0 = h == 0 ? i0[n2 * GEN_PS] : 0.f, b1 = h == 0 ? i1[n2 * GEN_PS] : 0.f;
            acc0 = MFMA32(a, b0, acc0);
            acc1 = MFMA32(a, b1, acc1);
        }
        const unsigned m0 = mkl ? mkl[(ob >> 5) * 64 + l31] : 0u, m1 = mkl ? mkl[(ob >> 5) * 64 + l31 + 32] : 0u;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma_row(r, h), orow = ob + row;
            if (orow < n_out) {
                float *q = out + orow * out_os + l31 * out_ps;
                q[0] = mkl ? ((m0 >> row) & 1 ? acc0[r] : 0.f) : scale * acc0[r];
                q[32 * out_ps] = mkl ? ((m1 >> row) & 1 ? acc1[r] : 0.f) : scale * acc1[r];
            }
        }
    }
}
// layer 0 of tangent a: one k-step, W0[o][2 a + h] against f (cos, -sin) of the primal encoding
__device__ __forceinline__ void jac_gen_l0(const float *W0, int W, int a, const float *pe, float freq, float *out, const unsigned *mkl) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    const float b0 = jac_dpe(pe, l31, a, h, freq), b1 = jac_dpe(pe, l31 + 32, a, h, freq);
    for (int ob = 32 * wv; ob < W; ob += 128) {
        const int o = ob + l31 < W ? ob + l31 : W - 1;
        f32x16 z;
#pragma unroll
        for (int r = 0; r < 16; ++r) z[r] = 0.f;
        const float wa = W0[o * 6 + 2 * a + h];
        const f32x16 acc0 = MFMA32(wa, b0, z), acc1 = MFMA32(wa, b1, z);
        const unsigned m0 = mkl[(ob >> 5) * 64 + l31], m1 = mkl[(ob >> 5) * 64 + l31 + 32];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mfma_row(r, h), orow = ob + row;
            if (orow < W) {
                out[orow * GEN_PS + l31] = (m0 >> row) & 1 ? acc0[r] : 0.f;
                out[orow * GEN_PS + l31 + 32] = (m1 >> row) & 1 ? acc1[r] : 0.f;
            }
        }
    }
}
// the generic form of jac_mfma_plane: the primal plane is gen_tile_core's sequence of gen_dense calls
__device__ __forceinline__ void jac_gen_plane(const HeadCfg &hc, const ndp_layer_desc &d, const float *params, float *sm, const JacLds &L,
                                              int a, float freq) {
    const int W = d.width;
    float *cur = sm, *nxt = sm + gen_buf(W);
    float *ho = L.ho4 + (a + 1) * 64 * NDP_NHMAX;
    if (a < 0) {
        gen_dense<true>(params + ndp_off_W0(&d), params + ndp_off_b0(&d), W, 6, L.pe, 1, 9, cur, GEN_PS, 1, 1.0f);
        __syncthreads();
        jac_pack_gen(cur, W, L.mk);
        for (int l = 1; l <= d.n_hidden; ++l) {
            gen_dense<true>(params + ndp_off_Wi(&d, l), params + ndp_off_bi(&d, l), W, W, cur, GEN_PS, 1, nxt, GEN_PS, 1, 1.0f);
            __syncthreads();
            jac_pack_gen(nxt, W, L.mk + l * JAC_MKW_GEN * 64);
            float *sw = cur; cur = nxt; nxt = sw;
        }
        gen_dense<false>(params + ndp_off_Wh(&d), params + ndp_off_bh(&d), hc.nh, W, cur, GEN_PS, 1, ho, 1, NDP_NHMAX, hc.mlp_scale);
    } else {
        jac_gen_l0(params + ndp_off_W0(&d), W, a, L.pe, freq, cur, L.mk);
        __syncthreads();
        for (int l = 1; l <= d.n_hidden; ++l) {
            jac_gen_dense(params + ndp_off_Wi(&d, l), W, W, cur, nxt, GEN_PS, 1, L.mk + l * JAC_MKW_GEN * 64, 1.0f);
            __syncthreads();
            float *sw = cur; cur = nxt; nxt = sw;
        }
        jac_gen_dense(params + ndp_off_Wh(&d), hc.nh, W, cur, ho, 1, NDP_NHMAX, nullptr, hc.mlp_scale);
    }
    if (threadIdx.x < 64)
        for (int j = hc.nh; j < NDP_NHMAX; ++j) ho[threadIdx.x * NDP_NHMAX + j] = 0.f;
    __syncthreads();
}

// ---- per point -----------------------------------------------------------------------------------------------------------------------------
// cofactor matrix C of J (rows r1 x r2, r2 x r0, r0 x r1: J^-1 = C^T / det, J^-T = C / det) and det J
__device__ __forceinline__ float jac_cofactor(const float *J, float *C) {
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const float *u = J + 3 * ((a + 1) % 3), *v = J + 3 * ((a + 2) % 3);
        C[3 * a] = u[1] * v[2] - u[2] * v[1];
        C[3 * a + 1] = u[2] * v[0] - u[0] * v[2];
        C[3 * a + 2] = u[0] * v[1] - u[1] * v[0];
    }
    float det = J[0] * C[0];
    det = fmaf(J[1], C[1], det);
    det = fmaf(J[2], C[2], det);
    return det;
}
// The level's warp of the lane's point (fwd_warp's head_warp_fwd on the same operands: the same bits) and J <- J_level J.
__device__ __forceinline__ void jac_point_level(const HeadCfg &hc, const JacLds &L, int lane, float (&J)[9]) {
    const float *o = L.ho4 + lane * NDP_NHMAX;
    float *x = L.xs + 4 * lane;
    float *row = L.rows + lane * NDP_NHMAX;
    PointHead c;
    float out[3], Jl[9];
    head_warp_fwd(hc, o, x, c, out);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
#pragma unroll
        for (int j = 0; j < NDP_NHMAX; j += 4) *reinterpret_cast<float4 *>(row + j) = *reinterpret_cast<const float4 *>(o + j);
        const float g[3] = {a == 0 ? 1.f : 0.f, a == 1 ? 1.f : 0.f, a == 2 ? 1.f : 0.f};
        float direct[3];
        head_warp_bwd(hc, x, c, g, 0.f, row, direct);              // row <- row a of A, direct <- row a of D
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            const float *T = L.ho4 + (b + 1) * 64 * NDP_NHMAX + lane * NDP_NHMAX;
            float s = direct[b];
            for (int j = 0; j < hc.nh; ++j) s = fmaf(row[j], T[j], s);
            Jl[3 * a + b] = s;
        }
    }
    float Jn[9];
    mat3_mul(Jl, J, Jn);
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = Jn[i];
    x[0] = out[0]; x[1] = out[1]; x[2] = out[2];
}

// The tile's points (L.xs, visible to every wave on entry) through levels lo .. hi: L.xs <- W(x), and in wave 0's lanes that hold a
// point (`mine`) J <- d W / d x.  Ends with a barrier.
template <bool GEN>
__device__ __forceinline__ void jac_tile_levels(const ndp_layer_desc &desc, int k0, const float *params_all, int p_stride, int lo, int hi,
                                                float *sm, const JacLds &L, bool mine, float (&J)[9]) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 9; ++i) J[i] = (i == 0 || i == 4 || i == 8) ? 1.f : 0.f;
    for (int l = lo; l <= hi; ++l) {
        const ndp_layer_desc dl = desc_at_level(desc, l);
        const HeadCfg hc = make_head_cfg(dl);
        const float *P = params_all + (size_t)l * p_stride;
        const float freq = ldexpf(1.0f, l + 1 + k0);
        if (GEN) {
            if (wv > 0) fwd_posenc(L.xs[4 * lane + wv - 1], freq, lane, wv - 1, L.pe, L.xs, false);
            __syncthreads();
#pragma unroll 1
            for (int a = -1; a < 3; ++a) jac_gen_plane(hc, dl, P, sm, L, a, freq);
        } else {
            FwdWeights fw;
            fwd_load_weights(hc, P, sm, fw);
            if (wv > 0) fwd_posenc(L.xs[4 * lane + wv - 1], freq, lane, wv - 1, L.pe, L.xs, false);
            __syncthreads();
#pragma unroll 1
            for (int a = -1; a < 3; ++a) jac_mfma_plane(hc, fw, sm, L, a, freq);
        }
        if (mine) jac_point_level(hc, L, lane, J);
        __syncthreads();
    }
}

template <bool GEN>
__device__ __forceinline__ void jac_body(const ndp_layer_desc &desc, int k0, const float *params_all, int p_stride, int lo, int hi,
                                         const float *x, int n, float *x_out, float *Jout, const float *nin, float *nout, float *sm) {
    const JacLds L = jac_lds<GEN>(sm, desc.width);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t p = (size_t)blockIdx.x * NDP_TILE + lane;
    const bool mine = wv == 0 && p < (size_t)n;
    if (wv == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) L.xs[4 * lane + k] = mine ? x[3 * p + k] : 0.f;
    }
    __syncthreads();
    float J[9];
    jac_tile_levels<GEN>(desc, k0, params_all, p_stride, lo, hi, sm, L, mine, J);
    if (!mine) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) x_out[3 * p + k] = L.xs[4 * lane + k];
#pragma unroll
    for (int i = 0; i < 9; ++i) Jout[9 * p + i] = J[i];
    if (nout) {
        float C[9], v[3];
        jac_cofactor(J, C);
        const float n0 = nin[3 * p], n1 = nin[3 * p + 1], n2 = nin[3 * p + 2];
#pragma unroll
        for (int a = 0; a < 3; ++a) v[a] = fmaf(C[3 * a + 2], n2, fmaf(C[3 * a + 1], n1, C[3 * a] * n0));
        // a vector whose squared length is within 2^-21 of 1 is unit to fp32 accuracy (what normalising in fp32 leaves behind) and is
        // written as it is: renormalising it would only move its last bits, and unit normals pass an identity warp unchanged
        const float s2 = fmaf(v[2], v[2], fmaf(v[1], v[1], v[0] * v[0]));
        const float len = fabsf(s2 - 1.0f) <= 0x1p-21f ? 1.0f : sqrtf(s2);
#pragma unroll
        for (int a = 0; a < 3; ++a) nout[3 * p + a] = v[a] / len;
    }
}

// Newton on W(x) = y for the tile's points, every iteration inside this launch (tiles are independent).  it = 0, 1, ..: evaluate W(x)
// and J; a point whose max |W(x) - y| <= tol is frozen with status = it (the steps it took); otherwise, while it < iters, it steps
// x <- x - J^-1 r (3 x 3 solve through the cofactor matrix).  A point that is still open after `iters` steps keeps status -1; one with
// non-finite values or |det J| < 1e-12 stops with -2.  The residual written is always that of the x written.
template <bool GEN>
__device__ __forceinline__ void inverse_body(const ndp_layer_desc &desc, int k0, const float *params_all, int p_stride, int lo, int hi,
                                             const float *y, int n, float *x, int iters, float tol, float *residual, int *status, float *sm) {
    const JacLds L = jac_lds<GEN>(sm, desc.width);
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const size_t p = (size_t)blockIdx.x * NDP_TILE + lane;
    const bool mine = wv == 0 && p < (size_t)n;
    bool open = mine;
    float yv[3] = {0.f, 0.f, 0.f}, xc[3] = {0.f, 0.f, 0.f}, res = 0.f;
    int st = -1;
    if (wv == 0) {
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (mine) { yv[k] = y[3 * p + k]; xc[k] = x[3 * p + k]; }
            L.xs[4 * lane + k] = xc[k];
        }
    }
    __syncthreads();
    for (int it = 0;; ++it) {
        float J[9];
        jac_tile_levels<GEN>(desc, k0, params_all, p_stride, lo, hi, sm, L, mine, J);
        if (wv == 0) {
            if (open) {
                float r[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) r[k] = L.xs[4 * lane + k] - yv[k];
                res = fmaxf(fabsf(r[0]), fmaxf(fabsf(r[1]), fabsf(r[2])));
                const bool finite = __builtin_isfinite(r[0]) && __builtin_isfinite(r[1]) && __builtin_isfinite(r[2]);
                if (!finite) { st = -2; open = false; res = r[0] + r[1] + r[2]; }
                else if (res <= tol) { st = it; open = false; }
                else if (it >= iters) open = false;
                else {
                    float C[9];
                    const float det = jac_cofactor(J, C);
                    if (!__builtin_isfinite(det) || fabsf(det) < 1e-12f) { st = -2; open = false; }
                    else {
#pragma unroll
                        for (int b = 0; b < 3; ++b) xc[b] -= fmaf(C[6 + b], r[2], fmaf(C[3 + b], r[1], C[b] * r[0])) / det;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) L.xs[4 * lane + k] = xc[k];
            const bool any = __ballot(open) != 0;
            if (lane == 0) *L.flag = any ? 1 : 0;
        }
        __syncthreads();
        if (!*L.flag) break;
    }
    if (!mine) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) x[3 * p + k] = xc[k];
    residual[p] = res;
    status[p] = st;
}

struct JacArgs {
    ndp_layer_desc desc;
    int k0, p_stride, lo, hi, n;
    const float *params;
};
extern "C" __global__ void __launch_bounds__(256)
k_pyramid_jac(JacArgs q, const float *x, float *x_out, float *J, const float *nin, float *nout) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    jac_body<false>(q.desc, q.k0, q.params, q.p_stride, q.lo, q.hi, x, q.n, x_out, J, nin, nout, sm);
}
extern "C" __global__ void __launch_bounds__(256)
k_gen_pyramid_jac(JacArgs q, const float *x, float *x_out, float *J, const float *nin, float *nout) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    jac_body<true>(q.desc, q.k0, q.params, q.p_stride, q.lo, q.hi, x, q.n, x_out, J, nin, nout, sm);
}
extern "C" __global__ void __launch_bounds__(256)
k_pyramid_inverse(JacArgs q, const float *y, float *x, int iters, float tol, float *residual, int *status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    inverse_body<false>(q.desc, q.k0, q.params, q.p_stride, q.lo, q.hi, y, q.n, x, iters, tol, residual, status, sm);
}
extern "C" __global__ void __launch_bounds__(256)
k_gen_pyramid_inverse(JacArgs q, const float *y, float *x, int iters, float tol, float *residual, int *status) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    inverse_body<true>(q.desc, q.k0, q.params, q.p_stride, q.lo, q.hi, y, q.n, x, iters, tol, residual, status, sm);
}

// ---- host ----------------------------------------------------------------------------------------------------------------------------------
static bool aligned4(const void *p) { return ((uintptr_t)p & 3) == 0; }
// what both entries refuse before any launch
static int jac_check(const char *who, const ndp_layer_desc *desc, int m, int k0, const float *params_all, int p_stride, int min_level,
                     int max_level, int n, JacArgs &q) {
    char msg[200];
    if (int rc = check_desc(desc)) return rc;
    if (n <= 0) { snprintf(msg, sizeof msg, "%s: n must be positive", who); return fail(NDP_E_INVALID, msg); }
    if (m < 1 || m > NDP_MAX_LEVELS || min_level < 0 || max_level >= m || min_level > max_level) {
        snprintf(msg, sizeof msg, "%s: levels need 1 <= m <= 16 and 0 <= min_level <= max_level < m", who);
        return fail(NDP_E_INVALID, msg);
    }
    if (min_level + 1 + k0 < -126 || max_level + 1 + k0 > 127) {
        snprintf(msg, sizeof msg, "%s: 2^(level + 1 + k0) must be in float range", who);
        return fail(NDP_E_INVALID, msg);
    }
    if (p_stride < ndp_param_count(desc) || (p_stride & 3)) {
        snprintf(msg, sizeof msg, "%s: p_stride must hold the level's parameters and be a multiple of 4", who);
        return fail(NDP_E_INVALID, msg);
    }
    if (!params_all || !aligned16(params_all)) {
        snprintf(msg, sizeof msg, "%s: params_all must be non-null and 16-byte aligned", who);
        return fail(NDP_E_INVALID, msg);
    }
    q.desc = *desc; q.k0 = k0; q.p_stride = p_stride; q.lo = min_level; q.hi = max_level; q.n = n; q.params = params_all;
    return 0;
}

extern "C" int ndp_pyramid_jac(const ndp_layer_desc *desc, int m, int k0, const float *params_all, int p_stride, int min_level,
                               int max_level, const float *x, int n, float *x_out, float *J, const float *normals_in,
                               float *normals_out, void *stream) {
    JacArgs q;
    if (int rc = jac_check("ndp_pyramid_jac", desc, m, k0, params_all, p_stride, min_level, max_level, n, q)) return rc;
    if (!x || !x_out || !J || !aligned4(x) || !aligned4(x_out) || !aligned4(J))
        return fail(NDP_E_INVALID, "ndp_pyramid_jac: x, x_out and J must be non-null and 4-byte aligned");
    if ((normals_in == nullptr) != (normals_out == nullptr))
        return fail(NDP_E_INVALID, "ndp_pyramid_jac: normals_in and normals_out go together");
    if (normals_in && (!aligned4(normals_in) || !aligned4(normals_out)))
        return fail(NDP_E_INVALID, "ndp_pyramid_jac: normals must be 4-byte aligned");
    const int tiles = (n + NDP_TILE - 1) / NDP_TILE;
    if (gen_is_generic(*desc)) {
        if (int rc = set_smem((const void *)k_gen_pyramid_jac, kSmemJacGenMax)) return rc;
        hipLaunchKernelGGL(k_gen_pyramid_jac, dim3(tiles), dim3(256), jac_gen_floats(desc->width) * 4, (hipStream_t)stream, q, x, x_out, J,
                           normals_in, normals_out);
    } else {
        if (int rc = set_smem((const void *)k_pyramid_jac, kSmemJacBytes)) return rc;
        hipLaunchKernelGGL(k_pyramid_jac, dim3(tiles), dim3(256), kSmemJacBytes, (hipStream_t)stream, q, x, x_out, J, normals_in, normals_out);
    }
    HIP_TRY(hipGetLastError(), "k_pyramid_jac launch");
    return 0;
}

extern "C" int ndp_pyramid_inverse(const ndp_layer_desc *desc, int m, int k0, const float *params_all, int p_stride, int min_level,
                                   int max_level, const float *y, int n, float *x, int iters, float tol, float *residual, int *status,
                                   void *stream) {
    JacArgs q;
    if (int rc = jac_check("ndp_pyramid_inverse", desc, m, k0, params_all, p_stride, min_level, max_level, n, q)) return rc;
    if (!y || !x || !residual || !status || !aligned4(y) || !aligned4(x) || !aligned4(residual) || !aligned4(status))
        return fail(NDP_E_INVALID, "ndp_pyramid_inverse: y, x, residual and status must be non-null and 4-byte aligned");
    if (iters < 1) return fail(NDP_E_INVALID, "ndp_pyramid_inverse: iters must be at least 1");
    if (!(tol > 0.f) || !(tol <= 3.4028234e38f)) return fail(NDP_E_INVALID, "ndp_pyramid_inverse: tol must be positive and finite");
    const int tiles = (n + NDP_TILE - 1) / NDP_TILE;
    if (gen_is_generic(*desc)) {
        if (int rc = set_smem((const void *)k_gen_pyramid_inverse, kSmemJacGenMax)) return rc;
        hipLaunchKernelGGL(k_gen_pyramid_inverse, dim3(tiles), dim3(256), jac_gen_floats(desc->width) * 4, (hipStream_t)stream, q, y, x, iters,
                           tol, residual, status);
    } else {
        if (int rc = set_smem((const void *)k_pyramid_inverse, kSmemJacBytes)) return rc;
        hipLaunchKernelGGL(k_pyramid_inverse, dim3(tiles), dim3(256), kSmemJacBytes, (hipStream_t)stream, q, y, x, iters, tol, residual, status);
    }
    HIP_TRY(hipGetLastError(), "k_pyramid_inverse launch");
    return 0;
}
