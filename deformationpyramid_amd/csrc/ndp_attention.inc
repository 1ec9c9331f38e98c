// ndp_attention.inc -- multi-head soft-max attention for stacked, unpadded problems, fused: the L x S x H scores are never stored
// (k_attention_*, ndp_attention_forward).  DESIGN.md "Attention".  fp32 throughout on the f32-input MFMA (16x16x4), no atomics, one
// writer per output element, every sum in one fixed order.  Problem b owns the query rows offQ[b] .. offQ[b + 1] and the key / value
// rows offK[b] .. offK[b + 1]; the entry checks the host's copies of both with check_offsets (ndp_abi_common.inc).
//
//   o[i, h D + d] = sum_j softmax_j(scale <q'_i,h , k'_j,h>) v[j, h D + d],      D = C / H
//   q' = q cos + rot(q) sin,  rot(x)[2m] = -x[2m + 1],  rot(x)[2m + 1] = x[2m]   (pe [rows, C, 2] = (cos, sin) per channel; v is not rotated)
//
// A workgroup (4 waves) owns AT_BM = 16 query rows of one (problem, head) and walks the keys in tiles of AT_BN = 64, ascending; wave
// w owns the keys 16 w .. 16 w + 15 of a tile.  The rotation is applied while an operand is staged into LDS: no rotated copy reaches
// global memory.  Both products are taken TRANSPOSED so that a query stays on its lane (lane & 15) through the whole walk:
//   scores  D = K'_tile Q'^T: the MFMA's A operand is a key row, its B operand a query row; in the 16x16 C/D map lane l holds the keys
//           4 (l >> 4) + r, r = 0 .. 3, of query l & 15.  The chain runs over ascending channels from 0, four per step.
//   P V     O^T += V^T P^T in four steps r: step r contracts the keys 4 g + r, g = 0 .. 3 -- the A operand is V[key 4 g + r][d], the
//           B operand of lane l is its OWN score register r.  No lane traffic between the two products.
// The soft-max runs online per wave: the tile's maximum of a query is taken over the lane's four scores and the three other lanes of
// the query (two xor shuffles; a maximum has no order), the running sum stays a per-lane partial.  Channels D .. DP - 1 (DP = D
// rounded up to 4) and rows beyond the problem are zeros in LDS, never reads; a key beyond S scores -inf.  At the end the four waves'
// (m, s, O) of a query are folded in wave order, each wave's four partial sums in lane-group order.
//
// COMPAT (k_attention_compat_*, ndp_attention_compat_forward; DESIGN.md "Outlier rejection"): the score of (i, j, h) is multiplied by
// the spatial compatibility of the correspondences i and j before the scale and the soft-max,
//   c[i, j] = max(0, 1 - (|s_i - s_j| - |t_i - t_j|)^2 / sigma_spat^2),      pos [rows, 6] = (s_xyz, t_xyz) per row
// in fp32 and in the reference's order of operations (outlier_rejection/pipeline.py:55-58): the norm of the source difference, the
// norm of the target difference, their difference squared, a true division by (float)(sigma_spat^2), 1 minus that, clamped at 0;
// sqrtf and the division are correctly rounded.  The key tile's 64 x 6 positions are staged in LDS behind the statistics, the lane's
// own query row's six coordinates stay in registers for the whole walk, and c is taken for the lane's four score registers between
// the score chain and the online soft-max.  c depends on (i, j) only and is recomputed per head: about 20 vector operations against
// D multiply-adds per pair.  c = 0 scores 0, not -inf: such a key takes part in the soft-max.  A key beyond S still scores -inf.
// Non-finite positions are the caller's error and are not checked on the device.
#define AT_BM 16
#define AT_BN 64
#define AT_MAX_H 16
#define AT_MAX_D 264
#define AT_STATS 512                   // floats behind the tiles: the waves' m [4][16], s [4][4][16], the fold's factors [4][16] and sums [16]
#define AT_MAX_ROWS (1 << 30)
#define AT_POS 6                       // floats of a correspondence's position row (COMPAT): source xyz, target xyz

// LDS row stride in words for DP channels: a multiple of 4 that is 4 modulo 8, so 16 rows x 4 consecutive words spread over the banks
__host__ __device__ static inline int at_ld(int DP) { return DP % 8 == 0 ? DP + 4 : DP; }
// floats of dynamic LDS: the query block, a key tile, a value tile, 16 words of slack (the P V step reads V's columns up to the next
// multiple of 16 -- those feed output rows d >= D, which are never written) and the statistics
__host__ __device__ static inline int at_lds_floats(int D) { return (AT_BM + 2 * AT_BN) * at_ld((D + 3) & ~3) + 16 + AT_STATS; }

// rows grow0 .. grow0 + nvalid - 1, channels ch0 .. ch0 + D - 1 of src [rows, C] -> dst [nrows][LD], rotated by pe if given; rows
// beyond nvalid and channels beyond D are zeros.  VEC: D a multiple of 4 and 16-byte aligned operands (every row of a head then is).
template <bool VEC>
__device__ __forceinline__ void at_stage(float *dst, int LD, const float *src, const float *pe, int C, int ch0, int D, int DP, size_t grow0,
                                         int nvalid, int nrows) {
    const int t = threadIdx.x;
    if (VEC) {
        const int n4 = DP >> 2;
        for (int idx = t; idx < nrows * n4; idx += 256) {
            const int row = idx / n4, c = (idx - row * n4) << 2;
            float4 x = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < nvalid) {
                const size_t e = (grow0 + row) * C + ch0 + c;
                x = *reinterpret_cast<const float4 *>(src + e);
                if (pe) {
                    const float4 p0 = *reinterpret_cast<const float4 *>(pe + 2 * e), p1 = *reinterpret_cast<const float4 *>(pe + 2 * e + 4);
                    x = make_float4(x.x * p0.x + (-x.y) * p0.y, x.y * p0.z + x.x * p0.w, x.z * p1.x + (-x.w) * p1.y, x.w * p1.z + x.z * p1.w);
                }
            }
            *reinterpret_cast<float4 *>(dst + row * LD + c) = x;
        }
    } else {
        for (int idx = t; idx < nrows * DP; idx += 256) {
            const int row = idx / DP, c = idx - row * DP;
            float x = 0.f;
            if (row < nvalid && c < D) {
                const size_t rb = (grow0 + row) * C, e = rb + ch0 + c;
                x = src[e];
                if (pe) {                                        // D is even with a code, so the partner lies in the same head
                    const float y = src[rb + ((ch0 + c) ^ 1)];
                    x = x * pe[2 * e] + (((ch0 + c) & 1) ? y : -y) * pe[2 * e + 1];
                }
            }
            dst[row * LD + c] = x;
        }
    }
}

// |a - b| of two points in the reference's order: the three squares summed in axis order, one correctly rounded square root
__device__ __forceinline__ float at_dist(const float *a, const float *b) {
    const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
    return sqrtf((dx * dx + dy * dy) + dz * dz);
}

template <int NT, bool VEC, bool COMPAT>
__device__ __forceinline__ void attention_body(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                               const float *pos_q, const float *pos_k, const int *offQ, const int *offK, int C, int D,
                                               float scale, float sigma2, float *out) {
    extern __shared__ __attribute__((aligned(16))) float at_sm[];
    const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z;
    const int q0 = offQ[b], L = offQ[b + 1] - q0, k0 = offK[b], S = offK[b + 1] - k0;
    const int r0 = blockIdx.x * AT_BM;
    if (r0 >= L) return;                                         // (uniform: the grid is sized by the largest problem)
    const int DP = (D + 3) & ~3, LD = at_ld(DP), ndt = (D + 15) >> 4, ch0 = h * D;
    float *Qs = at_sm, *Ks = Qs + AT_BM * LD, *Vs = Ks + AT_BN * LD, *st = Vs + AT_BN * LD + 16;
    const int lane = t & 63, w = t >> 6, l15 = lane & 15, g = lane >> 4;
    at_stage<VEC>(Qs, LD, q, pe_q, C, ch0, D, DP, (size_t)q0 + r0, min(AT_BM, L - r0), AT_BM);
    f32x4 o[NT];
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, s = 0.f;                                // query l15 over the keys this wave has met; s: this lane's share
    float *Ps = st + AT_STATS;                                   // COMPAT: [AT_BN][AT_POS], the key tile's positions
    float pq[AT_POS];                                            // COMPAT: query l15's own position (zeros beyond L: that row is never written)
    if (COMPAT) {
#pragma unroll
        for (int u = 0; u < AT_POS; ++u) pq[u] = r0 + l15 < L ? pos_q[((size_t)q0 + r0 + l15) * AT_POS + u] : 0.f;
    }
    const int n_jt = (S + AT_BN - 1) / AT_BN;
    for (int jt = 0; jt < n_jt; ++jt) {
        if (jt) __syncthreads();
        const int nv = min(AT_BN, S - jt * AT_BN), nrows = (nv + 15) & ~15;
        at_stage<VEC>(Ks, LD, k, pe_k, C, ch0, D, DP, (size_t)k0 + jt * AT_BN, nv, nrows);
        at_stage<VEC>(Vs, LD, v, nullptr, C, ch0, D, DP, (size_t)k0 + jt * AT_BN, nv, nrows);
        if (COMPAT) {                                            // the tile's position rows are contiguous; zeros beyond the problem
            for (int idx = t; idx < AT_BN * AT_POS; idx += 256)
                Ps[idx] = idx < nv * AT_POS ? pos_k[((size_t)k0 + jt * AT_BN) * AT_POS + idx] : 0.f;
        }
        __syncthreads();
        if (16 * w < nv) {                                       // (uniform per wave) this wave's 16 keys hold at least one of the problem
            f32x4 sc = f32x4{0.f, 0.f, 0.f, 0.f};
            const float *ka = Ks + (16 * w + l15) * LD + g, *qb = Qs + l15 * LD + g;
            for (int c = 0; c < DP; c += 4) sc = MFMA16(ka[c], qb[c], sc);
            float x[4], tm = -INFINITY;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float a = sc[r];
                if (COMPAT) {
                    const float *pk = Ps + (16 * w + 4 * g + r) * AT_POS;
                    const float dd = at_dist(pq, pk) - at_dist(pq + 3, pk + 3);
                    a *= fmaxf(0.f, 1.0f - (dd * dd) / sigma2);
                }
                x[r] = 16 * w + 4 * g + r < nv ? scale * a : -INFINITY;
                tm = fmaxf(tm, x[r]);
            }
            tm = fmaxf(tm, __shfl_xor(tm, 16));
            tm = fmaxf(tm, __shfl_xor(tm, 32));
            if (tm > m) {
                const float f = expf(m - tm);
                s *= f;
#pragma unroll
                for (int dt = 0; dt < NT; ++dt) o[dt] *= f;
                m = tm;
            }
            float p[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                p[r] = m > -INFINITY ? expf(x[r] - m) : 0.f;
                s += p[r];
            }
            const float *va = Vs + (16 * w + 4 * g) * LD + l15;
#pragma unroll
            for (int dt = 0; dt < NT; ++dt) {
                if (dt < ndt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[dt] = MFMA16(va[r * LD + 16 * dt], p[r], o[dt]);
                }
            }
        }
    }
    __syncthreads();
    float *Os = Ks;                                              // [4 waves][16 queries][LD]: O of query i, channel d at (16 w + i) LD + d
    float *cm = st, *cs = st + 64, *cf = st + 320, *ct = st + 384;
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * dt + 4 * g + r;
            if (d < D) Os[(16 * w + l15) * LD + d] = o[dt][r];
        }
    }
    if (g == 0) cm[16 * w + l15] = m;
    cs[(4 * w + g) * 16 + l15] = s;
    __syncthreads();
    if (t < AT_BM) {
        float M = -INFINITY;
        for (int u = 0; u < 4; ++u) M = fmaxf(M, cm[16 * u + t]);
        float sum = 0.f;
        for (int u = 0; u < 4; ++u) {
            const float mu = cm[16 * u + t];
            float f = 0.f;
            if (mu > -INFINITY) {
                f = expf(mu - M);
                sum += (((cs[(4 * u) * 16 + t] + cs[(4 * u + 1) * 16 + t]) + cs[(4 * u + 2) * 16 + t]) + cs[(4 * u + 3) * 16 + t]) * f;
            }
            cf[16 * u + t] = f;
        }
        ct[t] = sum;
    }
    __syncthreads();
    const int nq = min(AT_BM, L - r0);
    for (int idx = t; idx < nq * D; idx += 256) {
        const int i = idx / D, d = idx - i * D;
        float acc = 0.f;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const float f = cf[16 * u + i];
            if (f > 0.f) acc += Os[(16 * u + i) * LD + d] * f;
        }
        out[((size_t)q0 + r0 + i) * C + ch0 + d] = acc / ct[i];
    }
}

// NT = the number of 16-channel output tiles a wave's accumulators hold: D <= 16 NT.  _v4: 16-byte loads, the same bits.
#define AT_KERNEL(name, NT, VEC)                                                                                                \
    extern "C" __global__ void __launch_bounds__(256)                                                                           \
    name(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const int *offQ, const int *offK, int C, \
         int D, float scale, float *out) {                                                                                      \
        attention_body<NT, VEC, false>(q, k, v, pe_q, pe_k, nullptr, nullptr, offQ, offK, C, D, scale, 0.f, out);               \
    }
AT_KERNEL(k_attention_d16, 1, false)
AT_KERNEL(k_attention_d48, 3, false)
AT_KERNEL(k_attention_d144, 9, false)
AT_KERNEL(k_attention_d264, 17, false)
AT_KERNEL(k_attention_d16_v4, 1, true)
AT_KERNEL(k_attention_d48_v4, 3, true)
AT_KERNEL(k_attention_d144_v4, 9, true)
AT_KERNEL(k_attention_d264_v4, 17, true)
#undef AT_KERNEL
#define AT_KERNEL(name, NT, VEC)                                                                                                \
    extern "C" __global__ void __launch_bounds__(256)                                                                           \
    name(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const float *pos_q, const float *pos_k, \
         const int *offQ, const int *offK, int C, int D, float scale, float sigma2, float *out) {                               \
        attention_body<NT, VEC, true>(q, k, v, pe_q, pe_k, pos_q, pos_k, offQ, offK, C, D, scale, sigma2, out);                 \
    }
AT_KERNEL(k_attention_compat_d16, 1, false)
AT_KERNEL(k_attention_compat_d48, 3, false)
AT_KERNEL(k_attention_compat_d144, 9, false)
AT_KERNEL(k_attention_compat_d264, 17, false)
AT_KERNEL(k_attention_compat_d16_v4, 1, true)
AT_KERNEL(k_attention_compat_d48_v4, 3, true)
AT_KERNEL(k_attention_compat_d144_v4, 9, true)
AT_KERNEL(k_attention_compat_d264_v4, 17, true)
#undef AT_KERNEL

// ------------------------------------------------------------------------------------------------
// host entries.  Every refusal is decided before the first HIP call; nothing in an entry is data-dependent, so it does not synchronise.
// The refusals both entries share -> 0 with the largest L and whether the 16-byte staging serves the call.
static int at_check(const char *who, const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const int *offQ,
                    const int *offK, const int *offQ_host, const int *offK_host, int B, int C, int n_head, float scale, const float *out,
                    int *maxL, bool *vec) {
    if (int rc = check_batch(who, offQ_host && offK_host ? offQ_host : nullptr, B)) return rc;
    if (C < 1 || C > FM_MAX_C || n_head < 1 || n_head > AT_MAX_H || C % n_head != 0 || C / n_head > AT_MAX_D)
        return failf(NDP_E_UNSUPPORTED, "%s: served are 1 <= C <= %d, 1 <= n_head <= %d with C a multiple of n_head and C / n_head <= %d", who,
                     FM_MAX_C, AT_MAX_H, AT_MAX_D);
    int maxS = 0;
    if (int rc = check_offsets(who, offQ_host, B, 1, "a non-empty side, L and S", maxL)) return rc;
    if (int rc = check_offsets(who, offK_host, B, 1, "a non-empty side, L and S", &maxS)) return rc;
    if (offQ_host[B] > AT_MAX_ROWS || offK_host[B] > AT_MAX_ROWS) return failf(NDP_E_UNSUPPORTED, "%s: served are at most 2^30 rows a side", who);
    if (!q || !k || !v || !offQ || !offK || !out) return failf(NDP_E_INVALID, "%s: null pointer", who);
    if ((pe_q == nullptr) != (pe_k == nullptr)) return failf(NDP_E_INVALID, "%s: pe_q and pe_k are passed as both or neither", who);
    if (!fm_aligned4(q) || !fm_aligned4(k) || !fm_aligned4(v) || !fm_aligned4(pe_q) || !fm_aligned4(pe_k) || !fm_aligned4(offQ) ||
        !fm_aligned4(offK) || !fm_aligned4(out))
        return failf(NDP_E_INVALID, "%s: pointers must be 4-byte aligned", who);
    const int D = C / n_head;
    if (pe_q && D % 2 != 0) return failf(NDP_E_INVALID, "%s: a rotary code needs an even head dimension (C / n_head = %d)", who, D);
    if (!std::isfinite(scale)) return failf(NDP_E_INVALID, "%s: scale must be finite", who);
    *vec = D % 4 == 0 && aligned16(q) && aligned16(k) && aligned16(v) && aligned16(pe_q) && aligned16(pe_k);
    return 0;
}

static const int at_dmax[4] = {16, 48, 144, 264};
static inline int at_class(int D) { return D <= 16 ? 0 : D <= 48 ? 1 : D <= 144 ? 2 : 3; }

extern "C" int ndp_attention_forward(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const int *offQ,
                                     const int *offK, const int *offQ_host, const int *offK_host, int B, int C, int n_head, float scale,
                                     float *out, void *stream) {
    int maxL = 0;
    bool vec = false;
    if (int rc = at_check("ndp_attention_forward", q, k, v, pe_q, pe_k, offQ, offK, offQ_host, offK_host, B, C, n_head, scale, out, &maxL, &vec))
        return rc;
    const int D = C / n_head, cls = at_class(D);
    using Kern = void (*)(const float *, const float *, const float *, const float *, const float *, const int *, const int *, int, int, float, float *);
    static const Kern kern[2][4] = {{k_attention_d16, k_attention_d48, k_attention_d144, k_attention_d264},
                                    {k_attention_d16_v4, k_attention_d48_v4, k_attention_d144_v4, k_attention_d264_v4}};
    const Kern fn = kern[vec][cls];
    if (int rc = set_smem((const void *)fn, 4 * at_lds_floats(at_dmax[cls]))) return rc;
    const dim3 grid((maxL + AT_BM - 1) / AT_BM, n_head, B);
    hipLaunchKernelGGL(fn, grid, dim3(256), 4 * at_lds_floats(D), (hipStream_t)stream, q, k, v, pe_q, pe_k, offQ, offK, C, D, scale, out);
    HIP_TRY(hipGetLastError(), "k_attention launch");
    return 0;
}

// The compatibility-modulated form: pos_q [sum L][6], pos_k [sum S][6] are always both taken; sigma_spat is a double so that
// (float)(sigma_spat^2) is the divisor the reference's `** 2 / self.sigma_spat ** 2` rounds to.  +inf is served and means c == 1.
extern "C" int ndp_attention_compat_forward(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                            const float *pos_q, const float *pos_k, const int *offQ, const int *offK, const int *offQ_host,
                                            const int *offK_host, int B, int C, int n_head, float scale, double sigma_spat, float *out,
                                            void *stream) {
    const char *who = "ndp_attention_compat_forward";
    int maxL = 0;
    bool vec = false;
    if (int rc = at_check(who, q, k, v, pe_q, pe_k, offQ, offK, offQ_host, offK_host, B, C, n_head, scale, out, &maxL, &vec)) return rc;
    if (!pos_q || !pos_k) return failf(NDP_E_INVALID, "%s: null pointer (pos_q and pos_k are always both taken)", who);
    if (!fm_aligned4(pos_q) || !fm_aligned4(pos_k)) return failf(NDP_E_INVALID, "%s: pointers must be 4-byte aligned", who);
    if (!(sigma_spat > 0)) return failf(NDP_E_INVALID, "%s: sigma_spat must be positive (inf: no compatibility), got %g", who, sigma_spat);
    const float sigma2 = (float)(sigma_spat * sigma_spat);
    if (!(sigma2 > 0)) return failf(NDP_E_INVALID, "%s: sigma_spat^2 = %g^2 underflows float32", who, sigma_spat);
    const int D = C / n_head, cls = at_class(D);
    using Kern = void (*)(const float *, const float *, const float *, const float *, const float *, const float *, const float *, const int *,
                          const int *, int, int, float, float, float *);
    static const Kern kern[2][4] = {
        {k_attention_compat_d16, k_attention_compat_d48, k_attention_compat_d144, k_attention_compat_d264},
        {k_attention_compat_d16_v4, k_attention_compat_d48_v4, k_attention_compat_d144_v4, k_attention_compat_d264_v4}};
    const Kern fn = kern[vec][cls];
    const int pos_floats = AT_BN * AT_POS;                       // the key tile's positions, behind the statistics
    if (int rc = set_smem((const void *)fn, 4 * (at_lds_floats(at_dmax[cls]) + pos_floats))) return rc;
    const dim3 grid((maxL + AT_BM - 1) / AT_BM, n_head, B);
    hipLaunchKernelGGL(fn, grid, dim3(256), 4 * (at_lds_floats(D) + pos_floats), (hipStream_t)stream, q, k, v, pe_q, pe_k, pos_q, pos_k, offQ,
                       offK, C, D, scale, sigma2, out);
    HIP_TRY(hipGetLastError(), "k_attention_compat launch");
    return 0;
}
