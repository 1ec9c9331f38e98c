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

template <int NT, bool VEC, bool COMPAT, bool LSE = false>
__device__ __forceinline__ void attention_body(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                               const float *pos_q, const float *pos_k, const int *offQ, const int *offK, int C, int D,
                                               float scale, float sigma2, float *out, float *lse = nullptr) {
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
        if (LSE && r0 + t < L) lse[((size_t)q0 + r0 + t) * gridDim.y + h] = M + logf(sum);    // the row's log-sum-exp, for the backward
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

// ------------------------------------------------------------------------------------------------
// ABI 217: the forward with statistics and the backward (DESIGN.md "Attention backward").
//
// Forward with statistics (k_attention_lse_*, k_attention_compat_lse_*; ndp_attention_forward_lse): attention_body with LSE set -- the
// same instructions up to the fold, where the thread that folds a query's four waves also writes lse[i, h] = M + log(sum), the
// log-sum-exp of the row's scaled scores.  o is the bits of the entries above.
#define AT_KERNEL(name, NT, VEC)                                                                                                \
    extern "C" __global__ void __launch_bounds__(256)                                                                           \
    name(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const int *offQ, const int *offK, int C, \
         int D, float scale, float *out, float *lse) {                                                                          \
        attention_body<NT, VEC, false, true>(q, k, v, pe_q, pe_k, nullptr, nullptr, offQ, offK, C, D, scale, 0.f, out, lse);    \
    }
AT_KERNEL(k_attention_lse_d16, 1, false)
AT_KERNEL(k_attention_lse_d48, 3, false)
AT_KERNEL(k_attention_lse_d144, 9, false)
AT_KERNEL(k_attention_lse_d264, 17, false)
AT_KERNEL(k_attention_lse_d16_v4, 1, true)
AT_KERNEL(k_attention_lse_d48_v4, 3, true)
AT_KERNEL(k_attention_lse_d144_v4, 9, true)
AT_KERNEL(k_attention_lse_d264_v4, 17, true)
#undef AT_KERNEL
#define AT_KERNEL(name, NT, VEC)                                                                                                \
    extern "C" __global__ void __launch_bounds__(256)                                                                           \
    name(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const float *pos_q, const float *pos_k, \
         const int *offQ, const int *offK, int C, int D, float scale, float sigma2, float *out, float *lse) {                   \
        attention_body<NT, VEC, true, true>(q, k, v, pe_q, pe_k, pos_q, pos_k, offQ, offK, C, D, scale, sigma2, out, lse);      \
    }
AT_KERNEL(k_attention_compat_lse_d16, 1, false)
AT_KERNEL(k_attention_compat_lse_d48, 3, false)
AT_KERNEL(k_attention_compat_lse_d144, 9, false)
AT_KERNEL(k_attention_compat_lse_d264, 17, false)
AT_KERNEL(k_attention_compat_lse_d16_v4, 1, true)
AT_KERNEL(k_attention_compat_lse_d48_v4, 3, true)
AT_KERNEL(k_attention_compat_lse_d144_v4, 9, true)
AT_KERNEL(k_attention_compat_lse_d264_v4, 17, true)
#undef AT_KERNEL

// Backward: the gradient of o with respect to the UNROTATED q, k and v, given do; pe_* and pos_* are data and c is not differentiated.
// Everything is recomputed from q, k, v and lse -- no L x S array in global memory -- in two sweeps, each the forward's structure with
// one more product per tile, fp32 on the f32-input MFMA, no atomics, one writer per output element, every sum in one fixed order:
//   p = exp(x - lse_i),  x = scale c a,  a = <q'_i, k'_j>;   dp = <do_i, v_j>;   ds = p (dp - delta_i),  delta_i = sum_d o[i, d] do[i, d]
//   dv_j = sum_i p do_i,      dq'_i = sum_j (ds scale c) k'_j,      dk'_j = sum_i (ds scale c) q'_i
// A key beyond S has p = 0.  A key with c = 0 has p != 0: it feeds dv and delta, and nothing to dq' or dk'.
//   dq sweep (k_attention_dq_*): a workgroup owns 16 query rows of one (problem, head) and walks key tiles in ascending order; wave w
//     owns the keys 16 w .. 16 w + 15 of a tile.  Its prologue takes delta of its rows as the diagonal of O dO^T on the MFMA, by
//     the very chains that take dp (ab_chain), so that where o_i is v_j bit for bit (a problem with one key) dp - delta cancels
//     exactly, as it does in the soft-max backward that sums p dp -- and writes it to delta [sum L, H] for the other sweep.  Scores K' Q'^T and dp = V dO^T are
//     both taken with the key as the MFMA's A row and the query as its B column, so lane l holds the keys 4 (l >> 4) + r of query
//     l & 15 in both, as in the forward; dq'^T += K'^T t^T then runs in four steps r with the lane's OWN t[r] = ds scale c as the B
//     operand -- the forward's P V with K' in V's place.  p and t never leave the lane's registers.
//   dk / dv sweep (k_attention_dkv_*): the mirror image.  A workgroup owns 16 key rows and walks query tiles in ascending order, wave w
//     owns the queries 16 w .. 16 w + 15 of a tile; Q' K'^T and dO V^T have the query as the A row and the key as the B column, so a
//     KEY stays on its lane (l & 15); dv^T += dO^T p and dk'^T += Q'^T t take the lane's own p[r] and t[r] as B.  The tile's lse and
//     delta (and, with positions, its position rows) are staged in LDS next to it.
// At the end of either sweep the four waves' partial blocks are folded in wave order through LDS, and the block is UN-ROTATED while it
// is written: q' = q cos + rot(q) sin is linear, so dq = dq' cos + rot^T(dq' sin), rot^T(y)[2m] = y[2m + 1], rot^T(y)[2m + 1] = -y[2m],
// that is dq[2m] = dq'[2m] cos[2m] + dq'[2m + 1] sin[2m + 1] and dq[2m + 1] = dq'[2m + 1] cos[2m + 1] - dq'[2m] sin[2m].  No rotated
// copy reaches global memory.  Positions are a run-time switch here (pos_q == NULL: c == 1, the same instructions on x), so
// sigma_spat = +inf is the plain call's bits by construction.
//
// LDS.  A sweep holds the owned block twice (q' and do, or k' and v: 2 x 16 rows) and a walked tile twice (k' and v, or q' and do:
// 2 T rows), at_ld(DP) words a row, then 16 words of slack, AB_STATS words and T position rows:
//   ab_lds_floats(D) = (2 * 16 + 2 T) at_ld(DP) + 16 + 512 + 6 T.
// The forward's T = AT_BN = 64 would take (32 + 128) * 268 * 4 = 171 520 bytes at D = 264, above the 160 KiB (163 840 bytes) of a
// workgroup, so the tile is chosen by D:  T = 64 for D <= 144 (at most 160 * 148 + 912 words = 98 368 bytes), T = 48 for
// 144 < D <= 264 (at most 128 * 268 + 816 words = 140 480 bytes; three of the four waves then walk).  T is a multiple of 16 and at
// least 32, so that the fold's [4 waves][16][LD] block fits in the walked tiles.
#define AB_STATS 512                   // dq sweep: delta [16]; dk / dv sweep: the tile's lse [64] and delta [64]
__host__ __device__ static inline int ab_tile(int D) { return D <= 144 ? 64 : 48; }
__host__ __device__ static inline int ab_lds_floats(int D) {
    return (2 * AT_BM + 2 * ab_tile(D)) * at_ld((D + 3) & ~3) + 16 + AB_STATS + ab_tile(D) * AT_POS;
}

// <a row, b row> over DP channels on the MFMA: ONE chain over ascending channels from 0, four per step -- the forward's score chain,
// so that x here is the forward's x bit for bit and its rounding error cancels against the same error inside lse wherever a key
// dominates its row (measured: four interleaved chains, although each is more accurate, more than doubled the error of dq at
// D = 264).  Scores, dp and delta all go through here: equal operands give equal bits.
__device__ __forceinline__ f32x4 ab_chain(const float *a, const float *b, int DP) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < DP; c += 4) acc = MFMA16(a[c], b[c], acc);
    return acc;
}

// The same product on four interleaved chains -- chain u over the steps u, u + 4, ... of four channels, the steps behind the last
// whole group of four on chain 0, folded as (c0 + c1) + (c2 + c3): a quarter of one chain's length.  The dk / dv sweep takes the
// probabilities that weigh do in dv from this x.  One chain's x carries up to 3e-6 at D = 264 (partial sums near 64), which
// exp(x - lse) hands to p and p to dv at full size, where the forward's o = sum p v / s and ds = p (dp - delta) see it largely
// cancel; ds keeps the forward's chain, because there p has to agree with the p behind o and delta (a row-wise factor between the
// two turns into an error of dq and dk of the size of dp).  Only the D > 144 class (NT = 17) pays for this third D-long product:
// up to D = 144 dv stays under 0.7 of its bar on the forward's chain, and there p is the one probability for dv and ds.
__device__ __forceinline__ f32x4 ab_chain4(const float *a, const float *b, int DP) {
    f32x4 c0 = f32x4{0.f, 0.f, 0.f, 0.f}, c1 = c0, c2 = c0, c3 = c0;
    int c = 0;
    for (; c + 16 <= DP; c += 16) {
        c0 = MFMA16(a[c], b[c], c0);
        c1 = MFMA16(a[c + 4], b[c + 4], c1);
        c2 = MFMA16(a[c + 8], b[c + 8], c2);
        c3 = MFMA16(a[c + 12], b[c + 12], c3);
    }
    for (; c < DP; c += 4) c0 = MFMA16(a[c], b[c], c0);
    return (c0 + c1) + (c2 + c3);
}

// p = exp(x - lse) with the rounding of the difference carried along: yh + yl = x - lse exactly (two-sum), p = e^yh (1 + yl).  At
// |x - lse| of 4 .. 8 the plain difference alone costs p up to two of its ulps, on top of the rounding that lse itself carries.
__device__ __forceinline__ float ab_prob(float x, float lse) {
    const float nl = -lse, yh = x + nl, bb = yh - x, yl = (x - (yh - bb)) + (nl - bb);
    const float e = expf(yh);
    return e + e * yl;
}

// the four waves' partial of element (i, d), in wave order
__device__ __forceinline__ float ab_fold(const float *Os, int LD, int i, int d) {
    return ((Os[i * LD + d] + Os[(16 + i) * LD + d]) + Os[(32 + i) * LD + d]) + Os[(48 + i) * LD + d];
}

// fold the waves' [4][16][LD] block in Os and write rows 0 .. n - 1 of it to dst's rows grow0 .., un-rotated by pe if given
__device__ __forceinline__ void ab_write(float *dst, const float *pe, const float *Os, int LD, int C, int ch0, int D, size_t grow0, int n) {
    for (int idx = threadIdx.x; idx < n * D; idx += 256) {
        const int i = idx / D, d = idx - i * D;
        const size_t rb = (grow0 + i) * C, e = rb + ch0 + d;
        float x = ab_fold(Os, LD, i, d);
        if (pe) {                                                // D is even with a code, so the partner lies in the same head
            const float y = ab_fold(Os, LD, i, d ^ 1);
            const size_t e1 = rb + ch0 + (d ^ 1);
            x = x * pe[2 * e] + ((d & 1) ? -y : y) * pe[2 * e1 + 1];
        }
        dst[e] = x;
    }
}

template <int NT, bool VEC>
__device__ __forceinline__ void attention_dq_body(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                                  const float *pos_q, const float *pos_k, const float *o, const float *lse, const float *dout,
                                                  const int *offQ, const int *offK, int C, int D, float scale, float sigma2, float *delta,
                                                  float *dq) {
    constexpr int T = NT <= 9 ? 64 : 48;                         // ab_tile(D): NT = 17 serves 144 < D <= 264
    extern __shared__ __attribute__((aligned(16))) float at_sm[];
    const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
    const int q0 = offQ[b], L = offQ[b + 1] - q0, k0 = offK[b], S = offK[b + 1] - k0;
    const int r0 = blockIdx.x * AT_BM;
    if (r0 >= L) return;                                         // (uniform: the grid is sized by the largest problem)
    const int DP = (D + 3) & ~3, LD = at_ld(DP), ndt = (D + 15) >> 4, ch0 = h * D;
    float *Qs = at_sm, *Gs = Qs + AT_BM * LD, *Ks = Gs + AT_BM * LD, *Vs = Ks + T * LD, *st = Vs + T * LD + 16, *Ps = st + AB_STATS;
    const int lane = t & 63, w = t >> 6, l15 = lane & 15, g = lane >> 4;
    const bool compat = pos_q != nullptr;
    const int nq = min(AT_BM, L - r0);
    at_stage<VEC>(Qs, LD, q, pe_q, C, ch0, D, DP, (size_t)q0 + r0, nq, AT_BM);
    at_stage<VEC>(Gs, LD, dout, nullptr, C, ch0, D, DP, (size_t)q0 + r0, nq, AT_BM);
    at_stage<VEC>(Ks, LD, o, nullptr, C, ch0, D, DP, (size_t)q0 + r0, nq, AT_BM);       // the rows' o, for delta only
    __syncthreads();
    if (w == 0) {                                                // delta = diag(O dO^T), by the chain that takes dp (see the header)
        const f32x4 dd = ab_chain(Ks + l15 * LD + g, Gs + l15 * LD + g, DP);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            if (4 * g + r == l15) {
                st[l15] = dd[r];
                if (l15 < nq) delta[((size_t)q0 + r0 + l15) * H + h] = dd[r];
            }
        }
    }
    __syncthreads();
    const float dl = st[l15];                              // query l15's delta and lse (0 beyond L: that row is never written)
    const float ls = l15 < nq ? lse[((size_t)q0 + r0 + l15) * H + h] : 0.f;
    f32x4 acc[NT];
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) acc[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pq[AT_POS];
#pragma unroll
    for (int u = 0; u < AT_POS; ++u) pq[u] = compat && l15 < nq ? pos_q[((size_t)q0 + r0 + l15) * AT_POS + u] : 0.f;
    const int n_jt = (S + T - 1) / T;
    for (int jt = 0; jt < n_jt; ++jt) {
        if (jt) __syncthreads();
        const int nv = min(T, S - jt * T), nrows = (nv + 15) & ~15;
        at_stage<VEC>(Ks, LD, k, pe_k, C, ch0, D, DP, (size_t)k0 + jt * T, nv, nrows);
        at_stage<VEC>(Vs, LD, v, nullptr, C, ch0, D, DP, (size_t)k0 + jt * T, nv, nrows);
        if (compat) {
            for (int idx = t; idx < T * AT_POS; idx += 256) Ps[idx] = idx < nv * AT_POS ? pos_k[((size_t)k0 + jt * T) * AT_POS + idx] : 0.f;
        }
        __syncthreads();
        if (16 * w < nv) {                                       // (uniform per wave; never wave 3 when T = 48)
            const f32x4 sc = ab_chain(Ks + (16 * w + l15) * LD + g, Qs + l15 * LD + g, DP);
            const f32x4 dp = ab_chain(Vs + (16 * w + l15) * LD + g, Gs + l15 * LD + g, DP);
            float tt[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                float a = sc[r], cc = 1.0f;
                if (compat) {
                    const float *pk = Ps + (16 * w + 4 * g + r) * AT_POS;
                    const float dd = at_dist(pq, pk) - at_dist(pq + 3, pk + 3);
                    cc = fmaxf(0.f, 1.0f - (dd * dd) / sigma2);
                    a *= cc;
                }
                const float p = 16 * w + 4 * g + r < nv ? ab_prob(scale * a, ls) : 0.f;
                tt[r] = (p * (dp[r] - dl)) * (scale * cc);
            }
            const float *kt = Ks + (16 * w + 4 * g) * LD + l15;
#pragma unroll
            for (int dt = 0; dt < NT; ++dt) {
                if (dt < ndt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) acc[dt] = MFMA16(kt[r * LD + 16 * dt], tt[r], acc[dt]);
                }
            }
        }
    }
    __syncthreads();
    float *Os = Ks;                                              // [4 waves][16 queries][LD]
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * dt + 4 * g + r;
            if (d < D) Os[(16 * w + l15) * LD + d] = acc[dt][r];
        }
    }
    __syncthreads();
    ab_write(dq, pe_q, Os, LD, C, ch0, D, (size_t)q0 + r0, nq);
}

template <int NT, bool VEC>
__device__ __forceinline__ void attention_dkv_body(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                                   const float *pos_q, const float *pos_k, const float *lse, const float *dout,
                                                   const float *delta, const int *offQ, const int *offK, int C, int D, float scale,
                                                   float sigma2, float *dk, float *dv) {
    constexpr int T = NT <= 9 ? 64 : 48;
    constexpr bool DV4 = NT == 17;                               // dv's probabilities from ab_chain4 (its comment)
    extern __shared__ __attribute__((aligned(16))) float at_sm[];
    const int t = threadIdx.x, h = blockIdx.y, b = blockIdx.z, H = gridDim.y;
    const int q0 = offQ[b], L = offQ[b + 1] - q0, k0 = offK[b], S = offK[b + 1] - k0;
    const int c0 = blockIdx.x * AT_BM;
    if (c0 >= S) return;
    const int DP = (D + 3) & ~3, LD = at_ld(DP), ndt = (D + 15) >> 4, ch0 = h * D;
    float *Ks = at_sm, *Vs = Ks + AT_BM * LD, *Qs = Vs + AT_BM * LD, *Gs = Qs + T * LD, *st = Gs + T * LD + 16, *Ps = st + AB_STATS;
    const int lane = t & 63, w = t >> 6, l15 = lane & 15, g = lane >> 4;
    const bool compat = pos_q != nullptr;
    const int nk = min(AT_BM, S - c0);
    at_stage<VEC>(Ks, LD, k, pe_k, C, ch0, D, DP, (size_t)k0 + c0, nk, AT_BM);
    at_stage<VEC>(Vs, LD, v, nullptr, C, ch0, D, DP, (size_t)k0 + c0, nk, AT_BM);
    f32x4 ak[NT], av[NT];
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) ak[dt] = av[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    float pk[AT_POS];                                            // key l15's own position (zeros beyond S: that row is never written)
#pragma unroll
    for (int u = 0; u < AT_POS; ++u) pk[u] = compat && l15 < nk ? pos_k[((size_t)k0 + c0 + l15) * AT_POS + u] : 0.f;
    const int n_it = (L + T - 1) / T;
    for (int it = 0; it < n_it; ++it) {
        if (it) __syncthreads();
        const int nv = min(T, L - it * T), nrows = (nv + 15) & ~15;
        const size_t g0 = (size_t)q0 + it * T;
        at_stage<VEC>(Qs, LD, q, pe_q, C, ch0, D, DP, g0, nv, nrows);
        at_stage<VEC>(Gs, LD, dout, nullptr, C, ch0, D, DP, g0, nv, nrows);
        if (t < T) {
            st[t] = t < nv ? lse[(g0 + t) * H + h] : 0.f;
            st[64 + t] = t < nv ? delta[(g0 + t) * H + h] : 0.f;
        }
        if (compat) {
            for (int idx = t; idx < T * AT_POS; idx += 256) Ps[idx] = idx < nv * AT_POS ? pos_q[g0 * AT_POS + idx] : 0.f;
        }
        __syncthreads();
        if (16 * w < nv) {
            const f32x4 sc = ab_chain(Qs + (16 * w + l15) * LD + g, Ks + l15 * LD + g, DP);
            const f32x4 sv = DV4 ? ab_chain4(Qs + (16 * w + l15) * LD + g, Ks + l15 * LD + g, DP) : sc;
            const f32x4 dp = ab_chain(Gs + (16 * w + l15) * LD + g, Vs + l15 * LD + g, DP);
            float p[4], tt[4];                                   // p: the probability that weighs do in dv; tt = ds scale c
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int qi = 16 * w + 4 * g + r;
                float a = sc[r], av4 = sv[r], cc = 1.0f;
                if (compat) {
                    const float *pq = Ps + qi * AT_POS;
                    const float dd = at_dist(pq, pk) - at_dist(pq + 3, pk + 3);
                    cc = fmaxf(0.f, 1.0f - (dd * dd) / sigma2);
                    a *= cc;
                    av4 *= cc;
                }
                const bool in = qi < nv && l15 < nk;
                const float pc = in ? ab_prob(scale * a, st[qi]) : 0.f;                      // the forward's p, for ds
                p[r] = !DV4 ? pc : in ? ab_prob(scale * av4, st[qi]) : 0.f;
                tt[r] = (pc * (dp[r] - st[64 + qi])) * (scale * cc);
            }
            const float *gt = Gs + (16 * w + 4 * g) * LD + l15, *qt = Qs + (16 * w + 4 * g) * LD + l15;
#pragma unroll
            for (int dt = 0; dt < NT; ++dt) {
                if (dt < ndt) {
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        av[dt] = MFMA16(gt[r * LD + 16 * dt], p[r], av[dt]);
                        ak[dt] = MFMA16(qt[r * LD + 16 * dt], tt[r], ak[dt]);
                    }
                }
            }
        }
    }
    __syncthreads();
    float *Os = Qs;                                              // [4 waves][16 keys][LD], dv first, then dk'
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * dt + 4 * g + r;
            if (d < D) Os[(16 * w + l15) * LD + d] = av[dt][r];
        }
    }
    __syncthreads();
    ab_write(dv, nullptr, Os, LD, C, ch0, D, (size_t)k0 + c0, nk);
    __syncthreads();
#pragma unroll
    for (int dt = 0; dt < NT; ++dt) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int d = 16 * dt + 4 * g + r;
            if (d < D) Os[(16 * w + l15) * LD + d] = ak[dt][r];
        }
    }
    __syncthreads();
    ab_write(dk, pe_k, Os, LD, C, ch0, D, (size_t)k0 + c0, nk);
}

#define AB_KERNELS(NAME, NT, VEC)                                                                                               \
    extern "C" __global__ void __launch_bounds__(256)                                                                           \
    k_attention_dq_##NAME(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const float *pos_q, \
                          const float *pos_k, const float *o, const float *lse, const float *dout, const int *offQ, const int *offK, \
                          int C, int D, float scale, float sigma2, float *delta, float *dq) {                                   \
        attention_dq_body<NT, VEC>(q, k, v, pe_q, pe_k, pos_q, pos_k, o, lse, dout, offQ, offK, C, D, scale, sigma2, delta, dq); \
    }                                                                                                                           \
    extern "C" __global__ void __launch_bounds__(256)                                                                           \
    k_attention_dkv_##NAME(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const float *pos_q, \
                           const float *pos_k, const float *lse, const float *dout, const float *delta, const int *offQ,        \
                           const int *offK, int C, int D, float scale, float sigma2, float *dk, float *dv) {                    \
        attention_dkv_body<NT, VEC>(q, k, v, pe_q, pe_k, pos_q, pos_k, lse, dout, delta, offQ, offK, C, D, scale, sigma2, dk, dv); \
    }
AB_KERNELS(d16, 1, false)
AB_KERNELS(d48, 3, false)
AB_KERNELS(d144, 9, false)
AB_KERNELS(d264, 17, false)
AB_KERNELS(d16_v4, 1, true)
AB_KERNELS(d48_v4, 3, true)
AB_KERNELS(d144_v4, 9, true)
AB_KERNELS(d264_v4, 17, true)
#undef AB_KERNELS

// pos_q / pos_k of the two entries below: both (the compatibility-modulated form, sigma_spat as ndp_attention_compat_forward's) or
// neither (the plain form; sigma_spat is not read) -> 0 with sigma2
static int ab_check_pos(const char *who, const float *pos_q, const float *pos_k, double sigma_spat, float *sigma2) {
    *sigma2 = 0.f;
    if ((pos_q == nullptr) != (pos_k == nullptr)) return failf(NDP_E_INVALID, "%s: pos_q and pos_k are passed as both or neither", who);
    if (!pos_q) return 0;
    if (!fm_aligned4(pos_q) || !fm_aligned4(pos_k)) return failf(NDP_E_INVALID, "%s: pointers must be 4-byte aligned", who);
    if (!(sigma_spat > 0)) return failf(NDP_E_INVALID, "%s: sigma_spat must be positive (inf: no compatibility), got %g", who, sigma_spat);
    *sigma2 = (float)(sigma_spat * sigma_spat);
    if (!(*sigma2 > 0)) return failf(NDP_E_INVALID, "%s: sigma_spat^2 = %g^2 underflows float32", who, sigma_spat);
    return 0;
}

extern "C" int ndp_attention_forward_lse(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                         const float *pos_q, const float *pos_k, const int *offQ, const int *offK, const int *offQ_host,
                                         const int *offK_host, int B, int C, int n_head, float scale, double sigma_spat, float *out,
                                         float *lse, void *stream) {
    const char *who = "ndp_attention_forward_lse";
    int maxL = 0;
    bool vec = false;
    float sigma2 = 0.f;
    if (int rc = at_check(who, q, k, v, pe_q, pe_k, offQ, offK, offQ_host, offK_host, B, C, n_head, scale, out, &maxL, &vec)) return rc;
    if (!lse) return failf(NDP_E_INVALID, "%s: null pointer", who);
    if (!fm_aligned4(lse)) return failf(NDP_E_INVALID, "%s: pointers must be 4-byte aligned", who);
    if (int rc = ab_check_pos(who, pos_q, pos_k, sigma_spat, &sigma2)) return rc;
    const int D = C / n_head, cls = at_class(D);
    const dim3 grid((maxL + AT_BM - 1) / AT_BM, n_head, B);
    if (pos_q) {
        using Kern = void (*)(const float *, const float *, const float *, const float *, const float *, const float *, const float *,
                              const int *, const int *, int, int, float, float, float *, float *);
        static const Kern kern[2][4] = {
            {k_attention_compat_lse_d16, k_attention_compat_lse_d48, k_attention_compat_lse_d144, k_attention_compat_lse_d264},
            {k_attention_compat_lse_d16_v4, k_attention_compat_lse_d48_v4, k_attention_compat_lse_d144_v4, k_attention_compat_lse_d264_v4}};
        const Kern fn = kern[vec][cls];
        const int pos_floats = AT_BN * AT_POS;
        if (int rc = set_smem((const void *)fn, 4 * (at_lds_floats(at_dmax[cls]) + pos_floats))) return rc;
        hipLaunchKernelGGL(fn, grid, dim3(256), 4 * (at_lds_floats(D) + pos_floats), (hipStream_t)stream, q, k, v, pe_q, pe_k, pos_q, pos_k,
                           offQ, offK, C, D, scale, sigma2, out, lse);
    } else {
        using Kern = void (*)(const float *, const float *, const float *, const float *, const float *, const int *, const int *, int, int,
                              float, float *, float *);
        static const Kern kern[2][4] = {{k_attention_lse_d16, k_attention_lse_d48, k_attention_lse_d144, k_attention_lse_d264},
                                        {k_attention_lse_d16_v4, k_attention_lse_d48_v4, k_attention_lse_d144_v4, k_attention_lse_d264_v4}};
        const Kern fn = kern[vec][cls];
        if (int rc = set_smem((const void *)fn, 4 * at_lds_floats(at_dmax[cls]))) return rc;
        hipLaunchKernelGGL(fn, grid, dim3(256), 4 * at_lds_floats(D), (hipStream_t)stream, q, k, v, pe_q, pe_k, offQ, offK, C, D, scale, out, lse);
    }
    HIP_TRY(hipGetLastError(), "k_attention_lse launch");
    return 0;
}

// o, lse: what ndp_attention_forward_lse wrote for the same arguments.  delta [sum L][n_head] is the call's workspace (written by the
// dq sweep, read by the dk / dv sweep).  Two launches on the stream; does not synchronise.
extern "C" int ndp_attention_backward(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                      const float *pos_q, const float *pos_k, const float *o, const float *lse, const float *dout,
                                      const int *offQ, const int *offK, const int *offQ_host, const int *offK_host, int B, int C, int n_head,
                                      float scale, double sigma_spat, float *delta, float *dq, float *dk, float *dv, void *stream) {
    const char *who = "ndp_attention_backward";
    int maxL = 0, maxS = 0;
    bool vec = false;
    float sigma2 = 0.f;
    if (int rc = at_check(who, q, k, v, pe_q, pe_k, offQ, offK, offQ_host, offK_host, B, C, n_head, scale, dq, &maxL, &vec)) return rc;
    if (!o || !lse || !dout || !delta || !dk || !dv) return failf(NDP_E_INVALID, "%s: null pointer", who);
    if (!fm_aligned4(o) || !fm_aligned4(lse) || !fm_aligned4(dout) || !fm_aligned4(delta) || !fm_aligned4(dk) || !fm_aligned4(dv))
        return failf(NDP_E_INVALID, "%s: pointers must be 4-byte aligned", who);
    if (int rc = ab_check_pos(who, pos_q, pos_k, sigma_spat, &sigma2)) return rc;
    for (int b = 0; b < B; ++b) maxS = std::max(maxS, offK_host[b + 1] - offK_host[b]);
    vec = vec && aligned16(dout) && aligned16(o);
    const int D = C / n_head, cls = at_class(D);
    using KernQ = void (*)(const float *, const float *, const float *, const float *, const float *, const float *, const float *,
                           const float *, const float *, const float *, const int *, const int *, int, int, float, float, float *, float *);
    using KernK = void (*)(const float *, const float *, const float *, const float *, const float *, const float *, const float *,
                           const float *, const float *, const float *, const int *, const int *, int, int, float, float, float *, float *);
    static const KernQ kq[2][4] = {{k_attention_dq_d16, k_attention_dq_d48, k_attention_dq_d144, k_attention_dq_d264},
                                   {k_attention_dq_d16_v4, k_attention_dq_d48_v4, k_attention_dq_d144_v4, k_attention_dq_d264_v4}};
    static const KernK kk[2][4] = {{k_attention_dkv_d16, k_attention_dkv_d48, k_attention_dkv_d144, k_attention_dkv_d264},
                                   {k_attention_dkv_d16_v4, k_attention_dkv_d48_v4, k_attention_dkv_d144_v4, k_attention_dkv_d264_v4}};
    const KernQ fq = kq[vec][cls];
    const KernK fk = kk[vec][cls];
    if (int rc = set_smem((const void *)fq, 4 * ab_lds_floats(at_dmax[cls]))) return rc;
    if (int rc = set_smem((const void *)fk, 4 * ab_lds_floats(at_dmax[cls]))) return rc;
    hipLaunchKernelGGL(fq, dim3((maxL + AT_BM - 1) / AT_BM, n_head, B), dim3(256), 4 * ab_lds_floats(D), (hipStream_t)stream, q, k, v, pe_q,
                       pe_k, pos_q, pos_k, o, lse, dout, offQ, offK, C, D, scale, sigma2, delta, dq);
    HIP_TRY(hipGetLastError(), "k_attention_dq launch");
    hipLaunchKernelGGL(fk, dim3((maxS + AT_BM - 1) / AT_BM, n_head, B), dim3(256), 4 * ab_lds_floats(D), (hipStream_t)stream, q, k, v, pe_q,
                       pe_k, pos_q, pos_k, lse, dout, delta, offQ, offK, C, D, scale, sigma2, dk, dv);
    HIP_TRY(hipGetLastError(), "k_attention_dkv launch");
    return 0;
}
