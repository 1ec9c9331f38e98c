// ndp_kpconv_conv.inc -- the rigid KPConv forward (blocks.py:229-374 of the reference with deformable = False) in one fused kernel:
// k_kpc_rowflag (the positive-row flag of the normalisation, one int per support row) and k_kpc_forward; ndp_kpconv_forward and
// its workspace query.  DESIGN.md "KPConv convolution".  fp32 throughout, no atomics, every output element has one writer and every
// sum one fixed order: the same inputs give the same bits, and a query's bits do not depend on the other queries of the call.
//
//   valid(n,h) = 0 <= idx[n,h] < Ns                       (anything else is a shadow: nothing is read for it, it contributes 0)
//   d2(n,h,k)  = |(s[idx[n,h]] - q[n]) - kp[k]|^2         (kpc_d2: the differences, then fmaf(ez, ez, fmaf(ey, ey, ex * ex)))
//   w(n,h,k)   = 1 | max(0, 1 - sqrt(d2) / extent) | exp(-d2 / gden),  gden = fl32(2 (0.3 extent)^2 + 1e-9) formed in double
//   closest:     w kept only for the k that attains min_k d2 (the lowest such k)
//   wf[n,k,c]  = sum_h w(n,h,k) x[idx[n,h],c]             (MFMA16: contraction over h ascending from 0)
//   y[n,o]     = sum wf[n,k,c] W[k,c,o]                   (MFMA16: per chunk of 64 c one chain from 0 over k ascending, then the
//                                                          chunk's c ascending; the chunks' sums added in ascending order -- a
//                                                          blocked sum, not the single (k, c) chain of the definition)
//   normalize:   y[n,:] /= max(1, #{h valid : flag[idx[n,h]]}),  flag[r] = sum_c x[r,c] > 0   (an IEEE division)
//
// SHAPE.  A workgroup of four waves owns KC_PT = 16 queries and KC_CT = 64 output channels (grid.y walks the rest of Cout).  Its prologue
// writes the tile's neighbourhoods to LDS once: rel[p][h] = {s - q, the closest kernel point or -1 for a shadow} and sidx[p][h] = the
// support row or -1, and counts the flagged neighbours.  Then, per chunk of KC_CK = 64 input channels and group of 16 kernel points:
//   aggregation: wave v takes the points v, v + 4, v + 8, v + 12.  For one point the product wf[16 k][64 c] = w[16 k][H] X[H][64 c]
//     is four 16x16 accumulators; the A operand w(h = 4 s + (lane >> 4), k = lane & 15) is computed in the lane from rel, the B
//     operand x[row(h)][16 ct + (lane & 15)] is gathered from global memory, the loads of 32 neighbours in flight before their
//     first product.  The result goes to LDS as wf[p][k][c].
//   contraction: wave v owns the output columns 16 v .. 16 v + 15 of the workgroup's slice, for all 16 points:
//     part += wf[16 p][kk] W[kk][16 o] over kk = (k, c); one MFMA step contracts c = 16 u + 4 t + (lane >> 4), so the steps
//     (u, t) walk c in ascending order.  A comes from LDS, B is streamed from L2, one kernel point's rows in flight at a time.
// Only k < K and c < Cin are walked; what a tile pads (h >= H, c >= Cin, o >= Cout, n >= Nq) is a zero operand, never a read.
// No [N,K,Cin], [N,H,Cin] or [N,H,K] array exists outside LDS and registers.
// WHAT IS REPEATED.  The aggregation -- the gather of the feature rows and the influences -- runs once per (tile, chunk, group of
// 16 kernel points, slice of 64 output channels): a feature row is read Cout / 64 times per (point, chunk), and twice that at
// K > 16, not once.  A slice of 128 channels (two column tiles per wave) measured slower at (2 000 points, 256 channels) and
// (600, 512): the kernel is bound by load latency and the narrow slice brings more waves.  DESIGN.md "KPConv convolution".
#define KC_PT 16
#define KC_CK 64
#define KC_CT 64                       // output channels per workgroup: 16 per wave
#define KC_KG 16                       // kernel points per group (K <= 32: one or two groups)
#define KC_PS (KC_KG * KC_CK + 4)      // LDS words per point of wf (4 of padding: the 16 points of an A-operand read spread over the banks)
#define KC_MAX_K 32
#define KC_MAX_H 64
#define KC_MAX_C 1024
#define KC_MAX_N (1LL << 30)

__device__ __forceinline__ float kpc_d2(float dx, float dy, float dz, float kx, float ky, float kz) {
    const float ex = dx - kx, ey = dy - ky, ez = dz - kz;
    return fmaf(ez, ez, fmaf(ey, ey, ex * ex));
}

// flag[r] = sum_c x[r][c] > 0.  Sixteen lanes per row: lane j sums c = j, j + 16, ... ascending, then a fixed butterfly.
extern "C" __global__ void __launch_bounds__(256)
k_kpc_rowflag(const float *x, long long ns, int cin, int *flag) {
    const long long r = (long long)blockIdx.x * 16 + (threadIdx.x >> 4);
    const int j = threadIdx.x & 15;
    float acc = 0.f;
    if (r < ns)
        for (int c = j; c < cin; c += 16) acc += x[(size_t)r * cin + c];
#pragma unroll
    for (int m = 8; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 16);
    if (r < ns && j == 0) flag[r] = acc > 0.f;
}

extern "C" __global__ void __launch_bounds__(256)
k_kpc_forward(const float *__restrict__ q, const float *__restrict__ s, const int *__restrict__ idx, const float *__restrict__ x,
              const float *__restrict__ W, const float *__restrict__ kp, const int *__restrict__ flag, long long nq, long long ns,
              int H, int K, int cin, int cout, float extent, float gden, int influence, int closest, int normalize, float *__restrict__ y) {
    extern __shared__ __attribute__((aligned(16))) float kc_smem[];
    const int Hp = (H + 3) & ~3;
    float *wf = kc_smem;                                                 // [KC_PT][KC_PS]
    float4 *rel = reinterpret_cast<float4 *>(wf + KC_PT * KC_PS);        // [KC_PT][Hp]
    int *sidx = reinterpret_cast<int *>(rel + KC_PT * Hp);               // [KC_PT][Hp]
    int *cnt = sidx + KC_PT * Hp;                                        // [KC_PT]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, j = lane & 15, g = lane >> 4;
    const long long p0 = (long long)blockIdx.x * KC_PT;

    // ---- prologue: the tile's neighbourhoods
    for (int i = t; i < KC_PT * Hp; i += 256) {
        const int pl = i / Hp, h = i - pl * Hp;
        const long long n = p0 + pl;
        long long r = -1;
        if (n < nq && h < H) r = idx[(size_t)n * H + h];
        float4 v = make_float4(0.f, 0.f, 0.f, __int_as_float(-1));
        if (r >= 0 && r < ns) {
            v.x = s[3 * (size_t)r] - q[3 * (size_t)n];
            v.y = s[3 * (size_t)r + 1] - q[3 * (size_t)n + 1];
            v.z = s[3 * (size_t)r + 2] - q[3 * (size_t)n + 2];
            int kmin = 0;
            if (closest) {
                float best = INFINITY;
                for (int k = 0; k < K; ++k) {
                    const float d = kpc_d2(v.x, v.y, v.z, kp[3 * k], kp[3 * k + 1], kp[3 * k + 2]);
                    if (d < best) { best = d; kmin = k; }                // strict: the lowest k among equals stays
                }
            }
            v.w = __int_as_float(kmin);
        } else {
            r = -1;
        }
        rel[i] = v;
        sidx[i] = (int)r;
    }
    __syncthreads();
    if (t < KC_PT) {
        int c = 0;
        if (normalize)
            for (int h = 0; h < H; ++h) {
                const int r = sidx[t * Hp + h];
                if (r >= 0 && flag[r]) ++c;
            }
        cnt[t] = c > 1 ? c : 1;
    }

    const int ns4 = Hp >> 2;                                             // MFMA steps of the aggregation: four neighbours each
    const int ob = blockIdx.y * KC_CT + 16 * wv, o = ob + j;             // this wave's first output column, this lane's column
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int c0 = 0; c0 < cin; c0 += KC_CK) {
        const int cw = min(KC_CK, cin - c0), nct = (cw + 15) >> 4;       // channels of this chunk, and their tiles of 16
        f32x4 part = f32x4{0.f, 0.f, 0.f, 0.f};                          // the chunk's own chain (at most 32 x 64 terms), added to acc once
        for (int k0 = 0; k0 < K; k0 += KC_KG) {
            const int kn = min(KC_KG, K - k0);
            const int kme = k0 + j;                                      // the kernel point of this lane's A operand
            float kx = 0.f, ky = 0.f, kz = 0.f;
            if (kme < K) { kx = kp[3 * kme]; ky = kp[3 * kme + 1]; kz = kp[3 * kme + 2]; }
            __syncthreads();                                             // the previous contraction has read wf (first pass: cnt is written)
            // ---- aggregation: wf[p][k][c] of this wave's four points
            for (int pi = 0; pi < KC_PT / 4; ++pi) {
                const int pl = wv + 4 * pi;
                f32x4 d[4];
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) d[ct] = f32x4{0.f, 0.f, 0.f, 0.f};
                for (int s0 = 0; s0 < ns4; s0 += 8) {                    // eight steps (32 neighbours) of loads in flight at a time
                    float xb[4][8];
#pragma unroll
                    for (int st = 0; st < 8; ++st) {
                        if (s0 + st < ns4) {
                            const int r = sidx[pl * Hp + 4 * (s0 + st) + g];
                            const float *xr = x + ((size_t)(r >= 0 ? r : 0) * cin + c0);
#pragma unroll
                            for (int ct = 0; ct < 4; ++ct) {
                                const int c = 16 * ct + j;
                                xb[ct][st] = (ct < nct && r >= 0 && c < cw) ? xr[c] : 0.f;
                            }
                        }
                    }
#pragma unroll
                    for (int st = 0; st < 8; ++st) {
                        if (s0 + st < ns4) {
                            const float4 v = rel[pl * Hp + 4 * (s0 + st) + g];
                            const int code = __float_as_int(v.w);
                            float w = 0.f;
                            if (code >= 0 && kme < K && (!closest || code == kme)) {
                                const float d2 = kpc_d2(v.x, v.y, v.z, kx, ky, kz);
                                w = influence == 0 ? 1.f : influence == 1 ? fmaxf(0.f, 1.f - sqrtf(d2) / extent) : expf(-d2 / gden);
                            }
#pragma unroll
                            for (int ct = 0; ct < 4; ++ct)
                                if (ct < nct) d[ct] = MFMA16(w, xb[ct][st], d[ct]);
                        }
                    }
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (ct < nct) {
#pragma unroll
                        for (int r = 0; r < 4; ++r) wf[pl * KC_PS + (4 * g + r) * KC_CK + 16 * ct + j] = d[ct][r];     // D: row 4 g + r = k, column j = c
                    }
                }
            }
            __syncthreads();
            // ---- contraction with W[k0 .. k0 + kn)[c0 .. c0 + cw)[this wave's columns]
            if (ob < cout) {                                             // wave-uniform: a column beyond Cout inside the 16 is a zero operand
                for (int k = 0; k < kn; ++k) {
                    const float *Wk = W + ((size_t)(k0 + k) * cin + c0) * cout;
                    float b[16];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (u < nct) {
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) {
                                const int c = 16 * u + 4 * tt + g;       // step (u, tt) contracts c = 16 u + 4 tt + 0 .. 3: ascending c
                                b[4 * u + tt] = (c < cw && o < cout) ? Wk[c * cout + o] : 0.f;                         // (< 2^16 + 2^10: an int offset from a uniform base)
                            }
                        }
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (u < nct) {
                            const float *ap = wf + j * KC_PS + k * KC_CK + 16 * u + g;                    // A: row j = point
#pragma unroll
                            for (int tt = 0; tt < 4; ++tt) part = MFMA16(ap[4 * tt], b[4 * u + tt], part);
                        }
                    }
                }
            }
        }
        acc += part;                                                     // chunks in ascending order: a blocked sum, whose error grows with the chunk, not with Cin
    }
    // ---- epilogue.  D: row 4 g + r = point, column j = output channel
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int pl = 4 * g + r;
        const long long n = p0 + pl;
        if (n < nq && o < cout) {
            float v = acc[r];
            if (normalize) v = v / (float)cnt[pl];
            y[(size_t)n * cout + o] = v;
        }
    }
}

static int kpc_smem_bytes(int H) {
    const int Hp = (H + 3) & ~3;
    return (KC_PT * KC_PS + KC_PT * Hp * 4 + KC_PT * Hp + KC_PT) * 4;
}

static int kpc_check_dims(const char *who, long long nq, long long ns, int H, int K, int cin, int cout) {
    if (nq < 1 || ns < 1 || H < 1 || K < 1 || cin < 1 || cout < 1) return failf(NDP_E_INVALID, "%s: every dimension must be >= 1", who);
    if (nq > KC_MAX_N || ns > KC_MAX_N || H > KC_MAX_H || K > KC_MAX_K || cin > KC_MAX_C || cout > KC_MAX_C)
        return failf(NDP_E_UNSUPPORTED, "%s: served are Nq, Ns <= 2^30, H <= %d, K <= %d, Cin, Cout <= %d", who, KC_MAX_H, KC_MAX_K, KC_MAX_C);
    return 0;
}

extern "C" int ndp_kpconv_forward_workspace(long long nq, long long ns, int H, int K, int cin, int cout, long long *nbytes) {
    if (!nbytes) return fail(NDP_E_INVALID, "ndp_kpconv_forward_workspace: null pointer");
    if (int rc = kpc_check_dims("ndp_kpconv_forward_workspace", nq, ns, H, K, cin, cout)) return rc;
    *nbytes = (ns * 4 + 15) / 16 * 16;                                   // the positive-row flags
    return 0;
}

extern "C" int ndp_kpconv_forward(const float *q, const float *s, const int *idx, const float *x, const float *W, const float *kp,
                                  long long nq, long long ns, int H, int K, int cin, int cout, float extent, int influence, int aggregation,
                                  int normalize, void *ws, long long ws_bytes, float *y, void *stream) {
    if (int rc = kpc_check_dims("ndp_kpconv_forward", nq, ns, H, K, cin, cout)) return rc;
    if (!q || !s || !idx || !x || !W || !kp || !ws || !y) return fail(NDP_E_INVALID, "ndp_kpconv_forward: null pointer");
    for (const void *p : {(const void *)q, (const void *)s, (const void *)idx, (const void *)x, (const void *)W, (const void *)kp, (const void *)y})
        if ((uintptr_t)p & 3) return fail(NDP_E_INVALID, "ndp_kpconv_forward: every array must be 4-byte aligned");
    if (!aligned16(ws)) return fail(NDP_E_INVALID, "ndp_kpconv_forward: the workspace must be 16-byte aligned");
    if (!(extent > 0.f) || !std::isfinite(extent)) return fail(NDP_E_INVALID, "ndp_kpconv_forward: extent must be positive and finite");
    if (influence < 0 || influence > 2) return fail(NDP_E_INVALID, "ndp_kpconv_forward: influence must be 0 (constant), 1 (linear) or 2 (gaussian)");
    if (aggregation < 0 || aggregation > 1) return fail(NDP_E_INVALID, "ndp_kpconv_forward: aggregation must be 0 (sum) or 1 (closest)");
    if (normalize < 0 || normalize > 1) return fail(NDP_E_INVALID, "ndp_kpconv_forward: normalize must be 0 or 1");
    if (ws_bytes < (ns * 4 + 15) / 16 * 16) return fail(NDP_E_INVALID, "ndp_kpconv_forward: workspace smaller than ndp_kpconv_forward_workspace(...)");
    const double sigma = 0.3 * (double)extent;
    const float gden = (float)(2.0 * sigma * sigma + 1e-9);
    hipStream_t st = (hipStream_t)stream;
    int *flag = (int *)ws;
    if (normalize) {
        hipLaunchKernelGGL(k_kpc_rowflag, dim3((unsigned)((ns + 15) / 16)), dim3(256), 0, st, x, ns, cin, flag);
        HIP_TRY(hipGetLastError(), "k_kpc_rowflag launch");
    }
    const dim3 grid((unsigned)((nq + KC_PT - 1) / KC_PT), (unsigned)((cout + KC_CT - 1) / KC_CT)), block(256);
    if (int rc = set_smem((const void *)k_kpc_forward, kpc_smem_bytes(KC_MAX_H))) return rc;
    hipLaunchKernelGGL(k_kpc_forward, grid, block, kpc_smem_bytes(H), st, q, s, idx, x, W, kp, (const int *)flag, nq, ns, H, K, cin, cout,
                       extent, gden, influence, aggregation, normalize, y);
    HIP_TRY(hipGetLastError(), "k_kpc_forward launch");
    return 0;
}
