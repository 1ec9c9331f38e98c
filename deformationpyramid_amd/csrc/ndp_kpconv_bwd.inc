// ndp_kpconv_bwd.inc -- the backward of the rigid KPConv (ndp_kpconv_conv.inc) in the features x and the weights W: k_kpb_count,
// k_kpb_keys / k_kpb_rowstart (the transposed neighbour table), k_kpb_edge / k_kpb_gather (dx), k_kpb_dw / k_kpb_fold (dW);
// ndp_kpconv_backward and its workspace query.  DESIGN.md "KPConv backward".  Notation of ndp_kpconv_conv.inc's header.  Given dy [Nq,Cout]:
//
//   g[n,o]     = dy[n,o] / count[n]                        (normalize = 1: the forward's IEEE division by the same count; else g = dy)
//   dW[k,c,o]  = sum_n wf[n,k,c] g[n,o]
//   dwf[n,k,c] = sum_o g[n,o] W[k,c,o]
//   e[n,h,c]   = sum_k w(n,h,k) dwf[n,k,c]                 (the gradient one edge (n,h) sends to its support row)
//   dx[r,c]    = sum over (n,h) with idx[n,h] == r, valid:  e[n,h,c]
//
// count and the `closest` one-hot are constants (comparisons); q, s and kp get no gradient.  w is recomputed from the points with kpc_d2
// and the forward's influence expressions, so it has the forward's bits; nothing of the forward is kept but its inputs.  fp32 throughout,
// every contraction on the f32-input MFMA, no atomics, one writer per output element per launch, every sum in one fixed order: the same
// inputs give the same bits run to run.
//
// THE SUMMATION ORDERS.
//   dwf: one chain from 0 over o; an MFMA step t of a block of 16 columns contracts o = o0 + t, o0 + 4 + t, o0 + 8 + t, o0 + 12 + t
//        (a lane reads four consecutive columns as one 16-byte operand), the blocks o0 = 0, 16, ... ascending.
//   e:   one chain from 0 over k ascending (steps of 4) inside a group of 16 kernel points; at K > 16 the second group's sum is added to
//        the first's, which its own thread wrote to the slab buffer before.
//   dx:  ONE chain from +0 over the incoming edges of r in ascending (n,h).  The edges come from the transposed table: edge ids n H + h
//        sorted by support row with a stable radix sort (rocPRIM), shadows under the key Ns, which no row start ever reaches.  e passes
//        through global memory in slabs of queries (at most KB_SLAB_BYTES); a slab's gather continues the chain its predecessor left in
//        dx -- it reads dx[r,c], adds its edges in order and writes it back -- so the bits of dx do not depend on the slab size.  The
//        first slab's gather writes every row: a row without an incoming edge gets exactly +0.
//   wf:  as the forward's aggregation: one chain from 0 over h ascending.
//   dW:  a workgroup owns 16 kernel points x 16 input channels x 64 output channels (64 accumulators a lane) and walks query tiles of 16
//        in ascending order; a tile's step t contracts the queries 4 t .. 4 t + 3 of the tile: one chain from 0 over n.  When the block
//        count is small the walk is cut into `nseg` segments of consecutive tiles (a function of the dimensions alone: kpb_plan); each
//        segment writes its partial of the blocks it owns to the slab buffer and k_kpb_fold adds them, one thread per element, from
//        segment 0 upwards.  nseg K Cin Cout floats never exceed 32 MiB (nseg <= 512 / blocks, blocks >= K Cin Cout / 16384).
// SHADOWS.  Every idx outside 0 .. Ns-1 is a shadow here as in the forward: nothing is read for it, it sends nothing, and in the
// transposed table it sorts behind every row, where nothing looks.
#define KB_SLAB_BYTES (64LL << 20)
#define KB_WS 272                      // LDS words per query of k_kpb_dw's wf tile [16 k][16 c] (16 of padding: the four queries of an A read on 64 banks)
#define KB_GS 80                       // the same for its g tile [64 o]
#define KB_DW_TARGET 512               // workgroups k_kpb_dw aims at when it cuts the walk into segments

__device__ __forceinline__ float kpb_influence(float4 v, float kx, float ky, float kz, bool live, float extent, float gden, int influence) {
    float w = 0.f;
    if (live) {
        const float d2 = kpc_d2(v.x, v.y, v.z, kx, ky, kz);
        w = influence == 0 ? 1.f : influence == 1 ? fmaxf(0.f, 1.f - sqrtf(d2) / extent) : expf(-d2 / gden);
    }
    return w;
}

// rel[pl][h] = {s - q, the closest kernel point (0 without `closest`) or -1 for a shadow} of the tile's queries p0 .. p0 + 15 below n_end
__device__ __forceinline__ void kpb_tile_rel(float4 *rel, int *sidx, int Hs, const float *q, const float *s, const int *idx, const float *kp,
                                              long long p0, long long n_end, long long ns, int H, int K, int closest) {
    for (int i = threadIdx.x; i < KC_PT * Hs; i += 256) {
        const int pl = i / Hs, h = i - pl * Hs;
        const long long n = p0 + pl;
        long long r = -1;
        if (n < n_end && h < H) r = idx[(size_t)n * H + h];
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
                    if (d < best) { best = d; kmin = k; }
                }
            }
            v.w = __int_as_float(kmin);
        } else {
            r = -1;
        }
        rel[i] = v;
        if (sidx) sidx[i] = (int)r;
    }
}

// count[n] = max(1, #{h valid : flag[idx[n,h]]}): the forward's divisor
extern "C" __global__ void __launch_bounds__(256)
k_kpb_count(const int *__restrict__ idx, const int *__restrict__ flag, long long nq, long long ns, int H, int *__restrict__ cnt) {
    const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
    if (n >= nq) return;
    int c = 0;
    for (int h = 0; h < H; ++h) {
        const long long r = idx[(size_t)n * H + h];
        if (r >= 0 && r < ns && flag[r]) ++c;
    }
    cnt[n] = c > 1 ? c : 1;
}

// key[i] = the support row of edge i = n H + h, Ns for a shadow; val[i] = i
extern "C" __global__ void __launch_bounds__(256)
k_kpb_keys(const int *__restrict__ idx, long long ne, long long ns, unsigned *__restrict__ key, int *__restrict__ val) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= ne) return;
    const long long r = idx[i];
    key[i] = (r >= 0 && r < ns) ? (unsigned)r : (unsigned)ns;
    val[i] = (int)i;
}

// rstart[r] = the first position of the sorted keys that holds a key >= r, for r = 0 .. Ns (rstart[Ns]: where the shadows begin)
extern "C" __global__ void __launch_bounds__(256)
k_kpb_rowstart(const unsigned *__restrict__ key, long long ne, long long ns, int *__restrict__ rstart) {
    const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
    if (r > ns) return;
    long long lo = 0, hi = ne;
    while (lo < hi) {
        const long long mid = (lo + hi) >> 1;
        if (key[mid] < (unsigned)r) lo = mid + 1; else hi = mid;
    }
    rstart[r] = (int)lo;
}

// e[n - n0][h][c] for the queries n0 <= n < n1 of one slab.  A workgroup of four waves owns 16 queries and a chunk of 64 input channels
// (grid.y).  Per group of 16 kernel points: dwf[16 p][16 k][64 c] = g W^T over all of Cout into LDS (wave v: the kernel points v, v + 4,
// v + 8, v + 12, sixteen 16x16 accumulators), then per query e[H][64 c] = w[H][16 k] dwf[16 k][64 c] (wave v: the queries v, v + 4, ...).
// The dwf tile is stored with its 16-column blocks rotated by k & 3, so that the four kernel points of a B read fall on different banks.
extern "C" __global__ void __launch_bounds__(256)
k_kpb_edge(const float *__restrict__ q, const float *__restrict__ s, const int *__restrict__ idx, const float *__restrict__ W,
           const float *__restrict__ kp, const int *__restrict__ cnt, const float *__restrict__ dy, long long n0, long long n1, long long ns,
           int H, int K, int cin, int cout, float extent, float gden, int influence, int closest, int normalize, int wvec, float *e) {
    extern __shared__ __attribute__((aligned(16))) float kb_smem[];
    const int Hs = (H + 15) & ~15, coutp = (cout + 15) & ~15, gs = coutp + 4;
    float *dwf = kb_smem;                                                // [KC_PT][KC_PS]
    float4 *rel = reinterpret_cast<float4 *>(dwf + KC_PT * KC_PS);       // [KC_PT][Hs]
    float *gL = reinterpret_cast<float *>(rel + KC_PT * Hs);             // [KC_PT][gs]
    float *kpL = gL + KC_PT * gs;                                        // [KC_MAX_K][3]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, j = lane & 15, g = lane >> 4;
    const long long p0 = n0 + (long long)blockIdx.x * KC_PT;
    const int c0 = blockIdx.y * KC_CK, cw = min(KC_CK, cin - c0), nct = (cw + 15) >> 4;

    kpb_tile_rel(rel, nullptr, Hs, q, s, idx, kp, p0, n1, ns, H, K, closest);
    for (int i = t; i < 3 * KC_MAX_K; i += 256) kpL[i] = i < 3 * K ? kp[i] : 0.f;
    for (int i = t; i < KC_PT * coutp; i += 256) {
        const int pl = i / coutp, o = i - pl * coutp;
        const long long n = p0 + pl;
        float v = 0.f;
        if (n < n1 && o < cout) {
            v = dy[(size_t)n * cout + o];
            if (normalize) v = v / (float)cnt[n];
        }
        gL[pl * gs + o] = v;
    }

    for (int k0 = 0; k0 < K; k0 += KC_KG) {
        __syncthreads();                                                 // the prologue's tiles are written; the previous group's dwf is read
        // ---- dwf[p][kk][c] = sum_o g[p][o] W[k0 + kk][c0 + c][o]
        f32x4 acc[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int u = 0; u < 4; ++u) acc[i][u] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int o0 = 0; o0 < coutp; o0 += 16) {
            const float4 a = *reinterpret_cast<const float4 *>(gL + j * gs + o0 + 4 * g);
            const int o = o0 + 4 * g;
            float4 b[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int k = k0 + wv + 4 * i;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int c = 16 * u + j;
                    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
                    if (k < K && u < nct && c < cw && o < cout) {
                        const float *wp = W + ((size_t)k * cin + c0 + c) * cout + o;
                        if (wvec) {
                            v = *reinterpret_cast<const float4 *>(wp);   // cout % 4 == 0 and o % 4 == 0: all four inside
                        } else {
                            v.x = wp[0];
                            if (o + 1 < cout) v.y = wp[1];
                            if (o + 2 < cout) v.z = wp[2];
                            if (o + 3 < cout) v.w = wp[3];
                        }
                    }
                    b[i][u] = v;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (k0 + wv + 4 * i < K) {
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (u < nct) {
                            acc[i][u] = MFMA16(a.x, b[i][u].x, acc[i][u]);
                            acc[i][u] = MFMA16(a.y, b[i][u].y, acc[i][u]);
                            acc[i][u] = MFMA16(a.z, b[i][u].z, acc[i][u]);
                            acc[i][u] = MFMA16(a.w, b[i][u].w, acc[i][u]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int kk = wv + 4 * i;
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int r = 0; r < 4; ++r)                              // D: row 4 g + r = query, column j = channel; zeros where nothing was walked
                    dwf[(4 * g + r) * KC_PS + kk * KC_CK + ((16 * u + j + 16 * (kk & 3)) & 63)] = acc[i][u][r];
        }
        __syncthreads();
        // ---- e[p][h][c] = sum_kk w(p, h, k0 + kk) dwf[p][kk][c]
        for (int pi = 0; pi < KC_PT / 4; ++pi) {
            const int pl = wv + 4 * pi;
            const long long n = p0 + pl;
            if (n >= n1) continue;                                       // wave-uniform
            for (int h0 = 0; h0 < H; h0 += 16) {
                const float4 v = rel[pl * Hs + h0 + j];
                const int code = __float_as_int(v.w);
                float a[4];
#pragma unroll
                for (int tt = 0; tt < 4; ++tt) {
                    const int kk = 4 * tt + g, k = k0 + kk;
                    a[tt] = kpb_influence(v, kpL[3 * (k & 31)], kpL[3 * (k & 31) + 1], kpL[3 * (k & 31) + 2],
                                          code >= 0 && k < K && (!closest || code == k), extent, gden, influence);
                }
#pragma unroll
                for (int ct = 0; ct < 4; ++ct) {
                    if (ct < nct) {
                        f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                        for (int tt = 0; tt < 4; ++tt)                   // kk = 4 tt + g, kk & 3 = g
                            d = MFMA16(a[tt], dwf[pl * KC_PS + (4 * tt + g) * KC_CK + ((16 * ct + j + 16 * g) & 63)], d);
                        const int c = 16 * ct + j;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {                    // D: row 4 g + r = neighbour, column j = channel
                            const int h = h0 + 4 * g + r;
                            if (h < H && c < cw) {
                                float *ep = e + ((size_t)(n - n0) * H + h) * cin + c0 + c;
                                *ep = k0 == 0 ? d[r] : *ep + d[r];       // the second group of kernel points: this thread wrote *ep before
                            }
                        }
                    }
                }
            }
        }
    }
}

// One slab's share of dx: thread (r, c) walks the edges of r whose query lies in [n0, n1), in ascending edge id, and continues the chain
// in dx[r,c] (first slab: starts it at +0 and writes every row).
extern "C" __global__ void __launch_bounds__(256)
k_kpb_gather(const int *__restrict__ rstart, const int *__restrict__ edge, const float *__restrict__ e, long long n0, long long n1,
             long long ns, int H, int cin, int first, float *__restrict__ dx) {
    const long long total = ns * cin, step = (long long)gridDim.x * 256;
    const long long lo_id = n0 * H, hi_id = n1 * H;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += step) {
        const long long r = i / cin;
        const int c = (int)(i - r * cin);
        int lo = rstart[r], hi = rstart[r + 1];
        const int end = hi;
        while (lo < hi) {                                                // the first edge of this row at or behind the slab's first
            const int mid = (int)(((long long)lo + hi) >> 1);
            if (edge[mid] < lo_id) lo = mid + 1; else hi = mid;
        }
        const bool any = lo < end && edge[lo] < hi_id;
        if (!first && !any) continue;
        float acc = first ? 0.f : dx[i];
        for (int p = lo; p < end; ++p) {
            const long long id = edge[p];
            if (id >= hi_id) break;
            acc += e[(size_t)(id - lo_id) * cin + c];
        }
        dx[i] = acc;
    }
}

// dW's block (16 kernel points from k0, 16 input channels from c0, 64 output channels from o0) over the query tiles of one segment.
// Per tile: the neighbourhoods and g to LDS, wf[16 p][16 k][16 c] as the forward's aggregation computes it (wave v: the queries v, v + 4,
// v + 8, v + 12), then acc[(k, c)][o] += wf^T g with the tile's queries as the contracted index (wave v: the kernel points 4 v .. 4 v + 3).
extern "C" __global__ void __launch_bounds__(256)
k_kpb_dw(const float *__restrict__ q, const float *__restrict__ s, const int *__restrict__ idx, const float *__restrict__ x,
         const float *__restrict__ kp, const int *__restrict__ cnt, const float *__restrict__ dy, long long nq, long long ns, int H, int K,
         int cin, int cout, float extent, float gden, int influence, int closest, int normalize, int ncb, int nob, long long tiles_per_seg,
         long long ntiles, long long kcc, float *__restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) float kb_smem[];
    const int Hp = (H + 3) & ~3;
    float *wfL = kb_smem;                                                // [KC_PT][KB_WS]
    float *gL = wfL + KC_PT * KB_WS;                                     // [KC_PT][KB_GS]
    float4 *rel = reinterpret_cast<float4 *>(gL + KC_PT * KB_GS);        // [KC_PT][Hp]
    int *sidx = reinterpret_cast<int *>(rel + KC_PT * Hp);               // [KC_PT][Hp]
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, j = lane & 15, g = lane >> 4;
    const int ob = blockIdx.x % nob, cb = (blockIdx.x / nob) % ncb, kg = blockIdx.x / (nob * ncb);
    const int k0 = KC_KG * kg, c0 = 16 * cb, o0 = 64 * ob;
    const long long t0 = (long long)blockIdx.y * tiles_per_seg, t1 = min(ntiles, t0 + tiles_per_seg);
    const int kme = k0 + j;
    float kx = 0.f, ky = 0.f, kz = 0.f;
    if (kme < K) { kx = kp[3 * kme]; ky = kp[3 * kme + 1]; kz = kp[3 * kme + 2]; }
    const int ns4 = Hp >> 2;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int u = 0; u < 4; ++u) acc[i][u] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (long long tile = t0; tile < t1; ++tile) {
        const long long p0 = tile * KC_PT;
        __syncthreads();                                                 // the previous tile's contraction has read wfL and gL
        kpb_tile_rel(rel, sidx, Hp, q, s, idx, kp, p0, nq, ns, H, K, closest);
        for (int i = t; i < KC_PT * 64; i += 256) {
            const int pl = i >> 6, oo = i & 63;
            const long long n = p0 + pl;
            float v = 0.f;
            if (n < nq && o0 + oo < cout) {
                v = dy[(size_t)n * cout + o0 + oo];
                if (normalize) v = v / (float)cnt[n];
            }
            gL[pl * KB_GS + oo] = v;
        }
        __syncthreads();
        // ---- aggregation: wf[p][k][c] of this wave's four queries, the forward's chain over h
        for (int pi = 0; pi < KC_PT / 4; ++pi) {
            const int pl = wv + 4 * pi;
            f32x4 d = f32x4{0.f, 0.f, 0.f, 0.f};
            for (int s0 = 0; s0 < ns4; s0 += 8) {
                float xb[8];
#pragma unroll
                for (int st = 0; st < 8; ++st) {
                    if (s0 + st < ns4) {
                        const int r = sidx[pl * Hp + 4 * (s0 + st) + g];
                        xb[st] = (r >= 0 && c0 + j < cin) ? x[(size_t)r * cin + c0 + j] : 0.f;
                    }
                }
#pragma unroll
                for (int st = 0; st < 8; ++st) {
                    if (s0 + st < ns4) {
                        const float4 v = rel[pl * Hp + 4 * (s0 + st) + g];
                        const int code = __float_as_int(v.w);
                        const float w = kpb_influence(v, kx, ky, kz, code >= 0 && kme < K && (!closest || code == kme), extent, gden, influence);
                        d = MFMA16(w, xb[st], d);
                    }
                }
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) wfL[pl * KB_WS + (4 * g + r) * 16 + j] = d[r];       // D: row 4 g + r = k, column j = c
        }
        __syncthreads();
        // ---- contraction over the tile's queries
#pragma unroll
        for (int tt = 0; tt < 4; ++tt) {
            float b[4], a[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) b[u] = gL[(4 * tt + g) * KB_GS + 16 * u + j];
#pragma unroll
            for (int i = 0; i < 4; ++i) a[i] = wfL[(4 * tt + g) * KB_WS + (4 * wv + i) * 16 + j];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int u = 0; u < 4; ++u) acc[i][u] = MFMA16(a[i], b[u], acc[i][u]);
        }
    }
    // D of (i, u): row 4 g + r = input channel of the block, column j = output channel of the column tile u; kernel point k0 + 4 wv + i
    float *dst = out + (size_t)blockIdx.y * kcc;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int k = k0 + 4 * wv + i;
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int o = o0 + 16 * u + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = c0 + 4 * g + r;
                if (k < K && c < cin && o < cout) dst[((size_t)k * cin + c) * cout + o] = acc[i][u][r];
            }
        }
    }
}

// dW[i] = part[0][i] + part[1][i] + ... in ascending segment order
extern "C" __global__ void __launch_bounds__(256)
k_kpb_fold(const float *__restrict__ part, long long kcc, int nseg, float *__restrict__ dW) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= kcc) return;
    float acc = part[i];
    for (int sg = 1; sg < nseg; ++sg) acc += part[(size_t)sg * kcc + i];
    dW[i] = acc;
}

static int kpb_edge_smem_bytes(int H, int cout) {
    const int Hs = (H + 15) & ~15, coutp = (cout + 15) & ~15;
    return (KC_PT * KC_PS + KC_PT * Hs * 4 + KC_PT * (coutp + 4) + 3 * KC_MAX_K) * 4;
}
static int kpb_dw_smem_bytes(int H) {
    const int Hp = (H + 3) & ~3;
    return (KC_PT * KB_WS + KC_PT * KB_GS + KC_PT * Hp * 4 + KC_PT * Hp) * 4;
}

struct KpbPlan {                       // what the dimensions alone decide: the same for the size query and the entry
    long long ne, slabq, ntiles, tiles_per_seg, kcc, slab_bytes;
    int nseg, ncb, nob, nkg;
};

static int kpb_plan(const char *who, long long nq, long long ns, int H, int K, int cin, int cout, long long slab_queries, KpbPlan *p) {
    if (int rc = kpc_check_dims(who, nq, ns, H, K, cin, cout)) return rc;
    p->ne = nq * H;
    if (p->ne > 0x7fffffffLL) return failf(NDP_E_UNSUPPORTED, "%s: served are Nq H < 2^31 edges (an edge id is an int)", who);
    const long long per_query = (long long)H * cin * 4, most = std::max(16LL, KB_SLAB_BYTES / per_query / 16 * 16);
    if (slab_queries < 0 || slab_queries % 16 || slab_queries > most)
        return failf(NDP_E_INVALID, "%s: slab_queries must be 0 or a multiple of 16 whose slab fits %lld MiB (at most %lld here)", who,
                     KB_SLAB_BYTES >> 20, most);
    p->slabq = std::min((nq + 15) / 16 * 16, slab_queries ? slab_queries : most);
    p->ntiles = (nq + KC_PT - 1) / KC_PT;
    p->nkg = (K + KC_KG - 1) / KC_KG, p->ncb = (cin + 15) / 16, p->nob = (cout + 63) / 64;
    const long long blocks = (long long)p->nkg * p->ncb * p->nob;
    const long long want = std::min(p->ntiles, std::max(1LL, KB_DW_TARGET / blocks));
    p->tiles_per_seg = (p->ntiles + want - 1) / want;
    p->nseg = (int)((p->ntiles + p->tiles_per_seg - 1) / p->tiles_per_seg);
    p->kcc = (long long)K * cin * cout;
    p->slab_bytes = std::max(p->slabq * per_query, p->nseg > 1 ? p->nseg * p->kcc * 4 : 0LL);
    return 0;
}

struct KpbCarve {
    int *flag, *cnt, *vi, *vo, *rstart;
    unsigned *ki, *ko;
    void *tmp;
    float *slab;
    long long tmp_bytes, total;
};

static KpbCarve kpb_carve(void *ws, long long nq, long long ns, const KpbPlan &p) {
    KpCarve c(ws);
    KpbCarve o;
    o.flag = c.take<int>(ns);
    o.cnt = c.take<int>(nq);
    o.ki = c.take<unsigned>(p.ne);
    o.ko = c.take<unsigned>(p.ne);
    o.vi = c.take<int>(p.ne);
    o.vo = c.take<int>(p.ne);
    o.rstart = c.take<int>(ns + 1);
    o.tmp_bytes = kp_sort_temp_bound(p.ne);
    o.tmp = c.take<char>(o.tmp_bytes);
    o.slab = c.take<float>(p.slab_bytes / 4);                            // e of one slab, or dW's segment partials before it
    o.total = c.at;
    return o;
}

extern "C" int ndp_kpconv_backward_workspace(long long nq, long long ns, int H, int K, int cin, int cout, long long slab_queries, long long *nbytes) {
    if (!nbytes) return fail(NDP_E_INVALID, "ndp_kpconv_backward_workspace: null pointer");
    KpbPlan p;
    if (int rc = kpb_plan("ndp_kpconv_backward_workspace", nq, ns, H, K, cin, cout, slab_queries, &p)) return rc;
    *nbytes = kpb_carve(nullptr, nq, ns, p).total;
    return 0;
}

extern "C" int ndp_kpconv_backward(const float *q, const float *s, const int *idx, const float *x, const float *W, const float *kp,
                                   const float *dy, long long nq, long long ns, int H, int K, int cin, int cout, float extent, int influence,
                                   int aggregation, int normalize, long long slab_queries, void *ws, long long ws_bytes, float *dx, float *dW,
                                   void *stream) {
    const char *who = "ndp_kpconv_backward";
    KpbPlan p;
    if (int rc = kpb_plan(who, nq, ns, H, K, cin, cout, slab_queries, &p)) return rc;
    if (!q || !s || !idx || !x || !W || !kp || !dy || !ws) return failf(NDP_E_INVALID, "%s: null pointer", who);
    if (!dx && !dW) return failf(NDP_E_INVALID, "%s: dx and dW are both null: nothing to compute", who);
    for (const void *ptr : {(const void *)q, (const void *)s, (const void *)idx, (const void *)x, (const void *)W, (const void *)kp,
                            (const void *)dy, (const void *)dx, (const void *)dW})
        if ((uintptr_t)ptr & 3) return failf(NDP_E_INVALID, "%s: every array must be 4-byte aligned", who);
    if (!aligned16(ws)) return failf(NDP_E_INVALID, "%s: the workspace must be 16-byte aligned", who);
    if (!(extent > 0.f) || !std::isfinite(extent)) return failf(NDP_E_INVALID, "%s: extent must be positive and finite", who);
    if (influence < 0 || influence > 2) return failf(NDP_E_INVALID, "%s: influence must be 0 (constant), 1 (linear) or 2 (gaussian)", who);
    if (aggregation < 0 || aggregation > 1) return failf(NDP_E_INVALID, "%s: aggregation must be 0 (sum) or 1 (closest)", who);
    if (normalize < 0 || normalize > 1) return failf(NDP_E_INVALID, "%s: normalize must be 0 or 1", who);
    const KpbCarve c = kpb_carve(ws, nq, ns, p);
    if (ws_bytes < c.total) return failf(NDP_E_INVALID, "%s: workspace smaller than ndp_kpconv_backward_workspace(...)", who);
    const double sigma = 0.3 * (double)extent;
    const float gden = (float)(2.0 * sigma * sigma + 1e-9);
    hipStream_t st = (hipStream_t)stream;
    const dim3 block(256);
    if (dx) {                                                            // the sort's temporary size is rocPRIM's to name: asked before any launch
        int end_bit = 1;
        while (end_bit < 32 && (1LL << end_bit) <= ns) ++end_bit;
        size_t need = 0;
        HIP_TRY(rocprim::radix_sort_pairs(nullptr, need, c.ki, c.ko, c.vi, c.vo, (unsigned)p.ne, 0u, (unsigned)end_bit, st), "radix sort (size query)");
        if ((long long)need > c.tmp_bytes) return failf(NDP_E_UNSUPPORTED, "%s: the edge sort asks for more temporary storage than the workspace bound allows", who);
        if (int rc = set_smem((const void *)k_kpb_edge, kpb_edge_smem_bytes(KC_MAX_H, KC_MAX_C))) return rc;
    }
    if (dW)
        if (int rc = set_smem((const void *)k_kpb_dw, kpb_dw_smem_bytes(KC_MAX_H))) return rc;

    if (normalize) {
        hipLaunchKernelGGL(k_kpc_rowflag, dim3((unsigned)((ns + 15) / 16)), block, 0, st, x, ns, cin, c.flag);
        HIP_TRY(hipGetLastError(), "k_kpc_rowflag launch");
        hipLaunchKernelGGL(k_kpb_count, dim3((unsigned)((nq + 255) / 256)), block, 0, st, idx, (const int *)c.flag, nq, ns, H, c.cnt);
        HIP_TRY(hipGetLastError(), "k_kpb_count launch");
    }
    if (dW) {
        float *out = p.nseg > 1 ? c.slab : dW;
        hipLaunchKernelGGL(k_kpb_dw, dim3((unsigned)(p.nkg * p.ncb * p.nob), (unsigned)p.nseg), block, kpb_dw_smem_bytes(H), st, q, s, idx, x, kp,
                           (const int *)c.cnt, dy, nq, ns, H, K, cin, cout, extent, gden, influence, aggregation, normalize, p.ncb, p.nob,
                           p.tiles_per_seg, p.ntiles, p.kcc, out);
        HIP_TRY(hipGetLastError(), "k_kpb_dw launch");
        if (p.nseg > 1) {
            hipLaunchKernelGGL(k_kpb_fold, dim3((unsigned)((p.kcc + 255) / 256)), block, 0, st, (const float *)c.slab, p.kcc, p.nseg, dW);
            HIP_TRY(hipGetLastError(), "k_kpb_fold launch");
        }
    }
    if (dx) {
        int end_bit = 1;
        while (end_bit < 32 && (1LL << end_bit) <= ns) ++end_bit;
        hipLaunchKernelGGL(k_kpb_keys, dim3((unsigned)((p.ne + 255) / 256)), block, 0, st, idx, p.ne, ns, c.ki, c.vi);
        HIP_TRY(hipGetLastError(), "k_kpb_keys launch");
        size_t need = (size_t)c.tmp_bytes;
        HIP_TRY(rocprim::radix_sort_pairs(c.tmp, need, c.ki, c.ko, c.vi, c.vo, (unsigned)p.ne, 0u, (unsigned)end_bit, st), "radix sort");
        hipLaunchKernelGGL(k_kpb_rowstart, dim3((unsigned)((ns + 1 + 255) / 256)), block, 0, st, (const unsigned *)c.ko, p.ne, ns, c.rstart);
        HIP_TRY(hipGetLastError(), "k_kpb_rowstart launch");
        const int wvec = cout % 4 == 0 && ((uintptr_t)W & 15) == 0;
        const long long gather_blocks = std::min((ns * cin + 255) / 256, 1LL << 20);
        for (long long n0 = 0; n0 < nq; n0 += p.slabq) {
            const long long n1 = std::min(nq, n0 + p.slabq);
            hipLaunchKernelGGL(k_kpb_edge, dim3((unsigned)((n1 - n0 + KC_PT - 1) / KC_PT), (unsigned)((cin + KC_CK - 1) / KC_CK)), block,
                               kpb_edge_smem_bytes(H, cout), st, q, s, idx, W, kp, (const int *)c.cnt, dy, n0, n1, ns, H, K, cin, cout, extent, gden,
                               influence, aggregation, normalize, wvec, c.slab);
            HIP_TRY(hipGetLastError(), "k_kpb_edge launch");
            hipLaunchKernelGGL(k_kpb_gather, dim3((unsigned)gather_blocks), block, 0, st, (const int *)c.rstart, (const int *)c.vo,
                               (const float *)c.slab, n0, n1, ns, H, cin, n0 == 0 ? 1 : 0, dx);
            HIP_TRY(hipGetLastError(), "k_kpb_gather launch");
        }
    }
    return 0;
}
