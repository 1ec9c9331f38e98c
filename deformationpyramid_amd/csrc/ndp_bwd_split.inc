// ------------------------------------------------------------------------------------------------
// Level backward of the SPLIT arithmetic (engine gemm_mode bits 2 = bwd1, 4 = bwd2; gemm_mode 0 keeps the fp32-MFMA backward
// above).  Same arithmetic as ndp_fwd_split.inc -- every 128-wide contraction from two-way fp16 splits of both operands
// (x = hi + 2^-11 lo), three partial products, a main and a correction accumulator in fp32 -- and the same shape: ONE workgroup of 8
// waves per CU, a tile's dz and its input activation as row-major fp16 planes [2][64][..] in LDS, written once per tile from the fp32
// rows that come from HBM.
//   GRADIENT SCALE.  Activations and weights sit in fp16's range as they are; the gradient operands dz do not (1e-8 .. 1e-3, with
//   many binades inside one tile).  They are multiplied by S = 2^k before the split and the results by 1 / S afterwards -- both
//   exact -- with k chosen per pair and tick so that S max|dO| lies in [64, 128): k_eng_loss leaves max |dO| of the pair in
//   e.gmax[b].  dz2 = (dO Wh)[h2 > 0] and dz1 = (dz2 W2)[h1 > 0] are of dO's magnitude (the weights are O(0.1)); scaled values are
//   clamped to +-65504, which a gradient 500 times larger than every |dO| of its pair would need.
//   h0 IS RECOMPUTED in bwd1: the split forward does not store it, bwd1 forms z0 from the saved encoding with the forward's own two
//   MFMAs per point group (f8_l0_group: bitwise the split forward's h0) -- 131 MB per 128-pair tick less to write and as much less
//   to read.  (Behind an fp32 forward -- test configurations only -- the recomputed h0 differs from the forward's in its last bit.)
//   RELU MASKS are read from the hi plane of the activation: the split of an activation keeps hi > 0 whenever h > 0 (a positive h
//   below fp16's smallest subnormal gets hi = 2^-24, lo = the (negative) remainder -- still h = hi + 2^-11 lo exactly).
//   weight gradient  dW[o][k] += sum_p dz[p][o] h[p][k]  (contraction over the tile's 64 points): v_mfma_f32_32x32x16_f16, both
//                    operands need eight consecutive POINTS of one feature per lane = the transpose of the planes, which
//                    ds_read_b64_tr_b16 delivers on the way out of LDS (tr_frag: lane 4 j + q of a 16-lane group points at row
//                    p0 + j, columns c0 + 4 q ..; lane l receives column c0 + (l & 15) of rows p0 .. p0 + 3 -- any row stride).
//                    Wave w owns the 32 x 32 blocks (o-block w & 3, k-blocks 2 (w >> 2), + 1): 2 x 32 accumulator registers.
//   data gradient    dh[p][k] = sum_o dz[p][o] W[o][k]: v_mfma_f32_16x16x32_f16 with the TRANSPOSED weight slice as A operand
//                    (wave w owns input features 16 w .. 16 w + 15; 32 registers), B = the dz planes as they lie.
//   The small pieces stay on the vector pipe in fp32: bias gradients (column sums of the fp32 rows as they are loaded), ReLU masks
//   (sign of the activation's hi part), [dW0 | db0] (K = 6: per-lane fma, reduced across lanes once per launch).
// Sums are formed in a different order than in the fp32 kernels: tolerance parity, not bitwise (tests/test_hip_parity.py).
// The workgroup count per pair is half the fp32 kernels' (G / 2): workgroup x writes gradient partial x and ZEROES its regions of
// the partials x + G/2, ... that the update kernel also folds.
// ------------------------------------------------------------------------------------------------
typedef short s16x4v __attribute__((ext_vector_type(4)));
typedef short s16x8v __attribute__((ext_vector_type(8)));

// Row stride of the INPUT-ACTIVATION planes of the backward kernels: they are only ever read by transposing reads (weight gradient B
// operand) and 8-byte mask reads, and a 16-lane group of ds_read_b64_tr_b16 touches 4 rows x 32 contiguous bytes -- with 272-byte rows
// (right for the 16-byte fragment reads of the dz planes) those four pieces overlap in the banks, with 320-byte rows they tile all 64.
#ifndef B8_HROW
#define B8_HROW 160
#endif
// dz planes of bwd1 (read both ways: 16-byte fragments for the data gradient, transposing reads for the weight gradient): 336-byte rows
// keep the 16-byte reads of 16 rows conflict-free (84 words = 4 x 21) and spread the four rows of a transposing read over 0 / 20 / 40 / 60.
// (bwd2 has no LDS left for that and keeps 272-byte rows.)
#ifndef B8_ZROW1
#define B8_ZROW1 168
#endif
#define B8_HPLANE (64 * B8_HROW)
enum : int {                              // byte offsets of the dynamic LDS region of the split backward kernels
    B8_PZ = 0,                            // [2][64][F8_ROW] fp16: S dz of the layer
    B8_PH = B8_PZ + 2 * F8_PLANE * 2,     // [2][64][B8_HROW] fp16: the layer's input activation (bwd2 carve; bwd1 has its own below)
    B8_PE = B8_PH + 2 * B8_HPLANE * 2,    // [64][8] fp32 posenc rows (bwd1) / [64][16] dO rows (bwd2) -- 4 KB
    B8_FT = B8_PE + 64 * 16 * 4,          // [64][NDP_LD] fp32 tile (bwd2: h2, then dz1)
    B8_WH = B8_FT + 64 * NDP_LD * 4,      // [12][128] fp32 head matrix (bwd2)
    B8_TOTAL = B8_WH + NDP_WHROWS * NDP_W * 4
};
static constexpr int kSmemBwd8Bytes = B8_TOTAL;
enum : int {                              // bwd1: wider dz rows, no fp32 tile / head matrix
    B81_PZ = 0,
    B81_PH = B81_PZ + 2 * 64 * B8_ZROW1 * 2,
    B81_PE = B81_PH + 2 * B8_HPLANE * 2,          // [64][8] fp32 posenc rows
    B81_L0 = B81_PE + 64 * 8 * 4,                 // [64][F8_L0ROW] fp16: the tile's packed layer-0 operand rows (h0 recomputed)
    B81_TOTAL = B81_L0 + 64 * F8_L0ROW * 2
};
static constexpr int kSmemBwd18Bytes = B81_TOTAL;
static_assert(kSmemBwd18Bytes <= 160 * 1024, "split bwd1 LDS carve");
static_assert(kSmemBwd8Bytes <= 160 * 1024, "split backward LDS carve");

// eight consecutive points (16 ks + 8 (lane >> 5) ..) of feature f0 + (lane & 31) from a row-major plane
// (SWZ: the plane carries the fragment-read column swizzle f8_swz -- the dz planes, which are also read as 16-byte fragments)
template <int ROW, bool SWZ = false>
__device__ __forceinline__ h16x8 tr_frag(const _Float16 *plane, int ks, int f0, int lane) {
    const int lam = lane & 15, g = (lane >> 4) & 1, p0 = 16 * ks + 8 * (lane >> 5);
    const int r0 = p0 + (lam >> 2), c = f0 + 16 * g + 4 * (lam & 3);
    const _Float16 *a = plane + r0 * ROW + (SWZ ? c ^ f8_swz(r0) : c);
    const _Float16 *b = plane + (r0 + 4) * ROW + (SWZ ? c ^ f8_swz(r0 + 4) : c);
    const s16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v *)a);
    const s16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v *)b);
    const s16x8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(h16x8, v);
}

// The gradient scale of the pair: S = 2^k with S max|dO| in [64, 128), and 1 / S (both exact; S = 1 when every dO is zero)
struct B8Scale { float s, inv; };
__device__ __forceinline__ B8Scale b8_scale(const ndp_engine &e, int b) {
    const unsigned bits = e.gmax[b];
    int ex = (int)((bits >> 23) & 0xffu);                            // biased exponent of max |dO|
    if (bits == 0u) ex = 133;                                        // -> S = 1
    ex = ex < 8 ? 8 : (ex > 250 ? 250 : ex);
    B8Scale r;
    r.s = __uint_as_float((unsigned)(260 - ex) << 23);               // 2^(6 - (ex - 127))
    r.inv = __uint_as_float((unsigned)(ex - 6) << 23);
    return r;
}

// four float4 of a [64][128] fp32 tile per thread (rows (t >> 5) + 16 i, columns 4 (t & 31) ..) -> two fp16 planes.
// GRAD: a gradient tile -- scaled by `scale`, clamped to fp16's range.  Otherwise an activation (>= 0): hi > 0 whenever the value is.
template <int ROW, bool SWZ, bool GRAD>
__device__ __forceinline__ void b8_split_rows(const float4 (&v)[4], _Float16 *pl, int t, float scale = 1.0f) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (t >> 5) + 16 * i, c = SWZ ? (4 * (t & 31)) ^ f8_swz(row) : 4 * (t & 31);
        const float f[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
        h16x4 p0, p1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            _Float16 a, l;
            if (GRAD) {
                const float x = __builtin_amdgcn_fmed3f(f[e] * scale, -65504.0f, 65504.0f);
                f8_split2(x, a, l);
            } else {
                const float x = fminf(f[e], 65504.0f);
                a = (_Float16)(x > 0.f ? fmaxf(x, 5.9604645e-8f) : x);           // 2^-24: fp16's smallest subnormal
                l = (_Float16)((x - (float)a) * F8_LO_SCALE);
            }
            p0[e] = a; p1[e] = l;
        }
        *reinterpret_cast<h16x4 *>(pl + row * ROW + c) = p0;
        *reinterpret_cast<h16x4 *>(pl + 64 * ROW + row * ROW + c) = p1;
    }
}

// four activation values of point p, features c .. c + 3 (a lane of the 16x16 accumulator layout) -> the two fp16 planes; hi > 0
// whenever the value is (the rule of b8_split_rows for activations)
template <int ROW>
__device__ __forceinline__ void b8_split_act4(const float (&v)[4], _Float16 *pl, int p, int c) {
    h16x4 p0, p1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const float x = fminf(v[e], 65504.0f);
        const _Float16 a = (_Float16)(x > 0.f ? fmaxf(x, 5.9604645e-8f) : x);
        p0[e] = a; p1[e] = (_Float16)((x - (float)a) * F8_LO_SCALE);
    }
    *reinterpret_cast<h16x4 *>(pl + p * ROW + c) = p0;
    *reinterpret_cast<h16x4 *>(pl + 64 * ROW + p * ROW + c) = p1;
}

// transposed weight slice for the data gradient: A rows k = 16 wv + (lane & 15), contraction index o = 32 ks + 8 (lane >> 4) + e
__device__ __forceinline__ void b8_load_wt(const float *W /*[o][k]*/, int wv, int l15, int lk, h16x8 (&w)[2][4]) {
    const float *wc = W + 16 * wv + l15;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            _Float16 a, l;
            f8_split2(__builtin_amdgcn_fmed3f(wc[(32 * ks + 8 * lk + e) * NDP_W], -65504.0f, 65504.0f), a, l);
            w[0][ks][e] = a; w[1][ks][e] = l;
        }
}

// dW[2 blocks] += (S dz)^T h over the 64 points of the planes (wave: o-block ob, k-blocks kb, kb + 1); [m][0] main, [m][1] correction
template <int ZROW>
__device__ __forceinline__ void b8_wgrad_frags(const _Float16 *pz, const _Float16 *ph, int ks, int ob, int kb, int lane, h16x8 (&A)[2], h16x8 (&B)[2][2]) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {
        A[s] = tr_frag<ZROW, true>(pz + s * 64 * ZROW, ks, 32 * ob, lane);
        B[0][s] = tr_frag<B8_HROW>(ph + s * B8_HPLANE, ks, 32 * kb, lane);
        B[1][s] = tr_frag<B8_HROW>(ph + s * B8_HPLANE, ks, 32 * kb + 32, lane);
    }
}
// in the compiler's order (prefetching k-step ks + 1 behind the six MFMAs of k-step ks cost 24 registers: compile-time
// knobs, not the default, since retired)
template <int ZROW>
__device__ __forceinline__ void b8_wgrad(const _Float16 *pz, const _Float16 *ph, int ob, int kb, int lane, f32x16 (&acc)[2][2]) {
    h16x8 A[2], B[2][2];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        b8_wgrad_frags<ZROW>(pz, ph, ks, ob, kb, lane, A, B);
#pragma unroll
        for (int m = 0; m < 2; ++m) {
            acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[1], B[m][0], acc[m][1], 0, 0, 0);
            acc[m][1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], B[m][1], acc[m][1], 0, 0, 0);
            acc[m][0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[0], B[m][0], acc[m][0], 0, 0, 0);
        }
    }
}

// d[r] = (1 / S) sum_o (S dz)[16 g + l15][o] W[o][16 wv + 4 lk + r] for one of the tile's four point groups
template <int ZROW>
__device__ __forceinline__ void b8_dgrad_g(const h16x8 (&wt)[2][4], const _Float16 *pz, int g, int l15, int lk, float inv, f32x4v &d) {
    f32x4v dm, dc;
#pragma unroll
    for (int r = 0; r < 4; ++r) { dm[r] = 0.f; dc[r] = 0.f; }
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const _Float16 *rp = pz + (16 * g + l15) * ZROW + 32 * ks + ((8 * lk) ^ f8_swz(l15));
        const h16x8 B0 = *reinterpret_cast<const h16x8 *>(rp);
        const h16x8 B1 = *reinterpret_cast<const h16x8 *>(rp + 64 * ZROW);
        dc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[1][ks], B0, dc, 0, 0, 0);
        dc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[0][ks], B1, dc, 0, 0, 0);
        dm = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[0][ks], B0, dm, 0, 0, 0);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) d[r] = fmaf(dc[r], F8_LO_WEIGHT, dm[r]) * inv;
}

// The data gradient of a whole tile (bwd2), software-pipelined like f8_layer (F8_PIPE): the eight B fragments of point group g + 1 are
// requested before the twelve MFMAs of group g are issued, and the epilogue of group g - 1 -- epi(g, dm, dc, slice), cut into four
// slices by its caller -- sits between the k-steps of group g, pinned by scheduling barriers.  bwd1 keeps the compiler's order
// (b8_dgrad_g): it sits at the 256-register cap and the fragment ring spilled there (0.092 -> 0.102 ms; a compile-time knob, since retired).
template <int ZROW, class Epi>
__device__ __forceinline__ void b8_dgrad_tile(const h16x8 (&wt)[2][4], const _Float16 *pz, int l15, int lk, Epi epi) {
    constexpr int D = 2, NS = D + 1;                                  // fragments of step s + D are requested at step s (s = 4 g + ks)
    h16x8 Bf[NS][2];
    f32x4v dm[2], dc[2];
    const _Float16 *rp0 = pz + l15 * ZROW + ((8 * lk) ^ f8_swz(l15));
    auto fetch = [&](int s) {
        const _Float16 *rp = rp0 + 16 * (s >> 2) * ZROW + 32 * (s & 3);
        Bf[s % NS][0] = *reinterpret_cast<const h16x8 *>(rp);
        Bf[s % NS][1] = *reinterpret_cast<const h16x8 *>(rp + 64 * ZROW);
    };
#pragma unroll
    for (int s = 0; s < D; ++s) fetch(s);
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) { dm[g & 1][r] = 0.f; dc[g & 1][r] = 0.f; }
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int s = 4 * g + ks;
            if (s + D < 16) fetch(s + D);
            __builtin_amdgcn_sched_barrier(0);
            dc[g & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[1][ks], Bf[s % NS][0], dc[g & 1], 0, 0, 0);
            dc[g & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[0][ks], Bf[s % NS][1], dc[g & 1], 0, 0, 0);
            dm[g & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wt[0][ks], Bf[s % NS][0], dm[g & 1], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            if (g > 0) {
                epi(g - 1, dm[(g - 1) & 1], dc[(g - 1) & 1], ks);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) epi(3, dm[1], dc[1], e);
}

// store the wave's two 32 x 32 blocks of dW into a [128][128] gradient region
__device__ __forceinline__ void b8_store_dW(float *g, const f32x16 (&acc)[2][2], float inv, int ob, int kb, int l31, int h) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r)
            g[(32 * ob + mfma_row(r, h)) * NDP_W + 32 * (kb + m) + l31] = fmaf(acc[m][1][r], F8_LO_WEIGHT, acc[m][0][r]) * inv;
}

// column sums kept per thread (columns 4 (t & 31) .. + 3, rows (t >> 5) + 16 i) -> out[128]; scratch: >= 16 * 128 floats of LDS
// (LDS-only barriers: __syncthreads also waits for every global store of the wave to be acknowledged -- here the 64 gradient stores per
//  lane issued just before, a few microseconds at batch 1 -- and nothing below needs them ordered: the fused backward's tail, round 6)
template <bool LDS_ONLY = false>
__device__ __forceinline__ void b8_colsum_finish(const float4 &cs, float *scratch, float *out, int t) {
    if (LDS_ONLY) lds_barrier(); else __syncthreads();
    *reinterpret_cast<float4 *>(scratch + (t >> 5) * NDP_W + 4 * (t & 31)) = cs;
    if (LDS_ONLY) lds_barrier(); else __syncthreads();
    if (t < NDP_W) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += scratch[q * NDP_W + t];
        out[t] = s;
    }
}

struct Bwd8Setup {
    const float *params, *heads, *dO;
    float *act, *gpart;
    int n, plane, n_tiles, tile0, tile_step, n_part, p_stride;
};

// which tiles / which partial this workgroup owns; zero-fills [lo, hi) of the partials nobody writes.  false: nothing to do.
__device__ __forceinline__ bool eng_bwd8_setup(const ndp_engine &e, int parity, int lo, int hi, Bwd8Setup &j) {
    const int b = blockIdx.y, t = threadIdx.x;
    // (decision, level and geometry requested side by side and tested ONCE: the compiler sinks a load below every branch that does not
    //  need it -- three dependent scalar round trips in front of the weight requests)
    const ndp_pair_state *nsp = e.state + (size_t)(parity ^ 1) * e.B + b;   // written by k_eng_loss this tick
    struct { int decision, step_level; } ns;
    ns.decision = nsp->decision; ns.step_level = nsp->step_level;
    const ndp_pair_geom gm = e.geom[b];
    const int n = gm.K + gm.S;
    if ((ns.decision == NDP_DEC_IDLE) | (ns.decision == NDP_DEC_ADVANCE) | (n < 0) | (ns.step_level < 0)) return false;
    j.n = n; j.plane = e.n_cap; j.n_tiles = (n + NDP_TILE - 1) / NDP_TILE;
    j.tile0 = blockIdx.x; j.tile_step = gridDim.x;
    j.p_stride = e.p_stride;
    float *gp0 = e.gpart + (size_t)b * e.G * e.p_stride;
    const bool idle = (int)blockIdx.x >= j.n_tiles;                         // no tile: then the partials x + k G/2 have none either --
    const int zlo = idle ? 0 : lo, zhi = idle ? e.P : hi;                   // zero them entirely (whichever backward kernel runs first)
    for (int x = blockIdx.x + (idle ? 0 : gridDim.x); x < e.G; x += gridDim.x)   // else: our regions of the partials this launch does not have
        for (int i = zlo + t; i < zhi; i += 512) gp0[(size_t)x * e.p_stride + i] = 0.f;
    j.gpart = gp0 + (size_t)blockIdx.x * e.p_stride;
    if (idle) return false;
    j.params = e.params + ((size_t)b * e.m + ns.step_level) * e.p_stride;
    j.act = e.act + (size_t)b * 3 * e.n_cap * NDP_W;
    j.heads = e.heads + (size_t)b * e.n_cap * NDP_HROW;
    j.dO = e.dO + (size_t)b * e.n_cap * NDP_NHMAX;
    return true;
}

// ---- bwd1: dW1 += dz1^T h0 ; db1 ; dh0 = dz1 W1 ; dz0 = dh0 * [h0 > 0] ; [dW0 | db0] += dz0^T [pe | 1]
extern "C" __global__ void __launch_bounds__(512, 1)
k_eng_bwd1_8(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
    const ndp_layer_desc dd = {NDP_W, 2, 0, 0, 0, 0.f};
    const int off_W1 = ndp_off_Wi(&dd, 1), off_b1 = ndp_off_bi(&dd, 1), off_W0 = ndp_off_W0(&dd), off_b0 = ndp_off_b0(&dd);
    const int region_hi = ndp_off_Wi(&dd, 2);                       // [W0 | b0 | W1 | b1] is the head of the block
    Bwd8Setup j;
    if (!eng_bwd8_setup(e, parity, 0, region_hi, j)) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, lk = lane >> 4, l31 = lane & 31, h = lane >> 5;
    const int ob = wv & 3, kb = 2 * (wv >> 2);
    _Float16 *pz = reinterpret_cast<_Float16 *>(smb + B81_PZ), *ph = reinterpret_cast<_Float16 *>(smb + B81_PH);
    float *pes = reinterpret_cast<float *>(smb + B81_PE);
    _Float16 *l0rows = reinterpret_cast<_Float16 *>(smb + B81_L0);
    const B8Scale sc = b8_scale(e, blockIdx.y);
    h16x8 wt[2][4];
    b8_load_wt(j.params + off_W1, wv, l15, lk, wt);
    L0Ops w0;
    f8_l0_weights(j.params + off_W0, j.params + off_b0, 16 * wv + l15, lk, w0);
    f8_l0_init_rows(l0rows, 64, t, 512);
    f32x16 dW[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dW[m][0][r] = 0.f; dW[m][1][r] = 0.f; }
    float w0acc[4][7];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 7; ++c) w0acc[r][c] = 0.f;
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);                     // db1: column sums of the dz1 rows this thread loads
    // the fp32 rows of tile i + 1 are requested before the MFMAs of tile i are issued: the HBM latency sits under the contractions
    float4 vz[4];
    float pe6 = 0.f;
    auto request = [&](int tile) {
        const int base = tile * NDP_TILE;
        const float *zs = j.act + (2 * (size_t)j.plane + base) * NDP_W;
#pragma unroll
        for (int i = 0; i < 4; ++i) vz[i] = reinterpret_cast<const float4 *>(zs)[t + 512 * i];
        if (t < 384) pe6 = j.heads[(size_t)(base + t / 6) * NDP_HROW + 16 + t % 6];
    };
    request(j.tile0);
#ifdef NDP_PHASE_TIMING
    __shared__ unsigned long long arr[8];
    PT_INIT;
#endif
    for (int tile = j.tile0; tile < j.n_tiles; tile += j.tile_step) {
#ifdef NDP_PHASE_TIMING
        if (lane == 0) arr[wv] = __builtin_readcyclecounter();      // when each wave reaches the top barrier
#endif
        __syncthreads();                                             // the previous tile's reads of the planes are done
#ifdef NDP_PHASE_TIMING
        if (t < 8) { const unsigned long long a0 = arr[0], aw = arr[t]; pt_acc[t] += aw > a0 ? aw - a0 : 0; if (t == 0) pt_acc[8] += 1; }
#endif
#pragma unroll
        for (int i = 0; i < 4; ++i) { cs.x += vz[i].x; cs.y += vz[i].y; cs.z += vz[i].z; cs.w += vz[i].w; }
        b8_split_rows<B8_ZROW1, true, true>(vz, pz, t, sc.s);
        if (t < 384) { pes[(t / 6) * 8 + t % 6] = pe6; f8_l0_pack(pe6, t % 6, l0rows + (t / 6) * F8_L0ROW); }
        __syncthreads();
#pragma unroll
        for (int g = 0; g < 4; ++g) {                                // h0 = relu(z0) of the tile, this wave's 16 features, straight into the planes
            float z0[4];
            f8_l0_group(w0, l0rows, g, l15, lk, z0);
#pragma unroll
            for (int r = 0; r < 4; ++r) z0[r] = fmaxf(z0[r] * (1.0f / BF_HS), 0.f);                  // (f8_l0_group returns 2^6 z0)
            b8_split_act4<B8_HROW>(z0, ph, 16 * g + l15, 16 * wv + 4 * lk);
        }
        __syncthreads();
        if (tile + j.tile_step < j.n_tiles) request(tile + j.tile_step);
        b8_wgrad<B8_ZROW1>(pz, ph, ob, kb, lane, dW);
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4v d;
            b8_dgrad_g<B8_ZROW1>(wt, pz, g, l15, lk, sc.inv, d);
            const int p = 16 * g + l15;
            const h16x4 hm = *reinterpret_cast<const h16x4 *>(ph + p * B8_HROW + 16 * wv + 4 * lk);  // hi part: > 0 exactly where h0 is
            const float4 q0 = *reinterpret_cast<const float4 *>(pes + p * 8);
            const float2 q1 = *reinterpret_cast<const float2 *>(pes + p * 8 + 4);
            const float q[6] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float z0 = (float)hm[r] > 0.f ? d[r] : 0.f;
#pragma unroll
                for (int c = 0; c < 6; ++c) w0acc[r][c] = fmaf(z0, q[c], w0acc[r][c]);
                w0acc[r][6] += z0;
            }
        }
    }
    float *G = j.gpart;
    b8_store_dW(G + off_W1, dW, sc.inv, ob, kb, l31, h);
    float *scratch = reinterpret_cast<float *>(smb + B81_PZ);         // the planes are dead from here
    b8_colsum_finish(cs, scratch, G + off_b1, t);
    // [dW0 | db0]: lane partials for features 16 wv + 4 lk + r -> sum over the 16 lanes of the group
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 7; ++c) scratch[((16 * wv + 4 * lk + r) * 7 + c) * 16 + l15] = w0acc[r][c];
    __syncthreads();
    for (int i = t; i < NDP_W * 7; i += 512) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += scratch[i * 16 + q];
        const int k = i / 7, c = i % 7;
        if (c < 6) G[off_W0 + k * 6 + c] = s; else G[off_b0 + k] = s;
    }
    PT_FLUSH(24);
}

// ---- bwd2: dz2 = (dO Wh) * [h2 > 0] ; dWh += dO^T h2 ; dbh ; dW2 += dz2^T h1 ; db2 ; dh1 = dz2 W2 ; dz1 = dh1 * [h1 > 0] -> h2 plane
extern "C" __global__ void __launch_bounds__(512, 1)
k_eng_bwd2_8(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
    const ndp_layer_desc dd = {NDP_W, 2, 0, 0, 0, 0.f};
    const int off_W2 = ndp_off_Wi(&dd, 2), off_b2 = ndp_off_bi(&dd, 2), off_Wh = ndp_off_Wi(&dd, 3);
    Bwd8Setup j;
    if (!eng_bwd8_setup(e, parity, off_W2, e.P, j)) return;
    const int nh = make_head_cfg(desc_at_level(e.desc, e.state[(size_t)(parity ^ 1) * e.B + blockIdx.y].step_level)).nh;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, lk = lane >> 4, l31 = lane & 31, h = lane >> 5;
    const int ob = wv & 3, kb = 2 * (wv >> 2);
    _Float16 *pz = reinterpret_cast<_Float16 *>(smb + B8_PZ), *ph = reinterpret_cast<_Float16 *>(smb + B8_PH);
    float *dOs = reinterpret_cast<float *>(smb + B8_PE);             // [64][16] rows, read as broadcasts
    float *ft = reinterpret_cast<float *>(smb + B8_FT), *whs = reinterpret_cast<float *>(smb + B8_WH);
    const B8Scale sc = b8_scale(e, blockIdx.y);
    h16x8 wt[2][4];
    b8_load_wt(j.params + off_W2, wv, l15, lk, wt);
    for (int i = t; i < NDP_WHROWS * NDP_W; i += 512) whs[i] = i < nh * NDP_W ? j.params[off_Wh + i] : 0.f;
    f32x16 dW[2][2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dW[m][0][r] = 0.f; dW[m][1][r] = 0.f; }
    f32x4 gWh;                                                       // dWh[j = 4 lk + r][k = 16 wv + l15] on the fp32 16x16x4 MFMA
#pragma unroll
    for (int r = 0; r < 4; ++r) gWh[r] = 0.f;
    float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);                     // db2: column sums of the dz2 values this thread forms
    float4 gbh = make_float4(0.f, 0.f, 0.f, 0.f);                    // dbh partial: dO[row t >> 2][4 (t & 3) ..] over the tiles (t < 256)
    float4 v2[4], v1[4], vo = make_float4(0.f, 0.f, 0.f, 0.f);
    auto request = [&](int tile) {
        const int base = tile * NDP_TILE;
        const float *s2 = j.act + (2 * (size_t)j.plane + base) * NDP_W, *s1 = j.act + ((size_t)j.plane + base) * NDP_W;
#pragma unroll
        for (int i = 0; i < 4; ++i) { v2[i] = reinterpret_cast<const float4 *>(s2)[t + 512 * i]; v1[i] = reinterpret_cast<const float4 *>(s1)[t + 512 * i]; }
        if (t < 256) vo = reinterpret_cast<const float4 *>(j.dO + (size_t)base * NDP_NHMAX)[t];
    };
    request(j.tile0);
    __syncthreads();                                                 // whs staged
    PT_INIT;
    PT_DECL;
    for (int tile = j.tile0; tile < j.n_tiles; tile += j.tile_step) {
        const int base = tile * NDP_TILE;
        __syncthreads();                                             // the previous tile's reads of planes / tile / dO rows are done
        PT(0);
        b8_split_rows<B8_HROW, false, false>(v1, ph, t);             // h1 -> planes
#pragma unroll
        for (int i = 0; i < 4; ++i) *reinterpret_cast<float4 *>(ft + ((t >> 5) + 16 * i) * NDP_LD + 4 * (t & 31)) = v2[i];   // h2 -> fp32 tile
        if (t < 256) {
            *reinterpret_cast<float4 *>(dOs + 4 * t) = vo;
            gbh.x += vo.x; gbh.y += vo.y; gbh.z += vo.z; gbh.w += vo.w;
        }
        PT(1);
        __syncthreads();
        PT(2);
        // ---- dWh += dO^T h2 over the tile's 64 points (fp32 MFMA 16x16x4: A = dO[p][j = l15], B = h2[p][16 wv + l15]), HERE: it needs
        // only the h2 tile and the dO rows, and this phase (the dz2 chains, vector pipe only) has the matrix pipe idle (A/B on one box: 0.1437-0.1446 against 0.1476-0.1501 ms
        // with the stage behind the second barrier, in front of the weight-gradient MFMAs)
        {                                                           // every operand first (one LDS latency, not four), then the 16 MFMAs
            float oa[16], ob2[16];
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                const int p = mfma16_point(ks, lk);
                oa[ks] = dOs[p * NDP_NHMAX + l15]; ob2[ks] = ft[p * NDP_LD + 16 * wv + l15];
            }
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) gWh = MFMA16(oa[ks], ob2[ks], gWh);
        }
        PT(5);
        // dz2 of this thread's rows (t >> 5) + 16 i, columns 4 (t & 31) ..: the j = 0 .. nh-1 fma chain from zero, masked by h2 > 0
        float4 z[4];
        {
            float a[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) a[i][c] = 0.f;
            const float *dr = dOs + (t >> 5) * NDP_NHMAX;
            for (int jj = 0; jj < nh; ++jj) {                        // head row outermost: one read of its four weights serves the four rows
                const float4 w4 = *reinterpret_cast<const float4 *>(whs + jj * NDP_W + 4 * (t & 31));
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float dj = dr[16 * i * NDP_NHMAX + jj];
                    a[i][0] = fmaf(w4.x, dj, a[i][0]); a[i][1] = fmaf(w4.y, dj, a[i][1]);
                    a[i][2] = fmaf(w4.z, dj, a[i][2]); a[i][3] = fmaf(w4.w, dj, a[i][3]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                z[i] = make_float4(v2[i].x > 0.f ? a[i][0] : 0.f, v2[i].y > 0.f ? a[i][1] : 0.f, v2[i].z > 0.f ? a[i][2] : 0.f,
                                   v2[i].w > 0.f ? a[i][3] : 0.f);
                cs.x += z[i].x; cs.y += z[i].y; cs.z += z[i].z; cs.w += z[i].w;
            }
        }
        b8_split_rows<F8_ROW, true, true>(z, pz, t, sc.s);
        PT(3);
        __syncthreads();
        PT(4);
        if (tile + j.tile_step < j.n_tiles) request(tile + j.tile_step);
        b8_wgrad<F8_ROW>(pz, ph, ob, kb, lane, dW);
        PT(6);
        float *zo = j.act + (2 * (size_t)j.plane + base) * NDP_W;     // dz1 replaces h2 in HBM (bwd1 reads it)
        {
            h16x4 hm;
            float o4[4];
            b8_dgrad_tile<F8_ROW>(wt, pz, l15, lk, [&](int g, const f32x4v &dm, const f32x4v &dc, int r) {
                const int p = 16 * g + l15;
                if (r == 0) hm = *reinterpret_cast<const h16x4 *>(ph + p * B8_HROW + 16 * wv + 4 * lk);  // hi part: > 0 exactly where h1 is
                const float d = fmaf(dc[r], F8_LO_WEIGHT, dm[r]) * sc.inv;
                o4[r] = (float)hm[r] > 0.f ? d : 0.f;
                asm volatile("" : "+v"(o4[r]));
                if (r == 3) *reinterpret_cast<float4 *>(zo + p * NDP_W + 16 * wv + 4 * lk) = make_float4(o4[0], o4[1], o4[2], o4[3]);
            });
        }
        PT(7);
    }
    float *G = j.gpart;
    b8_store_dW(G + off_W2, dW, sc.inv, ob, kb, l31, h);
    float *scratch = reinterpret_cast<float *>(smb + B8_PZ);         // the planes are dead from here
    b8_colsum_finish(cs, scratch, G + off_b2, t);
    // ---- head stage results: dWh rows j < nh (D layout: lane holds column k = 16 wv + l15 of rows j = 4 lk + r), dbh
    float *gwh = G + off_Wh;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int jr = 4 * lk + r;
        if (jr < nh) gwh[jr * NDP_W + 16 * wv + l15] = gWh[r];
    }
    __syncthreads();
    if (t < 256) reinterpret_cast<float4 *>(scratch)[t] = gbh;
    __syncthreads();
    if (t < nh) {
        float s = 0.f;
        for (int q = 0; q < 64; ++q) s += scratch[4 * (4 * q + (t >> 2)) + (t & 3)];      // thread 4 q + (j >> 2), component j & 3
        gwh[nh * NDP_W + t] = s;
    }
    PT(8);
    PT_FLUSH(0);
}
