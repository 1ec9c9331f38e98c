// ------------------------------------------------------------------------------------------------
// Level forward of the SPLIT arithmetic (engine gemm_mode bit 1; gemm_mode 0 keeps the fp32-MFMA forward above).
//   Every contraction -- layer 0 (K = 6 + bias), the two 128 x 128 layers, the heads -- is evaluated from TWO-WAY fp16 SPLITS of both
//   operands in the ONE-ACCUMULATOR form: x' = 2^6 x (activations and weights alike), hi = fp16(x'), lo = fp16(x' - hi) unscaled --
//   11 + 11 significant bits and a sign, |x' - hi - lo| <= max(2^-22 |x'|, 2^-25) -- and THREE partial products on
//   v_mfma_f32_16x16x32_f16 into ONE fp32 accumulator (lo.hi, hi.lo, hi.hi; lo.lo is dropped), which then holds 2^12 of the layer's
//   pre-activation.  The pre-scale keeps lo in fp16's NORMAL range whenever hi is (an unscaled remainder of a weight of 0.09 would
//   be subnormal and lose its bits); operands are O(1) activations and O(0.1) weights here: a value beyond 1023 saturates.  (Round 3
//   and the first half of round 4: x = hi + 2^-11 lo with a main and a correction accumulator -- still the arithmetic of the
//   two-launch backward, ndp_bwd_split.inc; rounds 2 and 3: three-way bf16 splits and six products -- same accuracy class,
//   tests/test_split_accuracy.py, at twice the MFMAs.)  The fp32 MFMA runs at the fp32 VECTOR rate, the 16-bit MFMA at 16 times
//   that.  (Round 4 read tools/experiments/micro/coexec.hip as "neither runs next to the vector pipe of its SIMD"; round 5's
//   coexec2.hip -- independent MFMAs, fillers placed BETWEEN them -- shows two vector instructions hiding in every 16x16x32 gap:
//   f8_layer below is ordered for that.)  The epilogues: ONE v_med3 on the accumulator for ReLU and the fp16 bound, then scale +
//   convert + pack in one instruction per half (v_fma_mixlo/hi_f16) -- and a compare + select more only where the hi plane is read
//   as a ReLU mask (h1).  Results agree with the fp32 fma chain to its own rounding level but are not bitwise the chain.  The warp
//   is the exact arithmetic of the bitwise path.
//   Shape: ONE workgroup of 8 waves per CU.  Wave w owns 16 output columns of BOTH matrices (2 x 2 parts x 4 k-steps x 4 = 64
//   registers as MFMA A operands); a tile's activations are two row-major fp16 planes [2][64][136] in LDS, written straight from
//   the accumulator registers of the producing layer (a lane holds four consecutive features of a point); two plane sets alternate
//   between the layers (and between tiles) in fwd8_tile, three with fixed roles in the engine's pipelined forward (level_fwd9_body:
//   layer 0 and the heads ride in the layers' MFMA gaps, two barriers per tile); to HBM: h2 as fp32 rows from the registers, h1 as
//   fp32 rows or -- for the fused backward -- as that kernel's plane image, copied out of the planes in 1 KiB pieces; h0 only for a
//   backward on the fp32 MFMA; the heads read h2 as planes too.  With one workgroup per CU nothing hides a serial phase, so the per-point warp (one wave, 5.5k cycles of
//   dependent transcendental latency per tile) runs behind the workgroup's tile loop, 512 threads wide (eng_warp_tail), unless a
//   workgroup owns a single tile (the batch-1 shape: its 64 threads warp the tile's points).  Same head_warp_fwd code, same bits.
// ------------------------------------------------------------------------------------------------
// Workgroup barrier for LDS hazards only.  __syncthreads() also drains the vector-memory counter (s_waitcnt vmcnt(0)): every barrier
// of a tile then waits for the activation rows that were just queued for HBM -- nobody in these kernels reads them back.
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef _Float16 h16x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x2v __attribute__((ext_vector_type(2)));
typedef unsigned u32x4v __attribute__((ext_vector_type(4)));

#define F8_ROW 136                        /* 16-bit elements per plane row: 128 + 8 pad (272 B) */
#define F8_NP 2                           /* planes of a set in the forward: hi, lo */
#define F8_LO_SCALE 2048.0f               /* lo = fp16(2^11 (x - hi)): the two-accumulator form of the two-launch backward */
#define F8_LO_WEIGHT (1.0f / 2048.0f)
// Column swizzle of the planes that are read as 16-byte MFMA fragments (lane (l15, lk) reads row l15, columns 32 ks + 8 lk ..).  With
// 272-byte rows row r starts 4 banks after row r - 1, so the sixteen rows of ONE lk tile the 64 banks -- but a ds_read_b128 is not
// served by lk: its 16-lane groups are {0-3, 12-15, 20-27}, {4-11, 16-19, 28-31}, ... (MI355X_MICROARCH.md, LDS), i.e. rows 0-3 and
// 12-15 of one lk with rows 4-11 of the NEXT, and row 11 of lk + 1 lands on the banks of row 12 of lk: a 2-way conflict in every
// group, 0.39-0.48 of all LDS cycles in the three level kernels (profiles/r03_sq_counters_pmc.json, before).  Swapping the two
// 16-byte granules of each pair in rows 4..11 (mod 16) makes every group read ONE granule column of sixteen different rows.
__device__ __forceinline__ int f8_swz(int row) { return (((row >> 2) ^ (row >> 3)) & 1) << 3; }     // XOR on the bf16 column index
#define F8_PLANE (64 * F8_ROW)
// ---- the ONE-ACCUMULATOR split format (round 4; the fused backward's, this forward's, and the h1 plane image's in HBM): a tensor is
// multiplied by a power of two (2^6 for activations and weights), hi = fp16(x'), lo = fp16(x' - hi) UNSCALED, so that
// hi.hi + hi.lo + lo.hi add up in one fp32 accumulator.
#define BF_ROW 128                                /* fp16 elements per row of a plane image (256 B, no padding) */
#define BF_PLANE (64 * BF_ROW)
#define BF_HS 64.0f                               /* pre-scale of activations */
#define BF_WS 64.0f                               /* pre-scale of weights */
// granule swizzle of a plane image: XOR on the 16-byte granule index of a row (16 granules per row).  High two bits = row & 3
// (transposing reads), low two bits = g[(row >> 2) & 3], g = {0, 2, 3, 1} (fragment reads: ndp_bwd_fused.inc).
__device__ __forceinline__ int bf_swz(int row) { return (((row & 3) << 2) | ((0x1320 >> (((row >> 2) & 3) << 2)) & 3)) << 3; }   // XOR on the fp16 column index
#ifndef F8_PE_TILES
#define F8_PE_TILES 8
#endif
#define F8_L0ROW 32                       /* fp16 per packed layer-0 row of a point: the 32 contraction slots of one MFMA (20 used) */
enum : int {                              // byte offsets of the dynamic LDS region
    F8_PL0 = 0,                           // [2][64][F8_ROW] fp16: layer 0 -> layer 1, and layer 2 -> heads
    F8_PL1 = F8_PL0 + F8_NP * F8_PLANE * 2,   // [2][64][F8_ROW] fp16: layer 1 -> layer 2
    F8_PE = F8_PL1 + F8_NP * F8_PLANE * 2,    // F8_PE_TILES x [64][F8_L0ROW] fp16: packed layer-0 operand rows of a chunk of the workgroup's tiles
    F8_WH = F8_PE + F8_PE_TILES * 64 * F8_L0ROW * 2, // [2][16][F8_ROW] fp16 head weights (rows >= nh zero)
    F8_BH = F8_WH + F8_NP * 16 * F8_ROW * 2,  // [16] fp32 head bias
    F8_TOTAL = F8_BH + NDP_NHMAX * 4,         // (what k_pyramid_fwd8 builds on)
    F8_PL2 = F8_TOTAL,                        // [2][64][F8_ROW] fp16: the THIRD plane set of the engine's pipelined forward (level_fwd9_body: h2)
    F9_TOTAL = F8_PL2 + F8_NP * F8_PLANE * 2
};
static constexpr int kSmemFwd8Bytes = F9_TOTAL;
static_assert(kSmemFwd8Bytes <= 160 * 1024, "split forward LDS carve");

// x' (already scaled) -> hi, lo of the one-accumulator form.  ACT: an activation (>= 0): hi > 0 whenever the value is (the ReLU
// masks of the backward are read from the hi plane).
template <bool ACT>
__device__ __forceinline__ void bf_split(float x, _Float16 &hi, _Float16 &lo) {
    if (ACT) {
        x = fminf(x, 65504.0f);
        hi = (_Float16)(x > 0.f ? fmaxf(x, 5.9604645e-8f) : x);                  // 2^-24: fp16's smallest subnormal
    } else {
        x = __builtin_amdgcn_fmed3f(x, -65504.0f, 65504.0f);
        hi = (_Float16)x;
    }
    lo = (_Float16)(x - (float)hi);
}
// x' = 2^6 relu(v) saturated at fp16's largest value, from v' = 2^6 v: one v_med3 (ReLU and the bound together).
__device__ __forceinline__ float bf_act(float vs) { return __builtin_amdgcn_fmed3f(vs, 0.f, 65504.0f); }
// Where the hi plane of x' is going to be read as a ReLU mask, the mask travels in the SIGN of the hi part -- hi = -0 where v <= 0,
// hi >= +0 where v > 0 (a positive activation below fp16's range becomes +0): ONE v_med3 against -0 does ReLU, bound and mask (the
// median of (v, -0, bound) is -0 for v < 0), the conversions keep the sign of zero, and a -0 operand adds nothing to any product sum
// (x + -0 = x, and +0 + -0 = +0: the sums' bits do not change).  The backward reads the mask as "sign bit clear" (bf_pos).  A
// pre-activation that is EXACTLY +0 gives hi = +0, i.e. counts as positive (its contribution is multiplied by h = 0 or is a ReLU
// derivative at the kink: torch takes 0 there; this takes 1 -- measure zero for float inputs, documented in DESIGN section 4).
// Round 6 measured it against the earlier mask "hi > 0", which floored positive activations at fp16's smallest subnormal -- a compare,
// a v_med3 and a select per element in the forward's epilogues and in the backward's recomputation of h0 (a compile-time knob, since
// retired: profiles/r06_signmask_ab.txt).
__device__ __forceinline__ float bf_act_s(float vs) { return __builtin_amdgcn_fmed3f(vs, -0.0f, 65504.0f); }
__device__ __forceinline__ bool bf_pos(_Float16 hi) {
    return __builtin_amdgcn_classh(hi, 0x3c0);                       // +0, +subnormal, +normal, +inf: one v_cmp_class_f16, like the compare it replaces
}
// the split of such an x' (bf_split<true> without its bound and floor)
__device__ __forceinline__ void bf_split_act(float x, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}
// The same split from BOUNDED values y (>= 0, <= 65504 / s) in two instructions per element: v_fma_mixlo/hi_f16 multiplies by the scale
// s, converts and writes one half of the packed pair -- hi = fp16(s y) -- and the lo part's instruction reads that half back as its fp16
// addend: lo = fp16(s y - hi).  s y and s y - hi are exact in fp32 (s a power of two), so these are the bits of bf_split_act(s y)
// (tools/experiments/micro/mixprobe.hip: every in-range value, subnormal results included).  What it replaces per element: a
// multiplication, half a packing conversion, a conversion back, a subtraction, half a packing conversion.  NOT a saving in issue time: a
// v_fma_mix costs 8 cycles of its SIMD's vector issue, twice a plain VALU instruction (profiles/r05_micro_fma_mix.txt: three of them
// hide in a 32x32x16 gap where five or six v_med3 / conversions do) -- two of them are worth the four-and-a-half instructions they
// replace, no more.  In the forward's epilogue, which rides in MFMA gaps, it is instruction count and registers that matter; the same
// substitution in the fused backward and in the weight prologues, whose splits sit in the open, measured 4 % SLOWER
// (profiles/r05_bwd_mix_split_ab.txt: bitwise the same results) and was not kept.
template <bool SCALED, bool UPPER>
__device__ __forceinline__ void bf_mix_hi(unsigned &h, float y, float s) {          // half of h = fp16(s y); the LOWER half first (it defines h)
    if (SCALED) {
        if (UPPER) asm("v_fma_mixhi_f16 %0, %1, %2, 0" : "+v"(h) : "v"(y), "s"(s));
        else asm("v_fma_mixlo_f16 %0, %1, %2, 0" : "=v"(h) : "v"(y), "s"(s));
    } else {
        if (UPPER) asm("v_fma_mixhi_f16 %0, %1, 1.0, 0" : "+v"(h) : "v"(y));
        else asm("v_fma_mixlo_f16 %0, %1, 1.0, 0" : "=v"(h) : "v"(y));
    }
}
template <bool SCALED, bool UPPER>
__device__ __forceinline__ void bf_mix_lo(unsigned &l, float y, float s, unsigned h) {   // half of l = fp16(s y - the same half of h)
    if (SCALED) {
        if (UPPER) asm("v_fma_mixhi_f16 %0, %1, %2, -%3 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(y), "s"(s), "v"(h));
        else asm("v_fma_mixlo_f16 %0, %1, %2, -%3 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(y), "s"(s), "v"(h));
    } else {
        if (UPPER) asm("v_fma_mixhi_f16 %0, %1, 1.0, -%2 op_sel:[0,0,1] op_sel_hi:[0,0,1]" : "+v"(l) : "v"(y), "v"(h));
        else asm("v_fma_mixlo_f16 %0, %1, 1.0, -%2 op_sel_hi:[0,0,1]" : "=v"(l) : "v"(y), "v"(h));
    }
}
__device__ __forceinline__ void f8_split2(float x, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16)x;
    lo = (_Float16)((x - (float)hi) * F8_LO_SCALE);
}

// three-way bf16 split (the backward kernels' contractions, whose gradient operands span more binades than fp16 has)
__device__ __forceinline__ void f8_split3(float x, __bf16 &hi, __bf16 &mid, __bf16 &lo) {
    hi = (__bf16)x;
    const float r1 = x - (float)hi;
    mid = (__bf16)r1;
    lo = (__bf16)(r1 - (float)mid);
}

// ---- layer 0 (K = 6 encodings + bias) as ONE MFMA of packed split operands, the same one in the forward and in the backwards (which
// recompute h0 instead of reading it back: the forward does not store it) -- bitwise the same z0 in all of them.  One-accumulator
// format: W' = 2^6 W0 = Whi + Wlo, b' = 2^6 b0 = bhi + blo, pe = phi + plo (lo parts unscaled), the three partial products and the
// bias side by side in the 32 contraction slots of v_mfma_f32_16x16x32_f16 (lane (l15, lk) holds slots 8 lk .. 8 lk + 7):
//   slot    0..5        6     7     8..13       14..19      20..31
//   A       Whi[o][c]   bhi   blo   Whi[o][c]   Wlo[o][c]   0
//   B       phi[p][c]   1     1     plo[p][c]   phi[p][c]   0               ->  2^6 z0[p][o]
// A point's B operands are one row of F8_L0ROW fp16 in LDS (64 bytes: a wave's sixteen rows of a group are 1 KiB in a piece, one
// conflict-free 16-byte read per lane).  (Until round 4: two MFMAs -- main and 2^-11 correction accumulators -- and per group two
// reads whose padding lanes were zeroed by eight selects.)
struct L0Ops { h16x8 a; };
__device__ __forceinline__ void f8_l0_weights(const float *W0, const float *b0, int o, int lk, L0Ops &w) {
    _Float16 wh[6], wl[6], bh, bl;
#pragma unroll
    for (int c = 0; c < 6; ++c) bf_split<false>(W0[o * 6 + c] * BF_WS, wh[c], wl[c]);
    bf_split<false>(b0[o] * BF_WS, bh, bl);
    const _Float16 z = (_Float16)0.f;
    const h16x8 s0 = {wh[0], wh[1], wh[2], wh[3], wh[4], wh[5], bh, bl};
    const h16x8 s1 = {wh[0], wh[1], wh[2], wh[3], wh[4], wh[5], wl[0], wl[1]};
    const h16x8 s2 = {wl[2], wl[3], wl[4], wl[5], z, z, z, z};
    const h16x8 zz = {z, z, z, z, z, z, z, z};
    w.a = lk == 0 ? s0 : (lk == 1 ? s1 : (lk == 2 ? s2 : zz));
}

// one encoding value v (component c = 2 axis + {0 sin, 1 cos}) of a point -> its slots of the point's packed row
__device__ __forceinline__ void f8_l0_pack(float v, int c, _Float16 *row) {
    const _Float16 a = (_Float16)v, l = (_Float16)(v - (float)a);
    row[c] = a; row[8 + c] = l; row[14 + c] = a;
}
// the constant slots of n rows (the two "1" against the bias parts, zero padding): once per buffer
__device__ __forceinline__ void f8_l0_init_rows(_Float16 *rows, int n, int t, int nthreads) {
    for (int i = t; i < n; i += nthreads) {
        _Float16 *r = rows + i * F8_L0ROW;
        r[6] = (_Float16)1.0f; r[7] = (_Float16)1.0f;
#pragma unroll
        for (int q = 20; q < 32; ++q) r[q] = (_Float16)0.f;
    }
}
// 2^6 z0 of points 16 g + l15 (this lane: features 16 wv + 4 lk + r), from the tile's packed rows
__device__ __forceinline__ void f8_l0_group(const L0Ops &w, const _Float16 *rows, int g, int l15, int lk, float (&z)[4]) {
    const h16x8 b = *reinterpret_cast<const h16x8 *>(rows + (16 * g + l15) * F8_L0ROW + 8 * lk);
    f32x4v m = {0.f, 0.f, 0.f, 0.f};
    m = __builtin_amdgcn_mfma_f32_16x16x32_f16(w.a, b, m, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) z[r] = m[r];
}

struct Fwd8Weights {
    h16x8 w1[2][4], w2[2][4];             // [hi, lo][k-step of 32] of 2^6 W (one-accumulator format): row o = 16 wv + (lane & 15), k = 32 ks + 8 (lane >> 4) .. + 7
    L0Ops w0;                             // layer 0 of row o = 16 wv + (lane & 15): packed operand of its MFMA
    float b1[4], b2[4];                   // 2^12 b: the accumulators of layers 1 and 2 hold 2^12 z
};

__device__ __forceinline__ void f8_load_matrix(const float *W, int wv, int l15, int lk, h16x8 (&w)[2][4]) {
    const float *wr = W + (16 * wv + l15) * NDP_W + 8 * lk;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        const float4 v0 = *reinterpret_cast<const float4 *>(wr + 32 * ks), v1 = *reinterpret_cast<const float4 *>(wr + 32 * ks + 4);
        const float f[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            _Float16 a, l;
            bf_split<false>(f[e] * BF_WS, a, l);
            w[0][ks][e] = a; w[1][ks][e] = l;
        }
    }
}

__device__ __forceinline__ void fwd8_load_weights(const HeadCfg &hc, const float *P, unsigned char *smb, Fwd8Weights &fw) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, lk = lane >> 4;
    _Float16 *whs = reinterpret_cast<_Float16 *>(smb + F8_WH);
    float *bhs = reinterpret_cast<float *>(smb + F8_BH);
    const ndp_layer_desc dd = {NDP_W, 2, hc.motion, hc.rotfmt, 0, hc.mlp_scale};
    const float *W0 = P + ndp_off_W0(&dd), *b0 = P + ndp_off_b0(&dd);
    const float *W1 = P + ndp_off_Wi(&dd, 1), *b1 = P + ndp_off_bi(&dd, 1);
    const float *W2 = P + ndp_off_Wi(&dd, 2), *b2 = P + ndp_off_bi(&dd, 2);
    const float *Wh = P + ndp_off_Wi(&dd, 3);
    const float *bh = Wh + hc.nh * NDP_W;
    // The head matrix and bias are REQUESTED first and unconditionally (clamped index; a row >= nh is zeroed afterwards): as
    // `i < nh * 128 ? Wh[i] : 0` in a loop every one of the four items was a branch around a load with its own wait -- four dependent
    // global round trips behind the weights', half of the prologue of a single-tile workgroup (batch 1: round 6).
    static_assert(16 * NDP_W == 4 * 512, "four head-matrix items per thread");
    float whv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) whv[u] = Wh[min(t + 512 * u, hc.nh * NDP_W - 1)];
    const float bhv = bh[min(t, hc.nh - 1)];
    f8_load_matrix(W1, wv, l15, lk, fw.w1);
    f8_load_matrix(W2, wv, l15, lk, fw.w2);
    f8_l0_weights(W0, b0, 16 * wv + l15, lk, fw.w0);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int o = 16 * wv + 4 * lk + r;
        fw.b1[r] = b1[o] * (BF_WS * BF_HS); fw.b2[r] = b2[o] * (BF_WS * BF_HS);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {                                  // head matrix 2^6 Wh as two fp16 planes [16][F8_ROW] (rows >= nh zero)
        const int i = t + 512 * u;
        _Float16 a, l;
        bf_split<false>(i < hc.nh * NDP_W ? whv[u] * BF_WS : 0.f, a, l);
        const int o = (i >> 7) * F8_ROW + ((i & 127) ^ f8_swz(i >> 7));
        whs[o] = a; whs[16 * F8_ROW + o] = l;
    }
    if (t < NDP_NHMAX) bhs[t] = (t < hc.nh) ? bhv * (BF_WS * BF_HS) : 0.f;
}

// One point group's layer-0 value zs = 2^6 z (lane: point 16 g + l15, features 16 wv + 4 lk .. + 3) -> 2^6 relu(z) as the two fp16 planes layer 1
// reads; rows: the fp32 rows of relu(z) a backward on the fp32 MFMA reads, or nullptr.  (h0 as a plane image for the fused backward,
// like h1, was measured in round 4: that kernel 6 % shorter without its recomputation, this one 9 % longer with the extra 32 KB per
// tile to store -- no gain; the backward recomputes h0 from the saved encodings.)
__device__ __forceinline__ void f8_epilogue_v(const float (&z)[4], int g, _Float16 *pl, float *rows, int wv, int l15, int lk) {
    const int p = 16 * g + l15, c = 16 * wv + 4 * lk;
    if (rows)
        *reinterpret_cast<float4 *>(rows + p * NDP_W + c) = make_float4(fmaxf(z[0] * (1.0f / BF_HS), 0.f), fmaxf(z[1] * (1.0f / BF_HS), 0.f),
                                                                         fmaxf(z[2] * (1.0f / BF_HS), 0.f), fmaxf(z[3] * (1.0f / BF_HS), 0.f));
    float y[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) y[e] = bf_act(z[e]);
    unsigned hi[2], lo[2];
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        bf_mix_hi<false, false>(hi[q], y[2 * q], 1.0f); bf_mix_hi<false, true>(hi[q], y[2 * q + 1], 1.0f);
        bf_mix_lo<false, false>(lo[q], y[2 * q], 1.0f, hi[q]); bf_mix_lo<false, true>(lo[q], y[2 * q + 1], 1.0f, hi[q]);
    }
    _Float16 *dst = pl + p * F8_ROW + (c ^ f8_swz(l15));
    const u32x2v P0 = {hi[0], hi[1]}, P1 = {lo[0], lo[1]};
    *reinterpret_cast<u32x2v *>(dst) = P0;
    *reinterpret_cast<u32x2v *>(dst + F8_PLANE) = P1;
}
// 2^12 (bias + W h) for the wave's 16 columns: the three partial products of a k-step (lo.hi, hi.lo, hi.hi of 2^6 W and 2^6 h) into ONE
// accumulator per 16-point group.  ORDER (round 5).  tools/experiments/micro/coexec2.hip (profiles/r05_micro_coexec2.txt) measured
// what round 4's microbenchmark could not see behind its dependent MFMA triplets: a vector instruction placed BETWEEN two independent
// MFMAs is free -- two of them per 16x16x32 gap (five or six per 32x32x16 gap), with one wave per SIMD or two -- while behind a
// block of back-to-back MFMAs it is paid in full (the wave issues in order; a dependent MFMA, or simply the busy pipe, stalls
// everything that follows it in program order).  So: the four point groups are taken in two PAIRS; the two accumulators of a pair
// alternate MFMA by MFMA (consecutive MFMAs are independent: no issue stall on the accumulator, and a gap after each one), the
// epilogue of the first pair -- activation, split, stores: 26-30 small steps -- is dealt out over the gaps of the second pair's 24
// MFMAs, and the fragment reads of k-step s + 2 sit in front of k-step s.  Only the second pair's epilogue is in the open (the other
// wave of the SIMD, which runs a few hundred cycles apart, has MFMAs to place next to it).  Per accumulator the order of the
// products is what it was (k-step major; lo.hi, hi.lo, hi.hi): bitwise round 4's results.
// The epilogue itself costs 3 vector instructions per element instead of 5 (7 with the mask floor: 5): v_med3 for ReLU and bound on
// the accumulator as it is, then bf_mix_hi / bf_mix_lo (scale, convert, pack in one).  The bias is the C operand of the group's
// first MFMA (no accumulator initialisation).
struct F8Pair { float y[8]; unsigned hi[4], lo[4]; };
#define F8_ACC_BOUND (65504.0f * BF_WS)          /* 2^12 z that saturates 2^6 relu(z) at fp16's largest value */
//   planes (LDS): 2^6 h for the next layer;   rows: fp32 rows of h (the activation store of every backward but the fused one) or nullptr;
//   img: the tile's PLANE IMAGE in HBM or nullptr -- the fused backward's LDS layout (two [64][128] fp16 planes hi | lo, 256-byte
//   rows, bf_swz), which that kernel pulls into its region by LDS-DMA with nothing left to convert.
// Step k of the epilogue of the pair (g0, g0 + 1) -- one or two vector instructions each, except the stores.  Per group u (13 or 15
// steps): for each of its two packed pairs q: y, y, hi lower, hi upper, lo lower, lo upper; [rows: two steps of two scalings;] stores.
template <bool MASKED, bool ROWS>
struct F8EpiSteps { static constexpr int PER_GROUP = 12 + (ROWS ? 3 : 1), N = 2 * PER_GROUP; };
template <bool MASKED, bool ROWS>
__device__ __forceinline__ void f8_epi_step(F8Pair &st, const f32x4v &a0, const f32x4v &a1, int k, int g0, _Float16 *pl, float *rows,
                                            int wv, int l15, int lk) {
    constexpr int PG = F8EpiSteps<MASKED, ROWS>::PER_GROUP;
    const int u = k / PG, j = k - u * PG;                            // group of the pair, step within the group
    const f32x4v &am = u ? a1 : a0;
    if (j < 12) {
        const int q2 = j / 6, i = j - 6 * q2, e = 4 * u + 2 * q2, q = 2 * u + q2;   // packed pair q = elements e, e + 1 of the state
        if (i < 2) {
            const float v = am[2 * q2 + i];
            st.y[e + i] = __builtin_amdgcn_fmed3f(v, MASKED ? -0.0f : 0.f, F8_ACC_BOUND);
        }
        else if (i == 2 && MASKED) {                                 // scale, convert, pack -- keeping the sign of zero (v_fma_mix's + 0 would lose it)
            typedef float f32x2s __attribute__((ext_vector_type(2)));
            const f32x2s tv = {st.y[e] * (1.0f / BF_WS), st.y[e + 1] * (1.0f / BF_WS)};
            st.hi[q] = __builtin_bit_cast(unsigned, __builtin_convertvector(tv, h16x2));
        }
        else if (i == 3 && MASKED) {}
        else if (i == 2) bf_mix_hi<true, false>(st.hi[q], st.y[e], 1.0f / BF_WS);
        else if (i == 3) bf_mix_hi<true, true>(st.hi[q], st.y[e + 1], 1.0f / BF_WS);
        else if (i == 4) bf_mix_lo<true, false>(st.lo[q], st.y[e], 1.0f / BF_WS, st.hi[q]);
        else bf_mix_lo<true, true>(st.lo[q], st.y[e + 1], 1.0f / BF_WS, st.hi[q]);
        return;
    }
    const int g = g0 + u, p = 16 * g + l15, c = 16 * wv + 4 * lk;
    if (ROWS && j < 14) {                                            // h = 2^-12 y in place (the bounded value: 1023.5 at most)
        const int e = 4 * u + 2 * (j - 12);
        st.y[e] *= 1.0f / (BF_WS * BF_HS); st.y[e + 1] *= 1.0f / (BF_WS * BF_HS);
        return;
    }
    // (an UNSIGNED 32-bit element offset from the tile's uniform base: the store then takes the base from scalar registers and the
    //  offset from one vector register -- a signed int offset made every store a 64-bit vector add)
    if (ROWS) { const f32x4v rv = {st.y[4 * u], st.y[4 * u + 1], st.y[4 * u + 2], st.y[4 * u + 3]}; __builtin_nontemporal_store(rv, reinterpret_cast<f32x4v *>(rows + (unsigned)(p * NDP_W + c))); }
    _Float16 *dst = pl + p * F8_ROW + (c ^ f8_swz(l15));
    const u32x2v P0 = {st.hi[2 * u], st.hi[2 * u + 1]}, P1 = {st.lo[2 * u], st.lo[2 * u + 1]};
    *reinterpret_cast<u32x2v *>(dst) = P0;
    *reinterpret_cast<u32x2v *>(dst + F8_PLANE) = P1;
}
// A tile's activation planes (LDS, the forward's layout: 272-byte rows, f8_swz) -> its PLANE IMAGE in HBM (the fused backward's LDS
// layout: two [64][128] fp16 planes hi | lo, 256-byte rows, bf_swz -- that kernel pulls it in by LDS-DMA with nothing left to convert).
// Both swizzles move whole 16-byte granules within a row, so a lane carries one granule and a wave-instruction stores 1 KiB of
// CONTIGUOUS image: 4 reads + 4 stores per wave and tile.  (Until round 5 the image left from the accumulator registers, 8 bytes per
// lane and plane: a wave-instruction covered sixteen 32-byte row segments, and tools/experiments/micro/store_patterns.hip shows what
// that costs -- a CU streams a tile's 64 KB in 5.0-5.6k cycles in that shape against 3.1-3.2k, the HBM rate, with 16-byte stores.)
struct F8Copy { u32x4v v[4]; };
__device__ __forceinline__ void f8_image_read(const _Float16 *pl, int wv, int lane, F8Copy &c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = 4 * wv + i, sp = q >> 4, r = 4 * (q & 15) + (lane >> 4), gi = lane & 15;        // piece q: plane sp, rows 4 (q & 15) ..
        const int col = (8 * gi) ^ bf_swz(r);                                                          // the columns image granule gi of row r holds
        c.v[i] = *reinterpret_cast<const u32x4v *>(pl + sp * F8_PLANE + r * F8_ROW + (col ^ f8_swz(r)));
    }
}
__device__ __forceinline__ void f8_image_store(_Float16 *img, int wv, int lane, const F8Copy &c) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int q = 4 * wv + i;
        __builtin_nontemporal_store(c.v[i], reinterpret_cast<u32x4v *>(img + (unsigned)(512 * q + 8 * lane)));
    }
}
// Work of ANOTHER tile that rides in a layer's MFMA gaps (level_fwd9_body): pre(pr, ks) runs in front of a k-step's fragment requests
// (its own LDS reads are then OLDER than those, and waiting for them leaves the fragments in flight), gap(pr, gap) behind the MFMA
// that opens gap `gap` of pair `pr`.
struct F8NoExtra {
    __device__ __forceinline__ void pre(int, int) {}
    __device__ __forceinline__ void gap(int, int) {}
};
#ifndef F8_EPI_GAP0
#define F8_EPI_GAP0 2                     /* the first gaps of the second pair stay empty: the first pair's last MFMAs are still in the pipe */
#endif
template <bool MASKED, bool ROWS, class X>
__device__ __forceinline__ void f8_layer(const h16x8 (&w)[2][4], const float (&bias)[4], const _Float16 *pl_in, _Float16 *pl_out,
                                         float *rows, const _Float16 *img_src, _Float16 *img_dst, int wv, int l15, int lk, X &x) {
    constexpr int NSTEP = F8EpiSteps<MASKED, ROWS>::N, NGAP = 24 - F8_EPI_GAP0;
    const f32x4v bv = {bias[0], bias[1], bias[2], bias[3]};
    f32x4v am[4];
    h16x8 Bf[3][2][2];                                               // ring over the steps s = 4 pair + ks: [slot][group of the pair][hi, lo]
    const _Float16 *rp0 = pl_in + l15 * F8_ROW + ((8 * lk) ^ f8_swz(l15));
    auto fetch = [&](int s) {
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const _Float16 *rp = rp0 + 16 * (2 * (s >> 2) + u) * F8_ROW + 32 * (s & 3);
            Bf[s % 3][u][0] = *reinterpret_cast<const h16x8 *>(rp);
            Bf[s % 3][u][1] = *reinterpret_cast<const h16x8 *>(rp + F8_PLANE);
        }
    };
    // img_dst: the plane set img_src (the layer's INPUT planes: h1 under layer 2; the previous tile's h2 planes under layer 1 of the
    // pipelined forward) also leaves for HBM as a tile's plane image -- its reads first, the stores behind the first fragment requests
    // (the layer's own MFMAs wait for those anyway)
    F8Copy cp;
    if (img_dst) f8_image_read(img_src, wv, 16 * lk + l15, cp);
    fetch(0); fetch(1);
    if (img_dst) f8_image_store(img_dst, wv, 16 * lk + l15, cp);
    F8Pair st;
#pragma unroll
    for (int pr = 0; pr < 2; ++pr) {
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int s = 4 * pr + ks;
            x.pre(pr, ks);
            if (s + 2 < 8) fetch(s + 2);
#pragma unroll
            for (int pd = 0; pd < 3; ++pd) {                         // lo.hi, hi.lo, hi.hi
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int g = 2 * pr + u, gap = 6 * ks + 2 * pd + u;       // gap: the one BEHIND this MFMA (0..23 within the pair)
                    const f32x4v c0 = (ks == 0 && pd == 0) ? bv : am[g];
                    __builtin_amdgcn_sched_barrier(0);
                    am[g] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w[pd == 0 ? 1 : 0][ks], Bf[s % 3][u][pd == 1 ? 1 : 0], c0, 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);
                    x.gap(pr, gap);
                    __builtin_amdgcn_sched_barrier(0);
                    if (pr == 1 && gap >= F8_EPI_GAP0) {
                        const int i = gap - F8_EPI_GAP0;
#pragma unroll
                        for (int k = i * NSTEP / NGAP; k < (i + 1) * NSTEP / NGAP; ++k)
                            f8_epi_step<MASKED, ROWS>(st, am[0], am[1], k, 0, pl_out, rows, wv, l15, lk);
                    }
                }
            }
        }
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int k = 0; k < NSTEP; ++k) f8_epi_step<MASKED, ROWS>(st, am[2], am[3], k, 2, pl_out, rows, wv, l15, lk);
}

// Heads of points 16 w .. 16 w + 15 (waves 0..3): D[point][head row] = 2^12 (bh + Wh h2), one accumulator as in the layers; the scaled
// head outputs go to hout (row = point of the tile, hstride floats apart).
__device__ __forceinline__ void f8_heads(const HeadCfg &hc, const _Float16 *pl, const _Float16 *whs, const float *bhs, float *hout, int hstride,
                                         int wv, int l15, int lk) {
    const _Float16 *pl0 = pl;
    {
        f32x4v hm;                                                  // 2^12 (bh + Wh h2): one accumulator, as in the layers
        const float bj = bhs[l15];
#pragma unroll
        for (int r = 0; r < 4; ++r) hm[r] = bj;
        const _Float16 *ap = pl0 + (16 * wv + l15) * F8_ROW + ((8 * lk) ^ f8_swz(l15)), *bp = whs + l15 * F8_ROW + ((8 * lk) ^ f8_swz(l15));
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            h16x8 A[2], B[2];
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                A[s2] = *reinterpret_cast<const h16x8 *>(ap + s2 * F8_PLANE + 32 * ks);
                B[s2] = *reinterpret_cast<const h16x8 *>(bp + s2 * 16 * F8_ROW + 32 * ks);
            }
            hm = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[1], B[0], hm, 0, 0, 0);
            hm = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[0], B[1], hm, 0, 0, 0);
            hm = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[0], B[0], hm, 0, 0, 0);
        }
        // D layout: lane holds head row (column) l15 of points 4 lk + r
        float *hr = hout + (size_t)(16 * wv + 4 * lk) * hstride + l15;
#pragma unroll
        for (int r = 0; r < 4; ++r) hr[r * hstride] = hc.mlp_scale * (hm[r] * (1.0f / (BF_WS * BF_HS)));
    }
}

// One 64-point tile: packed encodings (LDS) -> [h0,] h1, h2 (HBM) and the scaled head outputs (saved record in HBM).  Three
// barriers.  The heads (waves 0..3: h2 planes x head-weight planes, 12 MFMAs per wave) run past the end of the tile, next to the
// other waves' layer 0 of the next one.  keep_h0: also store h0 as fp32 rows (a backward on the fp32 MFMA reads it; bwd1_8 recomputes
// it).  h1_image: the reader is the FUSED backward -- h1 goes to HBM as a plane image (f8_epilogue_slice) in place of its fp32 rows.
// hout / hstride: where the tile's scaled head outputs go (row = point of the tile): the saved record in HBM for the engine, an LDS
// table for the multi-level final warp.
__device__ __forceinline__ void fwd8_tile(const HeadCfg &hc, const Fwd8Weights &fw, const TileIO &io, int base, unsigned char *smb,
                                          const _Float16 *l0rows, bool keep_h0, int flip, float *hout, int hstride, bool h1_image = false) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, lk = lane >> 4;
    // The two plane sets swap roles from tile to tile: this tile's heads still read set `pl0` (h2) when the waves that have no
    // heads to do start the next tile's layer 0 -- which therefore writes the OTHER set.
    _Float16 *pl0 = reinterpret_cast<_Float16 *>(smb + (flip ? F8_PL1 : F8_PL0)), *pl1 = reinterpret_cast<_Float16 *>(smb + (flip ? F8_PL0 : F8_PL1));
    const _Float16 *whs = reinterpret_cast<const _Float16 *>(smb + F8_WH);
    const float *bhs = reinterpret_cast<const float *>(smb + F8_BH);
    float *a0 = io.act && keep_h0 ? io.act + (size_t)base * NDP_W : nullptr;
    float *a1 = io.act ? io.act + ((size_t)io.plane + base) * NDP_W : nullptr;
    float *a2 = io.act ? io.act + (2 * (size_t)io.plane + base) * NDP_W : nullptr;
    PT_DECL;
    // ---- layer 0: two MFMAs per point group (f8_l0_group)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float z4[4];
        f8_l0_group(fw.w0, l0rows, g, l15, lk, z4);
        f8_epilogue_v(z4, g, pl0, a0, wv, l15, lk);
    }
    PT(1);
    lds_barrier();
    PT(2);
    // layer 1: planes 0 -> planes 1 (their hi plane is the backward's ReLU mask when h1 travels as the image)
    F8NoExtra nox;
    if (a1 && !h1_image) f8_layer<true, true>(fw.w1, fw.b1, pl0, pl1, a1, nullptr, nullptr, wv, l15, lk, nox);
    else f8_layer<true, false>(fw.w1, fw.b1, pl0, pl1, nullptr, nullptr, nullptr, wv, l15, lk, nox);       // (an image leaves from the planes, under layer 2)
    PT(4);
    lds_barrier();
    PT(5);
    _Float16 *h1img = (h1_image && a1) ? reinterpret_cast<_Float16 *>(a1) : nullptr;
    const bool h2_image = h1_image && a2;                           // the fused backward reads h2 as a plane image too (round 6): no fp32 rows
    if (h2_image) f8_layer<true, false>(fw.w2, fw.b2, pl1, pl0, nullptr, pl1, h1img, wv, l15, lk, nox);   // (MASKED: its hi plane is dz2's ReLU mask)
    else if (a2) f8_layer<false, true>(fw.w2, fw.b2, pl1, pl0, a2, pl1, h1img, wv, l15, lk, nox);      // layer 2: planes 1 -> planes 0 (layer 1 is two barriers behind)
    else f8_layer<false, false>(fw.w2, fw.b2, pl1, pl0, nullptr, nullptr, nullptr, wv, l15, lk, nox);
    PT(7);
    lds_barrier();
    PT(8);
    // ---- no barrier below (see the role swap above)
    if (h2_image) {                                                 // h2's planes -> its image while they are stable (the next tile's layer 1 overwrites them:
        F8Copy cp;                                                  //   one barrier away, like the heads' reads)
        f8_image_read(pl0, wv, lane, cp);
        f8_image_store(reinterpret_cast<_Float16 *>(a2), wv, lane, cp);
    }
    if (wv < 4) f8_heads(hc, pl0, whs, bhs, hout, hstride, wv, l15, lk);
    PT(9);
}

// The positional encodings of a CHUNK of the workgroup's tiles (F8_PE_TILES of them) are computed by all 512 threads at once, before
// the chunk's tiles: six independent sincosf per thread, their inputs requested together.  (Until round 3 three waves encoded tile
// i + 1 during layer 1 of tile i: with the MFMA count of a layer halved by the fp16 splits those waves -- a load behind the tile's
// queued stores, then a transcendental chain -- were 4k cycles late at every layer-1 barrier, a third of the tile's time.)
__device__ __forceinline__ void level_fwd8_body(const HeadCfg &hc, const LevelJob &job, unsigned char *smb, bool keep_h0, bool h1_image = false) {
    const int t = threadIdx.x;
    Fwd8Weights fw;
    PT_DECL;
    fwd8_load_weights(hc, job.params, smb, fw);
    PT(0);
    TileIO io;
    io.x_in = job.x_in; io.shift_in = nullptr; io.x_out = job.x_out; io.shift_out = nullptr;
    io.act = job.act; io.heads = job.heads; io.nonrig = job.nonrig; io.n = job.n; io.plane = job.plane;
    _Float16 *l0rows = reinterpret_cast<_Float16 *>(smb + F8_PE);
    if (job.tile0 >= job.n_tiles) return;
    f8_l0_init_rows(l0rows, F8_PE_TILES * 64, t, 512);
    const int n_mine = (job.n_tiles - job.tile0 + job.tile_step - 1) / job.tile_step;       // tiles of this workgroup
    int flip = 0;
    constexpr int PER = (F8_PE_TILES * 192 + 511) / 512;            // (tile, point, axis) items per thread
    float xa[PER];                                                  // the coordinates of the NEXT chunk's items: requested a chunk of tiles ahead
    auto request_x = [&](int c0) {
        const int nc = min(F8_PE_TILES, n_mine - c0);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int it = t + 512 * i, k = it / 192, r = it - 192 * k;
            xa[i] = k < nc ? fwd_fetch_x(io, (job.tile0 + (c0 + k) * job.tile_step) * NDP_TILE, r / 3, r % 3) : 0.f;
        }
    };
    request_x(0);
    for (int c0 = 0; c0 < n_mine; c0 += F8_PE_TILES) {
        const int nc = min(F8_PE_TILES, n_mine - c0);
        lds_barrier();                                              // the previous chunk's encodings are consumed (and Wh / bh staged)
        {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int it = t + 512 * i, k = it / 192, r = it - 192 * k, pt = r / 3, axis = r - 3 * pt;
                if (k < nc) {
                    float sn, cs;
                    sincosf(xa[i] * job.freq, &sn, &cs);
                    float *hr = io.heads + (size_t)((job.tile0 + (c0 + k) * job.tile_step) * NDP_TILE + pt) * NDP_HROW + 16 + 2 * axis;
                    hr[0] = sn; hr[1] = cs;
                    _Float16 *row = l0rows + (k * 64 + pt) * F8_L0ROW;
                    f8_l0_pack(sn, 2 * axis, row);
                    f8_l0_pack(cs, 2 * axis + 1, row);
                }
            }
        }
        if (c0 + F8_PE_TILES < n_mine) request_x(c0 + F8_PE_TILES);     // (in flight under this chunk's tiles: the load was a round trip in the open per chunk)
        lds_barrier();
        PT(3);
        for (int k = 0; k < nc; ++k) {
            const int tile = job.tile0 + (c0 + k) * job.tile_step;
            fwd8_tile(hc, fw, io, tile * NDP_TILE, smb, l0rows + k * 64 * F8_L0ROW, keep_h0, flip,
                      io.heads + (size_t)tile * NDP_TILE * NDP_HROW, NDP_HROW, h1_image);
            flip ^= 1;
        }
        PT(6);
    }
}

// ------------------------------------------------------------------------------------------------
// The ENGINE's forward as a pipeline over the workgroup's tiles (round 5; the fused-backward configuration: h1 leaves as the plane
// image, h0 is not stored).  The knob builds of the reordered layers (profiles/r05_fwd_knobs.txt) show a tile made of 40 % FIXED
// phases between the two layers -- layer 0 (1.1k cycles: four dependent read - MFMA - epilogue chains per wave), the heads (0.8k,
// four waves), their barriers -- in which the matrix pipe, the LDS and the store path idle.  Here those phases ride in the MFMA gaps
// of the layers, which the first point pair of a layer leaves empty (f8_layer):
//   phase 1 of tile i:  layer 1 (planes A -> B)  +  the HEADS of tile i - 1 (planes C; waves 0..3)
//   phase 2 of tile i:  layer 2 (planes B -> C), B leaving as the h1 image  +  LAYER 0 of tile i + 1 (-> planes A)
// THREE plane sets with fixed roles (A = 2^6 h0, B = 2^6 h1, C = 2^6 h2) instead of two that swap, TWO barriers per tile instead of
// three.  Only a chunk's first tile (its encodings are computed at the chunk boundary) takes layer 0 in a phase of its own, and the
// workgroup's last tile its heads.  Arithmetic, per element and per accumulator, is fwd8_tile's: same bits.
// ------------------------------------------------------------------------------------------------
// layer 0 of the NEXT tile in the gaps of layer 2's first pair: group g reads its packed rows in front of k-step g, its MFMA sits in
// gap 6 g + 1, its epilogue (12 vector instructions and two LDS stores) in gaps 6 g + 4 .. 6 g + 9 (counted through into the second pair)
struct F9Layer0 {
    const L0Ops &w0; const _Float16 *rows; _Float16 *pl; int wv, l15, lk;
    h16x8 b; f32x4v z[2]; float y[4]; unsigned hi[2], lo[2];
    __device__ __forceinline__ F9Layer0(const L0Ops &w0_, const _Float16 *rows_, _Float16 *pl_, int wv_, int l15_, int lk_)
        : w0(w0_), rows(rows_), pl(pl_), wv(wv_), l15(l15_), lk(lk_) {}
    __device__ __forceinline__ void pre(int pr, int ks) {
        if (pr == 0) b = *reinterpret_cast<const h16x8 *>(rows + (16 * ks + l15) * F8_L0ROW + 8 * lk);
    }
    __device__ __forceinline__ void step(int g, int k) {             // step k (0..12) of group g's epilogue
        const f32x4v &zz = z[g & 1];
        if (k < 4) y[k] = bf_act(zz[k]);
        else if (k < 8) { const int q = (k - 4) >> 1; if (k & 1) bf_mix_hi<false, true>(hi[q], y[2 * q + 1], 1.0f); else bf_mix_hi<false, false>(hi[q], y[2 * q], 1.0f); }
        else if (k < 12) { const int q = (k - 8) >> 1; if (k & 1) bf_mix_lo<false, true>(lo[q], y[2 * q + 1], 1.0f, hi[q]); else bf_mix_lo<false, false>(lo[q], y[2 * q], 1.0f, hi[q]); }
        else {
            _Float16 *dst = pl + (16 * g + l15) * F8_ROW + ((16 * wv + 4 * lk) ^ f8_swz(l15));
            const u32x2v P0 = {hi[0], hi[1]}, P1 = {lo[0], lo[1]};
            *reinterpret_cast<u32x2v *>(dst) = P0;
            *reinterpret_cast<u32x2v *>(dst + F8_PLANE) = P1;
        }
    }
    __device__ __forceinline__ void gap(int pr, int gp) {
        const int i = 24 * pr + gp;                                  // gaps counted through both pairs
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            if (i == 6 * g + 1) {
                const f32x4v zero = {0.f, 0.f, 0.f, 0.f};
                z[g & 1] = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0.a, b, zero, 0, 0, 0);
            }
            const int e = i - (6 * g + 4);                           // 13 steps over 6 gaps
            if (e >= 0 && e < 6)
#pragma unroll
                for (int k = e * 13 / 6; k < (e + 1) * 13 / 6; ++k) step(g, k);
        }
    }
};
// the heads of the PREVIOUS tile in the gaps of layer 1's first pair (waves 0..3): k-step ks reads its four fragments in front of the
// layer's k-step ks, its three products sit in gaps 6 ks + 3 .. 6 ks + 5 (one accumulator, the order of f8_heads: same bits); the
// scaled outputs leave in the first gap of the second pair
struct F9Heads {
    const HeadCfg &hc; const _Float16 *ap, *bp; float *hr; int hstride;
    f32x4v hm; h16x8 A[2], B[2];
    __device__ __forceinline__ F9Heads(const HeadCfg &hc_, const _Float16 *pl, const _Float16 *whs, const float *bhs, float *hout, int hstride_,
                                       int wv, int l15, int lk) : hc(hc_), hstride(hstride_) {
        ap = pl + (16 * wv + l15) * F8_ROW + ((8 * lk) ^ f8_swz(l15));
        bp = whs + l15 * F8_ROW + ((8 * lk) ^ f8_swz(l15));
        hr = hout + (size_t)(16 * wv + 4 * lk) * hstride_ + l15;
        const float bj = bhs[l15];
#pragma unroll
        for (int r = 0; r < 4; ++r) hm[r] = bj;
    }
    __device__ __forceinline__ void pre(int pr, int ks) {
        if (pr != 0) return;
#pragma unroll
        for (int s2 = 0; s2 < 2; ++s2) {
            A[s2] = *reinterpret_cast<const h16x8 *>(ap + s2 * F8_PLANE + 32 * ks);
            B[s2] = *reinterpret_cast<const h16x8 *>(bp + s2 * 16 * F8_ROW + 32 * ks);
        }
    }
    __device__ __forceinline__ void gap(int pr, int gp) {
        if (pr == 0) {
            const int j = gp % 6;
            if (j == 3) hm = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[1], B[0], hm, 0, 0, 0);
            else if (j == 4) hm = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[0], B[1], hm, 0, 0, 0);
            else if (j == 5) hm = __builtin_amdgcn_mfma_f32_16x16x32_f16(A[0], B[0], hm, 0, 0, 0);
        } else if (gp == 1) {
#pragma unroll
            for (int r = 0; r < 4; ++r) hr[r * hstride] = hc.mlp_scale * (hm[r] * (1.0f / (BF_WS * BF_HS)));
        }
    }
};

__device__ __forceinline__ void level_fwd9_body(const HeadCfg &hc, const LevelJob &job, unsigned char *smb) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l15 = lane & 15, lk = lane >> 4;
    Fwd8Weights fw;
    PT_DECL;
    fwd8_load_weights(hc, job.params, smb, fw);
    PT(0);
    TileIO io;
    io.x_in = job.x_in; io.shift_in = nullptr; io.x_out = job.x_out; io.shift_out = nullptr;
    io.act = job.act; io.heads = job.heads; io.nonrig = job.nonrig; io.n = job.n; io.plane = job.plane;
    _Float16 *l0rows = reinterpret_cast<_Float16 *>(smb + F8_PE);
    _Float16 *plA = reinterpret_cast<_Float16 *>(smb + F8_PL0), *plB = reinterpret_cast<_Float16 *>(smb + F8_PL1), *plC = reinterpret_cast<_Float16 *>(smb + F8_PL2);
    const _Float16 *whs = reinterpret_cast<const _Float16 *>(smb + F8_WH);
    const float *bhs = reinterpret_cast<const float *>(smb + F8_BH);
    if (job.tile0 >= job.n_tiles) return;
    f8_l0_init_rows(l0rows, F8_PE_TILES * 64, t, 512);
    const int n_mine = (job.n_tiles - job.tile0 + job.tile_step - 1) / job.tile_step;       // tiles of this workgroup
    constexpr int PER = (F8_PE_TILES * 192 + 511) / 512;            // (tile, point, axis) items per thread
    float xa[PER];                                                  // the coordinates of the NEXT chunk's items: requested a chunk of tiles ahead
    auto request_x = [&](int c0) {
        const int nc = min(F8_PE_TILES, n_mine - c0);
#pragma unroll
        for (int i = 0; i < PER; ++i) {
            const int it = t + 512 * i, k = it / 192, r = it - 192 * k;
            xa[i] = k < nc ? fwd_fetch_x(io, (job.tile0 + (c0 + k) * job.tile_step) * NDP_TILE, r / 3, r % 3) : 0.f;
        }
    };
    request_x(0);
    int pending = -1;                                               // the tile whose heads are still to do (its h2 planes are in C)
    F8NoExtra nox;
    for (int c0 = 0; c0 < n_mine; c0 += F8_PE_TILES) {
        const int nc = min(F8_PE_TILES, n_mine - c0);
        lds_barrier();                                              // the previous chunk's encodings are consumed (and Wh / bh staged)
        {
#pragma unroll
            for (int i = 0; i < PER; ++i) {
                const int it = t + 512 * i, k = it / 192, r = it - 192 * k, pt = r / 3, axis = r - 3 * pt;
                if (k < nc) {
                    float sn, cs;
                    sincosf(xa[i] * job.freq, &sn, &cs);
                    float *hr = io.heads + (size_t)((job.tile0 + (c0 + k) * job.tile_step) * NDP_TILE + pt) * NDP_HROW + 16 + 2 * axis;
                    hr[0] = sn; hr[1] = cs;
                    _Float16 *row = l0rows + (k * 64 + pt) * F8_L0ROW;
                    f8_l0_pack(sn, 2 * axis, row);
                    f8_l0_pack(cs, 2 * axis + 1, row);
                }
            }
        }
        if (c0 + F8_PE_TILES < n_mine) request_x(c0 + F8_PE_TILES);     // (in flight under this chunk's tiles)
        lds_barrier();
        PT(3);
        // the chunk's first tile: layer 0 in the open (A is free: the last layer 1 is two barriers back)
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            float z4[4];
            f8_l0_group(fw.w0, l0rows, g, l15, lk, z4);
            f8_epilogue_v(z4, g, plA, nullptr, wv, l15, lk);
        }
        PT(1);
        lds_barrier();
        PT(2);
        for (int k = 0; k < nc; ++k) {
            const int tile = job.tile0 + (c0 + k) * job.tile_step, base = tile * NDP_TILE;
            // ---- phase 1: layer 1, A -> B (+ the previous tile's heads, waves 0..3)
            _Float16 *h2img = pending >= 0 ? reinterpret_cast<_Float16 *>(io.act + (2 * (size_t)io.plane + (size_t)pending * NDP_TILE) * NDP_W) : nullptr;
            if (pending >= 0 && wv < 4) {
                F9Heads hx(hc, plC, whs, bhs, io.heads + (size_t)pending * NDP_TILE * NDP_HROW, NDP_HROW, wv, l15, lk);
                f8_layer<true, false>(fw.w1, fw.b1, plA, plB, nullptr, plC, h2img, wv, l15, lk, hx);
            } else {
                f8_layer<true, false>(fw.w1, fw.b1, plA, plB, nullptr, plC, h2img, wv, l15, lk, nox);
            }
            PT(4);
            lds_barrier();
            PT(5);
            // ---- phase 2: layer 2, B -> C, B leaving as the h1 image (+ the next tile's layer 0 -> A)
            // (h2 has no fp32 rows any more: its planes -- MASKED, the hi plane is the backward's ReLU mask of dz2 -- leave as the tile's
            //  plane image under layer 1 of the NEXT tile, next to that tile's heads; the workgroup's last tile after the loop)
            _Float16 *h1img = reinterpret_cast<_Float16 *>(io.act + ((size_t)io.plane + base) * NDP_W);
            if (k + 1 < nc) {
                F9Layer0 lx(fw.w0, l0rows + (k + 1) * 64 * F8_L0ROW, plA, wv, l15, lk);
                f8_layer<true, false>(fw.w2, fw.b2, plB, plC, nullptr, plB, h1img, wv, l15, lk, lx);
            } else {
                f8_layer<true, false>(fw.w2, fw.b2, plB, plC, nullptr, plB, h1img, wv, l15, lk, nox);
            }
            PT(7);
            lds_barrier();
            PT(8);
            pending = tile;
        }
        PT(6);
    }
    if (pending >= 0) {
        F8Copy cp;
        f8_image_read(plC, wv, lane, cp);
        f8_image_store(reinterpret_cast<_Float16 *>(io.act + (2 * (size_t)io.plane + (size_t)pending * NDP_TILE) * NDP_W), wv, lane, cp);
        if (wv < 4) f8_heads(hc, plC, whs, bhs, io.heads + (size_t)pending * NDP_TILE * NDP_HROW, NDP_HROW, wv, l15, lk);
    }
    PT(9);
}

// The per-point warp of the bf16 forward (nets.py:119-135), point p of pair b: head record -> warped point (rows: NDP_NHMAX floats of
// LDS private to the calling thread)
__device__ __forceinline__ void eng_warp_point(const ndp_engine &e, const ndp_pair_state &st, int b, int p, float *o) {
    const HeadCfg hc = make_head_cfg(desc_at_level(e.desc, st.level));
    const float *hr = e.heads + ((size_t)b * e.n_cap + p) * NDP_HROW;
#pragma unroll
    for (int j = 0; j < NDP_NHMAX; j += 4) *reinterpret_cast<float4 *>(o + j) = *reinterpret_cast<const float4 *>(hr + j);
    float *pts = e.pts + (size_t)b * 2 * e.n_cap * 3;
    const float *xin = pts + ((size_t)st.cur * e.n_cap + p) * 3;
    const float x[3] = {xin[0], xin[1], xin[2]};
    PointHead c;
    float out[3];
    head_warp_fwd(hc, o, x, c, out);
    float *xo = pts + ((size_t)(st.cur ^ 1) * e.n_cap + p) * 3;
    xo[0] = out[0]; xo[1] = out[1]; xo[2] = out[2];
}

// the forward stage of one workgroup (blockIdx.x: first tile / tile step gridDim.x; blockIdx.y: pair)
__device__ __forceinline__ void eng_fwd8_stage(const ndp_engine &e, int parity, unsigned char *smb) {
    const int b = blockIdx.y;
    // state (level, buffer parity) and geometry in ONE test: a load is sunk below every branch that does not need it, which made them
    // three dependent scalar round trips in front of the weight requests (cur is 0 or 1)
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    struct { int level, cur; } st;
    st.level = stp->level; st.cur = stp->cur;
    const ndp_pair_geom gm = e.geom[b];
    LevelJob job;
    job.n = gm.K + gm.S;
    job.n_tiles = (job.n + NDP_TILE - 1) / NDP_TILE;
    if ((st.level >= e.m) | ((int)blockIdx.x >= job.n_tiles) | (st.cur < 0)) return;
    const HeadCfg hc = make_head_cfg(desc_at_level(e.desc, st.level));
    job.params = e.params + ((size_t)b * e.m + st.level) * e.p_stride;
    job.freq = level_freq(st.level, e.k0);
    job.nonrig = nullptr;
    float *pts = e.pts + (size_t)b * 2 * e.n_cap * 3;
    job.x_in = pts + (size_t)st.cur * e.n_cap * 3;
    job.x_out = pts + (size_t)(st.cur ^ 1) * e.n_cap * 3;
    job.act = e.act + (size_t)b * 3 * e.n_cap * NDP_W;
    job.heads = e.heads + (size_t)b * e.n_cap * NDP_HROW;
    job.plane = e.n_cap;
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    // fp32 rows of h0 only for a reader: a backward-1 on the fp32 MFMA (mixed test configurations) or bit 8 of gemm_mode (tests); the
    // split backwards recompute h0 with the forward's own two MFMAs.  The FUSED backward reads h1 as a plane image (in place of the
    // fp32 rows, same footprint); every other backward reads fp32 rows.
    const bool keep_h0 = !(e.gemm_mode & 2) || (e.gemm_mode & 8), h1_image = (e.gemm_mode & 7) == 7 && !(e.gemm_mode & 16);
    if (h1_image && !keep_h0) level_fwd9_body(hc, job, smb);         // the default configuration: the pipelined forward
    else level_fwd8_body(hc, job, smb, keep_h0, h1_image);
}

// The per-point warp rides in the forward launch.  A handful of resident pairs with ONE tile per workgroup: the tile's 64 per-point
// warps run on threads 0..63 of the workgroup that produced their head record (round 4: a launch of its own cost 4.7 us + a boundary
// of a 74 us tick at batch 1).  warp_tail (round 6, second half): the workgroup warps ALL the points of its tiles behind its tile loop,
// 512 threads at a time -- the head records of two sweeps (1024 points) are requested together into per-thread LDS rows (the tile
// regions are dead), then the per-point chains run.  The separate warp launch it replaced (kept as gemm_mode bit 512 until ABI
// 204) took 10.8 us + a kernel boundary of a 0.63 ms tick at 256 pairs and re-read 62 MB from HBM: here the records come back
// from this CU's own stores (profiles/r06_warp_tail_ab.txt).  Same eng_warp_point arithmetic.
__device__ __forceinline__ void eng_warp_tail(const ndp_engine &e, int parity, unsigned char *smb) {
    __syncthreads();                                                 // the tiles' head records (this workgroup's own stores) are visible
    const int b = blockIdx.y, t = threadIdx.x;
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    ndp_pair_state st;
    st.level = stp->level; st.cur = stp->cur;
    const ndp_pair_geom gm = e.geom[b];
    if ((st.level >= e.m) | (st.cur < 0) | (gm.K + gm.S < 0)) return;
    if (e.gmax && blockIdx.x == 0 && t == 0) e.gmax[b] = 0;          // this tick's max |dO| starts from zero (k_eng_loss raises it)
    const int n = gm.K + gm.S, n_tiles = (n + NDP_TILE - 1) / NDP_TILE;
    const HeadCfg hc = make_head_cfg(desc_at_level(e.desc, st.level));
    float *pts = e.pts + (size_t)b * 2 * e.n_cap * 3;
    float *rows = reinterpret_cast<float *>(smb) + t * NDP_LROW;     // [2 sweeps][512 threads][NDP_LROW]
    for (int k0 = 0; blockIdx.x + k0 * gridDim.x < n_tiles; k0 += 16) {       // sixteen of the workgroup's tiles per batch: two sweeps of eight
        int pp[2];
        float x[2][3];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int tile = blockIdx.x + (k0 + 8 * u + (t >> 6)) * gridDim.x, p = tile * NDP_TILE + (t & 63);
            pp[u] = tile < n_tiles && p < n ? p : -1;
            const int pc = pp[u] >= 0 ? p : 0;                       // (clamped: unconditional requests)
            const float4 *hr = reinterpret_cast<const float4 *>(e.heads + ((size_t)b * e.n_cap + pc) * NDP_HROW);
            const float4 h0 = hr[0], h1 = hr[1], h2 = hr[2], h3 = hr[3];
            const float *xin = pts + ((size_t)st.cur * e.n_cap + pc) * 3;
            x[u][0] = xin[0]; x[u][1] = xin[1]; x[u][2] = xin[2];
            float4 *o = reinterpret_cast<float4 *>(rows + u * 512 * NDP_LROW);
            o[0] = h0; o[1] = h1; o[2] = h2; o[3] = h3;
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            PointHead c;
            float out[3];
            head_warp_fwd(hc, rows + u * 512 * NDP_LROW, x[u], c, out);
            if (pp[u] >= 0) {
                float *xo = pts + ((size_t)(st.cur ^ 1) * e.n_cap + pp[u]) * 3;
                xo[0] = out[0]; xo[1] = out[1]; xo[2] = out[2];
            }
        }
    }
}

extern "C" __global__ void __launch_bounds__(512, 1)
k_eng_fwd8(ndp_engine e, int parity, int warp_tail) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
    PT_INIT;
    eng_fwd8_stage(e, parity, smb);
    if (warp_tail) eng_warp_tail(e, parity, smb);
    else {
        __syncthreads();                                             // the tile's head record (this workgroup's own stores) is visible
        const int b = blockIdx.y, t = threadIdx.x;
        const ndp_pair_state st = e.state[parity * e.B + b];
        if (st.level < e.m) {
            if (e.gmax && blockIdx.x == 0 && t == 0) e.gmax[b] = 0;  // this tick's max |dO| starts from zero (k_eng_loss raises it)
            const ndp_pair_geom gm = e.geom[b];
            const int p = blockIdx.x * NDP_TILE + t;
            if (t < NDP_TILE && p < gm.K + gm.S) eng_warp_point(e, st, b, p, reinterpret_cast<float *>(smb) + t * NDP_NHMAX);
        }
    }
    PT_FLUSH(12);
}

// ------------------------------------------------------------------------------------------------
// Final inference warp on the bf16 matrix pipe (registration.py:253-258 with the engine's split arithmetic): ALL points of a cloud
// through all m levels, the points staying in LDS from level to level (no activation stores at all).  A workgroup of 8 waves
// carries P8_TILES 64-point tiles: per level the two 128 x 128 weight slices are pulled into registers ONCE for the four tiles,
// the positional encoding of all 256 points is computed by all 512 threads at once, the tiles run through the layer / head
// stages of the engine's forward (fwd8_tile: same code, same bits per tile), and the per-point warps of the four tiles -- a chain of
// transcendentals that occupies ONE thread per point -- run together, 256 threads wide, instead of one wave at a time.
// The fp32-MFMA kernel (k_pyramid_fwd) stays for gemm_mode 0 and for the single-operator entry points.
// ------------------------------------------------------------------------------------------------
#define P8_TILES 4                            /* tiles per workgroup of the latency shape (one or two clouds: many workgroups, short ones) */
#define P8_TILES_MAX 8                        /* ... and of the throughput shape (round 6): half the weight prologues per cloud -- a launch of the batched engine's
                                                 finished pairs is one or two clouds wide, what it costs is the CU-time it holds next to the other engines' ticks */
static_assert(P8_TILES_MAX <= F8_PE_TILES, "the level's packed encodings live in the forward's encoding region");
enum : int {
    P8_PE = F8_PE,                              // [tiles][64][F8_L0ROW] fp16: packed encodings of the level (the engine forward's chunk region: unused here otherwise)
    P8_XS = F8_TOTAL,                           // [tiles * 64][4] the points (level input, replaced by the level output)
    P8_HO = P8_XS + P8_TILES_MAX * 64 * 4 * 4,  // [tiles * 64][16] scaled head outputs of the level
    P8_TOTAL = P8_HO + P8_TILES_MAX * 64 * NDP_NHMAX * 4
};
static constexpr int kSmemPyr8Bytes = P8_TOTAL;
static_assert(kSmemPyr8Bytes <= 160 * 1024, "split final-warp LDS carve");

extern "C" __global__ void __launch_bounds__(512, 1)
k_pyramid_fwd8(ndp_layer_desc desc, int m, int k0, int p_stride, WarpJobs jobs, int tiles) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
    const ndp_warp_job jb = jobs.j[blockIdx.y];
    const int base0 = blockIdx.x * NDP_TILE * tiles;
    if (base0 >= jb.n) return;
    const int t = threadIdx.x;
    const int nt = min(tiles, (jb.n - base0 + NDP_TILE - 1) / NDP_TILE), np = nt * NDP_TILE;
    _Float16 *pe = reinterpret_cast<_Float16 *>(smb + P8_PE);
    float *xs = reinterpret_cast<float *>(smb + P8_XS), *ho = reinterpret_cast<float *>(smb + P8_HO);
    f8_l0_init_rows(pe, P8_TILES_MAX * 64, t, 512);
    for (int i = t; i < np * 3; i += 512) {                          // level-0 input: x - shift_in (zero beyond n)
        const int q = i / 3, a = i - 3 * q, p = base0 + q;
        float v = 0.f;
        if (p < jb.n) { v = jb.x[3 * (size_t)p + a]; if (jb.shift_in) v -= jb.shift_in[a]; }
        xs[4 * q + a] = v;
    }
    TileIO io;
    io.x_in = nullptr; io.shift_in = nullptr; io.x_out = nullptr; io.shift_out = nullptr;
    io.act = nullptr; io.heads = nullptr; io.nonrig = nullptr; io.n = jb.n; io.plane = 0;
    __syncthreads();
    for (int l = 0; l < m; ++l) {
        const HeadCfg hc = make_head_cfg(desc_at_level(desc, l));
        Fwd8Weights fw;
        fwd8_load_weights(hc, jb.params + (size_t)l * p_stride, smb, fw);     // (the head planes in LDS are free: see the barrier below)
        const float freq = ldexpf(1.0f, l + 1 + k0);
        for (int i = t; i < np * 3; i += 512) {
            const int q = i / 3, a = i - 3 * q;
            float sn, cs;
            sincosf(xs[4 * q + a] * freq, &sn, &cs);
            f8_l0_pack(sn, 2 * a, pe + q * F8_L0ROW);
            f8_l0_pack(cs, 2 * a + 1, pe + q * F8_L0ROW);
        }
        __syncthreads();
        for (int k = 0; k < nt; ++k)
            fwd8_tile(hc, fw, io, base0 + k * NDP_TILE, smb, pe + k * 64 * F8_L0ROW, false, k & 1, ho + k * NDP_TILE * NDP_NHMAX, NDP_NHMAX);
        __syncthreads();                                             // every tile's head outputs are in LDS
        if (t < np) {
            const int p = base0 + t;
            PointHead c;
            float out[3];
            head_warp_fwd(hc, ho + t * NDP_NHMAX, xs + 4 * t, c, out);
            if (l == m - 1) {
                if (p < jb.n) {
                    if (jb.shift_out) { out[0] += jb.shift_out[0]; out[1] += jb.shift_out[1]; out[2] += jb.shift_out[2]; }
                    jb.x_out[3 * (size_t)p] = out[0]; jb.x_out[3 * (size_t)p + 1] = out[1]; jb.x_out[3 * (size_t)p + 2] = out[2];
                }
            } else {
                xs[4 * t] = out[0]; xs[4 * t + 1] = out[1]; xs[4 * t + 2] = out[2];
            }
        }
        __syncthreads();                                             // the level's output is the next level's input; Wh / bh may be restaged
    }
}
