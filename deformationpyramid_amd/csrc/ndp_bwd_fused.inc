// ------------------------------------------------------------------------------------------------
// FUSED level backward of the split arithmetic (round 4; engine gemm_mode 7 without bit 16): k_eng_bwd2_8 and k_eng_bwd1_8 in ONE
// launch per tick, a tile's dz1 never leaving the CU.
//   Per 64-point tile:  dz2 = (dO Wh) [h2 > 0];  dWh, dbh;  dW2 += dz2^T h1, db2;  dz1 = (dz2 W2) [h1 > 0]  -> fp16 planes in LDS;
//                       dW1 += dz1^T h0, db1;  dz0 = (dz1 W1) [h0 > 0];  [dW0 | db0] += dz0^T [pe | 1].
//   h2 is read from HBM as the forward's fp32 rows, h1 as the forward's PLANE IMAGE (2^6 h1 already split into this kernel's swizzled
//   fp16 planes: ndp_fwd_split.inc, f8_epilogue_slice), h0 is recomputed from the saved encoding with the forward's own layer-0 MFMA
//   per point group (f8_l0_group: bitwise the forward's h0).  Against the two round-3 kernels: one launch and one weight / partial
//   prologue less, and 2 x 152 MB per 128-pair tick that never cross HBM (dz1 written by bwd2, read back by bwd1).
//   ARITHMETIC: two-way fp16 splits as everywhere on the split path, but with ONE accumulator per product: every tensor is multiplied
//   by a power of two before its split (activations and weights by 2^6, gradients by S = 2^k per pair and tick with
//   S max|dO| in [2^8, 2^9)), hi = fp16(x'), lo = fp16(x' - hi) -- UNSCALED, so that hi.hi + hi.lo + lo.hi add up in the same fp32
//   accumulator; the pre-scale keeps lo's absolute floor (half an fp16 subnormal step, 2^-25) at 2^-31 of an O(1) activation or
//   weight and 2^-33 of the pair's largest gradient.  |x' - hi - lo| <= max(2^-22 |x'|, 2^-25): the accuracy class of the
//   two-accumulator form of round 3 (x = hi + 2^-11 lo, lo scaled by 2^11: the two-launch backward of bit 16), measured against
//   float64 by the same test (tests/test_split_accuracy.py); since the second half of round 4 the forward contracts in this form too.  What it buys here: the weight-gradient accumulators of BOTH layers are 64 registers instead of
//   128, which is what lets one kernel hold W1^T, W2^T, dW1 and dW2.  Range: a scaled operand saturates at +-65504, i.e. an
//   activation or weight beyond 1023 (the two-accumulator kernels: 65504) and a gradient 128 times the pair's largest |dO|.
//   LDS: four 32 KB regions.  A plane set is [hi, lo][64][128] fp16 with UNPADDED 256-byte rows and a 16-byte-granule XOR swizzle
//   (bf_swz) under which both access patterns are conflict-free: the 16-byte fragment reads (sixteen rows of one granule column per
//   lane group: the sixteen swizzle values of {rows 0-3, 12-15 at granule g} and {rows 4-11 at granule g ^ 1} are all different) and
//   the transposing reads (four consecutive rows x four granules: the four rows land in four different 64-byte bank groups).
//   The rows arrive by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave-instruction, no staging registers).  The NEXT tile's h2 rows
//   (needed as fp32 right after the next top barrier: dWh operand and ReLU mask) are requested at the start of the last stage of a
//   tile, into the region the dz2 planes have just left -- which is where the dz1 planes of that tile then go -- with the dO rows and
//   the encodings; the next tile's h1 plane image is requested at the END of that stage into R2 (the top of the tile waits for
//   everything but those four requests -- vmcnt(4): the counter retires in order -- the barrier in front of stage 3 for them).  So
//   the 32 KB that must land within one stage travel alone (with h1's 32 KB requested beside them the top-of-tile wait was ~1 us per
//   tile: -4 % at 256 pairs, -7 % at 128 without it).  Regions: R0 h0 planes, R2 h1 planes, and R1 / R3 alternating between
//   {h2 rows -> dz1 planes} and {dz2 planes} from tile to tile.  (Until the second half of round 4 h1 travelled as fp32 rows in
//   sixteen registers and was split first thing of a tile.)  Three barriers per tile.
//   COST MODEL (round 4, corrected in round 5): a vector instruction BEHIND a block of back-to-back (dependent) MFMAs is paid in
//   full -- the wave issues in order -- which is how the contraction loops here are written (three products per step on one
//   accumulator, the epilogue after them), and why [dW0 | db0] runs on the MFMA, masks are compared on the fp16 hi parts and value
//   operands are split without the mask floor.  Placed BETWEEN independent MFMAs two vector instructions per 16x16x32 gap are free
//   (tools/experiments/micro/coexec2.hip, profiles/r05_micro_coexec2.txt; round 4's coexec.hip could not see that behind its
//   dependent triplets): the forward is ordered that way since round 5 (f8_layer), and it bought 5 % -- that kernel is bound by its
//   store stream and its LDS traffic (profiles/r05_fwd_knobs.txt), as is this one by its loads.
// ------------------------------------------------------------------------------------------------
// (BF_ROW, BF_PLANE, BF_HS, BF_WS, bf_swz, bf_split: the plane-image format, defined in ndp_fwd_split.inc -- the forward writes h1 in it)
#define BF_PEROW 72                                 /* fp16 per row of the transposed encoding planes: 64 contraction slots + padding */
#define BF_DOROWS NDP_WHROWS                        /* head rows of the transposed dO planes (lanes beyond them read the last row: their products are not stored) */
// [dW0 | db0] = dz0^T [pe | 1] on the MFMA: the contraction runs over the tile's points in the order the swapped data gradient leaves
// them in a lane -- slot 8 lk + 4 (g & 1) + r of k-step g >> 1 <-> point 16 g + 4 lk + r.  This is that slot for point p.
__device__ __forceinline__ int bf_pe_slot(int p) { return ((p >> 5) << 5) | (((p >> 2) & 3) << 3) | (((p >> 4) & 1) << 2) | (p & 3); }
#define BF_REGION (2 * BF_PLANE * 2)                /* 32 768 B: one plane set, or one [64][128] fp32 tile */
enum : int {                                      // byte offsets of the dynamic LDS region
    BF_R0 = 0,                                    // four regions that rotate (see the header)
    BF_DO = 4 * BF_REGION,                        // [64][16] fp32 dO rows (LDS-DMA; last read in stage 2, the next tile's arrive from stage 4 on)
    BF_GBH = BF_DO + 64 * 16 * 4,                 // [256] float4: dbh partials (thread t < 256 adds its piece of every tile's dO rows)
    BF_PES = BF_GBH + 256 * 16,                   // [2][8][BF_PEROW] fp16: the encodings TRANSPOSED, hi | lo planes -- B operand of [dW0 | db0] (bf_pe_slot);
                                                  //   rows 0..5 the encodings, 6 the ones (hi plane), 7 zero -- which columns 7..15 of the product read
    BF_DOP = BF_PES + 2 * 8 * BF_PEROW * 2,       // [2][BF_DOROWS][BF_PEROW] fp16: S dO TRANSPOSED, hi | lo planes -- A operand of dWh, split ONCE per tile
                                                  //   (until round 6 every wave split the same sixteen values per lane: eight times the work)
    BF_PEQ = BF_DOP + 2 * BF_DOROWS * BF_PEROW * 2, // [64][6] fp32: the encoding values as they arrive (LDS-DMA, one dword per lane; read in stage 1 only)
    BF_L0 = BF_PEQ + 64 * 6 * 4,                  // [64][F8_L0ROW] fp16 packed layer-0 operand rows
    BF_WH = BF_L0 + 64 * F8_L0ROW * 2,            // [12][128] fp32 head matrix
    BF_GWH = BF_WH + NDP_WHROWS * NDP_W * 4,      // [8][48] float4: the dWh accumulators of the lanes that hold head rows 0..11 (lk < 3) -- touched once per tile,
                                                  //   they were what the register allocator sent to scratch inside the tile loop (a scratch reload waits for vmcnt(0))
    BF_TOTAL = BF_GWH + 8 * 48 * 16
};
static_assert(64 * NDP_W * 4 == BF_REGION, "an fp32 tile fills a region");
static constexpr int kSmemBwdFBytes = BF_TOTAL;
static_assert(kSmemBwdFBytes <= 160 * 1024, "fused backward LDS carve");

// The tile loop runs with MODE.FP16_OVFL = 1 -- a conversion to fp16 that overflows gives +-65504 instead of inf -- so the gradient
// splits of the tile loop drop their v_med3 bound (one vector instruction per element; the bits differ only where a scaled gradient
// exceeds 65504, i.e. 128 times its pair's largest |dO|: hi = 65504 either way, lo = the bounded remainder instead of 0).  Measured
// against the bounded split in round 6 (a compile-time knob, since retired): -2 % at 256 pairs, bitwise in range (profiles/r06_bwd_ovfl_ab.txt).
__device__ __forceinline__ void bf_split_g(float x, _Float16 &hi, _Float16 &lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}
// four float4 of a [64][128] fp32 tile per thread (rows (t >> 5) + 16 i, columns 4 (t & 31) ..), times `scale` -> the two planes
template <bool ACT>
__device__ __forceinline__ void bf_split_rows(const float4 (&v)[4], _Float16 *pl, int t, float scale) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int row = (t >> 5) + 16 * i, c = (4 * (t & 31)) ^ bf_swz(row);
        const float f[4] = {v[i].x, v[i].y, v[i].z, v[i].w};
        h16x4 p0, p1;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            _Float16 a, l;
            if (ACT) bf_split<true>(f[e] * scale, a, l); else bf_split_g(f[e] * scale, a, l);
            p0[e] = a; p1[e] = l;
        }
        *reinterpret_cast<h16x4 *>(pl + row * BF_ROW + c) = p0;
        *reinterpret_cast<h16x4 *>(pl + BF_PLANE + row * BF_ROW + c) = p1;
    }
}
// four scaled values of point p, features c .. c + 3 (a lane of the 16x16 accumulator layout) -> the two planes
template <bool ACT>
__device__ __forceinline__ void bf_split4(const float (&v)[4], _Float16 *pl, int p, int c) {
    h16x4 p0, p1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 a, l;
        bf_split<ACT>(v[e], a, l);
        p0[e] = a; p1[e] = l;
    }
    _Float16 *dst = pl + p * BF_ROW + (c ^ bf_swz(p));
    *reinterpret_cast<h16x4 *>(dst) = p0;
    *reinterpret_cast<h16x4 *>(dst + BF_PLANE) = p1;
}

// the same for values that are already bounded (and floored): 2^6 h of bf_act
__device__ __forceinline__ void bf_store4(const float (&v)[4], _Float16 *pl, int p, int c) {
    h16x4 p0, p1;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        _Float16 a, l;
        bf_split_act(v[e], a, l);
        p0[e] = a; p1[e] = l;
    }
    _Float16 *dst = pl + p * BF_ROW + (c ^ bf_swz(p));
    *reinterpret_cast<h16x4 *>(dst) = p0;
    *reinterpret_cast<h16x4 *>(dst + BF_PLANE) = p1;
}

// Per-lane LDS offsets (fp16 elements, relative to a plane set) of the two access patterns.  The swizzle of a lane's rows does not
// depend on the k-step or the point group -- rows move by multiples of 16 -- so every access below is one of these bases plus an
// immediate (written out here: left to the compiler, each of the ~100 swizzled addresses of a tile became a register of its own).
struct BfOffs {
    int tr[3][2];          // transposing reads: [A (f0 = 32 ob) | B (32 kb) | B (32 kb + 32)][rows r0, r0 + 4] at k-step 0
    int fr[4];             // 16-byte fragment reads of row l15: k-step 0..3 at point group 0
    int trh[2];            // transposing reads of a 16x16x32 B operand (dWh): feature 16 wv + l15 of points 8 lk .. + 3 / + 4 .. + 7 of a 32-point k-step
};
__device__ __forceinline__ BfOffs bf_offsets(int lane, int ob, int kb, int wv) {
    BfOffs o;
    const int lam = lane & 15, g = (lane >> 4) & 1, x = 8 * (lane >> 5) + (lam >> 2);      // row within a k-step's 16 points: x, x + 4
    const int f0[3] = {32 * ob, 32 * kb, 32 * kb + 32};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        const int c = f0[q] + 16 * g + 4 * (lam & 3);
        o.tr[q][0] = x * BF_ROW + (c ^ bf_swz(x));
        o.tr[q][1] = (x + 4) * BF_ROW + (c ^ bf_swz(x + 4));
    }
    const int l15 = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) o.fr[ks] = l15 * BF_ROW + ((32 * ks + 8 * lk) ^ bf_swz(l15));
    const int xh = 8 * lk + (l15 >> 2), ch = 16 * wv + 4 * (l15 & 3);
    o.trh[0] = xh * BF_ROW + (ch ^ bf_swz(xh));
    o.trh[1] = (xh + 4) * BF_ROW + (ch ^ bf_swz(xh + 4));
    return o;
}
// A region's base (fp16 elements from the start of the dynamic LDS) plus a lane's offset, made OPAQUE to the optimiser: what follows is
// then base register + immediate (plane, k-step and point-group offsets fit the 16-bit offset field); with the region's constant
// folded in, the sums beyond 64 KB did not, and every access got an address register of its own.
__device__ __forceinline__ int bf_base(int region_bytes, int off) {
    int b = region_bytes / 2 + off;
    asm volatile("" : "+v"(b));
    return b;
}
// eight consecutive points (16 ks + 8 (lane >> 5) ..) of one feature per lane from a swizzled plane (ds_read_b64_tr_b16, see tr_frag)
__device__ __forceinline__ h16x8 bf_tr_frag(const _Float16 *lds, int ks, int s, int base_a, int base_b) {
    const _Float16 *a = lds + base_a + (s * BF_PLANE + 16 * ks * BF_ROW);
    const _Float16 *b = lds + base_b + (s * BF_PLANE + 16 * ks * BF_ROW);
    const s16x4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v *)a);
    const s16x4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4v *)b);
    const s16x8v v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
    return __builtin_bit_cast(h16x8, v);
}

// One LDS-DMA piece (1 KiB: lane l's 16 bytes at gptr -> LDS byte lds_addr + 16 l), issued through inline asm ON PURPOSE: the compiler
// orders every later LDS read it cannot prove disjoint behind a global_load_lds it knows about with s_waitcnt vmcnt(0) -- the regions
// here are run-time offsets -- which made the whole prefetch synchronous.  The kernel waits itself (vmcnt(0) + barrier at the top of a
// tile); the compiler's own vmcnt arithmetic for ITS loads can only over-wait (the counter is in order).
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"          /* m0 on the clobber list is the point: the statement sets it */
__device__ __forceinline__ void bf_dma4(const void *gptr, int lds_addr) {     // 256 B: lane l's 4 bytes at its own gptr -> LDS lds_addr + 4 l
    const int a = __builtin_amdgcn_readfirstlane(lds_addr);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dword %0, off" : : "v"(gptr), "s"(a) : "memory", "m0");
}
// (`nt`: the activation tiles are read ONCE, 0.4 ms after the forward wrote them -- with non-temporal stores, see f8_image_store -- and
//  a tick moves 1 GB of them through caches of 32 + 256 MB: marked streaming they stop evicting what IS re-used from tick to tick --
//  parameters, moments, head records.  One engine's tick at 256 pairs: 0.737 -> 0.705 ms with these, the forward's stores and the
//  gradient partials marked, bitwise the same results; profiles/r05_nt_ab.txt)
__device__ __forceinline__ void bf_dma16(const void *gptr, int lds_addr) {
    const int a = __builtin_amdgcn_readfirstlane(lds_addr);
    asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, off nt" : : "v"(gptr), "s"(a) : "memory", "m0");
}
#pragma clang diagnostic pop

// transposed weight slice, scaled by 2^6, in the one-accumulator split: A rows k = 16 wv + (lane & 15), contraction index o = 32 ks + 8 (lane >> 4) + e
__device__ __forceinline__ void bf_load_wt(const float *W /*[o][k]*/, int wv, int l15, int lk, h16x8 (&w)[2][4]) {
    const float *wc = W + 16 * wv + l15;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            _Float16 a, l;
            bf_split<false>(wc[(32 * ks + 8 * lk + e) * NDP_W] * BF_WS, a, l);
            w[0][ks][e] = a; w[1][ks][e] = l;
        }
}

// dW[2 blocks] += (S dz)^T (2^6 h) over the 64 points of the planes at byte offsets rz / rh of the LDS (wave: o-block ob, k-blocks kb,
// kb + 1), one accumulator per block
__device__ __forceinline__ void bf_wgrad(const _Float16 *lds, int rz, int rh, const BfOffs &o, f32x16 (&acc)[2]) {
    const int za = bf_base(rz, o.tr[0][0]), zb = bf_base(rz, o.tr[0][1]);
    const int h0a = bf_base(rh, o.tr[1][0]), h0b = bf_base(rh, o.tr[1][1]), h1a = bf_base(rh, o.tr[2][0]), h1b = bf_base(rh, o.tr[2][1]);
    // eight steps s = 2 ks + m (k-step, block); the fragments of step s + 1 are requested before the three products of step s issue
    // (left to itself the compiler requests a step's fragments after the previous step's products and waits for them at once:
    // read - wait - three products, the transposing reads' latency in the open once per step)
    h16x8 A[2][2], B[2][2];
    auto fa = [&](int ks) { A[ks & 1][0] = bf_tr_frag(lds, ks, 0, za, zb); A[ks & 1][1] = bf_tr_frag(lds, ks, 1, za, zb); };
    auto fb = [&](int st) {
        const int ks = st >> 1, m = st & 1;
        B[st & 1][0] = bf_tr_frag(lds, ks, 0, m ? h1a : h0a, m ? h1b : h0b);
        B[st & 1][1] = bf_tr_frag(lds, ks, 1, m ? h1a : h0a, m ? h1b : h0b);
    };
    fa(0); fb(0);
#pragma unroll
    for (int st = 0; st < 8; ++st) {
        const int ks = st >> 1, m = st & 1;
        if (st + 1 < 8) { fb(st + 1); if (m == 1) fa(ks + 1); }
        __builtin_amdgcn_sched_barrier(0);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[ks & 1][1], B[st & 1][0], acc[m], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[ks & 1][0], B[st & 1][1], acc[m], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
        acc[m] = __builtin_amdgcn_mfma_f32_32x32x16_f16(A[ks & 1][0], B[st & 1][0], acc[m], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);
    }
}

// The data gradient of a tile's four point groups: d = sum_o (S dz)[16 g + l15][o] (2^6 W)[o][16 wv + 4 lk + r] (scaled by 2^6 S) per
// group; fr[ks]: the lane's fragment bases of the dz planes (bf_base).  SWAP: operands exchanged -- the accumulator then holds feature
// 16 wv + l15 of points 16 g + 4 lk + r.  Software-pipelined: the fragments of step s + 1 (s = 4 g + ks) are requested before the
// products of step s issue.  The epilogue of a group -- mask, split, stores -- comes as TWELVE steps epi(g, d, k), k = 0..11, of two
// or three vector instructions each, which follow the first three products of the next group in a block.
template <bool SWAP, class Epi>
__device__ __forceinline__ void bf_dgrad_tile(const h16x8 (&wt)[2][4], const _Float16 *lds, const int (&fr)[4], Epi epi) {
    h16x8 Bf[2][2];
    auto fetch = [&](int st) {
        const _Float16 *rp = lds + fr[st & 3] + 16 * (st >> 2) * BF_ROW;
        Bf[st & 1][0] = *reinterpret_cast<const h16x8 *>(rp);
        Bf[st & 1][1] = *reinterpret_cast<const h16x8 *>(rp + BF_PLANE);
    };
    fetch(0);
    f32x4v d, dp;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
#pragma unroll
        for (int r = 0; r < 4; ++r) d[r] = 0.f;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            const int st = 4 * g + ks;
            if (st + 1 < 16) fetch(st + 1);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int pd = 0; pd < 3; ++pd) {                         // lo.hi, hi.lo, hi.hi
                const h16x8 &bz = Bf[st & 1][pd == 1 ? 1 : 0], &wz = wt[pd == 0 ? 1 : 0][ks];
                d = SWAP ? __builtin_amdgcn_mfma_f32_16x16x32_f16(bz, wz, d, 0, 0, 0) : __builtin_amdgcn_mfma_f32_16x16x32_f16(wz, bz, d, 0, 0, 0);
            }
            __builtin_amdgcn_sched_barrier(0);
            if (ks == 0 && g > 0) {
#pragma unroll
                for (int k = 0; k < 12; ++k) epi(g - 1, dp, k);
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        dp = d;
    }
#pragma unroll
    for (int k = 0; k < 12; ++k) epi(3, dp, k);
}

__device__ __forceinline__ void bf_store_dW(float *g, const f32x16 (&acc)[2], float inv, int ob, int kb, int l31, int h) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            __builtin_nontemporal_store(acc[m][r] * inv, g + (32 * ob + mfma_row(r, h)) * NDP_W + 32 * (kb + m) + l31);
        }
}

// S = 2^k with S max|dO| in [2^8, 2^9), and 1 / S (both exact; S = 1 when every dO is zero)
__device__ __forceinline__ B8Scale bf_scale(const ndp_engine &e, int b) {
    const unsigned bits = e.gmax[b];
    int ex = (int)((bits >> 23) & 0xffu);                            // biased exponent of max |dO|
    if (bits == 0u) ex = 135;                                        // -> S = 1
    ex = ex < 10 ? 10 : (ex > 250 ? 250 : ex);
    B8Scale r;
    r.s = __uint_as_float((unsigned)(262 - ex) << 23);               // 2^(8 - (ex - 127))
    r.inv = __uint_as_float((unsigned)(ex - 8) << 23);
    return r;
}

// dz2 before its mask: a[i][c] = sum_j Wh[j][4 (t & 31) + c] (S dO)[row (t >> 5) + 16 i][j], the fp32 fma chain from zero, j ascending
// (NH > 0: the head count as a compile-time constant; 0: nh at run time)
template <int NH>
__device__ __forceinline__ void bf_dz2_chain(const float *whs, const float *dr, int t, int nh, float (&a)[4][4]) {
    const int n = NH > 0 ? NH : nh;
#pragma unroll
    for (int jj = 0; jj < n; ++jj) {                                 // head row outermost: one read of its four weights serves the four rows
        if (NH > 0 && jj > 0 && (jj & 1) == 0) __builtin_amdgcn_sched_barrier(0);   // (two head rows' operands in flight, not all six: registers)
        const float4 w4 = *reinterpret_cast<const float4 *>(whs + jj * NDP_W + 4 * (t & 31));
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float dj = dr[16 * i * NDP_NHMAX + jj];
            a[i][0] = fmaf(w4.x, dj, a[i][0]); a[i][1] = fmaf(w4.y, dj, a[i][1]);
            a[i][2] = fmaf(w4.z, dj, a[i][2]); a[i][3] = fmaf(w4.w, dj, a[i][3]);
        }
    }
}

// G == 1 (unless gemm_mode bit 1024; one workgroup holds a pair's whole gradient: the 256-slot engines): the Adam step of the two 128 x 128
// matrices -- 94 % of the parameters -- behind the tile loop, from the gradient as it stands in LDS (row-major: the values the partial
// stores carry), 16-byte accesses, 24 requests in flight per thread.  k_eng_update then steps what is left (biases, W0, heads) and skips
// these two ranges.  Saves the write and the read of 131 KB of gradient partial per pair (the partial's two matrix blocks are NOT written
// in this mode: gemm_mode bit 1024 -- everything in k_eng_update, bitwise the same state -- is what a test that looks at them sets) and
// all but eight of the update stage's 136 workgroups per pair;
// the arithmetic is eng_update_param's (ONE partial: its fold is the identity): same bits.  noinline: the tile loop keeps its registers.
__host__ __device__ inline bool bf_adam_in_tail(const ndp_engine &e) {
    return e.G == 1 && (e.gemm_mode & 7) == 7 && !(e.gemm_mode & (16 | 1024));
}
// (scalars and pointers by value: a reference to the engine record would put the whole kernel argument on the stack)
struct BfAdamK { float w1, b2, w2, eps, ns0, ns1; };
__device__ __attribute__((noinline)) void bf_adam_tail(float *p, float *m, float *v, BfAdamK k, int fresh /* level hand-over behind this step:
                                                       fresh moments (registration.py:176) */,
                                                       const float *gl /* LDS [2][128 * 128]: dW2, dW1 */, int off_W2, int off_W1) {
    const int t = threadIdx.x;
    const float ns0 = k.ns0, ns1 = k.ns1;
#pragma unroll 1
    for (int w = 0; w < 2; ++w) {
        const int off = w == 0 ? off_W2 : off_W1;
        const float4 *g4 = reinterpret_cast<const float4 *>(gl + w * NDP_W * NDP_W);
        float4 *p4 = reinterpret_cast<float4 *>(p + off), *m4 = reinterpret_cast<float4 *>(m + off), *v4 = reinterpret_cast<float4 *>(v + off);
#pragma unroll 1
        for (int i0 = t; i0 < NDP_W * NDP_W / 4; i0 += 2 * 512) {
            float4 P[2], M[2], V[2], Gv[2];
#pragma unroll
            for (int u = 0; u < 2; ++u) { P[u] = p4[i0 + 512 * u]; M[u] = m4[i0 + 512 * u]; V[u] = v4[i0 + 512 * u]; Gv[u] = g4[i0 + 512 * u]; }
#pragma unroll
            for (int u = 0; u < 2; ++u) {
                adam_update(P[u].x, Gv[u].x, M[u].x, V[u].x, k.w1, k.b2, k.w2, ns0, ns1, k.eps);
                adam_update(P[u].y, Gv[u].y, M[u].y, V[u].y, k.w1, k.b2, k.w2, ns0, ns1, k.eps);
                adam_update(P[u].z, Gv[u].z, M[u].z, V[u].z, k.w1, k.b2, k.w2, ns0, ns1, k.eps);
                adam_update(P[u].w, Gv[u].w, M[u].w, V[u].w, k.w1, k.b2, k.w2, ns0, ns1, k.eps);
                if (fresh) { M[u] = make_float4(0.f, 0.f, 0.f, 0.f); V[u] = make_float4(0.f, 0.f, 0.f, 0.f); }
                p4[i0 + 512 * u] = P[u]; m4[i0 + 512 * u] = M[u]; v4[i0 + 512 * u] = V[u];
            }
        }
    }
}

// the backward stage of one workgroup (blockIdx.x: first tile / tile step gridDim.x; blockIdx.y: pair)
__device__ __forceinline__ void eng_bwd_f_stage(const ndp_engine &e, int parity, unsigned char *smb) {
    const ndp_layer_desc dd = {NDP_W, 2, 0, 0, 0, 0.f};
    const int off_W0 = ndp_off_W0(&dd), off_b0 = ndp_off_b0(&dd), off_W1 = ndp_off_Wi(&dd, 1), off_b1 = ndp_off_bi(&dd, 1);
    const int off_W2 = ndp_off_Wi(&dd, 2), off_b2 = ndp_off_bi(&dd, 2), off_Wh = ndp_off_Wi(&dd, 3);
    Bwd8Setup j;
    if (!eng_bwd8_setup(e, parity, 0, e.P, j)) {
        if (bf_adam_in_tail(e) && e.state[(size_t)(parity ^ 1) * e.B + blockIdx.y].decision == NDP_DEC_ADVANCE) {
            // no step, fresh moments for the next level (registration.py:176): the two matrices' here, the rest in k_eng_update_rest
            float *m = e.adam_m + (size_t)blockIdx.y * e.p_stride, *v = e.adam_v + (size_t)blockIdx.y * e.p_stride;
            const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
            for (int i = threadIdx.x; i < NDP_W * NDP_W / 4; i += 512) {
                reinterpret_cast<float4 *>(m + off_W1)[i] = z; reinterpret_cast<float4 *>(v + off_W1)[i] = z;
                reinterpret_cast<float4 *>(m + off_W2)[i] = z; reinterpret_cast<float4 *>(v + off_W2)[i] = z;
            }
        }
        return;
    }
    const int nh = make_head_cfg(desc_at_level(e.desc, e.state[(size_t)(parity ^ 1) * e.B + blockIdx.y].step_level)).nh;
    PT_INIT;
    PT_DECL;
    const int t0 = threadIdx.x;
    int t = t0, lane = t & 63, wv = t >> 6, l15 = lane & 15, lk = lane >> 4, l31 = lane & 31, h = lane >> 5;
    int ob = wv & 3, kb = 2 * (wv >> 2);
    _Float16 *pet = reinterpret_cast<_Float16 *>(smb + BF_PES);
    float4 *gbhs = reinterpret_cast<float4 *>(smb + BF_GBH);
    _Float16 *l0rows = reinterpret_cast<_Float16 *>(smb + BF_L0);
    const _Float16 *lds16 = reinterpret_cast<const _Float16 *>(smb);
    float *whs = reinterpret_cast<float *>(smb + BF_WH);
    BfOffs offs = bf_offsets(lane, ob, kb, wv);
    const B8Scale sc = bf_scale(e, blockIdx.y);
    const float inv_w = 1.0f / BF_WS;
    const bool dump_dz1 = (e.gemm_mode & 32) != 0;                     // tests: dz1 also goes to HBM (over the h2 plane, where bwd2_8 leaves it)
    const int lds0 = (int)(size_t)(__attribute__((address_space(3))) unsigned char *)smb;   // LDS byte address of the dynamic region
    // a [64][128] fp32 tile of the activation store -> LDS region, 4 x 1 KiB per wave, asynchronous (vmcnt)
    auto dma_rows = [&](int plane_idx, int tile, int region) {
        const float *src = j.act + ((size_t)plane_idx * j.plane + (size_t)tile * NDP_TILE) * NDP_W;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int q = 4 * wv + i;                                // row pair (wv, lane: the per-tile opaque copies)
            bf_dma16(src + 2 * NDP_W * q + 4 * lane, lds0 + region + 1024 * q);
        }
    };
    // the tile's [64][16] dO rows: 4 x 1 KiB, waves 0..3
    auto dma_dO = [&](int tile) {
        if (wv < 4)
            bf_dma16(j.dO + (size_t)tile * NDP_TILE * NDP_NHMAX + 256 * wv + 4 * lane, lds0 + BF_DO + 1024 * wv);
    };
    dma_rows(2, j.tile0, BF_REGION);                                   // first tile: h2 plane image -> R1
    dma_dO(j.tile0);
    if (t < 256) gbhs[t] = make_float4(0.f, 0.f, 0.f, 0.f);
    h16x8 wt2[2][4], wt1[2][4];
    bf_load_wt(j.params + off_W2, wv, l15, lk, wt2);
    bf_load_wt(j.params + off_W1, wv, l15, lk, wt1);
    L0Ops w0;                                                        // layer 0's packed operand (four registers; until round 6 rebuilt per tile from
    f8_l0_weights(j.params + off_W0, j.params + off_b0, 16 * wv + l15, lk, w0);   //   an LDS copy of W0 | b0: ~60 vector instructions per wave and tile)
    f8_l0_init_rows(l0rows, 64, t, 512);
    {   // head matrix rows: requested unconditionally at a clamped index (as `i < nh * 128 ? Wh[i] : 0` each item was a branch around a
        // load with its own wait: three dependent global round trips in the prologue)
        static_assert(NDP_WHROWS * NDP_W == 3 * 512, "three head-matrix items per thread");
        float whv[3];
#pragma unroll
        for (int u = 0; u < 3; ++u) whv[u] = j.params[off_Wh + min(t + 512 * u, nh * NDP_W - 1)];
#pragma unroll
        for (int u = 0; u < 3; ++u) whs[t + 512 * u] = t + 512 * u < nh * NDP_W ? whv[u] : 0.f;
    }
    f32x16 dW2[2], dW1[2];
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) { dW2[m][r] = 0.f; dW1[m][r] = 0.f; }
    // 2^6 S dWh[j = 4 lk + r][k = 16 wv + l15]: kept in LDS between the tiles (BF_GWH; lanes lk == 3 hold rows 12..15, which no head has)
    f32x4v *gwh_l = reinterpret_cast<f32x4v *>(smb + BF_GWH) + 48 * wv + (lane < 48 ? lane : 0);
    if (lane < 48) { const f32x4v zero4 = {0.f, 0.f, 0.f, 0.f}; *gwh_l = zero4; }
    f32x4v gW0 = {0.f, 0.f, 0.f, 0.f};                               // S [dW0 | db0][feature 16 wv + 4 lk + r][column l15] (columns 0..5: W0, 6: b0)
    for (int i = t; i < 2 * 8 * BF_PEROW; i += 512) {                // the constant rows of the transposed encoding planes: row 6 = 1 (hi), row 7 = 0
        const int pl = i / (8 * BF_PEROW), n = (i / BF_PEROW) & 7;
        pet[i] = (_Float16)((pl == 0 && n == 6) ? 1.0f : 0.0f);
    }
    float4 cs2 = make_float4(0.f, 0.f, 0.f, 0.f);                    // db2: column sums of the dz2 values this thread forms
    float cs1[4] = {0.f, 0.f, 0.f, 0.f};                             // S db1: sums of this lane's S dz1 values (features 16 wv + 4 lk + r)
    // its six encoding values per point (columns 16..21 of the saved head record): waves 0..5, one dword per lane
    auto dma_pe = [&](int tile) {
        if (wv < 6) {
            const int idx = 64 * wv + lane;
            bf_dma4(j.heads + (size_t)(tile * NDP_TILE + idx / 6) * NDP_HROW + 16 + idx % 6, lds0 + BF_PEQ + 256 * wv);
        }
    };
    dma_pe(j.tile0);
    // A tile's dO rows, once they have landed (t < 256: row t >> 2, head rows 4 (t & 3) ..): dbh += dO; the rows scaled by S IN PLACE (the
    // dz2 chains then produce S dz2 -- powers of two commute with every rounding of the chain -- and nobody multiplies 16 values per
    // thread); S dO split ONCE into the transposed planes that dWh reads as its A operand.  Runs one stage AHEAD of the tile (in stage 4
    // of the previous one, whose dO rows are dead since stage 2), so that no barrier is needed between these writes and stage 2.
    _Float16 *dop = reinterpret_cast<_Float16 *>(smb + BF_DOP);
    auto dO_stage = [&](int tt) {
        if (tt < 256) {
            float4 *row = reinterpret_cast<float4 *>(smb + BF_DO) + tt;
            const float4 vo = *row;
            float4 g = gbhs[tt];
            g.x += vo.x; g.y += vo.y; g.z += vo.z; g.w += vo.w;
            gbhs[tt] = g;
            const float v[4] = {vo.x * sc.s, vo.y * sc.s, vo.z * sc.s, vo.w * sc.s};
            *row = make_float4(v[0], v[1], v[2], v[3]);
            if ((tt & 3) < BF_DOROWS / 4) {
                _Float16 *dp = dop + 4 * (tt & 3) * BF_PEROW + (tt >> 2);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    _Float16 a, l;
                    bf_split_g(v[e], a, l);
                    dp[e * BF_PEROW] = a; dp[(BF_DOROWS + e) * BF_PEROW] = l;
                }
            }
        }
    };
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                 // the first tile's: in the open, once per workgroup
    __syncthreads();
    dO_stage(t);
    PT(10);
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 1");      // MODE.FP16_OVFL for the tile loop (restored behind it)
    int par = 0;
    for (int tile = j.tile0; tile < j.n_tiles; tile += j.tile_step, par ^= 1) {
        const int base = tile * NDP_TILE;
        // The thread index is made opaque once per tile: every LDS / HBM address of the tile is then recomputed from it here (a few
        // vector instructions each) instead of being hoisted out of the tile loop as ~100 loop invariants that do not fit the
        // register file next to the stationary weights and accumulators (they went to scratch and came back one by one).
        t = t0;
        asm volatile("" : "+v"(t));
        lane = t & 63; wv = t >> 6; l15 = lane & 15; lk = lane >> 4; l31 = lane & 31; h = lane >> 5;
        ob = wv & 3; kb = 2 * (wv >> 2);
        offs = bf_offsets(lane, ob, kb, wv);
        const int rA = 0, rC = 2 * BF_REGION, rB = par ? 3 * BF_REGION : BF_REGION, rD = par ? BF_REGION : 3 * BF_REGION;
        const _Float16 *ph2 = reinterpret_cast<const _Float16 *>(smb + rB);                // the h2 plane image (hi | lo), until stage 3 takes the region for dz1
        const float *dOs = reinterpret_cast<const float *>(smb + BF_DO);
        _Float16 *ph1 = reinterpret_cast<_Float16 *>(smb + rC), *pz2 = reinterpret_cast<_Float16 *>(smb + rD);
        _Float16 *ph0 = reinterpret_cast<_Float16 *>(smb + rA), *pz1 = reinterpret_cast<_Float16 *>(smb + rB);
        // this wave's share of the tile's h2 rows has landed (and the small rows); its four h1 requests, issued last, may still be out:
        // the vector memory counter retires in order, and the h1 planes are not read before stage 3
        // (the FIRST tile has no h1 requests out yet -- they follow the barrier below -- and its last request is the encodings' one
        // dword per lane, which stage 1 reads: everything has to be in, vmcnt(0); the compiler's barrier is lgkmcnt-only because it
        // cannot see the inline-asm DMA)
        if (tile == j.tile0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        __syncthreads();                                             // ... everybody's; the previous tile's readers of every region are done
        PT(0);
        if (tile == j.tile0)
            dma_rows(1, tile, rC);                                   // the first tile's h1 PLANE IMAGE -> R2 (the forward stores h1 split and swizzled:
                                                                     //   32 KB per tile like the fp32 rows, nothing left to convert): first read in stage 3
        // ---- stage 1: the small rows -> LDS (the 2^6 h1 planes are already in R2: the forward's image, by DMA)
        if (t < 384) {
            const float pe6 = reinterpret_cast<const float *>(smb + BF_PEQ)[t];
            f8_l0_pack(pe6, t % 6, l0rows + (t / 6) * F8_L0ROW);
            const _Float16 ph = (_Float16)pe6;
            _Float16 *pr = pet + (t % 6) * BF_PEROW + bf_pe_slot(t / 6);
            pr[0] = ph; pr[8 * BF_PEROW] = (_Float16)(pe6 - (float)ph);
        }
        PTF(1);
        // ---- (no barrier: what follows reads only what the DMA brought -- dO rows, h2 rows -- and the staged head matrix)
        //      dWh, the dz2 chains -> S dz2 planes
        // dWh[j][c] += sum_p dO[p][j] h2[p][c] over the tile's 64 points, on the fp16 MFMA like everything else here (the fp32 MFMA it ran
        // on until round 4 -- sixteen 16x16x4 per wave and tile -- issues at the vector rate AND shuts the vector pipe of its SIMD out:
        // 3.6k cycles of a 29k-cycle tile): A = (S dO)^T, B = 2^6 h2, both split in registers from the fp32 rows in LDS (lane: head row /
        // column l15, points 32 s + 8 lk + e), two k-steps of three products into the one accumulator (scaled by 2^6 S; S is the pair's).
        {
            const _Float16 *ap = dop + (l15 < BF_DOROWS ? l15 : BF_DOROWS - 1) * BF_PEROW + 8 * lk;
            const int ha = bf_base(rB, offs.trh[0]), hb = bf_base(rB, offs.trh[1]);
            f32x4v *gl = reinterpret_cast<f32x4v *>(smb + BF_GWH) + 48 * wv + (lane < 48 ? lane : 0);
            f32x4v gWh = *gl;                                        // (lanes >= 48 read a slot that is not theirs: their rows are never stored)
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2) {
                const h16x8 Ah = *reinterpret_cast<const h16x8 *>(ap + 32 * s2), Al = *reinterpret_cast<const h16x8 *>(ap + BF_DOROWS * BF_PEROW + 32 * s2);
                const h16x8 Bh = bf_tr_frag(lds16, 2 * s2, 0, ha, hb), Bl = bf_tr_frag(lds16, 2 * s2, 1, ha, hb);
                gWh = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al, Bh, gWh, 0, 0, 0);
                gWh = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bl, gWh, 0, 0, 0);
                gWh = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah, Bh, gWh, 0, 0, 0);
            }
            if (lane < 48) *gl = gWh;
        }
        __builtin_amdgcn_sched_barrier(0);
        {   // dz2 of this thread's rows (t >> 5) + 16 i, columns 4 (t & 31) ..: the j = 0 .. nh-1 fma chain from zero in fp32 (K <= 12: on
            // split products its 6-term sums have nothing to average the 2^-22 per-product error over -- measured 3.7x the fp32
            // chain's error in dW2 -- and the MFMA form was not faster), masked by h2 > 0
            float4 z[4];
            float a[4][4];
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int c = 0; c < 4; ++c) a[i][c] = 0.f;
            const float *dr = dOs + (t >> 5) * NDP_NHMAX;
            // (the head count of NDP.yaml's SE3 / axis-angle levels as a compile-time trip count: every
            //  LDS address is then base + immediate and a row's dO values arrive in two reads; the run-time loop paid ~13 address and
            //  loop instructions and five reads per head row for its eight packed FMAs)
            if (nh == 6) bf_dz2_chain<6>(whs, dr, t, nh, a);
            else bf_dz2_chain<0>(whs, dr, t, nh, a);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int row = (t >> 5) + 16 * i;
                const h16x4 m2 = *reinterpret_cast<const h16x4 *>(ph2 + row * BF_ROW + ((4 * (t & 31)) ^ bf_swz(row)));   // h2's hi plane: the ReLU mask
                z[i] = make_float4(bf_pos(m2[0]) ? a[i][0] : 0.f, bf_pos(m2[1]) ? a[i][1] : 0.f, bf_pos(m2[2]) ? a[i][2] : 0.f, bf_pos(m2[3]) ? a[i][3] : 0.f);
                cs2.x += z[i].x; cs2.y += z[i].y; cs2.z += z[i].z; cs2.w += z[i].w;
            }
            bf_split_rows<false>(z, pz2, t, 1.0f);                  // (S dz2 already: the dO rows carry S)
        }
        PTF(3);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the h1 plane image
        __syncthreads();                                             // (the h2 rows are dead from here: their region takes the dz1 planes)
        PT(4);
        if (tile + j.tile_step < j.n_tiles) dma_dO(tile + j.tile_step);       // the next tile's dO rows (this tile's are dead since stage 2): in by stage 4,
                                                                              //   where dO_stage works on them
        // ---- stage 3: layer 2 -- weight gradient, data gradient -> S dz1 planes -- and h0 = relu(z0) -> 2^6 h0 planes (from the packed
        //      encoding rows written before the barrier above), ahead of the weight gradient.  Round 6 measured the recomputation in the
        //      24 MFMA gaps of the weight gradient and each data-gradient epilogue dealt over the next point group's gaps (a
        //      compile-time knob, since retired): same bits, no gain (profiles/r06_bwd_steps_ab.txt); the steps of h0_step are its unit.
        typedef float f32x2v __attribute__((ext_vector_type(2)));
        h16x8 h0_b; f32x4v h0_z; f32x2v h0_y[2]; h16x2 h0_hi[2];
        auto h0_step = [&](int i) {                                  // step i = 6 g + s of the recomputation (bitwise f8_l0_group + bf_act_s + bf_store4)
            const int g = i / 6, sx = i - 6 * g;
            if (sx == 0) h0_b = *reinterpret_cast<const h16x8 *>(l0rows + (16 * g + l15) * F8_L0ROW + 8 * lk);
            else if (sx == 1) { const f32x4v zero = {0.f, 0.f, 0.f, 0.f}; h0_z = __builtin_amdgcn_mfma_f32_16x16x32_f16(w0.a, h0_b, zero, 0, 0, 0); }
            else if (sx < 4) { const int q = sx - 2; h0_y[q][0] = bf_act_s(h0_z[2 * q]); h0_y[q][1] = bf_act_s(h0_z[2 * q + 1]); }   // 2^6 h0, bounded; its mask in hi's sign
            else if (sx == 4) { h0_hi[0] = __builtin_convertvector(h0_y[0], h16x2); h0_hi[1] = __builtin_convertvector(h0_y[1], h16x2); }
            else {
                const h16x2 l0 = __builtin_convertvector(h0_y[0] - __builtin_convertvector(h0_hi[0], f32x2v), h16x2);
                const h16x2 l1 = __builtin_convertvector(h0_y[1] - __builtin_convertvector(h0_hi[1], f32x2v), h16x2);
                const int p = 16 * g + l15, c = 16 * wv + 4 * lk;
                _Float16 *dst = ph0 + p * BF_ROW + (c ^ bf_swz(p));
                const h16x4 P0 = {h0_hi[0][0], h0_hi[0][1], h0_hi[1][0], h0_hi[1][1]}, P1 = {l0[0], l0[1], l1[0], l1[1]};
                *reinterpret_cast<h16x4 *>(dst) = P0;
                *reinterpret_cast<h16x4 *>(dst + BF_PLANE) = P1;
            }
        };
        // the epilogue of a point group of either data gradient: S dz = d / 2^6 where the activation's hi part is > 0 (the compare on the
        // fp16 itself), bounded, split -- in twelve steps (bf_dgrad_tile); e_* is its state between the steps
        f32x2v e_z[2]; h16x2 e_hi[2]; h16x4 e_hm; _Float16 e_m[4];
        auto epi_common = [&](const f32x4v &d, int k) {              // steps 1, 6..9 are the same for both layers
            if (k == 1) { e_z[0][0] = d[0] * inv_w; e_z[0][1] = d[1] * inv_w; e_z[1][0] = d[2] * inv_w; e_z[1][1] = d[3] * inv_w; }
            else if (k == 6 || k == 7) {
                const int q = k - 6;
                e_hi[q] = __builtin_convertvector(e_z[q], h16x2);
            } else if (k == 8 || k == 9) { const int q = k - 8; e_z[q] = e_z[q] - __builtin_convertvector(e_hi[q], f32x2v); }   // -> the lo parts, still fp32
        };
        float *zo = j.act + (2 * (size_t)j.plane + base) * NDP_W;
        auto epi2 = [&](int g, const f32x4v &d, int k) {
            const int p = 16 * g + l15, c = 16 * wv + 4 * lk;
            if (k == 0) e_hm = *reinterpret_cast<const h16x4 *>(ph1 + p * BF_ROW + (c ^ bf_swz(p)));   // hi part: > 0 exactly where h1 is
            else if (k >= 2 && k < 6) {
                const int r = k - 2;
                const float z = bf_pos(e_hm[r]) ? e_z[r >> 1][r & 1] : 0.f;                          // S dz1
                cs1[r] += z;
                e_z[r >> 1][r & 1] = z;
                if (k == 5 && dump_dz1)
                    *reinterpret_cast<float4 *>(zo + p * NDP_W + c) = make_float4(e_z[0][0] * sc.inv, e_z[0][1] * sc.inv, e_z[1][0] * sc.inv, e_z[1][1] * sc.inv);
            } else if (k == 10) {
                const h16x2 l0 = __builtin_convertvector(e_z[0], h16x2), l1 = __builtin_convertvector(e_z[1], h16x2);
                _Float16 *dst = pz1 + p * BF_ROW + (c ^ bf_swz(p));
                const h16x4 P0 = {e_hi[0][0], e_hi[0][1], e_hi[1][0], e_hi[1][1]}, P1 = {l0[0], l0[1], l1[0], l1[1]};
                *reinterpret_cast<h16x4 *>(dst) = P0;
                *reinterpret_cast<h16x4 *>(dst + BF_PLANE) = P1;
            } else epi_common(d, k);
        };
        const int fr2[4] = {bf_base(rD, offs.fr[0]), bf_base(rD, offs.fr[1]), bf_base(rD, offs.fr[2]), bf_base(rD, offs.fr[3])};
#pragma unroll
        for (int i = 0; i < 24; ++i) h0_step(i);
        __builtin_amdgcn_sched_barrier(0);
        bf_wgrad(lds16, rD, rC, offs, dW2);
        __builtin_amdgcn_sched_barrier(0);
        bf_dgrad_tile<false>(wt2, lds16, fr2, epi2);
        PTF(6);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");             // the next tile's dO rows (nothing else is out in this stage)
        __syncthreads();
        PT(7);
        // ---- stage 4: layer 1 -- weight gradient, data gradient -> dz0 -> [dW0 | db0]; the next tile's h2 image into the region layer 2 has
        //      finished with, its encodings, and dO_stage on its dO rows -- ahead of the weight gradient
        const bool has_next = tile + j.tile_step < j.n_tiles;
        float4 n_vo, n_g;
        auto next_step = [&](int i) {                                // step i of the next tile's preparation
            if (!has_next) return;
            const int nt = tile + j.tile_step;
            if (i < 4) {                                             // h2 image of the next tile over this tile's dz2 planes: 4 x 1 KiB per wave
                const int q = 4 * wv + i;
                bf_dma16(j.act + (2 * (size_t)j.plane + (size_t)nt * NDP_TILE) * NDP_W + 2 * NDP_W * q + 4 * lane, lds0 + rD + 1024 * q);
            } else if (i == 4) dma_pe(nt);
            else if (i < 10 && t < 256) {                            // dO_stage in five steps (waves 0..3)
                float4 *row = reinterpret_cast<float4 *>(smb + BF_DO) + t;
                if (i == 5) { n_vo = *row; n_g = gbhs[t]; }
                else if (i == 6) { n_g.x += n_vo.x; n_g.y += n_vo.y; n_g.z += n_vo.z; n_g.w += n_vo.w; gbhs[t] = n_g; }
                else if (i == 7) { n_vo.x *= sc.s; n_vo.y *= sc.s; n_vo.z *= sc.s; n_vo.w *= sc.s; *row = n_vo; }
                else if ((t & 3) < BF_DOROWS / 4) {
                    _Float16 *dp = dop + 4 * (t & 3) * BF_PEROW + (t >> 2);
                    const float v[2] = {i == 8 ? n_vo.x : n_vo.z, i == 8 ? n_vo.y : n_vo.w};
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        _Float16 a, l;
                        bf_split_g(v[e], a, l);
                        dp[(2 * (i - 8) + e) * BF_PEROW] = a; dp[(BF_DOROWS + 2 * (i - 8) + e) * BF_PEROW] = l;
                    }
                }
            }
        };
        // The data gradient with its operands SWAPPED (A = the dz1 fragment, B = the weight slice): the accumulator then holds
        // feature 16 wv + l15 of points 16 g + 4 lk + r -- which is the A-operand layout of a 16x16x32 MFMA whose contraction runs
        // over the points: two groups fill the eight slots of a lane, and [dW0 | db0] += (S dz0)^T [pe | 1] is three products per
        // 32 points on the transposed encoding planes (until the second half of round 4: seven fp32 FMAs per value -- 2.55 ns each
        // -- and two LDS reads per point).
        const int f = 16 * wv + l15;
        h16x2 zhp[4], zlp[4];                                        // S dz0 of this lane's eight points of a group pair: hi, lo (pairs of slots)
        h16x8 e_Bh, e_Bl;
        const _Float16 *bp = pet + (l15 < 7 ? l15 : 7) * BF_PEROW + 8 * lk;      // (columns 7..15 of the product: the zero row)
        auto epi1 = [&](int g, const f32x4v &d, int k) {
            if (k == 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) { const int p = 16 * g + 4 * lk + r; e_m[r] = ph0[p * BF_ROW + (f ^ bf_swz(p))]; }   // hi part: > 0 exactly where h0 is
            } else if (k >= 2 && k < 6) {
                const int r = k - 2;
                e_z[r >> 1][r & 1] = bf_pos(e_m[r]) ? e_z[r >> 1][r & 1] : 0.f;                      // S dz0
                if (k == 5 && (g & 1)) { e_Bh = *reinterpret_cast<const h16x8 *>(bp + 32 * (g >> 1)); e_Bl = *reinterpret_cast<const h16x8 *>(bp + 8 * BF_PEROW + 32 * (g >> 1)); }
            } else if (k == 10) {
                zhp[2 * (g & 1)] = e_hi[0]; zhp[2 * (g & 1) + 1] = e_hi[1];
                zlp[2 * (g & 1)] = __builtin_convertvector(e_z[0], h16x2); zlp[2 * (g & 1) + 1] = __builtin_convertvector(e_z[1], h16x2);
            } else if (k == 11) {
                if (g & 1) {
                    const h16x8 zh = {zhp[0][0], zhp[0][1], zhp[1][0], zhp[1][1], zhp[2][0], zhp[2][1], zhp[3][0], zhp[3][1]};
                    const h16x8 zl = {zlp[0][0], zlp[0][1], zlp[1][0], zlp[1][1], zlp[2][0], zlp[2][1], zlp[3][0], zlp[3][1]};
                    gW0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(zl, e_Bh, gW0, 0, 0, 0);
                    gW0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, e_Bl, gW0, 0, 0, 0);
                    gW0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(zh, e_Bh, gW0, 0, 0, 0);
                }
            } else epi_common(d, k);
        };
        const int fr1[4] = {bf_base(rB, offs.fr[0]), bf_base(rB, offs.fr[1]), bf_base(rB, offs.fr[2]), bf_base(rB, offs.fr[3])};
#pragma unroll
        for (int i = 0; i < 10; ++i) next_step(i);
        bf_wgrad(lds16, rB, rA, offs, dW1);
        __builtin_amdgcn_sched_barrier(0);
        // the next tile's h1 image, BETWEEN the stage's two contractions (round 6): the h2 image, which must land within this stage, still
        // has a head start of the weight gradient, and h1 -- read in stage 3 -- no longer has only stages 1-2 to arrive in, which this round
        // made 40 % shorter (requested at the end of the stage, round 4's place, a compile-time knob since retired: +1.3 % at 256 pairs,
        // profiles/r06_bwd_h1req_ab.txt)
        if (has_next) dma_rows(1, tile + j.tile_step, rC);
        __builtin_amdgcn_sched_barrier(0);
        bf_dgrad_tile<true>(wt1, lds16, fr1, epi1);
        PTF(9);
    }
    asm volatile("s_setreg_imm32_b32 hwreg(HW_REG_MODE, 23, 1), 0");
    // ---- the workgroup's gradient partial
    t = t0; lane = t & 63; wv = t >> 6; l15 = lane & 15; lk = lane >> 4; l31 = lane & 31; h = lane >> 5; ob = wv & 3; kb = 2 * (wv >> 2);
    float *G = j.gpart;
    const float inv_g = sc.inv * (1.0f / BF_HS);
    if (!bf_adam_in_tail(e)) {                                        // (stepped below straight from the accumulators otherwise: no partial of them)
        bf_store_dW(G + off_W2, dW2, inv_g, ob, kb, l31, h);
        bf_store_dW(G + off_W1, dW1, inv_g, ob, kb, l31, h);
    }
    float *scratch = reinterpret_cast<float *>(smb + BF_R0);          // the regions are dead from here
    cs2.x *= sc.inv; cs2.y *= sc.inv; cs2.z *= sc.inv; cs2.w *= sc.inv;     // (the chains summed S dz2)
    b8_colsum_finish<true>(cs2, scratch, G + off_b2, t);
    // dWh rows j < nh (D layout: lane holds column k = 16 wv + l15 of rows j = 4 lk + r), dbh
    float *gwh = G + off_Wh;
    const f32x4v gWh = *(reinterpret_cast<const f32x4v *>(smb + BF_GWH) + 48 * wv + (lane < 48 ? lane : 0));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int jr = 4 * lk + r;
        if (jr < nh) gwh[jr * NDP_W + 16 * wv + l15] = gWh[r] * inv_g;
    }
    lds_barrier();                                                   // (LDS only: not the gradient stores' acknowledgements)
    if (t < nh) {
        const float *gb = reinterpret_cast<const float *>(gbhs);
        float s = 0.f;
        for (int q = 0; q < 64; ++q) s += gb[4 * (4 * q + (t >> 2)) + (t & 3)];          // thread 4 q + (j >> 2), component j & 3
        gwh[nh * NDP_W + t] = s;
    }
    // [dW0 | db0]: complete in the accumulator (feature 16 wv + 4 lk + r, column l15);  db1: this lane's partial of features
    // 16 wv + 4 lk + r -> sum over the 16 lanes (points) of the group, in lane order
    lds_barrier();                                                   // (LDS only: not the gradient stores' acknowledgements)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int k = 16 * wv + 4 * lk + r;
        if (l15 < 6) G[off_W0 + k * 6 + l15] = gW0[r] * sc.inv;
        else if (l15 == 6) G[off_b0 + k] = gW0[r] * sc.inv;
    }
    float *scr1 = scratch + NDP_W * 8 * 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) scr1[(16 * wv + 4 * lk + r) * 16 + l15] = cs1[r];
    lds_barrier();                                                   // (LDS only: not the gradient stores' acknowledgements)
    for (int k = t; k < NDP_W; k += 512) {
        float s = 0.f;
#pragma unroll
        for (int q = 0; q < 16; ++q) s += scr1[k * 16 + q];
        G[off_b1 + k] = s * sc.inv;
    }
    if (bf_adam_in_tail(e)) {                                         // G == 1: this workgroup's partial IS the gradient
        lds_barrier();                                               // everybody is done with the scratch above
        float *gl = reinterpret_cast<float *>(smb + BF_R0);          // [2][128][128] fp32 = the four regions
#pragma unroll
        for (int mm = 0; mm < 2; ++mm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = (32 * ob + mfma_row(r, h)) * NDP_W + 32 * (kb + mm) + l31;
                gl[o] = dW2[mm][r] * inv_g;
                gl[NDP_W * NDP_W + o] = dW1[mm][r] * inv_g;
            }
        lds_barrier();
        const ndp_pair_state *nsp = e.state + (size_t)(parity ^ 1) * e.B + blockIdx.y;
        const int step_t = nsp->step_t, step_level = nsp->step_level;
        const BfAdamK ak = {e.adam_w1, e.adam_b2, e.adam_w2, e.adam_eps, e.adam_tab[2 * step_t], e.adam_tab[2 * step_t + 1]};
        bf_adam_tail(e.params + ((size_t)blockIdx.y * e.m + step_level) * e.p_stride, e.adam_m + (size_t)blockIdx.y * e.p_stride,
                     e.adam_v + (size_t)blockIdx.y * e.p_stride, ak, nsp->decision != NDP_DEC_STEP ? 1 : 0, gl, off_W2, off_W1);
    }
    PT(11);
}

extern "C" __global__ void __launch_bounds__(512, 1)
k_eng_bwd_f(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smb[];
    eng_bwd_f_stage(e, parity, smb);
    PT_FLUSH(24);
}
