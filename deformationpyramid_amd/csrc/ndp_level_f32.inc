// ndp_level_f32.inc -- the fp32-MFMA level kernels (what gemm_mode 0 runs): LDS carve, level forward, k_pyramid_fwd, the two-launch
// level backward (bwd2 / bwd1), the stand-alone k_level_* / k_head_bwd* kernels and k_grad_reduce.
//
// Design (see DESIGN.md):
//   * One workgroup = 256 threads = 4 wave64.  A tile is 64 points.  Wave w owns output columns
//     [32w, 32w+32) of every 128-wide layer.
//   * The 128x128 weight matrices are WEIGHT-STATIONARY IN REGISTERS: each lane holds its 64-float
//     slice in the v_mfma_f32_32x32x2_f32 B-operand layout (forward: W[o][k] slices of W1 and W2;
//     backward, one layer per kernel: the transposed slice) for the whole life of the workgroup,
//     so the only per-MFMA operand fetch is one LDS read of the activation.
//   * Activations move through two [64][132] LDS tiles (+4 float pad: ds_read_b128 of a column
//     block is bank-conflict free).  fp32 in, fp32 accumulate: the MFMA result is bitwise an fmaf
//     chain, which is what the 1e-4 parity budget needs.  Everything that is a small GEMM runs on
//     the matrix pipe too (6 -> 128 input layer, the 16-wide heads and the 6-wide input-layer
//     gradient on v_mfma_f32_16x16x4_f32): VALU loops over LDS next to MFMA phases are what a tile
//     used to wait for.
//   * The backward keeps one 128x128 dW in accumulator registers across all of the workgroup's tiles
//     and writes ONE partial per workgroup; partials are folded in index order by the Adam kernel --
//     no float atomics anywhere, results are bit-reproducible.
//   * The batched engine advances B independent pairs per launch, every pair at its own level and
//     iteration; the early-stop rule runs on the device in double, so the host never syncs per
//     iteration (the reference syncs three times: registration.py:226-232).  Slot refill, pair
//     preparation and the final all-point warp are batched single launches as well.
// ------------------------------------------------------------------------------------------------
// LDS carve (floats).  All scratch lives in the dynamic region (16-byte aligned offsets).
// ------------------------------------------------------------------------------------------------
#define NDP_WHROWS 12                     /* head rows staged in LDS (at most 6 + 1 + 3 + 1 = 11 are used) */
enum : int {
    L_BUFA = 0,
    L_BUFB = L_BUFA + 64 * NDP_LD,
    L_HO = L_BUFB,                        // [64][16] head outputs: reuses bufB, which is dead after layer 2
    L_PE = L_BUFB + 64 * NDP_LD,          // 2 x [64][9] posenc, double-buffered across tiles (stride 9: conflict-free)
    L_XS = L_PE + 2 * 64 * 9,             // 2 x [64][4] level input x
    L_WH = L_XS + 2 * 64 * 4,             // [12][NDP_LD] head weights
    L_BH = L_WH + NDP_WHROWS * NDP_LD,    // [16]
    L_FWD_TOTAL = L_BH + NDP_NHMAX
};
static constexpr int kSmemFwdBytes = L_FWD_TOTAL * 4;     // 80 640 B: two workgroups per CU
static_assert(2 * kSmemFwdBytes <= 160 * 1024, "forward LDS carve must allow two workgroups per CU");

struct LevelJob {
    const float *params;
    float freq;
    const float *x_in;
    float *x_out;
    float *act;        // [3][plane][128] or nullptr
    float *heads;      // [plane][NDP_HROW] or nullptr: 16 scaled head outputs + 6 posenc values
    float *nonrig;     // [n] or nullptr: gate value per point (levels with the nonrigidity head)
    int n;             // live points
    int plane;         // rows per activation plane (capacity, multiple of 64)
    int n_tiles;       // live tiles = ceil(n / 64)
    int tile0, tile_step;
};

// lane-resident slice of a 128x128 matrix in the 32x32x2 B-operand layout
//   forward : w[ks] = W[32*wv + l31][64*h + ks]        (contraction index k = 64*h + ks)
//   backward: w[ks] = W[64*h + ks][32*wv + l31]        (contraction index o = 64*h + ks)
// Both go through LDS: the matrix is pulled from L2/HBM by LDS-DMA as 1 KiB blocks (two consecutive rows per instruction,
// perfectly coalesced) into the row-pair padded image the backward tiles use (float index of (r, c) = 260 (r >> 1) +
// 128 (r & 1) + c; 64 pairs = 66 560 B, the two tile buffers of either carve), and the lanes pick their slices out of LDS.
// (Straight from global, a lane's 64 floats are 16 float4 loads that touch 64 different cache lines per instruction --
//  eight times the line requests the data needs: 27-28k cycles of prologue per workgroup, and per LEVEL in the final warp.)
#define WIMG_PAIR 260
__device__ __forceinline__ int wimg_row(int r) { return WIMG_PAIR * (r >> 1) + NDP_W * (r & 1); }
// wave wv lays down rows 32wv .. 32wv+31 of W (16 row pairs); asynchronous, wait with s_waitcnt vmcnt(0)
__device__ __forceinline__ void wimg_load_rows(const float *W, float *img /*LDS*/, int wv, int lane) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int q = 16 * wv + i;
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(W + 2 * NDP_W * q + 4 * lane),
                                         (__attribute__((address_space(3))) void *)(img + WIMG_PAIR * q), 16, 0, 0);
    }
}
// forward slice: the rows a wave reads are the rows it loaded itself, so no workgroup barrier is needed -- only its own
// DMA (vmcnt) before the reads, and its own reads (lgkmcnt) before the image is overwritten by the next matrix.
__device__ __forceinline__ void load_w_fwd(const float *W, float *img /*LDS*/, int wv, int l31, int h, float (&w)[64]) {
    wimg_load_rows(W, img, wv, threadIdx.x & 63);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    const float *src = img + wimg_row(32 * wv + l31) + 64 * h;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 v = *reinterpret_cast<const float4 *>(src + 4 * i);
        w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}
// backward (transposed) slice: a lane's column crosses the rows of all four waves -> barrier on both sides
__device__ __forceinline__ void load_w_bwd(const float *W, float *img /*LDS*/, int wv, int l31, int h, float (&w)[64]) {
    wimg_load_rows(W, img, wv, threadIdx.x & 63);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const float *src = img + 32 * wv + l31;
#pragma unroll
    for (int i = 0; i < 64; ++i) w[i] = src[wimg_row(64 * h + i)];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __syncthreads();
}

// OUT^T[o][p] += sum_k W[o][k] * in[p][k] for the 64 points of a tile: the weight slice is the MFMA A operand
// (row m = this lane's output feature 32wv + l31), the activation row of point l31 (+32) the B operand.  In the
// resulting C layout a lane holds point p = l31 (acc0) / l31 + 32 (acc1) and, per register group g = r >> 2, the FOUR
// CONSECUTIVE output features 32wv + 8g + 4h + (r & 3): epilogues read/write row-major tiles with b128 LDS accesses.
__device__ __forceinline__ void tile_gemm_64x32(const float *in /*LDS [64][LD]*/, const float (&w)[64],
                                                int l31, int h, f32x16 &acc0, f32x16 &acc1) {
    const float *r0 = in + l31 * NDP_LD + 64 * h;
    const float *r1 = r0 + 32 * NDP_LD;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 a0 = *reinterpret_cast<const float4 *>(r0 + 4 * i);
        const float4 a1 = *reinterpret_cast<const float4 *>(r1 + 4 * i);
        acc0 = MFMA32(w[4 * i], a0.x, acc0);     acc1 = MFMA32(w[4 * i], a1.x, acc1);
        acc0 = MFMA32(w[4 * i + 1], a0.y, acc0); acc1 = MFMA32(w[4 * i + 1], a1.y, acc1);
        acc0 = MFMA32(w[4 * i + 2], a0.z, acc0); acc1 = MFMA32(w[4 * i + 2], a1.z, acc1);
        acc0 = MFMA32(w[4 * i + 3], a0.w, acc0); acc1 = MFMA32(w[4 * i + 3], a1.w, acc1);
        // keep the compiler from hoisting all 32 operand reads to the top (64 extra live VGPRs -> spills
        // at the 256-register budget of two workgroups per CU); 4 iterations in flight are plenty
        if ((i & 3) == 3) asm volatile("" ::: "memory");
    }
}
// accumulators that start at the layer's bias: one extra MFMA k-step with A = (bias, 0), B = (1, 0) puts bias[o] into
// every element exactly (0 + b * 1), so the chain stays "bias, then k = 0 .. K-1" without 16 bias registers per lane
__device__ __forceinline__ void acc_init_bias(float bias_lane, int h, f32x16 &acc0, f32x16 &acc1) {
    f32x16 z;
#pragma unroll
    for (int r = 0; r < 16; ++r) z[r] = 0.f;
    const float a = h == 0 ? bias_lane : 0.f, b = h == 0 ? 1.0f : 0.f;
    acc0 = MFMA32(a, b, z);
    acc1 = MFMA32(a, b, z);
}
// ReLU epilogue of tile_gemm_64x32: [p][32wv + 8g + 4h .. +3] <- max(acc, 0), eight ds_write_b128 per lane
__device__ __forceinline__ void epilogue_relu(const f32x16 &acc0, const f32x16 &acc1, float *out /*LDS [64][LD]*/,
                                              int wv, int l31, int h) {
    float *o0 = out + l31 * NDP_LD + 32 * wv + 4 * h, *o1 = o0 + 32 * NDP_LD;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        *reinterpret_cast<float4 *>(o0 + 8 * g) = make_float4(fmaxf(acc0[4 * g], 0.f), fmaxf(acc0[4 * g + 1], 0.f),
                                                                fmaxf(acc0[4 * g + 2], 0.f), fmaxf(acc0[4 * g + 3], 0.f));
        *reinterpret_cast<float4 *>(o1 + 8 * g) = make_float4(fmaxf(acc1[4 * g], 0.f), fmaxf(acc1[4 * g + 1], 0.f),
                                                                fmaxf(acc1[4 * g + 2], 0.f), fmaxf(acc1[4 * g + 3], 0.f));
    }
}
// backward epilogue of tile_gemm_64x32: z = d * [hmask > 0] -> zout (same tile coordinates), b128 reads and writes
__device__ __forceinline__ void epilogue_mask(const f32x16 &d0, const f32x16 &d1, const float *hmask /*LDS*/,
                                              float *zout /*LDS*/, int wv, int l31, int h) {
    const int off = l31 * NDP_LD + 32 * wv + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 m0 = *reinterpret_cast<const float4 *>(hmask + off + 8 * g);
        const float4 m1 = *reinterpret_cast<const float4 *>(hmask + off + 32 * NDP_LD + 8 * g);
        *reinterpret_cast<float4 *>(zout + off + 8 * g) =
            make_float4(m0.x > 0.f ? d0[4 * g] : 0.f, m0.y > 0.f ? d0[4 * g + 1] : 0.f,
                        m0.z > 0.f ? d0[4 * g + 2] : 0.f, m0.w > 0.f ? d0[4 * g + 3] : 0.f);
        *reinterpret_cast<float4 *>(zout + off + 32 * NDP_LD + 8 * g) =
            make_float4(m1.x > 0.f ? d1[4 * g] : 0.f, m1.y > 0.f ? d1[4 * g + 1] : 0.f,
                        m1.z > 0.f ? d1[4 * g + 2] : 0.f, m1.w > 0.f ? d1[4 * g + 3] : 0.f);
    }
}

// [64][128] tile: LDS (row stride NDP_LD) -> global, 8 float4 per thread, fully coalesced
__device__ __forceinline__ void store_tile_from_lds(const float *src /*LDS*/, float *dst /*global [64][128]*/) {
    const int t = threadIdx.x;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = t + 256 * i;
        reinterpret_cast<float4 *>(dst)[idx] = *reinterpret_cast<const float4 *>(src + (idx >> 5) * NDP_LD + 4 * (idx & 31));
    }
}

// C/D layout of v_mfma_f32_32x32x2_f32: reg r of lane l holds row (r&3) + 8*(r>>2) + 4*(l>>5), col l&31
__device__ __forceinline__ int mfma_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// ------------------------------------------------------------------------------------------------
// Level forward  (nets.py:111-140)
// ------------------------------------------------------------------------------------------------
// lane-resident operands of one level (weight-stationary for as long as the level lasts)
struct FwdWeights {
    float w1[64], w2[64], w0b[3];
    float bias0, bias1, bias2;
};

// Loads a level's weights into registers and stages its head matrix in LDS (row stride NDP_LD, so that the
// 16x16x4 MFMA B-operand reads are conflict-free).  The caller must pass a barrier before the first head phase
// (the tile's own barriers do) and after the last one before reloading.
__device__ __forceinline__ void fwd_load_weights(const HeadCfg &hc, const float *P, float *sm, FwdWeights &fw) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    float *whs = sm + L_WH, *bhs = sm + L_BH;
    const ndp_layer_desc dd = {NDP_W, 2, hc.motion, hc.rotfmt, 0, hc.mlp_scale};
    const float *W0 = P + ndp_off_W0(&dd), *b0 = P + ndp_off_b0(&dd);
    const float *W1 = P + ndp_off_Wi(&dd, 1), *b1 = P + ndp_off_bi(&dd, 1);
    const float *W2 = P + ndp_off_Wi(&dd, 2), *b2 = P + ndp_off_bi(&dd, 2);
    const float *Wh = P + ndp_off_Wi(&dd, 3);      // == ndp_off_Wh for nonrigidity = 0
    const float *bh = Wh + hc.nh * NDP_W;
    load_w_fwd(W1, sm + L_BUFA, wv, l31, h, fw.w1);
    load_w_fwd(W2, sm + L_BUFA, wv, l31, h, fw.w2);
    fw.bias1 = b1[32 * wv + l31];
    fw.bias2 = b2[32 * wv + l31];
    // layer 0 (6 -> 128) also runs on the matrix pipe: K = 6 = 3 k-steps of the 32x32x2 MFMA
#pragma unroll
    for (int ks = 0; ks < 3; ++ks) fw.w0b[ks] = W0[(32 * wv + l31) * 6 + 2 * ks + h];
    fw.bias0 = b0[32 * wv + l31];
    for (int i = t; i < NDP_WHROWS * NDP_W; i += 256)
        whs[(i >> 7) * NDP_LD + (i & 127)] = (i < hc.nh * NDP_W) ? Wh[i] : 0.f;
    if (t < NDP_NHMAX) bhs[t] = (t < hc.nh) ? bh[t] : 0.f;
}

// where one tile's input comes from and where its outputs go
struct TileIO {
    const float *x_in;      // global [n][3], or nullptr: the tile's input already sits in LDS (xs)
    const float *shift_in;  // [3] subtracted from x_in (or nullptr)
    float *x_out;           // global [n][3], or nullptr: the warped points replace xs (next level reads them)
    const float *shift_out; // [3] added to x_out (or nullptr)
    float *act;             // [3][plane][128] or nullptr
    float *heads;           // [plane][NDP_HROW] or nullptr
    float *nonrig;          // [n] or nullptr
    int n, plane;
};

// level input of point `base + lane`, coordinate `axis` (zero beyond n)
__device__ __forceinline__ float fwd_fetch_x(const TileIO &io, int base, int lane, int axis) {
    const int p = base + lane;
    if (p >= io.n) return 0.f;
    const float xa = io.x_in[3 * (size_t)p + axis];
    return io.shift_in ? xa - io.shift_in[axis] : xa;
}

// positional encoding (nets.py:164-177) of one coordinate of one point -> pe / xs of the given LDS set
__device__ __forceinline__ void fwd_posenc(float xa, float freq, int lane, int axis, float *pe, float *xs, bool write_x) {
    float sn, cs;
    sincosf(xa * freq, &sn, &cs);
    pe[lane * 9 + 2 * axis] = sn;
    pe[lane * 9 + 2 * axis + 1] = cs;
    if (write_x) xs[4 * lane + axis] = xa;
}

// One 64-point tile from its positional encoding (pe) to the scaled head outputs (ho, which reuses bufB):
// 3 layers on the 32x32x2 MFMA, heads on the 16x16x4 MFMA; activations -> HBM.  Ends with a barrier.
__device__ __forceinline__ void fwd_tile_core(const HeadCfg &hc, const FwdWeights &fw, const TileIO &io, int base,
                                              float *sm, const float *pe) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    float *bufA = sm + L_BUFA, *bufB = sm + L_BUFB;
    float *whs = sm + L_WH, *bhs = sm + L_BH, *ho = sm + L_HO;
    PT_DECL;
    // ---- layer 0 (MFMA, bitwise the k = 0..5 fmaf chain starting from the bias) -> bufA
    {
        f32x16 acc0, acc1;
        acc_init_bias(fw.bias0, h, acc0, acc1);
#pragma unroll
        for (int ks = 0; ks < 3; ++ks) {
            const float a0 = pe[l31 * 9 + 2 * ks + h], a1 = pe[(l31 + 32) * 9 + 2 * ks + h];
            acc0 = MFMA32(fw.w0b[ks], a0, acc0);
            acc1 = MFMA32(fw.w0b[ks], a1, acc1);
        }
        epilogue_relu(acc0, acc1, bufA, wv, l31, h);
    }
    PT(2);
    __syncthreads();
    PT(3);
    // ---- layer 1 (MFMA) bufA -> bufB ; h0 goes to HBM as float4 rows while the matrix pipe works
    {
        f32x16 acc0, acc1;
        acc_init_bias(fw.bias1, h, acc0, acc1);
        if (io.act) store_tile_from_lds(bufA, io.act + (size_t)base * NDP_W);
        tile_gemm_64x32(bufA, fw.w1, l31, h, acc0, acc1);
        epilogue_relu(acc0, acc1, bufB, wv, l31, h);
    }
    PT(4);
    __syncthreads();
    PT(5);
    // ---- layer 2 (MFMA) bufB -> bufA ; h1 -> HBM
    {
        f32x16 acc0, acc1;
        acc_init_bias(fw.bias2, h, acc0, acc1);
        if (io.act) store_tile_from_lds(bufB, io.act + ((size_t)io.plane + base) * NDP_W);
        tile_gemm_64x32(bufB, fw.w2, l31, h, acc0, acc1);
        epilogue_relu(acc0, acc1, bufA, wv, l31, h);
    }
    PT(6);
    __syncthreads();                                                                          // bufB (h1) is dead from here
    PT(7);
    if (io.act) store_tile_from_lds(bufA, io.act + (2 * (size_t)io.plane + base) * NDP_W);   // h2 -> HBM
    PT(11);
    // ---- heads (nets.py:117,125,146) on the 16x16x4 MFMA: wave w owns points 16w..16w+15, the 16 columns are
    //      the head rows (zero beyond nh).  A[p][k]: lane = p + 16*(k mod 4 group); D[p][j]: lane = j + 16*(p/4).
    {
        const int l15 = lane & 15, lk = lane >> 4;
        f32x4 acc;
        const float bj = bhs[l15];
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = bj;
        const float *arow = bufA + (16 * wv + l15) * NDP_LD + 4 * lk;
        const float *brow = whs + (l15 < NDP_WHROWS ? l15 : 0) * NDP_LD + 4 * lk;
        const bool live = l15 < NDP_WHROWS;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const float4 a = *reinterpret_cast<const float4 *>(arow + 16 * q);
            float4 b = *reinterpret_cast<const float4 *>(brow + 16 * q);
            if (!live) b = make_float4(0.f, 0.f, 0.f, 0.f);
            acc = MFMA16(a.x, b.x, acc);
            acc = MFMA16(a.y, b.y, acc);
            acc = MFMA16(a.z, b.z, acc);
            acc = MFMA16(a.w, b.w, acc);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) ho[(16 * wv + 4 * lk + r) * NDP_NHMAX + l15] = hc.mlp_scale * acc[r];
    }
    PT(8);
    __syncthreads();
    PT(9);
}

// warp (nets.py:119-129) of the tile's 64 points by ONE wave (lane = point): reads ho / xs / pe of the tile.
__device__ __forceinline__ void fwd_warp(const HeadCfg &hc, const TileIO &io, int base, int lane, const float *ho,
                                         const float *pe, float *xs) {
    const int p = base + lane;
    const float *o = ho + lane * NDP_NHMAX;
    if (io.heads) {
        float *hr = io.heads + (size_t)p * NDP_HROW;
#pragma unroll
        for (int j = 0; j < NDP_NHMAX; j += 4)
            *reinterpret_cast<float4 *>(hr + j) = *reinterpret_cast<const float4 *>(o + j);
        const float *pr = pe + lane * 9;
        *reinterpret_cast<float4 *>(hr + 16) = make_float4(pr[0], pr[1], pr[2], pr[3]);
        *reinterpret_cast<float4 *>(hr + 20) = make_float4(pr[4], pr[5], 0.f, 0.f);
    }
    if (p < io.n) {
        PointHead c;
        float out[3];
        head_warp_fwd(hc, o, xs + 4 * lane, c, out);
        if (io.x_out) {
            if (io.shift_out) { out[0] += io.shift_out[0]; out[1] += io.shift_out[1]; out[2] += io.shift_out[2]; }
            io.x_out[3 * (size_t)p] = out[0]; io.x_out[3 * (size_t)p + 1] = out[1]; io.x_out[3 * (size_t)p + 2] = out[2];
        } else {
            xs[4 * lane] = out[0]; xs[4 * lane + 1] = out[1]; xs[4 * lane + 2] = out[2];
        }
        if (io.nonrig) io.nonrig[p] = c.nr;
    }
}

// All tiles of a workgroup through one level.  Software pipeline across tiles: while wave 0 warps tile i, waves
// 1..3 (one per coordinate axis) encode tile i+1 into the other pe/xs set from an x value they fetched at the top
// of tile i, so neither the x load latency nor sincosf sits on the critical path.
__device__ __forceinline__ void level_fwd_body(const HeadCfg &hc, const LevelJob &job, float *sm) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    FwdWeights fw;
    fwd_load_weights(hc, job.params, sm, fw);
    TileIO io;
    io.x_in = job.x_in; io.shift_in = nullptr; io.x_out = job.x_out; io.shift_out = nullptr;
    io.act = job.act; io.heads = job.heads; io.nonrig = job.nonrig; io.n = job.n; io.plane = job.plane;
    float *pe = sm + L_PE, *xs = sm + L_XS, *ho = sm + L_HO;
    int tile = job.tile0, cur = 0;
    if (tile >= job.n_tiles) return;
    if (wv > 0) fwd_posenc(fwd_fetch_x(io, tile * NDP_TILE, lane, wv - 1), job.freq, lane, wv - 1, pe, xs, true);
    __syncthreads();
    for (; tile < job.n_tiles; tile += job.tile_step) {
        const int next = tile + job.tile_step;
        float xn = 0.f;
        if (wv > 0 && next < job.n_tiles) xn = fwd_fetch_x(io, next * NDP_TILE, lane, wv - 1);
        fwd_tile_core(hc, fw, io, tile * NDP_TILE, sm, pe + cur * (64 * 9));
        if (wv == 0) fwd_warp(hc, io, tile * NDP_TILE, lane, ho, pe + cur * (64 * 9), xs + cur * (64 * 4));
        else if (next < job.n_tiles)
            fwd_posenc(xn, job.freq, lane, wv - 1, pe + (cur ^ 1) * (64 * 9), xs + (cur ^ 1) * (64 * 4), true);
        __syncthreads();
        cur ^= 1;
    }
}

// Whole pyramid for one 64-point tile per workgroup: the points stay in LDS from level to level, the weights of
// each level are re-read from L2 (135 KB per level; the grid is sized so that several clouds fill the chip).
struct WarpJobs {
    ndp_warp_job j[NDP_MAX_WARP_JOBS];
};
// A workgroup carries TWO 64-point tiles through all m levels (the two posenc / point sets of the LDS carve): the 135 KB of
// a level's weights are pulled from L2 once per 128 points instead of once per 64 -- the weight prologue was half of the
// kernel -- and the posenc of the second tile overlaps the warp of the first exactly as in the level kernel.
#define NDP_PYR_TILES 2
extern "C" __global__ void __launch_bounds__(256, 2)
k_pyramid_fwd(ndp_layer_desc desc, int m, int k0, int p_stride, WarpJobs jobs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const ndp_warp_job jb = jobs.j[blockIdx.y];
    const int base0 = blockIdx.x * NDP_TILE * NDP_PYR_TILES;
    if (base0 >= jb.n) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    float *pe = sm + L_PE, *xs = sm + L_XS, *ho = sm + L_HO;
    const bool two = base0 + NDP_TILE < jb.n;                      // the second tile holds points
    TileIO io;
    io.act = nullptr; io.heads = nullptr; io.nonrig = nullptr; io.n = jb.n; io.plane = 0;
    io.x_in = jb.x; io.shift_in = jb.shift_in;
    for (int l = 0; l < m; ++l) {
        const HeadCfg hc = make_head_cfg(desc_at_level(desc, l));
        FwdWeights fw;
        fwd_load_weights(hc, jb.params + (size_t)l * p_stride, sm, fw);
        io.x_out = l == m - 1 ? jb.x_out : nullptr;
        io.shift_out = l == m - 1 ? jb.shift_out : nullptr;
        const float freq = ldexpf(1.0f, l + 1 + k0);
        if (wv > 0) {
            const float xa = l == 0 ? fwd_fetch_x(io, base0, lane, wv - 1) : xs[4 * lane + wv - 1];
            fwd_posenc(xa, freq, lane, wv - 1, pe, xs, l == 0);
        }
        __syncthreads();
        fwd_tile_core(hc, fw, io, base0, sm, pe);
        if (wv == 0) fwd_warp(hc, io, base0, lane, ho, pe, xs);
        else if (two) {                                             // second tile's encoding while wave 0 warps the first
            const float xa = l == 0 ? fwd_fetch_x(io, base0 + NDP_TILE, lane, wv - 1) : xs[64 * 4 + 4 * lane + wv - 1];
            fwd_posenc(xa, freq, lane, wv - 1, pe + 64 * 9, xs + 64 * 4, l == 0);
        }
        __syncthreads();
        if (two) {
            fwd_tile_core(hc, fw, io, base0 + NDP_TILE, sm, pe + 64 * 9);
            if (wv == 0) fwd_warp(hc, io, base0 + NDP_TILE, lane, ho, pe + 64 * 9, xs + 64 * 4);
            __syncthreads();
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Level backward (autograd of nets.py:111-140 wrt the level's parameters), split by layer so that each
// kernel keeps only ONE 128x128 weight slice + ONE 128x128 gradient accumulator in registers
// (<= 256 VGPR+AGPR per lane => two workgroups per CU, whose load / VALU / MFMA phases overlap):
//   bwd2: dO -> dz2 = (dO Wh) * [h2>0] ; dWh += dO^T h2 ; dbh ; dW2 += dz2^T h1 ; db2 ; dh1 = dz2 W2 ;
//         dz1 = dh1 * [h1>0]  -> written over the (now dead) h2 plane of the activation store
//   bwd1: dW1 += dz1^T h0 ; db1 ; dh0 = dz1 W1 ; dz0 = dh0 * [h0>0] ; [dW0 | db0] += dz0^T [pe | 1]
// The per-point head backward (dO) is done before, one thread per point (k_head_bwd / k_eng_loss).
//
// LDS tiles of the backward are filled by LDS-DMA (global_load_lds_dwordx4: wave-uniform LDS base + 16 B x lane, so one
// instruction lays down 1 KiB = two consecutive rows of the [64][128] tile, contiguously).  The image is therefore padded
// per ROW PAIR, not per row:   float index of (row r, column c) = 260 (r >> 1) + 128 (r & 1) + c
// (16 B of pad after every 1 KiB block).  Everything stays base + immediate (an XOR swizzle of the 16-byte chunks needs a
// VGPR per address and spilled), the 16-lane groups of a ds_read_b128 over 16 rows hit 8 distinct 16-B slots (2-way, noise
// next to 64-cycle MFMAs), and the b32 operand reads of one row are conflict-free.  No staging registers (the register-
// staged loads had started to serialise -- one load in flight at a time -- once the head stage's accumulators moved into
// bwd2 at the 256-register cap), no ds_write pass, and the global side is perfectly linear: lane l of block q reads
// src + 1 KiB q + 16 B l.
// ------------------------------------------------------------------------------------------------
#define BP_PAIR 260                       /* floats per row pair: 2 x 128 + 4 pad */
#define BP_TILE (32 * BP_PAIR)            /* floats per [64][128] tile image */
#define NDP_PES 74                        /* posenc row stride in bwd1: banks 10 c + 4 lk never collide for c < 6, lk < 2 */
enum : int {
    LB_BUFA = 0,
    LB_BUFB = LB_BUFA + BP_TILE,
    LB_DO = LB_BUFB + BP_TILE,            // [64][17] (stride 17: conflict-free MFMA operand reads over the points)
    LB_PE = LB_DO + 64 * 17,              // [6][NDP_PES] posenc rows (bwd1)
    LB_WH = LB_DO + 64 * 17,              // [NDP_WHROWS][128] head matrix, rows >= nh zero (bwd2; shares the posenc slot of bwd1)
    LB_TOTAL = LB_WH + NDP_WHROWS * NDP_W
};
static_assert(6 * NDP_PES <= NDP_WHROWS * NDP_W, "posenc rows must fit the shared slot");
// bwd1 with the input gradient (DX): W0 [128][6] in the dO slot (bwd1 stages no dO), and behind the posenc rows the partial
// sums of dpe = dz0 . W0 over either half of the outputs, [half][channel][point]
#define LB1_DPE (LB_PE + 448)
static_assert(NDP_W * 6 <= 64 * 17, "W0 must fit the dO slot");
static_assert(6 * NDP_PES <= 448 && 448 + 2 * 6 * 64 <= NDP_WHROWS * NDP_W, "dpe partials must fit behind the posenc rows");
static constexpr int kSmemBwdBytes = LB_TOTAL * 4;       // 77.1 KB: two workgroups per CU
static_assert(2 * kSmemBwdBytes <= 160 * 1024, "backward LDS carve must allow two workgroups per CU");

struct BwdJob {
    const float *params;
    float *act;             // [3][plane][128]; plane 2 (h2) is overwritten with dz1 by bwd2
    const float *heads;     // [plane][NDP_HROW]
    const float *dO;        // [plane][16]
    float *gpart;           // this workgroup's partial [P]
    int n, plane, n_tiles, tile0, tile_step;
    // layer-generic view used by bwd2 (the NDP callers derive it from `act`; the NSFP chain walks its 8 planes):
    float *dz_plane;        // [plane][128] gradient wrt the layer's pre-activation, rewritten in place for the layer below
    const float *h_plane;   // [plane][128] the layer's input activation (post-ReLU)
    int w_off, b_off;       // offsets of the layer's weight / bias inside params and inside the partial
    int from_dO, wh_off, nh; // bwd2: recompute dz from dO through the nh head rows at params + wh_off (else: read dz_plane)
};

// NDP level: which slice of the flat parameter block the two generic backward stages work on
__host__ __device__ inline void bwd_job_ndp_layer2(BwdJob &job, int nh) {
    const ndp_layer_desc dd = {NDP_W, 2, 0, 0, 0, 0.f};
    job.w_off = ndp_off_Wi(&dd, 2); job.b_off = ndp_off_bi(&dd, 2);
    job.from_dO = 1; job.wh_off = ndp_off_Wi(&dd, 3); job.nh = nh;
}

// [64][128] tile: global -> padded LDS tile through registers (NSFP forward layers; the backward uses LDS-DMA)
__device__ __forceinline__ void load_tile_to_lds(const float *src /*[64][128] global*/, float *dst /*LDS [64][LD]*/) {
    const int t = threadIdx.x;
    float4 v[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) v[i] = reinterpret_cast<const float4 *>(src)[t + 256 * i];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int idx = t + 256 * i;           // float4 index 0..2047
        *reinterpret_cast<float4 *>(dst + (idx >> 5) * NDP_LD + 4 * (idx & 31)) = v[i];
    }
}

__device__ __forceinline__ int bp_row(int r) { return BP_PAIR * (r >> 1) + NDP_W * (r & 1); }

// [64][128] tile: global -> LDS image by LDS-DMA, 8 x 1 KiB per wave (one row pair per instruction), asynchronous:
// the caller waits with glds_wait() before the barrier that publishes the tile.
__device__ __forceinline__ void glds_tile(const float *src /*global [64][128]*/, float *dst /*LDS image*/) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const int q = 8 * wv + i;                                  // row pair
        __builtin_amdgcn_global_load_lds(
            (const __attribute__((address_space(1))) void *)(src + 2 * NDP_W * q + 4 * lane),
            (__attribute__((address_space(3))) void *)(dst + BP_PAIR * q), 16, 0, 0);
    }
}
__device__ __forceinline__ void glds_wait() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }

// tile_gemm_64x32 over an LDS-DMA tile image
__device__ __forceinline__ void tile_gemm_64x32_sw(const float *in /*LDS image*/, const float (&w)[64],
                                                   int l31, int h, f32x16 &acc0, f32x16 &acc1) {
    const float *r0 = in + bp_row(l31) + 64 * h;
    const float *r1 = r0 + 16 * BP_PAIR;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float4 a0 = *reinterpret_cast<const float4 *>(r0 + 4 * i);
        const float4 a1 = *reinterpret_cast<const float4 *>(r1 + 4 * i);
        acc0 = MFMA32(w[4 * i], a0.x, acc0);     acc1 = MFMA32(w[4 * i], a1.x, acc1);
        acc0 = MFMA32(w[4 * i + 1], a0.y, acc0); acc1 = MFMA32(w[4 * i + 1], a1.y, acc1);
        acc0 = MFMA32(w[4 * i + 2], a0.z, acc0); acc1 = MFMA32(w[4 * i + 2], a1.z, acc1);
        acc0 = MFMA32(w[4 * i + 3], a0.w, acc0); acc1 = MFMA32(w[4 * i + 3], a1.w, acc1);
        if ((i & 3) == 3) asm volatile("" ::: "memory");
    }
}

// backward epilogue of tile_gemm_64x32_sw: z = d * [hmask > 0] -> zout (same tile coordinates), b128 reads and writes
__device__ __forceinline__ void epilogue_mask_sw(const f32x16 &d0, const f32x16 &d1, const float *hmask /*LDS*/,
                                                 float *zout /*LDS*/, int wv, int l31, int h) {
    const int off = bp_row(l31) + 32 * wv + 4 * h;
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        const float4 m0 = *reinterpret_cast<const float4 *>(hmask + off + 8 * g);
        const float4 m1 = *reinterpret_cast<const float4 *>(hmask + off + 16 * BP_PAIR + 8 * g);
        *reinterpret_cast<float4 *>(zout + off + 8 * g) =
            make_float4(m0.x > 0.f ? d0[4 * g] : 0.f, m0.y > 0.f ? d0[4 * g + 1] : 0.f,
                        m0.z > 0.f ? d0[4 * g + 2] : 0.f, m0.w > 0.f ? d0[4 * g + 3] : 0.f);
        *reinterpret_cast<float4 *>(zout + off + 16 * BP_PAIR + 8 * g) =
            make_float4(m1.x > 0.f ? d1[4 * g] : 0.f, m1.y > 0.f ? d1[4 * g + 1] : 0.f,
                        m1.z > 0.f ? d1[4 * g + 2] : 0.f, m1.w > 0.f ? d1[4 * g + 3] : 0.f);
    }
}

// [64][128] tile: LDS image -> global, 8 float4 per thread, fully coalesced (thread t: rows (t >> 5) + 8i)
__device__ __forceinline__ void store_tile_from_lds_sw(const float *src /*LDS image*/, float *dst /*global [64][128]*/) {
    const int t = threadIdx.x;
    const float *s0 = src + bp_row(t >> 5) + 4 * (t & 31);
#pragma unroll
    for (int i = 0; i < 8; ++i)
        reinterpret_cast<float4 *>(dst)[t + 256 * i] = *reinterpret_cast<const float4 *>(s0 + 4 * BP_PAIR * i);
}

// dW[mt] += dz^T h   (rows o = 32*mt.., cols k = 32wv + l31), contraction over the tile's 64 points: A = dz[p][l31 + 32m],
// B = h[p][32wv + l31], both conflict-free b32 reads of one row.
// (A variant with the dW rows permuted so that one ds_read_b128 feeds all four A operands, software-pipelined by
//  hand, measured SLOWER: bwd1 0.214 ms against 0.180 ms -- the compiler's own schedule of the b32 reads wins.)
// COLSUM: the A operands are dz[p][l31 + 32m] for the 32 points of this lane's half -- adding them up as they pass gives
// the column sums of dz (the layer's bias gradient) on the idle VALU: cs[m] += dz[32h .. 32h+31][l31 + 32m].
template <bool COLSUM>
__device__ __forceinline__ void tile_outer_128x32_sw(const float *dz /*LDS image*/, const float *hin /*LDS image*/,
                                                     int wv, int l31, int h, f32x16 (&dW)[4], float (&cs)[4]) {
#pragma unroll 2
    for (int ks = 0; ks < 32; ++ks) {
        const int ro = 16 * BP_PAIR * h + bp_row(ks);                // row p = 32h + ks
        const float b = hin[ro + 32 * wv + l31];
        const float *dr = dz + ro + l31;
        const float a0 = dr[0], a1 = dr[32], a2 = dr[64], a3 = dr[96];
        dW[0] = MFMA32(a0, b, dW[0]);
        dW[1] = MFMA32(a1, b, dW[1]);
        dW[2] = MFMA32(a2, b, dW[2]);
        dW[3] = MFMA32(a3, b, dW[3]);
        if (COLSUM) { cs[0] += a0; cs[1] += a1; cs[2] += a2; cs[3] += a3; }
    }
}
// fold the two half-tile partials of tile_outer_128x32_sw<true> (taken from wave 0) -> out[128]   (sc: >= 256 floats of LDS)
__device__ __forceinline__ void outer_colsum_finish(const float (&cs)[4], float *sc, float *out) {
    const int t = threadIdx.x;
    __syncthreads();
    if (t < 64) {
#pragma unroll
        for (int m = 0; m < 4; ++m) sc[(t >> 5) * NDP_W + 32 * m + (t & 31)] = cs[m];
    }
    __syncthreads();
    if (t < NDP_W) out[t] = sc[t] + sc[NDP_W + t];
}

__device__ __forceinline__ void store_dW(float *g, const f32x16 (&dW)[4], int wv, int l31, int h) {
    const int col = 32 * wv + l31;
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) g[(32 * m + mfma_row(r, h)) * NDP_W + col] = dW[m][r];
}

// point of (k-step ks, lane group lk) in the 16x16x4 MFMA stages that contract over a tile's 64 points: rows 4 apart
// are 8 banks apart in the tile image, so the b32 B reads of a 32-lane group collide 2-way at worst
__device__ __forceinline__ int mfma16_point(int ks, int lk) { return 16 * (ks >> 2) + 4 * lk + (ks & 3); }

// hidden layer l: dW_l += dz_l^T h_{l-1} ; db_l ; dh_{l-1} = dz_l W_l ; dz_{l-1} = dh_{l-1} * [h_{l-1} > 0] written over dz_l.
// job.from_dO: l is the layer right below the heads.  Its dz = (dO Wh) * [h > 0] is computed here from dO (K = 16: eight
// k-steps) over the activation tile, in place -- never stored to HBM -- and the head stage of the backward rides along:
// dWh += dO^T h on the 16x16x4 MFMA (before h is overwritten), dbh from the registers that carry dO.
// (Round 1 had a separate head kernel that read the whole h plane a second time.)
__device__ __forceinline__ void bwd2_body(const HeadCfg &hc, const BwdJob &job, float *sm) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int l15 = lane & 15, lk = lane >> 4;
    float *bufA = sm + LB_BUFA, *bufB = sm + LB_BUFB;
    const float *W2 = job.params + job.w_off;
    float w2t[64];
    load_w_bwd(W2, sm + LB_BUFA, wv, l31, h, w2t);
    f32x16 dW2[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) dW2[m][r] = 0.f;
    float gb2[4] = {0.f, 0.f, 0.f, 0.f};            // db of this layer: column sums of dz, taken inside the dW outer product
    float *dOs = sm + LB_DO, *whs = sm + LB_WH;
    // head matrix (the MFMA A operand of dz = dO Wh) staged in LDS once: 8 registers through the GEMM phases were the
    // difference between spilling and not
    if (job.from_dO)
        for (int i = t; i < NDP_WHROWS * NDP_W; i += 256) whs[i] = i < job.nh * NDP_W ? job.params[job.wh_off + i] : 0.f;
    f32x4 gWha, gWhb;                               // dWh[j = 4lk + r][k = 32wv + l15 (a) / + 16 (b)]
#pragma unroll
    for (int r = 0; r < 4; ++r) { gWha[r] = 0.f; gWhb[r] = 0.f; }
    float4 gbh = make_float4(0.f, 0.f, 0.f, 0.f);   // partial sums of dO[.][4(t&3) ..]
    // the input-activation tile (bufA) of tile i+1 is requested as soon as tile i is done with it, under tile i's store
    if (job.tile0 < job.n_tiles) glds_tile(job.h_plane + (size_t)job.tile0 * NDP_TILE * NDP_W, bufA);
    for (int tile = job.tile0; tile < job.n_tiles; tile += job.tile_step) {
        const int base = tile * NDP_TILE;
        float *plane2 = job.dz_plane + (size_t)base * NDP_W;
        PT_DECL;
        glds_tile(plane2, bufB);                                                    // h (becomes dz below), or dz
        if (job.from_dO) {
            const float4 dv = reinterpret_cast<const float4 *>(job.dO + (size_t)base * NDP_NHMAX)[t];
            float *dr = dOs + (t >> 2) * 17 + 4 * (t & 3);
            dr[0] = dv.x; dr[1] = dv.y; dr[2] = dv.z; dr[3] = dv.w;
            gbh.x += dv.x; gbh.y += dv.y; gbh.z += dv.z; gbh.w += dv.w;
            glds_wait();
            __syncthreads();
            {   // dWh += dO^T h over the tile's 64 points (16 k-steps x two 16-column blocks of this wave's slab)
#pragma unroll 4
                for (int ks = 0; ks < 16; ++ks) {
                    const int p = mfma16_point(ks, lk);
                    const float a = dOs[p * 17 + l15];
                    const float *br = bufB + bp_row(p) + 32 * wv + l15;
                    const float b0 = br[0], b1 = br[16];
                    gWha = MFMA16(a, b0, gWha);
                    gWhb = MFMA16(a, b1, gWhb);
                }
            }
            f32x16 z0, z1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { z0[r] = 0.f; z1[r] = 0.f; }
#pragma unroll
            for (int ks = 0; ks < NDP_WHROWS / 2; ++ks) {                         // head rows j = 2ks + h < 12 (at most 11 exist)
                const float a = whs[(2 * ks + h) * NDP_W + 32 * wv + l31];
                const float b0 = dOs[l31 * 17 + 2 * ks + h], b1 = dOs[(l31 + 32) * 17 + 2 * ks + h];
                z0 = MFMA32(a, b0, z0);
                z1 = MFMA32(a, b1, z1);
            }
            epilogue_mask_sw(z0, z1, bufB, bufB, wv, l31, h);                       // own 32-column slab, in place
        } else {
            glds_wait();
        }
        PT(0);
        __syncthreads();
        PT(1);
        {
            f32x16 d0, d1;
#pragma unroll
            for (int r = 0; r < 16; ++r) { d0[r] = 0.f; d1[r] = 0.f; }
            tile_outer_128x32_sw<true>(bufB, bufA, wv, l31, h, dW2, gb2);
            tile_gemm_64x32_sw(bufB, w2t, l31, h, d0, d1);
            PT(2);
            __syncthreads();                       // every wave is done reading dz2
            PT(3);
            // dz1 goes through LDS so that HBM sees coalesced float4 rows (and the epilogue needs one base
            // address instead of 32 per-element addresses, which used to cost 58 spilled registers)
            epilogue_mask_sw(d0, d1, bufA, bufB, wv, l31, h);
        }
        PT(4);
        __syncthreads();
        PT(5);
        // bufA (the mask of the epilogue above) is dead from here: the next tile's copy starts now, under the store
        if (tile + job.tile_step < job.n_tiles)
            glds_tile(job.h_plane + (size_t)(tile + job.tile_step) * NDP_TILE * NDP_W, bufA);
        store_tile_from_lds_sw(bufB, plane2);
        PT(6);
        __syncthreads();
        PT(7);
    }
    float *G = job.gpart;
    store_dW(G + job.w_off, dW2, wv, l31, h);
    outer_colsum_finish(gb2, sm + LB_BUFA, G + job.b_off);
    if (!job.from_dO) return;
    // ---- head stage results: dWh rows j < nh, dbh
    float *gwh = G + job.wh_off;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int j = 4 * lk + r;
        if (j < job.nh) {
            gwh[j * NDP_W + 32 * wv + l15] = gWha[r];
            gwh[j * NDP_W + 32 * wv + 16 + l15] = gWhb[r];
        }
    }
    float *sh = sm + LB_BUFB;                       // [256] float4: the dO row partials (the tiles are dead)
    reinterpret_cast<float4 *>(sh)[t] = gbh;
    __syncthreads();
    if (t < job.nh) {
        float s = sh[t];                                                          // thread 4q + (j >> 2), component j & 3
#pragma unroll 8
        for (int q = 1; q < 64; ++q) s += sh[4 * (4 * q + (t >> 2)) + (t & 3)];
        gwh[job.nh * NDP_W + t] = s;
    }
}

// hidden layer 1 and the input layer: dW1 += dz1^T h0 ; db1 ; dh0 = dz1 W1 ; dz0 = dh0 * [h0 > 0] ;
// [dW0 | db0]^T += [pe | 1]^T dz0 (16x16x4 MFMA: rows = the 6 posenc channels and a row of ones, columns = this wave's 32 outputs)
// DX (the stand-alone operator when dL/dx is asked for; the engine's samples are detached): after the dW0 stage
//   dpe[p][c] = sum_o dz0[p][o] W0[o][c] ;  dx[p][k] += freq (pe[2k+1][p] dpe[p][2k] - pe[2k][p] dpe[p][2k+1])
// (pe = [sin, cos] per axis; dx holds the direct term of k_head_bwd_dx).  The contraction is 64 x 6 x 128 per tile next to
// 2 x 64 x 128 x 128 on the matrix pipe, so it runs as fmaf chains on the VALU, which idles under the MFMA stages: for point
// p = lane, wave w sums half w & 1 of the outputs (o ascending) for the channels 3 (w >> 1) .. + 2; the halves are then added, lower
// first.  A tile belongs to one workgroup and a point to one thread: plain read-modify-write in a fixed order, independent of the grid.
template <bool DX = false>
__device__ __forceinline__ void bwd1_body(const HeadCfg &hc, const BwdJob &job, float *sm, float *dx = nullptr, float freq = 0.f) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    const int l15 = lane & 15, lk = lane >> 4;
    float *bufA = sm + LB_BUFA, *bufB = sm + LB_BUFB, *pe = sm + LB_PE;
    const ndp_layer_desc dd = {NDP_W, 2, hc.motion, hc.rotfmt, 0, hc.mlp_scale};
    const float *W1 = job.params + ndp_off_Wi(&dd, 1);
    float w1t[64];
    load_w_bwd(W1, sm + LB_BUFA, wv, l31, h, w1t);
    f32x16 dW1[4];
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int r = 0; r < 16; ++r) dW1[m][r] = 0.f;
    f32x4 gW0a, gW0b;                              // [dW0 | db0]^T[c][o]: c = 4*lk + r (c = 6: db0), o = 32wv + l15 (a) / + 16 (b)
#pragma unroll
    for (int r = 0; r < 4; ++r) { gW0a[r] = 0.f; gW0b[r] = 0.f; }
    float gb1[4] = {0.f, 0.f, 0.f, 0.f};
    if (DX) {                                      // (published by the first barrier of the tile loop)
        const float *W0 = job.params + ndp_off_W0(&dd);
        for (int i = t; i < NDP_W * 6; i += 256) sm[LB_DO + i] = W0[i];
    }

    // the h0 tile (bufA) of tile i+1 is requested as soon as tile i is done with it, under tile i's dW0 stage
    if (job.tile0 < job.n_tiles) glds_tile(job.act + (size_t)job.tile0 * NDP_TILE * NDP_W, bufA);
    for (int tile = job.tile0; tile < job.n_tiles; tile += job.tile_step) {
        const int base = tile * NDP_TILE;
        PT_DECL;
        // ---- dz1 tile -> bufB (LDS-DMA), posenc -> pe
        glds_tile(job.act + (2 * (size_t)job.plane + base) * NDP_W, bufB);
        if (t < 64) {
            const float *hr = job.heads + (size_t)(base + t) * NDP_HROW;
            const float4 pa = *reinterpret_cast<const float4 *>(hr + 16);
            const float4 pb = *reinterpret_cast<const float4 *>(hr + 20);
            pe[t] = pa.x; pe[NDP_PES + t] = pa.y; pe[2 * NDP_PES + t] = pa.z; pe[3 * NDP_PES + t] = pa.w;
            pe[4 * NDP_PES + t] = pb.x; pe[5 * NDP_PES + t] = pb.y;
        }
        glds_wait();
        PT(0);
        __syncthreads();
        PT(1);
        // ---- dW1 += dz1^T h0 (+ db1) ; dh0 = dz1 W1
        f32x16 d0, d1;
        {
#pragma unroll
            for (int r = 0; r < 16; ++r) { d0[r] = 0.f; d1[r] = 0.f; }
            tile_outer_128x32_sw<true>(bufB, bufA, wv, l31, h, dW1, gb1);
            tile_gemm_64x32_sw(bufB, w1t, l31, h, d0, d1);
        }
        PT(2);
        __syncthreads();
        PT(3);
        // ---- dz0 = dh0 * [h0 > 0] -> bufB
        epilogue_mask_sw(d0, d1, bufA, bufB, wv, l31, h);
        PT(4);
        __syncthreads();
        PT(5);
        // bufA (h0: the mask of the epilogue above) is dead from here: the next tile's h0 arrives under the dW0 stage
        if (tile + job.tile_step < job.n_tiles)
            glds_tile(job.act + (size_t)(tile + job.tile_step) * NDP_TILE * NDP_W, bufA);
        // ---- [dW0 | db0]^T += [pe | 1]^T dz0 on the 16x16x4 MFMA: A[c][p] = pe[c][p] (c < 6), 1 (c = 6), B[p][o] = dz0[p][o]
        {
            const float *ap = pe + (l15 < 6 ? l15 : 0) * NDP_PES;
#pragma unroll 4
            for (int ks = 0; ks < 16; ++ks) {
                const int p = mfma16_point(ks, lk);
                float a = ap[p];
                if (l15 >= 6) a = l15 == 6 ? 1.0f : 0.f;
                const float *br = bufB + bp_row(p) + 32 * wv + l15;
                const float b0 = br[0], b1 = br[16];
                gW0a = MFMA16(a, b0, gW0a);
                gW0b = MFMA16(a, b1, gW0b);
            }
        }
        if (DX) {
            float *dpe = sm + LB1_DPE;
            {
                const int oh = wv & 1, c0 = 3 * (wv >> 1);
                const float *zr = bufB + bp_row(lane) + 64 * oh;                  // dz0[p = lane][64 oh ..]
                const float *wq = sm + LB_DO + 6 * 64 * oh + c0;                  // W0[64 oh ..][c0 ..]: wave-uniform (broadcast) reads
                float s0 = 0.f, s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const float4 z4 = *reinterpret_cast<const float4 *>(zr + 4 * i);
                    const float z[4] = {z4.x, z4.y, z4.z, z4.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const float *w = wq + 6 * (4 * i + j);
                        s0 = fmaf(z[j], w[0], s0); s1 = fmaf(z[j], w[1], s1); s2 = fmaf(z[j], w[2], s2);
                    }
                }
                float *dq = dpe + (6 * oh + c0) * 64 + lane;
                dq[0] = s0; dq[64] = s1; dq[128] = s2;
            }
            __syncthreads();
            if (wv < 3 && base + lane < job.n) {                                  // wave k: axis k of the tile's points
                const float *ds = dpe + (2 * wv) * 64 + lane, *dc = ds + 64;
                const float dsin = ds[0] + ds[6 * 64], dcos = dc[0] + dc[6 * 64];
                const float sn = pe[2 * wv * NDP_PES + lane], cs = pe[(2 * wv + 1) * NDP_PES + lane];
                float *q = dx + (size_t)(base + lane) * 3 + wv;
                *q += freq * (cs * dsin - sn * dcos);
            }
        }
        PT(6);
        __syncthreads();
        PT(7);
    }
    float *G = job.gpart;
    store_dW(G + ndp_off_Wi(&dd, 1), dW1, wv, l31, h);
    {   // dW0[o][c] (c < 6) and db0[o] (c = 6): lane holds c = 4*lk + r for its two columns
        float *gw0 = G + ndp_off_W0(&dd), *gb0 = G + ndp_off_b0(&dd);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int c = 4 * lk + r;
            if (c < 6) {
                gw0[(32 * wv + l15) * 6 + c] = gW0a[r];
                gw0[(32 * wv + 16 + l15) * 6 + c] = gW0b[r];
            } else if (c == 6) {
                gb0[32 * wv + l15] = gW0a[r];
                gb0[32 * wv + 16 + l15] = gW0b[r];
            }
        }
    }
    outer_colsum_finish(gb1, sm + LB_BUFA, G + ndp_off_bi(&dd, 1));
}

// ------------------------------------------------------------------------------------------------
// standalone kernels
// ------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(256, 2)
k_level_fwd(HeadCfg hc, LevelJob job) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    level_fwd_body(hc, job, sm);
}

extern "C" __global__ void __launch_bounds__(256, 2)
k_level_bwd2(HeadCfg hc, BwdJob job, int p_stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    job.gpart += (size_t)blockIdx.x * p_stride;
    bwd2_body(hc, job, sm);
}

extern "C" __global__ void __launch_bounds__(256, 2)
k_level_bwd1(HeadCfg hc, BwdJob job, int p_stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    job.gpart += (size_t)blockIdx.x * p_stride;
    bwd1_body(hc, job, sm);
}

// k_level_bwd1 that also adds the part of dL/dx that passes through the network to dx [n][3] (ndp_level_bwd with dx)
extern "C" __global__ void __launch_bounds__(256, 2)
k_level_bwd1_dx(HeadCfg hc, BwdJob job, int p_stride, float *dx, float freq) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    job.gpart += (size_t)blockIdx.x * p_stride;
    bwd1_body<true>(hc, job, sm, dx, freq);
}

// dO[p][16] = mlp_scale * dL/d(scaled head outputs) for p < n, zero rows up to `plane`
// DX: dx[p][3] = the direct part of dL/dx (head_warp_bwd) as well
template <bool DX>
__device__ __forceinline__ void head_bwd_body(const HeadCfg &hc, const float *x, const float *heads, const float *g, const float *g_nr,
                                              int n, int plane, float *dO, float *dx, float *rows) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= plane) return;
    float *out = dO + (size_t)p * NDP_NHMAX;
    if (p < n) {
        const float xv[3] = {x[3 * p], x[3 * p + 1], x[3 * p + 2]};
        const float gv[3] = {g[3 * p], g[3 * p + 1], g[3 * p + 2]};
        if (DX) {
            float dv[3];
            point_head_bwd(hc, heads + (size_t)p * NDP_HROW, xv, gv, g_nr ? g_nr[p] : 0.f, rows + threadIdx.x * NDP_NHMAX, out, nullptr, dv);
            dx[3 * p] = dv[0]; dx[3 * p + 1] = dv[1]; dx[3 * p + 2] = dv[2];
        } else {
            point_head_bwd(hc, heads + (size_t)p * NDP_HROW, xv, gv, g_nr ? g_nr[p] : 0.f, rows + threadIdx.x * NDP_NHMAX, out);
        }
    } else {
#pragma unroll
        for (int j = 0; j < NDP_NHMAX; j += 4) *reinterpret_cast<float4 *>(out + j) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}
extern "C" __global__ void __launch_bounds__(256)
k_head_bwd(HeadCfg hc, const float *x, const float *heads, const float *g, const float *g_nr, int n, int plane, float *dO) {
    __shared__ __attribute__((aligned(16))) float rows[256 * NDP_NHMAX];
    head_bwd_body<false>(hc, x, heads, g, g_nr, n, plane, dO, nullptr, rows);
}
extern "C" __global__ void __launch_bounds__(256)
k_head_bwd_dx(HeadCfg hc, const float *x, const float *heads, const float *g, const float *g_nr, int n, int plane, float *dO, float *dx) {
    __shared__ __attribute__((aligned(16))) float rows[256 * NDP_NHMAX];
    head_bwd_body<true>(hc, x, heads, g, g_nr, n, plane, dO, dx, rows);
}

extern "C" __global__ void k_grad_reduce(const float *gpart, int n_part, int p_stride, int P, float *grads) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= P) return;
    float s = gpart[i];
    for (int g = 1; g < n_part; ++g) s += gpart[(size_t)g * p_stride + i];
    grads[i] = s;
}
