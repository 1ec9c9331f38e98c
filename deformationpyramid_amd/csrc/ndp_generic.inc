// ndp_generic.inc -- the level kernels for every `width` / `depth` the YAML can name EXCEPT the shipped 128 / 3 (round 6).
//
// The reference builds any NDPLayer(depth, width) (model/nets.py:65-110: Linear(6, width), MLP of depth - 1 Linear(width, width) +
// ReLU at :295-304, the head branches); both shipped configurations use 128 / 3, which is what the MFMA kernels of this library are
// specialised for.  These kernels serve the rest of the surface -- 1 <= width <= 256, depth 1..4 (the oracle's own limits,
// oracle/ndp_oracle.c:20,238) -- behind the same entry points (ndp_level_fwd / ndp_level_bwd / ndp_pyramid_fwd* / ndp_engine_run), in
// fp32 on the fp32 matrix instruction (v_mfma_f32_32x32x2_f32: exact fp32 products, fp32 accumulation, contraction index ascending):
//   * a 64-point tile's activations are [feature][point] rows in LDS (stride 65), written and read by every stage in that layout;
//   * forward : out[o][p] = act(b[o] + sum_k W[o][k] in[k][p]) per 32-output block and wave: A = a lane's weight W[o][2s + h] straight
//               from global (each weight is read once per wave and tile), B = in[2s + h][p] for either half of the points, the bias as
//               the accumulators' first step -- the oracle's chain (bias, then k ascending: ndp_oracle.c:252-271) two k's at a time;
//   * backward: dh[k][p] = sum_o dz[o][p] W[o][k] the same way with the roles of k and o exchanged (the lanes' weight reads are then
//               contiguous); gW[o][k] = sum_p dz[o][p] h[k][p] per 32 x 32 block with BOTH operands out of the LDS rows, 32 steps over
//               the tile's points, added to the workgroup's partial by the element's one owner lane (deterministic; the oracle adds
//               point by point: same terms, another association -- compared at 1e-4 relative like the MFMA kernels of 128 / 3).
// A correctness path first (the first version ran these sums on the vector pipe with wave-uniform weights by scalar loads: 1 / 10 of the
// 128 / 3 kernels' rate, its weight gradients bound by LDS reads -- five per four FMAs; here two LDS reads feed 2048).
// Activation store of this path: [n_hidden + 1][plane][width] fp32 row-major (plane l = output of layer l, post-ReLU).
#define GEN_PS 65                       /* LDS floats between two features of a tile (64 points + 1) */
#define GEN_WMAX 256
#define GEN_HMAX 3                      /* n_hidden <= 3, i.e. depth <= 4 (oracle/ndp_oracle.c:238) */

__host__ __device__ inline bool gen_is_generic(const ndp_layer_desc &d) { return d.width != NDP_W || d.n_hidden != 2; }
__host__ __device__ inline bool gen_supported(const ndp_layer_desc &d) {
    return d.width >= 1 && d.width <= GEN_WMAX && d.n_hidden >= 0 && d.n_hidden <= GEN_HMAX;
}
// LDS carve (floats) of the forward: two activation buffers (each rounded up to 16 bytes: the rows behind them are read as float4 for any
// width), then the pe / xs double buffers and the head outputs the shared warp reads
__host__ __device__ inline int gen_buf(int W) { return (W * GEN_PS + 3) & ~3; }
__host__ __device__ inline int gen_fwd_pe(int W) { return 2 * gen_buf(W); }
__host__ __device__ inline int gen_fwd_xs(int W) { return gen_fwd_pe(W) + 2 * 64 * 9; }
__host__ __device__ inline int gen_fwd_ho(int W) { return gen_fwd_xs(W) + 2 * 64 * 4; }
__host__ __device__ inline int gen_fwd_floats(int W) { return gen_fwd_ho(W) + 64 * NDP_NHMAX; }
// ... of the backward: gradient buffer D, activation buffer I, dO rows [16][65], encodings [6][65]
__host__ __device__ inline int gen_bwd_do(int W) { return 2 * gen_buf(W); }
__host__ __device__ inline int gen_bwd_pe(int W) { return gen_bwd_do(W) + NDP_NHMAX * GEN_PS; }
__host__ __device__ inline int gen_bwd_floats(int W) { return gen_bwd_pe(W) + 6 * GEN_PS; }
static constexpr int kSmemGenFwdMax = (2 * GEN_WMAX * GEN_PS + 2 * 64 * 9 + 2 * 64 * 4 + 64 * NDP_NHMAX) * 4;
static constexpr int kSmemGenBwdMax = (2 * GEN_WMAX * GEN_PS + NDP_NHMAX * GEN_PS + 6 * GEN_PS) * 4;
static_assert(kSmemGenFwdMax <= 160 * 1024 && kSmemGenBwdMax <= 160 * 1024, "generic level kernels: LDS carve");

// out[o] (o < n_out) of the tile's 64 points = act(b[o] + sum_k W[o][k] in[k]), k ascending from the bias.
// in : value k of point p at in[k * in_ks + p * in_ps];  out: feature o of point p at out[o * out_os + p * out_ps].
// RELU: max(., 0) as `acc > 0 ? acc : 0`; else the value times `scale` (the heads' mlp_scale, nets.py:117).
// A wave takes the 32-output blocks ob = 32 wv, 32 wv + 128, ..; lane (l31, h): A = W[ob + l31][2 s + h], B = in[2 s + h][l31 (+ 32)].
template <bool RELU>
__device__ __forceinline__ void gen_dense(const float *Wm, const float *bv, int n_out, int n_in, const float *in, int in_ks, int in_ps,
                                          float *out, int out_os, int out_ps, float scale) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
    for (int ob = 32 * wv; ob < n_out; ob += 128) {
        const int o = ob + l31 < n_out ? ob + l31 : n_out - 1;       // (rows beyond n_out: computed from the last row, never stored)
        f32x16 acc0, acc1;
        acc_init_bias(bv[o], h, acc0, acc1);
        const float *wr = Wm + (size_t)o * n_in + h;
        const float *i0 = in + h * in_ks + l31 * in_ps, *i1 = i0 + 32 * in_ps;
        const int n2 = n_in & ~1;
#pragma unroll 8
        for (int k = 0; k < n2; k += 2) {
            const float a = wr[k];
            acc0 = MFMA32(a, i0[k * in_ks], acc0);
            acc1 = MFMA32(a, i1[k * in_ks], acc1);
        }
        if (n_in & 1) {                                              // odd contraction length: the last step's second slot is empty
            const float a = h == 0 ? wr[n2] : 0.f, b0 = h == 0 ? i0[n2 * in_ks] : 0.f, b1 = h == 0 ? i1[n2 * in_ks] : 0.f;
            acc0 = MFMA32(a, b0, acc0);
            acc1 = MFMA32(a, b1, acc1);
        }
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int orow = ob + mfma_row(r, h);
            if (orow < n_out) {
                float *q = out + orow * out_os + l31 * out_ps;
                q[0] = RELU ? (acc0[r] > 0.f ? acc0[r] : 0.f) : scale * acc0[r];
                q[32 * out_ps] = RELU ? (acc1[r] > 0.f ? acc1[r] : 0.f) : scale * acc1[r];
            }
        }
    }
}
// a tile's [feature][point] buffer <-> its rows of a [plane][W] activation plane (global side coalesced over the features)
__device__ __forceinline__ void gen_store_plane(const float *buf, float *dst /* + base * W */, int W) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int p = wv; p < 64; p += 4)
        for (int o = lane; o < W; o += 64) dst[p * W + o] = buf[o * GEN_PS + p];
}
__device__ __forceinline__ void gen_load_plane(float *buf, const float *src /* + base * W */, int W) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int p = wv; p < 64; p += 4)
        for (int o = lane; o < W; o += 64) buf[o * GEN_PS + p] = src[p * W + o];
}

// One 64-point tile from its positional encoding to the scaled head outputs (ho [64][16], rows >= nh zero); activations -> HBM.
// Ends with a barrier (the shared fwd_warp reads ho).
__device__ __forceinline__ void gen_tile_core(const HeadCfg &hc, const ndp_layer_desc &d, const float *params, const TileIO &io, int base,
                                              float *sm, const float *pe) {
    const int W = d.width;
    float *cur = sm, *nxt = sm + gen_buf(W), *ho = sm + gen_fwd_ho(W);
    gen_dense<true>(params + ndp_off_W0(&d), params + ndp_off_b0(&d), W, 6, pe, 1, 9, cur, GEN_PS, 1, 1.0f);
    __syncthreads();
    if (io.act) gen_store_plane(cur, io.act + (size_t)base * W, W);
    for (int l = 1; l <= d.n_hidden; ++l) {
        gen_dense<true>(params + ndp_off_Wi(&d, l), params + ndp_off_bi(&d, l), W, W, cur, GEN_PS, 1, nxt, GEN_PS, 1, 1.0f);
        __syncthreads();
        if (io.act) gen_store_plane(nxt, io.act + ((size_t)l * io.plane + base) * W, W);
        float *sw = cur; cur = nxt; nxt = sw;
    }
    gen_dense<false>(params + ndp_off_Wh(&d), params + ndp_off_bh(&d), hc.nh, W, cur, GEN_PS, 1, ho, 1, NDP_NHMAX, hc.mlp_scale);
    if (threadIdx.x < 64)
        for (int j = hc.nh; j < NDP_NHMAX; ++j) ho[threadIdx.x * NDP_NHMAX + j] = 0.f;
    __syncthreads();
}

// all tiles of a workgroup through one level (the pipeline of level_fwd_body: wave 0 warps tile i while waves 1..3 encode tile i + 1)
__device__ __forceinline__ void gen_level_fwd_body(const HeadCfg &hc, const ndp_layer_desc &d, const LevelJob &job, float *sm) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, W = d.width;
    TileIO io;
    io.x_in = job.x_in; io.shift_in = nullptr; io.x_out = job.x_out; io.shift_out = nullptr;
    io.act = job.act; io.heads = job.heads; io.nonrig = job.nonrig; io.n = job.n; io.plane = job.plane;
    float *pe = sm + gen_fwd_pe(W), *xs = sm + gen_fwd_xs(W), *ho = sm + gen_fwd_ho(W);
    int tile = job.tile0, cur = 0;
    if (tile >= job.n_tiles) return;
    if (wv > 0) fwd_posenc(fwd_fetch_x(io, tile * NDP_TILE, lane, wv - 1), job.freq, lane, wv - 1, pe, xs, true);
    __syncthreads();
    for (; tile < job.n_tiles; tile += job.tile_step) {
        const int next = tile + job.tile_step;
        float xn = 0.f;
        if (wv > 0 && next < job.n_tiles) xn = fwd_fetch_x(io, next * NDP_TILE, lane, wv - 1);
        gen_tile_core(hc, d, job.params, io, tile * NDP_TILE, sm, pe + cur * (64 * 9));
        if (wv == 0) fwd_warp(hc, io, tile * NDP_TILE, lane, ho, pe + cur * (64 * 9), xs + cur * (64 * 4));
        else if (next < job.n_tiles)
            fwd_posenc(xn, job.freq, lane, wv - 1, pe + (cur ^ 1) * (64 * 9), xs + (cur ^ 1) * (64 * 4), true);
        __syncthreads();
        cur ^= 1;
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_gen_level_fwd(HeadCfg hc, ndp_layer_desc d, LevelJob job) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    gen_level_fwd_body(hc, d, job, sm);
}

// engine stage 0 (what k_eng_fwd is for 128 / 3): blockIdx.y = pair, blockIdx.x = first tile
extern "C" __global__ void __launch_bounds__(256)
k_eng_fwd_gen(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.y;
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    const int level = stp->level, cur = stp->cur;
    if (level >= e.m) return;
    if (e.gmax && blockIdx.x == 0 && threadIdx.x == 0) e.gmax[b] = 0;
    const ndp_pair_geom gm = e.geom[b];
    LevelJob job;
    job.n = gm.K + gm.S;
    job.n_tiles = (job.n + NDP_TILE - 1) / NDP_TILE;
    if ((int)blockIdx.x >= job.n_tiles) return;
    const ndp_layer_desc dl = desc_at_level(e.desc, level);
    job.params = e.params + ((size_t)b * e.m + level) * e.p_stride;
    job.freq = level_freq(level, e.k0);
    job.nonrig = nullptr;
    float *pts = e.pts + (size_t)b * 2 * e.n_cap * 3;
    job.x_in = pts + (size_t)cur * e.n_cap * 3;
    job.x_out = pts + (size_t)(cur ^ 1) * e.n_cap * 3;
    job.act = e.act + (size_t)b * (e.desc.n_hidden + 1) * e.n_cap * e.desc.width;
    job.heads = e.heads + (size_t)b * e.n_cap * NDP_HROW;
    job.plane = e.n_cap;
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    gen_level_fwd_body(make_head_cfg(dl), dl, job, sm);
}

// the whole pyramid for one 64-point tile per workgroup (registration.py:253-258): the points stay in LDS from level to level
extern "C" __global__ void __launch_bounds__(256)
k_gen_pyramid_fwd(ndp_layer_desc desc, int m, int k0, int p_stride, WarpJobs jobs) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const ndp_warp_job jb = jobs.j[blockIdx.y];
    const int base = blockIdx.x * NDP_TILE;
    if (base >= jb.n) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, W = desc.width;
    float *pe = sm + gen_fwd_pe(W), *xs = sm + gen_fwd_xs(W), *ho = sm + gen_fwd_ho(W);
    TileIO io;
    io.act = nullptr; io.heads = nullptr; io.nonrig = nullptr; io.n = jb.n; io.plane = 0;
    io.x_in = jb.x; io.shift_in = jb.shift_in;
    for (int l = 0; l < m; ++l) {
        const ndp_layer_desc dl = desc_at_level(desc, l);
        const HeadCfg hc = make_head_cfg(dl);
        io.x_out = l == m - 1 ? jb.x_out : nullptr;
        io.shift_out = l == m - 1 ? jb.shift_out : nullptr;
        if (wv > 0) {
            const float xa = l == 0 ? fwd_fetch_x(io, base, lane, wv - 1) : xs[4 * lane + wv - 1];
            fwd_posenc(xa, ldexpf(1.0f, l + 1 + k0), lane, wv - 1, pe, xs, l == 0);
        }
        __syncthreads();
        gen_tile_core(hc, dl, jb.params + (size_t)l * p_stride, io, base, sm, pe);
        if (wv == 0) fwd_warp(hc, io, base, lane, ho, pe, xs);
        __syncthreads();
    }
}

// ---- backward ---------------------------------------------------------------------------------------------------------------------------
// gp[idx] of the workgroup's partial: the first tile of the workgroup writes, the others add (each element has ONE owner thread)
__device__ __forceinline__ void gen_acc(float *gp, bool first, float v) { *gp = first ? v : *gp + v; }

// dh[k] (k < n_k) of the tile's 64 points = sum over r ascending of z[r] * M[r][k] from zero (ndp_oracle.c:337-343 heads, :352-360 layers),
// the forward's contraction with the roles exchanged: A = M[2 s + h][kb + l31] (contiguous over the lanes), B = z[2 s + h][p].  A wave's
// blocks kb = 32 wv (+ 128) stay in registers until every wave is done reading z (the caller's barrier); gen_dgrad_write then lays them
// over the buffer z lived in.
struct GenDh { f32x16 a[2][2]; };
__device__ __forceinline__ void gen_dgrad(const float *Mm /*[n_r][n_k]*/, int n_r, int n_k, const float *z /*[r][GEN_PS]*/, GenDh &d) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        const int kb = 32 * wv + 128 * q;
#pragma unroll
        for (int r = 0; r < 16; ++r) { d.a[q][0][r] = 0.f; d.a[q][1][r] = 0.f; }
        if (kb >= n_k) continue;                                     // (wave-uniform)
        const int k = kb + l31 < n_k ? kb + l31 : n_k - 1;
        const float *mc = Mm + (size_t)h * n_k + k;
        const float *z0 = z + h * GEN_PS + l31, *z1 = z0 + 32;
        const int n2 = n_r & ~1;
#pragma unroll 8
        for (int r = 0; r < n2; r += 2) {
            const float a = mc[(size_t)r * n_k];
            d.a[q][0] = MFMA32(a, z0[r * GEN_PS], d.a[q][0]);
            d.a[q][1] = MFMA32(a, z1[r * GEN_PS], d.a[q][1]);
        }
        if (n_r & 1) {
            const float a = h == 0 ? mc[(size_t)n2 * n_k] : 0.f, b0 = h == 0 ? z0[n2 * GEN_PS] : 0.f, b1 = h == 0 ? z1[n2 * GEN_PS] : 0.f;
            d.a[q][0] = MFMA32(a, b0, d.a[q][0]);
            d.a[q][1] = MFMA32(a, b1, d.a[q][1]);
        }
    }
}
__device__ __forceinline__ void gen_dgrad_write(float *dst /*[k][GEN_PS]*/, int n_k, const GenDh &d) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int k = 32 * wv + 128 * q + mfma_row(r, h);
            if (k < n_k) { dst[k * GEN_PS + l31] = d.a[q][0][r]; dst[k * GEN_PS + l31 + 32] = d.a[q][1][r]; }
        }
}
// gW[o][k] += sum_p z[o][p] hin[k][p] (p ascending), gb[o] += sum_p z[o][p]: a wave takes 32 x 32 blocks of gW, both operands of the 32
// steps over the points come out of the [feature][point] rows (A = z[ob + l31][2 s + h], B = hin[kb + l31][2 s + h])
__device__ __forceinline__ void gen_wgrad(const float *z /*[o][GEN_PS]*/, const float *hin /*[k][GEN_PS]*/, int n_o, int n_k, float *gW, float *gb, bool first) {
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6, l31 = lane & 31, h = lane >> 5;
    for (int o = t; o < n_o; o += 256) {
        float s = 0.f;
        for (int p = 0; p < 64; ++p) s += z[o * GEN_PS + p];
        gen_acc(gb + o, first, s);
    }
    const int nkb = (n_k + 31) >> 5, nblk = ((n_o + 31) >> 5) * nkb;
    for (int blk = wv; blk < nblk; blk += 4) {
        const int ob = 32 * (blk / nkb), kb = 32 * (blk % nkb);
        const float *zr = z + (ob + l31 < n_o ? ob + l31 : n_o - 1) * GEN_PS + h;
        const float *hr = hin + (kb + l31 < n_k ? kb + l31 : n_k - 1) * GEN_PS + h;
        f32x16 acc;
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll 8
        for (int p = 0; p < 64; p += 2) acc = MFMA32(zr[p], hr[p], acc);
        if (kb + l31 < n_k) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int o = ob + mfma_row(r, h);
                if (o < n_o) gen_acc(gW + (size_t)o * n_k + kb + l31, first, acc[r]);
            }
        }
    }
}

// the backward of a workgroup's tiles: job.act = [n_hidden + 1][plane][W] as the forward left it, job.dO = [plane][16] from the head
// backward (k_head_bwd / k_eng_loss: mlp_scale * dL/d(scaled head outputs), zero rows beyond n), job.gpart = this workgroup's partial
// DX (ndp_level_bwd with dx; the engine's samples are detached): behind the layer-0 block, from D = dz0 and the saved encodings,
//   dx[p][k] += freq (pe[2k+1][p] dpe[p][2k] - pe[2k][p] dpe[p][2k+1]),  dpe[p][c] = sum_o dz0[o][p] W0[o][c]  (o ascending)
// on top of the direct term k_head_bwd_dx left there: one thread per point and axis, the tile's one workgroup -- no atomics.
template <bool DX = false>
__device__ __forceinline__ void gen_level_bwd_body(const HeadCfg &hc, const ndp_layer_desc &d, const BwdJob &job, float *sm,
                                                   float *dx = nullptr, float freq = 0.f) {
    const int t = threadIdx.x, W = d.width, nhid = d.n_hidden, NH = hc.nh;
    float *D = sm, *I = sm + gen_buf(W), *dOs = sm + gen_bwd_do(W), *pes = sm + gen_bwd_pe(W);
    float *gp = job.gpart;
    bool first = true;
    for (int tile = job.tile0; tile < job.n_tiles; tile += job.tile_step, first = false) {
        const size_t base = (size_t)tile * NDP_TILE;
        for (int idx = t; idx < 64 * NDP_NHMAX; idx += 256) dOs[(idx & 15) * GEN_PS + (idx >> 4)] = job.dO[base * NDP_NHMAX + idx];
        for (int idx = t; idx < 64 * 6; idx += 256) { const int p = idx / 6, k = idx - 6 * p; pes[k * GEN_PS + p] = job.heads[(base + p) * NDP_HROW + 16 + k]; }
        gen_load_plane(I, job.act + ((size_t)nhid * job.plane + base) * W, W);
        __syncthreads();
        GenDh acc;
        // heads (ndp_oracle.c:333-343): gbh, gWh from dO and the last activation; dh = dO Wh
        gen_wgrad(dOs, I, NH, W, gp + ndp_off_Wh(&d), gp + ndp_off_bh(&d), first);
        gen_dgrad(job.params + ndp_off_Wh(&d), NH, W, dOs, acc);
        gen_dgrad_write(D, W, acc);                                  // (D holds nothing yet: no barrier needed before the write)
        __syncthreads();
        for (int l = nhid; l >= 1; --l) {
            // dz_l = dh where the layer's output (in I) is positive (ndp_oracle.c:348), in place
            for (int idx = t; idx < W * GEN_PS; idx += 256) D[idx] = I[idx] > 0.f ? D[idx] : 0.f;
            __syncthreads();
            gen_load_plane(I, job.act + ((size_t)(l - 1) * job.plane + base) * W, W);     // the layer's input
            __syncthreads();
            gen_wgrad(D, I, W, W, gp + ndp_off_Wi(&d, l), gp + ndp_off_bi(&d, l), first);
            gen_dgrad(job.params + ndp_off_Wi(&d, l), W, W, D, acc);
            __syncthreads();                                         // every wave is done with dz_l
            gen_dgrad_write(D, W, acc);
            __syncthreads();
        }
        // layer 0 (ndp_oracle.c:363-368): dz0, gb0, gW0 against the saved encodings
        for (int idx = t; idx < W * GEN_PS; idx += 256) D[idx] = I[idx] > 0.f ? D[idx] : 0.f;
        __syncthreads();
        for (int o = t; o < W; o += 256) {
            float s = 0.f;
            for (int p = 0; p < 64; ++p) s += D[o * GEN_PS + p];
            gen_acc(gp + ndp_off_b0(&d) + o, first, s);
        }
        for (int idx = t; idx < 6 * W; idx += 256) {
            const int o = idx / 6, k = idx - 6 * o;
            float s = 0.f;
            for (int p = 0; p < 64; ++p) s = fmaf(D[o * GEN_PS + p], pes[k * GEN_PS + p], s);
            gen_acc(gp + ndp_off_W0(&d) + idx, first, s);
        }
        if (DX && t < 192 && base + (t & 63) < (size_t)job.n) {
            const int p = t & 63, k = t >> 6;                        // (k is wave-uniform: the W0 reads are)
            const float *w = job.params + ndp_off_W0(&d) + 2 * k;
            float dsin = 0.f, dcos = 0.f;
            for (int o = 0; o < W; ++o) {
                const float z = D[o * GEN_PS + p];
                dsin = fmaf(z, w[6 * o], dsin);
                dcos = fmaf(z, w[6 * o + 1], dcos);
            }
            float *q = dx + (base + p) * 3 + k;
            *q += freq * (pes[(2 * k + 1) * GEN_PS + p] * dsin - pes[2 * k * GEN_PS + p] * dcos);
        }
        __syncthreads();                                             // the next tile's loads overwrite I / dOs / pes
    }
}

extern "C" __global__ void __launch_bounds__(256)
k_gen_level_bwd(HeadCfg hc, ndp_layer_desc d, BwdJob job, int p_stride) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    job.gpart = job.gpart + (size_t)blockIdx.x * p_stride;
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    gen_level_bwd_body(hc, d, job, sm);
}
extern "C" __global__ void __launch_bounds__(256)
k_gen_level_bwd_dx(HeadCfg hc, ndp_layer_desc d, BwdJob job, int p_stride, float *dx, float freq) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    job.gpart = job.gpart + (size_t)blockIdx.x * p_stride;
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    gen_level_bwd_body<true>(hc, d, job, sm, dx, freq);
}

// engine stage 3 (both backward stages of the 128 / 3 kernels in one): blockIdx.y = pair, blockIdx.x = partial
extern "C" __global__ void __launch_bounds__(256)
k_eng_bwd_gen(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.y;
    const ndp_pair_state *nsp = e.state + (size_t)(parity ^ 1) * e.B + b;       // written by k_eng_loss this tick
    const int decision = nsp->decision, step_level = nsp->step_level;
    if (decision == NDP_DEC_IDLE || decision == NDP_DEC_ADVANCE) return;
    const ndp_pair_geom gm = e.geom[b];
    BwdJob job;
    job.n = gm.K + gm.S;
    job.n_tiles = (job.n + NDP_TILE - 1) / NDP_TILE;
    job.gpart = e.gpart + ((size_t)b * e.G + blockIdx.x) * e.p_stride;
    if ((int)blockIdx.x >= job.n_tiles) {                            // no tile for this workgroup: its partial reads as zero
        for (int i = threadIdx.x; i < e.P; i += 256) job.gpart[i] = 0.f;
        return;
    }
    const ndp_layer_desc dl = desc_at_level(e.desc, step_level);
    job.params = e.params + ((size_t)b * e.m + step_level) * e.p_stride;
    job.act = e.act + (size_t)b * (e.desc.n_hidden + 1) * e.n_cap * e.desc.width;
    job.heads = e.heads + (size_t)b * e.n_cap * NDP_HROW;
    job.dO = e.dO + (size_t)b * e.n_cap * NDP_NHMAX;
    job.plane = e.n_cap;
    job.tile0 = blockIdx.x;
    job.tile_step = gridDim.x;
    gen_level_bwd_body(make_head_cfg(dl), dl, job, sm);
}
