// ndp_eng_fwd.inc -- the engine's fp32 forward stage (k_eng_fwd) and what every later engine stage shares: level_freq,
// xcd_pair_block, NDP_LROW.  Stays ahead of ndp_fwd_split.inc.
// ------------------------------------------------------------------------------------------------
// batched engine kernels: blockIdx.y = pair
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ float level_freq(int level, int k0) { return ldexpf(1.0f, level + 1 + k0); }

extern "C" __global__ void __launch_bounds__(256, 2)
k_eng_fwd(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    const int b = blockIdx.y;
    const ndp_pair_state st = e.state[parity * e.B + b];
    if (st.level >= e.m) return;
    if (e.gmax && blockIdx.x == 0 && threadIdx.x == 0) e.gmax[b] = 0;   // this tick's max |dO| starts from zero (k_eng_loss raises it)
    const ndp_pair_geom gm = e.geom[b];
    LevelJob job;
    job.n = gm.K + gm.S;
    job.n_tiles = (job.n + NDP_TILE - 1) / NDP_TILE;
    if ((int)blockIdx.x >= job.n_tiles) return;
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
    PT_INIT;
    level_fwd_body(hc, job, sm);
    PT_FLUSH(12);
}

// XCD-aware placement of a (nvb, B) grid whose nvb workgroups per pair share that pair's data: hardware block L = y nvb + x runs on
// XCD L % 8 (observed dispatch order, MI355X_MICROARCH.md: used for speed only -- any placement computes the same thing), so the
// workgroups of one pair are taken from blocks that are congruent mod 8: they then share ONE XCD's L2 instead of pulling the pair's
// targets, indices and partials into eight of them.  (Pairs beyond the last full group of eight keep the plain order.)
__device__ __forceinline__ void xcd_pair_block(int nvb, int B, int &b, int &vb) {
    const int L = blockIdx.y * nvb + blockIdx.x, nfull = B & ~7;
    if (L < nfull * nvb) {
        const int slot = L >> 3;
        b = (slot / nvb) * 8 + (L & 7);
        vb = slot % nvb;
    } else {
        const int r = L - nfull * nvb;
        b = nfull + r / nvb;
        vb = r % nvb;
    }
}
// Per-thread head rows in LDS (run-time row offsets live there) are NDP_LROW = 20 floats apart, not 16: the 16-byte accesses of an
// eight-lane group then hit eight different bank quads and the scalar ones 4-way instead of 16-way ((16 t) mod 32 has two values,
// (20 t) mod 32 eight) -- SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of k_eng_loss 0.68 before.
#define NDP_LROW 20
