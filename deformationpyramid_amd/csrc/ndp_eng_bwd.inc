// ndp_eng_bwd.inc -- the engine's fp32 backward stage: eng_bwd_job and its two launches, k_eng_bwd2 and k_eng_bwd1.
// backward of the live tiles of every pair that takes an Adam step this tick (two launches, see bwd2/bwd1)
__device__ __forceinline__ bool eng_bwd_job(const ndp_engine &e, int parity, BwdJob &job, bool zero_idle_partial) {
    const int b = blockIdx.y;
    const ndp_pair_state ns = e.state[(size_t)(parity ^ 1) * e.B + b];     // written by k_eng_loss this tick
    if (ns.decision == NDP_DEC_IDLE || ns.decision == NDP_DEC_ADVANCE) return false;
    const ndp_pair_geom gm = e.geom[b];
    const int n = gm.K + gm.S;
    const int n_tiles = (n + NDP_TILE - 1) / NDP_TILE;
    float *gpart = e.gpart + ((size_t)b * e.G + blockIdx.x) * e.p_stride;
    if ((int)blockIdx.x >= n_tiles) {                  // no tile for this workgroup: its partial is zero
        if (zero_idle_partial) for (int i = threadIdx.x; i < e.P; i += 256) gpart[i] = 0.f;
        return false;
    }
    job.params = e.params + ((size_t)b * e.m + ns.step_level) * e.p_stride;
    job.act = e.act + (size_t)b * 3 * e.n_cap * NDP_W;
    job.heads = e.heads + (size_t)b * e.n_cap * NDP_HROW;
    job.dO = e.dO + (size_t)b * e.n_cap * NDP_NHMAX;
    job.gpart = gpart;
    job.n = n; job.plane = e.n_cap; job.n_tiles = n_tiles;
    job.tile0 = blockIdx.x; job.tile_step = gridDim.x;
    job.dz_plane = job.act + 2 * (size_t)e.n_cap * NDP_W;
    job.h_plane = job.act + (size_t)e.n_cap * NDP_W;
    job.from_dO = 0; job.wh_off = 0; job.nh = 0;
    return true;
}

extern "C" __global__ void __launch_bounds__(256, 2)
k_eng_bwd2(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    BwdJob job;
    if (!eng_bwd_job(e, parity, job, true)) return;                 // first backward kernel of the tick: idle partials read as zero
    bwd_job_ndp_layer2(job, make_head_cfg(desc_at_level(e.desc, e.state[(size_t)(parity ^ 1) * e.B + blockIdx.y].step_level)).nh);
    PT_INIT;
    bwd2_body(make_head_cfg(desc_at_level(e.desc, 0)), job, sm);
    PT_FLUSH(0);
}

extern "C" __global__ void __launch_bounds__(256, 2)
k_eng_bwd1(ndp_engine e, int parity) {
    extern __shared__ __attribute__((aligned(16))) float sm[];
    BwdJob job;
    if (!eng_bwd_job(e, parity, job, false)) return;
    PT_INIT;
    bwd1_body(make_head_cfg(desc_at_level(e.desc, 0)), job, sm);
    PT_FLUSH(24);
}
