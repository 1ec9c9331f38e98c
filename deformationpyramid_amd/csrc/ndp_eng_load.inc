// ndp_eng_load.inc -- pair preparation and slot (re)fill: k_pair_means*, LoadJobs, k_eng_load.  Stays ahead of ndp_nn_cells.inc.
// ---- pair preparation (registration.py:150-164) and slot (re)fill, batched over pairs ----------------------
// means of two clouds: blockIdx.x = 0 source, 1 target.  Double accumulation in a fixed order, one rounding.
extern "C" __global__ void __launch_bounds__(1024)
k_pair_means(const float *src, int n_src, const float *tgt, int n_tgt, float *means) {
    __shared__ double red[3][1024];
    const float *x = blockIdx.x ? tgt : src;
    const int n = blockIdx.x ? n_tgt : n_src, t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int p0 = t; p0 < n; p0 += 4 * 1024) {               // four independent loads in flight per thread
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + 1024 * u;
            v[u][0] = v[u][1] = v[u][2] = 0.f;
            if (p < n) { v[u][0] = x[3 * (size_t)p]; v[u][1] = x[3 * (size_t)p + 1]; v[u][2] = x[3 * (size_t)p + 2]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { s0 += (double)v[u][0]; s1 += (double)v[u][1]; s2 += (double)v[u][2]; }
    }
    red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if (t < d) { red[0][t] += red[0][t + d]; red[1][t] += red[1][t + d]; red[2][t] += red[2][t + d]; }
        __syncthreads();
    }
    if (t < 4) means[4 * blockIdx.x + t] = t < 3 ? (float)(red[t][0] / (double)n) : 0.f;
}

struct LoadJobs {
    ndp_load_job j[NDP_MAX_LOAD_JOBS];
};
// the means of the raw clouds of the jobs that ask for them (n_src > 0), ONE launch per load call instead of one k_pair_means per pair
// (24 576 launches per bench run, 4.6 % of the kernel time under two engines' contention: profiles/r04_bench_kernel_stats.csv):
// blockIdx.y = job, blockIdx.x = 0 source / 1 target; per block the code of k_pair_means -- same order, same bits
extern "C" __global__ void __launch_bounds__(1024)
k_pair_means_jobs(LoadJobs jobs) {
    __shared__ double red[3][1024];
    const ndp_load_job jb = jobs.j[blockIdx.y];
    if (!jb.params || !jb.means || jb.n_src <= 0) return;
    const float *x = blockIdx.x ? jb.tgt : jb.src;
    const int n = blockIdx.x ? jb.n_tgt : jb.n_src, t = threadIdx.x;
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (int p0 = t; p0 < n; p0 += 4 * 1024) {
        float v[4][3];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int p = p0 + 1024 * u;
            v[u][0] = v[u][1] = v[u][2] = 0.f;
            if (p < n) { v[u][0] = x[3 * (size_t)p]; v[u][1] = x[3 * (size_t)p + 1]; v[u][2] = x[3 * (size_t)p + 2]; }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) { s0 += (double)v[u][0]; s1 += (double)v[u][1]; s2 += (double)v[u][2]; }
    }
    red[0][t] = s0; red[1][t] = s1; red[2][t] = s2;
    __syncthreads();
    for (int d = 512; d > 0; d >>= 1) {
        if (t < d) { red[0][t] += red[0][t + d]; red[1][t] += red[1][t + d]; red[2][t] += red[2][t + d]; }
        __syncthreads();
    }
    if (t < 4) jb.means[4 * blockIdx.x + t] = t < 3 ? (float)(red[t][0] / (double)n) : 0.f;
}
extern "C" __global__ void __launch_bounds__(256)
k_eng_load(ndp_engine e, int parity, LoadJobs jobs) {
    const ndp_load_job jb = jobs.j[blockIdx.y];
    const int b = jb.slot, t = blockIdx.x * 256 + threadIdx.x, stride = gridDim.x * 256;
    ndp_pair_state *st = e.state + (size_t)parity * e.B + b;
    if (!jb.params) {                                        // park: the slot reads as finished
        if (t == 0) {
            ndp_pair_state c;
            memset(&c, 0, sizeof c);
            c.level = e.m;
            c.decision = NDP_DEC_IDLE;
            *st = c;
        }
        return;
    }
    float ms[3] = {0.f, 0.f, 0.f}, mt[3] = {0.f, 0.f, 0.f};
    if (jb.means) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { ms[a] = jb.means[a]; mt[a] = jb.means[4 + a]; }
    }
    const int n = jb.K + jb.S;
    // centred landmarks + centred source samples -> point buffer 0 (rest of the plane zero)
    float *pts = e.pts + (size_t)b * 2 * e.n_cap * 3;
    for (int i = t; i < e.n_cap; i += stride) {
        float v[3] = {0.f, 0.f, 0.f};
        if (i < n) {
            const float *q = i < jb.K ? jb.ldmk_s + 3 * (size_t)i
                                      : jb.src + 3 * (size_t)(jb.perm_s ? jb.perm_s[i - jb.K] : i - jb.K);
#pragma unroll
            for (int a = 0; a < 3; ++a) v[a] = q[a] - ms[a];
        }
        pts[3 * i] = v[0]; pts[3 * i + 1] = v[1]; pts[3 * i + 2] = v[2];
    }
    float *lt = e.ldmk_t + (size_t)b * e.n_cap * 3;
    for (int i = t; i < jb.K; i += stride) {
#pragma unroll
        for (int a = 0; a < 3; ++a) lt[3 * i + a] = jb.ldmk_t[3 * (size_t)i + a] - mt[a];
    }
    float *tg = e.tgt + (size_t)b * e.t_cap * 3;
    for (int i = t; i < jb.T; i += stride) {
        const float *q = jb.tgt + 3 * (size_t)(jb.perm_t ? jb.perm_t[i] : i);
#pragma unroll
        for (int a = 0; a < 3; ++a) tg[3 * i + a] = q[a] - mt[a];
    }
    // parameters of every level, fresh Adam moments
    {
        const float4 *src = reinterpret_cast<const float4 *>(jb.params);
        float4 *dst = reinterpret_cast<float4 *>(e.params + (size_t)b * e.m * e.p_stride);
        const int n4 = e.m * e.p_stride / 4;
        for (int i = t; i < n4; i += stride) dst[i] = src[i];
        float4 *am = reinterpret_cast<float4 *>(e.adam_m + (size_t)b * e.p_stride);
        float4 *av = reinterpret_cast<float4 *>(e.adam_v + (size_t)b * e.p_stride);
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = t; i < e.p_stride / 4; i += stride) { am[i] = z; av[i] = z; }
    }
    if (t == 0) {
        ndp_pair_geom g;
        g.K = jb.K; g.S = jb.S; g.T = jb.T; g.pad = 0;
        e.geom[b] = g;
        ndp_pair_state c;
        memset(&c, 0, sizeof c);
        c.loss_prev = 1e6;                                   // registration.py:179
        *st = c;
    }
}
