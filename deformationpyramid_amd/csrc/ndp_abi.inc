// ndp_abi.inc -- the host entries that choose between files (fp32 / split / generic kernels, the engine's tick and slot load, the
// nearest-neighbour shapes) and the small single-pair operator entries.  An entry that launches one file's kernels sits at that file's tail.
extern "C" int ndp_level_fwd(const ndp_layer_desc *desc, const float *params, int level, int k0,
                             const float *x, int n, float *x_out, float *act, float *heads, float *nonrig_out,
                             void *stream) {
    if (int rc = check_desc(desc)) return rc;
    if (n < 0 || !params || (n > 0 && (!x || !x_out))) return fail(NDP_E_INVALID, "ndp_level_fwd: null pointer / negative n");
    if (!aligned16(params) || (act && !aligned16(act)) || (heads && !aligned16(heads)))
        return fail(NDP_E_INVALID, "ndp_level_fwd: params/act/heads must be 16-byte aligned");
    if (n == 0) return 0;
    LevelJob job;
    job.params = params; job.freq = ldexpf(1.0f, level + 1 + k0);
    job.x_in = x; job.x_out = x_out; job.act = act; job.heads = heads;
    job.nonrig = desc->nonrigidity ? nonrig_out : nullptr;
    job.n = n; job.n_tiles = (n + NDP_TILE - 1) / NDP_TILE; job.plane = job.n_tiles * NDP_TILE;
    job.tile0 = 0; job.tile_step = 0;
    if (gen_is_generic(*desc)) {                                         // act: [n_hidden + 1][plane][width]
        if (int rc = set_smem((const void *)k_gen_level_fwd, kSmemGenFwdMax)) return rc;
        hipLaunchKernelGGL(k_gen_level_fwd, dim3(job.n_tiles < 1024 ? job.n_tiles : 1024), dim3(256), gen_fwd_floats(desc->width) * 4, (hipStream_t)stream,
                           make_head_cfg(*desc), *desc, job);
        HIP_TRY(hipGetLastError(), "k_gen_level_fwd launch");
        return 0;
    }
    if (int rc = set_smem((const void *)k_level_fwd, kSmemFwdBytes)) return rc;
    // one tile per workgroup: measured best for the final all-point warp (more tiles per workgroup save weight
    // loads but lengthen the warp, and throughput dropped 478 -> 438 pairs/s at 4 tiles per workgroup)
    const int grid = job.n_tiles < 1024 ? job.n_tiles : 1024;
    hipLaunchKernelGGL(k_level_fwd, dim3(grid), dim3(256), kSmemFwdBytes, (hipStream_t)stream, make_head_cfg(*desc), job);
    HIP_TRY(hipGetLastError(), "k_level_fwd launch");
    return 0;
}

extern "C" int ndp_level_bwd(const ndp_layer_desc *desc, const float *params, int level, int k0,
                             const float *x, int n, float *act, const float *heads, const float *g, const float *g_nr,
                             float *dO_work, float *grads_part, int n_part, int p_stride, void *stream, float *dx) {
    if (int rc = check_desc(desc)) return rc;
    if (n <= 0 || !params || !x || !act || !heads || !g || !dO_work || !grads_part || n_part < 1)
        return fail(NDP_E_INVALID, "ndp_level_bwd: null pointer / bad sizes");
    if (p_stride < ndp_param_count(desc)) return fail(NDP_E_INVALID, "ndp_level_bwd: p_stride < P");
    if (!aligned16(params) || !aligned16(act) || !aligned16(heads) || !aligned16(dO_work))
        return fail(NDP_E_INVALID, "ndp_level_bwd: params/act/heads/dO_work must be 16-byte aligned");
    // dx needs the level's frequency 2^(level + 1 + k0): a finite, normal float
    if (dx && (level < 0 || level >= NDP_MAX_LEVELS || level + 1 + k0 < -126 || level + 1 + k0 > 127))
        return fail(NDP_E_INVALID, "ndp_level_bwd: dx needs 0 <= level < 16 and 2^(level + 1 + k0) in float range");
    if (dx && ((uintptr_t)dx & 3)) return fail(NDP_E_INVALID, "ndp_level_bwd: dx must be 4-byte aligned");
    const float freq = dx ? ldexpf(1.0f, level + 1 + k0) : 0.f;
    BwdJob job;
    memset(&job, 0, sizeof job);
    job.params = params; job.act = act; job.heads = heads; job.dO = dO_work; job.gpart = grads_part;
    job.n = n; job.n_tiles = (n + NDP_TILE - 1) / NDP_TILE; job.plane = job.n_tiles * NDP_TILE;
    hipStream_t s = (hipStream_t)stream;
    if (n_part > job.n_tiles) {
        // partials with no tile must read as zero
        HIP_TRY(hipMemsetAsync(grads_part + (size_t)job.n_tiles * p_stride, 0,
                               sizeof(float) * (size_t)(n_part - job.n_tiles) * p_stride, s), "memset");
        n_part = job.n_tiles;
    }
    const HeadCfg hc = make_head_cfg(*desc);
    // dx: the head backward leaves the direct part of dL/dx there, the level backward adds the part through the network
    if (dx) hipLaunchKernelGGL(k_head_bwd_dx, dim3((job.plane + 255) / 256), dim3(256), 0, s, hc, x, heads, g,
                               desc->nonrigidity ? g_nr : nullptr, n, job.plane, dO_work, dx);
    else hipLaunchKernelGGL(k_head_bwd, dim3((job.plane + 255) / 256), dim3(256), 0, s, hc, x, heads, g,
                            desc->nonrigidity ? g_nr : nullptr, n, job.plane, dO_work);
    if (gen_is_generic(*desc)) {
        if (int rc = set_smem((const void *)k_gen_level_bwd, kSmemGenBwdMax)) return rc;
        if (dx) {
            if (int rc = set_smem((const void *)k_gen_level_bwd_dx, kSmemGenBwdMax)) return rc;
            hipLaunchKernelGGL(k_gen_level_bwd_dx, dim3(n_part), dim3(256), gen_bwd_floats(desc->width) * 4, s, hc, *desc, job, p_stride, dx, freq);
        } else hipLaunchKernelGGL(k_gen_level_bwd, dim3(n_part), dim3(256), gen_bwd_floats(desc->width) * 4, s, hc, *desc, job, p_stride);
        HIP_TRY(hipGetLastError(), "generic level backward launch");
        return 0;
    }
    if (int rc = set_smem((const void *)k_level_bwd2, kSmemBwdBytes)) return rc;
    if (int rc = set_smem((const void *)k_level_bwd1, kSmemBwdBytes)) return rc;
    job.dz_plane = act + 2 * (size_t)job.plane * NDP_W;
    job.h_plane = act + (size_t)job.plane * NDP_W;
    bwd_job_ndp_layer2(job, hc.nh);
    hipLaunchKernelGGL(k_level_bwd2, dim3(n_part), dim3(256), kSmemBwdBytes, s, hc, job, p_stride);
    if (dx) {
        if (int rc = set_smem((const void *)k_level_bwd1_dx, kSmemBwdBytes)) return rc;
        hipLaunchKernelGGL(k_level_bwd1_dx, dim3(n_part), dim3(256), kSmemBwdBytes, s, hc, job, p_stride, dx, freq);
    } else hipLaunchKernelGGL(k_level_bwd1, dim3(n_part), dim3(256), kSmemBwdBytes, s, hc, job, p_stride);
    HIP_TRY(hipGetLastError(), "level backward launch");
    return 0;
}

extern "C" int ndp_grad_reduce(const float *grads_part, int n_part, int p_stride, int P, float *grads, void *stream) {
    if (!grads_part || !grads || n_part < 1 || P < 1) return fail(NDP_E_INVALID, "ndp_grad_reduce: bad arguments");
    hipLaunchKernelGGL(k_grad_reduce, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, grads_part, n_part, p_stride, P, grads);
    HIP_TRY(hipGetLastError(), "k_grad_reduce launch");
    return 0;
}

extern "C" int ndp_pyramid_fwd_batch(const ndp_layer_desc *desc, int m, int k0, int p_stride,
                                     const ndp_warp_job *jobs, int n_jobs, void *stream);

extern "C" int ndp_pyramid_fwd(const ndp_layer_desc *desc, int m, int k0, const float *params_all, int p_stride,
                               const float *x, int n, float *x_out, void *stream) {
    if (int rc = check_desc(desc)) return rc;
    if (m < 0 || m > NDP_MAX_LEVELS || n < 0 || !x_out || (n > 0 && !x)) return fail(NDP_E_INVALID, "ndp_pyramid_fwd: bad arguments");
    if (n == 0) return 0;
    if (m == 0) {
        HIP_TRY(hipMemcpyAsync(x_out, x, sizeof(float) * 3 * (size_t)n, hipMemcpyDeviceToDevice, (hipStream_t)stream), "memcpy");
        return 0;
    }
    ndp_warp_job job;
    memset(&job, 0, sizeof job);
    job.params = params_all; job.x = x; job.x_out = x_out; job.n = n;
    return ndp_pyramid_fwd_batch(desc, m, k0, p_stride, &job, 1, stream);
}

static int pyramid_fwd_batch_impl(const ndp_layer_desc *desc, int m, int k0, int p_stride, const ndp_warp_job *jobs, int n_jobs,
                                  void *stream, bool split, int tiles = P8_TILES) {
    if (int rc = check_desc(desc)) return rc;
    if (m < 1 || m > NDP_MAX_LEVELS || n_jobs < 0 || (n_jobs > 0 && !jobs) || p_stride < ndp_param_count(desc) || (p_stride & 3))
        return fail(NDP_E_INVALID, "ndp_pyramid_fwd_batch: bad arguments");
    const bool generic = gen_is_generic(*desc);                        // one arithmetic there: `split` and `tiles` select nothing
    if (generic) { if (int rc = set_smem((const void *)k_gen_pyramid_fwd, kSmemGenFwdMax)) return rc; }
    else if (split) { if (int rc = set_smem((const void *)k_pyramid_fwd8, kSmemPyr8Bytes)) return rc; }
    else if (int rc = set_smem((const void *)k_pyramid_fwd, kSmemFwdBytes)) return rc;
    if (split && (tiles < 1 || tiles > P8_TILES_MAX)) return fail(NDP_E_INVALID, "ndp_pyramid_fwd_batch_split_tiles: tiles per workgroup must be 1..8");
    const int per_wg = generic ? NDP_TILE : NDP_TILE * (split ? tiles : NDP_PYR_TILES);       // points per workgroup
    for (int j0 = 0; j0 < n_jobs; j0 += NDP_MAX_WARP_JOBS) {
        WarpJobs wj;
        memset(&wj, 0, sizeof wj);
        int cnt = 0, max_wgs = 0;
        for (int j = j0; j < n_jobs && cnt < NDP_MAX_WARP_JOBS; ++j) {
            const ndp_warp_job &q = jobs[j];
            if (q.n < 0 || (q.n > 0 && (!q.params || !q.x || !q.x_out))) return fail(NDP_E_INVALID, "ndp_pyramid_fwd_batch: null pointer / negative n");
            if (!aligned16(q.params)) return fail(NDP_E_INVALID, "ndp_pyramid_fwd_batch: params must be 16-byte aligned");
            if (q.n == 0) continue;
            wj.j[cnt++] = q;
            const int wgs = (q.n + per_wg - 1) / per_wg;                                          // workgroups of this cloud
            if (wgs > max_wgs) max_wgs = wgs;
        }
        if (!cnt) continue;
        if (generic) hipLaunchKernelGGL(k_gen_pyramid_fwd, dim3(max_wgs, cnt), dim3(256), gen_fwd_floats(desc->width) * 4, (hipStream_t)stream, *desc, m, k0, p_stride, wj);
        else if (split) hipLaunchKernelGGL(k_pyramid_fwd8, dim3(max_wgs, cnt), dim3(512), kSmemPyr8Bytes, (hipStream_t)stream, *desc, m, k0, p_stride, wj, tiles);
        else hipLaunchKernelGGL(k_pyramid_fwd, dim3(max_wgs, cnt), dim3(256), kSmemFwdBytes, (hipStream_t)stream, *desc, m, k0, p_stride, wj);
        HIP_TRY(hipGetLastError(), "k_pyramid_fwd launch");
    }
    return 0;
}

extern "C" int ndp_pyramid_fwd_batch(const ndp_layer_desc *desc, int m, int k0, int p_stride,
                                     const ndp_warp_job *jobs, int n_jobs, void *stream) {
    return pyramid_fwd_batch_impl(desc, m, k0, p_stride, jobs, n_jobs, stream, false);
}

// The same warp with the engine's split arithmetic (gemm_mode & 1): the 128-wide contractions as three-way bf16 splits on the
// bf16 MFMA (k_pyramid_fwd8) -- fp32-level accuracy (1e-5 of the fp32-MFMA kernel on warped coordinates), not bitwise the chain.
extern "C" int ndp_pyramid_fwd_batch_split(const ndp_layer_desc *desc, int m, int k0, int p_stride,
                                           const ndp_warp_job *jobs, int n_jobs, void *stream) {
    return pyramid_fwd_batch_impl(desc, m, k0, p_stride, jobs, n_jobs, stream, true);
}
// ... with `tiles` 64-point tiles per workgroup (1..8; the entry above: 4).  More tiles per workgroup = fewer weight prologues per cloud
// (less CU-time per cloud, the batched engine's choice) at a longer latency of the launch (fewer, longer workgroups).  Same bits.
extern "C" int ndp_pyramid_fwd_batch_split_tiles(const ndp_layer_desc *desc, int m, int k0, int p_stride,
                                                 const ndp_warp_job *jobs, int n_jobs, int tiles, void *stream) {
    return pyramid_fwd_batch_impl(desc, m, k0, p_stride, jobs, n_jobs, stream, true, tiles);
}

extern "C" int ndp_pair_means(const float *src, int n_src, const float *tgt, int n_tgt, float *means, void *stream) {
    if (!src || !tgt || !means || n_src < 1 || n_tgt < 1) return fail(NDP_E_INVALID, "ndp_pair_means: bad arguments");
    hipLaunchKernelGGL(k_pair_means, dim3(2), dim3(1024), 0, (hipStream_t)stream, src, n_src, tgt, n_tgt, means);
    HIP_TRY(hipGetLastError(), "k_pair_means launch");
    return 0;
}

static int check_engine(const ndp_engine *e, const char *who) {
    if (!e) return fail(NDP_E_INVALID, "null engine");
    if (int rc = check_desc(&e->desc)) return rc;
    if (e->B < 1 || e->G < 1 || e->m < 1 || e->m > NDP_MAX_LEVELS || e->n_cap % NDP_TILE || e->t_cap % NDP_TILE ||
        e->P != ndp_param_count(&e->desc) || e->p_stride < e->P || (e->p_stride & 3)) {
        snprintf(g_err, sizeof g_err, "%s: inconsistent engine descriptor", who);
        return NDP_E_INVALID;
    }
    if (!e->geom || !e->state || !e->pts || !e->params || !e->gpart || !e->adam_m || !e->adam_v || !e->act ||
        !e->heads || !e->adam_tab || !e->dO) {
        snprintf(g_err, sizeof g_err, "%s: null buffer", who);
        return NDP_E_INVALID;
    }
    if (e->nn_cells && e->nn_cells_wide) {
        snprintf(g_err, sizeof g_err, "%s: nn_cells and nn_cells_wide together (one search takes the nearest-neighbour stage)", who);
        return NDP_E_INVALID;
    }
    if ((e->gemm_mode & 6) && !e->gmax) {
        snprintf(g_err, sizeof g_err, "%s: the split backward (gemm_mode & 6) needs the gmax buffer", who);
        return NDP_E_INVALID;
    }
    return 0;
}

// the two cell searches: what the engine must be (no HIP call: the tick plan asks too), then the LDS attributes ndp_engine_load needs
static int check_nn_cells(const ndp_engine *e, const char *who) {
    if (!nnc_fits(e->n_cap, e->t_cap))
        return failf(NDP_E_UNSUPPORTED, "%s: nn_cells needs n_cap and t_cap <= %d (ndp_engine_nn_cells_fits)", who, NNC_MAX);
    if (!e->nnc_geom || !e->nnc_start || !e->nnc_rec || !aligned16(e->nnc_start) || !aligned16(e->nnc_rec))
        return failf(NDP_E_INVALID, "%s: nn_cells without its grid buffers (nnc_geom, nnc_start, nnc_rec; 16-byte aligned)", who);
    return 0;
}
static int smem_nn_cells() {
    if (int rc = set_smem((const void *)k_eng_nn_cells_build, NNC_LDS_BYTES)) return rc;
    return set_smem((const void *)k_eng_nn_cells, NNC_LDS_BYTES);
}

static int check_nn_cells_wide(const ndp_engine *e, const char *who) {
    if (!nnw_fits(e->n_cap, e->t_cap))
        return failf(NDP_E_UNSUPPORTED, "%s: nn_cells_wide needs n_cap and t_cap <= %d (ndp_engine_nn_cells_wide_fits)", who, NNW_MAX);
    if (!e->nnc_geom || !e->nnc_start || !e->nnc_rec || !aligned16(e->nnc_start) || !aligned16(e->nnc_rec))
        return failf(NDP_E_INVALID, "%s: nn_cells_wide without its grid buffers (nnc_geom [B][8], nnc_start [B][2][NDP_NNC_START], nnc_rec [B][t_cap + n_cap][4]; 16-byte aligned)", who);
    return 0;
}
static int smem_nn_cells_wide() { return set_smem((const void *)k_eng_nn_cells_wide, NNW_LDS_BYTES); }

extern "C" int ndp_engine_load(const ndp_engine *e, int tick, const ndp_load_job *jobs, int n_jobs, void *stream) {
    if (int rc = check_engine(e, "ndp_engine_load")) return rc;
    if (n_jobs < 0 || n_jobs > NDP_MAX_LOAD_JOBS || (n_jobs > 0 && !jobs)) return fail(NDP_E_INVALID, "ndp_engine_load: bad job count");
    if (n_jobs == 0) return 0;
    LoadJobs lj;
    memset(&lj, 0, sizeof lj);
    bool any_means = false;
    for (int j = 0; j < n_jobs; ++j) {
        const ndp_load_job &q = jobs[j];
        if (q.slot < 0 || q.slot >= e->B) return fail(NDP_E_INVALID, "ndp_engine_load: slot out of range");
        if (q.params) {
            if (q.K < 0 || q.S < 0 || q.T < 0 || q.K + q.S < 1 || q.K + q.S > e->n_cap || q.T > e->t_cap)
                return fail(NDP_E_INVALID, "ndp_engine_load: pair does not fit the engine capacities");
            if ((q.K > 0 && (!q.ldmk_s || !q.ldmk_t)) || (q.S > 0 && !q.src) || (q.T > 0 && (!q.tgt || !e->tgt)) ||
                (q.K > 0 && !e->ldmk_t))
                return fail(NDP_E_INVALID, "ndp_engine_load: null cloud pointer");
            if (!aligned16(q.params)) return fail(NDP_E_INVALID, "ndp_engine_load: params must be 16-byte aligned");
            if (q.S > 0 && q.T == 0 && e->w_cd != 0.f)
                return fail(NDP_E_INVALID, "ndp_engine_load: samples without targets (S > 0, T == 0) under a Chamfer term (w_cd != 0): the loss would be 0/0");
        }
        if (q.params && q.n_src > 0) {
            if (!q.means || !q.src || !q.tgt || q.n_tgt < 1) return fail(NDP_E_INVALID, "ndp_engine_load: means to compute need src, tgt, n_tgt and the means buffer");
            any_means = true;
        }
        lj.j[j] = q;
    }
    if (any_means) {
        hipLaunchKernelGGL(k_pair_means_jobs, dim3(2, n_jobs), dim3(1024), 0, (hipStream_t)stream, lj);
        HIP_TRY(hipGetLastError(), "k_pair_means_jobs launch");
    }
    hipLaunchKernelGGL(k_eng_load, dim3(32, n_jobs), dim3(256), 0, (hipStream_t)stream, *e, tick & 1, lj);
    HIP_TRY(hipGetLastError(), "k_eng_load launch");
    if (e->nn_cells && e->w_cd != 0.f && e->t_cap > 0) {          // the grid of the new pairs' targets: they stay put while the pair lives
        if (int rc = check_nn_cells(e, "ndp_engine_load")) return rc;
        if (int rc = smem_nn_cells()) return rc;
        hipLaunchKernelGGL(k_eng_nn_cells_build, dim3(n_jobs), dim3(NNC_NT), NNC_LDS_BYTES, (hipStream_t)stream, *e, lj);
        HIP_TRY(hipGetLastError(), "k_eng_nn_cells_build launch");
    }
    if (e->nn_cells_wide && e->w_cd != 0.f && e->t_cap > 0) {
        if (int rc = check_nn_cells_wide(e, "ndp_engine_load")) return rc;
        if (int rc = smem_nn_cells_wide()) return rc;
        hipLaunchKernelGGL(k_eng_nnw_build, dim3(n_jobs), dim3(NNW_NT), NNW_SORT_LDS_BYTES, (hipStream_t)stream, *e, lj);
        HIP_TRY(hipGetLastError(), "k_eng_nnw_build launch");
    }
    return 0;
}

extern "C" int ndp_chamfer_nn_fwd(const float *x, int S, const float *y, int T,
                                  float *d2x, int *idx_x, float *d2y, int *idx_y, void *stream) {
    if (S <= 0 || T <= 0 || !x || !y || !d2x || !idx_x || !d2y || !idx_y) return fail(NDP_E_INVALID, "ndp_chamfer_nn_fwd: bad arguments");
    const int grid = (S + NN_QPB - 1) / NN_QPB + (T + NN_QPB - 1) / NN_QPB;
    hipLaunchKernelGGL(k_nn, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, S, y, T, d2x, idx_x, d2y, idx_y);
    HIP_TRY(hipGetLastError(), "k_nn launch");
    return 0;
}

extern "C" int ndp_chamfer_l1_bwd(const float *x, int S, const float *y, int T, float trunc,
                                  const float *d2x, const int *idx_x, const float *d2y, const int *idx_y,
                                  float *loss, float *gx, int point_sum, void *stream) {
    if (S <= 0 || T <= 0 || !x || !y || !d2x || !idx_x || !d2y || !idx_y || !loss) return fail(NDP_E_INVALID, "ndp_chamfer_l1_bwd: bad arguments");
    hipLaunchKernelGGL(k_chamfer_bwd, dim3((S + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, S, y, T, trunc, d2x, idx_x, d2y, idx_y, loss, gx, point_sum ? 1 : 0);
    HIP_TRY(hipGetLastError(), "k_chamfer_bwd launch");
    return 0;
}

extern "C" int ndp_landmark_mse_fwd_bwd(const float *x, const float *t, int K, float *loss, float *gx, void *stream) {
    if (K <= 0 || !x || !t || !loss) return fail(NDP_E_INVALID, "ndp_landmark_mse_fwd_bwd: bad arguments");
    hipLaunchKernelGGL(k_landmark, dim3((K + 255) / 256), dim3(256), 0, (hipStream_t)stream, x, t, K, loss, gx);
    HIP_TRY(hipGetLastError(), "k_landmark launch");
    return 0;
}

extern "C" int ndp_adam_step(float *params, const float *grads, float *m, float *v, int P,
                             float w1, float b2, float w2, float neg_step, float bc2_sqrt, float eps, void *stream) {
    if (P <= 0 || !params || !grads || !m || !v) return fail(NDP_E_INVALID, "ndp_adam_step: bad arguments");
    hipLaunchKernelGGL(k_adam, dim3((P + 255) / 256), dim3(256), 0, (hipStream_t)stream, params, grads, m, v, P, w1, b2, w2, neg_step, bc2_sqrt, eps);
    HIP_TRY(hipGetLastError(), "k_adam launch");
    return 0;
}

// One tick as data: the launches of its NDP_TICK_KERNELS stages, in launch order.  A stage has none (bwd1 under the fused or generic
// backward, nearest neighbours without a Chamfer term), one, or two (the wide cell search: sort, then search).  Every kernel takes
// (engine, parity) and at most one more int, `extra` (-1: none).
struct TickLaunch { const void *fn; ndp_stage_launch at; };
struct TickPlan {
    int n;
    TickLaunch l[2 * NDP_TICK_KERNELS];
    void add(int stage, const void *fn, const char *name, dim3 grid, int block, int lds_bytes, int extra = -1) {
        l[n++] = {fn, {name, stage, {(int)grid.x, (int)grid.y, (int)grid.z}, block, lds_bytes, extra}};
    }
};
#define NDP_K(k) (const void *)(k), #k

// Validate the engine and choose its tick's launches: everything ndp_engine_run decides, and no HIP call (ndp_engine_plan reports
// it on a machine without a GPU).  Stages: 0 forward, 1 nearest neighbours, 2 loss / decision / dL/dx', 3 bwd2, 4 bwd1, 5 update.
static int plan_tick(const ndp_engine *e, TickPlan *p) {
    if (int rc = check_engine(e, "ndp_engine_run")) return rc;
    if (e->gemm_mode & ~(1 | 2 | 4 | 8 | 16 | 32 | 1024))
        return fail(NDP_E_INVALID, "ndp_engine_run: gemm_mode is a mask of 1 (forward), 2 (bwd1), 4 (bwd2) on fp16 splits, 8 (the split forward keeps h0), 16 (bwd2 and bwd1 as two launches), 32 (the fused backward also writes dz1), 1024 (the whole Adam step in k_eng_update) (see ndp_hip.h)");
    const bool nn = e->w_cd != 0.f && e->t_cap > 0;
    if (nn && (!e->nn_row || !e->d2x || !e->d2y || !e->idx_x || !e->idx_y || !e->tgt))
        return fail(NDP_E_INVALID, "ndp_engine_run: Chamfer term without nearest-neighbour buffers");
    if (nn && (e->nn_mode < 0 || e->nn_mode > 2))
        return fail(NDP_E_INVALID, "ndp_engine_run: nn_mode must be 0 (one pass, vector pipe), 1 (latency shape) or 2 (one pass, matrix pipe)");
    // the column table of the one-pass vector kernel lives in LDS: only that shape has a size limit
    const int stage_x = nn1_stage_x(e->n_cap) ? 1 : 0;
    const int nn_lds = nn1_lds_floats(e->n_cap, stage_x) * 4;
    if (nn && e->nn_mode == 0 && nn_lds > 160 * 1024)
        return fail(NDP_E_UNSUPPORTED, "ndp_engine_run: n_cap too large for the one-pass nearest-neighbour kernel (nn_mode 0); use nn_mode 1");
    if (nn && e->nn_cells) if (int rc = check_nn_cells(e, "ndp_engine_run")) return rc;
    if (nn && e->nn_cells_wide) if (int rc = check_nn_cells_wide(e, "ndp_engine_run")) return rc;

    // width / depth other than 128 / 3: the generic fp32 level kernels (csrc/ndp_generic.inc); gemm_mode selects nothing there
    const bool generic = gen_is_generic(e->desc);
    const int mode = generic ? 0 : e->gemm_mode;
    // both backward layers on the splits: ONE launch (k_eng_bwd_f reads h1 as the SPLIT forward's plane image, so all three bits) and
    // nothing in stage 4, unless bit 16 asks for the two round-3 kernels
    const bool bwd_fused = (mode & 7) == 7 && !(mode & 16);
    const dim3 g_lvl(e->G, e->B);
    // the split kernels: one 8-wave workgroup per CU.  With all three of them on (mask 7) the engine is sized for that (G workgroups and
    // G partials per pair); in a mixed configuration they take half the fp32 grid and zero the partials they do not write.
    const dim3 g_8((mode & 7) == 7 ? e->G : (e->G > 1 ? e->G / 2 : 1), e->B);
    p->n = 0;
    if (generic) p->add(0, NDP_K(k_eng_fwd_gen), g_lvl, 256, gen_fwd_floats(e->desc.width) * 4);
    else if (mode & 1) {
        // one tile per workgroup and few of them: the per-point warp rides in the tile loop (ndp_fwd_split.inc); everything else: the
        // workgroup warps its tiles' points behind its tile loop (eng_warp_tail)
        const bool warp_in_fwd = (int)g_8.x == e->n_cap / NDP_TILE && e->B * (int)g_8.x <= 256;
        p->add(0, NDP_K(k_eng_fwd8), g_8, 512, kSmemFwd8Bytes, warp_in_fwd ? 0 : 1);
    } else p->add(0, NDP_K(k_eng_fwd), g_lvl, 256, kSmemFwdBytes);

    // a cell search takes the stage whatever nn_mode names; the latency shape has a 16-wave form for one or two pairs
    const dim3 g_nn_lat(e->n_cap / 64 + e->t_cap / 64, e->B);
    if (!nn) {}
    else if (e->nn_cells) p->add(1, NDP_K(k_eng_nn_cells), dim3(2, e->B), NNC_NT, NNC_LDS_BYTES);
    else if (e->nn_cells_wide) {
        const int q = nnw_chunks(e->n_cap, e->t_cap);
        p->add(1, NDP_K(k_eng_nnw_sort), dim3(e->B), NNW_NT, NNW_SORT_LDS_BYTES);
        p->add(1, NDP_K(k_eng_nn_cells_wide), dim3(2 * q, e->B), NNW_NT, NNW_LDS_BYTES, q);
    }
    else if (e->nn_mode == 1 && e->B <= 2) p->add(1, NDP_K(k_eng_nn_lat16), g_nn_lat, 1024, (3 * NN_STAGE + 2 * 1024) * 4);
    else if (e->nn_mode == 1) p->add(1, NDP_K(k_eng_nn_lat8), g_nn_lat, 512, (3 * NN_STAGE + 2 * 512) * 4);
    else if (eng_nn_mx8(*e)) p->add(1, NDP_K(k_eng_nn_mx8), dim3((e->t_cap + 511) / 512, e->B), 512, nn2_lds_floats(e->n_cap, 8) * 4);
    else p->add(1, NDP_K(k_eng_nn), dim3(nn1_row_chunks(e->t_cap), e->B), 256, nn_lds, stage_x);

    p->add(2, NDP_K(k_eng_loss), dim3((e->n_cap + 255) / 256 + 1, e->B), 256, 0);          // + 1: the loss / decision workgroup

    if (generic) p->add(3, NDP_K(k_eng_bwd_gen), g_lvl, 256, gen_bwd_floats(e->desc.width) * 4);
    else if (bwd_fused) p->add(3, NDP_K(k_eng_bwd_f), g_8, 512, kSmemBwdFBytes);
    else if (mode & 4) p->add(3, NDP_K(k_eng_bwd2_8), g_8, 512, kSmemBwd8Bytes);
    else p->add(3, NDP_K(k_eng_bwd2), g_lvl, 256, kSmemBwdBytes);

    if (generic || bwd_fused) {}
    else if (mode & 2) p->add(4, NDP_K(k_eng_bwd1_8), g_8, 512, kSmemBwd18Bytes);
    else p->add(4, NDP_K(k_eng_bwd1), g_lvl, 256, kSmemBwdBytes);

    if (bwd_fused && bf_adam_in_tail(*e)) p->add(5, NDP_K(k_eng_update_rest), dim3((upd_rest_count(e->P) + 255) / 256, e->B), 256, 0);
    else p->add(5, NDP_K(k_eng_update), dim3((e->P + 255) / 256, e->B), 256, 0);
    return 0;
}
#undef NDP_K

extern "C" int ndp_engine_plan(const ndp_engine *e, ndp_stage_launch *out, int *n_out) {
    if (!out || !n_out) return fail(NDP_E_INVALID, "ndp_engine_plan: null pointer");
    TickPlan p;
    if (int rc = plan_tick(e, &p)) return rc;
    for (int i = 0; i < p.n; ++i) out[i] = p.l[i].at;
    *n_out = p.n;
    return 0;
}

// n_ticks ticks from ONE plan; ev (optional): NDP_TICK_KERNELS + 1 events per tick, one ahead of every stage and one behind the last
// (an empty stage's two records stand back to back).  Only the launches of stages [stage_lo, stage_hi] are made.
static int engine_launch_ticks(const ndp_engine *e, int tick0, int n_ticks, hipStream_t s, hipEvent_t *ev, int stage_lo = 0, int stage_hi = NDP_TICK_KERNELS - 1) {
    TickPlan p;
    if (int rc = plan_tick(e, &p)) return rc;
    for (int i = 0; i < p.n; ++i)
        if (p.l[i].at.lds_bytes) if (int rc = set_smem(p.l[i].fn, p.l[i].at.lds_bytes)) return rc;
    for (int k = 0; k < n_ticks; ++k) {
        int parity = (tick0 + k) & 1;
        const TickLaunch *l = p.l;
        for (int stage = 0; stage < NDP_TICK_KERNELS; ++stage) {
            if (ev) (void)hipEventRecord(*ev++, s);
            for (; l < p.l + p.n && l->at.stage == stage; ++l) {
                if (stage < stage_lo || stage > stage_hi) continue;
                const dim3 grid(l->at.grid[0], l->at.grid[1], l->at.grid[2]);
                void *args[] = {const_cast<ndp_engine *>(e), &parity, const_cast<int *>(&l->at.extra)};
                (void)hipLaunchKernel(l->fn, grid, dim3(l->at.block), args, l->at.lds_bytes, s);
            }
        }
        if (ev) (void)hipEventRecord(*ev++, s);
    }
    HIP_TRY(hipGetLastError(), "engine launch");
    return 0;
}

extern "C" int ndp_engine_nn_workspace(int n_cap, int t_cap, long long *row_floats) {
    if (n_cap < 0 || t_cap < 0 || n_cap % NDP_TILE || t_cap % NDP_TILE || !row_floats)
        return fail(NDP_E_INVALID, "ndp_engine_nn_workspace: capacities must be multiples of 64");
    *row_floats = 2LL * nn1_row_chunks(t_cap) * n_cap;          // NnPart = {float, int} per (target chunk, source)
    return 0;
}

extern "C" int ndp_chamfer_nn_onepass(const float *x, int S, const float *y, int T, float *d2x, int *idx_x, float *d2y,
                                      int *idx_y, float *ws_row, void *stream) {
    if (S <= 0 || T <= 0 || !x || !y || !d2x || !idx_x || !d2y || !idx_y || !ws_row)
        return fail(NDP_E_INVALID, "ndp_chamfer_nn_onepass: bad arguments");
    const int n_cap = (S + NDP_TILE - 1) / NDP_TILE * NDP_TILE;
    const int stage_x = nn1_stage_x(n_cap) ? 1 : 0;
    const int lds = nn1_lds_floats(n_cap, stage_x) * 4;
    if (lds > 160 * 1024) return fail(NDP_E_UNSUPPORTED, "ndp_chamfer_nn_onepass: S too large for the column table in LDS");
    if (int rc = set_smem((const void *)k_nn1, lds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nn1, dim3((T + NN1_YCH - 1) / NN1_YCH), dim3(256), lds, s, x, S, y, T, n_cap, ws_row, d2y, idx_y, stage_x);
    hipLaunchKernelGGL(k_nn1_rows, dim3((S + 255) / 256), dim3(256), 0, s, S, T, n_cap, ws_row, d2x, idx_x);
    HIP_TRY(hipGetLastError(), "k_nn1 launch");
    return 0;
}

extern "C" int ndp_chamfer_nn_matrix(const float *x, int S, const float *y, int T, float *d2x, int *idx_x, float *d2y,
                                     int *idx_y, float *ws_row, void *stream) {
    if (S <= 0 || T <= 0 || !x || !y || !d2x || !idx_x || !d2y || !idx_y || !ws_row)
        return fail(NDP_E_INVALID, "ndp_chamfer_nn_matrix: bad arguments");
    const int n_cap = (S + NDP_TILE - 1) / NDP_TILE * NDP_TILE;
    const int lds = nn2_lds_floats(n_cap) * 4;
    if (int rc = set_smem((const void *)k_nn2, lds)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nn2, dim3((T + NN1_YCH - 1) / NN1_YCH), dim3(256), lds, s, x, S, y, T, n_cap, ws_row, d2y, idx_y);
    hipLaunchKernelGGL(k_nn1_rows, dim3((S + 255) / 256), dim3(256), 0, s, S, T, n_cap, ws_row, d2x, idx_x);
    HIP_TRY(hipGetLastError(), "k_nn2 launch");
    return 0;
}
extern "C" int ndp_engine_nn_matrix_fits(int) { return 1; }     // the sources are walked in passes: the static_asserts beside nn2_lds_floats

extern "C" int ndp_engine_nn_cells_fits(int n_cap, int t_cap) { return nnc_fits(n_cap, t_cap) ? 1 : 0; }
extern "C" int ndp_chamfer_nn_cells_workspace(int T, long long *floats) {
    if (T < 0 || !floats) return fail(NDP_E_INVALID, "ndp_chamfer_nn_cells_workspace: bad arguments");
    *floats = nnc_ws_floats(T);
    return 0;
}
extern "C" int ndp_chamfer_nn_cells(const float *x, int S, const float *y, int T, const int *prev_idx_x, const int *prev_idx_y,
                                    float *d2x, int *idx_x, float *d2y, int *idx_y, float *workspace, void *stream) {
    if (S <= 0 || T <= 0 || !x || !y || !d2x || !idx_x || !d2y || !idx_y || !workspace || !aligned16(workspace))
        return fail(NDP_E_INVALID, "ndp_chamfer_nn_cells: bad arguments (the workspace must be 16-byte aligned)");
    if (!nnc_fits(S, T)) return fail(NDP_E_UNSUPPORTED, "ndp_chamfer_nn_cells: S and T must be <= 2048 (ndp_engine_nn_cells_fits)");
    if (int rc = set_smem((const void *)k_nn_cells_build, NNC_LDS_BYTES)) return rc;
    if (int rc = set_smem((const void *)k_nn_cells, NNC_LDS_BYTES)) return rc;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_nn_cells_build, dim3(1), dim3(NNC_NT), NNC_LDS_BYTES, s, y, T, workspace);
    hipLaunchKernelGGL(k_nn_cells, dim3(2), dim3(NNC_NT), NNC_LDS_BYTES, s, x, S, y, T, prev_idx_x, prev_idx_y, d2x, idx_x, d2y, idx_y, workspace);
    HIP_TRY(hipGetLastError(), "k_nn_cells launch");
    return 0;
}
extern "C" int ndp_engine_nn_cells_wide_fits(int n_cap, int t_cap) { return nnw_fits(n_cap, t_cap) ? 1 : 0; }
extern "C" int ndp_chamfer_nn_cells_wide_workspace(int S, int T, long long *floats) {
    if (S < 0 || T < 0 || !floats) return fail(NDP_E_INVALID, "ndp_chamfer_nn_cells_wide_workspace: bad arguments");
    *floats = nnw_ws_floats(S, T);
    return 0;
}
extern "C" int ndp_chamfer_nn_cells_wide(const float *x, int S, const float *y, int T, const int *prev_idx_x, const int *prev_idx_y,
                                         float *d2x, int *idx_x, float *d2y, int *idx_y, float *workspace, void *stream) {
    if (S <= 0 || T <= 0 || !x || !y || !d2x || !idx_x || !d2y || !idx_y || !workspace || !aligned16(workspace))
        return fail(NDP_E_INVALID, "ndp_chamfer_nn_cells_wide: bad arguments (the workspace must be 16-byte aligned)");
    if (!nnw_fits(S, T)) return fail(NDP_E_UNSUPPORTED, "ndp_chamfer_nn_cells_wide: S and T must be <= 8192 (ndp_engine_nn_cells_wide_fits)");
    if (int rc = set_smem((const void *)k_nn_cells_wide, NNW_LDS_BYTES)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int Q = nnw_chunks(S, T);
    hipLaunchKernelGGL(k_nnw_build, dim3(1), dim3(NNW_NT), NNW_SORT_LDS_BYTES, s, y, T, workspace);
    hipLaunchKernelGGL(k_nnw_sort, dim3(1), dim3(NNW_NT), NNW_SORT_LDS_BYTES, s, x, S, T, workspace);
    hipLaunchKernelGGL(k_nn_cells_wide, dim3(2 * Q), dim3(NNW_NT), NNW_LDS_BYTES, s, x, S, y, T, prev_idx_x, prev_idx_y, d2x, idx_x, d2y, idx_y,
                       workspace, Q);
    HIP_TRY(hipGetLastError(), "k_nn_cells_wide launch");
    return 0;
}
extern "C" int ndp_engine_nn_onepass_fits(int n_cap) { return nn1_lds_floats(n_cap, nn1_stage_x(n_cap)) * 4 <= 160 * 1024 ? 1 : 0; }

extern "C" int ndp_engine_run(const ndp_engine *e, int tick0, int n_ticks, void *stream) {
    return engine_launch_ticks(e, tick0, n_ticks, (hipStream_t)stream, nullptr);
}

// ONE tick, only the launches of stages [stage_lo, stage_hi] (0 forward, 1 nearest neighbours, 2 loss / decision / dL/dx', 3 bwd2,
// 4 bwd1, 5 update): a test and measurement aid -- the buffers each kernel leaves behind (activations, dO, dz1, gradient partials)
// can be inspected between the stages.  Running the stages 0..5 of a tick in order, in any grouping, is ndp_engine_run(e, tick, 1).
extern "C" int ndp_engine_run_stages(const ndp_engine *e, int tick, int stage_lo, int stage_hi, void *stream) {
    if (stage_lo < 0 || stage_hi >= NDP_TICK_KERNELS || stage_lo > stage_hi) return fail(NDP_E_INVALID, "ndp_engine_run_stages: stages are 0..5, lo <= hi");
    return engine_launch_ticks(e, tick, 1, (hipStream_t)stream, nullptr, stage_lo, stage_hi);
}

// Profiling variant of ndp_engine_run: HIP events around every kernel of every tick, recorded on the launch stream;
// ms_out[NDP_TICK_KERNELS] receives the SUMMED duration of k_eng_fwd, k_eng_nn, k_eng_loss, k_eng_bwd2, k_eng_bwd1,
// k_eng_update.  Synchronises the stream before returning.  Used by bench.py for the roofline figures only.
extern "C" int ndp_engine_run_timed(const ndp_engine *e, int tick0, int n_ticks, void *stream, float *ms_out) {
    if (!e || !ms_out || n_ticks < 1 || n_ticks > 4096) return fail(NDP_E_INVALID, "ndp_engine_run_timed: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const int per = NDP_TICK_KERNELS + 1;
    hipEvent_t *ev = new hipEvent_t[(size_t)n_ticks * per];
    for (int i = 0; i < n_ticks * per; ++i) (void)hipEventCreate(&ev[i]);
    int rc = engine_launch_ticks(e, tick0, n_ticks, s, ev);
    hipError_t err = hipStreamSynchronize(s);
    for (int j = 0; j < NDP_TICK_KERNELS; ++j) ms_out[j] = 0.f;
    if (rc == 0 && err == hipSuccess) {
        for (int k = 0; k < n_ticks; ++k)
            for (int j = 0; j < NDP_TICK_KERNELS; ++j) {
                float ms = 0.f;
                (void)hipEventElapsedTime(&ms, ev[(size_t)k * per + j], ev[(size_t)k * per + j + 1]);
                ms_out[j] += ms;
            }
    }
    for (int i = 0; i < n_ticks * per; ++i) (void)hipEventDestroy(ev[i]);
    delete[] ev;
    if (rc) return rc;
    HIP_TRY(err, "ndp_engine_run_timed sync");
    return 0;
}
