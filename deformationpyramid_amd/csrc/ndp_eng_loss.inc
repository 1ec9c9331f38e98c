// ndp_eng_loss.inc -- the engine's loss stage: loss, early-stop decision and dL/dx' of every pair (k_eng_loss).  Behind
// ndp_nn_matrix.inc: the fold of the row partials asks which nearest-neighbour kernel wrote them.
// Does the engine's nearest-neighbour stage run as k_eng_nn_mx8 (one workgroup and ONE row partial per 512 targets)?  The launcher and
// the loss stage's fold of the row partials ask the same question.  The last clause holds for every n_cap (the static_assert beside
// nn2_lds_floats): there is no other kernel of nn_mode 2.  It stays written out because the compiler does not fold it, and k_eng_loss
// without it is other machine code.
__host__ __device__ inline bool eng_nn_mx8(const ndp_engine &e) {
    return e.w_cd != 0.f && e.t_cap > 0 && e.nn_mode == 2 && nn2_lds_floats(e.n_cap, 8) * 4 <= 160 * 1024;
}

// Loss, early-stop decision and dL/dx' for every pair (one launch per tick).
//   last workgroup of a pair: loss (registration.py:193-212; loss.py:185-258), the stop rule in double
//                     (registration.py:226-232) and the pair's next state;
//   the others      : the gradient of the loss wrt their 256 warped points -- own nearest-neighbour
//                     term, then the targets whose nearest source point it is, in ascending target
//                     index (the order a sequential CPU scatter-add produces), no atomics.
#define LG_CHUNK 2048
struct LossSmem {
    float red[256];
    int cnt[256], start[256];                                             // per-point bucket sizes / offsets
    int order[LG_CHUNK];                                                  // targets grouped by their nearest source point
    __attribute__((aligned(16))) float rows[256 * NDP_LROW];              // per-thread head rows
};
// block reductions over the 256 ACTIVE threads of a workgroup (t: their index; the others only keep the barriers company)
__device__ __forceinline__ float block_sum_256_t(float v, float *scratch, int t, bool act) {
    if (act) scratch[t] = v;
    __syncthreads();
#pragma unroll
    for (int s = 128; s >= 64; s >>= 1) {
        if (act && t < s) scratch[t] = scratch[t] + scratch[t + s];
        __syncthreads();
    }
    // the tree's last six levels live in one wave: lane shuffles instead of LDS + a barrier per level (lane t < s adds the value of lane
    // t + s exactly as scratch[t] + scratch[t + s] did: the same association, the same bits)
    if (act && t < 64) {
        float x = scratch[t];
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) x = x + __shfl_down(x, s);
        if (t == 0) scratch[0] = x;
    }
    __syncthreads();
    const float r = scratch[0];
    __syncthreads();
    return r;
}
__device__ __forceinline__ float l1_sum_t(const float *d2, int n, float trunc, float *scratch, int t, bool act) {
    float s = 0.f;
    for (int i0 = act ? t : n; i0 < n; i0 += 8 * 256) {             // eight values requested together, added in index order (one global round
        float v[8];                                                 // trip per 2048 entries instead of eight: round 6)
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = i0 + 256 * u < n ? d2[i0 + 256 * u] : 0.f;
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (i0 + 256 * u < n) s += (v[u] >= trunc) ? 0.f : sqrtf(v[u]);
    }
    return block_sum_256_t(s, scratch, t, act);
}
__device__ __forceinline__ float sq_sum_t(const float *x, const float *tt, int K, float *scratch, int t, bool act) {
    float s = 0.f;
    for (int k = act ? t : K; k < K; k += 256) {
        const float e0 = x[3 * k] - tt[3 * k], e1 = x[3 * k + 1] - tt[3 * k + 1], e2 = x[3 * k + 2] - tt[3 * k + 2];
        s += fmaf(e2, e2, fmaf(e1, e1, e0 * e0));
    }
    return block_sum_256_t(s, scratch, t, act);
}
// One virtual 256-thread block of the loss stage: vb < nvb - 1 the gradient of 256 warped points, vb == nvb - 1 loss + decision.
// t: index among the block's 256 active threads; act = false: a thread that only takes part in the barriers.
__device__ __forceinline__ void eng_loss_body(const ndp_engine &e, int parity, int b, int vb, int nvb, int t, bool act, LossSmem &sm_) {
    float *red = sm_.red, *rows = sm_.rows;
    int *cnt = sm_.cnt, *start = sm_.start, *order = sm_.order;
    PT_INIT;
    PT_DECL;
    // Only the scalar fields are read here; the per-level array travels memory to memory in the one thread that writes the next state
    // (a by-value copy of the struct parked 80 bytes in scratch in EVERY thread of the launch, behind a wait for its loads: round 6).
    const ndp_pair_state *stp = e.state + (size_t)parity * e.B + b;
    struct { int level, iter, break_counter, adam_t, cur, total_steps, total_evals; double loss_prev; } st;
    st.level = stp->level; st.iter = stp->iter; st.break_counter = stp->break_counter; st.adam_t = stp->adam_t; st.cur = stp->cur;
    st.total_steps = stp->total_steps; st.total_evals = stp->total_evals; st.loss_prev = stp->loss_prev;
    const ndp_pair_geom gm = e.geom[b];                                  // (requested next to the state, not behind the test on it)
    ndp_pair_state *nst = e.state + (size_t)(parity ^ 1) * e.B + b;
    if (st.level >= e.m) {
        if (vb == nvb - 1 && t == 0 && act) { *nst = *stp; nst->decision = NDP_DEC_IDLE; }
        return;
    }
    const int n = gm.K + gm.S;
    const float *x_out = e.pts + ((size_t)b * 2 + (st.cur ^ 1)) * e.n_cap * 3;
    const float *ldmk_t = e.ldmk_t + (size_t)b * e.n_cap * 3;
    const float *tgt = e.tgt + (size_t)b * e.t_cap * 3;
    const float *d2y = e.d2y + (size_t)b * e.t_cap;
    const int *idx_y = e.idx_y + (size_t)b * e.t_cap;
    // nearest target of a source: folded here from the one-pass kernel's per-chunk partials (nn_row_fold)
    const NnPart *rowpart = reinterpret_cast<const NnPart *>(e.nn_row) + (size_t)b * nn1_row_chunks(e.t_cap) * e.n_cap;
    const bool rows_final = e.nn_mode == 1 || e.nn_cells != 0 || e.nn_cells_wide != 0;       // latency shape / cell search: d2x / idx_x already hold the answer
    const int rows_cstep = eng_nn_mx8(e) ? 2 : 1;    // the 8-wave matrix-pipe kernel leaves one partial per 512 targets
    const bool use_cd = gm.S > 0 && e.w_cd != 0.f;
    const HeadCfg hcl = make_head_cfg(desc_at_level(e.desc, st.level));
    const bool use_reg = e.w_reg > 0.f && hcl.nonrig;
    const float *hrec = e.heads + (size_t)b * e.n_cap * NDP_HROW;

    if (vb == nvb - 1) {                 // the extra workgroup of the pair: loss + decision, concurrently with the gradient workgroups
        float loss = 0.f;
        PT(0);
        if (gm.K > 0) loss = sq_sum_t(x_out, ldmk_t, gm.K, red, t, act) * (1.0f / (float)gm.K);
        if (use_cd) {
            float sx = 0.f;
            if (rows_final) {
                for (int i = act ? t : gm.S; i < gm.S; i += 256) {
                    const float v = e.d2x[(size_t)b * e.n_cap + i];
                    sx += (v >= e.trunc) ? 0.f : sqrtf(v);
                }
            } else {
                for (int i0 = act ? t : gm.S; i0 < gm.S; i0 += 2 * 256) {                 // same per-thread order as one source at a time
                    int ii[2];
                    NnPart r[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) ii[s] = i0 + 256 * s < gm.S ? i0 + 256 * s : -1;
                    nn_row_fold_n<2>(rowpart, e.n_cap, gm.T, ii, r, rows_cstep);
#pragma unroll
                    for (int s = 0; s < 2; ++s)
                        if (ii[s] >= 0) sx += (r[s].d2 >= e.trunc) ? 0.f : sqrtf(r[s].d2);
                }
            }
            PT(1);
            sx = block_sum_256_t(sx, red, t, act);
            PT(2);
            const float sy = l1_sum_t(d2y, gm.T, e.trunc, red, t, act);
            PT(3);
            const float lcd = sx / (float)gm.S + sy / (float)gm.T;
            loss = gm.K > 0 ? loss + e.w_cd * lcd : lcd;
        }
        if (use_reg) {                                   // registration.py:216-220: + w_reg * BCELoss(nonrigidity, 0)
            float acc = 0.f;
            for (int i = act ? t : n; i < n; i += 256) {
                const float nr = 1.0f / (1.0f + expf(-hrec[(size_t)i * NDP_HROW + hcl.row_nr]));
                float l1 = logf(1.0f - nr);
                if (l1 < -100.0f) l1 = -100.0f;
                acc += -l1;
            }
            acc = block_sum_256_t(acc, red, t, act);
            loss = loss + e.w_reg * (acc * (1.0f / (float)n));
        }
        if (t == 0 && act) {
            int bc = st.break_counter;
            double lp = st.loss_prev;
            bool stop = false;
            if (e.early_stop) {
                const double L = (double)loss;
                if (L < 1e-4) stop = true;
                else {
                    if (fabs(lp - L) < lp * e.break_threshold_ratio) bc += 1;
                    if (bc >= e.max_break_count) stop = true;
                    else lp = L;
                }
            }
            const int decision = stop ? NDP_DEC_ADVANCE : (st.iter + 1 >= e.iters ? NDP_DEC_STEP_ADVANCE : NDP_DEC_STEP);
            // the next state = this one with the fields below replaced, written field by field (a private copy of the struct with its
            // per-level array lived in scratch, and every thread of every workgroup paid the 64-byte store that initialised it)
            *nst = *stp;
            nst->loss = loss;
            nst->decision = decision;
            nst->total_evals = st.total_evals + 1;
            nst->step_level = st.level;
            nst->step_t = st.adam_t + 1;
            if (decision != NDP_DEC_ADVANCE) nst->total_steps = st.total_steps + 1;
            if (decision == NDP_DEC_STEP) {
                nst->iter = st.iter + 1;
                nst->adam_t = st.adam_t + 1;
                nst->break_counter = bc;
                nst->loss_prev = lp;
            } else {                                       // registration.py:242-249 + :179-180
                nst->level = st.level + 1;
                nst->iter = 0;
                nst->adam_t = 0;
                nst->break_counter = 0;
                nst->loss_prev = 1e6;
                nst->cur = st.cur ^ 1;
            }
            if (decision != NDP_DEC_STEP) nst->evals_per_level[st.level] = st.iter + 1;
        }
        PT(4);
        PT_FLUSH(48);
        return;
    }
    // ---- gradient of the loss wrt the warped points of this workgroup
    const int p = act ? vb * 256 + t : e.n_cap;                          // (an inactive thread owns no point)
    if (vb * 256 >= n) return;
    float *dO_row = e.dO + ((size_t)b * e.n_cap + p) * NDP_NHMAX;
    float w[3] = {0.f, 0.f, 0.f}, g[3] = {0.f, 0.f, 0.f};
    // Requested up front, next to the warped point: the point's level input, which only the head backward at the end needs -- behind
    // the scatter it and the head record (below) were one more global round trip in the open (round 6).
    float xv[3] = {0.f, 0.f, 0.f};
    if (p < n) {
        const float *xin = e.pts + ((size_t)b * 2 + st.cur) * e.n_cap * 3 + 3 * p;
        w[0] = x_out[3 * p]; w[1] = x_out[3 * p + 1]; w[2] = x_out[3 * p + 2];
        xv[0] = xin[0]; xv[1] = xin[1]; xv[2] = xin[2];
    }
    const int i_self = p - gm.K;                     // sample index (negative for landmarks)
    // Every phase below is a chain of 1-2 us global round trips (tools/phase_timing.py), so what can be requested now is: the
    // chunk's nearest-source indices (local point of target c0 + t + 256 k, -1: not ours) travel with the row partials.
    // workgroup holds at least one sample AND there is a target to scatter (T == 0: the chunk loop below would never run, and with it
    // the head rows would never reach LDS -- ndp_engine_load refuses such a pair, this keeps a state written around it defined)
    const bool scatter = use_cd && gm.T > 0 && vb * 256 + 255 >= gm.K;
    const int i_lo = vb * 256 - gm.K;                      // sample index of thread 0
    // (UNCONDITIONAL loads at a clamped index -- idx_y is padded with -1 up to t_cap: as `cond ? idx_y[j] : -1` every one of the eight
    //  became a branch around a load with its own wait, eight dependent global round trips at the top of every gradient workgroup,
    //  a third of its time: round 6)
    int li[LG_CHUNK / 256];
#pragma unroll
    for (int k = 0; k < LG_CHUNK / 256; ++k) li[k] = -1;
    if (scatter) {
        const int jcap = e.t_cap - 1;
        int raw[LG_CHUNK / 256];
#pragma unroll
        for (int k = 0; k < LG_CHUNK / 256; ++k) raw[k] = idx_y[min(t + 256 * k, jcap)];
#pragma unroll
        for (int k = 0; k < LG_CHUNK / 256; ++k) li[k] = act && t + 256 * k < gm.T ? raw[k] - i_lo : -1;
    }
    if (p < gm.K) {
        const float invK = 1.0f / (float)gm.K;
#pragma unroll
        for (int a = 0; a < 3; ++a) g[a] = 2.0f * (w[a] - ldmk_t[3 * p + a]) * invK;
    } else if (p < n && use_cd) {
        NnPart nx;
        if (rows_final) { nx.d2 = e.d2x[(size_t)b * e.n_cap + i_self]; nx.idx = e.idx_x[(size_t)b * e.n_cap + i_self]; }
        else {
            nx = nn_row_fold(rowpart, e.n_cap, gm.T, i_self, rows_cstep);
            e.d2x[(size_t)b * e.n_cap + i_self] = nx.d2;             // kept for inspection; nothing on the path reads them
            e.idx_x[(size_t)b * e.n_cap + i_self] = nx.idx;
        }
        const float d2 = nx.d2;
        if (!(d2 >= e.trunc)) {
            const float *yy = tgt + 3 * nx.idx;
            const float inv = 1.0f / ((float)gm.S * sqrtf(d2));
#pragma unroll
            for (int a = 0; a < 3; ++a) g[a] = (w[a] - yy[a]) * inv;
        }
    }
    // the head record travels under the counting sort's first passes (16 registers that the row fold above had no room for)
    static_assert(NDP_NHMAX == 16, "four float4 per head row");
    float4 hr0 = make_float4(0.f, 0.f, 0.f, 0.f), hr1 = hr0, hr2 = hr0, hr3 = hr0;
    if (p < n) {
        const float4 *hsrc = reinterpret_cast<const float4 *>(hrec + (size_t)p * NDP_HROW);
        hr0 = hsrc[0]; hr1 = hsrc[1]; hr2 = hsrc[2]; hr3 = hsrc[3];
    }
#define LOSS_HR_STORE() do { if (p < n) { float4 *hd_ = reinterpret_cast<float4 *>(rows + t * NDP_LROW); hd_[0] = hr0; hd_[1] = hr1; hd_[2] = hr2; hd_[3] = hr3; } } while (0)
    if (!scatter) LOSS_HR_STORE();
    PT(0);
    if (scatter) {
        // Targets whose nearest source point belongs to this workgroup, grouped per point by a counting
        // sort in LDS (O(T) per workgroup instead of a T-long scan per point), each group then sorted so
        // that the contributions are added in ascending target index -- the order of a sequential CPU
        // scatter-add, hence bit-identical to the oracle -- without any float atomics.
        const bool live = p >= gm.K && p < n;
        for (int c0 = 0; c0 < gm.T; c0 += LG_CHUNK) {
            const int cn = min(LG_CHUNK, gm.T - c0);
            if (c0 > 0) {
#pragma unroll
                for (int k = 0; k < LG_CHUNK / 256; ++k) {
                    const int j = t + 256 * k;
                    const int raw = idx_y[min(c0 + j, e.t_cap - 1)];
                    li[k] = act && j < cn ? raw - i_lo : -1;
                }
            }
            __syncthreads();
            if (act) cnt[t] = 0;
            __syncthreads();
            // pass 1: count
#pragma unroll
            for (int k = 0; k < LG_CHUNK / 256; ++k)
                if (li[k] >= 0 && li[k] < 256) atomicAdd(&cnt[li[k]], 1);
            __syncthreads();
            PT(1);
            // exclusive scan of cnt -> start: inclusive scan inside each wave by lane shuffles, the four wave totals through LDS (two
            // barriers; until round 6 a Hillis-Steele scan through LDS with sixteen of them -- integers: the same offsets)
            const int mine = cnt[t];
            int inc = mine;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const int v = __shfl_up(inc, d);
                if ((t & 63) >= d) inc += v;
            }
            int *wsum = reinterpret_cast<int *>(red);                     // (the gradient workgroups have no other use for `red`)
            if (act && (t & 63) == 63) wsum[t >> 6] = inc;
            __syncthreads();
            int my_start = inc - mine;
#pragma unroll
            for (int w2 = 0; w2 < 3; ++w2) my_start += w2 < (t >> 6) ? wsum[w2] : 0;
            if (act) start[t] = my_start;                                 // becomes the fill cursor
            if (c0 == 0) LOSS_HR_STORE();
            __syncthreads();
            PT(2);
            // pass 2: fill
#pragma unroll
            for (int k = 0; k < LG_CHUNK / 256; ++k)
                if (li[k] >= 0 && li[k] < 256) order[atomicAdd(&start[li[k]], 1)] = c0 + t + 256 * k;
            __syncthreads();
            PT(3);
            if (live && mine > 0) {
                int *bk = order + my_start;                               // this thread's private range
                for (int a = 1; a < mine; ++a) {                          // insertion sort, ascending target index
                    const int v = bk[a];
                    int q = a - 1;
                    while (q >= 0 && bk[q] > v) { bk[q + 1] = bk[q]; --q; }
                    bk[q + 1] = v;
                }
                for (int a0 = 0; a0 < mine; a0 += 4) {                    // four entries requested together, added in order
                    float d2q[4], yq[4][3];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const int j = bk[min(a0 + u, mine - 1)];
                        d2q[u] = d2y[j];
                        yq[u][0] = tgt[3 * j]; yq[u][1] = tgt[3 * j + 1]; yq[u][2] = tgt[3 * j + 2];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        if (a0 + u < mine && !(d2q[u] >= e.trunc)) {
                            const float inv = 1.0f / ((float)gm.T * sqrtf(d2q[u]));
                            g[0] = fmaf(w[0] - yq[u][0], inv, g[0]);
                            g[1] = fmaf(w[1] - yq[u][1], inv, g[1]);
                            g[2] = fmaf(w[2] - yq[u][2], inv, g[2]);
                        }
                    }
                }
            }
        }
        if (gm.K > 0 && live) { g[0] = e.w_cd * g[0]; g[1] = e.w_cd * g[1]; g[2] = e.w_cd * g[2]; }   // registration.py:197
    }
    PT(4);
    // ---- per-point head backward: dO = mlp_scale * dL/d(scaled head outputs); zero rows pad the last tile
    float amax = 0.f;
    if (p < n) {
        float g_nr = 0.f;
        if (use_reg) {                                   // d/dnr of w_reg * mean(-log(1 - nr)), torch's BCE backward clamp
            const float nr = 1.0f / (1.0f + expf(-rows[t * NDP_LROW + hcl.row_nr]));
            const float den = (1.0f - nr) * nr;
            g_nr = e.w_reg * ((1.0f / (float)n) * (nr / (den > 1e-12f ? den : 1e-12f)));
        }
        point_head_bwd(hcl, nullptr, xv, g, g_nr, rows + t * NDP_LROW, dO_row, &amax);
    } else if (p < e.n_cap) {
#pragma unroll
        for (int j = 0; j < NDP_NHMAX; j += 4) *reinterpret_cast<float4 *>(dO_row + j) = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (e.gmax) {                                        // the pair's max |dO|: the split backward scales its gradient operands by it
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) amax = fmaxf(amax, __shfl_xor(amax, o));
        float *wm = rows;                                // (every thread is done with its row; one atomic per workgroup, not per wave)
        __syncthreads();
        if (act && (t & 63) == 0) wm[t >> 6] = amax;
        __syncthreads();
        if (t == 0 && act) {
            const float m4 = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
            if (m4 > 0.f) atomicMax(e.gmax + b, __float_as_uint(m4));      // non-negative floats order like their bit patterns
        }
    }
    PT(5);
    PT_FLUSH(36);
}

extern "C" __global__ void __launch_bounds__(256, 5)                     // five waves per SIMD: what the 31 KB of LDS allow (<= 96 registers)
k_eng_loss(ndp_engine e, int parity) {
    __shared__ LossSmem sm_;
    int b, vb;
    xcd_pair_block(gridDim.x, gridDim.y, b, vb);
    eng_loss_body(e, parity, b, vb, gridDim.x, threadIdx.x, true, sm_);
}
