// ndp_eng_update.inc -- the engine's update stage: fold of the gradient partials, Adam step, level hand-over (k_eng_update,
// k_eng_update_rest).
// fold the G partial gradients in index order, Adam step, level hand-over (fresh Adam state).
// (Four parameters per thread on 16-byte accesses: no faster at 128 pairs -- 0.0305 against 0.0315 ms -- and TWICE as slow at batch 1,
//  where the G = 32 partials are folded by a quarter of the threads: 0.023 against 0.012 ms.  One parameter per thread it stays.)
// parameter i of pair b: fold, Adam, hand-over (the whole update stage is this, for every i < P)
__device__ __forceinline__ void eng_update_param(const ndp_engine &e, int b, const ndp_pair_state &ns, const ndp_layer_desc &dl, int i) {
    float *m = e.adam_m + (size_t)b * e.p_stride, *v = e.adam_v + (size_t)b * e.p_stride;
    if (i >= ndp_param_count(&dl)) {                     // level 0 has no gate row: nothing to step, keep moments clean
        if (ns.decision != NDP_DEC_STEP) { m[i] = 0.f; v[i] = 0.f; }
        return;
    }
    if (ns.decision != NDP_DEC_ADVANCE) {
        const float *gp = e.gpart + (size_t)b * e.G * e.p_stride;
        float *p = e.params + ((size_t)b * e.m + ns.step_level) * e.p_stride;
        float pi = p[i], mi = m[i], vi = v[i];                           // (requested with the partials, not behind their fold)
        float g = __builtin_nontemporal_load(gp + i);
        int k = 1;
        // The other partials are requested TOGETHER (clamped index, added in index order while k < G): batch 1 folds G = 32 of them, and as
        // three batches of eight plus a tail of seven single loads that was eleven dependent global round trips (round 6).
        if (e.G > 9) {
            for (; k < e.G; k += 32) {
                float q[32];
#pragma unroll
                for (int u = 0; u < 32; ++u) q[u] = gp[(size_t)min(k + u, e.G - 1) * e.p_stride + i];
#pragma unroll
                for (int u = 0; u < 32; ++u)
                    if (k + u < e.G) g += q[u];
            }
        } else if (e.G > 3) {
            for (; k < e.G; k += 8) {
                float q[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) q[u] = gp[(size_t)min(k + u, e.G - 1) * e.p_stride + i];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    if (k + u < e.G) g += q[u];
            }
        }
        for (; k < e.G; ++k) g += gp[(size_t)k * e.p_stride + i];
        adam_update(pi, g, mi, vi, e.adam_w1, e.adam_b2, e.adam_w2, e.adam_tab[2 * ns.step_t],
                    e.adam_tab[2 * ns.step_t + 1], e.adam_eps);
        p[i] = pi; m[i] = mi; v[i] = vi;
    }
    if (ns.decision != NDP_DEC_STEP) { m[i] = 0.f; v[i] = 0.f; }             // registration.py:176
}
extern "C" __global__ void __launch_bounds__(256)
k_eng_update(ndp_engine e, int parity) {
    const int b = blockIdx.y;
    // (the three fields the step needs, requested side by side and tested once: behind the test on the decision the level and the step
    //  number were a second dependent scalar round trip)
    const ndp_pair_state *nsp = e.state + (size_t)(parity ^ 1) * e.B + b;   // written by k_eng_loss this tick
    ndp_pair_state ns;
    ns.decision = nsp->decision; ns.step_level = nsp->step_level; ns.step_t = nsp->step_t;
    const int i = blockIdx.x * 256 + threadIdx.x;
    if ((ns.decision == NDP_DEC_IDLE) | (i >= e.P) | (ns.step_level < 0) | (ns.step_t < 0)) return;
    eng_update_param(e, b, ns, desc_at_level(e.desc, ns.step_level), i);
}
// The update stage when the fused backward has stepped the two 128 x 128 matrices behind its tile loop (bf_adam_in_tail: G == 1):
// what is left -- [W0 | b0], b1, [b2 | Wh | bh] -- on a COMPACT grid (8 workgroups per pair at six heads instead of 136: the empty
// ones of the full grid cost more than the step itself, 17 us at 256 pairs).  Same eng_update_param, every decision handled there.
__host__ __device__ inline int upd_rest_count(int P) { const ndp_layer_desc dd = {NDP_W, 2, 0, 0, 0, 0.f}; return ndp_off_Wi(&dd, 1) + NDP_W + (P - ndp_off_bi(&dd, 2)); }
extern "C" __global__ void __launch_bounds__(256)
k_eng_update_rest(ndp_engine e, int parity) {
    const int b = blockIdx.y;
    const ndp_pair_state *nsp = e.state + (size_t)(parity ^ 1) * e.B + b;   // written by k_eng_loss this tick
    ndp_pair_state ns;
    ns.decision = nsp->decision; ns.step_level = nsp->step_level; ns.step_t = nsp->step_t;
    const ndp_layer_desc dd = {NDP_W, 2, 0, 0, 0, 0.f};
    const int n0 = ndp_off_Wi(&dd, 1);                              // [0, n0): W0 | b0
    const int c = blockIdx.x * 256 + threadIdx.x;
    const int i = c < n0 ? c : (c < n0 + NDP_W ? ndp_off_bi(&dd, 1) + (c - n0) : ndp_off_bi(&dd, 2) + (c - n0 - NDP_W));
    if ((ns.decision == NDP_DEC_IDLE) | (i >= e.P) | (ns.step_level < 0) | (ns.step_t < 0)) return;
    eng_update_param(e, b, ns, desc_at_level(e.desc, ns.step_level), i);
}
