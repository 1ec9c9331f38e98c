// ndp_flow_metrics.inc -- scene-flow metrics on the device: k_flow_metrics and ndp_flow_metrics.
// ------------------------------------------------------------------------------------------------
// Scene-flow metrics on the device (loss.py:382-403, 431-471): per subset {all, overlap, ~overlap} the sum of the end-point
// errors and the counts behind AccS / AccR / Outlier.  One workgroup, fixed order, double accumulation.
// out[3][5] doubles: {sum err, #(err < .025 | rel < .025), #(err < .05 | rel < .05), #(rel > .3), #points}.
// ------------------------------------------------------------------------------------------------
extern "C" __global__ void __launch_bounds__(1024)
k_flow_metrics(const float *flow, const float *gt, const unsigned char *overlap, int n, double *out) {
    __shared__ double red[1024];
    double acc[3][5];
    for (int s = 0; s < 3; ++s)
        for (int k = 0; k < 5; ++k) acc[s][k] = 0.0;
    for (int i = threadIdx.x; i < n; i += 1024) {
        const float d0 = flow[3 * (size_t)i] - gt[3 * (size_t)i], d1 = flow[3 * (size_t)i + 1] - gt[3 * (size_t)i + 1],
                    d2 = flow[3 * (size_t)i + 2] - gt[3 * (size_t)i + 2];
        const float g0 = gt[3 * (size_t)i], g1 = gt[3 * (size_t)i + 1], g2 = gt[3 * (size_t)i + 2];
        const float err = sqrtf((d0 * d0 + d1 * d1) + d2 * d2);
        const float rel = err / (sqrtf((g0 * g0 + g1 * g1) + g2 * g2) + 1e-20f);
        const double v[5] = {(double)err, (err < 0.025f || rel < 0.025f) ? 1.0 : 0.0, (err < 0.05f || rel < 0.05f) ? 1.0 : 0.0,
                             rel > 0.3f ? 1.0 : 0.0, 1.0};
        const int sub = overlap ? (overlap[i] ? 1 : 2) : 0;
        for (int k = 0; k < 5; ++k) {
            acc[0][k] += v[k];
            if (sub == 1) acc[1][k] += v[k];
            if (sub == 2) acc[2][k] += v[k];
        }
    }
    for (int s = 0; s < 3; ++s)
        for (int k = 0; k < 5; ++k) {
            const double tot = block_fold_one<1024>(acc[s][k], red, FoldSum());
            if (threadIdx.x == 0) out[5 * s + k] = tot;
        }
}

extern "C" int ndp_flow_metrics(const float *flow, const float *flow_gt, const unsigned char *overlap, int n, double *out15, void *stream) {
    if (n < 0 || !out15 || (n > 0 && (!flow || !flow_gt))) return fail(NDP_E_INVALID, "ndp_flow_metrics: bad arguments");
    hipLaunchKernelGGL(k_flow_metrics, dim3(1), dim3(1024), 0, (hipStream_t)stream, flow, flow_gt, overlap, n, out15);
    HIP_TRY(hipGetLastError(), "k_flow_metrics launch");
    return 0;
}
