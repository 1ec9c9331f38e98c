// ndp_abi_common.inc -- what every host entry uses (host-only): g_err / fail / failf / hip_fail / HIP_TRY, check_desc, aligned16,
// check_batch / check_offsets (the batched entries' host-side offsets), set_smem;
// and the entries about the library itself: ndp_version, ndp_last_error, ndp_build_id, ndp_abi_sizes.  Behind ndp_generic.inc
// (check_desc asks gen_supported), ahead of the first file that carries host entries of its own.
// ------------------------------------------------------------------------------------------------
// host side of the C ABI
// ------------------------------------------------------------------------------------------------
static thread_local char g_err[256] = "";
static int fail(int code, const char *msg) {
    snprintf(g_err, sizeof g_err, "%s", msg);
    return code;
}
__attribute__((format(printf, 2, 3))) static int failf(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return code;
}
static int hip_fail(hipError_t e, const char *what) {
    snprintf(g_err, sizeof g_err, "%s: %s", what, hipGetErrorString(e));
    return (int)e;
}
#define HIP_TRY(expr, what)                                   \
    do {                                                      \
        hipError_t _e = (expr);                               \
        if (_e != hipSuccess) return hip_fail(_e, what);      \
    } while (0)

static int check_desc(const ndp_layer_desc *d) {
    if (!d) return fail(NDP_E_INVALID, "null layer descriptor");
    if (gen_is_generic(*d) && !gen_supported(*d))                       // 128 / 3: the MFMA kernels; anything else: csrc/ndp_generic.inc
        return fail(NDP_E_UNSUPPORTED, "width must be 1..256 and depth 1..4 (width=128, depth=3 run on the MFMA kernels, the rest on the generic fp32 kernels)");
    if (d->motion < 0 || d->motion > 2) return fail(NDP_E_INVALID, "bad motion type");
    if (d->motion != NDP_MOTION_SFLOW && (d->rotfmt < NDP_ROT_AXIS_ANGLE || d->rotfmt > NDP_ROT_6D))
        return fail(NDP_E_INVALID, "bad rotation_format");
    return 0;
}
static bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// The batched entries (rigid, matching, KPConv inputs) take B problems as rows of stacked arrays, described by a HOST array the
// entry checks before anything is launched (the kernels read a device copy).  check_batch: B in 1..NDP_MAX_B (a grid dimension, and
// the 16 bits of cloud in KPConv's cell key) and the host array present.  check_offsets: that, and off_host [B + 1] starts at 0 or
// above, is monotone, and gives every problem at least min_rows rows -- `rows` is the entry's name for them in the message.
// max_rows (may be NULL): the largest problem.
#define NDP_MAX_B 65535
static int check_batch(const char *who, const void *host_array, int B) {
    if (B < 1 || B > NDP_MAX_B) return failf(NDP_E_INVALID, "%s: B must lie in 1..%d", who, NDP_MAX_B);
    if (!host_array) return failf(NDP_E_INVALID, "%s: null pointer", who);
    return 0;
}
static int check_offsets(const char *who, const int *off_host, int B, int min_rows, const char *rows, int *max_rows) {
    if (int rc = check_batch(who, off_host, B)) return rc;
    if (off_host[0] < 0) return failf(NDP_E_INVALID, "%s: offsets must start at 0 or above", who);
    int mx = 0;
    for (int b = 0; b < B; ++b) {
        if (off_host[b + 1] < off_host[b]) return failf(NDP_E_INVALID, "%s: offsets must be monotone", who);
        const int k = off_host[b + 1] - off_host[b];
        if (k < min_rows) return failf(NDP_E_INVALID, "%s: every problem needs %s >= %d (problem %d has %d)", who, rows, min_rows, b, k);
        mx = std::max(mx, k);
    }
    if (max_rows) *max_rows = mx;
    return 0;
}

// Raise a kernel's dynamic-LDS attribute to `bytes`, once per thread and size: the table keeps the largest size asked per kernel, and
// a kernel whose size grows with the problem (k_eng_nn, k_nn1, ...) goes to the runtime again when a caller asks for more.  One slot
// per kernel that is ever passed here: 41 named ones (10 level / pyramid, 4 Jacobian / inverse, 2 baseline, k_kpc_forward, k_kpb_edge,
// k_kpb_dw, the 16 a tick plan can name and k_eng_nn_cells_build, 5 NN operators) and the 6 attention families x {scalar, v4} x 4 head
// widths.  A full table only costs the runtime call every time.
static constexpr int kSmemKernels = 41 + 6 * 2 * 4;
static int set_smem(const void *fn, int bytes) {
    static thread_local struct { const void *fn; int bytes; } set[kSmemKernels];
    auto *slot = set;
    while (slot < set + kSmemKernels && slot->fn && slot->fn != fn) ++slot;
    if (slot < set + kSmemKernels && slot->fn == fn && slot->bytes >= bytes) return 0;
    HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes), "hipFuncSetAttribute");
    if (slot < set + kSmemKernels) { slot->fn = fn; slot->bytes = bytes; }
    return 0;
}

#ifdef NDP_PHASE_TIMING
extern "C" int ndp_debug_phase_read(unsigned long long *out64, int reset) {
    if (hipMemcpyFromSymbol(out64, HIP_SYMBOL(g_phase), sizeof(unsigned long long) * 96) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[96] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof z) != hipSuccess) return -1;
    }
    return 0;
}
#endif

#ifndef NDP_BUILD_ID
#define NDP_BUILD_ID "unversioned"
#endif
// ABI versions:
//   201: ndp_load_job gained n_src / n_tgt (88 bytes), `means` in/out
//   202: h2 as a plane image under gemm_mode 7
//   203: gemm_mode bits 512 / 1024, at G == 1 the matrix blocks of gpart are not written
//   204: gemm_mode bits 64 / 128 / 256 / 512 refused, gmax is [B]
//   205: ndp_level_bwd gained the trailing `dx` (dL/dx of the level's input points, may be NULL)
//   206: ndp_pyramid_jac, ndp_pyramid_inverse
//   207: ndp_engine gained nn_cells and its grid buffers, ndp_chamfer_nn_cells
//   208: ndp_engine gained nn_cells_wide (behind the existing fields; its grids: nnc_start / nnc_rec in a larger layout), ndp_chamfer_nn_cells_wide
//   209: ndp_sinkhorn_schedule, ndp_sinkhorn_workspace, ndp_sinkhorn_divergence
//   210: ndp_knn, ndp_normals_from_knn, ndp_point_to_plane
//   211: ndp_rigid_fit, ndp_rigid_score, ndp_ransac_rigid_workspace, ndp_ransac_rigid
//   212: ndp_feat_rowstats, ndp_feat_match_workspace, ndp_feat_match
//   213: ndp_voxel_subsample_workspace, ndp_voxel_subsample, ndp_radius_search_workspace, ndp_radius_search
//   214: ndp_kpconv_forward_workspace, ndp_kpconv_forward
//   215: ndp_attention_forward, ndp_feat_conf_workspace, ndp_feat_conf
//   216: ndp_attention_compat_forward
//   217: ndp_attention_forward_lse, ndp_attention_backward
//   218: ndp_engine_plan (ndp_stage_launch); k_eng_nn_mx is gone, ndp_engine_nn_matrix_fits answers 1 for every n_cap
//   219: ndp_kpconv_backward_workspace, ndp_kpconv_backward
extern "C" int ndp_version(void) { return 219; }
extern "C" const char *ndp_last_error(void) { return g_err; }
static const char k_build_tag[] = "NDP_BUILD_ID=" NDP_BUILD_ID;        // the loader finds this tag in the file without loading it
extern "C" const char *ndp_build_id(void) { return k_build_tag + 13; }
extern "C" int ndp_abi_sizes(int *out) {
    if (!out) return fail(NDP_E_INVALID, "ndp_abi_sizes: null pointer");
    out[0] = (int)sizeof(ndp_layer_desc); out[1] = (int)sizeof(ndp_pair_geom); out[2] = (int)sizeof(ndp_pair_state);
    out[3] = (int)sizeof(ndp_engine);     out[4] = (int)sizeof(ndp_warp_job);  out[5] = (int)sizeof(ndp_load_job);
    return 0;
}
