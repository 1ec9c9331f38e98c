/*
 * ndp_hip.h -- C ABI of libndp_hip.so, the MI355X (gfx950) implementation of the NDP per-pair
 * optimisation hot path.  Plain pointers and sizes only: every `float*`/`int*` below is a DEVICE
 * pointer to contiguous memory owned by the caller, `stream` is a hipStream_t passed as void*,
 * nothing is allocated inside, there is no global state, and every entry point returns
 *     0  success,   <0  invalid argument (NDP_E_*),   >0  a hipError_t from the launch.
 *
 * The reference has no C ABI: its "operator API" for this path is the Python surface of
 * model/registration.py, model/nets.py and model/loss.py.  Each entry point names the reference
 * code it replaces; INTEGRATION.md shows the ctypes binding a maintainer would add.
 *
 * Parameter layout of one level: include/ndp_types.h.  Points are float32 [n][3] row-major.
 * width = 128, depth = 3 (both shipped configs: NDP.yaml:24-25, LNDP.yaml:45-46) run on the MFMA kernels.  Every other
 * 1 <= width <= 256, 1 <= depth <= 4 the YAML can name (the reference builds any: nets.py:75,295-304) runs behind the SAME
 * entry points on generic fp32 kernels (csrc/ndp_generic.inc: the oracle's chains on the fp32 matrix instruction, about a third
 * of the 128 / 3 kernels' rate per layer; gemm_mode and the `split` entries select nothing there).  Their activation store is
 * [depth][n_cap][width] fp32 rows wherever this header says [3][n_cap][128].  Shapes beyond return NDP_E_UNSUPPORTED.
 */
#ifndef NDP_HIP_H
#define NDP_HIP_H

#include "ndp_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define NDP_E_INVALID     (-1)
#define NDP_E_UNSUPPORTED (-2)
#define NDP_MAX_LEVELS    16
#define NDP_TILE          64      /* points per tile; point capacities are multiples of this */
#define NDP_HROW          24      /* floats per point in the saved head record                 */

int ndp_version(void);                 /* 100*major + minor */
const char *ndp_last_error(void);      /* text of the last non-zero return on this thread */
/* Digest of the sources + flags the library was built from (the loader compares it with the tree and rebuilds or
 * refuses a stale library), and sizeof of the six structs that cross the ABI by value, in declaration order:
 * ndp_layer_desc, ndp_pair_geom, ndp_pair_state, ndp_engine, ndp_warp_job, ndp_load_job (the binding checks its mirror). */
const char *ndp_build_id(void);
int ndp_abi_sizes(int *out6);

/* ------------------------------------------------------------------ single-pair operators */

/* NDPLayer.forward for one level on n points (nets.py:111-140; posenc :164-177; MLP :295-304;
 * get_Rotation :144-161; rigid_body.py:19-56,89-119).
 *   x [n][3] -> x_out [n][3].
 *   act  (may be NULL): [3][n_cap][128] saved post-ReLU activations h0,h1,h2 for ndp_level_bwd ([depth][n_cap][width] in general)
 *   heads(may be NULL): [n_cap][NDP_HROW] per-point record: 16 scaled head outputs (rot.., scale,
 *                       trn, nr) followed by the 6 positional-encoding values and 2 pad floats
 *   nonrig_out (may be NULL): [n] gate values sigmoid(0.001 nr_branch(h)) when desc->nonrigidity
 *                       (the second element NDPLayer.forward returns, nets.py:133-140)
 * n_cap = n rounded up to NDP_TILE (row count of act/heads).                                   */
int ndp_level_fwd(const ndp_layer_desc *desc, const float *params, int level, int k0,
                  const float *x, int n, float *x_out, float *act, float *heads, float *nonrig_out,
                  void *stream);

/* Backward of one level given g = dL/dx_out [n][3] (autograd of nets.py:111-140): wrt its parameters, and -- when dx is
 * given -- wrt its input points.  act/heads come from ndp_level_fwd on the same
 * x and params; act is CONSUMED at 128 / 3 (its h2 plane is overwritten with an intermediate; the generic kernels leave it).  dO_work is
 * scratch of [n_cap][16] floats; g_nr (may be NULL) = dL/d(gate) [n] when desc->nonrigidity.  grads_part [n_part][P_stride] receives n_part partial sums
 * (deterministic: workgroup g sums tiles g, g+n_part, ...); ndp_grad_reduce folds them in index order.
 *   dx (may be NULL): [n][3] receives dL/dx, the warp's own dependence on x plus the path through the positional encoding and the
 *       network (f = 2^(level + 1 + k0); every point is written by one thread in a fixed order: reproducible, independent of n_part).
 *       NULL: x is a detached input (the reference's hot path, registration.py:243-249) -- the launches and the results of ABI 204;
 *       level / k0 are read only when dx is given.  The parameter gradients are the same bits either way.                        */
int ndp_level_bwd(const ndp_layer_desc *desc, const float *params, int level, int k0,
                  const float *x, int n, float *act, const float *heads, const float *g, const float *g_nr,
                  float *dO_work, float *grads_part, int n_part, int p_stride, void *stream, float *dx);

/* grads[P] = sum_{g<n_part} grads_part[g][:]  (fixed order). */
int ndp_grad_reduce(const float *grads_part, int n_part, int p_stride, int P, float *grads, void *stream);

/* Whole pyramid forward, levels 0..m-1 (Deformation_Pyramid.warp, nets.py:36-48; the final
 * inference warp of registration.py:254-255).  params_all: level l at params_all + l*p_stride.
 * desc->nonrigidity = 1 means "every level but the first carries the gate" (nets.py:26).        */
int ndp_pyramid_fwd(const ndp_layer_desc *desc, int m, int k0, const float *params_all, int p_stride,
                    const float *x, int n, float *x_out, void *stream);

/* Batched, single-launch form of the final inference warp: every job is one cloud pushed through all m
 * levels inside ONE kernel (grid = tiles x jobs; a workgroup keeps its 64 points in LDS from level to
 * level, so there is no intermediate HBM traffic and one launch fills the chip with several pairs).
 * Folds the centring and the un-centring of registration.py:150-153 / :258:
 *     x_out = pyramid(x - shift_in) + shift_out          (either shift may be NULL).
 * `jobs` is a HOST array (copied into the kernel arguments); all jobs share desc / m / k0 / p_stride. */
typedef struct ndp_warp_job {
    const float *params;             /* [m][p_stride] */
    const float *x;                  /* [n][3] */
    float *x_out;                    /* [n][3] (may alias x) */
    const float *shift_in;           /* [3] device, or NULL */
    const float *shift_out;          /* [3] device, or NULL */
    int n, pad;
} ndp_warp_job;
#define NDP_MAX_WARP_JOBS 32
int ndp_pyramid_fwd_batch(const ndp_layer_desc *desc, int m, int k0, int p_stride,
                          const ndp_warp_job *jobs, int n_jobs, void *stream);
/* The same warp with the engine's split arithmetic (ndp_engine.gemm_mode & 1): 128-wide contractions and layer 0 as two-way fp16
 * splits in the one-accumulator form (2^6 x = hi + lo, three partial products into one fp32 accumulator) on the fp16 MFMA; 256 points
 * per workgroup carried through all m levels in LDS.  fp32-level accuracy (within 1e-5 of ndp_pyramid_fwd_batch on warped
 * coordinates), not bitwise the fma chain; the 2^6 pre-scale means an activation or weight beyond about 1023 (65504 / 64)
 * saturates (layer 0's pre-activation at 65504).                                                                                  */
int ndp_pyramid_fwd_batch_split(const ndp_layer_desc *desc, int m, int k0, int p_stride,
                                const ndp_warp_job *jobs, int n_jobs, void *stream);
/* the same with `tiles` (1..8) 64-point tiles per workgroup instead of 4: fewer weight prologues per cloud, longer workgroups (the
   batched engine's throughput shape; identical results) */
int ndp_pyramid_fwd_batch_split_tiles(const ndp_layer_desc *desc, int m, int k0, int p_stride,
                                      const ndp_warp_job *jobs, int n_jobs, int tiles, void *stream);

/* The warp of levels min_level..max_level together with its per-point Jacobian, in one launch (csrc/ndp_jacobian.inc: a workgroup
 * carries a 64-point tile and three tangent rows per point through the levels; fp32 MFMA, no fp16 split).
 *   x [n][3] -> x_out [n][3]: bit for bit what ndp_pyramid_fwd gives for the same levels and input;
 *   J [n][9] row-major, J[3a+b] = d x_out_a / d x_b (first order; ReLU kinks take the derivative 0 of the level backward);
 *   normals_in / normals_out (both or neither; may be NULL) [n][3]: n' = cof(J) n / |cof(J) n|, which is J^-T n up to the factor
 *   det J -- no division by det J, so a fold does not blow up; where det J < 0 the SIGN of n' follows the cofactor matrix, i.e. it is
 *   opposite to J^-T n (a reflected patch keeps the orientation its cofactor matrix gives it).  A zero cof(J) n gives NaN.
 *   A cof(J) n whose fp32 squared length is within 2^-21 of 1 counts as unit and is written as it is (unit normals pass an identity
 *   warp bit for bit); |n'| is 1 to 3e-7 either way.
 * Refused before any launch (NDP_E_INVALID, NDP_E_UNSUPPORTED for the shape): n <= 0, levels outside 0 <= min_level <= max_level < m
 * <= 16, p_stride below the parameter count or not a multiple of 4, params_all not 16-byte aligned, NULL or misaligned (4 bytes)
 * x / x_out / J / normals, one of the normals pointers without the other.  Every point is written by one thread: reproducible,
 * independent of n.                                                                                                             */
int ndp_pyramid_jac(const ndp_layer_desc *desc, int m, int k0, const float *params_all, int p_stride, int min_level, int max_level,
                    const float *x, int n, float *x_out, float *J /*[n][9] row-major, J[3a+b] = dx'_a/dx_b*/,
                    const float *normals_in /*may be NULL*/, float *normals_out /*may be NULL*/, void *stream);

/* The inverse warp: Newton on W(x) = y with W the warp of levels min_level..max_level, every iteration of a 64-point tile inside ONE
 * launch (tiles are independent: no grid-wide synchronisation, no host round trip).
 *   y [n][3] targets; x [n][3] in: first guess (e.g. a copy of y), out: solution.
 *   Pass it = 0, 1, ..: evaluate W(x) and J; a point with max |W(x) - y| <= tol is frozen; otherwise, while it < iters, it steps
 *   x <- x - J^-1 (W(x) - y) (closed-form 3 x 3 solve through the cofactor matrix); at most `iters` steps, iters + 1 evaluations.
 *   residual [n]: max |W(x) - y| of the x written (the W of ndp_pyramid_fwd: a caller who recomputes it gets the same float);
 *   status [n] int: the number of steps taken when converged (0: the first guess already met tol and x is unchanged), -1 not
 *   converged within iters, -2 stopped on non-finite values or |det J| < 1e-12 (x is the last point evaluated).
 * No line search or trust region: where the field folds (det J <= 0 nearby) Newton may diverge, and the status says so.
 * Refusals as ndp_pyramid_jac, plus iters < 1 and tol not positive and finite.                                                   */
int ndp_pyramid_inverse(const ndp_layer_desc *desc, int m, int k0, const float *params_all, int p_stride, int min_level, int max_level,
                        const float *y, int n, float *x /*in: first guess, out: solution*/, int iters, float tol,
                        float *residual /*[n]*/, int *status /*[n] int*/, void *stream);

/* Per-cloud means (registration.py:150-153: src_pcd.mean(dim=0), tgt_pcd.mean(dim=0)); means[0..2] = source,
 * means[4..6] = target (means[3], means[7] = 0).  Accumulated in double in a fixed order, rounded once.   */
int ndp_pair_means(const float *src, int n_src, const float *tgt, int n_tgt, float *means, void *stream);

/* ---- Neural scene-flow prior (NSFP) baseline, SURVEY section 8 f3 ----------------------------------------------
 * x_out = x + MLP(x) with the 9-layer ReLU MLP of nets.py:256-292 (parameter layout: ndp_types.h), one launch per
 * layer, the 128x128 layers on the fp32 MFMA with the weight slice stationary in registers.
 * act: [8][cap][128] post-ReLU activations h1..h8 (cap = n rounded up to 64) saved for ndp_nsfp_bwd, or NULL for
 * inference, in which case tmp [2][cap][128] is the ping-pong scratch.  (registration.py:506-507, :534-536)          */
int ndp_nsfp_fwd(const float *params, const float *x, int n, float *x_out, float *act, float *tmp, void *stream);

/* Gradient of a scalar loss wrt all parameters given g = dL/dx_out [n][3] (autograd of registration.py:506-529).
 * act is consumed (h8 is overwritten by the running dz).  dO_work [cap][16]; grads_part [n_part][p_stride]
 * partials, one per workgroup, to be folded by ndp_grad_reduce (deterministic order, no atomics).                 */
int ndp_nsfp_bwd(const float *params, const float *x, int n, float *act, const float *g,
                 float *dO_work, float *grads_part, int n_part, int p_stride, void *stream);

/* ---- Nerfies baseline, SURVEY section 8 f3 (second half) ------------------------------------------------------------
 * Nerfies_Deformation.forward (nets.py:187-253): windowed 39-wide posenc -> 39->128 -> six 128x128 ReLU layers -> w / v
 * heads -> SE(3) exponential warp, plus the per-point Jacobian d warp / d x (carried forward as three tangent rows per
 * point: every buffer holds four planes [primal | d/dx0 | d/dx1 | d/dx2] of cap = n rounded up to 64 rows) and
 * reg = mean_p log(max(sigma_max(J_p), 1e-6))^2 (loss.py:373-379, per point in double).  Parameter layout:
 * [W_in 128x39 | b_in 128 | (W_l 128x128 | b_l 128) l=1..6 | W_h 6x128 (w rows, v rows) | b_h 6], P = 104 966.
 *   window6: HOST array of the six annealing weights of the iteration (nets.py:223-225)
 *   act: [save ? 7 : 2][4 cap][128] activation planes; pe: [cap][40]; heads: [4 cap][8]; work: [cap] doubles.           */
int ndp_nerfies_fwd(const float *params, const float *x, int n, const float *window6, float *x_out, float *J,
                    float *reg, float *act, int save, float *pe, float *heads, double *work, void *stream);
/* Gradient of a scalar loss wrt all parameters given g = dL/d(x_out) [n][3]; the regulariser carries none upstream (its
 * Jacobian is built with create_graph=False).  act (save = 1) is consumed.  dO_work [cap][16]; grads_part
 * [n_part][p_stride] partials for ndp_grad_reduce.                                                                     */
int ndp_nerfies_bwd(const float *params, const float *x, int n, float *act, const float *pe, const float *heads,
                    const float *g, float *dO_work, float *grads_part, int n_part, int p_stride, void *stream);

/* ---- Embedded-deformation N-ICP baseline, SURVEY section 8 f4 --------------------------------------------------------
 * Node graph: n_nodes positions `nodes` [n][3], axis-angle rotations `phi` [n][3], translations `t` [n][3]; every point has
 * six anchors (`anchors` [S][6] int32, -1 = the LAST node with weight 0, as upstream's negative indexing) with skinning
 * `weights` [S][6]; graph edges `edges` [n][K] int32 (-1 padded the same way) with `edge_w` [n][K].
 * ndp_ed_warp: R_work [n][9] <- axis_angle_to_matrix(phi) ; y = ED_warp(x) (geometry.py:37-49).  phi == NULL: R_work is used as it
 *              is (upstream's final warp runs with the R of the last loop iteration, registration.py:376, 449-453).
 * ndp_ed_arap: out[0] = arap_cost (loss.py:261-285) for the R of the last ndp_ed_warp.
 * ndp_ed_grad: grads [phi (3n) | t (3n)] = d/d(phi, t) of <gy, ED_warp(x)> + w_arap * arap  (gy = dL/dy [S][3], e.g. the
 * Chamfer gradient times w_cd): one workgroup per node, fixed summation order.                                          */
int ndp_ed_warp(const float *x, int S, const int *anchors, const float *weights, const float *nodes, int n_nodes,
                const float *phi, const float *t, float *R_work, float *y, void *stream);
int ndp_ed_arap(const float *nodes, int n_nodes, const float *R, const float *t, const int *edges, const float *edge_w,
                int K, float *out, void *stream);
int ndp_ed_grad(const float *x, int S, const int *anchors, const float *weights, const float *gy, const float *nodes,
                int n_nodes, const float *R, const float *t, const float *phi, const int *edges, const float *edge_w,
                int K, float w_arap, float *grads, void *stream);

/* Exact brute-force 1-NN in both directions (pytorch3d knn_points K=1 as called at loss.py:177-178):
 * d2x[i] = min_j |x_i - y_j|^2 (fma chain over x,y,z), idx_x[i] = lowest argmin; same for y->x.  */
int ndp_chamfer_nn_fwd(const float *x, int S, const float *y, int T,
                       float *d2x, int *idx_x, float *d2y, int *idx_y, void *stream);

/* The same result from ONE pass over the S x T squared distances (what the engine runs every tick): each distance is
 * evaluated once and serves both directions -- row minima thread-private, column minima by a cross-lane butterfly per
 * wave and an LDS table per workgroup, exact lowest indices by a re-scan of the winning 128-source block in LDS.
 * Bit-identical to ndp_chamfer_nn_fwd.  ws_row: scratch of ndp_engine_nn_workspace(S rounded up to 64, T rounded up
 * to 64) floats.                                                                                                   */
int ndp_chamfer_nn_onepass(const float *x, int S, const float *y, int T, float *d2x, int *idx_x, float *d2y,
                           int *idx_y, float *ws_row, void *stream);

/* The one-pass result with the S x T distances on the bf16 MATRIX pipe (the engine's nn_mode 2): |x - y|^2 = |x|^2 + |y|^2 - 2 x.y as
 * one contraction per 32 x 32 tile, every term a three-way bf16 split (two v_mfma_f32_32x32x16_bf16 per 1024 distances); that value
 * only SELECTS candidates -- every candidate within the rounding bound is re-evaluated with the exact fma chain, so d2 and the lowest
 * index are bit-identical to ndp_chamfer_nn_fwd.  2048 sources are resident in LDS at a time; more are walked in passes (highest
 * indices first, so the exact comparisons still end on the lowest index): no size limit since round 3
 * (ndp_engine_nn_matrix_fits(n_cap) is kept and returns 1: it cannot return anything else while the sources are walked in passes --
 * at most 2048 of them are resident, so the LDS carve has a worst case that is checked when the library is compiled).
 * ws_row as for ndp_chamfer_nn_onepass.                                                                                        */
int ndp_chamfer_nn_matrix(const float *x, int S, const float *y, int T, float *d2x, int *idx_x, float *d2y,
                          int *idx_y, float *ws_row, void *stream);
int ndp_engine_nn_matrix_fits(int n_cap);
/* 1 when the column table of the one-pass VECTOR kernel (engine nn_mode 0 / ndp_chamfer_nn_onepass) fits LDS for n_cap sources;
 * beyond that an engine must use nn_mode 1 (latency shape: no table, no size limit).                                                 */
int ndp_engine_nn_onepass_fits(int n_cap);

/* The same result from an exact grid ball search (what an engine with nn_cells runs every tick): the references of each direction are
 * sorted into a 64 x 8 x 8 grid (the wide search: 16^3) over the TARGETS' bounding box; a query evaluates, with the brute force's own fma chain, only the references in
 * the cells that the ball around it touches -- radius = its exact distance to a seed reference, widened by an explicit rounding margin
 * (csrc/ndp_nn_cells.inc) -- and keeps the smallest distance with the lowest index.  Bit-identical to ndp_chamfer_nn_fwd for ANY seeds.
 *   prev_idx_x [S] / prev_idx_y [T] (either may be NULL): seed indices, e.g. the previous call's idx_x / idx_y; an entry that is
 *   negative or not below the reference count is ignored (the seed then comes from the nearest non-empty cells).  They may alias
 *   idx_x / idx_y.   workspace: ndp_chamfer_nn_cells_workspace(T) floats, 16-byte aligned.
 * S, T <= 2048 (ndp_engine_nn_cells_fits); beyond that NDP_E_UNSUPPORTED.                                                           */
int ndp_chamfer_nn_cells(const float *x, int S, const float *y, int T, const int *prev_idx_x, const int *prev_idx_y,
                         float *d2x, int *idx_x, float *d2y, int *idx_y, float *workspace, void *stream);
int ndp_chamfer_nn_cells_workspace(int T, long long *floats);
/* 1 when an engine of these capacities can search by cells (ndp_engine.nn_cells): both <= 2048. */
int ndp_engine_nn_cells_fits(int n_cap, int t_cap);

/* The grid ball search for clouds of up to 8192 points (what an engine with nn_cells_wide runs every tick; csrc/ndp_nn_cells_wide.inc): the
 * same algorithm, geometry and result -- bit-identical to ndp_chamfer_nn_fwd for ANY seeds -- with both grids sorted in global memory (the
 * sources' by a launch of its own) and the queries of a direction split over workgroups of 2048.  Arguments as for ndp_chamfer_nn_cells;
 * workspace: ndp_chamfer_nn_cells_wide_workspace(S, T) floats, 16-byte aligned.
 * 1 <= S, T <= 8192 (ndp_engine_nn_cells_wide_fits); beyond that NDP_E_UNSUPPORTED.                                                    */
int ndp_chamfer_nn_cells_wide(const float *x, int S, const float *y, int T, const int *prev_idx_x, const int *prev_idx_y,
                              float *d2x, int *idx_x, float *d2y, int *idx_y, float *workspace, void *stream);
int ndp_chamfer_nn_cells_wide_workspace(int S, int T, long long *floats);
/* 1 when an engine of these capacities can run the wide cell search (ndp_engine.nn_cells_wide): both in 1..8192. */
int ndp_engine_nn_cells_wide_fits(int n_cap, int t_cap);

/* Truncated L1 Chamfer value and gradient from the NN result (loss.py:185-258 and its autograd):
 * loss[0] = sum_i sqrt(d2x_i)[d2x_i<trunc]/S + sum_j sqrt(d2y_j)[d2y_j<trunc]/T   (point_sum != 0: without the /S, /T --
 * point_reduction="sum", loss.py:233-235) ;
 * gx [S][3] = dloss/dx (contributions of y_j -> x_i added in ascending j).                      */
int ndp_chamfer_l1_bwd(const float *x, int S, const float *y, int T, float trunc,
                       const float *d2x, const int *idx_x, const float *d2y, const int *idx_y,
                       float *loss, float *gx, int point_sum, void *stream);

/* compute_flow_metrics / scene_flow_metrics (loss.py:382-403, 431-471) on the device: flow, flow_gt [n][3]; overlap [n]
 * bytes (0 / 1) or NULL.  out15 (device, 3 x 5 doubles), per subset {all, overlap, not overlap}:
 * {sum of end-point errors, #AccS hits, #AccR hits, #outliers, #points}; the caller divides (an empty subset gives NaN
 * like upstream's mean over nothing).                                                                                 */
int ndp_flow_metrics(const float *flow, const float *flow_gt, const unsigned char *overlap, int n, double *out15, void *stream);

/* Sinkhorn divergence baseline (registration.py:543-572 calls geomloss.SamplesLoss("sinkhorn", p=2, blur, reach); csrc/ndp_sinkhorn.inc).
 * The arithmetic is restated from the library's published algorithm (tensorized backend, debias, uniform weights, cost |u - v|^2 / 2)
 * in DESIGN.md "Sinkhorn baseline"; parity with the library itself is unverified.
 *
 * ndp_sinkhorn_schedule (host only): eps_list = [diameter^2] + [exp(e) for e in arange(2 ln diameter, 2 ln blur, 2 ln scaling)] +
 *   [blur^2] with numpy's arange (count ceil((stop - start) / step), none when diameter <= blur), in double.  Returns the number of
 *   entries and writes the first min(count, cap) of them to eps_out (host memory; may be NULL when cap == 0).
 * ndp_sinkhorn_workspace: *nfloats = 4 ceil(max(n, m) / 16) + 4 (n + m): one double per 16-row workgroup and side of the final
 *   kernel (the loss partials), then the potentials [f_ba n | f_aa n | g_ab m | g_bb m] twice (every step reads one copy and writes
 *   the other).  The workspace must be 8-byte aligned.
 * ndp_sinkhorn_divergence: x [n][3], y [m][3]; reach <= 0: balanced; diameter: norm of the extent of the joint bounding box, read
 *   by the caller.  loss_out: one device float; grad_x [n][3] (dloss/dx, the second cloud and the dual potentials held fixed) or
 *   NULL; potentials [2n + 2m] = (F_ba [n], F_aa [n], G_ab [m], G_bb [m]) or NULL.  Any n, m >= 1: the columns are streamed, the
 *   n x m matrix is never stored.  No atomics: the same inputs give the same bits.  1 + entries + 2 launches on `stream`.
 *   NDP_E_INVALID: n < 1, m < 1, blur <= 0, scaling outside (0, 1), diameter not positive and finite, reach not finite, a NULL
 *   x / y / ws / loss_out; NDP_E_UNSUPPORTED: a schedule of more than 256 entries.                                                */
int ndp_sinkhorn_schedule(double diameter, double blur, double scaling, double *eps_out, int cap);
int ndp_sinkhorn_workspace(int n, int m, long long *nfloats);
int ndp_sinkhorn_divergence(const float *x, int n, const float *y, int m, float blur, float reach, float scaling, double diameter,
                            float *ws, float *loss_out, float *grad_x, float *potentials, void *stream);

/* Surface normals (csrc/ndp_normals.inc; DESIGN.md "Surface normals").  Device pointers to contiguous fp32 / int32, nothing is
 * allocated, no atomics: the same inputs give the same bits.  One launch each on `stream`.
 *
 * ndp_knn: the K nearest references of every query, exact, by brute force (pytorch3d knn_points with K > 1, one cloud pair).
 *   q [nq][3], r [nr][3] -> d2 [nq][K] squared distances, idx [nq][K] reference indices, every row ascending in (d2, index): equal
 *   distances are listed by lower index.  A distance is ndp_chamfer_nn_fwd's chain (d = q - r per axis, fmaf(dz, dz, fmaf(dy, dy,
 *   dx * dx))), so column 0 at K = 1 is bit for bit its d2x / idx_x.  1 <= K <= 32, K <= nr, 1 <= nq, nr <= 16777216.
 *   NDP_E_INVALID: K outside 1..32 or above nr, nq or nr < 1, a NULL pointer; NDP_E_UNSUPPORTED: more than 16777216 points.
 * ndp_normals_from_knn: PCA normals.  p [n][3], idx [n][K] neighbour lists into p (K >= 3) -> normals [n][3], curvature [n] or NULL.
 *   Per point, over its K listed neighbours: mean, covariance C = (1/K) sum (p_k - mean)(p_k - mean)^T from differences, in double;
 *   normal = unit eigenvector of the smallest eigenvalue l0 (cyclic Jacobi in double, rounded to fp32 once); curvature =
 *   l0 / (l0 + l1 + l2).  Sign: with viewpoint (3 device floats) n . (viewpoint - p_i) >= 0; with NULL the component of largest
 *   magnitude is positive, the lowest axis winning ties.  A zero covariance gives the normal (0, 0, 0) and curvature 0; a row that
 *   lists an index outside [0, n) is not read and gives NaN.
 *   NDP_E_INVALID: K < 3, n < 1, a NULL p / idx / normals; NDP_E_UNSUPPORTED: more than 16777216 points.
 * ndp_point_to_plane: both directions' point-to-plane residuals and their gradient from ONE nearest-neighbour result (the four
 *   arrays of ndp_chamfer_nn_fwd).  Direction x: p = y[idx_x[i]], n = ny[idx_x[i]]; direction y: p = x[idx_y[j]], n = nx[idx_y[j]].
 *   mode 0: r = sqrt(sum_a ((x_a - p_a) n_a)^2), the reference's arithmetic as written (loss.py:87-88: the norm of the elementwise
 *   product, not a plane distance); mode 1: r = |sum_a (x_a - p_a) n_a|.
 *   out[1] = (1/S) sum_i r_i [d2x_i < trunc], out[2] the same over y with 1/T (trunc in squared units, +inf: the reference),
 *   out[0] = out[1] + out[2], out[3] = mean_i (1 - |cos(nx_i, ny[idx_x[i]])|) + mean_j (1 - |cos(ny_j, nx[idx_y[j]])|) (loss.py:200-210,
 *   cosine_similarity with eps 1e-6: a zero normal gives cos = 0; not truncated).  gx [S][3] or NULL: d out[0] / dx, indices and
 *   normals held constant, the terms direction y sends to x[idx_y[j]] added in ascending j.  mode 0 at r = 0 gives the reference's
 *   NaN (sqrt's backward at 0); mode 1 uses sign(0) = 0.  The gradient in y is the same entry with the clouds, normals and
 *   nearest-neighbour halves exchanged.
 *   NDP_E_INVALID: mode other than 0 / 1, S or T < 1, a NULL pointer other than gx, trunc NaN.                                          */
int ndp_knn(const float *q, int nq, const float *r, int nr, int K, float *d2, int *idx, void *stream);
int ndp_normals_from_knn(const float *p, int n, const int *idx, int K, const float *viewpoint, float *normals, float *curvature,
                         void *stream);
int ndp_point_to_plane(const float *x, int S, const float *y, int T, const float *nx, const float *ny, float trunc,
                       const float *d2x, const int *idx_x, const float *d2y, const int *idx_y, int mode, float *out, float *gx,
                       void *stream);

/* Rigid alignment from correspondences (csrc/ndp_rigid.inc; DESIGN.md "Rigid alignment").  Batched over B independent problems:
 * problem b owns the rows off[b] .. off[b + 1] of src [sum K][3] and tgt [sum K][3]; `off` is B + 1 device int32, `off_host` the same
 * B + 1 values in host memory, which the entries check.  Device pointers to contiguous fp32 / int32 / uint8; nothing is allocated,
 * no atomics, no random numbers: the same inputs give the same bits.  1 <= B <= 65535.
 *
 * ndp_rigid_fit: weighted Procrustes (Kabsch), the reference's arithmetic (correspondence/lepard/procrustes.py:30-43) in double:
 *   wn = w / (sum |w| + eps), mean_X = sum wn x, mean_Y = sum wn y, Sxy = sum (y - mean_Y) (wn (x - mean_X))^T from differences,
 *   the 3 x 3 SVD by one-sided Jacobi, R = U diag(1, 1, det U det V) V^T, t = mean_Y - R mean_X, condition = D.max / D.min (inf for
 *   a rank-deficient Sxy).  w [sum K] fp32 or NULL; mask [sum K] uint8 (non-zero = weight 1) or NULL, not both; both NULL: all ones.
 *   One workgroup per problem, one launch.  -> R [B][9] row-major, t [B][3], condition [B], status [B]: 0, or 1 when fewer than 3
 *   rows have a non-zero weight or the weights sum to zero, or 2 when Sxy has rank below 2 (the rows lie on a line or coincide):
 *   then R is the identity, t zero and the condition inf -- never NaN.  K = 0 is accepted (status 1).
 *   NDP_E_INVALID: B outside 1..65535, off_host not monotone or negative, w and mask together, eps negative or not finite, a NULL
 *   pointer other than w / mask.
 * ndp_rigid_score: H transforms per problem, T [B][H][12] = R row-major then t.  Per transform count [B][H] = number of rows with
 *   d2 < thr * thr (the product in fp32) and sse [B][H] (may be NULL) = the fp32 sum of those d2 in row order, with
 *     d_a = fmaf(R[a][0], sx, fmaf(R[a][1], sy, fmaf(R[a][2], sz, t[a]))) - y_a,   d2 = fmaf(dz, dz, fmaf(dy, dy, dx * dx)).
 *   One lane per transform, 256 per workgroup, the rows streamed through LDS in tiles of 2048: any K >= 1.  One launch.
 *   NDP_E_INVALID: B, off_host as above, a problem without rows, H < 1, thr not positive and finite, a NULL pointer other than sse.
 * ndp_ransac_rigid: `triples` [B][H][3] int32, indices into the problem's own rows, drawn by the caller.  A hypothesis is refused
 *   (flag bit 1) when two of its indices are equal or one lies outside [0, K); (2) when for one of its three edges
 *   min(|s_a - s_b|, |y_a - y_b|) < edge_ratio * max(...) in fp32 (edge_ratio 0: no such check); (4) when its triple is collinear:
 *   the three-point fit (ndp_rigid_fit's arithmetic with w = 1 and eps = 1e-4) has D[0] / D[1] above 1e6 -- the third singular
 *   value of a centred triple is eps-sized rounding (its Sxy has rank 2), so the ratio that says "degenerate" is that of the
 *   first two.  A refused hypothesis is not scored: count 0, transform identity.  The others are scored as ndp_rigid_score does.  The best hypothesis has
 *   the largest count, the lowest index among equals.  Refinement, refine_iters >= 0 times: the mask d2 < thr^2 under the current
 *   transform, then ndp_rigid_fit over that mask (eps = 1e-4); a mask of fewer than 3 rows or a fit with a status keeps the
 *   transform and ends the loop.  -> R [B][9], t [B][3], mask [sum K] under the final transform, count [B] its size, rmse [B] =
 *   sqrt(mean d2 over the mask), best [B] the hypothesis index, status [B]: 0, or 1 when no hypothesis has an inlier (R identity,
 *   t zero, mask zero, count 0, rmse 0, best -1).  h_count [B][H], h_flags [B][H], h_T [B][H][12]: the per-hypothesis results, each
 *   may be NULL.  ws: ndp_ransac_rigid_workspace(B, H) bytes, 4-byte aligned.  Three launches.  K >= 3 per problem, no upper limit.
 *   NDP_E_INVALID: B, off_host as above, a problem with K < 3, H < 1, thr not positive and finite, edge_ratio outside 0..1,
 *   refine_iters < 0, a NULL pointer other than h_count / h_flags / h_T, a misaligned workspace.                                */
int ndp_rigid_fit(const float *src, const float *tgt, const float *w, const unsigned char *mask, const int *off, const int *off_host,
                  int B, float eps, float *R, float *t, float *condition, int *status, void *stream);
int ndp_rigid_score(const float *T, const float *src, const float *tgt, const int *off, const int *off_host, int B, int H, float thr,
                    int *count, float *sse, void *stream);
int ndp_ransac_rigid_workspace(int B, int H, long long *nbytes);
int ndp_ransac_rigid(const float *src, const float *tgt, const int *off, const int *off_host, int B, const int *triples, int H, float thr,
                     float edge_ratio, int refine_iters, void *ws, float *R, float *t, unsigned char *mask, int *count, float *rmse,
                     int *best, int *status, int *h_count, int *h_flags, float *h_T, void *stream);

/* Descriptor matching (csrc/ndp_match.inc; DESIGN.md "Descriptor matching"; since ABI 212).  Batched over B independent problems:
 * problem b owns the rows offA[b] .. offA[b + 1] of A [sum S][C] and offB[b] .. offB[b + 1] of B [sum T][C], row-major fp32; the
 * `off*` are B + 1 device int32, the `off*_host` the same values in host memory, which the entries check.  The S x T matrix is
 * never stored.  Nothing is allocated, no atomics: the same inputs give the same bits.  1 <= B <= 65535, 1 <= C <= 1056, every
 * problem has S >= 1 and T >= 1.
 *
 * ndp_feat_rowstats: with a_ij = alpha * <A_i, B_j> + v_j (the dot product a k-ascending fp32 fma chain on the f32-input MFMA,
 *   the same bits with A and B exchanged), per row i of A:
 *     lse [sum S] = log(sum_j exp(a_ij) [+ exp(e[b])]),  max [sum S] = max_j a_ij,  arg [sum S] = the lowest j (local to the
 *   problem, int32) that attains it.  v [sum T] (per-column potential) and e [B] (one extra "dustbin" column per problem, which
 *   enters lse only) are device arrays or NULL; each of lse / max / arg may be NULL, not all three.  One launch.  Column
 *   statistics: call it with A and B (and their offsets) exchanged.
 *   NDP_E_INVALID: B, C, offsets as above (not monotone, negative, an empty side), a NULL or misaligned pointer, alpha not finite.
 * ndp_feat_match: per source row match_t [sum S] (the target index local to the problem, or -1) and conf [sum S] (the confidence
 *   of the row's best column, matched or not).  Row i matches j = arg_row[i] iff conf > thr and (mutual != 0: arg_col[j] == i).
 *   mode 0, dual_softmax (correspondence/lepard/matching.py:144-157): s = <fs_i, ft_j> / (C * temperature),
 *     conf_ij = softmax_i(s) softmax_j(s) = exp(2 s_ij - lse_row_i - lse_col_j); four row-statistics launches.
 *   mode 1, sinkhorn (matching.py:6-38, 159-170) on the unpadded problem: s = <fs_i, ft_j> / C augmented by a dustbin row and
 *     column of score bin_score, `iters` iterations from u = v = 0, conf = exp(s + u + v + log(S + T)); 2 iters + 1 row-statistics
 *     launches (2 at iters = 0).  `temperature` is not read.
 *   mode 2, mutual_nn (utils/benchmark_utils.py:335-359): the raw scores `temperature` * <fs_i, ft_j> (pass 1), conf = the score;
 *     thr may be -inf.
 *   ws: ndp_feat_match_workspace(B, sum S, sum T) bytes, 4-byte aligned.  All launches go to `stream` in order.
 *   NDP_E_INVALID: as ndp_feat_rowstats, a mode outside 0..2, temperature not positive and finite (modes 0, 2), bin_score not
 *   finite (mode 1), iters < 0, thr NaN.                                                                                        */
int ndp_feat_rowstats(const float *A, const float *B_rows, const int *offA, const int *offB, const int *offA_host, const int *offB_host,
                      int B, int C, float alpha, const float *v, const float *e, float *lse, float *max, int *arg, void *stream);
int ndp_feat_match_workspace(int B, long long nS, long long nT, long long *nbytes);
int ndp_feat_match(const float *fs, const float *ft, const int *offS, const int *offT, const int *offS_host, const int *offT_host,
                   int B, int C, int mode, float temperature, float bin_score, int iters, float thr, int mutual, void *ws,
                   int *match_t, float *conf, void *stream);

/* KPConv inputs (csrc/ndp_kpconv.inc; DESIGN.md "KPConv inputs"), ABI 213.  Stacked clouds: points [N][3] fp32 on the device and
 * B lengths, every one >= 1, their sum N, in HOST memory.  The grid of both operators is a sorted table of 64-bit cell keys
 * (cloud : 16 | iz : 16 | iy : 16 | ix : 16), sorted inside the library: memory is O(N) whatever the bounding box, a cloud never
 * sees another cloud's points, there are no floating-point atomics, and the same inputs give the same bits.  BOTH ENTRIES END IN
 * A SYNCHRONISE of `stream`: the size of the subsampled cloud is data, and so are the refusals below.
 *
 * ndp_voxel_subsample: barycentres of the occupied voxels of edge dl (batch_grid_subsampling, cpp_subsampling/grid_subsampling.cpp).
 *   Membership is the reference's in fp32: origin = floorf(min * (1 / dl)) * dl per cloud, i = floorf((p - origin) / dl) per axis.
 *   A barycentre is the sum of the voxel's points in ascending input index in double, divided by the count, rounded to fp32 once;
 *   feat [N][F] (F >= 0, NULL at F = 0) is averaged the same way.  Output order: per cloud ascending (iz, iy, ix); max_p > 0 keeps
 *   the first max_p voxels of each cloud.  out_pts [N][3] / out_feat [N][F] are sized for the worst case and filled for the first
 *   sum(out_lengths_host) rows; out_lengths_host [B] (HOST) receives the voxels kept per cloud; inverse [N] (may be NULL) the output
 *   row of every input point, -1 for a point of a voxel that max_p dropped.
 * ndp_radius_search: for every query the supports of its own cloud with d2 < radius * radius (strict; fp32; d2 is ndp_knn's chain
 *   of d = q - s), nearest first.  idx [nq][K] stacked-global support indices in (d2, index) order, padded with the shadow index
 *   ns = sum of the supports' lengths; d2 [nq][K] (may be NULL) the distances, padded with +inf; counts [nq] the number within the
 *   radius BEFORE the cut to K.  0 <= K <= 64; K = 0 fills counts only (idx may be NULL).  Queries may lie outside the supports'
 *   bounding box.
 * ws: at least ndp_*_workspace(...) bytes, 16-byte aligned; ws_bytes is checked.  The workspace queries need no device.
 *   NDP_E_INVALID: B outside 1..65535, a length < 1, dl or radius not positive and finite, K outside 0..64, a NULL pointer, a
 *   workspace too small or misaligned, a coordinate that is NaN or infinite.  NDP_E_UNSUPPORTED: more than 2^30 points, or a
 *   cloud that spans more than 65535 cells along an axis (voxels of edge dl; cells of edge 1.03125 * radius): it does not fit
 *   the key.                                                                                                                       */
int ndp_voxel_subsample_workspace(long long n, int B, long long *nbytes);
int ndp_voxel_subsample(const float *pts, const float *feat, int F, const int *lengths_host, int B, float dl, int max_p, void *ws,
                        long long ws_bytes, float *out_pts, float *out_feat, int *inverse, int *out_lengths_host, void *stream);
int ndp_radius_search_workspace(long long nq, long long ns, int B, long long *nbytes);
int ndp_radius_search(const float *q, const float *s, const int *q_lengths_host, const int *s_lengths_host, int B, float radius, int K,
                      void *ws, long long ws_bytes, int *idx, float *d2, int *counts, void *stream);

/* KPConv convolution (csrc/ndp_kpconv_conv.inc; DESIGN.md "KPConv convolution"), ABI 214: the forward of the reference's rigid
 * KPConv (lepard/blocks.py:229-374 with deformable = False) in one launch, plus a pre-pass over x when normalize = 1.
 * q [nq][3] queries, s [ns][3] supports, idx [nq][H] int32 stacked-global support rows as ndp_radius_search writes them,
 * x [ns][cin] features, W [K][cin][cout] weights, kp [K][3] kernel points, y [nq][cout]; all contiguous, on the device.
 *   valid(n,h) = 0 <= idx[n,h] < ns.  EVERY other value (the shadow ns, a negative, anything larger) is a shadow: nothing is read
 *                for it and it contributes nothing in any mode.  The reference would raise; here a bad table cannot fault.
 *   d2(n,h,k)  = |(s[idx[n,h]] - q[n]) - kp[k]|^2 in fp32
 *   w(n,h,k)   = 1 (influence 0, constant) | max(0, 1 - sqrt(d2) / extent) (1, linear) | exp(-d2 / (2 (0.3 extent)^2 + 1e-9)) (2, gaussian)
 *   aggregation 1 (closest): w is kept only for the k with the smallest d2(n,h,.), the lowest k among equals; 0 (sum): for all k
 *   wf[n,k,c]  = sum_h w(n,h,k) x[idx[n,h],c]        y[n,o] = sum_k sum_c wf[n,k,c] W[k,c,o]
 *   normalize 1: y[n,:] /= max(1, #{h valid : sum_c x[idx[n,h],c] > 0}), the reference's term (blocks.py:368-372), an IEEE fp32
 *                division; the flag of a support row is computed once per call in a fixed order.  normalize 0: the plain sum.
 * Both products run on the f32-input MFMA (exact fp32 products, one rounding per term, a fixed order); there are no atomics, the
 * same inputs give the same bits, and a query's result does not depend on the other queries of the call.  Nothing is
 * data-dependent: ndp_kpconv_forward launches on `stream` and DOES NOT synchronise.  The backward pass in x and W:
 * ndp_kpconv_backward below (ABI 219).
 * ws: at least ndp_kpconv_forward_workspace(...) bytes (the row flags), 16-byte aligned; ws_bytes is checked.  The query needs no device.
 *   NDP_E_UNSUPPORTED: outside 1 <= K <= 32, 1 <= H <= 64, 1 <= cin, cout <= 1024, 1 <= nq, ns <= 2^30 on the large side.
 *   NDP_E_INVALID: a dimension < 1, a NULL or misaligned pointer, extent not positive and finite, influence outside 0..2,
 *   aggregation or normalize outside 0..1, a workspace too small.                                                                 */
int ndp_kpconv_forward_workspace(long long nq, long long ns, int H, int K, int cin, int cout, long long *nbytes);
int ndp_kpconv_forward(const float *q, const float *s, const int *idx, const float *x, const float *W, const float *kp,
                       long long nq, long long ns, int H, int K, int cin, int cout, float extent, int influence, int aggregation,
                       int normalize, void *ws, long long ws_bytes, float *y, void *stream);
/* KPConv backward (csrc/ndp_kpconv_bwd.inc; DESIGN.md "KPConv backward"), ABI 219: the gradient of sum(y * dy) of ndp_kpconv_forward in
 * the features x and the weights W, for the same arguments and dy [nq][cout].
 *     g[n,o] = dy[n,o] / count[n] (normalize 1, the forward's division; else dy)     dW[k,c,o] = sum_n wf[n,k,c] g[n,o]
 *     dwf[n,k,c] = sum_o g[n,o] W[k,c,o]        dx[r,c] = sum over valid (n,h) with idx[n,h] == r of sum_k w(n,h,k) dwf[n,k,c]
 *   count and the `closest` choice are constants; q, s and kp get no gradient.  w is recomputed from the points with the forward's
 *   expressions; nothing of the forward is kept but its inputs.  dx [ns][cin] or dW [K][cin][cout] may be NULL: that gradient and its
 *   launches are skipped (both NULL is refused).
 *   fp32 on the f32-input MFMA, no atomics, one writer per output element per launch, every sum in one fixed order: the same bits run to
 *   run.  dx[r,c] is ONE chain from +0 over the incoming edges of r in ascending (n,h): the library transposes the table by a stable
 *   radix sort of the edge ids by support row (shadows -- every idx outside 0 .. ns-1 -- under a key no row reaches).  The per-edge
 *   gradients pass through global memory in slabs of `slab_queries` queries, at most 64 MiB; a slab continues the chain its predecessor
 *   left in dx, so the bits of dx do not depend on the slab size.  A support row without an incoming edge gets +0.  No [nq][K][cin]
 *   array exists in global memory.  dW: a workgroup owns 16 x 16 x 64 of (k, c, o) and walks the query tiles in ascending order; where
 *   that gives few workgroups the walk is cut into segments (a function of the dimensions only) whose partials one writer adds in
 *   ascending order.  The bits of dW do not depend on slab_queries or on whether dx is asked for, and the other way round.
 *   slab_queries: 0 (the library's choice: as many as 64 MiB hold) or a multiple of 16 whose slab fits 64 MiB.
 *   ws: ndp_kpconv_backward_workspace(...) bytes for the same slab_queries, 16-byte aligned: the slab buffer and O(nq H + ns) integers
 *   (flags, counts, the sort's keys, values and temporary storage, the row starts).  The query needs no device.  The edge count is
 *   known on the host: ndp_kpconv_backward launches on `stream` and DOES NOT synchronise.  Every refusal precedes the first launch.
 *   Refused as ndp_kpconv_forward, and NDP_E_INVALID: a NULL or misaligned dy, dx and dW both NULL, slab_queries negative, no multiple
 *   of 16 or too large for 64 MiB; NDP_E_UNSUPPORTED: nq H >= 2^31 (an edge id is an int).                                         */
int ndp_kpconv_backward_workspace(long long nq, long long ns, int H, int K, int cin, int cout, long long slab_queries, long long *nbytes);
int ndp_kpconv_backward(const float *q, const float *s, const int *idx, const float *x, const float *W, const float *kp, const float *dy,
                        long long nq, long long ns, int H, int K, int cin, int cout, float extent, int influence, int aggregation,
                        int normalize, long long slab_queries, void *ws, long long ws_bytes, float *dx, float *dW, void *stream);

/* Attention and the dense confidence matrix (csrc/ndp_attention.inc, the end of csrc/ndp_match.inc; DESIGN.md "Attention"), ABI 215:
 * what Lepard's repositioning transformer (correspondence/lepard/transformer.py, matching.py) needs between the KPFCN descriptors
 * and the match list.  Problems are stacked and unpadded as for ndp_feat_rowstats: problem b owns the rows off[b] .. off[b + 1];
 * the offsets are given twice, on the device and as a HOST copy which the entry checks before anything is launched.
 *
 * ndp_attention_forward: multi-head soft-max attention.  q [sum L][C], k, v [sum S][C] fp32, already projected; D = C / n_head;
 *   pe_q [sum L][C][2], pe_k [sum S][C][2]: (cos, sin) per channel of a rotary code, both or neither (NULL).
 *     o[i, h D + d] = sum_j softmax_j(scale <q'_i,h, k'_j,h>) v[j, h D + d]
 *     q' = q cos + rot(q) sin, rot(x)[2m] = -x[2m + 1], rot(x)[2m + 1] = x[2m] (VolumetricPositionEncoding.embed_rotary); v is not
 *     rotated.  The rotation is applied while an operand is staged: no rotated copy and no L x S x H score reaches global memory.
 *   One launch; scores and P V on the f32-input MFMA (exact fp32 products, one rounding per term), an online soft-max over key
 *   tiles in ascending order, every partial result folded in one fixed order, no atomics.  No bit of an output row depends on the
 *   other problems of the call, on the other query rows, or on where the row falls in its block.  Nothing is data-dependent: the
 *   entry DOES NOT synchronise.  The backward pass: ndp_attention_backward below (ABI 217).
 *   NDP_E_UNSUPPORTED: outside 1 <= C <= 1056, 1 <= n_head <= 16 with C % n_head == 0 and C / n_head <= 264, rows <= 2^30 a side.
 *   NDP_E_INVALID: B outside 1..65535, bad offsets (negative, not monotone, an empty side), a NULL or misaligned pointer, one of
 *   pe_q / pe_k without the other, a rotary code with an odd C / n_head, a scale that is not finite.
 * ndp_feat_conf: the dense dual-softmax confidence matrix conf [B][Smax][Tmax] (Smax, Tmax at least the largest problem's S, T):
 *     conf[b, i, j] = exp(a_ij - lse_row_i) exp(a_ij - lse_col_j),  a_ij = <fs_i, ft_j> / (C temperature)
 *   inside a problem's S x T and exactly 0 outside it (matching.py:144-157 on a padded batch).  Two ndp_feat_rowstats launches
 *   for the statistics, then one dense pass that recomputes a_ij with that kernel's operand order and chain.  Does not synchronise.
 *   ws: ndp_feat_conf_workspace(B, sum S, sum T) bytes, 4-byte aligned; the query needs no device.
 *   NDP_E_INVALID: as ndp_feat_rowstats, temperature not positive and finite, Smax / Tmax below the largest problem.
 *   Sinkhorn confidences are not served as a matrix.                                                                              */
int ndp_attention_forward(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const int *offQ,
                          const int *offK, const int *offQ_host, const int *offK_host, int B, int C, int n_head, float scale,
                          float *o, void *stream);
/* ndp_attention_compat_forward (ABI 216; DESIGN.md "Outlier rejection"): ndp_attention_forward with every score multiplied by the
 * spatial compatibility of the correspondences i and j before the scale and the soft-max -- what the nine layers of the reference's
 * Outlier_Rejection (correspondence/outlier_rejection/pipeline.py:52-58, geometry_attention.py:85-96) compute on M x M tensors:
 *     score[i, j, h] = scale (<q'_i,h, k'_j,h> c[i, j]),   c[i, j] = max(0, 1 - (|s_i - s_j| - |t_i - t_j|)^2 / sigma_spat^2)
 *   pos_q [sum L][6], pos_k [sum S][6] fp32: (s_xyz, t_xyz) of every row, always both.  c is taken in fp32 in the reference's order
 *   (two norms, their difference squared, a true division by (float)(sigma_spat^2), 1 minus, clamp at 0) with correctly rounded
 *   square roots and division, on the chip: no M x M array exists.  c = 0 scores 0 and takes part in the soft-max; a key beyond S
 *   scores -inf.  sigma_spat = +inf means c == 1: the bits of ndp_attention_forward.  Every promise of ndp_attention_forward holds.
 *   Non-finite positions are the caller's error and are not checked on the device.
 *   Refused as ndp_attention_forward, and NDP_E_INVALID: pos_q or pos_k NULL or misaligned, sigma_spat NaN or <= 0 (or so small
 *   that its square underflows fp32).                                                                                              */
int ndp_attention_compat_forward(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k,
                                 const float *pos_q, const float *pos_k, const int *offQ, const int *offK, const int *offQ_host,
                                 const int *offK_host, int B, int C, int n_head, float scale, double sigma_spat, float *o, void *stream);
/* Attention with statistics and the attention backward (ABI 217; DESIGN.md "Attention backward"): what training on the two entries
 * above needs.  pos_q / pos_k are both given (the compatibility-modulated form, sigma_spat as ndp_attention_compat_forward's) or
 * both NULL (the plain form; sigma_spat is not read).  sigma_spat = +inf is the plain form's bits.
 * ndp_attention_forward_lse: o as ndp_attention_forward / ndp_attention_compat_forward write it, bit for bit, and
 *   lse [sum L][n_head], lse[i, h] = log sum_j exp(score[i, j, h]), the log-sum-exp of the row's scaled (and modulated) scores.
 * ndp_attention_backward: given do [sum L][C] and the o, lse of ndp_attention_forward_lse for the same arguments,
 *     dq [sum L][C], dk, dv [sum S][C]: the gradient of sum(o * do) in the UNROTATED q, k and v.
 *   pe_* and pos_* are data: they get no gradient and c is not differentiated.  Two launches that recompute the scores tile by tile
 *   (no L x S array in global memory): the dq sweep (16 query rows a workgroup, key tiles in ascending order; it also writes
 *   delta[i, h] = sum_d o do) and the dk / dv sweep (16 key rows a workgroup, query tiles in ascending order).  A walked tile has 64
 *   rows for C / n_head <= 144 and 48 above, so that the LDS of a workgroup fits 160 KiB at C / n_head = 264.  fp32 on the f32-input
 *   MFMA, no atomics, one writer per output element, every sum in one fixed order: the same bits run to run.  A key with c = 0 takes
 *   part in the soft-max, so it feeds dv and delta, and feeds nothing to dq or dk.  The rotation is undone while a block is written:
 *   no rotated copy reaches global memory.  No bit of a row of dq depends on the other query rows, and none of any output on the
 *   other problems of the call.  delta [sum L][n_head] floats is the call's workspace.  Neither entry synchronises.
 *   Refused as ndp_attention_forward, and NDP_E_INVALID: a NULL or misaligned o, lse, do, delta, dq, dk or dv, one of pos_q / pos_k
 *   without the other, and with positions a sigma_spat that ndp_attention_compat_forward refuses.                                  */
int ndp_attention_forward_lse(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const float *pos_q,
                              const float *pos_k, const int *offQ, const int *offK, const int *offQ_host, const int *offK_host, int B,
                              int C, int n_head, float scale, double sigma_spat, float *o, float *lse, void *stream);
int ndp_attention_backward(const float *q, const float *k, const float *v, const float *pe_q, const float *pe_k, const float *pos_q,
                           const float *pos_k, const float *o, const float *lse, const float *dout, const int *offQ, const int *offK,
                           const int *offQ_host, const int *offK_host, int B, int C, int n_head, float scale, double sigma_spat,
                           float *delta, float *dq, float *dk, float *dv, void *stream);
int ndp_feat_conf_workspace(int B, long long nS, long long nT, long long *nbytes);
int ndp_feat_conf(const float *fs, const float *ft, const int *offS, const int *offT, const int *offS_host, const int *offT_host,
                  int B, int C, float temperature, void *ws, float *conf, int Smax, int Tmax, void *stream);

/* Landmark loss mean_k |x_k - t_k|^2 and gradient (registration.py:201-203). */
int ndp_landmark_mse_fwd_bwd(const float *x, const float *t, int K, float *loss, float *gx, void *stream);

/* torch.optim.Adam single-tensor step t (1-based) on P parameters (registration.py:176,237).
 * neg_step = -(lr / (1 - b1^t)), bc2_sqrt = sqrt(1 - b2^t) are computed by the caller in double
 * and passed as float, exactly as torch casts its Python scalars.                               */
int ndp_adam_step(float *params, const float *grads, float *m, float *v, int P,
                  float w1, float b2, float w2, float neg_step, float bc2_sqrt, float eps, void *stream);

/* ------------------------------------------------------------------ batched engine
 * B independent pairs advance together, one "tick" = one iteration of the inner loop of
 * optimize_deformation_pyramid (registration.py:184-238) for every unfinished pair, each pair at
 * its own level / iteration, early stop decided on the device (registration.py:226-232).        */

typedef struct ndp_pair_geom {
    int K;            /* landmark count (0 without landmarks)                        */
    int S;            /* Chamfer source samples (0 in landmark-only mode)            */
    int T;            /* Chamfer target samples                                      */
    int pad;
} ndp_pair_geom;

typedef struct ndp_pair_state {
    int level;                       /* current level; == m when the pair is finished           */
    int iter;                        /* loss evaluations done at this level                     */
    int break_counter;               /* registration.py:179                                     */
    int adam_t;                      /* Adam steps taken at this level                          */
    int cur;                         /* which half of pts[] is the level input                  */
    int decision;                    /* what this tick's update kernel must do (NDP_DEC_*)      */
    int total_steps;                 /* Adam steps over all levels                              */
    int total_evals;                 /* loss evaluations over all levels                        */
    float loss;                      /* last evaluated loss                                     */
    int step_level;                  /* level this tick's Adam step applies to                  */
    int step_t;                      /* Adam step number (1-based) of this tick's step          */
    int pad;
    double loss_prev;                /* registration.py:180                                     */
    int evals_per_level[NDP_MAX_LEVELS];
} ndp_pair_state;

enum { NDP_DEC_STEP = 0, NDP_DEC_ADVANCE = 1, NDP_DEC_STEP_ADVANCE = 2, NDP_DEC_IDLE = 3 };

typedef struct ndp_engine {
    ndp_layer_desc desc;             /* shared by all levels; nonrigidity = 1: levels > 0 gated  */
    int m, k0;
    int P, p_stride;                 /* params per level, padded stride (multiple of 4)         */
    int iters, max_break_count, early_stop;
    int B, G;                        /* pairs; blocks per pair in the level kernels             */
    int n_cap, t_cap;                /* per-pair capacities, multiples of NDP_TILE              */
    double break_threshold_ratio;
    float w_cd, trunc;
    float adam_w1, adam_b2, adam_w2, adam_eps;
    float w_reg, pad_f;              /* nonrigidity BCE weight (registration.py:216-220)         */
    ndp_pair_geom *geom;             /* [B]                                                     */
    ndp_pair_state *state;           /* [2][B] double-buffered by tick parity                   */
    float *pts;                      /* [B][2][n_cap][3]  landmarks first, then samples         */
    float *ldmk_t;                   /* [B][n_cap][3]                                           */
    float *tgt;                      /* [B][t_cap][3]                                           */
    float *params;                   /* [B][m][p_stride]                                        */
    float *gpart;                    /* [B][G][p_stride] gradient partials (G == 1 without gemm_mode bit 1024: the W1 / W2 blocks are not written) */
    float *adam_m, *adam_v;          /* [B][p_stride]                                           */
    float *act;                      /* [B][3][n_cap][128] fp32 rows of h0, h1, h2 ([B][depth][n_cap][width] for other shapes) -- except under the default gemm_mode 7 (fused
                                        split backward), where planes 1 and 2 hold h1 and (since ABI 202) h2 per 64-point tile as a
                                        PLANE IMAGE of the same size: two [64][128] fp16 planes hi = fp16(2^6 h) | lo = fp16(2^6 h - hi),
                                        rows of 256 bytes with their 16-byte granules XOR-swizzled (csrc/ndp_fwd_split.inc: bf_swz) --
                                        the backward's LDS layout, written by the forward and pulled in by LDS-DMA; the ReLU mask is
                                        hi's SIGN BIT: hi = -0 where the pre-activation is <= 0, hi >= +0 where it is positive.  Every activation a split forward stores -- image
                                        or fp32 row -- is the BOUNDED value: it saturates at 65504 / 64 = 1023.5 (the fp16 operand
                                        range of the 2^6-scaled splits); this network's activations are O(1)        */
    float *heads;                    /* [B][n_cap][NDP_HROW]                                    */
    float *d2x; int *idx_x;          /* [B][n_cap]                                              */
    float *d2y; int *idx_y;          /* [B][t_cap]                                              */
    const float *adam_tab;           /* [iters+1][2]: {neg_step, bc2_sqrt} for t = 1..iters     */
    float *dO;                       /* [B][n_cap][16] mlp_scale * dL/d(head outputs), this tick */
    float *nn_row;                   /* one-pass 1-NN row partials, B x ndp_engine_nn_workspace() floats (NULL if w_cd == 0) */
    int nn_mode, gemm_mode;          /* gemm_mode 0: level kernels on the fp32 MFMA, bitwise the oracle's fma chain.  Mask 1 forward,
                                        2 bwd1, 4 bwd2: their 128 x 128 contractions from two-way fp16 splits (x' = hi + lo of operands
                                        pre-scaled by a power of two, three products, fp32 accumulate; the two-launch backward of bit
                                        16: hi + 2^-11 lo) on the 16-bit MFMA -- fp32-level accuracy, not bitwise the chain
                                        (csrc/ndp_*_split.inc); 7 is what Registration uses by default.  With 1 | 2 the forward does
                                        not store h0 (act[b][0] is left untouched): the backward recomputes it from the saved
                                        encoding with the forward's own layer-0 MFMA; bit 8 makes the forward store it all the same
                                        (tests).  With 2 | 4 both backward layers run as ONE launch (k_eng_bwd_f,
                                        csrc/ndp_bwd_fused.inc: dz1 stays in LDS, one accumulator per product on operands pre-scaled
                                        by powers of two -- activations and weights beyond 1023 saturate there); bit 16: as the two
                                        launches k_eng_bwd2_8 + k_eng_bwd1_8 instead; bit 32 (tests): the fused launch also writes
                                        dz1 over the h2 plane of `act`, where the two-launch form leaves it.  1024: the whole Adam
                                        step in k_eng_update -- without it an engine with G == 1 steps the two 128 x 128 matrices
                                        behind the fused backward's tile loop (no gradient partial of them is written: gpart's two
                                        matrix blocks are then undefined) and the rest in k_eng_update_rest: bitwise the same state.
                                        No other bit is accepted (ABI 204: bits 64, 128, 256 and 512 selected measured variants,
                                        DESIGN.md section 0, and are refused).
                                        nn_mode 0: one-pass kernel, distances on the vector pipe; 2: the same on the bf16 matrix pipe
                                        with exact re-evaluation (bit-identical, any n_cap: k_eng_nn_mx8); 1: latency
                                        shape -- two passes in 64-query workgroups, S/64 + T/64 of them per pair -- for a handful of
                                        resident pairs   */
    unsigned int *gmax;              /* [B] bit pattern of max |dO| of the pair this tick (zeroed by the forward stage, raised by
                                        the loss stage): the power-of-two scale that puts the split backward's gradient operands
                                        into fp16's range.  Required when gemm_mode & 6, else may be NULL.                       */
    int nn_cells, pad_i;             /* ABI 207.  nn_cells != 0: the nearest-neighbour stage is the exact grid ball search
                                        (csrc/ndp_nn_cells.inc: k_eng_nn_cells, bit-identical results, needs
                                        ndp_engine_nn_cells_fits(n_cap, t_cap)) in place of the dense kernel nn_mode names; nn_mode
                                        keeps its value and meaning.  ndp_engine_load then also builds the grid of a slot's targets. */
    float *nnc_geom;                 /* [B][8] grid geometry per pair: origin[3], cells per unit length[3], 2 pad (NULL without nn_cells) */
    int *nnc_start;                  /* [B][NDP_NNC_START] cell_start of the targets' grid, x fastest (NULL without nn_cells)            */
    float *nnc_rec;                  /* [B][t_cap][4] the targets sorted by cell: {index bits, x, y, z}, 16-byte aligned (NULL without) */
    int nn_cells_wide, pad_w;        /* ABI 208.  nn_cells_wide != 0: the nearest-neighbour stage is the grid ball search for up to 8192
                                        points per cloud (csrc/ndp_nn_cells_wide.inc: k_eng_nnw_sort + k_eng_nn_cells_wide, bit-identical
                                        results, needs ndp_engine_nn_cells_wide_fits(n_cap, t_cap)) in place of the dense kernel nn_mode
                                        names.  Not together with nn_cells.  The grids live in the three buffers above in a layout of their
                                        own: nnc_geom [B][8] as there; nnc_start [B][2][NDP_NNC_START]: the targets' cell_start table, then
                                        the warped sources' (rewritten every tick); nnc_rec [B][t_cap + n_cap][4]: the targets' records,
                                        then the warped sources'.  ndp_engine_load builds the grid of a slot's targets.                    */
} ndp_engine;
#define NDP_NNC_START 4104           /* ints per cell_start table: 4096 + 1 entries, padded to a multiple of 4 */

/* Floats PER PAIR of the row-partial buffer of the one-pass nearest-neighbour kernel ({d2, idx} per source and
 * 128-target chunk).                                                                                             */
int ndp_engine_nn_workspace(int n_cap, int t_cap, long long *row_floats);

/* Launch n_ticks ticks starting at tick index tick0 (parity selects the state buffer read).
 * The caller initialises state[tick0 & 1] (level 0, iter 0, break_counter 0, loss_prev 1e6, cur 0).
 * Asynchronous on `stream`; read state[(tick0 + n_ticks) & 1] after synchronising.              */
int ndp_engine_run(const ndp_engine *e, int tick0, int n_ticks, void *stream);

/* Slot (re)fill in one launch for several pairs (registration.py:150-164: centring, sampling by the
 * permutation prefix, landmark centring; :133-140 the freshly initialised pyramid; :176 fresh Adam state):
 *   pts[slot][0][i]   = i < K ? ldmk_s[i] - mean_s : src[perm_s[i-K]] - mean_s      (i < K+S, rest zero)
 *   ldmk_t[slot][k]   = ldmk_t[k] - mean_t ;  tgt[slot][j] = tgt[perm_t[j]] - mean_t  (j < T)
 *   params[slot]      = params ; adam_m = adam_v = 0 ; geom = (K,S,T) ; state[tick & 1][slot] = fresh
 * perm_* NULL = identity, means NULL = no centring (n_src > 0: the means are computed by this call, see the struct).  A job with
 * params == NULL parks the slot (level = m).
 * `jobs` is a HOST array (copied into the kernel arguments); at most NDP_MAX_LOAD_JOBS per call.       */
typedef struct ndp_load_job {
    const float *src, *tgt;          /* raw clouds [n][3] (device) */
    const int *perm_s, *perm_t;      /* first S / T entries of the sampling permutations (device int32) or NULL */
    const float *ldmk_s, *ldmk_t;    /* [K][3] or NULL */
    const float *params;             /* [m][p_stride] initial parameters (device) or NULL = park */
    float *means;                    /* [8] as ndp_pair_means leaves them, or NULL.  With n_src > 0 they are an OUTPUT first: the call
                                        computes the means of src [n_src] / tgt [n_tgt] into `means` -- ONE launch for all such jobs
                                        of the call, the arithmetic of ndp_pair_means (same bits) -- and then centres with them */
    int slot, K, S, T;
    int n_src, n_tgt;                /* points of the raw clouds when the means are to be computed here, else 0 */
} ndp_load_job;
#define NDP_MAX_LOAD_JOBS 16
int ndp_engine_load(const ndp_engine *e, int tick, const ndp_load_job *jobs, int n_jobs, void *stream);

/* Same launches with HIP events around every kernel, recorded on `stream`; ms_out[NDP_TICK_KERNELS] (HOST memory)
 * receives the summed durations of the forward, NN, loss/gradient, backward-2 (+ heads), backward-1 and update
 * kernels over the n_ticks ticks.  Synchronises `stream`.  Measurement aid for bench.py (roofline), not a product path. */
#define NDP_TICK_KERNELS 6
int ndp_engine_run_timed(const ndp_engine *e, int tick0, int n_ticks, void *stream, float *ms_out);

/* ONE tick, restricted to the launches of stages [stage_lo, stage_hi]: 0 forward, 1 nearest neighbours, 2 loss / decision /
 * dL/dx', 3 bwd2, 4 bwd1, 5 update.  Test and measurement aid: the buffers a kernel leaves behind (act, heads, dO, gpart) can be
 * read between stages; the stages 0..5 of a tick run in order, in any grouping, equal ndp_engine_run(e, tick, 1).               */
int ndp_engine_run_stages(const ndp_engine *e, int tick, int stage_lo, int stage_hi, void *stream);

/* ABI 218.  The launches ONE tick of `e` makes, in launch order, without making them: what ndp_engine_run validates and chooses
 * (the same checks, codes and messages), and nothing else -- no HIP call, no buffer of the engine is dereferenced, so it answers on
 * a machine without a GPU.  A stage has zero launches (stage 4 under the fused or generic backward, stage 1 without a Chamfer
 * term), one, or two (stage 1 of nn_cells_wide: sort, then search).  out [2 * NDP_TICK_KERNELS], *n_out = records written.     */
typedef struct ndp_stage_launch {
    const char *kernel;              /* the kernel's name, a string literal of the library                                    */
    int stage;                       /* 0..NDP_TICK_KERNELS - 1                                                               */
    int grid[3], block;              /* workgroups x, y, z; threads per workgroup                                             */
    int lds_bytes;                   /* dynamic LDS of the launch                                                             */
    int extra;                       /* the kernel's third integer argument (k_eng_nn: stage_x; k_eng_fwd8: warp_tail, 1 = the points
                                        are warped behind the tile loop; k_eng_nn_cells_wide: query chunks Q), -1 where it takes none     */
} ndp_stage_launch;
int ndp_engine_plan(const ndp_engine *e, ndp_stage_launch *out, int *n_out);

#ifdef __cplusplus
}
#endif
#endif /* NDP_HIP_H */
