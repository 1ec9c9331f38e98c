// ndp_kernels.hip -- the one translation unit of libndp_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the NDP per-pair
// optimisation hot path, and the C ABI declared in include/ndp_hip.h.  This file is the spine only: it defines no kernel, no device
// function and no ABI entry.  The include list below, in order, is the file map; a file's kernels and the host
// entries that launch only them live together, entries that choose between files are in ndp_abi.inc.
//
// Compile: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (explicit fmaf only).
#include "ndp_device.h"                // shared by every file below: per-point head math (rotations, warp and its backward), block_fold, jacobi_cs

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_32x32x2f32((a), (b), (c), 0, 0, 0)
#define MFMA16(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

#include "ndp_phase_timing.inc"        // PT_* / PTF stamps of -DNDP_PHASE_TIMING experiment builds (empty in the product)
#include "ndp_level_f32.inc"           // fp32-MFMA level kernels (gemm_mode 0): LDS carve, level forward / backward, k_pyramid_fwd, k_grad_reduce
#include "ndp_ops.inc"                 // single-pair operators: brute-force and latency-shape NN, k_chamfer_bwd, k_landmark, k_adam
#include "ndp_eng_fwd.inc"             // engine forward stage on fp32 (k_eng_fwd); level_freq, xcd_pair_block, NDP_LROW for the stages below
#include "ndp_fwd_split.inc"           // level forward on two-way fp16 splits: k_eng_fwd8, k_pyramid_fwd8; the plane-image format
#include "ndp_nn_onepass.inc"          // one-pass NN on the vector pipe: k_eng_nn, k_eng_nn_lat8 / 16, k_nn1, k_nn1_rows
#include "ndp_nn_matrix.inc"           // one-pass NN with the distances on the bf16 matrix pipe: k_eng_nn_mx8, k_nn2
#include "ndp_eng_loss.inc"            // engine loss stage: loss, early-stop decision, dL/dx' (k_eng_loss)
#include "ndp_eng_bwd.inc"             // engine backward stage on fp32: eng_bwd_job, k_eng_bwd2, k_eng_bwd1
#include "ndp_bwd_split.inc"           // the two-launch backward on fp16 splits: k_eng_bwd2_8, k_eng_bwd1_8
#include "ndp_bwd_fused.inc"           // both backward layers in one launch: k_eng_bwd_f
#include "ndp_eng_update.inc"          // engine update stage: partial fold, Adam, level hand-over (k_eng_update, k_eng_update_rest)
#include "ndp_generic.inc"             // level kernels for every width / depth other than 128 / 3
#include "ndp_abi_common.inc"          // host only: error string, HIP_TRY, check_desc, check_batch / check_offsets, set_smem; ndp_version, ndp_build_id, ndp_abi_sizes
#include "ndp_nsfp.inc"                // NSFP baseline: kernels, ndp_nsfp_fwd / _bwd
#include "ndp_eng_load.inc"            // pair preparation and slot (re)fill: k_pair_means*, LoadJobs, k_eng_load
#include "ndp_nn_cells.inc"            // exact grid ball search (behind LoadJobs: its grid-build kernel rides behind k_eng_load)
#include "ndp_nn_cells_wide.inc"       // the same search for clouds of up to 8192 points: grids sorted in global memory, queries split over workgroups
#include "ndp_abi.inc"                 // host entries that choose between the files above: level / pyramid / engine load, the tick's launch plan (plan_tick) and its launcher, NN shapes, operators
#include "ndp_flow_metrics.inc"        // scene-flow metrics: k_flow_metrics, ndp_flow_metrics
#include "ndp_nerfies.inc"             // Nerfies baseline
#include "ndp_ed.inc"                  // embedded-deformation N-ICP baseline
#include "ndp_jacobian.inc"            // warp with its per-point Jacobian, inverse warp
#include "ndp_sinkhorn.inc"            // Sinkhorn divergence baseline: streamed soft-minimum step / final kernels, fixed-order loss reduce
#include "ndp_normals.inc"             // surface normals: exact K nearest neighbours, PCA normals, point-to-plane residuals and gradient
#include "ndp_rigid.inc"               // rigid alignment from correspondences: weighted Procrustes, residual counts, RANSAC over given triples
#include "ndp_match.inc"               // descriptor matching: S x T row statistics on the f32 MFMA, dual-softmax / dustbin OT / mutual-NN
#include "ndp_kpconv.inc"              // KPConv inputs: voxel barycentre subsampling and fixed-radius neighbours on a sorted cell-key table
#include "ndp_kpconv_conv.inc"         // KPConv convolution: neighbour aggregation and the contraction with the kernel weights on the f32 MFMA, one launch
#include "ndp_kpconv_bwd.inc"          // KPConv backward in the features and the weights: transposed neighbour table, slabbed edge gradients, blocked dW
#include "ndp_attention.inc"          // multi-head soft-max attention with rotary codes, fused: scores and P V on the f32 MFMA, online soft-max
