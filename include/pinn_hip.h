/* C-ABI of the MI355X-native PINN-elastodynamics hot path (libpinn_hip.so).
 *
 * The reference (Raocp/PINN-elastodynamics) has no FFI: its "operator interface" for this path is
 * the method surface of the TF1 model class.  Each entry point below names the reference graph
 * piece it replaces (file:line relative to the reference repository, INF =
 * ElasticWaveInfinite/ElasticWave.py).  INTEGRATION.md shows the ctypes binding a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - every pointer except `layers`, `lb`, `ub`, `term_weights`, `out_weights` is a DEVICE pointer
 *     owned by the caller; the library allocates nothing and keeps no state between calls;
 *   - all work is enqueued on `stream` (a hipStream_t passed as void*); calls return immediately;
 *   - return value: 0 on success, a negative PINN_ERR_* code for bad arguments, a positive
 *     hipError_t value if a launch failed.  Nothing throws.
 *   - flat parameter vector: W0, b0, W1, b1, ... with each W row-major [in, out] and each b of
 *     length out -- the arrays of the reference checkpoint [W_list, b_list] (INF:159-165)
 *     concatenated layer by layer;
 *   - `layers` = {3, H, ..., H, n_out} exactly like the reference's uv_layers (INF:645).
 */
#ifndef PINN_HIP_H
#define PINN_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* precision_mode: operand type of the matrix pipe (accumulation is always fp32) */
enum {
    PINN_PREC_BF16 = 0,   /* bf16 operands, one MFMA per product (BASELINE config "bf16-MFMA/fp32-accum") */
    PINN_PREC_F16X3 = 1,  /* fp16 hi + scaled-lo split, three MFMAs per product: fp32-class accuracy.  Limits of the class (DESIGN
                             section 7): (1) the hi + lo weights carry ~23 significant bits -- their split error is 1.75x the fp32
                             rounding of the same weights and, like it, the same for every point: where a residual is a > 1000-fold
                             cancellation of O(1) outputs (the plate's hole traction at trained weights) the gradient error does
                             not fall with the number of points as host fp32's does; (2) the weight gradient of padded widths <= 64
                             takes the layer states as fp16 high parts, and in the four- and five-stream collocation kernels the adjoints too (round 4: one
                             MFMA per product; forward and reverse chain keep hi + lo): a random rounding noise of 3.5e-4 / sqrt(points)
                             relative to the gradient (1e-5 at 4096 points, 2.5e-7 at 2 M) that stays inside host-fp32's own per-layer error at
                             the reference's trained weights -- the wider layouts use both parts of both;
                             (3) |w| <= 2047 in the
                             fused kernels' weight format (32 w must stay finite in fp16).  A larger weight is DETECTED when the weights
                             are packed: the call then returns NaN in every gradient entry and every loss sum (never a plausible wrong
                             number) -- pass PINN_FLAG_TWO_KERNEL to evaluate such weights (the two-kernel path holds |w| up to 65504);
                             pinn_fused_weight_limit() returns the bound;  (4) the collocation kernels of padded width 64 (wave and plate
                             heads, 8 or 4 hidden layers) hand the per-layer states to their activation reverse as fp16 high part + the TOP BYTE
                             of the fp16 low part (14 significant bits; round 4): measured at the reference's trained nets the gradient blocks
                             stay where full low parts put them (tools/studies/wgrad_operand_study.py, the per-layer fp32 bounds of the GPU
                             tests); since round 5 the lowest parked state of the four-stream kernel (S_2) travels without that byte -- which layers'
                             low parts the reverse needs was priced layer by layer (tools/studies/lo_policy_study.py: the upper layers carry it; at
                             the most sensitive reference net the worst per-layer multiple of fp32's own error moves 3.9 -> 4.6 of the tests' bound
                             of 6, elsewhere not at all); PINN_FLAG_STATE_FP16 drops the low parts altogether and is NOT parity-grade. */
    PINN_PREC_F16 = 2,    /* fp16 operands, one MFMA per product */
    PINN_PREC_BF16X3 = 3, /* bf16 hi/lo split, three MFMAs per product (16-bit significand).  As in PINN_PREC_F16X3 (2), the weight gradient
                             of padded width 64 takes the layer states (four- and five-stream kernels: the adjoints too) as high parts only --
                             here bf16 ones, 8 significant bits against fp16's 11: a random rounding noise c / sqrt(points) relative to the
                             gradient, about 8x the f16x3 one.  Measured on an MI355X at fresh Xavier weights (n = 64 / 1 024 / 16 384,
                             mean of four draws, tools/narrow_noise_study.py): c = 2.5e-3 for the four-stream wave head, 5.5e-3 for the one-stream value heads
                             (pinn_data_loss_grad, the hole traction), 9e-3 for the five-stream plate head (f16x3: 3e-4 / 7e-4 / 1.1e-3);
                             the two-kernel path and the wider layouts use both parts of both (1e-5). */
    PINN_PREC_FP32 = 4,   /* plain fp32 FMA arithmetic, no matrix pipe (the reference's own precision, INF:71-92): ~100x slower,
                             for parity checks; offered by every entry point (wave, data, fields, the plate family with its second
                             time derivative, the 4-input heads) */
    /* OR this into precision_mode when the PREVIOUS call on the same workspace used the same params_flat contents, layers and
     * mode: the packed MFMA weight fragments are still in the workspace and the repack launch is skipped (the reference feeds
     * one set of variables to every loss term of a step, INF:297-305; a step makes 3-4 calls). */
    PINN_FLAG_WEIGHTS_PACKED = 0x100,
    /* OR this into precision_mode to let the fused kernel of the 8-layer, width <= 64 collocation path park its per-layer states as fp16
     * high parts only (no low parts): 17 % faster, but the activation reverse then sees states rounded to 2^-12, which cancellation at
     * TRAINED weights amplifies (first-layer gradient blocks 5e-3 off at the reference's trained nets, fp32 itself 2e-4).  Fine far
     * from an optimum (early Adam steps); not parity-grade.  Ignored where it does not apply. */
    PINN_FLAG_STATE_FP16 = 0x200,
    /* OR this into precision_mode to keep this call off the fused persistent kernel: forward / reverse chain and weight gradient run as
     * the two-kernel path (state and adjoint panels through the workspace): slower, no |w| <= 2047 bound (see PINN_PREC_F16X3). */
    PINN_FLAG_TWO_KERNEL = 0x400
    /* PINN_ADJOINT_SHIFT(k), k = 0..24, may be OR'ed in as well: see below */
};

enum {
    PINN_OK = 0,
    PINN_ERR_NULL = -1,        /* a required pointer is NULL */
    PINN_ERR_LAYERS = -2,      /* unsupported layer list (see pinn_supported_width) */
    PINN_ERR_PRECISION = -3,   /* unknown precision_mode */
    PINN_ERR_WORKSPACE = -4,   /* workspace smaller than pinn_min_workspace_bytes() or misaligned */
    PINN_ERR_SIZE = -5,        /* n < 0 (n == 0 is a valid empty batch: zero sums, zero / untouched gradient); pinn_select_k: n >= 2^31 or k outside 0 .. n;
                                  pinn_sample_box / pinn_refine_keys: n >= 2^31, n_balls outside 0 .. PINN_MAX_BALLS, a ball's ndim outside {2, 3};
                                  pinn_binned_sums / pinn_causal_cdf / pinn_sample_box_cdf: n >= 2^31, n_bins outside 1 .. PINN_MAX_TIME_BINS, a bad range, eps or floor */
    PINN_ERR_COLLECTIVE = -6,  /* pinn_p2p_*: not connected; a coarse-grained buffer across devices (pinn_p2p_connect); or a rank did not arrive within the
                                * bounded wait of some call (pinn_p2p_set_timeout_ms, default 30 s) -- that call's buffer is then NaN on this rank */
    PINN_ERR_RANGE = -7,       /* pinn_wave2d_loss_grad_checked: gradient non-finite even on the two-kernel path with the reverse pass scaled by 2^-24 */
    PINN_ERR_STATE = -8,       /* pinn_lbfgs_*: state buffer shorter than pinn_lbfgs_state_bytes, not 256-byte aligned, or initialised for other sizes */
    PINN_ERR_HISTORY = -9      /* pinn_lbfgs_*: history outside 1 .. PINN_LBFGS_MAX_HISTORY */
};

/* Padded hidden width the kernels use for a real hidden width h (0 if unsupported). */
int pinn_supported_width(int h);
/* Largest |w| the fused kernels' weight format holds (2047); see PINN_PREC_F16X3 (3) and PINN_FLAG_TWO_KERNEL. */
float pinn_fused_weight_limit(void);

/* Which kernel path a loss + gradient call takes (round 5: no silent slow path).  `head` names the entry point family, `ws_bytes` is the
 * workspace the calls will be given (0: assume pinn_workspace_bytes() of a large set).  The answer is the rule the calls themselves apply
 * (same code), so a caller -- the model classes warn once -- can tell BEFORE training that a net lands on the two-kernel path, which is
 * 2.3-5x slower than the fused persistent kernel (profiles/r04_conf_time.txt): the fused kernel is compiled for the depths the reference
 * uses (padded width <= 64: 4 or 8 hidden layers; 96 / 128: 8; 160: 6; the 3-D net: 10 x 128). */
enum {
    PINN_HEAD_WAVE = 0,        /* pinn_wave2d_loss_grad: four streams */
    PINN_HEAD_DATA = 1,        /* pinn_data_loss_grad(_multi), pinn_plate2d_traction_loss_grad: one stream */
    PINN_HEAD_PLATE = 2,       /* pinn_plate2d_loss_grad: five streams (second time derivative) */
    PINN_HEAD_NC3D = 3,        /* pinn_nc3d_loss_grad: four inputs, five first-order streams */
    PINN_HEAD_NC3D_DATA = 4,   /* pinn_nc3d_data_loss_grad */
    PINN_HEAD_STREAMS = 5,     /* pinn_stream_loss_grad (the plate's pre-training losses, one set per call): always the two-kernel path */
    PINN_HEAD_STREAM_SETS = 6  /* pinn_stream_loss_grad_multi (all sets of a pre-training loss in one call): five streams; fused for 4 hidden layers
                                  of padded width <= 64 in f16x3 (bf16x3: padded width 64), the two-kernel path for every other net */
};
enum {
    PINN_PATH_FUSED_REGISTERS = 1,   /* fused persistent kernel, tile state in registers (padded width <= 64) */
    PINN_PATH_FUSED_LDS = 2,         /* fused persistent kernel, LDS-operand layout (padded widths 96 / 128 / 160) */
    PINN_PATH_TWO_KERNEL = 3,        /* chain_kernel + wgrad_kernel with state / adjoint panels through the workspace */
    PINN_PATH_FP32 = 4               /* PINN_PREC_FP32: the checker mode, no matrix pipe */
};
/* returns a PINN_PATH_* value, or a negative PINN_ERR_* code (unsupported layer list / precision mode) */
int pinn_path_for(const int* layers, int n_layers, int precision_mode, int head, size_t ws_bytes);
/* Process-wide counters of the paths the loss + gradient calls actually took since the last reset: counts[PINN_PATH_*] (index 0 unused).
 * `reset` != 0 zeroes them after the read.  Tests assert with it that a case ran where it was meant to run. */
void pinn_debug_path_counts(int64_t counts[5], int reset);

/* Workspace sizing.  `recommended` holds all tiles of an n-point call in one pass; anything
 * >= `min` works (the call then walks the points in several chunks).  The fused persistent kernel (one launch per call, what the
 * published numbers are measured with) needs one scratch image per workgroup on top of the fixed part -- pinn_workspace_bytes() of a
 * few hundred thousand points covers its 256 workgroups for every net --; a workspace that holds fewer than 64 of them makes the call
 * take the two-kernel path instead (same results, slower), it never runs a persistent launch on a handful of CUs. */
size_t pinn_workspace_bytes(const int* layers, int n_layers, int64_t n, int precision_mode);
size_t pinn_min_workspace_bytes(const int* layers, int n_layers, int precision_mode);

/* Replaces net_f_sig + the seven mean-squares + their gradient: INF:221-265 (SEMI:228-272,
 * CONF:304-348), INF:104-110, and d/d(W,b) as built by optimizer_Adam.minimize INF:131-133.
 *   loss_terms_out[i] = sum_n f_i(n)^2, i in (f_u,f_v,f_ut,f_vt,f_s11,f_s22,f_s12)   (INF:265 order)
 *   grad_flat_out (+)= d/dparams sum_i term_weights[i] * loss_terms[i]
 * The caller folds the loss layout (INF:119 / SEMI:127 / CONF:156) and reduce_mean's 1/N into
 * term_weights.  normalize != 0 applies INF:191's input map with lb/ub. */
int pinn_wave2d_loss_grad(const float* params_flat, const int* layers, int n_layers,
                          const float* x, const float* y, const float* t, int64_t n,
                          const double lb[3], const double ub[3], int normalize,
                          double E, double mu, double rho, int plane_strain,
                          const float term_weights[7],
                          float* loss_terms_out, float* grad_flat_out, int accumulate,
                          int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Same call, but brackets every kernel with HIP events on `stream` and returns, in the HOST array
 * kernel_ms, the summed durations of {weight repack, chain kernel (forward + reverse chain),
 * weight-gradient kernel, small reductions}.  Synchronous; used by bench.py's roofline leg only. */
int pinn_wave2d_loss_grad_profile(const float* params_flat, const int* layers, int n_layers,
                                  const float* x, const float* y, const float* t, int64_t n,
                                  const double lb[3], const double ub[3], int normalize,
                                  double E, double mu, double rho, int plane_strain,
                                  const float term_weights[7],
                                  float* loss_terms_out, float* grad_flat_out, int accumulate,
                                  int precision_mode, void* workspace, size_t ws_bytes, void* stream,
                                  float kernel_ms[4]);

/* Replaces the value-only terms on the small side sets and their gradient: loss_IC INF:111-114,
 * loss_SRC INF:115-116, loss_NB INF:117-118 (SEMI:125-126), loss_FIX CONF:145-146.
 *   loss_terms_out[o] = sum_n (Y_o(n) - targets[o][n])^2      (targets == NULL means 0)
 *   grad_flat_out (+)= d/dparams sum_o out_weights[o] * loss_terms[o]
 * targets is SoA [n_out][n]. */
int pinn_data_loss_grad(const float* params_flat, const int* layers, int n_layers,
                        const float* x, const float* y, const float* t, int64_t n,
                        const double lb[3], const double ub[3], int normalize,
                        const float* targets, const float* out_weights,
                        float* loss_terms_out, float* grad_flat_out, int accumulate,
                        int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Replaces net_uv + the Jacobian pieces net_e needs (INF:201-219), i.e. what predict/probe
 * evaluate (INF:337-359):  fields_out is SoA [4*n_out][n] = Y, dY/dx, dY/dy, dY/dt. */
int pinn_wave2d_fields(const float* params_flat, const int* layers, int n_layers,
                       const float* x, const float* y, const float* t, int64_t n,
                       const double lb[3], const double ub[3], int normalize,
                       float* fields_out, int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Per-point residual measure of the wave family -- net_f_sig (INF:221-265) evaluated for ranking, not for a loss:
 *   score_out[n] = sum_i term_weights[i] * f_i(n)^2,  i in (f_u,f_v,f_ut,f_vt,f_s11,f_s22,f_s12)   (INF:265 order)
 * score_out is a DEVICE array of n floats, term_weights a host array used as given (no normalisation).  Forward only: the four streams of
 * pinn_wave2d_fields, the seven residuals formed from them in the kernel, one float stored per point (fields stores 28).  Every compiled
 * family (all widths and operand modes, any depth) and PINN_PREC_FP32; one launch behind the repack, so pinn_min_workspace_bytes() is
 * enough for any n (PINN_PREC_FP32 walks the points in passes, as its fields call does); honours PINN_FLAG_WEIGHTS_PACKED; n == 0 is a
 * valid no-op.  Not a loss + gradient call: pinn_debug_path_counts does not count it.
 * Accuracy: the forward is the one of pinn_wave2d_fields in the same mode (the same kernel code up to the head); on top of it the head rounds
 * at most 16 eps32 * sum_i w_i a_i^2, a_i = the sum of the absolute values of the terms of f_i (measured: <= 0.12 of that bound in every
 * family).  Against the float64 residuals, relative L2 of s and of sqrt(s) over 1000 collocation points as a multiple of the same error of the
 * residuals evaluated in float32 on the host (MI355X; profiles/residual_score_accuracy.txt): f16x3 1.4 / 1.2 / 1.2 at fresh 4x32, fresh 8x64 and
 * the reference's trained 8x80 net, PINN_PREC_FP32 1.1 / 1.8 / 1.0.  Inside the source disc, where a trained net was never asked to satisfy the
 * equations, single points reach scores 1e6 times the median; a norm over a set that contains one is that point's rounding alone. */
int pinn_wave2d_residual_score(const float* params_flat, const int* layers, int n_layers,
                               const float* x, const float* y, const float* t, int64_t n,
                               const double lb[3], const double ub[3], int normalize,
                               double E, double mu, double rho, int plane_strain,
                               const float term_weights[7], float* score_out,
                               int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* The predict head of the wave family -- what predict evaluates (INF:337-347: net_uv INF:201-211 and net_e INF:213-219 on a point set) in one
 * launch that carries the STRAIN streams only: value, d/dx, d/dy.  The time tangent, which no predict output reads, is not computed.
 *   out is a DEVICE array, SoA [8][n], rows in the order  u, v, s11, s22, s12, e11, e22, e12
 *   u, v, s11, s22, s12 = outputs 0, 1, 4, 5, 6;  e11 = du/dx, e22 = dv/dy, e12 = du/dy + dv/dx  (the velocities ut, vt are not part of predict)
 * The forward is the one of pinn_wave2d_fields in the same mode for the streams carried (the same per-stream kernel code; the carried streams
 * agree with the fields call bit for bit), the head adds one rounding in e12.  Every compiled family (all widths and operand modes, any depth)
 * and PINN_PREC_FP32; one launch behind the repack, so pinn_min_workspace_bytes() is enough for any n (PINN_PREC_FP32 walks the points in
 * passes); honours PINN_FLAG_WEIGHTS_PACKED; n == 0 is a valid no-op.  Not a loss + gradient call: pinn_debug_path_counts does not count it.
 * layers must end in 7 outputs.  Timing: profiles/predict_head_calls.txt. */
int pinn_wave2d_predict(const float* params_flat, const int* layers, int n_layers,
                        const float* x, const float* y, const float* t, int64_t n,
                        const double lb[3], const double ub[3], int normalize,
                        float* out, int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* What the collocation data say about the material constants: fp64 sums over a point set of the wave residuals' squares and of their products
 * with the streams they are linear in.  net_f_sig (INF:221-265) is linear in the Hooke coefficients (c1, c2, G) and in rho, so the derivative
 * of a collocation loss by each of them is a moment sum of quantities the forward pass already carries -- no reverse pass.
 *   sums_out  DEVICE array of PINN_MATERIAL_SUMS doubles:
 *     k = 0..6 :  sum_n f_k(n)^2,  k in (f_u, f_v, f_ut, f_vt, f_s11, f_s22, f_s12)      (what the loss call reports, here in fp64)
 *     k = 7    :  sum_n f_s11 * e11        e11 = du/dx,  e22 = dv/dy,  e12 = du/dy + dv/dx   (INF:216-218)
 *     k = 8    :  sum_n f_s11 * e22
 *     k = 9    :  sum_n f_s22 * e11
 *     k = 10   :  sum_n f_s22 * e22
 *     k = 11   :  sum_n f_s12 * e12
 *     k = 12   :  sum_n f_u * d(ut)/dt
 *     k = 13   :  sum_n f_v * d(vt)/dt
 *   For a loss L = sum_i w_i sum_n f_i(n)^2 (w in the order of k = 0..6), with M_k = sums_out[k]:
 *     dL/dc1  = -2 (w4 M7 + w5 M10)        dL/dc2  = -2 (w4 M8 + w5 M9)
 *     dL/dG   = -2 w6 M11                  dL/drho = -2 (w0 M12 + w1 M13)
 *   No weights enter the call: the sums are raw.  The chain rule from (c1, c2, G) to (E, mu) in either plane mode is the caller's.
 * Forward only: the four streams of pinn_wave2d_fields and the residuals as pinn_wave2d_residual_score forms them (fp32); squares, products and
 * every addition in fp64.  Determinism: one record of partial sums per wave of the launch, written in a fixed place, then one workgroup adds the
 * records in index order -- no floating-point atomics; the sums are a function of the arguments alone.  Every compiled family (all widths and
 * operand modes, any depth) and PINN_PREC_FP32 (which walks the points in passes and adds the passes' totals in pass order);
 * pinn_min_workspace_bytes() is enough for any n; honours PINN_FLAG_WEIGHTS_PACKED; not a loss + gradient call: pinn_debug_path_counts does not
 * count it.  No host synchronisation; n == 0 writes zeros.
 * `sums_workspace` is device memory of pinn_material_sums_workspace_bytes() bytes (the partial records of the largest launch), 256-byte aligned;
 * it is scratch of the call.
 * Errors: layers not ending in 7 outputs: PINN_ERR_LAYERS; n < 0: PINN_ERR_SIZE; a NULL array that is needed: PINN_ERR_NULL; either workspace
 * short or misaligned: PINN_ERR_WORKSPACE.
 * Accuracy: the forward is the one of pinn_wave2d_fields in the same mode; on top of it the head rounds at most
 * 8 eps32 * sum_n a_i(n)^2 (k < 7) or 8 eps32 * sum_n a_i(n) |g(n)| (k >= 7), a_i = the sum of the absolute values of the terms of f_i, g the
 * second factor (measured: <= 0.16 of that bound in every family, 1 to 300 001 points).  Against the float64 sums, max_k |error_k| / S_k
 * (S_k = bound_k / (8 eps32); never |sum_k|: the moment sums cancel at a trained net) over 1000 collocation points as a multiple of the same
 * error of the sums evaluated in float32 on the host (MI355X): f16x3 2.2 / 4.6 / 1.7 at fresh 4x32, fresh 8x64 and the reference's trained 8x80
 * net, PINN_PREC_FP32 0.8 / 0.4 / 1.3.  Timing (the score call's, within 4 %) and the cost in training: profiles/material_sums_calls.txt. */
#define PINN_MATERIAL_SUMS 14
size_t pinn_material_sums_workspace_bytes(void);
int pinn_wave2d_material_sums(const float* params_flat, const int* layers, int n_layers,
                              const float* x, const float* y, const float* t, int64_t n,
                              const double lb[3], const double ub[3], int normalize,
                              double E, double mu, double rho, int plane_strain,
                              double* sums_out,
                              int precision_mode, void* workspace, size_t ws_bytes,
                              void* sums_workspace, size_t sums_ws_bytes, void* stream);

/* Per-field error sums of a predict output against reference data on the device: what the relative L2 comparison with FEM frames needs
 * (sqrt(sums[0][j] / sums[1][j]) per field), without downloading the fields.
 *   pred      DEVICE array [pred_rows][n], e.g. the output of a predict call
 *   rows      HOST array of n_rows entries: row rows[j] of pred is compared with row j of ref (FEM frames carry u, v, s11, s22, s12, no strains)
 *   ref       DEVICE array [n_rows][n]
 *   sums_out  DEVICE array of 2 * n_rows doubles, [2][n_rows]:  sum_i (pred[rows[j]][i] - ref[j][i])^2,  then  sum_i ref[j][i]^2
 * Differences and squares are formed in fp64.  Determinism: per-workgroup partial sums over contiguous index ranges, added by one final pass
 * in a fixed order (the scheme of pinn_refine_keys' mean); no floating-point atomics; the sums are a function of the arguments alone.  Rows of
 * pred that are not selected are never read.  No host synchronisation; n == 0 writes zeros.
 * `workspace` is device memory of pinn_field_error_workspace_bytes(n, n_rows) bytes (0 for arguments the call rejects), 256-byte aligned.
 * Errors: n < 0, n >= 2^31, n_rows outside 1 .. 16, pred_rows < 1 or a rows[j] outside 0 .. pred_rows - 1: PINN_ERR_SIZE; a NULL array that is
 * needed: PINN_ERR_NULL; short or misaligned workspace: PINN_ERR_WORKSPACE. */
size_t pinn_field_error_workspace_bytes(int64_t n, int n_rows);
int pinn_field_error_sums(const float* pred, int64_t pred_rows, const int* rows, int n_rows,
                          const float* ref, int64_t n, double* sums_out,
                          void* workspace, size_t ws_bytes, void* stream);

/* Deterministic top-k / bottom-k selection on the device: which k of the n floats in `score` are the largest (largest != 0) or the smallest.
 *   order   each float maps to a uint32 key that is monotone in the float order (sign-flip map: -0 < +0, a positive NaN above +inf, a negative
 *           NaN below -inf); elements are ordered by key (descending if `largest`, else ascending), then by index ascending
 *   result  the first k indices of that order, written to idx_out (device int32[k]) in ASCENDING INDEX order
 * Radix select on the keys (four 8-bit passes), then a stable compaction; integer atomics only, so the result is exactly reproducible; no host
 * synchronisation; any n.  `workspace` is device memory of pinn_select_workspace_bytes(n) bytes, 256-byte aligned, scratch of the call.
 * k == 0 is a valid no-op.  Errors: n < 0, n >= 2^31 or k outside 0 .. n: PINN_ERR_SIZE; short or misaligned workspace: PINN_ERR_WORKSPACE. */
size_t pinn_select_workspace_bytes(int64_t n);
int pinn_select_k(const float* score, int64_t n, int64_t k, int largest, int32_t* idx_out,
                  void* workspace, size_t ws_bytes, void* stream);

/* Candidate points drawn on the device: n points uniform in the box [lo, hi] of dim = 3 (x, y, t) or 4 (x, y, z, t) columns, written to the
 * DEVICE arrays x, y, (z), t of n floats (z is NULL iff dim == 3; lo / hi are host arrays of dim entries).  Replaces a host generator
 * (pointsets.lhs), the float64 -> float32 conversion and the upload in front of a residual-score call.
 *   generator  Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85), counter-based: point i reads the block
 *              counter = (lo32 idx, hi32 idx, stream_id, 0), key = (lo32 seed, hi32 seed), idx = first + i; coordinate k of the point, in the
 *              order x, y, (z), t, is made from output word r_k
 *   value      u = (r_k >> 8) * 2^-24;  min(fma(u, (float)(hi[k] - lo[k]), (float)lo[k]), (float)hi[k]) -- the difference in double, ONE fma
 * Determinism: no state and no host RNG; a point is a function of (seed, stream_id, idx, lo, hi) alone, whatever the grid, so the call
 * (first + m, n - m) gives the tail of the call (first, n), and ranks / rounds that use distinct stream ids get distinct points without
 * coordination.  One launch, no workspace, no host synchronisation; n == 0 is a valid no-op.
 * Errors: n < 0 or n >= 2^31: PINN_ERR_SIZE; dim outside {3, 4}: PINN_ERR_LAYERS; a NULL array: PINN_ERR_NULL. */
int pinn_sample_box(uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n, int dim,
                    const double lo[4], const double hi[4],
                    float* x, float* y, float* z, float* t, void* stream);

/* Selection keys from scores: what stands between a residual-score call and pinn_select_k when regions are excluded or points are to be DRAWN
 * with probability proportional to a residual measure instead of taken greedily.  Replaces host-side rejection of candidates (DelSrcPT,
 * DelHolePT) and a host-side weighted draw.  score, x, y, z, key_out are DEVICE arrays of n floats; balls is a HOST array.
 *   excluded        a point inside any of the n_balls balls: squared distance in fp32 over the first ndim coordinates (z may be NULL when no
 *                   ball has ndim == 3; x, y too when n_balls == 0), against the fp32 square of the radius; d2 < r2 excludes, and d2 == r2 as
 *                   well when keep_boundary == 0 (the two conventions of DelSrcPT)
 *   PINN_KEYS_MASK    key = score, -inf where excluded; a NaN score stays NaN.  One launch.
 *   PINN_KEYS_SAMPLE  a score that is not finite or is negative counts as excluded too.  q = score^power (the score itself at power == 1,
 *                   sqrtf at 0.5, powf otherwise), m = the mean of q over the points not excluded, p = q / (float)m + (float)c (the quotient
 *                   taken as 0 when m == 0 or no point is valid), u = ((r_0 >> 9) + 0.5) * 2^-23 from the Philox block of pinn_sample_box
 *                   with the last counter word 1 instead of 0, and  key = logf(p) - logf(-logf(u)),  -inf where excluded or p is not
 *                   positive.  The k largest keys (pinn_select_k with largest = 1) are then a weighted sample without replacement, P ~ p: the
 *                   Efraimidis-Spirakis / Gumbel top-k construction.  Two launches.
 * Determinism: m is accumulated in fp64 as per-workgroup partial sums over contiguous index ranges, which every workgroup of the second launch
 * adds again in the same fixed order; no floating-point atomics; the noise is a function of (seed, stream_id, first + i).  The keys are a
 * function of the arguments alone.  No host synchronisation.
 * `workspace` is device memory of pinn_refine_keys_workspace_bytes(n) bytes (0 for an n the call rejects), 256-byte aligned, scratch of the
 * call.  n == 0 is a valid no-op.
 * Errors: n < 0, n >= 2^31, n_balls outside 0 .. PINN_MAX_BALLS or an ndim outside {2, 3}: PINN_ERR_SIZE; an unknown mode: PINN_ERR_PRECISION;
 * a NULL array that is needed: PINN_ERR_NULL; short or misaligned workspace: PINN_ERR_WORKSPACE. */
typedef struct {
    double centre[3];
    double radius;
    int ndim;                  /* 2: disc in (x, y), 3: ball in (x, y, z) */
    int keep_boundary;         /* != 0: points ON the boundary stay */
} pinn_ball;
#define PINN_MAX_BALLS 4
enum { PINN_KEYS_MASK = 0, PINN_KEYS_SAMPLE = 1 };
size_t pinn_refine_keys_workspace_bytes(int64_t n);
int pinn_refine_keys(const float* score, int64_t n, const float* x, const float* y, const float* z,
                     const pinn_ball* balls, int n_balls, int mode, double power, double c,
                     uint64_t seed, uint32_t stream_id, uint64_t first,
                     float* key_out, void* workspace, size_t ws_bytes, void* stream);

/* ---- causal collocation sampling: time-binned score sums, the causal weights and their CDF, a box draw that follows it ---------------------
 * A loss with 1/N weights over points drawn with density ~ w(t) estimates the causally weighted loss of Wang, Sankaran and Perdikaris
 * ("Respecting causality is all you need"): w of a time slice = exp(-eps * accumulated residual of all earlier slices).  The three calls turn
 * per-point scores (pinn_wave2d_residual_score, masked by pinn_refine_keys) into such a set without a host round trip. */
#define PINN_MAX_TIME_BINS 64

/* Per-bin sums of `value` over n_bins equal bins of [lo, hi] of `coord`.  value, coord are DEVICE arrays of n floats; sums_out is a DEVICE array
 * of 2 * n_bins doubles, [2][n_bins]: the sum of value over the points of each bin, then their count (a double, exact).
 *   bin      all in fp32, so that numpy float32 reproduces it bit for bit:  d = coord - (float)lo;  q = d * scale  with
 *            scale = (float)(n_bins / (hi - lo)), the quotient taken in double;  b = (int)floorf(q), clamped to 0 .. n_bins - 1 (points
 *            outside [lo, hi] count in the first / last bin)
 *   skipped  neither summed nor counted: a point whose value is negative, not finite or NaN, or whose coord is NaN -- the -inf keys of
 *            PINN_KEYS_MASK keep excluded balls out of the profile this way
 * Values widen to fp64 before the first addition.  Determinism: per-workgroup partial records over contiguous index ranges, each walked in
 * a fixed order, added by one final pass in a fixed order (the scheme of pinn_field_error_sums); no floating-point atomics; the output is a
 * function of the arguments alone.
 * No host synchronisation; n == 0 writes zeros.
 * `workspace` is device memory of pinn_binned_sums_workspace_bytes(n, n_bins) bytes (0 for arguments the call rejects), 256-byte aligned.
 * Errors: n < 0, n >= 2^31, n_bins outside 1 .. PINN_MAX_TIME_BINS, or lo / hi not finite with hi > lo: PINN_ERR_SIZE; a NULL array that is
 * needed: PINN_ERR_NULL; short or misaligned workspace: PINN_ERR_WORKSPACE. */
size_t pinn_binned_sums_workspace_bytes(int64_t n, int n_bins);
int pinn_binned_sums(const float* value, const float* coord, int64_t n, double lo, double hi, int n_bins,
                     double* sums_out, void* workspace, size_t ws_bytes, void* stream);

/* The causal weights of the bins and the CDF of their density, from the [2][n_bins] output of pinn_binned_sums (`binned`, DEVICE).  w_out is
 * a DEVICE array of n_bins doubles, cdf_out a DEVICE array of n_bins + 1 floats.  In fp64, B = n_bins:
 *   m_b   = sum_b / count_b  (0 where the count is 0)
 *   c_0   = 0,  c_b = c_(b-1) + m_(b-1)  in ascending order
 *   w_b   = exp(-eps * c_b),  so w_0 = 1 exactly
 *   d_b   = max(w_b, floor)
 *   cdf_0 = 0,  cdf_b = (float)((d_0 + .. + d_(b-1)) / (d_0 + .. + d_(B-1)))  with the sums in ascending order,  cdf_B = 1 set explicitly
 * An entry that would come out below its predecessor after rounding, or is no number, takes the predecessor's value: the table never
 * decreases and holds no NaN.  floor = 1 or eps = 0 give the uniform table b / B (exact for B a power of two).  A floor above 1 is used as 1:
 * no w_b exceeds 1, so the densities are equal either way, and their sum cannot overflow however large the floor.
 * One small launch, no workspace, no host synchronisation.
 * Errors: n_bins outside 1 .. PINN_MAX_TIME_BINS, eps < 0, floor < 0 or either not finite: PINN_ERR_SIZE; a NULL array: PINN_ERR_NULL. */
int pinn_causal_cdf(const double* binned, int n_bins, double eps, double floor,
                    double* w_out, float* cdf_out, void* stream);

/* pinn_sample_box with the LAST column (t) drawn from the piecewise-constant density that t_cdf encodes over n_bins equal bins of
 * [lo_t, hi_t]; t_cdf is a DEVICE array of n_bins + 1 floats, t_cdf[0] = 0, t_cdf[n_bins] = 1, never decreasing (pinn_causal_cdf's cdf_out).
 * The call reads the same Philox block (last counter word 0) and the same words: the space columns are bit-identical to pinn_sample_box's
 * for the same (seed, stream_id, first + i).  The time column uses the word it always used:
 *   u = (r >> 8) * 2^-24
 *   b = the largest index in 0 .. n_bins - 1 with t_cdf[b] <= u  -- a bin of zero width is never chosen
 *   f = min((u - t_cdf[b]) / (t_cdf[b+1] - t_cdf[b]), 1)  in fp32, IEEE division
 *   s = ((float)b + f) / (float)n_bins
 *   t = min(fma(s, (float)(hi_t - lo_t), (float)lo_t), (float)hi_t)  -- ONE fma, as the box call
 * With the uniform table b / B, B a power of two, every step of the inverse is exact (u B - b and the divisions by powers of two round
 * nothing), s == u, and ALL columns are bit-identical to pinn_sample_box's.  A point is a function of (seed, stream_id, idx, lo, hi) and the
 * table alone, whatever the grid, so the call (first + m, n - m) gives the tail of the call (first, n).  One launch (the table is staged in
 * LDS once per workgroup, the search is at most 6 steps), no workspace, no host synchronisation; n == 0 is a valid no-op.
 * Errors: n < 0, n >= 2^31 or n_bins outside 1 .. PINN_MAX_TIME_BINS: PINN_ERR_SIZE; dim outside {3, 4}: PINN_ERR_LAYERS; a NULL array (t_cdf
 * included, whatever n): PINN_ERR_NULL. */
int pinn_sample_box_cdf(uint64_t seed, uint32_t stream_id, uint64_t first, int64_t n, int dim,
                        const double lo[4], const double hi[4], const float* t_cdf, int n_bins,
                        float* x, float* y, float* z, float* t, void* stream);

/* ---- plate-with-hole family (PLATE = PlateHoleQuarter/train/train.py); precision_mode must be a split mode ---------------
 * Streams of one net at raw or normalised (x,y,t): streams_out is SoA [5][n_out][n] = Y, dY/dx, dY/dy, dY/dt, d2Y/dt2.
 * Replaces the tf.gradients calls of net_dist_dt / net_part / net_vel (PLATE:330-356,398-402) and provides the frozen
 * distance / particular streams the composite needs. */
int pinn_net_streams(const float* params_flat, const int* layers, int n_layers,
                     const float* x, const float* y, const float* t, int64_t n,
                     const double lb[3], const double ub[3], int normalize,
                     float* streams_out, int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Replaces net_f_sig of the plate (composite u = P + D*N, PLATE:358-388; nested u_tt, plane stress, PLATE:404-439), the
 * five mean-squares PLATE:187-191 and their gradient w.r.t. the uv net only (D, P frozen, PLATE:240-241,249-250).
 *   frozen_streams: SoA [2][5][5][n] = streams (value,x,y,t,tt) x fields (u,v,s11,s22,s12) of D, then of P (pinn_net_streams)
 *   loss_terms_out[i] = sum_n f_i(n)^2, i in (f_u, f_v, f_s11, f_s22, f_s12)   (PLATE:439 order) */
int pinn_plate2d_loss_grad(const float* params_flat, const int* layers, int n_layers,
                           const float* x, const float* y, const float* t, int64_t n,
                           const double lb[3], const double ub[3], int normalize,
                           const float* frozen_streams, double E, double mu, double rho,
                           const float term_weights[5],
                           float* loss_terms_out, float* grad_flat_out, int accumulate,
                           int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Per-point residual measure of the plate family -- net_f_sig of the plate (composite PLATE:358-388, residuals PLATE:404-439) evaluated for
 * ranking, not for a loss:
 *   score_out[n] = sum_i term_weights[i] * f_i(n)^2,  i in (f_u, f_v, f_s11, f_s22, f_s12)   (PLATE:439 order)
 * score_out is a DEVICE array of n floats, term_weights a host array used as given (no normalisation), frozen_streams the [2][5][5][n] array
 * of pinn_plate2d_loss_grad at the same points.  Forward only: the five streams of pinn_net_streams, the composite and the five residuals
 * formed from them in the kernel, one float stored per point (pinn_net_streams stores 25 and leaves the composite to the caller).  Split
 * modes of every compiled width and PINN_PREC_FP32 (the other 16-bit modes: PINN_ERR_PRECISION, as the loss call); one launch behind the
 * repack, so pinn_min_workspace_bytes() is enough for any n (PINN_PREC_FP32 walks the points in passes); honours PINN_FLAG_WEIGHTS_PACKED;
 * n == 0 is a valid no-op.  Not a loss + gradient call: pinn_debug_path_counts does not count it.
 * Accuracy: the forward is the one of pinn_net_streams in the same mode (the same kernel code up to the head); on top of it the head rounds
 * at most 24 eps32 * sum_i |w_i| a_i^2, a_i = the sum of the absolute values of the leaf terms (P, D*N, 2*D*N, with their coefficients) of f_i
 * (measured: <= 0.10 of that bound in every family).  Against the float64 residuals, relative L2 of s and of sqrt(s) over 1000
 * collocation points as a multiple of the same error of the residuals evaluated in float32 on the host (MI355X;
 * profiles/residual_score_accuracy.txt), D and P from the reference's trained nets: f16x3 0.55 / 1.08 at a fresh 4x32 net,
 * 1.16 / 1.74 at the reference's trained 8x70 net, 1.92 / 2.32 at the trained 8x64 net; PINN_PREC_FP32 1.91 / 1.18, 0.73 / 1.11, 1.12 / 1.34.
 * Timing (MI355X, 8x64, 1 M points, profiles/refine_family_calls.txt): 1.24 ms against 1.47 ms for pinn_net_streams plus the composite and
 * residual formulas in torch on the device. */
int pinn_plate2d_residual_score(const float* params_flat, const int* layers, int n_layers,
                                const float* x, const float* y, const float* t, int64_t n,
                                const double lb[3], const double ub[3], int normalize,
                                const float* frozen_streams, double E, double mu, double rho,
                                const float term_weights[5], float* score_out,
                                int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* pinn_wave2d_material_sums for the plate family: what the collocation data say about E, mu and rho of the plane-stress plate.  The five
 * residuals of PLATE:404-439 are linear in the Hooke coefficients (c1, c2, G) of PLATE:416-418 and in rho, so the derivative of a collocation
 * loss by each is a moment sum of the composite's streams -- no reverse pass.
 *   sums_out  DEVICE array of PINN_MATERIAL_SUMS_PLATE doubles:
 *     k = 0..4 :  sum_n f_k(n)^2,  k in (f_u, f_v, f_s11, f_s22, f_s12)                    (what the loss call reports, here in fp64)
 *     k = 5, 6 :  sum_n f_s11 * e11,  sum_n f_s11 * e22       e11 = dU/dx, e22 = dV/dy, e12 = dU/dy + dV/dx of the composite F = P + D*N
 *     k = 7, 8 :  sum_n f_s22 * e11,  sum_n f_s22 * e22
 *     k = 9    :  sum_n f_s12 * e12
 *     k = 10,11:  sum_n f_u * d2U/dt2,  sum_n f_v * d2V/dt2
 *   For a loss L = sum_i w_i sum_n f_i(n)^2 (w in the order of k = 0..4), with M_k = sums_out[k]:
 *     dL/dc1  = -2 (w2 M5 + w3 M8)         dL/dc2  = -2 (w2 M6 + w3 M7)
 *     dL/dG   = -2 w4 M9                   dL/drho = -2 (w0 M10 + w1 M11)
 *   No weights enter the call; the chain rule from (c1, c2, G) to (E, mu) -- plane stress -- is the caller's.
 * frozen_streams is the [2][5][5][n] array of pinn_plate2d_loss_grad at the same points.  Forward only: the composite and the residuals as
 * pinn_plate2d_residual_score forms them (fp32); squares, products and every addition in fp64; the order of additions is fixed as in
 * pinn_wave2d_material_sums (one record per wave, one workgroup adds the records in index order; PINN_PREC_FP32 adds its passes' totals in
 * pass order), so the sums are a function of the arguments alone.  Split modes of every compiled width and PINN_PREC_FP32 (the other 16-bit
 * modes: PINN_ERR_PRECISION, as the score call); pinn_min_workspace_bytes() is enough for any n; honours PINN_FLAG_WEIGHTS_PACKED;
 * pinn_debug_path_counts does not count it.  No host synchronisation; n == 0 writes zeros (the point arrays and frozen_streams may be NULL).
 * `sums_workspace`: pinn_material_sums_workspace_bytes() bytes of device scratch, 256-byte aligned -- the one size for all three calls.
 * Errors: layers not 3 inputs -> 5 outputs: PINN_ERR_LAYERS; n < 0: PINN_ERR_SIZE; a NULL array that is needed: PINN_ERR_NULL; either
 * workspace short or misaligned: PINN_ERR_WORKSPACE.
 * Accuracy: the forward is the one of pinn_net_streams in the same mode; on top of it the head rounds at most 24 eps32 * sum_n a_i(n)^2
 * (k < 5) or 24 eps32 * sum_n a_i(n) |g(n)| (k >= 5), a_i = the sum of the absolute values of the leaf terms of f_i (P, D*N, 2*D*N, with their
 * coefficients), |g| the same of the second factor (measured: <= 0.06 of that bound in every family, 1 to 131 073 points).  Against the float64 sums, max_k |error_k| / S_k (S_k = bound_k / (24 eps32))
 * over 1000 collocation points as a multiple of the same error of the sums evaluated in float32 on the host (MI355X): f16x3 1.78 / 0.50 / 0.98 at a fresh 4x32 net and the
 * reference's trained 8x70 and 8x64 nets, PINN_PREC_FP32 1.85 / 0.52 / 0.43.
 * Timing and the cost in training: profiles/material_family_calls.txt. */
#define PINN_MATERIAL_SUMS_PLATE 12
int pinn_plate2d_material_sums(const float* params_flat, const int* layers, int n_layers,
                               const float* x, const float* y, const float* t, int64_t n,
                               const double lb[3], const double ub[3], int normalize,
                               const float* frozen_streams, double E, double mu, double rho,
                               double* sums_out,
                               int precision_mode, void* workspace, size_t ws_bytes,
                               void* sums_workspace, size_t sums_ws_bytes, void* stream);

/* The predict head of the plate family -- what predict evaluates (PLATE:561-570: the composite fields and strains of PLATE:358-388 on a point
 * set) in one launch of the uv net that carries the strain streams only: value, d/dx, d/dy (no time tangent, no second time derivative).
 *   frozen_streams  the [2][5][5][n] array of pinn_plate2d_loss_grad at the same points.  ONLY stream rows 0, 1, 2 (value, x, y) of D and of P
 *                   are read; rows 3 and 4 may hold anything
 *   composite       F0 = P0 + D0 N0,  Fk = Pk + Dk N0 + D0 Nk  (k = 1, 2), as pinn_plate2d_residual_score forms it
 *   out is a DEVICE array, SoA [8][n], rows in the order  u, v, s11, s22, s12, e11, e22, e12
 *                   = F0[u], F0[v], F0[s11], F0[s22], F0[s12], F1[u], F2[v], F2[u] + F1[v]
 * The forward is the one of pinn_net_streams in the same mode for the streams carried (the same per-stream kernel code), the head adds at
 * most six roundings (e12).  Split modes of every compiled width and PINN_PREC_FP32 (the other 16-bit modes: PINN_ERR_PRECISION, as the loss
 * call); any depth; one launch behind the repack, so pinn_min_workspace_bytes() is enough for any n; honours PINN_FLAG_WEIGHTS_PACKED; n == 0
 * is a valid no-op; no path counter moves.  layers must end in 5 outputs.  Timing: profiles/predict_head_calls.txt. */
int pinn_plate2d_predict(const float* params_flat, const int* layers, int n_layers,
                         const float* x, const float* y, const float* t, int64_t n,
                         const double lb[3], const double ub[3], int normalize,
                         const float* frozen_streams, float* out,
                         int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Replaces net_t + loss_HOLE (PLATE:452-461,192-193) and its gradient w.r.t. the uv net.
 *   frozen_and_normals: SoA [12][n] = D values (5 fields), P values (5 fields), nx, ny at the hole points
 *   loss_terms_out = (sum tx^2, sum ty^2) */
int pinn_plate2d_traction_loss_grad(const float* params_flat, const int* layers, int n_layers,
                                    const float* x, const float* y, const float* t, int64_t n,
                                    const double lb[3], const double ub[3], int normalize,
                                    const float* frozen_and_normals, const float weights[2],
                                    float* loss_terms_out, float* grad_flat_out, int accumulate,
                                    int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Replaces the pre-training losses loss_DIST / loss_PART (PLATE:194-215) and their gradients: a weighted sum of squares
 * over streams and outputs of ONE net,  sum_{s,o} weights[s*n_out+o] * sum_n (Y[s][o][n] - targets[s][o][n])^2
 * (targets SoA [5][n_out][n] or NULL = 0; weights is a host array of 5*n_out floats).
 *   loss_terms_out[o] = sum_s (weights[s][o]/max|weights|) * sum_n (...)^2 */
int pinn_stream_loss_grad(const float* params_flat, const int* layers, int n_layers,
                          const float* x, const float* y, const float* t, int64_t n,
                          const double lb[3], const double ub[3], int normalize,
                          const float* targets, const float* weights,
                          float* loss_terms_out, float* grad_flat_out, int accumulate,
                          int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* All point sets of a pre-training loss in ONE call (loss_DIST: 2 sets, loss_PART: 5; PLATE:194-215):
 *   loss = sum over sets k, streams s, outputs o of  sets[k].weights[s][o] * sum_n (Y[s][o][n] - sets[k].targets[s][o][n])^2
 *   grad_flat_out (+)= d/dparams loss      (the gradient of the UNnormalised loss)
 * The weights of ALL sets are normalised by ONE maximum, wmax = the largest |weights[s][o]| over every set of the call (outputs >= n_out do
 * not count):
 *   sets[k].loss_terms_out[o] = sum_s (sets[k].weights[s][o] / wmax) * sum_n (...)^2
 * so the caller's loss is wmax * the sum of every reported number.  (pinn_stream_loss_grad normalises by its one set's own maximum.)
 * An empty set (n == 0) reports zeros; n_sets <= PINN_MAX_STREAM_SETS.  A target row whose weight is 0 is not read.
 * For 4 hidden layers of padded width <= 64 in a split mode the call is repack (skipped under PINN_FLAG_WEIGHTS_PACKED) | ONE persistent
 * launch over all sets | ONE reduction (pinn_path_for(.., PINN_HEAD_STREAM_SETS, ws_bytes) == PINN_PATH_FUSED_REGISTERS, counted once).
 * Every other case -- another depth or width, PINN_FLAG_TWO_KERNEL, pinn_debug_set_fused(0), an unaligned workspace -- runs the sets
 * one after the other on pinn_stream_loss_grad's path (counted once per non-empty set) and returns the same quantities under the same
 * normalisation; PINN_PREC_FP32 likewise; the non-split 16-bit modes return PINN_ERR_PRECISION.
 * Workspace rule of the fused case: one scratch image per persistent workgroup behind the fixed part of the plan, 120 KB at padded width 32
 * and 240 KB at 64.  The launch uses min(256, images, steps) workgroups, steps = sum_k ceil(n_k / 64), and is declined (the sets then run on
 * the two-kernel path, same results) when the workspace holds fewer than min(64, steps) images.  pinn_min_workspace_bytes() holds 64 images
 * for these nets, and pinn_workspace_bytes(layers, n_max, mode), n_max the largest set, does from n_max = 1500 points on (0.7 images per
 * 16 points): pass the larger of the two, as the host classes do.  pinn_path_for does not know the step count: it answers
 * PINN_PATH_FUSED_REGISTERS when the workspace it is given holds 64 images.
 * The adjoint shift (PINN_ADJOINT_SHIFT) is ignored, as in pinn_stream_loss_grad: the reported sums carry the normalised weights. */
#define PINN_MAX_STREAM_SETS 8
typedef struct {
    const float* x; const float* y; const float* t; int64_t n;
    const float* targets;        /* SoA [5][n_out][n] or NULL (= 0) */
    float weights[5][8];         /* per (stream, output); unused outputs 0 */
    float* loss_terms_out;       /* device, >= n_out floats */
} pinn_stream_set;
int pinn_stream_loss_grad_multi(const float* params_flat, const int* layers, int n_layers,
                                const pinn_stream_set* sets, int n_sets,
                                const double lb[3], const double ub[3], int normalize,
                                float* grad_flat_out, int accumulate,
                                int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* The 16-bit operand modes run the reverse pass on adjoints  2 w_i f_i / max|w|  (fp16: |x| < 65504).  A residual that is
 * orders of magnitude above its trained size -- the first trial points of an L-BFGS line search far from the optimum, a stiff
 * material -- can overflow that range; the sums of squares stay finite but the gradient comes back non-finite.  OR
 * PINN_ADJOINT_SHIFT(k) into precision_mode to run the reverse pass on adjoints scaled by 2^-k (the gradient is scaled back
 * by 2^k in the reduction, so the result is the same number); k > 0 costs accuracy only for adjoint elements that drop below
 * fp16's normal range.  The host classes raise k when a gradient comes back non-finite and lower it again as the loss falls.
 * (pinn_stream_loss_grad, whose reported sums carry the normalised weights, ignores the shift.) */
#define PINN_ADJOINT_SHIFT(k) (((k) & 0x1f) << 16)

/* ---- The finite-gradient ladder as library calls (round 6): what the host classes do around every evaluation whose result they look at
 * (pinn_elastodynamics_amd/elastic_wave.py: evaluate_with_finite_gradient / leave_fused_path_if_weights_out_of_range), for callers of this ABI
 * that are not Python.  Two ranges bound the 16-bit modes: |w| <= pinn_fused_weight_limit() in the fused kernels' weight format (beyond it a
 * call returns NaN throughout: sums AND gradient) and the fp16 range of the reverse pass's adjoints (beyond it the gradient alone is non-finite).
 *   pinn_probe_ranges              one small reduction + a stream synchronisation: is grad_flat[0..n_params) finite, and max |params_flat[i]|
 *                                  (either pointer may be NULL).  Uses 16 bytes at the end of `workspace` (dead data between calls).
 *   pinn_wave2d_loss_grad_checked  pinn_wave2d_loss_grad (overwrite form) + the ladder, SYNCHRONOUS: evaluates with the flags in `state`, probes, and
 *                                  on a non-finite gradient either sets state->two_kernel (a weight beyond the fused format: the calls leave the
 *                                  fused path for good) or raises state->adjoint_shift by 4 (up to 24) and repeats.  PINN_OK: loss sums and gradient
 *                                  are finite and final; PINN_ERR_RANGE: the ladder is exhausted.  The caller keeps `state` between calls (start
 *                                  from zeros) and may lower adjoint_shift again as its loss falls (the host classes do at 1/256 of the loss the
 *                                  shift was raised at).  The TWO_KERNEL flag and the shift bits of precision_mode are ignored: `state` owns them.
 * The other families take the same ladder around their own call: probe, then PINN_FLAG_TWO_KERNEL or PINN_ADJOINT_SHIFT(k + 4). */
typedef struct pinn_range_state {
    int adjoint_shift;   /* in/out: 0..24 */
    int two_kernel;      /* in/out: 0 / 1 */
    int attempts;        /* out: evaluations the last checked call made */
    int reserved;
} pinn_range_state;
int pinn_probe_ranges(const float* params_flat, const float* grad_flat, int64_t n_params, void* workspace, size_t ws_bytes, void* stream,
                      int* grad_finite_out, float* max_abs_weight_out);
int pinn_wave2d_loss_grad_checked(const float* params_flat, const int* layers, int n_layers,
                                  const float* x, const float* y, const float* t, int64_t n,
                                  const double lb[3], const double ub[3], int normalize,
                                  double E, double mu, double rho, int plane_strain,
                                  const float term_weights[7],
                                  float* loss_terms_out, float* grad_flat_out,
                                  int precision_mode, void* workspace, size_t ws_bytes, void* stream, pinn_range_state* state);

/* Several value-only sets in ONE call (the reference evaluates loss_IC, loss_SRC, loss_NB / loss_FIX of a step from one set of
 * variables, INF:111-119,297-305): same arithmetic as pinn_data_loss_grad per set, gradients summed, sums of set k written to
 * sets[k].loss_terms_out[0..n_out).  For nets the fused kernel covers this is one launch instead of n_sets; otherwise the sets
 * are processed one after the other.  n_sets <= PINN_MAX_SETS; empty sets (n == 0) are skipped and report zeros. */
#define PINN_MAX_SETS 4
typedef struct {
    const float* x;
    const float* y;
    const float* t;
    int64_t n;
    const float* targets;      /* SoA [n_out][n] or NULL (= 0) */
    float out_weights[8];
    float* loss_terms_out;     /* device, >= n_out floats */
} pinn_point_set;
int pinn_data_loss_grad_multi(const float* params_flat, const int* layers, int n_layers,
                              const pinn_point_set* sets, int n_sets,
                              const double lb[3], const double ub[3], int normalize,
                              float* grad_flat_out, int accumulate,
                              int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* One call per rank per training step (round 5): what the step of INF:282-319 evaluates -- net_f_sig on the collocation
 * batch (pinn_wave2d_loss_grad's arguments), the value-only side sets (pinn_data_loss_grad_multi's), the gradient of their weighted sum
 * and, with `adam`, the optimizer update of INF:131-133 -- as
 *     weight repack | ONE persistent launch for all point sets | ONE reduction (+ Adam)
 * for the nets whose calls take the register-state fused kernel (padded width <= 64, 4 or 8 hidden layers: pinn_path_for).  The side sets'
 * workgroups are dispatched behind the collocation set's and start on the compute units that run out of collocation steps first, so a set of
 * N points no longer leaves most of the chip idle during its last of ceil(N / 64 / 256) steps (the 250,000-point share of one of 8 GPUs: 67
 * workgroups have a 16th step, 189 do not).  Every other case -- other widths / depths, PINN_PREC_FP32, no side points, an empty batch, a
 * workspace without room for both parts' scratch images -- makes the three calls one after the other inside: the RESULTS are the same bits
 * either way (same partial sums, same order of the final additions, same Adam expression).
 *   adam == NULL: the gradient is left in grad_flat_out (data-parallel ranks all-reduce it, then call pinn_adam_step);
 *   adam != NULL: params_flat, adam->m, adam->v are updated in place behind the reduction (and grad_flat_out still holds the gradient).
 * n_sets may be 0.  Loss sums as in the two calls it replaces. */
typedef struct {
    float* m;                  /* first / second moment, length n_params, updated in place */
    float* v;
    double lr, beta1, beta2, eps;
    int64_t step;              /* 1-based */
} pinn_adam_state;
int pinn_wave2d_step(float* params_flat, const int* layers, int n_layers,
                     const float* x, const float* y, const float* t, int64_t n,
                     const double lb[3], const double ub[3], int normalize,
                     double E, double mu, double rho, int plane_strain,
                     const float term_weights[7], float* loss_terms_out,
                     const pinn_point_set* sets, int n_sets,
                     float* grad_flat_out, int accumulate, const pinn_adam_state* adam,
                     int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* The plate's step the same way (PLATE:187-217: loss = 10 (loss_f_uv + loss_f_s + loss_HOLE)): pinn_plate2d_loss_grad's collocation set and
 * pinn_plate2d_traction_loss_grad's hole set in one persistent launch (five-stream part, then the one-stream part), one reduction (+ Adam).
 * What it saves matters most where the reference spends its time: the L-BFGS stage on ~45 k points is latency-bound (a handful of steps per
 * workgroup), and every evaluation is two launches less.  Same fall-back rule and the same bits as the separate calls. */
int pinn_plate2d_step(float* params_flat, const int* layers, int n_layers,
                      const float* x, const float* y, const float* t, int64_t n,
                      const double lb[3], const double ub[3], int normalize,
                      const float* frozen_streams, double E, double mu, double rho,
                      const float term_weights[5], float* loss_terms_out,
                      const float* hole_x, const float* hole_y, const float* hole_t, int64_t hole_n,
                      const float* hole_frozen_and_normals, const float hole_weights[2], float* hole_loss_terms_out,
                      float* grad_flat_out, int accumulate, const pinn_adam_state* adam,
                      int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* A traction boundary set of the wave family: the traction vector of net_surf_var (INF:267-276: s11 nx + s12 ny, s12 nx + s22 ny) on the
 * net's own stress outputs (u, v, ut, vt, s11, s22, s12; value stream only) with PER-POINT normals and PER-POINT targets -- a traction-free
 * cavity or inclined / curved free surface (targets 0), a prescribed time-dependent load (targets = the load) -- and its gradient:
 *   normals_and_tractions   DEVICE, SoA [4][n] = nx, ny, tx, ty at the set's points (traction-free: rows 2 and 3 zero)
 *   r_x = s11 nx + s12 ny - tx,   r_y = s12 nx + s22 ny - ty
 *   loss_terms_out = (sum r_x^2, sum r_y^2)      grad_flat_out (+)= d/dparams (weights[0] sum r_x^2 + weights[1] sum r_y^2)
 * The normals are used AS GIVEN: they are not normalised, so a caller may fold quadrature weights (arc length x time step) into them.
 * One stream through the net: the paths, workspace rule, flags and precision modes are pinn_data_loss_grad's (every 16-bit mode and
 * PINN_PREC_FP32; pinn_path_for(.., PINN_HEAD_DATA, ..) answers for it; one path count per call); for the nets the one-stream fused kernel
 * covers it runs there as set kind 2.  layers must end in 7 outputs (PINN_ERR_LAYERS); normals_and_tractions == NULL with n > 0 is
 * PINN_ERR_NULL; n == 0 writes zero sums and leaves the gradient as `accumulate` says.
 * Precision: the chain is the data head's, only the adjoint seed differs (three of seven outputs, two products each).  Measured against the
 * float64 oracle (profiles/wave_traction_calls.txt) its error is the data head's at the same net and points: sums 1e-7, gradient 6e-6 at
 * 16 385 points of the 8 x 64 net in PINN_PREC_F16X3, 2.6e-5 at 1000, 2.1e-4 at ONE point (both heads alike: the narrow one-stream kernel
 * hands its states to the weight gradient as fp16 high parts), 1.3e-7 at 8 x 80.  At the trained fixture weights_wave64.npz the error
 * falls with n as the data head's does (9e-5 at 1000 points, 1.6e-5 at 256 000): NO N-dependent bias of the kind the plate's traction
 * head carries was found. */
int pinn_wave2d_traction_loss_grad(const float* params_flat, const int* layers, int n_layers,
                                   const float* x, const float* y, const float* t, int64_t n,
                                   const double lb[3], const double ub[3], int normalize,
                                   const float* normals_and_tractions, const float weights[2],
                                   float* loss_terms_out, float* grad_flat_out, int accumulate,
                                   int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* pinn_wave2d_step with a traction set (INF:267-276, pinn_wave2d_traction_loss_grad's arguments as trac_*).  The value-only sets and the
 * traction set form ONE set table -- the one-stream part of the step's persistent launch, the traction set as set kind 2 behind the
 * value-only sets --, so n_sets <= PINN_MAX_SETS - 1 here (PINN_ERR_SIZE), all of the table's weights are normalised by ONE maximum, and the
 * step stays  weight repack | ONE persistent launch for all point sets | ONE reduction (+ Adam).
 * The fall-back rule and the same-bits guarantee are pinn_wave2d_step's: where the one launch does not apply -- other widths / depths,
 * PINN_PREC_FP32, an empty collocation batch, a workspace without room for both parts, pinn_debug_set_step_launch(0) -- the entry point
 * makes the separate calls inside: pinn_wave2d_loss_grad, then the same set table as one multi-set call into the same gradient, then
 * pinn_adam_step when adam != NULL.  The RESULTS are the same bits either way.  (They are NOT the bits of pinn_wave2d_step followed by
 * pinn_wave2d_traction_loss_grad: a set table has one weight normalisation and its sets share the workgroups' partial sums; the two agree
 * to the mode's accuracy.)
 * trac_loss_terms_out receives the two sums.  trac_n == 0 (trac_* pointers may then be NULL): exactly pinn_wave2d_step's calls, Adam fold
 * included; trac_loss_terms_out, if given, reports zeros.  trac_n > 0 needs every trac_* pointer (PINN_ERR_NULL); trac_n < 0 is
 * PINN_ERR_SIZE.  The arguments -- pointers, sizes, the layer list, the precision word, the collocation call's workspace -- are checked
 * before anything is written; with an EMPTY collocation batch (n == 0) a workspace too small for the sets' own plan is reported by the
 * multi-set call, after the collocation sums were zeroed.
 * Cost: profiles/wave_traction_calls.txt, section 3. */
int pinn_wave2d_step_traction(float* params_flat, const int* layers, int n_layers,
                              const float* x, const float* y, const float* t, int64_t n,
                              const double lb[3], const double ub[3], int normalize,
                              double E, double mu, double rho, int plane_strain,
                              const float term_weights[7], float* loss_terms_out,
                              const pinn_point_set* sets, int n_sets,
                              const float* trac_x, const float* trac_y, const float* trac_t, int64_t trac_n,
                              const float* trac_normals_and_tractions, const float trac_weights[2], float* trac_loss_terms_out,
                              float* grad_flat_out, int accumulate, const pinn_adam_state* adam,
                              int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* ---- 3-D Navier-Cauchy extension (BASELINE.json configs[4]).  NOT in the reference: all four reference scripts are 2-D + time
 * (SURVEY.md section 0), so these entry points have no reference lines to replace; they state the 3-D form of net_f_sig
 * (INF:221-265) the way oracle/nc3d_oracle.py spells it out, and parity for them is unpinned by definition.
 *   layers = {4, H x k, 12}; inputs (x, y, z, t); outputs (u,v,w, ut,vt,wt, s11,s22,s33, s12,s13,s23);
 *   residuals (f_u,f_v,f_w, f_ut,f_vt,f_wt, f_s11,f_s22,f_s33, f_s12,f_s13,f_s23); isotropic Hooke law, E, mu, rho as INF:33-35.
 *   loss_terms_out[i] = sum_n f_i(n)^2 (12 values), grad_flat_out (+)= d/dparams sum_i term_weights[i] * loss_terms[i].
 * Split-precision modes only (PINN_PREC_F16X3 / PINN_PREC_BF16X3).  Workspace sizing: the same two functions (layers[0] == 4). */
int pinn_nc3d_loss_grad(const float* params_flat, const int* layers, int n_layers,
                        const float* x, const float* y, const float* z, const float* t, int64_t n,
                        const double lb[4], const double ub[4], int normalize,
                        double E, double mu, double rho, const float term_weights[12],
                        float* loss_terms_out, float* grad_flat_out, int accumulate,
                        int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Value-only terms of the 4-input net (initial state, sources, the traction-free surface s33 = s13 = s23 = 0 of the half space):
 * pinn_data_loss_grad with four coordinates; targets SoA [n_out][n] or NULL, out_weights[n_out], loss_terms_out[n_out].
 * Round 6: the BASELINE configs[4] net (10 x 128, 12 outputs) takes the fused kernel's one-stream instantiation here as well
 * (pinn_path_for(.., PINN_HEAD_NC3D_DATA) = PINN_PATH_FUSED_LDS), every other layer list the two-kernel path. */
int pinn_nc3d_data_loss_grad(const float* params_flat, const int* layers, int n_layers,
                             const float* x, const float* y, const float* z, const float* t, int64_t n,
                             const double lb[4], const double ub[4], int normalize,
                             const float* targets, const float* out_weights,
                             float* loss_terms_out, float* grad_flat_out, int accumulate,
                             int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Forward only: fields_out [5][n_out][n] = the outputs and their derivatives w.r.t. x, y, z, t (predict of the 3-D case). */
int pinn_nc3d_fields(const float* params_flat, const int* layers, int n_layers,
                     const float* x, const float* y, const float* z, const float* t, int64_t n,
                     const double lb[4], const double ub[4], int normalize,
                     float* fields_out, int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* Per-point residual measure of the 3-D family -- the twelve residuals stated in oracle/nc3d_oracle.py (no reference lines: see above)
 * evaluated for ranking:
 *   score_out[n] = sum_i term_weights[i] * f_i(n)^2,  i in the residual order above
 * Conventions of pinn_wave2d_residual_score: score_out a DEVICE array of n floats, term_weights a host array used as given; forward only, the
 * five streams of pinn_nc3d_fields, the residuals formed in the kernel, one float stored per point (fields stores 60); split modes of every
 * compiled width and PINN_PREC_FP32; pinn_min_workspace_bytes() is enough for any n; honours PINN_FLAG_WEIGHTS_PACKED; n == 0 is a valid
 * no-op; no path counter moves.
 * Accuracy: the forward is the one of pinn_nc3d_fields in the same mode; on top of it the head rounds at most 24 eps32 * sum_i |w_i| a_i^2,
 * a_i = the sum of the absolute values of the terms of f_i with their coefficients (measured: <= 0.08 of that bound in every family).
 * Against the float64 residuals, relative L2 of s and of sqrt(s) over 1000 points as a multiple of the same error of the residuals
 * evaluated in float32 on the host (MI355X; profiles/residual_score_accuracy.txt): f16x3 1.20 / 1.23 at a fresh 3x32 net, 0.76 / 0.76 at a fresh 10x128
 * net; PINN_PREC_FP32 1.54 / 1.54, 1.70 / 1.70.  Timing (MI355X, 10x128, 1 M points, profiles/refine_family_calls.txt): 4.49 ms against
 * 4.85 ms for pinn_nc3d_fields plus the residual formulas in torch on the device. */
int pinn_nc3d_residual_score(const float* params_flat, const int* layers, int n_layers,
                             const float* x, const float* y, const float* z, const float* t, int64_t n,
                             const double lb[4], const double ub[4], int normalize,
                             double E, double mu, double rho, const float term_weights[12], float* score_out,
                             int precision_mode, void* workspace, size_t ws_bytes, void* stream);

/* pinn_wave2d_material_sums for the 3-D family: the twelve residuals of oracle/nc3d_oracle.py are linear in (c1, c2, G) = (lambda + 2G,
 * lambda, G) -- the plane-strain coefficients of INF:238-241 -- and in rho.
 *   sums_out  DEVICE array of PINN_MATERIAL_SUMS_NC3D doubles:
 *     k = 0..11  :  sum_n f_k(n)^2 in the residual order above (f_u, f_v, f_w, f_ut, f_vt, f_wt, f_s11, f_s22, f_s33, f_s12, f_s13, f_s23)
 *     k = 12, 13 :  sum_n f_s11 * e11,  sum_n f_s11 * (e22 + e33)         e11 = du/dx, e22 = dv/dy, e33 = dw/dz,
 *     k = 14, 15 :  sum_n f_s22 * e22,  sum_n f_s22 * (e11 + e33)         e12 = du/dy + dv/dx, e13 = du/dz + dw/dx, e23 = dv/dz + dw/dy
 *     k = 16, 17 :  sum_n f_s33 * e33,  sum_n f_s33 * (e11 + e22)
 *     k = 18..20 :  sum_n f_s12 * e12,  sum_n f_s13 * e13,  sum_n f_s23 * e23
 *     k = 21..23 :  sum_n f_u * d(ut)/dt,  sum_n f_v * d(vt)/dt,  sum_n f_w * d(wt)/dt
 *   For a loss L = sum_i w_i sum_n f_i(n)^2 (w in the order of k = 0..11), with M_k = sums_out[k]:
 *     dL/dc1  = -2 (w6 M12 + w7 M14 + w8 M16)        dL/dc2  = -2 (w6 M13 + w7 M15 + w8 M17)
 *     dL/dG   = -2 (w9 M18 + w10 M19 + w11 M20)      dL/drho = -2 (w0 M21 + w1 M22 + w2 M23)
 * Conventions of pinn_plate2d_material_sums: forward only, the residuals as pinn_nc3d_residual_score forms them (fp32; the pair sums
 * e22 + e33 etc. one fp32 addition each), squares, products and every addition in fp64 in a fixed order; split modes of every compiled width
 * and PINN_PREC_FP32 (which leaves the 24 terms of a pass in two halves of twelve rows -- squares, then moments -- and adds each sum's pass
 * totals in pass order); pinn_min_workspace_bytes() is enough for any n; honours PINN_FLAG_WEIGHTS_PACKED; no path counter moves; no host
 * synchronisation; n == 0 writes zeros (the point arrays may be NULL); `sums_workspace` of pinn_material_sums_workspace_bytes() bytes.
 * Errors: layers not 4 inputs -> 12 outputs: PINN_ERR_LAYERS; n < 0: PINN_ERR_SIZE; a NULL array that is needed: PINN_ERR_NULL; either
 * workspace short or misaligned: PINN_ERR_WORKSPACE; a non-split 16-bit mode: PINN_ERR_PRECISION.
 * Accuracy: the forward is the one of pinn_nc3d_fields in the same mode; on top of it the head rounds at most 12 eps32 * sum_n a_i(n)^2
 * (k < 12) or 12 eps32 * sum_n a_i(n) |g(n)| (k >= 12), a_i = the sum of the absolute values of the terms of f_i with their coefficients, |g|
 * the same of the second factor (measured: <= 0.08 of that bound in every family, 1 to 131 073 points).  Against the float64 sums, max_k |error_k| / S_k over 1000 points as a multiple of the same error
 * of the sums evaluated in float32 on the host (MI355X): f16x3 1.70 / 3.45 at a fresh 3x32 and a fresh 10x128 net, PINN_PREC_FP32 1.03 / 0.92.
 * Timing and the cost in training: profiles/material_family_calls.txt. */
#define PINN_MATERIAL_SUMS_NC3D 24
int pinn_nc3d_material_sums(const float* params_flat, const int* layers, int n_layers,
                            const float* x, const float* y, const float* z, const float* t, int64_t n,
                            const double lb[4], const double ub[4], int normalize,
                            double E, double mu, double rho,
                            double* sums_out,
                            int precision_mode, void* workspace, size_t ws_bytes,
                            void* sums_workspace, size_t sums_ws_bytes, void* stream);

/* Replaces tf.train.AdamOptimizer's update (INF:131-133; TF1 rule: epsilon outside the bias
 * correction).  step is 1-based.  All arrays are length n_params, updated in place. */
int pinn_adam_step(float* params_flat, float* m, float* v, const float* grad_flat, int64_t n_params,
                   double lr, double beta1, double beta2, double eps, int64_t step, void* stream);

/* ---- L-BFGS on the device.  Replaces tf.contrib.opt.ScipyOptimizerInterface(method 'L-BFGS-B') of the reference's second stage -- INF:122-129
 * (construction, options), INF:321-335 (train_bfgs), PLATE:220-247 (the three optimizers, 1000 x loss for the pre-training ones), PLATE:508-559 (the
 * three train_bfgs*) -- without bounds (the reference passes none).  A stage is a stream of kernels:  evaluate | advance | evaluate | advance ...
 * with no host round trip per evaluation; one advance is THREE launches whatever the history length (one pass over the history rows for every inner
 * product, one workgroup for the scalar logic and the m x m triangular solves of the compact representation of Byrd, Nocedal and Schnabel in fp64,
 * one pass that forms the direction and the next point).  All inner products accumulate in fp64 in a fixed order (no atomics): results are a
 * deterministic function of the inputs, so data-parallel ranks that advance on the same all-reduced buffer keep bit-identical parameters.
 *   State: ONE caller-owned device buffer, 256-byte aligned, of pinn_lbfgs_state_bytes bytes: the ring of pairs S[m][P], Y[m][P], x_k, g_k, d
 *   (fp32), S^T Y, Y^T Y, S^T g, Y^T g, the line search and the stop tests (fp64), a ring of the last PINN_LBFGS_LOSS_RING losses, the record.
 *   Loss: loss = sum_j loss_coeffs[j] * loss_sums[j] (j < n_sums <= PINN_LBFGS_MAX_SUMS), formed on the device in fp64; the gradient the optimizer
 *   sees is grad_scale * grad_flat (PLATE:220,230: coefficients and gradient of the pre-training stages carry the factor 1000).
 *   Line search: strong Wolfe with L-BFGS-B's constants (ftol 1e-3, gtol 0.9, xtol 0.1; More-Thuente's safeguarded interpolation), at most maxls
 *   trials, first step min(1, 1/||g||), later 1.  A trial whose loss or gradient is not finite counts as too long and is cut back; it never enters
 *   the history.  s_k is the difference of the two fp32 parameter vectors the loss kernels saw; a pair with s.y <= 2.2e-16 y.y is skipped.
 *   Stop rules (scipy's): (f_k - f_k+1) / max(|f_k|, |f_k+1|, 1) <= ftol; max|g| <= gtol; maxiter; maxfun; line search failed (after one restart
 *   along -g with an empty history); not finite at the start point; PINN_LBFGS_NONFINITE_GRAD: a trial whose LOSS satisfies the decrease condition
 *   came back with a non-finite gradient -- the 16-bit reverse pass overflowed (PINN_ADJOINT_SHIFT): the caller raises the shift and starts again
 *   from params_flat.  At a stop params_flat holds the last accepted point (the best one: every accepted step lowers the loss), and every
 *   further call leaves every buffer bitwise unchanged.
 *   pinn_lbfgs_advance   consumes the evaluation at params_flat (grad_flat, loss_sums) and writes the next point to evaluate into params_flat.
 *                        Asynchronous.  16-byte loads when params_flat and grad_flat are 16-byte aligned, scalar ones otherwise; any n_params.
 *   pinn_lbfgs_status    the ONE synchronising call: copies the record out.
 *   pinn_lbfgs_read_losses   losses of the evaluations [first, first + count) (count <= PINN_LBFGS_LOSS_RING, of the last ring's worth) as doubles.
 *   pinn_lbfgs_debug_read    tests: the current direction (n_params floats) and the held pairs, oldest first (max_pairs rows of n_params floats each;
 *                            any output may be NULL); *pairs_out = pairs held.  Synchronous. */
#define PINN_LBFGS_MAX_HISTORY 64
#define PINN_LBFGS_MAX_SUMS 128
#define PINN_LBFGS_LOSS_RING 1024
enum {
    PINN_LBFGS_RUNNING = 0,
    PINN_LBFGS_GTOL = 1,             /* max|g| <= gtol */
    PINN_LBFGS_FTOL = 2,             /* relative reduction of the loss <= ftol */
    PINN_LBFGS_MAXITER = 3,
    PINN_LBFGS_MAXFUN = 4,
    PINN_LBFGS_LINESEARCH = 5,       /* no acceptable step within maxls trials, also not along -g */
    PINN_LBFGS_NONFINITE_START = 6,  /* loss or gradient not finite at the first point */
    PINN_LBFGS_NONFINITE_GRAD = 7    /* acceptable loss, non-finite gradient: raise the adjoint shift / leave the fused path, start again */
};
typedef struct pinn_lbfgs_options {
    int history;                     /* pairs kept, 1 .. PINN_LBFGS_MAX_HISTORY (scipy: maxcor) */
    int maxiter, maxfun, maxls;
    double ftol, gtol;
} pinn_lbfgs_options;
typedef struct pinn_lbfgs_record {
    int status;                      /* PINN_LBFGS_* */
    int iterations, evaluations;
    int pairs, skipped;              /* pairs held now; pairs skipped by the curvature rule so far */
    int trials;                      /* of the current line search */
    int64_t loss_pos;                /* losses written to the ring so far (== evaluations) */
    double f, max_abs_grad, step;    /* at the last accepted point; the step that reached it */
} pinn_lbfgs_record;
size_t pinn_lbfgs_state_bytes(int64_t n_params, int history);      /* 0 for bad arguments */
int pinn_lbfgs_init(void* state, size_t state_bytes, int64_t n_params, const pinn_lbfgs_options* options, const float* loss_coeffs /* host */,
                    int n_sums, double grad_scale, void* stream);
int pinn_lbfgs_advance(void* state, float* params_flat, const float* grad_flat, const float* loss_sums, void* stream);
int pinn_lbfgs_status(const void* state, pinn_lbfgs_record* host_record, void* stream);
int pinn_lbfgs_read_losses(const void* state, int64_t first, int64_t count, double* host_out, void* stream);
int pinn_lbfgs_debug_read(const void* state, int64_t n_params, int history, float* direction_out, float* s_out, float* y_out, int max_pairs,
                          int* pairs_out, void* stream);

/* ---- Latency-floor all-reduce of the step's buffer [gradient | loss sums] (round 5; SURVEY sections 5 and 8e).  The message is ~119 KB:
 * latency-bound, so a ring or tree buys nothing.  One-shot: every rank WRITES its buffer into a slot of every peer's IPC-mapped receive buffer
 * over its point-to-point xGMI link, flags it, and every rank sums the world's slots locally in rank order (the same bits on every rank) --
 * with the TF1 Adam update of INF:131-133 in the same kernel.  One launch replaces all-reduce + pinn_adam_step and does not depend on RCCL's
 * small-message protocol (RCCL stays the default collective of the model classes; this is `collective="p2p"`).
 *   pinn_p2p_create   allocates this rank's receive buffer (2 parities x world slots x max_floats, fine-grained device memory -- the ONE
 *                     allocation this library makes, owned by the comm object) and returns its IPC handle;
 *   the caller exchanges the world's handles (any out-of-band channel: the model classes use torch.distributed.all_gather_object);
 *   pinn_p2p_connect  opens the peers' buffers;   pinn_p2p_allreduce  buf[0..n) <- sum over ranks, enqueued on `stream`; with `adam` the
 *                     first n_params entries of the sum also update params_flat / adam->m / adam->v;   every rank must make the same calls.
 *   pinn_p2p_status   synchronises the device and returns 0, or PINN_ERR_COLLECTIVE if some call failed;   pinn_p2p_peek_status reads the same
 *                     word (pinned host memory, written by the kernel) WITHOUT synchronising: meaningful behind a synchronisation the caller
 *                     made anyway -- the model classes read it at every host sync point of train() / train_bfgs() and raise.
 * Failure semantics (round 6):
 *   - a call succeeds or fails AS A WHOLE on a rank (grid agreement of its 64 workgroups): never a half-applied sum or Adam update;
 *   - a failed call leaves buf[0..n) = NaN on that rank (a caller that only looks at its loss / gradient still notices), skips Adam, sets the
 *     status word, and writes its call number into every peer's abort word: a peer that arrives later -- or had completed the call already --
 *     fails its current or next call at once.  Failure is sticky: every later call on the comm fails immediately;
 *   - the wait is bounded by the device's constant-rate wall clock: pinn_p2p_set_timeout_ms (default 30 000 ms, or the environment variable
 *     PINN_P2P_TIMEOUT_MS at create time): longer than legitimate skew between ranks (first-step lazy initialisation, a rank writing a
 *     checkpoint), short enough that a dead rank ends the run instead of hanging the GPU;
 *   - pinn_p2p_connect returns PINN_ERR_COLLECTIVE, before mapping anything, if this rank's or a peer's buffer is coarse-grained
 *     (hipExtMallocWithFlags(hipDeviceMallocFinegrained) refused) AND the two live on different physical devices (PCI bus ids travel with the
 *     handles): coarse-grained memory is coherent at kernel boundaries only.  Ranks that share one GPU (the tests) may use it.
 *   - calls of one comm are made on ONE stream (the grid agreement counts workgroups per call number);
 *   - pushes are 16-byte stores when buf is 16-byte aligned and n % 4 == 0 (the model classes' buffers are), 4-byte stores otherwise.
 * Single-node use across physical GPUs is UNVERIFIED on hardware (the builder's boxes have one GPU: world 2 on one device is what the tests run;
 * tests/test_gpu_dp.py::test_p2p_across_two_devices runs where torch.cuda.device_count() >= 2). */
#define PINN_IPC_HANDLE_BYTES 128      /* hipIpcMemHandle_t (64) + memory kind + PCI bus id of the owning device */
typedef struct pinn_p2p_comm pinn_p2p_comm;
int pinn_p2p_create(int rank, int world, int64_t max_floats, pinn_p2p_comm** comm_out, unsigned char handle_out[PINN_IPC_HANDLE_BYTES]);
int pinn_p2p_connect(pinn_p2p_comm* comm, const unsigned char* all_handles /* world x PINN_IPC_HANDLE_BYTES, rank order */);
int pinn_p2p_set_timeout_ms(pinn_p2p_comm* comm, double timeout_ms);
int pinn_p2p_allreduce(pinn_p2p_comm* comm, float* buf, int64_t n, float* params_flat, const pinn_adam_state* adam, int64_t n_params, void* stream);
int pinn_p2p_status(pinn_p2p_comm* comm, int* fine_grained_out);
int pinn_p2p_peek_status(pinn_p2p_comm* comm);
int pinn_p2p_destroy(pinn_p2p_comm* comm);
/* Testing hook (process-wide): 1 makes pinn_p2p_create allocate plain (coarse-grained) device memory, as if the runtime had refused the
 * fine-grained flag; returns the previous setting.  For the refusal test of pinn_p2p_connect. */
int pinn_p2p_debug_force_coarse(int enable);

/* Testing hook (process-wide): 0 forces the two-kernel path (chain + wgrad kernels) even where the
 * fused kernel applies; 1 (default) prefers the fused kernel.  Returns the previous setting.  Both paths
 * compute the same numbers to the precision mode's accuracy (tests/test_gpu_parity.py). */
int pinn_debug_set_fused(int enable);
/* Testing hook (process-wide): 0 makes the step entry points (pinn_wave2d_step, pinn_wave2d_step_traction, pinn_plate2d_step) take their
 * fall-back -- the separate calls inside -- even where the one launch applies; 1 (default) prefers the one launch.  Returns the previous
 * setting.  The results are the same bits either way, which is what the tests hold with it. */
int pinn_debug_set_step_launch(int enable);
/* Tuning hook (process-wide): the XCD-aware step assignment of the fused collocation kernels.  Workgroups are dispatched round-robin over the 8
 * XCDs and the odd XCDs of an MI355X run these kernels 2-3 % slower than the even ones (profiles/r05_workgroup_lifetimes.txt), so the even-XCD
 * workgroups take `permille` / 1000 more steps (as the tail of the launch; default 16).  0 turns it off; returns the previous setting.  The
 * assignment is static: results stay a deterministic function of the inputs and the launch shape. */
int pinn_debug_set_xcd_bonus(int permille);
/* Testing hook (process-wide): at most `cap` workgroups in a fused per-family launch (0: the default, one per compute unit) -- several steps per
 * workgroup on small test inputs.  Returns the previous setting. */
int pinn_debug_set_fused_grid_cap(int cap);
/* Query (round 6): the per-workgroup memory of the fused collocation kernel a layer list takes (f16x3; head = PINN_HEAD_WAVE / _PLATE / _NC3D) and the
 * cache policy compiled into it.  A persistent workgroup owns `*images_bytes` of parked state images and `*sums_bytes` of running weight-gradient
 * sums; a full grid is 256 of them.  Where that exceeds the 256 MB Infinity Cache the kernel marks ONE of the two classes non-temporal so that the other
 * stays resident (profiles/r06_footprint_and_cache_policy.txt).  Returns 0 (no hint), 1 (the sums), 2 (the images), or
 * PINN_ERR_LAYERS for a layer list without fused kernel.  Host-only, no device call. */
int pinn_debug_cache_policy(const int* layers, int n_layers, int head, size_t* images_bytes, size_t* sums_bytes);
/* Profiling hook (process-wide): device buffer of 128 uint64 that the fused kernel fills with shader-clock
 * stamps of its phases (workgroup 0 only); NULL turns it off. */
void pinn_debug_set_stamp_buffer(void* device_u64x128);
/* Rate in kHz of the device wall clock the launch-long stamps use (slots 120 / 121 of the stamp buffer: wall-clock ticks, 124 / 125: shader cycles of
 * workgroup 0 around all of its steps -- a launch's duration and the clock it ran at, measured by the kernel itself); 0 if unknown. */
int pinn_debug_wall_clock_khz(void);
/* Profiling hook (process-wide): host array of 4 floats; while set, every loss+gradient call brackets its kernels with HIP
 * events on the call's stream, synchronises, and writes milliseconds {repack, chain (or the whole fused kernel), weight gradient,
 * reductions} of that call (what pinn_wave2d_loss_grad_profile does for one entry point, here for all of them: bench.py's
 * roofline of the plate / 3-D kernels).  NULL turns it off. */
void pinn_debug_set_profile_buffer(float* host_ms4);
/* Profiling hook (process-wide), asynchronous: _arm(k) starts recording the next k (<= 4096) launches of the fused kernel: each is
 * bracketed by HIP events on its call's stream and nothing synchronises, so a running step loop keeps its back-to-back stream order
 * (bench.py's roofline leg: the launch time under the same conditions as the timed steps).  _read() stops the recording, waits for the
 * recorded launches, writes their milliseconds and stream counts (4 / 5: a collocation set, 1: the value-only side sets) in launch
 * order and returns how many there were.  Either output may be NULL. */
int pinn_debug_profile_ring_arm(int max_launches);
/* ... of every `every`-th step only (a step = one collocation launch and the side-set launches behind it; default 1): the events of a
 * bracketed launch put barrier packets between back-to-back kernels, which slowed a fully bracketed block by 3.8 % (round 4); at a stride
 * of 8 the block is the timed loop again to 0.5 %.  Applies to the next _arm(). */
void pinn_debug_profile_ring_stride(int every);
int pinn_debug_profile_ring_read(float* ms_out, int* streams_out, int capacity);

const char* pinn_error_string(int code);
int pinn_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PINN_HIP_H */
