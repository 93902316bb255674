/*
 * rnf_hip.h -- C ABI of librnf_hip.so: the MI355X (gfx950) implementation of the SO(3) normalizing-flow density path
 * of PKU-EPIC/RotationNormFlow.  Plain pointers and sizes only; no framework types.  All `dev` pointers are HIP
 * device pointers, all other pointers are host pointers.  Every call is stream-ordered on `stream` (a hipStream_t
 * passed as void*; NULL = the default stream) and performs no host synchronisation.
 *
 * Return value: 0 on success, non-zero on error; rnf_last_error() returns a thread-local message.
 *
 * The reference has no FFI for this path (it is 100% Python); each entry point cites the reference code it replaces
 * (paths relative to the reference tree).  INTEGRATION.md shows the ctypes binding and the module-level drop-in.
 */
#ifndef RNF_HIP_H
#define RNF_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RNF_ABI_VERSION 8

/* width of the conditioner MLP's hidden layers: flow/condition.py:9 (Nh=64, never overridden by any caller) */
#define RNF_HIDDEN 64

/* ---- layer table -------------------------------------------------------------------------------------------
 * A flow is described by an int32 table desc[n_layers][RNF_DESC_STRIDE] (host memory) in Flow.layers order
 * (flow/flow.py:36-51) plus one float32 parameter blob (device memory) built with the rnf_pack_* functions.
 *   desc[i][0] kind          RNF_LAYER_*
 *   desc[i][1] perm_row      row of the 6x3 permutation table used by this layer on the FORWARD pass
 *                            (flow/flow.py:13-15,64-70); the inverse pass uses the same row for the same layer
 *   desc[i][2] param_offset  offset of the layer's packed parameters in the blob, in floats (multiple of 4)
 *   desc[i][3] cond_slot     index of this layer among the layers that consume the feature vector, or -1
 *   desc[i][4] feat_offset   offset in the blob of the layer's packed feature-projection weights, or -1
 *   desc[i][5] precision     bits 0..7: RNF_PREC_* the layer's weight image was packed with (same for every MLP layer); bits 8..15
 *                            (ABI v7): RNF_PREC_* of the FALLBACK records of columns 6, 7 -- RNF_PREC_FP32 (0) or RNF_PREC_BF16X3;
 *                            bits 16..17 (ABI v7, RNF_LAYER_MOBIUS): order of the FIRST pass of the inverse root finder that stands in
 *                            for BinFind (flow/mobiusflow.py:189-224) -- 0 the library's default (third order), 1 third order, 2 fourth
 *                            order (pays on sharply peaked conditioner outputs, i.e. trained conditional flows); one value per flow
 *                            (the largest code of its layers), the returned grid cell is the same for either
 *   desc[i][6] fallback param_offset   } RNF_PREC_F16X2 flows only: offsets in the SAME blob of the layer's records packed with a strict
 *   desc[i][7] fallback feat_offset    } arithmetic (or -1; the feature-projection record is the RNF_PREC_FP32 image for either).  When
 *                            every MLP layer has them, each rnf_flow_pass call without states is GUARDED: a sample that ends
 *                            non-finite (an fp16 operand left the fp16 range, |x| >= 65504;
 *                            flow/condition.py:24-30 has no such limit) sets a device flag and the strict kernels, launched right
 *                            behind on the same stream, redo the chunk -- they return at once when the flag is clear.  No host
 *                            synchronisation; int32 word 1 of the last 8 bytes of the first 32 KiB of the workspace is 1 after a call in
 *                            which the re-run happened.
 */
#define RNF_DESC_STRIDE 8
#define RNF_LAYER_MOBIUS 1        /* flow/mobiusflow.py:27-183  MobiusFlow                                  */
#define RNF_LAYER_AFFINE16 2      /* flow/squeezetrans.py:161-174 Uncondition16Trans (any constant 4x4 M)   */
#define RNF_LAYER_AFFINE16_COND 3 /* flow/squeezetrans.py:41-55  Condition16Trans (M = I + MLP(feature))    */
#define RNF_LAYER_GS9 4           /* flow/squeezetrans.py:250-261 Uncondition9Trans (Gram-Schmidt of M R)      */
#define RNF_LAYER_GS36 5          /* flow/squeezetrans.py:350-361 Uncondition36Trans (6x6 on two columns)      */
/* conditional 3x3 layers, M = I + reshape(MLP(feature), 3, 3) per sample (records from rnf_pack_cond9): */
#define RNF_LAYER_COND9_GS 6      /* flow/squeezetrans.py:234-247 Condition9Trans                              */
#define RNF_LAYER_COND9_SMITH 7   /* flow/rottrans.py:168-181     Condition9RotRSmith                          */
#define RNF_LAYER_COND9_POLAR_L 8 /* flow/rottrans.py:108-121     Condition9RotL                               */
#define RNF_LAYER_COND9_POLAR_R 9 /* flow/rottrans.py:138-151     Condition9RotR                               */
#define RNF_LAYER_COND36 10       /* flow/squeezetrans.py:334-347 Condition36Trans (record from rnf_pack_cond36) */
/* layers whose per-sample matrix the CALLER builds and hands in (RnfFlowPass.side; desc param_offset = slot in the side buffer, no blob
 * record): the reference forms these matrices with batched torch ops that are not a per-sample function -- ConditionRot's U^T V of a
 * batched SVD (flow/rottrans.py:37-66; depends on the SVD routine's sign conventions) and ConditionLU's torch.diag over the BATCH
 * dimension (flow/squeezetrans.py:121-131) -- so the host side reproduces them with the same torch calls on outputs of
 * rnf_cond_mlp_forward and the kernels apply the result: */
#define RNF_LAYER_SIDE16 11       /* flow/squeezetrans.py:134-144 Condition16TransLU: calculate_16 with the given 4x4 (log|det|) */
#define RNF_LAYER_SIDE16_ROT 12   /* flow/rottrans.py:37-66     ConditionRot: the given orthogonal 4x4 on the quaternion, log-det 0 */
#define RNF_LAYER_SIDE9 13        /* flow/squeezetrans.py:264-277 Condition9TransLU: calculate_9 with the given 3x3 (first 9 of 16 floats) */

/* ---- arithmetic of the conditioner GEMMs --------------------------------------------------------------------
 * RNF_PREC_FP32  : exact fp32 (v_mfma_f32_32x32x2_f32; bit-for-bit an fp32 fma chain).
 * RNF_PREC_F16X2 : every fp32 operand carried as two fp16 terms (hi + unscaled lo: 22 significant bits while |x| >= 2^-3, absolute
 *                  resolution 2^-25 below), three fp16 MFMAs into one fp32 accumulator per product-sum; ~2.8x faster than the fp32-input
 *                  MFMA, which shares the VALU's FMA datapath.  The absolute floor is kept 2^-22 below the signal of EVERY layer by the
 *                  packers: a ReLU network computes the same function under per-unit power-of-two rescalings of its hidden layers, and
 *                  rnf_pack_* / rnf_pack_flow_device first move the layer to the point of that orbit where every hidden pre-activation
 *                  has an estimated rms in (1/4, 1/2] (csrc/equalize.h; exact, power-of-two factors), THEN split.  The host packers
 *                  audit the packed image against the exact network on probe inputs (rnf_last_pack_audit) and return 2 -- pack
 *                  RNF_PREC_FP32 instead -- when it is off by more than 4e-6, or when a (scaled) weight leaves the fp16 range
 *                  (|x| < 65504).  Activations beyond the fp16 range at run time are caught by the range guard (see desc columns 6, 7).
 * RNF_PREC_BF16X3: (ABI v7) every fp32 operand -- weight and activation -- as THREE bf16 terms hi + mid + lo (truncated splits: 24
 *                  significant bits, fp32's exponent range), six bf16 MFMAs (every term down to 2^-16 of the leading one) into one fp32
 *                  accumulator per product-sum.  Nothing data- or scale-dependent: no equalisation, no audit, no feature calibration, no range
 *                  guard.  Records are larger (rnf_mobius_packed_floats_prec / rnf_cond_packed_floats_prec: a weight tile is 3072 floats
 *                  instead of 2048), the feature-projection record holds the RNF_PREC_FP32 image, and the kernels stage synchronously.
 *                  Built by the host packers and by rnf_pack_flow_device (same bits); rnf_cond_mlp_forward and rnf_conditioner_forward
 *                  run it too.  The 16-rotation training forward and the backward sweeps run exact fp32 whatever the records hold.
 */
#define RNF_PREC_FP32 0
#define RNF_PREC_F16X2 1
#define RNF_PREC_BF16X3 2

int rnf_abi_version(void);
const char *rnf_last_error(void);
/* largest relative error of the conditioner outputs the last rnf_pack_mobius / rnf_pack_cond* call of this thread measured on its probe
 * inputs (split precision only; 0 after an exact-fp32 pack) */
double rnf_last_pack_audit(void);
/* Process-wide measurement / test switches; both return the previous setting.  rnf_set_equalize(0): the packers split the weights as given
 * (also RNF_EQUALIZE=0 in the environment).  rnf_set_pack_audit(0): the host packers still measure, but no longer refuse. */
/* Mean square of a feature entry that the packers called from THIS thread assume when they equalise a conditional layer (default 1; the
 * one data-dependent input of csrc/equalize.h).  Returns the previous value. */
double rnf_set_feature_ms(double mean_square);
int rnf_set_equalize(int on);
int rnf_set_pack_audit(int on);
/* rnf_set_fused(1) (or RNF_FUSED=1): forward passes of conditional flows whose every MLP layer is conditional and feature_dim <= 256 run with
 * the feature projection INSIDE the stack kernel (no projection scratch in HBM).  Off by default: slower than the two-kernel path on C4. */
int rnf_set_fused(int on);
/* Block size of the training backward sweep: 16-rotation workgroups (csrc/train_block16.h) or 64-rotation ones (csrc/train_kernels.h, K <= 64
 * only); 0 (default) picks by batch size.  RNF_TRAIN_BLOCK=16|64 in the environment does the same.  Returns the previous setting. */
int rnf_set_train_block(int rotations);

/* ---- parameter packing (host side, pure CPU; called once per parameter version) ------------------------------
 * Sizes are in floats.  `segments` (K) is any positive count (flow/mobiusflow.py:7-14 takes any): records hold ceil(K / 8) fc_last tiles,
 * the last one zero padded, and the kernels give the pad segments weight 0.  An inverse pass keeps a layer's segment parameters in
 * registers (64 per lane; beyond K = 128 the rest streams through a per-wave stash in RnfFlowPass.workspace); the training entry
 * points take K <= 512 (the conditioner outputs of a 16-rotation block live in LDS).  `feature_dim` (F) is the number of
 * feature inputs of the layer's MLP (0 for an unconditional Moebius layer).
 */
int64_t rnf_mobius_packed_floats(int32_t segments);                       /* RNF_PREC_FP32 / RNF_PREC_F16X2 records */
int64_t rnf_mobius_packed_floats_prec(int32_t segments, int32_t precision);   /* any RNF_PREC_* */
int64_t rnf_cond_packed_floats_prec(int32_t n_out /* 16, 9 or 36 */, int32_t precision);
int64_t rnf_affine16_packed_floats(void);
int64_t rnf_cond16_packed_floats(void);
int64_t rnf_featproj_packed_floats(int32_t feature_dim); /* 0 when feature_dim == 0 */

/* MobiusFlow.conditioner = ConditionalTransform(3+F, 4K) (flow/mobiusflow.py:40-43, flow/condition.py:10-22).
 * Weights are torch.nn.Linear layout [out, in], row-major.  fc_first_w is [64, 3+F] with the 3 y-inputs FIRST
 * (flow/mobiusflow.py:53-56).  fc_last_w is [4K, 64]: rows [0,K) raw segment weights, row K+3k+d = w_k[d]
 * (flow/mobiusflow.py:58-61).  out_layer receives rnf_mobius_packed_floats(K) floats; out_feat receives
 * rnf_featproj_packed_floats(F) floats (ignored when F == 0). */
int rnf_pack_mobius(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                    const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                    const float *fc_last_w, const float *fc_last_b, int32_t segments, int32_t feature_dim,
                    int32_t precision, float *out_layer, float *out_feat);

/* Uncondition16Trans.mat [4,4] row-major (flow/squeezetrans.py:164-165).  Packs M, log|det M|, M^-1 and
 * log|det M^-1| (the reference recomputes inv/det every call: squeezetrans.py:38,171-174). */
int rnf_pack_affine16(const float *mat16, float *out_layer);

/* UnconditionRot (flow/rottrans.py:8-23): mat16 = U^T V of the SVD of the 4x4 parameter (an orthogonal matrix, computed by the
 * caller exactly as the reference does); the layer rotates the quaternion and contributes a log-det of exactly 0.  Same record
 * size and layer kind (RNF_LAYER_AFFINE16) as rnf_pack_affine16; the inverse pass uses the transpose (rottrans.py:26-28). */
int rnf_pack_rot16(const float *mat16, float *out_layer);

/* Uncondition9Trans (n = 3) / Uncondition36Trans (n = 6), flow/squeezetrans.py:250-261, 350-361 (and their LU
 * parameterisations, whose assembled matrix is passed here): layer kinds RNF_LAYER_GS9 / RNF_LAYER_GS36.
 * Record: M row-major, then M^-1 (used by the inverse pass, squeezetrans.py:259-261,359-361). */
int64_t rnf_gs_packed_floats(int32_t n);
int rnf_pack_gs(const float *mat, int32_t n, float *out);

/* Condition16Trans.net = ConditionalTransform(F, 16) (flow/squeezetrans.py:42-44). fc_first_w [64,F], fc_last_w [16,64]. */
int rnf_pack_cond16(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                    const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                    const float *fc_last_w, const float *fc_last_b, int32_t feature_dim, int32_t precision,
                    float *out_layer, float *out_feat);

/* Same record for the conditional 3x3 layers (RNF_LAYER_COND9_*): fc_last has 9 rows. */
int rnf_pack_cond9(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                    const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                    const float *fc_last_w, const float *fc_last_b, int32_t feature_dim, int32_t precision,
                    float *out_layer, float *out_feat);

/* Condition36Trans (RNF_LAYER_COND36): fc_last has 36 rows in two tiles; record length rnf_cond36_packed_floats(). */
int64_t rnf_cond36_packed_floats(void);
int rnf_pack_cond36(const float *fc_first_w, const float *fc_first_b, const float *l1_w, const float *l1_b,
                    const float *l3_w, const float *l3_b, const float *l5_w, const float *l5_b,
                    const float *fc_last_w, const float *fc_last_b, int32_t feature_dim, int32_t precision,
                    float *out_layer, float *out_feat);

/* ---- the flow -------------------------------------------------------------------------------------------------
 * One pass through a packed flow: Flow.forward (flow/flow.py:53-72; ldj = sum of forward log-det-Jacobians) or Flow.inverse
 * (flow/flow.py:74-92: walks the table backwards; ldj = sum of inverse-map log-dets, MobiusFlow.inverse returns -ldj:
 * flow/mobiusflow.py:183), optionally fused with the base density and the NLL sum, or saving the layer inputs for training.  Which of
 * these a call is follows from the fields that are set; combinations no caller uses (log p with dir 1, states with feature_div or log p,
 * side with feature_div) are refused.  Fields left zero / NULL are off.
 */
typedef struct RnfFlowPass {
    size_t struct_bytes;        /* sizeof(RnfFlowPass); any other value is refused (header and library differ) */
    int32_t dir;                /* 0 Flow.forward, 1 Flow.inverse */
    int32_t feature_dim;        /* F, a multiple of 8 (pad on the host) */
    const float *rotation;      /* dev [n,3,3] float32 row-major contiguous */
    const float *feature;       /* dev [n,F] row-major contiguous, or NULL for an unconditional flow */
    int64_t n;
    /* > 0: shared feature rows.  `feature` holds n / feature_div rows and row r conditions rotations [r * feature_div, (r + 1) *
     * feature_div) -- the pose-estimation pattern of Agent.eval_acc (agent.py:238-263) and the density of one image on a grid of
     * rotations (eval.py:444-462), where the reference materialises feature.repeat(number_queries).  The feature projection runs once per
     * row.  n must be a multiple of feature_div; an inverse pass takes at most 128 segments here. */
    int64_t feature_div;
    /* dev float[n_side_layers][n][16]: the per-sample matrices of the RNF_LAYER_SIDE* layers (row-major; 3x3 ones in the first 9 floats),
     * in side-slot order.  Required when the flow has such layers. */
    const float *side;
    const float *blob;          /* dev: the packed parameter blob */
    const int32_t *desc;        /* host: int32 [n_layers][RNF_DESC_STRIDE] */
    int32_t n_layers, segments;
    /* Fused density evaluation (dir 0): Flow.forward + MatrixFisherN(A)._log_prob(R') + the NLL accumulation (agent.py:54-65,217-229;
     * utils/fisher.py:217-232).  fisher_A dev [B,3,3], fisher_c dev [B] with c_b = sum(S_b) + log(norm_b) (the host precomputes the proper
     * singular values, utils/fisher.py:67-76,93-97); sample i uses row i / (n / B) (fisher.py:226).  Both NULL (and B = 0): a uniform
     * base; one without the other is refused. */
    const float *fisher_A, *fisher_c;
    int64_t fisher_B;
    float *rotation_out;        /* dev [n,3,3] or NULL.  == rotation (in place) is allowed -- every lane reads its rotation before it writes
                                 * it -- but such a call runs WITHOUT the range guard (the exact-fp32 re-run would start from the already
                                 * overwritten input): an fp16 overflow then shows as NaN outputs instead of being repaired.  No other
                                 * overlap between inputs and outputs is supported. */
    float *ldj_out;             /* dev [n] or NULL */
    float *logp_out;            /* dev [n] or NULL (dir 0): per-sample log p = ldj + base */
    double *sum_out;            /* dev double[2] or NULL (dir 0): {sum_i log p_i, n}, accumulated in fp64 in a fixed order
                                 * (deterministic); written also when n == 0 */
    /* dev float[n_layers][n][9] or NULL: a training pass, which also saves the rotation entering every ITERATION position (dir 0: every
     * layer; dir 1: position 0 = the last flow layer) for rnf_flow_backward_pass.  Needs rotation_out; runs unguarded. */
    float *states;
    /* dev scratch of at least rnf_flow_pass_workspace_bytes(this struct) bytes: the block partials, the guard word (int32 word 1 of the
     * last 8 bytes of the first 32 KiB is 1 after a call in which the exact-fp32 re-run happened, see desc columns 6, 7), the feature
     * projection of the conditional layers and the per-wave stash of an inverse pass with more than 128 segments. */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfFlowPass;
int rnf_flow_pass(const RnfFlowPass *pass);
/* The workspace rnf_flow_pass requires for the same struct (the workspace fields are not read); 0 when struct_bytes is wrong. */
size_t rnf_flow_pass_workspace_bytes(const RnfFlowPass *pass);
/* Partials block + the feature-projection scratch of n_cond_layers conditional layers (the workspace of rnf_cond_mlp_forward). */
size_t rnf_workspace_bytes(int64_t n, int32_t n_cond_layers);

/* ConditionRot (flow/rottrans.py:37-66): the per-sample orthogonal 4x4 matrices U^T V of svd(I + reshape(mlp_out, 4, 4)), with the sign
 * conventions of the reference's torch.svd (LAPACK's dense-SVD path restated for 4x4, csrc/svd4_lapack.h; identical for >= 99.8 % of
 * random matrices, the rest differ like two LAPACK builds do).  mlp_out_dev [n][16] from rnf_cond_mlp_forward, rot_out_dev [n][16] = one
 * slot of the side buffer of an RNF_LAYER_SIDE16_ROT layer.  Stream-ordered, no host synchronisation.
 * fail_flag_dev (int32, may be null): bit 0 is OR-ed in when a sample has no usable result: a NaN / inf entry in its matrix or a singular
 * value beyond FLT_MAX (rot and the factors of that sample are then NaN throughout), or a QR iteration that did not converge within
 * LAPACK's sweep limit (the slot then holds the factors of the last sweep).  With the flag clear every rot is orthogonal to rounding,
 * whatever the scale of the matrix (it is rescaled by a power of two when its largest entry leaves [2^-24, 2^24]).  The caller zeroes the
 * flag and reads it back when convenient; other samples of the launch are not affected.
 * rnf_condrot_svd also returns the factors -- u_out_dev [n][16] (U row-major), s_out_dev [n][4] (decreasing), vt_out_dev [n][16] (V^T
 * row-major) -- which is what the backward of U^T V needs (d rot = -wU rot + rot wV with wU, wV from U^T dM V; flow/rottrans.py here), so
 * that evaluation AND training see the same routine's sign choices (ABI v6; v5 trained through the host's torch.svd). */
int rnf_condrot_matrices(const float *mlp_out_dev, int64_t n, float *rot_out_dev, int32_t *fail_flag_dev, void *stream);
int rnf_condrot_svd(const float *mlp_out_dev, int64_t n, float *rot_out_dev, float *u_out_dev, float *s_out_dev, float *vt_out_dev,
                    int32_t *fail_flag_dev, void *stream);

/* ConditionLU's per-sample matrices on the device (replaces flow/squeezetrans.py:120-131, the `einsum` over `torch.diag` -- ABI v7; until v6
 * the host library assembled them with torch ops):
 *     weight[n] = w_p (reshape(wl[n], C, C) * l_mask + l_eye) (reshape(wu[n], C, C) * u_mask + dvec),  dvec[d] = s_sign[d] exp(ws[d][d])
 * where `torch.diag` of the 2-D tensor s_sign * exp(ws) is its diagonal ACROSS THE BATCH (rows 0..C-1) and the C-vector is broadcast over
 * the last axis -- added to every row of the upper factor.  Reproduced as the reference defines it: the matrix of sample n depends on the
 * first C rows of the batch.  n = 1 follows the reference as well (torch.diag of a [1, C] tensor is the one-entry vector
 * s_sign[0] exp(ws[0][0]), broadcast to every column; its gradient lands in g_ws[0][0]); 1 < n < C is an error (the reference fails
 * to broadcast).
 * wl_dev, wu_dev, ws_dev: the three conditioners' outputs (rnf_cond_mlp_forward), rows of stride_wl / stride_wu (>= C*C) and stride_ws
 * (>= C) floats; C = 3 or 4; consts_dev = w_p [C*C] | l_mask [C*C] | u_mask [C*C] | l_eye [C*C] | s_sign [C] (the module's buffers);
 * add_identity != 0: + I (Condition9TransLU, squeezetrans.py:269-271); side_out_dev [n][16]: one slot of the side buffer of an
 * RNF_LAYER_SIDE16 / RNF_LAYER_SIDE9 layer (C x C row-major in the leading floats, the rest 0).
 * rnf_condlu_backward: g_side_dev [n][16] = dL/d(weight) -> g_wl_dev [n][C*C], g_wu_dev [n][C*C], g_ws_dev [n][C] (dense rows); the
 * batch-coupled diagonal's gradient lands in g_ws[d][d] only (every other entry 0).  scratch_dev: 4 floats. */
int rnf_condlu_matrices(const float *wl_dev, const float *wu_dev, const float *ws_dev, int32_t stride_wl, int32_t stride_wu, int32_t stride_ws,
                        int64_t n, int32_t C, const float *consts_dev, int32_t add_identity, float *side_out_dev, void *stream);
int rnf_condlu_backward(const float *wl_dev, const float *wu_dev, const float *ws_dev, int32_t stride_wl, int32_t stride_wu, int32_t stride_ws,
                        int64_t n, int32_t C, const float *consts_dev, const float *g_side_dev, float *g_wl_dev, float *g_wu_dev,
                        float *g_ws_dev, float *scratch_dev, void *stream);

/* ConditionalTransform(feature_dim, <= 16 outputs)(feature) alone (flow/condition.py:24-30): records packed by rnf_pack_cond16 at
 * layer_offset / feat_offset (floats) of blob_dev; out_dev float[n][16], output o in column o.  Workspace: rnf_workspace_bytes(n, 1).
 * RNF_PREC_BF16X3 projects the feature in exact fp32, as the flow pass does. */
int rnf_cond_mlp_forward(const float *feature_dev, int64_t n, int32_t feature_dim, const float *blob_dev, int32_t layer_offset,
                         int32_t feat_offset, int32_t precision, float *out_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- training (agent.py:75-92: loss = mean(-ldj), loss.backward(), Adam step) ----------------------------------------
 *
 * The backward pass works on the "plain" parameter blob: per layer, in reference state-dict order,
 *   Moebius / Condition16Trans conditioner (flow/condition.py): fc_first.weight [64][NI] | fc_first.bias | hidden[0] W,b |
 *       hidden[2] W,b | hidden[4] W,b | fc_last.weight [NO][64] | fc_last.bias  with NI = 3 + F, NO = 4 * segments
 *       (Moebius) or NI = F, NO = 16 (Condition16Trans);
 *   Uncondition16Trans (flow/squeezetrans.py:57-66): mat [16].
 * rnf_plain_layer_floats gives each layer's length; the gradient blob has the same layout.
 * train_desc: int32 [n_layers][3] = kind (| RNF_TRAIN_ORTHOGONAL for UnconditionRot, whose matrix is orthogonal and whose
 *             ldj is 0, flow/rottrans.py:14-23), perm_row, offset (floats) of the layer in the plain blob, in flow order.
 */
#define RNF_TRAIN_ORTHOGONAL 256
size_t rnf_plain_layer_floats(int32_t kind, int32_t segments, int32_t feature_dim);

/* Build the kernel blob on the device from the plain blob (same bits as rnf_pack_* on the host; the parameters change every
 * training iteration).  pack_desc: int32 [n_layers][4] = kind (| RNF_TRAIN_ORTHOGONAL), offset in the plain blob, offset of
 * the layer record in the kernel blob, offset of its feature-projection record (or -1), all in floats; record offsets are
 * multiples of 4.  feature_dim is the real (unpadded) width; records are laid out for it padded to a multiple of 8.
 * flags_dev: device int32, zeroed by the caller; bit 0 = a weight outside the fp16 range under RNF_PREC_F16X2 (the blob
 * then holds inf/NaN), bit 1 = a singular 4x4 matrix.  All three precisions; RNF_PREC_F16X2 alone is equalised (RNF_PREC_BF16X3
 * records are sized by rnf_mobius_packed_floats_prec / rnf_cond_packed_floats_prec, their projection records hold the fp32 image). */
int rnf_pack_flow_device(const float *plain_dev, const int32_t *pack_desc, int32_t n_layers, int32_t segments,
                         int32_t feature_dim, int32_t precision, float *blob_dev, int32_t *flags_dev, void *stream);

/* Training forward for small batches, from the PLAIN parameter blob (the layout rnf_flow_backward_pass reads: no packing step) on
 * 16-rotation workgroups in exact fp32 (csrc/train_block16.h) -- the arithmetic of the backward sweep's own forward recompute.  Replaces
 * Flow.forward inside the training step (agent.py:75-92) for flows made of Moebius, Uncondition16Trans / UnconditionRot and
 * Condition16Trans layers, n_layers <= 200, segments <= 512; other flows are refused (use rnf_flow_pass with states).  train_desc: the
 * table of rnf_flow_backward_pass; feature_dev [n][feature_dim], unpadded; states_dev float[n_layers][n][9]. */
int rnf_flow_forward_train_plain(const float *rotation_dev, const float *feature_dev, int64_t n, int32_t feature_dim,
                                 const float *plain_dev, const int32_t *train_desc, int32_t n_layers, int32_t segments,
                                 float *rotation_out_dev, float *ldj_out_dev, float *states_dev, float *acts_dev, void *stream);
/* acts_dev (may be NULL): rnf_train_acts_floats(n, conditioner layers, segments) floats in which the forward leaves every conditioner's
 * activations (2 KB per rotation and layer at 64 segments), for RnfFlowBackward.acts. */
size_t rnf_train_acts_floats(int64_t n, int32_t n_conditioner_layers, int32_t segments);

/* Reverse sweep of a training pass (RnfFlowPass with states): what autograd does for the reference, agent.py:79-80.  dir 1 gives the
 * gradients THROUGH Flow.inverse (flow/flow.py:74-92; MobiusFlow.inverse with BinFind.backward's implicit-function gradient of the root,
 * flow/mobiusflow.py:247-273; the affine layers apply M^-1, flow/squeezetrans.py:51-55,171-174).  Any segment count 1..512 (the
 * conditioner outputs of a 16-rotation block live in LDS), n_layers <= 400 like the forward passes (beyond 200 the sweep runs in chunks of
 * 200 layers).  Fields left zero / NULL are off. */
typedef struct RnfFlowBackward {
    size_t struct_bytes;        /* sizeof(RnfFlowBackward); any other value is refused (header and library differ) */
    int32_t dir;                /* direction of the training pass: 0 Flow.forward, 1 Flow.inverse */
    int32_t feature_dim;        /* F (unpadded) */
    const float *states;        /* dev float[n_layers][n][9]: what the training pass saved */
    /* dir 1: dev [n][9], the output of the inverse pass (each Moebius layer reads its root back from its own output, no second root
     * search); required there, unused for dir 0 */
    const float *rotation_out;
    const float *feature;       /* dev [n][F] or NULL */
    int64_t n;
    /* dev: the plain blob (see "training" above); may be NULL when `side` is set and no layer has plain parameters */
    const float *plain;
    /* host int32 [n_layers][3] in the order the pass visited the layers (dir 1: reversed).  A side layer's slot goes into bits 16..23 of
     * its kind word, its plain offset is unused (rnf_plain_layer_floats = 0). */
    const int32_t *train_desc;
    int32_t n_layers, segments;
    /* dev or NULL (dir 0): the activations rnf_flow_forward_train_plain left for the same n, table and K -- every layer must be a kind it
     * runs.  The 16-rotation sweep reads them back instead of recomputing each conditioner; the 64-rotation sweep of large batches
     * ignores them. */
    const float *acts;
    /* Side layers (RNF_LAYER_SIDE16 / SIDE16_ROT / SIDE9: Condition16TransLU, ConditionRot, Condition9TransLU; flow/squeezetrans.py:
     * 134-144,264-277, flow/rottrans.py:37-66): the caller builds their per-sample matrices with the reference's own tensor ops (the LU
     * layers' torch.diag couples the batch; ConditionRot's U^T V follows torch.svd's conventions), so the gradient chain is split.  side:
     * the RnfFlowPass.side buffer of the pass; side_grad: dev float[n_side][n][16] out, dL/d(matrix) (same layout) for the caller's
     * autograd to carry through those ops into the conditioner networks (rnf_cond_mlp_backward).  Both required when the flow has such
     * layers. */
    const float *side;
    float *side_grad;
    const float *g_rotation_out;    /* dev [n][9] or NULL (= zeros) */
    const float *g_ldj;             /* dev [n] */
    /* dev, plain layout, ACCUMULATED into: zero it first; NULL = skip every parameter gradient, for callers that only differentiate
     * w.r.t. the inputs: pose refinement, eval.py:464-478 */
    float *grads;
    /* dev [n][9] out: the gradient w.r.t. the rotations GIVEN to the pass.  Beyond 200 layers it also carries the gradient between the
     * chunks and may alias g_rotation_out. */
    float *g_rotation_in;
    float *g_feature;               /* dev [n][F], ACCUMULATED into, or NULL */
    float *layer_scratch;           /* dev float[n_layers], zeroed by the caller (batch sums of dL/dldj for the d log|det M| / dM term) */
    void *stream;
} RnfFlowBackward;
int rnf_flow_backward_pass(const RnfFlowBackward *pass);

/* Backward of ONE conditioner network evaluated by rnf_cond_mlp_forward.  plain_dev: the network's parameters in reference order
 * (fc_first.weight [64][F], .bias, layers.{1,3,5}.weight / .bias, fc_last.weight [n_out][64], .bias; flow/condition.py:14-22); g_out_dev
 * float[n][n_out]; grads_dev (same layout as plain_dev) and g_feature_dev [n][F] are ACCUMULATED into and may be NULL; scratch1_dev: one
 * zeroed float.  n_out <= 64. */
int rnf_cond_mlp_backward(const float *feature_dev, int64_t n, int32_t feature_dim, const float *plain_dev, int32_t n_out,
                          const float *g_out_dev, float *grads_dev, float *g_feature_dev, float *scratch1_dev, void *stream);

/* MatrixFisherN._log_prob alone (utils/fisher.py:217-232), same A/c convention; out [n]. */
int rnf_fisher_log_prob(const float *rotation_dev, int64_t n, const float *fisher_A_dev, const float *fisher_c_dev,
                        int64_t fisher_B, float *out_dev, void *stream);

/* Pose-accuracy epilogue of Agent.eval_acc (agent.py:266-283; utils/utils.py:231-235 min_geodesic_distance_rotmats): angle (radians)
 * between estimate i and the closest of its k ground-truth rotations.  est_dev float[n][9], gt_dev float[n][k][9], out_dev float[n]. */
int rnf_min_geodesic(const float *est_dev, const float *gt_dev, int64_t n, int32_t k, float *out_dev, void *stream);

/* Equivolumetric HEALPix grid over SO(3) for grid-search pose estimation, generated on the device already offset (replaces the host build of
 * utils/sd.py:47-82 generate_healpix_grid -- healpy's pix2vec in the RING ordering, scipy's from_euler, numpy's einsum -- and eval.py:440-442's
 * per-batch `samples = grid @ random_rot`).  out_dev float[72 * 8^level][3][3], row t * npix + p = Rx(phi_p) Rz(theta_p) Rx(tau_t) O with
 * nside = 2^level, npix = 12 nside^2, (theta_p, phi_p) the centre of pixel p, tau_t = 2 pi t / (6 nside), O = offset9_dev (row-major device
 * float[9]) or the identity when NULL.  fp64 inside, one rounding to fp32 per entry.  level 0..8 (level 8: 1.2e9 rows, 43 GB). */
int rnf_so3_healpix_grid(int32_t level, const float *offset9_dev, float *out_dev, void *stream);

/* The grid's hierarchy, for the coarse-to-fine beam search.  The children of level-l row r = t * npix + p (nside = 2^l) are the 12
 * level-(l + 1) rows with pixel ring(4 nest(p) + c), c = 0..3 (ring2nest / nest2ring of Gorski et al. 2005 at nside and 2 nside: the four
 * NESTED sub-pixels) and tilt 2t - 1, 2t, 2t + 1 modulo 6 * 2^(l + 1); child j = 4 k + c has tilt 2t - 1 + k.  The children of all level-l
 * rows cover every level-(l + 1) row (the odd tilts are shared by neighbouring parents, so some rows are children of several).
 * rows_out[q][j] = child j of parents[q] as a level-(l + 1) row (-1 for a parent outside 0..72 * 8^l - 1, e.g. the -1 padding of
 * rnf_grid_beam_select); rot_out[q][j] (optional) = its rotation, bit-identical to the row rnf_so3_healpix_grid(l + 1, offset) writes
 * (one shared row function; the rotation of row 0 for a child -1). */
typedef struct RnfGridChildren {
    size_t struct_bytes;        /* sizeof(RnfGridChildren); any other value is refused */
    int32_t level;              /* the parents' level l, 0..7 */
    const int64_t *parents;     /* dev int64[n]: g images * m parent rows each */
    int64_t n;                  /* 0..2^36 */
    const float *offset;        /* dev float[9] row-major, or NULL (identity) */
    int64_t *rows_out;          /* dev int64[n][12] */
    float *rot_out;             /* dev float[n][12][9], or NULL */
    void *stream;
} RnfGridChildren;
int rnf_so3_grid_children(const RnfGridChildren *children);

/* Beam selection per image: of its M candidates (log p, row), the `beam` best DISTINCT rows, ordered by log p descending (a NaN first, as
 * torch.argmax; -0 and +0 tie) and then row ascending; a row duplicated among the candidates counts once, with its best candidate.  Past
 * the distinct rows: row -1, log p -inf.  logp_out holds the candidate's value (a NaN as the canonical quiet NaN, -0 as +0).  A candidate
 * whose row is < 0 or > 2^31 - 2 is ignored.  Deterministic: no atomics, passes and block counts depend on (M, beam) alone, so results
 * are bit-identical from run to run and whatever g. */
typedef struct RnfGridBeamSelect {
    size_t struct_bytes;        /* sizeof(RnfGridBeamSelect); any other value is refused */
    const float *logp;          /* dev float[g][M] */
    const int64_t *rows;        /* dev int64[g][M] the candidates' rows, or NULL: candidate i is row i (distinct, no deduplication) */
    int64_t M;                  /* candidates per image, 1..2^31 - 1 */
    int32_t g;                  /* images, 1..65535 */
    int32_t beam;               /* 1..1024 */
    int64_t *rows_out;          /* dev int64[g][beam] */
    float *logp_out;            /* dev float[g][beam] */
    /* dev scratch of at least rnf_grid_beam_select_workspace_bytes(this struct) bytes = 2 g ceil(M / 4096) beam 8 (8 when M <= 4096) */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfGridBeamSelect;
int rnf_grid_beam_select(const RnfGridBeamSelect *select);
/* The workspace rnf_grid_beam_select requires for the same struct (the workspace fields are not read); 0 when struct_bytes, g, M or beam
 * are out of range. */
size_t rnf_grid_beam_select_workspace_bytes(const RnfGridBeamSelect *select);

/* Top-k pose modes of g images evaluated on one grid of the search above, with the probability mass each carries: the commented-out
 * `for top_k in [1, 2, 4]` of eval.py:243,297,406 and the spread of IPDF (Murphy et al. 2021, the expected angular error under the
 * predicted distribution).  Every grid cell has the same Haar volume and the flow densities are relative to the normalised Haar measure,
 * so exp(lp_i) / Q is cell i's mass.  Per image, with thr = 1 + 2 cos(separation_rad) (a row is "within sep" of mode m when
 * tr(M_m^T R_i) > thr; at separation_rad = pi every row is within sep of mode 0):
 *   mode 0      the first arg-max of the image's log p, a NaN winning (torch.argmax);
 *   mode j > 0  the first arg-max over the rows within sep of no earlier mode; index -1, log p -inf, mass 0 when there is none (and for
 *               every later mode);
 *   log_norm    log(sum_i exp(lp_i) / Q): the maximum M first, exp(lp_i - M) in fp32, sums in fp64;
 *   mass_j      sum exp(lp_i - M) / sum_i exp(lp_i - M) over mode j's region: the rows within sep of mode j and of no earlier mode
 *               (the masses add up to at most 1);
 *   spread      sum_i p_i min_g acos(clip((tr(G_g^T R_i) - 1) / 2, -1, 1)) in radians against the image's ground truths, p the masses.
 * A NaN in the image's log p: mode 0 as torch.argmax, modes > 0 index -1, log_norm, every mass and spread NaN.  A row without a finite
 * value has log_norm -inf and NaN masses of its modes.  Deterministic: bit-identical from run to run and whatever g (no atomics). */
typedef struct RnfGridModes {
    size_t struct_bytes;        /* sizeof(RnfGridModes); any other value is refused (header and library differ) */
    const float *logp;          /* dev float[g][Q]: image b's log p on grid row i */
    const float *grid;          /* dev float[Q][9], 16-byte aligned: the (offset) grid the log p were evaluated on */
    int64_t Q;                  /* >= 1 */
    int32_t g;                  /* images, 1..65535 */
    int32_t top_k;              /* k, 1..16 */
    double separation_rad;      /* 0 < sep <= pi */
    const float *gt;            /* dev float[g][n_gt][9] ground truths, or NULL (no spread) */
    int32_t n_gt;               /* 1..128 with gt */
    int64_t *index_out;         /* dev int64[g][k] */
    float *logp_out;            /* dev float[g][k] */
    float *mass_out;            /* dev float[g][k] */
    float *log_norm_out;        /* dev float[g] */
    float *spread_out;          /* dev float[g]; required with gt, ignored without */
    /* dev scratch of at least rnf_grid_modes_workspace_bytes(this struct) bytes = g * min(ceil(Q / 2048), 2048) * 8 * (top_k + 2): the
     * per-block partials of one pass (their count depends on Q alone) */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfGridModes;
int rnf_grid_modes(const RnfGridModes *modes);
/* The workspace rnf_grid_modes requires for the same struct (the workspace fields are not read); 0 when struct_bytes, g, Q or top_k are
 * out of range. */
size_t rnf_grid_modes_workspace_bytes(const RnfGridModes *modes);

/* Highest-density credible sets of g images' densities on one grid, and the HPD level of query log-densities (csrc/grid_credible.h).
 * Per image, with m the maximum of its log p (the first arg-max, a NaN winning), w_i = expf(lp_i - m) (the fp32 exponential of
 * rnf_grid_modes), the fixed-point mass W_i = rint(w_i 2^S) as an unsigned 64-bit integer and T = sum_i W_i:
 *   threshold_j    the largest value tau among the image's log p with sum_{lp_i >= tau} W_i >= ceil(alpha_j T): the set is {lp_i >= tau},
 *                  so ties with tau are all inside; -0 and +0 tie, and a zero threshold is reported as +0;
 *   count_j        the number of cells with lp_i >= threshold_j (count_j / Q is the set's volume as a fraction of SO(3));
 *   mass_j         sum_{lp_i >= tau} W_i / T;
 *   query_mass_q   sum_{lp_i > v_q} W_i / T, a strict inequality: the HPD level of a point whose log-density is v_q (0 at the mode);
 *   query_count_q  the number of cells with lp_i > v_q;
 *   log_norm       m + log(T / 2^S) - log Q, rnf_grid_modes' log_norm to 1e-6.
 * Fixed point: S = 62 - ceil(log2 Q).  w_i <= 1, so W_i <= 2^S and T <= Q 2^S <= 2^62: no sum can overflow, and integer sums do not
 * depend on the order they are taken in -- the select's histograms are exact.  Each W_i is off by at most 1/2 and T >= 2^S (the maximum's
 * own cell), so every reported mass fraction is within eps_fix(Q) = Q 2^-(S + 1) of the one with real-valued w_i: 1.1e-6 at level 5
 * (Q = 72 8^5, S = 40), 6.9e-5 at level 6 (S = 37); Q is limited to 2^26 (level 6).
 * A NaN in the image's log p, or a maximum of +inf: every threshold, mass and query mass is NaN, every count -1, log_norm NaN.  No finite
 * value in the image: log_norm -inf, thresholds and masses NaN, counts -1.  -inf cells elsewhere weigh 0 and are never inside a set.  A NaN
 * query has mass NaN and count -1.  Deterministic: bit-identical from run to run and whatever g.  Stream-ordered, no host
 * synchronisation, capturable in a HIP graph. */
typedef struct RnfGridCredible {
    size_t struct_bytes;        /* sizeof(RnfGridCredible); any other value is refused (header and library differ) */
    const float *logp;          /* dev float[g][Q]: image b's log p on grid row i */
    int64_t Q;                  /* 1..2^26 */
    int32_t g;                  /* images, 1..65535 */
    const double *levels;       /* HOST double[n_levels]: 0 < alpha_j < 1 (read during the call) */
    int32_t n_levels;           /* J, 1..8 */
    const float *queries;       /* dev float[g][n_queries] log-densities, or NULL with n_queries = 0 */
    int32_t n_queries;          /* G, 0..16 */
    float *threshold_out;       /* dev float[g][J] */
    int64_t *count_out;         /* dev int64[g][J] */
    float *mass_out;            /* dev float[g][J] */
    float *log_norm_out;        /* dev float[g] */
    float *query_mass_out;      /* dev float[g][G]; required with n_queries > 0 */
    int64_t *query_count_out;   /* dev int64[g][G]; required with n_queries > 0 */
    /* dev scratch, 8-byte aligned, of at least rnf_grid_credible_workspace_bytes(this struct) bytes: with nb = min(ceil(Q / 8192), 512)
     * blocks per image (a function of Q alone), g * (16 min(ceil(Q / 2048), 2048) + 20 + 128 J + nb (3072 J + 12 G)) rounded up to 16:
     * the maximum's partials, the select's state and one pass's per-block histograms */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfGridCredible;
int rnf_grid_credible(const RnfGridCredible *credible);
/* The workspace rnf_grid_credible requires for the same struct (the pointers are not read); 0 when struct_bytes, g, Q, n_levels or
 * n_queries are out of range. */
size_t rnf_grid_credible_workspace_bytes(const RnfGridCredible *credible);

/* The grid cell of rotations: the inverse of the row function of rnf_so3_healpix_grid (csrc/grid_locate.h).  With R' = R O^T (O the
 * offset, the identity when NULL) written as Rx(phi) Rz(theta) Rx(tau):
 *   z = R'00 clipped to [-1, 1], sin(theta) = hypot(R'10, R'20), phi = atan2(R'20, R'10), tau = atan2(R'02, -R'01);
 *   p = ang2pix in the RING ordering at nside = 2^level (Gorski et al. 2005), in the polar caps (|z| > 2/3) with sin(theta) and not
 *       sqrt(1 - z^2): tmp = nside sin(theta) / sqrt((1 + |z|) / 3);
 *   t = rint(tau / (2 pi / (6 nside))) mod 6 nside, so that a cell is centred on its grid tilt;  row = t * npix + p.
 * At a pole, R'10 = R'20 = 0 exactly: phi = 0 and tau = atan2(R'21, R'11) for z > 0, atan2(R'21, R'22) for z < 0.
 * fp64 inside from the fp32 entries, one thread per rotation.  A rotation with a non-finite entry has row -1.  Every row of the level's
 * grid (with the same offset) is located in its own cell.
 * What a cell is: the rotations that this function maps to the row.  The 72 * 8^level cells partition SO(3) into parts of equal Haar
 * volume, which is what makes a histogram over them comparable with exp(lp_i) / Q.  What it is not: the Voronoi cell of the grid
 * rotation; at level 1 about 73 % of Haar-uniform rotations lie in the cell whose grid rotation is also their geodesically nearest one.
 * rows_out and counts are both optional, at least one is required.  With counts, counts[b][row] is incremented by an integer atomic
 * for every rotation of image b whose row is not -1: integer sums do not depend on their order, so the counts are bit-identical from run
 * to run.  counts is accumulated into and never cleared: clear it before the first call, then stream a sample set through any number
 * of calls (a cell's count must stay below 2^31).  n = 0 is a no-op.  Stream-ordered, no host synchronisation, capturable. */
typedef struct RnfGridLocate {
    size_t struct_bytes;        /* sizeof(RnfGridLocate); any other value is refused (header and library differ) */
    int32_t level;              /* 0..8; with counts 0..6: Q = 72 * 8^level <= 2^26 */
    const float *rotations;     /* dev float[g][n][9] row-major */
    int64_t n;                  /* rotations per image, 0..2^36 */
    int32_t g;                  /* images, 1..65535 */
    const float *offset;        /* dev float[9] row-major, or NULL (identity): the offset the grid was generated with */
    int64_t *rows_out;          /* dev int64[g][n], or NULL */
    int32_t *counts;            /* dev int32[g][Q], or NULL */
    void *stream;
} RnfGridLocate;
int rnf_so3_grid_locate(const RnfGridLocate *locate);

/* How well g histograms over the grid's cells (rnf_so3_grid_locate) fit g densities on the grid (csrc/grid_locate.h).  Per image, with
 * c_i >= 0 the count of cell i (a negative count is read as 0), n = sum c_i, M the maximum of its log p (the first arg-max, a NaN
 * winning), w_i = expf(lp_i - M) (the fp32 exponential of rnf_grid_modes), Z = sum w_i and p_i = w_i / Z -- the density at the cell's
 * grid rotation, normalised over the grid: a midpoint value, not the cell's exact mass --
 *   stats[b][RNF_GRID_FIT_LOG_NORM]             M + log Z - log Q, rnf_grid_modes' log_norm to 1e-6;
 *   stats[b][RNF_GRID_FIT_LOG_LIKELIHOOD]       (1/n) sum c_i lp_i: the mean log p at the grid rotations of the samples' cells;
 *   stats[b][RNF_GRID_FIT_GRID_LOG_LIKELIHOOD]  log_likelihood - log_norm: the mean of log(p_i Q), IPDF's grid-normalised metric;
 *   stats[b][RNF_GRID_FIT_G]                    2 sum_{c_i > 0} c_i (log(c_i / n) - log p_i): the likelihood-ratio statistic, 2 n KL;
 *   stats[b][RNF_GRID_FIT_CHI2]                 sum (c_i - n p_i)^2 / (n p_i): Pearson's statistic;
 *   stats[b][RNF_GRID_FIT_N]                    n;   stats[b][RNF_GRID_FIT_OCCUPIED]  the number of cells with c_i > 0 (both exact).
 * After M, one pass: Z, S1 = sum c_i log c_i, S2 = sum c_i (lp_i - M), S3 = sum c_i^2 / w_i over the occupied cells, all in fp64, n and
 * the occupied cells as integers; g_stat = 2 (S1 - S2 + n log Z - n log n), chi2 = Z S3 / n - n.
 * Edge cases: a -inf cell with c_i = 0 contributes nothing.  An occupied cell with w_i = 0 -- lp_i = -inf, or expf underflowed, about
 * 104 below M -- makes log_likelihood -inf and g_stat = chi2 = +inf (grid_log_likelihood -inf, NaN when the row has no finite value).
 * A NaN in the image's log p, or a maximum of +inf: the five statistics are NaN, n and occupied are still counted.  n = 0: log_norm as
 * otherwise, the other four NaN.  A row without a finite value has log_norm -inf.
 * Deterministic: blocks per image depend on Q alone, fixed per-thread order, fixed shuffle trees, the finalise sums the block partials
 * in index order, no floating-point atomics -- bit-identical from run to run and whatever g.  Stream-ordered, no host synchronisation,
 * capturable in a HIP graph. */
#define RNF_GRID_FIT_LOG_NORM 0
#define RNF_GRID_FIT_LOG_LIKELIHOOD 1
#define RNF_GRID_FIT_GRID_LOG_LIKELIHOOD 2
#define RNF_GRID_FIT_G 3
#define RNF_GRID_FIT_CHI2 4
#define RNF_GRID_FIT_N 5
#define RNF_GRID_FIT_OCCUPIED 6
#define RNF_GRID_FIT_STATS 7
typedef struct RnfGridFit {
    size_t struct_bytes;        /* sizeof(RnfGridFit); any other value is refused (header and library differ) */
    const float *logp;          /* dev float[g][Q]: image b's log p on grid row i */
    const int32_t *counts;      /* dev int32[g][Q]: image b's samples in cell i */
    int64_t Q;                  /* 1..2^26 */
    int32_t g;                  /* images, 1..65535 */
    double *stats_out;          /* dev double[g][RNF_GRID_FIT_STATS] */
    /* dev scratch, 8-byte aligned, of at least rnf_grid_fit_workspace_bytes(this struct) bytes =
     * g * (16 min(ceil(Q / 2048), 2048) + 48 min(ceil(Q / 8192), 512) + 12) rounded up to 16: the maximum's and the pass's block partials */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfGridFit;
int rnf_grid_fit(const RnfGridFit *fit);
/* The workspace rnf_grid_fit requires for the same struct (the pointers are not read); 0 when struct_bytes, g or Q are out of range. */
size_t rnf_grid_fit_workspace_bytes(const RnfGridFit *fit);

/* The chart of a grid cell (csrc/grid_sample.h): point k is the rotation at (u0, u1, u2) in [0, 1]^3 of the cell of row rows[k] of the
 * level's grid (the cells of rnf_so3_grid_locate).  Row r = t * npix + p: ring2nest(p) gives (face, ix, iy) at nside = 2^level;
 *   x = (ix + u0) / nside, y = (iy + u1) / nside, jr = jrll(face) - x - y;
 *   jr < 1 (north cap): nr = jr, z = 1 - nr^2 / 3;  jr > 3 (south cap): nr = 4 - jr, z = nr^2 / 3 - 1;  else nr = 1, z = (2 - jr) 2 / 3;
 *   phi = (pi / 4) ((jpll(face) nr + x - y) mod 8) / nr;  tau = (t + u2 - 1/2) 2 pi / (6 nside);  rot = Rx(phi) Rz(theta) Rx(tau) O
 * (HEALPix's continuous face-to-sphere map, Gorski et al. 2005; sin(theta) = sqrt(tmp (2 - tmp)), tmp = nr^2 / 3, in the caps).  That map
 * is equal-area and the tilt is linear, so uniform u are Haar-uniform in the cell; u = (1/2, 1/2, 1/2) is the grid's own row to rounding.
 * fp64 inside, one rounding per entry at the store, one thread per point.  A row outside 0..72 * 8^level - 1 or a u outside [0, 1] (NaN
 * included) gives nine NaNs and no access.  A point on a cell's boundary (u = 0 or 1, or within rounding of it) may locate to the
 * neighbouring cell.  n = 0 is a no-op.  Stream-ordered, no host synchronisation, capturable. */
typedef struct RnfGridCellPoints {
    size_t struct_bytes;        /* sizeof(RnfGridCellPoints); any other value is refused (header and library differ) */
    int32_t level;              /* 0..6 */
    const float *offset;        /* dev float[9] row-major, or NULL (identity) */
    const int64_t *rows;        /* dev int64[n] */
    const float *u;             /* dev float[n][3] */
    int64_t n;                  /* points, 0..2^36 */
    float *rot_out;             /* dev float[n][9] row-major */
    void *stream;
} RnfGridCellPoints;
int rnf_so3_grid_cell_points(const RnfGridCellPoints *points);

/* Draws from g posteriors on grid rows (csrc/grid_sample.h).  Image b's masses are rnf_grid_credible's: W_i = rint(expf(lp_i - m) 2^S),
 * m the image's maximum, S = 62 - ceil(log2 Q); C is their inclusive prefix sum in row order and T = C_{Q-1} <= 2^62.  A target v in
 * [0, T) draws the row i with C_{i-1} <= v < C_i, so a row with W_i = 0 (lp_i = -inf, or more than (63 - ceil(log2 Q)) ln 2 below m: 26.3 at level 6) is never
 * drawn.  r64(k, b, s) = (word0 << 32) | word1 of Philox4x32-10 with key (seed low, seed high) on the counter (k, b low, b high, s),
 * k = draw_base + the draw's index in the call, b = image_base + the image's index in the call; mulhi = the high 64 bits of a product:
 *   RNF_GRID_SAMPLE_MULTINOMIAL  v_k = mulhi(r64(k, b, 0), T): independent draws;
 *   RNF_GRID_SAMPLE_SYSTEMATIC   a = mulhi(r64(0, b, 0), T), N = draws_total, T = q N + r: v_k = k q + (k r + a) / N (integer division)
 *                                = floor((k T + a) / N): one offset, N evenly spaced targets, |count_i - N p_i| < 1, ascending in k.
 * rot_out (needs level >= 0, Q = 72 * 8^level): with jitter the drawn row goes through rnf_so3_grid_cell_points' chart at
 * u_j = (word_j of the counter (k, b, 1) + 1/2) / 2^32, j = 0..2 (fp64) -- Haar-uniform within the drawn cell, so the draws follow the
 * piecewise-constant density; without jitter it is the row of rnf_so3_healpix_grid, bit for bit.  level = -1: any Q, rows only.
 * An image with a NaN, a maximum of +inf or no finite value (T = 0): index -1, target 0, total 0, NaN rotations, for that image alone.
 * Cost: one pass over the g Q values for the maximum, one for the sums of chunks of 64 rows, a scan of Q / 64 sums per image, then
 * O(log Q) + at most 64 masses per draw; every call pays the passes again, so tile the draws coarsely.  Deterministic: integer sums only, block
 * counts depend on Q alone, a draw's numbers on (seed, k, b) alone -- bit-identical from run to run, whatever images share a call and
 * however the draws are tiled.  Stream-ordered, no host synchronisation, capturable (the seed is an argument, so a replay repeats it). */
#define RNF_GRID_SAMPLE_MULTINOMIAL 0
#define RNF_GRID_SAMPLE_SYSTEMATIC 1
typedef struct RnfGridSample {
    size_t struct_bytes;        /* sizeof(RnfGridSample); any other value is refused (header and library differ) */
    const float *logp;          /* dev float[g][Q] */
    int64_t Q;                  /* 1..2^26 */
    int32_t g;                  /* images, 1..65535 */
    int32_t level;              /* -1, or 0..6 with Q == 72 * 8^level */
    int64_t draws;              /* per image in this call, >= 0 */
    int64_t draw_base;          /* global index of the call's first draw, >= 0; draw_base + draws <= draws_total */
    int64_t draws_total;        /* N, 1..2^30: the draws per image over all calls (systematic spacing) */
    int64_t image_base;         /* global index of the call's first image, >= 0 */
    int32_t method;             /* RNF_GRID_SAMPLE_* */
    int32_t jitter;             /* 0 or 1; read with rot_out alone */
    uint64_t seed;
    const float *offset;        /* dev float[9] row-major, or NULL (identity); read with rot_out alone */
    int64_t *index_out;         /* dev int64[g][draws] */
    uint64_t *target_out;       /* dev uint64[g][draws], or NULL: v_k */
    uint64_t *total_out;        /* dev uint64[g], or NULL: T */
    float *rot_out;             /* dev float[g][draws][9], or NULL */
    /* dev scratch, 8-byte aligned, of at least rnf_grid_sample_workspace_bytes(this struct) bytes =
     * g * (16 min(ceil(Q / 2048), 2048) + 8 ceil(Q / 64) + 20) rounded up to 16: the maximum's partials and the chunk prefix */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfGridSample;
int rnf_grid_sample(const RnfGridSample *sample);
/* The workspace rnf_grid_sample requires for the same struct (the pointers are not read); 0 when struct_bytes, g or Q are out of range. */
size_t rnf_grid_sample_workspace_bytes(const RnfGridSample *sample);

/* Pairwise sums of isotropic matrix-Fisher kernels between two sets of rotations (csrc/so3_kernel_sum.h): the kernel density estimate
 * on SO(3) and the prediction step of a Bayes filter on the SO(3) grid.  With w_g = softmax(log_weights[g]) over the n centres (w = 1/n
 * without log-weights),
 *   out[g][a][i] = log sum_j w_gj k_a(C_j, Q_i),   k_kappa(C, Q) = exp(-(kappa/2) |Q - C|_F^2 - l(kappa)),
 *   l(kappa) = c(kappa I) - 3 kappa = log(i0e(2 kappa) - i1e(2 kappa)) in fp64, l(0) = 0:
 * k_kappa(C, .) is the density of MF(kappa C) w.r.t. the Haar probability measure.  The exponent is formed from the nine differences of
 * the fp32 entries, never from tr(C^T Q) - 3, which loses all digits for sharp kernels.  Each (g, a, i) is a log-sum-exp about its
 * largest term: finite whenever a finite weight exists (a query 90 degrees from its nearest centre at kappa = 1e4 returns about -1e4).
 * leave_one_out != 0: the queries are the centres (queries NULL or == centres, m == n) and
 *   out[g][a][i] = log sum_{j != i} w_gj k_a(C_j, C_i) - log1p(-w_gi);   only index i is left out, a duplicate of C_i elsewhere counts.
 * Edge cases: a centre with log-weight -inf is left out whatever its entries; any other centre with a non-finite entry, or a NaN
 * log-weight, makes every output of that group NaN; a query with a non-finite entry is NaN; a group with no mass left (all weights
 * -inf, leave-one-out with n = 1, w_gi = 1) is NaN.  m = 0 is a no-op.
 * Deterministic: the centres are split into chunks of 4096 (a function of n alone), one (max, sum) partial is written per (query,
 * bandwidth, group, chunk) -- fp32 sums over at most 64 centres, fp64 above -- and a finalise combines the chunk partials in chunk
 * order in fp64, subtracts the normalisers and rounds once to fp32; no floating-point atomics.  A query's result is bit-identical from
 * run to run and whatever m, G, the query's position and the group's position are: queries and groups may be tiled over calls.
 * Four launches.  Stream-ordered, no host synchronisation, capturable in a HIP graph as a linear chain. */
typedef struct RnfSo3KernelSum {
    size_t struct_bytes;        /* sizeof(RnfSo3KernelSum); any other value is refused (header and library differ) */
    const float *centres;       /* dev float[n][9] row-major, 16-byte aligned */
    const float *queries;       /* dev float[m][9] row-major, 16-byte aligned, or NULL: the centres (then m must be n) */
    const float *log_weights;   /* dev float[G][n], or NULL (uniform weights) */
    int64_t n;                  /* centres, 1..2^24 */
    int64_t m;                  /* queries, 0..2^31 - 1 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    const double *kappas;       /* HOST double[J], each finite in 0..1e6 */
    int32_t J;                  /* bandwidths, 1..8 */
    int32_t leave_one_out;      /* 0, or != 0 as above */
    float *out;                 /* dev float[G][J][m] */
    /* dev scratch, 8-byte aligned, of at least rnf_so3_kernel_sum_workspace_bytes(this struct) bytes =
     * 12 G J ceil(n / 4096) m + 16 G ceil(n / 4096) + 8 G rounded up to 16 */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfSo3KernelSum;
int rnf_so3_kernel_sum(const RnfSo3KernelSum *sum);
/* The workspace rnf_so3_kernel_sum requires for the same struct (the pointers are not read); 0 when struct_bytes, J, G, n or m are out of
 * range or the size does not fit. */
size_t rnf_so3_kernel_sum_workspace_bytes(const RnfSo3KernelSum *sum);

/* Responsibility-weighted first moments of the same kernel sum (csrc/so3_kernel_moments.h): the score of the kernel density estimate,
 * its mean-shift step and its derivative with respect to the bandwidth.  One concentration kappa, no leave-one-out.  With
 * r_ij = w_gj k(C_j, Q_i) / sum_l w_gl k(C_l, Q_i), per group g and query i:
 *   log_density = log sum_j w_gj k(C_j, Q_i)        bit-identical to rnf_so3_kernel_sum's output for the same inputs with J = 1
 *   mean        = M_i = sum_j r_ij C_j              so that d log p / dQ_i = kappa (M_i - Q_i)
 *   msd         = D_i = sum_j r_ij |Q_i - C_j|_F^2  so that d log p / dkappa = -D_i / 2 - l'(kappa)
 *   rotation    = polar(M_i), the rotation that maximises tr(M_i^T R): the mean-shift step.  NaN where det M_i <= 0 (a convex
 *                 combination of rotations need not have a mean direction) or where M_i is too ill-conditioned to project
 *   step        = |rotation - Q_i|_F, NaN where rotation is
 * Any output pointer may be NULL, except that step requires rotation.  group_queries != 0: every group has its own m queries
 * (queries float[G][m][9]); otherwise the G groups share queries float[m][9].
 * The edge cases are those of rnf_so3_kernel_sum, for every output of the (group, query): a centre with log-weight -inf is left out
 * whatever its entries; another non-finite centre or a NaN log-weight makes its group NaN; a non-finite query is NaN; a group with no
 * mass is NaN; m = 0 is a no-op; kappa = 0 gives mean = sum_j w_gj C_j for every query.
 * Deterministic in the same way: chunks of 4096 centres, one partial (fp32 max, 11 fp64 sums: e, e d^2, e C[0..8]; fp32 over at most 64
 * centres) per (group, chunk, query), combined in chunk order in fp64, divided by the first sum and rounded once; no floating-point
 * atomics.  A query's outputs are bit-identical from run to run and whatever m, G, the query's position and the group's position
 * are, and whether its queries are shared or given per group.  Five launches.  Stream-ordered, no host synchronisation, capturable in a
 * HIP graph as a linear chain. */
typedef struct RnfSo3KernelMoments {
    size_t struct_bytes;        /* sizeof(RnfSo3KernelMoments); any other value is refused (header and library differ) */
    const float *centres;       /* dev float[n][9] row-major, 16-byte aligned */
    const float *queries;       /* dev float[m][9], or float[G][m][9] with group_queries; 16-byte aligned */
    const float *log_weights;   /* dev float[G][n], or NULL (uniform weights) */
    int64_t n;                  /* centres, 1..2^24 */
    int64_t m;                  /* queries (per group), 0..2^31 - 1 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    int32_t group_queries;      /* 0: the groups share the queries; != 0: one set per group */
    double kappa;               /* finite, 0..1e6 */
    float *log_density;         /* dev float[G][m], or NULL */
    float *mean;                /* dev float[G][m][9], or NULL */
    float *msd;                 /* dev float[G][m], or NULL */
    float *rotation;            /* dev float[G][m][9], or NULL */
    float *step;                /* dev float[G][m], or NULL; requires rotation */
    double *dlog_normaliser;    /* HOST double, or NULL: receives l'(kappa) (fp64, l'(0) = -3), also when m = 0 */
    /* dev scratch, 8-byte aligned, of at least rnf_so3_kernel_moments_workspace_bytes(this struct) bytes =
     * 92 G ceil(n / 4096) m + 16 G ceil(n / 4096) + 8 G + 4 ceil(n / 4096) rounded up to 16 */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfSo3KernelMoments;
int rnf_so3_kernel_moments(const RnfSo3KernelMoments *moments);
/* The workspace rnf_so3_kernel_moments requires for the same struct (the pointers are not read); 0 when struct_bytes, G, n or m are out
 * of range or the size does not fit. */
size_t rnf_so3_kernel_moments_workspace_bytes(const RnfSo3KernelMoments *moments);

/* The distribution function of the geodesic angle from query rotations to a weighted set of rotations (csrc/so3_angle_cdf.h): the
 * mass of a ball about an estimate, hence its error radii, and its expected error.  Centres, queries, log-weights and groups as
 * rnf_so3_kernel_moments.  With d2_ij = |Q_i - C_j|_F^2 = 8 sin^2(theta_ij / 2) from the nine fp32 differences (capped at FLT_MAX) and
 * theta_ij = 2 asin(min(1, sqrt(d2_ij / 8))), per group g and query i:
 *   mass[g][t][i]       = sum_j w_gj [d2_ij <= tau_t]     fp32, in [0, 1]
 *   mean_angle[g][i]    = sum_j w_gj theta_ij             radians
 *   mean_sq_angle[g][i] = sum_j w_gj theta_ij^2
 * The T thresholds, 0 <= T <= 8, come in exactly one of two forms: thresholds, HOST angles in radians in [0, pi] shared by all queries,
 * each converted to tau = (float)(8 sin^2(theta / 2)) in fp64 and rounded once (an angle >= pi is FLT_MAX: everything counts); or
 * query_tau, squared chordal distances on the device, one set per (group, query).  Both NULL with T = 0 is allowed when a moment output
 * is requested.  The comparison is made on d2, never on an angle.  Any output pointer may be NULL.
 * Edge cases: a centre with log-weight -inf is left out whatever its entries; another non-finite centre or a NaN log-weight makes its
 * group NaN; a non-finite query is NaN; a group with no mass is NaN; m = 0 is a no-op; a NaN query_tau entry gives a NaN mass for that
 * slot only; tau < 0 gives 0.
 * Deterministic: chunks of 4096 centres, normalised fp32 weights from a prepass, one fp64 partial per (group, chunk, query, slot) --
 * fp32 over at most 64 centres -- added in chunk order in fp64 and rounded once; no floating-point atomics.  A (group, query)'s outputs
 * are bit-identical from run to run and whatever m, G, the query's position and the group's position are, whether its queries are
 * shared or given per group, and however the thresholds are split over calls.  Five launches.  Stream-ordered, no host
 * synchronisation, capturable in a HIP graph as a linear chain. */
typedef struct RnfSo3AngleCdf {
    size_t struct_bytes;        /* sizeof(RnfSo3AngleCdf); any other value is refused (header and library differ) */
    const float *centres;       /* dev float[n][9] row-major, 16-byte aligned */
    const float *queries;       /* dev float[m][9], or float[G][m][9] with group_queries; 16-byte aligned */
    const float *log_weights;   /* dev float[G][n], or NULL (uniform weights) */
    int64_t n;                  /* centres, 1..2^24 */
    int64_t m;                  /* queries (per group), 0..2^31 - 1 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    int32_t group_queries;      /* 0: the groups share the queries; != 0: one set per group */
    int32_t T;                  /* thresholds, 0..8; 0 only with a moment output */
    const double *thresholds;   /* HOST double[T] angles in radians, each finite in [0, pi], or NULL */
    const float *query_tau;     /* dev float[G][T][m] squared chordal distances, or NULL; exactly one of the two when T > 0 */
    float *mass;                /* dev float[G][T][m], or NULL */
    float *mean_angle;          /* dev float[G][m], or NULL */
    float *mean_sq_angle;       /* dev float[G][m], or NULL */
    /* dev scratch, 8-byte aligned, of at least rnf_so3_angle_cdf_workspace_bytes(this struct) bytes =
     * 8 G S ceil(n / 4096) m + 16 G ceil(n / 4096) + 8 G + 4 G n rounded up to 16, with S = (T if mass is not NULL) + (2 if mean_angle or
     * mean_sq_angle is not NULL) */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfSo3AngleCdf;
int rnf_so3_angle_cdf(const RnfSo3AngleCdf *cdf);
/* The workspace rnf_so3_angle_cdf requires for the same struct (of the pointers only mass, mean_angle and mean_sq_angle are looked at,
 * for being NULL; none is read through); 0 when struct_bytes, T, G, n or m are out of range or the size does not fit. */
size_t rnf_so3_angle_cdf_workspace_bytes(const RnfSo3AngleCdf *cdf);

/* The distribution function of the geodesic angle from a weighted set of rotations to the NEAREST member of a set of query rotations
 * (csrc/so3_set_angle_cdf.h): the error about an estimate of a symmetric object (the set is the estimate's orbit E S_s under the
 * object's symmetry group) and the best-of-k error of k modes.  Centres, log-weights, groups, thresholds, outputs, arithmetic and
 * edge cases as rnf_so3_angle_cdf, with queries that are m sets of K members and
 *   d2_ij = min over the live members s of |Q_is - C_j|_F^2,     theta_ij = 2 asin(min(1, sqrt(d2_ij / 8)))
 * in place of the single distance.  A member is live when its nine entries are finite; every other member is padding and is skipped
 * (its distance is FLT_MAX), which is how sets of unequal size are passed.  A set with no live member is NaN in all of its outputs.
 * min is exact: a set's outputs depend neither on the order of its members nor on padding among them, and with K = 1 every output has
 * the bits of rnf_so3_angle_cdf for the same arguments.  Otherwise deterministic as rnf_so3_angle_cdf: a (group, set)'s outputs are
 * bit-identical from run to run and whatever m, G, the set's position and the group's position are, whether the sets are shared or
 * given per group, and however the thresholds are split over calls.  Five launches.  Stream-ordered, no host synchronisation,
 * capturable in a HIP graph as a linear chain. */
typedef struct RnfSo3SetAngleCdf {
    size_t struct_bytes;        /* sizeof(RnfSo3SetAngleCdf); any other value is refused (header and library differ) */
    const float *centres;       /* dev float[n][9] row-major, 16-byte aligned */
    const float *queries;       /* dev float[m][K][9], or float[G][m][K][9] with group_queries; 16-byte aligned */
    const float *log_weights;   /* dev float[G][n], or NULL (uniform weights) */
    int64_t n;                  /* centres, 1..2^24 */
    int64_t m;                  /* sets (per group), 0..2^31 - 1 */
    int32_t K;                  /* members per set, padding included, 1..4096 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    int32_t group_queries;      /* 0: the groups share the sets; != 0: m sets per group */
    int32_t T;                  /* thresholds, 0..8; 0 only with a moment output */
    const double *thresholds;   /* HOST double[T] angles in radians, each finite in [0, pi], or NULL */
    const float *query_tau;     /* dev float[G][T][m] squared chordal distances, or NULL; exactly one of the two when T > 0 */
    float *mass;                /* dev float[G][T][m], or NULL */
    float *mean_angle;          /* dev float[G][m], or NULL */
    float *mean_sq_angle;       /* dev float[G][m], or NULL */
    /* dev scratch, 8-byte aligned, of at least rnf_so3_set_angle_cdf_workspace_bytes(this struct) bytes: rnf_so3_angle_cdf's for m
     * queries; it does not grow with K */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfSo3SetAngleCdf;
int rnf_so3_set_angle_cdf(const RnfSo3SetAngleCdf *cdf);
/* The workspace rnf_so3_set_angle_cdf requires for the same struct (of the pointers only mass, mean_angle and mean_sq_angle are looked
 * at, for being NULL; none is read through); 0 when struct_bytes, T, K, G, n or m are out of range or the size does not fit. */
size_t rnf_so3_set_angle_cdf_workspace_bytes(const RnfSo3SetAngleCdf *cdf);

/* Neighbour-limited sums of matrix-Fisher kernels over the rows of the HEALPix SO(3) grid (csrc/so3_grid_local.h): the prediction step of
 * a Bayes filter on the grid at the levels where rnf_so3_kernel_sum's Q^2 pairs cannot run.  With the grid rows G_j of
 * rnf_so3_healpix_grid(level, offset), d^2 = |G_j - Q_i|_F^2 = 4 (1 - cos omega) and k_kappa the kernel of rnf_so3_kernel_sum,
 *   out[g][i] = log sum_{j : d^2(G_j, Q_i) <= d2_cut} exp(log_weights[g][j]) k_kappa(G_j, Q_i),     count[i] = the number of such j.
 * The log-weights are NOT normalised (rnf_so3_kernel_sum normalises its weights; this pass does not).  The neighbourhood is listed from
 * the grid's structure -- rings, an azimuth window per ring, a tilt window per pixel, each a superset -- and membership is decided by the
 * fp32 distance of the stored rows alone, which is symmetric bit for bit: neighbourhoods among grid rows are symmetric, and every row
 * counts once.  grid must hold the rows rnf_so3_healpix_grid wrote for the same level and offset; the queries may be any rotations.
 * Edge cases: an empty or massless neighbourhood gives -inf; a row with log-weight -inf drops out; a NaN log-weight inside a query's
 * neighbourhood makes that output NaN; a query with a non-finite entry gives NaN and count 0.  m = 0 is a no-op.
 * Deterministic: one thread per query, its terms in the order (ring, pixel, tilt) of increasing index, max-then-sum, fp32 within a
 * pixel's tilt run and fp64 above, no floating-point atomics.  A result is bit-identical from run to run and whatever m, G, the
 * query's position and the group's position are: queries and groups may be tiled over calls.
 * One launch, no workspace.  Stream-ordered, no host synchronisation, capturable in a HIP graph. */
typedef struct RnfSo3GridLocalSum {
    size_t struct_bytes;        /* sizeof(RnfSo3GridLocalSum); any other value is refused (header and library differ) */
    int32_t level;              /* 0..6: Q = 72 * 8^level grid rows */
    const float *offset;        /* dev float[9], the grid's offset O (row-major, a rotation), or NULL (the identity) */
    const float *grid;          /* dev float[Q][9] row-major, 16-byte aligned */
    const float *queries;       /* dev float[m][9] row-major, 16-byte aligned, or NULL: the grid rows (then m must be Q) */
    const float *log_weights;   /* dev float[G][Q], or NULL (zeros) */
    int64_t m;                  /* queries, 0..2^31 - 1 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    double kappa;               /* finite, 0..1e6 */
    double d2_cut;              /* finite, 0..8; 8 (180 degrees) covers every row: rows whose fp32 distance rounds above 8 included */
    float *out;                 /* dev float[G][m] */
    int32_t *count;             /* dev int32[m], or NULL */
    void *stream;
} RnfSo3GridLocalSum;
int rnf_so3_grid_local_sum(const RnfSo3GridLocalSum *sum);

/* The max-plus pass over the same neighbourhoods (csrc/so3_grid_local.h): the step of a Viterbi recursion on the grid, which the sum
 * cannot express (a log-sum has no arg-max).  With the rows, queries, kappa, d2_cut and log-weights of rnf_so3_grid_local_sum,
 *   out[g][i] = max_{j : d^2(G_j, Q_i) <= d2_cut} (log_weights[g][j] - (kappa/2) d^2(G_j, Q_i)) - l(kappa),
 *   arg[g][i] = the smallest row index j attaining that maximum,     count[i] = the number of such j.
 * The enumeration and the membership are the sum's own, bit for bit.  The maximum and the tie are decided on the sum's fp32 term
 * t = fma(-h, d^2, lw log2 e); the tie goes to the smallest row, compared explicitly (members arrive by ring, pixel and tilt, not by
 * row).  One sweep, no exp2.
 * Edge cases: an empty neighbourhood, or one whose members all have log-weight -inf, gives -inf and arg -1; a NaN log-weight inside a
 * query's neighbourhood gives NaN and arg -1; a query with a non-finite entry gives NaN, arg -1 and count 0.  m = 0 is a no-op.
 * Deterministic: one thread per query; a result is bit-identical from run to run and whatever m, G, the query's position and the
 * group's position are: queries and groups may be tiled over calls.
 * One launch, no workspace.  Stream-ordered, no host synchronisation, capturable in a HIP graph. */
typedef struct RnfSo3GridLocalMax {
    size_t struct_bytes;        /* sizeof(RnfSo3GridLocalMax); any other value is refused (header and library differ) */
    int32_t level;              /* 0..6: Q = 72 * 8^level grid rows */
    const float *offset;        /* dev float[9], the grid's offset O (row-major, a rotation), or NULL (the identity) */
    const float *grid;          /* dev float[Q][9] row-major, 16-byte aligned */
    const float *queries;       /* dev float[m][9] row-major, 16-byte aligned, or NULL: the grid rows (then m must be Q) */
    const float *log_weights;   /* dev float[G][Q], or NULL (zeros) */
    int64_t m;                  /* queries, 0..2^31 - 1 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    double kappa;               /* finite, 0..1e6 */
    double d2_cut;              /* finite, 0..8; 8 (180 degrees) covers every row */
    float *out;                 /* dev float[G][m] */
    int32_t *arg;               /* dev int32[G][m], required */
    int32_t *count;             /* dev int32[m], or NULL */
    void *stream;
} RnfSo3GridLocalMax;
int rnf_so3_grid_local_max(const RnfSo3GridLocalMax *max);

/* The two passes above on an ANISOTROPIC matrix-Fisher kernel (csrc/so3_grid_local.h): the transition of a grid filter whose motion
 * x' = x E, E ~ MF(A), drifts and is tighter about some body axes than others.  With the proper SVD A = U diag(s) V^T, the drift
 * Delta = U V^T and the symmetric concentration K = V diag(s) V^T (A = Delta K), the density of the step from Q to G is
 *   k_K(C, G) = exp(-1/2 tr((G - C) K (G - C)^T) - l(K)),   C = Q Delta,   l(K) = c(K) - tr K,
 * c the exact log-normaliser of rnf_fisher_exact (computed here on the host in fp64).  The drift is the CALLER's: this entry takes K
 * alone and evaluates k_K between the stored rows and the queries, so a drifting model passes the shifted rows C = G Delta (the rows of
 * the grid with offset O Delta) on one side.  With arg NULL it is rnf_so3_grid_local_sum,
 *   out[g][i] = log sum_{j : d^2(G_j, Q_i) <= d2_cut} exp(log_weights[g][j]) k_K(G_j, Q_i),
 * with arg non-NULL rnf_so3_grid_local_max (the largest term, and the smallest row attaining it).  Membership is the isotropic
 * passes' -- the fp32 |G_j - Q_i|_F^2 <= d2_cut on the stored rows, a ball -- and so are the enumeration, the order of the terms, the
 * edge cases, the determinism and the tiling: a result is bit-identical from run to run and whatever m, G, the query's position and
 * the group's position are.  The term is symmetric bit for bit in (row, query).  The exponent is bounded by -(s2 + s3)/4 d^2.  K = kappa I
 * is the isotropic kernel of concentration kappa (to rounding; the log-weights are NOT normalised here either).
 * Refused before any launch: a non-finite K; a K that is not symmetric to 1e-9 |K|_F; eigenvalues with a pair sum below -1e-9 |K|_F
 * (K is then not the symmetric factor of a proper SVD); a largest |eigenvalue| above 3e4 (the range rnf_fisher_exact is tested on);
 * and everything rnf_so3_grid_local_sum / _max refuse.  One launch, no workspace.  Stream-ordered, no host synchronisation, capturable. */
typedef struct RnfSo3GridLocalFisher {
    size_t struct_bytes;        /* sizeof(RnfSo3GridLocalFisher); any other value is refused (header and library differ) */
    int32_t level;              /* 0..6: Q = 72 * 8^level grid rows */
    const float *offset;        /* dev float[9], the offset of the rows in grid (row-major, a rotation), or NULL (the identity) */
    const float *grid;          /* dev float[Q][9] row-major, 16-byte aligned */
    const float *queries;       /* dev float[m][9] row-major, 16-byte aligned, or NULL: the grid rows (then m must be Q) */
    const float *log_weights;   /* dev float[G][Q], or NULL (zeros) */
    int64_t m;                  /* queries, 0..2^31 - 1 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    double concentration[9];    /* K row-major: symmetric, finite, eigenvalue pair sums >= 0, |eigenvalues| <= 3e4 */
    double d2_cut;              /* finite, 0..8; 8 (180 degrees) covers every row */
    float *out;                 /* dev float[G][m] */
    int32_t *arg;               /* dev int32[G][m], or NULL: the sum; non-NULL: the max-plus pass */
    int32_t *count;             /* dev int32[m], or NULL */
    void *stream;
} RnfSo3GridLocalFisher;
int rnf_so3_grid_local_fisher(const RnfSo3GridLocalFisher *fisher);

/* Harmonic analysis on SO(3) (csrc/so3_harmonics.h).  Y_l(x) is the vector of the 2l+1 orthonormal real spherical harmonics of degree
 * l, m = -l..l: sqrt2 (-1)^m Re Y_l^m for m > 0, sqrt2 (-1)^m Im Y_l^|m| for m < 0, Y_l^0 for m = 0 (for l = 1: y, z, x).  The Wigner
 * matrix D^l(R) is the real orthogonal (2l+1) x (2l+1) matrix with Y_l(R x) = D^l(R) Y_l(x): D^l(R1 R2) = D^l(R1) D^l(R2), D^0 = 1,
 * D^1(R)[i][j] = R[p_i][p_j] with p = (1, 2, 0).  Layout of the C_L = (L+1)(2L+1)(2L+3)/3 entries of degrees 0..L: the degrees one after
 * the other, degree l at l (4 l^2 - 1) / 3, row-major with m' (row) and m (column) from -l to l.  A 3x3 row is read through its
 * normalised quaternion (no Euler angles: no singular chart), so a row that is not exactly orthogonal, or is scaled, is read as the
 * rotation of that quaternion.  All three entries are stream-ordered, free of host synchronisation and capturable in a HIP graph as
 * a linear chain; each builds its constants in its own workspace, none keeps state. */
#define RNF_SO3_MAX_DEGREE 16

/* out[i] = the entries of D^l(rotations[i]), l <= lmax.  A rotation with a non-finite entry gives NaN entries for that row alone.
 * n = 0 is a no-op.  Two launches. */
typedef struct RnfSo3Wigner {
    size_t struct_bytes;        /* sizeof(RnfSo3Wigner); any other value is refused (header and library differ) */
    const float *rotations;     /* dev float[n][9] row-major */
    int64_t n;                  /* rotations, 0..2^24 */
    int32_t lmax;               /* L, 0..16 */
    float *out;                 /* dev float[n][C_L] */
    void *workspace;            /* dev scratch, 16-byte aligned, of at least rnf_so3_wigner_workspace_bytes(this struct) bytes */
    size_t workspace_bytes;
    void *stream;
} RnfSo3Wigner;
int rnf_so3_wigner(const RnfSo3Wigner *wigner);
/* 4 (2L+1)^2 (2 + 4L) rounded up to 16; 0 when struct_bytes, lmax or n are out of range (the pointers are not read) */
size_t rnf_so3_wigner_workspace_bytes(const RnfSo3Wigner *wigner);

/* The Fourier coefficients of weighted rotations: with w_g = softmax(log_weights[g]) (uniform without log-weights), formed as
 * rnf_so3_kernel_sum forms them,   out[g] = sum_j w_gj D(centres[j])   (all degrees up to lmax; out[g][0] = 1 up to rounding).
 * Edge cases: a centre with log-weight -inf is left out whatever its entries; another non-finite centre or a NaN log-weight makes its
 * group NaN; a group with no mass is NaN.
 * Deterministic: chunks of 4096 centres, normalised fp32 weights from a prepass, one fp64 partial per (group, chunk, coefficient) --
 * the exact products w D added in fp64 in centre order -- added in chunk order in fp64 and rounded once; no floating-point atomics.  A group's coefficients are
 * bit-identical from run to run and whatever G and the group's position are, and a coefficient's bits do not depend on lmax: groups and
 * degrees may be split over calls.  Seven launches. */
typedef struct RnfSo3Fourier {
    size_t struct_bytes;        /* sizeof(RnfSo3Fourier) */
    const float *centres;       /* dev float[n][9] row-major */
    const float *log_weights;   /* dev float[G][n], or NULL (uniform weights) */
    int64_t n;                  /* centres, 1..2^24 */
    int32_t G;                  /* groups (rows of log-weights), 1..65535 */
    int32_t lmax;               /* L, 0..16 */
    float *out;                 /* dev float[G][C_L] */
    /* dev scratch, 16-byte aligned, of at least rnf_so3_fourier_workspace_bytes(this struct) bytes = 8 G ceil(n / 4096) C_L +
     * 16 G ceil(n / 4096) + 8 G + 4 G n rounded up to 16, + 4 n (8L + 16) + 4 (2L+1)^2 (2 + 4L) rounded up to 16 */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfSo3Fourier;
int rnf_so3_fourier(const RnfSo3Fourier *fourier);
size_t rnf_so3_fourier_workspace_bytes(const RnfSo3Fourier *fourier);

/* The band-limited function with coefficients coeffs[g] at query rotations:   out[g][i] = sum_l sum_{m'm} coeffs[g][l, m', m]
 * D^l_{m'm}(queries[i]).  With coeffs^l = (2l+1) h_l F^l of rnf_so3_fourier this is a density relative to the normalised Haar measure
 * (uniform = 1), the measure convolved with the zonal kernel of multipliers h_l.  An entry's degrees are added in fp32 (at most 17
 * terms), the entries in fp64 in a fixed order, rounded once: a (group, query)'s value is bit-identical however queries and groups are
 * tiled over calls, and whether the queries are shared or given per group.  A non-finite query gives NaN for that query alone;
 * non-finite coefficients stay in their own group.  m = 0 is a no-op.  Two launches. */
typedef struct RnfSo3FourierEval {
    size_t struct_bytes;        /* sizeof(RnfSo3FourierEval) */
    const float *coeffs;        /* dev float[G][C_L] */
    const float *queries;       /* dev float[m][9], or float[G][m][9] with group_queries */
    int64_t m;                  /* queries (per group), 0..2^31 - 1 */
    int32_t G;                  /* groups (rows of coefficients), 1..65535 */
    int32_t group_queries;      /* 0: the groups share the queries; != 0: one set per group */
    int32_t lmax;               /* L, 0..16 */
    float *out;                 /* dev float[G][m] */
    void *workspace;            /* dev scratch, 16-byte aligned, of at least rnf_so3_fourier_eval_workspace_bytes(this struct) bytes */
    size_t workspace_bytes;
    void *stream;
} RnfSo3FourierEval;
int rnf_so3_fourier_eval(const RnfSo3FourierEval *eval);
/* 4 (2L+1)^2 (2 + 4L) rounded up to 16; 0 when struct_bytes, lmax, G or m are out of range (the pointers are not read) */
size_t rnf_so3_fourier_eval_workspace_bytes(const RnfSo3FourierEval *eval);

/* Proper SVD of B parameter matrices on the device (utils/fisher.py:53-76): A = U diag(s) V^T with U, V rotations (row-major, singular
 * vectors as columns), s[2] carrying the sign of det A; lam [B,4] = the Bingham parameters the sampler takes (utils/fisher.py:151-158).
 * Any output pointer may be NULL.  Stream-ordered, no host synchronisation. */
int rnf_fisher_proper_svd(const float *A_dev, int64_t B, float *U_dev, float *V_dev, float *s_dev, float *lam_dev, void *stream);

/* Log-constants c[b] of MatrixFisherN(A[b]) with the default normaliser approximation (utils/fisher.py:67-76 proper singular
 * values, :93-97 norm_type = 1): log p(R) = tr(A^T R) - c.  A_dev float[B][9], c_out_dev float[B]; fp64 inside. */
int rnf_fisher_log_const(const float *A_dev, int64_t B, float *c_out_dev, void *stream);

/* The same for either closed-form normaliser approximation of matrix_fisher_norm_N (utils/fisher.py:79-97):
 *   norm_type 1 (default): 1/sqrt(8 pi (s0+s1)(s1+s2)(s0+s2));
 *   norm_type 0: (1 + Q/6 + s0 s1 s2/6)/exp(s0+s1+s2), where the reference's `(S**2).sum()` has no `dim`: Q runs over ALL B matrices of
 *   the call (batch-coupled, reproduced as is);
 *   RNF_FISHER_NORM_EXACT (3): the exact integral that the reference's type 3 means (its scipy ODE indexes rows of the [B,3] tensor and
 *   serves no batch), evaluated per row by rnf_fisher_exact's kernel; needs no scratch.
 *   Type 2 (Monte-Carlo, below) is refused here.  scratch_dev: rnf_fisher_scratch_bytes(B) bytes of device memory (16 suffice here). */
#define RNF_FISHER_NORM_EXACT 3
size_t rnf_fisher_scratch_bytes(int64_t B);
/* norm_type 2 (utils/fisher.py:98-101): Monte-Carlo normaliser over approx_num uniform rotations for ONE matrix (B must be 1: the
 * reference broadcasts [approx_num,3,3] against [N,3,3]); counter-based Philox stream keyed by `seed` (statistical parity with the
 * reference's pytorch3d.random_rotations).  scratch_dev: 8 bytes. */
int rnf_fisher_log_const_mc(const float *A_dev, int64_t B, int64_t approx_num, uint64_t seed, void *scratch_dev, size_t scratch_bytes,
                            float *c_out_dev, void *stream);
int rnf_fisher_log_const_nt(const float *A_dev, int64_t B, int32_t norm_type, void *scratch_dev, size_t scratch_bytes,
                            float *c_out_dev, void *stream);

/* The exact log-normaliser of the matrix-Fisher density w.r.t. the Haar probability measure, and its derivative: with the proper singular
 * values s0 >= s1 >= |s2| of A,
 *   c(A) = s0+s1+s2 + log int_{-1}^{1} 1/2 i0e(1/2 (s0-s1)(1-u)) i0e(1/2 (s0+s1)(1+u)) exp(-(s1+s2)(1-u)) du,   dc/dA = U diag(dc/ds) V^T = E[R]
 * (i0e(x) = exp(-x) I0(x)), by a fixed 224-node Gauss-Legendre rule in fp64, one wave per matrix (csrc/fisher_exact.h).  Finite and smooth
 * for every finite A (A = 0: c = 0, E[R] = 0); a row's result is bit-identical whatever B and the row's position.  c_out_dev float[B],
 * mean_out_dev float[B][9] row-major; either may be NULL, not both.  B = 0 is a no-op.  Stream-ordered, no host synchronisation,
 * capturable in a HIP graph. */
int rnf_fisher_exact(const float *A_dev, int64_t B, float *c_out_dev, float *mean_out_dev, void *stream);
/* The entropy c - tr(A^T E[R]) of MF(A[b]) from the same kernel, summed in fp64 in a form without the cancellation of c against
 * tr(A^T E[R]) (both ~ |s|, which the fp32 outputs of rnf_fisher_exact cannot carry).  entropy_out_dev float[B]. */
int rnf_fisher_entropy(const float *A_dev, int64_t B, float *entropy_out_dev, void *stream);

/* Weighted moments of G groups of n rotations, M_g = sum_i w_gi R_gi, in fp64: the sufficient statistic of a matrix-Fisher fit.  With
 * log_weights, w_g = softmax(log_weights[g]) over the n rows (maximum subtracted, exp and sums in fp64; a -inf row contributes 0);
 * without, w = 1/n.  shared_rotations != 0: one set of rotations [n][9] serves every group (a grid and one row of log-densities per
 * image); it needs log_weights.  A group whose weights are all -inf, or that holds a NaN, yields NaN.  Deterministic: chunks of 4096
 * rows, fixed-order sums, no atomics -- a group's moment is bit-identical whatever G and the group's position.  Stream-ordered, no host
 * synchronisation, capturable in a HIP graph. */
typedef struct RnfRotationMoments {
    size_t struct_bytes;        /* sizeof(RnfRotationMoments); any other value is refused */
    const float *rotations;     /* dev float[G][n][9] row-major, or float[n][9] with shared_rotations */
    const float *log_weights;   /* dev float[G][n], or NULL (w = 1/n) */
    int64_t n;                  /* rotations per group, 1..2^40 */
    int64_t G;                  /* groups, >= 1; G * ceil(n / 4096) <= 2^31 - 1 */
    int32_t shared_rotations;   /* 0, or 1: rotations is [n][9] for every group */
    double *moments_out;        /* dev double[G][9] row-major */
    /* dev scratch, 8-byte aligned, of at least rnf_rotation_moments_workspace_bytes(this struct) bytes = G * ceil(n / 4096) * 88 */
    void *workspace;
    size_t workspace_bytes;
    void *stream;
} RnfRotationMoments;
int rnf_rotation_moments(const RnfRotationMoments *moments);
/* The workspace rnf_rotation_moments requires for the same struct (the workspace fields are not read); 0 when struct_bytes, n or G are
 * out of range. */
size_t rnf_rotation_moments_workspace_bytes(const RnfRotationMoments *moments);

/* The maximum-likelihood matrix-Fisher parameter of B moment matrices: A[b] with E_A[R] = dc/dA = moments[b] under the exact normaliser
 * (csrc/fisher_fit.h).  With the proper SVD moments[b] = U diag(d) V^T, A = U diag(s) V^T where s solves grad c(s) = d by a damped
 * Newton iteration with the analytic Hessian H = d2c/ds2 = Cov(Q_ii, Q_jj), one wave per matrix; a row's outputs are bit-identical
 * whatever B and the row's position.  status_out bits:
 *   RNF_FIT_CAPPED (1)         d on the boundary of conv{(1,1,1), (1,-1,-1), (-1,1,-1), (-1,-1,1)} (one sample, identical samples), or a
 *                              maximiser with s0 > max_concentration: the outputs are the maximiser of the likelihood over the box
 *                              |s_i| <= max_concentration, finite and ordered, s0 == max_concentration;
 *   RNF_FIT_NOT_CONVERGED (2)  the iteration cap was reached before |d - grad c(s)|_inf <= 5e-14: the last iterate;
 *   RNF_FIT_INPUT (4)          d more than 1e-5 outside that tetrahedron, or a non-finite moment: every output of the row is NaN.
 * moments = 0 gives A = 0 exactly.  The moments are fp64 because rounding d to fp32 moves s by ~6e-8 / lambda_min(H), which reaches
 * 4e-3 at s = (300, 200, 100).  Stream-ordered, no host synchronisation, capturable in a HIP graph. */
#define RNF_FIT_CAPPED 1
#define RNF_FIT_NOT_CONVERGED 2
#define RNF_FIT_INPUT 4
typedef struct RnfFisherFit {
    size_t struct_bytes;        /* sizeof(RnfFisherFit); any other value is refused */
    const double *moments;      /* dev double[B][9] row-major */
    int64_t B;                  /* >= 0 (0 is a no-op) */
    double max_concentration;   /* 0 < cap <= 3e4 (the range rnf_fisher_exact is tested on) */
    int32_t max_iterations;     /* 0: the library's cap of 64 Newton iterations; 1..64: a smaller one */
    float *A_out;               /* dev float[B][9] row-major */
    double *s_out;              /* dev double[B][3] the proper singular values of A, or NULL */
    double *hessian_out;        /* dev double[B][6]: H at s as (00, 01, 02, 11, 12, 22), or NULL */
    int32_t *iterations_out;    /* dev int32[B] Newton iterations used, or NULL */
    int32_t *status_out;        /* dev int32[B], or NULL */
    void *stream;
} RnfFisherFit;
int rnf_fisher_fit(const RnfFisherFit *fit);

/* EM for a K-component mixture of matrix-Fishers per group of rotations (csrc/fisher_mixture.h), w.r.t. the Haar probability measure:
 *   log p(R) = logsumexp_k( log_pi_k + tr(A_k^T R) - c(A_k) ),   c the exact log-normaliser of rnf_fisher_exact.
 * Rows, weights, groups and shared_rotations as RnfRotationMoments.  One iteration: responsibilities r_ik in fp64 from the fp32 inputs,
 * pi_k = sum_i w_i r_ik, M_k = sum_i w_i r_ik R_i / pi_k, A_k = the fit of rnf_fisher_fit to M_k rounded to fp32, c_k from the rounded
 * A_k.  The state between iterations is exactly (A_out fp32, log_pi_out fp64): a call with iterations = T equals T chained calls with
 * iterations = 1 (tol = 0), bit for bit; A_init may be A_out and log_pi_init may be log_pi_out.  Sums in the fixed order of
 * rnf_rotation_moments: a group's outputs do not depend on G, its position or shared_rotations, and for K = 1 one iteration gives the
 * A, s and status of rnf_rotation_moments + rnf_fisher_fit bit for bit.
 * A group stops once 0 <= L_t - L_(t-1) <= tol (tol = 0: every iteration runs), L_t = sum_i w_i log p(R_i) under the parameters before
 * iteration t.  status_out per component: the RNF_FIT_* bits of its last solve (CAPPED is legitimate: a component that collapses onto
 * one row is bounded by max_concentration), or RNF_MIX_EMPTY: log_pi = -inf on entry or pi_k underflowed to 0 -- the component keeps
 * its A, has log_pi = -inf and adds an exact +0.0 to every sum.  A group whose weights are all -inf, that holds a NaN, or whose
 * components are all empty is NaN in every output with status RNF_FIT_INPUT; only that group.
 * 2 * iterations + 3 launches (+ 1 with log_weights) whatever the data: stream-ordered, no host synchronisation, no atomics,
 * capturable in a HIP graph as a linear chain. */
#define RNF_MIX_EMPTY 8
typedef struct RnfFisherMixtureFit {
    size_t struct_bytes;        /* sizeof(RnfFisherMixtureFit); any other value is refused */
    const float *rotations;     /* dev float[G][n][9] row-major, or float[n][9] with shared_rotations */
    const float *log_weights;   /* dev float[G][n], or NULL (w = 1/n) */
    int64_t n;                  /* rotations per group, 1..2^40 */
    int64_t G;                  /* groups, >= 1; G * ceil(n / 4096) <= 2^31 - 1 */
    int32_t shared_rotations;   /* 0, or 1: rotations is [n][9] for every group (needs log_weights) */
    int32_t K;                  /* components, 1..8 */
    const float *A_init;        /* dev float[G][K][9] */
    const double *log_pi_init;  /* dev double[G][K], or NULL: uniform, log(1/K) */
    int32_t iterations;         /* 1..256 */
    double tol;                 /* >= 0 */
    double max_concentration;   /* 0 < cap <= 3e4, as RnfFisherFit */
    float *A_out;               /* dev float[G][K][9] */
    double *log_pi_out;         /* dev double[G][K] */
    double *s_out;              /* dev double[G][K][3]: the proper singular values of the component's last solve (NaN before one), or NULL */
    double *loglik_out;         /* dev double[G][iterations + 1]: entry t = L before iteration t, the last used one = L of the outputs, then NaN */
    double *weight_entropy_out; /* dev double[G]: -sum_i w_i log w_i, or NULL */
    float *log_resp_out;        /* dev float[G][K][n]: log r_ik under the outputs, or NULL */
    int32_t *status_out;        /* dev int32[G][K] */
    int32_t *iterations_out;    /* dev int32[G]: EM iterations run */
    void *workspace;            /* dev scratch, 8-byte aligned, of at least rnf_fisher_mixture_fit_workspace_bytes(this struct) bytes */
    size_t workspace_bytes;
    void *stream;
} RnfFisherMixtureFit;
int rnf_fisher_mixture_fit(const RnfFisherMixtureFit *fit);
/* 8 * (G * ceil(n / 4096) * (10 K + 14) + G * K + G) bytes; 0 when struct_bytes, n, G, K or iterations are out of range. */
size_t rnf_fisher_mixture_fit_workspace_bytes(const RnfFisherMixtureFit *fit);

/* log p of n rotations under ONE fitted mixture -- A_dev float[K][9], log_pi_dev double[K], rotation_dev float[n][9] -> logp_out_dev
 * float[n] and, unless NULL, log_resp_out_dev float[K][n] (log responsibilities) -- by the row function of the E-step above.  K in 1..8;
 * a component with log_pi = -inf is left out (log r = -inf).  n = 0 is a no-op.  Stream-ordered, capturable; no gradient. */
int rnf_fisher_mixture_log_prob(const float *A_dev, const double *log_pi_dev, int32_t K, const float *rotation_dev, int64_t n,
                                float *logp_out_dev, float *log_resp_out_dev, void *stream);

/* Gradient of MatrixFisherN._log_prob w.r.t. A (agent.py:57-65 keeps a network-predicted A in the autograd graph; the reference
 * differentiates torch.svd, utils/fisher.py:67-76,217-232):  g_A[b] = sum_i g_logp[i] R_i - (sum_i g_logp[i]) dc/dA_b over the n/B
 * samples of row b, dc/dA = U' diag(dc/ds) V'^T on the proper SVD (csrc/fisher_math.h), plus the batch coupling of norm_type 0.
 * rotation_dev float[n][9], g_A_dev float[B][9] (overwritten), scratch_dev: rnf_fisher_scratch_bytes(B) bytes.  fp64 accumulation.
 * norm_type 0, 1 or RNF_FISHER_NORM_EXACT (dc/dA = E[R], smooth at repeated and cancelling singular values). */
int rnf_fisher_log_prob_backward_param(const float *g_logp_dev, const float *rotation_dev, int64_t n, const float *A_dev, int64_t B,
                                   int32_t norm_type, void *scratch_dev, size_t scratch_bytes, float *g_A_dev, void *stream);

/* Gradient of rnf_fisher_log_prob w.r.t. the rotations (training with a matrix-Fisher base, agent.py:58-64):
 * g_rotation[i] = g_logp[i] * A[i / (n/B)]. */
int rnf_fisher_log_prob_backward(const float *g_logp_dev, int64_t n, const float *A_dev, int64_t B, float *g_rotation_dev,
                                 void *stream);

/* pytorch3d.transforms.matrix_to_quaternion as the reference calls it on sampled rotations (utils/fisher.py:242-243, context = 4) and
 * inside calculate_16 (flow/squeezetrans.py:34): rotation_dev float[n][9] -> quaternion_dev float[n][4], real part first, the candidate
 * with the largest component (published 0.7.5 rule). */
int rnf_matrix_to_quaternion(const float *rotation_dev, int64_t n, float *quaternion_dev, void *stream);

/* MatrixFisherN._sample (utils/fisher.py:117-207,234-243): n rotations per row of A, out [B,n,3,3].
 *   U_dev, V_dev [B,3,3]: proper SVD factors of A (det +1; utils/fisher.py:53-64); lam_dev [B,4]: the diagonal Bingham parameter
 *   (0, 2(S1+S2), 2(S0+S2), 2(S0+S1)) (utils/fisher.py:183-187).  Counter-based Philox stream keyed by `seed`: the same seed gives
 *   the same samples; parity with the reference's torch-generator samples is statistical.  fail_flag_dev (must point to one zeroed int32) is set to 1 if any sample exhausted its 4096 proposals. */
int rnf_fisher_sample(const float *U_dev, const float *V_dev, const float *lam_dev, int64_t B, int64_t n, uint64_t seed,
                      float *out_dev, int32_t *fail_flag_dev, void *stream);

/* ConditionalTransform.forward for one packed Moebius layer (flow/condition.py:24-30), unconditional input only:
 * y_dev [n,3] -> out_dev [n,4K] in the reference's output order.  Unit-test / bring-up entry point. */
int rnf_conditioner_forward(const float *y_dev, int64_t n, const float *layer_packed_dev, int32_t segments,
                            int32_t precision, float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* RNF_HIP_H */
