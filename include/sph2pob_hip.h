/*
 * sph2pob_hip.h — C ABI of libsph2pob_hip.so: the MI355X (gfx950) Sph2Pob spherical-IoU engine.
 *
 * The reference (ManuelVeras/sph-retina) has no FFI of its own: its hot path is Python that calls torch
 * element-wise ops plus three compiled mmcv-full 1.6.0 ops.  Each entry point below names the reference
 * interface it replaces (paths relative to the reference checkout).  A maintainer binds these from Python
 * with ctypes; no torch types cross this boundary.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM) unless stated; row-major, contiguous, fp32 ("f32") / int64
 *   - boxes are degrees: BFoV (theta, phi, alpha, beta) box_dim = 4; RBFoV (+gamma) box_dim = 5
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream); launchers only ENQUEUE:
 *     no allocation, no synchronisation, no ownership transfer, inputs are never written
 *   - return value: 0 on success, a negative SPH2POB_ERR_* for bad arguments, or a positive hipError_t
 */
#ifndef SPH2POB_HIP_H
#define SPH2POB_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* transform variant: sphdet/iou/sph_iou_api.py:91-98 (sph2pob_{standard,efficient,legacy}_iou) */
enum { SPH2POB_VARIANT_STANDARD = 0, SPH2POB_VARIANT_EFFICIENT = 1, SPH2POB_VARIANT_LEGACY = 2,
       /* the cheap approximate backends of SphOverlaps2D (sphdet/iou/sph_iou_api.py:128-175; BFoV, mode 'iou' only):
        * Sph-IoU and FoV-IoU closed forms of sphdet/iou/approximate_ious.py:3-54 — SURVEY §8f-4 */
       SPH2POB_VARIANT_SPH_IOU = 3, SPH2POB_VARIANT_FOV_IOU = 4,
       /* Unbiased IoU: exact spherical-polygon intersection area, BFoV and RBFoV, mode 'iou' only —
        * sphdet/iou/sph_iou_api.py:103-126 over unbiased_iou_bfov.py:4-204 / unbiased_iou_rbfov.py:4-182 (numpy on the
        * CPU in the reference; the default backend of SphOverlaps2D and an SphNMS calculator, sph_nms.py:11-12).
        * Double precision on the device.  With SPH2POB_FLAG_REFERENCE_ORDER it also reproduces the fp32 roundings
        * numpy applies to fp32 inputs (noisier: the reference's fp32 areas cancel catastrophically on small boxes). */
       SPH2POB_VARIANT_UNBIASED = 5,
       /* Naive IoU: planar IoU of the boxes in ERP pixel space (sph_iou_api.py:179-197; sph_nms.py:13-14), BFoV via
        * axis-aligned boxes, RBFoV via rotated boxes; no jitter, mode 'iou' only */
       SPH2POB_VARIANT_NAIVE = 6 };
/* OR-ed into `variant`: evaluate the transform in the reference's own fp32 operation order (bit-for-bit the
 * arithmetic of sph2pob_standard.py / sph2pob_efficient.py, ~3x the VALU work) instead of the closed-form core.
 * Both meet the parity bar on the benchmark distribution; on close-centre pairs the closed-form core is ~10x
 * closer to fp64 truth, the reference-order path ~3x closer to the reference's own fp32 rounding. */
enum { SPH2POB_FLAG_REFERENCE_ORDER = 0x100,
       /* accepted and ignored: round 1's opt-in near-parallel safeguard (pairs whose planar boxes the reference's two jitter
        * steps leave parallel to < 2.5e-4 rad take a first-order form without 1/sin(delta)) is part of every closed-form
        * kernel since round 2 */
       SPH2POB_FLAG_ROBUST_PARALLEL = 0x200,
       /* SPH2POB_VARIANT_NAIVE only: Sph2PlanarBoxTransform('sph2tan') instead of 'sph2pix' (naive_iou(box_formator=...),
        * sphdet/iou/sph_iou_api.py:179, sphdet/bbox/box_formator.py:98-106, :166-172) */
       SPH2POB_FLAG_NAIVE_TAN = 0x400 };
/* mode: sphdet/iou/sph_iou_api.py:49 ('iou' | 'iof') */
enum { SPH2POB_MODE_IOU = 0, SPH2POB_MODE_IOF = 1 };
/* rbb_edge: sphdet/iou/sph2pob_standard.py:110-118 */
enum { SPH2POB_EDGE_ARC = 0, SPH2POB_EDGE_CHORD = 1, SPH2POB_EDGE_TANGENT = 2 };
/* rbb_angle: sphdet/iou/sph2pob_standard.py:88-108 */
enum { SPH2POB_ANGLE_EQUATOR = 0, SPH2POB_ANGLE_PROJECT = 1 };
/* loss mode: sphdet/losses/sph2pob_iou_loss.py:19 */
enum { SPH2POB_LOSS_IOU = 0, SPH2POB_LOSS_GIOU = 1, SPH2POB_LOSS_DIOU = 2, SPH2POB_LOSS_CIOU = 3 };

enum {
    SPH2POB_OK = 0,
    SPH2POB_ERR_NULL = -1,    /* a required pointer is NULL while the element count is > 0 */
    SPH2POB_ERR_DIM = -2,     /* box_dim not in {4, 5}, or legacy variant with box_dim 5 (reference raises) */
    SPH2POB_ERR_OPTION = -3,  /* variant / mode / edge / angle / loss mode out of range */
    SPH2POB_ERR_SIZE = -4     /* negative count or a product that overflows the launch geometry */
};

/* Library identification: ABI version (bumped when the signature or the meaning of an existing entry point changes; purely
 * additive entry points — the _h16 family below — do not bump it: a caller detects them by symbol.  sph2pob_abi_version() returns
 * the value the library was built with) and the code-object target. */
#define SPH2POB_ABI_VERSION 6
int sph2pob_abi_version(void);
const char* sph2pob_target_arch(void);
const char* sph2pob_error_string(int code);

/*
 * Aligned Sph2Pob IoU: out[i] = clamp(IoU(b1[i], b2[i]), 0, 1), i < n.
 * Replaces _sph2pob_iou_auxiliary(..., is_aligned=True) = jitter -> transform -> jitter -> mmcv
 * box_iou_rotated -> clamp: sphdet/iou/sph_iou_api.py:48-86 (and the wrappers at :91-98).
 * b1, b2: (n, box_dim) f32; out: (n) f32.  Algorithmic HBM traffic: 2*4*box_dim + 4 bytes per pair.
 */
/* Precondition (b1, b2): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_iou_aligned_f32(const float* b1, const float* b2, float* out, int64_t n, int box_dim, int variant,
                            int mode, int edge, int angle, void* stream);

/*
 * Pairwise Sph2Pob IoU: out[i*n + j] = clamp(IoU(b1[i], b2[j]), 0, 1); rows = first argument, exactly the
 * (rows, cols) view of sphdet/iou/sph_iou_api.py:59-64,85 without materialising the m*n expanded pairs.
 * This is the call MaxIoUAssigner makes: overlaps = iou_calculator(gt_bboxes, bboxes)
 * (mmdet/core/bbox/assigners/max_iou_assigner.py:113).
 */
/* Precondition (b1, b2): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_iou_pairwise_f32(const float* b1, int64_t m, const float* b2, int64_t n, float* out, int box_dim,
                             int variant, int mode, int edge, int angle, void* stream);

/*
 * Planar oriented boxes of both roles, (n, 5) f32 each = (x, y, w, h, a[rad]); with jitter != 0 the spherical
 * and rotated jitters are applied around the transform exactly as Sph2PobTransfrom.new_forward does
 * (sphdet/losses/sph2pob_transform.py:26-30) — the shared front end of every Sph2Pob-wrapped OBB loss.
 * Replaces sph2pob_{standard,efficient,legacy}(sph_gt, sph_pred, rbb_angle_version='rad', ...):
 * sphdet/iou/sph2pob_standard.py:8-80, sph2pob_efficient.py:9-73, sph2pob_legacy.py:8-31.
 * variant: STANDARD, EFFICIENT or LEGACY (BFoV only); any other variant returns SPH2POB_ERR_OPTION.
 */
/* Precondition (b1, b2): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_transform_f32(const float* b1, const float* b2, float* planar1, float* planar2, int64_t n,
                          int box_dim, int variant, int edge, int angle, int jitter, void* stream);

/*
 * Adjoint of sph2pob_transform_f32 for variant STANDARD | EFFICIENT, rbb_angle 'equator': given the gradients of a
 * scalar w.r.t. the two (n, 5) planar boxes, writes its gradients w.r.t. the two (n, box_dim) spherical boxes
 * (degrees).  This is what lets every Sph2Pob-wrapped OBB loss (Sph2PobTransfrom.new_forward,
 * sphdet/losses/sph2pob_transform.py:24-35: L1 / GD / KF / IoU bodies) back-propagate to the spherical inputs without
 * torch autograd through the ~70 transform ops.  With jitter != 0 the clamp gates of both jitters are applied.
 * Any variant other than STANDARD or EFFICIENT returns SPH2POB_ERR_OPTION.
 */
/* Precondition (b1, b2): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_transform_bwd_f32(const float* b1, const float* b2, const float* grad_planar1, const float* grad_planar2,
                              float* grad_b1, float* grad_b2, int64_t n, int box_dim, int variant, int edge, int jitter,
                              void* stream);

/*
 * The same adjoint for the transforms without a closed-form backward here — sph2pob_legacy (BFoV only) and
 * rbb_angle = 'project' of sph2pob_standard / sph2pob_efficient (sphdet/iou/sph2pob_legacy.py:8-31,
 * sph2pob_standard.py:88-108, sph2pob_efficient.py:81-97: the reference differentiates them with torch autograd) — by
 * forward-mode differentiation of the reference-order transform (2 * box_dim passes on (value, derivative) pairs).
 * jitter != 0: the adjoint of jitter_spherical -> transform -> jitter_rotated (Sph2PobTransfrom('sph2pob_legacy'),
 * sphdet/losses/sph2pob_transform.py:12-16, :28-30).
 */
/* Precondition (b1, b2): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_transform_bwd_general_f32(const float* b1, const float* b2, const float* grad_planar1,
                                      const float* grad_planar2, float* grad_b1, float* grad_b2, int64_t n, int box_dim,
                                      int variant, int edge, int angle, int jitter, void* stream);

/*
 * Planar rotated-rectangle IoU on GIVEN planar boxes (x, y, w, h, a [rad]) — the op the reference obtains from mmcv
 * (`mmcv.ops.box_iou_rotated`, call sites sphdet/iou/sph_iou_api.py:79, :193; the vendored value-equivalent
 * `diff_iou_rotated_2d`, sphdet/iou/diff_iou_rotated.py:325-343, called directly by tests/test_all_ious.py:22-24).
 * aligned != 0: out[i] = IoU(p1[i], p2[i]), m == n; aligned == 0: out[i * n + j] = IoU(p1[i], p2[j]) (rows = p1).
 * mode: SPH2POB_MODE_IOU | SPH2POB_MODE_IOF.  No jitter and no clamp (as the mmcv op): exactly parallel edges are
 * handled by the boundary integral's clamped reciprocals, nearly parallel ones (|sin| < 2.5e-4) in double.
 */
int sph2pob_planar_iou_f32(const float* p1, int64_t m, const float* p2, int64_t n, float* out, int aligned, int mode,
                           void* stream);

/*
 * Sph2PobIoULoss element values: loss[i] = scale * w_i * L(pred[i], target[i]), L = 1 - IoU | GIoU | DIoU | CIoU
 * form; scale carries loss_weight (sph2pob_iou_loss.py:49).
 * Replaces Sph2PobTransfrom.new_forward (sphdet/losses/sph2pob_transform.py:24-35: clone, spherical jitter,
 * sph2pob_standard(..., 'rad'), rotated jitter) + obb_iou_loss (sphdet/losses/sph2pob_iou_loss.py:104-196, whose
 * IoU is mmcv diff_iou_rotated_2d, :122) + the element-weight step of weight_reduce_loss
 * (mmdet/models/losses/utils.py:44-45).  weight: NULL, (n) [weight_dim 1] or (n, box_dim) [weight_dim box_dim:
 * the per-box mean is taken as OBBIoULoss.forward does, sph2pob_iou_loss.py:43-48].  iou (optional, may be NULL)
 * receives the clamped planar IoU.  eps = the loss's eps (default 1e-6, sph2pob_iou_loss.py:17).
 */
/* Precondition (pred, target): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_loss_fwd_f32(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                         float* loss, float* iou, int64_t n, int box_dim, int loss_mode, float eps, void* stream);

/*
 * Adjoint of the above w.r.t. the spherical inputs (degrees): grad_pred[i,:] = g_i * dL_i/dpred[i,:], likewise
 * grad_target (optional, may be NULL), with g_i = grad_out[i * grad_stride] * scale * w_i  (grad_stride 0 =
 * one scalar upstream gradient, e.g. of a 'mean'/'sum' reduced loss; 1 = per element, reduction 'none').
 * Replaces torch autograd through the ~150 ops the reference records for this loss.  Recomputes the forward in
 * registers: reads only pred, target, weight and grad_out.
 */
/* Precondition (pred, target, grad_pred, grad_target): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_loss_bwd_f32(const float* pred, const float* target, const float* weight, int weight_dim,
                         const float* grad_out, int grad_stride, float scale, float* grad_pred, float* grad_target,
                         int64_t n, int box_dim, int loss_mode, float eps, void* stream);

/*
 * The same loss REDUCED in one go: out[0] = scale * sum_i w_i * L(pred[i], target[i]) — the forward kernel leaves one
 * partial sum per workgroup in `workspace` (no element buffer is written or re-read), a second launch adds the partials
 * in a fixed order (bitwise reproducible, no float atomics).  scale carries loss_weight and the 1 / n | 1 / (avg_factor +
 * eps) of weight_reduce_loss (mmdet/models/losses/utils.py:47-58).  workspace: device buffer of at least
 * sph2pob_loss_sum_workspace_floats(n) floats.  Backward: sph2pob_loss_bwd_f32 with grad_stride 0 and the same scale.
 */
int64_t sph2pob_loss_sum_workspace_floats(int64_t n);
/* Precondition (pred, target): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_loss_fwd_sum_f32(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                             float* out, float* workspace, int64_t n, int box_dim, int loss_mode, float eps,
                             void* stream);

/*
 * Forward AND gradients in one pass (the training call: the backward kernel recomputes the whole forward, so when the
 * gradient will be asked for anyway the loss value is a by-product of it): writes the loss elements (loss, may be NULL)
 * and / or their sum (out_sum + workspace as in sph2pob_loss_fwd_sum_f32, may be NULL), and
 *     grad_pred[i, :]   = scale * w_i * dL_i / dpred[i, :]        (n, box_dim)
 *     grad_target[i, :] = scale * w_i * dL_i / dtarget[i, :]      (optional, may be NULL)
 * i.e. the gradients for an upstream gradient of 1.  torch's backward then only scales them:
 * sph2pob_loss_grad_scale_f32: out[i, :] = stash[i, :] * grad_out[i * grad_stride]  (grad_stride 0: one scalar).
 * out may be the stash itself (in place); in place with a scalar upstream gradient of exactly 1.0 — a plain
 * `loss.backward()` — the launch returns after one scalar load per workgroup: the stash already is the gradient.
 */
/* Precondition (pred, target, grad_pred, grad_target; sph2pob_loss_grad_scale_f32 reads and writes one element at a time): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_loss_fwd_grad_f32(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                              float* loss, float* out_sum, float* workspace, float* grad_pred, float* grad_target,
                              int64_t n, int box_dim, int loss_mode, float eps, void* stream);
int sph2pob_loss_grad_scale_f32(const float* stash, const float* grad_out, int grad_stride, float* out, int64_t n,
                                int box_dim, void* stream);

/*
 * Sph2PobGDLoss / Sph2PobKFLoss: mmrotate's Gaussian-distance (gaussian_dist_loss.py) and KFIoU (kf_iou_loss.py) bodies
 * on the Sph2Pob planar boxes (the same front end as the IoU family: spherical jitter, sph2pob_standard(..., 'rad'),
 * rotated jitter), box X -> N((x, y), R(a) diag(w^2/4, h^2/4) R(a)^T) with w, h clamped to [1e-7, 1e7].  The bodies are
 * restated from mmrotate 0.3.2's published source (parity unpinned).  Per element, P = planar pred, T = planar target:
 *   GWD        d = sqrt(max(|mu_P - mu_T|^2 + alpha^2 * (tr S_P + tr S_T - 2 sqrt(max(tr(S_P S_T) + 2t, 1e-7))), 1e-7)),
 *              t = sqrt(max(det S_P det S_T, 1e-7)); OPT_NORMALIZE divides by 2 t^(1/4) (with mmrotate's clamps)
 *   KLD        d = KL(P || T)-like kld_loss with alpha (P is the reference Gaussian); OPT_SQRT: sqrt(max(d, 1e-7))
 *   JD         d = (kld(P, T) + kld(T, P)) / 2 before the sqrt; OPT_SQRT as KLD
 *   KLD_SYMMAX / KLD_SYMMIN   d = max | min of kld(P, T), kld(T, P), each after the OPT_SQRT step
 *   GD result: post(d) = [log1p(d) | sqrt(max(d, 1e-7)) | d], then 1 - 1 / (tau + .) if tau >= 1
 *   KF         loss = max(smoothL1_beta(|mu_P - mu_T|) summed over x, y + kf, 0), kf = 1 - KFIoU | -ln(KFIoU + eps) |
 *              exp(1 - KFIoU) - 1, KFIoU = Vb / (Vb_P + Vb_T - Vb + eps), Vb = 4 sqrt(det) of S_T - S_T (S_T + S_P)^-1 S_T
 *              (in closed form: always positive, where mmrotate's fp32 matrix inverse can give NaN)
 * type_flags: SPH2POB_GAUSS_* | SPH2POB_FLAG_REFERENCE_ORDER (reference-order front end).  fun: SPH2POB_GAUSS_FUN_NONE |
 * LOG1P | SQRT for the GD types, NONE | LN | EXP for KF.  opts: SPH2POB_GAUSS_OPT_* (KF ignores them, GWD reads NORMALIZE,
 * the kld family SQRT).  tau / alpha: GD only; beta / eps: KF only.  Every clamp gates the gradient as torch.clamp does.
 * The four entry points have the contracts of their sph2pob_loss_* counterparts (weights, scale, the deterministic sum,
 * grad_stride, the one-pass form + sph2pob_loss_grad_scale_f32, sph2pob_loss_sum_workspace_floats workspace).
 */
enum { SPH2POB_GAUSS_GWD = 0, SPH2POB_GAUSS_KLD = 1, SPH2POB_GAUSS_JD = 2, SPH2POB_GAUSS_KLD_SYMMAX = 3,
       SPH2POB_GAUSS_KLD_SYMMIN = 4, SPH2POB_GAUSS_KF = 5 };
enum { SPH2POB_GAUSS_FUN_NONE = 0, SPH2POB_GAUSS_FUN_LOG1P = 1, SPH2POB_GAUSS_FUN_SQRT = 2, SPH2POB_GAUSS_FUN_LN = 3,
       SPH2POB_GAUSS_FUN_EXP = 4 };
enum { SPH2POB_GAUSS_OPT_SQRT = 1, SPH2POB_GAUSS_OPT_NORMALIZE = 2 };
/* Precondition (pred, target, grad_pred, grad_target of the four sph2pob_gauss_loss entries): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_gauss_loss_fwd_f32(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                               float* loss, int64_t n, int box_dim, int type_flags, int fun, float tau, float alpha,
                               int opts, float beta, float eps, void* stream);
int sph2pob_gauss_loss_bwd_f32(const float* pred, const float* target, const float* weight, int weight_dim,
                               const float* grad_out, int grad_stride, float scale, float* grad_pred, float* grad_target,
                               int64_t n, int box_dim, int type_flags, int fun, float tau, float alpha, int opts,
                               float beta, float eps, void* stream);
int sph2pob_gauss_loss_fwd_sum_f32(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                                   float* out, float* workspace, int64_t n, int box_dim, int type_flags, int fun, float tau,
                                   float alpha, int opts, float beta, float eps, void* stream);
int sph2pob_gauss_loss_fwd_grad_f32(const float* pred, const float* target, const float* weight, int weight_dim,
                                    float scale, float* loss, float* out_sum, float* workspace, float* grad_pred,
                                    float* grad_target, int64_t n, int box_dim, int type_flags, int fun, float tau,
                                    float alpha, int opts, float beta, float eps, void* stream);

/*
 * out[0] = scale * sum(x[0..n)) — deterministic two-pass tree (bitwise reproducible, no float atomics); the
 * reduction step of weight_reduce_loss (mmdet/models/losses/utils.py:47-55).  workspace: device buffer of at
 * least sph2pob_sum_workspace_floats() floats.
 */
int sph2pob_sum_workspace_floats(void);
int sph2pob_sum_f32(const float* x, int64_t n, float scale, float* out, float* workspace, void* stream);

/*
 * Greedy per-class NMS with the Sph2Pob IoU as overlap: keep[i] = 1 iff sorted box i survives.
 * Replaces sph_nms_op (sphdet/bbox/nms/sph_nms.py:62-74: python while-loop, one full IoU pipeline + host sync per
 * kept box) for every class at once.  Input boxes must be sorted by (class ascending, score descending);
 * cls_sorted may be NULL (class-agnostic).  A box j is suppressed by an earlier kept box i of the same class when
 * IoU(box_i as bboxes1, box_j as bboxes2) > iou_threshold (`iou <= thr` keeps, :72).  variant: EFFICIENT (what
 * SphNMS('sph2pob_efficient') uses, sph_nms.py:9-10) or STANDARD.  k <= sph2pob_nms_max_boxes();
 * workspace: device buffer of sph2pob_nms_workspace_bytes(k) bytes (the k x ceil(k/64) suppression bit-matrix).
 */
int sph2pob_nms_max_boxes(void);
int64_t sph2pob_nms_workspace_bytes(int64_t k);
/* Precondition (boxes_sorted): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_nms_f32(const float* boxes_sorted, const int64_t* cls_sorted, int64_t k, int box_dim, int variant,
                    float iou_threshold, void* workspace, unsigned char* keep, void* stream);
/* Same with a caller-supplied bound on the largest class segment (boxes of one class): the suppression matrix is then
 * k x min(max_segment / 64 + 2, 512) words instead of k x k / 64, and k itself is unbounded (< 2^31); max_segment <=
 * sph2pob_nms_max_boxes() (32 704: such a segment spans at most 512 words at any offset).  cls_sorted == NULL means one segment (max_segment >= k).  Under-stating max_segment
 * truncates suppression for the over-long segment (never an out-of-bounds access).  multiclass_nms hands ALL
 * (box, class) candidates above score_thr to the NMS (sphdet/bbox/nms/utils.py:6-15): 5 000 boxes x 37 classes is
 * beyond the one-matrix limit of sph2pob_nms_f32 but ~1 700 per class. */
int64_t sph2pob_nms_segmented_workspace_bytes(int64_t k, int64_t max_segment);
/* Precondition (boxes_sorted): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_nms_segmented_f32(const float* boxes_sorted, const int64_t* cls_sorted, int64_t k, int box_dim, int variant,
                              float iou_threshold, int64_t max_segment, void* workspace, unsigned char* keep,
                              void* stream);

/*
 * sph_batched_nms without the host (sphdet/bbox/nms/sph_nms.py:22-60): UNSORTED boxes (k, box_dim), scores (k), class ids
 * idxs (k, int64; NULL = one class: sph_nms_op, :62-74) -> the kept boxes' original indices in descending-score order
 * (ties by ascending index), at most max_num of them, and dets = (box, score) rows of box_dim + 1 floats.  Four launches,
 * no host work: a one-workgroup bitonic sort of composite (class | -score | index) keys in LDS, the suppression matrix,
 * the per-class sweeps, and a one-workgroup sort of the kept boxes by score.  *status (device int) = number of rows written
 * to keep / dets, or -1 when a class id is outside [0, 262 143] (nothing valid was written: use the sorted-input entry
 * points).  k <= sph2pob_batched_nms_max_boxes() (16 384), any number per class.  keep / dets must hold min(max_num, k) rows;
 * workspace: sph2pob_batched_nms_workspace_bytes(k, box_dim) bytes, no initialisation.
 */
int sph2pob_batched_nms_max_boxes(void);
int64_t sph2pob_batched_nms_workspace_bytes(int64_t k, int box_dim);
/* Precondition (boxes): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_batched_nms_f32(const float* boxes, const float* scores, const int64_t* idxs, int64_t k, int box_dim, int variant,
                            float iou_threshold, int64_t max_num, void* workspace, int64_t* keep, float* dets, int* status,
                            void* stream);

/*
 * Detection post-processing for a whole minibatch: what SphRetinaHead._get_bboxes_single / _bbox_post_process
 * (sphdet/models/heads/sph_retina_head.py:101-216, :22-99) compute per image and level — sigmoid, filter_scores_and_topk
 * (mmdet/core/utils/misc.py:119-165), bbox_coder.decode, cat over the levels, SphNMS, [:max_per_img] — for B images as ten
 * launches whatever B is, nothing read back to the host, nothing allocated: capturable into a hipGraph.
 * Level tables are HOST arrays of num_levels <= 8 entries:
 *   cls_scores   device pointers, level l either the head's NCHW (B, A C, H_l, W_l) or the flattened (B, n_l, C); read in
 *                place.  The logical candidate index of (h, w, a, c) is the reference's ((h W + w) A + a) C + c
 *   bbox_preds   device pointers, laid out like cls_scores: (B, A box_dim, H_l, W_l) or (B, n_l, box_dim)
 *   anchors      device pointers, (n_l, box_dim), shared by the images
 *   level_n      n_l = H_l W_l A anchors;  level_hw: H_l W_l for the NCHW layout, 0 for the flattened one
 *   activation   0: cls_scores are probabilities; 1: logits, score = 1 / (1 + expf(-x)) in fp32 — the score a candidate is
 *                selected on is the score it is reported with
 * Per image and level: a candidate is valid iff score > score_thr (a NaN is dropped); the min(nms_pre, #valid) candidates that
 * come first in (score descending, candidate index ascending) order — torch's stable descending sort — are kept, in that
 * order; their boxes are decoded from their anchor and deltas with the arithmetic of sph2pob_coder_decode_f32 (means_host /
 * stds_host / max_ratio / coder_flags / ctr_clamp as there).  The levels' candidates, concatenated, then go through exactly
 * what sph2pob_batched_nms_f32 does for that image alone (per-class greedy NMS keeping iou <= iou_threshold, the first
 * max_per_img in descending score order, ties by candidate position).
 *   dets         (B, max_per_img, box_dim + 1) f32: box and score; rows from num_dets[b] on are 0
 *   labels       (B, max_per_img) int64, -1 from num_dets[b] on
 *   prior_inds   (B, max_per_img) int64: the detection's anchor as an index into the concatenated levels, -1 padded
 *   num_dets     (B) int64
 *   workspace    sph2pob_get_bboxes_workspace_bytes(level_n, num_levels, B, C, box_dim, nms_pre) bytes, no initialisation
 *                (0 = the shapes are not accepted): histograms, one 8-byte survivor slot per score, the candidate blocks of
 *                K_cap = sum_l min(nms_pre, n_l C) rows per image and B suppression matrices of K_cap^2 / 8 bytes
 * Errors, checked in this order before anything is enqueued: box_dim -> SPH2POB_ERR_DIM; a variant other than STANDARD |
 * EFFICIENT, SPH2POB_FLAG_REFERENCE_ORDER, activation, coder_flags, max_ratio < 0 -> SPH2POB_ERR_OPTION; num_levels outside
 * [1, 8], B outside [1, 65 535], C outside [1, 262 144], nms_pre <= 0, max_per_img < 0 -> SPH2POB_ERR_SIZE; a NULL table ->
 * SPH2POB_ERR_NULL; n_l < 1, n_l C >= 2^31 - 2^17, level_hw that does not divide n_l, K_cap > sph2pob_batched_nms_max_boxes()
 * -> SPH2POB_ERR_SIZE; a NULL table entry, output or workspace -> SPH2POB_ERR_NULL.
 */
int64_t sph2pob_get_bboxes_workspace_bytes(const int64_t* level_n, int num_levels, int64_t num_images, int64_t num_classes,
                                           int box_dim, int64_t nms_pre);
int sph2pob_get_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors,
                           const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                           int64_t num_classes, int box_dim, int activation, float score_thr, int64_t nms_pre,
                           const float* means_host, const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp,
                           int variant, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels,
                           int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream);
/*
 * The same post-processing with every NMS the reference's test configurations select: `variant_flags & 0xff` is STANDARD,
 * EFFICIENT, UNBIASED (SphNMS('unbiased_iou'): the bounding-circle cull first, the fp64 intersection area on its survivors) or
 * NAIVE (SphNMS('naive_iou'); with SPH2POB_FLAG_NAIVE_TAN the 'sph2tan' box formator), and class_agnostic = 1 runs one greedy
 * NMS over all candidates of an image whatever their class (PlanarNMS's default): candidates in (score descending, candidate
 * position ascending) order, one segment; labels / prior_inds are still each detection's own.  Tables, outputs, workspace
 * (sph2pob_get_bboxes_workspace_bytes), launch count and everything else as above; sph2pob_get_bboxes_f32 is this entry
 * restricted to STANDARD | EFFICIENT with class_agnostic = 0.
 * Errors, in the order above with these additions: box_dim -> SPH2POB_ERR_DIM; a variant other than STANDARD | EFFICIENT |
 * UNBIASED | NAIVE, SPH2POB_FLAG_REFERENCE_ORDER or an unknown flag bit, SPH2POB_FLAG_NAIVE_TAN with a variant other than NAIVE,
 * class_agnostic outside {0, 1}, activation, coder_flags, max_ratio < 0 -> SPH2POB_ERR_OPTION; then the sizes, tables and
 * pointers exactly as for sph2pob_get_bboxes_f32.
 */
int sph2pob_test_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors,
                            const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                            int64_t num_classes, int box_dim, int activation, float score_thr, int64_t nms_pre,
                            const float* means_host, const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp,
                            int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                            int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream);

/*
 * MaxIoUAssigner epilogue on a (k, n) overlaps matrix (rows = GT, columns = boxes), SURVEY §8f-1.
 * Replaces assign_wrt_overlaps (mmdet/core/bbox/assigners/max_iou_assigner.py:135-220) for k > 0, n > 0:
 *   max_overlaps, argmax_overlaps       = overlaps.max(dim=0)   (:171)   first maximal index on ties
 *   gt_max_overlaps, gt_argmax_overlaps = overlaps.max(dim=1)   (:174)
 *   assigned_gt_inds: -1; 0 where neg_iou_lo <= max < neg_iou_hi (:178-185); argmax + 1 where max >= pos_iou_thr
 *   (:188-189); low-quality matching (:200-207) for i ascending — the reference's python loop costs one host sync
 *   per GT.  assigned_labels (optional) = gt_labels[gt_ind - 1] or -1 (:209-216).
 * workspace: sph2pob_assign_workspace_bytes(k, n) bytes.
 */
int64_t sph2pob_assign_workspace_bytes(int64_t k, int64_t n);
int sph2pob_assign_f32(const float* overlaps, int64_t k, int64_t n, float pos_iou_thr, float neg_iou_lo,
                       float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                       const int64_t* gt_labels, float* max_overlaps, int64_t* argmax_overlaps, float* gt_max_overlaps,
                       int64_t* gt_argmax_overlaps, int64_t* assigned_gt_inds, int64_t* assigned_labels, void* workspace,
                       void* stream);

/*
 * MaxIoUAssigner.assign FUSED with the pairwise IoU (SURVEY §8f-1 as written: the k x n overlaps are never materialised).
 * Replaces `overlaps = self.iou_calculator(gt_bboxes, bboxes)` + `assign_wrt_overlaps`
 * (mmdet/core/bbox/assigners/max_iou_assigner.py:113, :135-220) for the closed-form sph2pob_standard_iou /
 * sph2pob_efficient_iou calculators (variant STANDARD | EFFICIENT, default arithmetic, rbb_angle 'equator', mode 'iou'):
 * the pairwise kernel keeps per-column and per-row running maxima (first index on ties, like torch.max) while it
 * finishes the pairs — culled pairs are exact zeros — and the finalize pass applies the thresholds and the low-quality
 * step (a GT row is re-evaluated only against a column tile that holds its maximum more than once).  Results are bit-identical to
 * sph2pob_iou_pairwise_f32 followed by sph2pob_assign_f32.
 *   ignore       optional (n) bytes: non-zero = the column's overlaps are -1 (`overlaps[:, ignore_max > thr] = -1`, :115-126)
 *   overlaps     optional (k, n): also write the matrix (for callers that want it; the assignment does not read it)
 *   gt_keys      (k) int64, the exchange format of the sharded form: per-GT (max IoU, first global column) as keys that
 *                order as SIGNED integers (torch.distributed / RCCL have no unsigned MAX)
 *   col_offset   global index of this shard's first column (0 when not sharded)
 *   workspace    sph2pob_iou_assign_workspace_bytes(k, n) bytes of scratch (per-chunk column partials, per-tile row
 *                partials): no initialisation, but untouched between reduce and finalize
 *   state        sph2pob_iou_assign_state_bytes(k, n) bytes (per-GT accumulators + arrival counters) that must be ZERO when a
 *                call is enqueued and are left zero by every completed call (one-call form: by the finalize pass; reduce: by
 *                its key pass): zero the buffer once after allocation, then reuse it stream-ordered (its layout moves with
 *                k: a buffer is clean for any (k, n) it is large enough for).  Kept apart from the scratch because the scratch's layout moves with k.
 * sph2pob_iou_assign_f32 = one device, two launches (pairwise kernel with the reductions; finalize).  The two halves exist
 * so that a job sharded on the box axis can put ONE all-reduce(MAX) of the k keys between them:
 * reduce = pairwise kernel + this shard's keys; finalize = column maxima, thresholds, low-quality step against the (global)
 * keys.  Outputs as for sph2pob_assign_f32 (argmax_overlaps, gt_max_overlaps, gt_argmax_overlaps, assigned_labels may be
 * NULL); gt_argmax_overlaps are global column indices.
 * Limits: k <= 262 140, n < 2^31 - 256, col_offset + n < 2^31 - 1.  Other variants / arithmetics: SPH2POB_ERR_OPTION (use
 * the two-call form on the matrix).
 */
int64_t sph2pob_iou_assign_workspace_bytes(int64_t k, int64_t n);
int64_t sph2pob_iou_assign_state_bytes(int64_t k, int64_t n);
/* Precondition (gt, boxes of the three sph2pob_iou_assign entries): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_iou_assign_reduce_f32(const float* gt, int64_t k, const float* boxes, int64_t n, int box_dim, int variant, int edge,
                                  const unsigned char* ignore, int64_t col_offset, float* overlaps, int64_t* gt_keys,
                                  void* workspace, void* state, void* stream);
int sph2pob_iou_assign_finalize_f32(const float* gt, int64_t k, const float* boxes, int64_t n, int box_dim, int variant, int edge,
                                    int64_t col_offset, const int64_t* gt_keys, float pos_iou_thr, float neg_iou_lo,
                                    float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                                    const int64_t* gt_labels, float* max_overlaps, int64_t* argmax_overlaps,
                                    float* gt_max_overlaps, int64_t* gt_argmax_overlaps, int64_t* assigned_gt_inds,
                                    int64_t* assigned_labels, void* workspace, void* stream);
int sph2pob_iou_assign_f32(const float* gt, int64_t k, const float* boxes, int64_t n, int box_dim, int variant, int edge,
                           const unsigned char* ignore, float* overlaps, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi,
                           float min_pos_iou, int match_low_quality, int gt_max_assign_all, const int64_t* gt_labels,
                           float* max_overlaps, int64_t* argmax_overlaps, float* gt_max_overlaps, int64_t* gt_argmax_overlaps,
                           int64_t* assigned_gt_inds, int64_t* assigned_labels, void* workspace, void* state, void* stream);

/*
 * Anchor targets for a whole minibatch: the fused assigner above with the image as a grid dimension, and the target
 * construction of AnchorHead._get_targets_single (mmdet/models/dense_heads/anchor_head.py:254-285 with PseudoSampler) as the
 * finalize pass's epilogue.  Replaces multi_apply(_get_targets_single, ...) over the images (anchor_head.py:202-299, :301-396)
 * for unmap_outputs-free heads (allowed_border = -1: every anchor is valid for every image): two launches for the batch, no
 * (k, n) matrix, nothing read back to the host.
 *   anchors      (n, box_dim), shared by all images
 *   gt           (num_gt, box_dim), the images' GT boxes concatenated; gt_labels (num_gt) int64 or NULL (RPN: label 0)
 *   gt_offsets   (num_images + 1) int64 ON THE DEVICE: image b owns rows gt_offsets[b] .. gt_offsets[b + 1] (it may own none).
 *                The host never reads them: offsets are clamped to [0, num_gt] before use
 *   k_max        HOST upper bound on the GT count of one image (<= num_gt; num_gt itself is always sufficient).  Grid,
 *                workspace and state are sized by it.  An image with more rows than k_max is CLAMPED to its first k_max rows
 *                (the later ones are not assigned): nothing is read or written out of bounds, and nothing is reported
 *   thresholds / match_low_quality / gt_max_assign_all as for sph2pob_iou_assign_f32 (no ignore mask in this form)
 * For image b and anchor j, with g = assigned_gt_inds[b, j] exactly what sph2pob_iou_assign_f32 gives for that image alone
 * (all 0, max_overlaps 0, for an image without GT: max_iou_assigner.py:148-165):
 *   assigned_gt_inds (B, n) int64, max_overlaps (B, n) f32, assigned_labels (B, n) int64 (optional; gt_labels[g - 1] | -1)
 *   labels         (B, n) int64       g > 0: gt_labels[g - 1] (0 when gt_labels is NULL); otherwise num_classes
 *   label_weights  (B, n) f32         g > 0: 1, or pos_weight when pos_weight > 0; g == 0: 1; g == -1: 0
 *   bbox_targets   (B, n, box_dim)    g > 0: the GT box (encode == 0: reg_decoded_bbox=True) or its deltas w.r.t. anchor j
 *                                     (encode != 0: the arithmetic of sph2pob_coder_encode_f32 with means_host / stds_host); else 0
 *   bbox_weights   (B, n, box_dim)    g > 0: 1; else 0
 *   num_pos, num_neg (B) int64        anchors with g > 0 / g == 0 (PseudoSampler's pos_inds / neg_inds)
 *   avg_factor     (1) f32            sum_b max(num_pos[b], 1): mmdet's num_total_pos (anchor_head.py:385) as a device scalar
 *   workspace    sph2pob_anchor_targets_workspace_bytes(num_images, num_gt, k_max, n) bytes of scratch, no initialisation
 *   state        sph2pob_anchor_targets_state_bytes(num_images, k_max, n) bytes, ZERO when a call is enqueued and left zero by
 *                every completed call, as the state of sph2pob_iou_assign_f32 (zero once after allocation, reuse stream-ordered;
 *                clean for any shape it is large enough for)
 * Limits: num_images <= 65 535, k_max <= 262 140, n < 2^31 - 256.  Errors, checked in this order before anything is enqueued:
 * box_dim -> SPH2POB_ERR_DIM; a variant other than STANDARD | EFFICIENT, SPH2POB_FLAG_REFERENCE_ORDER, a bad edge ->
 * SPH2POB_ERR_OPTION; num_images <= 0, num_gt < 0, n <= 0, k_max < 0 or > num_gt, a limit exceeded -> SPH2POB_ERR_SIZE; a NULL
 * among the required pointers (gt, and gt_labels with assigned_labels, only when num_gt > 0; workspace only when k_max > 0) -> SPH2POB_ERR_NULL.
 */
int64_t sph2pob_anchor_targets_workspace_bytes(int64_t num_images, int64_t num_gt, int64_t k_max, int64_t n);
int64_t sph2pob_anchor_targets_state_bytes(int64_t num_images, int64_t k_max, int64_t n);
/* Precondition (anchors, gt, bbox_targets, bbox_weights): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_anchor_targets_f32(const float* anchors, int64_t n, const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets,
                               int64_t num_images, int64_t num_gt, int64_t k_max, int box_dim, int variant, int edge, float pos_iou_thr,
                               float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                               int64_t num_classes, float pos_weight, int encode, const float* means_host, const float* stds_host,
                               int64_t* assigned_gt_inds, float* max_overlaps, int64_t* assigned_labels, int64_t* labels,
                               float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* num_pos, int64_t* num_neg,
                               float* avg_factor, void* workspace, void* state, void* stream);

/*
 * The same call for the calculators without a closed form: LEGACY, SPH_IOU, FOV_IOU (box_dim 4 only), UNBIASED and NAIVE
 * (box_dim 4 or 5; NAIVE with or without SPH2POB_FLAG_NAIVE_TAN).  Two launches for the batch, no (k, n) matrix, nothing read
 * back: phase 1 runs the variant's per-pair function — the one sph2pob_iou_pairwise_f32 runs for it with mode IOU, the given
 * edge and angle EQUATOR in the default arithmetic — on every (GT, anchor) pair (no cull) and keeps the per-anchor and per-GT
 * maxima; phase 2 is the finalize pass of sph2pob_anchor_targets_f32 with that function in its re-evaluation.  Arguments,
 * outputs, limits and the target table are those of sph2pob_anchor_targets_f32, and so are workspace and state: the same two
 * size entries, the same layout, the same zero-before / zero-after contract, so one zeroed state buffer serves both entries
 * alternately.  For image b the outputs are exactly what sph2pob_iou_pairwise_f32 + sph2pob_assign_f32 give for that image alone
 * (same function, same inputs, same bits), provided its overlaps are +0 or positive (no NaN): what every variant returns for
 * valid boxes.
 * Errors, in the order of sph2pob_anchor_targets_f32: box_dim (LEGACY / SPH_IOU / FOV_IOU with box_dim 5 included, as the
 * pairwise entry answers) -> SPH2POB_ERR_DIM; STANDARD | EFFICIENT (they have their own entry), SPH2POB_FLAG_REFERENCE_ORDER, a
 * bad edge -> SPH2POB_ERR_OPTION; then the sizes and the NULL checks.
 */
/* Precondition (anchors, gt, bbox_targets, bbox_weights): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_anchor_targets_any_f32(const float* anchors, int64_t n, const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets,
                                   int64_t num_images, int64_t num_gt, int64_t k_max, int box_dim, int variant, int edge, float pos_iou_thr,
                                   float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                                   int64_t num_classes, float pos_weight, int encode, const float* means_host, const float* stds_host,
                                   int64_t* assigned_gt_inds, float* max_overlaps, int64_t* assigned_labels, int64_t* labels,
                                   float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* num_pos, int64_t* num_neg,
                                   float* avg_factor, void* workspace, void* state, void* stream);

/* ---- box coder: the step immediately in front of the loss when reg_decoded_bbox=True --------------
 * Replaces sphdet/bbox/coder/delta_xywh_sph_bbox_coder.py:116-161 (bbox2delta), :164-263 (delta2bbox) for box_dim 4
 * and sphdet/bbox/coder/delta_xywha_rsph_bbox_coder.py:116-164, :167-268 for box_dim 5 (fifth delta = deg2rad of the
 * gamma difference; decoded gamma clamped to [-90+1e-7, 90-1e-7]).
 *
 * means / stds: HOST pointers to box_dim floats (copied into the kernel arguments; NULL = zeros / ones).
 * encode : deltas[i] = ((gt - proposal) / size, log(size ratio)[, deg2rad(dgamma)] - means) / stds, widths clipped at 1e-7.
 * decode : rois (n, box_dim), deltas (n, num_classes*box_dim) -> boxes (n, num_classes*box_dim);
 *          flags: SPH2POB_CODER_CLIP_BORDER (clamp to the sphere ranges, the reference's clip_border=True),
 *                 SPH2POB_CODER_CTR_CLAMP  (add_ctr_clamp=True: centre shift clamped to +-ctr_clamp, dwh only from above);
 *          max_ratio = |log(wh_ratio_clip)|.
 * decode_bwd: grad_deltas = J^T grad_boxes with the clamp gates of decode (what autograd gives the reference when the
 *          decoded boxes feed Sph2PobIoULoss: sphdet/models/heads/sph_retina_head.py:255-264).
 */
enum { SPH2POB_CODER_CLIP_BORDER = 1, SPH2POB_CODER_CTR_CLAMP = 2 };
/* Precondition (proposals, gt, deltas; rois, deltas, boxes, grad_boxes, grad_deltas of the decode entries): BFoV box arrays (box_dim == 4) must be 16-byte aligned; the Python layer copies a view that is not. */
int sph2pob_coder_encode_f32(const float* proposals, const float* gt, const float* means_host, const float* stds_host,
                             float* deltas, int64_t n, int box_dim, void* stream);
int sph2pob_coder_decode_f32(const float* rois, const float* deltas, const float* means_host, const float* stds_host,
                             float* boxes, int64_t n, int num_classes, int box_dim, float max_ratio, int flags,
                             float ctr_clamp, void* stream);
int sph2pob_coder_decode_bwd_f32(const float* rois, const float* deltas, const float* grad_boxes,
                                 const float* means_host, const float* stds_host, float* grad_deltas, int64_t n,
                                 int num_classes, int box_dim, float max_ratio, int flags, float ctr_clamp,
                                 void* stream);

/* ---- OBB L1 loss body: Sph2PobL1Loss after the Sph2Pob transform ----------------------------------
 * Replaces sphdet/losses/sph2pob_l1_loss.py:28-88 on PLANAR boxes (x, y, w, h, a[rad]) as produced by
 * sph2pob_transform_f32(..., jitter=1):  loss[i,k] = scale * weight[i,k] * |d[i,k]| with
 *   ENCODE: d = bbox2delta(proposals, gt) = ((gx-px)/pw, (gy-py)/ph, log(gw/pw), log(gh/ph), (wrap(ga)-wrap(pa))/pi),
 *           widths clipped at 1e-7; proposals = pred, gt = target (SWAP: the other way round, :31-32);
 *           MODULUS: wrap(a) = (a + pi) mod pi (:84-88); the reference then takes L1 against zeros (:34);
 *   otherwise d = pred - target.
 * weight: (n,5) or NULL.  The backward gives the gradients w.r.t. both planar boxes (feed them to
 * sph2pob_transform_bwd_f32 to reach the spherical boxes).  grad_target may be NULL.
 * NaN as in the reference's autograd graph: the adjoint of |d| is sgn(d) with sgn(NaN) = 0, so a NaN delta sends 0 down its own
 * column; a NaN operand still reaches every gradient it is multiplied or divided into (a NaN width: the other box's width).
 */
enum { SPH2POB_L1_ENCODE = 1, SPH2POB_L1_SWAP = 2, SPH2POB_L1_MODULUS = 4 };
int sph2pob_obb_l1_fwd_f32(const float* planar_pred, const float* planar_target, const float* weight, float scale,
                           float* loss, int64_t n, int flags, void* stream);
int sph2pob_obb_l1_bwd_f32(const float* planar_pred, const float* planar_target, const float* weight,
                           const float* grad_loss, float scale, float* grad_pred, float* grad_target, int64_t n,
                           int flags, void* stream);

/* ---- sigmoid focal loss: the classification half of SphRetinaHead.loss_single -------------------------------------------
 * Replaces FocalLoss(use_sigmoid=True) (mmdet/models/losses/focal_loss.py:159-244), i.e. mmcv.ops.sigmoid_focal_loss + the
 * weight step and reduction of weight_reduce_loss (mmdet/models/losses/utils.py:30-58), and the
 * cls_score.permute(0, 2, 3, 1).reshape(-1, C) copy in front of it (sphdet/models/heads/sph_retina_head.py:247-248).
 * Per element, x = logit, t = (label == c), in the logit-stable form (z = t ? -x : x, e = exp(-|z|), q = sigmoid(z) and
 * sigmoid(-z) both from e, s = softplus(z) = max(z, 0) + log1p(e), a = t ? alpha : 1 - alpha):
 *     L = a q^gamma s,    dL/dz = a q^gamma (q + gamma sigmoid(-z) s),    dL/dx = t ? -dL/dz : dL/dz
 * which is py_sigmoid_focal_loss (focal_loss.py:12-57) in exact arithmetic; it differs from mmcv's kernel only where that kernel
 * clamps log at FLT_MIN (logits beyond about +-16 on the wrong side).  gamma >= 0; 2 and 0 are multiplications, a general gamma
 * takes its integer part as multiplications and the rest through exp2(frac * log2 q).  A label is only ever COMPARED with the
 * class index: any value outside [0, C) (the background label C, -1, ...) means that no class of the row is positive.
 * weight_mode: NONE; ROW: weight (B, n) per anchor; ELEM: weight in logical (B, n, C) order.
 *
 * sph2pob_focal_loss_sum_f32 — the training call, for all levels of a head at once.  Level tables are HOST arrays of
 * num_levels <= 8 entries, as for sph2pob_get_bboxes_f32:
 *   logits       device pointers, level l either the head's NCHW (B, A C, H_l, W_l), read in place, or the flattened
 *                (B, n_l, C); anchor i of a level is (h W + w) A + a, its class c is channel a C + c.  (N, C): one level, B = 1
 *   grads        NULL (forward only), or device pointers laid out exactly like logits that receive
 *                scale_eff * w * dL/dx: the gradient of out[0] for an upstream gradient of 1
 *   level_n      n_l = H_l W_l A anchors (>= 0);  level_hw: H_l W_l for NCHW, 0 for the flattened layout (NULL: all flattened)
 *   labels       (B, n) int64, n = sum n_l, rows in level order: what sph2pob_anchor_targets_f32 writes; weight likewise
 *   scale        host factor (loss_weight, possibly over a host divisor); avg_factor: NULL, or a DEVICE float: then
 *                scale_eff = scale / (*avg_factor + FLT_EPSILON) (one fp32 division), else scale_eff = scale
 *   out          (1) f32 = scale_eff * sum w L.  The weighted element losses are added in double, one partial per workgroup in
 *                `workspace`, and the partials in a fixed order by one workgroup: no float atomics, the same bits on every call
 *   workspace    sph2pob_focal_loss_workspace_bytes(level_n, level_hw, num_levels, B, C) bytes (0: shapes not accepted), no
 *                initialisation
 * Two launches whatever B and the number of levels are; nothing is read back, nothing is allocated.  NCHW levels whose H W is a
 * multiple of 4 and whose pointers are 16-byte aligned are walked with 16-byte accesses, the others with the same arithmetic
 * one element at a time.  B n C == 0 writes out[0] = 0.
 * Errors, checked in this order before anything is enqueued: gamma < 0 (or NaN), weight_mode -> SPH2POB_ERR_OPTION; num_levels
 * outside [1, 8], B outside [0, 65 535], C outside [1, 2^24] -> SPH2POB_ERR_SIZE; a NULL level_n / logits table ->
 * SPH2POB_ERR_NULL; n_l < 0, level_hw that does not divide n_l, B n_l C >= 2^31 - 4096 -> SPH2POB_ERR_SIZE; a NULL table entry of
 * a level with elements, out, workspace, labels or (weight_mode != NONE) weight with elements -> SPH2POB_ERR_NULL.
 *
 * sph2pob_focal_loss_fwd_f32: loss[i, c] = scale * w * L on a flat (n, C) input (reduction 'none').
 * sph2pob_focal_loss_bwd_f32: grad_logits[i, c] = grad_out[(i C + c) * grad_stride] * scale_eff * w * dL/dx (grad_stride 0: one
 * device scalar, 1: per element) — reduction 'none', and a second backward through a retained graph.
 * sph2pob_focal_loss_grad_scale_f32: out[e] = stash[e] * grad_out[0], e < total; out may be the stash (in place), and in place
 * with grad_out[0] == 1 the launch returns after one scalar load per workgroup, as sph2pob_loss_grad_scale_f32 does.
 * The flat entries: weight_mode, gamma, grad_stride -> SPH2POB_ERR_OPTION; n < 0, C <= 0, n C > 2^38 -> SPH2POB_ERR_SIZE; n == 0
 * is a no-op; a NULL pointer with work to do -> SPH2POB_ERR_NULL.
 */
enum { SPH2POB_FOCAL_WEIGHT_NONE = 0, SPH2POB_FOCAL_WEIGHT_ROW = 1, SPH2POB_FOCAL_WEIGHT_ELEM = 2 };
int64_t sph2pob_focal_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                           int64_t num_classes);
int sph2pob_focal_loss_sum_f32(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int64_t num_classes, const int64_t* labels, const float* weight,
                               int weight_mode, float gamma, float alpha, float scale, const float* avg_factor, float* out,
                               void* workspace, void* stream);
int sph2pob_focal_loss_fwd_f32(const float* logits, const int64_t* labels, const float* weight, int weight_mode, float gamma, float alpha,
                               float scale, float* loss, int64_t n, int64_t num_classes, void* stream);
int sph2pob_focal_loss_bwd_f32(const float* logits, const int64_t* labels, const float* weight, int weight_mode, const float* grad_out,
                               int grad_stride, float gamma, float alpha, float scale, const float* avg_factor, float* grad_logits,
                               int64_t n, int64_t num_classes, void* stream);
int sph2pob_focal_loss_grad_scale_f32(const float* stash, const float* grad_out, float* out, int64_t total, void* stream);

/* ---- softmax cross-entropy, plain and with hard-negative mining: the classification half of SphSSDHead.loss_single -----------
 * Replaces, for softmax heads (use_sigmoid=False), the chain cls_score.permute(0, 2, 3, 1).reshape(B, -1, K) -> cat over the
 * levels -> F.cross_entropy(reduction='none') * label_weights -> per image nonzero() twice and topk(min(r P_b, N_b))
 * (sphdet/models/heads/sph_ssd_head.py:96-161), and mmdet's cross_entropy + weight_reduce_loss in plain mode.
 * K = score channels per anchor (C + 1, background last); channel a K + c of an NCHW level is class c of anchor a.  Per row i of
 * image b, with label t:
 *     valid  = 0 <= t < K and t != ignore_index; an invalid row has loss 0, gradient 0 and is neither positive nor negative
 *              (F.cross_entropy raises on an out-of-range label instead)
 *     l_i    = CE(x_i, t) * class_weight[t] * weight[b, i]
 *     plain  (neg_pos_ratio == -1): out = scale_eff * sum of l_i over the valid rows
 *     mining (neg_pos_ratio = r >= 0): positives = valid rows with t != background_label, negatives = rows with
 *              t == background_label, k_b = min(r P_b, N_b) from the labels on the device; the mined negatives of an image are the
 *              first k_b in the order (l_i descending, row index ascending), a NaN above +inf as torch.topk has it;
 *              out = scale_eff * sum_b (sum of l_i over positives + mined): ONE scalar, the sum of the reference's B values
 *     grad   = scale_eff * weight * class_weight[t] * (softmax(x_i)_j - [j == t]) on positive / mined (plain: valid) rows, an exact
 *              0.0 on every other element; every element of every level is written exactly once
 * Arithmetic (csrc/sph2pob_softmax.hpp): m = max_j x_j, e_j = expf(x_j - m), class sums in double without the maximum's own
 * term; CE = log1p(sum_{j != t} e_j) when the target is the maximum, else (m - x_t) + log1p(S - 1); the target's gradient
 * component is -(sum_{j != t} e_j) / S, never p_t - 1.  The tie rule (lowest row index first) is where the mined SET may differ
 * from torch.topk, whose choice among equal values is unspecified; the loss value does not depend on it.  The reference divides by
 * num_total_samples without the FLT_EPSILON of scale_eff.
 *
 * sph2pob_softmax_loss_sum_f32 — level tables, labels, weight (per row, or NULL), scale, avg_factor, out as for
 * sph2pob_focal_loss_sum_f32; class_weight NULL or (K,) device floats; workspace of
 * sph2pob_softmax_loss_workspace_bytes(level_n, level_hw, num_levels, B, K, mining) bytes (0: shapes not accepted), no
 * initialisation.  Launches: plain 2; mining 4 (rows -> keys, one workgroup per image for the cut, rows -> gradient, final), 3
 * without grads.  No float atomics, nothing read back: the same bits on every call.
 * Errors, in this order before anything is enqueued: neg_pos_ratio < -1 (or > 2^30) -> SPH2POB_ERR_OPTION; num_levels outside
 * [1, 8], B outside [0, 65 535], K outside [2, 4096] -> SPH2POB_ERR_SIZE; a NULL level_n / logits table -> SPH2POB_ERR_NULL;
 * n_l < 0, level_hw that does not divide n_l, B n_l K >= 2^31 - 4096 -> SPH2POB_ERR_SIZE; a NULL table entry of a level with
 * elements, out, workspace, or labels with rows -> SPH2POB_ERR_NULL.  B n == 0 writes out[0] = 0.
 *
 * sph2pob_softmax_loss_fwd_f32: loss[i] = scale * l_i on a flat (n, K) input (reduction 'none').
 * sph2pob_softmax_loss_bwd_f32: grad_logits[i, j] = grad_out[i * grad_stride] * scale_eff * weight * class_weight[t] * dCE/dx_j
 * (grad_stride 0: one device scalar, 1: per row).  grad_stride -> SPH2POB_ERR_OPTION; n < 0, K outside [2, 4096], n K > 2^38 ->
 * SPH2POB_ERR_SIZE; n == 0 is a no-op; a NULL pointer with work to do -> SPH2POB_ERR_NULL.
 */
int64_t sph2pob_softmax_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                             int64_t num_channels, int mining);
int sph2pob_softmax_loss_sum_f32(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                 int num_levels, int64_t num_images, int64_t num_channels, const int64_t* labels, const float* weight,
                                 const float* class_weight, int64_t ignore_index, int64_t background_label, int64_t neg_pos_ratio,
                                 float scale, const float* avg_factor, float* out, void* workspace, void* stream);
int sph2pob_softmax_loss_fwd_f32(const float* logits, const int64_t* labels, const float* weight, const float* class_weight,
                                 int64_t ignore_index, float scale, float* loss, int64_t n, int64_t num_channels, void* stream);
int sph2pob_softmax_loss_bwd_f32(const float* logits, const int64_t* labels, const float* weight, const float* class_weight,
                                 int64_t ignore_index, const float* grad_out, int grad_stride, float scale, const float* avg_factor,
                                 float* grad_logits, int64_t n, int64_t num_channels, void* stream);

/* ---- fused box-regression loss: the regression half of SphRetinaHead.loss_single ------------------------------------------
 * Replaces, for reg_decoded_bbox=True (sphdet/models/heads/sph_retina_head.py:252-265), the chain
 * bbox_pred.permute(0, 2, 3, 1).reshape(-1, dim) -> cat over the levels -> DeltaXYWH(A)SphBBoxCoder.decode -> Sph2PobIoULoss ->
 * / avg_factor and its backward by one pass that reads only the weights and, for the rows whose weight is not zero, their deltas,
 * anchors and targets.  Per such row the arithmetic is the composition's: sph2pob_coder_decode_f32 with num_classes = 1, then the
 * loss element and adjoint of sph2pob_loss_fwd_grad_f32, then the diagonal Jacobian of sph2pob_coder_decode_bwd_f32.
 *
 * sph2pob_bbox_loss_sum_f32 — level tables are HOST arrays of num_levels <= 8 entries, as for sph2pob_focal_loss_sum_f32:
 *   bbox_preds   device pointers, level l either the head's NCHW (B, A dim, H_l, W_l), read in place, or the flattened
 *                (B, n_l, dim); anchor i of a level is (h W + w) A + a, its component k is channel a dim + k
 *   grads        NULL (forward only), or device pointers laid out exactly like bbox_preds that receive
 *                scale_eff * w_i * J_decode^T dL/dbox: the gradient of out[0] for an upstream gradient of 1.  EVERY element of
 *                every level is written, exactly once: rows of weight 0 get +0.0f
 *   level_n      n_l = H_l W_l A anchors (>= 0);  level_hw: H_l W_l for NCHW, 0 for the flattened layout (NULL: all flattened)
 *   anchors      (n, dim), n = sum n_l, rows in level order, shared by all images (as sph2pob_anchor_targets_f32 takes them)
 *   targets      (B, n, dim) decoded ground-truth boxes: what sph2pob_anchor_targets_f32 writes with encode == 0
 *   weight       NULL (all ones), (B, n) when weight_dim == 1, (B, n, dim) when weight_dim == dim: the per-box mean is taken as
 *                OBBIoULoss takes it (sph2pob_loss_fwd_f32)
 *   means_host, stds_host, max_ratio, coder_flags, ctr_clamp   exactly those of sph2pob_coder_decode_f32
 *   loss_mode    SPH2POB_LOSS_* (| SPH2POB_FLAG_REFERENCE_ORDER), eps: as for sph2pob_loss_fwd_f32
 *   scale, avg_factor   as for sph2pob_focal_loss_sum_f32: scale_eff = scale / (*avg_factor + FLT_EPSILON) with a DEVICE float
 *   out          (1) f32 = scale_eff * sum_i w_i L(decode(anchor_i, delta_i), target_i): double partials per workgroup in
 *                `workspace`, added in a fixed order by one workgroup — no float atomics, no counter, the same bits on every call
 *   workspace    sph2pob_bbox_loss_workspace_bytes(level_n, level_hw, num_levels, B, box_dim) bytes (0: shapes not accepted)
 * A row whose mean weight is exactly 0 contributes an exact zero loss and zero gradient and its deltas and targets are NEVER READ:
 * a NaN there stays inert.  (The rule of the loss entries above is per wave of 64 rows, csrc/sph2pob_loss.hip; here it is per
 * row.)  Two launches whatever B and the number of levels are; nothing is read back, nothing is allocated; capturable.  The
 * gradient leaves in whole 16-byte stores along w for NCHW levels whose H W is a multiple of 4 (flattened: n_l dim a multiple of
 * 4) and whose gradient pointer is 16-byte aligned, one element at a time with the same values otherwise.  B n == 0 writes
 * out[0] = 0.  After the call torch's backward is sph2pob_focal_loss_grad_scale_f32 on the gradient buffer.
 * Errors, checked in this order before anything is enqueued: loss_mode flags -> SPH2POB_ERR_OPTION; box_dim -> SPH2POB_ERR_DIM;
 * loss mode, weight_dim (with a weight), coder_flags, max_ratio < 0 -> SPH2POB_ERR_OPTION; num_levels outside [1, 8], B outside
 * [0, 65 535] -> SPH2POB_ERR_SIZE; a NULL level_n / bbox_preds table -> SPH2POB_ERR_NULL; n_l < 0, level_hw that does not divide
 * n_l, B n_l dim >= 2^31 - 4096, more than 360 / dim anchors per position -> SPH2POB_ERR_SIZE; a NULL table entry of a level with
 * rows, out, workspace, anchors or targets with rows -> SPH2POB_ERR_NULL.
 */
int64_t sph2pob_bbox_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                          int box_dim);
int sph2pob_bbox_loss_sum_f32(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                              int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                              const float* weight, int weight_dim, const float* means_host, const float* stds_host, float max_ratio,
                              int coder_flags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
                              float* out, void* workspace, void* stream);

/* ---- fused L1 / SmoothL1 box loss on the head's ENCODED deltas: the regression half of loss_single by default -----------------
 * Replaces, for reg_decoded_bbox=False and loss_bbox = L1Loss / SmoothL1Loss (the reference's base configs;
 * mmdet/models/losses/smooth_l1_loss.py:10-52), the chain bbox_pred.permute(0, 2, 3, 1).reshape(-1, dim) -> cat over the levels ->
 * |pred - target| (or its smooth form) * weight -> sum / avg_factor and its backward by one pass that reads only the weights and,
 * for the rows with a non-zero weight, their deltas and targets.  Nothing is decoded: there are no anchors and no coder.
 *
 * sph2pob_delta_loss_sum_f32 — the arguments of sph2pob_bbox_loss_sum_f32 without anchors, coder and loss mode, with beta:
 *   bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim   exactly as for sph2pob_bbox_loss_sum_f32; grads
 *                receive (scale_eff * w_k) * s_k per element, EVERY element of every level written exactly once
 *   targets      (B, n, dim) ENCODED deltas: what sph2pob_anchor_targets_f32 writes with encode == 1
 *   weight       NULL (all ones), (B, n) when weight_dim == 1, (B, n, dim) when weight_dim == dim: each element loss is
 *                multiplied by ITS OWN weight (no row mean)
 *   beta         0: l1_loss — element loss d = |pred - target|, s = sign(pred - target) (0 at equality);
 *                > 0: smooth_l1_loss — ((0.5 d) d) / beta and s = (pred - target) / beta where d < beta, d - 0.5 beta and the
 *                sign otherwise.  fp32, in this operation order
 *   scale, avg_factor   as for sph2pob_focal_loss_sum_f32: scale_eff = scale / (*avg_factor + FLT_EPSILON) with a DEVICE float
 *   out          (1) f32 = scale_eff * sum over elements of w_k * loss_k: double partials per workgroup in `workspace`, added
 *                in a fixed order by one workgroup — no float atomics, the same bits on every call
 *   workspace    sph2pob_delta_loss_workspace_bytes(level_n, level_hw, num_levels, B, box_dim) bytes (0: shapes not accepted)
 * A row whose dim weights are ALL exactly 0 contributes an exact zero loss and +0.0f gradients and its deltas and targets are
 * NEVER READ: a NaN there stays inert.  The test is any != 0, so (+1, -1, 0, 0) is a live row; in a live row the elements of
 * weight 0 are evaluated and multiplied by 0, as in the composition (a NaN delta there reaches the sum).  Two launches whatever B
 * and the number of levels are; nothing is read back, nothing is allocated; capturable.  Store widths as for
 * sph2pob_bbox_loss_sum_f32.  B n == 0 writes out[0] = 0.  After the call torch's backward is
 * sph2pob_focal_loss_grad_scale_f32 on the gradient buffer.
 * Errors, checked in this order before anything is enqueued: box_dim -> SPH2POB_ERR_DIM; weight_dim (with a weight), beta < 0
 * or NaN -> SPH2POB_ERR_OPTION; then the shape and table checks of sph2pob_bbox_loss_sum_f32 with the same codes and limits
 * (num_levels, B -> SIZE; NULL level_n / bbox_preds table -> NULL; n_l, level_hw, B n_l dim >= 2^31 - 4096, more than
 * 360 / dim anchors per position -> SIZE); a NULL table entry of a level with rows, out, workspace, or targets with rows ->
 * SPH2POB_ERR_NULL.
 */
int64_t sph2pob_delta_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                           int box_dim);
int sph2pob_delta_loss_sum_f32(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int box_dim, const float* targets, const float* weight,
                               int weight_dim, float beta, float scale, const float* avg_factor, float* out, void* workspace,
                               void* stream);

/* ---- 16-bit head outputs: the five multi-level entries on float16 / bfloat16 level tensors, read where they are -----------------
 * Under mixed precision (torch.autocast; mmdet's fp16 = dict(...), whose force_fp32 is the cast these entries remove) the head's
 * outputs are 16-bit.  Each entry below takes the arguments of its _f32 sibling, in its order, and before `stream`
 *   dtype        SPH2POB_DTYPE_F16 | SPH2POB_DTYPE_BF16: the element type of every LEVEL pointer (logits / bbox_preds /
 *                cls_scores) and, for the losses, of the `grads` pointers.  Anchors, targets, weights, labels, avg_factor, out
 *                and every result stay fp32 / int64.
 * A level value is widened to fp32 on load (exact) and all arithmetic is the sibling's, in fp32 / double, unchanged: the item and
 * span geometry, the partial order and the layouts do not depend on dtype — a thread's four consecutive elements are one 8-byte
 * access, so the vector kinds need 8-byte alignment where fp32 needs 16.  Hence, for levels that qualify for the same kinds as
 * their fp32 copies (every tensor from an allocator does), the loss scalar and the four inference outputs have the BITS the
 * sibling gives on the levels converted to fp32.
 *
 * The three loss entries also take, between `workspace` and `dtype`,
 *   grad_out     NULL (an upstream gradient of 1), or a DEVICE float g: grads receive RNE(g * s), s being the fp32 value the
 *                sibling writes — one fp32 product, then ONE round-to-nearest-even narrowing (never a 16-bit value scaled
 *                afterwards: small fp16 gradients under a loss scale survive).  Ignored without grads
 *   skip_if_one  with grad_out: every workgroup returns at once when g == 1.0f exactly — `grads` then already hold the gradient
 *                of an earlier call with grad_out NULL (a device-side test, no host read; capturable)
 * and `out` may be NULL (then `workspace` may be too): no partials are written and no final pass is launched — the gradient-only
 * call of torch's backward.  With out, workspace is required as for the sibling.  out and grads both NULL: nothing is enqueued.
 * The protocol of an autograd node: forward with grads = a 16-bit stash and grad_out NULL; the first backward is the same call
 * with grad_out = g, skip_if_one = 1, out = NULL on the stash (in place: the levels are read, not the stash); a later backward
 * through a retained graph is that call into a fresh buffer with skip_if_one = 0.  No fp32 copy of a level or of a gradient
 * exists at any point.
 * Errors: a dtype outside the enum -> SPH2POB_ERR_OPTION, first; then the sibling's checks with its codes and in its order (out /
 * workspace as above), all before anything is enqueued.  There are no CPU twins: CPU tensors of a 16-bit dtype are converted by
 * the caller and take the _f32 twins.
 */
enum { SPH2POB_DTYPE_F16 = 1, SPH2POB_DTYPE_BF16 = 2 };
int sph2pob_focal_loss_sum_h16(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int64_t num_classes, const int64_t* labels, const float* weight,
                               int weight_mode, float gamma, float alpha, float scale, const float* avg_factor, float* out,
                               void* workspace, const float* grad_out, int skip_if_one, int dtype, void* stream);
int sph2pob_bbox_loss_sum_h16(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                              int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                              const float* weight, int weight_dim, const float* means_host, const float* stds_host, float max_ratio,
                              int coder_flags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
                              float* out, void* workspace, const float* grad_out, int skip_if_one, int dtype, void* stream);
int sph2pob_delta_loss_sum_h16(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int box_dim, const float* targets, const float* weight,
                               int weight_dim, float beta, float scale, const float* avg_factor, float* out, void* workspace,
                               const float* grad_out, int skip_if_one, int dtype, void* stream);
int sph2pob_get_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors,
                           const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes,
                           int box_dim, int activation, float score_thr, int64_t nms_pre, const float* means_host,
                           const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp, int variant,
                           float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels, int64_t* prior_inds,
                           int64_t* num_dets, void* workspace, int dtype, void* stream);
int sph2pob_test_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors,
                            const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes,
                            int box_dim, int activation, float score_thr, int64_t nms_pre, const float* means_host,
                            const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp, int variant_flags,
                            int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels,
                            int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream);

/* ---- fused Gaussian box-regression loss: loss_single's regression half with Sph2PobGDLoss / Sph2PobKFLoss -------------------------
 * sph2pob_bbox_loss_sum_f32 with the Gaussian body of the sph2pob_gauss_loss_* launchers in place of the IoU family: per row whose
 * mean weight is not zero, sph2pob_coder_decode_f32 with num_classes = 1, then the loss element and adjoint of
 * sph2pob_gauss_loss_fwd_grad_f32, then the diagonal Jacobian of sph2pob_coder_decode_bwd_f32; grads receive
 * ((scale_eff * w_i) * dL/dbox_k) * J_k.
 *
 * sph2pob_gauss_bbox_loss_sum_f32 — the arguments of sph2pob_bbox_loss_sum_f32 up to and including ctr_clamp, with their meaning,
 * layouts, limits, store widths and zero-weight rule (a row of mean weight exactly 0 is NEVER READ and gets an exact zero loss and
 * +0.0f gradients); then, in place of (loss_mode, eps),
 *   type_flags, fun, tau, alpha, opts, beta, eps   exactly the trailing parameters of sph2pob_gauss_loss_fwd_f32 (type_flags:
 *                SPH2POB_GAUSS_* | SPH2POB_FLAG_REFERENCE_ORDER)
 * then scale, avg_factor, out, workspace, stream as for sph2pob_bbox_loss_sum_f32, with
 *   workspace    sph2pob_gauss_bbox_loss_workspace_bytes(level_n, level_hw, num_levels, B, box_dim) bytes (0: shapes not accepted)
 * Two launches whatever B and the number of levels are; nothing is read back, nothing is allocated; capturable.  B n == 0 writes
 * out[0] = 0.  After the call torch's backward is sph2pob_focal_loss_grad_scale_f32 on the gradient buffer.
 * Errors, checked in this order before anything is enqueued: type_flags flags -> SPH2POB_ERR_OPTION; box_dim -> SPH2POB_ERR_DIM;
 * loss type, a post-map the type does not accept, opts bits, weight_dim (with a weight), coder_flags, max_ratio < 0 ->
 * SPH2POB_ERR_OPTION; then the shape and table checks of sph2pob_bbox_loss_sum_f32 with the same codes and limits (num_levels, B ->
 * SIZE; NULL level_n / bbox_preds table -> NULL; n_l, level_hw, B n_l dim >= 2^31 - 4096, more than 360 / dim anchors per position
 * -> SIZE); a NULL table entry of a level with rows, out, workspace, anchors or targets with rows -> SPH2POB_ERR_NULL.
 *
 * sph2pob_gauss_bbox_loss_sum_h16 — float16 / bfloat16 levels read where they are: differs from the _f32 entry exactly as
 * sph2pob_bbox_loss_sum_h16 differs from sph2pob_bbox_loss_sum_f32 (grad_out, skip_if_one, dtype in front of stream; out and
 * workspace may be NULL; the dtype is checked first).  No CPU twin.
 */
int64_t sph2pob_gauss_bbox_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                                int box_dim);
int sph2pob_gauss_bbox_loss_sum_f32(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                    int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                                    const float* weight, int weight_dim, const float* means_host, const float* stds_host,
                                    float max_ratio, int coder_flags, float ctr_clamp, int type_flags, int fun, float tau, float alpha,
                                    int opts, float beta, float eps, float scale, const float* avg_factor, float* out,
                                    void* workspace, void* stream);
int sph2pob_gauss_bbox_loss_sum_h16(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                    int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                                    const float* weight, int weight_dim, const float* means_host, const float* stds_host,
                                    float max_ratio, int coder_flags, float ctr_clamp, int type_flags, int fun, float tau, float alpha,
                                    int opts, float beta, float eps, float scale, const float* avg_factor, float* out,
                                    void* workspace, const float* grad_out, int skip_if_one, int dtype, void* stream);

/* ---- inference for softmax heads (use_sigmoid_cls=False: SphSSDHead, the two-channel SphRPNHead) ---------------------------------
 * The reference's `cls_score.softmax(-1)[:, :-1]` in front of filter_scores_and_topk (sphdet/models/heads/sph_ssd_head.py:330-347;
 * sph_rpn_head.py:52-57, softmax(dim=1)[:, 0], is K = 2), for B images, read from the head's own layout.  Every anchor has
 * K = num_classes + 1 logits, the background LAST inside the anchor's group of K: NCHW (B, A K, H_l, W_l), channel a K + j, or
 * flat (B, n_l, K).
 * The probability, pinned as the sigmoid of sph2pob_test_bboxes_f32 is (csrc/sph2pob_softmax.hpp, Prob): per anchor m = max_j x_j;
 * e_j = expf(x_j - m), the difference taken in fp32; S = sum_j e_j in double, in ascending class order; p_c = (float)((double)e_c
 * / S) for c < C = num_classes.  These are the e_j and the S of the loss (sph2pob_softmax_loss_sum_f32's Row), whose gradient
 * e_j * (1 / S) differs from e_j / S in the last bit of a double at most: a model infers with the probabilities it was trained
 * with.  A -inf logit has probability exactly 0.  A row with a NaN or a +inf (or without a finite logit) is NaN in all its
 * classes and so yields no candidate (score > score_thr is false); other rows are not touched.
 *
 * sph2pob_softmax_scores_f32 — the probabilities alone, one launch, nothing read back:
 *   logits       HOST table of num_levels <= 8 device pointers, laid out as above, read in place
 *   level_n      n_l anchors;  level_hw: H_l W_l for the NCHW layout, 0 for the flat one (NULL: every level flat)
 *   out          HOST table of device pointers: level l receives fp32 (B, A C, H_l, W_l) resp. (B, n_l, C) — the layout of the
 *                logits without the background channel, what sph2pob_test_bboxes_f32 takes with activation = 0
 * Errors, in this order, before anything is enqueued: num_levels outside [1, 8], B outside [0, 65 535], K = num_classes + 1
 * outside [2, 4096] -> SPH2POB_ERR_SIZE; a NULL level_n / logits / out table -> SPH2POB_ERR_NULL; per level n_l < 0, level_hw that
 * does not divide n_l, B n_l K >= 2^31 - 4096 -> SPH2POB_ERR_SIZE, a NULL entry of a level with B n_l > 0 -> SPH2POB_ERR_NULL.
 * B n_l == 0 everywhere: nothing is enqueued.
 * sph2pob_softmax_scores_h16 — float16 / bfloat16 logits read where they are (dtype: SPH2POB_DTYPE_*, checked first ->
 * SPH2POB_ERR_OPTION), widened on load; out stays fp32 and has the bits the _f32 entry gives on the widened logits.
 *
 * sph2pob_softmax_bboxes_f32 — sph2pob_test_bboxes_f32 for a softmax head in one call, eleven launches whatever B is, nothing
 * read back, nothing allocated, capturable.  The arguments of sph2pob_test_bboxes_f32 without `activation`; cls_scores are
 * the logits (K per anchor), num_classes = C = K - 1.  Stage 0 writes the probabilities above into the workspace, in the head's
 * layout without the background channel; from there on everything is what sph2pob_test_bboxes_f32 documents with activation = 0:
 * a candidate is (anchor, c) with index anchor C + c, valid iff p > score_thr, the selection, decode, NMS and outputs as there —
 * the result has the BITS of sph2pob_test_bboxes_f32 on the output of sph2pob_softmax_scores_f32.  labels lie in [0, C).
 *   workspace    sph2pob_softmax_bboxes_workspace_bytes(level_n, num_levels, B, C, box_dim, nms_pre) bytes, no initialisation
 *                (0 = the shapes are not accepted): that of sph2pob_test_bboxes_f32 plus 4 B n_l C bytes per level
 * Errors, in the order of sph2pob_test_bboxes_f32: box_dim -> SPH2POB_ERR_DIM; variant, flags, class_agnostic, coder_flags,
 * max_ratio < 0 -> SPH2POB_ERR_OPTION; num_levels outside [1, 8], B outside [1, 65 535], C < 1 or K = C + 1 > 4096, nms_pre <= 0,
 * max_per_img < 0 -> SPH2POB_ERR_SIZE; a NULL table -> SPH2POB_ERR_NULL; n_l < 1, n_l C >= 2^31 - 2^17, level_hw that does not
 * divide n_l, K_cap > sph2pob_batched_nms_max_boxes() -> SPH2POB_ERR_SIZE; a NULL table entry, output or workspace ->
 * SPH2POB_ERR_NULL; then B n_l K >= 2^31 - 4096 -> SPH2POB_ERR_SIZE.
 * sph2pob_softmax_bboxes_h16 — float16 / bfloat16 logits AND deltas read where they are (dtype checked first ->
 * SPH2POB_ERR_OPTION); no fp32 copy of either exists, only the C foreground probabilities are written, in fp32; the outputs have
 * the bits of the _f32 entry on the widened levels.  The _f32 entries have CPU twins, the _h16 ones do not.
 */
int sph2pob_softmax_scores_f32(const void* const* logits, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                               int64_t num_images, int64_t num_classes, void* const* out, void* stream);
int sph2pob_softmax_scores_h16(const void* const* logits, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                               int64_t num_images, int64_t num_classes, void* const* out, int dtype, void* stream);
int64_t sph2pob_softmax_bboxes_workspace_bytes(const int64_t* level_n, int num_levels, int64_t num_images, int64_t num_classes,
                                               int box_dim, int64_t nms_pre);
int sph2pob_softmax_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors,
                               const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                               int64_t num_classes, int box_dim, float score_thr, int64_t nms_pre, const float* means_host,
                               const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp, int variant_flags,
                               int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels,
                               int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream);
int sph2pob_softmax_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors,
                               const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                               int64_t num_classes, int box_dim, float score_thr, int64_t nms_pre, const float* means_host,
                               const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp, int variant_flags,
                               int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels,
                               int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream);

/*
 * sph2pob_sample_targets_f32 — random sampling of the anchor targets of a minibatch: mmdet's RandomSampler as the reference's
 * SphRandomSampler calls it (sphdet/bbox/sampler/sph_random_sampler.py:34-46 over mmdet/core/bbox/samplers/random_sampler.py,
 * add_gt_as_proposals=False) and the target lines of AnchorHead._get_targets_single with a real sampler (anchor_head.py:254-299),
 * applied to what sph2pob_anchor_targets_f32 wrote.  Two launches whatever B is, nothing read back to the host.
 *   assigned_gt_inds (B, n) int64     > 0 positive, == 0 negative, < 0 ignored, as sph2pob_anchor_targets_f32 writes it
 *   labels_in, label_weights_in (B, n), bbox_targets_in, bbox_weights_in (B, n, box_dim): the targets of the same call
 *   num_expected_pos = (int)(num * pos_fraction), computed by the caller; num; neg_pos_ub (< 0: none)
 * Per image b, with P_b / N_b the positive / negative rows, COUNTED by the kernel from assigned_gt_inds:
 *   k_pos = min(P_b, num_expected_pos);  k_neg = min(N_b, num - k_pos), and with neg_pos_ub >= 0 additionally at most
 *   (int64)(neg_pos_ub * (double)max(1, k_pos))
 *   rank(b, i) = word 0 of Philox4x32-10 (multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85) with key
 *   (seed & 0xffffffff, seed >> 32) and counter (i, b, 0, 0); an all-zero counter and key give 6627e8d5 e169c58d bc57ac4c
 *   9b00dbd8, all-ones give 408f276d 41c83b0e a20bc7c6 6d5451fd.  `ranks` (B, n) uint32, when non-NULL, replaces the generator
 *   (only the words of positive and negative rows are read)
 *   the sampled positives are the k_pos positive rows with the smallest (rank, i) — ties by ascending row index — and the sampled
 *   negatives the k_neg negative rows chosen likewise: a uniform k-subset up to rank ties (two of m rows tie with probability
 *   ~m^2 / 2^33), NOT the stream of torch.randperm, which no device implementation reproduces
 *   seed         a host int64, or — when seed_device is non-NULL, which then wins — one int64 ON THE DEVICE read by the kernels: a
 *                captured graph draws a fresh sample on every replay once the caller changes that word
 * Outputs (the four target pointers may EQUAL their inputs: the in-place form, which writes only the rows that leave the sample;
 * an output that overlaps an input in any other way is not supported):
 *   labels / label_weights / bbox_targets / bbox_weights   a sampled or ignored row keeps its input; a positive or negative row
 *                                     that is not sampled gets labels = num_classes, label_weights = 0, bbox_targets = 0, bbox_weights = 0
 *   sample_flags  (B, n) uint8        0: not sampled, 1: sampled positive, 2: sampled negative
 *   num_pos, num_neg (B) int64        k_pos, k_neg
 *   avg_factor      (1) f32           sum_b max(k_pos, 1) + sum_b max(k_neg, 1): mmdet's num_total_samples of a sampling head
 *   avg_factor_pos  (1) f32           sum_b max(k_pos, 1)
 *   workspace     sph2pob_sample_targets_workspace_bytes(num_images, n) bytes of scratch, no initialisation (0 for sizes the entry refuses)
 * Errors, checked in this order before anything is enqueued: box_dim -> SPH2POB_ERR_DIM; a NaN neg_pos_ub -> SPH2POB_ERR_OPTION;
 * num_images outside [1, 65 535], n outside [1, 2^31), num < 1, num_expected_pos outside [0, num] -> SPH2POB_ERR_SIZE; a NULL
 * input, output or workspace (seed_device and ranks may be NULL) -> SPH2POB_ERR_NULL.
 */
int64_t sph2pob_sample_targets_workspace_bytes(int64_t num_images, int64_t n);
int sph2pob_sample_targets_f32(const int64_t* assigned_gt_inds, int64_t num_images, int64_t n, int box_dim, const int64_t* labels_in,
                               const float* label_weights_in, const float* bbox_targets_in, const float* bbox_weights_in,
                               int64_t num_classes, int64_t num_expected_pos, int64_t num, double neg_pos_ub, int64_t seed,
                               const int64_t* seed_device, const uint32_t* ranks, int64_t* labels, float* label_weights,
                               float* bbox_targets, float* bbox_weights, unsigned char* sample_flags, int64_t* num_pos, int64_t* num_neg,
                               float* avg_factor, float* avg_factor_pos, void* workspace, void* stream);

/*
 * sph2pob_point_targets_f32 — the targets of an anchor-free (FCOS) head for a whole minibatch: what FCOSHead.get_targets and
 * centerness_target (mmdet/models/dense_heads/fcos_head.py:270-329, :415-434) compute through the reference's
 * SphFCOSHead._get_target_single (sphdet/models/heads/sph_fcos_head.py:107-203), per image and with (P, k) temporaries, and the two
 * normalisers that SphFCOSHead.loss obtains with nonzero() and len() (:68-82).  Two launches whatever B is, nothing read back.
 *   points (P, 2) f32, level-major: (x, y) of every location, level l owning the next level_n[l] rows
 *   the level table, HOST arrays of num_levels <= 8 entries, copied by value:
 *     level_n        points of the level (sum = P)
 *     range_lo/_hi   regress_ranges[l], as fp32
 *     sample_extent  strides[l] * center_sample_radius, rounded to fp32 by the caller (read with SPH2POB_POINT_CENTER_SAMPLING only)
 *     norm_stride    strides[l] (read with SPH2POB_POINT_NORM_ON_BBOX only)
 *   gt (num_gt, box_dim), gt_labels (num_gt) int64, gt_offsets (B + 1) int64: image b owns rows gt_offsets[b] : gt_offsets[b + 1],
 *   of which the first k_max are used (rows outside the tensor are never read, whatever the offsets say)
 *   img_h, img_w   the ERP image, 1 .. 2^24;  num_classes: the background label;  flags: SPH2POB_POINT_*
 * Per (image, point), in fp32 and in the reference's operation order (the library is built without contraction, so every float
 * output has the bits of the torch composition on the CPU):
 *   a GT goes to pixels as _sph2pix_box_transform then xywh2xyxy do it: x = (theta / 360) W, y = (phi / 180) H, w = (alpha / 360) W,
 *   h = (beta / 180) H, x1 = x - w / 2, ..., area = (x2 - x1) (y2 - y1);  l = x - x1, t = y - y1, r = x2 - x, b = y2 - y
 *   the GT is a candidate when min(l, t, r, b) > 0 — with centre sampling the same test on the centre box of :149-182, the GT's
 *   centre +- sample_extent cut to the GT with where and strict > — and range_lo <= max(l, t, r, b) <= range_hi, both ends included;
 *   a comparison with a NaN is false
 *   the candidate with the smallest area wins, the lowest index among equal areas (what areas.min(dim=1) returns on the CPU); an
 *   area >= 1e8 (the reference's INF) never wins
 * Outputs, every element written once:
 *   labels       (B, P) int64     the winner's label, num_classes without one
 *   gt_inds      (B, P) int64     1 + the winner's index inside the image, 0 without one
 *   bbox_targets (B, P, box_dim)  (l, t, r, b[, gamma]) of the winner, every component over norm_stride with NORM_ON_BBOX (the angle
 *                                 too: fcos_head.py:326-327 divides the reference's whole tensor); EXACT ZEROS without a winner — the
 *                                 reference leaves the distances to the image's GT 0 there and never reads them
 *   centerness   (B, P) f32       sqrt((min(l, r) / max(l, r)) (min(t, b) / max(t, b))) of the row as written; 0 without a winner
 *   num_pos      (B) int64        winners of the image
 *   avg_factor        (1) f32     max(sum_b num_pos, 1)
 *   centerness_denorm (1) f32     max(sum of centerness, 1e-6): the sum in double, per workgroup and then in one fixed order, rounded
 *                                 once (the reference's fp32 .sum() has no defined order)
 *   workspace    sph2pob_point_targets_workspace_bytes(B, P) bytes of scratch, no initialisation (0 for sizes the entry refuses)
 * B P == 0 is not an error: the two normalisers (1 and 1e-6) and num_pos are still written.
 * Errors, checked in this order before anything is enqueued: box_dim -> SPH2POB_ERR_DIM; num_levels outside [1, 8], B outside
 * [0, 65 535], P outside [0, 2^31 - 256), num_gt < 0 or >= 2^31, k_max < 0 or > num_gt, num_classes < 0, img_h / img_w outside
 * [1, 2^24], n_l < 0, sum n_l != P -> SPH2POB_ERR_SIZE (a NULL level_n -> SPH2POB_ERR_NULL); a NULL table the flags ask for, output,
 * input with rows or workspace -> SPH2POB_ERR_NULL; unknown flags, a NaN range, a sample_extent < 0 or NaN, a norm_stride <= 0 or NaN
 * -> SPH2POB_ERR_OPTION.
 *
 * sph2pob_point_coder_{encode,decode,decode_bwd}_f32 — bbox2distance and distance2bbox of the reference's
 * DistancePointSphBBoxCoder (sphdet/bbox/coder/distance_point_sph_bbox_coder.py:131-163, :71-128), one row per lane, in its fp32
 * operation order.  points (n, 2); rows of box_dim floats.
 *   encode      gt (n, box_dim) degrees -> distances (l, t, r, b[, gamma]); clamp = 1: each of the four clamped to
 *               [0, (float)(max_dis - eps)] as torch.clamp does (a NaN stays)
 *   decode      x1 = x - l, y1 = y - t, x2 = x + r, y2 = y + b; x clipped to [0, max_w] and y to [0, max_h] (a negative bound: that
 *               axis is not clipped); then xyxy2xywh and _pix2sph_box_transform: theta = (((x1 + x2) / 2) / W) 360, ...; gamma passes
 *   decode_bwd  grad_distances for grad_boxes, as torch's autograd delivers it through that composition: the clamp passes the
 *               gradient where the corner lies inside the closed interval; nothing flows to the points
 * Errors, in this order: box_dim -> SPH2POB_ERR_DIM; n < 0 or >= 2^31 - 256, img_h / img_w outside [1, 2^24] -> SPH2POB_ERR_SIZE;
 * a NULL tensor with n > 0 -> SPH2POB_ERR_NULL; a NaN bound, clamp outside {0, 1} -> SPH2POB_ERR_OPTION.  n == 0 is a no-op.
 */
enum { SPH2POB_POINT_CENTER_SAMPLING = 1, SPH2POB_POINT_NORM_ON_BBOX = 2 };
int64_t sph2pob_point_targets_workspace_bytes(int64_t num_images, int64_t num_points);
int sph2pob_point_targets_f32(const float* points, int64_t num_points, const int64_t* level_n, const float* range_lo, const float* range_hi,
                              const float* sample_extent, const float* norm_stride, int num_levels, const float* gt, const int64_t* gt_labels,
                              const int64_t* gt_offsets, int64_t num_images, int64_t num_gt, int64_t k_max, int box_dim, int64_t img_h,
                              int64_t img_w, int64_t num_classes, int flags, int64_t* labels, int64_t* gt_inds, float* bbox_targets,
                              float* centerness, int64_t* num_pos, float* avg_factor, float* centerness_denorm, void* workspace, void* stream);
int sph2pob_point_coder_encode_f32(const float* points, const float* gt, float* distances, int64_t n, int box_dim, int64_t img_h, int64_t img_w,
                                   int clamp, double max_dis, double eps, void* stream);
int sph2pob_point_coder_decode_f32(const float* points, const float* distances, float* boxes, int64_t n, int box_dim, int64_t img_h, int64_t img_w,
                                   float max_h, float max_w, void* stream);
int sph2pob_point_coder_decode_bwd_f32(const float* points, const float* distances, const float* grad_boxes, float* grad_distances, int64_t n,
                                       int box_dim, int64_t img_h, int64_t img_w, float max_h, float max_w, void* stream);

/* ---- batched inference for FCOS heads: class score x centerness, the point coder ---------------------------------------------------
 * sph2pob_fcos_bboxes_f32 — what SphFCOSHead._get_bboxes_single / _bbox_post_process (sphdet/models/heads/sph_fcos_head.py:246-323,
 * :205-244) compute per image and level, for B images: sph2pob_test_bboxes_f32 with a score factor and the distance-point coder.
 * Ten launches whatever B is (the selection and the NMS kernels of sph2pob_test_bboxes_f32, one candidate-build kernel of its own),
 * nothing read back, nothing allocated, capturable.  The arguments of sph2pob_test_bboxes_f32, with the anchor table and the delta
 * coder's block (means_host ... ctr_clamp) replaced:
 *   points        host array of L device pointers, (n_l, 2) fp32 pixel coordinates, 8-byte aligned, shared by the images
 *                 (each point is one 8-byte load that nothing checks: the Python layer copies a view that is not 16-byte aligned)
 *   bbox_preds    the distances (l, t, r, b[, gamma]) in pixels, laid out like cls_scores with box_dim channels per point
 *   centernesses  host array of L device pointers, laid out like cls_scores with ONE channel per point: NCHW (B, A, H_l, W_l) —
 *                 point ai = p A + a of image b is element (b A + a) H_l W_l + p — or flat (B, n_l)
 *   img_h, img_w  the coder's image (the ERP the pixels refer to); max_h, max_w: the clip bounds, a negative bound = that axis is
 *                 not clipped — all four as sph2pob_point_coder_decode_f32 has them
 *   activation    applies to BOTH cls_scores and centernesses: 1 = both are logits (the head's case), 0 = both are probabilities;
 *                 the sigmoid is the one pinned for sph2pob_test_bboxes_f32
 * Per image and level the candidates are selected on the CLASS SCORES ALONE, exactly as sph2pob_test_bboxes_f32 selects them
 * (score > score_thr, the first nms_pre in (class score descending, candidate index ascending) order): threshold and top-k never
 * see the centerness.  Each selected (point, class) then gets score = class score * factor, factor = the activated centerness of
 * its point, ONE fp32 multiply, and the box sph2pob_point_coder_decode_f32 gives for its point and distances.  The NMS runs on the
 * products (its order: product descending, ties by candidate position in the image's block, the levels concatenated, each in its
 * selection order), the first max_per_img survive, and dets carries the product.  A product below score_thr stays a candidate.
 * Special values: a centerness logit of -inf gives the factor +0 and the candidate is kept with the score +0; +inf gives 1.  A
 * NaN centerness gives a NaN product, which is not filtered: it is made the quiet NaN with the sign bit clear (0x7fc00000), which the
 * NMS key — it orders scores by their bit pattern — puts in front of every finite score, so such a candidate is kept, suppresses what
 * overlaps it in its class, and is reported first with a NaN score.
 *   prior_inds    the detection's point as an index into the concatenated levels
 *   workspace     sph2pob_get_bboxes_workspace_bytes(level_n, num_levels, B, C, box_dim, nms_pre) bytes: the pipeline and its
 *                 workspace are those of sph2pob_test_bboxes_f32
 * Errors, checked in this order before anything is enqueued: box_dim -> SPH2POB_ERR_DIM; the variant, flags, class_agnostic and
 * activation rules of sph2pob_test_bboxes_f32 -> SPH2POB_ERR_OPTION; num_levels, B, C, nms_pre, max_per_img as there ->
 * SPH2POB_ERR_SIZE; a NULL table (centernesses included) -> SPH2POB_ERR_NULL; n_l, level_hw, K_cap as there -> SPH2POB_ERR_SIZE;
 * img_h / img_w outside [1, 2^24] -> SPH2POB_ERR_SIZE; a NaN max_h / max_w -> SPH2POB_ERR_OPTION; a NULL table entry (a centerness
 * pointer included), output or workspace -> SPH2POB_ERR_NULL.
 * sph2pob_fcos_bboxes_h16: cls_scores, bbox_preds and centernesses of ONE 16-bit type (dtype: SPH2POB_DTYPE_*, checked first ->
 * SPH2POB_ERR_OPTION), read in place; everything after the loads is fp32: the result has the bits of the _f32 call on fp32 copies.
 */
int sph2pob_fcos_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* points,
                            const void* const* centernesses, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                            int64_t num_images, int64_t num_classes, int box_dim, int activation, float score_thr, int64_t nms_pre,
                            int64_t img_h, int64_t img_w, float max_h, float max_w, int variant_flags, int class_agnostic,
                            float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels, int64_t* prior_inds,
                            int64_t* num_dets, void* workspace, void* stream);
int sph2pob_fcos_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* points,
                            const void* const* centernesses, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                            int64_t num_images, int64_t num_classes, int box_dim, int activation, float score_thr, int64_t nms_pre,
                            int64_t img_h, int64_t img_w, float max_h, float max_w, int variant_flags, int class_agnostic,
                            float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels, int64_t* prior_inds,
                            int64_t* num_dets, void* workspace, int dtype, void* stream);

/* ---- fused box-regression loss of a point (FCOS) head: the regression half of SphFCOSHead.loss -------------------------------------
 * Replaces (sphdet/models/heads/sph_fcos_head.py:76-100) the chain bbox_pred.permute(0, 2, 3, 1).reshape(-1, dim) -> cat over the
 * levels -> a broadcast copy of the points -> DistancePointSphBBoxCoder.decode of all B n predictions and of all B n targets ->
 * Sph2PobIoULoss -> / avg_factor and its backward by one pass that reads only the weights and, for the rows whose weight is not zero,
 * their point, distances and target.  It is sph2pob_bbox_loss_sum_f32 with the point coder in place of the delta coder: per live row
 * sph2pob_point_coder_decode_f32 on the prediction and on the target with the same point, the loss element and adjoint of
 * sph2pob_loss_fwd_grad_f32, then sph2pob_point_coder_decode_bwd_f32 (the clip's gate included).
 *
 * sph2pob_point_bbox_loss_sum_f32 — bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, weight, weight_dim, loss_mode,
 * eps, scale, avg_factor, out, workspace, stream exactly as for sph2pob_bbox_loss_sum_f32 (a point head has A = 1 "anchor" per
 * position; the table takes any A), with
 *   bbox_preds   the distances (l, t, r, b[, gamma]) in pixels as the head produces them, NCHW (B, A dim, H_l, W_l) or flat (B, n_l, dim)
 *   points       (n, 2) fp32 pixel coordinates, n = sum n_l, rows in level order, shared by the images
 *   targets      (B, n, dim) target DISTANCES, as sph2pob_point_targets_f32 writes bbox_targets: they are decoded with the row's point
 *   img_h, img_w, max_h, max_w   the coder's image and the clip bounds (a negative bound: that axis is not clipped, the reference's
 *                loss), as sph2pob_point_coder_decode_f32 has them; the clip applies to prediction and target alike
 *   workspace    sph2pob_point_bbox_loss_workspace_bytes(level_n, level_hw, num_levels, B, box_dim) bytes (0: shapes not accepted)
 * Nothing flows to the points, the targets or the weights.  The row rule, the store rule, the two launches and B n == 0 are those of
 * sph2pob_bbox_loss_sum_f32: a row whose mean weight is exactly 0 is NEVER READ, its loss is an exact zero and its gradients +0.0f.
 * fp32 levels only: there is no _h16 sibling.
 * Errors, checked in this order before anything is enqueued: loss_mode flags -> SPH2POB_ERR_OPTION; box_dim -> SPH2POB_ERR_DIM; loss
 * mode, weight_dim (with a weight) -> SPH2POB_ERR_OPTION; the shape and table checks of sph2pob_bbox_loss_sum_f32 with the same codes
 * and limits (num_levels, B -> SIZE; a NULL level_n / bbox_preds table -> NULL; n_l, level_hw, B n_l dim, anchors per position -> SIZE;
 * a NULL table entry of a level with rows -> NULL); img_h / img_w outside [1, 2^24] -> SPH2POB_ERR_SIZE; a NULL out, workspace, or
 * points / targets with rows -> SPH2POB_ERR_NULL; a NaN max_h / max_w -> SPH2POB_ERR_OPTION.
 */
int64_t sph2pob_point_bbox_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                                int box_dim);
int sph2pob_point_bbox_loss_sum_f32(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                    int num_levels, int64_t num_images, int box_dim, const float* points, const float* targets,
                                    const float* weight, int weight_dim, int64_t img_h, int64_t img_w, float max_h, float max_w,
                                    int loss_mode, float eps, float scale, const float* avg_factor, float* out, void* workspace,
                                    void* stream);

/* ---- fused sigmoid binary cross-entropy on the head's NCHW logits --------------------------------------------------------------------
 * mmdet's binary_cross_entropy (mmdet/models/losses/cross_entropy_loss.py:64-143) without class_weight — FCOS' loss_centerness (soft
 * targets, one channel) and the RPN's stock loss_cls (hard labels, one channel, background label 1) — for all levels of a head at
 * once, with its backward: replaces the permute / reshape / cat of the levels, binary_cross_entropy_with_logits, the mask product,
 * the sum and the divide.
 *
 * sph2pob_bce_loss_sum_f32 — logits, grads, level_n, level_hw, num_levels, num_images, scale, avg_factor, out, workspace, stream
 * exactly as for sph2pob_focal_loss_sum_f32, num_channels = C in its place of num_classes, with
 *   targets      soft targets (B, n, C) f32, or NULL
 *   labels       hard labels (B, n) int64, or NULL.  Exactly one of the two is given.
 *   weight       NULL (weight_mode 0), (B, n) (1) or (B, n, C) (2)
 *   ignore_index mmdet's (default -100)
 * Hard labels (_expand_onehot_labels): the target of channel c is label == c; a label >= C gives an all-zero row (the RPN's
 * background label 1 with C = 1); a label < 0 or == ignore_index gives the row the weight 0.  Soft targets: the element's weight is
 * multiplied by (t >= 0) & (t != ignore_index).  Element: e = expf(-|x|), r = 1 / (1 + e), sigmoid(x) = x >= 0 ? r : e r,
 * loss = (float)((double)max(x, 0) - (double)x (double)t + (double)log1pf(e)) — one rounding —, dx = sigmoid(x) - t; the gradient
 * is (scale_eff w) dx.  EVERY element is evaluated and multiplied by its weight: an element of weight 0 is read (a NaN there gives
 * a NaN), as in sph2pob_focal_loss_sum_f32.  out[0] = scale_eff * sum w loss, added in double, one partial per workgroup, the
 * partials in a fixed order: the same bits on every call.  Two launches; nothing is read back or allocated; B n C == 0 writes 0.
 *   workspace    sph2pob_bce_loss_workspace_bytes(level_n, level_hw, num_levels, B, C) bytes (0: shapes not accepted)
 * Errors, checked in this order before anything is enqueued: weight_mode -> SPH2POB_ERR_OPTION; then the size and table checks of
 * sph2pob_focal_loss_sum_f32 with the same codes and limits (num_levels, B, C -> SIZE; a NULL level_n / logits table -> NULL; n_l,
 * level_hw, B n_l C -> SIZE; a NULL table entry of a level with elements -> NULL); targets AND labels given -> SPH2POB_ERR_NULL; a
 * NULL out or workspace, neither targets nor labels with elements, a NULL weight that weight_mode asks for with elements ->
 * SPH2POB_ERR_NULL.
 */
int64_t sph2pob_bce_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                         int64_t num_channels);
int sph2pob_bce_loss_sum_f32(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                             int num_levels, int64_t num_images, int64_t num_channels, const float* targets, const int64_t* labels,
                             const float* weight, int weight_mode, int64_t ignore_index, float scale, const float* avg_factor, float* out,
                             void* workspace, void* stream);

/*
 * sph2pob_rcnn_targets_f32 — the targets of the second stage of a two-stage detector for a whole minibatch, on per-image
 * proposals: per image MaxIoUAssigner.assign(proposals_b, gt_b), the reference's SphRandomSampler.sample(...,
 * add_gt_as_proposals) (sphdet/bbox/sampler/sph_random_sampler.py:24-52 over mmdet/core/bbox/samplers/random_sampler.py),
 * bbox2roi and SphShared2FCBBoxHead.get_targets (sphdet/models/heads/sph_rcnn_head.py:30-66), as one compact table of
 * S = num_images * num rows.  Four launches whatever B is; nothing is read back, allocated or kept between calls; no atomics on
 * floats: the same bits on every call; graph-capturable (a device seed is re-read on every replay).
 *   proposals      (B, M, row_stride) f32: only the first box_dim floats of a row are read, row_stride >= box_dim, so the `dets`
 *                  (B, max_per_img, box_dim + 1) of the batched inference entries are read in place with their score column
 *   num_proposals  (B) int64 ON THE DEVICE, each clamped to [0, M] before use (the `num_dets` of those entries); NULL: every
 *                  image has M proposals
 *   gt, gt_labels, gt_offsets, num_gt, k_max: the forms and the clamping rules of sph2pob_anchor_targets_f32 (gt_labels NULL:
 *                  label 0)
 *   variant        every variant the two anchor-target entries serve between them: STANDARD, EFFICIENT, LEGACY, SPH_IOU, FOV_IOU
 *                  (box_dim 4 only), UNBIASED, NAIVE (with or without SPH2POB_FLAG_NAIVE_TAN), in the default arithmetic; edge,
 *                  the four thresholds, match_low_quality, gt_max_assign_all as there
 * Assignment.  For image b with k_b GT rows and n_b proposals, assigned index g of proposal j = what sph2pob_iou_pairwise_f32 (mode
 * IOU, angle EQUATOR) + sph2pob_assign_f32 give on that image's first n_b proposals alone (the same per-pair function on the same
 * inputs: the same bits; all 0 for an image without GT), provided the overlaps are +0 or positive (no NaN): what every variant
 * returns for valid boxes.
 * Candidates.  With add_gt != 0 and k_b > 0, candidate c < k_b is GT row c with g = c + 1, max overlap 1, its own label and
 * is_gt = 1 (AssignResult.add_gt_), and candidate c >= k_b is proposal c - k_b; otherwise candidate c is proposal c.
 * Sampling: sph2pob_sample_targets_f32's, over the candidates — P_b / N_b the candidates with g > 0 / g == 0, k_pos and k_neg by its
 * formulas from num, num_expected_pos, neg_pos_ub; the sample of a side is its k candidates with the smallest (rank, c), rank(b, c)
 * = word 0 of Philox4x32-10 with the seed as key and counter (c, b, 0, 0); `ranks` (B, k_max + M) uint32, indexed by c, replace
 * the generator when non-NULL; seed / seed_device as there.
 * Outputs.  Image b owns rows [b num, (b + 1) num): its k_pos sampled positives in ascending c, then its k_neg sampled negatives
 * in ascending c (mmdet's unique()-sorted pos_inds then neg_inds: SamplingResult.bboxes), then padding:
 *                                        sampled positive                       sampled negative   padding
 *   rois           (S, 1 + box_dim) f32  (b, box)                               (b, box)           (b, 180, 90, 1, 1[, 0])
 *   labels         (S) int64             gt_labels[g - 1]                       num_classes        num_classes
 *   label_weights  (S) f32               1, or pos_weight when > 0              1                  0
 *   bbox_targets   (S, box_dim) f32      the GT box (encode == 0) or its deltas 0                  0
 *                                        w.r.t. the roi (sph2pob_coder_encode_f32's arithmetic with means_host / stds_host)
 *   bbox_weights   (S, box_dim) f32      1                                      0                  0
 *   pos_assigned_gt_inds (S) int64       g - 1, image-local                     -1                 -1
 *   sample_inds    (S) int64             c                                      c                  -1
 *   is_gt          (S) uint8             1 for a GT candidate, else 0           0                  0
 * The padding roi is a valid 1 x 1 degree box on the equator: a caller that decodes deltas against every row meets no zero-width
 * box, and its weights of 0 keep it out of every loss.
 *   num_pos, num_neg (B) int64           k_pos, k_neg
 *   avg_factor     (1) f32               max(sum_b (k_pos + k_neg), 1): the head's max(sum(label_weights > 0), 1)
 *   num_samples    (1) f32               sum_b (k_pos + k_neg): the bbox_targets.size(0) the head hands loss_bbox as avg_factor
 *   workspace      sph2pob_rcnn_targets_workspace_bytes(num_images, m, k_max) bytes of scratch, no initialisation (0 for sizes
 *                  the entry refuses)
 * Limits: num_images <= 65 535, k_max <= 262 140, m + k_max < 2^31, row_stride <= 4096, num <= 65 535 (the compaction scan
 * carries both sides' counts in the halves of one word).  Errors, checked in this order before anything is enqueued: box_dim
 * (LEGACY / SPH_IOU / FOV_IOU with box_dim 5 included) -> SPH2POB_ERR_DIM; a bad variant or edge, SPH2POB_FLAG_REFERENCE_ORDER, a
 * NaN neg_pos_ub, add_gt or encode outside {0, 1} -> SPH2POB_ERR_OPTION; num_images outside [1, 65 535], m < 1, num_gt < 0,
 * k_max < 0 or > num_gt, row_stride < box_dim, num < 1, num_expected_pos outside [0, num], a limit exceeded -> SPH2POB_ERR_SIZE; a
 * NULL proposals, gt_offsets, gt (with num_gt > 0), output or workspace -> SPH2POB_ERR_NULL (num_proposals, gt_labels,
 * seed_device, ranks, means_host and stds_host may be NULL).
 */
int64_t sph2pob_rcnn_targets_workspace_bytes(int64_t num_images, int64_t m, int64_t k_max);
int sph2pob_rcnn_targets_f32(const float* proposals, const int64_t* num_proposals, int64_t num_images, int64_t m, int64_t row_stride,
                             const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets, int64_t num_gt, int64_t k_max, int box_dim,
                             int variant, int edge, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi, float min_pos_iou,
                             int match_low_quality, int gt_max_assign_all, int64_t num, int64_t num_expected_pos, double neg_pos_ub, int64_t seed,
                             const int64_t* seed_device, const uint32_t* ranks, int add_gt, int64_t num_classes, float pos_weight, int encode,
                             const float* means_host, const float* stds_host, float* rois, int64_t* labels, float* label_weights,
                             float* bbox_targets, float* bbox_weights, int64_t* pos_assigned_gt_inds, int64_t* sample_inds,
                             unsigned char* is_gt, int64_t* num_pos, int64_t* num_neg, float* avg_factor, float* num_samples, void* workspace,
                             void* stream);

/*
 * sph2pob_rcnn_bboxes_f32 — inference of the second stage of a two-stage detector for a whole minibatch, on per-image rois: what
 * SphStandardRoIHead.simple_test_bboxes -> SphShared2FCBBoxHead.get_bboxes -> multiclass_nms compute per image
 * (sphdet/models/heads/sph_rcnn_head.py:127-177, :248-333; sphdet/bbox/nms/utils.py:6-95): softmax over K = C + 1 logits per roi,
 * bbox_coder.decode of the per-class deltas, `scores[:, :-1] > score_thr`, the NMS, [:max_per_img].  Eleven launches whatever B
 * is (the first of the ten behind stage 0 is a zeroing kernel, not a memset); nothing is read back, allocated or kept between
 * calls; no atomics on floats: the same bits on every call; capturable into a hipGraph.  All inputs are read in place:
 *   rois          (B, M, row_stride) f32: the box in columns [0, box_dim), row_stride >= box_dim — the `dets`
 *                 (B, max_per_img, box_dim + 1) of the batched inference entries go in with their score column
 *   num_rois      (B) int64 ON THE DEVICE, each clamped to [0, M] before use (the `num_dets` of those entries); NULL: every image
 *                 has M rois
 *   cls_score     (B, M, K) f32 logits, K = num_logits = C + 1, the background LAST
 *   bbox_pred     (B, M, C box_dim) f32 deltas, class c in columns [c box_dim, (c + 1) box_dim); (B, M, box_dim) with
 *                 reg_class_agnostic = 1; NULL: the head has no regression branch (with_reg = False)
 *   means_host ... ctr_clamp: the delta coder's block, as sph2pob_test_bboxes_f32 takes it (the reference's delta coder accepts
 *                 max_shape and does not use it: it is no argument)
 *   score_thr, variant_flags, class_agnostic, iou_threshold, max_per_img: as sph2pob_test_bboxes_f32 has them
 *   max_candidates  the capacity of an image's candidate block, see "Selection"
 * Score.  The probability of sph2pob_softmax_scores_f32 (csrc/sph2pob_softmax.hpp, Prob: m = max_j x_j, e_j = expf(x_j - m), the sum
 * in double in ascending class order, one divide): the bits that entry writes for the flat (B, M, K) layout.  A row with a NaN or
 * a +inf (or without a finite logit) is NaN in all its classes and yields no candidate; other rows are not touched.
 * Rows behind the count.  Row r >= num_rois[b] yields no candidate whatever score_thr is; its logits and deltas are never read and
 * may be uninitialised (its roi is not read either).
 * Selection.  Candidate (r, c), c < C, has index r C + c and is valid iff p > score_thr.  The reference hands ALL valid candidates
 * to the NMS; this entry the first min(max_candidates, #valid) of them in (probability descending, index ascending) order — the
 * selection of sph2pob_test_bboxes_f32 on one flat level of M rows with nms_pre = max_candidates — and reports #valid:
 *   num_valid     (B) int64: the valid candidates of every image, truncated or not
 * Exactness: greedy NMS decides a candidate from the higher-scored ones alone, and the detections are the kept candidates in
 * descending score order.  So image b's rows equal those of the untruncated computation whenever num_valid[b] <= max_candidates
 * (nothing was cut) OR num_dets[b] == max_per_img (the first max_per_img kept candidates all lie among the best max_candidates;
 * what was cut scores below every one of them and can neither suppress them nor come before them).  Both are device values:
 * a caller checks `(num_valid <= max_candidates) | (num_dets == max_per_img)` without a synchronisation.  With max_candidates >=
 * M min(C, floor(1 / score_thr)) nothing is ever cut (the probabilities of a row sum to 1).
 * Decode.  Only of the selected candidates: roi rois[b, r], deltas bbox_pred[b, r, c box_dim : (c + 1) box_dim] ([0, box_dim) when
 * class-agnostic), the arithmetic of sph2pob_coder_decode_f32.  bbox_pred == NULL: the box is the roi with components 2 and 3
 * clamped to [1e-7, 180 - 1e-7], both bounds narrowed to fp32 as torch's clamp_ narrows them (sph_rcnn_head.py:151-157).
 * NMS and outputs.  Exactly what sph2pob_test_bboxes_f32 does with its candidates: every calculator it serves (STANDARD, EFFICIENT,
 * UNBIASED, NAIVE with or without SPH2POB_FLAG_NAIVE_TAN), class_agnostic = 1 for PlanarNMS; ties by candidate position, which is
 * the index order among equal scores — the order multiclass_nms hands its candidates over in.
 *   dets          (B, max_per_img, box_dim + 1) f32: box and score; rows from num_dets[b] on are 0
 *   labels        (B, max_per_img) int64 in [0, C), -1 from num_dets[b] on
 *   prior_inds    (B, max_per_img) int64: the detection's roi row r, -1 padded
 *   num_dets      (B) int64
 *   workspace     sph2pob_rcnn_bboxes_workspace_bytes(B, M, K, box_dim, max_candidates) bytes, no initialisation (0 = the shapes
 *                 are not accepted): that of sph2pob_get_bboxes_workspace_bytes for one level of M rows with nms_pre =
 *                 max_candidates — 8 B M C bytes of survivor slots and B suppression matrices of min(max_candidates, M C)^2 / 8
 *                 bytes are its large parts — plus 4 B M C bytes of probabilities
 * Errors, checked in this order before anything is enqueued: box_dim -> SPH2POB_ERR_DIM; a variant other than STANDARD | EFFICIENT
 * | UNBIASED | NAIVE, SPH2POB_FLAG_REFERENCE_ORDER or an unknown flag bit, SPH2POB_FLAG_NAIVE_TAN with a variant other than NAIVE,
 * class_agnostic outside {0, 1}, coder_flags, max_ratio < 0, reg_class_agnostic outside {0, 1} -> SPH2POB_ERR_OPTION; B outside
 * [1, 65 535], K outside [2, 4096], max_candidates <= 0, max_per_img < 0, M < 1, row_stride < box_dim, M C >= 2^31 - 2^17,
 * min(max_candidates, M C) > sph2pob_batched_nms_max_boxes() -> SPH2POB_ERR_SIZE; a NULL rois, cls_score, output or workspace ->
 * SPH2POB_ERR_NULL (num_rois, bbox_pred, means_host and stds_host may be NULL).  The CPU twin ignores the workspace.
 */
int64_t sph2pob_rcnn_bboxes_workspace_bytes(int64_t num_images, int64_t m, int64_t num_logits, int box_dim, int64_t max_candidates);
int sph2pob_rcnn_bboxes_f32(const float* rois, const int64_t* num_rois, const float* cls_score, const float* bbox_pred, int64_t num_images,
                            int64_t m, int64_t row_stride, int64_t num_logits, int box_dim, int reg_class_agnostic, float score_thr,
                            int64_t max_candidates, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                            float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                            int64_t* labels, int64_t* prior_inds, int64_t* num_dets, int64_t* num_valid, void* workspace, void* stream);

/*
 * sph2pob_roi_extract_fwd_f32 / sph2pob_roi_extract_bwd_f32 — the RoI feature extractor of the second stage for a whole minibatch:
 * what SphStandardRoIHead._bbox_forward computes in front of the box head (sphdet/models/heads/sph_rcnn_head.py:211-230 with
 * sphdet/bbox/box_formator.py:25-49, :76-83) and SingleRoIExtractor behind it (mmdet/models/roi_heads/roi_extractors/
 * single_level_roi_extractor.py:36-55; RoIAlign of mmcv-full 1.6.0, pool_mode 'avg' — mmcv is not vendored in the reference: its
 * published algorithm, restated below).  Two launches forward, two backward, whatever B and the roi count are; nothing is read
 * back, allocated or kept between calls; capturable into a hipGraph.
 *   feats, heights, widths, strides   HOST tables of num_levels (1 .. 8) entries: the DEVICE pointer of level l, (B, C, H_l, W_l)
 *                 f32 read in place, its H_l, W_l and its stride (spatial_scale = 1 / stride, rounded to fp32 once)
 *   rois          form 0: (rows, row_stride) f32, the image index in column 0 and the box in columns [1, 1 + box_dim), row_stride >=
 *                 1 + box_dim — the reference's flat table;  form 1: (B, M, row_stride) with rows = B M, the box in columns
 *                 [0, box_dim), row_stride >= box_dim, the image is the row's b
 *   num_rois      form 1 only: (B) int64 ON THE DEVICE, each clamped to [0, M] before use, or NULL: every image has M
 *   img_h, img_w  the one img_shape of the batch;  pooled_h, pooled_w in [1, 64];  sampling_ratio >= 0 (0: adaptive);  aligned in
 *                 {0, 1};  finest_scale > 0
 * Per roi (theta, phi, alpha, beta[, gamma]) in degrees, all in fp32, in this order, nothing contracted, division and square root
 * correctly rounded:
 *   x = theta / 360 img_w;  y = phi / 180 img_h;  w = alpha / 360 img_w;  h = beta / 180 img_h
 *   box_dim 5:  a = gamma fl32(pi / 180);  (w, h) <- (|cos a| w + |sin a| h, |sin a| w + |cos a| h)
 *   (x1, y1, x2, y2) = (x - w / 2, y - h / 2, x + w / 2, y + h / 2), y1, y2 clamped to [0, img_h], x1, x2 to [0, img_w]
 *   level = #{k in 1 .. L - 1: fl32(sqrt((x2 - x1)(y2 - y1)) / finest_scale + 1e-6) >= 2^k}: floor(log2(.)) clamped to [0, L - 1]
 *   s = 1 / stride of that level, off = 0.5 if aligned else 0:
 *   sw = x1 s - off; sh = y1 s - off; ew = x2 s - off; eh = y2 s - off; rw = ew - sw; rh = eh - sh (not aligned: each max(., 1))
 *   bin_h = rh / PH; bin_w = rw / PW; gh = sampling_ratio > 0 ? sampling_ratio : (int)ceilf(rh / PH); gw likewise, each held to
 *   [0, 32 768]; count = max(gh gw, 1)
 *   out[c, ph, pw] = (sum over iy < gh, then ix < gw, of bilinear(y = sh + ph bin_h + (iy + .5) bin_h / gh, x likewise)) / count
 *   bilinear: 0 unless -1 <= y <= H and -1 <= x <= W;  y <= 0 -> 0;  y_low = (int)y;  y_low >= H - 1 -> y_high = y_low = H - 1,
 *   y = y_low, else y_high = y_low + 1 (x likewise);  ly = y - y_low, hy = 1 - ly;
 *   hy hx v(lo, lo) + hy lx v(lo, hi) + ly hx v(hi, lo) + ly lx v(hi, hi), added left to right
 * Outputs of the forward:
 *   roi_feats     (rows, C, PH, PW) f32: a fixed-order sum, the same bits on every call
 *   rois_xyxy     (rows, 4) f32: the planar box the reference hands to RoIAlign
 *   levels        (rows) int32
 *   prep          rows x 32 bytes, no initialisation: the roi's record (sw, sh, bin_w, bin_h, gw, gh, image, level), which the
 *                 backward reads in place of the rois.  Whatever it holds, the level, the image and the grid are clamped before use.
 * Zero rows.  A row behind its image's count; a row of form 0 whose image index is not an integer of [0, B); a row with a
 * non-finite box component: zeros in roi_feats, rois_xyxy and levels, no gradient.  Of a row behind the count nothing is read.
 * A roi without extent (gh = 0 or gw = 0) has no sample: zeros in roi_feats.
 * Backward: grad_feats[l] (B, C, H_l, W_l) += every term's weight times grad_out / count, for the records of `prep`, with fp32
 * atomic adds (the summation order is not fixed: the last bits can differ between calls; the CPU twin adds serially in a fixed
 * order).  zero_first = 1: the gradient buffers are zeroed first, by a launch on the same stream.  The gradient flows to the
 * features only, as in mmcv.
 * Errors, checked in this order before anything is enqueued: box_dim -> SPH2POB_ERR_DIM; form, aligned, zero_first outside {0, 1},
 * sampling_ratio < 0, a finest_scale that is not positive and finite -> SPH2POB_ERR_OPTION; img_h, img_w < 1, a row_stride
 * too small, form 1 with B M != rows -> SPH2POB_ERR_SIZE; num_levels outside [1, 8], pooled_h, pooled_w outside [1, 64], a stride that
 * is not positive and finite -> SPH2POB_ERR_OPTION; negative rows, B or C, rows >= 2^31, B > 2^24, C > 2^20, H_l, W_l outside
 * [1, 2^20], a level above 2^40 elements -> SPH2POB_ERR_SIZE; rows, B or C zero: SPH2POB_OK, nothing enqueued; a NULL table, level,
 * rois, grad_out, output or prep -> SPH2POB_ERR_NULL (num_rois may be NULL).
 */
int sph2pob_roi_extract_fwd_f32(const float* const* feats, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                                int64_t num_images, int64_t channels, const float* rois, int64_t rows, int64_t row_stride, int form, int64_t m,
                                const int64_t* num_rois, int box_dim, int64_t img_h, int64_t img_w, int pooled_h, int pooled_w,
                                int sampling_ratio, int aligned, float finest_scale, float* roi_feats, float* rois_xyxy, int32_t* levels,
                                void* prep, void* stream);
int sph2pob_roi_extract_bwd_f32(float* const* grad_feats, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                                int64_t num_images, int64_t channels, const float* grad_out, int64_t rows, int box_dim, int pooled_h, int pooled_w,
                                const void* prep, int zero_first, void* stream);

/* ---- fused box loss of the R-CNN head on its per-class deltas: the regression half of SphShared2FCBBoxHead.loss ---------------
 * Replaces (sphdet/models/heads/sph_rcnn_head.py:97-124) pos_inds = (labels >= 0) & (labels < C) ->
 * bbox_pred.view(S, -1, dim)[pos_inds, labels[pos_inds]] (-> bbox_coder.decode with reg_decoded_bbox) -> loss_bbox(..., weights,
 * avg_factor) and its backward — the index backward builds a zero tensor and scatters into it — by one pass over the Linear
 * head's output where it is.  The arguments both entries share:
 *   bbox_pred    (rows, num_slots * dim) f32: slot c of row r holds the deltas of class c
 *   grad         NULL (forward only), or (rows, num_slots * dim): the gradient of out[0] for an upstream gradient of 1.  EVERY
 *                element is written, exactly once: zeros, and a live row's dim values in its label's slot
 *   rows         S >= 0;  num_slots: num_classes, or 1 (reg_class_agnostic: every class reads slot 0);  num_classes: C >= 1
 *   labels       (rows) int64.  A row takes part when 0 <= label < C AND the family's weight rule holds; any other label
 *                (background C, ignore -1, ...) makes a dead row whatever its weight is — the reference's pos_inds, not a clamp
 *   targets      (rows, dim);  weight: NULL (all ones), (rows) when weight_dim == 1, (rows, dim) when weight_dim == dim
 *   scale, avg_factor, out, workspace   as for sph2pob_bbox_loss_sum_f32; workspace holds
 *                sph2pob_rcnn_loss_workspace_bytes(rows, num_slots, box_dim) bytes (0: shape not accepted), for either entry
 * sph2pob_rcnn_delta_loss_sum_f32 — L1 / SmoothL1 on ENCODED deltas: beta, the element function, the weight rule (any component
 *   != 0) and the product (scale_eff * w_k) * s_k are those of sph2pob_delta_loss_sum_f32.
 * sph2pob_rcnn_bbox_loss_sum_f32 — decode + IoU-family loss: means_host ... eps, the weight rule (row mean != 0) and the product
 *   ((scale_eff * w) * dL/dbox_k) * J_k are those of sph2pob_bbox_loss_sum_f32; the box a row's deltas are applied to is
 *   rois[r * roi_stride + roi_offset + k], k < dim: (rows, 1 + dim) rois with the image index in front are read in place with
 *   roi_stride = 1 + dim, roi_offset = 1; plain (rows, dim) boxes with (dim, 0).
 * On the selected slots the gradient has the BITS sph2pob_delta_loss_sum_f32 / sph2pob_bbox_loss_sum_f32 give on the gathered
 * rows as one flattened level (B = 1); out[0] differs from theirs by the order of the double partials only.  A dead row is NEVER
 * READ in bbox_pred, targets or rois, and of a live row only the label's slot is: NaN or Inf elsewhere stays inert; a dead row's
 * loss and whole gradient row are exact +0.0f.  Two launches; nothing is read back, nothing is allocated; capturable.  The
 * gradient leaves in whole 16-byte stores when grad is 16-byte aligned and num_slots * dim is a multiple of 4, one element at a
 * time with the same values otherwise.  rows == 0 writes out[0] = 0.
 * Errors, checked in this order before anything is enqueued: the option checks of the flat sibling with its codes (delta: box_dim
 * -> SPH2POB_ERR_DIM, weight_dim, beta -> SPH2POB_ERR_OPTION; bbox: loss_mode flags -> OPTION, box_dim -> DIM, loss mode,
 * weight_dim, coder_flags, max_ratio -> OPTION); num_classes outside [1, 20 480], num_slots < 1 or neither 1 nor num_classes ->
 * SPH2POB_ERR_OPTION; rows < 0, num_slots * dim > 4096 * 5, rows * num_slots * dim >= 2^31 - 4096 -> SPH2POB_ERR_SIZE;
 * roi_offset < 0 or roi_stride < roi_offset + dim -> SPH2POB_ERR_SIZE; a NULL out or workspace, or bbox_pred, labels, targets
 * or rois with rows -> SPH2POB_ERR_NULL.
 */
int64_t sph2pob_rcnn_loss_workspace_bytes(int64_t rows, int64_t num_slots, int box_dim);
int sph2pob_rcnn_delta_loss_sum_f32(const float* bbox_pred, float* grad, int64_t rows, int64_t num_slots, int64_t num_classes, int box_dim,
                                    const int64_t* labels, const float* targets, const float* weight, int weight_dim, float beta,
                                    float scale, const float* avg_factor, float* out, void* workspace, void* stream);
int sph2pob_rcnn_bbox_loss_sum_f32(const float* bbox_pred, float* grad, int64_t rows, int64_t num_slots, int64_t num_classes, int box_dim,
                                   const int64_t* labels, const float* rois, int64_t roi_stride, int64_t roi_offset, const float* targets,
                                   const float* weight, int weight_dim, const float* means_host, const float* stds_host, float max_ratio,
                                   int coder_flags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
                                   float* out, void* workspace, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SPH2POB_HIP_H */
