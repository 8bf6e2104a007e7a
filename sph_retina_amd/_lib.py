"""ctypes binding of libsph2pob_hip.so (the C ABI declared in include/sph2pob_hip.h).

No torch extension and no silent fallback: if a shared library is missing or a symbol is absent the product fails
loudly.  ``build()`` cross-compiles libsph2pob_hip.so for gfx950 with hipcc (works without a GPU) and compiles
libsph2pob_host.so — the CPU twins (`*_cpu`) of the same entry points, the product's own __host__ __device__ arithmetic
instantiated for the host (csrc/sph2pob_host.hip) — with the same compiler; both live in-tree under
sph_retina_amd/lib/ so they travel with the source tree.  CPU tensors are served by the host library, device tensors by
the HIP one; neither ever touches oracle/.
"""
import ctypes
import os
import shutil
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, 'csrc')
LIB_DIR = os.path.join(_HERE, 'lib')
LIB_PATH = os.path.join(LIB_DIR, 'libsph2pob_hip.so')
HOST_LIB_PATH = os.path.join(LIB_DIR, 'libsph2pob_host.so')
SOURCES = ['sph2pob_iou.hip', 'sph2pob_assign.hip', 'sph2pob_loss.hip', 'sph2pob_nms.hip', 'sph2pob_coder.hip', 'sph2pob_get_bboxes.hip',
           'sph2pob_focal.hip', 'sph2pob_bbox_loss.hip', 'sph2pob_delta_loss.hip', 'sph2pob_gauss_bbox_loss.hip', 'sph2pob_softmax.hip', 'sph2pob_softmax_bboxes.hip', 'sph2pob_sample.hip',
           'sph2pob_point_targets.hip', 'sph2pob_point_bbox_loss.hip', 'sph2pob_bce_loss.hip', 'sph2pob_rcnn_targets.hip', 'sph2pob_rcnn_bboxes.hip', 'sph2pob_roi_extract.hip', 'sph2pob_rcnn_loss.hip']
HOST_SOURCES = ['sph2pob_host.hip']
HOST_FLAGS = ['--offload-arch=gfx950', '--cuda-host-only', '-O2', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off', '-pthread']


def _host_has_fma():
    try:
        with open('/proc/cpuinfo') as f:
            return any(line.startswith('flags') and ' fma ' in line + ' ' for line in f)
    except OSError:
        return False


# the twins' explicit fmaf() calls (the kernels' v_fma_f32) as the hardware instruction instead of a libm call per product:
# the same bits (both round once), 1.6x the pairs per second per core.  Every MI355X host has it; a build machine without it
# keeps the libm call.
if _host_has_fma():
    HOST_FLAGS.append('-mfma')
# the entry points that have a CPU twin `<name>_cpu` with the same signature (the stream argument is ignored)
HOST_TWINS = ['sph2pob_iou_aligned_f32', 'sph2pob_iou_pairwise_f32', 'sph2pob_planar_iou_f32', 'sph2pob_transform_f32',
              'sph2pob_transform_bwd_f32', 'sph2pob_transform_bwd_general_f32', 'sph2pob_loss_fwd_f32', 'sph2pob_loss_bwd_f32',
              'sph2pob_loss_fwd_sum_f32', 'sph2pob_loss_fwd_grad_f32', 'sph2pob_loss_grad_scale_f32', 'sph2pob_sum_f32',
              'sph2pob_nms_segmented_f32', 'sph2pob_nms_f32', 'sph2pob_assign_f32', 'sph2pob_coder_encode_f32',
              'sph2pob_coder_decode_f32', 'sph2pob_coder_decode_bwd_f32', 'sph2pob_obb_l1_fwd_f32', 'sph2pob_obb_l1_bwd_f32',
              'sph2pob_gauss_loss_fwd_f32', 'sph2pob_gauss_loss_bwd_f32', 'sph2pob_gauss_loss_fwd_sum_f32',
              'sph2pob_gauss_loss_fwd_grad_f32', 'sph2pob_anchor_targets_f32', 'sph2pob_anchor_targets_any_f32', 'sph2pob_get_bboxes_f32', 'sph2pob_test_bboxes_f32', 'sph2pob_focal_loss_sum_f32',
              'sph2pob_focal_loss_fwd_f32', 'sph2pob_focal_loss_bwd_f32', 'sph2pob_focal_loss_grad_scale_f32', 'sph2pob_bbox_loss_sum_f32',
              'sph2pob_delta_loss_sum_f32', 'sph2pob_gauss_bbox_loss_sum_f32', 'sph2pob_softmax_loss_sum_f32',
              'sph2pob_softmax_loss_fwd_f32', 'sph2pob_softmax_loss_bwd_f32', 'sph2pob_softmax_scores_f32', 'sph2pob_softmax_bboxes_f32',
              'sph2pob_sample_targets_f32', 'sph2pob_point_targets_f32', 'sph2pob_point_coder_encode_f32', 'sph2pob_point_coder_decode_f32',
              'sph2pob_point_coder_decode_bwd_f32', 'sph2pob_fcos_bboxes_f32', 'sph2pob_point_bbox_loss_sum_f32', 'sph2pob_bce_loss_sum_f32',
              'sph2pob_rcnn_targets_f32', 'sph2pob_rcnn_bboxes_f32', 'sph2pob_roi_extract_fwd_f32', 'sph2pob_roi_extract_bwd_f32',
              'sph2pob_rcnn_delta_loss_sum_f32', 'sph2pob_rcnn_bbox_loss_sum_f32']
HEADERS = ['sph2pob_device.hpp', 'sph2pob_loss.hpp', 'sph2pob_fast.hpp', 'sph2pob_unbiased.hpp', 'sph2pob_coder.hpp', 'sph2pob_get_bboxes.hpp', 'sph2pob_assign.hpp', 'sph2pob_head_loss.hpp', 'sph2pob_focal.hpp', 'sph2pob_bbox_loss.hpp', 'sph2pob_delta_loss.hpp', 'sph2pob_span_loss.hpp', 'sph2pob_gauss_bbox_loss.hpp', 'sph2pob_softmax.hpp', 'sph2pob_sample.hpp',
           'sph2pob_point_targets.hpp', 'sph2pob_point_bbox_loss.hpp', 'sph2pob_bce_loss.hpp', 'sph2pob_rcnn_targets.hpp', 'sph2pob_rcnn_bboxes.hpp', 'sph2pob_roi_extract.hpp', 'sph2pob_rcnn_loss.hpp', 'sph2pob_class_levels.hpp', 'sph2pob_select.hpp', 'sph2pob_kernels_common.hpp', 'sph2pob_iou_entry.hpp', os.path.join('..', '..', 'include', 'sph2pob_hip.h')]
# -fno-slp-vectorize: hipcc otherwise pairs scalar fp32 mul/add into v_pk_* (+ v_mov shuffles); packed fp32 issues at
# half the rate of plain VALU on gfx950 (tools/ubench/valu_rate2.hip), measured 12 % slower on the dominant kernel
# -amdgpu-kernarg-preload-count: gfx950 hands the first kernel arguments to a wave in SGPRs at launch instead of making
# every wave fetch them with s_load (two dependent scalar loads stood in front of the first global load of the dominant
# kernel): 8.24 -> 8.04 us per 1 M pairs, 4.29 -> 4.11 at 250 k (profiles/r02w_ab_*.log); the compiler keeps a
# compatible entry for firmware without the feature
HIPCC_FLAGS = ['--offload-arch=gfx950', '-O3', '-std=c++17', '-fPIC', '-shared', '-ffp-contract=off',
               '-fno-slp-vectorize', '-mllvm', '-amdgpu-kernarg-preload-count=16'] + \
    os.environ.get('SPH2POB_EXTRA_HIPCC_FLAGS', '').split()

_c_f32p = ctypes.c_void_p
_i64 = ctypes.c_int64
_int = ctypes.c_int
_GAUSS_TAIL = [_int, _int, ctypes.c_float, ctypes.c_float, _int, ctypes.c_float, ctypes.c_float, ctypes.c_void_p]

# name -> argtypes (restype is always int unless listed in _RESTYPES); mirrors include/sph2pob_hip.h
SIGNATURES = {
    'sph2pob_abi_version': [],
    'sph2pob_target_arch': [],
    'sph2pob_error_string': [_int],
    'sph2pob_iou_aligned_f32': [_c_f32p, _c_f32p, _c_f32p, _i64, _int, _int, _int, _int, _int, ctypes.c_void_p],
    'sph2pob_iou_pairwise_f32': [_c_f32p, _i64, _c_f32p, _i64, _c_f32p, _int, _int, _int, _int, _int,
                                 ctypes.c_void_p],
    'sph2pob_planar_iou_f32': [_c_f32p, _i64, _c_f32p, _i64, _c_f32p, _int, _int, ctypes.c_void_p],
    'sph2pob_transform_f32': [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _i64, _int, _int, _int, _int, _int,
                              ctypes.c_void_p],
    'sph2pob_transform_bwd_f32': [_c_f32p] * 6 + [_i64, _int, _int, _int, _int, ctypes.c_void_p],
    'sph2pob_transform_bwd_general_f32': [_c_f32p] * 6 + [_i64, _int, _int, _int, _int, _int, ctypes.c_void_p],
    'sph2pob_loss_fwd_f32': [_c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p, _i64, _int, _int,
                             ctypes.c_float,
                             ctypes.c_void_p],
    'sph2pob_loss_bwd_f32': [_c_f32p, _c_f32p, _c_f32p, _int, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p, _i64,
                             _int, _int, ctypes.c_float, ctypes.c_void_p],
    'sph2pob_loss_sum_workspace_floats': [_i64],
    'sph2pob_loss_fwd_sum_f32': [_c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p, _i64, _int, _int,
                                 ctypes.c_float, ctypes.c_void_p],
    'sph2pob_loss_fwd_grad_f32': [_c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                  _i64, _int, _int, ctypes.c_float, ctypes.c_void_p],
    'sph2pob_loss_grad_scale_f32': [_c_f32p, _c_f32p, _int, _c_f32p, _i64, _int, ctypes.c_void_p],
    # Gaussian losses: the sph2pob_loss_* leading arguments, then (type_flags, fun, tau, alpha, opts, beta, eps)
    'sph2pob_gauss_loss_fwd_f32': [_c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_float, _c_f32p, _i64, _int] + _GAUSS_TAIL,
    'sph2pob_gauss_loss_bwd_f32': [_c_f32p, _c_f32p, _c_f32p, _int, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p, _i64,
                                   _int] + _GAUSS_TAIL,
    'sph2pob_gauss_loss_fwd_sum_f32': [_c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p, _i64, _int] +
                                      _GAUSS_TAIL,
    'sph2pob_gauss_loss_fwd_grad_f32': [_c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p, _c_f32p, _c_f32p,
                                        _c_f32p, _i64, _int] + _GAUSS_TAIL,
    'sph2pob_sum_workspace_floats': [],
    'sph2pob_sum_f32': [_c_f32p, _i64, ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_void_p],
    'sph2pob_assign_workspace_bytes': [_i64, _i64],
    'sph2pob_assign_f32': [_c_f32p, _i64, _i64, ctypes.c_float, ctypes.c_float, ctypes.c_float, ctypes.c_float, _int, _int,
                           ctypes.c_void_p] + [ctypes.c_void_p] * 7 + [ctypes.c_void_p],
    'sph2pob_iou_assign_workspace_bytes': [_i64, _i64],
    'sph2pob_iou_assign_reduce_f32': [_c_f32p, _i64, _c_f32p, _i64, _int, _int, _int, ctypes.c_void_p, _i64, _c_f32p,
                                      ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_iou_assign_finalize_f32': [_c_f32p, _i64, _c_f32p, _i64, _int, _int, _int, _i64, ctypes.c_void_p] +
                                       [ctypes.c_float] * 4 + [_int, _int] + [ctypes.c_void_p] * 9,
    'sph2pob_iou_assign_f32': [_c_f32p, _i64, _c_f32p, _i64, _int, _int, _int, ctypes.c_void_p, _c_f32p] +
                              [ctypes.c_float] * 4 + [_int, _int] + [ctypes.c_void_p] * 10,
    'sph2pob_iou_assign_state_bytes': [_i64, _i64],
    'sph2pob_anchor_targets_workspace_bytes': [_i64, _i64, _i64, _i64],
    'sph2pob_anchor_targets_state_bytes': [_i64, _i64, _i64],
    # anchors, n, gt, gt_labels, gt_offsets, num_images, num_gt, k_max, box_dim, variant, edge, 4 thresholds, 2 flags, num_classes,
    # pos_weight, encode, means, stds, 10 outputs, workspace, state, stream
    'sph2pob_anchor_targets_f32': [_c_f32p, _i64, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _i64, _i64, _i64, _int, _int, _int] +
                                  [ctypes.c_float] * 4 + [_int, _int, _i64, ctypes.c_float, _int] + [ctypes.c_void_p] * 15,
    # the same arguments, for the variants without a closed form
    'sph2pob_anchor_targets_any_f32': [_c_f32p, _i64, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _i64, _i64, _i64, _int, _int, _int] +
                                      [ctypes.c_float] * 4 + [_int, _int, _i64, ctypes.c_float, _int] + [ctypes.c_void_p] * 15,
    'sph2pob_nms_max_boxes': [],
    'sph2pob_nms_workspace_bytes': [_i64],
    'sph2pob_nms_f32': [_c_f32p, ctypes.c_void_p, _i64, _int, _int, ctypes.c_float, ctypes.c_void_p, ctypes.c_void_p,
                        ctypes.c_void_p],
    'sph2pob_nms_segmented_workspace_bytes': [_i64, _i64],
    'sph2pob_nms_segmented_f32': [_c_f32p, ctypes.c_void_p, _i64, _int, _int, ctypes.c_float, _i64, ctypes.c_void_p,
                                  ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_batched_nms_max_boxes': [],
    'sph2pob_batched_nms_workspace_bytes': [_i64, _int],
    'sph2pob_batched_nms_f32': [_c_f32p, _c_f32p, ctypes.c_void_p, _i64, _int, _int, ctypes.c_float, _i64] + [ctypes.c_void_p] * 5,
    'sph2pob_get_bboxes_workspace_bytes': [ctypes.c_void_p, _int, _i64, _i64, _int, _i64],
    # level tables (cls, bbox, anchors, n, hw), num_levels, B, C, box_dim, activation, score_thr, nms_pre, means, stds, max_ratio,
    # coder_flags, ctr_clamp, variant, iou_threshold, max_per_img, 4 outputs, workspace, stream
    'sph2pob_get_bboxes_f32': [ctypes.c_void_p] * 5 + [_int, _i64, _i64, _int, _int, ctypes.c_float, _i64, ctypes.c_void_p, ctypes.c_void_p,
                               ctypes.c_float, _int, ctypes.c_float, _int, ctypes.c_float, _i64] + [ctypes.c_void_p] * 6,
    # the same with (variant_flags, class_agnostic) in place of variant
    'sph2pob_test_bboxes_f32': [ctypes.c_void_p] * 5 + [_int, _i64, _i64, _int, _int, ctypes.c_float, _i64, ctypes.c_void_p, ctypes.c_void_p,
                                ctypes.c_float, _int, ctypes.c_float, _int, _int, ctypes.c_float, _i64] + [ctypes.c_void_p] * 6,
    'sph2pob_focal_loss_workspace_bytes': [ctypes.c_void_p, ctypes.c_void_p, _int, _i64, _i64],
    # level tables (logits, grads, n, hw), num_levels, B, C, labels, weight, weight_mode, gamma, alpha, scale, avg_factor, out,
    # workspace, stream
    'sph2pob_focal_loss_sum_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _i64, ctypes.c_void_p, _c_f32p, _int] + [ctypes.c_float] * 3 +
                                  [_c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_focal_loss_fwd_f32': [_c_f32p, ctypes.c_void_p, _c_f32p, _int] + [ctypes.c_float] * 3 + [_c_f32p, _i64, _i64, ctypes.c_void_p],
    'sph2pob_focal_loss_bwd_f32': [_c_f32p, ctypes.c_void_p, _c_f32p, _int, _c_f32p, _int] + [ctypes.c_float] * 3 +
                                  [_c_f32p, _c_f32p, _i64, _i64, ctypes.c_void_p],
    'sph2pob_focal_loss_grad_scale_f32': [_c_f32p, _c_f32p, _c_f32p, _i64, ctypes.c_void_p],
    'sph2pob_bbox_loss_workspace_bytes': [ctypes.c_void_p, ctypes.c_void_p, _int, _i64, _int],
    # level tables (bbox_preds, grads, n, hw), num_levels, B, box_dim, anchors, targets, weight, weight_dim, means, stds, max_ratio,
    # coder_flags, ctr_clamp, loss_mode, eps, scale, avg_factor, out, workspace, stream
    'sph2pob_bbox_loss_sum_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _int, _c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_float, _int, ctypes.c_float, _int, ctypes.c_float, ctypes.c_float, _c_f32p, _c_f32p,
                                  ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_gauss_bbox_loss_workspace_bytes': [ctypes.c_void_p, ctypes.c_void_p, _int, _i64, _int],
    # the arguments of sph2pob_bbox_loss_sum_f32 up to ctr_clamp, the Gaussian tail (type_flags, fun, tau, alpha, opts, beta, eps),
    # then scale, avg_factor, out, workspace, stream
    'sph2pob_gauss_bbox_loss_sum_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _int, _c_f32p, _c_f32p, _c_f32p, _int, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_float, _int, ctypes.c_float] + _GAUSS_TAIL[:-1] +
                                       [ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_delta_loss_workspace_bytes': [ctypes.c_void_p, ctypes.c_void_p, _int, _i64, _int],
    # level tables (bbox_preds, grads, n, hw), num_levels, B, box_dim, targets, weight, weight_dim, beta, scale, avg_factor, out,
    # workspace, stream
    'sph2pob_delta_loss_sum_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _int, _c_f32p, _c_f32p, _int, ctypes.c_float, ctypes.c_float,
                                   _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_softmax_loss_workspace_bytes': [ctypes.c_void_p, ctypes.c_void_p, _int, _i64, _i64, _int],
    # level tables (logits, grads, n, hw), num_levels, B, K, labels, weight, class_weight, ignore_index, background_label,
    # neg_pos_ratio (-1: plain), scale, avg_factor, out, workspace, stream
    'sph2pob_softmax_loss_sum_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _i64, ctypes.c_void_p, _c_f32p, _c_f32p, _i64, _i64, _i64,
                                    ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_softmax_loss_fwd_f32': [_c_f32p, ctypes.c_void_p, _c_f32p, _c_f32p, _i64, ctypes.c_float, _c_f32p, _i64, _i64, ctypes.c_void_p],
    'sph2pob_softmax_loss_bwd_f32': [_c_f32p, ctypes.c_void_p, _c_f32p, _c_f32p, _i64, _c_f32p, _int, ctypes.c_float, _c_f32p, _c_f32p,
                                    _i64, _i64, ctypes.c_void_p],
    # level tables (logits, n, hw), num_levels, B, C, output table, stream
    'sph2pob_softmax_scores_f32': [ctypes.c_void_p] * 3 + [_int, _i64, _i64, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_softmax_bboxes_workspace_bytes': [ctypes.c_void_p, _int, _i64, _i64, _int, _i64],
    # sph2pob_test_bboxes_f32 without `activation`
    'sph2pob_softmax_bboxes_f32': [ctypes.c_void_p] * 5 + [_int, _i64, _i64, _int, ctypes.c_float, _i64, ctypes.c_void_p, ctypes.c_void_p,
                                   ctypes.c_float, _int, ctypes.c_float, _int, _int, ctypes.c_float, _i64] + [ctypes.c_void_p] * 6,
    'sph2pob_sample_targets_workspace_bytes': [_i64, _i64],
    # gt_inds, B, n, box_dim, the four input targets, num_classes, num_expected_pos, num, neg_pos_ub, seed, seed_device, ranks, the four
    # output targets, sample_flags, num_pos, num_neg, avg_factor, avg_factor_pos, workspace, stream
    'sph2pob_sample_targets_f32': [ctypes.c_void_p, _i64, _i64, _int] + [ctypes.c_void_p] * 4 + [_i64, _i64, _i64, ctypes.c_double, _i64] +
                                  [ctypes.c_void_p] * 13,
    'sph2pob_point_targets_workspace_bytes': [_i64, _i64],
    # points, P, the level table (n, range_lo, range_hi, sample_extent, norm_stride), num_levels, gt, gt_labels, gt_offsets, B, num_gt, k_max,
    # box_dim, img_h, img_w, num_classes, flags, 7 outputs, workspace, stream
    'sph2pob_point_targets_f32': [_c_f32p, _i64] + [ctypes.c_void_p] * 5 + [_int, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _i64, _i64, _i64, _int,
                                                                              _i64, _i64, _i64, _int] + [ctypes.c_void_p] * 9,
    # points, gt, distances, n, box_dim, img_h, img_w, clamp, max_dis, eps, stream
    'sph2pob_point_coder_encode_f32': [_c_f32p, _c_f32p, _c_f32p, _i64, _int, _i64, _i64, _int, ctypes.c_double, ctypes.c_double, ctypes.c_void_p],
    # points, distances, [grad_boxes,] out, n, box_dim, img_h, img_w, max_h, max_w, stream
    'sph2pob_point_coder_decode_f32': [_c_f32p, _c_f32p, _c_f32p, _i64, _int, _i64, _i64, ctypes.c_float, ctypes.c_float, ctypes.c_void_p],
    'sph2pob_point_coder_decode_bwd_f32': [_c_f32p, _c_f32p, _c_f32p, _c_f32p, _i64, _int, _i64, _i64, ctypes.c_float, ctypes.c_float, ctypes.c_void_p],
    # level tables (cls, bbox, points, centernesses, n, hw), num_levels, B, C, box_dim, activation, score_thr, nms_pre, img_h, img_w, max_h,
    # max_w, variant_flags, class_agnostic, iou_threshold, max_per_img, 4 outputs, workspace, stream
    'sph2pob_fcos_bboxes_f32': [ctypes.c_void_p] * 6 + [_int, _i64, _i64, _int, _int, ctypes.c_float, _i64, _i64, _i64, ctypes.c_float,
                                ctypes.c_float, _int, _int, ctypes.c_float, _i64] + [ctypes.c_void_p] * 6,
    'sph2pob_point_bbox_loss_workspace_bytes': [ctypes.c_void_p, ctypes.c_void_p, _int, _i64, _int],
    # level tables (bbox_preds, grads, n, hw), num_levels, B, box_dim, points, targets, weight, weight_dim, img_h, img_w, max_h, max_w,
    # loss_mode, eps, scale, avg_factor, out, workspace, stream
    'sph2pob_point_bbox_loss_sum_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _int, _c_f32p, _c_f32p, _c_f32p, _int, _i64, _i64, ctypes.c_float,
                                        ctypes.c_float, _int, ctypes.c_float, ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_void_p,
                                        ctypes.c_void_p],
    'sph2pob_bce_loss_workspace_bytes': [ctypes.c_void_p, ctypes.c_void_p, _int, _i64, _i64],
    # level tables (logits, grads, n, hw), num_levels, B, C, targets, labels, weight, weight_mode, ignore_index, scale, avg_factor, out,
    # workspace, stream
    'sph2pob_bce_loss_sum_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _i64, _c_f32p, ctypes.c_void_p, _c_f32p, _int, _i64, ctypes.c_float,
                                 _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_rcnn_targets_workspace_bytes': [_i64, _i64, _i64],
    # proposals, num_proposals, B, M, row_stride, gt, gt_labels, gt_offsets, num_gt, k_max, box_dim, variant, edge, 4 thresholds, 2 flags,
    # num, num_expected_pos, neg_pos_ub, seed, seed_device, ranks, add_gt, num_classes, pos_weight, encode, means, stds, 12 outputs,
    # workspace, stream
    'sph2pob_rcnn_targets_f32': [_c_f32p, ctypes.c_void_p, _i64, _i64, _i64, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _i64, _i64, _int, _int,
                                 _int] + [ctypes.c_float] * 4 + [_int, _int, _i64, _i64, ctypes.c_double, _i64, ctypes.c_void_p, ctypes.c_void_p,
                                                                 _int, _i64, ctypes.c_float, _int] + [ctypes.c_void_p] * 16,
    'sph2pob_rcnn_bboxes_workspace_bytes': [_i64, _i64, _i64, _int, _i64],
    # rois, num_rois, cls_score, bbox_pred, B, M, row_stride, K, box_dim, reg_class_agnostic, score_thr, max_candidates, means, stds,
    # max_ratio, coder_flags, ctr_clamp, variant_flags, class_agnostic, iou_threshold, max_per_img, 5 outputs, workspace, stream
    'sph2pob_rcnn_bboxes_f32': [_c_f32p, ctypes.c_void_p, _c_f32p, _c_f32p, _i64, _i64, _i64, _i64, _int, _int, ctypes.c_float, _i64,
                                ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, _int, ctypes.c_float, _int, _int, ctypes.c_float, _i64] +
                               [ctypes.c_void_p] * 7,
    # level tables (feats, heights, widths, strides), num_levels, B, C, rois, rows, row_stride, form, M, num_rois, box_dim, img_h, img_w,
    # pooled_h, pooled_w, sampling_ratio, aligned, finest_scale, roi_feats, rois_xyxy, levels, prep, stream
    'sph2pob_roi_extract_fwd_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _i64, _c_f32p, _i64, _i64, _int, _i64, ctypes.c_void_p, _int, _i64, _i64,
                                    _int, _int, _int, _int, ctypes.c_float] + [ctypes.c_void_p] * 5,
    # level tables (grad_feats, heights, widths, strides), num_levels, B, C, grad_out, rows, box_dim, pooled_h, pooled_w, prep, zero_first, stream
    'sph2pob_roi_extract_bwd_f32': [ctypes.c_void_p] * 4 + [_int, _i64, _i64, _c_f32p, _i64, _int, _int, _int, ctypes.c_void_p, _int, ctypes.c_void_p],
    'sph2pob_rcnn_loss_workspace_bytes': [_i64, _i64, _int],
    # bbox_pred, grad, rows, num_slots, num_classes, box_dim, labels, targets, weight, weight_dim, beta, scale, avg_factor, out,
    # workspace, stream
    'sph2pob_rcnn_delta_loss_sum_f32': [_c_f32p, _c_f32p, _i64, _i64, _i64, _int, ctypes.c_void_p, _c_f32p, _c_f32p, _int, ctypes.c_float,
                                        ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p],
    # bbox_pred, grad, rows, num_slots, num_classes, box_dim, labels, rois, roi_stride, roi_offset, targets, weight, weight_dim, means,
    # stds, max_ratio, coder_flags, ctr_clamp, loss_mode, eps, scale, avg_factor, out, workspace, stream
    'sph2pob_rcnn_bbox_loss_sum_f32': [_c_f32p, _c_f32p, _i64, _i64, _i64, _int, ctypes.c_void_p, _c_f32p, _i64, _i64, _c_f32p, _c_f32p, _int,
                                       ctypes.c_void_p, ctypes.c_void_p, ctypes.c_float, _int, ctypes.c_float, _int, ctypes.c_float,
                                       ctypes.c_float, _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p],
    'sph2pob_coder_encode_f32': [_c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _c_f32p, _i64, _int,
                                 ctypes.c_void_p],
    'sph2pob_coder_decode_f32': [_c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _c_f32p, _i64, _int, _int,
                                 ctypes.c_float, _int, ctypes.c_float, ctypes.c_void_p],
    'sph2pob_coder_decode_bwd_f32': [_c_f32p, _c_f32p, _c_f32p, ctypes.c_void_p, ctypes.c_void_p, _c_f32p, _i64, _int,
                                     _int, ctypes.c_float, _int, ctypes.c_float, ctypes.c_void_p],
    'sph2pob_obb_l1_fwd_f32': [_c_f32p, _c_f32p, _c_f32p, ctypes.c_float, _c_f32p, _i64, _int, ctypes.c_void_p],
    'sph2pob_obb_l1_bwd_f32': [_c_f32p, _c_f32p, _c_f32p, _c_f32p, ctypes.c_float, _c_f32p, _c_f32p, _i64, _int,
                               ctypes.c_void_p],
}
# The 16-bit level entries (SPH2POB_DTYPE_*; no CPU twins): the arguments of the _f32 sibling with `dtype` in front of the stream,
# and for the losses (grad_out, skip_if_one) in front of that
H16_DTYPES = {'float16': 1, 'bfloat16': 2}
for _name in ('focal_loss_sum', 'bbox_loss_sum', 'delta_loss_sum', 'gauss_bbox_loss_sum'):
    SIGNATURES[f'sph2pob_{_name}_h16'] = SIGNATURES[f'sph2pob_{_name}_f32'][:-1] + [_c_f32p, _int, _int, ctypes.c_void_p]
for _name in ('get_bboxes', 'test_bboxes', 'softmax_scores', 'softmax_bboxes', 'fcos_bboxes'):
    SIGNATURES[f'sph2pob_{_name}_h16'] = SIGNATURES[f'sph2pob_{_name}_f32'][:-1] + [_int, ctypes.c_void_p]
_RESTYPES = {'sph2pob_loss_sum_workspace_floats': ctypes.c_int64, 'sph2pob_target_arch': ctypes.c_char_p, 'sph2pob_error_string': ctypes.c_char_p,
             'sph2pob_nms_workspace_bytes': ctypes.c_int64, 'sph2pob_nms_segmented_workspace_bytes': ctypes.c_int64, 'sph2pob_assign_workspace_bytes': ctypes.c_int64,
             'sph2pob_iou_assign_workspace_bytes': ctypes.c_int64, 'sph2pob_iou_assign_state_bytes': ctypes.c_int64,
             'sph2pob_anchor_targets_workspace_bytes': ctypes.c_int64, 'sph2pob_anchor_targets_state_bytes': ctypes.c_int64,
             'sph2pob_batched_nms_workspace_bytes': ctypes.c_int64, 'sph2pob_get_bboxes_workspace_bytes': ctypes.c_int64,
             'sph2pob_focal_loss_workspace_bytes': ctypes.c_int64, 'sph2pob_bbox_loss_workspace_bytes': ctypes.c_int64,
             'sph2pob_delta_loss_workspace_bytes': ctypes.c_int64, 'sph2pob_gauss_bbox_loss_workspace_bytes': ctypes.c_int64,
             'sph2pob_softmax_loss_workspace_bytes': ctypes.c_int64, 'sph2pob_softmax_bboxes_workspace_bytes': ctypes.c_int64,
             'sph2pob_sample_targets_workspace_bytes': ctypes.c_int64, 'sph2pob_point_targets_workspace_bytes': ctypes.c_int64,
             'sph2pob_point_bbox_loss_workspace_bytes': ctypes.c_int64, 'sph2pob_bce_loss_workspace_bytes': ctypes.c_int64,
             'sph2pob_rcnn_targets_workspace_bytes': ctypes.c_int64, 'sph2pob_rcnn_bboxes_workspace_bytes': ctypes.c_int64,
             'sph2pob_rcnn_loss_workspace_bytes': ctypes.c_int64}

# Entry points of libsph2pob_host.so alone, `<name>_cpu`: the CPU statement of a route that has no device entry yet, so the name is
# neither declared in include/sph2pob_hip.h nor exported by libsph2pob_hip.so.  name -> argtypes
# sph2pob_roi_extract_bwd_det_f32: the arguments of sph2pob_roi_extract_bwd_f32 with a scratch pointer (not read) in front of the stream
HOST_ONLY = {
    'sph2pob_roi_extract_bwd_det_f32': SIGNATURES['sph2pob_roi_extract_bwd_f32'][:-1] + [ctypes.c_void_p, ctypes.c_void_p],
}

ABI_VERSION = 6


class Sph2PobLibraryError(RuntimeError):
    pass


def _older_than(path, sources):
    if not os.path.exists(path):
        return True
    t = os.path.getmtime(path)
    deps = [os.path.join(CSRC, s) for s in sources] + [os.path.normpath(os.path.join(CSRC, h)) for h in HEADERS]
    return any(os.path.exists(d) and os.path.getmtime(d) > t for d in deps)


def _stale():
    return _older_than(LIB_PATH, SOURCES) or _older_than(HOST_LIB_PATH, HOST_SOURCES)


def _compile(flags, sources, out, verbose):
    """One hipcc -c per translation unit, in parallel, then one link.  Objects are kept under lib/obj/ and reused while they
    are newer than their source and every header and were built with the same flags (an edit to one .hip recompiles one unit)."""
    import hashlib
    from concurrent.futures import ThreadPoolExecutor
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        raise Sph2PobLibraryError(f'hipcc not found: cannot build {os.path.basename(out)}')
    os.makedirs(LIB_DIR, exist_ok=True)
    obj_dir = os.path.join(LIB_DIR, 'obj')
    os.makedirs(obj_dir, exist_ok=True)
    cflags = [f for f in flags if f != '-shared']
    tag = hashlib.sha1(' '.join(cflags).encode()).hexdigest()[:10]
    deps = [os.path.join(CSRC, h) for h in HEADERS]
    newest_header = max(os.path.getmtime(d) for d in deps if os.path.exists(d))

    def unit(src):
        path = os.path.join(CSRC, src)
        obj = os.path.join(obj_dir, f'{os.path.splitext(src)[0]}.{tag}.o')
        if os.path.exists(obj) and os.path.getmtime(obj) > max(os.path.getmtime(path), newest_header):
            return obj
        tmp = f'{obj}.tmp.{os.getpid()}'
        cmd = [hipcc] + cflags + ['-c', '-o', tmp, path]
        if verbose:
            print(' '.join(cmd))
        try:
            subprocess.check_call(cmd, cwd=CSRC)
            os.replace(tmp, obj)
        finally:
            if os.path.exists(tmp):
                os.remove(tmp)
        return obj

    with ThreadPoolExecutor(max_workers=min(len(sources), max(1, min(os.cpu_count() or 1, 8)))) as pool:
        objs = list(pool.map(unit, sources))
    tmp = f'{out}.tmp.{os.getpid()}'   # linked aside and renamed: other ranks / processes never see a partial file
    link = [hipcc] + [f for f in flags if f.startswith('--offload-arch') or f in ('-shared', '-fPIC', '-pthread', '--cuda-host-only')] + ['-o', tmp] + objs
    if verbose:
        print(' '.join(link))
    try:
        subprocess.check_call(link, cwd=CSRC)
        os.replace(tmp, out)
    finally:
        if os.path.exists(tmp):
            os.remove(tmp)


def build(force=False, verbose=False):
    """hipcc --offload-arch=gfx950 ... -> sph_retina_amd/lib/libsph2pob_hip.so (no GPU needed) and the host twins
    -> sph_retina_amd/lib/libsph2pob_host.so."""
    if force or _older_than(LIB_PATH, SOURCES):
        _compile(HIPCC_FLAGS, SOURCES, LIB_PATH, verbose)
    if force or _older_than(HOST_LIB_PATH, HOST_SOURCES):
        _compile(HOST_FLAGS, HOST_SOURCES, HOST_LIB_PATH, verbose)
    return LIB_PATH


_LIB = None


def lib():
    """The loaded library with typed entry points; raises Sph2PobLibraryError when it cannot be used."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise Sph2PobLibraryError(
            f'{LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"` '
            '(hipcc --offload-arch=gfx950).  There is no CPU / eager fallback for the Sph2Pob path.')
    try:
        handle = ctypes.CDLL(LIB_PATH)
    except OSError as e:
        raise Sph2PobLibraryError(f'cannot load {LIB_PATH}: {e}') from e
    for name, argtypes in SIGNATURES.items():
        try:
            fn = getattr(handle, name)
        except AttributeError as e:
            raise Sph2PobLibraryError(f'{LIB_PATH} does not export {name}') from e
        fn.argtypes = argtypes
        fn.restype = _RESTYPES.get(name, _int)
    if handle.sph2pob_abi_version() != ABI_VERSION:
        raise Sph2PobLibraryError('libsph2pob_hip.so ABI version mismatch: rebuild the library')
    _LIB = handle
    return _LIB


_HOST = None


def host_lib():
    """libsph2pob_host.so with typed `<name>_cpu` entry points (the CPU twins); raises Sph2PobLibraryError when unusable."""
    global _HOST
    if _HOST is not None:
        return _HOST
    if not os.path.exists(HOST_LIB_PATH):
        raise Sph2PobLibraryError(
            f'{HOST_LIB_PATH} is missing: build it with `python -c "import __graft_entry__ as g; g.build()"`.  CPU tensors '
            'are served by this library only (there is no eager / oracle fallback).')
    try:
        handle = ctypes.CDLL(HOST_LIB_PATH)
    except OSError as e:
        raise Sph2PobLibraryError(f'cannot load {HOST_LIB_PATH}: {e}') from e
    for name in HOST_TWINS:
        try:
            fn = getattr(handle, name + '_cpu')
        except AttributeError as e:
            raise Sph2PobLibraryError(f'{HOST_LIB_PATH} does not export {name}_cpu') from e
        fn.argtypes = SIGNATURES[name]
        fn.restype = _int
    for name, argtypes in HOST_ONLY.items():
        try:
            fn = getattr(handle, name + '_cpu')
        except AttributeError as e:
            raise Sph2PobLibraryError(f'{HOST_LIB_PATH} does not export {name}_cpu') from e
        fn.argtypes = argtypes
        fn.restype = _int
    handle.sph2pob_host_threads.restype = _int
    _HOST = handle
    return _HOST


def check(rc, what):
    if rc != 0:
        msg = lib().sph2pob_error_string(int(rc))
        raise Sph2PobLibraryError(f'{what} failed: {msg.decode() if msg else rc} (code {rc})')
