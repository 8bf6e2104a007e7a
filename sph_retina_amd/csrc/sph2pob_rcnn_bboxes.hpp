// Inference of the R-CNN stage for a minibatch (sph2pob_rcnn_bboxes_f32, include/sph2pob_hip.h): what the kernels
// (sph2pob_rcnn_bboxes.hip, cand_build_rois_kernel of sph2pob_get_bboxes.hip) and the CPU twin (sph2pob_host.hip) share — the table
// of the images' own rois, the live row count, the candidate's box and the argument checks — so that a CPU tensor gets the
// arithmetic and the checks a device tensor gets.  The probability is sph2pob_softmax.hpp's Prob, the decode sph2pob_coder.hpp's
// decode_one, the selection and the NMS those of sph2pob_get_bboxes.hpp on ONE flat level of M rows.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_coder.hpp"
#include "sph2pob_get_bboxes.hpp"
#include "sph2pob_softmax.hpp"

namespace sph2pob_rcnn_bb {

namespace GB = sph2pob_gb;
constexpr int kChunkElems = 1 << 14;   // the streaming chunk of sph2pob_get_bboxes.hip

// The priors of this entry: every image's own rois and the per-class deltas of the head
struct Rois {
    const float* rois;         // (B, M, row_stride): the box in columns [0, dim)
    const int64_t* num_rois;   // (B) on the device, or NULL: every image has M
    const float* bbox;         // (B, M, delta_stride) deltas, or NULL: the candidate's box is its roi
    int m;
    int row_stride;
    int delta_stride;          // C dim, or dim for class-agnostic deltas
    int per_class;             // 1: the deltas of class c start at column c dim; 0: at column 0
};

// live rows of image b: the count clamped to [0, M]
SPHG_DEV int live_rows(const int64_t* num_rois, int64_t b, int m) {
    if (!num_rois) return m;
    const int64_t n = num_rois[b];
    return n < 0 ? 0 : n > (int64_t)m ? m : (int)n;
}

// without deltas (with_reg = False): the roi, its components 2 and 3 clamped to [1e-7, 180 - 1e-7] as torch clamps an fp32 tensor
// with these python bounds — both narrowed to fp32 (the upper one IS 180.0f), a NaN passes
SPHG_DEV float clamp_extent(float v) {
    const float lo = 1e-7f, hi = (float)(180.0 - 1e-7);
    return v < lo ? lo : (v > hi ? hi : v);
}

// The box of candidate (r, c) of image b: decode_one on the roi and the class's deltas, or the clamped roi.  `p` is the roi row
// (its first DIM floats, the caller loads them)
template <int DIM>
SPHG_DEV void candidate_box(const Rois& R, const float* p_in, int64_t b, int r, int c, const sph2pob_coder::Norm& nm, float max_ratio,
                            int coder_flags, float ctr_clamp, float* box) {
    float p[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, d[5];
#pragma unroll
    for (int k = 0; k < DIM; k++) p[k] = p_in[k];
    if (R.bbox) {
        const float* q = R.bbox + (b * R.m + r) * (int64_t)R.delta_stride + (R.per_class ? c * DIM : 0);
#pragma unroll
        for (int k = 0; k < DIM; k++) d[k] = q[k];
        sph2pob_coder::decode_one<DIM, false>(p, d, nm, max_ratio, coder_flags, ctr_clamp, box, nullptr);
    } else {
#pragma unroll
        for (int k = 0; k < DIM; k++) box[k] = (k == 2 || k == 3) ? clamp_extent(p[k]) : p[k];
    }
}

// Argument checks of sph2pob_rcnn_bboxes_f32 and its twin up to the pointers, in the documented order (box_dim, the options, the
// sizes); fills the level table: one flat level of M rows, C classes, nms_pre = max_candidates
inline int make_roi_level(int64_t num_images, int64_t m, int64_t row_stride, int64_t num_logits, int box_dim, int reg_class_agnostic,
                          int variant_flags, int class_agnostic, int64_t max_candidates, int64_t max_per_img, float max_ratio, int coder_flags,
                          GB::Levels* out) {
    const int rc = GB::make_level_shapes(&m, nullptr, 1, num_images, num_logits - 1, box_dim, 0, variant_flags, class_agnostic, max_candidates,
                                         max_per_img, max_ratio, coder_flags, kChunkElems, true, out);
    if (rc == SPH2POB_ERR_DIM || rc == SPH2POB_ERR_OPTION) return rc;
    if (reg_class_agnostic < 0 || reg_class_agnostic > 1) return SPH2POB_ERR_OPTION;
    if (num_logits < sph2pob_softmax::kMinK || num_logits > sph2pob_softmax::kMaxK || row_stride < box_dim || row_stride > ((int64_t)1 << 30))
        return SPH2POB_ERR_SIZE;
    return rc;
}
inline Rois make_rois(const float* rois, const int64_t* num_rois, const float* bbox_pred, int64_t m, int64_t row_stride, int64_t num_classes,
                      int box_dim, int reg_class_agnostic) {
    return Rois{rois, num_rois, bbox_pred, (int)m, (int)row_stride, (int)(reg_class_agnostic ? box_dim : num_classes * box_dim),
                reg_class_agnostic ? 0 : 1};
}

}  // namespace sph2pob_rcnn_bb

// Stages 1-10 of sph2pob_rcnn_bboxes_f32 on the probabilities its stage 0 wrote — (B, M, C) fp32, -inf in the rows behind an image's
// count: pipeline() of sph2pob_get_bboxes.hip with cand_build_rois_kernel, which also leaves the number of valid candidates of every
// image in num_valid.  Defined in sph2pob_get_bboxes.hip and called from sph2pob_rcnn_bboxes.hip (inside the library only); the
// arguments are checked by the caller
extern "C" __attribute__((visibility("hidden"))) int sph2pob_rois_bboxes_on_probs(
    const float* probs, const sph2pob_rcnn_bb::Rois* rois, int64_t num_images, int64_t num_classes, int box_dim, float score_thr,
    int64_t max_candidates, const float* means_host, const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp, int variant_flags,
    int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets,
    int64_t* num_valid, void* workspace, void* stream);
