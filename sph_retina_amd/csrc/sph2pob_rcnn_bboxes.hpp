// Inference of the R-CNN stage for a minibatch (sph2pob_rcnn_bboxes_f32, include/sph2pob_hip.h): what the kernels
// (sph2pob_rcnn_bboxes.hip, cand_build_kernel<RoiSource> of sph2pob_get_bboxes.hip) and the CPU twin (sph2pob_host.hip) share — the
// table of the images' own rois, the live row count, the candidate source and the argument checks — so that a CPU tensor gets the
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
SPHG_DEV void candidate_box(const Rois& R, const float* p_in, int64_t b, int r, int c, const GB::Coder& cd, float* box) {
    float p[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, d[5];
#pragma unroll
    for (int k = 0; k < DIM; k++) p[k] = p_in[k];
    if (R.bbox) {
        const float* q = R.bbox + (b * R.m + r) * (int64_t)R.delta_stride + (R.per_class ? c * DIM : 0);
#pragma unroll
        for (int k = 0; k < DIM; k++) d[k] = q[k];
        sph2pob_coder::decode_one<DIM, false>(p, d, cd.nm, cd.max_ratio, cd.coder_flags, cd.ctr_clamp, box, nullptr);
    } else {
#pragma unroll
        for (int k = 0; k < DIM; k++) box[k] = (k == 2 || k == 3) ? clamp_extent(p[k]) : p[k];
    }
}

// The candidate source of this entry (see sph2pob_get_bboxes.hpp): one flat level whose priors are the images' own rois.  Key index
// r C + c -> roi row r, class c; the roi is one 16-byte load where the row's address allows it (row_stride is arbitrary, so that
// is decided per row; the bits are the same either way), the deltas of class c are gathered from the row's own C DIM.  On the device
// the first workgroup of an image also adds up the image's selection histogram — every valid candidate was counted there exactly
// once, whatever the cut — into num_valid (the twin counts them itself and leaves num_valid NULL here)
template <int DIM>
struct RoiSource {
    static constexpr int kDim = DIM;
    Rois R;
    GB::Coder cd;
    int64_t* num_valid;
    SPHG_DEV float operator()(const GB::Level& lv, int, int64_t b, int r, int c, float score, float (&box)[5], int* prior) const {
        *prior = r;
        const float* row = R.rois + ((int64_t)b * R.m + r) * R.row_stride;
        float p[5];
        if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
            const float4 v = *reinterpret_cast<const float4*>(row);
            p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; k++) p[k] = row[k];
        }
        if constexpr (DIM == 5) p[4] = row[4];
        candidate_box<DIM>(R, p, b, r, c, cd, box);
        return score;
    }
    // flat < lv.count.  A guard only: every selected key carries an index of the level
    SPHG_DEV bool has(const GB::Level& lv, int r) const { return r < lv.n; }
    // hist: the selection histograms of the call, kBins per image (one level); all threads of the workgroup come here together
    __device__ __forceinline__ void prologue(const int* __restrict__ hist, int b) const {
        __shared__ int valid_sum;
        const int* g = hist + (int64_t)b * GB::kBins;
        int s = 0;
        for (int i = threadIdx.x; i < GB::kBins; i += GB::kBuildBlock) s += g[i];
        if (threadIdx.x == 0) valid_sum = 0;
        __syncthreads();
        if (s) atomicAdd(&valid_sum, s);
        __syncthreads();
        if (threadIdx.x == 0) num_valid[b] = valid_sum;
    }
};

// Argument checks of sph2pob_rcnn_bboxes_f32 and its twin up to the pointers, in the documented order (box_dim, the options, the
// sizes); fills the level table: one flat level of M rows (sh.level_n[0]), C classes, nms_pre = max_candidates
inline int make_roi_level(const GB::Shape& sh, int64_t row_stride, int reg_class_agnostic, const GB::Selection& sel, const GB::Coder& cd,
                          const GB::Nms& nms, GB::Levels* out) {
    const int rc = GB::make_level_shapes(sh, sel, cd, nms, true, out);
    if (rc == SPH2POB_ERR_DIM || rc == SPH2POB_ERR_OPTION) return rc;
    if (reg_class_agnostic < 0 || reg_class_agnostic > 1) return SPH2POB_ERR_OPTION;
    const int64_t num_logits = sh.num_classes + 1;
    if (num_logits < sph2pob_softmax::kMinK || num_logits > sph2pob_softmax::kMaxK || row_stride < sh.box_dim || row_stride > ((int64_t)1 << 30))
        return SPH2POB_ERR_SIZE;
    return rc;
}
inline Rois make_rois(const float* rois, const int64_t* num_rois, const float* bbox_pred, int64_t m, int64_t row_stride, int64_t num_classes,
                      int box_dim, int reg_class_agnostic) {
    return Rois{rois, num_rois, bbox_pred, (int)m, (int)row_stride, (int)(reg_class_agnostic ? box_dim : num_classes * box_dim),
                reg_class_agnostic ? 0 : 1};
}

// Stages 1-10 of sph2pob_rcnn_bboxes_f32 on a checked level table whose scores are the probabilities its stage 0 wrote — (B, M, C)
// fp32, -inf in the rows behind an image's count: pipeline() of sph2pob_get_bboxes.hip with RoiSource, which also leaves the number
// of valid candidates of every image in num_valid.  Defined in sph2pob_get_bboxes.hip and called from sph2pob_rcnn_bboxes.hip (inside
// the library only)
__attribute__((visibility("hidden"))) int rois_bboxes_on_probs(const GB::Levels& L, const Rois& R, const GB::Shape& sh, const GB::Selection& sel,
                                                               const GB::Coder& cd, const GB::Nms& nms, const GB::Outputs& out,
                                                               int64_t* num_valid, void* workspace, void* stream);

}  // namespace sph2pob_rcnn_bb
