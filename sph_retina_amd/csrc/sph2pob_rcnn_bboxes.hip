// libsph2pob_hip.so — inference of the R-CNN stage for a minibatch (sph2pob_rcnn_bboxes_f32, include/sph2pob_hip.h): what
// SphStandardRoIHead.simple_test_bboxes -> SphShared2FCBBoxHead.get_bboxes -> multiclass_nms compute per image
// (sphdet/models/heads/sph_rcnn_head.py:127-177, :248-333; sphdet/bbox/nms/utils.py:6-95) — softmax over K = C + 1 logits, the
// decode of the per-class boxes of every roi, `scores > score_thr`, the NMS and [:max_per_img] — for B images with eleven launches
// whatever B is and without a host read.  gfx950 only.
//
// Here: the argument checks, the workspace and stage 0, the probabilities of the rows in front of every image's count (Prob of
// sph2pob_softmax.hpp, the bits of sph2pob_softmax_scores_f32 on the flat layout) as a (B, M, C) block of the workspace, -inf behind
// the count.  Stages 1-10 are pipeline() of sph2pob_get_bboxes.hip on that block as one flat level of M rows, with RoiSource
// (sph2pob_rcnn_bboxes.hpp) as the candidate source of cand_build_kernel: only the SELECTED candidates are decoded — at most
// max_candidates of the M C per image, where the reference decodes all of them.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_rcnn_bboxes.hpp"

namespace {

using namespace sph2pob_rcnn_bb;
using sph2pob_softmax::kBlock;
using sph2pob_softmax::kHoldK;
using sph2pob_softmax::Prob;

// Stage 0.  One workgroup per kBlock consecutive rows of ONE image, so that the image's count cuts the workgroup's rows at a
// workgroup-uniform place: the `live` rows in front of it are a contiguous span of logits — STAGED (K <= kHoldK): loaded coalesced
// into LDS, one row per lane there (the probabilities overwrite the row's own logits), stored coalesced; otherwise every lane walks
// its own row in memory, three times.  The rows behind the count get -inf — `p > score_thr` is false whatever the threshold — and
// nothing of them is loaded.  The arithmetic is Prob's on either path: the same bits.
template <bool STAGED>
__global__ __launch_bounds__(kBlock) void rcnn_prob_kernel(const float* __restrict__ logits, const int64_t* __restrict__ num_rois, int M, int K,
                                                         float* __restrict__ probs) {
    extern __shared__ float stage[];
    const int b = blockIdx.y, C = K - 1, t = threadIdx.x;
    const int row0 = (int)blockIdx.x * kBlock;
    const int rows = M - row0 < kBlock ? M - row0 : kBlock;
    const int ahead = live_rows(num_rois, b, M) - row0;
    const int live = ahead < 0 ? 0 : (ahead < rows ? ahead : rows);
    const float* x = logits + ((int64_t)b * M + row0) * K;
    float* o = probs + ((int64_t)b * M + row0) * C;
    if constexpr (STAGED) {
        for (int i = t; i < live * K; i += kBlock) stage[i] = x[i];
        __syncthreads();
        if (t < live) {
            float* h = stage + t * K;
            Prob r;
            r.begin();
            for (int j = 0; j < K; j++) r.see_max(h[j]);
            for (int j = 0; j < K; j++) { h[j] = r.e(h[j]); r.add(h[j]); }
            for (int j = 0; j < C; j++) h[j] = r.of(h[j]);
        }
        __syncthreads();
        for (int i = t; i < rows * C; i += kBlock) {
            const int row = i / C;
            o[i] = row < live ? stage[row * K + (i - row * C)] : -INFINITY;
        }
    } else {
        if (t >= rows) return;
        float* q = o + (int64_t)t * C;
        if (t < live) {
            const float* h = x + (int64_t)t * K;
            Prob r;
            r.begin();
            for (int j = 0; j < K; j++) r.see_max(h[j]);
            for (int j = 0; j < K; j++) r.see_sum(h[j]);
            for (int j = 0; j < C; j++) q[j] = r.p(h[j]);
        } else {
            for (int j = 0; j < C; j++) q[j] = -INFINITY;
        }
    }
}

int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

// the pipeline's own workspace for one level of M rows with nms_pre = max_candidates; 0: the shapes are not accepted
int64_t base_bytes(int64_t num_images, int64_t m, int64_t num_classes, int box_dim, int64_t max_candidates) {
    return sph2pob_get_bboxes_workspace_bytes(&m, 1, num_images, num_classes, box_dim, max_candidates);
}

}  // namespace

extern "C" {

int64_t sph2pob_rcnn_bboxes_workspace_bytes(int64_t num_images, int64_t m, int64_t num_logits, int box_dim, int64_t max_candidates) {
    if (num_logits < sph2pob_softmax::kMinK || num_logits > sph2pob_softmax::kMaxK) return 0;
    const int64_t base = base_bytes(num_images, m, num_logits - 1, box_dim, max_candidates);
    if (base <= 0) return 0;
    return up256(base) + 256 + up256(num_images * m * (num_logits - 1) * 4);
}

int sph2pob_rcnn_bboxes_f32(const float* rois, const int64_t* num_rois, const float* cls_score, const float* bbox_pred, int64_t num_images,
                            int64_t m, int64_t row_stride, int64_t num_logits, int box_dim, int reg_class_agnostic, float score_thr,
                            int64_t max_candidates, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                            float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                            int64_t* labels, int64_t* prior_inds, int64_t* num_dets, int64_t* num_valid, void* workspace, void* stream) {
    const GB::Shape sh{&m, nullptr, 1, num_images, num_logits - 1, box_dim};
    const GB::Selection sel{0, score_thr, max_candidates};
    const GB::Coder cd = GB::make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp);
    const GB::Nms nms{variant_flags, class_agnostic, iou_threshold, max_per_img};
    const GB::Outputs out{dets, labels, prior_inds, num_dets};
    GB::Levels L;
    if (int rc = make_roi_level(sh, row_stride, reg_class_agnostic, sel, cd, nms, &L)) return rc;
    if (!rois || !cls_score || !num_valid || !workspace || out.check(max_per_img)) return SPH2POB_ERR_NULL;
    const int64_t C = num_logits - 1;
    const int64_t base = base_bytes(num_images, m, C, box_dim, max_candidates);
    // the probabilities follow the pipeline's workspace, 256-byte aligned: an image's block is as aligned as it would be in a tensor
    // of its own, so the streaming stages keep their 16-byte loads where M C allows them
    float* probs = reinterpret_cast<float*>((reinterpret_cast<uintptr_t>(workspace) + (uintptr_t)base + 255) & ~(uintptr_t)255);
    hipStream_t s = (hipStream_t)stream;
    const int K = (int)num_logits;
    const dim3 grid((unsigned)((m + kBlock - 1) / kBlock), (unsigned)num_images), block(kBlock);
    if (K <= kHoldK)
        hipLaunchKernelGGL((rcnn_prob_kernel<true>), grid, block, (size_t)kBlock * K * sizeof(float), s, cls_score, num_rois, (int)m, K, probs);
    else
        hipLaunchKernelGGL((rcnn_prob_kernel<false>), grid, block, 0, s, cls_score, num_rois, (int)m, K, probs);
    if (const hipError_t e = hipGetLastError(); e != hipSuccess) return (int)e;
    L.lv[0].cls = probs;
    return rois_bboxes_on_probs(L, make_rois(rois, num_rois, bbox_pred, m, row_stride, C, box_dim, reg_class_agnostic), sh, sel, cd, nms, out,
                                num_valid, workspace, stream);
}

}  // extern "C"
