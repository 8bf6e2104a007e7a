// Fused box-regression loss of a point (FCOS) head — the regression half of SphFCOSHead.loss
// (sphdet/models/heads/sph_fcos_head.py:76-100): the argument checks and the arithmetic of one live row, shared by the kernel
// (sph2pob_point_bbox_loss.hip) and its CPU twin (sph2pob_host.hip).  The level table and the span geometry are those of the
// anchor heads' loss (sph2pob_bbox_loss.hpp); a row is decode_row<DIM, false> (sph2pob_point_targets.hpp) of the prediction and of
// the target with the same point, pair_loss<DIM, GRAD, FAST> (sph2pob_loss.hpp), then decode_row<DIM, true>: the composition's
// functions in the composition's order.
#pragma once
#include "sph2pob_bbox_loss.hpp"
#include "sph2pob_point_targets.hpp"

namespace sph2pob_point_bbox {

// The checks every entry starts with, in the documented order: check_options of the sibling without its coder options, the level
// table, the image range, then the caller's NULL checks, then the NaN rule of the clip bounds (check_image_late)
inline int check_and_levels(const void* const* preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                            int64_t B, int box_dim, const float* weight, int weight_dim, int64_t img_h, int64_t img_w, int loss_mode,
                            sph2pob_bbox::Levels* L) {
    if (int rc = sph2pob_bbox::check_options(box_dim, weight, weight_dim, 0.0f, 0, loss_mode)) return rc;
    if (int rc = sph2pob_bbox::make_levels(preds, grads, level_n, level_hw, num_levels, B, box_dim, true, L)) return rc;
    if (img_h < 1 || img_w < 1 || img_h > (1 << 24) || img_w > (1 << 24)) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}
inline int check_bounds(float max_h, float max_w) { return (max_h != max_h || max_w != max_w) ? SPH2POB_ERR_OPTION : SPH2POB_OK; }

// One live row: the loss of decode(pt, d) against decode(pt, t) and, under GRAD, g = J_decode^T ((gw gx)) with gw = scale_eff w —
// the product order of the composition's autograd chain, the clip's gate included.  Nothing flows to pt or t.
template <int DIM, bool GRAD, bool FAST>
SPHF_DEV float row_loss(const float (&pt)[2], const float (&d)[5], const float (&t)[5], const sph2pob_point::Image& im, int loss_mode,
                        float eps, float gw, float (&g)[5]) {
    float box[5], tbox[5], gx[5], gy[5];
    sph2pob_point::decode_row<DIM, false>(pt, d, nullptr, im, box);
    sph2pob_point::decode_row<DIM, false>(pt, t, nullptr, im, tbox);
    const float lo = sph2pob::pair_loss<DIM, GRAD, FAST>(box, tbox, loss_mode, eps, nullptr, gx, gy);
    if (GRAD) {
        float gb[5];
#pragma unroll
        for (int k = 0; k < 5; k++) gb[k] = k < DIM ? gw * gx[k] : 0.0f;
        sph2pob_point::decode_row<DIM, true>(pt, d, gb, im, g);
    }
    return lo;
}

}  // namespace sph2pob_point_bbox
