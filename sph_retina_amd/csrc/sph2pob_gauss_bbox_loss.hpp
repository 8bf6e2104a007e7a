// Fused Gaussian (GD / KF) box-regression loss: the option checks shared by the kernels' entries (sph2pob_gauss_bbox_loss.hip) and
// their CPU twin (sph2pob_host.hip).  Level table, span geometry and limits are those of sph2pob_bbox_loss.hpp; the arithmetic per
// positive anchor is the composition's: decode_one<DIM, true> (sph2pob_coder.hpp) then GaussBody::eval (sph2pob_loss.hpp).
#pragma once
#include "sph2pob_bbox_loss.hpp"

namespace sph2pob_gauss_bbox {

// the Gaussian option checks of the sph2pob_gauss_loss_* launchers, then the box-dim, weight-dim and coder checks of the IoU entry
inline int check_options(int box_dim, const float* weight, int weight_dim, float max_ratio, int coder_flags, int type_flags, int fun,
                         int opts) {
    if (int rc = sph2pob::gauss_check(weight, weight_dim, 0, box_dim, type_flags, fun, opts)) return rc;
    return sph2pob_bbox::check_options(box_dim, weight, weight_dim, max_ratio, coder_flags, SPH2POB_LOSS_IOU);
}

inline sph2pob::GaussBody make_body(int type_flags, int fun, float tau, float alpha, int opts, float beta, float eps) {
    return sph2pob::GaussBody{type_flags & 0xff, fun, tau, alpha, opts, beta, eps};
}

}  // namespace sph2pob_gauss_bbox
