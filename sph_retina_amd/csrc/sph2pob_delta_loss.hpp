// Fused L1 / SmoothL1 box loss on the head's ENCODED deltas — the regression half of SphRetinaHead.loss_single with the default
// reg_decoded_bbox=False and loss_bbox=dict(type='L1Loss') (mmdet/models/losses/smooth_l1_loss.py:10-52): the per-element
// arithmetic, the row rule and the option checks, shared by the kernels (sph2pob_delta_loss.hip) and their CPU twin
// (sph2pob_host.hip).  The level table, the span geometry and the shape checks are sph2pob_bbox_loss.hpp's, unchanged.
#pragma once
#include <math.h>

#include "sph2pob_bbox_loss.hpp"

namespace sph2pob_delta {

using sph2pob_bbox::delta_offset;
using sph2pob_bbox::effective_scale;
using sph2pob_bbox::Level;
using sph2pob_bbox::Levels;
using sph2pob_bbox::make_levels;
using sph2pob_bbox::workspace_doubles;

// the option checks the entry starts with: box_dim -> DIM; weight_dim (with a weight), beta < 0 or NaN -> OPTION
inline int check_options(int box_dim, const float* weight, int weight_dim, float beta) {
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (weight && weight_dim != 1 && weight_dim != box_dim) return SPH2POB_ERR_OPTION;
    if (!(beta >= 0.0f)) return SPH2POB_ERR_OPTION;
    return SPH2POB_OK;
}

// One element in fp32, in the reference's operation order: x = pred - target, d = |x|;
//   beta == 0 (l1_loss)         loss = d,                                            s = sign(x) (0 at equality, as torch.abs)
//   beta  > 0 (smooth_l1_loss)  loss = d < beta ? ((0.5 d) d) / beta : d - 0.5 beta, s = d < beta ? x / beta : sign(x)
// s is d loss / d pred.  A NaN x gives a NaN loss and a NaN s (every comparison fails: the outer branch, then sign keeps x).
SPHF_DEV void element(float pred, float target, float beta, float& loss, float& s) {
    const float x = pred - target, d = fabsf(x);
    const float sg = x > 0.0f ? 1.0f : (x < 0.0f ? -1.0f : (x == 0.0f ? 0.0f : x));
    if (beta > 0.0f && d < beta) {
        loss = ((0.5f * d) * d) / beta;
        s = x / beta;
    } else {
        loss = beta > 0.0f ? d - 0.5f * beta : d;
        s = sg;
    }
}

// The weights of one row, one per component, and whether the row takes part: ANY component != 0 (not the mean: (+1, -1, 0, 0)
// is a live row; a NaN weight is live too).  wd: 0 without a weight tensor, 1 for (B, n), DIM for (B, n, dim);
// `vec` (DIM == 4 only): the row is one 16-byte load.
template <int DIM>
SPHF_DEV bool row_weights(const float* __restrict__ w, int wd, bool vec, int64_t row, float (&out)[DIM]) {
    if (!w) {
#pragma unroll
        for (int k = 0; k < DIM; k++) out[k] = 1.0f;
        return true;
    }
    if (wd == 1) {
        const float v = w[row];
#pragma unroll
        for (int k = 0; k < DIM; k++) out[k] = v;
        return v != 0.0f;
    }
    if (DIM == 4 && vec) {
        const float4 v = *reinterpret_cast<const float4*>(w + row * 4);
        out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < DIM; k++) out[k] = w[row * DIM + k];
    }
    bool live = false;
#pragma unroll
    for (int k = 0; k < DIM; k++) live = live || out[k] != 0.0f;
    return live;
}

}  // namespace sph2pob_delta
