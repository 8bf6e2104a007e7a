// Sigmoid binary cross-entropy on a head's logits — mmdet's binary_cross_entropy (mmdet/models/losses/cross_entropy_loss.py:64-143)
// without class_weight: FCOS' loss_centerness (soft targets) and the RPN's stock loss_cls (hard labels, one channel).  The
// per-element arithmetic, the target / weight rule of an element and the argument checks (the level table:
// sph2pob_class_levels.hpp), shared by the kernel (sph2pob_bce_loss.hip) and its CPU twin (sph2pob_host.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_class_levels.hpp"
#include "sph2pob_head_loss.hpp"

namespace sph2pob_bce {

using namespace sph2pob_class;
using sph2pob_head::effective_scale;

// loss = max(x, 0) - x t + log1p(exp(-|x|)) and d loss / d x = sigmoid(x) - t of ONE (logit, target).  e and log1p(e) are fp32;
// the three terms are combined in double and rounded once, as the focal element combines its own (sph2pob_focal.hpp).  The sigmoid
// is r = 1 / (1 + e) on the side where it is the larger one and e r on the other: never 1 - (a rounded value).
SPHF_DEV void element(float x, float t, float& loss, float& dx) {
    const float e = expf(-fabsf(x));
    const float r = 1.0f / (1.0f + e);
    const float sig = x >= 0.0f ? r : e * r;
    loss = (float)((double)fmaxf(x, 0.0f) - (double)x * (double)t + (double)log1pf(e));
    dx = sig - t;
}

// Where the targets of a call come from: hard labels (B, n) — channel c of a row is label == c, a label >= C an all-zero row, a
// label < 0 or == ignore_index a row of weight 0 (_expand_onehot_labels) — or soft targets (B, n, C), whose weight is multiplied by
// (t >= 0) & (t != ignore_index).  weight: NULL / (B, n) / (B, n, C) by wmode.
struct Targets {
    const float* soft;
    const int64_t* hard;
    const float* weight;
    int wmode;
    int64_t ignore;
};

SPHF_DEV float weight_of(const float* w, int mode, int64_t row, int64_t C, int c) {
    return mode == 0 ? 1.0f : (mode == 1 ? w[row] : w[row * C + c]);
}
SPHF_DEV bool label_valid(int64_t lab, int64_t ignore) { return lab >= 0 && lab != ignore; }
// (label >= 0) & (label != ignore_index) on a float target, as torch compares a float tensor with a Python int: in double (every
// fp32 value is exact there; an ignore_index beyond 2^53 is its nearest double: it equals no fp32 value it should not)
SPHF_DEV bool soft_valid(float t, int64_t ignore) { return t >= 0.0f && (double)t != (double)ignore; }

// target and weight of element (row, c); HARD selects the label form
template <bool HARD>
SPHF_DEV void target_weight(const Targets& T, int64_t row, int64_t C, int c, float& t, float& w) {
    w = weight_of(T.weight, T.wmode, row, C, c);
    if (HARD) {
        const int64_t lab = T.hard[row];
        t = lab == (int64_t)c ? 1.0f : 0.0f;
        if (!label_valid(lab, T.ignore)) w = 0.0f;
    } else {
        t = T.soft[row * C + c];
        if (!soft_valid(t, T.ignore)) w = 0.0f;
    }
}

// Argument checks of sph2pob_bce_loss_sum_f32 / its twin in the documented order: weight_mode here, sizes and pointers in the
// shared walk, which fills the table; then the caller's pointer checks (check_tensors)
constexpr Family kFamily{1, (int64_t)1 << 24, false, INT64_MAX};
inline int make_levels(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                       int64_t B, int64_t C, int weight_mode, bool tables, Levels* out) {
    if (weight_mode < 0 || weight_mode > 2) return SPH2POB_ERR_OPTION;
    return walk_levels(kFamily, logits, grads, level_n, level_hw, num_levels, B, C, tables, 16, out);
}
// exactly one of targets / labels: both -> NULL whatever the sizes; neither, out, workspace, or a weight the mode asks for -> NULL
// (the target and the weight only when there are elements: nothing is read from them otherwise)
inline int check_tensors(const Levels& L, const float* targets, const int64_t* labels, const float* weight, int weight_mode, const float* out,
                         const void* workspace) {
    if (targets && labels) return SPH2POB_ERR_NULL;
    if (!out || !workspace || (L.elems > 0 && ((!targets && !labels) || (weight_mode != 0 && !weight)))) return SPH2POB_ERR_NULL;
    return SPH2POB_OK;
}

// workgroups of the partial-sum pass of a call with these shapes (scalar kinds: an upper bound) + 1
inline int64_t workspace_doubles(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t B, int64_t C) {
    Levels L;
    if (make_levels(nullptr, nullptr, level_n, level_hw, num_levels, B, C, 0, false, &L) != SPH2POB_OK) return 0;
    return (int64_t)L.blocks + 1;
}

}  // namespace sph2pob_bce
