// Sigmoid focal loss (mmdet/models/losses/focal_loss.py:12-57, the op the reference takes from mmcv.ops.sigmoid_focal_loss): the
// per-element arithmetic and the argument checks (the level table: sph2pob_class_levels.hpp), shared by the kernels
// (sph2pob_focal.hip) and their CPU twins (sph2pob_host.hip) so that a CPU tensor gets the arithmetic and the checks a device
// tensor gets.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_class_levels.hpp"
#include "sph2pob_head_loss.hpp"

namespace sph2pob_focal {

using sph2pob_head::aligned_to;
using sph2pob_head::effective_scale;
using sph2pob_head::kBlock;
using sph2pob_head::kMaxLevels;

// gamma split once on the host: q^gamma = q^gint * exp2(gfrac * log2 q), gint = min(floor(gamma), 8) exact multiplications (an
// integer gamma never meets log2 / exp2, whose absolute error in the exponent grows with gamma * |log2 q|).  mode: 2 and 0 are
// the special cases q * q and 1 (q^0 is 1 even where q underflows), -1 the general route.
struct Params {
    float gamma, alpha, gfrac;
    int gint, mode;
};
inline Params make_params(float gamma, float alpha) {
    Params p;
    p.gamma = gamma; p.alpha = alpha;
    const float fl = floorf(gamma);
    p.gint = (int)(fl < 8.0f ? fl : 8.0f);
    p.gfrac = gamma - (float)p.gint;
    p.mode = gamma == 2.0f ? 2 : (gamma == 0.0f ? 0 : -1);
    return p;
}

// loss = a q^gamma softplus(z) and d loss / d x of ONE (logit, target bit) in the logit-stable form: z = t ? -x : x,
// e = exp(-|z|), q = sigmoid(z) and qm = sigmoid(-z) both from e (never 1 - q of a rounded q), s = softplus(z) = max(z, 0) +
// log1p(e), a = t ? alpha : 1 - alpha.  d loss / d z = a q^gamma (q + gamma qm s): both terms have one sign, nothing cancels.
// The three transcendental-bearing values (e, 1 / (1 + e), log1p(e)) are fp32; they are COMBINED in double and rounded to fp32
// once per output: where the loss is largest (a confidently wrong logit: q -> 1, s -> z) the fp32 products a * q^gamma * s would
// each add half an ulp of a value near 16 a, which is as much as the torch composition's error there; the double combination
// leaves one rounding.  (A dozen double operations per element at half the fp32 rate.)
SPHF_DEV void element(float x, bool t, const Params& P, float& loss, float& dx) {
    const float z = t ? -x : x;
    const float e = expf(-fabsf(z));
    const float r = 1.0f / (1.0f + e);
    const float er = e * r;                      // the smaller of the two sigmoids, to fp32 relative accuracy
    const bool pos = z >= 0.0f;
    const double small = (double)er, large = pos ? 1.0 - small : (double)r;
    const double q = pos ? large : small, qm = pos ? small : large;
    const double s = (double)fmaxf(z, 0.0f) + (double)log1pf(e);
    double qg;
    if (P.mode == 2) qg = q * q;
    else if (P.mode == 0) qg = 1.0;
    else {
        qg = 1.0;
        for (int k = 0; k < P.gint; k++) qg *= q;
        if (P.gfrac > 0.0f) qg *= (double)exp2f(P.gfrac * log2f((float)q));
    }
    const double aq = (double)(t ? P.alpha : 1.0f - P.alpha) * qg;
    loss = (float)(aq * s);
    const float dz = (float)(aq * (q + ((double)P.gamma * qm) * s));
    dx = t ? -dz : dz;
}

// The level table: Level, Levels and the KIND_* of sph2pob_class_levels.hpp; a FLAT4 item is four consecutive elements, a FLAT1
// item one element.  Argument checks of sph2pob_focal_loss_sum_f32 / its twin, in the documented order: the options here, sizes
// and pointers in the shared walk, which fills the table (`tables`, `vec_bytes`: there)
using namespace sph2pob_class;
constexpr Family kFamily{1, (int64_t)1 << 24, false, INT64_MAX};
inline int make_levels(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                       int64_t B, int64_t C, int weight_mode, float gamma, bool tables, Levels* out, int vec_bytes = 16) {
    if (!(gamma >= 0.0f) || weight_mode < 0 || weight_mode > 2) return SPH2POB_ERR_OPTION;
    return walk_levels(kFamily, logits, grads, level_n, level_hw, num_levels, B, C, tables, vec_bytes, out);
}

// flat (N, C) entries: weight_mode, gamma, grad_stride -> OPTION; n < 0, C <= 0, N C too large -> SIZE
inline int flat_check(int64_t n, int64_t C, int weight_mode, float gamma, int grad_stride) {
    if (!(gamma >= 0.0f) || weight_mode < 0 || weight_mode > 2 || (grad_stride != 0 && grad_stride != 1)) return SPH2POB_ERR_OPTION;
    if (n < 0 || C <= 0 || C > ((int64_t)1 << 24) || n > ((int64_t)1 << 38) / C) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}

// workgroups of the partial-sum pass of a call with these shapes (scalar kinds: an upper bound) + 1
inline int64_t workspace_doubles(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t B, int64_t C) {
    Levels L;
    if (make_levels(nullptr, nullptr, level_n, level_hw, num_levels, B, C, 0, 0.0f, false, &L) != SPH2POB_OK) return 0;
    return (int64_t)L.blocks + 1;
}

// the element weight: 1, weight[row] or weight[row * C + c] (row = b n + anchor: the logical (B, n, C) order)
SPHF_DEV float weight_of(const float* w, int mode, int64_t row, int64_t C, int c) {
    return mode == 0 ? 1.0f : (mode == 1 ? w[row] : w[row * C + c]);
}

}  // namespace sph2pob_focal
