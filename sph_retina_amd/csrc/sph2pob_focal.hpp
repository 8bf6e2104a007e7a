// Sigmoid focal loss (mmdet/models/losses/focal_loss.py:12-57, the op the reference takes from mmcv.ops.sigmoid_focal_loss): the
// per-element arithmetic, the level table and the argument checks, shared by the kernels (sph2pob_focal.hip) and their CPU twins
// (sph2pob_host.hip) so that a CPU tensor gets the arithmetic and the checks a device tensor gets.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_head_loss.hpp"

namespace sph2pob_focal {

using sph2pob_head::aligned_to;
using sph2pob_head::effective_scale;
using sph2pob_head::kBlock;
using sph2pob_head::kMaxLevels;

constexpr int64_t kMaxLevelElems = ((int64_t)1 << 31) - 4096;   // elements of one level: 32-bit item indices inside a level

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

// One level of one call.  kind: how a thread's item maps onto memory
//   0  NCHW (B, A C, H, W), four consecutive positions p = h W + w of one (b, a) per item: 16-byte accesses at stride H W over the classes
//   1  NCHW, one position per item (H W % 4 != 0 or a base that is not 16-byte aligned)
//   2  flat (B, n_l, C), four consecutive elements per item
//   3  flat, one element per item
enum { KIND_NCHW4 = 0, KIND_NCHW1 = 1, KIND_FLAT4 = 2, KIND_FLAT1 = 3 };
struct Level {
    const float* logits;
    float* grad;           // laid out like logits; NULL in a forward-only call
    int n, hw, a, kind;    // anchors of the level; H W (0: flat); anchors per position
    int items;             // work items of the level
    int block_off;         // first workgroup of the level
    int64_t row_off;       // index of the level's first anchor inside an image's n rows
};
struct Levels {
    Level lv[kMaxLevels];
    int num, blocks;       // levels; workgroups of the whole call
    int64_t n_total;       // anchors of one image, all levels
    int64_t elems;         // B n C
};

// Argument checks of sph2pob_focal_loss_sum_f32 / its twin, in the documented order; fills the table.  `tables` false: shapes
// only (the workspace size), every level counted with its scalar kind (an upper bound on the workgroups).  `vec_bytes`: the
// alignment the vector kinds need — four elements: 16 for fp32 levels, 8 for the 16-bit levels of sph2pob_focal_loss_sum_h16,
// whose pointers the table keeps as float* all the same (sph2pob_head_loss.hpp, level_ptr).
inline int make_levels(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                       int64_t B, int64_t C, int weight_mode, float gamma, bool tables, Levels* out, int vec_bytes = 16) {
    if (!(gamma >= 0.0f) || weight_mode < 0 || weight_mode > 2) return SPH2POB_ERR_OPTION;
    if (num_levels < 1 || num_levels > kMaxLevels || B < 0 || B > 65535 || C <= 0 || C > ((int64_t)1 << 24)) return SPH2POB_ERR_SIZE;
    if (!level_n || (tables && !logits)) return SPH2POB_ERR_NULL;
    Levels L{};
    L.num = num_levels;
    int64_t blocks = 0, rows = 0;
    for (int l = 0; l < num_levels; l++) {
        const int64_t n = level_n[l], hw = level_hw ? level_hw[l] : 0;
        if (n < 0 || hw < 0 || (hw > 0 && n % hw != 0) || n > kMaxLevelElems / C || (B > 0 && n * C > kMaxLevelElems / B)) return SPH2POB_ERR_SIZE;
        const int64_t elems = B * n * C;
        Level& d = L.lv[l];
        d.n = (int)n; d.hw = (int)hw; d.a = hw > 0 ? (int)(n / hw) : 1;
        d.logits = tables ? (const float*)logits[l] : nullptr;
        d.grad = tables && grads ? (float*)grads[l] : nullptr;
        if (tables && elems > 0 && (!d.logits || (grads && !d.grad))) return SPH2POB_ERR_NULL;
        const bool al = tables && aligned_to(d.logits, vec_bytes) && aligned_to(d.grad, vec_bytes);
        int64_t items;
        if (hw > 0) {
            d.kind = al && hw % 4 == 0 ? KIND_NCHW4 : KIND_NCHW1;
            items = d.kind == KIND_NCHW4 ? B * n / 4 : B * n;
        } else {
            d.kind = al && elems % 4 == 0 ? KIND_FLAT4 : KIND_FLAT1;
            items = d.kind == KIND_FLAT4 ? elems / 4 : elems;
        }
        d.items = (int)items;
        d.block_off = (int)blocks;
        d.row_off = rows;
        blocks += (items + kBlock - 1) / kBlock;
        rows += n;
        L.elems += elems;
        if (blocks >= ((int64_t)1 << 31) - 1) return SPH2POB_ERR_SIZE;
    }
    L.blocks = (int)blocks; L.n_total = rows;
    *out = L;
    return SPH2POB_OK;
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
