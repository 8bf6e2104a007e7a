// Point (anchor-free) targets and the distance-point coder: what mmdet's FCOSHead.get_targets / centerness_target
// (mmdet/models/dense_heads/fcos_head.py:270-329, :415-434) compute through the reference's SphFCOSHead._get_target_single
// (sphdet/models/heads/sph_fcos_head.py:107-203), and bbox2distance / distance2bbox of
// sphdet/bbox/coder/distance_point_sph_bbox_coder.py:71-163.  The arithmetic of one GT row, one (point, GT) pair, one target row
// and one coder row, the argument checks and the workspace, shared by the kernels (sph2pob_point_targets.hip) and their CPU twins
// (sph2pob_host.hip): every float is computed by the same fp32 operations in the same order as the reference's torch composition on
// the CPU (the library is built with -ffp-contract=off), so a CPU tensor, a device tensor and that composition agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_head_loss.hpp"

namespace sph2pob_point {

using sph2pob_head::aligned_to;
using sph2pob_head::kBlock;
using sph2pob_head::kMaxLevels;

constexpr int kTile = kBlock;            // GT rows of one LDS tile: one row converted per thread
constexpr int64_t kMaxImages = 65535;    // grid.y
constexpr float kInf = 1e8f;             // the reference's INF (exact in fp32): an area >= kInf never wins
constexpr float kDenormFloor = 1e-6f;
constexpr int kFlagsMask = SPH2POB_POINT_CENTER_SAMPLING | SPH2POB_POINT_NORM_ON_BBOX;

// the level table, by value: a point's level is the first one whose end exceeds its index
struct Levels {
    int num;
    int end[kMaxLevels];                 // running sum of n_l
    float lo[kMaxLevels], hi[kMaxLevels], extent[kMaxLevels], norm[kMaxLevels];
};

// the level of point p: compares against the running sums (constant indices: the table stays in scalar registers)
SPHF_DEV int level_index(const Levels& L, int p) {
    int l = 0;
#pragma unroll
    for (int q = 0; q < kMaxLevels - 1; q++) l += (q + 1 < L.num && p >= L.end[q]) ? 1 : 0;
    return l;
}
// the level's row of the table.  The kernel reads it from an LDS copy of the table (a per-lane index into the by-value argument
// would make the compiler spill the whole table to scratch in every lane); the twin indexes the table itself
struct LevelRow { float lo, hi, extent, norm; };
inline LevelRow level_of_point(const Levels& L, int p) {
    const int l = level_index(L, p);
    return LevelRow{L.lo[l], L.hi[l], L.extent[l], L.norm[l]};
}

// the rows of an image that are used: its first k_max, and nothing outside the GT tensor whatever the offsets (device data) say
// (sph2pob_assign.hpp::image_rows is a DIFFERENT rule: it clamps an out-of-range begin into the tensor, here such an image has no rows)
SPHF_DEV int image_rows(int64_t begin, int64_t end, int64_t num_gt, int64_t k_max) {
    if (begin < 0 || begin > num_gt) return 0;
    int64_t k = end - begin;
    k = k < num_gt - begin ? k : num_gt - begin;
    k = k < k_max ? k : k_max;
    return k > 0 ? (int)k : 0;
}

// one GT in pixels: _sph2pix_box_transform then xywh2xyxy (box_formator.py:76-83, :25-31), the area of sph_fcos_head.py:127-128
struct Gt { float x1, y1, x2, y2, area, angle; };

SPHF_DEV Gt gt_pixels(const float* __restrict__ row, int dim, float img_w, float img_h) {
    const float x = (row[0] / 360.0f) * img_w, y = (row[1] / 180.0f) * img_h;
    const float w = (row[2] / 360.0f) * img_w, h = (row[3] / 180.0f) * img_h;
    Gt g;
    g.x1 = x - w / 2.0f; g.y1 = y - h / 2.0f; g.x2 = x + w / 2.0f; g.y2 = y + h / 2.0f;
    g.area = (g.x2 - g.x1) * (g.y2 - g.y1);
    g.angle = dim == 5 ? row[4] : 0.0f;
    return g;
}

// Is the GT a candidate for the point (x, y) of a level (sph_fcos_head.py:139-191)?  Every comparison is false on a NaN, as
// torch's min / max / > / >= / <= are on the reference's tensors: `inside` holds only when no edge is NaN, so the fmaxf chain sees
// no NaN where its value matters.
template <bool CENTER>
SPHF_DEV bool candidate(const Gt& g, float x, float y, float lo, float hi, float extent) {
    const float l = x - g.x1, t = y - g.y1, r = g.x2 - x, b = g.y2 - y;
    bool inside;
    if (CENTER) {   // the centre box of :149-182, built with where
        const float cx = (g.x1 + g.x2) / 2.0f, cy = (g.y1 + g.y2) / 2.0f;
        const float x_min = cx - extent, y_min = cy - extent, x_max = cx + extent, y_max = cy + extent;
        const float c0 = x_min > g.x1 ? x_min : g.x1, c1 = y_min > g.y1 ? y_min : g.y1;
        const float c2 = x_max > g.x2 ? g.x2 : x_max, c3 = y_max > g.y2 ? g.y2 : y_max;
        inside = (x - c0 > 0.0f) & (y - c1 > 0.0f) & (c2 - x > 0.0f) & (c3 - y > 0.0f);
    } else {
        inside = (l > 0.0f) & (t > 0.0f) & (r > 0.0f) & (b > 0.0f);
    }
    const float m = fmaxf(fmaxf(l, t), fmaxf(r, b));
    return inside & (m >= lo) & (m <= hi);
}

// The walk over an image's GT keeps the winner so far: the smallest area among the candidates, the lowest index on ties (strict <
// in ascending order), nothing at or above kInf, nothing with a NaN area
struct Best { float x1, y1, x2, y2, angle, area; int idx; };
SPHF_DEV Best no_best() { return Best{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, kInf, -1}; }
SPHF_DEV void offer(Best& best, const Gt& g, int j, bool cand) {
    if (cand && g.area < best.area) { best.x1 = g.x1; best.y1 = g.y1; best.x2 = g.x2; best.y2 = g.y2; best.angle = g.angle; best.area = g.area; best.idx = j; }
}

// The target row of a point: (l, t, r, b[, angle]) of the winner, every component over `norm` when norm > 0 (fcos_head.py:326-327),
// and the centerness of :426-434 on the row as written; exact zeros without a winner
template <int DIM>
SPHF_DEV float target_row(const Best& best, float x, float y, float norm, float (&t)[5]) {
    if (best.idx < 0) {
#pragma unroll
        for (int c = 0; c < 5; c++) t[c] = 0.0f;
        return 0.0f;
    }
    t[0] = x - best.x1; t[1] = y - best.y1; t[2] = best.x2 - x; t[3] = best.y2 - y; t[4] = best.angle;
    if (norm > 0.0f) {
#pragma unroll
        for (int c = 0; c < DIM; c++) t[c] = t[c] / norm;
    }
    const float lr = fminf(t[0], t[2]) / fmaxf(t[0], t[2]), tb = fminf(t[1], t[3]) / fmaxf(t[1], t[3]);
    return sqrtf(lr * tb);
}

// ---- arguments and workspace ----------------------------------------------------------------------------------------------------
inline int64_t blocks_per_image(int64_t P) { return (P + kBlock - 1) / kBlock; }

// box_dim -> DIM; L outside [1, 8], B outside [0, 65 535], P outside [0, 2^31 - 256), a negative n_l, sum n_l != P, num_gt or k_max
// < 0, k_max > num_gt, img_h / img_w outside [1, 2^24], num_classes < 0 -> SIZE; a NULL table -> NULL; flags, a NaN range, a centre
// extent that is negative or NaN, a norm stride that is not positive -> OPTION (the caller puts the NULL checks of the tensors
// between the two)
inline int check_shape(int64_t P, const int64_t* level_n, int num_levels, int64_t B, int64_t num_gt, int64_t k_max, int box_dim,
                       int64_t img_h, int64_t img_w, int64_t num_classes) {
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (num_levels < 1 || num_levels > kMaxLevels || B < 0 || B > kMaxImages || P < 0 || P >= ((int64_t)1 << 31) - kBlock) return SPH2POB_ERR_SIZE;
    if (num_gt < 0 || k_max < 0 || k_max > num_gt || num_gt >= ((int64_t)1 << 31) || num_classes < 0) return SPH2POB_ERR_SIZE;
    if (img_h < 1 || img_w < 1 || img_h > (1 << 24) || img_w > (1 << 24)) return SPH2POB_ERR_SIZE;
    if (!level_n) return SPH2POB_ERR_NULL;
    int64_t sum = 0;
    for (int l = 0; l < num_levels; l++) {
        if (level_n[l] < 0 || level_n[l] > P) return SPH2POB_ERR_SIZE;
        sum += level_n[l];
    }
    return sum == P ? SPH2POB_OK : SPH2POB_ERR_SIZE;
}

inline int make_levels(const int64_t* level_n, const float* range_lo, const float* range_hi, const float* sample_extent, const float* norm_stride,
                       int num_levels, int flags, Levels* L) {
    if (flags & ~kFlagsMask) return SPH2POB_ERR_OPTION;
    L->num = num_levels;
    int64_t end = 0;
    for (int l = 0; l < kMaxLevels; l++) {
        const bool in = l < num_levels;
        end += in ? level_n[l] : 0;
        L->end[l] = (int)end;
        L->lo[l] = in ? range_lo[l] : 0.0f;
        L->hi[l] = in ? range_hi[l] : 0.0f;
        L->extent[l] = in && (flags & SPH2POB_POINT_CENTER_SAMPLING) ? sample_extent[l] : 0.0f;
        L->norm[l] = in && (flags & SPH2POB_POINT_NORM_ON_BBOX) ? norm_stride[l] : 0.0f;
        if (!in) continue;
        if (L->lo[l] != L->lo[l] || L->hi[l] != L->hi[l]) return SPH2POB_ERR_OPTION;
        if ((flags & SPH2POB_POINT_CENTER_SAMPLING) && !(L->extent[l] >= 0.0f)) return SPH2POB_ERR_OPTION;
        if ((flags & SPH2POB_POINT_NORM_ON_BBOX) && !(L->norm[l] > 0.0f)) return SPH2POB_ERR_OPTION;
    }
    return SPH2POB_OK;
}

// The workspace: per workgroup of the target kernel one double (its centerness sum) and one int (its positives), image-major
struct Workspace { double* sums; int* counts; };
inline int64_t workspace_bytes(int64_t B, int64_t P) {
    if (B < 0 || B > kMaxImages || P < 0 || P >= ((int64_t)1 << 31) - kBlock) return 0;
    return 16 + 12 * B * blocks_per_image(P);
}
inline Workspace carve(void* workspace, int64_t B, int64_t P) {
    uintptr_t p = (reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15;
    Workspace w;
    w.sums = reinterpret_cast<double*>(p);
    w.counts = reinterpret_cast<int*>(p + 8 * (uintptr_t)(B * blocks_per_image(P)));
    return w;
}

// the two normalisers from the totals: max(positives, 1) and max(sum of centerness, 1e-6), each rounded to fp32 once
SPHF_DEV void normalisers(int64_t positives, double centerness_sum, float* avg_factor, float* centerness_denorm) {
    avg_factor[0] = (float)(positives > 1 ? positives : 1);
    const float s = (float)centerness_sum;
    centerness_denorm[0] = s > kDenormFloor ? s : kDenormFloor;
}

// ---- the coder --------------------------------------------------------------------------------------------------------------------
struct Image { float w, h, max_w, max_h; };   // max_* < 0: no clip

// torch.clamp(v, lo, hi): a NaN stays a NaN
SPHF_DEV float clamp_like_torch(float v, float lo, float hi) {
    v = v < lo ? lo : v;
    return v > hi ? hi : v;
}

// its backward: the gradient where v lies in [0, hi], +0 elsewhere (a NaN included)
SPHF_DEV float clamp_gate(float v, float hi, float g) { return (v >= 0.0f && v <= hi) ? g : 0.0f; }

// bbox2distance (:131-163): the GT to pixels, the four distances, clamped to [0, clamp_hi] when `clamp`
template <int DIM>
SPHF_DEV void encode_row(const float* __restrict__ pt, const float* __restrict__ gt, const Image& im, bool clamp, float clamp_hi, float (&d)[5]) {
    const Gt g = gt_pixels(gt, DIM, im.w, im.h);
    d[0] = pt[0] - g.x1; d[1] = pt[1] - g.y1; d[2] = g.x2 - pt[0]; d[3] = g.y2 - pt[1]; d[4] = g.angle;
    if (clamp) {
#pragma unroll
        for (int c = 0; c < 4; c++) d[c] = clamp_like_torch(d[c], 0.0f, clamp_hi);
    }
}

// distance2bbox (:71-128): corners, the clip, xyxy2xywh, _pix2sph_box_transform (box_formator.py:17-23, :85-92).  BWD: `out` is
// the gradient of the distances for the gradient `gb` of the box, as torch's autograd delivers it through that composition — the
// products and quotients in its order, the clamp passing the gradient where the corner lies inside the closed interval
template <int DIM, bool BWD>
SPHF_DEV void decode_row(const float* __restrict__ pt, const float* __restrict__ d, const float* __restrict__ gb, const Image& im, float (&out)[5]) {
    const float x1 = pt[0] - d[0], y1 = pt[1] - d[1], x2 = pt[0] + d[2], y2 = pt[1] + d[3];
    const bool clip_x = im.max_w >= 0.0f, clip_y = im.max_h >= 0.0f;
    if (!BWD) {
        const float cx1 = clip_x ? clamp_like_torch(x1, 0.0f, im.max_w) : x1, cx2 = clip_x ? clamp_like_torch(x2, 0.0f, im.max_w) : x2;
        const float cy1 = clip_y ? clamp_like_torch(y1, 0.0f, im.max_h) : y1, cy2 = clip_y ? clamp_like_torch(y2, 0.0f, im.max_h) : y2;
        out[0] = (((cx1 + cx2) / 2.0f) / im.w) * 360.0f;
        out[1] = (((cy1 + cy2) / 2.0f) / im.h) * 180.0f;
        out[2] = ((cx2 - cx1) / im.w) * 360.0f;
        out[3] = ((cy2 - cy1) / im.h) * 180.0f;
        out[4] = DIM == 5 ? d[4] : 0.0f;
    } else {
        const float gx = ((gb[0] * 360.0f) / im.w) / 2.0f, gy = ((gb[1] * 180.0f) / im.h) / 2.0f;
        const float gw = (gb[2] * 360.0f) / im.w, gh = (gb[3] * 180.0f) / im.h;
        float g_x1 = gx + (-gw), g_y1 = gy + (-gh), g_x2 = gx + gw, g_y2 = gy + gh;
        if (clip_x) { g_x1 = clamp_gate(x1, im.max_w, g_x1); g_x2 = clamp_gate(x2, im.max_w, g_x2); }
        if (clip_y) { g_y1 = clamp_gate(y1, im.max_h, g_y1); g_y2 = clamp_gate(y2, im.max_h, g_y2); }
        out[0] = -g_x1; out[1] = -g_y1; out[2] = g_x2; out[3] = g_y2;
        out[4] = DIM == 5 ? gb[4] : 0.0f;
    }
}

// box_dim -> DIM; n < 0 or >= 2^31 - 256, img_h / img_w outside [1, 2^24] -> SIZE; a NULL tensor with rows -> NULL; a NaN clip
// bound -> OPTION
inline int check_coder(const void* a, const void* b, const void* c, const void* d, int64_t n, int box_dim, int64_t img_h, int64_t img_w,
                       float bound0, float bound1) {
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (n < 0 || n >= ((int64_t)1 << 31) - kBlock || img_h < 1 || img_w < 1 || img_h > (1 << 24) || img_w > (1 << 24)) return SPH2POB_ERR_SIZE;
    if (n > 0 && (!a || !b || !c || !d)) return SPH2POB_ERR_NULL;
    if (bound0 != bound0 || bound1 != bound1) return SPH2POB_ERR_OPTION;
    return SPH2POB_OK;
}

}  // namespace sph2pob_point
