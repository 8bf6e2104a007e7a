// Shared by the assigner unit (sph2pob_assign.hip: the matrix epilogue, the fused route, the batched anchor targets) and its CPU
// twins (sph2pob_host.hip): the assignment rule and its threshold step, the target row of one anchor, and the argument checks, so
// that a CPU tensor gets the rule, the targets and the checks a device tensor gets.  Also here, once, for every target unit
// (sph2pob_rcnn_targets.{hpp,hip} too): the GT rows of an image (image_rows) and, device only, the packed max / first-argmax keys.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_coder.hpp"
#include "sph2pob_loss.hpp"

namespace sph2pob_assign {

#define SPHA_DEV __host__ __device__ __forceinline__

constexpr int kTile = 256;   // columns (anchors) of one workgroup: the kernels' block size, and what the size bound on n leaves room for

// MaxIoUAssigner's options (max_iou_assigner.py:45-65) as the entry points take them
struct Rule {
    float pos_thr, neg_lo, neg_hi, min_pos;
    int low_quality, assign_all;
};

// the threshold step (max_iou_assigner.py:177-186) on a column's maximum m at row am: -1 neither, 0 negative, am + 1 positive.
// Every comparison is false for a NaN maximum: -1.
SPHA_DEV int64_t threshold_index(float m, int64_t am, const Rule& r) {
    int64_t a = -1;
    if (m >= r.neg_lo && m < r.neg_hi) a = 0;
    if (m >= r.pos_thr) a = am + 1;
    return a;
}

// The targets of one anchor from its assigned index a (> 0 positive, 0 negative, -1 neither), AnchorHead._get_targets_single
// (anchor_head.py:254-285, PseudoSampler):
//   label gt_labels[a - 1] (0 without labels) | num_classes; label_weight 1 (pos_weight on positives when > 0) | 0 for -1;
//   t the GT box, or its deltas w.r.t. the anchor (ENCODE: sph2pob_coder::encode_one, the coder kernel's function) | 0;
//   box_weight 1 | 0.
// `anchor` and `g` (GT a - 1 of the image) are rows of DIM floats, read for a positive only; `gt_labels`: the image's, or null.
struct TargetRow { int64_t label; float label_weight, t[5], box_weight; };
template <int DIM, bool ENCODE>
SPHA_DEV TargetRow target_row(int64_t a, const float* anchor, const float* g, const int64_t* gt_labels, int64_t num_classes, float pos_weight,
                              const sph2pob_coder::Norm& nm) {
    const bool pos = a > 0;
    TargetRow r{pos ? (gt_labels ? gt_labels[a - 1] : 0) : num_classes, pos ? (pos_weight <= 0.0f ? 1.0f : pos_weight) : (a == 0 ? 1.0f : 0.0f),
                {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, pos ? 1.0f : 0.0f};
    if (pos) {
        if constexpr (ENCODE) sph2pob_coder::encode_one<DIM>(anchor, g, nm, r.t);
        else {
#pragma unroll
            for (int c = 0; c < DIM; c++) r.t[c] = g[c];
        }
    }
    return r;
}

// rows of image b in the concatenated GT (K rows), as the batched anchor targets, the R-CNN stage targets and their twins take
// them: offsets clamped to [0, K], the count to [0, k_max] (later rows are not assigned)
// (sph2pob_point_targets.hpp::image_rows is a DIFFERENT rule: an out-of-range begin gives no rows there, not a clamp)
struct ImageRows { int64_t lo; int k; };
SPHA_DEV ImageRows image_rows(const int64_t* gt_offsets, int64_t b, int64_t K, int64_t k_max) {
    int64_t lo = gt_offsets[b], hi = gt_offsets[b + 1];
    lo = lo < 0 ? 0 : (lo > K ? K : lo);
    hi = hi < 0 ? 0 : (hi > K ? K : hi);
    const int64_t k = hi - lo;
    return ImageRows{lo, (int)(k < 0 ? 0 : (k > k_max ? k_max : k))};
}

#if defined(__HIPCC__)
// ---- packed keys: order-preserving, for max / first-argmax reductions with one atomic.  (float bits mapped to an unsigned order)
// << 32 | an index that DEcreases with the position, so that the maximum key is the maximum value and, among equal values, the
// SMALLEST index — what torch.max(dim) returns.  IoUs are >= +0 (the kernels never produce -0) or -1 for ignored columns; a NaN
// sorts above every number.  `*_bits`: from a value's ordered bits (a wave has reduced them already). ----
__device__ __forceinline__ unsigned ordered_bits(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// the column key (and the matrix route's row key): low word = ~index
__device__ __forceinline__ unsigned long long pack_max_key_bits(unsigned ordered, unsigned j) {
    return ((unsigned long long)ordered << 32) | (unsigned)(0xffffffffu - j);
}
__device__ __forceinline__ unsigned long long pack_max_key(float v, int64_t j) { return pack_max_key_bits(ordered_bits(v), (unsigned)j); }
__device__ __forceinline__ int64_t max_key_index(unsigned long long key) { return (int64_t)(0xffffffffu - (unsigned)key); }
// the fused assigner's row key keeps bit 0 of the low word free for a "this value occurs at more than one column of the
// tile" flag: low = (0x7fffffff - index) << 1 | flag (indices < 2^31)
__device__ __forceinline__ unsigned long long pack_row_key_bits(unsigned ordered, unsigned j) {
    return ((unsigned long long)ordered << 32) | ((0x7fffffffu - j) << 1);
}
__device__ __forceinline__ unsigned long long pack_row_key(float v, unsigned j) { return pack_row_key_bits(ordered_bits(v), j); }
__device__ __forceinline__ unsigned row_key_index(unsigned long long key) { return 0x7fffffffu - ((unsigned)key >> 1); }
__device__ __forceinline__ float unpack_max_val(unsigned long long key) {
    unsigned u = (unsigned)(key >> 32);
    u = (u & 0x80000000u) ? (u & 0x7fffffffu) : ~u;
    return __uint_as_float(u);
}
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
__device__ __forceinline__ unsigned wave_max_u32(unsigned v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned w = __shfl_xor(v, o, 64);
        v = w > v ? w : v;
    }
    return v;
}
#endif

// ---- argument checks, in the documented order.  `rc` is what check_common(box_dim, variant, edge, 0) answered
// (sph2pob_iou_entry.hpp, next to dispatch()). ----
inline int closed_form_only(int rc, int variant) {   // the kernels that carry the reductions: standard / efficient, closed form
    if (rc) return rc;
    return ((variant & 0xff) > SPH2POB_VARIANT_EFFICIENT || (variant & SPH2POB_FLAG_REFERENCE_ORDER)) ? SPH2POB_ERR_OPTION : SPH2POB_OK;
}
// the fused single-image entries: column indices travel in 31 bits of a key, col_offset + n among them
inline int assign_fused_check(int rc, int64_t k, int64_t n, int variant, int64_t col_offset) {
    if ((rc = closed_form_only(rc, variant))) return rc;
    if (k <= 0 || n <= 0 || n >= ((int64_t)1 << 31) - kTile || k > (int64_t)65535 * 4 || col_offset < 0 || col_offset + n > (int64_t)0x7ffffffe)
        return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}
// the batched route that carries the per-pair functions: every variant the closed-form entry does not serve
inline int per_pair_only(int rc, int variant) {
    if (rc) return rc;
    return ((variant & 0xff) < SPH2POB_VARIANT_LEGACY || (variant & SPH2POB_FLAG_REFERENCE_ORDER)) ? SPH2POB_ERR_OPTION : SPH2POB_OK;
}
// sph2pob_anchor_targets_f32 / sph2pob_anchor_targets_any_f32 and their twins; `rc`: what the entry's variant rule
// (closed_form_only / per_pair_only) answered; `need_buffers`: workspace (for k_max > 0) and state are required — the twins use neither
inline int anchor_targets_check(int rc, const float* anchors, int64_t n, const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets,
                                int64_t num_images, int64_t num_gt, int64_t k_max, const int64_t* assigned_gt_inds,
                                const float* max_overlaps, const int64_t* assigned_labels, const int64_t* labels, const float* label_weights,
                                const float* bbox_targets, const float* bbox_weights, const int64_t* num_pos, const int64_t* num_neg,
                                const float* avg_factor, bool need_buffers, const void* workspace, const void* state) {
    if (rc) return rc;
    if (num_images <= 0 || num_images > 65535 || num_gt < 0 || k_max < 0 || k_max > num_gt || k_max > (int64_t)65535 * 4 || n <= 0 ||
        n >= ((int64_t)1 << 31) - kTile || num_gt > sph2pob::kMaxElems)
        return SPH2POB_ERR_SIZE;
    if (!anchors || !gt_offsets || (num_gt > 0 && !gt) || (need_buffers && ((k_max > 0 && !workspace) || !state)) || !assigned_gt_inds ||
        !max_overlaps || (assigned_labels && !gt_labels && num_gt > 0) || !labels || !label_weights || !bbox_targets || !bbox_weights || !num_pos ||
        !num_neg || !avg_factor)
        return SPH2POB_ERR_NULL;
    return SPH2POB_OK;
}

}  // namespace sph2pob_assign
