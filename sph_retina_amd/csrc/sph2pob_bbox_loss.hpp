// Fused box-regression loss — the regression half of SphRetinaHead.loss_single (sphdet/models/heads/sph_retina_head.py:252-265):
// the level table, the span geometry and the argument checks, shared by the kernels (sph2pob_bbox_loss.hip) and their CPU twin
// (sph2pob_host.hip).  The arithmetic per positive anchor is the composition's, unchanged: decode_one<DIM, true>
// (sph2pob_coder.hpp) then pair_loss<DIM, true, FAST> (sph2pob_loss.hpp).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_coder.hpp"
#include "sph2pob_head_loss.hpp"
#include "sph2pob_loss.hpp"

namespace sph2pob_bbox {

using sph2pob_head::aligned16;
using sph2pob_head::effective_scale;
using sph2pob_head::kMaxLevels;

constexpr int kWaves = 4;                  // waves of a workgroup; each owns one span
constexpr int kTile = 1440;                // floats of a wave's gradient tile in LDS: 32 positions x 9 anchors x 5 components
constexpr int kMaxSpanPos = 256;           // positions of a span at most
constexpr int kStack = kTile / 4;          // anchors of a span at most (box_dim >= 4): the bound of the positives' stack
constexpr int64_t kMaxLevelElems = ((int64_t)1 << 31) - 4096;   // B n_l box_dim of one level: 32-bit indices inside a level

// One level of one call.  A span is `ps` consecutive positions p = h W + w with all their A anchors (a flattened level: A = 1,
// a position is an anchor): the anchors [p_lo A, (p_lo + ps) A) of one image, contiguous in the level's anchor order.
struct Level {
    const float* pred;     // NCHW (B, A dim, H, W) or flat (B, n_l, dim)
    float* grad;           // laid out like pred; NULL in a forward-only call
    int n, hw, a;          // anchors of the level; H W (0: flat); anchors per position
    int pos, ps, spans;    // positions; positions of a span (a multiple of 4); spans of one image
    int items;             // B spans: one per wave
    int vec;               // the span's gradient rows leave in whole 16-byte stores
    int block_off;         // first workgroup of the level
    int64_t row_off;       // index of the level's first anchor inside an image's n rows
};
struct Levels {
    Level lv[kMaxLevels];
    int num, blocks;       // levels; workgroups of the whole call
    int64_t n_total;       // anchors of one image, all levels
    int64_t rows;          // B n
};

// the option checks every entry starts with, in the order of the IoU loss entries
inline int check_options(int box_dim, const float* weight, int weight_dim, float max_ratio, int coder_flags, int loss_mode_flags) {
    const int loss_mode = loss_mode_flags & 0xff;
    if (loss_mode_flags & ~(0xff | SPH2POB_FLAG_REFERENCE_ORDER)) return SPH2POB_ERR_OPTION;
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (loss_mode < 0 || loss_mode > 3) return SPH2POB_ERR_OPTION;
    if (weight && weight_dim != 1 && weight_dim != box_dim) return SPH2POB_ERR_OPTION;
    if ((coder_flags & ~3) || !(max_ratio >= 0.0f)) return SPH2POB_ERR_OPTION;
    return SPH2POB_OK;
}

// Shape checks in the documented order; fills the table.  `tables` false: shapes only (the workspace size).  `vec_bytes`: the
// alignment a four-element store needs — 16 for fp32 levels, 8 for the 16-bit levels of the _h16 entries, whose pointers the table
// keeps as float* all the same (sph2pob_head_loss.hpp, level_ptr).
inline int make_levels(const void* const* preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                       int64_t B, int dim, bool tables, Levels* out, int vec_bytes = 16) {
    if (dim != 4 && dim != 5) return SPH2POB_ERR_DIM;
    if (num_levels < 1 || num_levels > kMaxLevels || B < 0 || B > 65535) return SPH2POB_ERR_SIZE;
    if (!level_n || (tables && !preds)) return SPH2POB_ERR_NULL;
    Levels L{};
    L.num = num_levels;
    int64_t blocks = 0, rows = 0;
    for (int l = 0; l < num_levels; l++) {
        const int64_t n = level_n[l], hw = level_hw ? level_hw[l] : 0;
        if (n < 0 || hw < 0 || (hw > 0 && n % hw != 0) || n > kMaxLevelElems / dim || (B > 0 && n * dim > kMaxLevelElems / B)) return SPH2POB_ERR_SIZE;
        const int64_t a = hw > 0 ? n / hw : 1;
        if (n > 0 && a * dim * 4 > kTile) return SPH2POB_ERR_SIZE;   // four positions of every anchor must fit the tile
        Level& d = L.lv[l];
        d.n = (int)n; d.hw = (int)hw; d.a = (int)a;
        d.pos = n > 0 ? (int)(hw > 0 ? hw : n) : 0;
        int ps = n > 0 ? kTile / (int)(a * dim) : 4;
        ps = (ps < kMaxSpanPos ? ps : kMaxSpanPos) & ~3;
        d.ps = ps;
        d.spans = (d.pos + ps - 1) / ps;
        d.items = (int)(B * d.spans);
        d.pred = tables ? (const float*)preds[l] : nullptr;
        d.grad = tables && grads ? (float*)grads[l] : nullptr;
        if (tables && B * n > 0 && (!d.pred || (grads && !d.grad))) return SPH2POB_ERR_NULL;
        d.vec = d.grad && sph2pob_head::aligned_to(d.grad, vec_bytes) && (hw > 0 ? hw % 4 == 0 : (n * dim) % 4 == 0);
        d.block_off = (int)blocks;
        d.row_off = rows;
        blocks += (d.items + kWaves - 1) / kWaves;
        rows += n;
        if (blocks >= ((int64_t)1 << 31) - 1) return SPH2POB_ERR_SIZE;
    }
    L.blocks = (int)blocks; L.n_total = rows; L.rows = B * rows;
    *out = L;
    return SPH2POB_OK;
}

// workgroups of the partial-sum pass of a call with these shapes + 1
inline int64_t workspace_doubles(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t B, int dim) {
    Levels L;
    if (make_levels(nullptr, nullptr, level_n, level_hw, num_levels, B, dim, false, &L) != SPH2POB_OK) return 0;
    return (int64_t)L.blocks + 1;
}

// offset of component 0 of anchor i (inside the level) of image b in the level's pred / grad, and the stride between components
SPHF_DEV int64_t delta_offset(const Level& lv, int dim, int64_t b, int64_t i, int64_t* stride) {
    if (lv.hw > 0) {
        const int64_t p = i / lv.a, a = i - p * lv.a;
        *stride = lv.hw;
        return ((b * lv.a + a) * dim) * lv.hw + p;
    }
    *stride = 1;
    return (b * lv.n + i) * dim;
}

}  // namespace sph2pob_bbox
