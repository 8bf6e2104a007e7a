// The level table of the classification heads (sph2pob_focal, sph2pob_softmax): one Level / Levels, one walk over a call's levels
// with its size guards and its alignment rule, and the span of an anchor's class row.  Plain host + device code, used by the
// kernels and by their CPU twins (sph2pob_host.hip).  What a family checks about its own options stays in its make_levels, in
// front of the walk; what differs about the shapes is a Family.
#pragma once
#include <stdint.h>

#include "sph2pob_head_loss.hpp"

namespace sph2pob_class {

using sph2pob_head::aligned_to;
using sph2pob_head::kBlock;
using sph2pob_head::kMaxLevels;

constexpr int64_t kMaxLevelElems = ((int64_t)1 << 31) - 4096;   // elements of one level: 32-bit indices inside a level

// kind: how a thread's item maps onto memory (C: the channels of an anchor — the classes of focal, the K scores of softmax)
//   0  NCHW (B, A C, H, W), four consecutive positions p = h W + w of one (b, a) per item: one vector access per class plane, at stride H W
//   1  NCHW, one position per item (H W % 4 != 0 or a base that is not aligned to a vector access)
//   2  flat (B, n_l, C), one vector access at a time — focal: four consecutive elements per item; softmax: one row per item (C % 4 == 0)
//   3  flat, one element at a time — focal: one element per item; softmax: one row per item
enum { KIND_NCHW4 = 0, KIND_NCHW1 = 1, KIND_FLAT4 = 2, KIND_FLAT1 = 3 };
struct Level {
    const float* logits;   // (the 16-bit levels of an _h16 entry are kept as float* all the same: sph2pob_head_loss.hpp, level_ptr)
    float* grad;           // laid out like logits; NULL in a forward-only call
    int n, hw, a, kind;    // anchors of the level; H W (0: flat); anchors per position
    int items;             // work items of the level
    int block_off;         // first workgroup of the level
    int64_t row_off;       // index of the level's first anchor inside an image's n rows
};
struct Levels {
    Level lv[kMaxLevels];
    int num, blocks;       // levels; workgroups of one pass over them
    int64_t n_total;       // anchors of one image, all levels
    int64_t elems, rows;   // B n C; B n
    int64_t n_pad;         // n_total rounded up to 4
};

// What the walk has to know about a family.  flat_rows: a flat level's item is one row, the vector kind when C % 4 == 0 (softmax);
// otherwise the elements themselves, four per item when B n C % 4 == 0 (focal)
struct Family {
    int64_t min_channels, max_channels;   // C outside -> SIZE
    bool flat_rows;
    int64_t max_rows;                     // n_total at or above -> SIZE
};

// The size and pointer checks of a *_loss_sum entry / its twin, in the documented order (SIZE, then NULL; level by level); fills
// the table.  `tables` false: shapes only (the workspace size), every level counted with its scalar kind (an upper bound on the
// workgroups).  `vec_bytes`: the alignment the vector kinds need — four elements: 16 for fp32 levels, 8 for 16-bit ones.
inline int walk_levels(const Family& F, const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                       int num_levels, int64_t B, int64_t C, bool tables, int vec_bytes, Levels* out) {
    if (num_levels < 1 || num_levels > kMaxLevels || B < 0 || B > 65535 || C < F.min_channels || C > F.max_channels) return SPH2POB_ERR_SIZE;
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
            d.kind = al && (F.flat_rows ? C : elems) % 4 == 0 ? KIND_FLAT4 : KIND_FLAT1;
            items = F.flat_rows ? B * n : d.kind == KIND_FLAT4 ? elems / 4 : elems;
        }
        d.items = (int)items;
        d.block_off = (int)blocks;
        d.row_off = rows;
        blocks += (items + kBlock - 1) / kBlock;
        rows += n;
        L.elems += elems;
        if (blocks >= ((int64_t)1 << 31) - 1 || rows >= F.max_rows) return SPH2POB_ERR_SIZE;
    }
    L.blocks = (int)blocks; L.n_total = rows; L.n_pad = (rows + 3) / 4 * 4; L.rows = B * rows;
    *out = L;
    return SPH2POB_OK;
}

// element (b, anchor i of the level, channel c) of a level = base + c * stride — the twins' walk; the kernels' items keep their
// own 32-bit index arithmetic
SPHF_DEV void class_row_span(const Level& lv, int64_t C, int64_t b, int64_t i, int64_t* base, int64_t* stride) {
    if (lv.hw > 0) {
        const int64_t p = i / lv.a, a = i - p * lv.a;
        *base = (b * lv.a + a) * C * lv.hw + p; *stride = lv.hw;
    } else {
        *base = (b * lv.n + i) * C; *stride = 1;
    }
}

}  // namespace sph2pob_class
