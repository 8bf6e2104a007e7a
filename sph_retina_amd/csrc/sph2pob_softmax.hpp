// Softmax cross-entropy with optional hard-negative mining (SphSSDHead.loss_single, sphdet/models/heads/sph_ssd_head.py:96-161;
// mmdet's cross_entropy + weight_reduce_loss in plain mode): the row arithmetic, the order-preserving loss keys and the argument
// checks, shared by the kernels (sph2pob_softmax.hip) and their CPU twins (sph2pob_host.hip) so that a CPU tensor gets the
// arithmetic, the mined set and the checks a device tensor gets.  The level table is sph2pob_class_levels.hpp's, the cut of an image
// sph2pob_select.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_class_levels.hpp"
#include "sph2pob_get_bboxes.hpp"
#include "sph2pob_head_loss.hpp"
#include "sph2pob_select.hpp"

namespace sph2pob_softmax {

using sph2pob_head::aligned_to;
using sph2pob_head::effective_scale;
using sph2pob_head::kBlock;
using sph2pob_head::kMaxLevels;

constexpr int kMinK = 2, kMaxK = 4096;
constexpr int kCutBlock = 1024;   // threads of the per-image cut workgroup

// ---- one row, cancellation free ----------------------------------------------------------------------------------------------
// m = max_j x_j; e_j = expf(x_j - m), the difference taken in fp32: a correctly rounded fp32 subtraction IS the double difference
// narrowed to fp32.  jx is the one class whose term (exactly 1) is left out of the sums: the target when x_t == m, else the first
// maximum.  q = sum of e_j over j not in {t, jx}, in double.  Then, with et = e_t:
//     t == jx:  R = q        CE = log1p(R)                  sum_{j != t} e_j = q
//     else:     R = q + et   CE = (m - x_t) + log1p(R)      sum_{j != t} e_j = 1 + q
// S = 1 + R;  p_j = e_j / S;  d CE / d x_t = -(sum_{j != t} e_j) / S (never p_t - 1);  d CE / d x_j = p_j.
// The walk over the classes belongs to the caller (NCHW planes, a flat row, the twins' strided loop): pass 1 calls see_max for
// every class, then close_max; pass 2 calls see_sum for every class, then close_sum; pass 3 asks grad(c, x) per class.
struct Row {
    float m, xt, et;
    int t, jm, jx;
    double q, inv, nt;   // nt: sum_{j != t} e_j

    SPHF_DEV void begin(int target) { m = -INFINITY; xt = 0.0f; et = 1.0f; t = target; jm = 0; jx = 0; q = 0.0; inv = 0.0; nt = 0.0; }
    SPHF_DEV void see_max(int c, float x) {
        if (x > m) { m = x; jm = c; }
        if (c == t) xt = x;
    }
    SPHF_DEV void close_max() {
        jx = xt == m ? t : jm;
        et = jx == t ? 1.0f : expf(xt - m);
    }
    SPHF_DEV void see_sum(int c, float x) {
        if (c != t && c != jx) q += (double)expf(x - m);
    }
    // the row's cross-entropy, rounded to fp32 once
    SPHF_DEV float close_sum() {
        const bool top = jx == t;
        const double r = top ? q : q + (double)et;
        nt = top ? q : 1.0 + q;
        inv = 1.0 / (1.0 + r);
        return (float)((top ? 0.0 : (double)m - (double)xt) + log1p(r));
    }
    SPHF_DEV float grad(int c, float x) const {
        return c == t ? -(float)(nt * inv) : (float)((double)expf(x - m) * inv);
    }
};

// ---- one row without a target: the probabilities an inference call selects on and reports (sph2pob_softmax_scores_f32,
// sph2pob_softmax_bboxes_f32 and their twins) ------------------------------------------------------------------------------------
// Row's m and e_j; S = sum_j (double)e_j over ALL classes in ascending class order (the maximum's own term is expf(0) = 1 exactly,
// the 1 Row adds by hand); p_c = (float)((double)e_c / S).  This is Row's p_j = e_j * inv up to the last bit of the double
// quotient (a divide here, Row's product with the reciprocal there) — far below the fp32 narrowing.  A -inf logit: e = 0, p = 0
// exactly.  A NaN or +inf in the row (or no finite logit at all): x - m is NaN for it, S is NaN, every class of the row is NaN.
// The walk belongs to the caller as for Row: see_max for every class, then see_sum for every class, then p(x) per class.
struct Prob {
    float m;
    double s;
    SPHF_DEV void begin() { m = -INFINITY; s = 0.0; }
    SPHF_DEV void see_max(float x) { if (x > m) m = x; }
    SPHF_DEV float e(float x) const { return expf(x - m); }
    SPHF_DEV void add(float ej) { s += (double)ej; }
    SPHF_DEV float of(float ej) const { return (float)((double)ej / s); }
    // a caller that cannot keep e_j between the walks computes it twice (the same bits)
    SPHF_DEV void see_sum(float x) { add(e(x)); }
    SPHF_DEV float p(float x) const { return of(e(x)); }
};

// valid: 0 <= label < K and label != ignore_index; anything else has loss 0, gradient 0 and is neither positive nor negative
SPHF_DEV bool valid_label(int64_t lab, int K, int64_t ignore_index) { return lab >= 0 && lab < (int64_t)K && lab != ignore_index; }
// the row factor cw[label] * w of a valid row; the row loss is (CE * cw) * w and the gradient factor k0 * (cw * w)
SPHF_DEV float class_factor(const float* cw, int64_t lab) { return cw ? cw[lab] : 1.0f; }
SPHF_DEV float row_weight(const float* w, int64_t row) { return w ? w[row] : 1.0f; }
SPHF_DEV float row_loss(float ce, float cwl, float w) { return (ce * cwl) * w; }

// ---- keys: one 32-bit word per row between the passes -------------------------------------------------------------------------
// 0: the row takes no part (invalid label; in mining mode nothing else is 0);  1: a positive;  >= 2: a negative, the ascending
// image of its loss — a larger loss has a larger key, -inf maps to 0x007fffff, every NaN to 0xffffffff (above +inf, as torch.topk
// orders it).  The loss of a mined row is read back from its key: exact, except that -0 comes back as +0 and a NaN as the quiet one.
constexpr unsigned kKeyNone = 0u, kKeyPos = 1u, kKeyNaN = 0xffffffffu;
SPHF_DEV unsigned float_bits(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    unsigned u; __builtin_memcpy(&u, &v, 4); return u;
#endif
}
SPHF_DEV float bits_float(unsigned u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float v; __builtin_memcpy(&v, &u, 4); return v;
#endif
}
SPHF_DEV unsigned loss_key(float l) {
    if (l != l) return kKeyNaN;
    const unsigned u = float_bits(l + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
SPHF_DEV float key_loss(unsigned k) {
    if (k == kKeyNaN) return bits_float(0x7fc00000u);
    return bits_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
// the cut of one image (sph2pob_select.hpp, descending): the k-th largest negative key and the row index below which rows with
// exactly that key are taken.  Nothing mined: key = kKeyNaN, upto = 0
using sph2pob_select::Cut;
SPHF_DEV bool mined(unsigned key, int i, const Cut& c) { return key >= 2u && sph2pob_select::taken<true>(key, i, c); }
// k_b = min(r P_b, N_b)
SPHF_DEV int64_t mined_count(int64_t ratio, int64_t pos, int64_t neg) { const int64_t k = ratio * pos; return k < neg ? k : neg; }

// ---- levels ---------------------------------------------------------------------------------------------------------------------
// The level table: Level, Levels and the KIND_* of sph2pob_class_levels.hpp; a flat level's item is one row, walked with 16-byte
// accesses (FLAT4: K % 4 == 0 and aligned bases) or one element at a time (FLAT1); n_pad is the stride of one image's keys.
// Argument checks of sph2pob_softmax_loss_sum_f32 / its twin, in the documented order: the option here, sizes and pointers in the
// shared walk, which fills the table (`tables`: there)
using namespace sph2pob_class;
constexpr Family kFamily{kMinK, kMaxK, true, ((int64_t)1 << 31) - 8};
inline int make_levels(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                       int64_t B, int64_t K, int64_t neg_pos_ratio, bool tables, Levels* out) {
    if (neg_pos_ratio < -1 || neg_pos_ratio > ((int64_t)1 << 30)) return SPH2POB_ERR_OPTION;
    return walk_levels(kFamily, logits, grads, level_n, level_hw, num_levels, B, K, tables, 16, out);
}

// The workspace: doubles [0, blocks) the row pass's partials, [blocks, blocks + B) the mined sums of the images (mining), one
// spare; then (mining) B cuts and B n_pad keys
struct Workspace {
    double* partial;
    Cut* cut;
    unsigned* keys;
};
inline int64_t partial_doubles(int64_t blocks, int64_t B) { return (blocks + B + 1 + 1) / 2 * 2; }   // keeps what follows 16-byte aligned
inline int64_t workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t B, int64_t K, int mining) {
    Levels L;
    if (make_levels(nullptr, nullptr, level_n, level_hw, num_levels, B, K, -1, false, &L) != SPH2POB_OK) return 0;
    int64_t bytes = 8 * partial_doubles(L.blocks, B);
    if (mining) bytes += ((int64_t)sizeof(Cut) * B + 15) / 16 * 16 + 4 * B * L.n_pad;
    return bytes + 16;
}
// `blocks`: the upper bound workspace_bytes used (the scalar kinds), so that the carve does not move with the alignment of a call
inline Workspace carve(void* workspace, const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t B, int64_t K) {
    Levels U;
    make_levels(nullptr, nullptr, level_n, level_hw, num_levels, B, K, -1, false, &U);
    uintptr_t p = (reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15;
    Workspace w;
    w.partial = reinterpret_cast<double*>(p);
    p += 8 * (uintptr_t)partial_doubles(U.blocks, B);
    w.cut = reinterpret_cast<Cut*>(p);
    p += ((uintptr_t)sizeof(Cut) * (uintptr_t)B + 15) / 16 * 16;
    w.keys = reinterpret_cast<unsigned*>(p);
    return w;
}

// flat (N, K) entries: grad_stride -> OPTION; n < 0, K outside [2, 4096], N K too large -> SIZE
inline int flat_check(int64_t n, int64_t K, int grad_stride) {
    if (grad_stride != 0 && grad_stride != 1) return SPH2POB_ERR_OPTION;
    if (n < 0 || K < kMinK || K > kMaxK || n > ((int64_t)1 << 38) / K) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}

// ---- the probability pass of inference: the level table of sph2pob_softmax_scores_f32 and of stage 0 of
// sph2pob_softmax_bboxes_f32 --------------------------------------------------------------------------------------------------------
// Input (B, A K, H, W) or (B, n, K), background last in each anchor's K; output fp32 in the same layout without it: (B, A C, H, W)
// or (B, n, C), C = K - 1.  kind: how a thread's item maps onto memory
//   PROB_NCHW4  four consecutive positions of one (b, a) per item: one vector access per class plane (H W % 4 == 0, aligned bases)
//   PROB_NCHW1  one position per item
//   PROB_FLAT   one row per item; K <= kHoldK: a workgroup's kBlock rows are one contiguous span, staged through LDS with
//               coalesced loads and stores; above it every lane walks its own row in memory
// K <= kHoldK: a row's logits are read once and held (registers, or the LDS stage); above it the three walks read them again.
// The arithmetic is Prob's on either path: the same bits.
constexpr int kHoldK = 40;
enum { PROB_NCHW4 = 0, PROB_NCHW1 = 1, PROB_FLAT = 2 };
struct ProbLevel {
    const void* logits;    // float, or the 16-bit type of the _h16 entries
    float* out;
    int64_t items;         // work items of the level
    int hw, a, kind;       // H W (0: flat); anchors per position
    int block_off;         // first workgroup of the level
};
struct ProbLevels {
    ProbLevel lv[kMaxLevels];
    int num, blocks;
};
// Argument checks of sph2pob_softmax_scores_f32 / its twin, in the documented order; fills the table.  elem_bytes: 4, or 2 for
// the 16-bit entries (a vector access of four logits is then 8 bytes)
inline int make_prob_levels(const void* const* logits, void* const* out, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                            int64_t B, int64_t C, int elem_bytes, ProbLevels* res) {
    const int64_t K = C + 1;
    if (num_levels < 1 || num_levels > kMaxLevels || B < 0 || B > 65535 || C < kMinK - 1 || C > kMaxK - 1) return SPH2POB_ERR_SIZE;
    if (!level_n || !logits || !out) return SPH2POB_ERR_NULL;
    ProbLevels L{};
    L.num = num_levels;
    int64_t blocks = 0;
    for (int l = 0; l < num_levels; l++) {
        const int64_t n = level_n[l], hw = level_hw ? level_hw[l] : 0;
        if (n < 0 || hw < 0 || (hw > 0 && n % hw != 0) || n > kMaxLevelElems / K || (B > 0 && n * K > kMaxLevelElems / B)) return SPH2POB_ERR_SIZE;
        ProbLevel& d = L.lv[l];
        d.logits = logits[l]; d.out = (float*)out[l];
        if (B * n > 0 && (!d.logits || !d.out)) return SPH2POB_ERR_NULL;
        d.hw = (int)hw; d.a = hw > 0 ? (int)(n / hw) : 1;
        d.kind = hw == 0 ? PROB_FLAT : (hw % 4 == 0 && aligned_to(d.logits, 4 * elem_bytes) && aligned_to(d.out, 16)) ? PROB_NCHW4 : PROB_NCHW1;
        d.items = d.kind == PROB_NCHW4 ? B * n / 4 : B * n;
        d.block_off = (int)blocks;
        blocks += (d.items + kBlock - 1) / kBlock;
    }
    L.blocks = (int)blocks;   // (every level holds fewer than 2^31 elements: fewer than 2^26 workgroups in all)
    *res = L;
    return SPH2POB_OK;
}
// Argument checks of sph2pob_softmax_bboxes_f32 / _h16 and the twin, in the documented order: box_dim and the options as
// sph2pob_test_bboxes_f32 has them, K = C + 1 <= kMaxK with the sizes (C >= 1 is the pipeline's own check), the rest of that entry's
// checks, then the output pointers.  Fills the level table of the pipeline, its scores still the head's logits
inline int make_softmax_levels(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const sph2pob_gb::Shape& sh,
                               const sph2pob_gb::Selection& sel, const sph2pob_gb::Coder& cd, const sph2pob_gb::Nms& nms,
                               const sph2pob_gb::Outputs& out, sph2pob_gb::Levels* res) {
    const int rc = sph2pob_gb::make_levels(cls_scores, bbox_preds, anchors, sh, sel, cd, nms, res);
    if (rc == SPH2POB_ERR_DIM || rc == SPH2POB_ERR_OPTION) return rc;
    if (sh.num_classes > kMaxK - 1) return SPH2POB_ERR_SIZE;
    if (rc) return rc;
    return out.check(nms.max_per_img);
}
// the first logit of an NCHW item and of the probabilities it writes: position p of anchor (b, a) — class j lies j * hw further on
SPHF_DEV void prob_nchw_span(int64_t ba, int64_t p, int hw, int K, int64_t* in, int64_t* out) {
    *in = ba * K * hw + p; *out = ba * (K - 1) * hw + p;
}

}  // namespace sph2pob_softmax
