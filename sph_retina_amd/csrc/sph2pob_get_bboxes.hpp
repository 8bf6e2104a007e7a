// Shared by the batched inference entries (sph2pob_test_bboxes_f32 and its restricted front-end sph2pob_get_bboxes_f32, the softmax,
// FCOS and R-CNN entries: sph2pob_get_bboxes.hip, the NMS stage in sph2pob_nms.hip) and the CPU twins (sph2pob_host.hip): the parameter
// blocks, the level table, the order-preserving score keys, the score activation, the argument checks (the NMS entries' option check
// among them), the candidate sources and the declarations of the NMS stage, so that a CPU tensor gets the order, the arithmetic
// and the checks a device tensor gets.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_coder.hpp"
#include "sph2pob_point_targets.hpp"

namespace sph2pob_gb {

#define SPHG_DEV __host__ __device__ __forceinline__

constexpr int kMaxLevels = 8;
constexpr int kNmsIdxBits = 14, kNmsClsBits = 18;   // the composite NMS key: K <= 16 384 candidates, class ids in [0, 262 143]
constexpr int kChunkElems = 1 << 14;                // scores per streaming chunk of the selection kernels (sph2pob_get_bboxes.hip)
constexpr int kBuildBlock = 256;                    // threads of a cand_build workgroup: one tile of the level's selection

// The arguments of an inference entry, by concern.  The extern "C" entries and their _cpu twins fill these once; everything below
// them takes the blocks.  Shape: what the level table is sized from (level_hw NULL: every level is flat); Coder: the delta coder,
// the state of decode_one; Frame: the point coder's image as an entry gets it (a checked size is exact in fp32)
struct Shape { const int64_t* level_n; const int64_t* level_hw; int num_levels; int64_t num_images, num_classes; int box_dim; };
struct Selection { int activation; float score_thr; int64_t nms_pre; };
struct Coder { sph2pob_coder::Norm nm; float max_ratio; int coder_flags; float ctr_clamp; };
struct Nms { int variant_flags, class_agnostic; float iou_threshold; int64_t max_per_img; };
struct Frame {
    int64_t img_h, img_w;
    float max_h, max_w;
    sph2pob_point::Image image() const { return sph2pob_point::Image{(float)img_w, (float)img_h, max_w, max_h}; }
};
struct Outputs {
    float* dets; int64_t* labels; int64_t* prior_inds; int64_t* num_dets;
    // the rows may be missing only when there are none
    int check(int64_t max_per_img) const { return !num_dets || (max_per_img > 0 && (!dets || !labels || !prior_inds)) ? SPH2POB_ERR_NULL : SPH2POB_OK; }
};
// (the normalisation is read only for a box_dim the checks will accept: means / stds hold box_dim floats)
inline Coder make_coder(const float* means_host, const float* stds_host, int box_dim, float max_ratio, int coder_flags, float ctr_clamp) {
    return Coder{sph2pob_coder::make_norm(means_host, stds_host, box_dim == 4 || box_dim == 5 ? box_dim : 0), max_ratio, coder_flags, ctr_clamp};
}

// f(std::integral_constant<int, box_dim>) for a checked box_dim; f(T{}) for the element type of an _h16 entry's dtype (checked by
// the entry), and the same with dtype 0 = float
template <class F>
auto with_dim(int box_dim, F&& f) { return box_dim == 4 ? f(std::integral_constant<int, 4>{}) : f(std::integral_constant<int, 5>{}); }
template <class F>
auto with_h16(int dtype, F&& f) { return dtype == SPH2POB_DTYPE_F16 ? f(_Float16{}) : f(__bf16{}); }
template <class F>
auto with_f32_or_h16(int dtype, F&& f) { return dtype == 0 ? f(float{}) : with_h16(dtype, f); }

// One level of the head for one call.  A score tensor is read in MEMORY order m in [0, count) per image and mapped to the
// reference's logical candidate index f = ((h W + w) A + a) C + c:
//   NCHW (B, A C, H, W):  m = ch * hw + p  ->  f = p * (A C) + ch      (hw = H W, ac = A C)
//   flat (B, n, C):       m = f                                        (hw = count, ac = 1: the same formula)
struct Level {
    const float* cls;      // scores or logits; the _h16 entries keep their 16-bit pointers here too and read them as T
    const float* bbox;     // deltas, laid out like cls (and of its element type)
    const float* anchors;  // (n, dim)
    int n;                 // anchors of the level
    int count;             // n * C candidates per image
    int hw, ac;            // see above
    int sp, a;             // bbox gather: spatial size and anchors per location (NCHW), sp = 0 for the flat layout
    int cap;               // min(nms_pre, count): the level's share of the candidate block
    int prior_off;         // index of the level's first anchor in cat(mlvl_anchors)
    int chunk_off;         // first streaming chunk of the level (the next level's follows; see Levels::chunks)
    int64_t buf_off;       // first survivor slot of the level inside one image's survivor buffer
};
struct Levels {
    Level lv[kMaxLevels];
    int num;
    int chunks;            // streaming chunks of one image, all levels
    int k_cap;             // sum of cap: candidate stride of one image
    int64_t total;         // sum of count: survivor slots of one image
};

// larger score -> smaller unsigned; the order of torch's device sort by bit pattern except that -0 is +0
SPHG_DEV unsigned bits_of(float v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __float_as_uint(v);
#else
    unsigned u; __builtin_memcpy(&u, &v, 4); return u;
#endif
}
SPHG_DEV float float_of(unsigned u) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __uint_as_float(u);
#else
    float v; __builtin_memcpy(&v, &u, 4); return v;
#endif
}
SPHG_DEV unsigned desc_score_bits(float v) {
    unsigned u = bits_of(v + 0.0f);
    u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ~u;
}
SPHG_DEV float score_of_desc_bits(unsigned d) {
    const unsigned u = ~d;
    return float_of((u & 0x80000000u) ? (u & 0x7fffffffu) : ~u);
}
SPHG_DEV unsigned long long nms_class_key(int64_t c, float score, int j) {
    return ((unsigned long long)(c & (((int64_t)1 << kNmsClsBits) - 1)) << (32 + kNmsIdxBits)) |
           ((unsigned long long)desc_score_bits(score) << kNmsIdxBits) | (unsigned)j;
}

// the score a candidate is selected on AND reported with: fp32, 1 / (1 + exp(-x)) with the library expf and an IEEE divide
SPHG_DEV float activate(float x, int activation) { return activation ? 1.0f / (1.0f + expf(-x)) : x; }

// Selection histogram: a monotone map of the descending score key onto kBins bins, 512 bins per octave downwards from 1.0
// (probabilities fill the bins evenly; anything above 1 lands in bin 0, anything below 2^-16 in the last bin).  Any monotone
// map is correct: the bins only bound how many survivors the exact stage has to look at.
constexpr int kBins = 8192, kBinShift = 14;
SPHG_DEV int score_bin(unsigned dkey) {
    const unsigned one = 0x407fffffu;   // desc_score_bits(1.0f)
    if (dkey <= one) return 0;
    const unsigned b = (dkey - one) >> kBinShift;
    return b < (unsigned)kBins ? (int)b : kBins - 1;
}

inline int64_t k_cap_of(const int64_t* level_n, int num_levels, int64_t num_classes, int64_t nms_pre) {
    int64_t k = 0;
    for (int l = 0; l < num_levels; l++) {
        const int64_t c = level_n[l] * num_classes;
        k += c < nms_pre ? c : nms_pre;
    }
    return k;
}

// Option check of the NMS entries (sph2pob_nms_segmented_f32, sph2pob_nms_f32, sph2pob_batched_nms_f32) and of the host twin.  Not
// check_common(): a BFoV-only variant with box_dim 5 is an OPTION error here, not a DIM error.
inline int nms_check_options(int box_dim, int variant_flags) {
    const int variant = variant_flags & 0xff;
    // SPH2POB_FLAG_ROBUST_PARALLEL is accepted and has no effect here (a near-parallel pair is far above any threshold)
    if (variant_flags & ~(0xff | SPH2POB_FLAG_REFERENCE_ORDER | SPH2POB_FLAG_ROBUST_PARALLEL | SPH2POB_FLAG_NAIVE_TAN)) return SPH2POB_ERR_OPTION;
    if ((variant_flags & SPH2POB_FLAG_NAIVE_TAN) && variant != SPH2POB_VARIANT_NAIVE) return SPH2POB_ERR_OPTION;
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (variant != SPH2POB_VARIANT_STANDARD && variant != SPH2POB_VARIANT_EFFICIENT && variant != SPH2POB_VARIANT_UNBIASED &&
        variant != SPH2POB_VARIANT_NAIVE)
        return SPH2POB_ERR_OPTION;
    return SPH2POB_OK;
}

// What sph2pob_get_bboxes_f32 accepts of the variants sph2pob_test_bboxes_f32 serves (its own check, in front of the shared ones)
inline bool closed_form_variant(int variant) {
    const int v = variant & 0xff;
    return (v == SPH2POB_VARIANT_STANDARD || v == SPH2POB_VARIANT_EFFICIENT) && !(variant & ~(0xff | SPH2POB_FLAG_ROBUST_PARALLEL));
}

// Argument checks of sph2pob_test_bboxes_f32 and its twin, in the documented order, in two parts: the shapes (all the workspace
// size needs; level_hw may be NULL = flattened layout) fill the level table, then the pointer tables are checked and entered.
inline int make_level_shapes(const Shape& sh, const Selection& sel, const Coder& cd, const Nms& nms, bool have_tables, Levels* out) {
    if (sh.box_dim != 4 && sh.box_dim != 5) return SPH2POB_ERR_DIM;
    const int variant = nms.variant_flags, v = variant & 0xff;
    if ((v != SPH2POB_VARIANT_STANDARD && v != SPH2POB_VARIANT_EFFICIENT && v != SPH2POB_VARIANT_UNBIASED && v != SPH2POB_VARIANT_NAIVE) ||
        (variant & ~(0xff | SPH2POB_FLAG_ROBUST_PARALLEL | SPH2POB_FLAG_NAIVE_TAN)) ||
        ((variant & SPH2POB_FLAG_NAIVE_TAN) && v != SPH2POB_VARIANT_NAIVE) || nms.class_agnostic < 0 || nms.class_agnostic > 1 ||
        sel.activation < 0 || sel.activation > 1 || (cd.coder_flags & ~3) || !(cd.max_ratio >= 0.0f))
        return SPH2POB_ERR_OPTION;
    if (sh.num_levels < 1 || sh.num_levels > kMaxLevels || sh.num_images < 1 || sh.num_images > 65535 || sh.num_classes < 1 ||
        sh.num_classes > ((int64_t)1 << kNmsClsBits) || sel.nms_pre <= 0 || nms.max_per_img < 0 || nms.max_per_img > ((int64_t)1 << 30))
        return SPH2POB_ERR_SIZE;
    if (!have_tables || !sh.level_n) return SPH2POB_ERR_NULL;
    Levels L{};
    L.num = sh.num_levels;
    int64_t k_cap = 0, total = 0, chunks = 0, prior = 0;
    for (int l = 0; l < sh.num_levels; l++) {
        const int64_t n = sh.level_n[l], hw = sh.level_hw ? sh.level_hw[l] : 0, count = n * sh.num_classes;
        if (n < 1 || count >= ((int64_t)1 << 31) - 8 * kChunkElems || hw < 0 || (hw > 0 && n % hw != 0)) return SPH2POB_ERR_SIZE;
        Level& d = L.lv[l];
        d.n = (int)n; d.count = (int)count;
        d.hw = hw > 0 ? (int)hw : (int)count;
        d.ac = hw > 0 ? (int)(count / hw) : 1;
        d.sp = (int)hw; d.a = hw > 0 ? (int)(n / hw) : 1;
        d.cap = (int)(count < sel.nms_pre ? count : sel.nms_pre);
        d.prior_off = (int)prior; d.chunk_off = (int)chunks; d.buf_off = total;
        prior += n; total += count; k_cap += d.cap;
        chunks += (count + kChunkElems - 1) / kChunkElems;
        if (prior >= ((int64_t)1 << 31) || chunks >= ((int64_t)1 << 31)) return SPH2POB_ERR_SIZE;
    }
    if (k_cap > ((int64_t)1 << kNmsIdxBits)) return SPH2POB_ERR_SIZE;
    L.chunks = (int)chunks; L.k_cap = (int)k_cap; L.total = total;
    *out = L;
    return SPH2POB_OK;
}
inline int make_levels(const void* const* cls, const void* const* bbox, const void* const* anchors, const Shape& sh, const Selection& sel,
                       const Coder& cd, const Nms& nms, Levels* out) {
    if (int rc = make_level_shapes(sh, sel, cd, nms, cls && bbox && anchors && sh.level_hw, out)) return rc;
    for (int l = 0; l < sh.num_levels; l++) {
        if (!cls[l] || !bbox[l] || !anchors[l]) return SPH2POB_ERR_NULL;
        out->lv[l].cls = (const float*)cls[l]; out->lv[l].bbox = (const float*)bbox[l]; out->lv[l].anchors = (const float*)anchors[l];
    }
    return SPH2POB_OK;
}

// the deltas of anchor `ai` of image b, from the head layout, widened to fp32; T: the element type of the level tensors.  The layout
// decides the first element and the stride only; the DIM loads behind it are one sequence for both, issued together
template <int DIM, class T = float>
SPHG_DEV void gather_deltas(const Level& lv, int64_t b, int ai, float* d) {
    const T* q = reinterpret_cast<const T*>(lv.bbox);
    int64_t step = 1;
    if (lv.sp > 0) {
        const int p = ai / lv.a, a = ai - p * lv.a;
        q += (b * lv.a + a) * (int64_t)DIM * lv.sp + p;
        step = lv.sp;
    } else {
        q += (b * lv.n + ai) * (int64_t)DIM;
    }
#pragma unroll
    for (int k = 0; k < DIM; k++) d[k] = (float)q[k * step];
}

// ---- candidate sources: the rule selected key -> decoded box, reported score, prior index of one head, for cand_build_kernel
// (sph2pob_get_bboxes.hip) and for bboxes_cpu (sph2pob_host.hip) alike.  source(level, l, b, prior ai, class c, selected score, box,
// &prior index) returns the score the candidate goes into the NMS with; has(level, ai) is false for a key that is no candidate (it is
// skipped: nothing is loaded or stored for it); prologue() is what the first workgroup of an image does in
// front of the candidates (device only; nothing for most sources).  DIM and the element type T of the head tensors are compile-time

// The delta coders: anchor and deltas gathered from the head layout, decode_one()
template <int DIM, class T = float>
struct DeltaSource {
    static constexpr int kDim = DIM;
    Coder cd;
    SPHG_DEV float operator()(const Level& lv, int, int64_t b, int ai, int, float score, float (&box)[5], int* prior) const {
        float p[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, d[5];
#pragma unroll
        for (int k = 0; k < DIM; k++) p[k] = lv.anchors[(int64_t)ai * DIM + k];
        gather_deltas<DIM, T>(lv, b, ai, d);
        sph2pob_coder::decode_one<DIM, false>(p, d, cd.nm, cd.max_ratio, cd.coder_flags, cd.ctr_clamp, box, nullptr);
        *prior = lv.prior_off + ai;
        return score;
    }
    SPHG_DEV bool has(const Level&, int) const { return true; }
    __device__ __forceinline__ void prologue(const int*, int) const {}
};

// ---- score factors (FCOS heads: sph2pob_fcos_bboxes_f32) ----
// The centerness tensors of the levels, one channel per point, laid out like cls_scores: NCHW (B, A, H, W) or flat (B, n).  A table
// of its own, so that Level keeps its size for the entries without a factor
struct Factors { const void* p[kMaxLevels]; };

// the factor of point `ai` of image b, widened to fp32: element (b A + a) HW + p of the NCHW layout (ai = p A + a), b n + ai of the flat one
template <class T = float>
SPHG_DEV float gather_factor(const Level& lv, const void* factors, int64_t b, int ai) {
    const T* f = reinterpret_cast<const T*>(factors);
    if (lv.sp > 0) {
        const int p = ai / lv.a, a = ai - p * lv.a;
        return (float)f[(b * lv.a + a) * (int64_t)lv.sp + p];
    }
    return (float)f[b * lv.n + ai];
}

// the score a candidate goes into the NMS with and is reported with: one fp32 multiply.  A NaN product (a NaN centerness) becomes the
// quiet NaN with the sign bit clear, whatever sign the library's expf left it: the NMS key orders scores by their bits, and the kernel
// and its twin must order alike
SPHG_DEV float factor_score(float class_score, float factor) {
    const float s = class_score * factor;
    return s != s ? float_of(0x7fc00000u) : s;
}

// The point coder with a score factor (FCOS heads, sph2pob_fcos_bboxes_f32): Level::anchors holds the level's (n, 2) points, the
// distances are gathered like deltas, the centerness like a one-channel score; the candidate's score is the class score the key
// carries times activate(centerness), one fp32 multiply.  The centerness pointers come as a table of their own (the level table
// keeps its size for the other kernels), read with the workgroup-uniform level index
template <int DIM, class T = float>
struct PointSource {
    static constexpr int kDim = DIM;
    Factors F;
    sph2pob_point::Image im;
    int activation;
    SPHG_DEV float operator()(const Level& lv, int l, int64_t b, int ai, int, float score, float (&box)[5], int* prior) const {
        *prior = lv.prior_off + ai;
        const float2 xy = reinterpret_cast<const float2*>(lv.anchors)[ai];
        const float pt[2] = {xy.x, xy.y};
        float d[5];
        gather_deltas<DIM, T>(lv, b, ai, d);
        const float factor = activate(gather_factor<T>(lv, F.p[l], b, ai), activation);
        sph2pob_point::decode_row<DIM, false>(pt, d, nullptr, im, box);
        return factor_score(score, factor);
    }
    // flat < lv.count.  A guard only: every selected key carries an index of its level
    SPHG_DEV bool has(const Level& lv, int ai) const { return ai < lv.n; }
    __device__ __forceinline__ void prologue(const int*, int) const {}
};

// Argument checks of sph2pob_fcos_bboxes_f32 and its twin, in the documented order: the shapes as make_level_shapes has them, the
// coder's image (check_coder's rules: the size, then a NaN bound), then every level pointer.  Level::anchors holds the points
inline int make_point_levels(const void* const* cls, const void* const* bbox, const void* const* points, const void* const* factors,
                             const Shape& sh, const Selection& sel, const Nms& nms, const Frame& fr, Levels* out, Factors* fac) {
    if (int rc = make_level_shapes(sh, sel, Coder{}, nms, cls && bbox && points && factors && sh.level_hw, out)) return rc;
    if (fr.img_h < 1 || fr.img_w < 1 || fr.img_h > (1 << 24) || fr.img_w > (1 << 24)) return SPH2POB_ERR_SIZE;
    if (fr.max_h != fr.max_h || fr.max_w != fr.max_w) return SPH2POB_ERR_OPTION;
    *fac = Factors{};
    for (int l = 0; l < sh.num_levels; l++) {
        if (!cls[l] || !bbox[l] || !points[l] || !factors[l]) return SPH2POB_ERR_NULL;
        out->lv[l].cls = (const float*)cls[l]; out->lv[l].bbox = (const float*)bbox[l]; out->lv[l].anchors = (const float*)points[l];
        fac->p[l] = factors[l];
    }
    return SPH2POB_OK;
}

// The NMS stage of sph2pob_test_bboxes_f32, defined in sph2pob_nms.hip and called from sph2pob_get_bboxes.hip (inside the library
// only): B candidate blocks of stride k_cap, live counts on the device.
struct Candidates { const float* boxes; const float* scores; const int64_t* labels; const int* prior; const int* counts; int k_cap; };
__attribute__((visibility("hidden"))) int nms_batch_launch(const Candidates& cand, int64_t num_images, int box_dim, const Nms& nms,
                                                           void* nms_workspace, const Outputs& out, void* stream);
__attribute__((visibility("hidden"))) int64_t nms_batch_workspace_bytes(int64_t num_images, int k_cap, int box_dim);
// Stages 1-10 of sph2pob_test_bboxes_f32 on a checked level table whose scores are fp32 probabilities (activation 0) and whose
// deltas have the head's own element type (delta_dtype 0: fp32, else SPH2POB_DTYPE_*).  Defined in sph2pob_get_bboxes.hip and called
// from sph2pob_softmax_bboxes.hip, whose stage 0 wrote the probabilities (inside the library only)
__attribute__((visibility("hidden"))) int test_bboxes_on_probs(const Levels& L, const Shape& sh, const Selection& sel, const Coder& cd,
                                                               const Nms& nms, const Outputs& out, void* workspace, int delta_dtype,
                                                               void* stream);

}  // namespace sph2pob_gb
