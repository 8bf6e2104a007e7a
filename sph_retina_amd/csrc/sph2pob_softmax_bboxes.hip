// libsph2pob_hip.so — inference for softmax heads (sph2pob_softmax_scores_f32 / sph2pob_softmax_bboxes_f32 and their _h16 siblings,
// include/sph2pob_hip.h): the probability pass — per anchor the foreground probabilities of sph2pob_softmax::Prob, written in the
// head's own layout without the background channel — and, for the fused entry, stages 1-10 of sph2pob_test_bboxes_f32 on those
// probabilities (sph2pob_get_bboxes.hip) with the deltas read where the head left them.  Replaces `cls_score.softmax(-1)[:, :-1]`
// in front of filter_scores_and_topk (sphdet/models/heads/sph_ssd_head.py:330-347; sph_rpn_head.py:52-57 is K = 2).  gfx950 only.
//
// One launch over all levels and images.  NCHW levels: lanes run along the positions, so every class plane is read and written in
// whole lines; four consecutive positions per lane (one 16-byte access per plane, four independent rows) when H W % 4 == 0.  Flat
// levels: the kBlock rows of a workgroup are one contiguous span, staged through LDS (coalesced both ways), one row per lane on the
// staged copy.  Up to kHoldK classes a row's logits are read once and held; above it the three walks read them again (a row per
// lane is then long enough to stream on its own).  The arithmetic is Prob's everywhere.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_get_bboxes.hpp"
#include "sph2pob_softmax.hpp"

namespace {

using namespace sph2pob_softmax;
namespace GB = sph2pob_gb;

// V consecutive elements widened to fp32: one access for V = 4 (16 bytes of fp32, 8 bytes of a 16-bit type)
template <class T, int V>
__device__ __forceinline__ void load_v(const T* p, float* x) {
    if constexpr (V == 1) {
        x[0] = (float)p[0];
    } else if constexpr (std::is_same<T, float>::value) {
        const float4 v = *reinterpret_cast<const float4*>(p);
        x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
    } else {
        struct alignas(4 * sizeof(T)) Quad { T v[4]; };
        const Quad q = *reinterpret_cast<const Quad*>(p);
#pragma unroll
        for (int e = 0; e < 4; e++) x[e] = (float)q.v[e];
    }
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float* x) {
    if constexpr (V == 1) p[0] = x[0];
    else *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
}

// One NCHW item: V consecutive positions of one (b, a), V independent rows.  R > 0: the K <= R planes are loaded once, all loads
// issued before the first use (class index clamped: the loads past K repeat the last plane and are never looked at); R == 0: the
// walks read the planes again.
template <class T, int V, int R>
__device__ __forceinline__ void prob_nchw(const ProbLevel& lv, int64_t item, int K) {
    const int hw = lv.hw, per = hw / V;
    const int64_t ba = item / per, p = (item - ba * per) * V;
    int64_t in, out;
    prob_nchw_span(ba, p, hw, K, &in, &out);
    const T* x = reinterpret_cast<const T*>(lv.logits) + in;
    float* o = lv.out + out;
    Prob r[V];
#pragma unroll
    for (int e = 0; e < V; e++) r[e].begin();
    if constexpr (R > 0) {
        float h[R][V];
#pragma unroll
        for (int j = 0; j < R; j++) load_v<T, V>(x + (int64_t)(j < K ? j : K - 1) * hw, h[j]);
#pragma unroll
        for (int j = 0; j < R; j++)
            if (j < K)
#pragma unroll
                for (int e = 0; e < V; e++) r[e].see_max(h[j][e]);
#pragma unroll
        for (int j = 0; j < R; j++)
            if (j < K)
#pragma unroll
                for (int e = 0; e < V; e++) { h[j][e] = r[e].e(h[j][e]); r[e].add(h[j][e]); }   // (h keeps e_j from here on)
#pragma unroll
        for (int j = 0; j < R; j++)
            if (j < K - 1) {
                float q[V];
#pragma unroll
                for (int e = 0; e < V; e++) q[e] = r[e].of(h[j][e]);
                store_v<V>(o + (int64_t)j * hw, q);
            }
    } else {
        float h[V];
        for (int j = 0; j < K; j++) {
            load_v<T, V>(x + (int64_t)j * hw, h);
#pragma unroll
            for (int e = 0; e < V; e++) r[e].see_max(h[e]);
        }
        for (int j = 0; j < K; j++) {
            load_v<T, V>(x + (int64_t)j * hw, h);
#pragma unroll
            for (int e = 0; e < V; e++) r[e].see_sum(h[e]);
        }
        for (int j = 0; j < K - 1; j++) {
            load_v<T, V>(x + (int64_t)j * hw, h);
            float q[V];
#pragma unroll
            for (int e = 0; e < V; e++) q[e] = r[e].p(h[e]);
            store_v<V>(o + (int64_t)j * hw, q);
        }
    }
}

// The rows [row0, row0 + kBlock) of a flat level (fewer at its end), K <= kHoldK: their logits are one contiguous span — loaded
// coalesced into LDS, one row per lane there (the probabilities overwrite the row's own logits), stored coalesced.  All lanes of
// the workgroup come here together.
template <class T>
__device__ __forceinline__ void prob_flat_staged(const ProbLevel& lv, int64_t row0, int K, float* stage) {
    const int C = K - 1, t = threadIdx.x;
    const int64_t left = lv.items - row0;
    const int rows = left < kBlock ? (int)left : kBlock;
    const T* x = reinterpret_cast<const T*>(lv.logits) + row0 * K;
    for (int i = t; i < rows * K; i += kBlock) stage[i] = (float)x[i];
    __syncthreads();
    if (t < rows) {
        float* h = stage + t * K;
        Prob r;
        r.begin();
        for (int j = 0; j < K; j++) r.see_max(h[j]);
        for (int j = 0; j < K; j++) { h[j] = r.e(h[j]); r.add(h[j]); }
        for (int j = 0; j < C; j++) h[j] = r.of(h[j]);
    }
    __syncthreads();
    float* o = lv.out + row0 * C;
    for (int i = t; i < rows * C; i += kBlock) {
        const int row = i / C;
        o[i] = stage[row * K + (i - row * C)];
    }
}

// one flat row per lane, walked in memory (K > kHoldK)
template <class T>
__device__ __forceinline__ void prob_flat_row(const ProbLevel& lv, int64_t row, int K) {
    const T* x = reinterpret_cast<const T*>(lv.logits) + row * K;
    float* o = lv.out + row * (K - 1);
    Prob r;
    r.begin();
    for (int j = 0; j < K; j++) r.see_max((float)x[j]);
    for (int j = 0; j < K; j++) r.see_sum((float)x[j]);
    for (int j = 0; j < K - 1; j++) o[j] = r.p((float)x[j]);
}

// T: the element type of the logits; R: classes held per row (the smallest of 8, 24, kHoldK that is >= K), 0: K > kHoldK
template <class T, int R>
__global__ __launch_bounds__(kBlock) void softmax_prob_kernel(ProbLevels L, int K) {
    extern __shared__ float stage[];
    int l = 0;
#pragma unroll
    for (int q = 1; q < kMaxLevels; q++) l += (q < L.num && (int)blockIdx.x >= L.lv[q].block_off) ? 1 : 0;   // workgroup-uniform
    const ProbLevel& lv = L.lv[l];
    const int64_t first = (int64_t)((int)blockIdx.x - lv.block_off) * kBlock, item = first + threadIdx.x;
    if (lv.kind == PROB_FLAT) {
        if constexpr (R > 0) prob_flat_staged<T>(lv, first, K, stage);
        else if (item < lv.items) prob_flat_row<T>(lv, item, K);
    } else if (item < lv.items) {
        if (lv.kind == PROB_NCHW4) prob_nchw<T, 4, R>(lv, item, K);
        else prob_nchw<T, 1, R>(lv, item, K);
    }
}

template <class T>
int prob_launch(const ProbLevels& L, int K, hipStream_t s) {
    if (L.blocks == 0) return SPH2POB_OK;
    bool flat = false;
    for (int l = 0; l < L.num; l++) flat = flat || (L.lv[l].kind == PROB_FLAT && L.lv[l].items > 0);
    const size_t lds = flat && K <= kHoldK ? (size_t)kBlock * K * sizeof(float) : 0;   // at most 40 KiB
    const dim3 grid(L.blocks), block(kBlock);
    if (K <= 8) hipLaunchKernelGGL((softmax_prob_kernel<T, 8>), grid, block, lds, s, L, K);
    else if (K <= 24) hipLaunchKernelGGL((softmax_prob_kernel<T, 24>), grid, block, lds, s, L, K);
    else if (K <= kHoldK) hipLaunchKernelGGL((softmax_prob_kernel<T, kHoldK>), grid, block, lds, s, L, K);
    else hipLaunchKernelGGL((softmax_prob_kernel<T, 0>), grid, block, lds, s, L, K);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? SPH2POB_OK : (int)e;
}
// dtype 0: fp32 logits, else SPH2POB_DTYPE_*
int prob_launch_dtype(const ProbLevels& L, int K, int dtype, hipStream_t s) {
    return GB::with_f32_or_h16(dtype, [&](auto t) { return prob_launch<decltype(t)>(L, K, s); });
}

int softmax_scores(const void* const* logits, const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                   int64_t num_classes, void* const* out, int dtype, void* stream) {
    ProbLevels L;
    if (int rc = make_prob_levels(logits, out, level_n, level_hw, num_levels, num_images, num_classes, dtype ? 2 : 4, &L)) return rc;
    return prob_launch_dtype(L, (int)num_classes + 1, dtype, (hipStream_t)stream);
}

// the probability blocks of a fused call follow the pipeline's own workspace, each level's (B, n_l C) block 256-byte aligned: an
// image's block is as aligned as it would be in a tensor of its own, so the streaming stages keep their 16-byte loads
int64_t up256(int64_t x) { return (x + 255) / 256 * 256; }

int softmax_bboxes(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const GB::Shape& sh,
                   const GB::Selection& sel, const GB::Coder& cd, const GB::Nms& nms, const GB::Outputs& out, void* workspace, int dtype,
                   void* stream) {
    GB::Levels G;
    if (int rc = make_softmax_levels(cls_scores, bbox_preds, anchors, sh, sel, cd, nms, out, &G)) return rc;
    if (!workspace) return SPH2POB_ERR_NULL;
    const int64_t base = sph2pob_get_bboxes_workspace_bytes(sh.level_n, sh.num_levels, sh.num_images, sh.num_classes, sh.box_dim, sel.nms_pre);
    char* p = reinterpret_cast<char*>((reinterpret_cast<uintptr_t>(workspace) + (uintptr_t)base + 255) & ~(uintptr_t)255);
    void* outs[GB::kMaxLevels];
    for (int l = 0; l < sh.num_levels; l++) {
        outs[l] = p;
        p += up256(sh.num_images * sh.level_n[l] * sh.num_classes * 4);
    }
    ProbLevels L;
    if (int rc = make_prob_levels(cls_scores, outs, sh.level_n, sh.level_hw, sh.num_levels, sh.num_images, sh.num_classes, dtype ? 2 : 4, &L))
        return rc;
    if (int rc = prob_launch_dtype(L, (int)sh.num_classes + 1, dtype, (hipStream_t)stream)) return rc;
    for (int l = 0; l < sh.num_levels; l++) G.lv[l].cls = (const float*)outs[l];   // the selection runs on the probabilities
    return GB::test_bboxes_on_probs(G, sh, sel, cd, nms, out, workspace, dtype, stream);
}

bool h16(int dtype) { return dtype == SPH2POB_DTYPE_F16 || dtype == SPH2POB_DTYPE_BF16; }

}  // namespace

extern "C" {

int sph2pob_softmax_scores_f32(const void* const* logits, const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                               int64_t num_classes, void* const* out, void* stream) {
    return softmax_scores(logits, level_n, level_hw, num_levels, num_images, num_classes, out, 0, stream);
}

int sph2pob_softmax_scores_h16(const void* const* logits, const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                               int64_t num_classes, void* const* out, int dtype, void* stream) {
    if (!h16(dtype)) return SPH2POB_ERR_OPTION;
    return softmax_scores(logits, level_n, level_hw, num_levels, num_images, num_classes, out, dtype, stream);
}

int64_t sph2pob_softmax_bboxes_workspace_bytes(const int64_t* level_n, int num_levels, int64_t num_images, int64_t num_classes, int box_dim,
                                               int64_t nms_pre) {
    const int64_t base = sph2pob_get_bboxes_workspace_bytes(level_n, num_levels, num_images, num_classes, box_dim, nms_pre);
    if (base <= 0 || num_classes > kMaxK - 1) return 0;
    int64_t bytes = up256(base) + 256;
    for (int l = 0; l < num_levels; l++) bytes += up256(num_images * level_n[l] * num_classes * 4);
    return bytes;
}

// the two entries fill the parameter blocks (activation 0: the selection is on probabilities)
int sph2pob_softmax_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                               const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, float score_thr,
                               int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                               float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                               int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream) {
    return softmax_bboxes(cls_scores, bbox_preds, anchors, GB::Shape{level_n, level_hw, num_levels, num_images, num_classes, box_dim},
                          GB::Selection{0, score_thr, nms_pre}, GB::make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp),
                          GB::Nms{variant_flags, class_agnostic, iou_threshold, max_per_img}, GB::Outputs{dets, labels, prior_inds, num_dets}, workspace, 0,
                          stream);
}

int sph2pob_softmax_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                               const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, float score_thr,
                               int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                               float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                               int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream) {
    if (!h16(dtype)) return SPH2POB_ERR_OPTION;
    return softmax_bboxes(cls_scores, bbox_preds, anchors, GB::Shape{level_n, level_hw, num_levels, num_images, num_classes, box_dim},
                          GB::Selection{0, score_thr, nms_pre}, GB::make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp),
                          GB::Nms{variant_flags, class_agnostic, iou_threshold, max_per_img}, GB::Outputs{dets, labels, prior_inds, num_dets}, workspace,
                          dtype, stream);
}

}  // extern "C"
