// libsph2pob_hip.so — detection post-processing for a minibatch (sph2pob_test_bboxes_f32 / sph2pob_get_bboxes_f32, include/sph2pob_hip.h): per (image,
// level) exact top-k of the class scores above a threshold, read from the head's own layout; gather + decode of the selected
// candidates; then the batched NMS stage of sph2pob_nms.hip.  Replaces SphRetinaHead._get_bboxes_single / _bbox_post_process
// (sphdet/models/heads/sph_retina_head.py:101-216, :22-99) and filter_scores_and_topk (mmdet/core/utils/misc.py:119-165) for
// B images with a number of launches that does not depend on B, and without a host read.  gfx950 only.  sph2pob_fcos_bboxes_f32 is
// the same pipeline for SphFCOSHead (sph_fcos_head.py:246-323, :205-244): the selection on the class scores alone, then a cand_build
// of its own that decodes from points and multiplies the class score by the point's centerness.  sph2pob_rcnn_bboxes_f32
// (sph2pob_rcnn_bboxes.hip) is the pipeline once more, for the R-CNN stage: one flat level of the probabilities its stage 0 wrote,
// and cand_build_rois_kernel, whose priors are the images' own rois and whose deltas are per class.
//
// Selection, per (image, level), on the unique 64-bit keys (descending score bits << 32 | flat index):
//   zero          the histograms and the per-(image, level) records
//   topk_hist     stream 1: scores above the threshold -> a histogram of score_bin() (LDS per workgroup, integer atomics into the
//                 level's global histogram: the totals do not depend on the order of arrival)
//   topk_cut      the bin in which the nms_pre-th key falls, how many keys are wanted and how many lie in the bins up to it
//   topk_compact  stream 2: every key in those bins -> the level's survivor buffer, ballot + mbcnt compaction (the SET of
//                 survivors is fixed by the histogram, their order in the buffer is not and is never used)
//   topk_resolve  radix select among the survivors -> the exact nms_pre-th key; the keys up to it -> the level's selection
//   cand_build    rank of every selected key among the level's selection (the final order), anchor and deltas gathered from the
//                 head layout, decode_one(), box / score / label / prior index written at its place of the image's candidate block
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_coder.hpp"
#include "sph2pob_get_bboxes.hpp"   // (declares the NMS stage, sph2pob_nms_batch_launch)
#include "sph2pob_point_targets.hpp"   // (the point coder's decode_row)
#include "sph2pob_rcnn_bboxes.hpp"     // (the rois of the R-CNN stage and their candidate_box)

namespace {

using namespace sph2pob_gb;
namespace C = sph2pob_coder;
namespace PT = sph2pob_point;
namespace RB = sph2pob_rcnn_bb;

constexpr int kSelBlock = 256, kSelIters = 16, kChunk = kSelBlock * 4 * kSelIters;   // 16 384 scores per workgroup
constexpr int kResBlock = 1024, kRadixBits = 11, kRadix = 1 << kRadixBits;

struct Meta { int cut, want, through, slots; };   // per (image, level); slots: the compaction's arrival counter

__device__ __forceinline__ int rank_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}

// the level of a streaming chunk (workgroup-uniform; at most kMaxLevels entries)
__device__ __forceinline__ int level_of_chunk(const Levels& L, int chunk) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < kMaxLevels; q++) l += (q < L.num && chunk >= L.lv[q].chunk_off) ? 1 : 0;
    return l;
}

// Streams one chunk of one image's level in memory order, four consecutive scores per lane and step (one 16-byte load when the
// image's base is aligned), and hands every score above the threshold to f(descending key, flat index, valid): f is called by
// all lanes of a wave together, four times per step.  T: the element type of the scores — float, or a 16-bit type of the _h16
// entries: then the four scores are one 8-byte load, widened to fp32 here; everything after the load is fp32 either way.
template <class T, class F>
__device__ __forceinline__ void stream_chunk(const Level& lv, int64_t b, int chunk, int activation, float thr, F&& f) {
    const T* base = reinterpret_cast<const T*>(lv.cls) + b * (int64_t)lv.count;
    const bool vec = (lv.count & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & (4 * sizeof(T) - 1)) == 0;
    const int m_begin = chunk * kChunk;
    for (int it = 0; it < kSelIters; it++) {
        const int m0 = m_begin + (it * kSelBlock + (int)threadIdx.x) * 4;
        if (m_begin + it * kSelBlock * 4 >= lv.count) break;   // workgroup-uniform
        float x[4];
        if (vec && m0 + 3 < lv.count) {
            if constexpr (std::is_same<T, float>::value) {
                const float4 v = *reinterpret_cast<const float4*>(base + m0);
                x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w;
            } else {
                struct alignas(4 * sizeof(T)) Quad { T v[4]; };
                const Quad q = *reinterpret_cast<const Quad*>(base + m0);
#pragma unroll
                for (int e = 0; e < 4; e++) x[e] = (float)q.v[e];
            }
        } else {
#pragma unroll
            for (int e = 0; e < 4; e++) x[e] = m0 + e < lv.count ? (float)base[m0 + e] : 0.0f;
        }
        const int mc = m0 < lv.count ? m0 : 0;
        int ch = mc / lv.hw, p = mc - ch * lv.hw;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            const float s = activate(x[e], activation);
            const bool valid = m0 + e < lv.count && s > thr;   // NaN is dropped
            f(desc_score_bits(s), (unsigned)(p * lv.ac + ch), valid);
            if (++p == lv.hw) { p = 0; ch++; }
        }
    }
}

// Launch 1: the histograms and the per-(image, level) records start every call at zero.  A kernel on the call's stream, not a memset
// node: a captured call is then kernels only (a graph of this pipeline faulted on its second replay while launch 1
// was hipMemsetAsync).  V: int4 — 16-byte stores, the zeroed prefix is a multiple of 256 bytes — or int for a workspace whose base
// is not 16-byte aligned
constexpr int kZeroBlock = 256, kZeroGridMax = 1024;
template <class V>
__global__ __launch_bounds__(kZeroBlock) void zero_kernel(V* __restrict__ p, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * kZeroBlock + threadIdx.x; i < n; i += (int64_t)gridDim.x * kZeroBlock) p[i] = V{};
}
template <class V>
void launch_zero(void* p, int64_t bytes, hipStream_t s) {
    const int64_t n = bytes / (int64_t)sizeof(V), blocks = (n + kZeroBlock - 1) / kZeroBlock;
    hipLaunchKernelGGL(zero_kernel<V>, dim3((unsigned)(blocks < kZeroGridMax ? blocks : kZeroGridMax)), dim3(kZeroBlock), 0, s, (V*)p, n);
}

template <class T>
__global__ __launch_bounds__(kSelBlock) void topk_hist_kernel(Levels L, int activation, float thr, int* __restrict__ hist) {
    __shared__ int h[kBins];
    const int b = blockIdx.y, l = level_of_chunk(L, blockIdx.x);
    const Level& lv = L.lv[l];
    for (int i = threadIdx.x; i < kBins; i += kSelBlock) h[i] = 0;
    __syncthreads();
    int any = 0;
    stream_chunk<T>(lv, b, blockIdx.x - lv.chunk_off, activation, thr, [&](unsigned dkey, unsigned, bool valid) {
        if (valid) { atomicAdd(&h[score_bin(dkey)], 1); any = 1; }
    });
    if (!__syncthreads_or(any)) return;   // (a detector's scores are mostly below the threshold: most chunks stop here)
    int* g = hist + ((int64_t)b * L.num + l) * kBins;
    for (int i = threadIdx.x; i < kBins; i += kSelBlock)
        if (h[i]) atomicAdd(&g[i], h[i]);
}

// one workgroup per (image, level): the first bin at which the running count reaches nms_pre
__global__ __launch_bounds__(kResBlock) void topk_cut_kernel(Levels L, int nms_pre, const int* __restrict__ hist, Meta* __restrict__ meta) {
    __shared__ int part[kResBlock];
    const int l = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const int* g = hist + ((int64_t)b * L.num + l) * kBins;
    constexpr int per = kBins / kResBlock;
    int v[per], sum = 0;
#pragma unroll
    for (int q = 0; q < per; q++) { v[q] = g[t * per + q]; sum += v[q]; }
    part[t] = sum;
    __syncthreads();
    for (int o = 1; o < kResBlock; o <<= 1) {   // inclusive scan
        const int add = t >= o ? part[t - o] : 0;
        __syncthreads();
        part[t] += add;
        __syncthreads();
    }
    const int total = part[kResBlock - 1], want = total < nms_pre ? total : nms_pre;
    int run = part[t] - sum;   // keys in the bins in front of this thread's
    Meta* m = meta + (int64_t)b * L.num + l;
    if (want == 0) {
        if (t == 0) *m = Meta{-1, 0, 0, 0};
        return;
    }
#pragma unroll
    for (int q = 0; q < per; q++) {
        if (run < want && run + v[q] >= want) *m = Meta{t * per + q, want, run + v[q], 0};   // exactly one thread and bin
        run += v[q];
    }
}

template <class T>
__global__ __launch_bounds__(kSelBlock) void topk_compact_kernel(Levels L, int activation, float thr, Meta* __restrict__ meta,
                                                                unsigned long long* __restrict__ buf) {
    const int b = blockIdx.y, l = level_of_chunk(L, blockIdx.x);
    const Level& lv = L.lv[l];
    Meta* m = meta + (int64_t)b * L.num + l;
    const int cut = m->cut;
    if (cut < 0) return;
    unsigned long long* out = buf + b * L.total + lv.buf_off;
    stream_chunk<T>(lv, b, blockIdx.x - lv.chunk_off, activation, thr, [&](unsigned dkey, unsigned flat, bool valid) {
        const bool take = valid && score_bin(dkey) <= cut;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(take);
        if (mask == 0ull) return;   // wave-uniform
        int slot = 0;
        if (rank_below(mask) == 0 && take) slot = atomicAdd(&m->slots, __popcll(mask));   // the first taking lane reserves for the wave
        slot = __builtin_amdgcn_readlane(slot, __builtin_ctzll(mask));
        // the histogram counted exactly these keys: slot + rank < through <= count, the level's share of the buffer
        if (take) out[slot + rank_below(mask)] = ((unsigned long long)dkey << 32) | flat;
    });
}

// One workgroup per (image, level): the want-th smallest of `through` unique keys by a most-significant-digit radix select
// (six digits of 11 bits over the survivors; nothing to do when every survivor is wanted), then the keys up to it.
__global__ __launch_bounds__(kResBlock) void topk_resolve_kernel(Levels L, const Meta* __restrict__ meta, const unsigned long long* __restrict__ buf,
                                                                unsigned long long* __restrict__ sel) {
    __shared__ int h[kRadix];
    __shared__ int pick[2];
    const int l = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const Meta m = meta[(int64_t)b * L.num + l];
    if (m.want <= 0) return;
    const unsigned long long* in = buf + b * L.total + L.lv[l].buf_off;
    unsigned long long prefix = 0ull, decided = 0ull, last = ~0ull;   // keys with (key & decided) == prefix are still in the race
    if (m.through > m.want) {
        int remaining = m.want;   // rank (1-based) of the wanted key among the keys in the race
        for (int shift = 64 - kRadixBits; ; shift -= kRadixBits) {
            const int sh = shift < 0 ? 0 : shift;
            const int bits = shift < 0 ? kRadixBits + shift : kRadixBits;
            for (int i = t; i < kRadix; i += kResBlock) h[i] = 0;
            __syncthreads();
            for (int i = t; i < m.through; i += kResBlock) {
                const unsigned long long k = in[i];
                if ((k & decided) == prefix) atomicAdd(&h[(int)((k >> sh) & ((1u << bits) - 1u))], 1);
            }
            __syncthreads();
            if (t < 64) {   // wave 0: 32 digits per lane, a wave scan, then the lane that holds the crossing walks its digits
                int s = 0;
                for (int q = 0; q < kRadix / 64; q++) s += h[t * (kRadix / 64) + q];
                int inc = s;
                for (int o = 1; o < 64; o <<= 1) { const int v = __shfl_up(inc, o, 64); if (t >= o) inc += v; }
                const int before = inc - s;
                if (before < remaining && inc >= remaining) {
                    int run = before;
                    for (int q = 0; q < kRadix / 64; q++) {
                        const int c = h[t * (kRadix / 64) + q];
                        if (run < remaining && run + c >= remaining) { pick[0] = t * (kRadix / 64) + q; pick[1] = remaining - run; }
                        run += c;
                    }
                }
            }
            __syncthreads();
            prefix |= (unsigned long long)pick[0] << sh;
            decided |= (unsigned long long)((1u << bits) - 1u) << sh;
            remaining = pick[1];
            __syncthreads();
            if (sh == 0) break;
        }
        last = prefix;   // the want-th smallest key itself
    }
    // keys <= last -> the selection, compacted per wave through an LDS counter (their order is set by cand_build's ranks)
    unsigned long long* out = sel + ((int64_t)b * L.k_cap) + [&] { int o = 0; for (int q = 0; q < l; q++) o += L.lv[q].cap; return o; }();
    if (t == 0) pick[0] = 0;
    __syncthreads();
    for (int i0 = 0; i0 < m.through; i0 += kResBlock) {   // workgroup-uniform trip count: the ballots see whole waves
        const int i = i0 + t;
        const unsigned long long k = i < m.through ? in[i] : ~0ull;
        const bool take = i < m.through && k <= last;
        const unsigned long long mask = __builtin_amdgcn_ballot_w64(take);
        if (mask == 0ull) continue;
        int slot = 0;
        if (rank_below(mask) == 0 && take) slot = atomicAdd(&pick[0], __popcll(mask));
        slot = __builtin_amdgcn_readlane(slot, __builtin_ctzll(mask));
        const int at = slot + rank_below(mask);
        if (take && at < m.want) out[at] = k;   // (exactly `want` unique keys are <= last: the bound is a guard only)
    }
}

// One lane per selected key: its rank among the level's selection (tiles of the selection in LDS).  The part of cand_build the coders
// share: false for a lane (or a whole workgroup) without a key; else `mine` is the lane's key and `at` its row of the candidate block
constexpr int kBuildBlock = 256;
__device__ __forceinline__ bool cand_place(const Levels& L, const Meta* __restrict__ meta, const unsigned long long* __restrict__ sel,
                                           int* __restrict__ counts, unsigned long long (&tile)[kBuildBlock], unsigned long long& mine, int64_t& at) {
    const int l = blockIdx.y, b = blockIdx.z, t = threadIdx.x;
    const Meta* mb = meta + (int64_t)b * L.num;
    int off = 0, cap_off = 0, all = 0;
    for (int q = 0; q < L.num; q++) {
        const int w = mb[q].want;
        if (q < l) { off += w; cap_off += L.lv[q].cap; }
        all += w;
    }
    if (blockIdx.x == 0 && l == 0 && t == 0) counts[b] = all;
    const int want = mb[l].want;
    if ((int)blockIdx.x * kBuildBlock >= want) return false;   // workgroup-uniform
    const unsigned long long* in = sel + (int64_t)b * L.k_cap + cap_off;
    const int i = blockIdx.x * kBuildBlock + t;
    mine = i < want ? in[i] : ~0ull;
    int rank = 0;
    for (int j0 = 0; j0 < want; j0 += kBuildBlock) {
        __syncthreads();
        tile[t] = j0 + t < want ? in[j0 + t] : ~0ull;
        __syncthreads();
#pragma unroll 8
        for (int j = 0; j < kBuildBlock; j++) rank += tile[j] < mine ? 1 : 0;
    }
    at = (int64_t)b * L.k_cap + off + rank;
    return i < want;
}

// the delta coders: anchor and deltas gathered from the head layout, decode_one()
template <int DIM, class T>
__global__ __launch_bounds__(kBuildBlock) void cand_build_kernel(Levels L, const Meta* __restrict__ meta, const unsigned long long* __restrict__ sel,
                                                               int num_classes, C::Norm nm, float max_ratio, int coder_flags, float ctr_clamp,
                                                               float* __restrict__ boxes, float* __restrict__ scores, int64_t* __restrict__ labels,
                                                               int* __restrict__ prior, int* __restrict__ counts) {
    __shared__ unsigned long long tile[kBuildBlock];
    unsigned long long mine;
    int64_t at;
    if (!cand_place(L, meta, sel, counts, tile, mine, at)) return;
    const int l = blockIdx.y, b = blockIdx.z;
    const Level& lv = L.lv[l];
    const unsigned flat = (unsigned)mine;
    const int ai = (int)(flat / (unsigned)num_classes), c = (int)(flat - (unsigned)ai * (unsigned)num_classes);
    float p[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, d[5], box[5];
#pragma unroll
    for (int k = 0; k < DIM; k++) p[k] = lv.anchors[(int64_t)ai * DIM + k];
    gather_deltas<DIM, T>(lv, b, ai, d);
    C::decode_one<DIM, false>(p, d, nm, max_ratio, coder_flags, ctr_clamp, box, nullptr);
#pragma unroll
    for (int k = 0; k < DIM; k++) boxes[at * DIM + k] = box[k];
    scores[at] = score_of_desc_bits((unsigned)(mine >> 32));
    labels[at] = c;
    prior[at] = lv.prior_off + ai;
}

// The point coder with a score factor (FCOS heads, sph2pob_fcos_bboxes_f32): Level::anchors holds the level's (n, 2) points, the
// distances are gathered like deltas, the centerness like a one-channel score; the candidate's score is the class score the key
// carries times activate(centerness), one fp32 multiply.  The centerness pointers come as a table of their own (the level table
// keeps its size for the other kernels), read with the workgroup-uniform level index
template <int DIM, class T>
__global__ __launch_bounds__(kBuildBlock) void cand_build_points_kernel(Levels L, Factors F, const Meta* __restrict__ meta,
                                                                      const unsigned long long* __restrict__ sel, int num_classes, int activation,
                                                                      PT::Image im, float* __restrict__ boxes, float* __restrict__ scores,
                                                                      int64_t* __restrict__ labels, int* __restrict__ prior, int* __restrict__ counts) {
    __shared__ unsigned long long tile[kBuildBlock];
    unsigned long long mine;
    int64_t at;
    if (!cand_place(L, meta, sel, counts, tile, mine, at)) return;
    const int l = blockIdx.y, b = blockIdx.z;
    const Level& lv = L.lv[l];
    const unsigned flat = (unsigned)mine;
    const int ai = (int)(flat / (unsigned)num_classes), c = (int)(flat - (unsigned)ai * (unsigned)num_classes);
    if (flat >= (unsigned)lv.count) return;   // a guard only: every selected key carries an index of its level
    const float2 xy = reinterpret_cast<const float2*>(lv.anchors)[ai];
    const float pt[2] = {xy.x, xy.y};
    float d[5], box[5];
    gather_deltas<DIM, T>(lv, b, ai, d);
    const float factor = activate(gather_factor<T>(lv, F.p[l], b, ai), activation);
    PT::decode_row<DIM, false>(pt, d, nullptr, im, box);
#pragma unroll
    for (int k = 0; k < DIM; k++) boxes[at * DIM + k] = box[k];
    scores[at] = factor_score(score_of_desc_bits((unsigned)(mine >> 32)), factor);
    labels[at] = c;
    prior[at] = lv.prior_off + ai;
}

// The R-CNN stage (sph2pob_rcnn_bboxes_f32): one flat level whose priors are the images' own rois, (B, M, row_stride), with the
// head's per-class deltas (B, M, C DIM) — or class-agnostic ones, or none.  Key index r C + c -> roi row r, class c; the roi is one
// 16-byte load where the row's address allows it (row_stride is arbitrary, so that is decided per row), the deltas of class c
// are gathered from the row's own C DIM, the box is RB::candidate_box's.  The first workgroup of an image also adds up the image's
// selection histogram — every valid candidate was counted there exactly once, whatever the cut — into num_valid
template <int DIM>
__global__ __launch_bounds__(kBuildBlock) void cand_build_rois_kernel(Levels L, RB::Rois R, const Meta* __restrict__ meta,
                                                                    const unsigned long long* __restrict__ sel, const int* __restrict__ hist,
                                                                    int num_classes, C::Norm nm, float max_ratio, int coder_flags, float ctr_clamp,
                                                                    float* __restrict__ boxes, float* __restrict__ scores,
                                                                    int64_t* __restrict__ labels, int* __restrict__ prior, int* __restrict__ counts,
                                                                    int64_t* __restrict__ num_valid) {
    __shared__ unsigned long long tile[kBuildBlock];
    __shared__ int valid_sum;
    const int b = blockIdx.z;
    if (blockIdx.x == 0) {   // workgroup-uniform
        const int* g = hist + (int64_t)b * kBins;
        int s = 0;
        for (int i = threadIdx.x; i < kBins; i += kBuildBlock) s += g[i];
        if (threadIdx.x == 0) valid_sum = 0;
        __syncthreads();
        if (s) atomicAdd(&valid_sum, s);
        __syncthreads();
        if (threadIdx.x == 0) num_valid[b] = valid_sum;
    }
    unsigned long long mine;
    int64_t at;
    if (!cand_place(L, meta, sel, counts, tile, mine, at)) return;
    const unsigned flat = (unsigned)mine;
    if (flat >= (unsigned)L.lv[0].count) return;   // a guard only: every selected key carries an index of the level
    const int r = (int)(flat / (unsigned)num_classes), c = (int)(flat - (unsigned)r * (unsigned)num_classes);
    const float* row = R.rois + ((int64_t)b * R.m + r) * R.row_stride;
    float p[5], box[5];
    if ((reinterpret_cast<uintptr_t>(row) & 15) == 0) {
        const float4 v = *reinterpret_cast<const float4*>(row);
        p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; k++) p[k] = row[k];
    }
    if constexpr (DIM == 5) p[4] = row[4];
    RB::candidate_box<DIM>(R, p, b, r, c, nm, max_ratio, coder_flags, ctr_clamp, box);
#pragma unroll
    for (int k = 0; k < DIM; k++) boxes[at * DIM + k] = box[k];
    scores[at] = score_of_desc_bits((unsigned)(mine >> 32));
    labels[at] = c;
    prior[at] = r;
}

// workspace: histograms | meta (these two are zeroed by every call) | survivors | selection | candidate block | counts | NMS stage
struct Ws { int* hist; Meta* meta; unsigned long long* buf; unsigned long long* sel; float* boxes; float* scores; int64_t* labels; int* prior;
            int* counts; void* nms; int64_t zero_bytes, bytes; };
Ws make_ws(void* workspace, const Levels& L, int64_t B, int box_dim) {
    auto up = [](int64_t x) { return (x + 255) / 256 * 256; };
    Ws w;
    char* p = (char*)workspace;
    int64_t off = 0;
    w.hist = (int*)(p + off); off += up(B * L.num * kBins * 4);
    w.meta = (Meta*)(p + off); off += up(B * L.num * (int64_t)sizeof(Meta));
    w.zero_bytes = off;
    w.buf = (unsigned long long*)(p + off); off += up(B * L.total * 8);
    w.sel = (unsigned long long*)(p + off); off += up(B * L.k_cap * 8);
    w.boxes = (float*)(p + off); off += up(B * L.k_cap * box_dim * 4);
    w.scores = (float*)(p + off); off += up(B * L.k_cap * 4);
    w.labels = (int64_t*)(p + off); off += up(B * L.k_cap * 8);
    w.prior = (int*)(p + off); off += up(B * L.k_cap * 4);
    w.counts = (int*)(p + off); off += up(B * 4);
    w.nms = (void*)(p + off); off += sph2pob_nms_batch_workspace_bytes(B, L.k_cap, box_dim);
    w.bytes = off;
    return w;
}

// TS: the element type of cls_scores, TD: of bbox_preds (anchors and every output are fp32 / int64 whatever they are).  The public
// entries read both as one type; the softmax entries select on fp32 probabilities and gather the head's own deltas
// The ten launches on a checked level table: the selection on the class scores, `build(w, grid, s)` — the launch of the coder's
// cand_build — and the NMS stage
template <class TS, class Build>
int pipeline(const Levels& L, int64_t num_images, int box_dim, int activation, float score_thr, int64_t nms_pre, int variant_flags,
             int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets,
             void* workspace, void* stream, Build&& build) {
    if (!num_dets || !workspace || (max_per_img > 0 && (!dets || !labels || !prior_inds))) return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const int B = (int)num_images;
    const Ws w = make_ws(workspace, L, B, box_dim);
    const int pre = (int)(nms_pre < ((int64_t)1 << 30) ? nms_pre : ((int64_t)1 << 30));
    if ((reinterpret_cast<uintptr_t>(w.hist) & 15) == 0) launch_zero<int4>(w.hist, w.zero_bytes, s);
    else launch_zero<int>(w.hist, w.zero_bytes, s);
    hipLaunchKernelGGL(topk_hist_kernel<TS>, dim3(L.chunks, B), dim3(kSelBlock), 0, s, L, activation, score_thr, w.hist);
    hipLaunchKernelGGL(topk_cut_kernel, dim3(L.num, B), dim3(kResBlock), 0, s, L, pre, (const int*)w.hist, w.meta);
    hipLaunchKernelGGL(topk_compact_kernel<TS>, dim3(L.chunks, B), dim3(kSelBlock), 0, s, L, activation, score_thr, w.meta, w.buf);
    hipLaunchKernelGGL(topk_resolve_kernel, dim3(L.num, B), dim3(kResBlock), 0, s, L, (const Meta*)w.meta, (const unsigned long long*)w.buf, w.sel);
    int max_cap = 0;
    for (int l = 0; l < L.num; l++) max_cap = L.lv[l].cap > max_cap ? L.lv[l].cap : max_cap;
    build(w, dim3((max_cap + kBuildBlock - 1) / kBuildBlock, L.num, B), s);
    if (int rc = launch_status()) return rc;
    return sph2pob_nms_batch_launch(w.boxes, w.scores, w.labels, w.prior, w.counts, B, L.k_cap, box_dim, variant_flags, class_agnostic, iou_threshold,
                                    max_per_img, w.nms, dets, labels, prior_inds, num_dets, s);
}

template <class TS, class TD = TS>
int test_bboxes(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                int coder_flags, float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img,
                float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream) {
    Levels L;
    if (int rc = make_levels(cls_scores, bbox_preds, anchors, level_n, level_hw, num_levels, num_images, num_classes, box_dim, activation,
                             variant_flags, class_agnostic, nms_pre, max_per_img, max_ratio, coder_flags, kChunk, &L))
        return rc;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    return pipeline<TS>(L, num_images, box_dim, activation, score_thr, nms_pre, variant_flags, class_agnostic, iou_threshold, max_per_img, dets, labels,
                        prior_inds, num_dets, workspace, stream, [&](const Ws& w, dim3 bgrid, hipStream_t s) {
        if (box_dim == 4)
            hipLaunchKernelGGL((cand_build_kernel<4, TD>), bgrid, dim3(kBuildBlock), 0, s, L, (const Meta*)w.meta, (const unsigned long long*)w.sel,
                               (int)num_classes, nm, max_ratio, coder_flags, ctr_clamp, w.boxes, w.scores, w.labels, w.prior, w.counts);
        else
            hipLaunchKernelGGL((cand_build_kernel<5, TD>), bgrid, dim3(kBuildBlock), 0, s, L, (const Meta*)w.meta, (const unsigned long long*)w.sel,
                               (int)num_classes, nm, max_ratio, coder_flags, ctr_clamp, w.boxes, w.scores, w.labels, w.prior, w.counts);
    });
}

// T: the element type of cls_scores, bbox_preds and centernesses (points and every output are fp32 / int64)
template <class T>
int fcos_bboxes(const void* const* cls_scores, const void* const* bbox_preds, const void* const* points, const void* const* centernesses,
                const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                float score_thr, int64_t nms_pre, int64_t img_h, int64_t img_w, float max_h, float max_w, int variant_flags, int class_agnostic,
                float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace,
                void* stream) {
    Levels L;
    Factors F;
    if (int rc = make_point_levels(cls_scores, bbox_preds, points, centernesses, level_n, level_hw, num_levels, num_images, num_classes, box_dim,
                                   activation, variant_flags, class_agnostic, nms_pre, max_per_img, img_h, img_w, max_h, max_w, kChunk, &L, &F))
        return rc;
    const PT::Image im{(float)img_w, (float)img_h, max_w, max_h};
    return pipeline<T>(L, num_images, box_dim, activation, score_thr, nms_pre, variant_flags, class_agnostic, iou_threshold, max_per_img, dets, labels,
                       prior_inds, num_dets, workspace, stream, [&](const Ws& w, dim3 bgrid, hipStream_t s) {
        if (box_dim == 4)
            hipLaunchKernelGGL((cand_build_points_kernel<4, T>), bgrid, dim3(kBuildBlock), 0, s, L, F, (const Meta*)w.meta,
                               (const unsigned long long*)w.sel, (int)num_classes, activation, im, w.boxes, w.scores, w.labels, w.prior, w.counts);
        else
            hipLaunchKernelGGL((cand_build_points_kernel<5, T>), bgrid, dim3(kBuildBlock), 0, s, L, F, (const Meta*)w.meta,
                               (const unsigned long long*)w.sel, (int)num_classes, activation, im, w.boxes, w.scores, w.labels, w.prior, w.counts);
    });
}

}  // namespace

extern "C" {

int64_t sph2pob_get_bboxes_workspace_bytes(const int64_t* level_n, int num_levels, int64_t num_images, int64_t num_classes, int box_dim,
                                           int64_t nms_pre) {
    Levels L;
    if (make_level_shapes(level_n, nullptr, num_levels, num_images, num_classes, box_dim, 0, SPH2POB_VARIANT_EFFICIENT, 0, nms_pre, 0, 0.0f, 0,
                          kChunk, true, &L))
        return 0;
    return make_ws(nullptr, L, num_images, box_dim).bytes;
}

int sph2pob_test_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                            const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                            float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                            int coder_flags, float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img,
                            float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream) {
    return test_bboxes<float>(cls_scores, bbox_preds, anchors, level_n, level_hw, num_levels, num_images, num_classes, box_dim, activation, score_thr,
                              nms_pre, means_host, stds_host, max_ratio, coder_flags, ctr_clamp, variant_flags, class_agnostic, iou_threshold,
                              max_per_img, dets, labels, prior_inds, num_dets, workspace, stream);
}

int sph2pob_test_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                            const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                            float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                            int coder_flags, float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img,
                            float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream) {
    if (dtype != SPH2POB_DTYPE_F16 && dtype != SPH2POB_DTYPE_BF16) return SPH2POB_ERR_OPTION;
    auto run = [&](auto t) {
        return test_bboxes<decltype(t)>(cls_scores, bbox_preds, anchors, level_n, level_hw, num_levels, num_images, num_classes, box_dim, activation,
                                        score_thr, nms_pre, means_host, stds_host, max_ratio, coder_flags, ctr_clamp, variant_flags, class_agnostic,
                                        iou_threshold, max_per_img, dets, labels, prior_inds, num_dets, workspace, stream);
    };
    return dtype == SPH2POB_DTYPE_F16 ? run(_Float16{}) : run(__bf16{});
}

// Stages 1-10 on fp32 probabilities with the deltas of the head's own type (delta_dtype 0: fp32, else SPH2POB_DTYPE_*): the pipeline
// behind sph2pob_softmax_bboxes_f32 / _h16 (sph2pob_softmax_bboxes.hip), whose stage 0 wrote `probs`.  Inside the library only
int sph2pob_test_bboxes_on_probs(const void* const* probs, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                                 const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, float score_thr,
                                 int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                                 float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                                 int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, int delta_dtype, void* stream) {
    auto run = [&](auto t) {
        return test_bboxes<float, decltype(t)>(probs, bbox_preds, anchors, level_n, level_hw, num_levels, num_images, num_classes, box_dim, 0,
                                               score_thr, nms_pre, means_host, stds_host, max_ratio, coder_flags, ctr_clamp, variant_flags,
                                               class_agnostic, iou_threshold, max_per_img, dets, labels, prior_inds, num_dets, workspace, stream);
    };
    return delta_dtype == 0 ? run(float{}) : delta_dtype == SPH2POB_DTYPE_F16 ? run(_Float16{}) : run(__bf16{});
}

// Stages 1-10 of sph2pob_rcnn_bboxes_f32 (sph2pob_rcnn_bboxes.hip, whose stage 0 wrote `probs` and which checked the arguments): the
// selection on one flat level of M rows, cand_build_rois_kernel, the NMS stage.  Inside the library only
int sph2pob_rois_bboxes_on_probs(const float* probs, const RB::Rois* rois, int64_t num_images, int64_t num_classes, int box_dim, float score_thr,
                                 int64_t max_candidates, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                                 float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                                 int64_t* labels, int64_t* prior_inds, int64_t* num_dets, int64_t* num_valid, void* workspace, void* stream) {
    Levels L;
    const RB::Rois R = *rois;
    if (int rc = RB::make_roi_level(num_images, R.m, R.row_stride, num_classes + 1, box_dim, 1 - R.per_class, variant_flags, class_agnostic,
                                    max_candidates, max_per_img, max_ratio, coder_flags, &L))
        return rc;
    if (!probs || !num_valid) return SPH2POB_ERR_NULL;
    L.lv[0].cls = probs;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    return pipeline<float>(L, num_images, box_dim, 0, score_thr, max_candidates, variant_flags, class_agnostic, iou_threshold, max_per_img, dets, labels,
                           prior_inds, num_dets, workspace, stream, [&](const Ws& w, dim3 bgrid, hipStream_t s) {
        if (box_dim == 4)
            hipLaunchKernelGGL((cand_build_rois_kernel<4>), bgrid, dim3(kBuildBlock), 0, s, L, R, (const Meta*)w.meta, (const unsigned long long*)w.sel,
                               (const int*)w.hist, (int)num_classes, nm, max_ratio, coder_flags, ctr_clamp, w.boxes, w.scores, w.labels, w.prior,
                               w.counts, num_valid);
        else
            hipLaunchKernelGGL((cand_build_rois_kernel<5>), bgrid, dim3(kBuildBlock), 0, s, L, R, (const Meta*)w.meta, (const unsigned long long*)w.sel,
                               (const int*)w.hist, (int)num_classes, nm, max_ratio, coder_flags, ctr_clamp, w.boxes, w.scores, w.labels, w.prior,
                               w.counts, num_valid);
    });
}

// the closed-form calculators, per class: its own variant check (after the box_dim check, as documented), then the entry above
int sph2pob_get_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                           const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                           float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                           int coder_flags, float ctr_clamp, int variant, float iou_threshold, int64_t max_per_img, float* dets,
                           int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream) {
    if ((box_dim == 4 || box_dim == 5) && !closed_form_variant(variant)) return SPH2POB_ERR_OPTION;
    return sph2pob_test_bboxes_f32(cls_scores, bbox_preds, anchors, level_n, level_hw, num_levels, num_images, num_classes, box_dim, activation,
                                   score_thr, nms_pre, means_host, stds_host, max_ratio, coder_flags, ctr_clamp, variant, 0, iou_threshold,
                                   max_per_img, dets, labels, prior_inds, num_dets, workspace, stream);
}

int sph2pob_get_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                           const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                           float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                           int coder_flags, float ctr_clamp, int variant, float iou_threshold, int64_t max_per_img, float* dets,
                           int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream) {
    if (dtype != SPH2POB_DTYPE_F16 && dtype != SPH2POB_DTYPE_BF16) return SPH2POB_ERR_OPTION;
    if ((box_dim == 4 || box_dim == 5) && !closed_form_variant(variant)) return SPH2POB_ERR_OPTION;
    return sph2pob_test_bboxes_h16(cls_scores, bbox_preds, anchors, level_n, level_hw, num_levels, num_images, num_classes, box_dim, activation,
                                   score_thr, nms_pre, means_host, stds_host, max_ratio, coder_flags, ctr_clamp, variant, 0, iou_threshold,
                                   max_per_img, dets, labels, prior_inds, num_dets, workspace, dtype, stream);
}

// FCOS heads: the selection on the class scores alone, the point coder, score = class score * centerness
int sph2pob_fcos_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* points, const void* const* centernesses,
                            const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim,
                            int activation, float score_thr, int64_t nms_pre, int64_t img_h, int64_t img_w, float max_h, float max_w,
                            int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels,
                            int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream) {
    return fcos_bboxes<float>(cls_scores, bbox_preds, points, centernesses, level_n, level_hw, num_levels, num_images, num_classes, box_dim, activation,
                              score_thr, nms_pre, img_h, img_w, max_h, max_w, variant_flags, class_agnostic, iou_threshold, max_per_img, dets, labels,
                              prior_inds, num_dets, workspace, stream);
}

int sph2pob_fcos_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* points, const void* const* centernesses,
                            const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim,
                            int activation, float score_thr, int64_t nms_pre, int64_t img_h, int64_t img_w, float max_h, float max_w,
                            int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels,
                            int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream) {
    if (dtype != SPH2POB_DTYPE_F16 && dtype != SPH2POB_DTYPE_BF16) return SPH2POB_ERR_OPTION;
    auto run = [&](auto t) {
        return fcos_bboxes<decltype(t)>(cls_scores, bbox_preds, points, centernesses, level_n, level_hw, num_levels, num_images, num_classes, box_dim,
                                        activation, score_thr, nms_pre, img_h, img_w, max_h, max_w, variant_flags, class_agnostic, iou_threshold,
                                        max_per_img, dets, labels, prior_inds, num_dets, workspace, stream);
    };
    return dtype == SPH2POB_DTYPE_F16 ? run(_Float16{}) : run(__bf16{});
}

}  // extern "C"
