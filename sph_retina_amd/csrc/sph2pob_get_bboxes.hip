// libsph2pob_hip.so — detection post-processing for a minibatch (sph2pob_test_bboxes_f32 / sph2pob_get_bboxes_f32, include/sph2pob_hip.h): per (image,
// level) exact top-k of the class scores above a threshold, read from the head's own layout; gather + decode of the selected
// candidates; then the batched NMS stage of sph2pob_nms.hip.  Replaces SphRetinaHead._get_bboxes_single / _bbox_post_process
// (sphdet/models/heads/sph_retina_head.py:101-216, :22-99) and filter_scores_and_topk (mmdet/core/utils/misc.py:119-165) for
// B images with a number of launches that does not depend on B, and without a host read.  gfx950 only.  Every head runs the same
// pipeline() and the same cand_build_kernel; what differs is the candidate source the kernel is instantiated with, and the twin
// (bboxes_cpu of sph2pob_host.hip) calls the same sources: DeltaSource (sph2pob_get_bboxes.hpp) for the delta coders,
// PointSource (there) for SphFCOSHead (sph_fcos_head.py:246-323, :205-244: decode from points, class score times the point's
// centerness) and RoiSource (sph2pob_rcnn_bboxes.hpp) for the R-CNN stage, sph2pob_rcnn_bboxes_f32 (sph2pob_rcnn_bboxes.hip: one
// flat level of the probabilities its stage 0 wrote, the priors are the images' own rois and the deltas are per class).
//
// Selection, per (image, level), on the unique 64-bit keys (descending score bits << 32 | flat index):
//   zero          the histograms and the per-(image, level) records
//   topk_hist     stream 1: scores above the threshold -> a histogram of score_bin() (LDS per workgroup, integer atomics into the
//                 level's global histogram: the totals do not depend on the order of arrival)
//   topk_cut      the bin in which the nms_pre-th key falls, how many keys are wanted and how many lie in the bins up to it
//   topk_compact  stream 2: every key in those bins -> the level's survivor buffer, ballot + mbcnt compaction (the SET of
//                 survivors is fixed by the histogram, their order in the buffer is not and is never used)
//   topk_resolve  radix select among the survivors -> the exact nms_pre-th key; the keys up to it -> the level's selection
//   cand_build    rank of every selected key among the level's selection (the final order), then the head's candidate source:
//                 box / score / label / prior index written at its place of the image's candidate block
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_get_bboxes.hpp"    // (the parameter blocks, DeltaSource and PointSource, the declaration of the NMS stage)
#include "sph2pob_rcnn_bboxes.hpp"   // (RoiSource)

namespace {

using namespace sph2pob_gb;
namespace RB = sph2pob_rcnn_bb;

constexpr int kSelBlock = 256, kSelIters = 16, kChunk = kSelBlock * 4 * kSelIters;   // 16 384 scores per workgroup
static_assert(kChunk == kChunkElems, "the level table counts its chunks in kChunkElems");
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

// One lane per selected key: its rank among the level's selection (tiles of the selection in LDS).  False for a lane (or a whole
// workgroup) without a key; else `mine` is the lane's key and `at` its row of the candidate block
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

// Launch 6, for every head: the source's prologue in the first workgroup of an image (nothing, except for RoiSource), the place of
// the lane's key, key index -> (prior ai, class c), the source's guard, its box / score / prior index, the four stores
template <class Source>
__global__ __launch_bounds__(kBuildBlock) void cand_build_kernel(Levels L, const Meta* __restrict__ meta, const unsigned long long* __restrict__ sel,
                                                               int num_classes, Source source, float* __restrict__ boxes, float* __restrict__ scores,
                                                               int64_t* __restrict__ labels, int* __restrict__ prior, int* __restrict__ counts,
                                                               const int* __restrict__ hist) {
    __shared__ unsigned long long tile[kBuildBlock];
    const int l = blockIdx.y, b = blockIdx.z;
    if (blockIdx.x == 0 && l == 0) source.prologue(hist, b);   // workgroup-uniform
    unsigned long long mine;
    int64_t at;
    if (!cand_place(L, meta, sel, counts, tile, mine, at)) return;
    const unsigned flat = (unsigned)mine;
    const int ai = (int)(flat / (unsigned)num_classes), c = (int)(flat - (unsigned)ai * (unsigned)num_classes);
    const Level& lv = L.lv[l];
    if (!source.has(lv, ai)) return;
    float box[5];
    int prior_index;
    const float score = source(lv, l, b, ai, c, score_of_desc_bits((unsigned)(mine >> 32)), box, &prior_index);
#pragma unroll
    for (int k = 0; k < Source::kDim; k++) boxes[at * Source::kDim + k] = box[k];
    scores[at] = score;
    labels[at] = c;
    prior[at] = prior_index;
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
    w.nms = (void*)(p + off); off += nms_batch_workspace_bytes(B, L.k_cap, box_dim);
    w.bytes = off;
    return w;
}

// The ten launches on a checked level table: the selection on the class scores (TS: their element type), cand_build_kernel with the
// head's candidate source, the NMS stage
template <class TS, class Source>
int pipeline(const Levels& L, const Shape& sh, const Selection& sel, const Nms& nms, const Outputs& out, void* workspace, void* stream,
             const Source& source) {
    if (!workspace) return SPH2POB_ERR_NULL;
    if (int rc = out.check(nms.max_per_img)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int B = (int)sh.num_images;
    const Ws w = make_ws(workspace, L, B, sh.box_dim);
    const int pre = (int)(sel.nms_pre < ((int64_t)1 << 30) ? sel.nms_pre : ((int64_t)1 << 30));
    if ((reinterpret_cast<uintptr_t>(w.hist) & 15) == 0) launch_zero<int4>(w.hist, w.zero_bytes, s);
    else launch_zero<int>(w.hist, w.zero_bytes, s);
    hipLaunchKernelGGL(topk_hist_kernel<TS>, dim3(L.chunks, B), dim3(kSelBlock), 0, s, L, sel.activation, sel.score_thr, w.hist);
    hipLaunchKernelGGL(topk_cut_kernel, dim3(L.num, B), dim3(kResBlock), 0, s, L, pre, (const int*)w.hist, w.meta);
    hipLaunchKernelGGL(topk_compact_kernel<TS>, dim3(L.chunks, B), dim3(kSelBlock), 0, s, L, sel.activation, sel.score_thr, w.meta, w.buf);
    hipLaunchKernelGGL(topk_resolve_kernel, dim3(L.num, B), dim3(kResBlock), 0, s, L, (const Meta*)w.meta, (const unsigned long long*)w.buf, w.sel);
    int max_cap = 0;
    for (int l = 0; l < L.num; l++) max_cap = L.lv[l].cap > max_cap ? L.lv[l].cap : max_cap;
    hipLaunchKernelGGL(cand_build_kernel<Source>, dim3((max_cap + kBuildBlock - 1) / kBuildBlock, L.num, B), dim3(kBuildBlock), 0, s, L,
                       (const Meta*)w.meta, (const unsigned long long*)w.sel, (int)sh.num_classes, source, w.boxes, w.scores, w.labels, w.prior,
                       w.counts, (const int*)w.hist);
    if (int rc = launch_status()) return rc;
    return nms_batch_launch(Candidates{w.boxes, w.scores, w.labels, w.prior, w.counts, L.k_cap}, B, sh.box_dim, nms, w.nms, out, s);
}

// the delta coders on a checked level table.  TS: the element type of the scores, TD: of the deltas (anchors and every output are
// fp32 / int64 whatever they are)
template <class TS, class TD>
int delta_pipeline(const Levels& L, const Shape& sh, const Selection& sel, const Coder& cd, const Nms& nms, const Outputs& out, void* workspace,
                   void* stream) {
    return with_dim(sh.box_dim, [&](auto dim) {
        return pipeline<TS>(L, sh, sel, nms, out, workspace, stream, DeltaSource<decltype(dim)::value, TD>{cd});
    });
}

// the entries on the head's own tensors.  The public ones read scores and deltas (and centernesses) as one type T
struct Head { const void* const* cls_scores; const void* const* bbox_preds; const void* const* priors; };
template <class T>
int test_bboxes(const Head& h, const Shape& sh, const Selection& sel, const Coder& cd, const Nms& nms, const Outputs& out, void* workspace,
                void* stream) {
    Levels L;
    if (int rc = make_levels(h.cls_scores, h.bbox_preds, h.priors, sh, sel, cd, nms, &L)) return rc;
    return delta_pipeline<T, T>(L, sh, sel, cd, nms, out, workspace, stream);
}
template <class T>
int fcos_bboxes(const Head& h, const void* const* centernesses, const Shape& sh, const Selection& sel, const Frame& fr, const Nms& nms,
                const Outputs& out, void* workspace, void* stream) {
    Levels L;
    Factors F;
    if (int rc = make_point_levels(h.cls_scores, h.bbox_preds, h.priors, centernesses, sh, sel, nms, fr, &L, &F)) return rc;
    return with_dim(sh.box_dim, [&](auto dim) {
        return pipeline<T>(L, sh, sel, nms, out, workspace, stream, PointSource<decltype(dim)::value, T>{F, fr.image(), sel.activation});
    });
}

}  // namespace

namespace sph2pob_gb {
int test_bboxes_on_probs(const Levels& L, const Shape& sh, const Selection& sel, const Coder& cd, const Nms& nms, const Outputs& out,
                         void* workspace, int delta_dtype, void* stream) {
    return with_f32_or_h16(delta_dtype, [&](auto t) { return delta_pipeline<float, decltype(t)>(L, sh, sel, cd, nms, out, workspace, stream); });
}
}  // namespace sph2pob_gb

namespace sph2pob_rcnn_bb {
int rois_bboxes_on_probs(const GB::Levels& L, const Rois& R, const GB::Shape& sh, const GB::Selection& sel, const GB::Coder& cd, const GB::Nms& nms,
                         const GB::Outputs& out, int64_t* num_valid, void* workspace, void* stream) {
    return with_dim(sh.box_dim, [&](auto dim) {
        return pipeline<float>(L, sh, sel, nms, out, workspace, stream, RoiSource<decltype(dim)::value>{R, cd, num_valid});
    });
}
}  // namespace sph2pob_rcnn_bb

extern "C" {

int64_t sph2pob_get_bboxes_workspace_bytes(const int64_t* level_n, int num_levels, int64_t num_images, int64_t num_classes, int box_dim,
                                           int64_t nms_pre) {
    Levels L;
    if (make_level_shapes(Shape{level_n, nullptr, num_levels, num_images, num_classes, box_dim}, Selection{0, 0.0f, nms_pre}, Coder{},
                          Nms{SPH2POB_VARIANT_EFFICIENT, 0, 0.0f, 0}, true, &L))
        return 0;
    return make_ws(nullptr, L, num_images, box_dim).bytes;
}

// The public entries fill the parameter blocks, here and nowhere below
int sph2pob_test_bboxes_f32(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                            const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                            float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                            int coder_flags, float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img,
                            float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream) {
    return test_bboxes<float>(Head{cls_scores, bbox_preds, anchors}, Shape{level_n, level_hw, num_levels, num_images, num_classes, box_dim},
                              Selection{activation, score_thr, nms_pre}, make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp),
                              Nms{variant_flags, class_agnostic, iou_threshold, max_per_img}, Outputs{dets, labels, prior_inds, num_dets}, workspace, stream);
}

int sph2pob_test_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                            const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                            float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                            int coder_flags, float ctr_clamp, int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img,
                            float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream) {
    if (dtype != SPH2POB_DTYPE_F16 && dtype != SPH2POB_DTYPE_BF16) return SPH2POB_ERR_OPTION;
    return with_h16(dtype, [&](auto t) {
        return test_bboxes<decltype(t)>(Head{cls_scores, bbox_preds, anchors}, Shape{level_n, level_hw, num_levels, num_images, num_classes, box_dim},
                                        Selection{activation, score_thr, nms_pre}, make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp),
                                        Nms{variant_flags, class_agnostic, iou_threshold, max_per_img}, Outputs{dets, labels, prior_inds, num_dets}, workspace, stream);
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
    return fcos_bboxes<float>(Head{cls_scores, bbox_preds, points}, centernesses, Shape{level_n, level_hw, num_levels, num_images, num_classes, box_dim},
                              Selection{activation, score_thr, nms_pre}, Frame{img_h, img_w, max_h, max_w},
                              Nms{variant_flags, class_agnostic, iou_threshold, max_per_img}, Outputs{dets, labels, prior_inds, num_dets}, workspace, stream);
}

int sph2pob_fcos_bboxes_h16(const void* const* cls_scores, const void* const* bbox_preds, const void* const* points, const void* const* centernesses,
                            const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim,
                            int activation, float score_thr, int64_t nms_pre, int64_t img_h, int64_t img_w, float max_h, float max_w,
                            int variant_flags, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets, int64_t* labels,
                            int64_t* prior_inds, int64_t* num_dets, void* workspace, int dtype, void* stream) {
    if (dtype != SPH2POB_DTYPE_F16 && dtype != SPH2POB_DTYPE_BF16) return SPH2POB_ERR_OPTION;
    return with_h16(dtype, [&](auto t) {
        return fcos_bboxes<decltype(t)>(Head{cls_scores, bbox_preds, points}, centernesses, Shape{level_n, level_hw, num_levels, num_images, num_classes, box_dim},
                                        Selection{activation, score_thr, nms_pre}, Frame{img_h, img_w, max_h, max_w},
                                        Nms{variant_flags, class_agnostic, iou_threshold, max_per_img}, Outputs{dets, labels, prior_inds, num_dets}, workspace, stream);
    });
}

}  // extern "C"
