// R-CNN stage targets on per-image proposals for a minibatch (the operation, the table row, the checks and the workspace:
// sph2pob_rcnn_targets.hpp): four launches whatever B is, no host read, no state between calls.
//   rcnn_pairwise_kernel    grid (column tiles, row chunks, B).  One thread owns one proposal of the image and walks the chunk's GT
//                           rows from LDS with the variant's per-pair function on EVERY pair (the function the pairwise entry runs: the
//                           closed forms cull inside it).  The column's key is a running maximum in registers (equal values keep the
//                           first row); per row the wave reduces the value's ordered bits, a ballot names the first lane that holds the
//                           maximum and lane 0 takes the packed row key into the tile's LDS.  Written once per workgroup: col_part
//                           [chunk][j] and row_part[i][tile] — plain stores, nothing is accumulated across workgroups, so there is
//                           no state to keep zero.  Tiles behind the image's n_b proposals and chunks behind its k_b rows exit.
//   rcnn_candidates_kernel  grid (candidate tiles, B).  One thread per candidate slot c of (B, k_max + M): a GT candidate gets c + 1,
//                           a proposal the MaxIoUAssigner index from its column maximum over the chunks (sph2pob_assign::Rule) and,
//                           with match_low_quality, the low-quality step: the workgroup reduces the GT keys over the tiles 256 rows
//                           at a time into LDS; `overlaps[i, j] == gt_max[i]` can only hold when gt_max[i] <= the column's own
//                           maximum, and only then the pair is evaluated again (same function, same inputs, same bits).  A slot
//                           behind the image's candidates gets -1, which the select and the compaction skip.
//   rcnn_select_kernel      one workgroup per (image, side): sph2pob_sample.hpp's select_side, the body of sample_select_kernel, on
//                           the image's candidate slots (counts, rank words, radix select, tie walk, Pick).
//   rcnn_compact_kernel     one workgroup per image: an exclusive scan of the sampled flags over the candidates, 1 024 at a time,
//                           both sides' counts in the halves of one word (num <= 65 535), and the table row of every sampled
//                           candidate at its place — positives in ascending c, then negatives in ascending c, then padding.  Its
//                           first workgroup also writes the two sums from the picks, in integers.
// No atomics on floats and none on global memory: the same bits on every call.
#include "sph2pob_kernels_common.hpp"
#include "sph2pob_rcnn_targets.hpp"

namespace {

using namespace sph2pob_rcnn;
using sph2pob_assign::Rule;
using sph2pob_assign::threshold_index;
// the packed max / first-argmax keys: sph2pob_assign.hpp's, the column key for rows and columns alike
using sph2pob_assign::max_key_index;
using sph2pob_assign::ordered_bits;
using sph2pob_assign::pack_max_key_bits;
using sph2pob_assign::unpack_max_val;
using sph2pob_assign::wave_max_u32;
namespace SA = sph2pob_sample;
static_assert(kBlock == kTile, "one thread per column of a tile");

struct Boxes {
    const float* proposals; const int64_t* num_proposals; int64_t M, row_stride;
    const float* gt; const int64_t* gt_labels; const int64_t* gt_offsets; int64_t K; int k_max;
};
__device__ __forceinline__ const float* proposal_row(const Boxes& X, int b, int64_t j) { return X.proposals + ((int64_t)b * X.M + j) * X.row_stride; }

template <int VARIANT, int DIM>
__global__ __launch_bounds__(kBlock) void rcnn_pairwise_kernel(Boxes X, int edge, Shape S, unsigned long long* __restrict__ col_part,
                                                               unsigned long long* __restrict__ row_part) {
    __shared__ float row_raw[kRows][5];
    __shared__ unsigned long long row_key[kRows];
    const int tile = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z, lane = threadIdx.x & 63;
    const ImageRows im = image_rows(X.gt_offsets, b, X.K, X.k_max);
    const int n = (int)image_proposals(X.num_proposals, b, X.M);
    const int r0 = chunk * kRows;
    if (r0 >= im.k || tile * kTile >= n) return;   // workgroup-uniform
    const int rows = im.k - r0 < kRows ? im.k - r0 : kRows;
    if ((int)threadIdx.x < rows) {
        float g[5];
        load_row<DIM>(X.gt + (im.lo + r0 + threadIdx.x) * DIM, g);
#pragma unroll
        for (int c = 0; c < 5; c++) row_raw[threadIdx.x][c] = g[c];
        row_key[threadIdx.x] = 0ull;
    }
    const int jraw = tile * kTile + threadIdx.x;
    const bool valid = jraw < n;
    float a[5];
    load_row<DIM>(proposal_row(X, b, valid ? jraw : n - 1), a);   // a lane past the end works on the last proposal and contributes nothing
    __syncthreads();
    unsigned long long ck = 0ull;
    for (int i = 0; i < rows; i++) {
        float g[5];
#pragma unroll
        for (int c = 0; c < 5; c++) g[c] = row_raw[i][c];
        const float v = pair_iou_of<VARIANT, DIM>(g, a, edge);
        const unsigned ob = ordered_bits(v);
        const unsigned long long key = pack_max_key_bits(ob, (unsigned)(r0 + i));
        ck = key > ck ? key : ck;
        const unsigned mine = valid ? ob : 0u;
        const unsigned wm = wave_max_u32(mine);
        const unsigned long long eq = __builtin_amdgcn_ballot_w64(mine == wm);
        if (lane == 0 && wm != 0u) atomicMax(&row_key[i], pack_max_key_bits(wm, (unsigned)(jraw + __builtin_ctzll(eq))));   // wm == 0: a wave past n
    }
    __syncthreads();
    if (valid) col_part[((int64_t)b * S.chunks + chunk) * S.M + jraw] = ck;
    if ((int)threadIdx.x < rows) row_part[((int64_t)b * S.k_max + r0 + threadIdx.x) * S.tiles + tile] = row_key[threadIdx.x];
}

template <int VARIANT, int DIM>
__global__ __launch_bounds__(kBlock) void rcnn_candidates_kernel(Boxes X, int edge, Shape S, Rule rule, int add_gt,
                                                                 const unsigned long long* __restrict__ col_part,
                                                                 const unsigned long long* __restrict__ row_part, int64_t* __restrict__ cand) {
    __shared__ unsigned long long gt_key[kBlock];
    const int b = blockIdx.y;
    const ImageRows im = image_rows(X.gt_offsets, b, X.K, X.k_max);
    const int k = im.k, n = (int)image_proposals(X.num_proposals, b, X.M);
    const int koff = (int)gt_candidates(add_gt, k);
    const int64_t c0 = (int64_t)blockIdx.x * kBlock, c = c0 + threadIdx.x;
    const bool slot = c < S.C, proposal = slot && c >= koff && c < (int64_t)koff + n;
    const int j = proposal ? (int)(c - koff) : 0;
    int64_t a = !slot || c >= (int64_t)koff + n ? -1 : (c < koff ? c + 1 : 0);   // an image without GT: every proposal is background
    float m = 0.0f;
    if (proposal && k > 0) {
        const int chunks = (k + kRows - 1) / kRows;
        unsigned long long ck = 0ull;
        for (int ch = 0; ch < chunks; ch++) {
            const unsigned long long v = col_part[((int64_t)b * S.chunks + ch) * S.M + j];
            ck = v > ck ? v : ck;
        }
        m = unpack_max_val(ck);
        a = threshold_index(m, max_key_index(ck), rule);
    }
    // the low-quality step (max_iou_assigner.py:192-207); workgroup-uniform: the tile holds a proposal of an image with GT
    if (rule.low_quality && k > 0 && n > 0 && c0 + kBlock > koff && c0 < (int64_t)koff + n) {
        const int tiles = (n + kTile - 1) / kTile;
        float box[5] = {0.0f, 0.0f, 1.0f, 1.0f, 0.0f};
        if (proposal && rule.assign_all) load_row<DIM>(proposal_row(X, b, j), box);
        int best = -1;
        for (int r0 = 0; r0 < k; r0 += kBlock) {
            const int i = r0 + threadIdx.x;
            if (i < k) {   // the GT's maximum over the image's tiles, first column on equal values
                unsigned long long key = 0ull;
                for (int t = 0; t < tiles; t++) {
                    const unsigned long long v = row_part[((int64_t)b * S.k_max + i) * S.tiles + t];
                    key = v > key ? v : key;
                }
                gt_key[threadIdx.x] = key;
            }
            __syncthreads();
            const int rows = k - r0 < kBlock ? k - r0 : kBlock;
            if (proposal) {
                for (int ii = 0; ii < rows; ii++) {   // later GTs overwrite earlier ones: the largest matching row wins
                    const unsigned long long key = gt_key[ii];
                    const float gm = unpack_max_val(key);
                    if (!(gm >= rule.min_pos)) continue;
                    if (!rule.assign_all) {
                        if (max_key_index(key) == j) best = r0 + ii;
                    } else if (!(gm > m)) {   // IoU(i, j) <= m: equality needs gm <= m
                        float g[5];
                        load_row<DIM>(X.gt + (im.lo + r0 + ii) * DIM, g);
                        if (pair_iou_of<VARIANT, DIM>(g, box, edge) == gm) best = r0 + ii;
                    }
                }
            }
            __syncthreads();
        }
        if (best >= 0) a = best + 1;
    }
    if (slot) cand[(int64_t)b * S.C + c] = a;
}

// one workgroup of kCompactBlock threads per (image, side) over the image's C candidate slots: sph2pob_sample.hpp's select_side.  The
// candidates are a few thousand, every pass a few iterations: one load ahead
__global__ __launch_bounds__(kCompactBlock) void rcnn_select_kernel(const int64_t* __restrict__ cand, int C, int64_t c_pad, SA::Draw D,
                                                                    uint32_t* __restrict__ keys, SA::Pick* __restrict__ picks) {
    const int b = blockIdx.x;
    SA::select_side<kCompactBlock, 1>(cand + (int64_t)b * C, C, D.ranks ? D.ranks + (int64_t)b * C : nullptr, keys + (int64_t)b * c_pad, D,
                                      picks);
}

template <int DIM, bool ENCODE>
__global__ __launch_bounds__(kCompactBlock) void rcnn_compact_kernel(Boxes X, Shape S, int add_gt, int num, int64_t num_classes, float pos_weight,
                                                                     sph2pob_coder::Norm nm, const int64_t* __restrict__ cand, int64_t c_pad,
                                                                     const uint32_t* __restrict__ keys, const SA::Pick* __restrict__ picks, Table T) {
    constexpr int kWaves = kCompactBlock / 64;
    __shared__ unsigned s_wave[kWaves];
    __shared__ int64_t s_sum;
    const int b = blockIdx.x, tid = threadIdx.x;
    if (b == 0) {   // the batch's sums, in integers and one fixed order
        if (tid == 0) s_sum = 0;
        __syncthreads();
        int64_t part = 0;
        for (int i = tid; i < (int)S.B; i += kCompactBlock) part += picks[2 * i + SA::POS].k + picks[2 * i + SA::NEG].k;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_down(part, o, 64);
        if ((tid & 63) == 0 && part) atomicAdd((unsigned long long*)&s_sum, (unsigned long long)part);   // LDS, integers: any order, one sum
        __syncthreads();
        if (tid == 0) {
            T.num_samples[0] = (float)s_sum;
            T.avg_factor[0] = (float)(s_sum > 1 ? s_sum : 1);
        }
    }
    const ImageRows im = image_rows(X.gt_offsets, b, X.K, X.k_max);
    const int n = (int)image_proposals(X.num_proposals, b, X.M), koff = (int)gt_candidates(add_gt, im.k);
    const int total = koff + n;
    const SA::Pick pp = picks[2 * b + SA::POS], pn = picks[2 * b + SA::NEG];
    const int k_pos = (int)pp.k, k_neg = (int)pn.k;
    const int64_t* gb = cand + (int64_t)b * S.C;
    const uint32_t* kb = keys + (int64_t)b * c_pad;
    const float* gt_b = X.gt + im.lo * DIM;
    const int64_t* labels_b = X.gt_labels ? X.gt_labels + im.lo : nullptr;
    const int64_t base = (int64_t)b * num;
    if (tid == 0) { T.num_pos[b] = k_pos; T.num_neg[b] = k_neg; }
    unsigned running = 0u;   // sampled positives | sampled negatives << 16 in front of the chunk
    for (int c0 = 0; c0 < total; c0 += kCompactBlock) {   // whole workgroups: barriers inside
        const int c = c0 + tid;
        int64_t a = -1;
        int side = SA::IGNORED;
        if (c < total) { a = gb[c]; side = SA::side_of(a); }
        const bool in = side != SA::IGNORED && SA::sampled(kb[c], c, side == SA::POS ? pp : pn);   // (an ignored slot's word was never written)
        const unsigned long long mp = __ballot(in && side == SA::POS), mn = __ballot(in && side == SA::NEG);
        const unsigned long long below = (1ull << (tid & 63)) - 1ull;
        const unsigned in_wave = (unsigned)__popcll(mp & below) | ((unsigned)__popcll(mn & below) << 16);
        const unsigned before = sph2pob_select::tie_scan<kWaves>(in_wave, (unsigned)__popcll(mp) | ((unsigned)__popcll(mn) << 16), s_wave, running);
        if (in) {
            const int r = side == SA::POS ? (int)(before & 0xffffu) : k_pos + (int)(before >> 16);
            const bool from_gt = c < koff;
            const float* box = from_gt ? gt_b + (int64_t)c * DIM : proposal_row(X, b, c - koff);
            if (r < num) write_sampled<DIM, ENCODE>(T, base + r, b, c, a, from_gt, box, gt_b, labels_b, num_classes, pos_weight, nm);
        }
        __syncthreads();   // s_wave is reused
    }
    for (int r = k_pos + k_neg + tid; r < num; r += kCompactBlock) write_padding<DIM>(T, base + r, b, num_classes);
}

struct RcnnLaunch {
    Boxes X; int edge; Shape S; Rule rule; int add_gt; SA::Draw D; int64_t num_classes; float pos_weight; bool encode; sph2pob_coder::Norm nm;
    Table T; Workspace W; hipStream_t s; bool fast = true;
    template <int V, int D_> int run() {
        if (!fast) return SPH2POB_ERR_OPTION;
        if (S.k_max > 0)
            hipLaunchKernelGGL((rcnn_pairwise_kernel<V, D_>), dim3((unsigned)S.tiles, (unsigned)S.chunks, (unsigned)S.B), dim3(kBlock), 0, s, X, edge, S,
                               W.col_part, W.row_part);
        hipLaunchKernelGGL((rcnn_candidates_kernel<V, D_>), dim3((unsigned)((S.C + kBlock - 1) / kBlock), (unsigned)S.B), dim3(kBlock), 0, s, X, edge, S,
                           rule, add_gt, W.col_part, W.row_part, W.cand);
        hipLaunchKernelGGL(rcnn_select_kernel, dim3((unsigned)S.B, 2), dim3(kCompactBlock), 0, s, W.cand, (int)S.C, W.sample.n_pad, D, W.sample.keys,
                           W.sample.picks);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)S.B), dim3(kCompactBlock), 0, s, X, S, add_gt, (int)D.num, num_classes, pos_weight, nm, W.cand,
                               W.sample.n_pad, W.sample.keys, W.sample.picks, T);
        };
        if (encode) go(rcnn_compact_kernel<D_, true>); else go(rcnn_compact_kernel<D_, false>);
        return launch_status();
    }
};

}  // namespace

extern "C" {

int64_t sph2pob_rcnn_targets_workspace_bytes(int64_t num_images, int64_t m, int64_t k_max) { return workspace_bytes(num_images, m, k_max); }

int sph2pob_rcnn_targets_f32(const float* proposals, const int64_t* num_proposals, int64_t num_images, int64_t m, int64_t row_stride,
                             const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets, int64_t num_gt, int64_t k_max, int box_dim,
                             int variant, int edge, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi, float min_pos_iou,
                             int match_low_quality, int gt_max_assign_all, int64_t num, int64_t num_expected_pos, double neg_pos_ub, int64_t seed,
                             const int64_t* seed_device, const uint32_t* ranks, int add_gt, int64_t num_classes, float pos_weight, int encode,
                             const float* means_host, const float* stds_host, float* rois, int64_t* labels, float* label_weights,
                             float* bbox_targets, float* bbox_weights, int64_t* pos_assigned_gt_inds, int64_t* sample_inds,
                             unsigned char* is_gt, int64_t* num_pos, int64_t* num_neg, float* avg_factor, float* num_samples, void* workspace,
                             void* stream) {
    const Table T{rois, labels, label_weights, bbox_targets, bbox_weights, pos_assigned_gt_inds, sample_inds, is_gt, num_pos, num_neg, avg_factor,
                  num_samples};
    if (int rc = check(check_common(box_dim, variant, edge, 0), variant, proposals, num_images, m, row_stride, box_dim, gt, gt_offsets, num_gt, k_max,
                       num, num_expected_pos, neg_pos_ub, add_gt, encode, T, true, workspace))
        return rc;
    const Shape S = shape_of(num_images, m, k_max);
    return dispatch(variant, box_dim,
                    RcnnLaunch{Boxes{proposals, num_proposals, m, row_stride, gt, gt_labels, gt_offsets, num_gt, (int)k_max}, naive_edge(variant, edge), S,
                               Rule{pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all}, add_gt,
                               SA::Draw{num_expected_pos, num, neg_pos_ub, seed, seed_device, ranks}, num_classes, pos_weight, encode != 0,
                               sph2pob_coder::make_norm(means_host, stds_host, box_dim), T, carve(workspace, S), (hipStream_t)stream});
}

}  // extern "C"
