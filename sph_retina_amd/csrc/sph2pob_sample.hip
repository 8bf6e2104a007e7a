// Random sampling of anchor targets for a minibatch (the rank, the sizes and the selection rule: sph2pob_sample.hpp): two launches
// whatever B is, no host read.
//   sample_select_kernel  one workgroup per (image, side), grid (B, 2).  The first pass over the image's assigned_gt_inds counts
//                         P_b and N_b (both workgroups count both: k_neg needs k_pos, and they do not communicate) and writes the
//                         rank of every row of the workgroup's side into the workspace — Philox is 20 quarter-rate integer multiplies a row, so
//                         it is evaluated once and the later passes and the apply pass read the word back.  Then the k-th smallest
//                         rank by a four-digit radix select (LDS histogram, integer atomics; random ranks spread over the bins, so
//                         the atomics seldom meet) and, only when the rows tied at that rank are not all taken, one in-order walk
//                         for the row index up to which they are.  Digit decision and tie scan: sph2pob_select.hpp, ascending.
//   sample_apply_kernel   a streaming pass over (B, n): a row that stays in the sample, or is ignored, keeps its targets (copied
//                         when the output is another buffer, untouched when it is the input); a row that leaves gets the background
//                         label and zeros.  Four rows per thread with 16-byte accesses when n % 4 == 0 and the bases allow.  Its
//                         first workgroup also writes the sampled counts and the two averages from the picks, in integers.
// No float atomics and no global counters: the same bits on every call.
#include "sph2pob_sample.hpp"

namespace {

using namespace sph2pob_sample;

struct Draw {
    int64_t num_expected_pos, num;
    double neg_pos_ub;
    int64_t seed;
    const int64_t* seed_dev;     // wins over `seed` when non-NULL
    const uint32_t* ranks;       // (B, n) caller's ranks instead of the generator, or NULL
};

// One workgroup of kSelectBlock threads per (image, side).  Row i of the image belongs to thread i % kSelectBlock in every pass, so
// a thread reads back the rank words it wrote itself.
__global__ __launch_bounds__(kSelectBlock) void sample_select_kernel(const int64_t* __restrict__ gt_inds, int n, int64_t n_pad, Draw D,
                                                                     uint32_t* __restrict__ keys, Pick* __restrict__ picks) {
    constexpr int kWaves = kSelectBlock / 64, kAhead = 8;
    __shared__ unsigned hist[256];
    __shared__ unsigned s_count[2], s_prefix, s_rem, s_ties, s_wave[kWaves];
    __shared__ int s_upto;
    const int b = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    const int64_t* gb = gt_inds + (int64_t)b * n;
    const uint32_t* rank_in = D.ranks ? D.ranks + (int64_t)b * n : nullptr;
    uint32_t* kb = keys + (int64_t)b * n_pad;
    if (tid == 0) { s_count[0] = 0u; s_count[1] = 0u; s_prefix = 0u; s_rem = 0u; s_ties = 0u; s_upto = 0; }
    const uint64_t seed = (uint64_t)(D.seed_dev ? D.seed_dev[0] : D.seed);
    int64_t k = 0;

    // radix select, most significant digit first: after digit d the top 8 (d + 1) bits of the k-th smallest rank are known
    for (int d = 0; d < 4; d++) {
        const int shift = 24 - 8 * d;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = s_prefix, rem_in = s_rem;
        if (d == 0) {
            unsigned np = 0u, nn = 0u;
            for (int64_t i0 = tid; i0 < n; i0 += kAhead * kSelectBlock) {   // kAhead independent loads in flight, then the arithmetic
                int64_t g[kAhead];
                uint32_t r[kAhead];
#pragma unroll
                for (int u = 0; u < kAhead; u++) {
                    const int64_t i = i0 + (int64_t)u * kSelectBlock;
                    g[u] = i < n ? gb[i] : -1;   // past the end: an ignored row
                    r[u] = rank_in && i < n ? rank_in[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < kAhead; u++) {
                    const int64_t i = i0 + (int64_t)u * kSelectBlock;
                    const int c = side_of(g[u]);
                    np += c == POS; nn += c == NEG;
                    if (c == side) {
                        if (!rank_in) r[u] = row_rank(seed, (uint32_t)b, (uint32_t)i);
                        kb[i] = r[u];
                        atomicAdd(&hist[r[u] >> 24], 1u);
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { np += __shfl_down(np, o, 64); nn += __shfl_down(nn, o, 64); }
            if ((tid & 63) == 0) { atomicAdd(&s_count[POS], np); atomicAdd(&s_count[NEG], nn); }
        } else if (rem_in > 0u) {   // workgroup-uniform
            const unsigned known = 0xffffffffu << (shift + 8);   // the digits already fixed
            for (int64_t i0 = tid; i0 < n; i0 += kAhead * kSelectBlock) {
                int64_t g[kAhead];
                uint32_t r[kAhead];
#pragma unroll
                for (int u = 0; u < kAhead; u++) {   // both loads of every row at once: the word of a row of the other side is not used
                    const int64_t i = i0 + (int64_t)u * kSelectBlock;
                    g[u] = i < n ? gb[i] : -1;
                    r[u] = i < n ? kb[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < kAhead; u++) {
                    if (side_of(g[u]) == side && ((r[u] ^ prefix) & known) == 0u) atomicAdd(&hist[(r[u] >> shift) & 255u], 1u);
                }
            }
        }
        __syncthreads();
        if (d == 0) {
            int64_t kp, kn;
            sample_sizes((int64_t)s_count[POS], (int64_t)s_count[NEG], D.num_expected_pos, D.num, D.neg_pos_ub, &kp, &kn);
            k = side == POS ? kp : kn;   // <= the side's rows < 2^31
        }
        // the digit: the one bin that holds the rem-th smallest rank
        sph2pob_select::digit_decision<false>(hist, s_wave, &s_prefix, &s_rem, &s_ties, prefix, shift,
                                              [&](unsigned) { return d == 0 ? (unsigned)k : rem_in; });
    }
    const unsigned take = s_rem;          // rows tied at the k-th rank that are taken (>= 1 when anything is)
    const unsigned cut = s_prefix;
    const bool walk = take > 0u && take < s_ties;   // workgroup-uniform; otherwise every tied row is taken
    __syncthreads();

    // in-order walk: the index of the take-th row tied at the cut
    if (walk) {
        unsigned running = 0u;
        for (int64_t i0 = 0; i0 < n; i0 += kSelectBlock) {   // whole workgroups: barriers inside
            const int64_t i = i0 + tid;
            const bool tie = i < n && side_of(gb[i]) == side && kb[i] == cut;
            const unsigned long long m = __ballot(tie);
            const unsigned in_wave = (unsigned)__popcll(m & ((1ull << (tid & 63)) - 1ull));
            const unsigned before = sph2pob_select::tie_scan<kWaves>(in_wave, (unsigned)__popcll(m), s_wave, running);
            if (tie && before + 1u == take) s_upto = (int)(i + 1);   // one thread of one iteration
            __syncthreads();
            if (running >= take) break;   // workgroup-uniform
        }
    }
    if (tid == 0) {
        Pick p;
        p.cut.key = take > 0u ? cut : 0u;
        p.cut.upto = take > 0u ? (walk ? s_upto : n) : 0;
        p.k = k;
        picks[2 * b + side] = p;
    }
}

struct Targets {
    const int64_t* labels_in; const float* label_weights_in; const float* bbox_targets_in; const float* bbox_weights_in;
    int64_t* labels; float* label_weights; float* bbox_targets; float* bbox_weights;
    unsigned char* flags; int64_t* num_pos; int64_t* num_neg; float* avg_factor; float* avg_factor_pos;
    int64_t num_classes;
};

// the sampled counts of the images and the two averages, by the first workgroup: integers, one fixed order
__device__ __forceinline__ void write_counts(const Pick* __restrict__ picks, int B, const Targets& T) {
    __shared__ int64_t sm[2][kBlock / 64];
    int64_t sp = 0, sn = 0;
    for (int b = threadIdx.x; b < B; b += kBlock) {
        const int64_t kp = picks[2 * b + POS].k, kn = picks[2 * b + NEG].k;
        T.num_pos[b] = kp; T.num_neg[b] = kn;
        sp += kp > 1 ? kp : 1; sn += kn > 1 ? kn : 1;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { sp += __shfl_down(sp, o, 64); sn += __shfl_down(sn, o, 64); }
    if ((threadIdx.x & 63) == 0) { sm[0][threadIdx.x >> 6] = sp; sm[1][threadIdx.x >> 6] = sn; }
    __syncthreads();
    if (threadIdx.x == 0) {
        sp = 0; sn = 0;
#pragma unroll
        for (int wv = 0; wv < kBlock / 64; wv++) { sp += sm[0][wv]; sn += sm[1][wv]; }
        T.avg_factor[0] = (float)(sp + sn);
        T.avg_factor_pos[0] = (float)sp;
    }
}

// one row that is not part of a whole quad of leaving rows
template <int DIM>
__device__ __forceinline__ void apply_row(const Targets& T, int64_t r, bool keep) {
    if (keep) {
        if (T.labels != T.labels_in) T.labels[r] = T.labels_in[r];
        if (T.label_weights != T.label_weights_in) T.label_weights[r] = T.label_weights_in[r];
#pragma unroll
        for (int c = 0; c < DIM; c++) {
            if (T.bbox_targets != T.bbox_targets_in) T.bbox_targets[r * DIM + c] = T.bbox_targets_in[r * DIM + c];
            if (T.bbox_weights != T.bbox_weights_in) T.bbox_weights[r * DIM + c] = T.bbox_weights_in[r * DIM + c];
        }
    } else {
        T.labels[r] = T.num_classes;
        T.label_weights[r] = 0.0f;
#pragma unroll
        for (int c = 0; c < DIM; c++) { T.bbox_targets[r * DIM + c] = 0.0f; T.bbox_weights[r * DIM + c] = 0.0f; }
    }
}

// grid (workgroups of an image, B); V rows per thread.  V == 4: n % 4 == 0 and every base 16-byte aligned
template <int DIM, int V>
__global__ __launch_bounds__(kBlock) void sample_apply_kernel(const int64_t* __restrict__ gt_inds, int n, int64_t n_pad, int B,
                                                              const uint32_t* __restrict__ keys, const Pick* __restrict__ picks, Targets T) {
    if (blockIdx.x == 0 && blockIdx.y == 0) write_counts(picks, B, T);
    const int b = blockIdx.y;
    const int64_t i0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) * V;
    if (i0 >= n) return;
    const int64_t r0 = (int64_t)b * n + i0;
    const Pick pp = picks[2 * b + POS], pn = picks[2 * b + NEG];
    int64_t g[V];
    uint32_t rk[V];
    if constexpr (V == 4) {
        const longlong2 g01 = *reinterpret_cast<const longlong2*>(gt_inds + r0), g23 = *reinterpret_cast<const longlong2*>(gt_inds + r0 + 2);
        const uint4 kq = *reinterpret_cast<const uint4*>(keys + (int64_t)b * n_pad + i0);
        g[0] = g01.x; g[1] = g01.y; g[2] = g23.x; g[3] = g23.y;
        rk[0] = kq.x; rk[1] = kq.y; rk[2] = kq.z; rk[3] = kq.w;
    } else {
        g[0] = gt_inds[r0];
        rk[0] = keys[(int64_t)b * n_pad + i0];
    }
    bool keep[V], any_keep = false;
    unsigned char fl[V];
#pragma unroll
    for (int e = 0; e < V; e++) {
        const int c = side_of(g[e]);
        const bool in = c != IGNORED && sampled(rk[e], i0 + e, c == POS ? pp : pn);   // (an ignored row's word was never written)
        fl[e] = in ? (unsigned char)(c + 1) : (unsigned char)0;
        keep[e] = in || c == IGNORED;
        any_keep |= keep[e];
    }
    if constexpr (V == 4) {
        *reinterpret_cast<uchar4*>(T.flags + r0) = make_uchar4(fl[0], fl[1], fl[2], fl[3]);
        if (!any_keep) {   // the common quad: four rows leave, nothing is read
            const longlong2 lab = make_longlong2(T.num_classes, T.num_classes);
            const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            *reinterpret_cast<longlong2*>(T.labels + r0) = lab;
            *reinterpret_cast<longlong2*>(T.labels + r0 + 2) = lab;
            *reinterpret_cast<float4*>(T.label_weights + r0) = z;
#pragma unroll
            for (int c = 0; c < DIM; c++) {   // 4 DIM floats: DIM 16-byte stores
                *reinterpret_cast<float4*>(T.bbox_targets + r0 * DIM + 4 * c) = z;
                *reinterpret_cast<float4*>(T.bbox_weights + r0 * DIM + 4 * c) = z;
            }
            return;
        }
    } else {
        T.flags[r0] = fl[0];
    }
#pragma unroll
    for (int e = 0; e < V; e++) apply_row<DIM>(T, r0 + e, keep[e]);
}

}  // namespace

extern "C" {

int64_t sph2pob_sample_targets_workspace_bytes(int64_t num_images, int64_t n) { return workspace_bytes(num_images, n); }

int sph2pob_sample_targets_f32(const int64_t* gt_inds, int64_t num_images, int64_t n, int box_dim, const int64_t* labels_in,
                               const float* label_weights_in, const float* bbox_targets_in, const float* bbox_weights_in,
                               int64_t num_classes, int64_t num_expected_pos, int64_t num, double neg_pos_ub, int64_t seed,
                               const int64_t* seed_device, const uint32_t* ranks, int64_t* labels, float* label_weights,
                               float* bbox_targets, float* bbox_weights, unsigned char* sample_flags, int64_t* num_pos, int64_t* num_neg,
                               float* avg_factor, float* avg_factor_pos, void* workspace, void* stream) {
    if (int rc = check_shape(num_images, n, box_dim, num_expected_pos, num, neg_pos_ub)) return rc;
    if (!gt_inds || !labels_in || !label_weights_in || !bbox_targets_in || !bbox_weights_in || !labels || !label_weights || !bbox_targets ||
        !bbox_weights || !sample_flags || !num_pos || !num_neg || !avg_factor || !avg_factor_pos || !workspace) return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const Workspace ws = carve(workspace, num_images, n);
    const Draw D{num_expected_pos, num, neg_pos_ub, seed, seed_device, ranks};
    hipLaunchKernelGGL(sample_select_kernel, dim3((unsigned)num_images, 2), dim3(kSelectBlock), 0, s, gt_inds, (int)n, ws.n_pad, D, ws.keys, ws.picks);
    const Targets T{labels_in, label_weights_in, bbox_targets_in, bbox_weights_in, labels, label_weights, bbox_targets, bbox_weights,
                    sample_flags, num_pos, num_neg, avg_factor, avg_factor_pos, num_classes};
    const bool vec = n % 4 == 0 && aligned_to(gt_inds, 16) && aligned_to(labels, 16) && aligned_to(label_weights, 16) &&
                     aligned_to(bbox_targets, 16) && aligned_to(bbox_weights, 16) && aligned_to(sample_flags, 4);
    auto go = [&](auto kernel, int v) {
        const int64_t per_image = (n / v + kBlock - 1) / kBlock;
        hipLaunchKernelGGL(kernel, dim3((unsigned)per_image, (unsigned)num_images), dim3(kBlock), 0, s, gt_inds, (int)n, ws.n_pad, (int)num_images,
                           ws.keys, ws.picks, T);
    };
    if (box_dim == 4) { if (vec) go(sample_apply_kernel<4, 4>, 4); else go(sample_apply_kernel<4, 1>, 1); }
    else { if (vec) go(sample_apply_kernel<5, 4>, 4); else go(sample_apply_kernel<5, 1>, 1); }
    return launch_status();
}

}  // extern "C"
