// Random sampling of anchor targets for a minibatch (the rank, the sizes and the selection rule: sph2pob_sample.hpp): two launches
// whatever B is, no host read.
//   sample_select_kernel  one workgroup per (image, side), grid (B, 2): sph2pob_sample.hpp's select_side (the body the R-CNN stage's
//                         rcnn_select_kernel runs too) on the image's assigned_gt_inds.  It writes the rank of every row of the
//                         workgroup's side into the workspace — Philox is 20 quarter-rate integer multiplies a row, so it is
//                         evaluated once and the later passes and the apply pass read the word back (random ranks spread over the
//                         histogram's bins, so its atomics seldom meet) — and leaves the side's Pick.
//   sample_apply_kernel   a streaming pass over (B, n): a row that stays in the sample, or is ignored, keeps its targets (copied
//                         when the output is another buffer, untouched when it is the input); a row that leaves gets the background
//                         label and zeros.  Four rows per thread with 16-byte accesses when n % 4 == 0 and the bases allow.  Its
//                         first workgroup also writes the sampled counts and the two averages from the picks, in integers.
// No float atomics and no global counters: the same bits on every call.
#include "sph2pob_sample.hpp"

namespace {

using namespace sph2pob_sample;

// one workgroup of kSelectBlock threads per (image, side): the image's rows, then sph2pob_sample.hpp's select_side, 8 loads ahead
__global__ __launch_bounds__(kSelectBlock) void sample_select_kernel(const int64_t* __restrict__ gt_inds, int n, int64_t n_pad, Draw D,
                                                                     uint32_t* __restrict__ keys, Pick* __restrict__ picks) {
    const int b = blockIdx.x;
    select_side<kSelectBlock, 8>(gt_inds + (int64_t)b * n, n, D.ranks ? D.ranks + (int64_t)b * n : nullptr, keys + (int64_t)b * n_pad, D,
                                 picks);
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
