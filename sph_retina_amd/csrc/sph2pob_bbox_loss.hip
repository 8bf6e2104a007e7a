// Fused box-regression loss kernels (level table and checks: sph2pob_bbox_loss.hpp).
//   bbox_loss_kernel   ONE grid over all images and levels of a head: a workgroup finds its level in the table (as focal_sum_kernel
//                      does), each of its four waves owns one span — a few hundred consecutive anchors of one image and one level.
//                      The wave scans the span's weights and pushes the indices of the rows whose weight is not zero on a
//                      wave-private LDS stack (ballot / mbcnt, as the aligned chunk kernel compacts its survivors), then runs
//                      gather -> decode -> loss + adjoint -> decode adjoint in dense passes of up to 64 positives.  The gradients of
//                      the span are assembled in a wave-private LDS tile laid out like the span's slice of the head's tensor —
//                      zeros, then the positives' values — and leave in one sweep: every element is stored once, by one lane, in
//                      whole 16-byte stores along w where the level allows it.  The weighted losses are added in double and leave
//                      one partial per workgroup.
//   bbox_final_kernel  one workgroup adds the partials in a fixed order (no float atomics, no global counter: the same bits on
//                      every call)
// A row whose mean weight is exactly 0 is never gathered: its deltas and targets are not read, its loss and gradient are exact
// zeros.  (The loss kernels of sph2pob_loss.hip skip per wave of 64 rows; here the rule is per row.)
#include <type_traits>

#include "sph2pob_kernels_common.hpp"
#include "sph2pob_bbox_loss.hpp"

namespace {

namespace BL = sph2pob_bbox;
namespace CD = sph2pob_coder;

static_assert(kBlock == 64 * BL::kWaves, "one span per wave");

// waves per SIMD the kernel is compiled for: decode + loss + both adjoints + the gather / tile addressing take 144 - 152 VGPRs in
// the gradient instantiations (70 - 88 forward only), no scratch: three waves of 170 registers per SIMD.  The LDS (tile + stack:
// 26 KiB per workgroup) would admit six workgroups per CU
constexpr int kBboxWaves = 3;

__device__ __forceinline__ double block_sum_f64(double v) {
    __shared__ double sm[kBlock / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < kBlock / 64; k++) r += sm[k];
    }
    return r;
}

__device__ __forceinline__ int level_of_block(const BL::Levels& L, int block) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < BL::kMaxLevels; q++) l += (q < L.num && block >= L.lv[q].block_off) ? 1 : 0;
    return l;
}

template <int DIM, bool FAST, bool GRAD>
__global__ __launch_bounds__(kBlock, kBboxWaves) void bbox_loss_kernel(BL::Levels L, const float* __restrict__ anchors,
                                                                       const float* __restrict__ targets, const float* __restrict__ weight,
                                                                       int wd, CD::Norm nm, float max_ratio, int cflags, float ctr_clamp,
                                                                       int loss_mode, float eps, float scale,
                                                                       const float* __restrict__ avg_factor, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float tile_s[GRAD ? BL::kWaves * BL::kTile : 4];
    __shared__ unsigned short stack_s[BL::kWaves * BL::kStack];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int l = level_of_block(L, blockIdx.x);
    const BL::Level& lv = L.lv[l];
    const int item = ((int)blockIdx.x - lv.block_off) * BL::kWaves + wave;
    double acc = 0.0;
    if (item < lv.items) {   // wave-uniform
        const int b = item / lv.spans, sp = item - b * lv.spans;
        const int p_lo = sp * lv.ps;
        const int cnt = min(lv.ps, lv.pos - p_lo);        // positions of this span
        const int na = cnt * lv.a, i_lo = p_lo * lv.a;    // its anchors: [i_lo, i_lo + na) of the level
        const int64_t row0 = (int64_t)b * L.n_total + lv.row_off + i_lo;
        float* tile = tile_s + (GRAD ? wave * BL::kTile : 0);
        unsigned short* stack = stack_s + wave * BL::kStack;
        if (GRAD) {   // the span's slice of the gradient: zeros first
            const int used = lv.a * DIM * lv.ps;          // <= kTile, a multiple of 4
            for (int e = lane * 4; e < used; e += 256) *reinterpret_cast<float4*>(tile + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        // the rows that take part, in anchor order
        int top = 0;
        for (int s0 = 0; s0 < na; s0 += 64) {
            const int s = s0 + lane;
            const bool live = s < na && sph2pob::element_weight<DIM>(weight, wd, row0 + (s < na ? s : 0)) != 0.0f;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(live);
            if (live) stack[top + rank_below(m)] = (unsigned short)s;
            top += __popcll(m);
        }
        wave_lds_fence();
        const float k0 = GRAD ? BL::effective_scale(scale, avg_factor) : 0.0f;
        for (int base = 0; base < top; base += 64) {
            const int j = base + lane;
            if (j < top) {
                const int s = stack[j];
                const float w = sph2pob::element_weight<DIM>(weight, wd, row0 + s);
                float p[5], d[5], t[5], box[5], jac[5], gx[5], gy[5];
                int64_t stride;
                const int64_t off = BL::delta_offset(lv, DIM, b, i_lo + s, &stride);
                const float* ap = anchors + (lv.row_off + i_lo + s) * DIM;
                const float* tp = targets + (row0 + s) * DIM;
#pragma unroll
                for (int k = 0; k < 5; k++) {
                    p[k] = k < DIM ? ap[k] : 0.0f;
                    d[k] = k < DIM ? lv.pred[off + k * stride] : 0.0f;
                    t[k] = k < DIM ? tp[k] : 0.0f;
                    box[k] = 0.0f;
                }
                CD::decode_one<DIM, GRAD>(p, d, nm, max_ratio, cflags, ctr_clamp, box, GRAD ? jac : nullptr);
                const float lo = sph2pob::pair_loss<DIM, GRAD, FAST>(box, t, loss_mode, eps, nullptr, gx, gy);
                acc += (double)(lo * w);
                if (GRAD) {
                    const float g = k0 * w;
                    if (lv.hw > 0) {
                        const int pp = s / lv.a, aa = s - pp * lv.a;
#pragma unroll
                        for (int k = 0; k < DIM; k++) tile[(aa * DIM + k) * lv.ps + pp] = (g * gx[k]) * jac[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < DIM; k++) tile[s * DIM + k] = (g * gx[k]) * jac[k];
                    }
                }
            }
        }
        if (GRAD) {
            wave_lds_fence();
            // the tile is `rows` rows of `len` floats: NCHW — one row per channel, the span's positions; flat — one row
            const int rows = lv.hw > 0 ? lv.a * DIM : 1;
            const int len = lv.hw > 0 ? cnt : cnt * DIM;
            const int lstride = lv.hw > 0 ? lv.ps : 0;
            const int64_t gstride = lv.hw > 0 ? lv.hw : 0;
            float* g0 = lv.grad + (lv.hw > 0 ? (int64_t)b * lv.a * DIM * lv.hw + p_lo : ((int64_t)b * lv.n + i_lo) * DIM);
            if (lv.vec) {   // workgroup-uniform; len, lstride, gstride and g0 are multiples of 4 floats
                const int q4 = len >> 2, total = rows * q4;
                for (int e = lane; e < total; e += 64) {
                    const int r = e / q4, q = e - r * q4;
                    *reinterpret_cast<float4*>(g0 + r * gstride + 4 * q) = *reinterpret_cast<const float4*>(tile + r * lstride + 4 * q);
                }
            } else {
                const int total = rows * len;
                for (int e = lane; e < total; e += 64) {
                    const int r = e / len, q = e - r * len;
                    g0[r * gstride + q] = tile[r * lstride + q];
                }
            }
        }
    }
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// out[0] = scale_eff * (partials added in a fixed order): thread t adds partials t, t + 256, ... in turn, then the tree
__global__ __launch_bounds__(kBlock) void bbox_final_kernel(const double* __restrict__ partial, int nb, float scale,
                                                            const float* __restrict__ avg_factor, float* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += kBlock) acc += partial[i];
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) out[0] = (float)(r * (double)BL::effective_scale(scale, avg_factor));
}

template <int DIM, bool FAST, bool GRAD>
void launch(const BL::Levels& L, const float* anchors, const float* targets, const float* weight, int wd, const CD::Norm& nm,
            float max_ratio, int cflags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
            double* partial, hipStream_t s) {
    hipLaunchKernelGGL((bbox_loss_kernel<DIM, FAST, GRAD>), dim3(L.blocks), dim3(kBlock), 0, s, L, anchors, targets, weight, wd, nm,
                       max_ratio, cflags, ctr_clamp, loss_mode, eps, scale, avg_factor, partial);
}

}  // namespace

extern "C" {

int64_t sph2pob_bbox_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                          int box_dim) {
    return 8 * BL::workspace_doubles(level_n, level_hw, num_levels, num_images, box_dim);
}

int sph2pob_bbox_loss_sum_f32(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                              int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                              const float* weight, int weight_dim, const float* means_host, const float* stds_host, float max_ratio,
                              int coder_flags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
                              float* out, void* workspace, void* stream) {
    if (int rc = BL::check_options(box_dim, weight, weight_dim, max_ratio, coder_flags, loss_mode)) return rc;
    BL::Levels L;
    if (int rc = BL::make_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, true, &L)) return rc;
    if (!out || !workspace || (L.rows > 0 && (!anchors || !targets))) return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const CD::Norm nm = CD::make_norm(means_host, stds_host, box_dim);
    double* partial = (double*)workspace;
    const int mode = loss_mode & 0xff;
    if (L.blocks > 0) {
        const bool fast = !(loss_mode & SPH2POB_FLAG_REFERENCE_ORDER);
        auto go = [&](auto dim, auto fa, auto gr) {
            launch<decltype(dim)::value, decltype(fa)::value, decltype(gr)::value>(L, anchors, targets, weight, weight_dim, nm, max_ratio,
                                                                                   coder_flags, ctr_clamp, mode, eps, scale, avg_factor,
                                                                                   partial, s);
        };
        auto by_grad = [&](auto dim, auto fa) {
            if (grads) go(dim, fa, std::true_type{});
            else go(dim, fa, std::false_type{});
        };
        auto by_fast = [&](auto dim) {
            if (fast) by_grad(dim, std::true_type{});
            else by_grad(dim, std::false_type{});
        };
        if (box_dim == 4) by_fast(std::integral_constant<int, 4>{});
        else by_fast(std::integral_constant<int, 5>{});
    }
    hipLaunchKernelGGL(bbox_final_kernel, dim3(1), dim3(kBlock), 0, s, partial, L.blocks, scale, avg_factor, out);
    return launch_status();
}

}  // extern "C"
