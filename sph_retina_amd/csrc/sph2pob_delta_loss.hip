// Fused L1 / SmoothL1 box loss on the head's encoded deltas (element function and checks: sph2pob_delta_loss.hpp; level table and
// span geometry: sph2pob_bbox_loss.hpp, by inclusion — sph2pob_bbox_loss.hip is not touched, the scan and the stream-out below
// repeat its forty lines).
//   delta_loss_kernel  ONE grid over all images and levels of a head: a workgroup finds its level in the table, each of its four
//                      waves owns one span.  The wave scans the span's weights 64 rows at a time — a (B, n, 4) weight row is one
//                      16-byte load — and pushes the rows with ANY non-zero component on a wave-private LDS stack (ballot /
//                      mbcnt), then runs dense passes of up to 64 live rows: gather the dim deltas (stride H W in NCHW), the targets
//                      and the weights, one element function per component.  The span's gradient slice is assembled in a
//                      wave-private LDS tile — zeros, then the live rows' values — and leaves in one sweep: every element is
//                      stored once, in whole 16-byte stores along w where the level allows it.  The weighted element losses are
//                      added in double per lane, wave and workgroup: one partial per workgroup.
//   delta_final_kernel one workgroup adds the partials in a fixed order (no float atomics: the same bits on every call)
// There is next to no arithmetic: the kernel is bound by the weight scan and the tile stream-out, so nothing caps the waves per
// SIMD below what the LDS (tile + stack: 25 920 B per workgroup, six workgroups per CU) admits.
#include <type_traits>

#include "sph2pob_kernels_common.hpp"
#include "sph2pob_delta_loss.hpp"

namespace {

namespace BL = sph2pob_bbox;
namespace DL = sph2pob_delta;

static_assert(kBlock == 64 * BL::kWaves, "one span per wave");

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

// vec: bit 0 — a (B, n, 4) weight row is one aligned 16-byte load; bit 1 — so is a target row
template <int DIM, bool GRAD>
__global__ __launch_bounds__(kBlock) void delta_loss_kernel(BL::Levels L, const float* __restrict__ targets,
                                                            const float* __restrict__ weight, int wd, int vec, float beta, float scale,
                                                            const float* __restrict__ avg_factor, double* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float tile_s[GRAD ? BL::kWaves * BL::kTile : 4];
    __shared__ unsigned short stack_s[BL::kWaves * BL::kStack];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int l = level_of_block(L, blockIdx.x);
    const BL::Level& lv = L.lv[l];
    const int item = ((int)blockIdx.x - lv.block_off) * BL::kWaves + wave;
    const bool wvec = (vec & 1) != 0, tvec = (vec & 2) != 0;
    double acc = 0.0;
    if (item < lv.items) {   // wave-uniform
        const int b = item / lv.spans, sp = item - b * lv.spans;
        const int p_lo = sp * lv.ps;
        const int cnt = min(lv.ps, lv.pos - p_lo);        // positions of this span
        const int na = cnt * lv.a, i_lo = p_lo * lv.a;    // its anchors: [i_lo, i_lo + na) of the level, na <= kStack
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
            float wk[DIM];
            const bool live = DL::row_weights<DIM>(weight, wd, wvec, row0 + (s < na ? s : 0), wk) && s < na;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(live);
            if (live) stack[top + rank_below(m)] = (unsigned short)s;
            top += __popcll(m);
        }
        wave_lds_fence();
        const float k0 = GRAD ? DL::effective_scale(scale, avg_factor) : 0.0f;
        for (int base = 0; base < top; base += 64) {
            const int j = base + lane;
            if (j < top) {
                const int s = stack[j];
                float wk[DIM], d[DIM], t[DIM];
                DL::row_weights<DIM>(weight, wd, wvec, row0 + s, wk);
                int64_t stride;
                const int64_t off = DL::delta_offset(lv, DIM, b, i_lo + s, &stride);
                const float* tp = targets + (row0 + s) * DIM;
#pragma unroll
                for (int k = 0; k < DIM; k++) d[k] = lv.pred[off + k * stride];
                if (DIM == 4 && tvec) {
                    const float4 v = *reinterpret_cast<const float4*>(tp);
                    t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
                } else {
#pragma unroll
                    for (int k = 0; k < DIM; k++) t[k] = tp[k];
                }
                const int pp = lv.hw > 0 ? s / lv.a : 0, aa = s - pp * lv.a;
#pragma unroll
                for (int k = 0; k < DIM; k++) {
                    float lo, sk;
                    DL::element(d[k], t[k], beta, lo, sk);
                    acc += (double)(lo * wk[k]);
                    if (GRAD) {
                        const float g = (k0 * wk[k]) * sk;
                        if (lv.hw > 0) tile[(aa * DIM + k) * lv.ps + pp] = g;
                        else tile[s * DIM + k] = g;
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
__global__ __launch_bounds__(kBlock) void delta_final_kernel(const double* __restrict__ partial, int nb, float scale,
                                                             const float* __restrict__ avg_factor, float* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += kBlock) acc += partial[i];
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) out[0] = (float)(r * (double)DL::effective_scale(scale, avg_factor));
}

template <int DIM, bool GRAD>
void launch(const BL::Levels& L, const float* targets, const float* weight, int wd, int vec, float beta, float scale,
            const float* avg_factor, double* partial, hipStream_t s) {
    hipLaunchKernelGGL((delta_loss_kernel<DIM, GRAD>), dim3(L.blocks), dim3(kBlock), 0, s, L, targets, weight, wd, vec, beta, scale,
                       avg_factor, partial);
}

}  // namespace

extern "C" {

int64_t sph2pob_delta_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                           int box_dim) {
    return 8 * DL::workspace_doubles(level_n, level_hw, num_levels, num_images, box_dim);
}

int sph2pob_delta_loss_sum_f32(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int box_dim, const float* targets, const float* weight,
                               int weight_dim, float beta, float scale, const float* avg_factor, float* out, void* workspace,
                               void* stream) {
    if (int rc = DL::check_options(box_dim, weight, weight_dim, beta)) return rc;
    BL::Levels L;
    if (int rc = DL::make_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, true, &L)) return rc;
    if (!out || !workspace || (L.rows > 0 && !targets)) return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    if (L.blocks > 0) {
        const int wd = weight ? weight_dim : 0;
        const int vec = (box_dim == 4 && wd == 4 && BL::aligned16(weight) ? 1 : 0) | (box_dim == 4 && BL::aligned16(targets) ? 2 : 0);
        if (box_dim == 4) {
            if (grads) launch<4, true>(L, targets, weight, wd, vec, beta, scale, avg_factor, partial, s);
            else launch<4, false>(L, targets, weight, wd, vec, beta, scale, avg_factor, partial, s);
        } else {
            if (grads) launch<5, true>(L, targets, weight, wd, vec, beta, scale, avg_factor, partial, s);
            else launch<5, false>(L, targets, weight, wd, vec, beta, scale, avg_factor, partial, s);
        }
    }
    hipLaunchKernelGGL(delta_final_kernel, dim3(1), dim3(kBlock), 0, s, partial, L.blocks, scale, avg_factor, out);
    return launch_status();
}

}  // extern "C"
