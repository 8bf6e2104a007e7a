// Fused L1 / SmoothL1 box loss on the head's encoded deltas (element function and checks: sph2pob_delta_loss.hpp; level table:
// sph2pob_bbox_loss.hpp; the span scheme: sph2pob_span_loss.hpp).
//   delta_loss_kernel  a row takes part when ANY of its weights is not zero — a (B, n, 4) weight row is one 16-byte load; a live
//                      row gathers its dim deltas (stride H W in NCHW), targets and weights and runs one element function per
//                      component.
//   head_final_kernel  (sph2pob_head_loss.hpp) adds the partials in a fixed order
// There is next to no arithmetic: the kernel is bound by the weight scan and the tile stream-out, so nothing caps the waves per
// SIMD below what the LDS (tile + stack: 25 920 B per workgroup, six workgroups per CU) admits.
#include "sph2pob_span_loss.hpp"
#include "sph2pob_delta_loss.hpp"

namespace {

namespace BL = sph2pob_bbox;
namespace DL = sph2pob_delta;

// vec: bit 0 — a (B, n, 4) weight row is one aligned 16-byte load; bit 1 — so is a target row
// T: the element type of the levels (float, or the 16-bit types of sph2pob_delta_loss_sum_h16); gs: the upstream gradient (16-bit T)
template <class T, int DIM, bool GRAD>
__device__ __forceinline__ void delta_loss_body(const BL::Levels& L, const float* __restrict__ targets, const float* __restrict__ weight,
                                                int wd, int vec, float beta, float scale, const float* __restrict__ avg_factor, float gs,
                                                double* __restrict__ partial) {
    const bool wvec = (vec & 1) != 0, tvec = (vec & 2) != 0;
    span_loss<T, DIM, GRAD>(
        L, scale, avg_factor, gs, partial,
        [&](int64_t row) {
            float wk[DIM];
            return DL::row_weights<DIM>(weight, wd, wvec, row, wk);
        },
        [&](const BL::Level& lv, int b, int i, int64_t row, float k0, float (&g)[DIM], double& acc) {
            float wk[DIM], d[DIM], t[DIM];
            DL::row_weights<DIM>(weight, wd, wvec, row, wk);
            int64_t stride;
            const int64_t off = DL::delta_offset(lv, DIM, b, i, &stride);
            const float* tp = targets + row * DIM;
            const T* dp = level_ptr<T>(lv.pred) + off;
#pragma unroll
            for (int k = 0; k < DIM; k++) d[k] = load1(dp + k * stride);
            if (DIM == 4 && tvec) {
                const float4 v = *reinterpret_cast<const float4*>(tp);
                t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
            } else {
#pragma unroll
                for (int k = 0; k < DIM; k++) t[k] = tp[k];
            }
#pragma unroll
            for (int k = 0; k < DIM; k++) {
                float lo, sk;
                DL::element(d[k], t[k], beta, lo, sk);
                acc += (double)(lo * wk[k]);
                if (GRAD) g[k] = (k0 * wk[k]) * sk;
            }
        });
}

template <int DIM, bool GRAD>
__global__ __launch_bounds__(kBlock) void delta_loss_kernel(BL::Levels L, const float* __restrict__ targets,
                                                            const float* __restrict__ weight, int wd, int vec, float beta, float scale,
                                                            const float* __restrict__ avg_factor, double* __restrict__ partial) {
    delta_loss_body<float, DIM, GRAD>(L, targets, weight, wd, vec, beta, scale, avg_factor, 1.0f, partial);
}

// 16-bit levels: the gradient leaves as RNE_T(g ((k0 w_k) s_k)); partial NULL: a gradient-only call, no sum
template <class T, int DIM, bool GRAD>
__global__ __launch_bounds__(kBlock) void delta_loss_h16_kernel(BL::Levels L, const float* __restrict__ targets,
                                                                const float* __restrict__ weight, int wd, int vec, float beta, float scale,
                                                                const float* __restrict__ avg_factor, const float* __restrict__ grad_out,
                                                                int skip_if_one, double* __restrict__ partial) {
    bool done;
    const float gs = upstream_gradient(grad_out, skip_if_one, done);
    if (done) return;   // kernel-uniform
    delta_loss_body<T, DIM, GRAD>(L, targets, weight, wd, vec, beta, scale, avg_factor, gs, partial);
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
        by_dim_grad(box_dim, grads != nullptr, [&](auto dim, auto gr) {
            hipLaunchKernelGGL((delta_loss_kernel<decltype(dim)::value, decltype(gr)::value>), dim3(L.blocks), dim3(kBlock), 0, s, L, targets,
                               weight, wd, vec, beta, scale, avg_factor, partial);
        });
    }
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

int sph2pob_delta_loss_sum_h16(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int box_dim, const float* targets, const float* weight,
                               int weight_dim, float beta, float scale, const float* avg_factor, float* out, void* workspace,
                               const float* grad_out, int skip_if_one, int dtype, void* stream) {
    if (!sph2pob_head::h16_dtype_ok(dtype)) return SPH2POB_ERR_OPTION;
    if (int rc = DL::check_options(box_dim, weight, weight_dim, beta)) return rc;
    BL::Levels L;
    if (int rc = DL::make_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, true, &L, 8)) return rc;
    if ((out && !workspace) || (L.rows > 0 && !targets)) return SPH2POB_ERR_NULL;
    if (!out && !grads) return SPH2POB_OK;   // neither the sum nor the gradient is asked for
    hipStream_t s = (hipStream_t)stream;
    double* partial = out ? (double*)workspace : nullptr;
    if (L.blocks > 0) {
        const int wd = weight ? weight_dim : 0;
        const int vec = (box_dim == 4 && wd == 4 && BL::aligned16(weight) ? 1 : 0) | (box_dim == 4 && BL::aligned16(targets) ? 2 : 0);
        by_dtype_dim_grad(dtype, box_dim, grads != nullptr, [&](auto t, auto dim, auto gr) {
            hipLaunchKernelGGL((delta_loss_h16_kernel<decltype(t), decltype(dim)::value, decltype(gr)::value>), dim3(L.blocks), dim3(kBlock), 0, s,
                               L, targets, weight, wd, vec, beta, scale, avg_factor, grads ? grad_out : nullptr, skip_if_one, partial);
        });
    }
    if (!out) return L.blocks > 0 ? launch_status() : SPH2POB_OK;
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

}  // extern "C"
