// Fused box-regression loss kernels (level table and checks: sph2pob_bbox_loss.hpp; the span scheme: sph2pob_span_loss.hpp).
//   bbox_loss_kernel   decoded_span_loss with pair_loss: a row takes part when its mean weight is not zero; a live row runs
//                      gather -> decode -> loss + adjoint -> decode adjoint.  (The loss kernels of sph2pob_loss.hip skip per wave
//                      of 64 rows; here the rule is per row.)
//   head_final_kernel  (sph2pob_head_loss.hpp) adds the partials in a fixed order
#include "sph2pob_span_loss.hpp"

namespace {

namespace BL = sph2pob_bbox;
namespace CD = sph2pob_coder;

// waves per SIMD the kernel is compiled for: decode + loss + both adjoints + the gather / tile addressing take 144 - 152 VGPRs in
// the gradient instantiations (70 - 88 forward only), no scratch: three waves of 170 registers per SIMD.  The LDS (tile + stack:
// 26 KiB per workgroup) would admit six workgroups per CU
constexpr int kBboxWaves = 3;

// T: the element type of the levels (float, or the 16-bit types of sph2pob_bbox_loss_sum_h16); gs: the upstream gradient (16-bit T)
template <class T, int DIM, bool FAST, bool GRAD>
__device__ __forceinline__ void bbox_loss_body(const BL::Levels& L, const float* __restrict__ anchors, const float* __restrict__ targets,
                                               const float* __restrict__ weight, int wd, const CD::Norm& nm, float max_ratio, int cflags,
                                               float ctr_clamp, int loss_mode, float eps, float scale, const float* __restrict__ avg_factor,
                                               float gs, double* __restrict__ partial) {
    decoded_span_loss<T, DIM, GRAD>(L, anchors, targets, weight, wd, nm, max_ratio, cflags, ctr_clamp, scale, avg_factor, gs, partial,
                                    [&](const float (&box)[5], const float (&t)[5], float (&gx)[5], float (&gy)[5]) {
                                        return sph2pob::pair_loss<DIM, GRAD, FAST>(box, t, loss_mode, eps, nullptr, gx, gy);
                                    });
}

template <int DIM, bool FAST, bool GRAD>
__global__ __launch_bounds__(kBlock, kBboxWaves) void bbox_loss_kernel(BL::Levels L, const float* __restrict__ anchors,
                                                                       const float* __restrict__ targets, const float* __restrict__ weight,
                                                                       int wd, CD::Norm nm, float max_ratio, int cflags, float ctr_clamp,
                                                                       int loss_mode, float eps, float scale,
                                                                       const float* __restrict__ avg_factor, double* __restrict__ partial) {
    bbox_loss_body<float, DIM, FAST, GRAD>(L, anchors, targets, weight, wd, nm, max_ratio, cflags, ctr_clamp, loss_mode, eps, scale, avg_factor,
                                           1.0f, partial);
}

// 16-bit levels: the gradient leaves as RNE_T(g ((gw gx) jac)); partial NULL: a gradient-only call, no sum
template <class T, int DIM, bool FAST, bool GRAD>
__global__ __launch_bounds__(kBlock, kBboxWaves) void bbox_loss_h16_kernel(BL::Levels L, const float* __restrict__ anchors,
                                                                           const float* __restrict__ targets, const float* __restrict__ weight,
                                                                           int wd, CD::Norm nm, float max_ratio, int cflags, float ctr_clamp,
                                                                           int loss_mode, float eps, float scale,
                                                                           const float* __restrict__ avg_factor, const float* __restrict__ grad_out,
                                                                           int skip_if_one, double* __restrict__ partial) {
    bool done;
    const float gs = upstream_gradient(grad_out, skip_if_one, done);
    if (done) return;   // kernel-uniform
    bbox_loss_body<T, DIM, FAST, GRAD>(L, anchors, targets, weight, wd, nm, max_ratio, cflags, ctr_clamp, loss_mode, eps, scale, avg_factor, gs,
                                       partial);
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
        by_dim_grad(box_dim, grads != nullptr, [&](auto dim, auto gr) {
            constexpr int D = decltype(dim)::value;
            constexpr bool G = decltype(gr)::value;
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(kBlock), 0, s, L, anchors, targets, weight, weight_dim, nm, max_ratio, coder_flags,
                                   ctr_clamp, mode, eps, scale, avg_factor, partial);
            };
            if (fast) go(bbox_loss_kernel<D, true, G>);
            else go(bbox_loss_kernel<D, false, G>);
        });
    }
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

int sph2pob_bbox_loss_sum_h16(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                              int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                              const float* weight, int weight_dim, const float* means_host, const float* stds_host, float max_ratio,
                              int coder_flags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
                              float* out, void* workspace, const float* grad_out, int skip_if_one, int dtype, void* stream) {
    if (!sph2pob_head::h16_dtype_ok(dtype)) return SPH2POB_ERR_OPTION;
    if (int rc = BL::check_options(box_dim, weight, weight_dim, max_ratio, coder_flags, loss_mode)) return rc;
    BL::Levels L;
    if (int rc = BL::make_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, true, &L, 8)) return rc;
    if ((out && !workspace) || (L.rows > 0 && (!anchors || !targets))) return SPH2POB_ERR_NULL;
    if (!out && !grads) return SPH2POB_OK;   // neither the sum nor the gradient is asked for
    hipStream_t s = (hipStream_t)stream;
    const CD::Norm nm = CD::make_norm(means_host, stds_host, box_dim);
    double* partial = out ? (double*)workspace : nullptr;
    const int mode = loss_mode & 0xff;
    if (L.blocks > 0) {
        const bool fast = !(loss_mode & SPH2POB_FLAG_REFERENCE_ORDER);
        by_dtype_dim_grad(dtype, box_dim, grads != nullptr, [&](auto t, auto dim, auto gr) {
            using T = decltype(t);
            constexpr int D = decltype(dim)::value;
            constexpr bool G = decltype(gr)::value;
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(kBlock), 0, s, L, anchors, targets, weight, weight_dim, nm, max_ratio, coder_flags,
                                   ctr_clamp, mode, eps, scale, avg_factor, grads ? grad_out : nullptr, skip_if_one, partial);
            };
            if (fast) go(bbox_loss_h16_kernel<T, D, true, G>);
            else go(bbox_loss_h16_kernel<T, D, false, G>);
        });
    }
    if (!out) return L.blocks > 0 ? launch_status() : SPH2POB_OK;
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

}  // extern "C"
