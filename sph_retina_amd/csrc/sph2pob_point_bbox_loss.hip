// Fused box-regression loss of a point (FCOS) head (checks and the row: sph2pob_point_bbox_loss.hpp; the span scheme:
// sph2pob_span_loss.hpp).
//   point_bbox_loss_kernel  one span_loss instance: a row takes part when its mean weight is not zero; a live row gathers its point,
//                           its distances (stride H W in NCHW) and its target row, decodes both with the point coder, takes loss and
//                           adjoint and runs the decode's backward.  A row of weight 0 is never read.
//   head_final_kernel       (sph2pob_head_loss.hpp) adds the partials in a fixed order
#include "sph2pob_span_loss.hpp"
#include "sph2pob_point_bbox_loss.hpp"

namespace {

namespace BL = sph2pob_bbox;
namespace PT = sph2pob_point;

// waves per SIMD the kernel is compiled for, chosen from the reported registers as kBboxWaves was.  The point decode is lighter than
// the delta decode of bbox_loss_kernel: the gradient instantiations take 124 VGPRs in the default arithmetic and 135 in the
// reference order (65 - 84 forward only), no scratch.  Compiled for four waves (a budget of 128) the reference-order gradient
// instantiations spill 16 bytes per lane, so the bound stays at three; the default-arithmetic ones fit 128 registers as they are
// and run four waves per SIMD all the same.  The LDS (tile + stack: 26 KiB per workgroup) admits six workgroups per CU
constexpr int kPointBboxWaves = 3;

template <int DIM, bool FAST, bool GRAD>
__global__ __launch_bounds__(kBlock, kPointBboxWaves) void point_bbox_loss_kernel(BL::Levels L, const float* __restrict__ points,
                                                                                  const float* __restrict__ targets,
                                                                                  const float* __restrict__ weight, int wd, PT::Image im,
                                                                                  int loss_mode, float eps, float scale,
                                                                                  const float* __restrict__ avg_factor,
                                                                                  double* __restrict__ partial) {
    span_loss<float, DIM, GRAD>(
        L, scale, avg_factor, 1.0f, partial,
        [&](int64_t row) { return sph2pob::element_weight<DIM>(weight, wd, row) != 0.0f; },
        [&](const BL::Level& lv, int b, int i, int64_t row, float k0, float (&g)[DIM], double& acc) {
            const float w = sph2pob::element_weight<DIM>(weight, wd, row);
            float pt[2], d[5], t[5], g5[5];
            int64_t stride;
            const int64_t off = BL::delta_offset(lv, DIM, b, i, &stride);
            const float* pp = points + (lv.row_off + i) * 2;
            const float* tp = targets + row * DIM;
            pt[0] = pp[0]; pt[1] = pp[1];
#pragma unroll
            for (int k = 0; k < 5; k++) {
                d[k] = k < DIM ? lv.pred[off + k * stride] : 0.0f;
                t[k] = k < DIM ? tp[k] : 0.0f;
            }
            const float lo = sph2pob_point_bbox::row_loss<DIM, GRAD, FAST>(pt, d, t, im, loss_mode, eps, k0 * w, g5);
            acc += (double)(lo * w);
            if (GRAD) {
#pragma unroll
                for (int k = 0; k < DIM; k++) g[k] = g5[k];
            }
        });
}

}  // namespace

extern "C" {

int64_t sph2pob_point_bbox_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                                int box_dim) {
    return 8 * BL::workspace_doubles(level_n, level_hw, num_levels, num_images, box_dim);
}

int sph2pob_point_bbox_loss_sum_f32(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                    int num_levels, int64_t num_images, int box_dim, const float* points, const float* targets,
                                    const float* weight, int weight_dim, int64_t img_h, int64_t img_w, float max_h, float max_w,
                                    int loss_mode, float eps, float scale, const float* avg_factor, float* out, void* workspace,
                                    void* stream) {
    BL::Levels L;
    if (int rc = sph2pob_point_bbox::check_and_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, weight, weight_dim,
                                                      img_h, img_w, loss_mode, &L))
        return rc;
    if (!out || !workspace || (L.rows > 0 && (!points || !targets))) return SPH2POB_ERR_NULL;
    if (int rc = sph2pob_point_bbox::check_bounds(max_h, max_w)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const PT::Image im{(float)img_w, (float)img_h, max_w, max_h};
    double* partial = (double*)workspace;
    const int mode = loss_mode & 0xff;
    if (L.blocks > 0) {
        const bool fast = !(loss_mode & SPH2POB_FLAG_REFERENCE_ORDER);
        by_dim_grad(box_dim, grads != nullptr, [&](auto dim, auto gr) {
            constexpr int D = decltype(dim)::value;
            constexpr bool G = decltype(gr)::value;
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(kBlock), 0, s, L, points, targets, weight, weight_dim, im, mode, eps, scale,
                                   avg_factor, partial);
            };
            if (fast) go(point_bbox_loss_kernel<D, true, G>);
            else go(point_bbox_loss_kernel<D, false, G>);
        });
    }
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

}  // extern "C"
