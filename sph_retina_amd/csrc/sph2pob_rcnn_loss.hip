// Fused box loss of the R-CNN head on its per-class deltas (shape, row rule and checks: sph2pob_rcnn_loss.hpp).
//   rcnn_delta_loss_kernel  L1 / SmoothL1 on the encoded deltas: a row takes part when its label is a class and ANY of its weights
//                           is not zero; a live row runs sph2pob_delta::element per component of the label's slot.
//   rcnn_bbox_loss_kernel   decode + IoU-family loss: label a class and mean weight not zero; a live row runs decode_one ->
//                           pair_loss -> decode Jacobian on the label's slot and the row's roi.
//   head_final_kernel       (sph2pob_head_loss.hpp) adds the partials in a fixed order
// The walk (rcnn_run) is a sibling of span_loss (sph2pob_span_loss.hpp), which is left untouched: there a wave's gradient tile in
// LDS is as large as its slice of the head's tensor, which cannot hold rows of up to 20 480 floats.  Here a wave owns kRun
// consecutive rows, ONE lane per row: the lane reads the label, then the weight, and evaluates the row if it takes part — a run is
// at most 64 rows, so scan and evaluation are one pass and there is nothing to compact.  Per row only the slot index and the dim
// gradient values go to wave-private LDS; the wave then streams its rows' contiguous cnt * W floats out once — zeros, and a row's
// values where the element lies in the row's slot — every element stored by exactly one lane, in 16-byte stores when the gradient's
// base is 16-byte aligned and W % 4 == 0 (a float4 never crosses a row then; with dim 4 it is all zeros or a whole slot, with dim
// 5 it may straddle a slot edge and is built per element), one element at a time otherwise.  No zeroing launch, no atomics.
#include "sph2pob_kernels_common.hpp"
#include "sph2pob_rcnn_loss.hpp"

namespace {

namespace RL = sph2pob_rcnn_loss;
namespace DL = sph2pob_delta;
namespace CD = sph2pob_coder;

static_assert(kBlock == 64 * RL::kWaves, "one run per wave");

// waves per SIMD of the decoded kernel: the register budget of bbox_loss_kernel (sph2pob_bbox_loss.hip), whose row body this is
constexpr int kBboxWaves = 3;

// live(row, slot) -> bool: does row `row`, whose label selects `slot` >= 0, take part (the family's weight rule).
// eval(row, slot, k0, g, acc): one live row — adds the row's weighted losses to `acc` in component order and, under GRAD, leaves
// the DIM gradient values in g.
template <int DIM, bool GRAD, class Live, class Eval>
__device__ __forceinline__ void rcnn_run(const RL::Shape& sh, const int64_t* __restrict__ labels, float* __restrict__ grad, float scale,
                                         const float* __restrict__ avg_factor, double* __restrict__ partial, Live live, Eval eval) {
    __shared__ __attribute__((aligned(16))) float g_s[GRAD ? RL::kWaves * RL::kRun * DIM : 4];
    __shared__ int slot_s[RL::kWaves * RL::kRun];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int row_lo = ((int)blockIdx.x * RL::kWaves + wave) * RL::kRun;   // < rows + kWaves * kRun: no overflow
    const int cnt = min(RL::kRun, sh.rows - row_lo);                       // rows of this run; <= 0 for the waves past the end
    float* gw = g_s + (GRAD ? wave * RL::kRun * DIM : 0);
    int* sw = slot_s + wave * RL::kRun;
    double acc = 0.0;
    if (lane < cnt) {
        const int row = row_lo + lane;
        int slot = RL::slot_of(labels[row], sh.classes, sh.slots);
        if (slot >= 0 && !live((int64_t)row, slot)) slot = -1;
        float g[DIM];
        if (slot >= 0) {
            const float k0 = GRAD ? RL::effective_scale(scale, avg_factor) : 0.0f;
            eval((int64_t)row, slot, k0, g, acc);
        }
        if (GRAD) {
            sw[lane] = slot;
            if (slot >= 0) {
#pragma unroll
                for (int k = 0; k < DIM; k++) gw[lane * DIM + k] = g[k];
            }
        }
    }
    if (GRAD && cnt > 0) {   // wave-uniform
        wave_lds_fence();
        const int w = sh.w;
        float* g0 = grad + (int64_t)row_lo * w;
        const int total = cnt * w;   // <= kRun * kMaxRowFloats
        if (sh.vec) {                // kernel-uniform; g0 is 16-byte aligned and every row starts on a multiple of 4 floats
            for (int e = lane * 4; e < total; e += 256) {
                const int r = e / w, c = e - r * w;
                const int slot = sw[r];
                float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                if (DIM == 4) {
                    if ((c >> 2) == slot) v = *reinterpret_cast<const float4*>(gw + r * 4);
                } else {
                    const int lo = slot * DIM;   // the slot is columns [lo, lo + DIM); slot -1: none
                    float x[4];
#pragma unroll
                    for (int q = 0; q < 4; q++) {
                        const int k = c + q - lo;
                        x[q] = (slot >= 0 && k >= 0 && k < DIM) ? gw[r * DIM + k] : 0.0f;
                    }
                    v = make_float4(x[0], x[1], x[2], x[3]);
                }
                *reinterpret_cast<float4*>(g0 + e) = v;
            }
        } else {
            for (int e = lane; e < total; e += 64) {
                const int r = e / w, c = e - r * w;
                const int slot = sw[r], k = c - slot * DIM;
                g0[e] = (slot >= 0 && k >= 0 && k < DIM) ? gw[r * DIM + k] : 0.0f;
            }
        }
    }
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

template <int DIM, bool GRAD>
__global__ __launch_bounds__(kBlock) void rcnn_delta_loss_kernel(RL::Shape sh, const float* __restrict__ pred, float* __restrict__ grad,
                                                                 const int64_t* __restrict__ labels, const float* __restrict__ targets,
                                                                 const float* __restrict__ weight, int wd, float beta, float scale,
                                                                 const float* __restrict__ avg_factor, double* __restrict__ partial) {
    rcnn_run<DIM, GRAD>(
        sh, labels, grad, scale, avg_factor, partial,
        [&](int64_t row, int) {
            float wk[DIM];
            return DL::row_weights<DIM>(weight, wd, false, row, wk);
        },
        [&](int64_t row, int slot, float k0, float (&g)[DIM], double& acc) {
            float wk[DIM], d[DIM], t[DIM];
            DL::row_weights<DIM>(weight, wd, false, row, wk);
            const float* dp = pred + row * sh.w + slot * DIM;
            const float* tp = targets + row * DIM;
#pragma unroll
            for (int k = 0; k < DIM; k++) d[k] = dp[k];
#pragma unroll
            for (int k = 0; k < DIM; k++) t[k] = tp[k];
#pragma unroll
            for (int k = 0; k < DIM; k++) {
                float lo, sk;
                DL::element(d[k], t[k], beta, lo, sk);
                acc += (double)(lo * wk[k]);
                if (GRAD) g[k] = (k0 * wk[k]) * sk;
            }
        });
}

template <int DIM, bool FAST, bool GRAD>
__global__ __launch_bounds__(kBlock, kBboxWaves) void rcnn_bbox_loss_kernel(RL::Shape sh, const float* __restrict__ pred, float* __restrict__ grad,
                                                                            const int64_t* __restrict__ labels, const float* __restrict__ rois,
                                                                            int64_t roi_stride, int64_t roi_offset,
                                                                            const float* __restrict__ targets, const float* __restrict__ weight,
                                                                            int wd, CD::Norm nm, float max_ratio, int cflags, float ctr_clamp,
                                                                            int loss_mode, float eps, float scale,
                                                                            const float* __restrict__ avg_factor, double* __restrict__ partial) {
    rcnn_run<DIM, GRAD>(
        sh, labels, grad, scale, avg_factor, partial,
        [&](int64_t row, int) { return sph2pob::element_weight<DIM>(weight, wd, row) != 0.0f; },
        [&](int64_t row, int slot, float k0, float (&g)[DIM], double& acc) {
            const float w = sph2pob::element_weight<DIM>(weight, wd, row);
            float p[5], d[5], t[5], box[5], jac[5], gx[5], gy[5];
            const float* ap = rois + row * roi_stride + roi_offset;
            const float* dp = pred + row * sh.w + slot * DIM;
            const float* tp = targets + row * DIM;
#pragma unroll
            for (int k = 0; k < 5; k++) {
                p[k] = k < DIM ? ap[k] : 0.0f;
                d[k] = k < DIM ? dp[k] : 0.0f;
                t[k] = k < DIM ? tp[k] : 0.0f;
                box[k] = 0.0f;
            }
            CD::decode_one<DIM, GRAD>(p, d, nm, max_ratio, cflags, ctr_clamp, box, GRAD ? jac : nullptr);
            const float lo = sph2pob::pair_loss<DIM, GRAD, FAST>(box, t, loss_mode, eps, nullptr, gx, gy);
            acc += (double)(lo * w);
            if (GRAD) {
                const float gw = k0 * w;
#pragma unroll
                for (int k = 0; k < DIM; k++) g[k] = (gw * gx[k]) * jac[k];
            }
        });
}

// f(integral_constant<int, DIM>, bool_constant<GRAD>) for the box_dim (4 | 5) and the gradient request of a call
template <class F>
void by_dim_grad(int box_dim, bool grad, F&& f) {
    auto by_grad = [&](auto dim) {
        if (grad) f(dim, std::true_type{});
        else f(dim, std::false_type{});
    };
    if (box_dim == 4) by_grad(std::integral_constant<int, 4>{});
    else by_grad(std::integral_constant<int, 5>{});
}

}  // namespace

extern "C" {

int64_t sph2pob_rcnn_loss_workspace_bytes(int64_t rows, int64_t num_slots, int box_dim) {
    return 8 * RL::workspace_doubles(rows, num_slots, box_dim);
}

int sph2pob_rcnn_delta_loss_sum_f32(const float* bbox_pred, float* grad, int64_t rows, int64_t num_slots, int64_t num_classes, int box_dim,
                                    const int64_t* labels, const float* targets, const float* weight, int weight_dim, float beta,
                                    float scale, const float* avg_factor, float* out, void* workspace, void* stream) {
    if (int rc = DL::check_options(box_dim, weight, weight_dim, beta)) return rc;
    RL::Shape sh;
    if (int rc = RL::make_shape(rows, num_slots, num_classes, box_dim, &sh)) return rc;
    if (int rc = RL::check_tensors(sh, bbox_pred, labels, targets, false, nullptr, 0, 0, box_dim, out, workspace)) return rc;
    sh.vec = grad && RL::aligned16(grad) && sh.w % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    double* partial = (double*)workspace;
    if (sh.blocks > 0) {
        const int wd = weight ? weight_dim : 0;
        by_dim_grad(box_dim, grad != nullptr, [&](auto dim, auto gr) {
            hipLaunchKernelGGL((rcnn_delta_loss_kernel<decltype(dim)::value, decltype(gr)::value>), dim3(sh.blocks), dim3(kBlock), 0, s, sh,
                               bbox_pred, grad, labels, targets, weight, wd, beta, scale, avg_factor, partial);
        });
    }
    return launch_final(partial, sh.blocks, scale, avg_factor, out, s);
}

int sph2pob_rcnn_bbox_loss_sum_f32(const float* bbox_pred, float* grad, int64_t rows, int64_t num_slots, int64_t num_classes, int box_dim,
                                   const int64_t* labels, const float* rois, int64_t roi_stride, int64_t roi_offset, const float* targets,
                                   const float* weight, int weight_dim, const float* means_host, const float* stds_host, float max_ratio,
                                   int coder_flags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
                                   float* out, void* workspace, void* stream) {
    if (int rc = sph2pob_bbox::check_options(box_dim, weight, weight_dim, max_ratio, coder_flags, loss_mode)) return rc;
    RL::Shape sh;
    if (int rc = RL::make_shape(rows, num_slots, num_classes, box_dim, &sh)) return rc;
    if (int rc = RL::check_tensors(sh, bbox_pred, labels, targets, true, rois, roi_stride, roi_offset, box_dim, out, workspace)) return rc;
    sh.vec = grad && RL::aligned16(grad) && sh.w % 4 == 0;
    hipStream_t s = (hipStream_t)stream;
    const CD::Norm nm = CD::make_norm(means_host, stds_host, box_dim);
    double* partial = (double*)workspace;
    const int mode = loss_mode & 0xff;
    if (sh.blocks > 0) {
        const bool fast = !(loss_mode & SPH2POB_FLAG_REFERENCE_ORDER);
        by_dim_grad(box_dim, grad != nullptr, [&](auto dim, auto gr) {
            constexpr int D = decltype(dim)::value;
            constexpr bool G = decltype(gr)::value;
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(sh.blocks), dim3(kBlock), 0, s, sh, bbox_pred, grad, labels, rois, roi_stride, roi_offset, targets,
                                   weight, weight_dim, nm, max_ratio, coder_flags, ctr_clamp, mode, eps, scale, avg_factor, partial);
            };
            if (fast) go(rcnn_bbox_loss_kernel<D, true, G>);
            else go(rcnn_bbox_loss_kernel<D, false, G>);
        });
    }
    return launch_final(partial, sh.blocks, scale, avg_factor, out, s);
}

}  // extern "C"
