// libsph2pob_host.so — the CPU twins of the C ABI ("CPU twins with the same names suffixed _cpu").
//
// The reference's operators run on CPU tensors as well (tests/test_all_ious.py:88-104 runs every IoU with device='cpu';
// sphdet/iou/sph_iou_calculator.py:107-108 forces unbiased_iou to the CPU; MaxIoUAssigner's gpu_assign_thr moves the
// assignment to the CPU, mmdet/core/bbox/assigners/max_iou_assigner.py:100-110): this library serves those calls from the
// PRODUCT'S OWN arithmetic — the very __host__ __device__ functions of sph2pob_{device,fast,loss,unbiased}.hpp that the
// kernels run, instantiated for the host — on a small thread pool.  It is not the oracle and shares no code with it
// (oracle/ is the checker; tests/test_capi_symbols.py guards the separation).  Results follow the host's libm where the
// device uses ocml: within the fp32 noise documented in DESIGN.md §3, not bit-identical to the kernels.
//
// Every entry point has the signature of its HIP twin (the trailing stream argument is ignored: the call is synchronous) and
// returns the same error codes.
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_device.hpp"
#include "sph2pob_loss.hpp"
#include "sph2pob_fast.hpp"
#include "sph2pob_unbiased.hpp"
#include "sph2pob_iou_entry.hpp"
#include "sph2pob_coder.hpp"
#include "sph2pob_get_bboxes.hpp"
#include "sph2pob_assign.hpp"
#include "sph2pob_focal.hpp"
#include "sph2pob_bbox_loss.hpp"
#include "sph2pob_gauss_bbox_loss.hpp"
#include "sph2pob_delta_loss.hpp"
#include "sph2pob_rcnn_loss.hpp"
#include "sph2pob_softmax.hpp"
#include "sph2pob_sample.hpp"
#include "sph2pob_rcnn_targets.hpp"
#include "sph2pob_rcnn_bboxes.hpp"
#include "sph2pob_point_targets.hpp"
#include "sph2pob_point_bbox_loss.hpp"
#include "sph2pob_bce_loss.hpp"
#include "sph2pob_roi_extract.hpp"

namespace {

using namespace sph2pob;

int cpu_threads() {
    static int n = 0;
    if (n == 0) {
        const char* e = getenv("SPH2POB_CPU_THREADS");
        int v = e ? atoi(e) : 0;
        if (v <= 0) {
            v = (int)std::thread::hardware_concurrency();
            cpu_set_t set;
            if (sched_getaffinity(0, sizeof(set), &set) == 0) v = std::min(v, CPU_COUNT(&set));
        }
        n = std::max(1, std::min(v, 256));
    }
    return n;
}

// f(lo, hi) over [0, n) in contiguous chunks, one per thread; small jobs stay on the caller's thread
template <class F>
void parallel_for(int64_t n, int64_t grain, F&& f) {
    int t = (int)std::min<int64_t>(cpu_threads(), (n + grain - 1) / std::max<int64_t>(grain, 1));
    if (t <= 1) { if (n > 0) f((int64_t)0, n); return; }
    std::vector<std::thread> pool;
    pool.reserve(t - 1);
    const int64_t per = (n + t - 1) / t;
    for (int k = 1; k < t; k++) {
        const int64_t lo = k * per, hi = std::min(n, lo + per);
        if (lo < hi) pool.emplace_back([&f, lo, hi] { f(lo, hi); });
    }
    f((int64_t)0, std::min(n, per));
    for (auto& th : pool) th.join();
}

template <int DIM>
inline void load_box(const float* p, int64_t i, float (&b)[5]) {
    for (int k = 0; k < 5; k++) b[k] = k < DIM ? p[i * DIM + k] : 0.0f;
}

// ---- the IoU / transform family: checks, dispatch(), the per-pair selection and the row bodies are sph2pob_iou_entry.hpp's, as
// the kernels'; here are the loops.  row(e) for every e of [0, total) ----
template <class Row>
int for_rows(int64_t total, int64_t grain, Row&& row) {
    parallel_for(total, grain, [&](int64_t lo, int64_t hi) {
        for (int64_t e = lo; e < hi; e++) row(e);
    });
    return SPH2POB_OK;
}
// aligned (n == 0: out[e] of pair e) or pairwise (out[e] of row e / n and column e % n); the selection is made once per call
struct PairIou {
    const float *b1, *b2; float* out; int64_t total, n; int mode, edge, angle; bool fast = true;
    template <int V, int D> int run() {
        return with_pair_sel<V>(fast, angle, [&](auto variant, auto fast_core) {
            return for_rows(total, 2048, [&](int64_t e) {
                float x[5], y[5];
                load_box<D>(b1, n ? e / n : e, x);
                load_box<D>(b2, n ? e % n : e, y);
                out[e] = pair_iou_sel<decltype(variant)::value, D, decltype(fast_core)::value>(x, y, mode, edge, angle);
            });
        });
    }
};
struct Transform {
    const float *b1, *b2; float *o1, *o2; int64_t n; int edge, angle, jitter; bool fast = true;
    template <int V, int D> int run() {
        if constexpr (V > VARIANT_LEGACY) return SPH2POB_ERR_OPTION;
        else return for_rows(n, 2048, [&](int64_t i) {
            float x[5], y[5];
            load_box<D>(b1, i, x);
            load_box<D>(b2, i, y);
            transform_row<V, D>(x, y, edge, angle, jitter, o1 + i * 5, o2 + i * 5);
        });
    }
};
// the two adjoints (sph2pob_transform_bwd_f32 / _general_f32): the closed form or, DUAL, the dual-number one
template <bool DUAL>
struct TransformBwd {
    const float *b1, *b2, *g1, *g2; float *gb1, *gb2; int64_t n; int edge, angle, jitter; bool fast = true;
    template <int V, int D> int run() {
        if constexpr (V > (DUAL ? VARIANT_LEGACY : VARIANT_EFFICIENT)) return SPH2POB_ERR_OPTION;
        else return for_rows(n, DUAL ? 512 : 1024, [&](int64_t i) {
            float x[5], y[5];
            load_box<D>(b1, i, x);
            load_box<D>(b2, i, y);
            transform_bwd_row<V, D, DUAL>(x, y, g1 + i * 5, g2 + i * 5, edge, angle, jitter, gb1 + i * D, gb2 + i * D);
        });
    }
};

// ---- loss: the checks, element_weight and the per-pair bodies are sph2pob_loss.hpp's, as the kernels' ----
// one pass over the pairs: loss element (times w), IoU, gradients (times g) as asked for; returns the sum of the elements
template <int DIM, bool FAST, class Body>
double loss_pass(const Body& body, const float* pred, const float* target, const float* weight, int wd, float scale,
                 const float* grad_out, int grad_stride, float* loss, float* iou, float* gpred, float* gtarget, int64_t n) {
    const int t = cpu_threads();
    std::vector<double> partial((size_t)t + 1, 0.0);
    const int64_t per = (n + t - 1) / std::max(t, 1);
    parallel_for(n, 1024, [&](int64_t lo, int64_t hi) {
        double acc = 0.0;
        for (int64_t i = lo; i < hi; i++) {
            float x[5], y[5], gx[5], gy[5], io = 0.0f;
            const float w = scale * element_weight<DIM>(weight, wd, i);
            const float g = grad_out ? grad_out[i * grad_stride] * w : w;
            load_box<DIM>(pred, i, x);
            load_box<DIM>(target, i, y);
            const bool need_grad = gpred || gtarget;
            const float l = need_grad ? body.template eval<DIM, true, FAST>(x, y, &io, gx, gy)
                                      : body.template eval<DIM, false, FAST>(x, y, &io, gx, gy);
            const float lw = w == 0.0f ? 0.0f : l * w;   // the kernels skip all-zero-weight waves: a zero weight gives exact zeros
            if (loss) loss[i] = lw;
            if (iou) iou[i] = io;
            acc += lw;
            for (int k = 0; k < DIM; k++) {
                if (gpred) gpred[i * DIM + k] = g == 0.0f ? 0.0f : g * gx[k];
                if (gtarget) gtarget[i * DIM + k] = g == 0.0f ? 0.0f : g * gy[k];
            }
        }
        partial[(size_t)std::min<int64_t>(lo / std::max<int64_t>(per, 1), t)] += acc;
    });
    double s = 0.0;
    for (double v : partial) s += v;   // fixed order: reproducible for a given thread count
    return s;
}

// (box_dim, flags) select loss_pass<DIM, FAST> as they select the kernel
template <class Body, class... A>
double loss_pass_sel(const Body& body, int box_dim, int flags, A... a) {
    const bool fast = !(flags & SPH2POB_FLAG_REFERENCE_ORDER);
    if (box_dim == 4) return fast ? loss_pass<4, true>(body, a...) : loss_pass<4, false>(body, a...);
    return fast ? loss_pass<5, true>(body, a...) : loss_pass<5, false>(body, a...);
}

// the four forms of both families after the entry point's argument check (sph2pob_loss.hip: launch_fwd ...), each with
// its form's null-pointer and n == 0 rules
template <class Body>
int cpu_fwd(const float* pred, const float* target, const float* weight, int wd, float scale, float* loss, float* iou,
            int64_t n, int box_dim, int flags, const Body& body) {
    if (n == 0) return SPH2POB_OK;
    if (!pred || !target || !loss) return SPH2POB_ERR_NULL;
    loss_pass_sel(body, box_dim, flags, pred, target, weight, wd, scale, nullptr, 0, loss, iou, nullptr, nullptr, n);
    return SPH2POB_OK;
}

template <class Body>
int cpu_bwd(const float* pred, const float* target, const float* weight, int wd, const float* grad_out, int grad_stride,
            float scale, float* grad_pred, float* grad_target, int64_t n, int box_dim, int flags, const Body& body) {
    if (n == 0) return SPH2POB_OK;
    if (!pred || !target || !grad_out || !grad_pred) return SPH2POB_ERR_NULL;
    loss_pass_sel(body, box_dim, flags, pred, target, weight, wd, scale, grad_out, grad_stride, nullptr, nullptr, grad_pred,
                  grad_target, n);
    return SPH2POB_OK;
}

// (no workspace on the host; the elements are summed unscaled and the scale applied once, as the HIP form does)
template <class Body>
int cpu_fwd_sum(const float* pred, const float* target, const float* weight, int wd, float scale, float* out, int64_t n,
                int box_dim, int flags, const Body& body) {
    if (!out || (n > 0 && (!pred || !target))) return SPH2POB_ERR_NULL;
    const double s = n ? loss_pass_sel(body, box_dim, flags, pred, target, weight, wd, 1.0f, nullptr, 0, nullptr, nullptr,
                                       nullptr, nullptr, n)
                       : 0.0;
    out[0] = (float)(s * (double)scale);
    return SPH2POB_OK;
}

template <class Body>
int cpu_fwd_grad(const float* pred, const float* target, const float* weight, int wd, float scale, float* loss, float* out_sum,
                 float* grad_pred, float* grad_target, int64_t n, int box_dim, int flags, const Body& body) {
    if (n > 0 && (!pred || !target || !grad_pred)) return SPH2POB_ERR_NULL;
    const double s = n ? loss_pass_sel(body, box_dim, flags, pred, target, weight, wd, scale, nullptr, 0, loss, nullptr,
                                       grad_pred, grad_target, n)
                       : 0.0;
    if (out_sum) out_sum[0] = (float)s;
    return SPH2POB_OK;
}

// greedy NMS per class segment (sph2pob_nms_segmented_f32)
struct NmsRun {
    const float* boxes; const int64_t* cls; int64_t k; float thr; unsigned char* keep; int edge; bool fast = true;
    template <int V, int D> int run() {
        if constexpr (V == 2 || V == 3 || V == 4) return SPH2POB_ERR_OPTION;
        else {
            // class segments are independent: one thread sweeps a segment (the greedy dependency is serial inside it)
            std::vector<int64_t> starts;
            for (int64_t i = 0; i < k; i++)
                if (i == 0 || (cls && cls[i] != cls[i - 1])) starts.push_back(i);
            starts.push_back(k);
            const int64_t segs = (int64_t)starts.size() - 1;
            return with_pair_sel<V>(fast, ANGLE_EQUATOR, [&](auto variant, auto fast_core) {
                return for_rows(segs, 1, [&](int64_t s) {
                    const int64_t a = starts[(size_t)s], b = starts[(size_t)s + 1];
                    std::vector<unsigned char> removed((size_t)(b - a), 0);
                    for (int64_t i = a; i < b; i++) {
                        keep[i] = !removed[(size_t)(i - a)];
                        if (!keep[i]) continue;
                        float x[5];
                        load_box<D>(boxes, i, x);
                        for (int64_t j = i + 1; j < b; j++) {
                            if (removed[(size_t)(j - a)]) continue;
                            float y[5];
                            load_box<D>(boxes, j, y);
                            if (!(pair_iou_sel<decltype(variant)::value, D, decltype(fast_core)::value>(x, y, MODE_IOU, edge, ANGLE_EQUATOR) <= thr))
                                removed[(size_t)(j - a)] = 1;
                        }
                    }
                });
            });
        }
    }
};

}  // namespace

extern "C" {

int sph2pob_host_abi_version(void) { return 1; }
int sph2pob_host_threads(void) { return cpu_threads(); }

int sph2pob_iou_aligned_f32_cpu(const float* b1, const float* b2, float* out, int64_t n, int box_dim, int variant, int mode, int edge,
                                int angle, void*) {
    const int rc = check_iou(box_dim, variant, mode, edge, angle, n, n, {b1, b2, out});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim, PairIou{b1, b2, out, n, 0, mode, naive_edge(variant, edge), angle});
}

int sph2pob_iou_pairwise_f32_cpu(const float* b1, int64_t m, const float* b2, int64_t n, float* out, int box_dim, int variant, int mode,
                                 int edge, int angle, void*) {
    const int rc = check_iou(box_dim, variant, mode, edge, angle, m, n, {b1, b2, out});
    if (rc || m == 0 || n == 0) return rc;
    return dispatch(variant, box_dim, PairIou{b1, b2, out, m * n, n, mode, naive_edge(variant, edge), angle});
}

int sph2pob_transform_f32_cpu(const float* b1, const float* b2, float* planar1, float* planar2, int64_t n, int box_dim, int variant,
                              int edge, int angle, int jitter, void*) {
    const int rc = check_transform(box_dim, variant, SPH2POB_VARIANT_LEGACY, edge, angle, n, {b1, b2, planar1, planar2});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim, Transform{b1, b2, planar1, planar2, n, edge, angle, jitter});
}

int sph2pob_planar_iou_f32_cpu(const float* p1, int64_t m, const float* p2, int64_t n, float* out, int aligned, int mode, void*) {
    const int rc = check_planar_iou(p1, m, p2, n, out, aligned, mode);
    if (rc || m == 0 || n == 0) return rc;
    return for_rows(aligned ? n : m * n, 4096, [&](int64_t e) {
        out[e] = planar_pair(p1 + (aligned ? e : e / n) * 5, p2 + (aligned ? e : e % n) * 5, mode);
    });
}

int sph2pob_loss_fwd_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, float scale, float* loss,
                             float* iou, int64_t n, int box_dim, int loss_mode_flags, float eps, void*) {
    if (int rc = loss_check(weight, weight_dim, n, box_dim, loss_mode_flags)) return rc;
    return cpu_fwd(pred, target, weight, weight_dim, scale, loss, iou, n, box_dim, loss_mode_flags, IouBody{loss_mode_flags & 0xff, eps});
}

int sph2pob_loss_bwd_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, const float* grad_out,
                             int grad_stride, float scale, float* grad_pred, float* grad_target, int64_t n, int box_dim,
                             int loss_mode_flags, float eps, void*) {
    if (int rc = loss_check(weight, weight_dim, n, box_dim, loss_mode_flags, grad_stride)) return rc;
    return cpu_bwd(pred, target, weight, weight_dim, grad_out, grad_stride, scale, grad_pred, grad_target, n, box_dim, loss_mode_flags,
                   IouBody{loss_mode_flags & 0xff, eps});
}

int sph2pob_loss_fwd_sum_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, float scale, float* out,
                                 float*, int64_t n, int box_dim, int loss_mode_flags, float eps, void*) {
    if (int rc = loss_check(weight, weight_dim, n, box_dim, loss_mode_flags)) return rc;
    return cpu_fwd_sum(pred, target, weight, weight_dim, scale, out, n, box_dim, loss_mode_flags, IouBody{loss_mode_flags & 0xff, eps});
}

int sph2pob_loss_fwd_grad_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, float scale, float* loss,
                                  float* out_sum, float*, float* grad_pred, float* grad_target, int64_t n, int box_dim,
                                  int loss_mode_flags, float eps, void*) {
    if (int rc = loss_check(weight, weight_dim, n, box_dim, loss_mode_flags)) return rc;
    return cpu_fwd_grad(pred, target, weight, weight_dim, scale, loss, out_sum, grad_pred, grad_target, n, box_dim, loss_mode_flags,
                        IouBody{loss_mode_flags & 0xff, eps});
}

int sph2pob_gauss_loss_fwd_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                                   float* loss, int64_t n, int box_dim, int type_flags, int fun, float tau, float alpha, int opts,
                                   float beta, float eps, void*) {
    if (int rc = gauss_check(weight, weight_dim, n, box_dim, type_flags, fun, opts)) return rc;
    return cpu_fwd(pred, target, weight, weight_dim, scale, loss, nullptr, n, box_dim, type_flags,
                   GaussBody{type_flags & 0xff, fun, tau, alpha, opts, beta, eps});
}

int sph2pob_gauss_loss_bwd_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, const float* grad_out,
                                   int grad_stride, float scale, float* grad_pred, float* grad_target, int64_t n, int box_dim,
                                   int type_flags, int fun, float tau, float alpha, int opts, float beta, float eps, void*) {
    if (int rc = gauss_check(weight, weight_dim, n, box_dim, type_flags, fun, opts)) return rc;
    if (grad_stride != 0 && grad_stride != 1) return SPH2POB_ERR_OPTION;
    return cpu_bwd(pred, target, weight, weight_dim, grad_out, grad_stride, scale, grad_pred, grad_target, n, box_dim, type_flags,
                   GaussBody{type_flags & 0xff, fun, tau, alpha, opts, beta, eps});
}

int sph2pob_gauss_loss_fwd_sum_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                                       float* out, float*, int64_t n, int box_dim, int type_flags, int fun, float tau,
                                       float alpha, int opts, float beta, float eps, void*) {
    if (int rc = gauss_check(weight, weight_dim, n, box_dim, type_flags, fun, opts)) return rc;
    return cpu_fwd_sum(pred, target, weight, weight_dim, scale, out, n, box_dim, type_flags,
                       GaussBody{type_flags & 0xff, fun, tau, alpha, opts, beta, eps});
}

int sph2pob_gauss_loss_fwd_grad_f32_cpu(const float* pred, const float* target, const float* weight, int weight_dim, float scale,
                                        float* loss, float* out_sum, float*, float* grad_pred, float* grad_target,
                                        int64_t n, int box_dim, int type_flags, int fun, float tau, float alpha, int opts,
                                        float beta, float eps, void*) {
    if (int rc = gauss_check(weight, weight_dim, n, box_dim, type_flags, fun, opts)) return rc;
    return cpu_fwd_grad(pred, target, weight, weight_dim, scale, loss, out_sum, grad_pred, grad_target, n, box_dim, type_flags,
                        GaussBody{type_flags & 0xff, fun, tau, alpha, opts, beta, eps});
}

int sph2pob_loss_grad_scale_f32_cpu(const float* stash, const float* grad_out, int grad_stride, float* out, int64_t n, int box_dim, void*) {
    if (int rc = grad_scale_check(n, box_dim, grad_stride)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!stash || !grad_out || !out) return SPH2POB_ERR_NULL;
    if (grad_stride == 0 && out == stash && grad_out[0] == 1.0f) return SPH2POB_OK;
    const int64_t total = n * box_dim;
    for (int64_t e = 0; e < total; e++) out[e] = stash[e] * grad_out[grad_stride ? e / box_dim : 0];
    return SPH2POB_OK;
}

int sph2pob_sum_f32_cpu(const float* x, int64_t n, float scale, float* out, float* workspace, void*) {
    if (n < 0 || n > kMaxElems) return SPH2POB_ERR_SIZE;
    if (!out || !workspace || (n > 0 && !x)) return SPH2POB_ERR_NULL;   // the device's checks (no workspace is used here)
    double s = 0.0;
    for (int64_t i = 0; i < n; i++) s += x[i];
    out[0] = (float)(s * (double)scale);
    return SPH2POB_OK;
}

int sph2pob_transform_bwd_f32_cpu(const float* b1, const float* b2, const float* g1, const float* g2, float* gb1, float* gb2, int64_t n,
                                  int box_dim, int variant, int edge, int jitter, void*) {
    const int rc = check_transform(box_dim, variant, SPH2POB_VARIANT_EFFICIENT, edge, 0, n, {b1, b2, g1, g2, gb1, gb2});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim, TransformBwd<false>{b1, b2, g1, g2, gb1, gb2, n, edge, 0, jitter});
}

int sph2pob_transform_bwd_general_f32_cpu(const float* b1, const float* b2, const float* g1, const float* g2, float* gb1, float* gb2,
                                          int64_t n, int box_dim, int variant, int edge, int angle, int jitter, void*) {
    const int rc = check_transform(box_dim, variant, SPH2POB_VARIANT_LEGACY, edge, angle, n, {b1, b2, g1, g2, gb1, gb2});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim, TransformBwd<true>{b1, b2, g1, g2, gb1, gb2, n, edge, angle, jitter});
}

// ---- NMS on boxes sorted by (class, -score): sph2pob_nms_segmented_f32 / sph2pob_nms_f32 ----
int sph2pob_nms_segmented_f32_cpu(const float* boxes_sorted, const int64_t* cls_sorted, int64_t k, int box_dim, int variant_flags,
                                  float iou_threshold, int64_t max_segment, void* workspace, unsigned char* keep, void*) {
    (void)max_segment; (void)workspace;   // no suppression matrix on the host: no per-class limit either
    if (int rc = sph2pob_gb::nms_check_options(box_dim, variant_flags)) return rc;
    if (k < 0) return SPH2POB_ERR_SIZE;
    if (k == 0) return SPH2POB_OK;
    if (!boxes_sorted || !keep) return SPH2POB_ERR_NULL;
    return dispatch(variant_flags, box_dim, NmsRun{boxes_sorted, cls_sorted, k, iou_threshold, keep, naive_edge(variant_flags, EDGE_ARC)});
}
int sph2pob_nms_f32_cpu(const float* boxes_sorted, const int64_t* cls_sorted, int64_t k, int box_dim, int variant_flags, float iou_threshold,
                        void* workspace, unsigned char* keep, void* stream) {
    return sph2pob_nms_segmented_f32_cpu(boxes_sorted, cls_sorted, k, box_dim, variant_flags, iou_threshold, k, workspace, keep, stream);
}

// ---- MaxIoUAssigner epilogue on a (k, n) matrix: sph2pob_assign_f32 (mmdet max_iou_assigner.py:135-220) ----
int sph2pob_assign_f32_cpu(const float* ov, int64_t k, int64_t n, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi, float min_pos_iou,
                           int match_low_quality, int gt_max_assign_all, const int64_t* gt_labels, float* max_overlaps,
                           int64_t* argmax_overlaps, float* gt_max_overlaps, int64_t* gt_argmax_overlaps, int64_t* assigned_gt_inds,
                           int64_t* assigned_labels, void* workspace, void*) {
    (void)workspace;
    if (k <= 0 || n <= 0) return SPH2POB_ERR_SIZE;
    if (!ov || !max_overlaps || !argmax_overlaps || !gt_max_overlaps || !gt_argmax_overlaps || !assigned_gt_inds ||
        (assigned_labels && !gt_labels))
        return SPH2POB_ERR_NULL;
    const sph2pob_assign::Rule rule{pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all};
    parallel_for(n, 4096, [&](int64_t lo, int64_t hi) {   // columns: max / first argmax over the rows, thresholds
        for (int64_t j = lo; j < hi; j++) {
            float best = ov[j];
            int64_t bi = 0;
            for (int64_t i = 1; i < k; i++) {
                const float v = ov[i * n + j];
                if (v > best || (v != v && best == best)) { best = v; bi = i; }
            }
            max_overlaps[j] = best;
            argmax_overlaps[j] = bi;
            assigned_gt_inds[j] = sph2pob_assign::threshold_index(best, bi, rule);
        }
    });
    parallel_for(k, 1, [&](int64_t lo, int64_t hi) {      // rows: max / first argmax over the columns
        for (int64_t i = lo; i < hi; i++) {
            const float* row = ov + i * n;
            float best = row[0];
            int64_t bj = 0;
            for (int64_t j = 1; j < n; j++)
                if (row[j] > best || (row[j] != row[j] && best == best)) { best = row[j]; bj = j; }
            gt_max_overlaps[i] = best;
            gt_argmax_overlaps[i] = bj;
        }
    });
    if (match_low_quality) {   // later GTs overwrite earlier ones, like the reference's loop
        for (int64_t i = 0; i < k; i++) {
            const float g = gt_max_overlaps[i];
            if (!(g >= min_pos_iou)) continue;
            if (gt_max_assign_all) {
                const float* row = ov + i * n;
                for (int64_t j = 0; j < n; j++)
                    if (row[j] == g) assigned_gt_inds[j] = i + 1;
            } else {
                assigned_gt_inds[gt_argmax_overlaps[i]] = i + 1;
            }
        }
    }
    if (assigned_labels)
        for (int64_t j = 0; j < n; j++) assigned_labels[j] = assigned_gt_inds[j] > 0 ? gt_labels[assigned_gt_inds[j] - 1] : -1;
    return SPH2POB_OK;
}


}  // extern "C"

// ---- anchor targets for a minibatch: sph2pob_anchor_targets_f32 / sph2pob_anchor_targets_any_f32 after their checks (a loop over
// the images on the two twins above — the pairwise twin runs the variant's per-pair function —, then the target table of
// include/sph2pob_hip.h; workspace and state are not used) ----
namespace {
int anchor_targets_cpu(const float* anchors, int64_t n, const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets, int64_t num_images,
                       int64_t num_gt, int64_t k_max, int box_dim, int variant, int edge, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi,
                       float min_pos_iou, int match_low_quality, int gt_max_assign_all, int64_t num_classes, float pos_weight, int encode,
                       const float* means_host, const float* stds_host, int64_t* assigned_gt_inds, float* max_overlaps, int64_t* assigned_labels,
                       int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* num_pos, int64_t* num_neg,
                       float* avg_factor) {
    int rc = SPH2POB_OK;
    const sph2pob_coder::Norm nm = sph2pob_coder::make_norm(means_host, stds_host, box_dim);
    const int dim = box_dim;
    namespace A = sph2pob_assign;   // the kernel's element function, for this call's (dim, encode)
    const auto row = dim == 4 ? (encode ? A::target_row<4, true> : A::target_row<4, false>) : (encode ? A::target_row<5, true> : A::target_row<5, false>);
    std::vector<float> ov, gt_max;
    std::vector<int64_t> argmax(n), gt_argmax;
    int64_t total = 0;
    for (int64_t b = 0; b < num_images; b++) {
        const A::ImageRows im = A::image_rows(gt_offsets, b, num_gt, k_max);
        const int64_t lo = im.lo, k = im.k;
        int64_t* gi = assigned_gt_inds + b * n;
        float* mo = max_overlaps + b * n;
        const float* gt_b = gt + lo * dim;
        if (k == 0) {   // every anchor is background (max_iou_assigner.py:148-165)
            for (int64_t j = 0; j < n; j++) { gi[j] = 0; mo[j] = 0.0f; }
            if (assigned_labels) std::fill(assigned_labels + b * n, assigned_labels + (b + 1) * n, (int64_t)-1);
        } else {
            ov.resize(k * n); gt_max.resize(k); gt_argmax.resize(k);
            rc = sph2pob_iou_pairwise_f32_cpu(gt_b, k, anchors, n, ov.data(), box_dim, variant, SPH2POB_MODE_IOU, edge, SPH2POB_ANGLE_EQUATOR, nullptr);
            if (!rc)
                rc = sph2pob_assign_f32_cpu(ov.data(), k, n, pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all,
                                            gt_labels ? gt_labels + lo : nullptr, mo, argmax.data(), gt_max.data(), gt_argmax.data(), gi,
                                            assigned_labels ? assigned_labels + b * n : nullptr, nullptr, nullptr);
            if (rc) return rc;
        }
        int64_t np = 0, nn = 0;
        for (int64_t j = 0; j < n; j++) {
            const int64_t a = gi[j], e = b * n + j;
            np += a > 0; nn += a == 0;
            const A::TargetRow r = row(a, anchors + j * dim, a > 0 ? gt_b + (a - 1) * dim : nullptr, gt_labels ? gt_labels + lo : nullptr,
                                       num_classes, pos_weight, nm);
            labels[e] = r.label;
            label_weights[e] = r.label_weight;
            for (int c = 0; c < dim; c++) { bbox_targets[e * dim + c] = r.t[c]; bbox_weights[e * dim + c] = r.box_weight; }
        }
        num_pos[b] = np; num_neg[b] = nn;
        total += std::max<int64_t>(np, 1);
    }
    *avg_factor = (float)total;
    return SPH2POB_OK;
}
}  // namespace

extern "C" {

#define SPH2POB_ANCHOR_TARGETS_TWIN(NAME, VARIANT_RULE)                                                                                          \
    int NAME(const float* anchors, int64_t n, const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets, int64_t num_images,          \
             int64_t num_gt, int64_t k_max, int box_dim, int variant, int edge, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi,           \
             float min_pos_iou, int match_low_quality, int gt_max_assign_all, int64_t num_classes, float pos_weight, int encode,                 \
             const float* means_host, const float* stds_host, int64_t* assigned_gt_inds, float* max_overlaps, int64_t* assigned_labels,          \
             int64_t* labels, float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* num_pos, int64_t* num_neg,                \
             float* avg_factor, void* workspace, void* state, void*) {                                                                           \
        int rc = sph2pob_assign::anchor_targets_check(sph2pob_assign::VARIANT_RULE(check_common(box_dim, variant, edge, 0), variant), anchors, n, \
                                                      gt, gt_labels, gt_offsets, num_images, num_gt, k_max, assigned_gt_inds, max_overlaps,      \
                                                      assigned_labels, labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg,      \
                                                      avg_factor, false, workspace, state);                                                      \
        if (rc) return rc;                                                                                                                       \
        return anchor_targets_cpu(anchors, n, gt, gt_labels, gt_offsets, num_images, num_gt, k_max, box_dim, variant, edge, pos_iou_thr,         \
                                  neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all, num_classes, pos_weight, encode,    \
                                  means_host, stds_host, assigned_gt_inds, max_overlaps, assigned_labels, labels, label_weights, bbox_targets,   \
                                  bbox_weights, num_pos, num_neg, avg_factor);                                                                   \
    }
SPH2POB_ANCHOR_TARGETS_TWIN(sph2pob_anchor_targets_f32_cpu, closed_form_only)
SPH2POB_ANCHOR_TARGETS_TWIN(sph2pob_anchor_targets_any_f32_cpu, per_pair_only)
#undef SPH2POB_ANCHOR_TARGETS_TWIN

// ---- detection post-processing for a minibatch: sph2pob_test_bboxes_f32 / sph2pob_get_bboxes_f32 (the same keys, in the same
// order, sorted instead of selected; the NMS twin above on each image's candidates — one segment when class-agnostic; the
// workspace is not used).  `source` is the head's candidate source, the one cand_build_kernel is instantiated with
// (sph2pob_get_bboxes.hpp, sph2pob_rcnn_bboxes.hpp): it decodes the box of anchor, point or roi `ai` and returns the score the
// candidate goes on with ----
}  // extern "C"

namespace GB = sph2pob_gb;
namespace {

template <class Source>
int bboxes_cpu(const GB::Levels& L, const GB::Shape& sh, const GB::Selection& sel, const GB::Nms& nms, const GB::Outputs& out, const Source& source) {
    if (int rc = out.check(nms.max_per_img)) return rc;
    constexpr int dim = Source::kDim;
    const int64_t max_per_img = nms.max_per_img;
    std::vector<unsigned long long> keys, order;
    std::vector<float> boxes, scores, sorted;
    std::vector<int64_t> cls, prior, cls_sorted;
    std::vector<unsigned char> keep;
    for (int64_t b = 0; b < sh.num_images; b++) {
        boxes.clear(); scores.clear(); cls.clear(); prior.clear();
        for (int l = 0; l < L.num; l++) {
            const GB::Level& lv = L.lv[l];
            const float* base = lv.cls + b * (int64_t)lv.count;
            keys.clear();
            for (int m = 0; m < lv.count; m++) {
                const float s = GB::activate(base[m], sel.activation);
                if (!(s > sel.score_thr)) continue;
                const int ch = m / lv.hw, p = m - ch * lv.hw;
                keys.push_back(((unsigned long long)GB::desc_score_bits(s) << 32) | (unsigned)(p * lv.ac + ch));
            }
            const size_t want = std::min<size_t>(keys.size(), (size_t)lv.cap);
            std::partial_sort(keys.begin(), keys.begin() + want, keys.end());
            for (size_t i = 0; i < want; i++) {
                const unsigned flat = (unsigned)keys[i];
                const int ai = (int)(flat / (unsigned)sh.num_classes), c = (int)(flat - (unsigned)ai * (unsigned)sh.num_classes);
                if (!source.has(lv, ai)) continue;
                float box[5];
                int prior_index;
                const float score = source(lv, l, b, ai, c, GB::score_of_desc_bits((unsigned)(keys[i] >> 32)), box, &prior_index);
                boxes.insert(boxes.end(), box, box + dim);
                scores.push_back(score);
                cls.push_back((int64_t)c);
                prior.push_back(prior_index);
            }
        }
        // the batched NMS on this image: (class | descending score | position) order, the sweeps, the kept by (score | position)
        const int64_t k = (int64_t)scores.size();
        order.resize(k);
        for (int64_t j = 0; j < k; j++) order[j] = GB::nms_class_key(nms.class_agnostic ? 0 : cls[j], scores[j], (int)j);
        std::sort(order.begin(), order.end());
        sorted.resize(k * dim); cls_sorted.resize(k); keep.assign(k, 0);
        for (int64_t r = 0; r < k; r++) {
            const int64_t j = (int64_t)(order[r] & ((1u << GB::kNmsIdxBits) - 1u));
            for (int c = 0; c < dim; c++) sorted[r * dim + c] = boxes[j * dim + c];
            cls_sorted[r] = cls[j];
        }
        if (k > 0)
            if (int rc = sph2pob_nms_segmented_f32_cpu(sorted.data(), nms.class_agnostic ? nullptr : cls_sorted.data(), k, dim, nms.variant_flags,
                                                       nms.iou_threshold, k, nullptr, keep.data(), nullptr))
                return rc;
        keys.clear();
        for (int64_t r = 0; r < k; r++) {
            const int64_t j = (int64_t)(order[r] & ((1u << GB::kNmsIdxBits) - 1u));
            if (keep[r]) keys.push_back(((unsigned long long)GB::desc_score_bits(scores[j]) << 32) | (unsigned)j);
        }
        std::sort(keys.begin(), keys.end());
        const int64_t n = std::min<int64_t>((int64_t)keys.size(), max_per_img);
        out.num_dets[b] = n;
        for (int64_t r = 0; r < max_per_img; r++) {
            const int64_t e = b * max_per_img + r;
            const int64_t j = r < n ? (int64_t)(unsigned)keys[r] : -1;
            for (int c = 0; c < dim; c++) out.dets[e * (dim + 1) + c] = j >= 0 ? boxes[j * dim + c] : 0.0f;
            out.dets[e * (dim + 1) + dim] = j >= 0 ? scores[j] : 0.0f;
            out.labels[e] = j >= 0 ? cls[j] : -1;
            out.prior_inds[e] = j >= 0 ? prior[j] : -1;
        }
    }
    return SPH2POB_OK;
}

// the delta coders on a checked level table
int delta_bboxes_cpu(const GB::Levels& L, const GB::Shape& sh, const GB::Selection& sel, const GB::Coder& cd, const GB::Nms& nms,
                     const GB::Outputs& out) {
    return GB::with_dim(sh.box_dim, [&](auto dim) { return bboxes_cpu(L, sh, sel, nms, out, GB::DeltaSource<decltype(dim)::value>{cd}); });
}
}  // namespace

extern "C" {

int sph2pob_test_bboxes_f32_cpu(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                                const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                                float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                                int coder_flags, float ctr_clamp, int variant, int class_agnostic, float iou_threshold, int64_t max_per_img,
                                float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void*) {
    (void)workspace;
    const GB::Shape sh{level_n, level_hw, num_levels, num_images, num_classes, box_dim};
    const GB::Selection sel{activation, score_thr, nms_pre};
    const GB::Coder cd = GB::make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp);
    const GB::Nms nms{variant, class_agnostic, iou_threshold, max_per_img};
    GB::Levels L;
    if (int rc = GB::make_levels(cls_scores, bbox_preds, anchors, sh, sel, cd, nms, &L)) return rc;
    return delta_bboxes_cpu(L, sh, sel, cd, nms, GB::Outputs{dets, labels, prior_inds, num_dets});
}
// FCOS heads: the point coder's decode_row, score = class score * activate(centerness), one fp32 multiply (the kernel's)
int sph2pob_fcos_bboxes_f32_cpu(const void* const* cls_scores, const void* const* bbox_preds, const void* const* points,
                                const void* const* centernesses, const int64_t* level_n, const int64_t* level_hw, int num_levels,
                                int64_t num_images, int64_t num_classes, int box_dim, int activation, float score_thr, int64_t nms_pre,
                                int64_t img_h, int64_t img_w, float max_h, float max_w, int variant, int class_agnostic, float iou_threshold,
                                int64_t max_per_img, float* dets, int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void*) {
    (void)workspace;
    const GB::Shape sh{level_n, level_hw, num_levels, num_images, num_classes, box_dim};
    const GB::Selection sel{activation, score_thr, nms_pre};
    const GB::Frame fr{img_h, img_w, max_h, max_w};
    const GB::Nms nms{variant, class_agnostic, iou_threshold, max_per_img};
    GB::Levels L;
    GB::Factors F;
    if (int rc = GB::make_point_levels(cls_scores, bbox_preds, points, centernesses, sh, sel, nms, fr, &L, &F)) return rc;
    return GB::with_dim(box_dim, [&](auto dim) {
        return bboxes_cpu(L, sh, sel, nms, GB::Outputs{dets, labels, prior_inds, num_dets},
                          GB::PointSource<decltype(dim)::value>{F, fr.image(), activation});
    });
}
int sph2pob_get_bboxes_f32_cpu(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                               const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, int activation,
                               float score_thr, int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio,
                               int coder_flags, float ctr_clamp, int variant, float iou_threshold, int64_t max_per_img, float* dets,
                               int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void* stream) {
    if ((box_dim == 4 || box_dim == 5) && !sph2pob_gb::closed_form_variant(variant)) return SPH2POB_ERR_OPTION;
    return sph2pob_test_bboxes_f32_cpu(cls_scores, bbox_preds, anchors, level_n, level_hw, num_levels, num_images, num_classes, box_dim, activation,
                                       score_thr, nms_pre, means_host, stds_host, max_ratio, coder_flags, ctr_clamp, variant, 0, iou_threshold,
                                       max_per_img, dets, labels, prior_inds, num_dets, workspace, stream);
}

}  // extern "C"

// ---- box coders and the OBB L1 loss body (sph2pob_coder.hpp: the rows the kernels of sph2pob_coder.hip compute) ----
namespace {
namespace C = sph2pob_coder;

template <int DIM>
void coder_encode_rows(const float* proposals, const float* gt, const C::Norm& nm, float* deltas, int64_t n) {
    parallel_for(n, 1 << 14, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            float d[5];
            C::encode_one<DIM>(proposals + i * DIM, gt + i * DIM, nm, d);
            for (int k = 0; k < DIM; k++) deltas[i * DIM + k] = d[k];
        }
    });
}

template <int DIM, bool BWD>
void coder_decode_rows(const float* rois, const float* deltas, const float* grad_boxes, const C::Norm& nm, float* out, int64_t total,
                       int num_classes, float max_ratio, int flags, float ctr_clamp) {
    parallel_for(total, 1 << 14, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            float p[5] = {0, 0, 0, 0, 0}, b[5], j[5];
            const float* r = rois + (num_classes == 1 ? i : i / num_classes) * DIM;
            for (int k = 0; k < DIM; k++) p[k] = r[k];
            C::decode_one<DIM, BWD>(p, deltas + i * DIM, nm, max_ratio, flags, ctr_clamp, b, BWD ? j : nullptr);
            for (int k = 0; k < DIM; k++) out[i * DIM + k] = BWD ? grad_boxes[i * DIM + k] * j[k] : b[k];
        }
    });
}
}  // namespace

extern "C" {

int sph2pob_coder_encode_f32_cpu(const float* proposals, const float* gt, const float* means_host, const float* stds_host,
                                 float* deltas, int64_t n, int box_dim, void*) {
    if (int rc = C::check_encode(proposals, gt, deltas, n, box_dim)) return rc;
    if (n == 0) return 0;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    if (box_dim == 4) coder_encode_rows<4>(proposals, gt, nm, deltas, n);
    else coder_encode_rows<5>(proposals, gt, nm, deltas, n);
    return SPH2POB_OK;
}

int sph2pob_coder_decode_f32_cpu(const float* rois, const float* deltas, const float* means_host, const float* stds_host,
                                 float* boxes, int64_t n, int num_classes, int box_dim, float max_ratio, int flags,
                                 float ctr_clamp, void*) {
    if (int rc = C::check_decode(rois, deltas, deltas, boxes, n, num_classes, box_dim, max_ratio, flags)) return rc;
    if (n == 0) return 0;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    if (box_dim == 4) coder_decode_rows<4, false>(rois, deltas, nullptr, nm, boxes, n * num_classes, num_classes, max_ratio, flags, ctr_clamp);
    else coder_decode_rows<5, false>(rois, deltas, nullptr, nm, boxes, n * num_classes, num_classes, max_ratio, flags, ctr_clamp);
    return SPH2POB_OK;
}

int sph2pob_coder_decode_bwd_f32_cpu(const float* rois, const float* deltas, const float* grad_boxes, const float* means_host,
                                     const float* stds_host, float* grad_deltas, int64_t n, int num_classes, int box_dim,
                                     float max_ratio, int flags, float ctr_clamp, void*) {
    if (int rc = C::check_decode(rois, deltas, grad_boxes, grad_deltas, n, num_classes, box_dim, max_ratio, flags)) return rc;
    if (n == 0) return 0;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    if (box_dim == 4) coder_decode_rows<4, true>(rois, deltas, grad_boxes, nm, grad_deltas, n * num_classes, num_classes, max_ratio, flags, ctr_clamp);
    else coder_decode_rows<5, true>(rois, deltas, grad_boxes, nm, grad_deltas, n * num_classes, num_classes, max_ratio, flags, ctr_clamp);
    return SPH2POB_OK;
}

int sph2pob_obb_l1_fwd_f32_cpu(const float* planar_pred, const float* planar_target, const float* weight, float scale, float* loss,
                               int64_t n, int flags, void*) {
    if (int rc = C::check_l1(planar_pred, planar_target, planar_pred, loss, n, flags)) return rc;
    if (n == 0) return 0;
    parallel_for(n, 1 << 14, [&](int64_t lo, int64_t hi) {
        const float ones[5] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
        for (int64_t i = lo; i < hi; i++) {
            float d[5];
            C::l1_fwd_one(planar_pred + i * 5, planar_target + i * 5, weight ? weight + i * 5 : ones, scale, flags, d);
            for (int k = 0; k < 5; k++) loss[i * 5 + k] = d[k];
        }
    });
    return SPH2POB_OK;
}

int sph2pob_obb_l1_bwd_f32_cpu(const float* planar_pred, const float* planar_target, const float* weight, const float* grad_loss,
                               float scale, float* grad_pred, float* grad_target, int64_t n, int flags, void*) {
    if (int rc = C::check_l1(planar_pred, planar_target, grad_loss, grad_pred, n, flags)) return rc;
    if (n == 0) return 0;
    parallel_for(n, 1 << 14, [&](int64_t lo, int64_t hi) {
        const float ones[5] = {1.0f, 1.0f, 1.0f, 1.0f, 1.0f};
        for (int64_t i = lo; i < hi; i++) {
            float u[5], ga[5], gb[5];
            for (int k = 0; k < 5; k++) u[k] = grad_loss[i * 5 + k];
            C::l1_bwd_one(planar_pred + i * 5, planar_target + i * 5, weight ? weight + i * 5 : ones, u, scale, flags, ga, gb);
            for (int k = 0; k < 5; k++) grad_pred[i * 5 + k] = ga[k];
            if (grad_target)
                for (int k = 0; k < 5; k++) grad_target[i * 5 + k] = gb[k];
        }
    });
    return SPH2POB_OK;
}

}  // extern "C"

// ---- sigmoid focal loss: the twins of sph2pob_focal.hip on the element function of sph2pob_focal.hpp ----
namespace {
namespace FL = sph2pob_focal;
constexpr int64_t kFocalRows = 1024;   // rows of one partial sum: the partials do not move with the thread count

// The row walk of the three head-loss twins: f(lv, b, i, row, acc) for every row = b n_total + j of the call, lv the level of j
// and i = j - lv.row_off the anchor inside it; f adds the row's weighted losses to acc.  One double partial per kFocalRows rows,
// the partials added in order: the total does not move with the thread count.
template <class Levels, class F>
double head_rows_sum(const Levels& L, int64_t rows, F&& f) {
    const int64_t chunks = (rows + kFocalRows - 1) / kFocalRows;
    std::vector<double> part((size_t)chunks, 0.0);
    parallel_for(chunks, 4, [&](int64_t lo, int64_t hi) {
        for (int64_t ch = lo; ch < hi; ch++) {
            double acc = 0.0;
            for (int64_t row = ch * kFocalRows; row < std::min(rows, (ch + 1) * kFocalRows); row++) {
                const int64_t b = row / L.n_total, j = row - b * L.n_total;
                int l = 0;
                for (int q = 1; q < L.num; q++) l += j >= L.lv[q].row_off ? 1 : 0;
                f(L.lv[l], b, j - L.lv[l].row_off, row, acc);
            }
            part[(size_t)ch] = acc;
        }
    });
    double total = 0.0;
    for (double v : part) total += v;
    return total;
}

// The regression twins' row: a dead row (live false) is never read and gets DIM exact zeros at off + k * stride; a live one runs
// eval(off, stride).
template <int DIM, class Eval>
inline void box_row(const sph2pob_bbox::Level& lv, int64_t b, int64_t i, bool live, Eval&& eval) {
    int64_t stride;
    const int64_t off = sph2pob_bbox::delta_offset(lv, DIM, b, i, &stride);
    if (live) eval(off, stride);
    else if (lv.grad)
        for (int k = 0; k < DIM; k++) lv.grad[off + k * stride] = 0.0f;
}
}  // namespace

extern "C" {

int sph2pob_focal_loss_sum_f32_cpu(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                   int num_levels, int64_t num_images, int64_t num_classes, const int64_t* labels, const float* weight,
                                   int weight_mode, float gamma, float alpha, float scale, const float* avg_factor, float* out,
                                   void* workspace, void*) {
    FL::Levels L;
    if (int rc = FL::make_levels(logits, grads, level_n, level_hw, num_levels, num_images, num_classes, weight_mode, gamma, true, &L)) return rc;
    if (!out || !workspace || (L.elems > 0 && (!labels || (weight_mode != 0 && !weight)))) return SPH2POB_ERR_NULL;
    const FL::Params P = FL::make_params(gamma, alpha);
    const float k0 = FL::effective_scale(scale, avg_factor);
    const int64_t rows = L.elems > 0 ? num_images * L.n_total : 0, C = num_classes;
    const double total = head_rows_sum(L, rows, [&](const FL::Level& lv, int64_t b, int64_t i, int64_t row, double& acc) {
        int64_t base, stride;   // element (row, c) = base + c * stride
        sph2pob_class::class_row_span(lv, C, b, i, &base, &stride);
        const int64_t lab = labels[row];
        for (int c = 0; c < (int)C; c++) {
            float loss, dx;
            FL::element(lv.logits[base + c * stride], lab == (int64_t)c, P, loss, dx);
            const float we = FL::weight_of(weight, weight_mode, row, C, c);
            acc += (double)(loss * we);
            if (lv.grad) lv.grad[base + c * stride] = (k0 * we) * dx;
        }
    });
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

int sph2pob_focal_loss_fwd_f32_cpu(const float* logits, const int64_t* labels, const float* weight, int weight_mode, float gamma,
                                   float alpha, float scale, float* loss, int64_t n, int64_t num_classes, void*) {
    if (int rc = FL::flat_check(n, num_classes, weight_mode, gamma, 0)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !loss || (weight_mode != 0 && !weight)) return SPH2POB_ERR_NULL;
    const FL::Params P = FL::make_params(gamma, alpha);
    parallel_for(n, 1 << 10, [&](int64_t lo, int64_t hi) {
        for (int64_t row = lo; row < hi; row++)
            for (int c = 0; c < (int)num_classes; c++) {
                float l, dx;
                FL::element(logits[row * num_classes + c], labels[row] == (int64_t)c, P, l, dx);
                loss[row * num_classes + c] = (scale * FL::weight_of(weight, weight_mode, row, num_classes, c)) * l;
            }
    });
    return SPH2POB_OK;
}

int sph2pob_focal_loss_bwd_f32_cpu(const float* logits, const int64_t* labels, const float* weight, int weight_mode, const float* grad_out,
                                   int grad_stride, float gamma, float alpha, float scale, const float* avg_factor, float* grad_logits,
                                   int64_t n, int64_t num_classes, void*) {
    if (int rc = FL::flat_check(n, num_classes, weight_mode, gamma, grad_stride)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !grad_out || !grad_logits || (weight_mode != 0 && !weight)) return SPH2POB_ERR_NULL;
    const FL::Params P = FL::make_params(gamma, alpha);
    const float k0 = FL::effective_scale(scale, avg_factor);
    parallel_for(n, 1 << 10, [&](int64_t lo, int64_t hi) {
        for (int64_t row = lo; row < hi; row++)
            for (int c = 0; c < (int)num_classes; c++) {
                const int64_t e = row * num_classes + c;
                float l, dx;
                FL::element(logits[e], labels[row] == (int64_t)c, P, l, dx);
                grad_logits[e] = grad_out[grad_stride ? e : 0] * ((k0 * FL::weight_of(weight, weight_mode, row, num_classes, c)) * dx);
            }
    });
    return SPH2POB_OK;
}

int sph2pob_focal_loss_grad_scale_f32_cpu(const float* stash, const float* grad_out, float* out, int64_t total, void*) {
    if (total < 0 || total > ((int64_t)1 << 38)) return SPH2POB_ERR_SIZE;
    if (total == 0) return SPH2POB_OK;
    if (!stash || !grad_out || !out) return SPH2POB_ERR_NULL;
    const float s = grad_out[0];
    if (out == stash && s == 1.0f) return SPH2POB_OK;
    parallel_for(total, 1 << 16, [&](int64_t lo, int64_t hi) {
        for (int64_t e = lo; e < hi; e++) out[e] = stash[e] * s;
    });
    return SPH2POB_OK;
}

}  // extern "C"

// ---- sigmoid binary cross-entropy: the twin of sph2pob_bce_loss.hip on the element and target functions of sph2pob_bce_loss.hpp ----
namespace {
template <bool HARD>
double bce_rows(const sph2pob_bce::Levels& L, int64_t rows, int64_t C, const sph2pob_bce::Targets& T, float k0) {
    return head_rows_sum(L, rows, [&](const sph2pob_bce::Level& lv, int64_t b, int64_t i, int64_t row, double& acc) {
        int64_t base, stride;   // element (row, c) = base + c * stride
        sph2pob_class::class_row_span(lv, C, b, i, &base, &stride);
        for (int c = 0; c < (int)C; c++) {
            float t, we, loss, dx;
            sph2pob_bce::target_weight<HARD>(T, row, C, c, t, we);
            sph2pob_bce::element(lv.logits[base + c * stride], t, loss, dx);
            acc += (double)(loss * we);
            if (lv.grad) lv.grad[base + c * stride] = (k0 * we) * dx;
        }
    });
}
}  // namespace

extern "C" {

int sph2pob_bce_loss_sum_f32_cpu(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                 int num_levels, int64_t num_images, int64_t num_channels, const float* targets, const int64_t* labels,
                                 const float* weight, int weight_mode, int64_t ignore_index, float scale, const float* avg_factor,
                                 float* out, void* workspace, void*) {
    namespace BC = sph2pob_bce;
    BC::Levels L;
    if (int rc = BC::make_levels(logits, grads, level_n, level_hw, num_levels, num_images, num_channels, weight_mode, true, &L)) return rc;
    if (int rc = BC::check_tensors(L, targets, labels, weight, weight_mode, out, workspace)) return rc;
    const BC::Targets T{targets, labels, weight, weight_mode, ignore_index};
    const float k0 = BC::effective_scale(scale, avg_factor);
    const int64_t rows = L.elems > 0 ? num_images * L.n_total : 0;
    const double total = labels ? bce_rows<true>(L, rows, num_channels, T, k0) : bce_rows<false>(L, rows, num_channels, T, k0);
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

}  // extern "C"

// ---- fused box-regression losses: the twins of sph2pob_bbox_loss.hip and sph2pob_gauss_bbox_loss.hip on decode_one + the
// per-pair body (IouBody: pair_loss; GaussBody: pair_gauss_loss), row by row ----
namespace {
namespace BL = sph2pob_bbox;

template <int DIM, bool FAST, class Body>
double bbox_loss_rows(const BL::Levels& L, const float* anchors, const float* targets, const float* weight, int wd, const C::Norm& nm,
                      float max_ratio, int cflags, float ctr_clamp, const Body& body, float k0) {
    return head_rows_sum(L, L.rows, [&](const BL::Level& lv, int64_t b, int64_t i, int64_t row, double& acc) {
        const float w = element_weight<DIM>(weight, wd, row);
        box_row<DIM>(lv, b, i, w != 0.0f, [&](int64_t off, int64_t stride) {
            const int64_t j = lv.row_off + i;
            float p[5], d[5], t[5], box[5] = {0, 0, 0, 0, 0}, jac[5], gx[5], gy[5];
            for (int k = 0; k < 5; k++) {
                p[k] = k < DIM ? anchors[j * DIM + k] : 0.0f;
                d[k] = k < DIM ? lv.pred[off + k * stride] : 0.0f;
                t[k] = k < DIM ? targets[row * DIM + k] : 0.0f;
            }
            C::decode_one<DIM, true>(p, d, nm, max_ratio, cflags, ctr_clamp, box, jac);
            const float lo1 = body.template eval<DIM, true, FAST>(box, t, nullptr, gx, gy);
            acc += (double)(lo1 * w);
            if (lv.grad) {
                const float g = k0 * w;
                for (int k = 0; k < DIM; k++) lv.grad[off + k * stride] = (g * gx[k]) * jac[k];
            }
        });
    });
}

// the sum of the rows for the box_dim and the arithmetic of a call
template <class Body>
double bbox_loss_total(int box_dim, bool fast, const BL::Levels& L, const float* anchors, const float* targets, const float* weight, int wd,
                       const C::Norm& nm, float max_ratio, int cflags, float ctr_clamp, const Body& body, float k0) {
#define SPH_BBOX_ROWS(D, F) bbox_loss_rows<D, F>(L, anchors, targets, weight, wd, nm, max_ratio, cflags, ctr_clamp, body, k0)
    if (box_dim == 4) return fast ? SPH_BBOX_ROWS(4, true) : SPH_BBOX_ROWS(4, false);
    return fast ? SPH_BBOX_ROWS(5, true) : SPH_BBOX_ROWS(5, false);
#undef SPH_BBOX_ROWS
}
}  // namespace

extern "C" {

int sph2pob_bbox_loss_sum_f32_cpu(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                  int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                                  const float* weight, int weight_dim, const float* means_host, const float* stds_host, float max_ratio,
                                  int coder_flags, float ctr_clamp, int loss_mode, float eps, float scale, const float* avg_factor,
                                  float* out, void* workspace, void*) {
    if (int rc = BL::check_options(box_dim, weight, weight_dim, max_ratio, coder_flags, loss_mode)) return rc;
    BL::Levels L;
    if (int rc = BL::make_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, true, &L)) return rc;
    if (!out || !workspace || (L.rows > 0 && (!anchors || !targets))) return SPH2POB_ERR_NULL;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    const float k0 = BL::effective_scale(scale, avg_factor);
    const bool fast = !(loss_mode & SPH2POB_FLAG_REFERENCE_ORDER);
    double total = 0.0;
    if (L.rows > 0)
        total = bbox_loss_total(box_dim, fast, L, anchors, targets, weight, weight_dim, nm, max_ratio, coder_flags, ctr_clamp,
                                IouBody{loss_mode & 0xff, eps}, k0);
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

int sph2pob_gauss_bbox_loss_sum_f32_cpu(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                        int num_levels, int64_t num_images, int box_dim, const float* anchors, const float* targets,
                                        const float* weight, int weight_dim, const float* means_host, const float* stds_host,
                                        float max_ratio, int coder_flags, float ctr_clamp, int type_flags, int fun, float tau,
                                        float alpha, int opts, float beta, float eps, float scale, const float* avg_factor, float* out,
                                        void* workspace, void*) {
    if (int rc = sph2pob_gauss_bbox::check_options(box_dim, weight, weight_dim, max_ratio, coder_flags, type_flags, fun, opts)) return rc;
    BL::Levels L;
    if (int rc = BL::make_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, true, &L)) return rc;
    if (!out || !workspace || (L.rows > 0 && (!anchors || !targets))) return SPH2POB_ERR_NULL;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    const float k0 = BL::effective_scale(scale, avg_factor);
    const bool fast = !(type_flags & SPH2POB_FLAG_REFERENCE_ORDER);
    double total = 0.0;
    if (L.rows > 0)
        total = bbox_loss_total(box_dim, fast, L, anchors, targets, weight, weight_dim, nm, max_ratio, coder_flags, ctr_clamp,
                                sph2pob_gauss_bbox::make_body(type_flags, fun, tau, alpha, opts, beta, eps), k0);
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

}  // extern "C"

// ---- fused box-regression loss of a point head: the twin of sph2pob_point_bbox_loss.hip on the same row function ----
namespace {
template <int DIM, bool FAST>
double point_bbox_loss_rows(const BL::Levels& L, const float* points, const float* targets, const float* weight, int wd,
                            const sph2pob_point::Image& im, int mode, float eps, float k0) {
    return head_rows_sum(L, L.rows, [&](const BL::Level& lv, int64_t b, int64_t i, int64_t row, double& acc) {
        const float w = element_weight<DIM>(weight, wd, row);
        box_row<DIM>(lv, b, i, w != 0.0f, [&](int64_t off, int64_t stride) {
            const int64_t j = lv.row_off + i;
            const float pt[2] = {points[2 * j], points[2 * j + 1]};
            float d[5], t[5], g[5];
            for (int k = 0; k < 5; k++) {
                d[k] = k < DIM ? lv.pred[off + k * stride] : 0.0f;
                t[k] = k < DIM ? targets[row * DIM + k] : 0.0f;
            }
            const float lo1 = sph2pob_point_bbox::row_loss<DIM, true, FAST>(pt, d, t, im, mode, eps, k0 * w, g);
            acc += (double)(lo1 * w);
            if (lv.grad)
                for (int k = 0; k < DIM; k++) lv.grad[off + k * stride] = g[k];
        });
    });
}
}  // namespace

extern "C" {

int sph2pob_point_bbox_loss_sum_f32_cpu(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                        int num_levels, int64_t num_images, int box_dim, const float* points, const float* targets,
                                        const float* weight, int weight_dim, int64_t img_h, int64_t img_w, float max_h, float max_w,
                                        int loss_mode, float eps, float scale, const float* avg_factor, float* out, void* workspace, void*) {
    BL::Levels L;
    if (int rc = sph2pob_point_bbox::check_and_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, weight, weight_dim,
                                                      img_h, img_w, loss_mode, &L))
        return rc;
    if (!out || !workspace || (L.rows > 0 && (!points || !targets))) return SPH2POB_ERR_NULL;
    if (int rc = sph2pob_point_bbox::check_bounds(max_h, max_w)) return rc;
    const sph2pob_point::Image im{(float)img_w, (float)img_h, max_w, max_h};
    const float k0 = BL::effective_scale(scale, avg_factor);
    const bool fast = !(loss_mode & SPH2POB_FLAG_REFERENCE_ORDER);
    const int mode = loss_mode & 0xff;
    double total = 0.0;
    if (L.rows > 0) {
#define SPH_POINT_ROWS(D, F) point_bbox_loss_rows<D, F>(L, points, targets, weight, weight_dim, im, mode, eps, k0)
        if (box_dim == 4) total = fast ? SPH_POINT_ROWS(4, true) : SPH_POINT_ROWS(4, false);
        else total = fast ? SPH_POINT_ROWS(5, true) : SPH_POINT_ROWS(5, false);
#undef SPH_POINT_ROWS
    }
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

}  // extern "C"

// ---- fused L1 / SmoothL1 loss on encoded deltas: the twin of sph2pob_delta_loss.hip on the same element function, row by row ----
namespace {
namespace DL = sph2pob_delta;

template <int DIM>
double delta_loss_rows(const DL::Levels& L, const float* targets, const float* weight, int wd, float beta, float k0) {
    return head_rows_sum(L, L.rows, [&](const DL::Level& lv, int64_t b, int64_t i, int64_t row, double& acc) {
        float wk[DIM];
        const bool live = DL::row_weights<DIM>(weight, wd, false, row, wk);
        box_row<DIM>(lv, b, i, live, [&](int64_t off, int64_t stride) {
            for (int k = 0; k < DIM; k++) {
                float lo1, sk;
                DL::element(lv.pred[off + k * stride], targets[row * DIM + k], beta, lo1, sk);
                acc += (double)(lo1 * wk[k]);
                if (lv.grad) lv.grad[off + k * stride] = (k0 * wk[k]) * sk;
            }
        });
    });
}
}  // namespace

extern "C" {

int sph2pob_delta_loss_sum_f32_cpu(const void* const* bbox_preds, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                   int num_levels, int64_t num_images, int box_dim, const float* targets, const float* weight,
                                   int weight_dim, float beta, float scale, const float* avg_factor, float* out, void* workspace,
                                   void*) {
    if (int rc = DL::check_options(box_dim, weight, weight_dim, beta)) return rc;
    DL::Levels L;
    if (int rc = DL::make_levels(bbox_preds, grads, level_n, level_hw, num_levels, num_images, box_dim, true, &L)) return rc;
    if (!out || !workspace || (L.rows > 0 && !targets)) return SPH2POB_ERR_NULL;
    const float k0 = DL::effective_scale(scale, avg_factor);
    const int wd = weight ? weight_dim : 0;
    double total = 0.0;
    if (L.rows > 0)
        total = box_dim == 4 ? delta_loss_rows<4>(L, targets, weight, wd, beta, k0) : delta_loss_rows<5>(L, targets, weight, wd, beta, k0);
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

}  // extern "C"

// ---- fused box loss of the R-CNN head on its per-class deltas: the twins of sph2pob_rcnn_loss.hip on the same row rule
// (slot_of, then the family's weight rule) and the row bodies of the two twins above ----
namespace {
namespace RL = sph2pob_rcnn_loss;

// f(row, slot, g, acc) for every row whose label is a class; f returns whether the row takes part and then has added its weighted
// losses to acc and left the DIM gradient values in g.  The row's W gradient floats are written once: zeros and, for a live row,
// g in its slot.  One double partial per kFocalRows rows, added in order: the total does not move with the thread count.
template <int DIM, class F>
double rcnn_rows_sum(const RL::Shape& sh, const int64_t* labels, float* grad, F&& f) {
    const int64_t rows = sh.rows, chunks = (rows + kFocalRows - 1) / kFocalRows;
    std::vector<double> part((size_t)chunks, 0.0);
    parallel_for(chunks, 4, [&](int64_t lo, int64_t hi) {
        for (int64_t ch = lo; ch < hi; ch++) {
            double acc = 0.0;
            for (int64_t row = ch * kFocalRows; row < std::min(rows, (ch + 1) * kFocalRows); row++) {
                float g[DIM];
                int slot = RL::slot_of(labels[row], sh.classes, sh.slots);
                if (slot >= 0 && !f(row, slot, g, acc)) slot = -1;
                if (!grad) continue;
                float* gr = grad + row * sh.w;
                for (int c = 0; c < sh.w; c++) {
                    const int k = c - slot * DIM;
                    gr[c] = (slot >= 0 && k >= 0 && k < DIM) ? g[k] : 0.0f;
                }
            }
            part[(size_t)ch] = acc;
        }
    });
    double total = 0.0;
    for (double v : part) total += v;
    return total;
}

template <int DIM>
double rcnn_delta_rows(const RL::Shape& sh, const float* pred, float* grad, const int64_t* labels, const float* targets, const float* weight,
                       int wd, float beta, float k0) {
    return rcnn_rows_sum<DIM>(sh, labels, grad, [&](int64_t row, int slot, float (&g)[DIM], double& acc) {
        float wk[DIM];
        if (!DL::row_weights<DIM>(weight, wd, false, row, wk)) return false;
        const float* dp = pred + row * sh.w + slot * DIM;
        for (int k = 0; k < DIM; k++) {
            float lo1, sk;
            DL::element(dp[k], targets[row * DIM + k], beta, lo1, sk);
            acc += (double)(lo1 * wk[k]);
            g[k] = (k0 * wk[k]) * sk;
        }
        return true;
    });
}

template <int DIM, bool FAST>
double rcnn_bbox_rows(const RL::Shape& sh, const float* pred, float* grad, const int64_t* labels, const float* rois, int64_t roi_stride,
                      int64_t roi_offset, const float* targets, const float* weight, int wd, const C::Norm& nm, float max_ratio, int cflags,
                      float ctr_clamp, const IouBody& body, float k0) {
    return rcnn_rows_sum<DIM>(sh, labels, grad, [&](int64_t row, int slot, float (&g)[DIM], double& acc) {
        const float w = element_weight<DIM>(weight, wd, row);
        if (!(w != 0.0f)) return false;
        const float* ap = rois + row * roi_stride + roi_offset;
        const float* dp = pred + row * sh.w + slot * DIM;
        float p[5], d[5], t[5], box[5] = {0, 0, 0, 0, 0}, jac[5], gx[5], gy[5];
        for (int k = 0; k < 5; k++) {
            p[k] = k < DIM ? ap[k] : 0.0f;
            d[k] = k < DIM ? dp[k] : 0.0f;
            t[k] = k < DIM ? targets[row * DIM + k] : 0.0f;
        }
        C::decode_one<DIM, true>(p, d, nm, max_ratio, cflags, ctr_clamp, box, jac);
        const float lo1 = body.template eval<DIM, true, FAST>(box, t, nullptr, gx, gy);
        acc += (double)(lo1 * w);
        const float gw = k0 * w;
        for (int k = 0; k < DIM; k++) g[k] = (gw * gx[k]) * jac[k];
        return true;
    });
}
}  // namespace

extern "C" {

int sph2pob_rcnn_delta_loss_sum_f32_cpu(const float* bbox_pred, float* grad, int64_t rows, int64_t num_slots, int64_t num_classes,
                                        int box_dim, const int64_t* labels, const float* targets, const float* weight, int weight_dim,
                                        float beta, float scale, const float* avg_factor, float* out, void* workspace, void*) {
    if (int rc = DL::check_options(box_dim, weight, weight_dim, beta)) return rc;
    RL::Shape sh;
    if (int rc = RL::make_shape(rows, num_slots, num_classes, box_dim, &sh)) return rc;
    if (int rc = RL::check_tensors(sh, bbox_pred, labels, targets, false, nullptr, 0, 0, box_dim, out, workspace)) return rc;
    const float k0 = RL::effective_scale(scale, avg_factor);
    const int wd = weight ? weight_dim : 0;
    double total = 0.0;
    if (sh.rows > 0)
        total = box_dim == 4 ? rcnn_delta_rows<4>(sh, bbox_pred, grad, labels, targets, weight, wd, beta, k0)
                             : rcnn_delta_rows<5>(sh, bbox_pred, grad, labels, targets, weight, wd, beta, k0);
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

int sph2pob_rcnn_bbox_loss_sum_f32_cpu(const float* bbox_pred, float* grad, int64_t rows, int64_t num_slots, int64_t num_classes, int box_dim,
                                       const int64_t* labels, const float* rois, int64_t roi_stride, int64_t roi_offset,
                                       const float* targets, const float* weight, int weight_dim, const float* means_host,
                                       const float* stds_host, float max_ratio, int coder_flags, float ctr_clamp, int loss_mode, float eps,
                                       float scale, const float* avg_factor, float* out, void* workspace, void*) {
    if (int rc = BL::check_options(box_dim, weight, weight_dim, max_ratio, coder_flags, loss_mode)) return rc;
    RL::Shape sh;
    if (int rc = RL::make_shape(rows, num_slots, num_classes, box_dim, &sh)) return rc;
    if (int rc = RL::check_tensors(sh, bbox_pred, labels, targets, true, rois, roi_stride, roi_offset, box_dim, out, workspace)) return rc;
    const C::Norm nm = C::make_norm(means_host, stds_host, box_dim);
    const float k0 = RL::effective_scale(scale, avg_factor);
    const bool fast = !(loss_mode & SPH2POB_FLAG_REFERENCE_ORDER);
    const IouBody body{loss_mode & 0xff, eps};
    double total = 0.0;
    if (sh.rows > 0) {
#define SPH_RCNN_ROWS(D, F) rcnn_bbox_rows<D, F>(sh, bbox_pred, grad, labels, rois, roi_stride, roi_offset, targets, weight, weight_dim, nm, \
                                                 max_ratio, coder_flags, ctr_clamp, body, k0)
        if (box_dim == 4) total = fast ? SPH_RCNN_ROWS(4, true) : SPH_RCNN_ROWS(4, false);
        else total = fast ? SPH_RCNN_ROWS(5, true) : SPH_RCNN_ROWS(5, false);
#undef SPH_RCNN_ROWS
    }
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

}  // extern "C"

// ---- softmax cross-entropy, plain and mined: the twins of sph2pob_softmax.hip on the Row and the keys of sph2pob_softmax.hpp; the
// cut of an image by sph2pob_select.hpp's host_cut ----
namespace {
namespace SM = sph2pob_softmax;

// the three walks of one valid row: its cross-entropy, and (g != NULL) g[c * stride] = kw * d CE / d x_c
inline float softmax_row(const float* x, float* g, int64_t stride, int K, int64_t lab, float kw) {
    SM::Row r;
    r.begin((int)lab);
    for (int c = 0; c < K; c++) r.see_max(c, x[c * stride]);
    r.close_max();
    for (int c = 0; c < K; c++) r.see_sum(c, x[c * stride]);
    const float ce = r.close_sum();
    if (g)
        for (int c = 0; c < K; c++) g[c * stride] = kw * r.grad(c, x[c * stride]);
    return ce;
}
inline void softmax_zero_row(float* g, int64_t stride, int K) {
    for (int c = 0; c < K; c++) g[c * stride] = 0.0f;
}
}  // namespace

extern "C" {

int sph2pob_softmax_loss_sum_f32_cpu(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                     int num_levels, int64_t num_images, int64_t num_channels, const int64_t* labels, const float* weight,
                                     const float* class_weight, int64_t ignore_index, int64_t background_label, int64_t neg_pos_ratio,
                                     float scale, const float* avg_factor, float* out, void* workspace, void*) {
    SM::Levels L;
    if (int rc = SM::make_levels(logits, grads, level_n, level_hw, num_levels, num_images, num_channels, neg_pos_ratio, true, &L)) return rc;
    if (!out || !workspace || (L.rows > 0 && !labels)) return SPH2POB_ERR_NULL;
    const float k0 = SM::effective_scale(scale, avg_factor);
    const int K = (int)num_channels;
    const bool mining = neg_pos_ratio >= 0;
    const int64_t n = L.n_total;
    std::vector<unsigned> keys(mining ? (size_t)L.rows : 0);
    // first pass: plain — losses and gradients; mining — keys and the positives' losses
    double total = head_rows_sum(L, L.rows, [&](const SM::Level& lv, int64_t b, int64_t i, int64_t row, double& acc) {
        int64_t base, stride;
        sph2pob_class::class_row_span(lv, K, b, i, &base, &stride);
        const int64_t lab = labels[row];
        float* g = !mining && lv.grad ? lv.grad + base : nullptr;
        if (!SM::valid_label(lab, K, ignore_index)) {
            if (mining) keys[(size_t)row] = SM::kKeyNone;
            if (g) softmax_zero_row(g, stride, K);
            return;
        }
        const float cwl = SM::class_factor(class_weight, lab), w = SM::row_weight(weight, row);
        const float l = SM::row_loss(softmax_row(lv.logits + base, g, stride, K, lab, k0 * (cwl * w)), cwl, w);
        if (!mining) acc += (double)l;
        else if (lab != background_label) { keys[(size_t)row] = SM::kKeyPos; acc += (double)l; }
        else keys[(size_t)row] = SM::loss_key(l);
    });
    if (mining) {
        // the cut of every image: the k_b-th largest negative key, the rows tied at it taken in index order
        std::vector<SM::Cut> cuts((size_t)num_images);
        std::vector<uint32_t> scratch;
        for (int64_t b = 0; b < (L.rows > 0 ? num_images : 0); b++) {
            const unsigned* kb = keys.data() + b * n;
            int64_t pos = 0, neg = 0;
            for (int64_t j = 0; j < n; j++) { pos += kb[j] == SM::kKeyPos; neg += kb[j] >= 2u; }
            const int64_t k = SM::mined_count(neg_pos_ratio, pos, neg);
            SM::Cut c{SM::kKeyNaN, 0};
            double sum = 0.0;
            if (k > 0) {
                const int64_t take = sph2pob_select::host_cut<true>(n, k, [&](int64_t j, uint32_t* key) { *key = kb[j]; return kb[j] >= 2u; }, scratch, &c);
                for (int64_t j = 0; j < n; j++)
                    if (kb[j] >= 2u && kb[j] > c.key) sum += (double)SM::key_loss(kb[j]);
                sum += (double)take * (double)SM::key_loss(c.key);
            }
            cuts[(size_t)b] = c;
            total += sum;
        }
        if (grads)
            head_rows_sum(L, L.rows, [&](const SM::Level& lv, int64_t b, int64_t i, int64_t row, double&) {
                int64_t base, stride;
                sph2pob_class::class_row_span(lv, K, b, i, &base, &stride);
                const unsigned key = keys[(size_t)row];
                if (key == SM::kKeyPos || SM::mined(key, (int)(row - b * n), cuts[(size_t)b])) {
                    const int64_t lab = labels[row];
                    softmax_row(lv.logits + base, lv.grad + base, stride, K, lab, k0 * (SM::class_factor(class_weight, lab) * SM::row_weight(weight, row)));
                } else {
                    softmax_zero_row(lv.grad + base, stride, K);
                }
            });
    }
    out[0] = (float)(total * (double)k0);
    return SPH2POB_OK;
}

int sph2pob_softmax_loss_fwd_f32_cpu(const float* logits, const int64_t* labels, const float* weight, const float* class_weight,
                                     int64_t ignore_index, float scale, float* loss, int64_t n, int64_t num_channels, void*) {
    if (int rc = SM::flat_check(n, num_channels, 0)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !loss) return SPH2POB_ERR_NULL;
    const int K = (int)num_channels;
    parallel_for(n, 1 << 10, [&](int64_t lo, int64_t hi) {
        for (int64_t row = lo; row < hi; row++) {
            const int64_t lab = labels[row];
            if (!SM::valid_label(lab, K, ignore_index)) { loss[row] = 0.0f; continue; }
            const float cwl = SM::class_factor(class_weight, lab), w = SM::row_weight(weight, row);
            loss[row] = scale * SM::row_loss(softmax_row(logits + row * K, nullptr, 1, K, lab, 0.0f), cwl, w);
        }
    });
    return SPH2POB_OK;
}

int sph2pob_softmax_loss_bwd_f32_cpu(const float* logits, const int64_t* labels, const float* weight, const float* class_weight,
                                     int64_t ignore_index, const float* grad_out, int grad_stride, float scale, const float* avg_factor,
                                     float* grad_logits, int64_t n, int64_t num_channels, void*) {
    if (int rc = SM::flat_check(n, num_channels, grad_stride)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !grad_out || !grad_logits) return SPH2POB_ERR_NULL;
    const int K = (int)num_channels;
    const float k0 = SM::effective_scale(scale, avg_factor);
    parallel_for(n, 1 << 10, [&](int64_t lo, int64_t hi) {
        for (int64_t row = lo; row < hi; row++) {
            const int64_t lab = labels[row];
            if (!SM::valid_label(lab, K, ignore_index)) { softmax_zero_row(grad_logits + row * K, 1, K); continue; }
            const float cwl = SM::class_factor(class_weight, lab), w = SM::row_weight(weight, row);
            softmax_row(logits + row * K, grad_logits + row * K, 1, K, lab, grad_out[grad_stride ? row : 0] * (k0 * (cwl * w)));
        }
    });
    return SPH2POB_OK;
}

}  // extern "C"

// ---- inference for softmax heads: the twins of sph2pob_softmax_bboxes.hip on the Prob and the level table of sph2pob_softmax.hpp ----
namespace {
// every row of every level: the three walks of Prob, the probabilities written without the background channel
void softmax_prob_rows(const SM::ProbLevels& L, const int64_t* level_n, int64_t B, int K) {
    for (int l = 0; l < L.num; l++) {
        const SM::ProbLevel& lv = L.lv[l];
        const float* x = (const float*)lv.logits;
        const int64_t n = level_n[l];
        parallel_for(B * n, 1 << 10, [&](int64_t lo, int64_t hi) {
            for (int64_t row = lo; row < hi; row++) {
                int64_t in = row * K, out = row * (K - 1), stride = 1;
                if (lv.hw > 0) {
                    const int64_t b = row / n, i = row - b * n, p = i / lv.a, a = i - p * lv.a;
                    SM::prob_nchw_span(b * lv.a + a, p, lv.hw, K, &in, &out);
                    stride = lv.hw;
                }
                SM::Prob r;
                r.begin();
                for (int j = 0; j < K; j++) r.see_max(x[in + j * stride]);
                for (int j = 0; j < K; j++) r.see_sum(x[in + j * stride]);
                for (int j = 0; j < K - 1; j++) lv.out[out + j * stride] = r.p(x[in + j * stride]);
            }
        });
    }
}
}  // namespace

extern "C" {

int sph2pob_softmax_scores_f32_cpu(const void* const* logits, const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                   int64_t num_classes, void* const* out, void*) {
    SM::ProbLevels L;
    if (int rc = SM::make_prob_levels(logits, out, level_n, level_hw, num_levels, num_images, num_classes, 4, &L)) return rc;
    softmax_prob_rows(L, level_n, num_images, (int)num_classes + 1);
    return SPH2POB_OK;
}

// stage 0 into buffers of its own, then the twin of the pipeline on them (the workspace is not used)
int sph2pob_softmax_bboxes_f32_cpu(const void* const* cls_scores, const void* const* bbox_preds, const void* const* anchors, const int64_t* level_n,
                                   const int64_t* level_hw, int num_levels, int64_t num_images, int64_t num_classes, int box_dim, float score_thr,
                                   int64_t nms_pre, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                                   float ctr_clamp, int variant, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                                   int64_t* labels, int64_t* prior_inds, int64_t* num_dets, void* workspace, void*) {
    (void)workspace;
    const GB::Shape sh{level_n, level_hw, num_levels, num_images, num_classes, box_dim};
    const GB::Selection sel{0, score_thr, nms_pre};
    const GB::Coder cd = GB::make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp);
    const GB::Nms nms{variant, class_agnostic, iou_threshold, max_per_img};
    const GB::Outputs outs{dets, labels, prior_inds, num_dets};
    GB::Levels G;
    if (int rc = SM::make_softmax_levels(cls_scores, bbox_preds, anchors, sh, sel, cd, nms, outs, &G)) return rc;
    SM::ProbLevels L;
    std::vector<std::vector<float>> probs(num_levels);
    void* out[GB::kMaxLevels];
    for (int l = 0; l < num_levels; l++) out[l] = const_cast<void*>(cls_scores[l]);   // (shapes first: nothing is sized before the checks)
    if (int rc = SM::make_prob_levels(cls_scores, out, level_n, level_hw, num_levels, num_images, num_classes, 4, &L)) return rc;
    for (int l = 0; l < num_levels; l++) {
        probs[l].resize((size_t)(num_images * level_n[l] * num_classes));
        G.lv[l].cls = L.lv[l].out = probs[l].data();   // the selection runs on the probabilities
    }
    softmax_prob_rows(L, level_n, num_images, (int)num_classes + 1);
    return delta_bboxes_cpu(G, sh, sel, cd, nms, outs);
}

}  // extern "C"

// ---- inference of the R-CNN stage: the twin of sph2pob_rcnn_bboxes.hip — Prob on the rows in front of every image's count (-inf
// behind it, nothing of those rows is read), the count of the valid candidates, then the twin of the pipeline on one flat level with
// RoiSource of sph2pob_rcnn_bboxes.hpp (the workspace is not used) ----
extern "C" {

int sph2pob_rcnn_bboxes_f32_cpu(const float* rois, const int64_t* num_rois, const float* cls_score, const float* bbox_pred, int64_t num_images,
                                int64_t m, int64_t row_stride, int64_t num_logits, int box_dim, int reg_class_agnostic, float score_thr,
                                int64_t max_candidates, const float* means_host, const float* stds_host, float max_ratio, int coder_flags,
                                float ctr_clamp, int variant, int class_agnostic, float iou_threshold, int64_t max_per_img, float* dets,
                                int64_t* labels, int64_t* prior_inds, int64_t* num_dets, int64_t* num_valid, void* workspace, void*) {
    (void)workspace;
    namespace RB = sph2pob_rcnn_bb;
    const GB::Shape sh{&m, nullptr, 1, num_images, num_logits - 1, box_dim};
    const GB::Selection sel{0, score_thr, max_candidates};
    const GB::Coder cd = GB::make_coder(means_host, stds_host, box_dim, max_ratio, coder_flags, ctr_clamp);
    const GB::Nms nms{variant, class_agnostic, iou_threshold, max_per_img};
    const GB::Outputs out{dets, labels, prior_inds, num_dets};
    GB::Levels L;
    if (int rc = RB::make_roi_level(sh, row_stride, reg_class_agnostic, sel, cd, nms, &L)) return rc;
    if (!rois || !cls_score || !num_valid || out.check(max_per_img)) return SPH2POB_ERR_NULL;
    const int K = (int)num_logits, C = K - 1;
    std::vector<float> probs((size_t)(num_images * m * C));
    parallel_for(num_images * m, 1 << 10, [&](int64_t lo, int64_t hi) {
        for (int64_t row = lo; row < hi; row++) {
            const int64_t b = row / m;
            float* o = probs.data() + row * C;
            if (row - b * m >= RB::live_rows(num_rois, b, (int)m)) {
                for (int j = 0; j < C; j++) o[j] = -INFINITY;
                continue;
            }
            const float* x = cls_score + row * K;
            SM::Prob r;
            r.begin();
            for (int j = 0; j < K; j++) r.see_max(x[j]);
            for (int j = 0; j < K; j++) r.see_sum(x[j]);
            for (int j = 0; j < C; j++) o[j] = r.p(x[j]);
        }
    });
    for (int64_t b = 0; b < num_images; b++) {
        const float* p = probs.data() + b * m * C;
        int64_t n = 0;
        for (int64_t i = 0; i < m * C; i++) n += p[i] > score_thr ? 1 : 0;
        num_valid[b] = n;
    }
    L.lv[0].cls = probs.data();
    const RB::Rois R = RB::make_rois(rois, num_rois, bbox_pred, m, row_stride, C, box_dim, reg_class_agnostic);
    return GB::with_dim(box_dim, [&](auto dim) { return bboxes_cpu(L, sh, sel, nms, out, RB::RoiSource<decltype(dim)::value>{R, cd, nullptr}); });
}

}  // extern "C"

// ---- random sampling of anchor targets: sph2pob_sample.hpp's host_select per image (the kernels' rank and sizes; the cut of a side
// by sph2pob_select.hpp's host_cut instead of the radix select), then the rows applied in place (the workspace is not used) ----
extern "C" {

int sph2pob_sample_targets_f32_cpu(const int64_t* gt_inds, int64_t num_images, int64_t n, int box_dim, const int64_t* labels_in,
                                   const float* label_weights_in, const float* bbox_targets_in, const float* bbox_weights_in,
                                   int64_t num_classes, int64_t num_expected_pos, int64_t num, double neg_pos_ub, int64_t seed,
                                   const int64_t* seed_device, const uint32_t* ranks, int64_t* labels, float* label_weights,
                                   float* bbox_targets, float* bbox_weights, unsigned char* sample_flags, int64_t* num_pos, int64_t* num_neg,
                                   float* avg_factor, float* avg_factor_pos, void*, void*) {
    namespace SA = sph2pob_sample;
    if (int rc = SA::check_shape(num_images, n, box_dim, num_expected_pos, num, neg_pos_ub)) return rc;
    if (!gt_inds || !labels_in || !label_weights_in || !bbox_targets_in || !bbox_weights_in || !labels || !label_weights || !bbox_targets ||
        !bbox_weights || !sample_flags || !num_pos || !num_neg || !avg_factor || !avg_factor_pos) return SPH2POB_ERR_NULL;
    const uint64_t sd = SA::seed_of(seed, seed_device);
    parallel_for(num_images, 1, [&](int64_t lo, int64_t hi) {
        std::vector<uint32_t> rank((size_t)n);
        std::vector<uint32_t> scratch;
        for (int64_t b = lo; b < hi; b++) {
            const int64_t* g = gt_inds + b * n;
            const auto pick = SA::host_select([&](int64_t i) { return g[i]; }, n, b, ranks ? ranks + b * n : nullptr, sd, num_expected_pos, num,
                                              neg_pos_ub, rank, scratch);
            num_pos[b] = pick[SA::POS].k; num_neg[b] = pick[SA::NEG].k;
            for (int64_t i = 0; i < n; i++) {
                const int64_t r = b * n + i;
                const int c = SA::side_of(g[i]);
                const bool in = c != SA::IGNORED && SA::sampled(rank[(size_t)i], i, pick[c]);
                sample_flags[r] = in ? (unsigned char)(c + 1) : (unsigned char)0;
                if (in || c == SA::IGNORED) {   // the row keeps its targets
                    if (labels != labels_in) labels[r] = labels_in[r];
                    if (label_weights != label_weights_in) label_weights[r] = label_weights_in[r];
                    for (int d = 0; d < box_dim; d++) {
                        if (bbox_targets != bbox_targets_in) bbox_targets[r * box_dim + d] = bbox_targets_in[r * box_dim + d];
                        if (bbox_weights != bbox_weights_in) bbox_weights[r * box_dim + d] = bbox_weights_in[r * box_dim + d];
                    }
                } else {
                    labels[r] = num_classes;
                    label_weights[r] = 0.0f;
                    for (int d = 0; d < box_dim; d++) { bbox_targets[r * box_dim + d] = 0.0f; bbox_weights[r * box_dim + d] = 0.0f; }
                }
            }
        }
    });
    int64_t sp = 0, sn = 0;
    for (int64_t b = 0; b < num_images; b++) { sp += std::max<int64_t>(num_pos[b], 1); sn += std::max<int64_t>(num_neg[b], 1); }
    avg_factor[0] = (float)(sp + sn);
    avg_factor_pos[0] = (float)sp;
    return SPH2POB_OK;
}

}  // extern "C"

// ---- R-CNN stage targets on per-image proposals: sph2pob_rcnn_targets_f32 after its checks (sph2pob_rcnn_targets.hpp).  Per image
// the pairwise and the assign twin above on its first n_b proposals, the candidate list, the sampler's host_select on it, and the
// kernels' table rows compacted in the kernels' order (the workspace is not used) ----
extern "C" {

int sph2pob_rcnn_targets_f32_cpu(const float* proposals, const int64_t* num_proposals, int64_t num_images, int64_t m, int64_t row_stride,
                                 const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets, int64_t num_gt, int64_t k_max, int box_dim,
                                 int variant, int edge, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi, float min_pos_iou,
                                 int match_low_quality, int gt_max_assign_all, int64_t num, int64_t num_expected_pos, double neg_pos_ub,
                                 int64_t seed, const int64_t* seed_device, const uint32_t* ranks, int add_gt, int64_t num_classes, float pos_weight,
                                 int encode, const float* means_host, const float* stds_host, float* rois, int64_t* labels, float* label_weights,
                                 float* bbox_targets, float* bbox_weights, int64_t* pos_assigned_gt_inds, int64_t* sample_inds,
                                 unsigned char* is_gt, int64_t* num_pos, int64_t* num_neg, float* avg_factor, float* num_samples, void* workspace,
                                 void*) {
    namespace RC = sph2pob_rcnn;
    namespace SA = sph2pob_sample;
    const RC::Table T{rois, labels, label_weights, bbox_targets, bbox_weights, pos_assigned_gt_inds, sample_inds, is_gt, num_pos, num_neg, avg_factor,
                      num_samples};
    if (int rc = RC::check(check_common(box_dim, variant, edge, 0), variant, proposals, num_images, m, row_stride, box_dim, gt, gt_offsets, num_gt,
                           k_max, num, num_expected_pos, neg_pos_ub, add_gt, encode, T, false, workspace))
        return rc;
    const int dim = box_dim;
    const sph2pob_coder::Norm nm = sph2pob_coder::make_norm(means_host, stds_host, box_dim);
    const auto sampled_row = dim == 4 ? (encode ? RC::write_sampled<4, true> : RC::write_sampled<4, false>)
                                      : (encode ? RC::write_sampled<5, true> : RC::write_sampled<5, false>);
    const auto padding_row = dim == 4 ? RC::write_padding<4> : RC::write_padding<5>;
    const uint64_t sd = SA::seed_of(seed, seed_device);
    const int64_t C = k_max + m;
    std::vector<float> boxes, ov, max_ov, gt_max;
    std::vector<int64_t> cand, argmax, gt_argmax;
    std::vector<uint32_t> rank((size_t)C), scratch;
    int64_t total = 0;
    for (int64_t b = 0; b < num_images; b++) {
        const sph2pob_assign::ImageRows im = sph2pob_assign::image_rows(gt_offsets, b, num_gt, k_max);
        const int64_t k = im.k, n = RC::image_proposals(num_proposals, b, m), koff = RC::gt_candidates(add_gt, k), count = koff + n;
        const float* gt_b = gt + im.lo * dim;
        const int64_t* labels_b = gt_labels ? gt_labels + im.lo : nullptr;
        cand.assign((size_t)count, 0);   // an image without GT: every proposal is background (max_iou_assigner.py:148-165)
        for (int64_t c = 0; c < koff; c++) cand[(size_t)c] = c + 1;
        if (k > 0 && n > 0) {
            boxes.resize((size_t)(n * dim)); ov.resize((size_t)(k * n)); max_ov.resize((size_t)n); argmax.resize((size_t)n);
            gt_max.resize((size_t)k); gt_argmax.resize((size_t)k);
            for (int64_t j = 0; j < n; j++)
                for (int d = 0; d < dim; d++) boxes[(size_t)(j * dim + d)] = proposals[(b * m + j) * row_stride + d];
            int rc = sph2pob_iou_pairwise_f32_cpu(gt_b, k, boxes.data(), n, ov.data(), box_dim, variant, SPH2POB_MODE_IOU, edge, SPH2POB_ANGLE_EQUATOR,
                                                  nullptr);
            if (!rc)
                rc = sph2pob_assign_f32_cpu(ov.data(), k, n, pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all,
                                            nullptr, max_ov.data(), argmax.data(), gt_max.data(), gt_argmax.data(), cand.data() + koff, nullptr,
                                            nullptr, nullptr);
            if (rc) return rc;
        }
        const auto pick = SA::host_select([&](int64_t c) { return cand[(size_t)c]; }, count, b, ranks ? ranks + b * C : nullptr, sd, num_expected_pos,
                                          num, neg_pos_ub, rank, scratch);
        num_pos[b] = pick[SA::POS].k; num_neg[b] = pick[SA::NEG].k;
        total += pick[SA::POS].k + pick[SA::NEG].k;
        int64_t r = b * num;
        for (int side = 0; side < 2; side++)   // positives in ascending c, then negatives in ascending c
            for (int64_t c = 0; c < count; c++) {
                const int64_t a = cand[(size_t)c];
                if (SA::side_of(a) != side || !SA::sampled(rank[(size_t)c], c, pick[side])) continue;
                const bool from_gt = c < koff;
                sampled_row(T, r++, b, c, a, from_gt, from_gt ? gt_b + c * dim : proposals + (b * m + c - koff) * row_stride, gt_b, labels_b, num_classes,
                            pos_weight, nm);
            }
        for (; r < (b + 1) * num; r++) padding_row(T, r, b, num_classes);
    }
    num_samples[0] = (float)total;
    avg_factor[0] = (float)std::max<int64_t>(total, 1);
    return SPH2POB_OK;
}

}  // extern "C"

// ---- point (FCOS) targets and the distance-point coder: the rows of sph2pob_point_targets.hpp, the kernels' arithmetic.  The
// centerness sum is taken in double per image and then over the images in order (the workspace is not used) ----
extern "C" {

int sph2pob_point_targets_f32_cpu(const float* points, int64_t num_points, const int64_t* level_n, const float* range_lo, const float* range_hi,
                                  const float* sample_extent, const float* norm_stride, int num_levels, const float* gt, const int64_t* gt_labels,
                                  const int64_t* gt_offsets, int64_t num_images, int64_t num_gt, int64_t k_max, int box_dim, int64_t img_h,
                                  int64_t img_w, int64_t num_classes, int flags, int64_t* labels, int64_t* gt_inds, float* bbox_targets,
                                  float* centerness, int64_t* num_pos, float* avg_factor, float* centerness_denorm, void*, void*) {
    namespace PT = sph2pob_point;
    if (int rc = PT::check_shape(num_points, level_n, num_levels, num_images, num_gt, k_max, box_dim, img_h, img_w, num_classes)) return rc;
    const int64_t rows = num_images * num_points;
    if (!range_lo || !range_hi || ((flags & SPH2POB_POINT_CENTER_SAMPLING) && !sample_extent) || ((flags & SPH2POB_POINT_NORM_ON_BBOX) && !norm_stride) ||
        !avg_factor || !centerness_denorm || (num_images > 0 && (!gt_offsets || !num_pos)) ||
        (rows > 0 && (!points || !labels || !gt_inds || !bbox_targets || !centerness)) ||
        (rows > 0 && k_max > 0 && (!gt || !gt_labels))) return SPH2POB_ERR_NULL;
    PT::Levels L;
    if (int rc = PT::make_levels(level_n, range_lo, range_hi, sample_extent, norm_stride, num_levels, flags, &L)) return rc;
    const bool center = (flags & SPH2POB_POINT_CENTER_SAMPLING) != 0;
    const float W = (float)img_w, H = (float)img_h;
    std::vector<double> sums((size_t)num_images, 0.0);
    parallel_for(num_images, 1, [&](int64_t lo, int64_t hi) {
        std::vector<PT::Gt> g;
        for (int64_t b = lo; b < hi; b++) {
            const int64_t off = gt_offsets[b];
            const int k = PT::image_rows(off, gt_offsets[b + 1], num_gt, k_max);
            g.resize((size_t)k);
            for (int j = 0; j < k; j++) g[(size_t)j] = PT::gt_pixels(gt + (off + j) * box_dim, box_dim, W, H);
            int64_t pos = 0;
            double sum = 0.0;
            for (int64_t p = 0; p < num_points; p++) {
                const PT::LevelRow lv = PT::level_of_point(L, (int)p);
                const float x = points[2 * p], y = points[2 * p + 1];
                PT::Best best = PT::no_best();
                for (int j = 0; j < k; j++) {
                    const bool cand = center ? PT::candidate<true>(g[(size_t)j], x, y, lv.lo, lv.hi, lv.extent)
                                             : PT::candidate<false>(g[(size_t)j], x, y, lv.lo, lv.hi, lv.extent);
                    PT::offer(best, g[(size_t)j], j, cand);
                }
                float t[5];
                const float cent = box_dim == 4 ? PT::target_row<4>(best, x, y, lv.norm, t) : PT::target_row<5>(best, x, y, lv.norm, t);
                const int64_t r = b * num_points + p;
                labels[r] = best.idx >= 0 ? gt_labels[off + best.idx] : num_classes;
                gt_inds[r] = best.idx + 1;
                centerness[r] = cent;
                for (int c = 0; c < box_dim; c++) bbox_targets[r * box_dim + c] = t[c];
                pos += best.idx >= 0;
                sum += (double)cent;
            }
            num_pos[b] = pos;
            sums[(size_t)b] = sum;
        }
    });
    int64_t tot = 0;
    double sum = 0.0;
    for (int64_t b = 0; b < num_images; b++) { tot += num_pos[b]; sum += sums[(size_t)b]; }
    PT::normalisers(tot, sum, avg_factor, centerness_denorm);
    return SPH2POB_OK;
}

}  // extern "C"

namespace {
// MODE as in the kernel: 0 encode, 1 decode, 2 decode backward
template <int DIM, int MODE>
void point_coder_rows(const float* points, const float* a, const float* g, float* out, int64_t n, const sph2pob_point::Image& im, bool clamp, float clamp_hi) {
    namespace PT = sph2pob_point;
    parallel_for(n, 1 << 12, [&](int64_t lo, int64_t hi) {
        for (int64_t i = lo; i < hi; i++) {
            float r[5];
            if (MODE == 0) PT::encode_row<DIM>(points + 2 * i, a + i * DIM, im, clamp, clamp_hi, r);
            else if (MODE == 1) PT::decode_row<DIM, false>(points + 2 * i, a + i * DIM, nullptr, im, r);
            else PT::decode_row<DIM, true>(points + 2 * i, a + i * DIM, g + i * DIM, im, r);
            for (int c = 0; c < DIM; c++) out[i * DIM + c] = r[c];
        }
    });
}
}  // namespace

extern "C" {

int sph2pob_point_coder_encode_f32_cpu(const float* points, const float* gt, float* distances, int64_t n, int box_dim, int64_t img_h, int64_t img_w,
                                       int clamp, double max_dis, double eps, void*) {
    namespace PT = sph2pob_point;
    const float hi = clamp ? (float)(max_dis - eps) : 0.0f;
    if (int rc = PT::check_coder(points, gt, gt, distances, n, box_dim, img_h, img_w, hi, 0.0f)) return rc;
    if (clamp != 0 && clamp != 1) return SPH2POB_ERR_OPTION;
    const PT::Image im{(float)img_w, (float)img_h, -1.0f, -1.0f};
    if (box_dim == 4) point_coder_rows<4, 0>(points, gt, nullptr, distances, n, im, clamp != 0, hi);
    else point_coder_rows<5, 0>(points, gt, nullptr, distances, n, im, clamp != 0, hi);
    return SPH2POB_OK;
}

int sph2pob_point_coder_decode_f32_cpu(const float* points, const float* distances, float* boxes, int64_t n, int box_dim, int64_t img_h,
                                       int64_t img_w, float max_h, float max_w, void*) {
    namespace PT = sph2pob_point;
    if (int rc = PT::check_coder(points, distances, distances, boxes, n, box_dim, img_h, img_w, max_h, max_w)) return rc;
    const PT::Image im{(float)img_w, (float)img_h, max_w, max_h};
    if (box_dim == 4) point_coder_rows<4, 1>(points, distances, nullptr, boxes, n, im, false, 0.0f);
    else point_coder_rows<5, 1>(points, distances, nullptr, boxes, n, im, false, 0.0f);
    return SPH2POB_OK;
}

int sph2pob_point_coder_decode_bwd_f32_cpu(const float* points, const float* distances, const float* grad_boxes, float* grad_distances, int64_t n,
                                           int box_dim, int64_t img_h, int64_t img_w, float max_h, float max_w, void*) {
    namespace PT = sph2pob_point;
    if (int rc = PT::check_coder(points, distances, grad_boxes, grad_distances, n, box_dim, img_h, img_w, max_h, max_w)) return rc;
    const PT::Image im{(float)img_w, (float)img_h, max_w, max_h};
    if (box_dim == 4) point_coder_rows<4, 2>(points, distances, grad_boxes, grad_distances, n, im, false, 0.0f);
    else point_coder_rows<5, 2>(points, distances, grad_boxes, grad_distances, n, im, false, 0.0f);
    return SPH2POB_OK;
}

}  // extern "C"

// ---- the RoI feature extractor: the twins of sph2pob_roi_extract.hip — prepare_row, axis_entry and the bin sums of
// sph2pob_roi_extract.hpp, the axis entries recomputed per use.  Forward: the rois in parallel, every output one fixed-order sum.
// Backward: one thread, the rois, channels, bins and samples in ascending order — a fixed order where the kernel's atomics have none ----
namespace {
namespace RE = sph2pob_roi;
struct RoiAxis {
    float start, bin; int g, n;
    RE::Axis operator()(int k) const { const int q = k / g; return RE::axis_entry(start, bin, g, q, k - q * g, n); }
};
}  // namespace

extern "C" {

int sph2pob_roi_extract_fwd_f32_cpu(const float* const* feats, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                                    int64_t num_images, int64_t channels, const float* rois, int64_t rows, int64_t row_stride, int form, int64_t m,
                                    const int64_t* num_rois, int box_dim, int64_t img_h, int64_t img_w, int pooled_h, int pooled_w,
                                    int sampling_ratio, int aligned, float finest_scale, float* roi_feats, float* rois_xyxy, int32_t* levels,
                                    void* prep, void*) {
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (int rc = RE::check_options(form, m, row_stride, rows, num_images, box_dim, img_h, img_w, sampling_ratio, aligned, finest_scale)) return rc;
    RE::Levels L;
    if (int rc = RE::make_levels(const_cast<float* const*>(feats), false, heights, widths, strides, num_levels, num_images, channels, box_dim,
                                 pooled_h, pooled_w, rows, &L))
        return rc;
    if (L.num == 0) return SPH2POB_OK;
    if (!rois || !roi_feats || !rois_xyxy || !levels || !prep) return SPH2POB_ERR_NULL;
    const RE::Options o{box_dim, form, rows, form == 1 ? m : 1, row_stride, (int)num_images, (int)channels, (float)img_h, (float)img_w, finest_scale,
                        pooled_h, pooled_w, sampling_ratio, aligned};
    RE::Prep* records = static_cast<RE::Prep*>(prep);
    const int bins = pooled_h * pooled_w;
    parallel_for(rows, 8, [&](int64_t lo, int64_t hi) {
        for (int64_t r = lo; r < hi; r++) {
            records[r] = RE::prepare_row(L, o, rois, num_rois, r, rois_xyxy + r * 4);
            levels[r] = records[r].lvl;
            const RE::Prep p = RE::checked(records[r], L.num, (int)num_images);
            float* out = roi_feats + r * channels * bins;
            if (p.b < 0 || p.gh == 0 || p.gw == 0) {
                for (int64_t i = 0; i < channels * bins; i++) out[i] = 0.0f;
                continue;
            }
            const RE::Level lv = L.lv[p.lvl];
            const RoiAxis ty{p.sh, p.bin_h, p.gh, lv.h}, tx{p.sw, p.bin_w, p.gw, lv.w};
            const int64_t plane = (int64_t)lv.h * lv.w;
            for (int64_t c = 0; c < channels; c++)
                for (int y = 0; y < pooled_h; y++)
                    for (int x = 0; x < pooled_w; x++)
                        out[c * bins + y * pooled_w + x] = RE::bin_forward(lv.feat + (p.b * channels + c) * plane, lv.w, p, y, x, ty, tx);
        }
    });
    return SPH2POB_OK;
}

int sph2pob_roi_extract_bwd_f32_cpu(float* const* grad_feats, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                                    int64_t num_images, int64_t channels, const float* grad_out, int64_t rows, int box_dim, int pooled_h,
                                    int pooled_w, const void* prep, int zero_first, void*) {
    if (zero_first < 0 || zero_first > 1) return (box_dim != 4 && box_dim != 5) ? SPH2POB_ERR_DIM : SPH2POB_ERR_OPTION;
    RE::Levels L;
    if (int rc = RE::make_levels(grad_feats, true, heights, widths, strides, num_levels, num_images, channels, box_dim, pooled_h, pooled_w, rows, &L))
        return rc;
    if (L.num == 0) return SPH2POB_OK;
    if (!grad_out || !prep) return SPH2POB_ERR_NULL;
    if (zero_first)
        for (int l = 0; l < L.num; l++) memset(L.lv[l].grad, 0, sizeof(float) * num_images * channels * L.lv[l].h * L.lv[l].w);
    const RE::Prep* records = static_cast<const RE::Prep*>(prep);
    const int bins = pooled_h * pooled_w;
    for (int64_t r = 0; r < rows; r++) {
        const RE::Prep p = RE::checked(records[r], L.num, (int)num_images);
        if (p.b < 0 || p.gh == 0 || p.gw == 0) continue;
        const RE::Level lv = L.lv[p.lvl];
        const RoiAxis ty{p.sh, p.bin_h, p.gh, lv.h}, tx{p.sw, p.bin_w, p.gw, lv.w};
        const int64_t plane = (int64_t)lv.h * lv.w;
        const float count = RE::bin_count(p);
        for (int64_t c = 0; c < channels; c++) {
            float* g = lv.grad + (p.b * channels + c) * plane;
            for (int y = 0; y < pooled_h; y++)
                for (int x = 0; x < pooled_w; x++)
                    RE::bin_backward(lv.w, p, y, x, grad_out[(r * channels + c) * bins + y * pooled_w + x] / count, ty, tx,
                                     [g](int64_t at, float v) { g[at] += v; });
        }
    }
    return SPH2POB_OK;
}

// The gather form of the adjoint (csrc/sph2pob_roi_extract.hpp states its order and its bound) — an entry of this library alone:
// no device kernel computes it yet, so include/sph2pob_hip.h does not declare the name.  The arguments of
// sph2pob_roi_extract_bwd_f32 and, in front of the stream, the scratch a device route would need: not read here, NULL is fine.
// One thread: the rows in ascending order — so every pixel takes its rois in ascending row index — into a sum of its own per level,
// which the gradient buffer then takes once (zero_first = 1: the sum itself; 0: its value + the sum).  Per row the Wy, Wx of its
// reach (axis_weight), per channel and pixel of the reach t_r (gather_term over the bins with a term on both axes).  The result
// does not depend on sph2pob_host_threads()
int sph2pob_roi_extract_bwd_det_f32_cpu(float* const* grad_feats, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                                        int64_t num_images, int64_t channels, const float* grad_out, int64_t rows, int box_dim, int pooled_h,
                                        int pooled_w, const void* prep, int zero_first, void*, void*) {
    if (zero_first < 0 || zero_first > 1) return (box_dim != 4 && box_dim != 5) ? SPH2POB_ERR_DIM : SPH2POB_ERR_OPTION;
    RE::Levels L;
    if (int rc = RE::make_levels(grad_feats, true, heights, widths, strides, num_levels, num_images, channels, box_dim, pooled_h, pooled_w, rows, &L))
        return rc;
    if (L.num == 0) return SPH2POB_OK;
    if (!grad_out || !prep) return SPH2POB_ERR_NULL;
    std::vector<std::vector<float>> sums(L.num);
    for (int l = 0; l < L.num; l++) sums[l].assign((size_t)(num_images * channels * L.lv[l].h * L.lv[l].w), 0.0f);
    const RE::Prep* records = static_cast<const RE::Prep*>(prep);
    const int bins = pooled_h * pooled_w;
    std::vector<float> wy, wx, g(bins);
    std::vector<char> fy, fx;
    std::vector<int> ylo, yhi, xlo, xhi;
    for (int64_t r = 0; r < rows; r++) {
        const RE::Prep p = RE::checked(records[r], L.num, (int)num_images);
        if (p.b < 0 || p.gh == 0 || p.gw == 0) continue;
        const RE::Level lv = L.lv[p.lvl];
        int y0, y1, x0, x1;
        RE::axis_reach(p.sh, p.bin_h, pooled_h, lv.h, y0, y1);
        RE::axis_reach(p.sw, p.bin_w, pooled_w, lv.w, x0, x1);
        const int fh = y1 - y0 + 1, fw = x1 - x0 + 1;
        wy.assign((size_t)pooled_h * fh, 0.0f); fy.assign((size_t)pooled_h * fh, 0);
        wx.assign((size_t)pooled_w * fw, 0.0f); fx.assign((size_t)pooled_w * fw, 0);
        for (int q = 0; q < pooled_h; q++)
            for (int y = 0; y < fh; y++) {
                int terms;
                wy[(size_t)q * fh + y] = RE::axis_weight(p.sh, p.bin_h, p.gh, q, lv.h, y0 + y, terms);
                fy[(size_t)q * fh + y] = terms > 0;
            }
        for (int q = 0; q < pooled_w; q++)
            for (int x = 0; x < fw; x++) {
                int terms;
                wx[(size_t)q * fw + x] = RE::axis_weight(p.sw, p.bin_w, p.gw, q, lv.w, x0 + x, terms);
                fx[(size_t)q * fw + x] = terms > 0;
            }
        // the bins [lo, hi) between a pixel's first and last flagged one: the loops below test the flags inside
        ylo.assign(fh, pooled_h); yhi.assign(fh, 0); xlo.assign(fw, pooled_w); xhi.assign(fw, 0);
        for (int q = 0; q < pooled_h; q++)
            for (int y = 0; y < fh; y++)
                if (fy[(size_t)q * fh + y]) { ylo[y] = std::min(ylo[y], q); yhi[y] = q + 1; }
        for (int q = 0; q < pooled_w; q++)
            for (int x = 0; x < fw; x++)
                if (fx[(size_t)q * fw + x]) { xlo[x] = std::min(xlo[x], q); xhi[x] = q + 1; }
        const int64_t plane = (int64_t)lv.h * lv.w;
        const float count = RE::bin_count(p);
        for (int64_t c = 0; c < channels; c++) {
            for (int k = 0; k < bins; k++) g[k] = grad_out[(r * channels + c) * bins + k] / count;
            float* sum = sums[p.lvl].data() + (p.b * channels + c) * plane;
            for (int y = 0; y < fh; y++)
                for (int x = 0; x < fw; x++) {
                    float t = 0.0f;
                    bool reached = false;
                    for (int qy = ylo[y]; qy < yhi[y]; qy++) {
                        if (!fy[(size_t)qy * fh + y]) continue;
                        for (int qx = xlo[x]; qx < xhi[x]; qx++) {
                            if (!fx[(size_t)qx * fw + x]) continue;
                            t = RE::gather_term(t, g[qy * pooled_w + qx], wy[(size_t)qy * fh + y], wx[(size_t)qx * fw + x]);
                            reached = true;
                        }
                    }
                    if (reached) sum[(int64_t)(y0 + y) * lv.w + (x0 + x)] += t;
                }
        }
    }
    for (int l = 0; l < L.num; l++) {
        float* grad = L.lv[l].grad;
        const std::vector<float>& sum = sums[l];
        for (size_t i = 0; i < sum.size(); i++) grad[i] = zero_first ? sum[i] : grad[i] + sum[i];
    }
    return SPH2POB_OK;
}

}  // extern "C"
