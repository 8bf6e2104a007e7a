// Sigmoid binary cross-entropy kernel (the arithmetic and the checks: sph2pob_bce_loss.hpp).
//   bce_sum_kernel      ONE grid over all levels of a head, the item shapes of focal_sum_kernel (sph2pob_focal.hip) restated for a
//                       float target: a thread owns four consecutive positions of one (image, anchor) of an NCHW level and walks
//                       the C channel planes with 16-byte loads / stores at stride H W (NCHW4), or one position (NCHW1); four
//                       consecutive elements of a flat level (FLAT4), or one (FLAT1).  Hard labels and row weights are loaded once
//                       per position; soft targets and element weights are gathered from their (B, n, C) rows.  The weighted
//                       losses are added in double and leave one partial per workgroup
//   head_final_kernel   (sph2pob_head_loss.hpp) adds the partials in a fixed order
// Every element is evaluated and multiplied by its weight (a zero weight gives a zero, not a skipped read), as in the focal loss.
#include "sph2pob_bce_loss.hpp"

namespace {

using namespace sph2pob_bce;

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&x)[V]) {
    if constexpr (V == 4) { const float4 v = *reinterpret_cast<const float4*>(p); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
    else x[0] = p[0];
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&x)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else p[0] = x[0];
}

// NCHW: item -> (b, a, V consecutive positions); the sum of the item's weighted losses
template <int V, bool GRAD, bool HARD>
__device__ __forceinline__ double nchw_item(const Level& lv, int item, int C, int64_t n_total, const Targets& T, float k0) {
    const int per = lv.hw / V;
    const int ba = item / per, pq = item - ba * per;
    const int b = ba / lv.a, a = ba - b * lv.a;
    const int p0 = pq * V;
    const int64_t row0 = (int64_t)b * n_total + lv.row_off + (int64_t)p0 * lv.a + a;   // anchor (h W + w) A + a; the next position: + A
    int64_t lab[V];
    float w[V];
#pragma unroll
    for (int v = 0; v < V; v++) {
        const int64_t row = row0 + (int64_t)v * lv.a;
        lab[v] = HARD ? T.hard[row] : 0;
        w[v] = T.wmode == 1 ? T.weight[row] : 1.0f;
        if (HARD && !label_valid(lab[v], T.ignore)) w[v] = 0.0f;
    }
    const int64_t base = (int64_t)ba * C * lv.hw + p0;   // channel 0 of anchor a
    const float* x = lv.logits + base;
    float* g = GRAD ? lv.grad + base : nullptr;
    double acc = 0.0;
    for (int c = 0; c < C; c++) {
        float xv[V], gv[V];
        load_v<V>(x + (int64_t)c * lv.hw, xv);
#pragma unroll
        for (int v = 0; v < V; v++) {
            const int64_t row = row0 + (int64_t)v * lv.a;
            float t, we = w[v];
            if (HARD) {
                t = lab[v] == (int64_t)c ? 1.0f : 0.0f;
                if (T.wmode == 2) we = label_valid(lab[v], T.ignore) ? T.weight[row * C + c] : 0.0f;
            } else {
                t = T.soft[row * C + c];
                if (T.wmode == 2) we = T.weight[row * C + c];
                if (!soft_valid(t, T.ignore)) we = 0.0f;
            }
            float loss, dx;
            element(xv[v], t, loss, dx);
            acc += (double)(loss * we);
            gv[v] = (k0 * we) * dx;
        }
        if (GRAD) store_v<V>(g + (int64_t)c * lv.hw, gv);
    }
    return acc;
}

// flat (B, n_l, C): item -> V consecutive elements of the level
template <int V, bool GRAD, bool HARD>
__device__ __forceinline__ double flat_item(const Level& lv, int item, int C, int64_t n_total, const Targets& T, float k0) {
    const unsigned e0 = (unsigned)item * V;
    unsigned r = e0 / (unsigned)C;           // row inside the level: b n_l + i
    int c = (int)(e0 - r * (unsigned)C);
    float xv[V], gv[V];
    load_v<V>(lv.logits + e0, xv);
    double acc = 0.0;
#pragma unroll
    for (int v = 0; v < V; v++) {
        const unsigned b = r / (unsigned)lv.n;
        const int64_t row = (int64_t)b * n_total + lv.row_off + (r - b * (unsigned)lv.n);
        float t, we, loss, dx;
        target_weight<HARD>(T, row, C, c, t, we);
        element(xv[v], t, loss, dx);
        acc += (double)(loss * we);
        gv[v] = (k0 * we) * dx;
        if (++c == C) { c = 0; r++; }
    }
    if (GRAD) store_v<V>(lv.grad + e0, gv);
    return acc;
}

template <bool GRAD, bool HARD>
__global__ __launch_bounds__(kBlock) void bce_sum_kernel(Levels L, int C, Targets T, float scale, const float* __restrict__ avg_factor,
                                                         double* __restrict__ partial) {
    const int l = level_of_block(L, blockIdx.x);
    const Level& lv = L.lv[l];
    const int item = ((int)blockIdx.x - lv.block_off) * kBlock + (int)threadIdx.x;
    const float k0 = GRAD ? effective_scale(scale, avg_factor) : 0.0f;
    double acc = 0.0;
    if (item < lv.items) {
        switch (lv.kind) {   // workgroup-uniform
            case KIND_NCHW4: acc = nchw_item<4, GRAD, HARD>(lv, item, C, L.n_total, T, k0); break;
            case KIND_NCHW1: acc = nchw_item<1, GRAD, HARD>(lv, item, C, L.n_total, T, k0); break;
            case KIND_FLAT4: acc = flat_item<4, GRAD, HARD>(lv, item, C, L.n_total, T, k0); break;
            default: acc = flat_item<1, GRAD, HARD>(lv, item, C, L.n_total, T, k0); break;
        }
    }
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

}  // namespace

extern "C" {

int64_t sph2pob_bce_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                         int64_t num_channels) {
    return 8 * workspace_doubles(level_n, level_hw, num_levels, num_images, num_channels);
}

int sph2pob_bce_loss_sum_f32(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                             int num_levels, int64_t num_images, int64_t num_channels, const float* targets, const int64_t* labels,
                             const float* weight, int weight_mode, int64_t ignore_index, float scale, const float* avg_factor, float* out,
                             void* workspace, void* stream) {
    Levels L;
    if (int rc = make_levels(logits, grads, level_n, level_hw, num_levels, num_images, num_channels, weight_mode, true, &L)) return rc;
    if (int rc = check_tensors(L, targets, labels, weight, weight_mode, out, workspace)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Targets T{targets, labels, weight, weight_mode, ignore_index};
    double* partial = (double*)workspace;
    if (L.blocks > 0) {
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(kBlock), 0, s, L, (int)num_channels, T, scale, avg_factor, partial);
        };
        if (grads) { if (labels) go(bce_sum_kernel<true, true>); else go(bce_sum_kernel<true, false>); }
        else { if (labels) go(bce_sum_kernel<false, true>); else go(bce_sum_kernel<false, false>); }
    }
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

}  // extern "C"
