// Sigmoid focal loss kernels (the arithmetic: sph2pob_focal.hpp).
//   focal_sum_kernel    ONE grid over all levels of a head: a workgroup finds its level in the table (as topk_hist does), a
//                       thread owns four consecutive positions of one (image, anchor) of an NCHW level, loads their labels and
//                       weights once and walks the C class planes with 16-byte loads / stores at stride H W; the weighted losses
//                       are added in double and leave one partial per workgroup
//   head_final_kernel   (sph2pob_head_loss.hpp) adds the partials in a fixed order
//   focal_fwd / focal_bwd / focal_grad_scale   the flat (N, C) element forms and the stash scaling of torch's backward
// The stream is 4 bytes in and 4 bytes out per element; per element the VALU sees one expf, one log1pf and one division.
#include "sph2pob_focal.hpp"

namespace {

using namespace sph2pob_focal;

// V consecutive elements of a level of element type T (float, or the 16-bit types of the _h16 entry), as fp32: one 16-byte
// access for four floats, one 8-byte access for four 16-bit values
template <int V, class T>
__device__ __forceinline__ void load_v(const T* p, float (&x)[V]) {
    if constexpr (V == 4 && std::is_same<T, float>::value) { const float4 v = *reinterpret_cast<const float4*>(p); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
    else if constexpr (V == 4) load4(p, x);
    else x[0] = load1(p);
}
template <int V, class T>
__device__ __forceinline__ void store_v(T* p, const float (&x)[V]) {
    if constexpr (V == 4 && std::is_same<T, float>::value) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else if constexpr (V == 4) store4(p, x[0], x[1], x[2], x[3]);
    else store1(p, x[0]);
}

// the gradient value of one element: (k0 w) dx for fp32 levels, whose upstream gradient torch's backward applies to the stash;
// g ((k0 w) dx) for 16-bit levels, the upstream gradient folded in before the one narrowing
template <class T>
__device__ __forceinline__ float grad_value(float k0w, float dx, float gs) {
    if constexpr (std::is_same<T, float>::value) return k0w * dx;
    else return gs * (k0w * dx);
}

// NCHW: item -> (b, a, V consecutive positions); the sum of the item's weighted losses
template <class T, int V, bool GRAD>
__device__ __forceinline__ double nchw_item(const Level& lv, int item, int C, int64_t n_total, const int64_t* __restrict__ labels,
                                            const float* __restrict__ weight, int wmode, const Params& P, float k0, float gs) {
    const int per = lv.hw / V;
    const int ba = item / per, pq = item - ba * per;
    const int b = ba / lv.a, a = ba - b * lv.a;
    const int p0 = pq * V;
    const int64_t row0 = (int64_t)b * n_total + lv.row_off + (int64_t)p0 * lv.a + a;   // anchor (h W + w) A + a; the next position: + A
    int64_t lab[V];
    float w[V];
#pragma unroll
    for (int v = 0; v < V; v++) {
        lab[v] = labels[row0 + (int64_t)v * lv.a];
        w[v] = wmode == 1 ? weight[row0 + (int64_t)v * lv.a] : 1.0f;
    }
    const int64_t base = (int64_t)ba * C * lv.hw + p0;   // class 0 of channel a C
    const T* x = level_ptr<T>(lv.logits) + base;
    T* g = GRAD ? level_ptr<T>(lv.grad) + base : nullptr;
    double acc = 0.0;
    for (int c0 = 0; c0 < C; c0 += 4) {
        float xv[4][V];
#pragma unroll
        for (int j = 0; j < 4; j++) {   // four planes in flight before the first is used
            const int c = c0 + j < C ? c0 + j : C - 1;
            load_v<V>(x + (int64_t)c * lv.hw, xv[j]);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int c = c0 + j;
            if (c < C) {   // wave-uniform
                float gv[V];
#pragma unroll
                for (int v = 0; v < V; v++) {
                    float loss, dx;
                    element(xv[j][v], lab[v] == (int64_t)c, P, loss, dx);
                    const float we = wmode == 2 ? weight[(row0 + (int64_t)v * lv.a) * C + c] : w[v];
                    acc += (double)(loss * we);
                    gv[v] = grad_value<T>(k0 * we, dx, gs);
                }
                if (GRAD) store_v<V>(g + (int64_t)c * lv.hw, gv);
            }
        }
    }
    return acc;
}

// flat (B, n_l, C): item -> V consecutive elements of the level
template <class T, int V, bool GRAD>
__device__ __forceinline__ double flat_item(const Level& lv, int item, int C, int64_t n_total, const int64_t* __restrict__ labels,
                                            const float* __restrict__ weight, int wmode, const Params& P, float k0, float gs) {
    const unsigned e0 = (unsigned)item * V;
    unsigned r = e0 / (unsigned)C;           // row inside the level: b n_l + i
    int c = (int)(e0 - r * (unsigned)C);
    float xv[V], gv[V];
    load_v<V>(level_ptr<T>(lv.logits) + e0, xv);
    double acc = 0.0;
#pragma unroll
    for (int v = 0; v < V; v++) {
        const unsigned b = r / (unsigned)lv.n;
        const int64_t row = (int64_t)b * n_total + lv.row_off + (r - b * (unsigned)lv.n);
        float loss, dx;
        element(xv[v], labels[row] == (int64_t)c, P, loss, dx);
        const float we = weight_of(weight, wmode, row, C, c);
        acc += (double)(loss * we);
        gv[v] = grad_value<T>(k0 * we, dx, gs);
        if (++c == C) { c = 0; r++; }
    }
    if (GRAD) store_v<V>(level_ptr<T>(lv.grad) + e0, gv);
    return acc;
}

// The two kernels below hold the same dispatch — the workgroup's level, the thread's item, the level's kind — once per signature:
// the fp32 kernel keeps the code (and the ISA) it had before the 16-bit levels.
template <bool GRAD>
__global__ __launch_bounds__(kBlock) void focal_sum_kernel(Levels L, int C, const int64_t* __restrict__ labels, const float* __restrict__ weight,
                                                           int wmode, Params P, float scale, const float* __restrict__ avg_factor,
                                                           double* __restrict__ partial) {
    const int l = level_of_block(L, blockIdx.x);
    const Level& lv = L.lv[l];
    const int item = ((int)blockIdx.x - lv.block_off) * kBlock + (int)threadIdx.x;
    const float k0 = GRAD ? effective_scale(scale, avg_factor) : 0.0f;
    double acc = 0.0;
    if (item < lv.items) {
        switch (lv.kind) {   // workgroup-uniform
            case KIND_NCHW4: acc = nchw_item<float, 4, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, 1.0f); break;
            case KIND_NCHW1: acc = nchw_item<float, 1, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, 1.0f); break;
            case KIND_FLAT4: acc = flat_item<float, 4, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, 1.0f); break;
            default: acc = flat_item<float, 1, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, 1.0f); break;
        }
    }
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// 16-bit levels (sph2pob_focal_loss_sum_h16): the same items; the gradient leaves as RNE_T(g ((k0 w) dx)).  partial NULL: a
// gradient-only call (torch's backward), no sum
template <class T, bool GRAD>
__global__ __launch_bounds__(kBlock) void focal_sum_h16_kernel(Levels L, int C, const int64_t* __restrict__ labels, const float* __restrict__ weight,
                                                               int wmode, Params P, float scale, const float* __restrict__ avg_factor,
                                                               const float* __restrict__ grad_out, int skip_if_one, double* __restrict__ partial) {
    bool done;
    const float gs = upstream_gradient(grad_out, skip_if_one, done);
    if (done) return;   // kernel-uniform
    const int l = level_of_block(L, blockIdx.x);
    const Level& lv = L.lv[l];
    const int item = ((int)blockIdx.x - lv.block_off) * kBlock + (int)threadIdx.x;
    const float k0 = GRAD ? effective_scale(scale, avg_factor) : 0.0f;
    double acc = 0.0;
    if (item < lv.items) {
        switch (lv.kind) {   // workgroup-uniform
            case KIND_NCHW4: acc = nchw_item<T, 4, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, gs); break;
            case KIND_NCHW1: acc = nchw_item<T, 1, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, gs); break;
            case KIND_FLAT4: acc = flat_item<T, 4, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, gs); break;
            default: acc = flat_item<T, 1, GRAD>(lv, item, C, L.n_total, labels, weight, wmode, P, k0, gs); break;
        }
    }
    if (!partial) return;   // kernel-uniform
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

__global__ __launch_bounds__(kBlock) void focal_fwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ weight, int wmode, Params P, float scale,
                                                           float* __restrict__ out, int64_t total, int C) {
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t row = e / C;
        const int c = (int)(e - row * C);
        float loss, dx;
        element(x[e], labels[row] == (int64_t)c, P, loss, dx);
        out[e] = (scale * weight_of(weight, wmode, row, C, c)) * loss;
    }
}

__global__ __launch_bounds__(kBlock) void focal_bwd_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                           const float* __restrict__ weight, int wmode, const float* __restrict__ g,
                                                           int stride, Params P, float scale, const float* __restrict__ avg_factor,
                                                           float* __restrict__ out, int64_t total, int C) {
    const float k0 = effective_scale(scale, avg_factor);
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) {
        const int64_t row = e / C;
        const int c = (int)(e - row * C);
        float loss, dx;
        element(x[e], labels[row] == (int64_t)c, P, loss, dx);
        out[e] = g[stride ? e : 0] * ((k0 * weight_of(weight, wmode, row, C, c)) * dx);
    }
}

// out[e] = stash[e] * g[0]; in place with g[0] == 1 (a plain loss.backward()) the stash already is the gradient
__global__ __launch_bounds__(kBlock) void focal_grad_scale_kernel(const float* stash, const float* __restrict__ g, float* out, int64_t total) {
    if (out == stash && g[0] == 1.0f) return;
    const float s = g[0];
    for (int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x; e < total; e += (int64_t)gridDim.x * kBlock) out[e] = stash[e] * s;
}

unsigned capped_blocks(int64_t total) {
    int64_t blocks = (total + kBlock - 1) / kBlock;
    const int64_t cap = (int64_t)cu_count() * 8;
    return (unsigned)(blocks > cap ? cap : blocks);
}

}  // namespace

extern "C" {

int64_t sph2pob_focal_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                           int64_t num_classes) {
    return 8 * workspace_doubles(level_n, level_hw, num_levels, num_images, num_classes);
}

int sph2pob_focal_loss_sum_f32(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int64_t num_classes, const int64_t* labels, const float* weight,
                               int weight_mode, float gamma, float alpha, float scale, const float* avg_factor, float* out,
                               void* workspace, void* stream) {
    Levels L;
    if (int rc = make_levels(logits, grads, level_n, level_hw, num_levels, num_images, num_classes, weight_mode, gamma, true, &L)) return rc;
    if (!out || !workspace || (L.elems > 0 && (!labels || (weight_mode != 0 && !weight)))) return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const Params P = make_params(gamma, alpha);
    double* partial = (double*)workspace;
    if (L.blocks > 0) {
        if (grads)
            hipLaunchKernelGGL(focal_sum_kernel<true>, dim3(L.blocks), dim3(kBlock), 0, s, L, (int)num_classes, labels, weight, weight_mode, P,
                               scale, avg_factor, partial);
        else
            hipLaunchKernelGGL(focal_sum_kernel<false>, dim3(L.blocks), dim3(kBlock), 0, s, L, (int)num_classes, labels, weight, weight_mode, P,
                               scale, avg_factor, partial);
    }
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

int sph2pob_focal_loss_sum_h16(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                               int num_levels, int64_t num_images, int64_t num_classes, const int64_t* labels, const float* weight,
                               int weight_mode, float gamma, float alpha, float scale, const float* avg_factor, float* out,
                               void* workspace, const float* grad_out, int skip_if_one, int dtype, void* stream) {
    if (!sph2pob_head::h16_dtype_ok(dtype)) return SPH2POB_ERR_OPTION;
    Levels L;
    if (int rc = make_levels(logits, grads, level_n, level_hw, num_levels, num_images, num_classes, weight_mode, gamma, true, &L, 8)) return rc;
    if ((out && !workspace) || (L.elems > 0 && (!labels || (weight_mode != 0 && !weight)))) return SPH2POB_ERR_NULL;
    if (!out && !grads) return SPH2POB_OK;   // neither the sum nor the gradient is asked for
    hipStream_t s = (hipStream_t)stream;
    const Params P = make_params(gamma, alpha);
    double* partial = out ? (double*)workspace : nullptr;
    if (L.blocks > 0) {
        by_h16_dtype(dtype, [&](auto t) {
            using T = decltype(t);
            auto go = [&](auto kernel) {
                hipLaunchKernelGGL(kernel, dim3(L.blocks), dim3(kBlock), 0, s, L, (int)num_classes, labels, weight, weight_mode, P, scale,
                                   avg_factor, grads ? grad_out : nullptr, skip_if_one, partial);
            };
            if (grads) go(focal_sum_h16_kernel<T, true>);
            else go(focal_sum_h16_kernel<T, false>);
        });
    }
    if (!out) return L.blocks > 0 ? launch_status() : SPH2POB_OK;
    return launch_final(partial, L.blocks, scale, avg_factor, out, s);
}

int sph2pob_focal_loss_fwd_f32(const float* logits, const int64_t* labels, const float* weight, int weight_mode, float gamma, float alpha,
                               float scale, float* loss, int64_t n, int64_t num_classes, void* stream) {
    if (int rc = flat_check(n, num_classes, weight_mode, gamma, 0)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !loss || (weight_mode != 0 && !weight)) return SPH2POB_ERR_NULL;
    const int64_t total = n * num_classes;
    hipLaunchKernelGGL(focal_fwd_kernel, dim3(capped_blocks(total)), dim3(kBlock), 0, (hipStream_t)stream, logits, labels, weight, weight_mode,
                       make_params(gamma, alpha), scale, loss, total, (int)num_classes);
    return launch_status();
}

int sph2pob_focal_loss_bwd_f32(const float* logits, const int64_t* labels, const float* weight, int weight_mode, const float* grad_out,
                               int grad_stride, float gamma, float alpha, float scale, const float* avg_factor, float* grad_logits,
                               int64_t n, int64_t num_classes, void* stream) {
    if (int rc = flat_check(n, num_classes, weight_mode, gamma, grad_stride)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !grad_out || !grad_logits || (weight_mode != 0 && !weight)) return SPH2POB_ERR_NULL;
    const int64_t total = n * num_classes;
    hipLaunchKernelGGL(focal_bwd_kernel, dim3(capped_blocks(total)), dim3(kBlock), 0, (hipStream_t)stream, logits, labels, weight, weight_mode,
                       grad_out, grad_stride, make_params(gamma, alpha), scale, avg_factor, grad_logits, total, (int)num_classes);
    return launch_status();
}

int sph2pob_focal_loss_grad_scale_f32(const float* stash, const float* grad_out, float* out, int64_t total, void* stream) {
    if (total < 0 || total > ((int64_t)1 << 38)) return SPH2POB_ERR_SIZE;
    if (total == 0) return SPH2POB_OK;
    if (!stash || !grad_out || !out) return SPH2POB_ERR_NULL;
    hipLaunchKernelGGL(focal_grad_scale_kernel, dim3(capped_blocks(total)), dim3(kBlock), 0, (hipStream_t)stream, stash, grad_out, out, total);
    return launch_status();
}

}  // extern "C"
