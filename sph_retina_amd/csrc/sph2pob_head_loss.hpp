// What the three fused head losses (sph2pob_focal, sph2pob_bbox_loss, sph2pob_delta_loss) share: the bound of the level tables,
// the scale rule, and the reduction tail of their kernels — one double block sum, one level lookup, one final pass.  The first part
// is plain host + device code, used by the kernels and by their CPU twins (sph2pob_host.hip); the second needs the HIP compiler.
#pragma once
#include <hip/hip_runtime.h>
#include <float.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"

#define SPHF_DEV __host__ __device__ __forceinline__

namespace sph2pob_head {

constexpr int kMaxLevels = 8;
constexpr int kBlock = 256;   // 4 waves of 64 lanes

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// `bytes` (a power of two): what a thread's four consecutive elements need — 16 for fp32 levels, 8 for the 16-bit levels of the
// _h16 entries
inline bool aligned_to(const void* p, int bytes) { return (reinterpret_cast<uintptr_t>(p) & (uintptr_t)(bytes - 1)) == 0; }
inline bool h16_dtype_ok(int dtype) { return dtype == SPH2POB_DTYPE_F16 || dtype == SPH2POB_DTYPE_BF16; }

// the scale every kernel applies: `scale` (loss_weight, possibly over a host divisor), over (*avg_factor + FLT_EPSILON) when the
// divisor lives on the device (weight_reduce_loss, mmdet/models/losses/utils.py:55-57) — one IEEE division in fp32
SPHF_DEV float effective_scale(float scale, const float* avg_factor) {
    return avg_factor ? scale / (avg_factor[0] + FLT_EPSILON) : scale;
}

}  // namespace sph2pob_head

#if defined(__HIPCC__)
#include <type_traits>
// Internal linkage: the library is linked from separately compiled units and each instantiates its own copy of the final kernel.
namespace {

inline int launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? SPH2POB_OK : (int)e;
}

// CU count of the current device (a partitioned MI355X exposes fewer; 256 in SPX mode: 8 XCDs x 32 CUs); queried once, no
// synchronisation involved
static int cu_count() {
    static int n = 0;
    if (n == 0) {
        int dev = 0, v = 0;
        n = (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && v > 0) ? v : 256;
    }
    return n;
}

// ---- the level element type T of a kernel: float, or the 16-bit types of the _h16 entries.  T reaches the load and store sites
// only: a value is widened to fp32 on load (exact) and narrowed once on store, by the compiler's own conversion (round to nearest
// even; on gfx950 the packed v_cvt_pk_f16_f32 and v_cvt_pk_bf16_f32).  A level table keeps its pointers as float*: level_ptr<T>
// reads them as what the entry's dtype says they are.
using f16_t = _Float16;
using bf16_t = __bf16;
template <class T> struct alignas(4 * sizeof(T)) Quad { T v[4]; };   // four consecutive elements: one 16- or 8-byte access

template <class T> __device__ __forceinline__ const T* level_ptr(const float* p) { return reinterpret_cast<const T*>(p); }
template <class T> __device__ __forceinline__ T* level_ptr(float* p) { return reinterpret_cast<T*>(p); }

// The one narrowing of a ROUNDED fp32 value.  The empty asm pins the fp32 value in a register first: without it the compiler
// folds a preceding fp32 multiply into the conversion (v_fma_mixlo_f16 d, g, s, 0 — seen in the scalar kinds of the fp16 focal
// kernel), which rounds the exact product once instead of RNE_T(fl32(g s)) and turns g * -0 into +0.
template <class T> __device__ __forceinline__ T narrow(float v) {
    if constexpr (!std::is_same<T, float>::value) asm("" : "+v"(v));
    return (T)v;
}
template <class T> __device__ __forceinline__ float load1(const T* p) { return (float)p[0]; }
template <class T> __device__ __forceinline__ void store1(T* p, float v) { p[0] = narrow<T>(v); }
template <class T> __device__ __forceinline__ void load4(const T* p, float (&x)[4]) {
    const Quad<T> q = *reinterpret_cast<const Quad<T>*>(p);
#pragma unroll
    for (int k = 0; k < 4; k++) x[k] = (float)q.v[k];
}
template <class T> __device__ __forceinline__ void store4(T* p, float x0, float x1, float x2, float x3) {
    Quad<T> q;
    q.v[0] = narrow<T>(x0); q.v[1] = narrow<T>(x1); q.v[2] = narrow<T>(x2); q.v[3] = narrow<T>(x3);
    *reinterpret_cast<Quad<T>*>(p) = q;
}

// The upstream gradient of an _h16 loss kernel (include/sph2pob_hip.h): 1 without grad_out, else grad_out[0]; `done` when the
// workgroup has nothing to do — skip_if_one and the value is exactly 1: `grads` already hold the gradient (the device-side test of
// focal_grad_scale_kernel: no host read)
__device__ __forceinline__ float upstream_gradient(const float* __restrict__ grad_out, int skip_if_one, bool& done) {
    const float g = grad_out ? grad_out[0] : 1.0f;
    done = grad_out && skip_if_one && g == 1.0f;
    return g;
}

// f(T{}) for the level element type of a checked SPH2POB_DTYPE_* code
template <class F>
void by_h16_dtype(int dtype, F&& f) {
    if (dtype == SPH2POB_DTYPE_F16) f(f16_t{});
    else f(bf16_t{});
}

// the sum of a workgroup's values in thread 0 (0 elsewhere): shuffle tree per wave, then the four waves in order
__device__ __forceinline__ double block_sum_f64(double v) {
    __shared__ double sm[sph2pob_head::kBlock / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < sph2pob_head::kBlock / 64; k++) r += sm[k];
    }
    return r;
}

// the level of a workgroup (workgroup-uniform; at most kMaxLevels entries; a level without items is skipped by the next one's
// equal offset)
template <class Levels>
__device__ __forceinline__ int level_of_block(const Levels& L, int block) {
    int l = 0;
#pragma unroll
    for (int q = 1; q < sph2pob_head::kMaxLevels; q++) l += (q < L.num && block >= L.lv[q].block_off) ? 1 : 0;
    return l;
}

// out[0] = scale_eff * (partials added in a fixed order): thread t adds partials t, t + 256, ... in turn, then the tree.  No float
// atomics, no global counter: the same bits on every call
__global__ __launch_bounds__(sph2pob_head::kBlock) void head_final_kernel(const double* __restrict__ partial, int nb, float scale,
                                                                          const float* __restrict__ avg_factor, float* __restrict__ out) {
    double acc = 0.0;
    for (int i = threadIdx.x; i < nb; i += sph2pob_head::kBlock) acc += partial[i];
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) out[0] = (float)(r * (double)sph2pob_head::effective_scale(scale, avg_factor));
}

inline int launch_final(const double* partial, int nb, float scale, const float* avg_factor, float* out, hipStream_t s) {
    hipLaunchKernelGGL(head_final_kernel, dim3(1), dim3(sph2pob_head::kBlock), 0, s, partial, nb, scale, avg_factor, out);
    return launch_status();
}

}  // namespace
#endif
