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

// the scale every kernel applies: `scale` (loss_weight, possibly over a host divisor), over (*avg_factor + FLT_EPSILON) when the
// divisor lives on the device (weight_reduce_loss, mmdet/models/losses/utils.py:55-57) — one IEEE division in fp32
SPHF_DEV float effective_scale(float scale, const float* avg_factor) {
    return avg_factor ? scale / (avg_factor[0] + FLT_EPSILON) : scale;
}

}  // namespace sph2pob_head

#if defined(__HIPCC__)
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
