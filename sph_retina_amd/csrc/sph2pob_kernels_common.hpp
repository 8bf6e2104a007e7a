// Shared by the translation units of libsph2pob_hip.so (sph2pob_{iou,assign,loss,nms}.hip): constants, launch knobs, box loads and
// wave helpers.  The (VARIANT, DIM) dispatch, the argument checks every entry point starts with and the choice of a pair's IoU
// function are sph2pob_iou_entry.hpp's, shared with the host twins.  Internal: include/sph2pob_hip.h is the ABI.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_head_loss.hpp"
#include "sph2pob_device.hpp"
#include "sph2pob_loss.hpp"
#include "sph2pob_fast.hpp"
#include "sph2pob_unbiased.hpp"
#include "sph2pob_iou_entry.hpp"

namespace {

using namespace sph2pob;

using sph2pob_head::kBlock;   // 4 waves of 64 lanes; launch_status() and cu_count() come from sph2pob_head_loss.hpp too

// tuning / A-B knobs (environment, read once at load): SPH2POB_NO_COMPACT=1 disables the compacting kernels,
// SPH2POB_ALIGNED_KERNEL=persistent selects the persistent form of the aligned kernel for the closed-form arithmetic
// (the default is the one-round chunk form), SPH2POB_NO_PREFETCH=1 its register prefetch, SPH2POB_SLICES_PER_WAVE=s /
// SPH2POB_WGS_PER_CU=k override its grid rule (s slices per wave, or exactly k workgroups per CU), SPH2POB_PW_ROWS the
// pairwise kernel's rows per workgroup
static bool g_no_compact = getenv("SPH2POB_NO_COMPACT") != nullptr;
static bool g_prefetch = getenv("SPH2POB_NO_PREFETCH") == nullptr;
static int g_pw_rows = getenv("SPH2POB_PW_ROWS") ? atoi(getenv("SPH2POB_PW_ROWS")) : 0;
static int g_slices_per_wave = getenv("SPH2POB_SLICES_PER_WAVE") ? atoi(getenv("SPH2POB_SLICES_PER_WAVE")) : 0;
static int g_wgs_per_cu = getenv("SPH2POB_WGS_PER_CU") ? atoi(getenv("SPH2POB_WGS_PER_CU")) : 0;
static bool g_no_prio = getenv("SPH2POB_NO_PRIO") != nullptr;   // A/B: no wave priority in the chunk kernel
// A/B: SPH2POB_CHUNK_STORES=dword|lines|wt forces how the BFoV chunk kernel writes its results (a dword per lane; whole
// 128-byte lines, plain; whole lines, write-through); anything else leaves the choice to the launcher
enum { CHUNK_STORES_AUTO = 0, CHUNK_STORES_DWORD, CHUNK_STORES_LINES, CHUNK_STORES_WT };
static int g_chunk_stores = [] {
    const char* s = getenv("SPH2POB_CHUNK_STORES");
    return !s ? CHUNK_STORES_AUTO : s[0] == 'd' ? CHUNK_STORES_DWORD : s[0] == 'l' ? CHUNK_STORES_LINES : s[0] == 'w' ? CHUNK_STORES_WT : CHUNK_STORES_AUTO;
}();
static bool g_persistent = getenv("SPH2POB_ALIGNED_KERNEL") != nullptr && getenv("SPH2POB_ALIGNED_KERNEL")[0] == 'p';   // A/B: the persistent form

template <int DIM>
__device__ __forceinline__ void load_box(const float* __restrict__ p, int64_t i, float (&b)[5]) {
    if (DIM == 4) {  // one 16-byte load per lane: 1 KiB per wave instruction, fully coalesced
        // (non-temporal loads: 8.32 vs 8.04 us at 1 M pairs, 51.1 vs 50.4 at 8 M, 97.8 vs 104.1 at 16 M: not kept)
        float4 v = reinterpret_cast<const float4*>(p)[i];
        b[0] = v.x; b[1] = v.y; b[2] = v.z; b[3] = v.w; b[4] = 0.0f;
    } else {
        const float* q = p + i * 5;
#pragma unroll
        for (int k = 0; k < 5; k++) b[k] = q[k];
    }
}

constexpr int kQCap = 128;                    // per-wave survivor stack capacity (<= 63 carried + 64 pushed)

// number of set bits of a wave mask below this lane: v_mbcnt_lo + v_mbcnt_hi (the 64-bit shift / and / popcount form
// costs eight instructions)
__device__ __forceinline__ int rank_below(unsigned long long m) {
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
}
__device__ __forceinline__ void wave_lds_fence() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

}  // namespace
