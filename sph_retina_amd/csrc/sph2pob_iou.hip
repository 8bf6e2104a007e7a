// libsph2pob_hip.so — aligned IoU (the dominant kernels), the Sph2Pob transform and its adjoint, planar IoU: kernels + C-ABI
// launchers (include/sph2pob_hip.h).  gfx950 only.

#include <type_traits>

#include "sph2pob_kernels_common.hpp"

namespace {


template <int VARIANT, int DIM, bool FAST>
__global__ __launch_bounds__(kBlock) void iou_aligned_kernel(const float* __restrict__ b1,
                                                            const float* __restrict__ b2,
                                                            float* __restrict__ out, int64_t n, int mode, int edge,
                                                            int angle) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float x[5], y[5];
    load_box<DIM>(b1, i, x);
    load_box<DIM>(b2, i, y);
    out[i] = pair_iou_sel<VARIANT, DIM, FAST>(x, y, mode, edge, angle);
}

// ---- dominant kernel: aligned IoU, closed-form core, with wave-level compaction of the cull survivors ----
// ~60 % of the benchmark distribution's pairs are culled exactly by the bounding-circle test of stage 0 (hardware
// sin/cos, conservative margins); only survivors pay for accurate trig and the clip.  A naive `if (!culled) finish`
// leaves every wave running the finishing stage with ~40 % of its lanes.  Here each wave walks 64-pair slices, pushes
// the survivors' raw boxes on its own LDS stack (ballot + prefix rank => conflict-free consecutive slots, no atomics,
// no barriers: LDS operations of one wave are in order), and runs lean_finish only when 64 records are available, i.e.
// on fully populated waves.  Leftovers of the 4 waves of a workgroup are merged once at the end.
// Slices are grid-strided (slice = wave + k * waves).  A balanced workgroup-contiguous distribution (every workgroup
// floor / ceil of S / G slices instead of 12 next to 8) was measured 10.5 us against 8.9 us at 1 M pairs: at any moment
// the loads of all waves then span the whole 32 MB of input instead of one contiguous ~12 MB window, and the first data
// arrives after 3.0 us instead of 1.85 us (per-wave time stamps, tools/stamp_timeline.py; equal from 2 M pairs up).
// Stores: culled pairs write 0 from stage 0, survivors write from the finishing stage by index.
// Variants built and measured on MI355X this round (1 M pairs; profiles/r02b_ablation_*.log):
//   * a separating-axis reject after stage 1 + a second record stack so that the clip too runs on full waves (only
//     26 % of the pairs overlap, 40 % pass the cull): 8.80 us against 8.55 us without the second stack — the 35 % idle
//     clip lanes cost less than the extra LDS round trip and the longer per-wave dependency chain;
//   * rare lanes (jitter decisions, floors, near-parallel: 0.7 % of the survivors) re-run by a general form in place
//     12.1 us, deferred to an index stack and finished once per workgroup 11.0 us — hence lean_front's guarded blocks;
//   * no carried state at all: one wave per 128-pair chunk, cull both slices, compact, finish (one pass at 81 % lane
//     use, no workgroup merge, no barrier): 8.84 us against 8.96 us here at 1 M pairs, 56.9 against 55.1 us at 8 M;
//     one lane per pair without compaction 10.3 us / 66.0 us (profiles/r02f_ab_*.log);
//   * one survivor ring per WORKGROUP (LDS slot reservation with ds_add_rtn, per-chunk fill counters, chunks claimed by
//     compare-and-swap, slots recycled in order) so that a pass can start as soon as the workgroup holds 64 survivors and
//     all passes but one are full: bit-identical results, 14.2 us / 75.2 us — three dependent LDS round trips and
//     lane-0 sections per slice cost far more than the earlier start gains (profiles/r02i_ab_ring.log).
#if defined(SPH_STAMPS)
// DIAGNOSTIC BUILD ONLY (tools/stamp_timeline.py; never in the shipped library): per-wave time stamps of the dominant
// kernel, s_memrealtime (100 MHz, chip-wide), written to a buffer of their own that nothing else reads.
__device__ unsigned long long* g_stamps = nullptr;
__device__ __forceinline__ void stamp(int wave_global, int k) {
    if ((threadIdx.x & 63) == 0 && g_stamps) g_stamps[(size_t)wave_global * 8 + k] = __builtin_amdgcn_s_memrealtime();
}
// slot 6: where the wave ran (HW_ID | XCC_ID << 32); slot 7: any per-wave figure the caller wants on the timeline
__device__ __forceinline__ void stamp_where(int wave_global) {
    const unsigned hw = __builtin_amdgcn_s_getreg(4 | (31 << 11)), xcc = __builtin_amdgcn_s_getreg(20 | (31 << 11));
    if ((threadIdx.x & 63) == 0 && g_stamps) g_stamps[(size_t)wave_global * 8 + 6] = hw | ((unsigned long long)xcc << 32);
}
__device__ __forceinline__ void stamp_value(int wave_global, unsigned long long v) {
    if ((threadIdx.x & 63) == 0 && g_stamps) g_stamps[(size_t)wave_global * 8 + 7] = v;
}
#define SPH_STAMP(k) stamp(wave_global, k)
#define SPH_STAMP_WHERE() stamp_where(wave_global)
#define SPH_STAMP_VALUE(v) stamp_value(wave_global, v)
#else
#define SPH_STAMP(k)
#define SPH_STAMP_WHERE()
#define SPH_STAMP_VALUE(v)
#endif
template <int DIM>
struct WaveQueue {
    float f[2 * DIM][kQCap];   // raw (theta, phi, alpha, beta[, gamma]) of both boxes
    int idx[kQCap];            // pair index
};
constexpr int queue_lds_bytes(int dim) { return (kBlock / 64) * (2 * dim + 1) * kQCap * 4 + 64; }

template <int DIM>
__device__ __forceinline__ void queue_store(WaveQueue<DIM>& q, int slot, const float (&j1)[5], const float (&j2)[5], int i) {
#pragma unroll
    for (int k = 0; k < DIM; k++) { q.f[k][slot] = j1[k]; q.f[DIM + k][slot] = j2[k]; }
    q.idx[slot] = i;
}
template <int DIM>
__device__ __forceinline__ int queue_load(const WaveQueue<DIM>& q, int slot, float (&j1)[5], float (&j2)[5]) {
#pragma unroll
    for (int k = 0; k < 5; k++) { j1[k] = k < DIM ? q.f[k][slot] : 0.0f; j2[k] = k < DIM ? q.f[DIM + k][slot] : 0.0f; }
    return q.idx[slot];
}

// The reference-order finish is 15-35 KB of code per copy (ocml's sinf / cosf / acosf / asinf expansions): called, not
// inlined, so that the kernel's two call sites (loop and tail) share one copy and the kernel stays inside the 64 KB
// instruction cache.
template <int VARIANT, int DIM>
__device__ __attribute__((noinline)) float ref_finish(float a0, float a1, float a2, float a3, float a4, float b0, float b1, float b2,
                                                      float b3, float b4, int mode, int edge, int angle) {
    const float u1[5] = {a0, a1, a2, a3, a4}, u2[5] = {b0, b1, b2, b3, b4};
    return pair_iou<VARIANT, DIM>(u1, u2, mode, edge, angle);
}

// ARC: rbb_edge == 'arc' folded at compile time (the chord / tangent forms pull ocml's sinf / tanf argument reduction
// into the cull and the finishing stage: 8 copies of ~100 instructions the common launch never executes)
// REF: finish with the reference-order arithmetic (pair_iou) instead of the closed-form core: the cull is exact for it as
// well (disjoint planar rectangles give exactly 0 in the reference), so `set_arithmetic('reference')`, rbb_angle='project'
// (same planar sizes and positions, other angles: the circles do not change) and sph2pob_legacy (VARIANT 2: chord form of
// the cull) pay their ~3x VALU only for the survivors, on full waves.
template <int VARIANT, int DIM, bool PREFETCH, bool ARC, bool REF = false>
__global__ __launch_bounds__(kBlock, REF ? 4 : (DIM == 4 ? 7 : 5)) void iou_aligned_compact_kernel(const float* __restrict__ b1,
                                                                                      const float* __restrict__ b2,
                                                                                      float* __restrict__ out, int n,
                                                                                      int mode, int edge_arg) {
    __shared__ WaveQueue<DIM> queues[kBlock / 64];
    __shared__ int leftover[kBlock / 64];
    const int edge = ARC ? (int)EDGE_ARC : (edge_arg & 0xff);
    const int angle = REF ? (edge_arg >> 8) & 1 : (int)ANGLE_EQUATOR;   // reference-order finish only: rbb_angle
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    WaveQueue<DIM>& q = queues[wave];
    const int nslices = (n + 63) >> 6;
    const int wave_global = blockIdx.x * (kBlock / 64) + wave, nwaves = gridDim.x * (kBlock / 64);
    int count = 0;  // wave-uniform stack height
    auto finish = [&](const float (&u1)[5], const float (&u2)[5]) -> float {
        if constexpr (REF) return ref_finish<VARIANT, DIM>(u1[0], u1[1], u1[2], u1[3], u1[4], u2[0], u2[1], u2[2], u2[3], u2[4], mode, edge, angle);
        else return lean_finish<VARIANT, DIM>(u1, u2, mode, edge);
    };
    SPH_STAMP(0);
    SPH_STAMP_WHERE();
    // one slice: cull, push the survivors, finish 64 of them when a full wave of records is available
    auto slice = [&](const float (&x)[5], const float (&y)[5], int sl) {
        const int i = sl * 64 + lane;
        bool surv = false;
        if (i < n) {
            if (fast_cull<DIM, VARIANT == VARIANT_LEGACY>(x, y, edge)) out[i] = 0.0f;
            else surv = true;
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(surv);
        if (surv) queue_store<DIM>(q, count + rank_below(m), x, y, i);
        count += __popcll(m);
        if (sl == wave_global) SPH_STAMP(1);   // first slice culled: its data has arrived
        if (count >= 64) {  // wave-uniform
            count -= 64;
            wave_lds_fence();
            float u1[5], u2[5];
            const int j = queue_load<DIM>(q, count + lane, u1, u2);
            out[j] = finish(u1, u2);
            SPH_STAMP(4);   // (last) in-loop pass done
        }
    };
    auto fetch = [&](int sl, float (&x)[5], float (&y)[5]) {
        const int i = sl * 64 + lane;
        if (sl < nslices && i < n) { load_box<DIM>(b1, i, x); load_box<DIM>(b2, i, y); }
    };
    if (PREFETCH) {
        // software prefetch: the next slice's boxes are in flight while this slice is computed (register double buffer;
        // two register sets used alternately instead of the copy were measured slower: the loop body doubles)
        float nx[5] = {0, 0, 0, 0, 0}, ny[5] = {0, 0, 0, 0, 0};
        fetch(wave_global, nx, ny);
        for (int sl = wave_global; sl < nslices; sl += nwaves) {
            float x[5], y[5];
#pragma unroll
            for (int k = 0; k < 5; k++) { x[k] = nx[k]; y[k] = ny[k]; }
            fetch(sl + nwaves, nx, ny);
            slice(x, y, sl);
        }
    } else {
        for (int sl = wave_global; sl < nslices; sl += nwaves) {
            float x[5] = {0, 0, 0, 0, 0}, y[5] = {0, 0, 0, 0, 0};
            fetch(sl, x, y);
            slice(x, y, sl);
        }
    }
    // merge the < 64 leftovers of the four waves and finish them on as few, as full waves as possible
    SPH_STAMP(2);   // loop done
    SPH_STAMP_VALUE((unsigned long long)count);
    if (lane == 0) leftover[wave] = count;
    __syncthreads();
    SPH_STAMP(3);   // workgroup barrier passed
    const int c0 = leftover[0], c1 = leftover[1], c2 = leftover[2], c3 = leftover[3];
    const int total = c0 + c1 + c2 + c3;   // <= 252: at most one chunk per wave
    if (wave * 64 < total) {
        int k = wave * 64 + lane;
        if (k < total) {
            int w = 0;
            if (k >= c0) { k -= c0; w = 1; if (k >= c1) { k -= c1; w = 2; if (k >= c2) { k -= c2; w = 3; } } }
            float u1[5], u2[5];
            const int j = queue_load<DIM>(queues[w], k, u1, u2);
            out[j] = finish(u1, u2);
        }
    }
    SPH_STAMP(5);   // wave done
}

// ---- dominant kernel since round 2 (closed-form arithmetic): the one-round chunk form of the same pipeline ----
// One wave = one chunk of SLICES x 64 consecutive pairs and no carried state: the wave requests its whole chunk up front
// (the whole input is in flight after the first half microsecond), culls it, compacts the survivors on its own LDS stack
// (~51 of 128 for the benchmark distribution) and finishes them in ONE pass (a second one when more than 64 survive).
// No barrier, no merge, 64 VGPRs, so that the 1 954 workgroups of a 1 M-pair launch are all resident at once (8 per CU)
// and no wave ever runs two finishing passes back to back.  What was measured on MI355X (profiles/r02l_*):
//   * the SIMDs are saturated from the arrival of the first data to the end: a finishing pass costs a SIMD ~1 500 cycles
//     = 0.63 us with 8 resident waves (tools/ubench/finish_rate.hip: ~4 cycles per instruction whatever its kind, not
//     the 2 / 4 / 8 of independent instruction streams), a cull ~190, and the launch takes
//     ~3.0 us (kernel boundary + first data) + the VALU time; removing the finishing arithmetic leaves 4.5 us, removing
//     the cull arithmetic saves 0.9 us (r02l_ab_ablation_*.log);
//   * against the persistent form: 8.8 vs 9.0 us at 1 M pairs, 6.0 vs 6.3 at 500 k, 17.1 vs 18.9 at 2 M, 27.9 vs 30.4
//     at 4 M, 52.5 vs 54.3 at 8 M, RBFoV 11.8 vs 12.7 at 1 M; bit-identical results (r02l_ab_chunk_*.log) — the
//     persistent form's leftover merge also ends in partial passes (7 200 passes against 7 813 here, 6 250 if every
//     pass were full) and puts two passes and a barrier on every wave's critical path;
//   * pooling the survivors of 4 / 8 / 16 waves in one workgroup-wide stack (one ds_add_rtn per wave, one LDS-only
//     barrier, chunks assigned or claimed from a counter) so that all passes but one per workgroup are full: 12 % fewer
//     finishing instructions at 8 waves and NO gain (8.8-8.95 us at 1 M, 55-57 at 8 M; r02l_ab_pool_*.log) — the
//     barrier couples waves that sit on different SIMDs; built, measured, removed (and again with the cull phase at a
//     raised wave priority: 7.19 vs 7.29 us at 1 M, 15.5 vs 14.9 at 2 M, 49.5 vs 47.2 at 8 M: r03j_ab_pool_prio_*.log);
//   * workgroups of 1 / 2 / 4 / 8 / 16 independent waves: the same within 1 % from 100 k to 8 M pairs (16: +3 %;
//     r02z_ab_wg*.log); 4 stays;
//   * rotating which wave of the persistent form takes which leftover chunk: the hardware already rotates the
//     wave -> SIMD placement from workgroup to workgroup (tools/ubench/hwid.hip); +0.3 us, removed;
//   * finishing-pass trim, bit-identical (profiles/r08a_finish_trim.log): NaN test folded into the
//     `similar` test, no clamp of the clip's reciprocals, survivor mask and two-condition guards from ballots of single
//     compares: SQ_INSTS_VALU 3.62 -> 3.49 M per launch, 7.21 -> 7.05 us per 1 M pairs.  Measured on the ISA and not kept: a
//     "clean" bit from the cull (its range tests cost the cull more than the clamps they would skip), passes peeled out
//     of the loop (no hoisted rare-block constants, but every common one re-materialised per use: -5 v_mov, twice the code).
//   * wave prologue and slice glue of the BFoV launches (ISA of the <0, 4, true, 2> body; bit-identical results;
//     profiles/r09a_prologue_glue.log): 7.16 -> 6.92 us per 1 M pairs.  (i) 32-bit byte offsets from the
//     kernel-argument pointers (OFF32): per slice v_min_i32 + v_ashrrev_i32 + v_lshlrev_b64 + 2 v_lshl_add_u64 in front of
//     the first load become one v_lshlrev_b32 (+ v_or for the second slice; the clamp of the tail lanes only in the one
//     wave that holds the tail: clamping in every wave 7.08 us), each store loses its v_ashrrev_i32 + v_lshl_add_u64, the
//     stack holds the result's byte offset instead of the pair index; (ii) the wave number through v_readfirstlane: chunk
//     base, the `base >= n` test and the LDS base (formed once, was twice) are scalar; one zero register for both stores
//     of the culled pairs; the priority is a template parameter chosen by the launcher (was s_and + s_bitcmp + s_cselect
//     + branch, twice).  (i) WITHOUT the scalar wave number and the shared zero register is slower than the parent (7.23
//     us; 7.28 with hoisted constants as well), so (i) and (ii) go together; (ii) alone was not built.  (iii) the constants
//     that only guarded blocks use are formed inside those blocks (sph2pob_fast.hpp: SPH_RARE_CONST): 15 -> 8 v_mov_b32 in
//     front of the pass loop (the four upper clamp bounds and 3.0e38 are operands of the common path's v_med3, which takes
//     one SGPR and no literal: they stay).  It changes nothing at 1 M (6.92 vs 6.91 us without it) or 250 k (3.86 vs 3.87);
//     at 8 M the build without it read 47.9 us against the parent's 47.2 and 47.4 with it, so it is kept.
//     Measured and not kept: RBFoV on the 32-bit route: 10.09 -> 9.69 us at 1 M but 62.8 -> 63.4 at 8 M, where the 64-bit
//     instantiation of the same build read 60.0; RBFoV keeps 64-bit offsets.
//     The BFoV chunk kernel now has three instantiations per (variant, edge) instead of one (64-bit; 32-bit with and
//     without the priority): +0.2 MB of library (7.4 -> 7.6 MB).
//   * whole-line stores (LINES; profiles/r11a_store_floor.log, r11b_ab_lines_*.log; bit-identical results).
//     The dword stores (two masked zero stores in the cull, one scattered store in the pass) touched every 128-byte line
//     twice and left 4 MB dirty in the L2s for the kernel boundary.  A load-store-only kernel of this shape: dword per lane
//     4.04 us per launch, dwordx4 from lanes 0-31 3.21, the same write-through (sc1) 2.89, dword sc1 3.83, empty 2.71.  Here:
//     the chunk's results staged in 512 B of the wave's LDS and stored once after the pass loop.  Against the parent, 7
//     interleaved rounds (us per launch, parent / dword body of this build / plain lines / write-through lines):
//     250 k 4.33 / 4.37 / 4.46 / 4.45 (rounds 4.1-5.9: level), 1 M 6.75 / 6.81 / 6.90 / 6.31, 2 M 15.35 / 15.12 / 13.75 / 13.58,
//     8 M 47.04 / 46.59 / 45.03 / 44.79; efficient 1 M 6.85 / 6.86 / 6.89 / 6.37, 8 M 46.75 / 46.92 / 45.14 / 44.30.  bench.py,
//     three interleaved runs: 6.857 -> 6.233 us per step (spreads 0.042 / 0.171).  Write-through lines are the fastest arm
//     at every size where the arms differ, so they are the default everywhere; plain lines gain from 2 M pairs up and
//     nothing at 1 M (the staging's LDS traffic pays for the saved stores; the gain at 1 M is the write-through's: nothing
//     is left to write back while no SIMD can work).  A dword per lane written through was not built for this kernel (the
//     floor says 3.83 us against 2.89).  Four more instantiations per (variant, edge): 7.6 -> 8.2 MB of library.
//     250 k again with 15 rounds (parent / shipped / dword body): 4.249 / 4.260 / 4.227, efficient 3.866 / 3.828 / 3.805: level.
//     The shipped build (no knob) against the parent (profiles/r11c_*, r11d_*): iou.npy of bench.py --dump-outputs byte-identical
//     (default, 8 M pairs, efficient); bench.py 6.777 -> 6.260 us per step (three interleaved runs each, spreads 0.155 / 0.046);
//     --full, one run each: kernel_ms 6.84 -> 6.50, cold 10.56 -> 9.18, at_8m 48.64 -> 46.75 us; rocprofv3: traced average
//     7.85 -> 6.88 us, WRITE_SIZE 4.287 -> 4.000 MB per launch (the algorithmic bytes), SQ_INSTS_VALU 420.1 -> 441.1 per wave
//     (+21: the staging costs more issue than the stores it replaces), SQ_INSTS_SALU 579 k -> 634 k.
//   * instruction diet of the LINES bodies (ISA of the benched <0, 4, true, 2, true, true, true, true> body; bit-identical results;
//     profiles/r12_diet_*.log): SQ_INSTS_VALU 441.1 -> 415.3 per wave, SQ_INSTS_SALU 81.1 -> 79.6, 49 -> 48 VGPRs.
//     (i) one survivor mask per slice: the push branches on the scalar mask of the rank and the count (inverse ballot) instead of
//     on `!culled` rebuilt from the other sense of each compare: 3 compares per slice.  (ii) arc edges: the range test of the
//     cull covers theta and phi only (fast_cull_parts: why no extent can be culled wrongly): 2 v_max3_u32 per slice.  (iii) the
//     index column holds the result slot's offset from the start of `queues`, which is also the zero stores' address register;
//     the column's address is one v_lshl_add_u32 from a scalar base (count folded in); the slice's 256 s comes off the scalar
//     side of the `inside` compare; the pass forms its two addresses from the slot, not from registers set up in front of the
//     loop, and reads the index with the record: 6 -> 4 and 8 -> 5 VALU in the two pushes, 11 -> 8 in front of the pass loop,
//     one v_add fewer behind each pass.  (iv) lean_front / lean_finish: the centres without dy on the common path, the three
//     |x| as source modifiers: 8 per pass.  Not kept: `surv` from the failing senses of the same compares (the compiler merges
//     the two range tests into 2 v_cndmask + v_or + v_cmp: +2 per slice); the four centre products left to sink (six register
//     copies on the common path).  Times move less than the counts say, and not by the count alone: at 1 M pairs, 9 interleaved
//     rounds, parent / this build / without the |x| pins / centres as before / neither: 6.263 / 6.038 / 6.134 / 6.162 / 6.323 us;
//     the dword body, 5 VALU shorter (cull and finish only), read 6.753 -> 6.805 us with the |x| pins and 6.691 without: the
//     BFoV dword-store bodies ask lean_finish for none (ABS_PINS; 6.896 -> 6.781 us, r12_diet_ab_pins.log).  2 M 13.68 -> 13.42, 8 M 44.75 -> 43.10, nearby 1 M 12.63 -> 12.35,
//     RBFoV 1 M 10.14 -> 10.00 us.
template <int DIM, int SLICES>
struct ChunkQueue {
    float f[2 * DIM][64 * SLICES];
    int idx[64 * SLICES];   // pair index (OFF32: the byte offset of the pair's result, 4 * index)
};
// LINES: the chunk's results are staged in the wave's own LDS (`res`) and written after the pass loop as whole 128-byte
// lines.  The stack's index column holds the byte offset of the survivor's slot in `res` (< 256 SLICES) in 16 bits, so that
// the workgroup takes 19 456 B and eight stay resident per CU (a 32-bit column: 20 480 B, exactly 160 KiB for eight).
template <int DIM, int SLICES>
struct alignas(16) ChunkLineQueue {
    float f[2 * DIM][64 * SLICES];
    float res[64 * SLICES];
    unsigned short idx[64 * SLICES];
};
constexpr int kChunkSlices = 2;
// write-through whole lines at every size: fastest arm from 1 M to 8 M pairs, level with the others at 250 k (see the kernel's header)
constexpr int kChunkStoresDefault = CHUNK_STORES_WT;
static_assert(256 * kChunkSlices <= 65536, "a slot's byte offset in res fits the 16-bit index column");
// OFF32: every load and store of the chunk kernel is addressed by an unsigned 32-bit byte offset from its kernel-argument
// pointer (global_load / global_store v_off, s[base:base+1]: no 64-bit address arithmetic per lane), which needs the byte
// offset one past the last box, n * 4 * dim, to fit in 32 bits.  Above that the launcher takes the 64-bit instantiation.
constexpr bool chunk_offsets_fit_u32(int64_t n, int dim) { return n >= 0 && n * (4 * dim) < ((int64_t)1 << 32); }
static_assert(chunk_offsets_fit_u32(((int64_t)1 << 28) - 1, 4) && !chunk_offsets_fit_u32((int64_t)1 << 28, 4), "BFoV: n * 16 < 2^32");
static_assert(chunk_offsets_fit_u32(214748364, 5) && !chunk_offsets_fit_u32(214748365, 5), "RBFoV: n * 20 < 2^32");
static_assert(chunk_offsets_fit_u32(0, 4) && chunk_offsets_fit_u32(0, 5) && !chunk_offsets_fit_u32(-1, 4), "empty batch fits, a negative size never");
__device__ __forceinline__ const float* at_byte(const float* __restrict__ p, unsigned off) { return reinterpret_cast<const float*>(reinterpret_cast<const char*>(p) + off); }
__device__ __forceinline__ float* at_byte(float* __restrict__ p, unsigned off) { return reinterpret_cast<float*>(reinterpret_cast<char*>(p) + off); }
// PRIO: the load + cull phase at wave priority 1 (the launcher's choice: see below)
// LINES (BFoV 32-bit bodies; the launcher asks for it only when `out` is 16-byte aligned): no global store in the cull or
// the pass; see ChunkLineQueue and the end of the kernel.  WT: the line stores are write-through (sc1).
template <int VARIANT, int DIM, bool ARC, int SLICES, bool OFF32, bool PRIO, bool LINES = false, bool WT = false, int WAVES = kBlock / 64>
__global__ __launch_bounds__(64 * WAVES, DIM == 4 ? 8 : 7) void iou_aligned_chunk_kernel(const float* __restrict__ b1, const float* __restrict__ b2,
                                                                      float* __restrict__ out, int n, int mode, int edge_arg) {
    static_assert(!LINES || (DIM == 4 && OFF32), "whole-line stores are built for the BFoV 32-bit bodies only");
    static_assert(LINES || !WT, "write-through is a flavour of the line stores");
    using Queue = std::conditional_t<LINES, ChunkLineQueue<DIM, SLICES>, ChunkQueue<DIM, SLICES>>;
    __shared__ Queue queues[WAVES];
    static_assert(!LINES || 8 * sizeof(queues) + 4096 <= 160 * 1024, "eight workgroups per CU, at least 4 KiB clear of the 160 KiB of LDS");
    static_assert(!LINES || sizeof(queues) <= 65536, "a result slot's byte offset in `queues` fits the 16-bit index column");
    const int edge = ARC ? (int)EDGE_ARC : (edge_arg & 0xff);
    const int lane = threadIdx.x & 63;
    // the wave's number in an SGPR: its chunk, the test below and its LDS base (formed once) are scalar
    const int wave = OFF32 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : threadIdx.x >> 6;
    Queue& q = queues[wave];
    const int base = (blockIdx.x * WAVES + wave) * (64 * SLICES);
    if (base >= n) return;   // wave-uniform; the kernel has no barrier
    const int wave_global = blockIdx.x * WAVES + wave;
    (void)wave_global;
    SPH_STAMP(0);
    SPH_STAMP_WHERE();
#if defined(SPH_STAMPS)
    const unsigned long long clk0 = __builtin_amdgcn_s_memtime();
#endif
    // Wave priority.  The SIMD's arbiter serves the oldest wave first, so a wave whose boxes arrive late waits for its
    // cheap cull behind the finishing passes of the waves that got theirs early, and its own pass starts that much later:
    // the tail of a launch whose waves are all resident at once.  The load + cull phase runs at priority 1, the finishing
    // pass at 0 (any level above the pass's does the same): 7.76 -> 7.28 us per 1 M pairs, 12.3 -> 11.8 at 1.5 M, 5.21 -> 5.02
    // at 500 k, 11.66 -> 11.17 for 1 M nearby pairs; from 3 M pairs up, where workgroups start as others retire, it costs
    // 1-2.5 % instead (2.6 M: +2.8 %), and RBFoV launches lose 2.5 % at 1 M: the launcher asks for it for BFoV launches of
    // up to two rounds (profiles/r03g_ab_prio*.log).  A priority that falls (or rises) with the wave's progress through
    // its pass, to keep the waves of a SIMD in step (or to retire them one by one): 7.70 / 7.55 against 7.31 / 7.18 us.
    if (PRIO) __builtin_amdgcn_s_setprio(1);
    // BFoV: lanes past the end of the batch load the last pair again (never stored, never stacked): no zero fill of the
    // sixteen registers, no branch around the loads (8.31 -> 8.24 us per 1 M pairs; RBFoV's twenty dword loads were faster
    // behind the branch: 10.5 vs 10.7 us)
    float x[SLICES][5], y[SLICES][5];
    // OFF32: byte offset of lane's first result; slice s is at + 256 s, its BFoV boxes at 4 x that
    const unsigned o4 = (unsigned)(base + lane) * 4u;
    static_assert(!OFF32 || DIM == 4, "the 32-bit route is BFoV's (RBFoV: measured, not kept; see above)");
    if (OFF32) {
        auto load4 = [&](unsigned off, int s) {
            const float4 u = *reinterpret_cast<const float4*>(at_byte(b1, off)), v = *reinterpret_cast<const float4*>(at_byte(b2, off));
            x[s][0] = u.x; x[s][1] = u.y; x[s][2] = u.z; x[s][3] = u.w; x[s][4] = 0.0f;
            y[s][0] = v.x; y[s][1] = v.y; y[s][2] = v.z; y[s][3] = v.w; y[s][4] = 0.0f;
        };
        if (base + 64 * SLICES <= n) {   // wave-uniform: a whole chunk needs no clamp (clamping always: 7.08 vs 6.92 us)
#pragma unroll
            for (int s = 0; s < SLICES; s++) load4(o4 * 4u + s * 1024u, s);
        } else {
            const unsigned last = (unsigned)(n - 1) * 16u;
#pragma unroll
            for (int s = 0; s < SLICES; s++) { const unsigned o = o4 * 4u + s * 1024u; load4(o < last ? o : last, s); }
        }
    } else {
#pragma unroll
        for (int s = 0; s < SLICES; s++) {
            const int i = base + s * 64 + lane;
            if (DIM == 4) {
                const int il = i < n ? i : n - 1;
                load_box<DIM>(b1, il, x[s]);
                load_box<DIM>(b2, il, y[s]);
            } else {
#pragma unroll
                for (int k = 0; k < 5; k++) { x[s][k] = 0.0f; y[s][k] = 0.0f; }
                if (i < n) { load_box<DIM>(b1, i, x[s]); load_box<DIM>(b2, i, y[s]); }
            }
        }
    }
    int count = 0;
    float zero = 0.0f;   // ONE register for the stores of the culled pairs (left alone, a v_mov in front of each)
    if (OFF32) asm volatile("" : "+v"(zero));
    // LINES: the byte offset of lane's slot of slice 0 in `res`, from the start of `queues`, in ONE register: the address of the
    // zero stores (slice s at + 256 s) and, as it stands, the value of the index column — the pass stores through it without
    // adding the wave's base (left alone: the wave's base | 4 lane for the stores and a second form of it for each push)
    unsigned roff = 0;
    if constexpr (LINES) {
        roff = (unsigned)(reinterpret_cast<char*>(&q.res[lane]) - reinterpret_cast<char*>(queues));
        asm volatile("" : "+v"(roff));
    }
    auto res_at = [&](unsigned off) -> float& { return *reinterpret_cast<float*>(reinterpret_cast<char*>(queues) + off); };
#pragma unroll
    for (int s = 0; s < SLICES; s++) {
        const int i = base + s * 64 + lane;
        // (masks combined as masks, not through a bool)
#if defined(SPH_ABL_NOCULL)
        const bool culled = ((lane * 2654435761u + s * 40503u + blockIdx.x) >> 7) % 5 >= 2;   // ABLATION: 40 % survive, no cull arithmetic
#else
        const CullParts cp = fast_cull_parts<DIM, VARIANT == VARIANT_LEGACY>(x[s], y[s], edge);
        const bool culled = cp.in_sizes & cp.in_theta & cp.apart;
        const unsigned long long cm = __builtin_amdgcn_ballot_w64(cp.in_sizes) & __builtin_amdgcn_ballot_w64(cp.in_theta) &
                                      __builtin_amdgcn_ballot_w64(cp.apart);
#endif
        // (OFF32: 4 n < 2^30, so the slice's 256 s comes off the scalar side of a signed compare: no v_or per slice)
        const bool inside = OFF32 ? (int)o4 < (int)((unsigned)n * 4u) - s * 256 : i < n;
#if defined(SPH_ABL_NOCULL)
        const bool surv = inside & !culled;
        const unsigned long long m = __builtin_amdgcn_ballot_w64(surv);
#else
        // (the mask from the ballots of single compares, taken before the branch of the store: the ballot of `surv`, or of a
        // compare whose mask crosses a branch, costs two more VALU instructions; see CullParts)
        const unsigned long long m = __builtin_amdgcn_ballot_w64(inside) & ~cm;
        // LINES: nothing but the push reads the cull, so its branch takes the scalar mask of the rank and the count as it is (one
        // s_and_saveexec).  Built from `!culled` next to that mask, every condition was compared twice, once per sense: 6 VALU
        // instructions per chunk; built from the failing senses of the same compares, the two range tests were merged into
        // 2 v_cndmask + v_or + v_cmp.  The dword bodies keep the lane's own `culled` for the zero store.
        const bool surv = LINES ? __builtin_amdgcn_inverse_ballot_w64(m) : inside & !culled;
#endif
        if constexpr (LINES) res_at(roff + s * 256u) = zero;   // every lane, no branch: a survivor's result lands on it later
        else if (inside & culled) {   // (non-temporal stores here and below: 8.42 vs 8.30 us at 1 M, 51.4 vs 48.1 at 8 M)
            if (OFF32) *at_byte(out, o4 + s * 256u) = zero;
            else out[i] = 0.0f;
        }
        if (surv) {
            const int rank = rank_below(m), slot = count + rank;
#pragma unroll
            for (int k = 0; k < DIM; k++) {   // (count, a scalar, goes to the base: no v_add per slice)
                if constexpr (LINES) { (&q.f[k][count])[rank] = x[s][k]; (&q.f[DIM + k][count])[rank] = y[s][k]; }
                else { q.f[k][slot] = x[s][k]; q.f[DIM + k][slot] = y[s][k]; }
            }
            if constexpr (LINES) {
                // (the 16-bit column's address from a copy of the rank the compiler cannot relate to the records' address: ONE
                // v_lshl_add_u32 from the column's base + 2 count, a scalar; left alone it is (4 slot + base) - 2 slot, a shift
                // and a subtraction more)
                int rank16 = rank;
                asm volatile("" : "+v"(rank16));
                (&q.idx[count])[rank16] = (unsigned short)(roff + s * 256u);
            } else q.idx[slot] = OFF32 ? (int)(o4 + s * 256u) : i;
        }
        count += __popcll(m);
        if (s == 0) SPH_STAMP(1);
    }
    SPH_STAMP(2);
    SPH_STAMP(3);
    SPH_STAMP_VALUE((unsigned long long)count);
    wave_lds_fence();
    if (PRIO) __builtin_amdgcn_s_setprio(0);
    for (int b = 0; b < count; b += 64) {
        int slot = b + lane;
        // (LINES: a value the loop optimiser cannot turn into two address registers that are set up in front of the loop and
        // advanced in it: more than 99 % of the waves run one pass, which pays 3 VALU instructions for that set-up)
        if constexpr (LINES) asm volatile("" : "+v"(slot));
        if (slot < count) {
            float u1[5], u2[5];
#pragma unroll
            for (int k = 0; k < 5; k++) { u1[k] = k < DIM ? q.f[k][slot] : 0.0f; u2[k] = k < DIM ? q.f[DIM + k][slot] : 0.0f; }
            // LINES: the survivor's slot in `res`, read HERE with the record (one wait for both) and held in a register through the
            // pass: read behind it, the slot and the records' address stay live instead, and the column's address is formed from
            // both (see the push)
            unsigned rslot = 0;
            if constexpr (LINES) {
                int slot16 = slot;
                asm volatile("" : "+v"(slot16));
                rslot = q.idx[slot16];
                asm volatile("" : "+v"(rslot));
            }
#if defined(SPH_ABL_NOFINISH)
            const float r = u1[0] + u2[1] + u1[2] + u2[3] > 1e30f ? 1.0f : 0.5f;   // ABLATION: no finishing arithmetic
#else
            // (the BFoV dword-store bodies without lean_front's |x| pins: see there)
            const float r = lean_finish<VARIANT, DIM, 0, LINES || DIM != 4>(u1, u2, mode, edge);
#endif
            if constexpr (LINES) res_at(rslot) = r;   // in order behind the zero
            else if (OFF32) *at_byte(out, (unsigned)q.idx[slot]) = r;
            else out[q.idx[slot]] = r;
        }
    }
    if constexpr (LINES) {
        // the chunk's 128 results, once: lanes 0-31 read 16 bytes of `res` each and store them with ONE instruction, so that
        // every 128-byte line of the output is written whole.  The one wave that holds the batch's tail stores a dword per
        // lane as before: a line store never reaches past n.
        wave_lds_fence();
        if (base + 64 * SLICES <= n) {   // wave-uniform
            static_assert(SLICES == 2, "32 lanes x 16 bytes = the 128 results of two slices");
            if (lane < 32) {
                const float4 v = *reinterpret_cast<const float4*>(&q.res[4 * lane]);
                const unsigned off = (unsigned)base * 4u + 16u * lane;
                if constexpr (WT) {
                    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
                    const u32x4 w = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                    // (n * 4 fits: the 32-bit route; the descriptor's range check is a second guard, not the bound)
                    __builtin_amdgcn_raw_buffer_store_b128(w, __builtin_amdgcn_make_buffer_rsrc(out, 0, n * 4, 0x00020000), off, 0, /* sc1 */ 16);
                } else *reinterpret_cast<float4*>(at_byte(out, off)) = v;
            }
        } else {
#pragma unroll
            for (int s = 0; s < SLICES; s++)
                if (o4 + s * 256u < (unsigned)n * 4u) *at_byte(out, o4 + s * 256u) = q.res[s * 64 + lane];
        }
    }
    SPH_STAMP(5);
#if defined(SPH_STAMPS)
    if (lane == 0 && g_stamps) g_stamps[(size_t)wave_global * 8 + 4] = __builtin_amdgcn_s_memtime() - clk0;   // shader clocks of the wave's life
#endif
}


template <int VARIANT, int DIM>
__global__ __launch_bounds__(kBlock) void transform_kernel(const float* __restrict__ b1,
                                                          const float* __restrict__ b2, float* __restrict__ o1,
                                                          float* __restrict__ o2, int64_t n, int edge, int angle,
                                                          int jitter) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float x[5], y[5];
    load_box<DIM>(b1, i, x);
    load_box<DIM>(b2, i, y);
    transform_row<VARIANT, DIM>(x, y, edge, angle, jitter, o1 + i * 5, o2 + i * 5);
}


// ---- planar rotated IoU on given planar boxes (mmcv box_iou_rotated / diff_iou_rotated_2d values) ----
__global__ __launch_bounds__(kBlock) void planar_iou_kernel(const float* __restrict__ p1, int64_t m, const float* __restrict__ p2,
                                                           int64_t n, float* __restrict__ out, int aligned, int mode) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int64_t i = aligned ? j : (int64_t)blockIdx.y;
    if (j >= n) return;
    out[aligned ? j : i * n + j] = planar_pair(p1 + i * 5, p2 + j * 5, mode);
}

// ---- adjoint of the Sph2Pob transform: gradients of the planar boxes -> gradients of the spherical boxes ----
template <int VARIANT, int DIM>
__global__ __launch_bounds__(kBlock) void transform_bwd_kernel(const float* __restrict__ b1, const float* __restrict__ b2,
                                                              const float* __restrict__ g1, const float* __restrict__ g2,
                                                              float* __restrict__ gb1, float* __restrict__ gb2, int64_t n,
                                                              int edge, int jitter) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float x[5], y[5];
    load_box<DIM>(b1, i, x);
    load_box<DIM>(b2, i, y);
    transform_bwd_row<VARIANT, DIM, false>(x, y, g1 + i * 5, g2 + i * 5, edge, 0, jitter, gb1 + i * DIM, gb2 + i * DIM);
}

// adjoint of the reference-order transforms by forward-mode differentiation (legacy, rbb_angle='project')
template <int VARIANT, int DIM>
__global__ __launch_bounds__(kBlock) void transform_bwd_dual_kernel(const float* __restrict__ b1, const float* __restrict__ b2,
                                                                   const float* __restrict__ g1, const float* __restrict__ g2,
                                                                   float* __restrict__ gb1, float* __restrict__ gb2, int64_t n,
                                                                   int edge, int angle, int jitter) {
    int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    float x[5], y[5];
    load_box<DIM>(b1, i, x);
    load_box<DIM>(b2, i, y);
    transform_bwd_row<VARIANT, DIM, true>(x, y, g1 + i * 5, g2 + i * 5, edge, angle, jitter, gb1 + i * DIM, gb2 + i * DIM);
}

struct AlignedLaunch {
    const float *b1, *b2; float* out; int64_t n; int mode, edge, angle; hipStream_t s; bool fast = true;
    template <int V, int D> int run() {
        dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
        if (V <= 2 && n < ((int64_t)1 << 31) - 1024 && !g_no_compact) {
            // persistent-style grid.  Measured on MI355X (`tools/ab.py run --workload aligned ... label:SPH2POB_WGS_PER_CU=k`; round 1: tools/sweep_slices.sh): every CU must hold the same number of
            // workgroups (1 303 workgroups = 5.09 per CU take 12 % longer than 1 536 = 6 per CU); 6 per CU (24 waves per CU)
            // is the best or within noise of the best from 125 k to 8 M pairs; small launches want one slice per wave
            // rather than full survivor stacks.  Hence: whole multiples of the CU count, at most 6 per CU (and never
            // more than the LDS admits), at least one 64-pair slice per wave.
            const int64_t kCUs = cu_count();
            int64_t resident = (160 * 1024) / queue_lds_bytes(D);
            if (resident > (D == 4 ? 6 : 5)) resident = D == 4 ? 6 : 5;   // registers (__launch_bounds__) would admit 7 / 5
            int64_t slices = (n + 63) / 64;
            int64_t wgs = (slices + 3) / 4;
            if (g_slices_per_wave > 0) wgs = (slices + 4 * g_slices_per_wave - 1) / (4 * g_slices_per_wave);
            else if (wgs > kCUs) { wgs = (wgs + kCUs - 1) / kCUs * kCUs; if (wgs > kCUs * resident) wgs = kCUs * resident; }
            if (g_wgs_per_cu > 0) wgs = kCUs * g_wgs_per_cu;
            if (wgs < 1) wgs = 1;
            constexpr int VV = V > 2 ? 0 : V;
            const bool ref_finish = !fast || V == 2 || angle != SPH2POB_ANGLE_EQUATOR;
            const int edge_k = edge | (angle << 8);
#define SPH_PIPE(PF, ARC, REF) hipLaunchKernelGGL((iou_aligned_compact_kernel<VV, D, PF, ARC, REF>), dim3((unsigned)wgs), dim3(kBlock), 0, s, b1, b2, out, (int)n, mode, edge_k)
            if (!ref_finish && V < 2 && !g_persistent) {   // the default: one-round chunk kernel
                const unsigned cw = (unsigned)((n + kBlock * kChunkSlices - 1) / (kBlock * kChunkSlices));
                const int edge_k = edge | (angle << 8);
                // cull phase at a higher wave priority while (nearly) the whole grid is resident at once: see the kernel
                const bool prio = D == 4 && (int64_t)cw <= kCUs * 8 * 2 && !g_no_prio;
                const bool off32 = D == 4 && chunk_offsets_fit_u32(n, D);   // (RBFoV stays on 64-bit offsets: see the kernel)
                // whole-line stores need a 16-byte aligned output (a tensor view need not be); which form a size gets: see the kernel
                int stores = g_chunk_stores != CHUNK_STORES_AUTO ? g_chunk_stores : kChunkStoresDefault;
                if (!off32 || (reinterpret_cast<uintptr_t>(out) & 15) != 0) stores = CHUNK_STORES_DWORD;
#define SPH_CHUNK(ARC, O32, PRIO, LINES, WT) hipLaunchKernelGGL((iou_aligned_chunk_kernel<VV, D, ARC, kChunkSlices, O32, PRIO, LINES, WT>), dim3(cw), dim3(kBlock), 0, s, b1, b2, out, (int)n, mode, edge_k)
#define SPH_CHUNK_ARC(O32, PRIO, LINES, WT) do { if (edge == SPH2POB_EDGE_ARC) SPH_CHUNK(true, O32, PRIO, LINES, WT); else SPH_CHUNK(false, O32, PRIO, LINES, WT); } while (0)
#define SPH_CHUNK_STORES(PRIO) do { if (stores == CHUNK_STORES_WT) SPH_CHUNK_ARC(true, PRIO, true, true); else if (stores == CHUNK_STORES_LINES) SPH_CHUNK_ARC(true, PRIO, true, false); else SPH_CHUNK_ARC(true, PRIO, false, false); } while (0)
                // (a launch that is large enough for 64-bit offsets is far beyond two rounds: it never asks for the priority)
                if constexpr (D == 4) {   // (OFF32 and LINES are instantiated for BFoV only: the kernel's static_asserts)
                    if (!off32) SPH_CHUNK_ARC(false, false, false, false);
                    else if (prio) SPH_CHUNK_STORES(true);
                    else SPH_CHUNK_STORES(false);
                } else SPH_CHUNK_ARC(false, false, false, false);
#undef SPH_CHUNK_STORES
#undef SPH_CHUNK_ARC
#undef SPH_CHUNK
            } else
            if (ref_finish) { if (wgs > kCUs * 4) wgs = kCUs * 4; SPH_PIPE(true, false, true); }   // reference-order finish: 4 waves per SIMD
            else if (edge == SPH2POB_EDGE_ARC) { if (g_prefetch) SPH_PIPE(true, true, false); else SPH_PIPE(false, true, false); }
            else { if (g_prefetch) SPH_PIPE(true, false, false); else SPH_PIPE(false, false, false); }
#undef SPH_PIPE
        } else
            with_pair_sel<V>(fast, angle, [&](auto variant, auto fast_core) {
                hipLaunchKernelGGL((iou_aligned_kernel<decltype(variant)::value, D, decltype(fast_core)::value>), grid, dim3(kBlock), 0, s, b1, b2,
                                   out, n, mode, edge, angle);
            });
        return launch_status();
    }
};
struct TransformLaunch {
    const float *b1, *b2; float *o1, *o2; int64_t n; int edge, angle, jitter; hipStream_t s; bool fast = true;
    template <int V, int D> int run() {
        if constexpr (V > 2) return SPH2POB_ERR_OPTION;   // transform<V, D> computes nothing for the other IoU variants
        else {
            dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
            hipLaunchKernelGGL((transform_kernel<V, D>), grid, dim3(kBlock), 0, s, b1, b2, o1, o2, n, edge, angle, jitter);
            return launch_status();
        }
    }
};
// the two adjoints: the closed form (standard / efficient) or, DUAL, the dual-number one (legacy too)
template <bool DUAL>
struct TransformBwdLaunch {
    const float *b1, *b2, *g1, *g2; float *gb1, *gb2; int64_t n; int edge, angle, jitter; hipStream_t s; bool fast = true;
    template <int V, int D> int run() {
        if constexpr (V > (DUAL ? VARIANT_LEGACY : VARIANT_EFFICIENT)) return SPH2POB_ERR_OPTION;
        else {
            dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
            if constexpr (DUAL) hipLaunchKernelGGL((transform_bwd_dual_kernel<V, D>), grid, dim3(kBlock), 0, s, b1, b2, g1, g2, gb1, gb2, n, edge, angle, jitter);
            else hipLaunchKernelGGL((transform_bwd_kernel<V, D>), grid, dim3(kBlock), 0, s, b1, b2, g1, g2, gb1, gb2, n, edge, jitter);
            return launch_status();
        }
    }
};

}  // namespace

extern "C" {


int sph2pob_abi_version(void) { return SPH2POB_ABI_VERSION; }
const char* sph2pob_target_arch(void) { return "gfx950"; }

const char* sph2pob_error_string(int code) {
    switch (code) {
        case SPH2POB_OK: return "ok";
        case SPH2POB_ERR_NULL: return "null pointer with non-zero element count";
        case SPH2POB_ERR_DIM: return "box_dim must be 4 or 5 (legacy variant: 4 only)";
        case SPH2POB_ERR_OPTION: return "variant/mode/edge/angle/loss option out of range";
        case SPH2POB_ERR_SIZE: return "negative or too large element count";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown sph2pob error";
    }
}

int sph2pob_iou_aligned_f32(const float* b1, const float* b2, float* out, int64_t n, int box_dim, int variant,
                            int mode, int edge, int angle, void* stream) {
    const int rc = check_iou(box_dim, variant, mode, edge, angle, n, n, {b1, b2, out});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim, AlignedLaunch{b1, b2, out, n, mode, naive_edge(variant, edge), angle, (hipStream_t)stream});
}

int sph2pob_transform_f32(const float* b1, const float* b2, float* planar1, float* planar2, int64_t n,
                          int box_dim, int variant, int edge, int angle, int jitter, void* stream) {
    const int rc = check_transform(box_dim, variant, SPH2POB_VARIANT_LEGACY, edge, angle, n, {b1, b2, planar1, planar2});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim,
                    TransformLaunch{b1, b2, planar1, planar2, n, edge, angle, jitter, (hipStream_t)stream});
}

int sph2pob_planar_iou_f32(const float* p1, int64_t m, const float* p2, int64_t n, float* out, int aligned, int mode,
                           void* stream) {
    const int rc = check_planar_iou(p1, m, p2, n, out, aligned, mode);
    if (rc || m == 0 || n == 0) return rc;
    hipStream_t s = (hipStream_t)stream;
    const unsigned bx = (unsigned)((n + kBlock - 1) / kBlock);
    if (aligned) {
        hipLaunchKernelGGL(planar_iou_kernel, dim3(bx), dim3(kBlock), 0, s, p1, m, p2, n, out, 1, mode);
        return launch_status();
    }
    const int64_t kMaxRows = 65535;   // grid.y limit: walk the rows in slabs
    for (int64_t r0 = 0; r0 < m; r0 += kMaxRows) {
        const int64_t rows = m - r0 < kMaxRows ? m - r0 : kMaxRows;
        hipLaunchKernelGGL(planar_iou_kernel, dim3(bx, (unsigned)rows), dim3(kBlock), 0, s, p1 + r0 * 5, rows, p2, n,
                           out + r0 * n, 0, mode);
        if (const int launched = launch_status()) return launched;
    }
    return SPH2POB_OK;
}

int sph2pob_transform_bwd_f32(const float* b1, const float* b2, const float* grad_planar1, const float* grad_planar2,
                              float* grad_b1, float* grad_b2, int64_t n, int box_dim, int variant, int edge, int jitter,
                              void* stream) {
    const int rc = check_transform(box_dim, variant, SPH2POB_VARIANT_EFFICIENT, edge, 0, n, {b1, b2, grad_planar1, grad_planar2, grad_b1, grad_b2});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim,
                    TransformBwdLaunch<false>{b1, b2, grad_planar1, grad_planar2, grad_b1, grad_b2, n, edge, 0, jitter, (hipStream_t)stream});
}

int sph2pob_transform_bwd_general_f32(const float* b1, const float* b2, const float* grad_planar1,
                                      const float* grad_planar2, float* grad_b1, float* grad_b2, int64_t n, int box_dim,
                                      int variant, int edge, int angle, int jitter, void* stream) {
    const int rc = check_transform(box_dim, variant, SPH2POB_VARIANT_LEGACY, edge, angle, n, {b1, b2, grad_planar1, grad_planar2, grad_b1, grad_b2});
    if (rc || n == 0) return rc;
    return dispatch(variant, box_dim,
                    TransformBwdLaunch<true>{b1, b2, grad_planar1, grad_planar2, grad_b1, grad_b2, n, edge, angle, jitter, (hipStream_t)stream});
}

// Not part of the ABI (tests): the store form that SPH2POB_CHUNK_STORES forced when this copy was loaded: 0 none (the launcher's
// default), 1 dword, 2 lines, 3 write-through lines.
int sph2pob_debug_chunk_stores(void) { return g_chunk_stores; }

#if defined(SPH_STAMPS)
int sph2pob_debug_set_stamps(void* buffer) {
    unsigned long long* p = (unsigned long long*)buffer;
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), &p, sizeof(p));
}
#endif

}  // extern "C"
