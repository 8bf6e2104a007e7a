// libsph2pob_hip.so — pairwise IoU (the assigner call pattern), the MaxIoUAssigner epilogues, matrix and fused, and the fused
// assigner batched over a minibatch with the anchor-target construction as its epilogue — on the closed-form cull / compact /
// finish, or on any variant's per-pair function evaluated for every pair —: kernels + C-ABI launchers
// (include/sph2pob_hip.h).  gfx950 only.

#include <type_traits>

#include "sph2pob_kernels_common.hpp"
#include "sph2pob_assign.hpp"

namespace {

using namespace sph2pob_assign;   // the rule, the image's rows and the packed keys
static_assert(kBlock == sph2pob_assign::kTile, "one thread per column of a tile");

// a run-time flag as a compile-time one: the launchers pick a kernel's boolean template arguments through generic lambdas
template <class F>
auto with_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }

// ---- packed keys (ordered_bits, the column and the row key, unpack_max_val, wave_max_*: sph2pob_assign.hpp): what only the fused
// route adds ----
// what a row holds when no tile contributed (no ignore mask: IoU 0 at the shard's first column)
__device__ __forceinline__ unsigned long long row_floor(bool has_ignore, unsigned col_offset) {
    return has_ignore ? 0ull : pack_row_key(0.0f, col_offset);
}
// a per-GT accumulator (the maximum of the tiles' row keys, zero when no tile contributed) -> the GT's key, tie flag cleared
__device__ __forceinline__ unsigned long long acc_to_key(unsigned long long a, unsigned long long floor) { return (a > floor ? a : floor) & ~1ull; }
// keys travel between ranks as SIGNED 64-bit integers (torch.distributed has no unsigned MAX): top bit flipped
__device__ __forceinline__ long long key_to_signed(unsigned long long k) { return (long long)(k ^ 0x8000000000000000ull); }
__device__ __forceinline__ unsigned long long key_from_signed(long long k) { return (unsigned long long)k ^ 0x8000000000000000ull; }

// ---- one layout of the fused routes' two buffers, per image, in 64-bit words.
// workspace: col_part[chunks][n], then row_part[k][tiles] (what pairwise_compact_tile writes; overwritten by every call).
// state (zero between calls): one u64 accumulator per GT; the finalize pass's arrival counters; batched only, one line for the
// image's packed (positives | negatives << 32) count; and, batched only, behind the LAST image one line: [0] images that
// finished, [1] sum of max(positives, 1).  The batched route lays every image out for k_max rows whatever its own count; the
// single-image route is one image without the count lines. ----
constexpr int kAccLine = 8;        // u64 words per 64-byte line: every counter has a line of its own
// column tiles per first-level arrival counter; one more counter takes the groups' arrivals (a single counter serialises one
// returning atomic per workgroup: 1 535 tiles = +13 us, profiles/r05b_trace_fused_one_counter.txt)
constexpr int kTicketGroup = 32;
// distance of the accumulators: 256 bytes for k <= 1024, so that the GTs' atomics spread over memory channels (64 x 392 832
// anchors: 70.2 -> 65.5 us, profiles/r05d_ab_fused_stride.log; 16 slots per GT instead made the finalize pass read 64 KB per
// workgroup: slower, profiles/r05e_ab_fused_slots.log)
__host__ __device__ inline int64_t acc_stride(int64_t k) { return k <= 1024 ? 32 : 1; }
__host__ __device__ inline int64_t col_tiles(int64_t n) { return (n + kBlock - 1) / kBlock; }
__host__ __device__ inline int64_t ticket_groups(int64_t tiles) { return (tiles + kTicketGroup - 1) / kTicketGroup; }
struct Layout {
    int64_t tiles, chunks;               // column tiles of kBlock anchors; row chunks col_part has room for
    int64_t row_part, ws_words;          // workspace: col_part at 0, row_part, the image's words
    int64_t stride, counters;            // state: accumulator i at i * stride; counters[0]: top, [(1 + g) * kAccLine]: group g
    int64_t count, state_words;          // state: the image's count line (batched), the image's words
};
// k rows (k_max of the batch), n columns in `tiles` = col_tiles(n) tiles (a finalize kernel has them as its grid), `chunks` row
// chunks (the state does not depend on them)
__host__ __device__ inline Layout layout(int64_t k, int64_t n, int64_t tiles, int64_t chunks, bool batched) {
    Layout l;
    l.tiles = tiles;
    l.chunks = chunks;
    l.row_part = chunks * n;
    l.ws_words = l.row_part + k * l.tiles;
    l.stride = acc_stride(k);
    l.counters = (k * l.stride + kAccLine - 1) / kAccLine * kAccLine;
    l.count = l.counters + (1 + ticket_groups(l.tiles)) * kAccLine;
    l.state_words = l.count + (batched ? kAccLine : 0);
    return l;
}
__host__ __device__ inline int64_t row_chunks(int64_t k, int64_t rows_per_wg) { return k > 0 ? (k + rows_per_wg - 1) / rows_per_wg : 0; }

// ---- pairwise IoU for the assigner call pattern (few rows x many columns), closed-form core ----
// One thread owns one column box (anchor); a workgroup covers 256 columns x up to 64 rows (GT).  Per-box cull
// quantities are hoisted: rows live in LDS (broadcast reads), the column's in registers, so a culled pair costs
// ~15 VALU instructions + one coalesced store of 0.  Survivors are (row, column) index pairs pushed on the wave's
// LDS stack and finished 64 at a time on fully populated waves (same scheme as iou_aligned_compact_kernel); the < 64
// leftovers of the four waves are merged once at the end and finished on as few, as full waves as possible (with 8 rows per
// workgroup a wave stacks ~80 survivors: one full pass and a 16-lane one without the merge).
// ARC: rbb_edge == 'arc' folded at compile time, as in the aligned kernels (with a run-time edge the chord / tangent forms
// made this kernel 47 KB of code at 84 VGPRs).
// OUT: bit 0 = write the m x n matrix; bit 1 = the assigner's reductions (max_iou_assigner.py:171-176 without
// the matrix) — every finished survivor with IoU > 0 goes into the tile's per-column and per-row maxima in LDS (ds_max_u64 on
// packed keys; culled pairs and survivors that finish to 0 are covered by the initial values: exact zeros), written once per
// workgroup as
//   col_part[chunk][j]      max over the chunk's rows of (IoU[i][j], first row)         (chunk = blockIdx row chunk)
//   row_part[i][tile]       max over the tile's 256 columns of (IoU[i][j], first column, global index = col_offset + j),
//                           bit 0 = the value may occur at more than one column of the tile
//   row_acc[i * stride]     atomic max of the row's partials over ALL tiles (zero before the launch)
// `ignore` (optional, one byte per column): columns whose overlaps the assigner sets to -1 (max_iou_assigner.py:115-126)
// — they take part in no row maximum, their column maximum is (-1, row 0), and the matrix, when written, holds -1.
constexpr int kPwRows = 64;    // rows of one workgroup at most
constexpr int kRowSlots = 4;   // LDS copies of a row's running maximum (lane & 3): a pass holds a few rows, 64 lanes on one address serialise
// The tile's work, shared by the single-image kernel and the batched one (anchor_targets_pairwise_kernel): column tile bx of
// `tiles`, row chunk by; `stride` = distance of the per-GT accumulators in row_acc (Layout::stride).
template <int VARIANT, int DIM, bool ARC, int OUT>
__device__ __forceinline__ void pairwise_compact_tile(const float* __restrict__ b1, int m, const float* __restrict__ b2, int n,
                                                      float* __restrict__ out, int mode, int edge_arg, int rows_per_wg,
                                                      const unsigned char* __restrict__ ignore,
                                                      unsigned long long* __restrict__ col_part,
                                                      unsigned long long* __restrict__ row_part, unsigned col_offset,
                                                      unsigned long long* __restrict__ row_acc, const int bx, const int by,
                                                      const int tiles, const int64_t stride) {
    constexpr bool MATRIX = (OUT & 1) != 0, REDUCE = (OUT & 2) != 0;
    __shared__ float row_raw[kPwRows][5];
    __shared__ float4 row_cull[kPwRows];
    __shared__ int2 stack[kBlock / 64][kQCap];
    __shared__ int leftover[kBlock / 64];
    // sin / cos of every box's jittered colatitude, once per box instead of once per surviving pair (two of the three
    // sincos of a finishing pass): rows by their first threads, columns by their owner; the finishing lane — any lane,
    // the survivors are compacted — reads them by index
    __shared__ ColatTrig row_trig[kPwRows];
    __shared__ ColatTrig col_trig[kBlock];
    __shared__ float col_raw[DIM][kBlock];   // the finishing lanes read the column's box here, not from global memory (bit-equal;
                                             // fused 64 x 98 208: 31.2 -> 30.5 us, 64 x 392 832: 57.4 -> 53.6: profiles/r05a_ab_fused_variants.log)
    __shared__ int row_tie[REDUCE ? kPwRows : 1];
    __shared__ unsigned long long col_key[REDUCE ? kBlock : 1];
    __shared__ unsigned long long row_key[REDUCE ? kPwRows : 1][kRowSlots];
    __shared__ unsigned long long tile_base;   // what a row holds before any survivor: (0, first live column) or (-1, first ignored one)
    const int edge = ARC ? (int)EDGE_ARC : edge_arg;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r0 = by * rows_per_wg, rows = (m - r0 < rows_per_wg) ? m - r0 : rows_per_wg;
    if ((int)threadIdx.x < rows) {
        float g[5];
        load_box<DIM>(b1, r0 + threadIdx.x, g);
        CullBox cg = cull_box(g, edge);
#pragma unroll
        for (int k = 0; k < 5; k++) row_raw[threadIdx.x][k] = g[k];
        row_cull[threadIdx.x] = make_float4(cg.s, cg.c, cg.th_rev, cg.r);
        row_trig[threadIdx.x] = colat_trig(g[1], 1);
    }
    const int j = bx * kBlock + threadIdx.x;
    const bool valid = j < n;
    float a[5] = {0.0f, 0.0f, 1.0f, 1.0f, 0.0f};
    if (valid) load_box<DIM>(b2, j, a);
    const bool ign = (REDUCE || MATRIX) && ignore != nullptr && valid && ignore[j] != 0;
    const bool live = valid & !ign;
    col_trig[threadIdx.x] = colat_trig(a[1], 2);
#pragma unroll
    for (int k = 0; k < DIM; k++) col_raw[k][threadIdx.x] = a[k];
    if constexpr (REDUCE) {
        col_key[threadIdx.x] = pack_max_key(ign ? -1.0f : 0.0f, r0);
        if (threadIdx.x < kPwRows * kRowSlots) (&row_key[0][0])[threadIdx.x] = 0ull;
        if (kPwRows * kRowSlots > kBlock && threadIdx.x + kBlock < kPwRows * kRowSlots) (&row_key[0][0])[threadIdx.x + kBlock] = 0ull;
        if (threadIdx.x == 0) tile_base = 0ull;
        if (threadIdx.x < kPwRows) row_tie[threadIdx.x] = 0;
    }
    __syncthreads();
    if constexpr (REDUCE) {   // first live / first ignored column of each wave -> the tile's base key (a max over <= 8 candidates)
        const unsigned long long ml = __builtin_amdgcn_ballot_w64(live), mi = __builtin_amdgcn_ballot_w64(ign);
        if (lane == 0) {
            const int jw = bx * kBlock + wave * 64;
            if (ml) atomicMax(&tile_base, pack_row_key(0.0f, col_offset + jw + __builtin_ctzll(ml)));
            if (mi) atomicMax(&tile_base, pack_row_key(-1.0f, col_offset + jw + __builtin_ctzll(mi)));
        }
    }
    const CullBox ca = cull_box(a, edge);
    int2* st = stack[wave];
    int count = 0;
    auto finish_one = [&](int2 e) {
        float g[5], p[5];
#pragma unroll
        for (int k = 0; k < 5; k++) g[k] = row_raw[e.x][k];
#pragma unroll
        for (int k = 0; k < 5; k++) p[k] = k < DIM ? col_raw[k < DIM ? k : 0][e.y - bx * kBlock] : 0.0f;
        const float v = lean_finish<VARIANT, DIM, 1>(g, p, mode, edge, row_trig[e.x], col_trig[e.y - bx * kBlock]);
        if constexpr (MATRIX) out[(int64_t)(r0 + e.x) * n + e.y] = v;
        if constexpr (REDUCE) if (!(v <= 0.0f)) {   // > 0 or NaN: zeros are the initial values
            atomicMax(&col_key[e.y - bx * kBlock], pack_max_key(v, r0 + e.x));
            // the value already in the slot (a column of this row finished earlier) — equal value bits = a tie inside the tile
            const unsigned long long key = pack_row_key(v, col_offset + e.y);
            const unsigned long long old = atomicMax(&row_key[e.x][lane & (kRowSlots - 1)], key);
            if ((unsigned)(old >> 32) == (unsigned)(key >> 32)) row_tie[e.x] = 1;
        }
    };
    float* orow = out + (int64_t)r0 * n + j;   // this column's element of the tile's first row (cull rows at a higher
                                               // wave priority than the passes, as in the chunk kernel: no gain here)
    for (int i = 0; i < rows; i++) {
        const float4 rc = row_cull[i];
        const bool culled = cull_pair(CullBox{rc.x, rc.y, rc.z, rc.w}, ca), surv = live & !culled;
        if constexpr (MATRIX) {
            if (valid & (culled | ign)) *orow = ign ? -1.0f : 0.0f;
            orow += n;
        }
        const unsigned long long mk = __builtin_amdgcn_ballot_w64(surv);
        if (surv) st[count + rank_below(mk)] = make_int2(i, j);
        count += __popcll(mk);
        if (count >= 64) {
            count -= 64;
            wave_lds_fence();
            finish_one(st[count + lane]);
        }
    }
    // merge the < 64 leftovers of the four waves
    if (lane == 0) leftover[wave] = count;
    // LDS only: __syncthreads() would also wait for the acknowledgement of every store above (vmcnt(0))
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
    const int c0 = leftover[0], c1 = leftover[1], c2 = leftover[2], c3 = leftover[3];
    const int total = c0 + c1 + c2 + c3;   // <= 252: at most one chunk per wave
    if (wave * 64 < total) {
        int k = wave * 64 + lane;
        if (k < total) {
            int w = 0;
            if (k >= c0) { k -= c0; w = 1; if (k >= c1) { k -= c1; w = 2; if (k >= c2) { k -= c2; w = 3; } } }
            finish_one(stack[w][k]);
        }
    }
    if constexpr (REDUCE) {
        asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
        if (valid) col_part[(int64_t)by * n + j] = col_key[threadIdx.x];
        if ((int)threadIdx.x < rows) {
            unsigned long long best = tile_base;
#pragma unroll
            for (int t = 0; t < kRowSlots; t++) { const unsigned long long v = row_key[threadIdx.x][t]; best = v > best ? v : best; }
            int same = 0;   // slots that hold the maximum VALUE (each at a column of its own)
#pragma unroll
            for (int t = 0; t < kRowSlots; t++) same += (unsigned)(row_key[threadIdx.x][t] >> 32) == (unsigned)(best >> 32);
            // flag: conservative (a tie seen at a lower value also sets it; the finalize pass then only re-evaluates for nothing)
            row_part[(int64_t)(r0 + threadIdx.x) * tiles + bx] = best | (unsigned long long)(row_tie[threadIdx.x] | (same > 1));
            // the row's running maximum over all tiles: relaxed device-scope atomic, only from tiles that hold something
            // above the rows' common floor (0 at the shard's first column) — with an ignore mask the floor is not known
            // here, and every tile contributes
            if (ignore != nullptr || (unsigned)(best >> 32) > 0x80000000u)
                __hip_atomic_fetch_max(row_acc + (r0 + threadIdx.x) * stride, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

// Dispatch order of the tiles = LAST column tile first, all of its row chunks, then the tile before it: anchor grids end with their
// coarsest level (mmdet's AnchorGenerator walks the strides upwards) and their tiles grow heavier towards the end —
// the coarsest anchors survive the cull against nearly every GT and carry the longest serial chains of passes —, and
// the grid is larger than what is resident at once: dispatched last, the heaviest tiles started last.  Heaviest first:
// 64 x 98 208 anchors 21.7 -> 18.5 us, 64 x 392 832 47.2 -> 41.3 us with the rows-per-workgroup rule retuned for it
// (profiles/r03y_ab_pairwise*.log, r03z_ab_pairwise.log); tiles taken from both ends inwards instead: 20.2 / 42.1 us.
// A caller that lists the coarse level first gets the previous behaviour.  (tiles x chunks <= m n / 1024 + ..., and the
// m x n matrix has to fit the device: the linear id stays far below 2^32.  The same order from a transposed grid —
// chunks on x, tiles on y, no division — measured 1 % slower at 392 832 anchors: r04b_ab_pairwise_transposed.log.)
struct TileId { int bx, by; };   // column tile, row chunk
__device__ __forceinline__ TileId tail_first_tile() {   // grid (tiles, chunks[, images])
    const unsigned lid = blockIdx.y * gridDim.x + blockIdx.x;
    return TileId{(int)(gridDim.x - 1 - lid / gridDim.y), (int)(lid % gridDim.y)};
}

template <int VARIANT, int DIM, bool ARC, int OUT>
__global__ __launch_bounds__(kBlock, ARC ? 8 : 4) void iou_pairwise_compact_kernel(const float* __restrict__ b1, int m,
        const float* __restrict__ b2, int n, float* __restrict__ out, int mode, int edge_arg, int rows_per_wg,
        const unsigned char* __restrict__ ignore, unsigned long long* __restrict__ col_part, unsigned long long* __restrict__ row_part,
        unsigned col_offset, unsigned long long* __restrict__ row_acc) {
    const TileId t = tail_first_tile();
    pairwise_compact_tile<VARIANT, DIM, ARC, OUT>(b1, m, b2, n, out, mode, edge_arg, rows_per_wg, ignore, col_part, row_part, col_offset,
                                                  row_acc, t.bx, t.by, (int)gridDim.x, acc_stride(m));
}

// out[i*n + j]: consecutive lanes walk j (coalesced stores, b2 loads coalesced, b1 row is a broadcast).
template <int VARIANT, int DIM, bool FAST>
__global__ __launch_bounds__(kBlock) void iou_pairwise_kernel(const float* __restrict__ b1, int64_t m,
                                                             const float* __restrict__ b2, int64_t n,
                                                             float* __restrict__ out, int mode, int edge,
                                                             int angle) {
    int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    int64_t i = blockIdx.y;
    if (j >= n) return;
    float x[5], y[5];
    load_box<DIM>(b1, i, x);
    load_box<DIM>(b2, j, y);
    out[i * n + j] = pair_iou_sel<VARIANT, DIM, FAST>(x, y, mode, edge, angle);
}


// ---- MaxIoUAssigner epilogue: replaces overlaps.max(dim=0), overlaps.max(dim=1), the threshold steps
// and the python `for i in range(num_gts)` low-quality loop (one host sync per GT) of
// mmdet/core/bbox/assigners/max_iou_assigner.py:171-207 with three launches over the (k, n) overlaps matrix. ----
// A: one thread per column (anchor): running max / first argmax over the k rows, and per-wave row partials.
// Rows are taken 32 at a time: 32 independent coalesced loads per lane (unconditional, on clamped addresses, into a
// register array: written as `live ? ov[..] : -inf` each load sat behind its own branch and its own wait — 64 serial
// round trips per lane, 20 us instead of 9 for 64 x 98 208; requesting the NEXT round's 32 before this round's butterfly
// was measured too: 18.1 -> 17.4 us for the three kernels at 98 208 anchors, 41.2 -> 44.9 us at 392 832, not kept:
// r03r_ab_assign.log), then a transposing butterfly — at the stage
// with lane mask M a lane keeps the lower (bit clear) or upper (bit set) half of its rows and receives the partner's
// copy of that half — leaves lane L with the wave-wide maximum key of row (L >> 1) after 31 + 1 exchanges, instead of
// one 6-step wave reduction per row (192 exchanges per 32 rows).
constexpr int kAssignRows = 32;
__global__ __launch_bounds__(kBlock) void assign_cols_kernel(const float* __restrict__ ov, int k, int64_t n,
                                                            float* __restrict__ max_ov, int64_t* __restrict__ argmax_ov,
                                                            unsigned long long* __restrict__ partial, int nparts) {
    const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int part = blockIdx.x * (kBlock / 64) + (threadIdx.x >> 6);
    const bool valid = j < n;
    const int64_t jc = valid ? j : n - 1;   // clamp the address, mask the value
    const unsigned long long lane_mask = valid ? ~0ull : 0ull;   // a mask, not a select: selects here compile to 32 branches
    float best = -__builtin_inff();
    int besti = 0;
    for (int r0 = 0; r0 < k; r0 += kAssignRows) {
        unsigned long long key[kAssignRows];
        float raw[kAssignRows];
#pragma unroll
        for (int t = 0; t < kAssignRows; t++)   // unconditional (clamped addresses): all 32 loads are issued before the first wait
            raw[t] = ov[(int64_t)(r0 + t < k ? r0 + t : k - 1) * n + jc];
#pragma unroll
        for (int t = 0; t < kAssignRows; t++) {
            const int i = r0 + t;
            const float v = (valid && i < k) ? raw[t] : -__builtin_inff();
            const bool up = v > best || (v != v && best == best);   // torch.max: the first NaN is the maximum and stays
            best = up ? v : best;
            besti = up ? i : besti;
            key[t] = pack_max_key(v, j) & lane_mask;   // rows past k are reduced but never written
        }
#pragma unroll
        for (int cnt = kAssignRows, m = 32; cnt > 1; cnt >>= 1, m >>= 1) {
            const bool upper = (lane & m) != 0;
            const int half = cnt >> 1;
#pragma unroll
            for (int t = 0; t < half; t++) {
                const unsigned long long mine = upper ? key[t + half] : key[t];
                const unsigned long long send = upper ? key[t] : key[t + half];
                const unsigned long long recv = __shfl_xor(send, m, 64);
                key[t] = recv > mine ? recv : mine;
            }
        }
        const unsigned long long other = __shfl_xor(key[0], 1, 64);
        const unsigned long long row_max = other > key[0] ? other : key[0];
        const int i = r0 + (lane >> 1);
        if ((lane & 1) == 0 && i < k) partial[(int64_t)i * nparts + part] = row_max;
    }
    if (valid) { max_ov[j] = best; argmax_ov[j] = besti; }
}
// B: one workgroup per row (GT): reduce the per-wave partials
__global__ __launch_bounds__(kBlock) void assign_rows_kernel(const unsigned long long* __restrict__ partial, int nparts,
                                                            float* __restrict__ gt_max, int64_t* __restrict__ gt_argmax) {
    __shared__ unsigned long long sm[kBlock / 64];
    const int i = blockIdx.x;
    unsigned long long best = 0ull;
    for (int p0 = threadIdx.x; p0 < nparts; p0 += kBlock * 8) {   // 8 independent loads per round (a repeated last partial changes no maximum)
        unsigned long long v[8];
#pragma unroll
        for (int t = 0; t < 8; t++) {
            const int p = p0 + t * kBlock;
            v[t] = partial[(int64_t)i * nparts + (p < nparts ? p : nparts - 1)];
        }
#pragma unroll
        for (int t = 0; t < 8; t++) best = v[t] > best ? v[t] : best;
    }
    best = wave_max_u64(best);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = best;
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int w = 1; w < kBlock / 64; w++) best = sm[w] > best ? sm[w] : best;
        gt_max[i] = unpack_max_val(best);
        gt_argmax[i] = max_key_index(best);
    }
}
// C: thresholds + low-quality matching, one thread per column; later GTs overwrite earlier ones like the python loop
__global__ __launch_bounds__(kBlock) void assign_finalize_kernel(const float* __restrict__ ov, int k, int64_t n,
        const float* __restrict__ max_ov, const int64_t* __restrict__ argmax_ov, const float* __restrict__ gt_max,
        const int64_t* __restrict__ gt_argmax, float pos_thr, float neg_lo, float neg_hi, float min_pos, int low_quality, int assign_all,
        const int64_t* __restrict__ gt_labels, int64_t* __restrict__ gt_inds, int64_t* __restrict__ labels) {
    const Rule rule{pos_thr, neg_lo, neg_hi, min_pos, low_quality, assign_all};
    const int64_t jraw = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const bool valid = jraw < n;
    const int64_t j = valid ? jraw : n - 1;   // lanes past the end stay in the wave (v_readlane below reads lanes 0..31) and store nothing
    const float m = max_ov[j];
    const int64_t am = argmax_ov[j];   // unconditional: one round trip for both, not two
    int64_t a = threshold_index(m, am, rule);
    if (rule.low_quality) {
        if (rule.assign_all) {   // the column is re-read, 32 rows at a time: unconditional (clamped) loads, all issued before the first wait
            for (int r0 = 0; r0 < k; r0 += kAssignRows) {
                float raw[kAssignRows];
#pragma unroll
                for (int t = 0; t < kAssignRows; t++) raw[t] = ov[(int64_t)(r0 + t < k ? r0 + t : k - 1) * n + j];
                // the 32 row maxima of this round in one vector load (lane t holds row r0 + t), handed out with v_readlane;
                // a row past k or below min_pos becomes NaN, which equals nothing
                const int il = r0 + (int)(threadIdx.x & (kAssignRows - 1));
                const float gl = gt_max[il < k ? il : k - 1];
                const int gbits = __float_as_int((il < k && gl >= rule.min_pos) ? gl : __builtin_nanf(""));
#pragma unroll
                for (int t = 0; t < kAssignRows; t++) {
                    const float g = __int_as_float(__builtin_amdgcn_readlane(gbits, t));
                    a = raw[t] == g ? r0 + t + 1 : a;
                }
            }
        } else {
            for (int i = 0; i < k; i++)
                if (gt_max[i] >= rule.min_pos && gt_argmax[i] == j) a = i + 1;
        }
    }
    if (!valid) return;
    gt_inds[j] = a;
    if (labels) labels[j] = a > 0 ? gt_labels[a - 1] : -1;
}

// ---- fused assigner (no k x n matrix): phase 2 and 3 behind iou_pairwise_compact_kernel<.., OUT & 2> ----
// B' (the sharded form only): accumulators -> signed-order keys for the all-reduce; leaves the accumulators zero
__global__ __launch_bounds__(kBlock) void assign_keys_from_acc_kernel(unsigned long long* __restrict__ row_acc, int k, bool has_ignore,
                                                                     unsigned col_offset, long long* __restrict__ gt_keys) {
    const unsigned long long fl = row_floor(has_ignore, col_offset);
    for (int i = threadIdx.x; i < k; i += kBlock) {
        gt_keys[i] = key_to_signed(acc_to_key(row_acc[i * acc_stride(k)], fl));
        row_acc[i * acc_stride(k)] = 0ull;
    }
}
// ---- the per-pair function of C's re-evaluation (below), phase 1's by construction: `column` takes the lane's column once (j
// clamped to n - 1 past the end), `row` gives that column's IoU with GT row i. ----
// standard / efficient in the closed form: the cull and the finishing pass of pairwise_compact_tile
template <int VARIANT, int DIM, bool ARC>
struct ClosedFormPair {
    int edge;
    float a5[5] = {0.0f, 0.0f, 1.0f, 1.0f, 0.0f};
    bool have_column = false;
    CullBox ca{};
    ColatTrig ct{};
    __device__ __forceinline__ explicit ClosedFormPair(int edge_arg) : edge(ARC ? (int)EDGE_ARC : edge_arg) {}
    __device__ __forceinline__ void column(const float* __restrict__ b2, int j, bool valid) {
        if (valid) load_box<DIM>(b2, j, a5);
        ca = cull_box(a5, edge);
        ct = colat_trig(a5[1], 2);
        have_column = true;
    }
    __device__ __forceinline__ float row(const float* __restrict__ b1, int i) const {
        float g5[5];
        load_box<DIM>(b1, i, g5);
        const CullBox cg = cull_box(g5, edge);
        float v = 0.0f;
        if (!cull_pair(cg, ca)) v = lean_finish<VARIANT, DIM, 1>(g5, a5, MODE_IOU, edge, colat_trig(g5[1], 1), ct);
        return v;
    }
};
// every other variant: the function iou_pairwise_kernel runs for it in the default arithmetic with rbb_angle='equator' (`edge`
// carries SPH2POB_FLAG_NAIVE_TAN as EDGE_TANGENT, as in the pairwise entry) — the reference-order core for legacy / Sph-IoU /
// FoV-IoU, which have no other, the fast selection for the unbiased and the naive IoU (pair_sel_fast, sph2pob_iou_entry.hpp)
template <int VARIANT, int DIM>
__device__ __forceinline__ float per_pair_iou(const float (&g)[5], const float (&a)[5], int edge) {
    return pair_iou_sel<VARIANT, DIM, pair_sel_fast(VARIANT, true, ANGLE_EQUATOR)>(g, a, (int)MODE_IOU, edge, (int)ANGLE_EQUATOR);
}
template <int VARIANT, int DIM>
struct PerPairFunction {
    int edge;
    float a5[5];
    bool have_column = false;
    __device__ __forceinline__ explicit PerPairFunction(int edge_arg) : edge(edge_arg) {}
    __device__ __forceinline__ void column(const float* __restrict__ b2, int j, bool) {
        load_box<DIM>(b2, j, a5);
        have_column = true;
    }
    __device__ __forceinline__ float row(const float* __restrict__ b1, int i) const {
        float g5[5];
        load_box<DIM>(b1, i, g5);
        return per_pair_iou<VARIANT, DIM>(g5, a5, edge);
    }
};
template <int VARIANT, int DIM, bool ARC>
using PairOf = std::conditional_t<(VARIANT < VARIANT_LEGACY), ClosedFormPair<(VARIANT < VARIANT_LEGACY ? VARIANT : 0), DIM, ARC>, PerPairFunction<VARIANT, DIM>>;

// C': one workgroup per column tile (the tiles of phase 1).  Column maxima from the row chunks' partials, thresholds, and
// the low-quality step (max_iou_assigner.py:192-207) without the matrix: `overlaps[i, :] == gt_max[i]` can hold in this tile
//   * for gt_max[i] == 0 on every column that is not ignored (nothing overlaps GT i: every live IoU of the row is 0);
//   * for gt_max[i] == -1 on every ignored column (the whole row is ignored columns);
//   * for gt_max[i] > 0 only if the TILE's maximum of row i (row_part, still in the workspace) equals it — then at the
//     column the partial names and, only when phase 1 saw the value at a second column of the tile (bit 0 of the partial:
//     duplicated boxes, mirror-symmetric anchors), wherever a re-evaluation of the row against the tile's 256 columns with
//     the very functions phase 1 ran (same inputs, same bits) finds it.
// Later GTs overwrite earlier ones in the reference's loop: the largest matching i wins.
// FROM_ACC: the per-GT keys are phase 1's accumulators (one device); the last workgroup to finish zeroes them and the arrival
// counter for the next call.  Otherwise they are `gt_keys` (all-reduced by the caller).
// The column's share of C', common to the single-image kernel and the batched one (anchor_targets_finalize_kernel): returns
// the assigned index (-1 / 0 / GT + 1) of column `tile * 256 + threadIdx.x` (clamped to n - 1 past the end) and its maximum
// (m, am).  `stride`: distance of the per-GT accumulators (Layout::stride).
template <int VARIANT, int DIM, bool ARC, bool FROM_ACC>
__device__ __forceinline__ int64_t fused_finalize_column(const float* __restrict__ b1, int k, const float* __restrict__ b2, int n,
        int edge_arg, const unsigned long long* __restrict__ col_part, int chunks, const unsigned long long* __restrict__ row_part,
        const long long* __restrict__ gt_keys, unsigned long long* __restrict__ row_acc, const int64_t stride, bool has_ignore,
        unsigned col_offset, const Rule& rule, float* __restrict__ gt_max, int64_t* __restrict__ gt_argmax, const int tile, const int tiles,
        float& m_out, int64_t& am_out) {
    const int lane = threadIdx.x & 63;
    const int jraw = tile * kBlock + threadIdx.x;
    const bool valid = jraw < n;
    const int j = valid ? jraw : n - 1;
    const unsigned long long fl = row_floor(has_ignore, col_offset);
    auto row_key_of = [&](int i) -> unsigned long long {
        if (FROM_ACC) return acc_to_key(row_acc[i * stride], fl);
        return key_from_signed(gt_keys[i]);
    };
    if (tile == 0 && gt_max) {   // the per-GT results, decoded once
        for (int i = threadIdx.x; i < k; i += kBlock) {
            const unsigned long long key = row_key_of(i);
            gt_max[i] = unpack_max_val(key);
            if (gt_argmax) gt_argmax[i] = (int64_t)row_key_index(key);
        }
    }
    unsigned long long ck = 0ull;
    for (int c0 = 0; c0 < chunks; c0 += 8) {   // 8 independent loads per round (a repeated last chunk changes no maximum)
        unsigned long long v[8];
#pragma unroll
        for (int t = 0; t < 8; t++) v[t] = col_part[(int64_t)(c0 + t < chunks ? c0 + t : chunks - 1) * n + j];
#pragma unroll
        for (int t = 0; t < 8; t++) ck = v[t] > ck ? v[t] : ck;
    }
    const float m = unpack_max_val(ck);
    const int64_t am = max_key_index(ck);
    const bool ign = m < 0.0f;   // only an ignored column has a negative maximum
    int64_t a = threshold_index(m, am, rule);
    if (rule.low_quality) {
        int best = -1;
        if (!rule.assign_all) {
            for (int i = 0; i < k; i++) {
                const unsigned long long key = row_key_of(i);
                if (unpack_max_val(key) >= rule.min_pos && row_key_index(key) == col_offset + (unsigned)j) best = i;
            }
        } else {
            PairOf<VARIANT, DIM, ARC> pair(edge_arg);
            for (int r0 = 0; r0 < k; r0 += 64) {
                const int il = r0 + lane, ic = il < k ? il : k - 1;
                const unsigned long long gk = row_key_of(ic);
                const float g = unpack_max_val(gk);
                const bool on = il < k && g >= rule.min_pos;
                const unsigned long long zero = __builtin_amdgcn_ballot_w64(on && g == 0.0f);
                const unsigned long long neg = __builtin_amdgcn_ballot_w64(on && g == -1.0f);
                const unsigned long long pk = row_part[(int64_t)ic * tiles + tile];
                const bool here = on && g > 0.0f && (unsigned)(pk >> 32) == (unsigned)(gk >> 32);   // the row's maximum lives in this tile
                unsigned long long rec = __builtin_amdgcn_ballot_w64(here && (pk & 1ull));              // ... maybe at several columns
                unsigned long long one = __builtin_amdgcn_ballot_w64(here && !(pk & 1ull));             // ... at the one the partial names
                if (!ign && zero) best = r0 + 63 - __builtin_clzll(zero);
                if (ign && neg) { const int t = r0 + 63 - __builtin_clzll(neg); best = t > best ? t : best; }
                while (one) {   // wave-uniform; descending, so the first hit is the largest row
                    const int t = 63 - __builtin_clzll(one);
                    one &= ~(1ull << t);
                    const unsigned col = row_key_index(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)pk, t)));
                    if (valid && col == col_offset + (unsigned)j && r0 + t > best) best = r0 + t;
                }
                while (rec) {   // wave-uniform: rows whose maximum lives in this tile
                    const int t = __builtin_ctzll(rec);
                    rec &= rec - 1;
                    if (!pair.have_column) pair.column(b2, j, valid);
                    const float v = pair.row(b1, r0 + t);
                    const float gm = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(g), t));
                    if (!ign && v == gm && r0 + t > best) best = r0 + t;
                }
            }
        }
        if (best >= 0) a = best + 1;
    }
    m_out = m;
    am_out = am;
    return a;
}
// Arrival of one finalize workgroup at the two-level counters behind the accumulators (a returning atomic per workgroup on ONE
// address serialises): the last of each group of 32 tiles reports to the top counter; true (for the whole workgroup) in the
// last workgroup of the last group to report.  counters[0]: top, [1 + g]: group g, kAccLine words apart.  `extra` (thread 0's)
// is added to the first atomic: a caller passes 0 made to depend on an earlier returning atomic, which orders the two.
__device__ __forceinline__ bool finalize_arrive(unsigned long long* __restrict__ counters, const int tile, const int tiles, const unsigned extra = 0u) {
    __shared__ unsigned ticket;
    const int groups = (int)ticket_groups(tiles), grp = tile / kTicketGroup;
    const int members = grp == groups - 1 ? tiles - grp * kTicketGroup : kTicketGroup;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned t = __hip_atomic_fetch_add((unsigned*)(counters + (int64_t)(1 + grp) * kAccLine), 1u + extra, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        unsigned last = 0;
        if ((int)t == members - 1)
            last = (int)__hip_atomic_fetch_add((unsigned*)counters, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == groups - 1;
        ticket = last;
    }
    __syncthreads();
    return ticket != 0;
}
// what the last arrival does for the next call: the image's accumulators (the k rows it used) and every counter back to zero
__device__ __forceinline__ void reset_image_state(unsigned long long* __restrict__ acc, int k, const Layout& l) {
    for (int i = threadIdx.x; i < k; i += kBlock) acc[i * l.stride] = 0ull;
    for (int i = threadIdx.x; i <= (int)ticket_groups(l.tiles); i += kBlock) acc[l.counters + (int64_t)i * kAccLine] = 0ull;
}
template <int VARIANT, int DIM, bool ARC, bool FROM_ACC>
__global__ __launch_bounds__(kBlock) void assign_fused_finalize_kernel(const float* __restrict__ b1, int k, const float* __restrict__ b2,
        int n, int edge_arg, const unsigned long long* __restrict__ col_part, int chunks, const unsigned long long* __restrict__ row_part,
        const long long* __restrict__ gt_keys, unsigned long long* __restrict__ row_acc, bool has_ignore, unsigned col_offset,
        float pos_thr, float neg_lo, float neg_hi, float min_pos, int low_quality, int assign_all, const int64_t* __restrict__ gt_labels,
        float* __restrict__ max_ov, int64_t* __restrict__ argmax_ov, float* __restrict__ gt_max, int64_t* __restrict__ gt_argmax,
        int64_t* __restrict__ gt_inds, int64_t* __restrict__ labels) {
    const Rule rule{pos_thr, neg_lo, neg_hi, min_pos, low_quality, assign_all};
    const int tile = blockIdx.x, tiles = gridDim.x;
    const int j = tile * kBlock + threadIdx.x;
    const Layout l = layout(k, n, tiles, chunks, false);
    float m;
    int64_t am;
    const int64_t a = fused_finalize_column<VARIANT, DIM, ARC, FROM_ACC>(b1, k, b2, n, edge_arg, col_part, chunks, row_part, gt_keys, row_acc,
                                                                         l.stride, has_ignore, col_offset, rule, gt_max, gt_argmax, tile, tiles, m, am);
    if (j < n) {
        max_ov[j] = m;
        if (argmax_ov) argmax_ov[j] = am;
        gt_inds[j] = a;
        if (labels) labels[j] = a > 0 ? gt_labels[a - 1] : -1;
    }
    // every read of the accumulators above has returned (its value was used)
    if (FROM_ACC && finalize_arrive(row_acc + l.counters, tile, tiles)) reset_image_state(row_acc, k, l);
}


// ---- anchor targets for a minibatch (sph2pob_anchor_targets_f32): the fused assigner with the image as a grid dimension and
// the target construction of mmdet's AnchorHead._get_targets_single (anchor_head.py:254-285, PseudoSampler) as the finalize
// pass's epilogue.  Two launches for B images; every image owns a slice of the workspace and of the state, laid out for k_max
// rows whatever its own count (Layout). ----
// an image's rows in chunks of equal size, at most rows_per_wg each
__device__ __forceinline__ int image_chunks(int k, int rows_per_wg) { return (k + rows_per_wg - 1) / rows_per_wg; }

// grid (tiles, chunks_max, B): per image the tail-first order of iou_pairwise_compact_kernel; workgroups past the image's own
// chunks (all of them for an image without GT) exit at once
template <int VARIANT, int DIM, bool ARC>
__global__ __launch_bounds__(kBlock, ARC ? 8 : 4) void anchor_targets_pairwise_kernel(const float* __restrict__ gt,
        const int64_t* __restrict__ gt_offsets, int64_t K, int k_max, const float* __restrict__ anchors, int n, int edge_arg,
        int rows_per_wg, unsigned long long* __restrict__ workspace, unsigned long long* __restrict__ state) {
    const int b = blockIdx.z;
    const TileId t = tail_first_tile();
    const ImageRows im = image_rows(gt_offsets, b, K, k_max);
    const int chunks = image_chunks(im.k, rows_per_wg);
    if (t.by >= chunks) return;
    const Layout l = layout(k_max, n, col_tiles(n), row_chunks(k_max, rows_per_wg), true);
    unsigned long long* col_part = workspace + b * l.ws_words;
    pairwise_compact_tile<VARIANT, DIM, ARC, 2>(gt + im.lo * DIM, im.k, anchors, n, nullptr, (int)MODE_IOU, edge_arg, (im.k + chunks - 1) / chunks,
                                                nullptr, col_part, col_part + l.row_part, 0u, state + b * l.state_words, t.bx, t.by, (int)l.tiles,
                                                l.stride);
}

// Phase 1 of the batched route for the variants without a closed form (sph2pob_anchor_targets_any_f32): the grid, the image
// slices, the chunk rule and the three outputs of anchor_targets_pairwise_kernel, with per_pair_iou on EVERY pair of the tile in
// place of cull / compact / finish.  One thread owns one anchor (a lane past n works on anchor n - 1 and contributes nothing)
// and walks the chunk's rows from LDS: the column's key is a running maximum in registers (equal values keep the first row);
// per row the wave reduces the value's ordered bits, a ballot names the first lane that holds the maximum and tells whether a
// second one does, and lane 0 takes the packed row key into the tile's LDS with one ds_max_rtn_u64 — an equal value already
// there is the same value at a column of another wave: the "second column" flag either way (conservative, as in
// pairwise_compact_tile).  Every tile has a live column, so every row of the chunk gets a key: no tile base is needed.
// A -0 would sort below +0 in the keys while torch.max treats them alike: zeros are taken as +0.
template <int VARIANT, int DIM>
__global__ __launch_bounds__(kBlock) void anchor_targets_pairwise_any_kernel(const float* __restrict__ gt,
        const int64_t* __restrict__ gt_offsets, int64_t K, int k_max, const float* __restrict__ anchors, int n, int edge, int rows_per_wg,
        unsigned long long* __restrict__ workspace, unsigned long long* __restrict__ state) {
    __shared__ float row_raw[kPwRows][5];
    __shared__ unsigned long long row_key[kPwRows];
    __shared__ int row_tie[kPwRows];
    const int b = blockIdx.z;
    const TileId t = tail_first_tile();
    const ImageRows im = image_rows(gt_offsets, b, K, k_max);
    const int chunks = image_chunks(im.k, rows_per_wg);
    if (t.by >= chunks) return;
    const Layout l = layout(k_max, n, col_tiles(n), row_chunks(k_max, rows_per_wg), true);
    unsigned long long* col_part = workspace + b * l.ws_words;
    unsigned long long* row_part = col_part + l.row_part;
    unsigned long long* row_acc = state + b * l.state_words;
    const float* gt_b = gt + im.lo * DIM;
    const int rpw = (im.k + chunks - 1) / chunks;
    const int r0 = t.by * rpw, rows = (im.k - r0 < rpw) ? im.k - r0 : rpw;
    const int lane = threadIdx.x & 63;
    if ((int)threadIdx.x < rows) {
        float g[5];
        load_box<DIM>(gt_b, r0 + threadIdx.x, g);
#pragma unroll
        for (int c = 0; c < 5; c++) row_raw[threadIdx.x][c] = g[c];
        row_key[threadIdx.x] = 0ull;
        row_tie[threadIdx.x] = 0;
    }
    const int jraw = t.bx * kBlock + threadIdx.x;
    const bool valid = jraw < n;
    float a[5];
    load_box<DIM>(anchors, valid ? jraw : n - 1, a);
    __syncthreads();
    unsigned long long ck = 0ull;
    for (int i = 0; i < rows; i++) {
        float g[5];
#pragma unroll
        for (int c = 0; c < 5; c++) g[c] = row_raw[i][c];
        float v = per_pair_iou<VARIANT, DIM>(g, a, edge);
        v = v == 0.0f ? 0.0f : v;
        const unsigned long long key = pack_max_key(v, r0 + i);
        ck = key > ck ? key : ck;
        const unsigned ob = valid ? ordered_bits(v) : 0u;
        const unsigned wm = wave_max_u32(ob);
        const unsigned long long eq = __builtin_amdgcn_ballot_w64(ob == wm);
        if (lane == 0 && wm != 0u) {   // wm == 0: a wave past n
            const unsigned col = (unsigned)(jraw + __builtin_ctzll(eq));
            const unsigned long long old = atomicMax(&row_key[i], pack_row_key_bits(wm, col));
            if (__popcll(eq) > 1 || (unsigned)(old >> 32) == wm) row_tie[i] = 1;
        }
    }
    __syncthreads();
    if (valid) col_part[(int64_t)t.by * n + jraw] = ck;
    if ((int)threadIdx.x < rows) {
        const unsigned long long best = row_key[threadIdx.x] | (unsigned long long)row_tie[threadIdx.x];
        row_part[(int64_t)(r0 + threadIdx.x) * l.tiles + t.bx] = best;
        // as in pairwise_compact_tile: only tiles that hold something above the rows' common floor (0 at column 0)
        if ((unsigned)(best >> 32) > 0x80000000u)
            __hip_atomic_fetch_max(row_acc + (r0 + threadIdx.x) * l.stride, best, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

struct TargetOut {
    int64_t* gt_inds; float* max_ov; int64_t* assigned_labels; int64_t* labels; float* label_weights; float* bbox_targets;
    float* bbox_weights; int64_t* num_pos; int64_t* num_neg; float* avg_factor;
};
// grid (tiles, B).  The targets of column j of image b from its assigned index: sph2pob_assign::target_row, stored here.
// Counts: one ballot per wave into LDS, one packed atomic per workgroup into the image's state line; the image's last
// workgroup writes num_pos / num_neg and adds max(num_pos, 1) to the batch's sum, the batch's last image writes avg_factor.
// Each of these atomics returns before the arrival that publishes it is issued (finalize_arrive's `extra`).
template <int VARIANT, int DIM, bool ARC, bool ENCODE>
__global__ __launch_bounds__(kBlock) void anchor_targets_finalize_kernel(const float* __restrict__ gt,
        const int64_t* __restrict__ gt_labels, const int64_t* __restrict__ gt_offsets, int64_t K, int k_max,
        const float* __restrict__ anchors, int n, int edge_arg, int rows_per_wg, unsigned long long* __restrict__ workspace,
        unsigned long long* __restrict__ state, float pos_thr, float neg_lo, float neg_hi, float min_pos, int low_quality, int assign_all,
        int64_t num_classes, float pos_weight, sph2pob_coder::Norm nm, TargetOut o) {
    __shared__ unsigned wg_count[2];
    const Rule rule{pos_thr, neg_lo, neg_hi, min_pos, low_quality, assign_all};
    const int tile = blockIdx.x, tiles = gridDim.x, b = blockIdx.y, images = gridDim.y;
    const ImageRows im = image_rows(gt_offsets, b, K, k_max);
    const Layout l = layout(k_max, n, tiles, row_chunks(k_max, rows_per_wg), true);
    const float* gt_b = gt + im.lo * DIM;
    unsigned long long* acc = state + b * l.state_words;
    if (threadIdx.x < 2) wg_count[threadIdx.x] = 0u;
    float m = 0.0f;
    int64_t am = 0, a = 0;   // an image without GT: every anchor is background (max_iou_assigner.py:148-165)
    if (im.k > 0) {
        const unsigned long long* col_part = workspace + b * l.ws_words;
        a = fused_finalize_column<VARIANT, DIM, ARC, true>(gt_b, im.k, anchors, n, edge_arg, col_part, image_chunks(im.k, rows_per_wg),
                                                           col_part + l.row_part, nullptr, acc, l.stride, false, 0u, rule, nullptr, nullptr, tile,
                                                           tiles, m, am);
    }
    const int j = tile * kBlock + threadIdx.x;
    const bool valid = j < n, pos = valid && a > 0, neg = valid && a == 0;
    if (valid) {
        const int64_t e = (int64_t)b * n + j;
        float g[5], p[5];
        if (pos) {
            load_box<DIM>(gt_b, a - 1, g);
            if constexpr (ENCODE) load_box<DIM>(anchors, j, p);
        }
        const sph2pob_assign::TargetRow r = sph2pob_assign::target_row<DIM, ENCODE>(a, p, g, gt_labels ? gt_labels + im.lo : nullptr, num_classes,
                                                                                    pos_weight, nm);
        o.gt_inds[e] = a;
        o.max_ov[e] = m;
        if (o.assigned_labels) o.assigned_labels[e] = pos ? r.label : -1;
        o.labels[e] = r.label;
        o.label_weights[e] = r.label_weight;
        const float w = r.box_weight;
        if constexpr (DIM == 4) {   // one 16-byte store per row
            reinterpret_cast<float4*>(o.bbox_targets)[e] = make_float4(r.t[0], r.t[1], r.t[2], r.t[3]);
            reinterpret_cast<float4*>(o.bbox_weights)[e] = make_float4(w, w, w, w);
        } else {
#pragma unroll
            for (int c = 0; c < DIM; c++) { o.bbox_targets[e * DIM + c] = r.t[c]; o.bbox_weights[e * DIM + c] = w; }
        }
    }
    __syncthreads();   // wg_count is zero
    const unsigned long long mp = __builtin_amdgcn_ballot_w64(pos), mn = __builtin_amdgcn_ballot_w64(neg);
    if ((threadIdx.x & 63) == 0) {
        if (mp) atomicAdd(&wg_count[0], (unsigned)__popcll(mp));
        if (mn) atomicAdd(&wg_count[1], (unsigned)__popcll(mn));
    }
    __syncthreads();
    unsigned long long* count = acc + l.count;
    unsigned dep = 0u;
    if (threadIdx.x == 0) {
        const unsigned long long prev = __hip_atomic_fetch_add(count, (unsigned long long)wg_count[0] | ((unsigned long long)wg_count[1] << 32),
                                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        asm volatile("" : "+v"(dep) : "v"(prev));   // dep stays 0, and is not known before the count's atomic has returned
    }
    if (finalize_arrive(acc + l.counters, tile, tiles, dep)) {   // the image's last workgroup: its state back to zero, its counts out
        reset_image_state(acc, im.k, l);
        if (threadIdx.x == 0) {
            const unsigned long long c = __hip_atomic_load(count, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(count, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned np = (unsigned)c;
            o.num_pos[b] = (int64_t)np;
            o.num_neg[b] = (int64_t)(unsigned)(c >> 32);
            unsigned long long* batch = state + images * l.state_words;
            const unsigned long long prev = __hip_atomic_fetch_add(batch + 1, (unsigned long long)(np > 0u ? np : 1u), __ATOMIC_RELAXED,
                                                                   __HIP_MEMORY_SCOPE_AGENT);
            unsigned d2 = 0u;
            asm volatile("" : "+v"(d2) : "v"(prev));
            const unsigned done = __hip_atomic_fetch_add((unsigned*)batch, 1u + d2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((int)done == images - 1) {
                *o.avg_factor = (float)__hip_atomic_load(batch + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(batch, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                __hip_atomic_store(batch + 1, 0ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
        }
    }
}


// rows per workgroup of iou_pairwise_compact_kernel: enough to amortise the per-column setup and fill the survivor stacks,
// few enough that the grid holds thousands of workgroups; with the tail-first dispatch order, 64 GT
// (profiles/r03y_ab_pairwise_rows.log): 98 208 anchors 18.5 us at 8 rows, 19.9 at 12, 20.2 at 16, 33.9 at 32; 392 832
// anchors 49.1 us at 8, 47.0 at 12, 42.6 at 16, 41.1 at 22, 42.0 at 32 => about 4 096 workgroups, at least 8 rows, chunks of
// equal size
static int64_t pairwise_rows_per_wg(int64_t m, int64_t n) {
    int64_t rpw = g_pw_rows > 0 ? g_pw_rows : (m * col_tiles(n)) / 4096;
    if (rpw < 8 && g_pw_rows <= 0) rpw = 8;
    if (rpw < 4) rpw = 4;
    if (rpw > kPwRows) rpw = kPwRows;
    if (rpw > m) rpw = m;
    if (g_pw_rows <= 0) rpw = (m + (m + rpw - 1) / rpw - 1) / ((m + rpw - 1) / rpw);   // 64 rows: 23 -> 3 chunks of 22 / 22 / 20
    return rpw;
}
// the batched form: rows per workgroup from the rows the whole batch can hold (an image has at most k_max, the batch K)
static int64_t batch_rows_per_wg(int64_t images, int64_t K, int64_t k_max, int64_t n) {
    const int64_t total = images * k_max < K ? images * k_max : K;
    int64_t rpw = pairwise_rows_per_wg(total, n);
    return rpw > k_max ? k_max : rpw;
}
// the single-image fused route's buffers for rpw = pairwise_rows_per_wg(k, n)
static Layout fused_layout(int64_t k, int64_t n, int64_t rpw) { return layout(k, n, col_tiles(n), row_chunks(k, rpw), false); }

// iou_pairwise_compact_kernel in its three forms: the matrix alone (`red` == nullptr: the pairwise entry), the reductions, or both
struct Reductions { const unsigned char* ignore; unsigned long long *col_part, *row_part; unsigned col_offset; unsigned long long* row_acc; };
template <int V, int D>
static void launch_compact(const float* b1, int64_t m, const float* b2, int64_t n, float* out, int mode, int edge, int64_t rpw,
                           const Reductions* red, hipStream_t s) {
    const dim3 grid((unsigned)col_tiles(n), (unsigned)row_chunks(m, rpw));
    const Reductions r = red ? *red : Reductions{};
    with_flag(edge == SPH2POB_EDGE_ARC, [&](auto arc) {
        auto go = [&](auto out_bits) {
            hipLaunchKernelGGL((iou_pairwise_compact_kernel<V, D, decltype(arc)::value, decltype(out_bits)::value>), grid, dim3(kBlock), 0, s, b1,
                               (int)m, b2, (int)n, out, mode, edge, (int)rpw, r.ignore, r.col_part, r.row_part, r.col_offset, r.row_acc);
        };
        if (!red) go(std::integral_constant<int, 1>{});
        else if (out) go(std::integral_constant<int, 3>{});
        else go(std::integral_constant<int, 2>{});
    });
}
// standard / efficient as they are, every other variant as 0: a launcher that does not serve the others (the entry points'
// checks refuse them) names its kernels with this and instantiates nothing for them
constexpr int closed_form(int v) { return v >= 2 ? 0 : v; }
struct PairwiseLaunch {
    const float* b1; int64_t m; const float* b2; int64_t n; float* out; int mode, edge, angle; hipStream_t s; bool fast = true;
    template <int V, int D> int run() {
        const bool closed = fast && V < 2 && angle == SPH2POB_ANGLE_EQUATOR;
        if (closed && n < ((int64_t)1 << 31) - kBlock && m <= (int64_t)65535 * 4 && !g_no_compact) {
            launch_compact<closed_form(V), D>(b1, m, b2, n, out, mode, edge, pairwise_rows_per_wg(m, n), nullptr, s);
            return launch_status();
        }
        // grid.y is limited to 65535 rows per launch: walk the rows in slabs
        const int64_t kMaxRows = 65535;
        for (int64_t r0 = 0; r0 < m; r0 += kMaxRows) {
            int64_t rows = m - r0 < kMaxRows ? m - r0 : kMaxRows;
            with_pair_sel<V>(fast, angle, [&](auto variant, auto fast_core) {
                hipLaunchKernelGGL((iou_pairwise_kernel<decltype(variant)::value, D, decltype(fast_core)::value>), dim3((unsigned)col_tiles(n), (unsigned)rows),
                                   dim3(kBlock), 0, s, b1 + r0 * D, rows, b2, n, out + r0 * n, mode, edge, angle);
            });
            int rc = launch_status();
            if (rc) return rc;
        }
        return SPH2POB_OK;
    }
};
// the fused assigner's two halves and the batched route: closed-form standard / efficient only (the kernels that carry the reductions)
struct AssignReduceLaunch {
    const float* b1; int64_t m; const float* b2; int64_t n; float* out; int edge; const unsigned char* ignore; unsigned col_offset;
    long long* gt_keys /* NULL: leave the keys in the accumulators */; void* workspace; void* state; hipStream_t s; bool fast = true;
    template <int V, int D> int run() {
        if (V >= 2 || !fast) return SPH2POB_ERR_OPTION;
        const int64_t rpw = pairwise_rows_per_wg(m, n);
        const Layout l = fused_layout(m, n, rpw);
        unsigned long long *ws = (unsigned long long*)workspace, *acc = (unsigned long long*)state;
        const Reductions red{ignore, ws, ws + l.row_part, col_offset, acc};
        launch_compact<closed_form(V), D>(b1, m, b2, n, out, (int)MODE_IOU, edge, rpw, &red, s);
        if (gt_keys)
            hipLaunchKernelGGL(assign_keys_from_acc_kernel, dim3(1), dim3(kBlock), 0, s, acc, (int)m, ignore != nullptr, col_offset, gt_keys);
        return launch_status();
    }
};
struct AssignFinalizeLaunch {
    const float* b1; int64_t m; const float* b2; int64_t n; int edge; unsigned col_offset; const long long* gt_keys /* NULL: the accumulators */;
    bool has_ignore; Rule rule; const int64_t* gt_labels; float* max_ov; int64_t* argmax_ov;
    float* gt_max; int64_t* gt_argmax; int64_t* gt_inds; int64_t* labels; void* workspace; void* state; hipStream_t s; bool fast = true;
    template <int V, int D> int run() {
        if (V >= 2 || !fast) return SPH2POB_ERR_OPTION;
        const Layout l = fused_layout(m, n, pairwise_rows_per_wg(m, n));
        const unsigned long long* ws = (const unsigned long long*)workspace;
        with_flag(edge == SPH2POB_EDGE_ARC, [&](auto arc) {
            with_flag(gt_keys == nullptr, [&](auto from_acc) {
                hipLaunchKernelGGL((assign_fused_finalize_kernel<closed_form(V), D, decltype(arc)::value, decltype(from_acc)::value>),
                                   dim3((unsigned)l.tiles), dim3(kBlock), 0, s, b1, (int)m, b2, (int)n, edge, ws, (int)l.chunks, ws + l.row_part, gt_keys,
                                   (unsigned long long*)state, has_ignore, col_offset, rule.pos_thr, rule.neg_lo, rule.neg_hi, rule.min_pos,
                                   rule.low_quality, rule.assign_all, gt_labels, max_ov, argmax_ov, gt_max, gt_argmax, gt_inds, labels);
            });
        });
        return launch_status();
    }
};
struct AnchorTargetsLaunch {
    const float* anchors; int64_t n; const float* gt; const int64_t* gt_labels; const int64_t* gt_offsets; int64_t images, K, k_max; int edge;
    Rule rule; int64_t num_classes; float pos_weight; bool encode; sph2pob_coder::Norm nm;
    TargetOut o; void* workspace; void* state; hipStream_t s; bool fast = true;
    template <int V, int D> int run() {
        if (V >= 2 || !fast) return SPH2POB_ERR_OPTION;
        const int64_t rpw = k_max > 0 ? batch_rows_per_wg(images, K, k_max, n) : 1;
        const Layout l = layout(k_max, n, col_tiles(n), row_chunks(k_max, rpw), true);
        unsigned long long *ws = (unsigned long long*)workspace, *st = (unsigned long long*)state;
        with_flag(edge == SPH2POB_EDGE_ARC, [&](auto arc) {
            if (k_max > 0)
                hipLaunchKernelGGL((anchor_targets_pairwise_kernel<closed_form(V), D, decltype(arc)::value>),
                                   dim3((unsigned)l.tiles, (unsigned)l.chunks, (unsigned)images), dim3(kBlock), 0, s, gt, gt_offsets, K, (int)k_max,
                                   anchors, (int)n, edge, (int)rpw, ws, st);
            with_flag(encode, [&](auto enc) {
                hipLaunchKernelGGL((anchor_targets_finalize_kernel<closed_form(V), D, decltype(arc)::value, decltype(enc)::value>),
                                   dim3((unsigned)l.tiles, (unsigned)images), dim3(kBlock), 0, s, gt, gt_labels, gt_offsets, K, (int)k_max, anchors,
                                   (int)n, edge, (int)rpw, ws, st, rule.pos_thr, rule.neg_lo, rule.neg_hi, rule.min_pos, rule.low_quality,
                                   rule.assign_all, num_classes, pos_weight, nm, o);
            });
        });
        return launch_status();
    }
};
// the same two launches, buffers and sizes for the variants that run their per-pair function on every pair (legacy, Sph-IoU,
// FoV-IoU, unbiased, naive); `edge` carries SPH2POB_FLAG_NAIVE_TAN
struct AnchorTargetsAnyLaunch : AnchorTargetsLaunch {
    template <int V, int D> int run() {
        if constexpr (V < 2) return SPH2POB_ERR_OPTION;
        else {
            if (!fast) return SPH2POB_ERR_OPTION;
            const int64_t rpw = k_max > 0 ? batch_rows_per_wg(images, K, k_max, n) : 1;
            const Layout l = layout(k_max, n, col_tiles(n), row_chunks(k_max, rpw), true);
            unsigned long long *ws = (unsigned long long*)workspace, *st = (unsigned long long*)state;
            if (k_max > 0)
                hipLaunchKernelGGL((anchor_targets_pairwise_any_kernel<V, D>), dim3((unsigned)l.tiles, (unsigned)l.chunks, (unsigned)images),
                                   dim3(kBlock), 0, s, gt, gt_offsets, K, (int)k_max, anchors, (int)n, edge, (int)rpw, ws, st);
            with_flag(encode, [&](auto enc) {
                hipLaunchKernelGGL((anchor_targets_finalize_kernel<V, D, false, decltype(enc)::value>), dim3((unsigned)l.tiles, (unsigned)images),
                                   dim3(kBlock), 0, s, gt, gt_labels, gt_offsets, K, (int)k_max, anchors, (int)n, edge, (int)rpw, ws, st,
                                   rule.pos_thr, rule.neg_lo, rule.neg_hi, rule.min_pos, rule.low_quality, rule.assign_all, num_classes,
                                   pos_weight, nm, o);
            });
            return launch_status();
        }
    }
};

}  // namespace

extern "C" {


int sph2pob_iou_pairwise_f32(const float* b1, int64_t m, const float* b2, int64_t n, float* out, int box_dim,
                             int variant, int mode, int edge, int angle, void* stream) {
    const int rc = check_iou(box_dim, variant, mode, edge, angle, m, n, {b1, b2, out});
    if (rc || m == 0 || n == 0) return rc;
    return dispatch(variant, box_dim, PairwiseLaunch{b1, m, b2, n, out, mode, naive_edge(variant, edge), angle, (hipStream_t)stream});
}


// the matrix epilogue's workspace: one partial per row and wave of assign_cols_kernel
int64_t sph2pob_assign_workspace_bytes(int64_t k, int64_t n) { return k * (col_tiles(n) * (kBlock / 64)) * 8; }

int sph2pob_assign_f32(const float* overlaps, int64_t k, int64_t n, float pos_iou_thr, float neg_iou_lo,
                       float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                       const int64_t* gt_labels, float* max_overlaps, int64_t* argmax_overlaps, float* gt_max_overlaps,
                       int64_t* gt_argmax_overlaps, int64_t* assigned_gt_inds, int64_t* assigned_labels, void* workspace,
                       void* stream) {
    if (k <= 0 || n <= 0 || k > 0x7fffffff || n > kMaxElems || n > (int64_t)0xfffffffe) return SPH2POB_ERR_SIZE;
    if (!overlaps || !max_overlaps || !argmax_overlaps || !gt_max_overlaps || !gt_argmax_overlaps || !assigned_gt_inds ||
        !workspace || (assigned_labels && !gt_labels))
        return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const unsigned blocks = (unsigned)col_tiles(n);
    const int nparts = (int)(blocks * (kBlock / 64));
    unsigned long long* partial = (unsigned long long*)workspace;
    hipLaunchKernelGGL(assign_cols_kernel, dim3(blocks), dim3(kBlock), 0, s, overlaps, (int)k, n, max_overlaps,
                       argmax_overlaps, partial, nparts);
    hipLaunchKernelGGL(assign_rows_kernel, dim3((unsigned)k), dim3(kBlock), 0, s, partial, nparts, gt_max_overlaps,
                       gt_argmax_overlaps);
    hipLaunchKernelGGL(assign_finalize_kernel, dim3(blocks), dim3(kBlock), 0, s, overlaps, (int)k, n, max_overlaps,
                       argmax_overlaps, gt_max_overlaps, gt_argmax_overlaps, pos_iou_thr, neg_iou_lo, neg_iou_hi,
                       min_pos_iou, match_low_quality, gt_max_assign_all, gt_labels, assigned_gt_inds, assigned_labels);
    return launch_status();
}

int64_t sph2pob_iou_assign_workspace_bytes(int64_t k, int64_t n) {
    return k > 0 && n > 0 ? fused_layout(k, n, pairwise_rows_per_wg(k, n)).ws_words * 8 : 0;
}
int64_t sph2pob_iou_assign_state_bytes(int64_t k, int64_t n) {
    return k > 0 && n > 0 ? layout(k, n, col_tiles(n), 0, false).state_words * 8 : 0;
}

int sph2pob_iou_assign_reduce_f32(const float* gt, int64_t k, const float* boxes, int64_t n, int box_dim, int variant, int edge,
                                  const unsigned char* ignore, int64_t col_offset, float* overlaps, int64_t* gt_keys,
                                  void* workspace, void* state, void* stream) {
    int rc = sph2pob_assign::assign_fused_check(check_common(box_dim, variant, edge, 0), k, n, variant, col_offset);
    if (rc) return rc;
    if (!gt || !boxes || !gt_keys || !workspace || !state) return SPH2POB_ERR_NULL;
    return dispatch(variant, box_dim, AssignReduceLaunch{gt, k, boxes, n, overlaps, edge, ignore, (unsigned)col_offset,
                                                         (long long*)gt_keys, workspace, state, (hipStream_t)stream});
}

int sph2pob_iou_assign_finalize_f32(const float* gt, int64_t k, const float* boxes, int64_t n, int box_dim, int variant, int edge,
                                    int64_t col_offset, const int64_t* gt_keys, float pos_iou_thr, float neg_iou_lo,
                                    float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                                    const int64_t* gt_labels, float* max_overlaps, int64_t* argmax_overlaps,
                                    float* gt_max_overlaps, int64_t* gt_argmax_overlaps, int64_t* assigned_gt_inds,
                                    int64_t* assigned_labels, void* workspace, void* stream) {
    int rc = sph2pob_assign::assign_fused_check(check_common(box_dim, variant, edge, 0), k, n, variant, col_offset);
    if (rc) return rc;
    if (!gt || !boxes || !gt_keys || !workspace || !max_overlaps || !assigned_gt_inds || (assigned_labels && !gt_labels))
        return SPH2POB_ERR_NULL;
    return dispatch(variant, box_dim,
                    AssignFinalizeLaunch{gt, k, boxes, n, edge, (unsigned)col_offset, (const long long*)gt_keys, false,
                                         Rule{pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all}, gt_labels,
                                         max_overlaps, argmax_overlaps, gt_max_overlaps, gt_argmax_overlaps, assigned_gt_inds,
                                         assigned_labels, workspace, nullptr, (hipStream_t)stream});
}

int sph2pob_iou_assign_f32(const float* gt, int64_t k, const float* boxes, int64_t n, int box_dim, int variant, int edge,
                           const unsigned char* ignore, float* overlaps, float pos_iou_thr, float neg_iou_lo, float neg_iou_hi,
                           float min_pos_iou, int match_low_quality, int gt_max_assign_all, const int64_t* gt_labels,
                           float* max_overlaps, int64_t* argmax_overlaps, float* gt_max_overlaps, int64_t* gt_argmax_overlaps,
                           int64_t* assigned_gt_inds, int64_t* assigned_labels, void* workspace, void* state, void* stream) {
    int rc = sph2pob_assign::assign_fused_check(check_common(box_dim, variant, edge, 0), k, n, variant, 0);
    if (rc) return rc;
    if (!gt || !boxes || !workspace || !state || !max_overlaps || !assigned_gt_inds || (assigned_labels && !gt_labels)) return SPH2POB_ERR_NULL;
    // two launches: the per-GT keys stay in the workspace's accumulators, the finalize pass reads and clears them
    rc = dispatch(variant, box_dim, AssignReduceLaunch{gt, k, boxes, n, overlaps, edge, ignore, 0u, nullptr, workspace, state, (hipStream_t)stream});
    if (rc) return rc;
    return dispatch(variant, box_dim,
                    AssignFinalizeLaunch{gt, k, boxes, n, edge, 0u, nullptr, ignore != nullptr,
                                         Rule{pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all}, gt_labels,
                                         max_overlaps, argmax_overlaps, gt_max_overlaps, gt_argmax_overlaps, assigned_gt_inds, assigned_labels,
                                         workspace, state, (hipStream_t)stream});
}

int64_t sph2pob_anchor_targets_workspace_bytes(int64_t num_images, int64_t num_gt, int64_t k_max, int64_t n) {
    if (num_images <= 0 || num_gt <= 0 || k_max <= 0 || n <= 0) return 0;
    return num_images * layout(k_max, n, col_tiles(n), row_chunks(k_max, batch_rows_per_wg(num_images, num_gt, k_max, n)), true).ws_words * 8;
}
int64_t sph2pob_anchor_targets_state_bytes(int64_t num_images, int64_t k_max, int64_t n) {
    if (num_images <= 0 || k_max < 0 || n <= 0) return 0;
    return (num_images * layout(k_max, n, col_tiles(n), 0, true).state_words + kAccLine) * 8;   // + the batch's line behind the last image
}

int sph2pob_anchor_targets_f32(const float* anchors, int64_t n, const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets,
                               int64_t num_images, int64_t num_gt, int64_t k_max, int box_dim, int variant, int edge, float pos_iou_thr,
                               float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                               int64_t num_classes, float pos_weight, int encode, const float* means_host, const float* stds_host,
                               int64_t* assigned_gt_inds, float* max_overlaps, int64_t* assigned_labels, int64_t* labels,
                               float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* num_pos, int64_t* num_neg,
                               float* avg_factor, void* workspace, void* state, void* stream) {
    int rc = sph2pob_assign::anchor_targets_check(sph2pob_assign::closed_form_only(check_common(box_dim, variant, edge, 0), variant), anchors, n, gt,
                                                  gt_labels, gt_offsets, num_images, num_gt, k_max, assigned_gt_inds, max_overlaps, assigned_labels,
                                                  labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, avg_factor, true, workspace, state);
    if (rc) return rc;
    const TargetOut o{assigned_gt_inds, max_overlaps, assigned_labels, labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, avg_factor};
    return dispatch(variant, box_dim,
                    AnchorTargetsLaunch{anchors, n, gt, gt_labels, gt_offsets, num_images, num_gt, k_max, edge,
                                        Rule{pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all}, num_classes,
                                        pos_weight, encode != 0, sph2pob_coder::make_norm(means_host, stds_host, box_dim), o, workspace, state,
                                        (hipStream_t)stream});
}

int sph2pob_anchor_targets_any_f32(const float* anchors, int64_t n, const float* gt, const int64_t* gt_labels, const int64_t* gt_offsets,
                                   int64_t num_images, int64_t num_gt, int64_t k_max, int box_dim, int variant, int edge, float pos_iou_thr,
                                   float neg_iou_lo, float neg_iou_hi, float min_pos_iou, int match_low_quality, int gt_max_assign_all,
                                   int64_t num_classes, float pos_weight, int encode, const float* means_host, const float* stds_host,
                                   int64_t* assigned_gt_inds, float* max_overlaps, int64_t* assigned_labels, int64_t* labels,
                                   float* label_weights, float* bbox_targets, float* bbox_weights, int64_t* num_pos, int64_t* num_neg,
                                   float* avg_factor, void* workspace, void* state, void* stream) {
    int rc = sph2pob_assign::anchor_targets_check(sph2pob_assign::per_pair_only(check_common(box_dim, variant, edge, 0), variant), anchors, n, gt,
                                                  gt_labels, gt_offsets, num_images, num_gt, k_max, assigned_gt_inds, max_overlaps, assigned_labels,
                                                  labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, avg_factor, true, workspace, state);
    if (rc) return rc;
    if (variant & SPH2POB_FLAG_NAIVE_TAN) edge = SPH2POB_EDGE_TANGENT;   // as the pairwise entry hands it to naive_iou
    const TargetOut o{assigned_gt_inds, max_overlaps, assigned_labels, labels, label_weights, bbox_targets, bbox_weights, num_pos, num_neg, avg_factor};
    return dispatch(variant, box_dim,
                    AnchorTargetsAnyLaunch{{anchors, n, gt, gt_labels, gt_offsets, num_images, num_gt, k_max, edge,
                                            Rule{pos_iou_thr, neg_iou_lo, neg_iou_hi, min_pos_iou, match_low_quality, gt_max_assign_all}, num_classes,
                                            pos_weight, encode != 0, sph2pob_coder::make_norm(means_host, stds_host, box_dim), o, workspace, state,
                                            (hipStream_t)stream}});
}


}  // extern "C"
