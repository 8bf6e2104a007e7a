// Random sampling of anchor targets (mmdet's RandomSampler as the reference's SphRandomSampler calls it,
// sphdet/bbox/sampler/sph_random_sampler.py:34-46, followed by the target lines of AnchorHead._get_targets_single with a real
// sampler, anchor_head.py:254-299): the rank of a row, the sample sizes, the draw, the select of one (image, side) — the device's
// (select_side: the body of sample_select_kernel and of rcnn_select_kernel) and the host's (host_select: both CPU twins) —, the
// argument checks and the workspace (the selection rule: sph2pob_select.hpp), shared by the kernels (sph2pob_sample.hip,
// sph2pob_rcnn_targets.hip) and their CPU twins (sph2pob_host.hip) so that a CPU tensor gets the sample a device tensor gets, bit
// for bit (everything here is integer arithmetic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <vector>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_head_loss.hpp"
#include "sph2pob_select.hpp"

namespace sph2pob_sample {

using sph2pob_head::aligned_to;
using sph2pob_head::kBlock;

constexpr int kSelectBlock = 1024;   // threads of the one workgroup that selects for an (image, side)
constexpr int64_t kMaxImages = 65535;

// ---- rank(b, i): word 0 of Philox4x32-10 (Salmon et al., SC'11) with key (seed low, seed high) and counter (i, b, 0, 0) ----------
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
SPHF_DEV void philox4x32_10(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; r++) {
        const uint64_t p0 = (uint64_t)kPhiloxM0 * c[0], p1 = (uint64_t)kPhiloxM1 * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += kPhiloxW0; k1 += kPhiloxW1;
    }
}
SPHF_DEV uint32_t row_rank(uint64_t seed, uint32_t image, uint32_t row) {
    uint32_t c[4] = {row, image, 0u, 0u};
    philox4x32_10(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    return c[0];
}

// ---- classes and sizes ----------------------------------------------------------------------------------------------------------
// the side of a row from its assigned_gt_inds: 0 positive, 1 negative, 2 ignored (takes no part, left as it is)
enum { POS = 0, NEG = 1, IGNORED = 2 };
SPHF_DEV int side_of(int64_t gt_ind) { return gt_ind > 0 ? POS : gt_ind == 0 ? NEG : IGNORED; }

// k_pos = min(P, num_expected_pos); k_neg = min(N, num - k_pos), and with neg_pos_ub >= 0 at most (int64)(neg_pos_ub max(1, k_pos))
SPHF_DEV void sample_sizes(int64_t P, int64_t N, int64_t num_expected_pos, int64_t num, double neg_pos_ub, int64_t* k_pos, int64_t* k_neg) {
    const int64_t kp = P < num_expected_pos ? P : num_expected_pos;
    int64_t kn = num - kp;
    if (neg_pos_ub >= 0.0) {
        const double cap = neg_pos_ub * (double)(kp > 1 ? kp : 1);
        if (cap < (double)kn) kn = (int64_t)cap;   // (a product that exceeds kn, an infinite one included, caps nothing)
    }
    *k_pos = kp;
    *k_neg = N < kn ? N : kn;
}

// What the select pass leaves for one (image, side): the cut (sph2pob_select.hpp, ascending) — the k-th smallest rank of the side's
// rows and the row index below which rows with exactly that rank are taken — and k.  Nothing taken: key 0, upto 0
struct Pick { sph2pob_select::Cut cut; int64_t k; };
SPHF_DEV bool sampled(uint32_t rank, int64_t i, const Pick& p) { return sph2pob_select::taken<false>(rank, i, p.cut); }

// ---- the draw and the select of one (image, side), for every entry that samples (the anchors' sampler and the R-CNN stage) ------
struct Draw {
    int64_t num_expected_pos, num;
    double neg_pos_ub;
    int64_t seed;
    const int64_t* seed_dev;     // wins over `seed` when non-NULL
    const uint32_t* ranks;       // the caller's ranks of every row of every image instead of the generator, or NULL
};
SPHF_DEV uint64_t seed_of(int64_t seed, const int64_t* seed_dev) { return (uint64_t)(seed_dev ? seed_dev[0] : seed); }

// The host's select of image b, for the CPU twins: at(i) is the assigned index of row i of the image's n rows, `ranks_row` the
// caller's ranks of these rows (or NULL: the generator on `seed`, seed_of's answer).  Fills rank[i] for the rows that take part and
// returns the picks of the two sides (the cut by sph2pob_select.hpp's host_cut).  `rank` (>= n words) and `scratch` are the caller's.
template <class At>
inline std::array<Pick, 2> host_select(At&& at, int64_t n, int64_t b, const uint32_t* ranks_row, uint64_t seed, int64_t num_expected_pos,
                                       int64_t num, double neg_pos_ub, std::vector<uint32_t>& rank, std::vector<uint32_t>& scratch) {
    int64_t count[2] = {0, 0}, k[2];
    for (int64_t i = 0; i < n; i++) {
        const int c = side_of(at(i));
        if (c == IGNORED) continue;
        count[c]++;
        rank[(size_t)i] = ranks_row ? ranks_row[i] : row_rank(seed, (uint32_t)b, (uint32_t)i);
    }
    sample_sizes(count[POS], count[NEG], num_expected_pos, num, neg_pos_ub, &k[POS], &k[NEG]);
    std::array<Pick, 2> pick;
    for (int side = 0; side < 2; side++) {
        pick[side] = Pick{{0u, 0}, k[side]};
        sph2pob_select::host_cut<false>(n, k[side], [&](int64_t i, uint32_t* key) { *key = rank[(size_t)i]; return side_of(at(i)) == side; }, scratch,
                                        &pick[side].cut);
    }
    return pick;
}

#if defined(__HIPCC__)
// The device's select: the body of a kernel of BLOCK threads on grid (images, 2), one workgroup per (image, side) = (blockIdx.x,
// blockIdx.y).  `gb`: the assigned indices of the image's n rows; `rank_in`: the caller's ranks of these rows, or NULL; `kb`: the
// image's rank words.  The first pass counts P_b and N_b (both workgroups count both: k_neg needs k_pos, and they do not
// communicate) and writes the rank of every row of the workgroup's side into kb; then the k-th smallest rank by a four-digit radix
// select (LDS histogram, integer atomics) and, only when the rows tied at that rank are not all taken, one in-order walk for the row
// index up to which they are (digit decision and tie scan: sph2pob_select.hpp, ascending).  Thread 0 writes picks[2 blockIdx.x + blockIdx.y].
// Row i belongs to thread i % BLOCK in every pass, so a thread reads back the rank words it wrote itself; AHEAD: the rows a thread
// loads before it works on them.
template <int BLOCK, int AHEAD>
__device__ __forceinline__ void select_side(const int64_t* __restrict__ gb, int n, const uint32_t* __restrict__ rank_in, uint32_t* __restrict__ kb, const Draw& D,
                                            Pick* __restrict__ picks) {
    constexpr int kWaves = BLOCK / 64;
    __shared__ unsigned hist[256];
    __shared__ unsigned s_count[2], s_prefix, s_rem, s_ties, s_wave[kWaves];
    __shared__ int s_upto;
    const int b = blockIdx.x, side = blockIdx.y, tid = threadIdx.x;
    if (tid == 0) { s_count[0] = 0u; s_count[1] = 0u; s_prefix = 0u; s_rem = 0u; s_ties = 0u; s_upto = 0; }
    const uint64_t seed = seed_of(D.seed, D.seed_dev);
    int64_t k = 0;

    // radix select, most significant digit first: after digit d the top 8 (d + 1) bits of the k-th smallest rank are known
    for (int d = 0; d < 4; d++) {
        const int shift = 24 - 8 * d;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = s_prefix, rem_in = s_rem;
        if (d == 0) {
            unsigned np = 0u, nn = 0u;
            for (int64_t i0 = tid; i0 < n; i0 += AHEAD * BLOCK) {   // AHEAD independent loads in flight, then the arithmetic
                int64_t g[AHEAD];
                uint32_t r[AHEAD];
#pragma unroll
                for (int u = 0; u < AHEAD; u++) {
                    const int64_t i = i0 + (int64_t)u * BLOCK;
                    g[u] = i < n ? gb[i] : -1;   // past the end: an ignored row
                    r[u] = rank_in && i < n ? rank_in[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < AHEAD; u++) {
                    const int64_t i = i0 + (int64_t)u * BLOCK;
                    const int c = side_of(g[u]);
                    np += c == POS; nn += c == NEG;
                    if (c == side) {
                        if (!rank_in) r[u] = row_rank(seed, (uint32_t)b, (uint32_t)i);
                        kb[i] = r[u];
                        atomicAdd(&hist[r[u] >> 24], 1u);
                    }
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) { np += __shfl_down(np, o, 64); nn += __shfl_down(nn, o, 64); }
            if ((tid & 63) == 0) { atomicAdd(&s_count[POS], np); atomicAdd(&s_count[NEG], nn); }
        } else if (rem_in > 0u) {   // workgroup-uniform
            const unsigned known = 0xffffffffu << (shift + 8);   // the digits already fixed
            for (int64_t i0 = tid; i0 < n; i0 += AHEAD * BLOCK) {
                int64_t g[AHEAD];
                uint32_t r[AHEAD];
#pragma unroll
                for (int u = 0; u < AHEAD; u++) {   // both loads of every row at once: the word of a row of the other side is not used
                    const int64_t i = i0 + (int64_t)u * BLOCK;
                    g[u] = i < n ? gb[i] : -1;
                    r[u] = i < n ? kb[i] : 0u;
                }
#pragma unroll
                for (int u = 0; u < AHEAD; u++) {
                    if (side_of(g[u]) == side && ((r[u] ^ prefix) & known) == 0u) atomicAdd(&hist[(r[u] >> shift) & 255u], 1u);
                }
            }
        }
        __syncthreads();
        if (d == 0) {
            int64_t kp, kn;
            sample_sizes((int64_t)s_count[POS], (int64_t)s_count[NEG], D.num_expected_pos, D.num, D.neg_pos_ub, &kp, &kn);
            k = side == POS ? kp : kn;   // <= the side's rows < 2^31
        }
        // the digit: the one bin that holds the rem-th smallest rank
        sph2pob_select::digit_decision<false>(hist, s_wave, &s_prefix, &s_rem, &s_ties, prefix, shift,
                                              [&](unsigned) { return d == 0 ? (unsigned)k : rem_in; });
    }
    const unsigned take = s_rem;          // rows tied at the k-th rank that are taken (>= 1 when anything is)
    const unsigned cut = s_prefix;
    const bool walk = take > 0u && take < s_ties;   // workgroup-uniform; otherwise every tied row is taken
    __syncthreads();

    // in-order walk: the index of the take-th row tied at the cut
    if (walk) {
        unsigned running = 0u;
        for (int64_t i0 = 0; i0 < n; i0 += BLOCK) {   // whole workgroups: barriers inside
            const int64_t i = i0 + tid;
            const bool tie = i < n && side_of(gb[i]) == side && kb[i] == cut;
            const unsigned long long m = __ballot(tie);
            const unsigned in_wave = (unsigned)__popcll(m & ((1ull << (tid & 63)) - 1ull));
            const unsigned before = sph2pob_select::tie_scan<kWaves>(in_wave, (unsigned)__popcll(m), s_wave, running);
            if (tie && before + 1u == take) s_upto = (int)(i + 1);   // one thread of one iteration
            __syncthreads();
            if (running >= take) break;   // workgroup-uniform
        }
    }
    if (tid == 0) {
        Pick p;
        p.cut.key = take > 0u ? cut : 0u;
        p.cut.upto = take > 0u ? (walk ? s_upto : n) : 0;
        p.k = k;
        picks[2 * b + side] = p;
    }
}
#endif

// ---- arguments and workspace ----------------------------------------------------------------------------------------------------
// box_dim -> DIM; a NaN neg_pos_ub -> OPTION; B outside [1, 65 535], n outside [1, 2^31), num < 1, num_expected_pos outside
// [0, num] -> SIZE
inline int check_shape(int64_t B, int64_t n, int box_dim, int64_t num_expected_pos, int64_t num, double neg_pos_ub) {
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (neg_pos_ub != neg_pos_ub) return SPH2POB_ERR_OPTION;
    if (B < 1 || B > kMaxImages || n < 1 || n >= ((int64_t)1 << 31) || num < 1 || num_expected_pos < 0 || num_expected_pos > num) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}

// The workspace: 2 B picks, then B n_pad rank words (n_pad = n rounded up to 4: every image's words start 16-byte aligned); a row's
// word is written by the select workgroup of the row's side and read by the apply pass
struct Workspace { Pick* picks; uint32_t* keys; int64_t n_pad; };
inline int64_t padded(int64_t n) { return (n + 3) / 4 * 4; }
inline int64_t workspace_bytes(int64_t B, int64_t n) {
    if (B < 1 || B > kMaxImages || n < 1 || n >= ((int64_t)1 << 31)) return 0;
    return 16 + (int64_t)sizeof(Pick) * 2 * B + 4 * B * padded(n);
}
inline Workspace carve(void* workspace, int64_t B, int64_t n) {
    uintptr_t p = (reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15;
    Workspace w;
    w.picks = reinterpret_cast<Pick*>(p);
    w.keys = reinterpret_cast<uint32_t*>(p + sizeof(Pick) * 2 * (uintptr_t)B);
    w.n_pad = padded(n);
    return w;
}

}  // namespace sph2pob_sample
