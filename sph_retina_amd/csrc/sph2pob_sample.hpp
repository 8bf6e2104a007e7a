// Random sampling of anchor targets (mmdet's RandomSampler as the reference's SphRandomSampler calls it,
// sphdet/bbox/sampler/sph_random_sampler.py:34-46, followed by the target lines of AnchorHead._get_targets_single with a real
// sampler, anchor_head.py:254-299): the rank of a row, the sample sizes, the argument checks and the workspace (the selection rule:
// sph2pob_select.hpp), shared by the kernels (sph2pob_sample.hip) and their CPU twin (sph2pob_host.hip) so that a CPU tensor gets the sample a device
// tensor gets, bit for bit (everything here is integer arithmetic).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

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
