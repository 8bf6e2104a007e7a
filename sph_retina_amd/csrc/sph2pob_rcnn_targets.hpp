// R-CNN stage targets on per-image proposals (sph2pob_rcnn_targets_f32): per image MaxIoUAssigner.assign(proposals_b, gt_b), the
// reference's SphRandomSampler.sample(..., add_gt_as_proposals) (sphdet/bbox/sampler/sph_random_sampler.py:24-52), bbox2roi and
// SphShared2FCBBoxHead._get_target_single (sphdet/models/heads/sph_rcnn_head.py:30-66).  Shared by the kernels
// (sph2pob_rcnn_targets.hip) and their CPU twin (sph2pob_host.hip): the per-pair function of a variant, the image's proposals, the
// candidate list, the table row of one sampled candidate, the argument checks and the workspace — so that a CPU tensor gets the
// table a device tensor gets.  The assignment rule, the image's GT rows and the packed keys are sph2pob_assign.hpp's; the
// generator, the sizes, the draw and the select of a side are sph2pob_sample.hpp's, the cut sph2pob_select.hpp's.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_assign.hpp"
#include "sph2pob_iou_entry.hpp"
#include "sph2pob_sample.hpp"

namespace sph2pob_rcnn {

constexpr int kTile = sph2pob_assign::kTile;   // proposals (columns) of one workgroup of the pairwise and the candidate pass
// GT rows of one workgroup of the pairwise pass: the pass is as long as its longest workgroup, a serial chain of rows whose finishing
// pass diverges within the wave (B = 8, M = 1 000: 50.0 us at 32 rows, 27.8 at 16, 18.1 at 8: profiles/rcnn_targets_rows_ab.jsonl)
constexpr int kRows = 8;
constexpr int kCompactBlock = 1024;            // threads of the one workgroup that selects for an (image, side) / compacts an image
constexpr int64_t kMaxNum = 65535;             // the compaction scan carries both sides' running counts in the halves of one word
constexpr int64_t kMaxGt = (int64_t)65535 * 4;

// the IoU of (GT row, proposal): the function sph2pob_iou_pairwise_f32 runs for the variant with mode IOU and angle EQUATOR in
// the default arithmetic (`edge` carries SPH2POB_FLAG_NAIVE_TAN as EDGE_TANGENT); a -0 is taken as +0, as torch.max treats it
template <int VARIANT, int DIM>
SPH_DEV float pair_iou_of(const float (&g)[5], const float (&a)[5], int edge) {
    using namespace sph2pob;
    const float v = pair_iou_sel<VARIANT, DIM, pair_sel_fast(VARIANT, true, ANGLE_EQUATOR)>(g, a, (int)MODE_IOU, edge, (int)ANGLE_EQUATOR);
    return v == 0.0f ? 0.0f : v;
}

// rows of image b in the concatenated GT: sph2pob_assign.hpp's rule; and its proposals: the count clamped to [0, M] (no counts: M)
using sph2pob_assign::image_rows;
using sph2pob_assign::ImageRows;
SPHF_DEV int64_t image_proposals(const int64_t* num_proposals, int64_t b, int64_t M) {
    if (!num_proposals) return M;
    const int64_t n = num_proposals[b];
    return n < 0 ? 0 : (n > M ? M : n);
}
// the candidates of an image (sph_random_sampler.py:25-32): with add_gt and k > 0 its k GT rows, then its n proposals
SPHF_DEV int64_t gt_candidates(int add_gt, int64_t k) { return add_gt ? k : 0; }

// a box of DIM floats at `p` (any stride: the caller points at the row) as the five the per-pair functions take
template <int DIM>
SPHF_DEV void load_row(const float* p, float (&b)[5]) {
#pragma unroll
    for (int c = 0; c < 5; c++) b[c] = c < DIM ? p[c < DIM ? c : 0] : 0.0f;
}

// ---- the table (include/sph2pob_hip.h) ------------------------------------------------------------------------------------------
struct Table {
    float* rois; int64_t* labels; float* label_weights; float* bbox_targets; float* bbox_weights; int64_t* pos_assigned_gt_inds;
    int64_t* sample_inds; unsigned char* is_gt; int64_t* num_pos; int64_t* num_neg; float* avg_factor; float* num_samples;
};
// row r (global) of the table for sampled candidate c of image b with assigned index a (> 0 positive, 0 negative); `box`: the
// candidate's own DIM floats, `gt_b` / `labels_b`: the image's GT rows / labels (or null)
template <int DIM, bool ENCODE>
SPHF_DEV void write_sampled(const Table& T, int64_t r, int64_t b, int64_t c, int64_t a, bool from_gt, const float* box, const float* gt_b,
                            const int64_t* labels_b, int64_t num_classes, float pos_weight, const sph2pob_coder::Norm& nm) {
    float p[5], g[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    load_row<DIM>(box, p);
    if (a > 0) load_row<DIM>(gt_b + (a - 1) * DIM, g);
    const sph2pob_assign::TargetRow t = sph2pob_assign::target_row<DIM, ENCODE>(a, p, g, labels_b, num_classes, pos_weight, nm);
    T.rois[r * (DIM + 1)] = (float)b;
#pragma unroll
    for (int d = 0; d < DIM; d++) {
        T.rois[r * (DIM + 1) + 1 + d] = p[d];
        T.bbox_targets[r * DIM + d] = t.t[d];
        T.bbox_weights[r * DIM + d] = t.box_weight;
    }
    T.labels[r] = t.label;
    T.label_weights[r] = t.label_weight;
    T.pos_assigned_gt_inds[r] = a > 0 ? a - 1 : -1;
    T.sample_inds[r] = c;
    T.is_gt[r] = (a > 0 && from_gt) ? (unsigned char)1 : (unsigned char)0;
}
// a padding row: a valid 1 x 1 degree box on the equator, the background label, every weight 0
template <int DIM>
SPHF_DEV void write_padding(const Table& T, int64_t r, int64_t b, int64_t num_classes) {
    const float pad[5] = {180.0f, 90.0f, 1.0f, 1.0f, 0.0f};
    T.rois[r * (DIM + 1)] = (float)b;
#pragma unroll
    for (int d = 0; d < DIM; d++) {
        T.rois[r * (DIM + 1) + 1 + d] = pad[d];
        T.bbox_targets[r * DIM + d] = 0.0f;
        T.bbox_weights[r * DIM + d] = 0.0f;
    }
    T.labels[r] = num_classes;
    T.label_weights[r] = 0.0f;
    T.pos_assigned_gt_inds[r] = -1;
    T.sample_inds[r] = -1;
    T.is_gt[r] = (unsigned char)0;
}

// ---- arguments and workspace ----------------------------------------------------------------------------------------------------
struct Shape {
    int64_t B, M, k_max, C;      // images, proposal rows of an image, GT rows of an image at most, candidate slots k_max + M
    int64_t tiles, chunks;       // column tiles of kTile proposals, row chunks of kRows GT
};
inline Shape shape_of(int64_t B, int64_t M, int64_t k_max) {
    return Shape{B, M, k_max, k_max + M, (M + kTile - 1) / kTile, (k_max + kRows - 1) / kRows};
}
// In the order of the two neighbouring entries: box_dim -> DIM; the variant's rules, SPH2POB_FLAG_REFERENCE_ORDER, a bad edge, a
// NaN neg_pos_ub, add_gt / encode outside {0, 1} -> OPTION; the sizes -> SIZE; the pointers -> NULL.  `rc`: check_common's answer
inline int check(int rc, int variant, const float* proposals, int64_t B, int64_t M, int64_t row_stride, int box_dim, const float* gt,
                 const int64_t* gt_offsets, int64_t num_gt, int64_t k_max, int64_t num, int64_t num_expected_pos, double neg_pos_ub, int add_gt,
                 int encode, const Table& T, bool need_workspace, const void* workspace) {
    if (rc) return rc;
    if ((variant & SPH2POB_FLAG_REFERENCE_ORDER) || neg_pos_ub != neg_pos_ub || add_gt < 0 || add_gt > 1 || encode < 0 || encode > 1)
        return SPH2POB_ERR_OPTION;
    if (B < 1 || B > sph2pob_sample::kMaxImages || M < 1 || num_gt < 0 || k_max < 0 || k_max > num_gt || k_max > kMaxGt ||
        M + k_max >= ((int64_t)1 << 31) || row_stride < box_dim || row_stride > 4096 || num < 1 || num > kMaxNum || num_expected_pos < 0 ||
        num_expected_pos > num || num_gt > sph2pob::kMaxElems)
        return SPH2POB_ERR_SIZE;
    if (!proposals || !gt_offsets || (num_gt > 0 && !gt) || !T.rois || !T.labels || !T.label_weights || !T.bbox_targets || !T.bbox_weights ||
        !T.pos_assigned_gt_inds || !T.sample_inds || !T.is_gt || !T.num_pos || !T.num_neg || !T.avg_factor || !T.num_samples ||
        (need_workspace && !workspace))
        return SPH2POB_ERR_NULL;
    return SPH2POB_OK;
}

// The workspace, no initialisation: the assigned index of every candidate slot (B, C) int64 (-1 behind an image's candidates), the
// column maxima per row chunk (B, chunks, M) and the row maxima per column tile (B, k_max, tiles) as packed keys, then the
// sampler's workspace for (B, C): 2 B picks and the rank words
struct Workspace {
    int64_t* cand; unsigned long long* col_part; unsigned long long* row_part; sph2pob_sample::Workspace sample;
};
inline int64_t workspace_bytes(int64_t B, int64_t M, int64_t k_max) {
    if (B < 1 || B > sph2pob_sample::kMaxImages || M < 1 || k_max < 0 || k_max > kMaxGt || M + k_max >= ((int64_t)1 << 31)) return 0;
    const Shape s = shape_of(B, M, k_max);
    return 16 + 8 * B * (s.C + s.chunks * M + k_max * s.tiles) + sph2pob_sample::workspace_bytes(B, s.C);
}
inline Workspace carve(void* workspace, const Shape& s) {
    const uintptr_t p = (reinterpret_cast<uintptr_t>(workspace) + 15) & ~(uintptr_t)15;
    Workspace w;
    w.cand = reinterpret_cast<int64_t*>(p);
    w.col_part = reinterpret_cast<unsigned long long*>(w.cand + s.B * s.C);
    w.row_part = w.col_part + s.B * s.chunks * s.M;
    w.sample = sph2pob_sample::carve(w.row_part + s.B * s.k_max * s.tiles, s.B, s.C);
    return w;
}

}  // namespace sph2pob_rcnn
