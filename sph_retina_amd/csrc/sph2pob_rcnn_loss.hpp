// Fused box loss of the R-CNN head on its per-class deltas — the regression half of SphShared2FCBBoxHead.loss
// (sphdet/models/heads/sph_rcnn_head.py:97-124): the shape of a call, the row rule and the argument checks, shared by the kernels
// (sph2pob_rcnn_loss.hip) and their CPU twins (sph2pob_host.hip).  The Linear head's output is (rows, slots * dim): slot c of row r
// holds the deltas of class c (slots = C), or the only ones (slots = 1: reg_class_agnostic).  A row takes part when its label is a
// class, 0 <= label < C — the reference's pos_inds — AND the loss family's own weight rule holds; of such a row ONLY the label's
// slot is read.  The arithmetic per live row is that of the flat entries, unchanged: sph2pob_delta::element (sph2pob_delta_loss.hpp)
// or decode_one -> pair_loss (sph2pob_coder.hpp, sph2pob_loss.hpp), with their product orders.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_bbox_loss.hpp"
#include "sph2pob_delta_loss.hpp"

namespace sph2pob_rcnn_loss {

using sph2pob_head::aligned16;
using sph2pob_head::effective_scale;

constexpr int kWaves = 4;            // waves of a workgroup; each owns one run of rows
// Rows of a wave's run.  The launch is latency-bound at the real shape (S = 8 x 512 rows of W = 37 x 4 floats: 2.4 MB of
// gradient), so the run is sized to spread it: 16 rows give 256 waves in 64 workgroups, each wave streaming 9.5 KB; 64 rows would
// leave 64 waves on 16 of the 256 CUs.  At most 64, so that one lane holds one row and a run is scanned and evaluated in ONE pass.
constexpr int kRun = 16;
constexpr int kMaxRowFloats = 4096 * 5;                          // slots * dim of one row at most
constexpr int64_t kMaxElems = sph2pob_bbox::kMaxLevelElems;      // rows * slots * dim: 32-bit element indices
static_assert(kRun >= 1 && kRun <= 64 && (kRun * 5) % 4 == 0, "one lane per row; a wave's LDS slice keeps 16-byte alignment");

struct Shape {
    int rows, slots, classes;
    int w;        // slots * dim floats per row
    int blocks;   // workgroups: kWaves * kRun rows each
    int vec;      // the gradient leaves in whole 16-byte stores: 16-byte aligned base and w % 4 == 0
};

// Shape checks, in the documented order (after the family's option checks); fills the shape without its `vec`.
inline int make_shape(int64_t rows, int64_t num_slots, int64_t num_classes, int dim, Shape* out) {
    if (dim != 4 && dim != 5) return SPH2POB_ERR_DIM;
    if (num_classes < 1 || num_classes > kMaxRowFloats || num_slots < 1 || (num_slots != 1 && num_slots != num_classes)) return SPH2POB_ERR_OPTION;
    if (rows < 0 || num_slots * dim > kMaxRowFloats || rows > kMaxElems / (num_slots * dim)) return SPH2POB_ERR_SIZE;
    Shape s{};
    s.rows = (int)rows; s.slots = (int)num_slots; s.classes = (int)num_classes;
    s.w = (int)(num_slots * dim);
    s.blocks = (int)((rows + kWaves * kRun - 1) / (kWaves * kRun));
    *out = s;
    return SPH2POB_OK;
}

// workgroups of the partial-sum pass of a call with this shape + 1 (0: the shape is not accepted)
inline int64_t workspace_doubles(int64_t rows, int64_t num_slots, int dim) {
    Shape s;
    if (make_shape(rows, num_slots, num_slots, dim, &s) != SPH2POB_OK) return 0;
    return (int64_t)s.blocks + 1;
}

// the pointer checks both entries end with; `rois`: NULL for the delta entry
inline int check_tensors(const Shape& s, const void* bbox_pred, const void* labels, const void* targets, bool with_rois, const void* rois,
                         int64_t roi_stride, int64_t roi_offset, int dim, const void* out, const void* workspace) {
    if (with_rois && (roi_offset < 0 || roi_stride < roi_offset + dim)) return SPH2POB_ERR_SIZE;
    if (!out || !workspace) return SPH2POB_ERR_NULL;
    if (s.rows > 0 && (!bbox_pred || !labels || !targets || (with_rois && !rois))) return SPH2POB_ERR_NULL;
    return SPH2POB_OK;
}

// The slot a row's deltas are read from and its gradient written to, or -1 when the label is not a class (background C, padding,
// ignore -1, anything else): such a row does not take part whatever its weight is.
SPHF_DEV int slot_of(int64_t label, int classes, int slots) {
    if (label < 0 || label >= classes) return -1;
    return slots == 1 ? 0 : (int)label;
}

}  // namespace sph2pob_rcnn_loss
