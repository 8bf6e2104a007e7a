// Shared by the IoU / transform family of libsph2pob_hip.so (aligned and pairwise IoU, the transform, its two adjoints, the planar
// IoU: sph2pob_iou.hip, sph2pob_assign.hip) and their CPU twins (sph2pob_host.hip): the argument checks every entry point starts
// with, the (VARIANT, DIM) dispatch, the choice of a pair's IoU function and the row bodies, so that a CPU tensor gets the checks,
// the selection and the arithmetic a device tensor gets.  The kernel and the twin's loop differ in how they walk the rows and in how
// they load a spherical box (each library's load_box).  Nothing here needs the HIP runtime.
#pragma once
#include <stdint.h>

#include <initializer_list>
#include <type_traits>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_device.hpp"
#include "sph2pob_loss.hpp"
#include "sph2pob_fast.hpp"
#include "sph2pob_unbiased.hpp"

namespace sph2pob {

// ---- argument checks, in the documented order: common options, the entry's own option rule, size, the empty call, NULL ----
inline int check_common(int box_dim, int variant_flags, int edge, int angle) {
    const int variant = variant_flags & 0xff;
    if (variant_flags & ~(0xff | SPH2POB_FLAG_REFERENCE_ORDER | SPH2POB_FLAG_ROBUST_PARALLEL | SPH2POB_FLAG_NAIVE_TAN)) return SPH2POB_ERR_OPTION;
    if ((variant_flags & SPH2POB_FLAG_NAIVE_TAN) && variant != SPH2POB_VARIANT_NAIVE) return SPH2POB_ERR_OPTION;
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (variant < 0 || variant > SPH2POB_VARIANT_NAIVE || edge < 0 || edge > 2 || angle < 0 || angle > 1) return SPH2POB_ERR_OPTION;
    if (variant >= SPH2POB_VARIANT_LEGACY && variant <= SPH2POB_VARIANT_FOV_IOU && box_dim == 5)
        return SPH2POB_ERR_DIM;  // BFoV-only variants
    return SPH2POB_OK;
}
// the tail of every check: an (m, n) problem (m == n for the row-wise entries) and the pointers it needs.  An empty call is
// SPH2POB_OK whatever the pointers are: the caller returns on `rc || empty`.
inline int check_counts(int64_t m, int64_t n, std::initializer_list<const void*> pointers) {
    if (m < 0 || n < 0 || m > kMaxElems || n > kMaxElems) return SPH2POB_ERR_SIZE;
    if (m == 0 || n == 0) return SPH2POB_OK;
    for (const void* p : pointers)
        if (!p) return SPH2POB_ERR_NULL;
    return SPH2POB_OK;
}
// sph2pob_iou_aligned_f32 (m == n) / sph2pob_iou_pairwise_f32: the unbiased and the naive IoU have no IoF
inline int check_iou(int box_dim, int variant, int mode, int edge, int angle, int64_t m, int64_t n, std::initializer_list<const void*> pointers) {
    if (int rc = check_common(box_dim, variant, edge, angle)) return rc;
    if (mode < 0 || mode > 1 || ((variant & 0xff) >= SPH2POB_VARIANT_UNBIASED && mode != SPH2POB_MODE_IOU)) return SPH2POB_ERR_OPTION;
    return check_counts(m, n, pointers);
}
// sph2pob_transform_f32 and the dual-number adjoint (max_variant legacy), the closed-form adjoint (efficient; it takes no angle: 0)
inline int check_transform(int box_dim, int variant, int max_variant, int edge, int angle, int64_t n, std::initializer_list<const void*> pointers) {
    if (int rc = check_common(box_dim, variant, edge, angle)) return rc;
    if ((variant & 0xff) > max_variant) return SPH2POB_ERR_OPTION;
    return check_counts(n, n, pointers);
}
inline int check_planar_iou(const void* p1, int64_t m, const void* p2, int64_t n, const void* out, int aligned, int mode) {
    if (mode < 0 || mode > 1) return SPH2POB_ERR_OPTION;
    if (aligned && m != n) return SPH2POB_ERR_SIZE;
    return check_counts(m, n, {p1, p2, out});
}
// SPH2POB_FLAG_NAIVE_TAN travels to the naive IoU as EDGE_TANGENT (pair_iou_sel); any other call keeps its edge
inline int naive_edge(int variant_flags, int edge) { return (variant_flags & SPH2POB_FLAG_NAIVE_TAN) ? (int)EDGE_TANGENT : edge; }

// dispatch a (VARIANT, DIM) pair to a functor; f.fast: the call does not ask for the reference order
template <typename F>
int dispatch(int variant_flags, int box_dim, F&& f) {
    const int variant = variant_flags & 0xff;
    f.fast = !(variant_flags & SPH2POB_FLAG_REFERENCE_ORDER);   // SPH2POB_FLAG_ROBUST_PARALLEL: accepted, always on now
    if (variant == SPH2POB_VARIANT_STANDARD) return box_dim == 4 ? f.template run<0, 4>() : f.template run<0, 5>();
    if (variant == SPH2POB_VARIANT_EFFICIENT) return box_dim == 4 ? f.template run<1, 4>() : f.template run<1, 5>();
    if (variant == SPH2POB_VARIANT_SPH_IOU) return f.template run<3, 4>();
    if (variant == SPH2POB_VARIANT_FOV_IOU) return f.template run<4, 4>();
    if (variant == SPH2POB_VARIANT_UNBIASED) return box_dim == 4 ? f.template run<5, 4>() : f.template run<5, 5>();
    if (variant == SPH2POB_VARIANT_NAIVE) return box_dim == 4 ? f.template run<6, 4>() : f.template run<6, 5>();
    return f.template run<2, 4>();
}

// ---- the IoU of one pair.  FAST: the closed-form core of sph2pob_fast.hpp for standard / efficient, the default (double)
// arithmetic for the unbiased IoU; otherwise the reference-order path of sph2pob_device.hpp.  The naive IoU has one form. ----
template <int VARIANT, int DIM, bool FAST>
SPH_DEV float pair_iou_sel(const float (&x)[5], const float (&y)[5], int mode, int edge, int angle) {
    if constexpr (VARIANT == VARIANT_UNBIASED) return unbiased_pair_iou<DIM, !FAST>(x, y);
    else if constexpr (VARIANT == VARIANT_NAIVE) return naive_iou<DIM>(x, y, edge == EDGE_TANGENT);   // (edge carries SPH2POB_FLAG_NAIVE_TAN)
    else if constexpr (FAST) return pair_iou_fast<VARIANT, DIM>(x, y, mode, edge);
    else return pair_iou<VARIANT, DIM>(x, y, mode, edge, angle);
}
// The FAST a call gets (`fast`: no SPH2POB_FLAG_REFERENCE_ORDER): the closed form exists for standard / efficient with
// rbb_angle='equator' only; legacy, Sph-IoU and FoV-IoU have the reference order alone; naive is named with one value.
constexpr bool pair_sel_fast(int variant, bool fast, int angle) {
    return variant == VARIANT_NAIVE ? true : variant == VARIANT_UNBIASED ? fast : variant < VARIANT_LEGACY ? fast && angle == ANGLE_EQUATOR : false;
}
// f(integral_constant<int, V>, bool_constant<FAST>) for the call's selection: only what a variant can select is instantiated
template <int V, class F>
auto with_pair_sel(bool fast, int angle, F&& f) {
    constexpr std::integral_constant<int, V> v{};
    if constexpr (pair_sel_fast(V, true, ANGLE_EQUATOR) == pair_sel_fast(V, false, ANGLE_EQUATOR)) return f(v, std::bool_constant<pair_sel_fast(V, true, ANGLE_EQUATOR)>{});
    else return pair_sel_fast(V, fast, angle) ? f(v, std::true_type{}) : f(v, std::false_type{});
}

// ---- row bodies: the caller has loaded the two spherical boxes (x, y) and passes the row's own pointers ----
// the transform: planar boxes (x, y, w, h, angle) of the pair, with the reference's two jitters when asked for
template <int VARIANT, int DIM>
SPH_DEV void transform_row(float (&x)[5], float (&y)[5], int edge, int angle, int jitter, float* q1, float* q2) {
    if (jitter) jitter_spherical<DIM>(x, y);
    PBox p1, p2;
    transform<VARIANT, DIM>(x, y, edge, angle, p1, p2);
    if (jitter) jitter_rotated(p1, p2);
    q1[0] = p1.x; q1[1] = p1.y; q1[2] = p1.w; q1[3] = p1.h; q1[4] = p1.a;
    q2[0] = p2.x; q2[1] = p2.y; q2[2] = p2.w; q2[3] = p2.h; q2[4] = p2.a;
}
// its adjoint: gradients of the planar boxes (g1, g2: 5 floats) -> gradients of the spherical boxes (gb1, gb2: DIM floats).
// DUAL: forward-mode differentiation of the reference-order transforms (legacy, rbb_angle='project'); otherwise the closed form,
// which takes no angle
template <int VARIANT, int DIM, bool DUAL>
SPH_DEV void transform_bwd_row(const float (&x)[5], const float (&y)[5], const float* g1, const float* g2, int edge, int angle, int jitter,
                               float* gb1, float* gb2) {
    float gx[5], gy[5], p[5], q[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { p[k] = g1[k]; q[k] = g2[k]; }
    if constexpr (DUAL) transform_bwd_dual<VARIANT, DIM>(x, y, p, q, edge, angle, jitter != 0, gx, gy);
    else pair_transform_bwd<VARIANT, DIM>(x, y, p, q, edge, jitter != 0, gx, gy);
#pragma unroll
    for (int k = 0; k < DIM; k++) { gb1[k] = gx[k]; gb2[k] = gy[k]; }
}
// planar rotated IoU of two given planar boxes (5 floats each).  planar_iou_given, not planar_iou: no jitter runs in front of
// this entry, so coincident and near-parallel edges are its everyday input (sph2pob_device.hpp)
SPH_DEV float planar_pair(const float* a, const float* b, int mode) {
    const PBox A{a[0], a[1], a[2], a[3], a[4]}, B{b[0], b[1], b[2], b[3], b[4]};
    return planar_iou_given(A, B, mode);
}

}  // namespace sph2pob
