// Sph2PobIoULoss forward + hand-derived backward for one pair (device code, gfx950).
//
// Forward restates  Sph2PobTransfrom.new_forward (sphdet/losses/sph2pob_transform.py:24-35: clone, spherical
// jitter, sph2pob_standard(...,'rad'), rotated jitter)  followed by  obb_iou_loss
// (sphdet/losses/sph2pob_iou_loss.py:104-196: IoU | GIoU | DIoU | CIoU with obb2hbb_xyxy,
// sphdet/bbox/box_formator.py:33-54).  The reference's backward is torch autograd through ~150 recorded ops
// (transform + mmcv diff_iou_rotated_2d + penalty terms); here it is one closed-form adjoint:
//
//   planar boxes as functions of the inputs (normal branch of compute_rotate_matrix_auto):
//       pred   P = (-A/2, pi/2, k*alpha_g, k*beta_g, B_g - k*gamma_g)      k = pi/180
//       target T = (+A/2, pi/2, k*alpha_p, k*beta_p, B_p - k*gamma_p)
//       A   = angle(c_g, c_p)                      (great-circle distance of the centres)
//       B_g = atan2( c_p.d_g, -c_p.e_g)            (bearing of p seen from g in g's (south, east) frame)
//       B_p = atan2(-c_g.d_p,  c_g.e_p)
//   dI of the rectangle intersection = boundary transport: each clipped edge piece [s0, s1] of box X moves the
//   area by  len * (n . dc)  under translation, len/2 under growth of the matching extent and
//   -(s1^2 - s0^2)/2 under rotation about the centre (s measured from the edge midpoint, counter-clockwise).
//   The acos(clamp(.)) of the reference has zero gradient where the clamp is active (A/2 < 4.88e-4,
//   |cos a| > 1 - 1e-7); in-place clamps of the two jitters gate the gradient the same way torch.clamp_ does.
#pragma once
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_device.hpp"

namespace sph2pob {

enum : int { LOSS_IOU = 0, LOSS_GIOU = 1, LOSS_DIOU = 2, LOSS_CIOU = 3 };

struct ClipIv { float lo, hi; };
// clipped interval of P(tau) = p + tau*u, tau in [0, len], inside |x| <= hx, |y| <= hy (see clip_len)
SPH_DEV ClipIv clip_iv(float px, float py, float iux, float iuy, float len, float hx, float hy) {
    float ax = (-hx - px) * iux, bx = (hx - px) * iux;
    float ay = (-hy - py) * iuy, by = (hy - py) * iuy;
    float lo = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), 0.0f);
    float hi = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), len);
    // empty interval (also lo = +inf for an edge parallel to and outside a slab): collapse to [0, 0] so that the
    // length and the rotation term (hi + lo - len) * (hi - lo) stay finite
    const bool empty = !(hi > lo);
    return ClipIv{empty ? 0.0f : lo, empty ? 0.0f : hi};
}

// intersection area + its gradient w.r.t. one rectangle's own (centre-along-its-axes, w, h, a)
struct EdgeSet {
    float area2;      // twice the boundary-integral contribution (see edges_inside)
    float dcu, dcv;   // dI/d(centre) along the rectangle's own u and v axes
    float dw, dh, da; // dI/dw, dI/dh, dI/da
};
SPH_DEV EdgeSet edges_inside_grad(float pax, float pay, float c, float s, float ic, float is, float hwa, float hha,
                                  float hwb, float hhb, float wa, float ha, bool with_origin_terms) {
    float ux = hwa * c, uy = hwa * s, vx = -hha * s, vy = hha * c;
    float k0x = pax + ux + vx, k0y = pay + uy + vy;
    float k1x = pax - ux + vx, k1y = pay - uy + vy;
    float k2x = pax - ux - vx, k2y = pay - uy - vy;
    float k3x = pax + ux - vx, k3y = pay + uy - vy;
    ClipIv i0 = clip_iv(k0x, k0y, -ic, -is, wa, hwb, hhb);  // dir -u, outward normal +v
    ClipIv i1 = clip_iv(k1x, k1y, is, -ic, ha, hwb, hhb);   // dir -v, outward normal -u
    ClipIv i2 = clip_iv(k2x, k2y, ic, is, wa, hwb, hhb);    // dir +u, outward normal -v
    ClipIv i3 = clip_iv(k3x, k3y, -is, ic, ha, hwb, hhb);   // dir +v, outward normal +u
    float l0 = i0.hi - i0.lo, l1 = i1.hi - i1.lo, l2 = i2.hi - i2.lo, l3 = i3.hi - i3.lo;
    EdgeSet e;
    if (with_origin_terms) {
        float xu = pax * s - pay * c, xv = pax * c + pay * s;
        e.area2 = (l0 * (hha - xu) + l2 * (hha + xu)) + (l1 * (hwa - xv) + l3 * (hwa + xv));
    } else {
        e.area2 = hha * (l0 + l2) + hwa * (l1 + l3);
    }
    e.dcu = l3 - l1;
    e.dcv = l0 - l2;
    e.dw = 0.5f * (l1 + l3);
    e.dh = 0.5f * (l0 + l2);
    // rotation: -(s1^2 - s0^2)/2 with s = tau - len/2  ==  -(hi - lo) * ((hi + lo) - len) / 2
    e.da = -0.5f * ((l0 * ((i0.hi + i0.lo) - wa) + l2 * ((i2.hi + i2.lo) - wa)) +
                    (l1 * ((i1.hi + i1.lo) - ha) + l3 * ((i3.hi + i3.lo) - ha)));
    return e;
}

struct PlanarGrad { float x, w, h, a; };  // d(.)/d(x, w, h, a) of one planar box (y never carries gradient)

// What the front end (reference-order or closed-form) hands to the shared loss core: the two planar boxes after the
// rotated jitter in the frame "pred box at the origin" (target centre = (dx, dy)), gradient gates of every clamp /
// acos floor on the way, and the trig of the jittered spherical inputs for the chain rule.
struct LossFront {
    float dx, dy, ca, sa, cb, sb, wg, hg, wp, hp, c, s;   // (c, s) = cos / sin of (a_P - a_T)
    bool g_A, g_ag, g_ap, g_wg, g_hg, g_wp, g_hp;
    float sg, cg, sp, cp, sD, cD;  // sin/cos(phi_g), sin/cos(phi_p), sin/cos(theta_p - theta_g)
};

// reference-order front end: sph2pob_standard in the reference's fp32 operation order
template <int DIM>
SPH_DEV void loss_front_reference(const float (&b1)[5], const float (&b2)[5], LossFront& f) {
    PBox P, T;
    transform_standard<DIM>(b1, b2, EDGE_ARC, ANGLE_EQUATOR, P, T);
    const PBox P0 = P, T0 = T;  // before the rotated jitter: its clamp gates look at these
    jitter_rotated(P, T);
    f.dx = T.x - P.x; f.dy = T.y - P.y;
    f.sa = sinf(P.a); f.ca = cosf(P.a); f.sb = sinf(T.a); f.cb = cosf(T.a);
    f.c = f.ca * f.cb + f.sa * f.sb; f.s = f.sa * f.cb - f.ca * f.sb;
    f.wg = P.w; f.hg = P.h; f.wp = T.w; f.hp = T.h;
    {   // rotated-jitter clamp gates (sph_iou_api.py:237-240: in-place clamp_ => zero gradient outside)
        const float e = (float)kEpsS, e2 = (float)(2 * kEpsS), e5 = (float)(5 * kEpsS);
        const float ea = (float)kEpsA, ea2 = (float)(2 * kEpsA);
        bool similar = (fabsf(P0.x - T0.x) < e) | (fabsf(P0.w - T0.w) < e) | (fabsf(P0.h - T0.h) < e) |
                       (fabsf(P0.a - T0.a) < e);
        float pw = P0.w + (similar ? e2 : 0.0f), ph = P0.h + (similar ? e2 : 0.0f), pa = P0.a + (similar ? e : 0.0f);
        float tw = T0.w + (similar ? e : 0.0f), th = T0.h + (similar ? e : 0.0f), ta = T0.a + (similar ? e5 : 0.0f);
        if (fabsf(pa - ta) < ea) { pa += ea; ta += ea2; }
        const double pi = 3.141592653589793;
        f.g_wg = pw >= (float)(2 * kEpsA / 10); f.g_hg = ph >= (float)(2 * kEpsA / 10);
        f.g_wp = tw >= (float)(kEpsA / 10);     f.g_hp = th >= (float)(kEpsA / 10);
        bool in_a = !(pa < (float)(-2 * pi + 2 * kEpsA) || pa > (float)(2 * pi - kEpsA));
        bool in_b = !(ta < (float)(-2 * pi + kEpsA) || ta > (float)(2 * pi - 2 * kEpsA));
        f.g_ag = in_a;
        f.g_ap = in_b;
    }
    SBox g = load_sbox<DIM>(b1), p = load_sbox<DIM>(b2);
    f.sg = g.sp; f.cg = g.cp; f.sp = p.sp; f.cp = p.cp;
    f.cD = p.ct * g.ct + p.st * g.st;
    f.sD = p.st * g.ct - p.ct * g.st;
    // x' = +-acos(clamp(cos(A/2))) of compute_spherical_coordinate: gate on A/2 >= acos(1 - 1e-7)
    float N = f.sp * f.cg * f.cD - f.cp * f.sg, D = -f.sp * f.sD;
    float C = f.cg * f.cp + f.sg * f.sp * f.cD;
    f.g_A = atan2f(sqrtf(N * N + D * D), C) > 2.0f * 4.8828125e-4f;
    // acos(clamp(., -1+1e-7, 1-1e-7)) of compute_internal_angle: zero gradient where the clamp is active, i.e. where the
    // planar angle BEFORE its floor is within kGateAng of 0 | pi.  P0.a / T0.a are already floored (to kMinAng, whose
    // cosine is the clamp bound itself), so the angle is taken again from the bearings: a = atan2(N, D) - k * gamma
    float Np = f.cg * f.sp - f.sg * f.cp * f.cD, Dp = -f.sg * f.sD;
    const float kg = DIM == 5 ? b1[4] * kDeg2Rad : 0.0f, kp = DIM == 5 ? b2[4] * kDeg2Rad : 0.0f;
    f.g_ag = f.g_ag && fabsf(sinf(atan2f(N, D) - kg)) >= kGateAng;
    f.g_ap = f.g_ap && fabsf(sinf(atan2f(Np, Dp) - kp)) >= kGateAng;
}

}  // namespace sph2pob
#include "sph2pob_fast.hpp"

namespace sph2pob {
// 1 / b and a / b from the hardware reciprocal plus one Newton step (~1 ulp).  The IEEE divide expands to ~12
// instructions, 5 of them at the slow issue rate (v_div_scale x2, v_div_fmas, v_div_fixup, v_rcp): the loss kernels
// are VALU-issue-bound and divided 7 (forward) to 19 (backward) times per pair.  Only for denominators that cannot be
// 0 / inf (sums with eps, squares of clamped extents); the clip reciprocals use the bare, clamped v_rcp.
SPH_DEV float rcp_nr(float b) {
    float r = fast_rcp(b);
    return r * (2.0f - b * r);
}
SPH_DEV float fdiv(float a, float b) { return a * rcp_nr(b); }
}  // namespace sph2pob
namespace sph2pob {

// closed-form front end (sph2pob_fast.hpp): same planar boxes, ~4x fewer instructions
template <int DIM, int VARIANT = VARIANT_STANDARD>
SPH_DEV void loss_front_fast(const float (&b1)[5], const float (&b2)[5], LossFront& f, int edge = EDGE_ARC,
                             bool rot_jitter = true) {
    FastTrig t;
    PlanarPair q;
    // rot_jitter == "the caller ran jitter_spherical first", i.e. the angles are clamped into the range of the cheap trig
    if (rot_jitter) lean_front<VARIANT, DIM, true, true>(b1, b2, edge, q, &t);
    else lean_front<VARIANT, DIM, true, false>(b1, b2, edge, q, &t);
    if (!rot_jitter) { q.g_wg = q.g_hg = q.g_wp = q.g_hp = true; }
    f.dx = q.dx; f.dy = q.dy; f.ca = q.ca; f.sa = q.sa; f.cb = q.cb; f.sb = q.sb; f.c = q.c; f.s = q.s;
    f.wg = q.wg; f.hg = q.hg; f.wp = q.wp; f.hp = q.hp;
    f.g_A = q.g_A; f.g_ag = q.g_ag; f.g_ap = q.g_ap; f.g_wg = q.g_wg; f.g_hg = q.g_hg; f.g_wp = q.g_wp; f.g_hp = q.g_hp;
    f.sg = t.sg; f.cg = t.cg; f.sp = t.sp; f.cp = t.cp; f.sD = t.sD; f.cD = t.cD;
}

// Chain rule from gradients w.r.t. the two planar boxes (x, w, h, a) to gradients w.r.t. the spherical inputs
// (degrees).  x_split: P.x = -x_split*A and T.x = +(1 - x_split)*A ... expressed as dT.x/dA - dP.x/dA = 1:
// standard (x = -+A/2) passes 0.5, efficient (P.x = 0, T.x = A) passes 0.  Gates: acos(clamp) floors and the rotated
// jitter's clamps (from the front end), the spherical jitter's in-place clamps (here, when `jitter`).
template <int DIM>
SPH_DEV void planar_to_spherical_grads(const LossFront& f, PlanarGrad gP, PlanarGrad gT, float x_split,
                                       const float (&pred)[5], const float (&target)[5], bool jitter, int edge,
                                       float (&gpred)[5], float (&gtarget)[5]) {
    if (!f.g_wg) gP.w = 0.0f;
    if (!f.g_hg) gP.h = 0.0f;
    if (!f.g_wp) gT.w = 0.0f;
    if (!f.g_hp) gT.h = 0.0f;
    float GA = f.g_A ? ((1.0f - x_split) * gT.x - x_split * gP.x) : 0.0f;
    float Gag = f.g_ag ? gP.a : 0.0f;
    float Gap = f.g_ap ? gT.a : 0.0f;
    const float sg = f.sg, cg = f.cg, sp = f.sp, cp = f.cp, sD = f.sD, cD = f.cD;
    float N = sp * cg * cD - cp * sg;    //  c_p . d_g
    float D = -sp * sD;                  // -c_p . e_g
    float Np = cg * sp - sg * cp * cD;   // -c_g . d_p
    float Dp = -sg * sD;                 //  c_g . e_p
    float C = cg * cp + sg * sp * cD;    //  cos A
    float sin2 = N * N + D * D;          //  sin^2 A
    float inv_s = fast_rsq(sin2);
    inv_s = sin2 > 1e-20f ? inv_s * (1.5f - 0.5f * sin2 * inv_s * inv_s) : 0.0f;  // 1 / sin A, one Newton step
    float inv_s2 = inv_s * inv_s;
    // dA = -dC / sinA
    float dA_phg = -N * inv_s, dA_php = Np * inv_s;
    float dA_thg = -(sg * sp * sD) * inv_s, dA_thp = (sg * sp * sD) * inv_s;
    // dB_g = (D dN - N dD) / sin^2 A
    float dBg_phg = (D * (-C)) * inv_s2;
    float dBg_thg = (D * (sp * cg * sD) - N * (sp * cD)) * inv_s2;
    float dpdg = cp * cg * cD + sp * sg;  // d_p . d_g
    float dBg_php = (D * dpdg - N * (-cp * sD)) * inv_s2;
    float dBg_thp = (D * (-sp * cg * sD) - N * (-sp * cD)) * inv_s2;
    // dB_p = (D' dN' - N' dD') / sin^2 A
    float dBp_php = (Dp * C) * inv_s2;
    float dBp_thp = (Dp * (sg * cp * sD) - Np * (-sg * cD)) * inv_s2;
    float dBp_phg = (Dp * (-dpdg) - Np * (-cg * sD)) * inv_s2;
    float dBp_thg = (Dp * (-sg * cp * sD) - Np * (sg * cD)) * inv_s2;

    float r_g[5], r_p[5];  // gradients w.r.t. radians
    r_g[0] = GA * dA_thg + Gag * dBg_thg + Gap * dBp_thg;
    r_g[1] = GA * dA_phg + Gag * dBg_phg + Gap * dBp_phg;
    r_g[2] = gP.w; r_g[3] = gP.h; r_g[4] = -Gag;
    r_p[0] = GA * dA_thp + Gag * dBg_thp + Gap * dBp_thp;
    r_p[1] = GA * dA_php + Gag * dBg_php + Gap * dBp_php;
    r_p[2] = gT.w; r_p[3] = gT.h; r_p[4] = -Gap;

    // spherical-jitter shifts / clamps (sph_iou_api.py:244-258): gates look at the pre-clamp values
    const float eps1 = (float)kEpsS, eps2 = (float)(2 * kEpsS);
    bool similar = false;
    if (jitter) {
#pragma unroll
        for (int k = 0; k < DIM; k++) similar |= fabsf(pred[k] - target[k]) < eps1;
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        if (k >= DIM) { gpred[k] = 0.0f; gtarget[k] = 0.0f; continue; }
        float x1 = pred[k] - (similar ? eps2 : 0.0f), x2 = target[k] + (similar ? eps1 : 0.0f);
        float hi1 = k == 0 ? (float)(360.0 - kEpsS) : (float)(180.0 - kEpsS);
        float hi2 = k == 0 ? (float)(360.0 - 2 * kEpsS) : (float)(180.0 - 2 * kEpsS);
        bool in1 = !jitter || k == 4 || (x1 >= eps2 && x1 <= hi1);
        bool in2 = !jitter || (k == 4 ? (x2 >= (float)(-360.0 + 2 * kEpsS) && x2 <= (float)(360.0 - 2 * kEpsS))
                                      : (x2 >= eps1 && x2 <= hi2));
        float s1 = kDeg2Rad, s2 = kDeg2Rad;
        if ((k == 2 || k == 3) && edge != EDGE_ARC) {  // d(edge length)/d(fov): chord cos(f/2), tangent 1/cos^2(f/2)
            float jg = in1 ? fminf(fmaxf(x1, jitter ? eps2 : x1), jitter ? hi1 : x1) : x1;
            float jp = in2 ? fminf(fmaxf(x2, jitter ? eps1 : x2), jitter ? hi2 : x2) : x2;
            float c1 = cosf(0.5f * jg * kDeg2Rad), c2 = cosf(0.5f * jp * kDeg2Rad);
            s1 *= edge == EDGE_CHORD ? c1 : 1.0f / (c1 * c1);
            s2 *= edge == EDGE_CHORD ? c2 : 1.0f / (c2 * c2);
        }
        gpred[k] = in1 ? r_g[k] * s1 : 0.0f;
        gtarget[k] = in2 ? r_p[k] * s2 : 0.0f;
    }
}

// Per-pair loss element; when BWD, also d(loss)/d(pred[0..DIM)) and d(loss)/d(target[0..DIM)) in 1/degree.
template <int DIM, bool BWD, bool FAST>
SPH_DEV float pair_loss(const float (&pred)[5], const float (&target)[5], int loss_mode, float eps, float* iou_out,
                        float (&gpred)[5], float (&gtarget)[5]) {
    if (pair_has_nan<DIM>(pred, target)) {
        // torch propagates a NaN coordinate into the loss element and, through autograd, into every gradient of the
        // pair; the clamps / min / max on the way here would drop it and train on garbage
        const float qnan = __builtin_nanf("");
        if (iou_out) *iou_out = qnan;
#pragma unroll
        for (int k = 0; k < 5; k++) { gpred[k] = k < DIM ? qnan : 0.0f; gtarget[k] = k < DIM ? qnan : 0.0f; }
        return qnan;
    }
    float b1[5], b2[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { b1[k] = pred[k]; b2[k] = target[k]; }
    jitter_spherical<DIM>(b1, b2);
    LossFront f;
    if (FAST) loss_front_fast<DIM>(b1, b2, f);
    else loss_front_reference<DIM>(b1, b2, f);
    const float sa = f.sa, ca = f.ca, sb = f.sb, cb = f.cb, dx = f.dx, dy = f.dy;
    struct { float x, y, w, h; } P{0.0f, 0.0f, f.wg, f.hg}, T{dx, dy, f.wp, f.hp};

    // ---- planar IoU (value of mmcv diff_iou_rotated_2d: sphdet/iou/diff_iou_rotated.py:325-343) ----
    const float c = f.c, s = f.s;
    // clamped reciprocals: exactly parallel edges (s == 0 after the jitter bumps) give finite, correctly ordered bounds
    float ic = fminf(fmaxf(fast_rcp(c), -1e18f), 1e18f), is = fminf(fmaxf(fast_rcp(s), -1e18f), 1e18f);
    float hwa = 0.5f * P.w, hha = 0.5f * P.h, hwb = 0.5f * T.w, hhb = 0.5f * T.h;
    float pax = -(dx * cb + dy * sb), pay = -(dy * cb - dx * sb);
    float pbx = dx * ca + dy * sa, pby = dy * ca - dx * sa;
    EdgeSet eA = edges_inside_grad(pax, pay, c, s, ic, is, hwa, hha, hwb, hhb, P.w, P.h, true);
    EdgeSet eB = edges_inside_grad(pbx, pby, c, -s, ic, -is, hwb, hhb, hwa, hha, T.w, T.h, false);
    float I = 0.5f * fmaxf(eA.area2 + eB.area2, 0.0f);
    {   // near-parallel planar boxes (the two jitter steps cancelled: DESIGN.md §9): the value of the intersection comes
        // from the first-order form; the boundary-transport gradient terms above stay (their relative error there is the
        // integral's, a few percent at worst, on ~1e-4 of the pairs).  Wave-uniform guard: the common wave skips the code.
        const bool near = fminf(fabsf(s), fabsf(c)) < kNearParallel;
#if defined(__HIP_DEVICE_COMPILE__)
        if (__ballot(near) != 0ull)
#endif
            if (near) I = fmaxf(near_parallel_inter(pax, pay, c, s, hwa, hha, hwb, hhb), 0.0f);
    }
    float S1 = P.w * P.h, S2 = T.w * T.h;
    float U = S1 + S2 - I;
    float iou_raw = fdiv(I, U);
    float iou = fminf(fmaxf(iou_raw, 0.0f), 1.0f);
    if (iou_out) *iou_out = iou;

    // ---- penalty terms (sph2pob_iou_loss.py:139-194) ----
    float aca = fabsf(ca), asa = fabsf(sa), acb = fabsf(cb), asb = fabsf(sb);
    float Wg = aca * P.w + asa * P.h, Hg = asa * P.w + aca * P.h;
    float Wp = acb * T.w + asb * T.h, Hp = asb * T.w + acb * T.h;
    float x1g = P.x - Wg / 2.0f, x2g = P.x + Wg / 2.0f, y1g = P.y - Hg / 2.0f, y2g = P.y + Hg / 2.0f;
    float x1p = T.x - Wp / 2.0f, x2p = T.x + Wp / 2.0f, y1p = T.y - Hp / 2.0f, y2p = T.y + Hp / 2.0f;
    float cw = fmaxf(fmaxf(x2g, x2p) - fminf(x1g, x1p), 0.0f);
    float ch = fmaxf(fmaxf(y2g, y2p) - fminf(y1g, y1p), 0.0f);
    float loss, pen_ratio = 0.0f, c2 = 0.0f, rho2 = 0.0f, v = 0.0f, alpha = 0.0f, dv = 0.0f;
    float iw = 0.0f, ih = 0.0f, ae = 0.0f, au = 0.0f;
    if (loss_mode == LOSS_IOU) {
        loss = 1.0f - iou;
    } else if (loss_mode == LOSS_GIOU) {
        iw = fmaxf(fminf(x2g, x2p) - fmaxf(x1g, x1p), 0.0f);
        ih = fmaxf(fminf(y2g, y2p) - fmaxf(y1g, y1p), 0.0f);
        ae = cw * ch;
        au = S1 + S2 - iw * ih;
        pen_ratio = fdiv(ae - au, ae + eps);
        loss = 1.0f - (iou - fminf(fmaxf(pen_ratio, 0.0f), 1.0f));
    } else {
        c2 = cw * cw + ch * ch + eps;
        rho2 = dx * dx + dy * dy;
        pen_ratio = fdiv(rho2, c2);
        float pen = fminf(fmaxf(pen_ratio, 0.0f), 1.0f);
        if (loss_mode == LOSS_CIOU) {
            const float factor = (float)(4.0 / (3.141592653589793 * 3.141592653589793));
            dv = atan2_r(T.w, T.h + eps) - atan2_r(P.w, P.h + eps);   // widths and heights are positive
            v = factor * (dv * dv);
            alpha = fdiv((iou > 0.5f ? 1.0f : 0.0f) * v, 1.0f - iou + v + eps);
            pen = pen + alpha * v;
        }
        loss = 1.0f - (iou - pen);
    }
    if (!BWD) return loss;

    // =========================== adjoint ===========================
    PlanarGrad gP{0, 0, 0, 0}, gT{0, 0, 0, 0};
    // -- IoU term: L = 1 - iou  (torch.clamp passes gradient on the closed range [0, 1]) --
    if (iou_raw >= 0.0f && iou_raw <= 1.0f) {
        float inv_u = rcp_nr(U), inv_u2 = inv_u * inv_u;
        float LI = -(S1 + S2) * inv_u2;  // dL/dI
        float LS = I * inv_u2;           // dL/dS1 = dL/dS2
        if (eA.area2 + eB.area2 <= 0.0f) LI = 0.0f;
        // centre derivative in world x: dcu * cos(a) - dcv * sin(a)
        gP.x += LI * (eA.dcu * ca - eA.dcv * sa);
        gT.x += LI * (eB.dcu * cb - eB.dcv * sb);
        gP.w += LI * eA.dw + LS * P.h;  gP.h += LI * eA.dh + LS * P.w;  gP.a += LI * eA.da;
        gT.w += LI * eB.dw + LS * T.h;  gT.h += LI * eB.dh + LS * T.w;  gT.a += LI * eB.da;
    }
    if (loss_mode != LOSS_IOU) {
        // d(hbb extents)/d(w, h, a)
        float sgca = ca >= 0.0f ? 1.0f : -1.0f, sgsa = sa >= 0.0f ? 1.0f : -1.0f;
        float sgcb = cb >= 0.0f ? 1.0f : -1.0f, sgsb = sb >= 0.0f ? 1.0f : -1.0f;
        float dWg_a = -sgca * sa * P.w + sgsa * ca * P.h, dHg_a = sgsa * ca * P.w - sgca * sa * P.h;
        float dWp_a = -sgcb * sb * T.w + sgsb * cb * T.h, dHp_a = sgsb * cb * T.w - sgcb * sb * T.h;
        // which box supplies each side of the enclosing / intersecting hbb
        float g_x2 = x2g >= x2p ? 1.0f : 0.0f, g_x1 = x1g <= x1p ? 1.0f : 0.0f;
        float g_y2 = y2g >= y2p ? 1.0f : 0.0f, g_y1 = y1g <= y1p ? 1.0f : 0.0f;
        float Lcw = 0.0f, Lch = 0.0f;  // dL/dcw, dL/dch
        if (loss_mode == LOSS_GIOU) {
            if (pen_ratio >= 0.0f && pen_ratio <= 1.0f) {
                float den = ae + eps;
                float iden = rcp_nr(den), Rae = (eps + au) * (iden * iden), Rau = -iden;
                Lcw = Rae * ch; Lch = Rae * cw;
                // au = S1 + S2 - iw*ih
                gP.w += Rau * P.h; gP.h += Rau * P.w; gT.w += Rau * T.h; gT.h += Rau * T.w;
                float Liw = -Rau * ih, Lih = -Rau * iw;
                if (fminf(x2g, x2p) - fmaxf(x1g, x1p) < 0.0f) Liw = 0.0f;
                if (fminf(y2g, y2p) - fmaxf(y1g, y1p) < 0.0f) Lih = 0.0f;
                // iw = min(x2g, x2p) - max(x1g, x1p)
                float h_x2 = x2g <= x2p ? 1.0f : 0.0f, h_x1 = x1g >= x1p ? 1.0f : 0.0f;
                float h_y2 = y2g <= y2p ? 1.0f : 0.0f, h_y1 = y1g >= y1p ? 1.0f : 0.0f;
                float iwWg = 0.5f * (h_x2 + h_x1), iwWp = 0.5f * ((1 - h_x2) + (1 - h_x1));
                float ihHg = 0.5f * (h_y2 + h_y1), ihHp = 0.5f * ((1 - h_y2) + (1 - h_y1));
                gP.x += Liw * (h_x2 - h_x1);
                gT.x += Liw * ((1 - h_x2) - (1 - h_x1));
                float LWg = Liw * iwWg, LWp = Liw * iwWp, LHg = Lih * ihHg, LHp = Lih * ihHp;
                gP.w += LWg * aca + LHg * asa; gP.h += LWg * asa + LHg * aca; gP.a += LWg * dWg_a + LHg * dHg_a;
                gT.w += LWp * acb + LHp * asb; gT.h += LWp * asb + LHp * acb; gT.a += LWp * dWp_a + LHp * dHp_a;
            }
        } else {
            if (pen_ratio >= 0.0f && pen_ratio <= 1.0f) {
                float Lrho = rcp_nr(c2), Lc2 = -rho2 * (Lrho * Lrho);
                gT.x += Lrho * 2.0f * dx;
                gP.x -= Lrho * 2.0f * dx;
                Lcw = Lc2 * 2.0f * cw; Lch = Lc2 * 2.0f * ch;
            }
            if (loss_mode == LOSS_CIOU) {
                const float factor = (float)(4.0 / (3.141592653589793 * 3.141592653589793));
                float Ldv = alpha * factor * 2.0f * dv;  // alpha is a constant (torch.no_grad) :188-189
                float hpe = T.h + eps, hge = P.h + eps;
                float qp = rcp_nr(hpe * hpe + T.w * T.w), qg = rcp_nr(hge * hge + P.w * P.w);
                gT.w += Ldv * hpe * qp;  gT.h -= Ldv * T.w * qp;
                gP.w -= Ldv * hge * qg;  gP.h += Ldv * P.w * qg;
            }
        }
        if (fmaxf(x2g, x2p) - fminf(x1g, x1p) < 0.0f) Lcw = 0.0f;
        if (fmaxf(y2g, y2p) - fminf(y1g, y1p) < 0.0f) Lch = 0.0f;
        // cw = max(x2g, x2p) - min(x1g, x1p), x2 = x + W/2, x1 = x - W/2
        gP.x += Lcw * (g_x2 - g_x1);
        gT.x += Lcw * ((1 - g_x2) - (1 - g_x1));
        float LWg = Lcw * 0.5f * (g_x2 + g_x1), LWp = Lcw * 0.5f * ((1 - g_x2) + (1 - g_x1));
        float LHg = Lch * 0.5f * (g_y2 + g_y1), LHp = Lch * 0.5f * ((1 - g_y2) + (1 - g_y1));
        gP.w += LWg * aca + LHg * asa; gP.h += LWg * asa + LHg * aca; gP.a += LWg * dWg_a + LHg * dHg_a;
        gT.w += LWp * acb + LHp * asb; gT.h += LWp * asb + LHp * acb; gT.a += LWp * dWp_a + LHp * dHp_a;
    }

    // -- chain rule back to the spherical inputs (degrees) --
    planar_to_spherical_grads<DIM>(f, gP, gT, /*x_split=*/0.5f, pred, target, /*jitter=*/true, EDGE_ARC, gpred, gtarget);
    return loss;
}

// Adjoint of sph2pob_{standard,efficient}(...,'rad') (+ the two jitters when `jitter`): gradients of the two planar
// boxes (x, y, w, h, a) -> gradients of the spherical inputs.  y carries no gradient (it is the constant pi/2 | 0).
template <int VARIANT, int DIM>
SPH_DEV void pair_transform_bwd(const float (&in1)[5], const float (&in2)[5], const float (&g1)[5], const float (&g2)[5],
                                int edge, bool jitter, float (&gin1)[5], float (&gin2)[5]) {
    float b1[5], b2[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { b1[k] = in1[k]; b2[k] = in2[k]; }
    if (jitter) jitter_spherical<DIM>(b1, b2);
    LossFront f;
    loss_front_fast<DIM, VARIANT>(b1, b2, f, edge, jitter);
    PlanarGrad gP{g1[0], g1[2], g1[3], g1[4]}, gT{g2[0], g2[2], g2[3], g2[4]};
    planar_to_spherical_grads<DIM>(f, gP, gT, VARIANT == VARIANT_STANDARD ? 0.5f : 0.0f, in1, in2, jitter, edge, gin1, gin2);
}

// ================= Gaussian losses: Sph2PobGDLoss (GWD / KLD / JD / KLD sym-max / sym-min) and Sph2PobKFLoss =================
// mmrotate's gaussian_dist_loss.py / kf_iou_loss.py bodies (restated from the published source: parity UNPINNED) on the
// planar boxes the Sph2Pob front end produces.  Box X -> N(mu = (x, y), Sigma = R(a) diag(A, B) R(a)^T), A = w^2/4,
// B = h^2/4 (w, h clamped to [1e-7, 1e7]); with D = a_P - a_T, c2 = cos^2 D, s2 = sin^2 D every matrix expression has a
// closed form in (A_P, B_P, A_T, B_T, c2, s2) and the centre offset in the reference box's axes.  Every clamp gates its
// gradient as torch.clamp does (passes on the closed interval).
enum : int { GAUSS_GWD = 0, GAUSS_KLD = 1, GAUSS_JD = 2, GAUSS_KLD_SYMMAX = 3, GAUSS_KLD_SYMMIN = 4, GAUSS_KF = 5 };
enum : int { GFUN_NONE = 0, GFUN_LOG1P = 1, GFUN_SQRT = 2, GFUN_LN = 3, GFUN_EXP = 4 };
enum : int { GOPT_SQRT = 1, GOPT_NORMALIZE = 2 };

// sqrt(max(x, lo)) and its gate
SPH_DEV float sqrt_floor(float x, float lo, bool& pass) {
    pass = x >= lo;
    return sqrtf(fmaxf(x, lo));
}

// post-map of gaussian_dist_loss.postprocess: log1p | sqrt(max(., 1e-7)) | identity, then 1 - 1 / (tau + d) when tau >= 1
SPH_DEV float gauss_post(float d, int fun, float tau, float& dpost) {
    float v = d, g = 1.0f;
    if (fun == GFUN_LOG1P) {
        v = log1pf(d);
        g = rcp_nr(1.0f + d);
    } else if (fun == GFUN_SQRT) {
        bool pass;
        v = sqrt_floor(d, 1e-7f, pass);
        g = pass ? 0.5f * rcp_nr(v) : 0.0f;
    }
    if (tau >= 1.0f) {
        const float q = rcp_nr(tau + v);
        g *= q * q;
        v = ((tau - 1.0f) + v) * q;   // 1 - 1 / (tau + v) without the cancellation: at v ~ 3e-4 `1 - q` keeps 11 bits
    }
    dpost = g;
    return v;
}

// x - log1p(x) without the cancellation near 0 (x^2 / 2 - x^3 / 3 + ...: below 2^-6 the series, truncated at 2e-8 relative)
SPH_DEV float x_minus_log1p(float x) {
    if (fabsf(x) < 0.015625f) return x * x * (0.5f - x * ((1.0f / 3.0f) - x * (0.25f - x * 0.2f)));
    return x - log1pf(x);
}

// kld_loss before its sqrt / post-map, reference box a (the inverse is taken of a's covariance), other box b:
//   0.5 d^T Sa^-1 d / alpha^2 + 0.5 tr(Sa^-1 Sb) + 0.5 ln(det Sa / det Sb) - 1,   (u, v) = d in a's axes
// As pred -> target, 0.5 tr -> 1 and the logarithm -> 0 while the sum falls to 1e-5 and below: written as it stands the result
// keeps the absolute error of the 1 (1e-7, i.e. 1e-2 relative, and the gradient of its square root with it).  In the
// differences dA = Ab - Aa, dB = Bb - Ba (formed from the differences of the extents), eb = Bb - Ab, ea = Ba - Aa:
//   0.5 tr - 1 + 0.5 ln(.) = 0.5 [ (x - log1p x) + (y - log1p y) + s2 eb ea / (Aa Ba) ],   x = dA / Aa, y = dB / Ba
SPH_DEV float kld_raw(float Aa, float Ba, float dA, float dB, float eb, float ea, float u, float v, float s2, float ia2) {
    const float iAa = rcp_nr(Aa), iBa = rcp_nr(Ba);
    const float xy = 0.5f * (u * u * iAa + v * v * iBa);
    const float shape = (x_minus_log1p(dA * iAa) + x_minus_log1p(dB * iBa)) + s2 * eb * ea * (iAa * iBa);
    return xy * ia2 + 0.5f * shape;
}
// its adjoint for an upstream gradient G: accumulates d/d(Aa, Ba, Ab, Bb), d/d(centre offset x), d/d(a_a) through the
// axes of (u, v) [(ca, sa) = cos / sin a_a] and d/d(a_a - a_b) [cs = cos * sin of a_a - a_b]; the same differences keep the
// extent columns, which vanish as the boxes meet, free of the 1 - 1 they would otherwise be read off
SPH_DEV void kld_raw_adj(float G, float Aa, float Ba, float Ab, float Bb, float dA, float dB, float eb, float ea, float u, float v,
                         float ca, float sa, float s2, float cs, float ia2, float& gAa, float& gBa, float& gAb, float& gBb,
                         float& gdx, float& gaa, float& gdab) {
    const float iAa = rcp_nr(Aa), iBa = rcp_nr(Ba);
    const float gu = G * ia2 * u * iAa, gv = G * ia2 * v * iBa;
    gdx += gu * ca - gv * sa;
    gaa += gu * v - gv * u;
    const float hG = 0.5f * G;
    // tr(Sa^-1 Sb) = p + q, p - 1 = (dA + s2 eb) / Aa, q - 1 = (dB - s2 eb) / Ba
    gAa -= hG * iAa * ((dA + s2 * eb) * iAa + ia2 * u * u * iAa);
    gBa -= hG * iBa * ((dB - s2 * eb) * iBa + ia2 * v * v * iBa);
    // c2 / Aa + s2 / Ba - 1 / Ab = dA / (Aa Ab) - s2 ea / (Aa Ba),   s2 / Aa + c2 / Ba - 1 / Bb = dB / (Ba Bb) + s2 ea / (Aa Ba)
    const float se = s2 * ea * (iAa * iBa);
    gAb += hG * (dA * iAa * rcp_nr(Ab) - se);
    gBb += hG * (dB * iBa * rcp_nr(Bb) + se);
    gdab += G * cs * eb * ea * (iAa * iBa);
}

// The trailing parameters of the Gaussian launchers, and the per-pair body of their kernels and host twins.
struct GaussBody {
    int type, fun;   // GAUSS_*, GFUN_*
    float tau, alpha;
    int opts;        // GOPT_SQRT (kld family), GOPT_NORMALIZE (gwd)
    float beta, eps; // KF: smooth-L1 beta of the centre term, eps of the KFIoU denominator
    template <int DIM, bool BWD, bool FAST>
    SPH_DEV float eval(const float (&pred)[5], const float (&target)[5], float* iou_out, float (&gpred)[5],
                       float (&gtarget)[5]) const;
};

// The Gaussian body on the planar boxes a front end produced: the loss element and, when BWD, its gradients w.r.t. the two
// planar boxes.
template <bool BWD>
SPH_DEV float gauss_body(const LossFront& f, const GaussBody& p, PlanarGrad& gP, PlanarGrad& gT) {
    const float dx = f.dx, dy = f.dy, c2 = f.c * f.c, s2 = f.s * f.s, cs = f.c * f.s;
    // xy_wh_r_2_xy_sigma: wh.clamp(1e-7, 1e7), Sigma = R diag(wh / 2)^2 R^T
    const float wP = fminf(fmaxf(f.wg, 1e-7f), 1e7f), hP = fminf(fmaxf(f.hg, 1e-7f), 1e7f);
    const float wT = fminf(fmaxf(f.wp, 1e-7f), 1e7f), hT = fminf(fmaxf(f.hp, 1e-7f), 1e7f);
    const float AP = 0.25f * wP * wP, BP = 0.25f * hP * hP, AT = 0.25f * wT * wT, BT = 0.25f * hT * hT;
    const float detP = AP * BP, detT = AT * BT;
    // adjoint accumulators: d/d(A_P, B_P, A_T, B_T), d/d(dx = T.x - P.x), d/d(a_P - a_T), d/d(a_P), d/d(a_T) (centre axes)
    float gAP = 0.0f, gBP = 0.0f, gAT = 0.0f, gBT = 0.0f, gdx = 0.0f, gD = 0.0f, gaP = 0.0f, gaT = 0.0f;
    float loss;
    if (p.type == GAUSS_KF) {
        // kfiou_loss with pred_decode = T, targets_decode = P (Sigma_1 from T, Sigma_2 from P)
        const float V1 = 4.0f * sqrtf(detT), V2 = 4.0f * sqrtf(detP);
        // det(S_P + S_T); det of S_1 - S_1 (S_1 + S_2)^-1 S_1 = det S_P det S_T / det(S_P + S_T) > 0: Vb is never NaN here
        const float Ds = (AP + AT) * (BP + BT) * c2 + (AP + BT) * (BP + AT) * s2;
        const float iDs = rcp_nr(Ds);
        const float Vb = 4.0f * sqrtf(detP * detT * iDs);
        const float den = V1 + V2 - Vb + p.eps;
        const float iden = rcp_nr(den);
        const float K = Vb * iden;
        float kf;
        if (p.fun == GFUN_LN) kf = -logf(K + p.eps);
        else if (p.fun == GFUN_EXP) kf = expf(1.0f - K) - 1.0f;
        else kf = 1.0f - K;
        const float ax = fabsf(dx), ay = fabsf(dy), beta = p.beta;
        const float xy = (ax < beta ? 0.5f * ax * ax / beta : ax - 0.5f * beta) +
                         (ay < beta ? 0.5f * ay * ay / beta : ay - 0.5f * beta);
        const float raw = xy + kf;
        loss = fmaxf(raw, 0.0f);
        if (BWD && raw >= 0.0f) {
            const float sx = dx > 0.0f ? 1.0f : (dx < 0.0f ? -1.0f : 0.0f);
            gdx = sx * (ax < beta ? ax / beta : 1.0f);
            float gK;
            if (p.fun == GFUN_LN) gK = -rcp_nr(K + p.eps);
            else if (p.fun == GFUN_EXP) gK = -expf(1.0f - K);
            else gK = -1.0f;
            const float gVb = gK * (den + Vb) * (iden * iden), gV = -gK * Vb * (iden * iden);
            // V = 4 sqrt(A B): dV/dA = V / (2A)
            gAT += gV * 0.5f * V1 * rcp_nr(AT); gBT += gV * 0.5f * V1 * rcp_nr(BT);
            gAP += gV * 0.5f * V2 * rcp_nr(AP); gBP += gV * 0.5f * V2 * rcp_nr(BP);
            // ln Vb = ln 4 + (ln A_P + ln B_P + ln A_T + ln B_T - ln Ds) / 2
            const float h = 0.5f * gVb * Vb;
            gAP += h * (rcp_nr(AP) - ((BP + BT) * c2 + (BP + AT) * s2) * iDs);
            gBP += h * (rcp_nr(BP) - ((AP + AT) * c2 + (AP + BT) * s2) * iDs);
            gAT += h * (rcp_nr(AT) - ((BP + BT) * c2 + (AP + BT) * s2) * iDs);
            gBT += h * (rcp_nr(BT) - ((AP + AT) * c2 + (BP + AT) * s2) * iDs);
            gD -= h * 2.0f * cs * (AP - BP) * (AT - BT) * iDs;
        }
    } else if (p.type == GAUSS_GWD) {
        const float targ = detP * detT;
        bool pt, pr, pd;
        const float t = sqrt_floor(targ, 1e-7f, pt);
        const float Q = (AP * AT + BP * BT) * c2 + (AP * BT + BP * AT) * s2;   // tr(S_P S_T)
        const float R = Q + 2.0f * t;
        const float S = sqrt_floor(R, 1e-7f, pr);
        float whr = (AP + BP) + (AT + BT) - 2.0f * S;
        if (pt && pr) {
            // no floor is active: t = w_P h_P w_T h_T / 16 and tr S_P + tr S_T - 2 S = ((tr S_P + tr S_T)^2 - 4 R) / (... + 2 S) with
            //   (.)^2 - 4 R = (tr S_T - tr S_P)^2 + (w_P h_T - h_P w_T)^2 / 4 + 4 s2 (A_P - B_P)(A_T - B_T),
            // every term from differences of the extents: as pred -> target the subtraction above keeps 1e-7 of a Wasserstein
            // term that falls to 1e-5, and the gradient (1 / d) with it
            const float dw = wT - wP, dh = hT - hP;
            const float dtr = 0.25f * (dw * (wT + wP) + dh * (hT + hP)), cross = wP * dh - hP * dw;
            const float num = dtr * dtr + 0.25f * cross * cross + 4.0f * s2 * (AP - BP) * (AT - BT);
            whr = num * rcp_nr((AP + BP) + (AT + BT) + 2.0f * S);
        }
        const float d2 = (dx * dx + dy * dy) + p.alpha * p.alpha * whr;
        const float Dd = sqrt_floor(d2, 1e-7f, pd);
        float d = Dd, norm = 1.0f, r1 = 1.0f, r2 = 1.0f;
        bool p1 = true, p2 = true, p3 = true;
        const bool normalize = p.opts & GOPT_NORMALIZE;
        if (normalize) {   // 2 * sqrt(max(sqrt(max(t, 1e-7)), 1e-7)).clamp(1e-7)
            r1 = sqrt_floor(t, 1e-7f, p1);
            r2 = sqrt_floor(r1, 1e-7f, p2);
            p3 = r2 >= 1e-7f;
            norm = 2.0f * fmaxf(r2, 1e-7f);
            d = Dd * rcp_nr(norm);
        }
        float gd;
        loss = gauss_post(d, p.fun, p.tau, gd);
        if (BWD) {
            float gDd = gd, gt = 0.0f;
            if (normalize) {
                gDd = gd * rcp_nr(norm);
                const float gnorm = -gDd * Dd * rcp_nr(norm);
                // d norm / d t = 2 * (1 / (2 r2)) * (1 / (2 r1)), gated
                if (p1 && p2 && p3) gt += gnorm * 0.5f * rcp_nr(r1 * r2);
            }
            const float gd2 = pd ? gDd * 0.5f * rcp_nr(Dd) : 0.0f;
            gdx = 2.0f * dx * gd2;
            const float gwhr = p.alpha * p.alpha * gd2;
            gAP = gBP = gAT = gBT = gwhr;
            const float gR = pr ? -gwhr * rcp_nr(S) : 0.0f;   // whr = ... - 2 S
            gt += 2.0f * gR;
            const float gtarg = pt ? gt * 0.5f * rcp_nr(t) : 0.0f;
            gAP += gtarg * BP * detT + gR * (AT * c2 + BT * s2);
            gBP += gtarg * AP * detT + gR * (BT * c2 + AT * s2);
            gAT += gtarg * BT * detP + gR * (AP * c2 + BP * s2);
            gBT += gtarg * AT * detP + gR * (BP * c2 + AP * s2);
            gD = gR * 2.0f * cs * (AP - BP) * (BT - AT);
        }
    } else {   // kld family: P is the reference Gaussian of kld(P, T)
        const float ia2 = 1.0f / (p.alpha * p.alpha);
        const bool sq = p.opts & GOPT_SQRT;
        const float ca = f.ca, sa = f.sa, cb = f.cb, sb = f.sb;
        const float uP = dx * ca + dy * sa, vP = dy * ca - dx * sa;   // centre offset in P's axes
        const float uT = dx * cb + dy * sb, vT = dy * cb - dx * sb;   // ... in T's axes
        // differences of the covariances' eigenvalues, from the differences of the extents
        const float dA = 0.25f * (wT - wP) * (wT + wP), dB = 0.25f * (hT - hP) * (hT + hP);          // A_T - A_P, B_T - B_P
        const float eP = 0.25f * (hP - wP) * (hP + wP), eT = 0.25f * (hT - wT) * (hT + wT);          // B_P - A_P, B_T - A_T
        const float kPT = kld_raw(AP, BP, dA, dB, eT, eP, uP, vP, s2, ia2);
        const float kTP = p.type == GAUSS_KLD ? 0.0f : kld_raw(AT, BT, -dA, -dB, eP, eT, uT, vT, s2, ia2);
        float d, gPT = 0.0f, gTP = 0.0f;   // d(d) / d(kPT), d(d) / d(kTP)
        if (p.type == GAUSS_KLD || p.type == GAUSS_JD) {
            const float r = p.type == GAUSS_KLD ? kPT : 0.5f * (kPT + kTP);
            const float gr = p.type == GAUSS_KLD ? 1.0f : 0.5f;
            d = r;
            float gs = 1.0f;
            if (sq) { bool ps; d = sqrt_floor(r, 1e-7f, ps); gs = ps ? 0.5f * rcp_nr(d) : 0.0f; }
            gPT = gr * gs;
            gTP = p.type == GAUSS_KLD ? 0.0f : gr * gs;
        } else {
            float s1 = kPT, s2v = kTP, g1 = 1.0f, g2 = 1.0f;
            if (sq) {
                bool ps1, ps2;
                s1 = sqrt_floor(kPT, 1e-7f, ps1); g1 = ps1 ? 0.5f * rcp_nr(s1) : 0.0f;
                s2v = sqrt_floor(kTP, 1e-7f, ps2); g2 = ps2 ? 0.5f * rcp_nr(s2v) : 0.0f;
            }
            const bool mx = p.type == GAUSS_KLD_SYMMAX;
            d = mx ? fmaxf(s1, s2v) : fminf(s1, s2v);
            // torch.maximum / torch.minimum split the gradient evenly on a tie
            const float w1 = s1 == s2v ? 0.5f : ((s1 > s2v) == mx ? 1.0f : 0.0f);
            gPT = w1 * g1;
            gTP = (1.0f - w1) * g2;
        }
        float gd;
        loss = gauss_post(d, p.fun, p.tau, gd);
        if (BWD) {
            if (gPT != 0.0f)
                kld_raw_adj(gd * gPT, AP, BP, AT, BT, dA, dB, eT, eP, uP, vP, ca, sa, s2, cs, ia2, gAP, gBP, gAT, gBT, gdx, gaP, gD);
            if (gTP != 0.0f) {
                float gDtp = 0.0f;   // d/d(a_T - a_P)
                kld_raw_adj(gd * gTP, AT, BT, AP, BP, -dA, -dB, eP, eT, uT, vT, cb, sb, s2, -cs, ia2, gAT, gBT, gAP, gBP, gdx, gaT,
                            gDtp);
                gD -= gDtp;
            }
        }
    }
    if (!BWD) return loss;
    // A = w^2 / 4: dA/dw = w / 2; the clamp of w passes the gradient on [1e-7, 1e7]
    const bool gwP = f.wg >= 1e-7f && f.wg <= 1e7f, ghP = f.hg >= 1e-7f && f.hg <= 1e7f;
    const bool gwT = f.wp >= 1e-7f && f.wp <= 1e7f, ghT = f.hp >= 1e-7f && f.hp <= 1e7f;
    gP = PlanarGrad{-gdx, gwP ? 0.5f * wP * gAP : 0.0f, ghP ? 0.5f * hP * gBP : 0.0f, gD + gaP};
    gT = PlanarGrad{gdx, gwT ? 0.5f * wT * gAT : 0.0f, ghT ? 0.5f * hT * gBT : 0.0f, gaT - gD};
    return loss;
}

// Per-pair Gaussian loss element; when BWD, also d(loss)/d(pred[0..DIM)) and d(loss)/d(target[0..DIM)) in 1/degree.
// Reference-order arithmetic (FAST false): the VALUE is the body on the reference-order planar boxes, the reference's own
// float32 roundings.  The GRADIENT is the adjoint on the closed-form front end's boxes: the reference-order centres come out of
// acos(cos(A / 2)) in float32, where one ulp of the cosine moves a centre distance of half a degree by 0.25 % and the extent
// columns of a converged pair, which are differences of such terms, by several percent; a gradient has no roundings to reproduce.
template <int DIM, bool BWD, bool FAST>
SPH_DEV float pair_gauss_loss(const float (&pred)[5], const float (&target)[5], const GaussBody& p, float (&gpred)[5],
                              float (&gtarget)[5]) {
    if (pair_has_nan<DIM>(pred, target)) {   // a NaN coordinate: NaN loss and NaN gradients for the pair (as pair_loss)
        const float qnan = __builtin_nanf("");
#pragma unroll
        for (int k = 0; k < 5; k++) { gpred[k] = k < DIM ? qnan : 0.0f; gtarget[k] = k < DIM ? qnan : 0.0f; }
        return qnan;
    }
    float b1[5], b2[5];
#pragma unroll
    for (int k = 0; k < 5; k++) { b1[k] = pred[k]; b2[k] = target[k]; }
    jitter_spherical<DIM>(b1, b2);
    LossFront f;
    PlanarGrad gP{0, 0, 0, 0}, gT{0, 0, 0, 0};
    float loss;
    if (FAST) {
        loss_front_fast<DIM>(b1, b2, f);
        loss = gauss_body<BWD>(f, p, gP, gT);
    } else {
        loss_front_reference<DIM>(b1, b2, f);
        loss = gauss_body<false>(f, p, gP, gT);
        if (BWD) {
            loss_front_fast<DIM>(b1, b2, f);
            gauss_body<true>(f, p, gP, gT);
        }
    }
    if (!BWD) return loss;
    planar_to_spherical_grads<DIM>(f, gP, gT, /*x_split=*/0.5f, pred, target, /*jitter=*/true, EDGE_ARC, gpred, gtarget);
    return loss;
}

template <int DIM, bool BWD, bool FAST>
SPH_DEV float GaussBody::eval(const float (&pred)[5], const float (&target)[5], float*, float (&gpred)[5],
                              float (&gtarget)[5]) const {
    return pair_gauss_loss<DIM, BWD, FAST>(pred, target, *this, gpred, gtarget);
}

// The IoU family's trailing launcher parameters as a per-pair body (the kernels build it from the flat (loss_mode, eps) and
// call pair_loss themselves; the host twins' loss pass calls eval()).
struct IouBody {
    int loss_mode;
    float eps;
    template <int DIM, bool BWD, bool FAST>
    SPH_DEV float eval(const float (&pred)[5], const float (&target)[5], float* iou_out, float (&gpred)[5],
                       float (&gtarget)[5]) const {
        return pair_loss<DIM, BWD, FAST>(pred, target, loss_mode, eps, iou_out, gpred, gtarget);
    }
};

// ---- shared by the loss launchers (sph2pob_loss.hip) and their host twins (sph2pob_host.hip) ----
constexpr int64_t kMaxElems = (int64_t)1 << 38;  // grid.x = n / 256 must stay below 2^31

// per-element weight = mean over weight_dim columns (reference: sph2pob_transform.py:32-34 widens a (n,4) weight with its
// own mean, OBBIoULoss.forward then takes weight.mean(-1): sph2pob_iou_loss.py:48)
template <int DIM>
SPH_DEV float element_weight(const float* __restrict__ w, int wd, int64_t i) {
    if (!w) return 1.0f;
    if (wd == 1) return w[i];
    float v[DIM], s = 0.0f;   // wd == DIM here (the checks reject anything else): DIM loads in flight, not a loop of load + wait
#pragma unroll
    for (int k = 0; k < DIM; k++) v[k] = w[i * DIM + k];
#pragma unroll
    for (int k = 0; k < DIM; k++) s += v[k];
    if (DIM == 4) return (s + s / 4.0f) / 5.0f;
    return s / (float)DIM;
}

// argument checks of the IoU family: loss mode 0..3 (| SPH2POB_FLAG_REFERENCE_ORDER); the backward's grad_stride is
// checked with the mode (the other forms pass 0)
inline int loss_check(const float* weight, int weight_dim, int64_t n, int box_dim, int loss_mode_flags, int grad_stride = 0) {
    const int loss_mode = loss_mode_flags & 0xff;
    if (loss_mode_flags & ~(0xff | SPH2POB_FLAG_REFERENCE_ORDER)) return SPH2POB_ERR_OPTION;
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (loss_mode < 0 || loss_mode > 3 || (grad_stride != 0 && grad_stride != 1)) return SPH2POB_ERR_OPTION;
    if (weight && weight_dim != 1 && weight_dim != box_dim) return SPH2POB_ERR_OPTION;
    if (n < 0 || n > kMaxElems) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}

// argument checks of the Gaussian family: SPH2POB_GAUSS_* type (| SPH2POB_FLAG_REFERENCE_ORDER), a post-map the type
// accepts (GD: none | log1p | sqrt, KF: none | ln | exp), SPH2POB_GAUSS_OPT_* options
inline int gauss_check(const float* weight, int weight_dim, int64_t n, int box_dim, int type_flags, int fun, int opts) {
    const int type = type_flags & 0xff;
    if (type_flags & ~(0xff | SPH2POB_FLAG_REFERENCE_ORDER)) return SPH2POB_ERR_OPTION;
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (type < SPH2POB_GAUSS_GWD || type > SPH2POB_GAUSS_KF) return SPH2POB_ERR_OPTION;
    const bool fun_ok = type == SPH2POB_GAUSS_KF
                            ? (fun == SPH2POB_GAUSS_FUN_NONE || fun == SPH2POB_GAUSS_FUN_LN || fun == SPH2POB_GAUSS_FUN_EXP)
                            : (fun >= SPH2POB_GAUSS_FUN_NONE && fun <= SPH2POB_GAUSS_FUN_SQRT);
    if (!fun_ok || (opts & ~(SPH2POB_GAUSS_OPT_SQRT | SPH2POB_GAUSS_OPT_NORMALIZE))) return SPH2POB_ERR_OPTION;
    if (weight && weight_dim != 1 && weight_dim != box_dim) return SPH2POB_ERR_OPTION;
    if (n < 0 || n > kMaxElems) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}

// argument checks of sph2pob_loss_grad_scale_f32
inline int grad_scale_check(int64_t n, int box_dim, int grad_stride) {
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (grad_stride != 0 && grad_stride != 1) return SPH2POB_ERR_OPTION;
    if (n < 0 || n > kMaxElems) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}

static_assert(SPH2POB_GAUSS_GWD == GAUSS_GWD && SPH2POB_GAUSS_KLD == GAUSS_KLD && SPH2POB_GAUSS_JD == GAUSS_JD &&
              SPH2POB_GAUSS_KLD_SYMMAX == GAUSS_KLD_SYMMAX && SPH2POB_GAUSS_KLD_SYMMIN == GAUSS_KLD_SYMMIN &&
              SPH2POB_GAUSS_KF == GAUSS_KF, "loss type codes");
static_assert(SPH2POB_GAUSS_FUN_NONE == GFUN_NONE && SPH2POB_GAUSS_FUN_LOG1P == GFUN_LOG1P && SPH2POB_GAUSS_FUN_SQRT == GFUN_SQRT &&
              SPH2POB_GAUSS_FUN_LN == GFUN_LN && SPH2POB_GAUSS_FUN_EXP == GFUN_EXP, "post-map codes");
static_assert(SPH2POB_GAUSS_OPT_SQRT == GOPT_SQRT && SPH2POB_GAUSS_OPT_NORMALIZE == GOPT_NORMALIZE, "option bits");

}  // namespace sph2pob
