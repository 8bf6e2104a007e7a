// The spherical RoI feature extractor (sph2pob_roi_extract_fwd_f32 / _bwd_f32, include/sph2pob_hip.h): what the kernels
// (sph2pob_roi_extract.hip) and the CPU twins (sph2pob_host.hip) share — the level table, the argument checks, the per-roi prepare
// step (the box transform of SphStandardRoIHead._bbox_forward, the clamp, the level rule of SingleRoIExtractor.map_roi_levels and
// the roi's sampling frame), the per-axis bilinear entry and the bin sums of RoIAlign — so that a CPU tensor gets the arithmetic and
// the checks a device tensor gets.  Everything here is fp32 in the order the header states, nothing is contracted.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"

#define SPHR_DEV __host__ __device__ __forceinline__

namespace sph2pob_roi {

constexpr int kMaxLevels = 8;
constexpr int kMaxGrid = 1 << 15;   // samples per bin and axis: gh gw stays below 2^31 whatever the roi is
constexpr int kMaxPooled = 64;      // PH, PW
constexpr int kPrepWords = 8;       // the prepared record of a roi: 32 bytes

struct Level {
    const float* feat;   // (B, C, H, W)
    float* grad;         // the same shape, backward only
    int h, w;
    float scale;         // 1 / stride, rounded to fp32 once
};
struct Levels {
    Level lv[kMaxLevels];
    int num;
};

// The prepared record of a roi: its sampling frame on its level.  b < 0: the row holds zeros and takes no gradient
struct Prep {
    float sw, sh, bin_w, bin_h;
    int gw, gh, b, lvl;
};
static_assert(sizeof(Prep) == kPrepWords * 4, "a Prep is eight words");

struct Options {
    int box_dim, form;           // form 0: flat (N, 1 + dim) rows with the image index in front; 1: padded (B, M, >= dim)
    int64_t rows, m, row_stride;
    int num_images, channels;
    float img_h, img_w, finest_scale;
    int ph, pw, sampling_ratio, aligned;
};

SPHR_DEV bool finite32(float v) { return v - v == 0.0f; }

// One axis of the clamped planar box: centre c, extent e, in pixels, clamped to [0, hi]
SPHR_DEV void span(float c, float e, float hi, float& lo_out, float& hi_out) {
    const float half = e / 2.0f;
    float a = c - half, b = c + half;
    a = a < 0.0f ? 0.0f : (a > hi ? hi : a);
    b = b < 0.0f ? 0.0f : (b > hi ? hi : b);
    lo_out = a;
    hi_out = b;
}

// The level of a roi: the count of k in 1 .. L-1 with fl32(scale / finest_scale + 1e-6) >= 2^k — floor(log2(.)) clamped to
// [0, L-1] without a log2f (a NaN compares false: level 0)
SPHR_DEV int level_of(float x1, float y1, float x2, float y2, float finest_scale, int num_levels) {
    const float scale = sqrtf((x2 - x1) * (y2 - y1));
    const float t = scale / finest_scale + 1e-6f;
    int lvl = 0;
    float p = 2.0f;
    for (int k = 1; k < num_levels; k++, p *= 2.0f) lvl += t >= p ? 1 : 0;
    return lvl;
}

// The prepare step of row r.  Returns the record; xyxy gets the planar box the reference hands to RoIAlign (zeros for a refused row)
SPHR_DEV Prep prepare_row(const Levels& L, const Options& o, const float* __restrict__ rois, const int64_t* __restrict__ num_rois, int64_t r,
                          float* xyxy) {
    Prep p = {0.0f, 0.0f, 0.0f, 0.0f, 0, 0, -1, 0};
    xyxy[0] = xyxy[1] = xyxy[2] = xyxy[3] = 0.0f;
    const float* row = rois + r * o.row_stride;
    int b;
    if (o.form == 0) {
        const float bf = row[0];
        if (!(bf >= 0.0f && bf < (float)o.num_images) || bf != floorf(bf)) return p;
        b = (int)bf;
        row += 1;
    } else {
        b = (int)(r / o.m);
        if (num_rois) {   // the count clamped to [0, M]; the rows behind it are never read
            const int64_t n = num_rois[b];
            if (r - (int64_t)b * o.m >= (n < 0 ? 0 : n > o.m ? o.m : n)) return p;
        }
    }
    const float th = row[0], ph = row[1], al = row[2], be = row[3];
    const float ga = o.box_dim == 5 ? row[4] : 0.0f;
    if (!(finite32(th) && finite32(ph) && finite32(al) && finite32(be) && finite32(ga))) return p;
    const float x = th / 360.0f * o.img_w, y = ph / 180.0f * o.img_h;
    float w = al / 360.0f * o.img_w, h = be / 180.0f * o.img_h;
    if (o.box_dim == 5) {
        const float a = ga * 0.017453292519943295f;   // deg2rad: one fp32 product with fl32(pi / 180)
        const float ca = fabsf(cosf(a)), sa = fabsf(sinf(a));
        const float w2 = ca * w + sa * h, h2 = sa * w + ca * h;
        w = w2;
        h = h2;
    }
    float x1, y1, x2, y2;
    span(x, w, o.img_w, x1, x2);
    span(y, h, o.img_h, y1, y2);
    if (!(finite32(x1) && finite32(y1) && finite32(x2) && finite32(y2))) return p;   // an extent that overflowed to inf - inf
    xyxy[0] = x1; xyxy[1] = y1; xyxy[2] = x2; xyxy[3] = y2;
    const int lvl = L.num == 1 ? 0 : level_of(x1, y1, x2, y2, o.finest_scale, L.num);
    const float s = L.lv[lvl].scale, off = o.aligned ? 0.5f : 0.0f;
    const float sw = x1 * s - off, sh = y1 * s - off, ew = x2 * s - off, eh = y2 * s - off;
    float rw = ew - sw, rh = eh - sh;
    if (!o.aligned) {
        rw = rw > 1.0f ? rw : 1.0f;
        rh = rh > 1.0f ? rh : 1.0f;
    }
    const float bin_h = rh / (float)o.ph, bin_w = rw / (float)o.pw;
    float gh = o.sampling_ratio > 0 ? (float)o.sampling_ratio : ceilf(rh / (float)o.ph);
    float gw = o.sampling_ratio > 0 ? (float)o.sampling_ratio : ceilf(rw / (float)o.pw);
    gh = gh > 0.0f ? (gh < (float)kMaxGrid ? gh : (float)kMaxGrid) : 0.0f;
    gw = gw > 0.0f ? (gw < (float)kMaxGrid ? gw : (float)kMaxGrid) : 0.0f;
    p.sw = sw; p.sh = sh; p.bin_w = bin_w; p.bin_h = bin_h;
    p.gw = (int)gw; p.gh = (int)gh; p.b = b; p.lvl = lvl;
    return p;
}

// A record as a kernel may trust it: whatever the buffer holds, the level, the image and the grid are in range
SPHR_DEV Prep checked(Prep p, int num_levels, int num_images) {
    p.lvl = p.lvl < 0 ? 0 : (p.lvl >= num_levels ? num_levels - 1 : p.lvl);
    if (p.b >= num_images) p.b = -1;
    p.gw = p.gw < 0 ? 0 : (p.gw > kMaxGrid ? kMaxGrid : p.gw);
    p.gh = p.gh < 0 ? 0 : (p.gh > kMaxGrid ? kMaxGrid : p.gh);
    return p;
}

// One axis of a bilinear sample: the two pixel indices and their weights; lo < 0: the sample lies outside [-1, n] and adds nothing
struct Axis {
    int lo, hi;
    float l, h;   // the weights of hi and of lo
};

// sample i of bin q along an axis of n pixels: start + q bin + (i + .5) bin / g
SPHR_DEV Axis axis_entry(float start, float bin, int g, int q, int i, int n) {
    float y = start + (float)q * bin + ((float)i + 0.5f) * bin / (float)g;
    Axis a;
    if (!(y >= -1.0f && y <= (float)n)) {
        a.lo = -1; a.hi = 0; a.l = 0.0f; a.h = 0.0f;
        return a;
    }
    if (y <= 0.0f) y = 0.0f;
    int lo = (int)y, hi;
    if (lo >= n - 1) {
        hi = lo = n - 1;
        y = (float)lo;
    } else {
        hi = lo + 1;
    }
    a.lo = lo; a.hi = hi;
    a.l = y - (float)lo;
    a.h = 1.0f - a.l;
    return a;
}

SPHR_DEV float bin_count(const Prep& p) {
    const int c = p.gh * p.gw;
    return (float)(c > 1 ? c : 1);
}

// out[c, ph, pw] of a roi: the samples in (iy, ix) order, each hy hx v(lo, lo) + hy lx v(lo, hi) + ly hx v(hi, lo) + ly lx v(hi, hi)
// added left to right, then one division by the count.  `ay(k)` / `ax(k)` give entry k = q g + i of the axis
template <class AY, class AX>
SPHR_DEV float bin_forward(const float* __restrict__ plane, int w, const Prep& p, int ph, int pw, AY&& ay, AX&& ax) {
    float acc = 0.0f;
    for (int iy = 0; iy < p.gh; iy++) {
        const Axis y = ay(ph * p.gh + iy);
        if (y.lo < 0) continue;
        const float* r0 = plane + (int64_t)y.lo * w;
        const float* r1 = plane + (int64_t)y.hi * w;
        for (int ix = 0; ix < p.gw; ix++) {
            const Axis x = ax(pw * p.gw + ix);
            if (x.lo < 0) continue;
            const float w1 = y.h * x.h, w2 = y.h * x.l, w3 = y.l * x.h, w4 = y.l * x.l;
            acc += w1 * r0[x.lo] + w2 * r0[x.hi] + w3 * r1[x.lo] + w4 * r1[x.hi];
        }
    }
    return acc / bin_count(p);
}

// the adjoint: every term's weight times g = grad_out / count handed to add(pixel offset in the plane, value)
template <class AY, class AX, class ADD>
SPHR_DEV void bin_backward(int w, const Prep& p, int ph, int pw, float g, AY&& ay, AX&& ax, ADD&& add) {
    for (int iy = 0; iy < p.gh; iy++) {
        const Axis y = ay(ph * p.gh + iy);
        if (y.lo < 0) continue;
        const int64_t r0 = (int64_t)y.lo * w, r1 = (int64_t)y.hi * w;
        for (int ix = 0; ix < p.gw; ix++) {
            const Axis x = ax(pw * p.gw + ix);
            if (x.lo < 0) continue;
            add(r0 + x.lo, g * (y.h * x.h));
            add(r0 + x.hi, g * (y.h * x.l));
            add(r1 + x.lo, g * (y.l * x.h));
            add(r1 + x.hi, g * (y.l * x.l));
        }
    }
}

// ---- the gather form of the backward (sph2pob_roi_extract_bwd_det_f32_cpu in sph2pob_host.hip; no kernel computes it yet, the
// functions below are host and device alike so that one can): the adjoint as a per-pixel gather.  The bilinear weights are
// separable, so what roi r adds to pixel (y, x) of channel c is
//     t_r = sum over ph, then pw, of g[c, ph, pw] (Wy_r[ph, y] Wx_r[pw, x]),   g = grad_out / count (rounded once)
// with Wy_r[ph, y] the sum of the weights the samples iy = 0 .. gh - 1 of bin ph put on row y (each sample its lo term, then its hi
// term), Wx_r likewise.  Only the bins with at least one term on BOTH axes are summed (a bin that does not reach the pixel adds
// nothing, a non-finite grad_out there included), t_r starts at +0 and takes g (Wy Wx) left to right; the pixel's gradient starts at
// +0 and takes t_r of the rois of its (image, level) in ascending row index.  Every order is fixed: the same bits on every call.
// A pixel no roi reaches gets +0.0 (zero_first = 1) or keeps its value + 0.0.
// The bound against the float64 evaluation on the same fp32 weights, per pixel, barring underflow, with n the number of (roi, ph, pw)
// terms of the pixel and ty, tx the largest numbers of sample weights behind a Wy, Wx of those terms: a term carries one rounding of
// g, at most ty - 1 additions in Wy and tx - 1 in Wx (all weights are >= 0, so the relative bounds hold), one product Wy Wx, one
// product with g and at most n - 1 additions (the first term of a roi is added to +0, the first roi's t_r likewise: exact) —
// k = n + ty + tx roundings, (1 + u)^k - 1 <= k u / (1 - k u) <= (k + 1) u for k <= 4095, u = 2^-24:
//     |grad - f64| <= (n + max ty + max tx + 1) 2^-24 sum|terms|
// (zero_first = 0 adds the finished sum to the buffer's value: one more rounding, of that sum.) ----

// Wy[q, pix] of an axis of n pixels and its number of terms: the samples in ascending order, the lo term before the hi term
SPHR_DEV float axis_weight(float start, float bin, int g, int q, int n, int pix, int& terms) {
    float w = 0.0f;
    int t = 0;
    for (int i = 0; i < g; i++) {
        const Axis a = axis_entry(start, bin, g, q, i, n);
        if (a.lo < 0) continue;
        if (a.lo == pix) { w += a.h; t++; }
        if (a.hi == pix) { w += a.l; t++; }
    }
    terms = t;
    return w;
}

// one step of t_r
SPHR_DEV float gather_term(float t, float g, float wy, float wx) { return t + g * (wy * wx); }

// A range of pixels [lo, hi] of an axis of n pixels that holds every pixel the samples of `bins` bins can touch — a superset: the
// exact positions lie between start and start + bins bin, a sample's fp32 position is fewer than eight roundings of values up to
// |start| + |end| away, and it touches floor(.) and the pixel above.  Pixels outside take no term.  Only a speed-up: axis_weight
// decides what a pixel gets.  A NaN frame gives some range: no sample of it is valid
SPHR_DEV void axis_reach(float start, float bin, int bins, int n, int& lo, int& hi) {
    const float end = start + (float)bins * bin;
    const float m = 1.0f + (fabsf(start) + fabsf(end)) * 4.76837158203125e-07f;   // 2^-21
    float a = floorf((start < end ? start : end) - m), b = floorf((start < end ? end : start) + m) + 1.0f;
    const float top = (float)(n - 1);
    a = a > 0.0f ? (a < top ? a : top) : 0.0f;   // a NaN compares false: 0
    b = b > 0.0f ? (b < top ? b : top) : 0.0f;
    lo = (int)a;
    hi = (int)b;
}

// Argument checks of both entries up to the pointers, in the documented order; fills the level table
// (box_dim, the options, the sizes; an empty call — no rows, images or channels — is SPH2POB_OK with out->num = 0 whatever the
// pointers are; then the pointers).  `table` is the level table the entry reads or writes: features forward, gradients backward
inline int make_levels(float* const* table, bool is_grad, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                       int64_t num_images, int64_t channels, int box_dim, int pooled_h, int pooled_w, int64_t rows, Levels* out) {
    out->num = 0;
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (num_levels < 1 || num_levels > kMaxLevels || pooled_h < 1 || pooled_w < 1 || pooled_h > kMaxPooled || pooled_w > kMaxPooled)
        return SPH2POB_ERR_OPTION;
    if (rows < 0 || num_images < 0 || channels < 0 || rows > 0x7fffffff || num_images > (1 << 24) || channels > (1 << 20)) return SPH2POB_ERR_SIZE;
    if (rows == 0 || num_images == 0 || channels == 0) return SPH2POB_OK;
    if (!heights || !widths || !strides || !table) return SPH2POB_ERR_NULL;
    for (int l = 0; l < num_levels; l++) {
        if (!(strides[l] > 0.0f) || !finite32(strides[l])) return SPH2POB_ERR_OPTION;
        if (heights[l] < 1 || widths[l] < 1 || heights[l] > (1 << 20) || widths[l] > (1 << 20) ||
            num_images * channels * heights[l] * widths[l] > ((int64_t)1 << 40))
            return SPH2POB_ERR_SIZE;
        if (!table[l]) return SPH2POB_ERR_NULL;
        out->lv[l] = Level{is_grad ? nullptr : table[l], is_grad ? table[l] : nullptr, (int)heights[l], (int)widths[l],
                           (float)(1.0 / (double)strides[l])};
    }
    out->num = num_levels;
    return SPH2POB_OK;
}
// the options of the forward entry behind the level table: the roi form, the image, the sampling
inline int check_options(int form, int64_t m, int64_t row_stride, int64_t rows, int64_t num_images, int box_dim, int64_t img_h, int64_t img_w,
                         int sampling_ratio, int aligned, float finest_scale) {
    if (form < 0 || form > 1 || aligned < 0 || aligned > 1 || sampling_ratio < 0 || sampling_ratio > kMaxGrid || !(finest_scale > 0.0f) ||
        !finite32(finest_scale))
        return SPH2POB_ERR_OPTION;
    if (img_h < 1 || img_w < 1 || img_h > (1 << 24) || img_w > (1 << 24) || row_stride < box_dim + (form == 0 ? 1 : 0) || row_stride > (1 << 20))
        return SPH2POB_ERR_SIZE;
    if (form == 1 && rows > 0 && (m < 1 || m * num_images != rows)) return SPH2POB_ERR_SIZE;
    return SPH2POB_OK;
}

}  // namespace sph2pob_roi
