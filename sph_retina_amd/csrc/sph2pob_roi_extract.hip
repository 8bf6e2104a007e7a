// libsph2pob_hip.so — the spherical RoI feature extractor (sph2pob_roi_extract_fwd_f32 / _bwd_f32, include/sph2pob_hip.h): what
// SphStandardRoIHead._bbox_forward computes in front of the box head (sphdet/models/heads/sph_rcnn_head.py:211-230) — the sph2pix
// box transform, obb2hbb for RBFoV, the clamp to the image — and SingleRoIExtractor behind it (the level rule of map_roi_levels
// and mmcv's RoIAlign in 'avg' mode on the roi's level), for all rois of a minibatch with two launches forward and two backward,
// without a host read.  gfx950 only.
//
// Forward: roi_prepare_kernel (one thread per roi: the box, the level and the sampling frame, written to rois_xyxy / levels and
// kept as a 32-byte record for the backward), then roi_align_fwd_kernel.  The prepare step is a launch of its own and not the
// prologue of the align kernel: a roi is shared by C / kChannels workgroups, which would each redo it (the RBFoV sine and cosine
// included) and race on the roi's row of rois_xyxy, and the backward wants the record without the rois.
//
// The align kernels: a workgroup owns a roi and kChannels channels.  The bilinear weights are separable — a sample's row index and
// weights depend on (ph, iy) alone, its column's on (pw, ix) — so the roi needs PH gh + PW gw axis entries, not PH PW gh gw sample
// records: they are computed once into LDS when they fit kAxisCap (16 KiB; 37 samples per bin and axis at 7 x 7 fit eight times
// over) and recomputed per use otherwise, the same function either way.  The threads then walk (channel, bin) with the bin
// fastest: neighbouring lanes read neighbouring pixels of one plane and store the roi's C PH PW contiguous floats coalesced, each
// once.  Forward sums in a fixed order: the same bits on every call.  Backward adds with fp32 atomics — in LDS over the roi's
// footprint where that fits kTileFloats, then one global add per touched pixel; straight into memory otherwise: the order is not
// fixed.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/sph2pob_hip.h"
#include "sph2pob_head_loss.hpp"
#include "sph2pob_roi_extract.hpp"

namespace {

using namespace sph2pob_roi;

constexpr int kBlock = sph2pob_head::kBlock;
constexpr int kChannels = 64;     // channels of a workgroup: 64 x 49 outputs, 12 or 13 per thread
constexpr int kAxisCap = 1024;    // axis entries held in LDS (16 bytes each)
constexpr int kTileFloats = 8192; // the backward's LDS accumulator: a roi's footprint times a group of channels (32 KiB)

__global__ __launch_bounds__(kBlock) void roi_prepare_kernel(Levels L, Options o, const float* __restrict__ rois, const int64_t* __restrict__ num_rois,
                                                           float* __restrict__ rois_xyxy, int32_t* __restrict__ levels, Prep* __restrict__ prep) {
    const int64_t r = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (r >= o.rows) return;
    float box[4];
    const Prep p = prepare_row(L, o, rois, num_rois, r, box);
    prep[r] = p;
    for (int k = 0; k < 4; k++) rois_xyxy[r * 4 + k] = box[k];
    levels[r] = p.lvl;
}

// The axis entries of the workgroup's roi: in LDS (`cached`) or recomputed
struct AxisTable {
    const Axis* lds;
    float start, bin;
    int g, n;
    bool cached;
    __device__ __forceinline__ Axis operator()(int k) const {
        if (cached) return lds[k];
        const int q = k / g;
        return axis_entry(start, bin, g, q, k - q * g, n);
    }
};

// fills the tables of roi p on a (h, w) plane; every thread of the workgroup calls it (one barrier inside)
__device__ __forceinline__ void make_tables(const Prep& p, int ph, int pw, int h, int w, Axis* lds, AxisTable& ty, AxisTable& tx) {
    const int ny = ph * p.gh, nx = pw * p.gw;
    const bool cached = (int64_t)ny + nx <= kAxisCap;
    ty = AxisTable{lds, p.sh, p.bin_h, p.gh > 0 ? p.gh : 1, h, cached};
    tx = AxisTable{lds + (cached ? ny : 0), p.sw, p.bin_w, p.gw > 0 ? p.gw : 1, w, cached};
    if (cached) {
        for (int k = threadIdx.x; k < ny + nx; k += kBlock) {
            if (k < ny) {
                const int q = k / p.gh;
                lds[k] = axis_entry(p.sh, p.bin_h, p.gh, q, k - q * p.gh, h);
            } else {
                const int j = k - ny, q = j / p.gw;
                lds[k] = axis_entry(p.sw, p.bin_w, p.gw, q, j - q * p.gw, w);
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kBlock) void roi_align_fwd_kernel(Levels L, int num_images, int channels, int ph, int pw, const Prep* __restrict__ prep,
                                                             float* __restrict__ out) {
    __shared__ Axis lds[kAxisCap];
    const int64_t r = blockIdx.x;
    const int c0 = (int)blockIdx.y * kChannels;
    const int nc = channels - c0 < kChannels ? channels - c0 : kChannels;
    const int bins = ph * pw, total = nc * bins;
    float* o = out + (r * channels + c0) * (int64_t)bins;
    const Prep p = checked(prep[r], L.num, num_images);
    if (p.b < 0 || p.gh == 0 || p.gw == 0) {   // a refused row, a row behind the count, a roi without extent: zeros
        for (int i = threadIdx.x; i < total; i += kBlock) o[i] = 0.0f;
        return;
    }
    const Level lv = L.lv[p.lvl];
    AxisTable ty, tx;
    make_tables(p, ph, pw, lv.h, lv.w, lds, ty, tx);
    const int64_t plane = (int64_t)lv.h * lv.w;
    const float* base = lv.feat + ((int64_t)p.b * channels + c0) * plane;
    for (int i = threadIdx.x; i < total; i += kBlock) {
        const int c = i / bins, bin = i - c * bins;
        const int y = bin / pw, x = bin - y * pw;
        o[i] = bin_forward(base + c * plane, lv.w, p, y, x, ty, tx);
    }
}

__global__ __launch_bounds__(kBlock) void roi_align_bwd_kernel(Levels L, int num_images, int channels, int ph, int pw, const Prep* __restrict__ prep,
                                                             const float* __restrict__ grad_out) {
    __shared__ Axis lds[kAxisCap];
    __shared__ float tile[kTileFloats];
    __shared__ int box[4];
    const int64_t r = blockIdx.x;
    const int c0 = (int)blockIdx.y * kChannels;
    const int nc = channels - c0 < kChannels ? channels - c0 : kChannels;
    const int bins = ph * pw, total = nc * bins;
    const Prep p = checked(prep[r], L.num, num_images);
    if (p.b < 0 || p.gh == 0 || p.gw == 0) return;
    const Level lv = L.lv[p.lvl];
    AxisTable ty, tx;
    make_tables(p, ph, pw, lv.h, lv.w, lds, ty, tx);
    const int64_t plane = (int64_t)lv.h * lv.w;
    const float* go = grad_out + (r * channels + c0) * (int64_t)bins;
    float* base = lv.grad + ((int64_t)p.b * channels + c0) * plane;
    const float count = bin_count(p);
    // The roi's footprint on its plane, from the cached entries: rows [y0, y0 + fh), columns [x0, x0 + fw).  When it fits the tile,
    // the terms of a group of channels are added in LDS and every touched pixel gets ONE global add, in rows of fw contiguous floats
    // — 49 gh gw 4 terms per channel become at most fh fw adds.  Every bound below is workgroup-uniform.
    bool tiled = false;
    int y0 = 0, x0 = 0, fh = 0, fw = 0;
    if (ty.cached) {
        if (threadIdx.x == 0) { box[0] = 0x7fffffff; box[1] = -1; box[2] = 0x7fffffff; box[3] = -1; }
        __syncthreads();
        const int ny = ph * p.gh, nx = pw * p.gw;
        for (int k = threadIdx.x; k < ny + nx; k += kBlock) {
            const Axis a = lds[k];
            if (a.lo < 0) continue;
            atomicMin(&box[k < ny ? 0 : 2], a.lo);
            atomicMax(&box[k < ny ? 1 : 3], a.hi);
        }
        __syncthreads();
        y0 = box[0]; fh = box[1] - y0 + 1; x0 = box[2]; fw = box[3] - x0 + 1;
        if (fh <= 0 || fw <= 0) return;   // no sample inside the plane: nothing to add
        tiled = (int64_t)fh * fw <= kTileFloats;
    }
    if (!tiled) {
        for (int i = threadIdx.x; i < total; i += kBlock) {
            const int c = i / bins, bin = i - c * bins;
            const int y = bin / pw, x = bin - y * pw;
            float* g = base + c * plane;
            bin_backward(lv.w, p, y, x, go[i] / count, ty, tx, [g](int64_t at, float v) { atomicAdd(g + at, v); });
        }
        return;
    }
    const int area = fh * fw, group = kTileFloats / area, origin = y0 * fw + x0;
    for (int c1 = 0; c1 < nc; c1 += group) {
        const int ng = nc - c1 < group ? nc - c1 : group;
        for (int i = threadIdx.x; i < ng * area; i += kBlock) tile[i] = 0.0f;
        __syncthreads();
        for (int i = threadIdx.x; i < ng * bins; i += kBlock) {
            const int c = i / bins, bin = i - c * bins;
            const int y = bin / pw, x = bin - y * pw;
            float* t = tile + c * area;
            bin_backward(fw, p, y, x, go[(c1 + c) * bins + bin] / count, ty, tx, [t, origin](int64_t at, float v) { atomicAdd(t + (at - origin), v); });
        }
        __syncthreads();
        for (int i = threadIdx.x; i < ng * area; i += kBlock) {
            const float v = tile[i];
            if (v == 0.0f) continue;
            const int c = i / area, rem = i - c * area;
            const int yy = rem / fw, xx = rem - yy * fw;
            atomicAdd(base + (c1 + c) * plane + (int64_t)(y0 + yy) * lv.w + (x0 + xx), v);
        }
        __syncthreads();
    }
}

// the gradient buffers of all levels in one launch: level l holds n[l] floats
struct ZeroTable {
    float* p[kMaxLevels];
    int64_t end[kMaxLevels];   // running totals
    int num;
};
__global__ __launch_bounds__(kBlock) void roi_zero_kernel(ZeroTable z) {
    const int64_t total = z.end[z.num - 1];
    for (int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x; i < total; i += (int64_t)gridDim.x * kBlock) {
        int l = 0;
        while (l < z.num - 1 && i >= z.end[l]) l++;
        z.p[l][i - (l ? z.end[l - 1] : 0)] = 0.0f;
    }
}

dim3 align_grid(int64_t rows, int64_t channels) { return dim3((unsigned)rows, (unsigned)((channels + kChannels - 1) / kChannels)); }

}  // namespace

extern "C" {

int sph2pob_roi_extract_fwd_f32(const float* const* feats, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                                int64_t num_images, int64_t channels, const float* rois, int64_t rows, int64_t row_stride, int form, int64_t m,
                                const int64_t* num_rois, int box_dim, int64_t img_h, int64_t img_w, int pooled_h, int pooled_w,
                                int sampling_ratio, int aligned, float finest_scale, float* roi_feats, float* rois_xyxy, int32_t* levels,
                                void* prep, void* stream) {
    if (box_dim != 4 && box_dim != 5) return SPH2POB_ERR_DIM;
    if (int rc = check_options(form, m, row_stride, rows, num_images, box_dim, img_h, img_w, sampling_ratio, aligned, finest_scale)) return rc;
    Levels L;
    if (int rc = make_levels(const_cast<float* const*>(feats), false, heights, widths, strides, num_levels, num_images, channels, box_dim, pooled_h,
                             pooled_w, rows, &L))
        return rc;
    if (L.num == 0) return SPH2POB_OK;
    if (!rois || !roi_feats || !rois_xyxy || !levels || !prep) return SPH2POB_ERR_NULL;
    const Options o{box_dim, form, rows, form == 1 ? m : 1, row_stride, (int)num_images, (int)channels, (float)img_h, (float)img_w, finest_scale,
                    pooled_h, pooled_w, sampling_ratio, aligned};
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(roi_prepare_kernel, dim3((unsigned)((rows + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, L, o, rois, num_rois, rois_xyxy, levels,
                       static_cast<Prep*>(prep));
    if (int rc = launch_status()) return rc;
    hipLaunchKernelGGL(roi_align_fwd_kernel, align_grid(rows, channels), dim3(kBlock), 0, s, L, (int)num_images, (int)channels, pooled_h, pooled_w,
                       static_cast<const Prep*>(prep), roi_feats);
    return launch_status();
}

int sph2pob_roi_extract_bwd_f32(float* const* grad_feats, const int64_t* heights, const int64_t* widths, const float* strides, int num_levels,
                                int64_t num_images, int64_t channels, const float* grad_out, int64_t rows, int box_dim, int pooled_h, int pooled_w,
                                const void* prep, int zero_first, void* stream) {
    if (zero_first < 0 || zero_first > 1) return (box_dim != 4 && box_dim != 5) ? SPH2POB_ERR_DIM : SPH2POB_ERR_OPTION;
    Levels L;
    if (int rc = make_levels(grad_feats, true, heights, widths, strides, num_levels, num_images, channels, box_dim, pooled_h, pooled_w, rows, &L))
        return rc;
    if (L.num == 0) return SPH2POB_OK;   // an empty call enqueues nothing, the zeroing included
    if (!grad_out || !prep) return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    if (zero_first) {
        ZeroTable z;
        z.num = L.num;
        int64_t total = 0;
        for (int l = 0; l < L.num; l++) {
            z.p[l] = L.lv[l].grad;
            total += num_images * channels * L.lv[l].h * L.lv[l].w;
            z.end[l] = total;
        }
        const int64_t want = (total + kBlock - 1) / kBlock, cap = (int64_t)cu_count() * 16;
        hipLaunchKernelGGL(roi_zero_kernel, dim3((unsigned)(want < cap ? want : cap)), dim3(kBlock), 0, s, z);
        if (int rc = launch_status()) return rc;
    }
    hipLaunchKernelGGL(roi_align_bwd_kernel, align_grid(rows, channels), dim3(kBlock), 0, s, L, (int)num_images, (int)channels, pooled_h, pooled_w,
                       static_cast<const Prep*>(prep), grad_out);
    return launch_status();
}

}  // extern "C"
