// Point targets for a minibatch of an anchor-free (FCOS) head and the distance-point coder (the arithmetic, the checks and the
// workspace: sph2pob_point_targets.hpp).  Two launches whatever B is, no host read, no allocation: capturable.
//   point_targets_kernel  grid (workgroups of an image, B), one lane per (image, point).  The image's GT rows are converted to pixel
//                         corners once per workgroup, one row per thread, into an LDS tile of kTile rows (corners as one 16-byte
//                         slot, area and angle as one 8-byte slot: a ds_read_b128 and a ds_read_b64 per row, every lane the same
//                         address, which the LDS broadcasts), and the image is walked tile by tile, so any GT count works.  A
//                         lane keeps the winner so far in registers; its label is the one global read at the end.  The level of a
//                         point comes from the table by value, its row from an LDS copy of the table (one 16-byte read per lane).
//                         dim 4 targets leave in one 16-byte store when the base allows.
//                         Thread 0 writes the workgroup's positives (int) and its centerness sum (double) into the workspace.
//   point_final_kernel    one workgroup: num_pos of every image and the two normalisers from the partials, in one fixed order.
// No float atomics and no global counters: the same bits on every call.
#include "sph2pob_point_targets.hpp"

namespace {

using namespace sph2pob_point;

struct Outputs {
    int64_t* labels; int64_t* gt_inds; float* bbox_targets; float* centerness;
};

template <int DIM, bool CENTER, bool VEC>
__global__ __launch_bounds__(kBlock) void point_targets_kernel(const float* __restrict__ points, int P, Levels L, const float* __restrict__ gt,
                                                               const int64_t* __restrict__ gt_labels, const int64_t* __restrict__ gt_offsets,
                                                               int64_t num_gt, int64_t k_max, float img_w, float img_h, int64_t num_classes, Outputs O,
                                                               double* __restrict__ sums, int* __restrict__ counts) {
    __shared__ float4 s_box[kTile];
    __shared__ float2 s_aa[kTile];   // (area, angle)
    const int b = blockIdx.y, tid = threadIdx.x;
    const int p = blockIdx.x * kBlock + tid;
    const bool live = p < P;
    const int64_t off = gt_offsets[b];
    const int k = image_rows(off, gt_offsets[b + 1], num_gt, k_max);   // workgroup-uniform

    // the level table into LDS by constant indices, then one 16-byte read per lane at the lane's level
    __shared__ float4 s_level[kMaxLevels];
    if (tid == 0) {
#pragma unroll
        for (int q = 0; q < kMaxLevels; q++) s_level[q] = make_float4(L.lo[q], L.hi[q], L.extent[q], L.norm[q]);
    }
    __syncthreads();
    float x = 0.0f, y = 0.0f, lo = 0.0f, hi = 0.0f, extent = 0.0f, norm = 0.0f;
    if (live) {
        const float4 lv = s_level[level_index(L, p)];   // 0 .. kMaxLevels - 1 by construction
        x = points[2 * (int64_t)p]; y = points[2 * (int64_t)p + 1];
        lo = lv.x; hi = lv.y; extent = lv.z; norm = lv.w;
    }
    Best best = no_best();
    for (int j0 = 0; j0 < k; j0 += kTile) {   // whole workgroups: barriers inside
        const int m = k - j0 < kTile ? k - j0 : kTile;
        if (j0 > 0) __syncthreads();          // the previous tile has been read
        if (tid < m) {
            const Gt g = gt_pixels(gt + (off + j0 + tid) * DIM, DIM, img_w, img_h);
            s_box[tid] = make_float4(g.x1, g.y1, g.x2, g.y2);
            s_aa[tid] = make_float2(g.area, g.angle);
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < m; j++) {
                const float4 c = s_box[j];
                const float2 a = s_aa[j];
                const Gt g{c.x, c.y, c.z, c.w, a.x, a.y};
                offer(best, g, j0 + j, candidate<CENTER>(g, x, y, lo, hi, extent));
            }
        }
    }

    float t[5];
    float cent = 0.0f;
    int pos = 0;
    if (live) {
        cent = target_row<DIM>(best, x, y, norm, t);
        pos = best.idx >= 0 ? 1 : 0;
        const int64_t r = (int64_t)b * P + p;
        O.labels[r] = pos ? gt_labels[off + best.idx] : num_classes;
        O.gt_inds[r] = (int64_t)(best.idx + 1);
        O.centerness[r] = cent;
        if (VEC) {
            reinterpret_cast<float4*>(O.bbox_targets)[r] = make_float4(t[0], t[1], t[2], t[3]);
        } else {
#pragma unroll
            for (int c = 0; c < DIM; c++) O.bbox_targets[r * DIM + c] = t[c];
        }
    }
    // the workgroup's partials: positives by ballot, the centerness in double in one fixed order
    __shared__ int s_pos[kBlock / 64];
    const int wave_pos = (int)__popcll(__ballot(pos != 0));
    if ((tid & 63) == 0) s_pos[tid >> 6] = wave_pos;
    const double sum = block_sum_f64((double)cent);   // (its barrier also publishes s_pos)
    if (tid == 0) {
        int n = 0;
#pragma unroll
        for (int wv = 0; wv < kBlock / 64; wv++) n += s_pos[wv];
        const int64_t slot = (int64_t)b * gridDim.x + blockIdx.x;
        sums[slot] = sum;
        counts[slot] = n;
    }
}

// num_pos[b] = the image's positives; avg_factor and centerness_denorm from the totals.  Thread t owns images t, t + 256, ...  and
// partials t, t + 256, ...: one order, whatever the machine does
__global__ __launch_bounds__(kBlock) void point_final_kernel(const double* __restrict__ sums, const int* __restrict__ counts, int B, int per_image,
                                                             int64_t* __restrict__ num_pos, float* __restrict__ avg_factor,
                                                             float* __restrict__ centerness_denorm) {
    __shared__ int64_t s_tot[kBlock / 64];
    int64_t tot = 0;
    for (int b = threadIdx.x; b < B; b += kBlock) {
        int64_t n = 0;
        for (int i = 0; i < per_image; i++) n += counts[(int64_t)b * per_image + i];
        num_pos[b] = n;
        tot += n;
    }
    double acc = 0.0;
    const int64_t nb = (int64_t)B * per_image;
    for (int64_t i = threadIdx.x; i < nb; i += kBlock) acc += sums[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) tot += __shfl_down(tot, o, 64);
    if ((threadIdx.x & 63) == 0) s_tot[threadIdx.x >> 6] = tot;
    const double r = block_sum_f64(acc);   // (its barrier also publishes s_tot)
    if (threadIdx.x == 0) {
        tot = 0;
#pragma unroll
        for (int wv = 0; wv < kBlock / 64; wv++) tot += s_tot[wv];
        normalisers(tot, r, avg_factor, centerness_denorm);
    }
}

// ---- the coder: one lane per row ----------------------------------------------------------------------------------------------------
template <int DIM>
__device__ __forceinline__ void load_row(const float* __restrict__ p, int64_t i, bool vec, float (&v)[5]) {
    if (DIM == 4 && vec) {
        const float4 q = reinterpret_cast<const float4*>(p)[i];
        v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w; v[4] = 0.0f;
    } else {
#pragma unroll
        for (int c = 0; c < 5; c++) v[c] = c < DIM ? p[i * DIM + c] : 0.0f;
    }
}

template <int DIM>
__device__ __forceinline__ void store_row(float* __restrict__ p, int64_t i, bool vec, const float (&v)[5]) {
    if (DIM == 4 && vec) {
        reinterpret_cast<float4*>(p)[i] = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int c = 0; c < DIM; c++) p[i * DIM + c] = v[c];
    }
}

// MODE 0: encode (`a` the GT), 1: decode (`a` the distances), 2: decode backward (`a` the distances, `g` the boxes' gradient)
template <int DIM, int MODE>
__global__ __launch_bounds__(kBlock) void point_coder_kernel(const float* __restrict__ points, const float* __restrict__ a, const float* __restrict__ g,
                                                             float* __restrict__ out, int n, Image im, int clamp, float clamp_hi, bool vec) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float pt[2] = {points[2 * (int64_t)i], points[2 * (int64_t)i + 1]};
    float row[5], gb[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f}, r[5];
    load_row<DIM>(a, i, vec, row);
    if (MODE == 0) {
        encode_row<DIM>(pt, row, im, clamp != 0, clamp_hi, r);
    } else if (MODE == 1) {
        decode_row<DIM, false>(pt, row, nullptr, im, r);
    } else {
        load_row<DIM>(g, i, vec, gb);
        decode_row<DIM, true>(pt, row, gb, im, r);
    }
    store_row<DIM>(out, i, vec, r);
}

template <int MODE>
int launch_coder(const float* points, const float* a, const float* g, float* out, int64_t n, int box_dim, const Image& im, int clamp, float clamp_hi,
                 void* stream) {
    if (n == 0) return SPH2POB_OK;
    const bool vec = aligned_to(a, 16) && aligned_to(out, 16) && (MODE != 2 || aligned_to(g, 16));
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (box_dim == 4) hipLaunchKernelGGL((point_coder_kernel<4, MODE>), grid, dim3(kBlock), 0, (hipStream_t)stream, points, a, g, out, (int)n, im, clamp, clamp_hi, vec);
    else hipLaunchKernelGGL((point_coder_kernel<5, MODE>), grid, dim3(kBlock), 0, (hipStream_t)stream, points, a, g, out, (int)n, im, clamp, clamp_hi, vec);
    return launch_status();
}

}  // namespace

extern "C" {

int64_t sph2pob_point_targets_workspace_bytes(int64_t num_images, int64_t num_points) { return workspace_bytes(num_images, num_points); }

int sph2pob_point_targets_f32(const float* points, int64_t num_points, const int64_t* level_n, const float* range_lo, const float* range_hi,
                              const float* sample_extent, const float* norm_stride, int num_levels, const float* gt, const int64_t* gt_labels,
                              const int64_t* gt_offsets, int64_t num_images, int64_t num_gt, int64_t k_max, int box_dim, int64_t img_h,
                              int64_t img_w, int64_t num_classes, int flags, int64_t* labels, int64_t* gt_inds, float* bbox_targets,
                              float* centerness, int64_t* num_pos, float* avg_factor, float* centerness_denorm, void* workspace, void* stream) {
    if (int rc = check_shape(num_points, level_n, num_levels, num_images, num_gt, k_max, box_dim, img_h, img_w, num_classes)) return rc;
    const int64_t rows = num_images * num_points;
    if (!range_lo || !range_hi || ((flags & SPH2POB_POINT_CENTER_SAMPLING) && !sample_extent) || ((flags & SPH2POB_POINT_NORM_ON_BBOX) && !norm_stride) ||
        !avg_factor || !centerness_denorm || (num_images > 0 && (!gt_offsets || !num_pos)) ||
        (rows > 0 && (!points || !labels || !gt_inds || !bbox_targets || !centerness || !workspace)) ||
        (rows > 0 && k_max > 0 && (!gt || !gt_labels))) return SPH2POB_ERR_NULL;
    Levels L;
    if (int rc = make_levels(level_n, range_lo, range_hi, sample_extent, norm_stride, num_levels, flags, &L)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const Workspace ws = rows > 0 ? carve(workspace, num_images, num_points) : Workspace{nullptr, nullptr};
    const int per_image = rows > 0 ? (int)blocks_per_image(num_points) : 0;
    if (rows > 0) {
        const Outputs O{labels, gt_inds, bbox_targets, centerness};
        const dim3 grid((unsigned)per_image, (unsigned)num_images);
        const bool center = (flags & SPH2POB_POINT_CENTER_SAMPLING) != 0, vec = box_dim == 4 && aligned_to(bbox_targets, 16);
        auto go = [&](auto kernel) {
            hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, points, (int)num_points, L, gt, gt_labels, gt_offsets, num_gt, k_max, (float)img_w,
                               (float)img_h, num_classes, O, ws.sums, ws.counts);
        };
        if (box_dim == 4) {
            if (center) { if (vec) go(point_targets_kernel<4, true, true>); else go(point_targets_kernel<4, true, false>); }
            else { if (vec) go(point_targets_kernel<4, false, true>); else go(point_targets_kernel<4, false, false>); }
        } else {
            if (center) go(point_targets_kernel<5, true, false>); else go(point_targets_kernel<5, false, false>);
        }
        if (int rc = launch_status()) return rc;
    }
    hipLaunchKernelGGL(point_final_kernel, dim3(1), dim3(kBlock), 0, s, ws.sums, ws.counts, (int)num_images, per_image, num_pos, avg_factor,
                       centerness_denorm);
    return launch_status();
}

int sph2pob_point_coder_encode_f32(const float* points, const float* gt, float* distances, int64_t n, int box_dim, int64_t img_h, int64_t img_w,
                                   int clamp, double max_dis, double eps, void* stream) {
    const float hi = clamp ? (float)(max_dis - eps) : 0.0f;
    if (int rc = check_coder(points, gt, gt, distances, n, box_dim, img_h, img_w, hi, 0.0f)) return rc;
    if (clamp != 0 && clamp != 1) return SPH2POB_ERR_OPTION;
    return launch_coder<0>(points, gt, nullptr, distances, n, box_dim, Image{(float)img_w, (float)img_h, -1.0f, -1.0f}, clamp, hi, stream);
}

int sph2pob_point_coder_decode_f32(const float* points, const float* distances, float* boxes, int64_t n, int box_dim, int64_t img_h, int64_t img_w,
                                   float max_h, float max_w, void* stream) {
    if (int rc = check_coder(points, distances, distances, boxes, n, box_dim, img_h, img_w, max_h, max_w)) return rc;
    return launch_coder<1>(points, distances, nullptr, boxes, n, box_dim, Image{(float)img_w, (float)img_h, max_w, max_h}, 0, 0.0f, stream);
}

int sph2pob_point_coder_decode_bwd_f32(const float* points, const float* distances, const float* grad_boxes, float* grad_distances, int64_t n,
                                       int box_dim, int64_t img_h, int64_t img_w, float max_h, float max_w, void* stream) {
    if (int rc = check_coder(points, distances, grad_boxes, grad_distances, n, box_dim, img_h, img_w, max_h, max_w)) return rc;
    return launch_coder<2>(points, distances, grad_boxes, grad_distances, n, box_dim, Image{(float)img_w, (float)img_h, max_w, max_h}, 0, 0.0f, stream);
}

}  // extern "C"
