// The span scheme of the two fused regression losses (bbox_loss_kernel, delta_loss_kernel), once.  ONE grid covers all images and
// levels of a head: a workgroup finds its level in the table (sph2pob_bbox_loss.hpp), each of its four waves owns one span — a few
// hundred consecutive anchors of one image and one level.  The wave scans the span 64 rows at a time and pushes the indices of the
// rows that take part on a wave-private LDS stack (ballot / mbcnt, as the aligned chunk kernel compacts its survivors), then
// evaluates them in dense passes of up to 64.  The span's slice of the gradient is assembled in a wave-private LDS tile laid out
// like the head's tensor — zeros, then the live rows' values — and leaves in one sweep: every element is stored once, by one lane,
// in whole 16-byte stores along w where the level allows it.  The weighted losses are added in double per lane, wave and workgroup:
// one partial per workgroup.  A row that does not take part is never read: its loss and gradient are exact zeros.
// Device units only (after sph2pob_kernels_common.hpp's rank_below / wave_lds_fence).
#pragma once
#include <type_traits>

#include "sph2pob_kernels_common.hpp"
#include "sph2pob_bbox_loss.hpp"

namespace {

static_assert(kBlock == 64 * sph2pob_bbox::kWaves, "one span per wave");

// live(row) -> bool: does row `row` (of the (B, n) rows of the call) take part.
// eval(lv, b, i, row, k0, g, acc): one live row — anchor i of level lv in image b; adds the row's weighted losses to `acc` in
// component order and, under GRAD, leaves the DIM gradient values in g.
// T: the element type of the levels (eval reads lv.pred through level_ptr<T>).  The tile, the stack and the span geometry do not
// depend on it: a 16-bit T is narrowed in the stream-out, four values per 8-byte store, after the upstream gradient `gs` has been
// folded in on the way into the tile (fp32 levels leave gs to torch's backward).  16-bit T only: partial NULL — no sum is kept.
template <class T, int DIM, bool GRAD, class Live, class Eval>
__device__ __forceinline__ void span_loss(const sph2pob_bbox::Levels& L, float scale, const float* __restrict__ avg_factor, float gs,
                                          double* __restrict__ partial, Live live, Eval eval) {
    constexpr bool F32 = std::is_same<T, float>::value;
    namespace BL = sph2pob_bbox;
    __shared__ __attribute__((aligned(16))) float tile_s[GRAD ? BL::kWaves * BL::kTile : 4];
    __shared__ unsigned short stack_s[BL::kWaves * BL::kStack];
    const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
    const int l = level_of_block(L, blockIdx.x);
    const BL::Level& lv = L.lv[l];
    const int item = ((int)blockIdx.x - lv.block_off) * BL::kWaves + wave;
    double acc = 0.0;
    if (item < lv.items) {   // wave-uniform
        const int b = item / lv.spans, sp = item - b * lv.spans;
        const int p_lo = sp * lv.ps;
        const int cnt = min(lv.ps, lv.pos - p_lo);        // positions of this span
        const int na = cnt * lv.a, i_lo = p_lo * lv.a;    // its anchors: [i_lo, i_lo + na) of the level, na <= kStack
        const int64_t row0 = (int64_t)b * L.n_total + lv.row_off + i_lo;
        float* tile = tile_s + (GRAD ? wave * BL::kTile : 0);
        unsigned short* stack = stack_s + wave * BL::kStack;
        if (GRAD) {   // the span's slice of the gradient: zeros first
            const int used = lv.a * DIM * lv.ps;          // <= kTile, a multiple of 4
            for (int e = lane * 4; e < used; e += 256) *reinterpret_cast<float4*>(tile + e) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        // the rows that take part, in anchor order
        int top = 0;
        for (int s0 = 0; s0 < na; s0 += 64) {
            const int s = s0 + lane;
            const bool on = live(row0 + (s < na ? s : 0)) && s < na;
            const unsigned long long m = __builtin_amdgcn_ballot_w64(on);
            if (on) stack[top + rank_below(m)] = (unsigned short)s;
            top += __popcll(m);
        }
        wave_lds_fence();
        const float k0 = GRAD ? BL::effective_scale(scale, avg_factor) : 0.0f;
        for (int base = 0; base < top; base += 64) {
            const int j = base + lane;
            if (j < top) {
                const int s = stack[j];
                float g[DIM];
                eval(lv, b, i_lo + s, row0 + s, k0, g, acc);
                if (GRAD) {
                    if constexpr (!F32) {
#pragma unroll
                        for (int k = 0; k < DIM; k++) g[k] = gs * g[k];
                    }
                    if (lv.hw > 0) {
                        const int pp = s / lv.a, aa = s - pp * lv.a;
#pragma unroll
                        for (int k = 0; k < DIM; k++) tile[(aa * DIM + k) * lv.ps + pp] = g[k];
                    } else {
#pragma unroll
                        for (int k = 0; k < DIM; k++) tile[s * DIM + k] = g[k];
                    }
                }
            }
        }
        if (GRAD) {
            wave_lds_fence();
            // the tile is `rows` rows of `len` floats: NCHW — one row per channel, the span's positions; flat — one row
            const int rows = lv.hw > 0 ? lv.a * DIM : 1;
            const int len = lv.hw > 0 ? cnt : cnt * DIM;
            const int lstride = lv.hw > 0 ? lv.ps : 0;
            const int64_t gstride = lv.hw > 0 ? lv.hw : 0;
            T* g0 = level_ptr<T>(lv.grad) + (lv.hw > 0 ? (int64_t)b * lv.a * DIM * lv.hw + p_lo : ((int64_t)b * lv.n + i_lo) * DIM);
            if (lv.vec) {   // workgroup-uniform; len, lstride, gstride and g0 are multiples of 4 elements
                const int q4 = len >> 2, total = rows * q4;
                for (int e = lane; e < total; e += 64) {
                    const int r = e / q4, q = e - r * q4;
                    if constexpr (F32) {
                        *reinterpret_cast<float4*>(g0 + r * gstride + 4 * q) = *reinterpret_cast<const float4*>(tile + r * lstride + 4 * q);
                    } else {
                        const float4 v = *reinterpret_cast<const float4*>(tile + r * lstride + 4 * q);
                        store4(g0 + r * gstride + 4 * q, v.x, v.y, v.z, v.w);
                    }
                }
            } else {
                const int total = rows * len;
                for (int e = lane; e < total; e += 64) {
                    const int r = e / len, q = e - r * len;
                    g0[r * gstride + q] = narrow<T>(tile[r * lstride + q]);
                }
            }
        }
    }
    if (!F32 && !partial) return;   // kernel-uniform
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// span_loss for a loss on DECODED boxes (bbox_loss_kernel, gauss_bbox_loss_kernel): a row takes part when its mean weight is not
// zero; a live row runs gather -> decode_one -> pair(box, target, gx, gy) -> decode Jacobian.  pair returns the row's loss and,
// under GRAD, leaves d loss / d box in gx.  The gradient is ((k0 w) gx[k]) jac[k], the composition's product order.
template <class T, int DIM, bool GRAD, class Pair>
__device__ __forceinline__ void decoded_span_loss(const sph2pob_bbox::Levels& L, const float* __restrict__ anchors,
                                                  const float* __restrict__ targets, const float* __restrict__ weight, int wd,
                                                  const sph2pob_coder::Norm& nm, float max_ratio, int cflags, float ctr_clamp, float scale,
                                                  const float* __restrict__ avg_factor, float gs, double* __restrict__ partial, Pair pair) {
    namespace BL = sph2pob_bbox;
    span_loss<T, DIM, GRAD>(
        L, scale, avg_factor, gs, partial,
        [&](int64_t row) { return sph2pob::element_weight<DIM>(weight, wd, row) != 0.0f; },
        [&](const BL::Level& lv, int b, int i, int64_t row, float k0, float (&g)[DIM], double& acc) {
            const float w = sph2pob::element_weight<DIM>(weight, wd, row);
            float p[5], d[5], t[5], box[5], jac[5], gx[5], gy[5];
            int64_t stride;
            const int64_t off = BL::delta_offset(lv, DIM, b, i, &stride);
            const float* ap = anchors + (lv.row_off + i) * DIM;
            const float* tp = targets + row * DIM;
            const T* dp = level_ptr<T>(lv.pred);
#pragma unroll
            for (int k = 0; k < 5; k++) {
                p[k] = k < DIM ? ap[k] : 0.0f;
                d[k] = k < DIM ? (float)dp[off + k * stride] : 0.0f;
                t[k] = k < DIM ? tp[k] : 0.0f;
                box[k] = 0.0f;
            }
            sph2pob_coder::decode_one<DIM, GRAD>(p, d, nm, max_ratio, cflags, ctr_clamp, box, GRAD ? jac : nullptr);
            const float lo = pair(box, t, gx, gy);
            acc += (double)(lo * w);
            if (GRAD) {
                const float gw = k0 * w;
#pragma unroll
                for (int k = 0; k < DIM; k++) g[k] = (gw * gx[k]) * jac[k];
            }
        });
}

// f(integral_constant<int, DIM>, bool_constant<GRAD>) for the box_dim (4 | 5) and the gradient request of a call
template <class F>
void by_dim_grad(int box_dim, bool grad, F&& f) {
    auto by_grad = [&](auto dim) {
        if (grad) f(dim, std::true_type{});
        else f(dim, std::false_type{});
    };
    if (box_dim == 4) by_grad(std::integral_constant<int, 4>{});
    else by_grad(std::integral_constant<int, 5>{});
}

// f(T{}, integral_constant<int, DIM>, bool_constant<GRAD>) for the checked dtype of an _h16 entry
template <class F>
void by_dtype_dim_grad(int dtype, int box_dim, bool grad, F&& f) {
    by_h16_dtype(dtype, [&](auto t) { by_dim_grad(box_dim, grad, [&](auto dim, auto gr) { f(t, dim, gr); }); });
}

}  // namespace
