// Softmax cross-entropy kernels, plain and with hard-negative mining (the arithmetic, the keys and the cut rule: sph2pob_softmax.hpp).
//   softmax_rows_kernel   ONE grid over all levels of a head, the level found per workgroup as focal_sum_kernel does.  A thread owns
//                         four consecutive positions of one (image, anchor) of an NCHW level (16-byte accesses at stride H W over
//                         the K class planes) or one row of a flat level, and walks the classes three times: maximum, sums,
//                         gradient.  PLAIN: losses added in double, one partial per workgroup, gradients written on the way.
//                         KEYS (mining, first pass): one 32-bit key per row — none / positive / the negative's loss — and the
//                         positives' partial.  MINED (mining, last pass): a row is live when its key says positive or mined(key,
//                         index, the image's cut); live rows re-read their logits, the others get exact zeros and read nothing.
//   softmax_cut_kernel    one workgroup per image: P_b and N_b from the keys, k_b = min(r P_b, N_b), the k_b-th largest key by a
//                         four-digit radix select (LDS histogram, integer atomics; digit decision and tie scan: sph2pob_select.hpp),
//                         then one in-order walk: the mined losses added in double, the row index up to which ties at the cut are taken
//   head_final_kernel     (sph2pob_head_loss.hpp) adds the workgroups' and the images' partials in a fixed order
// No float atomics and no global counters: the same bits on every call.  One stream, no host read.
#include "sph2pob_softmax.hpp"

namespace {

using namespace sph2pob_softmax;

enum { PLAIN = 0, KEYS = 1, MINED = 2 };

struct Args {
    int K;
    const int64_t* labels;
    const float* weight;
    const float* class_weight;
    int64_t ignore_index, background;
    unsigned* keys;
    const Cut* cut;
};

template <int V>
__device__ __forceinline__ void load_v(const float* p, float (&x)[V]) {
    if constexpr (V == 4) { const float4 v = *reinterpret_cast<const float4*>(p); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
    else x[0] = p[0];
}
template <int V>
__device__ __forceinline__ void store_v(float* p, const float (&x)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(x[0], x[1], x[2], x[3]);
    else p[0] = x[0];
}

// V rows side by side: class c of all of them is V consecutive floats at x + c * stride
template <int V_>
struct PlaneWalk {
    static constexpr int V = V_;
    const float* x;
    float* g;
    int64_t stride;
    template <class F> __device__ __forceinline__ void read(int K, F&& f) const {
#pragma unroll 4
        for (int c = 0; c < K; c++) {
            float xv[V];
            load_v<V>(x + (int64_t)c * stride, xv);
            f(c, xv);
        }
    }
    template <class F> __device__ __forceinline__ void write(int K, F&& f) const {
#pragma unroll 2
        for (int c = 0; c < K; c++) {
            float xv[V], gv[V];
            load_v<V>(x + (int64_t)c * stride, xv);
            f(c, xv, gv);
            store_v<V>(g + (int64_t)c * stride, gv);
        }
    }
    __device__ __forceinline__ void zero(int K) const {
        float z[V];
#pragma unroll
        for (int v = 0; v < V; v++) z[v] = 0.0f;
        for (int c = 0; c < K; c++) store_v<V>(g + (int64_t)c * stride, z);
    }
};

// one contiguous row, W classes per access (W == 4: K % 4 == 0 and an aligned base)
template <int W>
struct RowWalk {
    static constexpr int V = 1;
    const float* x;
    float* g;
    template <class F> __device__ __forceinline__ void read(int K, F&& f) const {
#pragma unroll 2
        for (int c0 = 0; c0 < K; c0 += W) {
            float q[W];
            load_v<W>(x + c0, q);
#pragma unroll
            for (int j = 0; j < W; j++) { float xv[1] = {q[j]}; f(c0 + j, xv); }
        }
    }
    template <class F> __device__ __forceinline__ void write(int K, F&& f) const {
        for (int c0 = 0; c0 < K; c0 += W) {
            float q[W], o[W];
            load_v<W>(x + c0, q);
#pragma unroll
            for (int j = 0; j < W; j++) { float xv[1] = {q[j]}, gv[1]; f(c0 + j, xv, gv); o[j] = gv[0]; }
            store_v<W>(g + c0, o);
        }
    }
    __device__ __forceinline__ void zero(int K) const {
        float z[W];
#pragma unroll
        for (int j = 0; j < W; j++) z[j] = 0.0f;
        for (int c0 = 0; c0 < K; c0 += W) store_v<W>(g + c0, z);
    }
};

// The V rows of one item: image b, indices j[v] inside the image.  Returns what the item adds to its workgroup's partial: the valid
// rows' losses (PLAIN), the positives' (KEYS), nothing (MINED).
template <int MODE, bool GRAD, class Walk>
__device__ __forceinline__ double rows_body(const Walk& wk, const Args& A, int64_t n_total, int64_t n_pad, int b, const int (&j)[Walk::V], float k0) {
    constexpr int V = Walk::V;
    Row r[V];
    bool live[V], valid[V], pos[V];
    float cwl[V], w[V], loss[V];
    bool any = false;
#pragma unroll
    for (int v = 0; v < V; v++) {
        const int64_t row = (int64_t)b * n_total + j[v];
        const int64_t lab = A.labels[row];
        valid[v] = valid_label(lab, A.K, A.ignore_index);
        pos[v] = valid[v] && lab != A.background;
        if (MODE == MINED) {
            const unsigned key = A.keys[(int64_t)b * n_pad + j[v]];
            live[v] = key == kKeyPos || mined(key, j[v], A.cut[b]);
        } else {
            live[v] = valid[v];
        }
        r[v].begin(live[v] ? (int)lab : -1);
        cwl[v] = live[v] ? class_factor(A.class_weight, lab) : 0.0f;
        w[v] = live[v] ? row_weight(A.weight, row) : 0.0f;
        loss[v] = 0.0f;
        any = any || live[v];
    }
    if (any) {
        wk.read(A.K, [&](int c, const float (&xv)[V]) {
#pragma unroll
            for (int v = 0; v < V; v++) r[v].see_max(c, xv[v]);
        });
#pragma unroll
        for (int v = 0; v < V; v++) r[v].close_max();
        wk.read(A.K, [&](int c, const float (&xv)[V]) {
#pragma unroll
            for (int v = 0; v < V; v++) r[v].see_sum(c, xv[v]);
        });
#pragma unroll
        for (int v = 0; v < V; v++) {
            const float ce = r[v].close_sum();
            loss[v] = live[v] ? row_loss(ce, cwl[v], w[v]) : 0.0f;
        }
    }
    double acc = 0.0;
#pragma unroll
    for (int v = 0; v < V; v++) {
        if (MODE == KEYS) {
            A.keys[(int64_t)b * n_pad + j[v]] = !valid[v] ? kKeyNone : (pos[v] ? kKeyPos : loss_key(loss[v]));
            if (pos[v]) acc += (double)loss[v];
        } else if (MODE == PLAIN) {
            if (live[v]) acc += (double)loss[v];
        }
    }
    if (GRAD) {
        if (any) {
            float kw[V];
#pragma unroll
            for (int v = 0; v < V; v++) kw[v] = k0 * (cwl[v] * w[v]);
            wk.write(A.K, [&](int c, const float (&xv)[V], float (&gv)[V]) {
#pragma unroll
                for (int v = 0; v < V; v++) gv[v] = live[v] ? kw[v] * r[v].grad(c, xv[v]) : 0.0f;
            });
        } else {
            wk.zero(A.K);
        }
    }
    return acc;
}

template <int MODE, bool GRAD, int V>
__device__ __forceinline__ double nchw_item(const Level& lv, int item, const Args& A, const Levels& L, float k0) {
    const int per = lv.hw / V;
    const int ba = item / per, pq = item - ba * per;
    const int b = ba / lv.a, a = ba - b * lv.a;
    const int p0 = pq * V;
    int j[V];
#pragma unroll
    for (int v = 0; v < V; v++) j[v] = (int)lv.row_off + (p0 + v) * lv.a + a;   // anchor (h W + w) A + a
    const int64_t base = (int64_t)ba * A.K * lv.hw + p0;                        // class 0 of channel a K
    const PlaneWalk<V> wk{lv.logits + base, GRAD ? lv.grad + base : nullptr, (int64_t)lv.hw};
    return rows_body<MODE, GRAD>(wk, A, L.n_total, L.n_pad, b, j, k0);
}

template <int MODE, bool GRAD, int W>
__device__ __forceinline__ double flat_item(const Level& lv, int item, const Args& A, const Levels& L, float k0) {
    const int b = item / lv.n, i = item - b * lv.n;
    const int j[1] = {(int)lv.row_off + i};
    const int64_t base = (int64_t)item * A.K;
    const RowWalk<W> wk{lv.logits + base, GRAD ? lv.grad + base : nullptr};
    return rows_body<MODE, GRAD>(wk, A, L.n_total, L.n_pad, b, j, k0);
}

template <int MODE, bool GRAD>
__global__ __launch_bounds__(kBlock) void softmax_rows_kernel(Levels L, Args A, float scale, const float* __restrict__ avg_factor,
                                                              double* __restrict__ partial) {
    const int l = level_of_block(L, blockIdx.x);
    const Level& lv = L.lv[l];
    const int item = ((int)blockIdx.x - lv.block_off) * kBlock + (int)threadIdx.x;
    const float k0 = GRAD ? effective_scale(scale, avg_factor) : 0.0f;
    double acc = 0.0;
    if (item < lv.items) {
        switch (lv.kind) {   // workgroup-uniform
            case KIND_NCHW4: acc = nchw_item<MODE, GRAD, 4>(lv, item, A, L, k0); break;
            case KIND_NCHW1: acc = nchw_item<MODE, GRAD, 1>(lv, item, A, L, k0); break;
            case KIND_FLAT4: acc = flat_item<MODE, GRAD, 4>(lv, item, A, L, k0); break;
            default: acc = flat_item<MODE, GRAD, 1>(lv, item, A, L, k0); break;
        }
    }
    if (MODE == MINED) return;   // the gradient pass adds nothing: the mined losses were read from the keys
    const double r = block_sum_f64(acc);
    if (threadIdx.x == 0) partial[blockIdx.x] = r;
}

// hist[bin] += 1 for every lane that is `on`.  Loss keys crowd into a few bins of the leading digit (one sign and seven exponent
// bits), and 64 LDS atomics on one address take 64 turns: the lanes that share the bin of the first waiting lane are counted by
// one atomic of their number, twice over, and whoever is left adds for itself.  Called by whole waves (the ballots need no more).
__device__ __forceinline__ void hist_add(unsigned* hist, bool on, unsigned bin) {
    const int lane = (int)(threadIdx.x & 63);
    unsigned long long todo = __ballot(on);
#pragma unroll
    for (int round = 0; round < 2; round++) {
        if (todo == 0ull) return;   // wave-uniform
        const int leader = __ffsll((long long)todo) - 1;
        const unsigned lb = __shfl(bin, leader, 64);
        const unsigned long long same = __ballot(on && bin == lb);
        if (lane == leader) atomicAdd(&hist[lb], (unsigned)__popcll(same));
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) atomicAdd(&hist[bin], 1u);
}

// One workgroup of kCutBlock threads per image.  keys: n_pad words per image, the first n written by the KEYS pass.
__global__ __launch_bounds__(kCutBlock) void softmax_cut_kernel(const unsigned* __restrict__ keys, int n, int64_t n_pad, int64_t ratio,
                                                                Cut* __restrict__ cut, double* __restrict__ mined_sum) {
    constexpr int kWaves = kCutBlock / 64;
    __shared__ unsigned hist[256];
    __shared__ unsigned s_pos, s_prefix, s_rem, s_wave[kWaves];
    __shared__ int s_upto;
    __shared__ double s_sum[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const uint4* kb = reinterpret_cast<const uint4*>(keys + (int64_t)b * n_pad);   // 16-byte aligned: n_pad % 4 == 0
    const int quads = (int)(n_pad / 4);
    if (tid == 0) { s_pos = 0u; s_prefix = 0u; s_rem = 0u; s_upto = 0; }

    // radix select, most significant digit first: after digit d the cut key's top 8 (d + 1) bits are known
    for (int d = 0; d < 4; d++) {
        const int shift = 24 - 8 * d;
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        const unsigned prefix = s_prefix, rem_in = s_rem;
        if (d == 0 || rem_in > 0u) {   // workgroup-uniform
            const unsigned known = d == 0 ? 0u : 0xffffffffu << (shift + 8);   // the digits already fixed
            unsigned npos = 0u;
            for (int q0 = 0; q0 < quads; q0 += kCutBlock) {   // whole waves: hist_add ballots
                const int q = q0 + tid;
                uint4 kq = make_uint4(kKeyNone, kKeyNone, kKeyNone, kKeyNone);
                if (q < quads) kq = kb[q];
                const unsigned kv[4] = {kq.x, kq.y, kq.z, kq.w};
#pragma unroll
                for (int e = 0; e < 4; e++) {
                    const unsigned key = 4 * q + e < n ? kv[e] : kKeyNone;
                    if (key == kKeyPos) npos++;
                    hist_add(hist, key >= 2u && ((key ^ prefix) & known) == 0u, (key >> shift) & 255u);
                }
            }
            if (d == 0 && npos) atomicAdd(&s_pos, npos);
        }
        __syncthreads();
        // the digit: the one bin that holds the rem-th largest key; in the first round rem is k_b, from the negatives the bins hold
        sph2pob_select::digit_decision<true>(hist, s_wave, &s_prefix, &s_rem, nullptr, prefix, shift, [&](unsigned total) {
            return d == 0 ? (unsigned)mined_count(ratio, (int64_t)s_pos, (int64_t)total) : rem_in;
        });
    }
    const unsigned take = s_rem;                          // rows tied at the cut key that are mined (>= 1 when anything is)
    const unsigned cut_key = take > 0u ? s_prefix : kKeyNaN;
    __syncthreads();

    // in-order walk: the mined losses above the cut, and the index of the take-th row tied at it
    double acc = 0.0;
    unsigned running = 0u;
    for (int q0 = 0; q0 < quads; q0 += kCutBlock) {
        const int q = q0 + tid;
        unsigned kv[4] = {kKeyNone, kKeyNone, kKeyNone, kKeyNone};
        if (q < quads) {
            const uint4 kq = kb[q];
            kv[0] = kq.x; kv[1] = kq.y; kv[2] = kq.z; kv[3] = kq.w;
        }
        unsigned ties = 0u;
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (4 * q + e >= n) kv[e] = kKeyNone;
            if (take > 0u && kv[e] >= 2u && kv[e] > cut_key) acc += (double)key_loss(kv[e]);
            if (take > 0u && kv[e] == cut_key) ties++;
        }
        const unsigned incl = sph2pob_select::wave_prefix(ties);
        unsigned seen = sph2pob_select::tie_scan<kWaves>(incl - ties, incl, s_wave, running);
#pragma unroll
        for (int e = 0; e < 4; e++) {
            if (take > 0u && kv[e] == cut_key && ++seen == take) s_upto = 4 * q + e + 1;   // one thread of one iteration
        }
        __syncthreads();
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
    if ((tid & 63) == 0) s_sum[tid >> 6] = acc;
    __syncthreads();
    if (tid == 0) {
        double r = 0.0;
        for (int wv = 0; wv < kWaves; wv++) r += s_sum[wv];
        if (take > 0u) r += (double)take * (double)key_loss(cut_key);
        mined_sum[b] = r;
        Cut c;
        c.key = cut_key; c.upto = s_upto;
        cut[b] = c;
    }
}

// ---- flat (N, K): reduction 'none' and its backward, one row per thread ----
template <int W>
__device__ __forceinline__ void flat_row(const float* x, float* gx, int K, int64_t lab, float cwl, float w, float kg, float scale, float* loss) {
    Row r;
    r.begin((int)lab);
    const RowWalk<W> wk{x, gx};
    wk.read(K, [&](int c, const float (&xv)[1]) { r.see_max(c, xv[0]); });
    r.close_max();
    wk.read(K, [&](int c, const float (&xv)[1]) { r.see_sum(c, xv[0]); });
    const float ce = r.close_sum();
    if (loss) loss[0] = scale * row_loss(ce, cwl, w);
    if (gx) wk.write(K, [&](int c, const float (&xv)[1], float (&gv)[1]) { gv[0] = kg * r.grad(c, xv[0]); });
}

// loss (N,) when gx is NULL, else gx (N, K) = g[row * stride] * (k0 cw w) * d CE / d x
template <int W>
__global__ __launch_bounds__(kBlock) void softmax_flat_kernel(const float* __restrict__ x, const int64_t* __restrict__ labels,
                                                              const float* __restrict__ weight, const float* __restrict__ class_weight,
                                                              int64_t ignore_index, const float* __restrict__ g, int stride, float scale,
                                                              const float* __restrict__ avg_factor, float* __restrict__ loss,
                                                              float* __restrict__ gx, int64_t n, int K) {
    const float k0 = gx ? effective_scale(scale, avg_factor) : scale;
    for (int64_t row = (int64_t)blockIdx.x * kBlock + threadIdx.x; row < n; row += (int64_t)gridDim.x * kBlock) {
        const int64_t lab = labels[row];
        if (!valid_label(lab, K, ignore_index)) {
            if (loss) loss[row] = 0.0f;
            if (gx) { const RowWalk<W> wk{x + row * K, gx + row * K}; wk.zero(K); }
            continue;
        }
        const float cwl = class_factor(class_weight, lab), w = row_weight(weight, row);
        const float kg = gx ? g[stride ? row : 0] * (k0 * (cwl * w)) : 0.0f;
        flat_row<W>(x + row * K, gx ? gx + row * K : nullptr, K, lab, cwl, w, kg, scale, loss ? loss + row : nullptr);
    }
}

unsigned capped_blocks(int64_t total) {
    int64_t blocks = (total + kBlock - 1) / kBlock;
    const int64_t cap = (int64_t)cu_count() * 8;
    return (unsigned)(blocks > cap ? cap : blocks);
}

int launch_flat(const float* x, const int64_t* labels, const float* weight, const float* class_weight, int64_t ignore_index, const float* g,
                int stride, float scale, const float* avg_factor, float* loss, float* gx, int64_t n, int64_t K, hipStream_t s) {
    const bool vec = K % 4 == 0 && aligned_to(x, 16) && aligned_to(gx, 16);
    auto go = [&](auto kernel) {
        hipLaunchKernelGGL(kernel, dim3(capped_blocks(n)), dim3(kBlock), 0, s, x, labels, weight, class_weight, ignore_index, g, stride, scale,
                           avg_factor, loss, gx, n, (int)K);
    };
    if (vec) go(softmax_flat_kernel<4>);
    else go(softmax_flat_kernel<1>);
    return launch_status();
}

}  // namespace

extern "C" {

int64_t sph2pob_softmax_loss_workspace_bytes(const int64_t* level_n, const int64_t* level_hw, int num_levels, int64_t num_images,
                                             int64_t num_channels, int mining) {
    return workspace_bytes(level_n, level_hw, num_levels, num_images, num_channels, mining);
}

int sph2pob_softmax_loss_sum_f32(const void* const* logits, void* const* grads, const int64_t* level_n, const int64_t* level_hw,
                                 int num_levels, int64_t num_images, int64_t num_channels, const int64_t* labels, const float* weight,
                                 const float* class_weight, int64_t ignore_index, int64_t background_label, int64_t neg_pos_ratio,
                                 float scale, const float* avg_factor, float* out, void* workspace, void* stream) {
    Levels L;
    if (int rc = make_levels(logits, grads, level_n, level_hw, num_levels, num_images, num_channels, neg_pos_ratio, true, &L)) return rc;
    if (!out || !workspace || (L.rows > 0 && !labels)) return SPH2POB_ERR_NULL;
    hipStream_t s = (hipStream_t)stream;
    const bool mining = neg_pos_ratio >= 0;
    const Workspace ws = carve(workspace, level_n, level_hw, num_levels, num_images, num_channels);
    Args A{(int)num_channels, labels, weight, class_weight, ignore_index, background_label, ws.keys, ws.cut};
    int nb = 0;
    if (L.blocks > 0) {
        const dim3 grid(L.blocks), block(kBlock);
        nb = L.blocks;
        if (!mining) {
            if (grads) hipLaunchKernelGGL((softmax_rows_kernel<PLAIN, true>), grid, block, 0, s, L, A, scale, avg_factor, ws.partial);
            else hipLaunchKernelGGL((softmax_rows_kernel<PLAIN, false>), grid, block, 0, s, L, A, scale, avg_factor, ws.partial);
        } else {
            hipLaunchKernelGGL((softmax_rows_kernel<KEYS, false>), grid, block, 0, s, L, A, scale, avg_factor, ws.partial);
            hipLaunchKernelGGL(softmax_cut_kernel, dim3((unsigned)num_images), dim3(kCutBlock), 0, s, ws.keys, (int)L.n_total, L.n_pad,
                               neg_pos_ratio, ws.cut, ws.partial + L.blocks);
            nb += (int)num_images;
            if (grads) hipLaunchKernelGGL((softmax_rows_kernel<MINED, true>), grid, block, 0, s, L, A, scale, avg_factor, ws.partial);
        }
    }
    return launch_final(ws.partial, nb, scale, avg_factor, out, s);
}

int sph2pob_softmax_loss_fwd_f32(const float* logits, const int64_t* labels, const float* weight, const float* class_weight,
                                 int64_t ignore_index, float scale, float* loss, int64_t n, int64_t num_channels, void* stream) {
    if (int rc = flat_check(n, num_channels, 0)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !loss) return SPH2POB_ERR_NULL;
    return launch_flat(logits, labels, weight, class_weight, ignore_index, nullptr, 0, scale, nullptr, loss, nullptr, n, num_channels,
                       (hipStream_t)stream);
}

int sph2pob_softmax_loss_bwd_f32(const float* logits, const int64_t* labels, const float* weight, const float* class_weight,
                                 int64_t ignore_index, const float* grad_out, int grad_stride, float scale, const float* avg_factor,
                                 float* grad_logits, int64_t n, int64_t num_channels, void* stream) {
    if (int rc = flat_check(n, num_channels, grad_stride)) return rc;
    if (n == 0) return SPH2POB_OK;
    if (!logits || !labels || !grad_out || !grad_logits) return SPH2POB_ERR_NULL;
    return launch_flat(logits, labels, weight, class_weight, ignore_index, grad_out, grad_stride, scale, avg_factor, nullptr, grad_logits, n,
                       num_channels, (hipStream_t)stream);
}

}  // extern "C"
