// The k extreme 32-bit keys of an image's participating rows, ties at the k-th key taken in row order: what the softmax loss's
// hard-negative mining (DESCENDING on loss keys: softmax_cut_kernel) and the random sampler (ascending on Philox ranks:
// sample_select_kernel) share.  Plain host + device code: the rule a select leaves behind, and the host's way to it for the CPU
// twins (sph2pob_host.hip).  Device: the two workgroup-wide steps of the kernels' radix select; filling the histogram, obtaining k
// and whatever a walk carries along belong to the kernels.
#pragma once
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "sph2pob_head_loss.hpp"

namespace sph2pob_select {

// The cut of one image: the k-th key in the direction of the select, and the row index below which rows with exactly that key are
// taken.  (What "nothing taken" looks like is the family's choice: a key no participating row is beyond, upto 0.)
struct Cut { uint32_t key; int32_t upto; };
template <bool DESCENDING> SPHF_DEV bool beyond(uint32_t key, uint32_t cut_key) { return DESCENDING ? key > cut_key : key < cut_key; }
template <bool DESCENDING> SPHF_DEV bool taken(uint32_t key, int64_t i, const Cut& c) { return beyond<DESCENDING>(key, c.key) || (key == c.key && i < (int64_t)c.upto); }

// The cut of rows [0, n) by std::nth_element and one in-order walk.  part(i, &key): whether row i takes part, and its key; at
// least k rows do.  `scratch` is the caller's (reused from image to image).  Returns the rows tied at the cut that are taken;
// k == 0: none, and *cut keeps the caller's "nothing taken".
template <bool DESCENDING, class Part>
inline int64_t host_cut(int64_t n, int64_t k, Part&& part, std::vector<uint32_t>& scratch, Cut* cut) {
    if (k <= 0) return 0;
    scratch.clear();
    uint32_t key;
    for (int64_t i = 0; i < n; i++)
        if (part(i, &key)) scratch.push_back(key);
    std::nth_element(scratch.begin(), scratch.begin() + (k - 1), scratch.end(), [](uint32_t x, uint32_t y) { return beyond<DESCENDING>(x, y); });
    cut->key = scratch[(size_t)(k - 1)];
    int64_t take = k;
    for (uint32_t v : scratch) take -= beyond<DESCENDING>(v, cut->key) ? 1 : 0;
    int64_t seen = 0;
    for (int64_t i = 0; i < n && seen < take; i++)
        if (part(i, &key) && key == cut->key && ++seen == take) cut->upto = (int32_t)(i + 1);
    return take;
}

#if defined(__HIPCC__)
// inclusive prefix sum over the lanes of a wave
__device__ __forceinline__ unsigned wave_prefix(unsigned v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(v, o, 64);
        if ((int)(threadIdx.x & 63) >= o) v += up;
    }
    return v;
}

// The digit decision of one round of the radix select, most significant digit first; called by the whole workgroup (>= 256
// threads) after the barrier that completes the round's 256-bin histogram: two barriers inside.  Thread t < 256 holds the t-th bin
// in the direction of the select (DESCENDING: bin 255 - t), so `ahead`, the rows in the bins the select reaches first, is a prefix
// sum by the first four waves through s_wave[0..3] either way.  rem_of(total) gives the round's rank among the `total` rows of the
// histogram (the first round's k may depend on it).  The one thread whose bin holds the rem-th row, ahead < rem <= ahead + hist,
// writes *s_prefix = prefix | bin << shift, *s_rem = rem - ahead and, on the last digit, *s_ties = the rows tied at the key
// (s_ties may be NULL).  rem == 0: nothing is written.
template <bool DESCENDING, class RemOf>
__device__ __forceinline__ void digit_decision(const unsigned* hist, unsigned* s_wave, unsigned* s_prefix, unsigned* s_rem, unsigned* s_ties,
                                               unsigned prefix, int shift, RemOf&& rem_of) {
    const unsigned tid = threadIdx.x, bin = DESCENDING ? 255u - tid : tid;
    unsigned mine = 0u, incl = 0u;
    if (tid < 256u) {
        mine = hist[bin];
        incl = wave_prefix(mine);
        if ((tid & 63u) == 63u) s_wave[tid >> 6] = incl;
    }
    __syncthreads();
    if (tid < 256u) {
        unsigned before = 0u;
#pragma unroll
        for (unsigned wv = 0; wv < 3; wv++) before += wv < (tid >> 6) ? s_wave[wv] : 0u;
        const unsigned rem = rem_of(s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3]);
        const unsigned ahead = before + incl - mine;
        if (rem > 0u && ahead < rem && rem <= ahead + mine) {   // one thread
            *s_prefix = prefix | (bin << shift);
            *s_rem = rem - ahead;
            if (s_ties && shift == 0) *s_ties = mine;
        }
    }
    __syncthreads();
}

// The scan step of the in-order tie walk; called by the whole workgroup of WAVES waves once per chunk of rows (rows in thread
// order).  in_wave: the tied rows of the lower lanes of the thread's wave; wave_ties: those of the whole wave (read from lane 63).
// Returns the tied rows in front of the thread's own and adds the chunk's to `running` (workgroup-uniform).  One barrier inside;
// the caller puts another before the next call (s_wave is reused), which also publishes what the chunk's deciding thread wrote.
template <int WAVES>
__device__ __forceinline__ unsigned tie_scan(unsigned in_wave, unsigned wave_ties, unsigned* s_wave, unsigned& running) {
    const int wave = (int)(threadIdx.x >> 6);
    if ((threadIdx.x & 63) == 63) s_wave[wave] = wave_ties;
    __syncthreads();
    unsigned before = running, total = 0u;
#pragma unroll
    for (int wv = 0; wv < WAVES; wv++) {
        if (wv < wave) before += s_wave[wv];
        total += s_wave[wv];
    }
    running += total;
    return before + in_wave;
}
#endif

}  // namespace sph2pob_select
