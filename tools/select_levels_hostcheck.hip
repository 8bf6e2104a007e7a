// A stand-alone host program over the plain C++ parts of csrc/sph2pob_select.hpp and csrc/sph2pob_class_levels.hpp, meant for a
// sanitizer build (no GPU, nothing loaded into Python):
//   hipcc --offload-arch=gfx950 --cuda-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -fno-sanitize-recover=all \
//         tools/select_levels_hostcheck.hip -o select_levels_hostcheck && ./select_levels_hostcheck
// The level walk of both families on the test scenes' shapes, on B = 0 and on a level without anchors, every row span written into
// buffers of exactly the levels' sizes; the host cut in both directions on tied and untied keys, k from 0 to all.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../sph_retina_amd/csrc/sph2pob_focal.hpp"
#include "../sph_retina_amd/csrc/sph2pob_sample.hpp"
#include "../sph_retina_amd/csrc/sph2pob_softmax.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

namespace CL = sph2pob_class;
namespace SE = sph2pob_select;

// every (b, anchor, channel) of every level is written exactly once through class_row_span
template <class Make>
static void walk(const std::vector<int64_t>& ns, const std::vector<int64_t>& hws, int64_t B, int64_t C, bool flat_rows, Make&& make) {
    const int num = (int)ns.size();
    std::vector<std::vector<float>> x(num), g(num);
    std::vector<const void*> xp(num);
    std::vector<void*> gp(num);
    for (int l = 0; l < num; l++) {
        x[l].assign((size_t)(B * ns[l] * C), 0.0f); g[l].assign(x[l].size(), 0.0f);
        xp[l] = x[l].data(); gp[l] = g[l].data();   // (an empty vector's data() may be NULL: a level without elements may have no pointer)
    }
    CL::Levels U, L;
    CHECK(make(nullptr, nullptr, ns.data(), hws.data(), num, false, &U) == SPH2POB_OK);
    CHECK(make(xp.data(), gp.data(), ns.data(), hws.data(), num, true, &L) == SPH2POB_OK);
    int64_t n_total = 0, elems = 0;
    for (int l = 0; l < num; l++) {
        const CL::Level& lv = L.lv[l];
        CHECK(lv.row_off == n_total && lv.n == ns[l] && lv.block_off <= U.lv[l].block_off);
        const int64_t per_item = lv.kind == CL::KIND_NCHW4 ? 4 * C : (lv.hw > 0 || flat_rows) ? C : (lv.kind == CL::KIND_FLAT4 ? 4 : 1);
        CHECK((int64_t)lv.items * per_item == B * ns[l] * C);
        for (int64_t b = 0; b < B; b++)
            for (int64_t i = 0; i < ns[l]; i++) {
                int64_t base, stride;
                CL::class_row_span(lv, C, b, i, &base, &stride);
                for (int64_t c = 0; c < C; c++) lv.grad[base + c * stride] += 1.0f;
            }
        for (float v : g[l]) CHECK(v == 1.0f);
        n_total += ns[l]; elems += B * ns[l] * C;
    }
    CHECK(L.n_total == n_total && L.elems == elems && L.rows == B * n_total && L.n_pad % 4 == 0 && L.n_pad >= n_total && L.n_pad < n_total + 4);
    CHECK(L.blocks <= U.blocks && U.n_total == n_total);
}

static void levels() {
    const std::vector<int64_t> scene_n{96, 30, 1}, scene_hw{32, 15, 1}, big_n{4608}, big_hw{512}, flat_n{96, 0, 31}, flat_hw{0, 0, 0};
    for (int64_t B : {0, 1, 4})
        for (int64_t C : {6, 8}) {
            auto softmax = [&](const void* const* x, void* const* g, const int64_t* n, const int64_t* hw, int num, bool tables, CL::Levels* out) {
                return sph2pob_softmax::make_levels(x, g, n, hw, num, B, C, 3, tables, out);
            };
            auto focal = [&](const void* const* x, void* const* g, const int64_t* n, const int64_t* hw, int num, bool tables, CL::Levels* out) {
                return sph2pob_focal::make_levels(x, g, n, hw, num, B, C, 1, 2.0f, tables, out);
            };
            walk(scene_n, scene_hw, B, C, true, softmax); walk(scene_n, scene_hw, B, C, false, focal);
            walk(big_n, big_hw, B, C, true, softmax);     walk(big_n, big_hw, B, C, false, focal);
            walk(flat_n, flat_hw, B, C, true, softmax);   walk(flat_n, flat_hw, B, C, false, focal);
        }
    // the order of the checks: OPTION, then SIZE, then NULL
    CL::Levels L;
    const int64_t one[1] = {4}, bad[1] = {-1};
    CHECK(sph2pob_softmax::make_levels(nullptr, nullptr, one, nullptr, 0, 1, 1, -2, true, &L) == SPH2POB_ERR_OPTION);
    CHECK(sph2pob_softmax::make_levels(nullptr, nullptr, nullptr, nullptr, 1, 1, 1, 3, true, &L) == SPH2POB_ERR_SIZE);
    CHECK(sph2pob_softmax::make_levels(nullptr, nullptr, nullptr, nullptr, 1, 1, 6, 3, true, &L) == SPH2POB_ERR_NULL);
    CHECK(sph2pob_focal::make_levels(nullptr, nullptr, bad, nullptr, 1, 1, 0, 3, -1.0f, false, &L) == SPH2POB_ERR_OPTION);
    CHECK(sph2pob_focal::make_levels(nullptr, nullptr, bad, nullptr, 1, 1, 6, 0, 2.0f, false, &L) == SPH2POB_ERR_SIZE);
    CHECK(sph2pob_focal::make_levels(nullptr, nullptr, one, nullptr, 1, 1, 6, 0, 2.0f, true, &L) == SPH2POB_ERR_NULL);
}

// the cut against the definition: the taken rows are the first k of a stable sort by key in the direction
template <bool DESC>
static void cut_case(const std::vector<uint32_t>& keys, const std::vector<char>& part, int64_t k) {
    const int64_t n = (int64_t)keys.size();
    std::vector<uint32_t> scratch;
    SE::Cut c{DESC ? 0xffffffffu : 0u, 0};
    const SE::Cut none = c;
    const int64_t take = SE::host_cut<DESC>(n, k, [&](int64_t i, uint32_t* key) { *key = keys[(size_t)i]; return part[(size_t)i] != 0; }, scratch, &c);
    if (k == 0) { CHECK(take == 0 && c.key == none.key && c.upto == none.upto); }
    std::vector<int64_t> order;
    for (int64_t i = 0; i < n; i++) if (part[(size_t)i]) order.push_back(i);
    CHECK(k <= (int64_t)order.size());
    std::stable_sort(order.begin(), order.end(), [&](int64_t a, int64_t b) { return SE::beyond<DESC>(keys[(size_t)a], keys[(size_t)b]); });
    std::vector<char> want((size_t)n, 0);
    for (int64_t j = 0; j < k; j++) want[(size_t)order[(size_t)j]] = 1;
    int64_t got = 0, tied = 0;
    for (int64_t i = 0; i < n; i++) {
        const bool in = part[(size_t)i] && SE::taken<DESC>(keys[(size_t)i], i, c);   // (k == 0: the "nothing taken" cut takes nothing)
        CHECK(in == (want[(size_t)i] != 0));
        got += in; tied += in && keys[(size_t)i] == c.key;
    }
    CHECK(got == k && tied == take);
}

static void cuts() {
    uint32_t s = 12345u;
    auto next = [&]() { s = s * 1664525u + 1013904223u; return s; };
    for (int64_t n : {0, 1, 127, 4608}) {
        std::vector<char> part((size_t)n);
        int64_t parts = 0;
        for (auto& p : part) { p = next() % 5u != 0u; parts += p; }
        std::vector<uint32_t> tied((size_t)n, 0x3fe5d58eu), spread((size_t)n), few((size_t)n), ends((size_t)n);
        for (int64_t i = 0; i < n; i++) { spread[(size_t)i] = next(); few[(size_t)i] = next() % 3u; ends[(size_t)i] = next() % 2u ? 0xffffffffu : 0u; }
        for (const auto* keys : {&tied, &spread, &few, &ends})
            for (int64_t k : {(int64_t)0, (int64_t)1, parts / 2, parts - 1, parts}) {
                if (k < 0 || k > parts) continue;
                cut_case<true>(*keys, part, k);
                cut_case<false>(*keys, part, k);
            }
    }
}

int main() {
    levels();
    cuts();
    // the rules as the two families state them
    const SE::Cut c{7u, 5};
    CHECK(sph2pob_softmax::mined(9u, 100, c) && sph2pob_softmax::mined(7u, 4, c) && !sph2pob_softmax::mined(7u, 5, c) && !sph2pob_softmax::mined(1u, 0, c));
    const sph2pob_sample::Pick p{c, 3};
    CHECK(sph2pob_sample::sampled(6u, 100, p) && sph2pob_sample::sampled(7u, 4, p) && !sph2pob_sample::sampled(7u, 5, p) && !sph2pob_sample::sampled(8u, 0, p));
    static_assert(sizeof(sph2pob_sample::Pick) == 16 && sizeof(SE::Cut) == 8, "the workspace layout");
    printf("select / class-levels host check ok\n");
    return 0;
}
