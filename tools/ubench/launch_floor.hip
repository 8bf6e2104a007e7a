// Microbenchmark: what a stream-ordered launch of the dominant kernel's SHAPE costs before any arithmetic — the period of
// back-to-back launches of (a) an empty kernel, (b) the same with the chunk kernel's 18 KB of LDS per workgroup, (c) one
// that only loads its two 16-byte boxes per pair and stores 4 bytes (the memory side alone), on 1 954 workgroups of 256
// threads (1 M pairs).  (c) comes with four forms of its store, which leave different things behind for the kernel boundary:
// a dword per lane (the chunk kernel's form), 16 bytes from lanes 0-31 of each wave (every 128-byte line whole, by one
// instruction), and both again as write-through (sc1) stores, which leave nothing dirty in the L2s.
#include <hip/hip_runtime.h>
#include <stdio.h>
__global__ __launch_bounds__(256) void k_empty(float* out, int n) {
    if (n < 0) out[0] = 1.0f;
}
__global__ __launch_bounds__(256) void k_lds(float* out, int n) {
    __shared__ float q[4608];
    if (n < 0) { q[threadIdx.x] = 1.0f; out[0] = q[(threadIdx.x * 7) & 255]; }
}
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
enum { ST_DWORD = 0, ST_X4 = 1, ST_X4_WT = 2, ST_DWORD_WT = 3 };
constexpr int kAuxWriteThrough = 16;   // sc1
template <int STORE>
__global__ __launch_bounds__(256, 8) void k_stream(const float4* __restrict__ a, const float4* __restrict__ b, float* __restrict__ out, int n) {
    const int wave = (blockIdx.x * 4 + (threadIdx.x >> 6)) * 128, lane = threadIdx.x & 63;
    if (wave >= n) return;
    const int i0 = min(wave + lane, n - 1), i1 = min(wave + 64 + lane, n - 1);
    const float4 x0 = a[i0], y0 = b[i0], x1 = a[i1], y1 = b[i1];
    const float r0 = x0.x + y0.y, r1 = x1.z + y1.w;
    const auto rsrc = __builtin_amdgcn_make_buffer_rsrc(out, 0, n * 4, 0x00020000);
    if (STORE == ST_DWORD) {
        if (wave + lane < n) out[wave + lane] = r0;
        if (wave + 64 + lane < n) out[wave + 64 + lane] = r1;
    } else if (STORE == ST_DWORD_WT) {
        if (wave + lane < n) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r0), rsrc, (wave + lane) * 4, 0, kAuxWriteThrough);
        if (wave + 64 + lane < n) __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(r1), rsrc, (wave + 64 + lane) * 4, 0, kAuxWriteThrough);
    } else if (lane < 32 && wave + 4 * lane + 4 <= n) {   // (the values are beside the point: the same bytes to the same lines)
        const u32x4 v = {__float_as_uint(r0), __float_as_uint(r1), __float_as_uint(x0.y), __float_as_uint(y1.x)};
        if (STORE == ST_X4) *reinterpret_cast<u32x4*>(out + wave + 4 * lane) = v;
        else __builtin_amdgcn_raw_buffer_store_b128(v, rsrc, (wave + 4 * lane) * 4, 0, kAuxWriteThrough);
    }
}
static const char* const kStoreNames[4] = {"dword per lane", "dwordx4, lanes 0-31", "dwordx4 sc1, lanes 0-31", "dword sc1 per lane"};
static void launch_stream(int store, int wgs, hipStream_t st, const float4* a, const float4* b, float* out, int n) {
    if (store == ST_DWORD) k_stream<ST_DWORD><<<wgs, 256, 0, st>>>(a, b, out, n);
    else if (store == ST_X4) k_stream<ST_X4><<<wgs, 256, 0, st>>>(a, b, out, n);
    else if (store == ST_X4_WT) k_stream<ST_X4_WT><<<wgs, 256, 0, st>>>(a, b, out, n);
    else k_stream<ST_DWORD_WT><<<wgs, 256, 0, st>>>(a, b, out, n);
}
int main() {
    const int n = 1000000, wgs = (n + 511) / 512, reps = 5000;
    float4 *a, *b; float* out;
    (void)hipMalloc(&a, n * 16); (void)hipMalloc(&b, n * 16); (void)hipMalloc(&out, n * 4);
    (void)hipMemset(a, 0, n * 16); (void)hipMemset(b, 0, n * 16);
    hipEvent_t e0, e1; (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
    // what: 0 empty, 1 empty + LDS, 2 + s the stream kernel with store form s; the store forms three times over, interleaved, so
    // that their spread shows next to their differences (twice over in the hipGraph part below)
    for (int what : {0, 1, 2, 3, 4, 5, 2, 3, 4, 5, 2, 3, 4, 5}) {
        auto launch = [&]() {
            if (what == 0) k_empty<<<wgs, 256>>>(out, n);
            else if (what == 1) k_lds<<<wgs, 256>>>(out, n);
            else launch_stream(what - 2, wgs, 0, a, b, out, n);
        };
        for (int r = 0; r < 3000; r++) launch();
        (void)hipDeviceSynchronize();
        (void)hipEventRecord(e0);
        for (int r = 0; r < reps; r++) launch();
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        char name[96];
        if (what >= 2) snprintf(name, sizeof name, "load 32 B + store 4 B per pair, %s", kStoreNames[what - 2]);
        printf("%-58s %.3f us per launch (back to back, one stream)\n", what == 0 ? "empty kernel" : what == 1 ? "empty kernel + 18 KB LDS" : name, ms * 1e3 / reps);
    }
    // the same launches replayed from a hipGraph (100 kernel nodes captured from the stream, the graph launched 50 times)
    {
        hipStream_t st; (void)hipStreamCreate(&st);
        for (int what : {0, 2, 3, 4, 5, 2, 3, 4, 5}) {
            hipGraph_t graph; hipGraphExec_t exec;
            (void)hipStreamBeginCapture(st, hipStreamCaptureModeGlobal);
            for (int r = 0; r < 100; r++) {
                if (what == 0) k_empty<<<wgs, 256, 0, st>>>(out, n); else launch_stream(what - 2, wgs, st, a, b, out, n);
            }
            (void)hipStreamEndCapture(st, &graph);
            (void)hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
            for (int r = 0; r < 20; r++) (void)hipGraphLaunch(exec, st);
            (void)hipStreamSynchronize(st);
            (void)hipEventRecord(e0, st);
            for (int r = 0; r < 50; r++) (void)hipGraphLaunch(exec, st);
            (void)hipEventRecord(e1, st); (void)hipEventSynchronize(e1);
            float ms; (void)hipEventElapsedTime(&ms, e0, e1);
            char name[96];
            snprintf(name, sizeof name, "load 32 B + store 4 B, %s:", what >= 2 ? kStoreNames[what - 2] : "");
            printf("hipGraph of 100 nodes, %-48s %.3f us per node\n", what == 0 ? "empty kernel:" : name, ms * 1e3 / 5000);
            (void)hipGraphExecDestroy(exec); (void)hipGraphDestroy(graph);
        }
    }
    // how the empty launch depends on the grid
    for (int g : {1, 256, 512, 1024, 1954, 3908, 7816}) {
        for (int r = 0; r < 2000; r++) k_empty<<<g, 256>>>(out, n);
        (void)hipDeviceSynchronize();
        (void)hipEventRecord(e0);
        for (int r = 0; r < reps; r++) k_empty<<<g, 256>>>(out, n);
        (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
        float ms; (void)hipEventElapsedTime(&ms, e0, e1);
        printf("empty kernel, %5d workgroups of 256 threads: %.3f us per launch\n", g, ms * 1e3 / reps);
    }
    return 0;
}
