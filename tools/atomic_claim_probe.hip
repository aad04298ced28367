// atomic_claim_probe.hip -- how many returning agent-scope adds ONE word takes
// per microsecond on this MI355X: what bounds the tile claims of k_stream_nmc
// (csrc/ce_stream.hpp).  One kernel, one block of 4 waves per CU as the stream
// runs; lane 0 of every wave adds 1 to the same word `iters` times.
//   dep   each add waits for the one before it (a wave's claim latency under
//         contention: one add in flight per wave)
//   free  8 adds in flight per wave (the word's throughput)
// Prints one JSON line; profiles/stream_launch_phases.json keeps the figures.
// Build: make -C consensus-entropy_amd probes   (tools/_diag/atomic_claim_probe)
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

template <int DEPTH>
__global__ __launch_bounds__(256) void k_claims(uint32_t* word, int iters, uint32_t* sink) {
    if ((threadIdx.x & 63) != 0) return;
    uint32_t acc = 0;
    for (int i = 0; i < iters; i += DEPTH) {
        uint32_t v[DEPTH];
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) v[d] = __builtin_amdgcn_atomic_inc32(word, 0xffffffffu, __ATOMIC_RELAXED, "agent");
#pragma unroll
        for (int d = 0; d < DEPTH; ++d) acc ^= v[d];
    }
    if (acc == 0x9e3779b9u && iters < 0) sink[0] = acc;  // keeps the returns live
}

template <int DEPTH>
static double run(uint32_t* word, uint32_t* sink, int grid, int iters, uint32_t* total) {
    hipEvent_t a, b;
    (void)hipEventCreate(&a);
    (void)hipEventCreate(&b);
    float best = 1e30f;
    for (int r = 0; r < 4; ++r) {  // the first is the warm-up
        (void)hipMemset(word, 0, 4);
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL(k_claims<DEPTH>, dim3(grid), dim3(256), 0, 0, word, iters, sink);
        (void)hipEventRecord(b, 0);
        (void)hipEventSynchronize(b);
        float ms = 0;
        (void)hipEventElapsedTime(&ms, a, b);
        if (r > 0 && ms < best) best = ms;
    }
    (void)hipMemcpy(total, word, 4, hipMemcpyDeviceToHost);
    return (double)best * 1e3;  // us
}

int main() {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus <= 0) {
        printf("{\"error\": \"no device\"}\n");
        return 1;
    }
    uint32_t *word = nullptr, *sink = nullptr;
    if (hipMalloc(&word, 256) != hipSuccess || hipMalloc(&sink, 4) != hipSuccess) return 1;
    const int iters = 2048;  // per wave: 4 * cus * 2048 adds per launch (2.1M on 256 CUs)
    const double adds = 4.0 * cus * iters;
    uint32_t t1 = 0, t8 = 0;
    const double dep_us = run<1>(word, sink, cus, iters, &t1);
    const double free_us = run<8>(word, sink, cus, iters, &t8);
    const bool ok = t1 == (uint32_t)adds && t8 == (uint32_t)adds;  // no add lost
    printf("{\"probe\": \"atomic_claim_probe\", \"cus\": %d, \"waves\": %d, \"adds_per_launch\": %.0f, "
           "\"dep_us\": %.1f, \"dep_adds_per_us\": %.1f, \"dep_latency_us_per_wave_add\": %.3f, "
           "\"free_us\": %.1f, \"free_adds_per_us\": %.1f, \"counts_exact\": %s}\n",
           cus, 4 * cus, adds, dep_us, adds / dep_us, dep_us / iters, free_us, adds / free_us, ok ? "true" : "false");
    return ok ? 0 : 2;
}
