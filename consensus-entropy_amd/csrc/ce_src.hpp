// ce_src.hpp -- the item sources the scoring kernels are templated on: key(i)
// returns the order key of global item i.  CommitteeSrc (a committee tensor of
// any strides: mean, keys, and rows_small for the single-block pools, with
// kSmallThrottle, its default slot throttle), ArraySrc (precomputed entropies)
// and TableSrc (hc frequency rows).  No kernel here: the sources are arguments
// of k_partial, k_stream_direct, k_stream_seg, k_select_tiles and k_entropy,
// each instantiated by the one object that launches it.
#pragma once
#include <type_traits>

#include "ce_device.hpp"
#include "ce_wave.hpp"  // NoHook

namespace ce {

// item slots a lane keeps in flight in the single-block pools (rows_small).
// Measured on configs[2] (500 users x 1608, f32): all at once 14.24 us,
// 1 slot 13.52 us, 2 slots 14.68 us
// Round 4, after the approximate prefilter (profiles/r04_small_phase_prefilter.json):
// 1 slot 10.74 us, 2 slots 10.98 us, all 16-23 us (register spills);
// the last short slot issued with slot 0: C1 6.12 -> 6.42 us, C3 even; the
// single-pool launches with 2 / all slots in flight: C1 5.86 -> 6.04 / 6.68 us,
// the mix 6.6 -> 6.92 / 6.94 us.
#ifndef CE_SMALL_THR
#define CE_SMALL_THR 1
#endif
constexpr int kSmallThrottle = CE_SMALL_THR;

// ---------------------------------------------------------------------------
// Item sources.  key(i) returns the order key of global item i.
// ---------------------------------------------------------------------------
template <int DT, int C, bool VEC>
struct CommitteeSrc {
    const void* p;
    int64_t sN, sM, sC;
    int M;
    double dM, invM;
    bool pow2;
    static constexpr int kC = C;
    static constexpr int kDT = DT;
    static constexpr bool kVec = VEC;
    static constexpr int kUnr = DT == kF64 ? 4 : 8;
    __device__ __forceinline__ void mean(int64_t i, double (&m)[C]) const {
        committee_mean<DT, C, VEC, kUnr>(p, i * sN, M, sM, sC, dM, invM, pow2, m);
    }
    // IPL items at once: all their member loads in flight together
    // hook() runs after the means, before the first log (e.g. LogTablePrefetch::commit)
    template <int UNR, int IPL, class Hook = NoHook>
    __device__ __forceinline__ void keys(const int64_t (&items)[IPL], uint64_t (&k)[IPL], Hook hook = {}) const {
        int64_t offs[IPL];
#pragma unroll
        for (int u = 0; u < IPL; ++u) offs[u] = items[u] * sN;
        double m[IPL][C];
        committee_mean_multi<DT, C, VEC, UNR, IPL>(p, offs, M, sM, sC, dM, invM, pow2, m);
        hook();
#pragma unroll
        for (int u = 0; u < IPL; ++u) k[u] = order_key(entropy_row<C>(m[u]));
    }
    // The exact consensus rows (amg_test.py:441) of IPL item slots for the
    // latency-bound single-block pools: sink(u, m) receives slot u's row, for
    // u < nlive only (wave-uniform: no lane of the wave owns a real item at u
    // >= nlive).  When the whole committee fits one batch (M <= UNR) the loads
    // are issued item by item and each item's mean runs as soon as ITS loads
    // have landed.  Every slot's loads are issued, also for slots without a
    // real item (their addresses are clamped to the pool's last item: one
    // cache line per wave): loads under a branch leave the compiler unable to
    // count them, and it then waits for ALL of them (vmcnt(0)) before the log
    // table's commit.  hook() runs after the first means (e.g.
    // LogTablePrefetch::commit).
    template <int UNR, int IPL, class Sink, class Hook = NoHook, int THR = kSmallThrottle>
    __device__ __forceinline__ void rows_small(const int64_t (&items)[IPL], int nlive, Sink&& sink,
                                               Hook hook = {}) const {
        if (M > UNR) {
            // committees larger than one batch: f32 rows keep all IPL items' member
            // batches in flight (IPL x UNR x 4 VGPRs); f64 rows of C >= 4 would need
            // twice that, so they go item by item (UNR members in flight)
            if constexpr (!(DT == kF64 && C >= 4)) {
                int64_t offs[IPL];
#pragma unroll
                for (int u = 0; u < IPL; ++u) offs[u] = items[u] * sN;
                double m[IPL][C];
                committee_mean_multi<DT, C, VEC, UNR, IPL>(p, offs, M, sM, sC, dM, invM, pow2, m);
                hook();
#pragma unroll
                for (int u = 0; u < IPL; ++u)
                    if (u < nlive) sink(u, m[u]);
                return;
            }
#pragma unroll
            for (int u = 0; u < IPL; ++u) {
                double m[C];
                committee_mean<DT, C, VEC, UNR>(p, items[u] * sN, M, sM, sC, dM, invM, pow2, m);
                if (u == 0) hook();
                if (u < nlive) sink(u, m);
            }
            return;
        }
        MemberLoad<DT, C, VEC> ld[IPL][UNR];
        auto issue = [&](int u) {
#pragma unroll
            for (int v = 0; v < UNR; ++v) ld[u][v].load(p, items[u] * sN + (int64_t)(v < M ? v : M - 1) * sM, sC);
        };
        // THR item slots in flight per lane (THR < IPL: slot u + THR is issued
        // only once slot u has landed, so every block keeps a bounded share of
        // the memory queues instead of all of its bytes at once)
        constexpr int D = (THR > 0 && THR < IPL) ? THR : IPL;
#pragma unroll
        for (int i = 0; i < D; ++i) issue(i);
        hook();
        auto item = [&](auto full) {
#pragma unroll
            for (int i = 0; i < IPL; ++i) {
                const int u = i;
                if constexpr (D < IPL) {
                    if (i + D < IPL) {
                        // slot u landed (the asm reads its registers: the compiler waits
                        // for exactly those loads), then the next slot is issued; the
                        // memory clobber keeps that issue behind the wait
#pragma unroll
                        for (int v = 0; v < UNR; ++v) ld[u][v].pin();
                        asm volatile("" ::: "memory");
                        issue(i + D);
                    }
                }
                if (u >= nlive) continue;  // wave-uniform
                double acc[C];
#pragma unroll
                for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll
                for (int v = 0; v < UNR; ++v) {
                    if constexpr (decltype(full)::value) ld[u][v].add_to(acc);  // M == UNR: no padding
                    else ld[u][v].add_masked(acc, v < M);
                }
                double m[C];
#pragma unroll
                for (int c = 0; c < C; ++c) m[c] = div_members(acc[c], dM, invM, pow2);
                sink(u, m);
            }
        };
        if (M == UNR) item(std::true_type());
        else item(std::false_type());
    }
    __device__ __forceinline__ double entropy(int64_t i) const {
        double m[C];
        mean(i, m);
        return entropy_row<C>(m);
    }
    __device__ __forceinline__ uint64_t key(int64_t i) const { return order_key(entropy(i)); }
};

struct ArraySrc {  // precomputed entropies
    const double* e;
    __device__ __forceinline__ uint64_t key(int64_t i) const { return order_key(e[i]); }
};

template <int C>
struct TableSrc {  // hc frequency table rows [N_h, C] f64 (amg_test.py:451)
    const double* t;
    int64_t ld;
    __device__ __forceinline__ uint64_t key(int64_t i) const {
        double row[C];
#pragma unroll
        for (int c = 0; c < C; ++c) row[c] = t[i * ld + c];
        return order_key(entropy_row<C>(row));
    }
};

}  // namespace ce
