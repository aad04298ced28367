// ce_stream.hpp -- the streaming mc kernel (stage 1 of ce_select_mc, q <= 64).
//
// One pass over the committee tensor at HBM rate.  Every wave is independent
// while streaming (no block barriers in the loop): it owns a contiguous run of
// 64-item tiles, scores one item per lane, and keeps its own top-q candidates
// in registers (RegTopQ, one list slot per lane).  The block's four wave
// lists are merged once at the end.
//
// Item-major [N, M, C] tensors (each item's M*C values contiguous, R bytes)
// are staged through LDS: a wave's 64 x R-byte tile arrives by LDS-DMA
// (global_load_lds_dwordx4, 1 KiB per instruction, fully coalesced); each
// lane then reads its own item with ds_read_b128.  The 16-B chunks of row r
// are stored XOR-swizzled (chunk m at slot m ^ (r & 15), done on the SOURCE
// address since the DMA writes LDS linearly) so the 16 lanes of a
// ds_read_b128 group hit 16 different bank groups.  As soon as the tile sits
// in registers the next tile's DMA is issued into the same buffer, so the
// f64 arithmetic of tile t overlaps the HBM fetch of tile t+1.
// Member-major / strided tensors load straight to registers (coalesced across
// lanes for the reference's [M, N, C] stack).
//
// Holds ItemTile, StreamArgs and the three kernels k_stream_nmc,
// k_stream_direct (ce_launch_stream.o instantiates both) and k_stream_seg
// (ce_launch_small.o).  The wave primitives are in ce_wave.hpp, the fold's
// merge in ce_merge.hpp, the wide-class stream in ce_wide_stream.hpp.
#pragma once
#include "ce_device.hpp"
#include "ce_merge.hpp"  // fold_merge
#include "ce_topq.hpp"
#include "ce_wave.hpp"
#include "ce_ws.hpp"

namespace ce {

// ---------------------------------------------------------------------------
// Item-major tile: S 16-B chunks per item (R = 16 S bytes), 64 items per tile.
// ---------------------------------------------------------------------------
template <int S>
struct ItemTile {
    uint32_t u[S * 4];  // this lane's item, raw bytes, member-major [M][C]

    // LDS-DMA the 64-row tile starting at item t0 (rows >= n_valid re-read row
    // n_valid-1, a harmless in-bounds duplicate) into `lds` (64*16*S bytes).
    // AUX = cache-policy bits of the load (0 default, 2 = nt: the pool is
    // streamed once, so it need not displace anything in L2 / MALL).
    template <int AUX>
    __device__ __forceinline__ static void issue(const char* base, int64_t t0, int n_valid, char* lds) {
        const int lane = threadIdx.x & 63;
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const int p = k * 64 + lane;  // 16-B chunk index within the tile
            const int r = p / S, s = p % S;
            const int rs = r < n_valid ? r : n_valid - 1;
            const int m = s ^ (r & 15);
            const char* src = base + (t0 + rs) * (int64_t)(16 * S) + 16 * m;
            __builtin_amdgcn_global_load_lds(
                (const void*)src, (void __attribute__((address_space(3)))*)(lds + k * 1024), 16, 0, AUX);
        }
    }

    // Member-major [M, N, C] (the reference's stack np.array(pred_prob),
    // amg_test.py:441) with 16-B member rows (C * elem = 16): the tile is S = M
    // contiguous 1 KiB runs, member k's 64 items at lds + k*1024 -- one
    // LDS-DMA per member, no swizzle (lane l reads bytes l*16.. of each run:
    // 16 lanes of a ds_read_b128 group hit 16 distinct bank groups).
    template <int AUX>
    __device__ __forceinline__ static void issue_mnc(const char* base, int64_t t0, int n_valid, int64_t sMb,
                                                     char* lds) {
        const int lane = threadIdx.x & 63;
        const int64_t it = t0 + (lane < n_valid ? lane : n_valid - 1);
#pragma unroll
        for (int k = 0; k < S; ++k) {
            const char* src = base + (int64_t)k * sMb + it * 16;
            __builtin_amdgcn_global_load_lds(
                (const void*)src, (void __attribute__((address_space(3)))*)(lds + k * 1024), 16, 0, AUX);
        }
    }

    __device__ __forceinline__ void read_mnc(const char* lds) {
        const int lane = threadIdx.x & 63;
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(lds + m * 1024 + lane * 16);
            u[4 * m + 0] = v.x;
            u[4 * m + 1] = v.y;
            u[4 * m + 2] = v.z;
            u[4 * m + 3] = v.w;
        }
    }

    __device__ __forceinline__ void read(const char* lds) {
        const int lane = threadIdx.x & 63;
        typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
#pragma unroll
        for (int m = 0; m < S; ++m) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(lds + lane * 16 * S + 16 * (m ^ (lane & 15)));
            u[4 * m + 0] = v.x;
            u[4 * m + 1] = v.y;
            u[4 * m + 2] = v.z;
            u[4 * m + 3] = v.w;
        }
    }

    // element e (= m*C + c) widened to f64
    template <int DT>
    __device__ __forceinline__ double elem(int e) const {
        if constexpr (DT == kF32)
            return (double)__uint_as_float(u[e]);
        else if constexpr (DT == kF64)
            return __longlong_as_double((long long)(((uint64_t)u[2 * e + 1] << 32) | u[2 * e]));
        else
            return bf16_to_f64((u[e >> 1] >> (16 * (e & 1))) & 0xffffu);
    }

    // amg_test.py:441 for this lane's item: member-sequential f64 sum, / M
    template <int DT, int C>
    __device__ __forceinline__ void mean(double dM, double invM, bool pow2, double (&mean)[C]) const {
        constexpr int EB = DT == kF64 ? 8 : (DT == kF32 ? 4 : 2);
        constexpr int M = 16 * S / (C * EB);
        static_assert(M * C * EB == 16 * S, "tile row must hold whole members");
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0;
#pragma unroll
        for (int m = 0; m < M; ++m)
#pragma unroll
            for (int c = 0; c < C; ++c) acc[c] += elem<DT>(m * C + c);
#pragma unroll
        for (int c = 0; c < C; ++c) mean[c] = div_members(acc[c], dM, invM, pow2);
    }
};

template <int S, int RING = 1>
struct StreamSmemNMC {
    char tile[4][RING][64 * 16 * S];  // RING staging tiles per wave
    WaveLists lists;
};

struct StreamArgs {
    const void* p;
    int64_t N;
    int M;
    int64_t sN, sM, sC;
    double dM, invM;
    bool pow2;
    int64_t base_idx;
    int64_t per_wave;  // items per wave (multiple of 64)
    const uint32_t* excl;  // exclusion bitmap over items 0..N-1 (1 = out of the pool), or nullptr
    int nlists;        // workspace lists (>= gridDim.x); lists past the grid are written empty
    // stage 2 folded in (ctr != nullptr): the last block merges the grid's
    // lists into (oval, oidx), or into q records at ocand
    uint32_t* ctr;
    double* oval;
    int64_t* oidx;
    Cand* ocand;
    const Cand* extra;  // one more list merged by the fold (chunked jobs: the running list), or nullptr
    // the wide stream's device-side grid choice (heavy items in a folded launch,
    // k_wide_seed_pick): both grids are launched, the one whose role disagrees with
    // the vote exits at once (nullptr: no vote, the kernel runs)
    const uint32_t* vote;
    int vote_heavy;  // 1: run iff the vote picks the deep-ring grid; 0: iff it does not
    // the wide stream's prefilter floor (k_wide_seed_pick), one record, or nullptr
    // (then a chunked job's running list seeds it: extra[q - 1])
    const Cand* seed;
    // ordered tile claims (k_stream_nmc, folded item-major launches with two ring
    // slots): the workspace header's claim word (ce_ws.hpp, kWsClaimSlot), or
    // nullptr for the static grid-cyclic order; claim_from >= 4: the grid-cyclic
    // rounds (tiles per wave) every wave takes statically before it claims
    uint32_t* claim;
    int64_t claim_from;
};

// One tile of k_stream_nmc, in registers: this lane's item t0 + lane (of the
// wave's range, which ends at hi) scored, screened by the bitmap and offered to
// the wave's list.
template <int DT, int C, int S>
__device__ __forceinline__ void score_tile(const ItemTile<S>& t, const StreamArgs& a, int64_t t0, int64_t hi,
                                           RegTopQ& tq) {
    double mean[C];
    t.template mean<DT, C>(a.dM, a.invM, a.pow2, mean);
    const double h = entropy_row<C>(mean);
    const int64_t i = t0 + (threadIdx.x & 63);
    bool ok = i < hi;
    if (a.excl) ok = ok && !excluded(a.excl, i < hi ? i : hi - 1);
    tq.offer(order_key(h), i + a.base_idx, ok);
}

// Tiles per claimed unit of the ordered-claim order (2, 4 or 8; 0: the launcher
// never claims).  The choice is measured: profiles/stream_launch_phases.json.
#ifndef CE_STREAM_CLAIM_K
#define CE_STREAM_CLAIM_K 8
#endif

#ifdef CE_STREAM_STAMPS
// diagnostic build only (-DCE_STREAM_STAMPS, make stamps): per-wave wall-clock
// stamps (100 MHz) of k_stream_nmc, one row per wave of the grid:
// [0] first DMA issue, [1] last tile landed, [2] end of block_merge_write,
// [3] end of fold_merge (the last block's waves; 0 elsewhere), [4] tiles scored,
// [5] samples taken, then kStampSamples pairs {stamp, tile index} taken every
// `every` tiles of the wave (every = ceil(tiles per wave / kStampSamples)).
// The samples wait in LDS and are written out after the stream: no store
// enters the loop's vmcnt queue.
constexpr int kStampWaves = 4096, kStampSamples = 12, kStampCols = 6 + 2 * kStampSamples;
__device__ uint64_t g_stream_stamps[kStampWaves][kStampCols];
struct StreamStampSmem {
    uint64_t s[4][2 * kStampSamples];
};
#endif

// Item-major, dense rows of 16*S bytes, LDS-DMA staged (AUX: DMA cache policy);
// MNC: the member-major stack with 16-B member rows instead (S = M members,
// member stride a.sM elements).
// RING tiles per wave: 2 (the default for 16-KiB tiles) puts the next two
// tiles in flight while one is read -- 139 KB of LDS, so ONE block (4 waves)
// per CU instead of 2 blocks with one tile each: the same bytes in flight from
// half as many streams.  Measured on one box, alternating (profiles/
// r05_nmc_ring_ab.json): [N,M,C] 0.856-0.860 -> 0.883-0.884 of HBM, [M,N,C]
// 0.835 -> 0.846.
//
// Two tile orders.  Static (a.claim == nullptr: unfolded launches, the
// member-major stack, one ring slot): every wave computes its tiles from
// blockIdx.  Ordered claims (a.claim: folded item-major launches with two ring
// slots -- MCPlan.step / step_cands, the bench kernel): wave g takes tiles g, g +
// W, ... grid-cyclically for the first a.claim_from rounds (W = the grid's
// waves); the rest of the pool, from tile T0 = claim_from * W, is cut into units
// of K = CE_STREAM_CLAIM_K adjacent tiles, and a wave's next unit is T0 / K + v, v
// the value a returning agent-scope add of 1 on the workspace's claim word gave
// it.  Why: the waves do not keep step.  Stamped (profiles/
// stream_launch_phases.json), the static order's waves land their last tile over
// a span of 10 to 14 % of the launch, and the launch ends with its slowest wave,
// 6 % after the median one.  Claimed units go in pool order to whichever wave
// asks next, so the fast waves take more of the end of the pool and no wave ends
// more than one unit after the pool is exhausted.  No spinning, no wait between
// waves: a wave whose tile lies past the end drains its ring and goes to the
// merge; the grid's last block (fold_merge) stores the word back to zero.  Which
// wave scored an item does not matter to the result: the lists' order is total
// (NaN first, entropy descending, lowest position) and positions come from the
// tile index.
// Only the end of the pool is claimed, for two measured reasons: one word takes
// 88 returning adds per microsecond, fewer than the whole stream would make at K
// = 2 or 4 and less than twice what it would make at K = 8; and the compiler
// puts s_waitcnt vmcnt(0) in front of the first use of a claimed index (an
// LDS-DMA is a FLAT instruction that touches LDS and memory; with one pending
// its wait insertion drains the counter for any tracked result), which empties
// the ring once per claimed unit.  The static rounds never run that wait.
//
// The claim path's vmcnt queue (in-order return; S DMA instructions per tile,
// always: short tiles re-read their last row).  The wave scores positions p = 0,
// 1, ... of its tile sequence (ring slot p & 1); an issue cursor runs two
// positions ahead.  At position p the wave issues, in this order,
//     [a claim, when position p + 2 is a claimed unit's first tile, or the
//      static round claim_from - 2]                              DMA(p + 2)
// so at the wait of position p the queue holds, oldest first,
//     ... claim? DMA(p) | claim (issued at p - 1)? DMA(p + 1)
// and tile p has landed once at most S (+ 1 when position p - 1 issued a claim)
// instructions are outstanding.  A claim issued at position p is for the unit
// the cursor enters at position p + K (p + 2 for the first): it went out ahead
// of DMA(p + 2), which is DMA(p + K) or older, so the wait for tile p + K is also
// the wait for the claimed index.  One claim is in flight per wave at a time.
template <int DT, int C, int S, int AUX, bool MNC = false, int RING = 1>
__global__ __launch_bounds__(256) void k_stream_nmc(StreamArgs a, int q, Cand* __restrict__ wc) {
    static_assert(RING == 1 || RING == 2, "one or two tiles per wave");
    CE_DASSERT((int)gridDim.x <= a.nlists && q >= 1 && q <= kStreamMaxQ);
    __shared__ __attribute__((aligned(16))) StreamSmemNMC<S, RING> sm;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    RegTopQ tq;
    tq.init(q);
    const char* base = static_cast<const char*>(a.p);
    constexpr int EB = DT == kF64 ? 8 : (DT == kF32 ? 4 : 2);
    const int64_t sMb = a.sM * EB;
    auto issue = [&](int64_t t, int nv, int slot) {
        char* lds = sm.tile[w][slot];
        if constexpr (MNC) ItemTile<S>::template issue_mnc<AUX>(base, t, nv, sMb, lds);
        else ItemTile<S>::template issue<AUX>(base, t, nv, lds);
    };
    ItemTile<S> t;
#ifdef CE_STREAM_STAMPS
    __shared__ StreamStampSmem stamps;
    const int64_t gw = (int64_t)blockIdx.x * 4 + w;
    const int64_t st_waves = (int64_t)gridDim.x * 4;
    const int64_t st_every = max<int64_t>(1, (((a.N + 63) / 64 + st_waves - 1) / st_waves + kStampSamples - 1) / kStampSamples);
    int64_t st_it = 0;
    int st_n = 0;
    uint64_t st_landed = 0;
    uint64_t st_first = 0;
#define CE_SSAMPLE(tile_)                                            \
    {                                                                \
        if (st_it % st_every == 0 && st_n < kStampSamples) {         \
            if (lane == 0) {                                         \
                stamps.s[w][2 * st_n] = wall_clock64();              \
                stamps.s[w][2 * st_n + 1] = (uint64_t)(tile_);       \
            }                                                        \
            ++st_n;                                                  \
        }                                                            \
        ++st_it;                                                     \
    }
#define CE_SLANDED(last_) \
    if (last_) st_landed = wall_clock64();
#define CE_SSTAMP(col_) \
    if (lane == 0 && gw < kStampWaves) g_stream_stamps[gw][col_] = wall_clock64();
#define CE_SFIRST() st_first = wall_clock64();
#else
#define CE_SSAMPLE(tile_)
#define CE_SLANDED(last_)
#define CE_SSTAMP(col_)
#define CE_SFIRST()
#endif
    bool claims = false;
    if constexpr (!MNC && RING == 2 && CE_STREAM_CLAIM_K > 0) claims = a.claim != nullptr;  // grid-uniform
    if (claims) {
        if constexpr (!MNC && RING == 2 && CE_STREAM_CLAIM_K > 0) {
            constexpr int K = CE_STREAM_CLAIM_K;
            static_assert(K == 2 || K == 4 || K == 8, "an even number of tiles per unit");
            // the wave's number as a scalar: the cursor below lives in scalar registers
            const int wu = __builtin_amdgcn_readfirstlane(w);
            const int64_t nt = (a.N + 63) >> 6;  // tiles of the pool; a tile index >= nt: none
            const int64_t W = (int64_t)gridDim.x * 4, g = (int64_t)blockIdx.x * 4 + wu, R = a.claim_from;
            const int64_t T0 = R * W;  // the first claimed tile
            CE_DASSERT(R >= 4);
            // positions 0 and 1 (rounds 0 and 1) go out before the log table is staged:
            // the table's loads overlap the first fetch
            int64_t ta = min<int64_t>(g, nt), tb = min<int64_t>(g + W, nt);
            CE_SFIRST()
            if (ta < nt) issue(ta * 64, (int)min<int64_t>(64, a.N - ta * 64), 0);
            if (tb < nt) issue(tb * 64, (int)min<int64_t>(64, a.N - tb * 64), 1);
            stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
            // the issue cursor, two positions ahead of the tile being scored: js static
            // rounds handed out so far, then (claimed) tile isub of the unit at ibase
            int64_t js = 2, ibase = nt;
            int isub = 0, slot = 0;
            bool claimed = false, dead = false;  // dead: the cursor is past the pool's end (for good: tiles ascend)
            uint32_t c = 0;                      // the claim in flight (lane 0)
            bool claimed_prev = false;
            while (ta < nt) {  // position p: tile ta in ring slot `slot`
                if (tb < nt) {
                    if (claimed_prev) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S + 1) : "memory");
                    else asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S) : "memory");
                } else {
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the wave's last tile: drain
                }
                CE_SLANDED(tb >= nt)
                t.read(sm.tile[w][slot]);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                // the cursor moves to position p + 2
                int64_t tc;
                bool want;  // a claim goes out with this position
                if (js < R) {  // static rounds; the first claim two positions before its use
                    tc = g + js * W;
                    want = js == R - 2;
                    ++js;
                } else {
                    if (!claimed || ++isub == K) {  // into the first / the next claimed unit
                        claimed = true;
                        isub = 0;
                        ibase = dead ? nt : T0 + (int64_t)K * (int64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)c);
                    }
                    tc = ibase + isub;
                    want = isub == 0;  // the claim for the unit after this one: K >= 2 positions ahead
                }
                if (tc >= nt) {
                    tc = nt;
                    dead = true;
                }
                // (atomic_inc with no wrap, arrive_last's builtin: a returning add of 1
                // that the compiler's wave-level atomic combining leaves alone -- that
                // pass would follow the add with a wait for its result)
                claimed_prev = want && !dead;
                if (claimed_prev && lane == 0)
                    c = __builtin_amdgcn_atomic_inc32(a.claim, 0xffffffffu, __ATOMIC_RELAXED, "agent");
                if (tc < nt) issue(tc * 64, (int)min<int64_t>(64, a.N - tc * 64), slot);
                slot ^= 1;
                CE_SSAMPLE(ta)
                score_tile<DT, C, S>(t, a, ta * 64, a.N, tq);
                ta = tb;
                tb = tc;
            }
        }
    } else {
        stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
        int64_t lo, hi, step;
        // tile distribution (measured on two boxes, alternating runs,
        // profiles/r03_tile_order.json): item-major -- grid-cyclic, equal on a box
        // where a contiguous run per wave reaches 0.871 and +2.5 % (0.836 -> 0.859)
        // on one where it reaches only 0.836; member-major -- block-interleaved
        // (+0.3-0.5 % over runs), grid-cyclic 4 % slower there
        if constexpr (!MNC) {  // grid-cyclic: wave g takes tiles g, g + W, g + 2W, ... (W = the grid's waves), so
            // the tiles in flight at any moment form one contiguous sweep of the pool
            const int64_t W = (int64_t)gridDim.x * 4;
            lo = ((int64_t)blockIdx.x * 4 + w) * 64;
            hi = a.N;
            step = W * 64;
        } else {  // the block's 4 waves take alternate tiles of the block's run (adjacent bursts per member row;
            // 8 or 64 grid-cyclic sweeps, each over 1/8 or 1/64 of the pool, measured no better: r04_mnc_order.json)
            const int64_t blo = (int64_t)blockIdx.x * 4 * a.per_wave;
            hi = blo + 4 * a.per_wave < a.N ? blo + 4 * a.per_wave : a.N;
            lo = blo + 64 * w;
            step = 256;
        }
        if (lo > hi) lo = hi;
        CE_SFIRST()
#pragma unroll
        for (int r = 0; r < RING; ++r)
            if (lo + r * step < hi) issue(lo + r * step, (int)min<int64_t>(64, hi - lo - r * step), r);
        int slot = 0;
        for (int64_t t0 = lo; t0 < hi; t0 += step) {
            // S DMA instructions per tile (always: short tiles re-read their last row),
            // so the tiles issued after this one are (RING - 1) * S instructions
            if constexpr (RING == 2) {
                if (t0 + step < hi) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(S) : "memory");
                else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            CE_SLANDED(!(t0 + step < hi))
            const char* lds = sm.tile[w][slot];
            if constexpr (MNC) t.read_mnc(lds);
            else t.read(lds);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
            const int64_t t1 = t0 + RING * step;
            if (t1 < hi) issue(t1, (int)min<int64_t>(64, hi - t1), slot);
            slot = RING == 1 ? 0 : slot ^ 1;
            CE_SSAMPLE(t0 / 64)
            score_tile<DT, C, S>(t, a, t0, hi, tq);
        }
    }
#ifdef CE_STREAM_STAMPS
    if (lane == 0 && gw < kStampWaves) {
        uint64_t* row = g_stream_stamps[gw];
        row[0] = st_first;
        row[1] = st_landed;
        row[3] = 0;
        row[4] = (uint64_t)st_it;
        row[5] = (uint64_t)st_n;
        for (int k = 0; k < 2 * kStampSamples; ++k) row[6 + k] = k < 2 * st_n ? stamps.s[w][k] : 0;
    }
#endif
    block_merge_write<4>(tq, sm.lists, q, wc + (int64_t)blockIdx.x * q, a.nlists, nullptr, nullptr, 4, a.ctr != nullptr);
    CE_SSTAMP(2)
    if (a.ctr) fold_merge<4>(a.ctr, a.oval, a.oidx, a.ocand, q, wc, sm.lists, a.extra, claims ? a.claim : nullptr);
    CE_SSTAMP(3)
#undef CE_SSAMPLE
#undef CE_SLANDED
#undef CE_SSTAMP
#undef CE_SFIRST
}

// Any strides (vector loads when aligned): member-major [M, N, C] streams
// coalesced across lanes.  IPL items per lane per iteration keep IPL x M
// member loads in flight per lane.
template <class Src, int IPL, int UNR>
__device__ __forceinline__ void stream_direct_range(const Src& src, int64_t lo, int64_t hi, int64_t rel, int q,
                                                    RegTopQ& tq, const uint32_t* excl = nullptr) {
    const int lane = threadIdx.x & 63;
    for (int64_t t0 = lo; t0 < hi; t0 += 64 * IPL) {
        uint64_t k[IPL];
        int64_t items[IPL];
#pragma unroll
        for (int u = 0; u < IPL; ++u) {
            const int64_t i = t0 + 64 * u + lane;
            items[u] = i < hi ? i : hi - 1;  // clamped: every lane loads, no branch per item
        }
        src.template keys<UNR, IPL>(items, k);
#pragma unroll
        for (int u = 0; u < IPL; ++u) {
            const int64_t i = t0 + 64 * u + lane;
            bool ok = i < hi;
            if (excl) ok = ok && !excluded(excl, items[u]);  // items[u]: i clamped into the pool
            tq.offer(k[u], i + rel, ok);
        }
    }
}

template <class Src, int IPL, int UNR>
__global__ __launch_bounds__(256) void k_stream_direct(Src src, StreamArgs a, int q, Cand* __restrict__ wc) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    CE_DASSERT((int)gridDim.x <= a.nlists && q >= 1 && q <= kStreamMaxQ);
    __shared__ WaveLists sm;
    const int w = threadIdx.x >> 6;
    const int64_t gw = (int64_t)blockIdx.x * 4 + w;
    int64_t lo = gw * a.per_wave;
    int64_t hi = lo + a.per_wave;
    if (hi > a.N) hi = a.N;
    if (lo > hi) lo = hi;
    RegTopQ tq;
    tq.init(q);
    stream_direct_range<Src, IPL, UNR>(src, lo, hi, a.base_idx, q, tq, a.excl);
    block_merge_write<4>(tq, sm, q, wc + (int64_t)blockIdx.x * q, a.nlists, nullptr, nullptr, 4, a.ctr != nullptr);
    if (a.ctr) fold_merge<4>(a.ctr, a.oval, a.oidx, a.ocand, q, wc, sm, a.extra);
}

// Batched pools (amg_test.py:345's per-user loop in one launch): user u owns
// segment [offsets[u], offsets[u+1]), split over bpu consecutive blocks (block
// b: user b / bpu, part b % bpu) in whole iterations of 64*IPL items; the
// block's waves split its part the same way.  bpu == 1: the block's merged
// top-q is the user's final answer (oval/oidx, user-local positions); bpu > 1:
// the block writes its list to wc[b*q ..] for a per-user merge.
// offsets == nullptr: one segment [0, n) with positions base_idx + i (the
// single-launch path for small pools).  excl: exclusion bitmap over the
// tensor's items, or nullptr.  Launched with WAVES or fewer waves (a power of two).
template <class Src, int IPL, int UNR, int WAVES>
__global__ __launch_bounds__(64 * WAVES) void k_stream_seg(Src src, const int64_t* __restrict__ offsets, int64_t n,
                                                            int64_t base_idx, int q, int bpu,
                                                            double* __restrict__ oval, int64_t* __restrict__ oidx,
                                                            Cand* __restrict__ wc, const uint32_t* __restrict__ excl) {
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    __shared__ WaveListsT<WAVES> sm;
    __shared__ uint64_t fk_s[4 * WAVES];
    __shared__ int64_t fi_s[4 * WAVES];
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6, lane = threadIdx.x & 63;
    const int u = blockIdx.x / bpu, part = blockIdx.x % bpu;
    const int64_t s0 = offsets ? offsets[u] : 0, s1 = offsets ? offsets[u + 1] : n;
    const int64_t len = s1 > s0 ? s1 - s0 : 0;
    constexpr int64_t kIt = 64 * IPL;
    const int64_t its = (len + kIt - 1) / kIt;                  // iterations of the segment
    const int64_t its_b = (its + bpu - 1) / bpu;                // per block
    const int64_t its_w = (its_b + nw - 1) / nw;                // per wave
    int64_t lo = s0 + ((int64_t)part * its_b + (int64_t)w * its_w) * kIt;
    int64_t hi_b = s0 + ((int64_t)part + 1) * its_b * kIt;      // this block's end
    if (hi_b > s1) hi_b = s1;
    int64_t hi = lo + its_w * kIt < hi_b ? lo + its_w * kIt : hi_b;
    if (lo > hi) lo = hi;
    const int64_t rel = (offsets ? 0 : base_idx) - s0;
    // First iteration's keys, then a block-wide floor before any offer: the
    // best of each 16-lane row is a distinct item, so the q-th best of the
    // block's 4*nw row bests is an exact lower bound (q items of the block's
    // part are >= it).  Most candidates then fail the first ballot and the
    // sort networks a cold wave list would run on every early batch are skipped.
    uint64_t k0[IPL];
    int64_t it0[IPL];
    bool ok0[IPL];
#pragma unroll
    for (int v = 0; v < IPL; ++v) {
        const int64_t i = lo + 64 * v + lane;
        it0[v] = i < hi ? i : hi - 1;
        ok0[v] = false;
        k0[v] = 0;
    }
    if (lo < hi) {  // wave-uniform
        src.template keys<UNR, IPL>(it0, k0);
#pragma unroll
        for (int v = 0; v < IPL; ++v) {
            ok0[v] = lo + 64 * v + lane < hi;
            if (excl) ok0[v] = ok0[v] && !excluded(excl, it0[v]);
        }
    }
    uint64_t bk = 0;
    int64_t bi = INT64_MAX;
#pragma unroll
    for (int v = 0; v < IPL; ++v)
        if (ok0[v] && better(k0[v], lo + 64 * v + lane + rel, bk, bi)) {
            bk = k0[v];
            bi = lo + 64 * v + lane + rel;
        }
    row_best16(bk, bi);
    if ((lane & 15) == 0) {
        fk_s[w * 4 + (lane >> 4)] = bk;
        fi_s[w * 4 + (lane >> 4)] = bi;
    }
    __syncthreads();
    uint64_t fk = 0;
    int64_t fi = INT64_MAX;
    const int nb = 4 * nw;
    if (q <= nb) {
        bool hit = false;
        uint64_t vk = 0;
        int64_t vi = INT64_MAX;
        if (lane < nb) {
            vk = fk_s[lane];
            vi = fi_s[lane];
            int rank = 0;
            for (int v = 0; v < nb; ++v) rank += better(fk_s[v], fi_s[v], vk, vi);
            hit = vi != INT64_MAX && rank == q - 1;
        }
        const uint64_t m = __ballot(hit);
        if (m) {
            const int sl = __builtin_ctzll(m);
            fk = readlane64(vk, sl);
            fi = (int64_t)readlane64((uint64_t)vi, sl) + 1;  // admit candidates >= the bound
        }
    }
    RegTopQ tq;
    tq.init(q, fk, fi);
#pragma unroll
    for (int v = 0; v < IPL; ++v) tq.offer(k0[v], lo + 64 * v + lane + rel, ok0[v]);
    if (lo + kIt < hi) stream_direct_range<Src, IPL, UNR>(src, lo + kIt, hi, rel, q, tq, excl);
    if (bpu == 1) {
        const int64_t slot = (int64_t)u * q;
        block_merge_write<WAVES>(tq, sm, q, nullptr, 0, oval + slot, oidx + slot, nw);
    } else {
        block_merge_write<WAVES>(tq, sm, q, wc + (int64_t)blockIdx.x * q, 0, nullptr, nullptr, nw);
    }
}

}  // namespace ce
