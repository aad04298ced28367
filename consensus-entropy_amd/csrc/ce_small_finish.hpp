// ce_small_finish.hpp -- steps 2-4 of ce_small.hpp's header comment (floor,
// survivors' append, exact entropies + ranks, overflow branch): ONE text for
// k_select_tiles and select_tile (k_select_tiles_mix).
// A function-body FRAGMENT, not a header: no include guard, no declarations;
// ce_small.hpp includes it after step 1 of each.  Names it expects in scope:
// K, C, W, GS, BS, SM, sm, tid, w, lane, ntid, mrow, ak, sp, pos_of (local slot
// -> position), q, ov, oi.
// A fragment and not a function, because every function over the per-thread
// arrays (mrow, ak, sp) that was tried changed the ISA of every tile kernel
// (more VGPRs, new scratch), and configs[2] is pinned to that code; included
// twice, the text compiles to the code objects of the two copies it replaced,
// byte for byte (profiles/small_dedupe_codeobj.json).
#ifndef CE_SMALL_FINISH_FRAGMENT
#error "ce_small_finish.hpp is a function-body fragment: only ce_small.hpp includes it"
#endif
// 2. T = the group maximum of rank q-1 (with multiplicity): q distinct
//    items have approximate keys >= T
uint32_t bk = ak[0];
#pragma unroll
for (int v = 1; v < K; ++v) bk = bk > ak[v] ? bk : ak[v];
bk = group_max<GS>(bk);
if ((tid & (GS - 1)) == 0) sm.gm[tid / GS] = bk;
if (tid == 0) sm.cnt = 0;
__syncthreads();
const uint32_t mg = sm.gm[lane];
{
    int r = 0;
#pragma unroll
    for (int j = 0; j < 64 / W; ++j) {
        const uint32_t o = sm.gm[w * (64 / W) + j];
        r += (o > mg ? 1 : 0) + (o >= mg ? 0x10000 : 0);
    }
    sm.part[w][lane] = r;
}
__syncthreads();
uint32_t thr;  // survivors: approximate key >= thr (>= 1: never a slot without an item)
{
    int r = 0;
#pragma unroll
    for (int j = 0; j < W; ++j) r += sm.part[j][lane];
    const int above = r & 0xffff, notbelow = r >> 16;
    const int sl = __builtin_ctzll(__ballot(above < q && notbelow >= q));
    const uint32_t T = (uint32_t)__builtin_amdgcn_readlane((int)mg, sl);
    thr = 1;
    if (T != 0) {  // else fewer than q ordinary items: every item survives
        const float lim = approx_key_value(T) - 2.0f * kApproxErr2PerClass * C;
        const uint32_t b = __float_as_uint(lim);
        const uint32_t tk = (b >> 31) ? ~b : (b | 0x80000000u);
        thr = tk > 1 ? tk : 1;
    }
}
CE_STAMP(blockIdx.x, 2)
// 3. survivors -> LDS rows: the wave's K ballots first, then ONE atomic
//    per wave for all of its survivors
{
    bool pass[K];
    uint64_t msk[K];
    int tot = 0;
#pragma unroll
    for (int v = 0; v < K; ++v) {
        pass[v] = sp[v] | (ak[v] >= thr);
        msk[v] = __ballot(pass[v]);
        tot += __popcll(msk[v]);
    }
    if (tot) {  // wave-uniform
        int base = 0;
        if (lane == 0) base = atomicAdd(&sm.cnt, tot);
        base = __builtin_amdgcn_readfirstlane(base);
#pragma unroll
        for (int v = 0; v < K; ++v) {
            const int slot = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(msk[v] >> 32),
                                                              __builtin_amdgcn_mbcnt_lo((uint32_t)msk[v], 0));
            CE_DASSERT(slot >= 0);
            if (pass[v] && slot < SM::CAP) {
#pragma unroll
                for (int c = 0; c < C; ++c) sm.sv.m[c][slot] = mrow[v][c];
                sm.sv.nl[slot] = ntid - (uint32_t)(v * BS);  // ~(v * BS + tid)
            }
            base += __popcll(msk[v]);
        }
    }
}
__syncthreads();
CE_STAMP(blockIdx.x, 3)
const int nc = sm.cnt;
if (nc <= SM::CAP) {
    // 4. exact entropies of the survivors, P lanes per survivor (one
    //    class each: one glibc log per lane instead of C in a row --
    //    the wave issues each instruction once for all its lanes), the
    //    terms gathered by lane shuffles and summed in numpy's order;
    //    then ranks.  Up to 64/P survivors (the usual case) stay in
    //    wave 0: no second block barrier.
    constexpr int P = C <= 2 ? 2 : (C <= 4 ? 4 : 8);
    constexpr int SPW = 64 / P;
    static_assert(C <= 8, "single-block pools hold rows of <= 8 classes");
    CE_DASSERT(nc >= 0 && nc + 8 <= SM::CAP + 8);
    if (tid < 8) sm.cs[nc + tid] = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll 1
    for (int t0 = w * SPW; t0 < nc; t0 += W * SPW) {  // wave-uniform
        const int t = t0 + lane / P, c = lane % P;
        const int ts = t < nc ? t : 0;
        double x[C];
#pragma unroll
        for (int cc = 0; cc < C; ++cc) x[cc] = sm.sv.m[cc][ts];
        const double xc = sm.sv.m[c < C ? c : 0][ts];
        const double s = row_sum<C>(x);
        const double e = entr(row_quotient_one<C>(x, s, xc));
        double ee[C];
#pragma unroll
        for (int j = 0; j < C; ++j) ee[j] = __shfl(e, (lane & ~(P - 1)) + j);
        const uint64_t key = order_key(row_sum<C>(ee));
        CE_DASSERT(ts >= 0 && ts < SM::CAP);
        if (t < nc && c == 0) sm.cs[t] = make_uint4(sm.sv.nl[t], (uint32_t)key, (uint32_t)(key >> 32), 0u);
    }
    CE_STAMP(blockIdx.x, 5)
    auto rank_write = [&](int i) {  // survivor i takes the slot of its rank
        const uint4 me = sm.cs[i];
        int r = 0;
        // 8 triples per LDS round trip (the asm keeps the compiler from
        // unrolling a runtime-bounded loop itself: one round trip per
        // survivor measured 0.84 us); cs[nc, nc + 8) holds zero triples,
        // which beat nothing
#pragma unroll 1
        for (int j0 = 0; j0 < nc; j0 += 8) {
            CE_DASSERT(j0 + 8 <= SM::CAP + 8);  // the zero-padded triples [nc, nc + 8)
            uint4 a[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) a[k] = sm.cs[j0 + k];
#pragma unroll
            for (int k = 0; k < 8; ++k) r = add_if_beats(r, me, a[k]);
        }
        CE_DASSERT(i < nc && r >= 0 && r < nc);
        if (r < q) {
            ov[r] = key_to_val(((uint64_t)me.z << 32) | me.y);
            oi[r] = pos_of(~me.x);
        }
    };
    auto pad = [&](int i) {  // fewer survivors than q: padding
        ov[i] = __longlong_as_double(0x7ff8000000000000ll);
        oi[i] = -1;
    };
    if (nc <= SPW) {  // block-uniform: wave 0 wrote every triple and ranks them
        if (w == 0) {
            __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
            __builtin_amdgcn_wave_barrier();
            if (lane < nc) rank_write(lane);
            else if (lane < q) pad(lane);
        }
    } else {
        __syncthreads();
        if (tid < nc) rank_write(tid);
        else if (tid < q) pad(tid);
    }
    CE_STAMP(blockIdx.x, 4)
} else {
    // overflow (> CAP items at or near the floor): exact keys of every
    // item, per-wave lists + tree merge
    RegTopQ tq;
    tq.init(q);
#pragma unroll
    for (int v = 0; v < K; ++v) {
        const bool ok = sp[v] | (ak[v] != 0);
        const uint64_t key = ok ? order_key(entropy_row<C>(mrow[v])) : 0ull;
        tq.offer(key, pos_of((uint32_t)(v * BS + tid)), ok);
    }
    block_merge_write<W>(tq, sm.lists, q, nullptr, 0, ov, oi);
}
