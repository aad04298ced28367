// ce_abi_frames.hip -- C-ABI (include/ce.h): frames -> committee entropy ->
// top-q in one pass (k_frames_select, ce_frames.hpp), the
// same over the songs a session's exclusion bitmap leaves (ce_select_frames_excl)
// and the committee mean rows alone (ce_frames_consensus).  Every frames kernel
// is instantiated here only.
#include "ce_dispatch.hpp"  // resident_grid
#include "ce_frames.hpp"

using namespace ce;

// q <= 64: the streaming kernels' lists; 64 < q <= CE_MAX_Q: the lists of the
// entropy vector's selection + the N entropies behind them; q > CE_MAX_Q: the
// sort path (ws_frames, ce_ws.hpp).
extern "C" size_t ce_select_frames_workspace_bytes(int64_t N, int32_t q) { return ws_frames(N, q).bytes; }

// The member checks every frames entry point shares, in the order the ABI
// answers them (M, then the call's own arguments, then C): see frames_members.
static int frames_head(const ce_member* members, int32_t M) {
    if (!members || M < 1 || M > kMaxFrameMembers) return fail(CE_EINVAL, "need 1..%d members (got %d)", kMaxFrameMembers, M);
    return CE_OK;
}

static int frames_classes(int32_t C) {
    if (C != 2 && C != 3 && C != 4 && C != 8) return fail(CE_EUNSUPPORTED, "frame selection: C=%d not in {2, 3, 4, 8}", C);
    return CE_OK;
}

// the members and the pool's geometry into fa
static int frames_members(const ce_member* members, int32_t M, int32_t C, const int64_t* offsets,
                          const int64_t* perm_or_null, int64_t N, int64_t base_idx, FrameArgs& fa) {
    for (int m = 0; m < M; ++m) {
        const ce_member& x = members[m];
        if (x.dtype != CE_F32 && x.dtype != CE_F64) return fail(CE_EUNSUPPORTED, "member %d: float32/float64 only", m);
        if (!x.p && N > 0) return fail(CE_EINVAL, "member %d: null pointer", m);
        if (x.ld < C) return fail(CE_EINVAL, "member %d: row stride %lld < C", m, (long long)x.ld);
        const int eb = x.dtype == CE_F64 ? 8 : 4;
        fa.mem[m] = FrameMember{x.p, x.ld, x.dtype == CE_F64 ? kF64 : kF32, x.song_level ? 1 : 0,
                                ((uintptr_t)x.p % 16 == 0 && (x.ld * eb) % 16 == 0) ? 1 : 0, 0};
    }
    fa.M = M;
    fa.off = offsets;
    fa.perm = perm_or_null;
    fa.N = N;
    fa.dM = (double)M;
    fa.invM = 1.0 / (double)M;
    fa.pow2 = (M & (M - 1)) == 0;
    fa.base_idx = base_idx;
    return CE_OK;
}

// The flavour of the C-lanes kernels for a pool (grid: what the LDS-DMA
// flavour keeps resident).  LDS-DMA tiles for grouped frames once every wave
// runs >= 4 steps: at the reference's 1608 songs x 40 frames the tile round
// trips are exposed (DMA 44.6 us, direct 31.7 us); at 1M songs the tiles win
// (0.92 vs 1.49 ms).  Large shuffled pools: the gather's row loads
// non-temporal (GNT).
struct LanesFlavour {
    bool dma, gnt;
};
static LanesFlavour lanes_flavour(int grid, int64_t N, int step, const int64_t* perm_or_null) {
    static const int dma_env = [] {  // test knob: CE_AMD_FRAMES_DMA=0 / 1 forces direct loads / LDS-DMA tiles
        // (test_frames_dma_tiles_vs_oracle runs the tiles at the oracle's sizes with it)
        const char* e = getenv("CE_AMD_FRAMES_DMA");
        return e ? (e[0] == '0' ? 0 : 1) : -1;
    }();
    const int64_t steps_per_wave = cdiv(cdiv(N, (int64_t)grid * 4), (int64_t)step);
    const bool dma = !perm_or_null && (dma_env >= 0 ? dma_env == 1 : steps_per_wave >= 4);
    return LanesFlavour{dma, !dma && perm_or_null && steps_per_wave >= 4};
}

// ce_select_frames (excl == nullptr) and ce_select_frames_excl: one ladder,
// the exclusion kernels where a bitmap is given.
static int select_frames_run(const char* what, const ce_member* members, int32_t M, int32_t C, const int64_t* offsets,
                             const int64_t* perm_or_null, int64_t N, const uint32_t* excl, int32_t q,
                             int64_t base_idx, void* ws, size_t ws_bytes, double* val_out, int64_t* idx_out,
                             ce_stream_t stream) {
    int rc = check_q(q);
    if (rc) return rc;
    rc = frames_head(members, M);
    if (rc) return rc;
    if (N < 0 || (N > 0 && !offsets) || (q > 0 && (!val_out || !idx_out)))
        return fail(CE_EINVAL, "bad frame selection arguments");
    rc = frames_classes(C);
    if (rc) return rc;
    const int G = pool_blocks(N);
    const WsLayout L = ws_frames(N, q);
    rc = check_ws(L, ws, ws_bytes);
    if (rc) return rc;
    FrameArgs fa{};
    rc = frames_members(members, M, C, offsets, perm_or_null, N, base_idx, fa);
    if (rc) return rc;
    fa.nlists = G;
    const hipStream_t st = enter(stream);
    if (q == 0) return CE_OK;
    if (q > kStreamMaxQ) {  // per-song entropies to HBM, then the lists (q <= CE_MAX_Q) or the sort path
        if (q > CE_MAX_Q) {
            rc = check_sort_n(N);
            if (rc) return rc;
        }
        double* ent = ws_ptr<double>(ws, L.ent);
        if (N > 0) {
            const int eg = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(N, 256), 8192));
            switch (C) {
#define CE_FE(CC)                                                                                                  \
    case CC:                                                                                                       \
        if (excl) hipLaunchKernelGGL((k_frames_rows_excl<CC, false>), dim3(eg), dim3(256), 0, st, fa, excl, ent, (int64_t)0); \
        else hipLaunchKernelGGL((k_frames_entropy<CC>), dim3(eg), dim3(256), 0, st, fa, ent);                      \
        break;
                CE_FE(2) CE_FE(3) CE_FE(4) CE_FE(8)
#undef CE_FE
            }
        }
        select_entropies(L, ws, ent, N, q, base_idx, val_out, idx_out, st, excl);
        return check_launch(what);
    }
    const WsLists w = lists_view(L, ws);
    fa.ctr = w.ctr;
    fa.oval = val_out;
    fa.oidx = idx_out;
    fa.ocand = nullptr;
    auto go = [&](auto kern, int step, auto... tail) {  // step: songs per wave step (64 / lanes per song)
        // no more blocks than waves with a step of songs: an idle block still
        // writes an empty list that the grid's last block merges
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(resident_grid(kern, 0, G), cdiv(N, (int64_t)4 * step)));
        fa.per_wave = (cdiv(N, (int64_t)grid * 4) + step - 1) / step * step;
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, fa, q, w.c, tail...);
    };
    // C lanes per song (k_frames_lanes: whole-row reads, LDS-DMA tiles for
    // grouped dense members) where C divides the wave; lane per song otherwise
    // (k_frames_select, measured 2.7x slower at 1M songs x 40 frames)
    auto lanes_go = [&](auto dma_kern, auto direct_kern, auto gather_kern, int step, auto... tail) {
        const LanesFlavour f = lanes_flavour(resident_grid(dma_kern, 0, G), N, step, perm_or_null);
        note_kernel("ce::k_frames_lanes%s<%d, %s, %s>", excl ? "_excl" : "", 64 / step, f.dma ? "true" : "false",
                    f.gnt ? "true" : "false");
        if (f.dma) go(dma_kern, step, tail...);
        else if (f.gnt) go(gather_kern, step, tail...);
        else go(direct_kern, step, tail...);
    };
    if (excl) {
        switch (C) {
            case 2: lanes_go(k_frames_lanes_excl<2, true, false>, k_frames_lanes_excl<2, false, false>, k_frames_lanes_excl<2, false, true>, 32, excl); break;
            case 3: note_kernel("%s", "ce::k_frames_select_excl<3>"); go(k_frames_select_excl<3>, 64, excl); break;
            case 4: lanes_go(k_frames_lanes_excl<4, true, false>, k_frames_lanes_excl<4, false, false>, k_frames_lanes_excl<4, false, true>, 16, excl); break;
            default: lanes_go(k_frames_lanes_excl<8, true, false>, k_frames_lanes_excl<8, false, false>, k_frames_lanes_excl<8, false, true>, 8, excl); break;
        }
        return check_launch(what);
    }
    switch (C) {
        case 2: lanes_go(k_frames_lanes<2, true>, k_frames_lanes<2, false>, k_frames_lanes<2, false, true>, 32); break;
        case 3: note_kernel("%s", "ce::k_frames_select<3>"); go(k_frames_select<3>, 64); break;
        case 4: lanes_go(k_frames_lanes<4, true>, k_frames_lanes<4, false>, k_frames_lanes<4, false, true>, 16); break;
        default: lanes_go(k_frames_lanes<8, true>, k_frames_lanes<8, false>, k_frames_lanes<8, false, true>, 8); break;
    }
    return check_launch(what);
}

extern "C" int ce_select_frames(const ce_member* members, int32_t M, int32_t C, const int64_t* offsets,
                                const int64_t* perm_or_null, int64_t N, int32_t q, int64_t base_idx, void* ws,
                                size_t ws_bytes, double* val_out, int64_t* idx_out, ce_stream_t stream) {
    return select_frames_run("ce_select_frames", members, M, C, offsets, perm_or_null, N, nullptr, q, base_idx, ws,
                             ws_bytes, val_out, idx_out, stream);
}

// ce_select_frames over the songs whose bit is clear (the session's epoch
// from frame-level members: the bitmap is tested inside the frames kernels)
extern "C" int ce_select_frames_excl(const ce_member* members, int32_t M, int32_t C, const int64_t* offsets,
                                     const int64_t* perm_or_null, int64_t N, const uint32_t* excl, int32_t q,
                                     int64_t base_idx, void* ws, size_t ws_bytes, double* val_out, int64_t* idx_out,
                                     ce_stream_t stream) {
    if (!excl && N > 0) return fail(CE_EINVAL, "null exclusion bitmap");
    if (N <= 0)  // an empty pool has no bitmap to test: the plain ladder pads every slot
        return select_frames_run("ce_select_frames_excl", members, M, C, offsets, perm_or_null, N, nullptr, q, base_idx,
                                 ws, ws_bytes, val_out, idx_out, stream);
    return select_frames_run("ce_select_frames_excl", members, M, C, offsets, perm_or_null, N, excl, q, base_idx, ws,
                             ws_bytes, val_out, idx_out, stream);
}

// The committee mean rows (amg_test.py:441) of the songs whose bit is clear,
// from frame-level members: what the selections that need more than one global
// top-q (mix, batched) read as a one-member f64 committee.
extern "C" int ce_frames_consensus(const ce_member* members, int32_t M, int32_t C, const int64_t* offsets,
                                   const int64_t* perm_or_null, int64_t N, const uint32_t* excl_or_null, double* out,
                                   int64_t ld_out, ce_stream_t stream) {
    int rc = frames_head(members, M);
    if (rc) return rc;
    if (N < 0 || (N > 0 && (!offsets || !out))) return fail(CE_EINVAL, "bad frame consensus arguments");
    rc = frames_classes(C);
    if (rc) return rc;
    if (ld_out < C) return fail(CE_EINVAL, "output row stride %lld < C", (long long)ld_out);
    FrameArgs fa{};
    rc = frames_members(members, M, C, offsets, perm_or_null, N, 0, fa);
    if (rc) return rc;
    const hipStream_t st = enter(stream);
    if (N == 0) return CE_OK;
    const int G = pool_blocks(N);
    auto go = [&](auto kern, int step) {
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(resident_grid(kern, 0, G), cdiv(N, (int64_t)4 * step)));
        hipLaunchKernelGGL(kern, dim3(grid), dim3(256), 0, st, fa, excl_or_null, out, ld_out);
    };
    auto lanes_go = [&](auto dma_kern, auto direct_kern, auto gather_kern, int step) {
        const LanesFlavour f = lanes_flavour(resident_grid(dma_kern, 0, G), N, step, perm_or_null);
        note_kernel("ce::k_frames_consensus<%d, %s, %s>", 64 / step, f.dma ? "true" : "false", f.gnt ? "true" : "false");
        go(f.dma ? dma_kern : (f.gnt ? gather_kern : direct_kern), step);
    };
    switch (C) {
        case 2: lanes_go(k_frames_consensus<2, true, false>, k_frames_consensus<2, false, false>, k_frames_consensus<2, false, true>, 32); break;
        case 3: {
            note_kernel("%s", "ce::k_frames_rows_excl<3, true>");
            const int eg = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv(N, 256), 8192));
            hipLaunchKernelGGL((k_frames_rows_excl<3, true>), dim3(eg), dim3(256), 0, st, fa, excl_or_null, out, ld_out);
            break;
        }
        case 4: lanes_go(k_frames_consensus<4, true, false>, k_frames_consensus<4, false, false>, k_frames_consensus<4, false, true>, 16); break;
        default: lanes_go(k_frames_consensus<8, true, false>, k_frames_consensus<8, false, false>, k_frames_consensus<8, false, true>, 8); break;
    }
    return check_launch("ce_frames_consensus");
}
