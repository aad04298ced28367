// ce_ws_sanitize.cpp -- the workspace layout (ce_ws.hpp, nothing else) under
// ASan + UBSan: `make sanitize-ws`.  For every entry point's layout over a grid
// of sizes (negative and zero arguments included) it checks that
//   - every region lies inside `bytes` from a base misaligned by 0..255 bytes,
//   - the regions are pairwise disjoint,
//   - each is aligned as its users need (records 16 B, entropies and digit
//     totals 8 B, counters 4 B, the seed scratch 256 B),
//   - the regions one merge reads as one array of lists are adjacent,
//   - the lists hold the blocks the launches use;
// and, where `bytes` <= 64 MiB, allocates exactly `bytes` and writes the first
// and last byte of every region (larger sizes: the arithmetic only).
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "ce_ws.hpp"

using namespace ce;

struct Named {
    const char* name;
    Region r;
    size_t align;
};

static long g_layouts = 0, g_touched = 0;

[[noreturn]] static void die(const std::string& what, const char* msg, const char* region = "") {
    fprintf(stderr, "ce_ws_sanitize: %s: %s %s\n", what.c_str(), msg, region);
    abort();
}

static void check(const std::string& what, const WsLayout& L, size_t want_list_bytes) {
    ++g_layouts;
    const std::vector<Named> regs = {
        {"ctr", L.ctr, 4},       {"lists", L.lists, 16}, {"seg2", L.seg2, 16}, {"running", L.running, 16},
        {"seed", L.seed, 256},   {"ent", L.ent, 8},      {"a", L.a, 16},       {"b", L.b, 16},
        {"hist", L.hist, 4},     {"dtot", L.dtot, 8},    {"extra", L.extra, 16},
    };
    if (L.ctr.off != 0 || L.ctr.bytes != kWsHeader) die(what, "the counters are not the header");
    for (const Named& x : regs) {
        if (!x.r.bytes) continue;
        if (x.r.off % x.align) die(what, "misaligned region", x.name);
        if (x.r.end() < x.r.off) die(what, "region wraps", x.name);
        for (size_t m = 0; m < 256; ++m) {  // the caller's base, misaligned by m
            const uintptr_t base = 0x100000 + m;
            if (ws_base((const void*)base) - base + x.r.end() > L.bytes) die(what, "region past bytes", x.name);
        }
        for (const Named& y : regs)
            if (&x != &y && y.r.bytes && x.r.off < y.r.end() && y.r.off < x.r.end()) die(what, "regions overlap", x.name);
    }
    if (L.seg2.bytes && L.seg2.off != L.lists.end()) die(what, "seg2 not behind the lists");
    if (L.running.bytes && L.running.off != L.lists.end()) die(what, "running slot not behind the lists");
    if (L.seed.bytes && L.seed.bytes < kWideSeedUsed) die(what, "seed scratch too small");
    if (L.q) {  // a list layout
        if (L.lists.bytes + L.seg2.bytes + L.running.bytes != want_list_bytes) die(what, "list bytes");
        const int64_t nl = (int64_t)(want_list_bytes / ((size_t)L.q * kCandBytes));
        if (L.slot(0).off != L.lists.off || L.slot(nl - 1).end() != L.lists.off + want_list_bytes)
            die(what, "slots do not tile the lists");
        if (L.running.bytes && (L.slot(nl - 1).off != L.running.off || L.running.bytes != L.slot(0).bytes))
            die(what, "the running slot is not the last list");
    } else {  // a sort layout
        const size_t n = (size_t)L.g.n;
        if (L.ent.bytes != n * 8 || L.a.bytes != n * kCandBytes || L.b.bytes != n * kCandBytes ||
            L.hist.bytes != (size_t)256 * L.g.nw * 4 || L.dtot.bytes != 2048)
            die(what, "sort buffers");
        if (L.g.chunk % 64 || (int64_t)L.g.nw * L.g.chunk < L.g.n || L.g.nw < 1 || L.g.nw > kSortMaxWaves)
            die(what, "sort geometry");
    }
    if (L.bytes > ((size_t)64 << 20)) return;
    char* p = (char*)malloc(L.bytes);
    if (!p) die(what, "malloc");
    char* base = (char*)ws_base(p);
    for (const Named& x : regs)
        if (x.r.bytes) {
            base[x.r.off] = 1;
            base[x.r.end() - 1] = 2;
            ++g_touched;
        }
    if (L.seed.bytes) base[L.seed.off + kWideSeedSapx + (size_t)kWideVoteSamples * sizeof(float) - 1] = 3;
    free(p);
}

int main() {
    const int64_t Ns[] = {-1, 0, 1, 63, 64, 65, 4096, 4097, 65536, 65537, 100000000ll, 1ll << 32};
    const int32_t Qs[] = {-1, 0, 1, 64, 65, 2048, 2049, 100000};
    const int32_t Us[] = {0, 1, 64, 500};
    const int64_t Nhs[] = {0, 1, 1300, 5000};
    for (int64_t N : Ns)
        for (int32_t q : Qs) {
            const std::string at = "(N=" + std::to_string(N) + ", q=" + std::to_string(q) + ")";
            const size_t slot = (size_t)(q < 1 ? 1 : q) * kCandBytes, G = (size_t)pool_blocks(N);
            check("ws_topq" + at, ws_topq(N, q), G * slot);
            check("ws_mc" + at, ws_mc(N, q), G * slot);
            check("ws_chunk" + at, ws_chunk(N, q), (G + 1) * slot);
            check("ws_frames" + at, ws_frames(N, q), G * slot);
            if (q <= CE_MAX_Q) check("ws_lists" + at, ws_lists(N, q), G * slot);
            if (q > CE_MAX_Q) {  // the chunked job's two runs of q records
                const WsLayout L = ws_chunk(N, q);
                if (L.extra_slot(0, q).off != L.extra.off || L.extra_slot(1, q).end() != L.extra.end())
                    die("ws_chunk" + at, "extra slots");
            } else if (q > kStreamMaxQ && ws_frames(N, q).ent.bytes != (size_t)(N > 0 ? N : 0) * 8) {
                die("ws_frames" + at, "entropies");
            }
            for (int64_t Nh : Nhs) {
                const WsLayout L = ws_mix(N, Nh, q);
                check("ws_mix" + at + " N_h=" + std::to_string(Nh), L, (G + (size_t)pool_blocks(Nh)) * slot);
                if (q <= CE_MAX_Q && L.seg2.bytes != (size_t)pool_blocks(Nh) * slot) die("ws_mix" + at, "seg2 bytes");
                if (q <= CE_MAX_Q && L.bytes < ws_mc(N, q).bytes) die("ws_mix" + at, "does not cover ws_mc");
            }
            for (int32_t U : Us) {
                const size_t U1 = (size_t)(U < 1 ? 1 : U);
                const size_t nu = (size_t)batched_bpu(N, (int)U1) * U1;
                check("ws_batched" + at + " U=" + std::to_string(U), ws_batched(N, U, q), nu * slot);
                for (int64_t Nh : Nhs) {  // the batched mix: total_h hc rows over the same users
                    const std::string atm = at + " U=" + std::to_string(U) + " total_h=" + std::to_string(Nh);
                    const size_t nh = (size_t)batched_bpu(Nh, (int)U1) * U1;
                    const WsLayout L = ws_batched_mix(N, Nh, U, q);
                    check("ws_batched_mix" + atm, L, (nu + nh) * slot);
                    if (q <= CE_MAX_Q && L.seg2.bytes != nh * slot) die("ws_batched_mix" + atm, "seg2 bytes");
                    if (L.bytes < ws_batched(N, U, q).bytes) die("ws_batched_mix" + atm, "does not cover ws_batched");
                    if (q > CE_MAX_Q && L.g.n != (N > 0 ? N : 0) + Nh) die("ws_batched_mix" + atm, "sort records");
                }
            }
        }
    printf("ce_ws_sanitize: %ld layouts, %ld regions written: ok\n", g_layouts, g_touched);
    return 0;
}
