// ce_frames_lanes_body.hpp -- the body of the C-lanes-per-song frames kernels
// (ce_frames.hpp), a function-body fragment included by k_frames_lanes,
// k_frames_lanes_excl and k_frames_consensus, so the three are one text.  The
// including kernel has in scope: the template parameters C, DMA, GNT; FrameArgs
// a; int q and Cand* wc (the top-q sink); and
//   constexpr bool kExcl  songs whose bit is set in `excl` (const uint32_t*,
//                         may be null: no song is) are out of the pool
//   constexpr bool kRows  the sink: false = entropy -> the top-q lists,
//                         true = the committee mean row -> out[n * ld_out + c]
// A discarded branch leaves no code: k_frames_lanes (kExcl = kRows = false)
// compiles to what it did before the body moved here.
    static_assert(64 % C == 0, "C divides the wave");
    constexpr int G = 64 / C;  // songs per wave step
    constexpr int TB = DMA ? 16384 : 16;  // per-wave LDS tile
    if constexpr (!kRows) stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    __shared__ WaveLists sm;
    __shared__ __attribute__((aligned(16))) char tiles[4][TB];
    if constexpr (!kRows) CE_DASSERT((int)gridDim.x <= a.nlists && q >= 1 && q <= kStreamMaxQ);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int sg = lane / C, c = lane - sg * C;
    char* tile = tiles[w];
    const int64_t gw = (int64_t)blockIdx.x * 4 + w;
    // grid-cyclic steps (wave g: steps g, g + W, ...; ~1 % over a contiguous run per wave)
    const int64_t lo = gw * G, hi = a.N, step = (int64_t)gridDim.x * 4 * G;
    // frame-level members in member order (up to 4 read together by the direct path)
    int nf = 0, f_0 = 0, f_1 = 0, f_2 = 0, f_3 = 0;
    for (int mm = 0; mm < a.M; ++mm)
        if (!a.mem[mm].song_level) {
            f_0 = nf == 0 ? mm : f_0;
            f_1 = nf == 1 ? mm : f_1;
            f_2 = nf == 2 ? mm : f_2;
            f_3 = nf == 3 ? mm : f_3;
            ++nf;
        }
    RegTopQ tq;
    if constexpr (!kRows) tq.init(q);
    // in the pool: song nn exists and (kExcl) its bit is clear
    auto in_pool = [&](int64_t nn) {
        if (nn >= hi) return false;
        if constexpr (kExcl) {
            CE_DASSERT(nn >= 0 && (nn >> 5) < (a.N + 31) / 32);  // the bitmap word
            if (excl && excluded(excl, nn)) return false;
        }
        return true;
    };
    // the step's CSR offsets (this lane's song [f0, f1), the step's rows [R0,
    // R1) of songs [t, t + G)) are loaded ONCE per step and one step ahead:
    // the loads of step t + 1 are issued at the top of step t and land during
    // its tiles, so no member's first tile waits on an offsets round trip
    // (they were re-read per member before: 1M songs grouped 0.911 -> 0.880 ms,
    // profiles/r05_frames_offsets_ab.json)
    int64_t pf0 = 0, pf1 = 0, pR0 = 0, pR1 = 0;
    auto load_offs = [&](int64_t t) {
        const int64_t nn = t + sg;
        const int64_t tg = t + G < hi ? t + G : hi;
        if constexpr (kExcl) {  // an excluded song: no rows, [0, 0)
            const bool on = in_pool(nn);
            pf0 = on ? a.off[nn] : 0;
            pf1 = on ? a.off[nn + 1] : 0;
        } else {
            pf0 = nn < hi ? a.off[nn] : 0;
            pf1 = nn < hi ? a.off[nn + 1] : 0;
        }
        pR0 = a.off[t];
        pR1 = a.off[tg];
    };
    if (lo < hi) load_offs(lo);
    for (int64_t t0 = lo; t0 < hi; t0 += step) {
        const int64_t n = t0 + sg;
        bool live = n < hi;
        if constexpr (kExcl) live = in_pool(n);
        double acc = 0.0;  // np.add.reduce identity
        const int64_t sf0 = pf0, sf1 = pf1, sR0 = pR0, sR1 = pR1;
        if (t0 + step < hi) load_offs(t0 + step);
        if constexpr (kExcl)
            if (!__any(live)) continue;  // wave-uniform: every song of the step is out -- no load, no tile
        if (!DMA && nf <= 4) {
            // direct loads (shuffled frames): each batch's 8 frame indices are
            // read ONCE for every frame-level member, then all members' rows of
            // the batch are in flight together (perm read once, 2 serial round
            // trips per batch instead of 2 per batch and member); each member
            // keeps its own sequential group sum, and the means meet in member
            // order below
            const int64_t f0 = sf0, f1 = sf1;
            CE_DASSERT(f0 >= 0 && f0 <= f1);
            constexpr int B = 8;  // (4: 1M songs equal, 1608 songs 38.6 -> 42.4 us)
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
            for (int64_t fb = f0; fb < f1; fb += B) {
                int64_t r[B];
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    const int64_t f = fb + u < f1 ? fb + u : f1 - 1;
                    r[u] = a.perm ? a.perm[f] : f;
                }
                double v[4][B];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (k < nf) {  // wave-uniform
                        const FrameMember& fm = a.mem[k == 0 ? f_0 : (k == 1 ? f_1 : (k == 2 ? f_2 : f_3))];
#pragma unroll
                        for (int u = 0; u < B; ++u) {
                            const int64_t o = r[u] * fm.ld + c;
                            if constexpr (GNT)  // shuffled rows of a large pool: each read once
                                v[k][u] = fm.dt == kF64 ? __builtin_nontemporal_load(static_cast<const double*>(fm.p) + o)
                                                        : (double)__builtin_nontemporal_load(static_cast<const float*>(fm.p) + o);
                            else
                                v[k][u] = fm.dt == kF64 ? static_cast<const double*>(fm.p)[o]
                                                        : (double)static_cast<const float*>(fm.p)[o];
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < B; ++u) {
                    const bool in = fb + u < f1;
                    if (nf > 0 && in && v[0][u] == v[0][u]) { s0 += v[0][u]; ++c0; }
                    if (nf > 1 && in && v[1][u] == v[1][u]) { s1 += v[1][u]; ++c1; }
                    if (nf > 2 && in && v[2][u] == v[2][u]) { s2 += v[2][u]; ++c2; }
                    if (nf > 3 && in && v[3][u] == v[3][u]) { s3 += v[3][u]; ++c3; }
                }
            }
            int k = 0;
            for (int mm = 0; mm < a.M; ++mm) {
                const FrameMember& fm = a.mem[mm];
                double mean;
                if (fm.song_level) {
                    const int64_t o = (live ? n : t0) * fm.ld + c;
                    if (kExcl && !live)  // out of the pool: no song-level row is read
                        mean = 0.0;
                    else
                    mean = fm.dt == kF64 ? static_cast<const double*>(fm.p)[o]
                                         : (double)static_cast<const float*>(fm.p)[o];
                } else {
                    const double sk = k == 0 ? s0 : (k == 1 ? s1 : (k == 2 ? s2 : s3));
                    const int ck = k == 0 ? c0 : (k == 1 ? c1 : (k == 2 ? c2 : c3));
                    double x = ck ? sk / (double)ck : __longlong_as_double(0x7ff8000000000000ll);
                    if (fm.dt == kF32) x = (double)(float)x;  // the float32 result column
                    mean = x;
                    ++k;
                }
                acc += mean;
            }
        } else
        for (int mm = 0; mm < a.M; ++mm) {
            const FrameMember& fm = a.mem[mm];
            const int EB = fm.dt == kF64 ? 8 : 4;
            double mean;
            if (fm.song_level) {
                const int64_t o = (live ? n : t0) * fm.ld + c;
                if (kExcl && !live)  // out of the pool: no song-level row is read
                    mean = 0.0;
                else
                mean = fm.dt == kF64 ? static_cast<const double*>(fm.p)[o] : (double)static_cast<const float*>(fm.p)[o];
            } else {
                const int64_t f0 = sf0, f1 = sf1;
                CE_DASSERT(f0 >= 0 && f0 <= f1);
                double s = 0.0;
                int cnt = 0;
                const int RB = C * EB;
                const int64_t R0 = sR0, R1 = sR1;
                // the step's songs tile [R0, R1) (CSR offsets); a wave holding a song outside it
                // (offsets not monotone) reads its rows directly instead
                const bool inside = !live || (f0 >= R0 && f1 <= R1);
                if (DMA && !a.perm && fm.ld == C && RB % 16 == 0 && fm.vec && __all(inside)) {  // wave-uniform: LDS-DMA tiles
                    const char* mb = static_cast<const char*>(fm.p);
                    if (EB == 8) {
                        if constexpr (DMA && (C * 8) % 16 == 0) tile_song_sum<C, 8, TB>(mb, R0, R1, f0, f1, lane, c, tile, s, cnt);
                    } else {
                        if constexpr (DMA && (C * 4) % 16 == 0) tile_song_sum<C, 4, TB>(mb, R0, R1, f0, f1, lane, c, tile, s, cnt);
                    }
                } else {  // direct loads: batches of 8 rows in flight, added in row order
                    constexpr int B = 8;
                    for (int64_t fb = f0; fb < f1; fb += B) {
                        double v[B];
#pragma unroll
                        for (int u = 0; u < B; ++u) {
                            const int64_t f = fb + u < f1 ? fb + u : f1 - 1;
                            const int64_t r = a.perm ? a.perm[f] : f;
                            const int64_t o = r * fm.ld + c;
                            if constexpr (GNT)
                                v[u] = fm.dt == kF64 ? __builtin_nontemporal_load(static_cast<const double*>(fm.p) + o)
                                                     : (double)__builtin_nontemporal_load(static_cast<const float*>(fm.p) + o);
                            else
                                v[u] = fm.dt == kF64 ? static_cast<const double*>(fm.p)[o]
                                                     : (double)static_cast<const float*>(fm.p)[o];
                        }
#pragma unroll
                        for (int u = 0; u < B; ++u)
                            if (fb + u < f1 && v[u] == v[u]) {
                                s += v[u];
                                ++cnt;
                            }
                    }
                }
                double x = cnt ? s / (double)cnt : __longlong_as_double(0x7ff8000000000000ll);
                if (fm.dt == kF32) x = (double)(float)x;  // the float32 result column
                mean = x;
            }
            acc += mean;
        }
        double mv = div_members(acc, a.dM, a.invM, a.pow2);
        if constexpr (kRows) {  // consensus_prob[n, c] (amg_test.py:441); rows out of the pool are not written
            CE_DASSERT(!live || (n >= 0 && n < a.N && c < ld_out));
            if (live) out[n * ld_out + c] = mv;
        } else {
            // a song out of the pool has no row (NaN): give its lanes an ordinary one, so the wave
            // stays on the entropy's fast division (1M songs grouped, 30 % excluded: 0.774 -> 0.738 ms,
            // profiles/frames_session.json)
            if constexpr (kExcl) mv = live ? mv : 1.0;
            double row[C];
#pragma unroll
            for (int k = 0; k < C; ++k) row[k] = __shfl(mv, sg * C + k);
            const double h = entropy_row<C>(row);
            tq.offer(order_key(h), n + a.base_idx, live && c == 0);
        }
    }
    if constexpr (!kRows) {
        block_merge_write<4>(tq, sm, q, wc + (int64_t)blockIdx.x * q, a.nlists, nullptr, nullptr, 4, a.ctr != nullptr);
        if (a.ctr) fold_merge<4>(a.ctr, a.oval, a.oidx, a.ocand, q, wc, sm);
    }
