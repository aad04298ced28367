// ce_frames_select_body.hpp -- the body of the lane-per-song frames selection
// (ce_frames.hpp), a function-body fragment included by k_frames_select and
// k_frames_select_excl.  In scope: C; FrameArgs a; int q; Cand* wc; constexpr
// bool kExcl and the bitmap `excl` (songs whose bit is set are out of the pool:
// they read nothing and are never offered).  kExcl = false leaves
// k_frames_select the code it had before the body moved here.
    stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    __shared__ WaveLists sm;
    CE_DASSERT((int)gridDim.x <= a.nlists && q >= 1 && q <= kStreamMaxQ);
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t gw = (int64_t)blockIdx.x * 4 + w;
    int64_t lo = gw * a.per_wave;
    int64_t hi = lo + a.per_wave;
    if (hi > a.N) hi = a.N;
    if (lo > hi) lo = hi;
    RegTopQ tq;
    tq.init(q);
    for (int64_t t0 = lo; t0 < hi; t0 += 64) {
        const int64_t n = t0 + lane;
        bool live = n < hi;
        if constexpr (kExcl) {
            CE_DASSERT(!live || (n >= 0 && (n >> 5) < (a.N + 31) / 32));  // the bitmap word
            live = live && !(excl && excluded(excl, n));
        }
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0;  // np.add.reduce identity
        if (!kExcl || live)  // out of the pool: not even a song-level row is read
            for (int mm = 0; mm < a.M; ++mm) add_member_mean<C, 8>(a.mem[mm], a, n, live, acc);
        double mean[C];
#pragma unroll
        for (int c = 0; c < C; ++c) mean[c] = div_members(acc[c], a.dM, a.invM, a.pow2);
        if constexpr (kExcl) {  // out of the pool: an ordinary row, so the wave stays on the entropy's fast division
#pragma unroll
            for (int c = 0; c < C; ++c) mean[c] = live ? mean[c] : 1.0;
        }
        const double h = entropy_row<C>(mean);
        tq.offer(order_key(h), n + a.base_idx, live);
    }
    block_merge_write<4>(tq, sm, q, wc + (int64_t)blockIdx.x * q, a.nlists, nullptr, nullptr, 4, a.ctr != nullptr);
    if (a.ctr) fold_merge<4>(a.ctr, a.oval, a.oidx, a.ocand, q, wc, sm);
