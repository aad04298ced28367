// ce_frames_rows_body.hpp -- the body of the lane-per-song pass that writes one
// result per song to HBM (ce_frames.hpp), a function-body fragment included by
// k_frames_entropy and k_frames_rows_excl.  In scope: C; FrameArgs a; constexpr
// bool kExcl with the bitmap `excl` (may be null); constexpr bool kRows with
// the sinks: false = the entropy -> ent[n], true = the committee mean row ->
// out[n * ld_out + c].  A song out of the pool reads and writes nothing.
// kExcl = kRows = false leaves k_frames_entropy the code it had before.
    if constexpr (!kRows) stage_log_table();  // glibc log table -> LDS (ce_glibc_log.hpp)
    for (int64_t n = (int64_t)blockIdx.x * 256 + threadIdx.x; n < a.N; n += (int64_t)gridDim.x * 256) {
        if constexpr (kExcl) {
            CE_DASSERT(n >= 0 && (n >> 5) < (a.N + 31) / 32);  // the bitmap word
            if (excl && excluded(excl, n)) continue;
        }
        double acc[C];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = 0.0;  // np.add.reduce identity
        for (int mm = 0; mm < a.M; ++mm) add_member_mean<C, 8>(a.mem[mm], a, n, true, acc);
        double mean[C];
#pragma unroll
        for (int c = 0; c < C; ++c) mean[c] = div_members(acc[c], a.dM, a.invM, a.pow2);
        if constexpr (kRows) {
            CE_DASSERT(n < a.N && C <= ld_out);  // the consensus row
#pragma unroll
            for (int c = 0; c < C; ++c) out[n * ld_out + c] = mean[c];
        } else {
            ent[n] = entropy_row<C>(mean);
        }
    }
