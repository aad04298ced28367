// ce_cnn.hip -- C-ABI entries of the short-chunk CNN member (ce_cnn.hpp): host
// checks before any device call, then the launches; the only TU that
// instantiates its kernels.  Nothing allocates, nothing is read back.
#include "ce_abi.hpp"
#include "ce_cnn.hpp"

using namespace ce;

static bool cnn_nc_ok(int32_t nc) { return nc >= 16 && nc % 16 == 0 && nc <= kCnnMaxNc; }

// floats of one ping-pong buffer for one excerpt: block 1's pooled output, the largest activation
static size_t cnn_act_floats(int32_t T, int32_t nc) { return (size_t)(kCnnMels / 2) * (size_t)(T / 2) * (size_t)nc; }

static size_t cnn_buf_bytes(int64_t batch, int32_t T, int32_t nc) {
    return (cnn_act_floats(T, nc) * (size_t)batch * sizeof(float) + 255) / 256 * 256;
}

extern "C" size_t ce_cnn_weights_floats(int32_t nc) { return cnn_nc_ok(nc) ? (size_t)cnn_layout(nc).total : 0; }

extern "C" size_t ce_cnn_workspace_bytes(int64_t batch, int32_t T, int32_t nc) {
    if (batch < 1 || T < kCnnMels || !cnn_nc_ok(nc)) return 0;
    return 2 * cnn_buf_bytes(batch, T, nc) + 256;
}

extern "C" int ce_cnn_logmel(const float* wave, int64_t S, int64_t L, int64_t ld_wave, const float* basis,
                             const float* fb, float* mel, ce_stream_t stream) {
    // T <= 8 * 65535 frames: the frame tiles are the grid's y
    if (S < 0 || L < kCnnFft || L / kCnnHop + 1 > kMelFrames * 65535 || ld_wave < L)
        return fail(CE_EINVAL, "bad waveform shape S=%lld L=%lld (%d .. %lld) ld=%lld", (long long)S, (long long)L,
                    kCnnFft, (long long)kMelFrames * 65535 * kCnnHop - 1, (long long)ld_wave);
    if (S > 0x7fffffffLL) return fail(CE_EINVAL, "S=%lld excerpts in one call", (long long)S);
    if (S == 0) return CE_OK;
    if (!wave || !basis || !fb || !mel) return fail(CE_EINVAL, "null pointer");
    const int T = (int)(L / kCnnHop + 1);
    hipLaunchKernelGGL(k_cnn_logmel, dim3((unsigned)S, (unsigned)((T + kMelFrames - 1) / kMelFrames)), dim3(256), 0,
                       (hipStream_t)stream, wave, L, ld_wave, basis, fb, mel, T);
    return check_launch("ce_cnn_logmel");
}

template <int NT>
static void cnn_conv_launch(const CnnConvArgs& a, const CnnGeom& g, int64_t n, hipStream_t st) {
    const unsigned tiles = (unsigned)(((a.H + kConvTH - 1) / kConvTH) * ((a.W + kConvTW - 1) / kConvTW));
    hipLaunchKernelGGL(k_cnn_conv<NT>, dim3(tiles, (unsigned)((a.Cout + 32 * NT - 1) / (32 * NT)), (unsigned)n),
                       dim3(256), 0, st, a, g);
}

extern "C" int ce_cnn_forward_users(const float* mel, int64_t n, int32_t n_mels, int32_t T, const float* weights,
                                    int32_t nc, int32_t Uw, const int64_t* item_offsets, int32_t U, int64_t s_base,
                                    const uint32_t* excl, const int32_t* y, int64_t* cm, float* out, int64_t ld_out,
                                    void* ws, size_t ws_bytes, ce_stream_t stream) {
    if (n_mels != kCnnMels) return fail(CE_EINVAL, "the log-mel has %d bands, the network takes %d", n_mels, kCnnMels);
    if (T < kCnnMels) return fail(CE_EINVAL, "T=%d frames: seven 2x2 pools need T >= %d", T, kCnnMels);
    if (!cnn_nc_ok(nc))
        return fail(CE_EINVAL, "nc=%d must be a positive multiple of 16 (<= %d)", nc, kCnnMaxNc);
    if (U < 1 || (Uw != 1 && Uw != U)) return fail(CE_EINVAL, "Uw=%d must be 1 or U=%d (>= 1)", Uw, U);
    if (n < 0 || n > 65535 || s_base < 0 || ld_out < kCnnC)
        return fail(CE_EINVAL, "bad shape n=%lld (0 .. 65535) s_base=%lld ld_out=%lld", (long long)n,
                    (long long)s_base, (long long)ld_out);
    if ((y == nullptr) != (cm == nullptr)) return fail(CE_EINVAL, "y and cm come together");
    if (n == 0) return CE_OK;
    const size_t buf = cnn_buf_bytes(n, T, nc);
    if (ws_bytes < 2 * buf + 256)
        return fail(CE_EWORKSPACE, "workspace of %zu bytes, ce_cnn_workspace_bytes(%lld, %d, %d) = %zu", ws_bytes,
                    (long long)n, T, nc, 2 * buf + 256);
    if (!mel || !weights || !item_offsets || !out || !ws) return fail(CE_EINVAL, "null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const CnnLayout l = cnn_layout(nc);
    const CnnGeom g{item_offsets, excl, weights, Uw == 1 ? 0 : l.total, s_base, U};
    char* base = reinterpret_cast<char*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    float* ping = reinterpret_cast<float*>(base);
    float* pong = reinterpret_cast<float*>(base + buf);

    int H = kCnnMels / 2, W = T / 2;
    const int64_t per = (int64_t)H * W * (nc / kB1Cpt);
    hipLaunchKernelGGL(k_cnn_block1, dim3((unsigned)((per + 255) / 256), 1, (unsigned)n), dim3(256), 0, st, mel, T, nc,
                       g, l.w[0], l.sc[0], l.sh[0], ping);
    float* src = ping;
    float* dst = pong;
    for (int b = 1; b < kCnnBlocks; ++b) {
        const CnnConvArgs a{src, dst, l.w[b], l.sc[b], l.sh[b], H, W, l.cin[b], l.cout[b]};
        if (a.Cout >= 128) cnn_conv_launch<4>(a, g, n, st);
        else if (a.Cout >= 64) cnn_conv_launch<2>(a, g, n, st);
        else cnn_conv_launch<1>(a, g, n, st);
        H /= 2, W /= 2;
        float* t = src;
        src = dst, dst = t;
    }
    const int D = 4 * nc;
    const CnnHeadArgs ha{src, W, D, l.W1, l.s1, l.t1, l.W2, l.b2, out, ld_out, y,
                         reinterpret_cast<unsigned long long*>(cm)};
    hipLaunchKernelGGL(k_cnn_head, dim3((unsigned)n), dim3(256), 2 * (size_t)D * sizeof(float), st, ha, g);
    return check_launch("ce_cnn_forward_users");
}
