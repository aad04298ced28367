// ce_cnn.hip -- C-ABI entries of the short-chunk CNN member (ce_cnn.hpp): host
// checks before any device call, then the launches; the only TU that
// instantiates its kernels.  Nothing allocates, nothing is read back.  Both
// network entries (the forward, and ce_cnn_activations, which stops after a
// block and hands its output over) launch through cnn_blocks.
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

// The host checks both network entries make first, in this order.
static int cnn_check_net(int32_t n_mels, int32_t T, int32_t nc) {
    if (n_mels != kCnnMels) return fail(CE_EINVAL, "the log-mel has %d bands, the network takes %d", n_mels, kCnnMels);
    if (T < kCnnMels) return fail(CE_EINVAL, "T=%d frames: seven 2x2 pools need T >= %d", T, kCnnMels);
    if (!cnn_nc_ok(nc))
        return fail(CE_EINVAL, "nc=%d must be a positive multiple of 16 (<= %d)", nc, kCnnMaxNc);
    return CE_OK;
}

static int cnn_check_ws(int64_t n, int32_t T, int32_t nc, size_t ws_bytes) {
    const size_t need = 2 * cnn_buf_bytes(n, T, nc) + 256;
    if (ws_bytes < need)
        return fail(CE_EWORKSPACE, "workspace of %zu bytes, ce_cnn_workspace_bytes(%lld, %d, %d) = %zu", ws_bytes,
                    (long long)n, T, nc, need);
    return CE_OK;
}

// Blocks 1 .. last (1 <= last <= 7) of a batch, ping-pong through ws: the one
// launch sequence of both entries.  Returns the buffer block `last` wrote,
// [n, 128 >> last, T >> last, cout[last - 1]]; *Wl is its width.
static float* cnn_blocks(const float* mel, int64_t n, int32_t T, int32_t nc, const CnnLayout& l, const CnnGeom& g,
                         int last, void* ws, hipStream_t st, int* Wl) {
    const size_t buf = cnn_buf_bytes(n, T, nc);
    char* base = reinterpret_cast<char*>(((uintptr_t)ws + 255) & ~(uintptr_t)255);
    float* ping = reinterpret_cast<float*>(base);
    float* pong = reinterpret_cast<float*>(base + buf);

    int H = kCnnMels / 2, W = T / 2;
    const int64_t per = (int64_t)H * W * (nc / kB1Cpt);
    hipLaunchKernelGGL(k_cnn_block1, dim3((unsigned)((per + 255) / 256), 1, (unsigned)n), dim3(256), 0, st, mel, T, nc,
                       g, l.w[0], l.sc[0], l.sh[0], ping);
    float* src = ping;
    float* dst = pong;
    for (int b = 1; b < last; ++b) {
        const CnnConvArgs a{src, dst, l.w[b], l.sc[b], l.sh[b], H, W, l.cin[b], l.cout[b]};
        if (a.Cout >= 128) cnn_conv_launch<4>(a, g, n, st);
        else if (a.Cout >= 64) cnn_conv_launch<2>(a, g, n, st);
        else cnn_conv_launch<1>(a, g, n, st);
        H /= 2, W /= 2;
        float* t = src;
        src = dst, dst = t;
    }
    *Wl = W;
    return src;
}

extern "C" int ce_cnn_forward_users(const float* mel, int64_t n, int32_t n_mels, int32_t T, const float* weights,
                                    int32_t nc, int32_t Uw, const int64_t* item_offsets, int32_t U, int64_t s_base,
                                    const uint32_t* excl, const int32_t* y, int64_t* cm, float* out, int64_t ld_out,
                                    void* ws, size_t ws_bytes, ce_stream_t stream) {
    if (int rc = cnn_check_net(n_mels, T, nc)) return rc;
    if (U < 1 || (Uw != 1 && Uw != U)) return fail(CE_EINVAL, "Uw=%d must be 1 or U=%d (>= 1)", Uw, U);
    if (n < 0 || n > 65535 || s_base < 0 || ld_out < kCnnC)
        return fail(CE_EINVAL, "bad shape n=%lld (0 .. 65535) s_base=%lld ld_out=%lld", (long long)n,
                    (long long)s_base, (long long)ld_out);
    if ((y == nullptr) != (cm == nullptr)) return fail(CE_EINVAL, "y and cm come together");
    if (n == 0) return CE_OK;
    if (int rc = cnn_check_ws(n, T, nc, ws_bytes)) return rc;
    if (!mel || !weights || !item_offsets || !out || !ws) return fail(CE_EINVAL, "null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const CnnLayout l = cnn_layout(nc);
    const CnnGeom g{item_offsets, excl, weights, Uw == 1 ? 0 : l.total, s_base, U};
    int W = 0;
    const float* feat = cnn_blocks(mel, n, T, nc, l, g, kCnnBlocks, ws, st, &W);
    const int D = 4 * nc;
    const CnnHeadArgs ha{feat, W, D, l.W1, l.s1, l.t1, l.W2, l.b2, out, ld_out, y,
                         reinterpret_cast<unsigned long long*>(cm)};
    hipLaunchKernelGGL(k_cnn_head, dim3((unsigned)n), dim3(256), 2 * (size_t)D * sizeof(float), st, ha, g);
    return check_launch("ce_cnn_forward_users");
}

extern "C" int ce_cnn_activations(const float* mel, int64_t n, int32_t n_mels, int32_t T, const float* weights,
                                  int32_t nc, const int64_t* item_offsets, int32_t block, float* act, void* ws,
                                  size_t ws_bytes, ce_stream_t stream) {
    if (int rc = cnn_check_net(n_mels, T, nc)) return rc;
    if (block < 1 || block > kCnnBlocks) return fail(CE_EINVAL, "block=%d outside 1 .. %d", block, kCnnBlocks);
    if (n < 0 || n > 65535) return fail(CE_EINVAL, "bad shape n=%lld (0 .. 65535)", (long long)n);
    if (n == 0) return CE_OK;
    if (int rc = cnn_check_ws(n, T, nc, ws_bytes)) return rc;
    if (!mel || !weights || !item_offsets || !act || !ws) return fail(CE_EINVAL, "null pointer");
    const hipStream_t st = (hipStream_t)stream;
    const CnnLayout l = cnn_layout(nc);
    const CnnGeom g{item_offsets, nullptr, weights, 0, 0, 1};
    int W = 0;
    const float* src = cnn_blocks(mel, n, T, nc, l, g, block, ws, st, &W);
    if (int rc = check_launch("ce_cnn_activations")) return rc;
    const size_t floats = (size_t)n * (size_t)(kCnnMels >> block) * (size_t)W * (size_t)l.cout[block - 1];
    const hipError_t e = hipMemcpyAsync(act, src, floats * sizeof(float), hipMemcpyDeviceToDevice, st);
    if (e != hipSuccess) return fail(CE_ELAUNCH,"ce_cnn_activations: the copy: %s", hipGetErrorString(e));
    return CE_OK;
}
