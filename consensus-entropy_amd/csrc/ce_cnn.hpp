// ce_cnn.hpp -- the short-chunk CNN member, inference: the
// reference's ShortChunkCNN in eval mode (short_cnn.py:278-349, loaded by
// predict_cnn, amg_test.py:173-201) for every user's excerpts.
//
//   waveform [L] -> power spectrogram (n_fft 512, hop 256, periodic Hann,
//   centred, reflect padding) -> filter bank [257, 128] -> 10 log10(max(x, 1e-10))
//   -> spec_bn -> 7 x (conv 3x3 pad 1 + bias -> BatchNorm -> ReLU -> max-pool 2x2,
//   floor) -> max over the width left -> dense1 -> BatchNorm1d -> ReLU -> dense2
//   -> sigmoid: [4] f32 per excerpt.
//
// Kernels:
//   k_cnn_logmel  the front end up to the dB values, [S, 128, T] f32.  The DFT
//                 is a product with the windowed cos / sin basis (the caller
//                 builds it once); 8 frames per block, a thread per bin.
//   k_cnn_block1  Cin = 1, K = 9: direct VALU, spec_bn applied on the load (the
//                 zero padding stays zero), pool fused; writes [S, 64, T/2, nc].
//   k_cnn_conv    blocks 2-7: implicit GEMM on v_mfma_f32_32x32x2_f32.  Pixels
//                 are M, Cout is N, (ky, kx, ci) is K.  Activations are
//                 channel-innermost [S, H, W, C].
//   k_cnn_head    the global max, both dense layers, the sigmoid; with labels
//                 the argmax (np.argmax's rule) and cm[u, y, pred] += 1.
//
// One accumulator and one ordered f32 fma chain per output everywhere, no
// split-K and no float atomic: a result depends on neither the grid, the batch
// nor the form (one model / users) that launched it.  The chain order of
// k_cnn_conv: 8-channel chunks of ci ascending; inside a chunk the taps
// (ky, kx) row-major; inside a tap the chunk's channels ascending.
//
// Weights: every model is one packed f32 record (CnnLayout below; the conv bias
// and the BatchNorm statistics folded into scale / shift by the caller), the
// records stacked [Uw, floats]: Uw = 1 shares one model, Uw = U gives excerpt
// s the record of the user whose item_offsets[u] <= s < item_offsets[u+1].
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/ce.h"
#include "ce_members_users.hpp"  // np_argmax

namespace ce {

constexpr int kCnnMels = 128, kCnnFft = 512, kCnnHop = 256, kCnnBins = 257, kCnnC = 4, kCnnBlocks = 7;
constexpr int kCnnMaxNc = 1024;

// Where a model's tensors sit in its packed record, in floats (every offset a
// multiple of 16 floats, so float4 loads of a 256-B aligned stack are aligned):
//   spec            [16]: scale, shift of spec_bn, then zeros
//   w[i]            [9 * Cin_i, Cout_i]: row (ky * 3 + kx) * Cin + ci, Cout innermost
//   sc[i], sh[i]    [Cout_i]: BatchNorm(conv + bias) = fma(sc, conv, sh)
//   W1              [4nc (in), 4nc (out)]: dense1.weight transposed
//   s1, t1          [4nc]: BatchNorm1d(dense1) = fma(s1, W1 . f, t1)
//   W2              [4, 4nc]: dense2.weight
//   b2              [16]: dense2.bias, then zeros
struct CnnLayout {
    int cin[kCnnBlocks], cout[kCnnBlocks];
    int64_t spec, w[kCnnBlocks], sc[kCnnBlocks], sh[kCnnBlocks], W1, s1, t1, W2, b2, total;
};

__host__ __device__ inline CnnLayout cnn_layout(int nc) {
    CnnLayout l;
    const int mult[kCnnBlocks + 1] = {0, 1, 1, 2, 2, 2, 2, 4};
    int64_t o = 0;
    l.spec = o, o += 16;
    for (int i = 0; i < kCnnBlocks; ++i) {
        l.cin[i] = i == 0 ? 1 : mult[i] * nc;
        l.cout[i] = mult[i + 1] * nc;
        l.w[i] = o, o += (int64_t)9 * l.cin[i] * l.cout[i];
        l.sc[i] = o, o += l.cout[i];
        l.sh[i] = o, o += l.cout[i];
    }
    const int64_t d = 4 * (int64_t)nc;
    l.W1 = o, o += d * d;
    l.s1 = o, o += d;
    l.t1 = o, o += d;
    l.W2 = o, o += kCnnC * d;
    l.b2 = o, o += 16;
    l.total = o;
    return l;
}

// Who owns the excerpts of a launch.  Excerpt `i` of the launch is excerpt
// s = s_base + i of the stacked pool.
struct CnnGeom {
    const int64_t* item_offsets;  // [U + 1]
    const uint32_t* excl;         // bitmap over s, or nullptr
    const float* weights;         // [Uw, wstride]
    int64_t wstride;              // the record's floats; 0 when Uw == 1
    int64_t s_base;
    int U;
};

// The record of excerpt i's owner, or nullptr when the excerpt is excluded or
// no user owns it (block-uniform: every thread takes the same walk).
__device__ __forceinline__ const float* cnn_model(const CnnGeom& g, int64_t i, int* user = nullptr) {
    const int64_t s = g.s_base + i;
    if (g.excl && ((g.excl[s >> 5] >> (s & 31)) & 1u)) return nullptr;
    if (s < g.item_offsets[0] || s >= g.item_offsets[g.U]) return nullptr;
    int lo = 0, hi = g.U;  // item_offsets[lo] <= s < item_offsets[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (g.item_offsets[mid] <= s) lo = mid; else hi = mid;
    }
    if (user) *user = lo;
    return g.weights + (int64_t)lo * g.wstride;
}

// ReLU, the pool's maximum and the front end's clamp as torch computes them
// (relu, max_pool2d, clamp(min=)): a NaN goes through.  fmaxf would drop it.
__device__ __forceinline__ float cnn_relu(float v) { return v < 0.0f ? 0.0f : v; }
__device__ __forceinline__ float cnn_clamp_min(float v, float lo) { return v < lo ? lo : v; }
__device__ __forceinline__ float cnn_max(float a, float b) { return (b > a || b != b) ? b : a; }

// ---------------------------------------------------------------- front end
constexpr int kMelFrames = 8;                                        // frames per block
constexpr int kMelSpan = (kMelFrames - 1) * kCnnHop + kCnnFft;       // samples they cover
constexpr int kMelBlk = 32;                                          // terms per inner partial sum

// wave [S, L] (row pitch ld), basis [2, 512, 257] (cos plane, sin plane; the
// window multiplied in), fb [257, 128]; mel [S, 128, T], T = L / 256 + 1.
// Sums: a bin's 512 terms in 16 partial chains of 32 added in order onto the
// total; a mel band's 257 terms in one chain.  A NaN sample makes every
// band of the frames that cover it NaN (clamp(min=) keeps a NaN).
__global__ __launch_bounds__(256) void k_cnn_logmel(const float* __restrict__ wave, int64_t L, int64_t ld,
                                                    const float* __restrict__ basis, const float* __restrict__ fb,
                                                    float* __restrict__ mel, int T) {
    __shared__ float xs[kMelSpan];
    __shared__ float pw[kMelFrames][kCnnBins + 1];
    const int tid = threadIdx.x;
    const int64_t s = blockIdx.x;
    const int t0 = blockIdx.y * kMelFrames;
    const float* x = wave + s * ld;
    for (int i = tid; i < kMelSpan; i += 256) {
        int64_t p = (int64_t)t0 * kCnnHop - kCnnFft / 2 + i;
        if (p < 0) p = -p;
        if (p >= L) p = 2 * (L - 1) - p;
        xs[i] = (p >= 0 && p < L) ? x[p] : 0.0f;  // frames past T only (never stored)
    }
    __syncthreads();
    {
        const float* cb = basis + tid;
        const float* sb = basis + (int64_t)kCnnFft * kCnnBins + tid;
        float re[kMelFrames], im[kMelFrames];
#pragma unroll
        for (int j = 0; j < kMelFrames; ++j) re[j] = im[j] = 0.0f;
        for (int nb = 0; nb < kCnnFft; nb += kMelBlk) {
            float pr[kMelFrames], pi[kMelFrames];
#pragma unroll
            for (int j = 0; j < kMelFrames; ++j) pr[j] = pi[j] = 0.0f;
#pragma unroll 4
            for (int n = nb; n < nb + kMelBlk; ++n) {
                const float c = cb[(int64_t)n * kCnnBins], sn = sb[(int64_t)n * kCnnBins];
#pragma unroll
                for (int j = 0; j < kMelFrames; ++j) {
                    const float v = xs[j * kCnnHop + n];
                    pr[j] = fmaf(v, c, pr[j]);
                    pi[j] = fmaf(v, sn, pi[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < kMelFrames; ++j) re[j] += pr[j], im[j] += pi[j];
        }
#pragma unroll
        for (int j = 0; j < kMelFrames; ++j) pw[j][tid] = re[j] * re[j] + im[j] * im[j];
    }
    {  // bin 256 (its sine is zero): 32 lanes per frame, 16 terms each, a fixed tree
        const int j = tid >> 5, part = tid & 31;
        float p = 0.0f;
        for (int n = part * 16; n < part * 16 + 16; ++n)
            p = fmaf(xs[j * kCnnHop + n], basis[(int64_t)n * kCnnBins + 256], p);
        for (int d = 16; d >= 1; d >>= 1) p += __shfl_xor(p, d, 64);
        if (part == 0) pw[j][256] = p * p;
    }
    __syncthreads();
    const int m = tid & 127, jh = tid >> 7;
    float acc[kMelFrames / 2];
#pragma unroll
    for (int j = 0; j < kMelFrames / 2; ++j) acc[j] = 0.0f;
    for (int f = 0; f < kCnnBins; ++f) {
        const float w = fb[f * kCnnMels + m];
#pragma unroll
        for (int j = 0; j < kMelFrames / 2; ++j) acc[j] = fmaf(pw[jh * (kMelFrames / 2) + j][f], w, acc[j]);
    }
#pragma unroll
    for (int j = 0; j < kMelFrames / 2; ++j) {
        const int t = t0 + jh * (kMelFrames / 2) + j;
        if (t < T) mel[(s * kCnnMels + m) * T + t] = 10.0f * log10f(cnn_clamp_min(acc[j], 1e-10f));
    }
}

// ------------------------------------------------------------------ block 1
// mel [n, 128, T] -> out [n, 64, T / 2, nc].  nc / 4 threads per pooled pixel,
// thread c0 of them the channels c0 + j nc / 4 (j < 4: the 4 x 4 input patch is
// loaded once for four channels, and a store is a run of nc / 4 channels); the
// 9 taps row-major in one chain from 0.
constexpr int kB1Cpt = 4;

__global__ __launch_bounds__(256) void k_cnn_block1(const float* __restrict__ mel, int T, int nc, CnnGeom g,
                                                    int64_t w_off, int64_t sc_off, int64_t sh_off,
                                                    float* __restrict__ out) {
    const int64_t i = blockIdx.z;
    const float* wm = cnn_model(g, i);
    if (!wm) return;
    const int Wo = T / 2, Ho = kCnnMels / 2, q = nc / kB1Cpt;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= (int64_t)Ho * Wo * q) return;
    const int c0 = (int)(e % q);
    const int ox = (int)((e / q) % Wo), oy = (int)(e / ((int64_t)q * Wo));
    const float ss = wm[0], st = wm[1];
    const float* in = mel + i * kCnnMels * (int64_t)T;
    float p[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int y = 2 * oy - 1 + r, x = 2 * ox - 1 + k;
            p[r][k] = (y >= 0 && y < kCnnMels && x >= 0 && x < T) ? fmaf(ss, in[(int64_t)y * T + x], st) : 0.0f;
        }
    float* o = out + (i * Ho * Wo + (int64_t)oy * Wo + ox) * nc;
#pragma unroll
    for (int j = 0; j < kB1Cpt; ++j) {
        const int c = c0 + j * q;
        float w[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) w[t] = wm[w_off + t * nc + c];
        const float sc = wm[sc_off + c], sh = wm[sh_off + c];
        float best = 0.0f;
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int dx = 0; dx < 2; ++dx) {
                float a = 0.0f;
#pragma unroll
                for (int t = 0; t < 9; ++t) a = fmaf(p[dy + t / 3][dx + t % 3], w[t], a);
                const float v = cnn_relu(fmaf(sc, a, sh));
                best = (dy | dx) ? cnn_max(best, v) : v;
            }
        o[c] = best;
    }
}

// --------------------------------------------------------------- blocks 2-7
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kConvTH = 8, kConvTW = 16;                  // the block's pixel tile (even: whole pool windows)
constexpr int kConvPH = kConvTH + 2, kConvPW = kConvTW + 2;  // with its halo
constexpr int kConvCK = 8, kConvCKP = 9;                  // channels per chunk, and their pitch in LDS

struct CnnConvArgs {
    const float* in;  // [n, H, W, Cin]
    float* out;       // [n, H / 2, W / 2, Cout]
    int64_t w_off, sc_off, sh_off;
    int H, W, Cin, Cout;
};

// 4 waves; wave v owns pixel rows 2v, 2v + 1 of the tile: MFMA row m is pool
// window m >> 2 of that row pair, pixel (dy, dx) = ((m >> 1) & 1, m & 1) of it,
// so a lane's accumulator registers 4g .. 4g + 3 are one window (the C/D map:
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), column = lane & 31) and the
// pool needs no other lane.  NT 32-wide Cout tiles per wave share its A value.
template <int NT>
__global__ __launch_bounds__(256) void k_cnn_conv(CnnConvArgs a, CnnGeom g) {
    constexpr int BN = 32 * NT;
    __shared__ float As[kConvPH * kConvPW * kConvCKP];
    __shared__ __attribute__((aligned(16))) float Bs[9 * kConvCK * BN];
    const int64_t i = blockIdx.z;
    const float* wm = cnn_model(g, i);
    if (!wm) return;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, m = lane & 31, half = lane >> 5;
    const int tiles_x = (a.W + kConvTW - 1) / kConvTW;
    const int y0 = (blockIdx.x / tiles_x) * kConvTH, x0 = (blockIdx.x % tiles_x) * kConvTW, n0 = blockIdx.y * BN;
    const int py = 2 * wv + ((m >> 1) & 1), px = 2 * (m >> 2) + (m & 1);
    const float* in = a.in + i * a.H * (int64_t)a.W * a.Cin;
    const float* w = wm + a.w_off;
    f32x16 acc[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[nt][r] = 0.0f;
    for (int c0 = 0; c0 < a.Cin; c0 += kConvCK) {
        __syncthreads();  // the previous chunk's reads are done
        for (int e = tid; e < kConvPH * kConvPW * 2; e += 256) {
            const int p = e >> 1, q = e & 1;
            const int y = y0 - 1 + p / kConvPW, x = x0 - 1 + p % kConvPW;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (y >= 0 && y < a.H && x >= 0 && x < a.W)
                v = *reinterpret_cast<const float4*>(in + ((int64_t)y * a.W + x) * a.Cin + c0 + 4 * q);
            float* d = As + p * kConvCKP + 4 * q;
            d[0] = v.x, d[1] = v.y, d[2] = v.z, d[3] = v.w;
        }
        for (int e = tid; e < 9 * kConvCK * (BN / 4); e += 256) {
            const int kk = e / (BN / 4), cq = e % (BN / 4);
            const int col = n0 + 4 * cq;
            float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (col < a.Cout)
                v = *reinterpret_cast<const float4*>(
                    w + ((int64_t)(kk / kConvCK) * a.Cin + c0 + (kk % kConvCK)) * a.Cout + col);
            *reinterpret_cast<float4*>(Bs + kk * BN + 4 * cq) = v;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 9; ++t) {
            const float* ap = As + ((py + t / 3) * kConvPW + px + t % 3) * kConvCKP + half;
            const float* bp = Bs + (t * kConvCK + half) * BN + m;
#pragma unroll
            for (int cp = 0; cp < kConvCK / 2; ++cp) {
                const float av = ap[2 * cp];
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[nt] = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bp[2 * cp * BN + nt * 32], acc[nt], 0, 0, 0);
            }
        }
    }
    const int Ho = a.H / 2, Wo = a.W / 2;
    const int oy = (y0 >> 1) + wv;
    if (oy >= Ho) return;
    float* out = a.out + (i * Ho + oy) * (int64_t)Wo * a.Cout;
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) {
        const int col = n0 + nt * 32 + m;
        if (col >= a.Cout) continue;
        const float sc = wm[a.sc_off + col], sh = wm[a.sh_off + col];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int ox = (x0 >> 1) + 2 * q + half;
            if (ox >= Wo) continue;
            float best = cnn_relu(fmaf(sc, acc[nt][4 * q], sh));
#pragma unroll
            for (int r = 1; r < 4; ++r) best = cnn_max(best, cnn_relu(fmaf(sc, acc[nt][4 * q + r], sh)));
            out[(int64_t)ox * a.Cout + col] = best;
        }
    }
}

// --------------------------------------------------------------------- head
struct CnnHeadArgs {
    const float* in;  // [n, Wf, D], D = 4nc
    int Wf, D;
    int64_t W1, s1, t1, W2, b2;
    float* out;  // [*, 4] by s, row pitch ld_out
    int64_t ld_out;
    const int32_t* y;        // by s, or nullptr
    unsigned long long* cm;  // [U, 4, 4], or nullptr
};

// One block per excerpt.  dense1: a thread per output, its D terms in one
// chain; dense2: a wave per class, lane l the terms l, l + 64, .. in one chain,
// the 64 partial sums by a fixed xor tree, then the bias.
__global__ __launch_bounds__(256) void k_cnn_head(CnnHeadArgs a, CnnGeom g) {
    extern __shared__ float hsm[];
    float* f = hsm;
    float* h = hsm + a.D;
    __shared__ float p[kCnnC];
    const int64_t i = blockIdx.x;
    int u = 0;
    const float* wm = cnn_model(g, i, &u);
    if (!wm) return;
    const int tid = threadIdx.x;
    const float* in = a.in + i * a.Wf * (int64_t)a.D;
    for (int c = tid; c < a.D; c += 256) {
        float v = in[c];
        for (int x = 1; x < a.Wf; ++x) v = cnn_max(v, in[(int64_t)x * a.D + c]);
        f[c] = v;
    }
    __syncthreads();
    for (int o = tid; o < a.D; o += 256) {
        const float* w1 = wm + a.W1 + o;
        float s = 0.0f;
        for (int k = 0; k < a.D; ++k) s = fmaf(w1[(int64_t)k * a.D], f[k], s);
        h[o] = cnn_relu(fmaf(wm[a.s1 + o], s, wm[a.t1 + o]));
    }
    __syncthreads();
    const int c = tid >> 6, lane = tid & 63;
    {
        const float* w2 = wm + a.W2 + (int64_t)c * a.D;
        float s = 0.0f;
        for (int k = lane; k < a.D; k += 64) s = fmaf(w2[k], h[k], s);
        for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
        if (lane == 0) p[c] = 1.0f / (1.0f + expf(-(s + wm[a.b2 + c])));
    }
    __syncthreads();
    if (tid >= kCnnC) return;
    const int64_t s = g.s_base + i;
    a.out[s * a.ld_out + tid] = p[tid];
    if (tid == 0 && a.y && a.cm) {
        const int yv = a.y[s];
        if (yv >= 0 && yv < kCnnC) {
            const float q[kCnnC] = {p[0], p[1], p[2], p[3]};
            atomicAdd(a.cm + ((int64_t)u * kCnnC + yv) * kCnnC + np_argmax(q, kCnnC), 1ull);
        }
    }
}

}  // namespace ce
