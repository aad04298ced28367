// ce_xgb_fit.hpp -- on-device XGBClassifier refit (amg_test.py:507,
// mod.fit(X_batch, y, xgb_model=mod.get_booster())): every user's boosting
// rounds in one launch.  What is computed is stated row by row in include/ce.h
// (ce_xgb_fit_users) and restated in tests/xgb_fit_ref.py, which this header
// matches bit for bit; parity with xgboost 1.3.3 itself is unpinned (DESIGN.md
// §3 lists every choice, next to the predictor's).  ce_xgb_fit.hip
// instantiates the kernels.
//
// Two launches:
//   k_xgb_fit_margins  the start margins of every batch row: the users walk of
//                      ce_xgb_users.hpp with a finish that keeps the margins
//                      (no second walk), the batch as its geometry -- user u's
//                      "songs" are its batch rows, one frame each;
//   k_xgb_fit          one block per user: the finite check, every feature's
//                      stable sort (once per fit, kept in the workspace: the
//                      sorted indices do not fit the LDS), then the rounds, a
//                      serial chain.
//
// The split search: thread t owns feature t (+ blockDim per pass) and scans its
// sorted column from the high end, accumulating each open node's right side in
// double, serially: the contract's summation order.  The per-node scan state of
// every thread lives in LDS, 8 open nodes at a time (28 B per node and thread);
// the 16 open nodes the last level of a depth-5 tree can have take two scans.
// The only cross-thread reduction is over candidates (loss_chg, feature), by the
// tie rule: taken in feature order, a later one must be strictly greater.
// The end-of-column candidate of xgboost's scan never fires on a dense column
// (its left side holds no row, so its hessian is below min_child_weight) and is
// left out.
//
// What is measured and what is not (profiles/xgb_fit.json: 500 users x 400 rows
// x 260 features, whole calls only): the structure was chosen for the
// contract's summation order, not by A/B.  The candidate reduction (8 threads,
// each walking the pass's threads serially), the node statistics (one thread
// per open node over all rows) and the rank sort (n^2 / 8 loads per thread,
// 2 M at the 4096-row cap, which itself is only what the LDS holds) have no
// measurement of their own; batches near the cap are untimed.  Their bits are
// tested (tests/test_gpu_xgb_fit_edges.py: 4095 and 4096 rows, and 4096 rows x
// 512 features, the largest LDS the entry accepts).
#pragma once
#include "ce_xgb_users.hpp"

namespace ce {

constexpr int kXgbFitMaxRows = 4096;  // rows of one user's batch (sorted indices are 16 bits; g, h, pos in LDS)
constexpr int kXgbFitMaxDepth = 5;
constexpr int kXgbFitNodes = 63;      // a depth-5 tree
constexpr int kXgbFitSlots = 8;       // open nodes scanned at once
constexpr int kXgbFitOpen = 32;       // open nodes of one level (the last one's are only weighed)
constexpr int kXgbFitMaxThreads = 512;

// threads of a user's block: one per feature up to 512, whole waves
inline int xgb_fit_threads(int D) { return 64 * (((D < kXgbFitMaxThreads ? D : kXgbFitMaxThreads) + 63) / 64); }
inline int xgb_fit_rows_pad(int64_t n_max) { return (int)((n_max + 7) & ~(int64_t)7); }
// dynamic LDS of k_xgb_fit: the scan state, the tree under construction, the rows' g, h and node
inline size_t xgb_fit_lds_bytes(int NT, int nr) {
    return (size_t)kXgbFitSlots * NT * 28 + 64 * 16 + 64 * 12 + kXgbFitOpen * 12 + 64 * 2 + 64 * 2 + 2 * kXgbFitOpen +
           16 + (size_t)nr * 9;
}

// the workspace's parts (byte offsets, each 16-byte aligned)
struct XgbFitWs {
    size_t ident, m0, m1, sval, sidx, total;
    int Dp;  // the sorted indices' row pitch (D rounded up to even)
};
inline XgbFitWs xgb_fit_ws(int64_t R, int D, int G) {
    auto up = [](size_t v) { return (v + 15) & ~(size_t)15; };
    XgbFitWs w;
    w.Dp = (D + 1) & ~1;
    w.ident = 0;
    w.m0 = up((size_t)(R + 1) * sizeof(int64_t));
    w.m1 = w.m0 + up((size_t)R * G * sizeof(float));
    w.sval = w.m1 + up((size_t)R * G * sizeof(float));
    w.sidx = w.sval + up((size_t)R * D * sizeof(float));
    w.total = w.sidx + up((size_t)R * w.Dp * sizeof(uint16_t));
    return w;
}

// ---- start margins: the users walk with a finish that keeps them ---------------
struct XgbMarginFin : NoCounts {
    using takes_margins = void;
    float* m;  // [R, G] by CSR position
    __device__ __forceinline__ void row(const float (&)[kXgbMaxGroups], int, int64_t) {}
    __device__ __forceinline__ void margins(const float* mg, int G, int lane, int64_t q) {
        for (int g = 0; g < G; ++g) m[q * G + g] = mg[g * 64 + lane];
    }
};

// ident[i] = i, i <= R: the frame_offsets of a geometry whose songs are single rows
__global__ void k_xgb_fit_ident(int64_t* ident, int64_t R) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i <= R) ident[i] = i;
}

template <int XDT, int KF>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8, 8))) void k_xgb_fit_margins(
    XgbArgs a, UsersGeom ug, float* m, const uint2* __restrict__ table, const int32_t* __restrict__ tree_ids,
    const int32_t* __restrict__ group_offsets, int TT, int depth, int64_t L) {
    XgbMarginFin fin{{}, m};
    xgb_users<XDT, KF>(a, XgbUsersForests{table, tree_ids, group_offsets, TT, depth, L}, ug, fin);
}

// ---- the fit ----------------------------------------------------------------------
struct XgbFitArgs {
    const void* X;
    int64_t F;
    int D;
    int64_t ld;
    const int64_t* rows;         // [R] rows of X
    const int32_t* labels;       // [R]
    const int64_t* row_offsets;  // [U + 1]
    int G, rounds, max_depth, pack_depth, nr;  // nr: rows the LDS was sized for
    float eta, lambda, mcw;
    // outputs: tree (u rounds + r) G + k
    uint32_t* nodes;    // [T][2^pd - 1 (at least 1)][2]
    float* leaves;      // [T][2^pd]
    int32_t* left;      // [T][63]
    int32_t* right;     // [T][63]
    int32_t* split;     // [T][63]
    float* cond;        // [T][63]
    uint8_t* dleft;     // [T][63]
    int32_t* num_nodes; // [T]
    float* margins;     // [R, G] or nullptr
    int32_t* status;    // [U]
    // workspace
    float* m0;
    float* m1;
    float* sval;        // [R][D] the sorted values
    uint16_t* sidx;     // [R][Dp] the sorted batch positions
    int Dp;
};

template <int XDT>
__device__ __forceinline__ float xgb_fit_x(const void* X, int64_t at) {
    if constexpr (XDT == CE_F64)
        return (float)static_cast<const double*>(X)[at];
    else
        return static_cast<const float*>(X)[at];
}

template <int XDT>
__global__ __launch_bounds__(kXgbFitMaxThreads) void k_xgb_fit(XgbFitArgs a) {
    extern __shared__ double fsm[];
    const int NT = blockDim.x, tid = threadIdx.x, u = blockIdx.x;
    const int64_t r0 = a.row_offsets[u];
    const int64_t n64 = a.row_offsets[u + 1] - r0;
    if (n64 <= 0) return;  // no row: no new tree
    if (n64 > a.nr) {      // a batch the call was not sized for: not run
        if (tid == 0) a.status[u] = 2;
        return;
    }
    const int n = (int)n64, D = a.D, G = a.G;
    // ---- LDS ----
    double* eG = fsm;                         // [8][NT] the scan's right side per open node
    double* eH = eG + kXgbFitSlots * NT;      // [8][NT]
    double* nG = eH + kXgbFitSlots * NT;      // [64] node sums
    double* nH = nG + 64;                     // [64]
    float* eL = reinterpret_cast<float*>(nH + 64);  // [8][NT] last value seen
    float* bL = eL + kXgbFitSlots * NT;       // [8][NT] the thread's best loss_chg
    float* bT = bL + kXgbFitSlots * NT;       // [8][NT] and its threshold
    float* nW = bT + kXgbFitSlots * NT;       // [64] node weight
    float* nR = nW + 64;                      // [64] root gain
    float* ncond = nR + 64;                   // [64] split condition / leaf value
    float* obL = ncond + 64;                  // [32] the open node's best
    float* obT = obL + kXgbFitOpen;           // [32]
    int* obF = reinterpret_cast<int*>(obT + kXgbFitOpen);  // [32]
    float* gr = reinterpret_cast<float*>(obF + kXgbFitOpen);  // [nr]
    float* hs = gr + a.nr;                    // [nr]
    int16_t* nsplit = reinterpret_cast<int16_t*>(hs + a.nr);  // [64]
    int8_t* nleft = reinterpret_cast<int8_t*>(nsplit + 64);   // [64] left child (-1: a leaf); right = left + 1
    int8_t* nslot = nleft + 64;               // [64] the node's place among the open ones (-1: not open)
    int8_t* openl = nslot + 64;               // [32] open nodes in id order
    int8_t* nextl = openl + kXgbFitOpen;      // [32]
    int* ctl = reinterpret_cast<int*>(nextl + kXgbFitOpen);  // [4] nopen, nnodes, bad, nnext
    uint8_t* pos = reinterpret_cast<uint8_t*>(ctl + 4);       // [nr] the row's node

    // ---- the batch is dense, finite and in range, or the user is flagged and left alone ----
    if (tid == 0) ctl[2] = 0;
    __syncthreads();
    {
        bool bad = false;
        for (int i = tid; i < n; i += NT) {
            const int64_t row = a.rows[r0 + i];
            const int y = a.labels[r0 + i];
            bad |= row < 0 || row >= a.F || y < 0 || y >= G;
        }
        if (bad) ctl[2] = 1;
    }
    __syncthreads();
    if (ctl[2] == 0) {
        bool bad = false;
        for (int f = tid; f < D; f += NT)
            for (int i = 0; i < n; ++i) {
                const float x = xgb_fit_x<XDT>(a.X, a.rows[r0 + i] * a.ld + f);
                bad |= !(__builtin_fabsf(x) < __builtin_inff());
            }
        if (bad) ctl[2] = 1;
    }
    __syncthreads();
    if (ctl[2] != 0) {  // block-uniform
        if (tid == 0) a.status[u] = 1;
        return;
    }

    // ---- every feature's stable sort, once per fit: rank = rows below, and equal rows before ----
    // (8 rows ranked per pass over the column: an eighth of the loads)
    for (int f = tid; f < D; f += NT) {
        for (int i0 = 0; i0 < n; i0 += 8) {
            float xi[8];
            int rank[8];
#pragma unroll
            for (int q = 0; q < 8; ++q) {
                xi[q] = xgb_fit_x<XDT>(a.X, a.rows[r0 + min(i0 + q, n - 1)] * a.ld + f);
                rank[q] = 0;
            }
            for (int j = 0; j < n; ++j) {
                const float xj = xgb_fit_x<XDT>(a.X, a.rows[r0 + j] * a.ld + f);
#pragma unroll
                for (int q = 0; q < 8; ++q) rank[q] += (xj < xi[q] || (xj == xi[q] && j < i0 + q)) ? 1 : 0;
            }
#pragma unroll
            for (int q = 0; q < 8; ++q)
                if (i0 + q < n) {
                    a.sval[(r0 + rank[q]) * D + f] = xi[q];
                    a.sidx[(r0 + rank[q]) * a.Dp + f] = (uint16_t)(i0 + q);
                }
        }
    }
    __syncthreads();

    const double lam = (double)a.lambda, mcw = (double)a.mcw;
    const int pd = a.pack_depth, NIp = (1 << pd) - 1, NLp = 1 << pd, NIs = NIp > 0 ? NIp : 1;
    float* cur = a.m0;
    float* nxt = a.m1;
    for (int r = 0; r < a.rounds; ++r) {
        for (int k = 0; k < G; ++k) {
            // ---- gradients of group k from the round's starting margins ----
            for (int i = tid; i < n; i += NT) {
                const float* mi = cur + (r0 + i) * G;
                float p[kXgbMaxGroups];
                float mx = mi[0];
                for (int g = 1; g < G; ++g) mx = fmaxf(mi[g], mx);
                double wsum = 0.0;
                for (int g = 0; g < G; ++g) {
                    p[g] = glibc_expf(mi[g] - mx);
                    wsum += p[g];
                }
                const float ws = (float)wsum;
                float pk = 0.0f;
                for (int g = 0; g < G; ++g) {
                    const float q = p[g] / ws;
                    if (g == k) pk = q;
                }
                gr[i] = pk - (a.labels[r0 + i] == k ? 1.0f : 0.0f);
                hs[i] = fmaxf(2.0f * pk * (1.0f - pk), 1e-16f);
                pos[i] = 0;
            }
            if (tid < 64) {
                nleft[tid] = -1;
                nslot[tid] = -1;
                nsplit[tid] = 0;
                ncond[tid] = 0.0f;
            }
            if (tid == 0) {
                ctl[0] = 1;
                ctl[1] = 1;
                openl[0] = 0;
            }
            __syncthreads();
            if (tid == 0) nslot[0] = 0;
            for (int depth = 0;; ++depth) {
                __syncthreads();
                const int nopen = ctl[0];
                if (nopen == 0) break;  // block-uniform
                // ---- node statistics: double sums over the node's rows in batch order ----
                if (tid < nopen) {
                    const int nid = openl[tid];
                    double sg = 0.0, sh = 0.0;
                    for (int i = 0; i < n; ++i)
                        if (pos[i] == nid) {
                            sg += (double)gr[i];
                            sh += (double)hs[i];
                        }
                    nG[nid] = sg;
                    nH[nid] = sh;
                    nW[nid] = (float)(-sg / (sh + lam));
                    nR[nid] = (float)(sg * sg / (sh + lam));
                    obL[tid] = 0.0f;
                    obT[tid] = 0.0f;
                    obF[tid] = 0;
                }
                __syncthreads();
                if (depth == a.max_depth) {  // still open after max_depth levels: leaves
                    if (tid < nopen) ncond[openl[tid]] = nW[openl[tid]] * a.eta;
                    __syncthreads();
                    break;
                }
                // ---- the split search, 8 open nodes at a time ----
                for (int sg0 = 0; sg0 < nopen; sg0 += kXgbFitSlots) {
                    for (int f0 = 0; f0 < D; f0 += NT) {  // block-uniform
                        const int f = f0 + tid;
                        for (int s = 0; s < kXgbFitSlots; ++s) {
                            eG[s * NT + tid] = 0.0;
                            eH[s * NT + tid] = 0.0;
                            eL[s * NT + tid] = 0.0f;
                            bL[s * NT + tid] = 0.0f;
                            bT[s * NT + tid] = 0.0f;
                        }
                        if (f < D) {
                            for (int j0 = n; j0 > 0; j0 -= 8) {
                                int idx[8];
                                float fv[8];
#pragma unroll
                                for (int q = 0; q < 8; ++q) {
                                    const int j = max(j0 - 1 - q, 0);
                                    idx[q] = min((int)a.sidx[(r0 + j) * a.Dp + f], n - 1);
                                    fv[q] = a.sval[(r0 + j) * D + f];
                                }
#pragma unroll
                                for (int q = 0; q < 8; ++q) {
                                    if (j0 - 1 - q < 0) break;
                                    const int nid = pos[idx[q]];
                                    const unsigned s = (unsigned)((int)nslot[nid] - sg0);
                                    if (s >= (unsigned)kXgbFitSlots) continue;
                                    const int at = (int)s * NT + tid;
                                    const double eg = eG[at], eh = eH[at];
                                    const float last = eL[at];
                                    // eh > 0: the node has seen a row (every hessian is positive)
                                    if (eh > 0.0 && fv[q] != last && eh >= mcw) {
                                        const double cg = nG[nid] - eg, ch = nH[nid] - eh;
                                        if (ch >= mcw) {
                                            const float lc =
                                                (float)(cg * cg / (ch + lam) + eg * eg / (eh + lam) - (double)nR[nid]);
                                            if (__builtin_fabsf(lc) < __builtin_inff() && lc > bL[at]) {
                                                bL[at] = lc;
                                                bT[at] = (fv[q] + last) * 0.5f;
                                            }
                                        }
                                    }
                                    eG[at] = eg + (double)gr[idx[q]];
                                    eH[at] = eh + (double)hs[idx[q]];
                                    eL[at] = fv[q];
                                }
                            }
                        }
                        __syncthreads();
                        // the candidates of this pass in feature order: a later one must be strictly greater
                        if (tid < kXgbFitSlots && sg0 + tid < nopen) {
                            const int o = sg0 + tid;
                            float best = obL[o], thr = obT[o];
                            int bf = obF[o];
                            const int lim = min(NT, D - f0);
                            for (int t = 0; t < lim; ++t) {
                                const float lc = bL[tid * NT + t];
                                if (lc > best) {
                                    best = lc;
                                    thr = bT[tid * NT + t];
                                    bf = f0 + t;
                                }
                            }
                            obL[o] = best;
                            obT[o] = thr;
                            obF[o] = bf;
                        }
                        __syncthreads();
                    }
                }
                // ---- expand the level: open nodes in id order ----
                if (tid == 0) {
                    int nn = ctl[1], nnext = 0;
                    for (int o = 0; o < nopen; ++o) {
                        const int nid = openl[o];
                        nslot[nid] = -1;
                        if (obL[o] > 1e-6f && nn + 2 <= kXgbFitNodes) {
                            nleft[nid] = (int8_t)nn;
                            nsplit[nid] = (int16_t)obF[o];
                            ncond[nid] = obT[o];
                            nextl[nnext++] = (int8_t)nn;
                            nextl[nnext++] = (int8_t)(nn + 1);
                            nn += 2;
                        } else {
                            ncond[nid] = nW[nid] * a.eta;
                        }
                    }
                    for (int o = 0; o < nnext; ++o) {
                        openl[o] = nextl[o];
                        nslot[nextl[o]] = (int8_t)o;
                    }
                    ctl[0] = nnext;
                    ctl[1] = nn;
                }
                __syncthreads();
                // ---- the rows of a split node move to its children ----
                for (int i = tid; i < n; i += NT) {
                    const int nid = pos[i];
                    const int l = nleft[nid];
                    if (l >= 0) {
                        const float x = xgb_fit_x<XDT>(a.X, a.rows[r0 + i] * a.ld + nsplit[nid]);
                        pos[i] = (uint8_t)(x < ncond[nid] ? l : l + 1);
                    }
                }
            }
            __syncthreads();
            // ---- the margin of group k, and the tree in both forms ----
            for (int i = tid; i < n; i += NT) {
                const int64_t at = (r0 + i) * G + k;
                nxt[at] = cur[at] + ncond[pos[i]];
            }
            const int64_t t = ((int64_t)u * a.rounds + r) * G + k;
            const int nn = ctl[1];
            if (tid < kXgbFitNodes) {
                const int l = tid < nn ? nleft[tid] : -1;
                a.left[t * kXgbFitNodes + tid] = l;
                a.right[t * kXgbFitNodes + tid] = l >= 0 ? l + 1 : -1;
                a.split[t * kXgbFitNodes + tid] = l >= 0 ? nsplit[tid] : 0;
                a.cond[t * kXgbFitNodes + tid] = tid < nn ? ncond[tid] : 0.0f;
                a.dleft[t * kXgbFitNodes + tid] = l >= 0 ? 1 : 0;  // dense columns: the backward scan only
            }
            if (tid == 0) a.num_nodes[t] = nn;
            for (int e = tid; e < NIp + NLp; e += NT) {
                // perfect-tree entry e: inner node e (e < NIp) or leaf e - NIp; its path from the root
                const int h = e + 1;                    // 1-based heap index
                const int dep = 31 - __builtin_clz(h);  // its depth
                int nid = 0, d = 0;
                for (; d < dep && nleft[nid] >= 0; ++d) nid = nleft[nid] + ((h >> (dep - 1 - d)) & 1);
                if (e < NIp) {
                    // below a model leaf (or at it) the inner nodes stay {0, +0.0}: either branch, same leaf
                    const bool inner = d == dep && nleft[nid] >= 0;
                    a.nodes[(t * NIs + e) * 2] = inner ? ((uint32_t)nsplit[nid] | 0x80000000u) : 0u;
                    a.nodes[(t * NIs + e) * 2 + 1] = inner ? __float_as_uint(ncond[nid]) : 0u;
                } else {
                    a.leaves[t * NLp + (e - NIp)] = ncond[nid];  // a leaf above covers every leaf below it
                }
            }
            if (NIp == 0 && tid == 0) {
                a.nodes[t * 2] = 0u;
                a.nodes[t * 2 + 1] = 0u;
            }
            __syncthreads();
        }
        float* sw = cur;
        cur = nxt;
        nxt = sw;
    }
    if (a.margins)
        for (int i = tid; i < n * G; i += NT) a.margins[r0 * G + i] = cur[r0 * G + i];
}

}  // namespace ce
