// One model per graph beyond a CU's LDS (include/gcnmaxcut.h, gmc_inst_large_*): the two kernels of the gmc_inst_* sequence
// that are bound by a graph's size, for graphs of up to GMC_LARGE_MAX_GRAPH_NODES nodes.
//   linst_hw2    inst_hw2_k_kernel of instance.hip with a walk over the graph's 4-row tiles: grid (graph, min(tiles, 65535))
//                and workgroup y takes tiles y, y + gridDim.y, ...  The row arithmetic is that kernel's (one wave per row,
//                lane j columns j, j + 64, ..., then gmc::wave_sum), and a row's bytes do not depend on the workgroup that
//                takes it: H and Z0 equal inst_hw2_k_kernel's byte for byte on every batch both launch shapes hold.
//   the head     large.hip's four launches (prob + decode, loss terms + softmax backward, per-graph fold, GY2) on its grid
//                (graph, tile of kLargeTile = 256 rows), with its slots and its summation orders (stated there), and three
//                differences: the bias is the graph's own, b2 + g * K; the number of terminals is a run-time value,
//                terms = terminals ? min(n, K) : 0, also for the relaxed loss's "the neighbour is a terminal"; and the fold
//                writes db2_g straight into the gradient's [B,K] block.
// Kernel boundaries are the only synchronisation between workgroups: no spin waits, no arrival counters, no float atomics
// (the fold's one system-scope store of `loss` is large.hip's).  Every sum in a fixed order that depends on the graph alone:
// a graph's results have the same bits wherever it stands in a batch and whatever stands next to it.
#include "large_rows.h"

namespace {

// ---- linst_hw2 ------------------------------------------------------------------------------------------------------
struct LinstHw2Args {
    const int *goff;
    float *H;            // [R,ld] in: dinv o (A @ T0); out: relu(. + b1_g)
    const float *dinv;
    const float *b1;     // [B,F]
    const float *W2;     // [B,F,K]
    float *Z0;           // [R,K]
    int F;
    long ld;
};

constexpr int kHw2Rows = 4;          // rows per tile: one per wave
constexpr int kMaxGridY = 65535;

template <int K>
__global__ __launch_bounds__(256) void linst_hw2_kernel(LinstHw2Args a) {
    const int g = blockIdx.x;
    const int r0 = a.goff[g];
    const int n = a.goff[g + 1] - r0;
    const int lane = gmc::lane_id();
    const float *b1 = a.b1 + (long)g * a.F;
    const float *W2 = a.W2 + (long)g * a.F * K;
    const int stride = (int)gridDim.y * kHw2Rows;
    for (int l = gmc::uniform((int)(blockIdx.y * kHw2Rows + (threadIdx.x >> 6))); l < n; l += stride) {
        const long r = (long)r0 + l;
        float *h_row = a.H + r * a.ld;
        float z[K] = {};
        for (int c = lane; c < a.F; c += GMC_WAVE) {
            const float pre = h_row[c] + b1[c];
            const float h = pre > 0.f ? pre : 0.f;
            h_row[c] = h;
            float w[K];
            load_row<K>(W2, c, w);
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] = fmaf(h, w[k], z[k]);
        }
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] = gmc::wave_sum(z[k]);
        if (lane == 0) {
            const float d = a.dinv[r];
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] *= d;
            store_row<K>(a.Z0, r, z);
        }
    }
}

// ---- the head -------------------------------------------------------------------------------------------------------
struct LinstHeadArgs {
    gmc_batch b;
    const float *Z0;   // [R,K]
    const float *b2;   // [B,K]
    float C;
    int terminals;     // 1: rows 0..K-1 of a graph are its terminals; 0: no row is overridden
    float *P;          // [R,K]
    int *S;            // caller's, optional
    int *Sw;           // [R] workspace
    float *loss;
    float *GZd;        // [R,K] dinv o GZ; nullptr: forward only
    float *headpart;   // [slots][K+1]
    float *GY2;        // [R,K]
    float *db2;        // [B,K]: the gradient's block
};

template <int K>
__device__ __forceinline__ int terminals_of(const LinstHeadArgs &a, int n) {
    return a.terminals ? (n < K ? n : K) : 0;
}

template <int K>
__global__ __launch_bounds__(kLargeTile) void linst_prob_kernel(LinstHeadArgs a) {
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    float z[K] = {};
    gather_sum<K>(a.b, a.Z0, beg, end, live, z);
    if (!live) return;
    const int terms = terminals_of<K>(a, t.n);
    const float *b2 = a.b2 + (long)t.g * K;
    const float d = a.b.dinv[r];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) { z[k] = fmaf(z[k], d, b2[k]); m = fmaxf(m, z[k]); }
    float p[K], sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] = expf(z[k] - m); sum += p[k]; }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] *= inv;
    store_row<K>(a.P, r, p);
    int s;
    if (t.l < terms) {
        s = t.l;
    } else {
        s = 0;  // torch.argmax: first maximum wins
        float best = p[0];
#pragma unroll
        for (int k = 1; k < K; ++k)
            if (p[k] > best) { best = p[k]; s = k; }
    }
    a.Sw[r] = s;
    if (a.S) a.S[r] = s;
}

template <int K, bool SOFT>
__global__ __launch_bounds__(kLargeTile) void linst_loss_kernel(LinstHeadArgs a) {
    __shared__ float red[kLargeWaves * (K + 1)];
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    const int terms = terminals_of<K>(a, t.n);
    const bool train = a.GZd != nullptr;
    float v[K + 1] = {};   // gp[0..K-1], cut
    if constexpr (SOFT) {
        float u[K];        // Pt of this row
        if (t.l < terms) {
#pragma unroll
            for (int k = 0; k < K; ++k) u[k] = k == t.l ? 1.f : 0.f;
        } else {
            load_row<K>(a.P, r, u);
        }
        row_terms<K + 1, K>(beg, end, live, u, v, [&](int e, float (&acc)[K + 1], const float (&me)[K]) {
            const float w = a.b.vals ? a.b.vals[e] : 1.0f;
            const int lc = a.b.lcol[e];
            float q[K];
            if (lc < terms) {   // a terminal: e_lcol
#pragma unroll
                for (int k = 0; k < K; ++k) q[k] = k == lc ? 1.f : 0.f;
            } else {
                load_row<K>(a.P, a.b.gcol[e], q);
            }
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) { acc[k] += w * q[k]; dot += me[k] * q[k]; }
            acc[K] += w * (1.0f - dot);
        });
    } else {
        const float me[1] = {__int_as_float(a.Sw[r])};
        row_terms<K + 1, 1>(beg, end, live, me, v, [&](int e, float (&acc)[K + 1], const float (&mine)[1]) {
            const float w = a.b.vals ? a.b.vals[e] : 1.0f;
            const int sc = a.Sw[a.b.gcol[e]];
#pragma unroll
            for (int k = 0; k < K; ++k) acc[k] += sc == k ? w : 0.f;
            acc[K] += sc != __float_as_int(mine[0]) ? w : 0.f;
        });
    }
    float acc[K + 1] = {};  // cut, db2[0..K-1]
    if (live) {
        acc[0] = v[K];
        if (train) {
            float p[K];
            load_row<K>(a.P, r, p);   // the row's own softmax output (a terminal's too)
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) { v[k] *= a.C; dot += v[k] * p[k]; }
            const float d = a.b.dinv[r];
            float gz[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float zk = p[k] * (v[k] - dot);
                acc[1 + k] = zk;
                gz[k] = zk * d;
            }
            store_row<K>(a.GZd, r, gz);
        }
    }
    block_sum<K + 1, kLargeWaves>(acc, red);
    if (threadIdx.x == 0) {
        float *out = a.headpart + part_slot(t) * (K + 1);
#pragma unroll
        for (int k = 0; k <= K; ++k) out[k] = acc[k];
    }
}

// one workgroup (a wave) per graph; lane k < K + 1 folds sum k
template <int K>
__global__ __launch_bounds__(GMC_WAVE) void linst_fold_kernel(LinstHeadArgs a) {
    const int g = blockIdx.x, k = threadIdx.x;
    if (k > K) return;
    const int r0 = a.b.goff[g], n = a.b.goff[g + 1] - r0;
    const int tiles = (n + kLargeTile - 1) / kLargeTile;
    const float *p = a.headpart + ((long)(r0 / kLargeTile) + g) * (K + 1) + k;
    float s = 0.f;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) s += p[(long)t * (K + 1)];
    if (k == 0) {
        // one system-scope store: `loss` may be pinned host memory the caller watches
        if (a.loss) __hip_atomic_store(a.loss + g, -a.C * (s * 0.5f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else if (a.GZd) {
        a.db2[(long)g * K + (k - 1)] = s;
    }
}

template <int K>
__global__ __launch_bounds__(kLargeTile) void linst_gy2_kernel(LinstHeadArgs a) {
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    float y[K] = {};
    gather_sum<K>(a.b, a.GZd, beg, end, live, y);
    if (live) store_row<K>(a.GY2, r, y);
}

template <int K, bool SOFT>
int linst_head_launch(const LinstHeadArgs &a, hipStream_t st) {
    const dim3 grid(a.b.B, (a.b.n_max + kLargeTile - 1) / kLargeTile), block(kLargeTile);   // y <= 4096 at 2^20 nodes
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(linst_prob_kernel<K>, grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL((linst_loss_kernel<K, SOFT>), grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(linst_fold_kernel<K>, dim3(a.b.B), dim3(GMC_WAVE), 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    if (!a.GZd) return GMC_OK;
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(linst_gy2_kernel<K>, grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

int gmc_inst_large_hw2_launch(const gmc_batch *b, float *H, long ld, const float *b1, const float *W2, float *Z0, int F,
                              int K, hipStream_t st) {
    if (b->B == 0) return GMC_OK;
    if (b->n_max > GMC_LARGE_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    LinstHw2Args a{b->goff, H, b->dinv, b1, W2, Z0, F, ld};
    const int tiles = (b->n_max + kHw2Rows - 1) / kHw2Rows;
    const dim3 grid(b->B, tiles < kMaxGridY ? tiles : kMaxGridY);
    GmcProbeScope probe(GMC_K_DENSE_MFMA, st);   // the tag of hw2_k in the K-class sequence
    GMC_KWAY_DISPATCH(K, hipLaunchKernelGGL(linst_hw2_kernel<KK>, grid, dim3(256), 0, st, a));
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// GZd == nullptr: forward only (P, S, loss)
int gmc_inst_large_head_launch(const gmc_batch *b, const float *Z0, const float *b2, float C, int K, int loss_kind,
                               int terminals, float *P, int32_t *S, float *loss, int32_t *Sw, float *GZd, float *headpart,
                               float *GY2, float *db2, hipStream_t st) {
    if (!b || !Z0 || !b2 || !P || !Sw || !headpart || (GZd && (!GY2 || !db2))) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (b->n_max > GMC_LARGE_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (b->B == 0) return GMC_OK;
    LinstHeadArgs a{*b, Z0, b2, C, terminals, P, S, Sw, loss, GZd, headpart, GY2, db2};
    const bool soft = loss_kind == GMC_LOSS_EXPECTED_CUT;
    GMC_KWAY_DISPATCH(K, return soft ? linst_head_launch<KK, true>(a, st) : linst_head_launch<KK, false>(a, st));
    return GMC_OK;
}
