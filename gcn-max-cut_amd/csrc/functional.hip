// The kernels of the functional form of the model (gmc_fn_*): what the row-kernel sequence of gmc_kway_* / gmc_large_*
// lacks when the loss is the caller's - the probabilities without a decode, the softmax backward of a caller's dLoss/dP,
// and the two losses alone for K columns.  All are row-parallel launches on the grid of large.hip: (graph, tile of
// kLargeTile = 256 rows of the graph), several workgroups per graph, no LDS state per graph, so a graph may have up to
// GMC_LARGE_MAX_GRAPH_NODES nodes.  Kernel boundaries are the only synchronisation between workgroups: no spin waits, no
// arrival counters, no float atomics.
//   fn_prob         z = sum_e Z0[gcol[e],:], Z = fmaf(z, dinv, b2), P = softmax(Z)              (large_prob's arithmetic)
//   fn_softmax_bwd  GZ = P o (GP - rowsum(GP o P)); dinv o GZ to GZd [R,K]; the tile's K sums of GZ to part[slot][K]
//   fn_gy2          GY2[r,:] = sum_e GZd[gcol[e],:]                                             (layout [R,K]: hidden_bwd_k's)
//   fn_loss         the row's cut term of GMC_LOSS_CUT / GMC_LOSS_EXPECTED_CUT from P alone, GP = C * sum_e w_e (...) when
//                   asked for; the tile's sum to part[slot]
//   fn_fold         per graph: its tiles' partials in ascending order; V = K sums to db2part[g,:], or the one cut sum as
//                   loss[g] = -C * cut / 2 (one system-scope store: `loss` may be pinned host memory)
//
// Summation orders (all fixed: bitwise reproducible; large.hip's, whose device functions these kernels call).  A row of at
// most 64 entries: its lane, CSR order.  A longer row: its wave, lane j takes entries j, j + 64, ..., then the butterfly of
// gmc::wave_sum.  A tile's sums: the wave butterfly over the tile's rows, then the four waves ascending (block_sum).  A
// graph's sums: its tiles ascending.  The K terms of a row (GP . P, the softmax denominator): k ascending.
// A graph's first tile starts at the graph's first row, tiles past a graph's end exit at once, and graph g's partials live
// in the slots goff[g] / 256 + g onwards: a graph's results do not depend on what else is in the batch.
#include "large_rows.h"

namespace {

struct FnArgs {
    gmc_batch b;
    const float *Z0;     // [R,K]            fn_prob
    const float *b2;
    float *P;            // [R,K]            fn_prob: out
    const float *Pin;    // [R,K]            fn_softmax_bwd, fn_loss
    const float *GPin;   // [R,K]            fn_softmax_bwd
    float *GZd;          // [R,K]            dinv o GZ
    float *GY2;          // [R,K]
    float *part;         // [slots][V]
    float *GP;           // [R,K] or nullptr fn_loss: out
    float C;
    int terminals;       // fn_loss: nodes 0..K-1 of every graph are fixed to classes 0..K-1
};

template <int K>
__global__ __launch_bounds__(kLargeTile) void fn_prob_kernel(FnArgs a) {
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    float z[K] = {};
    gather_sum<K>(a.b, a.Z0, beg, end, live, z);
    if (!live) return;
    const float d = a.b.dinv[r];
    float m = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) { z[k] = fmaf(z[k], d, a.b2[k]); m = fmaxf(m, z[k]); }
    float p[K], sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) { p[k] = expf(z[k] - m); sum += p[k]; }
    const float inv = 1.0f / sum;
#pragma unroll
    for (int k = 0; k < K; ++k) p[k] *= inv;
    store_row<K>(a.P, r, p);
}

template <int K>
__global__ __launch_bounds__(kLargeTile) void fn_softmax_bwd_kernel(FnArgs a) {
    __shared__ float red[kLargeWaves * K];
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    float acc[K] = {};
    if (live) {
        float p[K], gp[K];
        load_row<K>(a.Pin, r, p);
        load_row<K>(a.GPin, r, gp);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) dot += gp[k] * p[k];
        const float d = a.b.dinv[r];
        float gz[K];
#pragma unroll
        for (int k = 0; k < K; ++k) {
            acc[k] = p[k] * (gp[k] - dot);
            gz[k] = acc[k] * d;
        }
        store_row<K>(a.GZd, r, gz);
    }
    block_sum<K, kLargeWaves>(acc, red);
    if (threadIdx.x == 0) {
        float *out = a.part + part_slot(t) * K;
#pragma unroll
        for (int k = 0; k < K; ++k) out[k] = acc[k];
    }
}

template <int K>
__global__ __launch_bounds__(kLargeTile) void fn_gy2_kernel(FnArgs a) {
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    float y[K] = {};
    gather_sum<K>(a.b, a.GZd, beg, end, live, y);
    if (live) store_row<K>(a.GY2, r, y);
}

// the class of a row of P: the first maximum (torch.argmax)
template <int K>
__device__ __forceinline__ int first_max(const float (&p)[K]) {
    int s = 0;
    float best = p[0];
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (p[k] > best) { best = p[k]; s = k; }
    return s;
}

// Pt of a row: e_l for a terminal (local id l < terms), else - SOFT - its row of P, or - hard - the one-hot of its class
template <int K, bool SOFT>
__device__ __forceinline__ void pt_row(const float *P, int row, int local, int terms, float (&u)[K]) {
    int one = local;
    if (local >= terms) {
        load_row<K>(P, row, u);
        if constexpr (SOFT) return;
        one = first_max<K>(u);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) u[k] = k == one ? 1.f : 0.f;
}

template <int K, bool SOFT>
__global__ __launch_bounds__(kLargeTile) void fn_loss_kernel(FnArgs a) {
    __shared__ float red[kLargeWaves];
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    const int terms = a.terminals ? (t.n < K ? t.n : K) : 0;
    float u[K];   // Pt of this row (hard: the one-hot of its class)
    pt_row<K, SOFT>(a.Pin, r, t.l, terms, u);
    float v[K + 1] = {};   // gp[0..K-1], cut
    row_terms<K + 1, K>(beg, end, live, u, v, [&](int e, float (&acc)[K + 1], const float (&me)[K]) {
        const float w = a.b.vals ? a.b.vals[e] : 1.0f;
        float q[K];
        pt_row<K, SOFT>(a.Pin, a.b.gcol[e], a.b.lcol[e], terms, q);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { acc[k] += w * q[k]; dot += me[k] * q[k]; }
        // (hard: dot is exactly 0 or 1, the term exactly 0 or w - what large_loss adds for S_u != S_v)
        acc[K] += w * (1.0f - dot);
    });
    if (live && a.GP) {
        float gp[K];
#pragma unroll
        for (int k = 0; k < K; ++k) gp[k] = v[k] * a.C;
        store_row<K>(a.GP, r, gp);
    }
    float cut[1] = {live ? v[K] : 0.f};
    block_sum<1, kLargeWaves>(cut, red);
    if (threadIdx.x == 0) a.part[part_slot(t)] = cut[0];
}

// one workgroup (a wave) per graph; lane k < V folds sum k of the graph's tiles.  loss != nullptr (V = 1): the sum is the
// graph's cut counted from both ends
__global__ __launch_bounds__(GMC_WAVE) void fn_fold_kernel(const int *goff, const float *part, int V, float *out, float C,
                                                           float *loss) {
    const int g = blockIdx.x, k = threadIdx.x;
    if (k >= V) return;
    const int r0 = goff[g], n = goff[g + 1] - r0;
    const int tiles = (n + kLargeTile - 1) / kLargeTile;
    const float *p = part + ((long)(r0 / kLargeTile) + g) * V + k;
    float s = 0.f;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) s += p[(long)t * V];
    if (loss) {
        // one system-scope store: `loss` may be pinned host memory the caller watches
        __hip_atomic_store(loss + g, -C * (s * 0.5f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    } else {
        out[(long)g * V + k] = s;
    }
}

dim3 tile_grid(const gmc_batch &b) { return dim3(b.B, (b.n_max + kLargeTile - 1) / kLargeTile); }

template <int K>
int softmax_bwd_launch(const FnArgs &a, float *db2part, hipStream_t st) {
    const dim3 grid = tile_grid(a.b), block(kLargeTile);
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(fn_softmax_bwd_kernel<K>, grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(fn_fold_kernel, dim3(a.b.B), dim3(GMC_WAVE), 0, st, a.b.goff, a.part, K, db2part, 0.f, nullptr);
    }
    GMC_LAUNCH_CHECK();
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(fn_gy2_kernel<K>, grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

template <int K, bool SOFT>
int loss_launch(const FnArgs &a, float *loss, hipStream_t st) {
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL((fn_loss_kernel<K, SOFT>), tile_grid(a.b), dim3(kLargeTile), 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(fn_fold_kernel, dim3(a.b.B), dim3(GMC_WAVE), 0, st, a.b.goff, a.part, 1, nullptr, a.C, loss);
    }
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

size_t gmc_fn_part_floats(const gmc_batch *b, int V) {
    return ((size_t)b->R / kLargeTile + (size_t)b->B + 1) * (size_t)V;
}

int gmc_fn_prob_launch(const gmc_batch *b, const float *Z0, const float *b2, int K, float *P, hipStream_t st) {
    if (!b || !Z0 || !b2 || !P) return GMC_ERR_NULL;
    if (b->n_max > GMC_LARGE_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (b->B == 0) return GMC_OK;
    FnArgs a{};
    a.b = *b; a.Z0 = Z0; a.b2 = b2; a.P = P;
    GmcProbeScope probe(GMC_K_HEAD, st);
    GMC_KWAY_DISPATCH(K, hipLaunchKernelGGL(fn_prob_kernel<KK>, tile_grid(a.b), dim3(kLargeTile), 0, st, a));
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

int gmc_fn_softmax_bwd_launch(const gmc_batch *b, const float *P, const float *GP, int K, float *GZd, float *part,
                              float *db2part, float *GY2, hipStream_t st) {
    if (!b || !P || !GP || !GZd || !part || !db2part || !GY2) return GMC_ERR_NULL;
    if (b->n_max > GMC_LARGE_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (b->B == 0) return GMC_OK;
    FnArgs a{};
    a.b = *b; a.Pin = P; a.GPin = GP; a.GZd = GZd; a.part = part; a.GY2 = GY2;
    GMC_KWAY_DISPATCH(K, return softmax_bwd_launch<KK>(a, db2part, st));
    return GMC_OK;
}

int gmc_fn_loss_launch(const gmc_batch *b, const float *P, int K, int terminals, float C, int loss_kind, float *part,
                       float *loss, float *GP, hipStream_t st) {
    if (!b || !P || !part || !loss) return GMC_ERR_NULL;
    if (b->n_max > GMC_LARGE_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (b->B == 0) return GMC_OK;
    FnArgs a{};
    a.b = *b; a.Pin = P; a.part = part; a.GP = GP; a.C = C; a.terminals = terminals;
    const bool soft = loss_kind == GMC_LOSS_EXPECTED_CUT;
    GMC_KWAY_DISPATCH(K, return soft ? loss_launch<KK, true>(a, loss, st) : loss_launch<KK, false>(a, loss, st));
    return GMC_OK;
}
