// The head of the K-class step for graphs that do not fit a CU's LDS (gmc_large_*: up to GMC_LARGE_MAX_GRAPH_NODES
// nodes): head_k_kernel of kway.hip as row-parallel launches that several workgroups share per graph.
//
// Every row does the per-row arithmetic of head_k_kernel; what that kernel reads from LDS by local node id these kernels
// read from global memory by batch row id (gcol).  Kernel boundaries are the only synchronisation between workgroups: no
// spin waits, no arrival counters, no float atomics.
//   large_prob   z = sum_e Z0[gcol[e],:], Z = fmaf(z, dinv, b2), P = softmax(Z), S = l for local rows l < K else the first
//                maximum; S goes to a workspace array (and to the caller's S when given)
//   large_loss   hard: the neighbours' classes from the S array; relaxed: the neighbour's Pt row is e_c for lcol[e] < K, else
//                P[gcol[e],:].  The row's cut term and GP = C * sum w ...; training: GZ = P o (GP - GP.P), dinv o GZ to a
//                workspace array [R,K].  The tile's K + 1 sums (cut, db2) go to headpart[slot][K+1]
//   large_fold   per graph: its tiles' partials in ascending order; loss[g] = -C * cut / 2 (one system-scope store: `loss`
//                may be pinned host memory), db2part[g,:]
//   large_gy2    training: GY2[r,:] = sum_e (dinv o GZ)[gcol[e],:]                      (layout [R,K]: hidden_bwd_k's)
//
// Grid: (graph, tile of kLargeTile = 256 rows within the graph).  A graph's first tile starts at the graph's first row and
// tiles past a graph's end exit at once, so a graph's results do not depend on what else is in the batch.
//
// Summation orders (all fixed: bitwise reproducible).
//   * A row of at most kLargeWaveRow = 64 entries is summed by its own lane in CSR order, as head_k_kernel does.
//   * A longer row (a hub) is taken by its wave: lane j adds entries j, j + 64, j + 128, ... of the row in that order, then
//     the 64 partials are added by the butterfly of gmc::wave_sum (lane distances 32, 16, 8, 4, 2, 1), as att_fwd does.
//   * A tile's K + 1 sums: block_sum's order - the wave butterfly over the tile's rows (one row per lane), then the four
//     waves ascending.  A graph's sums: its tiles ascending.  (head_k_kernel deals a graph's rows over 1024 / 512 threads
//     instead: the two heads agree to rounding, not to the bit.)
// The partials of graph g live in the slots goff[g] / 256 + g onwards (ceil(n_g / 256) of them): disjoint for any sizes,
// known on the device without a prefix sum over the graphs, R / 256 + B + 1 slots in all.
#include "large_rows.h"

namespace {

struct LargeArgs {
    gmc_batch b;
    const float *Z0;   // [R,K]
    const float *b2;
    float C;
    float *P;          // [R,K]
    int *S;            // caller's, optional
    int *Sw;           // [R] workspace
    float *loss;
    float *GZd;        // [R,K] dinv o GZ; nullptr: forward only
    float *headpart;   // [slots][K+1]
    float *GY2;        // [R,K]
    float *db2part;    // [B,K]
};

template <int K>
__global__ __launch_bounds__(kLargeTile) void large_prob_kernel(LargeArgs a) {
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    float z[K] = {};
    gather_sum<K>(a.b, a.Z0, beg, end, live, z);
    if (!live) return;
    const int terms = t.n < K ? t.n : K;
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
__global__ __launch_bounds__(kLargeTile) void large_loss_kernel(LargeArgs a) {
    __shared__ float red[kLargeWaves * (K + 1)];
    const Tile t = my_tile(a.b);
    if ((int)blockIdx.y * kLargeTile >= t.n) return;   // (workgroup-uniform)
    const bool live = t.l < t.n;
    const int r = t.r0 + (live ? t.l : 0);
    const int beg = a.b.rowptr[r], end = a.b.rowptr[r + 1];
    const int terms = t.n < K ? t.n : K;
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
            if (lc < K) {   // a terminal (lcol < K <= n, or lcol < n < K): e_lcol
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
__global__ __launch_bounds__(GMC_WAVE) void large_fold_kernel(LargeArgs a) {
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
        a.db2part[(long)g * K + (k - 1)] = s;
    }
}

template <int K>
__global__ __launch_bounds__(kLargeTile) void large_gy2_kernel(LargeArgs a) {
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
int large_head_launch(const LargeArgs &a, hipStream_t st) {
    const dim3 grid(a.b.B, (a.b.n_max + kLargeTile - 1) / kLargeTile), block(kLargeTile);
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(large_prob_kernel<K>, grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL((large_loss_kernel<K, SOFT>), grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(large_fold_kernel<K>, dim3(a.b.B), dim3(GMC_WAVE), 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    if (!a.GZd) return GMC_OK;
    {
        GmcProbeScope probe(GMC_K_HEAD, st);
        hipLaunchKernelGGL(large_gy2_kernel<K>, grid, block, 0, st, a);
    }
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// ---- rows of more than kLargeWaveRow entries of an F-wide aggregation, once more (launchers.h: gmc_large_hub_rows_launch)
struct HubRowsArgs {
    const int *rowptr, *col;
    const float *vals, *scale, *X;
    long ldx;
    const float *bias;
    int relu;
    float *Y;
    long ldy;
    int n_rows, F4;
};

// one wave per row, lane = float4 column (+ 64 per pass); a row of at most kLargeWaveRow entries is left alone
template <bool HAS_VAL>
__global__ __launch_bounds__(256) void large_hub_rows_kernel(HubRowsArgs a) {
    const int lane = gmc::lane_id();
    const int r = gmc::uniform((int)(blockIdx.x * 4 + (threadIdx.x >> 6)));
    if (r >= a.n_rows) return;
    const int beg = a.rowptr[r], end = a.rowptr[r + 1];
    if (end - beg <= kLargeWaveRow) return;
    const float s = a.scale ? a.scale[r] : 1.0f;
    for (int c = lane; c < a.F4; c += GMC_WAVE) {
        float4 acc = gmc::f4_zero();
        for (int e0 = beg; e0 < end; e0 += kLargeWaveRow) {   // (the first chunk: acc = 0 + its sum, exactly its sum)
            const int cnt = min(kLargeWaveRow, end - e0);
            float4 part = gmc::f4_zero();
            for (int j = 0; j < cnt; ++j) {
                const float4 x = reinterpret_cast<const float4 *>(a.X + (long)a.col[e0 + j] * a.ldx)[c];
                if (HAS_VAL) gmc::f4_fma(part, a.vals[e0 + j], x);
                else gmc::f4_add(part, x);
            }
            gmc::f4_add(acc, part);
        }
        const float4 bias = a.bias ? reinterpret_cast<const float4 *>(a.bias)[c] : gmc::f4_zero();
        float4 y;
        y.x = fmaf(acc.x, s, bias.x); y.y = fmaf(acc.y, s, bias.y); y.z = fmaf(acc.z, s, bias.z); y.w = fmaf(acc.w, s, bias.w);
        if (a.relu) {
            y.x = y.x > 0.f ? y.x : 0.f; y.y = y.y > 0.f ? y.y : 0.f;
            y.z = y.z > 0.f ? y.z : 0.f; y.w = y.w > 0.f ? y.w : 0.f;
        }
        reinterpret_cast<float4 *>(a.Y + (long)r * a.ldy)[c] = y;
    }
}

}  // namespace

int gmc_large_hub_rows_launch(const int32_t *rowptr, const int32_t *col, const float *vals, const float *scale,
                              const float *X, long ldx, const float *bias, int relu, float *Y, long ldy, int32_t n_rows,
                              int32_t F, int tag, hipStream_t st) {
    if (!rowptr || !col || !X || !Y) return GMC_ERR_NULL;
    if (F % 4 || ldx % 4 || ldy % 4 || !gmc_aligned16(X) || !gmc_aligned16(Y) || (bias && !gmc_aligned16(bias)))
        return GMC_ERR_ALIGN;
    if (n_rows <= 0) return GMC_OK;
    HubRowsArgs a{rowptr, col, vals, scale, X, ldx, bias, relu, Y, ldy, n_rows, F / 4};
    const dim3 grid((unsigned)((n_rows + 3) / 4));
    GmcProbeScope probe(tag, st);
    if (vals) hipLaunchKernelGGL(large_hub_rows_kernel<true>, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(large_hub_rows_kernel<false>, grid, dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

size_t gmc_large_headpart_floats(const gmc_batch *b, int K) {
    return ((size_t)b->R / kLargeTile + (size_t)b->B + 1) * (size_t)(K + 1);
}

// GZd == nullptr: forward only (P, S, loss)
int gmc_large_head_launch(const gmc_batch *b, const float *Z0, const float *b2, float C, int K, int loss_kind, float *P,
                          int32_t *S, float *loss, int32_t *Sw, float *GZd, float *headpart, float *GY2, float *db2part,
                          hipStream_t st) {
    if (!b || !Z0 || !b2 || !P || !Sw || !headpart || (GZd && (!GY2 || !db2part))) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (b->n_max > GMC_LARGE_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (b->B == 0) return GMC_OK;
    LargeArgs a{*b, Z0, b2, C, P, S, Sw, loss, GZd, headpart, GY2, db2part};
    const bool soft = loss_kind == GMC_LOSS_EXPECTED_CUT;
    GMC_KWAY_DISPATCH(K, return soft ? large_head_launch<KK, true>(a, st) : large_head_launch<KK, false>(a, st));
    return GMC_OK;
}
