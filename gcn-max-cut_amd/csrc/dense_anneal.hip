// Annealing of dense two-class instances on cached local fields (an extension: the reference samples and stops):
// gmc_dense_anneal_f32, stated to the operation in include/gcnmaxcut_dense.h.  The sparse decoders recompute a node's
// class sums from its CSR row on every visit; on a dense matrix that is n dependent loads per visit and a colouring with
// one node per colour.  Here a chain keeps ONE number per node, F[v] = W_1(v) - W_0(v): a visit reads F[v] and the class
// byte, and only an accepted move pays O(n) - one coalesced read of row v of W, 2 W[v][u] added to or taken from F[u].
//
// One WAVE per chain (candidate, problem), four chains of one problem per 256-thread workgroup, as kway_tabu.hip: the
// sweeps hold no workgroup barrier (the only one publishes the level table).  A chain's state is private to its wave,
// in LDS:
//
//   F      [n_pad] float   the fields, kept up to date move by move          (n_pad = n up to 16)
//   state  [n_pad] byte    the classes as they stand
//   snap   [n_pad] byte    the state of the largest objective so far
//
// 6 n_pad bytes per chain beside one copy of the level table (4 KB): 28 KB a workgroup at n = 1024, 100 KB at n = 4096.
// Lane j owns the entries j, j + 64, ... of F.
//
// A sweep walks the visit order in blocks of 64: lane k of a block loads the k-th node of the block and hashes ITS level
// (the 64-bit hash costs one lane-parallel evaluation per 64 visits), then the wave takes the visits one by one: node
// and level by v_readlane, F[v] and the class byte from one LDS address each (a broadcast), a wave-uniform decision.  A
// rejected visit - the large majority at low temperature - ends there.  An accepted one streams row v, eight loads per
// lane issued together, and updates the lane's own entries of F; the wave's own LDS traffic is ordered by tabu_body.h's
// wave_sync.
//
// The fields (step 1) and the score (step 2) read W by rows using the symmetry: lane j accumulates four of its own
// nodes v at a time and reads W[u][v] for u = 0, 1, ... - consecutive lanes read consecutive addresses, and every
// accumulator adds in ascending u, the order the header states.
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "tabu_body.h"   // wave_sync
#include "../../include/gcnmaxcut_dense.h"

#define GMC_DENSE_CHAINS 4      // chains (waves) per workgroup
#define GMC_DENSE_ROW_LOADS 8   // loads of a row a lane issues together

namespace {

using gmc::mix64;
using gmc::u64;
using gmc::wave_sync;

struct DenseArgs {
    int B, n, cands, anneal_sweeps, max_descent_sweeps, n_pad;
    long ld;
    const float *W;           // [B][n][ld]
    const float *node_cost;   // [B * n][2] or NULL
    const int *order;         // [B * n] local ids or NULL
    signed char *assign;      // [cands][B * n], in/out
    const float *inv_temp, *levels;
    u64 seed;
    float *score_all;         // [B][cands]
    int *snap_sweep, *sweeps; // [B][cands] or NULL
    long long *moves;         // [B][cands] or NULL
};

// Steps 1 and 2 of the header for the state S: with FIELDS the fields into F, with SCORE the score (every lane gets
// it; 0 without SCORE).  W: the problem's matrix, nc: its cost rows or NULL.
template <bool FIELDS, bool SCORE>
__device__ __forceinline__ float dense_pass(const float *W, long ld, const float *nc, int n, float *F,
                                            const unsigned char *S, int lane) {
#pragma clang fp contract(off)
    float cut = 0.f, cost = 0.f;
    for (int v0 = 0; v0 < n; v0 += 4 * GMC_WAVE) {
        int v[4], sv[4];
        bool live[4];
        float a0[4], a1[4], t[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            v[i] = v0 + GMC_WAVE * i + lane;
            live[i] = v[i] < n;
            sv[i] = live[i] ? S[v[i]] : 0;
            a0[i] = nc && live[i] ? nc[2 * v[i]] : 0.f;
            a1[i] = nc && live[i] ? nc[2 * v[i] + 1] : 0.f;
            t[i] = 0.f;
        }
#pragma unroll 2
        for (int u = 0; u < n; ++u) {
            const int su = S[u];   // one address for the wave: a broadcast
            const float *row = W + (long)u * ld;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const bool on = live[i] && v[i] != u;   // neither the diagonal nor a column >= n is read
                float w = 0.f;
                if (on) w = row[v[i]];                  // W[u][v] for W[v][u]
                if constexpr (FIELDS) {
                    a0[i] = on ? a0[i] + (su == 0 ? w : 0.f) : a0[i];
                    a1[i] = on ? a1[i] + (su == 1 ? w : 0.f) : a1[i];
                }
                if constexpr (SCORE) t[i] = on ? t[i] + (su != sv[i] ? w : 0.f) : t[i];
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!live[i]) continue;
            if constexpr (FIELDS) F[v[i]] = a1[i] - a0[i];
            if constexpr (SCORE) {
                cut += t[i];
                if (nc) cost += nc[2 * v[i] + sv[i]];
            }
        }
    }
    if constexpr (!SCORE) return 0.f;
    cut = gmc::wave_sum(cut) * 0.5f;
    if (!nc) return cut;
    return cut - gmc::wave_sum(cost);
}

// One sweep over the visit order on the chain's F and S.  ANNEAL: the Metropolis test of sweep `s` (base: the hash's
// part without the node); without it the descent's delta < 0.  Returns whether a node moved; obj and moves follow the
// accepted moves.
template <bool ANNEAL>
__device__ __forceinline__ int dense_sweep(const float *W, long ld, const int *ord, int n, float *F, unsigned char *S,
                                           const float *lv, float inv_t, u64 base, int lane, float &obj,
                                           long long &moves) {
#pragma clang fp contract(off)
    int moved = 0;
    auto node_of = [&](int i) {
        int v = -1;
        if (i < n) v = ord ? ord[i] : i;
        return (unsigned)v < (unsigned)n ? v : -1;
    };
    int next = node_of(lane);
    for (int i0 = 0; i0 < n; i0 += GMC_WAVE) {
        const int mine = next;
        next = node_of(i0 + GMC_WAVE + lane);   // the next block's nodes are in flight while this one is visited
        float level = 0.f;
        if constexpr (ANNEAL) level = lv[mix64(base + GMC_GOLD * (u64)(unsigned)mine) >> 54];
        const int count = n - i0 < GMC_WAVE ? n - i0 : GMC_WAVE;
        for (int k = 0; k < count; ++k) {
            const int v = __builtin_amdgcn_readlane(mine, k);
            if (v < 0) continue;   // wave-uniform
            const float f = F[v];  // one address for the wave: a broadcast
            const int c = S[v];
            const float delta = c == 0 ? f : -f;
            bool move = delta < 0.f;
            if constexpr (ANNEAL) {
                const float lvl = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(level), k));
                move = move || delta * inv_t <= lvl;
            }
            if (!__builtin_amdgcn_readfirstlane((int)move)) continue;   // every lane decided the same
            if (lane == 0) S[v] = (unsigned char)(1 - c);
            obj = obj - delta;
            moved = 1;
            if constexpr (ANNEAL) ++moves;
            const float *row = W + (long)v * ld;
            for (int u0 = 0; u0 < n; u0 += GMC_DENSE_ROW_LOADS * GMC_WAVE) {
                float w[GMC_DENSE_ROW_LOADS];
#pragma unroll
                for (int j = 0; j < GMC_DENSE_ROW_LOADS; ++j) {
                    const int u = u0 + GMC_WAVE * j + lane;
                    w[j] = 0.f;
                    if (u < n && u != v) w[j] = row[u];
                }
#pragma unroll
                for (int j = 0; j < GMC_DENSE_ROW_LOADS; ++j) {
                    const int u = u0 + GMC_WAVE * j + lane;
                    if (u < n && u != v) F[u] = F[u] + (c == 0 ? 2.0f * w[j] : -(2.0f * w[j]));
                }
            }
            wave_sync();   // the next visit reads the fields and the byte this one wrote
        }
    }
    return moved;
}

__global__ __launch_bounds__(256) void dense_chains_kernel(DenseArgs a) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    float *lv = reinterpret_cast<float *>(lds);
    if (a.anneal_sweeps > 0)
        for (int i = threadIdx.x; i < GMC_ANNEAL_LEVELS; i += blockDim.x) lv[i] = a.levels[i];
    __syncthreads();   // the launch's only workgroup barrier
    const int wave = gmc::uniform((int)(threadIdx.x >> 6)), lane = gmc::lane_id();
    const int cand = blockIdx.x * GMC_DENSE_CHAINS + wave, prob = blockIdx.y;
    if (cand >= a.cands) return;   // wave-uniform: the last workgroup of a problem
    const int n = a.n;
    unsigned char *chain = lds + 4 * GMC_ANNEAL_LEVELS + (long)wave * 6 * a.n_pad;
    float *F = reinterpret_cast<float *>(chain);
    unsigned char *S = chain + 4 * a.n_pad;
    unsigned char *snap = S + a.n_pad;
    const long r0 = (long)prob * n;
    const float *W = a.W + r0 * a.ld;
    const float *nc = a.node_cost ? a.node_cost + 2 * r0 : nullptr;
    const int *ord = a.order ? a.order + r0 : nullptr;
    signed char *st = a.assign + (long)cand * a.B * n + r0;
    const long own = (long)prob * a.cands + cand;

    for (int l = lane; l < n; l += GMC_WAVE) S[l] = snap[l] = (unsigned char)(st[l] & 1);
    wave_sync();

    int snap_sweep = 0;
    long long moves = 0, unused = 0;
    if (a.anneal_sweeps > 0) {
        float obj = dense_pass<true, true>(W, a.ld, nc, n, F, S, lane);
        float best_obj = obj;
        wave_sync();
        for (int s = 0; s < a.anneal_sweeps; ++s) {
            const float inv_t = a.inv_temp[s];
            // seed + GOLD * (ctr + 1), ctr = cand << 32 | s << 12 | v: the part without v (anneal_body.h's)
            const u64 base = a.seed + GMC_GOLD * ((((u64)(unsigned)cand << 32) | ((u64)(unsigned)s << 12)) + 1ULL);
            dense_sweep<true>(W, a.ld, ord, n, F, S, lv, inv_t, base, lane, obj, moves);
            if (obj > best_obj) {   // wave-uniform: every lane carries the same obj
                best_obj = obj;
                snap_sweep = s + 1;
                for (int l = lane; l < n; l += GMC_WAVE) snap[l] = S[l];
                wave_sync();
            }
        }
        for (int l = lane; l < n; l += GMC_WAVE) S[l] = snap[l];
        wave_sync();
    }
    dense_pass<true, false>(W, a.ld, nc, n, F, S, lane);   // the descent starts from fields without drift
    wave_sync();
    int sweeps = 0;
    float obj = 0.f;
    while (sweeps < a.max_descent_sweeps) {
        ++sweeps;
        if (!dense_sweep<false>(W, a.ld, ord, n, F, S, lv, 0.f, 0, lane, obj, unused)) break;
    }
    const float score = dense_pass<false, true>(W, a.ld, nc, n, F, S, lane);
    for (int l = lane; l < n; l += GMC_WAVE) st[l] = (signed char)S[l];
    if (lane == 0) {
        a.score_all[own] = score;
        if (a.snap_sweep) a.snap_sweep[own] = snap_sweep;
        if (a.sweeps) a.sweeps[own] = sweeps;
        if (a.moves) a.moves[own] = moves;
    }
}

struct DensePickArgs {
    int n, cands;
    long R;
    const signed char *assign;   // [cands][R]
    const float *score_all;      // [B][cands]
    int *best_assign;            // [R]
    float *best_score;           // [B]
    int *best_idx;               // [B]
};

// one workgroup per problem: the strictly best candidate, the first on ties, and its state
__global__ __launch_bounds__(256) void dense_pick_kernel(DensePickArgs a) {
    const int g = blockIdx.x;
    const int best = gmc::pick_best_index(a.score_all, a.cands, g, a.best_score, a.best_idx);
    const long r0 = (long)g * a.n;
    for (int l = threadIdx.x; l < a.n; l += blockDim.x) a.best_assign[r0 + l] = a.assign[(long)best * a.R + r0 + l];
}

bool dense_sizes_ok(int B, int n, int cands) { return B >= 0 && n >= 2 && n <= GMC_MAX_GRAPH_NODES && cands >= 1; }

}  // namespace

extern "C" size_t gmc_dense_anneal_workspace_bytes(int32_t B, int32_t n, int32_t cands) {
    return dense_sizes_ok(B, n, cands) ? GMC_DENSE_WORKSPACE_MIN : 0;
}

extern "C" int gmc_dense_anneal_f32(int32_t B, int32_t n, const float *W, int64_t ld, const float *node_cost,
                                    const int32_t *order, int32_t cands, int8_t *assign, const float *inv_temp,
                                    int32_t anneal_sweeps, const float *levels, uint64_t seed,
                                    int32_t max_descent_sweeps, void *workspace, size_t workspace_bytes, float *score_all,
                                    int32_t *best_assign, float *best_score, int32_t *best_idx, int32_t *snap_sweep,
                                    int32_t *sweeps, int64_t *moves, gmc_stream_t stream) {
    if (!W || !assign || !score_all || !best_assign || !best_score || !best_idx || !workspace) return GMC_ERR_NULL;
    if (B < 0 || cands < 1 || anneal_sweeps < 0 || max_descent_sweeps < 0) return GMC_ERR_SHAPE;
    if (anneal_sweeps > 0 && (!inv_temp || !levels)) return GMC_ERR_NULL;
    if (n < 2 || n > GMC_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (anneal_sweeps >= (1 << 20)) return GMC_ERR_SHAPE;
    if (ld < n) return GMC_ERR_SHAPE;
    if (workspace_bytes < gmc_dense_anneal_workspace_bytes(B, n, cands)) return GMC_ERR_WORKSPACE;
    if (B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int n_pad = (n + 15) & ~15;
    const int lds_bytes = 4 * GMC_ANNEAL_LEVELS + GMC_DENSE_CHAINS * 6 * n_pad;
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(dense_chains_kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    const DenseArgs a{B, n, cands, anneal_sweeps, max_descent_sweeps, n_pad, (long)ld, W, node_cost, order,
                      reinterpret_cast<signed char *>(assign), inv_temp, levels, seed, score_all, snap_sweep, sweeps,
                      reinterpret_cast<long long *>(moves)};
    {
        GmcProbeScope probe(GMC_K_ANNEAL, st);
        hipLaunchKernelGGL(dense_chains_kernel, dim3((cands + GMC_DENSE_CHAINS - 1) / GMC_DENSE_CHAINS, B), dim3(256),
                           (size_t)lds_bytes, st, a);
        GMC_LAUNCH_CHECK();
    }
    const DensePickArgs p{n, cands, (long)B * n, reinterpret_cast<const signed char *>(assign), score_all, best_assign,
                          best_score, best_idx};
    hipLaunchKernelGGL(dense_pick_kernel, dim3(B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
