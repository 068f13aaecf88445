// Tabu search under class-size bounds at K = 2..8 classes (an extension): gmc_kway_balance_f32, stated to the operation
// in include/gcnmaxcut.h.  It is gmc_kway_tabu_f32's chain (kway_tabu.hip: one WAVE per chain, W / until / state /
// snapshot in LDS, 4, 2 or 1 chains of one graph per 256-thread workgroup over one staged copy of the CSR or the
// batch's arrays, the 64-bit key scan, the max butterfly on the VALU, one lane per edge applying a move, the deferred
// snapshot copy, the scoring tail and the pick) with three additions:
//
//   - the class sizes s[c] (every node) and m[c] (movable nodes) and the bounds lo[c], hi[c]: wave-uniform integers,
//     selected by compares as gmc::Sums<K> is, so they stay in scalar registers and the chain's LDS stays at tabu's
//     n_pad * (4 K + 6) bytes;
//   - which moves a -> b a node of class a may make is a property of (a, b) alone, so it is worked out once per change
//     of the sizes as K rows of K bits (a byte per class in one 64-bit word) and the scan only shifts and masks:
//     `open` for a node that is not banned (free moves, and paired ones into a class with a movable node), `free_` for
//     a banned one (aspiration belongs to free moves only).  A node still enters the scan with ONE key, its best move
//     among the targets of its row: for a banned node rel + gain is monotone in the gain, as in tabu;
//   - the same scan serves the repair (rows: the moves that lower the violation; no bans, rank = v - first) and the
//     counter-move of a paired move (one row with one bit: class b -> a; no bans; the node just moved left out).
//
// A paired move changes no size, so the rows are rebuilt after free moves and repair moves only.  With lo = 0 and
// hi = n every row is "every other class", nothing is repaired and the arithmetic is tabu's, step for step.
// The snapshot copy stays deferred; a paired move does not know whether it improves before its counter-move is chosen,
// so a pending copy is made ahead of every paired move - the state then IS the best state, so the bytes are the same.
//
// gmc_kway_balance_c_f32 is the same search on cut minus per-node class costs: balance_cost_kernel<K>, the same body
// text (balance_kernel_body.inc) with the table started from the node's cost row - the repair's gains come from it
// too - and the snapshots scored by gmc::block_score.
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"
#include "tabu_body.h"

namespace {

using gmc::mix64;
using gmc::u64;
using gmc::GlobalCsr;
using gmc::LdsCsr;
using gmc::TabuLayout;
using gmc::tabu_layout;
using gmc::wave_sync;
using gmc::wave_max;
using gmc::ordered_bits;
using gmc::ordered_float;

struct BalanceArgs {
    gmc_batch b;
    int first;               // first movable local id: K with terminals, 0 without
    int cands, iterations;
    unsigned tenure_base, tenure_span, tenure_div;
    u64 seed;
    signed char *assign;     // [cands][R], in/out
    const int *size_lo;      // [B][K]
    const int *size_hi;      // [B][K]
    float *cut_all;          // [B][cands]
    int *best_iter;          // [B][cands] or NULL
    int *moves;              // [B][cands] or NULL
    int *repairs;            // [B][cands] or NULL
    int slots, staged, n_pad, chain_bytes, off_starts, off_vals, off_ids;
};

// the sizes and their bounds: wave-uniform, every index a constant once the loops are unrolled
// (s and m share a word, s in the low half and m in the high half - both are at most GMC_MAX_GRAPH_NODES = 4096 - and so do
// lo and hi, clamped to 0..n, which changes no compare against a size in 0..n; with four words a class the K = 7
// instantiation spilled 20 bytes of scratch)
template <int K>
struct Sizes {
    unsigned sm[K], lh[K];
    __device__ __forceinline__ int s(int k) const { return (int)(sm[k] & 0xffffu); }
    __device__ __forceinline__ int m(int k) const { return (int)(sm[k] >> 16); }
    __device__ __forceinline__ int lo(int k) const { return (int)(lh[k] & 0xffffu); }
    __device__ __forceinline__ int hi(int k) const { return (int)(lh[k] >> 16); }
};

// "the bounds admit a partition" of include/gcnmaxcut.h for a graph of n nodes; t = 1 under terminals
template <int K>
__device__ __forceinline__ bool bounds_admit(const int *lo, const int *hi, int n, int t) {
    bool ok = true;
    long long need = 0, room = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int l = lo[k], h = hi[k];
        ok = ok && l <= h && h >= t;
        need += l > t ? l : t;
        room += h;
    }
    return ok && need <= (long long)n && (long long)n <= room;
}

template <int K>
__device__ __forceinline__ int violation(const Sizes<K> &z) {
    int V = 0;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        V += z.lo(k) > z.s(k) ? z.lo(k) - z.s(k) : 0;
        V += z.s(k) > z.hi(k) ? z.s(k) - z.hi(k) : 0;
    }
    return V;
}

// one movable node leaves class a for class b (wave-uniform a, b)
template <int K>
__device__ __forceinline__ void resize(Sizes<K> &z, int a, int b) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const int d = (k == b ? 1 : 0) - (k == a ? 1 : 0);
        z.sm[k] += (unsigned)(d * 0x10001);   // (s and m are at least 1 where one is taken: no borrow between the halves)
    }
}

// rows of the search: bit (a * 8 + b) of free_ - the move a -> b is free; of open - it is free, or paired with a
// movable node in b to come back
template <int K>
__device__ __forceinline__ void search_rows(const Sizes<K> &z, u64 &open, u64 &free_) {
    open = 0;
    free_ = 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
#pragma unroll
        for (int b = 0; b < K; ++b) {
            if (a == b) continue;
            const bool fr = z.s(a) > z.lo(a) && z.s(b) < z.hi(b);
            const u64 bit = 1ULL << (a * 8 + b);
            free_ |= fr ? bit : 0ULL;
            open |= fr || z.m(b) >= 1 ? bit : 0ULL;
        }
    }
}

// rows of the repair: bit (a * 8 + b) - the move a -> b lowers the violation
template <int K>
__device__ __forceinline__ u64 repair_rows(const Sizes<K> &z) {
    u64 rows = 0;
#pragma unroll
    for (int a = 0; a < K; ++a) {
        const int da = z.s(a) > z.hi(a) ? -1 : z.s(a) <= z.lo(a) ? 1 : 0;
#pragma unroll
        for (int b = 0; b < K; ++b) {
            if (a == b) continue;
            const int db = z.s(b) < z.lo(b) ? -1 : z.s(b) >= z.hi(b) ? 1 : 0;
            rows |= da + db < 0 ? 1ULL << (a * 8 + b) : 0ULL;
        }
    }
    return rows;
}

// The chain's views of its LDS and its graph, and the two steps every kind of move shares.
template <int K, class G>
struct Chain {
    const G &g;
    float *W;
    unsigned *until;
    unsigned char *st;
    int first, n, n_mov, trips, lane;

    // The wave's best move as one 64-bit key (0: none) - the gain mapped to an order-preserving uint32 in the high
    // half, ~(rank * K + k) in the low half - over the movable nodes other than `skip`: a node of class c whose ban
    // has run out by `now` takes its targets from row c of `open`, a banned one from row c of `free_` and only when
    // rel + gain > best.  A wave-uniform trip count and unconditional loads from a clamped node, unrolled by two, as
    // in tabu: a lane past its last node reads node `first` and admits nothing.
    __device__ __forceinline__ u64 scan(u64 open, u64 free_, unsigned now, int r, int skip, float rel,
                                        float best) const {
        u64 key = 0;
#pragma unroll 2
        for (int t = 0; t < trips; ++t) {
            const int v0 = first + lane + (t << 6);
            const bool valid = v0 < n;
            const int v = valid ? v0 : first;
            const unsigned c = st[v];
            float w[K];
#pragma unroll
            for (int k = 0; k < K; ++k) w[k] = W[v * K + k];
            float wc = w[0];
#pragma unroll
            for (int j = 1; j < K; ++j) wc = c == (unsigned)j ? w[j] : wc;
            const bool is_free = until[v] <= now;
            const unsigned row = (unsigned)((is_free ? open : free_) >> ((c & 7u) << 3)) & 0xffu;
            int rank = v - first - r;
            rank = rank < 0 ? rank + n_mov : rank;
            // the node's own best move among its row's targets - the largest gain, the smallest k on ties
            float bg = -__builtin_inff();
            int bk = 0;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float gain = wc - w[k];
                const bool take = ((row >> k) & 1u) != 0u && gain > bg;
                bg = take ? gain : bg;
                bk = take ? k : bk;
            }
            // (a byte of no class: the node never moves)
            const bool adm = valid && v0 != skip && c < (unsigned)K && row != 0u && (is_free || rel + bg > best);
            const u64 cnd = ((u64)ordered_bits(bg) << 32) | (u64)(~(unsigned)(rank * K + bk));
            key = adm && cnd > key ? cnd : key;
        }
        return wave_max(key);
    }

    // step 4 of tabu: node v leaves class c for class k
    __device__ __forceinline__ void apply(int v, int c, int k) const { gmc::apply_move<K>(g, W, st, v, c, k, lane); }
};

// workgroup-uniform: the graph has a size the launch takes and bounds that admit a partition
template <int K>
__device__ __forceinline__ bool graph_runs(const gmc_batch &b, int first, int gi, const int *size_lo,
                                           const int *size_hi, int &n, bool &admitted) {
    n = b.goff[gi + 1] - b.goff[gi];
    admitted = false;
    if (n > b.n_max || n < (first > 1 ? first : 1)) return false;   // (the LDS is sized by n_max)
    admitted = bounds_admit<K>(size_lo + (long)gi * K, size_hi + (long)gi * K, n, first > 0 ? 1 : 0);
    return admitted;
}

// gmc_kway_balance_c_f32's launch: BalanceArgs' fields and the cost.  A struct of its own, so that BalanceArgs keeps its
// layout (balance_kernel<K>'s register allocation moves with it: DESIGN.md section 34).
struct BalanceCostArgs {
    gmc_batch b;
    int first;
    int cands, iterations;
    unsigned tenure_base, tenure_span, tenure_div;
    u64 seed;
    signed char *assign;
    const int *size_lo;
    const int *size_hi;
    float *cut_all;
    int *best_iter;
    int *moves;
    int *repairs;
    int slots, staged, n_pad, chain_bytes, off_starts, off_vals, off_ids;
    const float *node_cost;  // [R][K] by batch row (read from global memory)
};

// Two kernels over one body text (balance_kernel_body.inc, which says why): balance_kernel<K> is the launch without
// costs, balance_cost_kernel<K> the one with them.
#define GMC_COST false
#define GMC_CHAIN_ARGS BalanceArgs
#define GMC_CHAIN_KERNEL balance_kernel
#include "balance_kernel_body.inc"
#undef GMC_COST
#undef GMC_CHAIN_ARGS
#undef GMC_CHAIN_KERNEL

#define GMC_COST true
#define GMC_CHAIN_ARGS BalanceCostArgs
#define GMC_CHAIN_KERNEL balance_cost_kernel
#include "balance_kernel_body.inc"
#undef GMC_COST
#undef GMC_CHAIN_ARGS
#undef GMC_CHAIN_KERNEL

struct BalancePickArgs {
    gmc::PickArgs p;
    int first;
    const int *size_lo, *size_hi;
    int *feasible;   // [B] or NULL
};
template <int K>
__global__ __launch_bounds__(256) void balance_pick_kernel(BalancePickArgs a) {
    const int g = blockIdx.x;
    int n;
    bool admitted;
    const bool runs = graph_runs<K>(a.p.b, a.first, g, a.size_lo, a.size_hi, n, admitted);
    if (n > a.p.b.n_max || n < (a.first > 1 ? a.first : 1)) return;   // workgroup-uniform: a graph of the wrong size
    if (a.feasible && threadIdx.x == 0) a.feasible[g] = admitted ? 1 : 0;
    if (!runs) return;                                                // workgroup-uniform: the graphs the chains skipped
    gmc::pick_best(a.p);
}

template <int K>
int balance_launch(const BalanceArgs &a, const BalancePickArgs &p, int lds_bytes, hipStream_t st) {
    const int rc = gmc::chain_launch(balance_kernel<K>, a, lds_bytes, st);
    if (rc != GMC_OK) return rc;
    hipLaunchKernelGGL((balance_pick_kernel<K>), dim3(a.b.B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

template <int K>
int balance_cost_launch(const BalanceCostArgs &a, const BalancePickArgs &p, int lds_bytes, hipStream_t st) {
    const int rc = gmc::chain_launch(balance_cost_kernel<K>, a, lds_bytes, st);
    if (rc != GMC_OK) return rc;
    hipLaunchKernelGGL((balance_pick_kernel<K>), dim3(a.b.B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

extern "C" int gmc_kway_balance_fits(const gmc_batch *batch, int32_t K) {
    return gmc::chain_query(batch, K, false);
}

extern "C" int gmc_kway_balance_shape(const gmc_batch *batch, int32_t K) {
    return gmc::chain_query(batch, K, true);
}

extern "C" int gmc_kway_balance_f32(const gmc_batch *batch, int32_t K, int32_t terminals, int32_t cands, int8_t *assign,
                                    const int32_t *size_lo, const int32_t *size_hi, int32_t iterations,
                                    int32_t tenure_base, int32_t tenure_span, int32_t tenure_div, uint64_t seed,
                                    float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_idx,
                                    int32_t *best_iter, int32_t *moves, int32_t *repairs, int32_t *feasible,
                                    gmc_stream_t stream) {
    if (!batch || !assign || !size_lo || !size_hi || !cut_all || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    int first;
    TabuLayout L;
    int rc = gmc::chain_checks(batch, K, terminals, cands, iterations, tenure_base, tenure_span, tenure_div, first,
                               L);
    if (rc != GMC_OK || batch->B == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BalanceArgs a{*batch, first, cands, iterations, (unsigned)tenure_base, (unsigned)tenure_span,
                        (unsigned)tenure_div, seed, reinterpret_cast<signed char *>(assign), size_lo, size_hi, cut_all,
                        best_iter, moves, repairs, L.slots, L.staged, L.n_pad, L.chain_bytes, L.off_starts, L.off_vals,
                        L.off_ids};
    const BalancePickArgs p{{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign,
                             best_cut, best_idx}, first, size_lo, size_hi, feasible};
    GMC_KWAY_DISPATCH(K, rc = balance_launch<KK>(a, p, L.bytes, st));
    return rc;
}

extern "C" int gmc_kway_balance_c_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const float *node_cost,
                                      int32_t cands, int8_t *assign, const int32_t *size_lo, const int32_t *size_hi,
                                      int32_t iterations, int32_t tenure_base, int32_t tenure_span, int32_t tenure_div,
                                      uint64_t seed, float *cut_all, int32_t *best_assign, float *best_cut,
                                      int32_t *best_idx, int32_t *best_iter, int32_t *moves, int32_t *repairs,
                                      int32_t *feasible, gmc_stream_t stream) {
    if (!node_cost)   // the launch without costs: the twin, kernel for kernel
        return gmc_kway_balance_f32(batch, K, terminals, cands, assign, size_lo, size_hi, iterations, tenure_base,
                                    tenure_span, tenure_div, seed, cut_all, best_assign, best_cut, best_idx, best_iter,
                                    moves, repairs, feasible, stream);
    if (!batch || !assign || !size_lo || !size_hi || !cut_all || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    int first;
    TabuLayout L;
    int rc = gmc::chain_checks(batch, K, terminals, cands, iterations, tenure_base, tenure_span, tenure_div, first,
                               L);
    if (rc != GMC_OK || batch->B == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const BalanceCostArgs a{*batch, first, cands, iterations, (unsigned)tenure_base, (unsigned)tenure_span,
                            (unsigned)tenure_div, seed, reinterpret_cast<signed char *>(assign), size_lo, size_hi,
                            cut_all, best_iter, moves, repairs, L.slots, L.staged, L.n_pad, L.chain_bytes, L.off_starts,
                            L.off_vals, L.off_ids, node_cost};
    const BalancePickArgs p{{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign,
                             best_cut, best_idx}, first, size_lo, size_hi, feasible};
    GMC_KWAY_DISPATCH(K, rc = balance_cost_launch<KK>(a, p, L.bytes, st));
    return rc;
}
