// One-flip tabu search over decoded partitions at K = 2..8 classes (an extension: the reference samples and stops):
// gmc_kway_tabu_f32, stated to the operation in include/gcnmaxcut.h.  A chain is one (candidate, graph) pair; every
// iteration takes the best admissible single move, forbids moving that node again for a while and lets a move that
// would beat the best cut seen override the ban.
//
// One WAVE per chain, so the iteration loop holds no workgroup barrier: lane j owns the movable nodes first + j,
// first + j + 64, ...  The chain's state is private to its wave, in LDS:
//
//   W      [n_pad][K] float   the class sums of every node, kept up to date move by move   (n_pad = n_max up to 16)
//   until  [n_pad] uint32     the first iteration at which the node may move again
//   state  [n_pad] byte       the classes as they stand
//   snap   [n_pad] byte       the state of the largest cut so far
//
// n_pad * (4 K + 6) bytes per chain.  A 256-thread workgroup runs 4, 2 or 1 chains of ONE graph (tabu_layout: as many
// as fit), which share one staged copy of the graph's CSR in anneal_stage_csr's layout (starts, ids as uint16, vals);
// when the copy does not fit beside one chain, the chains read the batch's arrays in global memory - one template
// over LdsCsr / GlobalCsr (anneal_layout.h), so the arithmetic cannot differ.  The waves without a chain (slots < 4,
// or the last workgroup of a graph) wait at the closing barrier.
//
// An iteration: each lane scans its nodes (the W row, the class byte, until) for its best admissible move as ONE
// 64-bit key - the gain mapped to an order-preserving uint32 in the high half, ~(rank * K + k) in the low half; keys
// are unique, 0 means "none".  A node enters with its own best move only (the largest gain, the smallest k on ties: one
// subtraction and one compare per class, one key per node), and the scan has a wave-uniform trip count with
// unconditional loads, unrolled by two, so that the LDS reads of two nodes are in flight together - the first form, a
// key per (node, class) behind a branch on the class byte, took 4.0 us per iteration at n = 1000, K = 2 and 19.9 at
// K = 8, this one 2.6 and 10.6 (unrolled by four the compiler spilled 36 bytes of scratch).
// Then a 64-lane max butterfly on the VALU (v_permlane32/16_swap + DPP, as gmc::xor_add) gives
// every lane the winner, which is read straight from the key; then one lane per edge of the winner's row updates the
// neighbours' W rows (a row holds a neighbour once, so the read-modify-writes need no atomics).  The wave's own LDS
// traffic is ordered by wavefront-scope fences and wave barriers: no __syncthreads() inside the loop.
//
// The snapshot copy is deferred: an improving move only marks it pending; the state is copied before the first move
// that does not improve (and at the end), which gives the same bytes as copying at every improvement.
//
// After the chains the whole workgroup scores each of its snapshots with gmc::block_cut - 256 threads, the summation
// order of every other decoder, so the reported cuts carry the same bits - and writes them back; the second launch is
// the pick.  (The scoring is the tail of the chain launch and not a launch of its own: the pick needs every cut of a
// graph, so scoring and picking cannot share a launch without communication between workgroups, and this way the
// call stays at two launches with the snapshots scored out of LDS.)
//
// gmc_kway_tabu_c_f32 is the same search on cut minus per-node class costs: tabu_cost_kernel<K>, the same body text
// (tabu_kernel_body.inc) with the table started from the node's cost row and the snapshots scored by gmc::block_score.
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"
#include "tabu_body.h"   // the layout, wave_sync, wave_max, ordered_bits / ordered_float: shared with kway_balance.hip

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

struct TabuArgs {
    gmc_batch b;
    int first;               // first movable local id: K with terminals, 0 without
    int cands, iterations;
    unsigned tenure_base, tenure_span, tenure_div;
    u64 seed;
    signed char *assign;     // [cands][R], in/out
    float *cut_all;          // [B][cands]
    int *best_iter;          // [B][cands] or NULL
    int *moves;              // [B][cands] or NULL
    int slots, staged, n_pad, chain_bytes, off_starts, off_vals, off_ids;
};

// gmc_kway_tabu_c_f32's launch: TabuArgs' fields and the cost.  A struct of its own, so that TabuArgs keeps its layout.
struct TabuCostArgs {
    gmc_batch b;
    int first;
    int cands, iterations;
    unsigned tenure_base, tenure_span, tenure_div;
    u64 seed;
    signed char *assign;
    float *cut_all;
    int *best_iter;
    int *moves;
    int slots, staged, n_pad, chain_bytes, off_starts, off_vals, off_ids;
    const float *node_cost;  // [R][K] by batch row (read from global memory)
};

// Two kernels over one body text (tabu_kernel_body.inc, which says why): tabu_kernel<K> is the launch without costs,
// tabu_cost_kernel<K> the one with them.
#define GMC_COST false
#define GMC_CHAIN_ARGS TabuArgs
#define GMC_CHAIN_KERNEL tabu_kernel
#include "tabu_kernel_body.inc"
#undef GMC_COST
#undef GMC_CHAIN_ARGS
#undef GMC_CHAIN_KERNEL

#define GMC_COST true
#define GMC_CHAIN_ARGS TabuCostArgs
#define GMC_CHAIN_KERNEL tabu_cost_kernel
#include "tabu_kernel_body.inc"
#undef GMC_COST
#undef GMC_CHAIN_ARGS
#undef GMC_CHAIN_KERNEL

struct TabuPickArgs {
    gmc::PickArgs p;
    int first;
};
__global__ __launch_bounds__(256) void tabu_pick_kernel(TabuPickArgs a) {
    const int g = blockIdx.x;
    const int n = a.p.b.goff[g + 1] - a.p.b.goff[g];
    if (n > a.p.b.n_max || n < (a.first > 1 ? a.first : 1)) return;   // workgroup-uniform: the graphs the chains skipped
    gmc::pick_best(a.p);
}

}  // namespace

extern "C" int gmc_kway_tabu_fits(const gmc_batch *batch, int32_t K) {
    return gmc::chain_query(batch, K, false);
}

extern "C" int gmc_kway_tabu_shape(const gmc_batch *batch, int32_t K) {
    return gmc::chain_query(batch, K, true);
}

extern "C" int gmc_kway_tabu_f32(const gmc_batch *batch, int32_t K, int32_t terminals, int32_t cands, int8_t *assign,
                                 int32_t iterations, int32_t tenure_base, int32_t tenure_span, int32_t tenure_div,
                                 uint64_t seed, float *cut_all, int32_t *best_assign, float *best_cut,
                                 int32_t *best_idx, int32_t *best_iter, int32_t *moves, gmc_stream_t stream) {
    if (!batch || !assign || !cut_all || !best_assign || !best_cut || !best_idx) return GMC_ERR_NULL;
    int first;
    TabuLayout L;
    int rc = gmc::chain_checks(batch, K, terminals, cands, iterations, tenure_base, tenure_span, tenure_div, first,
                               L);
    if (rc != GMC_OK || batch->B == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TabuArgs a{*batch, first, cands, iterations, (unsigned)tenure_base, (unsigned)tenure_span,
                     (unsigned)tenure_div, seed, reinterpret_cast<signed char *>(assign), cut_all, best_iter, moves,
                     L.slots, L.staged, L.n_pad, L.chain_bytes, L.off_starts, L.off_vals, L.off_ids};
    GMC_KWAY_DISPATCH(K, rc = gmc::chain_launch(tabu_kernel<KK>, a, L.bytes, st));
    if (rc != GMC_OK) return rc;
    const TabuPickArgs p{{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign, best_cut,
                          best_idx}, first};
    hipLaunchKernelGGL(tabu_pick_kernel, dim3(batch->B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" int gmc_kway_tabu_c_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const float *node_cost,
                                   int32_t cands, int8_t *assign, int32_t iterations, int32_t tenure_base,
                                   int32_t tenure_span, int32_t tenure_div, uint64_t seed, float *cut_all,
                                   int32_t *best_assign, float *best_cut, int32_t *best_idx, int32_t *best_iter,
                                   int32_t *moves, gmc_stream_t stream) {
    if (!node_cost)   // the launch without costs: the twin, kernel for kernel
        return gmc_kway_tabu_f32(batch, K, terminals, cands, assign, iterations, tenure_base, tenure_span, tenure_div,
                                 seed, cut_all, best_assign, best_cut, best_idx, best_iter, moves, stream);
    if (!batch || !assign || !cut_all || !best_assign || !best_cut || !best_idx) return GMC_ERR_NULL;
    int first;
    TabuLayout L;
    int rc = gmc::chain_checks(batch, K, terminals, cands, iterations, tenure_base, tenure_span, tenure_div, first,
                               L);
    if (rc != GMC_OK || batch->B == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TabuCostArgs a{*batch, first, cands, iterations, (unsigned)tenure_base, (unsigned)tenure_span,
                         (unsigned)tenure_div, seed, reinterpret_cast<signed char *>(assign), cut_all, best_iter, moves,
                         L.slots, L.staged, L.n_pad, L.chain_bytes, L.off_starts, L.off_vals, L.off_ids, node_cost};
    GMC_KWAY_DISPATCH(K, rc = gmc::chain_launch(tabu_cost_kernel<KK>, a, L.bytes, st));
    if (rc != GMC_OK) return rc;
    const TabuPickArgs p{{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign, best_cut,
                          best_idx}, first};
    hipLaunchKernelGGL(tabu_pick_kernel, dim3(batch->B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
