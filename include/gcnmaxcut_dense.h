/* gcnmaxcut_dense.h - annealing of dense two-class instances (max-cut, Ising, QUBO on a full matrix) on cached local
 * fields, an extension of include/gcnmaxcut.h with entry points of its own.  It shares that header's status codes,
 * stream type and conventions: the library allocates nothing, every array is the caller's device memory of the size
 * stated here, every call is issued on the caller's stream and does not synchronise with the host.
 *
 * B problems of the same size n, 2 <= n <= GMC_MAX_GRAPH_NODES (the move counter's 12-bit node field), two classes, no
 * terminals.  Problem b owns the matrix W + b * n * ld (n rows of ld floats, ld >= n, symmetric) and the rows b * n ..
 * b * n + n - 1 of everything of R = B * n rows.  The objective is that of the per-node class costs of gcnmaxcut.h:
 *     obj(S) = cut(S) - sum_v node_cost[v][S_v],     cut(S) = sum_{u<v} W[u][v] [S_u != S_v].
 * The diagonal and the columns n .. ld-1 are never read.  W[u][v] and W[v][u] must hold the same bits; the kernel may read
 * either.  A class byte is taken as byte & 1.  assign [cands][R], best_assign [R] and the per-candidate outputs [B][cands]
 * are laid out as gmc_kway_refine_anneal_c_f32 lays them out, so the two calls can be compared array for array.
 *
 * Where the sparse decoders recompute a node's class sums from its CSR row on every visit, this call keeps ONE cached
 * local field per node, decides a visit from that number alone, and pays O(n) only for an accepted move: one coalesced
 * read of a row of W.
 *
 * ARITHMETIC.  Every product and every sum below is a float32 operation rounded on its own (no fused multiply-add); the
 * rule uses neither exp nor log (the caller's level table stands for them, as in the annealing).  mix64 is splitmix64's
 * finaliser, GOLD = 0x9E3779B97F4A7C15, all counters in uint64 arithmetic (wrapping).  "x takes a" below means
 * x = x + a.  A float32 restatement in numpy (tests/dense_ref.py) therefore agrees byte for byte.
 *
 * Per (candidate cand, problem), S the class bytes & 1:
 *  1. Fields.  For every v, W_k(v) (k = 0, 1) starts from node_cost[v][k] (+0.0f without costs); then for u = 0 .. n-1
 *     ascending, u != v, W_k(v) takes W[v][u] where S_u == k and +0.0f where it is not (the sparse kernels' select).
 *     F[v] = W_1(v) - W_0(v), one subtraction.
 *  2. Score of a state.  For every row v, t_v starts from +0 and, for u ascending, u != v, takes W[v][u] where
 *     S_u != S_v and +0.0f where not.  Lane j of 64 adds t_v for v = j, j + 64, ... ascending, from +0; the 64 lanes fold
 *     by the butterfly x[i] += x[i ^ d], d = 32, 16, 8, 4, 2, 1, and the result is multiplied by 0.5f: the cut.  The cost
 *     of a state is summed the same way from node_cost[v][S_v] (no halving); score = cut - cost, one subtraction (without
 *     costs: the cut).  obj and best_obj start at this score and `best` at the input state.
 *  3. Annealing sweep s = 0 .. anneal_sweeps - 1.  For i = 0 .. n-1: v = order ? order[i] : i, c = S_v,
 *         delta = c == 0 ? F[v] : -F[v]              (W[other] - W[own]: the quantity gmc_kway_refine_anneal_f32 tests at K = 2)
 *         h = mix64(seed + GOLD * (ctr + 1)),   ctr = (uint64)cand << 32 | (uint64)s << 12 | v      (gmc_refine_anneal_f32's)
 *     v moves iff delta < 0 || delta * inv_temp[s] <= levels[h >> 54].  On a move: S_v = 1 - c; obj = obj - delta; for
 *     every u != v, F[u] = F[u] + (c == 0 ? 2.0f * W[v][u] : -(2.0f * W[v][u])); moves is incremented.  After the sweep,
 *     if obj > best_obj: best = state, best_obj = obj, snap_sweep = s + 1 (0: the input state stayed the best).  An entry
 *     of `order` outside 0 .. n-1 is skipped.
 *  4. Descent.  With anneal_sweeps > 0: state = best and F is recomputed by step 1 from that state - the accumulated
 *     fields are dropped, so the descent starts without drift.  Sweeps in the same order; a node moves iff delta < 0 (the
 *     same updates, `moves` not counted).  The descent stops after a sweep that moves nothing or after
 *     max_descent_sweeps; `sweeps` counts the sweeps run, the one that moved nothing included, as the local search does.
 *  5. Final score and pick.  score_all[b][cand] is step 2 recomputed on the final state, not the running obj; assign
 *     receives the final state (bytes 0 / 1).  The pick is the strictly best candidate of a problem, the first on ties:
 *     best_idx [B], best_score [B], best_assign [R] (int32).
 *
 * By construction, with integer weights and costs whose partial sums stay below 2^24 every output is byte for byte that
 * of gmc_kway_refine_anneal_c_f32(K = 2, terminals = 0) when the CSR holds the non-zero entries of W and `order` is that
 * batch's colour order from gmc_order_host_t (made local: minus b * n) - on any graph, sparse or dense: a colour class is
 * an independent set, so the sequential visit in (colour, id) order equals the parallel colour step, and a +-0 entry
 * changes no sum.  For real weights the two calls follow the same rule but NOT the same rounding (the fields are
 * updated move by move here and summed afresh on every visit there; the running obj here is a recount there): the
 * contract for real weights is the numpy restatement.  Also by construction: (b) an all-zero node_cost gives the bytes
 * of NULL; (c) score_all is never below the input's score when the data are integers (the snapshot rule and the descent
 * only climb; with real weights the running obj may drift from the recount by rounding); (d) a chain's outputs depend
 * on its own problem, its index cand, the seed, the schedule and the table alone.  All outputs are reproducible bit for
 * bit.
 *
 * The kernel (csrc/dense_anneal.hip): one wave per chain, four chains per 256-thread workgroup; F, the class bytes and
 * the snapshot of a chain live in LDS, 6 bytes per node, rounded up to 16 nodes, beside one copy of the level table; no
 * workgroup barrier inside the sweeps, no atomics, no spin waits.  Launches: 2 for B > 0 (the chains; the pick) - the
 * number never depends on data.
 *
 * The workspace: gmc_dense_anneal_workspace_bytes(B, n, cands) bytes.  Every chain of this kernel fits LDS at every
 * admitted n, so nothing spills: the size is the constant GMC_DENSE_WORKSPACE_MIN for valid sizes and the call neither
 * reads nor writes the bytes (it is not assumed zeroed).  The argument stays so that a variant whose chains outgrow LDS
 * can take memory without a new signature.
 *
 * Argument checks, before any HIP call, in the order of the other decoders: a NULL required pointer (W, assign,
 * score_all, best_assign, best_score, best_idx, workspace; node_cost, order, snap_sweep, sweeps and moves may be NULL)
 * GMC_ERR_NULL; B < 0, cands < 1, anneal_sweeps < 0, max_descent_sweeps < 0 GMC_ERR_SHAPE; inv_temp or levels NULL with
 * anneal_sweeps > 0 GMC_ERR_NULL; n outside 2 .. GMC_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE; anneal_sweeps >= 2^20 (the
 * counter layout) GMC_ERR_SHAPE; ld < n GMC_ERR_SHAPE; a workspace below gmc_dense_anneal_workspace_bytes
 * GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a launch. */
#ifndef GCNMAXCUT_DENSE_H
#define GCNMAXCUT_DENSE_H

#include "gcnmaxcut.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMC_DENSE_WORKSPACE_MIN 16

/* bytes of workspace gmc_dense_anneal_f32 needs; host only; 0 for bad sizes (B < 0, n outside 2..GMC_MAX_GRAPH_NODES,
 * cands < 1) */
size_t gmc_dense_anneal_workspace_bytes(int32_t B, int32_t n, int32_t cands);

int gmc_dense_anneal_f32(int32_t B, int32_t n, const float *W /*[B][n][ld], symmetric*/, int64_t ld,
                         const float *node_cost /*[B*n][2] or NULL*/,
                         const int32_t *order /*[B*n]: per problem a permutation of 0..n-1, or NULL = identity*/,
                         int32_t cands, int8_t *assign /*[cands][B*n], in/out*/, const float *inv_temp /*[anneal_sweeps]*/,
                         int32_t anneal_sweeps, const float *levels /*[GMC_ANNEAL_LEVELS]*/, uint64_t seed,
                         int32_t max_descent_sweeps, void *workspace, size_t workspace_bytes,
                         float *score_all /*[B][cands]*/, int32_t *best_assign /*[B*n]*/, float *best_score /*[B]*/,
                         int32_t *best_idx /*[B]*/, int32_t *snap_sweep /*[B][cands] or NULL*/,
                         int32_t *sweeps /*[B][cands] or NULL*/,
                         int64_t *moves /*[B][cands] or NULL: accepted annealing moves*/, gmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
