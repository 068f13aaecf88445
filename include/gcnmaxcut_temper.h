/* gcnmaxcut_temper.h - parallel tempering (replica exchange) over decoded partitions at K = 2 .. GMC_KWAY_MAX_CLASSES
 * classes, an extension of include/gcnmaxcut.h with entry points of its own.  It shares that header's structs
 * (gmc_batch), status codes, stream type and conventions: the library allocates nothing, every array is the caller's
 * device memory of the size stated here, every call is issued on the caller's stream and does not synchronise with the
 * host.
 *
 * The `cands` candidates ("slots") of a graph are walkers of the annealing's Metropolis sweep
 * (gmc_kway_refine_anneal_c_f32, step 2), but instead of one cooling schedule shared by all of them they sit on ladders
 * of `rungs` fixed inverse temperatures, ladder[0] first (the caller's order; by convention the hottest).  Slot i belongs
 * to ladder copy c = i / rungs; the cands / rungs copies are independent.  After every round of round_sweeps sweeps the
 * walkers on neighbouring rungs of a copy exchange their rungs by the Metropolis rule.  Temperatures move between slots,
 * states stay in their slot: `state` is updated in place by its own workgroup only.
 *
 * ARITHMETIC.  Every product and every sum below is a float32 operation rounded on its own (no fused multiply-add); the
 * rule uses neither exp nor log (the caller's level table stands for them, as in the annealing).  mix64 is splitmix64's
 * finaliser, GOLD = GMC_TEMPER_GOLD = 0x9E3779B97F4A7C15, all counters in uint64 arithmetic (wrapping).  A float32
 * restatement in numpy therefore agrees byte for byte.
 *
 * Round t = 0 .. rounds - 1 for (slot i, graph g); one launch per round, one 256-thread workgroup per (slot, graph):
 *  1. Rung.  t = 0: the rung is i % rungs and the swap count is 0.  t > 0: let r be the slot's rung after round t - 1.
 *     The pairs of this round are the rungs (p, p + 1) with p = t (mod 2) and p + 1 < rungs; a rung in no pair stays.
 *     If r lies in the pair (p, p + 1), lo and hi are the slots of the same ladder copy that held rungs p and p + 1,
 *     x_lo and x_hi the scores their walkers had at the end of round t - 1, and
 *         d = (ladder[p + 1] - ladder[p]) * (x_hi - x_lo)                 two subtractions, one multiplication
 *         h = mix64(E + GOLD * ((((uint64)t << 40) | ((uint64)c << 8) | p) + 1)),   E = mix64(seed ^ GMC_TEMPER_TAG)
 *     The two slots exchange rungs iff d < 0 || d <= levels[h >> 54] - the move test's form; with the usual table
 *     (levels[j] = -log((j + 0.5) / 1024)) it accepts with probability min(1, exp(-d)), d = (beta_hi - beta_lo)(x_hi -
 *     x_lo) being the fall of sum beta * (-score) the exchange would undo.  Both partners compute the same decision from
 *     the same words; each writes its own rung and adds 1 to its own swap count.  The hash holds no graph index.
 *  2. Sweeps.  round_sweeps sweeps of step 2 of gmc_kway_refine_anneal_c_f32 at inv_temp = ladder[rung]: the same node
 *     visit in the same (colour, id) order, the sums starting from node_cost when it is given, the level of node v in
 *     sweep s being levels[mix64(seed + GOLD * ((cand << 32 | s << 12 | v) + 1)) >> 54] with cand = i and
 *     s = t * round_sweeps + j, j = 0 .. round_sweeps - 1.  `seed` enters unmixed.
 *  3. Best.  Before round 0's sweeps the best state is the input state and best_score its score.  After every sweep the
 *     score is recounted as the annealing recounts it (the cut, minus the cost with node_cost: gmc_kway_refine_anneal_c_f32's
 *     summation order); on a strictly larger score the best state, best_score and best_round = t are replaced - the
 *     annealing's snapshot rule.  The score after the round's last sweep is the x the next round reads.
 * After the call: state [cands][R] holds the walkers, best [cands][R] the best states, best_score [B][cands] their
 * scores, best_round [B][cands] the round that found them (0 also for the input), rung_out [B][cands] the rung of every
 * slot after the last round and swaps [B][cands] the exchanges it took part in.
 *
 * There is no descent and no pick inside: the caller hands `best` to gmc_kway_refine_anneal_c_f32 with
 * anneal_sweeps = 0, which descends, scores and picks.  rounds = 0 issues one launch that copies state to best, scores
 * it and writes best_round = 0, rung_out = i % rungs and swaps = 0.
 *
 * By construction:
 *  (a) Equality with the annealing.  When all ladder entries equal beta, `best` is byte for byte what
 *      gmc_kway_refine_anneal_c_f32 leaves in `assign` for anneal_sweeps = rounds * round_sweeps, every inv_temp equal to
 *      beta, max_descent_sweeps = 0 and the same seed, for every `rungs` that divides `cands` (an exchange then changes
 *      no temperature).  For unit and integer weights (and integer costs) best_score carries cut_all's bits.
 *  (b) Rungs.  After every round the rungs of a ladder copy are a permutation of 0 .. rungs - 1.
 *  (c) Score.  best_score is never below the score of the input state.
 *  (d) Reproducibility.  All outputs are reproducible bit for bit, and a slot's outputs depend on its graph, its ladder
 *      copy (the slots of the copy and their index), the seed, the ladder and the table alone - not on the graph's
 *      place in the batch nor on the rest of the batch.
 *
 * The workspace: gmc_kway_temper_workspace_bytes(batch, cands) bytes, 16-byte aligned: two planes of rung
 * [B][cands] int32 followed by two planes of score [B][cands] float, each plane padded to 16 bytes.  It is NOT assumed
 * zeroed: every word read is written by the call first.  Round t reads plane (t - 1) & 1 and writes plane t & 1; nothing
 * is updated in place across workgroups, kernel boundaries are the only synchronisation (no atomics, no spin waits).  A
 * rung read from the workspace is range-checked before it is used as an index (a slot whose own word is out of range
 * takes i % rungs and does not exchange), and a partner that is not found means no exchange; neither can arise from the
 * call's own writes.
 *
 * order / cgoff / cptr (device memory) come from gmc_order_host_t(K, terminals).  Launches: max(rounds, 1); the number
 * never depends on data.
 *
 * Argument checks, before any HIP call, in the order of gmc_kway_evolve_f32: a NULL required pointer (batch, order,
 * cgoff, cptr, ladder, levels, state, best, best_score, workspace; node_cost, best_round, rung_out and swaps may be
 * NULL) GMC_ERR_NULL; batch->abi GMC_ERR_ABI; a NULL goff / rowptr / lcol GMC_ERR_NULL; K outside
 * 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES; rungs outside 1..GMC_TEMPER_MAX_RUNGS, cands < 1, cands % rungs != 0,
 * rounds < 0, round_sweeps < 1 with rounds > 0 (< 0 with rounds = 0), rounds * round_sweeps >= 2^20 (the counter layout),
 * B < 0, terminals outside {0, 1} GMC_ERR_SHAPE; n_max below max(first, 1), first = K with terminals and 0 without, or
 * above GMC_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE; a workspace that is not 16-byte aligned GMC_ERR_ALIGN, one below
 * gmc_kway_temper_workspace_bytes GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a launch.  A graph with fewer than
 * `first` or more than n_max nodes inside a batch is skipped: nothing of it is written. */
#ifndef GCNMAXCUT_TEMPER_H
#define GCNMAXCUT_TEMPER_H

#include "gcnmaxcut.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMC_TEMPER_GOLD 0x9E3779B97F4A7C15ULL
#define GMC_TEMPER_TAG 0x54454D5045523031ULL /* "TEMPER01": separates the exchanges' draws from the sweeps' */
#define GMC_TEMPER_MAX_RUNGS 256

/* bytes of workspace gmc_kway_temper_f32 needs (0 for a NULL struct, another abi word, B < 0 or cands < 1); host only,
 * reads B */
size_t gmc_kway_temper_workspace_bytes(const gmc_batch *batch, int32_t cands);

int gmc_kway_temper_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const float *node_cost /*[R][K] or NULL*/,
                        const int32_t *order, const int32_t *cgoff, const int32_t *cptr, int32_t cands, int32_t rungs,
                        const float *ladder /*[rungs], 1/T, rung 0 first*/, int32_t rounds, int32_t round_sweeps,
                        const float *levels /*[GMC_ANNEAL_LEVELS]*/, uint64_t seed,
                        int8_t *state /*[cands][R], in/out: the walkers*/, int8_t *best /*[cands][R], out*/,
                        float *best_score /*[B][cands]*/, int32_t *best_round /*[B][cands] or NULL*/,
                        int32_t *rung_out /*[B][cands] or NULL*/, int32_t *swaps /*[B][cands] or NULL*/, void *workspace,
                        size_t workspace_bytes, gmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
