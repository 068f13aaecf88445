/* gcnmaxcut_bifurcation.h - discrete simulated bifurcation ("dSB": Goto, Tatsumura, Dixon 2019; the discrete form of Goto
 * et al. 2021) for dense two-class instances, an extension of include/gcnmaxcut_dense.h with entry points of its own.  It
 * takes that header's conventions: B problems of the same size n, 2 <= n <= GMC_MAX_GRAPH_NODES, problem b owns the matrix
 * W + b * n * ld (n rows of ld floats, ld >= n, symmetric) and the rows b * n .. b * n + n - 1 of everything of R = B * n
 * rows; two classes, no terminals; node_cost [R][2] or NULL; the library allocates nothing, every call is issued on the
 * caller's stream and does not synchronise with the host.
 *
 * The objective is gcnmaxcut_dense.h's: obj(S) = cut(S) - sum_v node_cost[v][S_v].  Class 0 is the spin s = +1, class 1 is
 * s = -1, as in the Ising door: maximising obj is minimising sum_{u<v} W[u][v] s_u s_v + sum_v g_v s_v with
 * g_v = node_cost[v][0] - node_cost[v][1], one subtraction (+0.0f without costs, and then never added).
 *
 * Where the annealing walks the nodes of a chain one after the other, this rule moves all nodes of all chains at once: a
 * time step is the product W . sign(X) - an [n, n] by [n, cands] GEMM on the fp32 matrix cores - and an elementwise
 * update.
 *
 * ARITHMETIC.  Every product and every sum below is a float32 operation rounded on its own (no contraction), except the
 * fmaf chain of step 2, which is what v_mfma_f32_16x16x4_f32 computes.  mix64 is splitmix64's finaliser,
 * GOLD = 0x9E3779B97F4A7C15, all counters in uint64 arithmetic (wrapping).  A float32 restatement in numpy
 * (tests/bifurcation_ref.py) follows the same text.
 *
 * A chain is one (candidate cand, problem) pair with two float32 numbers per node, position x_v and momentum y_v.  For step
 * t = 0 .. steps - 1, every v at once from the values of step t:
 *  1. s_u = x_u > 0 ? 1 : (x_u < 0 ? -1 : 0).
 *  2. f_v starts from +0.0f; for u = 0 .. n-1 ascending, f_v = fmaf(W[v][u], s_u, f_v), with W[v][v] taken as +0.0f.  The
 *     diagonal and the columns n .. ld-1 are never used: a NaN there reaches no output.  Since s_u is -1, 0 or +1, each
 *     step of the chain is one rounded addition.
 *  3. With a cost array, f_v = f_v + g_v.
 *  4. p = pump[t] * x_v; q = c0 * f_v; r = p + q; m = dt * r; y_v = y_v - m; m2 = dt * y_v; x_v = x_v + m2.
 *  5. Walls: if x_v > 1 then x_v = 1, y_v = 0; if x_v < -1 then x_v = -1, y_v = 0.
 * pump [steps] is the caller's float32 table of a0 - a(t) with a0 = 1 (as inv_temp is the annealing's; Python builds the
 * linear ramp from 1 to 0); c0 and dt are scalars of the call.  f is the negative force: the step descends
 * sum W s s + sum g s.  After the last step the class byte of v is x_v < 0 ? 1 : 0.  x and y are in/out, so a run can be
 * continued: one call of s1 + s2 steps equals a call of s1 steps followed by a call of s2 steps on the returned x, y with
 * the table's tail, byte for byte.
 *
 * SEEDED START (gmc_dense_sb_init_f32).  For cand and the local node v:
 *     h = mix64(seed + GOLD * (((uint64)cand << 32 | v) + 1))
 *     x = +0.0f
 *     t = (float)(int32)(h >> 40) - 8388608.0f      (24 bits, exact: an integer in -2^23 .. 2^23 - 1)
 *     u = t * 2^-23                                  (exact: -1 <= u < 1)
 *     y = amplitude * u                              (the one rounded operation)
 * Nothing is drawn on the host: a chain depends on its problem, cand, the seed and the parameters alone.
 *
 * LAYOUT.  x and y are two planes [R][cands] float32, row-major without padding: the element of row r = b * n + v and
 * candidate cand is plane[r * cands + cand] (numpy: shape (B * n, cands)); gmc_dense_sb_state_bytes is the size of each.
 * The candidates of a node lie side by side because the product is taken with rows = nodes: in the accumulator of
 * v_mfma_f32_16x16x4_f32 the 16 lanes of a register run along the columns, here the candidates, so the epilogue's loads
 * and stores of x, y and of the sign bytes are 16 consecutive elements per node (csrc/large_search.hip lays its class
 * bytes [R][cp] the same way).  The transposed product sign(X)^T . W would put nodes along the lanes, but it reads the
 * sign plane k-minor - a transposing, byte-wise trip into LDS on every k tile - where this form reads whole words.
 * assign is [cands][R] int8, gmc_dense_anneal_f32's layout, written once per call.
 *
 * CONTRACTS.  (a) With integer weights and costs whose partial sums stay below 2^24, f is exact in any order: x, y and the
 * class bytes after any number of steps are byte for byte the restatement's.  (b) Real weights: k runs ascending inside
 * one workgroup, there is no split over k and the edges are zero-filled, so the device is meant to be byte for byte the
 * k-ascending chain of step 2 (DESIGN.md section 41 says what was seen on the device).  (c) Splitting, above.
 * (d) A chain's bytes do not depend on cands, on which column of a tile it occupies, on B or on the problem's place in the
 * batch; an all-zero node_cost gives the bytes of NULL; two runs give the same bytes.
 *
 * The kernels (csrc/dense_sb.hip): an LDS-tiled fp32 MFMA product, tile 64 x 64 x 16, 32 x 64 x 16 or 64 x 16 x 16 chosen
 * per call from B, n and cands, whose epilogue is steps 3 - 5.  The signs of x live in two one-byte planes [R][cs],
 * cs = cands rounded up to 16, in the workspace: step t reads one and writes the other, so kernel boundaries are the only
 * synchronisation (no atomics, no spin waits); x and y are touched only by the thread that owns the element and update
 * in place.  The diagonal is zeroed as the W tile enters LDS.  Launches: steps + 1 for B > 0 (one that writes the signs
 * of the given x - and, with steps == 0, the class bytes - and one per step; the last step writes the class bytes) - the
 * number never depends on data.
 *
 * The workspace: gmc_dense_sb_workspace_bytes(B, n, cands) = 2 * B * n * cs + 16 bytes, not assumed zeroed; every word
 * read is written by the call first.
 *
 * Argument checks, before any HIP call, in gmc_dense_anneal_f32's order: a NULL required pointer (W, x, y, workspace,
 * assign; node_cost may be NULL) GMC_ERR_NULL; B < 0, cands < 1, steps < 0 GMC_ERR_SHAPE; pump NULL with steps > 0
 * GMC_ERR_NULL; n outside 2 .. GMC_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE; ld < n GMC_ERR_SHAPE; a workspace below
 * gmc_dense_sb_workspace_bytes GMC_ERR_WORKSPACE; c0 or dt not finite or not positive GMC_ERR_SHAPE; more than 2^31 - 1
 * tiles GMC_ERR_UNSUPPORTED; B == 0 returns GMC_OK without a launch.  steps == 0 writes the class bytes of the given x and
 * leaves x, y untouched.  gmc_dense_sb_init_f32: x or y NULL GMC_ERR_NULL; B < 0 or cands < 1 GMC_ERR_SHAPE; n
 * GMC_ERR_GRAPH_SIZE; an amplitude that is not finite GMC_ERR_SHAPE; B == 0 GMC_OK without a launch; else one launch. */
#ifndef GCNMAXCUT_BIFURCATION_H
#define GCNMAXCUT_BIFURCATION_H

#include "gcnmaxcut_dense.h"

#ifdef __cplusplus
extern "C" {
#endif

/* bytes of EACH of the two planes x and y; host only; 0 for bad sizes (B < 0, n outside 2..GMC_MAX_GRAPH_NODES,
 * cands < 1) */
size_t gmc_dense_sb_state_bytes(int32_t B, int32_t n, int32_t cands);

/* bytes of workspace gmc_dense_sb_f32 needs; host only; 0 for bad sizes */
size_t gmc_dense_sb_workspace_bytes(int32_t B, int32_t n, int32_t cands);

int gmc_dense_sb_init_f32(int32_t B, int32_t n, int32_t cands, uint64_t seed, float amplitude,
                          float *x /*[B*n][cands] out*/, float *y /*[B*n][cands] out*/, gmc_stream_t stream);

int gmc_dense_sb_f32(int32_t B, int32_t n, const float *W /*[B][n][ld], symmetric*/, int64_t ld,
                     const float *node_cost /*[B*n][2] or NULL*/, int32_t cands, float *x /*[B*n][cands], in/out*/,
                     float *y /*[B*n][cands], in/out*/, const float *pump /*[steps]*/, int32_t steps, float c0, float dt,
                     void *workspace, size_t workspace_bytes, int8_t *assign /*[cands][B*n] out*/, gmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
