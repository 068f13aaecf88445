/* gcnmaxcut_sdp.h - the low-rank semidefinite relaxation of max-cut (Goemans-Williamson) and its hyperplane rounding,
 * an extension of include/gcnmaxcut.h with entry points of its own.  It shares that header's structs (gmc_batch), status
 * codes, stream type and conventions: the library allocates nothing, every array is the caller's device memory of the
 * size stated here, every call is issued on the caller's stream and does not synchronise with the host.
 *
 * The relaxation.  max-cut's semidefinite program, maximise 1/2 sum_{uv} w_uv (1 - v_u . v_v) over unit vectors v_u, is
 * solved in its low-rank form (Burer-Monteiro): v_u has `rank` floats, and the "mixing method" updates one node at a
 * time, v_i <- -normalize(sum_j w_ij v_j), which never lowers the objective for any weights' signs.  Two classes only
 * (K = 2).  The reference direction t is the first coordinate axis, (1, 0, ..., 0); class 0 is "on t's side".  With a
 * per-node class cost (node_cost [R][2], the objective obj(S) = cut(S) - sum_v node_cost[v][S_v] of the `_c` entry points
 * of gcnmaxcut.h) s_v in {+1 class 0, -1 class 1} is relaxed to t . v_v, which adds a linear term along t.
 *
 * The state is V [R][rank] float32, one row per batch row, caller-owned; rank is 16, 32 or 64.
 *
 * The kernels run in the manner of gmc_large_round_conditional_f32: a graph is shared by several workgroups, a colour
 * step is one launch over that colour's nodes of every graph (nodes of one colour are pairwise non-adjacent, so the
 * in-place update of a colour is exactly Gauss-Seidel in colour order), kernel boundaries are the only synchronisation
 * (no atomics, no spin waits), the workspace is NOT assumed zeroed (every word read is written by the call first), and
 * rows are read by batch row id and neighbours through gcol (batch->gcol is required).  A node occupies `rank` adjacent
 * lanes, so a neighbour's row is one contiguous read of 64 to 256 bytes.  Graphs of 1 .. GMC_LARGE_MAX_GRAPH_NODES nodes
 * (2 .. with terminals).  All outputs are reproducible bit for bit, and a graph's outputs depend on its own rows, its
 * key and its colour classes alone - not on what else is in the batch.
 *
 * The order arrays (order / cgoff / cptr, device memory) and max_classes come from gmc_order_host_t(K = 2, terminals).
 *
 * ARITHMETIC.  Every product and every sum below is a float32 operation rounded on its own (no fused multiply-add);
 * square root and division are correctly rounded (IEEE round to nearest even).  A float32 restatement in numpy
 * therefore agrees byte for byte.  mix64 is splitmix64's finaliser, GMC_SDP_GOLD = 0x9E3779B97F4A7C15, all counters in
 * uint64 arithmetic (wrapping).
 *
 * 1. Init (init = 1).  Entry k of local node l of graph g is x_k = (float)(i - 2^23), i the top 24 bits of
 *    mix64(gkey[g] + GMC_SDP_GOLD * (l * rank + k + 1)) - an integer in -2^23 .. 2^23 - 1, exact in float32.  With
 *    s = the sum of the x_k * x_k by the butterfly of rule 2 and n = sqrt(s): V[row][k] = x_k / n; a row with s == 0
 *    becomes t.  With terminals = 1 local node 0 is +t and local node 1 is -t (that is (-1, 0, ..., 0) with +0.0f behind);
 *    those two rows are never visited.  With init = 0 V is taken as it is (gkey may then be NULL), so sweeps = a + b gives
 *    the bytes of sweeps = a followed by sweeps = b with init = 0.
 * 2. Visit of a movable node, row r.  g_k starts from +0.0f, except that g_0 starts from node_cost[r][0] -
 *    node_cost[r][1] when node_cost is given.  Then, for the row's CSR entries e in order, the diagonal entry
 *    (gcol[e] == r) skipped: g_k = g_k + w_e * V[gcol[e]][k]  (w_e = 1.0f without batch->vals).  With x_k = g_k * g_k the
 *    sum s is taken by a butterfly over the node's rank lanes: for d = rank/2, rank/4, ..., 1: x[i] = x[i] + x[i ^ d] for
 *    every i at once.  n = sqrt(s).  If n is 0 or not finite the row stays as it is; otherwise V[r][k] = -(g_k / n).
 *    A sweep visits the colour classes in ascending order; one launch per colour.
 * 3. Value (value [B]) after the last sweep: per row r one partial by one thread,
 *        p = +0.0f;  for the row's CSR entries in order, the diagonal skipped:
 *            d = +0.0f;  for k ascending: d = d + V[r][k] * V[gcol[e]][k];      p = p + w_e * (1.0f - d);
 *        x_r = 0.25f * p                     (every undirected edge is two entries: half of its 1/2 from each side)
 *        with node_cost (c0, c1 = node_cost[r][0..1]):  x_r = x_r - ((c0 + c1) * 0.5f + ((c0 - c1) * 0.5f) * V[r][0]);
 *    then a tile of 256 rows of the graph (rows past its end count +0.0f) by the butterfly over each wave of 64 rows,
 *    d = 32 .. 1, and the four waves' sums added ascending from +0.0f; then the graph's tiles ascending from +0.0f
 *    (gmc_large_round_conditional_f32's order, without its final * 0.5f).  It is the relaxed form of obj(S): an upper
 *    bound on the optimum only at the relaxation's optimum, not a certificate.
 * 4. Hyperplane m (m >= 0) of graph g: h_k = (float)(D - 6 * 2^20), D the sum of twelve draws d_j, j = 0..11, each the top
 *    20 bits of mix64((gkey[g] ^ GMC_SDP_PLANE_TAG) + GMC_SDP_GOLD * ((m * 12 + j) * 64 + k + 1)) - an exact integer (an
 *    Irwin-Hall stand-in for a Gaussian).  For row r: p = +0.0f; for k ascending: p = p + h_k * V[r][k], in one thread.  The
 *    class byte is 0 iff (p >= 0) == (h_0 >= 0), else 1.  With terminals = 1 local nodes 0 and 1 get bytes 0 and 1 outright.
 *    assign [planes][R] int8 holds plane first_plane + q in its row q: a plane's bytes depend neither on the batch nor
 *    on first_plane / planes.
 *
 * Launches of gmc_sdp_relax_f32: init + sweeps * max_classes + 2 (value, fold); of gmc_sdp_round_f32: 1.  The number
 * never depends on data.
 *
 * The workspace of gmc_sdp_relax_f32: gmc_sdp_workspace_bytes(batch, rank) bytes, 16-byte aligned: R / 256 + B + 1 float
 * partials of the value (the slots of graph g: goff[g] / 256 + g onwards), padded to 16 bytes.
 *
 * Argument checks, before any HIP call, in this order (those of the large decoders): a NULL required pointer
 * (batch, order, cgoff, cptr, V, value, workspace; gkey with init = 1; node_cost may be NULL) GMC_ERR_NULL; batch->abi
 * GMC_ERR_ABI; a NULL goff / rowptr / lcol / gcol GMC_ERR_NULL; rank other than 16, 32, 64, sweeps < 0, max_classes < 0,
 * B < 0, terminals or init outside {0, 1} GMC_ERR_SHAPE; n_max < 1 (2 with terminals) or > GMC_LARGE_MAX_GRAPH_NODES
 * GMC_ERR_GRAPH_SIZE; V or the workspace not 16-byte aligned GMC_ERR_ALIGN; R < 0 or a workspace below
 * gmc_sdp_workspace_bytes GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a launch.  gmc_sdp_round_f32 likewise
 * (batch, V, gkey, assign required; first_plane < 0, planes < 0 or first_plane + planes beyond 2^31 - 1 GMC_ERR_SHAPE; it
 * has no workspace; planes == 0 returns GMC_OK without a launch).
 * A graph with fewer nodes than that or more than n_max inside a batch is skipped: nothing of it is written. */
#ifndef GCNMAXCUT_SDP_H
#define GCNMAXCUT_SDP_H

#include "gcnmaxcut.h"

#ifdef __cplusplus
extern "C" {
#endif

#define GMC_SDP_GOLD 0x9E3779B97F4A7C15ULL
#define GMC_SDP_PLANE_TAG 0x53445020504C414EULL /* "SDP PLAN": separates the planes' draws from the init's */

/* bytes of workspace gmc_sdp_relax_f32 needs (0 for a NULL struct, another abi word, a rank other than 16, 32, 64 or
 * negative sizes); host only, reads B and R */
size_t gmc_sdp_workspace_bytes(const gmc_batch *batch, int32_t rank);

int gmc_sdp_relax_f32(const gmc_batch *batch, int32_t rank, int32_t terminals, const float *node_cost /*[R][2] or NULL*/,
                      const int32_t *order, const int32_t *cgoff, const int32_t *cptr, int32_t max_classes,
                      const uint64_t *gkey /*[B]; may be NULL with init = 0*/, int32_t init, int32_t sweeps,
                      float *V /*[R][rank], in/out*/, float *value /*[B]*/, void *workspace, size_t workspace_bytes,
                      gmc_stream_t stream);

int gmc_sdp_round_f32(const gmc_batch *batch, int32_t rank, int32_t terminals, const float *V /*[R][rank]*/,
                      const uint64_t *gkey /*[B]*/, int32_t first_plane, int32_t planes,
                      int8_t *assign /*[planes][R]*/, gmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
