// The seeded sampler and the annealing (with the local search as its descent) at K = 2..8 classes (an extension: the
// reference draws its uniforms from numpy's global RNG, samples and stops, TestingNeuralNetwork.py:18-98, and is
// 3-class).  Both algorithms are stated in include/gcnmaxcut.h.  The entry points of the reference's 3-class model
// (gmc_decode_sample_seeded_f32, gmc_refine_anneal_f32) and those of the models gmc_kway_forward serves
// (gmc_kway_decode_sample_seeded_f32, gmc_kway_refine_anneal_f32) check their own arguments and then run the same
// launches: the 3-class ones are K = 3.
//
// K is a template argument, one 256-thread workgroup per (candidate, graph).
//
// Sampler: a graph's key and the pair (iteration, local node) go through the counter-based hash of mix64.h, the top 53
// bits are the uniform (draw_body.h; large_search.hip draws with it too): nothing is generated on the host and nothing
// is copied.  The class bytes of a sample live in n_max bytes of LDS, the cut is gmc::block_cut's, so a sample scores
// bit for bit what gmc_decode_sample_f32 and gmc_refine_local_f32 report for the same assignment.  The pick kernel
// takes the winning iteration and REGENERATES that one assignment from the hash, so the [iters][R] array of all
// samples is optional: without it a call writes [B][iters] floats and [R] ints, whatever `iters` is.  The running sum
// of a row's probabilities lives in one register: the loop over the constant K is unrolled and stops comparing after
// the first class that takes the draw.
//
// Annealing: the LDS layout of anneal_layout.h (level table, state and best bytes, and the staged copy of the graph's
// CSR when it fits GMC_ANNEAL_LDS_BUDGET) - it does not depend on K.  The K sums of a node are compare-selected
// accumulators (move_body.h), "own sum" and "smallest among the others" unrolled compare chains; both accessor paths
// run one templated body (anneal_body.h, which kway_evolve.hip runs on its children too).
#include "gmc_common.h"
#include "cut_body.h"
#include "draw_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"
#include "anneal_body.h"

namespace {

using gmc::iteration_base;
using gmc::mix64;
using gmc::seeded_class_k;
using gmc::u64;
using gmc::AnnealArgs;
using gmc::AnnealLayout;
using gmc::GlobalCsr;
using gmc::LdsCsr;
using gmc::Sums;

// ---- the sampler --------------------------------------------------------------------------------------------------

struct SeededArgs {
    gmc_batch b;
    const float *P;          // [R,K]
    const u64 *gkey;         // [B]
    int iters;
    int first;               // first drawn local id: K with terminals (ids below it keep their own class), 0 without
    signed char *assign_all; // [iters][R] or NULL
    float *cut_all;          // [B][iters]
    int *best_assign;        // [R]        (the pick kernel)
    float *best_cut;         // [B]
    int *best_iter;          // [B]
    const float *node_cost;  // [R][K] or NULL: a sample scores cut - cost (gmc_kway_decode_sample_seeded_c_f32)
};

template <int K>
__global__ __launch_bounds__(256) void sample_seeded_k_kernel(SeededArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sa[];
    __shared__ float red[4];
    const int it = blockIdx.x, g = blockIdx.y;
    const int r0 = a.b.goff[g];
    const int n = a.b.goff[g + 1] - r0;
    const int first = a.first;
    if (n > a.b.n_max || n < first) return;   // (the LDS is sized by n_max; a graph without its terminals is skipped)
    const u64 base = iteration_base(a.gkey[g], it);
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const int c = l < first ? l : seeded_class_k<K>(base, l, a.P + (long)(r0 + l) * K);
        sa[l] = (unsigned char)c;
        if (a.assign_all) a.assign_all[(long)it * a.b.R + r0 + l] = (signed char)c;
    }
    __syncthreads();
    const float *nc = a.node_cost ? a.node_cost + (long)r0 * K : nullptr;
    const float cut = gmc::block_score<K>(a.b, nc, sa, r0, n, red);
    if (threadIdx.x == 0) a.cut_all[(long)g * a.iters + it] = cut;
}

// One workgroup per graph: the winning iteration, then its assignment again from the hash (never read from assign_all,
// so the call with and without that array runs the same code)
template <int K>
__global__ __launch_bounds__(256) void sample_seeded_k_pick_kernel(SeededArgs a) {
    const int g = blockIdx.x;
    const int r0 = a.b.goff[g], n = a.b.goff[g + 1] - r0;
    const int first = a.first;
    if (n > a.b.n_max || n < first) return;   // workgroup-uniform: the graphs the sampler skipped
    const int best = gmc::pick_best_index(a.cut_all, a.iters, g, a.best_cut, a.best_iter);
    const u64 base = iteration_base(a.gkey[g], best);
    for (int l = threadIdx.x; l < n; l += blockDim.x)
        a.best_assign[r0 + l] = l < first ? l : seeded_class_k<K>(base, l, a.P + (long)(r0 + l) * K);
}

template <int K>
int sample_launch_k(const SeededArgs &a, hipStream_t st) {
    {
        GmcProbeScope probe(GMC_K_SAMPLE, st);
        hipLaunchKernelGGL((sample_seeded_k_kernel<K>), dim3(a.iters, a.b.B), dim3(256), (size_t)a.b.n_max, st, a);
        GMC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL((sample_seeded_k_pick_kernel<K>), dim3(a.b.B), dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// what a sampler entry point does once its arguments are checked (B > 0, K in 2..8; first = K or 0)
int sample_launch(const gmc_batch *batch, const float *P, int K, int first, const uint64_t *gkey, int iters,
                  int8_t *assign_all, float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_iter,
                  gmc_stream_t stream, const float *node_cost = nullptr) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const SeededArgs a{*batch, P, reinterpret_cast<const u64 *>(gkey), iters, first,
                       reinterpret_cast<signed char *>(assign_all), cut_all, best_assign, best_cut, best_iter, node_cost};
    GMC_KWAY_DISPATCH(K, return sample_launch_k<KK>(a, st));
    return GMC_OK;
}

// ---- annealing + descent ------------------------------------------------------------------------------------------

// Two kernels over one body text (anneal_kernel_body.inc, which says why): anneal_k_kernel<K> is the launch without
// per-node class costs and keeps its name and, instruction for instruction, its code; anneal_k_cost_kernel<K> is the
// launch with them (a.node_cost != NULL).
template <int K>
__global__ __launch_bounds__(256) void anneal_k_kernel(AnnealArgs a) {
#define GMC_COST false
#include "anneal_kernel_body.inc"
#undef GMC_COST
}
template <int K>
__global__ __launch_bounds__(256) void anneal_k_cost_kernel(AnnealArgs a) {
#define GMC_COST true
#include "anneal_kernel_body.inc"
#undef GMC_COST
}

struct KPickArgs {
    gmc::PickArgs p;
    int first;
};
__global__ __launch_bounds__(256) void anneal_k_pick_kernel(KPickArgs a) {
    const int g = blockIdx.x;
    const int n = a.p.b.goff[g + 1] - a.p.b.goff[g];
    if (n > a.p.b.n_max || n < a.first) return;   // workgroup-uniform: the graphs the search skipped
    gmc::pick_best(a.p);
}

template <int K>
int anneal_launch_k(const AnnealArgs &a, int lds_bytes, hipStream_t st) {
    GmcProbeScope probe(GMC_K_ANNEAL, st);
    if (a.node_cost)
        hipLaunchKernelGGL((anneal_k_cost_kernel<K>), dim3(a.cands, a.b.B), dim3(256), (size_t)lds_bytes, st, a);
    else
        hipLaunchKernelGGL((anneal_k_kernel<K>), dim3(a.cands, a.b.B), dim3(256), (size_t)lds_bytes, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// what an annealing entry point does once its arguments are checked (B > 0, K in 2..8; first = K or 0)
int anneal_launch(const gmc_batch *batch, int K, int first, const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                  int cands, int8_t *assign, const float *inv_temp, int anneal_sweeps, const float *levels,
                  uint64_t seed, int max_descent_sweeps, float *cut_all, int32_t *best_assign, float *best_cut,
                  int32_t *best_idx, int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream,
                  const float *node_cost = nullptr) {
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AnnealLayout L = gmc::anneal_layout(batch);
    const AnnealArgs a{*batch, order, cgoff, cptr, cands, anneal_sweeps, max_descent_sweeps, first, inv_temp, levels, seed,
                       reinterpret_cast<signed char *>(assign), cut_all, snap_sweep, sweeps,
                       L.staged, L.n_pad, L.off_starts, L.off_vals, L.off_order, L.off_ids, node_cost};
    int rc = GMC_OK;
    GMC_KWAY_DISPATCH(K, rc = anneal_launch_k<KK>(a, L.bytes, st));
    if (rc != GMC_OK) return rc;
    const KPickArgs p{{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign, best_cut,
                       best_idx}, first};
    hipLaunchKernelGGL(anneal_k_pick_kernel, dim3(batch->B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

extern "C" int gmc_decode_sample_seeded_f32(const gmc_batch *batch, const float *P, const uint64_t *gkey,
                                            int32_t iters, int8_t *assign_all, float *cut_all, int32_t *best_assign,
                                            float *best_cut, int32_t *best_iter, gmc_stream_t stream) {
    if (!batch || !P || !gkey || !cut_all || !best_assign || !best_cut || !best_iter) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (iters < 1 || batch->B < 0) return GMC_ERR_SHAPE;
    if (batch->B > 0 && (batch->n_max < 3 || batch->n_max > 65535)) return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    return sample_launch(batch, P, 3, 3, gkey, iters, assign_all, cut_all, best_assign, best_cut, best_iter, stream);
}

// what gmc_kway_decode_sample_seeded_f32 and its _t twin do (terminals: 0 or 1); node_cost: the _c twin's, or NULL
static int kway_sample_seeded(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals, const float *node_cost,
                              const uint64_t *gkey, int32_t iters, int8_t *assign_all, float *cut_all,
                              int32_t *best_assign, float *best_cut, int32_t *best_iter, gmc_stream_t stream) {
    if (!batch || !P || !gkey || !cut_all || !best_assign || !best_cut || !best_iter) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (iters < 1 || batch->B < 0 || (terminals != 0 && terminals != 1)) return GMC_ERR_SHAPE;
    const int first = terminals ? K : 0;
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || batch->n_max > 65535))
        return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    return sample_launch(batch, P, K, first, gkey, iters, assign_all, cut_all, best_assign, best_cut, best_iter, stream,
                         node_cost);
}

extern "C" int gmc_kway_decode_sample_seeded_f32(const gmc_batch *batch, const float *P, int32_t K,
                                                 const uint64_t *gkey, int32_t iters, int8_t *assign_all,
                                                 float *cut_all, int32_t *best_assign, float *best_cut,
                                                 int32_t *best_iter, gmc_stream_t stream) {
    return gmc_kway_decode_sample_seeded_t_f32(batch, P, K, 1, gkey, iters, assign_all, cut_all, best_assign, best_cut,
                                               best_iter, stream);
}

extern "C" int gmc_kway_decode_sample_seeded_t_f32(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals,
                                                   const uint64_t *gkey, int32_t iters, int8_t *assign_all,
                                                   float *cut_all, int32_t *best_assign, float *best_cut,
                                                   int32_t *best_iter, gmc_stream_t stream) {
    return gmc_kway_decode_sample_seeded_c_f32(batch, P, K, terminals, nullptr, gkey, iters, assign_all, cut_all,
                                               best_assign, best_cut, best_iter, stream);
}

extern "C" int gmc_kway_decode_sample_seeded_c_f32(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals,
                                                   const float *node_cost, const uint64_t *gkey, int32_t iters,
                                                   int8_t *assign_all, float *cut_all, int32_t *best_assign,
                                                   float *best_cut, int32_t *best_iter, gmc_stream_t stream) {
    return kway_sample_seeded(batch, P, K, terminals, node_cost, gkey, iters, assign_all, cut_all, best_assign, best_cut,
                              best_iter, stream);
}

extern "C" int gmc_refine_anneal_staged(const gmc_batch *batch) {
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (batch->n_max < 3 || batch->n_max > GMC_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    return gmc::anneal_layout(batch).staged;
}

extern "C" int gmc_refine_anneal_f32(const gmc_batch *batch, const int32_t *order, const int32_t *cgoff,
                                     const int32_t *cptr, int32_t cands, int8_t *assign, const float *inv_temp,
                                     int32_t anneal_sweeps, const float *levels, uint64_t seed,
                                     int32_t max_descent_sweeps, float *cut_all, int32_t *best_assign, float *best_cut,
                                     int32_t *best_idx, int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !assign || !cut_all || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (cands < 1 || anneal_sweeps < 0 || anneal_sweeps >= (1 << 20) || max_descent_sweeps < 0 || batch->B < 0)
        return GMC_ERR_SHAPE;
    if (anneal_sweeps > 0 && (!inv_temp || !levels)) return GMC_ERR_NULL;
    if (batch->B > 0 && (batch->n_max < 3 || batch->n_max > GMC_MAX_GRAPH_NODES)) return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    return anneal_launch(batch, 3, 3, order, cgoff, cptr, cands, assign, inv_temp, anneal_sweeps, levels, seed,
                         max_descent_sweeps, cut_all, best_assign, best_cut, best_idx, snap_sweep, sweeps, stream);
}

// what gmc_kway_refine_anneal_f32 and its _t twin do (terminals: 0 or 1); node_cost: the _c twin's, or NULL
static int kway_refine_anneal(const gmc_batch *batch, int32_t K, int32_t terminals, const float *node_cost,
                              const int32_t *order,
                              const int32_t *cgoff, const int32_t *cptr, int32_t cands, int8_t *assign,
                              const float *inv_temp, int32_t anneal_sweeps, const float *levels, uint64_t seed,
                              int32_t max_descent_sweeps, float *cut_all, int32_t *best_assign, float *best_cut,
                              int32_t *best_idx, int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !assign || !cut_all || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (cands < 1 || anneal_sweeps < 0 || anneal_sweeps >= (1 << 20) || max_descent_sweeps < 0 || batch->B < 0 ||
        (terminals != 0 && terminals != 1))
        return GMC_ERR_SHAPE;
    if (anneal_sweeps > 0 && (!inv_temp || !levels)) return GMC_ERR_NULL;
    const int first = terminals ? K : 0;
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || batch->n_max > GMC_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    return anneal_launch(batch, K, first, order, cgoff, cptr, cands, assign, inv_temp, anneal_sweeps, levels, seed,
                         max_descent_sweeps, cut_all, best_assign, best_cut, best_idx, snap_sweep, sweeps, stream,
                         node_cost);
}

extern "C" int gmc_kway_refine_anneal_f32(const gmc_batch *batch, int32_t K, const int32_t *order,
                                          const int32_t *cgoff, const int32_t *cptr, int32_t cands, int8_t *assign,
                                          const float *inv_temp, int32_t anneal_sweeps, const float *levels,
                                          uint64_t seed, int32_t max_descent_sweeps, float *cut_all,
                                          int32_t *best_assign, float *best_cut, int32_t *best_idx,
                                          int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    return gmc_kway_refine_anneal_t_f32(batch, K, 1, order, cgoff, cptr, cands, assign, inv_temp, anneal_sweeps, levels,
                                        seed, max_descent_sweeps, cut_all, best_assign, best_cut, best_idx, snap_sweep,
                                        sweeps, stream);
}

extern "C" int gmc_kway_refine_anneal_t_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const int32_t *order,
                                            const int32_t *cgoff, const int32_t *cptr, int32_t cands, int8_t *assign,
                                            const float *inv_temp, int32_t anneal_sweeps, const float *levels,
                                            uint64_t seed, int32_t max_descent_sweeps, float *cut_all,
                                            int32_t *best_assign, float *best_cut, int32_t *best_idx,
                                            int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    return gmc_kway_refine_anneal_c_f32(batch, K, terminals, nullptr, order, cgoff, cptr, cands, assign, inv_temp,
                                        anneal_sweeps, levels, seed, max_descent_sweeps, cut_all, best_assign, best_cut,
                                        best_idx, snap_sweep, sweeps, stream);
}

extern "C" int gmc_kway_refine_anneal_c_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const float *node_cost,
                                            const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                                            int32_t cands, int8_t *assign, const float *inv_temp, int32_t anneal_sweeps,
                                            const float *levels, uint64_t seed, int32_t max_descent_sweeps,
                                            float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_idx,
                                            int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    return kway_refine_anneal(batch, K, terminals, node_cost, order, cgoff, cptr, cands, assign, inv_temp, anneal_sweeps,
                              levels, seed, max_descent_sweeps, cut_all, best_assign, best_cut, best_idx, snap_sweep,
                              sweeps, stream);
}
