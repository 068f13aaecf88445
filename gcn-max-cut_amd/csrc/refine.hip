// Single-node-move local search over decoded partitions (an extension: the reference stops at the best of its random
// samples, TestingNeuralNetwork.py:66-98).
//
// Per graph of the batch (local ids 0..n-1): nodes 0, 1, 2 never move (override_fixed_nodes, TrainingNeural.py:87-94).
// The movable nodes 3..n-1 are coloured first-fit in increasing id against their movable neighbours of smaller id
// (gmc_refine_order_host, on the host), so every colour class is an independent set among movable nodes.  A sweep
// visits the classes in increasing colour; each node v of a class sums, in fp32 and in the CSR order of its row, the
// weights of its edges to classes 0, 1 and 2 (self-loops skipped) into W0, W1, W2, and moves to the class k of the
// smallest W (lowest index on ties) iff W[k] < W[class(v)].  No two nodes of a class are adjacent, so the nodes of a
// class move in parallel and the result is that of a sequential sweep in (colour, id) order.  Sweeps stop after one
// that moves nothing, or after max_sweeps.  The refined candidates are then scored and picked by the sampler's own
// code (cut_body.h).
//
// One workgroup per (candidate, graph): the candidate's classes live in LDS as bytes (n_max <= 4096 -> 4 KB), one
// thread per node of the current class, a barrier between classes, a workgroup-wide OR closing every sweep: the
// descent every one-workgroup search ends with (move_body.h's descent_sweeps), here at K = 3 over the batch's arrays
// and with nothing else in LDS - no level table, no best state, no staged graph.
#include "gmc_common.h"
#include "cut_body.h"
#include "move_body.h"
#include "anneal_layout.h"

#include <vector>

namespace {

struct RefineArgs {
    gmc_batch b;
    const int *order;        // movable rows of each graph, sorted by (colour, id)
    const int *cgoff;        // [B+1] first class pointer of each graph
    const int *cptr;         // class k of graph g: order[cptr[cgoff[g]+k] .. cptr[cgoff[g]+k+1])
    int cands;
    int max_sweeps;
    signed char *assign;     // [cands][R], in/out
    float *cut_all;          // [B][cands]
    int *sweeps;             // [B][cands] or NULL
};

__global__ __launch_bounds__(256) void refine_local_kernel(RefineArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sa[];
    __shared__ float red[4];
    const int cand = blockIdx.x, g = blockIdx.y;
    const int r0 = a.b.goff[g];
    const int n = a.b.goff[g + 1] - r0;
    if (n > a.b.n_max || n < 3) return;   // (the LDS is sized by n_max; a graph without its 3 terminals is skipped)
    signed char *as = a.assign + (long)cand * a.b.R + r0;
    for (int l = threadIdx.x; l < n; l += blockDim.x) sa[l] = (unsigned char)as[l];
    __syncthreads();
    const int k0 = a.cgoff[g];
    const int classes = a.cgoff[g + 1] - k0 - 1;
    const gmc::GlobalCsr csr{a.b.rowptr + r0, a.b.lcol, a.b.vals, a.order, r0, 3};
    const int s = gmc::descent_sweeps<3>(csr, a.cptr, k0, classes, sa, n, a.max_sweeps);
    for (int l = threadIdx.x; l < n; l += blockDim.x) as[l] = (signed char)sa[l];
    const float cut = gmc::block_cut(a.b, sa, r0, n, red);
    if (threadIdx.x == 0) {
        a.cut_all[(long)g * a.cands + cand] = cut;
        if (a.sweeps) a.sweeps[(long)g * a.cands + cand] = s;
    }
}

__global__ __launch_bounds__(256) void refine_pick_kernel(gmc::PickArgs a) {
    const int n = a.b.goff[blockIdx.x + 1] - a.b.goff[blockIdx.x];
    if (n > a.b.n_max || n < 3) return;   // workgroup-uniform: the graphs the search skipped
    gmc::pick_best(a);
}

}  // namespace

// HOST routine (all pointers are host pointers): first-fit colouring of every graph's movable nodes first..n-1 and the
// (colour, id) order the kernels walk.  cptr_cap < R + B is refused before anything is written.  One body for
// gmc_refine_order_host (first = 3), gmc_round_order_host (first = K), gmc_large_round_order_host (first = K, graphs of
// up to max_nodes = GMC_LARGE_MAX_GRAPH_NODES nodes) and gmc_order_host_t (first = K or 0, graphs as large).  max_classes (optional): the largest class count of any graph.
static int order_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol, int first,
                      int max_nodes, int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap,
                      int32_t *max_classes = nullptr) {
    if (!goff || !rowptr || !lcol || !order || !cgoff || !cptr) return GMC_ERR_NULL;
    if (B < 0) return GMC_ERR_SHAPE;
    int n_max = 0;
    for (int g = 0; g < B; ++g) {
        const int n = goff[g + 1] - goff[g];
        if (n < first || n > max_nodes) return GMC_ERR_GRAPH_SIZE;
        n_max = n > n_max ? n : n_max;
    }
    if ((long long)cptr_cap < (long long)goff[B] + B) return GMC_ERR_SHAPE;
    std::vector<int> colour(n_max), mark, count;
    int pos = 0, kp = 0, most = 0;
    for (int g = 0; g < B; ++g) {
        const int r0 = goff[g], n = goff[g + 1] - r0;
        int ncol = 0;
        mark.clear();   // mark[c] == v: colour c is taken at node v; stamps of the previous graph must not survive
        for (int v = first; v < n; ++v) {
            for (int e = rowptr[r0 + v]; e < rowptr[r0 + v + 1]; ++e) {
                const int u = lcol[e];
                if (u >= first && u < v) mark[colour[u]] = v;   // colours taken by movable neighbours of smaller id
            }
            int c = 0;
            while (c < ncol && mark[c] == v) ++c;
            if (c == ncol) {
                ++ncol;
                mark.push_back(-1);
            }
            colour[v] = c;
        }
        most = ncol > most ? ncol : most;
        count.assign(ncol, 0);
        for (int v = first; v < n; ++v) ++count[colour[v]];
        cgoff[g] = kp;
        cptr[kp++] = pos;
        for (int c = 0; c < ncol; ++c) {   // count[c] becomes the next free place of class c
            const int m = count[c];
            count[c] = pos;
            pos += m;
            cptr[kp++] = pos;
        }
        for (int v = first; v < n; ++v) order[count[colour[v]]++] = r0 + v;   // increasing id inside each class
    }
    cgoff[B] = kp;
    if (max_classes) *max_classes = most;
    return GMC_OK;
}

extern "C" int gmc_refine_order_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol,
                                     int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap) {
    return order_host(B, goff, rowptr, lcol, 3, GMC_MAX_GRAPH_NODES, order, cgoff, cptr, cptr_cap);
}

// the same colouring with the movable nodes starting at K: the order gmc_round_conditional_f32 (round.hip) walks
extern "C" int gmc_round_order_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol,
                                    int32_t K, int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap) {
    if (!goff || !rowptr || !lcol || !order || !cgoff || !cptr) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    return order_host(B, goff, rowptr, lcol, K, GMC_MAX_GRAPH_NODES, order, cgoff, cptr, cptr_cap);
}

// gmc_round_order_host for graphs of up to GMC_LARGE_MAX_GRAPH_NODES nodes: the order the kernels of large_round.hip walk
extern "C" int gmc_large_round_order_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol,
                                          int32_t K, int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap,
                                          int32_t *max_classes) {
    if (!goff || !rowptr || !lcol || !order || !cgoff || !cptr || !max_classes) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    return order_host(B, goff, rowptr, lcol, K, GMC_LARGE_MAX_GRAPH_NODES, order, cgoff, cptr, cptr_cap, max_classes);
}

// gmc_large_round_order_host with the terminals optional: first = terminals ? K : 0, so without them every node is
// coloured and `order` holds all R rows
extern "C" int gmc_order_host_t(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol, int32_t K,
                                int32_t terminals, int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap,
                                int32_t *max_classes) {
    if (!goff || !rowptr || !lcol || !order || !cgoff || !cptr || !max_classes) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (terminals != 0 && terminals != 1) return GMC_ERR_SHAPE;
    return order_host(B, goff, rowptr, lcol, terminals ? K : 0, GMC_LARGE_MAX_GRAPH_NODES, order, cgoff, cptr, cptr_cap,
                      max_classes);
}

extern "C" int gmc_refine_local_f32(const gmc_batch *batch, const int32_t *order, const int32_t *cgoff,
                                    const int32_t *cptr, int32_t cands, int8_t *assign, int32_t max_sweeps,
                                    float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_idx,
                                    int32_t *sweeps, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !assign || !cut_all || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (cands < 1 || max_sweeps < 0 || batch->B < 0) return GMC_ERR_SHAPE;
    if (batch->B > 0 && (batch->n_max < 3 || batch->n_max > GMC_MAX_GRAPH_NODES)) return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    RefineArgs a{*batch, order, cgoff, cptr, cands, max_sweeps, reinterpret_cast<signed char *>(assign), cut_all, sweeps};
    {
        GmcProbeScope probe(GMC_K_REFINE, st);
        hipLaunchKernelGGL(refine_local_kernel, dim3(cands, batch->B), dim3(256), (size_t)batch->n_max, st, a);
        GMC_LAUNCH_CHECK();
    }
    gmc::PickArgs p{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign, best_cut, best_idx};
    hipLaunchKernelGGL(refine_pick_kernel, dim3(batch->B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
