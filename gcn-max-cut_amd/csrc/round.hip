// Rounding of node probabilities by conditional expectations, followed by the local search's descent (an extension:
// the reference decodes by argmax or by random samples, TestingNeuralNetwork.py:66-122).  The algorithm is stated in
// include/gcnmaxcut.h (gmc_round_conditional_f32); the colouring and the (colour, id) order are those of refine.hip
// with the movable nodes starting at K (gmc_round_order_host), the descent is the sweep loop refine.hip and the
// annealing run (move_body.h's descent_sweeps, refine.hip's being its K = 3), the score is cut_body.h's.
//
// One 256-thread workgroup per graph, K a template argument.  The workgroup's LDS, sized by n_max:
//
//   q      [n_max][K] float   the state: a node's row of P until it is rounded, e_class afterwards (terminals: from
//                             the start).  A node's K values are contiguous, so a neighbour costs one read of K floats.
//   cls    [n_max] byte       the class bytes: what the descent reads (the state is one-hot by then, so the sums over
//                             q are sums of the weights whose neighbour holds the class: one byte per neighbour instead
//                             of K floats, and at K = 3 literally move_body.h's sums), what block_cut scores, the output.
//
// (4K + 1) * n_max bytes: 33 * n_max at K = 8, beyond 64 KiB from n_max = 1986 (the launch raises the kernel's
// dynamic-LDS limit then), 132 KiB at n_max = GMC_MAX_GRAPH_NODES.
#include "gmc_common.h"
#include "cut_body.h"
#include "move_body.h"
#include "round_body.h"
#include "anneal_layout.h"

namespace {

using gmc::Sums;
using gmc::smallest;       // the pick of the smallest sum, and the descent over the class bytes: move_body.h
using gmc::state_sums;     // the sums over the state and a row's share of the expected cut: round_body.h
using gmc::expected_row;

struct RoundArgs {
    gmc_batch b;
    const float *P;          // [R][K]
    const int *order;        // movable rows of each graph, sorted by (colour, id)   (gmc_round_order_host)
    const int *cgoff;        // [B+1] first class pointer of each graph
    const int *cptr;         // class k of graph g: order[cptr[cgoff[g]+k] .. cptr[cgoff[g]+k+1])
    int max_descent_sweeps;
    int first;               // first movable local id: K with terminals, 0 without
    signed char *assign;     // [R]
    float *cut;              // [B]
    float *expected;         // [B] or NULL
    int *sweeps;             // [B] or NULL
    const float *node_cost;  // [R][K] by batch row or NULL (gmc_round_conditional_c_f32)
};

// Two kernels over one body text (round_kernel_body.inc; anneal_kernel_body.inc says why text): round_conditional_kernel<K>
// is the launch without per-node class costs and keeps its name and its code, round_conditional_cost_kernel<K> is the
// launch with them (a.node_cost != NULL).
template <int K>
__global__ __launch_bounds__(256) void round_conditional_kernel(RoundArgs a) {
#define GMC_COST false
#include "round_kernel_body.inc"
#undef GMC_COST
}
template <int K>
__global__ __launch_bounds__(256) void round_conditional_cost_kernel(RoundArgs a) {
#define GMC_COST true
#include "round_kernel_body.inc"
#undef GMC_COST
}

template <int K>
int round_launch(const RoundArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.b.n_max * (K * sizeof(float) + 1);
    const void *kernel = a.node_cost ? reinterpret_cast<const void *>(round_conditional_cost_kernel<K>)
                                     : reinterpret_cast<const void *>(round_conditional_kernel<K>);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    GmcProbeScope probe(GMC_K_REFINE, st);
    if (a.node_cost) hipLaunchKernelGGL((round_conditional_cost_kernel<K>), dim3(a.b.B), dim3(256), lds, st, a);
    else hipLaunchKernelGGL((round_conditional_kernel<K>), dim3(a.b.B), dim3(256), lds, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

// what the entry points do: the checks in the documented order, then the launch (terminals: 0 or 1; node_cost: the _c
// twin's, or NULL)
static int round_conditional(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals, const float *node_cost,
                             const int32_t *order,
                             const int32_t *cgoff, const int32_t *cptr, int32_t max_descent_sweeps, int8_t *assign,
                             float *cut, float *expected, int32_t *sweeps, gmc_stream_t stream) {
    if (!batch || !P || !order || !cgoff || !cptr || !assign || !cut) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (max_descent_sweeps < 0 || batch->B < 0 || (terminals != 0 && terminals != 1)) return GMC_ERR_SHAPE;
    const int first = terminals ? K : 0;
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || batch->n_max > GMC_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const RoundArgs a{*batch, P, order, cgoff, cptr, max_descent_sweeps, first,
                      reinterpret_cast<signed char *>(assign), cut, expected, sweeps, node_cost};
    GMC_KWAY_DISPATCH(K, return round_launch<KK>(a, st));
    return GMC_OK;
}

extern "C" int gmc_round_conditional_f32(const gmc_batch *batch, const float *P, int32_t K, const int32_t *order,
                                         const int32_t *cgoff, const int32_t *cptr, int32_t max_descent_sweeps,
                                         int8_t *assign, float *cut, float *expected, int32_t *sweeps,
                                         gmc_stream_t stream) {
    return gmc_round_conditional_t_f32(batch, P, K, 1, order, cgoff, cptr, max_descent_sweeps, assign, cut, expected,
                                       sweeps, stream);
}

extern "C" int gmc_round_conditional_t_f32(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals,
                                           const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                                           int32_t max_descent_sweeps, int8_t *assign, float *cut, float *expected,
                                           int32_t *sweeps, gmc_stream_t stream) {
    return gmc_round_conditional_c_f32(batch, P, K, terminals, nullptr, order, cgoff, cptr, max_descent_sweeps, assign,
                                       cut, expected, sweeps, stream);
}

extern "C" int gmc_round_conditional_c_f32(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals,
                                           const float *node_cost, const int32_t *order, const int32_t *cgoff,
                                           const int32_t *cptr, int32_t max_descent_sweeps, int8_t *assign, float *cut,
                                           float *expected, int32_t *sweeps, gmc_stream_t stream) {
    return round_conditional(batch, P, K, terminals, node_cost, order, cgoff, cptr, max_descent_sweeps, assign, cut,
                             expected, sweeps, stream);
}
