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
};

template <int K>
__global__ __launch_bounds__(256) void round_conditional_kernel(RoundArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    const int g = blockIdx.x;
    const int r0 = a.b.goff[g];
    const int n = a.b.goff[g + 1] - r0;
    const int first = a.first;
    if (n > a.b.n_max || n < first) return;   // (a batch that contradicts its own n_max: the LDS is sized by it)
    float *q = reinterpret_cast<float *>(lds);
    unsigned char *cls = lds + (size_t)a.b.n_max * K * sizeof(float);
    const int *rp = a.b.rowptr + r0;
    const int *col = a.b.lcol;
    const float *vals = a.b.vals;
    // state: terminals (l < first) e_l (their rows of P are not read), every other node its row of P
    const float *Pg = a.P + (long)r0 * K;
    for (int i = threadIdx.x; i < n * K; i += blockDim.x) {
        const int l = i / K, k = i - l * K;
        q[i] = l < first ? (l == k ? 1.0f : 0.0f) : Pg[i];
    }
    for (int l = threadIdx.x; l < n; l += blockDim.x) cls[l] = (unsigned char)(l < first ? l : 0);
    __syncthreads();
    const gmc::FloatState<K> state{q};
    if (a.expected) {   // workgroup-uniform
        float acc = 0.f;
        for (int l = threadIdx.x; l < n; l += blockDim.x) acc += expected_row<K>(rp, col, vals, state, l);
        acc = gmc::wave_sum(acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        if (threadIdx.x == 0) a.expected[g] = (((red[0] + red[1]) + red[2]) + red[3]) * 0.5f;
        __syncthreads();   // every row has read the unrounded state, thread 0 has read red
    }
    const int k0 = a.cgoff[g];
    const int classes = a.cgoff[g + 1] - k0 - 1;
    // rounding: one visit of every movable node, class by class
    for (int k = 0; k < classes; ++k) {
        const int hi = a.cptr[k0 + k + 1];
        for (int i = a.cptr[k0 + k] + threadIdx.x; i < hi; i += blockDim.x) {
            const int l = a.order[i] - r0;
            if ((unsigned)(l - first) >= (unsigned)(n - first)) continue;   // not a movable row: never touch LDS for it
            const Sums<K> s = state_sums<K>(rp, col, vals, state, l);
            float wk;
            const int kk = smallest<K>(s, wk);
#pragma unroll
            for (int c = 0; c < K; ++c) q[l * K + c] = c == kk ? 1.0f : 0.0f;
            cls[l] = (unsigned char)kk;
        }
        __syncthreads();   // the next class, the descent or the cut count reads what this one wrote
    }
    // descent: the local search's sweeps at K classes over the class bytes
    const gmc::GlobalCsr csr{rp, col, vals, a.order, r0, first};
    const int sw = gmc::descent_sweeps<K>(csr, a.cptr, k0, classes, cls, n, a.max_descent_sweeps);
    signed char *as = a.assign + r0;
    for (int l = threadIdx.x; l < n; l += blockDim.x) as[l] = (signed char)cls[l];
    const float cut = gmc::block_cut(a.b, cls, r0, n, red);   // scored as gmc_refine_local_f32 scores
    if (threadIdx.x == 0) {
        a.cut[g] = cut;
        if (a.sweeps) a.sweeps[g] = sw;
    }
}

template <int K>
int round_launch(const RoundArgs &a, hipStream_t st) {
    const size_t lds = (size_t)a.b.n_max * (K * sizeof(float) + 1);
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(round_conditional_kernel<K>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    GmcProbeScope probe(GMC_K_REFINE, st);
    hipLaunchKernelGGL((round_conditional_kernel<K>), dim3(a.b.B), dim3(256), lds, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

// what both entry points do: the checks in the documented order, then the launch (terminals: 0 or 1)
static int round_conditional(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals, const int32_t *order,
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
                      reinterpret_cast<signed char *>(assign), cut, expected, sweeps};
    GMC_KWAY_DISPATCH(K, return round_launch<KK>(a, st));
    return GMC_OK;
}

extern "C" int gmc_round_conditional_f32(const gmc_batch *batch, const float *P, int32_t K, const int32_t *order,
                                         const int32_t *cgoff, const int32_t *cptr, int32_t max_descent_sweeps,
                                         int8_t *assign, float *cut, float *expected, int32_t *sweeps,
                                         gmc_stream_t stream) {
    return round_conditional(batch, P, K, 1, order, cgoff, cptr, max_descent_sweeps, assign, cut, expected, sweeps,
                             stream);
}

extern "C" int gmc_round_conditional_t_f32(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals,
                                           const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                                           int32_t max_descent_sweeps, int8_t *assign, float *cut, float *expected,
                                           int32_t *sweeps, gmc_stream_t stream) {
    return round_conditional(batch, P, K, terminals, order, cgoff, cptr, max_descent_sweeps, assign, cut, expected,
                             sweeps, stream);
}
