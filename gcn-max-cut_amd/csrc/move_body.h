// The node visit shared by the local search (refine.hip), the annealing and the seeded search at K = 2..8 classes
// (anneal_body.h, kway_search.hip, kway_evolve.hip; the 3-class entry points are their K = 3), the rounding's descent
// (round.hip) and the kernels for large graphs (large_round.hip, large_search.hip): the class sums of a node, the move
// rules, and the descent's sweep loop of the one-workgroup kernels - one definition each, so that the kernels cannot
// drift apart.
#pragma once
#include "gmc_common.h"

namespace gmc {

// K floats in registers: every index below is a constant once the loops are unrolled (an index that is not would put
// the array into scratch)
template <int K>
struct Sums {
    float m[K];
};

// W_k = sum of the weights of the edges of local row l to neighbours of class k, fp32, in the CSR order of the row,
// self-loops skipped, a class byte outside 0..K-1 adding to none.  K sums chosen by compares (an indexed private array
// would live in scratch).  rp[l] .. rp[l + 1] are the row's edges in col / vals (NULL: all ones).  cls[u] is the class
// byte of node u: a pointer, or a view with an operator[] (large_search.hip keeps the bytes of one candidate a stride
// apart).  nc: the per-node class costs of the graph's rows, [n][K] by local id (the caller's node_cost + r0 * K), or
// NULL; with it W_k starts from nc[l][k] instead of +0 (the _c entry points of include/gcnmaxcut.h) and nothing else
// changes - the K loads come from global memory, once per visit.
template <int K, class RP, class COL, class CLS>
__device__ __forceinline__ Sums<K> class_sums_k(const RP *rp, const COL *col, const float *vals, const CLS &cls,
                                                int l, const float *nc = nullptr) {
    Sums<K> s;
#pragma unroll
    for (int k = 0; k < K; ++k) s.m[k] = nc ? nc[(long)l * K + k] : 0.f;
    const int e1 = rp[l + 1];
    for (int e = rp[l]; e < e1; ++e) {
        const int u = col[e];
        if (u == l) continue;
        const float w = vals ? vals[e] : 1.0f;
        const int cu = cls[u];
#pragma unroll
        for (int k = 0; k < K; ++k) s.m[k] += cu == k ? w : 0.f;
    }
    return s;
}

// the class of the smallest sum, the lowest index on ties; wk = that sum
template <int K>
__device__ __forceinline__ int smallest(const Sums<K> &s, float &wk) {
    int kk = 0;
    wk = s.m[0];
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (s.m[k] < wk) { kk = k; wk = s.m[k]; }
    return kk;
}

// the sum of class byte c, +inf for a byte outside 0..K-1
template <int K>
__device__ __forceinline__ float own_sum_or_inf(const Sums<K> &s, int c) {
    float wc = __builtin_inff();
#pragma unroll
    for (int j = 0; j < K; ++j) wc = c == j ? s.m[j] : wc;
    return wc;
}

// the class of the smallest sum among the classes other than c, the lowest index on ties; wk = that sum (a byte c
// outside 0..K-1 excludes none: smallest)
template <int K>
__device__ __forceinline__ int smallest_other(const Sums<K> &s, int c, float &wk) {
    int kk = c == 0 ? 1 : 0;
    wk = c == 0 ? s.m[1] : s.m[0];
#pragma unroll
    for (int k = 1; k < K; ++k)
        if (k != c && s.m[k] < wk) { kk = k; wk = s.m[k]; }
    return kk;
}

// One annealing visit of a node with sums w and class byte c (gmc_kway_refine_anneal_f32's rule): kk = the class of the
// smallest sum among the classes other than c; true iff the node moves there, i.e. delta = W[kk] - W[c] < 0 or
// delta * inv_t <= lv[h >> 54], h the node's hash.  A byte of no class equals no k: own sum +inf, the smallest of all K
// sums as the target, taken unconditionally (delta = 0 - inf); no branch, so the sums stay in registers.
template <int K>
__device__ __forceinline__ bool anneal_move(const Sums<K> &w, int c, float inv_t, const float *lv,
                                            unsigned long long h, int &kk) {
    const bool has_class = (unsigned)c < (unsigned)K;
    const float wc = own_sum_or_inf<K>(w, c);
    float wk;
    kk = smallest_other<K>(w, c, wk);
    wk = has_class ? wk : 0.f;
    const float delta = wk - wc;
    return delta < 0.f || delta * inv_t <= lv[h >> 54];
}

// One descent visit of local node l, the local search's rule: the node moves to the class kk of the smallest of its K
// sums (lowest index on ties) iff W[kk] < W[own]; a byte of no class has W[own] = +inf, so such a node always moves.
// g: a graph's CSR as one of anneal_layout.h's accessors (rp, col, vals); nc: class_sums_k's; true iff the node moved.
// The +inf is spelled as a test of the byte beside the compare, not as one more select in front of the own-sum chain:
// the visit is the critical path of a colour step, and at K = 3 that select made the rounding's descent 3 % slower.
template <int K, class G>
__device__ __forceinline__ bool descent_visit(const G &g, unsigned char *cls, int l, const float *nc = nullptr) {
    const Sums<K> s = class_sums_k<K>(g.rp, g.col, g.vals, cls, l, nc);
    const int c = cls[l];
    float wc = s.m[0];
#pragma unroll
    for (int j = 1; j < K; ++j) wc = c == j ? s.m[j] : wc;
    float wk;
    const int kk = smallest<K>(s, wk);
    if (wk < wc || (unsigned)c >= (unsigned)K) {
        cls[l] = (unsigned char)kk;
        return true;
    }
    return false;
}

// The descent of one 256-thread workgroup over the class bytes cls (LDS) of a graph of n nodes: sweeps over the colour
// classes cptr[k0] .. cptr[k0 + classes] of the (colour, id) order behind g.node(), one thread per node of the current
// class, a barrier between classes, a workgroup-wide OR closing every sweep; stops after a sweep that moved nothing or
// after max_sweeps.  An entry of the order that is not a movable row of this graph (a terminal l < first, or l >= n; first = K with
// terminals, 0 without: a run-time value behind g.movable(), so both serve from one instantiation) is
// never visited and never touches LDS.  Every thread must call it with cls published; on return every thread may read
// cls.  Returns the sweeps run, the last of them the one that moved nothing when the descent converged.  nc: the graph's
// per-node class costs as class_sums_k takes them, or NULL.
template <int K, class G>
__device__ __forceinline__ int descent_sweeps(const G &g, const int *cptr, int k0, int classes, unsigned char *cls,
                                              int n, int max_sweeps, const float *nc = nullptr) {
    // blockDim.x is read once, ahead of the sweeps: read inside the loop it becomes a vector load on every colour
    // step's critical path (the rounding at K = 3 ran 4.5 % slower; DESIGN.md section 23 has this and the other forms tried)
    const int threads = blockDim.x;
    int s = 0;
    while (s < max_sweeps) {
        ++s;
        int moved = 0;
        for (int k = 0; k < classes; ++k) {
            const int hi = cptr[k0 + k + 1];
            for (int i = cptr[k0 + k] + threadIdx.x; i < hi; i += threads) {
                const int l = g.node(i);
                if (!g.movable(l, n)) continue;
                if (descent_visit<K>(g, cls, l, nc)) moved = 1;
            }
            if (k + 1 < classes) __syncthreads();
        }
        if (!__syncthreads_or(moved)) break;
    }
    return s;
}

}  // namespace gmc
