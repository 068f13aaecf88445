// The node visit shared by the local search (refine.hip), the annealing (anneal.hip), the rounding's descent (round.hip)
// and the K-class search (kway_search.hip): the class sums of a node and the local search's move rule, one definition so
// that the kernels cannot drift apart.
#pragma once
#include "gmc_common.h"

namespace gmc {

// W0, W1, W2 of local node l: fp32 sums, in the CSR order of its row, of the weights of its edges to neighbours of class
// 0, 1 and 2 (self-loops skipped).  Three sums chosen by compares (an indexed private array would live in scratch); a
// class byte outside 0..2 adds to none of them.  rp[l] .. rp[l + 1] are the row's edges in col / vals (NULL: all ones).
template <class RP, class COL>
__device__ __forceinline__ void class_sums(const RP *rp, const COL *col, const float *vals, const unsigned char *sa,
                                           int l, float &w0, float &w1, float &w2) {
    w0 = 0.f; w1 = 0.f; w2 = 0.f;
    const int e1 = rp[l + 1];
    for (int e = rp[l]; e < e1; ++e) {
        const int u = col[e];
        if (u == l) continue;
        const float w = vals ? vals[e] : 1.0f;
        const int cu = sa[u];
        w0 += cu == 0 ? w : 0.f;
        w1 += cu == 1 ? w : 0.f;
        w2 += cu == 2 ? w : 0.f;
    }
}

// The local search's rule for a node of class byte c: kk = the class of the smallest W (lowest index on ties); true iff
// the node moves there, i.e. W[kk] < W[c] (a byte outside 0..2 has W[c] = inf: such a node always moves).
__device__ __forceinline__ bool local_move(float w0, float w1, float w2, int c, int &kk) {
    const float wc = c == 0 ? w0 : c == 1 ? w1 : c == 2 ? w2 : __builtin_inff();
    kk = 0;
    float wk = w0;
    if (w1 < wk) { kk = 1; wk = w1; }
    if (w2 < wk) { kk = 2; wk = w2; }
    return wk < wc;
}

// K floats in registers: every index below is a constant once the loops are unrolled (an index that is not would put
// the array into scratch)
template <int K>
struct Sums {
    float m[K];
};

// class_sums at K classes: W_k = sum of the weights of the edges of local row l to neighbours of class k, fp32, in the
// CSR order of the row, self-loops skipped, a class byte outside 0..K-1 adding to none (K = 3: class_sums, the same
// operations in the same order).  cls[u] is the class byte of node u: a pointer, or a view with an operator[]
// (large_search.hip keeps the bytes of one candidate a stride apart).
template <int K, class RP, class COL, class CLS>
__device__ __forceinline__ Sums<K> class_sums_k(const RP *rp, const COL *col, const float *vals, const CLS &cls,
                                                int l) {
    Sums<K> s;
#pragma unroll
    for (int k = 0; k < K; ++k) s.m[k] = 0.f;
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

}  // namespace gmc
