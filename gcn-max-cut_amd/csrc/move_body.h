// The node visit shared by the local search (refine.hip) and the annealing (anneal.hip): the class sums of a node and
// the local search's move rule, one definition so that the two kernels cannot drift apart.
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

}  // namespace gmc
