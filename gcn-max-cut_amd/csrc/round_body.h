// The two row sums of the rounding by conditional expectations, shared by its one-workgroup kernel (round.hip: the state
// in LDS, rows by local id) and its multi-workgroup kernels (large_round.hip: the state in global memory, rows by batch
// row id): one definition, so that the two cannot drift apart - the second promises the first's bytes.
//
// The state is read through an accessor Q: q.load(u, v) fills v[0..K-1] with the state row of node u.  rp[l] .. rp[l + 1]
// are the edges of row l in col (neighbour ids in the accessor's numbering, l itself marking a self-loop) and vals
// (NULL: all ones).
#pragma once
#include "move_body.h"

namespace gmc {

// the state as [n][K] floats (round.hip keeps them in LDS)
template <int K>
struct FloatState {
    const float *q;
    __device__ __forceinline__ void load(int u, float (&v)[K]) const {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = q[u * K + k];
    }
};

// M_k = sum over the edges of row l, CSR order, self-loops skipped, of w_e * q_u[k], from +0.  Product and sum are
// rounded separately: hipcc contracts a * b + c into one fused multiply-add unless told not to.  nc: the per-node class
// costs of the rows the CSR numbers ([.][K], row l at nc + l * K) or NULL; with it M_k starts from nc[l][k] instead of +0.
template <int K, class RP, class COL, class Q>
__device__ __forceinline__ Sums<K> state_sums(const RP *rp, const COL *col, const float *vals, const Q &q, int l,
                                              const float *nc = nullptr) {
#pragma clang fp contract(off)
    Sums<K> s;
#pragma unroll
    for (int k = 0; k < K; ++k) s.m[k] = nc ? nc[(long)l * K + k] : 0.f;
    const int e1 = rp[l + 1];
    for (int e = rp[l]; e < e1; ++e) {
        const int u = col[e];
        if (u == l) continue;
        const float w = vals ? vals[e] : 1.0f;
        float qu[K];
        q.load(u, qu);
#pragma unroll
        for (int k = 0; k < K; ++k) {
            const float t = w * qu[k];
            s.m[k] = s.m[k] + t;
        }
    }
    return s;
}

// the node's share of the expected cut: sum over its edges (self-loops skipped) of w_e * (1 - q_u . q_l)
template <int K, class RP, class COL, class Q>
__device__ __forceinline__ float expected_row(const RP *rp, const COL *col, const float *vals, const Q &q, int l) {
#pragma clang fp contract(off)
    float ql[K];
    q.load(l, ql);
    float acc = 0.f;
    const int e1 = rp[l + 1];
    for (int e = rp[l]; e < e1; ++e) {
        const int u = col[e];
        if (u == l) continue;
        const float w = vals ? vals[e] : 1.0f;
        float qu[K];
        q.load(u, qu);
        float dot = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) dot += qu[k] * ql[k];
        acc += w * (1.0f - dot);
    }
    return acc;
}

// the node's share of the expected cost: nc[l] . q_l, the products added in ascending k from +0, product and sum
// rounded separately
template <int K, class Q>
__device__ __forceinline__ float expected_cost_row(const float *nc, const Q &q, int l) {
#pragma clang fp contract(off)
    float ql[K];
    q.load(l, ql);
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float t = nc[(long)l * K + k] * ql[k];
        acc = acc + t;
    }
    return acc;
}

}  // namespace gmc
