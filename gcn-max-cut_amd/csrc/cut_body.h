// Cut count and best-candidate pick shared by the post-processing samplers (decode.hip, kway_search.hip), the local
// search (refine.hip), the rounding (round.hip), the annealing (kway_search.hip) and the evolution (kway_evolve.hip):
// all score their candidates with the same code, so a candidate a search does not move gets, bit for bit, the cut the
// sampler reports for it.
#pragma once
#include "gmc_common.h"

namespace gmc {

// Cut of the assignment `sa` (local node id -> class byte, in LDS) of the graph on batch rows r0 .. r0+n-1: the
// edge-parallel count over the CSR (each undirected edge seen twice -> / 2), one thread per row, a butterfly per
// wave, the four wave sums in a fixed order.  Every thread of the 256-thread workgroup must call it (one barrier);
// thread 0 gets the cut.  red: 4 floats of LDS.
//
// block_cut_csr is the count itself over any copy of the graph's CSR: rp[l] .. rp[l + 1] are the edges of local row l
// in col (local neighbour ids) and vals (NULL: all ones).  block_cut reads the batch's arrays in global memory; the
// annealing body (anneal_body.h) also calls block_cut_csr on the copy it keeps in LDS - one piece of code, one
// summation order, the same bits.
template <class RP, class COL>
__device__ __forceinline__ float block_cut_csr(const RP *rp, const COL *col, const float *vals, const unsigned char *sa,
                                               int n, float *red) {
    float cut = 0.f;
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const int me = sa[l];
        for (int e = rp[l]; e < (int)rp[l + 1]; ++e) {
            const float w = vals ? vals[e] : 1.0f;
            cut += sa[col[e]] != me ? w : 0.f;
        }
    }
    cut = wave_sum(cut);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cut;
    __syncthreads();
    return (((red[0] + red[1]) + red[2]) + red[3]) * 0.5f;
}

__device__ __forceinline__ float block_cut(const gmc_batch &b, const unsigned char *sa, int r0, int n, float *red) {
    return block_cut_csr(b.rowptr + r0, b.lcol, b.vals, sa, n, red);
}

// Cost of the assignment `sa` under the per-node class costs nc ([n][K] by local id: the caller's node_cost + r0 * K):
// the sum of nc[l][sa[l]], a class byte outside 0..K-1 adding nothing, over the rows l = tid, tid + 256, ... per thread,
// a butterfly per wave, the four wave sums in block_cut_csr's order.  Every thread of the 256-thread workgroup must
// call it (two barriers: the first lets thread 0 finish reading a block_cut's red); thread 0 gets the cost.
template <int K>
__device__ __forceinline__ float block_cost(const float *nc, const unsigned char *sa, int n, float *red) {
    float cost = 0.f;
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const unsigned c = sa[l];
        cost += c < (unsigned)K ? nc[(long)l * K + c] : 0.f;
    }
    cost = wave_sum(cost);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cost;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}

// The score of a state wherever one is scored: block_cut_csr, and with costs (nc != NULL, workgroup-uniform) one fp32
// subtraction of block_cost from it.  nc == NULL is block_cut_csr and nothing else.
template <int K, class RP, class COL>
__device__ __forceinline__ float block_score_csr(const RP *rp, const COL *col, const float *vals, const float *nc,
                                                 const unsigned char *sa, int n, float *red) {
#pragma clang fp contract(off)
    const float cut = block_cut_csr(rp, col, vals, sa, n, red);
    if (!nc) return cut;
    const float cost = block_cost<K>(nc, sa, n, red);
    return cut - cost;
}
template <int K>
__device__ __forceinline__ float block_score(const gmc_batch &b, const float *nc, const unsigned char *sa, int r0, int n,
                                             float *red) {
    return block_score_csr<K>(b.rowptr + r0, b.lcol, b.vals, nc, sa, n, red);
}

struct PickArgs {
    gmc_batch b;
    int iters;                     // candidates per graph
    const signed char *assign_all; // [iters][R]
    const float *cut_all;          // [B][iters]
    int *best_assign;  // [R]
    float *best_cut;   // [B]
    int *best_iter;    // [B]
};

// One workgroup (256 threads) per graph: the index of the strictly best of its `iters` candidate cuts, the first one on
// ties; thread 0 writes best_cut[g] and best_iter[g], every thread gets the index (one barrier).
__device__ __forceinline__ int pick_best_index(const float *cut_all, int iters, int g, float *best_cut, int *best_iter) {
    __shared__ int sbest;
    if (threadIdx.x == 0) {  // strict '>' keeps the first best (TestingNeuralNetwork.py:94)
        int bi = 0;
        float bc = cut_all[(long)g * iters];
        for (int i = 1; i < iters; ++i) {
            const float c = cut_all[(long)g * iters + i];
            if (c > bc) { bc = c; bi = i; }
        }
        sbest = bi;
        best_cut[g] = bc;
        best_iter[g] = bi;
    }
    __syncthreads();
    return sbest;
}

// One workgroup (256 threads) per graph: the strictly best candidate, the first one on ties, and its assignment.
__device__ __forceinline__ void pick_best(const PickArgs &a) {
    const int g = blockIdx.x;
    const int best = pick_best_index(a.cut_all, a.iters, g, a.best_cut, a.best_iter);
    const int r0 = a.b.goff[g], n = a.b.goff[g + 1] - r0;
    for (int l = threadIdx.x; l < n; l += blockDim.x)
        a.best_assign[r0 + l] = a.assign_all[(long)best * a.b.R + r0 + l];
}

}  // namespace gmc
