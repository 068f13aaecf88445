// The K-class annealing of one (candidate, graph) workgroup, shared by kway_search.hip (gmc_kway_refine_anneal_f32 and,
// at K = 3, gmc_refine_anneal_f32) and kway_evolve.hip (gmc_kway_evolve_f32, which improves every child with it): the
// staged copy of the graph's CSR and the body of steps 1-3 - annealing sweeps with the best state kept, then the
// descent (move_body.h's descent_sweeps).  One definition, so a child is improved by exactly the code that annealed its
// parents.
#pragma once
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"

namespace gmc {

// What a workgroup reads of its graph before it decides between the two accessors.
struct AnnealGraph {
    int r0, n;        // first batch row, nodes
    int k0, classes;  // first entry of cptr, colour classes
    int e0, nnz;      // first edge, edges
    int i0, movable;  // first entry of order, entries
};
__device__ __forceinline__ AnnealGraph anneal_graph(const AnnealArgs &a, int gi, int r0, int n) {
    AnnealGraph q;
    q.r0 = r0;
    q.n = n;
    q.k0 = a.cgoff[gi];
    q.classes = a.cgoff[gi + 1] - q.k0 - 1;
    q.e0 = a.b.rowptr[r0];
    q.nnz = a.b.rowptr[r0 + n] - q.e0;
    q.i0 = a.cptr[q.k0];
    q.movable = a.cptr[q.k0 + q.classes] - q.i0;
    return q;
}
// the copy is sized by n_max and nnz_max: a graph that contradicts them takes the global path
__device__ __forceinline__ bool anneal_fits_lds(const AnnealArgs &a, const AnnealGraph &q) {
    return a.staged && q.nnz >= 0 && q.nnz <= a.b.nnz_max && q.movable >= 0 && q.movable <= a.n_pad;
}
// Copies the graph's CSR and its part of `order` into the launch's LDS (anneal_layout.h); the caller's barrier
// publishes it.
__device__ __forceinline__ LdsCsr anneal_stage_csr(const AnnealArgs &a, const AnnealGraph &q, unsigned char *lds) {
    int *starts = reinterpret_cast<int *>(lds + a.off_starts);
    float *vals = a.b.vals ? reinterpret_cast<float *>(lds + a.off_vals) : nullptr;
    unsigned short *ord = reinterpret_cast<unsigned short *>(lds + a.off_order);
    unsigned short *ids = reinterpret_cast<unsigned short *>(lds + a.off_ids);
    for (int l = threadIdx.x; l <= q.n; l += blockDim.x) starts[l] = a.b.rowptr[q.r0 + l] - q.e0;
    for (int e = threadIdx.x; e < q.nnz; e += blockDim.x) {
        ids[e] = (unsigned short)a.b.lcol[q.e0 + e];
        if (vals) vals[e] = a.b.vals[q.e0 + e];
    }
    for (int i = threadIdx.x; i < q.movable; i += blockDim.x) {
        const int l = a.order[q.i0 + i] - q.r0;
        ord[i] = l >= a.first && l < q.n ? (unsigned short)l : (unsigned short)0xffff;
    }
    return LdsCsr{starts, ids, vals, ord, q.i0};
}

// Steps 1-3 of gmc_kway_refine_anneal_f32 on the state in sa (sb: a copy of it, the best-state buffer) for candidate
// blockIdx.x of graph blockIdx.y; on return sa holds the result and every thread may read it.  nc: the graph's rows of
// a.node_cost (class_sums_k's and block_cost's argument) or NULL: the sums start from it and the best state is kept by
// the objective, cut - cost.  COST says at compile time whether nc may be set: without it the body is, statement for
// statement, the one it was before costs existed (the run-time test alone cost 1.6 % at K = 3).
template <int K, bool COST = false, class G>
__device__ __forceinline__ void anneal_body_k(const AnnealArgs &a, const G &g, unsigned char *sa, unsigned char *sb,
                                              const float *lv, int n, int k0, int classes, float *red, int *flag,
                                              const float *nc = nullptr) {
    const int cand = blockIdx.x, gi = blockIdx.y;
    int snap = 0;
    if (a.anneal_sweeps > 0) {
        float best_cut;   // thread 0
        if constexpr (COST) best_cut = gmc::block_score_csr<K>(g.rp, g.col, g.vals, nc, sa, n, red);
        else best_cut = gmc::block_cut_csr(g.rp, g.col, g.vals, sa, n, red);
        __syncthreads();   // (thread 0 has read red before a graph without classes recounts)
        for (int s = 0; s < a.anneal_sweeps; ++s) {
            const float inv_t = a.inv_temp[s];
            // seed + GOLD * (ctr + 1), ctr = cand << 32 | s << 12 | v: the part without v (v < 2^12 only adds)
            const u64 base = a.seed + GMC_GOLD * ((((u64)(unsigned)cand << 32) | ((u64)(unsigned)s << 12)) + 1ULL);
            for (int k = 0; k < classes; ++k) {
                const int hi = a.cptr[k0 + k + 1];
                for (int i = a.cptr[k0 + k] + threadIdx.x; i < hi; i += blockDim.x) {
                    const int l = g.node(i);
                    if (!g.movable(l, n)) continue;   // not a movable row of this graph: never touch LDS for it
                    const Sums<K> w = gmc::class_sums_k<K>(g.rp, g.col, g.vals, sa, l, COST ? nc : nullptr);
                    const u64 h = mix64(base + GMC_GOLD * (u64)(unsigned)l);
                    int kk;
                    if (gmc::anneal_move<K>(w, sa[l], inv_t, lv, h, kk)) sa[l] = (unsigned char)kk;
                }
                __syncthreads();   // the next class, or the recount, reads what this one wrote
            }
            float cut;
            if constexpr (COST) cut = gmc::block_score_csr<K>(g.rp, g.col, g.vals, nc, sa, n, red);
            else cut = gmc::block_cut_csr(g.rp, g.col, g.vals, sa, n, red);
            if (threadIdx.x == 0) {
                const int better = cut > best_cut;
                if (better) best_cut = cut;
                *flag = better;
            }
            __syncthreads();   // (also: thread 0 has read red before the next recount writes it)
            if (*flag) {       // workgroup-uniform
                snap = s + 1;
                for (int l = threadIdx.x; l < n; l += blockDim.x) sb[l] = sa[l];
                __syncthreads();   // the next sweep moves nodes other threads are copying
            }
        }
        for (int l = threadIdx.x; l < n; l += blockDim.x) sa[l] = sb[l];
        __syncthreads();
    }
    // descent: the local search's sweeps from the best state
    const int s = descent_sweeps<K>(g, a.cptr, k0, classes, sa, n, a.max_descent_sweeps, COST ? nc : nullptr);
    if (threadIdx.x == 0) {
        if (a.snap_sweep) a.snap_sweep[(long)gi * a.cands + cand] = snap;
        if (a.sweeps) a.sweeps[(long)gi * a.cands + cand] = s;
    }
}

}  // namespace gmc
