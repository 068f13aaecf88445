// What the annealing kernels share (kway_search.hip: K classes, the 3-class entry point being K = 3; kway_evolve.hip:
// the children of a generation, through anneal_body.h): the launch arguments, the two accessors of a graph's CSR (the
// batch's arrays in global memory, the workgroup's copy in LDS; refine.hip and round.hip walk their descent through
// the global one) and the LDS layout of a launch.  None of it depends on the class count, so gmc_refine_anneal_staged
// answers for every K.
//
// One 256-thread workgroup per (candidate, graph), as in refine.hip.  Where the local search runs about 4 sweeps the
// annealing runs about 100 and recounts the cut after each, so what it re-reads every sweep lives in LDS:
//
//   levels   [1024] float      4096 B   the caller's table (the device evaluates neither exp nor log)
//   state    [n_pad] byte               the classes as they stand          (n_pad = n_max rounded up to 16)
//   best     [n_pad] byte               the snapshot with the largest cut so far
//   --- staged copy of the graph (only when it fits GMC_ANNEAL_LDS_BUDGET, see anneal_layout) ---
//   starts   [n_max + 1] int            CSR row starts, relative to the graph's first edge
//   vals     [nnz_max] float            edge weights (weighted batches only)
//   order    [n_pad] uint16             the movable nodes in (colour, id) order as local ids
//   ids      [nnz_max] uint16           neighbour ids (local ids fit 16 bits: n <= 4096)
//
// n = 1000, d = 7, unit weights: 4096 + 2 * 1008 + 4016 + 2016 + 14000 = 26144 B, six workgroups (24 waves) per CU.
// A batch whose copy would push a workgroup past the budget (40 KiB including GMC_ANNEAL_LDS_STATIC for the kernel's
// static LDS, so at least four workgroups = 16 waves, four per SIMD, fit the 160 KiB of a CU) runs the same
// code over the batch's arrays in global memory (12 KiB of LDS at most, eight workgroups per CU).  Both paths are one
// template over the accessor, so their arithmetic cannot differ.
#pragma once
#include "gmc_common.h"
#include "mix64.h"

#define GMC_ANNEAL_LDS_BUDGET (40 * 1024)
#define GMC_ANNEAL_LDS_STATIC 512   // allowance for red, flag and the barrier's word (288 B as built)

namespace gmc {

struct AnnealArgs {
    gmc_batch b;
    const int *order, *cgoff, *cptr;   // gmc_refine_order_host's output
    int cands, anneal_sweeps, max_descent_sweeps;
    int first;               // first movable local id: K with terminals, 0 without (in what was the struct's padding)
    const float *inv_temp;   // [anneal_sweeps]
    const float *levels;     // [GMC_ANNEAL_LEVELS]
    u64 seed;
    signed char *assign;     // [cands][R], in/out
    float *cut_all;          // [B][cands]
    int *snap_sweep;         // [B][cands] or NULL
    int *sweeps;             // [B][cands] or NULL
    int staged;              // the launch has room for the staged copy
    int n_pad, off_starts, off_vals, off_order, off_ids;   // LDS layout (bytes from the dynamic base)
    const float *node_cost;  // [R][K] by batch row or NULL (gmc_kway_refine_anneal_c_f32; read from global memory)
};

// the graph as the batch holds it in global memory
struct GlobalCsr {
    const int *rp;      // rowptr + r0: absolute edge positions of local row l
    const int *col;
    const float *vals;
    const int *order;
    int r0;
    int first;          // first movable local id: K with terminals, 0 without
    __device__ __forceinline__ int node(int i) const { return order[i] - r0; }
    // is local id l, an entry of the order, a movable row of this graph of n nodes?
    // (one unsigned compare, as the compiler made of `l < K || l >= n` while K was a literal: first <= n for every
    // graph a kernel runs, and a negative l wraps beyond any n - first)
    __device__ __forceinline__ bool movable(int l, int n) const { return (unsigned)(l - first) < (unsigned)(n - first); }
};
// the workgroup's copy in LDS (edge positions relative to the graph's first edge, order relative to its first entry)
struct LdsCsr {
    const int *rp;
    const unsigned short *col;
    const float *vals;
    const unsigned short *order;
    int i0;
    __device__ __forceinline__ int node(int i) const { return order[i - i0]; }
    // (an entry that is no movable row was staged as 0xffff: the copy has applied `first` already)
    __device__ __forceinline__ bool movable(int l, int n) const { return l < n; }
};

// LDS bytes of a launch for this batch and whether they include the staged copy
struct AnnealLayout {
    int staged, n_pad, off_starts, off_vals, off_order, off_ids, bytes;
};
inline AnnealLayout anneal_layout(const gmc_batch *b) {
    AnnealLayout L{};
    L.n_pad = (b->n_max + 15) & ~15;
    const int base = 4 * GMC_ANNEAL_LEVELS + 2 * L.n_pad;
    const long nnz = b->nnz_max > 0 ? b->nnz_max : 0;
    L.off_starts = base;
    L.off_vals = L.off_starts + (((b->n_max + 1) * 4 + 15) & ~15);
    L.off_order = L.off_vals + (b->vals ? (int)((nnz * 4 + 15) & ~15L) : 0);
    L.off_ids = L.off_order + 2 * L.n_pad;
    const long total = L.off_ids + ((nnz * 2 + 15) & ~15L);
    L.staged = nnz > 0 && total + GMC_ANNEAL_LDS_STATIC <= GMC_ANNEAL_LDS_BUDGET;
    L.bytes = L.staged ? (int)total : base;
    return L;
}

}  // namespace gmc
