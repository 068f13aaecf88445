// What the annealing kernels share (anneal.hip: 3 classes; kway_search.hip: K classes; kway_evolve.hip: the children of
// a generation, through anneal_body.h): the launch arguments, the
// two accessors of a graph's CSR (the batch's arrays in global memory, the workgroup's copy in LDS) and the LDS layout
// of a launch.  None of it depends on the class count, so one definition serves both and gmc_refine_anneal_staged
// answers for both.  The layout itself is described at the top of anneal.hip.
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
    const float *inv_temp;   // [anneal_sweeps]
    const float *levels;     // [GMC_ANNEAL_LEVELS]
    u64 seed;
    signed char *assign;     // [cands][R], in/out
    float *cut_all;          // [B][cands]
    int *snap_sweep;         // [B][cands] or NULL
    int *sweeps;             // [B][cands] or NULL
    int staged;              // the launch has room for the staged copy
    int n_pad, off_starts, off_vals, off_order, off_ids;   // LDS layout (bytes from the dynamic base)
};

// the graph as the batch holds it in global memory
struct GlobalCsr {
    const int *rp;      // rowptr + r0: absolute edge positions of local row l
    const int *col;
    const float *vals;
    const int *order;
    int r0;
    __device__ __forceinline__ int node(int i) const { return order[i] - r0; }
};
// the workgroup's copy in LDS (edge positions relative to the graph's first edge, order relative to its first entry)
struct LdsCsr {
    const int *rp;
    const unsigned short *col;
    const float *vals;
    const unsigned short *order;
    int i0;
    __device__ __forceinline__ int node(int i) const { return order[i - i0]; }
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
