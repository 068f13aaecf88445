// Annealing over decoded partitions, followed by the local search's descent (an extension: the reference stops at the
// best of its random samples, TestingNeuralNetwork.py:66-98).  The algorithm is stated in include/gcnmaxcut.h
// (gmc_refine_anneal_f32); the colouring, the (colour, id) order and the per-node sums W0, W1, W2 are those of
// refine.hip; the descent phase runs the same node visit (move_body.h).
//
// One 256-thread workgroup per (candidate, graph), as in refine.hip.  Where the local search runs about 4 sweeps this
// kernel runs about 100 and recounts the cut after each, so what it re-reads every sweep lives in LDS:
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
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"

namespace {

using gmc::mix64;
using gmc::u64;
using gmc::AnnealArgs;
using gmc::GlobalCsr;
using gmc::LdsCsr;
using gmc::AnnealLayout;
using gmc::anneal_layout;

template <class G>
__device__ __forceinline__ void anneal_body(const AnnealArgs &a, const G &g, unsigned char *sa, unsigned char *sb,
                                            const float *lv, int n, int k0, int classes, float *red, int *flag) {
    const int cand = blockIdx.x, gi = blockIdx.y;
    int snap = 0;
    if (a.anneal_sweeps > 0) {
        float best_cut = gmc::block_cut_csr(g.rp, g.col, g.vals, sa, n, red);   // thread 0
        __syncthreads();   // (thread 0 has read red before a graph without classes recounts)
        for (int s = 0; s < a.anneal_sweeps; ++s) {
            const float inv_t = a.inv_temp[s];
            // seed + GOLD * (ctr + 1), ctr = cand << 32 | s << 12 | v: the part without v (v < 2^12 only adds)
            const u64 base = a.seed + 0x9E3779B97F4A7C15ULL * ((((u64)(unsigned)cand << 32) | ((u64)(unsigned)s << 12)) + 1ULL);
            for (int k = 0; k < classes; ++k) {
                const int hi = a.cptr[k0 + k + 1];
                for (int i = a.cptr[k0 + k] + threadIdx.x; i < hi; i += blockDim.x) {
                    const int l = g.node(i);
                    if ((unsigned)l >= (unsigned)n) continue;   // not a row of this graph: never touch LDS for it
                    float w0, w1, w2;
                    gmc::class_sums(g.rp, g.col, g.vals, sa, l, w0, w1, w2);
                    const int c = sa[l];
                    int kk;
                    float wk, wc;
                    if (c == 0) {
                        wc = w0; kk = 1; wk = w1;
                        if (w2 < wk) { kk = 2; wk = w2; }
                    } else if (c == 1) {
                        wc = w1; kk = 0; wk = w0;
                        if (w2 < wk) { kk = 2; wk = w2; }
                    } else if (c == 2) {
                        wc = w2; kk = 0; wk = w0;
                        if (w1 < wk) { kk = 1; wk = w1; }
                    } else {   // a byte of no class: the local search's target, taken unconditionally (delta = -inf)
                        gmc::local_move(w0, w1, w2, c, kk);
                        wc = __builtin_inff(); wk = 0.f;
                    }
                    const float delta = wk - wc;
                    const u64 h = mix64(base + 0x9E3779B97F4A7C15ULL * (u64)(unsigned)l);
                    if (delta < 0.f || delta * inv_t <= lv[h >> 54]) sa[l] = (unsigned char)kk;
                }
                __syncthreads();   // the next class, or the recount, reads what this one wrote
            }
            const float cut = gmc::block_cut_csr(g.rp, g.col, g.vals, sa, n, red);
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
    // descent: refine.hip's sweeps, the same node visit (move_body.h)
    int s = 0;
    while (s < a.max_descent_sweeps) {
        ++s;
        int moved = 0;
        for (int k = 0; k < classes; ++k) {
            const int hi = a.cptr[k0 + k + 1];
            for (int i = a.cptr[k0 + k] + threadIdx.x; i < hi; i += blockDim.x) {
                const int l = g.node(i);
                if ((unsigned)l >= (unsigned)n) continue;
                float w0, w1, w2;
                gmc::class_sums(g.rp, g.col, g.vals, sa, l, w0, w1, w2);
                const int c = sa[l];
                int kk;
                if (gmc::local_move(w0, w1, w2, c, kk)) {
                    sa[l] = (unsigned char)kk;
                    moved = 1;
                }
            }
            if (k + 1 < classes) __syncthreads();
        }
        if (!__syncthreads_or(moved)) break;
    }
    if (threadIdx.x == 0) {
        if (a.snap_sweep) a.snap_sweep[(long)gi * a.cands + cand] = snap;
        if (a.sweeps) a.sweeps[(long)gi * a.cands + cand] = s;
    }
}

__global__ __launch_bounds__(256) void anneal_kernel(AnnealArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    __shared__ int flag;
    const int cand = blockIdx.x, gi = blockIdx.y;
    const int r0 = a.b.goff[gi];
    const int n = a.b.goff[gi + 1] - r0;
    if (n > a.b.n_max) return;   // (a batch that contradicts its own n_max: the LDS is sized by it)
    float *lv = reinterpret_cast<float *>(lds);
    unsigned char *sa = lds + 4 * GMC_ANNEAL_LEVELS;
    unsigned char *sb = sa + a.n_pad;
    signed char *as = a.assign + (long)cand * a.b.R + r0;
    for (int l = threadIdx.x; l < n; l += blockDim.x) sa[l] = sb[l] = (unsigned char)as[l];
    if (a.anneal_sweeps > 0)
        for (int i = threadIdx.x; i < GMC_ANNEAL_LEVELS; i += blockDim.x) lv[i] = a.levels[i];
    const int k0 = a.cgoff[gi];
    const int classes = a.cgoff[gi + 1] - k0 - 1;
    const int e0 = a.b.rowptr[r0];
    const int nnz = a.b.rowptr[r0 + n] - e0;
    const int i0 = a.cptr[k0];
    const int movable = a.cptr[k0 + classes] - i0;
    // the copy is sized by n_max and nnz_max: a graph that contradicts them takes the global path
    if (a.staged && nnz <= a.b.nnz_max && movable <= a.n_pad) {
        int *starts = reinterpret_cast<int *>(lds + a.off_starts);
        float *vals = a.b.vals ? reinterpret_cast<float *>(lds + a.off_vals) : nullptr;
        unsigned short *ord = reinterpret_cast<unsigned short *>(lds + a.off_order);
        unsigned short *ids = reinterpret_cast<unsigned short *>(lds + a.off_ids);
        for (int l = threadIdx.x; l <= n; l += blockDim.x) starts[l] = a.b.rowptr[r0 + l] - e0;
        for (int e = threadIdx.x; e < nnz; e += blockDim.x) {
            ids[e] = (unsigned short)a.b.lcol[e0 + e];
            if (vals) vals[e] = a.b.vals[e0 + e];
        }
        for (int i = threadIdx.x; i < movable; i += blockDim.x) {
            const int l = a.order[i0 + i] - r0;
            ord[i] = (unsigned)l < (unsigned)n ? (unsigned short)l : (unsigned short)0xffff;
        }
        __syncthreads();
        const LdsCsr g{starts, ids, vals, ord, i0};
        anneal_body(a, g, sa, sb, lv, n, k0, classes, red, &flag);
    } else {
        __syncthreads();
        const GlobalCsr g{a.b.rowptr + r0, a.b.lcol, a.b.vals, a.order, r0};
        anneal_body(a, g, sa, sb, lv, n, k0, classes, red, &flag);
    }
    for (int l = threadIdx.x; l < n; l += blockDim.x) as[l] = (signed char)sa[l];
    const float cut = gmc::block_cut(a.b, sa, r0, n, red);   // scored as gmc_refine_local_f32 scores
    if (threadIdx.x == 0) a.cut_all[(long)gi * a.cands + cand] = cut;
}

__global__ __launch_bounds__(256) void anneal_pick_kernel(gmc::PickArgs a) { gmc::pick_best(a); }

}  // namespace

extern "C" int gmc_refine_anneal_staged(const gmc_batch *batch) {
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (batch->n_max < 3 || batch->n_max > GMC_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    return anneal_layout(batch).staged;
}

extern "C" int gmc_refine_anneal_f32(const gmc_batch *batch, const int32_t *order, const int32_t *cgoff,
                                     const int32_t *cptr, int32_t cands, int8_t *assign, const float *inv_temp,
                                     int32_t anneal_sweeps, const float *levels, uint64_t seed,
                                     int32_t max_descent_sweeps, float *cut_all, int32_t *best_assign, float *best_cut,
                                     int32_t *best_idx, int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !assign || !cut_all || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (cands < 1 || anneal_sweeps < 0 || anneal_sweeps >= (1 << 20) || max_descent_sweeps < 0 || batch->B < 0)
        return GMC_ERR_SHAPE;
    if (anneal_sweeps > 0 && (!inv_temp || !levels)) return GMC_ERR_NULL;
    if (batch->B > 0 && (batch->n_max < 3 || batch->n_max > GMC_MAX_GRAPH_NODES)) return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const AnnealLayout L = anneal_layout(batch);
    AnnealArgs a{*batch, order, cgoff, cptr, cands, anneal_sweeps, max_descent_sweeps, inv_temp, levels, seed,
                 reinterpret_cast<signed char *>(assign), cut_all, snap_sweep, sweeps,
                 L.staged, L.n_pad, L.off_starts, L.off_vals, L.off_order, L.off_ids};
    {
        GmcProbeScope probe(GMC_K_ANNEAL, st);
        hipLaunchKernelGGL(anneal_kernel, dim3(cands, batch->B), dim3(256), (size_t)L.bytes, st, a);
        GMC_LAUNCH_CHECK();
    }
    gmc::PickArgs p{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign, best_cut, best_idx};
    hipLaunchKernelGGL(anneal_pick_kernel, dim3(batch->B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
