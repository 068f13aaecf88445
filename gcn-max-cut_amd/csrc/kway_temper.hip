// Parallel tempering over decoded partitions at K = 2..8 classes (an extension: the reference samples and stops):
// gmc_kway_temper_f32, stated in include/gcnmaxcut_temper.h.  The candidates of a graph are walkers of the annealing's
// sweep on ladders of fixed inverse temperatures; after every round neighbouring rungs of a ladder copy exchange their
// temperatures by the Metropolis rule.  States stay in their slot.
//
// One 256-thread workgroup per (slot, graph) and one launch per round: the launch boundary is the only synchronisation,
// a round reads one plane of the workspace's rungs and scores and writes the other (no atomics, no spin waits).  Every
// workgroup reads the few words of its own ladder copy itself: one thread per rung finds the partner, thread 0 decides.
// The LDS of a launch is the annealing's (anneal_layout.h): the walker in the state bytes, the best state in the best
// bytes, the staged CSR when it fits; the partner and the rung pass through the level table's first two words before the
// table is loaded.  The node visit, the recount and the staging are the annealing's device code (move_body.h,
// cut_body.h, anneal_body.h); the sweep loop is a body of its own because the walker, not the best state, must survive
// the round (anneal_body_k ends on its best state).
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"
#include "anneal_body.h"
#include "../../include/gcnmaxcut_temper.h"

static_assert(GMC_TEMPER_GOLD == GMC_GOLD, "one hash for the sweeps and the exchanges");

namespace {

using gmc::mix64;
using gmc::u64;
using gmc::AnnealArgs;
using gmc::AnnealLayout;
using gmc::GlobalCsr;
using gmc::LdsCsr;
using gmc::Sums;

struct TemperArgs {
    AnnealArgs an;            // assign: the walkers; anneal_sweeps: round_sweeps (0 in the launch of rounds = 0);
                              // inv_temp, cut_all, snap_sweep, sweeps, max_descent_sweeps unused
    int rungs, t;             // t: this round
    const float *ladder;      // [rungs]
    u64 exchange_seed;        // E = mix64(seed ^ GMC_TEMPER_TAG)
    const int *rung_prev;     // [B][cands]  the planes this round reads (never read at t = 0)
    const float *score_prev;
    int *rung_next;           // ... and writes
    float *score_next;
    signed char *best;        // [cands][R]
    float *best_score;        // [B][cands]
    int *best_round, *rung_out, *swaps;   // [B][cands] or NULL
};

// round_sweeps sweeps of the annealing's step 2 at one inverse temperature on the walker in sa, sb the best state so
// far; thread 0 carries best (its score) and x (the score after the last sweep run), every thread `changed`.
template <int K, bool COST, class G>
__device__ __forceinline__ void temper_sweeps_k(const AnnealArgs &a, const G &g, unsigned char *sa, unsigned char *sb,
                                                const float *lv, int n, int k0, int classes, float *red, int *flag,
                                                const float *nc, float inv_t, int s0, float &x, float &best,
                                                int &changed) {
    const int cand = blockIdx.x;
    for (int j = 0; j < a.anneal_sweeps; ++j) {
        const int s = s0 + j;
        // seed + GOLD * (ctr + 1), ctr = cand << 32 | s << 12 | v: the annealing's counter (anneal_body.h)
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
            const int better = cut > best;
            if (better) best = cut;
            x = cut;
            *flag = better;
        }
        __syncthreads();   // (also: thread 0 has read red before the next recount writes it)
        if (*flag) {       // workgroup-uniform
            changed = 1;
            for (int l = threadIdx.x; l < n; l += blockDim.x) sb[l] = sa[l];
            __syncthreads();   // the next sweep moves nodes other threads are copying
        }
    }
}

template <int K, bool COST>
__global__ __launch_bounds__(256) void temper_round_kernel(TemperArgs e) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    __shared__ int flag;
    const AnnealArgs &a = e.an;
    const int slot = blockIdx.x, gi = blockIdx.y;
    const int r0 = a.b.goff[gi];
    const int n = a.b.goff[gi + 1] - r0;
    if (n > a.b.n_max || n < a.first) return;   // (the LDS is sized by n_max; a graph without its terminals is skipped)
    float *lv = reinterpret_cast<float *>(lds);
    int *word = reinterpret_cast<int *>(lds);   // [0] the partner's place in the copy, [1] the rung: until the table is loaded
    unsigned char *sa = lds + 4 * GMC_ANNEAL_LEVELS;
    unsigned char *sb = sa + a.n_pad;
    signed char *st = a.assign + (long)slot * a.b.R + r0;
    signed char *bs = e.best + (long)slot * a.b.R + r0;
    const long own = (long)gi * a.cands + slot;
    const int t = e.t;
    if (t == 0) {
        for (int l = threadIdx.x; l < n; l += blockDim.x) sa[l] = sb[l] = (unsigned char)st[l];
    } else {
        for (int l = threadIdx.x; l < n; l += blockDim.x) {
            sa[l] = (unsigned char)st[l];
            sb[l] = (unsigned char)bs[l];
        }
    }

    // 1. the rung
    const int copy = slot / e.rungs;
    const long copy0 = (long)gi * a.cands + (long)copy * e.rungs;   // the copy's first word of a plane
    int rung = slot - copy * e.rungs, pair = -1, other = -1;
    if (t > 0) {
        const int r = e.rung_prev[own];
        if ((unsigned)r < (unsigned)e.rungs) {
            rung = r;
            const int p = ((r ^ t) & 1) ? r - 1 : r;   // the pair of this round's parity that holds r
            if (p >= 0 && p + 1 < e.rungs) {
                pair = p;
                other = r == p ? p + 1 : p;
            }
        }
    }
    if (threadIdx.x == 0) word[0] = -1;
    __syncthreads();
    if (other >= 0 && (int)threadIdx.x < e.rungs && e.rung_prev[copy0 + threadIdx.x] == other) word[0] = threadIdx.x;
    __syncthreads();
    if (threadIdx.x == 0) {
        int swapped = 0;
        const int partner = word[0];
        if (partner >= 0) {   // (so pair >= 0 as well)
#pragma clang fp contract(off)
            const float x_own = e.score_prev[own], x_other = e.score_prev[copy0 + partner];
            const float x_lo = rung == pair ? x_own : x_other, x_hi = rung == pair ? x_other : x_own;
            const float d = (e.ladder[pair + 1] - e.ladder[pair]) * (x_hi - x_lo);
            const u64 ctr = ((u64)(unsigned)t << 40) | ((u64)(unsigned)copy << 8) | (u64)(unsigned)pair;
            const u64 h = mix64(e.exchange_seed + GMC_GOLD * (ctr + 1ULL));
            swapped = d < 0.f || d <= a.levels[h >> 54];
        }
        if (swapped) rung = other;
        word[1] = rung;
        e.rung_next[own] = rung;
        if (e.rung_out) e.rung_out[own] = rung;
        if (e.swaps) {
            if (t == 0) e.swaps[own] = 0;
            else if (swapped) e.swaps[own] += 1;   // this slot's own word: no other workgroup touches it
        }
    }
    __syncthreads();
    rung = word[1];
    const float inv_t = e.ladder[rung];
    __syncthreads();   // everybody has the rung: the level table may take the words' place
    if (a.anneal_sweeps > 0)
        for (int i = threadIdx.x; i < GMC_ANNEAL_LEVELS; i += blockDim.x) lv[i] = a.levels[i];

    const gmc::AnnealGraph q = gmc::anneal_graph(a, gi, r0, n);
    const float *nc = nullptr;   // the graph's cost rows, by local id
    if constexpr (COST) {
        // held in a vector register pair, as the annealing's cost kernel holds it (anneal_kernel_body.inc): the scalar
        // file is what runs out
        unsigned long long bits = reinterpret_cast<unsigned long long>(a.node_cost + (long)r0 * K);
        asm volatile("" : "+v"(bits));
        nc = reinterpret_cast<const float *>(bits);
        // ... and so are the two pointers only the tail needs (K = 8 otherwise parks two scalars in a vector register)
        unsigned long long sbits = reinterpret_cast<unsigned long long>(st), bbits = reinterpret_cast<unsigned long long>(bs);
        asm volatile("" : "+v"(sbits), "+v"(bbits));
        st = reinterpret_cast<signed char *>(sbits);
        bs = reinterpret_cast<signed char *>(bbits);
    }

    // 2-3. the sweeps and the best state
    float x = 0.f, best = 0.f;   // thread 0
    int changed = t == 0;
    const int s0 = t * a.anneal_sweeps;
    auto run = [&](const auto &g) {
        if (t == 0) {   // the input is the best state so far
            if constexpr (COST) best = gmc::block_score_csr<K>(g.rp, g.col, g.vals, nc, sa, n, red);
            else best = gmc::block_cut_csr(g.rp, g.col, g.vals, sa, n, red);
            x = best;
            __syncthreads();   // (thread 0 has read red before a graph without classes recounts)
        } else if (threadIdx.x == 0) {
            best = e.best_score[own];
        }
        temper_sweeps_k<K, COST>(a, g, sa, sb, lv, n, q.k0, q.classes, red, &flag, nc, inv_t, s0, x, best, changed);
    };
    if (gmc::anneal_fits_lds(a, q)) {   // workgroup-uniform
        const LdsCsr g = gmc::anneal_stage_csr(a, q, lds);
        __syncthreads();
        run(g);
    } else {
        __syncthreads();
        const GlobalCsr g{a.b.rowptr + r0, a.b.lcol, a.b.vals, a.order, r0, a.first};
        run(g);
    }

    // the tail: the walker always, the best state only when this round replaced it
    for (int l = threadIdx.x; l < n; l += blockDim.x) st[l] = (signed char)sa[l];
    if (changed) {   // workgroup-uniform
        for (int l = threadIdx.x; l < n; l += blockDim.x) bs[l] = (signed char)sb[l];
        if (threadIdx.x == 0) {
            e.best_score[own] = best;
            if (e.best_round) e.best_round[own] = t;
        }
    }
    if (threadIdx.x == 0) e.score_next[own] = x;
}

template <int K>
int round_launch(const TemperArgs &e, int lds_bytes, hipStream_t st) {
    GmcProbeScope probe(GMC_K_ANNEAL, st);
    if (e.an.node_cost)
        hipLaunchKernelGGL((temper_round_kernel<K, true>), dim3(e.an.cands, e.an.b.B), dim3(256), (size_t)lds_bytes, st, e);
    else
        hipLaunchKernelGGL((temper_round_kernel<K, false>), dim3(e.an.cands, e.an.b.B), dim3(256), (size_t)lds_bytes, st, e);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

size_t plane_bytes(int B, int cands) { return ((size_t)B * (size_t)cands * 4 + 15) & ~(size_t)15; }

}  // namespace

extern "C" size_t gmc_kway_temper_workspace_bytes(const gmc_batch *batch, int32_t cands) {
    if (!batch || batch->abi != GMC_VERSION || batch->B < 0 || cands < 1) return 0;
    return 4 * plane_bytes(batch->B, cands);
}

extern "C" int gmc_kway_temper_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const float *node_cost,
                                   const int32_t *order, const int32_t *cgoff, const int32_t *cptr, int32_t cands,
                                   int32_t rungs, const float *ladder, int32_t rounds, int32_t round_sweeps,
                                   const float *levels, uint64_t seed, int8_t *state, int8_t *best, float *best_score,
                                   int32_t *best_round, int32_t *rung_out, int32_t *swaps, void *workspace,
                                   size_t workspace_bytes, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !ladder || !levels || !state || !best || !best_score || !workspace)
        return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (rungs < 1 || rungs > GMC_TEMPER_MAX_RUNGS || cands < 1 || cands % rungs != 0 || rounds < 0 || round_sweeps < 0 ||
        (rounds > 0 && round_sweeps < 1) || (int64_t)rounds * (int64_t)round_sweeps >= (1 << 20) || batch->B < 0 ||
        (terminals != 0 && terminals != 1))
        return GMC_ERR_SHAPE;
    const int first = terminals ? K : 0;
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || batch->n_max > GMC_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    if (!gmc_aligned16(workspace)) return GMC_ERR_ALIGN;
    if (workspace_bytes < gmc_kway_temper_workspace_bytes(batch, cands)) return GMC_ERR_WORKSPACE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const size_t plane = plane_bytes(batch->B, cands);
    unsigned char *ws = static_cast<unsigned char *>(workspace);
    int *rung_plane[2] = {reinterpret_cast<int *>(ws), reinterpret_cast<int *>(ws + plane)};
    float *score_plane[2] = {reinterpret_cast<float *>(ws + 2 * plane), reinterpret_cast<float *>(ws + 3 * plane)};
    const AnnealLayout L = gmc::anneal_layout(batch);
    const u64 exchange_seed = mix64(seed ^ GMC_TEMPER_TAG);
    const int launches = rounds > 0 ? rounds : 1;
    for (int t = 0; t < launches; ++t) {
        const int from = (t - 1) & 1, to = t & 1;
        const TemperArgs e{{*batch, order, cgoff, cptr, cands, rounds > 0 ? round_sweeps : 0, 0, first, nullptr, levels,
                            seed, reinterpret_cast<signed char *>(state), nullptr, nullptr, nullptr, L.staged, L.n_pad,
                            L.off_starts, L.off_vals, L.off_order, L.off_ids, node_cost},
                           rungs, t, ladder, exchange_seed, rung_plane[from], score_plane[from], rung_plane[to],
                           score_plane[to], reinterpret_cast<signed char *>(best), best_score, best_round, rung_out,
                           swaps};
        int rc = GMC_OK;
        GMC_KWAY_DISPATCH(K, rc = round_launch<KK>(e, L.bytes, st));
        if (rc != GMC_OK) return rc;
    }
    return GMC_OK;
}
