// The evolution stage over annealed candidates at K = 2..8 classes (an extension: the reference samples and stops):
// gmc_kway_evolve_f32, stated in include/gcnmaxcut.h.  The candidates of a graph form a population; a generation gives
// every slot a child of its own member and an elite member - class names aligned, the nodes they disagree on drawn
// from either - improves it with the annealing body of kway_search.hip (anneal_body.h: the same device code) and keeps
// it when it is no worse than the slot's member.
//
// One 256-thread workgroup per (slot, graph) and one launch per generation: the launch boundary is the only
// synchronisation, a generation reads one plane of the population and writes the other.  The LDS of a launch is the
// annealing's (anneal_layout.h): parent a lives in the state bytes, parent b in the best-state bytes until the
// crossover is done, and the K x K overlap counts, the class map and the three picks in the level table's bytes, which
// are loaded only after the crossover - not a byte more than the annealing's launch.  Every workgroup ranks its graph's
// `cands` cuts itself (cands^2 / 256 compares per thread, the loads of a step all to one address): no ranking launch.
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"
#include "anneal_body.h"

#define GMC_EVOLVE_SELECT 0x53454C4543543031ULL   // gcnmaxcut.h: the two hash domains of a generation
#define GMC_EVOLVE_CROSS 0x43524F5353303031ULL

namespace {

using gmc::mix64;
using gmc::u64;
using gmc::AnnealArgs;
using gmc::AnnealLayout;
using gmc::GlobalCsr;
using gmc::LdsCsr;

struct ScoreArgs {
    gmc_batch b;
    int K, cands;
    const signed char *pop;   // [cands][R]
    float *cut;               // [B][cands]
};

// plane 0 as the caller left it, scored as every decoder scores
__global__ __launch_bounds__(256) void evolve_score_kernel(ScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sa[];
    __shared__ float red[4];
    const int i = blockIdx.x, gi = blockIdx.y;
    const int r0 = a.b.goff[gi];
    const int n = a.b.goff[gi + 1] - r0;
    if (n > a.b.n_max || n < a.K) return;   // (the LDS is sized by n_max; a graph without its K terminals is skipped)
    const signed char *p = a.pop + (long)i * a.b.R + r0;
    for (int l = threadIdx.x; l < n; l += blockDim.x) sa[l] = (unsigned char)p[l];
    __syncthreads();
    const float cut = gmc::block_cut(a.b, sa, r0, n, red);
    if (threadIdx.x == 0) a.cut[(long)gi * a.cands + i] = cut;
}

struct EvolveArgs {
    AnnealArgs an;            // seed: the generation seed; assign, cut_all, snap_sweep, sweeps unused (NULL)
    const signed char *prev;  // [cands][R]  the plane this generation reads
    signed char *next;        // [cands][R]  ... and writes
    const float *cut_prev;    // [B][cands]
    float *cut_next;          // [B][cands]
    float *hist_prev;         // [B] or NULL: the best cut of the plane read
    int elite;                // clipped to 1..cands
    u64 select_seed, cross_seed;
};

template <int K>
__global__ __launch_bounds__(256) void evolve_generation_kernel(EvolveArgs e) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    __shared__ int flag;
    const AnnealArgs &a = e.an;
    const int slot = blockIdx.x, gi = blockIdx.y;
    const int r0 = a.b.goff[gi];
    const int n = a.b.goff[gi + 1] - r0;
    if (n > a.b.n_max || n < K) return;   // (the LDS is sized by n_max; a graph without its K terminals is skipped)
    float *lv = reinterpret_cast<float *>(lds);
    int *overlap = reinterpret_cast<int *>(lds);   // O[ca][cb]: in the level table's bytes until the crossover is done
    int *pi = overlap + K * K;                      // class of b -> class of a
    int *pick = pi + K;                             // the slots of rank r, r + 1 (cyclically) and 0
    static_assert(K * K + K + 3 <= GMC_ANNEAL_LEVELS, "the crossover's scratch lives in the level table");
    unsigned char *sa = lds + 4 * GMC_ANNEAL_LEVELS;
    unsigned char *sb = sa + a.n_pad;
    const signed char *pa = e.prev + (long)slot * a.b.R + r0;
    const float *cuts = e.cut_prev + (long)gi * a.cands;
    if (threadIdx.x < K * K) overlap[threadIdx.x] = 0;
    if (threadIdx.x < 3) pick[threadIdx.x] = -1;
    for (int l = threadIdx.x; l < n; l += blockDim.x) sa[l] = (unsigned char)pa[l];
    const gmc::AnnealGraph q = gmc::anneal_graph(a, gi, r0, n);
    const bool staged = gmc::anneal_fits_lds(a, q);   // workgroup-uniform
    LdsCsr gl{};
    if (staged) gl = gmc::anneal_stage_csr(a, q, lds);
    __syncthreads();

    // 1-2. rank (cut descending, slot ascending) and parents
    const int r = (int)(mix64(e.select_seed + GMC_GOLD * ((u64)(unsigned)slot + 1ULL)) % (u64)(unsigned)e.elite);
    const int r_next = r + 1 < e.elite ? r + 1 : 0;
    for (int j = threadIdx.x; j < a.cands; j += blockDim.x) {
        const float cj = cuts[j];
        int rank = 0;
        for (int k = 0; k < a.cands; ++k) {
            const float ck = cuts[k];
            rank += (ck > cj || (ck == cj && k < j)) ? 1 : 0;
        }
        if (rank == r) pick[0] = j;
        if (rank == r_next) pick[1] = j;
        if (rank == 0) pick[2] = j;
    }
    __syncthreads();
    int pb = pick[0];
    if (pb == slot) pb = e.elite > 1 ? pick[1] : -1;   // -1: a is the only elite member, the child starts as a
    if (e.hist_prev && slot == 0 && threadIdx.x == 0 && pick[2] >= 0) e.hist_prev[gi] = cuts[pick[2]];

    if (pb >= 0) {   // workgroup-uniform
        const signed char *pbp = e.prev + (long)pb * a.b.R + r0;
        for (int l = threadIdx.x; l < n; l += blockDim.x) sb[l] = (unsigned char)pbp[l];
        __syncthreads();
        // 3. overlap counts over the movable nodes (integer LDS atomics: any order gives the same counts)
        for (int l = K + threadIdx.x; l < n; l += blockDim.x) {
            const unsigned ca = sa[l], cb = sb[l];
            if (ca < (unsigned)K && cb < (unsigned)K) atomicAdd(&overlap[ca * K + cb], 1);
        }
        __syncthreads();
        if (threadIdx.x == 0) {   // greedy matching, K rounds: the largest count among unmatched pairs, lowest (ca, cb)
            unsigned used_a = 0, used_b = 0;
            for (int round = 0; round < K; ++round) {
                int best = -1, ba = 0, bb = 0;
                for (int ca = 0; ca < K; ++ca) {
                    if (used_a >> ca & 1) continue;
                    for (int cb = 0; cb < K; ++cb) {
                        if (used_b >> cb & 1) continue;
                        const int o = overlap[ca * K + cb];
                        if (o > best) { best = o; ba = ca; bb = cb; }
                    }
                }
                used_a |= 1u << ba;
                used_b |= 1u << bb;
                pi[bb] = ba;
            }
        }
        __syncthreads();
        // 4. crossover
        for (int l = threadIdx.x; l < n; l += blockDim.x) {
            unsigned c = l;   // a terminal
            if (l >= K) {
                const unsigned ca = sa[l], cb = sb[l];
                const unsigned cp = cb < (unsigned)K ? (unsigned)pi[cb] : ca;   // a byte of no class loses to a's
                c = ca;
                if (cp != ca) {
                    const u64 h = mix64(e.cross_seed + GMC_GOLD * ((((u64)(unsigned)slot << 32) | (u64)(unsigned)l) + 1ULL));
                    if (ca >= (unsigned)K || (h >> 63)) c = cp;
                }
            }
            sa[l] = sb[l] = (unsigned char)c;
        }
    } else {
        for (int l = threadIdx.x; l < n; l += blockDim.x) {
            const unsigned c = l < K ? (unsigned)l : sa[l];
            sa[l] = sb[l] = (unsigned char)c;
        }
    }
    __syncthreads();   // nobody reads the picks or pi any more: the level table may take their place
    if (a.anneal_sweeps > 0)
        for (int i = threadIdx.x; i < GMC_ANNEAL_LEVELS; i += blockDim.x) lv[i] = a.levels[i];
    __syncthreads();

    // 5. improve: the annealing's body, the generation seed in the place of seed and the slot in the place of cand
    if (staged) {
        gmc::anneal_body_k<K>(a, gl, sa, sb, lv, n, q.k0, q.classes, red, &flag);
    } else {
        const GlobalCsr g{a.b.rowptr + r0, a.b.lcol, a.b.vals, a.order, r0, a.first};
        gmc::anneal_body_k<K>(a, g, sa, sb, lv, n, q.k0, q.classes, red, &flag);
    }

    // 6. replace: the child iff its cut >= the cut of a
    const float cut = gmc::block_cut(a.b, sa, r0, n, red);
    if (threadIdx.x == 0) {
        const float cut_a = cuts[slot];
        const int child = cut >= cut_a;
        flag = child;
        e.cut_next[(long)gi * a.cands + slot] = child ? cut : cut_a;
    }
    __syncthreads();
    signed char *out = e.next + (long)slot * a.b.R + r0;
    if (flag) {
        for (int l = threadIdx.x; l < n; l += blockDim.x) out[l] = (signed char)sa[l];
    } else {
        for (int l = threadIdx.x; l < n; l += blockDim.x) out[l] = pa[l];
    }
}

struct EvolvePickArgs {
    gmc::PickArgs p;
    int K;
    float *hist_last;   // [B] or NULL: the best cut of the plane picked from
};
__global__ __launch_bounds__(256) void evolve_pick_kernel(EvolvePickArgs a) {
    const int g = blockIdx.x;
    const int n = a.p.b.goff[g + 1] - a.p.b.goff[g];
    if (n > a.p.b.n_max || n < a.K) return;   // workgroup-uniform: the graphs the generations skipped
    gmc::pick_best(a.p);
    if (a.hist_last && threadIdx.x == 0) a.hist_last[g] = a.p.best_cut[g];   // thread 0 wrote it
}

template <int K>
int generation_launch(const EvolveArgs &e, int lds_bytes, hipStream_t st) {
    GmcProbeScope probe(GMC_K_ANNEAL, st);
    hipLaunchKernelGGL((evolve_generation_kernel<K>), dim3(e.an.cands, e.an.b.B), dim3(256), (size_t)lds_bytes, st, e);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

extern "C" int gmc_kway_evolve_f32(const gmc_batch *batch, int32_t K, const int32_t *order, const int32_t *cgoff,
                                   const int32_t *cptr, int32_t cands, int8_t *pop, float *cut, int32_t generations,
                                   int32_t elite, const float *inv_temp, int32_t anneal_sweeps, const float *levels,
                                   uint64_t seed, int32_t max_descent_sweeps, int32_t *best_assign, float *best_cut,
                                   int32_t *best_idx, float *history, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !pop || !cut || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (cands < 1 || anneal_sweeps < 0 || anneal_sweeps >= (1 << 20) || max_descent_sweeps < 0 || batch->B < 0 ||
        generations < 0 || generations >= (1 << 20) || elite < 1)
        return GMC_ERR_SHAPE;
    if (anneal_sweeps > 0 && (!inv_temp || !levels)) return GMC_ERR_NULL;
    if (batch->B > 0 && (batch->n_max < K || batch->n_max > GMC_MAX_GRAPH_NODES)) return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const int B = batch->B;
    signed char *planes[2] = {reinterpret_cast<signed char *>(pop),
                              reinterpret_cast<signed char *>(pop) + (size_t)cands * (size_t)batch->R};
    float *cuts[2] = {cut, cut + (size_t)B * (size_t)cands};
    {
        GmcProbeScope probe(GMC_K_SAMPLE, st);
        const ScoreArgs s{*batch, K, cands, planes[0], cuts[0]};
        hipLaunchKernelGGL(evolve_score_kernel, dim3(cands, B), dim3(256), (size_t)batch->n_max, st, s);
        GMC_LAUNCH_CHECK();
    }
    const AnnealLayout L = gmc::anneal_layout(batch);
    for (int g = 1; g <= generations; ++g) {
        const u64 gen_seed = mix64(seed + GMC_GOLD * (u64)g);
        const int from = (g - 1) & 1, to = g & 1;
        const EvolveArgs e{{*batch, order, cgoff, cptr, cands, anneal_sweeps, max_descent_sweeps, K, inv_temp, levels,
                            gen_seed, nullptr, nullptr, nullptr, nullptr, L.staged, L.n_pad, L.off_starts, L.off_vals,
                            L.off_order, L.off_ids},
                           planes[from], planes[to], cuts[from], cuts[to],
                           history ? history + (size_t)(g - 1) * (size_t)B : nullptr, elite < cands ? elite : cands,
                           mix64(gen_seed ^ GMC_EVOLVE_SELECT), mix64(gen_seed ^ GMC_EVOLVE_CROSS)};
        int rc = GMC_OK;
        GMC_KWAY_DISPATCH(K, rc = generation_launch<KK>(e, L.bytes, st));
        if (rc != GMC_OK) return rc;
    }
    const int last = generations & 1;
    const EvolvePickArgs p{{*batch, cands, planes[last], cuts[last], best_assign, best_cut, best_idx}, K,
                           history ? history + (size_t)generations * (size_t)B : nullptr};
    hipLaunchKernelGGL(evolve_pick_kernel, dim3(B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
