// One-flip tabu search over decoded partitions at K = 2..8 classes (an extension: the reference samples and stops):
// gmc_kway_tabu_f32, stated to the operation in include/gcnmaxcut.h.  A chain is one (candidate, graph) pair; every
// iteration takes the best admissible single move, forbids moving that node again for a while and lets a move that
// would beat the best cut seen override the ban.
//
// One WAVE per chain, so the iteration loop holds no workgroup barrier: lane j owns the movable nodes first + j,
// first + j + 64, ...  The chain's state is private to its wave, in LDS:
//
//   W      [n_pad][K] float   the class sums of every node, kept up to date move by move   (n_pad = n_max up to 16)
//   until  [n_pad] uint32     the first iteration at which the node may move again
//   state  [n_pad] byte       the classes as they stand
//   snap   [n_pad] byte       the state of the largest cut so far
//
// n_pad * (4 K + 6) bytes per chain.  A 256-thread workgroup runs 4, 2 or 1 chains of ONE graph (tabu_layout: as many
// as fit), which share one staged copy of the graph's CSR in anneal_stage_csr's layout (starts, ids as uint16, vals);
// when the copy does not fit beside one chain, the chains read the batch's arrays in global memory - one template
// over LdsCsr / GlobalCsr (anneal_layout.h), so the arithmetic cannot differ.  The waves without a chain (slots < 4,
// or the last workgroup of a graph) wait at the closing barrier.
//
// An iteration: each lane scans its nodes (the W row, the class byte, until) for its best admissible move as ONE
// 64-bit key - the gain mapped to an order-preserving uint32 in the high half, ~(rank * K + k) in the low half; keys
// are unique, 0 means "none".  A node enters with its own best move only (the largest gain, the smallest k on ties: one
// subtraction and one compare per class, one key per node), and the scan has a wave-uniform trip count with
// unconditional loads, unrolled by two, so that the LDS reads of two nodes are in flight together - the first form, a
// key per (node, class) behind a branch on the class byte, took 4.0 us per iteration at n = 1000, K = 2 and 19.9 at
// K = 8, this one 2.6 and 10.6 (unrolled by four the compiler spilled 36 bytes of scratch).
// Then a 64-lane max butterfly on the VALU (v_permlane32/16_swap + DPP, as gmc::xor_add) gives
// every lane the winner, which is read straight from the key; then one lane per edge of the winner's row updates the
// neighbours' W rows (a row holds a neighbour once, so the read-modify-writes need no atomics).  The wave's own LDS
// traffic is ordered by wavefront-scope fences and wave barriers: no __syncthreads() inside the loop.
//
// The snapshot copy is deferred: an improving move only marks it pending; the state is copied before the first move
// that does not improve (and at the end), which gives the same bytes as copying at every improvement.
//
// After the chains the whole workgroup scores each of its snapshots with gmc::block_cut - 256 threads, the summation
// order of every other decoder, so the reported cuts carry the same bits - and writes them back; the second launch is
// the pick.  (The scoring is the tail of the chain launch and not a launch of its own: the pick needs every cut of a
// graph, so scoring and picking cannot share a launch without communication between workgroups, and this way the
// call stays at two launches with the snapshots scored out of LDS.)
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"
#include "move_body.h"
#include "anneal_layout.h"
#include "tabu_body.h"   // the layout, wave_sync, wave_max, ordered_bits / ordered_float: shared with kway_balance.hip

namespace {

using gmc::mix64;
using gmc::u64;
using gmc::GlobalCsr;
using gmc::LdsCsr;
using gmc::TabuLayout;
using gmc::tabu_layout;
using gmc::wave_sync;
using gmc::wave_max;
using gmc::ordered_bits;
using gmc::ordered_float;

struct TabuArgs {
    gmc_batch b;
    int first;               // first movable local id: K with terminals, 0 without
    int cands, iterations;
    unsigned tenure_base, tenure_span, tenure_div;
    u64 seed;
    signed char *assign;     // [cands][R], in/out
    float *cut_all;          // [B][cands]
    int *best_iter;          // [B][cands] or NULL
    int *moves;              // [B][cands] or NULL
    int slots, staged, n_pad, chain_bytes, off_starts, off_vals, off_ids;
};

// One chain on the calling wave: the table, the iterations, the snapshot left in sn.  lds: the chain's bytes.
template <int K, class G>
__device__ __forceinline__ void tabu_chain(const TabuArgs &a, const G &g, unsigned char *lds, int n, int cand,
                                           const signed char *in, int &best_it_out, int &moves_out) {
    const int lane = gmc::lane_id();
    float *W = reinterpret_cast<float *>(lds);
    unsigned *until = reinterpret_cast<unsigned *>(lds + (size_t)a.n_pad * K * 4);
    unsigned char *st = lds + (size_t)a.n_pad * (K * 4 + 4);
    unsigned char *sn = st + a.n_pad;
    const int first = a.first;
    const int n_mov = n - first;
    for (int l = lane; l < n; l += GMC_WAVE) {
        const unsigned char c = (unsigned char)in[l];
        st[l] = c;
        sn[l] = c;
        until[l] = 0u;
    }
    int best_it = 0, moves = 0;
    if (a.iterations > 0 && n_mov > 0) {
        wave_sync();
        for (int l = lane; l < n; l += GMC_WAVE) {
            const gmc::Sums<K> s = gmc::class_sums_k<K>(g.rp, g.col, g.vals, st, l);
#pragma unroll
            for (int k = 0; k < K; ++k) W[l * K + k] = s.m[k];
        }
        wave_sync();
        float rel = 0.0f, best = 0.0f;
        bool pending = false;   // the state is better than the snapshot and not copied yet
        const unsigned span = a.tenure_span + (a.tenure_div > 0 ? (unsigned)n_mov / a.tenure_div : 0u);
        const u64 base = a.seed + GMC_GOLD * (((u64)(unsigned)cand << 32) + 1ULL);   // it < 2^32 only adds
        const int trips = (n_mov + GMC_WAVE - 1) / GMC_WAVE;   // scan steps of a lane
        for (int it = 0; it < a.iterations; ++it) {
            const u64 h = mix64(base + GMC_GOLD * (u64)(unsigned)it);
            const int r = (int)((unsigned)h % (unsigned)n_mov);
            const unsigned tenure_draw = (unsigned)(h >> 32) % (span + 1u);
            // 2-3. the lane's best admissible move
            // (a wave-uniform trip count and unconditional loads from a clamped node, so that the unrolled steps' LDS
            // reads go out together: a lane past its last node reads node `first` and admits nothing)
            u64 key = 0;
#pragma unroll 2
            for (int t = 0; t < trips; ++t) {
                const int v0 = first + lane + (t << 6);
                const bool valid = v0 < n;
                const int v = valid ? v0 : first;
                const unsigned c = st[v];
                float w[K];
#pragma unroll
                for (int k = 0; k < K; ++k) w[k] = W[v * K + k];
                float wc = w[0];
#pragma unroll
                for (int j = 1; j < K; ++j) wc = c == (unsigned)j ? w[j] : wc;
                const bool is_free = until[v] <= (unsigned)it;
                int rank = v - first - r;
                rank = rank < 0 ? rank + n_mov : rank;
                // the node's own best move - the largest gain, the smallest k on ties - stands for all its moves: when
                // the node is banned, rel + gain is monotone in the gain, so if any of its moves is admissible this one is
                float bg = -__builtin_inff();
                int bk = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float gain = wc - w[k];
                    const bool take = c != (unsigned)k && gain > bg;
                    bg = take ? gain : bg;
                    bk = take ? k : bk;
                }
                // (a byte of no class: the node never moves)
                const bool adm = valid && c < (unsigned)K && (is_free || rel + bg > best);
                const u64 cnd = ((u64)ordered_bits(bg) << 32) | (u64)(~(unsigned)(rank * K + bk));
                key = adm && cnd > key ? cnd : key;
            }
            key = wave_max(key);
            const unsigned khi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key >> 32));
            const unsigned klo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key);
            if (khi == 0u && klo == 0u) continue;   // no admissible move (wave-uniform)
            const unsigned x = ~klo;
            const int k = (int)(x % (unsigned)K);
            int v = first + (int)(x / (unsigned)K) + r;
            v = v - first >= n_mov ? v - n_mov : v;
            const float gain = ordered_float(khi);
            const float new_rel = rel + gain;
            const bool improves = new_rel > best;
            if (!improves && pending) {   // the snapshot takes the state before this move
                const unsigned *s32 = reinterpret_cast<const unsigned *>(st);
                unsigned *d32 = reinterpret_cast<unsigned *>(sn);
                for (int i = lane; i < (a.n_pad >> 2); i += GMC_WAVE) d32[i] = s32[i];
                pending = false;
                wave_sync();
            }
            // 4. apply
            gmc::apply_move<K>(g, W, st, v, st[v], k, lane);
            if (lane == 0) {
                until[v] = gmc::ban_until(it, a.tenure_base, tenure_draw);
            }
            rel = new_rel;
            ++moves;
            // 5. best so far
            if (improves) {
                best = rel;
                best_it = it + 1;
                pending = true;
            }
            wave_sync();
        }
        if (pending) {
            const unsigned *s32 = reinterpret_cast<const unsigned *>(st);
            unsigned *d32 = reinterpret_cast<unsigned *>(sn);
            for (int i = lane; i < (a.n_pad >> 2); i += GMC_WAVE) d32[i] = s32[i];
        }
    }
    best_it_out = best_it;
    moves_out = moves;
}

template <int K>
__global__ __launch_bounds__(256) void tabu_kernel(TabuArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    const int gi = blockIdx.y;
    const int r0 = a.b.goff[gi];
    const int n = a.b.goff[gi + 1] - r0;
    if (n > a.b.n_max || n < (a.first > 1 ? a.first : 1)) return;   // (the LDS is sized by n_max; workgroup-uniform)
    const int wave = gmc::uniform((int)(threadIdx.x >> 6));
    const int cand0 = blockIdx.x * a.slots;
    const int cand = cand0 + wave;
    const int e0 = a.b.rowptr[r0];
    const int nnz = a.b.rowptr[r0 + n] - e0;
    // the copy is sized by n_max and nnz_max: a graph that contradicts them takes the global path
    const bool staged = a.staged && nnz >= 0 && nnz <= a.b.nnz_max;   // workgroup-uniform
    const bool runs = wave < a.slots && cand < a.cands;               // wave-uniform
    int best_it = 0, moves = 0;
    if (staged) {
        int *starts = reinterpret_cast<int *>(lds + a.off_starts);
        float *vals = a.b.vals ? reinterpret_cast<float *>(lds + a.off_vals) : nullptr;
        unsigned short *ids = reinterpret_cast<unsigned short *>(lds + a.off_ids);
        if (a.iterations > 0) {
            for (int l = threadIdx.x; l <= n; l += blockDim.x) starts[l] = a.b.rowptr[r0 + l] - e0;
            for (int e = threadIdx.x; e < nnz; e += blockDim.x) {
                ids[e] = (unsigned short)a.b.lcol[e0 + e];
                if (vals) vals[e] = a.b.vals[e0 + e];
            }
        }
        __syncthreads();
        if (runs) {
            const LdsCsr g{starts, ids, vals, nullptr, 0};
            tabu_chain<K>(a, g, lds + (size_t)wave * a.chain_bytes, n, cand, a.assign + (long)cand * a.b.R + r0,
                          best_it, moves);
        }
    } else if (runs) {
        const GlobalCsr g{a.b.rowptr + r0, a.b.lcol, a.b.vals, nullptr, r0, a.first};
        tabu_chain<K>(a, g, lds + (size_t)wave * a.chain_bytes, n, cand, a.assign + (long)cand * a.b.R + r0,
                      best_it, moves);
    }
    if (runs && gmc::lane_id() == 0) {
        if (a.best_iter) a.best_iter[(long)gi * a.cands + cand] = best_it;
        if (a.moves) a.moves[(long)gi * a.cands + cand] = moves;
    }
    __syncthreads();   // every chain of the workgroup has left its snapshot
    // the result and its score, chain by chain, the whole workgroup on each: scored as gmc_refine_local_f32 scores
    for (int s = 0; s < a.slots; ++s) {
        const int cs = cand0 + s;
        if (cs >= a.cands) break;   // workgroup-uniform
        const unsigned char *sn = lds + (size_t)s * a.chain_bytes + (size_t)a.n_pad * (K * 4 + 5);
        signed char *as = a.assign + (long)cs * a.b.R + r0;
        for (int l = threadIdx.x; l < n; l += blockDim.x) as[l] = (signed char)sn[l];
        const float cut = gmc::block_cut(a.b, sn, r0, n, red);
        if (threadIdx.x == 0) a.cut_all[(long)gi * a.cands + cs] = cut;
        __syncthreads();   // thread 0 has read red before the next recount writes it
    }
}

struct TabuPickArgs {
    gmc::PickArgs p;
    int first;
};
__global__ __launch_bounds__(256) void tabu_pick_kernel(TabuPickArgs a) {
    const int g = blockIdx.x;
    const int n = a.p.b.goff[g + 1] - a.p.b.goff[g];
    if (n > a.p.b.n_max || n < (a.first > 1 ? a.first : 1)) return;   // workgroup-uniform: the graphs the chains skipped
    gmc::pick_best(a.p);
}

}  // namespace

extern "C" int gmc_kway_tabu_fits(const gmc_batch *batch, int32_t K) {
    return gmc::chain_query(batch, K, false);
}

extern "C" int gmc_kway_tabu_shape(const gmc_batch *batch, int32_t K) {
    return gmc::chain_query(batch, K, true);
}

extern "C" int gmc_kway_tabu_f32(const gmc_batch *batch, int32_t K, int32_t terminals, int32_t cands, int8_t *assign,
                                 int32_t iterations, int32_t tenure_base, int32_t tenure_span, int32_t tenure_div,
                                 uint64_t seed, float *cut_all, int32_t *best_assign, float *best_cut,
                                 int32_t *best_idx, int32_t *best_iter, int32_t *moves, gmc_stream_t stream) {
    if (!batch || !assign || !cut_all || !best_assign || !best_cut || !best_idx) return GMC_ERR_NULL;
    int first;
    TabuLayout L;
    int rc = gmc::chain_checks(batch, K, terminals, cands, iterations, tenure_base, tenure_span, tenure_div, first,
                               L);
    if (rc != GMC_OK || batch->B == 0) return rc;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const TabuArgs a{*batch, first, cands, iterations, (unsigned)tenure_base, (unsigned)tenure_span,
                     (unsigned)tenure_div, seed, reinterpret_cast<signed char *>(assign), cut_all, best_iter, moves,
                     L.slots, L.staged, L.n_pad, L.chain_bytes, L.off_starts, L.off_vals, L.off_ids};
    GMC_KWAY_DISPATCH(K, rc = gmc::chain_launch(tabu_kernel<KK>, a, L.bytes, st));
    if (rc != GMC_OK) return rc;
    const TabuPickArgs p{{*batch, cands, reinterpret_cast<const signed char *>(assign), cut_all, best_assign, best_cut,
                          best_idx}, first};
    hipLaunchKernelGGL(tabu_pick_kernel, dim3(batch->B), dim3(256), 0, st, p);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
