// The seeded sampler and the annealing (with its descent) for graphs that do not fit one workgroup's LDS
// (gmc_large_sample_seeded_f32, gmc_large_anneal_f32: K = 2..8, up to GMC_LARGE_MAX_GRAPH_NODES nodes per graph).  The
// rules are kway_search.hip's, stated in include/gcnmaxcut.h; a draw and a node's visit are the same functions
// (draw_body.h, move_body.h), so on a graph both can run the class bytes, snapshots and sweep counts are those kernels'.
//
// As in large_round.hip a graph is shared by several workgroups, its state lives in the caller's workspace (not assumed
// zeroed: every word read is written by the call first) and kernel boundaries are the only synchronisation between
// workgroups: no spin waits, no arrival counters, no atomics.  Rows are batch row ids, neighbours are read through gcol.
//
// State: the class bytes of all candidates of a row side by side, [chunks][R][cp] with cp = min(64, the next power of
// two >= cands) and chunks = ceil(cands / cp); candidate c is lane c % cp of chunk c / cp.  In the launches that visit
// nodes a wave holds 64 / cp nodes times cp candidates: its lanes read a node's rowptr / gcol / vals entries at one
// address each (one request for up to 64 candidates, where a thread per (candidate, node) over [cands][R] would
// fetch the row once per candidate) and every neighbour's bytes as one contiguous run of cp bytes.  A workgroup of 256
// threads visits kPasses * 256 / cp nodes.  The caller's [cands][R] is transposed on the way in (init) and out (score).
//
//   init      state (and snapshot) from assign; per (graph, candidate) moved = swept = snap = take = 0, stopped = the
//             graph is one the call skips; the word `done` = 0
//   recount   a row's share of the cut of G = min(cp, 8) candidates (their bytes one load), a tile of kTile rows by
//             block_sum to part[slot][candidate]; the score launch also writes the bytes to assign [cands][R]
//   fold      per (graph, candidate): its tiles' slots ascending, * 0.5f; then first: best = cut; sweep: take = cut > best
//             (then best = cut, snap = s + 1); score: cut_all, sweeps, snap_sweep
//   snapshot  the rows of every (graph, candidate) with take set: snapshot = state
//   anneal    one launch per colour: the annealing visit of that colour's nodes of every graph and candidate
//   descend   one launch per colour (the local search's rule; a move sets moved of its (graph, candidate) by a plain
//             store of 1), then close: per (graph, candidate) not yet stopped swept += 1, stopped = !moved, moved = 0;
//             done = all have stopped.  Lanes of a stopped pair return at once; with `done` set a launch returns after
//             reading that one word.  After annealing sweeps the descent runs in the snapshot's bytes (no copy back).
//   pick      per graph the strictly best candidate, the first on ties; copy: its bytes from assign to best_assign
//   sampler   draw (the state written from the hash), recount (also to assign_all when given), fold, pick, regenerate
//
// Grids: the graph is the x dimension; y is the tile (of kTile rows in recount / copy / regenerate: at most 4096; of
// kPasses * 256 / cp rows or nodes of a colour class elsewhere: at most 32768); z walks the chunks (recount: the groups
// of G candidates) with a stride, so any candidate count fits.  Tiles past a graph's (a class's) end return at once, so
// a graph's results do not depend on what else is in the batch.  The slots of graph g: goff[g] / 256 + g onwards.
//
// Summation order of every cut, fixed: a row by its one thread in CSR order; a tile by block_sum (a butterfly per wave,
// the four waves ascending); a graph's tiles ascending.
#include "kway_rows.h"
#include "draw_body.h"
#include "mix64.h"
#include "move_body.h"

namespace {

using gmc::mix64;
using gmc::Sums;
using gmc::u64;

constexpr int kTile = 256;
constexpr int kWaves = kTile / GMC_WAVE;
constexpr int kPasses = 8;        // nodes a lane group visits in one launch
constexpr int kMaxZ = 65535;
constexpr int kWideCands = 1 << 24;   // the 24-bit candidate field of the counter of a graph beyond GMC_MAX_GRAPH_NODES

enum { kFoldFirst = 0, kFoldSweep = 1, kFoldScore = 2 };

struct Flags {      // the int words of the workspace, [B * cands] each
    int *moved, *stopped, *swept, *snap, *take;
    int *done;      // one word
};

struct SearchArgs {
    gmc_batch b;
    int K;
    int first;                       // first movable local id: K with terminals, 0 without
    const int *order, *cgoff, *cptr;
    int cands, lcp, chunks;          // cp = 1 << lcp
    unsigned char *sa;               // [chunks][R][cp] workspace: the state the node launches move
    unsigned char *sb;               // likewise: the snapshot
    Flags f;
    float *best;                     // [B * cands] workspace: the cut of the snapshot
    float *part;                     // [R / 256 + B + 1][chunks * cp] workspace
    const float *inv_temp, *levels;
    u64 seed;
    signed char *assign;             // [cands][R]: the caller's candidates (the sampler: assign_all or NULL)
    float *cut_all;                  // [B][cands]
    int *snap_out, *sweeps_out;      // [B][cands] or NULL
    int *best_assign;                // [R]
    float *best_cut;                 // [B]
    int *best_idx;                   // [B]
    const float *P;                  // [R][K]   (the sampler)
    const u64 *gkey;                 // [B]      (the sampler)
    int colour, sweep;               // of a colour launch / a sweep's fold
};

// the class bytes of one candidate: node u's byte is cp bytes after node u - 1's
struct CandBytes {
    const unsigned char *p;
    int lcp;
    __device__ __forceinline__ int operator[](int u) const { return p[(long)u << lcp]; }
};

// the graph of this workgroup and whether the call runs it (a graph with fewer than `first` or more than n_max nodes is skipped)
struct Graph { int g, r0, n; bool runs; };
__device__ __forceinline__ Graph my_graph(const SearchArgs &a) {
    Graph t;
    t.g = blockIdx.x;
    t.r0 = a.b.goff[t.g];
    t.n = a.b.goff[t.g + 1] - t.r0;
    t.runs = t.n >= a.first && t.n <= a.b.n_max;
    return t;
}

// this thread's place in the launches that hold candidates along the lanes
struct Lane { int cl, sub, npp; };   // candidate within the chunk, node within the pass, nodes per pass
__device__ __forceinline__ Lane my_lane(const SearchArgs &a) {
    return Lane{(int)threadIdx.x & ((1 << a.lcp) - 1), (int)threadIdx.x >> a.lcp, kTile >> a.lcp};
}
__device__ __forceinline__ long state_index(const SearchArgs &a, int chunk, int r, int cl) {
    return ((((long)chunk * a.b.R) + r) << a.lcp) + cl;
}

__global__ __launch_bounds__(kTile) void large_search_init_kernel(SearchArgs a, int with_snapshot) {
    const Graph t = my_graph(a);
    const Lane q = my_lane(a);
    for (int chunk = blockIdx.z; chunk < a.chunks; chunk += gridDim.z) {
        const int cand = (chunk << a.lcp) + q.cl;
        if (blockIdx.y == 0 && q.sub == 0 && cand < a.cands) {
            const long i = (long)t.g * a.cands + cand;
            a.f.moved[i] = 0;
            a.f.swept[i] = 0;
            a.f.snap[i] = 0;
            a.f.take[i] = 0;
            a.f.stopped[i] = t.runs ? 0 : 1;
            if (i == 0) *a.f.done = 0;
        }
        if (!t.runs) continue;
        for (int pass = 0; pass < kPasses; ++pass) {
            const int l = ((int)blockIdx.y * kPasses + pass) * q.npp + q.sub;
            if (l >= t.n) break;
            const int r = t.r0 + l;
            const unsigned char c = cand < a.cands ? (unsigned char)a.assign[(long)cand * a.b.R + r] : (unsigned char)0;
            const long i = state_index(a, chunk, r, q.cl);
            a.sa[i] = c;
            if (with_snapshot) a.sb[i] = c;
        }
    }
}

template <int K>
__global__ __launch_bounds__(kTile) void large_sample_draw_kernel(SearchArgs a) {
    const Graph t = my_graph(a);
    if (!t.runs) return;
    const Lane q = my_lane(a);
    const u64 key = a.gkey[t.g];
    for (int chunk = blockIdx.z; chunk < a.chunks; chunk += gridDim.z) {
        const int it = (chunk << a.lcp) + q.cl;
        const u64 base = gmc::iteration_base(key, it);
        for (int pass = 0; pass < kPasses; ++pass) {
            const int l = ((int)blockIdx.y * kPasses + pass) * q.npp + q.sub;
            if (l >= t.n) break;
            const int r = t.r0 + l;
            int c = 0;
            if (it < a.cands) c = l < a.first ? l : gmc::seeded_class_k<K>(base, l, a.P + (long)r * K);
            a.sa[state_index(a, chunk, r, q.cl)] = (unsigned char)c;
        }
    }
}

// the bytes of G neighbouring candidates of a row as one load, candidate j in bits 8 j .. 8 j + 7
template <int G>
__device__ __forceinline__ u64 load_group(const unsigned char *p) {
    if constexpr (G == 8) return *reinterpret_cast<const u64 *>(p);
    else if constexpr (G == 4) return *reinterpret_cast<const unsigned *>(p);
    else if constexpr (G == 2) return *reinterpret_cast<const unsigned short *>(p);
    else return *p;
}

// `out` (NULL: none) receives the bytes of the state as [cands][R]
template <int G>
__global__ __launch_bounds__(kTile) void large_search_recount_kernel(SearchArgs a, const unsigned char *state,
                                                                     signed char *out) {
    __shared__ float red[kWaves * G];
    const Graph t = my_graph(a);
    if (!t.runs || (int)blockIdx.y * kTile >= t.n) return;   // (workgroup-uniform)
    const int l = (int)blockIdx.y * kTile + (int)threadIdx.x;
    const int r = t.r0 + l;
    const long cpad = (long)a.chunks << a.lcp;
    const long slot = (long)(t.r0 / kTile) + t.g + blockIdx.y;
    for (long grp = blockIdx.z; grp < cpad / G; grp += gridDim.z) {   // (workgroup-uniform)
        const long c0 = grp * G;
        const unsigned char *base = state + state_index(a, (int)(c0 >> a.lcp), 0, (int)c0 & ((1 << a.lcp) - 1));
        float v[G];
#pragma unroll
        for (int j = 0; j < G; ++j) v[j] = 0.f;
        if (l < t.n) {
            const u64 me = load_group<G>(base + ((long)r << a.lcp));
            if (out) {
#pragma unroll
                for (int j = 0; j < G; ++j)
                    if (c0 + j < a.cands) out[(long)(c0 + j) * a.b.R + r] = (signed char)(me >> (8 * j));
            }
            const int e1 = a.b.rowptr[r + 1];
            for (int e = a.b.rowptr[r]; e < e1; ++e) {
                const float w = a.b.vals ? a.b.vals[e] : 1.0f;
                const u64 x = load_group<G>(base + ((long)a.b.gcol[e] << a.lcp)) ^ me;
#pragma unroll
                for (int j = 0; j < G; ++j) v[j] += ((x >> (8 * j)) & 0xff) != 0 ? w : 0.f;
            }
        }
        block_sum<G, kWaves>(v, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int j = 0; j < G; ++j) a.part[slot * cpad + c0 + j] = v[j];
        }
        __syncthreads();   // thread 0 has read red before the next group's waves write it
    }
}

// one thread per (graph, candidate)
__global__ __launch_bounds__(kTile) void large_search_fold_kernel(SearchArgs a, int mode) {
    const long i = (long)blockIdx.x * kTile + threadIdx.x;
    if (i >= (long)a.b.B * a.cands) return;
    const int g = (int)(i / a.cands);
    const int cand = (int)(i - (long)g * a.cands);
    const int r0 = a.b.goff[g], n = a.b.goff[g + 1] - r0;
    if (n < a.first || n > a.b.n_max) return;
    const int tiles = (n + kTile - 1) / kTile;
    const long cpad = (long)a.chunks << a.lcp;
    const float *p = a.part + ((long)(r0 / kTile) + g) * cpad + cand;
    float s = 0.f;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) s += p[t * cpad];
    const float cut = s * 0.5f;
    if (mode == kFoldFirst) {
        a.best[i] = cut;
    } else if (mode == kFoldSweep) {
        const int better = cut > a.best[i];
        if (better) {
            a.best[i] = cut;
            a.f.snap[i] = a.sweep + 1;
        }
        a.f.take[i] = better;
    } else {
        a.cut_all[i] = cut;
        if (a.sweeps_out) a.sweeps_out[i] = a.f.swept[i];
        if (a.snap_out) a.snap_out[i] = a.f.snap[i];
    }
}

__global__ __launch_bounds__(kTile) void large_search_snapshot_kernel(SearchArgs a) {
    const Graph t = my_graph(a);
    if (!t.runs) return;
    const Lane q = my_lane(a);
    for (int chunk = blockIdx.z; chunk < a.chunks; chunk += gridDim.z) {
        const int cand = (chunk << a.lcp) + q.cl;
        if (cand >= a.cands || !a.f.take[(long)t.g * a.cands + cand]) continue;
        for (int pass = 0; pass < kPasses; ++pass) {
            const int l = ((int)blockIdx.y * kPasses + pass) * q.npp + q.sub;
            if (l >= t.n) break;
            const long i = state_index(a, chunk, t.r0 + l, q.cl);
            a.sb[i] = a.sa[i];
        }
    }
}

// the entries of order this workgroup visits in a colour launch: lo + pass * npp + sub for pass = 0 .. kPasses - 1,
// below hi (lo >= hi: none)
struct ColourRange { long lo; int hi; };
__device__ __forceinline__ ColourRange colour_range(const SearchArgs &a, const Graph &t, const Lane &q) {
    const int k0 = a.cgoff[t.g];
    const int classes = a.cgoff[t.g + 1] - k0 - 1;
    if (a.colour >= classes) return ColourRange{0, 0};
    return ColourRange{(long)a.cptr[k0 + a.colour] + (long)blockIdx.y * kPasses * q.npp + q.sub, a.cptr[k0 + a.colour + 1]};
}

template <int K>
__global__ __launch_bounds__(kTile) void large_anneal_colour_kernel(SearchArgs a) {
    const Graph t = my_graph(a);
    if (!t.runs) return;
    const Lane q = my_lane(a);
    const ColourRange cr = colour_range(a, t, q);
    if (cr.lo >= cr.hi) return;
    const float inv_t = a.inv_temp[a.sweep];
    const bool wide = t.n > GMC_MAX_GRAPH_NODES;   // the counter layout is chosen by the graph's own node count
    for (int chunk = blockIdx.z; chunk < a.chunks; chunk += gridDim.z) {
        const int cand = (chunk << a.lcp) + q.cl;
        if (cand >= a.cands) continue;
        // seed + GOLD * (ctr + 1) without the node (v below 2^12 / 2^20 only adds)
        const u64 ctr = wide ? ((u64)(unsigned)cand << 40) | ((u64)(unsigned)a.sweep << 20)
                             : ((u64)(unsigned)cand << 32) | ((u64)(unsigned)a.sweep << 12);
        const u64 base = a.seed + GMC_GOLD * (ctr + 1ULL);
        unsigned char *mine = a.sa + state_index(a, chunk, 0, q.cl);
        const CandBytes cls{mine, a.lcp};
        for (int pass = 0; pass < kPasses; ++pass) {
            const long i = cr.lo + (long)pass * q.npp;
            if (i >= cr.hi) break;
            const int r = a.order[i];
            const int l = r - t.r0;
            if (l < a.first || l >= t.n) continue;   // not a movable row of this graph: never touch the state for it
            const Sums<K> w = gmc::class_sums_k<K>(a.b.rowptr, a.b.gcol, a.b.vals, cls, r);
            const u64 h = mix64(base + GMC_GOLD * (u64)(unsigned)l);
            int kk;
            if (gmc::anneal_move<K>(w, cls[r], inv_t, a.levels, h, kk)) mine[(long)r << a.lcp] = (unsigned char)kk;
        }
    }
}

// `state`: the bytes the descent moves (the snapshot's after annealing sweeps)
template <int K>
__global__ __launch_bounds__(kTile) void large_search_descent_colour_kernel(SearchArgs a, unsigned char *state) {
    if (*a.f.done) return;
    const Graph t = my_graph(a);
    if (!t.runs) return;
    const Lane q = my_lane(a);
    const ColourRange cr = colour_range(a, t, q);
    if (cr.lo >= cr.hi) return;
    for (int chunk = blockIdx.z; chunk < a.chunks; chunk += gridDim.z) {
        const int cand = (chunk << a.lcp) + q.cl;
        if (cand >= a.cands) continue;
        const long pair = (long)t.g * a.cands + cand;
        if (a.f.stopped[pair]) continue;
        unsigned char *mine = state + state_index(a, chunk, 0, q.cl);
        const CandBytes cls{mine, a.lcp};
        for (int pass = 0; pass < kPasses; ++pass) {
            const long i = cr.lo + (long)pass * q.npp;
            if (i >= cr.hi) break;
            const int r = a.order[i];
            const int l = r - t.r0;
            if (l < a.first || l >= t.n) continue;
            const Sums<K> s = gmc::class_sums_k<K>(a.b.rowptr, a.b.gcol, a.b.vals, cls, r);
            const float wc = gmc::own_sum_or_inf<K>(s, cls[r]);
            float wk;
            const int kk = gmc::smallest<K>(s, wk);
            if (wk < wc) {
                mine[(long)r << a.lcp] = (unsigned char)kk;
                a.f.moved[pair] = 1;
            }
        }
    }
}

// one workgroup: closes the sweep of every (graph, candidate)
__global__ __launch_bounds__(kTile) void large_search_close_kernel(Flags f, long pairs) {
    if (*f.done) return;
    int live = 0;
    for (long i = threadIdx.x; i < pairs; i += kTile) {
        if (f.stopped[i]) continue;
        f.swept[i] += 1;
        if (f.moved[i]) live = 1;
        else f.stopped[i] = 1;
        f.moved[i] = 0;
    }
    live = __syncthreads_or(live);
    if (threadIdx.x == 0 && !live) *f.done = 1;
}

// one thread per graph: the strictly best of its candidates' cuts, the first on ties
__global__ __launch_bounds__(kTile) void large_search_pick_kernel(SearchArgs a) {
    const int g = (int)blockIdx.x * kTile + (int)threadIdx.x;
    if (g >= a.b.B) return;
    const int n = a.b.goff[g + 1] - a.b.goff[g];
    if (n < a.first || n > a.b.n_max) return;
    const float *c = a.cut_all + (long)g * a.cands;
    int bi = 0;
    float bc = c[0];
    for (int i = 1; i < a.cands; ++i)
        if (c[i] > bc) { bc = c[i]; bi = i; }
    a.best_cut[g] = bc;
    a.best_idx[g] = bi;
}

__global__ __launch_bounds__(kTile) void large_search_copy_kernel(SearchArgs a) {
    const Graph t = my_graph(a);
    const int l = (int)blockIdx.y * kTile + (int)threadIdx.x;
    if (!t.runs || l >= t.n) return;
    a.best_assign[t.r0 + l] = a.assign[(long)a.best_idx[t.g] * a.b.R + t.r0 + l];
}

// the winning sample again from the hash (never read from assign_all)
template <int K>
__global__ __launch_bounds__(kTile) void large_sample_regenerate_kernel(SearchArgs a) {
    const Graph t = my_graph(a);
    const int l = (int)blockIdx.y * kTile + (int)threadIdx.x;
    if (!t.runs || l >= t.n) return;
    const u64 base = gmc::iteration_base(a.gkey[t.g], a.best_idx[t.g]);
    a.best_assign[t.r0 + l] = l < a.first ? l : gmc::seeded_class_k<K>(base, l, a.P + (long)(t.r0 + l) * K);
}

// ---- host ---------------------------------------------------------------------------------------------------------------

size_t pad4(size_t words) { return (words + 3) & ~(size_t)3; }
size_t pad16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

struct Layout {
    int lcp;
    size_t chunks, cpad, pairs, flag_words, best_words, part_words, state_bytes, bytes;
};
Layout layout(const gmc_batch *b, int cands) {
    Layout L{};
    while ((1 << L.lcp) < cands && L.lcp < 6) ++L.lcp;
    L.chunks = ((size_t)cands - 1) / ((size_t)1 << L.lcp) + 1;
    L.cpad = L.chunks << L.lcp;
    L.pairs = (size_t)b->B * (size_t)cands;
    L.flag_words = pad4(5 * L.pairs + 1);
    L.best_words = pad4(L.pairs);
    L.part_words = pad4(((size_t)b->R / kTile + (size_t)b->B + 1) * L.cpad);
    L.state_bytes = pad16(L.cpad * (size_t)b->R);
    L.bytes = 4 * (L.flag_words + L.best_words + L.part_words) + 2 * L.state_bytes;
    return L;
}

// the workspace's arrays into the arguments
void carve(SearchArgs &a, const Layout &L, void *workspace) {
    int *words = static_cast<int *>(workspace);
    a.f = Flags{words, words + L.pairs, words + 2 * L.pairs, words + 3 * L.pairs, words + 4 * L.pairs, words + 5 * L.pairs};
    a.best = reinterpret_cast<float *>(words + L.flag_words);
    a.part = a.best + L.best_words;
    a.sa = reinterpret_cast<unsigned char *>(a.part + L.part_words);
    a.sb = a.sa + L.state_bytes;
    a.lcp = L.lcp;
    a.chunks = (int)L.chunks;
}

struct Grids {
    dim3 block, lanes, nodes, rows, pairs, graphs;
    int groups_z;   // z of a recount launch
};
Grids grids(const SearchArgs &a, const Layout &L, int G) {
    Grids g;
    const int per = kPasses * (kTile >> a.lcp);   // rows (nodes of a class) of a workgroup with candidates along the lanes
    const int z = (int)(L.chunks < (size_t)kMaxZ ? L.chunks : (size_t)kMaxZ);
    const int class_tiles = (a.b.n_max - a.first + per - 1) / per;   // a colour class has at most n_max - first nodes
    g.block = dim3(kTile);
    g.lanes = dim3(a.b.B, (a.b.n_max + per - 1) / per, z);
    g.nodes = dim3(a.b.B, class_tiles > 0 ? class_tiles : 1, z);
    g.rows = dim3(a.b.B, (a.b.n_max + kTile - 1) / kTile);
    g.pairs = dim3((unsigned)((L.pairs + kTile - 1) / kTile));
    g.graphs = dim3((a.b.B + kTile - 1) / kTile);
    const size_t groups = L.cpad / (size_t)G;
    g.groups_z = (int)(groups < (size_t)kMaxZ ? groups : (size_t)kMaxZ);
    return g;
}

int recount_launch(const SearchArgs &a, const Grids &g, const unsigned char *state, signed char *out, hipStream_t st) {
    const dim3 grid(g.rows.x, g.rows.y, g.groups_z);
    switch (a.lcp) {
        case 0: hipLaunchKernelGGL(large_search_recount_kernel<1>, grid, g.block, 0, st, a, state, out); break;
        case 1: hipLaunchKernelGGL(large_search_recount_kernel<2>, grid, g.block, 0, st, a, state, out); break;
        case 2: hipLaunchKernelGGL(large_search_recount_kernel<4>, grid, g.block, 0, st, a, state, out); break;
        default: hipLaunchKernelGGL(large_search_recount_kernel<8>, grid, g.block, 0, st, a, state, out); break;
    }
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
int group_of(int lcp) { return lcp < 3 ? 1 << lcp : 8; }

int fold_launch(const SearchArgs &a, const Grids &g, int mode, hipStream_t st) {
    hipLaunchKernelGGL(large_search_fold_kernel, g.pairs, g.block, 0, st, a, mode);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

template <int K>
int sample_launch(SearchArgs a, const Layout &L, hipStream_t st) {
    const Grids g = grids(a, L, group_of(a.lcp));
    GmcProbeScope probe(GMC_K_SAMPLE, st);
    hipLaunchKernelGGL(large_sample_draw_kernel<K>, g.lanes, g.block, 0, st, a);
    GMC_LAUNCH_CHECK();
    int rc = recount_launch(a, g, a.sa, a.assign, st);
    if (rc != GMC_OK) return rc;
    rc = fold_launch(a, g, kFoldScore, st);
    if (rc != GMC_OK) return rc;
    hipLaunchKernelGGL(large_search_pick_kernel, g.graphs, g.block, 0, st, a);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(large_sample_regenerate_kernel<K>, g.rows, g.block, 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

template <int K>
int anneal_launch(SearchArgs a, const Layout &L, int max_classes, int anneal_sweeps, int max_descent_sweeps,
                  hipStream_t st) {
    const Grids g = grids(a, L, group_of(a.lcp));
    GmcProbeScope probe(GMC_K_REFINE, st);
    int rc;
    hipLaunchKernelGGL(large_search_init_kernel, g.lanes, g.block, 0, st, a, anneal_sweeps > 0 ? 1 : 0);
    GMC_LAUNCH_CHECK();
    if (anneal_sweeps > 0) {
        if ((rc = recount_launch(a, g, a.sa, nullptr, st)) != GMC_OK) return rc;
        if ((rc = fold_launch(a, g, kFoldFirst, st)) != GMC_OK) return rc;
        for (a.sweep = 0; a.sweep < anneal_sweeps; ++a.sweep) {
            for (a.colour = 0; a.colour < max_classes; ++a.colour) {
                hipLaunchKernelGGL(large_anneal_colour_kernel<K>, g.nodes, g.block, 0, st, a);
                GMC_LAUNCH_CHECK();
            }
            if ((rc = recount_launch(a, g, a.sa, nullptr, st)) != GMC_OK) return rc;
            if ((rc = fold_launch(a, g, kFoldSweep, st)) != GMC_OK) return rc;
            hipLaunchKernelGGL(large_search_snapshot_kernel, g.lanes, g.block, 0, st, a);
            GMC_LAUNCH_CHECK();
        }
    }
    unsigned char *state = anneal_sweeps > 0 ? a.sb : a.sa;   // the descent starts from the snapshot
    for (int s = 0; s < max_descent_sweeps; ++s) {
        for (a.colour = 0; a.colour < max_classes; ++a.colour) {
            hipLaunchKernelGGL(large_search_descent_colour_kernel<K>, g.nodes, g.block, 0, st, a, state);
            GMC_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(large_search_close_kernel, dim3(1), g.block, 0, st, a.f, (long)L.pairs);
        GMC_LAUNCH_CHECK();
    }
    if ((rc = recount_launch(a, g, state, a.assign, st)) != GMC_OK) return rc;
    if ((rc = fold_launch(a, g, kFoldScore, st)) != GMC_OK) return rc;
    hipLaunchKernelGGL(large_search_pick_kernel, g.graphs, g.block, 0, st, a);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(large_search_copy_kernel, g.rows, g.block, 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

bool sizes_ok(const gmc_batch *b, int32_t K, int32_t cands) {
    return b && b->abi == GMC_VERSION && K >= 2 && K <= GMC_KWAY_MAX_CLASSES && cands >= 1 && b->B >= 0 && b->R >= 0;
}

}  // namespace

extern "C" size_t gmc_large_search_workspace_bytes(const gmc_batch *batch, int32_t K, int32_t cands) {
    return sizes_ok(batch, K, cands) ? layout(batch, cands).bytes : 0;
}

// what gmc_large_sample_seeded_f32 and its _t twin do (terminals: 0 or 1)
static int large_sample_seeded(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals, const uint64_t *gkey,
                               int32_t iters, int8_t *assign_all, void *workspace, size_t workspace_bytes,
                               float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_iter,
                               gmc_stream_t stream) {
    if (!batch || !P || !gkey || !workspace || !cut_all || !best_assign || !best_cut || !best_iter) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol || !batch->gcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (iters < 1 || batch->B < 0 || (terminals != 0 && terminals != 1)) return GMC_ERR_SHAPE;
    const int first = terminals ? K : 0;
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || batch->n_max > GMC_LARGE_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    if (batch->R < 0) return GMC_ERR_WORKSPACE;
    const Layout L = layout(batch, iters);
    if (workspace_bytes < L.bytes) return GMC_ERR_WORKSPACE;
    if (batch->B == 0) return GMC_OK;
    SearchArgs a{};
    a.b = *batch;
    a.K = K;
    a.first = first;
    a.cands = iters;
    a.assign = reinterpret_cast<signed char *>(assign_all);
    a.cut_all = cut_all;
    a.best_assign = best_assign;
    a.best_cut = best_cut;
    a.best_idx = best_iter;
    a.P = P;
    a.gkey = reinterpret_cast<const u64 *>(gkey);
    carve(a, L, workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMC_KWAY_DISPATCH(K, return sample_launch<KK>(a, L, st));
    return GMC_OK;
}

extern "C" int gmc_large_sample_seeded_f32(const gmc_batch *batch, const float *P, int32_t K, const uint64_t *gkey,
                                           int32_t iters, int8_t *assign_all, void *workspace, size_t workspace_bytes,
                                           float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_iter,
                                           gmc_stream_t stream) {
    return large_sample_seeded(batch, P, K, 1, gkey, iters, assign_all, workspace, workspace_bytes, cut_all, best_assign,
                               best_cut, best_iter, stream);
}

extern "C" int gmc_large_sample_seeded_t_f32(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals,
                                             const uint64_t *gkey, int32_t iters, int8_t *assign_all, void *workspace,
                                             size_t workspace_bytes, float *cut_all, int32_t *best_assign,
                                             float *best_cut, int32_t *best_iter, gmc_stream_t stream) {
    return large_sample_seeded(batch, P, K, terminals, gkey, iters, assign_all, workspace, workspace_bytes, cut_all,
                               best_assign, best_cut, best_iter, stream);
}

// what gmc_large_anneal_f32 and its _t twin do (terminals: 0 or 1)
static int large_anneal(const gmc_batch *batch, int32_t K, int32_t terminals, const int32_t *order, const int32_t *cgoff,
                        const int32_t *cptr, int32_t max_classes, int32_t cands, int8_t *assign, const float *inv_temp,
                        int32_t anneal_sweeps, const float *levels, uint64_t seed, int32_t max_descent_sweeps,
                        void *workspace, size_t workspace_bytes, float *cut_all, int32_t *best_assign, float *best_cut,
                        int32_t *best_idx, int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !workspace || !assign || !cut_all || !best_assign || !best_cut || !best_idx)
        return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol || !batch->gcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (cands < 1 || anneal_sweeps < 0 || anneal_sweeps >= (1 << 20) || max_descent_sweeps < 0 || max_classes < 0 ||
        batch->B < 0 || (terminals != 0 && terminals != 1))
        return GMC_ERR_SHAPE;
    if (cands >= kWideCands && batch->n_max > GMC_MAX_GRAPH_NODES) return GMC_ERR_SHAPE;
    if (anneal_sweeps > 0 && (!inv_temp || !levels)) return GMC_ERR_NULL;
    const int first = terminals ? K : 0;
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || batch->n_max > GMC_LARGE_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    if (batch->R < 0) return GMC_ERR_WORKSPACE;
    const Layout L = layout(batch, cands);
    if (workspace_bytes < L.bytes) return GMC_ERR_WORKSPACE;
    if (batch->B == 0) return GMC_OK;
    SearchArgs a{};
    a.b = *batch;
    a.K = K;
    a.first = first;
    a.order = order;
    a.cgoff = cgoff;
    a.cptr = cptr;
    a.cands = cands;
    a.inv_temp = inv_temp;
    a.levels = levels;
    a.seed = seed;
    a.assign = reinterpret_cast<signed char *>(assign);
    a.cut_all = cut_all;
    a.snap_out = snap_sweep;
    a.sweeps_out = sweeps;
    a.best_assign = best_assign;
    a.best_cut = best_cut;
    a.best_idx = best_idx;
    carve(a, L, workspace);
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMC_KWAY_DISPATCH(K, return anneal_launch<KK>(a, L, max_classes, anneal_sweeps, max_descent_sweeps, st));
    return GMC_OK;
}

extern "C" int gmc_large_anneal_f32(const gmc_batch *batch, int32_t K, const int32_t *order, const int32_t *cgoff,
                                    const int32_t *cptr, int32_t max_classes, int32_t cands, int8_t *assign,
                                    const float *inv_temp, int32_t anneal_sweeps, const float *levels, uint64_t seed,
                                    int32_t max_descent_sweeps, void *workspace, size_t workspace_bytes, float *cut_all,
                                    int32_t *best_assign, float *best_cut, int32_t *best_idx, int32_t *snap_sweep,
                                    int32_t *sweeps, gmc_stream_t stream) {
    return large_anneal(batch, K, 1, order, cgoff, cptr, max_classes, cands, assign, inv_temp, anneal_sweeps, levels, seed,
                        max_descent_sweeps, workspace, workspace_bytes, cut_all, best_assign, best_cut, best_idx,
                        snap_sweep, sweeps, stream);
}

extern "C" int gmc_large_anneal_t_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const int32_t *order,
                                      const int32_t *cgoff, const int32_t *cptr, int32_t max_classes, int32_t cands,
                                      int8_t *assign, const float *inv_temp, int32_t anneal_sweeps, const float *levels,
                                      uint64_t seed, int32_t max_descent_sweeps, void *workspace, size_t workspace_bytes,
                                      float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_idx,
                                      int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream) {
    return large_anneal(batch, K, terminals, order, cgoff, cptr, max_classes, cands, assign, inv_temp, anneal_sweeps,
                        levels, seed, max_descent_sweeps, workspace, workspace_bytes, cut_all, best_assign, best_cut,
                        best_idx, snap_sweep, sweeps, stream);
}
