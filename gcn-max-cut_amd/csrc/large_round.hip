// The rounding by conditional expectations and the K-class local search for graphs that do not fit one workgroup's LDS
// (gmc_large_round_conditional_f32, gmc_large_local_search_f32: up to GMC_LARGE_MAX_GRAPH_NODES nodes per graph).  The
// rule is round.hip's and kway_search.hip's descent, stated in include/gcnmaxcut.h; the row sums are the same functions
// (round_body.h, move_body.h), so on a graph both can run the class bytes and the sweep counts are those kernels'.
//
// A graph is shared by several workgroups and its state lives in the caller's workspace: one class byte per batch row,
// kUnrounded marking a movable node the rounding has not visited yet (its state row is then its row of P; a rounded
// node's and a terminal's is the unit vector of its byte).  Rows are batch row ids, neighbours are read through gcol.
// Kernel boundaries are the only synchronisation between workgroups: no spin waits, no arrival counters, no atomics.
//
//   init      class bytes (terminals, markers / the caller's candidate), per graph moved = 0, swept = 0, stopped = the
//             graph is one the call skips; the word `done` = 0.  Every word of the workspace read later is written here.
//   expect    (expected given) a row's share of the expected cut over the unrounded state, a tile's sum to its slot
//   fold      per graph: its tiles' slots ascending, * 0.5f
//   round     one launch per colour: the nodes of that colour of every graph, one per thread; a thread reads the bytes
//             of its neighbours - none of its own colour - and writes its own
//   descend   per sweep one launch per colour (the local search's rule; a move sets the graph's `moved` by a plain
//             store of 1), then `close`: per graph not yet stopped swept += 1, stopped = !moved, moved = 0; done = every
//             graph has stopped.  Threads of a stopped graph return at once; with `done` set every later colour launch
//             returns after reading that one word.
//   score     a row's share of the cut count and its byte to assign, a tile's sum to its slot; fold as above (and sweeps)
//
// Grid of the row launches: (graph, tile of kTile = 256 rows of the graph); of the colour launches: (graph, tile of 256
// nodes of the graph's colour class).  The graph is the x dimension (up to 2^31 - 1), the tile the y dimension: at most
// GMC_LARGE_MAX_GRAPH_NODES / 256 = 4096.  Tiles past a graph's (a class's) end return at once, so a graph's results do
// not depend on what else is in the batch.  The slots of graph g: goff[g] / 256 + g onwards, as large.hip's.
//
// Summation orders, all fixed: a row by its one thread in CSR order (a hub row too: the byte contract fixes the order);
// a tile by block_sum (a butterfly per wave, the four waves ascending); a graph's tiles ascending.
#include "kway_rows.h"
#include "move_body.h"
#include "round_body.h"

namespace {

using gmc::Sums;

constexpr int kTile = 256;
constexpr int kWaves = kTile / GMC_WAVE;
constexpr unsigned char kUnrounded = 0xff;   // (no class: K <= 8)

struct Flags {      // the int words of the workspace
    int *moved;     // [B]
    int *stopped;   // [B]
    int *swept;     // [B]
    int *done;      // one word
};

struct LargeRoundArgs {
    gmc_batch b;
    const float *P;          // [R][K]; nullptr: the local search (the state starts from assign)
    int K;
    int first;               // first movable local id: K with terminals, 0 without
    const int *order, *cgoff, *cptr;
    unsigned char *cls;      // [R] workspace
    Flags f;
    float *part;             // [R / 256 + B + 1] workspace
    signed char *assign;     // [R]
    float *cut;              // [B]
    float *expected;         // [B] or NULL
    int *sweeps;             // [B] or NULL
    int colour;              // of a colour launch
};

// the state row of batch row u: its row of P while unrounded, the unit vector of its class byte afterwards
template <int K>
struct ByteState {
    const unsigned char *cls;
    const float *P;
    __device__ __forceinline__ void load(int u, float (&v)[K]) const {
        const int c = cls[u];
        if (c == kUnrounded) {
            const float *p = P + (long)u * K;
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = p[k];
        } else {
#pragma unroll
            for (int k = 0; k < K; ++k) v[k] = c == k ? 1.0f : 0.0f;
        }
    }
};

// the graph of this workgroup and whether the call runs it (a graph with fewer than `first` or more than n_max nodes is skipped)
struct Graph { int g, r0, n; bool runs; };
__device__ __forceinline__ Graph my_graph(const LargeRoundArgs &a) {
    Graph t;
    t.g = blockIdx.x;
    t.r0 = a.b.goff[t.g];
    t.n = a.b.goff[t.g + 1] - t.r0;
    t.runs = t.n >= a.first && t.n <= a.b.n_max;
    return t;
}
__device__ __forceinline__ long part_slot(const Graph &t) { return (long)(t.r0 / kTile) + t.g + blockIdx.y; }

// the batch row this thread visits in a colour launch, -1 for none
__device__ __forceinline__ int colour_row(const LargeRoundArgs &a, const Graph &t) {
    const int k0 = a.cgoff[t.g];
    const int classes = a.cgoff[t.g + 1] - k0 - 1;
    if (a.colour >= classes) return -1;
    const long i = (long)a.cptr[k0 + a.colour] + (long)blockIdx.y * kTile + threadIdx.x;
    if (i >= a.cptr[k0 + a.colour + 1]) return -1;
    const int r = a.order[i];
    const int l = r - t.r0;
    return l < a.first || l >= t.n ? -1 : r;   // not a movable row of this graph: never touch the state for it
}

__global__ __launch_bounds__(kTile) void large_round_init_kernel(LargeRoundArgs a) {
    const Graph t = my_graph(a);
    if (blockIdx.y == 0 && threadIdx.x == 0) {
        a.f.moved[t.g] = 0;
        a.f.swept[t.g] = 0;
        a.f.stopped[t.g] = t.runs ? 0 : 1;
        if (t.g == 0) *a.f.done = 0;
    }
    const int l = (int)blockIdx.y * kTile + (int)threadIdx.x;
    if (!t.runs || l >= t.n) return;
    const int r = t.r0 + l;
    a.cls[r] = a.P ? (l < a.first ? (unsigned char)l : kUnrounded) : (unsigned char)a.assign[r];
}

template <int K>
__global__ __launch_bounds__(kTile) void large_round_expect_kernel(LargeRoundArgs a) {
    __shared__ float red[kWaves];
    const Graph t = my_graph(a);
    if (!t.runs || (int)blockIdx.y * kTile >= t.n) return;   // (workgroup-uniform)
    const int l = (int)blockIdx.y * kTile + (int)threadIdx.x;
    float v[1] = {0.f};
    if (l < t.n) v[0] = gmc::expected_row<K>(a.b.rowptr, a.b.gcol, a.b.vals, ByteState<K>{a.cls, a.P}, t.r0 + l);
    block_sum<1, kWaves>(v, red);
    if (threadIdx.x == 0) a.part[part_slot(t)] = v[0];
}

// one thread per graph: out[g] = (its tiles' slots, ascending) * 0.5f; sweeps (score only): the descent sweeps run
__global__ __launch_bounds__(kTile) void large_round_fold_kernel(LargeRoundArgs a, float *out, int with_sweeps) {
    const int g = (int)blockIdx.x * kTile + (int)threadIdx.x;
    if (g >= a.b.B) return;
    const int r0 = a.b.goff[g], n = a.b.goff[g + 1] - r0;
    if (n < a.first || n > a.b.n_max) return;
    const int tiles = (n + kTile - 1) / kTile;
    const float *p = a.part + (long)(r0 / kTile) + g;
    float s = 0.f;
#pragma unroll 8
    for (int t = 0; t < tiles; ++t) s += p[t];
    out[g] = s * 0.5f;
    if (with_sweeps && a.sweeps) a.sweeps[g] = a.f.swept[g];
}

template <int K>
__global__ __launch_bounds__(kTile) void large_round_colour_kernel(LargeRoundArgs a) {
    const Graph t = my_graph(a);
    if (!t.runs) return;
    const int r = colour_row(a, t);
    if (r < 0) return;
    const Sums<K> s = gmc::state_sums<K>(a.b.rowptr, a.b.gcol, a.b.vals, ByteState<K>{a.cls, a.P}, r);
    float wk;
    a.cls[r] = (unsigned char)gmc::smallest<K>(s, wk);
}

template <int K>
__global__ __launch_bounds__(kTile) void large_descent_colour_kernel(LargeRoundArgs a) {
    if (*a.f.done) return;
    const Graph t = my_graph(a);
    if (a.f.stopped[t.g]) return;
    const int r = colour_row(a, t);
    if (r < 0) return;
    const Sums<K> s = gmc::class_sums_k<K>(a.b.rowptr, a.b.gcol, a.b.vals, a.cls, r);
    const float wc = gmc::own_sum_or_inf<K>(s, a.cls[r]);
    float wk;
    const int kk = gmc::smallest<K>(s, wk);
    if (wk < wc) {
        a.cls[r] = (unsigned char)kk;
        a.f.moved[t.g] = 1;
    }
}

// one workgroup: closes the sweep of every graph
__global__ __launch_bounds__(kTile) void large_descent_close_kernel(Flags f, int B) {
    if (*f.done) return;
    int live = 0;
    for (int g = threadIdx.x; g < B; g += kTile) {
        if (f.stopped[g]) continue;
        f.swept[g] += 1;
        if (f.moved[g]) live = 1;
        else f.stopped[g] = 1;
        f.moved[g] = 0;
    }
    live = __syncthreads_or(live);
    if (threadIdx.x == 0 && !live) *f.done = 1;
}

__global__ __launch_bounds__(kTile) void large_round_score_kernel(LargeRoundArgs a) {
    __shared__ float red[kWaves];
    const Graph t = my_graph(a);
    if (!t.runs || (int)blockIdx.y * kTile >= t.n) return;   // (workgroup-uniform)
    const int l = (int)blockIdx.y * kTile + (int)threadIdx.x;
    float v[1] = {0.f};
    if (l < t.n) {
        const int r = t.r0 + l;
        const int me = a.cls[r];
        a.assign[r] = (signed char)me;
        const int e1 = a.b.rowptr[r + 1];
        for (int e = a.b.rowptr[r]; e < e1; ++e) {
            const float w = a.b.vals ? a.b.vals[e] : 1.0f;
            v[0] += a.cls[a.b.gcol[e]] != me ? w : 0.f;
        }
    }
    block_sum<1, kWaves>(v, red);
    if (threadIdx.x == 0) a.part[part_slot(t)] = v[0];
}

size_t part_slots(const gmc_batch *b) { return ((size_t)b->R / kTile + (size_t)b->B + 1 + 3) & ~(size_t)3; }   // (padded too)
size_t flag_words(const gmc_batch *b) { return (3 * (size_t)b->B + 1 + 3) & ~(size_t)3; }   // a multiple of 16 bytes
size_t workspace_bytes(const gmc_batch *b) {
    return 4 * flag_words(b) + 4 * part_slots(b) + (((size_t)b->R + 15) & ~(size_t)15);
}

template <int K>
int large_round_launch(LargeRoundArgs a, int max_classes, int max_sweeps, hipStream_t st) {
    const dim3 block(kTile);
    const dim3 rows(a.b.B, (a.b.n_max + kTile - 1) / kTile);
    const int class_tiles = (a.b.n_max - a.first + kTile - 1) / kTile;   // a colour class has at most n_max - first nodes
    const dim3 nodes(a.b.B, class_tiles > 0 ? class_tiles : 1);
    const dim3 graphs((a.b.B + kTile - 1) / kTile);
    GmcProbeScope probe(GMC_K_REFINE, st);
    hipLaunchKernelGGL(large_round_init_kernel, rows, block, 0, st, a);
    GMC_LAUNCH_CHECK();
    if (a.P) {
        if (a.expected) {
            hipLaunchKernelGGL(large_round_expect_kernel<K>, rows, block, 0, st, a);
            GMC_LAUNCH_CHECK();
            hipLaunchKernelGGL(large_round_fold_kernel, graphs, block, 0, st, a, a.expected, 0);
            GMC_LAUNCH_CHECK();
        }
        for (a.colour = 0; a.colour < max_classes; ++a.colour) {
            hipLaunchKernelGGL(large_round_colour_kernel<K>, nodes, block, 0, st, a);
            GMC_LAUNCH_CHECK();
        }
    }
    for (int s = 0; s < max_sweeps; ++s) {
        for (a.colour = 0; a.colour < max_classes; ++a.colour) {
            hipLaunchKernelGGL(large_descent_colour_kernel<K>, nodes, block, 0, st, a);
            GMC_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(large_descent_close_kernel, dim3(1), block, 0, st, a.f, a.b.B);
        GMC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(large_round_score_kernel, rows, block, 0, st, a);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(large_round_fold_kernel, graphs, block, 0, st, a, a.cut, 1);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// the checks the two entry points share (P aside), in the family's order, and the launch
int large_round_run(const gmc_batch *batch, const float *P, bool rounding, int32_t K, int32_t terminals,
                    const int32_t *order,
                    const int32_t *cgoff, const int32_t *cptr, int32_t max_classes, int32_t max_sweeps, void *workspace,
                    size_t workspace_bytes_given, int8_t *assign, float *cut, float *expected, int32_t *sweeps,
                    gmc_stream_t stream) {
    if (!batch || (rounding && !P) || !order || !cgoff || !cptr || !workspace || !assign || !cut) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol || !batch->gcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (max_sweeps < 0 || max_classes < 0 || batch->B < 0 || (terminals != 0 && terminals != 1)) return GMC_ERR_SHAPE;
    const int first = terminals ? K : 0;
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || batch->n_max > GMC_LARGE_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    if (batch->R < 0 || workspace_bytes_given < workspace_bytes(batch)) return GMC_ERR_WORKSPACE;
    if (batch->B == 0) return GMC_OK;
    int *words = static_cast<int *>(workspace);
    const size_t B = (size_t)batch->B;
    const Flags f{words, words + B, words + 2 * B, words + 3 * B};
    float *part = reinterpret_cast<float *>(words + flag_words(batch));
    unsigned char *cls = reinterpret_cast<unsigned char *>(part + part_slots(batch));
    const LargeRoundArgs a{*batch, P, K, first, order, cgoff, cptr, cls, f, part, reinterpret_cast<signed char *>(assign), cut,
                           expected, sweeps, 0};
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMC_KWAY_DISPATCH(K, return large_round_launch<KK>(a, max_classes, max_sweeps, st));
    return GMC_OK;
}

}  // namespace

extern "C" size_t gmc_large_round_workspace_bytes(const gmc_batch *batch, int32_t K) {
    if (!batch || batch->abi != GMC_VERSION || K < 2 || K > GMC_KWAY_MAX_CLASSES || batch->B < 0 || batch->R < 0) return 0;
    return workspace_bytes(batch);
}

extern "C" int gmc_large_round_conditional_f32(const gmc_batch *batch, const float *P, int32_t K, const int32_t *order,
                                               const int32_t *cgoff, const int32_t *cptr, int32_t max_classes,
                                               int32_t max_descent_sweeps, void *workspace, size_t workspace_bytes,
                                               int8_t *assign, float *cut, float *expected, int32_t *sweeps,
                                               gmc_stream_t stream) {
    return large_round_run(batch, P, true, K, 1, order, cgoff, cptr, max_classes, max_descent_sweeps, workspace,
                           workspace_bytes, assign, cut, expected, sweeps, stream);
}

extern "C" int gmc_large_local_search_f32(const gmc_batch *batch, int32_t K, const int32_t *order, const int32_t *cgoff,
                                          const int32_t *cptr, int32_t max_classes, int32_t max_sweeps, void *workspace,
                                          size_t workspace_bytes, int8_t *assign, float *cut, int32_t *sweeps,
                                          gmc_stream_t stream) {
    return large_round_run(batch, nullptr, false, K, 1, order, cgoff, cptr, max_classes, max_sweeps, workspace,
                           workspace_bytes, assign, cut, nullptr, sweeps, stream);
}

// the two entry points above with the terminals optional (terminals = 0: every node is movable)
extern "C" int gmc_large_round_conditional_t_f32(const gmc_batch *batch, const float *P, int32_t K, int32_t terminals,
                                                 const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                                                 int32_t max_classes, int32_t max_descent_sweeps, void *workspace,
                                                 size_t workspace_bytes, int8_t *assign, float *cut, float *expected,
                                                 int32_t *sweeps, gmc_stream_t stream) {
    return large_round_run(batch, P, true, K, terminals, order, cgoff, cptr, max_classes, max_descent_sweeps, workspace,
                           workspace_bytes, assign, cut, expected, sweeps, stream);
}

extern "C" int gmc_large_local_search_t_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const int32_t *order,
                                            const int32_t *cgoff, const int32_t *cptr, int32_t max_classes,
                                            int32_t max_sweeps, void *workspace, size_t workspace_bytes, int8_t *assign,
                                            float *cut, int32_t *sweeps, gmc_stream_t stream) {
    return large_round_run(batch, nullptr, false, K, terminals, order, cgoff, cptr, max_classes, max_sweeps, workspace,
                           workspace_bytes, assign, cut, nullptr, sweeps, stream);
}
