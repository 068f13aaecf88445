// The low-rank semidefinite relaxation of max-cut by the mixing method and its hyperplane rounding
// (gmc_sdp_relax_f32, gmc_sdp_round_f32; K = 2, rank 16 / 32 / 64, up to GMC_LARGE_MAX_GRAPH_NODES nodes per graph).  The
// rules - init, visit, value, hyperplane - are stated to the operation in include/gcnmaxcut_sdp.h.
//
// As in large_round.hip a graph is shared by several workgroups, the state (V [R][rank], the caller's) lives in global
// memory and kernel boundaries are the only synchronisation between workgroups: no spin waits, no arrival counters, no
// atomics.  Rows are batch row ids, neighbours are read through gcol.
//
//   init      a node per `rank` adjacent lanes: the hash, the butterfly over the node's lanes, the division
//   visit     one launch per colour: the nodes of that colour of every graph, a node per `rank` adjacent lanes - a wave
//             holds 4, 2 or 1 nodes, a workgroup 16, 8 or 4; lane k of a node walks the node's CSR row and reads entry k
//             of every neighbour's row (the node's lanes together: one contiguous run of 4 * rank bytes per neighbour)
//   value     a row per thread (its edges in CSR order, each dot product k ascending), a tile of 256 rows by block_sum
//             to its slot; fold: per graph its tiles' slots ascending
//   round     a row per thread, its V row in registers; the workgroup draws a plane's normal into LDS (lane k entry k)
//             and every thread takes its row's side; a workgroup walks planes blockIdx.y, + gridDim.y, ...
//
// Grids.  Only x is relied on beyond 65,535: a colour class of a 2^20-node graph has up to 2^20 / 4 tiles at rank 64.
// x is always the tile (of the graph's rows, or of a colour class's nodes); the graphs are walked by y (z for round)
// with a stride of gridDim, so any batch size fits.  Tiles past a graph's (a class's) end do nothing, so a graph's
// results do not depend on what else is in the batch.  The value's slots of graph g: goff[g] / 256 + g onwards.
//
// sqrtf and `/` are the correctly rounded forms under hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt
// (batch_build.hip relies on the same); __fsqrt_rn is the native square root in this toolchain and is not used.
#include "../../include/gcnmaxcut_sdp.h"
#include "kway_rows.h"
#include "mix64.h"

#pragma clang fp contract(off)   // every product and every sum of the rules is rounded on its own

namespace {

using gmc::mix64;
using gmc::u64;

static_assert(GMC_SDP_GOLD == GMC_GOLD, "one golden-ratio constant");

constexpr int kTile = 256;
constexpr int kWaves = kTile / GMC_WAVE;
constexpr int kMaxYZ = 65535;
constexpr int kPlaneGroups = 16;   // workgroups (grid y) that share a row tile's planes: each keeps its rows in registers

struct SdpArgs {
    gmc_batch b;
    int first;                       // first movable local id: 2 with terminals, 0 without
    const float *cost;               // [R][2] or NULL
    const int *order, *cgoff, *cptr;
    const u64 *gkey;                 // [B]
    float *V;                        // [R][rank]
    float *value;                    // [B]
    float *part;                     // [R / 256 + B + 1] workspace
    int colour;                      // of a colour launch
};

struct Graph { int r0, n; bool runs; };
__device__ __forceinline__ Graph graph_of(const gmc_batch &b, int first, int g) {
    Graph t;
    t.r0 = b.goff[g];
    t.n = b.goff[g + 1] - t.r0;
    t.runs = t.n >= (first > 1 ? first : 1) && t.n <= b.n_max;
    return t;
}

// the sum of x over the RANK adjacent lanes of a node: x[i] += x[i ^ d], d = RANK / 2 .. 1 (every lane gets the total)
template <int RANK>
__device__ __forceinline__ float node_sum(float x) { return gmc::xor_tree<RANK / 2, 1>(x); }

template <int RANK>
__global__ __launch_bounds__(kTile) void sdp_init_kernel(SdpArgs a) {
    constexpr int kNodes = kTile / RANK;
    const int k = (int)threadIdx.x & (RANK - 1), sub = (int)threadIdx.x / RANK;
    for (int g = blockIdx.y; g < a.b.B; g += gridDim.y) {
        const Graph t = graph_of(a.b, a.first, g);
        const long l = (long)blockIdx.x * kNodes + sub;
        const bool live = t.runs && l < t.n;   // (a node's lanes agree; dead lanes run the butterfly on zeros)
        float x = 0.f;
        if (live) {
            const u64 i = mix64(a.gkey[g] + GMC_GOLD * ((u64)l * RANK + (u64)k + 1)) >> 40;
            x = (float)((int)i - (1 << 23));
        }
        const float s = node_sum<RANK>(x * x);
        if (!live) continue;
        float v;
        if (l < a.first) v = k == 0 ? (l == 0 ? 1.0f : -1.0f) : 0.0f;
        else if (s == 0.0f) v = k == 0 ? 1.0f : 0.0f;
        else v = x / sqrtf(s);
        a.V[(long)(t.r0 + l) * RANK + k] = v;
    }
}

template <int RANK>
__global__ __launch_bounds__(kTile) void sdp_visit_kernel(SdpArgs a) {
    constexpr int kNodes = kTile / RANK;
    const int k = (int)threadIdx.x & (RANK - 1), sub = (int)threadIdx.x / RANK;
    for (int g = blockIdx.y; g < a.b.B; g += gridDim.y) {
        const Graph t = graph_of(a.b, a.first, g);
        if (!t.runs) continue;
        const int k0 = a.cgoff[g];
        if (a.colour >= a.cgoff[g + 1] - k0 - 1) continue;
        const long i = (long)a.cptr[k0 + a.colour] + (long)blockIdx.x * kNodes + sub;
        int r = -1;
        if (i < a.cptr[k0 + a.colour + 1]) {
            r = a.order[i];
            const int l = r - t.r0;
            if (l < a.first || l >= t.n) r = -1;   // not a movable row of this graph: never touch the state for it
        }
        float gk = 0.0f;
        if (r >= 0) {
            if (a.cost && k == 0) gk = a.cost[2 * (long)r] - a.cost[2 * (long)r + 1];
            const int e1 = a.b.rowptr[r + 1];
            for (int e = a.b.rowptr[r]; e < e1; ++e) {
                const int u = a.b.gcol[e];
                if (u == r) continue;
                const float w = a.b.vals ? a.b.vals[e] : 1.0f;
                gk = gk + w * a.V[(long)u * RANK + k];
            }
        }
        const float n = sqrtf(node_sum<RANK>(gk * gk));
        if (r < 0 || n == 0.0f || !(n <= 3.402823466e+38f)) continue;   // (NaN and +inf both fail the comparison)
        a.V[(long)r * RANK + k] = -(gk / n);
    }
}

template <int RANK>
__global__ __launch_bounds__(kTile) void sdp_value_kernel(SdpArgs a) {
    __shared__ float red[kWaves];
    for (int g = blockIdx.y; g < a.b.B; g += gridDim.y) {
        const Graph t = graph_of(a.b, a.first, g);
        if (!t.runs || (long)blockIdx.x * kTile >= t.n) continue;   // (workgroup-uniform)
        const int l = (int)blockIdx.x * kTile + (int)threadIdx.x;
        float v[1] = {0.f};
        if (l < t.n) {
            const int r = t.r0 + l;
            const float *mine = a.V + (long)r * RANK;
            float p = 0.f;
            const int e1 = a.b.rowptr[r + 1];
            for (int e = a.b.rowptr[r]; e < e1; ++e) {
                const int u = a.b.gcol[e];
                if (u == r) continue;
                const float *theirs = a.V + (long)u * RANK;
                float d = 0.f;
#pragma unroll 8
                for (int k = 0; k < RANK; ++k) d = d + mine[k] * theirs[k];
                const float w = a.b.vals ? a.b.vals[e] : 1.0f;
                p = p + w * (1.0f - d);
            }
            float x = 0.25f * p;
            if (a.cost) {
                const float c0 = a.cost[2 * (long)r], c1 = a.cost[2 * (long)r + 1];
                x = x - ((c0 + c1) * 0.5f + ((c0 - c1) * 0.5f) * mine[0]);
            }
            v[0] = x;
        }
        __syncthreads();   // (red of the previous graph has been read)
        block_sum<1, kWaves>(v, red);
        if (threadIdx.x == 0) a.part[(long)(t.r0 / kTile) + g + blockIdx.x] = v[0];
    }
}

// one thread per graph: value[g] = its tiles' slots, ascending
__global__ __launch_bounds__(kTile) void sdp_fold_kernel(SdpArgs a) {
    const long g = (long)blockIdx.x * kTile + threadIdx.x;
    if (g >= a.b.B) return;
    const Graph t = graph_of(a.b, a.first, (int)g);
    if (!t.runs) return;
    const int tiles = (t.n + kTile - 1) / kTile;
    const float *p = a.part + (long)(t.r0 / kTile) + g;
    float s = 0.f;
    for (int i = 0; i < tiles; ++i) s = s + p[i];
    a.value[g] = s;
}

struct RoundArgs {
    gmc_batch b;
    int first;
    const float *V;
    const u64 *gkey;
    int first_plane, planes;
    signed char *assign;             // [planes][R]
};

template <int RANK>
__global__ __launch_bounds__(kTile) void sdp_round_kernel(RoundArgs a) {
    __shared__ float h[RANK];
    for (int g = blockIdx.z; g < a.b.B; g += gridDim.z) {
        const Graph t = graph_of(a.b, a.first, g);
        if (!t.runs || (long)blockIdx.x * kTile >= t.n) continue;   // (workgroup-uniform)
        const int l = (int)blockIdx.x * kTile + (int)threadIdx.x;
        const bool live = l < t.n;
        const long r = (long)t.r0 + (live ? l : 0);
        float v[RANK];
        {
            const float4 *row = reinterpret_cast<const float4 *>(a.V + r * RANK);   // (V is 16-byte aligned: checked)
#pragma unroll
            for (int q = 0; q < RANK / 4; ++q) {
                const float4 x = row[q];
                v[4 * q] = x.x; v[4 * q + 1] = x.y; v[4 * q + 2] = x.z; v[4 * q + 3] = x.w;
            }
        }
        const u64 key = a.gkey[g] ^ GMC_SDP_PLANE_TAG;
        for (int q = blockIdx.y; q < a.planes; q += gridDim.y) {
            const u64 m = (u64)a.first_plane + (u64)q;
            __syncthreads();   // (h of the previous plane has been read)
            if (threadIdx.x < RANK) {
                unsigned D = 0;
#pragma unroll
                for (int j = 0; j < 12; ++j)
                    D += (unsigned)(mix64(key + GMC_GOLD * ((m * 12 + (u64)j) * 64 + (u64)threadIdx.x + 1)) >> 44);
                h[threadIdx.x] = (float)((int)D - 6 * (1 << 20));
            }
            __syncthreads();
            float p = 0.f;
#pragma unroll
            for (int k = 0; k < RANK; ++k) p = p + h[k] * v[k];
            if (!live) continue;
            const signed char c = l < a.first ? (signed char)l : (signed char)((p >= 0.f) == (h[0] >= 0.f) ? 0 : 1);
            a.assign[(long)q * a.b.R + r] = c;
        }
    }
}

size_t part_slots(const gmc_batch *b) { return ((size_t)b->R / kTile + (size_t)b->B + 1 + 3) & ~(size_t)3; }
bool rank_ok(int32_t rank) { return rank == 16 || rank == 32 || rank == 64; }

#define GMC_SDP_RANK_DISPATCH(rank, ...)                           \
    switch (rank) {                                                \
        case 16: { constexpr int RR = 16; __VA_ARGS__; } break;    \
        case 32: { constexpr int RR = 32; __VA_ARGS__; } break;    \
        default: { constexpr int RR = 64; __VA_ARGS__; } break;    \
    }

template <int RANK>
int relax_launch(SdpArgs a, int init, int sweeps, int max_classes, hipStream_t st) {
    constexpr int kNodes = kTile / RANK;
    const dim3 block(kTile);
    const unsigned gy = a.b.B < kMaxYZ ? a.b.B : kMaxYZ;
    const int movable = a.b.n_max - a.first;   // a colour class has at most n_max - first nodes
    const dim3 rows((a.b.n_max + kNodes - 1) / kNodes, gy);
    const dim3 nodes(movable > 0 ? (movable + kNodes - 1) / kNodes : 1, gy);
    const dim3 tiles((a.b.n_max + kTile - 1) / kTile, gy);
    GmcProbeScope probe(GMC_K_REFINE, st);
    if (init) {
        hipLaunchKernelGGL(sdp_init_kernel<RANK>, rows, block, 0, st, a);
        GMC_LAUNCH_CHECK();
    }
    for (int s = 0; s < sweeps; ++s) {
        for (a.colour = 0; a.colour < max_classes; ++a.colour) {
            hipLaunchKernelGGL(sdp_visit_kernel<RANK>, nodes, block, 0, st, a);
            GMC_LAUNCH_CHECK();
        }
    }
    hipLaunchKernelGGL(sdp_value_kernel<RANK>, tiles, block, 0, st, a);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(sdp_fold_kernel, dim3((a.b.B + kTile - 1) / kTile), block, 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

template <int RANK>
int round_launch(RoundArgs a, hipStream_t st) {
    const dim3 grid((a.b.n_max + kTile - 1) / kTile, a.planes < kPlaneGroups ? a.planes : kPlaneGroups,
                    a.b.B < kMaxYZ ? a.b.B : kMaxYZ);
    GmcProbeScope probe(GMC_K_SAMPLE, st);
    hipLaunchKernelGGL(sdp_round_kernel<RANK>, grid, dim3(kTile), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// the checks both entry points share after their own pointers, in the large decoders' order
int check_batch(const gmc_batch *batch, int32_t rank, int32_t terminals, bool shape_ok) {
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol || !batch->gcol) return GMC_ERR_NULL;
    if (!rank_ok(rank) || !shape_ok || batch->B < 0 || (terminals != 0 && terminals != 1)) return GMC_ERR_SHAPE;
    if (batch->B > 0 && (batch->n_max < (terminals ? 2 : 1) || batch->n_max > GMC_LARGE_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    return GMC_OK;
}

}  // namespace

extern "C" size_t gmc_sdp_workspace_bytes(const gmc_batch *batch, int32_t rank) {
    if (!batch || batch->abi != GMC_VERSION || !rank_ok(rank) || batch->B < 0 || batch->R < 0) return 0;
    return 4 * part_slots(batch);
}

extern "C" int gmc_sdp_relax_f32(const gmc_batch *batch, int32_t rank, int32_t terminals, const float *node_cost,
                                 const int32_t *order, const int32_t *cgoff, const int32_t *cptr, int32_t max_classes,
                                 const uint64_t *gkey, int32_t init, int32_t sweeps, float *V, float *value,
                                 void *workspace, size_t workspace_bytes, gmc_stream_t stream) {
    if (!batch || !order || !cgoff || !cptr || !V || !value || !workspace || (init == 1 && !gkey)) return GMC_ERR_NULL;
    const int rc = check_batch(batch, rank, terminals, sweeps >= 0 && max_classes >= 0 && (init == 0 || init == 1));
    if (rc != GMC_OK) return rc;
    if (!gmc_aligned16(V) || !gmc_aligned16(workspace)) return GMC_ERR_ALIGN;
    if (batch->R < 0 || workspace_bytes < 4 * part_slots(batch)) return GMC_ERR_WORKSPACE;
    if (batch->B == 0) return GMC_OK;
    const SdpArgs a{*batch, terminals ? 2 : 0, node_cost, order, cgoff, cptr, reinterpret_cast<const u64 *>(gkey), V, value,
                    static_cast<float *>(workspace), 0};
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMC_SDP_RANK_DISPATCH(rank, return relax_launch<RR>(a, init, sweeps, max_classes, st));
    return GMC_OK;
}

extern "C" int gmc_sdp_round_f32(const gmc_batch *batch, int32_t rank, int32_t terminals, const float *V,
                                 const uint64_t *gkey, int32_t first_plane, int32_t planes, int8_t *assign,
                                 gmc_stream_t stream) {
    if (!batch || !V || !gkey || !assign) return GMC_ERR_NULL;
    const int rc = check_batch(batch, rank, terminals,
                               first_plane >= 0 && planes >= 0 && (int64_t)first_plane + planes <= INT32_MAX);
    if (rc != GMC_OK) return rc;
    if (!gmc_aligned16(V)) return GMC_ERR_ALIGN;
    if (batch->R < 0) return GMC_ERR_WORKSPACE;
    if (batch->B == 0 || planes == 0) return GMC_OK;
    const RoundArgs a{*batch, terminals ? 2 : 0, V, reinterpret_cast<const u64 *>(gkey), first_plane, planes,
                      reinterpret_cast<signed char *>(assign)};
    hipStream_t st = static_cast<hipStream_t>(stream);
    GMC_SDP_RANK_DISPATCH(rank, return round_launch<RR>(a, st));
    return GMC_OK;
}
