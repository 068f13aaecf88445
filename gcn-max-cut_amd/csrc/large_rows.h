// What the row-parallel kernels of large.hip and functional.hip share: the grid of (graph, tile of kLargeTile rows), the
// slots of a graph's tile partials, and a CSR row's sum by its lane or - a row of more than kLargeWaveRow entries - by its
// wave.  large.hip states the summation orders.
#pragma once
#include "kway_rows.h"

namespace {

constexpr int kLargeTile = 256;      // rows per workgroup, one per thread
constexpr int kLargeWaveRow = 64;    // longest row one lane walks
constexpr int kLargeWaves = kLargeTile / 64;

__device__ __forceinline__ float lane_value(float v, int src) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), src));
}

// acc += sum over the entries e of the row [beg, end) of term(e, acc, ctx): short rows by the lane that owns them, rows
// of more than kLargeWaveRow entries by the whole wave (the owner's ctx - C floats - broadcast first).  Every lane of the
// wave must call it; `live` = false: the lane owns no row.
template <int V, int C, class Term>
__device__ __forceinline__ void row_terms(int beg, int end, bool live, const float (&ctx)[C], float (&acc)[V], Term term) {
    const int lane = gmc::lane_id();
    const bool hub = live && end - beg > kLargeWaveRow;
    if (live && !hub)
        for (int e = beg; e < end; ++e) term(e, acc, ctx);
    unsigned long long todo = __ballot(hub);
    while (todo) {   // (wave-uniform)
        const int src = gmc::uniform(__ffsll(todo) - 1);
        todo &= todo - 1;
        const int b = __builtin_amdgcn_readlane(beg, src), en = __builtin_amdgcn_readlane(end, src);
        float c[C];
#pragma unroll
        for (int k = 0; k < C; ++k) c[k] = lane_value(ctx[k], src);
        float part[V] = {};
        for (int e = b + lane; e < en; e += GMC_WAVE) term(e, part, c);
#pragma unroll
        for (int k = 0; k < V; ++k) part[k] = gmc::wave_sum(part[k]);
        if (lane == src) {
#pragma unroll
            for (int k = 0; k < V; ++k) acc[k] = part[k];
        }
    }
}

// the tile of this workgroup: graph, first row of the graph, rows of the graph, local row of this thread
struct Tile { int g, r0, n, l; };
__device__ __forceinline__ Tile my_tile(const gmc_batch &b) {
    Tile t;
    t.g = blockIdx.x;
    t.r0 = b.goff[t.g];
    t.n = b.goff[t.g + 1] - t.r0;
    t.l = (int)blockIdx.y * kLargeTile + (int)threadIdx.x;
    return t;
}
__device__ __forceinline__ long part_slot(const Tile &t) { return (long)(t.r0 / kLargeTile) + t.g + blockIdx.y; }

// a row of K floats gathered from src (rows by batch row id), summed over the CSR row
template <int K>
__device__ __forceinline__ void gather_sum(const gmc_batch &b, const float *src, int beg, int end, bool live, float (&z)[K]) {
    const float none[1] = {0.f};
    row_terms<K, 1>(beg, end, live, none, z, [&](int e, float (&acc)[K], const float (&)[1]) {
        float q[K];
        load_row<K>(src, b.gcol[e], q);
#pragma unroll
        for (int k = 0; k < K; ++k) acc[k] += q[k];
    });
}

}  // namespace
