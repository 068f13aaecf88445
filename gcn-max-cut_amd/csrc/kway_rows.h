// What the K-wide row kernels of kway.hip and large.hip share: a row of K floats as vector accesses and the
// deterministic block sum.  (The dispatch of a runtime class count onto the template argument, GMC_KWAY_DISPATCH, is
// gmc_common.h's: the decoders use it too.)
#pragma once
#include "launchers.h"

namespace {

// a row of K floats of an LDS / global array whose rows start at multiples of K floats from a 16-byte aligned base:
// one 16-byte access per 4 columns when K allows it, 8-byte for the other even K
template <int K>
__device__ __forceinline__ void load_row(const float *base, int row, float (&v)[K]) {
    const float *p = base + (long)row * K;
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q) {
            const float4 t = reinterpret_cast<const float4 *>(p)[q];
            v[4 * q] = t.x; v[4 * q + 1] = t.y; v[4 * q + 2] = t.z; v[4 * q + 3] = t.w;
        }
    } else if constexpr (K % 2 == 0) {
#pragma unroll
        for (int q = 0; q < K / 2; ++q) {
            const float2 t = reinterpret_cast<const float2 *>(p)[q];
            v[2 * q] = t.x; v[2 * q + 1] = t.y;
        }
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) v[k] = p[k];
    }
}

template <int K>
__device__ __forceinline__ void store_row(float *base, long row, const float (&v)[K]) {
    float *p = base + row * K;
    if constexpr (K % 4 == 0) {
#pragma unroll
        for (int q = 0; q < K / 4; ++q)
            reinterpret_cast<float4 *>(p)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
    } else if constexpr (K % 2 == 0) {
#pragma unroll
        for (int q = 0; q < K / 2; ++q) reinterpret_cast<float2 *>(p)[q] = make_float2(v[2 * q], v[2 * q + 1]);
    } else {
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] = v[k];
    }
}

// Deterministic block sum of V values per thread (block_sum4 of head_body.h: wave butterfly, then the waves' partials
// in ascending order); result valid in thread 0.
template <int V, int WAVES>
__device__ __forceinline__ void block_sum(float (&v)[V], float *red /* [WAVES * V] */) {
    const int lane = gmc::lane_id(), wave = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < V; ++k) v[k] = gmc::wave_sum(v[k]);
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) red[wave * V + k] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < V; ++k) {
            float s = 0.f;
#pragma unroll
            for (int w = 0; w < WAVES; ++w) s += red[w * V + k];
            v[k] = s;
        }
    }
}

}  // namespace
