// The counter-based hash of the annealing's move levels (anneal_body.h) and of the seeded sampler's uniforms
// (draw_body.h): splitmix64's finaliser over seed + GOLD * (counter + 1), all in uint64 arithmetic.  One definition, so
// the kernels and their host restatements speak of the same function.
#pragma once
#include "gmc_common.h"

#define GMC_GOLD 0x9E3779B97F4A7C15ULL

namespace gmc {

typedef unsigned long long u64;

__host__ __device__ __forceinline__ u64 mix64(u64 z) {  // splitmix64 finaliser (dropout.hip)
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

}  // namespace gmc
