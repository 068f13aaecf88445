// The K-class draw of the seeded sampler, shared by its one-workgroup kernels (kway_search.hip) and the kernels for
// graphs beyond GMC_MAX_GRAPH_NODES (large_search.hip): one definition, so that a sample cannot depend on which of the
// two drew it.  The rule is stated in include/gcnmaxcut.h (gmc_kway_decode_sample_seeded_f32).
#pragma once
#include "gmc_common.h"
#include "mix64.h"

namespace gmc {

// key + GOLD * (((u64)it << 32 | l) + 1) without the node: l < 2^32 only adds GOLD * l
__device__ __forceinline__ u64 iteration_base(u64 key, int it) {
    return key + GMC_GOLD * (((u64)(unsigned)it << 32) + 1ULL);
}

// class of local node l >= K with probabilities p[0..K-1]: the first class j in 0..K-2 whose running double sum
// exceeds the hashed uniform, class K-1 otherwise (no compare against the last sum: a NaN row gives K-1)
template <int K>
__device__ __forceinline__ int seeded_class_k(u64 base, int l, const float *p) {
    const u64 h = mix64(base + GMC_GOLD * (u64)(unsigned)l);
    const double r = (double)(h >> 11) * 0x1.0p-53;   // [0, 1), exact
    double c = (double)p[0];
    int cls = K - 1;
    bool open = true;   // no class has taken the draw yet
#pragma unroll
    for (int j = 0; j < K - 1; ++j) {
        if (j > 0) c = c + (double)p[j];
        const bool take = open && r < c;
        cls = take ? j : cls;
        open = open && !take;
    }
    return cls;
}

}  // namespace gmc
