// The post-processing sampler of decode.hip with its uniforms drawn on the GPU from a seed (an extension: the
// reference draws them from numpy's global RNG, TestingNeuralNetwork.py:18-46, and decode.hip reproduces that stream).
// The draw rule is stated in include/gcnmaxcut.h (gmc_decode_sample_seeded_f32): a graph's key and the pair
// (iteration, local node) go through the counter-based hash of mix64.h, the top 53 bits of the result are the uniform.
// Nothing is generated on the host and nothing is copied; a graph's samples depend on its key alone.
//
// One 256-thread workgroup per (iteration, graph), as decode_sample_kernel: the sampled classes as bytes in LDS, the
// cut by gmc::block_cut, so a sample scores bit for bit what gmc_decode_sample_f32 and gmc_refine_local_f32 report for
// the same assignment.  The pick kernel takes the winning iteration by gmc::pick_best_index and REGENERATES that one
// assignment from the hash, so the [iters][R] array of all samples is optional: without it a call writes
// [B][iters] floats and [R] ints, whatever `iters` is.
#include "gmc_common.h"
#include "cut_body.h"
#include "mix64.h"

namespace {

using gmc::u64;

struct SeededArgs {
    gmc_batch b;
    const float *P;          // [R,3]
    const u64 *gkey;         // [B]
    int iters;
    signed char *assign_all; // [iters][R] or NULL
    float *cut_all;          // [B][iters]
    int *best_assign;        // [R]        (the pick kernel)
    float *best_cut;         // [B]
    int *best_iter;          // [B]
};

// key + GOLD * (((u64)it << 32 | l) + 1) without the node: l < 2^32 only adds GOLD * l
__device__ __forceinline__ u64 iteration_base(u64 key, int it) {
    return key + GMC_GOLD * (((u64)(unsigned)it << 32) + 1ULL);
}

// class of local node l >= 3 with probabilities p[0..2]: decode_sample_kernel's compare on the hashed uniform
__device__ __forceinline__ int seeded_class(u64 base, int l, const float *p) {
    const u64 h = gmc::mix64(base + GMC_GOLD * (u64)(unsigned)l);
    const double r = (double)(h >> 11) * 0x1.0p-53;                   // [0, 1), exact
    const double c0 = (double)p[0], c1 = c0 + (double)p[1];           // running sum in double (NumPy 1.x)
    return r < c0 ? 0 : (r < c1 ? 1 : 2);                             // class 2: r < c2, or the fallback
}

__global__ __launch_bounds__(256) void sample_seeded_kernel(SeededArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char sa[];
    __shared__ float red[4];
    const int it = blockIdx.x, g = blockIdx.y;
    const int r0 = a.b.goff[g];
    const int n = a.b.goff[g + 1] - r0;
    if (n > a.b.n_max) return;   // (a batch that contradicts its own n_max: the LDS is sized by it)
    const u64 base = iteration_base(a.gkey[g], it);
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const int c = l < 3 ? l : seeded_class(base, l, a.P + (long)(r0 + l) * 3);
        sa[l] = (unsigned char)c;
        if (a.assign_all) a.assign_all[(long)it * a.b.R + r0 + l] = (signed char)c;
    }
    __syncthreads();
    const float cut = gmc::block_cut(a.b, sa, r0, n, red);
    if (threadIdx.x == 0) a.cut_all[(long)g * a.iters + it] = cut;
}

// One workgroup per graph: the winning iteration, then its assignment again from the hash (never read from assign_all,
// so the call with and without that array runs the same code).
__global__ __launch_bounds__(256) void sample_seeded_pick_kernel(SeededArgs a) {
    const int g = blockIdx.x;
    const int best = gmc::pick_best_index(a.cut_all, a.iters, g, a.best_cut, a.best_iter);
    const int r0 = a.b.goff[g], n = a.b.goff[g + 1] - r0;
    const u64 base = iteration_base(a.gkey[g], best);
    for (int l = threadIdx.x; l < n; l += blockDim.x)
        a.best_assign[r0 + l] = l < 3 ? l : seeded_class(base, l, a.P + (long)(r0 + l) * 3);
}

}  // namespace

extern "C" int gmc_decode_sample_seeded_f32(const gmc_batch *batch, const float *P, const uint64_t *gkey,
                                            int32_t iters, int8_t *assign_all, float *cut_all, int32_t *best_assign,
                                            float *best_cut, int32_t *best_iter, gmc_stream_t stream) {
    if (!batch || !P || !gkey || !cut_all || !best_assign || !best_cut || !best_iter) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (iters < 1 || batch->B < 0) return GMC_ERR_SHAPE;
    if (batch->B > 0 && (batch->n_max < 3 || batch->n_max > 65535)) return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    SeededArgs a{*batch, P, reinterpret_cast<const u64 *>(gkey), iters, reinterpret_cast<signed char *>(assign_all),
                 cut_all, best_assign, best_cut, best_iter};
    {
        GmcProbeScope probe(GMC_K_SAMPLE, st);
        hipLaunchKernelGGL(sample_seeded_kernel, dim3(iters, batch->B), dim3(256), (size_t)batch->n_max, st, a);
        GMC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(sample_seeded_pick_kernel, dim3(batch->B), dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
