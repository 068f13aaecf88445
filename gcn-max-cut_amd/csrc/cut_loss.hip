// The loss of the GCN max-cut step on its own: per-graph loss and dLoss/dP for GIVEN probabilities P [R,3].
//
// What a caller of the autograd paths (gmc_forward + gmc_backward_from_gp, gmc_forward_features +
// gmc_backward_features_from_gp) otherwise builds in torch as dense [n,1000] products, one graph at a time
// (TrainingNeural.py:154-176,:291-309), here in O(edges): one workgroup per graph, the graph's rows in LDS, the same
// neighbour walk as the head (ELL table, overflow lists or CSR rows: head_body.h).  Reference lines replaced:
//   TrainingNeural.py:87-94    override_fixed_nodes (rows 0,1,2 <- e0,e1,e2, straight-through)
//   TrainingNeural.py:96-106   per-row argmax one-hot, straight-through          (GMC_LOSS_CUT only)
//   TrainingNeural.py:154-176,:291-309  loss = -C/2 * sum A o (1 - S S^T)
//   GMC_LOSS_CUT           loss = -C * cut(S),                                   GP = C * A_val @ onehot(S)
//   GMC_LOSS_EXPECTED_CUT  loss = -C/2 * sum_uv w_uv (1 - Pt_u . Pt_v),           GP = C * A_val @ Pt
// The sums run in the head's order (a thread's rows ascending, then the block tree): for GMC_LOSS_CUT the loss is,
// bit for bit, the one gmc_head_f32 reports for the same P.
#include "head_body.h"
#include "launchers.h"

namespace {

struct CutLossArgs {
    gmc_batch b;
    const float *P;
    float C;
    float *loss;
    float *GP;
};

template <int W, bool SOFT>
__global__ __launch_bounds__(kHeadThreads) void cut_loss_kernel(CutLossArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int g = blockIdx.x;
    const int r0 = a.b.goff[g];
    const int n = a.b.goff[g + 1] - r0;
    const int NP = a.b.n_max + 4;             // + 4 padding slots (ELL padding ids n..n+3): zero rows / class 3
    float *sP = lds;                          // [NP*3]  SOFT: Pt
    int *sS = reinterpret_cast<int *>(lds + 3 * NP);  // [NP]  !SOFT: argmax class of Pt
    float *red = lds + 4 * NP;                // [64]
    const uint4 none = make_uint4(0, 0, 0, 0);

    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const long r = r0 + l;
        float p0 = a.P[r * 3], p1 = a.P[r * 3 + 1], p2 = a.P[r * 3 + 2];
        int s;
        if (l < 3) {
            s = l;
            p0 = l == 0 ? 1.f : 0.f; p1 = l == 1 ? 1.f : 0.f; p2 = l == 2 ? 1.f : 0.f;
        } else {
            s = 0;  // torch.argmax: first maximum wins
            float best = p0;
            if (p1 > best) { best = p1; s = 1; }
            if (p2 > best) { s = 2; }
        }
        if constexpr (SOFT) {
            sP[3 * l] = p0; sP[3 * l + 1] = p1; sP[3 * l + 2] = p2;
        } else {
            sS[l] = s;
        }
    }
    if constexpr (SOFT) {
        if (threadIdx.x < 12) sP[3 * n + threadIdx.x] = 0.f;
    } else {
        if (threadIdx.x < 4) sS[n + threadIdx.x] = 3;  // a class no node has
    }
    __syncthreads();

    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const long r = r0 + l;
        float g0 = 0.f, g1 = 0.f, g2 = 0.f, cut = 0.f;
        if constexpr (SOFT) {
            // a padding id (>= n) arrives with weight 1 in a batch without weights: the id keeps it out of the sum
            const float u0 = sP[3 * l], u1 = sP[3 * l + 1], u2 = sP[3 * l + 2];
            for_neighbours<W>(a.b, r0, l, n, false, none, none, [&](int c, float w) {
                const float q0 = sP[3 * c], q1 = sP[3 * c + 1], q2 = sP[3 * c + 2];
                const float wv = c < n ? w : 0.f;
                g0 += wv * q0; g1 += wv * q1; g2 += wv * q2;
                cut += wv * (1.0f - (u0 * q0 + u1 * q1 + u2 * q2));
            });
        } else {
            const int me = sS[l];
            for_neighbours<W>(a.b, r0, l, n, false, none, none, [&](int c, float w) {
                const int sc = sS[c];  // padding slots carry class 3: no contribution
                g0 += sc == 0 ? w : 0.f; g1 += sc == 1 ? w : 0.f; g2 += sc == 2 ? w : 0.f;
                cut += (sc != me && sc != 3) ? w : 0.f;
            });
        }
        acc[0] += cut;
        if (a.GP) { a.GP[r * 3] = g0 * a.C; a.GP[r * 3 + 1] = g1 * a.C; a.GP[r * 3 + 2] = g2 * a.C; }
    }
    block_sum4(acc, red);
    // one system-scope store: `loss` may be pinned host memory the caller watches
    if (threadIdx.x == 0) __hip_atomic_store(a.loss + g, -a.C * (acc[0] * 0.5f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

template <int W, bool SOFT>
int launch(const CutLossArgs &a, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(cut_loss_kernel<W, SOFT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    GmcProbeScope probe(GMC_K_HEAD, st);
    hipLaunchKernelGGL((cut_loss_kernel<W, SOFT>), dim3(a.b.B), dim3(kHeadThreads), lds, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

}  // namespace

extern "C" int gmc_cut_loss_f32(const gmc_batch *batch, const float *P, float C, int32_t loss_kind, float *loss,
                                float *GP, gmc_stream_t stream) {
    if (!gmc_loss_kind_ok(loss_kind)) return GMC_ERR_LOSS;
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->gcol || !batch->lcol || !batch->dinv || !P || !loss) return GMC_ERR_NULL;
    if (batch->B < 0 || batch->R < 0 || batch->nnz < 0) return GMC_ERR_SHAPE;
    if (batch->B > 0 && (batch->n_max < 3 || batch->n_max > GMC_MAX_GRAPH_NODES)) return GMC_ERR_GRAPH_SIZE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const CutLossArgs a{*batch, P, C, loss, GP};
    const size_t lds = sizeof(float) * (4 * ((size_t)batch->n_max + 4) + 64);
    const int w = (batch->ell != nullptr && (batch->ell_width == 8 || batch->ell_width == 16)) ? batch->ell_width : 0;
    if (loss_kind == GMC_LOSS_EXPECTED_CUT)
        return w == 8 ? launch<8, true>(a, lds, st) : w == 16 ? launch<16, true>(a, lds, st) : launch<0, true>(a, lds, st);
    return w == 8 ? launch<8, false>(a, lds, st) : w == 16 ? launch<16, false>(a, lds, st) : launch<0, false>(a, lds, st);
}
