// C[M,Nc] = rowscale o (op(A) @ op(B)) in fp32 on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32, a k-ordered
// fmaf chain), for the dense-feature path of GraphConv layer 1 (TrainingNeural.py:80 with features that are not the
// padded adjacency):
//   NN  T0  = dinv o (X @ W1)   [R,N] . [N,F]
//   TN  dW1 = X^T @ U           [N,R] . [R,F]
//   NT  dX  = U @ W1^T          [R,F] . [F,N]
// ONE tile loop, templated on the two operand orientations; the orientation only decides how a tile travels from global
// memory to LDS.  Both LDS tiles are k-major ([GEMM_TK][GEMM_LD], the operand's row / column index contiguous), which is
// the order the MFMA operands want: lane l reads A[m = l&15][k = l>>4] and B[k = l>>4][n = l&15], i.e. four k rows of 16
// consecutive floats; GEMM_LD = 80 puts those four rows 16 banks apart (64 lanes, 64 different banks by the address arithmetic).
//
// Block tile 64 x 64 x 16, 256 threads: wave w owns the 32 x 32 quadrant (w>>1, w&1) as 2 x 2 MFMA tiles - four
// independent accumulators, chosen for the 40-cycle dependent latency of the 32-cycle instruction with ONE wave per
// SIMD.  64 x 64 and not larger: the workload's [1000,500] output gives 16 x 8 = 128 workgroups (a 128 x 128 tile: 32 on
// 256 CUs).  The next k tile is fetched into registers before the MFMAs of the current one and stored to the other LDS
// buffer after them: one barrier per k tile.
//
// Any M, Nc, K >= 1: rows / columns / k beyond the edge are zero-filled on the way in and not stored on the way out.
// k runs in ascending order inside one workgroup (no split over k, no atomics): bitwise reproducible.
#include "launchers.h"

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int GEMM_TM = 64, GEMM_TN = 64, GEMM_TK = 16;
constexpr int GEMM_LD = 80;   // floats per k row of an LDS tile (64 + 16: rows k .. k+3 start 16 banks apart)

struct GemmArgs {
    const float *A; long lda;
    const float *B; long ldb;
    const float *scale;
    float *C; long ldc;
    int M, Nc, K;
};

// One thread's float4 of a 64 x 16 operand tile: `rows` is the operand's own extent along the tile's 64-side (M for A,
// Nc for B), r0 the tile's first row there, k0 its first k.  KC: the operand is stored [rows][K] (k contiguous), else
// [K][rows].  16-byte loads are aligned (base 16-byte aligned, ld % 4 == 0, offsets multiples of 4); the last, partial
// group of a row is read element by element, never past the row's end.
template <bool KC>
__device__ __forceinline__ float4 gemm_fetch(const float *P, long ld, int r0, int rows, int k0, int K, int t) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if constexpr (KC) {
        const int r = r0 + (t >> 2), k = k0 + (t & 3) * 4;
        if (r < rows && k < K) {
            const float *p = P + (long)r * ld + k;
            if (k + 3 < K) {
                v = *reinterpret_cast<const float4 *>(p);
            } else {
                v.x = p[0];
                if (k + 1 < K) v.y = p[1];
                if (k + 2 < K) v.z = p[2];
            }
        }
    } else {
        const int k = k0 + (t >> 4), r = r0 + (t & 15) * 4;
        if (k < K && r < rows) {
            const float *p = P + (long)k * ld + r;
            if (r + 3 < rows) {
                v = *reinterpret_cast<const float4 *>(p);
            } else {
                v.x = p[0];
                if (r + 1 < rows) v.y = p[1];
                if (r + 2 < rows) v.z = p[2];
            }
        }
    }
    return v;
}

template <bool KC>
__device__ __forceinline__ void gemm_stage(float *S, const float4 &v, int t) {
    if constexpr (KC) {   // the thread holds four k of one row: a transposing store
        const int r = t >> 2, k = (t & 3) * 4;
        S[(k + 0) * GEMM_LD + r] = v.x;
        S[(k + 1) * GEMM_LD + r] = v.y;
        S[(k + 2) * GEMM_LD + r] = v.z;
        S[(k + 3) * GEMM_LD + r] = v.w;
    } else {
        const int k = t >> 4, r = (t & 15) * 4;
        *reinterpret_cast<float4 *>(S + k * GEMM_LD + r) = v;
    }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(256) void gemm_mfma_kernel(GemmArgs g) {
    __shared__ __attribute__((aligned(16))) float As[2][GEMM_TK * GEMM_LD];
    __shared__ __attribute__((aligned(16))) float Bs[2][GEMM_TK * GEMM_LD];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int m0 = blockIdx.x * GEMM_TM, n0 = blockIdx.y * GEMM_TN;
    const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
    const int li = lane & 15, lq = lane >> 4;

    f32x4 c00 = {0.f, 0.f, 0.f, 0.f}, c01 = c00, c10 = c00, c11 = c00;
    float4 ra = gemm_fetch<!TA>(g.A, g.lda, m0, g.M, 0, g.K, t);
    float4 rb = gemm_fetch<TB>(g.B, g.ldb, n0, g.Nc, 0, g.K, t);
    gemm_stage<!TA>(As[0], ra, t);
    gemm_stage<TB>(Bs[0], rb, t);
    __syncthreads();

    const int tiles = (g.K + GEMM_TK - 1) / GEMM_TK;
    for (int it = 0; it < tiles; ++it) {
        const int cur = it & 1;
        const bool more = it + 1 < tiles;
        if (more) {
            ra = gemm_fetch<!TA>(g.A, g.lda, m0, g.M, (it + 1) * GEMM_TK, g.K, t);
            rb = gemm_fetch<TB>(g.B, g.ldb, n0, g.Nc, (it + 1) * GEMM_TK, g.K, t);
        }
        const float *as = As[cur] + lq * GEMM_LD + wm + li;
        const float *bs = Bs[cur] + lq * GEMM_LD + wn + li;
        // every operand of the tile is requested before the first MFMA: one LDS latency per tile instead of one per
        // k step (left alone, the scheduler sinks each read next to its MFMAs and waits for it there with lgkmcnt(0))
        float fa0[GEMM_TK / 4], fa1[GEMM_TK / 4], fb0[GEMM_TK / 4], fb1[GEMM_TK / 4];
#pragma unroll
        for (int s = 0; s < GEMM_TK / 4; ++s) {
            fa0[s] = as[4 * s * GEMM_LD], fa1[s] = as[4 * s * GEMM_LD + 16];
            fb0[s] = bs[4 * s * GEMM_LD], fb1[s] = bs[4 * s * GEMM_LD + 16];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < GEMM_TK / 4; ++s) {
            c00 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa0[s], fb0[s], c00, 0, 0, 0);
            c01 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa0[s], fb1[s], c01, 0, 0, 0);
            c10 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa1[s], fb0[s], c10, 0, 0, 0);
            c11 = __builtin_amdgcn_mfma_f32_16x16x4f32(fa1[s], fb1[s], c11, 0, 0, 0);
        }
        if (more) {   // the other buffer: last read before the barrier that ended the previous iteration
            gemm_stage<!TA>(As[cur ^ 1], ra, t);
            gemm_stage<TB>(Bs[cur ^ 1], rb, t);
        }
        __syncthreads();
    }

    // D of a 16 x 16 tile: column = lane & 15, row = 4 * (lane >> 4) + j
    const int col0 = n0 + wn + li, col1 = col0 + 16;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int r0 = m0 + wm + 4 * lq + j, r1 = r0 + 16;
        if (r0 < g.M) {
            const float s = g.scale ? g.scale[r0] : 1.0f;
            float *c = g.C + (long)r0 * g.ldc;
            if (col0 < g.Nc) c[col0] = g.scale ? c00[j] * s : c00[j];
            if (col1 < g.Nc) c[col1] = g.scale ? c01[j] * s : c01[j];
        }
        if (r1 < g.M) {
            const float s = g.scale ? g.scale[r1] : 1.0f;
            float *c = g.C + (long)r1 * g.ldc;
            if (col0 < g.Nc) c[col0] = g.scale ? c10[j] * s : c10[j];
            if (col1 < g.Nc) c[col1] = g.scale ? c11[j] * s : c11[j];
        }
    }
}

}  // namespace

int gmc_gemm_launch(int ta, int tb, int M, int Nc, int K, const float *A, long lda, const float *B, long ldb,
                    const float *scale, float *C, long ldc, hipStream_t st) {
    if (!A || !B || !C) return GMC_ERR_NULL;
    if (M < 0 || Nc < 0 || K < 0) return GMC_ERR_SHAPE;
    if (lda < (ta ? M : K) || ldb < (tb ? K : Nc) || ldc < Nc) return GMC_ERR_SHAPE;
    if (ta && tb) return GMC_ERR_UNSUPPORTED;
    const long gy = ((long)Nc + GEMM_TN - 1) / GEMM_TN;
    if (gy > 65535) return GMC_ERR_UNSUPPORTED;
    if (!gmc_aligned16(A) || !gmc_aligned16(B) || !gmc_aligned16(C) || lda % 4 || ldb % 4 || ldc % 4) return GMC_ERR_ALIGN;
    if (M == 0 || Nc == 0) return GMC_OK;
    GemmArgs g{A, lda, B, ldb, scale, C, ldc, M, Nc, K};
    const dim3 grid((unsigned)((M + GEMM_TM - 1) / GEMM_TM), (unsigned)gy), block(256);
    GmcProbeScope probe(GMC_K_GEMM, st);
    if (ta)
        hipLaunchKernelGGL((gemm_mfma_kernel<true, false>), grid, block, 0, st, g);
    else if (tb)
        hipLaunchKernelGGL((gemm_mfma_kernel<false, true>), grid, block, 0, st, g);
    else
        hipLaunchKernelGGL((gemm_mfma_kernel<false, false>), grid, block, 0, st, g);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" int gmc_gemm_f32(int32_t ta, int32_t tb, int32_t M, int32_t Nc, int32_t K, const float *A, int64_t lda,
                            const float *B, int64_t ldb, const float *scale, float *C, int64_t ldc,
                            gmc_stream_t stream) {
    return gmc_gemm_launch(ta != 0, tb != 0, M, Nc, K, A, (long)lda, B, (long)ldb, scale, C, (long)ldc,
                           static_cast<hipStream_t>(stream));
}
