// The K-class step (number_classes K in 2..8): every kernel that sees the class count, as a template over K.
//
// The fused LDS kernels, the head of head_body.h and the hidden backward of hidden_bwd.hip are written for the three
// columns of the reference (TrainingNeural.py:91-93).  This file holds their K-wide forms for the one-kernel-per-operation
// ROW-KERNEL sequence on plain row-major [R, ld] buffers (the plan dense features take; api.hip: kway_*):
//   hw2_k          Z0[r,:] = dinv[r] * (H[r,:] @ W2)                       [R,K]   (:83; hw2_rows_kernel of dropout.hip)
//   head_k         per graph: Z = dinv o (A @ Z0) + b2, P = softmax(Z), terminals 0..K-1 <- e_0..e_{K-1}, S = argmax,
//                  loss; training: GP, softmax backward, db2 partials, GY2 = A @ (dinv o GZ)   (head_body.h, CSR walk)
//   hidden_bwd_k   Gs = dinv o relu'(H) o dinv o (GY2 @ W2^T), tile partials of dW2 [F,K] and db1   (hidden_bwd_kernel)
//   reduce_k       fixed-order fold of those partials and of the head's db2 partials              (colsum_reduce_kernel)
// Everything that does not see K - the W1 gather, both F-wide aggregations, dW1, the loss tail, Adam - is the existing
// kernel.  Each kernel keeps the summation order of its 3-wide model; no float atomics: bitwise reproducible.
#include "kway_rows.h"

namespace {

// ---- hw2_k ----------------------------------------------------------------------------------------------------------
struct Hw2KArgs {
    const float *H, *dinv, *W2;
    float *Z0;
    long R;
    int F;
    long ld;
};

// one wave per row, fixed-order butterfly sum (hw2_rows_kernel with fs = 0)
template <int K>
__global__ __launch_bounds__(256) void hw2_k_kernel(Hw2KArgs a) {
    const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int lane = gmc::lane_id();
    float z[K] = {};
    for (int c = lane; c < a.F; c += GMC_WAVE) {
        const float h = a.H[r * a.ld + c];
        float w[K];
        load_row<K>(a.W2, c, w);
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] = fmaf(h, w[k], z[k]);
    }
#pragma unroll
    for (int k = 0; k < K; ++k) z[k] = gmc::wave_sum(z[k]);
    if (lane == 0) {
        const float d = a.dinv[r];
#pragma unroll
        for (int k = 0; k < K; ++k) z[k] *= d;
        store_row<K>(a.Z0, r, z);
    }
}

// ---- head_k ---------------------------------------------------------------------------------------------------------
// threads of a head workgroup: 1024 as head_body.h up to 4 classes; the wider rows (K accumulators in each of the three
// neighbour loops) get 512 threads' register budget: K = 8 does not fit the 128 VGPRs of a 1024-thread workgroup
__host__ __device__ constexpr int head_k_threads(int K) { return K <= 4 ? 1024 : 512; }
constexpr int kHeadKWaves = 1024 / 64;   // slots of the block sum's LDS array (the widest workgroup's waves)

struct HeadKArgs {
    gmc_batch b;
    const float *Z0;   // [R,K]
    const float *b2;
    float C;
    float *P;          // [R,K]
    int *S;
    float *loss;
    float *GY2;        // [R,K]; nullptr: forward only
    float *db2part;    // [B,K]
    long b2_stride;    // floats from one graph's bias to the next: 0 = one shared conv2.bias, K = b2 [B,K] (instance.hip)
    int terminals;     // 1: rows 0..K-1 of a graph are the terminals; 0: no row is overridden (gmc_inst_*_t)
    const float *node_cost;   // [R,K] by batch row or NULL: the per-node class costs of the loss (gmc_inst_*_c)
};

// floats of dynamic LDS: sA [NP,K], sP [NP,K], SOFT: the terminals' own rows [K,K], sS [NP], the block sum's [waves, K+1]
__host__ __device__ inline size_t head_k_lds_floats(int n_max, int K, bool soft) {
    return (size_t)(2 * K + 1) * ((size_t)n_max + 4) + (size_t)kHeadKWaves * (K + 1) + (soft ? (size_t)K * K : 0);
}

// The head of graph blockIdx.x (head_body.h without the partial fold and the ELL table: one Z0, the CSR rows).
//   SOFT  the relaxed loss (GMC_LOSS_EXPECTED_CUT): loss = -C/2 sum_u sum_{v in N(u)} w_uv (1 - Pt_u . Pt_v),
//         GP_u = C sum_{v in N(u)} w_uv Pt_v, Pt = P with rows 0..K-1 replaced by e_0..e_{K-1}; S stays the argmax decode.
// A graph with fewer than K nodes (the host refuses one) has min(K, n) terminals: no access leaves the graph's rows.
// Without terminals (a.terminals == 0, a run-time value: the same instantiation) there are none: no row is overridden, S
// is the first maximum of every row, and both losses are those of gmc_fn_cut_loss_f32 with terminals = 0.
// With a.node_cost (a run-time pointer: the same instantiation) the loss is -C (cut - costsum), costsum = sum_u
// node_cost_u . Pt_u (SOFT) or sum_u node_cost[u][S_u]: gp starts from the node's cost row, so GP_u = C (sum_v w_uv Pt_v +
// node_cost_u), and the row's accumulator of the doubled cut takes cut_u - 2 cost_u - one sum, one block reduction,
// the LDS as it was.
template <int K, bool SOFT>
__global__ __launch_bounds__(head_k_threads(K)) void head_k_kernel(HeadKArgs a) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int g = blockIdx.x;
    const int r0 = a.b.goff[g];
    const int n = a.b.goff[g + 1] - r0;
    const int NP = a.b.n_max + 4;
    float *sA = lds;                                         // [NP*K]  Z0, later dinv*GZ
    float *sP = lds + K * NP;                                // [NP*K]  softmax output (SOFT: Pt)
    float *sT = lds + 2 * K * NP;                            // [K*K]   SOFT: the softmax rows of the terminals
    int *sS = reinterpret_cast<int *>(sT + (SOFT ? K * K : 0));   // [NP] argmax class (after every row array: those
    float *red = reinterpret_cast<float *>(sS) + NP;         // [waves*(K+1)]        keep their 16- / 8-byte alignment)
    const bool train = a.GY2 != nullptr;
    const int terms = a.terminals ? (n < K ? n : K) : 0;

    float bias[K];
#pragma unroll
    for (int k = 0; k < K; ++k) bias[k] = a.b2[(long)g * a.b2_stride + k];
    for (int i = threadIdx.x; i < K * n; i += blockDim.x) sA[i] = a.Z0[(long)r0 * K + i];
    __syncthreads();

    // phase 1: aggregate, bias, softmax, override, argmax
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const int r = r0 + l;
        float z[K] = {};
        for (int e = a.b.rowptr[r]; e < a.b.rowptr[r + 1]; ++e) {
            float q[K];
            load_row<K>(sA, a.b.lcol[e], q);
#pragma unroll
            for (int k = 0; k < K; ++k) z[k] += q[k];
        }
        const float d = a.b.dinv[r];
        float m = -INFINITY;
#pragma unroll
        for (int k = 0; k < K; ++k) { z[k] = fmaf(z[k], d, bias[k]); m = fmaxf(m, z[k]); }
        float p[K], sum = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) { p[k] = expf(z[k] - m); sum += p[k]; }
        const float inv = 1.0f / sum;
#pragma unroll
        for (int k = 0; k < K; ++k) p[k] *= inv;
        store_row<K>(a.P, r, p);
        int s;
        if (l < terms) {
            s = l;  // (e_l + p) - p: 1 at l, exactly 0 elsewhere -> argmax is l
        } else {
            s = 0;  // torch.argmax: first maximum wins
            float best = p[0];
#pragma unroll
            for (int k = 1; k < K; ++k)
                if (p[k] > best) { best = p[k]; s = k; }
        }
        if (SOFT && l < terms) {  // Pt: the terminal rows are e_l; the softmax backward below still needs the row itself
            store_row<K>(sT, l, p);
#pragma unroll
            for (int k = 0; k < K; ++k) p[k] = k == l ? 1.f : 0.f;
        }
        store_row<K>(sP, l, p);
        sS[l] = s;
        if (a.S) a.S[r] = s;
    }
    __syncthreads();

    // phase 2: cut value (+ GP, softmax backward, dinv*GZ when training)
    float acc[K + 1] = {};  // cut2, db2[0..K-1]
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const int r = r0 + l;
        float gp[K] = {}, cut = 0.f;
        if (a.node_cost) {
#pragma unroll
            for (int k = 0; k < K; ++k) gp[k] = a.node_cost[(long)r * K + k];
        }
        float cost = 0.f;   // the node's share of costsum
        if constexpr (SOFT) {
            float u[K];
            load_row<K>(sP, l, u);
            if (a.node_cost) {
#pragma unroll
                for (int k = 0; k < K; ++k) cost += gp[k] * u[k];
            }
            for (int e = a.b.rowptr[r]; e < a.b.rowptr[r + 1]; ++e) {
                const float w = a.b.vals ? a.b.vals[e] : 1.0f;
                float q[K];
                load_row<K>(sP, a.b.lcol[e], q);
                float dot = 0.f;
#pragma unroll
                for (int k = 0; k < K; ++k) { gp[k] += w * q[k]; dot += u[k] * q[k]; }
                cut += w * (1.0f - dot);
            }
        } else {
            const int me = sS[l];
            if (a.node_cost) {
#pragma unroll
                for (int k = 0; k < K; ++k) cost = me == k ? gp[k] : cost;
            }
            for (int e = a.b.rowptr[r]; e < a.b.rowptr[r + 1]; ++e) {
                const float w = a.b.vals ? a.b.vals[e] : 1.0f;
                const int sc = sS[a.b.lcol[e]];
#pragma unroll
                for (int k = 0; k < K; ++k) gp[k] += sc == k ? w : 0.f;
                cut += sc != me ? w : 0.f;
            }
        }
        if (a.node_cost) cut -= 2.0f * cost;   // (acc[0] is halved below)
        acc[0] += cut;
        if (train) {
            float p[K];
            if (SOFT && l < terms) load_row<K>(sT, l, p);
            else load_row<K>(sP, l, p);
            float dot = 0.f;
#pragma unroll
            for (int k = 0; k < K; ++k) { gp[k] *= a.C; dot += gp[k] * p[k]; }
            const float d = a.b.dinv[r];
            float gz[K];
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float zk = p[k] * (gp[k] - dot);
                acc[1 + k] += zk;
                gz[k] = zk * d;
            }
            store_row<K>(sA, l, gz);
        }
    }
    block_sum<K + 1, head_k_threads(K) / 64>(acc, red);  // contains a __syncthreads(): sA writes are visible after it
    if (threadIdx.x == 0) {
        // one system-scope store: `loss` may be pinned host memory the caller watches
        if (a.loss) __hip_atomic_store(a.loss + g, -a.C * (acc[0] * 0.5f), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        if (train) {
#pragma unroll
            for (int k = 0; k < K; ++k) a.db2part[(long)g * K + k] = acc[1 + k];
        }
    }
    if (!train) return;

    // phase 3: GY2 = A @ (dinv o GZ)   (A symmetric: A^T == A)
    for (int l = threadIdx.x; l < n; l += blockDim.x) {
        const int r = r0 + l;
        float y[K] = {};
        for (int e = a.b.rowptr[r]; e < a.b.rowptr[r + 1]; ++e) {
            float q[K];
            load_row<K>(sA, a.b.lcol[e], q);
#pragma unroll
            for (int k = 0; k < K; ++k) y[k] += q[k];
        }
        store_row<K>(a.GY2, r, y);
    }
}

// ---- hidden_bwd_k ---------------------------------------------------------------------------------------------------
constexpr int kTileRows = 64;     // rows per workgroup (gmc_hidden_tiles)
constexpr int kColThreads = 128;  // x float4 = 512 columns per grid.y slice
constexpr int kRowLanes = 2;

struct HiddenKArgs {
    const float *H;
    long ldh;
    const float *GY2;  // [R,K]
    const float *W2;   // [F,K]
    const float *dinv;
    float *Gs;
    long ldg;
    float *part;  // [tiles][F][K+1] = (dW2[f,0..K-1], db1[f])
    int R;
    int F;
};

template <int K>
__global__ __launch_bounds__(kColThreads * kRowLanes) void hidden_bwd_k_kernel(HiddenKArgs a) {
    __shared__ float red[4][K + 1][kColThreads];
    const int ct = threadIdx.x & (kColThreads - 1);
    const int rl = gmc::uniform((int)(threadIdx.x / kColThreads));
    const int c4 = blockIdx.y * kColThreads + ct;  // float4 column index
    const int F4 = a.F >> 2;
    const bool on = c4 < F4;
    const int cl = on ? c4 : F4 - 1;
    float w[4][K];
#pragma unroll
    for (int j = 0; j < 4; ++j) load_row<K>(a.W2, cl * 4 + j, w[j]);

    float dw[4][K] = {};
    float db[4] = {};
    const int rbeg = blockIdx.x * kTileRows;
    const int rend = min(rbeg + kTileRows, a.R);
#pragma unroll 2
    for (int r = rbeg + rl; r < rend; r += kRowLanes) {
        const float4 h = reinterpret_cast<const float4 *>(a.H + (long)r * a.ldh)[cl];
        const float d = a.dinv[r];
        float gy[K];
        load_row<K>(a.GY2, r, gy);   // (wave-uniform address: scalar loads)
        const float hv[4] = {h.x, h.y, h.z, h.w};
        float gs[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float gh = gy[0] * w[j][0];
#pragma unroll
            for (int k = 1; k < K; ++k) gh += gy[k] * w[j][k];
            const float gpre = hv[j] > 0.f ? gh * d : 0.f;
            gs[j] = gpre * d;
            db[j] += gpre;
            const float hd = hv[j] * d;
#pragma unroll
            for (int k = 0; k < K; ++k) dw[j][k] = fmaf(hd, gy[k], dw[j][k]);
        }
        if (on) reinterpret_cast<float4 *>(a.Gs + (long)r * a.ldg)[c4] = make_float4(gs[0], gs[1], gs[2], gs[3]);
    }
    // fold the row lanes (fixed order), then K + 1 floats per (thread, column)
    if (rl == 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < K; ++k) red[j][k][ct] = dw[j][k];
            red[j][K][ct] = db[j];
        }
    }
    __syncthreads();
    if (rl == 0 && on) {
        float *out = a.part + ((long)blockIdx.x * a.F + (long)c4 * 4) * (K + 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < K; ++k) out[j * (K + 1) + k] = dw[j][k] + red[j][k][ct];
            out[j * (K + 1) + K] = db[j] + red[j][K][ct];
        }
    }
}

// ---- reduce_k -------------------------------------------------------------------------------------------------------
// dW2[f,k], db1[f] = sum over tiles of part[tile][f][:]; db2 = sum over graphs (ascending).  The tiles are dealt over
// kRedLanes lanes, each ascending, then the lanes are added in ascending order: colsum_reduce_kernel's order.
struct ReduceKArgs {
    const float *part;
    int tiles;
    int F;
    float *dW2;
    float *db1;
    const float *db2part;
    int B;
    float *db2;
};

constexpr int kRedCols = 16;
constexpr int kRedLanes = 64;

template <int K>
__global__ __launch_bounds__(kRedCols * kRedLanes) void reduce_k_kernel(ReduceKArgs a) {
    __shared__ float red[kRedLanes][K + 1][kRedCols];
    const int cl = threadIdx.x & (kRedCols - 1);
    const int tl = threadIdx.x / kRedCols;
    if ((int)blockIdx.x == (a.F + kRedCols - 1) / kRedCols) {  // extra block: db2
        if (threadIdx.x < K) {
            float s = 0.f;
            for (int g = 0; g < a.B; ++g) s += a.db2part[(long)g * K + threadIdx.x];
            a.db2[threadIdx.x] = s;
        }
        return;
    }
    const int f = blockIdx.x * kRedCols + cl;
    float s[K + 1] = {};
    if (f < a.F) {
#pragma unroll 2
        for (int t = tl; t < a.tiles; t += kRedLanes) {
            const float *p = a.part + ((long)t * a.F + f) * (K + 1);
#pragma unroll
            for (int k = 0; k <= K; ++k) s[k] += p[k];
        }
    }
#pragma unroll
    for (int k = 0; k <= K; ++k) red[tl][k][cl] = s[k];
    __syncthreads();
    if (tl <= K && f < a.F) {  // thread (column, k = tl): the lanes' partials in ascending order
        float t = red[0][tl][cl];
#pragma unroll 8
        for (int i = 1; i < kRedLanes; ++i) t += red[i][tl][cl];
        if (tl < K) a.dW2[(long)f * K + tl] = t;
        else a.db1[f] = t;
    }
}

}  // namespace

int gmc_kway_hw2_launch(const float *H, long ld, const float *dinv, const float *W2, float *Z0, long R, int F, int K,
                        hipStream_t st) {
    if (R == 0) return GMC_OK;
    Hw2KArgs a{H, dinv, W2, Z0, R, F, ld};
    GmcProbeScope probe(GMC_K_DENSE_MFMA, st);   // the tag of the stand-alone H @ W2 product (gmc_dense_hw2_f32)
    GMC_KWAY_DISPATCH(K, hipLaunchKernelGGL(hw2_k_kernel<KK>, dim3((unsigned)((R + 3) / 4)), dim3(256), 0, st, a));
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

size_t gmc_kway_head_lds_bytes(int n_max, int K, int loss_kind) {
    return sizeof(float) * head_k_lds_floats(n_max, K, loss_kind == GMC_LOSS_EXPECTED_CUT);
}

template <int K, bool SOFT>
static int head_k_launch(const HeadKArgs &a, size_t lds, hipStream_t st) {
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(head_k_kernel<K, SOFT>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return (int)e;
    }
    GmcProbeScope probe(GMC_K_HEAD, st);
    hipLaunchKernelGGL((head_k_kernel<K, SOFT>), dim3(a.b.B), dim3(head_k_threads(K)), lds, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// GY2 == nullptr: forward only.  The graphs' tiles must fit a CU's LDS (GMC_ERR_GRAPH_SIZE otherwise).
int gmc_kway_head_launch(const gmc_batch *b, const float *Z0, const float *b2, float C, int K, int loss_kind, float *P,
                         int32_t *S, float *loss, float *GY2, float *db2part, hipStream_t st, long b2_stride,
                         int terminals, const float *node_cost) {
    if (!b || !Z0 || !b2 || !P || (GY2 && !db2part)) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    const size_t lds = gmc_kway_head_lds_bytes(b->n_max, K, loss_kind);
    if (lds > GMC_KWAY_LDS_BYTES) return GMC_ERR_GRAPH_SIZE;
    if (b->B == 0) return GMC_OK;
    HeadKArgs a{*b, Z0, b2, C, P, S, loss, GY2, db2part, b2_stride, terminals, node_cost};
    const bool soft = loss_kind == GMC_LOSS_EXPECTED_CUT;
    GMC_KWAY_DISPATCH(K, return soft ? head_k_launch<KK, true>(a, lds, st) : head_k_launch<KK, false>(a, lds, st));
    return GMC_OK;
}

// part must hold gmc_hidden_tiles(R) * F * (K + 1) floats
int gmc_kway_hidden_bwd_launch(const float *H, long ldh, const float *GY2, const float *W2, const float *dinv, float *Gs,
                               long ldg, float *part, int R, int F, int K, hipStream_t st) {
    if (F % 4 || ldh % 4 || ldg % 4) return GMC_ERR_ALIGN;
    if (R == 0) return GMC_OK;
    HiddenKArgs a{H, ldh, GY2, W2, dinv, Gs, ldg, part, R, F};
    dim3 grid(gmc_hidden_tiles(R), (F / 4 + kColThreads - 1) / kColThreads);   // (kTileRows rows each, as hidden_bwd.hip)
    GmcProbeScope probe(GMC_K_HIDDEN_BWD, st);
    GMC_KWAY_DISPATCH(K, hipLaunchKernelGGL(hidden_bwd_k_kernel<KK>, grid, dim3(kColThreads * kRowLanes), 0, st, a));
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

int gmc_kway_reduce_launch(const float *part, int tiles, int F, int K, float *dW2, float *db1, const float *db2part,
                           int B, float *db2, hipStream_t st) {
    ReduceKArgs a{part, tiles, F, dW2, db1, db2part, B, db2};
    const int grid = (F + kRedCols - 1) / kRedCols + 1;
    GmcProbeScope probe(GMC_K_COLSUM, st);
    GMC_KWAY_DISPATCH(K, hipLaunchKernelGGL(reduce_k_kernel<KK>, dim3(grid), dim3(kRedCols * kRedLanes), 0, st, a));
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
