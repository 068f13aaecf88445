// One model per graph (include/gcnmaxcut.h, gmc_inst_*): the kernels of the K-class row-kernel sequence that have to know
// which graph a row belongs to, because every graph of the batch brings its own conv1.bias, conv2.weight and conv2.bias.
//   inst_hw2_k         H[r,:] = relu(Hpre[r,:] + b1_g) written back in place, Z0[r,:] = dinv[r] * (H[r,:] @ W2_g)   [R,K]
//                      (hw2_k_kernel of kway.hip with the row's graph selecting b1 and W2; the per-graph bias and the
//                      relu of layer 1 ride in front of it, so H is read and written once for both)
//   inst_hidden_bwd_k  Gs = dinv o relu'(H) o dinv o (GY2 @ W2_g^T), tile partials of dW2_g [F,K] and db1_g [F]
//                      (hidden_bwd_k_kernel of kway.hip over tiles that start at the graph's first row)
//   inst_fold          dW2_g, db1_g = the graph's tile partials, added in ascending tile order
//   keep_best          rows of S -> best_S for the graphs whose loss improved, then best_loss / best_epoch
//   early_stop         keep_best behind the reference's tolerance / patience rule, per graph: a graph that stops is
//                      frozen from then on (gmc_inst_early_stop_f32)
//   inst_adam          adam.hip's update over the flat buffer cut by graph, so that a stopped graph's parameters,
//                      gradient and moments are neither read nor written (gmc_inst_adam_f32)
// The head is head_k_kernel of kway.hip with a bias stride (gmc_kway_head_launch); the W1 gather, both F-wide
// aggregations and dW1 are gmc_spmm_launch; Adam without early stopping is adam.hip's over the flat buffer.
//
// Grid of the row kernels: (graph, tile of the graph's rows) as in large.hip - blockIdx.x is the graph, so a row's graph
// is known without a search and without a [R] graph-id array; a tile past the graph's end returns at once.  A tile's
// partials live in slot goff[g] / 64 + g + tile (large.hip's scheme: disjoint for any sizes, R / 64 + B + 1 in all).
// No float atomics; every sum in a fixed order that depends on the graph alone: a graph's results have the same bits
// wherever it stands in a batch and whatever stands next to it.
#include "kway_rows.h"
#include "adam_body.h"

namespace {

// ---- inst_hw2_k -----------------------------------------------------------------------------------------------------
struct InstHw2Args {
    const int *goff;
    float *H;            // [R,ld] in: dinv o (A @ T0); out: relu(. + b1_g)
    const float *dinv;
    const float *b1;     // [B,F]
    const float *W2;     // [B,F,K]
    float *Z0;           // [R,K]
    int F;
    long ld;
};

// one wave per row, fixed-order butterfly sum; grid (B, ceil(n_max / 4))
template <int K>
__global__ __launch_bounds__(256) void inst_hw2_k_kernel(InstHw2Args a) {
    const int g = blockIdx.x;
    const int r0 = a.goff[g];
    const int n = a.goff[g + 1] - r0;
    const int l = gmc::uniform((int)(blockIdx.y * 4 + (threadIdx.x >> 6)));
    if (l >= n) return;
    const long r = (long)r0 + l;
    const int lane = gmc::lane_id();
    const float *b1 = a.b1 + (long)g * a.F;
    const float *W2 = a.W2 + (long)g * a.F * K;
    float *h_row = a.H + r * a.ld;
    float z[K] = {};
    for (int c = lane; c < a.F; c += GMC_WAVE) {
        const float pre = h_row[c] + b1[c];
        const float h = pre > 0.f ? pre : 0.f;
        h_row[c] = h;
        float w[K];
        load_row<K>(W2, c, w);
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

// ---- inst_hidden_bwd_k ----------------------------------------------------------------------------------------------
constexpr int kTileRows = 64;     // rows per workgroup
constexpr int kColThreads = 128;  // x float4 = 512 columns per grid.z slice
constexpr int kRowLanes = 2;

struct InstHiddenArgs {
    const int *goff;
    const float *H;
    long ldh;
    const float *GY2;  // [R,K]
    const float *W2;   // [B,F,K]
    const float *dinv;
    float *Gs;
    long ldg;
    float *part;       // [slots][F][K+1] = (dW2[f,0..K-1], db1[f])
    int F;
};

// hidden_bwd_k_kernel of kway.hip per (graph, tile, column slice); the two row lanes take the tile's even and odd rows
// counted from the graph's first row
template <int K>
__global__ __launch_bounds__(kColThreads * kRowLanes) void inst_hidden_bwd_k_kernel(InstHiddenArgs a) {
    __shared__ float red[4][K + 1][kColThreads];
    const int g = blockIdx.x;
    const int r0 = a.goff[g];
    const int n = a.goff[g + 1] - r0;
    if ((int)blockIdx.y * kTileRows >= n) return;   // (workgroup-uniform)
    const int ct = threadIdx.x & (kColThreads - 1);
    const int rl = gmc::uniform((int)(threadIdx.x / kColThreads));
    const int c4 = blockIdx.z * kColThreads + ct;  // float4 column index
    const int F4 = a.F >> 2;
    const bool on = c4 < F4;
    const int cl = on ? c4 : F4 - 1;
    const float *W2 = a.W2 + (long)g * a.F * K;
    float w[4][K];
#pragma unroll
    for (int j = 0; j < 4; ++j) load_row<K>(W2, cl * 4 + j, w[j]);

    float dw[4][K] = {};
    float db[4] = {};
    const int rbeg = r0 + (int)blockIdx.y * kTileRows;
    const int rend = min(rbeg + kTileRows, r0 + n);
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
        const long slot = (long)(r0 / kTileRows) + g + blockIdx.y;
        float *out = a.part + (slot * a.F + (long)c4 * 4) * (K + 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
#pragma unroll
            for (int k = 0; k < K; ++k) out[j * (K + 1) + k] = dw[j][k] + red[j][k][ct];
            out[j * (K + 1) + K] = db[j] + red[j][K][ct];
        }
    }
}

// ---- inst_fold ------------------------------------------------------------------------------------------------------
struct InstFoldArgs {
    const int *goff;
    const float *part;
    int F, K;
    float *dW2;   // [B,F,K]
    float *db1;   // [B,F]
};

constexpr int kFoldThreads = 256;

// thread = one of the F * (K + 1) entries of a graph's partial; the graph's tiles one after the other, ascending
__global__ __launch_bounds__(kFoldThreads) void inst_fold_kernel(InstFoldArgs a) {
    const int g = blockIdx.x;
    const int i = blockIdx.y * kFoldThreads + threadIdx.x;
    const int per = a.F * (a.K + 1);
    if (i >= per) return;
    const int r0 = a.goff[g];
    const int n = a.goff[g + 1] - r0;
    const int tiles = (n + kTileRows - 1) / kTileRows;
    const float *p = a.part + ((long)(r0 / kTileRows) + g) * per + i;
    float s = 0.f;
    for (int t = 0; t < tiles; ++t) s += p[(long)t * per];
    const int f = i / (a.K + 1), k = i - f * (a.K + 1);
    if (k < a.K) a.dW2[((long)g * a.F + f) * a.K + k] = s;
    else a.db1[(long)g * a.F + f] = s;
}

// ---- keep_best ------------------------------------------------------------------------------------------------------
struct KeepArgs {
    const int *goff;
    const int *S;
    const float *loss;
    int *best_S;
    float *best_loss;
    int *best_epoch;
    int epoch;
    int B;
};

constexpr int kKeepRows = 256;

// launch 1, grid (B, ceil(n_max / 256)): the rows of the graphs that improved.  best_loss is only read here - its store
// is launch 2's, behind the kernel boundary, so every workgroup of a graph sees the same comparison.
__global__ __launch_bounds__(kKeepRows) void keep_rows_kernel(KeepArgs a) {
    const int g = blockIdx.x;
    if (!(a.loss[g] < a.best_loss[g])) return;   // strict: the first minimum stays; a NaN loss never wins
    const int r0 = a.goff[g];
    const int l = (int)blockIdx.y * kKeepRows + (int)threadIdx.x;
    if (l < a.goff[g + 1] - r0) a.best_S[r0 + l] = a.S[r0 + l];
}

// launch 2: one thread per graph
__global__ __launch_bounds__(256) void keep_loss_kernel(KeepArgs a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.B) return;
    const float v = a.loss[g];
    if (v < a.best_loss[g]) {
        a.best_loss[g] = v;
        a.best_epoch[g] = a.epoch;
    }
}

// ---- early_stop -----------------------------------------------------------------------------------------------------
struct StopArgs {
    const int *goff;
    const int *S;
    const float *loss;
    float *prev_loss;
    int *stall;
    int *stop_epoch;
    int *best_S;
    float *best_loss;
    int *best_epoch;
    double tolerance;
    int epoch, patience, B;
};

// The rule of include/gcnmaxcut.h (TrainingNeural.py:429-444) for a graph that was running on entry: has the loss
// stalled in this epoch, and does that stall stop the graph now?  Both launches read the same state and evaluate this.
// Comparisons as written: a NaN loss never stalls; inf - inf is NaN in double as in Python and does not stall either.
__device__ __forceinline__ bool stop_stalled(const StopArgs &a, int g, float L) {
    const float p = a.prev_loss[g];
    return a.epoch > 0 && (L > p || fabs((double)p - (double)L) <= a.tolerance);
}

// launch 1, grid (B, ceil(n_max / 256)): the rows of the graphs that run, do not stop now and improved.  Every word
// of per-graph state is only read here - launch 2 stores it behind the kernel boundary.
__global__ __launch_bounds__(kKeepRows) void stop_rows_kernel(StopArgs a) {
    const int g = blockIdx.x;
    if (a.stop_epoch[g] >= 0) return;
    const float L = a.loss[g];
    if (stop_stalled(a, g, L) && a.stall[g] + 1 >= a.patience) return;   // stops now: the reference breaks before keep-best
    if (!(L < a.best_loss[g])) return;
    const int r0 = a.goff[g];
    const int l = (int)blockIdx.y * kKeepRows + (int)threadIdx.x;
    if (l < a.goff[g + 1] - r0) a.best_S[r0 + l] = a.S[r0 + l];
}

// launch 2: one thread per graph
__global__ __launch_bounds__(256) void stop_state_kernel(StopArgs a) {
    const int g = blockIdx.x * 256 + threadIdx.x;
    if (g >= a.B) return;
    if (a.stop_epoch[g] >= 0) return;            // stopped earlier: nothing of it is written
    const float L = a.loss[g];
    if (stop_stalled(a, g, L)) {
        const int s = a.stall[g] + 1;
        a.stall[g] = s;
        if (s >= a.patience) {
            a.stop_epoch[g] = a.epoch;
            return;
        }
    } else {
        a.stall[g] = 0;
    }
    if (L < a.best_loss[g]) {
        a.best_loss[g] = L;
        a.best_epoch[g] = a.epoch;
    }
    a.prev_loss[g] = L;
}

// ---- inst_adam ------------------------------------------------------------------------------------------------------
constexpr int kAdamThreads = 256;
constexpr int kAdamUnroll = 4;                                // float4 per thread, all loaded before the first update
constexpr int kAdamTile4 = kAdamThreads * kAdamUnroll;        // float4 of a graph's W1 per workgroup
constexpr int kAdamTileFloats = kAdamTile4 * 4;               // also the floats of a tile of the small blocks
static_assert(kAdamTileFloats == GMC_INST_ADAM_TILE_FLOATS, "include/gcnmaxcut.h documents the tile");

struct InstAdamArgs {
    gmc::AdamArgs a;
    const int *goff;
    const int *stop_epoch;   // NULL: all running
    int F, K;
    long off_b1, off_w2, off_b2;
    int w1_tiles;            // tiles of the largest graph's W1; the tiles from there on are the three small blocks'
};

// grid (B, w1_tiles + small tiles).  A workgroup of a stopped graph leaves after one (scalar) load; a tile past the
// graph's end likewise.  W1: float4 i of the graph's n_g * F / 4, thread t of tile j takes j * 1024 + t + 256 u.  The small
// blocks b1_g | W2_g | b2_g: scalar, because a K = 3 b2 segment starts off a 16-byte boundary.
__global__ __launch_bounds__(kAdamThreads) void inst_adam_kernel(InstAdamArgs q) {
    const int g = blockIdx.x;
    if (q.stop_epoch && q.stop_epoch[g] >= 0) return;
    const int t = blockIdx.y;
    if (t < q.w1_tiles) {
        const int r0 = q.goff[g];
        const long n4 = (long)(q.goff[g + 1] - r0) * (q.F >> 2);
        const long i0 = (long)t * kAdamTile4 + threadIdx.x;
        if ((long)t * kAdamTile4 >= n4) return;
        const long base = (long)r0 * q.F;
        float4 *P = reinterpret_cast<float4 *>(q.a.p + base);
        const float4 *G = reinterpret_cast<const float4 *>(q.a.g + base);
        float4 *M = reinterpret_cast<float4 *>(q.a.m + base);
        float4 *V = reinterpret_cast<float4 *>(q.a.v + base);
        float4 p[kAdamUnroll], gr[kAdamUnroll], m[kAdamUnroll], v[kAdamUnroll];
#pragma unroll
        for (int u = 0; u < kAdamUnroll; ++u) {
            const long i = i0 + u * kAdamThreads;
            if (i < n4) {
                p[u] = P[i];
                gr[u] = G[i];
                m[u] = M[i];
                v[u] = V[i];
            }
        }
#pragma unroll
        for (int u = 0; u < kAdamUnroll; ++u) {
            const long i = i0 + u * kAdamThreads;
            if (i < n4) {
                gmc::adam4(p[u], gr[u], m[u], v[u], q.a);
                P[i] = p[u];
                M[i] = m[u];
                V[i] = v[u];
            }
        }
        return;
    }
    const int FK = q.F * q.K;
    const int per = q.F + FK + q.K;
    const int s0 = (t - q.w1_tiles) * kAdamTileFloats;
    const int s1 = min(s0 + kAdamTileFloats, per);
    for (int i = s0 + (int)threadIdx.x; i < s1; i += kAdamThreads) {
        const long e = i < q.F        ? q.off_b1 + (long)g * q.F + i
                       : i < q.F + FK ? q.off_w2 + (long)g * FK + (i - q.F)
                                      : q.off_b2 + (long)g * q.K + (i - q.F - FK);
        gmc::adam1(q.a.p[e], q.a.g[e], q.a.m[e], q.a.v[e], q.a);
    }
}

}  // namespace

size_t gmc_inst_part_floats(const gmc_batch *b, int F, int K) {
    return ((size_t)b->R / kTileRows + (size_t)b->B + 1) * (size_t)F * (size_t)(K + 1);
}

int gmc_inst_hw2_launch(const gmc_batch *b, float *H, long ld, const float *b1, const float *W2, float *Z0, int F, int K,
                        hipStream_t st) {
    if (b->B == 0) return GMC_OK;
    InstHw2Args a{b->goff, H, b->dinv, b1, W2, Z0, F, ld};
    const dim3 grid(b->B, (b->n_max + 3) / 4);
    GmcProbeScope probe(GMC_K_DENSE_MFMA, st);   // the tag of hw2_k in the K-class sequence
    GMC_KWAY_DISPATCH(K, hipLaunchKernelGGL(inst_hw2_k_kernel<KK>, grid, dim3(256), 0, st, a));
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// part must hold gmc_inst_part_floats(b, F, K) floats
int gmc_inst_hidden_bwd_launch(const gmc_batch *b, const float *H, long ldh, const float *GY2, const float *W2, float *Gs,
                               long ldg, float *part, int F, int K, hipStream_t st) {
    if (F % 4 || ldh % 4 || ldg % 4) return GMC_ERR_ALIGN;
    if (b->B == 0) return GMC_OK;
    InstHiddenArgs a{b->goff, H, ldh, GY2, W2, b->dinv, Gs, ldg, part, F};
    const dim3 grid(b->B, (b->n_max + kTileRows - 1) / kTileRows, (F / 4 + kColThreads - 1) / kColThreads);
    GmcProbeScope probe(GMC_K_HIDDEN_BWD, st);
    GMC_KWAY_DISPATCH(K, hipLaunchKernelGGL(inst_hidden_bwd_k_kernel<KK>, grid, dim3(kColThreads * kRowLanes), 0, st, a));
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

int gmc_inst_fold_launch(const gmc_batch *b, const float *part, int F, int K, float *dW2, float *db1, hipStream_t st) {
    if (b->B == 0) return GMC_OK;
    InstFoldArgs a{b->goff, part, F, K, dW2, db1};
    const dim3 grid(b->B, (F * (K + 1) + kFoldThreads - 1) / kFoldThreads);
    GmcProbeScope probe(GMC_K_COLSUM, st);
    hipLaunchKernelGGL(inst_fold_kernel, grid, dim3(kFoldThreads), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" int gmc_inst_keep_best_f32(const gmc_batch *batch, const int32_t *S, const float *loss, int32_t epoch,
                                      int32_t *best_S, float *best_loss, int32_t *best_epoch, gmc_stream_t stream) {
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !S || !loss || !best_S || !best_loss || !best_epoch) return GMC_ERR_NULL;
    if (batch->B < 0 || batch->R < 0 || (batch->B > 0 && batch->n_max < 1)) return GMC_ERR_SHAPE;
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    KeepArgs a{batch->goff, S, loss, best_S, best_loss, best_epoch, epoch, batch->B};
    {
        GmcProbeScope probe(GMC_K_FINISH, st);
        hipLaunchKernelGGL(keep_rows_kernel, dim3(batch->B, (batch->n_max + kKeepRows - 1) / kKeepRows), dim3(kKeepRows), 0,
                           st, a);
        GMC_LAUNCH_CHECK();
    }
    GmcProbeScope probe(GMC_K_FINISH, st);
    hipLaunchKernelGGL(keep_loss_kernel, dim3((batch->B + 255) / 256), dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" int gmc_inst_early_stop_f32(const gmc_batch *batch, const int32_t *S, const float *loss, int32_t epoch,
                                       double tolerance, int32_t patience, float *prev_loss, int32_t *stall,
                                       int32_t *stop_epoch, int32_t *best_S, float *best_loss, int32_t *best_epoch,
                                       gmc_stream_t stream) {
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !S || !loss || !prev_loss || !stall || !stop_epoch || !best_S || !best_loss || !best_epoch)
        return GMC_ERR_NULL;
    if (batch->B < 0 || batch->R < 0 || (batch->B > 0 && batch->n_max < 1)) return GMC_ERR_SHAPE;
    if (patience < 1 || !(tolerance >= 0.0)) return GMC_ERR_SHAPE;   // (a NaN tolerance compares false)
    if (batch->B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    StopArgs a{batch->goff, S, loss, prev_loss, stall, stop_epoch, best_S, best_loss, best_epoch, tolerance, epoch, patience,
               batch->B};
    {
        GmcProbeScope probe(GMC_K_FINISH, st);
        hipLaunchKernelGGL(stop_rows_kernel, dim3(batch->B, (batch->n_max + kKeepRows - 1) / kKeepRows), dim3(kKeepRows), 0,
                           st, a);
        GMC_LAUNCH_CHECK();
    }
    GmcProbeScope probe(GMC_K_FINISH, st);
    hipLaunchKernelGGL(stop_state_kernel, dim3((batch->B + 255) / 256), dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" int gmc_inst_adam_f32(const gmc_batch *batch, int32_t F, int32_t K, float *param, const float *grad, float *m,
                                 float *v, double lr, double beta1, double beta2, double eps, int32_t step,
                                 const int32_t *stop_epoch, gmc_stream_t stream) {
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !param || !grad || !m || !v) return GMC_ERR_NULL;
    if (batch->B < 0 || batch->R < 0 || (batch->B > 0 && batch->n_max < 1) || F < 1 || K < 1 || step < 1) return GMC_ERR_SHAPE;
    if (F % 4) return GMC_ERR_ALIGN;
    if (!gmc_aligned16(param) || !gmc_aligned16(grad) || !gmc_aligned16(m) || !gmc_aligned16(v)) return GMC_ERR_ALIGN;
    if (batch->B == 0) return GMC_OK;
    const long R = batch->R, B = batch->B;
    const long count = R * F + B * ((long)F + (long)F * K + K);
    InstAdamArgs q{gmc::adam_args(param, grad, m, v, count, lr, beta1, beta2, eps, step), batch->goff, stop_epoch, F, K,
                   R * F, R * F + B * F, R * F + B * F + B * F * K, 0};
    const long w1_tiles = ((long)batch->n_max * (F / 4) + kAdamTile4 - 1) / kAdamTile4;
    const long small_tiles = ((long)F + (long)F * K + K + kAdamTileFloats - 1) / kAdamTileFloats;
    if (w1_tiles + small_tiles > 65535) return GMC_ERR_SHAPE;   // (n_max * F beyond 2^28: no batch of this library)
    q.w1_tiles = (int)w1_tiles;
    hipStream_t st = static_cast<hipStream_t>(stream);
    GmcProbeScope probe(GMC_K_ADAM, st);
    hipLaunchKernelGGL(inst_adam_kernel, dim3(batch->B, (unsigned)(w1_tiles + small_tiles)), dim3(kAdamThreads), 0, st, q);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
