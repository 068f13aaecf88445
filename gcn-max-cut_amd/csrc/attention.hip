// Graph-attention first layer (single-head GAT on the graph with self-loops added, then relu): the kernels of the
// gmc_att_* entry points (include/gcnmaxcut.h states the model).
//
// Row kernels on plain row-major [R, ld] buffers, one wave64 per row, in the style of spmm.hip.  The terms of row i are
// its CSR entries (CSR order) followed by ONE self term; term t of a row lives in lane t % 64 of its chunk of 64 terms.
//   att_scores      s_src[r] = T[r,:] . a_src, s_dst[r] = T[r,:] . a_dst                    (butterfly sum: hw2_rows_kernel)
//   att_fwd         z = s_dst[i] + s_src[j], e = leaky_relu(z), alpha = softmax over the row's terms (lanes over the
//                   terms, rows with more than 64 terms loop), alpha stored per CSR entry and per row (self term);
//                   H[i,:] = relu(sum_t alpha_t * T[j_t,:] + b1): lane -> SGPR broadcasts of (j_t, alpha_t), up to 8 row
//                   gathers in flight, the adds in term order
//   gy2_scale       GY2[r,0..2] *= dinv[r] (layer 2's row scale), ones[r] = 1: gmc_hidden_bwd_launch with `ones` as its
//                   dinv then leaves G = relu'(H) o ((dinv o GY2) @ W2^T), db1 = colsum(G), dW2 = H^T @ (dinv o GY2)
//   att_edge_bwd    da_t = G[i,:] . T[j_t,:] (a wave dot product per term, the T rows gathered again), softmax and
//                   leaky-relu backward: dz per entry / self term, ds_dst per row
//   att_bwd_t       the transposed aggregation: row j of the symmetric CSR lists the rows i that have j as a term; alpha_ij
//                   and dz_ij are read from the REVERSE entry, found by a binary search for j in row i (rows are sorted by
//                   column); ds_src[j] = sum dz_ij, dT[j,:] = sum alpha_ij * G[i,:] + ds_src[j] * a_src + ds_dst[j] * a_dst
//   att_avec_part / att_avec_fold   da_src = sum_j ds_src[j] * T[j,:], da_dst = sum_i ds_dst[i] * T[i,:]: partials per
//                   tile of 64 rows, then a fixed-order fold (hidden_bwd / colsum_reduce's scheme)
// No float atomics; every sum runs in a fixed order: two runs give the same bytes.
#include "launchers.h"

namespace {

constexpr int kWavesPerWg = 4;    // one row per wave
constexpr int kUnroll = 8;        // rows in flight per lane in the weighted gathers (divides 64)
constexpr int kDotUnroll = 4;     // T rows in flight in the edge backward
constexpr int kTileRows = 64;     // rows per partial of da_src / da_dst
constexpr int kRedCols = 16;
constexpr int kRedLanes = 64;

__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}

__device__ __forceinline__ float leaky(float z, float slope) { return z > 0.f ? z : slope * z; }

__device__ __forceinline__ float dot4(const float4 &a, const float4 &b, float acc) {
    acc = fmaf(a.x, b.x, acc); acc = fmaf(a.y, b.y, acc); acc = fmaf(a.z, b.z, acc); acc = fmaf(a.w, b.w, acc);
    return acc;
}

__device__ __forceinline__ float bcast(float v, int l) {
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), l));
}

// (beg, end) of CSR row r, wave-uniform
__device__ __forceinline__ void row_range(const int *rowptr, int r, int lane, int &beg, int &end) {
    const int rp = rowptr[r + min(lane, 1)];
    beg = __builtin_amdgcn_readlane(rp, 0);
    end = __builtin_amdgcn_readlane(rp, 1);
}

// One chunk of up to 64 terms: acc[p] += w_t * X[c_t, columns of p] for t = 0..cnt-1 in order; lane t holds (c_t, w_t),
// lanes >= cnt a valid row id.  All lane -> SGPR broadcasts first, then up to kUnroll row gathers in flight.
template <int NP>
__device__ __forceinline__ void gather_weighted(const float *X, long ldx, int myc, float myw, int cnt, const int (&cc)[NP],
                                                float4 (&acc)[NP]) {
#pragma unroll 1
    for (int j = 0; j < cnt; j += kUnroll) {
        float4 x[kUnroll][NP];
        float w[kUnroll];
        const float *src[kUnroll];
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            const long c = __builtin_amdgcn_readlane(myc, j + u);
            w[u] = bcast(myw, j + u);
            src[u] = X + c * ldx;
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (j + u < cnt) {  // wave-uniform
#pragma unroll
                for (int p = 0; p < NP; ++p) x[u][p] = reinterpret_cast<const float4 *>(src[u])[cc[p]];
            }
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) {
            if (j + u < cnt) {
#pragma unroll
                for (int p = 0; p < NP; ++p) gmc::f4_fma(acc[p], w[u], x[u][p]);
            }
        }
    }
}

// ---- att_scores -----------------------------------------------------------------------------------------------------
struct ScoreArgs {
    const float *T;
    long ld;
    const float *a_src, *a_dst;
    float *s_src, *s_dst;
    long R;
    int F;
};

__global__ __launch_bounds__(256) void att_scores_kernel(ScoreArgs a) {
    const long r = (long)blockIdx.x * kWavesPerWg + (threadIdx.x >> 6);
    if (r >= a.R) return;
    const int lane = gmc::lane_id();
    float s = 0.f, d = 0.f;
    for (int c = lane; c < a.F; c += GMC_WAVE) {
        const float t = a.T[r * a.ld + c];
        s = fmaf(t, a.a_src[c], s);
        d = fmaf(t, a.a_dst[c], d);
    }
    s = gmc::wave_sum(s);
    d = gmc::wave_sum(d);
    if (lane == 0) {
        a.s_src[r] = s;
        a.s_dst[r] = d;
    }
}

// ---- att_fwd --------------------------------------------------------------------------------------------------------
struct FwdArgs {
    const int *rowptr, *gcol;
    const float *T;
    long ld;
    const float *s_src, *s_dst;
    float slope;
    const float *bias;
    float *alpha_e;   // [nnz]
    float *alpha_s;   // [R] the self terms
    float *H;
    int R;
    int F;
};

// NP: 256-column passes of a lane per column block (a block is 256 * NP columns; wider rows loop over blocks)
template <int NP>
__global__ __launch_bounds__(256) void att_fwd_kernel(FwdArgs a) {
    const int lane = gmc::lane_id();
    const int i = gmc::uniform((int)(blockIdx.x * kWavesPerWg + (threadIdx.x >> 6)));
    if (i >= a.R) return;
    int beg, end;
    row_range(a.rowptr, i, lane, beg, end);
    const int deg = end - beg, nt = deg + 1;
    const float sd = a.s_dst[i];

    // softmax statistics over the terms (lanes over the terms)
    float m = -INFINITY;
#pragma unroll 1
    for (int t0 = 0; t0 < nt; t0 += 64) {
        const int t = t0 + lane;
        if (t < nt) m = fmaxf(m, leaky(sd + a.s_src[t < deg ? a.gcol[beg + t] : i], a.slope));
    }
    m = wave_max(m);
    float sum = 0.f;
#pragma unroll 1
    for (int t0 = 0; t0 < nt; t0 += 64) {
        const int t = t0 + lane;
        if (t < nt) sum += expf(leaky(sd + a.s_src[t < deg ? a.gcol[beg + t] : i], a.slope) - m);
    }
    sum = gmc::wave_sum(sum);

    const int F4 = a.F >> 2;
#pragma unroll 1
    for (int cb = 0; cb < F4; cb += 64 * NP) {   // (wave-uniform) column blocks
        bool on[NP];
        int cc[NP];
        float4 acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int c = cb + lane + 64 * p;
            on[p] = c < F4;
            cc[p] = on[p] ? c : F4 - 1;
            acc[p] = gmc::f4_zero();
        }
#pragma unroll 1
        for (int t0 = 0; t0 < nt; t0 += 64) {
            const int t = t0 + lane;
            const bool have = t < nt;
            const int col = have && t < deg ? a.gcol[beg + t] : i;
            float alpha = 0.f;
            if (have) {
                alpha = expf(leaky(sd + a.s_src[col], a.slope) - m) / sum;
                if (cb == 0) {
                    if (t < deg) a.alpha_e[beg + t] = alpha;
                    else a.alpha_s[i] = alpha;
                }
            }
            gather_weighted<NP>(a.T, a.ld, col, alpha, min(64, nt - t0), cc, acc);
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float4 b = reinterpret_cast<const float4 *>(a.bias)[cc[p]];
            float4 y;
            y.x = acc[p].x + b.x; y.y = acc[p].y + b.y; y.z = acc[p].z + b.z; y.w = acc[p].w + b.w;
            y.x = y.x > 0.f ? y.x : 0.f; y.y = y.y > 0.f ? y.y : 0.f;
            y.z = y.z > 0.f ? y.z : 0.f; y.w = y.w > 0.f ? y.w : 0.f;
            if (on[p]) reinterpret_cast<float4 *>(a.H + (long)i * a.ld)[cb + lane + 64 * p] = y;
        }
    }
}

// ---- gy2_scale ------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void att_gy2_scale_kernel(float *GY2, const float *dinv, float *ones, int R) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= R) return;
    const float d = dinv[r];
    float4 g = reinterpret_cast<float4 *>(GY2)[r];
    g.x *= d; g.y *= d; g.z *= d;
    reinterpret_cast<float4 *>(GY2)[r] = g;
    ones[r] = 1.0f;
}

// ---- att_edge_bwd ---------------------------------------------------------------------------------------------------
struct EdgeArgs {
    const int *rowptr, *gcol;
    const float *T, *G;
    long ld;
    const float *s_src, *s_dst;
    float slope;
    const float *alpha_e, *alpha_s;
    float *dz_e;      // [nnz]; holds da of the terms past a row's first 64 between the kernel's two passes
    float *dz_s;      // [R]
    float *ds_dst;    // [R]
    int R;
    int F;
};

// G[i,:] . T[j,:]: NP > 0: the G row in registers (F <= 256 * NP); NP == 0: any width, both rows streamed
template <int NP>
__device__ __forceinline__ float row_dot(const EdgeArgs &a, const float4 (&g)[NP ? NP : 1], const int (&cc)[NP ? NP : 1],
                                         const float *Gi, const float *Tj, int lane) {
    float d = 0.f;
    if constexpr (NP > 0) {
#pragma unroll
        for (int p = 0; p < NP; ++p) d = dot4(g[p], reinterpret_cast<const float4 *>(Tj)[cc[p]], d);
    } else {
        const int F4 = a.F >> 2;
        for (int c = lane; c < F4; c += 64)
            d = dot4(reinterpret_cast<const float4 *>(Gi)[c], reinterpret_cast<const float4 *>(Tj)[c], d);
    }
    return d;
}

template <int NP>
__global__ __launch_bounds__(256) void att_edge_bwd_kernel(EdgeArgs a) {
    constexpr int NR = NP ? NP : 1;
    const int lane = gmc::lane_id();
    const int i = gmc::uniform((int)(blockIdx.x * kWavesPerWg + (threadIdx.x >> 6)));
    if (i >= a.R) return;
    int beg, end;
    row_range(a.rowptr, i, lane, beg, end);
    const int deg = end - beg, nt = deg + 1;
    const float sd = a.s_dst[i];
    const float *Gi = a.G + (long)i * a.ld;
    const int F4 = a.F >> 2;
    float4 g[NR];
    int cc[NR];
#pragma unroll
    for (int p = 0; p < NR; ++p) {   // lanes past the row end carry zeros of G (and re-read the last float4 of T)
        const int c = lane + 64 * p;
        cc[p] = c < F4 ? c : F4 - 1;
        g[p] = NP && c < F4 ? reinterpret_cast<const float4 *>(Gi)[c] : gmc::f4_zero();
    }

    // pass 1: da_t per term (lane t % 64 of its chunk keeps it), dbar = sum_t alpha_t * da_t
    float da0 = 0.f, dbar = 0.f;
#pragma unroll 1
    for (int t0 = 0; t0 < nt; t0 += 64) {
        const int t = t0 + lane;
        const bool have = t < nt;
        const int col = have && t < deg ? a.gcol[beg + t] : i;
        const int cnt = min(64, nt - t0);
        float myda = 0.f;
#pragma unroll 1
        for (int j = 0; j < cnt; j += kDotUnroll) {
            float d[kDotUnroll];
#pragma unroll
            for (int u = 0; u < kDotUnroll; ++u) {
                const long c = __builtin_amdgcn_readlane(col, j + u);
                d[u] = 0.f;
                if (j + u < cnt) d[u] = row_dot<NP>(a, g, cc, Gi, a.T + c * a.ld, lane);   // wave-uniform branch
            }
#pragma unroll
            for (int u = 0; u < kDotUnroll; ++u) {
                if (j + u < cnt) {
                    const float s = gmc::wave_sum(d[u]);
                    if (lane == j + u) myda = s;
                }
            }
        }
        if (have) {
            dbar = fmaf(t < deg ? a.alpha_e[beg + t] : a.alpha_s[i], myda, dbar);
            if (t0 == 0) da0 = myda;
            else if (t < deg) a.dz_e[beg + t] = myda;   // (read back below by this same lane)
            else a.dz_s[i] = myda;
        }
    }
    dbar = gmc::wave_sum(dbar);

    // pass 2: softmax and leaky-relu backward
    float dsd = 0.f;
#pragma unroll 1
    for (int t0 = 0; t0 < nt; t0 += 64) {
        const int t = t0 + lane;
        if (t < nt) {
            const bool self = t >= deg;
            const int col = self ? i : a.gcol[beg + t];
            const float da = t0 == 0 ? da0 : self ? a.dz_s[i] : a.dz_e[beg + t];
            const float alpha = self ? a.alpha_s[i] : a.alpha_e[beg + t];
            const float z = sd + a.s_src[col];
            const float dz = alpha * (da - dbar) * (z > 0.f ? 1.0f : a.slope);
            if (self) a.dz_s[i] = dz;
            else a.dz_e[beg + t] = dz;
            dsd += dz;
        }
    }
    dsd = gmc::wave_sum(dsd);
    if (lane == 0) a.ds_dst[i] = dsd;
}

// ---- att_bwd_t ------------------------------------------------------------------------------------------------------
struct BwdTArgs {
    const int *rowptr, *gcol;
    int nnz;
    const float *G;
    long ld;
    const float *alpha_e, *alpha_s, *dz_e, *dz_s;
    const float *ds_dst;
    float *ds_src;
    const float *a_src, *a_dst;
    float *dT;
    int R;
    int F;
};

template <int NP>
__global__ __launch_bounds__(256) void att_bwd_t_kernel(BwdTArgs a) {
    const int lane = gmc::lane_id();
    const int j = gmc::uniform((int)(blockIdx.x * kWavesPerWg + (threadIdx.x >> 6)));
    if (j >= a.R) return;
    int beg, end;
    row_range(a.rowptr, j, lane, beg, end);
    const int deg = end - beg, nt = deg + 1;
    const float dsd = a.ds_dst[j];
    float dss = 0.f;
    const int F4 = a.F >> 2;
#pragma unroll 1
    for (int cb = 0; cb < F4; cb += 64 * NP) {
        bool on[NP];
        int cc[NP];
        float4 acc[NP];
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const int c = cb + lane + 64 * p;
            on[p] = c < F4;
            cc[p] = on[p] ? c : F4 - 1;
            acc[p] = gmc::f4_zero();
        }
        float part = 0.f;
#pragma unroll 1
        for (int t0 = 0; t0 < nt; t0 += 64) {
            const int t = t0 + lane;
            const bool have = t < nt;
            int row = j;
            float w = 0.f;
            if (have) {
                if (t < deg) {
                    row = a.gcol[beg + t];
                    // the reverse entry: j among the (sorted) columns of row `row`
                    int lo = a.rowptr[row], hi = a.rowptr[row + 1];
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (a.gcol[mid] < j) lo = mid + 1;
                        else hi = mid;
                    }
                    lo = min(lo, a.nnz - 1);   // (a structure that is not symmetric: stay inside the arrays)
                    w = a.alpha_e[lo];
                    if (cb == 0) part += a.dz_e[lo];
                } else {
                    w = a.alpha_s[j];
                    if (cb == 0) part += a.dz_s[j];
                }
            }
            gather_weighted<NP>(a.G, a.ld, row, w, min(64, nt - t0), cc, acc);
        }
        if (cb == 0) {
            dss = gmc::wave_sum(part);
            if (lane == 0) a.ds_src[j] = dss;
        }
#pragma unroll
        for (int p = 0; p < NP; ++p) {
            const float *as = a.a_src + 4 * cc[p], *ad = a.a_dst + 4 * cc[p];   // (not 16-byte aligned in the flat buffer)
            float4 y = acc[p];
            y.x = fmaf(dsd, ad[0], fmaf(dss, as[0], y.x));
            y.y = fmaf(dsd, ad[1], fmaf(dss, as[1], y.y));
            y.z = fmaf(dsd, ad[2], fmaf(dss, as[2], y.z));
            y.w = fmaf(dsd, ad[3], fmaf(dss, as[3], y.w));
            if (on[p]) reinterpret_cast<float4 *>(a.dT + (long)j * a.ld)[cb + lane + 64 * p] = y;
        }
    }
}

// ---- da_src, da_dst -------------------------------------------------------------------------------------------------
struct AvecArgs {
    const float *T;
    long ld;
    const float *ds_src, *ds_dst;
    float *part;   // [tiles][2][F]
    int R;
    int F;
};

__global__ __launch_bounds__(256) void att_avec_part_kernel(AvecArgs a) {
    const int c4 = blockIdx.y * 256 + threadIdx.x;
    const int F4 = a.F >> 2;
    const bool on = c4 < F4;
    const int cl = on ? c4 : F4 - 1;
    const int rbeg = blockIdx.x * kTileRows;
    const int rend = min(rbeg + kTileRows, a.R);
    float4 s = gmc::f4_zero(), d = gmc::f4_zero();
#pragma unroll 4
    for (int r = rbeg; r < rend; ++r) {
        const float4 t = reinterpret_cast<const float4 *>(a.T + (long)r * a.ld)[cl];
        gmc::f4_fma(s, a.ds_src[r], t);
        gmc::f4_fma(d, a.ds_dst[r], t);
    }
    if (on) {
        float4 *out = reinterpret_cast<float4 *>(a.part + (long)blockIdx.x * 2 * a.F);
        out[c4] = s;
        out[F4 + c4] = d;
    }
}

struct AvecFoldArgs {
    const float *part;
    int tiles;
    int F;
    float *da_src, *da_dst;
};

// the tiles dealt over kRedLanes lanes, each ascending, then the lanes added in ascending order (colsum_reduce's order)
__global__ __launch_bounds__(kRedCols * kRedLanes) void att_avec_fold_kernel(AvecFoldArgs a) {
    __shared__ float red[kRedLanes][2][kRedCols];
    const int cl = threadIdx.x & (kRedCols - 1);
    const int tl = threadIdx.x / kRedCols;
    const int f = blockIdx.x * kRedCols + cl;
    float s = 0.f, d = 0.f;
    if (f < a.F) {
#pragma unroll 2
        for (int t = tl; t < a.tiles; t += kRedLanes) {
            const float *p = a.part + (long)t * 2 * a.F + f;
            s += p[0];
            d += p[a.F];
        }
    }
    red[tl][0][cl] = s;
    red[tl][1][cl] = d;
    __syncthreads();
    if (tl < 2 && f < a.F) {
        float t = red[0][tl][cl];
#pragma unroll 8
        for (int i = 1; i < kRedLanes; ++i) t += red[i][tl][cl];
        (tl ? a.da_dst : a.da_src)[f] = t;
    }
}

unsigned row_grid(int R) { return (unsigned)((R + kWavesPerWg - 1) / kWavesPerWg); }

}  // namespace

size_t gmc_att_avec_part_floats(int R, int F) { return (size_t)((R + kTileRows - 1) / kTileRows) * 2 * F; }

int gmc_att_scores_launch(const float *T, long ld, const float *a_src, const float *a_dst, float *s_src, float *s_dst,
                          int R, int F, hipStream_t st) {
    if (R == 0) return GMC_OK;
    ScoreArgs a{T, ld, a_src, a_dst, s_src, s_dst, R, F};
    GmcProbeScope probe(GMC_K_DENSE_MFMA, st);   // (the tag of the stand-alone row products: hw2_rows, hw2_k)
    hipLaunchKernelGGL(att_scores_kernel, dim3(row_grid(R)), dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

int gmc_att_fwd_launch(const gmc_batch *b, const float *T, long ld, const float *s_src, const float *s_dst, float slope,
                       const float *bias, float *alpha_e, float *alpha_s, float *H, int F, hipStream_t st) {
    if (F % 4 || ld % 4 || !gmc_aligned16(T) || !gmc_aligned16(H) || !gmc_aligned16(bias)) return GMC_ERR_ALIGN;
    if (b->R == 0) return GMC_OK;
    FwdArgs a{b->rowptr, b->gcol, T, ld, s_src, s_dst, slope, bias, alpha_e, alpha_s, H, b->R, F};
    GmcProbeScope probe(GMC_K_AGG_FWD, st);
    if (F <= 256) hipLaunchKernelGGL(att_fwd_kernel<1>, dim3(row_grid(b->R)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(att_fwd_kernel<2>, dim3(row_grid(b->R)), dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

int gmc_att_gy2_scale_launch(float *GY2, const float *dinv, float *ones, int R, hipStream_t st) {
    if (R == 0) return GMC_OK;
    GmcProbeScope probe(GMC_K_HIDDEN_BWD, st);
    hipLaunchKernelGGL(att_gy2_scale_kernel, dim3((R + 255) / 256), dim3(256), 0, st, GY2, dinv, ones, R);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

int gmc_att_edge_bwd_launch(const gmc_batch *b, const float *T, const float *G, long ld, const float *s_src,
                            const float *s_dst, float slope, const float *alpha_e, const float *alpha_s, float *dz_e,
                            float *dz_s, float *ds_dst, int F, hipStream_t st) {
    if (F % 4 || ld % 4 || !gmc_aligned16(T) || !gmc_aligned16(G)) return GMC_ERR_ALIGN;
    if (b->R == 0) return GMC_OK;
    EdgeArgs a{b->rowptr, b->gcol, T, G, ld, s_src, s_dst, slope, alpha_e, alpha_s, dz_e, dz_s, ds_dst, b->R, F};
    const dim3 grid(row_grid(b->R)), block(256);
    GmcProbeScope probe(GMC_K_AGG_BWD, st);
    if (F <= 256) hipLaunchKernelGGL(att_edge_bwd_kernel<1>, grid, block, 0, st, a);
    else if (F <= 512) hipLaunchKernelGGL(att_edge_bwd_kernel<2>, grid, block, 0, st, a);
    else if (F <= 1024) hipLaunchKernelGGL(att_edge_bwd_kernel<4>, grid, block, 0, st, a);
    else hipLaunchKernelGGL(att_edge_bwd_kernel<0>, grid, block, 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

int gmc_att_bwd_t_launch(const gmc_batch *b, const float *G, long ld, const float *alpha_e, const float *alpha_s,
                         const float *dz_e, const float *dz_s, const float *ds_dst, float *ds_src, const float *a_src,
                         const float *a_dst, float *dT, int F, hipStream_t st) {
    if (F % 4 || ld % 4 || !gmc_aligned16(G) || !gmc_aligned16(dT)) return GMC_ERR_ALIGN;
    if (b->R == 0) return GMC_OK;
    BwdTArgs a{b->rowptr, b->gcol, b->nnz, G, ld, alpha_e, alpha_s, dz_e, dz_s, ds_dst, ds_src, a_src, a_dst, dT, b->R, F};
    GmcProbeScope probe(GMC_K_AGG_BWD, st);
    if (F <= 256) hipLaunchKernelGGL(att_bwd_t_kernel<1>, dim3(row_grid(b->R)), dim3(256), 0, st, a);
    else hipLaunchKernelGGL(att_bwd_t_kernel<2>, dim3(row_grid(b->R)), dim3(256), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// part must hold gmc_att_avec_part_floats(R, F) floats
int gmc_att_avec_launch(const float *T, long ld, const float *ds_src, const float *ds_dst, float *part, float *da_src,
                        float *da_dst, int R, int F, hipStream_t st) {
    if (F % 4 || ld % 4 || !gmc_aligned16(T) || !gmc_aligned16(part)) return GMC_ERR_ALIGN;
    if (R == 0) return GMC_OK;
    const int tiles = (R + kTileRows - 1) / kTileRows;
    {
        AvecArgs a{T, ld, ds_src, ds_dst, part, R, F};
        GmcProbeScope probe(GMC_K_COLSUM, st);
        hipLaunchKernelGGL(att_avec_part_kernel, dim3(tiles, (F / 4 + 255) / 256), dim3(256), 0, st, a);
        GMC_LAUNCH_CHECK();
    }
    AvecFoldArgs f{part, tiles, F, da_src, da_dst};
    GmcProbeScope probe(GMC_K_COLSUM, st);
    hipLaunchKernelGGL(att_avec_fold_kernel, dim3((F + kRedCols - 1) / kRedCols), dim3(kRedCols * kRedLanes), 0, st, f);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
