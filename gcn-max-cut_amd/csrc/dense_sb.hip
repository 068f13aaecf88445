// Discrete simulated bifurcation for dense two-class instances (an extension: the reference samples and stops):
// gmc_dense_sb_f32 and gmc_dense_sb_init_f32, stated to the operation in include/gcnmaxcut_bifurcation.h.  Where
// dense_anneal.hip walks a chain's nodes one after the other, a time step here moves every node of every chain at once:
//   F = W . sign(X)      [n, n] . [n, cands]   on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32, a k-ordered fmaf
//                                              chain), rows = nodes, columns = candidates
//   y -= dt * (pump * x + c0 * (F + g));  x += dt * y;  walls at +-1      the product's epilogue
//
// The tile loop is gemm_mfma.hip's: both LDS tiles k-major, the next k tile fetched into registers before the MFMAs of the
// current one and stored to the other buffer after them, one barrier per k tile, edges zero-filled on the way in, k
// ascending inside one workgroup.  What differs:
//   - the A operand is W itself ([v][u], k contiguous: a transposing store into LDS), of any ld and alignment - rows that
//     are not 16-byte aligned are read element by element - and its diagonal is zeroed on the way into LDS;
//   - the B operand is a SIGN: one byte per (node, candidate) in a plane [R][cs] of the workspace, cs = cands up to 16,
//     read as 4-byte words and converted to float on the way into LDS (a quarter of a float plane's traffic);
//   - the tile is chosen per call (sb_pick_tile): 64 x 64 (waves 2 x 2, four accumulators each), 32 x 64 (waves 1 x 4,
//     two accumulators each: twice the workgroups) or 64 x 16 (waves 4 x 1, one accumulator each: four times the
//     workgroups again, the fastest while the grid is small - a single wave's dependent MFMAs are hidden by the other
//     workgroups of its CU);
//   - the epilogue is the rule's steps 3 - 5 on the thread's own accumulator entries: x and y in place, the new sign into
//     the OTHER plane, so kernel boundaries are the only synchronisation.
// D of a 16 x 16 MFMA tile: column = lane & 15 (a candidate), row = 4 * (lane >> 4) + j (a node): the 16 lanes of a
// register touch 16 consecutive candidates of one node, which is why x, y and the signs are laid out [R][cands].
#include "gmc_common.h"
#include "mix64.h"
#include "../../include/gcnmaxcut_bifurcation.h"

namespace {

using gmc::mix64;
using gmc::u64;
using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int SB_TK = 16;
// floats per k row of an LDS tile of T columns: the four k rows a wave reads start 16 banks apart
constexpr int sb_ld(int T) { return (T % 64 == 16 || T % 64 == 48) ? T : T + 16; }

struct SbArgs {
    int B, n, cands, cs, mt, nt, wvec;
    long ld, R;
    const float *W;             // [B][n][ld]
    const float *node_cost;     // [R][2] or NULL
    float *x, *y;               // [R][cands]
    const signed char *sin;     // [R][cs]: the signs of step t
    signed char *sout;          // [R][cs]: those of step t + 1
    signed char *assign;        // [cands][R], the last step only (else NULL)
    const float *pump;          // this step's entry
    float c0, dt;
};

__device__ __forceinline__ signed char sb_sign(float x) { return x > 0.f ? 1 : (x < 0.f ? -1 : 0); }

template <int TM, int TN, int WR, int WC>
__global__ __launch_bounds__(64 * WR * WC) void sb_step_kernel(SbArgs a) {
#pragma clang fp contract(off)
    constexpr int NT = 64 * WR * WC, LDA = sb_ld(TM), LDB = sb_ld(TN);
    constexpr int MI = TM / (16 * WR), NI = TN / (16 * WC);
    constexpr int UA = TM * 4, UB = TN * 4;            // float4 units of a W tile, 4-byte words of a sign tile
    constexpr int FA = (UA + NT - 1) / NT, FB = (UB + NT - 1) / NT;
    static_assert(MI >= 1 && NI >= 1 && TM % (16 * WR) == 0 && TN % (16 * WC) == 0, "tile");
    __shared__ __attribute__((aligned(16))) float As[2][SB_TK * LDA];
    __shared__ __attribute__((aligned(16))) float Bs[2][SB_TK * LDB];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int per = a.mt * a.nt;
    const int prob = blockIdx.x / per, rem = blockIdx.x - prob * per;
    const int m0 = (rem / a.nt) * TM, n0 = (rem % a.nt) * TN;
    const int wm = (wave / WC) * (16 * MI), wn = (wave % WC) * (16 * NI);
    const int li = lane & 15, lq = lane >> 4;
    const int n = a.n;
    const long r0 = (long)prob * n;
    const float *W = a.W + r0 * a.ld;
    const signed char *sin = a.sin + r0 * a.cs;

    float4 ra[FA];
    int rb[FB];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int q = 0; q < FA; ++q) {
            const int idx = t + q * NT;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            const int row = m0 + (idx >> 2), k = k0 + (idx & 3) * 4;
            if ((UA % NT == 0 || idx < UA) && row < n && k < n) {
                const float *p = W + (long)row * a.ld + k;
                if (a.wvec && k + 3 < n) {
                    v = *reinterpret_cast<const float4 *>(p);
                } else {   // a partial group, or rows that are not 16-byte aligned: never past column n - 1
                    v.x = p[0];
                    if (k + 1 < n) v.y = p[1];
                    if (k + 2 < n) v.z = p[2];
                    if (k + 3 < n) v.w = p[3];
                }
                const int d = row - k;   // the diagonal is taken as +0.0f, whatever it holds
                if (d == 0) v.x = 0.f;
                if (d == 1) v.y = 0.f;
                if (d == 2) v.z = 0.f;
                if (d == 3) v.w = 0.f;
            }
            ra[q] = v;
        }
#pragma unroll
        for (int q = 0; q < FB; ++q) {
            const int idx = t + q * NT;
            const int u = k0 + idx / (TN / 4), c = n0 + (idx % (TN / 4)) * 4;
            int w = 0;
            if ((UB % NT == 0 || idx < UB) && u < n && c < a.cs)
                w = *reinterpret_cast<const int *>(sin + (long)u * a.cs + c);   // cs % 16 == 0: aligned, written whole
            rb[q] = w;
        }
    };
    auto stage = [&](int buf) {
#pragma unroll
        for (int q = 0; q < FA; ++q) {
            const int idx = t + q * NT;
            if (UA % NT != 0 && idx >= UA) continue;
            float *S = As[buf] + (idx & 3) * 4 * LDA + (idx >> 2);   // four k of one row: a transposing store
            S[0] = ra[q].x;
            S[LDA] = ra[q].y;
            S[2 * LDA] = ra[q].z;
            S[3 * LDA] = ra[q].w;
        }
#pragma unroll
        for (int q = 0; q < FB; ++q) {
            const int idx = t + q * NT;
            if (UB % NT != 0 && idx >= UB) continue;
            const int w = rb[q];
            const float4 v = make_float4((float)(signed char)(w & 0xff), (float)(signed char)((w >> 8) & 0xff),
                                         (float)(signed char)((w >> 16) & 0xff), (float)(signed char)((w >> 24) & 0xff));
            *reinterpret_cast<float4 *>(Bs[buf] + (idx / (TN / 4)) * LDB + (idx % (TN / 4)) * 4) = v;
        }
    };

    f32x4 acc[MI][NI];
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NI; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    fetch(0);
    stage(0);
    __syncthreads();
    const int tiles = (n + SB_TK - 1) / SB_TK;
    for (int it = 0; it < tiles; ++it) {
        const int cur = it & 1;
        const bool more = it + 1 < tiles;
        if (more) fetch((it + 1) * SB_TK);
        const float *as = As[cur] + lq * LDA + wm + li;
        const float *bs = Bs[cur] + lq * LDB + wn + li;
        float fa[MI][SB_TK / 4], fb[NI][SB_TK / 4];   // every operand of the tile is requested before the first MFMA
#pragma unroll
        for (int s = 0; s < SB_TK / 4; ++s) {
#pragma unroll
            for (int i = 0; i < MI; ++i) fa[i][s] = as[4 * s * LDA + 16 * i];
#pragma unroll
            for (int j = 0; j < NI; ++j) fb[j][s] = bs[4 * s * LDB + 16 * j];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < SB_TK / 4; ++s)
#pragma unroll
            for (int i = 0; i < MI; ++i)
#pragma unroll
                for (int j = 0; j < NI; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(fa[i][s], fb[j][s], acc[i][j], 0, 0, 0);
        if (more) stage(cur ^ 1);   // the other buffer: last read before the barrier that ended the previous iteration
        __syncthreads();
    }

    // steps 3 - 5 on the thread's own entries
    const float pump = *a.pump, c0 = a.c0, dt = a.dt;
    signed char *sout = a.sout + r0 * a.cs;
#pragma unroll
    for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j4 = 0; j4 < 4; ++j4) {
            const int v = m0 + wm + 16 * i + 4 * lq + j4;
            if (v >= n) continue;
            float g = 0.f;
            if (a.node_cost) g = a.node_cost[2 * (r0 + v)] - a.node_cost[2 * (r0 + v) + 1];
#pragma unroll
            for (int j = 0; j < NI; ++j) {
                const int cand = n0 + wn + 16 * j + li;
                if (cand >= a.cs) continue;
                signed char s = 0;
                if (cand < a.cands) {
                    float f = acc[i][j][j4];
                    if (a.node_cost) f = f + g;
                    const long e = (r0 + v) * a.cands + cand;
                    float xv = a.x[e], yv = a.y[e];
                    const float p = pump * xv;
                    const float q = c0 * f;
                    const float r = p + q;
                    const float m = dt * r;
                    yv = yv - m;
                    const float m2 = dt * yv;
                    xv = xv + m2;
                    if (xv > 1.f) {
                        xv = 1.f;
                        yv = 0.f;
                    } else if (xv < -1.f) {
                        xv = -1.f;
                        yv = 0.f;
                    }
                    a.x[e] = xv;
                    a.y[e] = yv;
                    s = sb_sign(xv);
                    if (a.assign) a.assign[(long)cand * a.R + r0 + v] = xv < 0.f ? 1 : 0;
                }
                sout[(long)v * a.cs + cand] = s;   // the columns cands .. cs - 1 hold 0: the next step reads whole words
            }
        }
}

// the signs of the given x into a plane, every byte of it; with `assign` the class bytes as well (steps == 0)
__global__ __launch_bounds__(256) void sb_signs_kernel(long R, int cands, int cs, const float *x, signed char *plane,
                                                       signed char *assign) {
    const long total = R * cs;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cs;
        const int c = (int)(i - r * cs);
        signed char s = 0;
        if (c < cands) {
            const float xv = x[r * cands + c];
            s = sb_sign(xv);
            if (assign) assign[(long)c * R + r] = xv < 0.f ? 1 : 0;
        }
        plane[i] = s;
    }
}

__global__ __launch_bounds__(256) void sb_init_kernel(long R, int n, int cands, u64 seed, float amplitude, float *x,
                                                      float *y) {
#pragma clang fp contract(off)
    const long total = R * cands;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const long r = i / cands;
        const unsigned cand = (unsigned)(i - r * cands), v = (unsigned)(r % n);
        const u64 h = mix64(seed + GMC_GOLD * ((((u64)cand << 32) | (u64)v) + 1ULL));
        const float t = (float)(int)(h >> 40) - 8388608.0f;
        const float u = t * 1.1920928955078125e-07f;   // 2^-23, exact
        x[i] = 0.f;
        y[i] = amplitude * u;
    }
}

bool sb_sizes_ok(int B, int n, int cands) { return B >= 0 && n >= 2 && n <= GMC_MAX_GRAPH_NODES && cands >= 1; }
long sb_cs(int cands) { return ((long)cands + 15) & ~15L; }
unsigned sb_flat_grid(long total) {
    const long blocks = (total + 255) / 256;
    return (unsigned)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks));
}

// 1: 64 x 64, 2: 32 x 64, 3: 64 x 16.  Fitted to the A/B of DESIGN.md section 41 (24 shapes, every tile forced): while
// the narrow tile's grid stays within 512 workgroups (two per CU) it is the fastest - one problem of n <= 2048 with 200
// candidates is 16 to 64 workgroups of 64 x 64 on 256 CUs - and it always is for candidates that fit one MFMA column
// tile; beyond that 64 x 64 once it gives more than 1024 workgroups and 32 x 64 (twice the workgroups) below.
int g_sb_tile = 0;   // a measurement hook (gmc_debug_set_sb_tile), 0 = choose
int sb_pick_tile(int B, int n, int cands) {
    if (g_sb_tile >= 1 && g_sb_tile <= 3) return g_sb_tile;
    const long rows = (long)B * ((n + 63) / 64);
    if (cands <= 16 || rows * ((cands + 15) / 16) <= 512) return 3;
    return rows * ((cands + 63) / 64) > 1024 ? 1 : 2;
}

template <int TM, int TN, int WR, int WC>
int sb_launch_step(SbArgs a, hipStream_t st) {
    a.mt = (a.n + TM - 1) / TM;
    a.nt = (a.cands + TN - 1) / TN;
    const long grid = (long)a.B * a.mt * a.nt;
    hipLaunchKernelGGL((sb_step_kernel<TM, TN, WR, WC>), dim3((unsigned)grid), dim3(64 * WR * WC), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

long sb_tiles(int tile, int B, int n, int cands) {
    const int tm = tile == 2 ? 32 : 64, tn = tile == 3 ? 16 : 64;
    return (long)B * ((n + tm - 1) / tm) * ((cands + tn - 1) / tn);
}

}  // namespace

// measurement hook, not part of the header: force the step kernel's tile (0 = choose per call); returns the old value
extern "C" int gmc_debug_set_sb_tile(int tile) {
    const int old = g_sb_tile;
    g_sb_tile = tile;
    return old;
}

extern "C" size_t gmc_dense_sb_state_bytes(int32_t B, int32_t n, int32_t cands) {
    return sb_sizes_ok(B, n, cands) ? (size_t)B * (size_t)n * (size_t)cands * sizeof(float) : 0;
}

extern "C" size_t gmc_dense_sb_workspace_bytes(int32_t B, int32_t n, int32_t cands) {
    return sb_sizes_ok(B, n, cands) ? 2 * (size_t)B * (size_t)n * (size_t)sb_cs(cands) + 16 : 0;
}

extern "C" int gmc_dense_sb_init_f32(int32_t B, int32_t n, int32_t cands, uint64_t seed, float amplitude, float *x,
                                     float *y, gmc_stream_t stream) {
    if (!x || !y) return GMC_ERR_NULL;
    if (B < 0 || cands < 1) return GMC_ERR_SHAPE;
    if (n < 2 || n > GMC_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (!(amplitude - amplitude == 0.f)) return GMC_ERR_SHAPE;
    if (B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long R = (long)B * n;
    hipLaunchKernelGGL(sb_init_kernel, dim3(sb_flat_grid(R * cands)), dim3(256), 0, st, R, n, cands, (u64)seed, amplitude,
                       x, y);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" int gmc_dense_sb_f32(int32_t B, int32_t n, const float *W, int64_t ld, const float *node_cost, int32_t cands,
                                float *x, float *y, const float *pump, int32_t steps, float c0, float dt, void *workspace,
                                size_t workspace_bytes, int8_t *assign, gmc_stream_t stream) {
    if (!W || !x || !y || !workspace || !assign) return GMC_ERR_NULL;
    if (B < 0 || cands < 1 || steps < 0) return GMC_ERR_SHAPE;
    if (steps > 0 && !pump) return GMC_ERR_NULL;
    if (n < 2 || n > GMC_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (ld < n) return GMC_ERR_SHAPE;
    if (workspace_bytes < gmc_dense_sb_workspace_bytes(B, n, cands)) return GMC_ERR_WORKSPACE;
    if (!(c0 > 0.f) || !(dt > 0.f) || !(c0 - c0 == 0.f) || !(dt - dt == 0.f)) return GMC_ERR_SHAPE;
    const int tile = sb_pick_tile(B, n, cands);
    if (sb_tiles(tile, B, n, cands) > 0x7fffffffL) return GMC_ERR_UNSUPPORTED;
    if (B == 0) return GMC_OK;
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long R = (long)B * n, cs = sb_cs(cands);
    // the planes start at the first 16-byte boundary of the workspace (the formula's 16 bytes pay for it)
    signed char *plane0 =
        reinterpret_cast<signed char *>((reinterpret_cast<uintptr_t>(workspace) + 15u) & ~(uintptr_t)15u);
    signed char *plane1 = plane0 + R * cs;
    signed char *out = reinterpret_cast<signed char *>(assign);
    hipLaunchKernelGGL(sb_signs_kernel, dim3(sb_flat_grid(R * cs)), dim3(256), 0, st, R, cands, (int)cs, x, plane0,
                       steps == 0 ? out : nullptr);
    GMC_LAUNCH_CHECK();
    SbArgs a{};
    a.B = B, a.n = n, a.cands = cands, a.cs = (int)cs, a.ld = (long)ld, a.R = R;
    a.wvec = gmc_aligned16(W) && ld % 4 == 0;
    a.W = W, a.node_cost = node_cost, a.x = x, a.y = y, a.c0 = c0, a.dt = dt;
    for (int s = 0; s < steps; ++s) {
        a.sin = s & 1 ? plane1 : plane0;
        a.sout = s & 1 ? plane0 : plane1;
        a.assign = s + 1 == steps ? out : nullptr;
        a.pump = pump + s;
        int rc;
        if (tile == 1)
            rc = sb_launch_step<64, 64, 2, 2>(a, st);
        else if (tile == 2)
            rc = sb_launch_step<32, 64, 1, 4>(a, st);
        else
            rc = sb_launch_step<64, 16, 4, 1>(a, st);
        if (rc != GMC_OK) return rc;
    }
    return GMC_OK;
}
