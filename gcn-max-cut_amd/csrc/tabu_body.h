// What the one-wave-per-chain searches share (kway_tabu.hip, kway_balance.hip): the LDS layout of a launch, the host
// side of their entry points (fits / shape, the argument checks, the launch), the ordering of a wave's own LDS traffic,
// the 64-lane max of a 64-bit key on the VALU, the order-preserving float <-> uint32 map and the steps of a chain that
// both kernels take in the same words.
#pragma once
#include "gmc_common.h"
#include "mix64.h"

#define GMC_TABU_LDS_BYTES (160 * 1024)   // the LDS of a CU
#define GMC_TABU_LDS_STATIC 512           // allowance for red and the pick's word (16 B as built)

namespace gmc {

// LDS of a launch: `slots` chains of chain_bytes each, then the staged copy.  Depends on n_max, nnz_max, vals and K.
struct TabuLayout {
    int fits;      // one chain's state fits a CU's LDS (and n_max is in 1..GMC_MAX_GRAPH_NODES)
    int slots;     // chains per workgroup: 4, 2 or 1
    int staged;    // the launch has room for the copy of the graph's CSR
    int n_pad, chain_bytes, off_starts, off_vals, off_ids, bytes;
};
inline TabuLayout tabu_layout(const gmc_batch *b, int K) {
    TabuLayout L{};
    const long cap = GMC_TABU_LDS_BYTES - GMC_TABU_LDS_STATIC;
    const long n_max = b->n_max > 0 ? b->n_max : 0;
    const long n_pad = (n_max + 15) & ~15L;
    const long chain = n_pad * (4 * K + 6);
    L.fits = n_max >= 1 && n_max <= GMC_MAX_GRAPH_NODES && chain <= cap;
    if (!L.fits) return L;
    const long nnz = b->nnz_max > 0 ? b->nnz_max : 0;
    const long starts = ((n_max + 1) * 4 + 15) & ~15L;
    const long vals = b->vals ? (nnz * 4 + 15) & ~15L : 0;
    const long ids = (nnz * 2 + 15) & ~15L;
    const long csr = starts + vals + ids;
    L.staged = nnz > 0 && chain + csr <= cap;
    const long room = cap - (L.staged ? csr : 0);
    L.slots = 4 * chain <= room ? 4 : 2 * chain <= room ? 2 : 1;
    L.n_pad = (int)n_pad;
    L.chain_bytes = (int)chain;
    L.off_starts = L.slots * L.chain_bytes;
    L.off_vals = L.off_starts + (int)starts;
    L.off_ids = L.off_vals + (int)vals;
    L.bytes = L.staged ? L.off_ids + (int)ids : L.off_starts;
    return L;
}

// gmc_kway_{tabu,balance}_fits, and with `shape` gmc_kway_{tabu,balance}_shape
inline int chain_query(const gmc_batch *batch, int K, bool shape) {
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    const TabuLayout L = tabu_layout(batch, K);
    if (!shape) return L.fits;
    return L.fits ? L.slots | (L.staged << 4) : GMC_ERR_GRAPH_SIZE;
}

// What the two entry points check after their own NULL test of the pointers each requires, in this order: the abi
// word, the batch's arrays, K, the shapes, the graph size.  GMC_OK: `first` (the first movable local id: K with
// terminals, 0 without) and L are the launch's; the caller returns GMC_OK without a launch for a batch of no graphs.
inline int chain_checks(const gmc_batch *batch, int K, int terminals, int cands, int iterations, int tenure_base,
                        int tenure_span, int tenure_div, int &first, TabuLayout &L) {
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || !batch->lcol) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (cands < 1 || iterations < 0 || tenure_base < 0 || tenure_span < 0 || tenure_div < 0 || batch->B < 0 ||
        (terminals != 0 && terminals != 1))
        return GMC_ERR_SHAPE;
    first = terminals ? K : 0;
    L = tabu_layout(batch, K);
    if (batch->B > 0 && (batch->n_max < (first > 1 ? first : 1) || !L.fits)) return GMC_ERR_GRAPH_SIZE;
    return GMC_OK;
}

// the chain launch of either search: Args holds the batch b, cands and slots
template <class Args>
int chain_launch(void (*kernel)(Args), const Args &a, int lds_bytes, hipStream_t st) {
    if (lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(kernel),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return (int)e;
    }
    GmcProbeScope probe(GMC_K_ANNEAL, st);
    hipLaunchKernelGGL(kernel, dim3((a.cands + a.slots - 1) / a.slots, a.b.B), dim3(256), (size_t)lds_bytes, st,
                       a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// orders the wave's own LDS traffic: what its lanes wrote before is what they read after
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// max(key[lane], key[lane ^ O]) of a 64-bit key on the VALU: the exchanges of gmc::xor_add on both halves
template <int O>
__device__ __forceinline__ unsigned long long xor_max(unsigned long long key) {
    using u64 = unsigned long long;
    const unsigned hi = (unsigned)(key >> 32), lo = (unsigned)key;
    u64 other;
    if constexpr (O == 32) {
        const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
        const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
        key = ((u64)rh[0] << 32) | rl[0];   // one of the two is the lane's own, the other its partner's
        other = ((u64)rh[1] << 32) | rl[1];
    } else if constexpr (O == 16) {
        const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
        const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
        key = ((u64)rh[0] << 32) | rl[0];
        other = ((u64)rh[1] << 32) | rl[1];
    } else if constexpr (O == 4) {
        unsigned th = __builtin_amdgcn_update_dpp(hi, hi, 0x104 /* row_shl:4 */, 0xf, 0x5, false);
        th = __builtin_amdgcn_update_dpp(th, hi, 0x114 /* row_shr:4 */, 0xf, 0xa, false);
        unsigned tl = __builtin_amdgcn_update_dpp(lo, lo, 0x104, 0xf, 0x5, false);
        tl = __builtin_amdgcn_update_dpp(tl, lo, 0x114, 0xf, 0xa, false);
        other = ((u64)th << 32) | tl;
    } else {
        static_assert(O == 8 || O == 2 || O == 1, "lane distance");
        constexpr int ctrl = O == 8 ? 0x128 /* row_ror:8 */ : O == 2 ? 0x4e /* quad_perm:[2,3,0,1] */ : 0xb1 /* [1,0,3,2] */;
        const unsigned th = __builtin_amdgcn_update_dpp(0u, hi, ctrl, 0xf, 0xf, false);
        const unsigned tl = __builtin_amdgcn_update_dpp(0u, lo, ctrl, 0xf, 0xf, false);
        other = ((u64)th << 32) | tl;
    }
    return other > key ? other : key;
}
__device__ __forceinline__ unsigned long long wave_max(unsigned long long key) {
    key = xor_max<32>(key);
    key = xor_max<16>(key);
    key = xor_max<8>(key);
    key = xor_max<4>(key);
    key = xor_max<2>(key);
    return xor_max<1>(key);
}

// float -> uint32 with the order of the floats (no NaN); -0.0 does not arise: a sum that starts at +0.0 and only adds
// and subtracts in round-to-nearest never becomes -0.0, nor does a difference of two such sums
__device__ __forceinline__ unsigned ordered_bits(float f) {
    const unsigned u = __float_as_uint(f);
    return u ^ ((u >> 31) ? 0xffffffffu : 0x80000000u);
}
__device__ __forceinline__ float ordered_float(unsigned o) {
    return __uint_as_float(o ^ ((o >> 31) ? 0x80000000u : 0xffffffffu));
}

// node v leaves class c for class k: one lane per edge of its row updates the neighbours' rows of W
template <int K, class G>
__device__ __forceinline__ void apply_move(const G &g, float *W, unsigned char *st, int v, int c, int k, int lane) {
    const int e1 = g.rp[v + 1];
    for (int e = (int)g.rp[v] + lane; e < e1; e += GMC_WAVE) {
        const int u = g.col[e];
        if (u == v) continue;
        const float wt = g.vals ? g.vals[e] : 1.0f;
        W[u * K + c] -= wt;
        W[u * K + k] += wt;
    }
    if (lane == 0) st[v] = (unsigned char)k;
}

// until[v] of a node moved at iteration `it` (it < 2^31: saturated is "never again")
__device__ __forceinline__ unsigned ban_until(int it, unsigned tenure_base, unsigned tenure_draw) {
    const u64 u = (u64)(unsigned)it + 1ULL + (u64)tenure_base + (u64)tenure_draw;
    return u > 0xffffffffULL ? 0xffffffffu : (unsigned)u;
}

}  // namespace gmc
