// What the one-wave-per-chain searches share (kway_tabu.hip, kway_balance.hip): the LDS layout of a launch, the ordering
// of a wave's own LDS traffic, the 64-lane max of a 64-bit key on the VALU and the order-preserving float <-> uint32 map.
#pragma once
#include "gmc_common.h"

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

}  // namespace gmc
