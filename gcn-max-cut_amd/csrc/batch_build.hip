// Building a batch on the device from directed entries (src, dst[, w]) in block-diagonal numbering: the device form of
// what graph.py's from_networkx + BatchArrays + gmc_ell_arrange_host do on the host, byte for byte.
//
// CSR stage (gmc_batch_build_csr), every step one launch, kernel boundaries the only synchronisation:
//   init      zero the degree counters, the list counters and the report
//   count     per entry: range check, graph of src, dst inside the same graph; integer atomicAdd on deg[src]
//   scan x3   rowptr = exclusive scan of deg (block sums, scan of the sums, add); the add launch also writes dinv and
//             files every row by length into one of three work lists (9..64, 65..4096, longer)
//   scatter   per entry (same check): position rowptr[src] + a cursor taken with an integer atomic - the order inside a
//             row is arbitrary here ...
//   sort x4   ... and the segmented sort restores the one order np.lexsort((cols, rows)) gives: rows of up to 8 entries by
//             8 lanes, up to 64 by a wave (both by rank, in registers), up to 4096 by a workgroup in LDS (bitonic network),
//             longer ones by the same network on global memory, one workgroup per row - SLOW (a star of 2^20 - 1 leaves
//             takes 210 passes over its 8 MB) and rare.  Keys are (column, weight bits): equal keys are equal bytes, so
//             two builds of the same entries in any input order give the same arrays.
//   validate  per sorted entry: duplicates, a missing or differently weighted reverse entry (binary search in the row of
//             dst), weights other than 1; per row: zero degree and the statistics BatchArrays.choose_width needs; per
//             graph (the grid's last B workgroups): overflow blocks for both widths and the graph's entries.
// Nothing is summed in floating point.  An entry whose ids are out of range or lie in two graphs is counted in the report
// and skipped: src[e] / dst[e] become an index only behind that check, in the same kernel.
//
// Table stage (gmc_batch_build_table): ovf_ptr (the same three-launch scan over the rows' block counts), the overflow
// lists, and the neighbour table in gmc_ell_arrange_host's slot order: one thread per group of four rows (kQuad) runs that
// routine's greedy pass and hill-climb with the quad's neighbours and slots in LDS ([entry][thread] columns) and its
// counters packed in registers.
#include "gmc_common.h"

#include <algorithm>

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;
constexpr int kScanBlock = kThreads * 4;   // rows of one scan workgroup
constexpr int kGroupMax = 8;               // entries a group of 8 lanes sorts
constexpr int kWaveMax = 64;               // entries a wave sorts
constexpr int kWgMax = 4096;               // entries a workgroup sorts in LDS (32 KiB of keys)
constexpr int kListGrid = 512;             // workgroups of the list-walking sort launches
constexpr int kGlobalThreads = 1024;
constexpr int kQuadThreads = 64;           // quads of one arrange workgroup

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
static int scan_blocks(long n) { return (int)((n + kScanBlock - 1) / kScanBlock); }

struct Ws {
    int32_t *deg;        // [R]   degree counters, then the scatter's countdown cursors
    int32_t *sums;       // [scan_blocks(R + 1)]
    int32_t *wave_rows;  // [R]   rows of 9..64 entries
    int32_t *wg_rows;    // [R]   rows of 65..4096
    int32_t *glob_rows;  // [R]   longer rows
    int32_t *counts;     // [4]   lengths of the three lists
    size_t bytes;
};

Ws carve(void *base, long R) {
    Ws w{};
    const uintptr_t p = reinterpret_cast<uintptr_t>(base);   // (nullptr: the size query, nothing is dereferenced)
    size_t o = 0;
    auto take = [&](size_t n) { int32_t *q = reinterpret_cast<int32_t *>(p + o); o += up16(n * sizeof(int32_t)); return q; };
    w.deg = take((size_t)R);
    w.sums = take((size_t)scan_blocks(R + 1) + 1);
    w.wave_rows = take((size_t)R);
    w.wg_rows = take((size_t)R);
    w.glob_rows = take((size_t)R);
    w.counts = take(4);
    w.bytes = o;
    return w;
}

// ---- small device helpers -------------------------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum_i(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// the graph whose rows hold r: the largest g in 0..B-1 with goff[g] <= r (reads goff[0..B-1] only)
__device__ __forceinline__ int graph_of(const int32_t *goff, int B, int r) {
    int lo = 0, hi = B - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (goff[mid] <= r) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// 0: a usable entry, 1: an id outside 0..R-1, 2: endpoints in two graphs
__device__ __forceinline__ int entry_state(const int32_t *goff, int B, int R, int s, int d) {
    if ((unsigned)s >= (unsigned)R || (unsigned)d >= (unsigned)R) return 1;
    const int g = graph_of(goff, B, s);
    const int lo = goff[g], hi = goff[g + 1];
    return (s >= lo && s < hi && d >= lo && d < hi) ? 0 : 2;
}

__device__ __forceinline__ u64 make_key(int col, float w) { return ((u64)(unsigned)col << 32) | (u64)__float_as_uint(w); }

// ---- CSR stage -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) bb_init_kernel(int32_t *deg, int R, int32_t *counts, int32_t *report) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i < R) deg[i] = 0;
    if (i < 4) counts[i] = 0;
    if (i < GMC_BB_REPORT_WORDS) report[i] = 0;
}

__global__ void __launch_bounds__(kThreads) bb_count_kernel(const int32_t *goff, int B, int R, long E, const int32_t *src,
                                                            const int32_t *dst, int32_t *deg, int32_t *report) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    const int s = src[e], d = dst[e];
    const int state = entry_state(goff, B, R, s, d);
    if (state == 0) atomicAdd(&deg[s], 1);
    else atomicAdd(&report[state == 1 ? GMC_BB_OUT_OF_RANGE : GMC_BB_CROSS_GRAPH], 1);
}

// the scanned value of element i of n = R + 1: MODE 0 the row's degree, MODE 1 its overflow blocks at width W
template <int MODE>
__device__ __forceinline__ int scan_value(const int32_t *in, long i, long R, int W) {
    if (i >= R) return 0;
    if (MODE == 0) return in[i];
    return (max(in[i + 1] - in[i] - W, 0) + 7) >> 3;
}

__device__ __forceinline__ int block_sum(int v, int *lds) {   // every thread gets the workgroup's sum
    v = wave_sum_i(v);
    if (gmc::lane_id() == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    int t = 0;
    for (unsigned w = 0; w < blockDim.x >> 6; ++w) t += lds[w];
    __syncthreads();
    return t;
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) bb_scan_sums_kernel(const int32_t *in, long R, int W, int32_t *sums) {
    __shared__ int lds[kThreads / 64];
    const long i0 = (long)blockIdx.x * kScanBlock + threadIdx.x * 4;
    int v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v += scan_value<MODE>(in, i0 + k, R, W);
    v = block_sum(v, lds);
    if (threadIdx.x == 0) sums[blockIdx.x] = v;
}

// one workgroup: sums[0..n) -> its exclusive prefix, 256 at a time with a carry
__global__ void __launch_bounds__(kThreads) bb_scan_top_kernel(int32_t *sums, int n) {
    __shared__ int lds[kThreads];
    int carry = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + threadIdx.x;
        const int own = i < n ? sums[i] : 0;
        lds[threadIdx.x] = own;
        __syncthreads();
        for (int o = 1; o < kThreads; o <<= 1) {
            const int add = (int)threadIdx.x >= o ? lds[threadIdx.x - o] : 0;
            __syncthreads();
            lds[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n) sums[i] = carry + lds[threadIdx.x] - own;
        carry += lds[kThreads - 1];
        __syncthreads();
    }
}

template <int MODE>
__global__ void __launch_bounds__(kThreads) bb_scan_add_kernel(const int32_t *in, long R, int W, const int32_t *sums,
                                                               int32_t *out, float *dinv, int32_t *wave_rows,
                                                               int32_t *wg_rows, int32_t *glob_rows, int32_t *counts) {
    __shared__ int lds[kThreads];
    const long i0 = (long)blockIdx.x * kScanBlock + threadIdx.x * 4;
    int v[4], own = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = scan_value<MODE>(in, i0 + k, R, W); own += v[k]; }
    lds[threadIdx.x] = own;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
        const int add = (int)threadIdx.x >= o ? lds[threadIdx.x - o] : 0;
        __syncthreads();
        lds[threadIdx.x] += add;
        __syncthreads();
    }
    int run = sums[blockIdx.x] + lds[threadIdx.x] - own;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const long i = i0 + k;
        if (i <= R) out[i] = run;
        run += v[k];
        if (MODE == 0 && i < R) {
            // numpy's 1 / sqrt(max(deg, 1)) in float32, both operations correctly rounded: plain sqrtf and / are, under
            // hipcc's default -fhip-fp32-correctly-rounded-divide-sqrt (v_sqrt_f32 + the fma correction, v_div_scale /
            // v_div_fmas / v_div_fixup); __fsqrt_rn is NOT - without OCML_BASIC_ROUNDED_OPERATIONS it is the native sqrt
            dinv[i] = 1.0f / sqrtf(fmaxf((float)v[k], 1.0f));
            if (v[k] > kWgMax) glob_rows[atomicAdd(&counts[2], 1)] = (int)i;
            else if (v[k] > kWaveMax) wg_rows[atomicAdd(&counts[1], 1)] = (int)i;
            else if (v[k] > kGroupMax) wave_rows[atomicAdd(&counts[0], 1)] = (int)i;
        }
    }
}

template <bool HAS_W>
__global__ void __launch_bounds__(kThreads) bb_scatter_kernel(const int32_t *goff, int B, int R, long E, const int32_t *src,
                                                              const int32_t *dst, const float *w, const int32_t *rowptr,
                                                              int32_t *cursor, int32_t *gcol, float *vals) {
    const long e = (long)blockIdx.x * kThreads + threadIdx.x;
    if (e >= E) return;
    const int s = src[e], d = dst[e];
    if (entry_state(goff, B, R, s, d) != 0) return;
    // the count launch gave row s exactly as many places as entries pass this same check
    const int pos = rowptr[s] + atomicSub(&cursor[s], 1) - 1;
    gcol[pos] = d;
    if (HAS_W) vals[pos] = w[e];
}

// rows of up to L entries, L lanes per row, sorted by rank in registers.  L = 8: row = the lane group's index (longer rows
// are left alone); L = 64: the rows of a list.
template <int L, bool HAS_W>
__device__ __forceinline__ void rank_sort_row(int r, int sl, const int32_t *goff, int B, const int32_t *rowptr,
                                              int32_t *gcol, int32_t *lcol, float *vals) {
    const int beg = r >= 0 ? rowptr[r] : 0;
    const int deg = r >= 0 ? rowptr[r + 1] - beg : 0;
    const bool mine = deg <= L && sl < deg;
    u64 key = ~(u64)0;
    if (mine) key = make_key(gcol[beg + sl], HAS_W ? vals[beg + sl] : 0.0f);
    int rank = 0;
#pragma unroll 8
    for (int j = 0; j < L; ++j) {
        const u64 other = __shfl(key, j, L);
        rank += (other < key || (other == key && j < sl)) ? 1 : 0;
    }
    if (mine) {
        const int col = (int)(key >> 32);
        gcol[beg + rank] = col;
        lcol[beg + rank] = col - goff[graph_of(goff, B, r)];
        if (HAS_W) vals[beg + rank] = __uint_as_float((unsigned)key);
    }
}

template <bool HAS_W>
__global__ void __launch_bounds__(kThreads) bb_sort_group_kernel(const int32_t *goff, int B, int R, const int32_t *rowptr,
                                                                 int32_t *gcol, int32_t *lcol, float *vals) {
    const long t = (long)blockIdx.x * kThreads + threadIdx.x;
    const long row = t >> 3;
    rank_sort_row<kGroupMax, HAS_W>(row < R ? (int)row : -1, (int)(t & 7), goff, B, rowptr, gcol, lcol, vals);
}

template <bool HAS_W>
__global__ void __launch_bounds__(kThreads) bb_sort_wave_kernel(const int32_t *goff, int B, const int32_t *rowptr,
                                                                const int32_t *rows, const int32_t *counts, int32_t *gcol,
                                                                int32_t *lcol, float *vals) {
    const int n = counts[0];
    const int wave = (int)(blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6));
    for (int i = wave; i < n; i += (int)gridDim.x * (kThreads / 64))
        rank_sort_row<kWaveMax, HAS_W>(rows[i], gmc::lane_id(), goff, B, rowptr, gcol, lcol, vals);
}

// The bitonic network in its one-direction form (the first step of every merge mirrors the upper half, so every
// compare-exchange moves the smaller key to the lower index): positions >= n act as +infinity without being stored.
template <int THREADS, class A>
__device__ __forceinline__ void bitonic_sort(A a, int n) {
    int P = 2;
    while (P < n) P <<= 1;
    for (int k = 2; k <= P; k <<= 1) {
        const int h = k >> 1;
        for (int t = threadIdx.x; t < (P >> 1); t += THREADS) {
            const int blk = t / h, off = t - blk * h;
            const int i = blk * k + off, l = blk * k + k - 1 - off;
            if (l < n) {
                const u64 x = a.load(i), y = a.load(l);
                if (x > y) { a.store(i, y); a.store(l, x); }
            }
        }
        __syncthreads();
        for (int j = h >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < (P >> 1); t += THREADS) {
                const int blk = t / j, off = t - blk * j;
                const int i = blk * 2 * j + off, l = i + j;
                if (l < n) {
                    const u64 x = a.load(i), y = a.load(l);
                    if (x > y) { a.store(i, y); a.store(l, x); }
                }
            }
            __syncthreads();
        }
    }
}

struct LdsKeys {
    u64 *k;
    __device__ __forceinline__ u64 load(int i) const { return k[i]; }
    __device__ __forceinline__ void store(int i, u64 v) const { k[i] = v; }
};
template <bool HAS_W>
struct GlobalKeys {
    int32_t *col; float *val;
    __device__ __forceinline__ u64 load(int i) const { return make_key(col[i], HAS_W ? val[i] : 0.0f); }
    __device__ __forceinline__ void store(int i, u64 v) const {
        col[i] = (int)(v >> 32);
        if (HAS_W) val[i] = __uint_as_float((unsigned)v);
    }
};

template <bool HAS_W>
__global__ void __launch_bounds__(kThreads) bb_sort_wg_kernel(const int32_t *goff, int B, const int32_t *rowptr,
                                                              const int32_t *rows, const int32_t *counts, int32_t *gcol,
                                                              int32_t *lcol, float *vals) {
    __shared__ u64 keys[kWgMax];
    const int n_rows = counts[1];
    for (int i = blockIdx.x; i < n_rows; i += gridDim.x) {
        const int r = rows[i], beg = rowptr[r];
        const int n = min(rowptr[r + 1] - beg, kWgMax);   // (the list holds rows of at most kWgMax entries)
        const int base = goff[graph_of(goff, B, r)];
        for (int t = threadIdx.x; t < n; t += kThreads) keys[t] = make_key(gcol[beg + t], HAS_W ? vals[beg + t] : 0.0f);
        __syncthreads();
        bitonic_sort<kThreads>(LdsKeys{keys}, n);
        for (int t = threadIdx.x; t < n; t += kThreads) {
            const int col = (int)(keys[t] >> 32);
            gcol[beg + t] = col;
            lcol[beg + t] = col - base;
            if (HAS_W) vals[beg + t] = __uint_as_float((unsigned)keys[t]);
        }
        __syncthreads();
    }
}

template <bool HAS_W>
__global__ void __launch_bounds__(kGlobalThreads) bb_sort_global_kernel(const int32_t *goff, int B, const int32_t *rowptr,
                                                                        const int32_t *rows, const int32_t *counts,
                                                                        int32_t *gcol, int32_t *lcol, float *vals) {
    const int n_rows = counts[2];
    for (int i = blockIdx.x; i < n_rows; i += gridDim.x) {
        const int r = rows[i], beg = rowptr[r], n = rowptr[r + 1] - beg;
        const int base = goff[graph_of(goff, B, r)];
        __syncthreads();
        bitonic_sort<kGlobalThreads>(GlobalKeys<HAS_W>{gcol + beg, vals + (HAS_W ? beg : 0)}, n);
        for (int t = threadIdx.x; t < n; t += kGlobalThreads) lcol[beg + t] = gcol[beg + t] - base;
    }
}

template <bool HAS_W>
__global__ void __launch_bounds__(kThreads) bb_validate_kernel(const int32_t *goff, int B, int R, int main_blocks,
                                                               const int32_t *rowptr, const int32_t *gcol,
                                                               const float *vals, int32_t *report) {
    __shared__ int lds[kThreads / 64];
    if ((int)blockIdx.x >= main_blocks) {   // one graph: its overflow blocks at both widths, its entries
        const int g = (int)blockIdx.x - main_blocks;
        const int r0 = min(max(goff[g], 0), R), r1 = min(max(goff[g + 1], r0), R);
        int b8 = 0, b16 = 0;
        for (int r = r0 + (int)threadIdx.x; r < r1; r += kThreads) {
            const int deg = rowptr[r + 1] - rowptr[r];
            b8 += (max(deg - 8, 0) + 7) >> 3;
            b16 += (max(deg - 16, 0) + 7) >> 3;
        }
        b8 = block_sum(b8, lds);
        b16 = block_sum(b16, lds);
        if (threadIdx.x == 0) {
            atomicMax(&report[GMC_BB_GRAPH_BLOCKS_8], b8);
            atomicMax(&report[GMC_BB_GRAPH_BLOCKS_16], b16);
            atomicAdd(&report[GMC_BB_BLOCKS_8], b8);
            atomicAdd(&report[GMC_BB_BLOCKS_16], b16);
            atomicMax(&report[GMC_BB_NNZ_MAX], rowptr[r1] - rowptr[r0]);
        }
        return;
    }
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    const int nnz = rowptr[R];
    int zero = 0, over8 = 0, over16 = 0, ex8 = 0, ex16 = 0, top = 0;
    if (i < R) {
        const int deg = rowptr[i + 1] - rowptr[i];
        zero = deg == 0;
        over8 = deg > 8; over16 = deg > 16;
        ex8 = max(deg - 8, 0); ex16 = max(deg - 16, 0);
        top = deg;
    }
    int dup = 0, asym = 0, nonunit = 0;
    if (i < nnz) {
        const int e = (int)i, c = gcol[e];
        int lo = 0, hi = R;   // the row of entry e: the last r with rowptr[r] <= e
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (rowptr[mid] <= e) lo = mid; else hi = mid - 1;
        }
        const int r = lo;
        dup = e > rowptr[r] && gcol[e - 1] == c;
        int a = rowptr[c];
        const int end = rowptr[c + 1];
        int b = end;
        while (a < b) {   // first entry of row c that is >= r
            const int mid = (a + b) >> 1;
            if (gcol[mid] < r) a = mid + 1; else b = mid;
        }
        asym = !(a < end && gcol[a] == r);
        if (HAS_W) {
            if (!asym) asym = vals[a] != vals[e];
            nonunit = vals[e] != 1.0f;
        }
    }
    const int lane = gmc::lane_id();
    zero = wave_sum_i(zero); over8 = wave_sum_i(over8); over16 = wave_sum_i(over16);
    ex8 = wave_sum_i(ex8); ex16 = wave_sum_i(ex16); top = wave_max_i(top);
    dup = wave_sum_i(dup); asym = wave_sum_i(asym); nonunit = wave_sum_i(nonunit);
    if (lane == 0) {
        if (zero) atomicAdd(&report[GMC_BB_ZERO_DEGREE], zero);
        if (over8) atomicAdd(&report[GMC_BB_ROWS_OVER_8], over8);
        if (over16) atomicAdd(&report[GMC_BB_ROWS_OVER_16], over16);
        if (ex8) atomicAdd(&report[GMC_BB_EXCESS_8], ex8);
        if (ex16) atomicAdd(&report[GMC_BB_EXCESS_16], ex16);
        if (top) {
            atomicMax(&report[GMC_BB_MAX_DEGREE], top);
            atomicMax(&report[GMC_BB_ROW_BLOCKS_8], (max(top - 8, 0) + 7) >> 3);
            atomicMax(&report[GMC_BB_ROW_BLOCKS_16], (max(top - 16, 0) + 7) >> 3);
        }
        if (dup) atomicAdd(&report[GMC_BB_DUPLICATE], dup);
        if (asym) atomicAdd(&report[GMC_BB_ASYMMETRIC], asym);
        if (nonunit) atomicAdd(&report[GMC_BB_NON_UNIT], nonunit);
    }
    if (i == 0) report[GMC_BB_NNZ] = nnz;
}

// ---- table stage -----------------------------------------------------------------------------------------------------
template <bool HAS_W>
__global__ void __launch_bounds__(kThreads) bb_ovf_fill_kernel(const int32_t *goff, int R, const int32_t *rowptr,
                                                               const int32_t *lcol, const float *vals, int W,
                                                               const int32_t *ovf_ptr, long capacity, uint16_t *ovf_ids,
                                                               float *ovf_vals) {
    const int g = blockIdx.x;
    const int r0 = goff[g], n = goff[g + 1] - r0;
    const int l = (int)(blockIdx.y * kThreads + threadIdx.x);
    if (r0 < 0 || n <= 0 || r0 + n > R || n + 4 > 65535 || l >= n) return;
    const int r = r0 + l, beg = rowptr[r], deg = rowptr[r + 1] - beg;
    const int slots = ((max(deg - W, 0) + 7) >> 3) * 8;
    const long base = (long)ovf_ptr[r] * 8;
    for (int k = 0; k < slots && base + k < capacity; ++k) {
        const bool has = W + k < deg;
        ovf_ids[base + k] = (uint16_t)(has ? lcol[beg + W + k] : n);   // padding: the zero row of the graph
        if (HAS_W) ovf_vals[base + k] = has ? vals[beg + W + k] : 0.0f;
    }
}

// rows (offsets inside a block of 16) that share one LDS cycle: ell_arrange.hip's kQuad
__device__ __forceinline__ int quad_row(int qd, int i) {
    const unsigned code = qd == 0 ? 0x6530u : qd == 1 ? 0x7421u : qd == 2 ? 0xEDB8u : 0xFCA9u;
    return (int)(code >> (4 * i)) & 15;
}
// the 24 permutations of {0,1,2,3} in std::next_permutation's order, two bits per element
#define GMC_BB_P(a, b, c, d) (unsigned char)((a) | ((b) << 2) | ((c) << 4) | ((d) << 6))
__device__ __constant__ unsigned char kPerm[24] = {
    GMC_BB_P(0, 1, 2, 3), GMC_BB_P(0, 1, 3, 2), GMC_BB_P(0, 2, 1, 3), GMC_BB_P(0, 2, 3, 1), GMC_BB_P(0, 3, 1, 2),
    GMC_BB_P(0, 3, 2, 1), GMC_BB_P(1, 0, 2, 3), GMC_BB_P(1, 0, 3, 2), GMC_BB_P(1, 2, 0, 3), GMC_BB_P(1, 2, 3, 0),
    GMC_BB_P(1, 3, 0, 2), GMC_BB_P(1, 3, 2, 0), GMC_BB_P(2, 0, 1, 3), GMC_BB_P(2, 0, 3, 1), GMC_BB_P(2, 1, 0, 3),
    GMC_BB_P(2, 1, 3, 0), GMC_BB_P(2, 3, 0, 1), GMC_BB_P(2, 3, 1, 0), GMC_BB_P(3, 0, 1, 2), GMC_BB_P(3, 0, 2, 1),
    GMC_BB_P(3, 1, 0, 2), GMC_BB_P(3, 1, 2, 0), GMC_BB_P(3, 2, 0, 1), GMC_BB_P(3, 2, 1, 0)};

__device__ __forceinline__ int byte_of(unsigned packed, int c) { return (int)(packed >> (8 * c)) & 0xff; }

// gmc_ell_arrange_host's arrange_quad for one quad per thread.  The quad's neighbours (per row: stably grouped by colour
// = id & 3, so "the next of colour c" is one packed counter away) and its slots live in LDS columns of this thread;
// per-row counters are four bytes of one register.
template <int W, bool HAS_W>
__global__ void __launch_bounds__(kQuadThreads) bb_arrange_kernel(const int32_t *goff, int R, const int32_t *rowptr,
                                                                  const int32_t *lcol, const float *vals, int NS,
                                                                  uint16_t *ell, float *ell_vals) {
    __shared__ uint16_t nb_id[4 * W][kQuadThreads];
    __shared__ uint16_t out_id[4 * W][kQuadThreads];
    __shared__ float nb_w[HAS_W ? 4 * W : 1][kQuadThreads];
    __shared__ float out_w[HAS_W ? 4 * W : 1][kQuadThreads];
    const int tid = threadIdx.x;
    const int g = blockIdx.x;
    const int r0 = goff[g], n = goff[g + 1] - r0;
    const int q = (int)(blockIdx.y * kQuadThreads) + tid;
    const int blk = (q >> 2) * 16, qd = q & 3;
    if (r0 < 0 || n <= 0 || r0 + n > R || n + 4 > 65535 || blk >= n) return;

    bool present[4];
    int rem[4];
    unsigned size[4], next[4];   // per colour: neighbours left, index of the next one
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int l = blk + quad_row(qd, i);
        present[i] = l < n;
        rem[i] = 0; size[i] = 0; next[i] = 0;
        if (!present[i]) continue;
        const int r = r0 + l, beg = rowptr[r];
        const int cnt = min(rowptr[r + 1] - beg, W);   // the first W neighbours: the rest are overflow entries
        for (int k = 0; k < cnt; ++k) size[i] += 1u << (8 * (lcol[beg + k] & 3));
        const unsigned s1 = byte_of(size[i], 0), s2 = s1 + byte_of(size[i], 1), s3 = s2 + byte_of(size[i], 2);
        next[i] = (s1 << 8) | (s2 << 16) | (s3 << 24);
        unsigned cur = next[i];
        for (int k = 0; k < cnt; ++k) {
            const int id = lcol[beg + k], c = id & 3;
            const int p = byte_of(cur, c);
            cur += 1u << (8 * c);
            nb_id[i * W + p][tid] = (uint16_t)id;
            if (HAS_W) nb_w[i * W + p][tid] = vals[beg + k];
        }
        rem[i] = cnt;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        for (int u = NS; u < W; ++u) {   // the slots the kernels skip
            out_id[i * W + u][tid] = (uint16_t)(n + (i & 3));
            if (HAS_W) out_w[i * W + u][tid] = 0.0f;
        }
    for (int u = 0; u < NS; ++u) {
        const int left = NS - u;   // slots still to fill, this one included
        const unsigned D = size[0] + size[1] + size[2] + size[3];   // remaining demand per colour (<= 64 each)
        unsigned best = kPerm[0];
        int best_conf = 99, best_gain = -1;
        for (int p = 0; p < 24; ++p) {
            const unsigned perm = kPerm[p];
            int conf = 0, gain = 0;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (!present[i] || rem[i] == 0) continue;   // absent row or only padding left
                const int c = (perm >> (2 * i)) & 3;
                const int have = byte_of(size[i], c);
                if (have) gain += 4 * byte_of(D, c) + have;
                else if (rem[i] >= left) ++conf;             // must place a neighbour now: off-colour
            }
            if (conf < best_conf || (conf == best_conf && gain > best_gain)) {
                best_conf = conf; best_gain = gain; best = perm;
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!present[i]) continue;
            const int want = (best >> (2 * i)) & 3;
            int c = want;
            if (rem[i] > 0 && byte_of(size[i], c) == 0 && rem[i] >= left) {   // forced off-colour: largest stock
                for (int cc = 0; cc < 4; ++cc)
                    if (byte_of(size[i], cc) > byte_of(size[i], c)) c = cc;
            }
            if (rem[i] > 0 && byte_of(size[i], c) != 0) {
                const int p = byte_of(next[i], c);
                next[i] += 1u << (8 * c);
                size[i] -= 1u << (8 * c);
                --rem[i];
                out_id[i * W + u][tid] = nb_id[i * W + p][tid];
                if (HAS_W) out_w[i * W + u][tid] = nb_w[i * W + p][tid];
            } else {   // padding: the all-zero row of the wanted quarter
                out_id[i * W + u][tid] = (uint16_t)(n + ((want - n) & 3));
                if (HAS_W) out_w[i * W + u][tid] = 0.0f;
            }
        }
    }
    // the hill-climb over swaps of two slots inside one row; cost of a slot = the largest number of distinct ids of one
    // quarter among the quad's ids
    auto slot_cost = [&](int u) {
        int ids[4] = {-1, -1, -1, -1};
        unsigned cnt = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!present[i]) continue;
            const int id = out_id[i * W + u][tid];
            bool dup = false;
#pragma unroll
            for (int j = 0; j < i; ++j) dup |= ids[j] == id;   // identical addresses broadcast
            if (!dup) { ids[i] = id; cnt += 1u << (8 * (id & 3)); }
        }
        return max(max(byte_of(cnt, 0), byte_of(cnt, 1)), max(byte_of(cnt, 2), byte_of(cnt, 3)));
    };
    for (int pass = 0, improved = 1; pass < 8 && improved; ++pass) {
        improved = 0;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (!present[i]) continue;
            for (int u = 0; u < NS; ++u)
                for (int v = u + 1; v < NS; ++v) {
                    const uint16_t a = out_id[i * W + u][tid], b = out_id[i * W + v][tid];
                    if ((a & 3) == (b & 3)) continue;   // same quarter: nothing changes
                    const int before = slot_cost(u) + slot_cost(v);
                    out_id[i * W + u][tid] = b; out_id[i * W + v][tid] = a;
                    if (slot_cost(u) + slot_cost(v) < before) {
                        if (HAS_W) {
                            const float t = out_w[i * W + u][tid];
                            out_w[i * W + u][tid] = out_w[i * W + v][tid];
                            out_w[i * W + v][tid] = t;
                        }
                        improved = 1;
                        continue;
                    }
                    out_id[i * W + u][tid] = a; out_id[i * W + v][tid] = b;
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (!present[i]) continue;
        const long base = (long)(r0 + blk + quad_row(qd, i)) * W;
        for (int u = 0; u < W; ++u) {
            ell[base + u] = out_id[i * W + u][tid];
            if (HAS_W) ell_vals[base + u] = out_w[i * W + u][tid];
        }
    }
}

template <bool HAS_W>
int csr_launch(int B, int R, long E, const int32_t *goff, const int32_t *src, const int32_t *dst, const float *w,
               int32_t *rowptr, int32_t *lcol, int32_t *gcol, float *vals, float *dinv, int32_t *report, const Ws &ws,
               hipStream_t st) {
    const int row_blocks = std::max(1, (int)(((long)std::max((int)R, (int)GMC_BB_REPORT_WORDS) + kThreads - 1) / kThreads));
    const int entry_blocks = (int)((E + kThreads - 1) / kThreads);
    const int sb = scan_blocks((long)R + 1);
    hipLaunchKernelGGL(bb_init_kernel, dim3(row_blocks), dim3(kThreads), 0, st, ws.deg, R, ws.counts, report);
    GMC_LAUNCH_CHECK();
    if (entry_blocks) {
        hipLaunchKernelGGL(bb_count_kernel, dim3(entry_blocks), dim3(kThreads), 0, st, goff, B, R, E, src, dst, ws.deg, report);
        GMC_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(bb_scan_sums_kernel<0>, dim3(sb), dim3(kThreads), 0, st, ws.deg, (long)R, 0, ws.sums);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(bb_scan_top_kernel, dim3(1), dim3(kThreads), 0, st, ws.sums, sb);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(bb_scan_add_kernel<0>, dim3(sb), dim3(kThreads), 0, st, ws.deg, (long)R, 0, ws.sums, rowptr, dinv,
                       ws.wave_rows, ws.wg_rows, ws.glob_rows, ws.counts);
    GMC_LAUNCH_CHECK();
    if (entry_blocks) {
        hipLaunchKernelGGL(bb_scatter_kernel<HAS_W>, dim3(entry_blocks), dim3(kThreads), 0, st, goff, B, R, E, src, dst, w,
                           rowptr, ws.deg, gcol, vals);
        GMC_LAUNCH_CHECK();
        const int group_blocks = (int)(((long)R * kGroupMax + kThreads - 1) / kThreads);
        hipLaunchKernelGGL(bb_sort_group_kernel<HAS_W>, dim3(group_blocks), dim3(kThreads), 0, st, goff, B, R, rowptr, gcol,
                           lcol, vals);
        GMC_LAUNCH_CHECK();
        hipLaunchKernelGGL(bb_sort_wave_kernel<HAS_W>, dim3(std::min(kListGrid, (R + 3) / 4)), dim3(kThreads), 0, st, goff, B,
                           rowptr, ws.wave_rows, ws.counts, gcol, lcol, vals);
        GMC_LAUNCH_CHECK();
        hipLaunchKernelGGL(bb_sort_wg_kernel<HAS_W>, dim3(std::min(kListGrid, R)), dim3(kThreads), 0, st, goff, B, rowptr,
                           ws.wg_rows, ws.counts, gcol, lcol, vals);
        GMC_LAUNCH_CHECK();
        hipLaunchKernelGGL(bb_sort_global_kernel<HAS_W>, dim3(std::min(kListGrid, R)), dim3(kGlobalThreads), 0, st, goff, B,
                           rowptr, ws.glob_rows, ws.counts, gcol, lcol, vals);
        GMC_LAUNCH_CHECK();
    }
    const int main_blocks = std::max(1, (int)((std::max((long)R, E) + kThreads - 1) / kThreads));
    hipLaunchKernelGGL(bb_validate_kernel<HAS_W>, dim3(main_blocks + B), dim3(kThreads), 0, st, goff, B, R, main_blocks,
                       rowptr, gcol, vals, report);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

template <int W, bool HAS_W>
int arrange_launch(int B, int R, int n_max, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol,
                   const float *vals, int NS, uint16_t *ell, float *ell_vals, hipStream_t st) {
    const int quads = (n_max + 15) / 16 * 4;
    hipLaunchKernelGGL((bb_arrange_kernel<W, HAS_W>), dim3(B, (quads + kQuadThreads - 1) / kQuadThreads), dim3(kQuadThreads),
                       0, st, goff, R, rowptr, lcol, vals, NS, ell, ell_vals);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// out[r] = +0 plus the weights of row r's entries one after the other in the row's (sorted) order, the entry on the
// diagonal skipped; one thread per row, so the order holds by construction (gmc_row_weight_sums_f32)
__global__ __launch_bounds__(kThreads) void bb_row_weight_sums_kernel(int R, const int32_t *rowptr, const int32_t *gcol,
                                                                      const float *vals, float *out) {
    const long r = (long)blockIdx.x * kThreads + threadIdx.x;
    if (r >= R) return;
    float s = 0.f;
    for (int e = rowptr[r]; e < rowptr[r + 1]; ++e)
        if (gcol[e] != r) s += vals ? vals[e] : 1.0f;
    out[r] = s;
}

}  // namespace

extern "C" int gmc_row_weight_sums_f32(int32_t R, const int32_t *rowptr, const int32_t *gcol, const float *vals,
                                       float *out, gmc_stream_t stream) {
    if (!rowptr || !out) return GMC_ERR_NULL;
    if (R < 0) return GMC_ERR_SHAPE;
    if (R == 0) return GMC_OK;
    if (!gcol) return GMC_ERR_NULL;
    hipLaunchKernelGGL(bb_row_weight_sums_kernel, dim3((R + kThreads - 1) / kThreads), dim3(kThreads), 0,
                       static_cast<hipStream_t>(stream), R, rowptr, gcol, vals, out);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" size_t gmc_batch_build_workspace_bytes(int32_t B, int32_t R, int64_t E) {
    if (B < 0 || R < 0 || E < 0 || E > INT32_MAX) return 0;
    return std::max<size_t>(carve(nullptr, R).bytes, 16);
}

extern "C" int gmc_batch_build_csr(int32_t B, int32_t R, int64_t E, const int32_t *goff, const int32_t *src,
                                   const int32_t *dst, const float *w, int32_t *rowptr, int32_t *lcol, int32_t *gcol,
                                   float *vals, float *dinv, int32_t *report, void *workspace, size_t workspace_bytes,
                                   gmc_stream_t stream) {
    if (!goff || !rowptr || !dinv || !report || !workspace) return GMC_ERR_NULL;
    if (E > 0 && (!src || !dst || !lcol || !gcol)) return GMC_ERR_NULL;
    if (w && E > 0 && !vals) return GMC_ERR_NULL;
    if (B < 0 || R < B || E < 0 || E > INT32_MAX) return GMC_ERR_SHAPE;   // (every graph has a row)
    if (workspace_bytes < gmc_batch_build_workspace_bytes(B, R, E)) return GMC_ERR_WORKSPACE;
    if (B == 0) return GMC_OK;
    const Ws ws = carve(workspace, R);
    hipStream_t st = static_cast<hipStream_t>(stream);
    return w ? csr_launch<true>(B, R, (long)E, goff, src, dst, w, rowptr, lcol, gcol, vals, dinv, report, ws, st)
             : csr_launch<false>(B, R, (long)E, goff, src, dst, w, rowptr, lcol, gcol, vals, dinv, report, ws, st);
}

extern "C" int gmc_batch_build_table(int32_t B, int32_t R, int32_t n_max, const int32_t *goff, const int32_t *rowptr,
                                     const int32_t *lcol, const float *vals, int32_t W, int32_t NS, uint16_t *ell,
                                     float *ell_vals, int32_t *ovf_ptr, uint16_t *ovf_ids, float *ovf_vals,
                                     int32_t ovf_blocks, void *workspace, size_t workspace_bytes, gmc_stream_t stream) {
    if (!goff || !rowptr || !lcol || !ell || !workspace) return GMC_ERR_NULL;
    if (vals && !ell_vals) return GMC_ERR_NULL;
    if (ovf_ptr && (!ovf_ids || (vals && !ovf_vals))) return GMC_ERR_NULL;
    if (B < 0 || R < B || ovf_blocks < 0 || (W != 8 && W != 16) || NS < 1 || NS > W) return GMC_ERR_SHAPE;
    if (B > 0 && (n_max < 3 || n_max + 4 > 65535)) return GMC_ERR_GRAPH_SIZE;
    if (workspace_bytes < gmc_batch_build_workspace_bytes(B, R, 0)) return GMC_ERR_WORKSPACE;
    if (B == 0) return GMC_OK;
    const Ws ws = carve(workspace, R);
    hipStream_t st = static_cast<hipStream_t>(stream);
    if (ovf_ptr) {
        const int sb = scan_blocks((long)R + 1);
        hipLaunchKernelGGL(bb_scan_sums_kernel<1>, dim3(sb), dim3(kThreads), 0, st, rowptr, (long)R, W, ws.sums);
        GMC_LAUNCH_CHECK();
        hipLaunchKernelGGL(bb_scan_top_kernel, dim3(1), dim3(kThreads), 0, st, ws.sums, sb);
        GMC_LAUNCH_CHECK();
        hipLaunchKernelGGL(bb_scan_add_kernel<1>, dim3(sb), dim3(kThreads), 0, st, rowptr, (long)R, W, ws.sums, ovf_ptr,
                           nullptr, nullptr, nullptr, nullptr, nullptr);
        GMC_LAUNCH_CHECK();
        const dim3 grid(B, (n_max + kThreads - 1) / kThreads);
        if (vals)
            hipLaunchKernelGGL(bb_ovf_fill_kernel<true>, grid, dim3(kThreads), 0, st, goff, R, rowptr, lcol, vals, W, ovf_ptr,
                               (long)ovf_blocks * 8, ovf_ids, ovf_vals);
        else
            hipLaunchKernelGGL(bb_ovf_fill_kernel<false>, grid, dim3(kThreads), 0, st, goff, R, rowptr, lcol, vals, W,
                               ovf_ptr, (long)ovf_blocks * 8, ovf_ids, ovf_vals);
        GMC_LAUNCH_CHECK();
    }
    if (W == 8)
        return vals ? arrange_launch<8, true>(B, R, n_max, goff, rowptr, lcol, vals, NS, ell, ell_vals, st)
                    : arrange_launch<8, false>(B, R, n_max, goff, rowptr, lcol, vals, NS, ell, ell_vals, st);
    return vals ? arrange_launch<16, true>(B, R, n_max, goff, rowptr, lcol, vals, NS, ell, ell_vals, st)
                : arrange_launch<16, false>(B, R, n_max, goff, rowptr, lcol, vals, NS, ell, ell_vals, st);
}
