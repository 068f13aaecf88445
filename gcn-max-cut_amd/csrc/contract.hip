// Contracting pinned nodes on the device (include/gcnmaxcut.h, "pinning any nodes to classes"): every node pinned to
// class c of a graph becomes that graph's super-node c, the free nodes follow in ascending order, parallel entries
// between a free node and a class are merged into one weight, entries between pinned nodes become the constant fixed_cut.
//
// Map stage (gmc_contract_map), every step one launch, kernel boundaries the only synchronisation:
//   init      class word of every row = free; its entry count, the per-graph class masks and the report = 0
//   pins      per pin: range checks, then an integer compare-and-swap free -> class on the row's word; a word that already
//             holds another class gets its conflict bit set (the thread that sets it counts the node, once)
//   count     per row (grid: graph x tile of 256 rows): a pinned row adds its class to the graph's "present" mask; a free row
//             walks its entries and leaves (1 << 32 | entries it will emit) and adds the classes it touches to the graph's
//             "has a free neighbour" mask (a wave ORs its masks first: one integer atomic per wave and mask)
//   scan x3   exclusive scan of those 64-bit words over R + 1 rows: the high half ranks the free rows, the low half places
//             every row's output entries (the sum of the low halves is E' <= E < 2^31: no carry into the ranks)
//   finish    node_map per row; per graph goff_out and the graph's share of the report
// Entries stage (gmc_contract_entries), on the class words and offsets the map stage left in the workspace:
//   emit      one thread per row, whatever its length (the only row regime).  A free row walks its sorted entries once:
//             free neighbours are emitted as they come, pinned ones are added to one of K running sums in registers
//             (ascending column = the row's own order), then every touched class is emitted in both directions with the
//             same bits.  A pinned row adds the weights of its entries to pinned nodes of another class and a larger row
//             id (every such edge once).  The 256 rows of a tile then fold those sums: the wave butterfly of distance
//             32, 16, .., 1, then wave 0 + wave 1 + wave 2 + wave 3 in that order
//   fold      per graph: its tiles' partials, added one after the other in ascending tile order to +0
// Nothing is added with a floating-point atomic, no kernel indexes a register array with a run-time value (no scratch),
// and a pin's node id becomes an index only behind its range check, in the same kernel.
#include "gmc_common.h"

#include <algorithm>

namespace {

typedef unsigned long long u64;

constexpr int kThreads = 256;              // rows of a tile
constexpr int kScanBlock = kThreads * 4;   // words of one scan workgroup
constexpr int kFree = -1;                  // class word of a row without a pin
constexpr int kConflict = 0x100;           // set on a class word that was given a second class
constexpr int kClassBits = 7;              // class of a pinned row's word (K <= 8)

static size_t up16(size_t x) { return (x + 15) & ~(size_t)15; }
static int scan_blocks(long n) { return (int)((n + kScanBlock - 1) / kScanBlock); }

struct Ws {
    int32_t *cls;     // [R]      class words
    u64 *val;         // [R]      free flag << 32 | output entries of the row
    u64 *off;         // [R + 1]  exclusive scan of val
    u64 *sums;        // [scan_blocks(R + 1) + 1]
    int32_t *gbits;   // [2B]     per graph: classes with a pinned node, classes with a free neighbour
    float *part;      // [R / 256 + B + 1]  fixed_cut partials: graph g's tiles from slot goff[g] / 256 + g
    size_t bytes;
};

Ws carve(void *base, long B, long R) {
    Ws w{};
    const uintptr_t p = reinterpret_cast<uintptr_t>(base);   // (nullptr: the size query, nothing is dereferenced)
    size_t o = 0;
    auto take = [&](size_t bytes) { const uintptr_t q = p + o; o += up16(bytes); return q; };
    w.cls = reinterpret_cast<int32_t *>(take((size_t)R * 4));
    w.val = reinterpret_cast<u64 *>(take((size_t)R * 8));
    w.off = reinterpret_cast<u64 *>(take(((size_t)R + 1) * 8));
    w.sums = reinterpret_cast<u64 *>(take(((size_t)scan_blocks(R + 1) + 1) * 8));
    w.gbits = reinterpret_cast<int32_t *>(take((size_t)B * 8));
    w.part = reinterpret_cast<float *>(take(((size_t)R / kThreads + (size_t)B + 1) * 4));
    w.bytes = o;
    return w;
}

__device__ __forceinline__ int hi32(u64 v) { return (int)(v >> 32); }
__device__ __forceinline__ int lo32(u64 v) { return (int)(unsigned)v; }

__device__ __forceinline__ int wave_or(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v |= __shfl_xor(v, o);
    return v;
}

// rows [r0, r1) of graph g inside 0..R, and this thread's row (r1 or more: none)
struct Rows { int r0, r1, r; };
__device__ __forceinline__ Rows tile_rows(const int32_t *goff, int R) {
    const int g = blockIdx.x;
    Rows t;
    t.r0 = min(max(goff[g], 0), R);
    t.r1 = min(max(goff[g + 1], t.r0), R);
    const long r = (long)t.r0 + (long)blockIdx.y * kThreads + threadIdx.x;
    t.r = r < t.r1 ? (int)r : t.r1;
    return t;
}

// ---- map stage -------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kThreads) ct_init_kernel(int32_t *cls, u64 *val, int R, int32_t *gbits, long nbits,
                                                           int32_t *report) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i < R) { cls[i] = kFree; val[i] = 0; }   // (val: a row no graph of the batch owns emits nothing)
    if (i < nbits) gbits[i] = 0;
    if (i < GMC_CT_REPORT_WORDS) report[i] = 0;
}

__global__ void __launch_bounds__(kThreads) ct_pins_kernel(long P, const int32_t *pin_node, const int32_t *pin_class, int R,
                                                           int K, int32_t *cls, int32_t *report) {
    const long p = (long)blockIdx.x * kThreads + threadIdx.x;
    if (p >= P) return;
    const int u = pin_node[p], c = pin_class[p];
    if ((unsigned)u >= (unsigned)R) { atomicAdd(&report[GMC_CT_PIN_OUT_OF_RANGE], 1); return; }
    if ((unsigned)c >= (unsigned)K) { atomicAdd(&report[GMC_CT_PIN_CLASS], 1); return; }
    const int old = atomicCAS(&cls[u], kFree, c);
    if (old == kFree || (old & kClassBits) == c) return;   // the first pin of the node, or a repeat of it
    if (!(atomicOr(&cls[u], kConflict) & kConflict)) atomicAdd(&report[GMC_CT_PIN_CONFLICT], 1);
}

__global__ void __launch_bounds__(kThreads) ct_count_kernel(const int32_t *goff, int R, const int32_t *rowptr,
                                                            const int32_t *gcol, const int32_t *cls, u64 *val,
                                                            int32_t *gbits) {
    const Rows t = tile_rows(goff, R);
    int present = 0, touched = 0;
    if (t.r < t.r1) {
        const int c = cls[t.r];
        if (c >= 0) {
            present = 1 << (c & kClassBits);
            val[t.r] = 0;
        } else {
            int nfree = 0;
            for (int e = rowptr[t.r]; e < rowptr[t.r + 1]; ++e) {
                const int cx = cls[gcol[e]];
                if (cx < 0) ++nfree; else touched |= 1 << (cx & kClassBits);
            }
            val[t.r] = ((u64)1 << 32) | (u64)(unsigned)(nfree + 2 * __popc(touched));
        }
    }
    present = wave_or(present);
    touched = wave_or(touched);
    if (gmc::lane_id() == 0) {
        if (present) atomicOr(&gbits[2 * (long)blockIdx.x], present);
        if (touched) atomicOr(&gbits[2 * (long)blockIdx.x + 1], touched);
    }
}

__device__ __forceinline__ u64 scan_value(const u64 *val, long i, long R) { return i < R ? val[i] : 0; }

__global__ void __launch_bounds__(kThreads) ct_scan_sums_kernel(const u64 *val, long R, u64 *sums) {
    __shared__ u64 lds[kThreads];
    const long i0 = (long)blockIdx.x * kScanBlock + threadIdx.x * 4;
    u64 v = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) v += scan_value(val, i0 + k, R);
    lds[threadIdx.x] = v;
    __syncthreads();
    for (int o = kThreads >> 1; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) lds[threadIdx.x] += lds[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) sums[blockIdx.x] = lds[0];
}

// one workgroup: sums[0..n) -> its exclusive prefix, 256 at a time with a carry
__global__ void __launch_bounds__(kThreads) ct_scan_top_kernel(u64 *sums, int n) {
    __shared__ u64 lds[kThreads];
    u64 carry = 0;
    for (int base = 0; base < n; base += kThreads) {
        const int i = base + threadIdx.x;
        const u64 own = i < n ? sums[i] : 0;
        lds[threadIdx.x] = own;
        __syncthreads();
        for (int o = 1; o < kThreads; o <<= 1) {
            const u64 add = (int)threadIdx.x >= o ? lds[threadIdx.x - o] : 0;
            __syncthreads();
            lds[threadIdx.x] += add;
            __syncthreads();
        }
        if (i < n) sums[i] = carry + lds[threadIdx.x] - own;
        carry += lds[kThreads - 1];
        __syncthreads();
    }
}

__global__ void __launch_bounds__(kThreads) ct_scan_add_kernel(const u64 *val, long R, const u64 *sums, u64 *off) {
    __shared__ u64 lds[kThreads];
    const long i0 = (long)blockIdx.x * kScanBlock + threadIdx.x * 4;
    u64 v[4], own = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = scan_value(val, i0 + k, R); own += v[k]; }
    lds[threadIdx.x] = own;
    __syncthreads();
    for (int o = 1; o < kThreads; o <<= 1) {
        const u64 add = (int)threadIdx.x >= o ? lds[threadIdx.x - o] : 0;
        __syncthreads();
        lds[threadIdx.x] += add;
        __syncthreads();
    }
    u64 run = sums[blockIdx.x] + lds[threadIdx.x] - own;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (i0 + k <= R) off[i0 + k] = run;
        run += v[k];
    }
}

__global__ void __launch_bounds__(kThreads) ct_finish_kernel(const int32_t *goff, int B, int R, int K, const int32_t *cls,
                                                             const u64 *off, const int32_t *gbits, int32_t *node_map,
                                                             int32_t *goff_out, int32_t *report) {
    const Rows t = tile_rows(goff, R);
    const int g = blockIdx.x;
    const int free_before = hi32(off[t.r0]);
    const int base = (int)((long)K * g + free_before);   // goff_out[g]
    if (t.r < t.r1) {
        const int c = cls[t.r];
        node_map[t.r] = c >= 0 ? base + (c & kClassBits) : (int)((long)K * (g + 1) + hi32(off[t.r]));
    }
    if (blockIdx.y != 0 || threadIdx.x != 0) return;
    goff_out[g] = base;
    const int present = gbits[2 * (long)g], touched = gbits[2 * (long)g + 1];
    if (present != (1 << K) - 1) atomicAdd(&report[GMC_CT_GRAPHS_MISSING_CLASS], 1);
    if (hi32(off[t.r1]) == free_before) atomicAdd(&report[GMC_CT_GRAPHS_NO_FREE], 1);
    const int bare = __popc(present & ~touched);
    if (bare) atomicAdd(&report[GMC_CT_BARE_TERMINALS], bare);
    if (g == B - 1) {
        goff_out[B] = (int)((long)K * B + hi32(off[R]));
        report[GMC_CT_NNZ] = lo32(off[R]);
        report[GMC_CT_PINNED] = R - hi32(off[R]);
    }
}

// ---- entries stage ---------------------------------------------------------------------------------------------------
struct EmitArgs {
    const int32_t *goff, *rowptr, *gcol;
    const float *vals;
    const int32_t *cls;
    const u64 *off;
    const int32_t *node_map, *goff_out;
    int32_t *src_out, *dst_out;
    float *w_out;
    float *part;
    long E_out;
    int R;
};

__device__ __forceinline__ void emit(const EmitArgs &a, long pos, int s, int d, float w) {
    if (pos < a.E_out) { a.src_out[pos] = s; a.dst_out[pos] = d; a.w_out[pos] = w; }
}

template <int KK, bool HAS_W>
__global__ void __launch_bounds__(kThreads) ct_emit_kernel(EmitArgs a) {
    __shared__ float lds[kThreads / GMC_WAVE];
    const Rows t = tile_rows(a.goff, a.R);
    const int g = blockIdx.x;
    float cut = 0.0f;   // a pinned row's share of fixed_cut
    if (t.r < t.r1) {
        const int r = t.r, c = a.cls[r];
        const int beg = a.rowptr[r], end = a.rowptr[r + 1];
        if (c >= 0) {
            for (int e = beg; e < end; ++e) {
                const int x = a.gcol[e], cx = a.cls[x];
                if (cx >= 0 && x > r && (cx & kClassBits) != (c & kClassBits)) cut += HAS_W ? a.vals[e] : 1.0f;
            }
        } else {
            long pos = lo32(a.off[r]);
            const int me = a.node_map[r], base = a.goff_out[g];
            float sum[KK];
#pragma unroll
            for (int k = 0; k < KK; ++k) sum[k] = 0.0f;
            int touched = 0;
            for (int e = beg; e < end; ++e) {
                const int x = a.gcol[e], cx = a.cls[x];
                const float w = HAS_W ? a.vals[e] : 1.0f;
                if (cx < 0) {
                    emit(a, pos++, me, a.node_map[x], w);
                } else {
                    const int k0 = cx & kClassBits;
                    touched |= 1 << k0;
#pragma unroll
                    for (int k = 0; k < KK; ++k) sum[k] = k == k0 ? sum[k] + w : sum[k];
                }
            }
#pragma unroll
            for (int k = 0; k < KK; ++k)
                if ((touched >> k) & 1) {
                    emit(a, pos, me, base + k, sum[k]);
                    emit(a, pos + 1, base + k, me, sum[k]);
                    pos += 2;
                }
        }
    }
    cut = gmc::wave_sum(cut);
    if (gmc::lane_id() == 0) lds[threadIdx.x >> 6] = cut;
    __syncthreads();
    if (threadIdx.x == 0 && (long)t.r0 + (long)blockIdx.y * kThreads < t.r1)
        a.part[t.r0 / kThreads + g + (int)blockIdx.y] = ((lds[0] + lds[1]) + lds[2]) + lds[3];
}

__global__ void __launch_bounds__(kThreads) ct_fold_kernel(const int32_t *goff, int B, int R, const float *part,
                                                           float *fixed_cut) {
    const long g = (long)blockIdx.x * kThreads + threadIdx.x;
    if (g >= B) return;
    const int r0 = min(max(goff[g], 0), R), r1 = min(max(goff[g + 1], r0), R);
    const int tiles = (r1 - r0 + kThreads - 1) / kThreads;
    float f = 0.0f;
    for (int j = 0; j < tiles; ++j) f += part[r0 / kThreads + g + j];
    fixed_cut[g] = f;
}

template <int KK>
int emit_launch(const EmitArgs &a, bool has_w, dim3 grid, hipStream_t st) {
    if (has_w) hipLaunchKernelGGL((ct_emit_kernel<KK, true>), grid, dim3(kThreads), 0, st, a);
    else hipLaunchKernelGGL((ct_emit_kernel<KK, false>), grid, dim3(kThreads), 0, st, a);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

// the checks the two stages share, in the library's order; GMC_OK: go on
int check_batch(const gmc_batch *batch, int K, const void *workspace, size_t workspace_bytes, int64_t extra) {
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (!batch->goff || !batch->rowptr || (batch->nnz > 0 && !batch->gcol)) return GMC_ERR_NULL;
    if (K < 2 || K > GMC_KWAY_MAX_CLASSES) return GMC_ERR_CLASSES;
    if (batch->B < 0 || batch->R < 0 || batch->nnz < 0 || batch->n_max < 0 || extra < 0) return GMC_ERR_SHAPE;
    if (batch->n_max > GMC_LARGE_MAX_GRAPH_NODES) return GMC_ERR_GRAPH_SIZE;
    if (workspace_bytes < gmc_contract_workspace_bytes(batch->B, batch->R, batch->nnz, K)) return GMC_ERR_WORKSPACE;
    return GMC_OK;
}

dim3 tile_grid(const gmc_batch *batch) {
    return dim3(batch->B, std::max(1, (batch->n_max + kThreads - 1) / kThreads));
}

}  // namespace

extern "C" size_t gmc_contract_workspace_bytes(int32_t B, int32_t R, int64_t E, int32_t K) {
    if (B < 0 || R < 0 || E < 0 || E > INT32_MAX || K < 2 || K > GMC_KWAY_MAX_CLASSES) return 0;
    return std::max<size_t>(carve(nullptr, B, R).bytes, 16);
}

extern "C" int gmc_contract_map(const gmc_batch *batch, int32_t K, int64_t P, const int32_t *pin_node,
                                const int32_t *pin_class, int32_t *node_map, int32_t *goff_out, int32_t *report,
                                void *workspace, size_t workspace_bytes, gmc_stream_t stream) {
    if (!batch || !node_map || !goff_out || !report || !workspace) return GMC_ERR_NULL;
    if (P > 0 && (!pin_node || !pin_class)) return GMC_ERR_NULL;
    const int rc = check_batch(batch, K, workspace, workspace_bytes, P);
    if (rc != GMC_OK) return rc;
    const int B = batch->B, R = batch->R;
    if (B == 0) return GMC_OK;
    const Ws ws = carve(workspace, B, R);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const long init_n = std::max<long>(std::max<long>(R, 2L * B), GMC_CT_REPORT_WORDS);
    hipLaunchKernelGGL(ct_init_kernel, dim3((unsigned)((init_n + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, ws.cls,
                       ws.val, R, ws.gbits, 2L * B, report);
    GMC_LAUNCH_CHECK();
    if (P > 0) {
        hipLaunchKernelGGL(ct_pins_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, (long)P,
                           pin_node, pin_class, R, K, ws.cls, report);
        GMC_LAUNCH_CHECK();
    }
    const dim3 grid = tile_grid(batch);
    hipLaunchKernelGGL(ct_count_kernel, grid, dim3(kThreads), 0, st, batch->goff, R, batch->rowptr, batch->gcol, ws.cls,
                       ws.val, ws.gbits);
    GMC_LAUNCH_CHECK();
    const int sb = scan_blocks((long)R + 1);
    hipLaunchKernelGGL(ct_scan_sums_kernel, dim3(sb), dim3(kThreads), 0, st, ws.val, (long)R, ws.sums);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_scan_top_kernel, dim3(1), dim3(kThreads), 0, st, ws.sums, sb);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_scan_add_kernel, dim3(sb), dim3(kThreads), 0, st, ws.val, (long)R, ws.sums, ws.off);
    GMC_LAUNCH_CHECK();
    hipLaunchKernelGGL(ct_finish_kernel, grid, dim3(kThreads), 0, st, batch->goff, B, R, K, ws.cls, ws.off, ws.gbits,
                       node_map, goff_out, report);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}

extern "C" int gmc_contract_entries(const gmc_batch *batch, int32_t K, const int32_t *node_map, const int32_t *goff_out,
                                    int64_t E_out, int32_t *src_out, int32_t *dst_out, float *w_out, float *fixed_cut,
                                    void *workspace, size_t workspace_bytes, gmc_stream_t stream) {
    if (!batch || !node_map || !goff_out || !fixed_cut || !workspace) return GMC_ERR_NULL;
    if (E_out > 0 && (!src_out || !dst_out || !w_out)) return GMC_ERR_NULL;
    const int rc = check_batch(batch, K, workspace, workspace_bytes, E_out);
    if (rc != GMC_OK) return rc;
    const int B = batch->B, R = batch->R;
    if (B == 0) return GMC_OK;
    const Ws ws = carve(workspace, B, R);
    hipStream_t st = static_cast<hipStream_t>(stream);
    const EmitArgs a{batch->goff, batch->rowptr, batch->gcol, batch->vals, ws.cls, ws.off, node_map, goff_out,
                     src_out, dst_out, w_out, ws.part, (long)E_out, R};
    int erc = GMC_OK;
    GMC_KWAY_DISPATCH(K, erc = emit_launch<KK>(a, batch->vals != nullptr, tile_grid(batch), st));
    if (erc != GMC_OK) return erc;
    hipLaunchKernelGGL(ct_fold_kernel, dim3((unsigned)((B + kThreads - 1) / kThreads)), dim3(kThreads), 0, st, batch->goff, B,
                       R, ws.part, fixed_cut);
    GMC_LAUNCH_CHECK();
    return GMC_OK;
}
