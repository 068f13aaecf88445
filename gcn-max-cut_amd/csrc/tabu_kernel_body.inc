// The chain and the kernel of gmc_kway_tabu_f32 and gmc_kway_tabu_c_f32 (kway_tabu.hip), included once for each with
// GMC_COST defined false / true: does the launch have per-node class costs?  The including file also names the
// argument struct (GMC_CHAIN_ARGS: TabuArgs, or TabuCostArgs = the same fields and node_cost) and the kernel
// (GMC_CHAIN_KERNEL).  Text and not a template parameter for anneal_kernel_body.inc's reasons: the kernel without costs
// keeps its name, its argument struct and its instructions (DESIGN.md section 35 has the comparison), and the cost
// kernel is the same statements with two differences - the table starts from the node's cost row, and the snapshots
// are scored by gmc::block_score.  The cost is read from global memory at those two places only.

// One chain on the calling wave: the table, the iterations, the snapshot left in sn.  lds: the chain's bytes.
// With GMC_COST, nc: the graph's cost rows by local id (node_cost + r0 * K).
template <int K, class G>
__device__ __forceinline__ void tabu_chain(const GMC_CHAIN_ARGS &a, const G &g, unsigned char *lds, int n, int cand,
                                           const signed char *in, int &best_it_out, int &moves_out
#if GMC_COST
                                           , const float *nc
#endif
                                           ) {
    const int lane = gmc::lane_id();
    float *W = reinterpret_cast<float *>(lds);
    unsigned *until = reinterpret_cast<unsigned *>(lds + (size_t)a.n_pad * K * 4);
    unsigned char *st = lds + (size_t)a.n_pad * (K * 4 + 4);
    unsigned char *sn = st + a.n_pad;
    const int first = a.first;
    const int n_mov = n - first;
    for (int l = lane; l < n; l += GMC_WAVE) {
        const unsigned char c = (unsigned char)in[l];
        st[l] = c;
        sn[l] = c;
        until[l] = 0u;
    }
    int best_it = 0, moves = 0;
    if (a.iterations > 0 && n_mov > 0) {
        wave_sync();
        for (int l = lane; l < n; l += GMC_WAVE) {
#if GMC_COST
            // (+ 0.0f: a sum that is -0.0 - a cost of -0.0 under a class without neighbours - enters the table as +0.0, so
            // that no gain is ever -0.0 and ordered_bits' order is the floats'; every other value is unchanged)
            const gmc::Sums<K> s = gmc::class_sums_k<K>(g.rp, g.col, g.vals, st, l, nc);
#pragma unroll
            for (int k = 0; k < K; ++k) W[l * K + k] = s.m[k] + 0.0f;
#else
            const gmc::Sums<K> s = gmc::class_sums_k<K>(g.rp, g.col, g.vals, st, l);
#pragma unroll
            for (int k = 0; k < K; ++k) W[l * K + k] = s.m[k];
#endif
        }
        wave_sync();
        float rel = 0.0f, best = 0.0f;
        bool pending = false;   // the state is better than the snapshot and not copied yet
        const unsigned span = a.tenure_span + (a.tenure_div > 0 ? (unsigned)n_mov / a.tenure_div : 0u);
        const u64 base = a.seed + GMC_GOLD * (((u64)(unsigned)cand << 32) + 1ULL);   // it < 2^32 only adds
        const int trips = (n_mov + GMC_WAVE - 1) / GMC_WAVE;   // scan steps of a lane
        for (int it = 0; it < a.iterations; ++it) {
            const u64 h = mix64(base + GMC_GOLD * (u64)(unsigned)it);
            const int r = (int)((unsigned)h % (unsigned)n_mov);
            const unsigned tenure_draw = (unsigned)(h >> 32) % (span + 1u);
            // 2-3. the lane's best admissible move
            // (a wave-uniform trip count and unconditional loads from a clamped node, so that the unrolled steps' LDS
            // reads go out together: a lane past its last node reads node `first` and admits nothing)
            u64 key = 0;
#pragma unroll 2
            for (int t = 0; t < trips; ++t) {
                const int v0 = first + lane + (t << 6);
                const bool valid = v0 < n;
                const int v = valid ? v0 : first;
                const unsigned c = st[v];
                float w[K];
#pragma unroll
                for (int k = 0; k < K; ++k) w[k] = W[v * K + k];
                float wc = w[0];
#pragma unroll
                for (int j = 1; j < K; ++j) wc = c == (unsigned)j ? w[j] : wc;
                const bool is_free = until[v] <= (unsigned)it;
                int rank = v - first - r;
                rank = rank < 0 ? rank + n_mov : rank;
                // the node's own best move - the largest gain, the smallest k on ties - stands for all its moves: when
                // the node is banned, rel + gain is monotone in the gain, so if any of its moves is admissible this one is
                float bg = -__builtin_inff();
                int bk = 0;
#pragma unroll
                for (int k = 0; k < K; ++k) {
                    const float gain = wc - w[k];
                    const bool take = c != (unsigned)k && gain > bg;
                    bg = take ? gain : bg;
                    bk = take ? k : bk;
                }
                // (a byte of no class: the node never moves)
                const bool adm = valid && c < (unsigned)K && (is_free || rel + bg > best);
                const u64 cnd = ((u64)ordered_bits(bg) << 32) | (u64)(~(unsigned)(rank * K + bk));
                key = adm && cnd > key ? cnd : key;
            }
            key = wave_max(key);
            const unsigned khi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key >> 32));
            const unsigned klo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key);
            if (khi == 0u && klo == 0u) continue;   // no admissible move (wave-uniform)
            const unsigned x = ~klo;
            const int k = (int)(x % (unsigned)K);
            int v = first + (int)(x / (unsigned)K) + r;
            v = v - first >= n_mov ? v - n_mov : v;
            const float gain = ordered_float(khi);
            const float new_rel = rel + gain;
            const bool improves = new_rel > best;
            if (!improves && pending) {   // the snapshot takes the state before this move
                const unsigned *s32 = reinterpret_cast<const unsigned *>(st);
                unsigned *d32 = reinterpret_cast<unsigned *>(sn);
                for (int i = lane; i < (a.n_pad >> 2); i += GMC_WAVE) d32[i] = s32[i];
                pending = false;
                wave_sync();
            }
            // 4. apply
            gmc::apply_move<K>(g, W, st, v, st[v], k, lane);
            if (lane == 0) {
                until[v] = gmc::ban_until(it, a.tenure_base, tenure_draw);
            }
            rel = new_rel;
            ++moves;
            // 5. best so far
            if (improves) {
                best = rel;
                best_it = it + 1;
                pending = true;
            }
            wave_sync();
        }
        if (pending) {
            const unsigned *s32 = reinterpret_cast<const unsigned *>(st);
            unsigned *d32 = reinterpret_cast<unsigned *>(sn);
            for (int i = lane; i < (a.n_pad >> 2); i += GMC_WAVE) d32[i] = s32[i];
        }
    }
    best_it_out = best_it;
    moves_out = moves;
}

#if GMC_COST
#define GMC_CHAIN_NC , nc
#else
#define GMC_CHAIN_NC
#endif

template <int K>
__global__ __launch_bounds__(256) void GMC_CHAIN_KERNEL(GMC_CHAIN_ARGS a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    const int gi = blockIdx.y;
    const int r0 = a.b.goff[gi];
    const int n = a.b.goff[gi + 1] - r0;
    if (n > a.b.n_max || n < (a.first > 1 ? a.first : 1)) return;   // (the LDS is sized by n_max; workgroup-uniform)
    const int wave = gmc::uniform((int)(threadIdx.x >> 6));
    const int cand0 = blockIdx.x * a.slots;
    const int cand = cand0 + wave;
    const int e0 = a.b.rowptr[r0];
    const int nnz = a.b.rowptr[r0 + n] - e0;
#if GMC_COST
    const float *nc = a.node_cost + (long)r0 * K;   // the graph's cost rows, by local id
#endif
    // the copy is sized by n_max and nnz_max: a graph that contradicts them takes the global path
    const bool staged = a.staged && nnz >= 0 && nnz <= a.b.nnz_max;   // workgroup-uniform
    const bool runs = wave < a.slots && cand < a.cands;               // wave-uniform
    int best_it = 0, moves = 0;
    if (staged) {
        int *starts = reinterpret_cast<int *>(lds + a.off_starts);
        float *vals = a.b.vals ? reinterpret_cast<float *>(lds + a.off_vals) : nullptr;
        unsigned short *ids = reinterpret_cast<unsigned short *>(lds + a.off_ids);
        if (a.iterations > 0) {
            for (int l = threadIdx.x; l <= n; l += blockDim.x) starts[l] = a.b.rowptr[r0 + l] - e0;
            for (int e = threadIdx.x; e < nnz; e += blockDim.x) {
                ids[e] = (unsigned short)a.b.lcol[e0 + e];
                if (vals) vals[e] = a.b.vals[e0 + e];
            }
        }
        __syncthreads();
        if (runs) {
            const LdsCsr g{starts, ids, vals, nullptr, 0};
            tabu_chain<K>(a, g, lds + (size_t)wave * a.chain_bytes, n, cand, a.assign + (long)cand * a.b.R + r0,
                          best_it, moves GMC_CHAIN_NC);
        }
    } else if (runs) {
        const GlobalCsr g{a.b.rowptr + r0, a.b.lcol, a.b.vals, nullptr, r0, a.first};
        tabu_chain<K>(a, g, lds + (size_t)wave * a.chain_bytes, n, cand, a.assign + (long)cand * a.b.R + r0,
                      best_it, moves GMC_CHAIN_NC);
    }
    if (runs && gmc::lane_id() == 0) {
        if (a.best_iter) a.best_iter[(long)gi * a.cands + cand] = best_it;
        if (a.moves) a.moves[(long)gi * a.cands + cand] = moves;
    }
    __syncthreads();   // every chain of the workgroup has left its snapshot
    // the result and its score, chain by chain, the whole workgroup on each: scored as gmc_refine_local_f32 scores
    for (int s = 0; s < a.slots; ++s) {
        const int cs = cand0 + s;
        if (cs >= a.cands) break;   // workgroup-uniform
        const unsigned char *sn = lds + (size_t)s * a.chain_bytes + (size_t)a.n_pad * (K * 4 + 5);
        signed char *as = a.assign + (long)cs * a.b.R + r0;
        for (int l = threadIdx.x; l < n; l += blockDim.x) as[l] = (signed char)sn[l];
#if GMC_COST
        const float cut = gmc::block_score<K>(a.b, nc, sn, r0, n, red);   // (the cut, minus the cost: one fp32 subtraction)
#else
        const float cut = gmc::block_cut(a.b, sn, r0, n, red);
#endif
        if (threadIdx.x == 0) a.cut_all[(long)gi * a.cands + cs] = cut;
        __syncthreads();   // thread 0 has read red before the next recount writes it
    }
}
#undef GMC_CHAIN_NC
