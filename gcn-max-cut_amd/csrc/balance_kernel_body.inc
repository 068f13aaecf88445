// The chain and the kernel of gmc_kway_balance_f32 and gmc_kway_balance_c_f32 (kway_balance.hip), included once for
// each with GMC_COST defined false / true, GMC_CHAIN_ARGS the argument struct (BalanceArgs, or BalanceCostArgs = the
// same fields and node_cost) and GMC_CHAIN_KERNEL the kernel's name: tabu_kernel_body.inc's arrangement and reasons.
// balance_kernel<K>'s register allocation moves with the argument struct's layout and with where statements stand
// (DESIGN.md section 34), so the kernel without costs keeps its struct and its statements, and the cost kernel differs
// in two places only - the table starts from the node's cost row, and the snapshots are scored by gmc::block_score.

// One chain on the calling wave: the sizes, the repair, the table, the iterations, the snapshot left in sn.
// With GMC_COST, nc: the graph's cost rows by local id (node_cost + r0 * K).
template <int K, class G>
__device__ __forceinline__ void balance_chain(const GMC_CHAIN_ARGS &a, const G &g, unsigned char *lds, int n, int cand,
                                              const signed char *in, const int *lo, const int *hi, int &best_it_out,
                                              int &moves_out, int &repairs_out
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
    Sizes<K> z;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        z.sm[k] = 0u;
        const int l = lo[k] < 0 ? 0 : lo[k] > n ? n : lo[k];   // (admitted bounds have lo <= n and hi >= 0)
        const int h = hi[k] < 0 ? 0 : hi[k] > n ? n : hi[k];
        z.lh[k] = (unsigned)l | ((unsigned)h << 16);
    }
    for (int l0 = 0; l0 < n; l0 += GMC_WAVE) {   // wave-uniform trip count: the ballots below take every lane
        const int l = l0 + lane;
        unsigned c = 0xffu;
        if (l < n) {
            c = (unsigned char)in[l];
            st[l] = (unsigned char)c;
            sn[l] = (unsigned char)c;
            until[l] = 0u;
        }
#pragma unroll
        for (int k = 0; k < K; ++k) {
            z.sm[k] += (unsigned)__popcll(__ballot(c == (unsigned)k)) +
                       ((unsigned)__popcll(__ballot(c == (unsigned)k && l >= first)) << 16);
        }
    }
    int best_it = 0, moves = 0, repairs = 0;
    int V = violation<K>(z);
    if (n_mov > 0 && (a.iterations > 0 || V > 0)) {
        wave_sync();
        for (int l = lane; l < n; l += GMC_WAVE) {
#if GMC_COST
            // (+ 0.0f: a sum of -0.0 enters the table as +0.0, as in tabu_kernel_body.inc)
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
        const Chain<K, G> ch{g, W, until, st, first, n, n_mov, (n_mov + GMC_WAVE - 1) / GMC_WAVE, lane};
        // the repair: the largest gain among the moves that lower the violation, until none is left
        // (every move lowers V, so the loop ends within V <= 2 n moves whatever the bytes are)
        while (V > 0) {
            const u64 rows = repair_rows<K>(z);
            const u64 key = ch.scan(rows, rows, 0xffffffffu, 0, -1, 0.0f, 0.0f);
            const unsigned khi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key >> 32));
            const unsigned klo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key);
            if (khi == 0u && klo == 0u) break;   // (wave-uniform)
            const unsigned x = ~klo;
            const int k = (int)(x % (unsigned)K);
            const int v = first + (int)(x / (unsigned)K);
            const int c = __builtin_amdgcn_readfirstlane((int)st[v]);   // (keeps the sizes in scalar registers)
            ch.apply(v, c, k);
            resize<K>(z, c, k);
            V = violation<K>(z);
            ++repairs;
            wave_sync();
        }
        if (repairs > 0) {   // the repaired state is the base of the search
            const unsigned *s32 = reinterpret_cast<const unsigned *>(st);
            unsigned *d32 = reinterpret_cast<unsigned *>(sn);
            for (int i = lane; i < (a.n_pad >> 2); i += GMC_WAVE) d32[i] = s32[i];
            wave_sync();
        }
        float rel = 0.0f, best = 0.0f;
        bool pending = false;   // the state is better than the snapshot and not copied yet
        const unsigned span = a.tenure_span + (a.tenure_div > 0 ? (unsigned)n_mov / a.tenure_div : 0u);
        const u64 base = a.seed + GMC_GOLD * (((u64)(unsigned)cand << 32) + 1ULL);   // it < 2^32 only adds
        u64 open, free_;
        search_rows<K>(z, open, free_);
        for (int it = 0; it < a.iterations; ++it) {
            const u64 h = mix64(base + GMC_GOLD * (u64)(unsigned)it);
            const int r = (int)((unsigned)h % (unsigned)n_mov);
            const unsigned tenure_draw = (unsigned)(h >> 32) % (span + 1u);
            const u64 key = ch.scan(open, free_, (unsigned)it, r, -1, rel, best);
            const unsigned khi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key >> 32));
            const unsigned klo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key);
            if (khi == 0u && klo == 0u) continue;   // no admissible move (wave-uniform)
            const unsigned x = ~klo;
            const int k = (int)(x % (unsigned)K);
            int v = first + (int)(x / (unsigned)K) + r;
            v = v - first >= n_mov ? v - n_mov : v;
            const float gain = ordered_float(khi);
            const int c = __builtin_amdgcn_readfirstlane((int)st[v]);   // (keeps the sizes in scalar registers)
            const bool is_free = ((free_ >> (c * 8 + k)) & 1ULL) != 0ULL;   // (wave-uniform)
            const float new_rel = rel + gain;
            if (pending && !(is_free && new_rel > best)) {   // the snapshot takes the state before this move
                const unsigned *s32 = reinterpret_cast<const unsigned *>(st);
                unsigned *d32 = reinterpret_cast<unsigned *>(sn);
                for (int i = lane; i < (a.n_pad >> 2); i += GMC_WAVE) d32[i] = s32[i];
                pending = false;
                wave_sync();
            }
            const unsigned ban = gmc::ban_until(it, a.tenure_base, tenure_draw);
            ch.apply(v, c, k);
            if (lane == 0) until[v] = ban;
            rel = new_rel;
            ++moves;
            if (is_free) {
                resize<K>(z, c, k);
                search_rows<K>(z, open, free_);
            } else {
                // the counter-move: the best movable u != v of class k goes to class c, bans ignored
                wave_sync();
                const u64 back = 1ULL << (k * 8 + c);
                const u64 key2 = ch.scan(back, back, 0xffffffffu, r, v, 0.0f, 0.0f);
                const unsigned k2hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(key2 >> 32));
                const unsigned k2lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)key2);
                if (k2hi != 0u || k2lo != 0u) {   // (always, for class bytes in 0..K-1: m[k] >= 1 before v came)
                    int u = first + (int)(~k2lo / (unsigned)K) + r;
                    u = u - first >= n_mov ? u - n_mov : u;
                    ch.apply(u, k, c);
                    if (lane == 0) until[u] = ban;
                    rel = rel + ordered_float(k2hi);
                }
            }
            // 5. best so far
            if (rel > best) {
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
    repairs_out = repairs;
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
    int n;
    bool admitted;
    if (!graph_runs<K>(a.b, a.first, gi, a.size_lo, a.size_hi, n, admitted)) return;
    const int *lo = a.size_lo + (long)gi * K;
    const int *hi = a.size_hi + (long)gi * K;
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
    int best_it = 0, moves = 0, repairs = 0;
    if (staged) {
        int *starts = reinterpret_cast<int *>(lds + a.off_starts);
        float *vals = a.b.vals ? reinterpret_cast<float *>(lds + a.off_vals) : nullptr;
        unsigned short *ids = reinterpret_cast<unsigned short *>(lds + a.off_ids);
        // (staged whatever the iteration count: the repair needs the table too)
        for (int l = threadIdx.x; l <= n; l += blockDim.x) starts[l] = a.b.rowptr[r0 + l] - e0;
        for (int e = threadIdx.x; e < nnz; e += blockDim.x) {
            ids[e] = (unsigned short)a.b.lcol[e0 + e];
            if (vals) vals[e] = a.b.vals[e0 + e];
        }
        __syncthreads();
        if (runs) {
            const LdsCsr g{starts, ids, vals, nullptr, 0};
            balance_chain<K>(a, g, lds + (size_t)wave * a.chain_bytes, n, cand, a.assign + (long)cand * a.b.R + r0, lo,
                             hi, best_it, moves, repairs GMC_CHAIN_NC);
        }
    } else if (runs) {
        const GlobalCsr g{a.b.rowptr + r0, a.b.lcol, a.b.vals, nullptr, r0, a.first};
        balance_chain<K>(a, g, lds + (size_t)wave * a.chain_bytes, n, cand, a.assign + (long)cand * a.b.R + r0, lo, hi,
                         best_it, moves, repairs GMC_CHAIN_NC);
    }
    if (runs && gmc::lane_id() == 0) {
        if (a.best_iter) a.best_iter[(long)gi * a.cands + cand] = best_it;
        if (a.moves) a.moves[(long)gi * a.cands + cand] = moves;
        if (a.repairs) a.repairs[(long)gi * a.cands + cand] = repairs;
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
