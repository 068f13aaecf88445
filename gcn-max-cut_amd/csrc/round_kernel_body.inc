// The body of round_conditional_kernel<K> and round_conditional_cost_kernel<K> (round.hip), included once in each with
// GMC_COST defined false / true: does the launch have per-node class costs (a.node_cost != NULL)?  With the cost as a
// run-time pointer of the one instantiation the NULL call measured 2.5 % slower at K = 3 (DESIGN.md section 33);
// included as text the NULL kernel compiles to the instructions it had before costs existed.
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    const int g = blockIdx.x;
    const int r0 = a.b.goff[g];
    const int n = a.b.goff[g + 1] - r0;
    const int first = a.first;
    if (n > a.b.n_max || n < first) return;   // (a batch that contradicts its own n_max: the LDS is sized by it)
    float *q = reinterpret_cast<float *>(lds);
    unsigned char *cls = lds + (size_t)a.b.n_max * K * sizeof(float);
    const int *rp = a.b.rowptr + r0;
    const int *col = a.b.lcol;
    const float *vals = a.b.vals;
    // state: terminals (l < first) e_l (their rows of P are not read), every other node its row of P
    const float *Pg = a.P + (long)r0 * K;
    for (int i = threadIdx.x; i < n * K; i += blockDim.x) {
        const int l = i / K, k = i - l * K;
        q[i] = l < first ? (l == k ? 1.0f : 0.0f) : Pg[i];
    }
    for (int l = threadIdx.x; l < n; l += blockDim.x) cls[l] = (unsigned char)(l < first ? l : 0);
    __syncthreads();
    const gmc::FloatState<K> state{q};
    const float *nc = GMC_COST ? a.node_cost + (long)r0 * K : nullptr;   // the graph's cost rows, by local id
    if (a.expected) {   // workgroup-uniform
        float acc = 0.f;
        for (int l = threadIdx.x; l < n; l += blockDim.x) acc += expected_row<K>(rp, col, vals, state, l);
        acc = gmc::wave_sum(acc);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
        __syncthreads();
        if constexpr (!GMC_COST) {
            if (threadIdx.x == 0) a.expected[g] = (((red[0] + red[1]) + red[2]) + red[3]) * 0.5f;
        } else {   // the expected cost in the same order (rows per thread, wave, four waves), then one subtraction
#pragma clang fp contract(off)
            float expected = (((red[0] + red[1]) + red[2]) + red[3]) * 0.5f;
            float cacc = 0.f;
            for (int l = threadIdx.x; l < n; l += blockDim.x) cacc += gmc::expected_cost_row<K>(nc, state, l);
            cacc = gmc::wave_sum(cacc);
            __syncthreads();   // every thread has read the cut's red
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cacc;
            __syncthreads();
            const float cost = ((red[0] + red[1]) + red[2]) + red[3];
            expected = expected - cost;
            if (threadIdx.x == 0) a.expected[g] = expected;
        }
        __syncthreads();   // every row has read the unrounded state, thread 0 has read red
    }
    const int k0 = a.cgoff[g];
    const int classes = a.cgoff[g + 1] - k0 - 1;
    // rounding: one visit of every movable node, class by class
    for (int k = 0; k < classes; ++k) {
        const int hi = a.cptr[k0 + k + 1];
        for (int i = a.cptr[k0 + k] + threadIdx.x; i < hi; i += blockDim.x) {
            const int l = a.order[i] - r0;
            if ((unsigned)(l - first) >= (unsigned)(n - first)) continue;   // not a movable row: never touch LDS for it
            const Sums<K> s = state_sums<K>(rp, col, vals, state, l, nc);
            float wk;
            const int kk = smallest<K>(s, wk);
#pragma unroll
            for (int c = 0; c < K; ++c) q[l * K + c] = c == kk ? 1.0f : 0.0f;
            cls[l] = (unsigned char)kk;
        }
        __syncthreads();   // the next class, the descent or the cut count reads what this one wrote
    }
    // descent: the local search's sweeps at K classes over the class bytes
    const gmc::GlobalCsr csr{rp, col, vals, a.order, r0, first};
    const int sw = gmc::descent_sweeps<K>(csr, a.cptr, k0, classes, cls, n, a.max_descent_sweeps, nc);
    signed char *as = a.assign + r0;
    for (int l = threadIdx.x; l < n; l += blockDim.x) as[l] = (signed char)cls[l];
    float cut;   // scored as gmc_refine_local_f32 scores
    if constexpr (GMC_COST) cut = gmc::block_score<K>(a.b, nc, cls, r0, n, red);
    else cut = gmc::block_cut(a.b, cls, r0, n, red);
    if (threadIdx.x == 0) {
        a.cut[g] = cut;
        if (a.sweeps) a.sweeps[g] = sw;
    }
