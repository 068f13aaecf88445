// The body of anneal_k_kernel<K> and anneal_k_cost_kernel<K> (kway_search.hip), included once in each with GMC_COST
// defined false / true: does the launch have per-node class costs (a.node_cost != NULL)?
//
// Why a compile-time flag, and why as text: the kernel holds both accessor bodies and sits at the SGPR ceiling.  With
// the cost as a run-time pointer of the one instantiation the K = 7 and 8 kernels spilled it to scratch (36 bytes a
// lane) and the NULL call measured 1.6 % slower at K = 3; the same body as a __device__ function called from two
// kernels measured 3 to 5 % slower on the NULL call (the compiler inlines in another order and allocates otherwise);
// a template <int K, bool COST> kernel would rename anneal_k_kernel<K>, which callers of the code object look up.
// Included as text the NULL kernel compiles to the instructions it had before costs existed.  DESIGN.md section 33 and
// profiles/r28_node_cost.json have the figures.
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    __shared__ float red[4];
    __shared__ int flag;
    const int cand = blockIdx.x, gi = blockIdx.y;
    const int r0 = a.b.goff[gi];
    const int n = a.b.goff[gi + 1] - r0;
    if (n > a.b.n_max || n < a.first) return;   // (the LDS is sized by n_max; a graph without its terminals is skipped)
    float *lv = reinterpret_cast<float *>(lds);
    unsigned char *sa = lds + 4 * GMC_ANNEAL_LEVELS;
    unsigned char *sb = sa + a.n_pad;
    signed char *as = a.assign + (long)cand * a.b.R + r0;
    for (int l = threadIdx.x; l < n; l += blockDim.x) sa[l] = sb[l] = (unsigned char)as[l];
    if (a.anneal_sweeps > 0)
        for (int i = threadIdx.x; i < GMC_ANNEAL_LEVELS; i += blockDim.x) lv[i] = a.levels[i];
    const gmc::AnnealGraph q = gmc::anneal_graph(a, gi, r0, n);
    const float *nc = nullptr;   // the graph's cost rows, by local id
    if constexpr (GMC_COST) {
        // held in a vector register pair: the scalar file is full (a scalar pointer is what spilled at K = 7 and 8), the
        // vector file is a third used, and every load through the pointer has a per-lane address anyway
        unsigned long long bits = reinterpret_cast<unsigned long long>(a.node_cost + (long)r0 * K);
        asm volatile("" : "+v"(bits));
        nc = reinterpret_cast<const float *>(bits);
    }
    if (gmc::anneal_fits_lds(a, q)) {
        const LdsCsr g = gmc::anneal_stage_csr(a, q, lds);
        __syncthreads();
        gmc::anneal_body_k<K, GMC_COST>(a, g, sa, sb, lv, n, q.k0, q.classes, red, &flag, nc);
    } else {
        __syncthreads();
        const GlobalCsr g{a.b.rowptr + r0, a.b.lcol, a.b.vals, a.order, r0, a.first};
        gmc::anneal_body_k<K, GMC_COST>(a, g, sa, sb, lv, n, q.k0, q.classes, red, &flag, nc);
    }
    for (int l = threadIdx.x; l < n; l += blockDim.x) as[l] = (signed char)sa[l];
    float cut;   // scored as gmc_refine_local_f32 scores
    if constexpr (GMC_COST) cut = gmc::block_score<K>(a.b, nc, sa, r0, n, red);
    else cut = gmc::block_cut(a.b, sa, r0, n, red);
    if (threadIdx.x == 0) a.cut_all[(long)gi * a.cands + cand] = cut;
