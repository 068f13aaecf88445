/* gcnmaxcut.h - C ABI of libgcnmaxcut_hip.so (MI355X / gfx950).
 *
 * Drop-in boundary for the ONE hot path of MJavaadAkhtar/GCN-max-cut: the 2-layer
 * GraphConv forward/backward, the 3-class cut loss and the Adam update behind
 * python/Training/TrainingNeural.py.  The reference is pure Python on top of
 * dgl.nn.pytorch.GraphConv + torch; it has no FFI of its own, so these are the entry
 * points a ctypes binding inside TrainingNeural.py would call (INTEGRATION.md shows
 * the stub).  Every comment below names the reference lines an entry point replaces.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; all pointers are DEVICE (HBM) pointers
 *    unless a comment says host; the library borrows them for the duration of the call.
 *  - every function returns int: 0 ok, <0 argument/shape error (gmc_error_string),
 *    >0 a hipError_t.  Nothing throws, nothing calls exit.
 *  - all work is enqueued on the caller's stream (`gmc_stream_t` == hipStream_t);
 *    no hidden synchronisation, no internal threads, no allocation, so every call can
 *    be captured into a hipGraph.
 *  - fp32 row-major, int32 indices.  Results are bitwise reproducible run to run
 *    (fixed summation orders, no float atomics).
 */
#ifndef GCNMAXCUT_H
#define GCNMAXCUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 0.2.0.  Incompatible with 0.1.x: gmc_batch and gmc_model start with an `abi` word and gmc_batch carries the
 * overflow lists, so callers compiled against a 0.1.x header must be recompiled ("ABI versions").
 * Every entry point that takes one of the two structs checks its `abi` word and returns GMC_ERR_ABI on a
 * mismatch instead of reading a differently laid out struct. */
#define GMC_VERSION 200

typedef void *gmc_stream_t; /* hipStream_t */

enum {
    GMC_OK = 0,
    GMC_ERR_NULL = -1,        /* required pointer is NULL */
    GMC_ERR_SHAPE = -2,       /* negative / inconsistent sizes */
    GMC_ERR_CLASSES = -3,     /* number_classes != 3: override_fixed_nodes is 3-wide (TrainingNeural.py:91-93) */
    GMC_ERR_ALIGN = -4,       /* pointer / leading dimension not 16-byte aligned */
    GMC_ERR_WORKSPACE = -5,   /* workspace too small */
    GMC_ERR_GRAPH_SIZE = -6,  /* a graph has < 3 or > GMC_MAX_GRAPH_NODES nodes */
    GMC_ERR_UNSUPPORTED = -7,
    GMC_ERR_ABI = -8,         /* gmc_batch.abi / gmc_model.abi != GMC_VERSION: caller built against another header */
    GMC_ERR_LOSS = -9         /* loss_kind is not one of GMC_LOSS_* */
};

/* The loss of a graph, for its probabilities P [n,3] and Pt = override_fixed_nodes(P) (rows 0,1,2 <- e0,e1,e2 with a
 * straight-through gradient, TrainingNeural.py:87-94):
 *  GMC_LOSS_CUT           the reference's: compute_loss (:291-309,:154-176) of apply_max_to_one_hot(Pt) (:96-106),
 *                         loss = -C * cut(S), S = row-argmax of Pt;  dLoss/dP = C * A_val @ onehot(S) (straight-through).
 *  GMC_LOSS_EXPECTED_CUT  the same compute_loss (:291-309,:154-176) of Pt itself, without the one-hot step of :96-106 -
 *                         the expected cut when every node draws its class independently from its row:
 *                         loss = -C/2 * sum_u sum_{v in N(u)} w_uv (1 - Pt_u . Pt_v);  dLoss/dP_u = C * sum_{v in N(u)}
 *                         w_uv Pt_v for every row u, rows 0..2 included.  (A self-loop would count as in the dense
 *                         formula; the reference's graphs have none.)  S stays the argmax decode.
 * Both are summed in a fixed order (bitwise reproducible) and stored with one system-scope store per graph. */
enum { GMC_LOSS_CUT = 0, GMC_LOSS_EXPECTED_CUT = 1 };

#define GMC_MAX_GRAPH_NODES 4096 /* per-graph head kernel keeps [n,3] tiles in LDS */
/* Largest hidden width F (gmc_model.F, the F of every entry point below that takes one): F must be a multiple of 4
 * in 1..GMC_MAX_HIDDEN; wider models return GMC_ERR_UNSUPPORTED. */
#define GMC_MAX_HIDDEN 4096

/* A block-diagonal batch of B graphs resident in HBM.  This is the CSR form of what
 * graphExtender.process_graphs_from_folder emits per graph (graphExtender.py:102-114:
 * the DGL graph == CSR structure, the padded adjacency == `vals` on that structure).
 * Built once per dataset by the host (gcn-max-cut_amd/graph.py). */
typedef struct gmc_batch {
    int32_t abi;           /* GMC_VERSION of the header the caller was compiled against (checked) */
    int32_t B;             /* graphs in the batch */
    int32_t R;             /* total nodes = sum n_g */
    int32_t nnz;           /* total directed edges = sum 2|E_g| */
    int32_t n_max;         /* max n_g */
    int32_t uniform_n;     /* n if every graph has n nodes, else 0 (XCD grouping hint) */
    int32_t nnz_max;       /* max directed edges of one graph (sizes the LDS index cache) */
    const int32_t *goff;   /* [B+1] first row of each graph */
    const int32_t *rowptr; /* [R+1] */
    const int32_t *gcol;   /* [nnz] neighbour as batch row id  (aggregation operand) */
    const int32_t *lcol;   /* [nnz] neighbour as local node id (row of W1 / column of X) */
    const float *vals;     /* [nnz] edge weight = X[u,v], or NULL when all ones */
    const float *dinv;     /* [R] clamp(degree,1)^-1/2  (in == out degree: undirected) */
    /* Optional ELL copy of the same structure for the LDS-tiled kernels (NULL: row kernels
     * only): W = ell_width slots per row (8 or 16), the row's FIRST min(degree, W) neighbours (CSR order) as
     * local ids in the slot order gmc_ell_arrange_host chose, padded with n_g..n_g+3 (all-zero tile rows),
     * weights 0.  Neighbours beyond the W-th of a row live in the overflow lists below. */
    const uint16_t *ell;   /* [R][W] */
    const float *ell_vals; /* [R][W] or NULL when all ones */
    int32_t ell_width;
    /* leading slots of a row that can hold a neighbour: 0 or ell_width = all of them; s < ell_width = slots
     * s..ell_width-1 of EVERY row are padding (gmc_ell_arrange_host lays a batch out that way when no row has
     * more than s neighbours, gmc_ell_slots_for tells s) - the LDS-tiled kernels then neither read nor add
     * those slots: 7 of 8 for d = 7 regular graphs (the headline workload), 12 of 16 for d = 12. */
    int32_t ell_slots;
    /* Overflow lists (NULL: no row of the batch has more than ell_width neighbours): the neighbours of row r
     * beyond its first ell_width, CSR order, in blocks of 8 local ids - blocks ovf_ptr[r] .. ovf_ptr[r+1]-1,
     * i.e. ids ovf_ids[8*ovf_ptr[r] ..), the last block of a row padded with n_g (weight 0).  A row with a
     * hub's degree then costs its own extra blocks (gathered by the wave that owns the row) instead of moving
     * the whole batch to the row kernels.  Summation order of a row: fixed (ELL slots and block entries dealt
     * over the lanes of a wave, then a butterfly), bitwise reproducible.  ovf_ptr with ovf_max_blocks == 0 (or
     * ovf_ids == NULL) is a batch without lists. */
    const int32_t *ovf_ptr;   /* [R+1] in blocks, or NULL */
    const uint16_t *ovf_ids;  /* [8 * ovf_ptr[R]] */
    const float *ovf_vals;    /* [8 * ovf_ptr[R]] or NULL when all ones */
    /* largest number of overflow blocks one graph of the batch has (host-known: the pointers above are device memory).
     * The fused LDS kernels keep a graph's blocks and one 16-bit descriptor per row in the few KB of LDS their tiles
     * leave over - at most 15 blocks per row, and as many per graph as fit (51 at n = 1000 with a 16-slot table, more
     * for smaller graphs); a batch beyond that, or one with edge weights AND overflow lists, runs on the row kernels. */
    int32_t ovf_max_blocks;
} gmc_batch;

/* GCNSoftmax parameters in DGL GraphConv layout (TrainingNeural.py:72-77):
 * conv1.weight [N,F], conv1.bias [F], conv2.weight [F,K], conv2.bias [K].  F: a multiple of 4, at most
 * GMC_MAX_HIDDEN (callers pad a hidden width that is not: gcn-max-cut_amd/engine.py). */
typedef struct gmc_model {
    int32_t abi;   /* GMC_VERSION of the header the caller was compiled against (checked) */
    int32_t N, F, K;
    int32_t flags; /* GMC_MODEL_* bits, 0 by default */
    const float *W1, *b1, *W2, *b2;
    /* F.dropout(h, p, training) between the layers (TrainingNeural.py:82; TrainingConfig.dropout :43).
     * 0 = identity: eval mode, and every reference configuration.  With p in (0,1) the entry points that
     * take a gmc_model apply H <- H o mask / (1-p) after relu, mask from a counter-based hash of
     * (dropout_seed, row, column) - reproducible from the seed, not torch's random stream - and run the
     * one-kernel-per-operation sequence.  gmc_backward_from_gp must be given the same p (and the workspace)
     * as the gmc_forward that produced P.  gmc_train_step_f32 has no dropout (it builds its own model). */
    float dropout_p;
    uint32_t dropout_seed_lo, dropout_seed_hi;
    /* Optional (NULL = not used): a copy of conv1.weight in the slab layout [ceil(F/16)][N][16] (element (r, c) at
     * ((c/16)*N + r)*16 + c%16, pad columns zero; gmc_w1_slab_floats floats).  The fused layer-1 forward streams the
     * 16 W1 columns of a slice into LDS per (graph, slice): from this copy a wave's LDS-DMA instruction reads one
     * contiguous KiB, from the [N,F] layout sixteen 64-byte pieces (8 % of the kernel's time).  The CALLER keeps
     * it equal to W1: gmc_w1_slab_f32 builds it; gmc_train_step_f32 and gmc_adam_devstep_model_f32 write the
     * updated W1 to both.  Results do not depend on it (same values, same order of operations). */
    const float *W1_slab;
} gmc_model;
/* gmc_train_fwd_bwd: grad has ONE more float after the N*F + F + F*3 + 3 gradient entries and
 * receives the sum of the batch's per-graph losses there (loss must be non-NULL).  Lets a
 * data-parallel caller carry the step's loss (TrainingNeural.py:387-388) through the gradient
 * all-reduce instead of a second collective. */
#define GMC_MODEL_GRAD_TAIL 1
/* gmc_forward, gmc_train_fwd_bwd and gmc_forward_features: the loss (and, training, its gradient) is
 * GMC_LOSS_EXPECTED_CUT instead of GMC_LOSS_CUT (compute_loss on override_fixed_nodes(P), TrainingNeural.py:291-309
 * on :87-94, without :96-106). */
#define GMC_MODEL_LOSS_EXPECTED 2

int gmc_version(void);
const char *gmc_error_string(int code);

/* HOST helper (all pointers are host pointers): fills the ELL neighbour table of a batch from
 * its CSR.  Inside each group of four rows that share an LDS cycle of the tiled kernels the
 * neighbours are ordered over the W slots so that a slot's four fetches fall into different LDS
 * bank quarters where possible; padding entries are n_g .. n_g+3 (four all-zero tile rows).
 * The slot order is the summation order of the LDS-tiled kernels (fixed per batch).  When no row of the
 * batch is longer than s = gmc_ell_slots_for(...) < W the neighbours are arranged over slots 0..s-1 and slots
 * s..W-1 of every row are padding: set gmc_batch.ell_slots = s for such a batch.  Of a row longer than W
 * the first W neighbours (CSR order) are placed; the caller puts the rest into the overflow lists. */
int gmc_ell_arrange_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol,
                         const float *vals, int32_t W, uint16_t *ell, float *ell_vals);
/* the slots gmc_ell_arrange_host uses for a batch with R rows (host pointer): the largest row length,
 * at least 7 (W = 8) / 9 (W = 16), at most W */
int gmc_ell_slots_for(int32_t R, const int32_t *rowptr, int32_t W);

/* Kernel tags reported by the timing probe (one per launch of the fused step). */
enum {
    GMC_K_GATHER_W1 = 0,  /* (X o dinv) @ W1 as a row gather of W1          TrainingNeural.py:80 */
    GMC_K_AGG_FWD = 1,    /* layer-1 aggregation + b1 + relu (+ fused H@W2)  :80-83; gmc_att_*: the attention aggregation */
    GMC_K_HEAD = 2,       /* per-graph [n,3] head: softmax, decode, loss, GY2 :83-106,:154-176 */
    GMC_K_HIDDEN_BWD = 3, /* dW2/db1 partials + Gs                           backward of :81-83 (gmc_att_*: two records, the
                           * row scaling of GY2 in front of it) */
    GMC_K_COLSUM = 4,     /* fold of the partials, db2 (gmc_att_*: three records, the partials of da_src / da_dst and their
                           * fold behind it) */
    GMC_K_AGG_BWD = 5,    /* conv1 backward aggregation                      backward of :80 (gmc_att_*: two records, the
                           * edge backward, then the transposed aggregation) */
    GMC_K_DW1 = 6,        /* dW1 gather-reduce over graphs */
    GMC_K_DW1_FOLD = 7,   /* fold of the dW1 chunk partials */
    GMC_K_ADAM = 8,       /* fused Adam                                      :386 */
    GMC_K_SPMM_USER = 9,  /* gmc_spmm_f32 called directly */
    GMC_K_DENSE_MFMA = 10, /* the stand-alone H @ W2 product: gmc_dense_hw2_f32, and hw2_k of the K-class sequence; gmc_att_*:
                            * two records, the attention scores (row dot products) and H @ W2 */
    GMC_K_BWD1_FUSED = 11, /* hidden backward + conv1 backward aggregation + dW1, one pass over H (a one-graph
                            * gmc_train_step_f32 computes the head in this launch as well: no GMC_K_HEAD record) */
    GMC_K_FWD1_FUSED = 12, /* W1 gather + layer-1 aggregation (+ fused H@W2), one kernel */
    GMC_K_DECODE = 13,     /* post-processing sampler + cut count */
    GMC_K_FINISH = 14,     /* fold of the gradient partials (+ fused Adam) over the flat buffer */
    GMC_K_REFINE = 15,     /* local search over decoded candidates + cut count (gmc_refine_local_f32); also the
                            * rounding by conditional expectations + descent (gmc_round_conditional_f32), and one
                            * record per call of gmc_large_round_conditional_f32 / gmc_large_local_search_f32 /
                            * gmc_large_anneal_f32 */
    GMC_K_ANNEAL = 16,     /* annealing + descent over decoded candidates + cut count (gmc_refine_anneal_f32,
                            * gmc_kway_refine_anneal_f32) */
    GMC_K_GEMM = 17,       /* dense fp32 GEMM on the matrix cores (gmc_gemm_f32; the dense-feature path) */
    GMC_K_SAMPLE = 18,     /* seeded post-processing sampler + cut count (gmc_decode_sample_seeded_f32,
                            * gmc_kway_decode_sample_seeded_f32; one record per call of gmc_large_sample_seeded_f32) */
    GMC_K_COUNT = 19
};

/* Timing probe for bench.py: between gmc_probe_begin and gmc_probe_end every kernel launch
 * of this library is bracketed by hipEventRecord on the stream it is launched on.
 * gmc_probe_end synchronises on the last event and returns the number of launches seen,
 * writing up to `max` (tag, milliseconds) pairs (host pointers). */
/* Kernel-sequence option: 1 (default) = fused layer kernels (T0 / Gs / U never leave LDS);
 * 0 = one kernel per operation (stand-alone SpMM, hidden backward, dW1).  Same results to
 * rounding.  Returns the previous setting.  Workspace sizes do not depend on it. */
int gmc_set_fuse(int on);

int gmc_probe_begin(int32_t capacity);
int gmc_probe_end(int32_t *tags, float *ms, int32_t max);
/* Valid after gmc_probe_end: the flavour word (below) of each recorded launch, 0 for a kernel that is not one of the
 * LDS-tiled families.  Writes up to `max` words (host pointer), returns the number of launches recorded. */
int gmc_probe_flavours(int32_t *words, int32_t max);

/* Flavour words: WHICH instantiation of an LDS-tiled kernel family a launch runs (the host picks one per batch
 * from n_max, the table width, the live slots, edge weights and overflow lists).  Bit fields of a non-negative int32: */
#define GMC_FLV_KERNEL(w) ((w) & 0x7)          /* family: GMC_FLV_FWD1 .. GMC_FLV_DW1 */
#define GMC_FLV_FS(w) (((w) >> 3) & 0x7f)      /* columns per slice: 16, 32, 64 */
#define GMC_FLV_W(w) (((w) >> 10) & 0x1f)      /* neighbour slots per row of the table: 8, 16 */
#define GMC_FLV_ACC(w) (((w) >> 15) & 0xf)     /* rows per thread: 4, 8 */
#define GMC_FLV_NS(w) (((w) >> 19) & 0x1f)     /* live slots the gathers read: 7, 8, 10, 12, 14, 16 */
#define GMC_FLV_HAS_VAL(w) (((w) >> 24) & 1)   /* edge weights */
#define GMC_FLV_OVF(w) (((w) >> 25) & 1)       /* overflow lists (hub rows) */
#define GMC_FLV_HEAD(w) (((w) >> 26) & 1)      /* bwd1_reg: the one-graph head runs inside the backward */
#define GMC_FLV_EPI(w) (((w) >> 27) & 1)       /* spmm_lds: fused (Y o scale) @ W2 epilogue */
#define GMC_FLV_SHARED(w) (((w) >> 28) & 1)    /* spmm_lds: one shared source table (the W1 row gather) */
#define GMC_FLV_PER(w) (1 << (((w) >> 29) & 3)) /* fwd1 / spmm_lds: column slices per workgroup item (1, 2, 4, 8) */
#define GMC_FLV_PER_MASK (3 << 29)             /* (not a template argument: it changes how the W2 partials fold) */
enum {
    GMC_FLV_FWD1 = 1,      /* fwd1_lds_kernel<FS, W, ACC, HAS_VAL, NS, OVF>: the fused layer-1 forward */
    GMC_FLV_BWD1 = 2,      /* bwd1_lds_kernel<FS, W, ACC, HAS_VAL, NS, OVF>: the fused backward, 16-slot tables */
    GMC_FLV_BWD1_REG = 3,  /* bwd1_reg_kernel<FS, ACC, HAS_VAL, NS, OVF, HEAD>: the fused backward, 8-slot tables */
    GMC_FLV_SPMM = 4,      /* spmm_lds_kernel<FS, W, ACC, EPI, HAS_VAL, SHARED, NS>: one-kernel-per-operation SpMM */
    GMC_FLV_DW1 = 5        /* dw1_lds_kernel<FS, W, ACC, HAS_VAL, NS>: one-kernel-per-operation dW1 gather */
};
/* HOST query (no HIP call; the batch's pointers are only tested against NULL): the flavour words of the LDS-tiled
 * launches a training step of this batch with hidden width F makes, in launch order - first the fused sequence
 * (fwd1, then bwd1; one_graph_step != 0: as gmc_train_step_f32 runs it, which computes a one-graph batch's head
 * inside the backward), then the one-kernel-per-operation sequence of gmc_set_fuse(0) (W1 gather, aggregation with
 * the W2 epilogue, backward aggregation, dW1), the latter only for batches without overflow lists.  Returns the
 * number of words (writes up to `max`), 0 when the batch takes the row kernels, <0 on bad arguments (F not a
 * multiple of 4 in 1..GMC_MAX_HIDDEN: GMC_ERR_SHAPE).  Wider F is a runtime slice count of the same kernels: every
 * word for F > 1024 is, with GMC_FLV_PER cleared, one that F = 1024 gives for the same batch. */
int gmc_lds_flavours(const gmc_batch *batch, int32_t F, int32_t one_graph_step, int32_t *words, int32_t max);

/* ---- building blocks (each is also used by the fused entry points below) ---------- */

/* Y[r,:] = act( scale[r] * sum_{e in row r} vals[e] * X[col[e],:] + bias ),  r < n_rows.
 * One CSR SpMM serves: the X@W1 row-gather (col=lcol, X=W1), DGL's update_all(copy_u,sum)
 * of GraphConv layer 1 (col=gcol, + bias + relu; TrainingNeural.py:80-81) and both
 * F-wide aggregations of its autograd backward (:385).  vals/scale/bias may be NULL.
 * group_rows > 0 asks for XCD-grouped scheduling: consecutive runs of that many rows
 * (one graph) are processed by workgroups of one XCD so neighbour rows are L2 hits.
 * If W2/Z0 are non-NULL (K must be 3) the layer-2 feature transform is fused into the
 * epilogue: Z0[r,:] = scale[r] * (Y[r,:] @ W2)   ((H*outdeg^-1/2)@W2, :83).
 * Any F >= 1; the 16-byte vector kernels serve F % 4 == 0 up to GMC_MAX_HIDDEN (wider or unaligned F without W2:
 * one column per lane; with W2: GMC_ERR_UNSUPPORTED). */
int gmc_spmm_f32(const int32_t *rowptr, const int32_t *col, const float *vals,
                 const float *scale, const float *X, int64_t ldx, const float *bias, int relu,
                 float *Y, int64_t ldy, int32_t n_rows, int32_t F, int32_t group_rows,
                 const float *W2, float *Z0, gmc_stream_t stream);

/* Z0[r,:] = dinv[r] * (H[r,:] @ W2), K == 3, on the matrix cores (v_mfma_f32_16x16x4_f32).
 * Stand-alone form of the only dense contraction on the path (TrainingNeural.py:83). */
int gmc_dense_hw2_f32(const float *H, int64_t ldh, const float *dinv, const float *W2,
                      float *Z0, int32_t n_rows, int32_t F, gmc_stream_t stream);

/* C[M,Nc] = scale o (op(A) @ op(B)) in exact fp32 on the matrix cores (v_mfma_f32_16x16x4_f32); ta / tb: 0 = the
 * operand as stored (A [M,K], B [K,Nc]), 1 = stored transposed (A [K,M], B [Nc,K]); all row-major with leading
 * dimensions; scale [M] or NULL.  The forms NN, TN and NT exist (ta = tb = 1: GMC_ERR_UNSUPPORTED) - the three dense
 * products of GraphConv layer 1 with features that are not the padded adjacency (TrainingNeural.py:80 and its
 * backward): T0 = dinv o (X @ W1), dW1 = X^T @ U, dX = U @ W1^T.  Any M, Nc, K >= 0 (M or Nc == 0 launches nothing);
 * A, B, C 16-byte aligned and lda, ldb, ldc multiples of 4, else GMC_ERR_ALIGN.  k is summed in ascending order by one
 * workgroup per 64 x 64 output tile: no atomics, bitwise reproducible. */
int gmc_gemm_f32(int32_t ta, int32_t tb, int32_t M, int32_t Nc, int32_t K, const float *A, int64_t lda,
                 const float *B, int64_t ldb, const float *scale, float *C, int64_t ldc, gmc_stream_t stream);

/* Per-graph head: Z = dinv * (A @ Z0) + b2, P = softmax(Z) (TrainingNeural.py:83-84);
 * rows 0,1,2 forced to e0,e1,e2 and S = row-argmax, first max wins (:87-106);
 * loss[g] = -C * cut(S) (:154-176,:291-309).  When GY2 != NULL also the start of
 * loss.backward(): GP = C*A_val@onehot(S), softmax backward, db2part[g,:] = colsum(GZ),
 * GY2 = A @ (dinv*GZ).  P [R,3], S [R], loss [B], db2part [B,3], GY2 [R,4] = (GY2[r,0..2], dinv[r])
 * (16-byte rows so the backward kernels fetch a row's constants with one aligned load).
 * Z0 is [z_parts][R][3]: partial products of the LDS-tiled layer-1 kernel (one per column
 * slice group), folded here in ascending order; z_parts = 1 for a plain [R,3] Z0. */
int gmc_head_f32(const gmc_batch *batch, const float *Z0, int32_t z_parts, const float *b2, float C,
                 float *P, int32_t *S, float *loss, float *GY2, float *db2part, gmc_stream_t stream);

/* gmc_head_f32 with the loss chosen by loss_kind (GMC_LOSS_*; gmc_head_f32 is this call with GMC_LOSS_CUT).  With
 * GMC_LOSS_EXPECTED_CUT loss[g] and the GP behind GY2 / db2part are those of compute_loss(override_fixed_nodes(P))
 * (TrainingNeural.py:291-309,:154-176 on :87-94); P and S are what gmc_head_f32 gives, bit for bit.  An unknown
 * loss_kind returns GMC_ERR_LOSS before anything else is looked at. */
int gmc_head_loss_f32(const gmc_batch *batch, const float *Z0, int32_t z_parts, const float *b2, float C,
                      int32_t loss_kind, float *P, int32_t *S, float *loss, float *GY2, float *db2part,
                      gmc_stream_t stream);

/* The loss alone, for given probabilities P [R,3] (the output of gmc_forward / gmc_forward_features, or any caller's):
 * loss[g] (device or pinned host memory, [B]) and, when GP != NULL, GP [R,3] = dLoss/dP as defined at GMC_LOSS_*
 * (for GMC_LOSS_CUT the straight-through C * A_val @ onehot(S) of TrainingNeural.py:96-106 + :291-309; for
 * GMC_LOSS_EXPECTED_CUT the exact gradient up to the straight-through override of :87-94).  O(edges): one workgroup
 * per graph walks the neighbour table, overflow lists or CSR rows as the head does, the rows held in LDS - what a
 * caller of gmc_backward_from_gp / gmc_backward_features_from_gp needs instead of the dense [n,1000] products of
 * :154-176.  Errors, all found before any HIP call: loss_kind GMC_ERR_LOSS, a NULL batch / P / loss GMC_ERR_NULL,
 * batch->abi GMC_ERR_ABI, sizes GMC_ERR_SHAPE, n_max GMC_ERR_GRAPH_SIZE.  B == 0 launches nothing. */
int gmc_cut_loss_f32(const gmc_batch *batch, const float *P, float C, int32_t loss_kind, float *loss, float *GP,
                     gmc_stream_t stream);

/* torch.optim.Adam.step (TrainingNeural.py:337,:386) over one flat buffer, fused:
 * m,v update + bias correction + parameter update in a single sweep. step >= 1.  The
 * hyper-parameters are doubles because torch derives 1-beta, lr/bias_correction1 and
 * sqrt(bias_correction2) in Python floats (doubles) before rounding them to fp32. */
int gmc_adam_f32(float *param, const float *grad, float *m, float *v, int64_t count, double lr,
                 double beta1, double beta2, double eps, int32_t step, gmc_stream_t stream);

/* Same update with the step number kept in device memory (*step_counter = steps done so far;
 * the call uses step_counter+1 and then increments it on the stream).  All arguments are
 * replay-invariant, so a whole epoch of the reference's one-step-per-graph schedule
 * (TrainingNeural.py:371-386) can be captured once into a hipGraph and replayed. */
int gmc_adam_devstep_f32(float *param, const float *grad, float *m, float *v, int64_t count, double lr,
                         double beta1, double beta2, double eps, int32_t *step_counter,
                         gmc_stream_t stream);

/* gmc_adam_devstep_f32 over the flat [W1 | b1 | W2 | b2] buffer of an N x F x 3 model; w1_slab (NULL = none)
 * receives the updated conv1.weight in the layout of gmc_model.W1_slab. */
int gmc_adam_devstep_model_f32(float *param, const float *grad, float *m, float *v, int32_t N, int32_t F,
                               float *w1_slab, double lr, double beta1, double beta2, double eps,
                               int32_t *step_counter, gmc_stream_t stream);

/* floats of, and the launch that builds, the slab copy of conv1.weight [N,F] described at gmc_model.W1_slab
 * (no counterpart in the reference: a layout the LDS-DMA of the fused forward reads in whole KiB pieces) */
size_t gmc_w1_slab_floats(int32_t N, int32_t F);
int gmc_w1_slab_f32(const float *W1, int32_t N, int32_t F, float *slab, gmc_stream_t stream);

/* ---- fused entry points ------------------------------------------------------------ */

/* Argument checks of gmc_forward, gmc_train_fwd_bwd, gmc_train_step_loss_f32, gmc_backward_from_gp, gmc_forward_features
 * and gmc_backward_features_from_gp: all before any HIP call, in this order - the first thing wrong decides the code.
 *  1. the struct pointers, and X of the *_features calls                                   GMC_ERR_NULL
 *  2. the structs: abi (GMC_ERR_ABI, before any other field is read), required pointer fields (NULL), K (CLASSES),
 *     sizes (SHAPE), F (UNSUPPORTED), dropout_p (SHAPE), W1_slab (ALIGN), n_max (GRAPH_SIZE; > N without X: SHAPE)
 *  3. the features: ldx < N (SHAPE), then X, ldx % 4, W1                                   GMC_ERR_ALIGN
 *  4. workspace and the output pointers P, GP, grad                                        GMC_ERR_NULL
 *  5. lddx < N (SHAPE), then grad, dX, lddx % 4                                            GMC_ERR_ALIGN
 *  6. the workspace size                                                                   GMC_ERR_WORKSPACE
 * gmc_train_step_loss_f32 looks at loss_kind (GMC_ERR_LOSS), then at param, grad, m, v, step_counter (NULL, ALIGN)
 * before all of that: the model of step 2 is made of them.  gmc_train_fwd_bwd with GMC_MODEL_GRAD_TAIL checks last that
 * loss is there (NULL).  The two size queries return 0 for a NULL struct or one whose abi word differs. */

/* `loss` of the entry points below may be device memory or PINNED HOST memory mapped into the device: each
 * graph's value is written with one system-scope store as soon as it is final (by the loss kernel, before the
 * backward kernels of the same call run), so a host thread watching that memory has the step's loss while the
 * rest of the step is still executing - the reference reads loss.item() every step (TrainingNeural.py:387-388).
 * gmc_host_device_pointer: the device-side address of such memory (hipHostGetDevicePointer; > 0 = hipError_t). */
int gmc_host_device_pointer(void *pinned_host, void **device_ptr);
/* n device floats -> pinned host memory (device-side address), one system-scope store each: how a data-parallel
 * rank hands the all-reduced loss of a step (the slot after the gradient, GMC_MODEL_GRAD_TAIL) to its host
 * thread before the optimizer kernels of that step run. */
int gmc_publish_f32(const float *src, int32_t n, float *pinned_dst, gmc_stream_t stream);

/* gmc_publish_f32 + gmc_adam_devstep_model_f32 as TWO launches instead of three: one wave stores the loss values and
 * advances *step_counter, the Adam sweep behind it uses the counter as it then stands (no trailing one-thread launch).
 * The tail of a data-parallel rank's step after the gradient all-reduce (TrainingNeural.py:386-388 on N GPUs). */
int gmc_publish_adam_devstep_model_f32(const float *publish_src, int32_t publish_n, float *pinned_dst, float *param,
                                       const float *grad, float *m, float *v, int32_t N, int32_t F, float *w1_slab,
                                       double lr, double beta1, double beta2, double eps, int32_t *step_counter,
                                       gmc_stream_t stream);

/* bytes of scratch gmc_forward / gmc_train_fwd_bwd need for this batch and model (64-bit sizes: R * F may exceed
 * 2^31 elements) */
size_t gmc_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training);

/* GCNSoftmax.forward for every graph of the batch (TrainingNeural.py:79-85):
 * P[R,3] = softmax(conv2(relu(conv1(A_pad)))).  If S/loss are non-NULL also the decode
 * and loss of evaluate_model (:555-561). */
int gmc_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream);

/* forward + loss + loss.backward() of train_single_epoch's loop body (:373-385) for the
 * SUM of the batch's per-graph losses.  grad is the flat [W1 | b1 | W2 | b2] buffer
 * (N*F + F + F*3 + 3 floats) and is overwritten (rows of dW1 no graph reaches are 0). */
int gmc_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                      size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad,
                      gmc_stream_t stream);

/* One whole optimizer step of train_single_epoch's loop body (:373-386) for the batch:
 * gmc_train_fwd_bwd followed by Adam, with the gradient fold and the Adam update fused into
 * one sweep over the flat buffers (param/grad/m/v, each N*F + F + F*3 + 3 floats, 16-byte
 * aligned).  The step number lives in device memory as for gmc_adam_devstep_f32, so the call is
 * replay-invariant (hipGraph).  Single-GPU form: with data parallelism the all-reduce has to
 * sit between the gradient and Adam (gmc_train_fwd_bwd + all-reduce + gmc_adam_*).
 * w1_slab (NULL = none): the slab copy of conv1.weight (gmc_model.W1_slab), equal to it on entry; the forward
 * reads it and the Adam sweep writes the updated weights to it as well, so it stays equal. */
int gmc_train_step_f32(const gmc_batch *batch, int32_t N, int32_t F, float *param, float C, void *workspace,
                       size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad, float *m,
                       float *v, double lr, double beta1, double beta2, double eps, int32_t *step_counter,
                       float *w1_slab, gmc_stream_t stream);

/* gmc_train_step_f32 with the loss chosen by loss_kind (GMC_LOSS_*; gmc_train_step_f32 is this call with
 * GMC_LOSS_CUT), as replay-invariant.  With GMC_LOSS_EXPECTED_CUT the step descends compute_loss on
 * override_fixed_nodes(P) (TrainingNeural.py:291-309 on :87-94, without :96-106); a one-graph batch then runs the
 * stand-alone head launch (the head inside the backward launch is GMC_LOSS_CUT only).  An unknown loss_kind returns
 * GMC_ERR_LOSS before anything else is looked at. */
int gmc_train_step_loss_f32(const gmc_batch *batch, int32_t N, int32_t F, float *param, float C, int32_t loss_kind,
                            void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad,
                            float *m, float *v, double lr, double beta1, double beta2, double eps,
                            int32_t *step_counter, float *w1_slab, gmc_stream_t stream);

/* Backward for a caller-supplied dLoss/dP (autograd.Function path: callers that build
 * their own loss from GCNSoftmax.forward's output, e.g. the reference's
 * override_fixed_nodes/apply_max_to_one_hot/compute_loss chain).  Requires the
 * workspace of the gmc_forward/gmc_train_fwd_bwd call that produced P. */
int gmc_backward_from_gp(const gmc_batch *batch, const gmc_model *model, void *workspace,
                         size_t workspace_bytes, const float *P, const float *GP, float *grad,
                         gmc_stream_t stream);

/* ---- features that are not the padded adjacency (learned node embeddings: net(g, embed.weight)) --------------------
 *
 * X [R, N] (leading dimension ldx >= N, a multiple of 4; 16-byte aligned): the feature rows of the batch's graphs
 * stacked in batch row order, N = model->N.  Layer 1's feature transform is then a dense GEMM (gmc_gemm_f32) instead of
 * the row gather of W1, and layer 1 ignores batch->vals (DGL's aggregation is structure-only; only the head's cut reads
 * edge weights).  Everything else is the one-kernel-per-operation sequence on row-major [R, F] buffers, dropout
 * (model->dropout_p) included.  A graph may have more nodes than N here.  Workspace: gmc_workspace_bytes_features
 * (NOT gmc_workspace_bytes: the two plans differ). */
size_t gmc_workspace_bytes_features(const gmc_batch *batch, const gmc_model *model, int training);

/* GCNSoftmax.forward(g, X) for every graph of the batch (TrainingNeural.py:79-85); S / loss as for gmc_forward.
 * Errors, all found before any HIP call: a NULL required pointer GMC_ERR_NULL, the structs' abi GMC_ERR_ABI, sizes
 * (ldx < N included) GMC_ERR_SHAPE, X or ldx GMC_ERR_ALIGN, GMC_ERR_WORKSPACE.  R == 0 launches nothing. */
int gmc_forward_features(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx, float C,
                         void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                         gmc_stream_t stream);

/* Backward of gmc_forward_features for a caller-supplied dLoss/dP: grad as for gmc_backward_from_gp (dW1 = X^T @ U is
 * written straight into it), dX [R, N] (leading dimension lddx, as ldx; NULL: not computed) = U @ W1^T.  Requires the
 * (training-sized) workspace, the X and the dropout (p, seed) of the gmc_forward_features call that produced P.
 * R == 0 launches nothing but the zeroing of grad. */
int gmc_backward_features_from_gp(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx,
                                  void *workspace, size_t workspace_bytes, const float *P, const float *GP,
                                  float *grad, float *dX, int64_t lddx, gmc_stream_t stream);

/* ---- number_classes K other than 3 (2 <= K <= GMC_KWAY_MAX_CLASSES) ---------------------------------------------------
 *
 * The entry points above are the reference's 3-class model and answer GMC_ERR_CLASSES for any other model->K.  These
 * three run the same 2-layer GraphConv with conv2.weight [F,K], conv2.bias [K] and a softmax over K columns
 * (TrainingNeural.py:72-85 with number_classes = K, :515-535 train_multi_class), K = model->K:
 *  - terminals: nodes 0..K-1 of every graph are fixed to classes 0..K-1 - override_fixed_nodes (:87-94) with eye(K) on the
 *    first K rows, same straight-through form; every graph needs at least K nodes (n_max < K: GMC_ERR_GRAPH_SIZE; a
 *    smaller graph inside a batch is the caller's to refuse: goff is device memory);
 *  - GMC_LOSS_CUT: loss = -C * cut(S), S = row-argmax (first maximum wins) with rows 0..K-1 forced to their own class,
 *    dLoss/dP = C * A_val @ onehot_K(S) on every row; GMC_LOSS_EXPECTED_CUT (GMC_MODEL_LOSS_EXPECTED in model->flags):
 *    as defined at GMC_LOSS_*, Pt = P with rows 0..K-1 replaced by e_0..e_{K-1}.  At K = 3 both are the definitions above.
 * Kernel sequence: one kernel per operation on row-major [R, ld] buffers (the plan of the *_features calls), the
 * class-count-free kernels shared with it, the K-wide ones from csrc/kway.hip; gmc_set_fuse does not matter.  The head
 * keeps a graph's [n,K] tiles in LDS: about (2K+1)(n_max+4) floats, GMC_ERR_GRAPH_SIZE beyond a CU's 160 KiB (K = 8: n_max
 * near 2400; K = 2: GMC_MAX_GRAPH_NODES).  No dropout (dropout_p > 0: GMC_ERR_UNSUPPORTED), W1_slab is not read.
 * P [R,K] and model->W2 must be 16-byte aligned (GMC_ERR_ALIGN, with grad).  Argument checks: the order documented
 * above for the fused entry points, with K outside 2..GMC_KWAY_MAX_CLASSES as step 2's GMC_ERR_CLASSES and dropout_p > 0
 * (UNSUPPORTED) behind the dropout_p range check.  Results are bitwise reproducible; K = 3 is allowed and agrees with
 * the entry points above to rounding (another kernel sequence). */
#define GMC_KWAY_MAX_CLASSES 8
/* bytes of scratch gmc_kway_forward / gmc_kway_train_fwd_bwd need (0 for a NULL struct, another abi word, or K outside
 * 2..GMC_KWAY_MAX_CLASSES) */
size_t gmc_kway_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training);
/* gmc_forward for K classes: P [R,K]; S [R] / loss [B] optional.  An empty batch returns GMC_OK without a launch. */
int gmc_kway_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace, size_t workspace_bytes,
                     float *P, int32_t *S, float *loss, gmc_stream_t stream);
/* gmc_train_fwd_bwd for K classes: grad is the flat [W1 | b1 | W2 | b2] buffer of N*F + F + F*K + K floats, plus the
 * tail slot with GMC_MODEL_GRAD_TAIL (loss must then be non-NULL).  An empty batch zeroes grad (and the tail slot)
 * without any other launch. */
int gmc_kway_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                           size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad, gmc_stream_t stream);

/* ---- graphs beyond GMC_MAX_GRAPH_NODES (extension: up to GMC_LARGE_MAX_GRAPH_NODES nodes per graph) -------------------
 *
 * Every entry point above keeps one graph's head in one workgroup with the graph's [n,K] state in LDS, which is what
 * GMC_MAX_GRAPH_NODES (and, for gmc_kway_*, the LDS bound near n_max = 2400 at K = 8) stands for.  These run the model of
 * gmc_kway_forward / gmc_kway_train_fwd_bwd - same signatures, K = model->K in 2..GMC_KWAY_MAX_CLASSES with 3 included,
 * same terminals, both losses (GMC_MODEL_LOSS_EXPECTED in model->flags), same layouts (P [R,K], grad [W1 | b1 | W2 | b2]
 * plus the tail slot with GMC_MODEL_GRAD_TAIL), same empty-batch behaviour - on graphs of up to GMC_LARGE_MAX_GRAPH_NODES
 * nodes.  Kernel sequence: that of gmc_kway_* (one kernel per operation on row-major [R, ld] buffers) with the head
 * replaced by the four row-parallel launches of csrc/large.hip, which several workgroups share per graph: probabilities
 * and decode; loss terms, dLoss/dP and the softmax backward; the per-graph fold (loss, db2 partials); GY2 (training only).
 * Each is a GMC_K_HEAD probe record.  Summation orders (csrc/large.hip states them; all fixed, results bitwise
 * reproducible, and a graph's P, S and loss do not depend on what else is in the batch): a row's neighbours in CSR order
 * by one lane, a row of more than 64 entries by a wave (lane j takes entries j, j + 64, ..., then a butterfly over the
 * lanes); the per-graph sums over tiles of 256 rows (wave butterfly, waves ascending), then over the tiles ascending.
 * So they agree with gmc_kway_* (and at K = 3 with gmc_*) to rounding, not to the bit.
 * No dropout (dropout_p > 0: GMC_ERR_UNSUPPORTED), W1_slab is not read.  P and model->W2 must be 16-byte aligned.
 * Argument checks: the order of gmc_kway_*, whose graph-size step here is n_max < K or n_max >
 * GMC_LARGE_MAX_GRAPH_NODES (no LDS condition).  The workspace is that of gmc_kway_* plus S [R], dinv o GZ [R,K]
 * (training) and the head's tile partials [R / 256 + B + 1][K + 1]. */
#define GMC_LARGE_MAX_GRAPH_NODES (1 << 20)
/* bytes of scratch gmc_large_forward / gmc_large_train_fwd_bwd need (0 for a NULL struct, another abi word, or K outside
 * 2..GMC_KWAY_MAX_CLASSES) */
size_t gmc_large_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training);
int gmc_large_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace, size_t workspace_bytes,
                      float *P, int32_t *S, float *loss, gmc_stream_t stream);
int gmc_large_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                            size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad, gmc_stream_t stream);
/* 1 when the model's ordinary entry points - gmc_* at model->K == 3, gmc_kway_* otherwise - would answer
 * GMC_ERR_GRAPH_SIZE for this batch because n_max is too large (beyond GMC_MAX_GRAPH_NODES, or, for gmc_kway_*, beyond what
 * the head's LDS tiles take at this K and loss), i.e. when the caller has to use gmc_large_*; 0 otherwise (an empty batch
 * included).  Negative: GMC_ERR_NULL, GMC_ERR_ABI, GMC_ERR_CLASSES (K outside 2..GMC_KWAY_MAX_CLASSES).  Host only. */
int gmc_large_required(const gmc_batch *batch, const gmc_model *model);

/* ---- the functional form of the model (extension): probabilities out, the caller's dLoss/dP in -------------------------
 *
 * The reference's own loop, P = net(g, X); loss = ...(P); loss.backward(); optimizer.step() (TrainingNeural.py:371-386),
 * for every class count and graph size of the library: K = model->K in 2..GMC_KWAY_MAX_CLASSES (3 included), graphs of
 * K..GMC_LARGE_MAX_GRAPH_NODES nodes, the padded adjacency or dense features.  gmc_backward_from_gp /
 * gmc_backward_features_from_gp above stay what they are: 3 classes, graphs of up to GMC_MAX_GRAPH_NODES nodes.
 *  - gmc_fn_forward: P [R,K] = softmax(conv2(relu(conv1(.)))) and nothing else - no terminals, loss or decode, exactly what
 *    GCNSoftmax.forward returns (:79-85).  X == NULL: the features are the padded adjacency, the kernel sequence is that of
 *    gmc_large_forward up to its head (W1 row gather, aggregation + bias + relu, H @ W2, each aggregation followed by the
 *    launch that sums rows of more than 64 entries again).  X != NULL: features X [R, N] under the conventions of
 *    gmc_forward_features (ldx >= N a multiple of 4, 16-byte aligned, layer 1 ignores batch->vals, a graph may have more
 *    nodes than N): layer 1's feature transform is gmc_gemm_f32.  The head is one row-parallel launch of
 *    csrc/functional.hip on the grid of csrc/large.hip (tiles of 256 rows, several workgroups per graph).
 *  - gmc_fn_backward: the gradient of sum(GP o P) for the caller's GP [R,K] = dLoss/dP.  It takes the workspace (and X) of
 *    the gmc_fn_forward call that produced P; the forward leaves H and Z0 there, and nothing that depends on P.  One
 *    backward per forward: the backward turns those buffers into its own scratch.
 *    GZ = P o (GP - rowsum(GP o P)) per row, dinv o GZ and the tile partials of db2 in one launch, the per-graph fold of
 *    those, GY2 = A @ (dinv o GZ), then the backward of gmc_large_train_fwd_bwd behind its head.  With X: dW1 = X^T @ U is
 *    written straight into grad and dX [R, N] (leading dimension lddx, as ldx; NULL: not computed) = U @ W1^T, both
 *    gmc_gemm_f32.  grad is the flat [W1 | b1 | W2 | b2] buffer of N*F + F + F*K + K floats; there is no tail slot
 *    (GMC_MODEL_GRAD_TAIL and GMC_MODEL_LOSS_EXPECTED are not read).  An empty batch zeroes grad and launches nothing else.
 *  - gmc_fn_cut_loss_f32: the two losses as defined for gmc_kway_* above, for given probabilities P [R,K]: loss [B] (device
 *    or pinned host memory: one system-scope store per graph) and, when GP != NULL, GP [R,K] = dLoss/dP.
 *    GMC_LOSS_CUT: loss = -C * cut(S), S the row argmax (first maximum wins), GP = C * A_val @ onehot_K(S);
 *    GMC_LOSS_EXPECTED_CUT: loss = -C/2 * sum w_uv (1 - Pt_u . Pt_v), GP = C * A_val @ Pt.  terminals = 1: nodes 0..K-1 of
 *    every graph are forced to classes 0..K-1 (rows 0..K-1 of Pt are e_0..e_{K-1}, straight-through: GP is written on
 *    every row), as everywhere in the library; n_max < K is then GMC_ERR_GRAPH_SIZE.  terminals = 0: no node is forced,
 *    Pt = P and S is the plain argmax - unconstrained max-K-cut.  Two launches: the rows' terms (a row reads its
 *    neighbours' rows of P; the hard loss takes their argmax on the fly), then the per-graph fold.
 * Summation orders (csrc/functional.hip states them; all fixed, no float atomics: results are bitwise reproducible and a
 * graph's P, loss, GP and share of the gradient's partials do not depend on what else is in the batch): a row's neighbours
 * in CSR order by one lane, a row of more than 64 entries by a wave (lane j takes entries j, j + 64, ..., then a butterfly
 * over the lanes); sums over a graph's rows by tiles of 256 rows (wave butterfly, waves ascending), then the tiles
 * ascending; the per-graph db2 partials [B,K] folded as gmc_kway_train_fwd_bwd folds them.
 * No dropout (dropout_p > 0: GMC_ERR_UNSUPPORTED), W1_slab is not read.  P, GP and model->W2 must be 16-byte aligned.
 * Argument checks, all before any HIP call, in the order documented for the fused entry points with the steps of
 * gmc_kway_*: 1. the struct pointers (NULL); 2. abi, required pointer fields, K (CLASSES), sizes (SHAPE), F (UNSUPPORTED),
 * dropout_p (SHAPE, then > 0 UNSUPPORTED), W1_slab (ALIGN), n_max < K or > GMC_LARGE_MAX_GRAPH_NODES (GRAPH_SIZE), n_max > N
 * without X (SHAPE); 3. with X: ldx < N (SHAPE), then X, ldx % 4, W1 (ALIGN); 4. workspace, P, GP, grad (NULL); 5. lddx < N
 * (SHAPE), then grad, P, GP, W2, dX, lddx % 4 (ALIGN); 6. the workspace size.  gmc_fn_cut_loss_f32: 1. batch (NULL); 2. abi,
 * goff / rowptr / gcol / lcol (NULL), K (CLASSES), sizes (SHAPE), loss_kind (GMC_ERR_LOSS), n_max (GRAPH_SIZE); 4. workspace,
 * P, loss (NULL); 5. P, GP (ALIGN); 6. the workspace size.  B == 0 returns GMC_OK without a launch (gmc_fn_backward: after
 * zeroing grad).  No call allocates or synchronises; everything is enqueued on the caller's stream. */
/* bytes of scratch one gmc_fn_forward + gmc_fn_backward pair needs (features != 0: X is given - no dW1 scratch); 0 for a
 * NULL struct, another abi word, or K outside 2..GMC_KWAY_MAX_CLASSES */
size_t gmc_fn_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int features);
int gmc_fn_forward(const gmc_batch *batch, const gmc_model *model, const float *X /* NULL: the padded adjacency */,
                   int64_t ldx, void *workspace, size_t workspace_bytes, float *P, gmc_stream_t stream);
int gmc_fn_backward(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx, void *workspace,
                    size_t workspace_bytes, const float *P, const float *GP, float *grad, float *dX /* or NULL */,
                    int64_t lddx, gmc_stream_t stream);
/* bytes of scratch gmc_fn_cut_loss_f32 needs: the tile partials, R / 256 + B + 1 floats (0 for a NULL batch, another abi
 * word, negative sizes or K outside 2..GMC_KWAY_MAX_CLASSES) */
size_t gmc_fn_cut_loss_workspace_bytes(const gmc_batch *batch, int32_t K);
int gmc_fn_cut_loss_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const float *P, float C, int32_t loss_kind,
                        void *workspace, size_t workspace_bytes, float *loss /*[B]*/, float *GP /*[R,K] or NULL*/,
                        gmc_stream_t stream);

/* ---- one model per graph (extension: the reference's model as an instance-wise solver, a whole batch per step) ---------
 *
 * The features of the reference are the padded adjacency, so row i of conv1.weight is the embedding of NODE ID i: a model
 * knows the graphs it was trained on.  These entry points train B independent models on the B graphs of a batch in one
 * launch sequence.  For a batch with R rows, K = model->K in 2..GMC_KWAY_MAX_CLASSES (3 included) and hidden width
 * F = model->F the gmc_model is a parameter-block descriptor (its layout is unchanged):
 *    W1 [R,F]    row goff[g] + l is the embedding of node l of graph g: graph g's own conv1.weight [n_g,F]
 *    b1 [B,F], W2 [B,F,K], b2 [B,K]   one conv1.bias, conv2.weight, conv2.bias per graph
 *    N           must equal batch->R (GMC_ERR_SHAPE)
 * The flat order is [W1 | b1 | W2 | b2], count = R*F + B*(F + F*K + K) floats; grad (and a caller's Adam moments) use
 * the same layout.  Graph g's forward, loss (GMC_LOSS_CUT, or GMC_LOSS_EXPECTED_CUT with GMC_MODEL_LOSS_EXPECTED in
 * model->flags), terminals (nodes 0..K-1 fixed to classes 0..K-1) and gradient are exactly those of gmc_kway_forward /
 * gmc_kway_train_fwd_bwd on the one-graph batch of g with a model of N = n_g holding g's four blocks.  Nothing couples
 * two graphs: a graph's P, S, loss and its slices of the gradient have the same bits wherever it stands in the batch and
 * whatever else the batch holds, and are bitwise reproducible (no float atomics, every sum in a fixed order).
 * GMC_MODEL_GRAD_TAIL is not read (no sum over the graphs exists to carry); dropout_p > 0: GMC_ERR_UNSUPPORTED; W1_slab
 * is not read.  Only undirected graphs with symmetric weights are batches of this library (gmc_batch), which step 7 uses.
 *
 * Kernel sequence (row-major [R, ld] buffers, the plan of gmc_kway_*; probe tag in brackets):
 *  1. T0 = dinv o (A_val @ W1)                  gmc_spmm_f32's kernel, column array gcol, source the stacked W1  [GATHER_W1]
 *  2. Hpre = dinv o (A @ T0)                    the same kernel, no bias, no relu                               [AGG_FWD]
 *  3. H = relu(Hpre + b1_g) written in place of Hpre, Z0[r,:] = dinv[r] * (H[r,:] @ W2_g): one wave per row, the row's
 *     graph is its workgroup's (grid = graph x 4-row tile).  The bias is added to the ROUNDED float32 Hpre
 *     (gmc_kway_* fuses it into one fma with the row scale: one rounding less); the H @ W2_g sum is hw2_k's - lane j
 *     takes columns j, j + 64, ... ascending, then a butterfly over the lanes                                    [DENSE_MFMA]
 *  4. the head of gmc_kway_* with graph g's b2 (the same kernel; the bias is read at b2 + g*K).  Its per-graph sums of
 *     the softmax backward ARE db2_g and go straight into the gradient.  Graph-size bound: that of gmc_kway_*       [HEAD]
 *  5. Gs = dinv o relu'(H) o dinv o (GY2 @ W2_g^T) and partials of dW2_g [F,K], db1_g [F] over tiles of 64 rows that
 *     start at the graph's first row (never two graphs in a tile; the two row lanes of a tile take its even and its odd
 *     rows, each ascending, then lane 0 + lane 1)                                                             [HIDDEN_BWD]
 *  6. dW2_g, db1_g = the graph's tile partials added one after the other, ascending                              [COLSUM]
 *  7. U = dinv o (A @ Gs)                       gmc_spmm_f32's kernel                                            [AGG_BWD]
 *  8. dW1[j,:] = sum over the entries e of row j of val[e] * U[gcol[e],:]: dW1 = A_val^T @ U, and A_val^T = A_val.  A
 *     plain SpMM without scale or bias (CSR order), because every row of W1 belongs to exactly one node: the per-chunk
 *     [N,F] partials and their fold, which gmc_kway_* needs for a W1 all graphs share, do not exist here            [DW1]
 * A training call is these eight launches, a forward the first four.  Adam: gmc_adam_f32 / gmc_adam_devstep_f32 over the
 * count floats (every instance shares the step number).
 *
 * Argument checks: all before any HIP call, in the order of gmc_kway_* - step 2's last item is N != R (SHAPE) in the
 * place of n_max > N.  An empty batch (R == 0) launches nothing and zeroes the count floats of grad.  Workspace: T0, H
 * [R, ld], Z0 [R,K]; training: GY2 [R,K] and the tile partials [R / 64 + B + 1][F][K+1]. */
/* bytes of scratch gmc_inst_forward / gmc_inst_train_fwd_bwd need (0 for a NULL struct, another abi word, or K outside
 * 2..GMC_KWAY_MAX_CLASSES) */
size_t gmc_inst_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training);
/* P [R,K]; S [R] / loss [B] optional */
int gmc_inst_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace, size_t workspace_bytes,
                     float *P, int32_t *S, float *loss, gmc_stream_t stream);
/* grad: the flat [dW1 [R,F] | db1 [B,F] | dW2 [B,F,K] | db2 [B,K]], overwritten */
int gmc_inst_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                           size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad, gmc_stream_t stream);
/* Keep every graph's best partition so far: for each graph g with loss[g] < best_loss[g] (strict: the first minimum
 * wins; a NaN loss never does) the rows goff[g]..goff[g+1]-1 of S [R] are copied into best_S [R], best_loss[g] = loss[g]
 * and best_epoch[g] = epoch.  Two launches (probe tag FINISH twice): the row-parallel copy only reads best_loss, the second
 * launch - one thread per graph, behind the kernel boundary - stores it, so the workgroups of one graph all see the same
 * comparison; no atomics, no waiting.  Initialise best_loss with +inf: epoch 0 then always wins.  Errors, before any HIP
 * call: a NULL pointer GMC_ERR_NULL, batch->abi GMC_ERR_ABI, negative sizes GMC_ERR_SHAPE.  B == 0 launches nothing. */
int gmc_inst_keep_best_f32(const gmc_batch *batch, const int32_t *S, const float *loss, int32_t epoch, int32_t *best_S,
                           float *best_loss, int32_t *best_epoch, gmc_stream_t stream);

/* Per-graph early stopping: the reference's tolerance / patience rule (TrainingNeural.py:429-444: train_model stops a
 * model whose loss has stalled `patience` times in a row) with keep-best behind it, for every graph of the batch on its
 * own.  THE RULE, per graph g and epoch e:
 *   L = loss[g], the loss measured in epoch e before that epoch's update; p = prev_loss[g] (+inf before epoch 0).
 *   g stalls when  e > 0 && (L > p || fabs((double)p - (double)L) <= tolerance).  Comparisons are taken as written, so a
 *   NaN loss never stalls (and never wins); the difference is taken in double because the reference compares Python
 *   floats of float32 losses.
 *   stalled:      stall[g] += 1; if stall[g] >= patience: stop_epoch[g] = e and NOTHING ELSE of g changes - no keep-best,
 *                 no prev_loss (the reference breaks before both; the Adam update of epoch e has been applied by then,
 *                 as in the reference).
 *   not stalled:  stall[g] = 0.
 *   not stopped in this call: keep-best exactly as gmc_inst_keep_best_f32 (strict <, the first minimum wins), then
 *                 prev_loss[g] = L.
 *   A graph with stop_epoch[g] >= 0 on entry is stopped: nothing of it is written, whatever its loss.
 * Start with prev_loss = +inf, stall = 0, stop_epoch = -1, best_loss = +inf.  It takes the place of
 * gmc_inst_keep_best_f32 in a loop with early stopping, in the same two-launch shape and for the same reason (probe tag
 * FINISH twice): the row launch only reads the per-graph state and copies the rows of S of the graphs that are running,
 * not stopping now, and improving; the one-thread-per-graph launch stores the decision behind the kernel boundary.  No
 * atomics, no waiting, no scratch.  Errors, before any HIP call, in this order: a NULL pointer GMC_ERR_NULL (batch
 * first), batch->abi GMC_ERR_ABI, negative sizes, patience < 1, a negative or NaN tolerance GMC_ERR_SHAPE.  B == 0
 * launches nothing. */
int gmc_inst_early_stop_f32(const gmc_batch *batch, const int32_t *S, const float *loss, int32_t epoch, double tolerance,
                            int32_t patience, float *prev_loss, int32_t *stall, int32_t *stop_epoch, int32_t *best_S,
                            float *best_loss, int32_t *best_epoch, gmc_stream_t stream);

/* gmc_adam_f32 over the flat [W1 [R,F] | b1 [B,F] | W2 [B,F,K] | b2 [B,K]] buffer of one model per graph (count = R*F +
 * B*(F + F*K + K) floats; param, grad, m, v in that layout), cut by graph: one launch (probe tag ADAM) whose grid is
 * graph x tile of that graph's own floats - its n_g * F floats of W1 in tiles of GMC_INST_ADAM_TILE_FLOATS as float4, then
 * its F + F*K + K floats of the three small blocks, scalar.  stop_epoch [B] or NULL (all running): a workgroup of a graph
 * with stop_epoch[g] >= 0 returns after reading that word - no byte of that graph's param, grad, m or v is read or
 * written.  The per-element update and the host-side derivation of lr / bias_correction1 and sqrt(bias_correction2) are
 * gmc_adam_f32's (one definition), so with no graph stopped param, m and v are byte for byte gmc_adam_f32's over the same
 * count floats.  Floats after count are never touched.  Errors, before any HIP call: a NULL batch / goff / param / grad /
 * m / v GMC_ERR_NULL (batch first, then batch->abi GMC_ERR_ABI); negative sizes, F < 1, K < 1, step < 1 GMC_ERR_SHAPE;
 * F % 4 or a buffer off a 16-byte boundary GMC_ERR_ALIGN.  B == 0 launches nothing. */
#define GMC_INST_ADAM_TILE_FLOATS 4096
int gmc_inst_adam_f32(const gmc_batch *batch, int32_t F, int32_t K, float *param, const float *grad, float *m, float *v,
                      double lr, double beta1, double beta2, double eps, int32_t step, const int32_t *stop_epoch,
                      gmc_stream_t stream);

/* ---- one model per graph for graphs beyond GMC_MAX_GRAPH_NODES (extension) -------------------------------------------------
 *
 * gmc_inst_forward_t / gmc_inst_train_fwd_bwd_t for graphs of up to GMC_LARGE_MAX_GRAPH_NODES nodes: the same model
 * descriptor (W1 [R,F], b1 [B,F], W2 [B,F,K], b2 [B,K], N == R), flat layout [W1 | b1 | W2 | b2], loss flag, `terminals`
 * (1: nodes 0..K-1 of every graph fixed to classes 0..K-1; 0: no node fixed, a graph then needs one node) and empty-batch
 * behaviour.  They take ANY batch within the bound, small graphs included; gmc_inst_* stays the faster sequence for the
 * graphs it accepts, and no entry point routes a batch from one to the other.
 *
 * Kernel sequence of a training call (probe tag in brackets; the numbers are gmc_inst_*'s steps):
 *  1. T0 = dinv o (A_val @ W1)        gmc_spmm_f32's kernel, then the rows of more than 64 entries once more      [GATHER_W1 x2]
 *  2. Hpre = dinv o (A @ T0)          likewise                                                                    [AGG_FWD x2]
 *  3. H = relu(Hpre + b1_g), Z0 = dinv o (H @ W2_g): gmc_inst_*'s row arithmetic (one wave per row, lane j columns j,
 *     j + 64, ..., then the butterfly) on a grid of (graph, min(ceil(n_max / 4), 65535)) whose workgroup y takes the
 *     graph's 4-row tiles y, y + gridDim.y, ...: H and Z0 are byte for byte gmc_inst_*'s                          [DENSE_MFMA]
 *  4. the head of gmc_large_* (four launches on a grid of (graph, tile of 256 rows): probabilities and decode; the loss
 *     terms and the softmax backward; the per-graph fold; GY2 = A @ (dinv o GZ)) with graph g's b2 read at b2 + g*K,
 *     terms = terminals ? min(n_g, K) : 0 terminals - also what decides, in the relaxed loss, whether a neighbour is a
 *     terminal - and the fold's per-graph sums of the softmax backward, which ARE db2_g, written straight into the
 *     gradient.  A forward ends after the first three of the four                                                  [HEAD x4]
 *  5. Gs and the tile partials of dW2_g, db1_g       gmc_inst_*'s kernel                                          [HIDDEN_BWD]
 *  6. their fold                                     gmc_inst_*'s kernel                                          [COLSUM]
 *  7. U = dinv o (A @ Gs)             gmc_spmm_f32's kernel, then the rows of more than 64 entries once more      [AGG_BWD x2]
 *  8. dW1 = A_val @ U                 likewise                                                                    [DW1 x2]
 * Summation orders: a row of at most 64 entries in CSR order by its lane; a longer row (a hub) in the head by its wave
 * (lane j entries j, j + 64, ..., then the butterfly over the lanes), in the four F-wide sums of steps 1, 2, 7, 8 as its
 * first 64 entries plus, one after the other, the sum of each further 64 (each in CSR order); a tile's K + 1 head sums
 * by the wave butterfly over its rows, then its four waves ascending; a graph's sums by its tiles ascending.  (The
 * one-workgroup head of gmc_inst_* deals a graph's rows over 1024 / 512 threads instead: the two agree in S and to
 * rounding in P, loss and gradient, not to the bit.)  No float atomics, no waiting between workgroups; a graph's results
 * have the same bits wherever it stands in the batch and are bitwise reproducible.
 *
 * Argument checks: all before any HIP call, in the order of gmc_inst_*_t, with n_max > GMC_LARGE_MAX_GRAPH_NODES
 * (GMC_ERR_GRAPH_SIZE) in the place of the one-workgroup head's bound, and W1 among the pointers that must be 16-byte
 * aligned (GMC_ERR_ALIGN: the launches for the rows of more than 64 entries read it as float4 only).  Workspace: gmc_inst_*'s buffers (T0, H [R, ld],
 * Z0 [R,K]; training: GY2 [R,K], the tile partials [R / 64 + B + 1][F][K+1]), then the decode Sw [R], the head's tile
 * partials [R / 256 + B + 1][K+1] and - training - dinv o GZ [R,K], each rounded up to 256 bytes.
 * Memory per node: the flat buffer, its gradient and two Adam moments 16 * F bytes, the workspace about 8 * ld bytes
 * (ld = F rounded up to 32): about 1.5 KB at F = 64.  gmc_inst_adam_f32 keeps its own bound (n_max * F up to about 2^28);
 * gmc_adam_f32 over the flat buffer has none. */
size_t gmc_inst_large_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training);
int gmc_inst_large_forward(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C, void *workspace,
                           size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream);
int gmc_inst_large_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C,
                                 void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad,
                                 gmc_stream_t stream);

/* ---- a graph-attention first layer (extension: the first of the "future improvements" of the reference's README) ------
 *
 * The entry points above have GraphConv(norm='both') as layer 1 (TrainingNeural.py:80).  These three replace that layer's
 * aggregation by single-head graph attention (GAT) on the graph with self-loops added, followed by relu; three classes;
 * layer 2, the head, both losses, the terminal override and the decoders are those of gmc_forward (TrainingNeural.py:83-106).
 * Per graph, on local nodes; the terms of row i are its CSR entries (rowptr / gcol / lcol) plus ONE self term - a self-loop
 * edge of the graph counts as one more ordinary term:
 *
 *   T[i,:]   = sum_e vals[e] * W1[lcol[e],:]                  (X @ W1 for X = the padded adjacency; no row scale)
 *   s_src[j] = T[j,:] . a_src        s_dst[i] = T[i,:] . a_dst
 *   z_ij     = s_dst[i] + s_src[j]   e_ij = z_ij > 0 ? z_ij : slope * z_ij          for j in terms(i)
 *   alpha_ij = exp(e_ij - m_i) / sum_j exp(e_ij - m_i),  m_i = max_j e_ij
 *   H[i,:]   = relu(sum_j alpha_ij * T[j,:] + b1)
 *   Z0 = dinv o (H @ W2), then the head of gmc_forward (GraphConv norm='both' for layer 2)
 *
 * No attention dropout and no feature dropout; edge weights enter through the features only (as in this library's GraphConv
 * aggregation); a node without neighbours has alpha_ii = 1.  a_src, a_dst: [F] device floats (any alignment), slope: the
 * negative slope of the leaky relu, in [0, 1] (0.2 in the GAT paper).
 *
 * Backward, with G = relu'(H) o (dinv o (GY2 @ W2^T)) the gradient at the pre-activation:
 *
 *   da_ij   = G[i,:] . T[j,:]
 *   de_ij   = alpha_ij * (da_ij - sum_k alpha_ik * da_ik)
 *   dz_ij   = de_ij * (z_ij > 0 ? 1 : slope)
 *   ds_dst[i] = sum_j dz_ij                       (row i's own terms)
 *   ds_src[j] = sum_{i: j in terms(i)} dz_ij      (the reverse edges)
 *   dT[j,:] = sum_{i: j in terms(i)} alpha_ij * G[i,:] + ds_src[j] * a_src + ds_dst[j] * a_dst
 *   da_src  = sum_j ds_src[j] * T[j,:]            da_dst = sum_i ds_dst[i] * T[i,:]
 *   dW1     = X^T @ dT;  db1 = colsum(G);  dW2, db2: as gmc_train_fwd_bwd
 *
 * The flat gradient is [dW1 | db1 | dW2 | db2 | da_src | da_dst]: N*F + F + F*3 + 3 + 2F floats, plus the tail slot with
 * GMC_MODEL_GRAD_TAIL.  The batch's CSR must be symmetric with each row's columns in ascending order (what
 * gcn-max-cut_amd/graph.py builds): the backward finds the reverse of an entry by a binary search.
 * Kernel sequence: one kernel per operation on row-major [R, ld] buffers (the plan of the *_features and gmc_kway_* calls),
 * the layer-1 kernels from csrc/attention.hip; gmc_set_fuse does not matter, the ELL table is read by the head only,
 * W1_slab is not read.  model->K must be 3 (GMC_ERR_CLASSES); dropout_p > 0: GMC_ERR_UNSUPPORTED.  Argument checks: the
 * order documented above for the fused entry points, with a_src / a_dst among step 1's pointers (NULL), dropout_p > 0
 * (UNSUPPORTED) at the end of step 2, the slope as step 3 (outside [0, 1] or NaN: SHAPE), and W1 / b1 with grad in step 5
 * (ALIGN; P and W2 need no alignment here, unlike gmc_kway_*: the 3-wide kernels read them with 4-byte accesses).  Results are bitwise reproducible (no float atomics: every sum runs in a fixed order). */
/* bytes of scratch gmc_att_forward / gmc_att_train_fwd_bwd need (0 for a NULL struct, another abi word, or K != 3) */
size_t gmc_att_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training);
/* gmc_forward with the attention layer: P [R,3]; S [R] / loss [B] optional.  An empty batch returns GMC_OK without a launch. */
int gmc_att_forward(const gmc_batch *batch, const gmc_model *model, const float *a_src, const float *a_dst, float slope,
                    float C, void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                    gmc_stream_t stream);
/* gmc_train_fwd_bwd with the attention layer: grad as laid out above (with GMC_MODEL_GRAD_TAIL loss must be non-NULL).  An
 * empty batch zeroes grad (and the tail slot) without any other launch. */
int gmc_att_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, const float *a_src, const float *a_dst,
                          float slope, float C, void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                          float *grad, gmc_stream_t stream);

/* ---- decode / post-processing (the caller of the path in BASELINE configs[4]) -------- */

/* Random-sampling post-processing of Testing/TestingNeuralNetwork.py:18-98 for every graph of
 * the batch: `iters` samples of the node probabilities P [R,3] (nodes 0,1,2 of each graph fixed
 * to classes 0,1,2; node l >= 3 takes the first class whose running float32 sum exceeds its
 * uniform draw, last class as fallback), cut value of each sample, strictly-best sample kept.
 * uniforms: device doubles, for graph g `iters` x (n_g - 3) values starting at uoff[g] (device
 * int64 [B+1]) in the reference's draw order (iteration-major, node-minor).
 * Outputs (device): assign_all [iters][R] int8, cut_all [B][iters], best_assign [R] int32,
 * best_cut [B], best_iter [B]. */
int gmc_decode_sample_f32(const gmc_batch *batch, const float *P, const double *uniforms,
                          const int64_t *uoff, int32_t iters, int8_t *assign_all, float *cut_all,
                          int32_t *best_assign, float *best_cut, int32_t *best_iter,
                          gmc_stream_t stream);

/* ---- the same sampler with its uniforms drawn on the GPU from a seed (extension) ----------------------------------
 *
 * gmc_decode_sample_f32 reads uniforms the caller drew on the host in numpy's order, which is what reproduces the
 * reference's numbers.  This entry point draws them itself from a counter-based hash: no uniform is generated on the
 * host or copied, results are reproducible from the seed and independent of how graphs are batched.
 *
 * The draw rule.  All arithmetic is modulo 2^64.
 *  - GOLD = 0x9E3779B97F4A7C15.
 *  - mix64 is the splitmix64 finaliser, exactly as in the annealing (stated at gmc_refine_anneal_f32 below).
 *  - A graph's key is key = mix64(seed + GOLD * (index + 1)).  index is the graph's position in its dataset, a
 *    non-negative integer.
 *  - The uniform for iteration it (0-based) and local node l of that graph is
 *    h = mix64(key + GOLD * (((u64)it << 32 | l) + 1)), then u = (double)(h >> 11) * 2^-53.  This lies in [0, 1) and
 *    is exact.
 *  - Nodes 0, 1, 2 are the terminals of classes 0, 1, 2.
 *  - Node l >= 3 takes its class exactly as decode_sample_kernel does today:
 *      c0 = (double)p[0];
 *      c1 = c0 + (double)p[1];
 *      class 0 if u < c0;
 *      else class 1 if u < c1;
 *      else class 2.
 * A graph's samples depend on its key alone.  They do not depend on the batch it sits in, on its position in the
 * batch, or on iters: iteration 5 of a 10-iteration call is iteration 5 of a 200-iteration call.
 *
 * gkey: device uint64 [B], the keys (the caller computes them: the library never sees the seed or the indices).
 * Outputs (device) as gmc_decode_sample_f32's: cut_all [B][iters], best_assign [R] int32 (the strictly best sample,
 * the first on ties), best_cut [B], best_iter [B]; a sample's cut has the bits gmc_decode_sample_f32 and
 * gmc_refine_local_f32(max_sweeps = 0) report for the same assignment.  assign_all [iters][R] int8 may be NULL: then
 * nothing of size iters x R is written (best_assign is regenerated from the hash either way) and every other output
 * equals the non-NULL call's.  Argument checks, before any HIP call, in the order of the other decoders: a NULL
 * pointer (assign_all aside) GMC_ERR_NULL, batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol GMC_ERR_NULL,
 * iters < 1 or B < 0 GMC_ERR_SHAPE, n_max < 3 or n_max > 65535 GMC_ERR_GRAPH_SIZE; B == 0 returns GMC_OK without a
 * launch.  A graph with fewer than 3 or more than n_max nodes inside a batch is skipped (nothing of it is written), as
 * gmc_round_conditional_f32 skips it.  The call allocates nothing and does not synchronise: two launches on the
 * caller's stream.  This is gmc_kway_decode_sample_seeded_f32 at K = 3: the same kernels. */
int gmc_decode_sample_seeded_f32(const gmc_batch *batch, const float *P, const uint64_t *gkey, int32_t iters,
                                 int8_t *assign_all, float *cut_all, int32_t *best_assign, float *best_cut,
                                 int32_t *best_iter, gmc_stream_t stream);

/* ---- local search over decoded partitions (extension: no counterpart in the reference) ---------------------------
 *
 * Single-node-move refinement of candidate partitions, per graph of the batch (local ids 0..n-1, CSR rows of an
 * undirected graph, weight 1 where vals is NULL):
 *  - nodes 0, 1, 2 never move, whatever class they hold (override_fixed_nodes, TrainingNeural.py:87-94); the
 *    movable nodes are 3..n-1.  An entry of `order` that names a terminal, or no row of its graph, is not visited;
 *  - colouring: first-fit over the movable nodes in increasing id, a node taking the smallest colour no movable
 *    neighbour of smaller id holds (self-loops and neighbours 0..2 ignored), so each colour class is an independent
 *    set among movable nodes;
 *  - one sweep visits the classes in increasing colour; every node v of a class sums in fp32, in the CSR order of its
 *    row, the weights of its edges to neighbours of class 0, 1 and 2 as the classes stand at the start of that colour
 *    step (self-loops skipped) into W0, W1, W2; with c = class(v) and k the class of the smallest W (lowest index on
 *    ties), v moves to k iff W[k] < W[c] (a class byte outside 0..2 counts for no W, and such a movable node takes k).
 *    The result equals a sequential sweep in (colour, id) order;
 *  - sweeps run until one moves nothing, or max_sweeps have run (max_sweeps = 0: no move).
 * Every move of a node with a class byte 0..2 raises the cut as gmc_decode_sample_f32 counts it.  That count takes
 * every edge of a byte outside 0..2 as cut, so giving such a node its class may lower it: "the refined cut is never
 * below the input cut" holds for candidates whose class bytes are all 0..2. */

/* HOST routine (all pointers are host pointers): the colouring above for a batch of B graphs (goff [B+1], rowptr,
 * lcol as in gmc_batch).  Writes order: per graph, the batch row ids of its movable nodes sorted by (colour, id)
 * (R - 3B entries; room for R suffices); cgoff [B+1] and cptr: class k of graph g is
 * order[cptr[cgoff[g]+k] .. cptr[cgoff[g]+k+1]), graph g has cgoff[g+1] - cgoff[g] - 1 classes (none for n = 3).
 * cptr needs at most R + B entries: cptr_cap < R + B returns GMC_ERR_SHAPE before anything is written; a graph
 * with < 3 or > GMC_MAX_GRAPH_NODES nodes GMC_ERR_GRAPH_SIZE. */
int gmc_refine_order_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol,
                          int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap);

/* The local search above on `cands` candidates of every graph: assign [cands][R] int8 (device, in/out) holds them
 * and receives the refined assignments; order / cgoff / cptr are gmc_refine_order_host's output in device memory.
 * Each refined candidate is then scored and picked exactly as gmc_decode_sample_f32 scores and picks its samples:
 * cut_all [B][cands], best_assign [R] int32 (the strictly best candidate, first wins), best_cut [B], best_idx [B].
 * sweeps [B][cands] (NULL: not written): the sweeps run, the last of them the one that moved nothing when the
 * candidate converged within max_sweeps.  Errors: a NULL pointer (sweeps aside) GMC_ERR_NULL, batch->abi
 * GMC_ERR_ABI, cands < 1 or max_sweeps < 0 GMC_ERR_SHAPE, n_max outside 3..GMC_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE;
 * B == 0 launches nothing.  A graph with fewer than 3 or more than n_max nodes inside a batch is skipped (nothing of
 * it is written), as gmc_round_conditional_f32 skips it. */
int gmc_refine_local_f32(const gmc_batch *batch, const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                         int32_t cands, int8_t *assign, int32_t max_sweeps, float *cut_all, int32_t *best_assign,
                         float *best_cut, int32_t *best_idx, int32_t *sweeps, gmc_stream_t stream);

/* ---- annealing over decoded partitions (extension: no counterpart in the reference) ------------------------------
 *
 * The local search above stops at the first single-move local optimum.  This search first runs annealing sweeps that
 * also accept moves that lose cut, keeps the best state it passes through, and then descends from it with the local
 * search.  Per (candidate `cand`, graph), with the colouring and order / cgoff / cptr of gmc_refine_order_host; nodes
 * 0, 1, 2 never move:
 *  1. state = the input candidate, best = state, best_cut = cut(state): the cut as gmc_decode_sample_f32 and
 *     gmc_refine_local_f32 count it (fp32, the same code, the same summation order).
 *  2. annealing sweeps s = 0 .. anneal_sweeps-1, each with inv_temp[s] = 1/T_s (finite, > 0).  A sweep visits the
 *     colour classes in increasing colour.  Every node v of a class (local id v) computes W0, W1, W2 exactly as the
 *     local search does: fp32 sums in the CSR order of its row, self-loops skipped, a class byte outside 0..2 counting
 *     for none.  With c = class(v), the target k is the class of the smaller W among the two classes other than c
 *     (the lower index on a tie) and delta = W[k] - W[c] in fp32;
 *         v moves to k  iff  delta < 0  or  delta * inv_temp[s] <= levels[h >> 54]      (one fp32 multiply)
 *         h = mix64(seed + 0x9E3779B97F4A7C15 * (ctr + 1)),   ctr = (uint64)cand << 32 | (uint64)s << 12 | v
 *     in uint64 arithmetic, mix64 the splitmix64 finaliser: z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 *     z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31.  A movable node whose class byte is outside 0..2 takes the
 *     local search's k (the smallest of all three W, lowest index on ties) unconditionally.  `levels` is a table of
 *     GMC_ANNEAL_LEVELS floats the caller supplies, so the device evaluates neither exp nor log; with
 *     levels[i] = (float)(-log((i + 0.5) / GMC_ANNEAL_LEVELS)), quantiles of an exponential variate, the rule is a
 *     Metropolis test (accept with probability exp(-delta / T)) at 10-bit resolution.
 *     After each sweep c_s = cut(state); if c_s > best_cut: best = state, best_cut = c_s (the snapshot).
 *  3. descent: state = best, then the sweeps of gmc_refine_local_f32, with exactly its rule, until one moves nothing or
 *     max_descent_sweeps have run.
 *  4. state is written back, scored and picked exactly as gmc_refine_local_f32 scores and picks.
 * By construction: a class is an independent set and the level depends only on (cand, s, v), so the parallel colour
 * step equals a sequential visit in (colour, id) order; anneal_sweeps = 0 is gmc_refine_local_f32 with
 * max_sweeps = max_descent_sweeps, bit for bit; the output cut of a candidate whose class bytes are all 0..2 is never
 * below its input cut (the cut count takes every edge of a byte outside 0..2 as cut, and the first visit of such a
 * node gives it a class, so its candidate's cut may fall); and a candidate's result depends on its graph, its index,
 * the seed and the schedule alone - not on the graph's place in the batch nor on the rest of the batch. */
#define GMC_ANNEAL_LEVELS 1024

/* The annealing above on `cands` candidates of every graph: assign [cands][R] int8 (device, in/out); order / cgoff /
 * cptr as for gmc_refine_local_f32; inv_temp [anneal_sweeps] and levels [GMC_ANNEAL_LEVELS] device floats (either may
 * be NULL when anneal_sweeps == 0).  Outputs as gmc_refine_local_f32's: cut_all [B][cands], best_assign [R] int32,
 * best_cut [B], best_idx [B]; optional (NULL: not written) snap_sweep [B][cands]: 0 = the descent started from the
 * input, s + 1 = from the snapshot taken after sweep s; sweeps [B][cands]: the descent sweeps run, counted as the
 * local search counts them.  Errors, all found before any HIP call: a NULL required pointer GMC_ERR_NULL, batch->abi
 * GMC_ERR_ABI, cands < 1, a negative sweep count or anneal_sweeps >= 2^20 (the counter layout) GMC_ERR_SHAPE, n_max
 * outside 3..GMC_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE; B == 0 launches nothing.  A graph with fewer than 3 or more than
 * n_max nodes inside a batch is skipped (nothing of it is written); an entry of `order` that names a terminal, or no
 * row of its graph, is not visited.  Two launches on the caller's stream.  This is gmc_kway_refine_anneal_f32 at
 * K = 3: the same kernels. */
int gmc_refine_anneal_f32(const gmc_batch *batch, const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                          int32_t cands, int8_t *assign, const float *inv_temp, int32_t anneal_sweeps,
                          const float *levels, uint64_t seed, int32_t max_descent_sweeps, float *cut_all,
                          int32_t *best_assign, float *best_cut, int32_t *best_idx, int32_t *snap_sweep,
                          int32_t *sweeps, gmc_stream_t stream);
/* DIAGNOSTIC host query (no HIP call; reads n_max, nnz_max and whether vals is NULL) for tests and timing scripts;
 * results never depend on its answer: 1 when gmc_refine_anneal_f32 keeps a copy of each graph's CSR in LDS for this
 * batch, 0 when the graphs are too large for that and it reads the batch's arrays in global memory (same results, bit
 * for bit); < 0 on a bad argument.  The layout does not depend on the class count, so the answer holds for
 * gmc_kway_refine_anneal_f32 on the same batch as well. */
int gmc_refine_anneal_staged(const gmc_batch *batch);

/* ---- rounding by conditional expectations (extension: no counterpart in the reference) ---------------------------
 *
 * GMC_LOSS_EXPECTED_CUT trains on the expected cut of rounding every node independently from its row of P.  This
 * decoder turns such a P into ONE partition whose cut is not below that expectation (the method of conditional
 * expectations), deterministically and with one visit per node, then optionally descends from it with the local
 * search.  It takes K = 2 .. GMC_KWAY_MAX_CLASSES classes.  Per graph of the batch (local ids 0..n-1, n >= K, CSR rows
 * of an undirected graph, weight w_e = 1 where vals is NULL); nodes 0..K-1 are the terminals of classes 0..K-1:
 *  1. state: q[u][0..K-1], fp32.  A terminal u has q_u = e_u; its row of P is never read into the result, whatever it
 *     holds (NaN included).  Every other node has q_u = its row of P as given (not renormalised).
 *  2. expected cut (optional output): 1/2 * sum_v sum_{e in row v, u != v} w_e * (1 - q_u . q_v) over that state,
 *     summed in fp32 - one partial per row, the rows of a thread added in ascending order, a butterfly per wave, the
 *     four wave sums ascending (the block sum of the cut count).  Reproducible run to run; the bits are not pinned.
 *  3. rounding: the movable nodes K..n-1 are coloured first-fit as for the local search above, with K in the place of
 *     3 (gmc_round_order_host).  The colour classes are visited in increasing colour.  Node v of a class computes, for
 *     every class k, M_k = sum_{e in row v, CSR order, u != v} w_e * q_u[k] starting from +0, the product and the sum
 *     each rounded to fp32 (no fused multiply-add), over the state as it stands at the start of that colour step.  v
 *     takes the class kk of the smallest M (the lowest index on ties): q_v becomes e_kk, its class byte kk.  No two
 *     nodes of a class are adjacent, so the result equals a sequential visit in (colour, id) order.
 *     M_k is the cut v loses in expectation by taking class k, so the smallest M keeps the conditional expectation of
 *     the cut from falling: in exact arithmetic the rounded cut is >= the expected cut of step 2.  In fp32 a decision
 *     can lose at most 2 (deg + 1) 2^-24 of the node's absolute weighted degree.
 *  4. descent: up to max_descent_sweeps sweeps of the local search's rule at K classes over the same state, which is
 *     one-hot by now, so the same M_k are the sums of the weights of v's edges to neighbours of class k: v moves to
 *     the class kk of the smallest M (lowest index on ties) iff M_kk < M_own; sweeps stop after one that moves
 *     nothing.  At K = 3 this is gmc_refine_local_f32 on the rounded assignment, byte for byte and sweep for sweep.
 *  5. score: the cut of the class bytes as gmc_decode_sample_f32 and gmc_refine_local_f32 count it (the same code,
 *     the same bits).
 * Nothing is claimed about denormal probabilities or products (a tie may then hinge on how they are flushed). */

/* HOST routine (all pointers are host pointers): gmc_refine_order_host's colouring and (colour, id) order with the
 * movable nodes starting at K instead of 3 (order: R - K*B entries; cptr_cap >= R + B as there).  K = 3 writes what
 * gmc_refine_order_host writes, array for array.  K outside 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES; a graph with
 * < K or > GMC_MAX_GRAPH_NODES nodes GMC_ERR_GRAPH_SIZE. */
int gmc_round_order_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol, int32_t K,
                         int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap);

/* The rounding above for every graph of the batch: P [R,K] device floats, order / cgoff / cptr gmc_round_order_host's
 * output for the same K in device memory.  Outputs (device): assign [R] int8 (a row of candidates for
 * gmc_refine_local_f32 / gmc_refine_anneal_f32 when K = 3), cut [B]; optional (NULL: not computed) expected [B], the
 * expected cut of step 2, and sweeps [B], the descent sweeps run, counted as gmc_refine_local_f32 counts them (0 for
 * max_descent_sweeps = 0).  Argument checks, before any HIP call, in the order of the other decoders: a NULL pointer
 * (expected and sweeps aside) GMC_ERR_NULL, batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol GMC_ERR_NULL, K outside
 * 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES, max_descent_sweeps < 0 or B < 0 GMC_ERR_SHAPE, n_max < K or n_max >
 * GMC_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE; B == 0 returns GMC_OK without a launch.  A graph with fewer than K or more
 * than n_max nodes inside a batch is skipped (nothing of it is written; the caller refuses such batches: goff is
 * device memory).  One 256-thread workgroup per graph keeps q [n_max][K] and the class bytes in LDS, (4K + 1) * n_max
 * bytes - 132 KiB for K = 8 at GMC_MAX_GRAPH_NODES, which fits, so that constant is the only size limit.  The call
 * allocates nothing and does not synchronise: one launch on the caller's stream, no atomics, bitwise reproducible. */
int gmc_round_conditional_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K,
                              const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                              int32_t max_descent_sweeps, int8_t *assign /*[R]*/, float *cut /*[B]*/,
                              float *expected /*[B] or NULL*/, int32_t *sweeps /*[B] or NULL*/, gmc_stream_t stream);

/* ---- the seeded sampler and the annealing at K classes (extension; K = 2 .. GMC_KWAY_MAX_CLASSES) ------------------
 *
 * gmc_decode_sample_seeded_f32, gmc_refine_local_f32 and gmc_refine_anneal_f32 are 3-class.  The two entry points below
 * are the same decoders for the models of gmc_kway_forward: nodes 0..K-1 of every graph are the terminals of classes
 * 0..K-1, P has K columns, class bytes are 0..K-1.  gmc_decode_sample_seeded_f32 and gmc_refine_anneal_f32 ARE these
 * two at K = 3: they check their own arguments as stated above and then launch the same kernels, so every output is
 * the K = 3 output by construction; gmc_refine_local_f32 keeps a kernel of its own (no level table, no best state, no
 * staged graph in LDS) around the descent loop all of them share.
 *
 * The K-class draw rule.  All arithmetic is modulo 2^64; GOLD, mix64 and a graph's key are those of
 * gmc_decode_sample_seeded_f32.
 *  - The uniform for iteration it (0-based) and local node l is h = mix64(key + GOLD * (((u64)it << 32 | l) + 1)), then
 *    u = (double)(h >> 11) * 2^-53, in [0, 1) and exact.
 *  - Nodes 0..K-1 are the terminals of classes 0..K-1, whatever their rows of P hold.
 *  - Node l >= K, with p its row of P: c_0 = (double)p[0], c_j = c_{j-1} + (double)p[j] (a running sum in double).
 *    The node takes the first class j in 0..K-2 with u < c_j, else class K-1.  Class K-1 is the fallback: no compare
 *    against c_{K-1} is made, so an all-zero row and a NaN row give K-1.
 * As at three classes a graph's samples depend on its key alone - not on the batch, its place in it, or iters. */

/* The K-class sampler for every graph of the batch: P [R,K] device floats, gkey [B] device uint64.  Outputs (device) as
 * gmc_decode_sample_seeded_f32's: cut_all [B][iters], best_assign [R] int32 (the strictly best sample, the first on
 * ties, regenerated from the hash), best_cut [B], best_iter [B]; assign_all [iters][R] int8 may be NULL, and every other
 * output is then equal.  A sample's cut has the bits gmc_refine_local_f32 / gmc_kway_refine_anneal_f32 report for the
 * same assignment (the same code).  Argument checks, before any HIP call, in the order of the other decoders: a NULL
 * pointer (assign_all aside) GMC_ERR_NULL, batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol GMC_ERR_NULL, K outside
 * 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES, iters < 1 or B < 0 GMC_ERR_SHAPE, n_max < K or n_max > 65535
 * GMC_ERR_GRAPH_SIZE; B == 0 returns GMC_OK without a launch.  A graph with fewer than K or more than n_max nodes
 * inside a batch is skipped (nothing of it is written), as gmc_round_conditional_f32 skips it.  The call allocates
 * nothing and does not synchronise: two launches on the caller's stream, no atomics, bitwise reproducible. */
int gmc_kway_decode_sample_seeded_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K,
                                      const uint64_t *gkey, int32_t iters, int8_t *assign_all /*or NULL*/,
                                      float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_iter,
                                      gmc_stream_t stream);

/* The K-class annealing: steps 1-4 of gmc_refine_anneal_f32 per (candidate `cand`, graph), with the colouring and
 * order / cgoff / cptr of gmc_round_order_host for the same K, and these generalisations:
 *  - nodes 0..K-1 never move, whatever class they hold; the movable nodes are K..n-1;
 *  - a node v computes W_0..W_{K-1}: fp32 sums in the CSR order of its row of the weights of its edges to neighbours
 *    of class 0..K-1, self-loops skipped, a class byte outside 0..K-1 counting for none;
 *  - annealing sweep: with c = class(v), the target k is the class of the smallest W among the K-1 classes other than c
 *    (the lowest index on ties), delta = W[k] - W[c] in fp32, and
 *        v moves to k  iff  delta < 0  or  delta * inv_temp[s] <= levels[h >> 54]
 *    with h, ctr = (uint64)cand << 32 | (uint64)s << 12 | v, the level table and the snapshot rule exactly those of
 *    gmc_refine_anneal_f32.  A movable node whose byte is outside 0..K-1 takes the class of the smallest of all K sums
 *    (lowest index on ties) unconditionally;
 *  - descent: the local search's rule at K classes, the one gmc_round_conditional_f32 runs in its step 4: v moves to
 *    the class kk of the smallest of all K sums (lowest index on ties) iff W[kk] < W[c] (a byte outside 0..K-1: always);
 *    sweeps until one moves nothing or max_descent_sweeps have run;
 *  - score and pick: as gmc_refine_local_f32 scores and picks (fp32, the same code).
 * anneal_sweeps = 0 is the K-class local search over `cands` candidates with max_sweeps = max_descent_sweeps; on the
 * one candidate gmc_round_conditional_f32(max_descent_sweeps = 0) writes it gives what that call gives with the
 * descent, assignment and sweep count.  At K = 3 every output equals gmc_refine_anneal_f32's, and with
 * anneal_sweeps = 0 gmc_refine_local_f32's.  What gmc_refine_anneal_f32 states "by construction" holds with 0..K-1 in
 * the place of 0..2.
 * Arguments and outputs as gmc_refine_anneal_f32's: assign [cands][R] int8 (in/out), inv_temp [anneal_sweeps] and
 * levels [GMC_ANNEAL_LEVELS] (either may be NULL when anneal_sweeps == 0), cut_all [B][cands], best_assign [R] int32,
 * best_cut [B], best_idx [B], optional snap_sweep / sweeps [B][cands].  Argument checks, before any HIP call: a NULL
 * required pointer GMC_ERR_NULL, batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol GMC_ERR_NULL, K outside
 * 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES, cands < 1, a negative sweep count, anneal_sweeps >= 2^20 or B < 0
 * GMC_ERR_SHAPE, anneal_sweeps > 0 with a NULL inv_temp or levels GMC_ERR_NULL, n_max outside K..GMC_MAX_GRAPH_NODES
 * GMC_ERR_GRAPH_SIZE; B == 0 returns GMC_OK without a launch.  A graph with fewer than K or more than n_max nodes
 * inside a batch is skipped.  The LDS of a launch is gmc_refine_anneal_f32's, which does not depend on K
 * (gmc_refine_anneal_staged answers for this call too).  The call allocates nothing and does not synchronise: two
 * launches on the caller's stream, no atomics, bitwise reproducible. */
int gmc_kway_refine_anneal_f32(const gmc_batch *batch, int32_t K, const int32_t *order, const int32_t *cgoff,
                               const int32_t *cptr, int32_t cands, int8_t *assign, const float *inv_temp,
                               int32_t anneal_sweeps, const float *levels, uint64_t seed, int32_t max_descent_sweeps,
                               float *cut_all, int32_t *best_assign, float *best_cut, int32_t *best_idx,
                               int32_t *snap_sweep, int32_t *sweeps, gmc_stream_t stream);

/* ---- evolution: recombining the candidates of a graph across generations (extension; K = 2 .. GMC_KWAY_MAX_CLASSES) --
 *
 * gmc_kway_refine_anneal_f32 improves every candidate on its own and keeps the best.  This stage lets the candidates of
 * a graph learn from each other: they form a population of `cands` members ("slots"), and every generation gives each
 * slot a child of its own member and one of the best members, improves the child with the annealing above and keeps it
 * when it is no worse.  Nodes 0..K-1 are the terminals of classes 0..K-1; the movable nodes are K..n-1.  All integer
 * arithmetic below is modulo 2^64; GOLD = 0x9E3779B97F4A7C15 and mix64 are those of gmc_refine_anneal_f32.
 *
 * Buffers.  pop [2][cands][R] int8 and cut [2][B][cands] float, both the caller's (device).  Plane 0 of pop holds the
 * input population, typically what gmc_kway_refine_anneal_f32 left in `assign`.  Generation g = 1..G reads plane
 * (g-1) & 1 of both and writes plane g & 1 of both; nothing is updated in place.  Before generation 1 one launch writes
 * plane 0 of cut: the cut of every member as gmc_refine_local_f32 counts it (fp32, the same code, the same bits).  What
 * the caller left in cut is never read.
 *
 * Seeds of generation g:  S_g = mix64(seed + GOLD * g),  select_g = mix64(S_g ^ 0x53454C4543543031),
 * cross_g = mix64(S_g ^ 0x43524F5353303031).
 *
 * Generation g for (slot i, graph), prev the plane it reads:
 *  1. rank.  The slots of prev are ordered by (cut descending, slot ascending); rank 0 is the first.  E = elite clipped
 *     to 1..cands; the elite set is the slots of rank 0..E-1.  (Cuts are compared as floats; nothing is claimed when
 *     one of them is NaN.)
 *  2. parents.  a = prev[i].  r = mix64(select_g + GOLD * (i + 1)) mod E; b = the slot of rank r, and if that slot is i
 *     itself, the slot of rank (r + 1) mod E.  With E = 1 and i the slot of rank 0 there is no b: the child is a, with
 *     the terminals set as in step 4, and steps 3 and 4 are not run.
 *  3. align.  O[ca][cb] = #{v in K..n-1 : a[v] = ca and b[v] = cb}, integers; a byte outside 0..K-1 in either parent
 *     counts for no pair.  K rounds of greedy matching: among the pairs (ca, cb) with ca and cb both unmatched take the
 *     one of the largest O, the lowest ca and then the lowest cb on ties, and set pi(cb) = ca.  pi is a bijection of
 *     0..K-1: b's class names translated into a's.
 *  4. crossover.  child[l] = l for the terminals l < K, whatever the parents hold there.  For a movable node v:
 *       b[v] outside 0..K-1:                  child[v] = a[v]         (a byte of no class loses to the other parent's)
 *       else a[v] == pi(b[v]):                child[v] = a[v]
 *       else a[v] outside 0..K-1:             child[v] = pi(b[v])
 *       else h = mix64(cross_g + GOLD * (((uint64)i << 32 | v) + 1)):  child[v] = pi(b[v]) if h >> 63, else a[v].
 *  5. improve.  Steps 1-3 of gmc_kway_refine_anneal_f32 on the child, with S_g in the place of seed and i in the place
 *     of cand: anneal_sweeps sweeps over inv_temp with the best state kept, then the descent up to max_descent_sweeps.
 *     It is the same device code.
 *  6. replace.  c = cut(improved child), scored as above.  Plane g & 1 gets, in slot i, the improved child and c iff
 *     c >= prev's cut of slot i, else a and its cut, both unchanged.  A tie goes to the child.  A slot's cut never
 *     falls from plane to plane.
 * Finish: the pick of gmc_refine_local_f32 (strictly best, first slot on ties) over plane G & 1: best_assign [R] int32,
 * best_cut [B], best_idx [B].  history [G+1][B] (NULL: not written): history[g] = the best cut of the plane generation
 * g wrote (g = 0: of the scored input); it never decreases with g.  G = 0 scores and picks.
 * By construction: the three seeds feed different hash domains, so a generation's selection, crossover and annealing
 * draws are independent; a slot's result depends on its graph, the population of the graph, the slot index, the seed
 * and the schedule alone - not on the graph's place in the batch nor on the rest of the batch; and two parents that
 * differ by a renaming of the classes on the movable nodes give a child that equals a there.
 *
 * Arguments: order / cgoff / cptr gmc_round_order_host's for the same K (device); inv_temp [anneal_sweeps] and levels
 * [GMC_ANNEAL_LEVELS] as for gmc_kway_refine_anneal_f32 (either may be NULL when anneal_sweeps == 0).  Argument checks,
 * before any HIP call, in that call's order: a NULL required pointer (history aside) GMC_ERR_NULL, batch->abi
 * GMC_ERR_ABI, a NULL goff / rowptr / lcol GMC_ERR_NULL, K outside 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES, cands < 1,
 * a negative sweep count, anneal_sweeps >= 2^20, B < 0, generations < 0, generations >= 2^20 or elite < 1
 * GMC_ERR_SHAPE, anneal_sweeps > 0 with a NULL inv_temp or levels GMC_ERR_NULL, n_max outside K..GMC_MAX_GRAPH_NODES
 * GMC_ERR_GRAPH_SIZE; B == 0 returns GMC_OK without a launch.  A graph with fewer than K or more than n_max nodes inside
 * a batch is skipped: nothing of it is written, history included.
 * One 256-thread workgroup per (slot, graph); every workgroup ranks the `cands` cuts of its graph itself, so a
 * generation is ONE launch and the call issues generations + 2: the scoring, the generations, the pick.  The LDS of a
 * generation's launch is gmc_kway_refine_anneal_f32's (gmc_refine_anneal_staged answers for this call too): parent b
 * lives in the best-state bytes and O, pi and the picks in the level table's until the crossover is done.  The
 * ranking costs cands^2 / 256 compares per thread of a workgroup.  The call allocates nothing and does not
 * synchronise; no float atomics (the counts of step 3 are integer LDS atomics: any order gives the same counts), no
 * communication between workgroups inside a launch, bitwise reproducible. */
int gmc_kway_evolve_f32(const gmc_batch *batch, int32_t K, const int32_t *order, const int32_t *cgoff,
                        const int32_t *cptr, int32_t cands, int8_t *pop /*[2][cands][R]*/,
                        float *cut /*[2][B][cands]*/, int32_t generations, int32_t elite, const float *inv_temp,
                        int32_t anneal_sweeps, const float *levels, uint64_t seed, int32_t max_descent_sweeps,
                        int32_t *best_assign, float *best_cut, int32_t *best_idx, float *history /*or NULL*/,
                        gmc_stream_t stream);

/* ---- one-flip tabu search over decoded partitions (extension; K = 2 .. GMC_KWAY_MAX_CLASSES) --------------------------
 *
 * The annealing proposes random moves under a temperature and remembers nothing.  This stage is the other classic move
 * rule of the max-cut literature: every iteration takes the BEST single move, forbids moving that node again for a
 * while (the tenure), and lets a move that would beat the best cut seen so far override the ban (aspiration).
 *
 * One chain is one (candidate `cand`, graph) pair and is independent of every other chain.  first = terminals ? K : 0;
 * the movable nodes are the local ids first..n-1 and n_mov = n - first.  All float arithmetic is fp32 and every step
 * named below is ONE fp32 operation (no multiply occurs, so no fused multiply-add can arise).  Integer arithmetic on
 * uint64 is modulo 2^64; GOLD = 0x9E3779B97F4A7C15 and mix64 are those of gmc_refine_anneal_f32.
 *
 * Table.  W[v][k], k = 0..K-1, v = 0..n-1: the sum, in the CSR order of v's row, of the weights of v's edges to
 *   neighbours of class k, starting from +0.0f; self-loops skipped, unit weights when batch->vals is NULL (the sums of
 *   gmc_kway_refine_anneal_f32, the same code).  Computed once, from the input state.  A class byte outside 0..K-1
 *   counts for no class (it adds to no sum and receives no update), and a movable node that holds one never moves:
 *   it keeps its byte.  (The annealing moves such a node at once; here it is inert.  The Python wrappers pass none.)
 * Running values.  rel = 0.0f (the sum of the gains taken), best = 0.0f, best_it = 0, snapshot = the input state,
 *   until[v] = 0 for every v.
 * Iteration it = 0..iterations-1:
 *   1. h = mix64(seed + GOLD * (((uint64)cand << 32 | it) + 1));  r = (uint32)h mod n_mov;
 *      span = tenure_span + (tenure_div > 0 ? n_mov / tenure_div : 0)  (integer division);
 *      tenure = tenure_base + (uint32)(h >> 32) mod (span + 1).
 *   2. For every movable v whose byte c = class(v) is in 0..K-1 and every k != c:  gain = W[v][c] - W[v][k].  The move
 *      (v, k) is admissible iff until[v] <= it, or rel + gain > best.
 *   3. Among the admissible moves the largest gain wins (compared as floats); ties go to the smallest
 *      rank = (v - first - r) mod n_mov (v - first - r + n_mov when negative), then to the smallest k.  With no
 *      admissible move the iteration moves nothing and steps 4 and 5 are skipped.
 *   4. class(v) = k.  For every edge (v, u, w) of v's row with u != v:  W[u][c] = W[u][c] - w, W[u][k] = W[u][k] + w.
 *      Then rel = rel + gain and until[v] = it + 1 + tenure (as an unbounded integer).
 *   5. If rel > best:  best = rel, best_it = it + 1, and the snapshot becomes the state.
 * Result.  The snapshot goes back into `assign`; best_iter [B][cands] (or NULL) receives best_it and moves [B][cands]
 *   (or NULL) the number of iterations that moved a node.  Every candidate is then scored as gmc_refine_local_f32
 *   scores (fp32, the same code, the same bits the sampler, the local search and the annealing report for the same
 *   bytes) into cut_all [B][cands], and picked as it picks (strictly best, first on ties): best_assign [R] int32,
 *   best_cut [B], best_idx [B].  iterations == 0 scores and picks only.
 * A row must hold a neighbour at most once (a simple graph, self-loops aside): the updates of step 4 are made by one
 *   lane per edge without atomics.  For a row that repeats a neighbour nothing is claimed.
 * By construction.  For unit and integer weights every sum is exact while it stays below 2^24 in magnitude; the cut of
 *   the result is then the input's cut plus `best`, so it is never below the input's, and when best_it < iterations
 *   the result is a local optimum under single moves of its movable nodes (a move of positive gain from the best
 *   state is admissible by aspiration and would have been taken at iteration best_it).  For other weights the table drifts by rounding:
 *   the result is then whatever the recount says and nothing stronger is claimed.  A chain depends on its graph, the
 *   input bytes, cand, seed and the five parameters - not on the batch, the graph's place in it, or cands.
 *
 * Argument checks, before any HIP call, in the order of gmc_kway_refine_anneal_t_f32: a NULL required pointer
 * (best_iter and moves aside) GMC_ERR_NULL, batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol GMC_ERR_NULL, K outside
 * 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES, cands < 1, iterations < 0 (so iterations < 2^31), a negative tenure
 * argument, B < 0 or terminals outside {0, 1} GMC_ERR_SHAPE, n_max < max(first, 1) or a batch gmc_kway_tabu_fits
 * refuses GMC_ERR_GRAPH_SIZE; B == 0 returns GMC_OK without a launch.  A graph with fewer than max(first, 1) or more
 * than n_max nodes inside a batch is skipped: nothing of it is written.
 *
 * One wave per chain; a 256-thread workgroup runs 4, 2 or 1 chains of one graph, as many as fit, which share one copy
 * of the graph's CSR in LDS when it fits beside them and read the batch's arrays otherwise (one code path over both).
 * With n_pad = n_max rounded up to 16 a chain keeps n_pad * (4 K + 6) bytes of LDS: W, until, the state and the
 * snapshot.  gmc_kway_tabu_fits is 1 iff n_max is in 1..GMC_MAX_GRAPH_NODES and n_pad * (4 K + 6) + 512 <= 160 KiB -
 * at K <= 8 that is every n_max up to GMC_MAX_GRAPH_NODES (K = 8: 4096 * 38 + 512 = 156,160 B) - else 0 (NULL
 * GMC_ERR_NULL, abi GMC_ERR_ABI, K GMC_ERR_CLASSES).  gmc_kway_tabu_shape tells what the launcher chose for a batch
 * and K: chains per workgroup (4, 2 or 1) + 16 if the CSR copy is staged in LDS; GMC_ERR_GRAPH_SIZE where
 * gmc_kway_tabu_fits is 0.  The call allocates nothing and does not synchronise: two launches on the caller's stream
 * (the chains, whose workgroups also score their snapshots; the pick), no atomics, no spin waits, no scratch, bitwise
 * reproducible. */
int gmc_kway_tabu_f32(const gmc_batch *batch, int32_t K, int32_t terminals, int32_t cands,
                      int8_t *assign /*[cands][R], in/out*/, int32_t iterations, int32_t tenure_base,
                      int32_t tenure_span, int32_t tenure_div, uint64_t seed, float *cut_all /*[B][cands]*/,
                      int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/, int32_t *best_idx /*[B]*/,
                      int32_t *best_iter /*[B][cands] or NULL*/, int32_t *moves /*[B][cands] or NULL*/,
                      gmc_stream_t stream);
int gmc_kway_tabu_fits(const gmc_batch *batch, int32_t K);
int gmc_kway_tabu_shape(const gmc_batch *batch, int32_t K);

/* ---- tabu search under class-size bounds (extension; K = 2 .. GMC_KWAY_MAX_CLASSES) ------------------------------------
 *
 * gmc_kway_tabu_f32 with a lower and an upper bound on the number of nodes of every class: max-bisection, balanced
 * max-K-cut and, on negated weights, balanced minimum cut.  It is the max-bisection tabu of the literature: a best move,
 * and where that move would break a bound, a best counter-move out of the class it entered.
 *
 * Everything of gmc_kway_tabu_f32 holds unchanged: fp32 throughout, every step ONE operation, no multiply; mix64, GOLD,
 * h, r, span and tenure of its step 1; the tie rank (v - first - r) mod n_mov; the table W[v][k] and its update on a
 * move (its step 4); first = terminals ? K : 0.
 *
 * Sizes.  size_lo and size_hi, int32 [B][K] in device memory: lo[c] and hi[c] of graph g are word g * K + c.
 *   s[c] = the number of nodes of the graph whose class byte is c, terminals included; m[c] = the same count over the
 *   movable nodes first..n-1.  A state is feasible iff lo[c] <= s[c] <= hi[c] for every class c, and
 *   V = sum over c of max(0, lo[c] - s[c]) + max(0, s[c] - hi[c]) is its violation.
 * Bounds admit a partition iff, with t = 1 under terminals and 0 without: lo[c] <= hi[c] and hi[c] >= t for every c, and
 *   sum of max(lo[c], t) <= n <= sum of hi[c] (sums as unbounded integers).  A graph whose bounds admit none is skipped as
 *   a graph of the wrong size is: nothing of it is written, by the chains or by the pick.  feasible [B] (or NULL)
 *   receives 0 for such a graph and 1 for a graph that ran; the word of a graph of the wrong size is not written.
 * Repair, before iteration 0 (also when iterations == 0).  While V > 0: among the moves (v: a -> b) of movable nodes v
 *   with a = class(v) in 0..K-1 and b != a for which da + db < 0, where
 *     da = -1 if s[a] > hi[a], +1 if s[a] <= lo[a], else 0;   db = -1 if s[b] < lo[b], +1 if s[b] >= hi[b], else 0
 *   (the move changes V by da + db), the largest gain = W[v][a] - W[v][b] wins, ties going to the smallest v - first,
 *   then to the smallest b; no bans, no hash.  The move is applied as tabu's step 4 (rel and until aside), s and m
 *   follow.  Under bounds that admit a partition and class bytes in 0..K-1 such a move exists while V > 0 (a class over
 *   its bound: some other class has room; otherwise some class sits above max(lo, t) and can give), every move lowers V
 *   by 1 or 2 (the largest gain decides, not the larger drop), so the repair ends within V <= 2 n moves; it also ends
 *   when no such move exists.  The repaired state is the base of the search: rel = best = 0.0f, best_it = 0, the snapshot is the repaired state,
 *   until[v] = 0 for every v.  repairs [B][cands] (or NULL) receives the number of repair moves.
 * Iteration it = 0..iterations-1:
 *   1. as tabu's step 1.
 *   2. A move (v: a -> b), v movable, a = class(v) in 0..K-1, b != a, gain = W[v][a] - W[v][b], is FREE iff
 *      s[a] > lo[a] and s[b] < hi[b]; any other move is PAIRED and exists only if m[b] >= 1.  A free move is admissible
 *      iff until[v] <= it, or rel + gain > best; a paired move iff until[v] <= it (no aspiration: the state after it
 *      is not feasible).
 *   3. as tabu's step 3: the largest gain, then the smallest rank, then the smallest b.  With no admissible move the
 *      iteration moves nothing.
 *   4. The move is applied as tabu's step 4: class(v) = b, the table, rel = rel + gain, until[v] = it + 1 + tenure.
 *      After a free move s[a], m[a] lose one and s[b], m[b] gain one.  After a paired move the counter-move follows,
 *      chosen from the updated table: among the movable u != v with class(u) = b the largest
 *      gain' = W[u][b] - W[u][a] wins, ties going to the smallest rank of u; bans are ignored, and m[b] >= 1 says that
 *      u exists.  class(u) = a, the table follows, rel = rel + gain', until[u] = it + 1 + tenure (the same tenure).
 *      The sizes are then what they were.
 *   5. as tabu's step 5, once per iteration, after the counter-move if there was one.
 *   The state is feasible after the repair and after every iteration.  moves counts the iterations that moved a node.
 * Result.  As gmc_kway_tabu_f32: the snapshot goes back into `assign`, best_iter, moves (and repairs), every candidate
 *   scored into cut_all with the bits gmc_kway_tabu_f32 reports for the same bytes, and picked.  iterations == 0 repairs,
 *   scores and picks.  A class byte outside 0..K-1 is inert as in tabu and counts for no class; the Python wrappers pass
 *   none, and nothing is claimed about the feasibility of a chain that holds one.
 * By construction.  With lo[c] = 0 and hi[c] = n for every class every move is free and nothing is repaired: every
 *   output is then byte for byte gmc_kway_tabu_f32's.  Every candidate written is feasible, so the pick is.
 *
 * Argument checks, before any HIP call, in gmc_kway_tabu_f32's order and with its codes; size_lo and size_hi are required
 * pointers (NULL: GMC_ERR_NULL), best_iter, moves, repairs and feasible may be NULL.  The bounds themselves are device
 * data and are judged by the kernels, graph by graph.  The launcher, the LDS (n_pad * (4 K + 6) bytes per chain: the
 * sizes and bounds are wave-uniform registers), gmc_kway_balance_fits and gmc_kway_balance_shape are gmc_kway_tabu_f32's,
 * value for value.  Two launches on the caller's stream, no atomics, no spin waits, no scratch, bitwise reproducible. */
int gmc_kway_balance_f32(const gmc_batch *batch, int32_t K, int32_t terminals, int32_t cands,
                         int8_t *assign /*[cands][R], in/out*/, const int32_t *size_lo /*[B][K]*/,
                         const int32_t *size_hi /*[B][K]*/, int32_t iterations, int32_t tenure_base,
                         int32_t tenure_span, int32_t tenure_div, uint64_t seed, float *cut_all /*[B][cands]*/,
                         int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/, int32_t *best_idx /*[B]*/,
                         int32_t *best_iter /*[B][cands] or NULL*/, int32_t *moves /*[B][cands] or NULL*/,
                         int32_t *repairs /*[B][cands] or NULL*/, int32_t *feasible /*[B] or NULL*/,
                         gmc_stream_t stream);
int gmc_kway_balance_fits(const gmc_batch *batch, int32_t K);
int gmc_kway_balance_shape(const gmc_batch *batch, int32_t K);

/* ---- the rounding and the K-class local search beyond GMC_MAX_GRAPH_NODES (extension) ---------------------------------
 *
 * gmc_round_conditional_f32 and gmc_kway_refine_anneal_f32 keep a graph's state in one workgroup's LDS and stop at
 * GMC_MAX_GRAPH_NODES.  The entry points below run the same two rules on graphs of K .. GMC_LARGE_MAX_GRAPH_NODES nodes,
 * a graph shared by several workgroups and its state kept in global memory:
 *  - gmc_large_round_conditional_f32: steps 1-5 of the gmc_round_conditional_f32 comment above, unchanged;
 *  - gmc_large_local_search_f32: the descent of gmc_kway_refine_anneal_f32 with anneal_sweeps = 0 on ONE candidate per
 *    graph (assign [R], in/out), "a byte outside 0..K-1 on a movable node: always moves" included.
 * Every node's sums are taken by one thread over its CSR row in order by the functions the one-workgroup kernels call, so
 * on every batch those kernels take as well, for the same sweep limit: assign and sweeps are byte for byte theirs; cut is
 * bit-equal for unit weights (every partial sum is an integer below 2^24) and agrees to rounding for real weights;
 * expected agrees to rounding.  All outputs are reproducible run to run, and a graph's outputs do not depend on what
 * else is in the batch.  What differs:
 *  - sizes: n_max in K .. GMC_LARGE_MAX_GRAPH_NODES; rows are read by batch row id and neighbours through gcol, so
 *    batch->gcol is required (a self-loop is gcol[e] == the row);
 *  - the order arrays: gmc_large_round_order_host's (gmc_round_order_host's on every batch that one accepts), in device
 *    memory, with max_classes, the largest class count of any graph, which tells the call how many colour launches to
 *    issue (a larger value costs launches and changes nothing; a smaller one leaves colours unvisited);
 *  - the workspace: gmc_large_round_workspace_bytes(batch, K) bytes of device memory, 16-byte aligned, NOT assumed
 *    zeroed (every word read is written by the call first): 3 B + 1 int words (per graph moved / stopped / sweeps run,
 *    one word "every graph has stopped") and R / 256 + B + 1 float partials, each of the two padded to 16 bytes, then
 *    R class bytes (0xff: a movable node not rounded yet), padded likewise - about 1.02 bytes per row;
 *  - the summation order of cut and expected: one partial per row (its edges in CSR order), a tile of 256 rows of the
 *    graph by a butterfly per wave and the four waves ascending, a graph's tiles ascending, then * 0.5f (the order of
 *    gmc_large_forward's loss);
 *  - the launches, all on the caller's stream, kernel boundaries being the only synchronisation between workgroups (no
 *    atomics, no spin waits): 1 (init) + 2 with expected + max_classes (rounding; none for the local search) +
 *    max_sweeps * (max_classes + 1) (a launch per colour, one closing the sweep) + 2 (score).  The call does not
 *    synchronise with the host, so ALL max_sweeps * (max_classes + 1) descent launches are issued whenever the descent
 *    converges; the threads of a graph that has stopped return at once, and once every graph has stopped a launch
 *    returns after reading one word.  A caller who knows the descent to be short passes a small max_sweeps.
 * Argument checks, before any HIP call: a NULL required pointer (workspace included; expected and sweeps may be NULL)
 * GMC_ERR_NULL, batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol / gcol GMC_ERR_NULL, K outside
 * 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES, a negative sweep count, max_classes < 0 or B < 0 GMC_ERR_SHAPE, n_max < K or
 * n_max > GMC_LARGE_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE, a workspace below gmc_large_round_workspace_bytes
 * GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a launch.  A graph with fewer than K or more than n_max nodes inside
 * a batch is skipped (nothing of it is written).  The probe shows one GMC_K_REFINE record per call. */

/* HOST routine (all pointers are host pointers): gmc_round_order_host for graphs of up to GMC_LARGE_MAX_GRAPH_NODES nodes
 * - the same first-fit colouring, arrays and argument checks; on a batch gmc_round_order_host accepts, the same three
 * arrays, array for array.  max_classes (required: NULL is GMC_ERR_NULL) receives the largest class count of any graph,
 * 0 for B == 0. */
int gmc_large_round_order_host(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol, int32_t K,
                               int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap, int32_t *max_classes);

/* bytes of workspace the two calls below need (0 for a NULL struct, another abi word, K outside 2..8 or negative sizes);
 * host only, reads B and R */
size_t gmc_large_round_workspace_bytes(const gmc_batch *batch, int32_t K);

int gmc_large_round_conditional_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K,
                                    const int32_t *order, const int32_t *cgoff, const int32_t *cptr, int32_t max_classes,
                                    int32_t max_descent_sweeps, void *workspace, size_t workspace_bytes,
                                    int8_t *assign /*[R]*/, float *cut /*[B]*/, float *expected /*[B] or NULL*/,
                                    int32_t *sweeps /*[B] or NULL*/, gmc_stream_t stream);

int gmc_large_local_search_f32(const gmc_batch *batch, int32_t K, const int32_t *order, const int32_t *cgoff,
                               const int32_t *cptr, int32_t max_classes, int32_t max_sweeps, void *workspace,
                               size_t workspace_bytes, int8_t *assign /*[R], in/out: one candidate per graph*/,
                               float *cut /*[B]*/, int32_t *sweeps /*[B] or NULL*/, gmc_stream_t stream);

/* ---- the seeded sampler and the annealing beyond GMC_MAX_GRAPH_NODES (extension) ---------------------------------------
 *
 * gmc_kway_decode_sample_seeded_f32 and gmc_kway_refine_anneal_f32 keep a graph's class bytes in one workgroup's LDS.
 * The two entry points below run the same rules at K = 2 .. GMC_KWAY_MAX_CLASSES on graphs of K ..
 * GMC_LARGE_MAX_GRAPH_NODES nodes, in the manner of gmc_large_round_conditional_f32: a graph shared by several workgroups,
 * the state in a caller-owned workspace that is NOT assumed zeroed (every word read is written by the call first), kernel
 * boundaries the only synchronisation between workgroups (no atomics, no spin waits), rows read by batch row id and
 * neighbours through gcol (batch->gcol is required), the order arrays and max_classes those of
 * gmc_large_round_order_host in device memory.  All outputs are reproducible run to run and a graph's outputs do not
 * depend on what else is in the batch.
 *
 * gmc_large_anneal_f32: steps 1-4 of gmc_kway_refine_anneal_f32 per (candidate, graph), unchanged - the initial score,
 * anneal_sweeps sweeps over the colour classes with that comment's move test, after each sweep a recount and a snapshot
 * on a strictly larger cut, the descent from the snapshot until a sweep moves nothing or max_descent_sweeps have run (the
 * stop is kept per (candidate, graph)), then score and pick.  A node's sums are taken by one thread over its CSR row in
 * order by the functions the one-workgroup kernel calls; the unconditional move of a byte outside 0..K-1 is included.
 *  - The counter of the move test is chosen per graph from its own node count n, so a candidate's result depends on its
 *    graph alone:
 *        n <= GMC_MAX_GRAPH_NODES:  ctr = (uint64)cand << 32 | (uint64)s << 12 | v     (gmc_kway_refine_anneal_f32's)
 *        n >  GMC_MAX_GRAPH_NODES:  ctr = (uint64)cand << 40 | (uint64)s << 20 | v     (v < 2^20, s < 2^20, cand < 2^24)
 *    With the first layout beyond 4096 nodes, node v of sweep s would share its hash with node v - 4096 of sweep s + 1.
 *    anneal_sweeps >= 2^20 is GMC_ERR_SHAPE as before; cands >= 2^24 with n_max > GMC_MAX_GRAPH_NODES is GMC_ERR_SHAPE.
 *  - The summation order of every cut (the initial score, each sweep's recount, the final score) is
 *    gmc_large_round_conditional_f32's: one partial per row (its edges in CSR order), a tile of 256 rows of the graph by
 *    a butterfly per wave and the four waves ascending, a graph's tiles ascending, then * 0.5f.  Snapshot decisions
 *    compare these floats.  For unit and integer weights every partial is an integer below 2^24, so on every batch
 *    gmc_kway_refine_anneal_f32 takes as well assign, cut_all, best_*, snap_sweep and sweeps are byte for byte that
 *    call's.  For other weights cut_all agrees to rounding and a near-tie between a sweep's cut and the snapshot's may be
 *    decided differently.  With anneal_sweeps = 0 no cut is compared: each candidate's assignment and sweep count are
 *    gmc_large_local_search_f32's on that candidate alone, for any weights.
 *  - Launches, all on the caller's stream:
 *        5 + [anneal_sweeps > 0] * (2 + anneal_sweeps * (max_classes + 3)) + max_descent_sweeps * (max_classes + 1)
 *    (init; the first recount and fold; per annealing sweep a launch per colour, recount, fold, snapshot; per descent
 *    sweep a launch per colour and one closing it; score, fold, pick, copy).  The number never depends on data: as in
 *    gmc_large_round_conditional_f32 every descent launch is issued, the lanes of a (candidate, graph) that has stopped
 *    return at once, and once all have stopped a launch returns after reading one word.
 *  - Arguments and outputs are gmc_kway_refine_anneal_f32's (assign [cands][R] int8 in/out, cut_all [B][cands],
 *    best_assign [R] int32, best_cut [B], best_idx [B], optional snap_sweep / sweeps [B][cands]) plus max_classes and
 *    the workspace.  Argument checks, before any HIP call: a NULL required pointer (workspace included) GMC_ERR_NULL,
 *    batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol / gcol GMC_ERR_NULL, K outside 2..GMC_KWAY_MAX_CLASSES
 *    GMC_ERR_CLASSES, cands < 1, a negative sweep count, anneal_sweeps >= 2^20, max_classes < 0, B < 0 or the cands bound
 *    above GMC_ERR_SHAPE, anneal_sweeps > 0 with a NULL inv_temp or levels GMC_ERR_NULL, n_max outside
 *    K..GMC_LARGE_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE, a workspace below gmc_large_search_workspace_bytes(batch, K, cands)
 *    GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a launch.  A graph with fewer than K or more than n_max nodes
 *    inside a batch is skipped (nothing of it is written).  The probe shows one GMC_K_REFINE record per call.
 *
 * gmc_large_sample_seeded_f32: the K-class draw rule above, unchanged ((u64)it << 32 | l has room for 2^20 local ids), so
 * a graph's samples depend on its key alone and are gmc_kway_decode_sample_seeded_f32's.  Outputs as that call's; the
 * draws go to assign_all [iters][R] when it is given and live in the workspace either way; cut_all in the summation
 * order above (bit-equal to that call's for unit and integer weights); the pick is the strictly best sample, the first on
 * ties, and best_assign is regenerated from the hash.  Five launches.  Argument checks: a NULL pointer (assign_all
 * aside, workspace included) GMC_ERR_NULL, batch->abi GMC_ERR_ABI, a NULL goff / rowptr / lcol / gcol GMC_ERR_NULL, K
 * GMC_ERR_CLASSES, iters < 1 or B < 0 GMC_ERR_SHAPE, n_max outside K..GMC_LARGE_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE, a
 * workspace below gmc_large_search_workspace_bytes(batch, K, iters) GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a
 * launch; graphs outside K..n_max nodes are skipped.  The probe shows one GMC_K_SAMPLE record per call.
 *
 * The workspace, 16-byte aligned device memory, with cp = min(64, the next power of two >= cands) and cpad = cands
 * rounded up to a multiple of cp: 5 B cands + 1 int words (per (graph, candidate) moved / stopped / sweeps run / snapshot
 * sweep / "take a snapshot", one word "all have stopped"), B cands floats (the snapshot's cut), (R / 256 + B + 1) cpad
 * float partials, each of the three padded to 16 bytes, then twice cpad R class bytes (state and snapshot, row by row
 * the cp candidates of a chunk side by side), padded likewise: about 2.02 cpad bytes per row. */

/* bytes of workspace the two calls below need for `cands` candidates (the sampler: iterations); 0 for a NULL struct,
 * another abi word, K outside 2..8, cands < 1 or negative sizes; host only, reads B and R */
size_t gmc_large_search_workspace_bytes(const gmc_batch *batch, int32_t K, int32_t cands);

int gmc_large_sample_seeded_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K, const uint64_t *gkey,
                                int32_t iters, int8_t *assign_all /*[iters][R] or NULL*/, void *workspace,
                                size_t workspace_bytes, float *cut_all /*[B][iters]*/, int32_t *best_assign /*[R]*/,
                                float *best_cut /*[B]*/, int32_t *best_iter /*[B]*/, gmc_stream_t stream);

int gmc_large_anneal_f32(const gmc_batch *batch, int32_t K, const int32_t *order, const int32_t *cgoff,
                         const int32_t *cptr, int32_t max_classes, int32_t cands, int8_t *assign /*[cands][R], in/out*/,
                         const float *inv_temp, int32_t anneal_sweeps, const float *levels, uint64_t seed,
                         int32_t max_descent_sweeps, void *workspace, size_t workspace_bytes,
                         float *cut_all /*[B][cands]*/, int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/,
                         int32_t *best_idx /*[B]*/, int32_t *snap_sweep /*or NULL*/, int32_t *sweeps /*or NULL*/,
                         gmc_stream_t stream);

/* ---- building a batch on the device from directed entries -------------------------------------------------------------
 * The arrays of a gmc_batch from E directed entries (src[e], dst[e][, w[e]]): int32 global row ids in block-diagonal
 * numbering (graph g owns rows goff[g] .. goff[g+1]-1), both directions of every undirected edge present, a self-loop
 * once.  What the reference's data path builds with dgl.from_networkx per graph (graphExtender.py:102) and what this
 * library's host code builds from that (CSR sorted by column inside a row, dinv = 1/sqrt(max(deg,1)) with numpy's
 * float32 bits, the neighbour table in gmc_ell_arrange_host's slot order, the 8-entry overflow blocks): the same bytes.
 * All pointers are device memory; nothing is allocated, everything runs on the caller's stream, the workspace need not
 * be zeroed, kernel boundaries are the only synchronisation, no floating-point value is summed, and two builds of the
 * same entries in any order give the same bytes.
 *
 * gmc_batch_build_csr writes rowptr [R+1], gcol / lcol [E], vals [E] (exactly when w is given), dinv [R] and the report,
 * in 11 launches (init, count, the three-launch scan, scatter, four sorts by row length, validate).  The row sorts: up
 * to 8 entries 8 lanes, up to 64 a wave, up to 4096 a workgroup in LDS, beyond that one workgroup per row on global
 * memory - slow (a star of 2^20 - 1 leaves is legal; estimated, not measured: on the order of 0.1 s) and rare.  An entry with an id
 * outside 0..R-1, or with endpoints in two graphs, is counted in the report and skipped: it is never used as an index,
 * and the arrays then hold the report's GMC_BB_NNZ < E entries.  The caller reads the report (one device-to-host copy)
 * and decides: any of the first five words non-zero is bad input.
 *
 * gmc_batch_build_table writes the neighbour table ell [R][W] (W = 8 or 16, NS live slots as gmc_ell_slots_for says)
 * and ell_vals (exactly when vals is given), and - when ovf_ptr is given - ovf_ptr [R+1] and the overflow lists of
 * ovf_blocks blocks of eight (the report's GMC_BB_BLOCKS_8 / _16).  n_max: the largest graph, n_max + 4 <= 65535.
 *
 * Argument checks, before any HIP call: a NULL required pointer (workspace included) GMC_ERR_NULL; B < 0, R < B, E
 * outside 0..2^31-1, W, NS outside 1..W, ovf_blocks < 0 GMC_ERR_SHAPE; n_max GMC_ERR_GRAPH_SIZE; a workspace below
 * gmc_batch_build_workspace_bytes(B, R, E) GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a launch. */
enum {
    GMC_BB_OUT_OF_RANGE = 0,    /* entries with an id outside 0..R-1 (skipped) */
    GMC_BB_CROSS_GRAPH = 1,     /* entries whose endpoints lie in two graphs (skipped) */
    GMC_BB_DUPLICATE = 2,       /* entries equal to their predecessor in the sorted row */
    GMC_BB_ASYMMETRIC = 3,      /* entries whose reverse is missing or has another weight */
    GMC_BB_ZERO_DEGREE = 4,     /* rows without entries */
    GMC_BB_MAX_DEGREE = 5,
    GMC_BB_ROWS_OVER_8 = 6,     /* rows longer than 8 / 16 entries, and the entries beyond */
    GMC_BB_ROWS_OVER_16 = 7,
    GMC_BB_EXCESS_8 = 8,
    GMC_BB_EXCESS_16 = 9,
    GMC_BB_ROW_BLOCKS_8 = 10,   /* most overflow blocks of a row / of a graph at either width */
    GMC_BB_ROW_BLOCKS_16 = 11,
    GMC_BB_GRAPH_BLOCKS_8 = 12,
    GMC_BB_GRAPH_BLOCKS_16 = 13,
    GMC_BB_BLOCKS_8 = 14,       /* overflow blocks of the whole batch */
    GMC_BB_BLOCKS_16 = 15,
    GMC_BB_NON_UNIT = 16,       /* weights that are not exactly 1.0 */
    GMC_BB_NNZ = 17,            /* entries kept: rowptr[R] */
    GMC_BB_NNZ_MAX = 18,        /* most entries of a graph */
    GMC_BB_REPORT_WORDS = 20
};

/* bytes of workspace either stage needs (about 16 R); 0 for negative sizes or E >= 2^31; host only */
size_t gmc_batch_build_workspace_bytes(int32_t B, int32_t R, int64_t E);

int gmc_batch_build_csr(int32_t B, int32_t R, int64_t E, const int32_t *goff /*[B+1]*/, const int32_t *src /*[E]*/,
                        const int32_t *dst /*[E]*/, const float *w /*[E] or NULL*/, int32_t *rowptr /*[R+1]*/,
                        int32_t *lcol /*[E]*/, int32_t *gcol /*[E]*/, float *vals /*[E], with w*/, float *dinv /*[R]*/,
                        int32_t *report /*[GMC_BB_REPORT_WORDS]*/, void *workspace, size_t workspace_bytes,
                        gmc_stream_t stream);

int gmc_batch_build_table(int32_t B, int32_t R, int32_t n_max, const int32_t *goff, const int32_t *rowptr,
                          const int32_t *lcol, const float *vals /*or NULL*/, int32_t W, int32_t NS,
                          uint16_t *ell /*[R][W]*/, float *ell_vals /*[R][W], with vals*/, int32_t *ovf_ptr /*[R+1] or NULL*/,
                          uint16_t *ovf_ids /*[8 ovf_blocks]*/, float *ovf_vals /*[8 ovf_blocks], with vals*/,
                          int32_t ovf_blocks, void *workspace, size_t workspace_bytes, gmc_stream_t stream);

/* ---- plain max-K-cut: the terminals optional ---------------------------------------------------------------------------
 * Everything above solves max-K-cut with local nodes 0..K-1 of every graph forced into classes 0..K-1 (the reference's
 * problem, TrainingNeural.py:87-94).  The entry points below are the ones above with one more argument, `terminals`,
 * directly after the class count (after `model` for the instance calls): 1 runs exactly what the entry point without
 * the `_t` runs - the same kernels, the same bytes on every output - and 0 solves the problem without terminals, the
 * standard max-K-cut.  The flag is a run-time argument of the same kernels: first = terminals ? K : 0 is the first
 * movable local id, and every rule above that says "l < K" reads "l < first".  With terminals = 0:
 *
 *   - rounding, step 1: every node's q is its row of P (no node starts as a unit vector); every node is visited;
 *   - the sampler's draw rule applies to every local id, with the same counter (iteration, local id);
 *   - annealing, local search and descent: every node is movable; the counters (the wide one of graphs beyond
 *     GMC_MAX_GRAPH_NODES included) and the level table are unchanged;
 *   - the head of the instance calls: no row is overridden, S is the first maximum on every row, and both losses (and
 *     their gradients) are those of gmc_fn_cut_loss_f32 with terminals = 0;
 *   - order / cgoff / cptr come from gmc_order_host_t with the same K and terminals: `order` then holds all R rows;
 *   - a graph needs one node, not K: the lower bound of GMC_ERR_GRAPH_SIZE is n_max >= 1.
 *
 * Checks and status codes are those of the entry point without the `_t`, in its order; terminals outside {0, 1} is
 * GMC_ERR_SHAPE, reported where that entry point reports its other shape errors.  The workspace queries are shared: no
 * size depends on the flag.
 *
 * gmc_order_host_t is a HOST routine (host pointers): gmc_large_round_order_host with first = terminals ? K : 0, for
 * graphs of up to GMC_LARGE_MAX_GRAPH_NODES nodes (the one-workgroup calls then refuse what is too large for them).
 * `order` receives R - first * B entries.  With terminals = 1 it writes what gmc_round_order_host and
 * gmc_large_round_order_host write, array for array.  NULL (max_classes included) GMC_ERR_NULL, K GMC_ERR_CLASSES,
 * terminals GMC_ERR_SHAPE, then the checks of gmc_large_round_order_host. */
int gmc_order_host_t(int32_t B, const int32_t *goff, const int32_t *rowptr, const int32_t *lcol, int32_t K,
                     int32_t terminals, int32_t *order, int32_t *cgoff, int32_t *cptr, int32_t cptr_cap,
                     int32_t *max_classes);

int gmc_round_conditional_t_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K, int32_t terminals,
                                const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                                int32_t max_descent_sweeps, int8_t *assign /*[R]*/, float *cut /*[B]*/,
                                float *expected /*[B] or NULL*/, int32_t *sweeps /*[B] or NULL*/, gmc_stream_t stream);

int gmc_kway_decode_sample_seeded_t_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K, int32_t terminals,
                                        const uint64_t *gkey /*[B]*/, int32_t iters,
                                        int8_t *assign_all /*[iters][R] or NULL*/, float *cut_all /*[B][iters]*/,
                                        int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/,
                                        int32_t *best_iter /*[B]*/, gmc_stream_t stream);

int gmc_kway_refine_anneal_t_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const int32_t *order,
                                 const int32_t *cgoff, const int32_t *cptr, int32_t cands,
                                 int8_t *assign /*[cands][R], in/out*/, const float *inv_temp, int32_t anneal_sweeps,
                                 const float *levels, uint64_t seed, int32_t max_descent_sweeps,
                                 float *cut_all /*[B][cands]*/, int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/,
                                 int32_t *best_idx /*[B]*/, int32_t *snap_sweep /*or NULL*/, int32_t *sweeps /*or NULL*/,
                                 gmc_stream_t stream);

int gmc_large_round_conditional_t_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K, int32_t terminals,
                                      const int32_t *order, const int32_t *cgoff, const int32_t *cptr,
                                      int32_t max_classes, int32_t max_descent_sweeps, void *workspace,
                                      size_t workspace_bytes, int8_t *assign /*[R]*/, float *cut /*[B]*/,
                                      float *expected /*[B] or NULL*/, int32_t *sweeps /*[B] or NULL*/,
                                      gmc_stream_t stream);

int gmc_large_local_search_t_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const int32_t *order,
                                 const int32_t *cgoff, const int32_t *cptr, int32_t max_classes, int32_t max_sweeps,
                                 void *workspace, size_t workspace_bytes, int8_t *assign /*[R], in/out*/,
                                 float *cut /*[B]*/, int32_t *sweeps /*[B] or NULL*/, gmc_stream_t stream);

int gmc_large_sample_seeded_t_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K, int32_t terminals,
                                  const uint64_t *gkey, int32_t iters, int8_t *assign_all /*[iters][R] or NULL*/,
                                  void *workspace, size_t workspace_bytes, float *cut_all /*[B][iters]*/,
                                  int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/, int32_t *best_iter /*[B]*/,
                                  gmc_stream_t stream);

int gmc_large_anneal_t_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const int32_t *order,
                           const int32_t *cgoff, const int32_t *cptr, int32_t max_classes, int32_t cands,
                           int8_t *assign /*[cands][R], in/out*/, const float *inv_temp, int32_t anneal_sweeps,
                           const float *levels, uint64_t seed, int32_t max_descent_sweeps, void *workspace,
                           size_t workspace_bytes, float *cut_all /*[B][cands]*/, int32_t *best_assign /*[R]*/,
                           float *best_cut /*[B]*/, int32_t *best_idx /*[B]*/, int32_t *snap_sweep /*or NULL*/,
                           int32_t *sweeps /*or NULL*/, gmc_stream_t stream);

int gmc_inst_forward_t(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C, void *workspace,
                       size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream);

int gmc_inst_train_fwd_bwd_t(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C,
                             void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad,
                             gmc_stream_t stream);

/* ---- pinning any nodes to classes: contraction on the device -----------------------------------------------------------
 * `terminals = 1` above means "local nodes 0..K-1 of every graph sit in classes 0..K-1".  Any other set of pinned nodes
 * (several per class, anywhere in the graph) is brought to that form by contracting every node pinned to class c into one
 * super-node c.  The rule, for graph g with n nodes, pinned set Pi with classes c(u), and free nodes F = V \ Pi in
 * ascending local id:
 *
 *   size         n' = K + |F| nodes.
 *   numbering    local id c is the super-node of class c; the free node of rank r in F gets local id K + r.
 *   node_map     node_map[row] = goff'[g] + (c(u) if pinned else K + rank), goff'[g] = K g + free rows before graph g.
 *   free-free    an entry (v, x, w) with both ends free is kept as (v', x', w); a self-loop on a free node is kept once.
 *   free-pinned  for a free v and a class c with at least one entry (v, u), u in Pi_c, the two entries (v', c, s) and
 *                (c, v', s): s is the float32 sum that starts at +0 and adds those entries' weights one after the other
 *                in ascending u (for unit weights: their count).  s is computed once and stored twice - both directions
 *                carry the same bits, as gmc_batch_build_csr demands - and the entries are kept whatever s is, 0 from
 *                signed weights included.
 *   pinned-pinned  no entry, and no self-loop on a pinned node.
 *   fixed_cut[g] the sum of w over undirected edges {u, x} with both ends pinned and c(u) != c(x), each edge once, in
 *                this order: (1) per pinned row u, t_u = +0 plus the weights of its entries (u, x) with x pinned, x > u
 *                and c(x) != c(u), one after the other in ascending x (free rows: t_u = 0); (2) per tile of 256
 *                consecutive rows of the graph, the first tile starting at the graph's first row (rows beyond the graph:
 *                0): the 64 values of each quarter are summed by a butterfly - v[i] <- v[i] + v[i ^ d] for d = 32, 16, 8,
 *                4, 2, 1 - and the four quarter sums q0..q3 give the tile's partial ((q0 + q1) + q2) + q3; (3) the graph's
 *                partials are added to +0 one after the other in ascending tile order.  All in float32.
 *
 * For every assignment p' of g' with p'[c] = c, cut_g(lift(p')) = cut_g'(p') + fixed_cut[g], lift(p')[row] =
 * p'[node_map[row]]: exact for integer weights while every sum stays below 2^24, to rounding otherwise.  The contracted
 * graph is what the library solves with terminals = 1.  A class without a pinned node in some graph (a graph without pins
 * included) has no super-node to stand for: that is bad input here, as is a super-node without a free neighbour (every
 * GraphConv path refuses its zero-degree row).
 *
 * Both stages read the sorted CSR of a gmc_batch (goff, rowptr, gcol, vals or NULL; B, R, nnz, n_max; n_max up to
 * GMC_LARGE_MAX_GRAPH_NODES), so "ascending u" is a row's own order.  All pointers are device memory; nothing is
 * allocated; the workspace is caller-owned, need not be zeroed, and carries the class words and offsets from
 * gmc_contract_map to gmc_contract_entries (the same buffer, untouched in between); kernel boundaries are the only
 * synchronisation; no scratch, no floating-point atomics; any order of the pin list gives the same bytes.
 *
 * gmc_contract_map (7 launches: init, pins, count, a three-launch scan, finish) takes P pins (pin_node[p] a global row
 * id, pin_class[p] its class), sets every row's class word from "free" with an integer compare-and-swap - a repeated
 * identical pin is harmless - ranks the free rows per graph, counts and places every row's output entries, and writes
 * node_map [R], goff_out [B+1] and the report.  The caller reads the report (one device-to-host copy) and decides: any of
 * the first six words non-zero is bad input, and GMC_CT_NNZ is the E' <= nnz that sizes gmc_contract_entries' outputs.
 *
 * gmc_contract_entries (2 launches) writes the E' directed entries of the rule (src_out, dst_out as global ids of the
 * contracted batch, w_out always, 1.0 for a batch without vals) in an order that is fixed for a given batch and pin set
 * and otherwise of no account - gmc_batch_build_csr gives the same bytes for any order - and fixed_cut [B].  Entries at
 * positions >= E_out are not written.  Row-length regimes: ONE - a thread walks its row's entries one after the other,
 * whatever the row's length, with the K running sums in registers, so the sum order above holds by construction.  A free
 * hub row therefore costs its length in dependent loads on one thread (a star of 2^20 - 1 leaves: see DESIGN.md
 * section 31); the workloads here have short rows.
 *
 * Argument checks, before any HIP call, in this order: a NULL batch or required pointer (workspace included; the pin
 * arrays when P > 0, the entry arrays when E_out > 0) GMC_ERR_NULL; batch->abi GMC_ERR_ABI; a NULL goff / rowptr / gcol
 * (gcol: with nnz > 0) GMC_ERR_NULL; K outside 2..GMC_KWAY_MAX_CLASSES GMC_ERR_CLASSES; a negative B, R, nnz, n_max, P or E_out GMC_ERR_SHAPE;
 * n_max beyond GMC_LARGE_MAX_GRAPH_NODES GMC_ERR_GRAPH_SIZE; a workspace below gmc_contract_workspace_bytes(B, R, nnz, K)
 * GMC_ERR_WORKSPACE; B == 0 returns GMC_OK without a launch. */
enum {
    GMC_CT_PIN_OUT_OF_RANGE = 0,      /* pins with a node id outside 0..R-1 (skipped, never used as an index) */
    GMC_CT_PIN_CLASS = 1,             /* pins with a class outside 0..K-1 (skipped) */
    GMC_CT_PIN_CONFLICT = 2,          /* nodes that were given two different classes */
    GMC_CT_GRAPHS_MISSING_CLASS = 3,  /* graphs in which some class has no pinned node */
    GMC_CT_GRAPHS_NO_FREE = 4,        /* graphs without a free node */
    GMC_CT_BARE_TERMINALS = 5,        /* (graph, class) pairs with pinned nodes none of which has a free neighbour */
    GMC_CT_NNZ = 6,                   /* E': directed entries of the contracted batch, <= nnz */
    GMC_CT_PINNED = 7,                /* pinned rows */
    GMC_CT_REPORT_WORDS = 8
};

/* bytes of workspace both stages need (about 20 R + 12 B); 0 for negative sizes, E >= 2^31 or K outside 2..8; host only */
size_t gmc_contract_workspace_bytes(int32_t B, int32_t R, int64_t E, int32_t K);

int gmc_contract_map(const gmc_batch *batch, int32_t K, int64_t P, const int32_t *pin_node /*[P]*/,
                     const int32_t *pin_class /*[P]*/, int32_t *node_map /*[R]*/, int32_t *goff_out /*[B+1]*/,
                     int32_t *report /*[GMC_CT_REPORT_WORDS]*/, void *workspace, size_t workspace_bytes,
                     gmc_stream_t stream);

int gmc_contract_entries(const gmc_batch *batch, int32_t K, const int32_t *node_map /*[R]*/,
                         const int32_t *goff_out /*[B+1]*/, int64_t E_out, int32_t *src_out /*[E_out]*/,
                         int32_t *dst_out /*[E_out]*/, float *w_out /*[E_out]*/, float *fixed_cut /*[B]*/,
                         void *workspace, size_t workspace_bytes, gmc_stream_t stream);

/* ---- per-node class costs: a linear term in the objective ---------------------------------------------------------------
 * Everything above maximises the pairwise objective cut(S) = sum over undirected edges {u,v} of w_uv [S_u != S_v].  The
 * entry points below are `_t` entry points with one more argument, `node_cost`, directly after `terminals`: [R][K] fp32
 * device memory, row-major, indexed by BATCH ROW (the row goff[g] + l of local node l of graph g), or NULL.  They serve
 *
 *   obj(S) = cut(S) - sum_v node_cost[v][S_v]
 *
 * the sum over every node of the graph, terminals included (their share is a constant of the graph); a class byte outside
 * 0..K-1 adds no cost, as it adds to no class sum.  A QUBO or an Ising model with fields is this objective at K = 2
 * (DESIGN.md section 33 has the two changes of variables).  With node_cost == NULL every `_c` entry point IS its `_t` twin
 * - the `_t` entry points are these calls with NULL - the same kernels, the same bytes on every output.  With a cost
 * the sampler and the head run the same instantiations (node_cost is a run-time pointer of theirs); the annealing and
 * the rounding launch a second kernel compiled from the same body text with the cost switched on
 * (anneal_k_cost_kernel<K>, round_conditional_cost_kernel<K>), so that the kernels of the NULL call keep, instruction
 * for instruction, the code they had (DESIGN.md section 33 has the measurements behind that).  The cost is read from
 * global memory (K loads per visit), never staged in LDS: the LDS of every launch is what it was.  No float atomics,
 * no scratch, bitwise reproducible.  Argument checks and status codes
 * are the `_t` twin's, in its order; node_cost is optional and its contents are never checked (a NaN or an infinity in it
 * behaves as it would in an edge weight).  The rules, operation by operation:
 *
 * 1. Class sums (annealing, local search / descent; move_body.h).  The K sums of a visit of local node v of the graph on
 *    rows r0.. start from node_cost[r0 + v][k] instead of +0.0f; the row's edges are then added in CSR order exactly as
 *    before.  Everything derived from the sums is unchanged: the smallest sum and the smallest among the others (lowest
 *    index on ties), the Metropolis test delta = W[kk] - W[c] against the level table, the descent's strict "<".  The same
 *    holds for the rounding's M_k (round_body.h): M_k starts from node_cost[r0 + v][k], and product and sum of every
 *    edge term stay separately rounded.  An all-+0.0f node_cost therefore gives the NULL call's bytes on every output.
 *
 * 2. Scores.  Wherever a state is scored - the sampler's cut_all, the rounding's cut, the annealing's best-state
 *    bookkeeping (the snapshot is taken when the OBJECTIVE improved) and its final cut_all, and so the input of every
 *    pick - the score is block_cut(...) - block_cost(...), one fp32 subtraction, not fused with the cut's halving:
 *    block_cut is the count stated above (edge-parallel, each edge twice, halved); block_cost sums node_cost[r0 + l][S_l]
 *    (nothing for a byte outside 0..K-1) over the rows l = t, t + 256, ... of thread t from +0, then the wave's butterfly
 *    (v[i] += v[i ^ d], d = 32 .. 1), then the four wave sums as ((q0 + q1) + q2) + q3 - block_cut's order (cut_body.h).
 *    best_cut / cut outputs hold that score; the plain cut of a returned state is score + its cost.
 *
 * 3. The rounding's `expected` output becomes the expected objective: the expected cut as before, minus the expected cost
 *    sum_v sum_k node_cost[v][k] q_v[k], q the state the rounding starts from (terminal rows e_l).  Order: per row
 *    t_v = +0 then + node_cost[v][k] * q_v[k] for k ascending, product and sum separately rounded; the rows l = t, t + 256,
 *    ... of thread t added from +0; butterfly; ((q0 + q1) + q2) + q3; then one fp32 subtraction from the (halved) expected
 *    cut.  obj(rounded) >= expected objective holds as before: the linear term is separable, so a visit that takes the
 *    smallest M_k (cost included) does not lower the conditional expectation; the descent never lowers obj.
 *
 * 4. Head of the instance calls (head_k_kernel).  gp[k] of row u starts from node_cost[u][k] before the edge loop, so
 *    GP_u = C (sum_v w_uv Pt_v + node_cost_u) (hard loss: Pt_v = e_{S_v}); the loss is -C (cut - costsum) with costsum =
 *    sum_u node_cost_u . Pt_u for GMC_LOSS_EXPECTED_CUT (Pt: P with the terminal rows overridden) and sum_u
 *    node_cost[u][S_u] for the hard loss.  Summation: row u adds (cut_u - 2 cost_u) to the accumulator that held cut_u
 *    (cut_u the row's doubled share, cost_u = the k-ascending dot product, or the one selected entry), and the block sum
 *    and the halving are the ones that were: one reduction, no extra LDS.  The softmax backward, db2, GY2 and everything
 *    downstream follow from gp unchanged.  The 3-class fused head and the gmc_inst_large_* sequence take no cost. */
int gmc_round_conditional_c_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K, int32_t terminals,
                                const float *node_cost /*[R][K] or NULL*/, const int32_t *order, const int32_t *cgoff,
                                const int32_t *cptr, int32_t max_descent_sweeps, int8_t *assign /*[R]*/,
                                float *cut /*[B]*/, float *expected /*[B] or NULL*/, int32_t *sweeps /*[B] or NULL*/,
                                gmc_stream_t stream);

int gmc_kway_decode_sample_seeded_c_f32(const gmc_batch *batch, const float *P /*[R,K]*/, int32_t K, int32_t terminals,
                                        const float *node_cost /*[R][K] or NULL*/, const uint64_t *gkey /*[B]*/,
                                        int32_t iters, int8_t *assign_all /*[iters][R] or NULL*/,
                                        float *cut_all /*[B][iters]*/, int32_t *best_assign /*[R]*/,
                                        float *best_cut /*[B]*/, int32_t *best_iter /*[B]*/, gmc_stream_t stream);

int gmc_kway_refine_anneal_c_f32(const gmc_batch *batch, int32_t K, int32_t terminals,
                                 const float *node_cost /*[R][K] or NULL*/, const int32_t *order, const int32_t *cgoff,
                                 const int32_t *cptr, int32_t cands, int8_t *assign /*[cands][R], in/out*/,
                                 const float *inv_temp, int32_t anneal_sweeps, const float *levels, uint64_t seed,
                                 int32_t max_descent_sweeps, float *cut_all /*[B][cands]*/, int32_t *best_assign /*[R]*/,
                                 float *best_cut /*[B]*/, int32_t *best_idx /*[B]*/, int32_t *snap_sweep /*or NULL*/,
                                 int32_t *sweeps /*or NULL*/, gmc_stream_t stream);

int gmc_inst_forward_c(const gmc_batch *batch, const gmc_model *model, int32_t terminals,
                       const float *node_cost /*[R][K] or NULL*/, float C, void *workspace, size_t workspace_bytes,
                       float *P, int32_t *S, float *loss, gmc_stream_t stream);

int gmc_inst_train_fwd_bwd_c(const gmc_batch *batch, const gmc_model *model, int32_t terminals,
                             const float *node_cost /*[R][K] or NULL*/, float C, void *workspace, size_t workspace_bytes,
                             float *P, int32_t *S, float *loss, float *grad, gmc_stream_t stream);

/* out[r] = the float32 sum that starts at +0 and adds the weights of row r's entries one after the other in the row's
 * (sorted) CSR order, the entry on the diagonal (gcol[e] == r) skipped; vals == NULL: every weight is 1.  One thread per
 * row, one launch, no atomics: the order holds by construction.  (maxcut.solve_qubo takes sum_j q_ij from it.)  NULL rowptr
 * / out GMC_ERR_NULL; R < 0 GMC_ERR_SHAPE; R == 0 GMC_OK without a launch; NULL gcol GMC_ERR_NULL. */
int gmc_row_weight_sums_f32(int32_t R, const int32_t *rowptr /*[R+1]*/, const int32_t *gcol /*[nnz], global row ids*/,
                            const float *vals /*[nnz] or NULL*/, float *out /*[R]*/, gmc_stream_t stream);

/* ---- per-node class costs in the two chain searches (extension) -----------------------------------------------------------
 * gmc_kway_tabu_f32 and gmc_kway_balance_f32 with `node_cost` ([R][K] fp32 by batch row, as above, or NULL) directly
 * after `terminals`: the chains then search obj(S) = cut(S) - sum_v node_cost[v][S_v] - a QUBO or an Ising model with
 * fields through one-flip tabu search, and with size bounds a cardinality-constrained QUBO.  Each rule is its twin's rule
 * with exactly these changes:
 *
 * Table.  W[v][k] of local node v of the graph on rows r0.. starts from node_cost[r0 + v][k] instead of +0.0f and then
 *   adds the row's weights in CSR order as before (rule 1 above: class_sums_k, the same code); a sum that comes out as
 *   -0.0f is stored as +0.0f (see "Negative zero").  gain = W[v][c] - W[v][k] is then the change of obj for the move
 *   v: c -> k, since the update of step 4 touches the neighbours' rows only and a node's own cost row never changes.
 *   Every other word of the twin's rule stands: the scan, the admissibility test rel + gain > best, h, r, the tenure
 *   draw, the tie order, the +- w update of the neighbours' rows, the deferred snapshot, best_iter and moves; for
 *   gmc_kway_balance_c_f32 also the sizes, the bounds test, the repair (its gains come from this table too), free and
 *   paired moves, the counter-move and repairs / feasible.  No step multiplies, so nothing can be contracted.  A
 *   terminal's cost row starts its W row like any other; it never moves, so only its score counts.
 * Scores.  Every snapshot is scored as rule 2 above states: block_cut(...) - block_cost(...), one fp32 subtraction, the
 *   same code (block_score<K>).  cut_all therefore carries, bit for bit, what gmc_kway_refine_anneal_c_f32 with
 *   anneal_sweeps = 0 and max_descent_sweeps = 0 reports for the same bytes and the same node_cost; a terminal's cost
 *   counts in it.  The pick is unchanged (strictly best score, first on ties).
 * Negative zero.  The twins' order-preserving key relies on gains that are never -0.0f.  With costs a -0.0f could
 *   arise in the table (a cost of -0.0f under a class without neighbours) and from it in a gain ((-0.0f) - (+0.0f)).
 *   The cost variants canonicalise ONCE, where the table is filled: W[v][k] = sum + (+0.0f), which turns -0.0f into
 *   +0.0f and changes no other value.  After that no table entry is -0.0f (x - x and x + (-x) are +0.0f in
 *   round-to-nearest; an update by a weight w leaves +0.0f + (+-0.0f) = +0.0f), so no gain is, and the key's order is the
 *   floats' order as in the twins.  block_cost sums from +0.0f, so the score cannot tell the two zeros apart either: a
 *   node_cost with -0.0f entries gives, on every output, the bytes of the same array with +0.0f entries.
 * By construction.  node_cost == NULL: each entry point IS its twin - the twin's kernels, the same bytes on every
 *   output.  An all-+0.0f node_cost gives the twin's bytes too (the sums start from +0.0f either way; cut - (+0.0f) is
 *   the cut).  With lo[c] = 0 and hi[c] = n gmc_kway_balance_c_f32 is gmc_kway_tabu_c_f32 byte for byte, for the same
 *   cost.  For integer weights and costs every sum is exact below 2^24 and obj(result) = obj(input or repaired state) + best.
 *
 * Argument checks and status codes are the twin's, in its order; node_cost is never tested (NULL selects the twin).
 * Costs must be finite; the C side does not check it.  A cost that is not cannot make a kernel index out of range -
 * the winner of an iteration is decoded from the low half of a key that only a valid (node, class) pair produced - but
 * nothing is claimed about the result.  The launches are the twins': one wave per chain, the same LDS layout
 * (gmc_kway_tabu_shape answers for these calls too), 4 / 2 / 1 chains per workgroup over the staged or the global CSR,
 * two launches on the caller's stream.  With a cost the chain launch is a second kernel compiled from the same body text
 * with the cost switched on (tabu_cost_kernel<K>, balance_cost_kernel<K>), so that the kernels of the twins keep,
 * instruction for instruction, the code they had.  The cost is read from global memory at the
 * table fill and in the scoring tail only and costs no LDS.  No atomics, no spin waits, no scratch, bitwise reproducible. */
int gmc_kway_tabu_c_f32(const gmc_batch *batch, int32_t K, int32_t terminals,
                        const float *node_cost /*[R][K] or NULL*/, int32_t cands, int8_t *assign /*[cands][R], in/out*/,
                        int32_t iterations, int32_t tenure_base, int32_t tenure_span, int32_t tenure_div, uint64_t seed,
                        float *cut_all /*[B][cands]*/, int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/,
                        int32_t *best_idx /*[B]*/, int32_t *best_iter /*[B][cands] or NULL*/,
                        int32_t *moves /*[B][cands] or NULL*/, gmc_stream_t stream);

int gmc_kway_balance_c_f32(const gmc_batch *batch, int32_t K, int32_t terminals,
                           const float *node_cost /*[R][K] or NULL*/, int32_t cands,
                           int8_t *assign /*[cands][R], in/out*/, const int32_t *size_lo /*[B][K]*/,
                           const int32_t *size_hi /*[B][K]*/, int32_t iterations, int32_t tenure_base,
                           int32_t tenure_span, int32_t tenure_div, uint64_t seed, float *cut_all /*[B][cands]*/,
                           int32_t *best_assign /*[R]*/, float *best_cut /*[B]*/, int32_t *best_idx /*[B]*/,
                           int32_t *best_iter /*[B][cands] or NULL*/, int32_t *moves /*[B][cands] or NULL*/,
                           int32_t *repairs /*[B][cands] or NULL*/, int32_t *feasible /*[B] or NULL*/,
                           gmc_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GCNMAXCUT_H */
