// The library's internal cross-file interface: every launcher and host query one translation unit defines and another
// calls.  (The C ABI is include/gcnmaxcut.h.)  All launchers enqueue on `st` and return a GMC_* code or a HIP error.
#pragma once
#include "gmc_common.h"

// ---- LDS-tiled kernels: the batch's geometry (spmm_lds.hip) ---------------------------------------------------------
// Everything the LDS-tiled kernels' template arguments share, worked out once from the gmc_batch fields (host only:
// never the device arrays).  fits == false: the graphs do not fit a CU's LDS and the row kernels serve the batch.
struct GmcLdsGeom {
    bool fits;
    int fs;       // columns per slice (16, 32, 64)
    int W;        // neighbour slots per table row (8, 16)
    int acc;      // rows per thread (4, 8)
    int ns;       // live slots the gathers read (ns_class; every slot with overflow lists)
    bool hv;      // edge weights (gmc_batch.ell_vals)
    bool ovf;     // overflow lists (gmc_has_overflow)
    int slices;   // ceil(F / fs)
};
GmcLdsGeom gmc_lds_geometry(const gmc_batch *b, int F);
bool gmc_lds_fits(const gmc_batch *b);
int gmc_lds_slices_per_group(const gmc_batch *b, int F);   // slices of one workgroup item: 1, 2, 4
int gmc_lds_groups(const gmc_batch *b, int F);             // slice groups per graph (Zpart partials of the W2 epilogue)
int device_cus(bool allow_override = true);                // compute units (gmc_debug_set_device_cus may override)

// ---- flavour words (GMC_FLV_*, gcnmaxcut.h) of the LDS-tiled launches; 0 = the launcher refuses the batch ----------
int gmc_fwd1_flavour(const gmc_batch *b, int F);
int gmc_bwd1_flavour(const gmc_batch *b, int F, bool head);
int gmc_spmm_lds_flavour(const gmc_batch *b, int F, int shared_src, int use_vals, bool epi);
int gmc_dw1_lds_flavour(const gmc_batch *b, int F);
// can the fused backward of this batch compute the one-graph head as well (gmc_bwd1_head)?
bool gmc_bwd1_takes_head(const gmc_batch *b);

// ---- the fused layer-1 kernels -------------------------------------------------------------------------------------
// H (slab layout) = relu(dinv o (A @ (dinv o (A_val @ W1[:n]))) + b1), Zpart[group][r][:] = dinv[r] * (H @ W2) over the
// group's columns.  W1_slab (optional): the [ceil(F/16)][N][16] copy of W1.
int gmc_fwd1_lds_launch(const gmc_batch *b, const float *W1, const float *b1, const float *W2, float *H, float *Zpart,
                        int F, hipStream_t st, const float *W1_slab, int N);
// the head's arguments for a fused backward launch that computes the one-graph head as well
struct gmc_bwd1_head {
    const float *Z0; int zparts; const float *b2; float C; float *P; int *S; float *loss; float *db2part; int *tick;
};
// dW1 partials [chunks][n_max][F] and column partials [chunks][F][4] = (dW2, db1) from the slab-layout H;
// head != nullptr (gmc_bwd1_takes_head only): the launch computes the head too and GY2 is not read
int gmc_bwd1_lds_launch(const gmc_batch *b, const float *H, const float *GY2, const float *W2, float *dw1part,
                        float *colpart, int F, int chunks, int graphs_per_chunk, hipStream_t st,
                        const gmc_bwd1_head *head);
// optional Adam fused into the gradient fold (single GPU); *step_counter (device) already holds this step's number
struct AdamFuse {
    float *param = nullptr, *m = nullptr, *v = nullptr;
    double lr = 0, beta1 = 0, beta2 = 0, eps = 0;
    int *step_counter = nullptr;
    float *w1_slab = nullptr;  // slab copy of W1 to refresh with the update (gmc_model.W1_slab)
};
// folds the fused backward's partials into grad; adam == nullptr: fold only
int gmc_finish_launch(const float *dw1part, const float *colpart, const float *db2part, int chunks, int n_max, int N,
                      int F, int B, float *grad, const AdamFuse *adam, const float *loss_for_tail, hipStream_t st);
int gmc_loss_tail_launch(const float *loss, int B, float *slot, hipStream_t st);

// ---- SpMM (spmm.hip: row kernels, spmm_lds.hip: LDS-tiled) ---------------------------------------------------------
// internal form of gmc_spmm_f32 with a probe tag
int gmc_spmm_launch(const int32_t *rowptr, const int32_t *col, const float *vals, const float *scale, const float *X,
                    int64_t ldx, const float *bias, int relu, float *Y, int64_t ldy, int32_t n_rows, int32_t F,
                    int32_t group_rows, const float *W2, float *Z0, int tag, hipStream_t st);
// Y = act(scale * A_g @ X + bias) per graph, LDS-staged; optional fused Zpart (W2 epilogue).  x_slab / y_slab: the
// operand uses the slab layout [slice][R][FS] instead of row-major with leading dimension ldx / ldy
int gmc_spmm_lds_launch(const gmc_batch *b, const float *X, long ldx, int x_slab, int shared_src, int use_vals,
                        const float *scale, const float *bias, int relu, float *Y, long ldy, int y_slab, int F,
                        const float *W2, float *Zpart, int tag, hipStream_t st);

// ---- dW1 (dw1.hip, spmm_lds.hip) ------------------------------------------------------------------------------------
int gmc_dw1_chunks(int B, bool lds, int slices);
size_t gmc_dw1_scratch_floats(const gmc_batch *b, int N, int F, bool lds);
int gmc_dw1_launch(const gmc_batch *b, const float *U, long ldu, float *dW1, float *scratch, int N, int F, bool lds,
                   hipStream_t st);
int gmc_dw1_lds_launch(const gmc_batch *b, const float *U, long ldu, int u_slab, float *out, int F, int chunks,
                       int graphs_per_chunk, hipStream_t st);

// ---- head (head.hip), hidden backward (hidden_bwd.hip), dropout (dropout.hip) --------------------------------------
// tick != nullptr: the launch also advances the device-side Adam step counter; loss_kind: GMC_LOSS_*
inline bool gmc_loss_kind_ok(int kind) { return kind == GMC_LOSS_CUT || kind == GMC_LOSS_EXPECTED_CUT; }
int gmc_head_launch(const gmc_batch *batch, const float *Z0, int32_t z_parts, const float *b2, float C, float *P,
                    int32_t *S, float *loss, float *GY2, float *db2part, int *tick, hipStream_t st, int loss_kind);
int gmc_head_bwd_launch(const gmc_batch *batch, const float *P, const float *GP, float *GY2, float *db2part,
                        hipStream_t st);
int gmc_hidden_tiles(int R);
int gmc_hidden_slab_tiles(int R);
int gmc_hidden_bwd_launch(const float *H, long ldh, const float *GY2, const float *W2, const float *dinv, float *Gs,
                          long ldg, float *part, int R, int F, hipStream_t st);
int gmc_hidden_bwd_slab_launch(const float *H, const float *GY2, const float *W2, const float *dinv, float *Gs,
                               float *part, int R, int F, int fs, hipStream_t st);
int gmc_colsum_reduce_launch(const float *part, int tiles, int F, float *dW2, float *db1, const float *db2part, int B,
                             float *db2, hipStream_t st);
int gmc_dropout_launch(float *H, long R, int F, int fs, long ld, float p, unsigned long long seed, hipStream_t st);
int gmc_hw2_rows_launch(const float *H, const float *dinv, const float *W2, float *Z0, long R, int F, int fs, long ld,
                        hipStream_t st);
int gmc_scale_copy_launch(const float *src, float *dst, int n, float s, hipStream_t st);

// ---- dense fp32 GEMM on the matrix cores (gemm_mfma.hip) ------------------------------------------------------------
// C[M,Nc] = scale o (op(A) @ op(B)), ta / tb: the operand is stored transposed; internal form of gmc_gemm_f32
int gmc_gemm_launch(int ta, int tb, int M, int Nc, int K, const float *A, long lda, const float *B, long ldb,
                    const float *scale, float *C, long ldc, hipStream_t st);

// ---- the K-class step (kway.hip): the K-wide forms of hw2_rows, the head, the hidden backward and the partials' fold ----
// K: 2..GMC_KWAY_MAX_CLASSES, else GMC_ERR_CLASSES.  Row-major operands: Z0, P, GY2 [R,K], W2 [F,K] (W2 and P 16-byte
// aligned), part [gmc_hidden_tiles(R)][F][K+1], db2part [B,K].
constexpr size_t GMC_KWAY_LDS_BYTES = 160 * 1024;   // a CU's LDS: what one graph's [n,K] tiles of the head may take
size_t gmc_kway_head_lds_bytes(int n_max, int K, int loss_kind);
int gmc_kway_hw2_launch(const float *H, long ld, const float *dinv, const float *W2, float *Z0, long R, int F, int K,
                        hipStream_t st);
// GY2 == nullptr: forward only (P, S, loss); GMC_ERR_GRAPH_SIZE when gmc_kway_head_lds_bytes exceeds GMC_KWAY_LDS_BYTES.
// b2_stride: floats from one graph's conv2.bias to the next - 0 = the one shared bias, K = b2 [B,K] (the per-graph
// models of instance.hip); the bias is read at b2 + g * b2_stride, so 0 is the launch it was before the argument.
// node_cost: [R,K] per-node class costs of the loss (gmc_inst_*_c) or NULL
int gmc_kway_head_launch(const gmc_batch *b, const float *Z0, const float *b2, float C, int K, int loss_kind, float *P,
                         int32_t *S, float *loss, float *GY2, float *db2part, hipStream_t st, long b2_stride = 0,
                         int terminals = 1, const float *node_cost = nullptr);
int gmc_kway_hidden_bwd_launch(const float *H, long ldh, const float *GY2, const float *W2, const float *dinv, float *Gs,
                               long ldg, float *part, int R, int F, int K, hipStream_t st);
int gmc_kway_reduce_launch(const float *part, int tiles, int F, int K, float *dW2, float *db1, const float *db2part,
                           int B, float *db2, hipStream_t st);

// ---- one model per graph (instance.hip): the kernels of the K-class sequence that select a graph's own b1 [B,F],
// W2 [B,F,K] by the row's graph.  Grids are (graph, tile of the graph's rows); part: gmc_inst_part_floats floats.
size_t gmc_inst_part_floats(const gmc_batch *b, int F, int K);
// H [R,ld] in place: relu(H + b1_g); Z0[r,:] = dinv[r] * (H[r,:] @ W2_g)
int gmc_inst_hw2_launch(const gmc_batch *b, float *H, long ld, const float *b1, const float *W2, float *Z0, int F, int K,
                        hipStream_t st);
int gmc_inst_hidden_bwd_launch(const gmc_batch *b, const float *H, long ldh, const float *GY2, const float *W2, float *Gs,
                               long ldg, float *part, int F, int K, hipStream_t st);
int gmc_inst_fold_launch(const gmc_batch *b, const float *part, int F, int K, float *dW2, float *db1, hipStream_t st);

// ---- one model per graph beyond a CU's LDS (instance_large.hip: gmc_inst_large_*), n_max up to GMC_LARGE_MAX_GRAPH_NODES.
// gmc_inst_hw2_launch with a grid that stays within 65,535 in y (a workgroup walks the graph's 4-row tiles): the same bytes
int gmc_inst_large_hw2_launch(const gmc_batch *b, float *H, long ld, const float *b1, const float *W2, float *Z0, int F,
                              int K, hipStream_t st);
// gmc_large_head_launch (same scratch: Sw [R], GZd [R,K], headpart [gmc_large_headpart_floats]) with b2 [B,K] read at
// b2 + g * K, terminals (0 / 1) a run-time value and the per-graph sums of the softmax backward written to db2 [B,K]
int gmc_inst_large_head_launch(const gmc_batch *b, const float *Z0, const float *b2, float C, int K, int loss_kind,
                               int terminals, float *P, int32_t *S, float *loss, int32_t *Sw, float *GZd, float *headpart,
                               float *GY2, float *db2, hipStream_t st);

// ---- the head for graphs beyond a CU's LDS (large.hip): head_k_kernel as row-parallel launches, several workgroups per
// graph (tiles of 256 rows).  Sw [R] ints, GZd [R,K] (dinv o GZ) and headpart [gmc_large_headpart_floats] are scratch.
size_t gmc_large_headpart_floats(const gmc_batch *b, int K);
// GZd == nullptr: forward only (P, S, loss); else GY2 [R,K] and db2part [B,K] are written too
int gmc_large_head_launch(const gmc_batch *b, const float *Z0, const float *b2, float C, int K, int loss_kind, float *P,
                          int32_t *S, float *loss, int32_t *Sw, float *GZd, float *headpart, float *GY2, float *db2part,
                          hipStream_t st);
// Rows of more than 64 entries of Y = act(scale * A @ X + bias), written again after gmc_spmm_launch (same operands; F and
// the leading dimensions multiples of 4, 16-byte aligned): the row kernels of spmm.hip add a row's entries one after the
// other in CSR order, whose float32 error grows with the degree (5.6e-5 of the sum for 4200 equal addends); here the
// row's sum is that of its first 64 entries plus, one after the other, the sum of each further 64 (each in CSR order), so
// the error grows with 64 + deg / 64.  Rows of up to 64 entries are left as spmm.hip wrote them.
int gmc_large_hub_rows_launch(const int32_t *rowptr, const int32_t *col, const float *vals, const float *scale,
                              const float *X, long ldx, const float *bias, int relu, float *Y, long ldy, int32_t n_rows,
                              int32_t F, int tag, hipStream_t st);

// ---- the functional form of the model (functional.hip: gmc_fn_*): row-parallel launches on large.hip's grid (graph, tile
// of 256 rows), K in 2..GMC_KWAY_MAX_CLASSES, P / GP / GZd / GY2 [R,K] 16-byte aligned.  part: gmc_fn_part_floats(b, V) floats
// of tile partials, V sums per tile (R / 256 + B + 1 slots, large.hip's).
size_t gmc_fn_part_floats(const gmc_batch *b, int V);
// P = softmax(dinv o (A @ Z0) + b2): gmc_large_head_launch's probabilities without decode and loss
int gmc_fn_prob_launch(const gmc_batch *b, const float *Z0, const float *b2, int K, float *P, hipStream_t st);
// the softmax backward of a caller's GP = dLoss/dP: GZd = dinv o GZ, db2part [B,K] (part: V = K), GY2 = A @ GZd
int gmc_fn_softmax_bwd_launch(const gmc_batch *b, const float *P, const float *GP, int K, float *GZd, float *part,
                              float *db2part, float *GY2, hipStream_t st);
// loss [B] (and GP [R,K] when given) of the probabilities P; part: V = 1
int gmc_fn_loss_launch(const gmc_batch *b, const float *P, int K, int terminals, float C, int loss_kind, float *part,
                       float *loss, float *GP, hipStream_t st);

// ---- the graph-attention first layer (attention.hip): the row kernels of the gmc_att_* entry points -----------------
// Row-major [R, ld] operands T (= X @ W1), H, G (gradient at layer 1's pre-activation), dT; per-row scalars s_src, s_dst,
// alpha_s, dz_s, ds_src, ds_dst [R]; per-CSR-entry scalars alpha_e, dz_e [nnz].  a_src / a_dst [F] need no alignment.
size_t gmc_att_avec_part_floats(int R, int F);
int gmc_att_scores_launch(const float *T, long ld, const float *a_src, const float *a_dst, float *s_src, float *s_dst,
                          int R, int F, hipStream_t st);
int gmc_att_fwd_launch(const gmc_batch *b, const float *T, long ld, const float *s_src, const float *s_dst, float slope,
                       const float *bias, float *alpha_e, float *alpha_s, float *H, int F, hipStream_t st);
// GY2 [R,4] rows scaled by dinv in place, ones[r] = 1
int gmc_att_gy2_scale_launch(float *GY2, const float *dinv, float *ones, int R, hipStream_t st);
int gmc_att_edge_bwd_launch(const gmc_batch *b, const float *T, const float *G, long ld, const float *s_src,
                            const float *s_dst, float slope, const float *alpha_e, const float *alpha_s, float *dz_e,
                            float *dz_s, float *ds_dst, int F, hipStream_t st);
int gmc_att_bwd_t_launch(const gmc_batch *b, const float *G, long ld, const float *alpha_e, const float *alpha_s,
                         const float *dz_e, const float *dz_s, const float *ds_dst, float *ds_src, const float *a_src,
                         const float *a_dst, float *dT, int F, hipStream_t st);
// da_src = sum_r ds_src[r] * T[r,:], da_dst = sum_r ds_dst[r] * T[r,:]; part: gmc_att_avec_part_floats(R, F) floats
int gmc_att_avec_launch(const float *T, long ld, const float *ds_src, const float *ds_dst, float *part, float *da_src,
                        float *da_dst, int R, int F, hipStream_t st);
