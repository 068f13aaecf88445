// C-ABI orchestration: the fused forward / training entry points of gcnmaxcut.h.
// Everything is enqueued on the caller's stream; nothing allocates or synchronises.
#include "launchers.h"
#include <stdlib.h>

namespace {

// Fused layer kernels (default) vs the one-kernel-per-op sequence: gmc_set_fuse(0) selects the latter
// (bench.py times the stand-alone SpMM kernel that way).  The shipped library reads no environment variables;
// tuning builds (`make variant DEFS=-DGMC_TUNING`) also honour GMC_FUSE=0 and GMC_SPMM_ALGO=rows.
int g_fuse = -1;
bool fuse_enabled() {
    if (g_fuse < 0) {
        g_fuse = 1;
#ifdef GMC_TUNING
        const char *e = getenv("GMC_FUSE");
        if (e && e[0] == '0') g_fuse = 0;
#endif
    }
    return g_fuse != 0;
}

// What a call asks of plan and carve.
struct Ask {
    bool training;     // the backward follows: its buffers are carved too
    bool train_step;   // gmc_train_step_loss_f32 (fused Adam; a one-graph batch may take the head into the backward)
    bool dense;        // a *_features entry point: X is not the padded adjacency (dW1 comes from a GEMM: no dW1 scratch)
    int loss;          // GMC_LOSS_*: the one internal form of the loss kind, converted once at the ABI boundary
};
// ... of the entry points whose loss kind is a bit of gmc_model.flags (read only from a struct of this header's layout)
int loss_of(const gmc_model *m) {
    return m && m->abi == GMC_VERSION && (m->flags & GMC_MODEL_LOSS_EXPECTED) ? GMC_LOSS_EXPECTED_CUT : GMC_LOSS_CUT;
}

// The kernel sequence of a call, decided once.  Three sequences:
//   row kernels (fs == 0) - the largest graph does not fit a CU's LDS;
//   fused LDS kernels (fused) - fused forward, head, fused backward + finish (train_step: + Adam);
//   one-kernel-per-operation LDS sequence - gmc_set_fuse(0), or dropout (which needs H before the W2 product).
// A batch with overflow lists (rows of more than ell_width neighbours) is served by the fused LDS kernels only: in the
// one-kernel-per-operation sequence it takes the row kernels.
// Dense features (gmc_forward_features: X is not the padded adjacency) always take the row kernels: the layer-1 GEMMs
// then address plain row-major [R, ld] buffers.
struct Plan {
    int fs;             // slice width of the LDS kernels and the slab layout [slice][R][fs]; 0 = row kernels
    bool fused;         // fused forward and fused backward
    bool head_in_bwd;   // train_step: the one-graph head runs inside the fused backward
    int zparts;         // partials in Z0 (fused W2 epilogue: one per slice group)
    int slices;         // column slices (LDS sequences)
    int chunks;         // dW1 chunks of the LDS sequences
};

Plan plan(const gmc_batch *b, int F, float dropout_p, bool fuse, const Ask &ask) {
    Plan p{};
    p.zparts = 1;
    if (ask.dense) return p;
    const bool dropout = dropout_p > 0.f;
    const GmcLdsGeom g = gmc_lds_geometry(b, F);
    bool lds = g.fits && !(g.ovf && (!fuse || dropout));
#ifdef GMC_TUNING
    static const bool forced_rows = [] {
        const char *e = getenv("GMC_SPMM_ALGO");
        return e && e[0] == 'r';
    }();
    if (forced_rows) lds = false;
#endif
    if (!lds) return p;
    p.fs = g.fs;
    p.slices = g.slices;
    p.chunks = gmc_dw1_chunks(b->B, true, g.slices);
    p.fused = fuse && !dropout;
    if (!dropout) p.zparts = gmc_lds_groups(b, F);   // (dropout: Z0 comes from its own kernel)
    // (the head inside the backward launch computes GMC_LOSS_CUT only)
    p.head_in_bwd = ask.train_step && ask.loss == GMC_LOSS_CUT && p.fused && p.chunks == 1 && gmc_bwd1_takes_head(b);
    return p;
}

struct Workspace {
    Plan plan;
    long ld;         // row kernels: leading dimension of the [R,F] buffers (F rounded up to 32 floats)
    float *T0;       // [R,ld]  (X o dinv)@W1, later Gs = dinv o Gpre
    float *H;        // [R,ld]  relu(conv1), later U = dinv o (A @ Gs)
    float *Z0;       // [plan.zparts,R,3]
    float *GY2;      // [R,4] = (GY2[r,0..2], dinv[r])
    float *part;     // [tiles,F,4]
    float *db2part;  // [B,3]
    float *dw1part;  // [chunks,N,F]
    float *W2s;      // [F,3] = W2 / (1-p), dropout only (last, so that forward-only carving shares the prefix)
    size_t bytes;
};

bool dropout_on(const gmc_model *m) { return m->dropout_p > 0.f; }
unsigned long long dropout_seed(const gmc_model *m) { return ((unsigned long long)m->dropout_seed_hi << 32) | m->dropout_seed_lo; }

size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }

// base == nullptr: sizes only (gmc_workspace_bytes)
Workspace carve(const gmc_batch *b, const gmc_model *m, const Ask &ask, void *base) {
    Workspace w{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(static_cast<char *>(base) + off) : nullptr;
        off += align_up(floats * sizeof(float));
        return p;
    };
    const size_t R = (size_t)b->R, F = (size_t)m->F;
    w.plan = plan(b, m->F, m->dropout_p, fuse_enabled(), ask);
    const int fs = w.plan.fs;
    w.ld = (long)((F + 31) / 32 * 32);
    const size_t cols = fs ? (F + fs - 1) / fs * fs : (size_t)w.ld;
    w.T0 = take(R * cols);
    w.H = take(R * cols);
    w.Z0 = take((size_t)w.plan.zparts * R * 3);
    if (ask.training) {
        w.GY2 = take(R * 4);  // (GY2[r,0..2], dinv[r]) per row: one aligned 16 B load downstream
        size_t tiles = (size_t)(fs ? gmc_hidden_slab_tiles(b->R) : gmc_hidden_tiles(b->R));
        if (fs && (size_t)w.plan.chunks > tiles) tiles = (size_t)w.plan.chunks;
        w.part = take(tiles * F * 4);
        w.db2part = take((size_t)b->B * 3);
        w.dw1part = take(ask.dense ? 0 : gmc_dw1_scratch_floats(b, m->N, m->F, fs != 0));
        if (dropout_on(m)) w.W2s = take(F * 3);
    }
    w.bytes = off;
    return w;
}

// the structs are there and were built against this header: nothing else of them is read before this passes
int check_abi(const gmc_batch *b, const gmc_model *m) {
    if (!b || !m) return GMC_ERR_NULL;
    if (b->abi != GMC_VERSION || m->abi != GMC_VERSION) return GMC_ERR_ABI;   // built against another header
    return GMC_OK;
}

// dense: features with their own N columns - a graph may then have more nodes than conv1.weight has rows
int check(const gmc_batch *b, const gmc_model *m, bool dense) {
    if (int rc = check_abi(b, m)) return rc;
    if (!b->goff || !b->rowptr || !b->gcol || !b->lcol || !b->dinv) return GMC_ERR_NULL;
    if (!m->W1 || !m->b1 || !m->W2 || !m->b2) return GMC_ERR_NULL;
    if (m->K != 3) return GMC_ERR_CLASSES;
    if (b->B < 0 || b->R < 0 || b->nnz < 0 || m->N <= 0 || m->F <= 0) return GMC_ERR_SHAPE;
    if (m->F % 4 || m->F > GMC_MAX_HIDDEN) return GMC_ERR_UNSUPPORTED;  // float4 rows
    if (!(m->dropout_p >= 0.f && m->dropout_p < 1.f)) return GMC_ERR_SHAPE;
    if (m->W1_slab && !gmc_aligned16(m->W1_slab)) return GMC_ERR_ALIGN;
    if (b->B > 0 && (b->n_max < 3 || b->n_max > GMC_MAX_GRAPH_NODES)) return GMC_ERR_GRAPH_SIZE;
    if (!dense && b->n_max > m->N) return GMC_ERR_SHAPE;  // more nodes than rows of conv1.weight
    return GMC_OK;
}

// One call of a fused entry point: what open() validated and carved, plus the optional parts its bodies look at.
struct Call {
    const gmc_batch *b; const gmc_model *m;
    const float *X = nullptr; long ldx = 0;   // dense features [R, N] (the *_features entry points: row kernel plan)
    float *dX = nullptr; long lddx = 0;       // backward with X: dX = U @ W1^T when asked for
    Ask ask{}; Workspace w{}; hipStream_t st = nullptr;   // (filled in by open)
    const AdamFuse *adam = nullptr;         // Adam fused into the gradient fold (gmc_train_step_loss_f32)
    const float *loss_tail = nullptr;       // per-graph losses whose sum goes to the slot after the gradient
    const gmc_bwd1_head *head = nullptr;    // the fused backward computes the one-graph head as well
};

// Opens a call: every argument check of the fused entry points, in the one order gcnmaxcut.h documents ("Argument
// checks"), then the carving of the workspace.  c carries b, m and X / ldx / dX / lddx as the caller handed them over;
// grad: required (and 16-byte aligned) by a training call; outputs: the call's other required pointers are all there.
int open(Call &c, Ask ask, void *workspace, size_t workspace_bytes, gmc_stream_t stream, const float *grad, bool outputs) {
    if (int rc = check(c.b, c.m, ask.dense)) return rc;               // 1. 2. (X: the *_features entry points)
    if (ask.dense) {                                                  // 3. the features (the GEMMs' operands)
        if (c.ldx < c.m->N) return GMC_ERR_SHAPE;
        if (!gmc_aligned16(c.X) || c.ldx % 4 || !gmc_aligned16(c.m->W1)) return GMC_ERR_ALIGN;
    }
    if (!workspace || !outputs || (ask.training && !grad)) return GMC_ERR_NULL;   // 4. workspace and outputs
    if (c.dX && c.lddx < c.m->N) return GMC_ERR_SHAPE;                // 5. grad and dX
    if (!gmc_aligned16(grad) || (c.dX && (!gmc_aligned16(c.dX) || c.lddx % 4))) return GMC_ERR_ALIGN;
    c.ask = ask;
    c.w = carve(c.b, c.m, ask, workspace);                            // 6. workspace size
    if (c.w.bytes > workspace_bytes) return GMC_ERR_WORKSPACE;
    c.st = static_cast<hipStream_t>(stream);
    return GMC_OK;
}

// floats of the flat gradient [dW1 | db1 | dW2 | db2]; with_tail: and the slot behind it (GMC_MODEL_GRAD_TAIL);
// zero_grad: the gradient of an empty batch
size_t grad_floats(const gmc_model *m, bool with_tail) {
    return (size_t)m->N * m->F + m->F + (size_t)m->F * 3 + 3 + (with_tail ? 1 : 0);
}
int zero_grad(const Call &c, float *grad, bool with_tail) {
    return (int)hipMemsetAsync(grad, 0, grad_floats(c.m, with_tail) * sizeof(float), c.st);
}

int group_rows(const gmc_batch *b) { return b->uniform_n > 0 ? b->uniform_n : b->n_max; }

// Y = act(dinv o (A @ X) + bias) over the batch with either implementation; Z0 (optional) gets
// the fused layer-2 feature transform (zparts partials on the LDS path).
int aggregate(const Call &c, const float *X, float *Y, const float *bias, int relu, const float *W2, float *Z0, int tag) {
    const gmc_batch *b = c.b;
    const long ld = c.w.ld;
    if (c.w.plan.fs) return gmc_spmm_lds_launch(b, X, ld, 1, 0, 0, b->dinv, bias, relu, Y, ld, 1, c.m->F, W2, Z0, tag, c.st);
    return gmc_spmm_launch(b->rowptr, b->gcol, nullptr, b->dinv, X, ld, bias, relu, Y, ld, b->R, c.m->F, group_rows(b),
                           W2, Z0, tag, c.st);
}

// c.X: layer 1's feature transform is a GEMM
int forward_body(const Call &c) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m;
    const Workspace &w = c.w; hipStream_t st = c.st;
    const int F = m->F;
    if (w.plan.fused)  // T0 lives only in LDS
        return gmc_fwd1_lds_launch(b, m->W1, m->b1, m->W2, w.H, w.Z0, F, st, m->W1_slab, m->N);
    // layer 1 feature transform:  T0 = dinv o (X @ W1), for X = the padded adjacency a row gather of W1:
    // T0 = dinv o (A_val @ W1[:n])
    const int fs = w.plan.fs;
    int rc = c.X ? gmc_gemm_launch(0, 0, b->R, F, m->N, c.X, c.ldx, m->W1, F, b->dinv, w.T0, w.ld, st)
             : fs ? gmc_spmm_lds_launch(b, m->W1, F, 0, 1, 1, b->dinv, nullptr, 0, w.T0, w.ld, 1, F, nullptr,
                                        nullptr, GMC_K_GATHER_W1, st)
                  : gmc_spmm_launch(b->rowptr, b->lcol, b->vals, b->dinv, m->W1, F, nullptr, 0, w.T0, w.ld,
                                    b->R, F, group_rows(b), nullptr, nullptr, GMC_K_GATHER_W1, st);
    if (rc) return rc;
    if (dropout_on(m)) {  // relu -> dropout -> layer-2 feature transform of the DROPPED activations (:81-83)
        rc = aggregate(c, w.T0, w.H, m->b1, 1, nullptr, nullptr, GMC_K_AGG_FWD);
        if (rc) return rc;
        rc = gmc_dropout_launch(w.H, b->R, F, fs, w.ld, m->dropout_p, dropout_seed(m), st);
        if (rc) return rc;
        return gmc_hw2_rows_launch(w.H, b->dinv, m->W2, w.Z0, b->R, F, fs, w.ld, st);
    }
    // layer 1 aggregation + bias + relu with the layer 2 feature transform fused in
    return aggregate(c, w.T0, w.H, m->b1, 1, m->W2, w.Z0, GMC_K_AGG_FWD);
}

// the stand-alone head launch; backward: it also leaves GY2 and the db2 partials for the backward
int head(const Call &c, float C, float *P, int32_t *S, float *loss, bool backward, int32_t *tick) {
    return gmc_head_launch(c.b, c.w.Z0, c.w.plan.zparts, c.m->b2, C, P, S, loss, backward ? c.w.GY2 : nullptr,
                           backward ? c.w.db2part : nullptr, tick, c.st, c.ask.loss);
}

// c.X: the dense features of the forward - dW1 = X^T @ U, and dX = U @ W1^T when asked for
int backward_body(const Call &c, float *grad) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m;
    const Workspace &w = c.w; hipStream_t st = c.st;
    const long F = m->F;
    float *dW1 = grad, *db1 = grad + (long)m->N * F, *dW2 = db1 + F, *db2 = dW2 + F * 3;
    float *Gs = w.T0, *U = w.H;
    const float *W2b = m->W2;
    if (dropout_on(m)) {  // relu'(H) o mask / (1-p): the mask is the zeros of the stored H, the factor rides on W2
        if (c.adam || !w.W2s) return GMC_ERR_UNSUPPORTED;
        int rc = gmc_scale_copy_launch(m->W2, w.W2s, (int)F * 3, 1.0f / (1.0f - m->dropout_p), st);
        if (rc) return rc;
        W2b = w.W2s;
    }
    if (w.plan.fused) {  // one pass over H: Gs and U live only in LDS
        const int chunks = w.plan.chunks, per = (b->B + chunks - 1) / chunks;
        int rc = gmc_bwd1_lds_launch(b, w.H, w.GY2, m->W2, w.dw1part, w.part, m->F, chunks, per, st, c.head);
        if (rc) return rc;
        return gmc_finish_launch(w.dw1part, w.part, w.db2part, chunks, b->n_max, m->N, m->F, b->B, grad, c.adam,
                                 c.loss_tail, st);
    }
    if (c.adam) return GMC_ERR_UNSUPPORTED;  // the fused Adam rides on the fused backward
    const int fs = w.plan.fs;
    int rc = fs ? gmc_hidden_bwd_slab_launch(w.H, w.GY2, W2b, b->dinv, Gs, w.part, b->R, m->F, fs, st)
                  : gmc_hidden_bwd_launch(w.H, w.ld, w.GY2, W2b, b->dinv, Gs, w.ld, w.part, b->R, m->F, st);
    if (rc) return rc;
    rc = gmc_colsum_reduce_launch(w.part, fs ? gmc_hidden_slab_tiles(b->R) : gmc_hidden_tiles(b->R), m->F,
                                  dW2, db1, w.db2part, b->B, db2, st);
    if (rc) return rc;
    // conv1 backward aggregation:  U = dinv o (A @ Gs)
    rc = aggregate(c, Gs, U, nullptr, 0, nullptr, nullptr, GMC_K_AGG_BWD);
    if (rc) return rc;
    if (c.X) {
        rc = gmc_gemm_launch(1, 0, m->N, m->F, b->R, c.X, c.ldx, U, w.ld, nullptr, dW1, F, st);
        if (!rc && c.dX) rc = gmc_gemm_launch(0, 1, b->R, m->N, m->F, U, w.ld, m->W1, F, nullptr, c.dX, c.lddx, st);
    } else {
        rc = gmc_dw1_launch(b, U, w.ld, dW1, w.dw1part, m->N, m->F, fs != 0, st);
    }
    if (rc || !c.loss_tail) return rc;
    return gmc_loss_tail_launch(c.loss_tail, b->B, db2 + 3, st);
}

size_t workspace_bytes(const gmc_batch *b, const gmc_model *m, int training, bool dense) {
    return check_abi(b, m) ? 0 : carve(b, m, Ask{training != 0, false, dense, loss_of(m)}, nullptr).bytes;
}

// gmc_forward (X == nullptr) and gmc_forward_features
int forward_call(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx, float C, void *workspace,
                 size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream) {
    Call c{batch, model, X, (long)ldx};
    int rc = open(c, Ask{false, false, X != nullptr, loss_of(model)}, workspace, workspace_bytes, stream, nullptr, P != nullptr);
    if (rc || batch->R == 0) return rc;
    rc = forward_body(c);
    return rc ? rc : head(c, C, P, S, loss, false, nullptr);
}

// forward, head and backward of an opened training call; tail: the loss sum goes to the slot after the gradient
int fwd_bwd(Call &c, float C, float *P, int32_t *S, float *loss, float *grad, bool tail) {
    if (c.b->R == 0) return zero_grad(c, grad, tail);
    int rc = forward_body(c);
    if (!rc) rc = head(c, C, P, S, loss, true, nullptr);
    if (rc) return rc;
    c.loss_tail = tail ? loss : nullptr;
    return backward_body(c, grad);
}

// gmc_backward_from_gp (X == nullptr) and gmc_backward_features_from_gp; neither knows of a tail slot
int backward_call(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx, void *workspace,
                  size_t workspace_bytes, const float *P, const float *GP, float *grad, float *dX, int64_t lddx, gmc_stream_t stream) {
    Call c{batch, model, X, (long)ldx, dX, (long)lddx};
    int rc = open(c, Ask{true, false, X != nullptr, loss_of(model)}, workspace, workspace_bytes, stream, grad, P && GP);
    if (rc) return rc;
    if (batch->R == 0) return zero_grad(c, grad, false);
    rc = gmc_head_bwd_launch(batch, P, GP, c.w.GY2, c.w.db2part, c.st);
    return rc ? rc : backward_body(c, grad);
}

}  // namespace

// the flavour words of a training step's LDS-tiled launches: the fused sequence's, then those of the
// one-kernel-per-operation sequence (gmc_set_fuse(0)) without dropout - with it the aggregation of the forward drops its
// W2 epilogue, i.e. takes the backward aggregation's word
extern "C" int gmc_lds_flavours(const gmc_batch *batch, int32_t F, int32_t one_graph_step, int32_t *words, int32_t max) {
    if (!batch) return GMC_ERR_NULL;
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;
    if (F <= 0 || F % 4 || F > GMC_MAX_HIDDEN || max < 0 || batch->B < 0) return GMC_ERR_SHAPE;
    int out[6], n = 0;
    const Plan fused = plan(batch, F, 0.f, true, Ask{true, one_graph_step != 0, false, GMC_LOSS_CUT});
    const Plan unfused = plan(batch, F, 0.f, false, Ask{true, false, false, GMC_LOSS_CUT});
    if (fused.fused) {
        out[n++] = gmc_fwd1_flavour(batch, F);
        out[n++] = gmc_bwd1_flavour(batch, F, fused.head_in_bwd);
    }
    if (unfused.fs) {
        out[n++] = gmc_spmm_lds_flavour(batch, F, 1, 1, false);   // W1 gather
        out[n++] = gmc_spmm_lds_flavour(batch, F, 0, 0, true);    // aggregation + relu + W2 epilogue
        out[n++] = gmc_spmm_lds_flavour(batch, F, 0, 0, false);   // backward aggregation
        out[n++] = gmc_dw1_lds_flavour(batch, F);
    }
    for (int i = 0; i < n && i < max; ++i)
        if (words) words[i] = out[i];
    return n;
}

extern "C" int gmc_set_fuse(int on) {
    const int prev = fuse_enabled() ? 1 : 0;
    g_fuse = on ? 1 : 0;
    return prev;
}

extern "C" int gmc_version(void) { return GMC_VERSION; }

extern "C" const char *gmc_error_string(int code) {
    switch (code) {
        case GMC_OK: return "ok";
        case GMC_ERR_NULL: return "required pointer is NULL";
        case GMC_ERR_SHAPE: return "negative or inconsistent sizes";
        case GMC_ERR_CLASSES: return "number_classes must be 3 (override_fixed_nodes is 3-wide)";
        case GMC_ERR_ALIGN: return "pointer or leading dimension not 16-byte aligned";
        case GMC_ERR_WORKSPACE: return "workspace too small";
        case GMC_ERR_GRAPH_SIZE: return "graph has fewer than 3 or more than GMC_MAX_GRAPH_NODES nodes";
        case GMC_ERR_UNSUPPORTED: return "unsupported shape (the hidden width F must be a multiple of 4 and <= 4096 = GMC_MAX_HIDDEN)";
        case GMC_ERR_LOSS: return "unknown loss kind (GMC_LOSS_CUT = 0, GMC_LOSS_EXPECTED_CUT = 1)";
        case GMC_ERR_ABI: return "gmc_batch.abi / gmc_model.abi differs from the library's GMC_VERSION: rebuild the caller against this include/gcnmaxcut.h";
        default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown gmc error";
    }
}

// device-side address of pinned (hipHostMalloc / hipHostRegister) host memory, for callers that let the kernels
// write a result - the per-graph losses - straight into host memory they poll
extern "C" int gmc_host_device_pointer(void *pinned_host, void **device_ptr) {
    if (!pinned_host || !device_ptr) return GMC_ERR_NULL;
    return (int)hipHostGetDevicePointer(device_ptr, pinned_host, 0);
}

extern "C" size_t gmc_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training) {
    return workspace_bytes(batch, model, training, false);
}

extern "C" size_t gmc_workspace_bytes_features(const gmc_batch *batch, const gmc_model *model, int training) {
    return workspace_bytes(batch, model, training, true);
}

extern "C" int gmc_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                           size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream) {
    return forward_call(batch, model, nullptr, 0, C, workspace, workspace_bytes, P, S, loss, stream);
}

extern "C" int gmc_forward_features(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx, float C,
                                    void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream) {
    if (!X) return GMC_ERR_NULL;   // (what tells the plain call from this one)
    return forward_call(batch, model, X, ldx, C, workspace, workspace_bytes, P, S, loss, stream);
}

extern "C" int gmc_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                                 size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad, gmc_stream_t stream) {
    Call c{batch, model};
    int rc = open(c, Ask{true, false, false, loss_of(model)}, workspace, workspace_bytes, stream, grad, P != nullptr);
    if (rc) return rc;
    const bool tail = (model->flags & GMC_MODEL_GRAD_TAIL) != 0;
    if (tail && !loss) return GMC_ERR_NULL;
    return fwd_bwd(c, C, P, S, loss, grad, tail);
}

extern "C" int gmc_train_step_f32(const gmc_batch *batch, int32_t N, int32_t F, float *param, float C,
                                  void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                                  float *grad, float *mom, float *var, double lr, double beta1, double beta2,
                                  double eps, int32_t *step_counter, float *w1_slab, gmc_stream_t stream) {
    return gmc_train_step_loss_f32(batch, N, F, param, C, GMC_LOSS_CUT, workspace, workspace_bytes, P, S, loss, grad,
                                   mom, var, lr, beta1, beta2, eps, step_counter, w1_slab, stream);
}

extern "C" int gmc_train_step_loss_f32(const gmc_batch *batch, int32_t N, int32_t F, float *param, float C, int32_t loss_kind,
                                       void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                                       float *grad, float *mom, float *var, double lr, double beta1, double beta2,
                                       double eps, int32_t *step_counter, float *w1_slab, gmc_stream_t stream) {
    if (!gmc_loss_kind_ok(loss_kind)) return GMC_ERR_LOSS;
    if (!param || !grad || !mom || !var || !step_counter) return GMC_ERR_NULL;
    if (!gmc_aligned16(param) || !gmc_aligned16(mom) || !gmc_aligned16(var)) return GMC_ERR_ALIGN;
    const long nW1 = (long)N * F;
    // (no GMC_MODEL_GRAD_TAIL: the step's gradient has no slot behind it; the loss kind travels in the Ask)
    const gmc_model model{GMC_VERSION, N, F, 3, 0, param, param + nW1, param + nW1 + F, param + nW1 + F + (long)F * 3, 0.f, 0u, 0u, w1_slab};
    Call c{batch, &model};
    int rc = open(c, Ask{true, true, false, loss_kind}, workspace, workspace_bytes, stream, grad, P != nullptr);
    if (rc) return rc;
    if (batch->R == 0 || !c.w.plan.fused) {  // general shapes: gradient, then the stand-alone Adam
        rc = fwd_bwd(c, C, P, S, loss, grad, false);
        return rc ? rc : gmc_adam_devstep_model_f32(param, grad, mom, var, N, F, w1_slab, lr, beta1, beta2, eps, step_counter,
                                                    stream);
    }
    rc = forward_body(c);
    if (rc) return rc;
    // One graph per step (the reference's own schedule): the backward launch computes the head as well - every one of
    // its workgroups for itself, the rows (GY2, dinv) never leave the CU - three launches per graph-step instead of four.
    // The head (launch) advances the step counter for the fused Adam of the finish kernel.
    const gmc_bwd1_head hd{c.w.Z0, c.w.plan.zparts, model.b2, C, P, S, loss, c.w.db2part, step_counter};
    if (c.w.plan.head_in_bwd) c.head = &hd;
    else if ((rc = head(c, C, P, S, loss, true, step_counter))) return rc;
    const AdamFuse af{param, mom, var, lr, beta1, beta2, eps, step_counter, w1_slab};
    c.adam = &af;
    return backward_body(c, grad);
}

extern "C" int gmc_backward_from_gp(const gmc_batch *batch, const gmc_model *model, void *workspace, size_t workspace_bytes,
                                    const float *P, const float *GP, float *grad, gmc_stream_t stream) {
    return backward_call(batch, model, nullptr, 0, workspace, workspace_bytes, P, GP, grad, nullptr, 0, stream);
}

extern "C" int gmc_backward_features_from_gp(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx,
                                             void *workspace, size_t workspace_bytes, const float *P, const float *GP,
                                             float *grad, float *dX, int64_t lddx, gmc_stream_t stream) {
    if (!X) return GMC_ERR_NULL;   // (what tells the plain call from this one)
    return backward_call(batch, model, X, ldx, workspace, workspace_bytes, P, GP, grad, dX, lddx, stream);
}

// ---- number_classes K in 2..GMC_KWAY_MAX_CLASSES: the row-kernel sequence with the K-wide kernels of kway.hip -------------
namespace {

struct KwayWorkspace {
    long ld;         // leading dimension of the [R,F] buffers (F rounded up to 32 floats)
    float *T0;       // [R,ld]  dinv o (A_val @ W1[:n]), later Gs = dinv o Gpre
    float *H;        // [R,ld]  relu(conv1), later U = dinv o (A @ Gs)
    float *Z0;       // [R,K]
    float *GY2;      // [R,K]
    float *part;     // [tiles,F,K+1]
    float *db2part;  // [B,K]
    float *dw1part;  // [chunks,N,F]
    int32_t *S;      // [R]            gmc_large_* only (large_carve): the decode, for the loss launch
    float *headpart; // [slots,K+1]    ... the head's tile partials (gmc_large_headpart_floats)
    float *GZd;      // [R,K]          ... dinv o GZ (training)
    size_t bytes;
};

// base == nullptr: sizes only
KwayWorkspace kway_carve(const gmc_batch *b, const gmc_model *m, bool training, void *base) {
    KwayWorkspace w{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(static_cast<char *>(base) + off) : nullptr;
        off += align_up(floats * sizeof(float));
        return p;
    };
    const size_t R = (size_t)b->R, F = (size_t)m->F, K = (size_t)m->K;
    w.ld = (long)((F + 31) / 32 * 32);
    w.T0 = take(R * w.ld);
    w.H = take(R * w.ld);
    w.Z0 = take(R * K);
    if (training) {
        w.GY2 = take(R * K);
        w.part = take((size_t)gmc_hidden_tiles(b->R) * F * (K + 1));
        w.db2part = take((size_t)b->B * K);
        w.dw1part = take(gmc_dw1_scratch_floats(b, m->N, m->F, false));
    }
    w.bytes = off;
    return w;
}

bool kway_classes_ok(int K) { return K >= 2 && K <= GMC_KWAY_MAX_CLASSES; }

// would gmc_kway_* refuse the batch for its size (the head keeps a graph's [n,K] tiles in a CU's LDS)?
bool kway_too_large(const gmc_batch *b, const gmc_model *m) {
    return b->n_max > GMC_MAX_GRAPH_NODES || gmc_kway_head_lds_bytes(b->n_max, m->K, loss_of(m)) > GMC_KWAY_LDS_BYTES;
}

// steps 1 and 2 of the documented order; large: the gmc_large_* / gmc_fn_* entry points (several workgroups per graph: no
// LDS bound); dense: features with their own N columns - a graph may then have more nodes than conv1.weight has rows
int kway_check(const gmc_batch *b, const gmc_model *m, bool large = false, bool dense = false) {
    if (int rc = check_abi(b, m)) return rc;
    if (!b->goff || !b->rowptr || !b->gcol || !b->lcol || !b->dinv) return GMC_ERR_NULL;
    if (!m->W1 || !m->b1 || !m->W2 || !m->b2) return GMC_ERR_NULL;
    if (!kway_classes_ok(m->K)) return GMC_ERR_CLASSES;
    if (b->B < 0 || b->R < 0 || b->nnz < 0 || m->N <= 0 || m->F <= 0) return GMC_ERR_SHAPE;
    if (m->F % 4 || m->F > GMC_MAX_HIDDEN) return GMC_ERR_UNSUPPORTED;  // float4 rows
    if (!(m->dropout_p >= 0.f && m->dropout_p < 1.f)) return GMC_ERR_SHAPE;
    if (m->dropout_p > 0.f) return GMC_ERR_UNSUPPORTED;                 // the K-class sequence has no dropout
    if (m->W1_slab && !gmc_aligned16(m->W1_slab)) return GMC_ERR_ALIGN;
    if (b->B > 0 && (b->n_max < m->K || (large ? b->n_max > GMC_LARGE_MAX_GRAPH_NODES : kway_too_large(b, m))))
        return GMC_ERR_GRAPH_SIZE;
    if (!dense && b->n_max > m->N) return GMC_ERR_SHAPE;  // more nodes than rows of conv1.weight
    return GMC_OK;
}

// gmc_large_*: the same buffers, then what the row-parallel head of large.hip keeps between its launches
KwayWorkspace large_carve(const gmc_batch *b, const gmc_model *m, bool training, void *base) {
    KwayWorkspace w = kway_carve(b, m, training, base);
    size_t off = w.bytes;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(static_cast<char *>(base) + off) : nullptr;
        off += align_up(floats * sizeof(float));
        return p;
    };
    w.S = reinterpret_cast<int32_t *>(take((size_t)b->R));
    w.headpart = take(gmc_large_headpart_floats(b, m->K));
    if (training) w.GZd = take((size_t)b->R * m->K);
    w.bytes = off;
    return w;
}

struct KwayCall {
    const gmc_batch *b; const gmc_model *m;
    bool large = false;   // gmc_large_*: the head of large.hip, graphs up to GMC_LARGE_MAX_GRAPH_NODES nodes
    KwayWorkspace w{}; hipStream_t st = nullptr;
    const float *X = nullptr; long ldx = 0;   // gmc_fn_*: dense features [R, N] instead of the padded adjacency
    float *dX = nullptr; long lddx = 0;       // ... backward: dX = U @ W1^T when asked for
};

int kway_open(KwayCall &c, bool training, void *workspace, size_t workspace_bytes, gmc_stream_t stream, const float *P,
              const float *grad) {
    if (int rc = kway_check(c.b, c.m, c.large)) return rc;                           // 1. 2.
    if (!workspace || !P || (training && !grad)) return GMC_ERR_NULL;                // 4. workspace and outputs
    if (!gmc_aligned16(grad) || !gmc_aligned16(P) || !gmc_aligned16(c.m->W2)) return GMC_ERR_ALIGN;   // 5.
    c.w = c.large ? large_carve(c.b, c.m, training, workspace) : kway_carve(c.b, c.m, training, workspace);   // 6. size
    if (c.w.bytes > workspace_bytes) return GMC_ERR_WORKSPACE;
    c.st = static_cast<hipStream_t>(stream);
    return GMC_OK;
}

// the two layers up to Z0 = dinv o (H @ W2); c.X: layer 1's feature transform is a GEMM
int kway_layers(const KwayCall &c) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m; const KwayWorkspace &w = c.w;
    const int F = m->F;
    int rc;
    if (c.X) {   // T0 = dinv o (X @ W1)
        rc = gmc_gemm_launch(0, 0, b->R, F, m->N, c.X, c.ldx, m->W1, F, b->dinv, w.T0, w.ld, c.st);
    } else {
        // T0 = dinv o (A_val @ W1[:n]): a row gather of W1
        rc = gmc_spmm_launch(b->rowptr, b->lcol, b->vals, b->dinv, m->W1, F, nullptr, 0, w.T0, w.ld, b->R, F,
                             group_rows(b), nullptr, nullptr, GMC_K_GATHER_W1, c.st);
        if (!rc && c.large)   // (gmc_large_*: rows of more than 64 entries once more, summed in chunks - launchers.h)
            rc = gmc_large_hub_rows_launch(b->rowptr, b->lcol, b->vals, b->dinv, m->W1, F, nullptr, 0, w.T0, w.ld, b->R, F,
                                           GMC_K_GATHER_W1, c.st);
    }
    if (rc) return rc;
    // H = relu(dinv o (A @ T0) + b1)
    rc = gmc_spmm_launch(b->rowptr, b->gcol, nullptr, b->dinv, w.T0, w.ld, m->b1, 1, w.H, w.ld, b->R, F, group_rows(b),
                         nullptr, nullptr, GMC_K_AGG_FWD, c.st);
    if (!rc && c.large)
        rc = gmc_large_hub_rows_launch(b->rowptr, b->gcol, nullptr, b->dinv, w.T0, w.ld, m->b1, 1, w.H, w.ld, b->R, F,
                                       GMC_K_AGG_FWD, c.st);
    if (rc) return rc;
    return gmc_kway_hw2_launch(w.H, w.ld, b->dinv, m->W2, w.Z0, b->R, F, m->K, c.st);
}

// forward and head; GY2 / db2part of the workspace are filled when it was carved for training
int kway_forward_body(const KwayCall &c, float C, float *P, int32_t *S, float *loss) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m; const KwayWorkspace &w = c.w;
    if (int rc = kway_layers(c)) return rc;
    if (c.large)
        return gmc_large_head_launch(b, w.Z0, m->b2, C, m->K, loss_of(m), P, S, loss, w.S, w.GZd, w.headpart, w.GY2,
                                     w.db2part, c.st);
    return gmc_kway_head_launch(b, w.Z0, m->b2, C, m->K, loss_of(m), P, S, loss, w.GY2, w.db2part, c.st);
}

int kway_backward_body(const KwayCall &c, float *grad, const float *loss_tail) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m; const KwayWorkspace &w = c.w;
    const long F = m->F, K = m->K;
    float *dW1 = grad, *db1 = grad + (long)m->N * F, *dW2 = db1 + F, *db2 = dW2 + F * K;
    float *Gs = w.T0, *U = w.H;
    int rc = gmc_kway_hidden_bwd_launch(w.H, w.ld, w.GY2, m->W2, b->dinv, Gs, w.ld, w.part, b->R, m->F, m->K, c.st);
    if (rc) return rc;
    rc = gmc_kway_reduce_launch(w.part, gmc_hidden_tiles(b->R), m->F, m->K, dW2, db1, w.db2part, b->B, db2, c.st);
    if (rc) return rc;
    // conv1 backward aggregation:  U = dinv o (A @ Gs)
    rc = gmc_spmm_launch(b->rowptr, b->gcol, nullptr, b->dinv, Gs, w.ld, nullptr, 0, U, w.ld, b->R, m->F, group_rows(b),
                         nullptr, nullptr, GMC_K_AGG_BWD, c.st);
    if (!rc && c.large)
        rc = gmc_large_hub_rows_launch(b->rowptr, b->gcol, nullptr, b->dinv, Gs, w.ld, nullptr, 0, U, w.ld, b->R, m->F,
                                       GMC_K_AGG_BWD, c.st);
    if (rc) return rc;
    if (c.X) {   // dW1 = X^T @ U straight into grad, dX = U @ W1^T
        rc = gmc_gemm_launch(1, 0, m->N, m->F, b->R, c.X, c.ldx, U, w.ld, nullptr, dW1, F, c.st);
        if (!rc && c.dX) rc = gmc_gemm_launch(0, 1, b->R, m->N, m->F, U, w.ld, m->W1, F, nullptr, c.dX, c.lddx, c.st);
    } else {
        rc = gmc_dw1_launch(b, U, w.ld, dW1, w.dw1part, m->N, m->F, false, c.st);
    }
    if (rc || !loss_tail) return rc;
    return gmc_loss_tail_launch(loss_tail, b->B, db2 + K, c.st);
}

}  // namespace

extern "C" size_t gmc_kway_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training) {
    if (check_abi(batch, model) || !kway_classes_ok(model->K)) return 0;
    return kway_carve(batch, model, training != 0, nullptr).bytes;
}

namespace {

int kway_forward_call(KwayCall c, float C, void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                      gmc_stream_t stream) {
    int rc = kway_open(c, false, workspace, workspace_bytes, stream, P, nullptr);
    if (rc || c.b->R == 0) return rc;
    return kway_forward_body(c, C, P, S, loss);
}

int kway_train_call(KwayCall c, float C, void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                    float *grad, gmc_stream_t stream) {
    int rc = kway_open(c, true, workspace, workspace_bytes, stream, P, grad);
    if (rc) return rc;
    const gmc_model *model = c.m;
    const bool tail = (model->flags & GMC_MODEL_GRAD_TAIL) != 0;
    if (tail && !loss) return GMC_ERR_NULL;
    if (c.b->R == 0) {
        const size_t n = (size_t)model->N * model->F + model->F + (size_t)model->F * model->K + model->K + (tail ? 1 : 0);
        return (int)hipMemsetAsync(grad, 0, n * sizeof(float), c.st);
    }
    rc = kway_forward_body(c, C, P, S, loss);
    return rc ? rc : kway_backward_body(c, grad, tail ? loss : nullptr);
}

}  // namespace

extern "C" int gmc_kway_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                                size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream) {
    return kway_forward_call(KwayCall{batch, model}, C, workspace, workspace_bytes, P, S, loss, stream);
}

extern "C" int gmc_kway_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                                      size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad,
                                      gmc_stream_t stream) {
    return kway_train_call(KwayCall{batch, model}, C, workspace, workspace_bytes, P, S, loss, grad, stream);
}

// ---- graphs beyond GMC_MAX_GRAPH_NODES: the same sequence with the head of large.hip ---------------------------------------
// The shared launchers were read for anything sized by n_max or N and for 32-bit products before they were relied on at
// these sizes: gmc_spmm_launch (element offsets long; xcd_remap is the identity once a group exceeds the grid),
// gmc_kway_hw2_launch, gmc_kway_hidden_bwd_launch / gmc_hidden_tiles, gmc_kway_reduce_launch, gmc_dw1_launch /
// gmc_dw1_scratch_floats ((N+3)/4 workgroups, long offsets) and gmc_loss_tail_launch needed no change.
extern "C" size_t gmc_large_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training) {
    if (check_abi(batch, model) || !kway_classes_ok(model->K)) return 0;
    return large_carve(batch, model, training != 0, nullptr).bytes;
}

extern "C" int gmc_large_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                                 size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream) {
    return kway_forward_call(KwayCall{batch, model, true}, C, workspace, workspace_bytes, P, S, loss, stream);
}

extern "C" int gmc_large_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                                       size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad,
                                       gmc_stream_t stream) {
    return kway_train_call(KwayCall{batch, model, true}, C, workspace, workspace_bytes, P, S, loss, grad, stream);
}

extern "C" int gmc_large_required(const gmc_batch *batch, const gmc_model *model) {
    if (int rc = check_abi(batch, model)) return rc;
    if (!kway_classes_ok(model->K)) return GMC_ERR_CLASSES;
    if (batch->B <= 0) return 0;
    if (model->K == 3) return batch->n_max > GMC_MAX_GRAPH_NODES ? 1 : 0;   // gmc_*: check()
    return kway_too_large(batch, model) ? 1 : 0;                            // gmc_kway_*: kway_check()
}

// ---- the functional form of the model: probabilities out, a caller's dLoss/dP in (functional.hip) -----------------------------
namespace {

// gmc_kway_*'s training buffers (the dW1 scratch only without features: with them dW1 is a GEMM into grad), then dinv o GZ
// [R,K] and the tile partials of db2
KwayWorkspace fn_carve(const gmc_batch *b, const gmc_model *m, bool features, void *base) {
    KwayWorkspace w{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(static_cast<char *>(base) + off) : nullptr;
        off += align_up(floats * sizeof(float));
        return p;
    };
    const size_t R = (size_t)b->R, F = (size_t)m->F, K = (size_t)m->K;
    w.ld = (long)((F + 31) / 32 * 32);
    w.T0 = take(R * w.ld);
    w.H = take(R * w.ld);
    w.Z0 = take(R * K);
    w.GY2 = take(R * K);
    w.part = take((size_t)gmc_hidden_tiles(b->R) * F * (K + 1));
    w.db2part = take((size_t)b->B * K);
    w.dw1part = take(features ? 0 : gmc_dw1_scratch_floats(b, m->N, m->F, false));
    w.GZd = take(R * K);
    w.headpart = take(gmc_fn_part_floats(b, m->K));
    w.bytes = off;
    return w;
}

// every argument check of gmc_fn_forward / gmc_fn_backward in the documented order, then the carving; c carries b, m and
// X / ldx / dX / lddx as the caller handed them over
int fn_open(KwayCall &c, void *workspace, size_t workspace_bytes, gmc_stream_t stream, const float *P, const float *GP,
            const float *grad, bool backward) {
    if (int rc = kway_check(c.b, c.m, true, c.X != nullptr)) return rc;              // 1. 2.
    if (c.X) {                                                                       // 3. the features
        if (c.ldx < c.m->N) return GMC_ERR_SHAPE;
        if (!gmc_aligned16(c.X) || c.ldx % 4 || !gmc_aligned16(c.m->W1)) return GMC_ERR_ALIGN;
    }
    if (!workspace || !P || (backward && (!GP || !grad))) return GMC_ERR_NULL;       // 4. workspace and outputs
    if (c.dX && c.lddx < c.m->N) return GMC_ERR_SHAPE;                               // 5.
    if (!gmc_aligned16(grad) || !gmc_aligned16(P) || !gmc_aligned16(GP) || !gmc_aligned16(c.m->W2) ||
        (c.dX && (!gmc_aligned16(c.dX) || c.lddx % 4)))
        return GMC_ERR_ALIGN;
    c.w = fn_carve(c.b, c.m, c.X != nullptr, workspace);                             // 6. size
    if (c.w.bytes > workspace_bytes) return GMC_ERR_WORKSPACE;
    c.st = static_cast<hipStream_t>(stream);
    return GMC_OK;
}

}  // namespace

extern "C" size_t gmc_fn_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int features) {
    if (check_abi(batch, model) || !kway_classes_ok(model->K)) return 0;
    return fn_carve(batch, model, features != 0, nullptr).bytes;
}

extern "C" int gmc_fn_forward(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx, void *workspace,
                              size_t workspace_bytes, float *P, gmc_stream_t stream) {
    KwayCall c{batch, model, true};
    c.X = X; c.ldx = (long)ldx;
    int rc = fn_open(c, workspace, workspace_bytes, stream, P, nullptr, nullptr, false);
    if (rc || batch->B == 0 || batch->R == 0) return rc;
    rc = kway_layers(c);
    return rc ? rc : gmc_fn_prob_launch(batch, c.w.Z0, model->b2, model->K, P, c.st);
}

extern "C" int gmc_fn_backward(const gmc_batch *batch, const gmc_model *model, const float *X, int64_t ldx, void *workspace,
                               size_t workspace_bytes, const float *P, const float *GP, float *grad, float *dX,
                               int64_t lddx, gmc_stream_t stream) {
    KwayCall c{batch, model, true};
    c.X = X; c.ldx = (long)ldx; c.dX = dX; c.lddx = (long)lddx;
    int rc = fn_open(c, workspace, workspace_bytes, stream, P, GP, grad, true);
    if (rc) return rc;
    if (batch->B == 0 || batch->R == 0) {
        const size_t n = (size_t)model->N * model->F + model->F + (size_t)model->F * model->K + model->K;
        return (int)hipMemsetAsync(grad, 0, n * sizeof(float), c.st);
    }
    rc = gmc_fn_softmax_bwd_launch(batch, P, GP, model->K, c.w.GZd, c.w.headpart, c.w.db2part, c.w.GY2, c.st);
    return rc ? rc : kway_backward_body(c, grad, nullptr);
}

extern "C" size_t gmc_fn_cut_loss_workspace_bytes(const gmc_batch *batch, int32_t K) {
    if (!batch || batch->abi != GMC_VERSION || !kway_classes_ok(K) || batch->B < 0 || batch->R < 0) return 0;
    return align_up(gmc_fn_part_floats(batch, 1) * sizeof(float));
}

extern "C" int gmc_fn_cut_loss_f32(const gmc_batch *batch, int32_t K, int32_t terminals, const float *P, float C,
                                   int32_t loss_kind, void *workspace, size_t workspace_bytes, float *loss, float *GP,
                                   gmc_stream_t stream) {
    if (!batch) return GMC_ERR_NULL;                                                  // 1.
    if (batch->abi != GMC_VERSION) return GMC_ERR_ABI;                                // 2. the struct, K, loss_kind
    if (!batch->goff || !batch->rowptr || !batch->gcol || !batch->lcol) return GMC_ERR_NULL;
    if (!kway_classes_ok(K)) return GMC_ERR_CLASSES;
    if (batch->B < 0 || batch->R < 0 || batch->nnz < 0) return GMC_ERR_SHAPE;
    if (!gmc_loss_kind_ok(loss_kind)) return GMC_ERR_LOSS;
    if (batch->B > 0 && ((terminals && batch->n_max < K) || batch->n_max > GMC_LARGE_MAX_GRAPH_NODES))
        return GMC_ERR_GRAPH_SIZE;
    if (!workspace || !P || !loss) return GMC_ERR_NULL;                               // 4. workspace and outputs
    if (!gmc_aligned16(P) || !gmc_aligned16(GP)) return GMC_ERR_ALIGN;                // 5.
    if (gmc_fn_cut_loss_workspace_bytes(batch, K) > workspace_bytes) return GMC_ERR_WORKSPACE;   // 6.
    if (batch->B == 0 || batch->R == 0) return GMC_OK;
    return gmc_fn_loss_launch(batch, P, K, terminals != 0, C, loss_kind, static_cast<float *>(workspace), loss, GP,
                              static_cast<hipStream_t>(stream));
}

// ---- one model per graph: the K-class row-kernel sequence with the grouped kernels of instance.hip -------------------------
// model: W1 [R,F] (row goff[g] + l = node l of graph g), b1 [B,F], W2 [B,F,K], b2 [B,K]; model->N must be batch->R.
namespace {

struct InstWorkspace {
    long ld;         // leading dimension of the [R,F] buffers (F rounded up to 32 floats)
    float *T0;       // [R,ld]  dinv o (A_val @ W1), later Gs = dinv o Gpre
    float *H;        // [R,ld]  dinv o (A @ T0), then relu(. + b1_g), later U = dinv o (A @ Gs)
    float *Z0;       // [R,K]
    float *GY2;      // [R,K]
    float *part;     // [slots,F,K+1]
    int32_t *S;      // [R]            gmc_inst_large_* only (inst_large_carve): the decode, for the loss launch
    float *headpart; // [slots,K+1]    ... the head's tile partials (gmc_large_headpart_floats)
    float *GZd;      // [R,K]          ... dinv o GZ (training)
    size_t bytes;
};

// base == nullptr: sizes only
InstWorkspace inst_carve(const gmc_batch *b, const gmc_model *m, bool training, void *base) {
    InstWorkspace w{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(static_cast<char *>(base) + off) : nullptr;
        off += align_up(floats * sizeof(float));
        return p;
    };
    const size_t R = (size_t)b->R, F = (size_t)m->F, K = (size_t)m->K;
    w.ld = (long)((F + 31) / 32 * 32);
    w.T0 = take(R * w.ld);
    w.H = take(R * w.ld);
    w.Z0 = take(R * K);
    if (training) {
        w.GY2 = take(R * K);
        w.part = take(gmc_inst_part_floats(b, m->F, m->K));
    }
    w.bytes = off;
    return w;
}

// gmc_inst_large_*: the same buffers, then what the row-parallel head of instance_large.hip keeps between its launches
InstWorkspace inst_large_carve(const gmc_batch *b, const gmc_model *m, bool training, void *base) {
    InstWorkspace w = inst_carve(b, m, training, base);
    size_t off = w.bytes;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(static_cast<char *>(base) + off) : nullptr;
        off += align_up(floats * sizeof(float));
        return p;
    };
    w.S = reinterpret_cast<int32_t *>(take((size_t)b->R));
    w.headpart = take(gmc_large_headpart_floats(b, m->K));
    if (training) w.GZd = take((size_t)b->R * m->K);
    w.bytes = off;
    return w;
}

// steps 1 and 2 of the documented order (kway_check with the stacked W1: N is the batch's row count); large: the
// gmc_inst_large_* entry points (several workgroups per graph: no LDS bound)
int inst_check(const gmc_batch *b, const gmc_model *m, int terminals, bool large = false) {
    if (int rc = check_abi(b, m)) return rc;
    if (!b->goff || !b->rowptr || !b->gcol || !b->lcol || !b->dinv) return GMC_ERR_NULL;
    if (!m->W1 || !m->b1 || !m->W2 || !m->b2) return GMC_ERR_NULL;
    if (!kway_classes_ok(m->K)) return GMC_ERR_CLASSES;
    if (b->B < 0 || b->R < 0 || b->nnz < 0 || m->N < 0 || m->F <= 0 || (terminals != 0 && terminals != 1))
        return GMC_ERR_SHAPE;
    if (m->F % 4 || m->F > GMC_MAX_HIDDEN) return GMC_ERR_UNSUPPORTED;  // float4 rows
    if (!(m->dropout_p >= 0.f && m->dropout_p < 1.f)) return GMC_ERR_SHAPE;
    if (m->dropout_p > 0.f) return GMC_ERR_UNSUPPORTED;
    if (m->W1_slab && !gmc_aligned16(m->W1_slab)) return GMC_ERR_ALIGN;
    if (b->B > 0 && (b->n_max < (terminals ? m->K : 1) ||
                     (large ? b->n_max > GMC_LARGE_MAX_GRAPH_NODES : kway_too_large(b, m))))
        return GMC_ERR_GRAPH_SIZE;
    if (m->N != b->R) return GMC_ERR_SHAPE;  // W1 has one row per node of the batch
    return GMC_OK;
}

struct InstCall {
    const gmc_batch *b; const gmc_model *m;
    InstWorkspace w{}; hipStream_t st = nullptr;
    int terminals = 1;   // 0: the head overrides no row (the _t entry points)
    bool large = false;  // gmc_inst_large_*: the kernels of instance_large.hip, graphs up to GMC_LARGE_MAX_GRAPH_NODES nodes
    const float *node_cost = nullptr;   // [R,K] per-node class costs of the loss (the _c entry points; never with large)
};

int inst_open(InstCall &c, bool training, void *workspace, size_t workspace_bytes, gmc_stream_t stream, const float *P,
              const float *grad) {
    if (int rc = inst_check(c.b, c.m, c.terminals, c.large)) return rc;                           // 1. 2.
    if (!workspace || !P || (training && !grad)) return GMC_ERR_NULL;                // 4. workspace and outputs
    if (!gmc_aligned16(grad) || !gmc_aligned16(P) || !gmc_aligned16(c.m->W2)) return GMC_ERR_ALIGN;   // 5.
    if (c.large && !gmc_aligned16(c.m->W1)) return GMC_ERR_ALIGN;   // (the hub-row launches read W1 as float4 only)
    c.w = c.large ? inst_large_carve(c.b, c.m, training, workspace) : inst_carve(c.b, c.m, training, workspace);   // 6. size
    if (c.w.bytes > workspace_bytes) return GMC_ERR_WORKSPACE;
    c.st = static_cast<hipStream_t>(stream);
    return GMC_OK;
}

// the blocks of the flat gradient [dW1 [R,F] | db1 [B,F] | dW2 [B,F,K] | db2 [B,K]]
struct InstGrad { float *dW1, *db1, *dW2, *db2; size_t count; };
InstGrad inst_grad(const gmc_batch *b, const gmc_model *m, float *grad) {
    const size_t R = (size_t)b->R, B = (size_t)b->B, F = (size_t)m->F, K = (size_t)m->K;
    InstGrad g{grad, grad + R * F, grad + R * F + B * F, grad + R * F + B * F + B * F * K, R * F + B * (F + F * K + K)};
    return g;
}

// forward and head; db2 != nullptr (training): GY2 of the workspace and db2 [B,K] - the head's per-graph sums - as well
int inst_forward_body(const InstCall &c, float C, float *P, int32_t *S, float *loss, float *db2) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m; const InstWorkspace &w = c.w;
    const int F = m->F;
    // T0 = dinv o (A_val @ W1): the gather of the stacked W1 by batch row id
    int rc = gmc_spmm_launch(b->rowptr, b->gcol, b->vals, b->dinv, m->W1, F, nullptr, 0, w.T0, w.ld, b->R, F,
                             group_rows(b), nullptr, nullptr, GMC_K_GATHER_W1, c.st);
    if (!rc && c.large)   // (gmc_inst_large_*: rows of more than 64 entries once more, summed in chunks - launchers.h)
        rc = gmc_large_hub_rows_launch(b->rowptr, b->gcol, b->vals, b->dinv, m->W1, F, nullptr, 0, w.T0, w.ld, b->R, F,
                                       GMC_K_GATHER_W1, c.st);
    if (rc) return rc;
    // dinv o (A @ T0); the graph's own bias and the relu are inst_hw2's
    rc = gmc_spmm_launch(b->rowptr, b->gcol, nullptr, b->dinv, w.T0, w.ld, nullptr, 0, w.H, w.ld, b->R, F, group_rows(b),
                         nullptr, nullptr, GMC_K_AGG_FWD, c.st);
    if (!rc && c.large)
        rc = gmc_large_hub_rows_launch(b->rowptr, b->gcol, nullptr, b->dinv, w.T0, w.ld, nullptr, 0, w.H, w.ld, b->R, F,
                                       GMC_K_AGG_FWD, c.st);
    if (rc) return rc;
    rc = c.large ? gmc_inst_large_hw2_launch(b, w.H, w.ld, m->b1, m->W2, w.Z0, F, m->K, c.st)
                 : gmc_inst_hw2_launch(b, w.H, w.ld, m->b1, m->W2, w.Z0, F, m->K, c.st);
    if (rc) return rc;
    if (c.large)
        return gmc_inst_large_head_launch(b, w.Z0, m->b2, C, m->K, loss_of(m), c.terminals, P, S, loss, w.S,
                                          db2 ? w.GZd : nullptr, w.headpart, w.GY2, db2, c.st);
    return gmc_kway_head_launch(b, w.Z0, m->b2, C, m->K, loss_of(m), P, S, loss, db2 ? w.GY2 : nullptr, db2, c.st, m->K,
                                c.terminals, c.node_cost);
}

int inst_backward_body(const InstCall &c, const InstGrad &g) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m; const InstWorkspace &w = c.w;
    float *Gs = w.T0, *U = w.H;
    int rc = gmc_inst_hidden_bwd_launch(b, w.H, w.ld, w.GY2, m->W2, Gs, w.ld, w.part, m->F, m->K, c.st);
    if (rc) return rc;
    rc = gmc_inst_fold_launch(b, w.part, m->F, m->K, g.dW2, g.db1, c.st);
    if (rc) return rc;
    // conv1 backward aggregation:  U = dinv o (A @ Gs)
    rc = gmc_spmm_launch(b->rowptr, b->gcol, nullptr, b->dinv, Gs, w.ld, nullptr, 0, U, w.ld, b->R, m->F, group_rows(b),
                         nullptr, nullptr, GMC_K_AGG_BWD, c.st);
    if (!rc && c.large)
        rc = gmc_large_hub_rows_launch(b->rowptr, b->gcol, nullptr, b->dinv, Gs, w.ld, nullptr, 0, U, w.ld, b->R, m->F,
                                       GMC_K_AGG_BWD, c.st);
    if (rc) return rc;
    // dW1 = A_val^T @ U = A_val @ U (undirected graphs, symmetric weights): every row of W1 belongs to one node
    rc = gmc_spmm_launch(b->rowptr, b->gcol, b->vals, nullptr, U, w.ld, nullptr, 0, g.dW1, m->F, b->R, m->F,
                         group_rows(b), nullptr, nullptr, GMC_K_DW1, c.st);
    if (!rc && c.large)
        rc = gmc_large_hub_rows_launch(b->rowptr, b->gcol, b->vals, nullptr, U, w.ld, nullptr, 0, g.dW1, m->F, b->R, m->F,
                                       GMC_K_DW1, c.st);
    return rc;
}

}  // namespace

extern "C" size_t gmc_inst_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training) {
    if (check_abi(batch, model) || !kway_classes_ok(model->K)) return 0;
    return inst_carve(batch, model, training != 0, nullptr).bytes;
}

namespace {

int inst_forward_call(InstCall c, float C, void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                      gmc_stream_t stream) {
    int rc = inst_open(c, false, workspace, workspace_bytes, stream, P, nullptr);
    if (rc || c.b->R == 0) return rc;
    return inst_forward_body(c, C, P, S, loss, nullptr);
}

int inst_train_call(InstCall c, float C, void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                    float *grad, gmc_stream_t stream) {
    int rc = inst_open(c, true, workspace, workspace_bytes, stream, P, grad);
    if (rc) return rc;
    const InstGrad g = inst_grad(c.b, c.m, grad);
    if (c.b->R == 0)   // an empty batch: its gradient (B * (F + F*K + K) floats: none when B is 0 too) is zero
        return g.count ? (int)hipMemsetAsync(grad, 0, g.count * sizeof(float), c.st) : GMC_OK;
    rc = inst_forward_body(c, C, P, S, loss, g.db2);
    return rc ? rc : inst_backward_body(c, g);
}

InstCall inst_call_of(const gmc_batch *batch, const gmc_model *model, int terminals, bool large,
                      const float *node_cost = nullptr) {
    InstCall c{batch, model};
    c.terminals = terminals;
    c.large = large;
    c.node_cost = node_cost;
    return c;
}

}  // namespace

extern "C" int gmc_inst_forward_t(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C,
                                  void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                                  gmc_stream_t stream) {
    return gmc_inst_forward_c(batch, model, terminals, nullptr, C, workspace, workspace_bytes, P, S, loss, stream);
}

extern "C" int gmc_inst_forward_c(const gmc_batch *batch, const gmc_model *model, int32_t terminals,
                                  const float *node_cost, float C, void *workspace, size_t workspace_bytes, float *P,
                                  int32_t *S, float *loss, gmc_stream_t stream) {
    return inst_forward_call(inst_call_of(batch, model, terminals, false, node_cost), C, workspace, workspace_bytes, P, S,
                             loss, stream);
}

extern "C" int gmc_inst_forward(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                                size_t workspace_bytes, float *P, int32_t *S, float *loss, gmc_stream_t stream) {
    return gmc_inst_forward_t(batch, model, 1, C, workspace, workspace_bytes, P, S, loss, stream);
}

extern "C" int gmc_inst_train_fwd_bwd_t(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C,
                                        void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                                        float *grad, gmc_stream_t stream) {
    return gmc_inst_train_fwd_bwd_c(batch, model, terminals, nullptr, C, workspace, workspace_bytes, P, S, loss, grad,
                                    stream);
}

extern "C" int gmc_inst_train_fwd_bwd_c(const gmc_batch *batch, const gmc_model *model, int32_t terminals,
                                        const float *node_cost, float C, void *workspace, size_t workspace_bytes,
                                        float *P, int32_t *S, float *loss, float *grad, gmc_stream_t stream) {
    return inst_train_call(inst_call_of(batch, model, terminals, false, node_cost), C, workspace, workspace_bytes, P, S,
                           loss, grad, stream);
}

extern "C" int gmc_inst_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, float C, void *workspace,
                                      size_t workspace_bytes, float *P, int32_t *S, float *loss, float *grad,
                                      gmc_stream_t stream) {
    return gmc_inst_train_fwd_bwd_t(batch, model, 1, C, workspace, workspace_bytes, P, S, loss, grad, stream);
}

// ---- one model per graph beyond GMC_MAX_GRAPH_NODES: the same sequence with the kernels of instance_large.hip ------------
// Every launch of the sequence was read for a grid dimension sized by n_max at n_max = GMC_LARGE_MAX_GRAPH_NODES:
// gmc_inst_hw2_launch has ceil(n_max / 4) workgroups in y (262,144: beyond 65,535 - gmc_inst_large_hw2_launch walks the
// tiles instead), gmc_inst_hidden_bwd_launch 16,384, the head 4,096, keep-best / early-stop 4,096; gmc_spmm_launch,
// gmc_large_hub_rows_launch and gmc_inst_fold_launch size no y or z dimension by n_max.  gmc_inst_adam_f32 refuses
// n_max * F beyond about 2^28 (GMC_ERR_SHAPE), as before.
extern "C" size_t gmc_inst_large_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training) {
    if (check_abi(batch, model) || !kway_classes_ok(model->K)) return 0;
    return inst_large_carve(batch, model, training != 0, nullptr).bytes;
}

extern "C" int gmc_inst_large_forward(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C,
                                      void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                                      gmc_stream_t stream) {
    return inst_forward_call(inst_call_of(batch, model, terminals, true), C, workspace, workspace_bytes, P, S, loss, stream);
}

extern "C" int gmc_inst_large_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, int32_t terminals, float C,
                                            void *workspace, size_t workspace_bytes, float *P, int32_t *S, float *loss,
                                            float *grad, gmc_stream_t stream) {
    return inst_train_call(inst_call_of(batch, model, terminals, true), C, workspace, workspace_bytes, P, S, loss, grad,
                           stream);
}

// ---- graph-attention first layer: the row-kernel sequence with the kernels of attention.hip -------------------------------
namespace {

struct AttWorkspace {
    long ld;           // leading dimension of the [R,F] buffers (F rounded up to 32 floats)
    float *T;          // [R,ld]  X @ W1 (kept for the backward)
    float *H;          // [R,ld]  relu(attention aggregation + b1), later dT
    float *Z0;         // [R,3]
    float *s_src, *s_dst, *alpha_s;   // [R]
    float *alpha_e;    // [nnz]
    float *G;          // [R,ld]  gradient at layer 1's pre-activation
    float *GY2;        // [R,4]
    float *part;       // [tiles,F,4]
    float *db2part;    // [B,3]
    float *dw1part;    // [chunks,N,F]
    float *ones, *dz_s, *ds_src, *ds_dst;   // [R]
    float *dz_e;       // [nnz]
    float *apart;      // [tiles,2,F]
    size_t bytes;
};

// base == nullptr: sizes only
AttWorkspace att_carve(const gmc_batch *b, const gmc_model *m, bool training, void *base) {
    AttWorkspace w{};
    size_t off = 0;
    auto take = [&](size_t floats) {
        float *p = base ? reinterpret_cast<float *>(static_cast<char *>(base) + off) : nullptr;
        off += align_up(floats * sizeof(float));
        return p;
    };
    const size_t R = (size_t)b->R, F = (size_t)m->F, nnz = (size_t)b->nnz;
    w.ld = (long)((F + 31) / 32 * 32);
    w.T = take(R * w.ld);
    w.H = take(R * w.ld);
    w.Z0 = take(R * 3);
    w.s_src = take(R);
    w.s_dst = take(R);
    w.alpha_s = take(R);
    w.alpha_e = take(nnz);
    if (training) {
        w.G = take(R * w.ld);
        w.GY2 = take(R * 4);
        w.part = take((size_t)gmc_hidden_tiles(b->R) * F * 4);
        w.db2part = take((size_t)b->B * 3);
        w.dw1part = take(gmc_dw1_scratch_floats(b, m->N, m->F, false));
        w.ones = take(R);
        w.dz_s = take(R);
        w.ds_src = take(R);
        w.ds_dst = take(R);
        w.dz_e = take(nnz);
        w.apart = take(gmc_att_avec_part_floats(b->R, m->F));
    }
    w.bytes = off;
    return w;
}

struct AttCall {
    const gmc_batch *b; const gmc_model *m;
    const float *a_src, *a_dst; float slope;
    AttWorkspace w{}; hipStream_t st = nullptr;
};

int att_open(AttCall &c, bool training, void *workspace, size_t workspace_bytes, gmc_stream_t stream, const float *P,
             const float *grad) {
    if (!c.b || !c.m || !c.a_src || !c.a_dst) return GMC_ERR_NULL;               // 1. (the vectors: as X of *_features)
    if (int rc = check(c.b, c.m, false)) return rc;                              // 2. (K must be 3)
    if (c.m->dropout_p > 0.f) return GMC_ERR_UNSUPPORTED;                        //    the attention sequence has no dropout
    if (!(c.slope >= 0.f && c.slope <= 1.f)) return GMC_ERR_SHAPE;               // 3. the slope of the leaky relu
    if (!workspace || !P || (training && !grad)) return GMC_ERR_NULL;            // 4. workspace and outputs
    if (!gmc_aligned16(grad) || !gmc_aligned16(c.m->W1) || !gmc_aligned16(c.m->b1)) return GMC_ERR_ALIGN;   // 5.
    c.w = att_carve(c.b, c.m, training, workspace);                              // 6. workspace size
    if (c.w.bytes > workspace_bytes) return GMC_ERR_WORKSPACE;
    c.st = static_cast<hipStream_t>(stream);
    return GMC_OK;
}

// forward and head; GY2 / db2part of the workspace are filled when it was carved for training
int att_forward_body(const AttCall &c, float C, float *P, int32_t *S, float *loss) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m; const AttWorkspace &w = c.w;
    const int F = m->F;
    // T = A_val @ W1[:n]: the row gather of W1 without a row scale
    int rc = gmc_spmm_launch(b->rowptr, b->lcol, b->vals, nullptr, m->W1, F, nullptr, 0, w.T, w.ld, b->R, F, group_rows(b),
                             nullptr, nullptr, GMC_K_GATHER_W1, c.st);
    if (rc) return rc;
    rc = gmc_att_scores_launch(w.T, w.ld, c.a_src, c.a_dst, w.s_src, w.s_dst, b->R, F, c.st);
    if (rc) return rc;
    rc = gmc_att_fwd_launch(b, w.T, w.ld, w.s_src, w.s_dst, c.slope, m->b1, w.alpha_e, w.alpha_s, w.H, F, c.st);
    if (rc) return rc;
    {
        GmcProbeScope probe(GMC_K_DENSE_MFMA, c.st);
        rc = gmc_hw2_rows_launch(w.H, b->dinv, m->W2, w.Z0, b->R, F, 0, w.ld, c.st);
    }
    if (rc) return rc;
    return gmc_head_launch(b, w.Z0, 1, m->b2, C, P, S, loss, w.GY2, w.GY2 ? w.db2part : nullptr, nullptr, c.st, loss_of(m));
}

int att_backward_body(const AttCall &c, float *grad, const float *loss_tail) {
    const gmc_batch *b = c.b; const gmc_model *m = c.m; const AttWorkspace &w = c.w;
    const long F = m->F;
    float *dW1 = grad, *db1 = grad + (long)m->N * F, *dW2 = db1 + F, *db2 = dW2 + F * 3;
    float *da_src = db2 + 3, *da_dst = da_src + F;
    float *dT = w.H;
    // layer 2's dinv travels in GY2; the hidden backward, given ones for layer 1's dinv, leaves G
    int rc = gmc_att_gy2_scale_launch(w.GY2, b->dinv, w.ones, b->R, c.st);
    if (rc) return rc;
    rc = gmc_hidden_bwd_launch(w.H, w.ld, w.GY2, m->W2, w.ones, w.G, w.ld, w.part, b->R, m->F, c.st);
    if (rc) return rc;
    rc = gmc_colsum_reduce_launch(w.part, gmc_hidden_tiles(b->R), m->F, dW2, db1, w.db2part, b->B, db2, c.st);
    if (rc) return rc;
    rc = gmc_att_edge_bwd_launch(b, w.T, w.G, w.ld, w.s_src, w.s_dst, c.slope, w.alpha_e, w.alpha_s, w.dz_e, w.dz_s,
                                 w.ds_dst, m->F, c.st);
    if (rc) return rc;
    rc = gmc_att_bwd_t_launch(b, w.G, w.ld, w.alpha_e, w.alpha_s, w.dz_e, w.dz_s, w.ds_dst, w.ds_src, c.a_src, c.a_dst,
                              dT, m->F, c.st);
    if (rc) return rc;
    rc = gmc_att_avec_launch(w.T, w.ld, w.ds_src, w.ds_dst, w.apart, da_src, da_dst, b->R, m->F, c.st);
    if (rc) return rc;
    rc = gmc_dw1_launch(b, dT, w.ld, dW1, w.dw1part, m->N, m->F, false, c.st);
    if (rc || !loss_tail) return rc;
    return gmc_loss_tail_launch(loss_tail, b->B, da_dst + F, c.st);
}

}  // namespace

extern "C" size_t gmc_att_workspace_bytes(const gmc_batch *batch, const gmc_model *model, int training) {
    if (check_abi(batch, model) || model->K != 3) return 0;
    return att_carve(batch, model, training != 0, nullptr).bytes;
}

extern "C" int gmc_att_forward(const gmc_batch *batch, const gmc_model *model, const float *a_src, const float *a_dst,
                               float slope, float C, void *workspace, size_t workspace_bytes, float *P, int32_t *S,
                               float *loss, gmc_stream_t stream) {
    AttCall c{batch, model, a_src, a_dst, slope};
    int rc = att_open(c, false, workspace, workspace_bytes, stream, P, nullptr);
    if (rc || batch->R == 0) return rc;
    return att_forward_body(c, C, P, S, loss);
}

extern "C" int gmc_att_train_fwd_bwd(const gmc_batch *batch, const gmc_model *model, const float *a_src,
                                     const float *a_dst, float slope, float C, void *workspace, size_t workspace_bytes,
                                     float *P, int32_t *S, float *loss, float *grad, gmc_stream_t stream) {
    AttCall c{batch, model, a_src, a_dst, slope};
    int rc = att_open(c, true, workspace, workspace_bytes, stream, P, grad);
    if (rc) return rc;
    const bool tail = (model->flags & GMC_MODEL_GRAD_TAIL) != 0;
    if (tail && !loss) return GMC_ERR_NULL;
    if (batch->R == 0) {
        const size_t n = (size_t)model->N * model->F + model->F + (size_t)model->F * 3 + 3 + 2 * (size_t)model->F + (tail ? 1 : 0);
        return (int)hipMemsetAsync(grad, 0, n * sizeof(float), c.st);
    }
    rc = att_forward_body(c, C, P, S, loss);
    return rc ? rc : att_backward_body(c, grad, tail ? loss : nullptr);
}
