"""CPU checks of one model per graph (include/gcnmaxcut.h, gmc_inst_*; engine.InstanceEngine; solve_dataset): the premise
pinned to the restatement of the reference (a model of n_nodes = n_g on the one-graph dataset IS the instance), the flat
layout, the per-graph Xavier init, keep-best, the status codes of the entry points in the documented order (fake
pointers: no call reaches a launch), the chunking of solve_dataset with a stub engine, its refusals, and the precondition
of the GPU cases of tests/test_gpu_instance.py on the float64 reference."""
import ctypes as C
import math

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import instance_ref as IR
from tests import kway_ref as KR
from tests import test_api_status as A
from tests import stepcheck, util
from tests.stepcheck import KEYS

SOME, ODD, BIG = A.SOME, A.ODD, A.BIG


# ---- the premise: the reference's model with n_nodes = n_g, trained on graph g alone, is graph g's instance
def oracle_step(nx_g, params, Cc):
    """Loss, P and autograd gradient of oracle.ref_dense (the restatement of the reference) in float64 for a model of
    n_nodes = n: the features are the adjacency padded to n columns; the loss pads to its hard-coded 1000."""
    n = nx_g.number_of_nodes()
    g = R.graph_from_networkx(nx_g)
    x = R.dense_adjacency(nx_g, n, torch.float64)
    a_pad = R.dense_adjacency(nx_g, R.PAD, torch.float64)
    leaf = {k: torch.tensor(np.asarray(v, np.float64), requires_grad=True) for k, v in params.items()}
    p = R.forward(leaf, g, x)
    loss = R.cut_loss(R.straight_through_one_hot(R.override_terminals(p)), a_pad, Cc)
    loss.backward()
    return float(loss.item()), p.detach().numpy(), {k: v.grad.numpy() for k, v in leaf.items()}


@pytest.mark.parametrize("spec,weights", [((14, 3, 1), "unit"), ((11, 4, 2), "real")])
def test_premise_at_three_classes_against_the_restatement_of_the_reference(built, spec, weights):
    g = util.near_regular(*spec)
    if weights == "real":
        rng = np.random.RandomState(7)
        for u, v in g.edges():
            g[u][v]["weight"] = float(np.float32(rng.uniform(0.3, 3.0)))
    n, F, Cc = g.number_of_nodes(), 6, 1.3
    params = KR.random_params(n, F, 3, 5)
    loss, P, grads = oracle_step(g, params, Cc)
    ref = IR.graph_step(KR.csr_of_handle(built.from_networkx(g)), params, Cc, "cut")
    assert np.abs(P - ref.P).max() < 1e-12
    assert abs(loss - ref.loss[0]) < 1e-12
    for k in KEYS:
        assert grads[k].shape == ref.grads[k].shape and np.abs(grads[k] - ref.grads[k]).max() < 1e-12, k


@pytest.mark.parametrize("K", (2, 5))
@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
def test_premise_at_other_class_counts_against_the_shared_model_restatement(built, K, loss):
    """A graph's instance is the K-class model restricted to the graph: in a shared model of N > n_g rows whose first n_g
    rows are the instance's, the graph alone gives the same P and loss, the same gradient on those rows and none below;
    and the batch restatement is the per-graph one, graph by graph."""
    graphs = [util.near_regular(13, 4, 3), util.near_regular(9, 3, 4)]
    csrs = [KR.csr_of_handle(built.from_networkx(g)) for g in graphs]
    params = [KR.random_params(len(c[0]) - 1, 8, K, 20 + i) for i, c in enumerate(csrs)]
    refs = IR.batch_step(csrs, params, 1.3, loss)
    for csr, p, ref in zip(csrs, params, refs):
        n = len(csr[0]) - 1
        shared = dict(p)
        shared["conv1.weight"] = np.concatenate([p["conv1.weight"], np.full((7, 8), 0.25, np.float32)])
        big = KR.f64_step([csr], shared, 1.3, loss)
        assert np.abs(big.P - ref.P).max() < 1e-12 and abs(big.loss[0] - ref.loss[0]) < 1e-12
        assert np.abs(big.grads["conv1.weight"][:n] - ref.grads["conv1.weight"]).max() < 1e-12
        assert not big.grads["conv1.weight"][n:].any()
        for k in KEYS[1:]:
            assert np.abs(big.grads[k] - ref.grads[k]).max() < 1e-12, k


# ---- the flat layout
def test_flat_layout_count_and_offsets(built):
    sizes, F, K = [5, 300, 65, 257], 12, 4
    offs, count = built.engine.instance_layout(sizes, F, K)
    R_, B = 627, 4
    assert offs == [0, R_ * F, R_ * F + B * F, R_ * F + B * F + B * F * K, R_ * F + B * (F + F * K + K)] == IR.flat_offsets(sizes, F, K)
    assert count == offs[-1] == 627 * 12 + 4 * (12 + 48 + 4)
    assert built.engine.instance_layout([], F, K) == ([0, 0, 0, 0, 0], 0)
    assert all(o % 4 == 0 for o in offs[:4])                 # every block 16-byte aligned for a float4 hidden width
    params = [KR.random_params(n, F, K, n) for n in sizes]
    flat = IR.pack(params)
    assert flat.size == count
    assert np.array_equal(flat[offs[0] + 5 * F:offs[0] + 305 * F].reshape(300, F), params[1]["conv1.weight"])
    assert np.array_equal(flat[offs[2] + 2 * F * K:offs[2] + 3 * F * K].reshape(F, K), params[2]["conv2.weight"])
    assert np.array_equal(flat[offs[3] + 3 * K:], params[3]["conv2.bias"])


# ---- the init
def test_xavier_bounds_and_determinism(built):
    sizes, F, K = [5, 40, 300], 10, 4
    torch.manual_seed(11)
    a = built.engine.draw_instance_parameters(sizes, F, K)
    torch.manual_seed(11)
    b = built.engine.draw_instance_parameters(sizes, F, K)
    torch.manual_seed(12)
    c = built.engine.draw_instance_parameters(sizes, F, K)
    assert len(a) == 3
    for n, (w1, w2), (v1, v2) in zip(sizes, a, b):
        assert tuple(w1.shape) == (n, F) and tuple(w2.shape) == (F, K)
        assert torch.equal(w1, v1) and torch.equal(w2, v2)
        b1, b2 = math.sqrt(6.0 / (n + F)), math.sqrt(6.0 / (F + K))
        assert float(w1.abs().max()) <= b1 and float(w2.abs().max()) <= b2
        if n * F >= 400:
            assert float(w1.abs().max()) > 0.9 * b1           # (uniform over the whole range, not a narrower one)
    assert not torch.equal(a[0][0], c[0][0])
    # the draws are the reference's for a model of n_nodes = n_g: graph by graph, conv1 and then conv2
    torch.manual_seed(11)
    for n, (w1, w2) in zip(sizes, a):
        r1 = torch.nn.init.xavier_uniform_(torch.empty(n, F))
        r2 = torch.nn.init.xavier_uniform_(torch.empty(F, K))
        assert torch.equal(r1, w1) and torch.equal(r2, w2)
    # a chunked dataset draws the same values as one chunk (solve_dataset under one seed)
    torch.manual_seed(11)
    two = built.engine.draw_instance_parameters(sizes[:2], F, K) + built.engine.draw_instance_parameters(sizes[2:], F, K)
    assert all(torch.equal(x[0], y[0]) and torch.equal(x[1], y[1]) for x, y in zip(a, two))


# ---- keep-best
def test_keep_best_first_minimum_wins_and_nan_never(built):
    kb = IR.KeepBest([0, 3, 5])
    assert np.isinf(kb.best_loss).all() and (kb.best_epoch == -1).all()
    S = [np.arange(5, dtype=np.int32) + 10 * e for e in range(5)]
    kb.update(S[0], [-3.0, np.nan], 0)
    assert kb.best_epoch.tolist() == [0, -1] and np.isinf(kb.best_loss[1])       # epoch 0 beats +inf; NaN does not
    assert kb.best_S.tolist() == [0, 1, 2, 0, 0]
    kb.update(S[1], [-3.0, -1.0], 1)                                               # a tie: the first minimum stays
    assert kb.best_epoch.tolist() == [0, 1] and kb.best_S.tolist() == [0, 1, 2, 13, 14]
    kb.update(S[2], [-4.0, np.nan], 2)
    assert kb.best_epoch.tolist() == [2, 1] and kb.best_S.tolist() == [20, 21, 22, 13, 14]
    kb.update(S[3], [-3.5, -0.5], 3)                                               # worse: nothing moves
    assert kb.best_epoch.tolist() == [2, 1] and kb.best_loss.tolist() == [-4.0, -1.0]
    assert kb.best_loss.dtype == np.float32 and kb.best_S.dtype == np.int32


# ---- status codes (fake pointers: no call reaches a launch)
def inst_call(hip, entry, batch=None, model=None, nbytes=BIG, **a):
    lib = hip.load()
    b = None if batch is None else C.byref(hip.GmcBatch(**batch))
    m = None if model is None else C.byref(hip.GmcModel(**model))
    g = {**dict(ws=SOME, P=SOME, S=None, loss=SOME, grad=SOME), **a}
    if entry == "gmc_inst_forward":
        return lib.gmc_inst_forward(b, m, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], None)
    return lib.gmc_inst_train_fwd_bwd(b, m, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], g["grad"], None)


def imodel(**kw):
    return A.model_fields(**{"K": 4, "N": 120, "flags": 0, **kw})       # N = the batch's rows (2 graphs of 60)


@pytest.mark.parametrize("entry", ("gmc_inst_forward", "gmc_inst_train_fwd_bwd"))
def test_status_codes_of_the_instance_entry_points(built, entry):
    hip = built.hip
    lib = hip.load()
    training = entry == "gmc_inst_train_fwd_bwd"
    bf = A.batch_fields()

    def code(**kw):
        kw.setdefault("batch", bf)
        kw.setdefault("model", imodel())
        return inst_call(hip, entry, **kw)

    assert code(batch=None) == -1 and code(model=None) == -1
    assert code(batch={**bf, "abi": 100}) == -8 and code(model=imodel(abi=100)) == -8
    for f in A.BATCH_PTRS:
        assert code(batch={**bf, f: None}) == -1, f
    for f in ("W1", "b1", "W2", "b2"):
        assert code(model=imodel(**{f: None})) == -1, f
    for K in (1, 9, 0, -3):
        assert code(model=imodel(K=K)) == -3, K
    for K in range(2, 9):                                                      # 3 included
        assert code(model=imodel(K=K), nbytes=0) == -5, K
    assert code(model=imodel(N=-1)) == -2 and code(batch={**bf, "R": -1}) == -2 and code(model=imodel(F=0)) == -2
    assert code(model=imodel(F=30)) == -7 and code(model=imodel(F=4100)) == -7
    assert code(model=imodel(dropout_p=1.0)) == -2
    assert code(model=imodel(dropout_p=0.5)) == -7
    assert code(model=imodel(K=1, dropout_p=0.5)) == -3                        # (documented order: K before dropout_p)
    assert code(model=imodel(W1_slab=ODD)) == -4
    assert code(batch={**bf, "n_max": 3}) == -6                                # fewer nodes than classes
    assert code(batch={**bf, "n_max": 4}, nbytes=0) == -5
    assert code(batch={**bf, "n_max": 4097}) == -6
    big = dict(R=4800, nnz=4800)
    assert code(batch={**bf, **big, "n_max": 2390}, model=imodel(K=8, N=4800), nbytes=0) == -5
    assert code(batch={**bf, **big, "n_max": 2420}, model=imodel(K=8, N=4800)) == -6   # the bound of gmc_kway_*
    assert code(batch={**bf, "n_max": 2420, "abi": 100}, model=imodel(K=8)) == -8
    assert code(model=imodel(N=1000)) == -2 and code(model=imodel(N=60)) == -2  # W1 has one row per node of the batch
    assert code(model=imodel(N=1000), batch={**bf, "n_max": 3}) == -6          # (graph size before that)
    assert code(ws=None) == -1 and code(P=None) == -1
    assert code(ws=None, model=imodel(N=1000)) == -2                           # (step 2 before step 4)
    assert code(P=ODD) == -4 and code(model=imodel(W2=ODD)) == -4
    assert code(P=ODD, ws=None) == -1                                          # (step 4 before step 5)
    if training:
        assert code(grad=None) == -1 and code(grad=ODD) == -4
        assert code(grad=ODD, nbytes=0) == -4                                  # (step 5 before step 6)
    assert code(loss=None, nbytes=0) == -5                                     # loss is optional; no tail slot here
    assert code(model=imodel(flags=1), loss=None, nbytes=0) == -5              # GMC_MODEL_GRAD_TAIL is not read
    for train_size in (0, 1):
        need = lib.gmc_inst_workspace_bytes(C.byref(hip.GmcBatch(**bf)), C.byref(hip.GmcModel(**imodel())), train_size)
        assert need > 256
        if bool(train_size) == training:
            assert code(nbytes=need - 1) == -5
    empty = {**bf, "B": 0, "R": 0, "nnz": 0, "n_max": 0}
    assert code(batch=empty, model=imodel(N=0)) == 0                           # launches nothing (count = 0: nothing to zero)


def test_instance_workspace_sizes_and_keep_best_codes(built):
    hip = built.hip
    lib = hip.load()
    bf = A.batch_fields(n=100, B=6)
    b = hip.GmcBatch(**bf)

    def size(K, training, **kw):
        return int(lib.gmc_inst_workspace_bytes(C.byref(b), C.byref(hip.GmcModel(**imodel(K=K, N=600, **kw))), training))

    assert size(1, 1) == 0 and size(9, 1) == 0 and size(4, 1, abi=100) == 0
    assert lib.gmc_inst_workspace_bytes(None, None, 1) == 0
    up = lambda x: (x + 255) // 256 * 256   # noqa: E731
    R_, ld, F = 600, 32, 32
    assert size(5, 0) == 2 * up(R_ * ld * 4) + up(R_ * 5 * 4)
    # training: GY2 [R,K] and the tile partials [R / 64 + B + 1][F][K+1]; no dW1 chunk partials, no db2 partials
    assert size(5, 1) == size(5, 0) + up(R_ * 5 * 4) + up((R_ // 64 + 6 + 1) * F * 6 * 4)

    def keep(batch=bf, **a):
        g = {**dict(S=SOME, loss=SOME, best_S=SOME, best_loss=SOME, best_epoch=SOME), **a}
        bb = None if batch is None else C.byref(hip.GmcBatch(**batch))
        return lib.gmc_inst_keep_best_f32(bb, g["S"], g["loss"], 3, g["best_S"], g["best_loss"], g["best_epoch"], None)

    assert keep(batch=None) == -1 and keep(batch={**bf, "abi": 100}) == -8 and keep(batch={**bf, "goff": None}) == -1
    for f in ("S", "loss", "best_S", "best_loss", "best_epoch"):
        assert keep(**{f: None}) == -1, f
    assert keep(batch={**bf, "B": -1}) == -2 and keep(batch={**bf, "n_max": 0}) == -2
    assert keep(batch={**bf, "B": 0, "R": 0, "n_max": 0}) == 0
    for name in ("gmc_inst_workspace_bytes", "gmc_inst_forward", "gmc_inst_train_fwd_bwd", "gmc_inst_keep_best_f32"):
        assert name in hip.SYMBOLS


def test_no_instantiation_of_the_instance_kernels_is_missing(built):
    names = util.kernel_symbols(built.hip.LIB_PATH)
    for K in range(2, 9):
        for kernel in ("inst_hw2_k_kernel", "inst_hidden_bwd_k_kernel"):
            assert any(f"{kernel}<{K}>" in s for s in names), (kernel, K)
    for kernel in ("inst_fold_kernel", "keep_rows_kernel", "keep_loss_kernel"):
        assert any(kernel in s for s in names), kernel


# ---- solve_dataset: chunking (a stub engine), refusals
def test_instance_chunks(built):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    chunks = T.instance_chunks([40, 30, 10, 50, 5], 50)
    assert [list(c) for c in chunks] == [[0], [1, 2], [3], [4]]
    assert [list(c) for c in T.instance_chunks([40, 30], 70)] == [[0, 1]]
    assert [list(c) for c in T.instance_chunks([40, 30], 40)] == [[0], [1]]
    assert [list(c) for c in T.instance_chunks([90, 5, 5], 10)] == [[0], [1, 2]]      # a larger graph: a chunk of its own
    assert T.instance_chunks([], 10) == []
    assert [list(c) for c in T.instance_chunks([3] * 7, 1 << 18)] == [list(range(7))]
    with pytest.raises(ValueError, match="max_rows_per_chunk"):
        T.instance_chunks([3], 0)


class StubEngine:
    """What solve_dataset asks of an InstanceEngine, on the CPU: the loss of graph g at epoch e is -(size + e % 3), the
    partition of epoch e is e everywhere but on the terminals."""
    made = []

    def __init__(self, handles, F, K, device=None, *, values=None):
        self.sizes = [h.n for h in handles]
        self.F, self.K, self.B, self.R = F, K, len(handles), sum(self.sizes)
        self.device = torch.device("cpu")
        self.values, self.steps, self.reset = values, 0, 0
        self.keep = IR.KeepBest(np.concatenate([[0], np.cumsum(self.sizes)]))
        StubEngine.made.append(self)

    def reset_parameters(self):
        self.reset += 1

    def train_fwd_bwd(self, C_, loss="cut"):
        e = self.steps
        S = torch.full((self.R,), e, dtype=torch.int32)
        off = 0
        for n in self.sizes:
            S[off:off + self.K] = torch.arange(self.K, dtype=torch.int32)
            off += n
        losses = torch.tensor([-(n + e % 3) * C_ for n in self.sizes], dtype=torch.float32)
        return torch.full((self.R, self.K), 1.0 / self.K), S, losses

    def adam_step(self, lr):
        self.steps += 1
        self.lr = lr

    def keep_best(self, S, losses, epoch):
        assert epoch == self.steps - 1
        self.keep.update(S.numpy(), losses.numpy(), epoch)

    best_S = property(lambda self: torch.from_numpy(self.keep.best_S))
    best_loss = property(lambda self: torch.from_numpy(self.keep.best_loss))
    best_epoch = property(lambda self: torch.from_numpy(self.keep.best_epoch))

    def parameters(self):
        return [{"conv1.weight": torch.zeros(n, self.F), "conv1.bias": torch.zeros(self.F),
                 "conv2.weight": torch.zeros(self.F, self.K), "conv2.bias": torch.zeros(self.K)} for n in self.sizes]


def small_dataset(built, sizes):
    ds = {}
    for i, n in enumerate(sizes):
        g = util.near_regular(n, 3, i)
        ds[i] = [built.from_networkx(g), None, g, [0, 1, 2]]
    return ds


def test_solve_dataset_chunks_by_rows_with_a_stub_engine(built, monkeypatch):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.setattr(T, "InstanceEngine", StubEngine)
    monkeypatch.delenv("GCN_MAXCUT_LOSS", raising=False)
    monkeypatch.delenv("GCN_MAXCUT_LAYER1", raising=False)
    sizes = [40, 30, 10, 50, 6]
    ds = small_dataset(built, sizes)
    cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=3, number_epochs=5, learning_rate=0.01, C=2.0,
                           patience=1, tolerance=1e9)                             # (both ignored: no early stopping)
    StubEngine.made = []
    out = T.solve_dataset(ds, cfg, max_rows_per_chunk=50)
    assert [e.sizes for e in StubEngine.made] == [[40], [30, 10], [50], [6]]
    assert all(e.steps == 5 and e.reset == 1 and e.lr == 0.01 and e.F == 8 and e.K == 3 for e in StubEngine.made)
    assert all(e.values == [None] * e.B for e in StubEngine.made)                  # unit weights
    assert len(out) == 5
    for n, res, item in zip(sizes, out, ds.values()):
        assert sorted(res) == ["best_epoch", "best_loss", "cut", "loss_history", "model", "partition", "probabilities"]
        assert res["loss_history"] == [-(n + e % 3) * 2.0 for e in range(5)]
        assert res["best_loss"] == min(res["loss_history"]) and res["best_epoch"] == 2      # first minimum: epoch 2, not 5
        assert res["partition"] == [0, 1, 2] + [2] * (n - 3)
        assert res["cut"] == TN.calculate_cut_value(res["partition"], item[2])
        assert tuple(res["probabilities"].shape) == (n, 3)
        assert callable(res["model"])
    StubEngine.made = []
    T.solve_dataset(ds, cfg)                                                       # the default: one chunk
    assert [e.sizes for e in StubEngine.made] == [sizes]
    assert T.solve_dataset({}, cfg) == []


def test_solve_dataset_refusals_need_no_gpu(built, monkeypatch):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.setattr(T, "InstanceEngine", StubEngine)
    monkeypatch.delenv("GCN_MAXCUT_LAYER1", raising=False)
    ds = small_dataset(built, [12, 6])
    cfg = dict(n_nodes=64, hidden_dim=8, number_epochs=1)
    with pytest.raises(NotImplementedError, match="dropout"):
        T.solve_dataset(ds, T.TrainingConfig(dropout=0.25, **cfg))
    with pytest.raises(ValueError, match="at least 8 nodes"):
        T.solve_dataset(ds, T.TrainingConfig(number_classes=8, **cfg))
    with pytest.raises(ValueError, match="number_classes"):
        T.solve_dataset(ds, T.TrainingConfig(number_classes=9, **cfg))
    with pytest.raises(ValueError, match="unknown loss"):
        T.solve_dataset(ds, T.TrainingConfig(**cfg), loss="hinge")
    monkeypatch.setenv("GCN_MAXCUT_LAYER1", "attention")
    with pytest.raises(NotImplementedError, match="layer1"):
        T.solve_dataset(ds, T.TrainingConfig(**cfg))
    monkeypatch.delenv("GCN_MAXCUT_LAYER1")
    # beyond the one-workgroup head (K = 8: near 2400 nodes; either loss): train_model serves one large graph
    g = nx.cycle_graph(2500)
    large = {0: [built.from_networkx(g), None, g, list(range(8))]}
    with pytest.raises(ValueError, match="train_model"):
        T.solve_dataset(large, T.TrainingConfig(number_classes=8, **cfg))
    assert built.engine.instance_too_large(2420, 8) and not built.engine.instance_too_large(2380, 8, "expected_cut")
    assert built.engine.instance_too_large(4097, 2) and not built.engine.instance_too_large(4096, 2)
    assert built.engine.instance_too_large(4097, 3) and not built.engine.instance_too_large(4096, 3, "expected_cut")
    StubEngine.made = []
    T.solve_dataset({0: large[0]}, T.TrainingConfig(number_classes=2, **cfg))      # K = 2 takes 2500 nodes
    assert [e.sizes for e in StubEngine.made] == [[2500]]


# ---- the precondition of the GPU cases
@pytest.mark.parametrize("case", IR.CASES, ids=IR.case_id)
def test_gpu_cases_are_decided_on_the_float64_reference(built, case):
    handles = [built.from_networkx(g) for g in IR.case_graphs(case)]
    csrs = [KR.csr_of_handle(h) for h in handles]
    sizes = [h.n for h in handles]
    assert sizes == IR.case_sizes(case) and min(sizes) >= max(case.K, 3)
    assert any(c[2] is not None for c in csrs) == (case.weights == "real")
    margin, gap = IR.decided(csrs, IR.case_params(case), 1.3, case.loss)
    assert margin >= KR.MARGIN and gap >= KR.KINK, (IR.case_id(case), margin, gap)
    # the row bars are within float32's reach: a float32 numpy evaluation with its own order keeps half of ROW_TOL
    ratio = IR.f32_row_ratio(csrs, IR.case_params(case), 1.3, case.loss)
    assert ratio <= stepcheck.ROW_TOL / 2, (IR.case_id(case), ratio)


def test_row_bars_are_beyond_float32_on_a_tiny_graph_with_many_units(built):
    """Why the cases are seeded by `f32_row_ratio` too: the terminals-only graph of 8 nodes with 516 hidden units at the
    first seed the tie and kink rules allow (1).  A b1 entry that cancels to 1.7e-4 (below ROW_FLOOR of the largest,
    0.25) is off by 1.4e-7 in plain float32 numpy - 5.5e-4 of its bar's scale, the bar being 2e-4 - with nothing of the
    library involved."""
    case = IR.Case("edge", 8, "unit", "cut", 1)
    csr = KR.csr_of_handle(built.from_networkx(IR.case_graphs(case)[0]))
    p = IR.case_params(case)[0]
    margin, gap = IR.decided([csr], [p], 1.3, "cut")
    assert margin >= KR.MARGIN and gap >= KR.KINK
    assert IR.f32_row_ratio([csr], [p], 1.3, "cut") > stepcheck.ROW_TOL


def test_case_list_covers_what_it_promises():
    assert len(IR.CASES) == 32
    for K, hidden in ((2, 4), (3, 12), (5, 260), (8, 516)):
        assert IR.HIDDEN[K] == hidden
        assert IR.case_sizes(IR.Case("edge", K, "unit", "cut", 0)) == [max(K, 3), max(K + 1, 3), 65]
        assert IR.case_sizes(IR.Case("mixed", K, "unit", "cut", 0)) == [max(5, K), 300, 65, 257]
    for field, values in (("weights", ("unit", "real")), ("loss", ("cut", "expected_cut")), ("batch", ("edge", "mixed"))):
        for v in values:
            assert sum(getattr(c, field) == v for c in IR.CASES) == 16
