"""CPU tests of the K-class model (number_classes K in 2..8): the float64 restatement tests/kway_ref.py against the
3-wide ones it generalises, the host functions that became width-agnostic (override_fixed_nodes,
simple_partition_assignment, the terminal relabelling of graphExtender), the status codes of the three gmc_kway_* entry
points, and the precondition of the GPU cases: on the float64 reference no row of a case is near a tie and no unit near
the relu kink, so tests/test_gpu_kway.py can demand identical partitions everywhere."""
import ctypes as C
import json
import os

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import expected_cut_ref as ER
from tests import kway_ref as KR
from tests import stepcheck
from tests import test_api_status as A
from tests.stepcheck import KEYS

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOME, ODD, BIG = A.SOME, A.ODD, A.BIG


def golden_csrs(built):
    out = []
    for rec in json.load(open(os.path.join(GOLD, "graphs.json")))["graphs"]:
        h = built.from_networkx(R.regular_graph(rec["n"], rec["d"], rec["seed"]))
        out.append(KR.csr_of_handle(h))
    return out


# ---- the restatement at K = 3 is the 3-wide one
def test_restatement_at_three_classes_is_the_three_wide_one(built):
    csrs = golden_csrs(built)
    params = KR.random_params(200, 16, 3, 5)
    W = [params[k] for k in KEYS]
    for i, (rp, cl, vl) in enumerate(csrs):
        dense, sparse = stepcheck.f64_forward(rp, cl, vl, *W), stepcheck.f64_forward_sparse(rp, cl, vl, *W)
        P = sparse["P"]
        S = KR.partition(P, 3)
        assert np.array_equal(S, stepcheck.f64_partition(P.copy())), i
        assert np.array_equal(KR.override(P), ER.override(P)), i
        for Cc in (1.0, 2.0, 1.7):
            loss, GP = KR.hard_loss_and_gp(rp, cl, vl, S, 3, Cc)
            s_loss, s_GP = stepcheck.f64_loss_and_gp_sparse(sparse, S, Cc)
            e_loss, e_GP = ER.hard_loss_and_gp(rp, cl, vl, S, Cc)
            assert loss == s_loss == e_loss, i
            assert np.array_equal(GP, s_GP) and np.array_equal(GP, e_GP), i
            if Cc != 1.7:   # the dense n x n form multiplies by C before it sums: the same bits for a power of two
                d_loss, d_GP = stepcheck.f64_loss_and_gp(dense, S, Cc)
                assert loss == d_loss and np.array_equal(GP, d_GP), i
            r_loss, r_GP = KR.relaxed_loss_and_gp(rp, cl, vl, P, Cc)
            x_loss, x_GP = ER.loss_and_gp(rp, cl, vl, P, Cc)
            assert r_loss == x_loss and np.array_equal(r_GP, x_GP), i
        assert KR.total_weight([(rp, cl, vl)]) == ER.total_weight([(rp, cl, vl)])
    # the whole step, both losses
    hard = KR.f64_step(csrs, params, 1.3, "cut")
    S_all = np.concatenate([KR.partition(stepcheck.f64_forward_sparse(*c, *W)["P"], 3) for c in csrs])
    old = stepcheck.f64_step(csrs, params, S_all, 1.3, sparse=True)
    assert np.array_equal(hard.P, old.P) and np.array_equal(hard.loss.astype(np.float32), old.loss) and old.near_ties == 0
    soft, old_soft = KR.f64_step(csrs, params, 1.3, "expected_cut"), ER.f64_step(csrs, params, 1.3)
    assert np.array_equal(soft.P, old_soft.P) and np.array_equal(soft.loss, old_soft.loss)
    for k in KEYS:
        assert np.array_equal(hard.grads[k], old.grads[k]), k
        assert np.array_equal(soft.grads[k], old_soft.grads[k]), k


def test_near_tie_rule_for_k_columns():
    P = np.array([[.5, .5], [.5, .5], [.3, .7], [.5 + 2e-7, .5 - 2e-7], [.9, .1]])
    assert KR.partition(P).tolist() == [0, 1, 1, 0, 0]
    assert KR.min_margin(P) == pytest.approx(4e-7)
    assert KR.near_tie_rows(P, np.array([0, 1, 1, 1, 0]), 1e-6) == 1          # the near-tie row may go either way
    with pytest.raises(AssertionError):
        KR.near_tie_rows(P, np.array([0, 1, 0, 0, 0]), 1e-6)                   # a decided row may not
    assert KR.min_margin(P[:2]) == float("inf")                                # terminals only


# ---- host functions that became width-agnostic
@pytest.mark.parametrize("K", (2, 3, 5))
def test_override_fixed_nodes_for_any_width(built, K):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    torch.manual_seed(K)
    h = torch.softmax(torch.randn(9, K), 1).requires_grad_(True)
    ov = T.override_fixed_nodes(h)
    want = torch.cat([torch.eye(K) + h.detach()[:K] - h.detach()[:K], h.detach()[K:]])
    assert torch.equal(ov.detach(), want)                                      # ((1 + p) - p: the reference's residue)
    assert ov.detach()[:K].argmax(1).tolist() == list(range(K))
    w = torch.randn(9, K)
    (ov * w).sum().backward()
    assert torch.equal(h.grad, w)                                              # straight-through on every row
    small = T.override_fixed_nodes(torch.full((2, 4), 0.25))                   # fewer rows than classes
    assert small.shape == (2, 4) and small.argmax(1).tolist() == [0, 1]


def test_override_fixed_nodes_at_three_classes_is_the_reference(built):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    for c in json.load(open(os.path.join(GOLD, "training.json")))["loss"]:
        P = np.asarray(c["P"], np.float32)
        ov = T.override_fixed_nodes(torch.from_numpy(P.copy())).numpy()
        assert ov.tobytes() == np.asarray(c["override"], np.float32).tobytes()


@pytest.mark.parametrize("K", (2, 5))
def test_simple_partition_assignment_for_any_width(built, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    rng = np.random.RandomState(K)
    P = rng.rand(12, K).astype(np.float32)
    P[:K] = np.roll(np.eye(K, dtype=np.float32), 1, axis=1)                    # the terminals' argmax is NOT their class
    want = P.argmax(1)
    want[:K] = np.arange(K)
    assert TN.simple_partition_assignment(torch.from_numpy(P)) == want.tolist()
    assert TN.simple_partition_assignment(torch.from_numpy(P[:1])) == [0]      # min(K, n) entries are fixed
    with pytest.raises(ValueError, match="number_classes"):
        TN._three_classes_only("the sampling post-processing", K)


# ---- terminals onto 0..K-1
def labelled(n, d, seed):
    g = R.regular_graph(n, d, seed)
    for u, v in g.edges():
        g[u][v]["weight"] = 1 + (u * 7 + v * 3) % 5                            # every edge recognisable
    return g


@pytest.mark.parametrize("K,terminals", [(2, [5, 9]), (2, [1, 0]), (4, [2, 7, 0, 11]), (4, [3, 2, 1, 0]), (4, [9, 1, 14, 3])])
def test_terminals_move_onto_the_first_labels(built, K, terminals):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    g = labelled(16, 3, K)
    before = g.copy()
    perm = GE.terminal_relabelling(list(terminals), K)
    assert sorted(perm) == sorted(perm.values())                               # a permutation of the labels it touches
    assert [perm[t] for t in terminals] == list(range(K))
    assert GE.move_terminals_to_front(g, list(terminals), K)
    full = {v: perm.get(v, v) for v in before.nodes}
    want = nx.relabel_nodes(before, full, copy=True)
    assert set(g.nodes) == set(range(16))
    assert {(min(u, v), max(u, v), d["weight"]) for u, v, d in g.edges(data=True)} == \
           {(min(u, v), max(u, v), d["weight"]) for u, v, d in want.edges(data=True)}
    for i, t in enumerate(terminals):                                          # node i is the old terminal i
        assert sorted(d["weight"] for _u, _v, d in g.edges(i, data=True)) == \
               sorted(d["weight"] for _u, _v, d in before.edges(t, data=True))


def test_terminal_lists_that_are_refused(built):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    assert GE.terminal_relabelling([4, 4], 2) is None and GE.terminal_relabelling([1, 2, 3], 2) is None
    g = labelled(16, 3, 1)
    edges = sorted(g.edges)
    assert not GE.move_terminals_to_front(g, [4, 99], 2) and sorted(g.edges) == edges   # a terminal the graph lacks


@pytest.mark.parametrize("K", (2, 4))
def test_process_graphs_from_folder_with_number_classes(built, K):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    graphs = {"a": labelled(16, 3, 1), "b": labelled(20, 5, 2), "dup": labelled(16, 3, 3), "short": labelled(16, 3, 4)}
    terms = {"a": [5, 9, 0, 12][:K], "b": [19, 1, 7, 3][:K], "dup": [4] * K, "short": [1, 2, 3, 4, 5][:K + 1]}
    before = {k: g.copy() for k, g in graphs.items()}
    ds = GE.process_graphs_from_folder(graphs, {k: list(v) for k, v in terms.items()}, 32, number_classes=K)
    assert sorted(ds) == [0, 1]                                                # the two bad lists are skipped
    for i, name in enumerate(("a", "b")):
        handle, a_pad, g, t = ds[i]
        n = before[name].number_of_nodes()
        assert t == list(range(K)) and handle.n == n and tuple(a_pad.shape) == (n, 32)
        perm = GE.terminal_relabelling(terms[name], K)
        full = {v: perm.get(v, v) for v in before[name].nodes}
        want = torch.zeros(n, 32)
        for u, v, d in before[name].edges(data=True):
            want[full[u], full[v]] = want[full[v], full[u]] = d["weight"]
        assert torch.equal(a_pad.cpu(), want)


def test_process_graphs_from_folder_at_three_classes_is_unchanged(built):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    out = []
    for kw in ({}, {"number_classes": 3}):
        graphs = {i: labelled(16, 3, 10 + i) for i in range(4)}
        terms = {0: [5, 9, 12], 1: [0, 7, 3], 2: [4, 1, 8], 3: [0, 1, 9]}     # (the last one is a list the reference skips)
        out.append((GE.process_graphs_from_folder(graphs, terms, 32, **kw), terms))
    (a, ta), (b, tb) = out
    assert sorted(a) == sorted(b) == [0, 1, 2] and ta == tb
    for i in a:
        assert torch.equal(a[i][1], b[i][1]) and a[i][3] == b[i][3] == [0, 1, 2]
        assert sorted(a[i][2].edges(data="weight")) == sorted(b[i][2].edges(data="weight"))
        assert np.array_equal(a[i][0].col, b[i][0].col) and np.array_equal(a[i][0].rowptr, b[i][0].rowptr)


# ---- status codes of the three entry points (fake pointers: no call reaches a launch)
def kway_call(hip, entry, batch=None, model=None, nbytes=BIG, **a):
    lib = hip.load()
    b = None if batch is None else C.byref(hip.GmcBatch(**batch))
    m = None if model is None else C.byref(hip.GmcModel(**model))
    g = {**dict(ws=SOME, P=SOME, S=None, loss=SOME, grad=SOME), **a}
    if entry == "gmc_kway_forward":
        return lib.gmc_kway_forward(b, m, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], None)
    return lib.gmc_kway_train_fwd_bwd(b, m, 1.0, g["ws"], nbytes, g["P"], g["S"], g["loss"], g["grad"], None)


def kmodel(**kw):
    return A.model_fields(**{"K": 4, **kw})


@pytest.mark.parametrize("entry", ("gmc_kway_forward", "gmc_kway_train_fwd_bwd"))
def test_status_codes_of_the_kway_entry_points(built, entry):
    hip = built.hip
    lib = hip.load()
    training = entry == "gmc_kway_train_fwd_bwd"
    bf = A.batch_fields()

    def code(**kw):
        kw.setdefault("batch", bf)
        kw.setdefault("model", kmodel())
        return kway_call(hip, entry, **kw)

    assert code(batch=None) == -1 and code(model=None) == -1
    assert code(batch={**bf, "abi": 100}) == -8 and code(model=kmodel(abi=100)) == -8
    for f in A.BATCH_PTRS:
        assert code(batch={**bf, f: None}) == -1, f
    for f in ("W1", "b1", "W2", "b2"):
        assert code(model=kmodel(**{f: None})) == -1, f
    for K in (1, 9, 0, -3):
        assert code(model=kmodel(K=K)) == -3, K
    for K in range(2, 9):                                                      # every class count in range gets past that
        assert code(model=kmodel(K=K), nbytes=0) == -5, K
    assert code(model=kmodel(N=0)) == -2 and code(batch={**bf, "R": -1}) == -2
    assert code(model=kmodel(F=30)) == -7 and code(model=kmodel(F=4100)) == -7
    assert code(model=kmodel(dropout_p=1.0)) == -2
    assert code(model=kmodel(dropout_p=0.5)) == -7                             # the K-class sequence has no dropout
    assert code(model=kmodel(K=1, dropout_p=0.5)) == -3                        # (documented order: K before dropout_p)
    assert code(batch={**bf, "n_max": 3}) == -6                                # fewer nodes than classes
    assert code(batch={**bf, "n_max": 4}, model=kmodel(K=4)) != -6
    assert code(batch={**bf, "n_max": 4097}) == -6
    # the head's [n,K] tiles must fit a CU's 160 KiB of LDS: K = 8 stops near n = 2400, K = 2 reaches 4096
    big = kmodel(K=8, N=4096)
    assert code(batch={**bf, "n_max": 2390}, model=big, nbytes=0) == -5
    assert code(batch={**bf, "n_max": 2420}, model=big) == -6
    assert code(batch={**bf, "n_max": 4096}, model=kmodel(K=2, N=4096), nbytes=0) == -5
    assert code(model=kmodel(N=48)) == -2                                      # more nodes than rows of conv1.weight
    assert code(ws=None) == -1 and code(P=None) == -1
    assert code(P=ODD) == -4 and code(model=kmodel(W2=ODD)) == -4
    if training:
        assert code(grad=None) == -1 and code(grad=ODD) == -4
        assert code(loss=None) == -1                                           # GMC_MODEL_GRAD_TAIL needs the losses
        assert code(loss=None, model=kmodel(flags=0), nbytes=0) == -5
    for train_size in (0, 1):
        need = lib.gmc_kway_workspace_bytes(C.byref(hip.GmcBatch(**bf)), C.byref(hip.GmcModel(**kmodel())), train_size)
        assert need > 256
        if bool(train_size) == training:
            assert code(nbytes=need - 1) == -5
    if not training:                                                           # returns before any launch
        assert code(batch={**bf, "B": 0, "R": 0, "nnz": 0, "n_max": 0}) == 0


def test_kway_workspace_sizes(built):
    hip = built.hip
    lib = hip.load()
    bf = A.batch_fields(n=100, B=6)
    b = hip.GmcBatch(**bf)

    def size(K, training, **kw):
        return int(lib.gmc_kway_workspace_bytes(C.byref(b), C.byref(hip.GmcModel(**kmodel(K=K, **kw))), training))

    assert size(1, 1) == 0 and size(9, 1) == 0 and size(4, 1, abi=100) == 0
    assert lib.gmc_kway_workspace_bytes(None, None, 1) == 0
    fwd = [size(K, 0) for K in range(2, 9)]
    trn = [size(K, 1) for K in range(2, 9)]
    assert fwd == sorted(fwd) and trn == sorted(trn) and all(t > f > 0 for f, t in zip(fwd, trn))
    # [R,ld] x 2 and [R,K]: the row-kernel buffers, each rounded up to 256 bytes
    R_, ld = 600, 32
    up = lambda x: (x + 255) // 256 * 256   # noqa: E731
    assert size(5, 0) == 2 * up(R_ * ld * 4) + up(R_ * 5 * 4)
    prev = lib.gmc_set_fuse(0)                                                 # the sequence does not depend on it
    try:
        assert [size(K, 1) for K in range(2, 9)] == trn
    finally:
        lib.gmc_set_fuse(prev)


def test_existing_entry_points_still_refuse_other_class_counts(built):
    hip = built.hip
    assert A.call(hip, "gmc_forward", A.batch_fields(), A.model_fields(K=2)) == -3
    assert A.call(hip, "gmc_train_fwd_bwd", A.batch_fields(), A.model_fields(K=4)) == -3
    assert hip.load().gmc_error_string(-3).decode().startswith("number_classes must be 3")
    for name in ("gmc_kway_workspace_bytes", "gmc_kway_forward", "gmc_kway_train_fwd_bwd"):
        assert name in hip.SYMBOLS


def test_engine_refuses_class_counts_outside_the_range(built):
    for K, kw in ((1, dict(kway=True)), (9, dict(kway=True)), (0, {}), (2, {}), (8, {})):
        with pytest.raises(ValueError, match="number_classes"):   # (2..8 without kway=True: the 3-class constructor)
            built.engine.FusedEngine(64, 16, K, device=torch.device("cpu"), **kw)


def test_refinement_calls_refuse_other_class_counts(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = labelled(16, 3, 1)
    for call in (TN.local_search_optimization, TN.annealing_optimization):
        for K in (2, 5):
            with pytest.raises(ValueError, match="number_classes"):
                call([0, 1] * 8, g, number_classes=K)


def test_cut_loss_keeps_requiring_three_columns(built):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    with pytest.raises(ValueError, match="number_classes"):
        T.cut_loss(None, torch.full((6, 2), 0.5))


def test_no_instantiation_of_the_kway_kernels_is_missing(built):
    names = [s for s in __import__("tests.util", fromlist=["util"]).kernel_symbols(built.hip.LIB_PATH) if "_k_kernel<" in s]
    for K in range(2, 9):
        for kernel in ("hw2_k_kernel", "hidden_bwd_k_kernel", "reduce_k_kernel"):
            assert any(f"{kernel}<{K}>" in s for s in names), (kernel, K)
        for soft in ("true", "false"):
            assert any(f"head_k_kernel<{K}, {soft}>" in s for s in names), (K, soft)


# ---- the precondition of the GPU cases
@pytest.mark.parametrize("case", KR.CASES, ids=KR.case_id)
def test_gpu_cases_are_decided_on_the_float64_reference(built, case):
    handles = [built.from_networkx(g) for g in KR.case_graphs(case)]
    csrs = [KR.csr_of_handle(h) for h in handles]
    assert all(h.n >= case.K for h in handles)
    assert any(c[2] is not None for c in csrs) == (case.weights == "real")
    params = KR.case_params(case)
    ref = KR.f64_step(csrs, params, 1.3, case.loss)
    off = 0
    for rp, _cl, _vl in csrs:
        n = len(rp) - 1
        margin = KR.min_margin(ref.P[off:off + n], case.K)
        assert margin >= KR.MARGIN, (KR.case_id(case), margin)
        off += n
    gap = KR.preactivation_gap(csrs, params)
    assert gap >= KR.KINK, (KR.case_id(case), gap)
    assert not stepcheck.kink_columns(csrs, params, KR.KINK, sparse=True).any()


@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
def test_three_way_comparison_batch_is_decided_too(built, loss):
    csrs = [KR.csr_of_handle(built.from_networkx(g)) for g in KR.three_way_graphs()]
    params = KR.three_way_params()
    ref = KR.f64_step(csrs, params, 1.3, loss)
    off = 0
    for rp, _cl, _vl in csrs:
        n = len(rp) - 1
        assert KR.min_margin(ref.P[off:off + n], 3) >= KR.MARGIN
        off += n
    assert KR.preactivation_gap(csrs, params) >= KR.KINK


def test_case_list_covers_what_it_promises():
    cases = KR.CASES
    for shape in KR.SHAPES:
        assert sum(c.shape == shape for c in cases) >= 2, shape
    for K in (2, 4, 5, 8):
        assert sum(c.K == K for c in cases) >= 2, K
    for loss in ("cut", "expected_cut"):
        assert sum(c.loss == loss for c in cases) >= 2
    assert {c.weights for c in cases} == {"unit", "real"}
    assert {KR.SHAPES[s][1] for s in KR.SHAPES} >= {4, 12, 260, 516}
