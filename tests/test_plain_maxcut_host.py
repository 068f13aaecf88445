"""CPU checks of plain max-K-cut (include/gcnmaxcut.h, "the terminals optional"): tests/plain_ref.py with first = K
equals the existing restatements output for output, gmc_order_host_t against the two host routines it generalises, the
status codes of every `_t` entry point in the documented order (no GPU needed), the Python refusals, and the seeding
rules of the cases tests/test_gpu_plain_instance.py runs."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import kway_search_ref as KS
from tests import large_round_ref as LRR
from tests import large_search_ref as LS
from tests import plain_ref as PR
from tests import rounding_ref as CR
from tests import seeded_ref as SR
from tests.test_refine_host import handles_of

KS_ALL = (2, 3, 4, 8)


def small_graphs(K):
    """(n, rowptr, col) of the shapes the GPU tests use that a CPU restatement walks in no time."""
    sizes = sorted({3, max(K, 3), K + 1, 65})
    return [PR.ring_with_chords(n, 10 + n) for n in sizes] + [PR.star_centre2(70)]


# ---- plain_ref with first = K is the existing restatements ---------------------------------------------------------------
@pytest.mark.parametrize("K", KS_ALL)
def test_order_with_terminals_is_the_existing_order(K):
    graphs = [g for g in small_graphs(K) if g[0] >= K]
    got, want = PR.order_arrays(graphs, K), LRR.order_arrays(graphs, K)
    for a, b in zip(got[:3], want[:3]):
        assert a.dtype == b.dtype and (a == b).all()
    assert got[3] == want[3]
    hs = handles_of([R.regular_graph(50, 6, 7), nx.complete_graph(9)])
    for a, b in zip(PR.order_arrays([(h.n, h.rowptr, h.col) for h in hs], K)[:3], CR.order_of_batch(hs, K)):
        assert (a == b).all()


def test_rounding_and_descent_with_terminals_are_the_existing_ones():
    seen = set()
    for K, n, rowptr, col, w, P in CR.cases():
        if (K, w is None) in seen:
            continue
        seen.add((K, w is None))
        got = PR.restate_round(n, rowptr, col, w, P, K, K, 100)
        seq = CR.round_sequential(n, rowptr, col, w, P, K)
        a1, sweeps = CR.descent(n, rowptr, col, w, seq, K, 100)
        assert (got["a0"] == seq).all() and (got["a1"] == a1).all() and got["sweeps"] == sweeps
        big = LRR.restate(n, np.asarray(rowptr, np.int64), np.asarray(col, np.int64), w, P, K, 100)
        assert (got["a0"] == big["a0"]).all() and (got["a1"] == big["a1"]).all() and got["sweeps"] == big["sweeps"]
        assert PR.expected_cut(n, rowptr, col, w, P, K, K) == CR.expected_cut(n, rowptr, col, w, P, K)
    assert len(seen) == 8


@pytest.mark.parametrize("K", KS_ALL)
def test_draws_with_terminals_are_the_existing_ones(K):
    key = int(SR.keys(5, [3])[0])
    for n in (3, K + 1, 65):
        P = PR.softmax_rows(n, K, 100 + n)
        assert (PR.assignments(P, key, 9, K) == KS.assignments(P, key, 9)).all()
        plain = PR.assignments(P, key, 9, 0)
        assert (plain[:, K:] == KS.assignments(P, key, 9)[:, K:]).all()       # the same counter for every local id
        m = min(n, K)
        assert not (plain[:, :m] == np.arange(m)).all()                       # ... and the first K are drawn too


@pytest.mark.parametrize("K", KS_ALL)
def test_annealing_with_terminals_is_the_existing_one(K):
    n, rowptr, col = PR.ring_with_chords(65, 3)
    table, inv_t = AR.levels(), LS.schedule(5)
    for w in (None, PR.integer_weights(n, rowptr, col, 1)):
        A = LS.candidates(n, K, 4, 9 + K)
        got = PR.anneal(n, rowptr, col, w, A, K, K, inv_t, table, 11, 20)
        out, snap, sweeps = KS.anneal(n, rowptr, col, w, A, K, inv_t, table, 11, 20)
        assert (got["assign"] == out).all() and (got["snap"] == snap).all() and (got["sweeps"] == sweeps).all()
        wide = PR.anneal(n, rowptr, col, w, A, K, K, inv_t, table, 11, 20, wide_layout=True)
        ref = LS.search(n, rowptr, col, w, A, K, inv_t, table, 11, 20)
        out_w, snap_w, sweeps_w = LS.anneal(n, rowptr, col, w, A, K, inv_t, table, 11, 20, wide_layout=True)
        assert (wide["assign"] == out_w).all() and (wide["snap"] == snap_w).all() and (wide["sweeps"] == sweeps_w).all()
        for k in ("assign", "cut_all", "snap", "sweeps", "best_assign"):
            assert (got[k] == ref[k]).all(), k
        assert got["best_idx"] == ref["best_idx"] and got["best_cut"] == ref["best_cut"]
        refined, refined_sweeps = KS.refine(n, rowptr, col, w, A, K, 20)
        local = PR.anneal(n, rowptr, col, w, A, K, K, np.zeros(0, np.float32), table, 0, 20)
        assert (local["assign"] == refined).all() and (local["sweeps"] == refined_sweeps).all()
        assert PR.best_single_move_gain(n, rowptr, col, w, local["assign"][1], K, K) == \
            LRR.best_single_move_gain(n, rowptr, col, w, local["assign"][1], K)


def test_without_terminals_the_path_and_the_star_reach_their_optimum():
    for graph, best in ((PR.path_021(), 2), (PR.star_centre2(70), 70)):
        n, rowptr, col = graph
        zero = np.zeros((1, n), np.int8)
        for first, want in ((0, best), (2, best - 1)):
            start = zero.copy()
            start[0, :first] = np.arange(first)
            out, _sweeps = PR.descent(n, start, 2, PR.tables_of(n, rowptr, col, None, first), 100)
            assert PR.cut(rowptr, col, None, out[0]) == want, (n, first)
            assert PR.best_single_move_gain(n, rowptr, col, None, out[0], 2, first) == 0.0


# ---- gmc_order_host_t ------------------------------------------------------------------------------------------------------
def order_t(lib, ba, K, terminals, cap=None):
    order = np.full(max(ba.R, 1), -7, np.int32)
    cgoff = np.full(ba.B + 1, -7, np.int32)
    cptr = np.full(ba.R + ba.B if cap is None else cap, -7, np.int32)
    most = C.c_int32(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    go = ba.goff.astype(np.int32)
    rc = lib.gmc_order_host_t(ba.B, p(go), p(ba.rowptr), p(ba.lcol), K, terminals, p(order), p(cgoff), p(cptr), cptr.size,
                              C.byref(most))
    return rc, order, cgoff, cptr, most.value


@pytest.mark.parametrize("K", KS_ALL)
def test_order_host_t(built, K):
    from gcn_max_cut_amd.graph import BatchArrays, GraphHandle
    lib = built.hip.load()
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    graphs = [PR.ring_with_chords(n, n) for n in (8, 65, 300, 9)] + [PR.star_centre2(70)]
    ba = BatchArrays([GraphHandle(n, rp, cl) for n, rp, cl in graphs])
    rc, order, cgoff, cptr, most = order_t(lib, ba, K, 1)
    assert rc == 0
    go = ba.goff.astype(np.int32)
    # terminals = 1: what the two existing host routines write, array for array
    o2, g2, c2 = np.full_like(order, -7), np.full_like(cgoff, -7), np.full_like(cptr, -7)
    assert lib.gmc_round_order_host(ba.B, p(go), p(ba.rowptr), p(ba.lcol), K, p(o2), p(g2), p(c2), c2.size) == 0
    o3, g3, c3, m3 = np.full_like(order, -7), np.full_like(cgoff, -7), np.full_like(cptr, -7), C.c_int32(-7)
    assert lib.gmc_large_round_order_host(ba.B, p(go), p(ba.rowptr), p(ba.lcol), K, p(o3), p(g3), p(c3), c3.size,
                                          C.byref(m3)) == 0
    for a, b, c in ((order, o2, o3), (cgoff, g2, g3), (cptr, c2, c3)):
        assert (a == b).all() and (a == c).all()
    assert most == m3.value
    # terminals = 0: every node is in the order, every class is an independent set, the restatement's arrays
    rc, order, cgoff, cptr, most = order_t(lib, ba, K, 0)
    assert rc == 0
    ref = PR.order_arrays(graphs, 0)
    assert (order[:ba.R] == ref[0]).all() and sorted(order[:ba.R].tolist()) == list(range(ba.R))
    assert (cgoff == ref[1]).all() and (cptr[:cgoff[-1]] == ref[2]).all() and (cptr[cgoff[-1]:] == -7).all()
    assert most == ref[3]
    for g in range(ba.B):
        r0 = int(ba.goff[g])
        for k in range(int(cgoff[g]), int(cgoff[g + 1]) - 1):
            nodes = set(order[cptr[k]:cptr[k + 1]].tolist())
            assert all(r0 <= v < int(ba.goff[g + 1]) for v in nodes)
            for v in nodes:
                nbrs = {int(u) + r0 for u in ba.lcol[ba.rowptr[v]:ba.rowptr[v + 1]]} - {v}
                assert not (nbrs & nodes), (g, k, v)


def test_order_host_t_status_codes(built):
    from gcn_max_cut_amd.graph import BatchArrays
    lib = built.hip.load()
    null, some, most = C.c_void_p(None), (C.c_int32 * 16)(), C.c_int32()
    f = lambda B=1, goff=some, K=4, t=0, cptr=some, cap=16, mc=C.byref(most): lib.gmc_order_host_t(
        B, goff, some, some, K, t, some, some, cptr, cap, mc)
    assert f(goff=null) == -1 and f(cptr=null) == -1 and f(mc=null) == -1                      # GMC_ERR_NULL
    for K in (-1, 0, 1, 9):
        assert f(K=K, t=2) == -3                                                               # GMC_ERR_CLASSES
    for t in (-1, 2, 7):
        assert f(t=t, B=-1) == -2                                                              # GMC_ERR_SHAPE
    assert f(B=-1) == -2
    goff = (C.c_int32 * 2)(0, 3)                                                               # a three-node graph
    assert f(goff=goff, K=4, t=1) == -6 and f(goff=goff, K=4, t=0) == 0                        # n = K - 1
    goff = (C.c_int32 * 2)(0, (1 << 20) + 1)
    assert f(goff=goff, t=0) == -6
    ba = BatchArrays(handles_of([R.regular_graph(60, 5, 1), nx.complete_graph(5)]))
    assert order_t(lib, ba, 5, 0, cap=ba.R + ba.B - 1)[0] == -2
    assert order_t(lib, ba, 5, 0, cap=ba.R + ba.B)[0] == 0
    assert order_t(lib, ba, 6, 1)[0] == -6 and order_t(lib, ba, 6, 0)[0] == 0


# ---- status codes of the device entry points (they fail before any HIP call) ---------------------------------------------
def _batch(hip, **kw):
    fields = dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, gcol=4096, lcol=4096, dinv=4096)
    return C.byref(hip.GmcBatch(**{**fields, **kw}))


def decoder_calls(lib):
    """name -> (call(batch, K, terminals, **overrides), names of the required pointers, upper node bound)."""
    some = C.c_void_p(4096)

    def args(kw, names):
        return [kw.get(n, some) for n in names]

    def rnd(b, K, t, **kw):
        P, order, cgoff, cptr, assign, cut = args(kw, ("P", "order", "cgoff", "cptr", "assign", "cut"))
        return lib.gmc_round_conditional_t_f32(b, P, K, t, order, cgoff, cptr, kw.get("sweeps_max", 10), assign, cut, None,
                                               None, None)

    def smp(b, K, t, **kw):
        P, gkey, cut_all, best_assign, best_cut, best_iter = args(kw, ("P", "gkey", "cut_all", "best_assign", "best_cut",
                                                                       "best_iter"))
        return lib.gmc_kway_decode_sample_seeded_t_f32(b, P, K, t, gkey, kw.get("iters", 4), None, cut_all, best_assign,
                                                       best_cut, best_iter, None)

    def ann(b, K, t, **kw):
        order, cgoff, cptr, assign, cut_all, best_assign, best_cut, best_idx = args(
            kw, ("order", "cgoff", "cptr", "assign", "cut_all", "best_assign", "best_cut", "best_idx"))
        return lib.gmc_kway_refine_anneal_t_f32(b, K, t, order, cgoff, cptr, kw.get("cands", 2), assign, some, 3, some, 0,
                                                kw.get("sweeps_max", 10), cut_all, best_assign, best_cut, best_idx, None,
                                                None, None)

    def lrnd(b, K, t, **kw):
        P, order, cgoff, cptr, ws, assign, cut = args(kw, ("P", "order", "cgoff", "cptr", "workspace", "assign", "cut"))
        return lib.gmc_large_round_conditional_t_f32(b, P, K, t, order, cgoff, cptr, 4, kw.get("sweeps_max", 10), ws,
                                                     kw.get("bytes", 1 << 30), assign, cut, None, None, None)

    def lls(b, K, t, **kw):
        order, cgoff, cptr, ws, assign, cut = args(kw, ("order", "cgoff", "cptr", "workspace", "assign", "cut"))
        return lib.gmc_large_local_search_t_f32(b, K, t, order, cgoff, cptr, 4, kw.get("sweeps_max", 10), ws,
                                                kw.get("bytes", 1 << 30), assign, cut, None, None)

    def lsmp(b, K, t, **kw):
        P, gkey, ws, cut_all, best_assign, best_cut, best_iter = args(
            kw, ("P", "gkey", "workspace", "cut_all", "best_assign", "best_cut", "best_iter"))
        return lib.gmc_large_sample_seeded_t_f32(b, P, K, t, gkey, kw.get("iters", 4), None, ws, kw.get("bytes", 1 << 30),
                                                 cut_all, best_assign, best_cut, best_iter, None)

    def lann(b, K, t, **kw):
        order, cgoff, cptr, assign, ws, cut_all, best_assign, best_cut, best_idx = args(
            kw, ("order", "cgoff", "cptr", "assign", "workspace", "cut_all", "best_assign", "best_cut", "best_idx"))
        return lib.gmc_large_anneal_t_f32(b, K, t, order, cgoff, cptr, 4, kw.get("cands", 2), assign, some, 3, some, 0,
                                          kw.get("sweeps_max", 10), ws, kw.get("bytes", 1 << 30), cut_all, best_assign,
                                          best_cut, best_idx, None, None, None)

    small, large = 4096, 1 << 20
    return {
        "gmc_round_conditional_t_f32": (rnd, ("P", "order", "cgoff", "cptr", "assign", "cut"), small, "sweeps_max"),
        "gmc_kway_decode_sample_seeded_t_f32": (smp, ("P", "gkey", "cut_all", "best_assign", "best_cut", "best_iter"),
                                                65535, "iters"),
        "gmc_kway_refine_anneal_t_f32": (ann, ("order", "cgoff", "cptr", "assign", "cut_all", "best_assign", "best_cut",
                                               "best_idx"), small, "cands"),
        "gmc_large_round_conditional_t_f32": (lrnd, ("P", "order", "cgoff", "cptr", "workspace", "assign", "cut"), large,
                                              "sweeps_max"),
        "gmc_large_local_search_t_f32": (lls, ("order", "cgoff", "cptr", "workspace", "assign", "cut"), large, "sweeps_max"),
        "gmc_large_sample_seeded_t_f32": (lsmp, ("P", "gkey", "workspace", "cut_all", "best_assign", "best_cut",
                                                 "best_iter"), large, "iters"),
        "gmc_large_anneal_t_f32": (lann, ("order", "cgoff", "cptr", "assign", "workspace", "cut_all", "best_assign",
                                          "best_cut", "best_idx"), large, "cands"),
    }


DECODERS = ("gmc_round_conditional_t_f32", "gmc_kway_decode_sample_seeded_t_f32", "gmc_kway_refine_anneal_t_f32",
            "gmc_large_round_conditional_t_f32", "gmc_large_local_search_t_f32", "gmc_large_sample_seeded_t_f32",
            "gmc_large_anneal_t_f32")


@pytest.mark.parametrize("name", DECODERS)
def test_decoder_entry_points_check_their_arguments_in_order(built, name):
    hip = built.hip
    call, pointers, bound, shape_arg = decoder_calls(hip.load())[name]
    null = C.c_void_p(None)
    batch = lambda **kw: _batch(hip, **kw)
    assert name in hip.SYMBOLS
    for t in (0, 1):
        # 1. NULL pointers, before the abi word
        assert call(None, 3, t) == -1
        for ptr in pointers:
            assert call(batch(abi=100), 3, t, **{ptr: null}) == -1, ptr
        # 2. the abi word, before the batch's pointers, the class count and the shapes
        assert call(batch(abi=100, lcol=None), 9, 2) == -8
        # 3. the batch's own pointers, before the class count
        for ptr in ("goff", "rowptr", "lcol"):
            assert call(batch(**{ptr: None}), 9, t) == -1, ptr
        # 4. the class count, before the shapes
        for K in (-3, 0, 1, 9):
            assert call(batch(), K, 2) == -3, K
        # 5. shapes - the flag among them - before the graph size
        assert call(batch(n_max=0), 3, t, **{shape_arg: -1}) == -2
        assert call(batch(n_max=0, B=-1), 3, t) == -2
        # 6. graph size: the upper bound with and without terminals
        assert call(batch(n_max=bound + 1), 3, t) == -6
        # an empty batch: nothing launched
        assert call(batch(B=0, R=0, n_max=0), 3, t) == 0
    for t in (-1, 2, 256):
        assert call(batch(n_max=0), 3, t) == -2, t                     # GMC_ERR_SHAPE, before the graph size
    # n_max = K - 1: refused with terminals, accepted without (the empty-batch return aside, nothing may launch here,
    # so the accepted call is told apart by the check that FOLLOWS the graph size: a workspace of 0 bytes, or B = 0)
    assert call(batch(n_max=7), 8, 1) == -6
    assert call(batch(n_max=0), 8, 0) == -6 and call(batch(n_max=0), 8, 1) == -6           # a graph needs one node
    if "workspace" in pointers:
        assert call(batch(n_max=7), 8, 0, bytes=0) == -5               # past the size check: GMC_ERR_WORKSPACE
        assert call(batch(n_max=7), 8, 1, bytes=0) == -6


def test_instance_entry_points_check_the_flag(built):
    hip = built.hip
    lib = hip.load()
    some = C.c_void_p(4096)
    model = lambda **kw: C.byref(hip.GmcModel(**{**dict(N=100, F=8, K=3, W1=4096, b1=4096, W2=4096, b2=4096), **kw}))
    fwd = lambda b, m, t, ws=some, nbytes=1 << 30: lib.gmc_inst_forward_t(b, m, t, 1.0, ws, nbytes, some, some, some, None)
    trn = lambda b, m, t, ws=some, nbytes=1 << 30: lib.gmc_inst_train_fwd_bwd_t(b, m, t, 1.0, ws, nbytes, some, some, some,
                                                                               some, None)
    assert {"gmc_inst_forward_t", "gmc_inst_train_fwd_bwd_t"} <= set(hip.SYMBOLS)
    for call in (fwd, trn):
        assert call(_batch(hip, abi=100), model(), 2) == -8                                    # the abi word first
        assert call(_batch(hip, lcol=None), model(K=9), 2) == -1                               # pointers, then
        assert call(_batch(hip), model(K=9), 2) == -3                                          # the class count, then
        for t in (-1, 2):
            assert call(_batch(hip, n_max=2), model(), t) == -2                                # the shapes: the flag
        assert call(_batch(hip, n_max=2), model(), 1) == -6                                    # n_max = K - 1
        assert call(_batch(hip, n_max=2), model(), 0, nbytes=0) == -5                          # accepted: on to the workspace
        assert call(_batch(hip, n_max=0), model(), 0) == -6
        assert call(_batch(hip, n_max=60), model(), 1, nbytes=0) == -5
        assert call(_batch(hip, n_max=60), model(N=99), 0) == -2                               # one W1 row per node


# ---- Python ---------------------------------------------------------------------------------------------------------------
def test_python_refusals_and_defaults(built):
    import inspect
    from gcn_max_cut_amd import engine, maxcut
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    for name in ("conditional_rounding", "sampling_optimization", "kway_local_search", "kway_annealing",
                 "assign_partitions_seeded_kway", "round_dataset", "search_dataset", "large_conditional_rounding",
                 "large_local_search", "large_sampling_optimization", "large_annealing", "round_large_dataset",
                 "search_large_dataset"):
        assert inspect.signature(getattr(TN, name)).parameters["terminals"].default is True, name
    assert inspect.signature(T.solve_dataset).parameters["terminals"].default is True
    assert inspect.signature(engine.InstanceEngine.__init__).parameters["terminals"].default is True
    assert inspect.signature(engine.FusedEngine.forward).parameters["terminals"].default is True
    assert inspect.signature(maxcut.solve).parameters["terminals"].default is False
    with pytest.raises(NotImplementedError, match="evolution"):
        TN.search_dataset(None, {}, generations=2, terminals=False)
    with pytest.raises(ValueError, match="at least 8 nodes"):
        engine.check_instance_sizes([12, 6], 8)
    engine.check_instance_sizes([12, 6, 3], 8, terminals=False)                 # the minimum is waived ...
    with pytest.raises(ValueError, match="beyond the one-workgroup head"):
        engine.check_instance_sizes([5000], 8, terminals=False)                 # ... the maximum is not
    # the host form of the draw: the first K nodes are drawn like any other
    P = PR.softmax_rows(12, 4, 3)
    fixed, plain = TN.assign_partitions_seeded_kway(P, 5, 3, 2), TN.assign_partitions_seeded_kway(P, 5, 3, 2, terminals=False)
    assert fixed[:4] == [0, 1, 2, 3] and fixed[4:] == plain[4:]
    key = int(SR.keys(5, [3])[0])
    assert plain == PR.assignments(P, key, 3, 0)[2].tolist()
    # the front door refuses what the per-graph models cannot hold, before it needs a GPU, and names the route
    ei = np.zeros((2, 0), np.int64)
    with pytest.raises(ValueError, match=r"functional.*search_large_dataset\(\.\.\., terminals=False\)"):
        maxcut.solve(ei, num_nodes=5000, hidden_dim=8, epochs=1, learning_rate=0.01, number_classes=8)
    with pytest.raises(ValueError, match="number_classes"):
        maxcut.solve(ei, num_nodes=10, hidden_dim=8, epochs=1, learning_rate=0.01, number_classes=9)


# ---- the cases of the GPU step test ---------------------------------------------------------------------------------------
def test_instance_cases_are_decided_and_within_float32_reach():
    """Sections 24 / 26 of DESIGN.md: a case is seeded so that identical partitions may be demanded (no row within
    MARGIN of an argmax tie - every row, none is overridden - and no unit within KINK of the relu kink) and so that a
    float32 evaluation in numpy stays within half of ROW_TOL."""
    done = {}
    for c in PR.INST_CASES:
        csrs = PR.inst_case_csrs(c)
        margin, gap, ratio = PR.inst_rules(csrs, PR.inst_case_params(c, csrs), PR.INST_C, c.loss)
        assert margin >= PR.MARGIN and gap >= PR.KINK and ratio <= 0.5, (PR.inst_case_id(c), margin, gap, ratio)
        done[(c.batch, c.K, c.weights)] = c.seed
    assert len(PR.INST_CASES) == 48
    assert any(len(rp) - 1 < c.K for c in PR.INST_CASES for rp, _cl, _w in PR.inst_case_csrs(c))   # a graph below K
