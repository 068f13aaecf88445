"""GPU tests of the rounding and the K-class local search for graphs beyond 4096 nodes (gmc_large_round_conditional_f32,
gmc_large_local_search_f32 and their Python API): byte for byte against the one-workgroup kernels
(gmc_round_conditional_f32, gmc_kway_refine_anneal_f32 without annealing) on every shape both run, byte for byte
against the restatement of tests/large_round_ref.py beyond 4096 nodes, and on every case the properties the header
states.  Outputs and the workspace are pre-filled with garbage, the terminals' rows of P are NaN.

Bars.  cut: exact for unit weights (every partial is an integer below 2^24), 1e-5 relative for real weights (the bar of
tests/test_gpu_rounding.py: a row adds at most deg terms, a tile 8 more levels, a graph its tiles - each rounding 2^-24
of a partial no larger than W_abs; 4096 tiles of a million-node graph run on unit weights only).  expected: 5e-5 W_abs
of float64 (test_rounding_host.SLACK).  A converged descent leaves no improving move: exactly none for unit weights;
for real weights the device compares fp32 row sums, each off its exact value by at most deg * 2^-24 of the row's
absolute weight, so a float64 gain of up to GAIN_EPS = 2 * deg_max * 2^-24 * (largest absolute row weight) may remain."""
import ctypes as C
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import kway_search_ref as KS
from tests import large_round_ref as LRR
from tests import rounding_ref as CR
from tests.test_gpu_kway_search import run_kanneal
from tests.test_gpu_rounding import RawBatch, hub40_graph, run_round, small_model
from tests.test_refine_host import handles_of, loop_graph
from tests.test_rounding_host import SLACK

pytestmark = pytest.mark.gpu

GARBAGE = -5
KS_ = (2, 3, 4, 8)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


class LargeBatch(RawBatch):
    """RawBatch with what the multi-workgroup kernels read on top: gcol (batch row ids) and the order arrays of
    gmc_large_round_order_host with max_classes."""

    def __init__(self, pkg, handles):
        super().__init__(pkg, handles)
        nnz = np.asarray([h.col.size for h in handles], np.int64)
        self.gcol_host = (self.lcol_host.astype(np.int64) + np.repeat(self.goff_host[:-1], nnz)).astype(np.int32)
        self.gcol = torch.from_numpy(self.gcol_host).cuda()
        self.c.gcol = pkg.hip.ptr(self.gcol)
        self._large_orders = {}

    def large_order(self, K):
        if K not in self._large_orders:
            order = np.zeros(max(self.R, 1), np.int32)
            cgoff = np.zeros(self.B + 1, np.int32)
            cptr = np.zeros(self.R + self.B, np.int32)
            most = C.c_int32(-1)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            go = self.goff_host.astype(np.int32)
            rc = self._lib.gmc_large_round_order_host(self.B, p(go), p(self.rowptr_host), p(self.lcol_host), K, p(order),
                                                      p(cgoff), p(cptr), cptr.size, C.byref(most))
            assert rc == 0, rc
            self._large_orders[K] = tuple(torch.from_numpy(a).cuda() for a in (order, cgoff, cptr)) + (most.value,)
        return self._large_orders[K]


def workspace(pkg, batch, K):
    need = pkg.hip.load().gmc_large_round_workspace_bytes(batch.ref(), K)
    assert need > 0
    return torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")   # garbage: the calls write what they read


def run_large_round(pkg, batch, P, K, descent, want_expected=True, want_sweeps=True):
    """gmc_large_round_conditional_f32 with every output and the workspace pre-filled with garbage."""
    hip = pkg.hip
    order, cgoff, cptr, most = batch.large_order(K)
    Pd = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    ws = workspace(pkg, batch, K)
    assign = torch.full((batch.R,), GARBAGE, dtype=torch.int8, device="cuda")
    cut = torch.full((batch.B,), float("nan"), device="cuda")
    expected = torch.full((batch.B,), float("nan"), device="cuda")
    sweeps = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_large_round_conditional_f32(batch.ref(), p(Pd), K, p(order), p(cgoff), p(cptr), most, descent,
                                                    p(ws), ws.numel(), p(assign), p(cut),
                                                    p(expected) if want_expected else None,
                                                    p(sweeps) if want_sweeps else None, hip.stream())
    hip.check(rc, "gmc_large_round_conditional_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut=cut, expected=expected, sweeps=sweeps).items()}


def run_large_search(pkg, batch, A, K, max_sweeps, want_sweeps=True):
    """gmc_large_local_search_f32 on A [R] int8 with the outputs and the workspace pre-filled with garbage."""
    hip = pkg.hip
    order, cgoff, cptr, most = batch.large_order(K)
    ws = workspace(pkg, batch, K)
    assign = torch.from_numpy(np.ascontiguousarray(A, np.int8)).cuda()
    cut = torch.full((batch.B,), float("nan"), device="cuda")
    sweeps = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_large_local_search_f32(batch.ref(), K, p(order), p(cgoff), p(cptr), most, max_sweeps, p(ws),
                                               ws.numel(), p(assign), p(cut), p(sweeps) if want_sweeps else None,
                                               hip.stream())
    hip.check(rc, "gmc_large_local_search_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut=cut, sweeps=sweeps).items()}


def gain_eps(h):
    """GAIN_EPS of the module text for one graph (0 for unit weights)."""
    if h.weight is None:
        return 0.0
    rowptr = np.asarray(h.rowptr, np.int64)
    row_abs = np.add.reduceat(np.abs(h.weight.astype(np.float64)), rowptr[:-1])
    return 2.0 * float(np.diff(rowptr).max()) * 2.0 ** -24 * float(row_abs.max())


def check_properties(h, K, P, r0, r1, max_sweeps, signed):
    """What the header states of one graph's outputs: r0 at descent 0, r1 after up to max_sweeps sweeps (dicts of this
    graph's assign, cut, expected, sweeps)."""
    W_abs = CR.abs_weight(h.rowptr, h.col, h.weight)
    exp64 = CR.expected_cut(h.n, h.rowptr, h.col, h.weight, P, K)
    cuts = []
    for r in (r0, r1):
        a = r["assign"]
        assert (a[:K] == np.arange(K)).all() and a.min() >= 0 and a.max() < K          # terminals keep their classes
        c64 = CR.cut(h.rowptr, h.col, h.weight, a)
        cuts.append(c64)
        print(f"n {h.n} K {K}: cut {r['cut']} (float64 recount {c64}), expected {r['expected']} (float64 {exp64}), "
              f"W_abs {W_abs}, sweeps {r['sweeps']}")
        if signed:
            assert abs(float(r["cut"]) - c64) <= 1e-5 * abs(c64)
        else:
            assert float(r["cut"]) == c64
        assert abs(float(r["expected"]) - exp64) <= SLACK * W_abs
    assert r0["sweeps"] == 0 and (max_sweeps == 0 or 1 <= r1["sweeps"] <= max_sweeps)
    assert cuts[0] >= exp64 - SLACK * W_abs                                            # the guarantee
    assert cuts[1] >= cuts[0]                                                          # a descent loses nothing
    if r1["sweeps"] < max_sweeps:                                                      # converged: a local optimum
        gain = (KS.best_single_move_gain(h.n, h.rowptr, h.col, h.weight, r1["assign"].tolist(), K) if h.n <= 5000
                else LRR.best_single_move_gain(h.n, h.rowptr, h.col, h.weight, r1["assign"], K))
        assert gain <= gain_eps(h), gain


def of_graph(out, batch, g):
    lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
    return dict(assign=out["assign"][lo:hi], cut=out["cut"][g], expected=out["expected"][g], sweeps=out["sweeps"][g])


# ---- against the one-workgroup kernels ----------------------------------------------------------------------------------
def shapes(K):
    """name -> graphs of one batch, for K classes (the first graph of "batch" has 5 nodes, or K where 5 < K: every
    graph needs its K terminals)."""
    return {
        "n_K": [nx.complete_graph(K)],
        "n_K1": [nx.complete_graph(K + 1)],
        "n255": [R.regular_graph(255, 4, 255 + K)],
        "n256": [R.regular_graph(256, 5, 256 + K)],
        "n257": [R.regular_graph(257, 4, 257 + K)],
        "path1030": [nx.path_graph(1030)],
        "batch_5_700_257": [nx.complete_graph(max(5, K)), R.regular_graph(700, 7, 700 + K),
                            CR.connected_gnp(257, 0.03, 257 + K)],
        "hub40": [hub40_graph(300, 40 + K)],
        "self_loops": [loop_graph(120, 5, 18 + K)],
        "gnp200": [CR.connected_gnp(200, 0.05, 200 + K)],
    }


SHAPES = [(K, name) for K in KS_ for name in sorted(shapes(2))] + [(3, "n4096"), (8, "n4096")]


@functools.lru_cache(maxsize=None)
def small_case(K, name, signed):
    """handles and P (terminal rows NaN; Pfull: every row drawn) of a shape the one-workgroup kernels run too."""
    graphs = [R.regular_graph(4096, 3, 4096)] if name == "n4096" else shapes(K)[name]
    if signed:
        graphs = [CR.signed_weights(g, 7 * i + K) for i, g in enumerate(graphs)]
    hs = handles_of(graphs)
    seed = 41 * K + len(name) + (1 if signed else 0)
    Ps = [CR.softmax_rows(h.n, K, seed + i, scale=2.0) for i, h in enumerate(hs)]
    for h, P in zip(hs, Ps):
        LRR.check_inputs(K, h.n, h.rowptr, h.col, h.weight, P)
    poisoned = [P.copy() for P in Ps]
    for P in poisoned:
        P[:K] = np.nan                                                 # the terminals' rows are never read
    return hs, np.concatenate(poisoned), Ps


@pytest.mark.parametrize("signed", (False, True), ids=("unit", "signed"))
@pytest.mark.parametrize("K,name", SHAPES)
def test_rounding_is_the_one_workgroup_kernels(pkg, K, name, signed):
    hs, P, Ps = small_case(K, name, signed)
    batch = LargeBatch(pkg, hs)
    got = {}
    for descent in (0, 100):
        want = run_round(pkg, batch, P, K, descent)
        got[descent] = new = run_large_round(pkg, batch, P, K, descent)
        assert new["assign"].tobytes() == want["assign"].tobytes(), int((new["assign"] != want["assign"]).sum())
        assert new["sweeps"].tobytes() == want["sweeps"].tobytes(), (new["sweeps"], want["sweeps"])
        if signed:
            assert (np.abs(new["cut"] - want["cut"]) <= 1e-5 * np.abs(want["cut"])).all(), (new["cut"], want["cut"])
        else:
            assert new["cut"].tobytes() == want["cut"].tobytes()
        again = run_large_round(pkg, batch, P, K, descent)             # two runs are byte-equal
        for k in new:
            assert new[k].tobytes() == again[k].tobytes(), k
        # NULL expected / sweeps leave the other outputs unchanged
        bare = run_large_round(pkg, batch, P, K, descent, want_expected=False, want_sweeps=False)
        assert bare["assign"].tobytes() == new["assign"].tobytes() and bare["cut"].tobytes() == new["cut"].tobytes()
        assert np.isnan(bare["expected"]).all() and (bare["sweeps"] == GARBAGE).all()
    one = run_large_round(pkg, batch, P, K, 1)                         # one sweep and no more
    assert (one["sweeps"] == 1).all()
    assert one["assign"].tobytes() == run_round(pkg, batch, P, K, 1)["assign"].tobytes()
    for g, h in enumerate(hs):
        check_properties(h, K, Ps[g], of_graph(got[0], batch, g), of_graph(got[100], batch, g), 100, signed)


@pytest.mark.parametrize("signed", (False, True), ids=("unit", "signed"))
@pytest.mark.parametrize("K,name", SHAPES)
def test_local_search_is_the_one_workgroup_kernels(pkg, K, name, signed):
    hs, _P, _Ps = small_case(K, name, signed)
    batch = LargeBatch(pkg, hs)
    A = np.random.RandomState(13 * K + len(name)).randint(0, K, batch.R).astype(np.int8)
    lo, hi = int(batch.goff_host[-2]), int(batch.goff_host[-1])
    if hi - lo > K:
        A[hi - 1] = K                                                  # a byte of no class on a movable node
    if hi - lo > K + 2:
        A[lo + K + 1] = -1
    for max_sweeps in (100, 1, 0):
        want = run_kanneal(pkg, batch, K, A[None, :].copy(), [], 0, max_sweeps)
        new = run_large_search(pkg, batch, A, K, max_sweeps)
        assert new["assign"].tobytes() == want["assign"][0].tobytes(), max_sweeps
        assert new["sweeps"].tobytes() == want["sweeps"][:, 0].tobytes(), max_sweeps
        if signed:
            assert (np.abs(new["cut"] - want["cut_all"][:, 0]) <= 1e-5 * np.abs(want["cut_all"][:, 0])).all()
        else:
            assert new["cut"].tobytes() == want["cut_all"][:, 0].tobytes()
        again = run_large_search(pkg, batch, A, K, max_sweeps, want_sweeps=False)
        assert again["assign"].tobytes() == new["assign"].tobytes() and again["cut"].tobytes() == new["cut"].tobytes()
        assert (again["sweeps"] == GARBAGE).all()
        if max_sweeps == 100:
            for g, h in enumerate(hs):
                if new["sweeps"][g] < 100:
                    a = new["assign"][int(batch.goff_host[g]):int(batch.goff_host[g + 1])]
                    assert KS.best_single_move_gain(h.n, h.rowptr, h.col, h.weight, a.tolist(), K) <= gain_eps(h)


# ---- beyond 4096 nodes: against the restatement -------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def big_reference(name):
    """The case, its handle, its colour tables and its restatement, computed once and shared."""
    from gcn_max_cut_amd.graph import GraphHandle
    K, n, rowptr, col, w, P, max_sweeps = LRR.big_case(name)
    tables = LRR.class_tables(n, rowptr, col, w, LRR.colouring(n, rowptr, col, K))
    a0 = LRR.round_by_classes(n, P, K, tables)
    a1, sweeps = LRR.descent(n, a0, K, tables, max_sweeps)
    for a in (a0, a1):
        a.setflags(write=False)
    poisoned = P.copy()
    poisoned[:K] = np.nan
    return GraphHandle(n, rowptr, col, w), tables, dict(a0=a0, a1=a1, sweeps=sweeps), poisoned


@pytest.mark.parametrize("name", sorted(LRR.BIG_CASES))
def test_beyond_4096_nodes_against_the_restatement(pkg, name):
    K, n, _rp, _col, w, P, max_sweeps = LRR.big_case(name)
    h, tables, ref, poisoned = big_reference(name)
    batch = LargeBatch(pkg, [h])
    r0 = run_large_round(pkg, batch, poisoned, K, 0)
    r1 = run_large_round(pkg, batch, poisoned, K, max_sweeps)
    assert r0["assign"].tobytes() == ref["a0"].tobytes(), int((r0["assign"] != ref["a0"]).sum())
    assert r1["assign"].tobytes() == ref["a1"].tobytes(), int((r1["assign"] != ref["a1"]).sum())
    assert r0["sweeps"][0] == 0 and r1["sweeps"][0] == ref["sweeps"]
    again = run_large_round(pkg, batch, poisoned, K, max_sweeps)
    for k in r1:
        assert r1[k].tobytes() == again[k].tobytes(), k
    check_properties(h, K, P, of_graph(r0, batch, 0), of_graph(r1, batch, 0), max_sweeps, w is not None)
    one = run_large_round(pkg, batch, poisoned, K, 1, want_expected=False)
    assert one["sweeps"][0] == 1 and np.isnan(one["expected"]).all()
    # the local search from a random assignment with two bytes of no class
    A = np.random.RandomState(len(name)).randint(0, K, n).astype(np.int8)
    A[n - 1], A[K + 1] = K, -1
    want, want_sweeps = LRR.descent(n, A, K, tables, max_sweeps)
    new = run_large_search(pkg, batch, A, K, max_sweeps)
    assert new["assign"].tobytes() == want.tobytes() and new["sweeps"][0] == want_sweeps
    c64 = CR.cut(h.rowptr, h.col, h.weight, new["assign"])
    assert float(new["cut"][0]) == c64 if w is None else abs(float(new["cut"][0]) - c64) <= 1e-5 * abs(c64)


def test_a_large_graph_rounds_the_same_alone_and_inside_a_batch(pkg):
    from gcn_max_cut_amd.graph import GraphHandle
    from tests import large_ref as LR
    K = 3
    specs = [LR.circulant(4097, 7, 6), LR.circulant(5, 3, None), LR.circulant(257, 6, None)]
    hs = [GraphHandle(n, rp, col, LRR.signed_edge_weights(n, rp, col, i)) for i, (n, rp, col) in enumerate(specs)]
    P = np.concatenate([LRR.softmax_rows(h.n, K, 90 + i, scale=2.0) for i, h in enumerate(hs)])
    batch = LargeBatch(pkg, hs)
    A = np.random.RandomState(4).randint(0, K, batch.R).astype(np.int8)
    for descent in (0, 100):
        together = run_large_round(pkg, batch, P, K, descent)
        searched = run_large_search(pkg, batch, A, K, descent)
        for g, h in enumerate(hs):
            lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
            single = LargeBatch(pkg, [h])
            alone = run_large_round(pkg, single, P[lo:hi], K, descent)
            assert alone["assign"].tobytes() == together["assign"][lo:hi].tobytes()
            for k in ("cut", "expected", "sweeps"):
                assert alone[k].tobytes() == together[k][g:g + 1].tobytes(), (k, g)
            alone = run_large_search(pkg, single, A[lo:hi], K, descent)
            assert alone["assign"].tobytes() == searched["assign"][lo:hi].tobytes()
            for k in ("cut", "sweeps"):
                assert alone[k].tobytes() == searched[k][g:g + 1].tobytes(), (k, g)


# ---- the Python API -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (3, 4))
def test_round_large_dataset_equals_round_dataset_on_small_graphs(pkg, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = small_model(pkg, K, [(60, 5, 61), (48, 6, 62), (100, 7, 63)], 128, 16, seed=K)
    for descent in (0, 100):
        want = TN.round_dataset(net, ds, descent_sweeps=descent)
        got = TN.round_large_dataset(net, ds, descent_sweeps=descent)
        assert len(got) == len(want) == len(ds)
        for a, b, (_handle, _a_pad, nx_g, _t) in zip(got, want, ds.values()):
            assert set(a) == set(b)
            for key in ("nodes", "rounded_assignment", "descent_sweeps", "simple_assignment", "simple_cut", "rounded_cut"):
                assert a[key] == b[key], key
            assert abs(a["expected_cut"] - b["expected_cut"]) <= SLACK * nx_g.number_of_edges()   # (another summation order)


@pytest.mark.parametrize("K", (3, 4))
def test_round_large_dataset_on_a_dataset_without_the_dense_adjacency(pkg, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    from tests.test_gpu_large_graphs import dataset_of
    N = 4200
    ds = dataset_of(pkg, [4200, 300], K, N, seed=60 + K)
    assert all(it[1] is None for it in ds.values())
    torch.manual_seed(K)
    net, _embed, _opt = T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=N, hidden_dim=8, number_classes=K))
    with pytest.raises(ValueError, match="4096 nodes.*argmax partition"):
        TN.round_dataset(net, ds)                                      # the one-workgroup decoder still refuses
    for descent in (0, 20):
        results = TN.round_large_dataset(net, ds, descent_sweeps=descent)
        for res, (handle, _none, nx_g, _t) in zip(results, ds.values()):
            assert res["nodes"] == handle.n == len(res["rounded_assignment"])
            assert res["rounded_assignment"][:K] == list(range(K))
            assert res["rounded_cut"] == TN.calculate_cut_value(res["rounded_assignment"], nx_g)
            assert res["simple_cut"] == TN.calculate_cut_value(res["simple_assignment"], nx_g)
            assert res["rounded_cut"] >= res["expected_cut"] - SLACK * nx_g.number_of_edges()
            assert res["descent_sweeps"] == 0 if descent == 0 else 1 <= res["descent_sweeps"] <= 20


def test_python_functions_on_a_5000_node_graph_equal_the_restatement(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    K, n, _rp, _col, w, P, max_sweeps = LRR.big_case("n5000_K3")
    h, tables, ref, _poisoned = big_reference("n5000_K3")
    a0, c0 = TN.large_conditional_rounding(P, h)
    a1, c1 = TN.large_conditional_rounding(torch.from_numpy(P), h, descent_sweeps=max_sweeps)
    assert a0 == ref["a0"].tolist() and a1 == ref["a1"].tolist()
    for a, c in ((a0, c0), (a1, c1)):
        c64 = CR.cut(h.rowptr, h.col, h.weight, a)
        assert abs(c - c64) <= 1e-5 * abs(c64)
    A = np.random.RandomState(9).randint(0, K, n)
    want, _sweeps = LRR.descent(n, A.astype(np.int8), K, tables, 100)
    got, cut = TN.large_local_search(A.tolist(), h, K, max_sweeps=100)
    assert got == want.tolist()
    c64 = CR.cut(h.rowptr, h.col, h.weight, got)
    assert abs(cut - c64) <= 1e-5 * abs(c64)
