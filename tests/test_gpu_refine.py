"""GPU tests of the local search over decoded partitions (gmc_refine_local_f32 and its Python API) against the CPU
restatement in tests/refine_ref.py: refined assignments byte for byte, sweep counts, cuts (unit and integer
weights exact, fp32 weights 1e-5 relative), the pick; max_sweeps = 0 against the sampler; decode_dataset and
local_search_optimization on a trained model."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import refine_ref as RR
from tests.test_refine_host import STAMP_GRAPH, VICTIM_GRAPH, gnp_graph, handles_of, hub_graph, loop_graph

pytestmark = pytest.mark.gpu

GARBAGE = -5


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def run_refine(pkg, batch, A, max_sweeps):
    """gmc_refine_local_f32 on A [cands, R] int8 with every output pre-filled with garbage."""
    hip = pkg.hip
    cands = A.shape[0]
    order, cgoff, cptr = batch.refine_order()
    assign = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    sweeps = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_refine_local_f32(batch.ref(), p(order), p(cgoff), p(cptr), cands, p(assign), max_sweeps,
                                         p(cut_all), p(best_assign), p(best_cut), p(best_idx), p(sweeps), hip.stream())
    hip.check(rc, "gmc_refine_local_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut_all=cut_all, best_assign=best_assign,
                                                    best_cut=best_cut, best_idx=best_idx, sweeps=sweeps).items()}


def check_against_restatement(pkg, graphs, cands, max_sweeps, seed, rel=0.0):
    from gcn_max_cut_amd.graph import GraphBatch
    hs = handles_of(graphs)
    batch = GraphBatch(hs, None, torch.device("cuda"))
    rng = np.random.RandomState(seed)
    A = rng.randint(0, 3, (cands, batch.R)).astype(np.int8)
    got = run_refine(pkg, batch, A, max_sweeps)
    assert np.isfinite(got["cut_all"]).all() and np.isfinite(got["best_cut"]).all()
    for g, h in enumerate(hs):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        ref, ref_sweeps = RR.refine(h.n, h.rowptr, h.col, h.weight, A[:, lo:hi], max_sweeps)
        assert (got["assign"][:, lo:hi] == ref).all(), (g, h.n, int((got["assign"][:, lo:hi] != ref).sum()))
        assert (got["sweeps"][g] == ref_sweeps).all()
        assert (got["sweeps"][g] <= max_sweeps).all()
        ref_cuts = np.array([RR.cut(h.rowptr, h.col, h.weight, a) for a in ref])
        if rel == 0.0:
            assert (got["cut_all"][g] == ref_cuts).all()
        else:
            assert np.abs(got["cut_all"][g] - ref_cuts).max() <= rel * ref_cuts.max()
        bi = int(np.argmax(got["cut_all"][g]))                          # first of the largest
        assert got["best_idx"][g] == bi and got["best_cut"][g] == got["cut_all"][g, bi]
        assert (got["best_assign"][lo:hi] == got["assign"][bi, lo:hi]).all()
    if max_sweeps == 0:
        assert (got["assign"] == A).all()
    return got


COMBOS = [(1, 0), (1, 1), (1, 100), (201, 0), (201, 1), (201, 100), (1000, 0), (1000, 1), (1000, 100)]
REGULAR = [(n, d) for n in (6, 50, 300, 1000) for d in (3, 7, 12) if d < n and n * d % 2 == 0]


@pytest.mark.parametrize("n,d", REGULAR)
@pytest.mark.parametrize("cands,max_sweeps", COMBOS)
def test_regular_graphs_match_the_restatement(pkg, n, d, cands, max_sweeps):
    check_against_restatement(pkg, [R.regular_graph(n, d, 31 * n + d)], cands, max_sweeps, seed=n + d + cands)


def weighted(g, kind, seed):
    rng = np.random.RandomState(seed)
    for u, v in g.edges():
        g[u][v]["weight"] = int(rng.randint(1, 5)) if kind == "int" else float(np.float32(rng.uniform(0.1, 2.0)))
    return g


OTHER = {
    "mixed": lambda: [nx.complete_graph(3), R.regular_graph(50, 6, 7), nx.complete_graph(4), R.regular_graph(300, 7, 8),
                      R.regular_graph(1000, 7, 9), R.regular_graph(6, 3, 10)],
    "n4096": lambda: [R.regular_graph(4096, 7, 11)],
    "gnp": lambda: [gnp_graph(1000, 0.01, 12)],
    "hub100": lambda: [hub_graph(500, 7, 13)],
    "self_loops": lambda: [loop_graph(300, 6, 14)],
    "int_weights": lambda: [weighted(R.regular_graph(300, 7, 15), "int", 1), weighted(R.regular_graph(100, 5, 16), "int", 2)],
}


@pytest.mark.parametrize("case", sorted(OTHER))
@pytest.mark.parametrize("cands,max_sweeps", [(1, 0), (201, 100), (1000, 1)])
def test_other_graphs_match_the_restatement(pkg, case, cands, max_sweeps):
    check_against_restatement(pkg, OTHER[case](), cands, max_sweeps, seed=len(case) + cands)


def test_a_graph_refines_the_same_whatever_graphs_precede_it_in_the_batch(pkg):
    """Nodes 3, 5, 6 in class 0 (5 and 6 adjacent).  In first-fit order ({3} {4, 5} {6}) node 3 moves to class 2, then
    5 to class 1, and 6 stays; the order {3} {4, 6} {5} would move 6 instead.  The same result alone and after a graph
    whose colouring could leave its stamps behind."""
    from gcn_max_cut_amd.graph import GraphBatch
    start = np.array([0, 1, 2, 0, 1, 0, 0], np.int8)
    outs = []
    for graphs in ([VICTIM_GRAPH()], [STAMP_GRAPH(), VICTIM_GRAPH()]):
        batch = GraphBatch(handles_of(graphs), None, torch.device("cuda"))
        A = np.zeros((1, batch.R), np.int8)
        A[0, :3] = [0, 1, 2]
        A[0, batch.R - 7:] = start
        got = run_refine(pkg, batch, A, 1)
        outs.append(got["assign"][0, batch.R - 7:].tolist())
    h = handles_of([VICTIM_GRAPH()])[0]
    ref = RR.refine(h.n, h.rowptr, h.col, None, start.reshape(1, -1), 1)[0][0].tolist()
    other = RR.refine(h.n, h.rowptr, h.col, None, start.reshape(1, -1), 1,
                      classes=[np.array([3]), np.array([4, 6]), np.array([5])])[0][0].tolist()
    assert ref[3:] == [2, 1, 1, 0] and other[3:] == [2, 1, 0, 1]
    assert outs[0] == outs[1] == ref
    check_against_restatement(pkg, [STAMP_GRAPH(), VICTIM_GRAPH()] * 20, 201, 100, seed=5)


def test_a_terminal_named_by_order_is_not_visited(pkg):
    """Nodes 0..K-1 never move, whatever class they hold - also when `order` names one.  Two 3-regular graphs of 16 nodes
    (the second with real weights), two candidates whose terminals hold foreign classes (node 0 class 1, node 1 class 2,
    node 2 class 0, at K = 4 node 3 class 0), and an `order` whose first entry of every graph's first colour class is
    overwritten by that graph's row 0.  The first colour class is visited on the input state, where row 0's movable
    neighbours hold its class, so that - checked here on the host - row 0 has strictly less weight towards some class
    than towards the one it holds: a visit would move it.
    gmc_refine_local_f32 (100 sweeps), gmc_refine_anneal_f32 (10 annealing sweeps + 100) and gmc_kway_refine_anneal_f32
    at K = 3 and 4 leave the terminals' bytes alone, report the cut of what they return and pick from it.

    The cut of the unit-weight graph is exact.  On the weighted graph the kernel adds its m = 48 CSR weights (sum S) in
    fp32 in some order, every partial sum <= S, so it is within m * 2^-24 * S of the float64 sum, half of that after
    the division by 2."""
    from gcn_max_cut_amd.graph import GraphBatch
    from tests import anneal_ref as AR
    hip = pkg.hip
    lib, p = hip.load(), hip.ptr
    hs = handles_of([R.regular_graph(16, 3, 41), weighted(R.regular_graph(16, 3, 42), "float", 6)])
    batch = GraphBatch(hs, None, torch.device("cuda"))
    h = batch.host
    go32 = h.goff.astype(np.int32)
    host = lambda a: a.ctypes.data_as(C.c_void_p)

    def edited_order(K, refine_entry):
        order, cgoff, cptr = np.zeros(h.R, np.int32), np.zeros(h.B + 1, np.int32), np.zeros(h.R + h.B, np.int32)
        if refine_entry:
            rc = lib.gmc_refine_order_host(h.B, host(go32), host(h.rowptr), host(h.lcol), host(order), host(cgoff),
                                           host(cptr), cptr.size)
        else:
            rc = lib.gmc_round_order_host(h.B, host(go32), host(h.rowptr), host(h.lcol), K, host(order), host(cgoff),
                                          host(cptr), cptr.size)
        hip.check(rc, "order")
        for g in range(h.B):
            assert cptr[cgoff[g] + 1] > cptr[cgoff[g]]                  # the first colour class has an entry
            order[cptr[cgoff[g]]] = go32[g]                             # ... which now names the graph's row 0
        return [torch.from_numpy(a).cuda() for a in (order, cgoff, cptr)]

    def candidates(K):
        A = np.random.RandomState(50 + K).randint(0, K, (2, h.R)).astype(np.int8)
        for g, hd in enumerate(hs):
            nbrs = np.asarray(hd.col[hd.rowptr[0]:hd.rowptr[1]])
            A[:, go32[g] + nbrs[nbrs >= K]] = 1                         # row 0's movable neighbours share its class
            A[:, go32[g]:go32[g] + K] = [1, 2, 0, 0][:K]
        for g, hd in enumerate(hs):                                     # a visit would move row 0: the case is not vacuous
            for a in A[:, go32[g]:go32[g + 1]]:
                W = np.zeros(K)
                for e in range(hd.rowptr[0], hd.rowptr[1]):
                    W[a[hd.col[e]]] += 1.0 if hd.weight is None else hd.weight[e]
                assert W.min() < W[a[0]], (K, g)
        return A

    inv_t = torch.from_numpy(AR.schedule(10)).cuda()
    lv = torch.from_numpy(AR.levels()).cuda()

    def run(K, call):
        A = candidates(K)
        assign = torch.from_numpy(A).cuda()
        cut_all = torch.full((h.B, 2), float("nan"), device="cuda")
        best_assign = torch.full((h.R,), GARBAGE, dtype=torch.int32, device="cuda")
        best_cut = torch.full((h.B,), float("nan"), device="cuda")
        best_idx = torch.full((h.B,), GARBAGE, dtype=torch.int32, device="cuda")
        hip.check(call(p(assign), (p(cut_all), p(best_assign), p(best_cut), p(best_idx))), f"K = {K}")
        torch.cuda.synchronize()
        out, cuts, ba, bi = (t.cpu().numpy() for t in (assign, cut_all, best_assign, best_idx))
        for g, hd in enumerate(hs):
            lo, hi = int(go32[g]), int(go32[g + 1])
            assert (out[:, lo:lo + K] == A[:, lo:lo + K]).all(), (K, g, out[:, lo:lo + K].tolist())
            assert ((out[:, lo:hi] >= 0) & (out[:, lo:hi] < K)).all()
            ref = np.array([RR.cut(hd.rowptr, hd.col, hd.weight, a) for a in out[:, lo:hi]])
            if hd.weight is None:
                assert (cuts[g] == ref).all(), (K, g)
            else:
                w = np.asarray(hd.weight, np.float64)
                assert np.abs(cuts[g] - ref).max() <= w.size * 2.0 ** -24 * w.sum() / 2, (K, g)
            assert bi[g] == int(np.argmax(cuts[g])) and (ba[lo:hi] == out[bi[g], lo:hi]).all()

    o3 = edited_order(3, True)
    run(3, lambda a, outs: lib.gmc_refine_local_f32(batch.ref(), p(o3[0]), p(o3[1]), p(o3[2]), 2, a, 100, *outs, None,
                                                    hip.stream()))
    run(3, lambda a, outs: lib.gmc_refine_anneal_f32(batch.ref(), p(o3[0]), p(o3[1]), p(o3[2]), 2, a, p(inv_t), 10,
                                                     p(lv), 1, 100, *outs, None, None, hip.stream()))
    for K in (3, 4):
        ok = edited_order(K, False)
        run(K, lambda a, outs: lib.gmc_kway_refine_anneal_f32(batch.ref(), K, p(ok[0]), p(ok[1]), p(ok[2]), 2, a,
                                                              p(inv_t), 10, p(lv), 1, 100, *outs, None, None,
                                                              hip.stream()))


@pytest.mark.parametrize("cands,max_sweeps", [(1, 100), (201, 100), (201, 1)])
def test_fp32_weights_match_the_restatement(pkg, cands, max_sweeps):
    graphs = [weighted(R.regular_graph(300, 7, 17), "float", 3), weighted(loop_graph(120, 5, 18), "float", 4)]
    check_against_restatement(pkg, graphs, cands, max_sweeps, seed=cands, rel=1e-5)


def test_zero_sweeps_score_exactly_as_the_sampler(pkg):
    """max_sweeps = 0: cuts, best cut and best index are what gmc_decode_sample_f32 reports for the same samples."""
    from gcn_max_cut_amd.graph import GraphBatch
    hip = pkg.hip
    graphs = [R.regular_graph(200, 7, 21), weighted(R.regular_graph(100, 6, 22), "float", 5), nx.complete_graph(3)]
    batch = GraphBatch(handles_of(graphs), None, torch.device("cuda"))
    iters = 201
    rng = np.random.RandomState(23)
    P = torch.from_numpy(rng.dirichlet([1, 1, 1], batch.R).astype(np.float32)).cuda()
    draws = [rng.rand(iters, int(n) - 3) for n in batch.sizes]
    uoff = np.zeros(batch.B + 1, np.int64)
    np.cumsum([d.size for d in draws], out=uoff[1:])
    u = torch.from_numpy(np.concatenate([d.ravel() for d in draws])).cuda()
    uo = torch.from_numpy(uoff).cuda()
    assign_all = torch.empty((iters, batch.R), dtype=torch.int8, device="cuda")
    cut_all = torch.empty((batch.B, iters), device="cuda")
    best_assign = torch.empty(batch.R, dtype=torch.int32, device="cuda")
    best_cut = torch.empty(batch.B, device="cuda")
    best_iter = torch.empty(batch.B, dtype=torch.int32, device="cuda")
    p = hip.ptr
    hip.check(hip.load().gmc_decode_sample_f32(batch.ref(), p(P), p(u), p(uo), iters, p(assign_all), p(cut_all),
                                               p(best_assign), p(best_cut), p(best_iter), hip.stream()), "decode")
    torch.cuda.synchronize()
    samples = assign_all.cpu().numpy()
    got = run_refine(pkg, batch, samples, 0)
    assert (got["assign"] == samples).all()
    assert (got["cut_all"] == cut_all.cpu().numpy()).all()
    assert (got["best_cut"] == best_cut.cpu().numpy()).all() and (got["best_idx"] == best_iter.cpu().numpy()).all()
    assert (got["best_assign"] == best_assign.cpu().numpy()).all()
    assert (got["sweeps"] == 0).all()


@pytest.fixture(scope="module")
def trained(pkg):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    from tests import util
    specs = [(50, 6, 50001), (100, 7, 100001), (200, 8, 200001), (300, 6, 300001), (500, 7, 500001)]
    ds = util.product_dataset(specs)
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=64)
    torch.manual_seed(0)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    for _ in range(5):
        T.train_single_epoch(ds, net, opt, embed, cfg, graphs_per_step=len(ds))
    net.eval()
    return net, ds


OLD_KEYS = {'nodes', 'simple_cut', 'simple_assignment', 'post_cut', 'post_assignment', 'improvement'}


def test_decode_dataset_default_is_unchanged_and_refines_on_request(pkg, trained):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = trained
    np.random.seed(7)
    results, _ = TN.test_multiple_graphs(net, ds, [50, 100, 200, 300, 500], post_processing_iterations=200, verbose=False)
    np.random.seed(7)
    plain = TN.decode_dataset(net, ds, 200)
    assert len(plain) == len(results) == len(ds)
    for f, r in zip(plain, results):
        assert set(f) == OLD_KEYS
        assert (f["simple_cut"], f["simple_assignment"], f["post_cut"], f["post_assignment"], f["improvement"]) == \
            (r["simple_cut"], r["simple_assignment"], r["post_cut"], r["post_assignment"], r["improvement"])
        assert f["nodes"] == r["nodes"]
    np.random.seed(7)
    refined = TN.decode_dataset(net, ds, 200, local_search_sweeps=100)
    for f, rf, (_g, _a, nx_g, _t) in zip(plain, refined, ds.values()):
        assert set(rf) == OLD_KEYS | {'refined_cut', 'refined_assignment', 'refined_from'}
        assert {k: rf[k] for k in OLD_KEYS} == f
        assert rf["refined_cut"] >= max(f["simple_cut"], f["post_cut"])
        assert rf["refined_cut"] == TN.calculate_cut_value(rf["refined_assignment"], nx_g)
        assert rf["refined_assignment"][:3] == [0, 1, 2]
        assert 0 <= rf["refined_from"] <= 200
    assert sum(rf["refined_cut"] > f["post_cut"] for f, rf in zip(plain, refined)) >= 4


def test_local_search_optimization_on_the_argmax_decode(pkg, trained):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = trained
    for g, a_pad, nx_g, _t in ds.values():
        with torch.no_grad():
            P = net(g, a_pad)
        simple = TN.simple_partition_assignment(P)
        got, cut = TN.local_search_optimization(simple, nx_g, max_sweeps=100)
        h = handles_of([nx_g])[0]
        ref, sweeps = RR.refine(h.n, h.rowptr, h.col, h.weight, np.asarray([simple], np.int8), 100)
        assert got == ref[0].tolist() and int(sweeps[0]) < 100
        assert cut == TN.calculate_cut_value(got, nx_g) >= TN.calculate_cut_value(simple, nx_g)
        assert got[:3] == [0, 1, 2]
        same, cut0 = TN.local_search_optimization(simple, nx_g, max_sweeps=0)
        assert same == simple and cut0 == TN.calculate_cut_value(simple, nx_g)
    with pytest.raises(ValueError):
        TN.local_search_optimization(simple[:-1], nx_g)
    with pytest.raises(ValueError):
        TN.local_search_optimization(simple[:-1] + [3], nx_g)
