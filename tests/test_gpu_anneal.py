"""GPU tests of the annealing over decoded partitions (gmc_refine_anneal_f32 and its Python API) against the CPU
restatement in tests/anneal_ref.py: assignments byte for byte, cuts, the pick, snapshot sweeps and descent sweeps
(unit, integer and dyadic weights: every fp32 sum is exact in any order); real-valued weights by invariants;
anneal_sweeps = 0 against gmc_refine_local_f32; seeds, batch position, the probe tag, the Python API on a trained
model and the cut quality on the device."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import refine_ref as RR
from tests import util
from tests.test_gpu_refine import run_refine
from tests.test_refine_host import gnp_graph, handles_of, hub_graph, loop_graph

pytestmark = pytest.mark.gpu

GARBAGE = -5


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def run_anneal(pkg, batch, A, inv_temp, seed, max_descent, table=None):
    """gmc_refine_anneal_f32 on A [cands, R] int8 with every output pre-filled with garbage."""
    hip = pkg.hip
    cands = A.shape[0]
    order, cgoff, cptr = batch.refine_order()
    assign = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    inv_t = torch.from_numpy(np.asarray(inv_temp, np.float32)).cuda() if len(inv_temp) else None
    lv = torch.from_numpy(AR.levels() if table is None else table).cuda() if len(inv_temp) else None
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    snap = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    sweeps = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_refine_anneal_f32(batch.ref(), p(order), p(cgoff), p(cptr), cands, p(assign), p(inv_t),
                                          len(inv_temp), p(lv), seed, max_descent, p(cut_all), p(best_assign),
                                          p(best_cut), p(best_idx), p(snap), p(sweeps), hip.stream())
    hip.check(rc, "gmc_refine_anneal_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut_all=cut_all, best_assign=best_assign,
                                                    best_cut=best_cut, best_idx=best_idx, snap=snap,
                                                    sweeps=sweeps).items()}


def staged(pkg, batch):
    return pkg.hip.load().gmc_refine_anneal_staged(batch.ref())


def batch_of(graphs):
    from gcn_max_cut_amd.graph import GraphBatch
    hs = handles_of(graphs)
    return hs, GraphBatch(hs, None, torch.device("cuda"))


def check_pick(got, batch):
    for g in range(batch.B):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        bi = int(np.argmax(got["cut_all"][g]))                          # first of the largest
        assert got["best_idx"][g] == bi and got["best_cut"][g] == got["cut_all"][g, bi]
        assert (got["best_assign"][lo:hi] == got["assign"][bi, lo:hi]).all()


def check_against_restatement(pkg, graphs, cands, sweeps, seed, max_descent=100, expect_staged=None, no_class=()):
    """no_class: (candidate, batch row, byte) triples - class bytes outside 0..2 put on movable nodes."""
    hs, batch = batch_of(graphs)
    if expect_staged is not None:
        assert staged(pkg, batch) == expect_staged
    rng = np.random.RandomState(seed)
    A = rng.randint(0, 3, (cands, batch.R)).astype(np.int8)
    for cand, row, byte in no_class:
        A[cand, row] = byte
    scale = 1.0 if batch.host.vals is None else float(batch.host.vals.mean())
    inv_t = AR.schedule(sweeps, scale=scale)
    got = run_anneal(pkg, batch, A, inv_t, seed, max_descent)
    assert np.isfinite(got["cut_all"]).all() and np.isfinite(got["best_cut"]).all()
    for g, h in enumerate(hs):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        ref, ref_snap, ref_sweeps = AR.anneal(h.n, h.rowptr, h.col, h.weight, A[:, lo:hi], inv_t, AR.levels(), seed,
                                              max_descent)
        assert (got["snap"][g] == ref_snap).all(), (g, h.n)
        assert (got["assign"][:, lo:hi] == ref).all(), (g, h.n, int((got["assign"][:, lo:hi] != ref).sum()))
        assert (got["sweeps"][g] == ref_sweeps).all()
        assert (got["cut_all"][g] == AR.cuts_f32(h.rowptr, h.col, h.weight, ref)).all()
        if not no_class:                                                # (every edge of a byte of no class counts as cut)
            assert (got["cut_all"][g] >= AR.cuts_f32(h.rowptr, h.col, h.weight, A[:, lo:hi])).all()
    check_pick(got, batch)
    return got


# n x d with the candidate count and the sweeps of each case; the copy of an n = 4096 graph does not fit the LDS budget
REGULAR = [(n, d, {3: 1, 7: 201, 12: 7}[d], 100 if (n, d) in ((500, 7), (1000, 7)) else 30)
           for n in (3, 4, 50, 500, 1000, 4096) for d in (3, 7, 12)]


@pytest.mark.parametrize("n,d,cands,sweeps", REGULAR)
def test_near_regular_graphs_match_the_restatement(pkg, n, d, cands, sweeps):
    check_against_restatement(pkg, [util.near_regular(n, d, 31 * n + d, attrs=False)], cands, sweeps, seed=n + d,
                              expect_staged=int(n < 4096))


def weighted(g, kind, seed):
    rng = np.random.RandomState(seed)
    for u, v in g.edges():
        g[u][v]["weight"] = {"int": lambda: int(rng.randint(1, 4)), "dyadic": lambda: int(rng.randint(1, 33)) / 8.0,
                             "real": lambda: float(np.float32(rng.uniform(0.1, 2.0)))}[kind]()
    return g


OTHER = {   # graphs, whether their copy fits the LDS budget
    "mixed": (lambda: [nx.complete_graph(3), R.regular_graph(50, 6, 7), nx.complete_graph(4), R.regular_graph(300, 7, 8),
                       R.regular_graph(1000, 7, 9), R.regular_graph(6, 3, 10)], 1),
    "mixed_with_4096": (lambda: [R.regular_graph(100, 5, 1), R.regular_graph(4096, 7, 2), nx.complete_graph(4),
                                 R.regular_graph(500, 12, 3), nx.complete_graph(3)], 0),
    "gnp_dense_staged": (lambda: [gnp_graph(150, 0.3, 12)], 1),
    "gnp_dense_global": (lambda: [gnp_graph(300, 0.25, 13)], 0),
    "hub100": (lambda: [hub_graph(500, 7, 13)], 1),
    "self_loops": (lambda: [loop_graph(300, 6, 14)], 1),
    "int_weights": (lambda: [weighted(R.regular_graph(300, 7, 15), "int", 1), weighted(loop_graph(100, 5, 16), "int", 2)], 1),
    "dyadic_weights": (lambda: [weighted(R.regular_graph(300, 7, 17), "dyadic", 3),
                                weighted(R.regular_graph(100, 5, 18), "dyadic", 4)], 1),
    "int_weights_global": (lambda: [weighted(R.regular_graph(1000, 7, 19), "int", 5)], 0),
    "dyadic_weights_global": (lambda: [weighted(R.regular_graph(1000, 12, 20), "dyadic", 6)], 0),
}


@pytest.mark.parametrize("case", sorted(OTHER))
@pytest.mark.parametrize("cands,sweeps", [(1, 100), (7, 30), (201, 30)])
def test_other_graphs_match_the_restatement(pkg, case, cands, sweeps):
    graphs, fits = OTHER[case]
    check_against_restatement(pkg, graphs(), cands, sweeps, seed=len(case) + cands, expect_staged=fits)


@pytest.mark.parametrize("fits,make", [(1, lambda: [R.regular_graph(300, 7, 81), loop_graph(120, 5, 82)]),
                                       (0, lambda: [weighted(R.regular_graph(1000, 7, 83), "int", 1)])])
@pytest.mark.parametrize("sweeps,max_descent", [(20, 100), (20, 0)])
def test_a_byte_of_no_class_on_a_movable_node_moves_unconditionally(pkg, fits, make, sweeps, max_descent):
    """Bytes 3, -1 and 100 on movable nodes (also on two adjacent ones): they count for no W and the first annealing
    sweep moves them to the local search's target whatever the level; compared with the restatement."""
    graphs = make()
    nb = int(next(iter(graphs[0][7])))                                  # a neighbour of node 7 of the first graph
    no_class = [(0, 7, 3), (0, nb if nb >= 3 else 9, -1), (2, 50, 100), (3, 299, 3), (4, 3, 3)]
    got = check_against_restatement(pkg, graphs, 7, sweeps, seed=17, max_descent=max_descent, expect_staged=fits,
                                    no_class=no_class)
    if max_descent:                                                     # the descent moves whatever byte is left
        assert ((got["assign"][:, 3:300] >= 0) & (got["assign"][:, 3:300] <= 2)).all()


def test_the_matrix_runs_both_paths_of_the_kernel():
    assert {fits for _g, fits in OTHER.values()} == {0, 1}
    assert {int(n < 4096) for n, *_ in REGULAR} == {0, 1}


def test_a_short_descent_limit_is_kept(pkg):
    got = check_against_restatement(pkg, [R.regular_graph(300, 7, 5)], 7, 10, seed=3, max_descent=1)
    assert (got["sweeps"] == 1).all()
    got = check_against_restatement(pkg, [R.regular_graph(300, 7, 5)], 7, 10, seed=3, max_descent=0)
    assert (got["sweeps"] == 0).all()


@pytest.mark.parametrize("fits,make", [(1, lambda: [weighted(R.regular_graph(300, 7, 21), "real", 7),
                                                   weighted(loop_graph(120, 5, 22), "real", 8)]),
                                       (0, lambda: [weighted(R.regular_graph(1000, 7, 23), "real", 9)])])
def test_real_weights_keep_the_invariants(pkg, fits, make):
    """The snapshot choice rests on block_cut's summation order there, so no byte-for-byte claim."""
    hs, batch = batch_of(make())
    assert staged(pkg, batch) == fits
    A = np.random.RandomState(4).randint(0, 3, (33, batch.R)).astype(np.int8)
    inv_t = AR.schedule(50, scale=float(batch.host.vals.mean()))
    scored = run_anneal(pkg, batch, A, [], 11, 0)                       # no sweep at all: block_cut of the input
    assert (scored["assign"] == A).all()
    got = run_anneal(pkg, batch, A, inv_t, 11, 100)
    assert (got["cut_all"] >= scored["cut_all"]).all()                  # the same fp32 count: no tolerance
    assert (got["cut_all"] > scored["cut_all"]).any()
    for g, h in enumerate(hs):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        out = got["assign"][:, lo:hi]
        assert (out[:, :3] == A[:, lo:lo + 3]).all()
        assert ((out >= 0) & (out <= 2)).all()
        for i in range(A.shape[0]):
            after = RR.cut(h.rowptr, h.col, h.weight, out[i])
            assert abs(got["cut_all"][g, i] - after) <= 1e-5 * after
            before = RR.cut(h.rowptr, h.col, h.weight, A[i, lo:hi])
            assert abs(scored["cut_all"][g, i] - before) <= 1e-5 * before
            assert 0 <= got["snap"][g, i] <= 50 and 1 <= got["sweeps"][g, i] <= 100
    assert (got["snap"] > 0).any()
    check_pick(got, batch)


@pytest.mark.parametrize("cands,max_sweeps", [(1, 100), (201, 100), (201, 1), (7, 0)])
def test_no_annealing_sweeps_is_the_local_search_bit_for_bit(pkg, cands, max_sweeps):
    graphs = [R.regular_graph(1000, 7, 31), weighted(R.regular_graph(300, 7, 32), "real", 1), nx.complete_graph(3),
              loop_graph(120, 5, 33), hub_graph(500, 7, 34)]
    _hs, batch = batch_of(graphs)
    A = np.random.RandomState(cands).randint(0, 3, (cands, batch.R)).astype(np.int8)
    want = run_refine(pkg, batch, A, max_sweeps)
    got = run_anneal(pkg, batch, A, [], 5, max_sweeps)
    for k in want:
        assert (got[k] == want[k]).all(), k
    assert (got["snap"] == 0).all()


def test_seed_decides_the_bytes(pkg):
    _hs, batch = batch_of([R.regular_graph(500, 7, 41), R.regular_graph(100, 5, 42)])
    A = np.random.RandomState(0).randint(0, 3, (7, batch.R)).astype(np.int8)
    inv_t = AR.schedule(30)
    a, b, c = (run_anneal(pkg, batch, A, inv_t, seed, 100) for seed in (1, 1, 2))
    for k in a:
        assert (a[k] == b[k]).all(), k
    assert (a["assign"] != c["assign"]).any(axis=1).any()
    high = run_anneal(pkg, batch, A, inv_t, 1 + (1 << 63), 100)          # the whole 64-bit seed reaches the hash
    assert (a["assign"] != high["assign"]).any()


def test_a_graph_anneals_the_same_alone_and_third_in_a_batch(pkg):
    g = R.regular_graph(500, 7, 51)
    _h1, alone = batch_of([g])
    _h3, third = batch_of([R.regular_graph(300, 12, 52), nx.complete_graph(4), g, R.regular_graph(50, 3, 53)])
    A = np.random.RandomState(1).randint(0, 3, (7, third.R)).astype(np.int8)
    lo, hi = int(third.goff_host[2]), int(third.goff_host[3])
    inv_t = AR.schedule(40)
    a = run_anneal(pkg, alone, A[:, lo:hi], inv_t, 3, 100)
    b = run_anneal(pkg, third, A, inv_t, 3, 100)
    assert (a["assign"] == b["assign"][:, lo:hi]).all()
    assert (a["cut_all"][0] == b["cut_all"][2]).all() and (a["snap"][0] == b["snap"][2]).all()
    assert (a["sweeps"][0] == b["sweeps"][2]).all() and a["best_idx"][0] == b["best_idx"][2]


def test_a_converged_descent_leaves_no_improving_move(pkg):
    graphs = [R.regular_graph(500, 7, 61), weighted(R.regular_graph(200, 6, 62), "int", 1)]
    hs, batch = batch_of(graphs)
    A = np.random.RandomState(2).randint(0, 3, (7, batch.R)).astype(np.int8)
    got = run_anneal(pkg, batch, A, AR.schedule(60, scale=float(batch.host.vals.mean())), 8, 100)
    assert (got["sweeps"] < 100).all()
    for g, h in enumerate(hs):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        for a in got["assign"][:, lo:hi]:
            assert RR.best_single_move_gain(h.n, h.rowptr, h.col, h.weight, a.tolist()) == 0


def test_probe_shows_the_anneal_tag_once_per_call(pkg):
    _hs, batch = batch_of([R.regular_graph(100, 5, 71)])
    A = np.random.RandomState(3).randint(0, 3, (4, batch.R)).astype(np.int8)
    with pkg.hip.Probe(8) as pr:
        run_anneal(pkg, batch, A, AR.schedule(5), 0, 10)
    assert [t for t, _ms in pr.records] == ["anneal"]
    with pkg.hip.Probe(8) as pr:
        run_anneal(pkg, batch, A, AR.schedule(5), 0, 10)
        run_anneal(pkg, batch, A, [], 0, 10)
    assert [t for t, _ms in pr.records] == ["anneal", "anneal"]


@pytest.fixture(scope="module")
def trained(pkg):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    specs = [(50, 6, 50001), (100, 7, 100001), (200, 8, 200001), (300, 6, 300001), (500, 7, 500001)]
    ds = util.product_dataset(specs)
    cfg = T.TrainingConfig(n_nodes=1000, hidden_dim=64)
    torch.manual_seed(0)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    for _ in range(5):
        T.train_single_epoch(ds, net, opt, embed, cfg, graphs_per_step=len(ds))
    net.eval()
    return net, ds


ANNEAL_KEYS = {'annealed_cut', 'annealed_assignment', 'annealed_from'}


def test_decode_dataset_default_is_unchanged_and_anneals_on_request(pkg, trained):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = trained
    np.random.seed(7)
    plain = TN.decode_dataset(net, ds, 200, local_search_sweeps=100)
    after_plain = np.random.rand()
    np.random.seed(7)
    zero = TN.decode_dataset(net, ds, 200, local_search_sweeps=100, anneal_sweeps=0, anneal_candidates=5, anneal_seed=9)
    assert zero == plain and np.random.rand() == after_plain           # same keys, values and RNG consumption
    np.random.seed(7)
    some = TN.decode_dataset(net, ds, 200, local_search_sweeps=100, anneal_sweeps=100, anneal_candidates=16)
    assert np.random.rand() == after_plain
    np.random.seed(7)
    every = TN.decode_dataset(net, ds, 200, anneal_sweeps=30)
    for f, r16, rall, (_g, _a, nx_g, _t) in zip(plain, some, every, ds.values()):
        assert set(r16) == set(f) | ANNEAL_KEYS and set(rall) == (set(f) - {'refined_cut', 'refined_assignment',
                                                                            'refined_from'}) | ANNEAL_KEYS
        assert {k: r16[k] for k in f} == f
        for r, limit in ((r16, 16), (rall, 201)):
            assert r["annealed_cut"] >= max(f["simple_cut"], f["post_cut"])
            assert r["annealed_cut"] == TN.calculate_cut_value(r["annealed_assignment"], nx_g)
            assert r["annealed_assignment"][:3] == [0, 1, 2]
            assert 0 <= r["annealed_from"] < limit
    with pytest.raises(ValueError):
        TN.decode_dataset(net, ds, 200, anneal_sweeps=10, anneal_candidates=202)


def test_annealing_optimization_on_the_argmax_decode(pkg, trained):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = trained
    for g, a_pad, nx_g, _t in ds.values():
        with torch.no_grad():
            P = net(g, a_pad)
        simple = TN.simple_partition_assignment(P)
        got, cut = TN.annealing_optimization(simple, nx_g, sweeps=40, seed=3)
        h = handles_of([nx_g])[0]
        ref, _snap, sweeps = AR.anneal(h.n, h.rowptr, h.col, h.weight, np.asarray([simple], np.int8), AR.schedule(40),
                                       AR.levels(), 3, 100)
        assert got == ref[0].tolist() and int(sweeps[0]) < 100
        assert cut == TN.calculate_cut_value(got, nx_g) >= TN.calculate_cut_value(simple, nx_g)
        assert got[:3] == [0, 1, 2]
        local, local_cut = TN.local_search_optimization(simple, nx_g)
        same, cut0 = TN.annealing_optimization(simple, nx_g, sweeps=0)
        assert same == local and cut0 == local_cut
        kept, cut00 = TN.annealing_optimization(simple, nx_g, sweeps=0, max_descent_sweeps=0)
        assert kept == simple and cut00 == TN.calculate_cut_value(simple, nx_g)
    with pytest.raises(ValueError):
        TN.annealing_optimization(simple[:-1], nx_g)
    with pytest.raises(ValueError):
        TN.annealing_optimization(simple[:-1] + [3], nx_g)
    with pytest.raises(ValueError):
        TN.annealing_optimization(simple, nx_g, sweeps=-1)


@pytest.mark.parametrize("n,graph_seed,cands", [(500, 100, 201), (500, 101, 201), (1000, 100, 16)])
def test_worst_annealed_candidate_beats_the_best_local_search_candidate_on_the_device(pkg, n, graph_seed, cands):
    """7-regular graphs, uniform random candidates with nodes 0..2 fixed, 100 sweeps from T = 1.5 to 0.15, seed 1.
    (The CPU restatement gives 1671 against 1602 and 1672 against 1604 at n = 500: tests/test_anneal_host.py.)"""
    _hs, batch = batch_of([nx.random_regular_graph(7, n, seed=graph_seed)])
    A = np.random.RandomState(0).randint(0, 3, (cands, n)).astype(np.int8)
    A[:, :3] = [0, 1, 2]
    local = run_refine(pkg, batch, A, 100)["cut_all"][0]
    annealed = run_anneal(pkg, batch, A, AR.schedule(100), 1, 100)["cut_all"][0]
    print(f"n {n} seed {graph_seed}: local search best {local.max()} mean {local.mean():.1f}; annealed best "
          f"{annealed.max()} mean {annealed.mean():.1f} worst {annealed.min()}")
    assert annealed.min() > local.max()
