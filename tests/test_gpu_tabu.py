"""GPU tests of the tabu stage (gmc_kway_tabu_f32 and its Python API) against the CPU restatement in tests/tabu_ref.py:
`assign`, `best_iter` and `moves` byte for byte on every kind of weight (each step of the rule is one fp32 operation,
so real-valued weights too), `cut_all` and the pick against a recount - the float64 count rounded once for unit and
integer weights, the device's own scoring of the same bytes through the annealing's entry point for real ones."""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import tabu_ref as TR
from tests import util
from tests.test_gpu_rounding import RawBatch, small_model
from tests.test_refine_host import gnp_graph, handles_of, loop_graph
from tests.test_tabu_host import lds_shape

pytestmark = pytest.mark.gpu

GARBAGE = -5
SEED = 0xFEEDC0DE1234567
TENURE = (3, 0, 10)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def weighted(g, kind, seed):
    rng = np.random.RandomState(seed)
    draw = {"int": lambda: int(rng.randint(1, 6)), "signed": lambda: int(rng.choice([-1, 1])),
            "real": lambda: float(np.float32(rng.uniform(0.1, 2.0)))}[kind]   # full mantissas
    for u, v in g.edges():
        g[u][v]["weight"] = draw()
    return g


def batch_of(pkg, graphs, global_csr=False):
    """(handles, RawBatch).  global_csr: nnz_max overstated (it only sizes the LDS copy), so the launcher leaves the
    copy out and the same graphs run over the batch's arrays in global memory."""
    hs = handles_of(graphs)
    batch = RawBatch(pkg, hs)
    if global_csr:
        batch.c.nnz_max = 1 << 24
    return hs, batch


def spans(batch):
    return [(int(batch.goff_host[g]), int(batch.goff_host[g + 1])) for g in range(batch.B)]


def shape_of(pkg, batch, K):
    s = pkg.hip.load().gmc_kway_tabu_shape(batch.ref(), K)
    assert s > 0, s
    return s & 15, s >> 4


def starts(batch, K, cands, terminals, seed):
    """[cands, R] int8: random classes, the terminals of every graph in their own."""
    A = np.random.RandomState(seed).randint(0, K, (cands, batch.R)).astype(np.int8)
    if terminals:
        for lo, hi in spans(batch):
            m = min(K, hi - lo)
            A[:, lo:lo + m] = np.arange(m)
    return A


def run_tabu(pkg, batch, K, terminals, A, iterations, tenure=TENURE, seed=SEED, counters=True, stream=None):
    """gmc_kway_tabu_f32 on A [cands, R] int8 with every output pre-filled with garbage; returns the status code too."""
    hip = pkg.hip
    cands = A.shape[0]
    assign = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    best_iter = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    moves = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = hip.load().gmc_kway_tabu_f32(batch.ref(), K, int(terminals), cands, p(assign), iterations, *tenure, seed,
                                          p(cut_all), p(best_assign), p(best_cut), p(best_idx),
                                          p(best_iter) if counters else None, p(moves) if counters else None,
                                          hip.stream())
    torch.cuda.synchronize()
    out = dict(assign=assign, cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_idx=best_idx,
               best_iter=best_iter, moves=moves)
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def check_pick(got, batch, ran):
    for g, (lo, hi) in enumerate(spans(batch)):
        if not ran[g]:
            assert np.isnan(got["best_cut"][g]) and got["best_idx"][g] == GARBAGE
            assert (got["best_assign"][lo:hi] == GARBAGE).all()
            continue
        bi = int(np.argmax(got["cut_all"][g]))                          # the first of the largest
        assert got["best_idx"][g] == bi and got["best_cut"][g].tobytes() == got["cut_all"][g, bi].tobytes()
        assert (got["best_assign"][lo:hi] == got["assign"][bi, lo:hi]).all()


def check(pkg, hs, batch, K, terminals, A, iterations, tenure=TENURE, seed=SEED, ref=None, exact_cuts=True):
    """One call against the restatement, graph by graph; a skipped graph keeps its garbage.  ref: per graph the
    (assign, best_it, moves) of tabu_all for at least A.shape[0] candidates (computed here when None)."""
    rc, got = run_tabu(pkg, batch, K, terminals, A, iterations, tenure, seed)
    assert rc == 0, rc
    first = K if terminals else 0
    ran = [max(first, 1) <= h.n <= batch.c.n_max for h in hs]
    cands = A.shape[0]
    refs = []
    for g, (h, (lo, hi)) in enumerate(zip(hs, spans(batch))):
        where = (g, h.n)
        if not ran[g]:
            assert (got["assign"][:, lo:hi] == A[:, lo:hi]).all() and np.isnan(got["cut_all"][g]).all(), where
            assert (got["best_iter"][g] == GARBAGE).all() and (got["moves"][g] == GARBAGE).all(), where
            refs.append(None)
            continue
        r = ref[g] if ref is not None else TR.tabu_all(h.n, h.rowptr, h.col, h.weight, A[:, lo:hi], K, terminals,
                                                       iterations, *tenure, seed=seed)
        refs.append(r)
        assert got["assign"][:, lo:hi].tobytes() == np.ascontiguousarray(r[0][:cands]).tobytes(), where
        assert got["best_iter"][g].tobytes() == r[1][:cands].tobytes(), where
        assert got["moves"][g].tobytes() == r[2][:cands].tobytes(), where
        if exact_cuts:
            assert got["cut_all"][g].tobytes() == AR.cuts_f32(h.rowptr, h.col, h.weight, got["assign"][:, lo:hi]).tobytes()
            assert (got["cut_all"][g] >= AR.cuts_f32(h.rowptr, h.col, h.weight, A[:, lo:hi])).all()
    check_pick(got, batch, ran)
    return got, refs


# ---- lane ownership, class counts, sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_mov", (0, 1, 63, 64, 65, 129))
def test_lane_ownership(pkg, n_mov):
    """n = K with terminals has nothing movable (n_mov = 0 must not divide); the other sizes sit around a wave."""
    for K, terminals in ((3, True), (2, False)):
        n = n_mov + (K if terminals else 0)
        if n < 2:                                                       # (a graph needs an edge for its arrays to exist)
            continue
        g = nx.complete_graph(n) if n <= 4 else util.near_regular(n, 3, n, attrs=False)
        hs, batch = batch_of(pkg, [g])
        got, _ = check(pkg, hs, batch, K, terminals, starts(batch, K, 3, terminals, n), 150)
        if n_mov == 0:
            assert (got["moves"] == 0).all() and (got["best_iter"] == 0).all()


@pytest.mark.parametrize("terminals", (True, False))
@pytest.mark.parametrize("K", range(2, 9))
def test_class_counts(pkg, K, terminals):
    hs, batch = batch_of(pkg, [R.regular_graph(100, 5, K)])
    got, _ = check(pkg, hs, batch, K, terminals, starts(batch, K, 5, terminals, K), 300)
    assert (got["moves"] > 0).all() and (got["best_iter"] > 0).all()


def test_4096_nodes_at_two_classes(pkg):
    hs, batch = batch_of(pkg, [util.near_regular(4096, 3, 4096, attrs=False)])
    check(pkg, hs, batch, 2, False, starts(batch, 2, 2, False, 1), 300)


def test_the_largest_graph_at_eight_classes_and_the_refusal_beyond(pkg):
    lib = pkg.hip.load()
    hs, batch = batch_of(pkg, [util.near_regular(4096, 3, 4097, attrs=False)])
    assert lib.gmc_kway_tabu_fits(batch.ref(), 8) == 1 and shape_of(pkg, batch, 8)[0] == 1
    check(pkg, hs, batch, 8, True, starts(batch, 8, 2, True, 2), 120)
    hs, batch = batch_of(pkg, [nx.cycle_graph(4097)])
    assert lib.gmc_kway_tabu_fits(batch.ref(), 8) == 0
    A = starts(batch, 8, 1, True, 3)
    rc, got = run_tabu(pkg, batch, 8, True, A, 10)
    assert rc == -6 and (got["assign"] == A).all() and np.isnan(got["cut_all"]).all()


def test_the_workloads_graph_at_2000_iterations(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(1000, 7, 17)])
    assert shape_of(pkg, batch, 2) == (4, 1)
    got, _ = check(pkg, hs, batch, 2, False, starts(batch, 2, 2, False, 4), 2000)
    assert (got["best_iter"] > 200).all()


# ---- chains per workgroup, staged against global ---------------------------------------------------------------------
PACKING = {4: (100, 3, 150), 2: (1100, 8, 60), 1: (2200, 8, 40)}   # slots -> n, K, iterations (d = 3)


@functools.lru_cache(maxsize=None)
def packing_case(slots):
    n, K, iterations = PACKING[slots]
    g = util.near_regular(n, 3, n, attrs=False)
    h = handles_of([g])[0]
    A = np.random.RandomState(slots).randint(0, K, (9, n)).astype(np.int8)
    A[:, :K] = np.arange(K)
    return g, A, TR.tabu_all(n, h.rowptr, h.col, h.weight, A, K, True, iterations, *TENURE, seed=SEED)


@pytest.mark.parametrize("global_csr", (False, True))
@pytest.mark.parametrize("slots", (4, 2, 1))
def test_chains_per_workgroup(pkg, slots, global_csr):
    """1, 3, 4, 5 and 9 candidates - fewer chains than slots, a full workgroup, a last workgroup with one chain - on
    shapes the launcher packs four, two and one to a workgroup, through the LDS copy of the CSR and without it."""
    n, K, iterations = PACKING[slots]
    g, A, ref = packing_case(slots)
    hs, batch = batch_of(pkg, [g], global_csr)
    assert shape_of(pkg, batch, K) == (slots, int(not global_csr))
    assert lds_shape(K, n, batch.c.nnz_max, False) == (slots, int(not global_csr))
    for cands in (1, 3, 4, 5, 9):
        check(pkg, hs, batch, K, True, A[:cands], iterations, ref=[ref])


def test_a_dense_graph_that_does_not_fit_the_copy(pkg):
    hs, batch = batch_of(pkg, [gnp_graph(600, 0.5, 6)])
    assert shape_of(pkg, batch, 2) == (4, 0)
    check(pkg, hs, batch, 2, False, starts(batch, 2, 5, False, 6), 200)


# ---- rows ----------------------------------------------------------------------------------------------------------
def hubs_graph():
    """200 nodes on a cycle, nodes 10, 20 and 30 raised to degree 64, 65 and 130 by edges to nodes from 40 up."""
    g = nx.cycle_graph(200)
    for hub, degree in ((10, 64), (20, 65), (30, 130)):
        for u in range(40, 40 + degree - 2):
            g.add_edge(hub, u)
        assert g.degree(hub) == degree
    return g


def isolated_graph():
    g = R.regular_graph(40, 3, 9)
    g.add_nodes_from(range(40, 46))                                     # degree 0: built from handles
    return g


@pytest.mark.parametrize("name", ("hubs", "isolated", "loops"))
@pytest.mark.parametrize("global_csr", (False, True))
def test_rows(pkg, name, global_csr):
    g = {"hubs": hubs_graph, "isolated": isolated_graph, "loops": lambda: loop_graph(60, 4, 3)}[name]()
    hs, batch = batch_of(pkg, [g], global_csr)
    if name == "isolated":
        assert (np.diff(hs[0].rowptr) == 0).sum() == 6
    for K, terminals in ((3, True), (2, False)):
        check(pkg, hs, batch, K, terminals, starts(batch, K, 3, terminals, 5), 300)


# ---- weights -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("global_csr", (False, True))
@pytest.mark.parametrize("kind", ("int", "signed"))
def test_integer_weights(pkg, kind, global_csr):
    hs, batch = batch_of(pkg, [weighted(R.regular_graph(120, 6, 12), kind, 3)], global_csr)
    for K, terminals in ((4, True), (2, False)):
        check(pkg, hs, batch, K, terminals, starts(batch, K, 4, terminals, 8), 300)


def device_recount(pkg, batch, K, assign):
    """The cut of every row of assign as the decoders score it: the annealing's entry point without a sweep."""
    hip = pkg.hip
    cands = assign.shape[0]
    order, cgoff, cptr = batch.refine_order(K)
    a = torch.from_numpy(np.ascontiguousarray(assign)).cuda()
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.empty(batch.R, dtype=torch.int32, device="cuda")
    best_cut = torch.empty(batch.B, device="cuda")
    best_idx = torch.empty(batch.B, dtype=torch.int32, device="cuda")
    p = hip.ptr
    hip.check(hip.load().gmc_kway_refine_anneal_f32(batch.ref(), K, p(order), p(cgoff), p(cptr), cands, p(a), None, 0,
                                                    None, 0, 0, p(cut_all), p(best_assign), p(best_cut), p(best_idx),
                                                    None, None, hip.stream()), "gmc_kway_refine_anneal_f32")
    torch.cuda.synchronize()
    assert (a.cpu().numpy() == assign).all()
    return cut_all.cpu().numpy()


@pytest.mark.parametrize("global_csr", (False, True))
def test_real_weights_byte_for_byte(pkg, global_csr):
    """Full-mantissa weights: the table drifts by rounding, the same way on both sides only if every update is the one
    fp32 operation the header names, in its order - a contracted or reordered update shows here."""
    K = 3
    hs, batch = batch_of(pkg, [weighted(R.regular_graph(150, 7, 21), "real", 7)], global_csr)
    A = starts(batch, K, 4, True, 9)
    got, _ = check(pkg, hs, batch, K, True, A, 300, exact_cuts=False)
    assert got["cut_all"].tobytes() == device_recount(pkg, batch, K, got["assign"]).tobytes()
    exact = np.asarray([TR.cut_f64(hs[0].rowptr, hs[0].col, hs[0].weight, a) for a in got["assign"]])
    assert np.abs(got["cut_all"][0] - exact).max() <= 1e-5 * exact.max()


# ---- batches -------------------------------------------------------------------------------------------------------
def test_a_mixed_batch(pkg):
    """5, 64 and 700 nodes, a graph below its terminals (skipped), and the 64-node graph twice."""
    K = 4
    g64 = util.near_regular(64, 3, 64, attrs=False)
    graphs = [util.near_regular(5, 2, 5, attrs=False), g64, nx.complete_graph(3), R.regular_graph(700, 5, 7), g64]
    hs, batch = batch_of(pkg, graphs)
    A = starts(batch, K, 5, True, 10)
    (lo1, hi1), (lo4, hi4) = spans(batch)[1], spans(batch)[4]
    A[:, lo4:hi4] = A[:, lo1:hi1]
    got, _ = check(pkg, hs, batch, K, True, A, 200)
    assert got["assign"][:, lo1:hi1].tobytes() == got["assign"][:, lo4:hi4].tobytes()
    for k in ("cut_all", "best_iter", "moves"):
        assert got[k][1].tobytes() == got[k][4].tobytes(), k
    _hs, alone = batch_of(pkg, [g64])
    rc, solo = run_tabu(pkg, alone, K, True, np.ascontiguousarray(A[:, lo1:hi1]), 200)
    assert rc == 0 and solo["assign"].tobytes() == np.ascontiguousarray(got["assign"][:, lo1:hi1]).tobytes()
    for k in ("cut_all", "best_iter", "moves"):
        assert solo[k][0].tobytes() == got[k][1].tobytes(), k


# ---- tenure --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tenure,stalls", (((40, 0, 0), True), ((0, 0, 0), False), ((3, 4, 0), False),
                                           ((2, 0, 1), False)))
def test_tenure(pkg, tenure, stalls):
    """tenure_base >= n_mov: every node ends up banned, iterations pass without an admissible move; base 0 with span
    0: a node may move back at once; tenure_div = 0: no size term; tenure_div = 1: up to n_mov."""
    hs, batch = batch_of(pkg, [R.regular_graph(30, 3, 5)])
    got, _ = check(pkg, hs, batch, 2, False, starts(batch, 2, 3, False, 2), 200, tenure)
    assert ((got["moves"] < 200).all() and (got["moves"] >= 30).all()) if stalls else (got["moves"] == 200).all()


def test_no_iterations_score_and_pick(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(100, 5, 3), weighted(R.regular_graph(50, 4, 4), "int", 1)])
    A = starts(batch, 3, 6, True, 3)
    got, _ = check(pkg, hs, batch, 3, True, A, 0)
    assert (got["assign"] == A).all() and (got["moves"] == 0).all() and (got["best_iter"] == 0).all()


# ---- reproducibility -------------------------------------------------------------------------------------------------
def test_two_runs_another_stream_and_null_counters_give_the_same_bytes(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(300, 7, 8), weighted(R.regular_graph(200, 6, 9), "real", 2)])
    A = starts(batch, 5, 7, False, 4)
    rc, first = run_tabu(pkg, batch, 5, False, A, 300)
    assert rc == 0 and (first["assign"] != A).any()
    runs = [run_tabu(pkg, batch, 5, False, A, 300), run_tabu(pkg, batch, 5, False, A, 300, stream=torch.cuda.Stream()),
            run_tabu(pkg, batch, 5, False, A, 300, counters=False)]
    for i, (rc, other) in enumerate(runs):
        assert rc == 0
        for k in first:
            if i == 2 and k in ("best_iter", "moves"):
                assert (other[k] == GARBAGE).all()
            else:
                assert other[k].tobytes() == first[k].tobytes(), (i, k)
    rc, reseeded = run_tabu(pkg, batch, 5, False, A, 300, seed=SEED + (1 << 63))   # the whole 64-bit seed reaches the hash
    assert rc == 0 and (reseeded["assign"] != first["assign"]).any()


def test_a_byte_of_no_class_is_inert(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(100, 5, 3)])
    A = starts(batch, 3, 3, True, 3)
    A[0, 10], A[1, 20], A[2, 99] = 3, -1, 100
    got, _ = check(pkg, hs, batch, 3, True, A, 200, exact_cuts=False)
    assert got["assign"][0, 10] == 3 and got["assign"][1, 20] == -1 and got["assign"][2, 99] == 100


# ---- the Python API ------------------------------------------------------------------------------------------------
def test_kway_tabu_search_on_one_graph(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = R.regular_graph(60, 5, 1)
    h = handles_of([g])[0]
    for K, terminals in ((3, True), (2, False)):
        a0 = np.random.RandomState(K).randint(0, K, 60).astype(np.int8)
        if terminals:
            a0[:K] = np.arange(K)
        assign, cut = TN.kway_tabu_search(a0.tolist(), g, K, iterations=150, seed=9, terminals=terminals)
        ref = TR.tabu(60, h.rowptr, h.col, h.weight, a0, K, terminals, 0, 150, seed=9)
        assert assign == ref.assign.tolist() and cut == TN.calculate_cut_value(assign, g)
        assert cut == TN.calculate_cut_value(a0.tolist(), g) + float(ref.best)
        default, _cut = TN.kway_tabu_search(a0.tolist(), g, K, seed=9, terminals=terminals)   # 20 n iterations
        assert default == TR.tabu(60, h.rowptr, h.col, h.weight, a0, K, terminals, 0, 1200, seed=9).assign.tolist()
    with pytest.raises(ValueError):
        TN.kway_tabu_search([0] * 60, g, 2, iterations=-1)
    with pytest.raises(ValueError):
        TN.kway_tabu_search([0] * 60, g, 2, tenure_base=-1)


def test_search_dataset_with_and_without_tabu(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    K = 4
    net, ds = small_model(pkg, K, [(60, 5, 61), (48, 6, 62), (100, 7, 63)], 128, 16, seed=K)
    kw = dict(samples=20, sample_seed=5, anneal_sweeps=20, anneal_seed=2)
    plain = TN.search_dataset(net, ds, **kw)
    zero = TN.search_dataset(net, ds, **kw, tabu_iterations=0, tabu_seed=3)
    assert repr(zero) == repr(plain)                                    # key for key, value for value, type for type
    for extra in (dict(), dict(generations=2, generation_sweeps=5)):
        base = TN.search_dataset(net, ds, **kw, **extra)
        tabu = TN.search_dataset(net, ds, **kw, **extra, tabu_iterations=200, tabu_seed=3)
        for res, b, (handle, _a_pad, nx_g, _t) in zip(tabu, base, ds.values()):
            assert set(res) == set(b) | {"tabu_cut", "tabu_assignment", "tabu_iteration"}
            assert repr({k: res[k] for k in b}) == repr(b)              # no other key changes
            a = res["tabu_assignment"]
            assert res["tabu_cut"] == TN.calculate_cut_value(a, nx_g)
            assert res["tabu_cut"] >= res.get("evolved_cut", res["searched_cut"])   # unit weights: never below its input
            assert a[:K] == list(range(K)) and 0 <= min(a) and max(a) < K and len(a) == handle.n
            assert 0 <= res["tabu_iteration"] <= 200
    with pytest.raises(ValueError):
        TN.search_dataset(net, ds, **kw, tabu_iterations=-1)


def test_maxcut_solve_with_and_without_tabu(pkg):
    from gcn_max_cut_amd import maxcut
    from tests.test_gpu_plain_instance import host_cuts, solve_inputs
    ei, ptr = solve_inputs()
    kw = dict(number_classes=2, hidden_dim=8, epochs=30, learning_rate=2e-2, samples=8, anneal_sweeps=20, seed=4)
    plain = maxcut.solve(ei, ptr, **kw)
    zero = maxcut.solve(ei, ptr, **kw, tabu_iterations=0)
    assert plain.annealed_cut is None and zero.annealed_cut is None
    for name in ("partition", "cut", "trained_cut", "rounded_cut", "ptr"):
        assert getattr(zero, name).cpu().numpy().tobytes() == getattr(plain, name).cpu().numpy().tobytes(), name
    res = maxcut.solve(ei, ptr, **kw, tabu_iterations=200)
    cut, annealed = res.cut.cpu().numpy(), res.annealed_cut.cpu().numpy()
    assert annealed.tobytes() == plain.cut.cpu().numpy().tobytes()
    assert (cut >= annealed).all()
    assert (cut >= np.maximum(res.trained_cut.cpu().numpy(), res.rounded_cut.cpu().numpy())).all()
    assert np.array_equal(cut, host_cuts(ei, ptr, res.partition.cpu().numpy()))
    for name in ("trained_cut", "rounded_cut", "ptr"):
        assert getattr(res, name).cpu().numpy().tobytes() == getattr(plain, name).cpu().numpy().tobytes(), name
    batch = pkg.GraphBatch.from_edge_index(ei, ptr)
    with pytest.raises(NotImplementedError):
        maxcut.solve_large_batch(batch, hidden_dim=8, epochs=1, learning_rate=1e-2, tabu_iterations=10)
