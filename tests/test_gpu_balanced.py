"""GPU tests of the tabu search under class-size bounds (gmc_kway_balance_f32 and its Python API) against the CPU
restatement in tests/balanced_ref.py: `assign`, `best_iter`, `moves`, `repairs`, `feasible` and the pick byte for byte
on every kind of weight; `cut_all` against the bits gmc_kway_tabu_f32 with iterations = 0 reports for the same bytes;
every candidate written within its bounds."""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import balanced_ref as BR
from tests import tabu_ref as TR
from tests import util
from tests.test_balanced_host import bridge_graph, bridge_starts, feasible
from tests.test_gpu_tabu import (GARBAGE, PACKING, SEED, TENURE, batch_of, check_pick, hubs_graph, isolated_graph,
                                 packing_case, run_tabu, spans, starts, weighted)
from tests.test_refine_host import gnp_graph, handles_of, loop_graph

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def exact(hs, K):
    """lo, hi int32 [B, K]: floor and ceil of n / K."""
    return (np.asarray([[h.n // K] * K for h in hs], np.int32), np.asarray([[-(-h.n // K)] * K for h in hs], np.int32))


def loose(hs, K):
    return np.zeros((len(hs), K), np.int32), np.asarray([[h.n] * K for h in hs], np.int32)


def shape_of(pkg, batch, K):
    s = pkg.hip.load().gmc_kway_balance_shape(batch.ref(), K)
    assert s > 0, s
    return s & 15, s >> 4


def run_balance(pkg, batch, K, terminals, A, lo, hi, iterations, tenure=TENURE, seed=SEED, optional=True, stream=None):
    """gmc_kway_balance_f32 on A [cands, R] int8 with every output pre-filled with garbage; returns the status code too."""
    hip = pkg.hip
    cands = A.shape[0]
    assign = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    size_lo = torch.from_numpy(np.ascontiguousarray(lo, np.int32)).cuda()
    size_hi = torch.from_numpy(np.ascontiguousarray(hi, np.int32)).cuda()
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    counters = {k: torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
                for k in ("best_iter", "moves", "repairs")}
    ok = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    opt = (lambda t: p(t)) if optional else (lambda t: None)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        rc = hip.load().gmc_kway_balance_f32(batch.ref(), K, int(terminals), cands, p(assign), p(size_lo), p(size_hi),
                                             iterations, *tenure, seed, p(cut_all), p(best_assign), p(best_cut),
                                             p(best_idx), opt(counters["best_iter"]), opt(counters["moves"]),
                                             opt(counters["repairs"]), opt(ok), hip.stream())
    torch.cuda.synchronize()
    out = dict(assign=assign, cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_idx=best_idx,
               feasible=ok, **counters)
    return rc, {k: v.cpu().numpy() for k, v in out.items()}


def check(pkg, hs, batch, K, terminals, A, lo, hi, iterations, tenure=TENURE, seed=SEED, ref=None):
    """One call against the restatement, graph by graph; a skipped graph keeps its garbage.  ref: per graph the
    (assign, best_it, moves, repairs) of balanced_all for at least A.shape[0] candidates (computed here when None)."""
    rc, got = run_balance(pkg, batch, K, terminals, A, lo, hi, iterations, tenure, seed)
    assert rc == 0, rc
    first = K if terminals else 0
    sized = [max(first, 1) <= h.n <= batch.c.n_max for h in hs]
    ran = [sized[g] and BR.admits(lo[g], hi[g], h.n, terminals) for g, h in enumerate(hs)]
    cands = A.shape[0]
    rc, scored = run_tabu(pkg, batch, K, terminals, got["assign"], 0)   # the bits tabu reports for the same bytes
    assert rc == 0 and (scored["assign"] == got["assign"]).all()
    for g, (h, (a, b)) in enumerate(zip(hs, spans(batch))):
        where = (g, h.n)
        assert got["feasible"][g] == (GARBAGE if not sized[g] else int(ran[g])), where
        if not ran[g]:
            assert (got["assign"][:, a:b] == A[:, a:b]).all() and np.isnan(got["cut_all"][g]).all(), where
            for k in ("best_iter", "moves", "repairs"):
                assert (got[k][g] == GARBAGE).all(), (where, k)
            continue
        r = ref[g] if ref is not None else BR.balanced_all(h.n, h.rowptr, h.col, h.weight, A[:, a:b], K, terminals,
                                                           lo[g], hi[g], iterations, *tenure, seed=seed)
        assert got["assign"][:, a:b].tobytes() == np.ascontiguousarray(r[0][:cands]).tobytes(), where
        assert got["best_iter"][g].tobytes() == r[1][:cands].tobytes(), where
        assert got["moves"][g].tobytes() == r[2][:cands].tobytes(), where
        assert got["repairs"][g].tobytes() == r[3][:cands].tobytes(), where
        assert got["cut_all"][g].tobytes() == scored["cut_all"][g].tobytes(), where
        for c in range(cands):
            assert feasible(got["assign"][c, a:b], K, lo[g], hi[g]), (where, c)
            assert (got["assign"][c, a:a + first] == np.arange(first)).all()
    check_pick(got, batch, ran)
    return got


# ---- lane ownership, class counts, sizes ----------------------------------------------------------------------------
@pytest.mark.parametrize("n_mov", (1, 63, 64, 65, 129))
def test_lane_ownership(pkg, n_mov):
    for K, terminals in ((3, True), (2, False)):
        n = n_mov + (K if terminals else 0)
        if n < 2:                                                       # (a graph needs an edge for its arrays to exist)
            continue
        g = nx.complete_graph(n) if n <= 4 else util.near_regular(n, 3, n, attrs=False)
        hs, batch = batch_of(pkg, [g])
        A = starts(batch, K, 3, terminals, n)
        A[0, (K if terminals else 0):] = 0                              # one candidate that needs the repair
        got = check(pkg, hs, batch, K, terminals, A, *exact(hs, K), 150)
        if n > 4:
            assert got["repairs"][0, 0] > 0


@pytest.mark.parametrize("terminals", (True, False))
@pytest.mark.parametrize("K", range(2, 9))
def test_class_counts(pkg, K, terminals):
    """About 60 nodes, one graph whose size K divides (lo = hi: every move is paired) and one it does not."""
    n = 60 - 60 % K
    hs, batch = batch_of(pkg, [util.near_regular(n, 3, K, attrs=False), util.near_regular(n + 1, 3, K + 10, attrs=False)])
    got = check(pkg, hs, batch, K, terminals, starts(batch, K, 3, terminals, K), *exact(hs, K), 300)
    assert (got["moves"] > 0).all() and (got["best_iter"] > 0).any()


def test_the_largest_graph_at_eight_classes_and_the_refusal_beyond(pkg):
    lib = pkg.hip.load()
    hs, batch = batch_of(pkg, [util.near_regular(4096, 3, 4097, attrs=False)])
    assert lib.gmc_kway_balance_fits(batch.ref(), 8) == 1 and shape_of(pkg, batch, 8)[0] == 1
    check(pkg, hs, batch, 8, True, starts(batch, 8, 2, True, 2), *exact(hs, 8), 64)
    hs, batch = batch_of(pkg, [nx.cycle_graph(4097)])
    assert lib.gmc_kway_balance_fits(batch.ref(), 8) == 0
    A = starts(batch, 8, 1, True, 3)
    rc, got = run_balance(pkg, batch, 8, True, A, *exact(hs, 8), 10)
    assert rc == -6 and (got["assign"] == A).all() and np.isnan(got["cut_all"]).all() and got["feasible"][0] == GARBAGE


def test_4096_nodes_in_one_class_take_2048_repair_moves(pkg):
    hs, batch = batch_of(pkg, [util.near_regular(4096, 3, 4096, attrs=False)])
    A = np.zeros((1, 4096), np.int8)
    got = check(pkg, hs, batch, 2, False, A, *exact(hs, 2), 16)
    assert got["repairs"][0, 0] == 2048


# ---- chains per workgroup, staged against global ---------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def packing_ref(slots):
    n, K, iterations = PACKING[slots]
    g, A, _tabu = packing_case(slots)
    h = handles_of([g])[0]
    lo, hi = exact([h], K)
    return BR.balanced_all(n, h.rowptr, h.col, h.weight, A, K, True, lo[0], hi[0], iterations, *TENURE, seed=SEED)


@pytest.mark.parametrize("global_csr", (False, True))
@pytest.mark.parametrize("slots", (4, 2, 1))
def test_chains_per_workgroup(pkg, slots, global_csr):
    n, K, iterations = PACKING[slots]
    g, A, _tabu = packing_case(slots)
    hs, batch = batch_of(pkg, [g], global_csr)
    assert shape_of(pkg, batch, K) == (slots, int(not global_csr))
    for cands in (1, 3, 4, 5, 9):
        check(pkg, hs, batch, K, True, A[:cands], *exact(hs, K), iterations, ref=[packing_ref(slots)])


# ---- bounds ----------------------------------------------------------------------------------------------------------
def test_a_mixed_batch_with_bounds_per_graph(pkg):
    """Graphs of 5, 64, 3 (below its terminals: skipped), 150 and 64 nodes: exact, loose, -, one-sided above, one-sided
    below; and the same batch with the bounds of graph 1 admitting no partition."""
    K = 4
    g64 = util.near_regular(64, 3, 64, attrs=False)
    graphs = [util.near_regular(5, 2, 5, attrs=False), g64, nx.complete_graph(3), R.regular_graph(150, 5, 7), g64]
    hs, batch = batch_of(pkg, graphs)
    lo, hi = exact(hs, K)
    lo[1], hi[1] = 0, 64
    lo[3] = 0                                                           # hi = ceil(150 / 4) only
    hi[4] = 64                                                          # lo = 16 only
    A = starts(batch, K, 5, True, 10)
    A[0, :] = 0
    for a, b in spans(batch):
        A[0, a:a + min(K, b - a)] = np.arange(min(K, b - a))
    got = check(pkg, hs, batch, K, True, A, lo, hi, 200)
    assert got["repairs"][3, 0] > 0 and got["repairs"][1, 0] == 0
    for bad_lo, bad_hi in (((20, 20, 20, 20), (64,) * 4), ((0,) * 4, (15,) * 4), ((5, 0, 0, 0), (4, 64, 64, 64)),
                           ((0,) * 4, (64, 0, 64, 64))):
        lo2, hi2 = lo.copy(), hi.copy()
        lo2[1], hi2[1] = bad_lo, bad_hi
        other = check(pkg, hs, batch, K, True, A, lo2, hi2, 200)
        assert other["feasible"].tolist() == [1, 0, GARBAGE, 1, 1]
        for g in (0, 3, 4):                                             # the others are unaffected
            a, b = spans(batch)[g]
            assert other["assign"][:, a:b].tobytes() == got["assign"][:, a:b].tobytes()
            assert other["cut_all"][g].tobytes() == got["cut_all"][g].tobytes()
            assert other["best_cut"][g].tobytes() == got["best_cut"][g].tobytes()


def test_a_class_held_at_its_terminal_and_an_empty_class(pkg):
    """lo = hi = 1 under terminals: m[b] = 0, no free and no paired move into class b.  hi = 0 without terminals: the class
    is emptied by the repair and stays empty."""
    K = 3
    hs, batch = batch_of(pkg, [R.regular_graph(60, 5, 3)])
    lo, hi = np.asarray([[0, 1, 0]], np.int32), np.asarray([[60, 1, 60]], np.int32)
    got = check(pkg, hs, batch, K, True, starts(batch, K, 4, True, 1), lo, hi, 200)
    assert ((got["assign"] == 1).sum(axis=1) == 1).all() and (got["repairs"] > 0).all() and (got["moves"] > 0).all()
    lo, hi = np.asarray([[0, 0, 0]], np.int32), np.asarray([[60, 0, 60]], np.int32)
    got = check(pkg, hs, batch, K, False, starts(batch, K, 4, False, 2), lo, hi, 200)
    assert not (got["assign"] == 1).any() and (got["moves"] > 0).all()


def test_loose_bounds_are_the_tabu_search_byte_for_byte(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(300, 7, 8), weighted(R.regular_graph(200, 6, 9), "real", 2),
                               weighted(R.regular_graph(120, 6, 12), "signed", 3)])
    for K, terminals in ((5, False), (3, True), (2, False), (8, True)):
        A = starts(batch, K, 6, terminals, K)
        rc, tabu = run_tabu(pkg, batch, K, terminals, A, 300)
        rc2, got = run_balance(pkg, batch, K, terminals, A, *loose(hs, K), 300)
        assert rc == 0 and rc2 == 0 and (got["assign"] != A).any()
        for k in tabu:
            assert got[k].tobytes() == tabu[k].tobytes(), (K, k)
        assert (got["repairs"] == 0).all() and (got["feasible"] == 1).all()


# ---- weights and rows ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("global_csr", (False, True))
@pytest.mark.parametrize("kind", ("unit", "int", "signed", "real"))
def test_weights(pkg, kind, global_csr):
    """Full-mantissa weights too: every update is the one fp32 operation the header names, in its order."""
    g = R.regular_graph(120, 6, 12)
    hs, batch = batch_of(pkg, [g if kind == "unit" else weighted(g, kind, 3)], global_csr)
    for K, terminals in ((4, True), (2, False)):
        check(pkg, hs, batch, K, terminals, starts(batch, K, 4, terminals, 8), *exact(hs, K), 300)


@pytest.mark.parametrize("name", ("hubs", "isolated", "loops"))
@pytest.mark.parametrize("global_csr", (False, True))
def test_rows(pkg, name, global_csr):
    g = {"hubs": hubs_graph, "isolated": isolated_graph, "loops": lambda: loop_graph(60, 4, 3)}[name]()
    hs, batch = batch_of(pkg, [g], global_csr)
    for K, terminals in ((3, True), (2, False)):
        check(pkg, hs, batch, K, terminals, starts(batch, K, 3, terminals, 5), *exact(hs, K), 300)


# ---- reproducibility, degenerate counts --------------------------------------------------------------------------------
def test_two_runs_another_stream_and_null_outputs_give_the_same_bytes(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(300, 7, 8), weighted(R.regular_graph(200, 6, 9), "real", 2)])
    A = starts(batch, 5, 7, False, 4)
    lo, hi = exact(hs, 5)
    rc, first = run_balance(pkg, batch, 5, False, A, lo, hi, 300)
    assert rc == 0 and (first["assign"] != A).any()
    runs = [run_balance(pkg, batch, 5, False, A, lo, hi, 300),
            run_balance(pkg, batch, 5, False, A, lo, hi, 300, stream=torch.cuda.Stream()),
            run_balance(pkg, batch, 5, False, A, lo, hi, 300, optional=False)]
    for i, (rc, other) in enumerate(runs):
        assert rc == 0
        for k in first:
            if i == 2 and k in ("best_iter", "moves", "repairs", "feasible"):
                assert (other[k] == GARBAGE).all()
            else:
                assert other[k].tobytes() == first[k].tobytes(), (i, k)
    rc, reseeded = run_balance(pkg, batch, 5, False, A, lo, hi, 300, seed=SEED + (1 << 63))
    assert rc == 0 and (reseeded["assign"] != first["assign"]).any()


def test_no_iterations_repair_score_and_pick_and_nothing_movable(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(100, 5, 3), weighted(R.regular_graph(50, 4, 4), "int", 1),
                               nx.complete_graph(3)])                  # n = K under terminals: n_mov = 0
    A = starts(batch, 3, 6, True, 3)
    got = check(pkg, hs, batch, 3, True, A, *exact(hs, 3), 0)
    assert (got["moves"] == 0).all() and (got["best_iter"] == 0).all() and (got["repairs"][:2] > 0).any()
    assert (got["repairs"][2] == 0).all()
    got = check(pkg, hs, batch, 3, True, A, *exact(hs, 3), 50)
    assert (got["moves"][2] == 0).all() and (got["moves"][:2] > 0).all()


# ---- the Python API ------------------------------------------------------------------------------------------------
def test_kway_balanced_search_on_one_graph(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = R.regular_graph(60, 5, 1)
    h = handles_of([g])[0]
    for K, terminals in ((3, True), (2, False)):
        a0 = np.random.RandomState(K).randint(0, K, 60).astype(np.int8)
        if terminals:
            a0[:K] = np.arange(K)
        lo, hi = BR.balanced_bounds(60, K)
        assign, cut = TN.kway_balanced_search(a0.tolist(), g, K, iterations=150, seed=9, terminals=terminals)
        ref = BR.balanced(60, h.rowptr, h.col, h.weight, a0, K, terminals, 0, lo, hi, 150, seed=9)
        assert assign == ref.assign.tolist() and cut == TN.calculate_cut_value(assign, g) and feasible(assign, K, lo, hi)
        default, _cut = TN.kway_balanced_search(a0.tolist(), g, K, seed=9, terminals=terminals)   # 20 n iterations
        assert default == BR.balanced(60, h.rowptr, h.col, h.weight, a0, K, terminals, 0, lo, hi, 1200, seed=9).assign.tolist()
        wide = ([10] * K, [40] * K)
        assign, cut = TN.kway_balanced_search(a0.tolist(), g, K, class_sizes=wide, iterations=150, seed=9, terminals=terminals)
        ref = BR.balanced(60, h.rowptr, h.col, h.weight, a0, K, terminals, 0, *wide, 150, seed=9)
        assert assign == ref.assign.tolist() and cut == TN.calculate_cut_value(assign, g)
        free, free_cut = TN.kway_balanced_search(a0.tolist(), g, K, class_sizes=([0] * K, [60] * K), iterations=150, seed=9,
                                                 terminals=terminals)
        assert (free, free_cut) == TN.kway_tabu_search(a0.tolist(), g, K, iterations=150, seed=9, terminals=terminals)


def edge_index_of(g, offset=0):
    e = np.asarray(list(g.edges()), np.int64) + offset
    return np.concatenate([e, e[:, ::-1]]).T


def cuts_f64(ei, w, ptr, part):
    out = []
    for g in range(len(ptr) - 1):
        inside = (ei[0] >= ptr[g]) & (ei[0] < ptr[g + 1])
        ww = np.ones(inside.sum()) if w is None else np.asarray(w, np.float64)[inside]
        out.append(float(((part[ei[0][inside]] != part[ei[1][inside]]) * ww).sum() / 2))
    return np.asarray(out)


@pytest.mark.parametrize("K", (2, 3))
def test_maxcut_solve_within_bounds(pkg, K):
    from gcn_max_cut_amd import maxcut
    g0, g1 = R.regular_graph(60, 5, K), R.regular_graph(61 + K % 2, 4, K + 1)
    ei = np.concatenate([edge_index_of(g0), edge_index_of(g1, 60)], axis=1)
    ptr = np.asarray([0, 60, 60 + g1.number_of_nodes()], np.int64)
    kw = dict(number_classes=K, hidden_dim=8, epochs=20, learning_rate=2e-2, samples=6, anneal_sweeps=10, seed=4)
    plain = maxcut.solve(ei, ptr, **kw)
    none = maxcut.solve(ei, ptr, **kw, class_sizes=None, balance_iterations=7)
    assert plain.unconstrained_cut is None and none.unconstrained_cut is None
    for name in ("partition", "cut", "trained_cut", "rounded_cut", "ptr"):
        assert getattr(none, name).cpu().numpy().tobytes() == getattr(plain, name).cpu().numpy().tobytes(), name
    res = maxcut.solve(ei, ptr, **kw, class_sizes="balanced", balance_iterations=300)
    part, cut = res.partition.cpu().numpy(), res.cut.cpu().numpy()
    assert res.unconstrained_cut.cpu().numpy().tobytes() == plain.cut.cpu().numpy().tobytes()
    for g in range(2):
        n = int(ptr[g + 1] - ptr[g])
        assert feasible(part[ptr[g]:ptr[g + 1]], K, *BR.balanced_bounds(n, K)), g
    assert np.array_equal(cut.astype(np.float64), cuts_f64(ei, None, ptr, part))
    for name in ("trained_cut", "rounded_cut", "ptr"):
        assert getattr(res, name).cpu().numpy().tobytes() == getattr(plain, name).cpu().numpy().tobytes(), name
    again = maxcut.solve(ei, ptr, **kw, class_sizes=maxcut.balanced_sizes(ptr, K), balance_iterations=300)
    assert again.partition.cpu().numpy().tobytes() == part.tobytes()
    with_tabu = maxcut.solve(ei, ptr, **kw, class_sizes="balanced", balance_iterations=300, tabu_iterations=100)
    assert with_tabu.annealed_cut is not None and (with_tabu.unconstrained_cut >= with_tabu.annealed_cut).all()
    assert with_tabu.partition.cpu().numpy().tobytes() == part.tobytes()   # the stage starts from the annealed candidates


def test_maxcut_solve_finds_the_bridge_as_a_balanced_minimum_cut(pkg):
    from gcn_max_cut_amd import maxcut
    g = bridge_graph(1)
    ei = edge_index_of(g)
    w = -np.ones(ei.shape[1], np.float32)
    res = maxcut.solve(ei, num_nodes=16, edge_weight=w, number_classes=2, hidden_dim=8, epochs=5, learning_rate=1e-2,
                       samples=4, anneal_sweeps=0, seed=1, class_sizes="balanced")
    part = res.partition.cpu().numpy()
    assert res.cut.cpu().tolist() == [-1.0] and cuts_f64(ei, w, [0, 16], part).tolist() == [-1.0]
    assert (part == 0).sum() == 8 and len(set(part[:8])) == 1 and len(set(part[8:])) == 1
    assert res.unconstrained_cut.cpu().item() >= -1.0
    hs, batch = batch_of(pkg, [bridge_graph()])
    got = check(pkg, hs, batch, 2, False, bridge_starts(), *exact(hs, 2), 320, seed=1)
    assert got["cut_all"].tolist() == [[-1.0] * 4]
