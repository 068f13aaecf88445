"""CPU checks of the two chain searches with per-node class costs (include/gcnmaxcut.h, gmc_kway_tabu_c_f32 and
gmc_kway_balance_c_f32): the restatement tests/chain_cost_ref.py against the twins' restatements,
its identities on integer data, brute force on tiny instances (as max-K-cut with costs under size bounds, and as
cardinality-constrained QUBOs), the contraction identity of pins with costs, the status codes of the two entry points,
the code object's notes, and the argument errors of the Python doors."""
import ctypes as C
import itertools
import subprocess

import numpy as np
import pytest

from oracle import ref_dense as R
from tests import balanced_ref as BR
from tests import chain_cost_ref as CC
from tests import node_cost_ref as NR
from tests import tabu_ref as TR
from tests import util
from tests.test_node_cost_host import _codes
from tests.test_refine_host import gnp_graph, handles_of, loop_graph
from tests.test_tabu_host import NULL, SOME, int_weighted, mk, start

F = np.float32

CHAINS = {   # graph, K, terminals, iterations, tenure
    "regular_k2": (lambda: R.regular_graph(40, 5, 1), 2, False, 120, (3, 0, 10)),
    "signed_k3_t": (lambda: int_weighted(R.regular_graph(36, 4, 2), 2, signed=True), 3, True, 120, (3, 0, 10)),
    "loops_k4": (lambda: loop_graph(30, 4, 3), 4, False, 100, (1, 3, 7)),
    "gnp_k8_t": (lambda: int_weighted(gnp_graph(30, 0.3, 4), 4), 8, True, 100, (0, 0, 0)),
}


def integer_cost(n, K, seed):
    return np.random.RandomState(seed).randint(-3, 4, (n, K)).astype(F)


def tight_bounds(n, K):
    return BR.balanced_bounds(n, K)


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_without_a_cost_and_with_zeros_the_restatement_is_the_twins(name):
    make, K, t, iters, tenure = CHAINS[name]
    h = handles_of([make()])[0]
    a0 = start(h.n, K, t, 5)
    args = (h.n, h.rowptr, h.col, h.weight)
    want = TR.tabu(*args, a0, K, t, 1, iters, *tenure, seed=9)
    lo, hi = tight_bounds(h.n, K)
    bad = np.zeros(h.n, np.int8)                                        # one class: the repair runs
    bad[:K if t else 0] = np.arange(K if t else 0)
    for cost in (None, np.zeros((h.n, K), F)):
        got = CC.tabu(*args, cost, a0, K, t, 1, iters, *tenure, seed=9)
        assert got.assign.tobytes() == want.assign.tobytes() and got[1:4] == want[1:4]
        for a in (a0, bad):
            w = BR.balanced(*args, a, K, t, 2, lo, hi, iters, *tenure, seed=9)
            g = CC.balanced(*args, cost, a, K, t, 2, lo, hi, iters, *tenure, seed=9)
            assert g.assign.tobytes() == w.assign.tobytes() and g[1:5] == w[1:5]


@pytest.mark.parametrize("name", sorted(CHAINS))
def test_the_objective_of_the_result_is_the_inputs_plus_best(name):
    """Integer weights and costs: every sum is exact, so cut - cost of the snapshot is the input's (for the balanced
    search: the repaired state's, which zero iterations return) plus `best`; and no snapshot leaves the bounds."""
    make, K, t, iters, tenure = CHAINS[name]
    h = handles_of([make()])[0]
    args = (h.n, h.rowptr, h.col, h.weight)
    cost = integer_cost(h.n, K, 7)
    obj = lambda a: NR.objective64(h.rowptr, h.col, h.weight, cost, a, K)
    a0 = start(h.n, K, t, 6)
    res = CC.tabu(*args, cost, a0, K, t, 0, iters, *tenure, seed=3)
    assert obj(res.assign) == obj(a0) + float(res.best) and res.best >= 0
    assert (res.assign[:K if t else 0] == a0[:K if t else 0]).all()
    other = CC.tabu(*args, None, a0, K, t, 0, iters, *tenure, seed=3)
    assert res.best_it > 0 and (res.assign != other.assign).any()       # (the cost is not a bystander)
    lo, hi = tight_bounds(h.n, K)
    bad = np.zeros(h.n, np.int8)
    bad[:K if t else 0] = np.arange(K if t else 0)
    for a in (a0, bad):
        repaired = CC.balanced(*args, cost, a, K, t, 0, lo, hi, 0, *tenure, seed=3)
        for its in (1, 7, iters):
            res = CC.balanced(*args, cost, a, K, t, 0, lo, hi, its, *tenure, seed=3)
            s, _m = BR.sizes(res.assign, K, 0)
            assert (s >= lo).all() and (s <= hi).all()
            assert res.repairs == repaired.repairs
            assert obj(res.assign) == obj(repaired.assign) + float(res.best)
    loose = CC.balanced(*args, cost, a0, K, t, 0, np.zeros(K, int), np.full(K, h.n), iters, *tenure, seed=3)
    plain = CC.tabu(*args, cost, a0, K, t, 0, iters, *tenure, seed=3)
    assert loose.assign.tobytes() == plain.assign.tobytes() and loose[1:3] == plain[1:3] and loose.repairs == 0


def test_a_negative_zero_cost_gives_the_bytes_of_a_positive_zero():
    """The header's canonicalisation: the table takes sum + (+0.0), so a cost of -0.0 under a class without
    neighbours leaves no trace.  (In the restatement the compares are float compares either way; the test pins that the
    table itself holds no -0.0, which is what the device's ordered key relies on.)"""
    h = handles_of([R.regular_graph(20, 3, 2)])[0]
    K = 4
    a0 = np.zeros(20, np.int8)                                          # classes 1..3 have no neighbours anywhere
    neg = np.full((20, K), -0.0, F)
    W = CC.class_sums(20, h.rowptr, h.col, h.weight, a0, K, neg)
    assert not np.signbit(W).any() and (W[:, 1:] == 0).all()
    a = CC.tabu(20, h.rowptr, h.col, None, neg, a0, K, False, 0, 60, seed=1)
    b = CC.tabu(20, h.rowptr, h.col, None, np.zeros((20, K), F), a0, K, False, 0, 60, seed=1)
    assert a.assign.tobytes() == b.assign.tobytes() and a[1:4] == b[1:4]


# ---- brute force ------------------------------------------------------------------------------------------------------
def best_of_chains(n, rowptr, col, w, cost, K, lo, hi, seed):
    """The best objective (float64) of 8 restatement chains of 20 n iterations from random starts."""
    A = np.random.RandomState(900 + seed).randint(0, K, (8, n)).astype(np.int8)
    res = [CC.balanced(n, rowptr, col, w, cost, A[i], K, False, i, lo, hi, 20 * n, seed=seed) for i in range(8)]
    for r in res:
        s = np.bincount(r.assign, minlength=K)
        assert (s >= lo).all() and (s <= hi).all()
    return max(NR.objective64(rowptr, col, w, cost, r.assign, K) for r in res)


@pytest.mark.parametrize("seed,n,K", CC.BRUTE_INSTANCES, ids=lambda v: str(v))
def test_the_restatement_reaches_the_optimum_under_size_bounds(seed, n, K):
    rowptr, col, w, cost, _edges, _quad, _lin = CC.drawn_instance(seed, n, K)
    lo, hi = tight_bounds(n, K)
    assert best_of_chains(n, rowptr, col, w, cost, K, lo, hi, seed) == CC.brute_force_max(n, K, rowptr, col, w, cost, lo, hi)


def qubo_bounds(n):
    """Between a third and a half of the variables set."""
    return n // 3, n // 2


@pytest.mark.parametrize("seed,n,K", CC.BRUTE_INSTANCES, ids=lambda v: str(v))
def test_cardinality_constrained_qubos_reach_the_brute_force_minimum(seed, n, K):
    """The same graphs read as QUBOs (node_cost_ref.qubo_to_maxcut: class 1 is x = 1, E = -obj) with lo <= sum x <= hi."""
    _rp, _cl, _w, _cost, edges, quad, lin = CC.drawn_instance(seed, n, K)
    rowptr, col, w, cost = NR.qubo_to_maxcut(n, edges, quad, lin)
    k_lo, k_hi = qubo_bounds(n)
    lo, hi = np.asarray([n - k_hi, k_lo]), np.asarray([n - k_lo, k_hi])
    best = min(NR.qubo_energy(edges, quad, lin, x) for x in itertools.product((0, 1), repeat=n) if k_lo <= sum(x) <= k_hi)
    assert -best_of_chains(n, rowptr, col, w, cost, 2, lo, hi, seed) == best


# ---- pins with costs --------------------------------------------------------------------------------------------------
def test_contraction_carries_the_costs_exactly():
    """objective_contracted + fixed_cut - fixed_cost == objective_original for every partition that honours the pins."""
    from gcn_max_cut_amd import graph as G
    K, n = 3, 9
    g = int_weighted(gnp_graph(n, 0.5, 11), 3, signed=True)
    h = handles_of([g])[0]
    cost = integer_cost(n, K, 12)
    nodes, classes = np.asarray([7, 0, 4, 2]), np.asarray([0, 1, 2, 1])
    ct = G.contract(h, nodes, classes, K)
    cost_c, fixed_cost = ct.contract_cost(cost)
    hc = ct.handle
    assert cost_c.shape == (hc.n, K) and cost_c.dtype == F and (cost_c[:K] == 0).all()
    assert fixed_cost == cost[7, 0] + cost[0, 1] + cost[4, 2] + cost[2, 1] and isinstance(fixed_cost, np.float32)
    free = np.flatnonzero(~ct.pinned)
    assert (cost_c[ct.node_map[free]] == cost[free]).all()
    seen = 0
    for tail in itertools.product(range(K), repeat=hc.n - K):
        part_c = np.asarray(list(range(K)) + list(tail))
        part = ct.lift(part_c)
        assert (part[nodes] == classes).all()
        left = NR.objective64(hc.rowptr, hc.col, hc.weight, cost_c, part_c, K) + float(ct.fixed_cut) - float(fixed_cost)
        assert left == NR.objective64(h.rowptr, h.col, h.weight, cost, part, K)
        seen += 1
    assert seen == K ** (n - 4)


# ---- the entry points without a GPU -----------------------------------------------------------------------------------
def test_the_status_codes_are_the_twins(built):
    hip = built.hip
    lib = hip.load()
    assert {"gmc_kway_tabu_c_f32", "gmc_kway_balance_c_f32"} <= set(hip.SYMBOLS)

    def tabu(batch, cost, K=4, t=1, cands=4, assign=SOME, iterations=10, base=3, span=0, div=10, cut_all=SOME,
             best_assign=SOME, best_cut=SOME, best_idx=SOME, size_lo=None):
        b = None if batch is None else C.byref(batch)
        tail = (cands, assign, iterations, base, span, div, 7, cut_all, best_assign, best_cut, best_idx, SOME, SOME, None)
        return _codes(lambda: lib.gmc_kway_tabu_c_f32(b, K, t, cost, *tail), lambda: lib.gmc_kway_tabu_f32(b, K, t, *tail))

    def balance(batch, cost, K=4, t=1, cands=4, assign=SOME, iterations=10, base=3, span=0, div=10, cut_all=SOME,
                best_assign=SOME, best_cut=SOME, best_idx=SOME, size_lo=SOME):
        b = None if batch is None else C.byref(batch)
        tail = (cands, assign, size_lo, SOME, iterations, base, span, div, 7, cut_all, best_assign, best_cut, best_idx,
                SOME, SOME, SOME, SOME, None)
        return _codes(lambda: lib.gmc_kway_balance_c_f32(b, K, t, cost, *tail),
                      lambda: lib.gmc_kway_balance_f32(b, K, t, *tail))

    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096)
    for f in (tabu, balance):
        for cost in (NULL, SOME):                                       # node_cost is never tested
            assert f(None, cost) == -1
            for name in ("assign", "cut_all", "best_assign", "best_cut", "best_idx"):
                assert f(mk(hip), cost, **{name: NULL}) == -1, name
            assert f(mk(hip, abi=100), cost) == -8 and f(mk(hip, abi=100), cost, assign=NULL) == -1
            for field in ("goff", "rowptr", "lcol"):
                assert f(mk(hip, **{field: None}), cost) == -1
                assert f(mk(hip, abi=100, **{field: None}), cost) == -8
            for K in (1, 9, 0):
                assert f(mk(hip), cost, K=K) == -3 and f(mk(hip), cost, K=K, cands=0) == -3
                assert f(mk(hip, lcol=None), cost, K=K) == -1
            for kw in (dict(cands=0), dict(iterations=-1), dict(base=-1), dict(span=-1), dict(div=-1), dict(t=2)):
                assert f(mk(hip), cost, **kw) == -2, kw
                assert f(mk(hip, n_max=3), cost, **kw) == -2
            assert f(mk(hip, B=-1), cost) == -2
            assert f(mk(hip, n_max=3), cost) == -6 and f(mk(hip, n_max=4097), cost) == -6
            assert f(mk(hip, n_max=0), cost, t=0) == -6
            for K in range(2, 9):
                assert f(empty, cost, K=K, t=0) == 0 and f(empty, cost, K=K, t=1) == 0
    assert balance(mk(hip), SOME, size_lo=NULL) == -1 and balance(mk(hip, abi=100), SOME, size_lo=NULL) == -1
    # fits / shape are unchanged and answer for the new calls too
    for K in (2, 8):
        for kw in (dict(n_max=100, nnz_max=700), dict(n_max=4096, nnz_max=28672), dict(n_max=4097)):
            b = C.byref(hip.GmcBatch(**kw))
            assert lib.gmc_kway_tabu_shape(b, K) == lib.gmc_kway_balance_shape(b, K)
            assert lib.gmc_kway_tabu_fits(b, K) == lib.gmc_kway_balance_fits(b, K) == int(kw["n_max"] <= 4096)


def test_the_header_states_the_two_rules():
    import os
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcnmaxcut.h")).read()
    for text in ("int gmc_kway_tabu_c_f32(", "int gmc_kway_balance_c_f32(", "Negative zero.", "W[v][k] = sum + (+0.0f)",
                 "Costs must be finite"):
        assert text in header, text


def test_every_cost_instantiation_is_in_the_code_object_and_none_uses_scratch(built):
    """The code object's own notes: no cost kernel has a private segment or spills a vector register, K = 2..8."""
    names = util.kernel_symbols(built.hip.LIB_PATH)
    for K in range(2, 9):
        assert sum(f"tabu_cost_kernel<{K}>" in s for s in names) == 1, K
        assert sum(f"balance_cost_kernel<{K}>" in s for s in names) == 1, K
    seen = 0
    for co in util.gfx950_code_objects(built.hip.LIB_PATH):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if "_cost_kernel" not in entry or ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            name = fields.get(".name", "")
            if "tabu_cost_kernel" not in name and "balance_cost_kernel" not in name:
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, name
            assert int(fields[".vgpr_spill_count"]) == 0, name
    assert seen == 14


# ---- the Python doors -------------------------------------------------------------------------------------------------
TRIANGLE = np.asarray([[0, 1, 1, 2, 2, 0], [1, 0, 2, 1, 0, 2]], np.int64)
KW = dict(hidden_dim=4, epochs=1, learning_rate=0.01)


def test_solve_keeps_its_refusals_and_names_solve_batch():
    from gcn_max_cut_amd import maxcut as mc
    zeros = np.zeros((3, 2), F)
    for word, extra in (("tabu", dict(tabu_iterations=5)), ("class_sizes", dict(class_sizes="balanced")),
                        ("fixed", dict(fixed=(np.array([0, 1]), np.array([0, 1]))))):
        with pytest.raises(NotImplementedError, match=word) as err:
            mc.solve(TRIANGLE, num_nodes=3, node_cost=zeros, **extra, **KW)
        assert "solve_batch(GraphBatch.from_edge_index(" in str(err.value)
    with pytest.raises(NotImplementedError, match="large"):
        mc.solve_large(TRIANGLE, num_nodes=3, node_cost=zeros, tabu_iterations=5, **KW)
    with pytest.raises(ValueError, match="class_sizes with fixed"):     # node weights stay out of scope
        mc.solve_batch(None, node_cost=zeros, class_sizes="balanced", fixed=(np.array([0, 1]), np.array([0, 1])), **KW)
    assert "fixed_cost" in mc.MaxCutResult.__dataclass_fields__


def test_the_doors_refuse_on_the_host():
    """Before the device is touched: none of these needs a GPU."""
    from gcn_max_cut_amd import maxcut as mc
    with pytest.raises(ValueError, match="cardinality"):
        mc.solve_qubo(TRIANGLE, num_nodes=3, cardinality=1, class_sizes="balanced", **KW)
    with pytest.raises(ValueError, match="cardinality"):
        mc.solve_qubo(TRIANGLE, num_nodes=3, cardinality=1.5, **KW)
    with pytest.raises(ValueError, match="graph 0"):                    # 4 ones of 3 variables
        mc.solve_qubo(TRIANGLE, num_nodes=3, cardinality=4, **KW)
    with pytest.raises(ValueError, match="graph 0"):
        mc.solve_qubo(TRIANGLE, num_nodes=3, cardinality=(2, 1), **KW)
    with pytest.raises(ValueError, match="graph 0"):
        mc.solve_qubo(TRIANGLE, num_nodes=3, class_sizes=([2, 2], [3, 3]), **KW)
    with pytest.raises(ValueError, match="graph 0"):
        mc.solve_ising(TRIANGLE, num_nodes=3, class_sizes=([0, 0], [1, 1]), **KW)
    with pytest.raises(ValueError, match="balance_iterations"):
        mc.solve_ising(TRIANGLE, num_nodes=3, class_sizes="balanced", balance_iterations=-1, **KW)
    with pytest.raises(ValueError, match="tabu_iterations"):
        mc.solve_qubo(TRIANGLE, num_nodes=3, tabu_iterations=-1, **KW)
    lo, hi = mc._cardinality_sizes((1, 2), np.asarray([0, 3, 8]))
    assert lo.tolist() == [[1, 1], [3, 1]] and hi.tolist() == [[2, 2], [4, 2]]
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = R.regular_graph(12, 3, 1)
    for bad in (np.zeros((11, 2), F), np.zeros((12, 3), F), np.zeros((12, 2), np.int64), np.full((12, 2), np.nan, F)):
        with pytest.raises(ValueError, match="node_cost"):
            TN.kway_tabu_search([i % 2 for i in range(12)], g, 2, terminals=False, node_cost=bad)
        with pytest.raises(ValueError, match="node_cost"):
            TN.kway_balanced_search([i % 2 for i in range(12)], g, 2, terminals=False, node_cost=bad)
