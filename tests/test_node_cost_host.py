"""CPU tests of the per-node class costs (include/gcnmaxcut.h, the ``_c`` entry points): the
restatement tests/node_cost_ref.py against the existing ones with no and with an all-zero cost, the rounding's guarantee
and the descent's local optimality for the objective cut - cost, the exact QUBO and Ising mappings, the doors' optimum
on small instances through the numpy restatement, and every argument error - raised before any HIP call, so all of it
runs without a GPU."""
import ctypes as C

import numpy as np
import pytest

from tests import anneal_ref as AR
from tests import kway_search_ref as KS
from tests import node_cost_ref as NC
from tests import plain_ref as PR
from tests import rounding_ref as RO
from tests import seeded_ref as SR
from tests.test_rounding_host import SLACK

F32 = np.float32


def graphs():
    """(n, rowptr, col, w): rings with chords of 9..40 nodes, unit and integer weights, and the centre-2 star."""
    out = []
    for i, n in enumerate((9, 17, 40)):
        n, rp, cl = PR.ring_with_chords(n, 60 + i)
        out.append((n, rp, cl, None))
        out.append((n, rp, cl, PR.integer_weights(n, rp, cl, 3 + i)))
    n, rp, cl = PR.star_centre2(70)
    out.append((n, rp, cl, None))
    return out


# ---- no cost and an all-zero cost are the existing restatements -----------------------------------------------------------
@pytest.mark.parametrize("K,terminals", [(2, False), (3, True), (8, False), (4, True)])
def test_zero_cost_is_the_existing_restatement_byte_for_byte(K, terminals):
    first = PR.first_of(K, terminals)
    for gi, (n, rp, cl, w) in enumerate(graphs()):
        if n < max(first, 1):
            continue
        zeros = np.zeros((n, K), F32)
        P = PR.softmax_rows(n, K, 11 * K + gi)
        key = SR.keys(5, [gi])[0]
        want = PR.sample(n, rp, cl, w, P, key, 6, first)
        for cost in (None, zeros):
            got = NC.sample(n, rp, cl, w, cost, P, key, 6, first)
            assert all(np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes() for k in want), (K, gi)
        A = np.random.RandomState(gi).randint(0, K, (3, n)).astype(np.int8)
        A[:, :first] = np.arange(first)
        scale = 1.0 if w is None else float(np.mean(w))
        inv_t = AR.schedule(5, scale=scale)
        want = PR.anneal(n, rp, cl, w, A, K, first, inv_t, AR.levels(), 77, 100)
        for cost in (None, zeros):
            got = NC.anneal(n, rp, cl, w, cost, A, K, first, inv_t, AR.levels(), 77, 100)
            for k in want:
                assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), (K, gi, k)
        want = PR.restate_round(n, rp, cl, w, P, K, first, 100)
        for cost in (None, zeros):
            got = NC.restate_round(n, rp, cl, w, cost, P, K, first, 100)
            assert (got["a0"] == want["a0"]).all() and (got["a1"] == want["a1"]).all() and got["sweeps"] == want["sweeps"]
            assert float(got["cut"]) == PR.cut(rp, cl, w, want["a1"])
        if terminals and n >= K:      # and, with terminals, the older ones
            assert (NC.round_conditional(n, rp, cl, w, None, P, K, K) == RO.round_sequential(n, rp, cl, w, P, K)).all()
            ref, snap, sw = KS.anneal(n, rp, cl, w, A, K, inv_t, AR.levels(), 77, 100)
            got = NC.anneal(n, rp, cl, w, zeros, A, K, K, inv_t, AR.levels(), 77, 100)
            assert (got["assign"] == ref).all() and (got["snap"] == snap).all() and (got["sweeps"] == sw).all()


def test_the_fp32_score_is_the_float64_objective_for_integer_data():
    rng = np.random.RandomState(1)
    for n, rp, cl, w in graphs():
        for K in (2, 3, 8):
            cost = rng.randint(-3, 4, (n, K)).astype(F32)
            a = rng.randint(0, K, n).astype(np.int8)
            assert float(NC.score(n, rp, cl, w, cost, a, K)) == NC.objective64(rp, cl, w, cost, a, K)
            a[0] = K + 1                                   # a byte of no class adds no cost and differs from every class
            assert float(NC.score(n, rp, cl, w, cost, a, K)) == NC.objective64(rp, cl, w, cost, a, K)


# ---- the guarantee and the local optimum, on drawn tiny graphs ---------------------------------------------------------
def tiny_cases():
    rng = np.random.RandomState(7)
    for i in range(24):
        n = 3 + i % 8                                      # 3..10
        K = 2 + i % 2
        _n, rp, cl = PR.ring_with_chords(n, 200 + i)
        w = PR.integer_weights(n, rp, cl, i) if i % 3 else None
        cost = rng.randint(-3, 4, (n, K)).astype(F32)
        P = PR.softmax_rows(n, K, 300 + i)
        yield n, rp, cl, w, cost, P, K, (K if i % 4 == 0 and n >= K else 0)


def test_rounded_objective_is_not_below_the_expected_objective():
    margins = []
    for n, rp, cl, w, cost, P, K, first in tiny_cases():
        a0 = NC.round_conditional(n, rp, cl, w, cost, P, K, first)
        expected = NC.expected_objective(n, rp, cl, w, cost, P, K, first)
        W_abs = RO.abs_weight(rp, cl, w)
        got = NC.objective64(rp, cl, w, cost, a0, K)
        print(f"n {n} K {K} first {first}: rounded {got} expected {expected:.6f}")
        assert got >= expected - SLACK * W_abs, (n, K, first, got, expected)
        margins.append(got - expected)
    assert max(margins) > 0


def test_after_a_converged_descent_no_single_move_raises_the_objective():
    for n, rp, cl, w, cost, P, K, first in tiny_cases():
        a0 = NC.round_conditional(n, rp, cl, w, cost, P, K, first)
        a1, sweeps = NC.descent(n, rp, cl, w, cost, a0, K, first, 100)
        assert sweeps < 100                               # converged: the last sweep moved nothing
        assert NC.objective64(rp, cl, w, cost, a1, K) >= NC.objective64(rp, cl, w, cost, a0, K)
        assert NC.best_single_move_gain(n, rp, cl, w, cost, a1, K, first) <= 0.0
        base = NC.objective64(rp, cl, w, cost, a1, K)     # and by recount, move by move
        for v in range(first, n):
            for k in range(K):
                b = a1.copy()
                b[v] = k
                assert NC.objective64(rp, cl, w, cost, b, K) <= base, (n, K, v, k)


# ---- the doors ---------------------------------------------------------------------------------------------------------
def test_mapping_identities_are_exact_for_integer_data():
    rng = np.random.RandomState(3)
    for seed, n in NC.DOOR_INSTANCES:
        n, edges, quad, lin = NC.drawn_instance(seed, n)
        rq = NC.qubo_to_maxcut(n, edges, quad, lin)
        ri = NC.ising_to_maxcut(n, edges, quad, lin)
        for _ in range(50):
            x = rng.randint(0, 2, n)
            assert -NC.objective64(*rq[:3], rq[3], x, 2) == NC.qubo_energy(edges, quad, lin, x)
            assert -float(NC.score(n, *rq, x.astype(np.int8), 2)) == NC.qubo_energy(edges, quad, lin, x)
            s = 1 - 2 * x                                  # class 0 is s = +1
            assert float(np.sum(quad)) - NC.objective64(*ri[:3], ri[3], x, 2) == NC.ising_energy(edges, quad, lin, s)


@pytest.mark.parametrize("seed,n", NC.DOOR_INSTANCES)
def test_the_restated_search_reaches_the_brute_force_optimum(seed, n):
    n, edges, quad, lin = NC.drawn_instance(seed, n)
    rp, cl, w, cost = NC.qubo_to_maxcut(n, edges, quad, lin)
    best, _ = NC.brute_force_min(n, lambda b: NC.qubo_energy(edges, quad, lin, b))
    obj, _a = NC.search(n, rp, cl, w, cost, 2, 8, 30, seed, float(np.abs(w).mean()))
    assert -obj == best
    rp, cl, w, cost = NC.ising_to_maxcut(n, edges, quad, lin)
    best, _ = NC.brute_force_min(n, lambda b: NC.ising_energy(edges, quad, lin, [1 - 2 * x for x in b]))
    obj, _a = NC.search(n, rp, cl, w, cost, 2, 8, 30, seed, float(np.abs(w).mean()))
    assert float(np.sum(quad)) - obj == best


# ---- argument errors, before any HIP call ------------------------------------------------------------------------------
TRIANGLE = np.array([[0, 1, 1, 2, 0, 2], [1, 0, 2, 1, 2, 0]], np.int64)
KW = dict(hidden_dim=4, epochs=1, learning_rate=0.1)


def test_solve_refuses_a_bad_node_cost_before_anything_is_built(built):
    mc = built.maxcut
    zeros = np.zeros((3, 2))
    for bad in (np.zeros((4, 2)), np.zeros((3, 3)), np.zeros(3), np.zeros((3, 2), np.int64)):
        with pytest.raises(ValueError, match="node_cost"):
            mc.solve(TRIANGLE, num_nodes=3, node_cost=bad, **KW)
    for value in (np.nan, np.inf, 1e300):                  # (1e300 is not finite in float32)
        bad = zeros.copy()
        bad[1, 1] = value
        with pytest.raises(ValueError, match="finite"):
            mc.solve(TRIANGLE, num_nodes=3, node_cost=bad, **KW)
    import torch
    with pytest.raises(ValueError, match="node_cost"):
        mc.solve(TRIANGLE, ptr=np.array([0, 3]), node_cost=torch.zeros(2, 2), **KW)
    with pytest.raises(NotImplementedError, match="tabu"):
        mc.solve(TRIANGLE, num_nodes=3, node_cost=zeros, tabu_iterations=5, **KW)
    with pytest.raises(NotImplementedError, match="class_sizes"):
        mc.solve(TRIANGLE, num_nodes=3, node_cost=zeros, class_sizes="balanced", **KW)
    with pytest.raises(NotImplementedError, match="fixed"):
        mc.solve(TRIANGLE, num_nodes=3, node_cost=zeros, fixed=(np.array([0, 1]), np.array([0, 1])), **KW)
    with pytest.raises(NotImplementedError, match="large"):
        mc.solve_large(TRIANGLE, num_nodes=3, node_cost=zeros, **KW)
    with pytest.raises(NotImplementedError, match="large"):
        mc.solve_large_batch(None, node_cost=zeros, **KW)
    with pytest.raises(ValueError, match="field"):
        mc.solve_ising(TRIANGLE, num_nodes=3, field=np.zeros(4), **KW)
    with pytest.raises(ValueError, match="quadratic"):
        mc.solve_qubo(TRIANGLE, num_nodes=3, quadratic=np.zeros(5), **KW)
    with pytest.raises(ValueError, match="finite"):
        mc.solve_qubo(TRIANGLE, num_nodes=3, linear=np.array([0.0, np.nan, 0.0]), **KW)


def test_the_large_engine_takes_no_node_cost(built):
    import torch
    with pytest.raises(NotImplementedError, match="node_cost"):
        built.engine.LargeInstanceEngine([], 4, 2, torch.device("cpu"), node_cost=torch.zeros(0, 2))


def _codes(call, twin):
    """Both calls on the same arguments give the same status code; returns it."""
    a, b = call(), twin()
    assert a == b, (a, b)
    return a


def test_the_c_entry_points_check_arguments_as_their_twins_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some = C.c_void_p(None), C.c_void_p(4096)        # (never dereferenced: the calls fail first)
    fields = dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096, gcol=4096, dinv=4096)
    batch = lambda **kw: C.byref(hip.GmcBatch(**{**fields, **kw}))
    model = lambda **kw: C.byref(hip.GmcModel(**{**dict(N=100, F=8, K=3, W1=4096, b1=4096, W2=4096, b2=4096), **kw}))
    assert {"gmc_round_conditional_c_f32", "gmc_kway_decode_sample_seeded_c_f32", "gmc_kway_refine_anneal_c_f32",
            "gmc_inst_forward_c", "gmc_inst_train_fwd_bwd_c", "gmc_row_weight_sums_f32"} <= set(hip.SYMBOLS)

    def rounding(b, cost, K=3, t=1, P=some, sweeps_max=10, cut=some):
        tail = (some, some, some, sweeps_max, some, cut, some, some, None)
        return _codes(lambda: lib.gmc_round_conditional_c_f32(b, P, K, t, cost, *tail),
                      lambda: lib.gmc_round_conditional_t_f32(b, P, K, t, *tail))

    def sampler(b, cost, K=3, t=1, P=some, iters=4, cut=some):
        tail = (some, iters, some, cut, some, some, some, None)
        return _codes(lambda: lib.gmc_kway_decode_sample_seeded_c_f32(b, P, K, t, cost, *tail),
                      lambda: lib.gmc_kway_decode_sample_seeded_t_f32(b, P, K, t, *tail))

    def annealing(b, cost, K=3, t=1, P=some, cands=4, cut=some):
        tail = (P, some, some, cands, some, some, 5, some, 1, 10, cut, some, some, some, some, some, None)
        return _codes(lambda: lib.gmc_kway_refine_anneal_c_f32(b, K, t, cost, *tail),
                      lambda: lib.gmc_kway_refine_anneal_t_f32(b, K, t, *tail))

    for f, shape in ((rounding, dict(sweeps_max=-1)), (sampler, dict(iters=0)), (annealing, dict(cands=0))):
        for cost in (null, some):                           # node_cost is optional and never checked
            assert f(None, cost) == -1
            assert f(batch(), cost, P=null) == -1
            assert f(batch(), cost, cut=null) == -1
            assert f(batch(abi=100), cost) == -8
            assert f(batch(abi=100), cost, P=null) == -1
            assert f(batch(lcol=None), cost, K=9) == -1
            for K in (0, 1, 9):
                assert f(batch(), cost, K=K, **shape) == -3
            assert f(batch(), cost, **shape) == -2
            assert f(batch(), cost, t=2) == -2
            assert f(batch(n_max=2), cost, t=1) == -6
            assert f(batch(n_max=0), cost, t=0) == -6
            assert f(batch(n_max=65536), cost, t=0) == -6
            assert f(batch(B=0, R=0, n_max=0), cost) == 0

    def instance(train):
        def f(b, m, cost, t=1, ws=some, ws_bytes=1 << 30, P=some, grad=some):
            if train:
                return _codes(lambda: lib.gmc_inst_train_fwd_bwd_c(b, m, t, cost, 1.0, ws, ws_bytes, P, some, some, grad, None),
                              lambda: lib.gmc_inst_train_fwd_bwd_t(b, m, t, 1.0, ws, ws_bytes, P, some, some, grad, None))
            return _codes(lambda: lib.gmc_inst_forward_c(b, m, t, cost, 1.0, ws, ws_bytes, P, some, some, None),
                          lambda: lib.gmc_inst_forward_t(b, m, t, 1.0, ws, ws_bytes, P, some, some, None))
        return f

    for train in (False, True):
        f = instance(train)
        for cost in (null, some):
            assert f(None, model(), cost) == -1
            assert f(batch(), None, cost) == -1
            assert f(batch(abi=100), model(), cost) == -8
            assert f(batch(), model(abi=100), cost) == -8
            for K in (1, 9):
                assert f(batch(), model(K=K), cost) == -3
            assert f(batch(), model(), cost, t=2) == -2
            assert f(batch(), model(), cost, ws=null) == -1
            assert f(batch(), model(), cost, P=null) == -1
            assert f(batch(), model(), cost, ws_bytes=16) == -5
            assert f(batch(n_max=2), model(), cost, t=1) == -6
            assert f(batch(n_max=4097), model(), cost, t=0) == -6
            if train:
                assert f(batch(), model(), cost, grad=null) == -1
    assert lib.gmc_row_weight_sums_f32(5, null, some, null, some, None) == -1
    assert lib.gmc_row_weight_sums_f32(5, some, some, null, null, None) == -1
    assert lib.gmc_row_weight_sums_f32(-1, some, some, null, some, None) == -2
    assert lib.gmc_row_weight_sums_f32(5, some, null, null, some, None) == -1
    assert lib.gmc_row_weight_sums_f32(0, some, null, null, some, None) == 0
