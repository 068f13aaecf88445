"""GPU tests of the two chain searches with per-node class costs (gmc_kway_tabu_c_f32, gmc_kway_balance_c_f32 and the
Python layers above them) against tests/chain_cost_ref.py: `assign`, `best_iter`, `moves`,
`repairs`, the bits of `cut_all` and the pick, byte for byte.

One batch of several graphs per case (the cost offset r0 * K is tested by every graph but the first): first + 1, 5, 63,
64, 65, 130 and 300 nodes and one graph the launch skips (5 < first with terminals at K = 8; n > n_max otherwise), 5
candidates (the last workgroup of a graph is partial), 3 n iterations.  K = 2, 3, 8 with and without terminals; unit,
signed and full-mantissa weights; integer, full-mantissa, barrier and negative-zero costs.  Every step of the rule is one
fp32 operation and the scores are restated in the device's summation order, so real data is bit for bit too."""
import functools

import numpy as np
import pytest
import torch

from tests import chain_cost_ref as CC
from tests import node_cost_ref as NR
from tests import plain_ref as PR
from tests import util
from tests.test_gpu_node_cost import Raw, csr_of, make_cost, run_anneal
from tests.test_tabu_host import lds_shape

pytestmark = pytest.mark.gpu
F = np.float32
GARBAGE = -5
SEED = 0xFEEDC0DE1234567
TENURE = (3, 0, 10)
CANDS = 5


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def symmetric_weights(n, rp, cl, kind, seed):
    """None for unit weights; signed: +-1; real: full mantissas in 0.1..2 - the same value on both entries of an edge."""
    if kind == "unit":
        return None
    rng = np.random.RandomState(seed)
    draw = {"signed": lambda: float(rng.choice([-1, 1])), "real": lambda: float(F(rng.uniform(0.1, 2.0)))}[kind]
    w, at = np.zeros(len(cl), F), {}
    for v in range(n):
        for e in range(int(rp[v]), int(rp[v + 1])):
            key = (min(v, int(cl[e])), max(v, int(cl[e])))
            if key not in at:
                at[key] = draw()
            w[e] = at[key]
    return w


@functools.lru_cache(maxsize=None)
def mixed_graphs(K, terminals, weights):
    """(csrs, n_max): the batch of the module's docstring.  With terminals at K = 8 the 5-node graph is below `first` and
    skipped; otherwise a 310-node graph is skipped by n_max = 300."""
    first = PR.first_of(K, terminals)
    sizes = [first + 1, 5, 63, 64, 65, 130, 300]
    if not (terminals and 5 < first):
        sizes.insert(3, 310)
    csrs = []
    for i, n in enumerate(sizes):
        if n < 3:                                                       # n = 1: one isolated node (no terminals)
            csrs.append((np.array([0] * (n + 1)), np.zeros(0, np.int64), None))
            continue
        _n, rp, cl = PR.ring_with_chords(n, 30 + i)
        w = symmetric_weights(n, rp, cl, weights, 40 + i)
        csrs.append((rp, cl, w))
    return tuple(csrs), 300


def batch_of(pkg, csrs, n_max=None, global_csr=False):
    batch = Raw(pkg, csrs)
    if n_max is not None:
        batch.c.n_max = n_max
        batch.c.nnz_max = int(max(len(cl) for (rp, cl, _w) in csrs if len(rp) - 1 <= n_max))
    if global_csr:
        batch.c.nnz_max = 1 << 24                                       # (it only sizes the LDS copy: the global path)
    return batch


def starts(batch, K, cands, terminals, seed):
    A = np.random.RandomState(seed).randint(0, K, (cands, batch.R)).astype(np.int8)
    if terminals:
        for lo, hi in batch.spans():
            m = min(K, hi - lo)
            A[:, lo:lo + m] = np.arange(m)
    return A


def exact_bounds(batch, K):
    """floor and ceil of n / K for every class of every graph: (lo, hi) int32 [B, K]."""
    n = batch.sizes
    return (np.repeat((n // K)[:, None], K, 1).astype(np.int32), np.repeat((-(-n // K))[:, None], K, 1).astype(np.int32))


def loose_bounds(batch, K):
    return np.zeros((batch.B, K), np.int32), np.repeat(batch.sizes[:, None], K, 1).astype(np.int32)


def run_chain(pkg, batch, K, terminals, cost, A, iterations, bounds=None, tenure=TENURE, seed=SEED, stream=None):
    """The entry point for the arguments - cost None: the twin without costs; "null": the _c entry point with NULL; an
    array: the _c entry point - on A [cands, R] int8 with every output pre-filled with garbage."""
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    cands = A.shape[0]
    full = lambda shape, value, dtype: torch.full(shape, value, dtype=dtype, device="cuda")
    out = dict(assign=torch.from_numpy(np.ascontiguousarray(A)).cuda(), cut_all=full((batch.B, cands), float("nan"), torch.float32),
               best_assign=full((batch.R,), GARBAGE, torch.int32), best_cut=full((batch.B,), float("nan"), torch.float32),
               best_idx=full((batch.B,), GARBAGE, torch.int32), best_iter=full((batch.B, cands), GARBAGE, torch.int32),
               moves=full((batch.B, cands), GARBAGE, torch.int32))
    tail = [iterations, *tenure, seed, p(out["cut_all"]), p(out["best_assign"]), p(out["best_cut"]), p(out["best_idx"]),
            p(out["best_iter"]), p(out["moves"])]
    head = [cands, p(out["assign"])]
    keep = []
    if bounds is not None:
        keep = [torch.from_numpy(np.ascontiguousarray(b, np.int32)).cuda() for b in bounds]
        head += [p(keep[0]), p(keep[1])]
        out["repairs"] = full((batch.B, cands), GARBAGE, torch.int32)
        out["feasible"] = full((batch.B,), GARBAGE, torch.int32)
        tail += [p(out["repairs"]), p(out["feasible"])]
    name = "gmc_kway_tabu" if bounds is None else "gmc_kway_balance"
    dev_cost = None if cost is None or isinstance(cost, str) else torch.from_numpy(np.ascontiguousarray(cost, F)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()):
        if cost is None:
            rc = getattr(lib, name + "_f32")(batch.ref(), K, int(terminals), *head, *tail, hip.stream())
        else:
            rc = getattr(lib, name + "_c_f32")(batch.ref(), K, int(terminals), p(dev_cost), *head, *tail, hip.stream())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(a, b, keys=None):
    for k in (keys or a):
        assert a[k].tobytes() == b[k].tobytes(), k


def check(pkg, batch, K, terminals, cost, A, iterations, bounds=None, anneal_score=True):
    """One call with a cost against the restatement, graph by graph; a skipped graph keeps its garbage."""
    got = run_chain(pkg, batch, K, terminals, cost, A, iterations, bounds)
    first = PR.first_of(K, terminals)
    counters = ("best_iter", "moves") + (("repairs",) if bounds is not None else ())
    ran = [max(first, 1) <= n <= batch.c.n_max for n in batch.sizes]
    assert not all(ran) or batch.B == 1
    for g, ((rp, cl, w), (lo, hi)) in enumerate(zip(batch.csrs, batch.spans())):
        where = (g, hi - lo)
        if not ran[g]:
            assert (got["assign"][:, lo:hi] == A[:, lo:hi]).all() and np.isnan(got["cut_all"][g]).all(), where
            assert all((got[k][g] == GARBAGE).all() for k in counters), where
            assert np.isnan(got["best_cut"][g]) and got["best_idx"][g] == GARBAGE, where
            assert (got["best_assign"][lo:hi] == GARBAGE).all(), where
            continue
        ref = CC.run(hi - lo, rp, cl, w, cost[lo:hi], A[:, lo:hi], K, terminals, iterations,
                     None if bounds is None else (bounds[0][g], bounds[1][g]), TENURE, SEED)
        assert got["assign"][:, lo:hi].tobytes() == np.ascontiguousarray(ref["assign"]).tobytes(), where
        for k in counters:
            assert got[k][g].tobytes() == ref[k].tobytes(), (k, where)
        assert got["cut_all"][g].tobytes() == ref["cut_all"].tobytes(), where
        assert got["best_idx"][g] == ref["best_idx"] and got["best_cut"][g].tobytes() == ref["best_cut"].tobytes(), where
        assert (got["best_assign"][lo:hi] == ref["best_assign"]).all(), where
        if bounds is not None:
            assert got["feasible"][g] == 1
            for a in got["assign"][:, lo:hi]:
                s = np.bincount(a, minlength=K)
                assert (s >= bounds[0][g]).all() and (s <= bounds[1][g]).all(), where
    if anneal_score:   # the bits gmc_kway_refine_anneal_c_f32 without a sweep reports for the same bytes and cost
        scored = run_anneal(pkg, batch, K, terminals, cost, got["assign"], np.zeros(0, F), 0, 0)
        for g in range(batch.B):
            if ran[g]:
                assert scored["cut_all"][g].tobytes() == got["cut_all"][g].tobytes(), g
    return got


def case_cost(kind, batch, K, terminals, seed):
    """make_cost's kinds, the barrier on one movable row of every graph that has one; a terminal's row holds a cost too."""
    first = PR.first_of(K, terminals)
    rows = [lo + first + (hi - lo - first) // 2 for lo, hi in batch.spans() if hi - lo > first]
    return make_cost(kind, batch.R, K, seed, rows)[0]


KT = [(2, False), (2, True), (3, False), (3, True), (8, False), (8, True)]
WEIGHTS = ("unit", "signed", "real")
COSTS = ("int", "real", "barrier")
# every (K, terminals) with every kind of weight; the kind of cost rotates so that each meets every K and every weight
CASES = [(K, t, w, COSTS[(i + j) % 3]) for i, (K, t) in enumerate(KT) for j, w in enumerate(WEIGHTS)]


@pytest.mark.parametrize("K,t,weights,costs", CASES, ids=lambda v: str(v))
def test_a_mixed_batch_matches_the_restatement_byte_for_byte(pkg, K, t, weights, costs):
    csrs, n_max = mixed_graphs(K, t, weights)
    batch = batch_of(pkg, csrs, n_max)
    cost = case_cost(costs, batch, K, t, 11 * K + t)
    A = starts(batch, K, CANDS, t, K)
    iterations = 3 * 65                                                 # about 3 n at the wave boundary
    check(pkg, batch, K, t, cost, A, iterations)
    got = check(pkg, batch, K, t, cost, A, iterations, exact_bounds(batch, K))
    assert (got["repairs"][got["repairs"] != GARBAGE] >= 0).all() and (got["repairs"] > 0).any()   # random starts are repaired


@pytest.mark.parametrize("K,t", [(2, False), (3, True)])
def test_three_n_iterations_on_the_300_node_graph(pkg, K, t):
    _n, rp, cl = PR.ring_with_chords(300, 3)
    batch = batch_of(pkg, [(rp, cl, symmetric_weights(300, rp, cl, "signed", 4))])
    cost = case_cost("int", batch, K, t, 5)
    A = starts(batch, K, 2, t, 6)
    got = check(pkg, batch, K, t, cost, A, 900)
    assert (got["best_iter"] > 0).all()
    check(pkg, batch, K, t, cost, A, 900, exact_bounds(batch, K))


@pytest.mark.parametrize("K,t", [(2, False), (8, True)])
def test_a_negative_zero_cost_gives_the_bytes_of_a_positive_zero(pkg, K, t):
    """Zeros mixed with -0.0, compared against the +0.0 array on every output; one graph starts in one class, so whole
    columns of the table are a bare cost (the -0.0 that would sort below +0.0 on ordered bits)."""
    csrs, n_max = mixed_graphs(K, t, "unit")
    batch = batch_of(pkg, csrs, n_max)
    rng = np.random.RandomState(3)
    neg = np.where(rng.randint(0, 2, (batch.R, K)) == 1, F(-0.0), F(0.0)).astype(F)
    assert np.signbit(neg).any() and not np.signbit(neg).all()
    pos = np.zeros((batch.R, K), F)
    A = starts(batch, K, CANDS, t, 2)
    lo, hi = batch.spans()[-1]
    A[:, lo + PR.first_of(K, t):hi] = 0
    for bounds in (None, exact_bounds(batch, K)):
        a = run_chain(pkg, batch, K, t, neg, A, 150, bounds)
        b = run_chain(pkg, batch, K, t, pos, A, 150, bounds)
        same(a, b)
        same(a, run_chain(pkg, batch, K, t, None, A, 150, bounds))      # and both are the twin


@pytest.mark.parametrize("K,t", [(2, False), (3, True), (8, True)])
def test_null_and_zero_costs_are_the_twins_and_loose_bounds_the_tabu_search(pkg, K, t):
    csrs, n_max = mixed_graphs(K, t, "real")
    batch = batch_of(pkg, csrs, n_max)
    A = starts(batch, K, CANDS, t, 7)
    zeros = np.zeros((batch.R, K), F)
    for bounds in (None, exact_bounds(batch, K)):
        twin = run_chain(pkg, batch, K, t, None, A, 150, bounds)
        same(twin, run_chain(pkg, batch, K, t, "null", A, 150, bounds))
        same(twin, run_chain(pkg, batch, K, t, zeros, A, 150, bounds))
    cost = case_cost("real", batch, K, t, 8)
    plain = run_chain(pkg, batch, K, t, cost, A, 150)
    loose = run_chain(pkg, batch, K, t, cost, A, 150, loose_bounds(batch, K))
    same(plain, loose, plain.keys())
    ran = loose["repairs"] != GARBAGE
    assert (loose["repairs"][ran] == 0).all() and (plain["assign"] != A).any()
    assert (plain["assign"] != run_chain(pkg, batch, K, t, None, A, 150)["assign"]).any()   # (the cost is not a bystander)


def test_an_out_of_bounds_start_is_repaired_under_exact_bounds(pkg):
    K, t = 3, True
    csrs, n_max = mixed_graphs(K, t, "signed")
    batch = batch_of(pkg, csrs, n_max)
    cost = case_cost("int", batch, K, t, 9)
    A = np.zeros((3, batch.R), np.int8)                                 # everything in class 0 but the terminals
    for lo, hi in batch.spans():
        A[:, lo:lo + K] = np.arange(K)
    got = check(pkg, batch, K, t, cost, A, 0, exact_bounds(batch, K))   # iterations = 0: repairs, scores and picks
    ran = got["repairs"] != GARBAGE
    assert (got["repairs"][ran] > 0).sum() >= 3 * 6 and (got["moves"][ran] == 0).all()
    check(pkg, batch, K, t, cost, A, 60, exact_bounds(batch, K))


def test_no_iterations_score_and_move_nothing_and_a_byte_of_no_class_never_moves(pkg):
    K, t = 3, True
    csrs, n_max = mixed_graphs(K, t, "unit")
    batch = batch_of(pkg, csrs, n_max)
    cost = case_cost("real", batch, K, t, 10)
    A = starts(batch, K, CANDS, t, 11)
    got = check(pkg, batch, K, t, cost, A, 0)
    assert (got["assign"] == A).all()
    ran = got["moves"] != GARBAGE
    assert (got["moves"][ran] == 0).all() and (got["best_iter"][ran] == 0).all()
    lo, hi = batch.spans()[-1]
    A[0, lo + 10], A[1, lo + 20], A[2, hi - 1] = 3, -1, 100
    got = check(pkg, batch, K, t, cost, A, 200)
    assert got["assign"][0, lo + 10] == 3 and got["assign"][1, lo + 20] == -1 and got["assign"][2, hi - 1] == 100


# ---- chains per workgroup, staged against global ---------------------------------------------------------------------
PACKING = {4: (100, 3, 150), 2: (1100, 8, 24), 1: (2200, 8, 16)}        # slots -> n, K, iterations (degree 3)


@functools.lru_cache(maxsize=None)
def packing_graph(slots):
    n = PACKING[slots][0]
    return csr_of(util.near_regular(n, 3, n, attrs=False))


@pytest.mark.parametrize("global_csr", (False, True))
@pytest.mark.parametrize("slots", (4, 2, 1))
def test_every_lds_shape(pkg, slots, global_csr):
    """Four, two and one chain to a workgroup, through the LDS copy of the CSR and (nnz_max overstated) without it."""
    n, K, iterations = PACKING[slots]
    batch = batch_of(pkg, [packing_graph(slots)], global_csr=global_csr)
    s = pkg.hip.load().gmc_kway_tabu_shape(batch.ref(), K)
    assert (s & 15, s >> 4) == (slots, int(not global_csr)) == lds_shape(K, n, batch.c.nnz_max, False)
    cost = case_cost("real", batch, K, True, slots)
    A = starts(batch, K, CANDS, True, slots)
    check(pkg, batch, K, True, cost, A, iterations, anneal_score=not global_csr)
    check(pkg, batch, K, True, cost, A, iterations, exact_bounds(batch, K), anneal_score=False)


# ---- reproducibility -------------------------------------------------------------------------------------------------
def test_two_calls_and_a_side_stream_give_the_same_bytes(pkg):
    K, t = 3, False
    csrs, n_max = mixed_graphs(K, t, "real")
    batch = batch_of(pkg, csrs, n_max)
    cost = case_cost("real", batch, K, t, 12)
    A = starts(batch, K, CANDS, t, 13)
    for bounds in (None, exact_bounds(batch, K)):
        first = run_chain(pkg, batch, K, t, cost, A, 150, bounds)
        same(first, run_chain(pkg, batch, K, t, cost, A, 150, bounds))
        same(first, run_chain(pkg, batch, K, t, cost, A, 150, bounds, stream=torch.cuda.Stream()))


# ---- the Python layers -----------------------------------------------------------------------------------------------
def test_the_one_graph_searches_take_a_cost(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from oracle import ref_dense as R
    from tests.test_refine_host import handles_of
    g = R.regular_graph(60, 5, 1)
    h = handles_of([g])[0]
    for K, t in ((3, True), (2, False)):
        a0 = np.random.RandomState(K).randint(0, K, 60).astype(np.int8)
        if t:
            a0[:K] = np.arange(K)
        cost = np.random.RandomState(K + 1).randint(-3, 4, (60, K)).astype(np.float64)
        obj = lambda a: NR.objective64(h.rowptr, h.col, h.weight, cost, a, K)
        assign, value = TN.kway_tabu_search(a0.tolist(), g, K, iterations=150, seed=9, terminals=t, node_cost=cost)
        ref = CC.tabu(60, h.rowptr, h.col, h.weight, cost.astype(F), a0, K, t, 0, 150, seed=9)
        assert assign == ref.assign.tolist() and value == obj(assign) == obj(a0) + float(ref.best)
        assign, value = TN.kway_balanced_search(a0.tolist(), g, K, iterations=150, seed=9, terminals=t,
                                                node_cost=torch.from_numpy(cost))
        lo, hi = np.full(K, 60 // K), np.full(K, -(-60 // K))
        ref = CC.balanced(60, h.rowptr, h.col, h.weight, cost.astype(F), a0, K, t, 0, lo, hi, 150, seed=9)
        assert assign == ref.assign.tolist() and value == obj(assign)
        assert (np.bincount(assign, minlength=K) >= lo).all() and (np.bincount(assign, minlength=K) <= hi).all()


def door_batch():
    from tests.test_gpu_node_cost import door_batch as make
    return make()


SOLVE = dict(hidden_dim=8, epochs=6, learning_rate=0.05, samples=6, anneal_sweeps=8, seed=3)


def objectives(ei, ptr, w, cost, part):
    """float64 per graph: the cut of `part` (every edge listed in both directions) minus its cost; (objective, cost)."""
    part = np.asarray(part, np.int64)
    obj, cst = [], []
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        inside = (ei[0] >= lo) & (ei[0] < hi)
        cut = float(w[inside][part[ei[0][inside]] != part[ei[1][inside]]].astype(np.float64).sum()) / 2
        c = float(cost[lo:hi][np.arange(hi - lo), part[lo:hi]].sum())
        obj.append(cut - c)
        cst.append(c)
    return np.asarray(obj), np.asarray(cst)


@pytest.mark.parametrize("K", (2, 3))
def test_solve_batch_takes_a_cost_with_the_tabu_stage_with_bounds_and_with_pins(pkg, K):
    mc = pkg.maxcut
    ei, ptr, w = door_batch()
    R_ = int(ptr[-1])
    cost = np.random.RandomState(4).randint(-3, 4, (R_, K)).astype(np.float64)
    make = lambda: pkg.GraphBatch.from_edge_index(ei, ptr, edge_weight=w)
    kw = dict(number_classes=K, node_cost=cost, **SOLVE)
    num = lambda t: t.cpu().numpy().astype(np.float64)
    base = mc.solve_batch(make(), **kw)
    # ---- the tabu stage
    res = mc.solve_batch(make(), tabu_iterations=120, **kw)
    obj, cst = objectives(ei, ptr, w, cost, res.partition.cpu().numpy())
    assert np.array_equal(num(res.cut), obj) and np.array_equal(num(res.node_cost_sum), cst)
    assert (res.cut >= res.annealed_cut).all() and res.annealed_cut.cpu().numpy().tobytes() == base.cut.cpu().numpy().tobytes()
    assert res.trained_cut.cpu().numpy().tobytes() == base.trained_cut.cpu().numpy().tobytes()
    # ---- the balanced stage
    res = mc.solve_batch(make(), class_sizes="balanced", balance_iterations=120, **kw)
    part = res.partition.cpu().numpy()
    obj, cst = objectives(ei, ptr, w, cost, part)
    assert np.array_equal(num(res.cut), obj) and np.array_equal(num(res.node_cost_sum), cst)
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        s = np.bincount(part[lo:hi], minlength=K)
        assert s.min() >= (hi - lo) // K and s.max() <= -(-(hi - lo) // K)
    # unconstrained_cut is the annealing's objective on this path (its temperature is in units of the mean ABSOLUTE edge
    # weight here, so it need not be `base.cut`): under loose bounds the balanced stage is the tabu stage on the annealed
    # candidates, which for integer data never ends below the best of them
    n = np.diff(ptr)
    loose = mc.solve_batch(make(), class_sizes=(np.zeros((len(n), K), np.int64), np.repeat(n[:, None], K, 1)),
                           balance_iterations=120, **kw)
    assert loose.unconstrained_cut.cpu().numpy().tobytes() == res.unconstrained_cut.cpu().numpy().tobytes()
    assert (loose.cut >= loose.unconstrained_cut).all()
    assert np.array_equal(num(loose.cut), objectives(ei, ptr, w, cost, loose.partition.cpu().numpy())[0])
    # ---- pins
    nodes = np.concatenate([lo + 3 * np.arange(K + 1) for lo in ptr[:-1]])   # apart on the ring: free neighbours
    classes = np.concatenate([np.arange(K + 1) % K for _ in ptr[:-1]])
    res = mc.solve_batch(make(), fixed=(nodes, classes), tabu_iterations=120, **kw)
    part = res.partition.cpu().numpy()
    assert (part[nodes] == classes).all() and res.ptr.cpu().tolist() == ptr.tolist()
    obj, cst = objectives(ei, ptr, w, cost, part)
    assert np.array_equal(num(res.cut), obj) and np.array_equal(num(res.node_cost_sum), cst)
    assert (res.cut >= res.annealed_cut).all() and (res.cut >= res.trained_cut).all() and (res.cut >= res.rounded_cut).all()
    pinned = np.asarray([cost[lo + 3 * np.arange(K + 1), np.arange(K + 1) % K].sum() for lo in ptr[:-1]])
    assert np.array_equal(num(res.fixed_cost), pinned) and res.fixed_cut is not None
    plain = mc.solve_batch(make(), fixed=(nodes, classes), **kw)
    assert plain.annealed_cut is None and np.array_equal(num(plain.cut), objectives(ei, ptr, w, cost, plain.partition.cpu().numpy())[0])
    assert res.annealed_cut.cpu().numpy().tobytes() == plain.cut.cpu().numpy().tobytes()


def test_the_doors_defaults_return_todays_bytes(pkg):
    ei, ptr, w = door_batch()
    lin = np.random.RandomState(2).randint(-3, 4, int(ptr[-1])).astype(np.float64)
    a = pkg.maxcut.solve_qubo(ei, ptr, quadratic=w, linear=lin, **SOLVE)
    b = pkg.maxcut.solve_qubo(ei, ptr, quadratic=w, linear=lin, tabu_iterations=0, class_sizes=None, cardinality=None, **SOLVE)
    assert a.x.cpu().numpy().tobytes() == b.x.cpu().numpy().tobytes() and a.energy.cpu().numpy().tobytes() == b.energy.cpu().numpy().tobytes()
    assert a.result.annealed_cut is None and a.result.unconstrained_cut is None


def edges_both(edges, values):
    ei = np.asarray([[i for i, _j in edges] + [j for _i, j in edges], [j for _i, j in edges] + [i for i, _j in edges]], np.int64)
    return ei, np.concatenate([values, values])


@pytest.mark.parametrize("seed,n,_K", CC.BRUTE_INSTANCES[:6], ids=lambda v: str(v))
def test_solve_qubo_with_a_cardinality(pkg, seed, n, _K):
    import itertools
    _rp, _cl, _w, _cost, edges, quad, lin = CC.drawn_instance(seed, n, 2)
    ei, both = edges_both(edges, quad)
    kw = dict(hidden_dim=8, epochs=10, learning_rate=0.05, samples=8, anneal_sweeps=30, seed=seed)
    k = n // 2
    res = pkg.maxcut.solve_qubo(ei, num_nodes=n, quadratic=both, linear=lin, cardinality=k, **kw)
    x = res.x.cpu().numpy()
    best = min(NR.qubo_energy(edges, quad, lin, b) for b in itertools.product((0, 1), repeat=n) if sum(b) == k)
    assert int(x.sum()) == k and float(res.energy[0]) == NR.qubo_energy(edges, quad, lin, x) >= best
    free = pkg.maxcut.solve_qubo(ei, num_nodes=n, quadratic=both, linear=lin, **kw)
    assert float(-res.result.unconstrained_cut[0]) == float(free.energy[0])   # what the call returns without the bound
    pair = pkg.maxcut.solve_qubo(ei, num_nodes=n, quadratic=both, linear=lin, cardinality=(1, 2), tabu_iterations=50, **kw)
    assert 1 <= int(pair.x.sum()) <= 2 and float(pair.energy[0]) == NR.qubo_energy(edges, quad, lin, pair.x.cpu().numpy())


def test_solve_ising_with_the_tabu_stage_and_with_bounds(pkg):
    ei, ptr, w = door_batch()
    h = np.random.RandomState(5).randint(-3, 4, int(ptr[-1])).astype(np.float64)
    once = ei[0] < ei[1]
    edges = list(zip(ei[0][once].tolist(), ei[1][once].tolist()))
    J = w[once].astype(np.float64)

    def energies(spins):
        out = []
        for lo, hi in zip(ptr[:-1], ptr[1:]):
            inside = [(i, j) for i, j in edges if lo <= i < hi]
            jj = [v for (i, _j), v in zip(edges, J) if lo <= i < hi]
            s = np.zeros(int(ptr[-1]))
            s[lo:hi] = spins[lo:hi]
            out.append(NR.ising_energy(inside, jj, h, s))
        return np.asarray(out)

    base = pkg.maxcut.solve_ising(ei, ptr, coupling=w, field=h, **SOLVE)
    res = pkg.maxcut.solve_ising(ei, ptr, coupling=w, field=h, tabu_iterations=150, **SOLVE)
    assert np.array_equal(res.energy.numpy(), energies(res.spins.cpu().numpy()))
    assert (res.energy <= base.energy).all()
    assert res.result.annealed_cut.cpu().numpy().tobytes() == base.result.cut.cpu().numpy().tobytes()
    bal = pkg.maxcut.solve_ising(ei, ptr, coupling=w, field=h, class_sizes="balanced", balance_iterations=100, **SOLVE)
    spins = bal.spins.cpu().numpy()
    assert np.array_equal(bal.energy.numpy(), energies(spins))
    for lo, hi in zip(ptr[:-1], ptr[1:]):
        assert abs(int(spins[lo:hi].sum())) <= (hi - lo) % 2            # zero magnetisation, or one spin over
