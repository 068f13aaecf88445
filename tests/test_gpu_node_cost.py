"""GPU tests of the per-node class costs (include/gcnmaxcut.h, the ``_c`` entry points).

Decoders: gmc_round_conditional_c_f32, gmc_kway_decode_sample_seeded_c_f32 and gmc_kway_refine_anneal_c_f32 against
tests/node_cost_ref.py byte for byte - assign, the pick, the sweep counters and the scores' bits - at K = 2, 3, 8, with
and without terminals, for integer costs, full-mantissa real costs and a 1e6 barrier; NULL equals the ``_t`` twin and an
all-+0.0f array equals NULL.  The batch holds graphs of different sizes (r0 != 0: indexing the cost by local id fails),
n = 1 (without terminals) or n = K (with: nothing movable), n = 257, a star with 70 leaves, a graph with self-loops and
signed integer edge weights; one more batch answers 0 to gmc_refine_anneal_staged.  The scores are restated in the
device's own summation order, so real-valued costs are bit for bit too; edge weights are integers.

Head: gmc_inst_forward_c / gmc_inst_train_fwd_bwd_c against the float64 model with the cost in the loss, at stepcheck's
bars (P 5e-7, gradient rows 2e-4 = FR.grad_ratios).  The batches are built from raw arrays, because a GraphBatch
refuses graphs below 3 nodes and the cases ask for n = 1 and n = K.

Front doors: solve(node_cost=...), solve_ising, solve_qubo."""
import ctypes as C
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from tests import anneal_ref as AR
from tests import functional_ref as FR
from tests import kway_ref as KR
from tests import node_cost_ref as NC
from tests import plain_ref as PR
from tests import rounding_ref as RO
from tests import seeded_ref as SR
from tests.stepcheck import KEYS, P_TOL
from tests.test_refine_host import loop_graph
from tests.test_rounding_host import SLACK

pytestmark = pytest.mark.gpu
F32 = np.float32
GARBAGE = -5
LOSS_BAR = 5e-5     # x C x (total |weight| + total |cost|): the bar tests/test_gpu_plain_instance.py has for weighted losses


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


class Raw:
    """A gmc_batch straight from (rowptr, col, w) graphs - any sizes from 1 node on - with gcol and dinv, so that the
    decoders and the instance sequence both take it, and the (colour, id) order of tests/plain_ref.py."""

    def __init__(self, pkg, csrs):
        hip = pkg.hip
        self.csrs = [(np.asarray(rp, np.int64), np.asarray(cl, np.int64), None if w is None else np.asarray(w, F32))
                     for rp, cl, w in csrs]
        self.sizes = np.asarray([len(rp) - 1 for rp, _cl, _w in self.csrs], np.int64)
        self.goff_host = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        nnz = [len(cl) for _rp, cl, _w in self.csrs]
        eoff = np.concatenate([[0], np.cumsum(nnz)]).astype(np.int64)
        self.B, self.R = len(self.csrs), int(self.goff_host[-1])
        rowptr = np.concatenate([[0]] + [rp[1:] + eoff[g] for g, (rp, _cl, _w) in enumerate(self.csrs)]).astype(np.int32)
        lcol = np.concatenate([cl for _rp, cl, _w in self.csrs] + [np.zeros(0, np.int64)]).astype(np.int32)
        gcol = np.concatenate([cl + self.goff_host[g] for g, (_rp, cl, _w) in enumerate(self.csrs)]
                              + [np.zeros(0, np.int64)]).astype(np.int32)
        unit = all(w is None for _rp, _cl, w in self.csrs)
        vals = None if unit else np.concatenate([np.ones(len(cl), F32) if w is None else w for _rp, cl, w in self.csrs])
        dinv = (1.0 / np.sqrt(np.maximum(np.diff(rowptr.astype(np.int64)), 1))).astype(F32)
        self.vals_host = vals
        dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
        pad = lambda a: a if a.size else np.zeros(1, a.dtype)           # (an empty tensor has no pointer to hand over)
        self.keep = [dev(self.goff_host.astype(np.int32)), dev(rowptr), dev(pad(lcol)), dev(pad(gcol)), dev(vals), dev(dinv)]
        p = hip.ptr
        self.c = hip.GmcBatch(B=self.B, R=self.R, nnz=int(eoff[-1]), n_max=int(self.sizes.max()), nnz_max=int(max(nnz)),
                              goff=p(self.keep[0]), rowptr=p(self.keep[1]), lcol=p(self.keep[2]), gcol=p(self.keep[3]),
                              vals=p(self.keep[4]), dinv=p(self.keep[5]))
        self._orders = {}

    def ref(self):
        return C.byref(self.c)

    def spans(self):
        return [(int(self.goff_host[g]), int(self.goff_host[g + 1])) for g in range(self.B)]

    def order(self, K, terminals):
        if (K, terminals) not in self._orders:
            arrays = PR.order_arrays([(len(rp) - 1, rp, cl) for rp, cl, _w in self.csrs], PR.first_of(K, terminals))[:3]
            self._orders[K, terminals] = tuple(
                torch.from_numpy(np.ascontiguousarray(a if a.size else np.zeros(1, np.int32))).cuda() for a in arrays)
        return self._orders[K, terminals]


def csr_of(g):
    """(rowptr, col, w or None) of a networkx graph (a self-loop listed once; integer `weight` attributes)."""
    n = g.number_of_nodes()
    rowptr, col, w = [0], [], []
    weighted = any("weight" in d for _u, _v, d in g.edges(data=True))
    for v in range(n):
        for u in sorted(g[v]):
            col.append(u)
            w.append(float(g[v][u].get("weight", 1.0)))
        rowptr.append(len(col))
    return np.asarray(rowptr, np.int64), np.asarray(col, np.int64), np.asarray(w, F32) if weighted else None


def signed_integer_weights(n, rp, cl, seed):
    """Symmetric weights in {-2, -1, 1, 2, 3} on the entries of a CSR."""
    rng = np.random.RandomState(seed)
    w = np.zeros(len(cl), F32)
    at = {}
    for v in range(n):
        for e in range(int(rp[v]), int(rp[v + 1])):
            u = int(cl[e])
            key = (min(u, v), max(u, v))
            if key not in at:
                at[key] = float(rng.choice([-2, -1, 1, 2, 3]))
            w[e] = at[key]
    return w


@functools.lru_cache(maxsize=None)
def decoder_graphs(K, terminals):
    """The graphs of the decoders' batch (see the module's docstring): rowptr / col / weights per graph."""
    n40, rp40, cl40 = PR.ring_with_chords(40, 5)
    small = PR.ring_with_chords(K, 6) if terminals and K >= 3 else None
    if terminals:      # n = K: nothing movable
        tiny = (small[1], small[2], None) if small else (np.array([0, 1, 2]), np.array([1, 0]), None)
    else:              # n = 1: one isolated node
        tiny = (np.array([0, 0]), np.zeros(0, np.int64), None)
    n257, rp257, cl257 = PR.ring_with_chords(257, 7)
    _ns, rps, cls_ = PR.star_centre2(70)
    n33, rp33, cl33 = PR.ring_with_chords(33, 8)
    return ((rp40, cl40, None), tiny, (rp257, cl257, None), (rps, cls_, None), csr_of(loop_graph(30, 4, 9)),
            (rp33, cl33, signed_integer_weights(n33, rp33, cl33, 10)))


def make_cost(kind, R, K, seed, pinned_rows):
    """(cost [R, K] float32, {row: cheap class}).  int: integers in -3..3; real: full-mantissa values of that size;
    barrier: integers, and 1e6 on every class but one of the pinned rows."""
    rng = np.random.RandomState(seed)
    if kind == "real":
        return (rng.uniform(-3.0, 3.0, (R, K)) * (1.0 + 2.0 ** -20)).astype(F32), {}
    cost = rng.randint(-3, 4, (R, K)).astype(F32)
    pins = {}
    if kind == "barrier":
        for row in pinned_rows:
            cheap = int(rng.randint(0, K))
            cost[row] = 1e6
            cost[row, cheap] = 0.0
            pins[row] = cheap
    return cost, pins


def _cost_args(cost):
    """(tensor kept alive, pointer): cost None -> the _t twin is called; "null" -> the _c entry point with NULL."""
    if cost is None or isinstance(cost, str):
        return None, None
    t = torch.from_numpy(np.ascontiguousarray(cost, F32)).cuda()
    return t, t.data_ptr()


def run_round(pkg, batch, P, K, t, cost, descent):
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    order, cgoff, cptr = batch.order(K, t)
    Pt = torch.from_numpy(np.ascontiguousarray(P, F32)).cuda()
    assign = torch.full((batch.R,), GARBAGE, dtype=torch.int8, device="cuda")
    cut = torch.full((batch.B,), float("nan"), device="cuda")
    expected = torch.full((batch.B,), float("nan"), device="cuda")
    sweeps = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    tail = (p(order), p(cgoff), p(cptr), descent, p(assign), p(cut), p(expected), p(sweeps), hip.stream())
    keep, cp = _cost_args(cost)
    if cost is None:
        hip.check(lib.gmc_round_conditional_t_f32(batch.ref(), p(Pt), K, int(t), *tail), "round_t")
    else:
        hip.check(lib.gmc_round_conditional_c_f32(batch.ref(), p(Pt), K, int(t), cp, *tail), "round_c")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut=cut, expected=expected, sweeps=sweeps).items()}


def run_sample(pkg, batch, P, K, t, cost, keys, iters):
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    Pt = torch.from_numpy(np.ascontiguousarray(P, F32)).cuda()
    gkey = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()
    assign_all = torch.full((iters, batch.R), GARBAGE, dtype=torch.int8, device="cuda")
    cut_all = torch.full((batch.B, iters), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_iter = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    tail = (p(gkey), iters, p(assign_all), p(cut_all), p(best_assign), p(best_cut), p(best_iter), hip.stream())
    keep, cp = _cost_args(cost)
    if cost is None:
        hip.check(lib.gmc_kway_decode_sample_seeded_t_f32(batch.ref(), p(Pt), K, int(t), *tail), "sample_t")
    else:
        hip.check(lib.gmc_kway_decode_sample_seeded_c_f32(batch.ref(), p(Pt), K, int(t), cp, *tail), "sample_c")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign_all=assign_all, cut_all=cut_all, best_assign=best_assign,
                                                    best_cut=best_cut, best_iter=best_iter).items()}


def run_anneal(pkg, batch, K, t, cost, A, inv_temp, seed, max_descent):
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    cands = A.shape[0]
    order, cgoff, cptr = batch.order(K, t)
    assign = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    inv_t = torch.from_numpy(np.asarray(inv_temp, F32)).cuda() if len(inv_temp) else None
    lv = torch.from_numpy(AR.levels()).cuda() if len(inv_temp) else None
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    snap = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    sweeps = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    tail = (p(order), p(cgoff), p(cptr), cands, p(assign), p(inv_t), len(inv_temp), p(lv), seed, max_descent, p(cut_all),
            p(best_assign), p(best_cut), p(best_idx), p(snap), p(sweeps), hip.stream())
    keep, cp = _cost_args(cost)
    if cost is None:
        hip.check(lib.gmc_kway_refine_anneal_t_f32(batch.ref(), K, int(t), *tail), "anneal_t")
    else:
        hip.check(lib.gmc_kway_refine_anneal_c_f32(batch.ref(), K, int(t), cp, *tail), "anneal_c")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut_all=cut_all, best_assign=best_assign, best_cut=best_cut,
                                                    best_idx=best_idx, snap=snap, sweeps=sweeps).items()}


def same_bytes(a, b):
    return all(a[k].tobytes() == b[k].tobytes() for k in a)


def probabilities(batch, K, seed, pins):
    P = np.concatenate([PR.softmax_rows(hi - lo, K, seed + g) for g, (lo, hi) in enumerate(batch.spans())])
    for row, cheap in pins.items():
        P[row] = np.eye(K, dtype=F32)[cheap]               # the sampler draws from P alone: the pinned rows are decided in it
    return P


def pinned_rows(batch, K, terminals):
    """One movable row of every graph that has one (not the first rows: those are the terminals)."""
    first = PR.first_of(K, terminals)
    return [lo + (hi - lo) // 2 for lo, hi in batch.spans() if hi - lo > first and (hi - lo) // 2 >= first]


CASES = [(K, t, kind) for K in (2, 3, 8) for t in (False, True) for kind in ("int", "real", "barrier")]


@pytest.mark.parametrize("K,t,kind", CASES, ids=lambda v: str(v))
def test_decoders_match_the_restatement_byte_for_byte(pkg, K, t, kind):
    graphs = decoder_graphs(K, t)
    batch = Raw(pkg, graphs)
    first = PR.first_of(K, t)
    assert pkg.hip.load().gmc_refine_anneal_staged(batch.ref()) == 1 or batch.c.n_max < 3
    cost, pins = make_cost(kind, batch.R, K, 17 * K + t, pinned_rows(batch, K, t))
    zeros = np.zeros((batch.R, K), F32)
    P = probabilities(batch, K, 40 * K, pins)
    keys = SR.keys(3 + K, range(2, 2 + batch.B))
    A = np.random.RandomState(K).randint(0, K, (3, batch.R)).astype(np.int8)
    for lo, hi in batch.spans():
        A[:, lo:lo + min(first, hi - lo)] = np.arange(min(first, hi - lo))
    A[1, batch.spans()[0][0] + first + 1] = K + 2          # a byte of no class on a movable node
    scale = float(np.mean(np.abs(batch.vals_host)))
    inv_t = AR.schedule(4, scale=scale)

    # NULL is the _t twin, an all-+0.0f array is NULL
    for run in (lambda c: run_round(pkg, batch, P, K, t, c, 100), lambda c: run_sample(pkg, batch, P, K, t, c, keys, 5),
                lambda c: run_anneal(pkg, batch, K, t, c, A, inv_t, 9, 100)):
        twin = run(None)
        assert same_bytes(twin, run("null")) and same_bytes(twin, run(zeros))

    rounded = run_round(pkg, batch, P, K, t, cost, 100)
    rounded0 = run_round(pkg, batch, P, K, t, cost, 0)
    sampled = run_sample(pkg, batch, P, K, t, cost, keys, 5)
    annealed = run_anneal(pkg, batch, K, t, cost, A, inv_t, 9, 100)
    scored = run_anneal(pkg, batch, K, t, cost, A, [], 9, 0)
    assert (scored["assign"] == A).all()
    for g, ((rp, cl, w), (lo, hi)) in enumerate(zip(batch.csrs, batch.spans())):
        n, cg = hi - lo, cost[lo:hi]
        what = (K, t, kind, g)
        ref = NC.restate_round(n, rp, cl, w, cg, P[lo:hi], K, first, 100)
        assert (rounded0["assign"][lo:hi] == ref["a0"]).all(), what
        assert (rounded["assign"][lo:hi] == ref["a1"]).all() and rounded["sweeps"][g] == ref["sweeps"], what
        assert rounded["cut"][g:g + 1].tobytes() == np.asarray([ref["cut"]], F32).tobytes(), what
        exp64 = NC.expected_objective(n, rp, cl, w, cg, P[lo:hi], K, first)
        scale_g = RO.abs_weight(rp, cl, w) + float(np.abs(cg.astype(np.float64)).sum())
        print(f"{what}: expected objective {rounded['expected'][g]} float64 {exp64} rounded {rounded['cut'][g]}")
        assert abs(float(rounded["expected"][g]) - exp64) <= SLACK * scale_g, what
        assert NC.objective64(rp, cl, w, cg, ref["a0"], K) >= exp64 - SLACK * scale_g, what
        ref = NC.sample(n, rp, cl, w, cg, P[lo:hi], keys[g], 5, first)
        assert (sampled["assign_all"][:, lo:hi] == ref["assign_all"]).all(), what
        assert sampled["cut_all"][g].tobytes() == ref["cut_all"].tobytes(), what
        assert (sampled["best_assign"][lo:hi] == ref["best_assign"]).all() and sampled["best_iter"][g] == ref["best_iter"]
        assert sampled["best_cut"][g] == ref["best_cut"], what
        ref = NC.anneal(n, rp, cl, w, cg, A[:, lo:hi], K, first, inv_t, AR.levels(), 9, 100)
        assert (annealed["assign"][:, lo:hi] == ref["assign"]).all(), what
        assert (annealed["snap"][g] == ref["snap"]).all() and (annealed["sweeps"][g] == ref["sweeps"]).all(), what
        assert annealed["cut_all"][g].tobytes() == ref["cut_all"].tobytes(), what
        assert (annealed["best_assign"][lo:hi] == ref["best_assign"]).all() and annealed["best_idx"][g] == ref["best_idx"]
        assert annealed["best_cut"][g] == ref["best_cut"], what
        for c in range(A.shape[0]):                        # no sweep at all: the score of the input, cost included
            assert scored["cut_all"][g, c] == NC.score(n, rp, cl, w, cg, A[c, lo:hi], K), what
    for row, cheap in pins.items():                        # the barrier pins its node in every output
        assert rounded["assign"][row] == cheap and rounded0["assign"][row] == cheap
        assert (annealed["assign"][:, row] == cheap).all() and annealed["best_assign"][row] == cheap
        assert (sampled["assign_all"][:, row] == cheap).all() and sampled["best_assign"][row] == cheap
    assert kind != "barrier" or len(pins) >= 4


def test_a_batch_that_is_not_staged_takes_the_global_path(pkg):
    """n = 1000, d = 7, integer weights: gmc_refine_anneal_staged answers 0 (as tests/test_gpu_kway_search.py builds it)."""
    g = nx.random_regular_graph(7, 1000, seed=19)
    rng = np.random.RandomState(5)
    for u, v in g.edges():
        g[u][v]["weight"] = int(rng.randint(1, 4))
    n40, rp40, cl40 = PR.ring_with_chords(40, 5)
    batch = Raw(pkg, [(rp40, cl40, None), csr_of(g)])
    assert pkg.hip.load().gmc_refine_anneal_staged(batch.ref()) == 0
    K, t = 3, False
    cost, _ = make_cost("real", batch.R, K, 3, [])
    A = np.random.RandomState(2).randint(0, K, (2, batch.R)).astype(np.int8)
    inv_t = AR.schedule(2, scale=float(np.mean(batch.vals_host)))
    twin = run_anneal(pkg, batch, K, t, None, A, inv_t, 4, 100)
    assert same_bytes(twin, run_anneal(pkg, batch, K, t, "null", A, inv_t, 4, 100))
    assert same_bytes(twin, run_anneal(pkg, batch, K, t, np.zeros((batch.R, K), F32), A, inv_t, 4, 100))
    got = run_anneal(pkg, batch, K, t, cost, A, inv_t, 4, 100)
    for gi, ((rp, cl, w), (lo, hi)) in enumerate(zip(batch.csrs, batch.spans())):
        ref = NC.anneal(hi - lo, rp, cl, w, cost[lo:hi], A[:, lo:hi], K, 0, inv_t, AR.levels(), 4, 100)
        assert (got["assign"][:, lo:hi] == ref["assign"]).all(), gi
        assert (got["snap"][gi] == ref["snap"]).all() and (got["sweeps"][gi] == ref["sweeps"]).all(), gi
        assert got["cut_all"][gi].tobytes() == ref["cut_all"].tobytes(), gi
        assert got["best_idx"][gi] == ref["best_idx"] and got["best_cut"][gi] == ref["best_cut"], gi


# ---- the head -----------------------------------------------------------------------------------------------------------
HIDDEN = {2: 4, 3: 12, 8: 36}
CC = 1.3


@functools.lru_cache(maxsize=None)
def head_graphs(K, terminals):
    """n = K, n = 1 (without terminals; with them a second n = K + 1), n = 1030 with integer weights and the star with
    unit weights (its centre sums 70 terms as it is: weights up to 3 would triple its pre-activations and with them what
    float32 loses on its logits)."""
    _n, rpk, clk = PR.ring_with_chords(K, 11) if K >= 3 else (2, np.array([0, 1, 2]), np.array([1, 0]))
    one = (np.array([0, 0]), np.zeros(0, np.int64), None)
    _n, rpk1, clk1 = PR.ring_with_chords(max(K + 1, 3), 12)
    n1030, rp, cl = PR.ring_with_chords(1030, 13)
    _ns, rps, cls_ = PR.star_centre2(70)
    return ((rpk, clk, None), (rpk1, clk1, None) if terminals else one,
            (rp, cl, PR.integer_weights(n1030, rp, cl, 14)), (rps, cls_, None))


def head_cost(graphs, K, t):
    """Real costs of a magnitude comparable to the node's degree, [R, K] float32."""
    rng = np.random.RandomState(31 * K + t)
    deg = np.concatenate([np.diff(rp) for rp, _cl, _w in graphs]).astype(np.float64)
    return (rng.uniform(-1.0, 1.0, (deg.size, K)) * np.maximum(deg, 1.0)[:, None]).astype(F32)


@functools.lru_cache(maxsize=None)
def head_params(K, t):
    """Per-graph parameters: for every graph the first seed for which, under both losses, the float64 forward keeps
    every row 1e-5 clear of an argmax tie and every layer-1 unit 1e-6 clear of the relu kink, and a float32 numpy
    evaluation of the step keeps a tenth of ROW_TOL on every gradient row (the three rules of tests/plain_ref.py's
    cases, with the cost in the loss).  A tenth, where those cases ask for half: numpy adds pairwise, the kernels add a
    row's up to 1030 terms one after the other, so on a gradient row that cancels the device may lose several times what
    numpy's float32 loses, and costs as large as the degree make such rows (the first draw for the star at K = 2 keeps
    0.41 of ROW_TOL in numpy's float32).  Likewise the probabilities of that evaluation stay within a quarter of
    P_TOL of float64 (n = 1030 rows leave numpy's float32 at a fifth of it on every draw): the star's centre sums 70 leaves one after the other, and at K = 8 some draws leave the device's float32
    at the bar (5.3e-7 and 6.2e-7 were measured where numpy's float32 keeps 7.5e-8 and 2.2e-7), cost or no cost - the
    forward is not what this file is about.
    The bars themselves stay stepcheck's."""
    graphs = head_graphs(K, t)
    cost = head_cost(graphs, K, t)
    out, lo = [], 0
    for g, csr in enumerate(graphs):
        n = len(csr[0]) - 1
        for seed in range(40):
            p = KR.random_params(n, HIDDEN[K], K, 100 * g + seed)
            margin, gap, ratio, p_err = NC.head_rules(csr, p, cost[lo:lo + n], CC, t)
            if margin >= 1e-5 and gap >= 1e-6 and ratio <= 0.1 and p_err <= 0.25 * P_TOL:
                break
        else:
            raise AssertionError(f"no parameters within the rules drawn for graph {g}")
        out.append(p)
        lo += n
    return tuple(out)


def run_inst(pkg, batch, params, K, t, cost, loss, train):
    """gmc_inst_forward_* / gmc_inst_train_fwd_bwd_* on raw buffers: P, S, loss and (training) the flat gradient."""
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    F, B, R = HIDDEN[K], batch.B, batch.R
    flat = np.concatenate([np.concatenate([q["conv1.weight"] for q in params]).ravel(),
                           np.concatenate([q["conv1.bias"] for q in params]).ravel(),
                           np.concatenate([q["conv2.weight"].ravel() for q in params]),
                           np.concatenate([q["conv2.bias"] for q in params]).ravel()]).astype(F32)
    count = flat.size
    buf = torch.zeros(count + 4, device="cuda")
    buf[:count] = torch.from_numpy(flat).cuda()
    o = np.cumsum([0, R * F, B * F, B * F * K])
    model = hip.GmcModel(N=R, F=F, K=K, flags=hip.MODEL_LOSS_EXPECTED if loss == "expected_cut" else 0,
                         W1=buf.data_ptr() + 4 * int(o[0]), b1=buf.data_ptr() + 4 * int(o[1]),
                         W2=buf.data_ptr() + 4 * int(o[2]), b2=buf.data_ptr() + 4 * int(o[3]))
    need = int(lib.gmc_inst_workspace_bytes(batch.ref(), C.byref(model), int(train)))
    assert need > 0
    ws = torch.full((max(need, 256),), 255, dtype=torch.uint8, device="cuda")
    P = torch.full((R, K), float("nan"), device="cuda")
    S = torch.full((R,), GARBAGE, dtype=torch.int32, device="cuda")
    losses = torch.full((B,), float("nan"), device="cuda")
    grad = torch.full((count + 4,), float("nan"), device="cuda")
    keep, cp = _cost_args(cost)
    head = (batch.ref(), C.byref(model), int(t)) + (() if cost is None else (cp,))
    tail = (CC, p(ws), ws.numel(), p(P), p(S), p(losses)) + ((p(grad),) if train else ()) + (hip.stream(),)
    name = ("gmc_inst_train_fwd_bwd" if train else "gmc_inst_forward") + ("_t" if cost is None else "_c")
    hip.check(getattr(lib, name)(*head, *tail), name)
    torch.cuda.synchronize()
    return dict(P=P.cpu().numpy(), S=S.cpu().numpy(), loss=losses.cpu().numpy(), grad=grad[:count].cpu().numpy()), o


def graph_grads(flat, o, batch, g, F, K):
    lo, hi = batch.spans()[g]
    return {"conv1.weight": flat[o[0] + lo * F:o[0] + hi * F].reshape(hi - lo, F),
            "conv1.bias": flat[o[1] + g * F:o[1] + (g + 1) * F],
            "conv2.weight": flat[o[2] + g * F * K:o[2] + (g + 1) * F * K].reshape(F, K),
            "conv2.bias": flat[o[3] + g * K:o[3] + (g + 1) * K]}


@pytest.mark.parametrize("K", (2, 3, 8))
@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
@pytest.mark.parametrize("t", (False, True), ids=("plain", "terminals"))
def test_head_with_a_cost_against_float64(pkg, K, loss, t):
    graphs = head_graphs(K, t)
    batch = Raw(pkg, graphs)
    F = HIDDEN[K]
    cost = head_cost(graphs, K, t)
    params = head_params(K, t)
    got, o = run_inst(pkg, batch, params, K, t, cost, loss, True)
    assert np.isfinite(got["P"]).all() and np.isfinite(got["grad"]).all()
    for g, (csr, p) in enumerate(zip(graphs, params)):
        lo, hi = batch.spans()[g]
        f, value, ref = NC.inst_step(csr, p, cost[lo:hi], CC, loss, t, S=got["S"][lo:hi])
        p_err = float(np.abs(got["P"][lo:hi] - f["P"]).max())
        assert p_err < P_TOL, (g, p_err)
        S_ref = f["P"].argmax(1)
        S_ref[:min(K, hi - lo) if t else 0] = np.arange(min(K, hi - lo) if t else 0)
        assert np.array_equal(got["S"][lo:hi], S_ref), g
        bar = LOSS_BAR * CC * (KR.total_weight([csr]) + float(np.abs(cost[lo:hi].astype(np.float64)).sum()))
        err = abs(float(got["loss"][g]) - value)
        worst_abs, worst_row = FR.grad_ratios(graph_grads(got["grad"], o, batch, g, F, K), ref)
        print(f"K {K} {loss} terminals {t} graph {g}: P {p_err:.2e} loss {got['loss'][g]:.6f} float64 {value:.6f} "
              f"err {err:.2e} bar {bar:.2e} grad {worst_abs:.2e} of ORACLE_BAR, rows {worst_row:.2e} of ROW_TOL")
        assert err <= bar, (g, got["loss"][g], value)
        assert worst_abs <= 1.0 and worst_row <= 1.0, (g, worst_abs, worst_row)
    fwd, _ = run_inst(pkg, batch, params, K, t, cost, loss, False)
    assert all(fwd[k].tobytes() == got[k].tobytes() for k in ("P", "S", "loss"))
    # NULL and an all-zero cost are the _t call, gradient included
    for train in (True, False):
        twin, _ = run_inst(pkg, batch, params, K, t, None, loss, train)
        for other in ("null", np.zeros((batch.R, K), F32)):
            res, _ = run_inst(pkg, batch, params, K, t, other, loss, train)
            assert all(res[k].tobytes() == twin[k].tobytes() for k in (("P", "S", "loss", "grad") if train else ("P", "S", "loss")))


# ---- the front doors ----------------------------------------------------------------------------------------------------
def door_batch():
    """Three rings with chords (20, 33, 12 nodes) as edge_index [2, E] (both directions), ptr and integer weights."""
    src, dst, w, ptr = [], [], [], [0]
    rng = np.random.RandomState(1)
    for i, n in enumerate((20, 33, 12)):
        _n, rp, cl = PR.ring_with_chords(n, 70 + i)
        ww = PR.integer_weights(n, rp, cl, 20 + i)
        for v in range(n):
            for e in range(int(rp[v]), int(rp[v + 1])):
                src.append(ptr[-1] + v)
                dst.append(ptr[-1] + int(cl[e]))
                w.append(float(ww[e]))
        ptr.append(ptr[-1] + n)
    return np.asarray([src, dst], np.int64), np.asarray(ptr, np.int64), np.asarray(w, F32)


SOLVE = dict(hidden_dim=8, epochs=6, learning_rate=0.05, samples=6, anneal_sweeps=8, seed=3)


@pytest.mark.parametrize("K,t", [(2, False), (3, True)])
def test_solve_with_a_node_cost(pkg, K, t):
    mc = pkg.maxcut
    ei, ptr, w = door_batch()
    plain = mc.solve(ei, ptr, edge_weight=w, number_classes=K, terminals=t, **SOLVE)
    assert plain.node_cost_sum is None
    zero = mc.solve(ei, ptr, edge_weight=w, number_classes=K, terminals=t, node_cost=np.zeros((int(ptr[-1]), K)), **SOLVE)
    assert zero.partition.cpu().numpy().tobytes() == plain.partition.cpu().numpy().tobytes()
    assert zero.cut.cpu().numpy().tobytes() == plain.cut.cpu().numpy().tobytes()
    assert (zero.node_cost_sum.cpu().numpy() == 0).all()
    cost = np.random.RandomState(4).randint(-3, 4, (int(ptr[-1]), K)).astype(np.float64)
    a = mc.solve(ei, ptr, edge_weight=w, number_classes=K, terminals=t, node_cost=cost, **SOLVE)
    b = mc.solve(ei, ptr, edge_weight=w, number_classes=K, terminals=t, node_cost=torch.from_numpy(cost).cuda(), **SOLVE)
    for name in ("partition", "cut", "trained_cut", "rounded_cut", "node_cost_sum"):
        assert getattr(a, name).cpu().numpy().tobytes() == getattr(b, name).cpu().numpy().tobytes(), name
    assert (a.cut >= a.trained_cut).all() and (a.cut >= a.rounded_cut).all()
    part = a.partition.cpu().numpy()
    sums = np.asarray([cost[lo:hi][np.arange(hi - lo), part[lo:hi]].sum() for lo, hi in zip(ptr[:-1], ptr[1:])])
    assert np.array_equal(a.node_cost_sum.cpu().numpy().astype(np.float64), sums)
    # cut + node_cost_sum is the plain cut of the partition, recounted by the annealing call with zero sweeps
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    from gcn_max_cut_amd.graph import GraphBatch
    batch = GraphBatch.from_edge_index(ei, ptr, edge_weight=w)
    recount = T._kway_anneal_on_gpu(batch, K, a.partition.to(torch.int8).reshape(1, -1).contiguous(), np.zeros(0, F32), 0, 0, t)[1]
    assert np.array_equal((a.cut + a.node_cost_sum).cpu().numpy(), recount.cpu().numpy())


def test_solve_ising_with_a_strong_uniform_field_opposes_it(pkg):
    ei, ptr, w = door_batch()
    for sign in (1.0, -1.0):
        res = pkg.maxcut.solve_ising(ei, ptr, coupling=w, field=np.full(int(ptr[-1]), 100.0 * sign), **SOLVE)
        assert (res.spins.cpu().numpy() == -sign).all()
        assert res.energy.dtype == torch.float64 and res.spins.dtype == torch.int8
        n = np.diff(ptr)
        sum_j = np.asarray([w[(ei[0] >= lo) & (ei[0] < hi)].sum() / 2 for lo, hi in zip(ptr[:-1], ptr[1:])], np.float64)
        assert np.array_equal(res.energy.numpy(), sum_j - 100.0 * n)


@pytest.mark.parametrize("seed,n", NC.DOOR_INSTANCES)
def test_the_doors_reach_the_brute_force_optimum(pkg, seed, n):
    n, edges, quad, lin = NC.drawn_instance(seed, n)
    ei = np.asarray([[i for i, _j in edges] + [j for _i, j in edges], [j for _i, j in edges] + [i for i, _j in edges]], np.int64)
    both = np.concatenate([quad, quad])
    kw = dict(hidden_dim=8, epochs=10, learning_rate=0.05, samples=8, anneal_sweeps=30, seed=seed)
    best, _ = NC.brute_force_min(n, lambda b: NC.qubo_energy(edges, quad, lin, b))
    res = pkg.maxcut.solve_qubo(ei, num_nodes=n, quadratic=both, linear=lin, **kw)
    x = res.x.cpu().numpy()
    assert float(res.energy[0]) == NC.qubo_energy(edges, quad, lin, x) == best
    once = pkg.maxcut.solve_qubo(ei[:, :len(edges)], num_nodes=n, quadratic=quad, linear=lin, pairs="once", **kw)
    assert once.x.cpu().numpy().tobytes() == x.tobytes() and float(once.energy[0]) == best
    best, _ = NC.brute_force_min(n, lambda b: NC.ising_energy(edges, quad, lin, [1 - 2 * v for v in b]))
    res = pkg.maxcut.solve_ising(ei, num_nodes=n, coupling=both, field=lin, **kw)
    s = res.spins.cpu().numpy()
    assert set(np.unique(s)) <= {-1, 1}
    assert float(res.energy[0]) == NC.ising_energy(edges, quad, lin, s) == best


def test_row_weight_sums(pkg):
    ei, ptr, w = door_batch()
    from gcn_max_cut_amd.graph import GraphBatch
    batch = GraphBatch.from_edge_index(ei, ptr, edge_weight=w)
    out = torch.full((batch.R,), float("nan"), device="cuda")
    hip = pkg.hip
    hip.check(hip.load().gmc_row_weight_sums_f32(batch.R, hip.ptr(batch.rowptr), hip.ptr(batch.gcol), hip.ptr(batch.vals),
                                                 hip.ptr(out), hip.stream()), "gmc_row_weight_sums_f32")
    want = np.zeros(batch.R)
    np.add.at(want, ei[0], w.astype(np.float64))
    assert np.array_equal(out.cpu().numpy().astype(np.float64), want)
    hip.check(hip.load().gmc_row_weight_sums_f32(batch.R, hip.ptr(batch.rowptr), hip.ptr(batch.gcol), None, hip.ptr(out),
                                                 hip.stream()), "gmc_row_weight_sums_f32")
    assert np.array_equal(out.cpu().numpy(), np.bincount(ei[0], minlength=batch.R).astype(F32))
