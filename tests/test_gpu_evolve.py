"""GPU tests of the evolution stage (gmc_kway_evolve_f32 and its Python API) against the CPU restatement in
tests/evolve_ref.py: both planes of the population and of its cuts, the pick and the history byte for byte on unit and
small-integer weights (every fp32 sum is exact in any order); real-valued weights by invariants; the alignment shown on
the device by a crossover without improvement; search_dataset with and without the new keywords."""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import evolve_ref as ER
from tests import util
from tests.test_gpu_anneal import weighted
from tests.test_gpu_kway_search import batch_of, run_kanneal, spans, staged, vals_of
from tests.test_gpu_rounding import RawBatch, small_model
from tests.test_refine_host import handles_of

pytestmark = pytest.mark.gpu

GARBAGE = -5
SEED = 0xC0FFEE12345


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


class SkippingBatch(RawBatch):
    """A RawBatch whose FIRST graph has fewer than K nodes: gmc_round_order_host refuses such a batch, so the order
    arrays are those of the other graphs with an empty entry for the first in front (the kernels skip it unread)."""

    def refine_order(self, K=3):
        if K not in self._orders:
            assert self.handles[0].n < K <= min(h.n for h in self.handles[1:])
            rest = RawBatch.__new__(RawBatch)
            rest.__dict__.update(self.__dict__)
            n0 = self.handles[0].n
            rest.B, rest.R = self.B - 1, self.R - n0
            rest.goff_host = self.goff_host[1:] - n0
            rest.rowptr_host = self.rowptr_host[n0:] - self.rowptr_host[n0]
            rest.lcol_host = self.lcol_host[self.rowptr_host[n0]:]
            rest._orders = {}
            order, cgoff, cptr = (t.cpu().numpy() for t in RawBatch.refine_order(rest, K))
            order = np.concatenate([order + n0, np.zeros(n0, np.int32)]).astype(np.int32)
            cptr = np.concatenate([[0], cptr]).astype(np.int32)
            cgoff = np.concatenate([[0], cgoff + 1]).astype(np.int32)
            self._orders[K] = tuple(torch.from_numpy(a).cuda() for a in (order, cgoff, cptr))
        return self._orders[K]


@functools.lru_cache(maxsize=None)
def graph_set(name, K):
    """(graphs, gmc_refine_anneal_staged of their batch)"""
    return {
        "edges": lambda: ([nx.complete_graph(K), nx.complete_graph(K + 1), util.near_regular(65, 3, 65, attrs=False),
                           util.near_regular(257, 7, 257, attrs=False)], 1),
        "small": lambda: ([R.regular_graph(60, 5, 1)], 1),
        "batch": lambda: ([nx.complete_graph(K - 1), R.regular_graph(60, 7, 60), util.near_regular(97, 3, 97, attrs=False)], 1),
        "staged": lambda: ([R.regular_graph(300, 7, 8)], 1),
        "global": lambda: ([nx.complete_graph(150)], 0),
        "weights_staged": lambda: ([weighted(R.regular_graph(300, 7, 15), "int", 1)], 1),
        "weights_global": lambda: ([weighted(R.regular_graph(1000, 7, 19), "int", 5)], 0),
    }[name]()


def make_batch(pkg, name, K):
    graphs, fits = graph_set(name, K)
    if name == "batch":
        hs = handles_of(graphs)
        batch = SkippingBatch(pkg, hs)
    else:
        hs, batch = batch_of(pkg, graphs)
    assert staged(pkg, batch) == fits, name
    return hs, batch


def population(batch, K, cands, seed):
    """[cands, R] int8: per graph three base partitions under random renamings of the classes with a fifth of the
    nodes redrawn (members that mostly agree up to class names, what the alignment is for); terminals 0..K-1."""
    rng = np.random.RandomState(seed)
    A = np.empty((cands, batch.R), np.int8)
    for lo, hi in spans(batch):
        n = hi - lo
        bases = rng.randint(0, K, (3, n))
        for i in range(cands):
            a = rng.permutation(K)[bases[i % 3]]
            redraw = rng.rand(n) < 0.2
            a[redraw] = rng.randint(0, K, int(redraw.sum()))
            a[:min(K, n)] = np.arange(min(K, n))
            A[i, lo:hi] = a
    return A


def run_evolve(pkg, batch, K, pop0, generations, elite, inv_temp, seed, max_descent, want_history=True):
    """gmc_kway_evolve_f32 on pop0 [cands, R] int8; plane 1, both planes of cut and every output pre-filled with
    garbage (plane 0 of cut with a finite one: the call must not trust it)."""
    hip = pkg.hip
    cands = pop0.shape[0]
    order, cgoff, cptr = batch.refine_order(K)
    pop = torch.full((2, cands, batch.R), GARBAGE, dtype=torch.int8, device="cuda")
    pop[0] = torch.from_numpy(np.ascontiguousarray(pop0)).cuda()
    cut = torch.full((2, batch.B, cands), float("nan"), device="cuda")
    cut[0] = 1e9
    inv_t = torch.from_numpy(np.asarray(inv_temp, np.float32)).cuda() if len(inv_temp) else None
    lv = torch.from_numpy(AR.levels()).cuda() if len(inv_temp) else None
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    history = torch.full((generations + 1, batch.B), float("nan"), device="cuda") if want_history else None
    p = hip.ptr
    rc = hip.load().gmc_kway_evolve_f32(batch.ref(), K, p(order), p(cgoff), p(cptr), cands, p(pop), p(cut), generations,
                                        elite, p(inv_t), len(inv_temp), p(lv), seed, max_descent, p(best_assign),
                                        p(best_cut), p(best_idx), p(history), hip.stream())
    hip.check(rc, "gmc_kway_evolve_f32")
    torch.cuda.synchronize()
    out = dict(pop=pop, cut=cut, best_assign=best_assign, best_cut=best_cut, best_idx=best_idx)
    if want_history:
        out["history"] = history
    return {k: v.cpu().numpy() for k, v in out.items()}


def schedule_for(batch, sweeps):
    scale = 1.0 if vals_of(batch) is None else float(vals_of(batch).mean())
    return AR.schedule(sweeps, t_start=0.6, scale=scale)


def compare(got, hs, batch, K, pop0, generations, elite, inv_t, seed, descent):
    """Every output of every graph against the restatement, byte for byte; what a skipped graph owns stays garbage."""
    for g, (h, (lo, hi)) in enumerate(zip(hs, spans(batch))):
        if h.n < K:
            assert (got["pop"][1, :, lo:hi] == GARBAGE).all() and (got["pop"][0, :, lo:hi] == pop0[:, lo:hi]).all()
            assert (got["cut"][0, g] == np.float32(1e9)).all() and np.isnan(got["cut"][1, g]).all()
            assert (got["best_assign"][lo:hi] == GARBAGE).all() and np.isnan(got["best_cut"][g])
            assert got["best_idx"][g] == GARBAGE and np.isnan(got["history"][:, g]).all()
            continue
        ref = ER.evolve(h.n, h.rowptr, h.col, h.weight, pop0[:, lo:hi], K, generations, elite, inv_t, AR.levels(), seed,
                        descent)
        where = (g, h.n)
        assert got["pop"][0, :, lo:hi].tobytes() == ref.pop[0].tobytes(), where
        assert got["cut"][0, g].tobytes() == ref.cut[0].tobytes(), where
        if ref.written:
            assert got["pop"][1, :, lo:hi].tobytes() == ref.pop[1].tobytes(), where
            assert got["cut"][1, g].tobytes() == ref.cut[1].tobytes(), where
        else:
            assert (got["pop"][1, :, lo:hi] == GARBAGE).all() and np.isnan(got["cut"][1, g]).all()
        assert got["best_assign"][lo:hi].tobytes() == ref.best_assign.tobytes(), where
        assert got["best_cut"][g].tobytes() == ref.best_cut.tobytes() and got["best_idx"][g] == ref.best_idx, where
        assert got["history"][:, g].tobytes() == ref.history.tobytes(), where
        assert (np.diff(ref.history) >= 0).all()


@pytest.mark.parametrize("case", ER.CASES, ids=lambda c: "-".join(str(x) for x in c))
def test_evolution_matches_the_restatement(pkg, case):
    K = case.K
    hs, batch = make_batch(pkg, case.graphs, K)
    pop0 = population(batch, K, case.cands, seed=K + case.cands)
    inv_t = schedule_for(batch, case.sweeps)
    args = (K, pop0, case.generations, case.elite, inv_t, SEED + K, case.descent)
    got = run_evolve(pkg, batch, *args)
    compare(got, hs, batch, *args)
    bare = run_evolve(pkg, batch, *args, want_history=False)            # history = NULL changes nothing else
    for k in bare:
        assert bare[k].tobytes() == got[k].tobytes(), k


def test_the_case_list_covers_the_promised_shapes():
    cs = ER.CASES
    assert {c.K for c in cs} >= {2, 3, 8} and {c.generations for c in cs} >= {0, 1, 3}
    assert {(c.cands, c.elite) for c in cs} >= {(1, 1), (2, 1), (2, 2), (70, 1), (70, 2), (70, 71)}
    assert any(c.sweeps == 0 and c.descent == 0 for c in cs) and any(c.graphs == "batch" for c in cs)
    assert {graph_set(c.graphs, c.K)[1] for c in cs} == {0, 1}
    sizes = {g.number_of_nodes() - c.K for c in cs for g in graph_set(c.graphs, c.K)[0]}
    assert {-1, 0, 1} <= sizes and {65, 257} <= {g.number_of_nodes() for g in graph_set("edges", 3)[0]}


@pytest.mark.parametrize("K", (2, 3, 8))
def test_parents_that_differ_by_class_names_give_the_child_a(pkg, K):
    """Crossover alone (no sweep of either kind): slot 1 is slot 0 with the classes renamed on the movable nodes, so
    either child is its own parent a; a third member that is no renaming shows the crossover does mix."""
    hs, batch = batch_of(pkg, [util.near_regular(257, 7, 257, attrs=False)])
    rng = np.random.RandomState(K)
    a = rng.randint(0, K, batch.R).astype(np.int8)
    a[:K] = np.arange(K)
    perm = np.roll(np.arange(K), 1)
    b = perm[a].astype(np.int8)
    b[:K] = np.arange(K)
    got = run_evolve(pkg, batch, K, np.stack([a, b]), 1, 2, [], SEED, 0)
    assert (got["pop"][1] == got["pop"][0]).all() and (got["cut"][1] == got["cut"][0]).all()
    compare(got, hs, batch, K, np.stack([a, b]), 1, 2, [], SEED, 0)
    other = rng.randint(0, K, batch.R).astype(np.int8)
    other[:K] = np.arange(K)
    h = hs[0]
    for slot, (x, y) in enumerate([(a, other), (other, a)]):
        child = np.asarray(ER.child_of(x, y, K, ER.seeds(SEED, 1)[2], slot))
        assert (child != x).any() and (child != y).any()
        pi = ER.align(x.tolist(), y.tolist(), K)
        assert ((child == x) | (child == np.asarray([pi[int(c)] for c in y]))).all()
    mixed = run_evolve(pkg, batch, K, np.stack([a, other]), 1, 2, [], SEED, 0)
    compare(mixed, hs, batch, K, np.stack([a, other]), 1, 2, [], SEED, 0)
    assert h.n == 257


def test_bytes_of_no_class_and_foreign_terminals(pkg):
    """Bytes outside 0..K-1 on movable nodes of either parent and terminals that hold another class: the child gets
    the other parent's byte and its terminals are 0..K-1; a kept parent stays as it was."""
    K = 4
    hs, batch = batch_of(pkg, [R.regular_graph(100, 5, 3), util.near_regular(65, 3, 65, attrs=False)])
    pop0 = population(batch, K, 7, 9)
    pop0[0, 10], pop0[1, 10], pop0[2, 11], pop0[3, 120], pop0[4, 5] = K, -1, 100, K, -1
    pop0[5, :K] = 3
    pop0[6, 100:100 + K] = [1, 0, 3, 2]
    for sweeps, descent in ((0, 0), (4, 100)):
        inv_t = schedule_for(batch, sweeps)
        for elite in (1, 7):
            got = run_evolve(pkg, batch, K, pop0, 2, elite, inv_t, SEED, descent)
            compare(got, hs, batch, K, pop0, 2, elite, inv_t, SEED, descent)


@pytest.mark.parametrize("K,name", [(4, "real_staged"), (8, "real_global")])
def test_real_weights_keep_the_invariants(pkg, K, name):
    """The replacement rests on block_cut's summation order there, so no byte-for-byte claim."""
    g = {"real_staged": lambda: weighted(R.regular_graph(300, 7, 21), "real", 7),
         "real_global": lambda: weighted(R.regular_graph(1000, 7, 23), "real", 9)}[name]()
    hs, batch = batch_of(pkg, [g])
    assert staged(pkg, batch) == (name == "real_staged")
    pop0 = population(batch, K, 33, 4)
    inv_t = schedule_for(batch, 10)
    runs = [run_evolve(pkg, batch, K, pop0, G, 8, inv_t, 11, 100) for G in (0, 1, 2, 3)]
    again = run_evolve(pkg, batch, K, pop0, 3, 8, inv_t, 11, 100)
    for k in again:
        assert again[k].tobytes() == runs[3][k].tobytes(), k           # two runs are byte-equal
    planes = [runs[0]["cut"][0, 0]] + [runs[G]["cut"][G & 1, 0] for G in (1, 2, 3)]
    for G in (1, 2, 3):                                                 # a run of G generations goes through those of G - 1
        assert runs[G]["cut"][(G - 1) & 1, 0].tobytes() == planes[G - 1].tobytes()
        assert (planes[G] >= planes[G - 1]).all()                      # a slot's cut never falls (the same fp32 count)
        assert runs[G]["history"][:G, 0].tobytes() == runs[G - 1]["history"][:, 0].tobytes()
    assert (planes[3] > planes[0]).any()
    hist = runs[3]["history"][:, 0]
    assert (np.diff(hist) >= 0).all() and hist[3] == runs[3]["best_cut"][0] == planes[3].max()
    for G in (1, 2, 3):
        out = runs[G]["pop"][G & 1]
        assert (out[:, :K] == np.arange(K)).all() and ((out >= 0) & (out < K)).all()
        for i in range(out.shape[0]):
            recount = sum(d["weight"] for u, v, d in g.edges(data=True) if out[i, u] != out[i, v])
            # fp32 recount: at most deg + 8 roundings of 2^-24 each on sums of positive terms
            assert abs(float(planes[G][i]) - recount) <= 1e-5 * recount


def test_seed_and_batch_position(pkg):
    K = 5
    g = R.regular_graph(300, 7, 51)
    _h1, alone = batch_of(pkg, [g])
    _h3, third = batch_of(pkg, [R.regular_graph(100, 12, 52), nx.complete_graph(K), g, R.regular_graph(50, 3, 53)])
    pop0 = population(third, K, 9, 1)
    lo, hi = spans(third)[2]
    inv_t = AR.schedule(5, t_start=0.6)
    a = run_evolve(pkg, alone, K, pop0[:, lo:hi], 2, 3, inv_t, 3, 100)
    b = run_evolve(pkg, third, K, pop0, 2, 3, inv_t, 3, 100)
    assert a["pop"].tobytes() == np.ascontiguousarray(b["pop"][:, :, lo:hi]).tobytes()
    for k in ("best_cut", "best_idx"):
        assert a[k][0] == b[k][2]
    assert a["cut"][:, 0].tobytes() == b["cut"][:, 2].tobytes() and a["history"][:, 0].tobytes() == b["history"][:, 2].tobytes()
    c = run_evolve(pkg, third, K, pop0, 2, 3, inv_t, 4, 100)
    assert (b["pop"][0] != c["pop"][0]).any()
    high = run_evolve(pkg, third, K, pop0, 2, 3, inv_t, 3 + (1 << 63), 100)   # the whole 64-bit seed reaches the hash
    assert (b["pop"][0] != high["pop"][0]).any()


def test_the_annealing_call_is_unchanged_by_an_evolve_call_on_the_stream(pkg):
    K = 4
    hs, batch = batch_of(pkg, [R.regular_graph(300, 7, 61), weighted(R.regular_graph(200, 6, 62), "int", 1)])
    A = np.random.RandomState(2).randint(0, K, (5, batch.R)).astype(np.int8)
    inv_t = AR.schedule(10, scale=float(batch.host.vals.mean()))
    before = run_kanneal(pkg, batch, K, A, inv_t, 8, 100)
    run_evolve(pkg, batch, K, before["assign"], 2, 2, schedule_for(batch, 4), 8, 100)
    after = run_kanneal(pkg, batch, K, A, inv_t, 8, 100)
    for k in before:
        assert before[k].tobytes() == after[k].tobytes(), k


def test_probe_shows_the_launches_under_existing_tags(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(100, 5, 71)])
    pop0 = population(batch, 4, 4, 3)
    with pkg.hip.Probe(8) as pr:
        run_evolve(pkg, batch, 4, pop0, 3, 2, AR.schedule(2), 0, 10)
        run_evolve(pkg, batch, 4, pop0, 0, 2, [], 0, 10)
    assert [t for t, _ms in pr.records] == ["sample", "anneal", "anneal", "anneal", "sample"]


# ---- the Python API ---------------------------------------------------------------------------------------------------
def test_search_dataset_with_and_without_generations(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    K = 4
    net, ds = small_model(pkg, K, [(60, 5, 61), (48, 6, 62), (100, 7, 63)], 128, 16, seed=K)
    kw = dict(samples=20, sample_seed=5, anneal_sweeps=20, anneal_seed=2)
    plain = TN.search_dataset(net, ds, **kw)
    zero = TN.search_dataset(net, ds, **kw, generations=0, generation_sweeps=7, elite=3)
    assert repr(zero) == repr(plain)                                    # key for key, value for value, type for type
    evolved = TN.search_dataset(net, ds, **kw, generations=2, generation_sweeps=5)
    for res, base, (handle, _a_pad, nx_g, _t) in zip(evolved, plain, ds.values()):
        assert set(res) == set(base) | {"evolved_cut", "evolved_assignment", "evolved_history"}
        assert repr({k: res[k] for k in base}) == repr(base)          # no other key changes
        a = res["evolved_assignment"]
        assert res["evolved_cut"] == TN.calculate_cut_value(a, nx_g) >= res["searched_cut"]
        assert a[:K] == list(range(K)) and 0 <= min(a) and max(a) < K and len(a) == handle.n
        hist = res["evolved_history"]
        assert len(hist) == 3 and hist[0] == res["searched_cut"] and hist[-1] == res["evolved_cut"]
        assert hist == sorted(hist)


def test_kway_evolution_on_one_graph(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    K = 3
    g = R.regular_graph(60, 5, 1)
    hs, batch = batch_of(pkg, [g])
    pop0 = population(batch, K, 7, 5)
    assign, cut, history = TN.kway_evolution(pop0.tolist(), g, K, generations=2, generation_sweeps=4, seed=9)
    h = hs[0]
    ref = ER.evolve(h.n, h.rowptr, h.col, h.weight, pop0, K, 2, max(2, 7 // 4), AR.schedule(4, t_start=0.6), AR.levels(),
                    9, 100)
    assert assign == ref.best_assign.tolist() and cut == float(ref.best_cut) == TN.calculate_cut_value(assign, g)
    assert history == ref.history.tolist()
    kept, cut0, hist0 = TN.kway_evolution(pop0, g, K, generations=0)
    cuts = AR.cuts_f32(h.rowptr, h.col, h.weight, pop0)
    best = int(np.argmax(cuts))
    assert kept == pop0[best].tolist() and cut0 == float(cuts[best]) == history[0] and hist0 == [cut0]
