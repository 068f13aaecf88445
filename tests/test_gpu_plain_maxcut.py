"""GPU tests of the decoders with the terminals optional (include/gcnmaxcut.h, "plain max-K-cut"; round.hip,
kway_search.hip, large_round.hip, large_search.hip) against tests/plain_ref.py.

Every comparison is byte for byte: assignments, cuts, picks and sweep counts.  The weights are unit or small integers,
so every float32 sum of them is exact in any order and a cut is the same number however it is summed; the rounding's
sums are products with probabilities, taken by device and restatement alike in the CSR order of the row.  Only the
expected cut (one float32 sum over a whole graph against float64) is compared within a bar: test_rounding_host.SLACK
of the graph's absolute weight.

Shapes: graphs of 3, K, K + 1, 5, 65, 257 and 300 nodes (3 where K is below it: a batch takes graphs of at least three
nodes) and the star of 70 leaves whose centre is node 2 - its row has more than 64 entries - in ONE batch, so every
graph also sits between others; for the large entry points the same batch plus a graph of 4100 nodes, which takes the
wide counter.  With terminals the graphs below K nodes are left out (they are refused)."""
import ctypes as C
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from tests import anneal_ref as AR
from tests import large_ref as LR
from tests import large_search_ref as LS
from tests import plain_ref as PR
from tests import seeded_ref as SR
from tests.test_gpu_large_rounding import LargeBatch
from tests.test_rounding_host import SLACK

pytestmark = pytest.mark.gpu

GARBAGE = -5
KS_ = (2, 3, 4, 8)
WEIGHTS = ("unit", "integer")
SEED, ITERS, CANDS, SWEEPS, DESCENT = 11, 7, 3, 5, 40


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


@functools.lru_cache(maxsize=None)
def graphs_of(K, weights, terminals, big=False):
    """[(n, rowptr, col, w)] of the batch."""
    sizes = [3, max(K, 3), K + 1, 5, 65, 257, 300]
    if terminals:
        sizes = [n for n in sizes if n >= K]
    out = [PR.ring_with_chords(n, 20 + i) for i, n in enumerate(sizes)]
    out.insert(2, PR.star_centre2(70))
    if big:
        out.insert(1, LR.circulant(4100, 5, 3))
    return tuple((n, rp, cl, PR.integer_weights(n, rp, cl, 3 + i) if weights == "integer" else None)
                 for i, (n, rp, cl) in enumerate(out))


@functools.lru_cache(maxsize=None)
def probabilities(K, R):
    P = PR.softmax_rows(R, K, 77 + K)
    P.setflags(write=False)
    return P


class Batch(LargeBatch):
    """LargeBatch (tests/test_gpu_large_rounding.py) whose order arrays come from gmc_order_host_t."""

    def order_t(self, K, terminals):
        key = (K, terminals)
        if key not in self._large_orders:
            order = np.zeros(max(self.R, 1), np.int32)
            cgoff = np.zeros(self.B + 1, np.int32)
            cptr = np.zeros(self.R + self.B, np.int32)
            most = C.c_int32(-1)
            p = lambda a: a.ctypes.data_as(C.c_void_p)
            go = self.goff_host.astype(np.int32)
            rc = self._lib.gmc_order_host_t(self.B, p(go), p(self.rowptr_host), p(self.lcol_host), K, terminals, p(order),
                                            p(cgoff), p(cptr), cptr.size, C.byref(most))
            assert rc == 0, rc
            self._large_orders[key] = tuple(torch.from_numpy(a).cuda() for a in (order, cgoff, cptr)) + (most.value,)
        return self._large_orders[key]


def batch_of(pkg, graphs):
    from gcn_max_cut_amd.graph import GraphHandle
    return Batch(pkg, [GraphHandle(n, rp, cl, w) for n, rp, cl, w in graphs])


def call(pkg, name, t, head, tail):
    """Entry point `name` (t None), or its `_t` twin with terminals = t after `head`."""
    lib = pkg.hip.load()
    if t is None:
        pkg.hip.check(getattr(lib, name)(*head, *tail), name)
    else:
        twin = name[:-len("_f32")] + "_t_f32"
        pkg.hip.check(getattr(lib, twin)(*head, t, *tail), twin)
    torch.cuda.synchronize()


def full(shape, value, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device="cuda")


def host(**tensors):
    return {k: v.cpu().numpy() for k, v in tensors.items()}


def ws_round(pkg, batch, K):
    need = pkg.hip.load().gmc_large_round_workspace_bytes(batch.ref(), K)
    assert need > 0
    return full((need,), 0xA5, torch.uint8)


def ws_search(pkg, batch, K, cands):
    need = pkg.hip.load().gmc_large_search_workspace_bytes(batch.ref(), K, cands)
    assert need > 0
    return full((need,), 0xA5, torch.uint8)


# every runner pre-fills its outputs (and the workspace) with garbage: NaN cuts, -5 classes and counts
def run_round(pkg, batch, P, K, t, descent, large=False):
    p = pkg.hip.ptr
    order, cgoff, cptr, most = batch.order_t(K, 1 if t is None else t)
    Pd = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    assign, cut = full((batch.R,), GARBAGE, torch.int8), full((batch.B,), float("nan"))
    expected, sweeps = full((batch.B,), float("nan")), full((batch.B,), GARBAGE, torch.int32)
    if large:
        ws = ws_round(pkg, batch, K)
        call(pkg, "gmc_large_round_conditional_f32", t, (batch.ref(), p(Pd), K),
             (p(order), p(cgoff), p(cptr), most, descent, p(ws), ws.numel(), p(assign), p(cut), p(expected), p(sweeps),
              pkg.hip.stream()))
    else:
        call(pkg, "gmc_round_conditional_f32", t, (batch.ref(), p(Pd), K),
             (p(order), p(cgoff), p(cptr), descent, p(assign), p(cut), p(expected), p(sweeps), pkg.hip.stream()))
    return host(assign=assign, cut=cut, expected=expected, sweeps=sweeps)


def run_sample(pkg, batch, P, K, t, keys, iters, large=False):
    p = pkg.hip.ptr
    Pd = torch.from_numpy(np.ascontiguousarray(P)).cuda()
    gkey = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()
    assign_all = full((iters, batch.R), GARBAGE, torch.int8)
    cut_all, best_cut = full((batch.B, iters), float("nan")), full((batch.B,), float("nan"))
    best_assign, best_iter = full((batch.R,), GARBAGE, torch.int32), full((batch.B,), GARBAGE, torch.int32)
    if large:
        ws = ws_search(pkg, batch, K, iters)
        call(pkg, "gmc_large_sample_seeded_f32", t, (batch.ref(), p(Pd), K),
             (p(gkey), iters, p(assign_all), p(ws), ws.numel(), p(cut_all), p(best_assign), p(best_cut), p(best_iter),
              pkg.hip.stream()))
    else:
        call(pkg, "gmc_kway_decode_sample_seeded_f32", t, (batch.ref(), p(Pd), K),
             (p(gkey), iters, p(assign_all), p(cut_all), p(best_assign), p(best_cut), p(best_iter), pkg.hip.stream()))
    return host(assign_all=assign_all, cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_iter=best_iter)


def run_anneal(pkg, batch, K, t, A, inv_temp, seed, descent, large=False):
    p = pkg.hip.ptr
    cands = A.shape[0]
    order, cgoff, cptr, most = batch.order_t(K, 1 if t is None else t)
    assign = torch.from_numpy(np.array(A, np.int8)).cuda()
    inv_t = torch.from_numpy(np.asarray(inv_temp, np.float32)).cuda() if len(inv_temp) else None
    lv = torch.from_numpy(AR.levels()).cuda() if len(inv_temp) else None
    cut_all, best_cut = full((batch.B, cands), float("nan")), full((batch.B,), float("nan"))
    best_assign, best_idx = full((batch.R,), GARBAGE, torch.int32), full((batch.B,), GARBAGE, torch.int32)
    snap, sweeps = full((batch.B, cands), GARBAGE, torch.int32), full((batch.B, cands), GARBAGE, torch.int32)
    if large:
        ws = ws_search(pkg, batch, K, cands)
        call(pkg, "gmc_large_anneal_f32", t, (batch.ref(), K),
             (p(order), p(cgoff), p(cptr), most, cands, p(assign), p(inv_t), len(inv_temp), p(lv), seed, descent, p(ws),
              ws.numel(), p(cut_all), p(best_assign), p(best_cut), p(best_idx), p(snap), p(sweeps), pkg.hip.stream()))
    else:
        call(pkg, "gmc_kway_refine_anneal_f32", t, (batch.ref(), K),
             (p(order), p(cgoff), p(cptr), cands, p(assign), p(inv_t), len(inv_temp), p(lv), seed, descent, p(cut_all),
              p(best_assign), p(best_cut), p(best_idx), p(snap), p(sweeps), pkg.hip.stream()))
    return host(assign=assign, cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_idx=best_idx, snap=snap,
                sweeps=sweeps)


def run_local(pkg, batch, K, t, A, max_sweeps):
    """gmc_large_local_search_f32 / _t on A [R] int8."""
    p = pkg.hip.ptr
    order, cgoff, cptr, most = batch.order_t(K, 1 if t is None else t)
    ws = ws_round(pkg, batch, K)
    assign = torch.from_numpy(np.array(A, np.int8)).cuda()
    cut, sweeps = full((batch.B,), float("nan")), full((batch.B,), GARBAGE, torch.int32)
    call(pkg, "gmc_large_local_search_f32", t, (batch.ref(), K),
         (p(order), p(cgoff), p(cptr), most, max_sweeps, p(ws), ws.numel(), p(assign), p(cut), p(sweeps), pkg.hip.stream()))
    return host(assign=assign, cut=cut, sweeps=sweeps)


def same_bytes(a, b, what):
    assert sorted(a) == sorted(b)
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), (what, k)


def starts(batch, K, cands, first, seed=5):
    """[cands, R] int8: random classes, local ids below `first` in their own class, two bytes of no class."""
    A = np.random.RandomState(seed).randint(0, K, (cands, batch.R)).astype(np.int8)
    for g in range(batch.B):
        r0, n = int(batch.goff_host[g]), int(batch.sizes[g])
        A[:, r0:r0 + min(first, n)] = np.arange(min(first, n), dtype=np.int8)
        if n > first + 2:
            A[0, r0 + n - 1], A[0, r0 + first + 1] = K, -1
    return A


# ---- terminals = 1 is the existing entry point, byte for byte ---------------------------------------------------------
@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("K", KS_)
def test_with_terminals_every_twin_returns_the_bytes_of_its_entry_point(pkg, K, weights):
    batch = batch_of(pkg, graphs_of(K, weights, True))
    P = probabilities(K, batch.R)
    keys = SR.keys(SEED, range(batch.B))
    A = starts(batch, K, CANDS, K)
    inv_t = LS.schedule(SWEEPS)
    for large in (False, True):
        what = (K, weights, large)
        for descent in (0, DESCENT):
            same_bytes(run_round(pkg, batch, P, K, 1, descent, large), run_round(pkg, batch, P, K, None, descent, large), what)
        same_bytes(run_sample(pkg, batch, P, K, 1, keys, ITERS, large), run_sample(pkg, batch, P, K, None, keys, ITERS, large),
                   what)
        for schedule in (inv_t, []):
            same_bytes(run_anneal(pkg, batch, K, 1, A, schedule, SEED, DESCENT, large),
                       run_anneal(pkg, batch, K, None, A, schedule, SEED, DESCENT, large), what)
    same_bytes(run_local(pkg, batch, K, 1, A[1], DESCENT), run_local(pkg, batch, K, None, A[1], DESCENT), (K, weights))
    # the large twins once more with a graph of 4100 nodes in the batch: the wide counter with first = K
    batch = batch_of(pkg, graphs_of(K, weights, True, True))
    assert int(batch.sizes.max()) == 4100
    P = probabilities(K, batch.R)
    keys = SR.keys(SEED, range(batch.B))
    A = starts(batch, K, CANDS, K)
    what = (K, weights, "4100")
    for descent in (0, DESCENT):
        same_bytes(run_round(pkg, batch, P, K, 1, descent, True), run_round(pkg, batch, P, K, None, descent, True), what)
    same_bytes(run_sample(pkg, batch, P, K, 1, keys, ITERS, True), run_sample(pkg, batch, P, K, None, keys, ITERS, True), what)
    for schedule in (inv_t, []):
        same_bytes(run_anneal(pkg, batch, K, 1, A, schedule, SEED, DESCENT, True),
                   run_anneal(pkg, batch, K, None, A, schedule, SEED, DESCENT, True), what)
    same_bytes(run_local(pkg, batch, K, 1, A[1], DESCENT), run_local(pkg, batch, K, None, A[1], DESCENT), what)


# ---- terminals = 0 against the restatement ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def reference(K, weights, big=False):
    """plain_ref over every graph of the batch with first = 0, computed once: per graph the rounding (descent 0 and
    DESCENT), the expected cut, the samples, the annealing and the local search from `starts`."""
    graphs = graphs_of(K, weights, False, big)
    R = sum(g[0] for g in graphs)
    P = probabilities(K, R)
    sizes = np.asarray([g[0] for g in graphs], np.int64)

    class Shape:       # what `starts` reads of a batch
        pass
    shape = Shape()
    shape.B, shape.R, shape.sizes = len(graphs), R, sizes
    shape.goff_host = np.concatenate([[0], np.cumsum(sizes)])
    A = starts(shape, K, CANDS, 0)
    keys = SR.keys(SEED, range(len(graphs)))
    table, inv_t = AR.levels(), LS.schedule(SWEEPS)
    out, r0 = [], 0
    for g, (n, rp, cl, w) in enumerate(graphs):
        Pg = P[r0:r0 + n]
        tables = PR.tables_of(n, rp, cl, w, 0)
        a0 = PR.round_conditional(n, Pg, K, 0, tables)
        a1, sw = PR.descent(n, a0[None], K, tables, DESCENT)
        wide = big and n > LS.SMALL_NODES
        out.append(dict(
            a0=a0, a1=a1[0], sweeps=int(sw[0]), expected=PR.expected_cut(n, rp, cl, w, Pg, K, 0),
            sample=PR.sample(n, rp, cl, w, Pg, int(keys[g]), ITERS, 0),
            anneal=PR.anneal(n, rp, cl, w, A[:, r0:r0 + n], K, 0, inv_t, table, SEED, DESCENT, wide_layout=wide, tables=tables),
            local=PR.anneal(n, rp, cl, w, A[:, r0:r0 + n], K, 0, [], table, 0, DESCENT, tables=tables)))
        r0 += n
    return graphs, A, out


def check_round(got, graphs, ref, descent):
    r0 = 0
    for g, ((n, rp, cl, w), want) in enumerate(zip(graphs, ref)):
        a = want["a1"] if descent else want["a0"]
        assert np.array_equal(got["assign"][r0:r0 + n], a), g
        assert got["cut"][g] == np.float32(PR.cut(rp, cl, w, a)), g
        assert got["sweeps"][g] == (want["sweeps"] if descent else 0), g
        w_abs = float(cl.size if w is None else np.abs(w).sum()) / 2
        assert abs(float(got["expected"][g]) - want["expected"]) <= SLACK * w_abs, g
        r0 += n


def check_sample(got, graphs, ref):
    r0 = 0
    for g, ((n, _rp, _cl, _w), want) in enumerate(zip(graphs, ref)):
        s = want["sample"]
        assert np.array_equal(got["assign_all"][:, r0:r0 + n], s["assign_all"]), g
        assert got["cut_all"][g].tobytes() == s["cut_all"].tobytes(), g
        assert np.array_equal(got["best_assign"][r0:r0 + n], s["best_assign"]), g
        assert got["best_cut"][g] == s["best_cut"] and got["best_iter"][g] == s["best_iter"], g
        r0 += n


def check_search(got, graphs, ref, key):
    r0 = 0
    for g, ((n, _rp, _cl, _w), want) in enumerate(zip(graphs, ref)):
        s = want[key]
        assert np.array_equal(got["assign"][:, r0:r0 + n], s["assign"]), (key, g)
        assert got["cut_all"][g].tobytes() == s["cut_all"].tobytes(), (key, g)
        assert np.array_equal(got["snap"][g], s["snap"]) and np.array_equal(got["sweeps"][g], s["sweeps"]), (key, g)
        assert np.array_equal(got["best_assign"][r0:r0 + n], s["best_assign"]), (key, g)
        assert got["best_cut"][g] == s["best_cut"] and got["best_idx"][g] == s["best_idx"], (key, g)
        r0 += n


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("K", KS_)
def test_without_terminals_the_one_workgroup_decoders_are_the_restatement(pkg, K, weights):
    graphs, A, ref = reference(K, weights)
    batch = batch_of(pkg, graphs)
    P = probabilities(K, batch.R)
    keys = SR.keys(SEED, range(batch.B))
    assert int(batch.sizes.min()) == 3 and (K <= 3 or int(batch.sizes.min()) < K)
    runs = []
    for _ in range(2):
        r0, r1 = run_round(pkg, batch, P, K, 0, 0), run_round(pkg, batch, P, K, 0, DESCENT)
        smp = run_sample(pkg, batch, P, K, 0, keys, ITERS)
        ann = run_anneal(pkg, batch, K, 0, A, LS.schedule(SWEEPS), SEED, DESCENT)
        loc = run_anneal(pkg, batch, K, 0, A, [], 0, DESCENT)
        runs.append((r0, r1, smp, ann, loc))
    for a, b in zip(*runs):                                             # two runs: the same bytes
        same_bytes(a, b, (K, weights))
    r0, r1, smp, ann, loc = runs[0]
    check_round(r0, graphs, ref, 0)
    check_round(r1, graphs, ref, DESCENT)
    check_sample(smp, graphs, ref)
    check_search(ann, graphs, ref, "anneal")
    check_search(loc, graphs, ref, "local")
    # no node is fixed: a converged descent leaves no improving move of ANY node, the first K included
    off = 0
    for g, (n, rp, cl, w) in enumerate(graphs):
        for assign, sweeps in ((r1["assign"][off:off + n], r1["sweeps"][g]), (loc["assign"][1, off:off + n], loc["sweeps"][g, 1])):
            assert sweeps < DESCENT
            assert PR.best_single_move_gain(n, rp, cl, w, assign, K, 0) == 0.0, g
        off += n
    # ... and the draws move the first K nodes too
    first = smp["assign_all"][:, :min(K, 3)]
    assert not (first == np.arange(first.shape[1])).all()


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("K", KS_)
def test_without_terminals_the_large_entry_points_are_the_one_workgroup_ones(pkg, K, weights):
    graphs, A, _ref = reference(K, weights)
    batch = batch_of(pkg, graphs)
    P = probabilities(K, batch.R)
    keys = SR.keys(SEED, range(batch.B))
    w_abs = np.asarray([float(cl.size if w is None else np.abs(w).sum()) / 2 for _n, _rp, cl, w in graphs])
    for descent in (0, DESCENT):
        big, one = run_round(pkg, batch, P, K, 0, descent, large=True), run_round(pkg, batch, P, K, 0, descent)
        # (the expected cut is one float32 sum per graph, folded by tiles there and by waves here: a bar, not bytes)
        assert (np.abs(big.pop("expected") - one.pop("expected")) <= SLACK * w_abs).all()
        same_bytes(big, one, descent)
    same_bytes(run_sample(pkg, batch, P, K, 0, keys, ITERS, large=True), run_sample(pkg, batch, P, K, 0, keys, ITERS), "sample")
    for schedule in (LS.schedule(SWEEPS), []):
        same_bytes(run_anneal(pkg, batch, K, 0, A, schedule, SEED, DESCENT, large=True),
                   run_anneal(pkg, batch, K, 0, A, schedule, SEED, DESCENT), len(schedule))
    small = run_anneal(pkg, batch, K, 0, A[1:2], [], 0, DESCENT)
    large = run_local(pkg, batch, K, 0, A[1], DESCENT)
    assert np.array_equal(large["assign"], small["assign"][0]) and np.array_equal(large["cut"], small["cut_all"][:, 0])
    assert np.array_equal(large["sweeps"], small["sweeps"][:, 0])


@pytest.mark.parametrize("weights", WEIGHTS)
@pytest.mark.parametrize("K", KS_)
def test_without_terminals_at_4100_nodes_the_large_entry_points_are_the_restatement(pkg, K, weights):
    graphs, A, ref = reference(K, weights, big=True)
    batch = batch_of(pkg, graphs)
    assert int(batch.sizes.max()) == 4100
    P = probabilities(K, batch.R)
    keys = SR.keys(SEED, range(batch.B))
    check_round(run_round(pkg, batch, P, K, 0, 0, large=True), graphs, ref, 0)
    check_round(run_round(pkg, batch, P, K, 0, DESCENT, large=True), graphs, ref, DESCENT)
    check_sample(run_sample(pkg, batch, P, K, 0, keys, ITERS, large=True), graphs, ref)
    ann = run_anneal(pkg, batch, K, 0, A, LS.schedule(SWEEPS), SEED, DESCENT, large=True)
    check_search(ann, graphs, ref, "anneal")
    same_bytes(ann, run_anneal(pkg, batch, K, 0, A, LS.schedule(SWEEPS), SEED, DESCENT, large=True), "twice")
    check_search(run_anneal(pkg, batch, K, 0, A, [], 0, DESCENT, large=True), graphs, ref, "local")
    loc = run_local(pkg, batch, K, 0, A[1], DESCENT)
    off = 0
    for g, ((n, _rp, _cl, _w), want) in enumerate(zip(graphs, ref)):
        assert np.array_equal(loc["assign"][off:off + n], want["local"]["assign"][1]), g
        assert loc["sweeps"][g] == want["local"]["sweeps"][1] and loc["cut"][g] == want["local"]["cut_all"][1], g
        off += n


# ---- what the flag means ----------------------------------------------------------------------------------------------
def test_the_path_and_the_star_reach_their_optimum_only_without_terminals(pkg):
    """K = 2.  On the path 0 - 2 - 1 the optimum cuts both edges, on the star whose centre is node 2 all 70; with nodes 0
    and 1 forced apart one edge is lost whatever the rest does.  The start is all zeros (with terminals: node 1 in its
    own class, as every candidate of that problem has it)."""
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    path = nx.Graph([(0, 2), (2, 1)])
    star = nx.Graph([(2, v) for v in range(71) if v != 2])
    for graph, best in ((path, 2), (star, 70)):
        n = graph.number_of_nodes()
        for search in (TN.kway_local_search, TN.large_local_search):
            plain, cut = search([0] * n, graph, 2, terminals=False)
            assert cut == best and TN.calculate_cut_value(plain, graph) == best, (n, search.__name__)
            fixed, cut = search([0, 1] + [0] * (n - 2), graph, 2)
            assert cut == best - 1 and fixed[:2] == [0, 1], (n, search.__name__)
        P = np.full((n, 2), 0.5, np.float32)
        for rounding in (TN.conditional_rounding, TN.large_conditional_rounding):
            assert rounding(P, graph, 5, terminals=False)[1] == best
            assert rounding(P, graph, 5)[1] == best - 1
        assert TN.kway_annealing([0] * n, graph, 2, sweeps=5, terminals=False)[1] == best
        assert TN.large_annealing([0] * n, graph, 2, sweeps=5, terminals=False)[1] == best
        assert TN.sampling_optimization(P, graph, 64, seed=1, terminals=False)[1] <= best
        a, c = TN.sampling_optimization(P, graph, 8, seed=1, graph_index=3, terminals=False)
        b, d = TN.large_sampling_optimization(P, graph, 8, seed=1, graph_index=3, terminals=False)
        assert a == b and c == d
        host_form = [TN.assign_partitions_seeded_kway(P, 1, 3, it, terminals=False) for it in range(8)]
        assert a in host_form and c == max(TN.calculate_cut_value(h, graph) for h in host_form)


@pytest.mark.parametrize("K", (4, 8))
def test_a_batch_whose_largest_graph_is_below_K_runs_without_terminals(pkg, K):
    """n_max = 3 < K: refused with terminals (GMC_ERR_GRAPH_SIZE), and without them the one-workgroup and the large
    decoders run it - the path 0 - 2 - 1 twice, so the second graph starts off a tile - and equal the restatement."""
    n, rp, cl = PR.path_021()
    graphs = ((n, rp, cl, None), (n, rp, cl, None))
    batch = batch_of(pkg, graphs)
    assert int(batch.sizes.max()) == 3
    P = probabilities(K, batch.R)
    keys = SR.keys(SEED, range(batch.B))
    A = np.random.RandomState(K).randint(0, K, (CANDS, batch.R)).astype(np.int8)
    table, inv_t = AR.levels(), LS.schedule(SWEEPS)
    ref = []
    for g in range(2):
        Pg, Ag = P[3 * g:3 * g + 3], A[:, 3 * g:3 * g + 3]
        tables = PR.tables_of(n, rp, cl, None, 0)
        a0 = PR.round_conditional(n, Pg, K, 0, tables)
        a1, sw = PR.descent(n, a0[None], K, tables, DESCENT)
        ref.append(dict(a0=a0, a1=a1[0], sweeps=int(sw[0]), expected=PR.expected_cut(n, rp, cl, None, Pg, K, 0),
                        sample=PR.sample(n, rp, cl, None, Pg, int(keys[g]), ITERS, 0),
                        anneal=PR.anneal(n, rp, cl, None, Ag, K, 0, inv_t, table, SEED, DESCENT, tables=tables),
                        local=PR.anneal(n, rp, cl, None, Ag, K, 0, [], table, 0, DESCENT, tables=tables)))
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    scratch = [np.zeros(8, np.int32) for _ in range(3)]
    assert batch._lib.gmc_order_host_t(2, p(batch.goff_host.astype(np.int32)), p(batch.rowptr_host), p(batch.lcol_host), K, 1,
                                       p(scratch[0]), p(scratch[1]), p(scratch[2]), 8, C.byref(C.c_int32())) == -6
    batch._large_orders[(K, 1)] = batch.order_t(K, 0)    # (any arrays: the calls with terminals fail before they read them)
    for large in (False, True):
        with pytest.raises(ValueError, match="gmc error -6"):
            run_round(pkg, batch, P, K, 1, 0, large)
        with pytest.raises(ValueError, match="gmc error -6"):
            run_sample(pkg, batch, P, K, 1, keys, ITERS, large)
        with pytest.raises(ValueError, match="gmc error -6"):
            run_anneal(pkg, batch, K, 1, A, inv_t, SEED, DESCENT, large)
        check_round(run_round(pkg, batch, P, K, 0, 0, large), graphs, ref, 0)
        check_round(run_round(pkg, batch, P, K, 0, DESCENT, large), graphs, ref, DESCENT)
        check_sample(run_sample(pkg, batch, P, K, 0, keys, ITERS, large), graphs, ref)
        check_search(run_anneal(pkg, batch, K, 0, A, inv_t, SEED, DESCENT, large), graphs, ref, "anneal")
        check_search(run_anneal(pkg, batch, K, 0, A, [], 0, DESCENT, large), graphs, ref, "local")


# ---- the dataset functions ----------------------------------------------------------------------------------------------
def plain_model(K, seed):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    torch.manual_seed(seed)
    net, _embed, _opt = T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=64, hidden_dim=16, number_classes=K))
    net.eval()
    return net


@pytest.mark.parametrize("K", (2, 4, 8))
def test_dataset_functions_without_terminals(pkg, K):
    """round_dataset / search_dataset and their large twins with terminals=False on the path 0 - 2 - 1 (below K nodes at
    K = 4 and 8) and two graphs of 40 and 31 nodes: candidate 0 is the row argmax of P (first maximum) with its cut
    recounted on the host, the rounding, the samples and the search are the restatement's from the P of the same
    forward, and the large functions return what the one-workgroup ones return."""
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from tests.test_gpu_plain_instance import plain_dataset
    ds = plain_dataset(pkg, [3, 40, 31])
    ds[0][2].remove_edges_from(list(ds[0][2].edges()))
    ds[0][2].add_edges_from([(0, 2), (2, 1)])
    ds[0][0] = pkg.from_networkx(ds[0][2])                                  # the path, as handle and as graph
    net = plain_model(K, 7 + K)
    eng = net.engine()
    handles = [it[0] for it in ds.values()]
    batch = pkg.GraphBatch(handles, None, eng.device)
    if K > 3:
        with pytest.raises(ValueError, match="at least"):
            TN.round_dataset(net, ds)                                       # with terminals the path is refused
    P = eng.forward(batch, 1.0, terminals=False)[0].cpu().numpy()
    samples, sweeps = 6, 4
    table, inv_t = AR.levels(), TN.anneal_schedule(sweeps)
    keys = TN.sample_keys(3, range(len(ds)))
    for descent in (0, DESCENT):
        rounded = TN.round_dataset(net, ds, descent_sweeps=descent, terminals=False)
        large = TN.round_large_dataset(net, ds, descent_sweeps=descent, terminals=False)
        for g, (res, big, item) in enumerate(zip(rounded, large, ds.values())):
            h, nx_g = item[0], item[2]
            r0 = int(batch.goff_host[g])
            Pg = P[r0:r0 + h.n]
            assert res["simple_assignment"] == Pg.argmax(1).tolist(), g          # numpy: the first maximum
            assert res["simple_cut"] == TN.calculate_cut_value(res["simple_assignment"], nx_g), g
            want = PR.restate_round(h.n, h.rowptr, h.col, None, Pg, K, 0, descent)
            assert res["rounded_assignment"] == (want["a1"] if descent else want["a0"]).tolist(), g
            assert res["descent_sweeps"] == (want["sweeps"] if descent else 0), g
            assert res["rounded_cut"] == TN.calculate_cut_value(res["rounded_assignment"], nx_g), g
            assert abs(res["expected_cut"] - PR.expected_cut(h.n, h.rowptr, h.col, None, Pg, K, 0)) <= \
                SLACK * nx_g.number_of_edges(), g
            assert {k: v for k, v in big.items() if k != "expected_cut"} == \
                {k: v for k, v in res.items() if k != "expected_cut"}, g
            assert abs(big["expected_cut"] - res["expected_cut"]) <= SLACK * nx_g.number_of_edges(), g
    found = TN.search_dataset(net, ds, samples, sample_seed=3, anneal_sweeps=sweeps, anneal_seed=5, max_descent_sweeps=DESCENT,
                              terminals=False)
    large = TN.search_large_dataset(net, ds, samples, sample_seed=3, anneal_sweeps=sweeps, anneal_seed=5,
                                    max_descent_sweeps=DESCENT, terminals=False)
    for g, (res, big, item) in enumerate(zip(found, large, ds.values())):
        h, nx_g = item[0], item[2]
        r0 = int(batch.goff_host[g])
        Pg = P[r0:r0 + h.n]
        a0 = PR.restate_round(h.n, h.rowptr, h.col, None, Pg, K, 0, 0)["a0"]
        smp = PR.sample(h.n, h.rowptr, h.col, None, Pg, int(keys[g]), samples, 0)
        assert res["simple_assignment"] == Pg.argmax(1).tolist() and res["rounded_assignment"] == a0.tolist(), g
        assert res["post_assignment"] == smp["best_assign"].tolist() and res["post_cut"] == smp["best_cut"], g
        cands = np.concatenate([Pg.argmax(1).astype(np.int8)[None], a0[None], smp["assign_all"]])
        want = PR.anneal(h.n, h.rowptr, h.col, None, cands, K, 0, inv_t, table, 5, DESCENT)
        assert res["searched_assignment"] == want["best_assign"].tolist() and res["searched_from"] == want["best_idx"], g
        assert res["searched_cut"] == want["best_cut"] == TN.calculate_cut_value(res["searched_assignment"], nx_g), g
        assert res["searched_cut"] >= max(res["simple_cut"], res["rounded_cut"], res["post_cut"]), g
        assert {k: v for k, v in big.items() if k != "expected_cut"} == {k: v for k, v in res.items() if k != "expected_cut"}, g
    assert found[0]["searched_cut"] == 2                                    # the path: both edges, no node forced
    # the library's own bound stays: a dataset whose largest graph is below K is refused by the shared model's forward
    if K > 3:
        with pytest.raises(ValueError, match="gmc error -6"):
            TN.round_dataset(net, {0: ds[0]}, terminals=False)
