"""GPU tests of the K-class decoders (gmc_kway_decode_sample_seeded_f32, gmc_kway_refine_anneal_f32 and their Python
API) against the CPU restatement in tests/kway_search_ref.py: samples, assignments, cuts, the pick, snapshot sweeps and
descent sweeps byte for byte (unit, integer and dyadic weights: every fp32 sum is exact in any order); real-valued
weights by invariants; anneal_sweeps = 0 against the rounding's descent; K = 3 against the 3-class entry points; seeds,
batch position, the probe tags, and search_dataset on small trained models."""
import functools

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import kway_search_ref as KS
from tests import refine_ref as RR
from tests import rounding_ref as RO
from tests import seeded_ref as SR
from tests import util
from tests.test_gpu_anneal import run_anneal, weighted
from tests.test_gpu_refine import run_refine
from tests.test_gpu_rounding import RawBatch, run_round, small_model
from tests.test_gpu_seeded_sampler import run_seeded
from tests.test_refine_host import gnp_graph, handles_of, hub_graph, loop_graph

pytestmark = pytest.mark.gpu

GARBAGE = -5
KS_ = (2, 4, 5, 8)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def batch_of(pkg, graphs):
    """A GraphBatch; with a two-node graph (K = 2, n = K: nothing movable), which GraphBatch refuses, the RawBatch of
    tests/test_gpu_rounding.py."""
    from gcn_max_cut_amd.graph import GraphBatch
    hs = handles_of(graphs)
    if min(h.n for h in hs) < 3:
        return hs, RawBatch(pkg, hs)
    return hs, GraphBatch(hs, None, torch.device("cuda"))


def vals_of(batch):
    return batch.vals_host if isinstance(batch, RawBatch) else batch.host.vals


def spans(batch):
    return [(int(batch.goff_host[g]), int(batch.goff_host[g + 1])) for g in range(batch.B)]


def run_ksample(pkg, batch, P, keys, iters, keep=True):
    """gmc_kway_decode_sample_seeded_f32 with every output pre-filled with garbage; keep=False: assign_all = NULL."""
    hip = pkg.hip
    K = P.shape[1]
    Pt = torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda()
    gkey = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()
    assign_all = torch.full((iters, batch.R), GARBAGE, dtype=torch.int8, device="cuda") if keep else None
    cut_all = torch.full((batch.B, iters), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_iter = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_kway_decode_sample_seeded_f32(batch.ref(), p(Pt), K, p(gkey), iters, p(assign_all), p(cut_all),
                                                      p(best_assign), p(best_cut), p(best_iter), hip.stream())
    hip.check(rc, "gmc_kway_decode_sample_seeded_f32")
    torch.cuda.synchronize()
    out = dict(cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_iter=best_iter)
    if keep:
        out["assign_all"] = assign_all
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_kanneal(pkg, batch, K, A, inv_temp, seed, max_descent):
    """gmc_kway_refine_anneal_f32 on A [cands, R] int8 with every output pre-filled with garbage."""
    hip = pkg.hip
    cands = A.shape[0]
    order, cgoff, cptr = batch.refine_order(K)
    assign = torch.from_numpy(np.ascontiguousarray(A)).cuda()
    inv_t = torch.from_numpy(np.asarray(inv_temp, np.float32)).cuda() if len(inv_temp) else None
    lv = torch.from_numpy(AR.levels()).cuda() if len(inv_temp) else None
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    snap = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    sweeps = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_kway_refine_anneal_f32(batch.ref(), K, p(order), p(cgoff), p(cptr), cands, p(assign), p(inv_t),
                                               len(inv_temp), p(lv), seed, max_descent, p(cut_all), p(best_assign),
                                               p(best_cut), p(best_idx), p(snap), p(sweeps), hip.stream())
    hip.check(rc, "gmc_kway_refine_anneal_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut_all=cut_all, best_assign=best_assign,
                                                    best_cut=best_cut, best_idx=best_idx, snap=snap,
                                                    sweeps=sweeps).items()}


def staged(pkg, batch):
    return pkg.hip.load().gmc_refine_anneal_staged(batch.ref())


# ---- the sampler ------------------------------------------------------------------------------------------------------
def probabilities(n, K, seed):
    """softmax rows with, from node K on (where the graph has them): the K one-hot rows, an all-zero row, a NaN row;
    the terminals' rows hold NaN (they are never read)."""
    P = RO.softmax_rows(n, K, seed, scale=1.0)
    P[:K] = np.nan
    extra = [*np.eye(K, dtype=np.float32), np.zeros(K, np.float32), np.full(K, np.nan, np.float32)]
    for node, row in zip(range(K, n), extra):
        P[node] = row
    return P


def sampler_graph_sets(K):
    return {"nK": [nx.complete_graph(K)], "nK1": [nx.complete_graph(K + 1)], "n65": [util.near_regular(65, 3, 65)],
            "n257": [util.near_regular(257, 7, 257)],
            "batch": [R.regular_graph(60, 7, 60), util.near_regular(97, 3, 97), nx.complete_graph(K + 2)]}


@pytest.mark.parametrize("iters", (1, 7, 33))
@pytest.mark.parametrize("K", KS_)
def test_sampler_matches_the_restatement(pkg, K, iters):
    for name, graphs in sampler_graph_sets(K).items():
        hs, batch = batch_of(pkg, graphs)
        P = np.concatenate([probabilities(h.n, K, 100 * K + i) for i, h in enumerate(hs)])
        keys = SR.keys(7 + K, range(4, 4 + batch.B))
        got = run_ksample(pkg, batch, P, keys, iters)
        bare = run_ksample(pkg, batch, P, keys, iters, keep=False)
        for k in bare:
            assert bare[k].tobytes() == got[k].tobytes(), (name, k)
        for g, (h, (lo, hi)) in enumerate(zip(hs, spans(batch))):
            ref = KS.sample(h, P[lo:hi], keys[g], iters)
            assert (got["assign_all"][:, lo:hi] == ref["assign_all"]).all(), (name, g)
            assert got["cut_all"][g].tobytes() == ref["cut_all"].tobytes(), (name, g)
            assert (got["best_assign"][lo:hi] == ref["best_assign"]).all()
            assert got["best_cut"][g] == ref["best_cut"] and got["best_iter"][g] == ref["best_iter"]
            a = got["assign_all"][:, lo:hi]
            assert (a[:, :K] == np.arange(K)).all()
            for j in range(min(K, h.n - K)):
                assert (a[:, K + j] == j).all()                        # one-hot rows
            assert (a[:, 2 * K:2 * K + 2] == K - 1).all()              # the all-zero and the NaN row: the fallback


@pytest.mark.parametrize("K", KS_)
def test_samples_depend_on_the_key_alone(pkg, K):
    g = util.near_regular(97, 3, 97)
    _h1, alone = batch_of(pkg, [g])
    _h3, third = batch_of(pkg, [R.regular_graph(60, 7, 60), nx.complete_graph(K + 2), g])
    P = np.concatenate([probabilities(int(n), K, 5 + i) for i, n in enumerate(third.sizes)])
    lo, hi = spans(third)[2]
    keys = SR.keys(3, (9, 8, 7))
    a = run_ksample(pkg, alone, P[lo:hi], keys[2:], 7)
    b = run_ksample(pkg, third, P, keys, 7)
    long = run_ksample(pkg, third, P, keys, 33)
    assert (a["assign_all"] == b["assign_all"][:, lo:hi]).all() and (a["cut_all"][0] == b["cut_all"][2]).all()
    assert (a["best_assign"] == b["best_assign"][lo:hi]).all() and a["best_iter"][0] == b["best_iter"][2]
    assert (b["assign_all"][5] == long["assign_all"][5]).all() and (b["cut_all"][:, 5] == long["cut_all"][:, 5]).all()
    other = run_ksample(pkg, third, P, SR.keys(4, (9, 8, 7)), 7)
    assert (other["assign_all"] != b["assign_all"]).any()


# ---- the annealing ----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def anneal_graph_sets(K):
    """name -> (graphs, whether the batch's copy fits the LDS budget)"""
    return {
        "unit": ([nx.complete_graph(K), nx.complete_graph(K + 1), util.near_regular(65, 3, 65, attrs=False),
                  util.near_regular(257, 7, 257, attrs=False), R.regular_graph(300, 7, 8), gnp_graph(150, 0.1, 12),
                  hub_graph(300, 7, 13), loop_graph(120, 6, 14)], 1),
        "weights_staged": ([weighted(R.regular_graph(300, 7, 15), "int", 1), weighted(loop_graph(100, 5, 16), "dyadic", 2)], 1),
        "weights_global": ([weighted(R.regular_graph(1000, 7, 19), "int", 5)], 0),
    }


def check_against_restatement(pkg, K, graphs, cands, sweeps, seed, max_descent=100, expect_staged=None, no_class=()):
    """no_class: (candidate, batch row, byte) triples - class bytes outside 0..K-1 put on movable nodes."""
    hs, batch = batch_of(pkg, graphs)
    if expect_staged is not None:
        assert staged(pkg, batch) == expect_staged
    rng = np.random.RandomState(seed)
    A = rng.randint(0, K, (cands, batch.R)).astype(np.int8)
    for cand, row, byte in no_class:
        A[cand, row] = byte
    scale = 1.0 if vals_of(batch) is None else float(vals_of(batch).mean())
    inv_t = AR.schedule(sweeps, scale=scale)
    got = run_kanneal(pkg, batch, K, A, inv_t, seed, max_descent)
    assert np.isfinite(got["cut_all"]).all() and np.isfinite(got["best_cut"]).all()
    for g, (h, (lo, hi)) in enumerate(zip(hs, spans(batch))):
        ref, ref_snap, ref_sweeps = KS.anneal(h.n, h.rowptr, h.col, h.weight, A[:, lo:hi], K, inv_t, AR.levels(), seed,
                                              max_descent)
        assert (got["snap"][g] == ref_snap).all(), (g, h.n)
        assert (got["assign"][:, lo:hi] == ref).all(), (g, h.n, int((got["assign"][:, lo:hi] != ref).sum()))
        assert (got["sweeps"][g] == ref_sweeps).all()
        assert (got["cut_all"][g] == AR.cuts_f32(h.rowptr, h.col, h.weight, ref)).all()
        assert (got["assign"][:, lo:lo + K] == A[:, lo:lo + K]).all()
        if not no_class:                                                # (every edge of a byte of no class counts as cut)
            assert (got["cut_all"][g] >= AR.cuts_f32(h.rowptr, h.col, h.weight, A[:, lo:hi])).all()
        bi = int(np.argmax(got["cut_all"][g]))                          # first of the largest
        assert got["best_idx"][g] == bi and got["best_cut"][g] == got["cut_all"][g, bi]
        assert (got["best_assign"][lo:hi] == got["assign"][bi, lo:hi]).all()
    return got


@pytest.mark.parametrize("cands,sweeps", [(1, 30), (7, 30), (33, 10)])
@pytest.mark.parametrize("name", ("unit", "weights_staged", "weights_global"))
@pytest.mark.parametrize("K", KS_)
def test_annealing_matches_the_restatement(pkg, K, name, cands, sweeps):
    graphs, fits = anneal_graph_sets(K)[name]
    check_against_restatement(pkg, K, graphs, cands, sweeps, seed=K + cands, expect_staged=fits)


def test_the_matrix_runs_both_paths_of_the_kernel():
    assert {fits for _g, fits in anneal_graph_sets(4).values()} == {0, 1}


@pytest.mark.parametrize("name", ("unit", "weights_global"))
@pytest.mark.parametrize("K", KS_)
def test_a_byte_of_no_class_on_a_movable_node_moves_unconditionally(pkg, K, name):
    """Bytes K (2 at K = 2), -1 and 100 on movable nodes, two adjacent ones included, with and without a descent."""
    graphs, fits = anneal_graph_sets(K)[name]
    hs, batch = batch_of(pkg, graphs)
    g0 = len(hs) - 1 if name == "unit" else 0                           # the last graph of the unit batch, else the only one
    lo, hi = spans(batch)[g0]
    h = hs[g0]
    v = K + 5
    nb = next(int(u) for u in h.col[h.rowptr[v]:h.rowptr[v + 1]] if u >= K and u != v)
    no_class = [(0, lo + v, K), (0, lo + nb, -1), (2, lo + 50, 100), (3, hi - 1, K), (4, lo + K, K)]
    for max_descent in (100, 0):
        got = check_against_restatement(pkg, K, graphs, 7, 20, seed=17, max_descent=max_descent, expect_staged=fits,
                                        no_class=no_class)
        out = got["assign"][:, lo + K:hi]
        assert ((out >= 0) & (out < K)).all()                          # the first annealing sweep gives every node a class


@pytest.mark.parametrize("K", (2, 3, 8))
def test_no_annealing_sweeps_on_the_rounded_assignment_is_the_roundings_descent(pkg, K):
    graphs = [R.regular_graph(300, 7, 31), weighted(R.regular_graph(100, 5, 32), "real", 1), nx.complete_graph(K),
              loop_graph(120, 5, 33), hub_graph(300, 7, 34)]
    hs, batch = batch_of(pkg, graphs)
    P = np.concatenate([RO.softmax_rows(h.n, K, 40 + i) for i, h in enumerate(hs)])
    rounded = run_round(pkg, batch, P, K, 0)
    for d in (1, 100):
        want = run_round(pkg, batch, P, K, d)
        got = run_kanneal(pkg, batch, K, rounded["assign"][None, :].copy(), [], 0, d)
        assert (got["assign"][0] == want["assign"]).all() and (got["sweeps"][:, 0] == want["sweeps"]).all()
        assert got["cut_all"][:, 0].tobytes() == want["cut"].tobytes() and (got["snap"] == 0).all()


def test_three_classes_equal_the_three_class_entry_points(pkg):
    graphs = [R.regular_graph(1000, 7, 31), weighted(R.regular_graph(300, 7, 32), "real", 1), nx.complete_graph(3),
              loop_graph(120, 5, 33), hub_graph(500, 7, 34)]
    hs, batch = batch_of(pkg, graphs)
    P = np.concatenate([probabilities(h.n, 3, 50 + i) for i, h in enumerate(hs)])
    keys = SR.keys(11, range(batch.B))
    for keep in (True, False):
        want, got = run_seeded(pkg, batch, P, keys, 33, keep), run_ksample(pkg, batch, P, keys, 33, keep)
        assert sorted(want) == sorted(got)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), k
    A = np.random.RandomState(3).randint(0, 3, (33, batch.R)).astype(np.int8)
    A[1, 7], A[2, 1100] = 3, -1
    inv_t = AR.schedule(30, scale=float(batch.host.vals.mean()))
    want, got = run_anneal(pkg, batch, A, inv_t, 5, 100), run_kanneal(pkg, batch, 3, A, inv_t, 5, 100)
    for k in want:
        assert got[k].tobytes() == want[k].tobytes(), k
    for max_sweeps in (100, 1, 0):
        want, got = run_refine(pkg, batch, A, max_sweeps), run_kanneal(pkg, batch, 3, A, [], 5, max_sweeps)
        for k in want:
            assert got[k].tobytes() == want[k].tobytes(), (k, max_sweeps)
        assert (got["snap"] == 0).all()


@pytest.mark.parametrize("K,fits,make", [(4, 1, lambda: [weighted(R.regular_graph(300, 7, 21), "real", 7),
                                                         weighted(loop_graph(120, 5, 22), "real", 8)]),
                                         (8, 0, lambda: [weighted(R.regular_graph(1000, 7, 23), "real", 9)])])
def test_real_weights_keep_the_invariants(pkg, K, fits, make):
    """The snapshot choice rests on block_cut's summation order there, so no byte-for-byte claim."""
    hs, batch = batch_of(pkg, make())
    assert staged(pkg, batch) == fits
    A = np.random.RandomState(4).randint(0, K, (33, batch.R)).astype(np.int8)
    inv_t = AR.schedule(50, scale=float(batch.host.vals.mean()))
    scored = run_kanneal(pkg, batch, K, A, [], 11, 0)                   # no sweep at all: block_cut of the input
    assert (scored["assign"] == A).all()
    got = run_kanneal(pkg, batch, K, A, inv_t, 11, 100)
    again = run_kanneal(pkg, batch, K, A, inv_t, 11, 100)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k
    assert (got["cut_all"] >= scored["cut_all"]).all()                  # the same fp32 count: no tolerance
    assert (got["cut_all"] > scored["cut_all"]).any()
    for g, (h, (lo, hi)) in enumerate(zip(hs, spans(batch))):
        out = got["assign"][:, lo:hi]
        assert (out[:, :K] == A[:, lo:lo + K]).all()
        assert ((out >= 0) & (out < K)).all()
        for i in range(A.shape[0]):
            after = RR.cut(h.rowptr, h.col, h.weight, out[i])
            # fp32 recount: at most deg + 8 roundings of 2^-24 each on sums of positive terms
            assert abs(got["cut_all"][g, i] - after) <= 1e-5 * after
            assert 0 <= got["snap"][g, i] <= 50 and 1 <= got["sweeps"][g, i] <= 100


def test_seed_and_batch_position(pkg):
    K = 5
    g = R.regular_graph(300, 7, 51)
    _h1, alone = batch_of(pkg, [g])
    _h3, third = batch_of(pkg, [R.regular_graph(100, 12, 52), nx.complete_graph(K), g, R.regular_graph(50, 3, 53)])
    A = np.random.RandomState(1).randint(0, K, (7, third.R)).astype(np.int8)
    lo, hi = spans(third)[2]
    inv_t = AR.schedule(30)
    a = run_kanneal(pkg, alone, K, A[:, lo:hi], inv_t, 3, 100)
    b = run_kanneal(pkg, third, K, A, inv_t, 3, 100)
    assert (a["assign"] == b["assign"][:, lo:hi]).all()
    assert (a["cut_all"][0] == b["cut_all"][2]).all() and (a["snap"][0] == b["snap"][2]).all()
    assert (a["sweeps"][0] == b["sweeps"][2]).all() and a["best_idx"][0] == b["best_idx"][2]
    c = run_kanneal(pkg, third, K, A, inv_t, 4, 100)
    assert (b["assign"] != c["assign"]).any(axis=1).any()
    high = run_kanneal(pkg, third, K, A, inv_t, 3 + (1 << 63), 100)      # the whole 64-bit seed reaches the hash
    assert (b["assign"] != high["assign"]).any()


def test_a_converged_descent_leaves_no_improving_move(pkg):
    K = 4
    hs, batch = batch_of(pkg, [R.regular_graph(300, 7, 61), weighted(R.regular_graph(200, 6, 62), "int", 1)])
    A = np.random.RandomState(2).randint(0, K, (5, batch.R)).astype(np.int8)
    got = run_kanneal(pkg, batch, K, A, AR.schedule(40, scale=float(batch.host.vals.mean())), 8, 100)
    assert (got["sweeps"] < 100).all()
    for h, (lo, hi) in zip(hs, spans(batch)):
        for a in got["assign"][:, lo:hi]:
            assert KS.best_single_move_gain(h.n, h.rowptr, h.col, h.weight, a.tolist(), K) == 0


def test_probe_shows_one_tag_per_call(pkg):
    hs, batch = batch_of(pkg, [R.regular_graph(100, 5, 71)])
    A = np.random.RandomState(3).randint(0, 4, (4, batch.R)).astype(np.int8)
    P = probabilities(100, 4, 1)
    with pkg.hip.Probe(8) as pr:
        run_kanneal(pkg, batch, 4, A, AR.schedule(5), 0, 10)
        run_ksample(pkg, batch, P, SR.keys(0, [0]), 3)
        run_kanneal(pkg, batch, 4, A, [], 0, 10)
        run_ksample(pkg, batch, P, SR.keys(0, [0]), 3, keep=False)
    assert [t for t, _ms in pr.records] == ["anneal", "sample", "anneal", "sample"]


# ---- the Python API ---------------------------------------------------------------------------------------------------
SEARCH_KEYS = {'nodes', 'simple_cut', 'simple_assignment', 'expected_cut', 'rounded_cut', 'rounded_assignment',
               'post_cut', 'post_assignment', 'searched_cut', 'searched_assignment', 'searched_from'}


@pytest.mark.parametrize("K", (2, 4))
def test_search_dataset(pkg, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = small_model(pkg, K, [(60, 5, 61), (48, 6, 62), (100, 7, 63)], 128, 16, seed=K)
    results = TN.search_dataset(net, ds, samples=20, sample_seed=5, anneal_sweeps=20, anneal_seed=2)
    rounded = TN.round_dataset(net, ds, 0)
    local = TN.search_dataset(net, ds, samples=20, sample_seed=5, anneal_sweeps=0, candidates=2)
    none = TN.search_dataset(net, ds, samples=0, anneal_sweeps=0)
    assert len(results) == len(ds) == len(local) == len(none)
    for i, (res, rnd, loc, non, (handle, a_pad, nx_g, _t)) in enumerate(zip(results, rounded, local, none, ds.values())):
        assert set(res) == SEARCH_KEYS == set(loc) and set(non) == SEARCH_KEYS - {'post_cut', 'post_assignment'}
        assert res["nodes"] == handle.n
        for what in ("simple", "rounded", "post", "searched"):
            a = res[what + "_assignment"]
            assert res[what + "_cut"] == TN.calculate_cut_value(a, nx_g), what
            assert a[:K] == list(range(K)) and 0 <= min(a) and max(a) < K and len(a) == handle.n
        assert res["searched_cut"] >= max(res["simple_cut"], res["rounded_cut"], res["post_cut"])
        assert 0 <= res["searched_from"] < 22
        for k in ("simple_cut", "simple_assignment", "expected_cut", "rounded_cut", "rounded_assignment"):
            assert res[k] == rnd[k] == loc[k] == non[k], k
        with torch.no_grad():
            P = net(handle, a_pad)
        one, one_cut = TN.sampling_optimization(P, nx_g, 20, seed=5, graph_index=i)
        assert one == res["post_assignment"] == loc["post_assignment"] and one_cut == res["post_cut"]
        h = handles_of([nx_g])[0]
        ref = KS.sample(h, P.cpu().numpy(), SR.keys(5, [i])[0], 20)
        assert ref["best_assign"].tolist() == one and float(ref["best_cut"]) == one_cut
        assert TN.assign_partitions_seeded_kway(P.cpu().numpy(), 5, i, int(ref["best_iter"])) == one
        # the local search alone over the argmax and the rounded candidates: the better of the two descents
        simple = res["simple_assignment"]
        descents = [TN.kway_local_search(a, nx_g, K) for a in (simple, res["rounded_assignment"])]
        best = 0 if descents[0][1] >= descents[1][1] else 1
        assert (loc["searched_assignment"], loc["searched_cut"], loc["searched_from"]) == (*descents[best], best)
        assert non["searched_cut"] == loc["searched_cut"] and non["searched_assignment"] == loc["searched_assignment"]
        # the single-graph functions against the restatement
        start = np.asarray([simple], np.int8)
        got, cut = TN.kway_annealing(simple, nx_g, K, sweeps=20, seed=3)
        ref, _snap, sweeps = KS.anneal(h.n, h.rowptr, h.col, h.weight, start, K, AR.schedule(20), AR.levels(), 3, 100)
        assert got == ref[0].tolist() and int(sweeps[0]) < 100
        assert cut == TN.calculate_cut_value(got, nx_g) >= res["simple_cut"]
        ref, _sw = KS.refine(h.n, h.rowptr, h.col, h.weight, start, K, 100)
        assert descents[0][0] == ref[0].tolist()
        assert TN.kway_annealing(simple, nx_g, K, sweeps=0) == descents[0]
        kept, cut0 = TN.kway_local_search(simple, nx_g, K, max_sweeps=0)
        assert kept == simple and cut0 == res["simple_cut"]
    with pytest.raises(ValueError):
        TN.search_dataset(net, ds, samples=20, candidates=23)


def test_three_class_results_are_unchanged_by_a_k_class_call(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net3, ds3 = small_model(pkg, 3, [(60, 5, 71), (48, 6, 72)], 128, 16, seed=5)
    net4, ds4 = small_model(pkg, 4, [(60, 5, 73)], 128, 16, seed=6, epochs=1)
    before = TN.decode_dataset(net3, ds3, 20, anneal_sweeps=10, sample_seed=4)
    TN.search_dataset(net4, ds4, samples=10, anneal_sweeps=10)
    assert TN.decode_dataset(net3, ds3, 20, anneal_sweeps=10, sample_seed=4) == before
    three = TN.search_dataset(net3, ds3, samples=20, sample_seed=4, anneal_sweeps=0)
    for b, t in zip(before, three):                                     # at K = 3 the seeded samples are the 3-class ones
        assert (b["post_cut"], b["post_assignment"]) == (t["post_cut"], t["post_assignment"])
