"""GPU tests of the sampler and the annealing for graphs beyond 4096 nodes (gmc_large_sample_seeded_f32,
gmc_large_anneal_f32 and their Python API): byte for byte against the one-workgroup kernels
(gmc_kway_decode_sample_seeded_f32, gmc_kway_refine_anneal_f32) on every shape both run with unit, integer and dyadic
weights (every fp32 cut is then exact in any summation order); byte for byte against the restatement of
tests/large_search_ref.py beyond 4096 nodes, where the counter of the move test has its 20-bit fields; with no
annealing sweeps against gmc_large_local_search_f32 and gmc_large_round_conditional_f32 for any weights; and for real
and signed weights the properties the header states.  Outputs are pre-filled with garbage and the workspace with 0xA5.

Bars.  cut_all: exact where the weights are unit, integer or dyadic; 1e-5 relative to the float64 recount for real
weights (the bar of tests/test_gpu_large_rounding.py for cut: a row adds at most deg terms, a tile 8 more levels, a
graph its tiles, each rounding 2^-24 of a partial).  A converged descent leaves no improving move beyond that module's
GAIN_EPS."""
import functools

import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import large_ref as LR
from tests import large_round_ref as LRR
from tests import large_search_ref as LS
from tests import rounding_ref as CR
from tests import seeded_ref as SR
from tests.test_gpu_anneal import weighted
from tests.test_gpu_kway_search import run_kanneal, run_ksample
from tests.test_gpu_large_rounding import LargeBatch, gain_eps, run_large_round, run_large_search, shapes
from tests.test_gpu_rounding import small_model
from tests.test_refine_host import handles_of
from tests.test_rounding_host import SLACK

pytestmark = pytest.mark.gpu

GARBAGE = -5
KS_ = (2, 3, 4, 8)
COMBOS = [(1, 30), (7, 30), (33, 10), (65, 5), (130, 3)]               # (candidates, annealing sweeps): every cp boundary


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def workspace(pkg, batch, K, cands):
    need = pkg.hip.load().gmc_large_search_workspace_bytes(batch.ref(), K, cands)
    assert need > 0
    return torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")   # garbage: the calls write what they read


def run_large_sample(pkg, batch, P, keys, iters, keep=True):
    """gmc_large_sample_seeded_f32 with every output pre-filled with garbage; keep=False: assign_all = NULL."""
    hip = pkg.hip
    K = P.shape[1]
    Pt = torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda()
    gkey = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()
    ws = workspace(pkg, batch, K, iters)
    assign_all = torch.full((iters, batch.R), GARBAGE, dtype=torch.int8, device="cuda") if keep else None
    cut_all = torch.full((batch.B, iters), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_iter = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_large_sample_seeded_f32(batch.ref(), p(Pt), K, p(gkey), iters, p(assign_all), p(ws), ws.numel(),
                                                p(cut_all), p(best_assign), p(best_cut), p(best_iter), hip.stream())
    hip.check(rc, "gmc_large_sample_seeded_f32")
    torch.cuda.synchronize()
    out = dict(cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_iter=best_iter)
    if keep:
        out["assign_all"] = assign_all
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_large_anneal(pkg, batch, K, A, inv_temp, seed, max_descent, want_extra=True, order=None):
    """gmc_large_anneal_f32 on A [cands, R] int8 with every output pre-filled with garbage."""
    hip = pkg.hip
    cands = A.shape[0]
    order, cgoff, cptr, most = batch.large_order(K) if order is None else order
    assign = torch.from_numpy(np.array(A, np.int8)).cuda()
    inv_t = torch.from_numpy(np.asarray(inv_temp, np.float32)).cuda() if len(inv_temp) else None
    lv = torch.from_numpy(AR.levels()).cuda() if len(inv_temp) else None
    ws = workspace(pkg, batch, K, cands)
    cut_all = torch.full((batch.B, cands), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_idx = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    snap = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    sweeps = torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_large_anneal_f32(batch.ref(), K, p(order), p(cgoff), p(cptr), most, cands, p(assign), p(inv_t),
                                         len(inv_temp), p(lv), seed, max_descent, p(ws), ws.numel(), p(cut_all),
                                         p(best_assign), p(best_cut), p(best_idx), p(snap) if want_extra else None,
                                         p(sweeps) if want_extra else None, hip.stream())
    hip.check(rc, "gmc_large_anneal_f32")
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in dict(assign=assign, cut_all=cut_all, best_assign=best_assign,
                                                    best_cut=best_cut, best_idx=best_idx, snap=snap,
                                                    sweeps=sweeps).items()}


def spans(batch):
    return [(int(batch.goff_host[g]), int(batch.goff_host[g + 1])) for g in range(batch.B)]


def start(batch, K, cands, seed):
    """[cands, R] int8: random classes; bytes of no class on movable nodes of the last graph in the first and the last
    candidate."""
    A = np.random.RandomState(seed).randint(0, K, (cands, batch.R)).astype(np.int8)
    lo, hi = spans(batch)[-1]
    if hi - lo > K:
        A[0, hi - 1] = K
        A[-1, hi - 1] = -1
    if hi - lo > K + 2:
        A[0, lo + K + 1] = -1
    return A


def same(new, want, keys=("assign", "cut_all", "best_assign", "best_cut", "best_idx", "snap", "sweeps")):
    for k in keys:
        assert new[k].tobytes() == want[k].tobytes(), (k, int((new[k] != want[k]).sum()))


# ---- against the one-workgroup kernels ----------------------------------------------------------------------------------
SHAPES = [(K, name) for K in KS_ for name in sorted(shapes(2))] + [(3, "n4096"), (8, "n4096")]


@functools.lru_cache(maxsize=None)
def small_handles(K, name, kind):
    graphs = [R.regular_graph(4096, 3, 4096)] if name == "n4096" else shapes(K)[name]
    if kind != "unit":
        graphs = [weighted(g, kind, 7 * i + K) for i, g in enumerate(graphs)]
    return handles_of(graphs)


@pytest.mark.parametrize("kind", ("unit", "dyadic"))
@pytest.mark.parametrize("K,name", SHAPES)
def test_annealing_is_the_one_workgroup_kernels(pkg, K, name, kind):
    batch = LargeBatch(pkg, small_handles(K, name, kind))
    scale = 1.0 if batch.vals_host is None else float(batch.vals_host.mean())
    for cands, sweeps in COMBOS:
        A = start(batch, K, cands, 13 * K + len(name) + cands)
        inv_t = AR.schedule(sweeps, scale=scale)
        want = run_kanneal(pkg, batch, K, A, inv_t, LS.SEED, 100)
        new = run_large_anneal(pkg, batch, K, A, inv_t, LS.SEED, 100)
        same(new, want)


@pytest.mark.parametrize("cands,sweeps", COMBOS)
@pytest.mark.parametrize("K", KS_)
def test_every_candidate_count_on_a_batch(pkg, K, cands, sweeps):
    batch = LargeBatch(pkg, small_handles(K, "batch_5_700_257", "dyadic" if K in (3, 8) else "unit"))
    scale = 1.0 if batch.vals_host is None else float(batch.vals_host.mean())
    A = start(batch, K, cands, K + cands)
    for n_sweeps, descent in ((sweeps, 100), (sweeps, 0), (0, 2)):
        inv_t = AR.schedule(n_sweeps, scale=scale)
        same(run_large_anneal(pkg, batch, K, A, inv_t, 5, descent), run_kanneal(pkg, batch, K, A, inv_t, 5, descent))


@pytest.mark.parametrize("K", (2, 4))
def test_snapshots_kept_and_taken(pkg, K):
    """The case whose candidates the CPU check (test_large_search_host.py) shows to keep their start and to take later
    snapshots: against the one-workgroup kernel and the restatement."""
    h, A, inv_t = LS.condition_case(K)
    A = A.copy()                                                       # (the shared case is read-only)
    batch = LargeBatch(pkg, [h])
    new = run_large_anneal(pkg, batch, K, A, inv_t, LS.SEED, 100)
    same(new, run_kanneal(pkg, batch, K, A, inv_t, LS.SEED, 100))
    ref = LS.search(h.n, h.rowptr, h.col, h.weight, A, K, inv_t, AR.levels(), LS.SEED, 100)
    assert (new["snap"][0] == 0).any() and (new["snap"][0] > 0).any()
    assert new["assign"].tobytes() == ref["assign"].tobytes() and (new["snap"][0] == ref["snap"]).all()
    plain = run_large_anneal(pkg, batch, K, A, [], LS.SEED, 100)
    assert (plain["assign"] != new["assign"]).any()


def sampler_graphs(K):
    s = shapes(K)
    return [s[name][0] for name in ("n_K", "n_K1", "n255", "n256", "n257", "path1030", "hub40", "self_loops")] + \
        s["batch_5_700_257"]


@pytest.mark.parametrize("kind", ("unit", "dyadic"))
@pytest.mark.parametrize("iters", (1, 7, 33))
@pytest.mark.parametrize("K", KS_)
def test_sampler_is_the_one_workgroup_kernels(pkg, K, iters, kind):
    graphs = sampler_graphs(K)
    if kind != "unit":
        graphs = [weighted(g, kind, 3 * i + K) for i, g in enumerate(graphs)]
    batch = LargeBatch(pkg, handles_of(graphs))
    P = CR.softmax_rows(batch.R, K, 5 * K + iters, scale=1.5)
    for lo, _hi in spans(batch):
        P[lo:lo + K] = np.nan                                          # the terminals' rows are never read
    lo = spans(batch)[5][0]
    P[lo + K:lo + 2 * K] = np.eye(K, dtype=np.float32)                 # one-hot rows, an all-zero row, a NaN row
    P[lo + 2 * K], P[lo + 2 * K + 1] = 0.0, np.nan
    keys = SR.keys(3 + iters, range(2, 2 + batch.B))
    want = run_ksample(pkg, batch, P, keys, iters)
    new = run_large_sample(pkg, batch, P, keys, iters)
    for k in want:
        assert new[k].tobytes() == want[k].tobytes(), k
    bare = run_large_sample(pkg, batch, P, keys, iters, keep=False)
    for k in bare:
        assert bare[k].tobytes() == want[k].tobytes(), k


# ---- beyond 4096 nodes: against the restatement -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(LS.BIG_CASES))
def test_beyond_4096_nodes_against_the_restatement(pkg, name):
    from gcn_max_cut_amd.graph import GraphHandle
    K, n, rowptr, col, w, A, inv_t, max_descent, _groups = LS.big_case(name)
    ref = LS.big_reference(name)
    batch = LargeBatch(pkg, [GraphHandle(n, rowptr, col, w)])
    new = run_large_anneal(pkg, batch, K, A, inv_t, LS.SEED, max_descent)
    assert new["assign"].tobytes() == ref["assign"].tobytes(), int((new["assign"] != ref["assign"]).sum())
    assert new["cut_all"][0].tobytes() == ref["cut_all"].tobytes()
    assert (new["snap"][0] == ref["snap"]).all() and (new["sweeps"][0] == ref["sweeps"]).all()
    assert new["best_assign"].tobytes() == ref["best_assign"].tobytes()
    assert new["best_cut"][0] == ref["best_cut"] and new["best_idx"][0] == ref["best_idx"]
    iters = 2 if n > 100000 else 5
    P = LRR.softmax_rows(n, K, len(name) + K)
    P[:K] = np.nan
    key = SR.keys(7, [3])
    want = LS.sample(n, rowptr, col, w, P, key[0], iters)
    got = run_large_sample(pkg, batch, P, key, iters)
    for k in ("assign_all", "best_assign"):
        assert got[k].tobytes() == want[k].tobytes(), k
    assert got["cut_all"][0].tobytes() == want["cut_all"].tobytes()
    assert got["best_cut"][0] == want["best_cut"] and got["best_iter"][0] == want["best_iter"]
    bare = run_large_sample(pkg, batch, P, key, iters, keep=False)
    assert bare["best_assign"].tobytes() == want["best_assign"].tobytes()
    assert bare["cut_all"].tobytes() == got["cut_all"].tobytes()


def test_one_batch_with_both_counter_layouts(pkg):
    from gcn_max_cut_amd.graph import GraphHandle
    K, cands = 4, 5
    specs = LS.mixed_batch()
    hs = [GraphHandle(n, rp, col, LS.integer_edge_weights(n, rp, col, i) if i != 1 else None)
          for i, (n, rp, col) in enumerate(specs)]
    batch = LargeBatch(pkg, hs)
    assert [LS.wide(h.n) for h in hs] == [False, True, True]
    A = start(batch, K, cands, 21)
    inv_t = LS.schedule(5)
    new = run_large_anneal(pkg, batch, K, A, inv_t, LS.SEED, 20)
    for g, (h, (lo, hi)) in enumerate(zip(hs, spans(batch))):
        ref = LS.search(h.n, h.rowptr, h.col, h.weight, A[:, lo:hi], K, inv_t, AR.levels(), LS.SEED, 20)
        assert new["assign"][:, lo:hi].tobytes() == ref["assign"].tobytes(), g
        assert new["cut_all"][g].tobytes() == ref["cut_all"].tobytes()
        assert (new["snap"][g] == ref["snap"]).all() and (new["sweeps"][g] == ref["sweeps"]).all()
        assert new["best_assign"][lo:hi].tobytes() == ref["best_assign"].tobytes() and new["best_idx"][g] == ref["best_idx"]
    small = LargeBatch(pkg, hs[:1])                                    # the 300-node graph: the one-workgroup kernel's bytes
    lo, hi = spans(batch)[0]
    want = run_kanneal(pkg, small, K, A[:, lo:hi], inv_t, LS.SEED, 20)
    assert new["assign"][:, lo:hi].tobytes() == want["assign"].tobytes()


# ---- no annealing sweeps: the large local search ------------------------------------------------------------------------
@pytest.mark.parametrize("K,kind", [(2, "real"), (3, "unit"), (8, "real")])
def test_no_annealing_sweeps_is_the_large_local_search(pkg, K, kind):
    from gcn_max_cut_amd.graph import GraphHandle
    n, rp, col = LR.circulant(4300, 7, 5)
    graphs = [CR.connected_gnp(257, 0.03, 260 + K), R.regular_graph(700, 7, 700 + K)]
    if kind == "real":
        graphs = [CR.signed_weights(g, 5 * i + K) for i, g in enumerate(graphs)]
    hs = handles_of(graphs) + [GraphHandle(n, rp, col, LRR.signed_edge_weights(n, rp, col, K) if kind == "real" else None)]
    batch = LargeBatch(pkg, hs)
    P = np.concatenate([CR.softmax_rows(h.n, K, 30 + i, scale=2.0) for i, h in enumerate(hs)])
    rounded = run_large_round(pkg, batch, P, K, 0)["assign"]
    A = start(batch, K, 4, 3 * K)
    A[1] = rounded
    for descent in (100, 1, 0):
        new = run_large_anneal(pkg, batch, K, A, [], LS.SEED, descent)
        assert (new["snap"] == 0).all()
        for i in range(A.shape[0]):
            want = run_large_search(pkg, batch, A[i], K, descent)
            assert new["assign"][i].tobytes() == want["assign"].tobytes(), (descent, i)
            assert new["sweeps"][:, i].tobytes() == want["sweeps"].tobytes(), (descent, i)
            assert new["cut_all"][:, i].tobytes() == want["cut"].tobytes()   # the same summation order
        want = run_large_round(pkg, batch, P, K, descent)
        assert new["assign"][1].tobytes() == want["assign"].tobytes() and (new["sweeps"][:, 1] == want["sweeps"]).all()


# ---- real-valued and signed weights: by properties ----------------------------------------------------------------------
def by_hand_order(batch, graphs, K):
    """The order arrays of a batch with a graph of fewer than K nodes (the host routine refuses it): the restatement's."""
    order, cgoff, cptr, most = LRR.order_arrays(graphs, K)
    cptr = np.concatenate([cptr, np.zeros(batch.R + batch.B - cptr.size, np.int32)])
    order = np.concatenate([order, np.zeros(batch.R - order.size, np.int32)])
    return tuple(torch.from_numpy(a).cuda() for a in (order, cgoff, cptr)) + (most,)


def test_real_and_signed_weights_keep_the_properties(pkg):
    from gcn_max_cut_amd.graph import GraphHandle
    K, cands, sweeps = 4, 9, 12
    specs = [LR.circulant(3, 2, None), LR.circulant(300, 6, 4), LR.circulant(4500, 7, 8)]
    hs = [GraphHandle(n, rp, col, LRR.signed_edge_weights(n, rp, col, i)) for i, (n, rp, col) in enumerate(specs)]
    batch = LargeBatch(pkg, hs)
    order = by_hand_order(batch, specs, K)
    A = start(batch, K, cands, 17)
    A[:, 3:3 + K], A[:, 303:303 + K] = np.arange(K), np.arange(K)      # the terminals hold their classes
    valid = ((A >= 0) & (A < K))
    inv_t = AR.schedule(sweeps, scale=float(np.abs(batch.vals_host).mean()))
    got = run_large_anneal(pkg, batch, K, A, inv_t, LS.SEED, 100, order=order)
    again = run_large_anneal(pkg, batch, K, A, inv_t, LS.SEED, 100, order=order)
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k               # two runs are byte-equal
    bare = run_large_anneal(pkg, batch, K, A, inv_t, LS.SEED, 100, want_extra=False, order=order)
    same(bare, got, ("assign", "cut_all", "best_assign", "best_cut", "best_idx"))
    assert (bare["snap"] == GARBAGE).all() and (bare["sweeps"] == GARBAGE).all()
    # the graph with fewer than K nodes is left unwritten
    assert (got["assign"][:, :3] == A[:, :3]).all() and (got["best_assign"][:3] == GARBAGE).all()
    assert np.isnan(got["cut_all"][0]).all() and np.isnan(got["best_cut"][0]) and got["best_idx"][0] == GARBAGE
    assert (got["snap"][0] == GARBAGE).all() and (got["sweeps"][0] == GARBAGE).all()
    scored = run_large_anneal(pkg, batch, K, A, [], LS.SEED, 0, order=order)   # no sweep at all: the score of the input
    assert (scored["assign"] == A).all()
    for g, (h, (lo, hi)) in enumerate(zip(hs, spans(batch))):
        if g == 0:
            continue
        out = got["assign"][:, lo:hi]
        assert (out[:, :K] == np.arange(K)).all() and ((out >= 0) & (out < K)).all()
        best = int(got["best_idx"][g])
        assert best == int(np.argmax(got["cut_all"][g])) and got["best_cut"][g] == got["cut_all"][g, best]
        assert (got["best_assign"][lo:hi] == out[best]).all()
        for i in range(cands):
            after = CR.cut(h.rowptr, h.col, h.weight, out[i])
            bound = 1e-5 * abs(after)
            print(f"graph {g} candidate {i}: cut {got['cut_all'][g, i]} (float64 recount {after}), input "
                  f"{scored['cut_all'][g, i]}, snap {got['snap'][g, i]}, sweeps {got['sweeps'][g, i]}")
            assert abs(float(got["cut_all"][g, i]) - after) <= bound
            if valid[i, lo:hi].all():
                before = CR.cut(h.rowptr, h.col, h.weight, A[i, lo:hi])
                assert abs(float(scored["cut_all"][g, i]) - before) <= 1e-5 * abs(before)
                assert after >= before - bound
            assert 0 <= got["snap"][g, i] <= sweeps and 1 <= got["sweeps"][g, i] <= 100
            if got["sweeps"][g, i] < 100:                              # converged: a local optimum
                gain = LRR.best_single_move_gain(h.n, h.rowptr, h.col, h.weight, out[i], K)
                assert gain <= gain_eps(h), gain
        # the graph alone gives what it gives third in the batch
        alone = run_large_anneal(pkg, LargeBatch(pkg, [h]), K, A[:, lo:hi], inv_t, LS.SEED, 100)
        assert alone["assign"].tobytes() == out.tobytes()
        for k in ("cut_all", "snap", "sweeps", "best_cut", "best_idx"):
            assert alone[k][0].tobytes() == got[k][g].tobytes(), (k, g)
    # the sampler: alone and in the batch, the skipped graph unwritten
    P = np.concatenate([LRR.softmax_rows(h.n, K, 40 + i) for i, h in enumerate(hs)])
    keys = SR.keys(9, range(3))
    s = run_large_sample(pkg, batch, P, keys, 7)
    assert (s["assign_all"][:, :3] == GARBAGE).all() and np.isnan(s["cut_all"][0]).all() and s["best_iter"][0] == GARBAGE
    lo, hi = spans(batch)[2]
    alone = run_large_sample(pkg, LargeBatch(pkg, hs[2:]), P[lo:hi], keys[2:], 7)
    assert alone["assign_all"].tobytes() == s["assign_all"][:, lo:hi].tobytes()
    assert alone["cut_all"][0].tobytes() == s["cut_all"][2].tobytes() and alone["best_iter"][0] == s["best_iter"][2]
    for i in range(7):
        c64 = CR.cut(hs[2].rowptr, hs[2].col, hs[2].weight, s["assign_all"][i, lo:hi])
        assert abs(float(s["cut_all"][2, i]) - c64) <= 1e-5 * abs(c64)


def test_probe_shows_one_record_per_call(pkg):
    K = 4
    batch = LargeBatch(pkg, handles_of([R.regular_graph(100, 5, 71)]))
    A = start(batch, K, 4, 3)
    P = CR.softmax_rows(100, K, 1)
    with pkg.hip.Probe(8) as pr:
        run_large_anneal(pkg, batch, K, A, AR.schedule(5), 0, 10)
        run_large_sample(pkg, batch, P, SR.keys(0, [0]), 3)
        run_large_anneal(pkg, batch, K, A, [], 0, 10)
        run_large_sample(pkg, batch, P, SR.keys(0, [0]), 3, keep=False)
    assert [t for t, _ms in pr.records] == ["refine", "sample", "refine", "sample"]


# ---- the Python API -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 4))
def test_search_large_dataset_equals_search_dataset_on_small_graphs(pkg, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net, ds = small_model(pkg, K, [(60, 5, 61), (48, 6, 62), (100, 7, 63)], 128, 16, seed=K)
    for kw in (dict(samples=20, sample_seed=5, anneal_sweeps=20, anneal_seed=2), dict(samples=70, anneal_sweeps=4),
               dict(samples=20, sample_seed=5, anneal_sweeps=0, candidates=2), dict(samples=0, anneal_sweeps=0),
               dict(samples=9, anneal_sweeps=3, candidates=1)):
        want = TN.search_dataset(net, ds, **kw)
        got = TN.search_large_dataset(net, ds, **kw)
        assert len(got) == len(want) == len(ds)
        for a, b, (_handle, _a_pad, nx_g, _t) in zip(got, want, ds.values()):
            assert set(a) == set(b)
            for key in set(b) - {"expected_cut"}:
                assert a[key] == b[key], (key, kw)
            assert abs(a["expected_cut"] - b["expected_cut"]) <= SLACK * nx_g.number_of_edges()   # (another summation order)
            assert kw.get("candidates") == 1 or a["searched_cut"] >= a["rounded_cut"]
    with pytest.raises(ValueError):
        TN.search_large_dataset(net, ds, samples=20, candidates=23)
    handle, a_pad, nx_g, _t = next(iter(ds.values()))
    with torch.no_grad():
        P = net(handle, a_pad)
    assert TN.large_sampling_optimization(P, nx_g, 20, seed=5) == TN.sampling_optimization(P, nx_g, 20, seed=5)
    assert TN.large_sampling_optimization(P.cpu().numpy(), handle, 20, seed=5, graph_index=2) == \
        TN.sampling_optimization(P, nx_g, 20, seed=5, graph_index=2)
    assert TN.large_sampling_optimization(P, nx_g, 0) == (None, -float("inf"))
    simple = TN.simple_partition_assignment(P)
    assert TN.large_annealing(simple, nx_g, K, sweeps=20, seed=3) == TN.kway_annealing(simple, nx_g, K, sweeps=20, seed=3)
    assert TN.large_annealing(simple, handle, K, sweeps=0) == TN.kway_local_search(simple, nx_g, K)
    assert TN.large_annealing(simple, nx_g, K, sweeps=0, max_descent_sweeps=0)[0] == simple


@pytest.mark.parametrize("K", (2, 4))
def test_search_large_dataset_on_a_dataset_without_the_dense_adjacency(pkg, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    from tests.test_gpu_large_graphs import dataset_of
    N = 4100
    ds = dataset_of(pkg, [4097, 300], K, N, seed=70 + K)
    assert all(it[1] is None for it in ds.values())
    torch.manual_seed(K)
    net, _embed, _opt = T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=N, hidden_dim=8, number_classes=K))
    with pytest.raises(ValueError, match="4096 nodes.*argmax partition.*search_large_dataset"):
        TN.search_dataset(net, ds)                                     # the one-workgroup decoders still refuse
    results = TN.search_large_dataset(net, ds, samples=6, sample_seed=1, anneal_sweeps=8, anneal_seed=4,
                                      max_descent_sweeps=20)
    rounded = TN.round_large_dataset(net, ds, 0)
    for i, (res, rnd, (handle, _none, nx_g, _t)) in enumerate(zip(results, rounded, ds.values())):
        assert res["nodes"] == handle.n
        for what in ("simple", "rounded", "post", "searched"):
            a = res[what + "_assignment"]
            assert res[what + "_cut"] == TN.calculate_cut_value(a, nx_g), what
            assert a[:K] == list(range(K)) and 0 <= min(a) and max(a) < K and len(a) == handle.n
        assert res["searched_cut"] >= max(res["simple_cut"], res["rounded_cut"], res["post_cut"])
        assert 0 <= res["searched_from"] < 8
        for k in ("simple_cut", "simple_assignment", "expected_cut", "rounded_cut", "rounded_assignment"):
            assert res[k] == rnd[k], k
    handle, _none, nx_g, _t = next(iter(ds.values()))
    part = results[0]["rounded_assignment"]
    with pytest.raises(ValueError, match="gmc_kway_refine_anneal_f32.*gmc error -6"):
        TN.kway_annealing(part, nx_g, K, sweeps=2)                     # the one-workgroup annealing keeps its limit
    got, cut = TN.large_annealing(part, handle, K, sweeps=4, seed=2, max_descent_sweeps=20)
    ref = LS.search(handle.n, handle.rowptr, handle.col, None, np.asarray([part], np.int8), K, AR.schedule(4),
                    AR.levels(), 2, 20)
    assert got == ref["assign"][0].tolist() and cut == TN.calculate_cut_value(got, nx_g) >= results[0]["rounded_cut"]


def test_three_class_results_are_unchanged_by_a_large_call(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    net3, ds3 = small_model(pkg, 3, [(60, 5, 71), (48, 6, 72)], 128, 16, seed=5)
    net4, ds4 = small_model(pkg, 4, [(60, 5, 73)], 128, 16, seed=6, epochs=1)
    before = TN.decode_dataset(net3, ds3, 20, anneal_sweeps=10, sample_seed=4)
    TN.search_large_dataset(net4, ds4, samples=10, anneal_sweeps=10)
    TN.search_large_dataset(net3, ds3, samples=10, anneal_sweeps=10)
    assert TN.decode_dataset(net3, ds3, 20, anneal_sweeps=10, sample_seed=4) == before
