"""GPU tests of the seeded post-processing sampler (gmc_decode_sample_seeded_f32 and its Python API) against the CPU
restatement in tests/seeded_ref.py: samples, cuts and the pick byte for byte (draws one float32 ulp either side of both
class boundaries included), the call without the [iters][R] array, independence of batch / iters / run, scores
against the numpy-stream sampler and the local search, and the Python entry points."""
import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import seeded_ref as SR
from tests import util
from tests.test_gpu_refine import run_refine, weighted
from tests.test_refine_host import handles_of

pytestmark = pytest.mark.gpu

GARBAGE = -5
ITERS = (1, 3, 64)


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def run_seeded(pkg, batch, P, keys, iters, keep=True):
    """gmc_decode_sample_seeded_f32 with every output pre-filled with garbage; keep=False: assign_all = NULL."""
    hip = pkg.hip
    Pt = torch.from_numpy(np.ascontiguousarray(P, np.float32)).cuda()
    gkey = torch.from_numpy(np.ascontiguousarray(keys, np.uint64).view(np.int64)).cuda()
    assign_all = torch.full((iters, batch.R), GARBAGE, dtype=torch.int8, device="cuda") if keep else None
    cut_all = torch.full((batch.B, iters), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_iter = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    rc = hip.load().gmc_decode_sample_seeded_f32(batch.ref(), p(Pt), p(gkey), iters, p(assign_all), p(cut_all),
                                                 p(best_assign), p(best_cut), p(best_iter), hip.stream())
    hip.check(rc, "gmc_decode_sample_seeded_f32")
    torch.cuda.synchronize()
    out = dict(cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_iter=best_iter)
    if keep:
        out["assign_all"] = assign_all
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bytes(got, want):
    assert sorted(got) == sorted(want)
    for k in got:
        a, b = np.asarray(got[k]), np.asarray(want[k])
        assert a.dtype == b.dtype and a.shape == b.shape, k
        assert a.tobytes() == b.tobytes(), k


def f32_at_or_below(u):
    f = np.float32(u)
    return f if float(f) <= u else np.nextafter(f, np.float32(-np.inf))


def f32_above(u):
    f = np.float32(u)
    return f if float(f) > u else np.nextafter(f, np.float32(np.inf))


# a row that needs the fallback to class 2 (for u >= 0.75), then saturated rows
FIXED_ROWS = ((0.25, 0.25, 0.25), (1, 0, 0), (0, 1, 0), (0, 0, 1))


def directed_probabilities(n, key, iters, seed):
    """[n, 3] float32: a softmax of random logits (n < 7: one skewed row); nodes 3..6 carry FIXED_ROWS (n >= 7); then
    (n >= 23), for four (iteration, node) pairs each, p[0] at the largest float32 <= u and at the smallest float32 > u
    of that draw (class 1 / class 0), and c1 = p[0] + p[1] at the same two places (class 2 / class 1).  Returns P and
    the expected class of every directed (iteration, node)."""
    rng = np.random.RandomState(seed)
    logits = rng.standard_normal((n, 3)) * 2.0
    e = np.exp(logits - logits.max(1, keepdims=True))
    P = (e / e.sum(1, keepdims=True)).astype(np.float32)
    expect = {}
    if n < 7:
        P[3:] = (0.9, 0.05, 0.05)     # mostly class 0: on K5 the best cut (nodes 3, 4 apart) is rare, and tied
    for node, row in zip(range(3, n if n >= 7 else 3), FIXED_ROWS):
        P[node] = row
        for it in range(iters if max(row) == 1 else 0):               # (the fallback row: class 2 also for u >= 0.75)
            expect[it, node] = int(np.argmax(row))
    if n >= 23:
        u = SR.uniforms(key, iters, n)
        its = [(0, 1, 31, 63)[j] % iters for j in range(4)]
        node = 7
        for it in its:
            x = float(u[it, node])
            P[node] = (f32_at_or_below(x), 0.125, 0.0)                 # u >= c0, u < c1
            expect[it, node] = 1
            x = float(u[it, node + 1])
            P[node + 1] = (f32_above(x), 0.125, 0.0)                   # u < c0
            expect[it, node + 1] = 0
            x = float(u[it, node + 2])
            p0 = 0.25 if x >= 0.5 else 0.0                             # c1 = p0 + p1 is exact in double
            P[node + 2] = (p0, f32_at_or_below(x - p0), 0.0)           # u >= c1
            expect[it, node + 2] = 2
            x = float(u[it, node + 3])
            p0 = 0.25 if x >= 0.5 else 0.0
            P[node + 3] = (p0, f32_above(x - p0), 0.0)                 # u >= c0, u < c1
            expect[it, node + 3] = 1
            node += 4
    return P, expect


def graphs_of(case):
    if case == "n3":
        return [nx.complete_graph(3)]                                  # no draw at all
    if case == "n4":
        return [nx.complete_graph(4)]
    if case == "n65_d3":
        return [util.near_regular(65, 3, 65)]
    if case == "n257_d7":
        return [util.near_regular(257, 7, 257)]
    if case == "n1030_d7":
        return [R.regular_graph(1030, 7, 1030)]
    if case == "batch":
        return [R.regular_graph(60, 7, 60), util.near_regular(97, 3, 97), nx.complete_graph(5)]
    if case == "int_weights":                                          # fp32 sums of small integers: exact in any order
        return [weighted(R.regular_graph(300, 7, 15), "int", 1), weighted(util.near_regular(65, 7, 16), "int", 2)]
    raise KeyError(case)


CASES = ("n3", "n4", "n65_d3", "n257_d7", "n1030_d7", "batch", "int_weights")
INDICES = (7, 0, 159)                                                  # dataset positions: distinct keys


_built_cases = {}


def case_of(case, iters, seed=12345):
    """(handles, P [R,3], keys [B], restatement per graph, directed expectations) - computed once per (case, iters)."""
    if (case, iters) not in _built_cases:
        hs = handles_of(graphs_of(case))
        keys = SR.keys(seed, INDICES[:len(hs)])
        rows, refs = [], []
        for g, (h, key) in enumerate(zip(hs, keys)):
            P, expect = directed_probabilities(h.n, key, iters, 100 * len(case) + g)
            ref = SR.sample(h, P, key, iters)
            for (it, node), cls in expect.items():                      # the directed rows do what they were made for
                assert ref["assign_all"][it, node] == cls, (case, g, it, node)
            rows.append(P)
            refs.append(ref)
        _built_cases[case, iters] = (hs, np.concatenate(rows), keys, refs)
    return _built_cases[case, iters]


def restated(batch, refs, iters, keep=True):
    """The restatement of the whole batch in the layout of the entry point's outputs."""
    out = dict(cut_all=np.stack([r["cut_all"] for r in refs]),
               best_assign=np.concatenate([r["best_assign"] for r in refs]),
               best_cut=np.array([r["best_cut"] for r in refs], np.float32),
               best_iter=np.array([r["best_iter"] for r in refs], np.int32))
    if keep:
        out["assign_all"] = np.concatenate([r["assign_all"] for r in refs], axis=1)
    return out


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("case", CASES)
def test_samples_cuts_and_pick_equal_the_restatement(pkg, case, iters):
    from gcn_max_cut_amd.graph import GraphBatch
    hs, P, keys, refs = case_of(case, iters)
    batch = GraphBatch(hs, None, torch.device("cuda"))
    assert (batch.vals is not None) == (case == "int_weights")
    got = run_seeded(pkg, batch, P, keys, iters)
    same_bytes(got, restated(batch, refs, iters))
    assert (got["assign_all"][:, batch.goff_host[:-1]] == 0).all()     # terminals
    if case == "n3":
        assert (got["cut_all"] == 3).all() and (got["best_iter"] == 0).all()


@pytest.mark.parametrize("iters", ITERS)
@pytest.mark.parametrize("case", ("n3", "n1030_d7", "batch", "int_weights"))
def test_without_the_sample_array_every_other_output_is_the_same(pkg, case, iters):
    from gcn_max_cut_amd.graph import GraphBatch
    hs, P, keys, refs = case_of(case, iters)
    batch = GraphBatch(hs, None, torch.device("cuda"))
    full = run_seeded(pkg, batch, P, keys, iters)
    lean = run_seeded(pkg, batch, P, keys, iters, keep=False)
    assert "assign_all" not in lean
    full.pop("assign_all")
    same_bytes(lean, full)
    same_bytes(lean, restated(batch, refs, iters, keep=False))
    if case == "batch" and iters == 64:
        # the 5-node graph has 9 possible samples: its best cut is tied between iterations, and the first one wins
        cuts = refs[2]["cut_all"]
        winners = np.flatnonzero(cuts == cuts.max())
        assert winners.size >= 2 and winners[0] > 0 and lean["best_iter"][2] == winners[0]
        lo = int(batch.goff_host[2])
        assert (lean["best_assign"][lo:] == refs[2]["assign_all"][winners[0]]).all()


def test_a_graphs_samples_depend_on_its_key_alone(pkg):
    from gcn_max_cut_amd.graph import GraphBatch
    hs, P, keys, refs = case_of("batch", 64)
    batch = GraphBatch(hs, None, torch.device("cuda"))
    lo, hi = int(batch.goff_host[1]), int(batch.goff_host[2])
    inside = run_seeded(pkg, batch, P, keys, 64)
    again = run_seeded(pkg, batch, P, keys, 64)
    same_bytes(again, inside)                                          # two runs
    alone_batch = GraphBatch([hs[1]], None, torch.device("cuda"))     # the 97-node graph alone, with its key
    alone = run_seeded(pkg, alone_batch, P[lo:hi], keys[1:2], 64)
    assert alone["assign_all"].tobytes() == np.ascontiguousarray(inside["assign_all"][:, lo:hi]).tobytes()
    assert alone["cut_all"].tobytes() == inside["cut_all"][1:2].tobytes()
    assert alone["best_assign"].tobytes() == inside["best_assign"][lo:hi].tobytes()
    assert alone["best_cut"].tobytes() == inside["best_cut"][1:2].tobytes()
    assert alone["best_iter"].tobytes() == inside["best_iter"][1:2].tobytes()
    moved = GraphBatch([hs[1], hs[0]], None, torch.device("cuda"))    # another position in another batch
    swapped = run_seeded(pkg, moved, np.concatenate([P[lo:hi], P[:lo]]), keys[[1, 0]], 64)
    assert swapped["assign_all"][:, :hi - lo].tobytes() == alone["assign_all"].tobytes()
    assert swapped["cut_all"][0].tobytes() == alone["cut_all"][0].tobytes()
    short = run_seeded(pkg, batch, P, keys, 3)                         # iteration i of any call is iteration i
    assert short["assign_all"].tobytes() == inside["assign_all"][:3].tobytes()
    assert short["cut_all"].tobytes() == np.ascontiguousarray(inside["cut_all"][:, :3]).tobytes()
    other = run_seeded(pkg, batch, P, SR.keys(12346, INDICES), 64)     # and another seed gives other samples
    assert (other["assign_all"] != inside["assign_all"]).any()


def test_scores_are_those_of_the_other_decoders(pkg):
    """Real-valued weights: the seeded samples score, bit for bit, what gmc_refine_local_f32(max_sweeps = 0) reports
    for them, and what gmc_decode_sample_f32 reports when it is fed the same uniforms."""
    from gcn_max_cut_amd.graph import GraphBatch
    hip = pkg.hip
    graphs = [weighted(R.regular_graph(200, 7, 21), "float", 5), R.regular_graph(100, 6, 22), nx.complete_graph(3)]
    hs = handles_of(graphs)
    batch = GraphBatch(hs, None, torch.device("cuda"))
    iters = 33
    keys = SR.keys(99, INDICES)
    P = np.random.RandomState(23).dirichlet([1, 1, 1], batch.R).astype(np.float32)
    got = run_seeded(pkg, batch, P, keys, iters)
    assert np.isfinite(got["cut_all"]).all()
    for g, (h, key) in enumerate(zip(hs, keys)):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        assert (got["assign_all"][:, lo:hi] == SR.assignments(P[lo:hi], key, iters)).all()
    refined = run_refine(pkg, batch, got["assign_all"], 0)
    assert (refined["assign"] == got["assign_all"]).all()
    assert (bits(refined["cut_all"]) == bits(got["cut_all"])).all()
    assert (bits(refined["best_cut"]) == bits(got["best_cut"])).all()
    assert (refined["best_idx"] == got["best_iter"]).all() and (refined["best_assign"] == got["best_assign"]).all()
    draws = [SR.uniforms(key, iters, h.n)[:, 3:] for h, key in zip(hs, keys)]
    uoff = np.zeros(batch.B + 1, np.int64)
    np.cumsum([d.size for d in draws], out=uoff[1:])
    u = torch.from_numpy(np.concatenate([d.ravel() for d in draws])).cuda()
    uo = torch.from_numpy(uoff).cuda()
    Pt = torch.from_numpy(P).cuda()
    assign_all = torch.full((iters, batch.R), GARBAGE, dtype=torch.int8, device="cuda")
    cut_all = torch.full((batch.B, iters), float("nan"), device="cuda")
    best_assign = torch.full((batch.R,), GARBAGE, dtype=torch.int32, device="cuda")
    best_cut = torch.full((batch.B,), float("nan"), device="cuda")
    best_iter = torch.full((batch.B,), GARBAGE, dtype=torch.int32, device="cuda")
    p = hip.ptr
    hip.check(hip.load().gmc_decode_sample_f32(batch.ref(), p(Pt), p(u), p(uo), iters, p(assign_all), p(cut_all),
                                               p(best_assign), p(best_cut), p(best_iter), hip.stream()), "decode")
    torch.cuda.synchronize()
    fed = dict(assign_all=assign_all, cut_all=cut_all, best_assign=best_assign, best_cut=best_cut, best_iter=best_iter)
    same_bytes(got, {k: v.cpu().numpy() for k, v in fed.items()})


def test_a_probed_call_is_tagged_sample(pkg):
    from gcn_max_cut_amd.graph import GraphBatch
    hs, P, keys, _refs = case_of("batch", 3)
    batch = GraphBatch(hs, None, torch.device("cuda"))
    with pkg.hip.Probe(8) as pr:
        run_seeded(pkg, batch, P, keys, 3)
    tags = [tag for tag, _ms in pr.records]
    assert tags == ["sample"] and "decode" not in tags
    assert pr.records[0][1] > 0


# ---- the Python entry points
def rng_state_equal(a, b):
    return a[0] == b[0] and (a[1] == b[1]).all() and a[2:] == b[2:]


def test_post_processing_optimization_with_a_seed(pkg, monkeypatch):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    monkeypatch.delenv(TN.SAMPLE_SEED_ENV, raising=False)
    g = R.regular_graph(60, 5, 60)
    (h,) = handles_of([g])
    P, _ = directed_probabilities(60, SR.keys(2 ** 63 + 5, [4])[0], 25, 8)
    np.random.seed(11)
    before = np.random.get_state()
    got_assign, got_cut = TN.post_processing_optimization(torch.from_numpy(P), g, 25, seed=2 ** 63 + 5, graph_index=4)
    assert rng_state_equal(before, np.random.get_state())              # numpy's RNG neither read nor advanced
    ref = SR.sample(h, P, SR.keys(2 ** 63 + 5, [4])[0], 25)
    assert got_assign == ref["best_assign"].tolist() and got_cut == float(ref["best_cut"])
    assert isinstance(got_cut, int) and got_cut == TN.calculate_cut_value(got_assign, g)
    assert got_assign == TN.assign_partitions_seeded(P, 2 ** 63 + 5, 4, ref["best_iter"])
    monkeypatch.setenv(TN.SAMPLE_SEED_ENV, str(2 ** 63 + 5))            # the switch, read at call time
    assert TN.post_processing_optimization(P, g, 25, graph_index=4) == (got_assign, got_cut)
    assert rng_state_equal(before, np.random.get_state())
    assert TN.post_processing_optimization(P, g, 0, seed=1) == (None, -float("inf"))


@pytest.fixture(scope="module")
def small_model(pkg):
    specs = [(50, 6, 50001), (100, 7, 100001), (30, 5, 30001)]
    ds = util.product_dataset(specs)
    T, cfg, net, embed, opt, _params = util.model(16)
    for _ in range(3):
        T.train_single_epoch(ds, net, opt, embed, cfg, graphs_per_step=len(ds))
    net.eval()
    return net, ds


OLD_KEYS = {'nodes', 'simple_cut', 'simple_assignment', 'post_cut', 'post_assignment', 'improvement'}


def test_decode_dataset_and_test_multiple_graphs_agree_under_a_seed(pkg, small_model, monkeypatch):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    monkeypatch.delenv(TN.SAMPLE_SEED_ENV, raising=False)
    net, ds = small_model
    seed = 12345
    np.random.seed(5)
    before = np.random.get_state()
    fast = TN.decode_dataset(net, ds, 8, sample_seed=seed)
    results, _ = TN.test_multiple_graphs(net, ds, [50, 100, 30], post_processing_iterations=8, verbose=False, seed=seed)
    assert rng_state_equal(before, np.random.get_state())
    assert len(fast) == len(results) == len(ds) == 3
    for index, (f, r, (g, a_pad, nx_g, _t)) in enumerate(zip(fast, results, ds.values())):
        assert set(f) == OLD_KEYS
        assert (f["simple_cut"], f["simple_assignment"], f["post_cut"], f["post_assignment"], f["improvement"]) == \
            (r["simple_cut"], r["simple_assignment"], r["post_cut"], r["post_assignment"], r["improvement"])
        with torch.no_grad():
            P = net(g, a_pad).cpu().numpy()
        ref = SR.sample(g, P, SR.keys(seed, [index])[0], 8)             # a graph's index: its position in the dataset
        assert f["post_assignment"] == ref["best_assign"].tolist() and f["post_cut"] == float(ref["best_cut"])
    # the two searches get the samples they refine, and change none of the other keys
    searched = TN.decode_dataset(net, ds, 8, local_search_sweeps=5, anneal_sweeps=5, sample_seed=seed)
    for f, s, (_g, _a, nx_g, _t) in zip(fast, searched, ds.values()):
        assert set(s) == OLD_KEYS | {'refined_cut', 'refined_assignment', 'refined_from',
                                     'annealed_cut', 'annealed_assignment', 'annealed_from'}
        assert {k: s[k] for k in OLD_KEYS} == f
        assert s["refined_cut"] >= max(f["simple_cut"], f["post_cut"]) <= s["annealed_cut"]
        assert s["refined_cut"] == TN.calculate_cut_value(s["refined_assignment"], nx_g)
        assert s["annealed_cut"] == TN.calculate_cut_value(s["annealed_assignment"], nx_g)
        assert 0 <= s["refined_from"] <= 8 and 0 <= s["annealed_from"] <= 8
    # the environment switch gives what the argument gives
    monkeypatch.setenv(TN.SAMPLE_SEED_ENV, str(seed))
    assert TN.decode_dataset(net, ds, 8) == fast
    via_env, _ = TN.test_multiple_graphs(net, ds, [50, 100, 30], post_processing_iterations=8, verbose=False)
    assert [r["post_assignment"] for r in via_env] == [f["post_assignment"] for f in fast]
    assert TN.decode_dataset(net, ds, 8, sample_seed=seed + 1) != fast  # (the argument wins)
    assert rng_state_equal(before, np.random.get_state())


def test_skipped_graphs_still_count_in_test_multiple_graphs(pkg, small_model, monkeypatch):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    monkeypatch.delenv(TN.SAMPLE_SEED_ENV, raising=False)
    net, ds = small_model
    fast = TN.decode_dataset(net, ds, 8, sample_seed=7)
    results, _ = TN.test_multiple_graphs(net, ds, [50, 30], post_processing_iterations=8, verbose=False, seed=7)
    assert [r["nodes"] for r in results] == [50, 30]                    # the 100-node graph is skipped, index 2 stays 2
    assert [r["post_assignment"] for r in results] == [fast[0]["post_assignment"], fast[2]["post_assignment"]]


def test_without_a_seed_the_numpy_stream_is_drawn_as_before(pkg, small_model, monkeypatch):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    monkeypatch.delenv(TN.SAMPLE_SEED_ENV, raising=False)
    net, ds = small_model
    np.random.seed(3)
    plain = TN.decode_dataset(net, ds, 8)
    after = np.random.get_state()
    eng = net.engine()
    batch = util.batch_of(pkg, eng, ds)
    P, _S, _loss = eng.forward(batch, 1.0, want_loss=True)
    np.random.seed(3)
    best_assign, best_cut, _cut_all, assign_all = TN._sample_on_gpu(batch, P, 8)   # the numpy branch, called directly
    assert rng_state_equal(after, np.random.get_state())                # the same number of draws
    assert tuple(assign_all.shape) == (8, batch.R)
    best_assign, best_cut = best_assign.cpu().numpy(), best_cut.cpu().numpy()
    for g, f in enumerate(plain):
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        assert f["post_assignment"] == best_assign[lo:hi].tolist() and f["post_cut"] == float(best_cut[g])
    assert plain != TN.decode_dataset(net, ds, 8, sample_seed=3)        # (another stream altogether)


def test_a_two_class_model_is_still_refused(pkg, monkeypatch):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.delenv(TN.SAMPLE_SEED_ENV, raising=False)
    cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=2)
    net, _embed, _opt = T.setup_model_and_optimizer(cfg)
    ds = GE.process_graphs_from_folder({0: R.regular_graph(40, 5, 51)}, {0: [3, 9]}, 64, number_classes=2)
    (g, a_pad, nx_g, _t), = ds.values()
    net.eval()
    with torch.no_grad():
        P = net(g, a_pad)
    assert tuple(P.shape) == (40, 2)
    with pytest.raises(ValueError, match="number_classes"):
        TN.decode_dataset(net, ds, 4, sample_seed=1)
    with pytest.raises(ValueError, match="number_classes"):
        TN.post_processing_optimization(P, nx_g, 4, seed=1)
    monkeypatch.setenv(TN.SAMPLE_SEED_ENV, "1")
    with pytest.raises(ValueError, match="number_classes"):
        TN.decode_dataset(net, ds, 4)
