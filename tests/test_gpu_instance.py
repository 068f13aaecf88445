"""GPU tests of one model per graph (gmc_inst_*, csrc/instance.hip, engine.InstanceEngine, solve_dataset) against the
float64 restatement of tests/instance_ref.py.

Bars: stepcheck's (P_TOL for the probabilities, ORACLE_BAR / ROW_TOL / ROW_FLOOR for every gradient row, the terminals'
rows of conv1.weight included) and LOSS_BAR = 5e-5 * C * total weight for weighted and relaxed losses, exactly as
tests/test_gpu_kway.py uses them.  S must be the reference's everywhere and the hard loss of a unit-weight graph exactly
-C * cut: tests/test_instance_host.py asserts on the float64 reference that no case has a row within 1e-5 of a tie or a
unit within 1e-6 of the relu kink.  It also asserts that a plain float32 numpy evaluation of every case (its own order,
nothing of the library in it) keeps half of ROW_TOL: on graphs of a handful of nodes with hundreds of hidden units a b1
entry that cancels to below ROW_FLOOR is beyond the row bar in any float32 arithmetic (instance_ref.f32_row_ratio says
why; with the seed the other two rules alone allow, the 8-node graph at hidden 516 missed the bar on the MI355X at the
very entry, column 21 of b1, at which that numpy evaluation misses it with a ratio of 5.5e-4 against 2e-4).

The cases are instance_ref.CASES: the batches (K, K+1, 65) and (5, 300, 65, 257) x K in {2, 3, 5, 8} (hidden 4, 12, 260,
516) x unit / real weights x both losses.  Two sizes are not literally those numbers: a GraphBatch takes graphs of at
least 3 nodes (K = 2: the first two graphs have 3), and a graph of 5 nodes cannot carry 8 terminals, so at K = 8 the
first graph of the second batch is the terminals-only graph of 8 nodes (what the 5-node graph is at K = 5).

No cross-talk: a graph whose parameters are NaN has a NaN loss under the relaxed loss; the hard loss is -C * cut of a
partition and stays a number (every comparison with NaN is false: class 0), so there the test asks for the other graphs'
bytes only."""
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import instance_ref as IR
from tests import kway_ref as KR
from tests import stepcheck, util
from tests.stepcheck import KEYS, ORACLE_BAR, P_TOL, ROW_FLOOR, ROW_TOL

pytestmark = pytest.mark.gpu
LOSS_BAR = 5e-5
CC = 1.3
TAGS = ["gather_w1", "agg_fwd", "dense_mfma", "head", "hidden_bwd", "colsum", "agg_bwd", "dw1"]


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def engine_with(pkg, handles, params):
    F, K = params[0]["conv2.weight"].shape
    eng = pkg.engine.InstanceEngine(handles, F, K)
    for g, p in enumerate(params):
        for k, v in eng.views(g).items():
            v.copy_(torch.from_numpy(p[k]))
    return eng


def run_step(pkg, eng, Cc, loss):
    """One poisoned train_fwd_bwd under the probe: the scratch and the gradient are NaN before it.  Returns P, S, loss,
    the per-graph gradient dicts, the launches' tags."""
    eng._workspace(True).fill_(255)
    eng.grad.fill_(float("nan"))
    with pkg.hip.Probe(64) as probe:
        P, S, losses = eng.train_fwd_bwd(Cc, loss=loss)
        grads = [{k: v.cpu().numpy() for k, v in eng.views(g, eng.grad).items()} for g in range(eng.B)]
    assert not any(probe.flavours)
    return P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads, [t for t, _ms in probe.records]


def graph_bytes(eng, out, g):
    """Everything a step reports of graph g, as bytes: its rows of P and S, its loss, its four gradient slices."""
    P, S, losses, grads, _tags = out
    r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
    return (P[r0:r1].tobytes(), S[r0:r1].tobytes(), losses[g:g + 1].tobytes()) + tuple(grads[g][k].tobytes() for k in KEYS)


def judge(eng, out, refs, csrs, params, Cc, exact_loss, what):
    P, S, losses, grads, _tags = out
    K = eng.K
    assert P.shape == (eng.R, K) and np.isfinite(P).all() and losses.dtype == np.float32
    worst_p = worst_rows = worst_loss = 0.0
    for g, (ref, csr, p) in enumerate(zip(refs, csrs, params)):
        r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
        p_err = float(np.abs(P[r0:r1] - ref.P).max())
        assert p_err < P_TOL, (what, g, p_err)
        assert np.array_equal(S[r0:r1], KR.partition(ref.P, K)), (what, g)
        bar = LOSS_BAR * Cc * KR.total_weight([csr])
        err = abs(float(losses[g]) - ref.loss[0])
        print(f"{what} graph {g}: loss {losses[g]:.6f} float64 {ref.loss[0]:.6f} err {err:.2e} bar {bar:.2e}")
        if exact_loss:   # unit weights: the cut is an integer, the loss its one float32 product with -C
            cut = round(-ref.loss[0] / Cc)
            assert abs(-ref.loss[0] / Cc - cut) < 1e-9 and losses[g] == -(np.float32(Cc) * np.float32(cut)), (what, g)
        assert err <= bar, (what, g, losses[g], ref.loss[0])
        res = stepcheck.compare_grads(grads[g], ref.grads, what=(what, g), grad_bar=ORACLE_BAR, row_tol=ROW_TOL,
                                      row_floor=ROW_FLOOR, kinks=(1e-7, 3), csrs=[csr], params=p, sparse=True)
        assert not res["bad_cols"], (what, g, res)
        worst_p, worst_rows, worst_loss = max(worst_p, p_err), max(worst_rows, res["rows"]), max(worst_loss, err)
    print(f"{what}: P {worst_p:.2e} rows {worst_rows:.2e} loss {worst_loss:.2e}")


def case_setup(pkg, case):
    handles = [pkg.from_networkx(g) for g in IR.case_graphs(case)]
    return handles, [KR.csr_of_handle(h) for h in handles], IR.case_params(case)


# ---- one poisoned step of every case against float64
@pytest.mark.parametrize("case", IR.CASES, ids=IR.case_id)
def test_step_against_float64(pkg, case):
    handles, csrs, params = case_setup(pkg, case)
    eng = engine_with(pkg, handles, params)
    assert (eng.batch.host.vals is not None) == (case.weights == "real")
    assert eng.count == IR.flat_offsets([h.n for h in handles], IR.HIDDEN[case.K], case.K)[-1]
    assert np.array_equal(eng.flat[:eng.count].cpu().numpy(), IR.pack(params))
    out = run_step(pkg, eng, CC, case.loss)
    assert out[4] == TAGS, out[4]
    refs = IR.batch_step(csrs, params, CC, case.loss)
    what = IR.case_id(case)
    judge(eng, out, refs, csrs, params, CC, case.loss == "cut" and case.weights == "unit", what)
    # a second step gives the same bytes; the forward alone reports the same P, S and loss
    again = run_step(pkg, eng, CC, case.loss)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], again[:3]))
    assert eng.grad[:eng.count].cpu().numpy().tobytes() == np.concatenate(
        [np.concatenate([g[k].ravel() for g in out[3]]) for k in KEYS]).tobytes()
    with pkg.hip.Probe(16) as probe:
        Pf, Sf, lf = (t.cpu().numpy() for t in eng.forward(CC, loss=case.loss))
    assert [t for t, _ms in probe.records] == TAGS[:4]
    assert np.array_equal(Pf, out[0]) and np.array_equal(Sf, out[1]) and np.array_equal(lf, out[2]), what


# ---- independence, byte for byte
@pytest.mark.parametrize("case", [IR.Case("mixed", 3, "real", "cut", 0), IR.Case("mixed", 5, "unit", "expected_cut", 0),
                                  IR.Case("mixed", 8, "real", "expected_cut", 3)], ids=IR.case_id)
def test_a_graph_does_not_depend_on_its_batch(pkg, case):
    """Each graph of the (5, 300, 65, 257) batch alone, first, in the middle and last: the same bytes every time, those of
    the whole batch's step included; a second run of the same step gives them again."""
    handles, _csrs, params = case_setup(pkg, case)
    eng = engine_with(pkg, handles, params)
    whole = run_step(pkg, eng, CC, case.loss)
    assert [graph_bytes(eng, run_step(pkg, eng, CC, case.loss), g) for g in range(4)] == \
        [graph_bytes(eng, whole, g) for g in range(4)]
    for g in range(4):
        want = graph_bytes(eng, whole, g)
        a, b = [i for i in range(4) if i != g][:2]
        for order in ([g], [g, a, b], [a, g, b], [a, b, g]):
            e = engine_with(pkg, [handles[i] for i in order], [params[i] for i in order])
            assert graph_bytes(e, run_step(pkg, e, CC, case.loss), order.index(g)) == want, (g, order)


# ---- no cross-talk
@pytest.mark.parametrize("loss", ("expected_cut", "cut"))
def test_nan_parameters_of_one_graph_stay_in_that_graph(pkg, loss):
    case = IR.Case("mixed", 5, "real", loss, 0)
    handles, _csrs, params = case_setup(pkg, case)
    eng = engine_with(pkg, handles, params)
    clean = run_step(pkg, eng, CC, loss)
    for v in eng.views(1).values():
        v.fill_(float("nan"))
    dirty = run_step(pkg, eng, CC, loss)
    for g in (0, 2, 3):
        assert graph_bytes(eng, dirty, g) == graph_bytes(eng, clean, g), g
    if loss == "expected_cut":
        assert np.isnan(dirty[2][1])
    assert np.isnan(dirty[0][300 // 2 + 5]).all()                    # (a row of graph 1: its probabilities are gone)
    assert np.isfinite(dirty[2][[0, 2, 3]]).all()


# ---- three epochs against the float64 Adam replay
@pytest.mark.parametrize("K", (2, 4))
def test_three_epochs_against_a_float64_adam_replay(pkg, K):
    """train_fwd_bwd + adam_step three times on two graphs from the engine's own init: after every step the moments and
    the parameter update of every graph are those of a float64 Adam step from the device's state before it, with the
    gradient of the partition the device chose (bars of test_trainer_epochs_against_a_float64_adam_replay: m 1e-4, v 2e-4
    of the largest, update within 2 % where the gradient is at least 1 % of the largest).  hidden_dim = 10 is padded to 12
    inside: the padding columns stay exactly zero."""
    F, lr = 10, 1e-3
    graphs = [R.regular_graph(60, 7, 31), R.regular_graph(48, 6, 32)]
    handles = [pkg.from_networkx(g) for g in graphs]
    csrs = [KR.csr_of_handle(h) for h in handles]
    eng = pkg.engine.InstanceEngine(handles, F, K)
    assert eng.Fp == 12 and eng.count == 108 * 12 + 2 * (12 + 12 * K + K)
    torch.manual_seed(K)
    eng.reset_parameters()
    torch.manual_seed(K)
    for g, (w1, w2) in enumerate(pkg.engine.draw_instance_parameters([60, 48], F, K)):
        v = eng.views(g)
        assert torch.equal(v["conv1.weight"].cpu(), w1) and torch.equal(v["conv2.weight"].cpu(), w2)
        assert not v["conv1.bias"].any() and not v["conv2.bias"].any()
    snap = lambda buf: [{k: t.cpu().numpy().astype(np.float64) for k, t in eng.views(g, buf).items()} for g in range(2)]  # noqa: E731
    for t in range(1, 4):
        before, m0, v0 = snap(eng.flat), snap(eng.m), snap(eng.v)
        _P, S, losses = eng.train_fwd_bwd(1.0)
        eng.adam_step(lr)
        assert eng.step_count == t
        params32 = [{k: b[k].astype(np.float32) for k in KEYS} for b in before]
        refs = IR.batch_step(csrs, params32, 1.0, "cut", S_got=S.cpu().numpy())
        after, m_got, v_got = snap(eng.flat), snap(eng.m), snap(eng.v)
        for g, ref in enumerate(refs):
            assert losses[g].item() == np.float32(ref.loss[0]), (t, g)                     # -cut: exact
            for k in KEYS:
                gr = ref.grads[k]
                m1, v1, upd = IR.adam_f64(m0[g][k], v0[g][k], gr, t, lr)
                assert np.abs(m_got[g][k] - m1).max() <= 1e-4 * max(np.abs(m1).max(), 1e-30), (t, g, k)
                assert np.abs(v_got[g][k] - v1).max() <= 2e-4 * max(np.abs(v1).max(), 1e-30), (t, g, k)
                big = np.abs(gr) >= 1e-2 * np.abs(gr).max()
                rel = np.abs((after[g][k] - before[g][k]) - upd)[big] / np.abs(upd[big])
                assert big.any() and rel.max() < 0.02, (t, g, k, rel.max())
        for buf in (eng.flat, eng.grad, eng.m, eng.v):
            b = eng.blocks(buf)
            assert not b["conv1.weight"][:, F:].any() and not b["conv1.bias"][:, F:].any()
            assert not b["conv2.weight"][:, F:].any()


# ---- keep-best
def test_keep_best_against_the_host_restatement(pkg):
    case = IR.Case("mixed", 3, "unit", "cut", 0)
    handles, _csrs, params = case_setup(pkg, case)
    eng = engine_with(pkg, handles, params)
    host = IR.KeepBest(eng.batch.goff_host)
    assert torch.isinf(eng.best_loss).all() and (eng.best_epoch == -1).all()

    def same():
        assert eng.best_loss.cpu().numpy().tobytes() == host.best_loss.tobytes()
        assert eng.best_epoch.cpu().numpy().tobytes() == host.best_epoch.tobytes()
        assert eng.best_S.cpu().numpy().tobytes() == host.best_S.tobytes()

    history = []
    for epoch in range(6):
        _P, S, losses = eng.train_fwd_bwd(1.0)
        eng.adam_step(3e-2)
        with pkg.hip.Probe(8) as probe:
            eng.keep_best(S, losses, epoch)
        assert [t for t, _ms in probe.records] == ["finish", "finish"]
        host.update(S.cpu().numpy(), losses.cpu().numpy(), epoch)
        history.append(losses.cpu().numpy())
        same()
        if epoch == 0:
            assert (host.best_epoch == 0).all()                                     # epoch 0 wins against +inf
    history = np.stack(history)
    assert np.array_equal(host.best_loss, history.min(0)) and np.array_equal(host.best_epoch, history.argmin(0))
    assert len({h.tobytes() for h in history}) > 1                                  # (the losses did move)
    # made-up outcomes on the device: a NaN, a tie with the best, a new minimum, a worse loss
    S = torch.arange(eng.R, dtype=torch.int32, device=eng.device)
    best = eng.best_loss.clone()
    losses = torch.stack([best[0] * float("nan"), best[1], best[2] - 1.0, best[3] + 1.0])
    eng.keep_best(S, losses, 99)
    host.update(S.cpu().numpy(), losses.cpu().numpy(), 99)
    same()
    assert host.best_epoch.tolist()[2] == 99 and 99 not in host.best_epoch.tolist()[:2] + host.best_epoch.tolist()[3:]
    assert host.best_S[305:370].tolist() == list(range(305, 370))


# ---- module(g)
def dataset_for(K, specs, N):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: [int(t) for t in np.random.RandomState(s).permutation(n)[:K]] for i, (n, d, s) in enumerate(specs)}
    ds = GE.process_graphs_from_folder(graphs, terms, N, number_classes=K)
    assert len(ds) == len(specs) and all(it[3] == list(range(K)) for it in ds.values())
    return ds


def test_module_of_a_graph_is_an_ordinary_model(pkg):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    K, F = 4, 16
    ds = dataset_for(K, [(40, 5, 41), (30, 4, 42), (52, 6, 43)], 64)
    items = list(ds.values())
    handles = [it[0] for it in items]
    eng = pkg.engine.InstanceEngine(handles, F, K, values=[h.edge_values(it[1]) for h, it in zip(handles, items)])
    torch.manual_seed(9)
    eng.reset_parameters()
    state = torch.random.get_rng_state()
    P, _S, losses = eng.forward(1.0)
    for g, item in enumerate(items):
        net = eng.module(g)
        n = item[0].n
        assert isinstance(net, T.GCNSoftmax) and tuple(net.conv1.weight.shape) == (n, F)
        assert tuple(net.conv2.weight.shape) == (F, K)
        for k, v in eng.views(g).items():
            assert torch.equal(dict(net.named_parameters())[k].detach().cpu(), v.cpu()), k
            assert dict(net.named_parameters())[k].data_ptr() != v.data_ptr()           # copies
        cfg = T.TrainingConfig(n_nodes=n, hidden_dim=F, number_classes=K)
        ev = T.evaluate_model(net, {0: item}, cfg)
        assert ev["num_samples"] == 1 and ev["total_loss"] == float(losses[g]), (g, ev, float(losses[g]))
        with torch.no_grad():
            Pg = net(item[0], item[1])
        r0 = int(eng.batch.goff_host[g])
        err = float((Pg - P[r0:r0 + n]).abs().max())
        print(f"module({g}): P err {err:.2e}")
        assert tuple(Pg.shape) == (n, K) and err < P_TOL
    assert torch.equal(torch.random.get_rng_state(), state)                            # building modules draws nothing


# ---- solve_dataset end to end
@pytest.mark.parametrize("K", (3, 2))
@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
def test_solve_dataset_end_to_end(pkg, K, loss):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    ds = dataset_for(K, [(40, 5, 41), (30, 4, 42)], 64)
    cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=K, number_epochs=20, learning_rate=1e-2, patience=1)
    torch.manual_seed(5)
    one = T.solve_dataset(ds, cfg, loss=loss)
    torch.manual_seed(5)
    two = T.solve_dataset(ds, cfg, loss=loss, max_rows_per_chunk=40)
    assert len(one) == len(two) == 2
    for res, other, item in zip(one, two, ds.values()):
        n = item[0].n
        assert list(res) == ["best_loss", "best_epoch", "partition", "cut", "probabilities", "loss_history", "model"]
        assert len(res["partition"]) == n and res["partition"][:K] == list(range(K))
        assert set(res["partition"]) <= set(range(K))
        assert res["cut"] == TN.calculate_cut_value(res["partition"], item[2])
        hist = res["loss_history"]
        assert len(hist) == 20 and all(np.isfinite(hist))                          # (no early stopping: patience ignored)
        assert res["best_loss"] == min(hist) and res["best_epoch"] == hist.index(min(hist))
        if loss == "cut":
            assert res["best_loss"] == -float(res["cut"])
        assert tuple(res["probabilities"].shape) == (n, K)
        assert torch.allclose(res["probabilities"].sum(1), torch.ones(n), atol=1e-5)
        # two chunks under the same seed: byte for byte
        for key in ("best_loss", "best_epoch", "partition", "cut", "loss_history"):
            assert res[key] == other[key], key
        assert torch.equal(res["probabilities"], other["probabilities"])
        net, onet = res["model"](), other["model"]()
        assert isinstance(net, T.GCNSoftmax) and tuple(net.conv1.weight.shape) == (n, 8)
        for a, b in zip(net.parameters(), onet.parameters()):
            assert torch.equal(a, b)
        # the model is the last epoch's: its forward gives the probabilities of one more step's forward, not the kept ones
        ev = T.evaluate_model(net, {0: item}, T.TrainingConfig(n_nodes=n, hidden_dim=8, number_classes=K), loss=loss)
        assert np.isfinite(ev["total_loss"])
    with pytest.raises(NotImplementedError, match="dropout"):
        T.solve_dataset(ds, T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=K, dropout=0.5))
    with pytest.raises(ValueError, match="at least 8 nodes"):
        T.solve_dataset({0: [pkg.from_networkx(util.near_regular(6, 3, 1)), None, util.near_regular(6, 3, 1), [0, 1, 2]]},
                        T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=8))


# ---- the one shared kernel touched: the K-class head through gmc_kway_train_fwd_bwd
def test_kway_step_gives_the_same_bytes_twice(pkg):
    case = KR.CASES[12]                                              # batch3, K = 4, real weights, hard loss
    handles = [pkg.from_networkx(g) for g in KR.case_graphs(case)]
    params = KR.case_params(case)
    N, F = params["conv1.weight"].shape
    eng = pkg.engine.FusedEngine(N, F, case.K, kway=True)
    for k, v in eng.views().items():
        v.copy_(torch.from_numpy(params[k]))
    batch = pkg.GraphBatch(handles, None, eng.device)
    outs = []
    for _ in range(2):
        util.poison(eng, batch)
        P, S, losses = eng.train_fwd_bwd(batch, CC, loss=case.loss)
        outs.append((P.cpu().numpy().tobytes(), S.cpu().numpy().tobytes(), losses.cpu().numpy().tobytes(),
                     eng.grad[:eng.count + 1].cpu().numpy().tobytes()))
    assert outs[0] == outs[1]
    ref = KR.f64_step([KR.csr_of_handle(h) for h in handles], params, CC, case.loss)
    assert np.abs(np.frombuffer(outs[0][0], np.float32).reshape(-1, case.K) - ref.P).max() < P_TOL
