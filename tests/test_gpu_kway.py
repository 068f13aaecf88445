"""GPU tests of the K-class model (number_classes K in 2..8; gmc_kway_* and csrc/kway.hip) against the float64
restatement of tests/kway_ref.py: one poisoned training step per case of kway_ref.CASES (the smallest shapes at which
each K-wide kernel can go wrong, K in {2, 4, 5, 8}, unit and real-valued weights, both losses), K = 3 through the new
entry point against the fused 3-way one, the trainer's eager sequence against a float64 Adam replay,
train_multi_class(num_classes=2) with its checkpoint and evaluate_model, the documented refusals, and the 3-way step
around a K-way call.

Bars: stepcheck's (P_TOL for the probabilities, ORACLE_BAR / ROW_TOL / ROW_FLOOR for the gradient).  S must be the
reference's everywhere: tests/test_kway_host.py asserts on the float64 reference that no case has a row within 1e-5 of
a tie or a unit within 1e-6 of the relu kink.  The hard loss of a unit-weight graph is exactly -C * cut; weighted and
relaxed losses are within 5e-5 * C * (total edge weight), as tests/test_gpu_expected_cut.py judges its losses.

Measured on the MI355X (the tests print each figure with -s), worst over the 22 cases: P 2.4e-7 (bar 5e-7); gradient row
ratio 1.6e-4 (hidden 516, K = 4, real weights; 1.4e-4 at n = K + 1 = 3, below 1e-5 for most cases; bar 2e-4); relaxed /
weighted loss 2.1e-4 absolute on a loss near -7,700 (n = 1030, K = 8; bar 0.39)."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import kway_ref as KR
from tests import stepcheck, util
from tests.stepcheck import KEYS, ORACLE_BAR, P_TOL, ROW_FLOOR, ROW_TOL

pytestmark = pytest.mark.gpu
LOSS_BAR = 5e-5
CC = 1.3


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def engine_with(pkg, params):
    N, F = params["conv1.weight"].shape
    K = params["conv2.weight"].shape[1]
    eng = pkg.engine.FusedEngine(N, F, K, kway=K != 3)
    for k, v in eng.views().items():
        v.copy_(torch.from_numpy(params[k]))
    return eng


def run_step(pkg, eng, batch, Cc, loss, fuse=None):
    """One poisoned train_fwd_bwd under the probe (stepcheck.run_step with the loss keyword)."""
    with util.fused(pkg, fuse):
        util.poison(eng, batch)
        with pkg.hip.Probe(64) as probe:
            P, S, losses = eng.train_fwd_bwd(batch, Cc, loss=loss)
            grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}
    return stepcheck.Step(P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads, float(eng.grad[eng.count]),
                          [t for t, _ms in probe.records], list(probe.flavours))


def grad_rules(csrs, params):
    return dict(grad_bar=ORACLE_BAR, row_tol=ROW_TOL, row_floor=ROW_FLOOR, kinks=(1e-7, 3), csrs=csrs, params=params,
                sparse=True)


def wave_sum32(values):
    """The sum the library puts behind the gradient (loss_tail_kernel, and the fused fold): float32, the values dealt over
    64 lanes, then the butterfly of gmc::wave_sum (lane distances 32, 16, .., 1) - lane 0's total."""
    lanes = np.zeros(64, np.float32)
    for b, v in enumerate(np.asarray(values, np.float32)):
        lanes[b % 64] = np.float32(lanes[b % 64] + v)
    idx = np.arange(64)
    for dist in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[idx ^ dist]).astype(np.float32)
    return lanes[0]


def judge(got, ref, csrs, params, Cc, exact_loss, what):
    """A Step against the float64 Ref: P, S identical to the reference's decode, the losses, the tail, the gradient."""
    K = params["conv2.weight"].shape[1]
    assert got.P.shape == ref.P.shape and got.P.shape[1] == K, what
    p_err = float(np.abs(got.P - ref.P).max())
    assert np.isfinite(got.P).all() and p_err < P_TOL, (what, p_err)
    off, worst = 0, 0.0
    for g, (rp, _cl, _vl) in enumerate(csrs):
        n = len(rp) - 1
        assert np.array_equal(got.S[off:off + n], KR.partition(ref.P[off:off + n], K)), (what, g)
        bar = LOSS_BAR * Cc * KR.total_weight([csrs[g]])
        err = abs(float(got.loss[g]) - ref.loss[g])
        print(f"{what} graph {g}: loss {got.loss[g]:.6f} float64 {ref.loss[g]:.6f} err {err:.2e} bar {bar:.2e}")
        if exact_loss:   # unit weights: the cut is an integer, the loss its one float32 product with -C
            cut = round(-ref.loss[g] / Cc)
            assert abs(-ref.loss[g] / Cc - cut) < 1e-9 and got.loss[g] == -(np.float32(Cc) * np.float32(cut)), \
                (what, g, got.loss[g], ref.loss[g])
        assert err <= bar, (what, g, got.loss[g], ref.loss[g])
        worst = max(worst, err)
        off += n
    assert got.loss.dtype == np.float32 and got.tail == float(wave_sum32(got.loss)), (what, got.tail)
    res = stepcheck.compare_grads(got.grads, ref.grads, what=what, **grad_rules(csrs, params))
    assert not res["bad_cols"], (what, res)                      # (no unit of a case is near the relu kink)
    print(f"{what}: P {p_err:.2e} rows {res['rows']:.2e} loss {worst:.2e}")
    return res


# ---- every case of the list: one whole step against float64
@pytest.mark.parametrize("case", KR.CASES, ids=KR.case_id)
def test_step_against_float64(pkg, case):
    handles = [pkg.from_networkx(g) for g in KR.case_graphs(case)]
    csrs = [KR.csr_of_handle(h) for h in handles]
    params = KR.case_params(case)
    eng = engine_with(pkg, params)
    batch = pkg.GraphBatch(handles, None, eng.device)
    assert (batch.host.vals is not None) == (case.weights == "real")
    got = run_step(pkg, eng, batch, CC, case.loss)
    assert got.tags == ["gather_w1", "agg_fwd", "dense_mfma", "head", "hidden_bwd", "colsum", "agg_bwd", "dw1"], got.tags
    assert not any(got.flavours)                                 # row kernels only: no LDS-tiled launch
    ref = KR.f64_step(csrs, params, CC, case.loss)
    what = KR.case_id(case)
    judge(got, ref, csrs, params, CC, case.loss == "cut" and case.weights == "unit", what)
    assert not got.grads["conv1.weight"][batch.n_max:].any()     # rows past every graph's n: exactly 0
    # a second step gives the same bytes; the forward alone reports the same P, S and loss
    again = run_step(pkg, eng, batch, CC, case.loss)
    assert again.P.tobytes() == got.P.tobytes() and again.loss.tobytes() == got.loss.tobytes()
    for k in KEYS:
        assert again.grads[k].tobytes() == got.grads[k].tobytes(), k
    Pf, Sf, lf = (t.cpu().numpy() for t in eng.forward(batch, CC, want_loss=True, loss=case.loss))
    assert np.array_equal(Pf, got.P) and np.array_equal(Sf, got.S) and np.array_equal(lf, got.loss), what


# ---- K = 3 through the new entry point against the fused 3-way one
@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
def test_three_classes_through_the_kway_entry_against_the_fused_one(pkg, loss):
    handles = [pkg.from_networkx(g) for g in KR.three_way_graphs()]
    csrs = [KR.csr_of_handle(h) for h in handles]
    params = KR.three_way_params()
    eng = engine_with(pkg, params)
    assert not eng.kway
    batch = pkg.GraphBatch(handles, None, eng.device)
    old = run_step(pkg, eng, batch, CC, loss, fuse=1)
    assert "fwd1_fused" in old.tags and "bwd1_fused" in old.tags, old.tags
    # the same engine's model struct and gradient buffer through gmc_kway_train_fwd_bwd
    lib, p = pkg.hip.load(), pkg.hip.ptr
    model = eng._call_model(loss=loss)
    need = int(lib.gmc_kway_workspace_bytes(batch.ref(), C.byref(model), 1))
    ws = torch.full((need,), 255, dtype=torch.uint8, device="cuda")
    P = torch.full((batch.R, 3), float("nan"), device="cuda")
    S = torch.full((batch.R,), -1, dtype=torch.int32, device="cuda")
    losses = torch.full((batch.B,), float("nan"), device="cuda")
    eng.grad.fill_(float("nan"))
    with pkg.hip.Probe(64) as probe:
        rc = lib.gmc_kway_train_fwd_bwd(batch.ref(), C.byref(model), CC, p(ws), need, p(P), p(S), p(losses), p(eng.grad),
                                        pkg.hip.stream())
        pkg.hip.check(rc, "gmc_kway_train_fwd_bwd")
    new = stepcheck.Step(P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(),
                         {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}, float(eng.grad[eng.count]),
                         [t for t, _ms in probe.records], list(probe.flavours))
    assert new.tags[:4] == ["gather_w1", "agg_fwd", "dense_mfma", "head"] and not any(new.flavours), new.tags
    assert np.array_equal(new.S, old.S)
    if loss == "cut":
        assert new.loss.tobytes() == old.loss.tobytes()          # unit weights: -C * cut, bit for bit
    ref = KR.f64_step(csrs, params, CC, loss)
    for name, got in (("fused", old), ("kway", new)):
        judge(got, ref, csrs, params, CC, loss == "cut", f"K=3 {loss} {name}")
    # FusedEngine(..., 3, kway=True): the engine's own route to the same sequence, byte for byte
    keng = pkg.engine.FusedEngine(*params["conv1.weight"].shape, 3, kway=True)
    for k, v in keng.views().items():
        v.copy_(torch.from_numpy(params[k]))
    assert keng.kway
    via = run_step(pkg, keng, batch, CC, loss)
    assert via.tags == new.tags and via.tail == new.tail
    assert via.P.tobytes() == new.P.tobytes() and via.S.tobytes() == new.S.tobytes() and via.loss.tobytes() == new.loss.tobytes()
    for k in KEYS:
        assert via.grads[k].tobytes() == new.grads[k].tobytes(), k
    with pytest.raises(NotImplementedError, match="number_classes"):
        keng.train_step(batch, 1e-3)


# ---- the trainer's eager sequence against a float64 Adam replay
def dataset_for(pkg, K, specs, N):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: [int(t) for t in np.random.RandomState(s).permutation(n)[:K]] for i, (n, d, s) in enumerate(specs)}
    ds = GE.process_graphs_from_folder(graphs, terms, N, number_classes=K)
    assert len(ds) == len(specs) and all(it[3] == list(range(K)) for it in ds.values())
    return ds


@pytest.mark.parametrize("K", (2, 4))
def test_trainer_epochs_against_a_float64_adam_replay(pkg, K):
    """Three epochs of FusedTrainer.epoch on two graphs (one step per epoch): the returned loss is the sum of the per-graph
    losses, and after every step the moments and the parameter update are those of a float64 Adam step from the device's
    state before it, with the gradient of the partition the device chose (the bars of
    test_adam_parity_step_by_step_on_the_reference_schedule: m 1e-4, v 2e-4 of the largest, update within 2 % where the
    gradient is at least 1 % of the largest)."""
    from gcn_max_cut_amd.Training import TrainingNeural as T
    N, F = 128, 16
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=F, number_classes=K, learning_rate=1e-3)
    torch.manual_seed(K)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    ds = dataset_for(pkg, K, [(60, 7, 31), (48, 6, 32)], N)
    csrs = util.csrs_of(ds)
    tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=2)
    eng = tr.eng
    assert eng.kway and eng.K == K
    net.train()
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, cfg.learning_rate
    for t in range(1, 4):
        before = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views().items()}
        m0 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.m).items()}
        v0 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.v).items()}
        total = tr.epoch(ds)
        assert eng.step_count == t
        per_graph = tr._loss_slots[0, :2].cpu().numpy()
        assert total == float(per_graph.sum(dtype=np.float32)), (t, total, per_graph)
        assert tr._out[0].shape[1] == K
        S = tr._out[1][:eng_rows(ds)].cpu().numpy()
        params32 = {k: before[k].astype(np.float32) for k in KEYS}
        ref = KR.f64_step(csrs, params32, cfg.C, "cut", S_got=S)
        assert np.array_equal(per_graph, ref.loss.astype(np.float32)), (t, per_graph, ref.loss)   # -cut: exact
        for k in KEYS:
            g = ref.grads[k]
            m1 = b1 * m0[k] + (1 - b1) * g
            v1 = b2 * v0[k] + (1 - b2) * g * g
            upd = -lr / (1 - b1 ** t) * m1 / (np.sqrt(v1) / np.sqrt(1 - b2 ** t) + eps)
            m_got, v_got = eng.views(eng.m)[k].cpu().numpy(), eng.views(eng.v)[k].cpu().numpy()
            assert np.abs(m_got - m1).max() <= 1e-4 * max(np.abs(m1).max(), 1e-30), (t, k)
            assert np.abs(v_got - v1).max() <= 2e-4 * max(np.abs(v1).max(), 1e-30), (t, k)
            got_upd = eng.views()[k].cpu().numpy().astype(np.float64) - before[k]
            big = np.abs(g) >= 1e-2 * np.abs(g).max()
            rel = np.abs(got_upd - upd)[big] / np.abs(upd[big])
            assert big.any() and rel.max() < 0.02, (t, k, rel.max())
    sd = net.state_dict()
    assert tuple(sd["conv2.weight"].shape) == (F, K) and tuple(sd["conv2.bias"].shape) == (K,)


def eng_rows(ds):
    return sum(it[0].n for it in ds.values())


# ---- train_multi_class(num_classes=2), its checkpoint, evaluate_model
def test_train_multi_class_two_way_checkpoint_and_evaluation(pkg, tmp_path, monkeypatch):
    from gcn_max_cut_amd import commons
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.chdir(tmp_path)
    N, F = 64, 8
    ds = dataset_for(pkg, 2, [(40, 5, 41), (30, 4, 42)], N)
    commons.save_object(ds, str(tmp_path / "two.pkl"))
    torch.manual_seed(3)
    net, best, epoch, _w, history = T.train_multi_class(str(tmp_path / "two.pkl"), "two_way", num_classes=2, n_nodes=N,
                                                        hidden_dim=F, number_epochs=2, learning_rate=1e-2)
    assert epoch == 1 and len(history) == 2 and best == min(history) and all(np.isfinite(history))
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=F, number_classes=2)
    loaded, _inputs, saved_cfg = T.load_neural_model(str(tmp_path / "final_two_way.pth"), cfg)
    assert saved_cfg.number_classes == 2
    sd = loaded.state_dict()
    assert tuple(sd["conv2.weight"].shape) == (F, 2) and tuple(sd["conv2.bias"].shape) == (2,)
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    ev = T.evaluate_model(loaded, ds, cfg)
    cuts = []
    for handle, a_pad, nx_g, _t in ds.values():
        with torch.no_grad():
            P = loaded(handle, a_pad)
        assert tuple(P.shape) == (handle.n, 2)
        part = TN.simple_partition_assignment(P)
        assert part[:2] == [0, 1]
        cuts.append(sum(d.get("weight", 1) for u, v, d in nx_g.edges(data=True) if part[u] != part[v]))
        assert cuts[-1] == TN.calculate_cut_value(part, nx_g)
        res = TN.test_single_graph(loaded, handle, a_pad, nx_g, [0, 1], post_processing_iterations=0)
        assert res["success"] and res["simple_cut"] == cuts[-1] and res["simple_assignment"] == part
    assert ev["num_samples"] == 2 and ev["total_loss"] == -float(sum(cuts))
    soft = T.evaluate_model(loaded, ds, cfg, loss="expected_cut")
    assert np.isfinite(soft["total_loss"]) and soft["total_loss"] != ev["total_loss"]


# ---- what a model with another class count refuses
def test_refusals_of_a_two_class_model(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=2)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    ds = dataset_for(pkg, 2, [(40, 5, 51)], 64)
    (g, a_pad, nx_g, _t), = ds.values()
    net.eval()
    with pytest.raises(NotImplementedError, match="train_model"):
        net(g, a_pad)                                            # with gradients
    with torch.no_grad():
        P = net(g, a_pad)
    assert tuple(P.shape) == (40, 2)
    with pytest.raises(ValueError, match="number_classes"):
        TN.decode_dataset(net, ds, 4)
    with pytest.raises(ValueError, match="number_classes"):
        T.cut_loss(g, P)
    with pytest.raises(ValueError, match="number_classes"):
        TN.post_processing_optimization(P, nx_g, 4)
    eng = net.engine()
    batch = pkg.GraphBatch([g], None, eng.device)
    for call in (lambda: eng.train_step(batch, 1e-3), lambda: eng.ensure_slab(), lambda: eng.set_dropout(0.5),
                 lambda: eng.backward_from_gp(batch, P, P), lambda: eng.workspace_bytes_features(batch, True),
                 lambda: eng.forward_features(batch, torch.zeros(40, 64))):
        with pytest.raises(NotImplementedError, match="number_classes"):
            call()
    drop_cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=2, dropout=0.25)
    dnet, dembed, dopt = T.setup_model_and_optimizer(drop_cfg)
    with pytest.raises(NotImplementedError, match="number_classes"):
        T.train_single_epoch(ds, dnet, dopt, dembed, drop_cfg)
    small = pkg.GraphBatch([pkg.from_networkx(nx.path_graph(3))], None, eng.device)
    eng5 = pkg.engine.FusedEngine(64, 8, 5, kway=True)
    with pytest.raises(ValueError, match="at least 5 nodes"):
        eng5.forward(small)
    for K, kw in ((1, dict(kway=True)), (9, dict(kway=True)), (2, {})):   # (2 without kway: the 3-class constructor)
        with pytest.raises(ValueError, match="number_classes"):
            pkg.engine.FusedEngine(64, 8, K, **kw)


# ---- the 3-way step is what it was, around a K-way call
def test_three_way_step_is_unchanged_by_a_kway_call(pkg):
    ds = util.product_dataset([(60, 7, 61), (48, 6, 62)])
    outs = []
    for between in (False, True):
        T, cfg, net, embed, opt, params = util.model(32, seed=5)
        eng = net.engine()
        batch = util.batch_of(pkg, eng, ds)
        if between:
            case = KR.CASES[8]
            handles = [pkg.from_networkx(g) for g in KR.case_graphs(case)]
            keng = engine_with(pkg, KR.case_params(case))
            assert type(keng) is type(eng) and keng.kway
            run_step(pkg, keng, pkg.GraphBatch(handles, None, keng.device), CC, case.loss)
        got = stepcheck.run_step(pkg, eng, batch, 1.0)
        outs.append(got)
    a, b = outs
    assert a.tags == b.tags and a.flavours == b.flavours
    assert a.P.tobytes() == b.P.tobytes() and a.S.tobytes() == b.S.tobytes() and a.loss.tobytes() == b.loss.tobytes()
    assert a.tail == b.tail
    for k in KEYS:
        assert a.grads[k].tobytes() == b.grads[k].tobytes(), k
