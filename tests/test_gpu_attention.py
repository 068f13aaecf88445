"""GPU tests of the graph-attention first layer (gmc_att_*, csrc/attention.hip, FusedEngine(N, F, 3, attention=True),
GATSoftmax) against the float64 restatement of tests/attention_ref.py: one poisoned training step per case of
attention_ref.CASES (n = 3 and 4, a node of degree 0, hub rows of 71 and 141 terms, a self-loop, n = 65 and 1030, a batch
of three graphs, d = 12, hidden 4 / 12 / 260 / 516, unit and real-valued weights, both losses), zero attention vectors
against the mean aggregation, the trainer's eager sequence against a float64 Adam replay over six tensors,
train_model(layer1="attention") with its checkpoint, evaluate_model and the decoders, the documented refusals, and the
graphconv step around an attention call.

Bars: stepcheck's - P_TOL for the probabilities (for the two stars alone, where a float32 torch evaluation of the same
formulas is itself further than P_TOL / 4 from float64: four times its error, never above PROB_TOL: `probability_bar`), ORACLE_BAR / ROW_TOL /
ROW_FLOOR for the gradient, da_src and da_dst judged as parameter rows.  S must be the reference's everywhere: tests/test_attention_host.py asserts on the float64
reference that no case has a row within 1e-5 of a tie, a unit within 1e-6 of the relu kink or a score within 1e-6 of the
leaky relu's.  The hard loss of a unit-weight graph is exactly -C * cut; weighted and relaxed losses are within
5e-5 * C * (total edge weight).

Measured on the MI355X (the tests print each figure with -s), worst over the 30 cases: P 2.3e-7 at the P_TOL bar, 1.3e-6 and
3.9e-6 at the two stars (float32 torch: 1.3e-6 and 2.9e-6; bars 5.3e-6 and 1.2e-5); gradient row ratio 7.8e-5, 1.35e-4 on
da_src / da_dst (hidden 516; bar 2e-4); weighted / relaxed loss 3.8e-4 absolute on a loss near -7,000 (bar 0.3)."""
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import attention_ref as AR
from tests import kway_ref as KR
from tests import stepcheck, util
from tests.stepcheck import KEYS, ORACLE_BAR, P_TOL, PROB_TOL, ROW_FLOOR, ROW_TOL

pytestmark = pytest.mark.gpu
LOSS_BAR = 5e-5
CC = 1.3
STEP_TAGS = ["gather_w1", "dense_mfma", "agg_fwd", "dense_mfma", "head", "hidden_bwd", "hidden_bwd", "colsum", "agg_bwd",
             "agg_bwd", "colsum", "colsum", "dw1"]


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def engine_with(pkg, params):
    N, F = params["conv1.weight"].shape
    eng = pkg.engine.FusedEngine(N, F, 3, attention=True)
    for k, v in eng.views().items():
        v.copy_(torch.from_numpy(params[k]))
    return eng


def batch_for(pkg, eng, handles):
    return pkg.GraphBatch(handles, None, eng.device, allow_zero_degree=True)


def run_step(pkg, eng, batch, Cc, loss):
    """One poisoned train_fwd_bwd under the probe (stepcheck.run_step with the loss keyword)."""
    util.poison(eng, batch)
    with pkg.hip.Probe(64) as probe:
        P, S, losses = eng.train_fwd_bwd(batch, Cc, loss=loss)
        grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}
    return stepcheck.Step(P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads, float(eng.grad[eng.count]),
                          [t for t, _ms in probe.records], list(probe.flavours))


def wave_sum32(values):
    """The sum the library puts behind the gradient (loss_tail_kernel): float32, the values dealt over 64 lanes, then the
    butterfly of gmc::wave_sum (lane distances 32, 16, .., 1) - lane 0's total."""
    lanes = np.zeros(64, np.float32)
    for b, v in enumerate(np.asarray(values, np.float32)):
        lanes[b % 64] = np.float32(lanes[b % 64] + v)
    idx = np.arange(64)
    for dist in (32, 16, 8, 4, 2, 1):
        lanes = (lanes + lanes[idx ^ dist]).astype(np.float32)
    return lanes[0]


# the shapes whose probabilities float32 cannot give to P_TOL: a star's hub row sums over all of its leaves
HUB_SHAPES = ("star70", "star140")


def probability_bar(shape, csrs, params, Cc, loss, ref):
    """P_TOL.  For the shapes of HUB_SHAPES alone, where a float32 torch evaluation of the same formulas
    (attention_ref.float32_yardstick, on the CPU) is itself further than a quarter of P_TOL from float64: four times
    that evaluation's error (the summation orders differ), never above PROB_TOL.  Every other case stays at P_TOL whatever
    torch's figure is."""
    p32, _rows = AR.float32_yardstick(csrs, params, Cc, loss, ref)
    return (min(max(P_TOL, 4 * p32), PROB_TOL) if shape in HUB_SHAPES else P_TOL), p32


def judge(got, ref, csrs, params, Cc, loss, exact_loss, what, shape):
    """A Step against the float64 Ref: P, S identical to the reference's decode, the losses, the tail, the six gradients."""
    assert got.P.shape == ref.P.shape and got.P.shape[1] == 3, what
    p_err = float(np.abs(got.P - ref.P).max())
    p_bar, p32 = probability_bar(shape, csrs, params, Cc, loss, ref)
    print(f"{what}: P {p_err:.2e} (bar {p_bar:.1e}, float32 torch {p32:.1e})")
    assert np.isfinite(got.P).all() and p_err < p_bar, (what, p_err, p_bar)
    off, worst = 0, 0.0
    for g, (rp, _cl, _vl) in enumerate(csrs):
        n = len(rp) - 1
        assert np.array_equal(got.S[off:off + n], KR.partition(ref.P[off:off + n], 3)), (what, g)
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
    for k in AR.ATT_KEYS:
        r = np.asarray(ref.grads[k], np.float64)
        e = np.abs(np.asarray(got.grads[k], np.float64).reshape(r.shape) - r)
        print(f"{what} {k}: max err {e.max():.2e} of max {np.abs(r).max():.2e}")
    res = stepcheck.compare_grads(got.grads, ref.grads, what=what, grad_bar=ORACLE_BAR, row_tol=ROW_TOL,
                                  row_floor=ROW_FLOOR)
    vec = AR.vector_rows(got.grads, ref.grads, ORACLE_BAR, ROW_TOL, ROW_FLOOR, what)
    print(f"{what}: P {p_err:.2e} rows {res['rows']:.2e} attention rows {vec:.2e} loss {worst:.2e}")
    return res


# ---- every case of the list: one whole step against float64
@pytest.mark.parametrize("case", AR.CASES, ids=AR.case_id)
def test_step_against_float64(pkg, case):
    handles = [pkg.from_networkx(g) for g in AR.case_graphs(case)]
    csrs = [KR.csr_of_handle(h) for h in handles]
    params = AR.case_params(case)
    eng = engine_with(pkg, params)
    batch = batch_for(pkg, eng, handles)
    assert (batch.host.vals is not None) == (case.weights == "real")
    got = run_step(pkg, eng, batch, CC, case.loss)
    assert got.tags == STEP_TAGS, got.tags
    assert not any(got.flavours)                                 # row kernels only: no LDS-tiled launch
    ref, _gaps = AR.f64_step(csrs, params, CC, case.loss)
    what = AR.case_id(case)
    judge(got, ref, csrs, params, CC, case.loss, case.loss == "cut" and case.weights == "unit", what, case.shape)
    assert not got.grads["conv1.weight"][batch.n_max:].any()     # rows past every graph's n: exactly 0
    # a second step gives the same bytes; the forward alone reports the same P, S and loss
    again = run_step(pkg, eng, batch, CC, case.loss)
    assert again.P.tobytes() == got.P.tobytes() and again.loss.tobytes() == got.loss.tobytes() and again.tail == got.tail
    for k in AR.ATT_KEYS:
        assert again.grads[k].tobytes() == got.grads[k].tobytes(), k
    Pf, Sf, lf = (t.cpu().numpy() for t in eng.forward(batch, CC, want_loss=True, loss=case.loss))
    assert np.array_equal(Pf, got.P) and np.array_equal(Sf, got.S) and np.array_equal(lf, got.loss), what


# ---- zero attention vectors: every term of a row weighs the same
@pytest.mark.parametrize("shape", ("batch3", "star70", "deg0"))
def test_zero_attention_vectors_give_the_mean_aggregation(pkg, shape):
    case = AR.Case(shape, "real", "cut", 0)
    handles = [pkg.from_networkx(g) for g in AR.case_graphs(case)]
    params = AR.case_params(case)
    params["conv1.attn_src"][:] = 0
    params["conv1.attn_dst"][:] = 0
    eng = engine_with(pkg, params)
    P = eng.forward(batch_for(pkg, eng, handles))[0].cpu().numpy()
    W1, b1, W2, b2 = (params[k].astype(np.float64) for k in KEYS)
    want = []
    for h in handles:
        rp, cl, vl = KR.csr_of_handle(h)
        T = stepcheck.csr_mm(rp, cl, None if vl is None else vl.astype(np.float64), W1[:h.n])
        deg = np.diff(rp).astype(np.float64)
        Hm = np.maximum((stepcheck.csr_mm(rp, cl, None, T) + T) / (deg + 1)[:, None] + b1, 0.0)   # mean over N(i) + {i}
        dinv = 1.0 / np.sqrt(np.maximum(deg, 1))
        Z = dinv[:, None] * stepcheck.csr_mm(rp, cl, None, dinv[:, None] * Hm @ W2) + b2
        E = np.exp(Z - Z.max(1, keepdims=True))
        want.append(E / E.sum(1, keepdims=True))
    want = np.concatenate(want)
    err = float(np.abs(P - want).max())
    # the bar of `probability_bar` (HUB_SHAPES only): float32 torch is 7.3e-7 from float64 at the 70-leaf star's hub
    p32 = float(np.abs(AR.dense_step([KR.csr_of_handle(h) for h in handles], params, 1.0, "cut", torch.float32)[0] - want).max())
    bar = min(max(P_TOL, 4 * p32), PROB_TOL) if shape in HUB_SHAPES else P_TOL
    print(f"mean aggregation {shape}: P {err:.2e} (bar {bar:.1e}, float32 torch {p32:.1e})")
    assert err < bar, (err, bar)


# ---- the trainer's eager sequence against a float64 Adam replay over six tensors
def dataset_for(specs, N):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: R.seeded_terminals(n, s) for i, (n, d, s) in enumerate(specs)}
    ds = GE.process_graphs_from_folder(graphs, terms, N)
    assert len(ds) == len(specs)
    return ds


def test_trainer_epochs_against_a_float64_adam_replay(pkg):
    """Three epochs of FusedTrainer.epoch on two graphs (one step per epoch): the returned loss is the sum of the per-graph
    losses, and after every step the moments and the parameter update of all SIX tensors are those of a float64 Adam step
    from the device's state before it (the bars of tests/test_gpu_kway.py's replay: m 1e-4, v 2e-4 of the largest, update
    within 2 % where the gradient is at least 1 % of the largest)."""
    from gcn_max_cut_amd.Training import TrainingNeural as T
    N, F = 128, 16
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=F, learning_rate=1e-3)
    torch.manual_seed(11)
    net, embed, opt = T.setup_model_and_optimizer(cfg, layer1="attention")
    assert isinstance(net, T.GATSoftmax) and list(net.state_dict()) == [
        "conv1.weight", "conv1.bias", "conv1.attn_src", "conv1.attn_dst", "conv2.weight", "conv2.bias"]
    ds = dataset_for([(60, 7, 31), (48, 6, 32)], N)
    csrs = util.csrs_of(ds)
    tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=2)
    eng = tr.eng
    assert eng.attention and not eng.kway and eng.count == N * F + F + 3 * F + 3 + 2 * F
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
        params32 = {k: before[k].astype(np.float32) for k in AR.ATT_KEYS}
        ref, _gaps = AR.f64_step(csrs, params32, cfg.C, "cut")
        S = tr._out[1][:sum(len(c[0]) - 1 for c in csrs)].cpu().numpy()
        assert np.array_equal(S, np.concatenate([KR.partition(p, 3) for p in np.split(ref.P, [len(csrs[0][0]) - 1])]))
        assert np.array_equal(per_graph, ref.loss.astype(np.float32)), (t, per_graph, ref.loss)   # -cut: exact
        for k in AR.ATT_KEYS:
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
    tr.sync_optimizer_state()
    named = dict(net.named_parameters())
    assert len(named) == 6 and all(opt.state[p]["step"].item() == 3.0 for p in named.values())


# ---- train_model(layer1="attention"), its checkpoint, evaluate_model and the decoders
@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
def test_train_model_checkpoint_evaluation_and_decoders(pkg, tmp_path, monkeypatch, loss):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.chdir(tmp_path)
    N, F = 64, 8
    ds = dataset_for([(40, 5, 41), (30, 4, 42)], N)
    torch.manual_seed(3)
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=F, number_epochs=2, learning_rate=1e-2, save_directory="gat.pth")
    net, best, epoch, _w, history = T.train_model(ds, cfg, loss=loss, layer1="attention")
    assert isinstance(net, T.GATSoftmax) and epoch == 1 and len(history) == 2 and best == min(history)
    assert all(np.isfinite(history))
    plain = T.TrainingConfig(n_nodes=N, hidden_dim=F)
    loaded, _inputs, _cfg = T.load_neural_model(str(tmp_path / "final_gat.pth"), plain)   # (not told: the keys say so)
    assert isinstance(loaded, T.GATSoftmax)
    sd = loaded.state_dict()
    assert set(sd) == set(AR.ATT_KEYS) and tuple(sd["conv1.attn_src"].shape) == (F,)
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    ev = T.evaluate_model(loaded, ds, plain)
    cuts = []
    for handle, a_pad, nx_g, _t in ds.values():
        with torch.no_grad():
            P = loaded(handle, a_pad)
        assert tuple(P.shape) == (handle.n, 3)
        part = TN.simple_partition_assignment(P)
        assert part[:3] == [0, 1, 2]
        cuts.append(sum(d.get("weight", 1) for u, v, d in nx_g.edges(data=True) if part[u] != part[v]))
        res = TN.test_single_graph(loaded, handle, a_pad, nx_g, [0, 1, 2], post_processing_iterations=4, seed=5)
        assert res["success"] and res["simple_cut"] == cuts[-1] and res["simple_assignment"] == part
    assert ev["num_samples"] == 2 and ev["total_loss"] == -float(sum(cuts))
    soft = T.evaluate_model(loaded, ds, plain, loss="expected_cut")
    assert np.isfinite(soft["total_loss"]) and soft["total_loss"] != ev["total_loss"]
    dec = TN.decode_dataset(loaded, ds, 8, local_search_sweeps=5, anneal_sweeps=5, sample_seed=7)
    rnd = TN.round_dataset(loaded, ds, descent_sweeps=3)
    for g, (d, r) in enumerate(zip(dec, rnd)):
        assert d["simple_cut"] == r["simple_cut"] == cuts[g]
        assert d["refined_cut"] >= d["simple_cut"] and d["annealed_cut"] >= d["simple_cut"] and d["post_cut"] >= 0
        assert r["rounded_cut"] >= 0 and np.isfinite(r["expected_cut"])


# ---- what the attention model refuses
def test_refusals_of_the_attention_model(pkg):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8)
    net, embed, opt = T.setup_model_and_optimizer(cfg, layer1="attention")
    ds = dataset_for([(40, 5, 51)], 64)
    (g, a_pad, _nx_g, _t), = ds.values()
    net.eval()
    with pytest.raises(NotImplementedError, match="layer1"):
        net(g, a_pad)                                            # with gradients
    with torch.no_grad():
        P = net(g, a_pad)
        with pytest.raises(NotImplementedError, match="layer1"):
            net(g, torch.rand(40, 64, device=a_pad.device))      # dense features
    assert tuple(P.shape) == (40, 3)
    eng = net.engine()
    batch = pkg.GraphBatch([g], None, eng.device)
    for call in (lambda: eng.train_step(batch, 1e-3), lambda: eng.ensure_slab(), lambda: eng.set_dropout(0.5),
                 lambda: eng.backward_from_gp(batch, P, P), lambda: eng.workspace_bytes_features(batch, True),
                 lambda: eng.forward_features(batch, torch.zeros(40, 64)),
                 lambda: eng.backward_features_from_gp(batch, torch.zeros(40, 64), P, P, None)):
        with pytest.raises(NotImplementedError, match="layer1"):
            call()
    drop_cfg = T.TrainingConfig(n_nodes=64, hidden_dim=8, dropout=0.25)
    dnet, dembed, dopt = T.setup_model_and_optimizer(drop_cfg, layer1="attention")
    with pytest.raises(NotImplementedError, match="layer1"):
        T.train_single_epoch(ds, dnet, dopt, dembed, drop_cfg)
    with pytest.raises(ValueError, match="layer1"):
        T.train_single_epoch(ds, net, opt, embed, cfg, layer1="graphconv")
    for K, kw in ((2, {}), (4, {}), (3, dict(kway=True))):
        with pytest.raises(ValueError, match="layer1"):
            pkg.engine.FusedEngine(64, 8, K, attention=True, **kw)
    with pytest.raises(ValueError, match="layer1"):
        T.setup_model_and_optimizer(T.TrainingConfig(n_nodes=64, hidden_dim=8, number_classes=2), layer1="attention")
    with pytest.raises(pkg.DGLError):                      # graphconv keeps refusing nodes without neighbours
        pkg.GraphBatch([pkg.from_networkx(AR.with_isolated_node(20, 3, 3))], None, eng.device)


# ---- the graphconv step is what it was, around an attention call
def test_graphconv_step_is_unchanged_by_an_attention_call(pkg):
    ds = util.product_dataset([(60, 7, 61), (48, 6, 62)])
    outs = []
    for between in (False, True):
        T, cfg, net, embed, opt, params = util.model(32, seed=5)
        eng = net.engine()
        batch = util.batch_of(pkg, eng, ds)
        if between:
            case = AR.CASES[8]
            handles = [pkg.from_networkx(g) for g in AR.case_graphs(case)]
            aeng = engine_with(pkg, AR.case_params(case))
            assert type(aeng) is type(eng) and aeng.attention and not eng.attention
            run_step(pkg, aeng, batch_for(pkg, aeng, handles), CC, case.loss)
        outs.append(stepcheck.run_step(pkg, eng, batch, 1.0))
    a, b = outs
    assert a.tags == b.tags and a.flavours == b.flavours
    assert a.P.tobytes() == b.P.tobytes() and a.S.tobytes() == b.S.tobytes() and a.loss.tobytes() == b.loss.tobytes()
    assert a.tail == b.tail
    for k in KEYS:
        assert a.grads[k].tobytes() == b.grads[k].tobytes(), k
