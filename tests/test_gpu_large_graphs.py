"""GPU tests of the large-graph path (gmc_large_*: the row-parallel head of csrc/large.hip, graphs of up to 2^20 nodes)
against the float64 restatement of tests/kway_ref.py: one poisoned training step per case of large_ref.CASES through the
entry point itself (the tile edges, past the old limits, a hub on the wave-per-row path, K in {2, 3, 4, 8}, both losses,
unit and real-valued weights, 70,000 and 2^20 nodes), the same inputs through gmc_kway_* where both run, determinism and
composition, the existing steps around a large call, the trainer against a float64 Adam replay, train_model -> checkpoint ->
load_neural_model -> evaluate_model on datasets without the dense adjacency, and the documented refusals.

Bars: stepcheck's (P_TOL for the probabilities, ORACLE_BAR / ROW_TOL / ROW_FLOOR for the gradient).  S must be the
reference's everywhere for the cases of at most 10,000 rows; the two cases above 65,535 nodes may differ on at most 8 rows
whose float64 margin is below 1e-6 (tests/test_large_graphs_host.py asserts the preconditions).  The hard loss of a
unit-weight graph is exactly -C * cut; the others are within 5e-5 * C * (total edge weight).

Measured on the MI355X (the tests print each figure with -s): see DESIGN.md section 19."""
import ctypes as C

import networkx as nx
import numpy as np
import pytest
import torch

from tests import kway_ref as KR
from tests import large_ref as LR
from tests import stepcheck, util
from tests.stepcheck import KEYS, ORACLE_BAR, P_TOL, ROW_FLOOR, ROW_TOL
from tests.test_gpu_kway import wave_sum32

pytestmark = pytest.mark.gpu
LOSS_BAR = 5e-5
CC = LR.CC
FWD_TAGS = ["gather_w1", "agg_fwd", "dense_mfma"]
BWD_TAGS = ["hidden_bwd", "colsum", "agg_bwd", "dw1"]
# gmc_large_*: each F-wide aggregation is followed by the launch that sums the rows of more than 64 entries again, in
# chunks (same tag), and the head is four launches (three without the backward)
LARGE_FWD = ["gather_w1"] * 2 + ["agg_fwd"] * 2 + ["dense_mfma"]
LARGE_BWD = ["hidden_bwd", "colsum"] + ["agg_bwd"] * 2 + ["dw1"]


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


def library_step(pkg, eng, batch, Cc, loss, entry="gmc_large_train_fwd_bwd"):
    """One call of a gmc_large_* / gmc_kway_* entry point itself under the probe, every buffer poisoned first."""
    lib, p = pkg.hip.load(), pkg.hip.ptr
    train = "train" in entry
    model = eng._call_model(loss=loss)
    size = getattr(lib, entry[:entry.index("_", 4)] + "_workspace_bytes")      # gmc_large_ / gmc_kway_workspace_bytes
    need = int(size(batch.ref(), C.byref(model), int(train)))
    assert need > 0
    ws = torch.full((need,), 255, dtype=torch.uint8, device="cuda")
    P = torch.full((batch.R, eng.K), float("nan"), device="cuda")
    S = torch.full((batch.R,), -1, dtype=torch.int32, device="cuda")
    losses = torch.full((batch.B,), float("nan"), device="cuda")
    eng.grad.fill_(float("nan"))
    with pkg.hip.Probe(64) as probe:
        args = (batch.ref(), C.byref(model), Cc, p(ws), need, p(P), p(S), p(losses))
        rc = getattr(lib, entry)(*args, *((p(eng.grad),) if train else ()), pkg.hip.stream())
        pkg.hip.check(rc, entry)
    grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()} if train else None
    return stepcheck.Step(P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads,
                          float(eng.grad[eng.count]) if train else None, [t for t, _ms in probe.records], list(probe.flavours))


def engine_step(pkg, eng, batch, Cc, loss):
    util.poison(eng, batch)
    with pkg.hip.Probe(64) as probe:
        P, S, losses = eng.train_fwd_bwd(batch, Cc, loss=loss)
        grads = {k: v.cpu().numpy() for k, v in eng.views(eng.grad).items()}
    return stepcheck.Step(P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads, float(eng.grad[eng.count]),
                          [t for t, _ms in probe.records], list(probe.flavours))


def same_bytes(a, b, grads=True):
    assert a.P.tobytes() == b.P.tobytes() and a.S.tobytes() == b.S.tobytes() and a.loss.tobytes() == b.loss.tobytes()
    if grads:
        assert a.tail == b.tail
        for k in KEYS:
            assert a.grads[k].tobytes() == b.grads[k].tobytes(), k


def grad_rules(csrs, params):
    return dict(grad_bar=ORACLE_BAR, row_tol=ROW_TOL, row_floor=ROW_FLOOR, kinks=(1e-7, 3), csrs=csrs, params=params,
                sparse=True)


def judge(got, ref, csrs, params, Cc, exact_loss, what, max_ties=0):
    """A Step against the float64 Ref: P, S (the reference's decode; `max_ties`: but for that many rows within LR.TIE of
    a tie), the losses, the tail, the gradient."""
    K = params["conv2.weight"].shape[1]
    assert got.P.shape == ref.P.shape and got.P.shape[1] == K, what
    p_err = float(np.abs(got.P - ref.P).max())
    print(f"{what}: P {p_err:.2e}")
    assert np.isfinite(got.P).all() and p_err < P_TOL, (what, p_err)
    off, worst, ties = 0, 0.0, 0
    for g, (rp, _cl, _vl) in enumerate(csrs):
        n = len(rp) - 1
        if max_ties:
            ties += KR.near_tie_rows(ref.P[off:off + n], got.S[off:off + n], LR.TIE, (what, g))
            assert np.array_equal(got.S[off:off + min(K, n)], np.arange(min(K, n)))
        else:
            assert np.array_equal(got.S[off:off + n], KR.partition(ref.P[off:off + n], K)), (what, g)
        bar = LOSS_BAR * Cc * KR.total_weight([csrs[g]])
        err = abs(float(got.loss[g]) - ref.loss[g])
        print(f"{what} graph {g}: loss {got.loss[g]:.6f} float64 {ref.loss[g]:.6f} err {err:.2e} bar {bar:.2e}")
        if exact_loss:   # unit weights: the cut is an integer, the loss its one float32 product with -C
            cut = round(-ref.loss[g] / Cc)
            assert abs(-ref.loss[g] / Cc - cut) < 1e-6 and got.loss[g] == -(np.float32(Cc) * np.float32(cut)), \
                (what, g, got.loss[g], ref.loss[g])
        assert err <= bar, (what, g, got.loss[g], ref.loss[g])
        worst = max(worst, err)
        off += n
    assert ties <= max_ties, (what, ties)
    if got.grads is None:
        return None
    assert got.loss.dtype == np.float32 and got.tail == float(wave_sum32(got.loss)), (what, got.tail)
    res = stepcheck.compare_grads(got.grads, ref.grads, what=what, **grad_rules(csrs, params))
    assert not res["bad_cols"], (what, res)
    print(f"{what}: P {p_err:.2e} rows {res['rows']:.2e} loss {worst:.2e} ties {ties}")
    return res


# ---- every case of the list: one whole step of gmc_large_train_fwd_bwd against float64
@pytest.mark.parametrize("case", LR.CASES, ids=LR.case_id)
def test_step_against_float64(pkg, case):
    csrs, params = LR.case_csrs(case), LR.case_params(case)
    eng = engine_with(pkg, params)
    batch = pkg.GraphBatch(LR.case_handles(pkg, case), None, eng.device)
    assert (batch.host.vals is not None) == (case.weights == "real")
    got = library_step(pkg, eng, batch, CC, case.loss)
    assert got.tags == LARGE_FWD + ["head"] * 4 + LARGE_BWD, got.tags
    assert not any(got.flavours)
    big = LR.is_big(case)
    ref = LR.reference(case, S_got=got.S if big else None)
    what = LR.case_id(case)
    judge(got, ref, csrs, params, CC, case.loss == "cut" and case.weights == "unit", what, LR.MAX_TIES if big else 0)
    assert not got.grads["conv1.weight"][batch.n_max:].any()                   # rows past every graph's n: exactly 0
    # a second step gives the same bytes; the forward alone reports the same P, S and loss
    same_bytes(library_step(pkg, eng, batch, CC, case.loss), got)
    fwd = library_step(pkg, eng, batch, CC, case.loss, "gmc_large_forward")
    assert fwd.tags == LARGE_FWD + ["head"] * 3, fwd.tags
    same_bytes(fwd, got, grads=False)
    # the engine takes a batch its ordinary sequence refuses to these entry points, and no other
    need = case.shape in ("n4097", "n5000", "k8n2500", "star4200", "hubring4200") or big
    assert eng.needs_large(batch, case.loss) == need
    via = engine_step(pkg, eng, batch, CC, case.loss)
    if need:
        assert via.tags == got.tags
        same_bytes(via, got)
        Pf, Sf, lf = (t.cpu().numpy() for t in eng.forward(batch, CC, want_loss=True, loss=case.loss))
        assert Pf.tobytes() == got.P.tobytes() and Sf.tobytes() == got.S.tobytes() and lf.tobytes() == got.loss.tobytes()
    else:
        assert via.tags.count("head") <= 1, via.tags


# ---- against gmc_kway_* on the same inputs
@pytest.mark.parametrize("case", LR.COMPARE, ids=LR.case_id)
def test_large_head_against_the_one_workgroup_head(pkg, case):
    csrs, params = LR.case_csrs(case), LR.case_params(case)
    eng = engine_with(pkg, params)
    batch = pkg.GraphBatch(LR.case_handles(pkg, case), None, eng.device)
    large = library_step(pkg, eng, batch, CC, case.loss)
    kway = library_step(pkg, eng, batch, CC, case.loss, "gmc_kway_train_fwd_bwd")
    assert kway.tags == FWD_TAGS + ["head"] + BWD_TAGS and large.tags == LARGE_FWD + ["head"] * 4 + LARGE_BWD
    assert np.array_equal(large.S, kway.S)
    ref = LR.reference(case)
    exact = case.loss == "cut" and case.weights == "unit"
    for name, got in (("large", large), ("kway", kway)):                       # each within one bar of the same reference
        judge(got, ref, csrs, params, CC, exact, f"{LR.case_id(case)} {name}")
    if exact:
        assert large.loss.tobytes() == kway.loss.tobytes()
    assert float(np.abs(large.P - kway.P).max()) < 2 * P_TOL
    stepcheck.compare_grads(large.grads, kway.grads, grad_bar=2 * ORACLE_BAR, row_tol=2 * ROW_TOL, row_floor=ROW_FLOOR,
                            what=LR.case_id(case))


# ---- composition: a graph alone and inside a batch
@pytest.mark.parametrize("case", [c for c in LR.CASES if c.shape == "batch"], ids=LR.case_id)
def test_a_graph_computes_the_same_alone_and_inside_a_batch(pkg, case):
    params = LR.case_params(case)
    eng = engine_with(pkg, params)
    handles = LR.case_handles(pkg, case)
    batch = pkg.GraphBatch(handles, None, eng.device)
    whole = library_step(pkg, eng, batch, CC, case.loss, "gmc_large_forward")
    for g, h in enumerate(handles):
        alone = library_step(pkg, eng, pkg.GraphBatch([h], None, eng.device), CC, case.loss, "gmc_large_forward")
        lo, hi = int(batch.goff_host[g]), int(batch.goff_host[g + 1])
        assert alone.P.tobytes() == whole.P[lo:hi].tobytes() and alone.S.tobytes() == whole.S[lo:hi].tobytes(), g
        assert alone.loss.tobytes() == whole.loss[g:g + 1].tobytes(), g


# ---- the existing steps are what they were, around a large call
def test_existing_steps_are_unchanged_by_a_large_call(pkg):
    ds = util.product_dataset([(60, 7, 61), (48, 6, 62)])
    kcase = KR.CASES[8]
    outs = []
    for between in (False, True):
        T, cfg, net, embed, opt, params = util.model(32, seed=5)
        eng = net.engine()
        batch = util.batch_of(pkg, eng, ds)
        keng = engine_with(pkg, KR.case_params(kcase))
        kbatch = pkg.GraphBatch([pkg.from_networkx(g) for g in KR.case_graphs(kcase)], None, keng.device)
        if between:
            case = next(c for c in LR.CASES if c.shape == "n4097")
            leng = engine_with(pkg, LR.case_params(case))
            got = engine_step(pkg, leng, pkg.GraphBatch(LR.case_handles(pkg, case), None, leng.device), CC, case.loss)
            assert got.tags.count("head") == 4
        outs.append((stepcheck.run_step(pkg, eng, batch, 1.0), engine_step(pkg, keng, kbatch, CC, kcase.loss)))
    (a3, ak), (b3, bk) = outs
    assert "fwd1_fused" in a3.tags and ak.tags.count("head") == 1
    for a, b in ((a3, b3), (ak, bk)):
        assert a.tags == b.tags and a.flavours == b.flavours
        same_bytes(a, b)


# ---- the trainer's eager sequence against a float64 Adam replay
def dataset_of(pkg, sizes, K, N, adjacency="none", seed=0):
    """A dataset through process_graphs_from_folder: circulants with chords as networkx graphs, K terminals."""
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    graphs = {}
    for i, n in enumerate(sizes):
        _n, rp, col = LR.circulant(n, 7, seed + i)
        rows = np.repeat(np.arange(n), np.diff(rp))
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from(zip(rows[rows < col].tolist(), col[rows < col].tolist()), weight=1)
        graphs[i] = g
    terms = {i: [10 * (j + 1) for j in range(K)] for i in graphs}              # (moved onto 0..K-1 by the call)
    ds = GE.process_graphs_from_folder(graphs, terms, N, number_classes=K, adjacency=adjacency)
    assert len(ds) == len(sizes)
    return ds


@pytest.mark.parametrize("K", (3, 4))
def test_trainer_epochs_against_a_float64_adam_replay(pkg, K):
    """Three epochs of FusedTrainer.epoch on one graph of 4100 nodes (one step per epoch): the returned loss is the graph's
    loss, and after every step the moments and the parameter update are those of a float64 Adam step from the device's
    state before it, with the gradient of the partition the device chose (the bars of test_gpu_kway.py's replay: m 1e-4,
    v 2e-4 of the largest, update within 2 % where the gradient is at least 1 % of the largest).  One term more than
    there: the update is m^ / (sqrt(v^) + eps), so it cannot be held tighter than the first moment it is made from -
    each entry is allowed, on top of the 2 %, what an error of 1e-4 * max|m| (the moment's own bar) does to it.  With
    32,800 entries of conv1.weight instead of 2,048 the moment of some judged entry cancels to 1e-7 of the largest by the
    third step (0.9 m + 0.1 g with g of the other sign; a float64 replay on the CPU shows it), where float32 keeps no
    digit of it: measured without the term, 2.6 % on one entry at K = 3, step 3."""
    from gcn_max_cut_amd.Training import TrainingNeural as T
    N, F = 4100, 8
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=F, number_classes=K, learning_rate=1e-3)
    torch.manual_seed(K)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    ds = dataset_of(pkg, [4100], K, N)
    assert ds[0][1] is None
    csrs = [KR.csr_of_handle(ds[0][0])]
    tr = T.FusedTrainer(net, opt, cfg, graphs_per_step=1)
    eng = tr.eng
    assert eng.kway == (K != 3) and eng.K == K
    net.train()
    b1, b2, eps, lr = 0.9, 0.999, 1e-8, cfg.learning_rate
    for t in range(1, 4):
        before = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views().items()}
        m0 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.m).items()}
        v0 = {k: v.cpu().numpy().astype(np.float64) for k, v in eng.views(eng.v).items()}
        with pkg.hip.Probe(64) as probe:
            total = tr.epoch(ds)
        tags = [t_ for t_, _ms in probe.records]
        assert tr._large and tags.count("head") == 4 and "fwd1_fused" not in tags, tags
        assert eng.step_count == t
        per_graph = tr._loss_slots[0, :1].cpu().numpy()
        assert total == float(per_graph.sum(dtype=np.float32)), (t, total, per_graph)
        S = tr._out[1][:4100].cpu().numpy()
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
            # what the first moment's own bar leaves of the update: d upd = lr / (1 - b1^t) * dm / (sqrt(v^) + eps)
            slack = lr / (1 - b1 ** t) * 1e-4 * np.abs(m1).max() / (np.sqrt(v1) / np.sqrt(1 - b2 ** t) + eps)
            excess = (np.abs(got_upd - upd) - slack)[big] / np.abs(upd[big])
            print(f"K={K} step {t} {k}: update error beyond the moment's bar {excess.max():.2e} of the update (bar 0.02)")
            assert big.any() and excess.max() < 0.02, (t, k, excess.max())


# ---- train_model on a dataset without the dense adjacency, its checkpoint, evaluate_model
def numpy_cut(handle, part):
    rows = np.repeat(np.arange(handle.n), np.diff(handle.rowptr))
    part = np.asarray(part)
    return int((part[rows] != part[handle.col]).sum()) // 2


@pytest.mark.parametrize("loss", ("cut", "expected_cut"))
def test_train_model_checkpoint_and_evaluation_without_the_dense_adjacency(pkg, tmp_path, monkeypatch, loss):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    monkeypatch.chdir(tmp_path)
    N, F = 4500, 8
    ds = dataset_of(pkg, [4500, 300], 3, N, seed=40)
    assert all(it[1] is None for it in ds.values())
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=F, number_epochs=2, learning_rate=1e-2, save_directory="large.pth",
                           save_frequency=1000)
    torch.manual_seed(3)
    net, best, epoch, _w, history = T.train_model(ds, cfg, loss=loss)
    assert epoch == 1 and len(history) == 2 and best == min(history) and all(np.isfinite(history))
    assert net._fused_trainer._large and net.engine().step_count == 4          # one step per graph, the small one included
    loaded, _inputs, saved_cfg = T.load_neural_model(str(tmp_path / "final_large.pth"), cfg)
    assert saved_cfg.n_nodes == N
    sd = loaded.state_dict()
    for k, v in net.state_dict().items():
        assert torch.equal(v.cpu(), sd[k].cpu()), k
    ev = T.evaluate_model(loaded, ds, cfg)
    cuts = []
    for handle, none, _nx_g, _t in ds.values():
        with torch.no_grad():
            P = loaded(handle, none)
        assert tuple(P.shape) == (handle.n, 3)
        part = TN.simple_partition_assignment(P)
        assert part[:3] == [0, 1, 2]
        cuts.append(numpy_cut(handle, part))
    assert ev["num_samples"] == 2 and ev["total_loss"] == -float(sum(cuts)) and sum(cuts) > 0
    soft = T.evaluate_model(loaded, ds, cfg, loss="expected_cut")
    assert np.isfinite(soft["total_loss"]) and soft["total_loss"] != ev["total_loss"]
    assert history[0] < 0


# ---- what a large graph refuses
def test_refusals_for_a_large_graph(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    N = 4200
    cfg = T.TrainingConfig(n_nodes=N, hidden_dim=8)
    net, embed, opt = T.setup_model_and_optimizer(cfg)
    ds = dataset_of(pkg, [4200], 3, N, seed=50)
    (g, none, nx_g, terms), = ds.values()
    net.eval()
    with torch.no_grad():
        P = net(g, none)
    assert tuple(P.shape) == (4200, 3) and bool(torch.isfinite(P).all())
    for call in (lambda: TN.decode_dataset(net, ds, 4), lambda: TN.decode_dataset(net, ds, 4, local_search_sweeps=2),
                 lambda: TN.decode_dataset(net, ds, 4, anneal_sweeps=2), lambda: TN.round_dataset(net, ds),
                 lambda: TN.search_dataset(net, ds, 4), lambda: TN.test_single_graph(net, g, none, nx_g, terms, 4),
                 lambda: TN.test_multiple_graphs(net, ds, [4200], 4, verbose=False), lambda: T.cut_loss(g, P)):
        with pytest.raises(ValueError, match="4096 nodes.*argmax partition"):
            call()
    eng = net.engine()
    batch = pkg.GraphBatch([g], None, eng.device)
    assert eng.needs_large(batch)
    X = torch.zeros(4200, N)
    for call in (lambda: eng.train_step(batch, 1e-3), lambda: eng.backward_from_gp(batch, P, P),
                 lambda: eng.train_fwd_bwd(batch, slab=True), lambda: eng.workspace_bytes_features(batch, True),
                 lambda: eng.forward_features(batch, X)):
        with pytest.raises(NotImplementedError, match="4200 nodes"):
            call()
    with eng.dropout(0.5, 1):
        for call in (lambda: eng.forward(batch), lambda: eng.train_fwd_bwd(batch), lambda: eng.workspace_bytes(batch, True)):
            with pytest.raises(NotImplementedError, match="dropout.*4200 nodes"):
                call()
    drop_cfg = T.TrainingConfig(n_nodes=N, hidden_dim=8, dropout=0.25)
    dnet, dembed, dopt = T.setup_model_and_optimizer(drop_cfg)
    with pytest.raises(NotImplementedError, match="dropout.*4200 nodes"):
        T.train_single_epoch(ds, dnet, dopt, dembed, drop_cfg)
    net.train()
    with pytest.raises(NotImplementedError, match="autograd.*4200 nodes"):
        net(g, none)
    att = pkg.engine.FusedEngine(N, 8, 3, attention=True)
    for call in (lambda: att.forward(batch), lambda: att.train_fwd_bwd(batch)):
        with pytest.raises(NotImplementedError, match="attention.*4200 nodes"):
            call()
    keng = pkg.engine.FusedEngine(2600, 8, 8, kway=True)                       # K = 8: the one-workgroup head stops near 2400
    kbatch = pkg.GraphBatch([pkg.GraphHandle(*LR.circulant(2500, 7, 1))], None, keng.device)
    assert keng.needs_large(kbatch) and keng.forward(kbatch)[0].shape == (2500, 8)
    wide = T.TrainingConfig(n_nodes=20000)                                     # hidden_dim = n_nodes // 2 = 10000
    with pytest.raises(ValueError, match="explicit hidden_dim"):
        pkg.engine.FusedEngine(wide.dim_embedding, wide.hidden_dim, 3)
