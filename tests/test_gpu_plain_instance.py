"""GPU tests of one model per graph WITHOUT terminals (gmc_inst_forward_t / gmc_inst_train_fwd_bwd_t with terminals = 0,
engine.InstanceEngine(terminals=False), solve_dataset(terminals=False)) and of the front door maxcut.solve.

The float64 step is plain_ref.inst_step: functional_ref's forward / backward (stepcheck's f64_forward_sparse /
f64_backward_sparse) around functional_ref.loss_and_gp(..., terminals=False).  Bars: stepcheck's P_TOL for the
probabilities, ORACLE_BAR and ROW_TOL / ROW_FLOOR for every gradient row (functional_ref.grad_ratios), and
LOSS_BAR = 5e-5 * C * total weight for weighted and relaxed losses, as tests/test_gpu_instance.py has them.  S must be
the reference's row argmax on EVERY row and the hard loss of a unit-weight graph exactly -C * cut(S):
tests/test_plain_maxcut_host.py asserts on the float64 reference that no case has a row within 1e-5 of a tie or a unit
within 1e-6 of the relu kink, and that a float32 numpy evaluation keeps half of ROW_TOL.

The cases are plain_ref.INST_CASES: the batches (3, K, K + 1, 65), (5, 300, 65, 257) and the star of 70 leaves whose
centre is node 2, K in {2, 3, 4, 8} (hidden 4, 12, 20, 36), unit and integer weights, both losses.  At K = 4 and 8 the
batches hold graphs of fewer than K nodes: what terminals = 1 refuses."""
import numpy as np
import pytest
import torch

from tests import functional_ref as FR
from tests import instance_ref as IR
from tests import kway_ref as KR
from tests import plain_ref as PR
from tests.stepcheck import KEYS, P_TOL

pytestmark = pytest.mark.gpu
LOSS_BAR = 5e-5
CC = PR.INST_C


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def handles_of(pkg, csrs):
    return [pkg.GraphHandle(len(rp) - 1, rp, cl, w) for rp, cl, w in csrs]


def engine_with(pkg, handles, params, terminals):
    F, K = params[0]["conv2.weight"].shape
    eng = pkg.engine.InstanceEngine(handles, F, K, terminals=terminals)
    for g, p in enumerate(params):
        for k, v in eng.views(g).items():
            v.copy_(torch.from_numpy(p[k]))
    return eng


def run_step(eng, Cc, loss):
    """One train_fwd_bwd with the scratch and the gradient poisoned: P, S, loss, the per-graph gradient dicts."""
    eng._workspace(True).fill_(255)
    eng.grad.fill_(float("nan"))
    P, S, losses = eng.train_fwd_bwd(Cc, loss=loss)
    grads = [{k: v.cpu().numpy() for k, v in eng.views(g, eng.grad).items()} for g in range(eng.B)]
    return P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads


def graph_bytes(eng, out, g):
    P, S, losses, grads = out
    r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
    return (P[r0:r1].tobytes(), S[r0:r1].tobytes(), losses[g:g + 1].tobytes()) + tuple(grads[g][k].tobytes() for k in KEYS)


@pytest.mark.parametrize("case", PR.INST_CASES, ids=PR.inst_case_id)
def test_step_without_terminals_against_float64(pkg, case):
    csrs = PR.inst_case_csrs(case)
    params = PR.inst_case_params(case, csrs)
    handles = handles_of(pkg, csrs)
    eng = engine_with(pkg, handles, params, terminals=False)
    assert (eng.batch.host.vals is not None) == (case.weights == "integer")
    out = run_step(eng, CC, case.loss)
    P, S, losses, grads = out
    what = PR.inst_case_id(case)
    assert np.isfinite(P).all() and losses.dtype == np.float32
    for g, (csr, p) in enumerate(zip(csrs, params)):
        f, value, ref = PR.inst_step(csr, p, CC, case.loss)
        r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
        p_err = float(np.abs(P[r0:r1] - f["P"]).max())
        assert p_err < P_TOL, (what, g, p_err)
        assert np.array_equal(S[r0:r1], f["P"].argmax(1)), (what, g)             # every row: none is overridden
        bar = LOSS_BAR * CC * KR.total_weight([csr])
        err = abs(float(losses[g]) - value)
        worst_abs, worst_row = FR.grad_ratios(grads[g], ref)
        print(f"{what} graph {g}: P {p_err:.2e} loss {losses[g]:.6f} float64 {value:.6f} err {err:.2e} bar {bar:.2e} "
              f"grad {worst_abs:.2e} of ORACLE_BAR, rows {worst_row:.2e} of ROW_TOL")
        assert err <= bar, (what, g, losses[g], value)
        assert worst_abs <= 1.0 and worst_row <= 1.0, (what, g, worst_abs, worst_row)
        if case.loss == "cut" and case.weights == "unit":
            cut = round(-value / CC)
            assert abs(-value / CC - cut) < 1e-9 and losses[g] == -(np.float32(CC) * np.float32(cut)), (what, g)
            Pg = torch.from_numpy(P[r0:r1]).cuda()
            fn = pkg.functional.cut_loss(handles[g], Pg, CC, relaxed=False, terminals=False)
            assert float(fn) == float(losses[g]), (what, g)
    # a second step gives the same bytes; the forward alone reports the same P, S and loss
    again = run_step(eng, CC, case.loss)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], again[:3]))
    assert [graph_bytes(eng, again, g) for g in range(eng.B)] == [graph_bytes(eng, out, g) for g in range(eng.B)]
    Pf, Sf, lf = (t.cpu().numpy() for t in eng.forward(CC, loss=case.loss))
    assert np.array_equal(Pf, P) and np.array_equal(Sf, S) and np.array_equal(lf, losses), what


@pytest.mark.parametrize("case", [PR.InstCase("mixed", 3, "integer", "cut", 1), PR.InstCase("mixed", 8, "unit", "expected_cut", 0)],
                         ids=PR.inst_case_id)
def test_without_terminals_a_graph_does_not_depend_on_its_batch(pkg, case):
    csrs = PR.inst_case_csrs(case)
    params = PR.inst_case_params(case, csrs)
    handles = handles_of(pkg, csrs)
    eng = engine_with(pkg, handles, params, terminals=False)
    whole = run_step(eng, CC, case.loss)
    for g in range(4):
        want = graph_bytes(eng, whole, g)
        a, b = [i for i in range(4) if i != g][:2]
        for order in ([g], [a, g, b], [a, b, g]):
            e = engine_with(pkg, [handles[i] for i in order], [params[i] for i in order], terminals=False)
            assert graph_bytes(e, run_step(e, CC, case.loss), order.index(g)) == want, (g, order)


@pytest.mark.parametrize("case", [IR.Case("mixed", 3, "real", "cut", 0), IR.Case("mixed", 8, "real", "expected_cut", 3),
                                  IR.Case("edge", 2, "unit", "expected_cut", 2)], ids=IR.case_id)
def test_with_terminals_the_twins_return_the_bytes_of_gmc_inst(pkg, case):
    """gmc_inst_forward_t / gmc_inst_train_fwd_bwd_t with terminals = 1 (what the engine calls) against gmc_inst_forward /
    gmc_inst_train_fwd_bwd called directly, both on poisoned buffers: every output byte, the whole flat gradient."""
    import ctypes as C
    hip = pkg.hip
    handles = [pkg.from_networkx(g) for g in IR.case_graphs(case)]
    eng = engine_with(pkg, handles, IR.case_params(case), terminals=True)
    P, S, losses, _grads = run_step(eng, CC, case.loss)
    grad = eng.grad[:eng.count].cpu().numpy()
    ws = eng._workspace(True)
    ws.fill_(255)
    P2 = torch.full_like(eng._outputs()[0], float("nan"))
    S2 = torch.full((eng.R,), -5, dtype=torch.int32, device=eng.device)
    l2 = torch.full((eng.B,), float("nan"), device=eng.device)
    g2 = torch.full_like(eng.grad, float("nan"))
    rc = eng.lib.gmc_inst_train_fwd_bwd(eng.batch.ref(), C.byref(eng._model(case.loss)), CC, hip.ptr(ws), ws.numel(),
                                        hip.ptr(P2), hip.ptr(S2), hip.ptr(l2), hip.ptr(g2), hip.stream())
    hip.check(rc, "gmc_inst_train_fwd_bwd")
    assert P2.cpu().numpy().tobytes() == P.tobytes() and S2.cpu().numpy().tobytes() == S.tobytes()
    assert l2.cpu().numpy().tobytes() == losses.tobytes() and g2[:eng.count].cpu().numpy().tobytes() == grad.tobytes()
    ws.fill_(255)
    P3, S3, l3 = torch.full_like(P2, float("nan")), torch.full_like(S2, -5), torch.full_like(l2, float("nan"))
    rc = eng.lib.gmc_inst_forward(eng.batch.ref(), C.byref(eng._model(case.loss)), CC, hip.ptr(ws), ws.numel(), hip.ptr(P3),
                                  hip.ptr(S3), hip.ptr(l3), hip.stream())
    hip.check(rc, "gmc_inst_forward")
    Pf, Sf, lf = eng.forward(CC, loss=case.loss)
    assert torch.equal(P3, Pf) and torch.equal(S3, Sf) and l3.cpu().numpy().tobytes() == lf.cpu().numpy().tobytes()
    assert P3.cpu().numpy().tobytes() == P.tobytes()


# ---- an engine over a ready batch, and its subset ---------------------------------------------------------------------------
def test_an_engine_over_a_ready_batch_and_its_subset_keep_the_flag(pkg):
    """InstanceEngine(GraphBatch.from_edge_index(...), terminals=False) against the engine built from handles: the same
    bytes of a step; after an Adam step, subset() - which reads the handles back from the batch - goes on with the flag
    (an engine that dropped it would force rows 0..K-1 and report other bytes) and with the same bytes as the subset of
    the engine built from handles."""
    case = PR.InstCase("mixed", 4, "integer", "expected_cut", 0)
    csrs = PR.inst_case_csrs(case)
    params = PR.inst_case_params(case, csrs)
    handles = handles_of(pkg, csrs)
    rows, cols, ws, ptr = [], [], [], [0]
    for rp, cl, w in csrs:
        n = len(rp) - 1
        rows.append(np.repeat(np.arange(n), np.diff(rp)) + ptr[-1])
        cols.append(cl.astype(np.int64) + ptr[-1])
        ws.append(w)
        ptr.append(ptr[-1] + n)
    ei = np.stack([np.concatenate(rows), np.concatenate(cols)])
    ready = pkg.GraphBatch.from_edge_index(ei, np.asarray(ptr), edge_weight=np.concatenate(ws))
    F, K = params[0]["conv2.weight"].shape
    with pytest.raises(ValueError, match="lives on"):
        pkg.engine.InstanceEngine(ready, F, K, torch.device("cpu"))
    with pytest.raises(ValueError, match="values"):
        pkg.engine.InstanceEngine(ready, F, K, values=[None] * 4)
    eng, ref = engine_with(pkg, ready, params, terminals=False), engine_with(pkg, handles, params, terminals=False)
    assert eng.batch is ready and eng.device == ready.device
    out, want = run_step(eng, CC, case.loss), run_step(ref, CC, case.loss)
    assert [graph_bytes(eng, out, g) for g in range(4)] == [graph_bytes(ref, want, g) for g in range(4)]
    for e in (eng, ref):
        e.adam_step(1e-2)
        e.keep_best(torch.from_numpy(out[1]).to(e.device), torch.from_numpy(out[2]).to(e.device), 0)
    sub, ref_sub = eng.subset([0, 2]), ref.subset([0, 2])
    assert sub.terminals is False and ref_sub.terminals is False and sub.step_count == 1
    assert sub.batch.sizes.tolist() == [5, 65] and sub.batch.host.vals is not None
    got, want = run_step(sub, CC, case.loss), run_step(ref_sub, CC, case.loss)
    assert [graph_bytes(sub, got, g) for g in range(2)] == [graph_bytes(ref_sub, want, g) for g in range(2)]
    assert np.array_equal(got[1], got[0].argmax(1))                      # no row is overridden in the subset either
    forced = engine_with(pkg, [handles[0], handles[2]], [params[0], params[2]], terminals=True)
    assert not np.array_equal(run_step(forced, CC, case.loss)[2], run_step(
        engine_with(pkg, [handles[0], handles[2]], [params[0], params[2]], terminals=False), CC, case.loss)[2])


# ---- solve_dataset(terminals=False) ---------------------------------------------------------------------------------------
def plain_dataset(pkg, sizes):
    """Dataset items [handle, None, networkx graph, terminals (unused)] of small connected graphs."""
    import networkx as nx
    ds = {}
    for i, n in enumerate(sizes):
        _n, rp, cl = PR.ring_with_chords(n, 60 + i)
        g = nx.Graph()
        g.add_nodes_from(range(n))
        g.add_edges_from((v, int(u)) for v in range(n) for u in cl[rp[v]:rp[v + 1]] if v < u)
        ds[i] = [pkg.from_networkx(g), None, g, []]
    return ds


@pytest.mark.parametrize("K", (2, 4))
def test_solve_dataset_without_terminals_against_a_float64_adam_replay(pkg, K):
    """solve_dataset(terminals=False) over three small graphs (one of them below K nodes at K = 4) for five epochs, and
    the same five epochs on an engine from the same seed: after every step the moments and the parameter update of every
    graph are those of a float64 Adam step from the device's state before it, with the float64 gradient without
    terminals (the bars of tests/test_gpu_instance.py's replay); the losses and the kept partitions are solve_dataset's."""
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    from gcn_max_cut_amd.Training import TrainingNeural as T
    F, lr, epochs = 8, 1e-2, 5
    ds = plain_dataset(pkg, [3, 40, 31])
    cfg = T.TrainingConfig(n_nodes=64, hidden_dim=F, number_classes=K, number_epochs=epochs, learning_rate=lr)
    with pytest.raises(ValueError, match="at least"):
        T.solve_dataset(ds, T.TrainingConfig(n_nodes=64, hidden_dim=F, number_classes=4, number_epochs=1))
    torch.manual_seed(3)
    results = T.solve_dataset(ds, cfg, loss="expected_cut", terminals=False)
    handles = [it[0] for it in ds.values()]
    csrs = [KR.csr_of_handle(h) for h in handles]
    eng = pkg.engine.InstanceEngine(handles, F, K, terminals=False)
    torch.manual_seed(3)
    eng.reset_parameters()
    snap = lambda buf: [{k: t.cpu().numpy().astype(np.float64) for k, t in eng.views(g, buf).items()} for g in range(3)]  # noqa: E731
    history = []
    for t in range(1, epochs + 1):
        before, m0, v0 = snap(eng.flat), snap(eng.m), snap(eng.v)
        _P, S, losses = eng.train_fwd_bwd(cfg.C, loss="expected_cut")
        eng.adam_step(lr)
        eng.keep_best(S, losses, t - 1)
        history.append(losses.cpu().numpy())
        after, m_got, v_got = snap(eng.flat), snap(eng.m), snap(eng.v)
        for g, csr in enumerate(csrs):
            p32 = {k: before[g][k].astype(np.float32) for k in KEYS}
            _f, value, grads = PR.inst_step(csr, p32, cfg.C, "expected_cut")
            assert abs(float(losses[g]) - value) <= LOSS_BAR * cfg.C * KR.total_weight([csr]), (t, g)
            for k in KEYS:
                gr = np.asarray(grads[k], np.float64)
                m1, v1, upd = IR.adam_f64(m0[g][k], v0[g][k], gr, t, lr)
                assert np.abs(m_got[g][k] - m1).max() <= 1e-4 * max(np.abs(m1).max(), 1e-30), (t, g, k)
                assert np.abs(v_got[g][k] - v1).max() <= 2e-4 * max(np.abs(v1).max(), 1e-30), (t, g, k)
                big = np.abs(gr) >= 1e-2 * np.abs(gr).max()
                rel = np.abs((after[g][k] - before[g][k]) - upd)[big] / np.abs(upd[big])
                assert big.any() and rel.max() < 0.02, (t, g, k, rel.max())
    history = np.stack(history)
    best_S = eng.best_S.cpu().numpy()
    for g, (res, item) in enumerate(zip(results, ds.values())):
        r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
        assert res["loss_history"] == [float(x) for x in history[:, g]]
        assert res["best_loss"] == float(history[:, g].min()) and res["best_epoch"] == int(history[:, g].argmin())
        assert res["partition"] == best_S[r0:r1].tolist() and set(res["partition"]) <= set(range(K))
        assert res["cut"] == TN.calculate_cut_value(res["partition"], item[2])
    # early stopping rides on the same engine: the flag reaches the engines it rebuilds.  The tolerance is chosen between
    # the graphs' own loss steps, so some stop at once and others run on: a compaction (InstanceEngine.subset) happens,
    # and every history is still a prefix of the run without early stopping - which an engine rebuilt WITH terminals
    # would not give (its losses fix nodes 0..K-1)
    def stop_epochs(tol):
        """The rule of gmc_inst_early_stop_f32 at patience 1 on the recorded losses: the first epoch e > 0 whose loss rose
        or moved by at most tol (None: the graph runs to the end)."""
        out = []
        for g in range(history.shape[1]):
            h = history[:, g].astype(np.float64)
            hit = [e for e in range(1, epochs) if h[e] > h[e - 1] or abs(h[e - 1] - h[e]) <= tol]
            out.append(hit[0] if hit else None)
        return out

    moves = np.sort(np.abs(np.diff(history.astype(np.float64), axis=0)).ravel())
    tols = [float((a + b) / 2) for a, b in zip(moves, moves[1:]) if b > a]
    tol = next(t for t in tols if len(set(stop_epochs(t))) > 1 and any(e is not None and e < epochs - 1 for e in stop_epochs(t)))
    predicted = stop_epochs(tol)
    cfg_stop = T.TrainingConfig(n_nodes=64, hidden_dim=F, number_classes=K, number_epochs=epochs, learning_rate=lr,
                                tolerance=tol, patience=1)
    calls = []
    real_subset = pkg.engine.InstanceEngine.subset
    pkg.engine.InstanceEngine.subset = lambda self, keep: calls.append(list(keep)) or real_subset(self, keep)
    try:
        torch.manual_seed(3)
        stopped = T.solve_dataset(ds, cfg_stop, loss="expected_cut", terminals=False, early_stopping=True, check_every=1,
                                  compact_fraction=0.0)
    finally:
        pkg.engine.InstanceEngine.subset = real_subset
    assert calls, "no compaction happened"
    for res, other, stop in zip(results, stopped, predicted):
        n = epochs if stop is None else stop + 1
        assert other["stopped_epoch"] == stop and other["loss_history"] == res["loss_history"][:n]


# ---- the front door -------------------------------------------------------------------------------------------------------
def cycle_edges(n, r0):
    return [(r0 + v, r0 + (v + 1) % n) for v in range(n)]


def solve_inputs():
    """edge_index / ptr of the path 0 - 2 - 1 and two even cycles (8 and 64 nodes), both directions of every edge."""
    edges = [(0, 2), (2, 1)] + cycle_edges(8, 3) + cycle_edges(64, 11)
    ei = np.asarray(edges + [(b, a) for a, b in edges], np.int64).T
    return ei, np.asarray([0, 3, 11, 75], np.int64)


def host_cuts(ei, ptr, partition):
    part = np.asarray(partition)
    cuts = []
    for g in range(len(ptr) - 1):
        inside = (ei[0] >= ptr[g]) & (ei[0] < ptr[g + 1])
        cuts.append(float((part[ei[0][inside]] != part[ei[1][inside]]).sum()) / 2)
    return np.asarray(cuts, np.float32)


def test_maxcut_solve(pkg):
    from gcn_max_cut_amd import maxcut
    ei, ptr = solve_inputs()
    kw = dict(number_classes=2, hidden_dim=8, epochs=30, learning_rate=2e-2, samples=8, anneal_sweeps=20, seed=4)
    state = torch.random.get_rng_state()
    res = maxcut.solve(torch.from_numpy(ei), torch.from_numpy(ptr), **kw)
    assert torch.equal(torch.random.get_rng_state(), state)                         # torch's generator is left alone
    assert res.partition.is_cuda and res.partition.dtype == torch.int32 and tuple(res.partition.shape) == (75,)
    assert res.ptr.cpu().tolist() == ptr.tolist()
    part, cut = res.partition.cpu().numpy(), res.cut.cpu().numpy()
    trained, rounded = res.trained_cut.cpu().numpy(), res.rounded_cut.cpu().numpy()
    print("cut", cut, "trained", trained, "rounded", rounded)
    assert set(part.tolist()) <= {0, 1}
    assert np.array_equal(cut, host_cuts(ei, ptr, part))                            # the cut of the partition returned
    assert (cut >= np.maximum(trained, rounded)).all()
    assert cut[0] == 2.0                                                            # the path: both edges
    assert (cut <= np.asarray([2, 8, 64], np.float32)).all()
    # the cut of best_S and of the rounding are cuts of real partitions
    assert (trained == np.round(trained)).all() and (rounded == np.round(rounded)).all()
    # the same seeds: the same bytes
    again = maxcut.solve(ei, ptr, **kw)
    for name in ("partition", "cut", "trained_cut", "rounded_cut", "ptr"):
        assert getattr(again, name).cpu().numpy().tobytes() == getattr(res, name).cpu().numpy().tobytes(), name
    # a batch built from handles holds the same bytes as the one built on the device: the same result
    built_here = pkg.GraphBatch.from_edge_index(ei, ptr)
    from_handles = pkg.GraphBatch(built_here.handles(), None, built_here.device)
    third = maxcut.solve_batch(from_handles, **kw)
    for name in ("partition", "cut", "trained_cut", "rounded_cut", "ptr"):
        assert getattr(third, name).cpu().numpy().tobytes() == getattr(res, name).cpu().numpy().tobytes(), name
    # with terminals nodes 0 and 1 of every graph are forced apart: the path loses an edge
    fixed = maxcut.solve(ei, ptr, terminals=True, **kw)
    fp = fixed.partition.cpu().numpy()
    assert fixed.cut.cpu().numpy()[0] == 1.0 and all(fp[r:r + 2].tolist() == [0, 1] for r in ptr[:-1])
    assert np.array_equal(fixed.cut.cpu().numpy(), host_cuts(ei, ptr, fp))
