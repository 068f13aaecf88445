"""GPU tests of one model per graph beyond 4096 nodes (gmc_inst_large_*, csrc/instance_large.hip,
engine.LargeInstanceEngine, maxcut.solve_large) against the float64 step of tests/large_instance_ref.py.

Bars: stepcheck's P_TOL for the probabilities, ORACLE_BAR and ROW_TOL / ROW_FLOOR for every gradient row, and LOSS_BAR =
5e-5 * C * total weight for weighted and relaxed losses, as tests/test_gpu_instance.py has them.  S must be the
reference's decode on every row and the hard loss of a unit-weight graph exactly -C * cut: tests/test_large_instance_host.py
asserts the preconditions on the float64 reference.  The two cases above 65,535 nodes follow large_ref's rule: at most
MAX_TIES rows, each within TIE of a tie in the reference, may decode the other way, and the hard loss and its gradient are
then those of the partition the device chose."""

import numpy as np
import pytest
import torch

from tests import functional_ref as FR
from tests import instance_ref as IR
from tests import kway_ref as KR
from tests import large_instance_ref as LI
from tests import large_ref as LR
from tests import plain_ref as PR
from tests import stepcheck
from tests.stepcheck import KEYS, ORACLE_BAR, P_TOL, ROW_FLOOR, ROW_TOL

pytestmark = pytest.mark.gpu
LOSS_BAR = 5e-5
CC = LI.CC
TAGS = (["gather_w1"] * 2 + ["agg_fwd"] * 2 + ["dense_mfma"] + ["head"] * 4 + ["hidden_bwd", "colsum"] + ["agg_bwd"] * 2 +
        ["dw1"] * 2)
FORWARD_TAGS = TAGS[:8]


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def engine_with(pkg, handles, params, terminals, cls="LargeInstanceEngine"):
    F, K = params[0]["conv2.weight"].shape
    eng = getattr(pkg.engine, cls)(handles, F, K, terminals=bool(terminals))
    for g, p in enumerate(params):
        for k, v in eng.views(g).items():
            v.copy_(torch.from_numpy(p[k]))
    return eng


def run_step(pkg, eng, Cc, loss):
    """One train_fwd_bwd under the probe with the scratch and the gradient poisoned: P, S, loss, the per-graph gradient
    dicts, the launches' tags."""
    eng._workspace(True).fill_(255)
    eng.grad.fill_(float("nan"))
    with pkg.hip.Probe(64) as probe:
        P, S, losses = eng.train_fwd_bwd(Cc, loss=loss)
        grads = [{k: v.cpu().numpy() for k, v in eng.views(g, eng.grad).items()} for g in range(eng.B)]
    assert not any(probe.flavours)
    return P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy(), grads, [t for t, _ms in probe.records]


def graph_bytes(eng, out, g):
    """Everything a step reports of graph g, as bytes: its rows of P and S, its loss, its four gradient slices."""
    P, S, losses, grads = out[:4]
    r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
    return (P[r0:r1].tobytes(), S[r0:r1].tobytes(), losses[g:g + 1].tobytes()) + tuple(grads[g][k].tobytes() for k in KEYS)


def case_setup(pkg, case):
    return LI.case_handles(pkg, case), LI.case_csrs(case), LI.case_params(case)


# ---- one poisoned step of every case against float64
@pytest.mark.parametrize("case", LI.CASES, ids=LI.case_id)
def test_step_against_float64(pkg, case):
    handles, csrs, params = case_setup(pkg, case)
    eng = engine_with(pkg, handles, params, case.terminals)
    what, K, big = LI.case_id(case), case.K, LI.is_big(case)
    assert (eng.batch.host.vals is not None) == (case.weights == "real")
    assert np.array_equal(eng.flat[:eng.count].cpu().numpy(), IR.pack(params))
    out = run_step(pkg, eng, CC, case.loss)
    P, S, losses, grads, tags = out
    assert tags == TAGS, tags
    assert P.shape == (eng.R, K) and np.isfinite(P).all() and losses.dtype == np.float32
    for g, (csr, p) in enumerate(zip(csrs, params)):
        r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
        ref = LI.step(csr, p, CC, case.loss, case.terminals, S_got=S[r0:r1] if big else None)
        p_err = float(np.abs(P[r0:r1] - ref.P).max())
        assert p_err < P_TOL, (what, g, p_err)
        if big:
            ties = LI.near_ties(ref.P, S[r0:r1], K, case.terminals)
            assert ties <= LR.MAX_TIES, (what, ties)
        else:
            assert np.array_equal(S[r0:r1], LI.decode(ref.P, K, case.terminals)), (what, g)
        first = LI.forced(r1 - r0, K, case.terminals)
        assert np.array_equal(S[r0:r0 + first], np.arange(first)), (what, g)
        bar = LOSS_BAR * CC * KR.total_weight([csr])
        err = abs(float(losses[g]) - ref.loss)
        worst_abs, worst_row = FR.grad_ratios(grads[g], ref.grads)
        print(f"{what} graph {g}: P {p_err:.2e} loss {losses[g]:.6f} float64 {ref.loss:.6f} err {err:.2e} bar {bar:.2e} "
              f"grad {worst_abs:.2e} of ORACLE_BAR, rows {worst_row:.2e} of ROW_TOL")
        assert err <= bar, (what, g, losses[g], ref.loss)
        if case.loss == "cut" and case.weights == "unit":   # the cut is an integer, the loss its one float32 product with -C
            cut = round(-ref.loss / CC)
            assert abs(-ref.loss / CC - cut) < 1e-9 and losses[g] == -(np.float32(CC) * np.float32(cut)), (what, g)
        res = stepcheck.compare_grads(grads[g], ref.grads, what=(what, g), grad_bar=ORACLE_BAR, row_tol=ROW_TOL,
                                      row_floor=ROW_FLOOR)
        assert res["rows"] <= ROW_TOL and worst_abs <= 1.0 and worst_row <= 1.0, (what, g, res, worst_abs, worst_row)
    # a second step gives the same bytes; the forward alone reports the same P, S and loss
    again = run_step(pkg, eng, CC, case.loss)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(out[:3], again[:3])), what
    assert [graph_bytes(eng, again, g) for g in range(eng.B)] == [graph_bytes(eng, out, g) for g in range(eng.B)], what
    eng._workspace(False).fill_(255)
    with pkg.hip.Probe(16) as probe:
        Pf, Sf, lf = (t.cpu().numpy() for t in eng.forward(CC, loss=case.loss))
    assert [t for t, _ms in probe.records] == FORWARD_TAGS
    assert Pf.tobytes() == P.tobytes() and Sf.tobytes() == S.tobytes() and lf.tobytes() == losses.tobytes(), what


# ---- against gmc_inst_*_t on batches both accept
def forward_buffers(eng, Cc, loss):
    """H [R, ld] and Z0 [R, K] as a forward leaves them in the (poisoned) workspace: the second and third buffer of the
    layout include/gcnmaxcut.h states, each rounded up to 256 bytes."""
    ws = eng._workspace(False)
    ws.fill_(255)
    eng.forward(Cc, loss=loss)
    ld = (eng.Fp + 31) // 32 * 32
    up = lambda x: (x + 255) // 256 * 256   # noqa: E731
    h0, z0 = up(eng.R * ld * 4), 2 * up(eng.R * ld * 4)
    raw = ws.cpu().numpy()
    return raw[h0:h0 + eng.R * ld * 4].tobytes(), raw[z0:z0 + eng.R * eng.K * 4].tobytes()


@pytest.mark.parametrize("case", LI.COMPARE, ids=LI.case_id)
def test_against_the_one_workgroup_sequence(pkg, case):
    """The two sequences on the same inputs: identical S, P within twice P_TOL, the gradient within twice the bars, the
    unit hard loss byte-equal - and H and Z0 byte-equal: the tile walk of linst_hw2 changes no row's bytes."""
    handles, csrs, params = case_setup(pkg, case)
    large = engine_with(pkg, handles, params, case.terminals)
    small = engine_with(pkg, handles, params, case.terminals, "InstanceEngine")
    got, want = run_step(pkg, large, CC, case.loss), run_step(pkg, small, CC, case.loss)
    what = LI.case_id(case)
    assert got[1].tobytes() == want[1].tobytes(), what
    p_err = float(np.abs(got[0].astype(np.float64) - want[0]).max())
    assert p_err <= 2 * P_TOL, (what, p_err)
    for g, csr in enumerate(csrs):
        if case.loss == "cut" and case.weights == "unit":
            assert got[2][g:g + 1].tobytes() == want[2][g:g + 1].tobytes(), (what, g)
        assert abs(float(got[2][g]) - float(want[2][g])) <= 2 * LOSS_BAR * CC * KR.total_weight([csr]), (what, g)
        ref = {k: want[3][g][k].astype(np.float64) for k in KEYS}
        res = stepcheck.compare_grads(got[3][g], ref, what=(what, g), grad_bar=2 * ORACLE_BAR, row_tol=2 * ROW_TOL,
                                      row_floor=ROW_FLOOR)
        print(f"{what} graph {g}: P {p_err:.2e} rows {res['rows']:.2e}")
    assert forward_buffers(large, CC, case.loss) == forward_buffers(small, CC, case.loss), what


# ---- independence, byte for byte; no cross-talk
BATCH_CASES = [c for c in LI.CASES if c.shape == "batch" and c.K != 2]   # (5, 700, 257): K = 3, 4 with terminals, 8 without
assert [(c.K, c.terminals) for c in BATCH_CASES] == [(3, 1), (4, 1), (8, 0)]


@pytest.mark.parametrize("case", BATCH_CASES, ids=LI.case_id)
def test_a_graph_does_not_depend_on_its_batch(pkg, case):
    """Each graph of the (5, 700, 257) batch alone, first, in the middle and last: the same bytes every time."""
    handles, _csrs, params = case_setup(pkg, case)
    eng = engine_with(pkg, handles, params, case.terminals)
    whole = run_step(pkg, eng, CC, case.loss)
    for g in range(3):
        want = graph_bytes(eng, whole, g)
        a, b = [i for i in range(3) if i != g]
        for order in ([g], [g, a, b], [a, g, b], [a, b, g]):
            e = engine_with(pkg, [handles[i] for i in order], [params[i] for i in order], case.terminals)
            assert graph_bytes(e, run_step(pkg, e, CC, case.loss), order.index(g)) == want, (g, order)


@pytest.mark.parametrize("case", BATCH_CASES[1:], ids=LI.case_id)
def test_nan_parameters_of_one_graph_stay_in_that_graph(pkg, case):
    handles, _csrs, params = case_setup(pkg, case)
    eng = engine_with(pkg, handles, params, case.terminals)
    clean = run_step(pkg, eng, CC, case.loss)
    for v in eng.views(1).values():
        v.fill_(float("nan"))
    dirty = run_step(pkg, eng, CC, case.loss)
    for g in (0, 2):
        assert graph_bytes(eng, dirty, g) == graph_bytes(eng, clean, g), g
    assert np.isnan(dirty[2][1]) and np.isnan(dirty[0][5 + 350]).all()       # the relaxed loss of graph 1, one of its rows
    assert np.isfinite(dirty[2][[0, 2]]).all()


# ---- the existing paths are where they were
def test_existing_paths_give_the_same_bytes_around_a_large_instance_call(pkg):
    """gmc_inst_train_fwd_bwd_t and gmc_large_train_fwd_bwd before and after a gmc_inst_large_train_fwd_bwd call that
    shares their workspace buffer; InstanceEngine still refuses 4097 nodes."""
    case = LI.Case("mixed", 4, "real", "expected_cut", 1, 0)
    handles, _csrs, params = case_setup(pkg, case)
    small = engine_with(pkg, handles, params, 1, "InstanceEngine")
    large = engine_with(pkg, handles, params, 1)
    big_case = next(c for c in LR.CASES if c.shape == "n4097")                # K = 3, unit weights, hard loss
    shared_params = LR.case_params(big_case)
    N, F = shared_params["conv1.weight"].shape
    fused = pkg.engine.FusedEngine(N, F, big_case.K, kway=False)
    for k, v in fused.views().items():
        v.copy_(torch.from_numpy(shared_params[k]))
    batch = pkg.GraphBatch(LR.case_handles(pkg, big_case), None, fused.device)
    assert fused.needs_large(batch)
    ws = torch.empty(max(small.workspace_bytes(True), large.workspace_bytes(True), fused.workspace_bytes(batch, True)),
                     dtype=torch.uint8, device=small.device)
    small._ws = large._ws = fused._ws = ws

    def fused_step():
        ws.fill_(255)
        fused.grad.fill_(float("nan"))
        P, S, losses = fused.train_fwd_bwd(batch, CC)
        return tuple(t.cpu().numpy().tobytes() for t in (P, S, losses, fused.grad[:fused.count + 1]))

    def small_step():
        out = run_step(pkg, small, CC, case.loss)
        return [graph_bytes(small, out, g) for g in range(small.B)], out[4]

    before_small, before_fused = small_step(), fused_step()
    assert before_small[1] == ["gather_w1", "agg_fwd", "dense_mfma", "head", "hidden_bwd", "colsum", "agg_bwd", "dw1"]
    run_step(pkg, large, CC, case.loss)
    assert small._ws is ws and large._ws is ws and fused._ws is ws
    assert small_step() == before_small and fused_step() == before_fused
    with pytest.raises(ValueError, match="beyond the one-workgroup head"):
        pkg.engine.InstanceEngine(LR.case_handles(pkg, big_case), 8, 3)


# ---- the engine: epochs, keep-best, subset, early stopping, a batch built on the device
def edge_index_of(csrs):
    rows, cols, ws, ptr = [], [], [], [0]
    for rp, cl, w in csrs:
        n = len(rp) - 1
        rows.append(np.repeat(np.arange(n), np.diff(rp)) + ptr[-1])
        cols.append(np.asarray(cl, np.int64) + ptr[-1])
        ws.append(w)
        ptr.append(ptr[-1] + n)
    weight = None if ws[0] is None else np.concatenate(ws)
    return np.stack([np.concatenate(rows), np.concatenate(cols)]), np.asarray(ptr, np.int64), weight


def engine_graphs():
    return [LR.circulant(5, 3), LR.circulant(300, 7, 11), LR.circulant(4100, 7, 12)]


@pytest.mark.parametrize("K,terminals", ((3, True), (2, False)))
def test_five_epochs_against_a_float64_adam_replay_and_keep_best(pkg, K, terminals):
    """train_fwd_bwd + adam_step + keep_best five times over (5, 300, 4100) from the engine's own init: after every step
    the moments and the update of every graph are those of a float64 Adam step from the device's state before it with
    the float64 gradient (the bars of tests/test_gpu_instance.py's replay), best_S / best_loss / best_epoch are the host
    restatement's; then subset([0, 2]) goes on with the same bytes for its graphs, and an engine over the batch built
    on the device from edge_index gives the bytes of the one built from handles."""
    F, lr, loss = 8, 1e-2, "expected_cut"
    csrs = [(rp.astype(np.int32), cl.astype(np.int32), None) for _n, rp, cl in engine_graphs()]
    handles = [pkg.GraphHandle(len(rp) - 1, rp, cl, None) for rp, cl, _w in csrs]
    eng = pkg.engine.LargeInstanceEngine(handles, F, K, terminals=terminals)
    ei, ptr, _w = edge_index_of(csrs)
    twin = pkg.engine.LargeInstanceEngine(pkg.GraphBatch.from_edge_index(ei, ptr), F, K, terminals=terminals)
    for e in (eng, twin):
        torch.manual_seed(K)
        e.reset_parameters()
    host = IR.KeepBest(eng.batch.goff_host)
    snap = lambda buf: [{k: t.cpu().numpy().astype(np.float64) for k, t in eng.views(g, buf).items()} for g in range(3)]  # noqa: E731
    for t in range(1, 6):
        before, m0, v0 = snap(eng.flat), snap(eng.m), snap(eng.v)
        _P, S, losses = eng.train_fwd_bwd(1.0, loss=loss)
        eng.adam_step(lr)
        eng.keep_best(S, losses, t - 1)
        _P2, S2, losses2 = twin.train_fwd_bwd(1.0, loss=loss)
        twin.adam_step(lr)
        twin.keep_best(S2, losses2, t - 1)
        host.update(S.cpu().numpy(), losses.cpu().numpy(), t - 1)
        after, m_got, v_got = snap(eng.flat), snap(eng.m), snap(eng.v)
        for g, csr in enumerate(csrs):
            p32 = {k: before[g][k].astype(np.float32) for k in KEYS}
            ref = LI.step(csr, p32, 1.0, loss, terminals)
            assert abs(float(losses[g]) - ref.loss) <= LOSS_BAR * KR.total_weight([csr]), (t, g)
            for k in KEYS:
                gr = np.asarray(ref.grads[k], np.float64)
                m1, v1, upd = IR.adam_f64(m0[g][k], v0[g][k], gr, t, lr)
                assert np.abs(m_got[g][k] - m1).max() <= 1e-4 * max(np.abs(m1).max(), 1e-30), (t, g, k)
                assert np.abs(v_got[g][k] - v1).max() <= 2e-4 * max(np.abs(v1).max(), 1e-30), (t, g, k)
                # the update is m1 / sqrt(v1): judged relative to itself where neither the gradient nor m1 - in which
                # 0.9 m0 and 0.1 g may cancel from the second step on, and the bar on m is relative to the largest
                # entry - is below 1 % of its tensor's largest
                big = (np.abs(gr) >= 1e-2 * np.abs(gr).max()) & (np.abs(m1) >= 1e-2 * np.abs(m1).max())
                rel = np.abs((after[g][k] - before[g][k]) - upd)[big] / np.abs(upd[big])
                assert big.any() and rel.max() < 0.02, (t, g, k, rel.max())
        assert eng.best_loss.cpu().numpy().tobytes() == host.best_loss.tobytes()
        assert eng.best_epoch.cpu().numpy().tobytes() == host.best_epoch.tobytes()
        assert eng.best_S.cpu().numpy().tobytes() == host.best_S.tobytes()
    for name in ("flat", "grad", "m", "v", "best_S", "best_loss", "best_epoch"):
        assert torch.equal(getattr(eng, name), getattr(twin, name)), name
    # subset([0, 2]) goes on where the engine stands, with the same bytes for its graphs
    sub = eng.subset([0, 2])
    assert type(sub) is pkg.engine.LargeInstanceEngine and sub.terminals is terminals and sub.step_count == 5
    assert sub.batch.sizes.tolist() == [5, 4100]
    whole, part = run_step(pkg, eng, 1.0, loss), run_step(pkg, sub, 1.0, loss)
    assert [graph_bytes(sub, part, 0), graph_bytes(sub, part, 1)] == [graph_bytes(eng, whole, 0), graph_bytes(eng, whole, 2)]
    eng.adam_step(lr)
    sub.adam_step(lr)
    for g_sub, g in enumerate((0, 2)):
        for buf_e, buf_s in ((eng.flat, sub.flat), (eng.m, sub.m), (eng.v, sub.v)):
            for k in KEYS:
                assert torch.equal(eng.views(g, buf_e)[k], sub.views(g_sub, buf_s)[k]), (g, k)


def test_early_stop_freezes_a_stopped_graph(pkg):
    """early_stop with adam_step(running_only=True): a graph that stopped keeps every byte of its parameters, moments,
    best partition and state while the others move."""
    handles = [pkg.GraphHandle(*g) for g in engine_graphs()]
    eng = pkg.engine.LargeInstanceEngine(handles, 8, 2, terminals=False)
    torch.manual_seed(1)
    eng.reset_parameters()
    eng.stop_epoch[1] = 0                                                     # graph 1 stopped earlier
    _P, S, losses = eng.train_fwd_bwd(1.0, loss="expected_cut")
    eng.adam_step(1e-2, running_only=True)
    eng.early_stop(S, losses, 0, 1e-9, 2)
    r0, r1 = int(eng.batch.goff_host[1]), int(eng.batch.goff_host[2])
    frozen = lambda: ([eng.views(1, buf)[k].cpu().numpy().tobytes() for buf in (eng.flat, eng.m, eng.v) for k in KEYS],  # noqa: E731
                      eng.best_S[r0:r1].cpu().numpy().tobytes(), float(eng.best_loss[1]), int(eng.stall[1]))
    moving = lambda: [eng.views(g, eng.flat)[KEYS[0]].cpu().numpy().tobytes() for g in (0, 2)]   # noqa: E731
    was, moved = frozen(), moving()
    assert not any(np.frombuffer(b, np.float32).any() for b in was[0][4:])     # its moments were never written
    assert float(eng.best_loss[1]) == float("inf") and float(eng.best_loss[2]) < 0
    for epoch in (1, 2):
        _P, S, losses = eng.train_fwd_bwd(1.0, loss="expected_cut")
        eng.adam_step(1e-2, running_only=True)
        eng.early_stop(S, losses, epoch, 1e-9, 2)
    assert frozen() == was and all(a != b for a, b in zip(moving(), moved))
    assert eng.stopped().tolist()[1] == 0


# ---- solve_large
def cycle_edges(n, r0):
    return [(r0 + v, r0 + (v + 1) % n) for v in range(n)]


def solve_inputs():
    """edge_index / ptr of the path 0 - 2 - 1, an even cycle of 4100 nodes and a ring of 5000 nodes plus chords, both
    directions of every edge; and the graphs' CSRs."""
    n, rp, cl = PR.ring_with_chords(5000, 3)
    chords = [(3 + 4100 + v, 3 + 4100 + int(u)) for v in range(n) for u in cl[rp[v]:rp[v + 1]] if v < u]
    edges = [(0, 2), (2, 1)] + cycle_edges(4100, 3) + chords
    ei = np.asarray(edges + [(b, a) for a, b in edges], np.int64).T
    return ei, np.asarray([0, 3, 4103, 9103], np.int64)


def host_cuts(ei, ptr, partition):
    part = np.asarray(partition)
    cuts = []
    for g in range(len(ptr) - 1):
        inside = (ei[0] >= ptr[g]) & (ei[0] < ptr[g + 1])
        cuts.append(float((part[ei[0][inside]] != part[ei[1][inside]]).sum()) / 2)
    return np.asarray(cuts, np.float32)


@pytest.mark.parametrize("K", (2, 3))
def test_solve_large(pkg, K):
    from gcn_max_cut_amd import maxcut
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    ei, ptr = solve_inputs()
    kw = dict(number_classes=K, hidden_dim=8, epochs=20, learning_rate=2e-2, samples=6, anneal_sweeps=10,
              max_descent_sweeps=100, seed=4)
    with pytest.raises(ValueError, match="solve_large"):
        maxcut.solve(ei, ptr, **kw)                                                 # the front door keeps refusing
    state = torch.random.get_rng_state()
    res = maxcut.solve_large(torch.from_numpy(ei), torch.from_numpy(ptr), **kw)
    assert torch.equal(torch.random.get_rng_state(), state)                         # torch's generator is left alone
    assert isinstance(res, maxcut.MaxCutResult) and res.partition.is_cuda and res.partition.dtype == torch.int32
    assert tuple(res.partition.shape) == (9103,) and res.ptr.cpu().tolist() == ptr.tolist()
    part, cut = res.partition.cpu().numpy(), res.cut.cpu().numpy()
    trained, rounded = res.trained_cut.cpu().numpy(), res.rounded_cut.cpu().numpy()
    print("cut", cut, "trained", trained, "rounded", rounded)
    assert set(part.tolist()) <= set(range(K))
    assert np.array_equal(cut, host_cuts(ei, ptr, part))                            # the cut of the partition returned
    assert (cut >= np.maximum(trained, rounded)).all()
    assert cut[0] == 2.0 and cut[1] <= 4100                                         # the path: both edges
    assert (trained == np.round(trained)).all() and (rounded == np.round(rounded)).all()
    # after the descent no single move gains
    batch = pkg.GraphBatch.from_edge_index(ei, ptr)
    for g, h in enumerate(batch.handles()):
        own = part[ptr[g]:ptr[g + 1]]
        assert PR.best_single_move_gain(h.n, h.rowptr, h.col, None, own, K, 0) <= 0.0, g
    # the same seeds: the same bytes
    again = maxcut.solve_large(ei, ptr, **kw)
    names = ("partition", "cut", "trained_cut", "rounded_cut", "ptr")
    for name in names:
        assert getattr(again, name).cpu().numpy().tobytes() == getattr(res, name).cpu().numpy().tobytes(), name
    # the result is the hand composition of LargeInstanceEngine and the three large decoders
    eng = pkg.engine.LargeInstanceEngine(batch, 8, K, terminals=False)
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(4)
        eng.reset_parameters()
    for epoch in range(20):
        _P, S, losses = eng.train_fwd_bwd(1.0, loss="expected_cut")
        eng.adam_step(2e-2)
        eng.keep_best(S, losses, epoch)
    P, _S, _l = eng.forward(1.0, loss="expected_cut")
    r_assign, r_cut, _, _ = T._round_on_gpu(batch, P, 0, False, large=True)
    best = eng.best_S.to(torch.int8).reshape(1, -1)
    _, t_cut, _ = T._kway_anneal_on_gpu(batch, K, best.clone(), np.zeros(0, np.float32), 0, 0, terminals=False, large=True)
    samples = T._kway_sample_on_gpu(batch, P, 6, 4, range(batch.B), True, terminals=False, large=True)[3]
    cands = torch.cat([best, r_assign.reshape(1, -1), samples]).contiguous()
    inv_temp = T.anneal_schedule(10, scale=T._mean_edge_weight(batch))
    h_part, h_cut, _ = T._kway_anneal_on_gpu(batch, K, cands, inv_temp, 4, 100, terminals=False, large=True)
    for got, want in ((h_part, res.partition), (h_cut, res.cut), (t_cut, res.trained_cut), (r_cut, res.rounded_cut)):
        assert got.cpu().numpy().tobytes() == want.cpu().numpy().tobytes()
    # a batch built from handles holds the same bytes as the one built on the device: the same result
    third = maxcut.solve_large_batch(pkg.GraphBatch(batch.handles(), None, batch.device), **kw)
    for name in names:
        assert getattr(third, name).cpu().numpy().tobytes() == getattr(res, name).cpu().numpy().tobytes(), name
    # with terminals nodes 0..K-1 of every graph hold classes 0..K-1
    fixed = maxcut.solve_large(ei, ptr, terminals=True, **kw)
    fp = fixed.partition.cpu().numpy()
    assert all(fp[r:r + K].tolist() == list(range(K)) for r in ptr[:-1])
    assert np.array_equal(fixed.cut.cpu().numpy(), host_cuts(ei, ptr, fp))
    assert (fixed.cut.cpu().numpy() >= np.maximum(fixed.trained_cut.cpu().numpy(), fixed.rounded_cut.cpu().numpy())).all()
