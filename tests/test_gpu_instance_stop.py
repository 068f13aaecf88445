"""GPU tests of per-graph early stopping for one model per graph (gmc_inst_early_stop_f32, gmc_inst_adam_f32,
InstanceEngine.early_stop / adam_step(running_only=True) / subset, solve_dataset(early_stopping=True)).

Everything here is byte for byte: the segmented Adam sweep against gmc_adam_f32 over the same floats (one definition of
the update), the device's stop state against the restatement of tests/instance_stop_ref.py, a frozen graph against
itself, a compacted engine against the uncompacted one, and an early-stopped graph against a solo run of the same graph
without early stopping for stopped_epoch + 1 epochs.  The one bar that is not zero is the float64 check of the moments in
the masked test: m within 1e-4 and v within 2e-4 of the largest entry, the bars of
test_three_epochs_against_a_float64_adam_replay."""
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import instance_ref as IR
from tests import instance_stop_ref as SR
from tests import util

pytestmark = pytest.mark.gpu
LR = 1e-2
SENTINEL = 1234.5


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def sizes_of(batch, K):
    raw = {"mixed": (5, 300, 65, 257), "edge": ("K", "K+1", 256), "single": (65,)}[batch] if isinstance(batch, str) else batch
    return [max({"K": K, "K+1": K + 1}.get(n, n), 3, K) for n in raw]


def engine_of(pkg, sizes, F, K):
    handles = [pkg.from_networkx(util.near_regular(n, 3, 50 + i)) for i, n in enumerate(sizes)]
    eng = pkg.engine.InstanceEngine(handles, F, K)
    assert eng.Fp == F and list(eng.batch.sizes) == list(sizes)
    return eng


def fill_random(eng, seed):
    """Random param / grad / m / v (v >= 0) over the count floats, a sentinel in the four floats after them."""
    gen = torch.Generator().manual_seed(seed)
    for buf, scale, positive in ((eng.flat, 1.0, False), (eng.grad, 0.3, False), (eng.m, 0.1, False), (eng.v, 0.01, True)):
        x = torch.randn(eng.count, generator=gen) * scale
        buf[:eng.count].copy_(x * x if positive else x)
        buf[eng.count:].fill_(SENTINEL)


def snapshot(eng):
    return {k: getattr(eng, k).clone() for k in ("flat", "grad", "m", "v")}


def restore(eng, snap):
    for k, t in snap.items():
        getattr(eng, k).copy_(t)


def flat_adam(pkg, eng, step):
    rc = pkg.hip.load().gmc_adam_f32(pkg.hip.ptr(eng.flat), pkg.hip.ptr(eng.grad), pkg.hip.ptr(eng.m), pkg.hip.ptr(eng.v),
                                     eng.count, LR, 0.9, 0.999, 1e-8, step, pkg.hip.stream())
    pkg.hip.check(rc, "gmc_adam_f32")


def inst_adam(pkg, eng, step, stop):
    """gmc_inst_adam_f32 with ``stop`` = None (a NULL mask) or an int32 device tensor; asserts the one launch's tag."""
    with pkg.hip.Probe(4) as probe:
        rc = pkg.hip.load().gmc_inst_adam_f32(eng.batch.ref(), eng.Fp, eng.K, pkg.hip.ptr(eng.flat), pkg.hip.ptr(eng.grad),
                                              pkg.hip.ptr(eng.m), pkg.hip.ptr(eng.v), LR, 0.9, 0.999, 1e-8, step,
                                              pkg.hip.ptr(stop), pkg.hip.stream())
        pkg.hip.check(rc, "gmc_inst_adam_f32")
    assert [t for t, _ms in probe.records] == ["adam"]


def host(eng):
    return {k: getattr(eng, k).cpu().numpy() for k in ("flat", "m", "v", "grad")}


# ---- Adam, byte for byte
ADAM_CASES = [("mixed", 4, 2), ("mixed", 12, 3), ("mixed", 260, 8), ("edge", 4, 3), ("edge", 12, 8), ("edge", 260, 2),
              ("single", 4, 8), ("single", 12, 3), ("single", 260, 3)]


@pytest.mark.parametrize("batch,F,K", ADAM_CASES, ids=[f"{b}-F{F}-K{K}" for b, F, K in ADAM_CASES])
def test_segmented_adam_is_the_flat_sweep_byte_for_byte(pkg, batch, F, K):
    eng = engine_of(pkg, sizes_of(batch, K), F, K)
    if (batch, K) in (("edge", 3), ("single", 3)):
        assert eng.B * K % 4                                    # b2 segments off the 16-byte grid
    fill_random(eng, 7 * F + K)
    start = snapshot(eng)
    none_stopped = torch.full((eng.B,), -1, dtype=torch.int32, device=eng.device)
    for step in (1, 7):
        restore(eng, start)
        flat_adam(pkg, eng, step)
        want = host(eng)
        assert not np.array_equal(want["flat"][:eng.count], start["flat"][:eng.count].cpu().numpy())
        for stop in (None, none_stopped):
            restore(eng, start)
            inst_adam(pkg, eng, step, stop)
            got = host(eng)
            for k in ("flat", "m", "v", "grad"):
                assert got[k].tobytes() == want[k].tobytes(), (k, step, stop is None)
                assert (got[k][eng.count:] == SENTINEL).all(), (k, step)        # the four floats after count
    # the engine's own door
    restore(eng, start)
    eng.step_count = 6
    eng.adam_step(LR, running_only=True)
    assert eng.step_count == 7 and host(eng)["flat"].tobytes() == want["flat"].tobytes()


@pytest.mark.parametrize("rows", (-1, 0, 1))
def test_segmented_adam_at_the_edges_of_its_w1_tile(pkg, rows):
    F, K = 4, 3
    n = pkg.hip.INST_ADAM_TILE_FLOATS // F + rows               # one row fewer than, exactly and one more than a tile
    eng = engine_of(pkg, [n], F, K)
    fill_random(eng, n)
    start = snapshot(eng)
    flat_adam(pkg, eng, 3)
    want = host(eng)
    restore(eng, start)
    inst_adam(pkg, eng, 3, None)
    got = host(eng)
    for k in ("flat", "m", "v"):
        assert got[k].tobytes() == want[k].tobytes(), k
        assert (got[k][eng.count:] == SENTINEL).all()


# ---- Adam, masked
@pytest.mark.parametrize("stopped", ([0], [1], [3], [0, 1, 2, 3]), ids=("first", "middle", "last", "all"))
def test_masked_adam_passes_stopped_graphs_by(pkg, stopped):
    F, K = 12, 3
    sizes = sizes_of("mixed", K)
    eng = engine_of(pkg, sizes, F, K)
    segs = SR.segments(sizes, F, K)
    fill_random(eng, 3)
    clean = snapshot(eng)
    inst_adam(pkg, eng, 4, None)
    unmasked = host(eng)
    restore(eng, clean)
    for g in stopped:                                          # whatever a stopped graph's gradient holds is not read
        eng.grad[torch.from_numpy(segs[g]).to(eng.device)] = float("nan")
    stop = torch.full((4,), -1, dtype=torch.int32)
    stop[stopped] = 2
    before = host(eng)
    inst_adam(pkg, eng, 4, stop.to(eng.device))
    got = host(eng)
    for g, seg in enumerate(segs):
        for k in ("flat", "m", "v"):
            want = before if g in stopped else unmasked
            assert got[k][seg].tobytes() == want[k][seg].tobytes(), (g, k)
    assert all((got[k][eng.count:] == SENTINEL).all() for k in ("flat", "m", "v"))
    assert np.isfinite(got["flat"][:eng.count]).all()
    # float64: the moments of the running graphs, the stopped ones as they were
    _p64, m64, v64 = SR.adam_f64_masked(sizes, F, K, before["flat"][:eng.count], before["grad"][:eng.count],
                                        before["m"][:eng.count], before["v"][:eng.count], 4, LR,
                                        [g in stopped for g in range(4)])
    assert np.abs(got["m"][:eng.count] - m64).max() <= 1e-4 * np.abs(m64).max()
    assert np.abs(got["v"][:eng.count] - v64).max() <= 2e-4 * np.abs(v64).max()


# ---- the stop rule on the device
def device_state(eng):
    return tuple(getattr(eng, k).cpu().numpy().tobytes() for k in ("prev_loss", "stall", "stop_epoch", "best_S", "best_loss",
                                                                   "best_epoch"))


def made_up_S(eng, e):
    return ((torch.arange(eng.R, dtype=torch.int32) * 7 + e) % 3).to(eng.device)


@pytest.mark.parametrize("key", list(SR.SEQUENCES), ids=[f"tol{t}-patience{p}" for t, p in SR.SEQUENCES])
def test_stop_rule_against_the_restatement(pkg, key):
    tol, pat = key
    seqs = SR.SEQUENCES[key]
    sizes = [(5, 300, 65, 257)[i % 4] for i in range(len(seqs))]
    eng = engine_of(pkg, sizes, 4, 3)
    rule = SR.StopRule(eng.batch.goff_host, tol, pat)
    assert device_state(eng) == rule.state()                   # +inf, 0, -1; zeros, +inf, -1
    for e in range(SR.EPOCHS):
        S = made_up_S(eng, e)
        losses = np.asarray([s.losses[e] for s in seqs], np.float32)
        with pkg.hip.Probe(4) as probe:
            eng.early_stop(S, torch.from_numpy(losses).to(eng.device), e, tol, pat)
        assert [t for t, _ms in probe.records] == ["finish", "finish"]
        rule.update(S.cpu().numpy(), losses, e)
        assert device_state(eng) == rule.state(), e
    stops = eng.stopped()
    assert stops.dtype == torch.int32 and not stops.is_cuda
    assert [int(x) if x >= 0 else None for x in stops] == [s.stop for s in seqs]
    assert eng.best_epoch.cpu().tolist() == [s.best_epoch for s in seqs]
    eng.reset_parameters()
    assert device_state(eng) == SR.StopRule(eng.batch.goff_host, tol, pat).state()


def test_with_patience_out_of_reach_the_best_is_keep_bests(pkg):
    key = (0.25, 2)
    seqs = SR.SEQUENCES[key]
    sizes = [(5, 300, 65, 257)[i % 4] for i in range(len(seqs))]
    a, b = engine_of(pkg, sizes, 4, 3), engine_of(pkg, sizes, 4, 3)
    for e in range(SR.EPOCHS):
        S = made_up_S(a, e)
        losses = torch.from_numpy(np.asarray([s.losses[e] for s in seqs], np.float32)).to(a.device)
        a.early_stop(S, losses, e, key[0], SR.EPOCHS + 1)
        b.keep_best(S, losses, e)
        assert device_state(a)[3:] == device_state(b)[3:], e
    assert (a.stopped() == -1).all() and (b.stop_epoch == -1).all()


# ---- frozen means frozen; compaction changes nothing
def trained_engine(pkg):
    case = IR.Case("mixed", 3, "unit", "cut", 0)
    handles = [pkg.from_networkx(g) for g in IR.case_graphs(case)]
    params = IR.case_params(case)
    F, K = params[0]["conv2.weight"].shape
    eng = pkg.engine.InstanceEngine(handles, F, K)
    for g, p in enumerate(params):
        for k, v in eng.views(g).items():
            v.copy_(torch.from_numpy(p[k]))
    return eng


def steps(eng, first_epoch, n):
    out = None
    for e in range(first_epoch, first_epoch + n):
        P, S, losses = eng.train_fwd_bwd(1.0)
        eng.adam_step(3e-2, running_only=True)
        eng.early_stop(S, losses, e, 1e-4, 20)
        out = (P.cpu().numpy(), S.cpu().numpy(), losses.cpu().numpy())
    return out


def graph_state(eng, g, out=None):
    """Everything the engine holds of graph g, as bytes: parameters, moments, best and stop state (and its rows of a
    step's P and S and its loss)."""
    seg = SR.segments(eng.batch.sizes, eng.Fp, eng.K)[g]
    r0, r1 = int(eng.batch.goff_host[g]), int(eng.batch.goff_host[g + 1])
    got = [getattr(eng, k).cpu().numpy()[seg].tobytes() for k in ("flat", "m", "v")]
    got.append(eng.best_S.cpu().numpy()[r0:r1].tobytes())
    got += [getattr(eng, k).cpu().numpy()[g:g + 1].tobytes() for k in ("best_loss", "best_epoch", "prev_loss", "stall",
                                                                       "stop_epoch")]
    if out is not None:
        got += [out[0][r0:r1].tobytes(), out[1][r0:r1].tobytes(), out[2][g:g + 1].tobytes()]
    return got


def test_a_stopped_graph_is_frozen_and_the_others_do_not_notice(pkg):
    free, held = trained_engine(pkg), trained_engine(pkg)
    held.stop_epoch[1] = 0
    before = graph_state(held, 1)
    out_free, out_held = steps(free, 0, 3), steps(held, 0, 3)
    assert free.step_count == held.step_count == 3
    assert graph_state(held, 1) == before
    assert graph_state(free, 1)[:3] != before[:3]                               # (the steps do move a running graph)
    for g in (0, 2, 3):
        assert graph_state(held, g, out_held) == graph_state(free, g, out_free), g
    assert held.stopped().tolist() == [-1, 0, -1, -1] and free.stopped().tolist() == [-1] * 4


def test_compaction_changes_nothing(pkg):
    full = trained_engine(pkg)
    steps(full, 0, 2)
    full.stop_epoch[1] = 0
    sub = full.subset([0, 2, 3])
    assert sub.step_count == 2 and sub.B == 3 and list(sub.batch.sizes) == [full.batch.sizes[g] for g in (0, 2, 3)]
    assert sub.flat.data_ptr() != full.flat.data_ptr()
    for j, g in enumerate((0, 2, 3)):
        assert graph_state(sub, j) == graph_state(full, g), g                   # carried across as it stands
    out_full, out_sub = steps(full, 2, 3), steps(sub, 2, 3)
    assert sub.step_count == full.step_count == 5
    for j, g in enumerate((0, 2, 3)):
        assert graph_state(sub, j, out_sub) == graph_state(full, g, out_full), g
    assert sub.stopped().tolist() == [-1, -1, -1]
    with pytest.raises(ValueError, match="ascend"):
        full.subset([2, 0])


# ---- solve_dataset end to end
# four regular graphs with unit weights (n, degree, seed).  The torch seed, learning rate, patience and epochs of each
# case were chosen on an MI355X so that the stop epochs spread: the test asserts the spread, so a drift is loud.
SPECS = [(40, 5, 41), (30, 4, 42), (66, 5, 43), (52, 6, 44)]
E2E = {"cut": dict(K=3, seed=3, lr=3e-2, patience=5, epochs=40, tolerance=1e-4),             # stops at 30, 32, 38, -
       "expected_cut": dict(K=2, seed=0, lr=3e-2, patience=3, epochs=40, tolerance=1e-2)}    # stops at -, 34, -, 10


def dataset_for(K, specs, N):
    from gcn_max_cut_amd.DataGenerator import graphExtender as GE
    graphs = {i: R.regular_graph(n, d, s) for i, (n, d, s) in enumerate(specs)}
    terms = {i: [int(t) for t in np.random.RandomState(s).permutation(n)[:K]] for i, (n, d, s) in enumerate(specs)}
    ds = GE.process_graphs_from_folder(graphs, terms, N, number_classes=K)
    assert len(ds) == len(specs) and all(it[3] == list(range(K)) for it in ds.values())
    return ds


def comparable(res):
    out = {k: v for k, v in res.items() if k not in ("model", "probabilities")}
    out["probabilities"] = res["probabilities"].numpy().tobytes()
    out["parameters"] = [p.detach().cpu().numpy().tobytes() for p in res["model"]().parameters()]
    return out


@pytest.mark.parametrize("loss", list(E2E))
def test_solve_dataset_with_early_stopping_end_to_end(pkg, loss):
    from gcn_max_cut_amd.Training import TrainingNeural as T
    c = E2E[loss]
    K, F = c["K"], 8
    ds = dataset_for(K, SPECS, 128)
    items = list(ds.values())
    sizes = [it[0].n for it in items]
    cfg = dict(n_nodes=128, hidden_dim=F, number_classes=K, learning_rate=c["lr"], patience=c["patience"],
               tolerance=c["tolerance"])

    def solve(dataset, epochs, burn=0, **kw):
        torch.manual_seed(c["seed"])
        pkg.engine.draw_instance_parameters(sizes[:burn], F, K)     # the draws of the graphs in front of a solo graph
        return T.solve_dataset(dataset, T.TrainingConfig(number_epochs=epochs, **cfg), loss=loss, **kw)

    base = solve(ds, c["epochs"], early_stopping=True, check_every=1)
    stops = [r["stopped_epoch"] for r in base]
    print(f"{loss}: stop epochs {stops}, best epochs {[r['best_epoch'] for r in base]}")
    assert None in stops and len({s for s in stops if s is not None}) >= 2, stops
    want = [comparable(r) for r in base]
    for kw in (dict(check_every=0), dict(check_every=5), dict(check_every=1, max_rows_per_chunk=100),
               dict(check_every=5, compact_fraction=0.0, max_rows_per_chunk=70)):
        assert [comparable(r) for r in solve(ds, c["epochs"], early_stopping=True, **kw)] == want, kw
    for g, (res, item) in enumerate(zip(base, items)):
        n, stop = sizes[g], res["stopped_epoch"]
        ran = c["epochs"] if stop is None else stop + 1
        hist = res["loss_history"]
        assert list(res)[-1] == "stopped_epoch" and len(hist) == ran and len(res["partition"]) == n
        assert SR.replay(hist, c["tolerance"], c["patience"]) == (stop, res["best_loss"], res["best_epoch"])
        if loss == "cut":
            assert all(x == int(x) for x in hist) and res["best_loss"] == -float(res["cut"])
        # the same graph alone, without early stopping, for as many epochs as it ran
        (solo,) = solve({0: item}, ran, burn=g)
        assert "stopped_epoch" not in solo and solo["loss_history"] == hist
        for a, b in zip(res["model"]().parameters(), solo["model"]().parameters()):
            assert torch.equal(a, b)
        if stop is None or solo["best_epoch"] != stop:      # (the early-stopped best comes from the epochs before the stop)
            for key in ("best_loss", "best_epoch", "partition", "cut"):
                assert res[key] == solo[key], (g, key)
        else:
            assert res["best_epoch"] < stop and res["best_loss"] > solo["best_loss"]
        # the probabilities are the forward of the returned parameters
        eng = pkg.engine.InstanceEngine([item[0]], F, K, values=[item[0].edge_values(item[1])])
        named = dict(res["model"]().named_parameters())
        for k, v in eng.views(0).items():
            v.copy_(named[k].detach())
        P, _S, _l = eng.forward(1.0, loss=loss)
        assert torch.equal(P.cpu(), res["probabilities"]), g
