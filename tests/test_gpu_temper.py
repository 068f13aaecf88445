"""GPU tests of parallel tempering over decoded partitions (include/gcnmaxcut_temper.h, csrc/kway_temper.hip; DESIGN.md
section 39): gmc_kway_temper_f32 against tests/temper_ref.py byte for byte - state, best, best_round, rung_out, swaps and
the bits of best_score.

The cases cover K = 2, 3, 8; terminals on and off; cost NULL, all-zero (the bytes of NULL) and real; unit, signed
integer and full-mantissa real weights; rungs 1, 2, 3, 8; cands = rungs, 2 rungs, 24; rounds 0, 1, 2, 5; round_sweeps 1,
3 - each value of each axis in at least one case, not their product.  One mixed batch (temper_ref.mixed_graphs): n = 5,
37, 130, a star with a row of 70 entries, a colour class of 300 nodes, and a graph below `first` that is skipped (its
bytes keep the sentinel); every case runs it twice more, with nnz_max overstated (the global-CSR path: equal bytes) and
a second time (equal bytes).  Then: an n = 4096 cycle at K = 8, property (a) against a device call of
gmc_kway_refine_anneal_c_f32, a graph alone against the same graph inside the batch, and the solver doors."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import anneal_ref as AR
from tests import node_cost_ref as NC
from tests import plain_ref as PR
from tests import temper_ref as TR
from tests.test_gpu_node_cost import Raw, door_batch, run_anneal

pytestmark = pytest.mark.gpu
F32 = np.float32
GARBAGE = -5
SEED = 0x1234567


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def run_temper(pkg, batch, K, t, cost, state, rungs, ladder, rounds, round_sweeps, seed, optional=True):
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    cands = state.shape[0]
    order, cgoff, cptr = batch.order(K, t)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    st, lad, lv = dev(state), dev(np.asarray(ladder, F32)), dev(AR.levels())
    ct = None if cost is None else dev(np.asarray(cost, F32))
    best = torch.full((cands, batch.R), GARBAGE, dtype=torch.int8, device="cuda")
    best_score = torch.full((batch.B, cands), float("nan"), device="cuda")
    ints = [torch.full((batch.B, cands), GARBAGE, dtype=torch.int32, device="cuda") for _ in range(3)]
    best_round, rung, swaps = ints if optional else (None, None, None)
    need = int(lib.gmc_kway_temper_workspace_bytes(batch.ref(), cands))
    assert need == 4 * ((batch.B * cands * 4 + 15) // 16 * 16)
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")     # not zeroed: every word read is written first
    rc = lib.gmc_kway_temper_f32(batch.ref(), K, int(t), p(ct), p(order), p(cgoff), p(cptr), cands, rungs, p(lad), rounds,
                                 round_sweeps, p(lv), seed, p(st), p(best), p(best_score), p(best_round), p(rung), p(swaps),
                                 p(ws), need, hip.stream())
    hip.check(rc, "gmc_kway_temper_f32")
    torch.cuda.synchronize()
    out = dict(state=st, best=best, best_score=best_score)
    if optional:
        out.update(best_round=best_round, rung=rung, swaps=swaps)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bytes(a, b, keys=None):
    return all(a[k].tobytes() == b[k].tobytes() for k in (keys or a))


CASES, cands_of = TR.CASES, TR.cands_of


def test_the_cases_cover_every_value_of_every_axis():
    axes = list(zip(*CASES))
    assert set(axes[0]) == {2, 3, 8} and set(axes[1]) == {False, True} and set(axes[2]) == {None, "zero", "real"}
    assert set(axes[3]) == {"unit", "signed", "real"} and set(axes[4]) == {1, 2, 3, 8}
    assert set(axes[5]) == {"r", "2r", 24} and set(axes[6]) == {0, 1, 2, 5} and set(axes[7]) == {1, 3}


@pytest.mark.parametrize("K,t,cost_kind,weights,rungs,cands,rounds,round_sweeps", CASES, ids=lambda v: str(v))
def test_the_device_matches_the_restatement_byte_for_byte(pkg, K, t, cost_kind, weights, rungs, cands, rounds,
                                                          round_sweeps):
    graphs = TR.mixed_graphs(weights, K, t)
    batch = Raw(pkg, graphs)
    first = PR.first_of(K, t)
    cands = cands_of(cands, rungs)
    assert pkg.hip.load().gmc_refine_anneal_staged(batch.ref()) == 1
    state = TR.start_states(batch.sizes, K, first, cands, 11 * K + rungs)
    state[1 % cands, batch.spans()[1][0] + first + 1] = K + 2          # a byte of no class on a movable node
    cost = TR.cost_of(cost_kind, batch.R, K, 5 + K)
    ladder = TR.ladder(rungs, scale=TR.mean_abs(graphs))
    args = (state, rungs, ladder, rounds, round_sweeps, SEED)
    got = run_temper(pkg, batch, K, t, cost, *args)
    assert same_bytes(got, run_temper(pkg, batch, K, t, cost, *args)), "two runs differ"
    slim = run_temper(pkg, batch, K, t, cost, *args, optional=False)     # the optional outputs as NULL
    assert same_bytes(slim, got, slim.keys())
    if cost_kind == "zero":
        assert same_bytes(got, run_temper(pkg, batch, K, t, None, *args)), "an all-zero cost is not NULL"
    wide = Raw(pkg, graphs)
    wide.c.nnz_max = 1 << 20                                             # overstated: no staged copy fits
    assert pkg.hip.load().gmc_refine_anneal_staged(wide.ref()) == 0
    assert same_bytes(got, run_temper(pkg, wide, K, t, cost, *args)), "the global-CSR path differs"

    table = AR.levels()
    skipped = 0
    for g, ((rp, cl, w), (lo, hi)) in enumerate(zip(batch.csrs, batch.spans())):
        n, what = hi - lo, (K, t, g)
        if TR.skipped(n, K, t):                                          # nothing of it is written
            skipped += 1
            assert (got["state"][:, lo:hi] == state[:, lo:hi]).all() and (got["best"][:, lo:hi] == GARBAGE).all(), what
            assert np.isnan(got["best_score"][g]).all(), what
            assert all((got[k][g] == GARBAGE).all() for k in ("best_round", "rung", "swaps")), what
            continue
        ref = TR.temper(n, rp, cl, w, None if cost is None else cost[lo:hi], state[:, lo:hi], K, first, rungs, ladder,
                        rounds, round_sweeps, table, SEED)
        print(what, "n", n, "swaps", int(ref["swaps"].sum()) // 2, "of", ref["proposals"], "best_round", ref["best_round"])
        assert (got["state"][:, lo:hi] == ref["state"]).all(), what
        assert (got["best"][:, lo:hi] == ref["best"]).all(), what
        assert got["best_score"][g].tobytes() == ref["best_score"].tobytes(), what
        assert (got["best_round"][g] == ref["best_round"]).all(), what
        assert (got["rung"][g] == ref["rung"]).all() and (got["swaps"][g] == ref["swaps"]).all(), what
        assert (np.sort(got["rung"][g].reshape(-1, rungs), axis=1) == np.arange(rungs)).all(), what      # property (b)
    assert skipped == (2 if t and K == 8 else 1 if t else 0)


def cycle(n):
    rowptr = 2 * np.arange(n + 1, dtype=np.int64)
    col = np.stack([(np.arange(n) - 1) % n, (np.arange(n) + 1) % n], axis=1)
    return rowptr, np.sort(col, axis=1).reshape(-1).astype(np.int64), None


def test_a_cycle_of_4096_nodes_at_8_classes(pkg):
    rp, cl, w = cycle(4096)
    batch = Raw(pkg, [(rp, cl, w)])
    state = TR.start_states(batch.sizes, 8, 8, 2, 3)
    ladder = TR.ladder(2)
    got = run_temper(pkg, batch, 8, True, None, state, 2, ladder, 1, 1, SEED)
    ref = TR.temper(4096, rp, cl, w, None, state, 8, 8, 2, ladder, 1, 1, AR.levels(), SEED)
    for k in ("state", "best"):
        assert (got[k] == ref[k]).all(), k
    assert got["best_score"][0].tobytes() == ref["best_score"].tobytes()
    assert (got["best_round"][0] == ref["best_round"]).all() and (got["rung"][0] == [0, 1]).all()


@pytest.mark.parametrize("K,t,weights,cost_kind,rungs", [(2, False, "unit", None, 2), (3, True, "signed", "int", 3),
                                                         (8, True, "real", "real", 6)])
def test_equal_rungs_are_the_annealing(pkg, K, t, weights, cost_kind, rungs):
    """Property (a), against the device's own annealing call."""
    graphs = TR.mixed_graphs(weights, K, t)
    batch = Raw(pkg, graphs)
    first = PR.first_of(K, t)
    state = TR.start_states(batch.sizes, K, first, 6, 21)
    cost = TR.cost_of("real", batch.R, K, 9) if cost_kind else None
    if cost_kind == "int":
        cost = np.round(cost).astype(F32)
    beta = F32(1.0 / (0.4 * TR.mean_abs(graphs)))
    rounds, round_sweeps = 3, 2
    got = run_temper(pkg, batch, K, t, cost, state, rungs, np.full(rungs, beta, F32), rounds, round_sweeps, SEED)
    ann = run_anneal(pkg, batch, K, t, cost, state, np.full(rounds * round_sweeps, beta, F32), SEED, 0)
    live = np.concatenate([np.arange(lo, hi) for lo, hi in batch.spans() if not TR.skipped(hi - lo, K, t)])
    assert (got["best"][:, live] == ann["assign"][:, live]).all()
    assert (ann["snap"] != 0).any()
    if weights != "real" and cost_kind != "real":
        rows = [g for g, (lo, hi) in enumerate(batch.spans()) if not TR.skipped(hi - lo, K, t)]
        assert got["best_score"][rows].tobytes() == ann["cut_all"][rows].tobytes()
    # property (c): never below the input's score
    scored = run_anneal(pkg, batch, K, t, cost, state, [], SEED, 0)
    rows = [g for g, (lo, hi) in enumerate(batch.spans()) if not TR.skipped(hi - lo, K, t)]
    assert (got["best_score"][rows] >= scored["cut_all"][rows]).all()


def test_a_graph_alone_and_inside_a_batch(pkg):
    """Property (d): the place in the batch and the rest of the batch do not matter."""
    K, t, rungs = 3, True, 4
    graphs = TR.mixed_graphs("real", K, t)
    batch = Raw(pkg, graphs)
    g = 3                                                                # the n = 130 graph, not the first of the batch
    lo, hi = batch.spans()[g]
    assert hi - lo == 130 and lo > 0
    state = TR.start_states(batch.sizes, K, K, 8, 31)
    cost = TR.cost_of("real", batch.R, K, 2)
    ladder = TR.ladder(rungs, scale=TR.mean_abs(graphs))
    inside = run_temper(pkg, batch, K, t, cost, state, rungs, ladder, 4, 2, SEED)
    alone = run_temper(pkg, Raw(pkg, [graphs[g]]), K, t, cost[lo:hi], state[:, lo:hi], rungs, ladder, 4, 2, SEED)
    assert (inside["state"][:, lo:hi] == alone["state"]).all() and (inside["best"][:, lo:hi] == alone["best"]).all()
    for k in ("best_score", "best_round", "rung", "swaps"):
        assert inside[k][g].tobytes() == alone[k][0].tobytes(), k


SOLVE = dict(hidden_dim=8, epochs=6, learning_rate=0.05, samples=6, anneal_sweeps=8, seed=3)


def test_solve_batch_with_the_stage(pkg):
    from gcn_max_cut_amd.graph import GraphBatch
    mc = pkg.maxcut
    ei, ptr, w = door_batch()
    batch = GraphBatch.from_edge_index(ei, ptr, edge_weight=w)
    plain = mc.solve_batch(batch, **SOLVE)
    off = mc.solve_batch(batch, tempering_rounds=0, tempering_sweeps=2, tempering_rungs=4, **SOLVE)
    for name in ("partition", "cut", "trained_cut", "rounded_cut"):
        assert getattr(plain, name).cpu().numpy().tobytes() == getattr(off, name).cpu().numpy().tobytes(), name
    assert off.annealed_cut is None
    on = mc.solve_batch(batch, tempering_rounds=3, tempering_sweeps=2, tempering_rungs=4, **SOLVE)
    assert (on.cut >= on.annealed_cut).all()
    assert on.annealed_cut.cpu().numpy().tobytes() == plain.cut.cpu().numpy().tobytes()
    again = mc.solve(ei, ptr, edge_weight=w, tempering_rounds=3, tempering_sweeps=2, tempering_rungs=4, **SOLVE)
    assert again.partition.cpu().numpy().tobytes() == on.partition.cpu().numpy().tobytes()
    part = on.partition.cpu().numpy()
    for g, (lo, hi) in enumerate(zip(ptr[:-1], ptr[1:])):
        _n, rp, cl = PR.ring_with_chords(int(hi - lo), 70 + g)
        ww = PR.integer_weights(int(hi - lo), rp, cl, 20 + g)
        assert float(on.cut[g]) == NC.cut64(rp, cl, ww, part[lo:hi])
    with pytest.raises(ValueError, match="tempering_rungs"):
        mc.solve_batch(batch, tempering_rounds=3, tempering_rungs=16, **SOLVE)       # 8 candidates
    # with pins the stage runs on the contracted batch and every cut is a recount of the lifted partition
    nodes = np.concatenate([[lo, lo + 1] for lo in ptr[:-1]])
    classes = np.tile([0, 1], len(ptr) - 1)
    pinned = mc.solve(ei, ptr, edge_weight=w, fixed=(nodes, classes), tempering_rounds=3, tempering_sweeps=2,
                      tempering_rungs=4, **SOLVE)
    part = pinned.partition.cpu().numpy()
    assert (part[nodes] == classes).all() and (pinned.cut >= pinned.annealed_cut).all()
    for g, (lo, hi) in enumerate(zip(ptr[:-1], ptr[1:])):
        _n, rp, cl = PR.ring_with_chords(int(hi - lo), 70 + g)
        assert float(pinned.cut[g]) == NC.cut64(rp, cl, PR.integer_weights(int(hi - lo), rp, cl, 20 + g), part[lo:hi])


def test_solve_ising_with_the_stage_reaches_the_brute_force_energy(pkg):
    seed, n = NC.DOOR_INSTANCES[4]
    n, edges, quad, lin = NC.drawn_instance(seed, n)
    ei = np.asarray([[i for i, _j in edges] + [j for _i, j in edges], [j for _i, j in edges] + [i for i, _j in edges]], np.int64)
    best, _ = NC.brute_force_min(n, lambda b: NC.ising_energy(edges, quad, lin, [1 - 2 * v for v in b]))
    res = pkg.maxcut.solve_ising(ei, num_nodes=n, coupling=np.concatenate([quad, quad]), field=lin, hidden_dim=8, epochs=10,
                                 learning_rate=0.05, samples=6, anneal_sweeps=4, seed=seed, tempering_rounds=10,
                                 tempering_sweeps=2, tempering_rungs=4)
    s = res.spins.cpu().numpy()
    assert float(res.energy[0]) == NC.ising_energy(edges, quad, lin, s) == best
    assert (res.result.cut >= res.result.annealed_cut).all()


def test_kway_tempering_of_one_graph(pkg):
    import networkx as nx
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    g = nx.random_regular_graph(5, 60, seed=4)
    parts = np.random.RandomState(0).randint(0, 3, (8, 60))
    parts[:, :3] = np.arange(3)
    part, cut, info = T.kway_tempering(parts, g, 3, rounds=6, round_sweeps=2, rungs=4, seed=5)
    assert cut == sum(part[u] != part[v] for u, v in g.edges()) and part[:3] == [0, 1, 2]
    assert sorted(info) == ["best_round", "rung", "scores", "swaps"] and sorted(info["rung"][:4]) == [0, 1, 2, 3]
    assert cut >= max(info["scores"]) and len(info["swaps"]) == 8
    with pytest.raises(ValueError, match="rungs"):
        T.kway_tempering(parts[:6], g, 3, rungs=4)
