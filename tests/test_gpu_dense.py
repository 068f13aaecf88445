"""GPU tests of the annealing of dense two-class instances on cached local fields (include/gcnmaxcut_dense.h,
csrc/dense_anneal.hip): gmc_dense_anneal_f32 against tests/dense_ref.py byte for byte - assign, the
bits of score_all, the pick, snap_sweep, sweeps and moves.

The cases (dense_ref.CASES) cover n = 2, 3, 63, 64, 65, 130, 257 (the lane-stride edges); B = 1, 3; cands = 1, 3, 4, 5, 9
(the four-chains-per-workgroup edge); ld = n and ld > n, the padding and the diagonal filled with NaN (they are not read);
order NULL, a random permutation and the colour order of the graph; unit complete, +-1, integer and full-mantissa real
weights at densities 1, 0.5, 0.1 and 0.03; costs NULL, zeros (the bytes of NULL), -0.0, integer, real and a 1e6 barrier;
anneal_sweeps = 0 (descent only) and max_descent_sweeps = 0 - each value of each axis in at least one case, not their
product.  Every case runs twice (equal bytes) and with the optional outputs NULL.  On the integer cases every output also
equals gmc_kway_refine_anneal_c_f32(K = 2, terminals = 0) on the CSR of the same graphs in the same colour order.  Then:
accepted and refused uphill moves both occur, one n = 4096 case for the size bound, Testing.dense_annealing, and the three
doors, which return the recounted energies of their partitions."""
import numpy as np
import pytest
import torch

from tests import anneal_ref as AR
from tests import dense_ref as DR
from tests.test_gpu_node_cost import Raw, run_anneal

pytestmark = pytest.mark.gpu
F32 = np.float32
GARBAGE = -5
KEYS = ("assign", "score_all", "best_assign", "best_score", "best_idx", "snap", "sweeps", "moves")


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    return built


def run_dense(pkg, W, cost, order, assign, inv_temp, seed, max_descent, optional=True):
    """W [B, n, ld] (host) -> the call's outputs as numpy arrays."""
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    B, n, ld = W.shape
    cands = assign.shape[0]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Wd, ct, od, st = dev(W), dev(cost), dev(order), dev(assign)
    inv_t = dev(np.asarray(inv_temp, F32)) if len(inv_temp) else None
    lv = dev(AR.levels()) if len(inv_temp) else None
    score_all = torch.full((B, cands), float("nan"), device="cuda")
    best_assign = torch.full((B * n,), GARBAGE, dtype=torch.int32, device="cuda")
    best_score = torch.full((B,), float("nan"), device="cuda")
    best_idx = torch.full((B,), GARBAGE, dtype=torch.int32, device="cuda")
    snap, sweeps = (torch.full((B, cands), GARBAGE, dtype=torch.int32, device="cuda") for _ in range(2))
    moves = torch.full((B, cands), GARBAGE, dtype=torch.int64, device="cuda")
    need = int(lib.gmc_dense_anneal_workspace_bytes(B, n, cands))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    extra = (p(snap), p(sweeps), p(moves)) if optional else (None, None, None)
    rc = lib.gmc_dense_anneal_f32(B, n, p(Wd), ld, p(ct), p(od), cands, p(st), p(inv_t), len(inv_temp), p(lv), seed,
                                  max_descent, p(ws), need, p(score_all), p(best_assign), p(best_score), p(best_idx),
                                  *extra, hip.stream())
    hip.check(rc, "gmc_dense_anneal_f32")
    torch.cuda.synchronize()
    assert (ws == 0xA5).all()
    out = dict(assign=st, score_all=score_all, best_assign=best_assign, best_score=best_score, best_idx=best_idx)
    if optional:
        out.update(snap=snap, sweeps=sweeps, moves=moves)
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bytes(a, b, keys=None):
    return all(a[k].tobytes() == b[k].tobytes() for k in (keys or a))


def test_the_cases_cover_every_value_of_every_axis():
    axes = list(zip(*DR.CASES))
    assert set(axes[0]) == {2, 3, 63, 64, 65, 130, 257} and set(axes[1]) == {1, 3} and set(axes[2]) == {1, 3, 4, 5, 9}
    assert 0 in axes[3] and any(p > 0 for p in axes[3]) and set(axes[4]) == {None, "perm", "colour"}
    assert set(axes[5]) == {"unit", "pm1", "int", "real"}
    assert set(axes[7]) == {None, "zero", "negzero", "int", "real", "barrier"}
    assert 0 in axes[8] and 0 in axes[9]
    assert ("unit", 1.0) in {(c[5], c[6]) for c in DR.CASES}
    assert sum(DR.is_integer_case(c) for c in DR.CASES) >= 5


@pytest.mark.parametrize("case", DR.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_device_matches_the_restatement_byte_for_byte(pkg, case):
    n, B, cands, _pad, order_kind, _weights, _density, cost_kind, sweeps, descent = case
    i = DR.case_inputs(case)
    args = (i["W"], i["cost"], i["order"], i["assign"], i["inv_temp"], DR.SEED, descent)
    got = run_dense(pkg, *args)
    assert same_bytes(got, run_dense(pkg, *args)), "two runs differ"
    slim = run_dense(pkg, *args, optional=False)
    assert same_bytes(slim, got, slim.keys()), "the optional outputs change the others"
    if cost_kind == "zero":
        assert same_bytes(got, run_dense(pkg, i["W"], None, *args[2:])), "an all-zero cost is not NULL"
    ref = DR.anneal_batch(i["W"], i["cost"], i["order"], i["assign"], i["inv_temp"], AR.levels(), DR.SEED, descent)
    print(case, "moves", int(ref["moves"].sum()), "uphill taken", ref["uphill"], "refused", ref["refused"])
    for k in KEYS:
        assert got[k].tobytes() == ref[k].tobytes(), (case, k)
    assert not np.isnan(got["score_all"]).any()                      # neither the padding nor the diagonal was read
    if sweeps:
        assert got["moves"].sum() == ref["moves"].sum() > 0
    if sweeps and n >= 63:                                           # uphill moves are both taken and refused
        assert ref["uphill"] > 0 and ref["refused"] > 0 and ref["moves"].sum() > ref["uphill"]
    if not DR.is_integer_case(case):
        return
    # the sparse annealing on the CSR of the same graphs, in the same (colour, id) order
    csrs = [DR.csr_of_dense(i["square"][b]) for b in range(B)]
    batch = Raw(pkg, csrs)
    order = batch.order(2, False)[0].cpu().numpy()[:B * n] - np.repeat(np.arange(B) * n, n)
    assert (order == (np.tile(np.arange(n), B) if i["order"] is None else i["order"])).all()
    ann = run_anneal(pkg, batch, 2, False, i["cost"], i["assign"] & 1, i["inv_temp"], DR.SEED, descent)
    assert (got["assign"] == ann["assign"]).all() and got["score_all"].tobytes() == ann["cut_all"].tobytes()
    assert (got["best_assign"] == ann["best_assign"]).all() and got["best_score"].tobytes() == ann["best_cut"].tobytes()
    assert (got["best_idx"] == ann["best_idx"]).all() and (got["sweeps"] == ann["sweeps"]).all()
    if sweeps:                                                       # (the sparse call writes snap = 0 without annealing too)
        assert (got["snap"] == ann["snap"]).all()


def test_one_problem_of_4096_nodes(pkg):
    n = 4096
    W = DR.weights_of("real", n, 5)[None]
    cost = DR.cost_of("real", n, 6)
    assign = np.random.RandomState(8).randint(0, 2, (1, n)).astype(np.int8)
    inv_temp = AR.schedule(2, scale=DR.rms_field(W))
    got = run_dense(pkg, W, cost, None, assign, inv_temp, DR.SEED, 1)
    ref = DR.anneal_batch(W, cost, None, assign, inv_temp, AR.levels(), DR.SEED, 1)
    for k in KEYS:
        assert got[k].tobytes() == ref[k].tobytes(), k
    assert 0 < ref["moves"].sum() < 2 * n


def test_dense_annealing_of_one_instance(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    n = 40
    W = DR.weights_of("int", n, 3, 0.5)
    parts = np.random.RandomState(1).randint(0, 2, (6, n))
    part, score, info = T.dense_annealing(parts, W, sweeps=10, seed=4)
    part = np.asarray(part)
    assert score == sum(W[u, v] for u in range(n) for v in range(u + 1, n) if part[u] != part[v])
    assert sorted(info) == ["moves", "scores", "snap_sweep", "sweeps"] and score == max(info["scores"])
    inv_temp = T.anneal_schedule(10, scale=DR.rms_field(W[None]))
    ref = DR.anneal(W, None, None, parts.astype(np.int8), inv_temp, AR.levels(), 4, 100)
    assert (part == ref["best_assign"]).all() and info["moves"] == ref["moves"].tolist()
    with pytest.raises(ValueError, match="symmetric"):
        T.dense_annealing(parts, np.triu(W), sweeps=2)
    with pytest.raises(ValueError, match="finite"):
        T.dense_annealing(parts, np.where(W == 3, np.inf, W), sweeps=2)
    with pytest.raises(ValueError, match="permutation"):
        T.dense_annealing(parts, W, sweeps=2, order=np.zeros(n, np.int64))


def test_the_doors_return_the_recounted_energies_of_their_partitions(pkg):
    mc = pkg.maxcut
    B, n = 2, 24
    rng = np.random.RandomState(11)
    M = np.stack([DR.weights_of("int", n, 40 + b) for b in range(B)]).astype(np.float64)
    lin = rng.randint(-3, 4, (B, n)).astype(np.float64)
    run = dict(candidates=6, anneal_sweeps=12, seed=3)

    res = mc.solve_dense(M, **run)
    part = res.partition.cpu().numpy()
    assert part.shape == (B, n) and res.node_cost_sum is None and tuple(res.moves.shape) == (B, 6)
    for b in range(B):
        cut = sum(M[b, u, v] for u in range(n) for v in range(u + 1, n) if part[b, u] != part[b, v])
        assert float(res.cut[b]) == cut
    again = mc.solve_dense(torch.from_numpy(M).cuda(), **run)
    assert again.partition.cpu().numpy().tobytes() == part.tobytes()
    cost = rng.randint(-2, 3, (B, n, 2)).astype(np.float64)
    withc = mc.solve_dense(M, node_cost=cost, **run)
    pc = withc.partition.cpu().numpy()
    sums = np.asarray([cost[b][np.arange(n), pc[b]].sum() for b in range(B)])
    assert np.array_equal(withc.node_cost_sum.cpu().numpy().astype(np.float64), sums)

    ising = mc.solve_ising_dense(M, lin, **run)
    s = ising.spins.cpu().numpy()
    assert set(np.unique(s)) <= {-1, 1} and ising.energy.dtype == torch.float64
    for b in range(B):
        H = DR.ising_energy(M[b], lin[b], s[b])
        assert float(ising.energy[b]) == H == float(np.triu(M[b], 1).sum()) - float(ising.result.cut[b])

    qubo = mc.solve_qubo_dense(M, lin, **run)
    x = qubo.x.cpu().numpy()
    for b in range(B):
        E = DR.qubo_energy(M[b], lin[b], x[b])
        assert float(qubo.energy[b]) == E == -float(qubo.result.cut[b])
    one = mc.solve_qubo_dense(M[0], lin[0], **run)                    # a single [n, n] matrix
    assert tuple(one.x.shape) == (1, n) and float(one.energy[0]) == DR.qubo_energy(M[0], lin[0], one.x.cpu().numpy()[0])
    with pytest.raises(ValueError, match="symmetric"):
        mc.solve_dense(np.triu(M[0]))
    with pytest.raises(ValueError, match="finite"):
        mc.solve_ising_dense(np.where(M[0] == 2, np.nan, M[0]))
