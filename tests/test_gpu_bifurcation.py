"""GPU tests of the discrete simulated bifurcation of dense instances (include/gcnmaxcut_bifurcation.h, csrc/dense_sb.hip;
DESIGN.md section 41): gmc_dense_sb_f32 against tests/bifurcation_ref.py byte for byte on x, y and the class bytes.

The cases (bifurcation_ref.CASES) cover n = 2, 15, 16, 17, 63, 64, 65, 130; cands = 1, 15, 16, 17, 64, 65, 200; B = 1, 3;
ld = n and ld = n + 5, the padding and the diagonal filled with NaN; steps = 0, 1, 2, 37; +-1, small-integer and
full-mantissa real weights; costs NULL, zeros, integer and real - each value of each axis in at least one case, the tile
edges in both dimensions together, and c0 * dt large enough that both walls are hit within 37 steps (asserted on the CPU by
tests/test_bifurcation_host.py).  The byte-for-byte equality on REAL weights is the header's contract (b): the MFMA's
k-ascending fmaf chain.  Every case runs twice (equal bytes).  Then every tile of the step kernel on the same inputs, one
n = 4096 case (the longest k loop), splitting, a chain moved to another column and another cands, a problem alone against
the same problem third in a batch, the seeded start, Testing.dense_bifurcation, and the doors."""
import numpy as np
import pytest
import torch

from tests import bifurcation_ref as BR
from tests import dense_ref as DR

pytestmark = pytest.mark.gpu
F32 = np.float32
REFS = {}


@pytest.fixture(scope="module")
def pkg(built):
    built.hip.require_gpu()
    yield built
    built.hip.load().gmc_debug_set_sb_tile(0)


def run_sb(pkg, W, cost, x, y, pump, c0, dt):
    """W [B, n, ld] (host), x / y [B * n, cands] -> (x, y, assign) as numpy arrays; the workspace is poisoned."""
    hip, p = pkg.hip, pkg.hip.ptr
    lib = hip.load()
    B, n, ld = W.shape
    cands = x.shape[1]
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    Wd, ct, xd, yd = dev(W), dev(cost), dev(x), dev(y)
    pd = dev(np.asarray(pump, F32)) if len(pump) else None
    assign = torch.full((cands, B * n), -5, dtype=torch.int8, device="cuda")
    need = int(lib.gmc_dense_sb_workspace_bytes(B, n, cands))
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device="cuda")
    assert int(lib.gmc_dense_sb_state_bytes(B, n, cands)) == xd.numel() * 4
    rc = lib.gmc_dense_sb_f32(B, n, p(Wd), ld, p(ct), cands, p(xd), p(yd), p(pd), len(pump), float(c0), float(dt), p(ws),
                              need, p(assign), hip.stream())
    hip.check(rc, "gmc_dense_sb_f32")
    torch.cuda.synchronize()
    return xd.cpu().numpy(), yd.cpu().numpy(), assign.cpu().numpy()


def same(a, b):
    return all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def where(a, b):
    names = ("x", "y", "assign")
    return {k: int((p.view(np.uint8 if p.dtype == np.int8 else np.uint32) != q.view(
        np.uint8 if q.dtype == np.int8 else np.uint32)).sum()) for k, p, q in zip(names, a, b)}


def reference(case):
    if case not in REFS:                                                  # computed once, shared, left unchanged
        i = BR.case_inputs(case)
        REFS[case] = (i, BR.run_batch(i["W"], i["cost"], i["x"], i["y"], i["pump"], i["c0"], i["dt"]))
    return REFS[case]


def args_of(i):
    return i["W"], i["cost"], i["x"], i["y"], i["pump"], i["c0"], i["dt"]


@pytest.mark.parametrize("case", BR.CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_the_device_matches_the_restatement_byte_for_byte(pkg, case):
    i, ref = reference(case)
    got = run_sb(pkg, *args_of(i))
    assert not np.isnan(got[0]).any() and not np.isnan(got[1]).any(), "a NaN of the padding or the diagonal was read"
    assert same(got, run_sb(pkg, *args_of(i))), "two runs differ"
    print(case, "elements that differ", where(got, ref))
    assert same(got, ref), where(got, ref)
    if case[6] == 0:
        assert got[0].tobytes() == i["x"].tobytes() and got[1].tobytes() == i["y"].tobytes()
    if case[5] == "zero":
        assert same(got, run_sb(pkg, i["W"], None, *args_of(i)[2:])), "an all-zero cost is not NULL"


@pytest.mark.parametrize("tile", (1, 2, 3))
def test_every_tile_of_the_step_kernel(pkg, tile):
    """The per-call choice takes 64 x 16 on every small case (its grid stays within 512 workgroups); the other two are
    chosen by the two batches of the next test.  Each tile is forced here on cases with edges in both dimensions, integer
    and real."""
    lib = pkg.hip.load()
    try:
        lib.gmc_debug_set_sb_tile(tile)
        for case in (BR.CASES[3], BR.CASES[6], BR.CASES[8], BR.CASES[9]):
            i, ref = reference(case)
            got = run_sb(pkg, *args_of(i))
            assert same(got, ref), (case, where(got, ref))
    finally:
        lib.gmc_debug_set_sb_tile(0)


@pytest.mark.parametrize("n,B,cands", ((130, 22, 200), (65, 257, 65)))
def test_enough_workgroups_choose_the_larger_tiles(pkg, n, B, cands):
    """B = 22, n = 130, cands = 200: 22 * 3 * 13 = 858 workgroups of 64 x 16, past the 512 up to which that tile is chosen,
    and 264 of 64 x 64: the 32 x 64 tile.  B = 257, n = 65, cands = 65: 257 * 2 * 2 = 1028 workgroups of 64 x 64, past the
    1024 from which that tile is chosen."""
    square = np.stack([DR.weights_of("real" if b % 2 else "int", n, 900 + b) for b in range(B)])
    x = np.concatenate([BR.init(n, cands, 3, 0.1)[0]] * B)
    y = np.concatenate([BR.init(n, cands, 3, 0.1)[1]] * B)
    args = (DR.padded(square, n), DR.cost_of("real", B * n, 4), x, y, BR.pump_table(2), F32(4 * BR.scale_c0(square)), 1.25)
    got = run_sb(pkg, *args)
    ref = BR.run_batch(*args)
    assert same(got, ref), where(got, ref)


def test_the_longest_k_loop(pkg):
    """n = 4096, cands = 16, 3 steps on +-1 weights (64 MB of W): exact sums, so byte for byte."""
    n, cands = 4096, 16
    W = DR.weights_of("pm1", n, 41)[None]
    x, y = BR.init(n, cands, 9, 0.1)
    args = (DR.padded(W, n), None, x, y, BR.pump_table(3), F32(4 * BR.scale_c0(W)), 1.25)
    got = run_sb(pkg, *args)
    ref = BR.run_batch(*args)
    assert same(got, ref), where(got, ref)


def test_splitting_a_run_on_the_device(pkg):
    i, ref = reference(BR.CASES[9])                                       # n = 130, B = 3, real, 37 steps
    W, cost, x, y, pump, c0, dt = args_of(i)
    for cut in (1, 20):
        first = run_sb(pkg, W, cost, x, y, pump[:cut], c0, dt)
        second = run_sb(pkg, W, cost, first[0], first[1], pump[cut:], c0, dt)
        assert same(second, ref), (cut, where(second, ref))


def test_a_chain_moved_to_another_column_and_another_cands(pkg):
    i, ref = reference(BR.CASES[5])                                       # n = 64, cands = 65, real
    W, cost, x, y, pump, c0, dt = args_of(i)
    pick = [64, 3, 17, 40, 0]                                             # five chains, shuffled, in a call of five
    got = run_sb(pkg, W, cost, x[:, pick], y[:, pick], pump, c0, dt)
    assert got[0].tobytes() == ref[0][:, pick].tobytes() and got[1].tobytes() == ref[1][:, pick].tobytes()
    assert got[2].tobytes() == ref[2][pick].tobytes()


def test_a_problem_alone_against_the_same_problem_third_in_a_batch(pkg):
    i, ref = reference(BR.CASES[9])                                       # B = 3
    W, cost, x, y, pump, c0, dt = args_of(i)
    n = W.shape[1]
    alone = run_sb(pkg, W[2:3], cost[2 * n:], x[2 * n:], y[2 * n:], pump, c0, dt)
    assert alone[0].tobytes() == ref[0][2 * n:].tobytes() and alone[1].tobytes() == ref[1][2 * n:].tobytes()
    assert alone[2].tobytes() == ref[2][:, 2 * n:].tobytes()


@pytest.mark.parametrize("n,B,cands", ((2, 1, 1), (65, 3, 17), (130, 1, 200)))
def test_the_seeded_start_against_its_restatement(pkg, n, B, cands):
    hip, p = pkg.hip, pkg.hip.ptr
    x = torch.full((B * n, cands), float("nan"), device="cuda")
    y = torch.full((B * n, cands), float("nan"), device="cuda")
    hip.check(hip.load().gmc_dense_sb_init_f32(B, n, cands, BR.SEED, 0.1, p(x), p(y), hip.stream()), "init")
    torch.cuda.synchronize()
    rx, ry = BR.init(n, cands, BR.SEED, 0.1)
    assert x.cpu().numpy().tobytes() == np.concatenate([rx] * B).tobytes()
    assert y.cpu().numpy().tobytes() == np.concatenate([ry] * B).tobytes()


def recount(W, cost, part):
    return float(BR.objective(DR._square(W), cost, np.asarray(part, np.int64)[None])[0])


def test_dense_bifurcation_and_its_state(pkg):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    W = DR.weights_of("int", 65, 8)
    cost = DR.cost_of("int", 65, 9)
    parts, scores, state = T.dense_bifurcation(W, candidates=17, steps=37, seed=5, node_cost=cost)
    x, y = BR.init(65, 17, 5, 0.1)
    ref = BR.run(W, cost, x, y, BR.pump_table(37), F32(BR.scale_c0(W[None])), 1.25)
    assert state["x"].tobytes() == ref[0].tobytes() and state["y"].tobytes() == ref[1].tobytes()
    assert parts.tobytes() == ref[2].tobytes()
    assert [float(s) for s in scores] == [recount(W, cost, q) for q in parts]
    again, _, state2 = T.dense_bifurcation(W, candidates=17, steps=3, seed=5, node_cost=cost, state=state)
    cont = BR.run(W, cost, ref[0], ref[1], BR.pump_table(3), F32(BR.scale_c0(W[None])), 1.25)
    assert state2["x"].tobytes() == cont[0].tobytes() and again.tobytes() == cont[2].tobytes()


def test_the_doors(pkg):
    from gcn_max_cut_amd import maxcut
    W = DR.weights_of("int", 65, 18)
    cost = DR.cost_of("int", 65, 19)
    plain = maxcut.solve_dense(W, candidates=9, anneal_sweeps=5, seed=3, node_cost=cost)
    zero = maxcut.solve_dense(W, candidates=9, anneal_sweeps=5, seed=3, node_cost=cost, bifurcation_steps=0)
    for k in ("partition", "cut", "node_cost_sum", "moves"):
        assert getattr(plain, k).cpu().numpy().tobytes() == getattr(zero, k).cpu().numpy().tobytes(), k
    res = maxcut.solve_dense(W, candidates=9, anneal_sweeps=5, seed=3, node_cost=cost, bifurcation_steps=30)
    part = res.partition.cpu().numpy()[0]
    assert float(res.cut.item()) == recount(W, cost, part)
    # descent alone after the bifurcation: never below the bifurcation's own best partition
    parts = BR.run(W, cost, *BR.init(65, 9, 3, 0.1), BR.pump_table(30), F32(BR.scale_c0(W[None])), 1.25)[2]
    only = maxcut.solve_dense(W, candidates=9, anneal_sweeps=0, seed=3, node_cost=cost, bifurcation_steps=30)
    assert float(only.cut.item()) >= max(recount(W, cost, q) for q in parts)
    rng = np.random.RandomState(2)
    M = DR.weights_of("int", 33, 21).astype(np.float64)
    lin = rng.randint(-3, 4, 33).astype(np.float64)
    ising = maxcut.solve_ising_dense(M, lin, candidates=9, anneal_sweeps=5, seed=1, bifurcation_steps=30)
    assert float(ising.energy.item()) == DR.ising_energy(M, lin, ising.spins.cpu().numpy()[0])
    assert float(ising.energy.item()) == float(np.triu(M, 1).sum()) - float(ising.result.cut.item())
    qubo = maxcut.solve_qubo_dense(M, lin, candidates=9, anneal_sweeps=5, seed=1, bifurcation_steps=30)
    assert float(qubo.energy.item()) == DR.qubo_energy(M, lin, qubo.x.cpu().numpy()[0])
    assert float(qubo.energy.item()) == -float(qubo.result.cut.item())
    with pytest.raises(ValueError):
        maxcut.solve_dense(W, partitions=np.zeros((2, 65), np.int8), bifurcation_steps=3)
