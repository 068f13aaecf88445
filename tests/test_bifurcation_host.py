"""CPU-side checks of the discrete simulated bifurcation of dense instances (include/gcnmaxcut_bifurcation.h,
csrc/dense_sb.hip, Testing.dense_bifurcation, the bifurcation_* keywords of maxcut.solve_dense / solve_ising_dense /
solve_qubo_dense): the ledger of the fifth header, the two size formulas, the argument checks (all answered before any HIP
call), the Python signatures and refusals, the header's key phrases, the kernels' code object notes (no scratch, no
spills), and on the numpy restatement tests/bifurcation_ref.py alone: splitting, independence, the all-zero cost, that the
walls are hit in both directions on the GPU tests' inputs, the changes of variables against direct energy evaluation, and
the brute-force optimum of drawn small instances."""
import ast
import ctypes as C
import inspect
import os
import subprocess

import numpy as np
import pytest

from tests import bifurcation_ref as BR
from tests import dense_ref as DR
from tests import util
from tests.test_dense_host import brute_force, declarations

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gcnmaxcut_bifurcation.h")
BOUNDS = "test_gpu_bounds_bifurcation"
F32 = np.float32

COVERED = {"gmc_dense_sb_f32": (BOUNDS, "test_dense_sb"), "gmc_dense_sb_init_f32": (BOUNDS, "test_dense_sb_init")}
EXEMPT = {"gmc_dense_sb_state_bytes": "a size query", "gmc_dense_sb_workspace_bytes": "a size query"}


def test_ledger_of_the_fifth_header(built):
    names = declarations(HEADER)
    assert names == sorted(built.hip.BIFURCATION_SYMBOLS) and len(names) == 4
    lib = built.hip.load()
    for name in names:
        assert hasattr(lib, name), name
        assert (name in COVERED) != (name in EXEMPT), name
    assert set(COVERED) | set(EXEMPT) == set(names)
    for other, table in (("gcnmaxcut.h", built.hip.SYMBOLS), ("gcnmaxcut_sdp.h", built.hip.SDP_SYMBOLS),
                         ("gcnmaxcut_temper.h", built.hip.TEMPER_SYMBOLS), ("gcnmaxcut_dense.h", built.hip.DENSE_SYMBOLS)):
        assert not set(names) & set(declarations(os.path.join(ROOT, "include", other))) and not set(names) & set(table)
    for name, (module, fn) in COVERED.items():
        tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
        assert fn in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (name, fn)
    assert "BIFURCATION_SYMBOLS" in open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert '#include "gcnmaxcut_dense.h"' in open(HEADER).read()


def test_the_two_size_formulas(built):
    lib = built.hip.load()
    state, work = lib.gmc_dense_sb_state_bytes, lib.gmc_dense_sb_workspace_bytes
    for B, n, cands in ((1, 2, 1), (3, 130, 5), (16, 1024, 200), (0, 64, 8), (1, 4096, 16), (2, 65, 17)):
        assert state(B, n, cands) == 4 * B * n * cands, (B, n, cands)
        assert work(B, n, cands) == 2 * B * n * ((cands + 15) // 16 * 16) + 16, (B, n, cands)
    for f in (state, work):
        assert f(-1, 64, 8) == 0 and f(1, 1, 8) == 0 and f(1, 4097, 8) == 0 and f(1, 64, 0) == 0


def test_argument_checks_answer_before_any_hip_call(built):
    lib = built.hip.load()
    some = C.c_void_p(4096)          # (never dereferenced: the calls fail first)
    names = ("W", "x", "y", "ws", "assign")
    enough = int(lib.gmc_dense_sb_workspace_bytes(2, 60, 8))

    def call(B=2, n=60, ld=60, cost=some, cands=8, pump=some, steps=5, c0=0.5, dt=1.25, ws_bytes=enough, **ptrs):
        a = dict({k: some for k in names}, **ptrs)
        return lib.gmc_dense_sb_f32(B, n, a["W"], ld, cost, cands, a["x"], a["y"], pump, steps, c0, dt, a["ws"], ws_bytes,
                                    a["assign"], None)

    for name in names:
        assert call(**{name: None}) == -1, name
    assert call(B=-1) == -2 and call(cands=0) == -2 and call(steps=-1) == -2
    assert call(pump=None) == -1 and call(pump=None, steps=0, B=0) == 0
    assert call(n=1) == -6 and call(n=4097, ld=4097) == -6 and call(n=0) == -6
    assert call(ld=59) == -2 and call(ld=61, B=0) == 0
    assert call(ws_bytes=enough - 1) == -5 and call(ws_bytes=0) == -5
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert call(c0=bad) == -2 and call(dt=bad) == -2, bad
    assert call(B=0) == 0 and call(B=0, n=2, ld=2) == 0 and call(B=0, n=4096, ld=4096) == 0
    assert call(cost=None, B=0) == 0 and call(cost=None, ws_bytes=0) == -5
    # NULL before the sizes, the sizes before pump, pump before n, n before ld, ld before the workspace, that before c0 / dt
    assert call(W=None, cands=0) == -1 and call(cands=0, pump=None) == -2 and call(pump=None, n=1) == -1
    assert call(n=1, ld=0) == -6 and call(ld=59, ws_bytes=0) == -2 and call(ws_bytes=0, c0=0.0) == -5
    assert call(c0=0.0, B=0) == -2

    def init(B=2, n=60, cands=8, amplitude=0.1, x=some, y=some):
        return lib.gmc_dense_sb_init_f32(B, n, cands, 7, amplitude, x, y, None)

    assert init(x=None) == -1 and init(y=None) == -1
    assert init(B=-1) == -2 and init(cands=0) == -2 and init(n=1) == -6 and init(n=4097) == -6
    assert init(amplitude=float("nan")) == -2 and init(amplitude=float("inf")) == -2
    assert init(B=0) == 0 and init(B=0, amplitude=0.0) == 0 and init(x=None, cands=0) == -1 and init(cands=0, n=1) == -2


def test_python_signatures_and_refusals(built):
    from gcn_max_cut_amd import maxcut
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    p = inspect.signature(T.dense_bifurcation).parameters
    assert [(k, v.default) for k, v in p.items()] == [
        ("W", inspect.Parameter.empty), ("candidates", 200), ("steps", 1000), ("dt", 1.25), ("c0", None),
        ("amplitude", 0.1), ("seed", 0), ("node_cost", None), ("state", None)]
    tail = [("bifurcation_steps", 0), ("bifurcation_dt", 1.25), ("bifurcation_c0", None)]
    p = inspect.signature(maxcut.solve_dense).parameters
    assert [(k, v.default) for k, v in p.items()][:5] == [
        ("W", inspect.Parameter.empty), ("candidates", 200), ("anneal_sweeps", 100), ("seed", 0), ("node_cost", None)]
    for door, second in ((maxcut.solve_dense, "candidates"), (maxcut.solve_ising_dense, "field"),
                         (maxcut.solve_qubo_dense, "linear")):
        q = inspect.signature(door).parameters
        assert list(q)[1] == second and q["candidates"].default == 200 and q["anneal_sweeps"].default == 100
        assert [(k, v.default) for k, v in q.items()][-3:] == tail
        assert all(q[k].kind is inspect.Parameter.KEYWORD_ONLY for k, _ in tail)
        with pytest.raises(ValueError, match="partitions"):
            door(np.zeros((4, 4), F32), partitions=np.zeros((2, 4), np.int8), bifurcation_steps=3)
        with pytest.raises(ValueError, match="bifurcation_steps"):
            door(np.zeros((4, 4), F32), bifurcation_steps=-1)
    for text in (T.dense_bifurcation.__doc__, maxcut.solve_dense.__doc__, T.bifurcation_pump.__doc__,
                 T.bifurcation_c0.__doc__):
        assert "PROVISIONAL" in text and "section 41" in " ".join(text.split())
    assert T.bifurcation_pump(5).tobytes() == BR.pump_table(5).tobytes() and T.bifurcation_pump(5).dtype == F32
    assert T.bifurcation_pump(1).tolist() == [1.0] and T.bifurcation_pump(0).size == 0
    assert T.bifurcation_pump(1000)[0] == 1 and T.bifurcation_pump(1000)[-1] == 0


def test_the_header_states_the_rule():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("s_u = x_u > 0 ? 1 : (x_u < 0 ? -1 : 0)", "f_v = fmaf(W[v][u], s_u, f_v)", "W[v][v] taken as +0.0f",
                   "g_v = node_cost[v][0] - node_cost[v][1]", "f_v = f_v + g_v",
                   "p = pump[t] * x_v; q = c0 * f_v; r = p + q; m = dt * r; y_v = y_v - m; m2 = dt * y_v; x_v = x_v + m2",
                   "if x_v > 1 then x_v = 1, y_v = 0; if x_v < -1 then x_v = -1, y_v = 0", "x_v < 0 ? 1 : 0",
                   "h = mix64(seed + GOLD * (((uint64)cand << 32 | v) + 1))", "(float)(int32)(h >> 40) - 8388608.0f",
                   "y = amplitude * u", "0x9E3779B97F4A7C15", "never used", "Launches: steps + 1",
                   "plane[r * cands + cand]", "not assumed zeroed", "no atomics, no spin waits", "byte for byte"):
        assert phrase in text, phrase


def test_the_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    assert sum("sb_step_kernel" in s for s in names) == 3
    assert sum("sb_signs_kernel" in s for s in names) == 1 and sum("sb_init_kernel" in s for s in names) == 1
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            name = fields.get(".name", "")
            if not any(k in name for k in ("sb_step_kernel", "sb_signs_kernel", "sb_init_kernel")):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, name
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, name
            # two buffers of two k-major tiles at most: 2 * 16 * (80 + 80) floats
            assert int(fields[".group_segment_fixed_size"]) <= 2 * 16 * 160 * 4, name
    assert seen == 5


# ---- the rule itself, on the restatement ---------------------------------------------------------------------------------
def small(kind="real", cost="real", n=21, cands=6, steps=9):
    W = DR.weights_of(kind, n, 31)
    c = DR.cost_of(cost, n, 32)
    x, y = BR.init(n, cands, BR.SEED, 0.1)
    return W, c, x, y, BR.pump_table(steps), F32(4.0 * BR.scale_c0(W[None])), F32(1.25)


def same(a, b):
    return all(p.tobytes() == q.tobytes() for p, q in zip(a, b))


def test_splitting_a_run_changes_no_byte():
    W, c, x, y, pump, c0, dt = small()
    whole = BR.run(W, c, x, y, pump, c0, dt)
    for cut in (0, 1, 4, 9):
        first = BR.run(W, c, x, y, pump[:cut], c0, dt)
        assert same(whole, BR.run(W, c, first[0], first[1], pump[cut:], c0, dt)), cut
    nothing = BR.run(W, c, x, y, pump[:0], c0, dt)
    assert nothing[0].tobytes() == x.tobytes() and nothing[1].tobytes() == y.tobytes()
    assert (nothing[2] == 0).all()                                        # x = +0 everywhere: class 0


def test_a_chain_depends_on_its_own_problem_index_seed_and_parameters_alone():
    W, c, x, y, pump, c0, dt = small()
    full = BR.run(W, c, x, y, pump, c0, dt)
    assert same(full, BR.run(W, c, x, y, pump, c0, dt))                  # two runs
    xa, ya = BR.init(21, 1, BR.SEED, 0.1, cand_ids=[4])                   # candidate 4 alone, in column 0
    assert xa.tobytes() == x[:, 4:5].tobytes() and ya.tobytes() == y[:, 4:5].tobytes()
    alone = BR.run(W, c, xa, ya, pump, c0, dt)
    assert alone[0].tobytes() == full[0][:, 4:5].tobytes() and alone[1].tobytes() == full[1][:, 4:5].tobytes()
    assert alone[2].tobytes() == full[2][4:5].tobytes()
    # a problem alone and third in a batch
    others = np.stack([DR.weights_of("real", 21, 77), DR.weights_of("int", 21, 78), W])
    cost3 = np.concatenate([DR.cost_of("real", 21, 5), DR.cost_of("int", 21, 6), c])
    bx, by, ba = BR.run_batch(others, cost3, np.tile(x, (3, 1)), np.tile(y, (3, 1)), pump, c0, dt)
    assert bx[42:].tobytes() == full[0].tobytes() and by[42:].tobytes() == full[1].tobytes()
    assert ba[:, 42:].tobytes() == full[2].tobytes()
    # another seed changes the start, other parameters the run
    assert BR.init(21, 6, BR.SEED + 1, 0.1)[1].tobytes() != y.tobytes()
    assert BR.run(W, c, x, y, pump, c0, F32(1.0))[0].tobytes() != full[0].tobytes()


def test_an_all_zero_cost_gives_the_bytes_of_none():
    for kind in ("real", "int"):
        W, _c, x, y, pump, c0, dt = small(kind, None)
        plain = BR.run(W, None, x, y, pump, c0, dt)
        assert same(plain, BR.run(W, DR.cost_of("zero", 21, 0), x, y, pump, c0, dt))
        assert same(plain, BR.run(W, DR.cost_of("negzero", 21, 0), x, y, pump, c0, dt))


def test_the_seeded_start():
    x, y = BR.init(130, 9, BR.SEED, 0.1)
    assert x.tobytes() == np.zeros((130, 9), F32).tobytes()              # +0.0f, not -0.0f
    assert float(np.abs(y).max()) <= 0.1 and y.min() < -0.09 and y.max() > 0.09 and abs(float(y.mean())) < 0.01
    assert len(np.unique(y)) > 1100                                      # no two chains or nodes share a stream
    # the stated operations by hand, for one entry
    h = BR.mix64(BR.SEED + BR.GOLD * (((5 << 32) | 77) + 1))
    want = F32(0.1) * ((F32(h >> 40) - F32(8388608.0)) * F32(2.0 ** -23))
    assert y[77, 5] == want


def test_the_walls_are_hit_in_both_directions_on_the_gpu_tests_inputs():
    """Asserted here so that a GPU test cannot pass without exercising the wall branch: every case of 37 steps hits both
    walls, and the cases together hit them thousands of times."""
    total = {"up": 0, "down": 0}
    for case in BR.CASES:
        i = BR.case_inputs(case)
        tally = {}
        x, y, a = BR.run_batch(i["W"], i["cost"], i["x"], i["y"], i["pump"], i["c0"], i["dt"], tally)
        assert not np.isnan(x).any() and not np.isnan(y).any()
        if case[6] == 37:
            assert tally["up"] > 0 and tally["down"] > 0, (case, tally)
            assert (np.abs(x) == 1).any(), case
        for k in tally:
            total[k] += tally[k]
    print("wall hits", total)
    assert total["up"] > 1000 and total["down"] > 1000


def test_the_cases_cover_every_value_of_every_axis():
    axes = list(zip(*BR.CASES))
    assert set(axes[0]) == {2, 15, 16, 17, 63, 64, 65, 130} and set(axes[1]) == {1, 3}
    assert set(axes[2]) == {1, 15, 16, 17, 64, 65, 200} and set(axes[3]) == {0, 5}
    assert set(axes[4]) == {"pm1", "int", "real"} and {None, "int", "real"} <= set(axes[5])
    assert set(axes[6]) == {0, 1, 2, 37}
    # the tile edges in both dimensions together
    assert {(17, 17), (65, 65), (63, 64), (64, 65)} <= {(c[0], c[2]) for c in BR.CASES}
    assert sum(BR.is_integer_case(c) for c in BR.CASES) >= 5


def test_the_changes_of_variables_against_direct_energy_evaluation():
    """obj(S) = sum_{u<v} W/2 - sum_v (c_v0 + c_v1)/2 - (sum_{u<v} W s_u s_v + sum_v g_v s_v)/2 with s = 1 - 2 S and
    g = c_v0 - c_v1 - the quantity a step descends - and the two doors' maps on top of it."""
    n = 9
    rng = np.random.RandomState(3)
    M = DR.weights_of("int", n, 12).astype(np.float64)
    lin = rng.randint(-3, 4, n).astype(np.float64)
    for door in ("ising", "qubo"):
        w, cost = (DR.ising_to_dense if door == "ising" else DR.qubo_to_dense)(M, lin)
        w64, c64 = w.astype(np.float64), cost.astype(np.float64)
        g = c64[:, 0] - c64[:, 1]
        for bits in rng.randint(0, 2, (40, n)):
            s = 1.0 - 2.0 * bits
            descended = float(np.triu(w64, 1).dot(s).dot(s)) + float(g.dot(s))
            obj = float(BR.objective(w, cost, bits[None])[0])
            assert obj == float(np.triu(w64, 1).sum()) / 2 - float(c64.sum()) / 2 - descended / 2
            assert obj == float(DR.scores(w, cost, bits[None].astype(np.int64))[0])
            if door == "ising":
                assert DR.ising_energy(M, lin, s) == float(np.triu(M, 1).sum()) - obj
            else:
                assert DR.qubo_energy(M, lin, bits) == -obj


# (kind, seed, n) of the drawn instances: complete graphs, couplings +-1 or integers in -3..4 without 0, integer fields /
# linear terms in -3..3 - tests/test_dense_host.py's family.  The restatement runs 32 candidates for 60 steps at dt = 1.25,
# c0 = 0.5 / rms_field and amplitude 0.1 (the defaults of Testing.dense_bifurcation), then a float64 single-move descent,
# and must reach the brute-force optimum of every one: 12 instances, 24 runs.
DRAWN = [(kind, seed, n) for kind in ("pm1", "int") for seed, n in ((0, 6), (1, 8), (2, 10), (3, 11), (4, 12), (5, 16))]
DRAWN_RUN = dict(cands=32, steps=60)


@pytest.mark.parametrize("kind,seed,n", DRAWN)
def test_the_restatement_and_descent_reach_the_brute_force_optimum(kind, seed, n):
    M = DR.weights_of(kind, n, 300 + seed).astype(np.float64)
    lin = np.random.RandomState(400 + seed).randint(-3, 4, n).astype(np.float64)
    up = np.triu(M, 1)
    for door in ("ising", "qubo"):
        if door == "ising":
            w, cost = DR.ising_to_dense(M, lin)
            best = brute_force(n, lambda b: (((1 - 2 * b) @ up) * (1 - 2 * b)).sum(axis=1) + (1 - 2 * b) @ lin)
        else:
            w, cost = DR.qubo_to_dense(M, lin)
            best = brute_force(n, lambda b: ((b @ up) * b).sum(axis=1) + b @ lin)
        x, y = BR.init(n, DRAWN_RUN["cands"], seed, 0.1)
        _x, _y, assign = BR.run(w, cost, x, y, BR.pump_table(DRAWN_RUN["steps"]), BR.scale_c0(w[None]), 1.25)
        S = BR.descend(DR._square(w), cost, assign.astype(np.int64))
        obj = BR.objective(DR._square(w), cost, S)
        state = S[int(np.argmax(obj))]
        energy = DR.ising_energy(M, lin, 1 - 2 * state) if door == "ising" else DR.qubo_energy(M, lin, state)
        before = BR.objective(DR._square(w), cost, assign.astype(np.int64))
        print(kind, seed, n, door, "optimum", best, "reached", energy, "candidates at it", int((obj == obj.max()).sum()),
              "before the descent", int((before == obj.max()).sum()))
        assert energy == best
