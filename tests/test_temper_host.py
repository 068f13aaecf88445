"""CPU-side checks of parallel tempering over decoded partitions (include/gcnmaxcut_temper.h, csrc/kway_temper.hip,
Testing.kway_tempering, the solver doors' tempering keywords): the ledger of the third header, the argument checks (all
answered before any HIP call), the workspace formula, the Python refusals and defaults, the properties of the rule on
its numpy restatement tests/temper_ref.py - (a) equal rungs are the annealing, (b) the rungs of a ladder copy stay a
permutation, (c) the best score never falls below the input's, (d) a slot depends on its own ladder copy alone - that
accepted and refused exchanges both occur on the GPU tests' inputs, the brute-force optimum of drawn tiny +-1 Ising
instances, and the kernels' code object notes (no scratch)."""
import ast
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import anneal_ref as AR
from tests import node_cost_ref as NC
from tests import plain_ref as PR
from tests import temper_ref as TR
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gcnmaxcut_temper.h")
BOUNDS = "test_gpu_bounds_temper"
F32 = np.float32

# the ledger of include/gcnmaxcut_temper.h, as tests/test_sdp_host.py keeps the second header's
COVERED = {"gmc_kway_temper_f32": (BOUNDS, "test_temper")}
EXEMPT = {"gmc_kway_temper_workspace_bytes": "a size query"}


def declarations(path=HEADER):
    code = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"(?:^|\n)\s*(?:int|size_t)\s+(gmc_\w+)\s*\(([^;{]*?)\)\s*;", code))


def test_ledger_of_the_third_header(built):
    names = declarations()
    assert names == sorted(built.hip.TEMPER_SYMBOLS) and len(names) == 2
    lib = built.hip.load()
    for name in names:
        assert hasattr(lib, name), name
        assert (name in COVERED) != (name in EXEMPT), name
    assert set(COVERED) | set(EXEMPT) == set(names)
    # the other two headers and their tables gain no name
    for other, table in (("gcnmaxcut.h", built.hip.SYMBOLS), ("gcnmaxcut_sdp.h", built.hip.SDP_SYMBOLS)):
        assert not set(names) & set(declarations(os.path.join(ROOT, "include", other))) and not set(names) & set(table)
    for name, (module, fn) in COVERED.items():
        tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
        assert fn in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (name, fn)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "TEMPER_SYMBOLS" in entry


def test_the_workspace_formula(built):
    lib, G = built.hip.load(), built.hip.GmcBatch
    size = lambda B, cands: lib.gmc_kway_temper_workspace_bytes(C.byref(G(B=B, R=10 * B, n_max=10)), cands)
    for B, cands in ((1, 1), (3, 3), (3, 24), (160, 200), (7, 256), (0, 8)):
        assert size(B, cands) == 4 * ((B * cands * 4 + 15) // 16 * 16), (B, cands)
    assert size(1, 1) == 64 and size(3, 3) == 4 * 48
    assert size(3, 0) == 0 and size(-1, 8) == 0 and lib.gmc_kway_temper_workspace_bytes(None, 8) == 0
    assert lib.gmc_kway_temper_workspace_bytes(C.byref(G(abi=100, B=3, R=30)), 8) == 0


def test_argument_checks_answer_before_any_hip_call(built):
    lib = built.hip.load()
    some = C.c_void_p(4096)          # (never dereferenced: the calls fail first)
    G = built.hip.GmcBatch
    good = dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096)
    names = ("order", "cgoff", "cptr", "ladder", "levels", "state", "best", "best_score", "ws")

    def call(batch=None, K=3, terminals=1, cost=None, cands=8, rungs=4, rounds=3, round_sweeps=2, ws_bytes=1 << 20,
             best_round=some, rung_out=some, swaps=some, **ptrs):
        a = dict({k: some for k in names}, **ptrs)
        b = C.byref(batch if batch is not None else G(**good))
        return lib.gmc_kway_temper_f32(b, K, terminals, cost, a["order"], a["cgoff"], a["cptr"], cands, rungs, a["ladder"],
                                       rounds, round_sweeps, a["levels"], 7, a["state"], a["best"], a["best_score"],
                                       best_round, rung_out, swaps, a["ws"], ws_bytes, None)

    assert lib.gmc_kway_temper_f32(None, 3, 1, None, some, some, some, 8, 4, some, 3, 2, some, 7, some, some, some, some,
                                   some, some, some, 1 << 20, None) == -1
    for name in names:
        assert call(**{name: None}) == -1, name
    assert call(batch=G(abi=100, **good)) == -8
    for name in ("goff", "rowptr", "lcol"):
        assert call(batch=G(**dict(good, **{name: None}))) == -1, name
    assert call(K=1) == -3 and call(K=9) == -3
    assert call(rungs=0) == -2 and call(rungs=257, cands=257) == -2 and call(rungs=256, cands=256, ws_bytes=0) == -5
    assert call(cands=0) == -2 and call(cands=9) == -2 and call(cands=6) == -2           # rungs must divide cands
    assert call(rounds=-1) == -2 and call(round_sweeps=0) == -2 and call(round_sweeps=-1, rounds=0) == -2
    assert call(rounds=1 << 10, round_sweeps=1 << 10) == -2 and call(rounds=1 << 16, round_sweeps=1 << 16) == -2
    assert call(rounds=(1 << 10) - 1, round_sweeps=1 << 10, batch=G(**dict(good, B=0, R=0, n_max=0))) == 0
    assert call(terminals=2) == -2 and call(terminals=-1) == -2 and call(batch=G(**dict(good, B=-1))) == -2
    assert call(batch=G(**dict(good, n_max=2))) == -6 and call(batch=G(**dict(good, n_max=2)), terminals=0, ws_bytes=0) == -5
    assert call(batch=G(**dict(good, n_max=0)), terminals=0) == -6 and call(batch=G(**dict(good, n_max=4097))) == -6
    assert call(ws=C.c_void_p(4104)) == -4
    need = 4 * ((2 * 8 * 4 + 15) // 16 * 16)
    assert call(ws_bytes=need - 1) == -5 and call(ws_bytes=0) == -5
    assert call(batch=G(**dict(good, B=0, R=0, n_max=0))) == 0 and call(batch=G(**dict(good, B=0, R=0, n_max=0)), rounds=0, round_sweeps=0) == 0
    # the optional pointers are optional: the same answers without them
    assert call(best_round=None, rung_out=None, swaps=None, ws_bytes=need - 1) == -5
    # NULL comes before the abi word, the abi word before the classes, the classes before the shape, the shape before the
    # size, the size before the alignment, the alignment before the workspace's size
    assert call(batch=G(abi=100, **good), state=None, K=9) == -1 and call(batch=G(abi=100, **good), K=9) == -8
    assert call(K=9, cands=9) == -3 and call(cands=9, batch=G(**dict(good, n_max=2))) == -2
    assert call(batch=G(**dict(good, n_max=2)), ws=C.c_void_p(4104)) == -6
    assert call(ws=C.c_void_p(4104), ws_bytes=0) == -4


def test_python_refusals_and_defaults(built):
    from gcn_max_cut_amd import maxcut
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    doors = (maxcut.solve, maxcut.solve_batch, maxcut.solve_large, maxcut.solve_large_batch, maxcut.solve_ising,
             maxcut.solve_qubo)
    for door in doors:
        p = inspect.signature(door).parameters
        assert (p["tempering_rounds"].default, p["tempering_sweeps"].default, p["tempering_rungs"].default) == (0, 4, 8)
        assert all(p[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("tempering_rounds", "tempering_sweeps",
                                                                         "tempering_rungs")), door.__name__
    assert inspect.signature(maxcut.solve) == inspect.signature(maxcut.solve_large)
    assert inspect.signature(maxcut.solve_batch) == inspect.signature(maxcut.solve_large_batch)
    kt = inspect.signature(T.kway_tempering).parameters
    assert [(k, v.default) for k, v in kt.items()][3:] == [
        ("rounds", 50), ("round_sweeps", 4), ("rungs", 8), ("t_hot", 1.5), ("t_cold", 0.15), ("seed", 0),
        ("max_descent_sweeps", 100), ("terminals", True), ("node_cost", None)]
    ei, kw = np.zeros((2, 0), np.int64), dict(hidden_dim=8, epochs=1, learning_rate=0.01)
    for door in (maxcut.solve_large, ):
        with pytest.raises(NotImplementedError, match="tempering"):
            door(ei, num_nodes=10, tempering_rounds=5, **kw)
    with pytest.raises(NotImplementedError, match="tempering"):
        maxcut.solve_large_batch(None, tempering_rounds=5, **kw)
    for door in (maxcut.solve, maxcut.solve_ising, maxcut.solve_qubo):
        with pytest.raises(NotImplementedError, match="tempering_rounds.*tabu_iterations"):
            door(ei, num_nodes=10, tempering_rounds=5, tabu_iterations=5, **kw)
        with pytest.raises(NotImplementedError, match="tempering_rounds.*class_sizes"):
            door(ei, num_nodes=10, tempering_rounds=5, class_sizes="balanced", **kw)
        with pytest.raises(ValueError, match="tempering_rungs"):
            door(ei, num_nodes=10, tempering_rounds=5, samples=5, **kw)                   # 7 candidates, 8 rungs
        with pytest.raises(ValueError, match="tempering_rounds"):
            door(ei, num_nodes=10, tempering_rounds=-1, **kw)
        with pytest.raises(ValueError, match="tempering_sweeps"):
            door(ei, num_nodes=10, tempering_rounds=5, tempering_sweeps=0, **kw)
    with pytest.raises(NotImplementedError, match="tempering_rounds.*tabu_iterations"):
        maxcut.solve_batch(None, tempering_rounds=5, tabu_iterations=5, **kw)
    # the ladder: geometric, float32, hottest first, in units of `scale`
    lad = T.temper_ladder(8, 1.5, 0.15, 2.0)
    assert lad.dtype == np.float32 and lad.tobytes() == TR.ladder(8, 1.5, 0.15, 2.0).tobytes()
    assert lad[0] == F32(1 / 3.0) and np.isclose(lad[-1], 1 / 0.3) and (np.diff(lad) > 0).all()
    assert np.allclose(lad[1:] / lad[:-1], 10 ** (1 / 7)) and T.temper_ladder(1).tolist() == [F32(1 / 1.5)]
    for bad in (0, 257):
        with pytest.raises(ValueError, match="rungs"):
            T.temper_ladder(bad)
    with pytest.raises(ValueError, match="rungs"):
        T._temper_arguments("x", 12, 5, 4, 8)
    with pytest.raises(ValueError, match="round_sweeps"):
        T._temper_arguments("x", 8, 5, 0, 8)
    with pytest.raises(ValueError, match="2\\^20"):
        T._temper_arguments("x", 8, 1 << 10, 1 << 10, 8)
    T._temper_arguments("x", 8, 0, 0, 8)


# ---- the rule itself, on the restatement ---------------------------------------------------------------------------------
TABLE = AR.levels()
SEED = 0x1234567          # tests/test_gpu_temper.py's


def live_graphs(weights, K, t):
    lo = 0
    for rp, cl, w in TR.mixed_graphs(weights, K, t):
        n = len(rp) - 1
        if not TR.skipped(n, K, t):
            yield lo, n, rp, cl, w
        lo += n


@pytest.mark.parametrize("K,t,weights,costly,rungs", [(2, False, "unit", False, 2), (3, True, "signed", True, 3),
                                                      (8, True, "real", True, 6), (3, False, "real", False, 1)])
def test_equal_rungs_are_the_annealing(K, t, weights, costly, rungs):
    """Property (a), against tests/node_cost_ref.py's one-node-at-a-time annealing; and the all-candidates score against
    its one-candidate form."""
    first = PR.first_of(K, t)
    graphs = TR.mixed_graphs(weights, K, t)
    R = sum(len(rp) - 1 for rp, _cl, _w in graphs)
    state = TR.start_states([len(rp) - 1 for rp, _cl, _w in graphs], K, first, 6, 21)
    cost = TR.cost_of("real", R, K, 9) if costly else None
    beta = F32(1.0 / (0.4 * TR.mean_abs(graphs)))
    for lo, n, rp, cl, w in list(live_graphs(weights, K, t))[:4]:          # (the 302-node graph: the GPU test has it)
        cg = None if cost is None else cost[lo:lo + n]
        st = state[:, lo:lo + n]
        got = TR.temper(n, rp, cl, w, cg, st, K, first, rungs, np.full(rungs, beta, F32), 3, 2, TABLE, SEED)
        ref = NC.anneal(n, rp, cl, w, cg, st, K, first, np.full(6, beta, F32), TABLE, SEED, 0)
        assert (got["best"] == ref["assign"]).all(), (K, n)
        assert got["best_score"].tobytes() == ref["cut_all"].tobytes(), (K, n)
        assert (got["best_round"] == (np.maximum(ref["snap"], 1) - 1) // 2).all()
        one = np.asarray([NC.score(n, rp, cl, w, cg, row, K) for row in st], F32)
        assert TR.scores(n, rp, cl, w, cg, st, K).tobytes() == one.tobytes()
        assert (got["best_score"] >= one).all()                              # property (c)


def test_rungs_stay_a_permutation_and_both_branches_are_taken():
    """Property (b) after every round, (c), and over the cases of tests/test_gpu_temper.py: 0 < swaps < proposals."""
    swaps = proposals = 0
    for K, t, cost_kind, weights, rungs, cands, rounds, round_sweeps in TR.CASES:
        first, cands = PR.first_of(K, t), TR.cands_of(cands, rungs)
        graphs = TR.mixed_graphs(weights, K, t)
        sizes = [len(rp) - 1 for rp, _cl, _w in graphs]
        state = TR.start_states(sizes, K, first, cands, 11 * K + rungs)
        cost = TR.cost_of(cost_kind, sum(sizes), K, 5 + K)
        ladder = TR.ladder(rungs, scale=TR.mean_abs(graphs))
        for lo, n, rp, cl, w in live_graphs(weights, K, t):
            if n > 200:
                continue
            trace = []
            cg = None if cost is None else cost[lo:lo + n]
            out = TR.temper(n, rp, cl, w, cg, state[:, lo:lo + n], K, first, rungs, ladder, rounds, round_sweeps, TABLE,
                            SEED, trace)
            assert len(trace) == rounds
            for rung in trace + [out["rung"]]:
                assert (np.sort(rung.reshape(-1, rungs), axis=1) == np.arange(rungs)).all()
            assert (out["best_score"] >= TR.scores(n, rp, cl, w, cg, state[:, lo:lo + n], K)).all()
            assert out["swaps"].sum() % 2 == 0 and out["swaps"].max(initial=0) <= max(rounds - 1, 0)
            swaps += int(out["swaps"].sum()) // 2
            proposals += out["proposals"]
    print("exchanges accepted", swaps, "of", proposals)
    assert 0 < swaps < proposals


def test_a_slot_depends_on_its_own_ladder_copy_alone():
    """Property (d) on the restatement: the second ladder copy run as slots 4..7 of 8 and, the hash's copy index and
    candidate ids aside, nothing of the first copy enters - dropping copy 0's states changes copy 1 not at all when the
    ids are kept; and two runs agree."""
    K, t, rungs = 3, True, 4
    _lo, n, rp, cl, w = list(live_graphs("real", K, t))[2]
    state = TR.start_states([n], K, K, 8, 31)
    ladder = TR.ladder(rungs, scale=1.1)
    a = TR.temper(n, rp, cl, w, None, state, K, K, rungs, ladder, 4, 2, TABLE, SEED)
    b = TR.temper(n, rp, cl, w, None, state, K, K, rungs, ladder, 4, 2, TABLE, SEED)
    assert all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in a)
    other = state.copy()
    other[:4, K:] = (other[:4, K:] + 1) % K                                  # another copy 0
    c = TR.temper(n, rp, cl, w, None, other, K, K, rungs, ladder, 4, 2, TABLE, SEED)
    for k in ("state", "best", "best_score", "best_round", "rung", "swaps"):
        assert a[k][4:].tobytes() == c[k][4:].tobytes(), k


# (seed, n) of the drawn instances: a ring with chords, couplings +-1, no field; chosen on the CPU so that every one of
# them reaches its brute-force optimum with the parameters below
ISING = ((0, 8), (1, 10), (2, 12), (3, 13), (4, 14), (5, 14))
ISING_RUN = dict(cands=8, rungs=4, rounds=10, round_sweeps=2)


def ising_instance(seed, n):
    _n, rp, cl = PR.ring_with_chords(n, 400 + seed)
    edges = [(v, int(u)) for v in range(n) for u in cl[rp[v]:rp[v + 1]] if v < u]
    J = np.random.RandomState(500 + seed).choice([-1.0, 1.0], size=len(edges))
    return edges, J


@pytest.mark.parametrize("seed,n", ISING)
def test_the_restatement_reaches_the_brute_force_optimum_of_tiny_spin_glasses(seed, n):
    edges, J = ising_instance(seed, n)
    spins = 1 - 2 * ((np.arange(1 << n)[:, None] >> np.arange(n)) & 1)         # all 2^n states
    i, j = np.asarray(edges).T
    optimum = float((spins[:, i] * spins[:, j] * J).sum(axis=1).min())
    rp, cl, w, _cost = NC.ising_to_maxcut(n, edges, J, np.zeros(n))
    run = ISING_RUN
    state = np.random.RandomState(seed).randint(0, 2, (run["cands"], n)).astype(np.int8)
    out = TR.temper(n, rp, cl, w, None, state, 2, 0, run["rungs"], TR.ladder(run["rungs"], scale=2.0), run["rounds"],
                    run["round_sweeps"], TABLE, seed)
    energy = float(J.sum()) - float(out["best_score"].max())                    # H(s) = sum J - cut (w = 2 J)
    print(seed, n, "optimum", optimum, "reached", energy, "best_round", out["best_round"])
    assert energy == optimum


def test_the_header_states_the_rule():
    text = " ".join(open(HEADER).read().split())
    assert f"0x{TR.TAG:016X}ULL" in text and "0x9E3779B97F4A7C15" in text
    for phrase in ("(ladder[p + 1] - ladder[p]) * (x_hi - x_lo)", "d < 0 || d <= levels[h >> 54]", "(uint64)t << 40",
                   "NOT assumed", "(a) Equality with the annealing", "permutation of 0 .. rungs - 1"):
        assert phrase in text, phrase


def test_every_instantiation_is_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for K in range(2, 9):
        for cost in ("false", "true"):
            assert sum(f"temper_round_kernel<{K}, {cost}>" in s for s in names) == 1, (K, cost)
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if not ("temper" in entry and ".name:" in entry):
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            if "temper" not in fields.get(".name", ""):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
            # the static LDS of a round is the annealing's, inside the allowance anneal_layout.h budgets for
            assert int(fields[".group_segment_fixed_size"]) <= 288, fields[".name"]
    assert seen == 14
