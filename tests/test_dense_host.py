"""CPU-side checks of the annealing of dense instances on cached local fields (include/gcnmaxcut_dense.h,
csrc/dense_anneal.hip, Testing.dense_annealing, maxcut.solve_dense / solve_ising_dense / solve_qubo_dense): the ledger of
the fourth header, the workspace formula, the argument checks (all answered before any HIP call), the kernels' code object
notes (no scratch), the properties of the rule on its numpy restatement tests/dense_ref.py - (a) with integer data it is
the sparse annealing's restatement at K = 2 on the same graph given as CSR, (b) an all-zero cost gives the bytes of NULL,
(c) score_all is never below the input's score, (d) a chain depends on its own problem, index, seed and schedule alone -
that uphill moves are both taken and refused on the GPU tests' inputs, the two changes of variables against direct energy
evaluation, and the brute-force optimum of drawn small Ising and QUBO instances."""
import ast
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from tests import anneal_ref as AR
from tests import dense_ref as DR
from tests import node_cost_ref as NC
from tests import util

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "gcnmaxcut_dense.h")
BOUNDS = "test_gpu_bounds_dense"
F32 = np.float32
TABLE = AR.levels()

# the ledger of include/gcnmaxcut_dense.h, as tests/test_temper_host.py keeps the third header's
COVERED = {"gmc_dense_anneal_f32": (BOUNDS, "test_dense_anneal")}
EXEMPT = {"gmc_dense_anneal_workspace_bytes": "a size query"}


def declarations(path=HEADER):
    code = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    return sorted(m.group(1) for m in re.finditer(r"(?:^|\n)\s*(?:int|size_t)\s+(gmc_\w+)\s*\(([^;{]*?)\)\s*;", code))


def test_ledger_of_the_fourth_header(built):
    names = declarations()
    assert names == sorted(built.hip.DENSE_SYMBOLS) and len(names) == 2
    lib = built.hip.load()
    for name in names:
        assert hasattr(lib, name), name
        assert (name in COVERED) != (name in EXEMPT), name
    assert set(COVERED) | set(EXEMPT) == set(names)
    # the other three headers and their tables gain no name
    for other, table in (("gcnmaxcut.h", built.hip.SYMBOLS), ("gcnmaxcut_sdp.h", built.hip.SDP_SYMBOLS),
                         ("gcnmaxcut_temper.h", built.hip.TEMPER_SYMBOLS)):
        assert not set(names) & set(declarations(os.path.join(ROOT, "include", other))) and not set(names) & set(table)
    for name, (module, fn) in COVERED.items():
        tree = ast.parse(open(os.path.join(ROOT, "tests", module + ".py")).read())
        assert fn in {n.name for n in tree.body if isinstance(n, ast.FunctionDef)}, (name, fn)
    entry = open(os.path.join(ROOT, "__graft_entry__.py")).read()
    assert "DENSE_SYMBOLS" in entry


def test_the_workspace_formula(built):
    size = built.hip.load().gmc_dense_anneal_workspace_bytes
    for B, n, cands in ((1, 2, 1), (3, 130, 5), (160, 1024, 200), (0, 64, 8), (1, 4096, 1)):
        assert size(B, n, cands) == 16, (B, n, cands)                # GMC_DENSE_WORKSPACE_MIN: nothing spills from LDS
    assert size(-1, 64, 8) == 0 and size(1, 1, 8) == 0 and size(1, 4097, 8) == 0 and size(1, 64, 0) == 0
    assert "#define GMC_DENSE_WORKSPACE_MIN 16" in open(HEADER).read()


def test_argument_checks_answer_before_any_hip_call(built):
    lib = built.hip.load()
    some = C.c_void_p(4096)          # (never dereferenced: the calls fail first)
    names = ("W", "assign", "score_all", "best_assign", "best_score", "best_idx", "ws")

    def call(B=2, n=60, ld=60, cost=some, order=some, cands=8, inv_temp=some, sweeps=5, levels=some, descent=3,
             ws_bytes=16, snap=some, swp=some, moves=some, **ptrs):
        a = dict({k: some for k in names}, **ptrs)
        return lib.gmc_dense_anneal_f32(B, n, a["W"], ld, cost, order, cands, a["assign"], inv_temp, sweeps, levels, 7,
                                        descent, a["ws"], ws_bytes, a["score_all"], a["best_assign"], a["best_score"],
                                        a["best_idx"], snap, swp, moves, None)

    for name in names:
        assert call(**{name: None}) == -1, name
    assert call(B=-1) == -2 and call(cands=0) == -2 and call(sweeps=-1) == -2 and call(descent=-1) == -2
    assert call(inv_temp=None) == -1 and call(levels=None) == -1
    assert call(inv_temp=None, levels=None, sweeps=0, B=0) == 0                        # no schedule without sweeps
    assert call(n=1) == -6 and call(n=4097, ld=4097) == -6 and call(n=0) == -6
    assert call(sweeps=1 << 20) == -2 and call(sweeps=(1 << 20) - 1, B=0) == 0
    assert call(ld=59) == -2 and call(ld=61, B=0) == 0
    assert call(ws_bytes=15) == -5 and call(ws_bytes=0) == -5
    assert call(B=0) == 0 and call(B=0, n=2, ld=2) == 0 and call(B=0, n=4096, ld=4096) == 0
    # the optional pointers are optional: the same answers without them
    assert call(cost=None, order=None, snap=None, swp=None, moves=None, ws_bytes=15) == -5
    assert call(cost=None, order=None, snap=None, swp=None, moves=None, B=0) == 0
    # NULL comes before the sizes, the sizes before the schedule's pointers, those before n, n before the counter's
    # bound, that before ld, ld before the workspace
    assert call(W=None, cands=0) == -1 and call(cands=0, inv_temp=None) == -2 and call(inv_temp=None, n=1) == -1
    assert call(n=1, sweeps=1 << 20) == -6 and call(sweeps=1 << 20, ld=59, ws_bytes=0) == -2
    assert call(ld=59, ws_bytes=0) == -2 and call(n=4097, ld=5) == -6


def test_python_signatures_and_refusals(built):
    from gcn_max_cut_amd import maxcut
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as T
    p = inspect.signature(T.dense_annealing).parameters
    assert [(k, v.default) for k, v in p.items()][2:] == [
        ("sweeps", 100), ("t_start", 1.5), ("t_end", 0.15), ("seed", 0), ("max_descent_sweeps", 100), ("node_cost", None),
        ("order", None)]
    p = inspect.signature(maxcut.solve_dense).parameters
    assert [(k, v.default) for k, v in p.items()][:5] == [
        ("W", inspect.Parameter.empty), ("candidates", 200), ("anneal_sweeps", 100), ("seed", 0), ("node_cost", None)]
    for door, second in ((maxcut.solve_ising_dense, "field"), (maxcut.solve_qubo_dense, "linear")):
        q = inspect.signature(door).parameters
        assert list(q)[1] == second and q["candidates"].default == 200 and q["anneal_sweeps"].default == 100
    for text in (T.dense_annealing.__doc__, maxcut.solve_dense.__doc__, T.dense_scale.__doc__):
        assert "PROVISIONAL" in text and "section 40" in " ".join(text.split())


def test_the_header_states_the_rule():
    text = " ".join(open(HEADER).read().split())
    for phrase in ("F[v] = W_1(v) - W_0(v)", "delta = c == 0 ? F[v] : -F[v]", "delta < 0 || delta * inv_temp[s] <= levels[h >> 54]",
                   "(uint64)cand << 32 | (uint64)s << 12 | v", "F[u] = F[u] + (c == 0 ? 2.0f * W[v][u] : -(2.0f * W[v][u]))",
                   "x[i] += x[i ^ d]", "0x9E3779B97F4A7C15", "never read", "not the running obj", "NOT the same rounding",
                   "Launches: 2"):
        assert phrase in text, phrase


def test_the_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    assert sum("dense_chains_kernel" in s for s in names) == 1 and sum("dense_pick_kernel" in s for s in names) == 1
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            if "dense_chains_kernel" not in fields.get(".name", "") and "dense_pick_kernel" not in fields.get(".name", ""):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
            # the chains' LDS is dynamic; the static part is the pick's word
            assert int(fields[".group_segment_fixed_size"]) <= 16, fields[".name"]
    assert seen == 2


# ---- the rule itself, on the restatement ---------------------------------------------------------------------------------
SEED = 0x1234567
GRAPHS = (("complete", lambda: DR.weights_of("int", 24, 1)), ("half", lambda: DR.weights_of("pm1", 33, 2, 0.5)),
          ("regular7", lambda: DR.regular_dense(30, 7, 3)))


@pytest.mark.parametrize("name,make", GRAPHS, ids=[g[0] for g in GRAPHS])
@pytest.mark.parametrize("costly", (False, True))
def test_integer_data_give_the_sparse_annealing(name, make, costly):
    """Property (a), against tests/node_cost_ref.py's one-node-at-a-time annealing on the CSR of the non-zero entries in
    the (colour, id) order; (b) and (c) on the way."""
    W = make()
    n = W.shape[0]
    rp, cl, w = DR.csr_of_dense(W)
    if name == "regular7":
        assert (np.diff(rp) == 7).all()
    order = DR.colour_order(n, rp, cl)
    cost = DR.cost_of("int", n, 5) if costly else None
    A = np.random.RandomState(4).randint(0, 2, (5, n)).astype(np.int8)
    inv_temp = AR.schedule(6, scale=DR.rms_field(W[None]))
    got = DR.anneal(W, cost, order, A, inv_temp, TABLE, SEED, 5)
    ref = NC.anneal(n, rp, cl, w, cost, A, 2, 0, inv_temp, TABLE, SEED, 5)
    assert (got["assign"] == ref["assign"]).all() and got["score_all"].tobytes() == ref["cut_all"].tobytes()
    assert (got["snap"] == ref["snap"]).all() and (got["sweeps"] == ref["sweeps"]).all()
    assert got["best_idx"] == ref["best_idx"] and (got["best_assign"] == ref["best_assign"]).all()
    assert got["uphill"] > 0 and got["refused"] > 0
    # descent only
    got0 = DR.anneal(W, cost, order, A, [], TABLE, SEED, 5)
    ref0 = NC.anneal(n, rp, cl, w, cost, A, 2, 0, [], TABLE, SEED, 5)
    assert (got0["assign"] == ref0["assign"]).all() and (got0["sweeps"] == ref0["sweeps"]).all()
    # (c) never below the input's score
    start = DR.scores(DR._square(W), cost, A.astype(np.int64))
    assert (got["score_all"] >= start).all() and (got0["score_all"] >= start).all()
    if not costly:                                                       # (b) zeros are NULL
        zero = DR.anneal(W, DR.cost_of("zero", n, 0), order, A, inv_temp, TABLE, SEED, 5)
        assert all(np.asarray(zero[k]).tobytes() == np.asarray(got[k]).tobytes() for k in got)


def test_a_chain_depends_on_its_own_problem_index_seed_and_schedule_alone():
    """Property (d): a candidate run alone under its own index equals the candidate inside the call; the other candidates'
    states do not matter; another seed or schedule changes it; two runs agree."""
    W = DR.weights_of("real", 40, 7)
    cost = DR.cost_of("real", 40, 8)
    A = np.random.RandomState(2).randint(0, 2, (4, 40)).astype(np.int8)
    inv_temp = AR.schedule(5, scale=DR.rms_field(W[None]))
    full = DR.anneal(W, cost, None, A, inv_temp, TABLE, SEED, 4)
    again = DR.anneal(W, cost, None, A, inv_temp, TABLE, SEED, 4)
    per = ("assign", "score_all", "snap", "sweeps", "moves")
    assert all(full[k].tobytes() == again[k].tobytes() for k in per)
    alone = DR.anneal(W, cost, None, A[2:3], inv_temp, TABLE, SEED, 4, cand_ids=[2])
    assert all(full[k][2:3].tobytes() == alone[k].tobytes() for k in per)
    other = A.copy()
    other[:2] ^= 1
    mixed = DR.anneal(W, cost, None, other, inv_temp, TABLE, SEED, 4)
    assert all(full[k][2:].tobytes() == mixed[k][2:].tobytes() for k in per)
    assert DR.anneal(W, cost, None, A, inv_temp, TABLE, SEED + 1, 4)["assign"].tobytes() != full["assign"].tobytes()
    assert DR.anneal(W, cost, None, A[2:3], inv_temp, TABLE, SEED, 4)["moves"].tobytes() != alone["moves"].tobytes()


def test_uphill_moves_are_taken_and_refused_on_the_gpu_tests_inputs():
    taken = refused = 0
    for case in DR.CASES:
        i = DR.case_inputs(case)
        ref = DR.anneal_batch(i["W"], i["cost"], i["order"], i["assign"], i["inv_temp"], TABLE, DR.SEED, case[9])
        assert not np.isnan(ref["score_all"]).any()
        if case[8] and case[0] >= 63:
            assert ref["uphill"] > 0 and ref["refused"] > 0, case
        taken += ref["uphill"]
        refused += ref["refused"]
    print("uphill moves taken", taken, "refused", refused)
    assert taken > 0 and refused > 0


# ---- the doors' changes of variables ---------------------------------------------------------------------------------------
def test_the_changes_of_variables_against_direct_energy_evaluation():
    n = 9
    rng = np.random.RandomState(3)
    M = DR.weights_of("int", n, 12).astype(np.float64)
    lin = rng.randint(-3, 4, n).astype(np.float64)
    w_i, c_i = DR.ising_to_dense(M, lin)
    w_q, c_q = DR.qubo_to_dense(M, lin)
    assert (w_i == 2 * M).all() and (w_q == M / 2).all() and (c_q[:, 0] == 0).all()
    assert (c_q[:, 1] == lin + M.sum(axis=1) / 2).all()
    for bits in rng.randint(0, 2, (40, n)):
        S = bits[None].astype(np.int64)
        obj_i = float(DR.scores(w_i, c_i, S)[0])
        obj_q = float(DR.scores(w_q, c_q, S)[0])
        assert DR.ising_energy(M, lin, 1 - 2 * bits) == float(np.triu(M, 1).sum()) - obj_i
        assert DR.qubo_energy(M, lin, bits) == -obj_q
    # the row sums' stated order: j ascending in float32
    real = DR.weights_of("real", 70, 5)
    acc = np.zeros(70, F32)
    for j in range(70):
        acc = acc + real[:, j]                                              # (the diagonal is +0: it changes no sum)
    assert DR._row_sums(real).tobytes() == acc.tobytes()


# (kind, seed, n) of the drawn instances: complete graphs, couplings +-1 or integers in -3..4 without 0, integer fields /
# linear terms in -3..3.  The restatement runs with 64 candidates and 50 sweeps and must reach the brute-force optimum of
# every one - none was swapped out, and no sweep count had to be raised on the machine that drew the list.
DRAWN = [(kind, seed, n) for kind in ("pm1", "int") for seed, n in ((0, 6), (1, 8), (2, 10), (3, 11), (4, 12), (5, 12))]
DRAWN_RUN = dict(cands=64, sweeps=50)


def brute_force(n, energy_of_all):
    bits = (np.arange(1 << n)[:, None] >> np.arange(n)) & 1               # all 2^n states
    return float(energy_of_all(bits).min())


@pytest.mark.parametrize("kind,seed,n", DRAWN)
def test_the_restatement_reaches_the_brute_force_optimum(kind, seed, n):
    M = DR.weights_of(kind, n, 300 + seed).astype(np.float64)
    lin = np.random.RandomState(400 + seed).randint(-3, 4, n).astype(np.float64)
    up = np.triu(M, 1)
    A = np.random.RandomState(seed).randint(0, 2, (DRAWN_RUN["cands"], n)).astype(np.int8)
    for door in ("ising", "qubo"):
        if door == "ising":
            w, cost = DR.ising_to_dense(M, lin)
            best = brute_force(n, lambda b: (((1 - 2 * b) @ up) * (1 - 2 * b)).sum(axis=1) + (1 - 2 * b) @ lin)
        else:
            w, cost = DR.qubo_to_dense(M, lin)
            best = brute_force(n, lambda b: ((b @ up) * b).sum(axis=1) + b @ lin)
        inv_temp = AR.schedule(DRAWN_RUN["sweeps"], scale=DR.rms_field(w[None]))
        out = DR.anneal(w, cost, None, A, inv_temp, TABLE, seed, 100)
        state = out["best_assign"]
        energy = DR.ising_energy(M, lin, 1 - 2 * state) if door == "ising" else DR.qubo_energy(M, lin, state)
        print(kind, seed, n, door, "optimum", best, "reached", energy, "candidates at it",
              int((out["score_all"] == out["best_score"]).sum()))
        assert energy == best
