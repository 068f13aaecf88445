"""CPU checks of the evolution stage (include/gcnmaxcut.h, gmc_kway_evolve_f32): the properties the header states "by
construction" on the restatement tests/evolve_ref.py, every status code of the entry point in the documented order
(found before any HIP call: no GPU needed), the exported symbol, the kernels in the gfx950 code object without scratch,
and the new Python arguments' refusals."""
import ctypes as C
import inspect
import json
import os
import subprocess

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import evolve_ref as ER
from tests import util
from tests.test_refine_host import handles_of, loop_graph


def golden_graphs():
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "graphs.json")
    return [R.regular_graph(rec["n"], rec["d"], rec["seed"]) for rec in json.load(open(path))["graphs"]]


def graphs_for(K):
    return golden_graphs()[:2] + [nx.complete_graph(K), nx.complete_graph(K + 1), loop_graph(36, 4, 2),
                                  util.near_regular(65, 3, 65, attrs=False)]


def population(n, K, cands, seed):
    rng = np.random.RandomState(seed)
    A = rng.randint(0, K, (cands, n)).astype(np.int8)
    A[:, :K] = np.arange(K)
    return A


# ---- the restatement's properties ------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", (2, 4, 8))
def test_slot_cuts_never_fall_and_terminals_stay(built, K):
    inv_t, table = AR.schedule(4, t_start=0.6), AR.levels()
    for gi, h in enumerate(handles_of(graphs_for(K))):
        pop0 = population(h.n, K, 6, 10 * K + gi)
        runs = [ER.evolve(h.n, h.rowptr, h.col, h.weight, pop0, K, G, 3, inv_t, table, 5, 100) for G in range(4)]
        assert (runs[0].pop[0] == pop0).all() and not runs[0].written
        for G in (1, 2, 3):
            new, old = runs[G].cut[G & 1], runs[G].cut[(G - 1) & 1]
            assert (new >= old).all(), (K, gi, G)                       # a slot's cut never falls from plane to plane
            assert old.tobytes() == runs[G - 1].cut[(G - 1) & 1].tobytes()   # G generations go through those of G - 1
            assert (runs[G].pop[G & 1][:, :K] == np.arange(K)).all()
            assert (runs[G].cut[G & 1] == AR.cuts_f32(h.rowptr, h.col, h.weight, runs[G].pop[G & 1])).all()
            kept = new == old
            same = (runs[G].pop[G & 1] == runs[G].pop[(G - 1) & 1]).all(axis=1)
            assert (same <= kept).all()                                 # an unchanged member has an unchanged cut
        hist = runs[3].history
        assert hist.shape == (4,) and (np.diff(hist) >= 0).all()
        assert hist[3] == runs[3].best_cut == runs[3].cut[1].max()
        assert (runs[3].best_assign == runs[3].pop[1, runs[3].best_idx]).all()


@pytest.mark.parametrize("K", (2, 5))
def test_no_generation_returns_the_best_of_the_input(built, K):
    h = handles_of([R.regular_graph(40, 5, 1)])[0]
    pop0 = population(h.n, K, 9, K)
    pop0[4] = pop0[7]                                                   # a tie: the first slot wins
    got = ER.evolve(h.n, h.rowptr, h.col, None, pop0, K, 0, 2, AR.schedule(3), AR.levels(), 1, 100)
    cuts = AR.cuts_f32(h.rowptr, h.col, None, pop0)
    best = int(np.argmax(cuts))
    assert got.best_idx == best and got.best_cut == cuts[best] and (got.best_assign == pop0[best]).all()
    assert got.history.tolist() == [cuts[best]] and got.cut[0].tobytes() == cuts.tobytes()
    assert ER.ranking(cuts)[0] == best and ER.ranking([3.0, 5.0, 5.0, 1.0]) == [1, 2, 0, 3]


@pytest.mark.parametrize("K", (2, 3, 8))
def test_a_renamed_parent_gives_the_child_a(built, K):
    n = 80
    rng = np.random.RandomState(K)
    a = rng.randint(0, K, n)
    a[:K] = np.arange(K)
    for perm in (np.roll(np.arange(K), 1), rng.permutation(K), np.arange(K)):
        b = perm[a]
        b[:K] = np.arange(K)                                            # the terminals anchor only K nodes
        pi = ER.align(a.tolist(), b.tolist(), K)
        assert all(pi[int(perm[c])] == c for c in set(a[K:].tolist()))
        assert sorted(pi) == sorted(pi.values()) == list(range(K))      # a bijection, empty classes included
        for slot in (0, 3):
            assert ER.child_of(a, b, K, 12345, slot) == a.tolist()
    # a class a never uses: the matching still ends as a bijection and the child is a
    a2 = np.where(a == K - 1, 0, a)
    a2[:K] = np.arange(K)
    assert ER.child_of(a2, np.roll(np.arange(K), 1)[a2], K, 1, 0)[K:] == a2[K:].tolist()
    # ties: the lowest ca, then the lowest cb
    assert ER.align([0, 1, 0, 1, 0, 1], [0, 1, 0, 1, 1, 0], 2) == {0: 0, 1: 1}    # every count is 1
    assert ER.align([1, 0, 0, 1], [1, 0, 1, 0], 2) == {1: 0, 0: 1}                # the terminals' bytes are not counted


def test_crossover_takes_every_node_from_one_of_aligned_parents(built):
    K, n = 4, 200
    rng = np.random.RandomState(0)
    a, b = rng.randint(0, K, n), rng.randint(0, K, n)
    pi = ER.align(a.tolist(), b.tolist(), K)
    tb = np.asarray([pi[int(c)] for c in b])
    child = np.asarray(ER.child_of(a, b, K, 99, 2))
    assert child[:K].tolist() == list(range(K))
    assert ((child[K:] == a[K:]) | (child[K:] == tb[K:])).all()
    differ = a[K:] != tb[K:]
    took_b = (child[K:] == tb[K:]) & differ
    assert 0.3 < took_b.sum() / differ.sum() < 0.7                      # the top bit of a hash: about half
    assert ER.child_of(a, b, K, 99, 3) != child.tolist() and ER.child_of(a, b, K, 98, 2) != child.tolist()
    # bytes of no class: the other parent's byte; in both parents: a's
    a2, b2 = a.copy(), b.copy()
    a2[10], b2[11], a2[12], b2[12] = K, -1, 100, K
    c2 = ER.child_of(a2, b2, K, 99, 2)
    pi2 = ER.align(a2.tolist(), b2.tolist(), K)
    assert c2[10] == pi2[int(b2[10])] and c2[11] == a2[11] and c2[12] == 100
    assert ER.child_of(a2, None, K, 99, 2) == list(range(K)) + a2[K:].tolist()


def test_one_candidate_and_an_elite_of_one(built):
    K = 3
    h = handles_of([R.regular_graph(40, 5, 1)])[0]
    inv_t, table = AR.schedule(4, t_start=0.6), AR.levels()
    # cands = 1: never a parent b, whatever elite says - the slot is annealed again and again, the better state kept
    pop0 = population(h.n, K, 1, 1)
    for elite in (1, 2, 9):
        assert ER.parent_b([7.0], elite, 123, 0) is None
    one = ER.evolve(h.n, h.rowptr, h.col, None, pop0, K, 3, 1, inv_t, table, 2, 100)
    assert (np.diff(one.history) >= 0).all() and one.best_idx == 0
    assert one.pop.tobytes() == ER.evolve(h.n, h.rowptr, h.col, None, pop0, K, 3, 5, inv_t, table, 2, 100).pop.tobytes()
    # elite = 1: every other slot mates with the best, the best with nobody
    cuts = np.asarray([4.0, 9.0, 9.0, 2.0], np.float32)
    assert [ER.parent_b(cuts, 1, 77, i) for i in range(4)] == [1, None, 1, 1]
    assert [ER.parent_b(cuts, 0, 77, i) for i in range(4)] == [1, None, 1, 1]      # clipped to 1..cands
    # elite >= 2: never oneself, always one of the elite; beyond cands: clipped
    for elite in (2, 3, 4, 50):
        for sel in range(20):
            for i in range(4):
                pb = ER.parent_b(cuts, elite, sel, i)
                assert pb is not None and pb != i and pb in ER.ranking(cuts)[:min(elite, 4)]
    assert [ER.parent_b(cuts, 50, 5, i) for i in range(4)] == [ER.parent_b(cuts, 4, 5, i) for i in range(4)]


def test_the_three_seeds_of_a_generation_differ():
    seen = set()
    for seed in (0, 1, (1 << 64) - 1):
        for g in (1, 2, 1000):
            seen.update(ER.seeds(seed, g))
    assert len(seen) == 27
    assert ER.SELECT != ER.CROSS


# ---- status codes (fake pointers: no call reaches a launch) ----------------------------------------------------------
NULL, SOME = C.c_void_p(None), C.c_void_p(4096)


def mk(hip, **kw):
    return hip.GmcBatch(**{**dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096), **kw})


def test_status_codes_of_the_evolution(built):
    hip = built.hip
    lib = hip.load()
    assert "gmc_kway_evolve_f32" in hip.SYMBOLS

    def f(batch, K=4, order=SOME, cgoff=SOME, cptr=SOME, cands=4, pop=SOME, cut=SOME, generations=3, elite=2,
          inv_temp=SOME, sweeps=10, levels=SOME, descent=10, best_assign=SOME, best_cut=SOME, best_idx=SOME, history=SOME):
        b = None if batch is None else C.byref(batch)
        return lib.gmc_kway_evolve_f32(b, K, order, cgoff, cptr, cands, pop, cut, generations, elite, inv_temp, sweeps,
                                       levels, 7, descent, best_assign, best_cut, best_idx, history, None)
    b = mk(hip)
    assert f(None) == -1
    for name in ("order", "cgoff", "cptr", "pop", "cut", "inv_temp", "levels", "best_assign", "best_cut", "best_idx"):
        assert f(b, **{name: NULL}) == -1, name
    assert f(mk(hip, abi=100)) == -8 and f(mk(hip, abi=100), order=NULL) == -1     # the order: NULL, then the abi word
    for field in ("goff", "rowptr", "lcol"):
        assert f(mk(hip, **{field: None})) == -1, field
        assert f(mk(hip, abi=100, **{field: None})) == -8              # ... then the batch's arrays
    for K in (1, 9, 0, -3):
        assert f(b, K=K) == -3, K
        assert f(b, K=K, cands=0) == -3 and f(b, K=K, generations=-1) == -3   # ... then the class count
        assert f(mk(hip, lcol=None), K=K) == -1
    for kw in (dict(cands=0), dict(sweeps=-1), dict(descent=-1), dict(sweeps=1 << 20), dict(generations=-1),
               dict(generations=1 << 20), dict(elite=0), dict(elite=-2)):
        assert f(b, **kw) == -2, kw                                     # ... then the shape
        assert f(b, inv_temp=NULL, **kw) == -2                          # ... before the tables
        assert f(mk(hip, n_max=3), **kw) == -2
    assert f(mk(hip, B=-1)) == -2
    assert f(mk(hip, n_max=3), inv_temp=NULL) == -1                    # the tables before the graph size
    assert f(mk(hip, n_max=3)) == -6 and f(mk(hip, n_max=4097)) == -6
    assert f(mk(hip, n_max=2), K=3) == -6
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096)
    for K in range(2, 9):
        assert f(empty, K=K) == 0
        assert f(empty, K=K, sweeps=0, inv_temp=NULL, levels=NULL, history=NULL) == 0
        assert f(empty, K=K, generations=0, elite=1000) == 0
        assert f(mk(hip, n_max=K - 1), K=K) == -6
    assert f(empty, generations=(1 << 20) - 1, sweeps=(1 << 20) - 1) == 0
    assert f(empty, elite=0) == -2 and f(empty, K=9) == -3


def test_header_states_the_rule(built):
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcnmaxcut.h")).read()
    assert "int gmc_kway_evolve_f32(" in header
    assert f"0x{ER.SELECT:016X}" in header and f"0x{ER.CROSS:016X}" in header
    assert "generations + 2" in header                                  # the launch count is a closed formula
    assert "GMC_K_COUNT = 19" in header                                 # the new launches reuse tags


def test_every_instantiation_is_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for K in range(2, 9):
        assert sum(f"evolve_generation_kernel<{K}>" in s for s in names) == 1, K
    for kernel in ("evolve_score_kernel", "evolve_pick_kernel"):
        assert sum(kernel in s for s in names) == 1, kernel
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if not ("evolve_" in entry and ".name:" in entry):
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            if "evolve_" not in fields.get(".name", ""):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
            # the static LDS of a generation is the annealing's, inside the allowance anneal_layout.h budgets for
            if "generation" in fields[".name"]:
                assert int(fields[".group_segment_fixed_size"]) <= 288, fields[".name"]
    assert seen == 9


# ---- the Python surface (everything here is decided before a GPU is asked for) ---------------------------------------
def test_new_keywords_and_their_defaults(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    sig = inspect.signature(TN.search_dataset)
    assert sig.parameters["generations"].default == 0                   # nothing new is launched by default
    assert sig.parameters["elite"].default is None
    assert sig.parameters["generation_sweeps"].default == TN.EVOLVE_GENERATION_SWEEPS
    assert [p for p in sig.parameters][:3] == ["model", "processed_graphs", "samples"]
    evo = inspect.signature(TN.kway_evolution).parameters
    assert (evo["generations"].default, evo["generation_sweeps"].default, evo["t_start"].default, evo["t_end"].default,
            evo["seed"].default, evo["max_descent_sweeps"].default, evo["elite"].default) == (
        TN.EVOLVE_GENERATIONS, TN.EVOLVE_GENERATION_SWEEPS, TN.EVOLVE_T_START, 0.15, 0, 100, None)
    # the refusals search_dataset had come first and stay what they were
    for kw in (dict(samples=-1), dict(anneal_sweeps=-1), dict(max_descent_sweeps=-1), dict(candidates=0),
               dict(samples=5, candidates=8), dict(samples=0, candidates=3)):
        with pytest.raises(ValueError) as plain:
            TN.search_dataset(None, {}, **kw)
        with pytest.raises(ValueError) as with_new:
            TN.search_dataset(None, {}, generations=-1, elite=0, **kw)
        assert str(with_new.value) == str(plain.value) and "search_dataset:" not in str(plain.value)
    for kw in (dict(generations=-1), dict(generation_sweeps=-1), dict(elite=0), dict(generations=1 << 20)):
        with pytest.raises(ValueError, match="search_dataset"):
            TN.search_dataset(None, {}, **kw)
    assert TN._evolve_arguments("x", 201, 3, 3, None, 10) == 50 and TN._evolve_arguments("x", 1, 0, 0, None, 0) == 2
    assert TN._evolve_arguments("x", 5, 3, 3, 7, 10) == 7


def test_kway_evolution_refuses_what_it_cannot_take(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = nx.convert_node_labels_to_integers(R.regular_graph(16, 3, 1))
    good = [[i % 4 for i in range(16)]] * 3
    for K in (1, 9, 0):
        with pytest.raises(ValueError, match="number_classes"):
            TN.kway_evolution(good, g, K)
    with pytest.raises(ValueError, match="partitions must be"):
        TN.kway_evolution(good[0], g, 4)
    with pytest.raises(ValueError, match="partitions must be"):
        TN.kway_evolution([row[:-1] for row in good], g, 4)
    with pytest.raises(ValueError, match="outside 0..1"):
        TN.kway_evolution(good, g, 2)
    with pytest.raises(ValueError, match="at least 5 nodes"):
        TN.kway_evolution([[0, 1, 2, 3]], nx.complete_graph(4), 5)
    for kw in (dict(generations=-1), dict(generation_sweeps=-1), dict(max_descent_sweeps=-1), dict(elite=0)):
        with pytest.raises(ValueError, match="kway_evolution"):
            TN.kway_evolution(good, g, 4, **kw)
