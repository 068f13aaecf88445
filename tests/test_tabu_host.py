"""CPU checks of the tabu stage (include/gcnmaxcut.h, gmc_kway_tabu_f32): the properties the header states "by
construction" on the restatement tests/tabu_ref.py, the restatement against brute force on tiny graphs, the status codes
of the entry points (no GPU needed) and gmc_kway_tabu_fits / gmc_kway_tabu_shape at their boundaries."""
import ctypes as C
import itertools
import os

import numpy as np
import pytest

from oracle import ref_dense as R
from tests import tabu_ref as TR
from tests import util
from tests.test_refine_host import gnp_graph, handles_of, loop_graph

NULL, SOME = C.c_void_p(None), C.c_void_p(4096)


def int_weighted(g, seed, signed=False):
    rng = np.random.RandomState(seed)
    for u, v in g.edges():
        g[u][v]["weight"] = int(rng.choice([-1, 1])) if signed else int(rng.randint(1, 6))
    return g


def start(n, K, terminals, seed):
    a = np.random.RandomState(seed).randint(0, K, n).astype(np.int8)
    if terminals:
        a[:K] = np.arange(K)
    return a


CASES = {   # graph, K, terminals, iterations, tenure (base, span, div)
    "regular_k2": (lambda: R.regular_graph(60, 5, 1), 2, False, 200, (3, 0, 10)),
    "regular_k3_t": (lambda: R.regular_graph(60, 5, 2), 3, True, 200, (3, 0, 10)),
    "gnp_k8_t": (lambda: gnp_graph(40, 0.3, 3), 8, True, 150, (0, 0, 0)),
    "int_k4": (lambda: int_weighted(R.regular_graph(50, 6, 4), 4), 4, False, 200, (2, 5, 0)),
    "signed_k2": (lambda: int_weighted(R.regular_graph(50, 6, 5), 5, signed=True), 2, False, 200, (3, 0, 10)),
    "hub_loops_k3": (lambda: loop_graph(45, 4, 6), 3, True, 120, (1, 3, 7)),
    "long_tenure": (lambda: R.regular_graph(20, 3, 7), 2, False, 100, (50, 0, 0)),
}


@pytest.fixture(scope="module", params=sorted(CASES))
def chain(request):
    make, K, t, iters, tenure = CASES[request.param]
    h = handles_of([make()])[0]
    a0 = start(h.n, K, t, 11)
    res = TR.tabu(h.n, h.rowptr, h.col, h.weight, a0, K, t, 2, iters, *tenure, seed=77, trace=True)
    return h, K, t, iters, tenure, a0, res


def test_the_cut_of_the_result_is_the_inputs_plus_best(chain):
    h, K, t, iters, tenure, a0, res = chain
    before, after = TR.cut_f64(h.rowptr, h.col, h.weight, a0), TR.cut_f64(h.rowptr, h.col, h.weight, res.assign)
    assert after == before + float(res.best) and res.best >= 0
    assert 0 <= res.best_it <= iters and 0 <= res.moves <= iters
    if res.best_it == 0:
        assert (res.assign == a0).all() and res.best == 0


def test_the_terminals_never_move(chain):
    h, K, t, iters, tenure, a0, res = chain
    first = K if t else 0
    assert (res.assign[:first] == a0[:first]).all()
    assert all(v >= first for _it, v, _k, _g, _tabu in res.trace)
    assert ((res.assign >= 0) & (res.assign < K)).all()


def test_no_iterations_return_the_input(chain):
    h, K, t, _iters, tenure, a0, _res = chain
    res = TR.tabu(h.n, h.rowptr, h.col, h.weight, a0, K, t, 0, 0, *tenure, seed=77)
    assert (res.assign == a0).all() and res.best_it == 0 and res.moves == 0 and res.best == 0


def test_a_banned_node_moves_only_by_aspiration(chain):
    """Replays the trace: a move recorded as tabu must have had rel + gain > best, every other one a free node."""
    h, K, t, iters, tenure, a0, res = chain
    first = K if t else 0
    until = {}
    rel = best = np.float32(0)
    state = a0.copy()
    for it, v, k, gain, was_tabu in res.trace:
        banned = until.get(v, 0) > it
        assert banned == was_tabu
        if banned:
            assert np.float32(rel + gain) > best
        assert k != state[v]
        state[v] = k
        rel = np.float32(rel + gain)
        _r, tenure_it = TR.draws(77, 2, it, h.n - first, *tenure)
        until[v] = it + 1 + tenure_it
        best = max(best, rel)
    assert len(res.trace) == res.moves and best == res.best


def test_the_snapshot_is_a_local_optimum_when_the_best_came_early(chain):
    h, K, t, iters, tenure, a0, res = chain
    assert res.best_it < iters                                          # (every case above runs past its best state)
    first = K if t else 0
    W = TR.class_sums(h.n, h.rowptr, h.col, h.weight, res.assign, K)
    own = W[np.arange(h.n), res.assign]
    assert (own[first:, None] - W[first:] <= 0).all()


def test_a_chain_depends_on_neither_the_batch_nor_the_candidate_count():
    """The restatement takes one graph and one candidate index: what it returns for candidate 2 of five is what it
    returns for candidate 2 of nine, and a graph's arrays do not change with the batch they are cut from."""
    gs = [R.regular_graph(30, 3, 1), R.regular_graph(40, 5, 2)]
    hs = handles_of(gs)
    A9 = np.stack([start(40, 3, True, s) for s in range(9)])
    nine = TR.tabu_all(40, hs[1].rowptr, hs[1].col, hs[1].weight, A9, 3, True, 80, seed=5)
    five = TR.tabu_all(40, hs[1].rowptr, hs[1].col, hs[1].weight, A9[:5], 3, True, 80, seed=5)
    for x, y in zip(nine, five):
        assert (x[:5] == y).all()
    again = handles_of([gs[1]])[0]
    assert (again.rowptr == hs[1].rowptr).all() and (again.col == hs[1].col).all()
    other = TR.tabu_all(40, hs[1].rowptr, hs[1].col, hs[1].weight, A9[:5], 3, True, 80, seed=6)
    assert (other[0] != five[0]).any()


def test_a_byte_of_no_class_is_inert():
    h = handles_of([R.regular_graph(30, 4, 3)])[0]
    a0 = start(30, 3, True, 1)
    a0[10], a0[20] = 3, -1
    res = TR.tabu(30, h.rowptr, h.col, h.weight, a0, 3, True, 0, 100, seed=1, trace=True)
    assert res.assign[10] == 3 and res.assign[20] == -1 and all(v not in (10, 20) for _i, v, *_r in res.trace)
    assert res.moves == 100


# ---- optimality on tiny graphs -------------------------------------------------------------------------------------
# 24 drawn cases: G(n, 0.5) (an isolated node joined to its successor), n = 6..10 x K = 2, 3 x terminals on / off, and
# four more at n = 9, 10; graph seed 100 + index; every node in class 0 (the terminals in their own); 50 n iterations.
DRAWN = [(n, K, t) for n in range(6, 11) for K in (2, 3) for t in (True, False)] + \
        [(9, 3, True), (9, 3, False), (10, 3, True), (10, 2, False)]
REACHES_THE_OPTIMUM = list(range(24))   # every drawn case does; none was dropped


def brute_force(h, K, first):
    rows = np.repeat(np.arange(h.n), np.diff(h.rowptr))
    tail = np.array(list(itertools.product(range(K), repeat=h.n - first)), np.int8)
    full = np.concatenate([np.tile(np.arange(first, dtype=np.int8), (tail.shape[0], 1)), tail], axis=1)
    return int(((full[:, rows] != full[:, h.col]).sum(axis=1) // 2).max())


@pytest.mark.parametrize("index", REACHES_THE_OPTIMUM)
def test_the_restatement_reaches_the_optimum_of_a_tiny_graph(index):
    assert len(DRAWN) == 24 and len(REACHES_THE_OPTIMUM) >= 20
    n, K, t = DRAWN[index]
    h = handles_of([gnp_graph(n, 0.5, 100 + index)])[0]
    first = K if t else 0
    a0 = np.zeros(n, np.int8)
    a0[:first] = np.arange(first)
    res = TR.tabu(n, h.rowptr, h.col, h.weight, a0, K, t, 0, 50 * n, seed=100 + index)
    assert TR.cut_f64(h.rowptr, h.col, None, res.assign) == brute_force(h, K, first)


# ---- the entry points without a GPU --------------------------------------------------------------------------------
def mk(hip, **kw):
    return hip.GmcBatch(**{**dict(B=2, R=100, n_max=60, nnz_max=420, goff=4096, rowptr=4096, lcol=4096), **kw})


def test_status_codes_of_the_tabu_search(built):
    hip = built.hip
    lib = hip.load()
    assert {"gmc_kway_tabu_f32", "gmc_kway_tabu_fits", "gmc_kway_tabu_shape"} <= set(hip.SYMBOLS)

    def f(batch, K=4, t=1, cands=4, assign=SOME, iterations=10, base=3, span=0, div=10, cut_all=SOME, best_assign=SOME,
          best_cut=SOME, best_idx=SOME, best_iter=SOME, moves=SOME):
        b = None if batch is None else C.byref(batch)
        return lib.gmc_kway_tabu_f32(b, K, t, cands, assign, iterations, base, span, div, 7, cut_all, best_assign,
                                     best_cut, best_idx, best_iter, moves, None)
    b = mk(hip)
    assert f(None) == -1
    for name in ("assign", "cut_all", "best_assign", "best_cut", "best_idx"):
        assert f(b, **{name: NULL}) == -1, name
    assert f(mk(hip, abi=100)) == -8 and f(mk(hip, abi=100), assign=NULL) == -1   # the order: NULL, then the abi word
    for field in ("goff", "rowptr", "lcol"):
        assert f(mk(hip, **{field: None})) == -1, field
        assert f(mk(hip, abi=100, **{field: None})) == -8              # ... then the batch's arrays
    for K in (1, 9, 0, -3):
        assert f(b, K=K) == -3, K
        assert f(b, K=K, cands=0) == -3 and f(b, K=K, iterations=-1) == -3   # ... then the class count
        assert f(mk(hip, lcol=None), K=K) == -1
    for kw in (dict(cands=0), dict(cands=-1), dict(iterations=-1), dict(iterations=-(1 << 31)), dict(base=-1),
               dict(span=-1), dict(div=-1), dict(t=2), dict(t=-1)):
        assert f(b, **kw) == -2, kw                                     # ... then the shape
        assert f(mk(hip, n_max=3), **kw) == -2                          # ... before the graph size
    assert f(mk(hip, B=-1)) == -2
    assert f(mk(hip, n_max=3)) == -6 and f(mk(hip, n_max=4097)) == -6 and f(mk(hip, n_max=0), t=0) == -6
    assert f(mk(hip, n_max=2), K=3) == -6
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096)
    for K in range(2, 9):
        for t in (0, 1):
            assert f(empty, K=K, t=t) == 0
            assert f(empty, K=K, t=t, iterations=0, best_iter=NULL, moves=NULL) == 0
        assert f(mk(hip, n_max=K - 1), K=K) == -6
    assert f(empty, iterations=(1 << 31) - 1, base=(1 << 31) - 1, span=(1 << 31) - 1, div=(1 << 31) - 1) == 0
    assert f(empty, cands=0) == -2 and f(empty, K=9) == -3


@pytest.mark.parametrize("K", (2, 8))
def test_fits_at_its_boundary(built, K):
    """n_pad * (4 K + 6) + 512 <= 160 KiB holds up to GMC_MAX_GRAPH_NODES for every K <= 8, so the node bound decides."""
    hip = built.hip
    lib = hip.load()
    q = lambda **kw: lib.gmc_kway_tabu_fits(C.byref(hip.GmcBatch(**kw)), K)
    assert 4096 * (4 * 8 + 6) + 512 <= 160 * 1024
    assert q(n_max=1) == 1 and q(n_max=4096, nnz_max=1 << 24) == 1 and q(n_max=4097) == 0 and q(n_max=0) == 0
    assert q(n_max=4096, vals=4096) == 1                                # the edges never decide: the global path takes them
    assert lib.gmc_kway_tabu_fits(None, K) == -1 and q(n_max=10, abi=100) == -8
    assert lib.gmc_kway_tabu_fits(C.byref(hip.GmcBatch(n_max=10)), 9) == -3
    assert lib.gmc_kway_tabu_shape(C.byref(hip.GmcBatch(n_max=4097)), K) == -6
    assert lib.gmc_kway_tabu_shape(None, K) == -1


def lds_shape(K, n_max, nnz_max, weighted):
    """The launcher's arithmetic, restated: (chains per workgroup, staged)."""
    cap = 160 * 1024 - 512
    up = lambda x: (x + 15) & ~15
    chain = up(n_max) * (4 * K + 6)
    csr = up((n_max + 1) * 4) + (up(nnz_max * 4) if weighted else 0) + up(nnz_max * 2)
    staged = nnz_max > 0 and chain + csr <= cap
    room = cap - (csr if staged else 0)
    return (4 if 4 * chain <= room else 2 if 2 * chain <= room else 1), int(staged)


def test_shape_is_the_stated_arithmetic(built):
    hip = built.hip
    lib = hip.load()
    seen = set()
    for K in range(2, 9):
        for n_max, nnz_max in ((1, 0), (100, 700), (1000, 7000), (600, 180000), (2000, 14000), (4096, 12288), (4096, 28672),
                               (1100, 7700), (2100, 14700), (800, 38352)):
            for vals in (None, 4096):
                got = lib.gmc_kway_tabu_shape(C.byref(hip.GmcBatch(n_max=n_max, nnz_max=nnz_max, vals=vals)), K)
                slots, staged = lds_shape(K, n_max, nnz_max, vals is not None)
                assert got == (slots | staged << 4), (K, n_max, nnz_max, vals)
                seen.add((slots, staged))
    assert seen == {(s, g) for s in (4, 2, 1) for g in (0, 1)}          # every shape the kernel has is reachable


def test_header_states_the_rule():
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "gcnmaxcut.h")).read()
    for text in ("int gmc_kway_tabu_f32(", "int gmc_kway_tabu_fits(", "int gmc_kway_tabu_shape(", "until[v] <= it",
                 "rel + gain > best", "n_pad * (4 K + 6)"):
        assert text in header, text
    assert "#define GMC_VERSION 200" in header


def test_every_instantiation_is_in_the_code_object(built):
    names = util.kernel_symbols(built.hip.LIB_PATH)
    for K in range(2, 9):
        assert sum(f"tabu_kernel<{K}>" in s for s in names) == 1, K


def test_no_instantiation_uses_scratch(built):
    """The twin of test_balanced_host's: the code object's own notes say that tabu_kernel<2..8> and tabu_pick_kernel
    have no private segment and spill no vector register to memory."""
    import subprocess
    seen = 0
    for co in util.gfx950_code_objects(built.hip.LIB_PATH):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            if "tabu_kernel" not in fields.get(".name", "") and "tabu_pick_kernel" not in fields.get(".name", ""):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0, fields[".name"]
    assert seen == 8                                                    # K = 2..8 and the pick


def test_solve_large_takes_the_keyword_and_refuses_the_stage():
    from gcn_max_cut_amd import maxcut
    with pytest.raises(NotImplementedError, match="tabu"):
        maxcut.solve_large(np.zeros((2, 0), np.int64), num_nodes=10, hidden_dim=8, epochs=1, learning_rate=0.01,
                           tabu_iterations=5)
    with pytest.raises(ValueError, match="tabu_iterations"):
        maxcut.solve_batch(None, hidden_dim=8, epochs=1, learning_rate=0.01, tabu_iterations=-1)
