"""CPU checks of the sampler and the annealing for graphs beyond 4096 nodes (include/gcnmaxcut.h:
gmc_large_search_workspace_bytes, gmc_large_sample_seeded_f32, gmc_large_anneal_f32): the vectorised restatement of
tests/large_search_ref.py against its one-node-at-a-time definition and against tests/kway_search_ref.py, the two
counter layouts, the conditions the GPU cases must meet, every status code of the entry points in the documented order
(found before any HIP call: no GPU needed), the kernels' metadata in the gfx950 code object, and the Python refusals."""
import ctypes as C
import subprocess

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import kway_search_ref as KS
from tests import large_ref as LR
from tests import large_search_ref as LS
from tests import seeded_ref as SR
from tests import util
from tests.test_anneal_host import dyadic_weights
from tests.test_kway_search_host import KS_SMALL
from tests.test_refine_host import handles_of, loop_graph

SMALL = {
    "nK": lambda K: (nx.complete_graph(K), None),
    "nK1": lambda K: (nx.complete_graph(K + 1), None),
    "regular": lambda K: (R.regular_graph(34, 5, 1), None),
    "self_loops": lambda K: (loop_graph(36, 4, 2), None),
    "dyadic": lambda K: (R.regular_graph(30, 6, 3), 4),
}


def start(h, K, cands, seed):
    A = np.random.RandomState(seed).randint(0, K, (cands, h.n)).astype(np.int8)
    if h.n > 12:
        A[1, 9] = K                                                    # bytes of no class: count for nothing, move
        A[2, 11] = -1
    return A


@pytest.mark.parametrize("K", (2, 3, 8))
@pytest.mark.parametrize("case", sorted(SMALL))
def test_vectorised_restatement_equals_the_sequential_definition(case, K):
    g, wseed = SMALL[case](K)
    h = handles_of([g])[0]
    w = None if wseed is None else dyadic_weights(h, wseed)
    A = start(h, K, 4, len(case) + K)
    inv_t, table = LS.schedule(8), AR.levels()
    for wide_layout in (False, True):
        for max_descent in (0, 100):
            out, snap, sweeps = LS.anneal(h.n, h.rowptr, h.col, w, A, K, inv_t, table, 9, max_descent,
                                          wide_layout=wide_layout)
            for i in range(A.shape[0]):
                a, sn, sw = LS.sequential(h.n, h.rowptr, h.col, w, A[i].tolist(), K, inv_t, table, 9, max_descent,
                                          cand=i, wide_layout=wide_layout)
                assert out[i].tolist() == a and snap[i] == sn and sweeps[i] == sw, (case, K, i, wide_layout)
            assert (out[:, :K] == A[:, :K]).all()
    out2, snap2, _ = LS.anneal(h.n, h.rowptr, h.col, w, A[2:], K, inv_t, table, 9, 100, cand_ids=[2, 3])
    out, snap, _ = LS.anneal(h.n, h.rowptr, h.col, w, A, K, inv_t, table, 9, 100)
    assert (out2 == out[2:]).all() and (snap2 == snap[2:]).all()


@pytest.mark.parametrize("K", (2, 4, 8))
@pytest.mark.parametrize("case", sorted(KS_SMALL))
def test_up_to_4096_nodes_the_restatement_is_kway_search_refs(case, K):
    """The old counter layout: byte for byte tests/kway_search_ref.py on every graph of its own cases."""
    g, wseed = KS_SMALL[case](K)
    h = handles_of([g])[0]
    w = None if wseed is None else dyadic_weights(h, wseed)
    A = start(h, K, 5, len(case) + K)
    inv_t, table = AR.schedule(12), AR.levels()
    assert not LS.wide(h.n)
    for max_descent in (0, 100):
        got = LS.anneal(h.n, h.rowptr, h.col, w, A, K, inv_t, table, 9, max_descent)
        want = KS.anneal(h.n, h.rowptr, h.col, w, A, K, inv_t, table, 9, max_descent)
        for a, b in zip(got, want):
            assert a.tobytes() == np.asarray(b, a.dtype).tobytes()
    plain, snap0, sw0 = LS.anneal(h.n, h.rowptr, h.col, w, A, K, inv_t[:0], table, 9, 100)
    ref, ref_sw = KS.refine(h.n, h.rowptr, h.col, w, A, K, 100)
    assert (plain == ref).all() and (sw0 == ref_sw).all() and (snap0 == 0).all()
    P = np.random.RandomState(K).dirichlet(np.ones(K), h.n).astype(np.float32)
    key = SR.keys(5, [2])[0]
    got, want = LS.sample(h.n, h.rowptr, h.col, w, P, key, 7), KS.sample(h, P, key, 7) if w is None else None
    if want is not None:
        for k in want:
            assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


def test_the_counter_layouts():
    assert not LS.wide(4096) and LS.wide(4097)
    assert LS.counter(3, 5, 7, False) == (3 << 32) | (5 << 12) | 7 and LS.counter(3, 5, 7, True) == (3 << 40) | (5 << 20) | 7
    # the old layout's collision beyond 4096 nodes, and none in the new one up to 2^20 nodes and sweeps, 2^24 candidates
    assert LS.counter(0, 0, 4096 + 9, False) == LS.counter(0, 1, 9, False)
    assert LS.counter(0, 0, 4096 + 9, True) != LS.counter(0, 1, 9, True)
    assert LS.counter((1 << 24) - 1, (1 << 20) - 1, (1 << 20) - 1, True) == (1 << 64) - 1
    nodes = np.asarray([0, 5, 4095, 4096, (1 << 20) - 1])
    for layout in (False, True):
        got = LS.level_indices(12345, [0, 3, 70000], 6, nodes, layout)
        want = [[LS.level_index(12345, c, 6, int(v), layout) for v in nodes] for c in (0, 3, 70000)]
        assert got.tolist() == want
    assert (LS.level_indices(9, [0, 2], 4, nodes[:3], False) == AR.level_indices(9, [0, 2], 4, nodes[:3])).all()
    assert LS.level_index(9, 2, 4, 77, False) == AR.level_index(9, 2, 4, 77)


def test_at_4097_nodes_the_old_layout_gives_other_bytes():
    """The GPU test of the 4097-node cases cannot pass on the one-workgroup kernel's counter."""
    for name in ("n4097_K2", "n4097_K8"):
        K, n, rowptr, col, w, A, inv_t, max_descent, groups = LS.big_case(name)
        ref = LS.big_reference(name)
        old = LS.anneal(n, rowptr, col, w, A, K, inv_t, AR.levels(), LS.SEED, max_descent, groups=groups,
                        wide_layout=False)
        assert (old[0] != ref["assign"]).any()


def test_the_cases_exercise_snapshots_and_acceptance():
    """Among the annealing cases some candidate keeps its start (snap_sweep == 0), some takes a later snapshot, and some
    final assignment differs from what no annealing sweeps give - otherwise the snapshot and acceptance code could be
    wrong unnoticed."""
    kept = later = differs = 0
    for name in ("n4097_K2", "n5000_K3", "star4200"):
        K, n, rowptr, col, w, A, inv_t, max_descent, groups = LS.big_case(name)
        ref = LS.big_reference(name)
        plain, _snap, _sw = LS.anneal(n, rowptr, col, w, A, K, inv_t[:0], AR.levels(), LS.SEED, max_descent,
                                      groups=groups)
        kept += int((ref["snap"] == 0).sum())
        later += int((ref["snap"] > 0).sum())
        differs += int((plain != ref["assign"]).any(axis=1).sum())
    for K in (2, 4):
        h, A, inv_t = LS.condition_case(K)
        out, snap, _sw = LS.anneal(h.n, h.rowptr, h.col, h.weight, A, K, inv_t, AR.levels(), LS.SEED, 100)
        plain, _s, _w = LS.anneal(h.n, h.rowptr, h.col, h.weight, A, K, inv_t[:0], AR.levels(), LS.SEED, 100)
        assert (snap == 0).any() and (snap > 0).any(), snap
        assert (plain != out).any()
        kept += int((snap == 0).sum())
    assert kept >= 1 and later >= 1 and differs >= 1, (kept, later, differs)


# ---- status codes (fake pointers: no call reaches a launch) ----------------------------------------------------------
NULL, SOME = C.c_void_p(None), C.c_void_p(4096)


def mk(hip, **kw):
    return hip.GmcBatch(**{**dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096, gcol=4096), **kw})


def test_status_codes_of_the_large_sampler(built):
    hip = built.hip
    lib = hip.load()
    size = lib.gmc_large_search_workspace_bytes

    def f(batch, P=SOME, K=4, gkey=SOME, iters=5, assign_all=SOME, ws=SOME, ws_bytes=None, cut_all=SOME,
          best_assign=SOME, best_cut=SOME, best_iter=SOME):
        b = None if batch is None else C.byref(batch)
        if ws_bytes is None:
            ws_bytes = 0 if batch is None else max(size(b, K if 2 <= K <= 8 else 2, max(iters, 1)), 16)
        return lib.gmc_large_sample_seeded_f32(b, P, K, gkey, iters, assign_all, ws, ws_bytes, cut_all, best_assign,
                                               best_cut, best_iter, None)
    b = mk(hip)
    assert f(None) == -1
    for name in ("P", "gkey", "ws", "cut_all", "best_assign", "best_cut", "best_iter"):
        assert f(b, **{name: NULL}) == -1, name
    assert f(mk(hip, abi=100)) == -8
    assert f(mk(hip, abi=100), P=NULL) == -1                           # the order: NULL, then the abi word
    for field in ("goff", "rowptr", "lcol", "gcol"):
        assert f(mk(hip, **{field: None})) == -1, field
        assert f(mk(hip, abi=100, **{field: None})) == -8              # ... then the batch's arrays
    for K in (1, 9, 0, -3):
        assert f(b, K=K) == -3, K
        assert f(mk(hip, gcol=None), K=K) == -1                        # ... then the class count
        assert f(b, K=K, iters=0) == -3
    assert f(b, iters=0) == -2 and f(mk(hip, B=-1)) == -2
    assert f(mk(hip, n_max=3), iters=0) == -2                          # ... then the shape, then the graph size
    assert f(mk(hip, n_max=3)) == -6 and f(mk(hip, n_max=(1 << 20) + 1)) == -6
    assert f(mk(hip, n_max=2), K=3) == -6
    assert f(mk(hip, n_max=3), ws_bytes=0) == -6                       # ... then the workspace
    need = size(C.byref(b), 4, 5)
    assert f(b, ws_bytes=need - 1) == -5
    assert f(mk(hip, n_max=4097, R=5000), ws_bytes=need) == -5         # (4097 nodes are no refusal)
    assert f(mk(hip, n_max=1 << 20, R=1 << 20, B=1), ws_bytes=need) == -5
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096, gcol=4096)
    for K in range(2, 9):                                              # every class count in range gets past all checks
        assert f(empty, K=K) == 0
        assert f(empty, K=K, assign_all=NULL) == 0
        assert f(mk(hip, n_max=K - 1), K=K) == -6
    assert f(empty, iters=0) == -2 and f(empty, K=9) == -3 and f(empty, ws_bytes=0) == -5


def test_status_codes_of_the_large_annealing(built):
    hip = built.hip
    lib = hip.load()
    size = lib.gmc_large_search_workspace_bytes

    def f(batch, K=4, order=SOME, cgoff=SOME, cptr=SOME, classes=5, cands=4, assign=SOME, inv_temp=SOME, sweeps=10,
          levels=SOME, descent=10, ws=SOME, ws_bytes=None, cut_all=SOME, best_assign=SOME, best_cut=SOME, best_idx=SOME):
        b = None if batch is None else C.byref(batch)
        if ws_bytes is None:
            ws_bytes = 0 if batch is None else max(size(b, K if 2 <= K <= 8 else 2, max(cands, 1)), 16)
        return lib.gmc_large_anneal_f32(b, K, order, cgoff, cptr, classes, cands, assign, inv_temp, sweeps, levels, 7,
                                        descent, ws, ws_bytes, cut_all, best_assign, best_cut, best_idx, NULL, NULL, None)
    b = mk(hip)
    # 1. NULL pointers (before the abi word is read), the workspace among them
    assert f(None) == -1
    for name in ("order", "cgoff", "cptr", "assign", "inv_temp", "levels", "ws", "cut_all", "best_assign", "best_cut",
                 "best_idx"):
        assert f(b, **{name: NULL}) == -1, name
    # 2. the abi word, 3. the batch's own pointers, gcol among them
    assert f(mk(hip, abi=100)) == -8 and f(mk(hip, abi=100), order=NULL) == -1
    for field in ("goff", "rowptr", "lcol", "gcol"):
        assert f(mk(hip, **{field: None})) == -1, field
        assert f(mk(hip, abi=100, **{field: None})) == -8
    # 4. the class count, before the shapes
    for K in (1, 9, 0, -3):
        assert f(b, K=K) == -3, K
        assert f(b, K=K, cands=0) == -3
        assert f(mk(hip, gcol=None), K=K) == -1
    # 5. shapes: the annealing's own and the family's
    assert f(b, cands=0) == -2 and f(b, sweeps=-1) == -2 and f(b, descent=-1) == -2 and f(mk(hip, B=-1)) == -2
    assert f(b, classes=-1) == -2
    assert f(b, sweeps=1 << 20) == -2                                  # the counter keeps 20 bits for the sweep
    assert f(mk(hip, n_max=4097, R=5000), cands=1 << 24, ws_bytes=16) == -2   # ... and 24 for the candidate beyond 4096 nodes
    assert f(mk(hip, n_max=4097, R=5000), cands=1 << 24, inv_temp=NULL, ws_bytes=16) == -2
    assert f(mk(hip, n_max=4096, R=5000), cands=1 << 24, ws_bytes=16) == -5   # the old layout has 32
    assert f(mk(hip, n_max=4097, R=5000), cands=(1 << 24) - 1, ws_bytes=16) == -5
    assert f(b, cands=0, inv_temp=NULL) == -2                          # the shape before the tables
    # 6. the tables, before the graph size
    assert f(mk(hip, n_max=3), inv_temp=NULL) == -1
    assert f(mk(hip, n_max=3), levels=NULL) == -1                      # anneal_sweeps > 0 with NULL levels
    assert f(b, sweeps=0, inv_temp=NULL, levels=NULL, ws_bytes=0) == -5
    # 7. the graph size, before the workspace
    assert f(mk(hip, n_max=3), ws_bytes=0) == -6 and f(mk(hip, n_max=(1 << 20) + 1), ws_bytes=0) == -6
    assert f(mk(hip, n_max=2), K=3, ws_bytes=0) == -6
    # 8. the workspace
    need = size(C.byref(b), 4, 4)
    assert f(b, ws_bytes=need - 1) == -5
    assert f(b, cands=5, ws_bytes=need) == -5                          # a candidate more: a larger workspace
    assert f(mk(hip, n_max=4097, R=5000), ws_bytes=need) == -5         # (4097 nodes are no refusal)
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096, gcol=4096)
    for K in range(2, 9):
        assert f(empty, K=K) == 0
        assert f(empty, K=K, sweeps=0, inv_temp=NULL, levels=NULL) == 0   # no annealing: neither table is needed
        assert f(mk(hip, n_max=K - 1), K=K) == -6
    assert f(empty, sweeps=(1 << 20) - 1) == 0
    for name in ("gmc_large_search_workspace_bytes", "gmc_large_sample_seeded_f32", "gmc_large_anneal_f32"):
        assert name in hip.SYMBOLS


def test_workspace_bytes(built):
    hip = built.hip
    f = hip.load().gmc_large_search_workspace_bytes
    batch = lambda **kw: C.byref(hip.GmcBatch(**{**dict(B=2, R=100, n_max=60), **kw}))
    assert f(None, 3, 4) == 0
    assert f(batch(abi=100), 3, 4) == 0
    for K in (-1, 0, 1, 9):
        assert f(batch(), K, 4) == 0
    assert f(batch(), 3, 0) == 0 and f(batch(), 3, -1) == 0
    assert f(batch(B=-1), 3, 4) == 0 and f(batch(R=-1), 3, 4) == 0
    by_cands = [f(batch(), 3, c) for c in (1, 2, 3, 5, 9, 17, 33, 64, 65, 129, 202)]
    assert all(a < b for a, b in zip(by_cands, by_cands[1:]))
    assert all(s % 16 == 0 for s in by_cands)
    assert by_cands[0] >= 2 * 100 + 4 * (5 * 2 + 1) + 4 * 2           # state and snapshot, the flag words, the cuts
    big = f(batch(B=1, R=1 << 20, n_max=1 << 20), 3, 202)
    assert 2 * 256 * (1 << 20) <= big <= 2.05 * 256 * (1 << 20)        # about 2.02 cpad bytes per row
    assert f(batch(B=1, R=1 << 20, n_max=1 << 20), 3, 10) <= 2.05 * 16 * (1 << 20)
    assert f(batch(B=200), 3, 4) > f(batch(B=2), 3, 4)
    assert f(batch(), 2, 4) == f(batch(), 8, 4)                        # the state is bytes: no dependence on K


TEMPLATED = ("large_sample_draw_kernel", "large_sample_regenerate_kernel", "large_anneal_colour_kernel",
             "large_search_descent_colour_kernel")
PLAIN = ("large_search_init_kernel", "large_search_fold_kernel", "large_search_snapshot_kernel",
         "large_search_close_kernel", "large_search_pick_kernel", "large_search_copy_kernel")
RECOUNT = "large_search_recount_kernel"


def test_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for kernel in TEMPLATED:
        for K in range(2, 9):
            assert sum(f"{kernel}<{K}>(" in s for s in names) == 1, (kernel, K)
    for G in (1, 2, 4, 8):
        assert sum(f"{RECOUNT}<{G}>(" in s for s in names) == 1, G
    for kernel in PLAIN:
        assert sum(f"{kernel}(" in s for s in names) == 1, kernel
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            if not any(k in fields.get(".name", "") for k in TEMPLATED + PLAIN + (RECOUNT,)):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
    assert seen == 7 * len(TEMPLATED) + len(PLAIN) + 4


# ---- the Python functions' refusals (all raised before a GPU is asked for) -------------------------------------------
def test_python_refusals(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = nx.convert_node_labels_to_integers(R.regular_graph(16, 3, 1))
    good = [i % 4 for i in range(16)]
    for K in (1, 9, 0):
        with pytest.raises(ValueError, match="number_classes"):
            TN.large_annealing(good, g, K)
    with pytest.raises(ValueError, match="entries"):
        TN.large_annealing(good[:-1], g, 4)
    with pytest.raises(ValueError, match="outside 0..3"):
        TN.large_annealing(good[:-1] + [4], g, 4)
    with pytest.raises(ValueError, match="outside 0..1"):
        TN.large_annealing(good, g, 2)
    with pytest.raises(ValueError, match="outside"):
        TN.large_annealing([-1] + good[1:], g, 4)
    with pytest.raises(ValueError, match="at least 5 nodes"):
        TN.large_annealing([0, 1, 2, 3], nx.complete_graph(4), 5)
    with pytest.raises(ValueError, match="sweeps"):
        TN.large_annealing(good, g, 4, sweeps=-1)
    with pytest.raises(ValueError, match="sweeps"):
        TN.large_annealing(good, g, 4, max_descent_sweeps=-1)
    with pytest.raises(ValueError, match="number_classes"):
        TN.large_sampling_optimization(np.full((16, 9), 1 / 9, np.float32), g)
    with pytest.raises(ValueError, match="number_classes"):
        TN.large_sampling_optimization(np.full((16, 1), 1.0, np.float32), g)
    with pytest.raises(ValueError, match="number_classes"):
        TN.large_sampling_optimization(np.full(16, 1.0, np.float32), g)
    with pytest.raises(ValueError, match="rows"):
        TN.large_sampling_optimization(np.full((15, 4), 0.25, np.float32), g)
    with pytest.raises(ValueError, match="at least 5 nodes"):
        TN.large_sampling_optimization(np.full((4, 5), 0.2, np.float32), nx.complete_graph(4))
    for kw in (dict(samples=-1), dict(anneal_sweeps=-1), dict(max_descent_sweeps=-1), dict(candidates=0),
               dict(samples=5, candidates=8), dict(samples=0, candidates=3)):
        with pytest.raises(ValueError):
            TN.search_large_dataset(None, {}, **kw)
    built.install_compat()                                             # the reference's import roots mirror the module
    import Testing.TestingNeuralNetwork as mirror
    assert mirror.search_large_dataset is TN.search_large_dataset
    assert mirror.large_annealing is TN.large_annealing
    assert mirror.large_sampling_optimization is TN.large_sampling_optimization


def test_the_small_functions_still_stop_at_4096_nodes(built):
    """The one-workgroup decoders keep their limit and name the new functions after their old wording."""
    from gcn_max_cut_amd.graph import GraphHandle
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    for what in ("decode_dataset", "search_dataset", "round_dataset"):
        with pytest.raises(ValueError, match="4096 nodes.*argmax partition.*large_conditional_rounding.*"
                                             "large_sampling_optimization, large_annealing and search_large_dataset"):
            TN._decoder_graph_size(what, 4097)
        TN._decoder_graph_size(what, 4096)
    hip = built.hip
    lib = hip.load()
    b = C.byref(mk(hip, n_max=4097, R=5000))
    assert lib.gmc_kway_refine_anneal_f32(b, 4, SOME, SOME, SOME, 4, SOME, SOME, 10, SOME, 7, 10, SOME, SOME, SOME, SOME,
                                          NULL, NULL, None) == -6
    assert lib.gmc_refine_anneal_f32(b, SOME, SOME, SOME, 4, SOME, SOME, 10, SOME, 7, 10, SOME, SOME, SOME, SOME, NULL,
                                     NULL, None) == -6
    assert lib.gmc_kway_decode_sample_seeded_f32(C.byref(mk(hip, n_max=65536, R=70000)), SOME, 4, SOME, 5, SOME, SOME,
                                                 SOME, SOME, SOME, None) == -6
    n, rowptr, col = LR.circulant(4097, 4, None)
    big = GraphHandle(n, rowptr, col)
    items = {0: (big, None, None, [0, 1, 2])}

    class Model:                                                       # refused before the model is run
        def engine(self):
            class E:
                K = 3
                device = "cpu"
            return E()

        def eval(self):
            pass
    for call in (TN.search_dataset, TN.decode_dataset):
        with pytest.raises(ValueError, match="4096 nodes"):
            call(Model(), items)
