"""CPU checks of the K-class decoders (include/gcnmaxcut.h, gmc_kway_decode_sample_seeded_f32 and
gmc_kway_refine_anneal_f32): the vectorised restatement tests/kway_search_ref.py against its one-node-at-a-time
definition, its agreement at K = 3 with the 3-class restatements (anneal_ref, refine_ref, seeded_ref), the product's
host form of the draw rule, the sampler's edge rows, every status code of both entry points in the documented order
(found before any HIP call: no GPU needed), the 14 kernel instantiations in the gfx950 code object, and the refusals
of the new Python functions."""
import ctypes as C
import subprocess

import networkx as nx
import numpy as np
import pytest
import torch

from oracle import ref_dense as R
from tests import anneal_ref as AR
from tests import kway_search_ref as KS
from tests import refine_ref as RR
from tests import rounding_ref as RO
from tests import seeded_ref as SR
from tests import util
from tests.test_anneal_host import SMALL, dyadic_weights
from tests.test_refine_host import handles_of, loop_graph

KS_SMALL = {
    "nK": lambda K: (nx.complete_graph(K), None),
    "nK1": lambda K: (nx.complete_graph(K + 1), None),
    "regular": lambda K: (R.regular_graph(40, 5, 1), None),
    "self_loops": lambda K: (loop_graph(36, 4, 2), None),
    "dyadic": lambda K: (R.regular_graph(30, 6, 3), 4),
}


@pytest.mark.parametrize("K", (2, 4, 8))
@pytest.mark.parametrize("case", sorted(KS_SMALL))
def test_vectorised_restatement_equals_the_sequential_definition(case, K):
    g, wseed = KS_SMALL[case](K)
    h = handles_of([g])[0]
    w = None if wseed is None else dyadic_weights(h, wseed)
    rng = np.random.RandomState(len(case) + K)
    cands = 5
    A = rng.randint(0, K, (cands, h.n)).astype(np.int8)
    if h.n > 12:
        A[1, 9] = K                                                    # bytes of no class: count for nothing, move
        A[2, 11] = -1
    inv_t, table = AR.schedule(12), AR.levels()
    for max_descent in (0, 100):
        out, snap, sweeps = KS.anneal(h.n, h.rowptr, h.col, w, A, K, inv_t, table, 9, max_descent)
        for i in range(cands):
            a, sn, sw = KS.sequential(h.n, h.rowptr, h.col, w, A[i].tolist(), K, inv_t, table, 9, max_descent, cand=i)
            assert out[i].tolist() == a and snap[i] == sn and sweeps[i] == sw, (case, K, i)
        assert (out[:, :K] == A[:, :K]).all()
        if h.n > 12:
            assert 0 <= out[1, 9] < K and 0 <= out[2, 11] < K          # the first annealing sweep gives them a class
    out2, snap2, _ = KS.anneal(h.n, h.rowptr, h.col, w, A[3:], K, inv_t, table, 9, 100, cand_ids=[3, 4])
    assert (out2 == out[3:]).all() and (snap2 == snap[3:]).all()
    # no annealing sweeps: the K-class local search, which is the descent of the rounding restatement
    plain, snap0, sw0 = KS.anneal(h.n, h.rowptr, h.col, w, A, K, inv_t[:0], table, 9, 100)
    ref, ref_sw = KS.refine(h.n, h.rowptr, h.col, w, A, K, 100)
    assert (plain == ref).all() and (sw0 == ref_sw).all() and (snap0 == 0).all()
    clean = rng.randint(0, K, (1, h.n)).astype(np.int8)
    got, got_sw = KS.refine(h.n, h.rowptr, h.col, w, clean, K, 100)
    want, want_sw = RO.descent(h.n, h.rowptr, h.col, w, clean[0], K, 100)
    assert (got[0] == want).all() and got_sw[0] == want_sw
    if got_sw[0] < 100:
        assert KS.best_single_move_gain(h.n, h.rowptr, h.col, w, got[0].tolist(), K) == 0


@pytest.mark.parametrize("case", sorted(SMALL))
def test_three_classes_are_the_three_class_restatements(case):
    """On the graphs of tests/test_anneal_host.py: anneal_ref.anneal and refine_ref.refine byte for byte."""
    g, wseed = SMALL[case]()
    h = handles_of([g])[0]
    w = None if wseed is None else dyadic_weights(h, wseed)
    A = np.random.RandomState(len(case)).randint(0, 3, (5, h.n)).astype(np.int8)
    if h.n > 6:
        A[1, 5] = 3
    inv_t, table = AR.schedule(12), AR.levels()
    for max_descent in (0, 100):
        got = KS.anneal(h.n, h.rowptr, h.col, w, A, 3, inv_t, table, 9, max_descent)
        want = AR.anneal(h.n, h.rowptr, h.col, w, A, inv_t, table, 9, max_descent)
        for a, b in zip(got, want):
            assert a.tobytes() == np.asarray(b, a.dtype).tobytes()
    for max_sweeps in (0, 1, 100):
        got = KS.refine(h.n, h.rowptr, h.col, w, A, 3, max_sweeps)
        want = RR.refine(h.n, h.rowptr, h.col, w, A, max_sweeps)
        assert (got[0] == want[0]).all() and (got[1] == want[1]).all()
    assert KS.sequential_sweep(h.n, h.rowptr, h.col, w, A[0].tolist(), 3) == \
        RR.sequential_sweep(h.n, h.rowptr, h.col, w, A[0].tolist())
    _colour, classes = RR.colouring(h.n, h.rowptr, h.col)
    assert all((a == b).all() for a, b in zip(KS.classes_of(h.n, h.rowptr, h.col, 3), classes))


def softmax(n, K, seed):
    return RO.softmax_rows(n, K, seed)


@pytest.mark.parametrize("n", (3, 4, 65, 257))
def test_three_class_samples_are_seeded_refs(n):
    P = softmax(n, 3, n)
    rows = np.array(((0.25, 0.25, 0.25), (1, 0, 0), (0, 1, 0), (0, 0, 1)), np.float32)[:max(0, min(4, n - 3))]
    P[3:3 + len(rows)] = rows
    for seed, index in ((0, 0), (7, 3), ((1 << 64) - 1, 11)):
        key = SR.keys(seed, [index])[0]
        for iters, first in ((1, 0), (33, 0), (4, 29)):
            got = KS.assignments(P, key, iters, first)
            assert got.tobytes() == SR.assignments(P, key, iters, first).tobytes()
    h = handles_of([util.near_regular(n, 3, n) if n > 4 else nx.complete_graph(n)])[0]
    key = SR.keys(5, [2])[0]
    got, want = KS.sample(h, P, key, 7), SR.sample(h, P, key, 7)
    for k in want:
        assert np.asarray(got[k]).tobytes() == np.asarray(want[k]).tobytes(), k


@pytest.mark.parametrize("K", range(2, 9))
def test_host_form_of_the_draw_rule_equals_the_restatement(built, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    for n in (K, K + 1, 40):
        P = softmax(n, K, 10 * K + n)
        for seed, index in ((0, 0), (12345, 7), ((1 << 64) - 3, 2)):
            key = SR.keys(seed, [index])[0]
            ref = KS.assignments(P, key, 6)
            for it in (0, 5):
                assert TN.assign_partitions_seeded_kway(P, seed, index, it) == ref[it].tolist()
            if K == 3:
                assert TN.assign_partitions_seeded_kway(P, seed, index, 5) == TN.assign_partitions_seeded(P, seed, index, 5)
    assert (TN.sample_keys(9, range(4)) == SR.keys(9, range(4))).all()


@pytest.mark.parametrize("K", (2, 3, 5, 8))
def test_sampler_edge_rows(built, K):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    n, iters = K + 3 * K + 4, 40
    P = softmax(n, K, K)
    P[:K] = np.nan                                                     # terminals: their rows are never read
    P[0] = np.eye(K, dtype=np.float32)[K - 1]
    for j in range(K):
        P[K + j] = np.eye(K, dtype=np.float32)[j]                      # one-hot rows: that class in every iteration
    P[2 * K] = 0.0                                                     # an all-zero row: the fallback
    P[2 * K + 1] = np.nan                                              # a NaN row: every compare is false
    P[2 * K + 2] = 0.0
    P[2 * K + 2, K - 1] = np.nan                                       # the last sum is never compared
    key = SR.keys(3, [0])[0]
    a = KS.assignments(P, key, iters)
    assert (a[:, :K] == np.arange(K)).all()
    for j in range(K):
        assert (a[:, K + j] == j).all()
    assert (a[:, 2 * K:2 * K + 3] == K - 1).all()
    assert ((a >= 0) & (a < K)).all()
    rest = a[:, 2 * K + 3:]
    assert len(np.unique(rest)) == K                                   # softmax rows reach every class in 40 draws
    # iteration i of a short call is iteration i of a long one
    assert (KS.assignments(P, key, 7)[5] == a[5]).all() and (KS.assignments(P, key, 3, first_iter=20) == a[20:23]).all()
    for it in (0, 17):
        assert TN.assign_partitions_seeded_kway(P, 3, 0, it) == a[it].tolist()
    # the running sum is a double sum of the float32 entries: a draw between the float32 and the double sum decides
    u = SR.uniforms(key, 1, n)[0]
    assert ((u >= 0) & (u < 1)).all()


# ---- status codes (fake pointers: no call reaches a launch) ----------------------------------------------------------
NULL, SOME = C.c_void_p(None), C.c_void_p(4096)


def mk(hip, **kw):
    return hip.GmcBatch(**{**dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096), **kw})


def test_status_codes_of_the_kway_sampler(built):
    hip = built.hip
    lib = hip.load()

    def f(batch, P=SOME, K=4, gkey=SOME, iters=5, assign_all=SOME, cut_all=SOME, best_assign=SOME, best_cut=SOME,
          best_iter=SOME):
        b = None if batch is None else C.byref(batch)
        return lib.gmc_kway_decode_sample_seeded_f32(b, P, K, gkey, iters, assign_all, cut_all, best_assign, best_cut,
                                                     best_iter, None)
    b = mk(hip)
    assert f(None) == -1
    for name in ("P", "gkey", "cut_all", "best_assign", "best_cut", "best_iter"):
        assert f(b, **{name: NULL}) == -1, name
    assert f(mk(hip, abi=100)) == -8
    assert f(mk(hip, abi=100), P=NULL) == -1                           # the order: NULL, then the abi word
    for field in ("goff", "rowptr", "lcol"):
        assert f(mk(hip, **{field: None})) == -1, field
        assert f(mk(hip, abi=100, **{field: None})) == -8              # ... then the batch's arrays
    for K in (1, 9, 0, -3):
        assert f(b, K=K) == -3, K
        assert f(mk(hip, lcol=None), K=K) == -1                        # ... then the class count
        assert f(b, K=K, iters=0) == -3
    assert f(b, iters=0) == -2 and f(mk(hip, B=-1)) == -2
    assert f(mk(hip, n_max=3), iters=0) == -2                          # ... then the shape, then the graph size
    assert f(mk(hip, n_max=3)) == -6 and f(mk(hip, n_max=65536)) == -6
    assert f(mk(hip, n_max=2), K=3) == -6
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096)
    for K in range(2, 9):                                              # every class count in range gets past all checks
        assert f(empty, K=K) == 0
        assert f(empty, K=K, assign_all=NULL) == 0
        assert f(mk(hip, n_max=K - 1), K=K) == -6
    assert f(empty, iters=0) == -2 and f(empty, K=9) == -3


def test_status_codes_of_the_kway_annealing(built):
    hip = built.hip
    lib = hip.load()

    def f(batch, K=4, order=SOME, cgoff=SOME, cptr=SOME, cands=4, assign=SOME, inv_temp=SOME, sweeps=10, levels=SOME,
          descent=10, cut_all=SOME, best_assign=SOME, best_cut=SOME, best_idx=SOME):
        b = None if batch is None else C.byref(batch)
        return lib.gmc_kway_refine_anneal_f32(b, K, order, cgoff, cptr, cands, assign, inv_temp, sweeps, levels, 7,
                                              descent, cut_all, best_assign, best_cut, best_idx, NULL, NULL, None)
    b = mk(hip)
    assert f(None) == -1
    for name in ("order", "cgoff", "cptr", "assign", "inv_temp", "levels", "cut_all", "best_assign", "best_cut", "best_idx"):
        assert f(b, **{name: NULL}) == -1, name
    assert f(mk(hip, abi=100)) == -8 and f(mk(hip, abi=100), order=NULL) == -1
    for field in ("goff", "rowptr", "lcol"):
        assert f(mk(hip, **{field: None})) == -1, field
        assert f(mk(hip, abi=100, **{field: None})) == -8
    for K in (1, 9, 0, -3):
        assert f(b, K=K) == -3, K
        assert f(b, K=K, cands=0) == -3                                # the class count before the shape
        assert f(mk(hip, lcol=None), K=K) == -1
    assert f(b, cands=0) == -2 and f(b, sweeps=-1) == -2 and f(b, descent=-1) == -2 and f(mk(hip, B=-1)) == -2
    assert f(b, sweeps=1 << 20) == -2                                  # the counter keeps 20 bits for the sweep
    assert f(b, cands=0, inv_temp=NULL) == -2                          # the shape before the tables
    assert f(mk(hip, n_max=3), inv_temp=NULL) == -1                    # the tables before the graph size
    assert f(mk(hip, n_max=3)) == -6 and f(mk(hip, n_max=4097)) == -6
    assert f(mk(hip, n_max=2), K=3) == -6
    empty = hip.GmcBatch(B=0, goff=4096, rowptr=4096, lcol=4096)
    for K in range(2, 9):
        assert f(empty, K=K) == 0
        assert f(empty, K=K, sweeps=0, inv_temp=NULL, levels=NULL) == 0   # no annealing: neither table is needed
        assert f(mk(hip, n_max=K - 1), K=K) == -6
    assert f(empty, sweeps=(1 << 20) - 1) == 0
    for name in ("gmc_kway_decode_sample_seeded_f32", "gmc_kway_refine_anneal_f32"):
        assert name in hip.SYMBOLS
    # the LDS layout does not depend on K: the 3-class query answers for this entry point
    assert lib.gmc_refine_anneal_staged(C.byref(hip.GmcBatch(n_max=1000, nnz_max=7000))) == 1
    assert lib.gmc_refine_anneal_staged(C.byref(hip.GmcBatch(n_max=1000, nnz_max=7000, vals=4096))) == 0


def test_no_instantiation_of_the_search_kernels_is_missing_or_spills(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for K in range(2, 9):
        for kernel in ("sample_seeded_k_kernel", "sample_seeded_k_pick_kernel", "anneal_k_kernel"):
            assert sum(f"{kernel}<{K}>" in s for s in names) == 1, (kernel, K)
    assert any("anneal_k_pick_kernel" in s for s in names)
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if not ("_k_" in entry and ".name:" in entry):
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith(".") and ":" in l)
            name = fields.get(".name", "")
            if "anneal_k_kernel" not in name and "sample_seeded_k_" not in name:
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, name
            assert int(fields[".vgpr_spill_count"]) == 0, name
    assert seen == 21


# ---- the Python functions' refusals (all raised before a GPU is asked for) -------------------------------------------
def test_new_python_functions_refuse_what_they_cannot_take(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = nx.convert_node_labels_to_integers(R.regular_graph(16, 3, 1))
    good = [i % 4 for i in range(16)]
    for call in (TN.kway_local_search, TN.kway_annealing):
        for K in (1, 9, 0):
            with pytest.raises(ValueError, match="number_classes"):
                call(good, g, K)
        with pytest.raises(ValueError, match="entries"):
            call(good[:-1], g, 4)
        with pytest.raises(ValueError, match="outside 0..3"):
            call(good[:-1] + [4], g, 4)
        with pytest.raises(ValueError, match="outside 0..1"):
            call(good, g, 2)
        with pytest.raises(ValueError, match="outside"):
            call([-1] + good[1:], g, 4)
        with pytest.raises(ValueError, match="at least 5 nodes"):
            call([0, 1, 2, 3], nx.complete_graph(4), 5)
    with pytest.raises(ValueError, match="max_sweeps"):
        TN.kway_local_search(good, g, 4, max_sweeps=-1)
    with pytest.raises(ValueError, match="sweeps"):
        TN.kway_annealing(good, g, 4, sweeps=-1)
    with pytest.raises(ValueError, match="sweeps"):
        TN.kway_annealing(good, g, 4, max_descent_sweeps=-1)
    with pytest.raises(ValueError, match="number_classes"):
        TN.sampling_optimization(np.full((16, 9), 1 / 9, np.float32), g)
    with pytest.raises(ValueError, match="number_classes"):
        TN.sampling_optimization(torch.full((16, 1), 1.0), g)
    with pytest.raises(ValueError, match="rows"):
        TN.sampling_optimization(np.full((15, 4), 0.25, np.float32), g)
    with pytest.raises(ValueError, match="at least 5 nodes"):
        TN.sampling_optimization(np.full((4, 5), 0.2, np.float32), nx.complete_graph(4))
    with pytest.raises(ValueError, match="number_classes"):
        TN.assign_partitions_seeded_kway(np.full((16, 9), 1 / 9, np.float32), 0)
    with pytest.raises(ValueError, match="iteration"):
        TN.assign_partitions_seeded_kway(np.full((16, 4), 0.25, np.float32), 0, 0, -1)
    with pytest.raises(ValueError, match="index"):
        TN.assign_partitions_seeded_kway(np.full((16, 4), 0.25, np.float32), 0, -1)
    for kw in (dict(samples=-1), dict(anneal_sweeps=-1), dict(max_descent_sweeps=-1), dict(candidates=0),
               dict(samples=5, candidates=8), dict(samples=0, candidates=3)):
        with pytest.raises(ValueError):
            TN.search_dataset(None, {}, **kw)
    # the 3-class functions keep refusing
    with pytest.raises(ValueError, match="number_classes"):
        TN.local_search_optimization(good, g, number_classes=4)
