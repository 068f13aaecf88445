"""CPU checks of the rounding and the local search for graphs beyond 4096 nodes (include/gcnmaxcut.h:
gmc_large_round_order_host, gmc_large_round_workspace_bytes, gmc_large_round_conditional_f32,
gmc_large_local_search_f32): the host colouring against gmc_round_order_host and against the restatement of
tests/large_round_ref.py, the entry points' argument checks (no GPU needed), the kernels' metadata in the gfx950 code
object, the vectorised restatement against the sequential ones, and the Python refusals."""
import ctypes as C
import subprocess

import networkx as nx
import numpy as np
import pytest

from oracle import ref_dense as R
from tests import kway_search_ref as KS
from tests import large_ref as LR
from tests import large_round_ref as LRR
from tests import rounding_ref as CR
from tests import util
from tests.test_refine_host import handles_of
from tests.test_rounding_host import ORDER_BATCHES, order_from_K


def large_order(ba, K, cap=None):
    """gmc_large_round_order_host on a BatchArrays: (rc, order, cgoff, cptr, max_classes), outputs pre-filled."""
    from gcn_max_cut_amd import hip
    order = np.full(max(ba.R, 1), -7, np.int32)
    cgoff = np.full(ba.B + 1, -7, np.int32)
    cptr = np.full(ba.R + ba.B if cap is None else cap, -7, np.int32)
    most = C.c_int32(-7)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    go = ba.goff.astype(np.int32)
    rc = hip.load().gmc_large_round_order_host(ba.B, p(go), p(ba.rowptr), p(ba.lcol), K, p(order), p(cgoff), p(cptr),
                                               cptr.size, C.byref(most))
    return rc, order, cgoff, cptr, most.value


@pytest.mark.parametrize("name", sorted(ORDER_BATCHES))
def test_large_order_equals_round_order_where_both_run(built, name):
    from gcn_max_cut_amd.graph import BatchArrays
    hs = handles_of(ORDER_BATCHES[name]())
    ba = BatchArrays(hs)
    ran = 0
    for K in (2, 3, 5, 8):
        want = order_from_K(ba, K)
        got = large_order(ba, K)
        assert got[0] == want[0]
        if min(h.n for h in hs) < K:
            assert got[0] == -6
            continue
        assert got[0] == 0
        ran += 1
        for a, b in zip(want[1:], got[1:4]):                          # array for array, the untouched tails included
            assert a.dtype == b.dtype and (a == b).all(), K
        cgoff = got[2]
        assert got[4] == int(np.diff(cgoff).max()) - 1
    assert ran >= 2


BEYOND = {
    "circ4097": lambda: [LR.circulant(4097, 7, 6)],
    "star4200": lambda: [LR.star(4200, 5)],
    "circ70000": lambda: [LR.circulant(70000, 7, None)],
    "batch": lambda: [LR.circulant(5, 3, None), LR.circulant(4097, 6, None), LR.circulant(257, 7, 3)],
}


@pytest.mark.parametrize("name", sorted(BEYOND))
def test_large_order_beyond_4096_nodes_is_the_restatements(built, name):
    from gcn_max_cut_amd.graph import BatchArrays, GraphHandle
    graphs = BEYOND[name]()
    ba = BatchArrays([GraphHandle(n, rp, col) for n, rp, col in graphs])
    for K in (3, 5) if name != "circ70000" else (4,):
        rc, order, cgoff, cptr, most = large_order(ba, K)
        assert rc == 0
        ref_order, ref_cgoff, ref_cptr, ref_most = LRR.order_arrays(graphs, K)
        moving = ba.R - K * ba.B
        assert (order[:moving] == ref_order).all() and (order[moving:] == -7).all()
        assert (cgoff == ref_cgoff).all()
        assert (cptr[:cgoff[-1]] == ref_cptr).all() and (cptr[cgoff[-1]:] == -7).all()
        assert most == ref_most >= 1
        if name == "star4200":
            assert most == 2                                           # the hub and everything else
        assert order_from_K(ba, K)[0] == -6                            # the one-workgroup routine keeps its refusal
        r0 = 0
        for g, (n, rp, col) in enumerate(graphs):
            classes = LRR.classes_from_order(order, cgoff, cptr, g, r0)
            assert [c.tolist() for c in classes] == [c.tolist() for c in LRR.colouring(n, rp, col, K)]
            r0 += n


def test_the_fast_colouring_is_rounding_refs(built):
    for K, n, rowptr, col, _w, _P in CR.cases()[::5]:
        want = CR.colouring(n, rowptr, col, K)[1]
        got = LRR.colouring(n, rowptr, col, K)
        assert [c.tolist() for c in got] == [c.tolist() for c in want]


def test_large_order_status_codes(built):
    lib = built.hip.load()
    null = C.c_void_p(None)
    some = (C.c_int32 * 16)()
    most = C.c_int32(-7)
    f = lib.gmc_large_round_order_host
    assert f(1, null, some, some, 4, some, some, some, 16, C.byref(most)) == -1               # GMC_ERR_NULL
    assert f(1, some, some, some, 4, some, some, null, 16, C.byref(most)) == -1
    assert f(1, some, some, some, 4, some, some, some, 16, null) == -1                        # max_classes is required
    for K in (-1, 0, 1, 9):
        assert f(1, some, some, some, K, some, some, some, 16, C.byref(most)) == -3           # GMC_ERR_CLASSES
    assert f(-1, some, some, some, 4, some, some, some, 16, C.byref(most)) == -2              # GMC_ERR_SHAPE
    goff = (C.c_int32 * 2)(0, 3)
    assert f(1, goff, some, some, 4, some, some, some, 16, C.byref(most)) == -6               # fewer than K nodes
    assert most.value == -7                                                                   # nothing written
    assert f(1, goff, some, some, 3, some, some, some, 16, C.byref(most)) == 0 and most.value == 0
    big = (C.c_int32 * 2)(0, 4097)
    assert lib.gmc_round_order_host(1, big, some, some, 2, some, some, some, 16) == -6        # the old limit stays
    assert lib.gmc_refine_order_host(1, big, some, some, some, some, some, 16) == -6
    over = (C.c_int32 * 2)(0, (1 << 20) + 1)
    assert f(1, over, some, some, 2, some, some, some, 16, C.byref(most)) == -6               # the new one
    assert f(1, big, some, some, 2, some, some, some, 16, C.byref(most)) == -2                # cptr_cap < R + B
    zero = (C.c_int32 * 1)(0)
    most.value = -7
    assert f(0, zero, some, some, 2, some, some, some, 0, C.byref(most)) == 0 and most.value == 0   # an empty batch


def test_device_entry_points_check_arguments_without_a_gpu(built):
    hip = built.hip
    lib = hip.load()
    null, some = C.c_void_p(None), C.c_void_p(4096)                    # (never dereferenced: the calls fail first)
    fields = dict(B=2, R=100, n_max=60, goff=4096, rowptr=4096, lcol=4096, gcol=4096)
    batch = lambda **kw: C.byref(hip.GmcBatch(**{**fields, **kw}))
    need = lib.gmc_large_round_workspace_bytes(batch(), 3)

    def rnd(b, P=some, K=3, order=some, cgoff=some, cptr=some, classes=4, sweeps_max=10, ws=some, ws_bytes=None,
            assign=some, cut=some, expected=some, sweeps=some):
        return lib.gmc_large_round_conditional_f32(b, P, K, order, cgoff, cptr, classes, sweeps_max, ws,
                                                   need if ws_bytes is None else ws_bytes, assign, cut, expected,
                                                   sweeps, None)

    def srch(b, P=None, K=3, order=some, cgoff=some, cptr=some, classes=4, sweeps_max=10, ws=some, ws_bytes=None,
             assign=some, cut=some, expected=None, sweeps=some):
        return lib.gmc_large_local_search_f32(b, K, order, cgoff, cptr, classes, sweeps_max, ws,
                                              need if ws_bytes is None else ws_bytes, assign, cut, sweeps, None)

    for f, required in ((rnd, ("P", "order", "cgoff", "cptr", "ws", "assign", "cut")),
                        (srch, ("order", "cgoff", "cptr", "ws", "assign", "cut"))):
        # 1. NULL pointers (before the abi word is read), the workspace among them
        assert f(None) == -1
        for name in required:
            assert f(batch(), **{name: null}) == -1, name
            assert f(batch(abi=100), **{name: null}) == -1, name
        # 2. the abi word, before the batch's pointers, the class count and the shapes
        assert f(batch(abi=100)) == -8
        assert f(batch(abi=100, gcol=None), K=9, sweeps_max=-1) == -8
        # 3. the batch's own pointers, gcol among them, before the class count
        for name in ("goff", "rowptr", "lcol", "gcol"):
            assert f(batch(**{name: None}), K=9) == -1, name
        # 4. the class count, before the shapes
        for K in (-3, 0, 1, 9, 100):
            assert f(batch(), K=K, sweeps_max=-1) == -3, K
        # 5. shapes, before the graph size
        assert f(batch(n_max=2), sweeps_max=-1) == -2
        assert f(batch(n_max=2), classes=-1) == -2
        assert f(batch(n_max=2, B=-1)) == -2
        # 6. the graph size, before the workspace
        assert f(batch(n_max=2), ws_bytes=0) == -6
        assert f(batch(n_max=7), K=8, ws_bytes=0) == -6
        assert f(batch(n_max=(1 << 20) + 1), ws_bytes=0) == -6
        # 7. the workspace
        assert f(batch(), ws_bytes=need - 1) == -5
        assert f(batch(n_max=1 << 20, R=1 << 20, B=1), ws_bytes=need) == -5      # (4097 nodes are no refusal any more)
        # an empty batch: nothing launched, whatever the optional outputs
        empty = lib.gmc_large_round_workspace_bytes(batch(B=0, R=0, n_max=0), 3)
        assert f(batch(B=0, R=0, n_max=0), ws_bytes=empty) == 0
        assert f(batch(B=0, R=0, n_max=0), ws_bytes=empty, expected=null, sweeps=null) == 0
    assert {"gmc_large_round_order_host", "gmc_large_round_workspace_bytes", "gmc_large_round_conditional_f32",
            "gmc_large_local_search_f32"} <= set(hip.SYMBOLS)


def test_workspace_bytes(built):
    hip = built.hip
    f = hip.load().gmc_large_round_workspace_bytes
    batch = lambda **kw: C.byref(hip.GmcBatch(**{**dict(B=2, R=100, n_max=60), **kw}))
    assert f(None, 3) == 0
    assert f(batch(abi=100), 3) == 0
    for K in (-1, 0, 1, 9):
        assert f(batch(), K) == 0
    sizes = [f(batch(R=R_, B=1, n_max=R_), 3) for R_ in (100, 5000, 70000, 1 << 20)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    assert sizes[0] >= 100 + 4 * 4 + 4 * 2                             # the class bytes, the flag words, the partials
    assert sizes[-1] <= 2 * (1 << 20)                                  # about a byte per row
    assert f(batch(B=200), 3) > f(batch(B=2), 3)
    assert all(s % 16 == 0 for s in sizes)


KERNELS = ("large_round_expect_kernel", "large_round_colour_kernel", "large_descent_colour_kernel")
PLAIN = ("large_round_init_kernel", "large_round_fold_kernel", "large_descent_close_kernel", "large_round_score_kernel")


def test_kernels_are_in_the_code_object_without_scratch(built):
    lib_path = built.hip.LIB_PATH
    names = util.kernel_symbols(lib_path)
    for kernel in KERNELS:
        for K in range(2, 9):
            assert any(f"{kernel}<{K}>(" in s for s in names), (kernel, K)
    for kernel in PLAIN:
        assert any(f"{kernel}(" in s for s in names), kernel
    seen = 0
    for co in util.gfx950_code_objects(lib_path):
        notes = subprocess.run([f"{util.ROCM_LLVM}/llvm-readelf", "--notes", "-"], input=co, capture_output=True,
                               check=True).stdout.decode()
        for entry in notes.split("\n  - ")[1:]:
            if ".name:" not in entry:
                continue
            fields = dict(l.strip().split(":", 1) for l in entry.splitlines() if l.strip().startswith("."))
            if not any(k in fields.get(".name", "") for k in KERNELS + PLAIN):
                continue
            seen += 1
            assert int(fields[".private_segment_fixed_size"]) == 0, fields[".name"]
            assert int(fields[".vgpr_spill_count"]) == 0 and int(fields[".sgpr_spill_count"]) == 0, fields[".name"]
    assert seen == 7 * len(KERNELS) + len(PLAIN)


def test_the_vectorised_restatement_equals_the_sequential_ones(built):
    rng = np.random.RandomState(5)
    for i, (K, n, rowptr, col, w, P) in enumerate(CR.cases()):
        LRR.check_inputs(K, n, rowptr, col, w, P)
        tables = LRR.class_tables(n, rowptr, col, w, LRR.colouring(n, rowptr, col, K))
        seq = CR.round_sequential(n, rowptr, col, w, P, K)
        poisoned = P.copy()
        poisoned[:K] = np.nan                                          # the terminals' rows are never read
        got = LRR.round_by_classes(n, poisoned, K, tables)
        assert got.dtype == np.int8 and (got == seq).all(), (K, n)
        for max_sweeps in (0, 1, 100):
            want, want_sweeps = CR.descent(n, rowptr, col, w, seq, K, max_sweeps)
            a, s = LRR.descent(n, got, K, tables, max_sweeps)
            assert (a == want).all() and s == want_sweeps, (K, n, max_sweeps)
        if i % 4 == 0:                                                 # the local search from anywhere, a byte of no class too
            A = rng.randint(0, K, (1, n)).astype(np.int8)
            A[0, K + 3], A[0, n - 1] = K, -1
            want, want_sweeps = KS.refine(n, rowptr, col, w, A, K, 100)
            a, s = LRR.descent(n, A[0], K, tables, 100)
            assert (a == want[0]).all() and s == want_sweeps[0]
            gain = LRR.best_single_move_gain(n, rowptr, col, w, a, K)
            assert gain == pytest.approx(KS.best_single_move_gain(n, rowptr, col, w, a.tolist(), K), abs=1e-12)


def test_the_restatement_on_a_hub_and_self_loops(built):
    """Rows of more than 64 entries take a table of their own: the same bytes as the sequential form."""
    from tests.test_refine_host import hub_graph, loop_graph
    for K, g in ((3, hub_graph(300, 7, 5)), (4, CR.signed_weights(hub_graph(200, 5, 6), 3)), (2, loop_graph(120, 5, 7))):
        h = handles_of([g])[0]
        P = CR.softmax_rows(h.n, K, 17 + K)
        tables = LRR.class_tables(h.n, h.rowptr, h.col, h.weight, LRR.colouring(h.n, h.rowptr, h.col, K))
        assert K == 2 or any(len(groups) > 1 for groups in tables)
        seq = CR.round_sequential(h.n, h.rowptr, h.col, h.weight, P, K)
        got = LRR.round_by_classes(h.n, P, K, tables)
        assert (got == seq).all()
        want, want_sweeps = CR.descent(h.n, h.rowptr, h.col, h.weight, seq, K, 100)
        a, s = LRR.descent(h.n, got, K, tables, 100)
        assert (a == want).all() and s == want_sweeps


def test_python_refusals(built):
    from gcn_max_cut_amd.Testing import TestingNeuralNetwork as TN
    g = R.regular_graph(20, 3, 1)
    for K in (1, 9):
        with pytest.raises(ValueError, match="number_classes"):
            TN.large_conditional_rounding(np.full((20, K), 1.0 / K, np.float32), g)
        with pytest.raises(ValueError, match="number_classes"):
            TN.large_local_search([0] * 20, g, K)
    with pytest.raises(ValueError, match="at least 5 nodes"):
        TN.large_conditional_rounding(np.full((4, 5), 0.2, np.float32), nx.complete_graph(4))
    with pytest.raises(ValueError, match="at least 5 nodes"):
        TN.large_local_search([0, 1, 2, 3], nx.complete_graph(4), 5)
    with pytest.raises(ValueError, match="descent_sweeps"):
        TN.large_conditional_rounding(np.full((20, 3), 1.0 / 3, np.float32), g, descent_sweeps=-1)
    with pytest.raises(ValueError, match="max_sweeps"):
        TN.large_local_search([0, 1, 2] + [0] * 17, g, 3, max_sweeps=-1)
    with pytest.raises(ValueError, match="rows"):
        TN.large_conditional_rounding(np.full((19, 3), 1.0 / 3, np.float32), g)
    with pytest.raises(ValueError, match="entries"):
        TN.large_local_search([0] * 19, g, 3)
    with pytest.raises(ValueError, match="class outside"):
        TN.large_local_search([0, 1, 2] + [3] * 17, g, 3)
    with pytest.raises(ValueError, match="descent_sweeps"):
        TN.round_large_dataset(None, {}, descent_sweeps=-1)
    # the decoders that stay at 4096 nodes name the new functions after their old wording
    with pytest.raises(ValueError, match="4096 nodes.*argmax partition.*large_conditional_rounding"):
        TN._decoder_graph_size("round_dataset", 4097)
    built.install_compat()                                             # the reference's import roots mirror the module
    import Testing.TestingNeuralNetwork as mirror
    assert mirror.round_large_dataset is TN.round_large_dataset
    assert mirror.large_conditional_rounding is TN.large_conditional_rounding
    assert mirror.large_local_search is TN.large_local_search
